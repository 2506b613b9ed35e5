// Device UTF-8 validation of text messages for MI355X (gfx950): kmws_utf8_validate.
//
// RFC 6455 5.6 / 8.1: the payload of a text message is well-formed UTF-8, and
// an endpoint that receives anything else fails the connection (1007).  kuma
// hands text payloads to the application unchecked (onWsFrame,
// WebSocketImpl.cpp:268-301); this entry is opt-in and changes nothing else.
//
// A batch is many frames of many streams; messages are fragmented, a code point
// may straddle fragments, control frames interleave, and a message may begin in
// one batch and end in the next.  Five kernels after the unmask plan
// (launch_plan: descriptor checks and the tile -> frame records):
//   1. utf8_elem_kernel: lane i turns frame i into a scan element (Utf8Elem,
//      kmws_utf8_rule.hpp: what the frame does to its stream's message state,
//      with its own last <= 3 payload bytes), folds the stream's carry into a
//      stream's first frame, seeds first_bad[i], and reduces its block;
//   2. utf8_scan_aggs_kernel: one block scans the block aggregates;
//   3. utf8_ctx_kernel: lane i gets the state before frame i, stores how the
//      frame sees itself (checked?, slot, look-back at its first byte), applies
//      rule (b) -- a FIN frame that ends inside a code point, which an empty
//      frame can do -- and keeps the state after each stream's last frame;
//   4. utf8_payload_kernel: one block per 16 KiB tile, 256 lanes x 4 x 16-byte
//      `nt` buffer loads issued before the first use; each word takes the three
//      bytes before it from the neighbour lane's word (lane 0 of a wave from a
//      4-byte load), or from the scan at a frame start.  An all-ASCII word after
//      an ASCII byte is one OR and a test; any other word inside a frame runs the
//      rule four bytes per operation (utf8_word_bad_swar); a word with a frame edge
//      walks its bytes.  The first frame at which a message breaks goes to
//      first_bad[slot] by atomicMin;
//   5. utf8_finish_kernel: out[i] from first_bad[slot]; carry_out per stream.
// Nothing is stored to the payload.  Algorithmic bytes: the checked payload
// read once + ~32 B per frame (descriptor, flags, element, verdict).
#include "kmws_common.hpp"
#include "kmws_utf8_rule.hpp"

namespace kmws {

constexpr uint32_t kUtf8None = 0xFFFFFFFFu;  // first_bad: holds frame + 1 of the BAD frame, 0 = before this batch
constexpr uint32_t kStatusBadStreams = kStatusBadDesc;  // a malformed stream_first: the same caller error bit

// ---- workspace: the unmask plan's, then the per-frame and per-stream arrays ----
struct Utf8Ws {
    size_t plan_bytes;  // WsHead + tile records
    size_t first_bad, elems, aggs, pre, carry, total;
    uint32_t nblk;  // scan blocks of kBlock frames
};
static size_t r16(size_t x) { return (x + 15) & ~(size_t)15; }
static Utf8Ws utf8_ws(uint64_t span, uint32_t n, uint32_t n_streams)
{
    Utf8Ws w;
    w.nblk = (n + kBlock - 1) / kBlock;
    w.plan_bytes = kmws_unmask_workspace_size(span);
    w.first_bad = r16(w.plan_bytes);
    w.elems = w.first_bad + r16((size_t)n * 4);
    w.aggs = w.elems + r16((size_t)n * 8);
    w.pre = w.aggs + r16((size_t)w.nblk * 8);
    w.carry = w.pre + r16((size_t)w.nblk * 8);
    w.total = w.carry + r16((size_t)n_streams * 8);
    return w;
}

// Inclusive scan of one element per lane over the block (Hillis-Steele in LDS);
// s[] holds the inclusive values on return.
__device__ __forceinline__ Utf8Elem block_scan(Utf8Elem e, Utf8Elem* s)
{
    const int tid = threadIdx.x;
    s[tid] = e;
    __syncthreads();
#pragma unroll
    for (int dlt = 1; dlt < kBlock; dlt <<= 1) {
        const Utf8Elem t = tid >= dlt ? utf8_combine(s[tid - dlt], s[tid]) : s[tid];
        __syncthreads();
        s[tid] = t;
        __syncthreads();
    }
    return s[tid];
}

// The stream of frame i: the last s in [0, ns) with first[s] <= i (empty streams
// before it share its start and lose).  Every index stays in range whatever the
// array holds.  first == nullptr: one stream.
__device__ __forceinline__ uint32_t stream_of(const uint32_t* __restrict__ first, uint32_t ns, uint32_t i)
{
    if (!first) return 0u;
    uint32_t lo = 0, hi = ns - 1;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo + 1) / 2;
        if (first[mid] <= i) lo = mid; else hi = mid - 1;
    }
    return lo;
}
__device__ __forceinline__ uint32_t stream_begin(const uint32_t* __restrict__ first, uint32_t s)
{
    return first ? first[s] : 0u;
}
__device__ __forceinline__ uint32_t stream_end(const uint32_t* __restrict__ first, uint32_t n, uint32_t s)
{
    return first ? first[s + 1] : n;
}

// kmws_utf8_carry has byte alignment: read and written byte by byte.
__device__ __forceinline__ uint64_t load_carry(const kmws_utf8_carry* __restrict__ c, uint32_t s)
{
    uint64_t x = 0;
    if (c)
        for (int k = 0; k < 8; ++k) x |= (uint64_t)c[s].b[k] << (8 * k);
    return x;
}
__device__ __forceinline__ void store_carry(kmws_utf8_carry* __restrict__ c, uint32_t s, uint64_t x)
{
    for (int k = 0; k < 8; ++k) c[s].b[k] = (uint8_t)(x >> (8 * k));
}

__global__ void __launch_bounds__(kBlock) utf8_elem_kernel(const uint8_t* __restrict__ base, uint64_t span,
                                                           const kmws_desc* __restrict__ d,
                                                           const uint16_t* __restrict__ flags, uint32_t n, int masked,
                                                           const uint32_t* __restrict__ first, uint32_t ns,
                                                           const kmws_utf8_carry* __restrict__ carry_in,
                                                           Utf8Elem* __restrict__ elems, uint32_t* __restrict__ first_bad,
                                                           Utf8Elem* __restrict__ aggs, uint32_t nblk,
                                                           WsHead* __restrict__ head)
{
    __shared__ Utf8Elem s_scan[kBlock];
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (first && i <= ns) {  // stream_first: [0] == 0, ascending, [ns] == n
        const uint32_t x = first[i];
        if ((i == 0 && x != 0u) || (i == ns && x != n) || (i < ns && x > first[i + 1]))
            atomicOr(&head->status, kStatusBadStreams);
    }
    Utf8Elem e = utf8_identity();
    if (i < n) {
        const kmws_desc df = d[i];
        const uint32_t ob = flags[i] & 0xFFu, op = ob & 0x0Fu;
        uint32_t nb = 0, tail = 0;
        if (df.off > span || df.off + (uint64_t)df.len > span) {
            atomicOr(&head->status, kStatusBadDesc);  // never read outside the span
        } else if (op < 8u) {
            nb = df.len < 3u ? df.len : 3u;
            for (uint32_t k = 0; k < nb; ++k) {
                const uint32_t j = df.len - nb + k;
                uint32_t b = base[df.off + j];
                if (masked) b ^= (df.key >> (8u * (j & 3u))) & 0xFFu;
                tail = (tail << 8) | b;
            }
        }
        e = utf8_frame_elem(ob, i, tail, nb);
        uint32_t fb = kUtf8None;
        const uint32_t s = stream_of(first, ns, i);
        if (stream_begin(first, s) == i) {
            bool bad = false;
            const Utf8Elem st = utf8_carry_unpack(load_carry(carry_in, s), i, &bad);
            e = utf8_combine(st, e);
            // a carried message already BAD: its slot is this frame -- unless this
            // frame heads a new message, which replaces it and owns the slot
            if (bad && (op == 0u || op >= 8u)) fb = 0u;
        }
        elems[i] = e;
        first_bad[i] = fb;
    }
    const Utf8Elem inc = block_scan(e, s_scan);
    if (threadIdx.x == kBlock - 1 && blockIdx.x < nblk) aggs[blockIdx.x] = inc;
}

// pre[b] = the combination of aggs[0 .. b): one block, kBlock aggregates a round.
__global__ void __launch_bounds__(kBlock) utf8_scan_aggs_kernel(const Utf8Elem* __restrict__ aggs,
                                                                Utf8Elem* __restrict__ pre, uint32_t nblk)
{
    __shared__ Utf8Elem s_scan[kBlock];
    Utf8Elem run = utf8_identity();
    for (uint32_t c0 = 0; c0 < nblk; c0 += kBlock) {
        const uint32_t b = c0 + threadIdx.x;
        const Utf8Elem e = b < nblk ? aggs[b] : utf8_identity();
        block_scan(e, s_scan);
        const Utf8Elem ex = threadIdx.x ? s_scan[threadIdx.x - 1] : utf8_identity();
        if (b < nblk) pre[b] = utf8_combine(run, ex);
        run = utf8_combine(run, s_scan[kBlock - 1]);
        __syncthreads();  // the next round rewrites s_scan
    }
}

// The state before and after every frame.  Overwrites elems[i] with frame i's
// view of itself (Utf8View: the payload pass and the finish read it).
__global__ void __launch_bounds__(kBlock) utf8_ctx_kernel(const uint16_t* __restrict__ flags, uint32_t n,
                                                          const uint32_t* __restrict__ first, uint32_t ns,
                                                          const kmws_utf8_carry* __restrict__ carry_in,
                                                          Utf8Elem* __restrict__ elems, const Utf8Elem* __restrict__ pre,
                                                          uint32_t* __restrict__ first_bad,
                                                          Utf8Elem* __restrict__ carry_tmp)
{
    __shared__ Utf8Elem s_scan[kBlock];
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    const Utf8Elem e = i < n ? elems[i] : utf8_identity();
    block_scan(e, s_scan);
    if (i >= n) return;
    Utf8Elem before = utf8_combine(pre[blockIdx.x], threadIdx.x ? s_scan[threadIdx.x - 1] : utf8_identity());
    const Utf8Elem after = utf8_combine(before, e);
    const uint32_t s = stream_of(first, ns, i);
    if (stream_begin(first, s) == i) {  // the scan's element already holds the carry: unfold it for the view
        bool bad = false;
        before = utf8_carry_unpack(load_carry(carry_in, s), i, &bad);
    }
    const uint32_t ob = flags[i] & 0xFFu;
    const Utf8View v = utf8_frame_view(before, ob, i);
    elems[i] = Utf8Elem{v.slot, v.w};
    // rule (b): a checked message that ends (FIN) inside a code point.  A closing
    // frame's element is its own tail (utf8_frame_elem), also under a carry.
    if ((v.w & kUtf8Checked) && (ob & 0x80u)) {
        const uint32_t nb = utf8_elem_nb(e);
        const uint32_t L = nb >= 3u ? utf8_elem_ctx(e) : (((v.w << (8u * nb)) | utf8_elem_ctx(e)) & 0xFFFFFFu);
        if (utf8_pending(L)) atomicMin(&first_bad[v.slot], i + 1u);
    }
    if (i + 1u == stream_end(first, n, s)) carry_tmp[s] = after;
}

// Byte r (-4 .. 15) of the window: the dword before the word, then the word.
__device__ __forceinline__ uint32_t window_byte(uint32_t prev, const u32x4& w, int r)
{
    const uint32_t dw = r < 0 ? prev : (r < 4 ? w.x : (r < 8 ? w.y : (r < 12 ? w.z : w.w)));
    return (dw >> (8u * ((uint32_t)r & 3u))) & 0xFFu;
}

// The bytes of the 16-byte word at address a (w; prev = the dword before it,
// both unmasked) that belong to the frame [off, end), whose look-back at its
// first byte is ctx: does the byte rule reject one of them?  The look-back of
// the word's first byte is the three bytes before it where the frame has them,
// else ctx and the frame's bytes up to it.
__device__ __forceinline__ bool word_bad(uint32_t prev, const u32x4& w, uint64_t a, uint64_t off, uint64_t end,
                                         uint32_t ctx)
{
    const bool deep = off + 3u <= a;
    // the word and its look-back lie inside the frame: four bytes per operation
    if (deep && end >= a + 16u) return utf8_word_bad_swar(prev, w.x, w.y, w.z, w.w);
    // a frame edge in or just before the word (rare): a rolled loop, compact code
    const int s = deep ? -3 : (int)((int64_t)off - (int64_t)a);  // > -3
    const int e = end >= a + 16u ? 16 : (int)(end - a);
    uint32_t L = deep ? 0u : (ctx & 0xFFFFFFu);
    bool bad = false;
#pragma unroll 1
    for (int r = s; r < e; ++r) {
        const uint32_t b = window_byte(prev, w, r);
        if (r >= 0) bad |= utf8_byte_bad(b, L);
        L = utf8_append(L, b);
    }
    return bad;
}

constexpr int kUtf8V = (int)(kPlanTile / 16 / kBlock);  // 16-byte words per lane
constexpr int kUtf8PolLoad = 2;                          // `nt`: the payload is read once
constexpr int kUtf8RsrcWord3 = 0x00020000;

__device__ __forceinline__ void report_bad(uint32_t* __restrict__ first_bad, uint32_t slot, uint32_t frame)
{
    // verdict words only fall: a stale read costs one atomic more, never a verdict
    if (__builtin_nontemporal_load(&first_bad[slot]) > frame + 1u) atomicMin(&first_bad[slot], frame + 1u);
}

// Waves per SIMD asked of the register allocator: the read-only stream runs
// faster with more blocks in flight (all-ASCII 4 GiB: 0.84 ms at 8 waves, 1.17 ms
// at 5), and the word form's class masks are what costs registers.  7 fits the
// plain kernel without scratch; the masked one (the rotated keys on top) fits 4.
template <bool MASKED>
__global__ void __launch_bounds__(kBlock, MASKED ? 4 : 7) utf8_payload_kernel(const uint8_t* __restrict__ base, uint64_t span,
                                                              const kmws_desc* __restrict__ d, uint32_t n,
                                                              const TileRec* __restrict__ map,
                                                              const WsHead* __restrict__ head,
                                                              const Utf8View* __restrict__ views,
                                                              uint32_t* __restrict__ first_bad, TileMapping tm,
                                                              uint32_t b0)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t tile = tile_of_block(b0 + blockIdx.x, tm);
    const uint64_t lo = (uint64_t)tile * kPlanTile;
    const uint64_t hi = lo + kPlanTile < span ? lo + kPlanTile : span;
    const TileRecPair recs = *reinterpret_cast<const TileRecPair*>(map + tile);
    if (head->status != 0u) return;  // a bad plan: the records mean nothing
    const bool cov = tile_rec_covered(recs.at, n);
    const uint32_t f = tile_rec_frame(recs.at, n);
    uint32_t fl = tile_rec_frame(recs.next, n);
    if (f >= n) return;
    if (fl >= n) fl = n - 1;
    if (fl < f) fl = f;

    // Tiles of unchecked frames (binary, compressed, control) leave before loading.
    Utf8View fv = Utf8View{0u, 0u};
    kmws_desc d0 = kmws_desc{0ull, 0u, 0u};
    if (cov) {
        fv = views[f];
        if (!(fv.w & kUtf8Checked)) return;
        d0 = d[f];
    } else {
        bool any = false;
        for (uint32_t g = f + (uint32_t)tid; g <= fl; g += kBlock) any |= (views[g].w & kUtf8Checked) != 0u;
        if (!__syncthreads_or(any)) return;
    }

    // every payload load of the tile, then the four words' look-back of each
    // wave's lane 0 (lanes 0-3 load the dword before word i = lane of lane 0)
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<uint8_t*>(base) + lo, (short)0, (int)((hi - lo + 15) & ~15ull), kUtf8RsrcWord3);
    u32x4 v[kUtf8V];
#pragma unroll
    for (int i = 0; i < kUtf8V; ++i) {
        const uint32_t x = 16u * (uint32_t)(tid + kBlock * i);
        if (lo + x < hi) v[i] = __builtin_amdgcn_raw_buffer_load_b128(rs, (int)x, 0, kUtf8PolLoad);
        else v[i] = u32x4{0, 0, 0, 0};
    }
    uint32_t edge = 0;
    if (lane < kUtf8V) {
        const uint64_t ae = lo + 16u * (uint64_t)(64 * wave + kBlock * lane);
        if (ae >= 4u && ae <= span) edge = *reinterpret_cast<const uint32_t*>(base + ae - 4);
    }
    uint32_t prev[kUtf8V];
#pragma unroll
    for (int i = 0; i < kUtf8V; ++i) {
        const uint32_t up = __shfl_up(v[i].w, 1);
        const uint32_t ed = __shfl(edge, i);
        prev[i] = lane == 0 ? ed : up;
    }

    if (cov) {
        // One frame covers the tile (block-uniform): a word of ASCII bytes after
        // an ASCII byte is decided by one OR and a test.
        const uint32_t r = MASKED ? recs.at.rkey : 0u;
        const uint64_t end = d0.off + d0.len;
        bool slow[kUtf8V];
        bool any = false;
#pragma unroll
        for (int i = 0; i < kUtf8V; ++i) {
            const uint64_t a = lo + 16u * (uint64_t)(tid + kBlock * i);
            const u32x4 w = v[i] ^ r;
            const uint32_t hb = (w.x | w.y | w.z | w.w) & 0x80808080u;
            slow[i] = hb != 0u || ((prev[i] ^ r) & 0x80000000u) != 0u || a < d0.off + 3u;
            any |= slow[i];
        }
        bool bad = false;
        if (__any(any)) {
#pragma unroll
            for (int i = 0; i < kUtf8V; ++i) {
                const uint64_t a = lo + 16u * (uint64_t)(tid + kBlock * i);
                if (slow[i]) bad |= word_bad(prev[i] ^ r, v[i] ^ r, a, d0.off, end, fv.w);
            }
        }
        const unsigned long long m = __ballot(bad);  // one report per wave
        if (m != 0ull && lane == __ffsll((long long)m) - 1) report_bad(first_bad, fv.slot, f);
        return;
    }

    // Several frames (or a frame edge) in the tile: each word finds its frames
    // in the sorted descriptors [f, fl].
#pragma unroll
    for (int i = 0; i < kUtf8V; ++i) {
        const uint64_t a = lo + 16u * (uint64_t)(tid + kBlock * i);
        if (a >= hi) continue;
        uint32_t gl = f, gh = fl + 1u;  // the first frame that ends after a
        while (gl < gh) {
            const uint32_t mid = gl + (gh - gl) / 2;
            const kmws_desc dm = d[mid];
            if (dm.off + dm.len <= a) gl = mid + 1; else gh = mid;
        }
        for (uint32_t g = gl; g <= fl; ++g) {
            const kmws_desc dg = d[g];
            if (dg.off >= a + 16u) break;
            if (dg.len == 0u) continue;
            const Utf8View gv = views[g];
            if (!(gv.w & kUtf8Checked)) continue;
            const uint32_t r = MASKED ? rot_key(dg.key, dg.off) : 0u;
            const uint64_t end = dg.off + dg.len;
            const u32x4 w = v[i] ^ r;
            const bool plain = dg.off + 3u <= a && end >= a + 16u && ((w.x | w.y | w.z | w.w) & 0x80808080u) == 0u &&
                               ((prev[i] ^ r) & 0x80000000u) == 0u;
            if (!plain && word_bad(prev[i] ^ r, w, a, dg.off, end, gv.w)) report_bad(first_bad, gv.slot, g);
        }
    }
}

__global__ void __launch_bounds__(kBlock) utf8_finish_kernel(uint32_t n, const uint32_t* __restrict__ first,
                                                             uint32_t ns, const Utf8View* __restrict__ views,
                                                             const uint32_t* __restrict__ first_bad,
                                                             const Utf8Elem* __restrict__ carry_tmp,
                                                             const kmws_utf8_carry* __restrict__ carry_in,
                                                             kmws_utf8_carry* __restrict__ carry_out,
                                                             uint8_t* __restrict__ out)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i < n) {
        const Utf8View v = views[i];
        uint8_t r = KMWS_UTF8_NOT_TEXT;
        if (v.w & kUtf8Checked) {
            const uint32_t fb = first_bad[v.slot];
            r = fb > i + 1u ? KMWS_UTF8_OK : (fb == i + 1u ? KMWS_UTF8_BAD : KMWS_UTF8_AFTER_BAD);
        }
        out[i] = r;
    }
    if (carry_out && i < ns) {
        const uint32_t s = i;
        uint64_t c;
        if (stream_begin(first, s) >= stream_end(first, n, s)) {
            c = load_carry(carry_in, s);  // an empty stream
        } else {
            const Utf8Elem after = carry_tmp[s];
            const bool chk = (after.w & (kUtf8Open | kUtf8Checked)) == (kUtf8Open | kUtf8Checked);
            c = utf8_carry_pack(after, chk && after.slot < n && first_bad[after.slot] != kUtf8None);
        }
        store_carry(carry_out, s, c);
    }
}

__global__ void __launch_bounds__(kBlock) utf8_carry_copy_kernel(uint32_t ns,
                                                                 const kmws_utf8_carry* __restrict__ carry_in,
                                                                 kmws_utf8_carry* __restrict__ carry_out)
{
    const uint32_t s = blockIdx.x * kBlock + threadIdx.x;
    if (s < ns) store_carry(carry_out, s, load_carry(carry_in, s));
}

static bool have_device()
{
    static const bool have = kmws_device_count() > 0;
    return have;
}

}  // namespace kmws

using namespace kmws;

extern "C" {

size_t kmws_utf8_workspace_size(uint64_t span, uint32_t n, uint32_t n_streams)
{
    return utf8_ws(span, n, n_streams).total;
}

kmws_status kmws_utf8_validate(const uint8_t* base, uint64_t span, const kmws_desc* descs, const uint16_t* flags,
                               uint32_t n, int payload_masked, const uint32_t* stream_first, uint32_t n_streams,
                               const kmws_utf8_carry* carry_in, kmws_utf8_carry* carry_out, uint8_t* out,
                               void* workspace, size_t workspace_bytes, void* stream)
{
    if (n >= 0x80000000u || n_streams >= 0x80000000u) return KMWS_ERR_INVALID_PARAM;
    if (n && (!base || !descs || !flags || !out || !workspace)) return KMWS_ERR_INVALID_PARAM;
    if (reinterpret_cast<uintptr_t>(base) & 15u) return KMWS_ERR_INVALID_PARAM;
    if (n && (n_streams == 0u || (!stream_first && n_streams != 1u))) return KMWS_ERR_INVALID_PARAM;
    const Utf8Ws w = utf8_ws(span, n, n_streams);
    if (n && workspace_bytes < w.total) return KMWS_ERR_BUFFER_TOO_SMALL;
    if (!have_device()) return KMWS_ERR_NOT_SUPPORTED;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (n == 0) {  // nothing to judge: every stream's state passes through
        if (carry_out && n_streams)
            hipLaunchKernelGGL(utf8_carry_copy_kernel, dim3((n_streams + kBlock - 1) / kBlock), dim3(kBlock), 0, s,
                               n_streams, carry_in, carry_out);
        return hip_status(hipGetLastError());
    }
    kmws_status st = launch_plan(span, descs, n, workspace, w.plan_bytes, s);
    if (st != KMWS_OK) return st;
    note_device_batch(span, s);

    uint8_t* wsb = static_cast<uint8_t*>(workspace);
    WsHead* head = static_cast<WsHead*>(workspace);
    const TileRec* map = reinterpret_cast<const TileRec*>(head + 1);
    uint32_t* first_bad = reinterpret_cast<uint32_t*>(wsb + w.first_bad);
    Utf8Elem* elems = reinterpret_cast<Utf8Elem*>(wsb + w.elems);
    Utf8Elem* aggs = reinterpret_cast<Utf8Elem*>(wsb + w.aggs);
    Utf8Elem* pre = reinterpret_cast<Utf8Elem*>(wsb + w.pre);
    Utf8Elem* carry_tmp = reinterpret_cast<Utf8Elem*>(wsb + w.carry);
    const Utf8View* views = reinterpret_cast<const Utf8View*>(elems);
    const uint32_t sblk = stream_first ? (n_streams + 1u + kBlock - 1) / kBlock : 0u;
    const int masked = payload_masked != 0;

    hipLaunchKernelGGL(utf8_elem_kernel, dim3(w.nblk > sblk ? w.nblk : sblk), dim3(kBlock), 0, s, base, span, descs,
                       flags, n, masked, stream_first, n_streams, carry_in, elems, first_bad, aggs, w.nblk, head);
    hipLaunchKernelGGL(utf8_scan_aggs_kernel, dim3(1), dim3(kBlock), 0, s, aggs, pre, w.nblk);
    hipLaunchKernelGGL(utf8_ctx_kernel, dim3(w.nblk), dim3(kBlock), 0, s, flags, n, stream_first, n_streams, carry_in,
                       elems, pre, first_bad, carry_tmp);

    const uint64_t ntiles = (span + kPlanTile - 1) / kPlanTile;  // launch_plan bounded it
    Split sp;
    (void)split_of(KMWS_SCHED_SPLIT4, &sp);
    const TileMapping tm = tile_mapping((uint32_t)(span / kPlanTile), sp);  // the partial last tile maps to itself
    constexpr uint64_t kMaxBlocks = (1ull << 32) / kBlock / 2;
    for (uint64_t b0 = 0; b0 < ntiles; b0 += kMaxBlocks) {
        const dim3 grid((uint32_t)(ntiles - b0 < kMaxBlocks ? ntiles - b0 : kMaxBlocks));
        if (masked)
            hipLaunchKernelGGL(utf8_payload_kernel<true>, grid, dim3(kBlock), 0, s, base, span, descs, n, map, head,
                               views, first_bad, tm, (uint32_t)b0);
        else
            hipLaunchKernelGGL(utf8_payload_kernel<false>, grid, dim3(kBlock), 0, s, base, span, descs, n, map, head,
                               views, first_bad, tm, (uint32_t)b0);
    }
    const uint32_t fin_lanes = carry_out && n_streams > n ? n_streams : n;
    hipLaunchKernelGGL(utf8_finish_kernel, dim3((fin_lanes + kBlock - 1) / kBlock), dim3(kBlock), 0, s, n,
                       stream_first, n_streams, views, first_bad, carry_tmp, carry_in, carry_out, out);
    return hip_status(hipGetLastError());
}

}  // extern "C"
