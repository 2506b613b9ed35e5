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
// (launch_plan: descriptor checks and the tile -> frame records); the first
// three are the scan core of kmws_stream_scan.hpp with Utf8Op, one frame a lane:
//   1. utf8_elem_kernel: lane i turns frame i into a scan element (Utf8Elem,
//      kmws_utf8_rule.hpp: what the frame does to its stream's message state,
//      with its own last <= 3 payload bytes), folds the stream's carry into a
//      stream's first frame, seeds first_bad[i], and reduces its block;
//   2. utf8_scan_aggs_kernel: scan_aggregates over the block aggregates;
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
// kmws_unmask_utf8_batch / kmws_unpack_unmask_utf8 (below, "the fused in-place
// pass") run kernels 1-3 and 5 as they are around a payload pass that also
// unmasks in place.  kmws_gather_unmask_utf8 / kmws_unpack_gather_utf8
// (kmws_pack.hip) run them around the gather's copy grid, through the host
// launchers declared in kmws_utf8_dev.hpp; kmws_reframe_utf8_batch /
// kmws_unpack_reframe_utf8 around the reframe's, with skip_flag naming the
// frames that pass leaves out (control frames to kernels 1 and 3).
#include "kmws_common.hpp"
#include "kmws_stream_scan.hpp"
#include "kmws_unmask_tile.hpp"
#include "kmws_utf8_dev.hpp"
#include "kmws_utf8_rule.hpp"
#include "kmws_workspace.hpp"

namespace kmws {

constexpr uint32_t kStatusBadStreams = kStatusBadDesc;  // a malformed stream_first: the same caller error bit

// The workspaces (utf8_ws, fused_ws) are laid out in kmws_workspace.hpp.
static_assert(sizeof(Utf8Elem) == kWsUtf8ElemBytes && sizeof(Utf8View) == sizeof(Utf8Elem),
              "the layout's element size; the views replace the elements in place");

struct Utf8Op {  // two dwords, moved one by one
    using T = Utf8Elem;
    static __device__ __forceinline__ T identity() { return utf8_identity(); }
    static __device__ __forceinline__ T compose(T a, T b) { return utf8_combine(a, b); }
    static __device__ __forceinline__ T shfl_up(T v, int dlt) { return T{__shfl_up(v.slot, dlt), __shfl_up(v.w, dlt)}; }
    static __device__ __forceinline__ T load(const T* p) { return T{p->slot, p->w}; }
    static __device__ __forceinline__ void store(T* p, T v) { p->slot = v.slot, p->w = v.w; }
};

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
                                                           uint32_t skip_flag,
                                                           const uint32_t* __restrict__ first, uint32_t ns,
                                                           const kmws_utf8_carry* __restrict__ carry_in,
                                                           Utf8Elem* __restrict__ elems, uint32_t* __restrict__ first_bad,
                                                           Utf8Elem* __restrict__ aggs, uint32_t nblk,
                                                           WsHead* __restrict__ head)
{
    __shared__ Utf8Elem s_wave[kScanWaves];
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (stream_first_bad(first, ns, n, i)) atomicOr(&head->status, kStatusBadStreams);
    Utf8Elem e = utf8_identity();
    if (i < n) {
        const kmws_desc df = d[i];
        const uint32_t ob = utf8_op_byte(flags[i], skip_flag), op = ob & 0x0Fu;
        uint32_t nb = 0, tail = 0;
        if (flags[i] & skip_flag) {
            // skipped by the pass: a control frame whose descriptor may point anywhere
        } else if (df.off > span || df.off + (uint64_t)df.len > span) {
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
    Utf8Elem total;
    block_scan_excl<Utf8Op>(e, s_wave, &total);
    if (threadIdx.x == 0 && blockIdx.x < nblk) aggs[blockIdx.x] = total;
}

// pre[b] = the combination of aggs[0 .. b).
__global__ void __launch_bounds__(kBlock) utf8_scan_aggs_kernel(const Utf8Elem* __restrict__ aggs,
                                                                Utf8Elem* __restrict__ pre, uint32_t nblk)
{
    __shared__ Utf8Elem s_wave[kScanWaves];
    scan_aggregates<Utf8Op>(nblk, s_wave, [&](uint32_t b) { return b < nblk ? aggs[b] : utf8_identity(); },
                            [&](uint32_t b, Utf8Elem p) { pre[b] = p; });
}

// The state before and after every frame.  Overwrites elems[i] with frame i's
// view of itself (Utf8View: the payload pass and the finish read it).
__global__ void __launch_bounds__(kBlock) utf8_ctx_kernel(const uint16_t* __restrict__ flags, uint32_t n,
                                                          uint32_t skip_flag,
                                                          const uint32_t* __restrict__ first, uint32_t ns,
                                                          const kmws_utf8_carry* __restrict__ carry_in,
                                                          Utf8Elem* __restrict__ elems, const Utf8Elem* __restrict__ pre,
                                                          uint32_t* __restrict__ first_bad,
                                                          Utf8Elem* __restrict__ carry_tmp)
{
    __shared__ Utf8Elem s_wave[kScanWaves];
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    const Utf8Elem e = i < n ? elems[i] : utf8_identity();
    Utf8Elem total;
    const Utf8Elem excl = block_scan_excl<Utf8Op>(e, s_wave, &total);
    if (i >= n) return;
    Utf8Elem before = utf8_combine(pre[blockIdx.x], excl);
    const Utf8Elem after = utf8_combine(before, e);
    const uint32_t s = stream_of(first, ns, i);
    if (stream_begin(first, s) == i) {  // the scan's element already holds the carry: unfold it for the view
        bool bad = false;
        before = utf8_carry_unpack(load_carry(carry_in, s), i, &bad);
    }
    const uint32_t ob = utf8_op_byte(flags[i], skip_flag);
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

constexpr int kUtf8V = (int)(kPlanTile / 16 / kBlock);  // 16-byte words per lane
constexpr int kUtf8PolLoad = 2;                          // `nt`: the payload is read once
constexpr int kUtf8RsrcWord3 = 0x00020000;

// ---- the checks of a loaded tile: the validator's and the fused pass's ----
// v[i]: the lane's word at lo + 16 (tid + kBlock i), prev[i]: the dword before
// it, both as they lie in memory.
//
// One frame f (d0, view fv, rotated key r; 0: a plain payload) covers the tile,
// block-uniform: a word of ASCII bytes after an ASCII byte is decided by one OR
// and a test, and a wave that holds no other word skips the rule.
__device__ __forceinline__ void covered_tile_check(const u32x4 (&v)[kUtf8V], const uint32_t (&prev)[kUtf8V],
                                                   uint32_t r, uint64_t lo, const kmws_desc& d0, Utf8View fv,
                                                   uint32_t f, uint32_t* __restrict__ first_bad)
{
    const int tid = threadIdx.x, lane = tid & 63;
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
}

// Several frames (or a frame edge) in the tile: each of the lane's words below
// hi finds its frames in the sorted descriptors [f, fl] and is checked against
// every checked one.  MASKED: the payload is still masked with the frames' keys.
template <bool MASKED>
__device__ __forceinline__ void frames_check(const u32x4 (&v)[kUtf8V], const uint32_t (&prev)[kUtf8V], uint64_t lo,
                                             uint64_t hi, const kmws_desc* __restrict__ d, uint32_t f, uint32_t fl,
                                             const Utf8View* __restrict__ views, uint32_t* __restrict__ first_bad)
{
    const int tid = threadIdx.x;
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
            if (plain_word_frame_bad(v[i] ^ r, prev[i] ^ r, a, dg.off, dg.off + dg.len, gv.w))
                report_bad(first_bad, gv.slot, g);
        }
    }
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
        covered_tile_check(v, prev, MASKED ? recs.at.rkey : 0u, lo, d0, fv, f, first_bad);
        return;
    }

    // Several frames (or a frame edge) in the tile.
    frames_check<MASKED>(v, prev, lo, hi, d, f, fl, views, first_bad);
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

// ---- the fused in-place pass: kmws_unmask_utf8_batch / kmws_unpack_unmask_utf8 ----
//
// One kernel family does what unmask_split_kernel / unmask_tail_kernel
// (kmws_unmask.hip) and utf8_payload_kernel<true> do in two trips over the
// payload: the tile is loaded once, every word's mask is built by the apply's
// three paths (the record's rotated key of a covered tile; two block-uniform
// descriptors in the capped launches; descriptors staged in LDS), the unmasked
// words are stored with the apply's store policy, and the words of checked
// frames are validated from the registers that hold them.  On the one- and
// two-frame paths the stores go first: nothing of the rule stands between a
// word's arrival and its store, and a tile of unchecked frames (binary, RSV1,
// control) ends after them on a block-uniform test of its frames' views -- the
// plain unmask and a scalar load that arrives under the payload.  What follows
// the stores touches registers, LDS and scalars only, and the stores are
// straight-line code (kFusedNoStore): a wait on the vector memory counter there
// would wait for the stores' write-through as well.  The LDS-staged path loads
// descriptors and views to validate, so it validates first and stores last.
//
// The look-back of a word's first byte is the dword before it.  Inside a wave
// that is the neighbour lane's register.  For lane 0 of a wave, the validator
// alone may read it from memory; here that dword belongs to another wave or to
// another block's tile, which may or may not have stored it unmasked already.
// So no look-back is read from the payload while this kernel runs:
//   - the dword before each tile comes from utf8_edges_kernel, which saves it,
//     still masked, ahead of this kernel in stream order (4 B per tile);
//   - the dword before each of a tile's other fifteen 1 KiB rows is the last
//     register of lane 63 of the wave that loaded the row before: handed over
//     in LDS behind one barrier, which stands after the stores and is reached
//     only by tiles that hold a checked frame.  (The other form, a pre-pass
//     that saves all sixteen dwords of a tile and a kernel with no barrier, was
//     built and timed and lost on every kind of payload: each of those dwords
//     costs the pre-pass a memory request of its own.  DESIGN 4 has the times.)
// A saved dword is XORed with the frame's rotated key like the words (the dword
// before a 16-byte word has the word's key phase) and is used only where the
// frame reaches three bytes back, as word_bad has it.
constexpr int kFusedRows = (int)(kPlanTile / 1024);  // a wave-instruction loads 1 KiB: row = wave + 4 * i
// A store that must not happen takes this offset, past every tile's resource,
// and is dropped by the buffer's range check: the stores stay straight-line
// code, so the compiler keeps track of which loads have arrived (fused_tile).
constexpr uint32_t kFusedNoStore = 0x7FFFFFF0u;
static_assert(kUtf8V == kUnmaskV && kFusedRows == 4 * kUtf8V, "the validator's tile is the apply's");

// Blocks of a capped launch per CU.  The apply streams best with 2 (its stores
// follow its loads at once); here a block goes on to validate after its stores,
// and with 2 blocks per CU nothing covers that time: the 4 GiB ASCII batch ran
// 2.64 ms at 2, 1.86 ms at 3 and 1.47 ms at 4 blocks per CU (mixed text 3.39 /
// 2.42 / 1.99 ms), the same bytes marked binary 1.29 / 1.36 / 1.39 ms against the
// unmask's 1.30.  4 is also what the kernel's registers allow.
constexpr unsigned kFusedBlocksPerCu = 4;
constexpr unsigned kFusedStaticLds = kUnmaskStaticLds + 4u * (unsigned)kFusedRows;  // + s_row

// edges[t]: the dword before tile t as it lies in memory before the payload
// pass (tile 0 has none: 0).
__global__ void __launch_bounds__(kBlock) utf8_edges_kernel(const uint8_t* __restrict__ base,
                                                            uint32_t* __restrict__ edges, uint32_t ntiles)
{
    const uint32_t t = blockIdx.x * kBlock + threadIdx.x;
    if (t < ntiles) edges[t] = t ? *reinterpret_cast<const uint32_t*>(base + (uint64_t)t * kPlanTile - 4) : 0u;
}

// The look-back dword of each of the lane's words, still masked: the neighbour
// lane's last dword, for lane 0 of a wave the row hand-over; edge: the saved
// dword before the tile (block-uniform).  Has a barrier.
__device__ __forceinline__ void fused_lookback(const u32x4 (&v)[kUtf8V], uint32_t edge, uint32_t* s_row,
                                               uint32_t (&prev)[kUtf8V])
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 63) {
#pragma unroll
        for (int i = 0; i < kUtf8V; ++i) s_row[wave + 4 * i] = v[i].w;  // the end of row wave + 4 * i
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < kUtf8V; ++i) {
        const uint32_t up = __shfl_up(v[i].w, 1);
        const uint32_t ed = (wave == 0 && i == 0) ? edge : s_row[wave + 4 * i - 1];
        prev[i] = lane == 0 ? ed : up;
    }
}

// Word i of the lane (w, prev: as loaded, masked) against frame g = [off, end)
// with rotated key r and view gv: reports the frame if the rule rejects a byte
// of it in this word.
__device__ __forceinline__ bool fused_word_frame_bad(const u32x4& v, uint32_t prev, uint64_t a, uint64_t off,
                                                     uint64_t end, uint32_t r, uint32_t ctx)
{
    return plain_word_frame_bad(v ^ r, prev ^ r, a, off, end, ctx);
}

// Mask, store and validate a loaded tile.  rec, rec_next, ok, pre: as
// finish_tile (kmws_unmask.hip) takes them; the masks are the apply's own
// (the record's key, two_frame_masks, staged_masks: kmws_unmask_tile.hpp) and
// so are the store policies; edge: see fused_lookback.
template <bool FULL, bool TWO, bool NT>
__device__ __forceinline__ void fused_tile(uint8_t* __restrict__ base, uint64_t tile_lo, uint64_t tile_hi,
                                           const kmws_desc* __restrict__ d, uint32_t n, TileRec rec, TileRec rec_next,
                                           bool ok, const u32x4 (&v)[kUtf8V], uint32_t edge,
                                           const Utf8View* __restrict__ views, uint32_t* __restrict__ first_bad,
                                           uint64_t* s_off, uint64_t* s_end, uint32_t* s_key, uint32_t* s_row,
                                           const u32x4* pre)
{
    constexpr int V = kUtf8V;
    using Cfg = UnmaskCfg<V>;
    constexpr int SP = !NT ? kPolPlain : (TWO ? kPolStreamStoreLarge : kPolStreamStoreSmall);
    const int tid = threadIdx.x;
    const __amdgpu_buffer_rsrc_t rs = tile_rsrc(base, tile_lo, tile_hi);

    // One frame covers the tile: the record holds the whole mask.  No
    // descriptor, LDS or barrier before the stores; whether the frame is
    // checked is one scalar load that arrives under them.
    if (FULL && tile_rec_covered(rec, n)) {
        const uint32_t r = rec.rkey;
        const uint32_t f = tile_rec_frame(rec, n);
        // the frame's view and descriptor: two scalar loads that depend on the
        // record alone, issued together and under the payload (a bad plan's
        // record may hold anything: the index stays in range)
        const uint32_t fi = f < n ? f : 0u;
        const Utf8View fv = views[fi];
        const kmws_desc d0 = d[fi];
        // A bad plan stores nothing: its stores go through a resource of no
        // bytes, which drops them.  Not `if (ok)`: after a branch around the
        // stores the compiler no longer knows that the loads have arrived, and
        // waits for the whole memory queue -- the stores' write-through included
        // -- at the next use of a loaded word (the ASCII batch ran 2.86 ms so,
        // DESIGN 4).
        const __amdgpu_buffer_rsrc_t rs_ok = __builtin_amdgcn_make_buffer_rsrc(
            base + tile_lo, (short)0, ok ? (int)Cfg::kTile : 0, kBufferRsrcWord3);
        // each word is stored when it arrives, and nothing of what follows -- the
        // wait for the view and the descriptor least of all -- moves up between
        // or ahead of the stores
#pragma unroll
        for (int i = 0; i < V; ++i) {
            __builtin_amdgcn_sched_barrier(0);
            store_word<SP>(v[i] ^ r, rs_ok, 16u * (uint32_t)(tid + kBlock * i));
        }
        __builtin_amdgcn_sched_barrier(0);
        // block-uniform: binary, RSV1 and control tiles end here (a covering
        // frame is never empty and never starts past the tile's first byte)
        if (!ok | (f >= n) | !(fv.w & kUtf8Checked) | (d0.len == 0u) | (d0.off > tile_lo)) return;
        uint32_t prev[V];
        fused_lookback(v, edge, s_row, prev);
        covered_tile_check(v, prev, r, tile_lo, d0, fv, f, first_bad);
        return;
    }

    // frames [f0, flast] are the only ones that can overlap the tile
    const uint32_t f0 = tile_rec_frame(rec, n);
    const uint32_t flast = tile_rec_frame(rec_next, n);
    const kmws_desc d0 = d[f0 < n ? f0 : 0];

    // Two frames at most, in the capped launches: both descriptors are
    // block-uniform scalars, every mask is built before the first store.
    if (TWO && FULL && flast <= f0 + 1 && f0 < n) {
        const bool two = flast > f0 && flast < n;
        const kmws_desc d1 = two ? d[flast] : kmws_desc{~0ull, 0u, 0u};
        u32x4 m[V];
        const auto [r0, r1, s0, t0, s1, t1] = two_frame_masks(tile_lo, d0, d1, tid, m);
        // the two views: scalar loads beside the descriptors', used after the stores
        const Utf8View v0 = views[f0];
        const Utf8View v1 = two ? views[flast] : Utf8View{0u, 0u};
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int i = 0; i < V; ++i) {
            const bool st = ok && (m[i].x | m[i].y | m[i].z | m[i].w) != 0u;
            store_word<SP>(v[i] ^ m[i], rs, st ? 16u * (uint32_t)(tid + kBlock * i) : kFusedNoStore);
        }
        if (!ok) return;
        const bool c0 = (v0.w & kUtf8Checked) != 0u && t0 > s0, c1 = (v1.w & kUtf8Checked) != 0u && t1 > s1;
        if (!c0 && !c1) return;  // block-uniform
        uint32_t prev[V];
        fused_lookback(v, edge, s_row, prev);
#pragma unroll
        for (int i = 0; i < V; ++i) {
            const uint32_t x = 16u * (uint32_t)(tid + kBlock * i);
            const uint64_t a = tile_lo + x;
            if (c0 && s0 < x + 16 && t0 > x &&
                fused_word_frame_bad(v[i], prev[i], a, d0.off, d0.off + d0.len, r0, v0.w))
                report_bad(first_bad, v0.slot, f0);
            if (c1 && s1 < x + 16 && t1 > x &&
                fused_word_frame_bad(v[i], prev[i], a, d1.off, d1.off + d1.len, r1, v1.w))
                report_bad(first_bad, v1.slot, flast);
        }
        return;
    }

    // General path: the descriptors of the frames overlapping the tile staged
    // in LDS, a byte-exact mask per 16-byte word.
    u32x4 m[V];
    staged_masks(tile_lo, tile_hi, d, n, f0, flast, pre, s_off, s_end, s_key, tid, m);
    // Validation of the words of checked frames: utf8_payload_kernel's general path.
    bool any = false;
    uint32_t fl = flast >= n ? n - 1 : flast;
    if (fl < f0) fl = f0;
    if (ok && f0 < n)
        for (uint32_t g = f0 + (uint32_t)tid; g <= fl; g += kBlock) any |= (views[g].w & kUtf8Checked) != 0u;
    if (__syncthreads_or(any)) {
        uint32_t prev[V];
        fused_lookback(v, edge, s_row, prev);
        frames_check<true>(v, prev, tile_lo, tile_hi, d, f0, fl, views, first_bad);
    }
    // The stores come last here: the validation above loads descriptors and
    // views, and a load's wait also waits for every store issued before it.
#pragma unroll
    for (int i = 0; i < V; ++i) {
        const uint32_t x = 16u * (uint32_t)(tid + kBlock * i);
        const u32x4 mm = m[i];
        const bool st = ok && (mm.x | mm.y | mm.z | mm.w) != 0u;  // past a partial tile's end the resource drops it
        store_word<SP>(v[i] ^ mm, rs, st ? x : kFusedNoStore);
    }
}

// One block per full tile, the apply's grid (unmask_split_kernel): the same
// block -> tile mapping, metadata loads ahead of the payload loads, and in the
// uncapped launches the tile's descriptors ahead of both.
template <bool TWO, bool NT>
__global__ void __launch_bounds__(kBlock) unmask_utf8_split_kernel(uint8_t* __restrict__ base,
                                                                   const kmws_desc* __restrict__ d, uint32_t n,
                                                                   const TileRec* __restrict__ map,
                                                                   const WsHead* __restrict__ head,
                                                                   const Utf8View* __restrict__ views,
                                                                   uint32_t* __restrict__ first_bad,
                                                                   const uint32_t* __restrict__ edges, TileMapping tm,
                                                                   uint32_t b0)
{
    using Cfg = UnmaskCfg<kUtf8V>;
    __shared__ uint64_t s_off[Cfg::kCap];
    __shared__ uint64_t s_end[Cfg::kCap];
    __shared__ uint32_t s_key[Cfg::kCap];
    __shared__ uint32_t s_row[kFusedRows];
    const uint32_t tile = tile_of_block(b0 + blockIdx.x, tm);
    const uint64_t lo = (uint64_t)tile * Cfg::kTile;
    const TileRecPair recs = *reinterpret_cast<const TileRecPair*>(map + tile);
    const TileRec rec = recs.at, rec_next = recs.next;
    const uint32_t status = head->status;
    const uint32_t edge = edges[tile];  // block-uniform: a scalar load, ahead of the payload
    u32x4 v[kUtf8V];
    if constexpr (!TWO) {
        const uint32_t f = tile_rec_frame(rec, n), fl = tile_rec_frame(rec_next, n);
        const uint32_t fi = f + threadIdx.x;
        u32x4 pre = u32x4{0, 0, 0, 0};
        if (fi < n && fi <= fl) pre = *reinterpret_cast<const u32x4*>(d + fi);
        load_tile<kUtf8V, true>(base, lo, lo + Cfg::kTile, v);
        __builtin_amdgcn_sched_barrier(0);
        fused_tile<true, TWO, NT>(base, lo, lo + Cfg::kTile, d, n, rec, rec_next, (status & kStatusBadDesc) == 0, v,
                                  edge, views, first_bad, s_off, s_end, s_key, s_row, &pre);
        return;
    }
    __builtin_amdgcn_sched_barrier(0);
    load_tile<kUtf8V, true>(base, lo, lo + Cfg::kTile, v);
    __builtin_amdgcn_sched_barrier(0);
    fused_tile<true, TWO, NT>(base, lo, lo + Cfg::kTile, d, n, rec, rec_next, (status & kStatusBadDesc) == 0, v, edge,
                              views, first_bad, s_off, s_end, s_key, s_row, nullptr);
}

// One block for the partial last tile of a span.
__global__ void __launch_bounds__(kBlock) unmask_utf8_tail_kernel(uint8_t* __restrict__ base, uint64_t span,
                                                                  const kmws_desc* __restrict__ d, uint32_t n,
                                                                  const TileRec* __restrict__ map,
                                                                  const WsHead* __restrict__ head,
                                                                  const Utf8View* __restrict__ views,
                                                                  uint32_t* __restrict__ first_bad,
                                                                  const uint32_t* __restrict__ edges, uint32_t tile)
{
    using Cfg = UnmaskCfg<kUtf8V>;
    __shared__ uint64_t s_off[Cfg::kCap];
    __shared__ uint64_t s_end[Cfg::kCap];
    __shared__ uint32_t s_key[Cfg::kCap];
    __shared__ uint32_t s_row[kFusedRows];
    const uint64_t tile_lo = (uint64_t)tile * Cfg::kTile;
    const uint32_t edge = edges[tile];  // block-uniform: a scalar load, ahead of the payload
    u32x4 v[kUtf8V];
    load_tile<kUtf8V, false>(base, tile_lo, span, v);
    __builtin_amdgcn_sched_barrier(0);
    fused_tile<false, false, true>(base, tile_lo, span, d, n, map[tile], map[tile + 1],
                                   (head->status & kStatusBadDesc) == 0, v, edge, views, first_bad, s_off, s_end,
                                   s_key, s_row, nullptr);
}

// ---- the host path: kmws_decoder_set_utf8_check (kmws_decoder.cpp) ----
//
// unmask_pieces_kernel (kmws_unmask.hip) with the validation in its pass: block
// b handles piece pieces[b] of one frame's 16-byte aligned hull, 256 lanes x 4
// words, word w0 + tid + 256 i -- so a wave-instruction loads one 1 KiB row, row
// = wave + 4 i, the layout fused_lookback hands over.  The frame's message
// state is not scanned for here: the host decoder walks each connection's
// frames in order and passes the view (kmws_utf8_stream.hpp).  The unmask is the
// pieces kernel's (piece_hull, load_piece, store_piece: kmws_unmask_tile.hpp);
// a key of 0 stores nothing (an unmasked frame of a CLIENT-mode decoder is only
// checked).  The look-back of the piece's
// first word is `edge`, which the HOST read before the launch: the piece before
// belongs to another block, which may or may not have stored those bytes
// unmasked already (the race of the fused in-place pass above; here every
// payload lies in host memory, so the host reads the 4 bytes while it builds the
// piece list and no pre-pass kernel is needed).  Piece 0 starts at the frame's
// first byte and takes its look-back from the view.  A rejected byte is
// reported with a plain byte store of 1 to the frame's verdict byte in pinned
// host memory, at most one lane per wave; the host zeroes the bytes before the
// launch and reads them after its wait.
static_assert(kPieceWords == kUtf8V * kBlock, "a piece is a tile of the validator: fused_lookback's rows");
__global__ void __launch_bounds__(kBlock) unmask_pieces_utf8_kernel(uint8_t* __restrict__ base,
                                                                    const kmws_desc* __restrict__ d,
                                                                    const Utf8View* __restrict__ views,
                                                                    const PieceRecEdge* __restrict__ pieces,
                                                                    uint8_t* __restrict__ verdict)
{
    constexpr int V = kUtf8V;
    __shared__ uint32_t s_row[kFusedRows];
    const PieceRecEdge pr = pieces[blockIdx.x];
    const kmws_desc x = d[pr.frame];
    const Utf8View fv = views[pr.frame];
    const PieceHull h = piece_hull(x, pr.piece);
    u32x4 v[V];
    load_piece(base, h, v);
    if (x.key != 0u) store_piece(base, x, h, v);  // block-uniform
    if (!(fv.w & kUtf8Checked)) return;  // block-uniform: binary, RSV1 and control frames end here
    uint32_t prev[V];
    fused_lookback(v, pr.piece ? pr.edge : 0u, s_row, prev);
    bool bad = false;
#pragma unroll
    for (int i = 0; i < V; ++i) {
        const uint64_t w = h.w0 + threadIdx.x + (uint64_t)kBlock * i;
        if (w < h.w1) bad |= fused_word_frame_bad(v[i], prev[i], 16 * w, x.off, h.end, h.r, fv.w);  // past the hull: nothing
    }
    const unsigned long long m = __ballot(bad);  // one report per wave
    if (m != 0ull && (int)(threadIdx.x & 63) == __ffsll((long long)m) - 1) verdict[fv.slot] = (uint8_t)1;
}

kmws_status launch_unmask_pieces_utf8(uint8_t* base, const kmws_desc* descs, const Utf8View* views,
                                      const PieceRecEdge* pieces, uint32_t np, uint8_t* verdict, hipStream_t s)
{
    if (np == 0) return KMWS_OK;
    if (!base || !descs || !views || !pieces || !verdict) return KMWS_ERR_INVALID_PARAM;
    hipLaunchKernelGGL(unmask_pieces_utf8_kernel, dim3(np), dim3(kBlock), 0, s, base, descs, views, pieces, verdict);
    return hip_status(hipGetLastError());
}

kmws_status stream_args_check(bool ptrs_ok, const void* a, const void* b, uint32_t n, const uint32_t* stream_first,
                              uint32_t n_streams, size_t need, size_t have)
{
    if (n >= 0x80000000u || n_streams >= 0x80000000u) return KMWS_ERR_INVALID_PARAM;
    if (n && !ptrs_ok) return KMWS_ERR_INVALID_PARAM;
    if ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b)) & 15u) return KMWS_ERR_INVALID_PARAM;
    if (n && (n_streams == 0u || (!stream_first && n_streams != 1u))) return KMWS_ERR_INVALID_PARAM;
    if (have < need) return KMWS_ERR_BUFFER_TOO_SMALL;
    if (!have_device()) return KMWS_ERR_NOT_SUPPORTED;
    return KMWS_OK;
}

// The per-frame kernels of a batch (1-3 of the list above) and the finish (5),
// on the frame arrays of a workspace whose status word has been cleared.
struct Utf8Arrays {
    uint32_t* first_bad;
    Utf8Elem *elems, *aggs, *pre, *carry_tmp;
    const Utf8View* views;
    uint32_t nblk;
};
static Utf8Arrays utf8_arrays(void* workspace, const FrameArraysWs& w)
{
    return Utf8Arrays{at<uint32_t>(workspace, w.first_bad), at<Utf8Elem>(workspace, w.elems),
                      at<Utf8Elem>(workspace, w.aggs),      at<Utf8Elem>(workspace, w.pre),
                      at<Utf8Elem>(workspace, w.carry),     at<const Utf8View>(workspace, w.elems), w.nblk};
}
static void launch_utf8_frames(const Utf8Arrays& a, WsHead* head, const uint8_t* base, uint64_t span,
                               const kmws_desc* descs, const uint16_t* flags, uint32_t n, int masked,
                               uint32_t skip_flag, const uint32_t* stream_first, uint32_t n_streams,
                               const kmws_utf8_carry* carry_in, hipStream_t s)
{
    const uint32_t sblk = stream_first ? (n_streams + 1u + kBlock - 1) / kBlock : 0u;
    hipLaunchKernelGGL(utf8_elem_kernel, dim3(a.nblk > sblk ? a.nblk : sblk), dim3(kBlock), 0, s, base, span, descs,
                       flags, n, masked, skip_flag, stream_first, n_streams, carry_in, a.elems, a.first_bad, a.aggs,
                       a.nblk, head);
    hipLaunchKernelGGL(utf8_scan_aggs_kernel, dim3(1), dim3(kBlock), 0, s, a.aggs, a.pre, a.nblk);
    hipLaunchKernelGGL(utf8_ctx_kernel, dim3(a.nblk), dim3(kBlock), 0, s, flags, n, skip_flag, stream_first, n_streams,
                       carry_in, a.elems, a.pre, a.first_bad, a.carry_tmp);
}
static void launch_utf8_finish(const Utf8Arrays& a, uint32_t n, const uint32_t* stream_first, uint32_t n_streams,
                               const kmws_utf8_carry* carry_in, kmws_utf8_carry* carry_out, uint8_t* out, hipStream_t s)
{
    const uint32_t fin_lanes = carry_out && n_streams > n ? n_streams : n;
    hipLaunchKernelGGL(utf8_finish_kernel, dim3((fin_lanes + kBlock - 1) / kBlock), dim3(kBlock), 0, s, n,
                       stream_first, n_streams, a.views, a.first_bad, a.carry_tmp, carry_in, carry_out, out);
}
kmws_status launch_utf8_carry_copy(uint32_t n_streams, const kmws_utf8_carry* carry_in, kmws_utf8_carry* carry_out,
                                   hipStream_t s)
{
    if (carry_out && n_streams)
        hipLaunchKernelGGL(utf8_carry_copy_kernel, dim3((n_streams + kBlock - 1) / kBlock), dim3(kBlock), 0, s,
                           n_streams, carry_in, carry_out);
    return hip_status(hipGetLastError());
}

// ---- for the validating gather (kmws_pack.hip, declared in kmws_utf8_dev.hpp) ----
Utf8FrameArrays launch_utf8_frame_state(void* workspace, const FrameArraysWs& fa, const uint8_t* base, uint64_t span,
                                        const kmws_desc* descs, const uint16_t* flags, uint32_t n, int masked,
                                        uint32_t skip_flag, const uint32_t* stream_first, uint32_t n_streams,
                                        const kmws_utf8_carry* carry_in, hipStream_t s)
{
    const Utf8Arrays a = utf8_arrays(workspace, fa);
    launch_utf8_frames(a, at<WsHead>(workspace, 0), base, span, descs, flags, n, masked, skip_flag, stream_first,
                       n_streams, carry_in, s);
    return Utf8FrameArrays{a.views, a.first_bad};
}
void launch_utf8_frame_finish(void* workspace, const FrameArraysWs& fa, uint32_t n, const uint32_t* stream_first,
                              uint32_t n_streams, const kmws_utf8_carry* carry_in, kmws_utf8_carry* carry_out,
                              uint8_t* out, hipStream_t s)
{
    launch_utf8_finish(utf8_arrays(workspace, fa), n, stream_first, n_streams, carry_in, carry_out, out, s);
}

// The argument checks of the fused entries: the schedule to run (`code`), then
// the stream arguments.  Every failure ahead of the workspace size is
// KMWS_ERR_INVALID_PARAM, so the schedule's test stands in front.
static kmws_status fused_check(const uint8_t* base, bool ptrs_ok, uint32_t n, const uint32_t* stream_first,
                               uint32_t n_streams, uint64_t span, int schedule, size_t workspace_bytes,
                               const FusedWs& w, Schedule* sc)
{
    if (!decode_schedule(schedule < 0 ? default_schedule(span, n) : (uint32_t)schedule, sc))
        return KMWS_ERR_INVALID_PARAM;
    return stream_args_check(ptrs_ok, base, nullptr, n, stream_first, n_streams, n ? w.total : 0, workspace_bytes);
}

// Behind a launched plan (and the header parse, if any): the look-back
// pre-pass, the per-frame kernels on the still-masked payload, the fused
// payload pass on the apply's grids, the finish.
static kmws_status launch_fused(const Schedule& sc, uint8_t* base, uint64_t span, const kmws_desc* descs,
                                const uint16_t* flags, uint32_t n, const uint32_t* stream_first, uint32_t n_streams,
                                const kmws_utf8_carry* carry_in, kmws_utf8_carry* carry_out, uint8_t* out,
                                void* workspace, const FusedWs& w, hipStream_t s)
{
    const Utf8Arrays a = utf8_arrays(workspace, w.u.fa);
    WsHead* head = at<WsHead>(workspace, 0);
    const TileRec* map = at<const TileRec>(workspace, w.u.plan.map);
    uint32_t* edges = at<uint32_t>(workspace, w.edges);
    const uint64_t ntiles = w.u.plan.ntiles;  // launch_plan bounded it
    const uint64_t nfull = span / kPlanTile;
    if (ntiles)
        hipLaunchKernelGGL(utf8_edges_kernel, dim3((uint32_t)((ntiles + kBlock - 1) / kBlock)), dim3(kBlock), 0, s,
                           base, edges, (uint32_t)ntiles);
    launch_utf8_frames(a, head, base, span, descs, flags, n, 1, kUtf8SkipNone, stream_first, n_streams, carry_in, s);

    // the apply's test for the capped launches and its means (dynamic LDS the
    // kernel does not use), with this kernel's own number of blocks per CU
    const unsigned lds_pad = unmask_capped(span, n) ? lds_pad_for(kFusedBlocksPerCu, kFusedStaticLds) : 0u;
    const TileMapping tm = tile_mapping((uint32_t)nfull, sc.split);
    launch_split_grid(nfull, lds_pad, sc.temporal, [&](auto two, auto nt, dim3 grid, uint32_t b0, unsigned pad) {
        hipLaunchKernelGGL((unmask_utf8_split_kernel<decltype(two)::value, decltype(nt)::value>), grid, dim3(kBlock), pad,
                           s, base, descs, n, map, head, a.views, a.first_bad, edges, tm, b0);
    });
    if (ntiles > nfull)  // the partial last tile
        hipLaunchKernelGGL(unmask_utf8_tail_kernel, dim3(1), dim3(kBlock), 0, s, base, span, descs, n, map, head,
                           a.views, a.first_bad, edges, (uint32_t)nfull);
    launch_utf8_finish(a, n, stream_first, n_streams, carry_in, carry_out, out, s);
    return hip_status(hipGetLastError());
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
    const Utf8Ws w = utf8_ws(span, n, n_streams);
    kmws_status st = stream_args_check(base && descs && flags && out && workspace, base, nullptr, n, stream_first,
                                       n_streams, n ? w.total : 0, workspace_bytes);
    if (st != KMWS_OK) return st;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (n == 0) return launch_utf8_carry_copy(n_streams, carry_in, carry_out, s);  // every stream's state passes through
    st = launch_plan(span, descs, n, workspace, w.plan.total, s);
    if (st != KMWS_OK) return st;
    note_device_batch(span, s);

    const Utf8Arrays a = utf8_arrays(workspace, w.fa);
    WsHead* head = at<WsHead>(workspace, 0);
    const TileRec* map = at<const TileRec>(workspace, w.plan.map);
    const int masked = payload_masked != 0;
    launch_utf8_frames(a, head, base, span, descs, flags, n, masked, kUtf8SkipNone, stream_first, n_streams, carry_in,
                       s);

    Split sp;
    (void)split_of(KMWS_SCHED_SPLIT4, &sp);
    const TileMapping tm = tile_mapping((uint32_t)(span / kPlanTile), sp);  // the partial last tile maps to itself
    launch_split_grid(w.plan.ntiles, 0u, false, [&](auto, auto, dim3 grid, uint32_t b0, unsigned) {  // launch_plan bounded it
        if (masked)
            hipLaunchKernelGGL(utf8_payload_kernel<true>, grid, dim3(kBlock), 0, s, base, span, descs, n, map, head,
                               a.views, a.first_bad, tm, b0);
        else
            hipLaunchKernelGGL(utf8_payload_kernel<false>, grid, dim3(kBlock), 0, s, base, span, descs, n, map, head,
                               a.views, a.first_bad, tm, b0);
    });
    launch_utf8_finish(a, n, stream_first, n_streams, carry_in, carry_out, out, s);
    return hip_status(hipGetLastError());
}

size_t kmws_unmask_utf8_workspace_size(uint64_t span, uint32_t n, uint32_t n_streams)
{
    return fused_ws(span, n, n_streams).total;
}

kmws_status kmws_unmask_utf8_batch(uint8_t* base, uint64_t span, const kmws_desc* descs, const uint16_t* flags,
                                   uint32_t n, const uint32_t* stream_first, uint32_t n_streams,
                                   const kmws_utf8_carry* carry_in, kmws_utf8_carry* carry_out, uint8_t* out,
                                   void* workspace, size_t workspace_bytes, int schedule, void* stream)
{
    const FusedWs w = fused_ws(span, n, n_streams);
    Schedule sc;
    kmws_status st = fused_check(base, base && descs && flags && out && workspace, n, stream_first, n_streams, span,
                                 schedule, workspace_bytes, w, &sc);
    if (st != KMWS_OK) return st;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (n == 0) return launch_utf8_carry_copy(n_streams, carry_in, carry_out, s);
    st = launch_plan(span, descs, n, workspace, w.u.plan.total, s);
    if (st != KMWS_OK) return st;
    note_device_batch(2 * span, s);
    return launch_fused(sc, base, span, descs, flags, n, stream_first, n_streams, carry_in, carry_out, out, workspace,
                        w, s);
}

kmws_status kmws_unpack_unmask_utf8(uint8_t* wire, uint64_t wire_len, const uint64_t* hdr_off, uint32_t n, int mode,
                                    kmws_desc* out_desc, uint16_t* out_flags, uint8_t* out_err,
                                    const uint32_t* stream_first, uint32_t n_streams, const kmws_utf8_carry* carry_in,
                                    kmws_utf8_carry* carry_out, uint8_t* out_utf8, void* workspace,
                                    size_t workspace_bytes, int schedule, void* stream)
{
    const FusedWs w = fused_ws(wire_len, n, n_streams);
    Schedule sc;
    if (!mode_ok(mode)) return KMWS_ERR_INVALID_PARAM;
    const bool fits = w.u.plan.ntiles <= 0x7FFFFFFFull;  // the plan's tile index
    kmws_status st = fused_check(wire, wire && hdr_off && out_desc && out_flags && out_utf8 && workspace && fits, n,
                                 stream_first, n_streams, wire_len, schedule, workspace_bytes, w, &sc);
    if (st != KMWS_OK) return st;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (n == 0) return launch_utf8_carry_copy(n_streams, carry_in, carry_out, s);
    st = launch_unpack_plan(wire, wire_len, hdr_off, n, mode, out_desc, out_flags, out_err, workspace, s);
    if (st != KMWS_OK) return st;
    note_device_batch(2 * wire_len, s);
    return launch_fused(sc, wire, wire_len, out_desc, out_flags, n, stream_first, n_streams, carry_in, carry_out,
                        out_utf8, workspace, w, s);
}

}  // extern "C"
