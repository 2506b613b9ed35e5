// The message table of a device batch for MI355X (gfx950): kmws_msg_index.  The
// rule is stated in kmws_msg_rule.hpp; this file is the two segmented scans of
// it over a batch of many streams' frames, both through the scan core of
// kmws_stream_scan.hpp at four consecutive frames a lane.
//
// Scan A (MsgStateOp) gives the state before each frame: two last-writer words
// in 11 bits under msg_compose, a stream's first frame composed behind the
// constant of its carry.  Scan B (MsgSumOp) needs that state: from it a frame's
// class follows, and a record's totals are a segmented sum (MsgSum) that is
// reset where a record starts and at a stream's first frame.  Five kernels:
//   1. msg_state_kernel: a lane reads its frames' flags, finds the stream edges
//      and scans the block's state functions; per block the aggregate.  Its lanes
//      also check stream_first and the carries; status bits ride above the
//      aggregate;
//   2. msg_scan_states_kernel: scan_aggregates over those, and the status word's
//      store: cleared, or the OR of the blocks';
//   3. msg_class_kernel: scan A again, now behind the block's prefix: the state
//      before every frame, its class, and with the members' lengths the block's
//      scan B.  Per frame one 16-bit word (class, stream edges, the records
//      started before it in the block), per block the aggregate;
//   4. msg_scan_sums_kernel: scan_aggregates over those; *msg_count, and status
//      bit 1 when msg_cap is too small;
//   5. msg_finish_kernel: scan B again from the stored words and the lengths,
//      behind the block's prefix.  A record's totals are complete at the next
//      reset point: the lane that owns it writes the record from the exclusive
//      value there, and the lane of frame n - 1 writes the last one from the
//      inclusive value.  msg_of per frame, carry_out at a stream's last frame;
//      per stream stream_msg_first and an empty stream's carry.
// Nothing is stored per frame between the passes but the 16-bit word: flags (2 B)
// are read twice and the lengths (one dword of a 16-byte descriptor) twice,
// which is cheaper than storing and reloading a 24-byte sum per frame.
// Vector stores and plain C++ only.
#include <stddef.h>

#include "kmws_common.hpp"
#include "kmws_msg_rule.hpp"
#include "kmws_stream_scan.hpp"
#include "kmws_workspace.hpp"

namespace kmws {

constexpr int kMsgV = (int)kScanFramesPerLane;
static_assert(kMsgV == 4, "a lane's frames are one 64-bit word of the per-frame array");
static_assert(kMsgBlockFrames == kScanBlockFrames, "the constant the tests read");
static_assert(sizeof(kmws_msg) == 48 && sizeof(kmws_msg_carry) == 16 && sizeof(MsgSum) == 24, "the ABI and the workspace");

// The per-frame word: the class (bits 0-2), the frame is its stream's first /
// last, and from bit 6 the records started before it in its block (< 1024).
constexpr uint32_t kMsgClsFirst = 8u, kMsgClsLast = 16u;
constexpr int kMsgClsStartsShift = 6;
static_assert(((kScanBlockFrames - 1) << kMsgClsStartsShift) <= 0xFFFFu, "the count fits the word");

struct MsgStateOp : ScanWordOp {  // scan A: one state function in 11 bits
    static __device__ __forceinline__ T identity() { return msg_identity(); }
    static __device__ __forceinline__ T compose(T a, T b) { return msg_compose(a, b); }
};
// Scan B.  A sum in memory is read and written field by field (a struct copy
// through a pointer keeps it out of registers).
struct MsgSumOp {
    using T = MsgSum;
    static __device__ __forceinline__ T identity() { return msg_sum_identity(); }
    static __device__ __forceinline__ T compose(const T& a, const T& b) { return msg_sum_compose(a, b); }
    static __device__ __forceinline__ T shfl_up(const T& v, int dlt)
    {
        T r;
        r.starts = __shfl_up(v.starts, dlt), r.first = __shfl_up(v.first, dlt);
        r.last = __shfl_up(v.last, dlt), r.frames = __shfl_up(v.frames, dlt);
        r.bytes = __shfl_up((unsigned long long)v.bytes, dlt);
        return r;
    }
    static __device__ __forceinline__ T load(const T* p) { return T{p->starts, p->first, p->last, p->frames, p->bytes}; }
    static __device__ __forceinline__ void store(T* p, const T& v)
    {
        p->starts = v.starts, p->first = v.first, p->last = v.last, p->frames = v.frames, p->bytes = v.bytes;
    }
};

// kmws_msg_carry has byte alignment: read and written byte by byte.
__device__ __forceinline__ kmws_msg_carry msg_load_carry(const kmws_msg_carry* __restrict__ c, uint32_t s)
{
    kmws_msg_carry r;
    for (int k = 0; k < 16; ++k) r.b[k] = c ? c[s].b[k] : (uint8_t)0;
    return r;
}
__device__ __forceinline__ void msg_store_carry(kmws_msg_carry* __restrict__ c, uint32_t s, const kmws_msg_carry& v)
{
    for (int k = 0; k < 16; ++k) c[s].b[k] = v.b[k];
}

// A lane's four frames for scan A: inc[k] = the state function of frames 0..k
// (a stream's first frame behind the constant of its carry), and per frame b0,
// the stream edge bits and, at a stream's first frame, the carried state.
struct MsgLane {
    uint32_t inc[kMsgV], b0[kMsgV], edge[kMsgV], carried[kMsgV];
};
__device__ __forceinline__ void msg_lane_states(const uint16_t* __restrict__ flags, uint32_t n,
                                                const uint32_t* __restrict__ first, uint32_t ns,
                                                const kmws_msg_carry* __restrict__ carry_in, uint32_t i0, MsgLane& L)
{
#pragma unroll
    for (int k = 0; k < kMsgV; ++k) L.inc[k] = msg_identity(), L.b0[k] = 0x80u | KMWS_OP_PING, L.edge[k] = L.carried[k] = 0u;
    if (i0 >= n) return;
    const LaneStreams streams(first, ns, n, i0, kMsgV);
#pragma unroll
    for (int k = 0; k < kMsgV; ++k) {
        const uint32_t i = i0 + k;
        uint32_t f = msg_identity();
        if (i < n) {
            L.b0[k] = flags[i] & 0xFFu;
            f = msg_frame_fn(L.b0[k]);
            const FrameStream fs = streams.at(i);
            if (fs.first) {
                const uint32_t c = carry_in ? carry_in[fs.s].b[0] : 0u;
                L.carried[k] = (c & kMsgOpen) ? c : 0u;
                f = msg_compose(msg_const(L.carried[k]), f);
                L.edge[k] |= kMsgClsFirst;
            }
            if (fs.last) L.edge[k] |= kMsgClsLast;
        }
        L.inc[k] = k ? msg_compose(L.inc[k - 1], f) : f;
    }
}

__global__ void __launch_bounds__(kBlock) msg_state_kernel(const uint16_t* __restrict__ flags, uint32_t n,
                                                           const uint32_t* __restrict__ first, uint32_t ns,
                                                           const kmws_msg_carry* __restrict__ carry_in,
                                                           uint32_t* __restrict__ aggs_a)
{
    __shared__ uint32_t s_wave[kScanWaves];
    const uint32_t i0 = (blockIdx.x * kBlock + threadIdx.x) * kMsgV;
    bool bad_args = false;
#pragma unroll
    for (int k = 0; k < kMsgV; ++k) {
        const uint32_t x = i0 + k;
        bad_args |= stream_first_bad(first, ns, n, x);
        if (carry_in && x < ns) bad_args |= !msg_carry_ok(msg_load_carry(carry_in, x));
    }
    MsgLane L;
    msg_lane_states(flags, n, first, ns, carry_in, i0, L);
    uint32_t total;
    block_scan_excl<MsgStateOp>(L.inc[kMsgV - 1], s_wave, &total);
    const int any_bad = __syncthreads_or(bad_args ? 1 : 0);
    if (threadIdx.x == 0) aggs_a[blockIdx.x] = total | (any_bad ? kStatusBadDesc << 16 : 0u);
}

// pre_a[b] = the composition of aggs_a[0 .. b); the status word = the OR of the
// blocks' status bits, stored (so cleared when there are none).
__global__ void __launch_bounds__(kBlock) msg_scan_states_kernel(const uint32_t* __restrict__ aggs_a,
                                                                 uint32_t* __restrict__ pre_a, uint32_t nagg,
                                                                 WsHead* __restrict__ head)
{
    __shared__ uint32_t s_wave[kScanWaves];
    uint32_t status = 0;
    const auto load = [&](uint32_t b) {
        const uint32_t a = b < nagg ? aggs_a[b] : msg_identity();
        status |= a >> 16;
        return a & kMsgFnBits;
    };
    scan_aggregates<MsgStateOp>(nagg, s_wave, load, [&](uint32_t b, uint32_t p) { pre_a[b] = p; });
    const int any_bad = __syncthreads_or((int)(status & kStatusBadDesc));
    if (threadIdx.x == 0) head->status = any_bad ? kStatusBadDesc : 0u;
}

__global__ void __launch_bounds__(kBlock) msg_class_kernel(const kmws_desc* __restrict__ d,
                                                           const uint16_t* __restrict__ flags, uint32_t n,
                                                           const uint32_t* __restrict__ first, uint32_t ns,
                                                           const kmws_msg_carry* __restrict__ carry_in,
                                                           const uint32_t* __restrict__ pre_a,
                                                           uint16_t* __restrict__ cls_out, MsgSum* __restrict__ aggs_b)
{
    __shared__ uint32_t s_wave[kScanWaves];
    __shared__ MsgSum s_sum[kScanWaves];
    const uint32_t i0 = (blockIdx.x * kBlock + threadIdx.x) * kMsgV;
    MsgLane L;
    msg_lane_states(flags, n, first, ns, carry_in, i0, L);
    uint32_t total_a;
    // everything before the lane's first frame; a constant function unless that frame starts the batch
    const uint32_t excl_a = msg_compose(pre_a[blockIdx.x], block_scan_excl<MsgStateOp>(L.inc[kMsgV - 1], s_wave, &total_a));

    // Only the count of scan B is needed per frame here: the lane's frames are
    // folded into one sum for the block scan, the starts counted beside it.
    MsgSum lane_sum = msg_sum_identity();
    uint32_t cw[kMsgV], started[kMsgV];
#pragma unroll
    for (int k = 0; k < kMsgV; ++k) {
        const uint32_t i = i0 + k;
        cw[k] = 0u;
        started[k] = msg_sum_starts(lane_sum);  // before frame k, in the lane
        if (i < n) {
            const bool at_first = (L.edge[k] & kMsgClsFirst) != 0u;
            const uint32_t before = k ? msg_compose(excl_a, L.inc[k - 1]) : excl_a;
            const uint32_t c = msg_class(at_first ? L.carried[k] : msg_state_of(before),
                                         at_first ? false : msg_seen_of(before), L.b0[k]);
            cw[k] = c | L.edge[k];
            lane_sum = msg_sum_compose(lane_sum, msg_sum_of(c, at_first, i, (c & kMsgMember) ? d[i].len : 0u));
        }
    }
    MsgSum total;
    const MsgSum excl = block_scan_excl<MsgSumOp>(lane_sum, s_sum, &total);
    uint64_t word = 0;  // whole blocks in the workspace: no test against n
#pragma unroll
    for (int k = 0; k < kMsgV; ++k)
        word |= (uint64_t)(cw[k] | ((msg_sum_starts(excl) + started[k]) << kMsgClsStartsShift)) << (16 * k);
    *reinterpret_cast<uint64_t*>(cls_out + i0) = word;
    if (threadIdx.x == 0) MsgSumOp::store(&aggs_b[blockIdx.x], total);
}

// pre_b[b] = the composition of aggs_b[0 .. b), pre_b[nblk] = the batch's total;
// *msg_count; status bit 1 joins what kernel 2 stored when msg_cap is too small.
__global__ void __launch_bounds__(kBlock) msg_scan_sums_kernel(const MsgSum* __restrict__ aggs_b,
                                                               MsgSum* __restrict__ pre_b, uint32_t nblk,
                                                               uint32_t msg_cap, uint32_t* __restrict__ msg_count,
                                                               WsHead* __restrict__ head)
{
    __shared__ MsgSum s_sum[kScanWaves];
    const auto load = [&](uint32_t b) {
        MsgSum a = MsgSumOp::load(&aggs_b[b < nblk ? b : 0u]);  // nblk >= 1
        if (b >= nblk) a = msg_sum_identity();
        return a;
    };
    const MsgSum run = scan_aggregates<MsgSumOp>(nblk, s_sum, load,
                                                 [&](uint32_t b, const MsgSum& p) { MsgSumOp::store(&pre_b[b], p); });
    if (threadIdx.x == 0) {
        MsgSumOp::store(&pre_b[nblk], run);
        const uint32_t count = msg_sum_starts(run);
        *msg_count = count;
        if (count > msg_cap) head->status = head->status | kStatusBadDesc;
    }
}

struct MsgArrays {
    const kmws_desc* d;
    const uint16_t* flags;
    const uint64_t* pos;
    const uint8_t *utf8, *proto;
    const uint32_t* first;
    uint32_t ns;
    const kmws_msg_carry* carry_in;
};
// The record of the running message of v, whose stream is s.
__device__ __forceinline__ kmws_msg msg_record_at(const MsgSum& v, uint32_t s, const MsgArrays& a)
{
    const uint32_t b0 = a.flags[v.first] & 0xFFu;
    kmws_msg m = msg_record(v, s, b0, msg_load_carry((b0 & 15u) ? nullptr : a.carry_in, s));
    m.off = a.pos ? a.pos[v.first] : a.d[v.first].off;
    const uint64_t last_at = a.pos ? a.pos[v.last] : a.d[v.last].off;
    if (last_at + a.d[v.last].len - m.off == m.bytes) m.bits |= (uint8_t)KMWS_MSG_CONTIG;
    m.utf8 = a.utf8 ? a.utf8[v.last] : (uint8_t)0;
    m.proto = a.proto ? a.proto[v.last] : (uint8_t)0;
    return m;
}
// A record goes out as three 16-byte stores; kmws_msg has 8-byte alignment.
typedef u32x4 u32x4_a8 __attribute__((aligned(8)));
static_assert(offsetof(kmws_msg, off) == 0 && offsetof(kmws_msg, bytes) == 8 && offsetof(kmws_msg, prior) == 16 &&
                  offsetof(kmws_msg, stream) == 24 && offsetof(kmws_msg, first) == 28 && offsetof(kmws_msg, last) == 32 &&
                  offsetof(kmws_msg, frames) == 36 && offsetof(kmws_msg, b0) == 40 && offsetof(kmws_msg, bits) == 41 &&
                  offsetof(kmws_msg, utf8) == 42 && offsetof(kmws_msg, proto) == 43 && offsetof(kmws_msg, reserved) == 44,
              "the words msg_store_record puts together");
__device__ __forceinline__ void msg_store_record(kmws_msg* __restrict__ msgs, uint32_t msg_cap, const MsgSum& v,
                                                 const MsgArrays& a)
{
    const uint32_t idx = msg_sum_starts(v) - 1u;
    if (idx >= msg_cap) return;  // status bit 1 says so
    const kmws_msg m = msg_record_at(v, stream_of(a.first, a.ns, v.first), a);
    u32x4_a8* dst = reinterpret_cast<u32x4_a8*>(msgs + idx);
    dst[0] = u32x4{(uint32_t)m.off, (uint32_t)(m.off >> 32), (uint32_t)m.bytes, (uint32_t)(m.bytes >> 32)};
    dst[1] = u32x4{(uint32_t)m.prior, (uint32_t)(m.prior >> 32), m.stream, m.first};
    dst[2] = u32x4{m.last, m.frames, m.b0 | (uint32_t)m.bits << 8 | (uint32_t)m.utf8 << 16 | (uint32_t)m.proto << 24,
                   m.reserved};
}

__global__ void __launch_bounds__(kBlock) msg_finish_kernel(MsgArrays a, uint32_t n,
                                                            kmws_msg_carry* __restrict__ carry_out,
                                                            uint32_t* __restrict__ msg_of, kmws_msg* __restrict__ msgs,
                                                            uint32_t msg_cap, uint32_t* __restrict__ stream_msg_first,
                                                            const uint16_t* __restrict__ cls,
                                                            const MsgSum* __restrict__ pre_b, uint32_t nblk)
{
    __shared__ MsgSum s_sum[kScanWaves];
    const uint32_t i0 = (blockIdx.x * kBlock + threadIdx.x) * kMsgV;
    if (blockIdx.x < nblk) {  // the same for the whole block: the barrier inside is met by all or none
        const uint64_t word = *reinterpret_cast<const uint64_t*>(cls + i0);
        MsgSum e[kMsgV], lane_sum = msg_sum_identity();
        uint32_t cw[kMsgV];
#pragma unroll
        for (int k = 0; k < kMsgV; ++k) {
            const uint32_t i = i0 + k;
            e[k] = msg_sum_identity();
            cw[k] = (uint32_t)(word >> (16 * k)) & 0xFFFFu;
            if (i < n) e[k] = msg_sum_of(cw[k], (cw[k] & kMsgClsFirst) != 0u, i, (cw[k] & kMsgMember) ? a.d[i].len : 0u);
            lane_sum = msg_sum_compose(lane_sum, e[k]);
        }
        MsgSum total;
        MsgSum in = msg_sum_compose(MsgSumOp::load(&pre_b[blockIdx.x]), block_scan_excl<MsgSumOp>(lane_sum, s_sum, &total));
#pragma unroll
        for (int k = 0; k < kMsgV; ++k) {
            const uint32_t i = i0 + k;
            if (i >= n) continue;
            const MsgSum ex = in;  // everything before frame i, then through it
            in = msg_sum_compose(ex, e[k]);
            // a reset point: the record before it is complete
            if ((cw[k] & (kMsgStart | kMsgClsFirst)) && msg_sum_frames(ex)) msg_store_record(msgs, msg_cap, ex, a);
            if (i == n - 1u && msg_sum_frames(in)) msg_store_record(msgs, msg_cap, in, a);
            if (msg_of) msg_of[i] = (cw[k] & kMsgMember) ? msg_sum_starts(in) - 1u : KMWS_MSG_NONE;
            if (carry_out && (cw[k] & kMsgClsLast)) {
                const uint32_t s = stream_of(a.first, a.ns, i);
                const kmws_msg_carry c = msg_load_carry(a.carry_in, s);
                // a stream without a member reads frame 0's flags for nothing: msg_carry_after passes c through
                const kmws_msg rec = msg_record(in, s, a.flags[msg_sum_frames(in) ? in.first : 0u] & 0xFFu, c);
                msg_store_carry(carry_out, s, msg_carry_after(in, rec, c));
            }
        }
    }
    if (!stream_msg_first && !carry_out) return;
#pragma unroll
    for (int k = 0; k < kMsgV; ++k) {
        const uint32_t s = i0 + k;
        if (s > a.ns) continue;
        const uint32_t f = s < a.ns ? stream_begin(a.first, s) : n;
        if (stream_msg_first)  // the records before the stream's first frame; past the last frame: all
            stream_msg_first[s] = f < n ? msg_sum_starts(pre_b[f / kScanBlockFrames]) + (cls[f] >> kMsgClsStartsShift)
                                        : msg_sum_starts(pre_b[nblk]);
        if (carry_out && s < a.ns && f >= stream_end(a.first, n, s))  // an empty stream keeps its carry
            msg_store_carry(carry_out, s, msg_load_carry(a.carry_in, s));
    }
}

// n == 0: no record, every stream's state passes through.
__global__ void __launch_bounds__(kBlock) msg_empty_kernel(uint32_t ns, const kmws_msg_carry* __restrict__ carry_in,
                                                           kmws_msg_carry* __restrict__ carry_out,
                                                           uint32_t* __restrict__ stream_msg_first,
                                                           uint32_t* __restrict__ msg_count)
{
    const uint32_t s = blockIdx.x * kBlock + threadIdx.x;
    if (s == 0) *msg_count = 0u;
    if (stream_msg_first && s <= ns) stream_msg_first[s] = 0u;
    if (carry_out && s < ns) msg_store_carry(carry_out, s, msg_load_carry(carry_in, s));
}

}  // namespace kmws

using namespace kmws;

extern "C" {

size_t kmws_msg_workspace_size(uint32_t n, uint32_t n_streams) { return msg_ws(n, n_streams).total; }

kmws_status kmws_msg_index(const kmws_desc* descs, const uint16_t* flags, const uint64_t* pos, const uint8_t* utf8,
                           const uint8_t* proto, uint32_t n, const uint32_t* stream_first, uint32_t n_streams,
                           const kmws_msg_carry* carry_in, kmws_msg_carry* carry_out, uint32_t* msg_of, kmws_msg* msgs,
                           uint32_t msg_cap, uint32_t* msg_count, uint32_t* stream_msg_first, void* workspace,
                           size_t workspace_bytes, void* stream)
{
    if (!msg_count || !workspace) return KMWS_ERR_INVALID_PARAM;
    const MsgWs w = msg_ws(n, n_streams);
    const kmws_status st = stream_args_check(descs && flags && msgs, nullptr, nullptr, n, stream_first, n_streams,
                                             n ? w.total : 0, workspace_bytes);
    if (st != KMWS_OK) return st;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (n == 0) {
        hipLaunchKernelGGL(msg_empty_kernel, dim3(n_streams / kBlock + 1), dim3(kBlock), 0, s, n_streams, carry_in,
                           carry_out, stream_msg_first, msg_count);
        return hip_status(hipGetLastError());
    }
    note_device_batch(30ull * n, s);

    WsHead* head = at<WsHead>(workspace, 0);
    uint32_t* aggs_a = at<uint32_t>(workspace, w.aggs_a);
    uint32_t* pre_a = at<uint32_t>(workspace, w.pre_a);
    MsgSum* aggs_b = at<MsgSum>(workspace, w.aggs_b);
    MsgSum* pre_b = at<MsgSum>(workspace, w.pre_b);
    uint16_t* cls = at<uint16_t>(workspace, w.cls);
    const uint32_t nagg = w.first_pass(stream_first);
    hipLaunchKernelGGL(msg_state_kernel, dim3(nagg), dim3(kBlock), 0, s, flags, n, stream_first, n_streams, carry_in,
                       aggs_a);
    hipLaunchKernelGGL(msg_scan_states_kernel, dim3(1), dim3(kBlock), 0, s, aggs_a, pre_a, nagg, head);
    hipLaunchKernelGGL(msg_class_kernel, dim3(w.nblk), dim3(kBlock), 0, s, descs, flags, n, stream_first, n_streams,
                       carry_in, pre_a, cls, aggs_b);
    hipLaunchKernelGGL(msg_scan_sums_kernel, dim3(1), dim3(kBlock), 0, s, aggs_b, pre_b, w.nblk, msg_cap, msg_count,
                       head);
    const MsgArrays arr{descs, flags, pos, utf8, proto, stream_first, n_streams, carry_in};
    const bool per_stream = stream_msg_first || carry_out;
    hipLaunchKernelGGL(msg_finish_kernel, dim3(per_stream ? nagg : w.nblk), dim3(kBlock), 0, s, arr, n, carry_out,
                       msg_of, msgs, msg_cap, stream_msg_first, cls, pre_b, w.nblk);
    return hip_status(hipGetLastError());
}

}  // extern "C"
