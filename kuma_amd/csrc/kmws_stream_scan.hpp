// The segmented-scan core of the per-stream frame checks: the frame-state
// kernels of every UTF-8 entry (kmws_utf8.hip), kmws_proto.hip, kmws_msg.hip.
//
// Each computes, per frame, a state that depends on every earlier frame of the
// same stream and on a carry from the last batch.  What a run of frames does to
// the state is an element of a monoid (the rule headers state identity and
// compose); a stream's first frame is composed behind an element that absorbs
// everything in front of it, so the state before every frame of a batch of many
// streams is one plain exclusive scan, stated here once: block_scan_excl over a
// block, scan_aggregates over the blocks' aggregates; a frame pass composes its
// block's prefix in front.  Beside it, the stream helpers and the argument check.
#pragma once
#include "kmws_common.hpp"

namespace kmws {

// Frames a block of kmws_proto_check and kmws_msg_index covers: 256 lanes, four
// consecutive frames each, scanned in registers first.  A round of
// scan_aggregates takes as many.  The UTF-8 kernels keep one frame a lane.
constexpr uint32_t kScanFramesPerLane = 4;
constexpr uint32_t kScanBlockFrames = 1024;
constexpr int kScanWaves = kBlock / 64;
static_assert(kScanBlockFrames == kScanFramesPerLane * kBlock, "a block's frames are its lanes'");

// ---- the monoid ----
// A scan element is described by a stateless struct Op: the type T, identity(),
// compose(a, b) = "a, then b", shfl_up(v, delta), and load / store of a T in LDS
// (a struct copied through a pointer may stay out of registers: such an Op moves
// its fields one by one).  ScanWordOp: the last three for one 32-bit word.
struct ScanWordOp {
    using T = uint32_t;
    static __device__ __forceinline__ T shfl_up(T v, int dlt) { return __shfl_up(v, dlt); }
    static __device__ __forceinline__ T load(const T* p) { return *p; }
    static __device__ __forceinline__ void store(T* p, T v) { *p = v; }
};

// Exclusive scan over the block of one element per lane -- the wave by lane
// shuffles, the waves through s_wave (kScanWaves LDS entries, free again after
// the next barrier), one barrier; *total: the whole block's.
template <class Op>
__device__ __forceinline__ typename Op::T block_scan_excl(typename Op::T v, typename Op::T* s_wave,
                                                          typename Op::T* total)
{
    using T = typename Op::T;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int dlt = 1; dlt < 64; dlt <<= 1) {
        const T up = Op::shfl_up(v, dlt);
        if (lane >= dlt) v = Op::compose(up, v);
    }
    const T before = Op::shfl_up(v, 1);
    if (lane == 63) Op::store(&s_wave[wave], v);
    __syncthreads();
    T pre = Op::identity(), tot = Op::identity();
#pragma unroll
    for (int w = 0; w < kScanWaves; ++w) {
        const T a = Op::load(&s_wave[w]);
        if (w < wave) pre = Op::compose(pre, a);
        tot = Op::compose(tot, a);
    }
    *total = tot;
    if (lane) pre = Op::compose(pre, before);
    return pre;
}

// The scan of nagg block aggregates by one block: load(b) returns aggregate b
// (the identity past nagg; it may OR status bits into a variable of the lane),
// store(b, p) takes p = the composition of aggregates [0, b) for every b < nagg.
template <class Op, class Load, class Store>
__device__ __forceinline__ typename Op::T scan_aggregates(uint32_t nagg, typename Op::T* s_wave, Load load,
                                                          Store store)
{
    using T = typename Op::T;
    constexpr int V = (int)kScanFramesPerLane;
    T run = Op::identity();
    for (uint32_t c0 = 0; c0 < nagg; c0 += kScanBlockFrames) {
        const uint32_t b0 = c0 + threadIdx.x * V;
        T a[V], lane_sum = Op::identity();
#pragma unroll
        for (int k = 0; k < V; ++k) {
            a[k] = load(b0 + k);
            lane_sum = Op::compose(lane_sum, a[k]);
        }
        T total;
        T before = Op::compose(run, block_scan_excl<Op>(lane_sum, s_wave, &total));
#pragma unroll
        for (int k = 0; k < V; ++k) {
            if (b0 + k < nagg) store(b0 + k, before);
            before = Op::compose(before, a[k]);
        }
        run = Op::compose(run, total);
        __syncthreads();  // the next round rewrites s_wave
    }
    return run;
}

// ---- streams ----
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

// Entry x (0 .. ns) of stream_first breaks its contract: [0] == 0, ascending, [ns] == n.
__device__ __forceinline__ bool stream_first_bad(const uint32_t* __restrict__ first, uint32_t ns, uint32_t n,
                                                 uint32_t x)
{
    if (!first || x > ns) return false;
    const uint32_t v = first[x];
    return (x == 0 && v != 0u) || (x == ns && v != n) || (x < ns && v > first[x + 1]);
}

// The streams of a lane's `count` consecutive frames from i0 < n on: two
// searches for the lane, one per frame only where they differ.
struct FrameStream {
    uint32_t s;
    bool first, last;  // of its stream s
};
struct LaneStreams {
    const uint32_t* first;
    uint32_t ns, n, s_lo, s_hi;
    __device__ __forceinline__ LaneStreams(const uint32_t* __restrict__ first_, uint32_t ns_, uint32_t n_, uint32_t i0,
                                           uint32_t count)
        : first(first_), ns(ns_), n(n_)
    {
        const uint32_t ilast = i0 + count - 1 < n ? i0 + count - 1 : n - 1;
        s_lo = stream_of(first, ns, i0), s_hi = stream_of(first, ns, ilast);
    }
    __device__ __forceinline__ FrameStream at(uint32_t i) const  // i: one of the lane's frames, below n
    {
        const uint32_t s = s_lo == s_hi ? s_lo : stream_of(first, ns, i);
        return FrameStream{s, stream_begin(first, s) == i, i + 1u == stream_end(first, n, s)};
    }
};

// The argument checks every per-stream entry makes on its streams and
// workspace, in this order: n and n_streams below 2^31; ptrs_ok for a batch
// with frames; a and b (either may be null) 16-byte aligned; one stream, or
// stream_first and at least one (all KMWS_ERR_INVALID_PARAM); `have` workspace
// bytes against `need` (KMWS_ERR_BUFFER_TOO_SMALL); a gfx950 device
// (KMWS_ERR_NOT_SUPPORTED).  Defined in kmws_utf8.hip.
kmws_status stream_args_check(bool ptrs_ok, const void* a, const void* b, uint32_t n, const uint32_t* stream_first,
                              uint32_t n_streams, size_t need, size_t have);

}  // namespace kmws
