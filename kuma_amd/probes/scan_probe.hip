// Test-only probes of the segmented-scan core (kuma_amd/csrc/kmws_stream_scan.hpp),
// built into libkmws_scan_probe.so by kuma_amd/build.py: build_test_variants()
// and loaded by tests/test_gpu_scan_core.py.  The product library never sees
// this file.
//
// The product monoids absorb what a scan gets wrong: a stream's first frame
// turns everything in front of it into a constant.  The two Ops here do the
// opposite.  An element is a half-open interval of indices; a, then b is an
// interval again only where a ends at b's start, and anything else (a dropped
// prefix, a swapped order, an element taken twice) sets a flag that no later
// compose clears.  The identity is a value of its own.
//   IntervalOp: a struct with a 64-bit field, moved field by field as MsgSumOp is;
//   WordOp:     the same in one word over ScanWordOp, 16 + 16 bits.
// One kernel per core function; each stores everything every lane saw.
#include "kmws_common.hpp"
#include "kmws_stream_scan.hpp"

namespace kmws {

struct Interval {  // 24 bytes; tests/test_gpu_scan_core.py: INTERVAL
    uint32_t lo, hi, ident, broken;
    uint64_t count;
};
static_assert(sizeof(Interval) == 24, "the layout the tests read");

struct IntervalOp {
    using T = Interval;
    static __device__ __forceinline__ T identity() { return T{0xFFFFFFFFu, 0xFFFFFFFFu, 1u, 0u, 0u}; }
    static __device__ __forceinline__ T compose(const T& a, const T& b)
    {
        if (a.ident) return b;
        if (b.ident) return a;
        return T{a.lo, b.hi, 0u, a.broken | b.broken | (a.hi != b.lo ? 1u : 0u), a.count + b.count};
    }
    static __device__ __forceinline__ T shfl_up(const T& v, int dlt)
    {
        T r;
        r.lo = __shfl_up(v.lo, dlt), r.hi = __shfl_up(v.hi, dlt);
        r.ident = __shfl_up(v.ident, dlt), r.broken = __shfl_up(v.broken, dlt);
        r.count = __shfl_up((unsigned long long)v.count, dlt);
        return r;
    }
    static __device__ __forceinline__ T load(const T* p) { return T{p->lo, p->hi, p->ident, p->broken, p->count}; }
    static __device__ __forceinline__ void store(T* p, const T& v)
    {
        p->lo = v.lo, p->hi = v.hi, p->ident = v.ident, p->broken = v.broken, p->count = v.count;
    }
};

// lo in bits 0-15, hi in bits 16-31; two words that are no interval of the tests.
constexpr uint32_t kWordIdentity = 0xFFFFFFFFu, kWordPoison = 0xFFFEFFFEu;
struct WordOp : ScanWordOp {
    static __device__ __forceinline__ T identity() { return kWordIdentity; }
    static __device__ __forceinline__ T compose(T a, T b)
    {
        if (a == kWordIdentity) return b;
        if (b == kWordIdentity) return a;
        if (a == kWordPoison || b == kWordPoison || (a >> 16) != (b & 0xFFFFu)) return kWordPoison;
        return (a & 0xFFFFu) | (b & 0xFFFF0000u);
    }
};

// scan_aggregates by one block.  bits[b] rides beside aggregate b as the status
// bits of the product callers do: ORed into a lane variable by the load callback,
// reduced over the block at the end.  total[t]: what lane t got back.
template <class Op>
__global__ void __launch_bounds__(kBlock) probe_scan_aggs_kernel(const typename Op::T* __restrict__ aggs,
                                                                 const uint32_t* __restrict__ bits, uint32_t nagg,
                                                                 typename Op::T* __restrict__ pre,
                                                                 typename Op::T* __restrict__ total,
                                                                 uint32_t* __restrict__ status)
{
    using T = typename Op::T;
    __shared__ T s_wave[kScanWaves];
    uint32_t seen = 0;
    const auto load = [&](uint32_t b) {
        if (b >= nagg) return Op::identity();
        seen |= bits[b];
        return Op::load(&aggs[b]);
    };
    const T run = scan_aggregates<Op>(nagg, s_wave, load, [&](uint32_t b, const T& p) { Op::store(&pre[b], p); });
    Op::store(&total[threadIdx.x], run);
    const int any = __syncthreads_or((int)seen);
    if (threadIdx.x == 0) *status = any ? 1u : 0u;
}

// block_scan_excl: lane t of block B holds elems[B * kBlock + t]; its exclusive
// value and the total it was given go to the same index.
template <class Op>
__global__ void __launch_bounds__(kBlock) probe_block_scan_kernel(const typename Op::T* __restrict__ elems,
                                                                  typename Op::T* __restrict__ excl,
                                                                  typename Op::T* __restrict__ total)
{
    using T = typename Op::T;
    __shared__ T s_wave[kScanWaves];
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    T tot;
    const T e = block_scan_excl<Op>(Op::load(&elems[i]), s_wave, &tot);
    Op::store(&excl[i], e);
    Op::store(&total[i], tot);
}

// Four consecutive frames a lane, as kmws_proto_check and kmws_msg_index take
// them: per frame below n its stream by stream_of and by LaneStreams::at, and
// the first (bit 0) / last (bit 1) flags.
__global__ void __launch_bounds__(kBlock) probe_streams_kernel(const uint32_t* __restrict__ first, uint32_t ns,
                                                               uint32_t n, uint32_t* __restrict__ s_direct,
                                                               uint32_t* __restrict__ s_lane,
                                                               uint8_t* __restrict__ edges)
{
    const uint32_t i0 = (blockIdx.x * kBlock + threadIdx.x) * kScanFramesPerLane;
    if (i0 >= n) return;
    const LaneStreams streams(first, ns, n, i0, kScanFramesPerLane);
    for (uint32_t k = 0; k < kScanFramesPerLane; ++k) {
        const uint32_t i = i0 + k;
        if (i >= n) break;
        const FrameStream fs = streams.at(i);
        s_direct[i] = stream_of(first, ns, i);
        s_lane[i] = fs.s;
        edges[i] = (uint8_t)((fs.first ? 1u : 0u) | (fs.last ? 2u : 0u));
    }
}

// stream_first_bad for every x below count (the caller goes past ns).
__global__ void __launch_bounds__(kBlock) probe_first_bad_kernel(const uint32_t* __restrict__ first, uint32_t ns,
                                                                 uint32_t n, uint32_t count, uint8_t* __restrict__ bad)
{
    const uint32_t x0 = (blockIdx.x * kBlock + threadIdx.x) * kScanFramesPerLane;
    for (uint32_t k = 0; k < kScanFramesPerLane; ++k)
        if (x0 + k < count) bad[x0 + k] = stream_first_bad(first, ns, n, x0 + k) ? 1 : 0;
}

}  // namespace kmws

using namespace kmws;

extern "C" {

uint32_t kmws_probe_round(void) { return kScanBlockFrames; }
uint32_t kmws_probe_block(void) { return (uint32_t)kBlock; }

int kmws_probe_scan_aggs_interval(const void* aggs, const uint32_t* bits, uint32_t nagg, void* pre, void* total,
                                  uint32_t* status, void* stream)
{
    hipLaunchKernelGGL(probe_scan_aggs_kernel<IntervalOp>, dim3(1), dim3(kBlock), 0, static_cast<hipStream_t>(stream),
                       static_cast<const Interval*>(aggs), bits, nagg, static_cast<Interval*>(pre),
                       static_cast<Interval*>(total), status);
    return (int)hipGetLastError();
}

int kmws_probe_scan_aggs_word(const void* aggs, const uint32_t* bits, uint32_t nagg, void* pre, void* total,
                              uint32_t* status, void* stream)
{
    hipLaunchKernelGGL(probe_scan_aggs_kernel<WordOp>, dim3(1), dim3(kBlock), 0, static_cast<hipStream_t>(stream),
                       static_cast<const uint32_t*>(aggs), bits, nagg, static_cast<uint32_t*>(pre),
                       static_cast<uint32_t*>(total), status);
    return (int)hipGetLastError();
}

// elems, excl and total hold nblocks * 256 elements each.
int kmws_probe_block_scan_interval(const void* elems, uint32_t nblocks, void* excl, void* total, void* stream)
{
    hipLaunchKernelGGL(probe_block_scan_kernel<IntervalOp>, dim3(nblocks), dim3(kBlock), 0,
                       static_cast<hipStream_t>(stream), static_cast<const Interval*>(elems),
                       static_cast<Interval*>(excl), static_cast<Interval*>(total));
    return (int)hipGetLastError();
}

int kmws_probe_block_scan_word(const void* elems, uint32_t nblocks, void* excl, void* total, void* stream)
{
    hipLaunchKernelGGL(probe_block_scan_kernel<WordOp>, dim3(nblocks), dim3(kBlock), 0,
                       static_cast<hipStream_t>(stream), static_cast<const uint32_t*>(elems),
                       static_cast<uint32_t*>(excl), static_cast<uint32_t*>(total));
    return (int)hipGetLastError();
}

// first: ns + 1 entries or null (then ns == 1); the outputs hold n entries each.
int kmws_probe_streams(const uint32_t* first, uint32_t ns, uint32_t n, uint32_t* s_direct, uint32_t* s_lane,
                       uint8_t* edges, void* stream)
{
    if (n == 0 || ns == 0) return -1;
    hipLaunchKernelGGL(probe_streams_kernel, dim3((n + kScanBlockFrames - 1) / kScanBlockFrames), dim3(kBlock), 0,
                       static_cast<hipStream_t>(stream), first, ns, n, s_direct, s_lane, edges);
    return (int)hipGetLastError();
}

// first: ns + 1 entries or null; bad holds count entries.
int kmws_probe_first_bad(const uint32_t* first, uint32_t ns, uint32_t n, uint32_t count, uint8_t* bad, void* stream)
{
    if (count == 0) return -1;
    hipLaunchKernelGGL(probe_first_bad_kernel, dim3((count + kScanBlockFrames - 1) / kScanBlockFrames), dim3(kBlock), 0,
                       static_cast<hipStream_t>(stream), first, ns, n, count, bad);
    return (int)hipGetLastError();
}

}  // extern "C"
