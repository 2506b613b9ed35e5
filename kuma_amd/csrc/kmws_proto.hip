// RFC 6455 frame-sequence and CLOSE rules per stream for MI355X (gfx950):
// kmws_proto_check.  The rule is stated in kmws_proto_rule.hpp; this file is
// the segmented scan of it over a batch of many streams' frames.
//
// What a frame does to its stream's state (IDLE / OPEN / CLOSED / FAILED) is a
// function on four states packed in one byte, and a stream's first frame is
// composed behind the constant function of the carried state, so the state
// before every frame is a plain scan of bytes under proto_compose: the scan
// core of kmws_stream_scan.hpp with ProtoOp, four consecutive frames a lane.
// Three kernels:
//   1. proto_elem_kernel: a lane reads its frames' descriptors, flags and error
//      bytes, decides each frame's local class (a lane that owns a CLOSE frame
//      walks its at most 125 payload bytes serially: the other 63 lanes of its
//      wave wait, and CLOSE frames are at most one per connection), finds the
//      stream edges, scans the block and stores per frame the local class (with
//      the stream edge bits) and the block-inclusive function, per block the
//      aggregate.  Its lanes also check stream_first and the carries.  Status
//      bits do not go to the status word (no kernel has cleared it yet) but ride
//      above the block's aggregate;
//   2. proto_scan_aggs_kernel: scan_aggregates, and the status word's store:
//      cleared, or the OR of the blocks';
//   3. proto_finish_kernel: element-wise.  The state before frame i is the
//      block's prefix composed with the inclusive value of frame i - 1 applied
//      to any state (a constant function since the stream's first frame), or the
//      carried state at a stream's first frame; out[i] from it, carry_out at a
//      stream's last frame, an empty stream's carry copied.
// Algorithmic bytes per frame: 16 + 2 (+ 1) read, 2 stored by kernel 1; 2 + 2
// read, 1 stored by kernel 3.  Vector stores and plain C++ only.
#include "kmws_common.hpp"
#include "kmws_proto_rule.hpp"
#include "kmws_stream_scan.hpp"
#include "kmws_workspace.hpp"

namespace kmws {

constexpr int kProtoV = (int)kScanFramesPerLane;
static_assert(kProtoV == 4, "a lane's frames are one 32-bit word of the per-frame arrays");
static_assert(kProtoBlockFrames == kScanBlockFrames, "the constant the tests read");

struct ProtoOp : ScanWordOp {  // one state function in a byte
    static __device__ __forceinline__ T identity() { return proto_identity(); }
    static __device__ __forceinline__ T compose(T a, T b) { return proto_compose(a, b); }
};

// The per-frame byte beside the local class (bits 0-3): the frame is its
// stream's first (its carried state in bits 4-5) / its stream's last.
constexpr uint32_t kProtoFirst = 0x40u, kProtoLast = 0x80u;

__device__ __forceinline__ uint32_t proto_load_carry(const kmws_proto_carry* __restrict__ c, uint32_t s)
{
    return c ? c[s].b[0] : 0u;
}
// kmws_proto_carry has byte alignment: written byte by byte.
__device__ __forceinline__ void proto_store_carry(kmws_proto_carry* __restrict__ c, uint32_t s, uint32_t state)
{
    c[s].b[0] = (uint8_t)state;
    for (int k = 1; k < 8; ++k) c[s].b[k] = (uint8_t)0;
}

__global__ void __launch_bounds__(kBlock) proto_elem_kernel(const uint8_t* __restrict__ base, uint64_t span,
                                                            const kmws_desc* __restrict__ d,
                                                            const uint16_t* __restrict__ flags,
                                                            const uint8_t* __restrict__ err, uint32_t n, int masked,
                                                            uint32_t rsv_allowed, const uint32_t* __restrict__ first,
                                                            uint32_t ns, const kmws_proto_carry* __restrict__ carry_in,
                                                            uint8_t* __restrict__ local_out,
                                                            uint8_t* __restrict__ incl_out,
                                                            uint16_t* __restrict__ aggs, uint32_t nblk)
{
    __shared__ uint32_t s_wave[kScanWaves];
    const uint32_t i0 = (blockIdx.x * kBlock + threadIdx.x) * kProtoV;
    bool bad_args = false;
#pragma unroll
    for (int k = 0; k < kProtoV; ++k) {
        const uint32_t x = i0 + k;
        bad_args |= stream_first_bad(first, ns, n, x);
        if (x < ns) bad_args |= proto_load_carry(carry_in, x) > kProtoFailed;
    }

    uint32_t inc[kProtoV];  // the lane's frames, scanned: inc[k] = frames 0..k
    uint32_t lw = 0;
#pragma unroll
    for (int k = 0; k < kProtoV; ++k) inc[k] = proto_identity();
    if (i0 < n) {
        const LaneStreams streams(first, ns, n, i0, kProtoV);
#pragma unroll
        for (int k = 0; k < kProtoV; ++k) {
            const uint32_t i = i0 + k;
            if (i >= n) break;
            const kmws_desc df = d[i];
            const uint32_t b0 = flags[i] & 0xFFu, e = err ? err[i] : 0u;
            uint32_t local = proto_local_head(b0, df.len, e, rsv_allowed);
            if (e == 0u && proto_needs_body(b0, df.len) && df.len <= 125u) {
                if (df.off > span || df.off + (uint64_t)df.len > span)
                    bad_args = true;  // never read outside the span
                else if (local == 0u)
                    local = proto_close_body(base + df.off, df.len, masked ? df.key : 0u);
            }
            uint32_t f = proto_frame_fn(local, b0);
            const FrameStream fs = streams.at(i);
            if (fs.first) {
                const uint32_t c = proto_load_carry(carry_in, fs.s) & 3u;
                f = proto_compose(proto_const(c), f);
                local |= kProtoFirst | (c << 4);
            }
            if (fs.last) local |= kProtoLast;
            lw |= local << (8 * k);
            inc[k] = k ? proto_compose(inc[k - 1], f) : f;
        }
#pragma unroll
        for (int k = 1; k < kProtoV; ++k)
            if (i0 + k >= n) inc[k] = inc[k - 1];
    }
    uint32_t total;
    const uint32_t excl = block_scan_excl<ProtoOp>(inc[kProtoV - 1], s_wave, &total);
    if (blockIdx.x < nblk) {  // whole blocks in the workspace: no test against n
        uint32_t iw = 0;
#pragma unroll
        for (int k = 0; k < kProtoV; ++k) iw |= proto_compose(excl, inc[k]) << (8 * k);
        *reinterpret_cast<uint32_t*>(local_out + i0) = lw;
        *reinterpret_cast<uint32_t*>(incl_out + i0) = iw;
    }
    const int any_bad = __syncthreads_or(bad_args ? 1 : 0);
    if (threadIdx.x == 0) aggs[blockIdx.x] = (uint16_t)(total | (any_bad ? kStatusBadDesc << 8 : 0u));
}

// pre[b] = the composition of aggs[0 .. b); the status word = the OR of the
// blocks' status bits, stored (so cleared when there are none).
__global__ void __launch_bounds__(kBlock) proto_scan_aggs_kernel(const uint16_t* __restrict__ aggs,
                                                                 uint8_t* __restrict__ pre, uint32_t nagg,
                                                                 WsHead* __restrict__ head)
{
    __shared__ uint32_t s_wave[kScanWaves];
    uint32_t status = 0;
    const auto load = [&](uint32_t b) {
        const uint32_t a = b < nagg ? aggs[b] : proto_identity();
        status |= a >> 8;
        return a & 0xFFu;
    };
    scan_aggregates<ProtoOp>(nagg, s_wave, load, [&](uint32_t b, uint32_t p) { pre[b] = (uint8_t)p; });
    const int any_bad = __syncthreads_or((int)(status & kStatusBadDesc));
    if (threadIdx.x == 0) head->status = any_bad ? kStatusBadDesc : 0u;
}

__global__ void __launch_bounds__(kBlock) proto_finish_kernel(const uint16_t* __restrict__ flags, uint32_t n,
                                                              const uint32_t* __restrict__ first, uint32_t ns,
                                                              const kmws_proto_carry* __restrict__ carry_in,
                                                              kmws_proto_carry* __restrict__ carry_out,
                                                              const uint8_t* __restrict__ local_in,
                                                              const uint8_t* __restrict__ incl_in,
                                                              const uint8_t* __restrict__ pre, uint8_t* __restrict__ out)
{
    const uint32_t i0 = (blockIdx.x * kBlock + threadIdx.x) * kProtoV;
    if (i0 < n) {
        const uint32_t lw = *reinterpret_cast<const uint32_t*>(local_in + i0);
        const uint32_t iw = *reinterpret_cast<const uint32_t*>(incl_in + i0);
        const uint32_t p = pre[blockIdx.x];
        // everything before the lane's first frame; a constant function unless that frame starts the batch
        uint32_t fn = threadIdx.x ? proto_compose(p, incl_in[i0 - 1]) : p;
        uint32_t ow = 0;
#pragma unroll
        for (int k = 0; k < kProtoV; ++k) {
            const uint32_t i = i0 + k;
            if (i >= n) break;
            const uint32_t lb = (lw >> (8 * k)) & 0xFFu;
            const uint32_t before = (lb & kProtoFirst) ? (lb >> 4) & 3u : proto_apply(fn, kProtoIdle);
            ow |= proto_verdict(before, lb & 15u, flags[i] & 0xFFu) << (8 * k);
            fn = proto_compose(p, (iw >> (8 * k)) & 0xFFu);
            if (carry_out && (lb & kProtoLast)) proto_store_carry(carry_out, stream_of(first, ns, i), proto_apply(fn, kProtoIdle));
        }
        if (i0 + kProtoV <= n && (reinterpret_cast<uintptr_t>(out + i0) & 3u) == 0u) {
            *reinterpret_cast<uint32_t*>(out + i0) = ow;
        } else {
#pragma unroll
            for (int k = 0; k < kProtoV; ++k)
                if (i0 + k < n) out[i0 + k] = (uint8_t)(ow >> (8 * k));
        }
    }
    if (carry_out) {
#pragma unroll
        for (int k = 0; k < kProtoV; ++k) {
            const uint32_t s = i0 + k;  // an empty stream keeps its carry
            if (s < ns && stream_begin(first, s) >= stream_end(first, n, s))
                proto_store_carry(carry_out, s, proto_load_carry(carry_in, s));
        }
    }
}

__global__ void __launch_bounds__(kBlock) proto_carry_copy_kernel(uint32_t ns,
                                                                  const kmws_proto_carry* __restrict__ carry_in,
                                                                  kmws_proto_carry* __restrict__ carry_out)
{
    const uint32_t s = blockIdx.x * kBlock + threadIdx.x;
    if (s < ns) proto_store_carry(carry_out, s, proto_load_carry(carry_in, s));
}

}  // namespace kmws

using namespace kmws;

extern "C" {

size_t kmws_proto_workspace_size(uint32_t n, uint32_t n_streams) { return proto_ws(n, n_streams).total; }

kmws_status kmws_proto_check(const uint8_t* base, uint64_t span, const kmws_desc* descs, const uint16_t* flags,
                             const uint8_t* err, uint32_t n, int payload_masked, uint32_t rsv_allowed,
                             const uint32_t* stream_first, uint32_t n_streams, const kmws_proto_carry* carry_in,
                             kmws_proto_carry* carry_out, uint8_t* out, void* workspace, size_t workspace_bytes,
                             void* stream)
{
    if (rsv_allowed & ~0x70u) return KMWS_ERR_INVALID_PARAM;
    const ProtoWs w = proto_ws(n, n_streams);
    const kmws_status st = stream_args_check(base && descs && flags && out && workspace, base, nullptr, n,
                                             stream_first, n_streams, n ? w.total : 0, workspace_bytes);
    if (st != KMWS_OK) return st;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (n == 0) {  // every stream's state passes through
        if (carry_out && n_streams)
            hipLaunchKernelGGL(proto_carry_copy_kernel, dim3((n_streams + kBlock - 1) / kBlock), dim3(kBlock), 0, s,
                               n_streams, carry_in, carry_out);
        return hip_status(hipGetLastError());
    }
    note_device_batch(20ull * n, s);

    uint16_t* aggs = at<uint16_t>(workspace, w.aggs);
    uint8_t* pre = at<uint8_t>(workspace, w.pre);
    uint8_t* local = at<uint8_t>(workspace, w.local);
    uint8_t* incl = at<uint8_t>(workspace, w.incl);
    const uint32_t nagg = w.first_pass(stream_first);
    hipLaunchKernelGGL(proto_elem_kernel, dim3(nagg), dim3(kBlock), 0, s, base, span, descs, flags, err, n,
                       payload_masked != 0, rsv_allowed, stream_first, n_streams, carry_in, local, incl, aggs, w.nblk);
    hipLaunchKernelGGL(proto_scan_aggs_kernel, dim3(1), dim3(kBlock), 0, s, aggs, pre, nagg, at<WsHead>(workspace, 0));
    const uint32_t sblk = (uint32_t)ceil_div(n_streams, kScanBlockFrames);
    hipLaunchKernelGGL(proto_finish_kernel, dim3(carry_out && sblk > w.nblk ? sblk : w.nblk), dim3(kBlock), 0, s, flags,
                       n, stream_first, n_streams, carry_in, carry_out, local, incl, pre, out);
    return hip_status(hipGetLastError());
}

}  // extern "C"
