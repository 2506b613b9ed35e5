// Bench and test support of include/kmws_bench.h; kmws_arena_place times the unmask's own plan and apply.
#include "kmws_bench.h"
#include "kmws_common.hpp"
#include "kmws_unmask_tile.hpp"

namespace kmws {

// ---- synthetic fill: byte i = byte (i & 7) of splitmix64(seed + (i >> 3)) ----
__global__ void __launch_bounds__(kBlock) fill_synthetic_kernel(uint8_t* __restrict__ base, uint64_t bytes,
                                                                uint64_t seed)
{
    const uint64_t nw = bytes >> 4;
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    for (uint64_t w = (uint64_t)blockIdx.x * kBlock + threadIdx.x; w < nw; w += stride) {
        const uint64_t a = splitmix64(seed + 2 * w), b = splitmix64(seed + 2 * w + 1);
        *reinterpret_cast<u32x4*>(base + 16 * w) =
            u32x4{(uint32_t)a, (uint32_t)(a >> 32), (uint32_t)b, (uint32_t)(b >> 32)};
    }
    if (blockIdx.x == 0 && threadIdx.x < (bytes & 15)) {
        const uint64_t i = (nw << 4) + threadIdx.x;
        base[i] = (uint8_t)(splitmix64(seed + (i >> 3)) >> (8 * (i & 7)));
    }
}

__global__ void __launch_bounds__(kBlock) uniform_descs_kernel(kmws_desc* __restrict__ d, uint32_t n,
                                                               uint64_t stride, uint32_t len, uint64_t key_seed)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    kmws_desc x;
    x.off = (uint64_t)i * stride;
    x.len = len;
    x.key = (uint32_t)splitmix64(key_seed + i);
    d[i] = x;
}

// ---- independent checker: simple byte-wise restatement, not the product path ----
constexpr int kCheckBytes = 4096;  // bytes per checker block

__global__ void __launch_bounds__(kBlock) check_unmasked_kernel(const uint8_t* __restrict__ base, uint64_t bytes,
                                                                uint64_t seed, const kmws_desc* __restrict__ d,
                                                                uint32_t n, unsigned long long* mismatches)
{
    __shared__ uint32_t s_first;
    const uint64_t nblk = (bytes + kCheckBytes - 1) / kCheckBytes;
    unsigned long long bad = 0;
    for (uint64_t blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
    const uint64_t blk_lo = blk * kCheckBytes;
    __syncthreads();
    if (threadIdx.x == 0) {
        // first frame with off + len > blk_lo (binary search over sorted descs)
        uint32_t lo = 0, hi = n;
        while (lo < hi) {
            const uint32_t mid = (lo + hi) >> 1;
            if (d[mid].off + d[mid].len <= blk_lo) lo = mid + 1; else hi = mid;
        }
        s_first = lo;
    }
    __syncthreads();
    uint32_t f = s_first;
    const uint64_t p0 = blk_lo + 16u * threadIdx.x;
    for (int k = 0; k < 16; ++k) {
        const uint64_t p = p0 + k;
        if (p >= bytes) break;
        while (f < n && d[f].off + d[f].len <= p) ++f;
        uint8_t expect = (uint8_t)(splitmix64(seed + (p >> 3)) >> (8 * (p & 7)));
        if (f < n && d[f].off <= p) {
            const uint32_t key = d[f].key;
            expect ^= (uint8_t)(key >> (8 * ((p - d[f].off) & 3)));
        }
        bad += base[p] != expect;
    }
    }
    if (bad) atomicAdd(mismatches, bad);
}

}  // namespace kmws

using namespace kmws;

extern "C" {

void* kmws_arena_alloc(uint64_t bytes, int device, int* contiguous)
{
    if (contiguous) *contiguous = 0;
    if (bytes == 0) return nullptr;
    int prev = -1;
    if (hipGetDevice(&prev) != hipSuccess) return nullptr;
    if (device != prev && hipSetDevice(device) != hipSuccess) return nullptr;
    void* p = nullptr;
    if (hipExtMallocWithFlags(&p, bytes, hipDeviceMallocContiguous) == hipSuccess && p) {
        if (contiguous) *contiguous = 1;
    } else {
        (void)hipGetLastError();
        p = nullptr;
        if (hipMalloc(&p, bytes) != hipSuccess) {
            (void)hipGetLastError();
            p = nullptr;
        }
    }
    if (device != prev) (void)hipSetDevice(prev);
    return p;
}

void kmws_arena_free(void* p, int device)
{
    if (!p) return;
    int prev = -1;
    if (hipGetDevice(&prev) != hipSuccess) return;
    if (device != prev) (void)hipSetDevice(device);
    (void)hipFree(p);
    if (device != prev) (void)hipSetDevice(prev);
}

int64_t kmws_arena_place(uint8_t* arena, uint64_t arena_bytes, uint64_t span, uint64_t step, void* stream,
                         float* frac_out, uint32_t max_out)
{
    // Offsets 0, step, 2 step, ... with offset + span <= arena_bytes.  The probe
    // batch: uniform 64 KiB frames over the span (contents are whatever the arena
    // holds; XOR applied twice leaves them unchanged); an offset scores the better
    // of the split-4 and split-8 schedules (which one leads depends on the
    // placement, and kmws_unmask_autotune then picks among all).
    constexpr uint64_t kFrame = 65536;
    if (!arena || span == 0 || span > arena_bytes || step == 0 || (step & 15u) ||
        (reinterpret_cast<uintptr_t>(arena) & 15u) || span / kFrame > 0xFFFFFFFFull)
        return KMWS_ERR_INVALID_PARAM;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const uint32_t n = (uint32_t)((span + kFrame - 1) / kFrame);
    const size_t ws_bytes = kmws_unmask_workspace_size(span);
    kmws_desc* d = nullptr;
    void* ws = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    int64_t result = KMWS_ERR_FAILED;
    if (hipMalloc(reinterpret_cast<void**>(&d), (size_t)n * sizeof(kmws_desc)) != hipSuccess ||
        hipMalloc(&ws, ws_bytes) != hipSuccess || hipEventCreate(&e0) != hipSuccess ||
        hipEventCreate(&e1) != hipSuccess) {
        (void)hipGetLastError();
    } else {
        hipLaunchKernelGGL(uniform_descs_kernel, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, s, d, n, kFrame,
                           (uint32_t)kFrame, 0x706c6163ull);
        // the last frame ends at the span (uniform_descs gives every frame kFrame bytes)
        const uint32_t last_len = (uint32_t)(span - (uint64_t)(n - 1) * kFrame);
        kmws_status st = hip_status(hipMemcpyAsync(&d[n - 1].len, &last_len, sizeof(last_len),
                                                   hipMemcpyHostToDevice, s));
        if (st == KMWS_OK) st = hip_status(hipStreamSynchronize(s));
        float best = 1e30f;
        uint64_t pick = 0;
        uint32_t k = 0;
        for (uint64_t off = 0; st == KMWS_OK && off + span <= arena_bytes; off += step, ++k) {
            float t = 1e30f;
            for (int rep = 0; rep < 4 && st == KMWS_OK; ++rep) {  // min of two pairs per schedule
                st = launch_plan(span, d, n, ws, ws_bytes, s);
                if (st == KMWS_OK) st = hip_status(hipEventRecord(e0, s));
                Schedule sc;
                (void)decode_schedule((rep & 1 ? KMWS_SCHED_SPLIT8 : KMWS_SCHED_SPLIT4) | KMWS_SCHED_NT_STORES, &sc);
                for (int i = 0; i < 2 && st == KMWS_OK; ++i)
                    st = launch_apply(sc, arena + off, span, d, n, ws, ws_bytes, s);
                if (st == KMWS_OK) st = hip_status(hipEventRecord(e1, s));
                if (st == KMWS_OK) st = hip_status(hipEventSynchronize(e1));
                float ms = 0;
                if (st == KMWS_OK && hipEventElapsedTime(&ms, e0, e1) == hipSuccess && ms < t) t = ms;
            }
            if (st != KMWS_OK) break;
            // fraction of the 8 TB/s HBM peak: 2 passes x (2 span + 16 n) bytes
            if (frac_out && k < max_out) frac_out[k] = (float)(2.0 * (2.0 * span + 16.0 * n) / (t * 1e-3) / 8e12);
            if (t < best) {
                best = t;
                pick = off;
            }
        }
        uint32_t status = 0;
        if (st == KMWS_OK) st = hip_status(hipMemcpy(&status, ws, sizeof(status), hipMemcpyDeviceToHost));
        result = st != KMWS_OK ? (int64_t)st : (status != 0 ? (int64_t)KMWS_ERR_FAILED : (int64_t)pick);
    }
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    if (ws) (void)hipFree(ws);
    if (d) (void)hipFree(d);
    return result;
}

kmws_status kmws_fill_synthetic(uint8_t* base, uint64_t bytes, uint64_t seed, void* stream)
{
    if (!base && bytes) return KMWS_ERR_INVALID_PARAM;
    if ((reinterpret_cast<uintptr_t>(base) & 15u)) return KMWS_ERR_INVALID_PARAM;
    if (bytes == 0) return KMWS_OK;
    hipLaunchKernelGGL(fill_synthetic_kernel, dim3(8192), dim3(kBlock), 0, static_cast<hipStream_t>(stream), base,
                       bytes, seed);
    return hip_status(hipGetLastError());
}

kmws_status kmws_fill_uniform_descs(kmws_desc* descs, uint32_t n, uint64_t stride, uint32_t len,
                                    uint64_t key_seed, void* stream)
{
    if (!descs && n) return KMWS_ERR_INVALID_PARAM;
    if (n == 0) return KMWS_OK;
    hipLaunchKernelGGL(uniform_descs_kernel, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0,
                       static_cast<hipStream_t>(stream), descs, n, stride, len, key_seed);
    return hip_status(hipGetLastError());
}

kmws_status kmws_check_unmasked(const uint8_t* base, uint64_t bytes, uint64_t seed, const kmws_desc* descs,
                                uint32_t n, unsigned long long* mismatches, void* stream)
{
    if ((!base && bytes) || !mismatches) return KMWS_ERR_INVALID_PARAM;
    if (bytes == 0) return KMWS_OK;
    uint64_t nb = (bytes + kCheckBytes - 1) / kCheckBytes;
    if (nb > 65536) nb = 65536;  // grid-stride beyond this
    hipLaunchKernelGGL(check_unmasked_kernel, dim3((uint32_t)nb), dim3(kBlock), 0, static_cast<hipStream_t>(stream),
                       base, bytes, seed, descs, n, mismatches);
    return hip_status(hipGetLastError());
}

}  // extern "C"
