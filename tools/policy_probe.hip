// Cache-policy probe for the unmask apply's stream on MI355X: the split-4
// in-place XOR of 16 KiB tiles, one 256-lane block per tile, 2 blocks resident
// per CU (the product's LDS pad), with buffer loads and stores whose cache
// policy is a template immediate.  Every load policy x every store policy,
// interleaved in one process over one allocation filled with random bytes.
// Stand-alone (no library): tools/membw_probe.hip's other modes need product
// entry points that no longer exist.
// `depth` mode: the same stream with the product's policies (nt loads, nt sc1
// stores) over pairs (B, D) -- B blocks resident per CU, D payload loads
// outstanding per lane: word i is waited for, load i + D issued, word i stored
// (D = 4: all loads up front, the policy mode's kernel) -- B x D x 4 KiB of
// payload in flight per CU.
//
// build: hipcc -x hip --offload-arch=gfx950 -O3 -std=c++17 tools/policy_probe.hip -o tools/policy_probe
// run:   tools/policy_probe [GiB = 64] [reps = 5]
//        tools/policy_probe depth [GiB = 64] [reps = 5]
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { \
    fprintf(stderr, "%s:%d %s\n", __FILE__, __LINE__, hipGetErrorString(e_)); exit(1); } } while (0)

constexpr int kB = 256, kV = 4;
constexpr uint32_t kTile = kB * kV * 16;
// buffer aux immediates on gfx950: bit 0 sc0, bit 1 nt, bit 4 sc1
constexpr int kPol[5] = {2, 18, 16, 17, 0};
static const char* const kPolName[5] = {"nt", "nt sc1", "sc1", "sc0 sc1", "plain"};

__device__ __forceinline__ uint64_t mix64(uint64_t x)
{
    uint64_t z = x + 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

__global__ void __launch_bounds__(256) fill_random(u32x4* p, uint64_t nw)
{
    for (uint64_t w = (uint64_t)blockIdx.x * 256 + threadIdx.x; w < nw; w += (uint64_t)gridDim.x * 256) {
        const uint64_t a = mix64(2 * w), b = mix64(2 * w + 1);
        p[w] = u32x4{(uint32_t)a, (uint32_t)(a >> 32), (uint32_t)b, (uint32_t)(b >> 32)};
    }
}

// block b takes tile (b mod 4) * (grid / 4) + b / 4; the grid is a multiple of 4
template <int LP, int SP>
__global__ void __launch_bounds__(kB) xor_split4(uint8_t* base, uint32_t c)
{
    const uint32_t q = gridDim.x >> 2;
    const uint64_t tile = (uint64_t)(blockIdx.x & 3u) * q + (blockIdx.x >> 2);
    const __amdgpu_buffer_rsrc_t rs =
        __builtin_amdgcn_make_buffer_rsrc(base + tile * kTile, (short)0, (int)kTile, 0x00020000);
    u32x4 v[kV];
#pragma unroll
    for (int i = 0; i < kV; ++i)
        v[i] = __builtin_amdgcn_raw_buffer_load_b128(rs, (int)(16u * (threadIdx.x + kB * i)), 0, LP);
#pragma unroll
    for (int i = 0; i < kV; ++i)
        __builtin_amdgcn_raw_buffer_store_b128(v[i] ^ c, rs, (int)(16u * (threadIdx.x + kB * i)), 0, SP);
}

// D loads outstanding per lane; the next load goes out ahead of the store (vmcnt
// is one in-order queue: a load issued behind a store waits for that store too)
template <int D>
__global__ void __launch_bounds__(kB) xor_split4_depth(uint8_t* base, uint32_t c)
{
    constexpr int LP = 2, SP = 18;  // nt loads, nt sc1 stores
    const uint32_t q = gridDim.x >> 2;
    const uint64_t tile = (uint64_t)(blockIdx.x & 3u) * q + (blockIdx.x >> 2);
    const __amdgpu_buffer_rsrc_t rs =
        __builtin_amdgcn_make_buffer_rsrc(base + tile * kTile, (short)0, (int)kTile, 0x00020000);
    u32x4 v[kV];
#pragma unroll
    for (int i = 0; i < D; ++i)
        v[i] = __builtin_amdgcn_raw_buffer_load_b128(rs, (int)(16u * (threadIdx.x + kB * i)), 0, LP);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int i = 0; i < kV; ++i) {
        const u32x4 w = v[i] ^ c;
        __builtin_amdgcn_sched_barrier(0);
        if (i + D < kV)
            v[i + D] = __builtin_amdgcn_raw_buffer_load_b128(rs, (int)(16u * (threadIdx.x + kB * (i + D))), 0, LP);
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_raw_buffer_store_b128(w, rs, (int)(16u * (threadIdx.x + kB * i)), 0, SP);
        __builtin_amdgcn_sched_barrier(0);
    }
}

static void launch_depth(int d, uint8_t* buf, uint32_t grid, unsigned pad)
{
    switch (d) {
    case 1: hipLaunchKernelGGL(xor_split4_depth<1>, dim3(grid), dim3(kB), pad, 0, buf, 0x5a5a5a5au); break;
    case 2: hipLaunchKernelGGL(xor_split4_depth<2>, dim3(grid), dim3(kB), pad, 0, buf, 0x5a5a5a5au); break;
    case 3: hipLaunchKernelGGL(xor_split4_depth<3>, dim3(grid), dim3(kB), pad, 0, buf, 0x5a5a5a5au); break;
    default: hipLaunchKernelGGL(xor_split4_depth<4>, dim3(grid), dim3(kB), pad, 0, buf, 0x5a5a5a5au); break;
    }
}

// (blocks per CU, loads outstanding per lane), interleaved like the policies
static int depth_mode(uint8_t* buf, uint64_t bytes, uint32_t tiles, int lds, int reps)
{
    static const int kPairs[][2] = {{2, 4}, {2, 3}, {3, 2}, {6, 1}, {5, 1}, {7, 1}, {4, 2}, {8, 1}, {3, 3}, {5, 2}};
    constexpr int kN = sizeof(kPairs) / sizeof(kPairs[0]);
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0));
    CK(hipEventCreate(&e1));
    std::vector<float> ms[kN];
    for (int r = 0; r < reps + 1; ++r)
        for (int p = 0; p < kN; ++p) {
            const unsigned pad = (unsigned)lds / (kPairs[p][0] + 1) + 1;  // one more block does not fit
            CK(hipEventRecord(e0, 0));
            launch_depth(kPairs[p][1], buf, tiles, pad);
            CK(hipEventRecord(e1, 0));
            CK(hipEventSynchronize(e1));
            CK(hipGetLastError());
            float t = 0;
            CK(hipEventElapsedTime(&t, e0, e1));
            if (r > 0) ms[p].push_back(t);  // round 0 warms up
        }
    printf("split-4 in-place XOR, %.1f GiB, random fill, nt loads, nt sc1 stores, %d reps; share of 8 TB/s\n",
           bytes / 1073741824.0, reps);
    for (int p = 0; p < kN; ++p) {
        std::vector<float> v = ms[p];
        std::sort(v.begin(), v.end());
        const double med = v[v.size() / 2];
        printf("blocks/CU %d depth %d (%2d KiB/CU) median %8.3f ms  best %8.3f  worst %8.3f  -> %.4f\n", kPairs[p][0],
               kPairs[p][1], 4 * kPairs[p][0] * kPairs[p][1], med, v.front(), v.back(),
               2.0 * bytes / (med * 1e-3) / 8e12);
    }
    return 0;
}

template <int L, int S>
static void launch(uint8_t* buf, uint32_t grid, unsigned pad)
{
    hipLaunchKernelGGL((xor_split4<kPol[L], kPol[S]>), dim3(grid), dim3(kB), pad, 0, buf, 0x5a5a5a5au);
}

template <int L>
static void launch_s(int s, uint8_t* buf, uint32_t grid, unsigned pad)
{
    switch (s) {
    case 0: launch<L, 0>(buf, grid, pad); break;
    case 1: launch<L, 1>(buf, grid, pad); break;
    case 2: launch<L, 2>(buf, grid, pad); break;
    case 3: launch<L, 3>(buf, grid, pad); break;
    default: launch<L, 4>(buf, grid, pad); break;
    }
}

static void launch_ls(int l, int s, uint8_t* buf, uint32_t grid, unsigned pad)
{
    switch (l) {
    case 0: launch_s<0>(s, buf, grid, pad); break;
    case 1: launch_s<1>(s, buf, grid, pad); break;
    case 2: launch_s<2>(s, buf, grid, pad); break;
    case 3: launch_s<3>(s, buf, grid, pad); break;
    default: launch_s<4>(s, buf, grid, pad); break;
    }
}

int main(int argc, char** argv)
{
    const bool depth = argc > 1 && strcmp(argv[1], "depth") == 0;
    if (depth) --argc, ++argv;
    const uint64_t bytes = (argc > 1 ? strtoull(argv[1], 0, 0) : 64ull) << 30;
    const int reps = argc > 2 ? atoi(argv[2]) : 5;
    const uint64_t tiles = bytes / kTile;
    if (tiles == 0 || (tiles & 3) || tiles > 0x7FFFFFFFull) {
        fprintf(stderr, "size must be a positive multiple of 64 KiB below 32 TiB\n");
        return 1;
    }
    uint8_t* buf = nullptr;
    CK(hipMalloc(&buf, bytes));
    hipLaunchKernelGGL(fill_random, dim3(8192), dim3(256), 0, 0, (u32x4*)buf, bytes / 16);
    CK(hipDeviceSynchronize());
    int lds = 0;
    CK(hipDeviceGetAttribute(&lds, hipDeviceAttributeMaxSharedMemoryPerMultiprocessor, 0));
    if (depth) return depth_mode(buf, bytes, (uint32_t)tiles, lds, reps);
    const unsigned pad = (unsigned)lds / 3 + 1;  // a third block does not fit: 2 per CU
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0));
    CK(hipEventCreate(&e1));
    std::vector<float> ms[5][5];
    for (int r = 0; r < reps + 1; ++r)
        for (int l = 0; l < 5; ++l)
            for (int s = 0; s < 5; ++s) {
                CK(hipEventRecord(e0, 0));
                launch_ls(l, s, buf, (uint32_t)tiles, pad);
                CK(hipEventRecord(e1, 0));
                CK(hipEventSynchronize(e1));
                CK(hipGetLastError());
                float t = 0;
                CK(hipEventElapsedTime(&t, e0, e1));
                if (r > 0) ms[l][s].push_back(t);  // round 0 warms up
            }
    printf("split-4 in-place XOR, %.1f GiB, random fill, 2 blocks/CU, %d reps; share of 8 TB/s (2 x buffer / time)\n",
           bytes / 1073741824.0, reps);
    for (int l = 0; l < 5; ++l)
        for (int s = 0; s < 5; ++s) {
            std::vector<float> v = ms[l][s];
            std::sort(v.begin(), v.end());
            const double med = v[v.size() / 2];
            printf("loads %-8s stores %-8s median %8.3f ms  best %8.3f  worst %8.3f  -> %.4f\n", kPolName[l], kPolName[s],
                   med, v.front(), v.back(), 2.0 * bytes / (med * 1e-3) / 8e12);
        }
    return 0;
}
