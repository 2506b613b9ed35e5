// Host check of kmws::tile_of_block (kuma_amd/csrc/kmws_common.hpp), the
// block -> tile mapping of the unmask apply grid: for every placement kind and
// a list of whole-tile counts it must be a permutation of [0, nfull) and equal
// the division formulas it replaced, restated below as the reference.
// tests/test_tile_of_block.py builds and runs this (host code only).
#include <cstdint>
#include <cstdio>
#include <vector>

#include "kmws_common.hpp"

// The mapping as the apply kernel computed it with run-time divisions.
static uint32_t reference_tile(uint32_t b, uint32_t nfull, uint32_t k, uint32_t c, uint32_t w)
{
    uint32_t tile = b;
    if (c == 0) {
        const uint32_t q = nfull / k;
        if (b < q * k) tile = (b % k) * q + b / k;
    } else if (w <= 1) {
        const uint64_t run = (uint64_t)k * c;
        if (b < nfull / run * run) {
            const uint32_t x = b % k, i = b / k;
            tile = (i / c) * (uint32_t)run + x * c + i % c;
        }
    } else {
        const uint32_t kg = k / w;
        const uint64_t run = (uint64_t)kg * c;
        const uint64_t per = (uint64_t)nfull / w / run * run;
        if (b < per * w) {
            const uint32_t x = b % k, i = b / k;
            const uint32_t g = x % w, xi = x / w;
            tile = (uint32_t)(g * per) + (i / c) * (uint32_t)run + xi * c + i % c;
        }
    }
    return tile;
}

int main()
{
    const uint32_t sizes[] = {0, 1, 7, 8, 63, 64, 127, 128, 129, 131, 1000, 4099, 32768 + 7};
    // the (k, c, w) of each kind, restated from the parent's table
    const uint32_t want[6][3] = {{8, 16, 2}, {1, 0, 1}, {2, 0, 1}, {8, 0, 1}, {8, 16, 1}, {4, 0, 1}};
    unsigned long long checked = 0;
    int bad = 0;
    for (uint32_t kind = 0; kind < 6; ++kind) {
        kmws::Split sp;
        if (!kmws::split_of(kind, &sp) || sp.k != want[kind][0] || sp.c != want[kind][1] || sp.w != want[kind][2]) {
            std::printf("kind %u: split (%u, %u, %u)\n", kind, sp.k, sp.c, sp.w);
            return 1;
        }
        for (uint32_t nfull : sizes) {
            std::vector<uint8_t> seen(nfull, 0);
            for (uint32_t b = 0; b < nfull; ++b) {
                const uint32_t t = kmws::tile_of_block(b, nfull, sp);
                const uint32_t r = reference_tile(b, nfull, sp.k, sp.c, sp.w);
                if (t != r || t >= nfull || seen[t]) {
                    if (bad++ < 10)
                        std::printf("kind %u nfull %u block %u: tile %u, reference %u%s\n", kind, nfull, b, t, r,
                                    t < nfull && seen[t] ? " (taken twice)" : "");
                    continue;
                }
                seen[t] = 1;
                ++checked;
            }
        }
    }
    kmws::Split none;
    if (kmws::split_of(6, &none) || kmws::split_of(0xFF, &none)) {
        std::printf("kind 6 or 255 accepted\n");
        return 1;
    }
    if (bad) return 1;
    std::printf("OK %llu blocks\n", checked);
    return 0;
}
