// Host check of kuma_amd/csrc/kmws_workspace.hpp: every workspace layout over
// a sweep of frame counts, mean regions (both copy forms), spans and stream
// counts.  Per point: every region starts at the alignment its element needs,
// lies inside `total`, holds count x element size bytes for the count the
// launchers run over, overlaps no other region (the edge-word area and the
// chunk map share their offset, and only one of them is live), nothing wraps
// in 64 bits, and a composed layout's prefix is the layout it is composed from.
// Build: hipcc -x hip --offload-host-only (tests/test_workspace_layout.py).
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "kmws_workspace.hpp"

using namespace kmws;

static int g_fail = 0;
static long g_cases = 0;
#define CHECK(cond)                                                                   \
    do {                                                                              \
        if (!(cond) && g_fail++ < 10) fprintf(stderr, "FAIL line %d: %s\n", __LINE__, #cond); \
    } while (0)

struct Region {
    const char* name;
    uint64_t off, count, elem, align;
};

static void check_regions(const std::vector<Region>& rs, uint64_t total)
{
    for (const Region& r : rs) {
        CHECK(r.off % r.align == 0);
        CHECK(r.count <= ~0ull / r.elem);  // count x element size does not wrap
        const uint64_t bytes = r.count * r.elem;
        CHECK(r.off + bytes >= r.off && r.off + bytes <= total);
        if (g_fail && g_fail < 10) fprintf(stderr, "  region %s off %llu count %llu total %llu\n", r.name,
                                           (unsigned long long)r.off, (unsigned long long)r.count,
                                           (unsigned long long)total);
    }
    for (size_t i = 0; i < rs.size(); ++i)
        for (size_t j = i + 1; j < rs.size(); ++j) {
            const uint64_t bi = rs[i].count * rs[i].elem, bj = rs[j].count * rs[j].elem;
            if (bi == 0 || bj == 0) continue;  // an empty region overlaps nothing
            CHECK(rs[i].off + bi <= rs[j].off || rs[j].off + bj <= rs[i].off);
        }
}

static const Region kHead{"head", 0, 1, sizeof(WsHead), 16};

static bool same(const PlanWs& a, const PlanWs& b)
{
    return a.ntiles == b.ntiles && a.map == b.map && a.map_count == b.map_count && a.total == b.total;
}
static bool same(const FrameArraysWs& a, const FrameArraysWs& b)
{
    return a.first_bad == b.first_bad && a.elems == b.elems && a.aggs == b.aggs && a.pre == b.pre &&
           a.carry == b.carry && a.total == b.total && a.n == b.n && a.nblk == b.nblk && a.n_streams == b.n_streams;
}
static bool same(const CopyLayout& a, const CopyLayout& b)
{
    return a.nt == b.nt && a.nrows == b.nrows && a.chunks == b.chunks && a.tiles == b.tiles && a.totals == b.totals &&
           a.rows == b.rows && a.states == b.states && a.zero_words == b.zero_words && a.edge == b.edge &&
           a.rec == b.rec && a.max_units == b.max_units && a.cmap == b.cmap && a.dense == b.dense &&
           a.n_chunks == b.n_chunks && a.total == b.total;
}

static void add_plan(std::vector<Region>& rs, const PlanWs& w, uint64_t span)
{
    CHECK(w.ntiles == span / kPlanTile + (span % kPlanTile != 0));
    CHECK(w.map_count == w.ntiles + 1);  // the sentinel
    rs.push_back({"tile records", w.map, w.map_count, sizeof(TileRec), alignof(TileRec)});
}
static void add_frame_arrays(std::vector<Region>& rs, const FrameArraysWs& w, uint64_t front, uint32_t n,
                             uint32_t n_streams)
{
    CHECK(w.first_bad >= front && w.n == n && w.n_streams == n_streams);
    CHECK(w.nblk == n / kBlock + (n % kBlock != 0));
    rs.push_back({"first_bad", w.first_bad, n, 4, 4});
    rs.push_back({"elems / views", w.elems, n, kWsUtf8ElemBytes, 8});
    rs.push_back({"aggs", w.aggs, w.nblk, kWsUtf8ElemBytes, 8});
    rs.push_back({"pre", w.pre, w.nblk, kWsUtf8ElemBytes, 8});
    rs.push_back({"carry", w.carry, n_streams, kWsUtf8ElemBytes, 8});
}
static void add_copy(std::vector<Region>& rs, const CopyLayout& w, uint32_t n, uint64_t cap)
{
    CHECK(w.nt == (uint64_t)n / kWsScanTile + (n % kWsScanTile != 0));
    CHECK(w.nrows == (uint64_t)n / kBlock + (n % kBlock != 0));
    CHECK(w.chunks == (n != 0 && cap / n < kChunkFormBelow));
    rs.push_back({"tile prefixes + totals", w.tiles, (uint64_t)w.nt + 1, kWsV2Bytes, 16});
    rs.push_back({"row prefixes", w.rows, w.nrows, kWsV2Bytes, 16});
    CHECK(w.totals == w.tiles + (uint64_t)w.nt * kWsV2Bytes);
    // the one-pass front's tile states lie inside the row prefixes, and its
    // zeroing runs from the head through them without a gap
    CHECK(w.states == w.rows && w.states % 8 == 0 && (uint64_t)w.nt * 8 <= (uint64_t)w.nrows * kWsV2Bytes);
    CHECK(w.tiles == sizeof(WsHead) && w.rows == w.totals + kWsV2Bytes && w.zero_words * 8 == w.states + w.nt * 8ull);
    CHECK(w.cmap == w.edge);  // the alias: one form is live
    if (w.chunks) {
        CHECK(w.n_chunks == cap / kWsChunkBytes + (cap % kWsChunkBytes != 0) && w.max_units == 0);
        rs.push_back({"chunk map", w.cmap, w.n_chunks + 1, 4, 4});
        rs.push_back({"dense list", w.dense, w.n_chunks, 4, 4});
    } else {
        // a region of R bytes takes at most (4 ceil(R / 64) + 60 + 255) / 256 <= R / 4096 + 319 / 256
        // wave units (unit_bound, kmws_pack.hip); the regions sum to at most cap
        CHECK(w.max_units % (kBlock / 64) == 0 && w.n_chunks == 0);
        CHECK(w.max_units * 256 >= cap / 16 + 319ull * n);
        rs.push_back({"edge words", w.edge, (uint64_t)n * kWsEdgeWords, 16, 16});
        rs.push_back({"unit records", w.rec, w.max_units, kWsUnitRecBytes, 32});
    }
}

static const uint32_t kNs[] = {0, 1, 2, 255, 256, 257, 2047, 2048, 2049, 65536, (1u << 20) + 1, 0x7FFFFFFFu};
static const uint64_t kMeans[] = {0, 1, 300, 4104, 16383, 16384, 65550};
static const uint64_t kSpans[] = {0, 1, 16383, 16384, 16385, 1ull << 31, (1ull << 32) + 16400, 1ull << 40};

int main()
{
    for (uint64_t span : kSpans) {
        const PlanWs p = plan_ws(span);
        std::vector<Region> rs{kHead};
        add_plan(rs, p, span);
        check_regions(rs, p.total);
        ++g_cases;
        for (uint32_t n : kNs) {
            const uint32_t streams[] = {0, 1, 2, n + 1};
            for (uint32_t ns : streams) {
                const Utf8Ws u = utf8_ws(span, n, ns);
                std::vector<Region> ru{kHead};
                add_plan(ru, u.plan, span);
                add_frame_arrays(ru, u.fa, u.plan.total, n, ns);
                check_regions(ru, u.total);
                CHECK(same(u.plan, p) && same(u.fa, frame_arrays_ws(p.total, n, ns)) && u.total >= p.total);
                ++g_cases;

                const FusedWs f = fused_ws(span, n, ns);
                ru.push_back({"edges", f.edges, f.u.plan.ntiles, 4, 4});
                check_regions(ru, f.total);
                CHECK(same(f.u.plan, u.plan) && same(f.u.fa, u.fa) && f.u.total == u.total && f.edges >= u.total);
                ++g_cases;
            }
        }
    }
    for (uint32_t n : kNs) {
        for (uint64_t mean : kMeans) {
            const uint64_t cap = (uint64_t)n * mean;
            const CopyLayout c = copy_ws(n, cap);
            std::vector<Region> rc{kHead};
            add_copy(rc, c, n, cap);
            check_regions(rc, c.total);
            ++g_cases;

            const CopyFamilyWs re = reframe_ws(n, cap);
            std::vector<Region> rr = rc;
            rr.push_back({"outgoing flags", re.oflags, n, 2, 2});
            check_regions(rr, re.total);
            CHECK(same(re.copy, c) && re.oflags >= c.total);
            ++g_cases;

            const uint32_t streams[] = {0, 1, 2, n + 1};
            for (uint32_t ns : streams) {
                const CopyFamilyWs g = gather_utf8_ws(n, cap, ns);
                std::vector<Region> rg = rc;
                add_frame_arrays(rg, g.fa, c.total, n, ns);
                check_regions(rg, g.total);
                CHECK(same(g.copy, c) && g.total == g.fa.total);
                ++g_cases;

                const CopyFamilyWs x = reframe_utf8_ws(n, cap, ns);
                std::vector<Region> rx = rr;
                add_frame_arrays(rx, x.fa, re.total, n, ns);
                check_regions(rx, x.total);
                CHECK(same(x.copy, c) && x.oflags == re.oflags && x.total == x.fa.total);
                ++g_cases;
            }
        }
        const PackHeadersWs h = pack_headers_ws(n);
        CHECK(h.nt == (uint64_t)n / kWsScanTile + (n % kWsScanTile != 0) && h.nrows == (uint64_t)n / kBlock + (n % kBlock != 0));
        CHECK(h.total % 8 == 0);  // zeroed as 8-byte words
        check_regions({kHead, {"tile states", h.states, h.nt, 8, 8}}, h.total);
        ++g_cases;
    }
    if (g_fail) {
        fprintf(stderr, "%d checks failed\n", g_fail);
        return 1;
    }
    printf("OK %ld cases\n", g_cases);
    return 0;
}
