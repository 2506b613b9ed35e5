// Host check of kuma_amd/csrc/kmws_resident_proto.hpp: the resident worker's
// mailbox format -- the job word, job_done's half-range rule, the descriptor
// and verdict tags, hull_words, the split of a job over its parts and the
// edge-word pick -- at the values no GPU test reaches in its lifetime (40-bit
// job numbers, 16- and 11-bit tags wrapping) and against brute-force
// restatements.  The layouts are static_asserts of the header itself.
// Build: hipcc -x hip --offload-host-only (tests/test_resident_proto.py).
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "kmws_resident_proto.hpp"

using namespace kmws;

static int g_fail = 0;
static long g_cases = 0;
#define CHECK(cond)                                                                   \
    do {                                                                              \
        if (!(cond) && g_fail++ < 10) fprintf(stderr, "FAIL line %d: %s\n", __LINE__, #cond); \
    } while (0)

static const uint64_t kFlagBits[5] = {kWriteThroughBit, kCheckBit, kCancelBit, kClaimedBit, kQuitBit};

static void check_fields(uint64_t w, uint64_t job, uint32_t n, uint32_t parts, uint64_t flags)
{
    CHECK(job_number(w) == job && job_count(w) == n && job_parts(w) == parts);
    CHECK((job_write_through(w) != 0) == ((flags & kWriteThroughBit) != 0));
    CHECK((job_checked(w) != 0) == ((flags & kCheckBit) != 0));
    CHECK((job_cancelled(w) != 0) == ((flags & kCancelBit) != 0));
    CHECK((job_claimed(w) != 0) == ((flags & kClaimedBit) != 0));
    CHECK((job_quit(w) != 0) == ((flags & kQuitBit) != 0));
}

static void job_word()
{
    const uint64_t jobs[] = {0, 1, (1ull << 16) - 1, 1ull << 16, 1ull << 39, (1ull << 40) - 1};
    const uint32_t counts[] = {1, 31, 32, (uint32_t)kResMaxDescs};
    for (uint64_t job : jobs)
        for (uint32_t n : counts)
            for (uint32_t parts = 1; parts <= (uint32_t)kResParts; ++parts) {
                for (uint32_t m = 0; m < 32; ++m, ++g_cases) {
                    uint64_t flags = 0;
                    for (int b = 0; b < 5; ++b)
                        if (m >> b & 1u) flags |= kFlagBits[b];
                    check_fields(pack_job(job, n, parts, flags), job, n, parts, flags);
                }
                // the bits the host sets and clears on a posted word (claim, release, withdraw, quit)
                for (uint32_t m = 0; m < 4; ++m)
                    for (int b = 2; b < 5; ++b, ++g_cases) {
                        const uint64_t flags = (m & 1u ? kWriteThroughBit : 0) | (m & 2u ? kCheckBit : 0);
                        const uint64_t w = pack_job(job, n, parts, flags);
                        check_fields(w | kFlagBits[b], job, n, parts, flags | kFlagBits[b]);
                        check_fields((w | kFlagBits[b]) & ~kFlagBits[b], job, n, parts, flags);
                        CHECK(((w | kFlagBits[b]) & ~kFlagBits[b]) == w);
                    }
            }
}

static void done_rule()
{
    const uint64_t ss[] = {0, 1, 1ull << 39, (1ull << 40) - 1};
    const uint64_t half = 1ull << 39;
    for (uint64_t s : ss) {
        const uint64_t yes[] = {s, s + 1, s + half - 1}, no[] = {s - 1, s - half};
        for (uint64_t d : yes) { CHECK(job_done(d & kJobMask, s)); ++g_cases; }
        for (uint64_t d : no) { CHECK(!job_done(d & kJobMask, s)); ++g_cases; }
    }
}

static void tags()
{
    // s = 0, the tags' wrap-arounds (11 and 16 bits), low 16 bits zero, the job number's own wrap
    const uint64_t ss[] = {0, 1, 0x7FF, 0x800, 0xFFFF, 0x10000, 0x12340000, 1ull << 39, (1ull << 40) - 1};
    const uint64_t addrs[] = {0, (1ull << 48) - 16};
    const uint32_t lens[] = {0, 1, kLenMask};
    for (uint64_t s : ss) {
        const uint64_t before = (s - 1) & kJobMask;
        for (uint64_t addr : addrs) {
            for (uint32_t len : lens) {
                const ResDesc x{addr, len, 0xA55A1234u};
                const ResDesc t = tag_desc(x, s), old = tag_desc(x, before);
                CHECK(desc_tagged(t, s) && !desc_tagged(t, before) && !desc_tagged(old, s));
                // one half from the job before (the host writes the halves as two stores)
                CHECK(!desc_tagged(ResDesc{old.addr, t.len, t.key}, s));
                CHECK(!desc_tagged(ResDesc{t.addr, old.len, old.key}, s));
                const ResDesc u = untag_desc(t);
                CHECK(u.addr == x.addr && u.len == x.len && u.key == x.key);
                ++g_cases;
            }
            const uint64_t v = tag_verdict(addr, s), vold = tag_verdict(addr, before);
            CHECK(verdict_tagged(v, s) && !verdict_tagged(v, before) && !verdict_tagged(vold, s));
            CHECK(untag_verdict(v) == addr);
            ++g_cases;
        }
    }
}

static void hulls()
{
    for (uint64_t r = 0; r < 16; ++r)
        for (uint32_t len = 0; len < 50; ++len, ++g_cases) {
            const uint64_t addr = 0x7F0000001000ull + r;
            uint32_t words = 0;
            uint64_t last = ~0ull;
            for (uint64_t q = addr; q < addr + len; ++q)
                if ((q >> 4) != last) { last = q >> 4; ++words; }
            CHECK(hull_words(addr, len) == words);
        }
}

static void parts_split()
{
    const uint32_t round = (uint32_t)(kResBlock * kResWords);
    for (uint32_t total = 0; total <= 5u * 4096u; ++total, ++g_cases) {
        uint64_t want = total / kPartWords;
        if (want < 1) want = 1;
        if (want > (uint64_t)kResParts) want = kResParts;
        const uint32_t parts = part_count(total);
        CHECK(parts == want);
        uint32_t at = 0, largest = 0;
        for (uint32_t p = 0; p < parts; ++p) {
            const PartRange r = part_range(total, p, parts);
            CHECK(r.begin == at && r.end >= r.begin);
            if (r.end - r.begin > largest) largest = r.end - r.begin;
            at = r.end;
        }
        CHECK(at == total);
        if (checked_fits(total, parts)) CHECK(largest <= round);
        CHECK(checked_fits(total, parts) == (largest <= round));  // the largest part is the ceiling share
    }
}

// Every hull word of the job in order; the part's first word found by walking.
static void edge_job(const std::vector<ResDesc>& d)
{
    struct Word { int32_t index; uint32_t k; };
    std::vector<Word> walk;
    for (size_t i = 0; i < d.size(); ++i) {
        uint64_t last = ~0ull;
        uint32_t k = 0;
        for (uint64_t q = d[i].addr; q < d[i].addr + d[i].len; ++q)
            if ((q >> 4) != last) { last = q >> 4; walk.push_back(Word{(int32_t)i, k++}); }
    }
    const uint32_t total = (uint32_t)walk.size();
    for (uint32_t parts = 1; parts <= (uint32_t)kResParts; ++parts)
        for (uint32_t p = 0; p < parts; ++p) {
            const uint32_t wb = part_range(total, p, parts).begin;
            const EdgePick e = edge_pick(d.data(), (uint32_t)d.size(), total, p, parts);
            if (wb >= total || walk[wb].k == 0) CHECK(e.index < 0);  // (on a payload's first word: the view)
            else CHECK(e.index == walk[wb].index && e.offset == 16u * walk[wb].k - 4u);
        }
    ++g_cases;
}

static void edges()
{
    const uint64_t base = 0x7F0000100000ull;
    // one read of sixteen 4 KiB frames, 2-14 byte headers between them
    for (uint64_t b : {0ull, 3ull, 17ull}) {
        std::vector<ResDesc> d;
        uint64_t at = base + b;
        for (uint32_t i = 0; i < 16; ++i) {
            at += 2 + (i * 5) % 13;
            d.push_back(ResDesc{at, 4096, 0x01020304u * (i + 1)});
            at += 4096;
        }
        edge_job(d);
    }
    edge_job({ResDesc{base, 65536, 1}});
    uint64_t rng = 0x5EED;
    auto next = [&](uint64_t mod) { rng = splitmix64(rng); return rng % mod; };
    for (int j = 0; j < 300; ++j) {
        std::vector<ResDesc> d;
        uint64_t at = base + next(4096);
        const uint64_t n = 1 + next(32);
        for (uint64_t i = 0; i < n; ++i) {
            at += next(41);
            const uint32_t len = (uint32_t)next(9001);
            d.push_back(ResDesc{at, len, (uint32_t)next(1ull << 32)});
            at += len;
        }
        edge_job(d);
    }
    // parts that start on a payload's first hull word: none; inside one: the four bytes before
    const ResDesc two[] = {ResDesc{base, 16 * 2048, 1}, ResDesc{base + (1u << 20), 16 * 2048, 2}};
    CHECK(edge_pick(two, 2, 4096, 0, 4).index < 0 && edge_pick(two, 2, 4096, 2, 4).index < 0);
    const EdgePick in0 = edge_pick(two, 2, 4096, 1, 4), in1 = edge_pick(two, 2, 4096, 3, 4);
    CHECK(in0.index == 0 && in0.offset == 16 * 1024 - 4 && in1.index == 1 && in1.offset == 16 * 1024 - 4);
    ++g_cases;
}

int main()
{
    job_word();
    done_rule();
    tags();
    hulls();
    parts_split();
    edges();
    if (g_fail) {
        fprintf(stderr, "%d checks failed\n", g_fail);
        return 1;
    }
    printf("OK %ld cases\n", g_cases);
    return 0;
}
