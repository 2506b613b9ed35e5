// Host check of kuma_amd/csrc/kmws_msg_rule.hpp and the msg layout of
// kmws_workspace.hpp -- the very functions the kernels of kmws_msg.hip call:
//  1. msg_compose is associative over all triples of a small domain that holds
//     every kind of state function (keeps or sets the state byte to none or to
//     one of four open states; keeps, sets or clears `seen`), the identity and
//     the constants behave as such, and a composition applies like its parts;
//  2. msg_sum_compose is associative over random triples of canonical sums with
//     counts up to 2^28 and byte totals past 2^32, and msg_sum_identity is one;
//  3. every sequence of up to 6 frames over a boundary alphabet (data heads with
//     and without FIN, an RSV bit, a reserved opcode, CONTINUE with and without
//     FIN, control frames with and without payload, a length next to 2^32), from
//     each kind of carry (none, open, open with a total past 2^32): scan A by
//     msg_compose behind msg_const(carry), msg_class, scan B by msg_sum_compose,
//     the records taken at the reset points and at the end as the finish kernel
//     takes them, equal a sequential walk restated here; both scans' totals
//     are the same folded from the right;
//  4. the workspace layout: order, alignment, no overlap, bounds, monotone total.
// Prints "OK <count> cases".  Build: hipcc -x hip --offload-host-only
// (tests/test_msg_rule.py), once plain and once under ASan + UBSan.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "kmws_msg_rule.hpp"
#include "kmws_workspace.hpp"

using namespace kmws;

static int g_fail = 0;
static long g_cases = 0;
#define CHECK(cond)                                                                   \
    do {                                                                              \
        if (!(cond) && g_fail++ < 10) fprintf(stderr, "FAIL line %d: %s\n", __LINE__, #cond); \
    } while (0)

// ---- 1. scan A ----
static const uint32_t kStates[] = {0u, 0x81u, 0x82u, 0xC1u, 0xF7u};
static int state_domain(uint32_t* out)
{
    int n = 0;
    const uint32_t seen[] = {0u, kMsgSeenSet, kMsgSeenClear};
    for (uint32_t sn : seen) {
        out[n++] = sn;  // keeps the state
        for (uint32_t st : kStates) out[n++] = kMsgSet | st | sn;
    }
    return n;
}
static void check_state_monoid()
{
    uint32_t dom[32];
    const int n = state_domain(dom);
    CHECK(n == 18 && dom[0] == msg_identity());
    for (int a = 0; a < n; ++a) {
        CHECK(msg_compose(dom[a], msg_identity()) == dom[a] && msg_compose(msg_identity(), dom[a]) == dom[a]);
        for (uint32_t st : kStates) {
            CHECK(msg_compose(dom[a], msg_const(st)) == msg_const(st));  // a constant absorbs what is before it
            CHECK(msg_state_of(msg_const(st)) == st && !msg_seen_of(msg_const(st)));
        }
        for (int b = 0; b < n; ++b) {
            const uint32_t ab = msg_compose(dom[a], dom[b]);
            CHECK((ab & ~kMsgFnBits) == 0u);
            for (uint32_t st : kStates)
                for (int seen = 0; seen < 2; ++seen) {
                    CHECK(msg_apply_state(ab, st) == msg_apply_state(dom[b], msg_apply_state(dom[a], st)));
                    CHECK(msg_apply_seen(ab, seen != 0) == msg_apply_seen(dom[b], msg_apply_seen(dom[a], seen != 0)));
                }
            for (int c = 0; c < n; ++c) {
                CHECK(msg_compose(ab, dom[c]) == msg_compose(dom[a], msg_compose(dom[b], dom[c])));
                ++g_cases;
            }
        }
    }
    for (uint32_t b0 = 0; b0 < 256; ++b0) CHECK((msg_frame_fn(b0) & ~kMsgFnBits) == 0u);
}

// ---- 2. scan B ----
static uint64_t g_rng = 0x243F6A8885A308D3ull;
static uint64_t rnd()
{
    g_rng ^= g_rng << 13, g_rng ^= g_rng >> 7, g_rng ^= g_rng << 17;
    return g_rng;
}
static bool same(const MsgSum& a, const MsgSum& b)
{
    return a.starts == b.starts && a.first == b.first && a.last == b.last && a.frames == b.frames && a.bytes == b.bytes;
}
static MsgSum random_sum()
{
    MsgSum v = msg_sum_identity();
    const uint64_t r = rnd();
    if (r & 1) {  // holds a reset: maybe starts, maybe a running record that began at one
        v.starts = kMsgSumReset | (uint32_t)((r >> 8) % (1u << 28)) * (uint32_t)((r >> 1) & 1);
        if (msg_sum_starts(v) && (r & 4)) v.first = (uint32_t)(rnd() % 0x7FFFFFFFu);
    }
    if (r & 8) {  // holds members
        v.frames = (1u + (uint32_t)((r >> 40) % (1u << 28))) | ((r & 16) ? kMsgSumFin : 0u);
        v.last = (uint32_t)(rnd() % 0x7FFFFFFFu);
        v.bytes = rnd() >> ((r >> 5) & 1 ? 20 : 40);  // up to 2^44
    }
    return v;
}
static void check_sum_monoid()
{
    bool past32 = false;
    for (int t = 0; t < 200000; ++t) {
        const MsgSum a = random_sum(), b = random_sum(), c = random_sum();
        CHECK(same(msg_sum_compose(msg_sum_compose(a, b), c), msg_sum_compose(a, msg_sum_compose(b, c))));
        CHECK(same(msg_sum_compose(a, msg_sum_identity()), a) && same(msg_sum_compose(msg_sum_identity(), a), a));
        past32 |= msg_sum_compose(a, b).bytes > 0xFFFFFFFFull;
        ++g_cases;
    }
    CHECK(past32);
}

// ---- 3. sequences ----
struct Frame {
    uint8_t b0;
    uint32_t len;
};
static const Frame kAlphabet[] = {
    {0x81, 3},           // TEXT, FIN
    {0x02, 200},         // BINARY
    {0x80, 0},           // CONTINUE, FIN, empty
    {0x00, 126},         // CONTINUE
    {0x42, 0xFFFFFFF0u}, // BINARY, RSV1, a length next to 2^32
    {0x89, 0},           // PING, empty
    {0x8A, 5},           // PONG with payload
    {0x85, 1},           // a reserved opcode as a head, FIN
    {0x88, 2},           // CLOSE
};
constexpr int kA = (int)(sizeof(kAlphabet) / sizeof(kAlphabet[0]));
constexpr int kMaxLen = 6;

struct Rec {
    uint64_t off, bytes, prior;
    uint32_t first, last, frames, b0, bits;
};
struct Walk {
    Rec recs[kMaxLen];
    int nrec;
    uint32_t msg_of[kMaxLen];
    uint8_t carry[16];
};

// the rule restated: a sequential walk, nothing shared with the header
static void walk_restated(const Frame* f, const uint64_t* pos, int n, const uint8_t* carry_in, Walk* w)
{
    bool open = (carry_in[0] & 0x80) != 0;
    uint32_t b0 = carry_in[0] & 0x7F;
    uint64_t prior = 0;
    for (int k = 0; k < 8; ++k) prior |= (uint64_t)carry_in[8 + k] << (8 * k);
    int cur = -1;
    uint64_t end_of[kMaxLen] = {0};
    w->nrec = 0;
    for (int i = 0; i < n; ++i) {
        const int op = f[i].b0 & 15;
        const bool fin = (f[i].b0 & 0x80) != 0;
        bool member = false;
        if (op >= 8) {
        } else if (op != 0) {
            cur = w->nrec++;
            w->recs[cur] = Rec{pos[i], 0, 0, (uint32_t)i, (uint32_t)i, 0, (uint32_t)(f[i].b0 & 0x7F), KMWS_MSG_BEGIN};
            open = member = true;
        } else if (open) {
            if (cur < 0) {
                cur = w->nrec++;
                w->recs[cur] = Rec{pos[i], 0, prior, (uint32_t)i, (uint32_t)i, 0, b0, 0};
            }
            member = true;
        }
        w->msg_of[i] = member ? (uint32_t)cur : KMWS_MSG_NONE;
        if (member) {
            Rec& r = w->recs[cur];
            r.bytes += f[i].len, r.frames += 1, r.last = (uint32_t)i;
            end_of[cur] = pos[i] + f[i].len;
            if (fin) r.bits |= KMWS_MSG_END, open = false;
        }
    }
    for (int r = 0; r < w->nrec; ++r)
        if (end_of[r] - w->recs[r].off == w->recs[r].bytes) w->recs[r].bits |= KMWS_MSG_CONTIG;
    memset(w->carry, 0, 16);
    if (open && cur < 0) memcpy(w->carry, carry_in, 16);
    else if (open) {
        w->carry[0] = (uint8_t)(0x80 | w->recs[cur].b0);
        const uint64_t total = w->recs[cur].prior + w->recs[cur].bytes;
        for (int k = 0; k < 8; ++k) w->carry[8 + k] = (uint8_t)(total >> (8 * k));
    }
}

static kmws_msg finish_record(const MsgSum& v, const Frame* f, const uint64_t* pos, const kmws_msg_carry& carry)
{
    kmws_msg m = msg_record(v, 0u, f[v.first].b0, carry);
    m.off = pos[v.first];
    if (pos[v.last] + f[v.last].len - m.off == m.bytes) m.bits |= (uint8_t)KMWS_MSG_CONTIG;
    return m;
}
static void check_record(const kmws_msg& m, const Rec& r)
{
    CHECK(m.off == r.off && m.bytes == r.bytes && m.prior == r.prior && m.stream == 0u);
    CHECK(m.first == r.first && m.last == r.last && m.frames == r.frames && m.b0 == r.b0 && m.bits == r.bits);
    CHECK(m.utf8 == 0 && m.proto == 0 && m.reserved == 0u);
}

static void check_sequence(const int* idx, int n, const kmws_msg_carry& carry)
{
    Frame f[kMaxLen];
    uint64_t pos[kMaxLen], at = (1ull << 40) + 3;
    for (int k = 0; k < n; ++k) f[k] = kAlphabet[idx[k]], pos[k] = at, at += f[k].len;
    Walk w;
    walk_restated(f, pos, n, carry.b, &w);

    CHECK(msg_carry_ok(carry));
    uint32_t run = msg_const(msg_carry_state(carry)), fn[kMaxLen], cls[kMaxLen];
    MsgSum e[kMaxLen], v[kMaxLen];
    for (int k = 0; k < n; ++k) {
        CHECK((run & kMsgSet) && (run & (kMsgSeenSet | kMsgSeenClear)));  // a constant from the first frame on
        cls[k] = msg_class(msg_state_of(run), msg_seen_of(run), f[k].b0);
        fn[k] = msg_frame_fn(f[k].b0);
        run = msg_compose(run, fn[k]);
        e[k] = msg_sum_of(cls[k], k == 0, (uint32_t)k, (cls[k] & kMsgMember) ? f[k].len : 0u);
        v[k] = k ? msg_sum_compose(v[k - 1], e[k]) : e[k];
    }
    // the same totals folded from the right
    uint32_t run_r = fn[n - 1];
    MsgSum sum_r = e[n - 1];
    for (int k = n - 2; k >= 0; --k) run_r = msg_compose(fn[k], run_r), sum_r = msg_sum_compose(e[k], sum_r);
    CHECK(msg_compose(msg_const(msg_carry_state(carry)), run_r) == run && same(sum_r, v[n - 1]));

    int nrec = 0;
    for (int k = 0; k < n; ++k) {
        if (k && (cls[k] & kMsgStart) && msg_sum_frames(v[k - 1])) {  // a reset point: the record before it is complete
            CHECK((int)msg_sum_starts(v[k - 1]) - 1 == nrec);
            check_record(finish_record(v[k - 1], f, pos, carry), w.recs[nrec++]);
        }
        CHECK(((cls[k] & kMsgMember) ? msg_sum_starts(v[k]) - 1u : KMWS_MSG_NONE) == w.msg_of[k]);
    }
    kmws_msg last;
    memset(&last, 0, sizeof(last));
    if (msg_sum_frames(v[n - 1])) {
        CHECK((int)msg_sum_starts(v[n - 1]) - 1 == nrec);
        last = finish_record(v[n - 1], f, pos, carry);
        check_record(last, w.recs[nrec++]);
    }
    CHECK(nrec == w.nrec && (int)msg_sum_starts(v[n - 1]) == w.nrec);
    const kmws_msg_carry after = msg_carry_after(v[n - 1], last, carry);
    CHECK(memcmp(after.b, w.carry, 16) == 0 && msg_carry_ok(after));
    CHECK(msg_state_of(run) == msg_carry_state(after));  // scan A's last state is the carried one
    ++g_cases;
}

// ---- 4. layout ----
struct Region {
    uint64_t off, count, elem, align;
};
static void check_layout()
{
    static const uint32_t kNs[] = {0, 1, 2, 255, 256, 257, 2047, 2048, 2049, 65536, (1u << 20) + 1, 0x7FFFFFFFu};
    uint64_t prev_row[4] = {0, 0, 0, 0};
    for (uint32_t n : kNs) {
        const uint32_t streams[] = {0, 1, 2, n + 1};
        uint64_t prev = 0;
        for (int si = 0; si < 4; ++si) {
            const uint32_t ns = streams[si];
            const MsgWs w = msg_ws(n, ns);
            const uint64_t F = kMsgBlockFrames;
            CHECK(w.nblk == n / F + (n % F != 0));
            const uint64_t sblk = ((uint64_t)ns + 1 + F - 1) / F;
            CHECK(w.nagg == (w.nblk > sblk ? w.nblk : sblk));
            CHECK((uint64_t)w.nblk * F >= n);
            const Region rs[] = {{0, 1, sizeof(WsHead), 16},
                                 {w.aggs_a, w.nagg, 4, 4},
                                 {w.pre_a, w.nagg, 4, 4},
                                 {w.aggs_b, w.nblk, sizeof(MsgSum), 8},
                                 {w.pre_b, (uint64_t)w.nblk + 1, sizeof(MsgSum), 8},
                                 {w.cls, (uint64_t)w.nblk * F, 2, 8}};  // a lane's four words go out as one
            uint64_t end = 0;
            for (const Region& r : rs) {
                CHECK(r.off % r.align == 0);
                CHECK(r.off >= end);  // ordered, so no two overlap
                end = r.off + r.count * r.elem;
                CHECK(end >= r.off && end <= w.total);
            }
            // 2 B a frame in whole blocks, 8 B a block of either kind, 48 B a block of frames and the total
            CHECK(w.total <= 16 + 2ull * ((uint64_t)n + F) + 8ull * w.nagg + 48ull * ((uint64_t)w.nblk + 1) + 80);
            CHECK(w.total >= prev && w.total >= prev_row[si]);  // monotone in n_streams and in n
            prev = prev_row[si] = w.total;
            ++g_cases;
        }
    }
}

int main()
{
    check_state_monoid();
    check_sum_monoid();
    kmws_msg_carry carries[3];
    carries[0] = msg_carry_make(0u, 0ull);
    carries[1] = msg_carry_make(kMsgOpen | 0x01u, 0ull);
    carries[2] = msg_carry_make(kMsgOpen | 0x42u, (1ull << 33) + 7);
    kmws_msg_carry bad = carries[1];
    bad.b[0] = 0x01;
    CHECK(!msg_carry_ok(bad));
    bad = carries[1], bad.b[5] = 1;
    CHECK(!msg_carry_ok(bad) && msg_carry_prior(carries[2]) == (1ull << 33) + 7);
    int idx[kMaxLen];
    for (int n = 1; n <= kMaxLen; ++n) {
        long total = 1;
        for (int k = 0; k < n; ++k) total *= kA;
        for (long c = 0; c < total; ++c) {
            long x = c;
            for (int k = 0; k < n; ++k) idx[k] = (int)(x % kA), x /= kA;
            for (const kmws_msg_carry& cr : carries) check_sequence(idx, n, cr);
        }
    }
    check_layout();
    if (g_fail) {
        fprintf(stderr, "%d checks failed\n", g_fail);
        return 1;
    }
    printf("OK %ld cases\n", g_cases);
    return 0;
}
