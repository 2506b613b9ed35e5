// Host check of kuma_amd/csrc/kmws_proto_rule.hpp, kmws_proto_stream.hpp and
// the proto layout of kmws_workspace.hpp -- the very functions the kernels and
// the decoder call:
//  1. proto_compose is associative over all 256^3 triples of function bytes;
//     the identity and the constants behave as such;
//  2. every sequence of up to 6 frames over a boundary alphabet (each opcode
//     class, FIN on and off, RSV on and off, CLOSE with a good and a bad body),
//     from each of the 4 carry states: an inclusive scan by proto_compose behind
//     proto_const(carry), then proto_verdict, equals a sequential walk restated
//     here from the RFC's rule; and so do the kmws_proto_stream.hpp functions
//     (IDLE and OPEN, the states a decoder can be in: OPEN is reached by
//     feeding an unfinished head first);
//  3. the CLOSE body rule on masked bytes equals the rule on plain bytes;
//  4. the workspace layout: alignment, bounds, no overlap, no 64-bit wrap.
// Prints "OK <count> cases".  Build: hipcc -x hip --offload-host-only
// (tests/test_proto_rule.py), once plain and once under ASan + UBSan.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "kmws_proto_stream.hpp"
#include "kmws_workspace.hpp"

using namespace kmws;

static int g_fail = 0;
static long g_cases = 0;
#define CHECK(cond)                                                                   \
    do {                                                                              \
        if (!(cond) && g_fail++ < 10) fprintf(stderr, "FAIL line %d: %s\n", __LINE__, #cond); \
    } while (0)

struct Frame {
    uint8_t b0;
    uint32_t len;
    const char* body;  // CLOSE only
};

static const char kGoodBody[] = "\x03\xe8ok";        // 1000 "ok"
static const char kBadCode[] = "\x03\xee";           // 1006
static const char kBadReason[] = "\x03\xe8\xe2\x82";  // ends inside a code point
static const Frame kAlphabet[] = {
    {0x81, 3, nullptr},        // TEXT, FIN
    {0x02, 200, nullptr},      // BINARY
    {0x80, 0, nullptr},        // CONTINUE, FIN
    {0x00, 126, nullptr},      // CONTINUE
    {0xC1, 3, nullptr},        // TEXT, FIN, RSV1 (allowed in this check)
    {0xA2, 3, nullptr},        // BINARY, FIN, RSV2 (not allowed)
    {0xC0, 3, nullptr},        // CONTINUE, FIN, RSV1
    {0x89, 0, nullptr},        // PING
    {0x09, 0, nullptr},        // PING without FIN
    {0x8A, 126, nullptr},      // PONG of 126 bytes
    {0x83, 0, nullptr},        // opcode 3
    {0x88, 4, kGoodBody},      // CLOSE 1000 "ok"
    {0x88, 2, kBadCode},       // CLOSE 1006
    {0x88, 4, kBadReason},     // CLOSE, reason cut
};
constexpr int kA = (int)(sizeof(kAlphabet) / sizeof(kAlphabet[0]));
constexpr uint32_t kRsvAllowed = 0x40u;

// ---- the rule restated: a sequential walk, nothing shared with the header ----
static bool utf8_ok_restated(const uint8_t* p, uint32_t n)
{
    uint32_t i = 0;
    while (i < n) {
        const uint8_t c = p[i];
        uint32_t need, lo = 0x80, hi = 0xBF;
        if (c < 0x80) { ++i; continue; }
        if (c >= 0xC2 && c <= 0xDF) need = 1;
        else if (c >= 0xE0 && c <= 0xEF) { need = 2; if (c == 0xE0) lo = 0xA0; if (c == 0xED) hi = 0x9F; }
        else if (c >= 0xF0 && c <= 0xF4) { need = 3; if (c == 0xF0) lo = 0x90; if (c == 0xF4) hi = 0x8F; }
        else return false;
        if (i + need >= n) return false;  // ends inside the code point (or a continuation is wrong before that)
        if (p[i + 1] < lo || p[i + 1] > hi) return false;
        for (uint32_t k = 2; k <= need; ++k)
            if (p[i + k] < 0x80 || p[i + k] > 0xBF) return false;
        i += need + 1;
    }
    return true;
}
static int local_restated(const Frame& f)
{
    const int op = f.b0 & 15, fin = f.b0 >> 7, rsv = f.b0 & 0x70;
    const bool data_head = op == 1 || op == 2;
    if (rsv & ~(data_head ? (int)kRsvAllowed : 0)) return KMWS_PROTO_RSV;
    if ((op >= 3 && op <= 7) || op >= 11) return KMWS_PROTO_OPCODE;
    if (op >= 8 && (!fin || f.len > 125)) return KMWS_PROTO_CONTROL;
    if (op == 8 && f.len >= 1) {
        if (f.len == 1) return KMWS_PROTO_CLOSE_PAYLOAD;
        const int code = ((uint8_t)f.body[0] << 8) | (uint8_t)f.body[1];
        const bool ok = (code >= 1000 && code <= 1003) || (code >= 1007 && code <= 1014) || (code >= 3000 && code <= 4999);
        if (!ok) return KMWS_PROTO_CLOSE_PAYLOAD;
        if (!utf8_ok_restated((const uint8_t*)f.body + 2, f.len - 2)) return KMWS_PROTO_CLOSE_REASON;
    }
    return 0;
}
enum { IDLE = 0, OPEN = 1, CLOSED = 2, FAILED = 3 };
static int step_restated(int* state, const Frame& f)
{
    const int op = f.b0 & 15, fin = f.b0 >> 7;
    if (*state == FAILED) return KMWS_PROTO_AFTER_FAIL;
    if (*state == CLOSED) return KMWS_PROTO_AFTER_CLOSE;
    int v = local_restated(f);
    if (!v && *state == IDLE && op == 0) v = KMWS_PROTO_CONTINUATION;
    if (!v && *state == OPEN && (op == 1 || op == 2)) v = KMWS_PROTO_INTERLEAVED;
    if (v) *state = FAILED;
    else if (op == 8) *state = CLOSED;
    else if (op < 8) *state = fin ? IDLE : OPEN;
    return v;
}

static uint32_t local_of(const Frame& f)
{
    return proto_local(f.b0, f.len, 0u, kRsvAllowed, (const uint8_t*)f.body, 0u);
}

static void check_sequence(const int* idx, int n)
{
    uint32_t local[6], fn[6];
    for (int k = 0; k < n; ++k) {
        local[k] = local_of(kAlphabet[idx[k]]);
        fn[k] = proto_frame_fn(local[k], kAlphabet[idx[k]].b0);
    }
    for (int carry = 0; carry < 4; ++carry) {
        int st = carry;
        uint32_t run = proto_const((uint32_t)carry);  // the stream's first frame is composed behind it
        ProtoStream ps;
        ps.rsv_allowed = (uint8_t)kRsvAllowed;
        const bool host = carry == IDLE || carry == OPEN;
        if (carry == OPEN) CHECK(proto_stream_frame(ps, 0x02u, nullptr, 0u, 0u) == KMWS_PROTO_OK);
        for (int k = 0; k < n; ++k) {
            const Frame& f = kAlphabet[idx[k]];
            const uint32_t before = proto_apply(run, 0u);
            CHECK(run == proto_const(before));  // a constant: any input state gives the same
            const int want = step_restated(&st, f);
            CHECK((int)proto_verdict(before, local[k], f.b0) == want);
            run = proto_compose(run, fn[k]);
            CHECK((int)proto_apply(run, 2u) == st);
            if (host) {
                CHECK(proto_stream_frame(ps, f.b0, (const uint8_t*)f.body, f.len, 0u) == want);
                CHECK(ps.state == st);
            }
        }
        ++g_cases;
    }
}

static void check_compose()
{
    for (uint32_t a = 0; a < 256; ++a) {
        CHECK(proto_compose(a, proto_identity()) == a && proto_compose(proto_identity(), a) == a);
        for (uint32_t s = 0; s < 4; ++s) {
            CHECK(proto_compose(a, proto_const(s)) == proto_const(s));                  // a constant absorbs what is before it
            CHECK(proto_compose(proto_const(s), a) == proto_const(proto_apply(a, s)));  // and stays one
            CHECK(proto_apply(proto_const(s), a & 3u) == s && proto_apply(proto_identity(), s) == s);
        }
        for (uint32_t b = 0; b < 256; ++b) {
            const uint32_t ab = proto_compose(a, b);
            CHECK(ab < 256);
            for (uint32_t s = 0; s < 4; ++s) CHECK(proto_apply(ab, s) == proto_apply(b, proto_apply(a, s)));
            uint32_t differ = 0;
            for (uint32_t c = 0; c < 256; ++c) differ += proto_compose(ab, c) != proto_compose(a, proto_compose(b, c));
            CHECK(differ == 0);  // associative
        }
    }
    g_cases += 256l * 256 * 256;
}

// Rule 5 on masked bytes, and through the stream's private copy (which must
// leave the caller's bytes as they are).
static void check_masked_close()
{
    const char* bodies[] = {kGoodBody, kBadCode, kBadReason};
    const uint32_t lens[] = {4, 2, 4};
    const uint32_t keys[] = {0u, 0x04030201u, 0xFFFFFFFFu, 0x80E2EE03u};
    for (int b = 0; b < 3; ++b)
        for (uint32_t key : keys) {
            uint8_t m[8], keep[8];
            for (uint32_t j = 0; j < lens[b]; ++j) m[j] = (uint8_t)(bodies[b][j] ^ (uint8_t)(key >> (8 * (j & 3))));
            memcpy(keep, m, sizeof(m));
            const uint32_t want = proto_close_body((const uint8_t*)bodies[b], lens[b], 0u);
            CHECK(proto_close_body(m, lens[b], key) == want);
            ProtoStream ps;
            CHECK(proto_stream_frame(ps, 0x88u, m, lens[b], key) == (int)want);
            CHECK(memcmp(keep, m, lens[b]) == 0);
            CHECK(ps.state == (want ? FAILED : CLOSED));
            proto_stream_reset(ps);
            CHECK(ps.state == IDLE);
            ++g_cases;
        }
    // a 125-byte CLOSE through the private copy: the longest it must hold
    uint8_t big[125];
    big[0] = 0x03, big[1] = 0xE8;
    memset(big + 2, 'a', 123);
    ProtoStream ps;
    CHECK(proto_stream_frame(ps, 0x88u, big, 125u, 0u) == KMWS_PROTO_OK);
    ++g_cases;
}

struct Region {
    uint64_t off, count, elem, align;
};
static void check_layout()
{
    static const uint32_t kNs[] = {0, 1, 2, 255, 256, 257, 2047, 2048, 2049, 65536, (1u << 20) + 1, 0x7FFFFFFFu};
    for (uint32_t n : kNs) {
        const uint32_t streams[] = {0, 1, 2, n + 1};
        for (uint32_t ns : streams) {
            const ProtoWs w = proto_ws(n, ns);
            const uint64_t F = kProtoBlockFrames;
            CHECK(w.nblk == n / F + (n % F != 0));
            const uint64_t sblk = ((uint64_t)ns + 1 + F - 1) / F;
            CHECK(w.nagg == (w.nblk > sblk ? w.nblk : sblk));
            // the frame arrays hold whole blocks, stored as 32-bit words
            const Region rs[] = {{0, 1, sizeof(WsHead), 16},           {w.aggs, w.nagg, 2, 2}, {w.pre, w.nagg, 1, 1},
                                 {w.local, (uint64_t)w.nblk * F, 1, 4}, {w.incl, (uint64_t)w.nblk * F, 1, 4}};
            for (const Region& r : rs) {
                CHECK(r.off % r.align == 0);
                CHECK(r.off + r.count * r.elem >= r.off && r.off + r.count * r.elem <= w.total);
                CHECK((uint64_t)w.nblk * F >= n);
            }
            for (int i = 0; i < 5; ++i)
                for (int j = i + 1; j < 5; ++j) {
                    const uint64_t bi = rs[i].count * rs[i].elem, bj = rs[j].count * rs[j].elem;
                    if (bi && bj) CHECK(rs[i].off + bi <= rs[j].off || rs[j].off + bj <= rs[i].off);
                }
            CHECK(w.total <= 16 + 2ull * ((uint64_t)n + F) + 3ull * w.nagg + 48);  // about 2 B a frame, 3 B a block
            ++g_cases;
        }
    }
}

int main()
{
    check_compose();
    int idx[6];
    for (int n = 1; n <= 6; ++n) {
        long total = 1;
        for (int k = 0; k < n; ++k) total *= kA;
        for (long c = 0; c < total; ++c) {
            long x = c;
            for (int k = 0; k < n; ++k) idx[k] = (int)(x % kA), x /= kA;
            check_sequence(idx, n);
        }
    }
    check_masked_close();
    check_layout();
    if (g_fail) {
        fprintf(stderr, "%d checks failed\n", g_fail);
        return 1;
    }
    printf("OK %ld cases\n", g_cases);
    return 0;
}
