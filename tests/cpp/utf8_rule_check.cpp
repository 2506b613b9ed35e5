// Host check of kuma_amd/csrc/kmws_utf8_rule.hpp: the byte rule, the scan
// operator, the frame element / view and the carry that kmws_utf8.hip's kernels
// call, driven the way the kernels drive them, over every string of length 1-4
// over an alphabet of boundary bytes, under every split into fragments (one
// text message: head, CONTINUE frames, FIN on the last) and every cut of the
// frame list into two batches joined by the carry.  Expected verdicts come
// from a decoder restated here by code point arithmetic (lead -> length,
// accumulate, range of the code points still reachable), not by byte tables.
// Also: the 16-byte word form of the rule against the byte rule on random
// windows, and the operator's associativity on random triples.
// Build: hipcc -x hip --offload-host-only (tests/test_utf8_rule.py).
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "kmws_utf8_rule.hpp"

using namespace kmws;

static const uint8_t kAlphabet[] = {0x00, 0x7F, 0x80, 0x8F, 0x90, 0x9F, 0xA0, 0xBF, 0xC0, 0xC1, 0xC2, 0xDF,
                                    0xE0, 0xE1, 0xEC, 0xED, 0xEE, 0xEF, 0xF0, 0xF1, 0xF3, 0xF4, 0xF5, 0xFF};
constexpr int kA = sizeof(kAlphabet);

// ---- restated decoder ----
struct RefDec {
    int remaining = 0;  // continuation bytes still expected
    uint32_t acc = 0;   // code point bits so far
    uint32_t min_cp = 0;
};
// false: b cannot follow (no completion of the bytes so far is well-formed).
static bool ref_step(RefDec& d, uint8_t b)
{
    if (d.remaining == 0) {
        if (b < 0x80) return true;
        if (b >= 0xC0 && b < 0xE0) { d.remaining = 1; d.acc = b & 0x1Fu; d.min_cp = 0x80; }
        else if (b >= 0xE0 && b < 0xF0) { d.remaining = 2; d.acc = b & 0x0Fu; d.min_cp = 0x800; }
        else if (b >= 0xF0 && b < 0xF8) { d.remaining = 3; d.acc = b & 0x07u; d.min_cp = 0x10000; }
        else return false;
    } else {
        if ((b & 0xC0) != 0x80) return false;
        d.acc = (d.acc << 6) | (b & 0x3Fu);
        --d.remaining;
    }
    // the code points still reachable: [lo, hi]
    const uint32_t lo = d.acc << (6 * d.remaining), hi = lo | ((1u << (6 * d.remaining)) - 1u);
    if (hi < d.min_cp) { return false; }                  // overlong whatever follows
    if (lo > 0x10FFFFu) { return false; }                 // beyond Unicode whatever follows
    if (lo >= 0xD800u && hi <= 0xDFFFu) { return false; } // a surrogate whatever follows
    return true;
}

static int g_fail = 0;
static void fail(const char* what, const uint8_t* s, int len, unsigned split)
{
    if (g_fail++ < 10) {
        fprintf(stderr, "FAIL %s:", what);
        for (int i = 0; i < len; ++i) fprintf(stderr, " %02X", s[i]);
        fprintf(stderr, " split %u\n", split);
    }
}

// The kernels' procedure on frames [f0, f1) of one stream with carry c_in:
// elements, scan, views, byte rule, rule (b); writes verdicts, returns carry out.
static uint64_t run_batch(const uint8_t* const* pay, const int* len, const uint8_t* ob, int f0, int f1,
                          uint64_t c_in, int* verdict)
{
    uint32_t first_bad[8];
    Utf8Elem el[8], before[8];
    Utf8View view[8];
    if (f0 == f1) return c_in;
    Utf8Elem run = utf8_identity();
    for (int i = f0; i < f1; ++i) {
        const int k = i - f0;
        uint32_t nb = len[i] < 3 ? (uint32_t)len[i] : 3u, tail = 0;
        for (uint32_t j = 0; j < nb; ++j) tail = (tail << 8) | pay[i][len[i] - nb + j];
        el[k] = utf8_frame_elem(ob[i], (uint32_t)k, tail, nb);
        first_bad[k] = 0xFFFFFFFFu;
        if (k == 0) {
            bool bad = false;
            const Utf8Elem st = utf8_carry_unpack(c_in, 0u, &bad);
            el[k] = utf8_combine(st, el[k]);
            const uint32_t op = ob[i] & 0x0Fu;
            if (bad && (op == 0u || op >= 8u)) first_bad[0] = 0u;
            before[k] = st;
        } else {
            before[k] = run;
        }
        run = utf8_combine(run, el[k]);
    }
    const Utf8Elem after = run;
    for (int i = f0; i < f1; ++i) {
        const int k = i - f0;
        view[k] = utf8_frame_view(before[k], ob[i], (uint32_t)k);
        if (!(view[k].w & kUtf8Checked)) continue;
        uint32_t L = view[k].w & 0xFFFFFFu;
        for (int j = 0; j < len[i]; ++j) {
            if (utf8_byte_bad(pay[i][j], L) && first_bad[view[k].slot] > (uint32_t)k + 1u)
                first_bad[view[k].slot] = (uint32_t)k + 1u;
            L = utf8_append(L, pay[i][j]);
        }
        if (ob[i] & 0x80u) {  // rule (b), from the element's tail as the kernel does
            const uint32_t nb = utf8_elem_nb(el[k]);
            const uint32_t Le = nb >= 3u ? utf8_elem_ctx(el[k])
                                         : (((view[k].w << (8u * nb)) | utf8_elem_ctx(el[k])) & 0xFFFFFFu);
            if (utf8_pending(Le) && first_bad[view[k].slot] > (uint32_t)k + 1u) first_bad[view[k].slot] = k + 1u;
        }
    }
    for (int i = f0; i < f1; ++i) {
        const int k = i - f0;
        if (!(view[k].w & kUtf8Checked)) { verdict[i] = 0; continue; }
        const uint32_t fb = first_bad[view[k].slot];
        verdict[i] = fb > (uint32_t)k + 1u ? 1 : (fb == (uint32_t)k + 1u ? 2 : 3);
    }
    const bool chk = (after.w & (kUtf8Open | kUtf8Checked)) == (kUtf8Open | kUtf8Checked);
    return utf8_carry_pack(after, chk && first_bad[after.slot] != 0xFFFFFFFFu);
}

static uint64_t rnd_state = 0x1234567ull;
static uint32_t rnd()
{
    rnd_state = rnd_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(rnd_state >> 33);
}
static Utf8Elem rnd_elem()
{
    const uint32_t nb = rnd() & 3u;
    uint32_t w = (rnd() & (nb == 0 ? 0u : (nb == 1 ? 0xFFu : (nb == 2 ? 0xFFFFu : 0xFFFFFFu)))) | (nb << 24);
    if (rnd() & 1u) w |= kUtf8Reset | ((rnd() & 1u) ? kUtf8Open : 0u) | ((rnd() & 1u) ? kUtf8Checked : 0u);
    return Utf8Elem{(w & kUtf8Reset) ? rnd() & 0xFFu : 0u, w};
}

int main()
{
    unsigned long long cases = 0;
    uint8_t s[4];
    for (int len = 1; len <= 4; ++len) {
        int idx[4] = {0, 0, 0, 0};
        for (;;) {
            for (int i = 0; i < len; ++i) s[i] = kAlphabet[idx[i]];
            // expected: first bad byte, or a dangling tail
            RefDec d;
            int bad_at = -1;
            for (int i = 0; i < len && bad_at < 0; ++i)
                if (!ref_step(d, s[i])) bad_at = i;
            const bool dangling = bad_at < 0 && d.remaining != 0;
            for (unsigned split = 0; split < (1u << (len - 1)); ++split) {  // bit i: a cut after byte i
                const uint8_t* pay[4];
                int flen[4], start[5], nf = 0;
                uint8_t ob[4];
                start[0] = 0;
                for (int i = 0; i < len; ++i)
                    if (i == len - 1 || (split >> i & 1u)) {
                        pay[nf] = s + start[nf];
                        flen[nf] = i + 1 - start[nf];
                        ++nf;
                        start[nf] = i + 1;
                    }
                for (int f = 0; f < nf; ++f) ob[f] = (uint8_t)((f == 0 ? 1 : 0) | (f == nf - 1 ? 0x80 : 0));
                int expect[4];
                int bad_frame = -1;
                if (bad_at >= 0) {
                    for (int f = 0; f < nf; ++f)
                        if (bad_at >= start[f] && bad_at < start[f] + flen[f]) bad_frame = f;
                } else if (dangling) {
                    bad_frame = nf - 1;
                }
                for (int f = 0; f < nf; ++f) expect[f] = bad_frame < 0 || f < bad_frame ? 1 : (f == bad_frame ? 2 : 3);
                for (int cut = 0; cut <= nf; ++cut) {  // cut == 0 / nf: one batch (and an empty one)
                    int got[4] = {-1, -1, -1, -1};
                    const uint64_t c = run_batch(pay, flen, ob, 0, cut, 0ull, got);
                    const uint64_t c2 = run_batch(pay, flen, ob, cut, nf, c, got);
                    for (int f = 0; f < nf; ++f)
                        if (got[f] != expect[f]) { fail("verdict", s, len, split | (unsigned)cut << 8); break; }
                    if (c2 != 0ull) fail("carry after FIN", s, len, split | (unsigned)cut << 8);
                    ++cases;
                }
            }
            int k = len - 1;
            while (k >= 0 && ++idx[k] == kA) idx[k--] = 0;
            if (k < 0) break;
        }
    }
    // the word form (utf8_word_bad_swar) against the byte rule, on windows of 22
    // bytes: [0,3) look-back only, [3,6) the three bytes before the word, [6,22)
    // the word.  It must flag the word when the byte rule's first error in [3,22)
    // lies in the word, and must not flag unless the byte rule rejects a byte of [3,22).
    unsigned long long windows = 0;
    for (int t = 0; t < 6000000; ++t) {
        uint8_t wnd[22];
        const uint32_t mode = rnd() & 3u;
        for (int i = 0; i < 22; ++i) wnd[i] = mode == 0 ? (uint8_t)(rnd() & 0xFFu) : kAlphabet[rnd() % kA];
        if (mode >= 2) {  // mostly well-formed: sequences laid end to end, then one byte changed (mode 3)
            static const uint8_t seqs[][5] = {{1, 0x41}, {2, 0xC2, 0x80}, {2, 0xDF, 0xBF}, {3, 0xE0, 0xA0, 0x80},
                                              {3, 0xED, 0x9F, 0xBF}, {3, 0xEF, 0xBF, 0xBF}, {4, 0xF0, 0x90, 0x80, 0x80},
                                              {4, 0xF4, 0x8F, 0xBF, 0xBF}, {3, 0xE1, 0x80, 0x80}, {4, 0xF1, 0xBF, 0x80, 0xBF}};
            int i = 0;
            while (i < 22) {
                const uint8_t* q = seqs[rnd() % 10];
                for (int k = 0; k < q[0] && i < 22; ++k) wnd[i++] = q[1 + k];
            }
            if (mode == 3) wnd[3 + rnd() % 19] = kAlphabet[rnd() % kA];
        }
        bool pre = false, word = false;
        for (int i = 3; i < 22; ++i) {
            const uint32_t L = (uint32_t)wnd[i - 1] | ((uint32_t)wnd[i - 2] << 8) | ((uint32_t)wnd[i - 3] << 16);
            if (utf8_byte_bad(wnd[i], L)) (i < 6 ? pre : word) = true;
        }
        auto dw = [&](int i) {
            return (uint32_t)wnd[i] | ((uint32_t)wnd[i + 1] << 8) | ((uint32_t)wnd[i + 2] << 16) | ((uint32_t)wnd[i + 3] << 24);
        };
        const bool sw = utf8_word_bad_swar(dw(2), dw(6), dw(10), dw(14), dw(18));
        if ((!pre && word && !sw) || (sw && !pre && !word)) {
            if (g_fail++ < 10) {
                fprintf(stderr, "FAIL word form (pre %d word %d swar %d):", pre, word, sw);
                for (int i = 0; i < 22; ++i) fprintf(stderr, " %02X", wnd[i]);
                fprintf(stderr, "\n");
            }
        }
        windows += (!pre && word) ? 1 : 0;
    }
    if (windows < 1000000) { fprintf(stderr, "too few informative windows: %llu\n", windows); return 1; }
    // associativity
    for (int t = 0; t < 2000000; ++t) {
        const Utf8Elem a = rnd_elem(), b = rnd_elem(), c = rnd_elem();
        const Utf8Elem l = utf8_combine(utf8_combine(a, b), c), r = utf8_combine(a, utf8_combine(b, c));
        if (l.slot != r.slot || l.w != r.w) {
            if (g_fail++ < 10)
                fprintf(stderr, "FAIL assoc: (%x,%x) (%x,%x) (%x,%x)\n", a.slot, a.w, b.slot, b.w, c.slot, c.w);
        }
    }
    if (g_fail) {
        fprintf(stderr, "%d failures\n", g_fail);
        return 1;
    }
    printf("OK %llu cases\n", cases);
    return 0;
}
