// Host check of kuma_amd/csrc/kmws_utf8_stream.hpp: the two halves of the host
// path's UTF-8 message state (kmws_decoder_set_utf8_check), driven the way
// kmws_decoder.cpp drives them -- the parse-time half per frame in wire order
// (header byte 0 and the frame's last min(len, 3) bytes, unmasked with the
// key), then the delivery-time half per frame with the device's bad bit -- over
// every string of length 1-4 over utf8_rule_check.cpp's boundary alphabet, cut
// into 1-4 fragments at every non-decreasing choice of cut positions (so empty
// fragments occur at the start, in the middle and at the end: head, CONTINUE
// frames, FIN on the last), once as they are and once with a PING holding
// non-UTF-8 bytes between any two fragments.  The device's bit for a frame is a
// byte-rule walk restated here (what unmask_pieces_utf8_kernel computes: the
// rule on the frame's own bytes from the view's look-back); the expected
// verdicts come from a sequential decoder restated by code point arithmetic.
// Then a fixed scenario: a message sequence, a dropped generation, a reset.
// Build: hipcc -x hip --offload-host-only (tests/test_utf8_stream.py).
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "kmws_utf8_stream.hpp"

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
    const uint32_t lo = d.acc << (6 * d.remaining), hi = lo | ((1u << (6 * d.remaining)) - 1u);
    if (hi < d.min_cp) return false;                   // overlong whatever follows
    if (lo > 0x10FFFFu) return false;                  // beyond Unicode whatever follows
    if (lo >= 0xD800u && hi <= 0xDFFFu) return false;  // a surrogate whatever follows
    return true;
}

struct Frame {
    uint8_t ob;
    uint8_t masked[8];  // as on the wire
    int len;
    uint32_t key;
};

static int g_fail = 0;

// The decoder's procedure on one connection's frames; verdicts out.
static void run_stream(Utf8Stream& st, const Frame* fr, int nf, int* verdict)
{
    Utf8StreamView view[16];
    bool dev_bad[16];
    for (int i = 0; i < nf; ++i) {  // parse time, wire order
        uint32_t nb = 0;
        const uint32_t tail = utf8_stream_tail(fr[i].masked, (size_t)fr[i].len, fr[i].key, &nb);
        view[i] = utf8_stream_frame(st, fr[i].ob, tail, nb);
        // the payload pass: checked frames only, the byte rule from the view's look-back
        dev_bad[i] = false;
        if (view[i].w & kUtf8Checked) {
            uint32_t L = view[i].w & 0xFFFFFFu;
            for (int j = 0; j < fr[i].len; ++j) {
                const uint32_t b = (uint32_t)(fr[i].masked[j] ^ (uint8_t)(fr[i].key >> (8 * (j & 3))));
                if (utf8_byte_bad(b, L)) dev_bad[i] = true;
                L = utf8_append(L, b);
            }
        }
    }
    for (int i = 0; i < nf; ++i) verdict[i] = utf8_stream_verdict(st, view[i], dev_bad[i]);  // delivery time
}

static Frame make_frame(uint8_t ob, const uint8_t* p, int len, uint32_t key)
{
    Frame f;
    f.ob = ob;
    f.len = len;
    f.key = key;
    memset(f.masked, 0, sizeof(f.masked));
    for (int j = 0; j < len; ++j) f.masked[j] = (uint8_t)(p[j] ^ (uint8_t)(key >> (8 * (j & 3))));
    return f;
}

static void check(bool ok, const char* what)
{
    if (!ok && g_fail++ < 10) fprintf(stderr, "FAIL %s\n", what);
}

int main()
{
    unsigned long long cases = 0;
    uint8_t s[4];
    static const uint8_t kPing[3] = {0xFF, 0xC0, 0x80};
    for (int len = 1; len <= 4; ++len) {
        int idx[4] = {0, 0, 0, 0};
        for (;;) {
            for (int i = 0; i < len; ++i) s[i] = kAlphabet[idx[i]];
            RefDec d;
            int bad_at = -1;
            for (int i = 0; i < len && bad_at < 0; ++i)
                if (!ref_step(d, s[i])) bad_at = i;
            const bool dangling = bad_at < 0 && d.remaining != 0;
            for (int nfrag = 1; nfrag <= 4; ++nfrag) {
                int cut[5] = {0, 0, 0, 0, 0};  // cut[1..nfrag-1], non-decreasing in [0, len]
                for (;;) {
                    int start[5];
                    start[0] = 0;
                    for (int f = 1; f < nfrag; ++f) start[f] = cut[f];
                    start[nfrag] = len;
                    // expected: BAD at the fragment that holds the first bad byte, or (dangling) at the FIN
                    int bad_frag = -1;
                    if (bad_at >= 0) {
                        for (int f = 0; f < nfrag; ++f)
                            if (bad_at >= start[f] && bad_at < start[f + 1]) bad_frag = f;
                    } else if (dangling) {
                        bad_frag = nfrag - 1;
                    }
                    for (int ping = 0; ping < 2; ++ping) {
                        Frame fr[16];
                        int expect[16], nf = 0;
                        for (int f = 0; f < nfrag; ++f) {
                            if (ping && f) {
                                fr[nf] = make_frame(0x89, kPing, 3, 0x01020304u * (uint32_t)f);
                                expect[nf++] = KMWS_UTF8_NOT_TEXT;
                            }
                            const uint8_t ob = (uint8_t)((f == 0 ? 1 : 0) | (f == nfrag - 1 ? 0x80 : 0));
                            fr[nf] = make_frame(ob, s + start[f], start[f + 1] - start[f],
                                                (f & 1) ? 0u : 0xA1B2C3D4u + (uint32_t)cases);  // masked and unmasked
                            expect[nf++] = bad_frag < 0 || f < bad_frag ? KMWS_UTF8_OK
                                                                        : (f == bad_frag ? KMWS_UTF8_BAD : KMWS_UTF8_AFTER_BAD);
                        }
                        Utf8Stream st;
                        int got[16];
                        run_stream(st, fr, nf, got);
                        bool same = true;
                        for (int i = 0; i < nf; ++i) same &= got[i] == expect[i];
                        if (!same && g_fail++ < 10) {
                            fprintf(stderr, "FAIL verdict:");
                            for (int i = 0; i < len; ++i) fprintf(stderr, " %02X", s[i]);
                            fprintf(stderr, " frags %d cuts %d %d %d ping %d got", nfrag, cut[1], cut[2], cut[3], ping);
                            for (int i = 0; i < nf; ++i) fprintf(stderr, " %d/%d", got[i], expect[i]);
                            fprintf(stderr, "\n");
                        }
                        // after the FIN the stream is between messages: a CONTINUE is not text
                        uint32_t nb = 0;
                        const Utf8StreamView v = utf8_stream_frame(st, 0x80, utf8_stream_tail(kPing, 3, 0u, &nb), 3u);
                        check(utf8_stream_verdict(st, v, true) == KMWS_UTF8_NOT_TEXT, "CONTINUE after FIN");
                        ++cases;
                    }
                    int k = nfrag - 1;  // next non-decreasing cut vector
                    while (k >= 1 && cut[k] == len) --k;
                    if (k < 1) break;
                    ++cut[k];
                    for (int j = k + 1; j < nfrag; ++j) cut[j] = cut[k];
                }
            }
            int k = len - 1;
            while (k >= 0 && ++idx[k] == kA) idx[k--] = 0;
            if (k < 0) break;
        }
    }

    // ---- a message sequence on one stream, frames delivered in a later pass ----
    {
        static const uint8_t kBadTxt[2] = {0x41, 0xFF}, kOkTxt[2] = {0xC3, 0xA9}, kFF[4] = {0xFF, 0xFF, 0xFF, 0xFF};
        const Frame fr[] = {
            make_frame(0x01, kBadTxt, 2, 7u),  // text head, bad byte: BAD
            make_frame(0x00, kOkTxt, 2, 0u),   // CONTINUE: AFTER_BAD
            make_frame(0x8A, kFF, 4, 9u),      // PONG: 0
            make_frame(0x80, kOkTxt, 0, 0u),   // empty FIN: AFTER_BAD
            make_frame(0x01, kOkTxt, 1, 5u),   // text head ending inside a code point: OK so far
            make_frame(0x80, kOkTxt + 1, 1, 0u),  // completes it: OK
            make_frame(0x02, kFF, 4, 3u),      // binary: 0
            make_frame(0x80, kFF, 4, 3u),      // its CONTINUE + FIN: 0
            make_frame(0xC1, kFF, 4, 3u),      // RSV1 text: 0
            make_frame(0x80, kFF, 1, 0u),      // CONTINUE with no open message: 0
            make_frame(0x01, kOkTxt, 1, 0u),   // text head, pending
            make_frame(0x80, kOkTxt, 0, 0u),   // empty FIN while a code point is pending: BAD (rule (b))
        };
        const int want[] = {2, 3, 0, 3, 1, 1, 0, 0, 0, 0, 1, 2};
        Utf8Stream st;
        int got[12];
        run_stream(st, fr, 12, got);
        for (int i = 0; i < 12; ++i) check(got[i] == want[i], "message sequence");
    }
    // ---- a dropped generation: the open message is not checkable until the next head ----
    {
        static const uint8_t kTxt[1] = {0x41}, kBad[1] = {0xFF};
        Utf8Stream st;
        uint32_t nb = 0;
        const Utf8StreamView a = utf8_stream_frame(st, 0x01, utf8_stream_tail(kTxt, 1, 0u, &nb), 1u);  // head, delivered
        const Utf8StreamView b = utf8_stream_frame(st, 0x00, utf8_stream_tail(kTxt, 1, 0u, &nb), 1u);  // dropped
        const Utf8StreamView c = utf8_stream_frame(st, 0x00, utf8_stream_tail(kBad, 1, 0u, &nb), 1u);  // parsed before the drop
        check(utf8_stream_verdict(st, a, false) == KMWS_UTF8_OK, "before the drop");
        utf8_stream_drop(st, b);
        const Utf8StreamView e = utf8_stream_frame(st, 0x80, utf8_stream_tail(kBad, 1, 0u, &nb), 1u);  // parsed after it
        check(utf8_stream_verdict(st, c, true) == KMWS_UTF8_NOT_TEXT, "in flight across the drop");
        check(!(e.w & kUtf8Checked) && utf8_stream_verdict(st, e, true) == KMWS_UTF8_NOT_TEXT, "after the drop");
        const Utf8StreamView f = utf8_stream_frame(st, 0x81, utf8_stream_tail(kBad, 1, 0u, &nb), 1u);  // the next head
        check(utf8_stream_verdict(st, f, true) == KMWS_UTF8_BAD, "next head after the drop");
        // reset: between messages, nothing remembered
        const Utf8StreamView g = utf8_stream_frame(st, 0x01, utf8_stream_tail(kTxt, 1, 0u, &nb), 1u);
        check(utf8_stream_verdict(st, g, false) == KMWS_UTF8_OK, "open before reset");
        utf8_stream_reset(st);
        const Utf8StreamView h = utf8_stream_frame(st, 0x80, utf8_stream_tail(kTxt, 1, 0u, &nb), 1u);
        check(utf8_stream_verdict(st, h, false) == KMWS_UTF8_NOT_TEXT, "CONTINUE after reset");
    }
    if (g_fail) {
        fprintf(stderr, "%d failures\n", g_fail);
        return 1;
    }
    printf("OK %llu cases\n", cases);
    return 0;
}
