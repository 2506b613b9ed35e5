// What the UTF-8 payload passes share: the rule on a 16-byte word held in
// registers (kmws_utf8.hip: the validator and the fused in-place pass;
// kmws_pack.hip: the validating gather), the verdict word's update, and the
// host launchers of the per-frame kernels for a payload pass that lives in
// another translation unit (no relocatable device code: kernels are launched
// from the file that defines them).
#pragma once
#include "kmws_common.hpp"
#include "kmws_utf8_rule.hpp"
#include "kmws_workspace.hpp"

namespace kmws {

constexpr uint32_t kUtf8None = 0xFFFFFFFFu;  // first_bad: holds frame + 1 of the BAD frame, 0 = before this batch

// Byte r (-4 .. 15) of the window: the dword before the word, then the word.
__device__ __forceinline__ uint32_t window_byte(uint32_t prev, const u32x4& w, int r)
{
    const uint32_t dw = r < 0 ? prev : (r < 4 ? w.x : (r < 8 ? w.y : (r < 12 ? w.z : w.w)));
    return (dw >> (8u * ((uint32_t)r & 3u))) & 0xFFu;
}

// The bytes of the 16-byte word at address a (w; prev = the dword before it,
// both unmasked) that belong to the frame [off, end), whose look-back at its
// first byte is ctx: does the byte rule reject one of them?  The look-back of
// the word's first byte is the three bytes before it where the frame has them,
// else ctx and the frame's bytes up to it.
__device__ __forceinline__ bool word_bad(uint32_t prev, const u32x4& w, uint64_t a, uint64_t off, uint64_t end,
                                         uint32_t ctx)
{
    const bool deep = off + 3u <= a;
    // the word and its look-back lie inside the frame: four bytes per operation
    if (deep && end >= a + 16u) return utf8_word_bad_swar(prev, w.x, w.y, w.z, w.w);
    // a frame edge in or just before the word (rare): a rolled loop, compact code
    const int s = deep ? -3 : (int)((int64_t)off - (int64_t)a);  // > -3
    const int e = end >= a + 16u ? 16 : (int)(end - a);
    uint32_t L = deep ? 0u : (ctx & 0xFFFFFFu);
    bool bad = false;
#pragma unroll 1
    for (int r = s; r < e; ++r) {
        const uint32_t b = window_byte(prev, w, r);
        if (r >= 0) bad |= utf8_byte_bad(b, L);
        L = utf8_append(L, b);
    }
    return bad;
}

// Word w (prev: the dword before it, both plain) against the frame [off, end)
// with look-back ctx at its first byte: a word of ASCII bytes after an ASCII
// byte, inside the frame from three bytes before it on, is one OR and a test.
__device__ __forceinline__ bool plain_word_frame_bad(const u32x4& w, uint32_t prev, uint64_t a, uint64_t off,
                                                     uint64_t end, uint32_t ctx)
{
    const bool plain = off + 3u <= a && end >= a + 16u && ((w.x | w.y | w.z | w.w) & 0x80808080u) == 0u &&
                       (prev & 0x80000000u) == 0u;
    return !plain && word_bad(prev, w, a, off, end, ctx);
}

__device__ __forceinline__ void report_bad(uint32_t* __restrict__ first_bad, uint32_t slot, uint32_t frame)
{
    // verdict words only fall: a stale read costs one atomic more, never a verdict
    if (__builtin_nontemporal_load(&first_bad[slot]) > frame + 1u) atomicMin(&first_bad[slot], frame + 1u);
}

// ---- the per-frame kernels around a payload pass of another file ----
// `fa`: where the frame arrays lie in `workspace` (kmws_workspace.hpp), whose
// WsHead holds the status word.  launch_utf8_frame_state runs utf8_elem_kernel, utf8_scan_aggs_kernel and
// utf8_ctx_kernel on the payloads at base + descs[i].off (masked != 0: still
// masked with descs[i].key); a descriptor outside [0, span) or a malformed
// stream_first ORs status bit 1 into the head, which the caller has cleared in
// stream order before.  The payload pass then reads views[i] (checked?, slot,
// look-back at the frame's first byte) and reports into first_bad[slot];
// launch_utf8_frame_finish turns both into out[] and carry_out.
// skip_flag: the bits of flags[i] with which the payload pass leaves frame i
// out (the reframe: KMWS_FLAG_SKIP; kUtf8SkipNone: no such bit).  Such a frame
// is a control frame to the check -- NOT_TEXT, the message state untouched --
// and its descriptor is neither range-checked nor followed.
constexpr uint32_t kUtf8SkipNone = 0u;
__device__ __forceinline__ uint32_t utf8_op_byte(uint32_t fl, uint32_t skip_flag)
{
    return (fl & skip_flag) ? 0x80u | KMWS_OP_PING : fl & 0xFFu;
}
struct Utf8FrameArrays {
    const Utf8View* views;
    uint32_t* first_bad;
};
Utf8FrameArrays launch_utf8_frame_state(void* workspace, const FrameArraysWs& fa, const uint8_t* base, uint64_t span,
                                        const kmws_desc* descs, const uint16_t* flags, uint32_t n, int masked,
                                        uint32_t skip_flag, const uint32_t* stream_first, uint32_t n_streams,
                                        const kmws_utf8_carry* carry_in, hipStream_t s);
void launch_utf8_frame_finish(void* workspace, const FrameArraysWs& fa, uint32_t n, const uint32_t* stream_first,
                              uint32_t n_streams, const kmws_utf8_carry* carry_in, kmws_utf8_carry* carry_out,
                              uint8_t* out, hipStream_t s);
// carry_out = carry_in for every stream (an empty batch).
kmws_status launch_utf8_carry_copy(uint32_t n_streams, const kmws_utf8_carry* carry_in, kmws_utf8_carry* carry_out,
                                   hipStream_t s);

}  // namespace kmws
