// Where everything lies in a caller workspace: one function per kind returns
// byte offsets, the element counts the launchers run over, and `total`, which
// the public kmws_*_workspace_size functions return.  The entries take every
// device pointer through at<T>(workspace, offset); nothing else adds a byte
// count to a workspace pointer.  Host code (tests/cpp/workspace_layout_check.cpp sweeps it).
// Every kind starts with the WsHead; `|` reads "behind, rounded up as the function says":
//   plan = head | tile records + sentinel     utf8 = plan | frame arrays     fused = utf8 | edges
//   copy = head | tile prefixes + totals | row prefixes | unit form: edge words | unit records
//                                                       | chunk form: chunk map | dense list
//   reframe = copy | outgoing flags     gather_utf8 = copy | frame arrays     reframe_utf8 = reframe | frame arrays
//   pack_headers = head | tile states     proto = head | block aggregates | their prefixes | per-frame bytes
//   msg = head | state aggregates | their prefixes | sum aggregates | their prefixes + total | per-frame words
// The one alias: the copy's edge words and its chunk map start at the same
// offset (edge == cmap); a batch takes one form (copy_uses_chunks), only that
// form's regions are live and the other's counts are 0.  Inside one region: the
// one-pass chunk front keeps its tile states in the first nt 8-byte words of the
// row prefixes, and the frame arrays' elements become the frames' views in place.
#pragma once
#include "kmws_common.hpp"
#include "kmws_msg_rule.hpp"
#include "kmws_stream_scan.hpp"

namespace kmws {

template <class T>  // T carries the const of a read-only workspace
inline T* at(const void* ws, uint64_t off)
{
    return ws ? reinterpret_cast<T*>(reinterpret_cast<uintptr_t>(ws) + off) : nullptr;
}

// Element sizes and tile shapes of types and kernels this header cannot see;
// each is tied to its owner by a static_assert next to it.
constexpr uint64_t kWsV2Bytes = 16, kWsUnitRecBytes = 32, kWsUtf8ElemBytes = 8;
constexpr uint64_t kWsScanTile = 2048;    // frames per scan tile (kmws_pack.hip: kScanTile)
constexpr uint64_t kWsUnitWords = 256;    // 16-byte words per wave unit (kUnitWords)
constexpr uint64_t kWsEdgeWords = 5;      // edge words per frame (kEdgeWords)
constexpr uint64_t kWsChunkBytes = 4096;  // bytes per chunk (kChunkBytes)
// Mean region bound cap / n below which the copy takes the chunk form (measured: kmws_pack.hip).
constexpr uint64_t kChunkFormBelow = 16384;
inline uint64_t ceil_div(uint64_t a, uint64_t b) { return (a + b - 1) / b; }

// The unmask plan: TileRec map[map_count], one per tile of kPlanTile bytes (the
// partial last one included) and the sentinel.
struct PlanWs {
    uint64_t ntiles, map, map_count, total;
};
inline PlanWs plan_ws(uint64_t span)
{
    const uint64_t ntiles = ceil_div(span, kPlanTile);
    return PlanWs{ntiles, sizeof(WsHead), ntiles + 1, sizeof(WsHead) + (ntiles + 1) * sizeof(TileRec)};
}

// The UTF-8 check's arrays behind `front` bytes: uint32_t first_bad[n], Utf8Elem
// elems[n] (then the views), aggs[nblk], pre[nblk] (nblk scan blocks of kBlock
// frames), carry[n_streams].
struct FrameArraysWs {
    uint64_t first_bad, elems, aggs, pre, carry, total;
    uint32_t n, nblk, n_streams;
};
inline FrameArraysWs frame_arrays_ws(uint64_t front, uint32_t n, uint32_t n_streams)
{
    FrameArraysWs w{};
    w.n = n, w.n_streams = n_streams, w.nblk = (uint32_t)ceil_div(n, kBlock);
    w.first_bad = r16(front);
    w.elems = w.first_bad + r16((uint64_t)n * 4);
    w.aggs = w.elems + r16((uint64_t)n * kWsUtf8ElemBytes);
    w.pre = w.aggs + r16((uint64_t)w.nblk * kWsUtf8ElemBytes);
    w.carry = w.pre + r16((uint64_t)w.nblk * kWsUtf8ElemBytes);
    w.total = w.carry + r16((uint64_t)n_streams * kWsUtf8ElemBytes);
    return w;
}

// kmws_utf8_validate: plan | frame arrays.  The fused unmask + UTF-8 pass: that
// | uint32_t edges[ntiles], one look-back dword per tile.
struct Utf8Ws {
    PlanWs plan;
    FrameArraysWs fa;
    uint64_t total;
};
inline Utf8Ws utf8_ws(uint64_t span, uint32_t n, uint32_t n_streams)
{
    const PlanWs plan = plan_ws(span);
    const FrameArraysWs fa = frame_arrays_ws(plan.total, n, n_streams);
    return Utf8Ws{plan, fa, fa.total};
}
struct FusedWs {
    Utf8Ws u;
    uint64_t edges, total;
};
inline FusedWs fused_ws(uint64_t span, uint32_t n, uint32_t n_streams)
{
    const Utf8Ws u = utf8_ws(span, n, n_streams);
    return FusedWs{u, r16(u.total), r16(u.total) + r16(u.plan.ntiles * 4)};
}

// The copy (encode, gather) in both forms.
inline bool copy_uses_chunks(uint32_t n, uint64_t cap) { return n && cap / n < kChunkFormBelow; }
struct CopyLayout {
    uint32_t nt, nrows;   // scan tiles of kWsScanTile frames, rows of kBlock frames
    bool chunks;          // the form
    uint64_t tiles, totals;  // V2[nt + 1]: tile prefixes, then the totals
    uint64_t rows;        // V2[nrows]: a row's prefix inside its tile
    uint64_t states;      // == rows: uint64_t[nt], the one-pass chunk front's tile states
    uint64_t zero_words;  // 8-byte words from offset 0 that front zeroes: head, tiles, states
    uint64_t edge, rec, max_units;   // unit form: u32x4[n * kWsEdgeWords], UnitRec[max_units]
    uint64_t cmap, dense, n_chunks;  // chunk form: uint32_t[n_chunks + 1], uint32_t[n_chunks]; cmap == edge
    uint64_t total;
};
inline CopyLayout copy_ws(uint32_t n, uint64_t cap)
{
    CopyLayout w{};
    w.nt = (uint32_t)ceil_div(n, kWsScanTile), w.nrows = (uint32_t)ceil_div(n, kBlock);
    w.chunks = copy_uses_chunks(n, cap);
    w.tiles = r16(sizeof(WsHead));
    w.totals = w.tiles + (uint64_t)w.nt * kWsV2Bytes;
    w.rows = w.states = w.totals + kWsV2Bytes;
    w.zero_words = (w.states + (uint64_t)w.nt * 8) / 8;
    // edge words and records (or the chunk map) on whole 256-byte lines
    w.edge = w.rec = w.cmap = w.dense = r256(w.rows + (uint64_t)w.nrows * kWsV2Bytes);
    if (!w.chunks) {
        // sum of unit_bound(R_f) <= cap / (16 U) + n (1 + 63 / U), U = kWsUnitWords,
        // rounded up to whole blocks: every wave of the copy grid reads its record
        const uint64_t u = ceil_div(cap, kWsUnitWords * 16) + n + ceil_div(63ull * n, kWsUnitWords) + 1;
        w.max_units = ceil_div(u, kBlock / 64) * (kBlock / 64);
        w.rec = w.edge + r256((uint64_t)n * kWsEdgeWords * 16);
        w.total = w.rec + w.max_units * kWsUnitRecBytes;
    } else {
        w.n_chunks = ceil_div(cap, kWsChunkBytes);  // upper bound: the chunks of dst_cap
        w.dense = w.cmap + r256((w.n_chunks + 1) * 4);
        w.total = w.dense + r256(w.n_chunks * 4);
    }
    return w;
}

// The copy family: copy [| uint16_t oflags[n], the outgoing flags kmws_unpack_reframe*
// derives] [| frame arrays, the validating forms]; a part left out is zeroes.
struct CopyFamilyWs {
    CopyLayout copy;
    uint64_t oflags;
    FrameArraysWs fa;
    uint64_t total;
};
inline CopyFamilyWs copy_family_ws(uint32_t n, uint64_t cap, bool reframe, bool utf8, uint32_t n_streams)
{
    CopyFamilyWs w{};
    w.copy = copy_ws(n, cap);
    w.total = w.copy.total;
    if (reframe) w.oflags = r256(w.total), w.total = w.oflags + r16(2ull * n);
    if (utf8) w.fa = frame_arrays_ws(r256(w.total), n, n_streams), w.total = w.fa.total;
    return w;
}
inline CopyFamilyWs reframe_ws(uint32_t n, uint64_t cap) { return copy_family_ws(n, cap, true, false, 0); }
inline CopyFamilyWs gather_utf8_ws(uint32_t n, uint64_t cap, uint32_t ns) { return copy_family_ws(n, cap, false, true, ns); }
inline CopyFamilyWs reframe_utf8_ws(uint32_t n, uint64_t cap, uint32_t ns) { return copy_family_ws(n, cap, true, true, ns); }

// The blocks of a per-stream scan at four frames a lane (kmws_stream_scan.hpp): nblk
// blocks of F = kScanBlockFrames hold frames; the first pass also runs over the
// n_streams + 1 entries of stream_first, so nagg = the blocks of the longer of the
// two, each with an aggregate (its status bits above it) and a scanned prefix.
struct StreamBlocks {
    uint32_t nblk, nagg;
    // The first pass's blocks: without stream_first there is one stream, whose carry block 0 checks.
    uint32_t first_pass(const uint32_t* stream_first) const { return stream_first ? nagg : nblk; }
};
inline StreamBlocks stream_blocks(uint32_t n, uint32_t n_streams)
{
    const uint32_t nblk = (uint32_t)ceil_div(n, kScanBlockFrames);
    const uint32_t sblk = (uint32_t)ceil_div((uint64_t)n_streams + 1, kScanBlockFrames);
    return StreamBlocks{nblk, nblk > sblk ? nblk : sblk};
}

// kmws_proto_check: head | uint16_t aggs[nagg] | uint8_t pre[nagg] | uint8_t local[nblk * F]
// | uint8_t incl[nblk * F].  The frame arrays cover whole blocks: a lane stores its
// four frames' bytes as one word.
struct ProtoWs : StreamBlocks {
    uint64_t aggs, pre, local, incl, total;
};
inline ProtoWs proto_ws(uint32_t n, uint32_t n_streams)
{
    ProtoWs w{stream_blocks(n, n_streams)};
    w.aggs = r16(sizeof(WsHead));
    w.pre = w.aggs + r16((uint64_t)w.nagg * 2);
    w.local = w.pre + r16((uint64_t)w.nagg);
    w.incl = w.local + (uint64_t)w.nblk * kScanBlockFrames;
    w.total = w.incl + (uint64_t)w.nblk * kScanBlockFrames;
    return w;
}

// kmws_msg_index: head | uint32_t aggs_a[nagg] | uint32_t pre_a[nagg] | MsgSum aggs_b[nblk]
// | MsgSum pre_b[nblk + 1] | uint16_t cls[nblk * F].  Scan A has nagg aggregates;
// scan B has an aggregate per block of frames, and its prefixes end with the
// batch's total.  cls covers whole blocks: a lane stores its four frames' words as one.
struct MsgWs : StreamBlocks {
    uint64_t aggs_a, pre_a, aggs_b, pre_b, cls, total;
};
inline MsgWs msg_ws(uint32_t n, uint32_t n_streams)
{
    MsgWs w{stream_blocks(n, n_streams)};
    w.aggs_a = r16(sizeof(WsHead));
    w.pre_a = w.aggs_a + r16((uint64_t)w.nagg * 4);
    w.aggs_b = w.pre_a + r16((uint64_t)w.nagg * 4);
    w.pre_b = w.aggs_b + r16((uint64_t)w.nblk * sizeof(MsgSum));
    w.cls = w.pre_b + r16(((uint64_t)w.nblk + 1) * sizeof(MsgSum));
    w.total = w.cls + (uint64_t)w.nblk * kScanBlockFrames * 2;
    return w;
}

// kmws_pack_headers with wire offsets: head | uint64_t states[nt], one per scan
// tile; the kernel's front zeroes all of it, total / 8 words.
struct PackHeadersWs {
    uint32_t nt, nrows;
    uint64_t states, total;
};
inline PackHeadersWs pack_headers_ws(uint32_t n)
{
    const uint32_t nt = (uint32_t)ceil_div(n, kWsScanTile);
    return PackHeadersWs{nt, (uint32_t)ceil_div(n, kBlock), r16(sizeof(WsHead)), r16(sizeof(WsHead)) + (uint64_t)nt * 8};
}

}  // namespace kmws
