// include/kmws_wshandler.hpp's protocol check (setProtocolCheck /
// lastFrameProto) the way a kuma server would use it: the handler reads
// lastFrameProto() inside its frame callback and would close with 1002 (1007
// for KMWS_PROTO_CLOSE_REASON) when it is not KMWS_PROTO_OK.
//   host: a CLIENT-mode handler and unmasked frames -- the check needs no GPU
//   gpu:  the above, and a SERVER-mode handler with masked frames, without an
//         RxLoop and with one (asynchronous and synchronous)
// Build: tests/test_wshandler_proto.py.
#include <cstdio>
#include <cstring>
#include <deque>
#include <functional>
#include <string>
#include <vector>

#include "kmws_wshandler.hpp"

using kmws::ws::BufferChain;
using kmws::ws::FrameHeader;
using kmws::ws::WSError;
using kmws::ws::WSHandler;
using kmws::ws::WSMode;

static int g_fail = 0;
#define CHECK(x)                                                     \
    do {                                                             \
        if (!(x)) {                                                  \
            ++g_fail;                                                \
            std::fprintf(stderr, "FAIL %s:%d %s\n", __FILE__, __LINE__, #x); \
        }                                                            \
    } while (0)

static std::vector<uint8_t> frame(int opcode, int fin, int rsv1, const std::string& payload, bool mask, uint8_t k0)
{
    const uint8_t key[4] = {k0, 0x5a, 0xc3, 0x0f};
    FrameHeader h;
    std::memset(static_cast<void*>(&h), 0, sizeof(h));
    h.fin = fin;
    h.rsv1 = rsv1;
    h.opcode = opcode;
    h.mask = mask;
    h.length = (uint32_t)payload.size();
    std::memcpy(h.maskey, key, 4);
    uint8_t hb[KMWS_MAX_HEADER_SIZE];
    const int n = WSHandler::encodeFrameHeader(h, hb);
    std::vector<uint8_t> w(hb, hb + n);
    for (size_t i = 0; i < payload.size(); ++i) w.push_back((uint8_t)(payload[i] ^ (mask ? key[i % 4] : 0)));
    return w;
}
static void append(std::vector<uint8_t>& w, const std::vector<uint8_t>& f) { w.insert(w.end(), f.begin(), f.end()); }

// One connection that stays clean up to a CLOSE whose reason is cut inside a
// code point, and one that interleaves a data head into an open message.
static std::vector<uint8_t> wire_a(bool mask)
{
    std::vector<uint8_t> w;
    append(w, frame(1, 0, 1, "compressed", mask, 1));  // RSV1: negotiated below
    append(w, frame(9, 1, 0, "?", mask, 2));
    append(w, frame(0, 1, 0, std::string(300, 'x'), mask, 3));
    append(w, frame(8, 1, 0, std::string("\x03\xe8", 2) + "bye \xe2\x82", mask, 4));
    return w;
}
static const int kWantA[4] = {KMWS_PROTO_OK, KMWS_PROTO_OK, KMWS_PROTO_OK, KMWS_PROTO_CLOSE_REASON};
static std::vector<uint8_t> wire_b(bool mask)
{
    std::vector<uint8_t> w;
    append(w, frame(2, 0, 0, "head", mask, 5));
    append(w, frame(1, 1, 0, "another head", mask, 6));
    append(w, frame(0, 1, 0, "tail", mask, 7));
    append(w, frame(8, 1, 0, std::string("\x03\xe8", 2), mask, 8));
    return w;
}
static const int kWantB[4] = {KMWS_PROTO_OK, KMWS_PROTO_INTERLEAVED, KMWS_PROTO_AFTER_FAIL, KMWS_PROTO_AFTER_FAIL};

static void collect(WSHandler& h, std::vector<int>& out)
{
    h.setFrameCallback([&h, &out](FrameHeader, BufferChain&) {
        out.push_back(h.lastFrameProto());
        return 0;
    });
}
static void expect(const std::vector<int>& got, const int (&want)[4], bool on)
{
    CHECK(got.size() == 4);
    for (size_t i = 0; i < got.size() && i < 4; ++i) CHECK(got[i] == (on ? want[i] : 0));
}

static void direct(WSMode mode)
{
    const bool mask = mode == WSMode::SERVER;
    for (int on = 0; on < 2; ++on) {
        WSHandler a, b;
        a.setMode(mode), b.setMode(mode);
        a.setProtocolCheck(on != 0, 0x40);
        b.setProtocolCheck(on != 0);
        std::vector<int> ga, gb;
        collect(a, ga), collect(b, gb);
        std::vector<uint8_t> wa = wire_a(mask), wb = wire_b(mask);
        CHECK(a.handleData(wa.data(), 7) == WSError::NEED_MORE_DATA);  // a read that cuts a frame
        CHECK(a.handleData(wa.data() + 7, wa.size() - 7) == WSError::CLOSED);
        CHECK(b.handleData(wb.data(), wb.size()) == WSError::CLOSED);
        expect(ga, kWantA, on != 0);
        expect(gb, kWantB, on != 0);
        CHECK(a.lastFrameProto() == (on ? KMWS_PROTO_CLOSE_REASON : 0));  // the last delivered frame's, as lastFrameUtf8
    }
    // RSV1 that nobody negotiated
    WSHandler c;
    c.setMode(mode);
    c.setProtocolCheck(true);
    std::vector<int> gc;
    collect(c, gc);
    std::vector<uint8_t> wa = wire_a(mask);
    CHECK(c.handleData(wa.data(), wa.size()) == WSError::CLOSED);
    CHECK(gc.size() == 4 && gc[0] == KMWS_PROTO_RSV && gc[3] == KMWS_PROTO_AFTER_FAIL);
}

struct FakeLoop {
    std::deque<std::function<void()>> tasks;
    kmws::RxLoop::Poster poster()
    {
        return [this](kmws::RxLoop::Task t) { tasks.push_back(std::move(t)); };
    }
    void iterate()
    {
        std::deque<std::function<void()>> now;
        now.swap(tasks);
        for (auto& t : now) t();
    }
};

static void with_rx_loop()
{
    for (int on = 0; on < 2; ++on)
        for (int async = 0; async < 2; ++async) {
            FakeLoop loop;
            kmws::RxLoop rx(loop.poster(), 0, async != 0);
            CHECK(rx.valid());
            WSHandler a, b;
            a.setMode(WSMode::SERVER), b.setMode(WSMode::SERVER);
            a.setRxLoop(&rx), b.setRxLoop(&rx);
            a.setProtocolCheck(on != 0, 0x40);
            b.setProtocolCheck(on != 0);
            std::vector<int> ga, gb;
            collect(a, ga), collect(b, gb);
            std::vector<uint8_t> wa = wire_a(true), wb = wire_b(true);
            // two connections in the same generations, a read per loop iteration
            (void)a.handleData(wa.data(), 20);
            (void)b.handleData(wb.data(), 12);
            loop.iterate();
            (void)a.handleData(wa.data() + 20, wa.size() - 20);
            (void)b.handleData(wb.data() + 12, wb.size() - 12);
            for (int spin = 0; spin < 100000 && (rx.inflight() || rx.pending() || !loop.tasks.empty()); ++spin)
                loop.iterate();
            expect(ga, kWantA, on != 0);
            expect(gb, kWantB, on != 0);
        }
}

int main(int argc, char** argv)
{
    const std::string mode = argc > 1 ? argv[1] : "host";
    direct(WSMode::CLIENT);
    if (mode == "gpu") {
        direct(WSMode::SERVER);
        with_rx_loop();
    }
    if (g_fail) {
        std::fprintf(stderr, "%d failures\n", g_fail);
        return 1;
    }
    std::printf("OK\n");
    return 0;
}
