// include/kmws_wshandler.hpp's UTF-8 check (setUtf8Check / lastFrameUtf8) the
// way a kuma server would use it: a SERVER-mode handler receives masked text
// messages, reads lastFrameUtf8() inside its frame callback and would close
// with 1007 on KMWS_UTF8_BAD.  One BAD and one OK message, fragmented so that a
// code point straddles two frames, without an RxLoop (one GPU batch per
// handleData) and with one (frames delivered by the loop's posted task).
//   host: no GPU needed -- empty frames, and the check switched off
//   gpu:  the above
// Build: tests/test_wshandler_utf8.py.
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

struct Rec {
    int opcode, fin, utf8;
    std::string payload;
};

static void collect(WSHandler& h, std::vector<Rec>& out)
{
    h.setFrameCallback([&h, &out](FrameHeader hdr, BufferChain& buf) {
        out.push_back(Rec{hdr.opcode, hdr.fin, h.lastFrameUtf8(),
                          std::string(static_cast<const char*>(buf.readPtr()), buf.length())});
        return 0;
    });
}

static std::vector<uint8_t> frame(int opcode, int fin, const std::string& payload, bool mask, uint8_t k0)
{
    const uint8_t key[4] = {k0, 0x5a, 0xc3, 0x0f};
    FrameHeader h;
    std::memset(static_cast<void*>(&h), 0, sizeof(h));
    h.fin = fin;
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

// The wire of one connection: a BAD message (a lone continuation byte in its
// second fragment, a PING in between, a third fragment after it), then an OK
// message whose U+00E9 straddles its two fragments, then a binary frame of FFs.
static std::vector<uint8_t> wire(bool mask)
{
    std::vector<uint8_t> w;
    append(w, frame(1, 0, std::string(300, 'a') + "\xc3", mask, 1));
    append(w, frame(9, 1, "\xff\xfe", mask, 2));
    append(w, frame(0, 0, "\xa9 then \x80 alone", mask, 3));
    append(w, frame(0, 1, "tail", mask, 4));
    append(w, frame(1, 0, std::string(5000, 'b') + "\xc3", mask, 5));
    append(w, frame(0, 1, "\xa9" + std::string(70, 'c'), mask, 6));
    append(w, frame(2, 1, std::string(64, '\xff'), mask, 7));
    return w;
}
static const int kWant[7] = {KMWS_UTF8_OK,  KMWS_UTF8_NOT_TEXT, KMWS_UTF8_BAD,     KMWS_UTF8_AFTER_BAD,
                             KMWS_UTF8_OK,  KMWS_UTF8_OK,       KMWS_UTF8_NOT_TEXT};

static void check_verdicts(const std::vector<Rec>& got, bool on)
{
    CHECK(got.size() == 7);
    for (size_t i = 0; i < got.size() && i < 7; ++i) CHECK(got[i].utf8 == (on ? kWant[i] : 0));
    if (got.size() == 7) {
        CHECK(got[2].payload == "\xa9 then \x80 alone" && got[5].payload == "\xa9" + std::string(70, 'c'));
        CHECK(got[6].payload == std::string(64, '\xff'));
    }
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

static void gpu_checks()
{
    for (int on = 0; on < 2; ++on) {
        // without an RxLoop: one GPU batch per handleData, reads cut mid-frame
        {
            WSHandler h;
            h.setMode(WSMode::SERVER);
            h.setUtf8Check(on != 0);
            std::vector<Rec> got;
            collect(h, got);
            std::vector<uint8_t> w = wire(true);
            const size_t cut = 200;
            CHECK(h.handleData(w.data(), cut) == WSError::NEED_MORE_DATA);
            CHECK(h.handleData(w.data() + cut, w.size() - cut) == WSError::NOERR);
            check_verdicts(got, on != 0);
        }
        // with an RxLoop, asynchronous and synchronous: delivered by the loop's task
        for (int async = 0; async < 2; ++async) {
            FakeLoop loop;
            kmws::RxLoop rx(loop.poster(), 0, async != 0);
            CHECK(rx.valid());
            WSHandler h;
            h.setMode(WSMode::SERVER);
            h.setRxLoop(&rx);
            h.setUtf8Check(on != 0);
            std::vector<Rec> got;
            collect(h, got);
            std::vector<uint8_t> w = wire(true);
            // a read per loop iteration: the message state crosses generations
            const size_t cuts[4] = {0, 320, 5400, w.size()};
            for (int i = 0; i < 3; ++i) {
                const WSError r = h.handleData(w.data() + cuts[i], cuts[i + 1] - cuts[i]);
                CHECK(r == WSError::NOERR || r == WSError::NEED_MORE_DATA);
                loop.iterate();
            }
            for (int spin = 0; spin < 100000 && (rx.inflight() || rx.pending() || !loop.tasks.empty()); ++spin)
                loop.iterate();
            check_verdicts(got, on != 0);
        }
    }
}

static void host_checks()
{
    // CLIENT mode, empty frames: no GPU work
    for (int on = 0; on < 2; ++on) {
        WSHandler h;
        h.setUtf8Check(on != 0);
        std::vector<Rec> got;
        collect(h, got);
        std::vector<uint8_t> w;
        append(w, frame(1, 1, "", false, 0));
        append(w, frame(9, 1, "", false, 0));
        append(w, frame(2, 1, "", false, 0));
        CHECK(h.handleData(w.data(), w.size()) == WSError::NOERR);
        CHECK(got.size() == 3);
        if (got.size() == 3) {
            CHECK(got[0].utf8 == (on ? KMWS_UTF8_OK : 0));
            CHECK(got[1].utf8 == 0 && got[2].utf8 == 0);
        }
    }
}

int main(int argc, char** argv)
{
    const std::string mode = argc > 1 ? argv[1] : "host";
    host_checks();
    if (mode == "gpu") gpu_checks();
    if (g_fail) {
        std::fprintf(stderr, "%d failures\n", g_fail);
        return 1;
    }
    std::printf("OK\n");
    return 0;
}
