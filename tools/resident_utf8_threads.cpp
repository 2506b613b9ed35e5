// kuma's call pattern on T = 1 and T = 8 loop threads with
// kmws_decoder_set_utf8_check off and on, without an interpreter lock between
// the threads (tools/bench_resident_utf8.py measures the same workload from
// Python threads, whose bookkeeping at eight threads costs more than a flush).
// Each thread owns a SERVER-mode decoder and a pinned 64 KiB read buffer; one
// read = 16 (or argv[3]) masked FIN frames of 4 KiB, restored untimed before each call and
// unmasked (and checked) in place by kmws_decoder_feed.  Texts: all ASCII;
// mixed 1-3-byte; the mixed bytes marked binary.  One JSON line per row: each
// thread's median call time and the aggregate rate sum(wire bytes / median).
// Uses only entries older than the resident worker's check, so one binary
// measures any build through LD_LIBRARY_PATH.
//
//   g++ -std=c++17 -O2 -I include tools/resident_utf8_threads.cpp -L kuma_amd/lib -lkmws_gpu -lpthread
//       (one line) -o tools/resident_utf8_threads
//   tools/resident_utf8_threads [calls=2000] [warmup=200] [frames per read=16, 1..16]
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "kmws_gpu.h"

namespace {

using Clock = std::chrono::steady_clock;
int kFrames = 16;  // per read (argv[3])
constexpr size_t kLen = 4096;

std::vector<uint8_t> body_of(const std::string& kind)
{
    std::vector<uint8_t> b;
    if (kind == "ascii") {
        for (size_t i = 0; i < kLen; ++i) b.push_back((uint8_t)(0x20 + (i * 7) % 0x5F));
        return b;
    }
    static const uint8_t unit[18] = {'a', 0xC3, 0xA9, 'b', 'c', 0xE2, 0x82, 0xAC, 'd', 0xC3, 0xA9,
                                     'e', 0xE2, 0x82, 0xAC, 'f', 0xC3, 0xA9};
    while (b.size() + sizeof unit <= kLen) b.insert(b.end(), unit, unit + sizeof unit);
    b.resize(kLen, '.');
    return b;
}

std::vector<uint8_t> wire_of(const std::string& kind, int tid)
{
    const std::vector<uint8_t> body = body_of(kind);
    std::vector<uint8_t> w;
    for (int f = 0; f < kFrames; ++f) {
        const uint8_t key[4] = {(uint8_t)(0x37 + 11 * tid + f), 0xfa, (uint8_t)(0x21 + f), 0x3d};
        w.push_back(kind == "binary" ? 0x82 : 0x81);
        w.push_back(0x80 | 126);
        w.push_back((uint8_t)(kLen >> 8));
        w.push_back((uint8_t)(kLen & 0xFF));
        w.insert(w.end(), key, key + 4);
        for (size_t i = 0; i < kLen; ++i) w.push_back(body[i] ^ key[i & 3]);
    }
    return w;
}

struct Seen {
    int frames = 0, ok = 0;
};
int on_frame(const kmws_frame_hdr* h, uint8_t*, size_t, void* user)
{
    Seen* s = static_cast<Seen*>(user);
    s->frames++;
    s->ok += kmws_frame_utf8(h) == KMWS_UTF8_OK;
    return 0;
}

bool row(int T, const std::string& kind, int check, int calls, int warmup)
{
    std::atomic<int> ready{0}, bad{0};
    std::atomic<bool> go{false};
    std::vector<double> med(T, 0.0);
    std::vector<std::thread> th;
    size_t wire_bytes = 0;
    for (int t = 0; t < T; ++t)
        th.emplace_back([&, t] {
            const std::vector<uint8_t> wire = wire_of(kind, t);
            if (t == 0) wire_bytes = wire.size();
            uint8_t* buf = static_cast<uint8_t*>(kmws_host_alloc(wire.size(), 0));
            kmws_decoder* dec = kmws_decoder_create(KMWS_MODE_SERVER, 0);
            if (!buf || !dec) std::exit(3);
            kmws_decoder_set_utf8_check(dec, check);
            Seen seen;
            std::vector<double> lat;
            lat.reserve(calls);
            auto call = [&](bool timed) {
                std::memcpy(buf, wire.data(), wire.size());  // recv (untimed)
                const auto t0 = Clock::now();
                const int rc = kmws_decoder_feed(dec, buf, wire.size(), on_frame, &seen);
                const double s = std::chrono::duration<double>(Clock::now() - t0).count();
                if (rc != 0) bad.fetch_add(1);
                if (timed) lat.push_back(s);
            };
            for (int i = 0; i < warmup; ++i) call(false);
            ready.fetch_add(1);
            while (!go.load(std::memory_order_acquire)) std::this_thread::yield();
            for (int i = 0; i < calls; ++i) call(true);
            const int want_ok = check && kind != "binary" ? seen.frames : 0;
            if (seen.frames != kFrames * (warmup + calls) || seen.ok != want_ok) bad.fetch_add(1);
            std::sort(lat.begin(), lat.end());
            med[t] = lat[lat.size() / 2];
            kmws_decoder_destroy(dec);
            kmws_host_free(buf);
        });
    while (ready.load() < T) std::this_thread::yield();
    go.store(true, std::memory_order_release);
    for (auto& x : th) x.join();
    double agg = 0;
    std::string per = "[";
    for (int t = 0; t < T; ++t) {
        agg += (double)wire_bytes / med[t];
        char b[32];
        std::snprintf(b, sizeof b, "%s%.2f", t ? ", " : "", med[t] * 1e6);
        per += b;
    }
    per += "]";
    std::vector<double> m = med;
    std::sort(m.begin(), m.end());
    std::printf("{\"case\": \"resident_utf8_threads\", \"threads\": %d, \"payload\": \"%s\", \"check\": %d, "
                "\"frames\": %d, \"calls\": %d, \"median_us\": %.2f, \"thread_median_us\": %s, \"agg_gib_s\": %.3f, \"verified\": %s}\n",
                T, kind.c_str(), check, kFrames, calls, m[m.size() / 2] * 1e6, per.c_str(), agg / (1u << 30),
                bad.load() == 0 ? "true" : "false");
    std::fflush(stdout);
    return bad.load() == 0;
}

}  // namespace

int main(int argc, char** argv)
{
    const int calls = argc > 1 ? std::max(200, std::atoi(argv[1])) : 2000;
    const int warmup = argc > 2 ? std::max(1, std::atoi(argv[2])) : 200;
    if (argc > 3) kFrames = std::min(16, std::max(1, std::atoi(argv[3])));
    if (kmws_device_count() < 1) {
        std::printf("{\"error\": \"no gfx950 device\"}\n");
        return 1;
    }
    bool ok = true;
    // every check-off row first: from its first checked job on, a process's grid
    // is the validating instantiation, also for its unchecked jobs
    for (int check : {0, 1})
        for (int T : {1, 8})
            for (const char* kind : {"ascii", "mixed", "binary"}) ok = row(T, kind, check, calls, warmup) && ok;
    return ok ? 0 : 1;
}
