// Thread check of the plain-C++ part of csrc/hnr_launch.h (LdsLimit, PerDeviceValue, knob): host code only, no HIP runtime, no GPU.
//   clang++ -std=c++17 -O1 -g -fsanitize=thread -pthread tools/launch_state_check.cpp -o /tmp/launch_state_check && /tmp/launch_state_check
// Run by hand on a CPU machine; prints "launch_state_check: ok" and exits 0, or says what failed (ThreadSanitizer reports races itself).
#include <stdio.h>
#include <thread>
#include <vector>

#include "../hybridneuralrendering_amd/csrc/hnr_launch.h"

using namespace hnr;

static std::atomic<int> failures{0};
#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "FAILED line %d: %s\n", __LINE__, #cond); ++failures; } } while (0)

constexpr int THREADS = 8, ROUNDS = 20000, DEVICES = 5;

template <class F> static void in_threads(F &&f)
{
    std::vector<std::thread> th;
    for (int t = 0; t < THREADS; ++t) th.emplace_back(f, t);
    for (auto &x : th) x.join();
}

static int cached_knob() { static const int v = knob("HNR_CHECK_KNOB", 1, 0, 100); return v; }      // the call-site idiom of the library

int main()
{
    // ---- one successful set per device, and no "launch" (a return of 0) before it
    {
        LdsLimit lim;
        std::atomic<int> sets[DEVICES] = {}, early{0};
        std::atomic<int> set_done[DEVICES] = {};                  // what the stub has finished setting (stands for the runtime's own state)
        in_threads([&](int t) {
            for (int i = 0; i < ROUNDS; ++i) {
                const int dev = (i + t) % DEVICES;
                const int rc = lim.raise(dev, 100 * 1024, [&](int bytes) {
                    sets[dev].fetch_add(1);
                    std::this_thread::yield();                    // a slow attribute call: the other threads arrive meanwhile
                    set_done[dev].store(bytes);
                    return 0;
                });
                if (rc != 0 || set_done[dev].load() < 100 * 1024) early.fetch_add(1);      // this is where the kernel would be launched
            }
        });
        for (int d = 0; d < DEVICES; ++d) { CHECK(sets[d].load() == 1); CHECK(lim.limit(d) == 100 * 1024); }
        CHECK(early.load() == 0);
        CHECK(lim.limit(DEVICES) == -1);                          // an unused device stays unset
        // a later call that asks for more sets again, once; one that asks for less does not
        int again = 0;
        CHECK(lim.raise(0, 120 * 1024, [&](int) { ++again; return 0; }) == 0);
        CHECK(lim.raise(0, 64 * 1024, [&](int) { ++again; return 0; }) == 0);
        CHECK(again == 1 && lim.limit(0) == 120 * 1024);
        // a device index outside the table: set every time, nothing recorded
        again = 0;
        CHECK(lim.raise(-1, 1024, [&](int) { ++again; return 0; }) == 0 && lim.raise(MAX_DEVICES, 1024, [&](int) { ++again; return 0; }) == 0 && again == 2);
    }
    // ---- a failed set leaves the object not done: every caller sees the error until a set succeeds, and only then a 0
    {
        LdsLimit lim;
        std::atomic<int> fail_left{50}, ok_sets{0}, errors{0}, early{0}, set_done{0};
        in_threads([&](int) {
            for (int i = 0; i < ROUNDS; ++i) {
                const int rc = lim.raise(3, 80 * 1024, [&](int bytes) {
                    if (fail_left.fetch_sub(1) > 0) return 719;   // an error code of the runtime's
                    ok_sets.fetch_add(1);
                    set_done.store(bytes);
                    return 0;
                });
                if (rc != 0) { errors.fetch_add(1); CHECK(rc == 719); }
                else if (set_done.load() < 80 * 1024) early.fetch_add(1);
            }
        });
        CHECK(errors.load() == 50 && ok_sets.load() == 1 && early.load() == 0 && lim.limit(3) == 80 * 1024);
        LdsLimit never;
        CHECK(never.raise(0, 1024, [](int) { return 1; }) == 1 && never.limit(0) == -1);
    }
    // ---- the per-device value: every thread gets the queried value; a failed query gives the fallback
    {
        PerDeviceValue v;
        std::atomic<int> wrong{0};
        in_threads([&](int t) {
            for (int i = 0; i < ROUNDS; ++i) {
                const int dev = (i + t) % DEVICES;
                if (v.get(dev, 256, [](int d) { return 100 + d; }) != 100 + dev) wrong.fetch_add(1);
            }
        });
        CHECK(wrong.load() == 0);
        PerDeviceValue f;
        CHECK(f.get(0, 256, [](int) { return 0; }) == 256 && f.get(-1, 256, [](int) { return 7; }) == 256);
    }
    // ---- knob: read once under threads, clamped; knob_now follows the environment
    {
        setenv("HNR_CHECK_KNOB", "250", 1);
        std::atomic<int> wrong{0};
        in_threads([&](int) { for (int i = 0; i < ROUNDS; ++i) if (cached_knob() != 100) wrong.fetch_add(1); });
        CHECK(wrong.load() == 0);
        setenv("HNR_CHECK_KNOB", "7", 1);
        CHECK(cached_knob() == 100);                              // read once per process
        CHECK(knob_now("HNR_CHECK_KNOB", 1) == 7 && knob_now("HNR_CHECK_KNOB", 1, 10, 20) == 10);
        unsetenv("HNR_CHECK_KNOB");
        CHECK(knob_now("HNR_CHECK_KNOB", 25, 0, 400) == 25 && knob_now("HNR_CHECK_KNOB", 1) == 1);
        setenv("HNR_CHECK_KNOB", "abc", 1);
        CHECK(knob_now("HNR_CHECK_KNOB", 5) == 0);                // atoi
    }
    if (failures) { fprintf(stderr, "launch_state_check: %d check(s) failed\n", failures.load()); return 1; }
    printf("launch_state_check: ok (%d threads x %d rounds)\n", THREADS, ROUNDS);
    return 0;
}
