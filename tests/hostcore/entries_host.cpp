// Driver of tests/test_entries_host.py: what the library calls share around their device entries
// (finch_rs_amd/csrc/fh_entries.h) on its own (nothing else of the library), one scenario per run: `entries_host <scenario>`
// prints "ok" and returns 0, or says which check failed.  The launches and takes are fakes that log (kind, m, slot).
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <mutex>
#include <new>
#include <string>
#include <thread>
#include <vector>

#include "fh_entries.h"

#define CHECK(c)                                                                \
    do {                                                                        \
        if (!(c)) {                                                             \
            fprintf(stderr, "line %d: check failed: %s\n", __LINE__, #c);       \
            fflush(stderr);                                                     \
            _Exit(1);                                                           \
        }                                                                       \
    } while (0)

static constexpr int CAPACITY = -5; // (any code: the header knows none of the library's)

// a run of two_slot over fakes: launch m fails with -7 where m == bad_launch, take m where m == bad_take; the log as text
struct Run {
    std::string log;
    int rc = 0;
};
static Run run_two_slot(size_t n, fh::EntryError &err, long bad_launch = -1, long bad_take = -1, long fail_elsewhere_in_take = -1) {
    Run r;
    auto note = [&](char kind, size_t m, int slot) {
        CHECK(slot == (int)(m & 1));
        r.log += (r.log.empty() ? "" : " ") + std::string(1, kind) + std::to_string(m);
    };
    r.rc = fh::two_slot(
        n, err,
        [&](size_t m, int slot) {
            note('L', m, slot);
            return (long)m == bad_launch ? -7 : 0;
        },
        [&](size_t m, int slot) {
            note('T', m, slot);
            if ((long)m == fail_elsewhere_in_take) // another entry fails while this one is between two iterations
                std::thread([&] { err.fail(-9, "elsewhere"); }).join();
            return (long)m == bad_take ? -8 : 0;
        });
    return r;
}

// 1: the order of launches and takes, the slots (checked in note())
static void two_slot_order() {
    const char *want[] = {"", "L0 T0", "L0 L1 T0 T1", "", "", "L0 L1 T0 L2 T1 L3 T2 L4 T3 T4"};
    for (size_t n : {0, 1, 2, 5}) {
        fh::EntryError err;
        const Run r = run_two_slot(n, err);
        CHECK(r.rc == 0 && r.log == want[n] && !err.failed());
    }
}

// 2: launch 3 fails: take 2 is not called, nothing later runs, the code comes back
static void launch_fails() {
    fh::EntryError err;
    const Run r = run_two_slot(5, err, 3);
    CHECK(r.rc == -7 && r.log == "L0 L1 T0 L2 T1 L3");
    CHECK(!err.failed()); // (reporting it is the caller's business)
    fh::EntryError err0;
    const Run first = run_two_slot(5, err0, 0);
    CHECK(first.rc == -7 && first.log == "L0");
}

// 3: take 1 fails: launch 2 has happened before it, launch 3 and take 2 have not
static void take_fails() {
    fh::EntryError err;
    const Run r = run_two_slot(5, err, -1, 1);
    CHECK(r.rc == -8 && r.log == "L0 L1 T0 L2 T1");
}

// 4: another thread's fail() between two iterations: 0, and no further launch
static void failure_elsewhere() {
    fh::EntryError err;
    const Run r = run_two_slot(5, err, -1, -1, 1);
    CHECK(r.rc == 0 && r.log == "L0 L1 T0 L2 T1");
    CHECK(err.failed() && err.rc() == -9 && err.msg() == "elsewhere");
    const Run none = run_two_slot(5, err); // failed before the first iteration: the first launch is out, nothing is taken
    CHECK(none.rc == 0 && none.log == "L0");
}

// 5: sixteen threads fail at once: one pair survives, and it is one thread's pair
static void error_under_contention() {
    for (int round = 0; round < 200; ++round) {
        fh::EntryError err;
        std::atomic<bool> go{false};
        fh::fork_join(16, [&](unsigned t) {
            if (t == 0) go = true;
            while (!go) std::this_thread::yield();
            err.fail(-100 - (int)t, "thread " + std::to_string(t));
            CHECK(err.failed());
        });
        CHECK(err.failed() && err.rc() <= -100 && err.rc() > -116);
        CHECK(err.msg() == "thread " + std::to_string(-100 - err.rc()));
    }
    fh::EntryError none;
    CHECK(!none.failed() && none.rc() == 0 && none.msg().empty());
}

// 6: for_entries: every entry once, entry 0 on the caller's thread; one entry throws bad_alloc, one returns early; the cleanup
// of each runs once
static void entries() {
    for (unsigned n : {1u, 3u, 16u}) {
        const unsigned thrower = n - 1, early = n / 2; // (n = 1: the one entry throws)
        fh::EntryError err;
        std::vector<std::atomic<int>> ran(n), cleaned(n), finished(n);
        const std::thread::id caller = std::this_thread::get_id();
        fh::for_entries(n, err, CAPACITY, [&](unsigned e) {
            CHECK(e < n);
            ++ran[e];
            fh::Finally cleanup{[&] { ++cleaned[e]; }};
            if (e == 0) CHECK(std::this_thread::get_id() == caller);
            if (e == thrower) throw std::bad_alloc();
            if (e == early) return;
            ++finished[e];
        });
        for (unsigned e = 0; e < n; ++e) {
            CHECK(ran[e] == 1 && cleaned[e] == 1);
            CHECK(finished[e] == (e == thrower || e == early ? 0 : 1));
        }
        CHECK(err.failed() && err.rc() == CAPACITY && err.msg() == "out of host memory");
    }
    fh::EntryError err;
    unsigned ran = 0;
    fh::for_entries(0, err, CAPACITY, [&](unsigned) { ++ran; });
    fh::for_entries(4, err, CAPACITY, [&](unsigned) {});
    CHECK(ran == 0 && !err.failed());
}

int main(int argc, char **argv) {
    const int scenario = argc > 1 ? atoi(argv[1]) : 0;
    switch (scenario) {
    case 1: two_slot_order(); break;
    case 2: launch_fails(); break;
    case 3: take_fails(); break;
    case 4: failure_elsewhere(); break;
    case 5: error_under_contention(); break;
    case 6: entries(); break;
    default: fprintf(stderr, "usage: entries_host 1..6\n"); return 2;
    }
    puts("ok");
    return 0;
}
