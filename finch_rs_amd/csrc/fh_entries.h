// fh_entries.h -- what the library calls (fh_library.cpp) share around their device entries: one host thread per entry
// (for_entries), the first error any of them meets (EntryError), and the loop that keeps launch m + 1 on the device while the
// host takes the result of launch m (two_slot).  What an entry opens, launches and makes of a result is the call's own.
// Standard library only.
#pragma once

#include <atomic>
#include <cstddef>
#include <mutex>
#include <new>
#include <string>
#include <thread>
#include <utility>
#include <vector>

namespace fh {

// job(t) for t = 0 .. n - 1, one thread each (the caller's runs job(0)).  A thread that cannot be created (EAGAIN under a
// thread limit) must not take the process down -- a vector of joinable threads that unwinds calls std::terminate -- so its
// share runs on the calling thread instead.
template <class J>
static void fork_join(unsigned n, J job) {
    std::vector<std::thread> th;
    th.reserve(n ? n - 1 : 0); // (before the first thread exists: may throw freely)
    unsigned started = 1;
    try {
        for (; started < n; ++started) th.emplace_back(job, started);
    } catch (...) {
    }
    if (n) job(0u);
    for (unsigned t = started; t < n; ++t) job(t);
    for (auto &x : th) x.join();
}

// The first error of a call's entries wins; the others see failed() and stop early.  rc() and msg() are for the caller, once
// the entries have joined.  (Hidden: the shared library exports nothing of it.)
class __attribute__((visibility("hidden"))) EntryError {
public:
    void fail(int rc, std::string msg) {
        std::lock_guard<std::mutex> g(mu_);
        if (rc_ == 0) rc_ = rc, msg_ = std::move(msg);
        failed_ = true;
    }
    bool failed() const { return failed_; }
    int rc() const { return rc_; }
    const std::string &msg() const { return msg_; }

private:
    std::mutex mu_;
    int rc_ = 0;
    std::string msg_;
    std::atomic<bool> failed_{false};
};

// f() when the scope is left, by whatever way: an entry's close of its device object
template <class F>
struct Finally {
    F f;
    ~Finally() { f(); }
};
template <class F>
Finally(F) -> Finally<F>;

// body(e) for e = 0 .. n_entries - 1 on a thread each (fork_join); an entry that runs out of host memory fails the call with
// capacity_rc and leaves the others to finish
template <class Body>
static void for_entries(unsigned n_entries, EntryError &err, int capacity_rc, Body body) {
    fork_join(n_entries, [&](unsigned e) {
        try {
            body(e);
        } catch (const std::bad_alloc &) {
            err.fail(capacity_rc, "out of host memory");
        }
    });
}

// launch(m, slot) for m = 0 .. n - 1 into the slots m & 1, take(m, slot) -- the wait and the host's work -- after
// launch(m + 1): the device works on m + 1 while the host takes m.  Both return 0 or an error, the first of which ends the loop
// and is handed back; so does another entry's failure, seen before a take, with 0.
template <class Launch, class Take>
static int two_slot(size_t n, const EntryError &err, Launch launch, Take take) {
    int rc = n ? launch((size_t)0, 0) : 0;
    for (size_t m = 0; rc == 0 && m < n && !err.failed(); ++m) {
        if (m + 1 < n && (rc = launch(m + 1, (int)((m + 1) & 1))) != 0) break;
        rc = take(m, (int)(m & 1));
    }
    return rc;
}

} // namespace fh
