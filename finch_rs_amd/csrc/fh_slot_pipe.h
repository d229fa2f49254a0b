// fh_slot_pipe.h -- the hand-off between the thread that fills a sketcher's two staging buffers ("slots") and the thread that
// pushes what is in them to the device: two slots, one producer, one consumer, jobs in the order they were published.  The
// pipe owns the producer thread and aborts and joins it in its destructor, so that nothing joinable unwinds when the consumer
// leaves by exception.  WHEN a slot may be filled again is the caller's rule (release): a push may return before the device
// has read the slot it was given.  Declare the pipe after everything its producer touches.  Standard library only.
#pragma once

#include <atomic>
#include <chrono>
#include <condition_variable>
#include <deque>
#include <mutex>
#include <thread>
#include <utility>

namespace fh {

template <class Job>
class SlotPipe {
public:
    // starts the producer: body(pipe) runs on it, and the pipe is closed when body returns or throws
    template <class Body>
    explicit SlotPipe(Body body)
        : producer_([this, body = std::move(body)]() mutable {
              bool threw = false;
              try {
                  body(*this);
              } catch (...) {
                  threw = true;
              }
              std::lock_guard<std::mutex> g(mu_);
              threw_ = threw;
              closed_ = true;
              cv_.notify_all();
          }) {}
    ~SlotPipe() {
        abort();
        producer_.join();
    }

    // producer side
    bool acquire(int slot) { // waits until the slot is free; false: aborted (the slot is not taken)
        const Clock::time_point t0 = Clock::now();
        std::unique_lock<std::mutex> lk(mu_);
        cv_.wait(lk, [&] { return free_[slot] || aborted_; });
        producer_waited_ += Clock::now() - t0;
        if (aborted_) return false;
        free_[slot] = false;
        return true;
    }
    void publish(const Job &job) {
        std::lock_guard<std::mutex> g(mu_);
        ready_.push_back(job);
        cv_.notify_all();
    }

    // consumer side
    bool next(Job &job) { // false: the producer is done and nothing is left
        const Clock::time_point t0 = Clock::now();
        std::unique_lock<std::mutex> lk(mu_);
        cv_.wait(lk, [&] { return !ready_.empty() || closed_; });
        consumer_waited_ += Clock::now() - t0;
        if (ready_.empty()) return false;
        job = ready_.front();
        ready_.pop_front();
        return true;
    }
    void release(int slot) { // the slot may be filled again
        std::lock_guard<std::mutex> g(mu_);
        free_[slot] = true;
        cv_.notify_all();
    }
    void abort() { // wakes both sides; acquire() returns false from now on, next() hands out what was published before
        std::lock_guard<std::mutex> g(mu_);
        aborted_ = true;
        cv_.notify_all();
    }
    const std::atomic<bool> &aborted() const { return aborted_; } // (the flag itself: a reader loop can keep an eye on it)
    bool producer_threw() const { // meaningful once next() has returned false
        std::lock_guard<std::mutex> g(mu_);
        return threw_;
    }
    // seconds spent inside acquire() / next(), for the traces
    double producer_waited() const {
        std::lock_guard<std::mutex> g(mu_);
        return producer_waited_.count();
    }
    double consumer_waited() const {
        std::lock_guard<std::mutex> g(mu_);
        return consumer_waited_.count();
    }

private:
    using Clock = std::chrono::steady_clock;
    mutable std::mutex mu_;
    std::condition_variable cv_;
    bool free_[2] = {true, true}, closed_ = false, threw_ = false;
    std::atomic<bool> aborted_{false};
    std::deque<Job> ready_;
    std::chrono::duration<double> producer_waited_{0}, consumer_waited_{0};
    std::thread producer_; // (last: it starts in the constructor's initialiser list and uses everything above)
};

} // namespace fh
