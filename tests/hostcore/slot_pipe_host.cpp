// Driver of tests/test_slot_pipe_host.py: the two-slot hand-off of finch_rs_amd/csrc/fh_slot_pipe.h on its own (nothing else of
// the library), one scenario per run: `slot_pipe_host <scenario>` prints "ok" and returns 0, or says which check failed.
// A "slot" here is a few bytes the producer writes and the consumer reads back, like a staging buffer and its copy to the
// device: a slot handed out too early shows as a failed check, and as a data race under ThreadSanitizer.
#include <atomic>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <new>
#include <stdexcept>
#include <thread>

#include "fh_slot_pipe.h"

#define CHECK(c)                                                                \
    do {                                                                        \
        if (!(c)) {                                                             \
            fprintf(stderr, "line %d: check failed: %s\n", __LINE__, #c);       \
            fflush(stderr);                                                     \
            _Exit(1);                                                           \
        }                                                                       \
    } while (0)

struct Job {
    int slot;
    uint32_t seq;
    bool more; // the slot's acquisition goes on with the next job
};
using Pipe = fh::SlotPipe<Job>;

static constexpr uint32_t N_JOBS = 5000;
static uint32_t slot_data[2][4];          // what the producer fills; plain memory on purpose
static std::atomic<bool> held[2];         // from a successful acquire() until the consumer gives the slot back
static std::atomic<uint32_t> n_taken{0};  // acquisitions made by the producer
static std::atomic<uint32_t> n_given{0};  // ... given back by the consumer (counted just before release())

static void take(Pipe &p, int slot, bool &ok) {
    ok = p.acquire(slot);
    if (!ok) return;
    CHECK(!held[slot].exchange(true)); // never while the consumer still holds it
    CHECK(++n_taken - n_given.load() <= 2); // two slots: never more than two acquisitions ahead of the consumer
}
static void fill(int slot, uint32_t seq) {
    for (uint32_t &w : slot_data[slot]) w = seq;
}
static void check_filled(int slot, uint32_t seq) {
    for (uint32_t w : slot_data[slot]) CHECK(w == seq);
}
static void give(Pipe &p, int slot) {
    CHECK(held[slot].exchange(false));
    ++n_given;
    p.release(slot);
}
static void spin_a_little() { // (lets the other thread reach the wait it was about to enter; either order is a valid run)
    for (int i = 0; i < 200; ++i) std::this_thread::yield();
}

// 1: slots alternate, the consumer releases the job's own slot (the text pump, BGZF)
static void own_slot() {
    Pipe pipe([](Pipe &p) {
        for (uint32_t i = 0; i < N_JOBS; ++i) {
            bool ok;
            take(p, (int)(i & 1), ok);
            CHECK(ok);
            fill((int)(i & 1), i);
            p.publish(Job{(int)(i & 1), i, false});
        }
    });
    uint32_t want = 0;
    for (Job job; pipe.next(job); ++want) {
        CHECK(job.seq == want && job.slot == (int)(want & 1));
        check_filled(job.slot, job.seq);
        give(pipe, job.slot);
    }
    CHECK(want == N_JOBS && !pipe.producer_threw() && !pipe.aborted());
    CHECK(pipe.producer_waited() >= 0 && pipe.consumer_waited() >= 0);
}

// 2: the consumer releases the slot of the job BEFORE this one (the FASTQ host strip): that slot is still being read while
// this job is taken, and must not have changed
static void previous_slot() {
    Pipe pipe([](Pipe &p) {
        for (uint32_t i = 0; i < N_JOBS; ++i) {
            bool ok;
            take(p, (int)(i & 1), ok);
            CHECK(ok);
            fill((int)(i & 1), i);
            p.publish(Job{(int)(i & 1), i, false});
        }
    });
    uint32_t want = 0;
    int prev_slot = -1;
    for (Job job; pipe.next(job); ++want) {
        CHECK(job.seq == want && job.slot == (int)(want & 1));
        check_filled(job.slot, job.seq);
        if (prev_slot >= 0) {
            check_filled(prev_slot, want - 1);
            give(pipe, prev_slot);
        }
        prev_slot = job.slot;
    }
    CHECK(want == N_JOBS && held[prev_slot] && !held[prev_slot ^ 1]);
}

// 3: one acquisition, 1..5 jobs out of it, released after the last (gzip)
static void several_jobs_per_slot() {
    Pipe pipe([](Pipe &p) {
        uint32_t seq = 0;
        for (uint32_t batch = 0; seq < N_JOBS; ++batch) {
            const int slot = (int)(batch & 1);
            bool ok;
            take(p, slot, ok);
            CHECK(ok);
            const uint32_t pieces = 1 + batch % 5;
            for (uint32_t j = 0; j < pieces; ++j, ++seq) {
                slot_data[slot][j % 4] = seq; // (a piece: the earlier ones of the batch stay as they are)
                p.publish(Job{slot, seq, j + 1 < pieces});
            }
        }
    });
    uint32_t want = 0, batch = 0, piece = 0;
    for (Job job; pipe.next(job); ++want) {
        CHECK(job.seq == want && job.slot == (int)(batch & 1) && job.more == (piece + 1 < 1 + batch % 5));
        CHECK(held[job.slot]);
        if (job.more) {
            ++piece;
            continue;
        }
        for (uint32_t j = 0; j <= piece; ++j) // this batch's pieces, not those of the batch that gets the slot next
            CHECK(slot_data[job.slot][j % 4] >= want - piece && slot_data[job.slot][j % 4] <= want);
        give(pipe, job.slot);
        ++batch;
        piece = 0;
    }
    CHECK(want >= N_JOBS && n_taken == n_given);
}

// 4: abort() while the producer waits in acquire(): acquire() fails, what was published still arrives, then the end
static void abort_blocked_producer() {
    std::atomic<bool> about_to_block{false}, refused{false};
    {
        Pipe pipe([&](Pipe &p) {
            for (uint32_t i = 0;; ++i) {
                if (i == 2) about_to_block = true;
                bool ok;
                take(p, (int)(i & 1), ok);
                if (!ok) break;
                CHECK(i < 2); // nothing is released: the third acquire() can only fail
                p.publish(Job{(int)(i & 1), i, false});
            }
            refused = true;
        });
        while (!about_to_block) std::this_thread::yield();
        spin_a_little();
        pipe.abort();
        CHECK(pipe.aborted());
        Job job;
        CHECK(pipe.next(job) && job.seq == 0);
        CHECK(pipe.next(job) && job.seq == 1);
        CHECK(!pipe.next(job));
        CHECK(refused && !pipe.producer_threw());
        CHECK(!pipe.next(job)); // (and stays so)
    }
}

// 5: a producer with nothing to say
static void empty_producer() {
    Pipe pipe([](Pipe &) {});
    Job job;
    CHECK(!pipe.next(job) && !pipe.producer_threw() && !pipe.aborted());
}

// 6: the consumer leaves by exception; the pipe's destructor stops and joins the producer (a joinable std::thread that unwinds
// would end the process)
static void consumer_throws(bool producer_blocked) {
    std::atomic<bool> about_to_block{false}, producer_left{false};
    bool caught = false;
    try {
        Pipe pipe([&](Pipe &p) {
            for (uint32_t i = 0;; ++i) {
                if (i == 2) about_to_block = true;
                bool ok;
                take(p, (int)(i & 1), ok);
                if (!ok) break;
                fill((int)(i & 1), i);
                p.publish(Job{(int)(i & 1), i, false});
            }
            producer_left = true;
        });
        Job job;
        if (producer_blocked) { // nothing is released: the producer gets as far as its third acquire()
            while (!about_to_block) std::this_thread::yield();
            spin_a_little();
        } else { // the producer is kept busy publishing
            for (uint32_t i = 0; i < 1000; ++i) {
                CHECK(pipe.next(job) && job.seq == i);
                give(pipe, job.slot);
            }
        }
        throw std::runtime_error("the consumer gives up");
    } catch (const std::runtime_error &) {
        caught = true;
    }
    CHECK(caught && producer_left);
}

// 7: the producer's body throws: the pipe is closed, and says so
static void producer_throws() {
    Pipe pipe([](Pipe &p) {
        bool ok;
        take(p, 0, ok);
        CHECK(ok);
        p.publish(Job{0, 0, false});
        throw std::bad_alloc();
    });
    Job job;
    CHECK(pipe.next(job) && job.seq == 0);
    CHECK(!pipe.next(job));
    CHECK(pipe.producer_threw());
}

int main(int argc, char **argv) {
    const int scenario = argc > 1 ? atoi(argv[1]) : 0;
    switch (scenario) {
    case 1: own_slot(); break;
    case 2: previous_slot(); break;
    case 3: several_jobs_per_slot(); break;
    case 4: abort_blocked_producer(); break;
    case 5: empty_producer(); break;
    case 6:
        consumer_throws(true);
        held[0] = held[1] = false;
        n_taken = n_given = 0;
        consumer_throws(false);
        break;
    case 7: producer_throws(); break;
    default: fprintf(stderr, "usage: slot_pipe_host 1..7\n"); return 2;
    }
    puts("ok");
    return 0;
}
