// batch_order.hpp -- the ORDER of a file run's batches and nothing about what a batch is: which stage of which batch may run
// when, on which thread, and what becomes of a failure.  Host-only (no HIP include; tests/model/batch_order_tsan.cpp drives it
// with fake stages under the thread sanitizer).  file_pipeline.hpp supplies the stages:
//   acquire(k, slot) -> reads of batch k now in the slot: 0 = no further batch, < 0 = failure;  on helper threads, two batches
//     ahead; with serial_acquire in batch order and never two at a time (a one-pass reader), else as the threads come;
//   pack(k, slot)    -> the slot made ready for the device, behind the batch's acquire on the same thread;
//   enqueue(k, slot) -> on the calling thread, in batch order, the moment the batch is packed;
//   collect(k, slot) -> on a helper thread per batch: everything up to the ordered point (the wait for the device, the text);
//   write(k, slot)   -> behind it: batch k only after batches 0 .. k-1 are through (written, or given up on).
// mark(what, k) sees the stage boundaries (the trace).  The stages return 0 or a failure code; one that fails leaves its message in slot.err,
// one that throws fails with rc_thrown (no exception leaves a task unseen).  A slot carries a batch through all stages and is reused
// n_slots (>= 3) batches later: batch k is packed only after batch k - n_slots is through (`written` counts those).
// The run's failure is kept HERE, not in the slots: the first one recorded wins and is never cleared or overwritten.  From
// then on no batch behind a failed one (`stop_at`: the first) is acquired, enqueued or written; the batches ahead of it still
// leave in order, every task still ends, and the call returns that code and (in err) that message.
#pragma once
#include <condition_variable>
#include <cstdint>
#include <exception>
#include <future>
#include <mutex>
#include <string>
#include <vector>

template <class Slot, class Acquire, class Pack, class Enqueue, class Collect, class Write, class Mark>
int run_batches_in_order(Slot *const *slots, int n_slots, bool serial_acquire, int rc_thrown, Acquire acquire, Pack pack, Enqueue enqueue,
                         Collect collect, Write write, Mark mark, std::string &err)
{
    std::mutex gate_m;
    std::condition_variable gate_cv;
    int64_t written = 0, acquired = 0, stop_at = INT64_MAX;
    int run_rc = 0;
    auto wait_for = [&](int64_t &counter, int64_t upto) {
        std::unique_lock<std::mutex> lk(gate_m);
        gate_cv.wait(lk, [&] { return counter >= upto; });
    };
    auto bump = [&](int64_t &counter) {
        { std::lock_guard<std::mutex> lk(gate_m); counter++; }
        gate_cv.notify_all();
    };
    auto failed_before = [&](int64_t k) { std::lock_guard<std::mutex> lk(gate_m); return stop_at < k; };
    // a stage of batch k: true if it failed (the failure is recorded)
    auto fails = [&](int64_t k, Slot &s, const char *what, auto &&stage) {
        int rc;
        try { rc = stage(); }
        catch (const std::exception &e) { s.err = std::string(what) + e.what(); rc = rc_thrown; }
        if (!rc) return false;
        std::lock_guard<std::mutex> lk(gate_m);
        s.rc = rc;
        if (!run_rc) { run_rc = rc; err = s.err; }
        if (k < stop_at) stop_at = k;
        return true;
    };
    std::vector<std::future<void>> packed, posted;
    auto start_pack = [&](int64_t k) {
        packed.push_back(std::async(std::launch::async, [&, k] {
            Slot &s = *slots[k % n_slots];
            if (k >= n_slots) wait_for(written, k - n_slots + 1);          // the slot's previous batch is through
            if (serial_acquire) wait_for(acquired, k);
            s.rc = 0;
            int64_t m = s.m = 0;
            bool failed = failed_before(k);
            if (!failed) {
                mark("acquire begins", k);
                failed = fails(k, s, "batch preparation: ", [&] { m = acquire(k, s); return m < 0 ? (int)m : 0; });
                mark("acquired", k);
            }
            if (serial_acquire) bump(acquired);                            // (the batches behind this one must not wait for ever)
            if (!failed && m > 0) { s.m = m; fails(k, s, "batch preparation: ", [&] { return pack(k, s); }); }
            mark("packed", k);
        }));
    };
    auto start_post = [&](int64_t k) {
        posted.push_back(std::async(std::launch::async, [&, k] {
            Slot &s = *slots[k % n_slots];
            const bool failed = fails(k, s, "SAM text of a batch: ", [&] { return collect(k, s); });
            wait_for(written, k);                                          // records in input order
            if (!failed && !failed_before(k)) {
                fails(k, s, "SAM text of a batch: ", [&] { return write(k, s); });
                mark("written", k);
            }
            bump(written);
        }));
    };
    for (int64_t k : {0, 1}) start_pack(k);
    for (int64_t k = 0;; k++) {
        Slot &s = *slots[k % n_slots];
        packed[(size_t)k].wait();
        if (failed_before(k + 1) || s.m == 0) break;                       // batch k or one before it failed, or the source is exhausted
        start_pack(k + 2);
        mark("enqueue begins", k);
        if (fails(k, s, "batch preparation: ", [&] { return enqueue(k, s); })) break;
        mark("enqueued", k);
        start_post(k);
    }
    for (auto &f : packed) f.wait();
    for (auto &f : posted) f.wait();
    return run_rc;
}
