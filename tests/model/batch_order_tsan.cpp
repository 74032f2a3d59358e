// batch_order_tsan.cpp -- npore_amd/csrc/batch_order.hpp driven by fake stages, meant for -fsanitize=thread
// (tests/test_batch_order.py builds and runs it).  A slot is three integers and a message; every stage sleeps a few
// deterministic pseudo-random microseconds, so that the interleavings differ from batch to batch and from seed to seed.
// One line per case on stdout; the first violated expectation ends the program with status 1.
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <new>
#include <stdexcept>
#include <thread>

#include "../../npore_amd/csrc/batch_order.hpp"

namespace {
constexpr int N_SLOTS = 6, RC_THROWN = -77;
enum Stage { ACQUIRE, PACK, ENQUEUE, COLLECT, WRITE, NONE };
const char *const STAGE_NAME[] = {"acquire", "pack", "enqueue", "collect", "write", "none"};
enum How { RETURNS, THROWS_RUNTIME_ERROR, THROWS_BAD_ALLOC };

struct Slot { int rc = 0; int64_t m = 0; int in_use = 0; std::string err; };

struct Case {
    int64_t n; bool serial; Stage fail_stage; int64_t fail_at; How how; unsigned seed;
};

[[noreturn]] void violated(const Case &c, const std::string &what)
{
    std::printf("VIOLATED  n=%lld serial=%d fail=%s@%lld how=%d seed=%u: %s\n", (long long)c.n, (int)c.serial, STAGE_NAME[c.fail_stage],
                (long long)c.fail_at, (int)c.how, c.seed, what.c_str());
    std::fflush(stdout);
    std::_Exit(1);
}

int64_t reads_of(int64_t k) { return 1 + k % 3; }

void run_case(const Case &c)
{
    Slot store[N_SLOTS];
    Slot *slots[N_SLOTS];
    for (int i = 0; i < N_SLOTS; i++) slots[i] = &store[i];
    const auto main_thread = std::this_thread::get_id();
    // what the fake stages saw; everything a stage checks is ordered by the skeleton itself (that is the claim under test),
    // so plain variables would do where the skeleton is right -- atomics keep the CHECKS free of races where it is not
    std::atomic<int64_t> next_acquire{0}, next_enqueue{0}, next_write{0}, written_ok{0}, marks{0};
    std::atomic<int> in_acquire{0};
    std::vector<std::atomic<int>> collected((size_t)c.n + 2), write_calls((size_t)c.n + 2);
    for (auto &a : collected) a = 0;
    for (auto &a : write_calls) a = 0;
    auto nap = [&](int64_t k, int stage) {
        unsigned x = c.seed * 2654435761u + (unsigned)k * 40503u + (unsigned)stage * 9176u;
        x ^= x >> 13; x *= 0x5bd1e995u; x ^= x >> 15;
        std::this_thread::sleep_for(std::chrono::microseconds(x % 120));
    };
    // the injected failure: a code and a message of its own, returned or thrown
    auto inject = [&](int64_t k, Stage st, Slot &s) -> int {
        if (st != c.fail_stage || k != c.fail_at) return 0;
        if (c.how == THROWS_RUNTIME_ERROR) throw std::runtime_error("boom");
        if (c.how == THROWS_BAD_ALLOC) throw std::bad_alloc();
        s.err = std::string(STAGE_NAME[st]) + " of batch " + std::to_string(k) + " failed";
        return -(10 + (int)st);
    };
    std::string err;
    const int rc = run_batches_in_order(
        slots, N_SLOTS, c.serial, RC_THROWN,
        [&](int64_t k, Slot &s) -> int64_t {
            if (s.in_use) violated(c, "slot of batch " + std::to_string(k) + " acquired while its previous batch is unwritten");
            if (c.serial) {
                if (in_acquire.exchange(1)) violated(c, "two serial acquires at a time");
                if (next_acquire.fetch_add(1) != k) violated(c, "serial acquire of batch " + std::to_string(k) + " out of order");
            }
            nap(k, ACQUIRE);
            if (c.serial) in_acquire = 0;
            if (const int bad = inject(k, ACQUIRE, s)) return bad;
            if (k >= c.n) return 0;
            s.in_use = 1;
            return reads_of(k);
        },
        [&](int64_t k, Slot &s) {
            if (!s.in_use || s.m != reads_of(k)) violated(c, "pack of batch " + std::to_string(k) + " without its acquire");
            nap(k, PACK);
            return inject(k, PACK, s);
        },
        [&](int64_t k, Slot &s) {
            if (std::this_thread::get_id() != main_thread) violated(c, "enqueue off the calling thread");
            if (next_enqueue.fetch_add(1) != k || s.m != reads_of(k)) violated(c, "enqueue of batch " + std::to_string(k) + " out of order");
            nap(k, ENQUEUE);
            return inject(k, ENQUEUE, s);
        },
        [&](int64_t k, Slot &s) {
            nap(k, COLLECT);
            collected[(size_t)k] = 1;
            return inject(k, COLLECT, s);
        },
        [&](int64_t k, Slot &s) {
            if (write_calls[(size_t)k].fetch_add(1)) violated(c, "batch " + std::to_string(k) + " written twice");
            if (next_write.fetch_add(1) != k) violated(c, "write of batch " + std::to_string(k) + " out of order");
            if (!collected[(size_t)k]) violated(c, "write of batch " + std::to_string(k) + " before its collect");
            if (c.fail_stage != NONE && k > c.fail_at) violated(c, "batch " + std::to_string(k) + " written behind the failed one");
            nap(k, WRITE);
            if (const int bad = inject(k, WRITE, s)) return bad;
            s.in_use = 0;
            written_ok++;
            return 0;
        },
        [&](const char *, int64_t) { marks++; }, err);
    // the call has returned: every task has ended (a deadlock is the test's time limit)
    if (c.fail_stage == NONE) {
        if (rc != 0 || !err.empty()) violated(c, "a clean run returned " + std::to_string(rc) + " '" + err + "'");
        if (written_ok != c.n) violated(c, std::to_string(written_ok) + " batches written");
        if (next_enqueue != c.n) violated(c, std::to_string(next_enqueue) + " batches enqueued");
    } else {
        const std::string prefix = c.fail_stage == COLLECT || c.fail_stage == WRITE ? "SAM text of a batch: " : "batch preparation: ";
        const int want_rc = c.how == RETURNS ? -(10 + (int)c.fail_stage) : RC_THROWN;
        const std::string want_err = c.how == RETURNS                ? std::string(STAGE_NAME[c.fail_stage]) + " of batch " + std::to_string(c.fail_at) + " failed"
                                     : c.how == THROWS_RUNTIME_ERROR ? prefix + "boom"
                                                                     : prefix + std::bad_alloc().what();
        if (rc != want_rc || err != want_err) violated(c, "returned " + std::to_string(rc) + " '" + err + "', not " + std::to_string(want_rc) + " '" + want_err + "'");
        // the batches ahead of the failed one have left, in order (the write stage checked the order); none behind it
        if (written_ok != c.fail_at) violated(c, std::to_string(written_ok) + " batches written");
    }
    std::printf("ok  n=%2lld serial=%d fail=%-7s@%2lld how=%d seed=%u  rc=%d written=%lld marks=%lld\n", (long long)c.n, (int)c.serial,
                STAGE_NAME[c.fail_stage], (long long)c.fail_at, (int)c.how, c.seed, rc, (long long)written_ok.load(), (long long)marks.load());
}
}  // namespace

int main()
{
    int64_t batches = 0;
    for (unsigned seed = 1; seed <= 3; seed++)
        for (int serial = 0; serial < 2; serial++) {
            for (int64_t n : {0, 1, 2, 5, 6, 7, 19}) { run_case(Case{n, serial != 0, NONE, -1, RETURNS, seed}); batches += n; }
            // one injected failure per run: every stage, at batches 0, 1, 2, 6 and 8 of 19.  collect and write at batch 2 are
            // the cases with more than N_SLOTS batches behind the failure: the slot of batch 2 is packed again (batch 8) and
            // again (batch 14) before the run ends, and the failure must still be what the call returns
            for (int st = ACQUIRE; st <= WRITE; st++)
                for (int64_t at : {0, 1, 2, 6, 8}) { run_case(Case{19, serial != 0, (Stage)st, at, RETURNS, seed}); batches += 19; }
            for (int st = ACQUIRE; st <= WRITE; st++) {
                run_case(Case{19, serial != 0, (Stage)st, 2, THROWS_RUNTIME_ERROR, seed});
                run_case(Case{19, serial != 0, (Stage)st, 8, THROWS_BAD_ALLOC, seed});
                batches += 38;
            }
        }
    std::printf("%lld fake batches, all expectations held\n", (long long)batches);
    return 0;
}
