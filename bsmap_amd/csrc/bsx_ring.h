// bsx_ring.h — the ordered hand-offs of the command line's pipeline (bsmap_main.cpp), free of bsx.h so that they can be run alone
// (tests/harness/ring_check.cpp, under AddressSanitizer and ThreadSanitizer):
//   Ring       batches pass through the stages in input order over a fixed set of slots
//   Gate       at most NC holders at a time, granted in batch order
//   LeakChain  the value behind batch k-1 is handed to batch k
#pragma once
#include <condition_variable>
#include <mutex>
#include <utility>
#include <vector>

namespace bsx_ring {

// what the ring keeps per slot; the payload type derives from it
struct SlotState {
    int stage = 0;    // 0 free, then whatever stages the user counts (the command line: 1 parsed, 2 aligned, 3 formatted)
    long batch = -1;  // ordinal of the batch the slot holds while stage != 0
};

template <class S>   // S: a SlotState with the batch's data
struct Ring {
    const int NS;
    std::vector<S> slot;
    explicit Ring(int ns) : NS(ns), slot(ns) {}
    std::mutex mu;
    std::condition_variable cv;
    long n_batches = -1;  // known once the producer reaches the end of the input
    S &at(long k) { return slot[k % NS]; }
    // wait until batch k is in `stage`; false when the input ended before batch k.  A slot is shared by the batches
    // k, k+NS, ...: a consumer must not mistake an older batch that is still in the same stage for its own, so the slot
    // carries the ordinal of the batch it holds (stage 0 = free: the parser takes it for whatever batch comes next).
    bool acquire(long k, int stage)
    {
        std::unique_lock<std::mutex> lk(mu);
        cv.wait(lk, [&] { return (n_batches >= 0 && k >= n_batches) || (at(k).stage == stage && (stage == 0 || at(k).batch == k)); });
        return !(n_batches >= 0 && k >= n_batches);
    }
    void release(long k, int stage) { { std::lock_guard<std::mutex> lk(mu); at(k).stage = stage; at(k).batch = stage ? k : -1; } cv.notify_all(); }
    void finish(long n) { { std::lock_guard<std::mutex> lk(mu); n_batches = n; } cv.notify_all(); }
};

// Compute slots of one GPU: at most `nc` of its `nb` device batches hold the gate at a time, and it is granted in batch order — this gate sees the batches
// first, first + stride, ... — so a later batch never overtakes an earlier one (results are consumed in input order).  With nc == nb every batch may always
// run: `gated` is false, and enter() and leave() return on that test alone, without touching the mutex.
struct Gate {
    std::mutex mu;
    std::condition_variable cv;
    bool gated = false;
    int free_slots = 0;
    long next = 0, stride = 1;
    void init(int nc, int nb, long first, long stride_) { gated = nc < nb; free_slots = nc; next = first; stride = stride_; }
    void enter(long k)
    {
        if (!gated) return;
        std::unique_lock<std::mutex> lk(mu);
        cv.wait(lk, [&] { return free_slots > 0 && next == k; });
        free_slots--; next = k + stride;
        lk.unlock();
        cv.notify_all();
    }
    void leave()
    {
        if (!gated) return;
        { std::lock_guard<std::mutex> lk(mu); free_slots++; }
        cv.notify_all();
    }
};

// A value handed from batch to batch in input order, whichever thread runs which batch: take(k) waits for the value behind batch k-1 (the initial `value`
// for batch 0), put(k, v) leaves the one behind batch k.
template <class V>
struct LeakChain {
    std::mutex mu;
    std::condition_variable cv;
    long have = -1;  // `value` is the one behind batch `have`
    V value;
    V take(long k)
    {
        std::unique_lock<std::mutex> lk(mu);
        cv.wait(lk, [&] { return have == k - 1; });
        return value;
    }
    void put(long k, V v) { { std::lock_guard<std::mutex> lk(mu); value = std::move(v); have = k; } cv.notify_all(); }
};

}  // namespace bsx_ring
