// drives bsx_ring.h (the command line's ordered hand-offs) without a GPU, in the thread shape of bsmap_main.cpp over an int payload:
//   ring  <NS> <NG> <n> <cut>  one producer 0->1 (the parse stage's loop: with cut = 1 batch n is a partial one, "release(k, 1); k++; finish(k)"), NG consumers 1->2
//                              strided k = g, g+NG, ..., one consumer 2->3, one 3->0; every stage must see every batch once, in order, with the payload of ITS batch
//   late  <NS> <n>             waiters on batches >= n of the stages 1..3 that stand before finish(n) is called: all return false
//   gate  <NC> <ND>            NB = 3 threads per gate, 30 batches: never more than NC holders, grants in batch order
//   chain                      4 threads, put(k, f_k(take(k))) over 40 batches = f_39(...f_0(1))
// Every thread sleeps 0-200 us between its steps, from a fixed seed.  Exit status 0 and "ok" on success, a message and 1 otherwise.
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <thread>
#include "../../bsmap_amd/csrc/bsx_ring.h"

namespace {

struct IntSlot : bsx_ring::SlotState { long v = -1; };
typedef bsx_ring::Ring<IntSlot> Ring;

std::atomic<int> failed(0);
#define CHECK(c, ...) do { if (!(c)) { if (!failed.exchange(1)) { fprintf(stderr, "ring_check: " __VA_ARGS__); fprintf(stderr, " [%s]\n", #c); } } } while (0)

struct Nap {
    std::mt19937 rng;
    explicit Nap(unsigned id) : rng(20240u + id) {}
    void operator()() { std::this_thread::sleep_for(std::chrono::microseconds(rng() % 201)); }
};

long tag(long k, int stage) { return k * 4 + stage; }  // what the stage that moves batch k to `stage` writes

int run_ring(int NS, int NG, long n, bool cut)
{
    Ring ring(NS);
    const long want = n + (cut ? 1 : 0);
    std::vector<std::vector<long>> seen1(NG);
    std::vector<long> seen0, seen2, seen3;
    std::thread producer([&] {
        Nap nap(0);
        long k = 0;
        for (;; k++) {
            const bool got = ring.acquire(k, 0);  // (the end of the input is not known yet: a free slot is always granted)
            CHECK(got, "producer refused batch %ld", k);
            IntSlot &s = ring.at(k);
            CHECK(s.v == (k < NS ? -1 : tag(k - NS, 0)), "batch %ld: free slot holds %ld", k, s.v);  // the slot's last user is batch k - NS, written out
            nap();
            if (k == n) {  // the input ends here; a partial last batch is handed on before the count is published
                if (cut) { s.v = tag(k, 1); seen0.push_back(k); ring.release(k, 1); k++; }
                break;
            }
            s.v = tag(k, 1); seen0.push_back(k);
            ring.release(k, 1);
        }
        ring.finish(k);
    });
    std::vector<std::thread> gpu;
    for (int g = 0; g < NG; g++)
        gpu.emplace_back([&, g] {
            Nap nap(1 + g);
            for (long k = g; ring.acquire(k, 1); k += NG) {
                IntSlot &s = ring.at(k);
                CHECK(s.batch == k && s.v == tag(k, 1), "stage 1, batch %ld: slot holds batch %ld, payload %ld", k, s.batch, s.v);
                nap();
                s.v = tag(k, 2); seen1[g].push_back(k);
                ring.release(k, 2);
            }
        });
    auto serial = [&](int from, std::vector<long> &seen, unsigned id) {
        Nap nap(id);
        for (long k = 0; ring.acquire(k, from); k++) {
            IntSlot &s = ring.at(k);
            CHECK(s.batch == k && s.v == tag(k, from), "stage %d, batch %ld: slot holds batch %ld, payload %ld", from, k, s.batch, s.v);
            nap();
            s.v = tag(k, (from + 1) % 4); seen.push_back(k);
            ring.release(k, (from + 1) % 4);
        }
    };
    std::thread format(serial, 2, std::ref(seen2), 100u);
    serial(3, seen3, 101u);  // the write stage runs on the main thread
    producer.join();
    for (std::thread &t : gpu) t.join();
    format.join();
    auto in_order = [&](const std::vector<long> &v, const char *what) {
        CHECK((long)v.size() == want, "%s saw %zu batches of %ld", what, v.size(), want);
        for (size_t i = 0; i < v.size(); i++) CHECK(v[i] == (long)i, "%s: position %zu is batch %ld", what, i, v[i]);
    };
    in_order(seen0, "stage 0"); in_order(seen2, "stage 2"); in_order(seen3, "stage 3");
    long total1 = 0;
    for (int g = 0; g < NG; g++) {
        total1 += (long)seen1[g].size();
        for (size_t i = 0; i < seen1[g].size(); i++) CHECK(seen1[g][i] == g + (long)i * NG, "stage 1, consumer %d: position %zu is batch %ld", g, i, seen1[g][i]);
        CHECK((long)seen1[g].size() == (want > g ? (want - g + NG - 1) / NG : 0), "stage 1, consumer %d saw %zu batches", g, seen1[g].size());
    }
    CHECK(total1 == want, "stage 1 saw %ld batches of %ld", total1, want);
    for (long k = want; k < want + 2 * NS; k += NS - 1)   // behind the end nobody is served, whatever the slot holds
        for (int st = 0; st < 4; st++) CHECK(!ring.acquire(k, st), "batch %ld granted at stage %d after finish(%ld)", k, st, want);
    return failed;
}

int run_late(int NS, long n)
{
    Ring ring(NS);
    for (long k = 0; k < n; k++) { ring.at(k).v = tag(k, 1); ring.release(k, 1 + (int)(k % 3)); }  // (batches in flight when the end becomes known)
    std::atomic<int> standing(0), refused(0);
    std::vector<std::thread> th;
    const long ks[3] = {n, n + 1, n + NS};
    for (long k : ks)
        for (int st = 1; st <= 3; st++)
            th.emplace_back([&, k, st] { standing++; if (!ring.acquire(k, st)) refused++; });
    while (standing < 9) std::this_thread::yield();
    Nap(7)();
    CHECK(refused == 0, "a waiter behind the end returned before finish");
    ring.finish(n);
    for (std::thread &t : th) t.join();
    CHECK(refused == 9, "%d of 9 waiters behind the end were refused", (int)refused);
    return failed;
}

int run_gate(int NC, int ND)
{
    const int NB = 3, NG = ND * NB;
    const long n = 30;
    std::vector<bsx_ring::Gate> gates(ND);
    for (int d = 0; d < ND; d++) gates[d].init(NC, NB, d, ND);
    std::vector<std::atomic<int>> holders(ND);
    for (auto &h : holders) h = 0;
    // The grant itself happens inside enter(); what a holder can see once it is back says this about the order.  Every earlier batch of the gate was granted
    // before batch k, so (1) its thread had asked by then, and (2) it has announced its leave unless it still held the gate when k got in: with k at most NC
    // holders, so at most NC - 1 earlier batches without the announcement (NC = 1: every earlier batch is through, the order is strict).
    std::vector<std::atomic<char>> asked(n), leaving(n);
    for (long k = 0; k < n; k++) { asked[k] = 0; leaving[k] = 0; }
    std::atomic<long> granted(0);
    std::vector<std::thread> th;
    for (int g = 0; g < NG; g++)
        th.emplace_back([&, g] {
            Nap nap(g);
            const int d = g % ND;
            for (long k = g; k < n; k += NG) {
                nap();
                asked[k] = 1;
                gates[d].enter(k);
                const int h = ++holders[d];
                CHECK(h <= NC, "gate %d: %d holders of %d", d, h, NC);
                int inside = 0;
                for (long e = d; e < k; e += ND) { CHECK(asked[e], "gate %d: batch %ld got in before batch %ld had asked", d, k, e); inside += !leaving[e]; }
                CHECK(inside <= NC - 1, "gate %d: batch %ld got in with %d earlier batches not through", d, k, inside);
                granted++;
                nap();
                --holders[d];
                leaving[k] = 1;
                gates[d].leave();
            }
        });
    for (std::thread &t : th) t.join();
    CHECK(granted == n, "%ld of %ld batches got through", (long)granted, n);
    return failed;
}

unsigned long long f(long k, unsigned long long x) { return x * 31ull + (unsigned long long)k; }  // (does not commute: the order of the batches shows)

int run_chain()
{
    const int T = 4;
    const long n = 40;
    bsx_ring::LeakChain<unsigned long long> chain;
    chain.value = 1;
    std::vector<std::thread> th;
    for (int t = 0; t < T; t++)
        th.emplace_back([&, t] { Nap nap(t); for (long k = t; k < n; k += T) { nap(); const unsigned long long v = chain.take(k); nap(); chain.put(k, f(k, v)); } });
    for (std::thread &t : th) t.join();
    unsigned long long want = 1;
    for (long k = 0; k < n; k++) want = f(k, want);
    const unsigned long long got = chain.take(n);
    CHECK(got == want, "chain ends at %llu, sequential %llu", got, want);
    return failed;
}

}  // namespace

int main(int argc, char **argv)
{
    int bad = 2;
    if (argc == 6 && !strcmp(argv[1], "ring")) bad = run_ring(atoi(argv[2]), atoi(argv[3]), atol(argv[4]), atoi(argv[5]) != 0);
    else if (argc == 4 && !strcmp(argv[1], "late")) bad = run_late(atoi(argv[2]), atol(argv[3]));
    else if (argc == 4 && !strcmp(argv[1], "gate")) bad = run_gate(atoi(argv[2]), atoi(argv[3]));
    else if (argc == 2 && !strcmp(argv[1], "chain")) bad = run_chain();
    if (!bad) printf("ok\n");
    return bad;
}
