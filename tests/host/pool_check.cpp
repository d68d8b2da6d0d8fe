// pool_check.cpp -- stand-alone check of the host worker pool (blinky_amd/csrc/bk_hostpool.cpp): links that unit alone, no HIP, no
// Python.  Prints what failed and exits non-zero.  Run it a second time with BLINKY_HIP_FIXUP_THREADS=1 (the variable is read when the
// pool is first used); `make sanitize` builds it with ThreadSanitizer.
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <stdexcept>
#include <thread>
#include <vector>

#include "../../blinky_amd/csrc/bk_hostpool.h"

static int g_failed = 0;
#define CHECK(cond, ...)                                      \
    do {                                                      \
        if (!(cond)) {                                        \
            ++g_failed;                                       \
            fprintf(stderr, "pool_check: FAILED %s: ", #cond); \
            fprintf(stderr, __VA_ARGS__);                     \
            fprintf(stderr, "\n");                            \
        }                                                     \
    } while (0)

static const size_t kSizes[] = {0, 1, 2, 255, 256, 10007};

// every index of [0, n) exactly once, whoever visits it
static void visits_host_parallel(size_t parts)
{
    std::vector<std::atomic<int>> seen(parts);
    for (auto &s : seen) s.store(0);
    bk::host_parallel(parts, [&](size_t i) {
        if (i < parts) seen[i].fetch_add(1, std::memory_order_relaxed);
        else CHECK(false, "host_parallel(%zu) handed out index %zu", parts, i);
    });
    for (size_t i = 0; i < parts; ++i)
        if (seen[i].load() != 1) { CHECK(false, "host_parallel(%zu): index %zu visited %d times", parts, i, seen[i].load()); break; }
}

static void visits_pool_runs(size_t n, size_t run, size_t nthreads)
{
    std::vector<std::atomic<int>> seen(n);
    for (auto &s : seen) s.store(0);
    std::atomic<int> bad{0};
    bk::pool_runs(n, run, nthreads, [&](size_t worker, bk::Runs &runs) {
        for (size_t first, count; runs.next(&first, &count);) {
            if (!count || first + count > n || worker >= (nthreads ? nthreads : 1) || (nthreads > 1 && count > run)) { bad.fetch_add(1); continue; }
            for (size_t i = first; i < first + count; ++i) seen[i].fetch_add(1, std::memory_order_relaxed);
        }
    });
    CHECK(bad.load() == 0, "pool_runs(%zu, %zu, %zu): %d runs out of range", n, run, nthreads, bad.load());
    for (size_t i = 0; i < n; ++i)
        if (seen[i].load() != 1) { CHECK(false, "pool_runs(%zu, %zu, %zu): index %zu visited %d times", n, run, nthreads, i, seen[i].load()); break; }
}

static void check_visits(size_t pool)
{
    for (size_t n : kSizes) visits_host_parallel(n);
    for (size_t parts : {pool > 1 ? pool - 1 : (size_t)1, pool, pool + 1, 3 * pool + 1}) visits_host_parallel(parts);
    for (size_t n : kSizes)
        for (size_t run : {(size_t)1, (size_t)7, (size_t)128})
            for (size_t nthreads : {(size_t)1, pool > 1 ? pool - 1 : (size_t)1, pool, pool + 1}) visits_pool_runs(n, run, nthreads);
}

// the job throws on the caller's turn (the caller is the last worker: index want - 1)
static void check_throwing_section(size_t want)
{
    std::atomic<int> in_flight{0}, started{0};
    std::atomic<size_t> next{0};
    struct Inside {
        std::atomic<int> &n;
        explicit Inside(std::atomic<int> &c) : n(c) { n.fetch_add(1); }
        ~Inside() { n.fetch_sub(1); }
    };
    bool caught = false;
    try {
        bk::HostPool::get().run(want, [&](size_t worker) {
            Inside inside(in_flight);
            started.fetch_add(1);
            if (worker == want - 1) {
                for (int spin = 0; spin < 1000 && started.load() < 2; ++spin) std::this_thread::yield();      // (let a pooled worker get into the job, if one comes)
                throw std::runtime_error("caller's turn");
            }
            while (next.fetch_add(1, std::memory_order_relaxed) < 200000) {}                                    // a worker in the middle of its piece
        });
    } catch (const std::runtime_error &) {
        caught = true;
    }
    CHECK(caught, "run(%zu): the exception did not reach the caller", want);
    CHECK(in_flight.load() == 0, "run(%zu): %d workers still inside the job after run() returned", want, in_flight.load());
}

// four threads submit sections at the same time: each its own sum
static void check_concurrent_submitters(size_t pool)
{
    const size_t n = 10007;
    unsigned long long sums[4] = {0, 0, 0, 0};
    std::vector<std::thread> submitters;
    for (int k = 0; k < 4; ++k)
        submitters.emplace_back([&, k] {
            for (int round = 0; round < 20; ++round) {
                std::atomic<unsigned long long> sum{0};
                bk::pool_runs(n, 64, pool + 1, [&](size_t, bk::Runs &runs) {
                    unsigned long long s = 0;
                    for (size_t first, count; runs.next(&first, &count);)
                        for (size_t i = first; i < first + count; ++i) s += (unsigned long long)i * (unsigned)(k + 1);
                    sum.fetch_add(s, std::memory_order_relaxed);
                });
                if (round == 0 || sum.load() != sums[k]) sums[k] = round == 0 ? sum.load() : ~0ull;
            }
        });
    for (std::thread &t : submitters) t.join();
    for (int k = 0; k < 4; ++k) {
        const unsigned long long want = (unsigned long long)n * (n - 1) / 2 * (unsigned)(k + 1);
        CHECK(sums[k] == want, "submitter %d: sum %llu, expected %llu", k, sums[k], want);
    }
}

int main()
{
    const size_t pool = bk::HostPool::get().size();
    size_t want_pool = std::min<size_t>(std::max(1u, std::thread::hardware_concurrency()), 128);
    if (const char *e = getenv("BLINKY_HIP_FIXUP_THREADS")) want_pool = (size_t)std::max(1, std::min(256, atoi(e)));
    CHECK(pool == want_pool, "the pool has %zu threads, expected %zu", pool, want_pool);

    check_visits(pool);
    for (size_t want : {(size_t)1, (size_t)2, pool, pool + 1}) {
        check_throwing_section(want);
        visits_pool_runs(10007, 7, pool + 1);          // the next section on the same pool
        visits_host_parallel(257);
    }
    check_concurrent_submitters(pool);

    if (g_failed) { fprintf(stderr, "pool_check: %d checks failed (pool of %zu)\n", g_failed, pool); return 1; }
    printf("pool_check ok: pool of %zu threads\n", pool);
    return 0;
}
