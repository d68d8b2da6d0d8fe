// bk_hostpool.h -- the library's process-wide pool of host worker threads: the re-derivation of flagged lensmap entries, the host
// build paths and the plate uploads run their parallel sections on it.  No HIP, nothing of the context: the standard library only.
#pragma once

#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <cstddef>
#include <functional>
#include <mutex>
#include <thread>
#include <vector>

namespace bk {

/* job(i) for i in [0, parts) on the pool, the caller waiting; parts <= 1 or a pool of one thread: on the calling thread */
void host_parallel(size_t parts, const std::function<void(size_t)> &job);

#pragma GCC visibility push(hidden)

/* A small process-wide pool of worker threads for the host re-evaluation (creating 64-256 threads per build cost more
 * than the evaluations themselves).  Created on first use; its threads sleep on a condition variable and are JOINED when
 * the library is unloaded or the process exits (a function-local static: destroyed by dlclose / exit handlers, after which
 * no code of this library runs any more). */
class HostPool {
public:
    static HostPool &get();
    size_t size() const { return threads_.size(); }
    /* run job(worker_index) on UP TO `want` workers (<= size() + 1; the caller is one of them) and wait for those that started: every job
     * passed here draws its work from a counter its workers share and returns when that is used up - a worker index that never gets its
     * turn is no loss */
    void run(size_t want, const std::function<void(size_t)> &job);
    ~HostPool();

private:
    HostPool();
    void loop();
    std::mutex m_, submit_mutex_;
    std::condition_variable wake_, finished_;
    const std::function<void(size_t)> *job_ = nullptr;
    size_t want_ = 0, next_ = 0, done_ = 0;
    bool stop_ = false;
    std::vector<std::thread> threads_;
};

/* [0, n) in runs of `run` consecutive indices, which the workers of a section draw from a shared counter until it is used up (the
 * pieces of work cost very different amounts: equal static shares leave most workers waiting for the unluckiest) */
class Runs {
public:
    Runs(size_t n, size_t run) : n_(n), run_(run) {}
    bool next(size_t *first, size_t *count)
    {
        const size_t i0 = next_.fetch_add(run_, std::memory_order_relaxed);
        if (i0 >= n_) return false;
        *first = i0;
        *count = std::min(run_, n_ - i0);
        return true;
    }

private:
    std::atomic<size_t> next_{0};
    const size_t n_, run_;
};

/* body(worker, runs) on `nthreads` pool workers, each taking runs from `runs` while there are any - what a worker needs for its runs
 * (a copy of the interpreter) it makes and destroys itself, on its own thread.  nthreads <= 1: on the calling thread, the whole range
 * as one run, the pool not touched. */
template <typename Body>
void pool_runs(size_t n, size_t run, size_t nthreads, Body body)
{
    Runs runs(n, nthreads <= 1 ? n : run);
    if (nthreads <= 1) { body((size_t)0, runs); return; }
    HostPool::get().run(nthreads, [&](size_t worker) { body(worker, runs); });
}

#pragma GCC visibility pop

}  // namespace bk
