// bk_hostpool.cpp -- the worker pool of bk_hostpool.h.
#include "bk_hostpool.h"

#include <cstdlib>

namespace bk {

HostPool &HostPool::get()
{
    static HostPool pool;
    return pool;
}

void HostPool::run(size_t want, const std::function<void(size_t)> &job)
{
    if (!want) return;
    std::unique_lock<std::mutex> submit(submit_mutex_);  // one parallel section at a time
    // The caller is the last worker: the section starts now, not when the first sleeper has woken up (waking forty sleepers through
    // one mutex takes longer than a short section's whole work - the jobs here all draw their work from a shared counter, so whoever
    // arrives late simply takes less).
    const size_t pooled = want - 1;
    if (pooled) {
        {
            std::lock_guard<std::mutex> lock(m_);
            job_ = &job;
            want_ = pooled;
            next_ = 0;
            done_ = 0;
        }
        if (pooled >= threads_.size() / 2) wake_.notify_all();
        else for (size_t i = 0; i < pooled; ++i) wake_.notify_one();
    }
    // (the caller's job returns when the shared counter is used up: workers that have not even woken yet are not waited for -
    //  their turns are withdrawn - only those that are in the middle of their last piece; the same when the caller's job throws
    //  - Interp::clone's std::bad_alloc - so that no worker is left running a job that no longer exists)
    const auto withdraw = [&] {
        if (!pooled) return;
        std::unique_lock<std::mutex> lock(m_);
        want_ = next_;
        finished_.wait(lock, [&] { return done_ == want_; });
        job_ = nullptr;
        want_ = next_ = done_ = 0;
    };
    try {
        job(pooled);
    } catch (...) {
        withdraw();
        throw;
    }
    withdraw();
}

HostPool::~HostPool()
{
    {
        std::lock_guard<std::mutex> lock(m_);
        stop_ = true;
    }
    wake_.notify_all();
    for (std::thread &t : threads_) if (t.joinable()) t.join();
}

HostPool::HostPool()
{
    unsigned hw = std::thread::hardware_concurrency();
    size_t workers = std::min<size_t>(hw ? hw : 1, 128);
    if (const char *e = getenv("BLINKY_HIP_FIXUP_THREADS")) workers = (size_t)std::max(1, std::min(256, atoi(e)));
    for (size_t i = 0; i < workers; ++i) threads_.emplace_back([this] { loop(); });
}

void HostPool::loop()
{
    for (;;) {
        const std::function<void(size_t)> *job = nullptr;
        size_t mine = 0;
        {
            std::unique_lock<std::mutex> lock(m_);
            wake_.wait(lock, [&] { return stop_ || next_ < want_; });
            if (stop_) return;
            job = job_;
            mine = next_++;
        }
        (*job)(mine);
        {
            std::lock_guard<std::mutex> lock(m_);
            if (++done_ == want_) finished_.notify_all();
        }
    }
}

void host_parallel(size_t parts, const std::function<void(size_t)> &job)
{
    if (parts <= 1) { if (parts) job(0); return; }
    pool_runs(parts, 1, std::min(parts, HostPool::get().size()), [&](size_t, Runs &runs) {
        for (size_t first, count; runs.next(&first, &count);)
            for (size_t i = first; i < first + count; ++i) job(i);
    });
}

}  // namespace bk
