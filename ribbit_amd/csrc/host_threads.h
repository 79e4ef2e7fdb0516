// host_threads.h -- every team of host threads the library starts goes through here (no HIP: refine.cpp, parallel_merge.cpp and
// host_planes.cpp include it too).  A team is nt parts of one piece of work, part 0 on the calling thread; a thread that cannot
// start leaves its part to the caller, every started thread is joined on every way out, and an exception in any part comes
// out on the caller after the join -- so a failed allocation inside a team reaches guarded() (api_internal.h) like any other
// instead of ending the process in std::terminate.  The threads that live longer than one parallel loop (feeders, tabler,
// presize, ...) stay where they are made and keep an exception inside themselves; JoinOnExit is their guard.
#pragma once
#include <algorithm>
#include <atomic>
#include <cerrno>
#include <cstdint>
#include <cstdlib>
#include <exception>
#include <functional>
#include <mutex>
#include <new>
#include <system_error>
#include <thread>
#include <vector>

namespace rb {

// How many host threads a stage may use: `asked` (the handle's ribbit_hip_set_host_threads) if non-zero, else RIBBIT_THREADS,
// else one GPU's share of the host.  Every caller clamps further by its own grain.
inline unsigned host_thread_count(unsigned asked) {
    if (asked) return asked;
    if (const char *env = std::getenv("RIBBIT_THREADS")) return (unsigned)std::max(1, std::atoi(env));
    return std::max(1u, std::min(std::thread::hardware_concurrency(), 16u));
}

// RIBBIT_PROFILE=1: the stages' wall-clock lines on stderr
inline bool profile_on() {
    static const bool on = std::getenv("RIBBIT_PROFILE") != nullptr;
    return on;
}

// Test hook (ribbit_host_debug_thread_faults): in every team of two parts or more, thread start number `refuse_from` and the
// later ones fail as the system's would, and part `throw_in` throws std::bad_alloc before its body; -1: off.
struct ThreadFaults {
    std::atomic<int32_t> refuse_from{-1}, throw_in{-1};
    std::atomic<int64_t> injected{0};
};
inline ThreadFaults g_thread_faults;
inline int64_t set_thread_faults(int32_t refuse_from, int32_t throw_in) {
    g_thread_faults.refuse_from = refuse_from;
    g_thread_faults.throw_in = throw_in;
    return g_thread_faults.injected.exchange(0);
}

// fn(t) for every t in [0, nt): part 0 here, the others on threads of their own (or here, one after the other, from the first
// thread that cannot start).  The first exception of any part is rethrown here when all parts are over.
template <class F>
void on_threads(unsigned nt, F &&fn) {
    if (nt <= 1) { fn(0u); return; }
    std::exception_ptr first;
    std::mutex first_lock;
    auto part = [&](unsigned t) {
        try {
            if ((int32_t)t == g_thread_faults.throw_in.load(std::memory_order_relaxed)) { ++g_thread_faults.injected; throw std::bad_alloc(); }
            fn(t);
        } catch (...) {
            std::lock_guard<std::mutex> lk(first_lock);
            if (!first) first = std::current_exception();
        }
    };
    std::vector<std::thread> pool;
    unsigned started = 1;
    try {
        pool.reserve(nt - 1);
        for (; started < nt; ++started) {
            const int32_t refuse_from = g_thread_faults.refuse_from.load(std::memory_order_relaxed);
            if (refuse_from >= 0 && (int32_t)(started - 1) >= refuse_from) { ++g_thread_faults.injected; throw std::system_error(EAGAIN, std::generic_category()); }
            pool.emplace_back(part, started);
        }
    } catch (...) {}      // (no thread, or no memory for one: parts `started` .. nt - 1 are the caller's)
    part(0);
    for (unsigned t = started; t < nt; ++t) part(t);
    for (std::thread &th : pool) th.join();
    if (first) std::rethrow_exception(first);
}

// fn(lo, hi, t) over [0, n) cut into nt contiguous pieces: piece t = [n t / nt, n (t + 1) / nt)
template <class F>
void over_pieces(size_t n, unsigned nt, F &&fn) {
    nt = std::max(nt, 1u);
    on_threads(nt, [&](unsigned t) { fn(n * t / nt, n * (t + 1) / nt, t); });
}

// Joins the threads it names when the scope ends, however it ends (a joinable std::thread's destructor ends the process);
// `before` (may be empty) runs first: where a thread waits for a signal to stop, that is the place to give it.  Declare it AFTER
// everything its threads touch: locals die in reverse order, so the guard joins before any of that goes.  Allocates nothing.
struct JoinOnExit {
    std::thread *threads[4] = {nullptr, nullptr, nullptr, nullptr};      // joined in this order where joinable
    std::function<void()> before;
    template <class... T>
    explicit JoinOnExit(std::function<void()> b, T &...t) : threads{&t...}, before(std::move(b)) { static_assert(sizeof...(T) <= 4, "room for four threads"); }
    template <size_t N>
    JoinOnExit(std::function<void()> b, std::thread (&all)[N]) : before(std::move(b)) {
        static_assert(N <= 4, "room for four threads");
        for (size_t k = 0; k < N; ++k) threads[k] = &all[k];
    }
    JoinOnExit(const JoinOnExit &) = delete;
    JoinOnExit &operator=(const JoinOnExit &) = delete;
    ~JoinOnExit() {
        if (before) before();
        for (std::thread *t : threads) if (t && t->joinable()) t->join();
    }
};

}  // namespace rb
