// best.hip -- the best non-overlapping rows of the loaded record (api_best.cpp: ribbit_hip_record_best): the subset of the rows in
// which no two overlap and which covers the most bases, as include/ribbit_hip.h states it (weighted interval scheduling with the
// tie rule of the contract).  No coverage bitmap is read and no count goes to the host in between.  On the handle's stream, every
// launch over all n rows:
//   keys:     one lane per row, clipped in 64-bit: key = e' << 32 | s', an empty row gets the all-ones key (no real key equals it:
//             e' <= L < 2^31), value = the row's index; r, the number of non-empty rows, is a ballot and a popc per wave and turn,
//             summed in a register, one atomic per wave
//   sort:     a rocPRIM radix sort of pairs over the bits a key can have.  It is stable and the values start ascending, so the order
//             is (e', s', index); the empty rows are its tail and are not compacted away
//   sufmin:   an inclusive rocPRIM min-scan of s' over the sorted order read from its end (the empty rows' 0xFFFFFFFF is the
//             minimum's neutral element): rev[j] = the least s' at the positions n - 1 - j .. n - 1
//   prepare:  one lane per sorted position k (0-based): w_k << 32 | p(k) in one word, p(k) by an upper-bound binary search of s'_k
//             in the sorted ends before k, w_k = e'_k - s'_k; the take flag zeroed; and whether k is a segment head: k == 0 or no
//             row from k on starts before the end of row k - 1 (then every row before k ends at or before every later start, so
//             p >= k for all of those: the recurrence and the walk back of the segment need nothing of the rows before it)
//   dp:       one lane per sorted position; only a head works: it walks its segment forward, dp relative to the segment's base
//             (0) into `dp`, and then back from the segment's last position with the contract's strict comparison, setting take
//             flags.  Plain loads and stores, no atomics in the walk; the lane's own stores are the only ones it reads back.  The
//             segments' totals are `bases`: summed over the wave, one 64-bit atomic per wave
//   select:   a rocPRIM flagged select of the sorted row indices by the take flags: the chosen rows by ascending start
#include <cstring>

#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>

#include "row_kernels.h"

namespace rb {

namespace {

constexpr uint64_t EMPTY_KEY = ~(uint64_t)0;
enum : uint8_t { INSIDE = 0, HEAD = 1, EMPTY = 2 };      // a sorted position: inside a segment, its first row, an empty row (the tail)

// One lane per row, rows in grid-stride waves (every lane of a wave takes the same number of turns: the ballot sees whole waves).
__global__ void __launch_bounds__(ROW_THREADS) best_keys_kernel(const int32_t *__restrict__ iv, int64_t n, int64_t length, uint64_t *__restrict__ keys,
                                                                 int32_t *__restrict__ index, uint32_t *__restrict__ count) {
    const int lane = threadIdx.x & 63;
    const int64_t waves = (int64_t)gridDim.x * (ROW_THREADS / 64);
    uint32_t some = 0;
    for (int64_t base = ((int64_t)blockIdx.x * (ROW_THREADS / 64) + (threadIdx.x >> 6)) * 64; base < n; base += waves * 64) {
        const int64_t i = base + lane;
        bool has = false;
        if (i < n) {
            const auto [s, e] = clip_row(iv, i, length);
            has = s < e;
            keys[i] = has ? (uint64_t)e << 32 | (uint64_t)s : EMPTY_KEY;
            index[i] = (int32_t)i;
        }
        some += (uint32_t)__popcll(__ballot(has));
    }
    if (lane == 0 && some) atomicAdd(count, some);
}

// the s' of the sorted keys from the last position backwards
struct StartsFromTheEnd {
    const uint64_t *sorted;
    int64_t n;
    __host__ __device__ uint32_t operator()(int64_t j) const { return (uint32_t)sorted[n - 1 - j]; }
};

__global__ void __launch_bounds__(ROW_THREADS) best_prepare_kernel(const uint64_t *__restrict__ sorted, int64_t n, const uint32_t *__restrict__ rev,
                                                                    uint64_t *__restrict__ pw, uint8_t *__restrict__ head, uint8_t *__restrict__ take) {
    for (int64_t k = (int64_t)blockIdx.x * ROW_THREADS + threadIdx.x; k < n; k += (int64_t)gridDim.x * ROW_THREADS) {
        const uint64_t key = sorted[k];
        take[k] = 0;
        if (key == EMPTY_KEY) { head[k] = EMPTY; continue; }
        const uint32_t s = (uint32_t)key, e = (uint32_t)(key >> 32);
        int64_t lo = 0, hi = k;              // the rows before k that end at or before s (every row that does comes before k)
        while (lo < hi) {
            const int64_t mid = lo + (hi - lo) / 2;
            if ((uint32_t)(sorted[mid] >> 32) <= s) lo = mid + 1; else hi = mid;
        }
        pw[k] = (uint64_t)(e - s) << 32 | (uint64_t)lo;
        head[k] = k == 0 || rev[n - 1 - k] >= (uint32_t)(sorted[k - 1] >> 32) ? HEAD : INSIDE;
    }
}

// Sorted positions in grid-stride waves, as the keys.  With f the head's position, the count c of rows before a row stands for
// dp(c) = 0 when c == f (the segment's base) and dp[c - 1] otherwise, c - 1 being a position of the segment that the lane has
// written.  Back: the row at j is taken exactly when dp(j + 1) > dp(j), which is the contract's w + dp(p) > dp(j).
__global__ void __launch_bounds__(ROW_THREADS) best_dp_kernel(const uint64_t *__restrict__ pw, const uint8_t *__restrict__ head, int64_t n, int32_t *dp,
                                                               uint8_t *__restrict__ take, unsigned long long *__restrict__ bases) {
    const int lane = threadIdx.x & 63;
    const int64_t waves = (int64_t)gridDim.x * (ROW_THREADS / 64);
    unsigned long long sum = 0;
    for (int64_t base = ((int64_t)blockIdx.x * (ROW_THREADS / 64) + (threadIdx.x >> 6)) * 64; base < n; base += waves * 64) {
        const int64_t f = base + lane;
        if (f < n && head[f] == HEAD) {
            int64_t j = f;
            uint64_t cur = pw[j];            // w << 32 | p
            int32_t last = 0;                // dp of the position before j
            for (;;) {
                const bool more = j + 1 < n && head[j + 1] == INSIDE;
                const uint64_t next = more ? pw[j + 1] : cur;      // (asked for before the dependent load below)
                const int64_t p = (int64_t)(uint32_t)cur;
                const int32_t with = (int32_t)(cur >> 32) + (p == f ? 0 : p == j ? last : dp[p - 1]);
                last = max(last, with);
                dp[j] = last;
                if (!more) break;
                ++j;
                cur = next;
            }
            sum += (unsigned long long)last;
            int32_t here = last;             // dp of j
            while (j >= f) {
                const int32_t before = j == f ? 0 : dp[j - 1];
                if (here > before) {
                    take[j] = 1;
                    j = (int64_t)(uint32_t)pw[j] - 1;
                    if (j >= f) here = dp[j];
                } else {
                    --j;
                    here = before;
                }
            }
        }
    }
    sum = wave_sum(sum);
    if (lane == 0 && sum) atomicAdd(bases, sum);
}

// over the bits a key can have: the positions 0 .. length in its high half
hipError_t sort_rows(void *scratch, size_t &bytes, const uint64_t *keys, uint64_t *sorted, const int32_t *index, int32_t *order, int64_t n, int64_t length,
                     hipStream_t stream) {
    return rocprim::radix_sort_pairs(scratch, bytes, keys, sorted, index, order, (size_t)n, 0u, 32 + bits_for(length), stream);
}

hipError_t scan_starts(void *scratch, size_t &bytes, const uint64_t *sorted, uint32_t *rev, int64_t n, hipStream_t stream) {
    return rocprim::inclusive_scan(scratch, bytes, rocprim::make_transform_iterator(rocprim::make_counting_iterator<int64_t>(0), StartsFromTheEnd{sorted, n}),
                                   rev, (size_t)n, rocprim::minimum<uint32_t>(), stream);
}

hipError_t select_taken(void *scratch, size_t &bytes, const int32_t *order, const uint8_t *take, int32_t *selected, unsigned long long *count, int64_t n,
                        hipStream_t stream) {
    return rocprim::select(scratch, bytes, order, take, selected, count, (size_t)n, stream);
}

}  // namespace

BestLayout best_layout(int64_t n, int64_t length) {
    const size_t rows = (size_t)n;
    size_t a = 0, b = 0, c = 0;
    (void)sort_rows(nullptr, a, nullptr, nullptr, nullptr, nullptr, n, length, 0);
    (void)scan_starts(nullptr, b, nullptr, nullptr, n, 0);
    (void)select_taken(nullptr, c, nullptr, nullptr, nullptr, nullptr, n, 0);
    BestLayout at{};
    WorkCarver w;
    at.keys = w.take(2 * rows * sizeof(uint64_t));
    at.work = w.take(3 * rows * sizeof(int32_t));
    at.flags = w.take(2 * rows);
    at.totals = w.take(sizeof(BestTotals));
    at.selected = w.take(rows * sizeof(int32_t));
    w.close(at, std::max(a, std::max(b, c)));
    return at;
}

hipError_t launch_best(const int32_t *rows, int64_t n, int64_t length, uint8_t *work, size_t work_bytes, const BestLayout &at, hipStream_t stream) {
    if (work_bytes < at.bytes) return hipErrorInvalidValue;
    uint64_t *keys = region<uint64_t>(work, at.keys), *sorted = keys + n;
    int32_t *index = region<int32_t>(work, at.work), *order = index + n;
    uint32_t *rev = reinterpret_cast<uint32_t *>(index + 2 * n);
    uint64_t *pw = keys;                            // (the unsorted keys and indices are done with after the sort)
    int32_t *dp = index;
    uint8_t *head = region<uint8_t>(work, at.flags), *take = head + n;
    BestTotals *totals = region<BestTotals>(work, at.totals);
    int32_t *selected = region<int32_t>(work, at.selected);
    void *scratch = work + at.scratch;
    const size_t scratch_bytes = at.scratch_bytes;
    const dim3 grid(grid_for(n, ROW_THREADS, ROW_MAX_BLOCKS)), block(ROW_THREADS);
    hipError_t e = hipMemsetAsync(totals, 0, sizeof(BestTotals), stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(best_keys_kernel, grid, block, 0, stream, rows, n, length, keys, index, &totals->rows);
    size_t bytes = scratch_bytes;
    if ((e = sort_rows(scratch, bytes, keys, sorted, index, order, n, length, stream)) != hipSuccess) return e;
    bytes = scratch_bytes;
    if ((e = scan_starts(scratch, bytes, sorted, rev, n, stream)) != hipSuccess) return e;
    hipLaunchKernelGGL(best_prepare_kernel, grid, block, 0, stream, sorted, n, rev, pw, head, take);
    hipLaunchKernelGGL(best_dp_kernel, grid, block, 0, stream, pw, head, n, dp, take, &totals->bases);
    bytes = scratch_bytes;
    if ((e = select_taken(scratch, bytes, order, take, selected, &totals->selected, n, stream)) != hipSuccess) return e;
    return hipGetLastError();
}

}  // namespace rb
