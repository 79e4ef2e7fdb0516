// nearest.hip -- for every query interval of the loaded record, the target it lies in or overlaps and its neighbours to either
// side (api_nearest.cpp: ribbit_hip_record_nearest; include/ribbit_hip.h has the contract).  On the handle's stream:
//   keys:     one lane per target, clipped in 64-bit: a[j] = s' << 32 | e' and b[j] = e' << 32 | s'; an empty target gets the
//             all-ones key in both (s', e' < 2^31: no real key is all ones), so the sorts put it behind every real one and no
//             search below ever stops on it
//   sort:     a and b with the value j, each by a rocPRIM radix sort of pairs over all 64 bits (the values come from a counting
//             iterator); the sorts are stable, so j breaks ties: order A = (s', e', j), order B = (e', s', j)
//   scan in:  one lane per position k of order A: e'_k << 32 | ~k (0 for an empty target's position)
//   scan:     rocPRIM inclusive scan with max: its high half is M[k], the greatest e' among the first k + 1 targets of order A,
//             its low half ~(the position that holds it, the lowest among equals)
//   queries:  one lane per query, clipped in 64-bit, four bisections:
//               pa = #{ s'_k <= s } and pe = #{ s'_k < e } in the A keys, pb = #{ e'_k <= s } in the B keys,
//               po = the first k < pe with M[k] > s in the scanned keys (M does not descend)
//             inside iff pa > 0 and M[pa - 1] >= e: the hit is the position the scan names there; otherwise over iff po < pe
//             (M[po] > s >= M[po - 1] makes e'_po = M[po], and po < pe makes s'_po < e); left is position pb - 1 of order B,
//             right position pe of order A unless that is an empty target's.  Nothing walks the overlapping targets.
// The key kernel and the query kernel take one item per lane and stride beyond ROW_MAX_BLOCKS blocks.
#include <cstring>

#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>

#include "row_kernels.h"

namespace rb {

namespace {

constexpr uint64_t NEAR_EMPTY = ~(uint64_t)0;

__global__ void __launch_bounds__(ROW_THREADS) nearest_keys_kernel(const int32_t *__restrict__ targets, int64_t m, int64_t length, uint64_t *__restrict__ a,
                                                                    uint64_t *__restrict__ b) {
    for (int64_t j = (int64_t)blockIdx.x * ROW_THREADS + threadIdx.x; j < m; j += (int64_t)gridDim.x * ROW_THREADS) {
        const auto [s, e] = clip_row(targets, j, length);
        const bool has = s < e;
        a[j] = has ? (uint64_t)s << 32 | (uint64_t)e : NEAR_EMPTY;
        b[j] = has ? (uint64_t)e << 32 | (uint64_t)s : NEAR_EMPTY;
    }
}

__global__ void __launch_bounds__(ROW_THREADS) nearest_scan_input_kernel(const uint64_t *__restrict__ a_sorted, int64_t m, uint64_t *__restrict__ reach) {
    for (int64_t k = (int64_t)blockIdx.x * ROW_THREADS + threadIdx.x; k < m; k += (int64_t)gridDim.x * ROW_THREADS) {
        const uint64_t key = a_sorted[k];
        reach[k] = key == NEAR_EMPTY ? 0 : key << 32 | (uint32_t)~(uint32_t)k;
    }
}

// the number of leading keys of keys[0 .. m) whose high half is below `limit` (the high halves do not descend)
__device__ inline int64_t high_below(const uint64_t *__restrict__ keys, int64_t m, uint64_t limit) {
    int64_t lo = 0, hi = m;
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo) / 2;
        if ((keys[mid] >> 32) < limit) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__global__ void __launch_bounds__(ROW_THREADS) nearest_queries_kernel(const int32_t *__restrict__ queries, int64_t n, int64_t length,
                                                                       const uint64_t *__restrict__ a_sorted, const uint64_t *__restrict__ b_sorted,
                                                                       const uint64_t *__restrict__ reach, const int32_t *__restrict__ order_a,
                                                                       const int32_t *__restrict__ order_b, int64_t m, RibbitNearest *__restrict__ out) {
    for (int64_t i = (int64_t)blockIdx.x * ROW_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * ROW_THREADS) {
        const auto [s, e] = clip_row(queries, i, length);
        RibbitNearest r{RIBBIT_NEAREST_APART, -1, -1, -1, -1, -1};
        if (s < e) {
            // (s + 1 <= length < 2^31: an empty target's high half, 2^32 - 1, is never below a limit)
            const int64_t pa = high_below(a_sorted, m, (uint64_t)s + 1), pe = pa + high_below(a_sorted + pa, m - pa, (uint64_t)e);
            const int64_t pb = high_below(b_sorted, m, (uint64_t)s + 1);
            bool inside = false;
            if (pa > 0) {
                const uint64_t top = reach[pa - 1];
                if ((int64_t)(top >> 32) >= e) {
                    inside = true;
                    r.kind = RIBBIT_NEAREST_INSIDE;
                    r.hit = order_a[(uint32_t)~(uint32_t)top];
                }
            }
            if (!inside) {
                const int64_t po = high_below(reach, pe, (uint64_t)s + 1);
                if (po < pe) {
                    r.kind = RIBBIT_NEAREST_OVER;
                    r.hit = order_a[po];
                }
            }
            if (pb > 0) {
                r.left = order_b[pb - 1];
                r.left_dist = (int32_t)(s - (int64_t)(b_sorted[pb - 1] >> 32));
            }
            if (pe < m) {
                const uint64_t key = a_sorted[pe];
                if (key != NEAR_EMPTY) {
                    r.right = order_a[pe];
                    r.right_dist = (int32_t)((int64_t)(key >> 32) - e);
                }
            }
        }
        out[i] = r;
    }
}

hipError_t sort_by_key(void *scratch, size_t &bytes, const uint64_t *in, uint64_t *out, int32_t *order, int64_t m, hipStream_t stream) {
    return rocprim::radix_sort_pairs(scratch, bytes, in, out, rocprim::counting_iterator<int32_t>(0), order, (size_t)m, 0u, 64u, stream);
}

hipError_t scan_reach(void *scratch, size_t &bytes, const uint64_t *in, uint64_t *out, int64_t m, hipStream_t stream) {
    return rocprim::inclusive_scan(scratch, bytes, in, out, (size_t)m, rocprim::maximum<uint64_t>(), stream);
}

}  // namespace

NearestLayout nearest_layout(int64_t n, int64_t n_targets) {
    size_t a = 0, b = 0;
    if (n_targets > 0) {
        (void)sort_by_key(nullptr, a, nullptr, nullptr, nullptr, n_targets, 0);
        (void)scan_reach(nullptr, b, nullptr, nullptr, n_targets, 0);
    }
    NearestLayout at{};
    WorkCarver w;
    at.keys = w.take(4 * (size_t)n_targets * sizeof(uint64_t));
    at.order = w.take(2 * (size_t)n_targets * sizeof(int32_t));
    at.out = w.take((size_t)n * sizeof(RibbitNearest));
    w.close(at, std::max(a, b));
    return at;
}

hipError_t launch_nearest(const int32_t *queries, int64_t n, const int32_t *targets, int64_t n_targets, int64_t length, uint8_t *work, size_t work_bytes,
                          const NearestLayout &at, hipStream_t stream) {
    if (work_bytes < at.bytes) return hipErrorInvalidValue;
    const int64_t m = n_targets;
    uint64_t *a = region<uint64_t>(work, at.keys), *b = a + m, *a_sorted = a + 2 * m, *b_sorted = a + 3 * m;
    uint64_t *reach_in = a, *reach = b;      // (the unsorted keys are done with once both sorts have run)
    int32_t *order_a = region<int32_t>(work, at.order), *order_b = order_a + m;
    RibbitNearest *out = region<RibbitNearest>(work, at.out);
    void *scratch = work + at.scratch;
    const size_t scratch_bytes = at.scratch_bytes;
    hipError_t e;
    if (m > 0) {
        const dim3 grid(grid_for(m, ROW_THREADS, ROW_MAX_BLOCKS));
        hipLaunchKernelGGL(nearest_keys_kernel, grid, dim3(ROW_THREADS), 0, stream, targets, m, length, a, b);
        size_t bytes = scratch_bytes;
        if ((e = sort_by_key(scratch, bytes, a, a_sorted, order_a, m, stream)) != hipSuccess) return e;
        bytes = scratch_bytes;
        if ((e = sort_by_key(scratch, bytes, b, b_sorted, order_b, m, stream)) != hipSuccess) return e;
        hipLaunchKernelGGL(nearest_scan_input_kernel, grid, dim3(ROW_THREADS), 0, stream, a_sorted, m, reach_in);
        bytes = scratch_bytes;
        if ((e = scan_reach(scratch, bytes, reach_in, reach, m, stream)) != hipSuccess) return e;
    }
    if (n > 0)
        hipLaunchKernelGGL(nearest_queries_kernel, dim3(grid_for(n, ROW_THREADS, ROW_MAX_BLOCKS)), dim3(ROW_THREADS), 0, stream, queries, n, length, a_sorted,
                           b_sorted, reach, order_a, order_b, m, out);
    return hipGetLastError();
}

}  // namespace rb
