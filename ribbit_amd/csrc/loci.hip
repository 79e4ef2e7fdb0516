// loci.hip -- merged, sorted loci and a per-window density of the loaded record (api_loci.cpp: ribbit_hip_record_loci,
// ribbit_hip_record_density).  Both read the 1-bit-per-base coverage bitmap that mask.hip's coverage kernel builds from the BED
// rows; nothing is sorted.  On the handle's stream:
//   run ranks:  a lane takes LOCI_LANE_WORDS consecutive bitmap words; the number of run starts and run ends in them (inside the
//               scan's input iterator), packed into one 64-bit word -> exclusive ranks (rocPRIM scan)
//   run bounds: every lane writes its starts and its ends at their ranks: the k-th start pairs with the k-th end, both ascending
//   join:       head flag (the gap before a run is larger than `gap`) and run length, packed -> inclusive scan: locus id and the
//               covered positions so far; one lane per run writes its locus's start (a head) or end (the run before the next head)
//   rows:       one lane per row: clipped in 64-bit, an upper-bound search of s' in the loci's starts, atomicAdd on `rows`,
//               atomicMax on the key (e' - s') << 32 | (0xFFFFFFFF - row): the longest row wins, among equals the lowest index
//   finish:     one lane per locus: `covered` as the difference of the prefix at its end and at the end of the locus before,
//               `best_row` from the key's low half
//   density:    one lane per window (short windows) or one wavefront per window with a cross-lane sum: popcount of the
//               window's words, the two edge words masked
// A bit at a position >= length is never set (the coverage kernel clips), and the words behind the bitmap are zero (padding,
// kernels.h: coverage_words), so a run that reaches the record's end ends there.
#include <cstring>

#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>

#include "kernels.h"

namespace rb {

namespace {

constexpr int LOCI_THREADS = 256;
constexpr int64_t LOCI_MAX_BLOCKS = 256 * 32;      // blocks of a launch at most; the kernels stride
// windows of at least this many bases are summed by a whole wavefront (64 words: one word per lane and pass)
constexpr int64_t DENSITY_WAVE_FROM = 64 * 32;

// the words of lane t with the bits around them: where runs start and end in each word
struct LaneWords {
    uint32_t w[LOCI_LANE_WORDS];
    uint32_t prev_msb, next_lsb;
    __host__ __device__ LaneWords(const uint32_t *bits, int64_t t) {
        const uint4 a = *(const uint4 *)(bits + LOCI_LANE_WORDS * t), b = *(const uint4 *)(bits + LOCI_LANE_WORDS * t + 4);
        w[0] = a.x; w[1] = a.y; w[2] = a.z; w[3] = a.w;
        w[4] = b.x; w[5] = b.y; w[6] = b.z; w[7] = b.w;
        prev_msb = t > 0 ? bits[LOCI_LANE_WORDS * t - 1] >> 31 : 0u;
        next_lsb = bits[LOCI_LANE_WORDS * (t + 1)] & 1u;
    }
    __host__ __device__ bool empty() const { return !(w[0] | w[1] | w[2] | w[3] | w[4] | w[5] | w[6] | w[7]); }
    // bit p: position p of word j is covered and the position before it is not
    __host__ __device__ uint32_t starts(int j) const { return w[j] & ~((w[j] << 1) | (j ? w[j - 1] >> 31 : prev_msb)); }
    // bit p: position p of word j is covered and the position behind it is not (the run ends at p + 1)
    __host__ __device__ uint32_t ends(int j) const { return w[j] & ~((w[j] >> 1) | ((j + 1 < LOCI_LANE_WORDS ? w[j + 1] & 1u : next_lsb) << 31)); }
};
static_assert(LOCI_LANE_WORDS == 8, "a lane loads its words as two dwordx4");

struct RunCounts {
    const uint32_t *bits;
    __host__ __device__ uint64_t operator()(int64_t t) const {
        const LaneWords lw(bits, t);
        if (lw.empty()) return 0;
        uint32_t ns = 0, ne = 0;
#pragma unroll
        for (int j = 0; j < LOCI_LANE_WORDS; ++j) {
            if (!lw.w[j]) continue;
            ns += (uint32_t)__builtin_popcount(lw.starts(j));
            ne += (uint32_t)__builtin_popcount(lw.ends(j));
        }
        return (uint64_t)ns << 32 | ne;      // (a record has fewer than 2^30 runs: the low half never carries)
    }
};

__global__ void __launch_bounds__(LOCI_THREADS) run_bounds_kernel(const uint32_t *__restrict__ bits, int64_t lanes, const uint64_t *__restrict__ off,
                                                                  int32_t *__restrict__ run_start, int32_t *__restrict__ run_end) {
    for (int64_t t = (int64_t)blockIdx.x * LOCI_THREADS + threadIdx.x; t < lanes; t += (int64_t)gridDim.x * LOCI_THREADS) {
        const LaneWords lw(bits, t);
        if (lw.empty()) continue;
        int64_t rs = (int64_t)(off[t] >> 32), re = (int64_t)(uint32_t)off[t];
#pragma unroll
        for (int j = 0; j < LOCI_LANE_WORDS; ++j) {
            if (!lw.w[j]) continue;
            const int64_t base = (LOCI_LANE_WORDS * t + j) * 32;
            for (uint32_t s = lw.starts(j); s; s &= s - 1) run_start[rs++] = (int32_t)(base + __ffs((int)s) - 1);
            for (uint32_t e = lw.ends(j); e; e &= e - 1) run_end[re++] = (int32_t)(base + __ffs((int)e));
        }
    }
}

struct JoinIn {
    const int32_t *run_start, *run_end;
    int32_t gap;
    __host__ __device__ uint64_t operator()(int64_t k) const {
        const bool head = k == 0 || run_start[k] - run_end[k - 1] > gap;      // (both in [0, 2^31), the later one first: no overflow)
        return (uint64_t)head << 32 | (uint32_t)(run_end[k] - run_start[k]);  // (the lengths sum to at most L < 2^31)
    }
};

__global__ void __launch_bounds__(LOCI_THREADS) locus_bounds_kernel(const int32_t *__restrict__ run_start, const int32_t *__restrict__ run_end,
                                                                    int64_t n_runs, const uint64_t *__restrict__ join,
                                                                    int32_t *__restrict__ locus_start, int32_t *__restrict__ post,
                                                                    RibbitLocus *__restrict__ loci, uint32_t *__restrict__ count) {
    for (int64_t k = (int64_t)blockIdx.x * LOCI_THREADS + threadIdx.x; k < n_runs; k += (int64_t)gridDim.x * LOCI_THREADS) {
        const uint32_t id1 = (uint32_t)(join[k] >> 32);      // locus id + 1
        if (k == 0 || (uint32_t)(join[k - 1] >> 32) != id1) {
            locus_start[id1 - 1] = run_start[k];
            loci[id1 - 1].start = run_start[k];
        }
        if (k == n_runs - 1 || (uint32_t)(join[k + 1] >> 32) != id1) {
            loci[id1 - 1].end = run_end[k];
            post[id1 - 1] = (int32_t)(uint32_t)join[k];
        }
        if (k == n_runs - 1) count[0] = id1;
    }
}

__global__ void __launch_bounds__(LOCI_THREADS) locus_rows_kernel(const int32_t *__restrict__ iv, int64_t n, int64_t length,
                                                                  const uint64_t *__restrict__ join, int64_t n_runs,
                                                                  const int32_t *__restrict__ locus_start, RibbitLocus *__restrict__ loci,
                                                                  unsigned long long *__restrict__ key) {
    const int64_t n_loci = (int64_t)(join[n_runs - 1] >> 32);
    for (int64_t i = (int64_t)blockIdx.x * LOCI_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * LOCI_THREADS) {
        const int64_t s = max((int64_t)iv[2 * i], (int64_t)0), e = min((int64_t)iv[2 * i + 1], length);
        if (s >= e) continue;
        int64_t lo = 0, hi = n_loci;          // the first locus that starts behind s
        while (lo < hi) {
            const int64_t mid = lo + (hi - lo) / 2;
            if (locus_start[mid] <= s) lo = mid + 1; else hi = mid;
        }
        if (lo == 0) continue;                // (never: a non-empty row is covered, so a locus starts at or before it)
        atomicAdd(&loci[lo - 1].rows, 1);
        atomicMax(key + (lo - 1), (unsigned long long)(e - s) << 32 | (0xFFFFFFFFull - (unsigned long long)i));
    }
}

__global__ void __launch_bounds__(LOCI_THREADS) locus_finish_kernel(const uint64_t *__restrict__ join, int64_t n_runs, const int32_t *__restrict__ post,
                                                                    const unsigned long long *__restrict__ key, RibbitLocus *__restrict__ loci) {
    const int64_t n_loci = (int64_t)(join[n_runs - 1] >> 32);
    for (int64_t id = (int64_t)blockIdx.x * LOCI_THREADS + threadIdx.x; id < n_loci; id += (int64_t)gridDim.x * LOCI_THREADS) {
        loci[id].covered = post[id] - (id ? post[id - 1] : 0);
        loci[id].best_row = (int32_t)(0xFFFFFFFFu - (uint32_t)key[id]);
    }
}

// covered positions of word w inside [lo, hi), for a word that holds some of them
__device__ inline int32_t window_word(const uint32_t *__restrict__ bits, int64_t w, int64_t lo, int64_t hi) {
    uint32_t m = ~0u;
    if (w == (lo >> 5)) m &= ~0u << (lo & 31);
    if (w == ((hi - 1) >> 5)) m &= ~0u >> (31 - ((hi - 1) & 31));
    return __popc(bits[w] & m);
}

__global__ void __launch_bounds__(LOCI_THREADS) density_lane_kernel(const uint32_t *__restrict__ bits, int64_t length, int64_t window,
                                                                    int64_t n_windows, int32_t *__restrict__ covered) {
    for (int64_t k = (int64_t)blockIdx.x * LOCI_THREADS + threadIdx.x; k < n_windows; k += (int64_t)gridDim.x * LOCI_THREADS) {
        const int64_t lo = k * window, hi = min(lo + window, length);
        int32_t sum = 0;
        for (int64_t w = lo >> 5; w <= (hi - 1) >> 5; ++w) sum += window_word(bits, w, lo, hi);
        covered[k] = sum;
    }
}

__global__ void __launch_bounds__(LOCI_THREADS) density_wave_kernel(const uint32_t *__restrict__ bits, int64_t length, int64_t window,
                                                                    int64_t n_windows, int32_t *__restrict__ covered) {
    const int lane = threadIdx.x & 63;
    const int64_t waves = (int64_t)gridDim.x * (LOCI_THREADS / 64);
    for (int64_t k = (int64_t)blockIdx.x * (LOCI_THREADS / 64) + (threadIdx.x >> 6); k < n_windows; k += waves) {
        const int64_t lo = k * window, hi = min(lo + window, length);
        int32_t sum = 0;
        for (int64_t w = (lo >> 5) + lane; w <= (hi - 1) >> 5; w += 64) sum += window_word(bits, w, lo, hi);
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) sum += __shfl_down(sum, d);
        if (lane == 0) covered[k] = sum;
    }
}

auto run_counts(const uint32_t *bits) {
    return rocprim::make_transform_iterator(rocprim::make_counting_iterator<int64_t>(0), RunCounts{bits});
}

auto join_in(const int32_t *run_start, const int32_t *run_end, int32_t gap) {
    return rocprim::make_transform_iterator(rocprim::make_counting_iterator<int64_t>(0), JoinIn{run_start, run_end, gap});
}

template <typename It>
hipError_t scan_packed(void *scratch, size_t &bytes, It in, uint64_t *out, int64_t items, hipStream_t stream) {
    return rocprim::inclusive_scan(scratch, bytes, in, out, (size_t)items, rocprim::plus<uint64_t>(), stream);
}

}  // namespace

size_t loci_scan_scratch_bytes(int64_t items) {
    size_t a = 0, b = 0;
    (void)scan_packed(nullptr, a, run_counts(nullptr), (uint64_t *)nullptr, items, 0);
    (void)scan_packed(nullptr, b, join_in(nullptr, nullptr, 0), (uint64_t *)nullptr, items, 0);
    return std::max(a, b) + 256;
}

hipError_t launch_run_ranks(const uint32_t *bits, int64_t length, uint64_t *off, void *scratch, size_t scratch_bytes, hipStream_t stream) {
    const hipError_t e = hipMemsetAsync(off, 0, sizeof(uint64_t), stream);
    if (e != hipSuccess) return e;
    return scan_packed(scratch, scratch_bytes, run_counts(bits), off + 1, loci_lanes(length), stream);
}

void launch_run_bounds(const uint32_t *bits, int64_t length, const uint64_t *off, int32_t *run_start, int32_t *run_end, hipStream_t stream) {
    const int64_t lanes = loci_lanes(length);
    hipLaunchKernelGGL(run_bounds_kernel, dim3(grid_for(lanes, LOCI_THREADS, LOCI_MAX_BLOCKS)), dim3(LOCI_THREADS), 0, stream, bits, lanes, off, run_start, run_end);
}

hipError_t launch_loci(const int32_t *run_start, const int32_t *run_end, int64_t n_runs, int32_t gap, const int32_t *intervals, int64_t n,
                       int64_t length, uint64_t *join, int32_t *locus_start, int32_t *post, unsigned long long *key, RibbitLocus *loci,
                       uint32_t *count, void *scratch, size_t scratch_bytes, hipStream_t stream) {
    if (n_runs <= 0) return hipSuccess;
    hipError_t e = scan_packed(scratch, scratch_bytes, join_in(run_start, run_end, gap), join, n_runs, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(locus_bounds_kernel, dim3(grid_for(n_runs, LOCI_THREADS, LOCI_MAX_BLOCKS)), dim3(LOCI_THREADS), 0, stream, run_start, run_end, n_runs, join, locus_start,
                       post, loci, count);
    hipLaunchKernelGGL(locus_rows_kernel, dim3(grid_for(n, LOCI_THREADS, LOCI_MAX_BLOCKS)), dim3(LOCI_THREADS), 0, stream, intervals, n, length, join, n_runs, locus_start, loci, key);
    hipLaunchKernelGGL(locus_finish_kernel, dim3(grid_for(n_runs, LOCI_THREADS, LOCI_MAX_BLOCKS)), dim3(LOCI_THREADS), 0, stream, join, n_runs, post, key, loci);
    return hipGetLastError();
}

void launch_density(const uint32_t *bits, int64_t length, int64_t window, int64_t n_windows, int32_t *covered, hipStream_t stream) {
    if (n_windows <= 0) return;
    if (window < DENSITY_WAVE_FROM)
        hipLaunchKernelGGL(density_lane_kernel, dim3(grid_for(n_windows, LOCI_THREADS, LOCI_MAX_BLOCKS)), dim3(LOCI_THREADS), 0, stream, bits, length, window, n_windows, covered);
    else
        hipLaunchKernelGGL(density_wave_kernel, dim3(grid_for(n_windows * 64, LOCI_THREADS, LOCI_MAX_BLOCKS)), dim3(LOCI_THREADS), 0, stream, bits, length, window, n_windows, covered);
}

}  // namespace rb
