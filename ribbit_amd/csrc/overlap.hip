// overlap.hip -- the rows of the loaded record set against a second set of intervals, OTHER (api_overlap.cpp:
// ribbit_hip_record_overlap).  A is the coverage bitmap of the rows (the mask's, build_coverage), B the bitmap that mask.hip's
// coverage kernel makes of OTHER's intervals, both coverage_words(length) words.  On the handle's stream:
//   block counts: a lane takes LOCI_LANE_WORDS consecutive words of each bitmap (two dwordx4 loads each; the padding makes that
//                 bound-check-free): popc of A, of B and of A & B.  The first two, packed into one 64-bit word, are the lane's
//                 entry of `sums`; all three are summed over the wave and leave as one atomic per wave and counter
//   block ranks:  exclusive scan of `sums` (rocPRIM): rank[t] = (covered positions of A before block t) << 32 | (of B)
//   other:        one lane per OTHER interval, clipped in 64-bit: its sort keys (s' and e'; an empty interval gets `length` for
//                 both, which no search below counts), and whether it holds a position of A (rank(e') - rank(s') > 0);
//                 `other` and `other_hit` are a ballot and a popc per wave, summed in a register, one atomic each per wave
//   sort:         the keys of the starts and of the ends, each by a rocPRIM radix sort of the bits a position can have
//   rows:         one lane per row, clipped in 64-bit: bases = rank(e') - rank(s') in B, others = (starts < e') - (ends <= s')
//                 by two binary searches (an interval that ends at or before s' also starts before e', so the difference is
//                 the number that does neither); `rows` and `rows_hit` as `other` and `other_hit`
// rank(p) = the prefix of p's block + the popc of the whole words before p in the block (at most 7) + the popc of p's word below
// p.  p = length lies in a word of the bitmap (length / 32 + 1 words hold positions, coverage_words is more).
#include <cstring>

#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>

#include "bit_blocks.h"
#include "row_kernels.h"

namespace rb {

namespace {

// (ROW_MAX_BLOCKS, four blocks per CU: a stride of the block counts covers 2^26 positions, and a record or a row set beyond one
// stride is still small enough to test)

// totals: rows_bases, other_bases, both_bases
__global__ void __launch_bounds__(ROW_THREADS) overlap_counts_kernel(const uint32_t *__restrict__ a_bits, const uint32_t *__restrict__ b_bits, int64_t lanes,
                                                                     uint64_t *__restrict__ sums, unsigned long long *__restrict__ totals) {
    unsigned long long in_a = 0, in_b = 0, in_both = 0;
    for (int64_t t = (int64_t)blockIdx.x * ROW_THREADS + threadIdx.x; t < lanes; t += (int64_t)gridDim.x * ROW_THREADS) {
        uint32_t a[LOCI_LANE_WORDS], b[LOCI_LANE_WORDS];
        load_block(a_bits, t, a);
        load_block(b_bits, t, b);
        uint32_t any = 0;
#pragma unroll
        for (int j = 0; j < LOCI_LANE_WORDS; ++j) any |= a[j] | b[j];
        uint32_t na = 0, nb = 0, nab = 0;
        if (any) {
#pragma unroll
            for (int j = 0; j < LOCI_LANE_WORDS; ++j) {
                na += (uint32_t)__popc(a[j]);
                nb += (uint32_t)__popc(b[j]);
                nab += (uint32_t)__popc(a[j] & b[j]);
            }
        }
        sums[t] = (uint64_t)na << 32 | nb;      // (a record has fewer than 2^31 positions: the low half never carries)
        in_a += na;
        in_b += nb;
        in_both += nab;
    }
    in_a = wave_sum(in_a);
    in_b = wave_sum(in_b);
    in_both = wave_sum(in_both);
    if ((threadIdx.x & 63) == 0) {
        if (in_a) atomicAdd(totals + 0, in_a);
        if (in_b) atomicAdd(totals + 1, in_b);
        if (in_both) atomicAdd(totals + 2, in_both);
    }
}

// covered positions of the bitmap before p, 0 <= p <= length; HIGH: the bitmap's prefixes are the high halves of `rank`
template <bool HIGH>
__device__ inline uint32_t rank_at(const uint32_t *__restrict__ bits, const uint64_t *__restrict__ rank, int64_t p) {
    const uint64_t r = rank[block_of(p)];
    return (HIGH ? (uint32_t)(r >> 32) : (uint32_t)r) + ones_before_in_block(bits, p);
}

// One lane per interval, intervals in grid-stride waves (every lane of a wave takes the same number of turns: the ballots see
// whole waves).  counts: the number of non-empty intervals, and of those that hold a position of the other bitmap.
__global__ void __launch_bounds__(ROW_THREADS) overlap_other_kernel(const int32_t *__restrict__ iv, int64_t n, int64_t length, const uint32_t *__restrict__ a_bits,
                                                                    const uint64_t *__restrict__ rank, uint32_t *__restrict__ starts,
                                                                    uint32_t *__restrict__ ends, int32_t *__restrict__ counts) {
    const int lane = threadIdx.x & 63;
    const int64_t waves = (int64_t)gridDim.x * (ROW_THREADS / 64);
    int32_t some = 0, hit = 0;
    for (int64_t base = ((int64_t)blockIdx.x * (ROW_THREADS / 64) + (threadIdx.x >> 6)) * 64; base < n; base += waves * 64) {
        const int64_t i = base + lane;
        bool has = false, hits = false;
        if (i < n) {
            const auto [s, e] = clip_row(iv, i, length);
            has = s < e;
            starts[i] = (uint32_t)(has ? s : length);
            ends[i] = (uint32_t)(has ? e : length);
            hits = has && rank_at<true>(a_bits, rank, e) != rank_at<true>(a_bits, rank, s);
        }
        some += (int32_t)__popcll(__ballot(has));
        hit += (int32_t)__popcll(__ballot(hits));
    }
    if (lane == 0) {
        if (some) atomicAdd(counts + 0, some);
        if (hit) atomicAdd(counts + 1, hit);
    }
}

__device__ inline int32_t count_below(const uint32_t *__restrict__ keys, int64_t m, uint32_t limit) {      // keys < limit
    int64_t lo = 0, hi = m;
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (keys[mid] < limit) lo = mid + 1; else hi = mid;
    }
    return (int32_t)lo;
}

// per_row: (others, bases) of every row; counts: the number of non-empty rows, and of those with bases > 0
__global__ void __launch_bounds__(ROW_THREADS) overlap_rows_kernel(const int32_t *__restrict__ iv, int64_t n, int64_t length, const uint32_t *__restrict__ b_bits,
                                                                   const uint64_t *__restrict__ rank, const uint32_t *__restrict__ starts,
                                                                   const uint32_t *__restrict__ ends, int64_t n_other, int32_t *__restrict__ per_row,
                                                                   int32_t *__restrict__ counts) {
    const int lane = threadIdx.x & 63;
    const int64_t waves = (int64_t)gridDim.x * (ROW_THREADS / 64);
    int32_t some = 0, hit = 0;
    for (int64_t base = ((int64_t)blockIdx.x * (ROW_THREADS / 64) + (threadIdx.x >> 6)) * 64; base < n; base += waves * 64) {
        const int64_t i = base + lane;
        bool has = false, hits = false;
        if (i < n) {
            const auto [s, e] = clip_row(iv, i, length);
            int32_t others = 0, bases = 0;
            has = s < e;
            if (has) {
                bases = (int32_t)(rank_at<false>(b_bits, rank, e) - rank_at<false>(b_bits, rank, s));
                // (s + 1 <= length: the empty intervals' keys are never below it)
                others = count_below(starts, n_other, (uint32_t)e) - count_below(ends, n_other, (uint32_t)s + 1u);
            }
            per_row[2 * i] = others;
            per_row[2 * i + 1] = bases;
            hits = bases > 0;
        }
        some += (int32_t)__popcll(__ballot(has));
        hit += (int32_t)__popcll(__ballot(hits));
    }
    if (lane == 0) {
        if (some) atomicAdd(counts + 0, some);
        if (hit) atomicAdd(counts + 1, hit);
    }
}

hipError_t scan_ranks(void *scratch, size_t &bytes, const uint64_t *sums, uint64_t *rank, int64_t lanes, hipStream_t stream) {
    return rocprim::exclusive_scan(scratch, bytes, sums, rank, (uint64_t)0, (size_t)lanes, rocprim::plus<uint64_t>(), stream);
}

// over the bits a key can have: the positions 0 .. length
hipError_t sort_keys(void *scratch, size_t &bytes, const uint32_t *in, uint32_t *out, int64_t m, int64_t length, hipStream_t stream) {
    return rocprim::radix_sort_keys(scratch, bytes, in, out, (size_t)m, 0u, bits_for(length), stream);
}

}  // namespace

OverlapLayout overlap_layout(int64_t n, int64_t n_other, int64_t length) {
    size_t a = 0, b = 0;
    (void)scan_ranks(nullptr, a, nullptr, nullptr, loci_lanes(length), 0);
    if (n_other > 0) (void)sort_keys(nullptr, b, nullptr, nullptr, n_other, length, 0);
    OverlapLayout at{};
    WorkCarver w;
    at.other = w.take(2 * (size_t)n_other * sizeof(int32_t));
    at.b_bits = w.take((size_t)coverage_words(length) * sizeof(uint32_t));
    at.ranks = w.take(2 * (size_t)loci_lanes(length) * sizeof(uint64_t));
    at.keys = w.take(4 * (size_t)n_other * sizeof(uint32_t));
    at.totals = w.take(sizeof(RibbitOverlapTotals));
    at.per_row = w.take(2 * (size_t)n * sizeof(int32_t));
    w.close(at, std::max(a, b));
    return at;
}

hipError_t launch_overlap(const uint32_t *a_bits, int64_t length, const int32_t *rows, int64_t n, const int32_t *other_host, int64_t n_other, uint8_t *work,
                          size_t work_bytes, const OverlapLayout &at, hipStream_t stream) {
    if (work_bytes < at.bytes) return hipErrorInvalidValue;
    const int64_t lanes = loci_lanes(length);
    int32_t *other = region<int32_t>(work, at.other);
    uint32_t *b_bits = region<uint32_t>(work, at.b_bits);
    uint64_t *sums = region<uint64_t>(work, at.ranks), *rank = sums + lanes;
    uint32_t *starts = region<uint32_t>(work, at.keys), *ends = starts + n_other, *starts_sorted = ends + n_other, *ends_sorted = starts_sorted + n_other;
    RibbitOverlapTotals *totals = region<RibbitOverlapTotals>(work, at.totals);
    int32_t *per_row = region<int32_t>(work, at.per_row);
    void *scratch = work + at.scratch;
    const size_t scratch_bytes = at.scratch_bytes;
    hipError_t e = hipMemsetAsync(totals, 0, sizeof(RibbitOverlapTotals), stream);
    if (e != hipSuccess) return e;
    if ((e = hipMemsetAsync(b_bits, 0, (size_t)coverage_words(length) * sizeof(uint32_t), stream)) != hipSuccess) return e;
    if (n_other > 0) {
        if ((e = hipMemcpyAsync(other, other_host, 2 * (size_t)n_other * sizeof(int32_t), hipMemcpyHostToDevice, stream)) != hipSuccess) return e;
        launch_mask_coverage(other, n_other, length, b_bits, stream);
    }
    hipLaunchKernelGGL(overlap_counts_kernel, dim3(grid_for(lanes, ROW_THREADS, ROW_MAX_BLOCKS)), dim3(ROW_THREADS), 0, stream, a_bits, b_bits, lanes, sums,
                       reinterpret_cast<unsigned long long *>(&totals->rows_bases));
    size_t bytes = scratch_bytes;
    if ((e = scan_ranks(scratch, bytes, sums, rank, lanes, stream)) != hipSuccess) return e;
    if (n_other > 0) {
        hipLaunchKernelGGL(overlap_other_kernel, dim3(grid_for(n_other, ROW_THREADS, ROW_MAX_BLOCKS)), dim3(ROW_THREADS), 0, stream, other, n_other, length, a_bits,
                           rank, starts, ends, &totals->other);
        bytes = scratch_bytes;
        if ((e = sort_keys(scratch, bytes, starts, starts_sorted, n_other, length, stream)) != hipSuccess) return e;
        bytes = scratch_bytes;
        if ((e = sort_keys(scratch, bytes, ends, ends_sorted, n_other, length, stream)) != hipSuccess) return e;
    }
    if (n > 0)
        hipLaunchKernelGGL(overlap_rows_kernel, dim3(grid_for(n, ROW_THREADS, ROW_MAX_BLOCKS)), dim3(ROW_THREADS), 0, stream, rows, n, length, b_bits, rank,
                           starts_sorted, ends_sorted, n_other, per_row, &totals->rows);
    return hipGetLastError();
}

}  // namespace rb
