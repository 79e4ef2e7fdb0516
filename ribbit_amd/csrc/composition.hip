// composition.hip -- the base composition of every row, of its flanks and of every window of the loaded record
// (api_composition.cpp: ribbit_hip_record_composition, ribbit_hip_record_base_windows; include/ribbit_hip.h has the contract).
// Nothing here reads the ASCII: a base's class is in the scan's own bit planes (device_planes.h), C = ~hi & lo, G = hi & ~lo,
// T = hi & lo, other = brk, and hi and lo are 0 wherever brk is 1, so the three need no mask; A is what is left of a length.
// On the handle's stream:
//   block counts: a lane takes the COMP_BLOCK_WORDS consecutive words of a block of COMP_BLOCK bases from each plane (two
//                 dwordx4 loads each; the planes are whole tiles, so no load needs a bound check): popc of C, G, T and other
//                 as one BaseSums
//   prefix:       exclusive scan of the block counts (rocPRIM, a BaseSums with its own plus): prefix[t] = the four counts of
//                 the positions before block t.  Every field's total is below 2^31.  This depends on the record alone: the
//                 host side keeps it until the next load
//   cover ranks:  the same two steps for the rows' coverage bitmap (the mask's, build_coverage), one uint32 per block; these
//                 belong to the rows and are made again with them, the base prefix is not
//   rows:         one lane per row, clipped in 64-bit before any address is formed: the prefixes at lo, s', e' and hi, each the
//                 scanned value of the position's block + the popc of the whole words before the position in the block (at
//                 most 7) + the popc of the position's word below it; the 13 values are differences
//   windows:      one lane per window: the prefixes at both of its ends, five differences
// brk is 1 for every position >= L: no prefix is taken beyond L, and the one at L counts only the bits below it.  p = L lies in
// a word of every plane and of the bitmap (L / 32 + 1 words hold positions).  The kernels stride beyond ROW_MAX_BLOCKS blocks.
#include <cstring>

#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>

#include "bit_blocks.h"
#include "row_kernels.h"

namespace rb {

namespace {

static_assert(COMP_BLOCK_WORDS == 8 && COMP_BLOCK_WORDS == WORDS_PER_LANE && COMP_BLOCK_WORDS == LOCI_LANE_WORDS,
              "a lane loads its words as two dwordx4, and a block is a lane's words of the scan tile and of the coverage bitmap");
static_assert(TILE_WORDS % COMP_BLOCK_WORDS == 0 && LEAD_WORDS % 4 == 0, "the blocks tile the planes, 16-byte aligned");

struct SumsPlus {
    __host__ __device__ BaseSums operator()(const BaseSums &a, const BaseSums &b) const {
        return BaseSums{a.c + b.c, a.g + b.g, a.t + b.t, a.other + b.other};
    }
};

__device__ inline void add_word(BaseSums &s, uint32_t hi, uint32_t lo, uint32_t brk) {
    s.c += (uint32_t)__popc(~hi & lo);
    s.g += (uint32_t)__popc(hi & ~lo);
    s.t += (uint32_t)__popc(hi & lo);
    s.other += (uint32_t)__popc(brk);
}

__global__ void __launch_bounds__(ROW_THREADS) composition_counts_kernel(const uint32_t *__restrict__ hi, const uint32_t *__restrict__ lo,
                                                                          const uint32_t *__restrict__ brk, int64_t blocks, BaseSums *__restrict__ sums) {
    for (int64_t t = (int64_t)blockIdx.x * ROW_THREADS + threadIdx.x; t < blocks; t += (int64_t)gridDim.x * ROW_THREADS) {
        uint32_t h[COMP_BLOCK_WORDS], l[COMP_BLOCK_WORDS], b[COMP_BLOCK_WORDS];
        load_block(hi, t, h);
        load_block(lo, t, l);
        load_block(brk, t, b);
        BaseSums s{0, 0, 0, 0};
#pragma unroll
        for (int j = 0; j < COMP_BLOCK_WORDS; ++j) add_word(s, h[j], l[j], b[j]);
        sums[t] = s;
    }
}

__global__ void __launch_bounds__(ROW_THREADS) composition_cover_counts_kernel(const uint32_t *__restrict__ bits, int64_t blocks, uint32_t *__restrict__ sums) {
    for (int64_t t = (int64_t)blockIdx.x * ROW_THREADS + threadIdx.x; t < blocks; t += (int64_t)gridDim.x * ROW_THREADS) {
        uint32_t w[COMP_BLOCK_WORDS];
        load_block(bits, t, w);
        uint32_t s = 0;
#pragma unroll
        for (int j = 0; j < COMP_BLOCK_WORDS; ++j) s += (uint32_t)__popc(w[j]);
        sums[t] = s;
    }
}

// C, G, T and other of the positions before p, 0 <= p <= length
__device__ inline BaseSums bases_before(const DevicePlanes &pl, const BaseSums *__restrict__ prefix, int64_t p) {
    const int64_t w = p >> 5, t = block_of(p);
    BaseSums s = prefix[t];
    for (int64_t j = t * COMP_BLOCK_WORDS; j < w; ++j) add_word(s, pl.hi[j], pl.lo[j], pl.brk[j]);
    const uint32_t below = bits_below(p);
    add_word(s, pl.hi[w] & below, pl.lo[w] & below, pl.brk[w] & below);
    return s;
}

// covered positions before p, 0 <= p <= length
__device__ inline uint32_t covered_before(const uint32_t *__restrict__ bits, const uint32_t *__restrict__ rank, int64_t p) {
    return rank[block_of(p)] + ones_before_in_block(bits, p);
}

__global__ void __launch_bounds__(ROW_THREADS) composition_rows_kernel(const int32_t *__restrict__ rows, int64_t n, int32_t flank, DevicePlanes pl,
                                                                        const BaseSums *__restrict__ prefix, const uint32_t *__restrict__ bits,
                                                                        const uint32_t *__restrict__ rank, RibbitRowComposition *__restrict__ out) {
    const int64_t length = pl.length;
    for (int64_t i = (int64_t)blockIdx.x * ROW_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * ROW_THREADS) {
        const int64_t s = min(max((int64_t)rows[2 * i], (int64_t)0), length), e = min(max((int64_t)rows[2 * i + 1], s), length);
        const int64_t lo = max(s - (int64_t)flank, (int64_t)0), hi = min(e + (int64_t)flank, length);
        const BaseSums at_lo = bases_before(pl, prefix, lo), at_s = bases_before(pl, prefix, s), at_e = bases_before(pl, prefix, e),
                       at_hi = bases_before(pl, prefix, hi);
        const uint32_t cov_lo = covered_before(bits, rank, lo), cov_s = covered_before(bits, rank, s), cov_e = covered_before(bits, rank, e),
                       cov_hi = covered_before(bits, rank, hi);
        RibbitRowComposition r;
        r.c = (int32_t)(at_e.c - at_s.c);
        r.g = (int32_t)(at_e.g - at_s.g);
        r.t = (int32_t)(at_e.t - at_s.t);
        r.other = (int32_t)(at_e.other - at_s.other);
        r.a = (int32_t)(e - s) - r.c - r.g - r.t - r.other;
        r.left = (int32_t)(s - lo);
        r.left_gc = (int32_t)((at_s.c - at_lo.c) + (at_s.g - at_lo.g));
        r.left_other = (int32_t)(at_s.other - at_lo.other);
        r.left_covered = (int32_t)(cov_s - cov_lo);
        r.right = (int32_t)(hi - e);
        r.right_gc = (int32_t)((at_hi.c - at_e.c) + (at_hi.g - at_e.g));
        r.right_other = (int32_t)(at_hi.other - at_e.other);
        r.right_covered = (int32_t)(cov_hi - cov_e);
        out[i] = r;
    }
}

__global__ void __launch_bounds__(ROW_THREADS) composition_windows_kernel(DevicePlanes pl, const BaseSums *__restrict__ prefix, int64_t window, int64_t n_windows,
                                                                           RibbitBaseCounts *__restrict__ out) {
    for (int64_t k = (int64_t)blockIdx.x * ROW_THREADS + threadIdx.x; k < n_windows; k += (int64_t)gridDim.x * ROW_THREADS) {
        const int64_t from = k * window, to = min(from + window, pl.length);      // (k < ceil(length / window): from < length)
        const BaseSums a = bases_before(pl, prefix, from), b = bases_before(pl, prefix, to);
        RibbitBaseCounts r;
        r.c = (int32_t)(b.c - a.c);
        r.g = (int32_t)(b.g - a.g);
        r.t = (int32_t)(b.t - a.t);
        r.other = (int32_t)(b.other - a.other);
        r.a = (int32_t)(to - from) - r.c - r.g - r.t - r.other;
        out[k] = r;
    }
}

hipError_t scan_sums(void *scratch, size_t &bytes, const BaseSums *sums, BaseSums *prefix, int64_t blocks, hipStream_t stream) {
    return rocprim::exclusive_scan(scratch, bytes, sums, prefix, BaseSums{0, 0, 0, 0}, (size_t)blocks, SumsPlus(), stream);
}

hipError_t scan_cover(void *scratch, size_t &bytes, const uint32_t *sums, uint32_t *rank, int64_t blocks, hipStream_t stream) {
    return rocprim::exclusive_scan(scratch, bytes, sums, rank, (uint32_t)0, (size_t)blocks, rocprim::plus<uint32_t>(), stream);
}

// cover_blocks: the blocks of the rows' coverage (0: the windows have none); out_bytes: the result.  Either call may have to make
// the record's prefix first, so the scratch serves that scan too.
CompositionLayout composition_layout(size_t cover_blocks, size_t out_bytes, int64_t length) {
    size_t a = 0, b = 0;
    (void)scan_sums(nullptr, a, nullptr, nullptr, loci_lanes(length), 0);
    if (cover_blocks) (void)scan_cover(nullptr, b, nullptr, nullptr, loci_lanes(length), 0);
    CompositionLayout at{};
    WorkCarver w;
    at.cover = w.take(2 * cover_blocks * sizeof(uint32_t));
    at.out = w.take(out_bytes);
    w.close(at, std::max(a, b));
    return at;
}

}  // namespace

CompositionLayout composition_rows_layout(int64_t n, int64_t length) {
    return composition_layout((size_t)loci_lanes(length), (size_t)n * sizeof(RibbitRowComposition), length);
}

CompositionLayout composition_windows_layout(int64_t n_windows, int64_t length) {
    return composition_layout(0, (size_t)n_windows * sizeof(RibbitBaseCounts), length);
}

hipError_t launch_composition_prefix(const DevicePlanes &pl, BaseSums *sums, uint8_t *work, size_t work_bytes, const CompositionLayout &at, hipStream_t stream) {
    if (work_bytes < at.bytes) return hipErrorInvalidValue;
    const int64_t blocks = loci_lanes(pl.length);
    BaseSums *prefix = sums + blocks;
    void *scratch = work + at.scratch;
    hipLaunchKernelGGL(composition_counts_kernel, dim3(grid_for(blocks, ROW_THREADS, ROW_MAX_BLOCKS)), dim3(ROW_THREADS), 0, stream, pl.hi, pl.lo, pl.brk, blocks,
                       sums);
    size_t bytes = at.scratch_bytes;
    const hipError_t e = scan_sums(scratch, bytes, sums, prefix, blocks, stream);
    return e != hipSuccess ? e : hipGetLastError();
}

hipError_t launch_composition_rows(const DevicePlanes &pl, const BaseSums *sums, const uint32_t *bits, const int32_t *rows, int64_t n, int32_t flank, uint8_t *work,
                                   size_t work_bytes, const CompositionLayout &at, hipStream_t stream) {
    if (work_bytes < at.bytes) return hipErrorInvalidValue;
    const int64_t blocks = loci_lanes(pl.length);
    const BaseSums *prefix = sums + blocks;
    uint32_t *cover_sums = region<uint32_t>(work, at.cover), *cover_rank = cover_sums + blocks;
    RibbitRowComposition *out = region<RibbitRowComposition>(work, at.out);
    void *scratch = work + at.scratch;
    hipLaunchKernelGGL(composition_cover_counts_kernel, dim3(grid_for(blocks, ROW_THREADS, ROW_MAX_BLOCKS)), dim3(ROW_THREADS), 0, stream, bits, blocks,
                       cover_sums);
    size_t bytes = at.scratch_bytes;
    const hipError_t e = scan_cover(scratch, bytes, cover_sums, cover_rank, blocks, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(composition_rows_kernel, dim3(grid_for(n, ROW_THREADS, ROW_MAX_BLOCKS)), dim3(ROW_THREADS), 0, stream, rows, n, flank, pl, prefix, bits,
                       cover_rank, out);
    return hipGetLastError();
}

hipError_t launch_composition_windows(const DevicePlanes &pl, const BaseSums *sums, int64_t window, int64_t n_windows, uint8_t *work, size_t work_bytes,
                                      const CompositionLayout &at, hipStream_t stream) {
    if (work_bytes < at.bytes) return hipErrorInvalidValue;
    const BaseSums *prefix = sums + loci_lanes(pl.length);
    RibbitBaseCounts *out = region<RibbitBaseCounts>(work, at.out);
    hipLaunchKernelGGL(composition_windows_kernel, dim3(grid_for(n_windows, ROW_THREADS, ROW_MAX_BLOCKS)), dim3(ROW_THREADS), 0, stream, pl, prefix, window,
                       n_windows, out);
    return hipGetLastError();
}

}  // namespace rb
