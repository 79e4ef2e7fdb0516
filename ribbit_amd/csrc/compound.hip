// compound.hip -- the rows of the loaded record chained into compound loci (api_compound.cpp: ribbit_hip_record_compounds): the
// ordered membership of the rows in gap-joined chains with per-chain counts, as include/ribbit_hip.h states it.  No coverage bitmap
// is read and nothing goes to the host in between.  On the handle's stream, every launch over all n rows:
//   keys:     one lane per row, clipped in 64-bit: key = s' << 32 | e', an empty row gets the all-ones key (no real key equals it:
//             s' < L < 2^31), value = the row's index
//   sort:     a rocPRIM radix sort of pairs over the bits a key can have.  It is stable and the values start ascending, so the order
//             is (s', e', index): the sorted indices are `members`; the empty rows are its tail and are not compacted away
//   reach:    an inclusive rocPRIM max-scan of e' over the sorted order (an empty row brings 0)
//   flags:    one lane per sorted position k: head (k == 0 or s'_k - reach_{k-1} > gap, in 64-bit: gap = INT32_MAX cannot wrap),
//             switch (not a head, and its label is not the label of k - 1) and overlap (not a head, s'_k < reach_{k-1}), one byte
//   chains:   an inclusive rocPRIM sum-scan of the head bits: the chain id of every position, from 1
//   keys2:    one lane per position: key = chain id << 32 | label biased to unsigned (negative labels order below the others), an
//             empty row all ones again; a head writes where its chain starts, the last non-empty position writes r behind the
//             last chain's start and the two counts (no atomics: each of these words has one writer)
//   sort2:    a rocPRIM radix sort of those keys alone.  A chain's positions stay its positions, so a label that is not its
//             predecessor's in this order is a distinct label of the chain at a position of the chain
//   sums:     an inclusive rocPRIM scan of (width, switch, overlap, distinct) per position, int64 for the widths
//   finish:   one lane per chain: its sums are the difference of two prefixes, its end the reach of its last position: O(1) however
//             long the chain is
// Two sorts because the two orders answer different questions: (s', e', index) is the membership and decides the chains, and only
// once the chains are known can the labels be ordered within them to count the distinct ones.
#include <cstring>

#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>

#include "row_kernels.h"

namespace rb {

namespace {

constexpr uint64_t EMPTY_KEY = ~(uint64_t)0;
enum : uint8_t { HEAD = 1, SWITCH = 2, OVERLAP = 4 };

__global__ void __launch_bounds__(ROW_THREADS) compound_keys_kernel(const int32_t *__restrict__ iv, int64_t n, int64_t length, uint64_t *__restrict__ keys,
                                                                         int32_t *__restrict__ index) {
    for (int64_t i = (int64_t)blockIdx.x * ROW_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * ROW_THREADS) {
        const auto [s, e] = clip_row(iv, i, length);
        keys[i] = s < e ? (uint64_t)s << 32 | (uint64_t)e : EMPTY_KEY;
        index[i] = (int32_t)i;
    }
}

// the e' of the sorted keys, 0 for the empty rows of the tail
struct EndsInOrder {
    const uint64_t *sorted;
    __host__ __device__ uint32_t operator()(int64_t k) const {
        const uint64_t key = sorted[k];
        return key == EMPTY_KEY ? 0u : (uint32_t)key;
    }
};

__global__ void __launch_bounds__(ROW_THREADS) compound_flags_kernel(const uint64_t *__restrict__ sorted, const int32_t *__restrict__ order,
                                                                          const uint32_t *__restrict__ reach, const int32_t *__restrict__ labels, int64_t n,
                                                                          int32_t gap, uint8_t *__restrict__ flags) {
    for (int64_t k = (int64_t)blockIdx.x * ROW_THREADS + threadIdx.x; k < n; k += (int64_t)gridDim.x * ROW_THREADS) {
        const uint64_t key = sorted[k];
        uint8_t f = 0;
        if (key != EMPTY_KEY) {
            if (k == 0) {
                f = HEAD;
            } else {
                const int64_t s = (int64_t)(key >> 32), before = (int64_t)reach[k - 1];
                if (s - before > (int64_t)gap) f = HEAD;
                else f = (uint8_t)((labels[order[k]] != labels[order[k - 1]] ? SWITCH : 0) | (s < before ? OVERLAP : 0));
            }
        }
        flags[k] = f;
    }
}

struct HeadBits {
    const uint8_t *flags;
    __host__ __device__ uint32_t operator()(int64_t k) const { return flags[k] & HEAD; }
};

__global__ void __launch_bounds__(ROW_THREADS) compound_keys2_kernel(const uint64_t *__restrict__ sorted, const int32_t *__restrict__ order,
                                                                          const uint32_t *__restrict__ chain, const uint8_t *__restrict__ flags,
                                                                          const int32_t *__restrict__ labels, int64_t n, uint64_t *__restrict__ keys2,
                                                                          int32_t *__restrict__ first, CompoundTotals *__restrict__ totals) {
    for (int64_t k = (int64_t)blockIdx.x * ROW_THREADS + threadIdx.x; k < n; k += (int64_t)gridDim.x * ROW_THREADS) {
        if (sorted[k] == EMPTY_KEY) { keys2[k] = EMPTY_KEY; continue; }
        const uint32_t c = chain[k];                     // 1 .. n
        keys2[k] = (uint64_t)c << 32 | (uint64_t)((uint32_t)labels[order[k]] ^ 0x80000000u);
        if (flags[k] & HEAD) first[c - 1] = (int32_t)k;
        if (k == n - 1 || sorted[k + 1] == EMPTY_KEY) {      // the last non-empty position: r = k + 1
            first[c] = (int32_t)(k + 1);
            totals->rows = (uint32_t)(k + 1);
            totals->chains = c;
        }
    }
}

// what position k brings to its chain: its width and flags in the first order, and whether the label at k in the second order is
// not the label before it (the first position of a chain differs from its predecessor by the chain id)
struct SumsOfPosition {
    const uint64_t *sorted, *sorted2;
    const uint8_t *flags;
    __host__ __device__ CompoundSums operator()(int64_t k) const {
        const uint64_t key = sorted[k];
        if (key == EMPTY_KEY) return CompoundSums{0, 0, 0, 0, 0};
        const uint8_t f = flags[k];
        return CompoundSums{(unsigned long long)((uint32_t)key - (uint32_t)(key >> 32)), (f & SWITCH) ? 1u : 0u, (f & OVERLAP) ? 1u : 0u,
                            k == 0 || sorted2[k] != sorted2[k - 1] ? 1u : 0u, 0};
    }
};

struct AddSums {
    __host__ __device__ CompoundSums operator()(const CompoundSums &a, const CompoundSums &b) const {
        return CompoundSums{a.bases + b.bases, a.switches + b.switches, a.overlaps + b.overlaps, a.classes + b.classes, 0};
    }
};

__global__ void __launch_bounds__(ROW_THREADS) compound_finish_kernel(const uint64_t *__restrict__ sorted, const uint32_t *__restrict__ reach,
                                                                           const int32_t *__restrict__ first, const CompoundSums *__restrict__ sums,
                                                                           const CompoundTotals *__restrict__ totals, int64_t n,
                                                                           RibbitCompound *__restrict__ compounds) {
    const int64_t count = min((int64_t)totals->chains, n);
    for (int64_t c = (int64_t)blockIdx.x * ROW_THREADS + threadIdx.x; c < count; c += (int64_t)gridDim.x * ROW_THREADS) {
        const int64_t f = first[c], l = first[c + 1];      // the chain's positions are [f, l)
        if (f < 0 || l <= f || l > n) { compounds[c] = RibbitCompound{0, 0, 0, 0, 0, 0, 0, -1, 0}; continue; }      // (never: the host refuses it)
        const CompoundSums to = sums[l - 1];
        const CompoundSums from = f ? sums[f - 1] : CompoundSums{0, 0, 0, 0, 0};
        compounds[c] = RibbitCompound{(int64_t)(to.bases - from.bases), (int32_t)(sorted[f] >> 32), (int32_t)reach[l - 1], (int32_t)(l - f),
                                      (int32_t)(to.classes - from.classes), (int32_t)(to.switches - from.switches), (int32_t)(to.overlaps - from.overlaps),
                                      (int32_t)f, 0};
    }
}

// the bits a key can have: the starts 0 .. length - 1 in its high half, below the all-ones of an empty row
hipError_t sort_rows(void *scratch, size_t &bytes, const uint64_t *keys, uint64_t *sorted, const int32_t *index, int32_t *order, int64_t n, int64_t length,
                     hipStream_t stream) {
    return rocprim::radix_sort_pairs(scratch, bytes, keys, sorted, index, order, (size_t)n, 0u, 32 + bits_for(length), stream);
}

hipError_t scan_reach(void *scratch, size_t &bytes, const uint64_t *sorted, uint32_t *reach, int64_t n, hipStream_t stream) {
    return rocprim::inclusive_scan(scratch, bytes, rocprim::make_transform_iterator(rocprim::make_counting_iterator<int64_t>(0), EndsInOrder{sorted}), reach,
                                   (size_t)n, rocprim::maximum<uint32_t>(), stream);
}

hipError_t scan_heads(void *scratch, size_t &bytes, const uint8_t *flags, uint32_t *chain, int64_t n, hipStream_t stream) {
    return rocprim::inclusive_scan(scratch, bytes, rocprim::make_transform_iterator(rocprim::make_counting_iterator<int64_t>(0), HeadBits{flags}), chain,
                                   (size_t)n, rocprim::plus<uint32_t>(), stream);
}

// the chain ids 1 .. n in the high half, below the all-ones of an empty row
hipError_t sort_labels(void *scratch, size_t &bytes, const uint64_t *keys2, uint64_t *sorted2, int64_t n, hipStream_t stream) {
    return rocprim::radix_sort_keys(scratch, bytes, keys2, sorted2, (size_t)n, 0u, 32 + bits_for(n + 1), stream);
}

hipError_t scan_sums(void *scratch, size_t &bytes, const uint64_t *sorted, const uint64_t *sorted2, const uint8_t *flags, CompoundSums *sums, int64_t n,
                     hipStream_t stream) {
    return rocprim::inclusive_scan(scratch, bytes,
                                   rocprim::make_transform_iterator(rocprim::make_counting_iterator<int64_t>(0), SumsOfPosition{sorted, sorted2, flags}), sums,
                                   (size_t)n, AddSums(), stream);
}

}  // namespace

CompoundLayout compound_layout(int64_t n, int64_t length) {
    const size_t rows = (size_t)n;
    size_t a = 0, b = 0, c = 0, d = 0, e = 0;
    (void)sort_rows(nullptr, a, nullptr, nullptr, nullptr, nullptr, n, length, 0);
    (void)scan_reach(nullptr, b, nullptr, nullptr, n, 0);
    (void)scan_heads(nullptr, c, nullptr, nullptr, n, 0);
    (void)sort_labels(nullptr, d, nullptr, nullptr, n, 0);
    (void)scan_sums(nullptr, e, nullptr, nullptr, nullptr, nullptr, n, 0);
    CompoundLayout at{};
    WorkCarver w;
    at.keys = w.take(3 * rows * sizeof(uint64_t));
    at.work = w.take((3 * rows + 1) * sizeof(int32_t));
    at.sums = w.take(rows * sizeof(CompoundSums));
    at.flags = w.take(rows);
    at.totals = w.take(sizeof(CompoundTotals));
    at.compounds = w.take(rows * sizeof(RibbitCompound));
    at.members = w.take(rows * sizeof(int32_t));
    w.close(at, std::max(std::max(a, b), std::max(c, std::max(d, e))));
    return at;
}

hipError_t launch_compounds(const int32_t *rows, const int32_t *labels, int64_t n, int64_t length, int32_t gap, uint8_t *work, size_t work_bytes,
                            const CompoundLayout &at, hipStream_t stream) {
    if (work_bytes < at.bytes) return hipErrorInvalidValue;
    uint64_t *keys = region<uint64_t>(work, at.keys), *sorted = keys + n, *sorted2 = keys + 2 * n;
    uint64_t *keys2 = keys;                         // (the unsorted keys and indices are done with after the first sort)
    int32_t *index = region<int32_t>(work, at.work), *first = index + 2 * n;
    uint32_t *chain = reinterpret_cast<uint32_t *>(index), *reach = chain + n;
    CompoundSums *sums = region<CompoundSums>(work, at.sums);
    uint8_t *flags = region<uint8_t>(work, at.flags);
    CompoundTotals *totals = region<CompoundTotals>(work, at.totals);
    RibbitCompound *compounds = region<RibbitCompound>(work, at.compounds);
    int32_t *members = region<int32_t>(work, at.members);
    void *scratch = work + at.scratch;
    const size_t scratch_bytes = at.scratch_bytes;
    const dim3 grid(grid_for(n, ROW_THREADS, ROW_MAX_BLOCKS)), block(ROW_THREADS);
    hipError_t e = hipMemsetAsync(totals, 0, sizeof(CompoundTotals), stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(compound_keys_kernel, grid, block, 0, stream, rows, n, length, keys, index);
    size_t bytes = scratch_bytes;
    if ((e = sort_rows(scratch, bytes, keys, sorted, index, members, n, length, stream)) != hipSuccess) return e;
    bytes = scratch_bytes;
    if ((e = scan_reach(scratch, bytes, sorted, reach, n, stream)) != hipSuccess) return e;
    hipLaunchKernelGGL(compound_flags_kernel, grid, block, 0, stream, sorted, members, reach, labels, n, gap, flags);
    bytes = scratch_bytes;
    if ((e = scan_heads(scratch, bytes, flags, chain, n, stream)) != hipSuccess) return e;
    hipLaunchKernelGGL(compound_keys2_kernel, grid, block, 0, stream, sorted, members, chain, flags, labels, n, keys2, first, totals);
    bytes = scratch_bytes;
    if ((e = sort_labels(scratch, bytes, keys2, sorted2, n, stream)) != hipSuccess) return e;
    bytes = scratch_bytes;
    if ((e = scan_sums(scratch, bytes, sorted, sorted2, flags, sums, n, stream)) != hipSuccess) return e;
    hipLaunchKernelGGL(compound_finish_kernel, grid, block, 0, stream, sorted, reach, first, sums, totals, n, compounds);
    return hipGetLastError();
}

}  // namespace rb
