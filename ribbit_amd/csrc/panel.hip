// panel.hip -- primer pairs pooled into multiplex PCR panels: which pairs may not share a tube, their degrees, the Welsh-Powell
// order and the first fit along it (include/ribbit_hip.h has the contract, kernels.h the layout and the order of the launches).
// No record is read.
//   panel_items_kernel      a lane per pair, once: both oligos as 64 bits (the right one reverse-complemented here, once), both
//                           again with their bases reversed, which is what a placement takes of its partner (primer_shortlist.h),
//                           the span in 64 bits, the group and the size range.  A row without a pair has kl = 0.
//   panel_conflicts_kernel  THE HOT PATH: n^2 pair-to-pair tests of four duplexes, each up to 63 placements of one shift, one XOR
//                           and a few AND-shifts.  A block is one wavefront; lane t owns row 64 blockIdx.x + t and keeps its item
//                           in registers.  blockIdx.y is a chunk of column words.  Per word the wavefront stages the 64 columns'
//                           items in LDS (4 KiB); then every lane walks the same column at the same time, so each LDS read is one
//                           address for the whole wavefront, a broadcast.  A lane ends with three masks of the word (dimer, size,
//                           near), stores their OR as the matrix word with a plain vector store -- every word has one owner, there
//                           are no atomics on the matrix -- and adds their popcounts to its four sums, which go to counts[] by one
//                           vector atomic add each at the end of the chunk (several chunks add to one row).
//                           The bits that must be zero are zero by construction: the diagonal and a column without a pair are
//                           skipped, a column at or beyond n is staged as an item without a pair, and a row without a pair
//                           skips the walk.
//                           A wavefront per block, not four: at n = 4096 that is 64 x 64 blocks, 16 wavefronts a CU, where blocks
//                           of 256 rows would leave three SIMDs of four idle.  The columns staged again by every wavefront are 4 KiB
//                           per 16,384 duplexes.
//   panel_keys_kernel       ~conflicts << 32 | index, all ones without a pair; rocPRIM sorts them ascending
//   panel_first_fit_kernel  ONE workgroup of 1024 lanes, so that the matrix never crosses PCIe.  For each pair of the order:
//                           the lanes walk its row's words and set forbidden[pool_of[j]] (LDS OR) for every set bit j that has
//                           a pool; barrier; the lanes look for the lowest pool that is neither forbidden nor full below the
//                           pools in use (LDS minimum; the next unused pool always fits) and clear the words they looked at;
//                           barrier; lane 0 records the choice; barrier.  n dependent steps of three barriers: no spinning,
//                           nothing between workgroups.  pool_of and the pools' member counts are global memory, written by lane
//                           0 and read by the workgroup's other lanes behind a barrier (one CU, one L1); forbidden and full are
//                           2 x 8 KiB of LDS, a bit per pool, and the order comes through LDS 1024 keys at a time.
// Bounds: a row index is below n wherever it indexes; a matrix word is below n words; a column index from a set bit is below n
// because the bits at and beyond n are zero, and is checked again before pool_of is read; a pool is below the pools in use, which
// are at most the pairs placed so far, so its bit lies in the 2048 words.
#include <cstring>

#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>

#include "primer_shortlist.h"

namespace rb {

namespace {

constexpr int ITEM_THREADS = 256;
constexpr int FIT_THREADS = 1024;
constexpr int POOL_WORDS = RIBBIT_PANEL_MAX_PAIRS / 32;
static_assert(PANEL_TILE == 64, "a tile is a wavefront's lanes and a matrix word's bits");
static_assert(sizeof(RibbitPanelRow) == 32 && sizeof(RibbitPanelParams) == 20, "8 and 5 ints");

__global__ __launch_bounds__(ITEM_THREADS) void panel_items_kernel(const RibbitRowPrimerPair *__restrict__ pairs, const int32_t *__restrict__ extra, int64_t n,
                                                                    PanelItem *__restrict__ items) {
    for (int64_t i = (int64_t)blockIdx.x * ITEM_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * ITEM_THREADS) {
        const RibbitRowPrimerPair &p = pairs[i];
        PanelItem it{};
        if (p.left.start >= 0) {
            it.kl = p.left.length;
            it.kr = p.right.length;
            it.l = bases_of(p.left) & low_bases(it.kl);
            it.r = reverse_complement(bases_of(p.right) & low_bases(it.kr), it.kr);
            it.rl = reversed(it.l, it.kl);
            it.rr = reversed(it.r, it.kr);
            it.start = p.left.start;
            it.end = (int64_t)p.right.start + p.right.length;
            it.group = extra ? extra[3 * i] : -1;
            it.size_lo = extra ? extra[3 * i + 1] : p.product;
            it.size_hi = extra ? extra[3 * i + 2] : p.product;
        }
        items[i] = it;
    }
}

// any(a, b) > max_cross_any or end(a, b) > max_cross_end for one of the four combinations of a row's and a column's oligos
__device__ inline bool dimer_of(const PanelItem &me, const PanelItem &o, int any_n, int max_end) {
    return !duplex_within_reversed(me.l, me.kl, o.rl, o.kl, any_n, max_end) || !duplex_within_reversed(me.l, me.kl, o.rr, o.kr, any_n, max_end) ||
           !duplex_within_reversed(me.r, me.kr, o.rl, o.kl, any_n, max_end) || !duplex_within_reversed(me.r, me.kr, o.rr, o.kr, any_n, max_end);
}

__global__ __launch_bounds__(PANEL_TILE) void panel_conflicts_kernel(const PanelItem *__restrict__ items, int64_t n, int64_t words, const RibbitPanelParams prm,
                                                                      unsigned long long *__restrict__ matrix, int32_t *__restrict__ counts) {
    __shared__ PanelItem tile[PANEL_TILE];
    const int lane = threadIdx.x;
    const int64_t i = (int64_t)blockIdx.x * PANEL_TILE + lane;
    const bool row = i < n;
    const PanelItem me = row ? items[i] : PanelItem{};
    const bool has = me.kl > 0;
    const int64_t first = words * blockIdx.y / gridDim.y, last = words * (blockIdx.y + 1) / gridDim.y;
    const int any_n = prm.max_cross_any + 1, max_end = prm.max_cross_end;
    const int64_t gap = prm.size_gap, hull_max = prm.max_cross_product;
    int32_t sum_any = 0, sum_dimer = 0, sum_size = 0, sum_near = 0;
    for (int64_t w = first; w < last; ++w) {
        const int64_t column = w * PANEL_TILE + lane;
        __syncthreads();      // (the last word's walk is over)
        tile[lane] = column < n ? items[column] : PanelItem{};
        __syncthreads();
        unsigned long long dimer = 0, size = 0, near = 0;
        if (has) {
            for (int c = 0; c < PANEL_TILE; ++c) {
                const PanelItem &o = tile[c];
                if (o.kl == 0 || w * PANEL_TILE + c == i) continue;
                const unsigned long long bit = 1ull << c;
                if (dimer_of(me, o, any_n, max_end)) dimer |= bit;
                if (gap > 0 && (int64_t)me.size_lo - o.size_hi < gap && (int64_t)o.size_lo - me.size_hi < gap) size |= bit;
                if (hull_max > 0 && me.group >= 0 && me.group == o.group && max(me.end, o.end) - min((int64_t)me.start, (int64_t)o.start) <= hull_max) near |= bit;
            }
        }
        if (row) matrix[i * words + w] = dimer | size | near;
        sum_any += __popcll(dimer | size | near);
        sum_dimer += __popcll(dimer);
        sum_size += __popcll(size);
        sum_near += __popcll(near);
    }
    if (sum_any) {      // (only a row that has a pair)
        atomicAdd(&counts[4 * i], sum_any);
        if (sum_dimer) atomicAdd(&counts[4 * i + 1], sum_dimer);
        if (sum_size) atomicAdd(&counts[4 * i + 2], sum_size);
        if (sum_near) atomicAdd(&counts[4 * i + 3], sum_near);
    }
}

__global__ __launch_bounds__(ITEM_THREADS) void panel_keys_kernel(const PanelItem *__restrict__ items, const int32_t *__restrict__ counts, int64_t n,
                                                                   unsigned long long *__restrict__ keys) {
    for (int64_t i = (int64_t)blockIdx.x * ITEM_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * ITEM_THREADS)
        keys[i] = items[i].kl > 0 ? (unsigned long long)(~(uint32_t)counts[4 * i]) << 32 | (unsigned long long)i : NO_KEY;
}

__global__ __launch_bounds__(FIT_THREADS) void panel_first_fit_kernel(const unsigned long long *__restrict__ sorted, const unsigned long long *__restrict__ matrix,
                                                                       const int32_t *__restrict__ counts, int64_t n, int64_t words, int32_t pool_size, int32_t *pool_of,
                                                                       int32_t *members, PanelHeader *__restrict__ header, RibbitPanelRow *__restrict__ rows) {
    __shared__ uint32_t forbidden[POOL_WORDS], full[POOL_WORDS];
    __shared__ unsigned long long order[FIT_THREADS];
    __shared__ int32_t chosen, in_use, placed;
    const int t = threadIdx.x;
    for (int w = t; w < POOL_WORDS; w += FIT_THREADS) forbidden[w] = full[w] = 0u;
    for (int64_t i = t; i < n; i += FIT_THREADS) {
        pool_of[i] = -1;
        members[i] = 0;
    }
    if (t == 0) in_use = placed = 0;
    __syncthreads();
    for (int64_t step = 0; step < n; ++step) {
        const int at = (int)(step % FIT_THREADS);
        if (at == 0) {      // (the barrier behind the last step lies between the last read of order[] and this write)
            order[t] = step + t < n ? sorted[step + t] : NO_KEY;
            __syncthreads();
        }
        const unsigned long long key = order[at];
        if (key == NO_KEY) break;      // (the same in every lane: the rows without a pair sort last)
        const int64_t i = (int64_t)(key & 0xffffffffull);
        const int32_t used = in_use;
        if (t == 0) chosen = used;      // (the next unused pool always fits)
        for (int64_t w = t; w < words; w += FIT_THREADS) {
            unsigned long long bits = matrix[i * words + w];
            while (bits) {
                const int64_t j = w * PANEL_TILE + __builtin_ctzll(bits);
                bits &= bits - 1ull;
                const int32_t p = j < n ? pool_of[j] : -1;
                if (p >= 0 && p < used) atomicOr(&forbidden[p >> 5], 1u << (p & 31));
            }
        }
        __syncthreads();
        // the lowest pool below `used` that is neither forbidden nor full; the words looked at are cleared for the next step
        for (int w = t; 32 * w < used; w += FIT_THREADS) {
            const uint32_t open = ~(forbidden[w] | full[w]);
            forbidden[w] = 0u;
            if (open) {
                const int32_t p = 32 * w + __ffs(open) - 1;
                if (p < used) atomicMin(&chosen, p);
            }
        }
        __syncthreads();
        if (t == 0) {
            const int32_t p = chosen;
            pool_of[i] = p;
            if (++members[p] >= pool_size) full[p >> 5] |= 1u << (p & 31);
            if (p == used) in_use = used + 1;
            ++placed;
        }
        __syncthreads();
    }
    __syncthreads();
    for (int64_t i = t; i < n; i += FIT_THREADS) {
        RibbitPanelRow r{};
        r.pool = pool_of[i];
        r.conflicts = counts[4 * i];
        r.dimer = counts[4 * i + 1];
        r.size = counts[4 * i + 2];
        r.near = counts[4 * i + 3];
        rows[i] = r;
    }
    if (t == 0) *header = PanelHeader{in_use, placed};
}

hipError_t sort_keys(void *scratch, size_t &bytes, const unsigned long long *keys, unsigned long long *sorted, int64_t n, hipStream_t stream) {
    return rocprim::radix_sort_keys(scratch, bytes, keys, sorted, (size_t)n, 0u, 64u, stream);
}

}  // namespace

PanelLayout panel_layout(int64_t n) {
    const size_t rows = (size_t)n;
    size_t sort_bytes = 0;
    (void)sort_keys(nullptr, sort_bytes, nullptr, nullptr, n, 0);
    PanelLayout at{};
    WorkCarver w;
    at.items = w.take(rows * sizeof(PanelItem));
    at.matrix = w.take(rows * (size_t)panel_words(n) * sizeof(unsigned long long));
    at.counts = w.take(4 * rows * sizeof(int32_t));
    at.keys = w.take(2 * rows * sizeof(unsigned long long));
    at.pool_of = w.take(2 * rows * sizeof(int32_t));
    at.header = w.take(sizeof(PanelHeader));
    at.rows = w.take(rows * sizeof(RibbitPanelRow));
    w.close(at, sort_bytes);
    return at;
}

hipError_t launch_panel_conflicts(const RibbitRowPrimerPair *pairs, const int32_t *extra, int64_t n, const RibbitPanelParams &prm, uint8_t *work, size_t work_bytes,
                                  const PanelLayout &at, hipStream_t stream) {
    if (work_bytes < at.bytes || n < 1 || n > RIBBIT_PANEL_MAX_PAIRS) return hipErrorInvalidValue;
    PanelItem *items = region<PanelItem>(work, at.items);
    int32_t *counts = region<int32_t>(work, at.counts);
    const hipError_t e = hipMemsetAsync(counts, 0, 4 * (size_t)n * sizeof(int32_t), stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(panel_items_kernel, dim3((unsigned)((n + ITEM_THREADS - 1) / ITEM_THREADS)), dim3(ITEM_THREADS), 0, stream, pairs, extra, n, items);
    const int64_t words = panel_words(n);
    hipLaunchKernelGGL(panel_conflicts_kernel, dim3((unsigned)words, (unsigned)panel_chunks(n)), dim3(PANEL_TILE), 0, stream, items, n, words, prm,
                       region<unsigned long long>(work, at.matrix), counts);
    return hipGetLastError();
}

hipError_t launch_panel_order(int64_t n, uint8_t *work, size_t work_bytes, const PanelLayout &at, hipStream_t stream) {
    if (work_bytes < at.bytes || n < 1 || n > RIBBIT_PANEL_MAX_PAIRS) return hipErrorInvalidValue;
    unsigned long long *keys = region<unsigned long long>(work, at.keys);
    hipLaunchKernelGGL(panel_keys_kernel, dim3((unsigned)((n + ITEM_THREADS - 1) / ITEM_THREADS)), dim3(ITEM_THREADS), 0, stream, region<PanelItem>(work, at.items),
                       region<int32_t>(work, at.counts), n, keys);
    size_t bytes = at.scratch_bytes;
    const hipError_t e = sort_keys(work + at.scratch, bytes, keys, keys + n, n, stream);
    return e != hipSuccess ? e : hipGetLastError();
}

hipError_t launch_panel_first_fit(int64_t n, const RibbitPanelParams &prm, uint8_t *work, size_t work_bytes, const PanelLayout &at, hipStream_t stream) {
    if (work_bytes < at.bytes || n < 1 || n > RIBBIT_PANEL_MAX_PAIRS) return hipErrorInvalidValue;
    int32_t *pool_of = region<int32_t>(work, at.pool_of);
    hipLaunchKernelGGL(panel_first_fit_kernel, dim3(1), dim3(FIT_THREADS), 0, stream, region<unsigned long long>(work, at.keys) + n,
                       region<unsigned long long>(work, at.matrix), region<int32_t>(work, at.counts), n, panel_words(n), prm.pool_size, pool_of, pool_of + n,
                       region<PanelHeader>(work, at.header), region<RibbitPanelRow>(work, at.rows));
    return hipGetLastError();
}

}  // namespace rb
