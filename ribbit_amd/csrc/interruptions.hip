// interruptions.hip -- every row's CIGAR decoded into interruptions and the pure stretch (api_interruptions.cpp:
// ribbit_hip_record_interruptions), as include/ribbit_hip.h states it.  The CIGARs are short and skewed (25 bytes on average, a
// few rows with thousands of ops), so nothing here is a loop per row: the ops of all rows are one array, every sum a row or an
// interruption needs is the difference of two prefix sums over that array, and the one thing that is no sum, the longest stretch
// of a row, is a segmented max-scan.  No lane's work grows with the number of ops of its row.  On the handle's stream:
//   count:    one lane per 16 aligned bytes of the pool, with the 16 before them (an op's digits may start in those): a forward
//             walk over the 27 bytes in registers that keeps the value and the number of the digits seen since the last letter.
//             The lane counts the op letters of its own 16 bytes and checks the grammar there: a byte outside 0-9=MXID, a letter
//             without digits, with more than ten or with a value outside 1 .. 2^31 - 1 records its offset with an atomicMin
//   scan:     an exclusive rocPRIM sum-scan of the lanes' counts, in place: where each lane's ops go, and the number of ops
//   emit:     the same walk again; a letter writes its op: pool offset << 33 | kind << 31 | length
//   rows:     one lane per row (and one more): the ops before offsets[i] = its lane's prefix + the letters of that lane before the
//             byte, which is the row's first op; a non-empty row marks that op with i + 1 (its head) and checks that its last
//             byte is a letter (digits at a row's end: atomicMin of the row's end)
//   sums:     an inclusive rocPRIM scan over the ops of (match, x, ins, del, run heads, interruption heads, last row head): a run
//             is a maximal stretch of ops of one row that are all matches or all not, its head the op that differs in that from
//             the one before it or is a row's head.  64-bit sums: they run over all rows
//   heads:    one lane per op: a run's head writes its op index at the run's number; the last op writes the counts
//   runs:     one lane per run: its ops are [head, next run's head), its row the last row head's, its offsets and sums
//             differences of prefixes.  A run of non-matches is an interruption and writes its record, its clipped width and where
//             its observed bases start; a run of matches writes its key (length << 32 | ~start: the longest wins, the leftmost
//             among equals)
//   best:     an inclusive rocPRIM max-scan of the keys, restarted at every row's first run (the segmented scan's operator)
//   offsets:  an exclusive rocPRIM sum-scan of the widths, 64-bit; one lane per interruption narrows the offsets to int32, one
//             writes the total
//   finish:   one lane per row: its totals are differences of prefixes at its first op and at the next row's, its pure stretch
//             the best key at its last run; sums that do not fit record the row with an atomicMin
// The host reads the totals here (one synchronise), refuses what they report and sizes the observed text; then
//   spans:    one lane per 4096 observed bytes: the interruption that holds the span's first byte (bisection)
//   gather:   one workgroup per span, 16 output bytes per lane: the lane bisects for its first byte's interruption between its
//             span's and the next span's, then moves on to the next one when a byte lies behind the current one's end (the one
//             after it, or a bisection again when that one is empty too); one aligned 16-byte store
// The scans run over interruptions_op_cap(P) elements, the most ops a pool of P bytes can have, and read the true counts from
// device memory: elements behind the count are the scan's identity.  3 memsets, 7 kernels and 4 rocPRIM scans before the
// synchronise, 2 kernels after it.
#include <cstring>

#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>

#include "row_kernels.h"

namespace rb {

namespace {

constexpr uint32_t NONE = 0xffffffffu;
constexpr uint32_t MAX_LEN = 0x7fffffffu;
enum : uint32_t { MATCH = 0, SUBST = 1, INS = 2, DEL = 3, DIGIT = 4, OTHER = 5 };
static_assert(sizeof(InterruptionTotals) == 32 && sizeof(InterruptionSums) == 48 && sizeof(InterruptionBest) == 16, "as InterruptionLayout says");
static_assert(sizeof(RibbitInterruption) == 32 && sizeof(RibbitRowPurity) == 32, "as include/ribbit_hip.h says");

__device__ __forceinline__ uint32_t kind_of_byte(uint32_t c) {
    return c - '0' < 10u ? DIGIT : (c == '=' || c == 'M') ? MATCH : c == 'X' ? SUBST : c == 'I' ? INS : c == 'D' ? DEL : OTHER;
}
__device__ __forceinline__ uint32_t op_kind(uint64_t op) { return (uint32_t)(op >> 31) & 3u; }
__device__ __forceinline__ uint32_t op_len(uint64_t op) { return (uint32_t)op & MAX_LEN; }
__device__ __forceinline__ uint32_t op_at(uint64_t op) { return (uint32_t)(op >> 33); }

// Lane c's walk over pool bytes [16 c - 11, 16 c + 16).  EMIT false: -> the op letters of [16 c, 16 c + 16), the grammar checked;
// EMIT true: those ops written from ops[base] on.
// (a pool of good grammar has at most `cap` ops; one of bad grammar may have more letters, which are not written)
template <bool EMIT>
__device__ __forceinline__ uint32_t walk_chunk(const uint4 *__restrict__ pool, int64_t c, int64_t pool_bytes, uint64_t *__restrict__ ops, uint32_t base,
                                               uint32_t cap, uint32_t *__restrict__ bad_at) {
    const uint4 before = c ? pool[c - 1] : make_uint4(0, 0, 0, 0), own = pool[c];
    const uint32_t w[8] = {before.x, before.y, before.z, before.w, own.x, own.y, own.z, own.w};
    uint64_t value = 0;
    uint32_t digits = 0, found = 0, bad = NONE;
#pragma unroll
    for (int t = 5; t < 32; ++t) {
        const uint32_t byte = (w[t >> 2] >> (8 * (t & 3))) & 0xffu, kind = kind_of_byte(byte);
        const int64_t p = 16 * c - 16 + t;
        const bool mine = t >= 16 && p < pool_bytes;
        if (kind == DIGIT) {
            value = digits < 10 ? value * 10 + (byte - '0') : (uint64_t)MAX_LEN + 1;      // (an eleventh digit: the count decides below)
            digits = min(digits + 1, 11u);
        } else {
            if (mine) {
                if (kind == OTHER) {
                    bad = min(bad, (uint32_t)p);
                } else {
                    if (digits < 1 || digits > 10 || value < 1 || value > MAX_LEN) bad = min(bad, (uint32_t)p);
                    if (EMIT && base + found < cap) ops[base + found] = (uint64_t)p << 33 | (uint64_t)kind << 31 | (uint64_t)min(value, (uint64_t)MAX_LEN);
                    ++found;
                }
            }
            value = 0;
            digits = 0;
        }
    }
    if (!EMIT && bad != NONE) atomicMin(bad_at, bad);
    return found;
}

__global__ void __launch_bounds__(ROW_THREADS) int_count_kernel(const uint4 *__restrict__ pool, int64_t chunks, int64_t pool_bytes, uint32_t *__restrict__ counts,
                                                                InterruptionTotals *__restrict__ totals) {
    for (int64_t c = (int64_t)blockIdx.x * ROW_THREADS + threadIdx.x; c <= chunks; c += (int64_t)gridDim.x * ROW_THREADS)
        counts[c] = c < chunks ? walk_chunk<false>(pool, c, pool_bytes, nullptr, 0, 0, &totals->bad_at) : 0u;
}

__global__ void __launch_bounds__(ROW_THREADS) int_emit_kernel(const uint4 *__restrict__ pool, int64_t chunks, int64_t pool_bytes, const uint32_t *__restrict__ prefix,
                                                               uint64_t *__restrict__ ops, uint32_t cap) {
    for (int64_t c = (int64_t)blockIdx.x * ROW_THREADS + threadIdx.x; c < chunks; c += (int64_t)gridDim.x * ROW_THREADS)
        (void)walk_chunk<true>(pool, c, pool_bytes, ops, prefix[c], cap, nullptr);
}

// first_op[i] = the ops before byte offsets[i], i = 0 .. n; a non-empty row's first op gets the row's head mark
__global__ void __launch_bounds__(ROW_THREADS) int_row_heads_kernel(const uint8_t *__restrict__ pool, const int32_t *__restrict__ offsets, int64_t n, int64_t pool_bytes,
                                                                    const uint32_t *__restrict__ prefix, uint32_t *__restrict__ first_op, uint32_t *__restrict__ op_row,
                                                                    uint32_t cap, InterruptionTotals *__restrict__ totals) {
    const uint32_t ops = min(prefix[(pool_bytes + 15) / 16], cap);
    for (int64_t i = (int64_t)blockIdx.x * ROW_THREADS + threadIdx.x; i <= n; i += (int64_t)gridDim.x * ROW_THREADS) {
        const int64_t at = min(max((int64_t)offsets[i], (int64_t)0), pool_bytes);      // (the host has checked: 0 .. pool_bytes, ascending)
        const uint4 chunk = reinterpret_cast<const uint4 *>(pool)[at >> 4];              // (a zero chunk follows the pool's last)
        const uint32_t w[4] = {chunk.x, chunk.y, chunk.z, chunk.w};
        uint32_t first = prefix[at >> 4];
#pragma unroll
        for (int t = 0; t < 16; ++t)
            first += t < (int)(at & 15) && kind_of_byte((w[t >> 2] >> (8 * (t & 3))) & 0xffu) < DIGIT;
        first = min(first, ops);
        first_op[i] = first;
        if (i == n) { totals->ops = ops; continue; }
        const int64_t end = min(max((int64_t)offsets[i + 1], at), pool_bytes);
        if (end == at) continue;
        if (kind_of_byte(pool[end - 1]) >= DIGIT) atomicMin(&totals->bad_at, (uint32_t)end);      // (a byte that is no digit either has recorded itself)
        if (first < ops) op_row[first] = (uint32_t)i + 1;
    }
}

// whether op j heads a run, and whether that run is an interruption
__device__ __forceinline__ void heads_of_op(const uint64_t *__restrict__ ops, const uint32_t *__restrict__ op_row, int64_t j, bool *run, bool *site) {
    const bool match = op_kind(ops[j]) == MATCH;
    *run = op_row[j] != 0 || j == 0 || (op_kind(ops[j - 1]) == MATCH) != match;
    *site = *run && !match;
}

struct SumsOfOp {
    const uint64_t *ops;
    const uint32_t *op_row;
    const InterruptionTotals *totals;
    __host__ __device__ InterruptionSums operator()(int64_t j) const {
        if (j >= (int64_t)totals->ops) return InterruptionSums{0, 0, 0, 0, 0, 0, 0, 0};
        const uint64_t op = ops[j];
        const uint32_t kind = op_kind(op);
        const unsigned long long len = op_len(op);
        bool run, site;
        heads_of_op(ops, op_row, j, &run, &site);
        return InterruptionSums{kind == MATCH ? len : 0, kind == SUBST ? len : 0, kind == INS ? len : 0, kind == DEL ? len : 0, run ? 1u : 0u, site ? 1u : 0u, op_row[j], 0};
    }
};

struct AddInterruptionSums {
    __host__ __device__ InterruptionSums operator()(const InterruptionSums &a, const InterruptionSums &b) const {
        return InterruptionSums{a.match + b.match, a.x + b.x, a.ins + b.ins, a.del + b.del, a.runs + b.runs, a.sites + b.sites, a.row > b.row ? a.row : b.row, 0};
    }
};

__device__ __forceinline__ InterruptionSums sums_before(const InterruptionSums *__restrict__ sums, int64_t j) {
    return j > 0 ? sums[j - 1] : InterruptionSums{0, 0, 0, 0, 0, 0, 0, 0};
}
__device__ __forceinline__ unsigned long long query_of(const InterruptionSums &s) { return s.match + s.x + s.ins; }

__global__ void __launch_bounds__(ROW_THREADS) int_run_heads_kernel(const uint64_t *__restrict__ ops, const uint32_t *__restrict__ op_row,
                                                                    const InterruptionSums *__restrict__ sums, uint32_t *__restrict__ run_head,
                                                                    InterruptionTotals *__restrict__ totals) {
    const int64_t count = totals->ops;
    for (int64_t j = (int64_t)blockIdx.x * ROW_THREADS + threadIdx.x; j < count; j += (int64_t)gridDim.x * ROW_THREADS) {
        bool run, site;
        heads_of_op(ops, op_row, j, &run, &site);
        const InterruptionSums s = sums[j];
        if (run) run_head[s.runs - 1] = (uint32_t)j;       // (s.runs >= 1: op 0 heads a run)
        if (j == count - 1) {
            run_head[s.runs] = (uint32_t)count;
            totals->runs = s.runs;
            totals->sites = s.sites;
        }
    }
}

__device__ __forceinline__ int32_t clamp_int32(long long v) { return (int32_t)min(max(v, (long long)INT32_MIN), (long long)INT32_MAX); }

__global__ void __launch_bounds__(ROW_THREADS) int_runs_kernel(const int32_t *__restrict__ iv, const int32_t *__restrict__ offsets, int64_t n, int64_t length,
                                                               const uint64_t *__restrict__ ops, const uint32_t *__restrict__ op_row,
                                                               const uint32_t *__restrict__ first_op, const InterruptionSums *__restrict__ sums,
                                                               const uint32_t *__restrict__ run_head, const InterruptionTotals *__restrict__ totals,
                                                               InterruptionBest *__restrict__ best, RibbitInterruption *__restrict__ sites,
                                                               uint32_t *__restrict__ width, int32_t *__restrict__ source) {
    const int64_t count = totals->runs, n_ops = totals->ops;
    for (int64_t r = (int64_t)blockIdx.x * ROW_THREADS + threadIdx.x; r < count; r += (int64_t)gridDim.x * ROW_THREADS) {
        // (on a pool whose grammar is bad the indices below are still indices: the host refuses the result)
        const int64_t head = min((int64_t)run_head[r], n_ops - 1), next = min(max((int64_t)run_head[r + 1], head + 1), n_ops);
        const InterruptionSums from = sums_before(sums, head), to = sums[next - 1];
        const int64_t row = min(max((int64_t)to.row - 1, (int64_t)0), n - 1);
        const InterruptionSums base = sums_before(sums, min((int64_t)first_op[row], head));
        const long long s = iv[2 * row];
        const unsigned long long q_from = query_of(from) - query_of(base), q_to = query_of(to) - query_of(base);
        const bool first_of_row = op_row[head] != 0;
        if (op_kind(ops[head]) == MATCH) {
            const unsigned long long len = min(to.match - from.match, (unsigned long long)MAX_LEN);
            best[r] = InterruptionBest{len << 32 | (unsigned long long)(NONE - (uint32_t)min(q_from, (unsigned long long)MAX_LEN)), first_of_row ? 1u : 0u, 0};
            continue;
        }
        best[r] = InterruptionBest{0, first_of_row ? 1u : 0u, 0};
        const int64_t id = (int64_t)to.sites - 1;      // (the run's head is the last interruption head up to its last op)
        if (id < 0 || id >= (int64_t)totals->sites) continue;
        const long long start = s + (long long)q_from, end = s + (long long)q_to;
        const uint32_t cigar_at = first_of_row ? (uint32_t)offsets[row] : head > 0 ? op_at(ops[head - 1]) + 1 : 0u;
        sites[id] = RibbitInterruption{(int32_t)row, clamp_int32(start), clamp_int32(end), (int32_t)min(to.x - from.x, (unsigned long long)MAX_LEN),
                                       (int32_t)min(to.ins - from.ins, (unsigned long long)MAX_LEN), (int32_t)min(to.del - from.del, (unsigned long long)MAX_LEN),
                                       (int32_t)cigar_at, (int32_t)(op_at(ops[next - 1]) + 1 - cigar_at)};
        const long long a = min(max(start, 0ll), (long long)length), b = min(max(end, a), (long long)length);
        width[id] = (uint32_t)(b - a);
        source[id] = (int32_t)a;
    }
}

struct BestOfRun {
    const InterruptionBest *best;
    const InterruptionTotals *totals;
    __host__ __device__ InterruptionBest operator()(int64_t r) const { return r < (int64_t)totals->runs ? best[r] : InterruptionBest{0, 1, 0}; }
};
// the segmented scan's operator: a run that is its row's first takes nothing from the runs before it
struct MaxWithinRow {
    __host__ __device__ InterruptionBest operator()(const InterruptionBest &a, const InterruptionBest &b) const {
        return b.head ? b : InterruptionBest{a.key > b.key ? a.key : b.key, a.head, 0};
    }
};

struct WidthOfSite {
    const uint32_t *width;
    const InterruptionTotals *totals;
    __host__ __device__ unsigned long long operator()(int64_t id) const { return id < (int64_t)totals->sites ? width[id] : 0ull; }
};

__global__ void __launch_bounds__(ROW_THREADS) int_offsets_kernel(const unsigned long long *__restrict__ offsets64, int32_t *__restrict__ offsets32,
                                                                  InterruptionTotals *__restrict__ totals) {
    const int64_t count = totals->sites;
    for (int64_t id = (int64_t)blockIdx.x * ROW_THREADS + threadIdx.x; id <= count; id += (int64_t)gridDim.x * ROW_THREADS) {
        offsets32[id] = (int32_t)min(offsets64[id], (unsigned long long)INT32_MAX);      // (more than INT32_MAX: the host refuses the total)
        if (id == count) totals->observed = offsets64[id];
    }
}

__global__ void __launch_bounds__(ROW_THREADS) int_finish_kernel(const int32_t *__restrict__ iv, int64_t n, const uint32_t *__restrict__ first_op,
                                                                 const InterruptionSums *__restrict__ sums, const InterruptionBest *__restrict__ best,
                                                                 RibbitRowPurity *__restrict__ rows, InterruptionTotals *__restrict__ totals) {
    for (int64_t i = (int64_t)blockIdx.x * ROW_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * ROW_THREADS) {
        const int64_t f = first_op[i], l = max((int64_t)first_op[i + 1], f);
        const InterruptionSums base = sums_before(sums, f), to = sums_before(sums, l);
        const long long s = iv[2 * i];
        const unsigned long long query = query_of(to) - query_of(base), del = to.del - base.del;
        if (query + del > (unsigned long long)INT32_MAX || s + (long long)query > (long long)INT32_MAX) atomicMin(&totals->bad_row, (uint32_t)i);
        int32_t pure_start = (int32_t)s, pure_end = (int32_t)s;
        if (l > f && to.runs > 0) {
            const unsigned long long key = best[to.runs - 1].key;
            if (key) {
                pure_start = clamp_int32(s + (long long)(NONE - (uint32_t)key));
                pure_end = clamp_int32(s + (long long)(NONE - (uint32_t)key) + (long long)(key >> 32));
            }
        }
        rows[i] = RibbitRowPurity{(int32_t)base.sites, (int32_t)(to.sites - base.sites), (int32_t)min(to.x - base.x, (unsigned long long)MAX_LEN),
                                  (int32_t)min(to.ins - base.ins, (unsigned long long)MAX_LEN), (int32_t)min(del, (unsigned long long)MAX_LEN),
                                  (int32_t)min(query, (unsigned long long)MAX_LEN), pure_start, pure_end};
    }
}

// the last id in [lo, hi] whose observed bases start at or before `byte` (offsets ascend; offsets[lo] <= byte)
__device__ __forceinline__ int32_t site_of_byte(const int32_t *__restrict__ offsets, int32_t lo, int32_t hi, int32_t byte) {
    while (lo < hi) {
        const int32_t mid = lo + (hi - lo + 1) / 2;
        if (offsets[mid] <= byte) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// span_site[b] = the interruption that holds observed byte b * SPAN (the last byte for b = spans)
__global__ void __launch_bounds__(ROW_THREADS) int_spans_kernel(const int32_t *__restrict__ offsets, int32_t sites, int64_t total, int64_t spans,
                                                                int32_t *__restrict__ span_site) {
    const int64_t b = (int64_t)blockIdx.x * ROW_THREADS + threadIdx.x;
    if (b > spans) return;
    span_site[b] = site_of_byte(offsets, 0, sites - 1, (int32_t)min(b * INTERRUPTION_SPAN, total - 1));
}

__global__ void __launch_bounds__(ROW_THREADS) int_gather_kernel(const uint8_t *__restrict__ ascii, const int32_t *__restrict__ offsets, const int32_t *__restrict__ source,
                                                                 const int32_t *__restrict__ span_site, int32_t sites, int64_t total, uint4 *__restrict__ out) {
    static_assert(INTERRUPTION_SPAN == 16 * ROW_THREADS, "a workgroup gathers one span, 16 bytes per lane");
    const int64_t spans = (total + INTERRUPTION_SPAN - 1) / INTERRUPTION_SPAN;
    for (int64_t b = blockIdx.x; b < spans; b += gridDim.x) {
        const int64_t o = b * INTERRUPTION_SPAN + 16 * (int64_t)threadIdx.x;
        if (o >= total) continue;
        const int32_t last = span_site[b + 1];
        int32_t id = site_of_byte(offsets, span_site[b], last, (int32_t)o);
        int32_t from = offsets[id], to = offsets[id + 1], src = source[id];
        uint64_t w[2] = {0, 0};      // (the loop holds a bisection and is not unrolled: the bytes go into one of two registers)
        for (int t = 0; t < 16; ++t) {
            const int32_t byte = (int32_t)o + t;
            if (byte >= total) break;
            if (byte >= to) {      // the next interruption with bases: the one behind this one, or found by bisection when that one has none
                id = byte < offsets[id + 2] ? id + 1 : site_of_byte(offsets, id + 2, last, byte);
                from = offsets[id]; to = offsets[id + 1]; src = source[id];
            }
            const uint64_t base = (uint64_t)ascii[src + (byte - from)] << (8 * (t & 7));
            if (t < 8) w[0] |= base; else w[1] |= base;
        }
        out[o >> 4] = make_uint4((uint32_t)w[0], (uint32_t)(w[0] >> 32), (uint32_t)w[1], (uint32_t)(w[1] >> 32));
    }
}

hipError_t scan_counts(void *scratch, size_t &bytes, uint32_t *counts, size_t n, hipStream_t stream) {
    return rocprim::exclusive_scan(scratch, bytes, counts, counts, 0u, n, rocprim::plus<uint32_t>(), stream);
}
hipError_t scan_sums(void *scratch, size_t &bytes, const uint64_t *ops, const uint32_t *op_row, const InterruptionTotals *totals, InterruptionSums *sums, size_t cap,
                     hipStream_t stream) {
    return rocprim::inclusive_scan(scratch, bytes, rocprim::make_transform_iterator(rocprim::make_counting_iterator<int64_t>(0), SumsOfOp{ops, op_row, totals}), sums,
                                   cap, AddInterruptionSums(), stream);
}
hipError_t scan_best(void *scratch, size_t &bytes, const InterruptionBest *in, const InterruptionTotals *totals, InterruptionBest *out, size_t cap, hipStream_t stream) {
    return rocprim::inclusive_scan(scratch, bytes, rocprim::make_transform_iterator(rocprim::make_counting_iterator<int64_t>(0), BestOfRun{in, totals}), out, cap,
                                   MaxWithinRow(), stream);
}
hipError_t scan_widths(void *scratch, size_t &bytes, const uint32_t *width, const InterruptionTotals *totals, unsigned long long *offsets64, size_t cap,
                       hipStream_t stream) {
    return rocprim::exclusive_scan(scratch, bytes, rocprim::make_transform_iterator(rocprim::make_counting_iterator<int64_t>(0), WidthOfSite{width, totals}), offsets64,
                                   0ull, cap, rocprim::plus<unsigned long long>(), stream);
}

}  // namespace

InterruptionLayout interruptions_layout(int64_t n, size_t pool_bytes) {
    const size_t cap = interruptions_op_cap(pool_bytes), chunks = (pool_bytes + 15) / 16;
    size_t a = 0, b = 0, c = 0, d = 0;
    (void)scan_counts(nullptr, a, nullptr, chunks + 1, 0);
    (void)scan_sums(nullptr, b, nullptr, nullptr, nullptr, nullptr, cap, 0);
    (void)scan_best(nullptr, c, nullptr, nullptr, nullptr, cap, 0);
    (void)scan_widths(nullptr, d, nullptr, nullptr, nullptr, cap + 1, 0);
    InterruptionLayout at{};
    WorkCarver w;
    at.counts = w.take((chunks + 1) * sizeof(uint32_t));
    at.ops = w.take(cap * sizeof(uint64_t));
    at.op_row = w.take(cap * sizeof(uint32_t));
    at.first_op = w.take(((size_t)n + 1) * sizeof(uint32_t));
    at.sums = w.take(cap * sizeof(InterruptionSums));
    at.run_head = w.take((cap + 1) * sizeof(uint32_t));
    at.best = w.take(2 * cap * sizeof(InterruptionBest));
    at.width = w.take((cap + 1) * sizeof(uint32_t));
    at.source = w.take(cap * sizeof(int32_t));
    at.offsets64 = w.take((cap + 1) * sizeof(unsigned long long));
    at.spans = w.take(((size_t)INT32_MAX / INTERRUPTION_SPAN + 3) * sizeof(int32_t));      // (the observed bytes are at most INT32_MAX)
    at.rows = w.take((size_t)n * sizeof(RibbitRowPurity));
    at.sites = w.take(cap * sizeof(RibbitInterruption));
    at.offsets32 = w.take((cap + 1) * sizeof(int32_t));
    at.totals = w.take(sizeof(InterruptionTotals));
    w.close(at, std::max(std::max(a, b), std::max(c, d)));
    return at;
}

hipError_t launch_interruptions(const int32_t *rows, const int32_t *offsets, const uint8_t *pool, int64_t n, size_t pool_bytes, int64_t length, uint8_t *work,
                                size_t work_bytes, const InterruptionLayout &at, hipStream_t stream) {
    if (work_bytes < at.bytes) return hipErrorInvalidValue;
    void *scratch = work + at.scratch;
    const size_t scratch_bytes = at.scratch_bytes;
    const size_t cap = interruptions_op_cap(pool_bytes);
    const int64_t chunks = (int64_t)((pool_bytes + 15) / 16);
    uint32_t *counts = region<uint32_t>(work, at.counts), *op_row = region<uint32_t>(work, at.op_row);
    uint32_t *first_op = region<uint32_t>(work, at.first_op), *run_head = region<uint32_t>(work, at.run_head);
    uint32_t *width = region<uint32_t>(work, at.width);
    uint64_t *ops = region<uint64_t>(work, at.ops);
    InterruptionSums *sums = region<InterruptionSums>(work, at.sums);
    InterruptionBest *best_in = region<InterruptionBest>(work, at.best), *best = best_in + cap;
    int32_t *source = region<int32_t>(work, at.source), *offsets32 = region<int32_t>(work, at.offsets32);
    unsigned long long *offsets64 = region<unsigned long long>(work, at.offsets64);
    RibbitRowPurity *out_rows = region<RibbitRowPurity>(work, at.rows);
    RibbitInterruption *sites = region<RibbitInterruption>(work, at.sites);
    InterruptionTotals *totals = region<InterruptionTotals>(work, at.totals);
    const dim3 block(ROW_THREADS), by_chunk(grid_for(chunks + 1, ROW_THREADS, ROW_MAX_BLOCKS)), by_row(grid_for(n + 1, ROW_THREADS, ROW_MAX_BLOCKS)),
        by_op(grid_for((int64_t)cap + 1, ROW_THREADS, ROW_MAX_BLOCKS));
    hipError_t e;
    // the totals start as: no ops, nothing bad (bad_at and bad_row lie side by side)
    if ((e = hipMemsetAsync(totals, 0, sizeof(InterruptionTotals), stream)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(&totals->bad_at, 0xff, 2 * sizeof(uint32_t), stream)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(op_row, 0, cap * sizeof(uint32_t), stream)) != hipSuccess) return e;
    hipLaunchKernelGGL(int_count_kernel, by_chunk, block, 0, stream, reinterpret_cast<const uint4 *>(pool), chunks, (int64_t)pool_bytes, counts, totals);
    size_t bytes = scratch_bytes;
    if ((e = scan_counts(scratch, bytes, counts, (size_t)chunks + 1, stream)) != hipSuccess) return e;
    hipLaunchKernelGGL(int_emit_kernel, by_chunk, block, 0, stream, reinterpret_cast<const uint4 *>(pool), chunks, (int64_t)pool_bytes, counts, ops, (uint32_t)cap);
    hipLaunchKernelGGL(int_row_heads_kernel, by_row, block, 0, stream, pool, offsets, n, (int64_t)pool_bytes, counts, first_op, op_row, (uint32_t)cap, totals);
    bytes = scratch_bytes;
    if ((e = scan_sums(scratch, bytes, ops, op_row, totals, sums, cap, stream)) != hipSuccess) return e;
    hipLaunchKernelGGL(int_run_heads_kernel, by_op, block, 0, stream, ops, op_row, sums, run_head, totals);
    hipLaunchKernelGGL(int_runs_kernel, by_op, block, 0, stream, rows, offsets, n, length, ops, op_row, first_op, sums, run_head, totals, best_in, sites, width, source);
    bytes = scratch_bytes;
    if ((e = scan_best(scratch, bytes, best_in, totals, best, cap, stream)) != hipSuccess) return e;
    bytes = scratch_bytes;
    if ((e = scan_widths(scratch, bytes, width, totals, offsets64, cap + 1, stream)) != hipSuccess) return e;
    hipLaunchKernelGGL(int_offsets_kernel, by_op, block, 0, stream, offsets64, offsets32, totals);
    hipLaunchKernelGGL(int_finish_kernel, by_row, block, 0, stream, rows, n, first_op, sums, best, out_rows, totals);
    return hipGetLastError();
}

hipError_t launch_interruption_gather(const uint8_t *ascii, uint8_t *work, const InterruptionLayout &at, uint32_t sites, int64_t observed, uint8_t *out,
                                      hipStream_t stream) {
    const int64_t spans = (observed + INTERRUPTION_SPAN - 1) / INTERRUPTION_SPAN;
    const int32_t *offsets32 = region<const int32_t>(work, at.offsets32), *source = region<const int32_t>(work, at.source);
    int32_t *span_site = region<int32_t>(work, at.spans);
    hipLaunchKernelGGL(int_spans_kernel, dim3(grid_for(spans + 1, ROW_THREADS, INT32_MAX)), dim3(ROW_THREADS), 0, stream, offsets32, (int32_t)sites, observed, spans,
                       span_site);
    hipLaunchKernelGGL(int_gather_kernel, dim3(grid_for(spans, 1, 256 * 64)), dim3(ROW_THREADS), 0, stream, ascii, offsets32, source, span_site, (int32_t)sites,
                       observed, reinterpret_cast<uint4 *>(out));
    return hipGetLastError();
}

}  // namespace rb
