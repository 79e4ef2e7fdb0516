// classes.hip -- the rows of the loaded record grouped by canonical motif class (api_classes.cpp: ribbit_hip_record_classes), as
// include/ribbit_hip.h states it: the class of a motif is the least of the 2k strings that are its rotations and the rotations of
// its reverse complement, the strand says whether a rotation of the motif itself is that least string.  Integer and byte work on
// wave64; no count goes to the host in between.  On the handle's stream:
//   short:    one lane per row, rows in grid-stride waves.  A motif of k <= 32 bases is read with aligned 8-byte loads (at most five,
//             only the words it touches) and a funnel shift, 2-bit packed into one register (first base in the high bits of the 2k
//             bit field, A < C < G < T, so integer order is byte order), its reverse complement by a bit reversal; k rotations of
//             each by shifts, the minimum kept.  It writes the class as ASCII at the row's own offset, the strand byte, and the
//             row's sort item.  A row with k > 32 is appended to a list instead (a ballot, a popc and one atomic per wave and turn)
//   long:     one wavefront (a block of 64) per listed row: the motif and its reverse complement are staged in LDS, each twice in a
//             row, so that a rotation is a plain window.  Lane j judges the candidates j, j + 64, ... of the 2k (a start and a
//             strand) against its best so far, byte by byte with early exit, then six steps of a wave reduction compare two
//             candidates the same way.  Equal strings: the lower candidate number, and the k candidates of the motif itself come
//             first, so ties go to '+'
//   sort:     one rocPRIM merge sort of the items (key, row, offset) with a comparator that is a total order: the 64-bit key (10
//             bits of length, then the first 27 bases of the class), then, only for equal keys with k > 27, the class bytes from
//             base 28 on, then the row index
//   heads:    one lane per sorted position: whether its class differs from its predecessor's (key; bytes for k > 27)
//   scan:     a rocPRIM inclusive scan of the head flags: the group id of every sorted position (plus one)
//   reduce:   a rocPRIM reduce_by_key over the group ids: rows, bases (64-bit), the maximum of width << 32 | ~index, the least index
//   groups:   one lane per group: the aggregate as a RibbitMotifClass
#include <cstring>

#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>

#include "row_kernels.h"

namespace rb {

namespace {

constexpr int SHORT_MAX = 32;                   // bases one 64-bit register holds
constexpr int KEY_BASES = 27;                   // bases the key holds behind its 10 bits of length
constexpr int MOTIF_MAX = 1023;

struct ClassAgg {                               // what a group's rows reduce to
    int64_t bases;
    uint64_t longest;                           // width << 32 | ~index
    int32_t rows, first;
};
static_assert(sizeof(ClassItem) == 16 && sizeof(ClassAgg) == 24, "as ClassesLayout says");

// the 2-bit codes of 8 ASCII bases (A 0, C 1, G 2, T 3), the first (lowest) byte in the highest two of 16 bits
__device__ inline uint64_t pack8(uint64_t v) {
    const uint64_t x = ((v >> 1) & 0x0303030303030303ull) ^ ((v >> 2) & 0x0101010101010101ull);
    const uint64_t y = ((x & 0x00FF00FF00FF00FFull) << 2) | ((x >> 8) & 0x00FF00FF00FF00FFull);
    const uint64_t z = ((y & 0x0000FFFF0000FFFFull) << 4) | ((y >> 16) & 0x0000FFFF0000FFFFull);
    return ((z & 0xFFFFFFFFull) << 8) | (z >> 32);
}

__device__ inline uint8_t base_of(uint32_t code) { return (uint8_t)(0x54474341u >> (8 * code)); }      // "ACGT"
__device__ inline uint32_t code_of(uint8_t c) { return ((c >> 1) & 3u) ^ ((c >> 2) & 1u); }

// the key of a class of k bases whose first min(k, 27) bases are `head`, right-aligned
__device__ inline uint64_t class_key(int k, uint64_t head) { return (uint64_t)k << 54 | head << (2 * (KEY_BASES - min(k, KEY_BASES))); }

// Rows in grid-stride waves (every lane of a wave takes the same number of turns: the ballot sees whole waves).  pool is 8-byte
// aligned and has 16 readable bytes behind its last motif.
__global__ void __launch_bounds__(ROW_THREADS) classes_short_kernel(const int32_t *__restrict__ off, const uint8_t *__restrict__ pool, int64_t n,
                                                                      ClassItem *__restrict__ items, uint8_t *__restrict__ classes,
                                                                      uint8_t *__restrict__ strands, int32_t *__restrict__ long_rows,
                                                                      unsigned long long *__restrict__ n_long) {
    const int lane = threadIdx.x & 63;
    const int64_t waves = (int64_t)gridDim.x * (ROW_THREADS / 64);
    for (int64_t base = ((int64_t)blockIdx.x * (ROW_THREADS / 64) + (threadIdx.x >> 6)) * 64; base < n; base += waves * 64) {
        const int64_t i = base + lane;
        bool is_long = false;
        if (i < n) {
            const uint32_t o = (uint32_t)off[i];
            const int k = off[i + 1] - (int32_t)o;
            is_long = k > SHORT_MAX;
            if (!is_long) {
                const uint64_t *w = reinterpret_cast<const uint64_t *>(pool + (o & ~7u));
                const int words = (int)((o & 7u) + (uint32_t)k + 7u) >> 3;      // 1 .. 5
                const uint64_t w0 = w[0], w1 = words > 1 ? w[1] : 0, w2 = words > 2 ? w[2] : 0, w3 = words > 3 ? w[3] : 0, w4 = words > 4 ? w[4] : 0;
                const int sh = (int)(o & 7u) * 8;
                const uint64_t v0 = sh ? w0 >> sh | w1 << (64 - sh) : w0, v1 = sh ? w1 >> sh | w2 << (64 - sh) : w1;
                const uint64_t v2 = sh ? w2 >> sh | w3 << (64 - sh) : w2, v3 = sh ? w3 >> sh | w4 << (64 - sh) : w3;
                const int spare = 64 - 2 * k;                                  // 0 .. 62
                const uint64_t mask = ~(uint64_t)0 >> spare;
                uint64_t u = (pack8(v0) << 48 | pack8(v1) << 32 | pack8(v2) << 16 | pack8(v3)) >> spare;
                uint64_t r = __brevll(~u);                                     // the complement, its 2-bit groups reversed ...
                r = ((r & 0x5555555555555555ull) << 1 | ((r >> 1) & 0x5555555555555555ull)) >> spare;      // ... and each group's bits put back
                uint64_t best_u = u, best_r = r;
                for (int t = 1; t < k; ++t) {
                    u = (u << 2 | u >> (2 * k - 2)) & mask;
                    r = (r << 2 | r >> (2 * k - 2)) & mask;
                    best_u = min(best_u, u);
                    best_r = min(best_r, r);
                }
                const uint64_t cls = min(best_u, best_r);
                for (int t = 0; t < k; ++t) classes[o + t] = base_of((uint32_t)(cls >> (2 * (k - 1 - t))) & 3u);
                strands[i] = best_u <= best_r ? '+' : '-';
                items[i] = ClassItem{class_key(k, k > KEY_BASES ? cls >> (2 * (k - KEY_BASES)) : cls), (uint32_t)i, o};
            }
        }
        const unsigned long long votes = __ballot(is_long);
        if (votes) {                                                           // (the same for all of the wave)
            unsigned long long slot = 0;
            if (lane == 0) slot = atomicAdd(n_long, (unsigned long long)__popcll(votes));
            slot = __shfl(slot, 0);
            if (is_long) long_rows[slot + (unsigned long long)__popcll(votes & ((1ull << lane) - 1))] = (int32_t)i;
        }
    }
}

// -1, 0, 1: the k bytes at a against the k bytes at b
__device__ inline int compare_windows(const uint8_t *s, int a, int b, int k) {
    for (int t = 0; t < k; ++t) {
        const int x = s[a + t], y = s[b + t];
        if (x != y) return x < y ? -1 : 1;
    }
    return 0;
}

// One wavefront per block and per listed row.  LDS: motif | motif | reverse complement | reverse complement, k bytes each, so
// candidate c < k is the window at c and candidate c >= k (rotation c - k of the reverse complement) the window at c + k.
__global__ void __launch_bounds__(64) classes_long_kernel(const int32_t *__restrict__ off, const uint8_t *__restrict__ pool, ClassItem *__restrict__ items,
                                                          uint8_t *__restrict__ classes, uint8_t *__restrict__ strands,
                                                          const int32_t *__restrict__ long_rows, const unsigned long long *__restrict__ n_long) {
    __shared__ uint8_t s[4 * (MOTIF_MAX + 1)];
    const int lane = threadIdx.x;
    const unsigned long long count = *n_long;
    for (unsigned long long at = blockIdx.x; at < count; at += gridDim.x) {
        const int32_t i = long_rows[at];
        const uint32_t o = (uint32_t)off[i];
        const int k = min(off[i + 1] - (int32_t)o, MOTIF_MAX);                  // (33 .. 1023: the host has checked)
        for (int t = lane; t < k; t += 64) {
            const uint8_t c = pool[o + t], cc = base_of(3u - code_of(c));
            s[t] = s[k + t] = c;
            s[3 * k - 1 - t] = s[4 * k - 1 - t] = cc;
        }
        __syncthreads();
        auto start = [k](int c) { return c < k ? c : c + k; };
        int best = lane;                                                       // (2k > 64: every lane has a candidate)
        for (int c = lane + 64; c < 2 * k; c += 64)
            if (compare_windows(s, start(c), start(best), k) < 0) best = c;
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) {
            const int other = __shfl_down(best, d);
            if (lane + d < 64) {
                const int order = compare_windows(s, start(other), start(best), k);
                if (order < 0 || (order == 0 && other < best)) best = other;
            }
        }
        best = __shfl(best, 0);
        const int from = start(best);
        for (int t = lane; t < k; t += 64) classes[o + t] = s[from + t];
        if (lane == 0) {
            uint64_t head = 0;
            for (int t = 0; t < KEY_BASES; ++t) head = head << 2 | code_of(s[from + t]);
            strands[i] = best < k ? '+' : '-';
            items[i] = ClassItem{class_key(k, head), (uint32_t)i, o};
        }
        __syncthreads();                                                       // (the next row's staging overwrites s)
    }
}

// whether two rows' classes differ beyond their equal keys: only a class of more than 27 bases has bytes the key does not hold
__host__ __device__ inline int compare_tails(const uint8_t *classes, const ClassItem &a, const ClassItem &b) {
    const int k = (int)(a.key >> 54);
    for (int t = KEY_BASES; t < k; ++t) {
        const int x = classes[a.off + t], y = classes[b.off + t];
        if (x != y) return x < y ? -1 : 1;
    }
    return 0;
}

struct ClassLess {
    const uint8_t *classes;
    __host__ __device__ bool operator()(const ClassItem &a, const ClassItem &b) const {
        if (a.key != b.key) return a.key < b.key;
        const int order = compare_tails(classes, a, b);
        return order ? order < 0 : a.row < b.row;
    }
};

__global__ void __launch_bounds__(ROW_THREADS) classes_heads_kernel(const ClassItem *__restrict__ sorted, const uint8_t *__restrict__ classes, int64_t n,
                                                                      uint32_t *__restrict__ head) {
    for (int64_t j = (int64_t)blockIdx.x * ROW_THREADS + threadIdx.x; j < n; j += (int64_t)gridDim.x * ROW_THREADS) {
        bool first = j == 0;
        if (!first) {
            const ClassItem a = sorted[j - 1], b = sorted[j];
            first = a.key != b.key || compare_tails(classes, a, b) != 0;
        }
        head[j] = first ? 1u : 0u;
    }
}

// what the row at sorted position j brings to its group
struct RowOfGroup {
    const ClassItem *sorted;
    const int32_t *iv;
    int64_t length;
    __host__ __device__ ClassAgg operator()(int64_t j) const {
        const uint32_t row = sorted[j].row;
        const auto [s, e] = clip_row(iv, (int64_t)row, length);
        const int64_t width = max(e - s, (int64_t)0);
        return ClassAgg{width, (uint64_t)width << 32 | (uint64_t)(uint32_t)~row, 1, (int32_t)row};
    }
};

struct JoinRows {
    __host__ __device__ ClassAgg operator()(const ClassAgg &a, const ClassAgg &b) const {
        return ClassAgg{a.bases + b.bases, a.longest > b.longest ? a.longest : b.longest, a.rows + b.rows, a.first < b.first ? a.first : b.first};
    }
};

__global__ void __launch_bounds__(ROW_THREADS) classes_groups_kernel(const ClassAgg *__restrict__ agg, const int32_t *__restrict__ off,
                                                                       const unsigned long long *__restrict__ n_groups, int64_t n,
                                                                       RibbitMotifClass *__restrict__ groups) {
    const int64_t count = min((int64_t)*n_groups, n);
    for (int64_t g = (int64_t)blockIdx.x * ROW_THREADS + threadIdx.x; g < count; g += (int64_t)gridDim.x * ROW_THREADS) {
        const ClassAgg a = agg[g];
        groups[g] = RibbitMotifClass{a.bases, off[a.first + 1] - off[a.first], a.rows, a.first, (int32_t)~(uint32_t)a.longest};
    }
}

hipError_t sort_items(void *scratch, size_t &bytes, ClassItem *items, ClassItem *sorted, const uint8_t *classes, int64_t n, hipStream_t stream) {
    return rocprim::merge_sort(scratch, bytes, items, sorted, (size_t)n, ClassLess{classes}, stream);
}

hipError_t scan_heads(void *scratch, size_t &bytes, const uint32_t *head, uint32_t *gid, int64_t n, hipStream_t stream) {
    return rocprim::inclusive_scan(scratch, bytes, head, gid, (size_t)n, rocprim::plus<uint32_t>(), stream);
}

hipError_t reduce_groups(void *scratch, size_t &bytes, const uint32_t *gid, const ClassItem *sorted, const int32_t *iv, int64_t length, ClassAgg *agg,
                         unsigned long long *n_groups, int64_t n, hipStream_t stream) {
    return rocprim::reduce_by_key(scratch, bytes, gid, rocprim::make_transform_iterator(rocprim::make_counting_iterator<int64_t>(0), RowOfGroup{sorted, iv, length}),
                                  (size_t)n, rocprim::make_discard_iterator(), agg, n_groups, JoinRows(), rocprim::equal_to<uint32_t>(), stream);
}

}  // namespace

ClassesLayout classes_layout(int64_t n, size_t pool_bytes) {
    const size_t rows = (size_t)n;
    size_t a = 0, b = 0, c = 0;
    (void)sort_items(nullptr, a, nullptr, nullptr, nullptr, n, 0);
    (void)scan_heads(nullptr, b, nullptr, nullptr, n, 0);
    (void)reduce_groups(nullptr, c, nullptr, nullptr, nullptr, 0, nullptr, nullptr, n, 0);
    ClassesLayout at{};
    WorkCarver w;
    at.items = w.take(2 * rows * sizeof(ClassItem));
    at.agg = w.take(rows * sizeof(ClassAgg));
    at.heads = w.take(2 * rows * sizeof(uint32_t));
    at.long_rows = w.take(rows * sizeof(int32_t));
    at.header = w.take(sizeof(ClassHeader));
    at.groups = w.take(rows * sizeof(RibbitMotifClass));
    at.strands = w.take(rows);
    at.classes = w.take(pool_bytes);
    w.close(at, std::max(a, std::max(b, c)));
    return at;
}

hipError_t launch_classes(const int32_t *rows, const int32_t *offsets, const uint8_t *pool, int64_t n, int64_t length, uint8_t *work, size_t work_bytes,
                          const ClassesLayout &at, hipStream_t stream) {
    if (work_bytes < at.bytes) return hipErrorInvalidValue;
    ClassItem *items = region<ClassItem>(work, at.items), *sorted = items + n;
    ClassAgg *agg = region<ClassAgg>(work, at.agg);
    uint32_t *head = region<uint32_t>(work, at.heads), *gid = head + n;
    int32_t *long_rows = region<int32_t>(work, at.long_rows);
    ClassHeader *header = region<ClassHeader>(work, at.header);
    RibbitMotifClass *groups = region<RibbitMotifClass>(work, at.groups);
    uint8_t *strands = region<uint8_t>(work, at.strands), *classes = region<uint8_t>(work, at.classes);
    void *scratch = work + at.scratch;
    const size_t scratch_bytes = at.scratch_bytes;
    const dim3 grid(grid_for(n, ROW_THREADS, ROW_MAX_BLOCKS)), block(ROW_THREADS);
    hipError_t e = hipMemsetAsync(header, 0, sizeof(ClassHeader), stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(classes_short_kernel, grid, block, 0, stream, offsets, pool, n, items, classes, strands, long_rows, &header->long_rows);
    // (how many rows are long stays on the device: at most one block per row, and a block that finds the list empty ends at once)
    hipLaunchKernelGGL(classes_long_kernel, dim3(grid_for(n, 1, ROW_MAX_BLOCKS)), dim3(64), 0, stream, offsets, pool, items, classes, strands, long_rows,
                       &header->long_rows);
    size_t bytes = scratch_bytes;
    if ((e = sort_items(scratch, bytes, items, sorted, classes, n, stream)) != hipSuccess) return e;
    hipLaunchKernelGGL(classes_heads_kernel, grid, block, 0, stream, sorted, classes, n, head);
    bytes = scratch_bytes;
    if ((e = scan_heads(scratch, bytes, head, gid, n, stream)) != hipSuccess) return e;
    bytes = scratch_bytes;
    if ((e = reduce_groups(scratch, bytes, gid, sorted, rows, length, agg, &header->groups, n, stream)) != hipSuccess) return e;
    hipLaunchKernelGGL(classes_groups_kernel, grid, block, 0, stream, agg, offsets, &header->groups, n, groups);
    return hipGetLastError();
}

}  // namespace rb
