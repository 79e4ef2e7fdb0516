// primer_products.hip -- in-silico PCR on the loaded record: the sites of oligos on either strand, from the bit planes the scans
// read, and the products of primer pairs among those sites (api_primer_products.cpp: ribbit_hip_record_oligo_sites,
// ribbit_hip_record_primer_products; include/ribbit_hip.h has the contract, kernels.h the order of the launches).
//   uniques    The oligos become sort items (length, bases, index); one rocPRIM merge sort, head flags, one inclusive sum: every
//              oligo knows its unique oligo, and equal oligos are searched once.  On tiled simulated data 1.6 million primers are
//              some thousands of oligos: without this step the work per position grows with the copies.
//   patterns   A unique oligo u gives two patterns on the forward strand, both k <= 32 bits of the hi and of the lo plane with
//              window base j at bit j: 2 u, its bases with the seed at the window's END (a forward site), and 2 u + 1, its reverse
//              complement with the seed at the window's START (a reverse site).  The seed key of a pattern is its seed's bits in
//              plane form, hi << 16 | lo (2 seed <= 32 bits): the key of a position of the record then is two funnel shifts of the
//              plane words and no interleave.  The patterns are sorted by key with one rocPRIM radix sort.
//   scan       The hot path, one pass over the three planes in device_planes.h's tile shape: a wavefront per tile, a lane owns
//              WORDS_PER_LANE consecutive words, so the word before and behind a position's word are the lane's own or its
//              neighbour's and a window of 32 bases is one funnel shift of two of them.  A position whose seed holds a brk bit is
//              skipped, and so is one whose key's hash has no bit in a bitmap of all patterns' hashed keys (16 bits per pattern, a
//              megabyte for a chromosome's primers: one load in front of some twenty dependent ones).  Its key is bisected in the
//              sorted keys (the lower bound, a fixed number of steps for the whole wavefront), and for every pattern behind an
//              equal key the whole window is verified:
//              popcount(((w_hi ^ o_hi) | (w_lo ^ o_lo)) & non_seed) <= d and (w_brk & window) == 0.  The lead padding and the tail
//              have brk = 1, so a window that hangs off the record refuses itself.
//   lists      Every pattern has one counter and max_sites slots; the device memory is fixed before the scan.  A site takes its slot
//              with a returning add and is written only when slot < max_sites, so the count is exact whatever the list holds.  The
//              add is aggregated per wavefront: the lanes that found a site of one pattern in the same step (a homopolymer: all
//              64) send one add, and each takes base + its rank.  Slots are taken in no fixed order, so a list that is complete
//              (count <= max_sites) is sorted afterwards, one wavefront per list, bitonic in LDS: the result is the same from run
//              to run.  A list that is not complete is never read.
//   products   One lane per pair over its four sorted lists (product_walk.h, shared with primer_specific.hip): for every forward
//              site two bisections per reverse list give the sites in [x + k1, x + max_product - k2]; the same walk gives `own`
//              and `shortest_other`.
// Integer vector atomics only; no inline assembly.
#include <cstring>

#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>

#include "product_walk.h"

namespace rb {

namespace {

constexpr int SCAN_WAVES = 4;
constexpr int MAX_SITES = 1024;
static_assert(sizeof(RibbitRowProducts) == 32 && sizeof(RibbitOligoSites) == 16 && sizeof(RibbitOligo) == 12 && sizeof(ProductPattern) == 16, "8, 4, 3 and 4 ints");

struct OligoItem {
    unsigned long long bases;
    uint32_t length, index;
};
struct OligoLess {
    __host__ __device__ bool operator()(const OligoItem &a, const OligoItem &b) const {
        if (a.length != b.length) return a.length < b.length;
        if (a.bases != b.bases) return a.bases < b.bases;
        return a.index < b.index;
    }
};
__host__ __device__ inline uint32_t low_bits(int k) { return k >= 32 ? 0xffffffffu : (1u << k) - 1u; }
// the even bits of v, packed
__device__ inline uint32_t even_bits(unsigned long long v) {
    v &= 0x5555555555555555ull;
    v = (v | (v >> 1)) & 0x3333333333333333ull;
    v = (v | (v >> 2)) & 0x0f0f0f0f0f0f0f0full;
    v = (v | (v >> 4)) & 0x00ff00ff00ff00ffull;
    v = (v | (v >> 8)) & 0x0000ffff0000ffffull;
    v = (v | (v >> 16)) & 0x00000000ffffffffull;
    return (uint32_t)v;
}
// bits sh .. sh + 31 of hi : lo, 0 <= sh <= 31
__device__ inline uint32_t funnel(uint32_t lo, uint32_t hi, int sh) { return (uint32_t)((((unsigned long long)hi << 32) | lo) >> sh); }

// a unique oligo's pattern on one strand: strand 0 its bases, strand 1 their reverse complement
__device__ inline ProductPattern pattern_of(const UniqueOligo &u, uint32_t id) {
    const int k = (int)u.length;
    uint32_t hi = even_bits(u.bases >> 1), lo = even_bits(u.bases);
    if (id & 1u) {
        hi = (~__brev(hi) >> (32 - k)) & low_bits(k);
        lo = (~__brev(lo) >> (32 - k)) & low_bits(k);
    }
    return ProductPattern{hi, lo, id, (uint32_t)k};
}
// where the pattern's window starts before the position of its seed, and its bases outside the seed
__device__ inline int seed_offset(const ProductPattern &p, int seed) { return (p.id & 1u) ? 0 : (int)p.k - seed; }
__device__ inline uint32_t non_seed(const ProductPattern &p, int seed) { return (p.id & 1u) ? low_bits((int)p.k) & ~low_bits(seed) : low_bits((int)p.k - seed); }
__device__ inline uint32_t seed_key(const ProductPattern &p, int seed) {
    const int off = seed_offset(p, seed);
    return ((p.hi >> off) & low_bits(seed)) << 16 | ((p.lo >> off) & low_bits(seed));
}

__global__ void __launch_bounds__(ROW_THREADS) oligo_items_kernel(const RibbitOligo *__restrict__ oligos, int64_t n, OligoItem *__restrict__ items) {
    for (int64_t i = (int64_t)blockIdx.x * ROW_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * ROW_THREADS) {
        const RibbitOligo o = oligos[i];
        const unsigned long long bases = (unsigned long long)(uint32_t)o.bases_hi << 32 | (uint32_t)o.bases_lo;
        items[i] = OligoItem{o.length >= 32 ? bases : bases & ((1ull << (2 * o.length)) - 1ull), (uint32_t)o.length, (uint32_t)i};
    }
}

__global__ void __launch_bounds__(ROW_THREADS) oligo_heads_kernel(const OligoItem *__restrict__ sorted, int64_t n, uint32_t *__restrict__ head) {
    for (int64_t i = (int64_t)blockIdx.x * ROW_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * ROW_THREADS)
        head[i] = i == 0 || sorted[i].length != sorted[i - 1].length || sorted[i].bases != sorted[i - 1].bases ? 1u : 0u;
}

// every oligo's unique oligo; the unique oligos and the keys of their two patterns
__global__ void __launch_bounds__(ROW_THREADS) oligo_uniques_kernel(const OligoItem *__restrict__ sorted, const uint32_t *__restrict__ head, const uint32_t *__restrict__ gid,
                                                                      int64_t n, int seed, uint32_t *__restrict__ unique_of, UniqueOligo *__restrict__ uniques,
                                                                      uint32_t *__restrict__ keys, uint32_t *__restrict__ ids, ProductHeader *__restrict__ header) {
    for (int64_t i = (int64_t)blockIdx.x * ROW_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * ROW_THREADS) {
        const OligoItem it = sorted[i];
        const uint32_t u = gid[i] - 1u;
        unique_of[it.index] = u;
        if (head[i]) {
            const UniqueOligo uo{it.bases, it.length, 0u};
            uniques[u] = uo;
            for (uint32_t strand = 0; strand < 2; ++strand) {
                keys[2 * u + strand] = seed_key(pattern_of(uo, 2 * u + strand), seed);
                ids[2 * u + strand] = 2 * u + strand;
            }
        }
        if (i == n - 1) header->uniques = u + 1u;
    }
}

__global__ void __launch_bounds__(ROW_THREADS) pattern_fill_kernel(const uint32_t *__restrict__ ids_sorted, const UniqueOligo *__restrict__ uniques, int64_t n_patterns,
                                                                     ProductPattern *__restrict__ patterns) {
    for (int64_t i = (int64_t)blockIdx.x * ROW_THREADS + threadIdx.x; i < n_patterns; i += (int64_t)gridDim.x * ROW_THREADS)
        patterns[i] = pattern_of(uniques[ids_sorted[i] >> 1], ids_sorted[i]);
}

// ---- the site scan
__device__ inline uint32_t key_hash(uint32_t key, int log2_bits) { return (key * 0x9e3779b1u) >> (32 - log2_bits); }

__global__ void __launch_bounds__(ROW_THREADS) filter_fill_kernel(const uint32_t *__restrict__ keys, int64_t n_patterns, int log2_bits, uint32_t *__restrict__ filter) {
    for (int64_t i = (int64_t)blockIdx.x * ROW_THREADS + threadIdx.x; i < n_patterns; i += (int64_t)gridDim.x * ROW_THREADS) {
        const uint32_t h = key_hash(keys[i], log2_bits);
        atomicOr(&filter[h >> 5], 1u << (h & 31u));
    }
}

// The lanes that hold a site of one pattern in this step take consecutive slots of its list with one add.  Every lane of the
// wavefront calls it, with `hit` or without.
__device__ inline void push_sites(bool hit, uint32_t id, int32_t x, uint32_t *__restrict__ counts, int32_t *__restrict__ lists, int max_sites, int lane) {
    unsigned long long pending = __ballot(hit);
    while (pending) {
        const int leader = __builtin_ctzll(pending);
        const uint32_t id_l = (uint32_t)__shfl((int)id, leader);
        const bool mine = hit && id == id_l;
        const unsigned long long same = __ballot(mine);
        uint32_t base = 0;
        if (lane == leader) base = atomicAdd(&counts[id_l], (uint32_t)__popcll(same));
        base = (uint32_t)__shfl((int)base, leader);
        if (mine) {
            const uint32_t slot = base + (uint32_t)__popcll(same & ((1ull << lane) - 1ull));
            if (slot < (uint32_t)max_sites) lists[(int64_t)id * max_sites + slot] = x;
            hit = false;
        }
        pending &= ~same;
    }
}

__global__ void __launch_bounds__(64 * SCAN_WAVES) site_scan_kernel(DevicePlanes pl, const uint32_t *__restrict__ keys, const ProductPattern *__restrict__ patterns,
                                                                   uint32_t n_patterns, const uint32_t *__restrict__ filter, int filter_log2, int seed,
                                                                   int max_mismatches, int max_sites, uint32_t *__restrict__ counts, int32_t *__restrict__ lists) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t seed_bits = low_bits(seed);
    uint32_t top = 1;      // the bisection's first step: the largest power of two <= n_patterns
    while (2ull * top <= n_patterns) top <<= 1;
    for (int64_t tile = (int64_t)blockIdx.x * SCAN_WAVES + wave; tile < pl.ntiles; tile += (int64_t)gridDim.x * SCAN_WAVES) {
        const int64_t w0 = tile * TILE_WORDS + (int64_t)lane * WORDS_PER_LANE;
        // the word before the lane's first (index -1 is the lead padding: brk = 1)
        uint32_t prev_h = pl.hi[w0 - 1], prev_l = pl.lo[w0 - 1], prev_b = pl.brk[w0 - 1];
        uint32_t cur_h = pl.hi[w0], cur_l = pl.lo[w0], cur_b = pl.brk[w0];
        for (int i = 0; i < WORDS_PER_LANE; ++i) {
            const int64_t w = w0 + i;
            const uint32_t next_h = pl.hi[w + 1], next_l = pl.lo[w + 1], next_b = pl.brk[w + 1];      // (at most word ntiles * TILE_WORDS: the tail)
            // a wavefront whose 64 words here are all brk (an N block, the tail) has nothing to look up
            if (__any(cur_b != 0xffffffffu)) {
                for (int b = 0; b < 32; ++b) {
                    bool live = (funnel(cur_b, next_b, b) & seed_bits) == 0u;
                    const uint32_t key = (funnel(cur_h, next_h, b) & seed_bits) << 16 | (funnel(cur_l, next_l, b) & seed_bits);
                    if (filter && live) {
                        const uint32_t h = key_hash(key, filter_log2);
                        live = (filter[h >> 5] >> (h & 31u)) & 1u;
                    }
                    if (!__any(live)) continue;
                    // the first pattern whose key is not below this one
                    uint32_t at = 0;
                    for (uint32_t step = top; step; step >>= 1) {
                        const uint32_t probe = at + step;
                        if (live && probe <= n_patterns && keys[probe - 1] < key) at = probe;
                    }
                    for (;;) {
                        const bool candidate = live && at < n_patterns && keys[at] == key;
                        if (!__any(candidate)) break;
                        bool hit = false;
                        uint32_t id = 0;
                        int32_t x = 0;
                        if (candidate) {
                            const ProductPattern p = patterns[at];
                            const int off = seed_offset(p, seed), sh = 32 + b - off;      // 6 .. 63: where the window starts in prev : cur : next
                            const uint32_t wh = sh < 32 ? funnel(prev_h, cur_h, sh) : funnel(cur_h, next_h, sh - 32);
                            const uint32_t wl = sh < 32 ? funnel(prev_l, cur_l, sh) : funnel(cur_l, next_l, sh - 32);
                            const uint32_t wb = sh < 32 ? funnel(prev_b, cur_b, sh) : funnel(cur_b, next_b, sh - 32);
                            hit = (wb & low_bits((int)p.k)) == 0u && (int)__popc(((wh ^ p.hi) | (wl ^ p.lo)) & non_seed(p, seed)) <= max_mismatches;
                            id = p.id;
                            x = (int32_t)(w * 32 + b - off);
                            ++at;
                        }
                        push_sites(hit, id, x, counts, lists, max_sites, lane);
                    }
                }
            }
            prev_h = cur_h; prev_l = cur_l; prev_b = cur_b;
            cur_h = next_h; cur_l = next_l; cur_b = next_b;
        }
    }
}

// every complete list of 2 .. max_sites sites in ascending order: one wavefront per list, bitonic in LDS
__global__ void __launch_bounds__(64) sort_lists_kernel(const uint32_t *__restrict__ counts, int64_t n_patterns, int max_sites, int32_t *__restrict__ lists) {
    __shared__ int32_t s[MAX_SITES];
    const int lane = threadIdx.x;
    for (int64_t t = blockIdx.x; t < n_patterns; t += gridDim.x) {
        const uint32_t c = counts[t];
        if (c < 2u || c > (uint32_t)max_sites) continue;      // (the same for the whole block)
        int32_t *list = lists + t * max_sites;
        int n = 64;
        while (n < (int)c) n <<= 1;
        for (int i = lane; i < n; i += 64) s[i] = i < (int)c ? list[i] : INT32_MAX;
        __syncthreads();
        for (int k = 2; k <= n; k <<= 1)
            for (int j = k >> 1; j > 0; j >>= 1) {
                for (int i = lane; i < n; i += 64) {
                    const int other = i ^ j;
                    if (other > i) {
                        const int32_t a = s[i], b = s[other];
                        if ((a > b) == ((i & k) == 0)) { s[i] = b; s[other] = a; }
                    }
                }
                __syncthreads();
            }
        for (int i = lane; i < (int)c; i += 64) list[i] = s[i];
        __syncthreads();
    }
}

// ---- the products of a pair (product_walk.h)
__global__ void __launch_bounds__(ROW_THREADS) pair_products_kernel(const int32_t *__restrict__ pairs, int64_t n_pairs, const uint32_t *__restrict__ unique_of,
                                                                      const UniqueOligo *__restrict__ uniques, const uint32_t *__restrict__ counts,
                                                                      const int32_t *__restrict__ lists, int max_product, int max_sites, RibbitRowProducts *__restrict__ out) {
    for (int64_t i = (int64_t)blockIdx.x * ROW_THREADS + threadIdx.x; i < n_pairs; i += (int64_t)gridDim.x * ROW_THREADS) {
        const int32_t ia = pairs[4 * i], ib = pairs[4 * i + 1], left_start = pairs[4 * i + 2], right_start = pairs[4 * i + 3];
        out[i] = ia >= 0 ? pair_products(unique_of[ia], unique_of[ib], left_start, right_start, uniques, counts, lists, max_product, max_sites) : RibbitRowProducts{};
    }
}

// ---- the sites of the oligos as they were given
__global__ void __launch_bounds__(ROW_THREADS) site_lens_kernel(const uint32_t *__restrict__ unique_of, const uint32_t *__restrict__ counts, int64_t n, int max_sites,
                                                                  uint32_t *__restrict__ lens) {
    for (int64_t i = (int64_t)blockIdx.x * ROW_THREADS + threadIdx.x; i < 2 * n; i += (int64_t)gridDim.x * ROW_THREADS) {
        const uint32_t c = counts[2 * unique_of[i >> 1] + (uint32_t)(i & 1)];
        lens[i] = c <= (uint32_t)max_sites ? c : 0u;
    }
}

__global__ void __launch_bounds__(ROW_THREADS) oligo_sites_kernel(const uint32_t *__restrict__ unique_of, const uint32_t *__restrict__ counts,
                                                                    const uint32_t *__restrict__ lens, const uint32_t *__restrict__ offsets, int64_t n, int max_sites,
                                                                    RibbitOligoSites *__restrict__ out, ProductHeader *__restrict__ header) {
    for (int64_t i = (int64_t)blockIdx.x * ROW_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * ROW_THREADS) {
        const uint32_t u = unique_of[i], f = counts[2 * u], v = counts[2 * u + 1];
        out[i] = RibbitOligoSites{(int32_t)f, (int32_t)v, f <= (uint32_t)max_sites ? (int32_t)offsets[2 * i] : -1, v <= (uint32_t)max_sites ? (int32_t)offsets[2 * i + 1] : -1};
        if (i == n - 1) header->positions = offsets[2 * i + 1] + lens[2 * i + 1];
    }
}

// a lane per kept list
__global__ void __launch_bounds__(ROW_THREADS) site_gather_kernel(const uint32_t *__restrict__ unique_of, const uint32_t *__restrict__ lens,
                                                                    const uint32_t *__restrict__ offsets, int64_t n, int max_sites, const int32_t *__restrict__ lists,
                                                                    int32_t *__restrict__ flat) {
    for (int64_t i = (int64_t)blockIdx.x * ROW_THREADS + threadIdx.x; i < 2 * n; i += (int64_t)gridDim.x * ROW_THREADS) {
        const int32_t *list = lists + (int64_t)(2 * unique_of[i >> 1] + (uint32_t)(i & 1)) * max_sites;
        for (uint32_t j = 0; j < lens[i]; ++j) flat[offsets[i] + j] = list[j];
    }
}

hipError_t sort_items(void *scratch, size_t &bytes, OligoItem *items, OligoItem *sorted, int64_t n, hipStream_t stream) {
    return rocprim::merge_sort(scratch, bytes, items, sorted, (size_t)n, OligoLess(), stream);
}
hipError_t sum_words(void *scratch, size_t &bytes, const uint32_t *in, uint32_t *out, int64_t n, bool inclusive, hipStream_t stream) {
    return inclusive ? rocprim::inclusive_scan(scratch, bytes, in, out, (size_t)n, rocprim::plus<uint32_t>(), stream)
                     : rocprim::exclusive_scan(scratch, bytes, in, out, 0u, (size_t)n, rocprim::plus<uint32_t>(), stream);
}
hipError_t sort_keys(void *scratch, size_t &bytes, const uint32_t *keys, uint32_t *keys_sorted, const uint32_t *ids, uint32_t *ids_sorted, int64_t n, hipStream_t stream) {
    return rocprim::radix_sort_pairs(scratch, bytes, keys, keys_sorted, ids, ids_sorted, (size_t)n, 0, 32, stream);
}

bool params_fit(const RibbitProductParams &prm) {
    return prm.seed >= 6 && prm.seed <= 16 && prm.max_mismatches >= 0 && prm.max_product >= 1 && prm.max_sites >= 1 && prm.max_sites <= MAX_SITES;
}

}  // namespace

ProductLayout products_layout(int64_t n_oligos, int64_t n_pairs) {
    const size_t n = (size_t)n_oligos;
    size_t a = 0, b = 0, c = 0, d = 0;
    (void)sort_items(nullptr, a, nullptr, nullptr, n_oligos, 0);
    (void)sum_words(nullptr, b, nullptr, nullptr, 2 * n_oligos, true, 0);
    (void)sum_words(nullptr, c, nullptr, nullptr, 2 * n_oligos, false, 0);
    (void)sort_keys(nullptr, d, nullptr, nullptr, nullptr, nullptr, 2 * n_oligos, 0);
    ProductLayout at{};
    WorkCarver w;
    at.items = w.take(2 * n * sizeof(OligoItem));
    at.heads = w.take(2 * n * sizeof(uint32_t));
    at.unique_of = w.take(n * sizeof(uint32_t));
    at.uniques = w.take(n * sizeof(UniqueOligo));
    at.keys = w.take(4 * 2 * n * sizeof(uint32_t));
    at.patterns = w.take(2 * n * sizeof(ProductPattern));
    at.counts = w.take(2 * n * sizeof(uint32_t));
    at.filter = w.take(((size_t)1 << product_filter_log2(n_oligos)) / 8);
    at.lens = w.take(2 * 2 * n * sizeof(uint32_t));
    at.header = w.take(sizeof(ProductHeader));
    at.out = w.take(std::max(n * sizeof(RibbitOligoSites), (size_t)n_pairs * sizeof(RibbitRowProducts)));
    w.close(at, std::max(std::max(a, b), std::max(c, d)));
    return at;
}

hipError_t launch_product_uniques(const RibbitOligo *oligos, int64_t n, const RibbitProductParams &prm, uint8_t *work, size_t work_bytes, const ProductLayout &at,
                                  hipStream_t stream) {
    if (work_bytes < at.bytes || n < 1 || !params_fit(prm)) return hipErrorInvalidValue;
    OligoItem *items = region<OligoItem>(work, at.items), *sorted = items + n;
    uint32_t *head = region<uint32_t>(work, at.heads), *gid = head + n, *unique_of = region<uint32_t>(work, at.unique_of);
    uint32_t *keys = region<uint32_t>(work, at.keys), *ids = keys + 2 * n;
    ProductHeader *header = region<ProductHeader>(work, at.header);
    const dim3 grid(grid_for(n, ROW_THREADS, ROW_MAX_BLOCKS)), block(ROW_THREADS);
    hipError_t e = hipMemsetAsync(header, 0, sizeof(ProductHeader), stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(oligo_items_kernel, grid, block, 0, stream, oligos, n, items);
    size_t bytes = at.scratch_bytes;
    if ((e = sort_items(work + at.scratch, bytes, items, sorted, n, stream)) != hipSuccess) return e;
    hipLaunchKernelGGL(oligo_heads_kernel, grid, block, 0, stream, sorted, n, head);
    bytes = at.scratch_bytes;
    if ((e = sum_words(work + at.scratch, bytes, head, gid, n, true, stream)) != hipSuccess) return e;
    hipLaunchKernelGGL(oligo_uniques_kernel, grid, block, 0, stream, sorted, head, gid, n, (int)prm.seed, unique_of, region<UniqueOligo>(work, at.uniques), keys, ids, header);
    return hipGetLastError();
}

hipError_t launch_product_scan(const DevicePlanes &pl, int64_t n, int64_t uniques, const RibbitProductParams &prm, uint8_t *work, size_t work_bytes, const ProductLayout &at,
                               int32_t *lists, bool use_filter, hipStream_t stream) {
    if (work_bytes < at.bytes || uniques < 1 || uniques > n || !params_fit(prm) || pl.tail_words < 1) return hipErrorInvalidValue;
    const int64_t n_patterns = 2 * uniques;
    uint32_t *keys = region<uint32_t>(work, at.keys), *ids = keys + 2 * n, *keys_sorted = ids + 2 * n, *ids_sorted = keys_sorted + 2 * n;
    ProductPattern *patterns = region<ProductPattern>(work, at.patterns);
    uint32_t *counts = region<uint32_t>(work, at.counts);
    size_t bytes = at.scratch_bytes;
    hipError_t e = sort_keys(work + at.scratch, bytes, keys, keys_sorted, ids, ids_sorted, n_patterns, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(pattern_fill_kernel, dim3(grid_for(n_patterns, ROW_THREADS, ROW_MAX_BLOCKS)), dim3(ROW_THREADS), 0, stream, ids_sorted,
                       region<UniqueOligo>(work, at.uniques), n_patterns, patterns);
    if ((e = hipMemsetAsync(counts, 0, (size_t)n_patterns * sizeof(uint32_t), stream)) != hipSuccess) return e;
    const int filter_log2 = product_filter_log2(n);
    uint32_t *filter = region<uint32_t>(work, at.filter);
    if (use_filter) {
        if ((e = hipMemsetAsync(filter, 0, ((size_t)1 << filter_log2) / 8, stream)) != hipSuccess) return e;
        hipLaunchKernelGGL(filter_fill_kernel, dim3(grid_for(n_patterns, ROW_THREADS, ROW_MAX_BLOCKS)), dim3(ROW_THREADS), 0, stream, keys_sorted, n_patterns, filter_log2, filter);
    }
    hipLaunchKernelGGL(site_scan_kernel, dim3(grid_for(pl.ntiles, SCAN_WAVES, 4 * ROW_MAX_BLOCKS)), dim3(64 * SCAN_WAVES), 0, stream, pl, keys_sorted, patterns,
                       (uint32_t)n_patterns, use_filter ? filter : nullptr, filter_log2, (int)prm.seed, (int)prm.max_mismatches, (int)prm.max_sites, counts, lists);
    hipLaunchKernelGGL(sort_lists_kernel, dim3(grid_for(n_patterns, 1, 8 * ROW_MAX_BLOCKS)), dim3(64), 0, stream, counts, n_patterns, (int)prm.max_sites, lists);
    return hipGetLastError();
}

hipError_t launch_pair_products(const int32_t *pairs, int64_t n_pairs, const RibbitProductParams &prm, uint8_t *work, size_t work_bytes, const ProductLayout &at,
                                const int32_t *lists, hipStream_t stream) {
    if (work_bytes < at.bytes || n_pairs < 1 || !params_fit(prm)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(pair_products_kernel, dim3(grid_for(n_pairs, ROW_THREADS, ROW_MAX_BLOCKS)), dim3(ROW_THREADS), 0, stream, pairs, n_pairs,
                       region<uint32_t>(work, at.unique_of), region<UniqueOligo>(work, at.uniques), region<uint32_t>(work, at.counts), lists, (int)prm.max_product,
                       (int)prm.max_sites, region<RibbitRowProducts>(work, at.out));
    return hipGetLastError();
}

hipError_t launch_oligo_sites(int64_t n, const RibbitProductParams &prm, uint8_t *work, size_t work_bytes, const ProductLayout &at, hipStream_t stream) {
    if (work_bytes < at.bytes || n < 1 || !params_fit(prm)) return hipErrorInvalidValue;
    const uint32_t *unique_of = region<uint32_t>(work, at.unique_of), *counts = region<uint32_t>(work, at.counts);
    uint32_t *lens = region<uint32_t>(work, at.lens), *offsets = lens + 2 * n;
    hipLaunchKernelGGL(site_lens_kernel, dim3(grid_for(2 * n, ROW_THREADS, ROW_MAX_BLOCKS)), dim3(ROW_THREADS), 0, stream, unique_of, counts, n, (int)prm.max_sites, lens);
    size_t bytes = at.scratch_bytes;
    const hipError_t e = sum_words(work + at.scratch, bytes, lens, offsets, 2 * n, false, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(oligo_sites_kernel, dim3(grid_for(n, ROW_THREADS, ROW_MAX_BLOCKS)), dim3(ROW_THREADS), 0, stream, unique_of, counts, lens, offsets, n,
                       (int)prm.max_sites, region<RibbitOligoSites>(work, at.out), region<ProductHeader>(work, at.header));
    return hipGetLastError();
}

void launch_site_gather(int64_t n, const RibbitProductParams &prm, uint8_t *work, const ProductLayout &at, const int32_t *lists, int32_t *flat, hipStream_t stream) {
    const uint32_t *lens = region<uint32_t>(work, at.lens);
    hipLaunchKernelGGL(site_gather_kernel, dim3(grid_for(2 * n, ROW_THREADS, ROW_MAX_BLOCKS)), dim3(ROW_THREADS), 0, stream, region<uint32_t>(work, at.unique_of), lens,
                       lens + 2 * n, n, (int)prm.max_sites, lists, flat);
}

}  // namespace rb
