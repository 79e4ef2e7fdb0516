// amplicons.hip -- every primer pair typed on the loaded record: where its first product lies and how long the repeat tract
// inside it is (api_amplicons.cpp: ribbit_hip_record_pair_amplicons; include/ribbit_hip.h has the contract, kernels.h the order of
// the launches).  The sites come from primer_products.hip's site search (kernels.h, at ProductLayout); two kernels follow it.
//   first product   One lane per pair over its four sorted lists: product_walk.h's pair_products for the counts (no product is the
//                   pair's own), and first_product for the least (f.x, v.x + v.k, forward_of, reverse_of).
//   tract           One wavefront per pair with a product, four to a block, no LDS and no barrier.  The motif's two strands are
//                   packed into plane form with ballots, word j kept by lane j (1023 letters are 32 words).  The inner part is
//                   walked 64 words at a time, a word per lane: ok = ~((hi ^ hi_m) | (lo ^ lo_m) | brk | brk_m), the _m planes
//                   being the planes m bases back, a word offset of m / 32 and a funnel of m % 32.  A run of ok ends where a
//                   zero follows a one; the zero before it is in the lane's own word, or the maximum of the earlier lanes' last
//                   zeros (an inclusive scan by shuffles), or carried over from the words before.  The longest run of the 64
//                   words that would beat the tract held (a wave maximum of length << 32 | ~start: the leftmost of equals) is
//                   judged: its first m letters against every rotation of w and of revcomp(w), a lane per rotation, 32 letters per
//                   XOR, the motif's words broadcast by shuffles.  A run that fails is set aside and the next longest judged.
// Integer vector operations only; no inline assembly.
#include <hip/hip_runtime.h>

#include "product_walk.h"

namespace rb {

namespace {

constexpr int TRACT_WAVES = 4;
static_assert(sizeof(RibbitRowAmplicon) == 64, "16 ints");

__device__ inline uint32_t low_bits(int k) { return k >= 32 ? 0xffffffffu : (1u << k) - 1u; }
// bits sh .. sh + 31 of hi : lo, 0 <= sh <= 31
__device__ inline uint32_t funnel(uint32_t lo, uint32_t hi, int sh) { return (uint32_t)((((unsigned long long)hi << 32) | lo) >> sh); }
// A 0, C 1, G 2, T 3 of an upper-case letter
__device__ inline uint32_t code_of(uint8_t c) {
    const uint32_t x = (c >> 1) & 3u;
    return x ^ (x >> 1);
}

__device__ inline RibbitRowAmplicon no_amplicon() {
    RibbitRowAmplicon a = {};
    a.record = a.start = a.end = a.inner_start = a.inner_end = a.tract_start = a.tract_end = -1;
    return a;
}

__global__ void __launch_bounds__(ROW_THREADS) pair_amplicons_kernel(const int32_t *__restrict__ pairs, int64_t n_pairs, const uint32_t *__restrict__ unique_of,
                                                                       const UniqueOligo *__restrict__ uniques, const uint32_t *__restrict__ counts,
                                                                       const int32_t *__restrict__ lists, int max_product, int max_sites, int32_t record,
                                                                       RibbitRowAmplicon *__restrict__ out) {
    for (int64_t i = (int64_t)blockIdx.x * ROW_THREADS + threadIdx.x; i < n_pairs; i += (int64_t)gridDim.x * ROW_THREADS) {
        const int32_t ia = pairs[4 * i], ib = pairs[4 * i + 1];
        RibbitRowAmplicon a = no_amplicon();
        if (ia >= 0) {
            const uint32_t ua = unique_of[ia], ub = unique_of[ib];
            const RibbitRowProducts r = pair_products(ua, ub, -1, -1, uniques, counts, lists, max_product, max_sites);
            a.left_forward = r.left_forward;
            a.left_reverse = r.left_reverse;
            a.right_forward = r.right_forward;
            a.right_reverse = r.right_reverse;
            a.products = r.products;
            if (r.products > 0) {
                const FirstProduct p = first_product(ua, ub, uniques, counts, lists, max_product, max_sites);
                a.record = record;
                a.start = p.start;
                a.end = p.end;
                a.forward_of = p.forward_of;
                a.reverse_of = p.reverse_of;
                a.inner_start = p.inner_start;
                a.inner_end = p.inner_end;
            }
        }
        out[i] = a;
    }
}

// ---- the tract
__device__ inline unsigned long long wave_max(unsigned long long v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v = max(v, __shfl_xor(v, d));
    return v;      // (every lane's)
}

// Whether the m letters at `start` are a rotation of the motif on strand 0 (-> 0), else on strand 1 (-> 1), else -1.  The 2 m
// letters from `start` on are periodic bases, so rotation p of the motif is the motif itself at start + p.  Every lane of the
// wavefront calls it with the same arguments; m0h .. m1l: word `lane` of the two strands' planes.
__device__ inline int tract_strand(const DevicePlanes &pl, int64_t start, int m, uint32_t m0h, uint32_t m0l, uint32_t m1h, uint32_t m1l, int lane) {
    bool fits0 = false, fits1 = false;
    for (int p0 = 0; p0 < m; p0 += 64) {
        const bool live = p0 + lane < m;
        const int64_t at = start + (live ? p0 + lane : 0);
        uint32_t d0 = 0, d1 = 0;
        for (int j = 0; 32 * j < m; ++j) {
            const uint32_t w0h = (uint32_t)__shfl((int)m0h, j), w0l = (uint32_t)__shfl((int)m0l, j);
            const uint32_t w1h = (uint32_t)__shfl((int)m1h, j), w1l = (uint32_t)__shfl((int)m1l, j);
            const int64_t bit = at + 32 * j, w = bit >> 5;      // (w + 1 is at most two words behind the tract: inside the tail)
            const int sh = (int)(bit & 31);
            const uint32_t rh = funnel(pl.hi[w], pl.hi[w + 1], sh), rl = funnel(pl.lo[w], pl.lo[w + 1], sh);
            const uint32_t mask = low_bits(m - 32 * j);
            d0 |= ((rh ^ w0h) | (rl ^ w0l)) & mask;
            d1 |= ((rh ^ w1h) | (rl ^ w1l)) & mask;
        }
        fits0 = fits0 || (live && d0 == 0u);
        fits1 = fits1 || (live && d1 == 0u);
    }
    return __any(fits0) ? 0 : __any(fits1) ? 1 : -1;
}

__global__ void __launch_bounds__(64 * TRACT_WAVES) amplicon_tracts_kernel(DevicePlanes pl, const uint8_t *__restrict__ pool, const int32_t *__restrict__ offsets,
                                                                           int64_t n_pairs, RibbitRowAmplicon *__restrict__ rows) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int64_t i = (int64_t)blockIdx.x * TRACT_WAVES + wave; i < n_pairs; i += (int64_t)gridDim.x * TRACT_WAVES) {
        // (everything up to the word loop is the same in all 64 lanes)
        if (rows[i].products <= 0) continue;
        const int64_t is = rows[i].inner_start, ie = rows[i].inner_end;
        const int m = offsets[i + 1] - offsets[i];
        if (ie - is < 2 * (int64_t)m) continue;
        const uint8_t *w = pool + (offsets[i] - offsets[0]);
        // the motif (strand 0) and its reverse complement (strand 1) in plane form: 64 letters per ballot, word j to lane j
        uint32_t m0h = 0, m0l = 0, m1h = 0, m1l = 0;
        for (int c = 0; 64 * c < m; ++c) {
            const int j = 64 * c + lane;
            const uint32_t c0 = j < m ? code_of(w[j]) : 0u, c1 = j < m ? 3u - code_of(w[m - 1 - j]) : 0u;
            const unsigned long long h0 = __ballot(c0 & 2u), l0 = __ballot(c0 & 1u), h1 = __ballot(c1 & 2u), l1 = __ballot(c1 & 1u);
            if (lane == 2 * c) { m0h = (uint32_t)h0; m0l = (uint32_t)l0; m1h = (uint32_t)h1; m1l = (uint32_t)l1; }
            if (lane == 2 * c + 1) { m0h = (uint32_t)(h0 >> 32); m0l = (uint32_t)(l0 >> 32); m1h = (uint32_t)(h1 >> 32); m1l = (uint32_t)(l1 >> 32); }
        }
        // ok[x] is defined for from <= x < ie; the position before `from` counts as a zero, and so does ie
        const int64_t from = is + m, w_first = from >> 5, w_last = ie >> 5;
        const int q = m >> 5, r = m & 31;
        int64_t carry_zero = from - 1;      // the last position so far that is no ok
        uint32_t carry_top = 0;             // ok of the last position of the word before
        int64_t best_start = -1;
        uint32_t best_len = 2u * (uint32_t)m - 1u;      // (a tract has 2 m bases at least)
        int best_strand = 0;
        for (int64_t wb = w_first; wb <= w_last; wb += 64) {
            const int64_t W = wb + lane, lo_pos = W * 32;
            uint32_t okw = 0;
            if (W <= w_last) {
                const uint32_t h = pl.hi[W], l = pl.lo[W], b = pl.brk[W];
                // the planes m bases back (W - q - 1 >= -1: the lead padding)
                const int64_t Wm = W - q;
                const uint32_t hm = r ? funnel(pl.hi[Wm - 1], pl.hi[Wm], 32 - r) : pl.hi[Wm];
                const uint32_t lm = r ? funnel(pl.lo[Wm - 1], pl.lo[Wm], 32 - r) : pl.lo[Wm];
                const uint32_t bm = r ? funnel(pl.brk[Wm - 1], pl.brk[Wm], 32 - r) : pl.brk[Wm];
                okw = ~((h ^ hm) | (l ^ lm) | b | bm);
                if (lo_pos < from) okw &= ~low_bits((int)(from - lo_pos));
                if (lo_pos + 32 > ie) okw &= low_bits((int)(ie - lo_pos));
            }
            // where a run ends: a zero behind a one
            const uint32_t top = okw >> 31;
            uint32_t before = (uint32_t)__shfl_up((int)top, 1);
            if (lane == 0) before = carry_top;
            const uint32_t fall = ~okw & ((okw << 1) | before);
            // the last zero before this lane's word
            const int64_t own_zero = ~okw ? lo_pos + 31 - __clz((int)~okw) : -1;
            int64_t upto = own_zero;      // (inclusive maximum over the lanes up to this one)
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const int64_t other = __shfl_up(upto, d);
                if (lane >= d) upto = max(upto, other);
            }
            int64_t zero_before = __shfl_up(upto, 1);
            zero_before = lane == 0 ? carry_zero : max(zero_before, carry_zero);
            carry_zero = max(carry_zero, __shfl(upto, 63));
            carry_top = (uint32_t)__shfl((int)top, 63);
            // the runs that end in this lane's word, longest first, until one is a tract or none is left that would beat the one held
            unsigned long long limit = ~0ull;
            for (;;) {
                unsigned long long mine = 0;
                for (uint32_t f = fall; f; f &= f - 1u) {
                    const int b = __ffs((int)f) - 1;
                    const uint32_t zeros_below = ~okw & low_bits(b);
                    const int64_t u = (zeros_below ? lo_pos + 31 - __clz((int)zeros_below) : zero_before) + 1, run = lo_pos + b - u;
                    if (run < m) continue;
                    const unsigned long long key = (unsigned long long)(run + m) << 32 | (0xffffffffu - (uint32_t)(u - m));
                    if ((uint32_t)(run + m) > best_len && key < limit && key > mine) mine = key;
                }
                const unsigned long long longest = wave_max(mine);
                if (longest == 0) break;
                const int64_t start = (int64_t)(0xffffffffu - (uint32_t)longest);
                const int strand = tract_strand(pl, start, m, m0h, m0l, m1h, m1l, lane);
                if (strand >= 0) {
                    best_start = start;
                    best_len = (uint32_t)(longest >> 32);
                    best_strand = strand;
                    break;      // (the others of these words are no longer, and lie behind it)
                }
                if (mine == longest) limit = longest;
            }
        }
        if (lane == 0 && best_start >= 0) {
            rows[i].tract_start = (int32_t)best_start;
            rows[i].tract_end = (int32_t)(best_start + best_len);
            rows[i].tract_strand = best_strand;
        }
    }
}

}  // namespace

AmpliconLayout amplicon_layout(int64_t n_pairs) {
    AmpliconLayout at{};
    WorkCarver w;
    at.rows = w.take((size_t)n_pairs * sizeof(RibbitRowAmplicon));
    at.sites = site_room(w, 2 * n_pairs);
    w.close(at, 0);
    return at;
}

hipError_t launch_pair_amplicons(const DevicePlanes &pl, const int32_t *pairs, int64_t n_pairs, const uint8_t *pool, const int32_t *offsets, int32_t record,
                                 const RibbitProductParams &prm, uint8_t *work, size_t work_bytes, const AmpliconLayout &at, const int32_t *site_lists,
                                 hipStream_t stream) {
    if (work_bytes < at.bytes || n_pairs < 1 || prm.max_product < 1 || prm.max_sites < 1 || record < 0 || pl.tail_words < 2) return hipErrorInvalidValue;
    uint8_t *pw = work + at.sites.offset;
    RibbitRowAmplicon *rows = region<RibbitRowAmplicon>(work, at.rows);
    hipLaunchKernelGGL(pair_amplicons_kernel, dim3(grid_for(n_pairs, ROW_THREADS, ROW_MAX_BLOCKS)), dim3(ROW_THREADS), 0, stream, pairs, n_pairs,
                       region<uint32_t>(pw, at.sites.layout.unique_of), region<UniqueOligo>(pw, at.sites.layout.uniques), region<uint32_t>(pw, at.sites.layout.counts), site_lists,
                       (int)prm.max_product, (int)prm.max_sites, record, rows);
    hipLaunchKernelGGL(amplicon_tracts_kernel, dim3(grid_for(n_pairs, TRACT_WAVES, 4 * ROW_MAX_BLOCKS)), dim3(64 * TRACT_WAVES), 0, stream, pl, pool, offsets, n_pairs, rows);
    return hipGetLastError();
}

}  // namespace rb
