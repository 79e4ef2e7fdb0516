// primers.hip -- a forward primer in the left flank and a reverse primer in the right flank of every target of the loaded record
// (api_primers.cpp: ribbit_hip_record_primers; include/ribbit_hip.h has the contract).  Nothing here reads the ASCII: a base's
// 2-bit code is 2 hi + lo of the scan's own bit planes (device_planes.h: A 0, C 1, G 2, T 3), `other` is brk, and the rows'
// coverage is the mask's bitmap (build_coverage); bit p & 31 of word p >> 5 in all four, as composition.hip reads them.
// One wavefront per (target, side), PRIMER_WAVES of them to a workgroup, each with its own slice of LDS for a window of up to
// `cap` bases (the flank); the wavefronts of a workgroup never wait for each other (no __syncthreads):
//   stage:    the window's words of hi, lo, brk and the bitmap into LDS, one word per lane and turn (a window of W bases spans at
//             most W / 32 + 2 words, and every position of a window is below L, so every word read holds positions)
//   expand:   one byte per position, code | blocked << 2
//   prefixes: per chunk of 64 positions a wave scan (__shfl_up) with the chunk before as carry: the inclusive sums of the steps'
//             dH and dS (step i is the pair of positions i - 1, i), and the exclusive counts of C + G, of blocked positions and
//             of positions where a run of max_run + 1 equal bases ends, packed 10 bits each in one word (a window has at most
//             1000 < 1024 positions, and every count only grows, so packed words subtract field by field without a borrow)
//   search:   a lane takes the starts p = lane, lane + 64, ... and every length k for each: five prefix differences, two terminal
//             look-ups, one 32-bit division.  A blocked base or a run ends the lengths of a start, since every longer candidate
//             holds it too.  The lane keeps the least key penalty << 32 | distance << 8 | k and counts the admissible ones
//   result:   the wave's least key (__shfl_xor) and the sum of the counts (wave_sum); lane 0 takes start and Tm from the key
//             again and reads the candidate's bases from LDS
// A run flag at position i looks back at most 31 positions: a candidate has at most RIBBIT_PRIMER_MAX_LENGTH = 32 bases, so
// with max_run >= 32 no run of max_run + 1 fits into one and no flag is set.  The flags of a candidate [p, p + k) are those at
// p + max_run .. p + k - 1, whose look-back stays inside it.
// LDS: 3 words and a byte per position, 13.5 KB per wavefront at the largest flank, 54 KB per workgroup: two workgroups fit a
// CU's 160 KB there, and at the default flank of 200 (2.7 KB per wavefront) the wavefronts' registers are what limits them.
// The kernel strides beyond ROW_MAX_BLOCKS blocks.
#include <hip/hip_runtime.h>

#include "row_kernels.h"

namespace rb {

namespace {

constexpr int PRIMER_WAVES = 4;
constexpr int PRIMER_THREADS = 64 * PRIMER_WAVES;
static_assert(PRIMER_THREADS == ROW_THREADS, "the launch shape of the row outputs");
static_assert(RIBBIT_PRIMER_MAX_FLANK < 1024 && RIBBIT_PRIMER_MAX_LENGTH <= 32, "three 10-bit counts in a word; a candidate's bases in 64 bits");
static_assert(sizeof(RibbitRowPrimers) == 56 && sizeof(RibbitPrimer) == 24, "14 ints");

// SantaLucia 1998, dH in 100 cal/mol and dS in 0.1 cal/(K mol), step a b at 4 a + b
__constant__ int32_t NN_H[16] = {-79, -84, -78, -72, -85, -80, -106, -78, -82, -98, -80, -84, -72, -82, -85, -79};
__constant__ int32_t NN_S[16] = {-222, -224, -210, -204, -227, -199, -272, -210, -222, -244, -199, -224, -213, -222, -227, -222};

constexpr uint32_t GC_ONE = 1u, BLOCKED_ONE = 1u << 10, RUN_ONE = 1u << 20, FIELD = 1023u;
constexpr unsigned long long NO_KEY = ~0ull;

// the words of LDS a wavefront takes for windows of up to cap bases
__host__ __device__ inline int window_words(int cap) { return cap / 32 + 2; }
__host__ __device__ inline int wave_lds_words(int cap) { return cap + cap + (cap + 1) + 4 * window_words(cap) + (cap + 3) / 4; }

// what one wavefront writes is read by its other lanes: LDS operations of a wavefront complete in order, the compiler must keep them so
__device__ inline void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

__device__ inline bool is_gc(uint32_t code) { return code == 1u || code == 2u; }

struct Window {
    const int32_t *sh, *ss;      // inclusive step sums up to position i
    const uint32_t *cnt;         // packed exclusive counts before position i, 0 .. n
    const uint8_t *code;
};

// Tm of the unblocked candidate [p, p + k) of the window, k >= 2, in tenths of a degree
__device__ inline int32_t melting(const Window &w, int p, int k) {
    const uint32_t first = w.code[p] & 3u, last = w.code[p + k - 1] & 3u;
    int32_t h = w.sh[p + k - 1] - w.sh[p], s = w.ss[p + k - 1] - w.ss[p] - 11 * (k - 1) - 362;
    h += (is_gc(first) ? 1 : 23) + (is_gc(last) ? 1 : 23);
    s += (is_gc(first) ? -28 : 41) + (is_gc(last) ? -28 : 41);
    return (int32_t)((uint32_t)(-h * 10000) / (uint32_t)(-s)) - 2732;      // (both sums are negative)
}

__global__ void __launch_bounds__(PRIMER_THREADS) primers_kernel(const int32_t *__restrict__ targets, int64_t n_targets, DevicePlanes pl, const uint32_t *__restrict__ bits,
                                                                RibbitPrimerParams prm, int cap, RibbitRowPrimers *__restrict__ out) {
    extern __shared__ uint32_t lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nw = window_words(cap);
    int32_t *sh = reinterpret_cast<int32_t *>(lds + (size_t)wave * wave_lds_words(cap)), *ss = sh + cap;
    uint32_t *cnt = reinterpret_cast<uint32_t *>(ss + cap), *words = cnt + cap + 1;
    uint8_t *code = reinterpret_cast<uint8_t *>(words + 4 * nw);
    const Window win{sh, ss, cnt, code};
    const int64_t length = pl.length, items = 2 * n_targets;
    const int look_back = prm.max_run < 32 ? prm.max_run : 0;      // (0: no run fits a candidate)
    for (int64_t item = (int64_t)blockIdx.x * PRIMER_WAVES + wave; item < items; item += (int64_t)gridDim.x * PRIMER_WAVES) {
        const int64_t t = item >> 1;
        const bool right = item & 1;
        const int64_t s = min(max((int64_t)targets[2 * t], (int64_t)0), length), e = min(max((int64_t)targets[2 * t + 1], s), length);
        const int64_t from = right ? e : max(s - (int64_t)prm.flank, (int64_t)0), to = right ? min(e + (int64_t)prm.flank, length) : s;
        const int n = (int)(to - from);      // 0 .. flank <= cap
        // stage
        const int64_t w0 = from >> 5;
        const int n_words = n > 0 ? (int)(((to - 1) >> 5) - w0) + 1 : 0;      // <= nw
        for (int j = lane; j < 4 * n_words; j += 64) {
            const int plane = j / n_words, at = j - plane * n_words;
            const uint32_t *src = plane == 0 ? pl.hi : plane == 1 ? pl.lo : plane == 2 ? pl.brk : bits;
            words[plane * nw + at] = src[w0 + at];
        }
        wave_sync();
        // expand
        for (int i = lane; i < n; i += 64) {
            const int64_t p = from + i;
            const int at = (int)((p >> 5) - w0), bit = (int)(p & 31);
            const uint32_t h = (words[at] >> bit) & 1u, l = (words[nw + at] >> bit) & 1u, blocked = ((words[2 * nw + at] | words[3 * nw + at]) >> bit) & 1u;
            code[i] = (uint8_t)(2u * h + l + 4u * blocked);
        }
        if (lane == 0) cnt[0] = 0;
        wave_sync();
        // prefixes
        int32_t carry_h = 0, carry_s = 0;
        uint32_t carry_c = 0;
        for (int base = 0; base < n; base += 64) {
            const int i = base + lane;
            const bool valid = i < n;
            int32_t vh = 0, vs = 0;
            uint32_t vc = 0;
            if (valid) {
                const uint32_t c = code[i], cd = c & 3u;
                if (i > 0) {
                    const uint32_t step = 4u * (code[i - 1] & 3u) + cd;
                    vh = NN_H[step];
                    vs = NN_S[step];
                }
                bool run = look_back > 0 && i >= look_back;
                for (int j = 1; run && j <= look_back; ++j) run = (code[i - j] & 3u) == cd;
                vc = (is_gc(cd) ? GC_ONE : 0u) + ((c >> 2) ? BLOCKED_ONE : 0u) + (run ? RUN_ONE : 0u);
            }
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const int32_t uh = __shfl_up(vh, d), us = __shfl_up(vs, d);
                const uint32_t uc = __shfl_up(vc, d);
                if (lane >= d) { vh += uh; vs += us; vc += uc; }
            }
            vh += carry_h;
            vs += carry_s;
            vc += carry_c;
            if (valid) {
                sh[i] = vh;
                ss[i] = vs;
                cnt[i + 1] = vc;
            }
            carry_h = __shfl(vh, 63);
            carry_s = __shfl(vs, 63);
            carry_c = __shfl(vc, 63);
        }
        wave_sync();
        // search
        unsigned long long best = NO_KEY;
        uint32_t found = 0;
        for (int p = lane; p + prm.min_length <= n; p += 64) {
            const uint32_t before = cnt[p], first = code[p] & 3u;
            for (int k = prm.min_length; k <= prm.max_length && p + k <= n; ++k) {
                const uint32_t upto = cnt[p + k], in = upto - before;
                if ((in >> 10) & FIELD) break;                                                    // (1)
                if (k > prm.max_run && ((upto - cnt[p + prm.max_run]) >> 20)) break;              // (3)
                const int32_t g = (int32_t)(in & FIELD);
                if (100 * g < prm.gc_min_percent * k || 100 * g > prm.gc_max_percent * k) continue;      // (2)
                if (prm.gc_clamp && !is_gc(right ? first : code[p + k - 1] & 3u)) continue;       // (4)
                const int32_t tm = melting(win, p, k);
                if (tm < prm.tm_min || tm > prm.tm_max) continue;                                 // (5)
                ++found;
                const uint32_t penalty = (uint32_t)(abs(tm - prm.tm_opt) + 10 * abs(k - prm.opt_length)), distance = (uint32_t)(right ? p : n - (p + k));
                const unsigned long long key = (unsigned long long)penalty << 32 | distance << 8 | (uint32_t)k;
                best = key < best ? key : best;
            }
        }
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) {
            const unsigned long long other = __shfl_xor(best, d);
            best = other < best ? other : best;
        }
        const unsigned long long total = wave_sum(found);
        if (lane == 0) {
            RibbitPrimer r{-1, 0, 0, 0, 0, 0};
            if (best != NO_KEY) {
                const int k = (int)(best & 255u), distance = (int)((best >> 8) & 0xffffffu), p = right ? distance : n - distance - k;
                unsigned long long bases = 0;
                for (int j = 0; j < k; ++j) bases |= (unsigned long long)(code[p + j] & 3u) << (2 * j);
                r.start = (int32_t)(from + p);
                r.length = k;
                r.tm = melting(win, p, k);
                r.penalty = (int32_t)(best >> 32);
                r.bases_lo = (int32_t)(uint32_t)bases;
                r.bases_hi = (int32_t)(uint32_t)(bases >> 32);
            }
            if (right) {
                out[t].right = r;
                out[t].right_candidates = (int32_t)total;
            } else {
                out[t].left = r;
                out[t].left_candidates = (int32_t)total;
            }
        }
        wave_sync();      // (the next window is staged over this one)
    }
}

}  // namespace

PrimerLayout primers_layout(int64_t n_targets) {
    PrimerLayout at{};
    WorkCarver w;
    at.out = w.take((size_t)n_targets * sizeof(RibbitRowPrimers));
    w.close(at, 0);
    return at;
}

hipError_t launch_primers(const DevicePlanes &pl, const uint32_t *bits, const int32_t *targets, int64_t n_targets, const RibbitPrimerParams &prm, uint8_t *work,
                          size_t work_bytes, const PrimerLayout &at, hipStream_t stream) {
    if (work_bytes < at.bytes || prm.flank < 0 || prm.flank > RIBBIT_PRIMER_MAX_FLANK || prm.min_length < 2 || prm.max_length > RIBBIT_PRIMER_MAX_LENGTH) return hipErrorInvalidValue;
    const int cap = std::max(prm.flank, 1);
    const size_t lds_bytes = (size_t)PRIMER_WAVES * wave_lds_words(cap) * sizeof(uint32_t);      // 54 KB at most
    hipLaunchKernelGGL(primers_kernel, dim3(grid_for(2 * n_targets, PRIMER_WAVES, ROW_MAX_BLOCKS)), dim3(PRIMER_THREADS), lds_bytes, stream, targets, n_targets, pl,
                       bits, prm, cap, region<RibbitRowPrimers>(work, at.out));
    return hipGetLastError();
}

}  // namespace rb
