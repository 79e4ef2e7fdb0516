// primer_window.h -- the front end that primers.hip, primer_pairs.hip and primer_specific.hip share: one wavefront brings a window of up to `cap`
// bases of the loaded record into its own slice of LDS and makes the prefixes every candidate of the window is judged from
// (include/ribbit_hip.h has the contract).  Nothing here reads the ASCII: a base's 2-bit code is 2 hi + lo of the scan's own bit
// planes (device_planes.h: A 0, C 1, G 2, T 3), `other` is brk, and the rows' coverage is the mask's bitmap (build_coverage); bit
// p & 31 of word p >> 5 in all four, as composition.hip reads them.
//   stage:    the window's words of hi, lo, brk and the bitmap into LDS, one word per lane and turn (a window of W bases spans at
//             most W / 32 + 2 words, and every position of a window is below L, so every word read holds positions)
//   expand:   one byte per position, code | blocked << 2
//   prefixes: per chunk of 64 positions a wave scan (__shfl_up) with the chunk before as carry: the inclusive sums of the steps'
//             dH and dS (step i is the pair of positions i - 1, i), and the exclusive counts of C + G, of blocked positions and
//             of positions where a run of max_run + 1 equal bases ends, packed 10 bits each in one word (a window has at most
//             1000 < 1024 positions, and every count only grows, so packed words subtract field by field without a borrow)
//   judge:    a candidate [p, p + k) from five prefix differences, two terminal look-ups and one 32-bit division.  A blocked base
//             or a run ends the lengths of a start, since every longer candidate holds it too.
// A run flag at position i looks back at most 31 positions: a candidate has at most RIBBIT_PRIMER_MAX_LENGTH = 32 bases, so
// with max_run >= 32 no run of max_run + 1 fits into one and no flag is set.  The flags of a candidate [p, p + k) are those at
// p + max_run .. p + k - 1, whose look-back stays inside it.
// The wavefronts of a workgroup never wait for each other (no __syncthreads).  Included by those .hip files only (the latter two through primer_shortlist.h).
#pragma once
#include <hip/hip_runtime.h>

#include "row_kernels.h"

namespace rb {

namespace {

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
    int32_t *sh, *ss;      // inclusive step sums up to position i
    uint32_t *cnt;         // packed exclusive counts before position i, 0 .. n
    uint32_t *words;       // the staged words, four planes of window_words(cap) each
    uint8_t *code;
};

// a wavefront's slice, wave_lds_words(cap) words from `base`
__device__ inline Window window_at(uint32_t *base, int cap) {
    Window w;
    w.sh = reinterpret_cast<int32_t *>(base);
    w.ss = w.sh + cap;
    w.cnt = reinterpret_cast<uint32_t *>(w.ss + cap);
    w.words = w.cnt + cap + 1;
    w.code = reinterpret_cast<uint8_t *>(w.words + 4 * window_words(cap));
    return w;
}

// Tm of the unblocked candidate [p, p + k) of the window, k >= 2, in tenths of a degree
__device__ inline int32_t melting(const Window &w, int p, int k) {
    const uint32_t first = w.code[p] & 3u, last = w.code[p + k - 1] & 3u;
    int32_t h = w.sh[p + k - 1] - w.sh[p], s = w.ss[p + k - 1] - w.ss[p] - 11 * (k - 1) - 362;
    h += (is_gc(first) ? 1 : 23) + (is_gc(last) ? 1 : 23);
    s += (is_gc(first) ? -28 : 41) + (is_gc(last) ? -28 : 41);
    return (int32_t)((uint32_t)(-h * 10000) / (uint32_t)(-s)) - 2732;      // (both sums are negative)
}

// the look-back of the run flags (0: no run fits a candidate)
__device__ inline int run_look_back(const RibbitPrimerParams &prm) { return prm.max_run < 32 ? prm.max_run : 0; }

// stage, expand, prefixes: the positions [from, from + n) of the record, 0 <= n <= cap, into the wavefront's slice
__device__ inline void fill_window(const Window &w, int cap, const DevicePlanes &pl, const uint32_t *__restrict__ bits, int64_t from, int n, int look_back, int lane) {
    const int nw = window_words(cap);
    uint32_t *words = w.words;
    uint8_t *code = w.code;
    const int64_t to = from + n;
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
    if (lane == 0) w.cnt[0] = 0;
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
            w.sh[i] = vh;
            w.ss[i] = vs;
            w.cnt[i + 1] = vc;
        }
        carry_h = __shfl(vh, 63);
        carry_s = __shfl(vs, 63);
        carry_c = __shfl(vc, 63);
    }
    wave_sync();
}

// the verdict on the candidate [p, p + k) of a window of n positions, p + k <= n, min_length <= k: STOP when no longer candidate
// of this start can be admissible either (rules 1 and 3), SKIP when this one is not (2, 4, 5), else TAKE with its Tm
enum Verdict { STOP, SKIP, TAKE };
__device__ inline Verdict judge(const Window &w, const RibbitPrimerParams &prm, bool right, int p, int k, uint32_t before, uint32_t first, int32_t &tm) {
    const uint32_t upto = w.cnt[p + k], in = upto - before;
    if ((in >> 10) & FIELD) return STOP;                                                    // (1)
    if (k > prm.max_run && ((upto - w.cnt[p + prm.max_run]) >> 20)) return STOP;            // (3)
    const int32_t g = (int32_t)(in & FIELD);
    if (100 * g < prm.gc_min_percent * k || 100 * g > prm.gc_max_percent * k) return SKIP;      // (2)
    if (prm.gc_clamp && !is_gc(right ? first : w.code[p + k - 1] & 3u)) return SKIP;        // (4)
    tm = melting(w, p, k);
    if (tm < prm.tm_min || tm > prm.tm_max) return SKIP;                                    // (5)
    return TAKE;
}

// a candidate's key in the order of the choice, (penalty, distance, k), and the three again from a key
__device__ inline unsigned long long candidate_key(const RibbitPrimerParams &prm, bool right, int p, int k, int n, int32_t tm) {
    const uint32_t penalty = (uint32_t)(abs(tm - prm.tm_opt) + 10 * abs(k - prm.opt_length)), distance = (uint32_t)(right ? p : n - (p + k));
    return (unsigned long long)penalty << 32 | distance << 8 | (uint32_t)k;
}

// the record of the candidate a key names: its start and Tm from the key again, its bases from LDS
__device__ inline RibbitPrimer primer_of(const Window &w, unsigned long long key, bool right, int64_t from, int n) {
    const int k = (int)(key & 255u), distance = (int)((key >> 8) & 0xffffffu), p = right ? distance : n - distance - k;
    unsigned long long bases = 0;
    for (int j = 0; j < k; ++j) bases |= (unsigned long long)(w.code[p + j] & 3u) << (2 * j);
    RibbitPrimer r;
    r.start = (int32_t)(from + p);
    r.length = k;
    r.tm = melting(w, p, k);
    r.penalty = (int32_t)(key >> 32);
    r.bases_lo = (int32_t)(uint32_t)bases;
    r.bases_hi = (int32_t)(uint32_t)(bases >> 32);
    return r;
}

__device__ inline unsigned long long wave_min(unsigned long long v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        const unsigned long long other = __shfl_xor(v, d);
        v = other < v ? other : v;
    }
    return v;
}

}  // namespace

}  // namespace rb
