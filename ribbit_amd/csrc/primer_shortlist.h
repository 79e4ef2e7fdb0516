// primer_shortlist.h -- what primer_pairs.hip and primer_specific.hip share on top of primer_window.h: an oligo as 64 bits and the
// ungapped duplex of two of them, and one side of a target from its window to its shortlist in LDS (include/ribbit_hip.h has
// the contract, steps (1) and (2) of the selection).
// An oligo is its bases 5' to 3', two bits each, base i at bits 2 i of 64: a left candidate's bases as they stand, a right
// candidate's reversed (a bit reversal with the two bits of each base swapped back), complemented and shifted down.  A placement
// of a against b is one shift of b's reversed bases and one XOR: x = a ^ shifted, m = x & (x >> 1) & 0x5555..., bit 2 i of m set
// where a[i] is bonded.  "m holds a run of n" is at most six AND-shift steps (has_run); a run through a 3' base is the leading or
// the trailing ones of m there (count leading / trailing zeros of its complement).  Only a chosen pair's five values take the
// run lengths themselves (longest_run, a loop).
//   shortlist_side:
//     pass 1    a lane takes the starts p = lane, lane + 64, ... and keeps the admissible lengths of each by the five rules
//               as a bit set, one word per start in LDS (bit k - 1).  Then the wavefront walks the starts that have any,
//               one candidate at a time, WITH A LANE PER PLACEMENT: the oligo of k bases against itself has 2 k - 1 <= 63
//               placements, every lane tests its own against the three self limits, and one __any says whether the
//               candidate passes.  Lane 0 writes the start's word back with the passing lengths only.
//     shortlist `shortlist` rounds, each a wave minimum of the keys (penalty, distance, k) of the flagged candidates that
//               are greater than the last winner (no two candidates share a key); lane r keeps round r's key and writes
//               its RibbitPrimer to the side's shortlist in LDS.  No sorted per-lane lists, no indexed registers.
// A lane per candidate in pass 1 (a first version) left the wavefront waiting for its busiest lane: the admissible candidates are
// few (some 65 a side at the defaults) and come in clusters of neighbouring lengths of one start.  A lane per placement keeps
// 35 .. 49 of 64 lanes busy for every candidate and needs no balancing.
// LDS per wavefront: the window's 3 words and a byte per position, a word per start, 96 words of shortlists: 3.9 KB at the
// default flank of 200, 17.9 KB at 1000.  A workgroup has 4 wavefronts, or 2 where 4 would take more than 64 KB.
// Included by those two .hip files, and by panel.hip for the oligo and the duplex alone.
#pragma once
#include <hip/hip_runtime.h>

#include "primer_window.h"

namespace rb {

namespace {

constexpr int PAIR_WAVES = 4;
constexpr int SHORTLIST = RIBBIT_PRIMER_PAIR_SHORTLIST;
constexpr int PRIMER_WORDS = (int)(sizeof(RibbitPrimer) / sizeof(uint32_t));
constexpr size_t PAIR_LDS_LIMIT = 64 << 10;
static_assert(SHORTLIST * SHORTLIST == 64, "a lane per pair of the two shortlists");
static_assert(sizeof(RibbitRowPrimerPair) == 128, "32 ints");
constexpr unsigned long long EVEN = 0x5555555555555555ull;

__host__ __device__ inline int pair_wave_words(int cap) { return wave_lds_words(cap) + cap + 2 * SHORTLIST * PRIMER_WORDS; }
// the wavefronts of a workgroup and the LDS of one, for windows of up to cap bases
inline int pair_waves(int cap) { return PAIR_WAVES * (size_t)pair_wave_words(cap) * sizeof(uint32_t) <= PAIR_LDS_LIMIT ? PAIR_WAVES : PAIR_WAVES / 2; }

// the bits of the first k bases, 0 <= k <= 32
__device__ inline unsigned long long low_bases(int k) { return k >= 32 ? ~0ull : (1ull << (2 * k)) - 1ull; }

// the k >= 1 bases of o in reverse order
__device__ inline unsigned long long reversed(unsigned long long o, int k) {
    const unsigned long long r = __brevll(o);
    return (((r >> 1) & EVEN) | ((r & EVEN) << 1)) >> (64 - 2 * k);
}
__device__ inline unsigned long long reverse_complement(unsigned long long o, int k) { return ~reversed(o, k) & low_bases(k); }

// m (even bits only) holds n >= 1 set even bits in a row
__device__ inline bool has_run(unsigned long long m, int n) {
    if (n > 32) return false;
    int have = 1;
    while (2 * have <= n) {
        m &= m >> (2 * have);
        have *= 2;
    }
    if (n > have) m &= m >> (2 * (n - have));
    return m != 0;
}
__device__ inline int longest_run(unsigned long long m) {
    int r = 0;
    while (m) {
        m &= m >> 2;
        ++r;
    }
    return r;
}
// the run of set even bits that ends at base `top` going down, and the one that starts at base `bottom` going up; m has no bit
// at or above base 32
__device__ inline int run_down_from(unsigned long long m, int top) {
    const unsigned long long t = (~m & EVEN) << (62 - 2 * top);
    return min(t ? __builtin_clzll(t) >> 1 : 32, top + 1);
}
__device__ inline int run_up_from(unsigned long long m, int bottom) {
    const unsigned long long t = (~m & EVEN) >> (2 * bottom);
    return t ? __builtin_ctzll(t) >> 1 : 32 - bottom;
}

// One placement of a (ka bases) against b (kb bases, rb its reversed bases): a[i] meets rb[i + d], -(ka - 1) <= d <= kb - 1, which
// is the contract's c = kb - 1 - d.  The pairs exist for lo <= i < hi; a's 3' base has one when hi == ka, b's 3' base when d <= 0,
// at i = lo = -d.
struct Placement {
    unsigned long long m;      // bit 2 i: a[i] is bonded
    int lo, hi;
};
__device__ inline Placement placement(unsigned long long a, int ka, unsigned long long rb, int kb, int d) {
    const unsigned long long x = a ^ (d >= 0 ? rb >> (2 * d) : rb << (-2 * d));
    Placement pl;
    pl.lo = max(0, -d);
    pl.hi = min(ka, kb - d);
    pl.m = x & (x >> 1) & EVEN & low_bases(pl.hi) & ~low_bases(pl.lo);
    return pl;
}
// the pairs of a placement of an oligo of k bases with itself that may close a hairpin: i < j = c - i with a loop of
// RIBBIT_PRIMER_HAIRPIN_LOOP bases or more between them, i <= (c - 1 - LOOP) / 2
__device__ inline unsigned long long hairpin_part(const Placement &pl, int k, int d) {
    const int c = k - 1 - d, room = c - 1 - RIBBIT_PRIMER_HAIRPIN_LOOP;
    return room < 0 ? 0ull : pl.m & low_bases((room >> 1) + 1);
}

// placement d of a against b breaks a limit: a run of any_n, a run of more than max_end through a 3' base, or, with hairpin_n > 0
// and a == b, a stem of hairpin_n
__device__ inline bool placement_fails(unsigned long long a, int ka, unsigned long long rb, int kb, int d, int any_n, int max_end, int hairpin_n) {
    const Placement pl = placement(a, ka, rb, kb, d);
    if (has_run(pl.m, any_n)) return true;
    if (pl.hi == ka && run_down_from(pl.m, ka - 1) > max_end) return true;
    if (d <= 0 && run_up_from(pl.m, pl.lo) > max_end) return true;
    return hairpin_n > 0 && has_run(hairpin_part(pl, ka, d), hairpin_n);
}
// any(a, b) <= any_n - 1 and end(a, b) <= max_end, by one lane; rb: b's bases reversed (a caller that meets one b many times, as
// panel.hip's lanes meet a column, reverses it once)
__device__ inline bool duplex_within_reversed(unsigned long long a, int ka, unsigned long long rb, int kb, int any_n, int max_end) {
    for (int d = -(ka - 1); d <= kb - 1; ++d)
        if (placement_fails(a, ka, rb, kb, d, any_n, max_end, 0)) return false;
    return true;
}
__device__ inline bool duplex_within(unsigned long long a, int ka, unsigned long long b, int kb, int any_n, int max_end) {
    return duplex_within_reversed(a, ka, reversed(b, kb), kb, any_n, max_end);
}
// the values themselves of one placement; `stem` only where a == b
struct Runs { int32_t any, end, stem; };
__device__ inline Runs placement_runs(unsigned long long a, int ka, unsigned long long rb, int kb, int d) {
    const Placement pl = placement(a, ka, rb, kb, d);
    Runs r{longest_run(pl.m), 0, longest_run(hairpin_part(pl, ka, d))};
    if (pl.hi == ka) r.end = run_down_from(pl.m, ka - 1);
    if (d <= 0) r.end = max(r.end, run_up_from(pl.m, pl.lo));
    return r;
}
__device__ inline int32_t wave_max(int32_t v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v = max(v, __shfl_xor(v, d));
    return v;
}
__device__ inline unsigned long long wave_or(unsigned long long v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v |= __shfl_xor(v, d);
    return v;
}
// (any, end) of a against b, and with a == b the hairpin: a lane per placement (ka + kb - 1 <= 63), then the wave's maxima
__device__ inline Runs wave_runs(unsigned long long a, int ka, unsigned long long b, int kb, int lane) {
    Runs r{0, 0, 0};
    if (lane < ka + kb - 1) r = placement_runs(a, ka, reversed(b, kb), kb, lane - (ka - 1));
    return Runs{wave_max(r.any), wave_max(r.end), wave_max(r.stem)};
}

__device__ inline unsigned long long bases_of(const RibbitPrimer &p) { return (unsigned long long)(uint32_t)p.bases_hi << 32 | (uint32_t)p.bases_lo; }

// a pair of the two shortlists in the order of the choice: (pair penalty, product, rank_l, rank_r); its low six bits are its lane
__device__ inline unsigned long long pair_key(int32_t pair_penalty, int32_t product, int l, int r) {
    return (unsigned long long)(uint32_t)pair_penalty << 38 | (unsigned long long)(uint32_t)product << 6 | (unsigned long long)(l << 3 | r);
}

// step (3) on the pair of the shortlists' ranks l and r, by one lane over all its placements: its key when it is admissible, else NO_KEY
__device__ inline unsigned long long judge_pair(const RibbitPrimer &a, const RibbitPrimer &b, const RibbitPrimerPairParams &pair, int l, int r) {
    const int32_t difference = abs(a.tm - b.tm);
    if (difference > pair.max_tm_difference) return NO_KEY;
    if (!duplex_within(bases_of(a), a.length, reverse_complement(bases_of(b), b.length), b.length, pair.max_pair_any + 1, pair.max_pair_end)) return NO_KEY;
    return pair_key(a.penalty + b.penalty + difference, b.start + b.length - a.start, l, r);
}

// The chosen pair into rec, by the whole wavefront: lane `winner` holds its two primers a and b, they go to every lane (__shfl), and
// the five values are wave maxima with a lane per placement.  The six counts are the caller's.
__device__ inline void fill_chosen_pair(RibbitRowPrimerPair &rec, const RibbitPrimer &a, const RibbitPrimer &b, int winner, int lane) {
    rec.left = RibbitPrimer{__shfl(a.start, winner), __shfl(a.length, winner), __shfl(a.tm, winner), __shfl(a.penalty, winner), __shfl(a.bases_lo, winner), __shfl(a.bases_hi, winner)};
    rec.right = RibbitPrimer{__shfl(b.start, winner), __shfl(b.length, winner), __shfl(b.tm, winner), __shfl(b.penalty, winner), __shfl(b.bases_lo, winner), __shfl(b.bases_hi, winner)};
    const unsigned long long wa = bases_of(rec.left), wb = reverse_complement(bases_of(rec.right), rec.right.length);
    const Runs left = wave_runs(wa, rec.left.length, wa, rec.left.length, lane), rights = wave_runs(wb, rec.right.length, wb, rec.right.length, lane),
               both = wave_runs(wa, rec.left.length, wb, rec.right.length, lane);
    rec.tm_difference = abs(rec.left.tm - rec.right.tm);
    rec.pair_penalty = rec.left.penalty + rec.right.penalty + rec.tm_difference;
    rec.product = rec.right.start + rec.right.length - rec.left.start;
    rec.left_rank = winner >> 3;
    rec.right_rank = winner & 7;
    rec.left_self_any = left.any;
    rec.left_self_end = left.end;
    rec.left_hairpin = left.stem;
    rec.right_self_any = rights.any;
    rec.right_self_end = rights.end;
    rec.right_hairpin = rights.stem;
    rec.pair_any = both.any;
    rec.pair_end = both.end;
}

// a wavefront's slice of LDS: the window, a word per start, the two shortlists
struct PairSlice {
    Window win;
    uint32_t *passing;         // a word per start: bit k - 1, the candidate of k bases passes
    RibbitPrimer *listed;      // the left side's shortlist, then the right side's
};
__device__ inline PairSlice pair_slice_at(uint32_t *lds, int wave, int cap) {
    uint32_t *slice = lds + (size_t)wave * pair_wave_words(cap);
    PairSlice s;
    s.win = window_at(slice, cap);
    s.passing = slice + wave_lds_words(cap);
    s.listed = reinterpret_cast<RibbitPrimer *>(s.passing + cap);
    return s;
}

// the target t clipped to the record, and a side's window of it
struct TargetSpan { int64_t s, e; };
__device__ inline TargetSpan target_span(const int32_t *__restrict__ targets, int64_t t, int64_t length) {
    const int64_t s = min(max((int64_t)targets[2 * t], (int64_t)0), length);
    return TargetSpan{s, min(max((int64_t)targets[2 * t + 1], s), length)};
}

// One side of a target: the window [from, from + n) staged, its candidates judged (pass 1, the self checks) and the best
// min(shortlist, passed) of them written to listed[0 ..) in order.  -> the side's admissible and passing candidates, the same
// in every lane.  Every lane of the wavefront calls it.
struct SideCounts { int32_t found, passed; };
__device__ inline SideCounts shortlist_side(const PairSlice &sl, RibbitPrimer *listed, int cap, const DevicePlanes &pl, const uint32_t *__restrict__ bits,
                                            const RibbitPrimerParams &prm, const RibbitPrimerPairParams &pair, bool right, int64_t from, int n, int look_back, int lane) {
    const Window &win = sl.win;
    uint32_t *passing = sl.passing;
    fill_window(win, cap, pl, bits, from, n, look_back, lane);
    // pass 1: the admissible lengths of every start ...
    uint32_t found = 0;
    for (int p = lane; p + prm.min_length <= n; p += 64) {
        const uint32_t before = win.cnt[p], first = win.code[p] & 3u;
        uint32_t admissible = 0;
        for (int k = prm.min_length; k <= prm.max_length && p + k <= n; ++k) {
            int32_t tm;
            const Verdict v = judge(win, prm, right, p, k, before, first, tm);
            if (v == STOP) break;
            if (v == TAKE) admissible |= 1u << (k - 1);
        }
        found += (uint32_t)__popc(admissible);
        passing[p] = admissible;
    }
    wave_sync();
    // ... and which of them pass: the wavefront walks the starts that have any, one candidate at a time, a lane per placement
    // (2 k - 1 <= 63 of them); lane 0 writes the start's word back
    uint32_t passed = 0;
    for (int base = 0; base + prm.min_length <= n; base += 64) {
        const uint32_t word = base + lane + prm.min_length <= n ? passing[base + lane] : 0u;
        unsigned long long starts = __ballot(word != 0u);
        while (starts) {
            const int from_lane = __builtin_ctzll(starts), p = base + from_lane;
            starts &= starts - 1ull;
            uint32_t admissible = (uint32_t)__shfl((int)word, from_lane), pass = 0;
            const int longest = 32 - __clz(admissible);
            const unsigned long long bases = wave_or(lane < longest ? (unsigned long long)(win.code[p + lane] & 3u) << (2 * lane) : 0ull);
            while (admissible) {
                const int k = __ffs(admissible);      // (bit k - 1)
                admissible &= admissible - 1u;
                const unsigned long long forward = bases & low_bases(k), o = right ? reverse_complement(forward, k) : forward;
                const bool fails = lane < 2 * k - 1 && placement_fails(o, k, reversed(o, k), k, lane - (k - 1), pair.max_self_any + 1, pair.max_self_end, pair.max_hairpin + 1);
                if (!__any(fails)) pass |= 1u << (k - 1);
            }
            passed += (uint32_t)__popc(pass);
            if (lane == 0) passing[p] = pass;
        }
    }
    const SideCounts counts{(int32_t)__shfl(wave_sum(found), 0), (int32_t)passed};      // (passed is the same in every lane)
    wave_sync();
    // shortlist
    const int rounds = min(pair.shortlist, counts.passed);
    unsigned long long last = 0, mine = NO_KEY;      // (every key is above 0: its k is)
    for (int r = 0; r < rounds; ++r) {
        unsigned long long best = NO_KEY;
        for (int p = lane; p + prm.min_length <= n; p += 64) {
            uint32_t pass = passing[p];
            while (pass) {
                const int k = __ffs(pass);
                pass &= pass - 1u;
                const unsigned long long key = candidate_key(prm, right, p, k, n, melting(win, p, k));
                best = key > last && key < best ? key : best;
            }
        }
        best = wave_min(best);
        last = best;
        mine = lane == r ? best : mine;
    }
    if (lane < rounds) listed[lane] = primer_of(win, mine, right, from, n);
    wave_sync();      // (the next window is staged over this one; the shortlist is read by the caller)
    return counts;
}

}  // namespace

}  // namespace rb
