// primer_pairs.hip -- the two primers of every target of the loaded record chosen as one pair, each checked for self-dimers and
// hairpins and the pair for cross-dimers (api_primer_pairs.cpp: ribbit_hip_record_primer_pairs; include/ribbit_hip.h has the
// contract).  One wavefront per target does the left side, then the right side, then the pairs, so the shortlists never leave LDS
// (through global memory 2 x 8 candidates per target would be over 300 MB at 800,000 targets).  The window's staging, expansion,
// prefix scans and the verdict of the five rules on a candidate are primer_window.h's, shared with primers.hip; the oligos as 64
// bits, the duplex of two of them and a side's way from its window to its shortlist (pass 1, the self checks, the shortlist
// rounds) are primer_shortlist.h's, shared with primer_specific.hip, which does send the shortlists through global memory, in
// batches.
//   per side:           shortlist_side (primer_shortlist.h)
//   the pairs:          lane 8 l + r judges the pair (l, r), all its placements; one wave minimum of
//                       pair_penalty << 38 | product << 6 | l << 3 | r picks, and the key's low six bits are the winner's lane.
//                       Its two primers go to every lane (__shfl), the five values are wave maxima with a lane per placement
//                       again, and lane 0 writes the record.
// The kernel strides beyond ROW_MAX_BLOCKS blocks.  No atomics, no inline assembly.
#include <hip/hip_runtime.h>

#include "primer_shortlist.h"

namespace rb {

namespace {

__global__ void __launch_bounds__(64 * PAIR_WAVES) primer_pairs_kernel(const int32_t *__restrict__ targets, int64_t n_targets, DevicePlanes pl, const uint32_t *__restrict__ bits,
                                                                      RibbitPrimerParams prm, RibbitPrimerPairParams pair, int cap, RibbitRowPrimerPair *__restrict__ out) {
    extern __shared__ uint32_t lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, waves = blockDim.x >> 6;
    const PairSlice sl = pair_slice_at(lds, wave, cap);
    RibbitPrimer *listed = sl.listed;
    const int64_t length = pl.length;
    const int look_back = run_look_back(prm);
    for (int64_t t = (int64_t)blockIdx.x * waves + wave; t < n_targets; t += (int64_t)gridDim.x * waves) {
        const TargetSpan span = target_span(targets, t, length);
        const int64_t s = span.s, e = span.e;
        const int64_t left_from = max(s - (int64_t)prm.flank, (int64_t)0), right_to = min(e + (int64_t)prm.flank, length);
        const SideCounts lc = shortlist_side(sl, listed, cap, pl, bits, prm, pair, false, left_from, (int)(s - left_from), look_back, lane);
        const SideCounts rc = shortlist_side(sl, listed + SHORTLIST, cap, pl, bits, prm, pair, true, e, (int)(right_to - e), look_back, lane);
        const int32_t left_candidates = lc.found, right_candidates = rc.found, left_passed = lc.passed, right_passed = rc.passed;
        // the pairs
        const int n_left = min(pair.shortlist, left_passed), n_right = min(pair.shortlist, right_passed);
        const int l = lane >> 3, r = lane & 7;
        RibbitPrimer a = {-1, 0, 0, 0, 0, 0}, b = a;
        unsigned long long key = NO_KEY;
        if (l < n_left && r < n_right) {
            a = listed[l];
            b = listed[SHORTLIST + r];
            key = judge_pair(a, b, pair, l, r);
        }
        const unsigned long long best = wave_min(key);
        const int32_t admissible_pairs = (int32_t)__popcll(__ballot(key != NO_KEY));
        // the winner's lane is its key's low six bits: its two primers to every lane, then the five values with a lane per placement
        RibbitRowPrimerPair rec = {};
        rec.left.start = rec.right.start = -1;
        if (best != NO_KEY) fill_chosen_pair(rec, a, b, (int)(best & 63u), lane);
        rec.left_candidates = left_candidates;
        rec.right_candidates = right_candidates;
        rec.left_passed = left_passed;
        rec.right_passed = right_passed;
        rec.pairs_tried = n_left * n_right;
        rec.pairs_admissible = admissible_pairs;
        if (lane == 0) out[t] = rec;
        wave_sync();      // (the next target's shortlists are written over these)
    }
}

}  // namespace

PrimerPairLayout primer_pairs_layout(int64_t n_targets) {
    PrimerPairLayout at{};
    WorkCarver w;
    at.out = w.take((size_t)n_targets * sizeof(RibbitRowPrimerPair));
    w.close(at, 0);
    return at;
}

hipError_t launch_primer_pairs(const DevicePlanes &pl, const uint32_t *bits, const int32_t *targets, int64_t n_targets, const RibbitPrimerParams &prm,
                               const RibbitPrimerPairParams &pair, uint8_t *work, size_t work_bytes, const PrimerPairLayout &at, hipStream_t stream) {
    if (work_bytes < at.bytes || prm.flank < 0 || prm.flank > RIBBIT_PRIMER_MAX_FLANK || prm.min_length < 2 || prm.max_length > RIBBIT_PRIMER_MAX_LENGTH ||
        pair.shortlist < 1 || pair.shortlist > SHORTLIST)
        return hipErrorInvalidValue;
    const int cap = std::max(prm.flank, 1);
    const size_t wave_bytes = (size_t)pair_wave_words(cap) * sizeof(uint32_t);      // 17.9 KB at most
    const int waves = pair_waves(cap);
    hipLaunchKernelGGL(primer_pairs_kernel, dim3(grid_for(n_targets, waves, ROW_MAX_BLOCKS)), dim3(64 * waves), waves * wave_bytes, stream, targets, n_targets, pl, bits, prm,
                       pair, cap, region<RibbitRowPrimerPair>(work, at.out));
    return hipGetLastError();
}

}  // namespace rb
