// primer_specific.hip -- the best primer pair of every target that amplifies nothing else in the loaded record
// (api_primer_specific.cpp: ribbit_hip_record_specific_primer_pairs; include/ribbit_hip.h has the contract, kernels.h the order of
// the launches).  Where primer_pairs.hip keeps the two shortlists of a target in LDS and takes the best admissible pair of them,
// here all 8 x 8 pairs are judged by an in-silico PCR, so the shortlists go through global memory, a batch of targets at a time:
//   shortlists   primer_shortlists_kernel: one wavefront per target, both sides by primer_shortlist.h's shortlist_side, exactly as
//                primer_pairs_kernel makes them; then 16 lanes write the target's 16 RibbitPrimer (an empty place has start -1)
//                and lane 0 its four counts and the number of its shortlisted primers.
//   oligos       One inclusive sum (rocPRIM) over those numbers says where a target's oligos start; shortlisted_oligos_kernel
//                writes them one behind the other, the left ones as they stand, the right ones reverse-complemented (as
//                ordered), so no empty place reaches the search.  The last target's sum is the batch's number of oligos.
//   sites        primer_products.hip's site search (kernels.h, at ProductLayout): uniques, patterns, one pass over the planes, every
//                kept list sorted.
//   the walk     specific_pairs_kernel: one wavefront per target, lane 8 l + r for the pair (l, r).  The lane judges the pair's
//                admissibility from the stored shortlists (judge_pair, as primer_pairs_kernel), counts its products over its
//                four sorted lists (product_walk.h, as pair_products_kernel) and calls it over, specific or other.  The four
//                counts are ballots and popcounts; the winner is one wave minimum of the packed key over the specific lanes;
//                its place is the popcount of the admissible lanes with a smaller key; the pair in place 0 is the wave minimum
//                over the admissible lanes.  The winner's two primers go to every lane and its five dimer values are wave
//                maxima with a lane per placement (fill_chosen_pair), its products come by __shfl, and lane 0 writes the three
//                records.  No LDS.
// For a genome (api_primer_genome.cpp: ribbit_hip_record_shortlist_verdicts) the shortlists come up from the host and the loaded
// record may be another one than they were made on: held_places_kernel counts each target's held places, the same sum and
// shortlisted_oligos_kernel make the batch's oligos without primer_shortlists_kernel, the site scan is the same, and
// shortlist_verdicts_kernel judges the 64 pairs as above but hands out the outcome of every pair as four masks, not a choice.
// The kernels stride beyond ROW_MAX_BLOCKS blocks.  No atomics of their own (the site scan's integer vector atomics are
// primer_products.hip's), no inline assembly.
#include <cstring>

#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>

#include "primer_shortlist.h"
#include "product_walk.h"

namespace rb {

namespace {

static_assert(SLOTS == 2 * SHORTLIST, "two shortlists a target");
static_assert(sizeof(RibbitRowSpecific) == 32 && sizeof(RibbitRowProducts) == 32 && sizeof(RibbitOligo) == 12, "8, 8 and 3 ints");
static_assert(sizeof(RibbitTargetVerdicts) == 176 && sizeof(RibbitPrimer) == 24, "four masks and 36 ints; 6 ints");

__global__ void __launch_bounds__(64 * PAIR_WAVES) primer_shortlists_kernel(const int32_t *__restrict__ targets, int64_t n_targets, DevicePlanes pl,
                                                                           const uint32_t *__restrict__ bits, RibbitPrimerParams prm, RibbitPrimerPairParams pair, int cap,
                                                                           RibbitPrimer *__restrict__ lists, int32_t *__restrict__ counts, uint32_t *__restrict__ n_oligos) {
    extern __shared__ uint32_t lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, waves = blockDim.x >> 6;
    const PairSlice sl = pair_slice_at(lds, wave, cap);
    const int64_t length = pl.length;
    const int look_back = run_look_back(prm);
    for (int64_t t = (int64_t)blockIdx.x * waves + wave; t < n_targets; t += (int64_t)gridDim.x * waves) {
        const TargetSpan span = target_span(targets, t, length);
        const int64_t left_from = max(span.s - (int64_t)prm.flank, (int64_t)0), right_to = min(span.e + (int64_t)prm.flank, length);
        const SideCounts lc = shortlist_side(sl, sl.listed, cap, pl, bits, prm, pair, false, left_from, (int)(span.s - left_from), look_back, lane);
        const SideCounts rc = shortlist_side(sl, sl.listed + SHORTLIST, cap, pl, bits, prm, pair, true, span.e, (int)(right_to - span.e), look_back, lane);
        const int n_left = min(pair.shortlist, lc.passed), n_right = min(pair.shortlist, rc.passed);
        if (lane < SLOTS) {
            const bool held = lane < SHORTLIST ? lane < n_left : lane - SHORTLIST < n_right;
            lists[t * SLOTS + lane] = held ? sl.listed[lane] : RibbitPrimer{-1, 0, 0, 0, 0, 0};
        }
        if (lane == 0) {
            counts[4 * t] = lc.found;
            counts[4 * t + 1] = rc.found;
            counts[4 * t + 2] = lc.passed;
            counts[4 * t + 3] = rc.passed;
            n_oligos[t] = (uint32_t)(n_left + n_right);
        }
        wave_sync();      // (the next target's shortlists are written over these)
    }
}

// a lane per place of the shortlists: the primers that are there as oligos 5' to 3', a target's one behind the other
__global__ void __launch_bounds__(ROW_THREADS) shortlisted_oligos_kernel(const RibbitPrimer *__restrict__ lists, const uint32_t *__restrict__ n_oligos,
                                                                           const uint32_t *__restrict__ upto, int64_t n_targets, RibbitOligo *__restrict__ oligos,
                                                                           SpecificHeader *__restrict__ header) {
    for (int64_t i = (int64_t)blockIdx.x * ROW_THREADS + threadIdx.x; i < n_targets * SLOTS; i += (int64_t)gridDim.x * ROW_THREADS) {
        const int64_t t = i / SLOTS;
        const int slot = (int)(i - t * SLOTS);
        if (i == n_targets * SLOTS - 1) header->oligos = upto[t];
        const RibbitPrimer p = lists[i];
        if (p.start < 0) continue;
        // the left ones fill their shortlist from rank 0 on, so the right ones start behind as many as there are
        int before = slot;
        if (slot >= SHORTLIST) {
            before = slot - SHORTLIST;
            for (int l = 0; l < SHORTLIST; ++l) before += lists[t * SLOTS + l].start >= 0;
        }
        const unsigned long long bases = slot < SHORTLIST ? bases_of(p) : reverse_complement(bases_of(p), p.length);
        oligos[(int64_t)(upto[t] - n_oligos[t]) + before] = RibbitOligo{p.length, (int32_t)(uint32_t)bases, (int32_t)(uint32_t)(bases >> 32)};
    }
}

__global__ void __launch_bounds__(64 * PAIR_WAVES) specific_pairs_kernel(const RibbitPrimer *__restrict__ lists, const int32_t *__restrict__ side_counts,
                                                                        const uint32_t *__restrict__ n_oligos, const uint32_t *__restrict__ upto, int64_t n_targets,
                                                                        RibbitPrimerPairParams pair, const uint32_t *__restrict__ unique_of,
                                                                        const UniqueOligo *__restrict__ uniques, const uint32_t *__restrict__ counts,
                                                                        const int32_t *__restrict__ site_lists, int max_product, int max_sites,
                                                                        RibbitRowPrimerPair *__restrict__ out_pairs, RibbitRowProducts *__restrict__ out_products,
                                                                        RibbitRowSpecific *__restrict__ out_specific) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, waves = blockDim.x >> 6;
    for (int64_t t = (int64_t)blockIdx.x * waves + wave; t < n_targets; t += (int64_t)gridDim.x * waves) {
        const int32_t left_passed = side_counts[4 * t + 2], right_passed = side_counts[4 * t + 3];
        const int n_left = min(pair.shortlist, left_passed), n_right = min(pair.shortlist, right_passed);
        const int64_t first_oligo = (int64_t)(upto[t] - n_oligos[t]);
        const int l = lane >> 3, r = lane & 7;
        RibbitPrimer a = {-1, 0, 0, 0, 0, 0}, b = a;
        unsigned long long key = NO_KEY;
        RibbitRowProducts found = {};
        if (l < n_left && r < n_right) {
            a = lists[t * SLOTS + l];
            b = lists[t * SLOTS + SHORTLIST + r];
            key = judge_pair(a, b, pair, l, r);
            if (key != NO_KEY)
                found = pair_products(unique_of[first_oligo + l], unique_of[first_oligo + n_left + r], a.start, b.start, uniques, counts, site_lists, max_product, max_sites);
        }
        const bool admissible = key != NO_KEY, over = admissible && found.products < 0, specific = admissible && !over && found.products - found.own == 0;
        const int32_t others = found.products < 0 ? -1 : found.products - found.own;
        const unsigned long long best = wave_min(specific ? key : NO_KEY), first = wave_min(key);
        RibbitRowSpecific sum = {};
        sum.pairs_admissible = (int32_t)__popcll(__ballot(admissible));
        sum.pairs_specific = (int32_t)__popcll(__ballot(specific));
        sum.pairs_over = (int32_t)__popcll(__ballot(over));
        sum.pairs_other = sum.pairs_admissible - sum.pairs_specific - sum.pairs_over;
        sum.place = best != NO_KEY ? (int32_t)__popcll(__ballot(admissible && key < best)) : -1;
        sum.first_products = first != NO_KEY ? __shfl(others, (int)(first & 63u)) : 0;
        // the winner's lane is its key's low six bits
        const int winner = (int)(best & 63u);
        RibbitRowPrimerPair rec = {};
        rec.left.start = rec.right.start = -1;
        RibbitRowProducts prod = {};
        if (best != NO_KEY) {
            fill_chosen_pair(rec, a, b, winner, lane);
            prod.left_forward = __shfl(found.left_forward, winner);
            prod.left_reverse = __shfl(found.left_reverse, winner);
            prod.right_forward = __shfl(found.right_forward, winner);
            prod.right_reverse = __shfl(found.right_reverse, winner);
            prod.products = __shfl(found.products, winner);
            prod.own = __shfl(found.own, winner);
            prod.shortest_other = __shfl(found.shortest_other, winner);
        }
        rec.left_candidates = side_counts[4 * t];
        rec.right_candidates = side_counts[4 * t + 1];
        rec.left_passed = left_passed;
        rec.right_passed = right_passed;
        rec.pairs_tried = n_left * n_right;
        rec.pairs_admissible = sum.pairs_admissible;
        if (lane == 0) {
            out_pairs[t] = rec;
            out_products[t] = prod;
            out_specific[t] = sum;
        }
    }
}

// ---- shortlists that were made elsewhere, judged on the loaded record (ribbit_hip_record_shortlist_verdicts)
// a lane per target: the held places of its two uploaded shortlists (the caller has checked that they are the first ones)
__global__ void __launch_bounds__(ROW_THREADS) held_places_kernel(const RibbitPrimer *__restrict__ lists, int64_t n_targets, uint32_t *__restrict__ n_left,
                                                                    uint32_t *__restrict__ n_oligos) {
    for (int64_t t = (int64_t)blockIdx.x * ROW_THREADS + threadIdx.x; t < n_targets; t += (int64_t)gridDim.x * ROW_THREADS) {
        uint32_t left = 0, right = 0;
        for (int k = 0; k < SHORTLIST; ++k) {
            left += lists[t * SLOTS + k].start >= 0;
            right += lists[t * SLOTS + SHORTLIST + k].start >= 0;
        }
        n_left[t] = left;
        n_oligos[t] = left + right;
    }
}

// One wavefront per target, lane 8 l + r for the pair (l, r), as specific_pairs_kernel: the lane judges the pair's admissibility
// from the stored primers and counts its products on this record, with the own positions only when this is the home record.  The
// four masks are ballots, first_others comes from the lane of the wave-minimum key, and lanes 0 to 15 write the site counts of the
// target's 16 places.  No LDS.
__global__ void __launch_bounds__(64 * PAIR_WAVES) shortlist_verdicts_kernel(const RibbitPrimer *__restrict__ lists, const uint32_t *__restrict__ n_left_of,
                                                                            const uint32_t *__restrict__ n_oligos, const uint32_t *__restrict__ upto, int64_t n_targets,
                                                                            RibbitPrimerPairParams pair, int home, const uint32_t *__restrict__ unique_of,
                                                                            const UniqueOligo *__restrict__ uniques, const uint32_t *__restrict__ counts,
                                                                            const int32_t *__restrict__ site_lists, int max_product, int max_sites,
                                                                            RibbitTargetVerdicts *__restrict__ out) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, waves = blockDim.x >> 6;
    for (int64_t t = (int64_t)blockIdx.x * waves + wave; t < n_targets; t += (int64_t)gridDim.x * waves) {
        const int n_left = (int)n_left_of[t], n_right = (int)n_oligos[t] - n_left;
        const int64_t first_oligo = (int64_t)(upto[t] - n_oligos[t]);
        const int l = lane >> 3, r = lane & 7;
        unsigned long long key = NO_KEY;
        RibbitRowProducts found = {};
        if (l < n_left && r < n_right) {
            const RibbitPrimer a = lists[t * SLOTS + l], b = lists[t * SLOTS + SHORTLIST + r];
            key = judge_pair(a, b, pair, l, r);
            if (key != NO_KEY)
                found = pair_products(unique_of[first_oligo + l], unique_of[first_oligo + n_left + r], home ? a.start : -1, home ? b.start : -1, uniques, counts, site_lists,
                                      max_product, max_sites);
        }
        const bool admissible = key != NO_KEY, over = admissible && found.products < 0;
        const int32_t others = over ? -1 : found.products - found.own;
        const unsigned long long m_admissible = __ballot(admissible), m_over = __ballot(over), m_other = __ballot(admissible && others > 0),
                                 m_own = __ballot(admissible && found.own != 0);
        const unsigned long long first = wave_min(key);
        const int32_t first_others = first != NO_KEY ? __shfl(others, (int)(first & 63u)) : 0;
        if (lane < SLOTS) {
            const int rank = lane < SHORTLIST ? lane : lane - SHORTLIST;
            const bool held = lane < SHORTLIST ? rank < n_left : rank < n_right;
            uint32_t forward = 0, reverse = 0;
            if (held) {
                const uint32_t u = unique_of[first_oligo + (lane < SHORTLIST ? rank : n_left + rank)];
                forward = counts[2 * u];
                reverse = counts[2 * u + 1];
            }
            out[t].forward[lane] = (int32_t)forward;
            out[t].reverse[lane] = (int32_t)reverse;
        }
        if (lane == 0) {
            out[t].admissible = m_admissible;
            out[t].over = m_over;
            out[t].other = m_other;
            out[t].own = m_own;
            out[t].first_others = first_others;
            out[t].records = 1;
            out[t].home_records = home;
            out[t].reserved = 0;
        }
    }
}

hipError_t sum_counts(void *scratch, size_t &bytes, const uint32_t *in, uint32_t *out, int64_t n, hipStream_t stream) {
    return rocprim::inclusive_scan(scratch, bytes, in, out, (size_t)n, rocprim::plus<uint32_t>(), stream);
}

bool specific_params_fit(const RibbitPrimerParams &prm, const RibbitPrimerPairParams &pair) {
    return prm.flank >= 0 && prm.flank <= RIBBIT_PRIMER_MAX_FLANK && prm.min_length >= 2 && prm.max_length <= RIBBIT_PRIMER_MAX_LENGTH && pair.shortlist >= 1 &&
           pair.shortlist <= SHORTLIST;
}

// the inclusive sum of the targets' counts behind them, then the counted primers of `lists` as oligos one behind the other and
// their number in the header
hipError_t oligos_of_lists(const RibbitPrimer *lists, uint32_t *n_oligos, int64_t n_targets, uint8_t *work, const WorkLayout &at, size_t oligos, size_t header,
                           hipStream_t stream) {
    uint32_t *upto = n_oligos + n_targets;
    // (the layout may be a larger batch's: what the sum asks for these targets must fit its region)
    size_t bytes = 0;
    hipError_t e = sum_counts(nullptr, bytes, n_oligos, upto, n_targets, stream);
    if (e != hipSuccess) return e;
    if (bytes > at.scratch_bytes) return hipErrorInvalidValue;
    if ((e = sum_counts(work + at.scratch, bytes, n_oligos, upto, n_targets, stream)) != hipSuccess) return e;
    hipLaunchKernelGGL(shortlisted_oligos_kernel, dim3(grid_for(n_targets * SLOTS, ROW_THREADS, ROW_MAX_BLOCKS)), dim3(ROW_THREADS), 0, stream, lists, n_oligos, upto, n_targets,
                       region<RibbitOligo>(work, oligos), region<SpecificHeader>(work, header));
    return hipGetLastError();
}

}  // namespace

SpecificLayout specific_layout(int64_t n_targets) {
    const size_t n = (size_t)n_targets;
    size_t a = 0;
    (void)sum_counts(nullptr, a, nullptr, nullptr, n_targets, 0);
    SpecificLayout at{};
    WorkCarver w;
    at.lists = w.take(n * SLOTS * sizeof(RibbitPrimer));
    at.side_counts = w.take(4 * n * sizeof(int32_t));
    at.n_oligos = w.take(2 * n * sizeof(uint32_t));
    at.oligos = w.take(n * SLOTS * sizeof(RibbitOligo));
    at.header = w.take(sizeof(SpecificHeader));
    at.pairs = w.take(n * sizeof(RibbitRowPrimerPair));
    at.products = w.take(n * sizeof(RibbitRowProducts));
    at.specific = w.take(n * sizeof(RibbitRowSpecific));
    at.sites = site_room(w, n_targets * SLOTS);
    w.close(at, a);
    return at;
}

hipError_t launch_primer_shortlists(const DevicePlanes &pl, const uint32_t *bits, const int32_t *targets, int64_t n_targets, const RibbitPrimerParams &prm,
                                    const RibbitPrimerPairParams &pair, uint8_t *work, size_t work_bytes, const SpecificLayout &at, hipStream_t stream) {
    if (work_bytes < at.bytes || n_targets < 1 || !specific_params_fit(prm, pair)) return hipErrorInvalidValue;
    const int cap = std::max(prm.flank, 1);
    const size_t wave_bytes = (size_t)pair_wave_words(cap) * sizeof(uint32_t);
    const int waves = pair_waves(cap);
    RibbitPrimer *lists = region<RibbitPrimer>(work, at.lists);
    uint32_t *n_oligos = region<uint32_t>(work, at.n_oligos);
    hipLaunchKernelGGL(primer_shortlists_kernel, dim3(grid_for(n_targets, waves, ROW_MAX_BLOCKS)), dim3(64 * waves), waves * wave_bytes, stream, targets, n_targets, pl, bits,
                       prm, pair, cap, lists, region<int32_t>(work, at.side_counts), n_oligos);
    return oligos_of_lists(lists, n_oligos, n_targets, work, at, at.oligos, at.header, stream);
}

hipError_t launch_specific_pairs(int64_t n_targets, const RibbitPrimerPairParams &pair, const RibbitProductParams &product, uint8_t *work, size_t work_bytes,
                                 const SpecificLayout &at, const int32_t *site_lists, hipStream_t stream) {
    if (work_bytes < at.bytes || n_targets < 1 || pair.shortlist < 1 || pair.shortlist > SHORTLIST || product.max_product < 1 || product.max_sites < 1)
        return hipErrorInvalidValue;
    const uint32_t *n_oligos = region<uint32_t>(work, at.n_oligos);
    uint8_t *pw = work + at.sites.offset;
    hipLaunchKernelGGL(specific_pairs_kernel, dim3(grid_for(n_targets, PAIR_WAVES, ROW_MAX_BLOCKS)), dim3(64 * PAIR_WAVES), 0, stream, region<RibbitPrimer>(work, at.lists),
                       region<int32_t>(work, at.side_counts), n_oligos, n_oligos + n_targets, n_targets, pair, region<uint32_t>(pw, at.sites.layout.unique_of),
                       region<UniqueOligo>(pw, at.sites.layout.uniques), region<uint32_t>(pw, at.sites.layout.counts), site_lists, (int)product.max_product, (int)product.max_sites,
                       region<RibbitRowPrimerPair>(work, at.pairs), region<RibbitRowProducts>(work, at.products), region<RibbitRowSpecific>(work, at.specific));
    return hipGetLastError();
}

VerdictLayout verdict_layout(int64_t n_targets) {
    const size_t n = (size_t)n_targets;
    size_t a = 0;
    (void)sum_counts(nullptr, a, nullptr, nullptr, n_targets, 0);
    VerdictLayout at{};
    WorkCarver w;
    at.n_oligos = w.take(2 * n * sizeof(uint32_t));
    at.n_left = w.take(n * sizeof(uint32_t));
    at.oligos = w.take(n * SLOTS * sizeof(RibbitOligo));
    at.header = w.take(sizeof(SpecificHeader));
    at.verdicts = w.take(n * sizeof(RibbitTargetVerdicts));
    at.sites = site_room(w, n_targets * SLOTS);
    w.close(at, a);
    return at;
}

hipError_t launch_listed_oligos(const RibbitPrimer *lists, int64_t n_targets, uint8_t *work, size_t work_bytes, const VerdictLayout &at, hipStream_t stream) {
    if (work_bytes < at.bytes || n_targets < 1) return hipErrorInvalidValue;
    uint32_t *n_oligos = region<uint32_t>(work, at.n_oligos);
    hipLaunchKernelGGL(held_places_kernel, dim3(grid_for(n_targets, ROW_THREADS, ROW_MAX_BLOCKS)), dim3(ROW_THREADS), 0, stream, lists, n_targets,
                       region<uint32_t>(work, at.n_left), n_oligos);
    return oligos_of_lists(lists, n_oligos, n_targets, work, at, at.oligos, at.header, stream);
}

hipError_t launch_shortlist_verdicts(const RibbitPrimer *lists, int64_t n_targets, bool home, const RibbitPrimerPairParams &pair, const RibbitProductParams &product,
                                     uint8_t *work, size_t work_bytes, const VerdictLayout &at, const int32_t *site_lists, hipStream_t stream) {
    if (work_bytes < at.bytes || n_targets < 1 || product.max_product < 1 || product.max_sites < 1) return hipErrorInvalidValue;
    const uint32_t *n_oligos = region<uint32_t>(work, at.n_oligos);
    uint8_t *pw = work + at.sites.offset;
    hipLaunchKernelGGL(shortlist_verdicts_kernel, dim3(grid_for(n_targets, PAIR_WAVES, ROW_MAX_BLOCKS)), dim3(64 * PAIR_WAVES), 0, stream, lists,
                       region<uint32_t>(work, at.n_left), n_oligos, n_oligos + n_targets, n_targets, pair, home ? 1 : 0, region<uint32_t>(pw, at.sites.layout.unique_of),
                       region<UniqueOligo>(pw, at.sites.layout.uniques), region<uint32_t>(pw, at.sites.layout.counts), site_lists, (int)product.max_product, (int)product.max_sites,
                       region<RibbitTargetVerdicts>(work, at.verdicts));
    return hipGetLastError();
}

}  // namespace rb
