// api_primer_genome.cpp -- the specific primer pairs of a genome of many records: a target's two shortlists as they leave the
// record they were made on, their admissible pairs judged on any loaded record (primer_specific.hip), the judgements summed over
// the records and the choice made from the sum; see api_internal.h for the map of the files behind include/ribbit_hip.h.
// ribbit_hip_record_primer_shortlists runs the first launch of ribbit_hip_record_specific_primer_pairs and copies the lists and the
// side counts back.  ribbit_hip_record_shortlist_verdicts takes such lists down again, a batch of targets at a time by the rule of
// that call: their held primers become the batch's oligos on the device, the site search (search_sites, api_internal.h) finds them
// on the loaded record, and one wavefront per target judges its 64 pairs (rb::VerdictLayout).  Everything that comes from the caller is
// checked before it goes down, because the kernels index by it.
// The host twins work from the bytes of the sequence with the host code behind the twins they combine (primers_host.h) and share
// nothing with the kernels.  The sum and the choice need no GPU and no sequence.
#include "primers_host.h"

#include <string>

namespace {

static_assert(sizeof(RibbitTargetShortlists) == 400 && sizeof(RibbitTargetVerdicts) == 176 && sizeof(RibbitPrimer) == 24, "100 ints; four masks and 36 ints; 6 ints");
using rb::SLOTS;
constexpr size_t LIST_BYTES = SLOTS * sizeof(RibbitPrimer), SHORTLIST_BATCH = 32768;

// the lists as the kernels index them: the held places first, no more of them than `shortlist`, every held primer of least .. 32 bases
int check_lists(const RibbitTargetShortlists *lists, size_t n, int32_t shortlist, int32_t least) {
    for (size_t i = 0; i < n; ++i)
        for (const RibbitPrimer *side : {lists[i].left, lists[i].right}) {
            const int held = host_held_places(side);
            for (int k = held; k < RIBBIT_PRIMER_PAIR_SHORTLIST; ++k)
                if (side[k].start >= 0) return fail(RIBBIT_E_ARG, "target %zu: a held place behind an empty one", i);
            if (held > shortlist) return fail(RIBBIT_E_ARG, "target %zu: %d held places, more than shortlist %d", i, held, (int)shortlist);
            for (int k = 0; k < held; ++k)
                if (side[k].length < least || side[k].length > RIBBIT_PRIMER_MAX_LENGTH)
                    return fail(RIBBIT_E_ARG, "target %zu: a primer of %d bases, not %d .. %d", i, (int)side[k].length, (int)least, RIBBIT_PRIMER_MAX_LENGTH);
        }
    return RIBBIT_OK;
}

int check_verdict_args(const RibbitTargetShortlists *lists, size_t n_targets, int32_t home, const RibbitPrimerPairParams *pair, const RibbitProductParams *product,
                       const void *verdicts) {
    if ((!lists && n_targets > 0) || !verdicts) return fail(RIBBIT_E_ARG, "null argument");
    if (n_targets > MAX_TARGETS) return fail(RIBBIT_E_ARG, "%zu targets", n_targets);
    if (home != 0 && home != 1) return fail(RIBBIT_E_ARG, "home %d is neither 0 nor 1", (int)home);
    int rc;
    if ((rc = check_primer_pair_params(pair))) return rc;
    if ((rc = check_primer_product_params(product))) return rc;
    return check_lists(lists, n_targets, pair->shortlist, product->seed);
}

// a target's pairs in the order of the choice and the mask of their bits
struct ListedPairs {
    std::vector<RibbitRowPrimerPair> ordered;
    RibbitRowPrimerPair none;
    uint64_t admissible = 0;
};
uint64_t bit_of(const RibbitRowPrimerPair &r) { return (uint64_t)1 << (8 * r.left_rank + r.right_rank); }
void listed_pairs(const RibbitTargetShortlists &lists, const RibbitPrimerPairParams &pair, ListedPairs &out) {
    host_listed_pairs(lists, pair, out.ordered, out.none);
    out.admissible = 0;
    for (const RibbitRowPrimerPair &r : out.ordered) out.admissible |= bit_of(r);
}

// the verdicts of a record without a base: no sites, and `admissible` from the lists alone
void verdicts_without_sites(const RibbitTargetShortlists *lists, size_t n, int32_t home, const RibbitPrimerPairParams &pair, RibbitTargetVerdicts *out) {
    ListedPairs found;
    for (size_t i = 0; i < n; ++i) {
        listed_pairs(lists[i], pair, found);
        out[i] = RibbitTargetVerdicts{};
        out[i].admissible = found.admissible;
        out[i].records = 1;
        out[i].home_records = home;
    }
}

// ---- the GPU forms
int record_shortlists_impl(RibbitHandle *h, const int32_t *intervals, size_t n, const int32_t *targets, size_t n_targets, const RibbitPrimerParams *params,
                           const RibbitPrimerPairParams *pair, const RibbitTargetShortlists **lists) {
    if (!h) return fail(RIBBIT_E_ARG, "null handle");
    int rc;
    if ((rc = check_primer_args(intervals, n, targets, n_targets, params, lists))) return rc;
    if ((rc = check_primer_pair_params(pair))) return rc;
    if (!h->loaded) return fail(RIBBIT_E_STATE, "no record loaded");
    RibbitHandle::RowBufs &buf = h->rows;
    const size_t batch = std::max<size_t>(1, std::min(buf.specific_batch ? buf.specific_batch : SHORTLIST_BATCH, n_targets));
    // the targets' records, and behind them one batch as the device holds it: the lists, then the four counts of every target
    const size_t per_batch_target = LIST_BYTES + 4 * sizeof(int32_t);
    if ((rc = buf.h_shortlists.ensure(std::max<size_t>(n_targets, 1) * sizeof(RibbitTargetShortlists) + batch * per_batch_target, true))) return rc;
    RibbitTargetShortlists *out = reinterpret_cast<RibbitTargetShortlists *>(buf.h_shortlists.p);
    uint8_t *up = buf.h_shortlists.p + std::max<size_t>(n_targets, 1) * sizeof(RibbitTargetShortlists);
    *lists = out;
    if (n_targets == 0) return RIBBIT_OK;
    if (h->length == 0) {      // (every flank is empty)
        RibbitTargetShortlists none{};
        std::fill(none.left, none.left + RIBBIT_PRIMER_PAIR_SHORTLIST, NO_PRIMER);
        std::fill(none.right, none.right + RIBBIT_PRIMER_PAIR_SHORTLIST, NO_PRIMER);
        std::fill(out, out + n_targets, none);
        return RIBBIT_OK;
    }
    if ((rc = bind_device(h))) return rc;
    const rb::SpecificLayout at = rb::specific_layout((int64_t)batch);
    if ((rc = buf.d_work.ensure(at.bytes, true))) return rc;
    const StageSegment down{targets, 2 * n_targets * sizeof(int32_t)};
    const uint8_t *d_targets = nullptr;
    if ((rc = stage_down(h, &down, 1, &d_targets))) return rc;
    if ((rc = build_coverage(h, intervals, n))) return rc;
    uint8_t *work = buf.d_work.p;
    for (size_t from = 0; from < n_targets; from += batch) {
        const size_t m = std::min(batch, n_targets - from);
        HIP_TRY(rb::launch_primer_shortlists(h->planes(), buf.d_mask_bits.p, reinterpret_cast<const int32_t *>(d_targets) + 2 * from, (int64_t)m, *params, *pair, work,
                                             buf.d_work.cap, at, h->stream));
        HIP_TRY(hipMemcpyAsync(up, work + at.lists, m * LIST_BYTES, hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipMemcpyAsync(up + batch * LIST_BYTES, work + at.side_counts, m * 4 * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));
        const int32_t *counts = reinterpret_cast<const int32_t *>(up + batch * LIST_BYTES);
        for (size_t i = 0; i < m; ++i) {
            RibbitTargetShortlists &t = out[from + i];
            std::memcpy(t.left, up + i * LIST_BYTES, LIST_BYTES);      // (left[8] and right[8] lie one behind the other, as on the device)
            t.left_candidates = counts[4 * i];
            t.right_candidates = counts[4 * i + 1];
            t.left_passed = counts[4 * i + 2];
            t.right_passed = counts[4 * i + 3];
        }
    }
    // what the device returned
    for (size_t i = 0; i < n_targets; ++i) {
        const RibbitTargetShortlists &t = out[i];
        const Flanks f = flanks_of(targets, i, params->flank, h->length);
        bool good = t.left_passed >= 0 && t.right_passed >= 0 && t.left_passed <= t.left_candidates && t.right_passed <= t.right_candidates &&
                    host_held_places(t.left) == std::min(pair->shortlist, t.left_passed) && host_held_places(t.right) == std::min(pair->shortlist, t.right_passed);
        for (int side = 0; side < 2 && good; ++side) {
            const RibbitPrimer *list = side ? t.right : t.left;
            const int64_t lo = side ? f.e : f.lo, hi = side ? f.hi : f.s;
            const int held = host_held_places(list);
            for (int k = 0; k < RIBBIT_PRIMER_PAIR_SHORTLIST; ++k) {
                const RibbitPrimer &q = list[k];
                good = good && (k < held ? q.length >= params->min_length && q.length <= params->max_length && q.start >= lo && (int64_t)q.start + q.length <= hi
                                         : q.start == -1 && q.length == 0);
            }
        }
        if (!good) return fail(RIBBIT_E_INTERNAL, "target %zu: a shortlist the GPU made lies outside its flank", i);
    }
    return RIBBIT_OK;
}

int record_verdicts_impl(RibbitHandle *h, const RibbitTargetShortlists *lists, size_t n_targets, int32_t home, const RibbitPrimerPairParams *pair,
                         const RibbitProductParams *product, const RibbitTargetVerdicts **verdicts) {
    if (!h) return fail(RIBBIT_E_ARG, "null handle");
    int rc;
    if ((rc = check_verdict_args(lists, n_targets, home, pair, product, verdicts))) return rc;
    if (!h->loaded) return fail(RIBBIT_E_STATE, "no record loaded");
    RibbitHandle::RowBufs &buf = h->rows;
    if ((rc = buf.h_verdicts.ensure(std::max<size_t>(n_targets, 1) * sizeof(RibbitTargetVerdicts), true))) return rc;
    RibbitTargetVerdicts *out = reinterpret_cast<RibbitTargetVerdicts *>(buf.h_verdicts.p);
    *verdicts = out;
    if (n_targets == 0) return RIBBIT_OK;
    if (h->length == 0) {
        verdicts_without_sites(lists, n_targets, home, *pair, out);
        return RIBBIT_OK;
    }
    if ((rc = bind_device(h))) return rc;
    const size_t batch = std::min(site_batch(h, SLOTS, *product), n_targets);
    const rb::VerdictLayout at = rb::verdict_layout((int64_t)batch);
    if ((rc = buf.d_work.ensure(at.bytes, true))) return rc;
    if ((rc = buf.h_specific_header.ensure(sizeof(rb::SpecificHeader) / sizeof(uint32_t)))) return rc;
    if ((rc = buf.h_product_header.ensure(sizeof(rb::ProductHeader) / sizeof(uint32_t)))) return rc;
    uint8_t *work = buf.d_work.p;
    std::vector<RibbitPrimer> packed(batch * SLOTS);
    for (size_t from = 0; from < n_targets; from += batch) {
        const size_t m = std::min(batch, n_targets - from);
        // the 16 primers of every target one behind the other, as the kernels index them (every batch ends in a synchronise, so the
        // staging buffer is free again)
        for (size_t i = 0; i < m; ++i) std::memcpy(&packed[i * SLOTS], lists[from + i].left, LIST_BYTES);
        const StageSegment down{packed.data(), m * LIST_BYTES};
        const uint8_t *d_at = nullptr;
        if ((rc = stage_down(h, &down, 1, &d_at))) return rc;
        const RibbitPrimer *d_lists = reinterpret_cast<const RibbitPrimer *>(d_at);
        HIP_TRY(rb::launch_listed_oligos(d_lists, (int64_t)m, work, buf.d_work.cap, at, h->stream));
        HIP_TRY(hipMemcpyAsync(buf.h_specific_header.p, work + at.header, sizeof(rb::SpecificHeader), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));
        const size_t oligos = reinterpret_cast<const rb::SpecificHeader *>(buf.h_specific_header.p)->oligos;
        if (oligos > SLOTS * m) return fail(RIBBIT_E_INTERNAL, "%zu listed primers of %zu targets", oligos, m);
        rb::VerdictLayout use = at;
        if (oligos > 0) {
            SiteSearch found;
            if ((rc = search_sites(h, reinterpret_cast<const RibbitOligo *>(work + at.oligos), oligos, 0, *product, work + at.sites.offset, at.sites.layout.bytes, true, found)))
                return rc;
            use.sites.layout = found.at;
        }
        HIP_TRY(rb::launch_shortlist_verdicts(d_lists, (int64_t)m, home != 0, *pair, *product, work, buf.d_work.cap, use, buf.d_site_lists.p, h->stream));
        HIP_TRY(hipMemcpyAsync(out + from, work + at.verdicts, m * sizeof(RibbitTargetVerdicts), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));
    }
    // what the device returned
    for (size_t i = 0; i < n_targets; ++i) {
        const RibbitTargetVerdicts &v = out[i];
        const int n_left = host_held_places(lists[i].left), n_right = host_held_places(lists[i].right);
        uint64_t tried = 0;
        for (int l = 0; l < n_left; ++l) tried |= (((uint64_t)1 << n_right) - 1) << (8 * l);
        bool good = (v.admissible & ~tried) == 0 && ((v.over | v.other | v.own) & ~v.admissible) == 0 && (v.over & (v.other | v.own)) == 0 && v.records == 1 &&
                    v.home_records == home && v.reserved == 0 && v.first_others >= -1 && (v.admissible != 0 || v.first_others == 0) && (home != 0 || v.own == 0);
        for (size_t k = 0; k < SLOTS; ++k) {
            const bool held = k < SLOTS / 2 ? (int)k < n_left : (int)(k - SLOTS / 2) < n_right;
            good = good && v.forward[k] >= 0 && v.reverse[k] >= 0 && (held || v.forward[k] + v.reverse[k] == 0);
        }
        if (!good) return fail(RIBBIT_E_INTERNAL, "target %zu: the verdicts the GPU gave do not add up", i);
    }
    return RIBBIT_OK;
}

// ---- the host twins
int host_record_shortlists_impl(const char *sequence, int64_t length, const int32_t *intervals, size_t n, const int32_t *targets, size_t n_targets,
                                const RibbitPrimerParams *params, const RibbitPrimerPairParams *pair, RibbitTargetShortlists **lists) {
    int rc;
    if ((rc = check_primer_args(intervals, n, targets, n_targets, params, lists))) return rc;
    if ((rc = check_primer_pair_params(pair))) return rc;
    if ((rc = check_sequence(sequence, length))) return rc;
    const unsigned char *seq = reinterpret_cast<const unsigned char *>(sequence);
    const std::vector<uint8_t> covered = host_covered(length, intervals, n);
    const RibbitPrimerParams prm = *params;
    const RibbitPrimerPairParams prs = *pair;
    Handed<RibbitTargetShortlists> out;
    if ((rc = hand_out<RibbitTargetShortlists>(nullptr, n_targets, false, out))) return rc;
    const unsigned threads = (unsigned)std::max<size_t>(1, std::min<size_t>(rb::host_thread_count(0), n_targets / 4));
    rb::over_pieces(n_targets, threads, [&](size_t lo, size_t hi, unsigned) {
        for (size_t i = lo; i < hi; ++i) host_target_shortlists(seq, covered, flanks_of(targets, i, prm.flank, length), prm, prs, out[i]);
    });
    *lists = out.release();
    return RIBBIT_OK;
}

int host_record_verdicts_impl(const char *sequence, int64_t length, const RibbitTargetShortlists *lists, size_t n_targets, int32_t home, const RibbitPrimerPairParams *pair,
                              const RibbitProductParams *product, RibbitTargetVerdicts **verdicts) {
    int rc;
    if ((rc = check_verdict_args(lists, n_targets, home, pair, product, verdicts))) return rc;
    if ((rc = check_sequence(sequence, length))) return rc;
    const unsigned char *seq = reinterpret_cast<const unsigned char *>(sequence);
    const RibbitPrimerPairParams prs = *pair;
    const RibbitProductParams prd = *product;
    Handed<RibbitTargetVerdicts> out;
    if ((rc = hand_out<RibbitTargetVerdicts>(nullptr, n_targets, false, out))) return rc;
    // every target's admissible pairs from its lists alone
    std::vector<ListedPairs> found(n_targets);
    const unsigned threads = (unsigned)std::max<size_t>(1, std::min<size_t>(rb::host_thread_count(0), n_targets / 4));
    rb::over_pieces(n_targets, threads, [&](size_t lo, size_t hi, unsigned) {
        for (size_t i = lo; i < hi; ++i) listed_pairs(lists[i], prs, found[i]);
    });
    // the sites of every distinct oligo among the held places, each searched once
    HostOligoIndex index;
    std::vector<size_t> oligo_of(n_targets * SLOTS, SIZE_MAX);
    for (size_t i = 0; i < n_targets; ++i)
        for (size_t k = 0; k < SLOTS; ++k) {
            const bool right = k >= SLOTS / 2;
            const RibbitPrimer &p = right ? lists[i].right[k - SLOTS / 2] : lists[i].left[k];
            if ((int)(right ? k - SLOTS / 2 : k) >= host_held_places(right ? lists[i].right : lists[i].left)) continue;
            oligo_of[i * SLOTS + k] = index.add(host_listed_oligo(p, right));
        }
    index.search(seq, length, prd);
    // the judgement
    for (size_t i = 0; i < n_targets; ++i) {
        RibbitTargetVerdicts v{};
        v.admissible = found[i].admissible;
        v.records = 1;
        v.home_records = home;
        for (size_t k = 0; k < SLOTS; ++k)
            if (oligo_of[i * SLOTS + k] != SIZE_MAX) {
                v.forward[k] = (int32_t)index.sites(oligo_of[i * SLOTS + k]).forward.size();
                v.reverse[k] = (int32_t)index.sites(oligo_of[i * SLOTS + k]).reverse.size();
            }
        for (size_t at = 0; at < found[i].ordered.size(); ++at) {
            const RibbitRowPrimerPair &r = found[i].ordered[at];
            const RibbitRowProducts p = host_products_among(index.sites(oligo_of[i * SLOTS + (size_t)r.left_rank]), index.sites(oligo_of[i * SLOTS + SLOTS / 2 + (size_t)r.right_rank]),
                                                            r.left.length, r.right.length, home ? r.left.start : -1, home ? r.right.start : -1, prd);
            const bool over = p.products < 0;
            const int32_t others = over ? -1 : p.products - p.own;
            if (over) v.over |= bit_of(r);
            if (others > 0) v.other |= bit_of(r);
            if (p.own) v.own |= bit_of(r);
            if (at == 0) v.first_others = others;
        }
        out[i] = v;
    }
    *verdicts = out.release();
    return RIBBIT_OK;
}

// ---- the sum and the choice
int verdicts_merge_impl(RibbitTargetVerdicts *into, const RibbitTargetVerdicts *from, size_t n) {
    if ((!into || !from) && n > 0) return fail(RIBBIT_E_ARG, "null argument");
    for (size_t i = 0; i < n; ++i)
        if (into[i].admissible != from[i].admissible) return fail(RIBBIT_E_ARG, "target %zu: the two verdicts are of different admissible pairs", i);
    for (size_t i = 0; i < n; ++i) {
        RibbitTargetVerdicts &a = into[i];
        const RibbitTargetVerdicts &b = from[i];
        a.over |= b.over;
        a.other |= b.other;
        a.own |= b.own;
        for (size_t k = 0; k < SLOTS; ++k) {
            a.forward[k] = saturating_sum(a.forward[k], b.forward[k]);
            a.reverse[k] = saturating_sum(a.reverse[k], b.reverse[k]);
        }
        a.first_others = a.first_others == -1 || b.first_others == -1 ? -1 : saturating_sum(a.first_others, b.first_others);
        a.records = saturating_sum(a.records, b.records);
        a.home_records = saturating_sum(a.home_records, b.home_records);
    }
    return RIBBIT_OK;
}

int popcount(uint64_t v) { return __builtin_popcountll(v); }

int shortlists_choose_impl(const RibbitTargetShortlists *lists, const RibbitTargetVerdicts *verdicts, size_t n, const RibbitPrimerPairParams *pair, RibbitRowPrimerPair **pairs,
                           RibbitRowProducts **products, RibbitRowSpecific **specific) {
    if (((!lists || !verdicts) && n > 0) || !pairs || !products || !specific) return fail(RIBBIT_E_ARG, "null argument");
    if (n > MAX_TARGETS) return fail(RIBBIT_E_ARG, "%zu targets", n);
    int rc;
    if ((rc = check_primer_pair_params(pair))) return rc;
    if ((rc = check_lists(lists, n, pair->shortlist, 1))) return rc;
    for (size_t i = 0; i < n; ++i)
        if (verdicts[i].home_records != 1)
            return fail(RIBBIT_E_ARG, "target %zu: judged on %d home records, not 1", i, (int)verdicts[i].home_records);
    Handed<RibbitRowPrimerPair> out_pairs;
    Handed<RibbitRowProducts> out_products;
    Handed<RibbitRowSpecific> out_specific;
    if ((rc = hand_out<RibbitRowPrimerPair>(nullptr, n, false, out_pairs))) return rc;
    if ((rc = hand_out<RibbitRowProducts>(nullptr, n, false, out_products))) return rc;
    if ((rc = hand_out<RibbitRowSpecific>(nullptr, n, false, out_specific))) return rc;
    // a team of host threads, a piece of the targets each (the 64 duplexes of a target are most of the work); the first target whose
    // verdicts do not fit its lists is refused
    const unsigned threads = (unsigned)std::max<size_t>(1, std::min<size_t>(rb::host_thread_count(0), n / 64));
    std::vector<size_t> unfit(threads, SIZE_MAX);
    const RibbitPrimerPairParams prs = *pair;
    rb::over_pieces(n, threads, [&](size_t lo, size_t hi, unsigned part) {
        ListedPairs found;
        for (size_t i = lo; i < hi; ++i) {
            const RibbitTargetVerdicts &v = verdicts[i];
            listed_pairs(lists[i], prs, found);
            if (found.admissible != v.admissible) {
                unfit[part] = i;
                return;
            }
            RibbitRowSpecific s{};
            s.place = -1;
            s.pairs_admissible = popcount(v.admissible);
            s.pairs_over = popcount(v.over & v.admissible);
            s.pairs_other = popcount(v.other & v.admissible & ~v.over);
            s.pairs_specific = s.pairs_admissible - s.pairs_over - s.pairs_other;
            s.first_products = v.first_others;
            out_pairs[i] = found.none;
            out_products[i] = RibbitRowProducts{};
            for (size_t at = 0; at < found.ordered.size(); ++at) {
                const RibbitRowPrimerPair &r = found.ordered[at];
                if ((v.over | v.other) & bit_of(r)) continue;
                s.place = (int32_t)at;
                out_pairs[i] = r;
                RibbitRowProducts p{};
                p.left_forward = v.forward[r.left_rank];
                p.left_reverse = v.reverse[r.left_rank];
                p.right_forward = v.forward[SLOTS / 2 + (size_t)r.right_rank];
                p.right_reverse = v.reverse[SLOTS / 2 + (size_t)r.right_rank];
                p.own = (v.own & bit_of(r)) ? 1 : 0;
                p.products = p.own;
                out_products[i] = p;
                break;
            }
            out_specific[i] = s;
        }
    });
    const size_t first_unfit = *std::min_element(unfit.begin(), unfit.end());
    if (first_unfit != SIZE_MAX) return fail(RIBBIT_E_ARG, "target %zu: the verdicts are not of these lists' admissible pairs", first_unfit);
    *pairs = out_pairs.release();
    *products = out_products.release();
    *specific = out_specific.release();
    return RIBBIT_OK;
}

}  // namespace

extern "C" {

int ribbit_hip_record_primer_shortlists(RibbitHandle *h, const int32_t *intervals, size_t n, const int32_t *targets, size_t n_targets, const RibbitPrimerParams *params,
                                        const RibbitPrimerPairParams *pair_params, const RibbitTargetShortlists **lists) {
    return guarded("the primer shortlists", [&]() -> int { return record_shortlists_impl(h, intervals, n, targets, n_targets, params, pair_params, lists); });
}

int ribbit_hip_record_shortlist_verdicts(RibbitHandle *h, const RibbitTargetShortlists *lists, size_t n_targets, int32_t home, const RibbitPrimerPairParams *pair_params,
                                         const RibbitProductParams *product_params, const RibbitTargetVerdicts **verdicts) {
    return guarded("the shortlists' verdicts", [&]() -> int { return record_verdicts_impl(h, lists, n_targets, home, pair_params, product_params, verdicts); });
}

int ribbit_host_record_primer_shortlists(const char *sequence, int64_t length, const int32_t *intervals, size_t n, const int32_t *targets, size_t n_targets,
                                         const RibbitPrimerParams *params, const RibbitPrimerPairParams *pair_params, RibbitTargetShortlists **lists) {
    return guarded("the primer shortlists",
                   [&]() -> int { return host_record_shortlists_impl(sequence, length, intervals, n, targets, n_targets, params, pair_params, lists); });
}

int ribbit_host_record_shortlist_verdicts(const char *sequence, int64_t length, const RibbitTargetShortlists *lists, size_t n_targets, int32_t home,
                                          const RibbitPrimerPairParams *pair_params, const RibbitProductParams *product_params, RibbitTargetVerdicts **verdicts) {
    return guarded("the shortlists' verdicts",
                   [&]() -> int { return host_record_verdicts_impl(sequence, length, lists, n_targets, home, pair_params, product_params, verdicts); });
}

int ribbit_primer_verdicts_merge(RibbitTargetVerdicts *into, const RibbitTargetVerdicts *from, size_t n) {
    return guarded("the sum of the shortlists' verdicts", [&]() -> int { return verdicts_merge_impl(into, from, n); });
}

int ribbit_primer_shortlists_choose(const RibbitTargetShortlists *lists, const RibbitTargetVerdicts *verdicts, size_t n, const RibbitPrimerPairParams *pair_params,
                                    RibbitRowPrimerPair **pairs, RibbitRowProducts **products, RibbitRowSpecific **specific) {
    return guarded("the choice among the shortlists", [&]() -> int { return shortlists_choose_impl(lists, verdicts, n, pair_params, pairs, products, specific); });
}

void ribbit_primer_genome_free(void *from_a_host_function) { std::free(from_a_host_function); }

}  // extern "C"
