// api_primer_specific.cpp -- the best primer pair of every target of a record that amplifies nothing else in it
// (primer_specific.hip); see api_internal.h for the map of the files behind include/ribbit_hip.h.  The GPU form puts two row outputs
// together: the targets and the rows' coverage go down as for ribbit_hip_record_primer_pairs, and per batch of targets the
// shortlisted primers go through the site search of ribbit_hip_record_primer_products without leaving the device (search_sites,
// api_internal.h; its work buffer is a region of this call's, rb::SpecificLayout::sites).  A batch's number of oligos is read in
// the middle of it.  A batch is as many targets as site_batch gives at 16 oligos per target; every batch scans the record once.
// After the copy back everything the device returned is checked.
// The host twin works from the bytes of the sequence with the host code behind the two twins it combines (primers_host.h): every
// admissible pair of a target in the order of the choice, the sites of every distinct oligo letter by letter, the pairs walked until
// one is specific.  It shares nothing with the kernels.  The text needs no GPU.
#include "primers_host.h"

#include <string>

namespace {

static_assert(sizeof(RibbitRowSpecific) == 32 && sizeof(RibbitRowProducts) == 32 && sizeof(RibbitRowPrimerPair) == 128, "8, 8 and 32 ints");

int check_args(const int32_t *intervals, size_t n, const int32_t *targets, size_t n_targets, const RibbitPrimerParams *params, const RibbitPrimerPairParams *pair,
               const RibbitProductParams *product, const void *pairs, const void *products, const void *specific) {
    if (!products || !specific) return fail(RIBBIT_E_ARG, "null argument");
    int rc;
    if ((rc = check_primer_args(intervals, n, targets, n_targets, params, pairs))) return rc;
    if ((rc = check_primer_pair_params(pair))) return rc;
    if ((rc = check_primer_product_params(product))) return rc;
    if (params->min_length < product->seed) return fail(RIBBIT_E_ARG, "min_length %d is below seed %d: a primer would be shorter than the seed", (int)params->min_length, (int)product->seed);
    return RIBBIT_OK;
}

void no_pair_records(const RibbitRowPrimerPair &counts, RibbitRowPrimerPair &pair, RibbitRowProducts &products) {
    pair = RibbitRowPrimerPair{};
    pair.left = pair.right = NO_PRIMER;
    pair.left_candidates = counts.left_candidates;
    pair.right_candidates = counts.right_candidates;
    pair.left_passed = counts.left_passed;
    pair.right_passed = counts.right_passed;
    pair.pairs_tried = counts.pairs_tried;
    pair.pairs_admissible = counts.pairs_admissible;
    products = RibbitRowProducts{};
}

int record_specific_impl(RibbitHandle *h, const int32_t *intervals, size_t n, const int32_t *targets, size_t n_targets, const RibbitPrimerParams *params,
                         const RibbitPrimerPairParams *pair, const RibbitProductParams *product, const RibbitRowPrimerPair **pairs, const RibbitRowProducts **products,
                         const RibbitRowSpecific **specific) {
    if (!h) return fail(RIBBIT_E_ARG, "null handle");
    int rc;
    if ((rc = check_args(intervals, n, targets, n_targets, params, pair, product, pairs, products, specific))) return rc;
    if (!h->loaded) return fail(RIBBIT_E_STATE, "no record loaded");
    RibbitHandle::RowBufs &buf = h->rows;
    const size_t room = std::max<size_t>(n_targets, 1);
    if ((rc = buf.h_specific.ensure(room * (sizeof(RibbitRowPrimerPair) + sizeof(RibbitRowProducts) + sizeof(RibbitRowSpecific)), true))) return rc;
    RibbitRowPrimerPair *out_pairs = reinterpret_cast<RibbitRowPrimerPair *>(buf.h_specific.p);
    RibbitRowProducts *out_products = reinterpret_cast<RibbitRowProducts *>(out_pairs + room);
    RibbitRowSpecific *out_specific = reinterpret_cast<RibbitRowSpecific *>(out_products + room);
    *pairs = out_pairs;
    *products = out_products;
    *specific = out_specific;
    if (n_targets == 0) return RIBBIT_OK;
    const int64_t length = h->length;
    if (length == 0) {      // (every flank is empty)
        RibbitRowSpecific none{};
        none.place = -1;
        for (size_t i = 0; i < n_targets; ++i) {
            no_pair_records(RibbitRowPrimerPair{}, out_pairs[i], out_products[i]);
            out_specific[i] = none;
        }
        return RIBBIT_OK;
    }
    if ((rc = bind_device(h))) return rc;
    const size_t batch = std::min(site_batch(h, rb::SLOTS, *product), n_targets);
    const rb::SpecificLayout at = rb::specific_layout((int64_t)batch);
    if ((rc = buf.d_work.ensure(at.bytes, true))) return rc;
    if ((rc = buf.h_specific_header.ensure(sizeof(rb::SpecificHeader) / sizeof(uint32_t)))) return rc;
    if ((rc = buf.h_product_header.ensure(sizeof(rb::ProductHeader) / sizeof(uint32_t)))) return rc;
    const StageSegment down{targets, 2 * n_targets * sizeof(int32_t)};
    const uint8_t *d_targets = nullptr;
    if ((rc = stage_down(h, &down, 1, &d_targets))) return rc;
    if ((rc = build_coverage(h, intervals, n))) return rc;
    uint8_t *work = buf.d_work.p;
    for (size_t from = 0; from < n_targets; from += batch) {
        const size_t m = std::min(batch, n_targets - from);
        HIP_TRY(rb::launch_primer_shortlists(h->planes(), buf.d_mask_bits.p, reinterpret_cast<const int32_t *>(d_targets) + 2 * from, (int64_t)m, *params, *pair, work,
                                             buf.d_work.cap, at, h->stream));
        HIP_TRY(hipMemcpyAsync(buf.h_specific_header.p, work + at.header, sizeof(rb::SpecificHeader), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));
        const size_t oligos = reinterpret_cast<const rb::SpecificHeader *>(buf.h_specific_header.p)->oligos;
        if (oligos > rb::SLOTS * m) return fail(RIBBIT_E_INTERNAL, "%zu shortlisted primers of %zu targets", oligos, m);
        rb::SpecificLayout use = at;
        if (oligos > 0) {
            SiteSearch found;
            if ((rc = search_sites(h, reinterpret_cast<const RibbitOligo *>(work + at.oligos), oligos, 0, *product, work + at.sites.offset, at.sites.layout.bytes, true, found)))
                return rc;
            use.sites.layout = found.at;
        }
        HIP_TRY(rb::launch_specific_pairs((int64_t)m, *pair, *product, work, buf.d_work.cap, use, buf.d_site_lists.p, h->stream));
        HIP_TRY(hipMemcpyAsync(out_pairs + from, work + at.pairs, m * sizeof(RibbitRowPrimerPair), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipMemcpyAsync(out_products + from, work + at.products, m * sizeof(RibbitRowProducts), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipMemcpyAsync(out_specific + from, work + at.specific, m * sizeof(RibbitRowSpecific), hipMemcpyDeviceToHost, h->stream));
    }
    HIP_TRY(hipStreamSynchronize(h->stream));
    // what the device returned
    for (size_t i = 0; i < n_targets; ++i) {
        const RibbitRowPrimerPair &r = out_pairs[i];
        const RibbitRowProducts &p = out_products[i];
        const RibbitRowSpecific &s = out_specific[i];
        const Flanks f = flanks_of(targets, i, params->flank, length);
        const auto inside = [&](const RibbitPrimer &q, int64_t lo, int64_t hi) {
            return q.length >= params->min_length && q.length <= params->max_length && q.start >= lo && (int64_t)q.start + q.length <= hi;
        };
        bool good = s.pairs_specific >= 0 && s.pairs_over >= 0 && s.pairs_other >= 0 && s.pairs_admissible == s.pairs_specific + s.pairs_over + s.pairs_other &&
                    s.pairs_admissible == r.pairs_admissible && r.pairs_admissible <= r.pairs_tried && r.left_passed <= r.left_candidates &&
                    r.right_passed <= r.right_candidates && s.reserved[0] == 0 && s.reserved[1] == 0 && s.place >= -1 && (s.place < 0 || s.place < s.pairs_admissible) &&
                    (s.place >= 0) == (s.pairs_specific > 0) && s.first_products >= -1 && (s.pairs_admissible > 0 || s.first_products == 0) &&
                    (s.place != 0 || s.first_products == 0);
        if (s.place >= 0) {
            good = good && r.left.start >= 0 && r.right.start >= 0 && inside(r.left, f.lo, f.s) && inside(r.right, f.e, f.hi) && p.products >= 0 && p.products - p.own == 0 &&
                   p.shortest_other == 0 && p.reserved == 0 && std::min(std::min(p.left_forward, p.left_reverse), std::min(p.right_forward, p.right_reverse)) >= 0 &&
                   std::max(std::max(p.left_forward, p.left_reverse), std::max(p.right_forward, p.right_reverse)) <= product->max_sites;
        } else {
            good = good && r.left.start == -1 && r.right.start == -1 && r.left.length == 0 && r.right.length == 0 &&
                   p.left_forward + p.left_reverse + p.right_forward + p.right_reverse + p.products + p.own + p.shortest_other + p.reserved == 0;
        }
        if (!good) return fail(RIBBIT_E_INTERNAL, "target %zu: the pairs the GPU counted do not add up", i);
    }
    return RIBBIT_OK;
}

// ---- host twin
struct TargetPairs {
    std::vector<RibbitRowPrimerPair> ordered;
    std::vector<size_t> oligos;      // the ids of every ordered pair's two oligos in the twin's index
    RibbitRowPrimerPair none;
};

int host_record_specific_impl(const char *sequence, int64_t length, const int32_t *intervals, size_t n, const int32_t *targets, size_t n_targets,
                              const RibbitPrimerParams *params, const RibbitPrimerPairParams *pair, const RibbitProductParams *product, RibbitRowPrimerPair **pairs,
                              RibbitRowProducts **products, RibbitRowSpecific **specific) {
    int rc;
    if ((rc = check_args(intervals, n, targets, n_targets, params, pair, product, pairs, products, specific))) return rc;
    if ((rc = check_sequence(sequence, length))) return rc;
    const unsigned char *seq = reinterpret_cast<const unsigned char *>(sequence);
    const std::vector<uint8_t> covered = host_covered(length, intervals, n);
    const RibbitPrimerParams prm = *params;
    const RibbitPrimerPairParams prs = *pair;
    const RibbitProductParams prd = *product;
    Handed<RibbitRowPrimerPair> out_pairs;
    Handed<RibbitRowProducts> out_products;
    Handed<RibbitRowSpecific> out_specific;
    if ((rc = hand_out<RibbitRowPrimerPair>(nullptr, n_targets, false, out_pairs))) return rc;
    if ((rc = hand_out<RibbitRowProducts>(nullptr, n_targets, false, out_products))) return rc;
    if ((rc = hand_out<RibbitRowSpecific>(nullptr, n_targets, false, out_specific))) return rc;
    // every target's admissible pairs in the order of the choice
    std::vector<TargetPairs> found(n_targets);
    const unsigned threads = (unsigned)std::max<size_t>(1, std::min<size_t>(rb::host_thread_count(0), n_targets / 4));
    rb::over_pieces(n_targets, threads, [&](size_t lo, size_t hi, unsigned) {
        for (size_t i = lo; i < hi; ++i) host_ordered_pairs(seq, covered, flanks_of(targets, i, prm.flank, length), prm, prs, found[i].ordered, found[i].none);
    });
    // the sites of every distinct oligo among them, each searched once
    HostOligoIndex index;
    for (TargetPairs &t : found)
        for (const RibbitRowPrimerPair &r : t.ordered) {
            std::string a, b;
            host_pair_oligos(r, a, b);
            t.oligos.push_back(index.add(a));
            t.oligos.push_back(index.add(b));
        }
    index.search(seq, length, prd);
    // the walk
    for (size_t i = 0; i < n_targets; ++i) {
        const TargetPairs &t = found[i];
        RibbitRowSpecific s{};
        s.place = -1;
        s.pairs_admissible = (int32_t)t.ordered.size();
        no_pair_records(t.none, out_pairs[i], out_products[i]);
        for (size_t at = 0; at < t.ordered.size(); ++at) {
            const RibbitRowPrimerPair &r = t.ordered[at];
            const RibbitRowProducts p = host_products_among(index.sites(t.oligos[2 * at]), index.sites(t.oligos[2 * at + 1]), r.left.length, r.right.length, r.left.start,
                                                            r.right.start, prd);
            const bool over = p.products < 0, is_specific = !over && p.products - p.own == 0;
            if (at == 0) s.first_products = over ? -1 : p.products - p.own;
            s.pairs_over += over;
            s.pairs_specific += is_specific;
            s.pairs_other += !over && !is_specific;
            if (is_specific && s.place < 0) {
                s.place = (int32_t)at;
                out_pairs[i] = r;
                out_products[i] = p;
            }
        }
        out_specific[i] = s;
    }
    *pairs = out_pairs.release();
    *products = out_products.release();
    *specific = out_specific.release();
    return RIBBIT_OK;
}

// ---- the text
int bed_primer_specific_text_impl(const char *bed, size_t bed_len, const RibbitRowPrimerPair *pairs, const RibbitRowProducts *products, const RibbitRowSpecific *specific,
                                  size_t n, char **text, size_t *len) {
    if (!text || !len || (!bed && bed_len > 0) || ((!pairs || !products || !specific) && n > 0)) return fail(RIBBIT_E_ARG, "null argument");
    return bed_pair_rows_text(bed, bed_len, pairs, n, "the rows' specific primer pairs", 288, text, len, [&](std::string &out, size_t i) {
        const RibbitRowSpecific &s = specific[i];
        put_product_columns(out, pairs[i], products[i]);
        if (s.place < 0) {
            out += "\t.";
        } else {
            out += '\t';
            put_number(out, s.place);
        }
        for (const int32_t v : {s.pairs_specific, s.pairs_over, s.pairs_other}) {
            out += '\t';
            put_number(out, v);
        }
    });
}

}  // namespace

extern "C" {

int ribbit_hip_record_specific_primer_pairs(RibbitHandle *h, const int32_t *intervals, size_t n, const int32_t *targets, size_t n_targets, const RibbitPrimerParams *params,
                                            const RibbitPrimerPairParams *pair_params, const RibbitProductParams *product_params, const RibbitRowPrimerPair **pairs,
                                            const RibbitRowProducts **products, const RibbitRowSpecific **specific) {
    return guarded("the specific primer pairs",
                   [&]() -> int { return record_specific_impl(h, intervals, n, targets, n_targets, params, pair_params, product_params, pairs, products, specific); });
}

int ribbit_host_record_specific_primer_pairs(const char *sequence, int64_t length, const int32_t *intervals, size_t n, const int32_t *targets, size_t n_targets,
                                             const RibbitPrimerParams *params, const RibbitPrimerPairParams *pair_params, const RibbitProductParams *product_params,
                                             RibbitRowPrimerPair **pairs, RibbitRowProducts **products, RibbitRowSpecific **specific) {
    return guarded("the specific primer pairs", [&]() -> int {
        return host_record_specific_impl(sequence, length, intervals, n, targets, n_targets, params, pair_params, product_params, pairs, products, specific);
    });
}

void ribbit_primer_specific_free(void *from_the_host_twin) { std::free(from_the_host_twin); }

int ribbit_hip_debug_set_specific_batch(RibbitHandle *h, size_t targets) {
    if (!h) return fail(RIBBIT_E_ARG, "null handle");
    h->rows.specific_batch = targets;
    return RIBBIT_OK;
}

int ribbit_bed_primer_specific_text(const char *bed_text, size_t bed_len, const RibbitRowPrimerPair *pairs, const RibbitRowProducts *products,
                                    const RibbitRowSpecific *specific, size_t n, char **text, size_t *len) {
    return guarded("the rows' specific primer pairs as text",
                   [&]() -> int { return bed_primer_specific_text_impl(bed_text, bed_len, pairs, products, specific, n, text, len); });
}

}  // extern "C"
