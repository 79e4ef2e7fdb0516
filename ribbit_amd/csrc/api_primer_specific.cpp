// api_primer_specific.cpp -- the best primer pair of every target of a record that amplifies nothing else in it
// (primer_specific.hip); see api_internal.h for the map of the files behind include/ribbit_hip.h.  The GPU form puts two row outputs
// together: the targets and the rows' coverage go down as for ribbit_hip_record_primer_pairs, and per batch of targets the
// shortlisted primers go through ribbit_hip_record_primer_products' uniques, patterns and site scan without leaving the device
// (the work buffer of those launches is a region of this call's, rb::SpecificLayout).  Two counts the device finds are read in
// the middle of a batch: its oligos, and their unique ones, which size the site lists (the handle's own buffer, as there).
// A batch is as many targets as SPECIFIC_LIST_BYTES of site lists hold at the worst case of 16 distinct oligos per target; every
// batch scans the record once.  After the copy back everything the device returned is checked.
// The host twin works from the bytes of the sequence with the host code behind the two twins it combines (primers_host.h): every
// admissible pair of a target in the order of the choice, the sites of every distinct oligo letter by letter, the pairs walked until
// one is specific.  It shares nothing with the kernels.  The text needs no GPU.
#include "primers_host.h"

#include <map>
#include <string>

namespace {

static_assert(sizeof(RibbitRowSpecific) == 32 && sizeof(RibbitRowProducts) == 32 && sizeof(RibbitRowPrimerPair) == 128, "8, 8 and 32 ints");
constexpr size_t SPECIFIC_LIST_BYTES = (size_t)256 << 20, SLOTS = 2 * RIBBIT_PRIMER_PAIR_SHORTLIST, MAX_BATCH_SITES = (size_t)1 << 29;

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

// the targets of one batch: as many as the site lists' room holds, or what the test asked for, within what one site scan takes
size_t batch_targets(const RibbitHandle *h, const RibbitProductParams &product) {
    const size_t per_target = SLOTS * (size_t)product.max_sites;      // the list slots of a target's patterns of one strand
    const size_t by_rule = std::max<size_t>(1, SPECIFIC_LIST_BYTES / (2 * per_target * sizeof(int32_t)));
    return std::min(h->rows.specific_batch ? h->rows.specific_batch : by_rule, std::max<size_t>(1, MAX_BATCH_SITES / per_target));
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
    const size_t batch = std::min(batch_targets(h, *product), n_targets);
    const rb::SpecificLayout at = rb::specific_layout((int64_t)batch);
    if ((rc = buf.d_work.ensure(at.bytes, true))) return rc;
    if ((rc = buf.h_specific_header.ensure(sizeof(rb::SpecificHeader) / sizeof(uint32_t)))) return rc;
    if ((rc = buf.h_product_header.ensure(sizeof(rb::ProductHeader) / sizeof(uint32_t)))) return rc;
    const StageSegment down{targets, 2 * n_targets * sizeof(int32_t)};
    const uint8_t *d_targets = nullptr;
    if ((rc = stage_down(h, &down, 1, &d_targets))) return rc;
    if ((rc = build_coverage(h, intervals, n))) return rc;
    uint8_t *work = buf.d_work.p, *product_work = work + at.product_work;
    for (size_t from = 0; from < n_targets; from += batch) {
        const size_t m = std::min(batch, n_targets - from);
        HIP_TRY(rb::launch_primer_shortlists(h->planes(), buf.d_mask_bits.p, reinterpret_cast<const int32_t *>(d_targets) + 2 * from, (int64_t)m, *params, *pair, work,
                                             buf.d_work.cap, at, h->stream));
        HIP_TRY(hipMemcpyAsync(buf.h_specific_header.p, work + at.header, sizeof(rb::SpecificHeader), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));
        const size_t oligos = reinterpret_cast<const rb::SpecificHeader *>(buf.h_specific_header.p)->oligos;
        if (oligos > SLOTS * m) return fail(RIBBIT_E_INTERNAL, "%zu shortlisted primers of %zu targets", oligos, m);
        // the site search's own layout for exactly these oligos, inside the room that was set aside for 16 a target
        rb::SpecificLayout use = at;
        if (oligos > 0) {
            use.product = rb::products_layout((int64_t)oligos, 0);
            if (use.product.bytes > at.product.bytes) return fail(RIBBIT_E_INTERNAL, "%zu oligos need %zu bytes, not the %zu set aside", oligos, use.product.bytes, at.product.bytes);
            HIP_TRY(rb::launch_product_uniques(reinterpret_cast<const RibbitOligo *>(work + at.oligos), (int64_t)oligos, *product, product_work, at.product.bytes, use.product,
                                               h->stream));
            HIP_TRY(hipMemcpyAsync(buf.h_product_header.p, product_work + use.product.header, sizeof(rb::ProductHeader), hipMemcpyDeviceToHost, h->stream));
            HIP_TRY(hipStreamSynchronize(h->stream));
            const size_t uniques = reinterpret_cast<const rb::ProductHeader *>(buf.h_product_header.p)->uniques;
            if (uniques < 1 || uniques > oligos) return fail(RIBBIT_E_INTERNAL, "%zu unique oligos of %zu", uniques, oligos);
            // the lists' room is fixed here, by the patterns, and does not grow with the sites the scan finds
            if ((rc = buf.d_site_lists.ensure(2 * uniques * (size_t)product->max_sites, true))) return rc;
            HIP_TRY(rb::launch_product_scan(h->planes(), (int64_t)oligos, (int64_t)uniques, *product, product_work, at.product.bytes, use.product, buf.d_site_lists.p, true,
                                            h->stream));
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
    RibbitRowPrimerPair none;
};

int host_record_specific_impl(const char *sequence, int64_t length, const int32_t *intervals, size_t n, const int32_t *targets, size_t n_targets,
                              const RibbitPrimerParams *params, const RibbitPrimerPairParams *pair, const RibbitProductParams *product, RibbitRowPrimerPair **pairs,
                              RibbitRowProducts **products, RibbitRowSpecific **specific) {
    int rc;
    if ((rc = check_args(intervals, n, targets, n_targets, params, pair, product, pairs, products, specific))) return rc;
    if (length < 0 || length > (int64_t)INT32_MAX) return fail(RIBBIT_E_ARG, "a record of %lld bases", (long long)length);
    if (!sequence && length > 0) return fail(RIBBIT_E_ARG, "bad sequence");
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
    std::map<std::string, size_t> index;
    std::vector<const std::string *> distinct;
    for (const TargetPairs &t : found)
        for (const RibbitRowPrimerPair &r : t.ordered) {
            std::string a, b;
            host_pair_oligos(r, a, b);
            for (const std::string *o : {&a, &b}) {
                const auto at = index.emplace(*o, distinct.size());
                if (at.second) distinct.push_back(&at.first->first);
            }
        }
    std::vector<HostSites> sites(distinct.size());
    const unsigned site_threads = (unsigned)std::max<size_t>(1, std::min<size_t>(rb::host_thread_count(0), distinct.size()));
    rb::over_pieces(distinct.size(), site_threads, [&](size_t lo, size_t hi, unsigned) {
        for (size_t k = lo; k < hi; ++k) sites[k] = host_oligo_sites(seq, length, *distinct[k], prd);
    });
    // the walk
    for (size_t i = 0; i < n_targets; ++i) {
        const TargetPairs &t = found[i];
        RibbitRowSpecific s{};
        s.place = -1;
        s.pairs_admissible = (int32_t)t.ordered.size();
        no_pair_records(t.none, out_pairs[i], out_products[i]);
        for (size_t at = 0; at < t.ordered.size(); ++at) {
            const RibbitRowPrimerPair &r = t.ordered[at];
            std::string a, b;
            host_pair_oligos(r, a, b);
            const RibbitRowProducts p = host_products_among(sites[index.at(a)], sites[index.at(b)], r.left.length, r.right.length, r.left.start, r.right.start, prd);
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
enum : int { BAD_LENGTH = 1 };

int bed_primer_specific_text_impl(const char *bed, size_t bed_len, const RibbitRowPrimerPair *pairs, const RibbitRowProducts *products, const RibbitRowSpecific *specific,
                                  size_t n, char **text, size_t *len) {
    if (!text || !len || (!bed && bed_len > 0) || ((!pairs || !products || !specific) && n > 0)) return fail(RIBBIT_E_ARG, "null argument");
    const size_t parts = bed_text_parts(bed_len);
    BedLines lines;
    int rc;
    if ((rc = lines.find(bed, bed_len, parts))) return rc;
    if (lines.count() != n) return fail(RIBBIT_E_ARG, "the BED text has %zu lines, not the %zu of the rows", lines.count(), n);
    return write_pieces(
        parts, "the rows' specific primer pairs", text, len,
        [&](size_t k, std::string &out) {
            const size_t from = n * k / parts, to = n * (k + 1) / parts;
            out.reserve(lines.start[to] - lines.start[from] + 288 * (to - from));
            for (size_t i = from; i < to; ++i) {
                const RibbitRowPrimerPair &r = pairs[i];
                const RibbitRowSpecific &s = specific[i];
                if (const RibbitPrimer *bad = bad_primer(r)) return PieceRefusal{BAD_LENGTH, i, (size_t)(uint32_t)bad->length};
                put_field(out, lines[i]);
                put_pair_columns(out, r);
                put_product_columns(out, r, products[i]);
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
                out += '\n';
            }
            return PieceRefusal{};
        },
        [](const PieceRefusal &bad) { return fail(RIBBIT_E_ARG, "row %zu: a primer of %d bases, not 1 .. %d", bad.a, (int)(int32_t)(uint32_t)bad.b, RIBBIT_PRIMER_MAX_LENGTH); });
}

}  // namespace

// ---- what api_primer_genome.cpp takes from here (primers_host.h)
size_t rbapi::specific_batch_targets(const RibbitHandle *h, const RibbitProductParams &product) { return batch_targets(h, product); }

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
