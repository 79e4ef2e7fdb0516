// api_amplicons.cpp -- every chosen primer pair typed on any loaded record: the sites of its two oligos, its products, where the
// first of them lies and the repeat tract inside it (amplicons.hip); see api_internal.h for the map of the files behind
// include/ribbit_hip.h.  The GPU form serves the pairs in batches by the rule of ribbit_hip_record_specific_primer_pairs (site_batch,
// api_internal.h), with two oligos per pair: a batch's oligos, its pairs and its motifs go down through stage_down, the oligos go
// through the site search of ribbit_hip_record_primer_products (search_sites; its work buffer is a region of this call's,
// rb::AmpliconLayout::sites), and two kernels fill the records.  After the copy back everything the device returned is checked.
// The host twin works from the bytes of the sequence with the host code behind the products' twin (primers_host.h): every pair of
// sites walked for the least key, the tract found as the contract first states it, every phase of both strands tried letter by
// letter.  It shares nothing with the kernels.  The sum and the text need no GPU.
#include "primers_host.h"

#include <string>

namespace {

static_assert(sizeof(RibbitRowAmplicon) == 64 && sizeof(RibbitRowPrimerPair) == 128, "16 and 32 ints");
constexpr int32_t MAX_MOTIF = 1023;

RibbitRowAmplicon no_amplicon() {
    RibbitRowAmplicon a{};
    a.record = a.start = a.end = a.inner_start = a.inner_end = a.tract_start = a.tract_end = -1;
    return a;
}

// the motifs as ribbit_hip_record_classes takes them, with its wording
int check_motifs(const char *motifs, const int32_t *offsets, size_t n) {
    if (n == 0) return RIBBIT_OK;
    if (!offsets) return fail(RIBBIT_E_ARG, "null argument");
    if (offsets[0] != 0) return fail(RIBBIT_E_ARG, "the motifs' offsets start at %d, not at 0", (int)offsets[0]);
    for (size_t i = 0; i < n; ++i) {
        const int64_t k = (int64_t)offsets[i + 1] - offsets[i];
        if (!motifs) return fail(RIBBIT_E_ARG, "null argument");
        if (k < 0) return fail(RIBBIT_E_ARG, "row %zu: the motifs' offsets do not ascend (%d, then %d; a pool has fewer than 2^31 bytes)", i, (int)offsets[i], (int)offsets[i + 1]);
        if (k == 0) return fail(RIBBIT_E_ARG, "row %zu: an empty motif", i);
        if (k > MAX_MOTIF) return fail(RIBBIT_E_ARG, "row %zu: a motif of %lld bytes (at most %d)", i, (long long)k, (int)MAX_MOTIF);
        for (int64_t j = 0; j < k; ++j) {
            const char c = motifs[offsets[i] + j];
            if (c != 'A' && c != 'C' && c != 'G' && c != 'T') return fail(RIBBIT_E_ARG, "row %zu: a motif with a byte outside ACGT", i);
        }
    }
    return RIBBIT_OK;
}

int check_args(const RibbitRowPrimerPair *pairs, size_t n, const char *motifs, const int32_t *offsets, int32_t record, const RibbitProductParams *params, const void *rows) {
    if (!rows) return fail(RIBBIT_E_ARG, "null argument");
    int rc;
    if ((rc = check_product_pairs(pairs, n, params))) return rc;
    if (record < 0) return fail(RIBBIT_E_ARG, "record %d is below 0", (int)record);
    return check_motifs(motifs, offsets, n);
}

int record_amplicons_impl(RibbitHandle *h, const RibbitRowPrimerPair *pairs, size_t n, const char *motifs, const int32_t *offsets, int32_t record,
                          const RibbitProductParams *params, const RibbitRowAmplicon **rows) {
    if (!h) return fail(RIBBIT_E_ARG, "null handle");
    int rc;
    if ((rc = check_args(pairs, n, motifs, offsets, record, params, rows))) return rc;
    if (!h->loaded) return fail(RIBBIT_E_STATE, "no record loaded");
    RibbitHandle::RowBufs &buf = h->rows;
    if ((rc = buf.h_amplicons.ensure(std::max<size_t>(n, 1) * sizeof(RibbitRowAmplicon), true))) return rc;
    RibbitRowAmplicon *out = reinterpret_cast<RibbitRowAmplicon *>(buf.h_amplicons.p);
    *rows = out;
    if (n == 0) return RIBBIT_OK;
    std::fill(out, out + n, no_amplicon());
    const int64_t length = h->length;
    if (length == 0) return RIBBIT_OK;      // (no window fits: no sites, no products)
    if ((rc = bind_device(h))) return rc;
    const size_t batch = std::min(site_batch(h, 2, *params), n);
    const rb::AmpliconLayout at = rb::amplicon_layout((int64_t)batch);
    if ((rc = buf.d_work.ensure(at.bytes, true))) return rc;
    if ((rc = buf.h_product_header.ensure(sizeof(rb::ProductHeader) / sizeof(uint32_t)))) return rc;
    uint8_t *work = buf.d_work.p;
    std::vector<RibbitOligo> oligos;
    std::vector<int32_t> quads;
    for (size_t from = 0; from < n; from += batch) {
        const size_t m = std::min(batch, n - from);
        // the oligos of the pairs that have any, two each, and for every pair {a's oligo, b's oligo, -1, -1}: no product is its own
        oligos.clear();
        quads.assign(4 * m, -1);
        for (size_t i = 0; i < m; ++i) {
            if (!has_pair(pairs[from + i])) continue;
            RibbitOligo a, b;
            pair_oligos(pairs[from + i], a, b);
            quads[4 * i] = (int32_t)oligos.size();
            quads[4 * i + 1] = (int32_t)oligos.size() + 1;
            oligos.push_back(a);
            oligos.push_back(b);
        }
        if (oligos.empty()) continue;
        const StageSegment down[4] = {{oligos.data(), oligos.size() * sizeof(RibbitOligo)},
                                      {quads.data(), quads.size() * sizeof(int32_t)},
                                      {offsets + from, (m + 1) * sizeof(int32_t)},
                                      {motifs + offsets[from], (size_t)(offsets[from + m] - offsets[from])}};
        const uint8_t *d_at[4] = {nullptr, nullptr, nullptr, nullptr};
        if ((rc = stage_down(h, down, 4, d_at))) return rc;
        SiteSearch found;
        if ((rc = search_sites(h, reinterpret_cast<const RibbitOligo *>(d_at[0]), oligos.size(), 0, *params, work + at.sites.offset, at.sites.layout.bytes, true, found))) return rc;
        rb::AmpliconLayout use = at;
        use.sites.layout = found.at;
        HIP_TRY(rb::launch_pair_amplicons(h->planes(), reinterpret_cast<const int32_t *>(d_at[1]), (int64_t)m, d_at[3], reinterpret_cast<const int32_t *>(d_at[2]), record,
                                          *params, work, buf.d_work.cap, use, buf.d_site_lists.p, h->stream));
        HIP_TRY(hipMemcpyAsync(out + from, work + at.rows, m * sizeof(RibbitRowAmplicon), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));
    }
    // what the device returned
    for (size_t i = 0; i < n; ++i) {
        const RibbitRowAmplicon &a = out[i];
        bool good = a.reserved == 0;
        for (const int32_t c : {a.left_forward, a.left_reverse, a.right_forward, a.right_reverse}) good = good && c >= 0 && c <= length;
        const bool over = std::max(std::max(a.left_forward, a.left_reverse), std::max(a.right_forward, a.right_reverse)) > params->max_sites;
        good = good && (over ? a.products == -1 : a.products >= 0);
        if (!has_pair(pairs[i])) good = good && a.left_forward + a.left_reverse + a.right_forward + a.right_reverse + a.products == 0;
        if (a.products > 0) {
            const int64_t k = (int64_t)offsets[i + 1] - offsets[i];
            good = good && a.record == record && a.start >= 0 && a.start < a.inner_start && a.inner_start <= a.inner_end && a.inner_end < a.end && a.end <= length &&
                   (int64_t)a.end - a.start <= params->max_product && (a.forward_of | 1) == 1 && (a.reverse_of | 1) == 1 && (a.tract_strand | 1) == 1;
            good = good && (a.tract_start < 0 ? a.tract_start == -1 && a.tract_end == -1 && a.tract_strand == 0
                                              : a.tract_start >= a.inner_start && a.tract_end <= a.inner_end && (int64_t)a.tract_end - a.tract_start >= 2 * k);
        } else {
            good = good && a.record == -1 && a.start == -1 && a.end == -1 && a.inner_start == -1 && a.inner_end == -1 && a.tract_start == -1 && a.tract_end == -1 &&
                   a.forward_of == 0 && a.reverse_of == 0 && a.tract_strand == 0;
        }
        if (!good) return fail(RIBBIT_E_INTERNAL, "pair %zu: the amplicon the GPU placed does not add up", i);
    }
    return RIBBIT_OK;
}

// ---- the host twin, in letters
struct Site { int64_t x, k; int32_t of; };

// the longest stretch of [is, ie) that reads as the motif repeated, at any phase, on either strand: every phase walked on its own
void host_tract(const unsigned char *seq, int64_t is, int64_t ie, const std::string &w, RibbitRowAmplicon &a) {
    const int64_t m = (int64_t)w.size();
    int64_t best_start = -1, best_len = 0;
    int32_t best_strand = 0;
    const std::string strands[2] = {w, reverse_complement(w)};
    for (int32_t strand = 0; strand < 2; ++strand)
        for (int64_t phase = 0; phase < m; ++phase) {
            // position x reads as this strand's letter (phase + x - is) mod m
            int64_t run_from = is;
            for (int64_t x = is; x <= ie; ++x) {
                const bool fits = x < ie && letter_at(seq, x) == strands[strand][(size_t)((phase + x - is) % m)];
                if (fits) continue;
                const int64_t len = x - run_from;
                if (len >= 2 * m && (len > best_len || (len == best_len && run_from < best_start))) {
                    best_start = run_from;
                    best_len = len;
                    best_strand = strand;
                }
                run_from = x + 1;
            }
        }
    if (best_start >= 0) {
        a.tract_start = (int32_t)best_start;
        a.tract_end = (int32_t)(best_start + best_len);
        a.tract_strand = best_strand;
    }
}

RibbitRowAmplicon amplicon_of(const unsigned char *seq, int64_t length, const RibbitRowPrimerPair &pair, const std::string &motif, int32_t record,
                              const RibbitProductParams &prm) {
    RibbitRowAmplicon a = no_amplicon();
    if (!has_pair(pair)) return a;
    std::string oa, ob;
    host_pair_oligos(pair, oa, ob);
    const HostSites sa = host_oligo_sites(seq, length, oa, prm), sb = host_oligo_sites(seq, length, ob, prm);
    a.left_forward = (int32_t)sa.forward.size();
    a.left_reverse = (int32_t)sa.reverse.size();
    a.right_forward = (int32_t)sb.forward.size();
    a.right_reverse = (int32_t)sb.reverse.size();
    if (std::max(std::max(a.left_forward, a.left_reverse), std::max(a.right_forward, a.right_reverse)) > prm.max_sites) {
        a.products = -1;
        return a;
    }
    std::vector<Site> forward, reverse;
    for (const int32_t x : sa.forward) forward.push_back(Site{x, (int64_t)oa.size(), 0});
    for (const int32_t x : sb.forward) forward.push_back(Site{x, (int64_t)ob.size(), 1});
    for (const int32_t x : sa.reverse) reverse.push_back(Site{x, (int64_t)oa.size(), 0});
    for (const int32_t x : sb.reverse) reverse.push_back(Site{x, (int64_t)ob.size(), 1});
    const Site *first_f = nullptr, *first_v = nullptr;
    for (const Site &f : forward)
        for (const Site &v : reverse) {
            if (f.x + f.k > v.x || v.x + v.k - f.x > prm.max_product) continue;
            ++a.products;
            bool less = !first_f;
            if (!less) {
                const int64_t mine[4] = {f.x, v.x + v.k, f.of, v.of}, held[4] = {first_f->x, first_v->x + first_v->k, first_f->of, first_v->of};
                less = std::lexicographical_compare(mine, mine + 4, held, held + 4);
            }
            if (less) {
                first_f = &f;
                first_v = &v;
            }
        }
    if (a.products == 0) return a;
    a.record = record;
    a.start = (int32_t)first_f->x;
    a.end = (int32_t)(first_v->x + first_v->k);
    a.forward_of = first_f->of;
    a.reverse_of = first_v->of;
    a.inner_start = (int32_t)(first_f->x + first_f->k);
    a.inner_end = (int32_t)first_v->x;
    host_tract(seq, a.inner_start, a.inner_end, motif, a);
    return a;
}

int host_record_amplicons_impl(const char *sequence, int64_t length, const RibbitRowPrimerPair *pairs, size_t n, const char *motifs, const int32_t *offsets, int32_t record,
                               const RibbitProductParams *params, RibbitRowAmplicon **rows) {
    int rc;
    if ((rc = check_args(pairs, n, motifs, offsets, record, params, rows))) return rc;
    if ((rc = check_sequence(sequence, length))) return rc;
    const unsigned char *seq = reinterpret_cast<const unsigned char *>(sequence);
    const RibbitProductParams prm = *params;
    Handed<RibbitRowAmplicon> out;
    if ((rc = hand_out<RibbitRowAmplicon>(nullptr, n, false, out))) return rc;
    const unsigned threads = (unsigned)std::max<size_t>(1, std::min<size_t>(rb::host_thread_count(0), n));
    rb::over_pieces(n, threads, [&](size_t lo, size_t hi, unsigned) {
        for (size_t i = lo; i < hi; ++i)
            out[i] = amplicon_of(seq, length, pairs[i], std::string(motifs + offsets[i], (size_t)(offsets[i + 1] - offsets[i])), record, prm);
    });
    *rows = out.release();
    return RIBBIT_OK;
}

// ---- the sum over records
int amplicons_merge_impl(RibbitRowAmplicon *into, const RibbitRowAmplicon *from, size_t n) {
    if ((!into || !from) && n > 0) return fail(RIBBIT_E_ARG, "null argument");
    for (size_t i = 0; i < n; ++i) {
        const RibbitRowAmplicon a = into[i], &b = from[i];
        RibbitRowAmplicon sum = a.products > 0 ? a : b;      // (the first record's product)
        sum.left_forward = saturating_sum(a.left_forward, b.left_forward);
        sum.left_reverse = saturating_sum(a.left_reverse, b.left_reverse);
        sum.right_forward = saturating_sum(a.right_forward, b.right_forward);
        sum.right_reverse = saturating_sum(a.right_reverse, b.right_reverse);
        sum.products = a.products == -1 || b.products == -1 ? -1 : saturating_sum(a.products, b.products);
        if (sum.products <= 0) {
            const RibbitRowAmplicon counts = sum;
            sum = no_amplicon();
            sum.left_forward = counts.left_forward;
            sum.left_reverse = counts.left_reverse;
            sum.right_forward = counts.right_forward;
            sum.right_reverse = counts.right_reverse;
            sum.products = counts.products;
        }
        into[i] = sum;
    }
    return RIBBIT_OK;
}

// ---- the text
enum : int { BAD_LENGTH = 1, NOT_A_ROW = 2, BAD_RECORD = 3 };

int bed_marker_text_impl(const char *bed, size_t bed_len, const RibbitRowPrimerPair *pairs, const RibbitRowAmplicon *amplicons, const char *names,
                         const int32_t *name_offsets, size_t n_records, size_t n, char **text, size_t *len) {
    if (!text || !len || (!bed && bed_len > 0) || ((!pairs || !amplicons) && n > 0) || ((!names || !name_offsets) && n_records > 0)) return fail(RIBBIT_E_ARG, "null argument");
    if (n_records > (size_t)INT32_MAX) return fail(RIBBIT_E_ARG, "%zu records", n_records);
    for (size_t k = 0; k < n_records; ++k)
        if (name_offsets[k] < 0 || name_offsets[k + 1] < name_offsets[k]) return fail(RIBBIT_E_ARG, "record %zu: the names' offsets do not ascend", k);
    const size_t parts = bed_text_parts(bed_len);
    BedLines lines;
    int rc;
    if ((rc = lines.find(bed, bed_len, parts))) return rc;
    if (lines.count() != n) return fail(RIBBIT_E_ARG, "the BED text has %zu lines, not the %zu of the rows", lines.count(), n);
    return write_pieces(
        parts, "the rows' markers", text, len,
        [&](size_t k, std::string &out) {
            const size_t from = n * k / parts, to = n * (k + 1) / parts;
            out.reserve(lines.start[to] - lines.start[from] + 256 * (to - from));
            for (size_t i = from; i < to; ++i) {
                const RibbitRowPrimerPair &r = pairs[i];
                const RibbitRowAmplicon &a = amplicons[i];
                if (const RibbitPrimer *bad = bad_primer(r)) return PieceRefusal{BAD_LENGTH, i, (size_t)(uint32_t)bad->length};
                const BedField line = lines[i];
                const BedRow row = bed_row(line.from, line.to);
                if (!row.ok || row.motif.size() == 0) return PieceRefusal{NOT_A_ROW, i, 0};
                if (a.products > 0 && (a.record < 0 || (size_t)a.record >= n_records)) return PieceRefusal{BAD_RECORD, i, (size_t)(uint32_t)a.record};
                put_field(out, line);
                if (r.left.start < 0 || r.right.start < 0) {
                    for (int c = 0; c < 20; ++c) out += "\t.";
                    out += '\n';
                    continue;
                }
                put_primer(out, r.left, false);
                put_primer(out, r.right, true);
                out += '\t';
                put_number(out, r.product);
                if (a.products < 0) {
                    out += "\t.";
                } else {
                    out += '\t';
                    put_number(out, a.products);
                }
                if (a.products != 1) {
                    for (int c = 0; c < 10; ++c) out += "\t.";
                    out += '\n';
                    continue;
                }
                out += '\t';
                out.append(names + name_offsets[a.record], (size_t)(name_offsets[a.record + 1] - name_offsets[a.record]));
                out += '\t';
                put_number(out, a.start);
                out += '\t';
                put_number(out, a.end);
                out += '\t';
                out += a.forward_of == 0 ? (a.reverse_of == 1 ? '+' : 'l') : (a.reverse_of == 0 ? '-' : 'r');
                out += '\t';
                put_number(out, (int64_t)a.end - a.start);
                out += '\t';
                put_number(out, (int64_t)a.end - a.start - r.product);
                if (a.tract_start < 0) {
                    out += "\t.\t.\t.\t.";
                } else {
                    const int64_t bases = (int64_t)a.tract_end - a.tract_start;
                    for (const int64_t v : {(int64_t)a.tract_start, (int64_t)a.tract_end, bases, bases / (int64_t)row.motif.size()}) {
                        out += '\t';
                        put_number(out, v);
                    }
                }
                out += '\n';
            }
            return PieceRefusal{};
        },
        [](const PieceRefusal &bad) {
            if (bad.why == BAD_LENGTH) return fail(RIBBIT_E_ARG, "row %zu: a primer of %d bases, not 1 .. %d", bad.a, (int)(int32_t)(uint32_t)bad.b, RIBBIT_PRIMER_MAX_LENGTH);
            if (bad.why == NOT_A_ROW) return fail(RIBBIT_E_ARG, "line %zu of the BED text is not a row", bad.a);
            return fail(RIBBIT_E_ARG, "row %zu: record %d is none of the names", bad.a, (int)(int32_t)(uint32_t)bad.b);
        });
}

}  // namespace

extern "C" {

int ribbit_hip_record_pair_amplicons(RibbitHandle *h, const RibbitRowPrimerPair *pairs, size_t n, const char *motifs, const int32_t *offsets, int32_t record,
                                     const RibbitProductParams *params, const RibbitRowAmplicon **rows) {
    return guarded("the pairs' amplicons", [&]() -> int { return record_amplicons_impl(h, pairs, n, motifs, offsets, record, params, rows); });
}

int ribbit_host_record_pair_amplicons(const char *sequence, int64_t length, const RibbitRowPrimerPair *pairs, size_t n, const char *motifs, const int32_t *offsets,
                                      int32_t record, const RibbitProductParams *params, RibbitRowAmplicon **rows) {
    return guarded("the pairs' amplicons", [&]() -> int { return host_record_amplicons_impl(sequence, length, pairs, n, motifs, offsets, record, params, rows); });
}

int ribbit_pair_amplicons_merge(RibbitRowAmplicon *into, const RibbitRowAmplicon *from, size_t n) {
    return guarded("the sum of the pairs' amplicons", [&]() -> int { return amplicons_merge_impl(into, from, n); });
}

void ribbit_pair_amplicons_free(void *from_the_host_twin) { std::free(from_the_host_twin); }

int ribbit_bed_marker_text(const char *bed_text, size_t bed_len, const RibbitRowPrimerPair *pairs, const RibbitRowAmplicon *amplicons, const char *names,
                           const int32_t *name_offsets, size_t n_records, size_t n, char **text, size_t *len) {
    return guarded("the rows' markers as text", [&]() -> int { return bed_marker_text_impl(bed_text, bed_len, pairs, amplicons, names, name_offsets, n_records, n, text, len); });
}

}  // extern "C"
