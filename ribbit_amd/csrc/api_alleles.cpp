// api_alleles.cpp -- the chosen pairs typed on many assemblies: a sample's row of cells from its summed amplicons, every marker's
// alleles over the sample-major matrix (alleles.hip), both texts; see api_internal.h for the map of the files behind
// include/ribbit_hip.h.  The GPU form reads no record and needs none loaded.  Markers go down in batches of ALLELE_CELL_BUDGET cells
// (or of what ribbit_hip_debug_set_specific_batch asked for, counting markers): the host matrix stays sample-major, so a batch is
// n_samples + 2 segments of stage_down, the markers' stretch of every sample's row on a 16-byte pitch, then their designed products
// and motif lengths; one launch fills the batch's records in the handle's work buffer and one copy brings them back.  After the
// last batch everything the device returned is checked.
// The host twin is plain loops over one marker's column with std::sort.  It shares nothing with the kernel.  The texts need no GPU.
#include "primers_host.h"

#include <string>

namespace {

static_assert(sizeof(RibbitRowAlleles) == 64 && sizeof(RibbitRowAmplicon) == 64, "16 ints each");
constexpr size_t ALLELE_CELL_BUDGET = (size_t)16 << 20;      // cells of one batch: 64 MiB on their way down
constexpr int32_t CELL_SEVERAL = -1, CELL_OVER = -2;

int check_shape(size_t n_samples, size_t n) {
    if (n_samples < 1 || n_samples > RIBBIT_ALLELES_MAX_SAMPLES) return fail(RIBBIT_E_ARG, "%zu samples, not 1 .. %d", n_samples, RIBBIT_ALLELES_MAX_SAMPLES);
    if (n > (size_t)RIBBIT_ALLELES_MAX_MARKERS) return fail(RIBBIT_E_ARG, "%zu markers (at most %d)", n, RIBBIT_ALLELES_MAX_MARKERS);
    return RIBBIT_OK;
}

// the least index of [0, count) that `bad` refuses, or count: walked in pieces on the host thread team
template <typename Bad>
size_t first_refused(size_t count, Bad bad) {
    const unsigned threads = (unsigned)std::max<size_t>(1, std::min<size_t>(rb::host_thread_count(0), count >> 20));
    std::vector<size_t> found(threads, count);
    rb::over_pieces(count, threads, [&](size_t lo, size_t hi, unsigned t) {
        for (size_t k = lo; k < hi; ++k)
            if (bad(k)) { found[t] = k; return; }
    });
    return *std::min_element(found.begin(), found.end());
}

int check_cells(const int32_t *cells, size_t n_samples, size_t n) {
    const size_t at = first_refused(n_samples * n, [&](size_t k) { return cells[k] < CELL_OVER; });
    if (at < n_samples * n) return fail(RIBBIT_E_ARG, "cell %zu (sample %zu, marker %zu) is %d, below -2", at, at / n, at % n, (int)cells[at]);
    return RIBBIT_OK;
}

int check_args(const int32_t *cells, size_t n_samples, size_t n, const int32_t *designed, const int32_t *motif_lengths, const void *rows) {
    if (!rows) return fail(RIBBIT_E_ARG, "null argument");
    if (const int rc = check_shape(n_samples, n)) return rc;
    if ((!cells || !designed || !motif_lengths) && n > 0) return fail(RIBBIT_E_ARG, "null argument");
    const size_t at = first_refused(n, [&](size_t i) { return motif_lengths[i] < 1; });
    if (at < n) return fail(RIBBIT_E_ARG, "marker %zu: a motif length of %d, below 1", at, (int)motif_lengths[at]);
    return check_cells(cells, n_samples, n);
}

int marker_alleles_impl(RibbitHandle *h, const int32_t *cells, size_t n_samples, size_t n, const int32_t *designed, const int32_t *motif_lengths,
                        const RibbitRowAlleles **rows) {
    if (!h) return fail(RIBBIT_E_ARG, "null handle");
    if (rows) *rows = nullptr;      // (the answer's only when the call succeeds)
    int rc;
    if ((rc = check_args(cells, n_samples, n, designed, motif_lengths, rows))) return rc;
    RibbitHandle::RowBufs &buf = h->rows;
    if ((rc = buf.h_alleles.ensure(std::max<size_t>(n, 1) * sizeof(RibbitRowAlleles), true))) return rc;
    RibbitRowAlleles *out = reinterpret_cast<RibbitRowAlleles *>(buf.h_alleles.p);
    if (n == 0) {
        *rows = out;
        return RIBBIT_OK;
    }
    if ((rc = bind_device(h))) return rc;
    const size_t by_budget = std::max<size_t>(rb::ALLELE_RUN, ALLELE_CELL_BUDGET / n_samples / rb::ALLELE_RUN * rb::ALLELE_RUN);
    const size_t batch = std::min(buf.specific_batch ? buf.specific_batch : by_budget, n);
    const rb::AllelesLayout at = rb::alleles_layout((int64_t)batch);
    if ((rc = buf.d_work.ensure(at.bytes, true))) return rc;
    const bool profile = rb::profile_on();
    double copy_ms = 0.0, kernel_ms = 0.0;
    OwnedEvent ev[3];
    if (profile)
        for (OwnedEvent &e : ev) HIP_TRY(e.create());
    std::vector<StageSegment> down(n_samples + 2);
    std::vector<const uint8_t *> d_at(n_samples + 2, nullptr);
    for (size_t from = 0; from < n; from += batch) {
        const size_t m = std::min(batch, n - from);
        for (size_t s = 0; s < n_samples; ++s) down[s] = StageSegment{cells + s * n + from, m * sizeof(int32_t)};
        down[n_samples] = StageSegment{designed + from, m * sizeof(int32_t)};
        down[n_samples + 1] = StageSegment{motif_lengths + from, m * sizeof(int32_t)};
        if (profile) HIP_TRY(hipEventRecord(ev[0], h->stream));
        if ((rc = stage_down(h, down.data(), down.size(), d_at.data()))) return rc;
        if (profile) HIP_TRY(hipEventRecord(ev[1], h->stream));
        HIP_TRY(rb::launch_marker_alleles(reinterpret_cast<const int32_t *>(d_at[0]), (int64_t)(round16(m * sizeof(int32_t)) / sizeof(int32_t)), (int64_t)n_samples, (int64_t)m,
                                          reinterpret_cast<const int32_t *>(d_at[n_samples]), reinterpret_cast<const int32_t *>(d_at[n_samples + 1]), buf.d_work.p,
                                          buf.d_work.cap, at, h->stream));
        if (profile) HIP_TRY(hipEventRecord(ev[2], h->stream));
        HIP_TRY(hipMemcpyAsync(out + from, buf.d_work.p + at.rows, m * sizeof(RibbitRowAlleles), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));
        if (profile) {
            float ms[2] = {0, 0};
            (void)hipEventElapsedTime(&ms[0], ev[0], ev[1]);
            (void)hipEventElapsedTime(&ms[1], ev[1], ev[2]);
            copy_ms += ms[0];
            kernel_ms += ms[1];
        }
    }
    if (profile) std::fprintf(stderr, "[alleles] markers %zu samples %zu batch %zu copy_ms %.3f kernel_ms %.3f\n", n, n_samples, batch, copy_ms, kernel_ms);
    // what the device returned
    const int64_t S = (int64_t)n_samples;
    const RibbitRowAlleles none{};
    for (size_t i = 0; i < n; ++i) {
        const RibbitRowAlleles &r = out[i];
        const int64_t t = r.typed;
        bool good = r.reserved == 0 && t >= 0 && r.absent >= 0 && r.several >= 0 && r.over >= 0;
        if (designed[i] <= 0) {
            good = std::memcmp(&r, &none, sizeof r) == 0;
        } else {
            good = good && t + r.absent + r.several + r.over == S && r.alleles >= (t > 0) && r.alleles <= t && r.same >= 0 && r.same <= t && r.off_step >= 0 && r.off_step <= t &&
                   r.het_num >= 0 && r.het_num <= t * t && r.pic_num >= 0 && r.pic_num <= t * t * t * t;
            good = good && (t == 0 ? r.min_size == 0 && r.max_size == 0 && r.major_size == 0 && r.major_count == 0
                                   : r.min_size > 0 && r.min_size <= r.major_size && r.major_size <= r.max_size && r.major_count >= 1 && r.major_count <= t);
        }
        if (!good) return fail(RIBBIT_E_INTERNAL, "marker %zu: the alleles the GPU counted do not add up", i);
    }
    *rows = out;
    return RIBBIT_OK;
}

// ---- the host twin
RibbitRowAlleles alleles_of(const int32_t *cells, size_t n_samples, size_t n, size_t i, int32_t designed, int32_t motif_length) {
    RibbitRowAlleles r{};
    if (designed <= 0) return r;
    std::vector<int64_t> sizes;
    for (size_t s = 0; s < n_samples; ++s) {
        const int32_t c = cells[s * n + i];
        if (c > 0) {
            sizes.push_back(c);
            r.same += c == designed;
            r.off_step += ((int64_t)c - designed) % motif_length != 0;
        } else if (c == 0) {
            ++r.absent;
        } else if (c == CELL_SEVERAL) {
            ++r.several;
        } else {
            ++r.over;
        }
    }
    std::sort(sizes.begin(), sizes.end());
    const int64_t t = (int64_t)sizes.size();
    r.typed = (int32_t)t;
    int64_t Q = 0, F = 0;
    for (size_t a = 0; a < sizes.size();) {
        size_t b = a;
        while (b < sizes.size() && sizes[b] == sizes[a]) ++b;
        const int64_t c = (int64_t)(b - a);
        Q += c * c;
        F += c * c * c * c;
        ++r.alleles;
        if (c > r.major_count) {      // (ascending sizes: of equal counts the first, the least, stays)
            r.major_count = (int32_t)c;
            r.major_size = (int32_t)sizes[a];
        }
        a = b;
    }
    if (t > 0) {
        r.min_size = (int32_t)sizes.front();
        r.max_size = (int32_t)sizes.back();
    }
    r.het_num = t * t - Q;
    r.pic_num = t * t * t * t - t * t * Q - Q * Q + F;
    return r;
}

int host_marker_alleles_impl(const int32_t *cells, size_t n_samples, size_t n, const int32_t *designed, const int32_t *motif_lengths, RibbitRowAlleles **rows) {
    int rc;
    if ((rc = check_args(cells, n_samples, n, designed, motif_lengths, rows))) return rc;
    Handed<RibbitRowAlleles> out;
    if ((rc = hand_out<RibbitRowAlleles>(nullptr, n, false, out))) return rc;
    const unsigned threads = (unsigned)std::max<size_t>(1, std::min<size_t>(rb::host_thread_count(0), n >> 10));
    rb::over_pieces(n, threads, [&](size_t lo, size_t hi, unsigned) {
        for (size_t i = lo; i < hi; ++i) out[i] = alleles_of(cells, n_samples, n, i, designed[i], motif_lengths[i]);
    });
    *rows = out.release();
    return RIBBIT_OK;
}

int amplicon_sizes_impl(const RibbitRowAmplicon *sum, size_t n, int32_t *cells) {
    if ((!sum || !cells) && n > 0) return fail(RIBBIT_E_ARG, "null argument");
    for (size_t i = 0; i < n; ++i) {
        const RibbitRowAmplicon &a = sum[i];
        if (a.products < -1) return fail(RIBBIT_E_ARG, "pair %zu: products %d is below -1", i, (int)a.products);
        if (a.products == 1 && (int64_t)a.end - a.start <= 0) return fail(RIBBIT_E_ARG, "pair %zu: a product from %d to %d", i, (int)a.start, (int)a.end);
        cells[i] = a.products == 1 ? a.end - a.start : a.products == 0 ? 0 : a.products > 1 ? CELL_SEVERAL : CELL_OVER;
    }
    return RIBBIT_OK;
}

// ---- the texts
enum : int { BAD_LENGTH = 1, NOT_A_ROW = 2, BAD_TYPED = 3, BAD_CELL = 4 };

// num / den to four decimals, rounded half up in integers
void put_ratio(std::string &out, int64_t num, int64_t den) {
    const int64_t v = (num * 10000 + den / 2) / den;      // (num <= den <= 2^40: below 2^54)
    put_number(out, v / 10000);
    out += '.';
    for (int64_t place = 1000; place > 0; place /= 10) out += (char)('0' + v / place % 10);
}

int bed_alleles_text_impl(const char *bed, size_t bed_len, const RibbitRowPrimerPair *pairs, const RibbitRowAlleles *rows, size_t n_samples, size_t n, char **text,
                          size_t *len) {
    if (!text || !len || (!bed && bed_len > 0) || ((!pairs || !rows) && n > 0)) return fail(RIBBIT_E_ARG, "null argument");
    int rc;
    if ((rc = check_shape(n_samples, n))) return rc;
    const size_t parts = bed_text_parts(bed_len);
    BedLines lines;
    if ((rc = lines.find(bed, bed_len, parts))) return rc;
    if (lines.count() != n) return fail(RIBBIT_E_ARG, "the BED text has %zu lines, not the %zu of the rows", lines.count(), n);
    return write_pieces(
        parts, "the rows' alleles", text, len,
        [&](size_t k, std::string &out) {
            const size_t from = n * k / parts, to = n * (k + 1) / parts;
            out.reserve(lines.start[to] - lines.start[from] + 256 * (to - from));
            for (size_t i = from; i < to; ++i) {
                const RibbitRowPrimerPair &p = pairs[i];
                const RibbitRowAlleles &r = rows[i];
                if (const RibbitPrimer *bad = bad_primer(p)) return PieceRefusal{BAD_LENGTH, i, (size_t)(uint32_t)bad->length};
                put_field(out, lines[i]);
                if (p.left.start < 0 || p.right.start < 0) {
                    for (int c = 0; c < 23; ++c) out += "\t.";
                    out += '\n';
                    continue;
                }
                if (r.typed < 0 || (size_t)r.typed > n_samples) return PieceRefusal{BAD_TYPED, i, (size_t)(uint32_t)r.typed};
                put_primer(out, p.left, false);
                put_primer(out, p.right, true);
                out += '\t';
                put_number(out, p.product);
                const bool any = r.typed > 0;
                const int64_t t2 = (int64_t)r.typed * r.typed;
                int column = 0;
                for (const int64_t v : {(int64_t)n_samples, (int64_t)r.typed, (int64_t)r.absent, (int64_t)r.several, (int64_t)r.over, (int64_t)r.alleles, (int64_t)r.min_size,
                                        (int64_t)r.max_size, (int64_t)r.major_size, (int64_t)r.major_count, (int64_t)r.same, (int64_t)r.off_step}) {
                    out += '\t';
                    const bool a_size = column == 6 || column == 7 || column == 8;
                    if (a_size && !any) out += '.'; else put_number(out, v);
                    ++column;
                }
                if (any) {
                    out += '\t';
                    put_ratio(out, r.het_num, t2);
                    out += '\t';
                    put_ratio(out, r.pic_num, t2 * t2);
                } else {
                    out += "\t.\t.";
                }
                out += '\n';
            }
            return PieceRefusal{};
        },
        [&](const PieceRefusal &bad) {
            if (bad.why == BAD_LENGTH) return fail(RIBBIT_E_ARG, "row %zu: a primer of %d bases, not 1 .. %d", bad.a, (int)(int32_t)(uint32_t)bad.b, RIBBIT_PRIMER_MAX_LENGTH);
            return fail(RIBBIT_E_ARG, "row %zu: %d typed cells of %zu samples", bad.a, (int)(int32_t)(uint32_t)bad.b, n_samples);
        });
}

int allele_matrix_text_impl(const char *bed, size_t bed_len, const int32_t *cells, size_t n_samples, size_t n, const int32_t *designed, const char *names,
                            const int32_t *name_offsets, char **text, size_t *len) {
    if (!text || !len || (!bed && bed_len > 0) || ((!cells || !designed) && n > 0) || !names || !name_offsets) return fail(RIBBIT_E_ARG, "null argument");
    int rc;
    if ((rc = check_shape(n_samples, n))) return rc;
    for (size_t s = 0; s < n_samples; ++s)
        if (name_offsets[s] < 0 || name_offsets[s + 1] < name_offsets[s]) return fail(RIBBIT_E_ARG, "sample %zu: the names' offsets do not ascend", s);
    const size_t parts = bed_text_parts(bed_len);
    BedLines lines;
    if ((rc = lines.find(bed, bed_len, parts))) return rc;
    if (lines.count() != n) return fail(RIBBIT_E_ARG, "the BED text has %zu lines, not the %zu of the rows", lines.count(), n);
    return write_pieces(
        parts, "the allele matrix", text, len,
        [&](size_t k, std::string &out) {
            const size_t from = n * k / parts, to = n * (k + 1) / parts;
            if (k == 0) {
                out += "#name\tstart\tend\tmotif\tdesigned";
                for (size_t s = 0; s < n_samples; ++s) {
                    out += '\t';
                    out.append(names + name_offsets[s], (size_t)(name_offsets[s + 1] - name_offsets[s]));
                }
                out += '\n';
            }
            for (size_t i = from; i < to; ++i) {
                const BedField line = lines[i];
                const BedRow row = bed_row(line.from, line.to);
                if (!row.ok) return PieceRefusal{NOT_A_ROW, i, 0};
                put_field(out, BedField{line.from, row.motif.to});      // (name, start, end, motif)
                out += '\t';
                if (designed[i] > 0) put_number(out, designed[i]); else out += '.';
                for (size_t s = 0; s < n_samples; ++s) {
                    const int32_t c = cells[s * n + i];
                    if (c < CELL_OVER) return PieceRefusal{BAD_CELL, s * n + i, 0};
                    out += '\t';
                    if (c > 0) put_number(out, c); else out += c == 0 ? '.' : c == CELL_SEVERAL ? '+' : '*';
                }
                out += '\n';
            }
            return PieceRefusal{};
        },
        [&](const PieceRefusal &bad) {
            if (bad.why == NOT_A_ROW) return fail(RIBBIT_E_ARG, "line %zu of the BED text is not a row", bad.a);
            return fail(RIBBIT_E_ARG, "cell %zu (sample %zu, marker %zu) is %d, below -2", bad.a, bad.a / n, bad.a % n, (int)cells[bad.a]);
        });
}

}  // namespace

extern "C" {

int ribbit_pair_amplicon_sizes(const RibbitRowAmplicon *sum, size_t n, int32_t *cells) {
    return guarded("the pairs' product sizes", [&]() -> int { return amplicon_sizes_impl(sum, n, cells); });
}

int ribbit_hip_marker_alleles(RibbitHandle *h, const int32_t *cells, size_t n_samples, size_t n, const int32_t *designed, const int32_t *motif_lengths,
                              const RibbitRowAlleles **rows) {
    return guarded("the markers' alleles", [&]() -> int { return marker_alleles_impl(h, cells, n_samples, n, designed, motif_lengths, rows); });
}

int ribbit_host_marker_alleles(const int32_t *cells, size_t n_samples, size_t n, const int32_t *designed, const int32_t *motif_lengths, RibbitRowAlleles **rows) {
    return guarded("the markers' alleles", [&]() -> int { return host_marker_alleles_impl(cells, n_samples, n, designed, motif_lengths, rows); });
}

void ribbit_alleles_free(void *from_the_host_twin) { std::free(from_the_host_twin); }

int ribbit_bed_alleles_text(const char *bed_text, size_t bed_len, const RibbitRowPrimerPair *pairs, const RibbitRowAlleles *rows, size_t n_samples, size_t n, char **text,
                            size_t *len) {
    return guarded("the rows' alleles as text", [&]() -> int { return bed_alleles_text_impl(bed_text, bed_len, pairs, rows, n_samples, n, text, len); });
}

int ribbit_allele_matrix_text(const char *bed_text, size_t bed_len, const int32_t *cells, size_t n_samples, size_t n, const int32_t *designed, const char *names,
                              const int32_t *name_offsets, char **text, size_t *len) {
    return guarded("the allele matrix as text", [&]() -> int { return allele_matrix_text_impl(bed_text, bed_len, cells, n_samples, n, designed, names, name_offsets, text, len); });
}

}  // extern "C"
