// api_primers.cpp -- a forward and a reverse primer in the flanks of every target of a record (primers.hip); see api_internal.h
// for the map of the files behind include/ribbit_hip.h.  The GPU form reads the bit planes the load packed and the coverage bitmap
// the mask builds of the record's rows (build_coverage, api_mask.cpp), stages the targets through stage_down and runs on the handle's
// stream; it keeps nothing between calls and leaves what the other row outputs keep (the bitmap's rows, the base prefix) as it
// finds it.  The host twin works from the bytes of the sequence and computes every candidate on its own, base by base, without a
// prefix, so that it states the contract a second time instead of repeating the kernel; the text needs no GPU.
#include "primers_host.h"

#include <tuple>

namespace {

void no_primers(RibbitRowPrimers *rows, size_t n) {
    for (size_t i = 0; i < n; ++i) rows[i] = RibbitRowPrimers{NO_PRIMER, NO_PRIMER, 0, 0};
}

int record_primers_impl(RibbitHandle *h, const int32_t *intervals, size_t n, const int32_t *targets, size_t n_targets, const RibbitPrimerParams *params,
                        const RibbitRowPrimers **rows) {
    if (!h) return fail(RIBBIT_E_ARG, "null handle");
    int rc;
    if ((rc = check_primer_args(intervals, n, targets, n_targets, params, rows))) return rc;
    if (!h->loaded) return fail(RIBBIT_E_STATE, "no record loaded");
    RibbitHandle::RowBufs &buf = h->rows;
    if ((rc = buf.h_primers.ensure(std::max<size_t>(n_targets, 1), true))) return rc;
    *rows = buf.h_primers.p;
    if (n_targets == 0) return RIBBIT_OK;
    const int64_t length = h->length;
    if (length == 0) {      // (every flank is empty)
        no_primers(buf.h_primers.p, n_targets);
        return RIBBIT_OK;
    }
    if ((rc = bind_device(h))) return rc;
    const rb::PrimerLayout at = rb::primers_layout((int64_t)n_targets);
    if ((rc = buf.d_work.ensure(at.bytes, true))) return rc;
    const StageSegment down{targets, 2 * n_targets * sizeof(int32_t)};
    const uint8_t *d_targets = nullptr;
    if ((rc = stage_down(h, &down, 1, &d_targets))) return rc;
    if ((rc = build_coverage(h, intervals, n))) return rc;
    HIP_TRY(rb::launch_primers(h->planes(), buf.d_mask_bits.p, reinterpret_cast<const int32_t *>(d_targets), (int64_t)n_targets, *params, buf.d_work.p,
                               buf.d_work.cap, at, h->stream));
    HIP_TRY(hipMemcpyAsync(buf.h_primers.p, buf.d_work.p + at.out, n_targets * sizeof(RibbitRowPrimers), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    for (size_t i = 0; i < n_targets; ++i) {
        const RibbitRowPrimers &r = buf.h_primers.p[i];
        const Flanks f = flanks_of(targets, i, params->flank, length);
        const auto inside = [&](const RibbitPrimer &p, int64_t from, int64_t to) {
            return p.start == -1 ? p.length == 0 : p.length >= params->min_length && p.length <= params->max_length && p.start >= from && (int64_t)p.start + p.length <= to;
        };
        if (!inside(r.left, f.lo, f.s) || !inside(r.right, f.e, f.hi) || r.left_candidates < (r.left.start >= 0) || r.right_candidates < (r.right.start >= 0))
            return fail(RIBBIT_E_INTERNAL, "target %zu: a primer the GPU found lies outside its flank", i);
    }
    return RIBBIT_OK;
}

// ---- host twin: the bytes themselves, every candidate from scratch
// the best admissible candidate of the window [from, to) and their number
int32_t side(const unsigned char *seq, const std::vector<uint8_t> &covered, int64_t from, int64_t to, bool right, const RibbitPrimerParams &prm, RibbitPrimer &best) {
    best = NO_PRIMER;
    int32_t found = 0;
    int64_t best_distance = 0;
    for (int64_t p = from; p < to; ++p)
        for (int32_t k = prm.min_length; k <= prm.max_length && p + k <= to; ++k) {
            const Candidate c = candidate(seq, covered, p, k, right ? p : p + k - 1, prm);
            if (!c.ok) continue;
            ++found;
            const int32_t penalty = std::abs(c.tm - prm.tm_opt) + 10 * std::abs(k - prm.opt_length);
            const int64_t distance = right ? p - from : to - (p + k);
            if (best.start >= 0 && std::make_tuple(best.penalty, best_distance, best.length) <= std::make_tuple(penalty, distance, k)) continue;
            uint64_t bases = 0;
            for (int32_t j = 0; j < k; ++j) bases |= (uint64_t)code_of(seq[p + j]) << (2 * j);
            best = RibbitPrimer{(int32_t)p, k, c.tm, penalty, (int32_t)(uint32_t)bases, (int32_t)(uint32_t)(bases >> 32)};
            best_distance = distance;
        }
    return found;
}

int host_record_primers_impl(const char *sequence, int64_t length, const int32_t *intervals, size_t n, const int32_t *targets, size_t n_targets,
                             const RibbitPrimerParams *params, RibbitRowPrimers **rows) {
    int rc;
    if ((rc = check_primer_args(intervals, n, targets, n_targets, params, rows))) return rc;
    if ((rc = check_sequence(sequence, length))) return rc;
    const unsigned char *seq = reinterpret_cast<const unsigned char *>(sequence);
    std::vector<uint8_t> covered((size_t)length, 0);
    const CoveredRuns runs(clipped_sorted_rows(length, intervals, n));
    for (size_t k = 0; k < runs.start.size(); ++k) std::fill(covered.begin() + runs.start[k], covered.begin() + runs.end[k], 1);
    Handed<RibbitRowPrimers> out;
    if ((rc = hand_out<RibbitRowPrimers>(nullptr, n_targets, false, out))) return rc;
    const RibbitPrimerParams prm = *params;
    const unsigned threads = (unsigned)std::max<size_t>(1, std::min<size_t>(rb::host_thread_count(0), n_targets / 16));
    rb::over_pieces(n_targets, threads, [&](size_t lo, size_t hi, unsigned) {
        for (size_t i = lo; i < hi; ++i) {
            const Flanks f = flanks_of(targets, i, prm.flank, length);
            RibbitRowPrimers &r = out[i];
            r.left_candidates = side(seq, covered, f.lo, f.s, false, prm, r.left);
            r.right_candidates = side(seq, covered, f.e, f.hi, true, prm, r.right);
        }
    });
    *rows = out.release();
    return RIBBIT_OK;
}

// ---- the text
enum : int { BAD_LENGTH = 1 };

int bed_primers_text_impl(const char *bed, size_t bed_len, const RibbitRowPrimers *rows, size_t n, char **text, size_t *len) {
    if (!text || !len || (!bed && bed_len > 0) || (!rows && n > 0)) return fail(RIBBIT_E_ARG, "null argument");
    const size_t parts = bed_text_parts(bed_len);
    BedLines lines;
    int rc;
    if ((rc = lines.find(bed, bed_len, parts))) return rc;
    if (lines.count() != n) return fail(RIBBIT_E_ARG, "the BED text has %zu lines, not the %zu of the rows", lines.count(), n);
    return write_pieces(
        parts, "the rows' primers", text, len,
        [&](size_t k, std::string &out) {
            const size_t from = n * k / parts, to = n * (k + 1) / parts;
            out.reserve(lines.start[to] - lines.start[from] + 128 * (to - from));
            for (size_t i = from; i < to; ++i) {
                const RibbitRowPrimers &r = rows[i];
                for (const RibbitPrimer *p : {&r.left, &r.right})
                    if (p->start >= 0 && (p->length < 1 || p->length > RIBBIT_PRIMER_MAX_LENGTH)) return PieceRefusal{BAD_LENGTH, i, (size_t)(uint32_t)p->length};
                put_field(out, lines[i]);
                put_primer(out, r.left, false);
                put_primer(out, r.right, true);
                out += '\t';
                if (r.left.start >= 0 && r.right.start >= 0) put_number(out, (int64_t)r.right.start + r.right.length - r.left.start); else out += '.';
                out += '\t';
                put_number(out, r.left_candidates);
                out += '\t';
                put_number(out, r.right_candidates);
                out += '\n';
            }
            return PieceRefusal{};
        },
        [](const PieceRefusal &bad) { return fail(RIBBIT_E_ARG, "row %zu: a primer of %d bases, not 1 .. %d", bad.a, (int)(int32_t)(uint32_t)bad.b, RIBBIT_PRIMER_MAX_LENGTH); });
}

}  // namespace

extern "C" {

void ribbit_primer_params_default(RibbitPrimerParams *params) {
    if (params) *params = RibbitPrimerParams{200, 18, 25, 20, 570, 600, 630, 40, 60, 4, 1};
}

int ribbit_hip_record_primers(RibbitHandle *h, const int32_t *intervals, size_t n, const int32_t *targets, size_t n_targets, const RibbitPrimerParams *params,
                              const RibbitRowPrimers **rows) {
    return guarded("the primers", [&]() -> int { return record_primers_impl(h, intervals, n, targets, n_targets, params, rows); });
}

int ribbit_host_record_primers(const char *sequence, int64_t length, const int32_t *intervals, size_t n, const int32_t *targets, size_t n_targets,
                               const RibbitPrimerParams *params, RibbitRowPrimers **rows) {
    return guarded("the primers", [&]() -> int { return host_record_primers_impl(sequence, length, intervals, n, targets, n_targets, params, rows); });
}

void ribbit_primers_free(RibbitRowPrimers *rows) { std::free(rows); }

int ribbit_bed_primers_text(const char *bed_text, size_t bed_len, const RibbitRowPrimers *rows, size_t n, char **text, size_t *len) {
    return guarded("the rows' primers as text", [&]() -> int { return bed_primers_text_impl(bed_text, bed_len, rows, n, text, len); });
}

}  // extern "C"
