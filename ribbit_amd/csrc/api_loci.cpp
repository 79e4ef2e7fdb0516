// api_loci.cpp -- merged, sorted loci and the per-window density of a record (loci.hip); see api_internal.h for the map of the
// files behind include/ribbit_hip.h.  The GPU forms read the coverage bitmap the mask builds (build_coverage, api_mask.cpp) and run
// on the handle's stream; the host twins sort the clipped rows and sweep them, without a per-base array, so that they state the
// contract a second time instead of repeating the kernels; the loci's text needs no GPU either.
#include "bed_text.h"

namespace {

constexpr size_t MAX_ROWS = (size_t)INT32_MAX;      // (best_row is an int32)

int check_rows(const int32_t *intervals, size_t n) {
    if (!intervals && n > 0) return fail(RIBBIT_E_ARG, "null argument");
    if (n > MAX_ROWS) return fail(RIBBIT_E_ARG, "%zu intervals", n);
    return RIBBIT_OK;
}

int check_length(int64_t length) {
    if (length < 0 || length > (int64_t)INT32_MAX) return fail(RIBBIT_E_ARG, "a record of %lld bases", (long long)length);
    return RIBBIT_OK;
}

int64_t window_count(int64_t length, int64_t window) { return (length + window - 1) / window; }

int record_loci_impl(RibbitHandle *h, const int32_t *intervals, size_t n, int32_t gap, const RibbitLocus **loci, size_t *n_loci) {
    if (!h) return fail(RIBBIT_E_ARG, "null handle");
    if (!loci || !n_loci) return fail(RIBBIT_E_ARG, "null argument");
    if (gap < 0) return fail(RIBBIT_E_ARG, "gap %d is negative", (int)gap);
    int rc;
    if ((rc = check_rows(intervals, n))) return rc;
    if (!h->loaded) return fail(RIBBIT_E_STATE, "no record loaded");
    static const RibbitLocus kNone{};
    *loci = &kNone;
    *n_loci = 0;
    const int64_t length = h->length;
    if (length == 0 || n == 0) return RIBBIT_OK;
    if ((rc = bind_device(h))) return rc;
    if ((rc = build_coverage(h, intervals, n))) return rc;
    const int64_t lanes = rb::loci_lanes(length);
    if ((rc = h->rows.d_loci_off.ensure((size_t)lanes + 1))) return rc;
    if ((rc = h->rows.d_work.ensure(rb::loci_scan_scratch_bytes(lanes), true))) return rc;
    if ((rc = h->rows.h_loci_count.ensure(2))) return rc;
    HIP_TRY(rb::launch_run_ranks(h->rows.d_mask_bits.p, length, h->rows.d_loci_off.p, h->rows.d_work.p, h->rows.d_work.cap, h->stream));
    HIP_TRY(hipMemcpyAsync(h->rows.h_loci_count.p, h->rows.d_loci_off.p + lanes, sizeof(uint64_t), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    const uint64_t ranks = h->rows.h_loci_count.p[0];
    const size_t runs = (size_t)(ranks >> 32);
    if (runs != (size_t)(uint32_t)ranks || runs > n) return fail(RIBBIT_E_INTERNAL, "%zu run starts, %zu run ends, %zu rows", runs, (size_t)(uint32_t)ranks, n);
    if (runs == 0) return RIBBIT_OK;      // every row is empty
    // d_loci_i32: run starts | run ends | locus starts | covered prefixes; d_loci_u64: the join's prefixes | the rows' keys | the count
    if ((rc = h->rows.d_loci_i32.ensure(4 * runs, true))) return rc;
    if ((rc = h->rows.d_loci_u64.ensure(2 * runs + 1, true))) return rc;
    if ((rc = h->rows.d_loci.ensure(runs, true))) return rc;
    if ((rc = h->rows.d_work.ensure(rb::loci_scan_scratch_bytes((int64_t)runs), true))) return rc;
    int32_t *run_start = h->rows.d_loci_i32.p, *run_end = run_start + runs, *locus_start = run_end + runs, *post = locus_start + runs;
    uint64_t *join = h->rows.d_loci_u64.p, *key = join + runs, *count = key + runs;
    rb::launch_run_bounds(h->rows.d_mask_bits.p, length, h->rows.d_loci_off.p, run_start, run_end, h->stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemsetAsync(key, 0, (runs + 1) * sizeof(uint64_t), h->stream));
    HIP_TRY(hipMemsetAsync(h->rows.d_loci.p, 0, runs * sizeof(RibbitLocus), h->stream));
    HIP_TRY(rb::launch_loci(run_start, run_end, (int64_t)runs, gap, h->rows.d_mask_iv.p, (int64_t)n, length, join, locus_start, post,
                            reinterpret_cast<unsigned long long *>(key), h->rows.d_loci.p, reinterpret_cast<uint32_t *>(count), h->rows.d_work.p,
                            h->rows.d_work.cap, h->stream));
    HIP_TRY(hipMemcpyAsync(h->rows.h_loci_count.p + 1, count, sizeof(uint64_t), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    const size_t found = (size_t)(uint32_t)h->rows.h_loci_count.p[1];
    if (found < 1 || found > runs) return fail(RIBBIT_E_INTERNAL, "%zu loci of %zu runs", found, runs);
    if ((rc = h->rows.h_loci.ensure(found, true))) return rc;
    HIP_TRY(hipMemcpyAsync(h->rows.h_loci.p, h->rows.d_loci.p, found * sizeof(RibbitLocus), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    *loci = h->rows.h_loci.p;
    *n_loci = found;
    return RIBBIT_OK;
}

int record_density_impl(RibbitHandle *h, const int32_t *intervals, size_t n, int32_t window, const int32_t **covered, size_t *n_windows) {
    if (!h) return fail(RIBBIT_E_ARG, "null handle");
    if (!covered || !n_windows) return fail(RIBBIT_E_ARG, "null argument");
    if (window < 1) return fail(RIBBIT_E_ARG, "window %d is below 1", (int)window);
    int rc;
    if ((rc = check_rows(intervals, n))) return rc;
    if (!h->loaded) return fail(RIBBIT_E_STATE, "no record loaded");
    static const int32_t kNone[1] = {0};
    *covered = kNone;
    *n_windows = 0;
    const int64_t length = h->length;
    if (length == 0) return RIBBIT_OK;
    if ((rc = bind_device(h))) return rc;
    const size_t windows = (size_t)window_count(length, window);
    if ((rc = h->rows.d_work.ensure(windows * sizeof(int32_t), true))) return rc;
    if ((rc = h->rows.h_density.ensure(windows, true))) return rc;
    if ((rc = build_coverage(h, intervals, n))) return rc;
    rb::launch_density(h->rows.d_mask_bits.p, length, window, (int64_t)windows, reinterpret_cast<int32_t *>(h->rows.d_work.p), h->stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(h->rows.h_density.p, h->rows.d_work.p, windows * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    *covered = h->rows.h_density.p;
    *n_windows = windows;
    return RIBBIT_OK;
}

// ---- host twins: the clipped, non-empty rows sorted by start (clipped_sorted_rows), then one sweep
int host_record_loci_impl(int64_t length, const int32_t *intervals, size_t n, int32_t gap, RibbitLocus **loci, size_t *n_loci) {
    if (!loci || !n_loci) return fail(RIBBIT_E_ARG, "null argument");
    if (gap < 0) return fail(RIBBIT_E_ARG, "gap %d is negative", (int)gap);
    int rc;
    if ((rc = check_rows(intervals, n)) || (rc = check_length(length))) return rc;
    const std::vector<ClippedRow> rows = clipped_sorted_rows(length, intervals, n);
    std::vector<RibbitLocus> out;
    int64_t run_from = 0, run_to = -1, best = 0;      // the open run, and the length of the open locus's best row
    for (const ClippedRow &r : rows) {
        if (out.empty() || r.s > run_to) {            // a new run (a row that abuts the open run continues it)
            if (!out.empty()) out.back().covered += (int32_t)(run_to - run_from);
            if (out.empty() || r.s - run_to > gap) {
                out.push_back(RibbitLocus{(int32_t)r.s, 0, 0, 0, 0});
                best = 0;
            }
            run_from = r.s;
            run_to = r.e;
        } else {
            run_to = std::max(run_to, r.e);
        }
        RibbitLocus &l = out.back();
        l.end = (int32_t)run_to;
        ++l.rows;
        if (r.e - r.s > best || (r.e - r.s == best && (int64_t)r.index < l.best_row)) {
            best = r.e - r.s;
            l.best_row = (int32_t)r.index;
        }
    }
    if (!out.empty()) out.back().covered += (int32_t)(run_to - run_from);
    if ((rc = hand_out(out.data(), out.size(), false, loci))) return rc;
    *n_loci = out.size();
    return RIBBIT_OK;
}

int host_record_density_impl(int64_t length, const int32_t *intervals, size_t n, int32_t window, int32_t **covered, size_t *n_windows) {
    if (!covered || !n_windows) return fail(RIBBIT_E_ARG, "null argument");
    if (window < 1) return fail(RIBBIT_E_ARG, "window %d is below 1", (int)window);
    int rc;
    if ((rc = check_rows(intervals, n)) || (rc = check_length(length))) return rc;
    const std::vector<ClippedRow> rows = clipped_sorted_rows(length, intervals, n);
    const int64_t windows = window_count(length, window);
    int32_t *mem = static_cast<int32_t *>(std::calloc((size_t)std::max<int64_t>(windows, 1), sizeof(int32_t)));
    if (!mem) return fail(RIBBIT_E_NOMEM, "out of host memory for %lld windows", (long long)windows);
    // every stretch [from, to) that the sweep newly covers goes to the windows it meets
    int64_t covered_to = 0;
    for (const ClippedRow &r : rows) {
        int64_t from = std::max(r.s, covered_to);
        const int64_t to = r.e;
        while (from < to) {
            const int64_t k = from / window, stop = std::min(to, (k + 1) * (int64_t)window);
            mem[k] += (int32_t)(stop - from);
            from = stop;
        }
        covered_to = std::max(covered_to, to);
    }
    *covered = mem;
    *n_windows = (size_t)windows;
    return RIBBIT_OK;
}

// ---- the loci as text
int bed_loci_text_impl(const char *name, const char *bed, size_t bed_len, const RibbitLocus *loci, size_t n_loci, char **text, size_t *len) {
    if (!name || !text || !len || (!bed && bed_len > 0) || (!loci && n_loci > 0)) return fail(RIBBIT_E_ARG, "null argument");
    // the BED text's line starts are found in pieces, and the loci's lines are written in as many pieces
    const size_t parts = n_loci ? bed_text_parts(bed_len) : 1;
    BedLines lines;
    int rc;
    if (n_loci && (rc = lines.find(bed, bed_len, parts))) return rc;
    const size_t n_lines = lines.count(), name_len = std::strlen(name);
    const size_t out_parts = std::max<size_t>(1, std::min<size_t>(parts, n_loci >> 12));
    return write_pieces(out_parts, "loci", text, len, [&](size_t k, std::string &out) {
        for (size_t i = n_loci * k / out_parts; i < n_loci * (k + 1) / out_parts; ++i) {
            const RibbitLocus &l = loci[i];
            if (l.best_row < 0 || (size_t)l.best_row >= n_lines) return PieceRefusal{1, i};
            const BedField line = lines[(size_t)l.best_row];
            const BedRow row = bed_row(line.from, line.to);
            if (!row.ok) return PieceRefusal{1, i};
            out.append(name, name_len);
            for (const int32_t v : {l.start, l.end, l.rows, l.covered}) {
                out += '\t';
                put_number(out, v);
            }
            put_field(out, BedField{row.tail, line.to});      // the row's last ten columns, with the tab before them
            out += '\n';
        }
        return PieceRefusal{};
    }, [&](const PieceRefusal &b) {
        return fail(RIBBIT_E_ARG, "locus %zu: its best row %d is not a row of 11 tab-separated columns of the BED text (%zu lines)", b.a, (int)loci[b.a].best_row, n_lines);
    });
}

}  // namespace

extern "C" {

int ribbit_hip_record_loci(RibbitHandle *h, const int32_t *intervals, size_t n, int32_t gap, const RibbitLocus **loci, size_t *n_loci) {
    return guarded("the loci", [&]() -> int { return record_loci_impl(h, intervals, n, gap, loci, n_loci); });
}

int ribbit_hip_record_density(RibbitHandle *h, const int32_t *intervals, size_t n, int32_t window, const int32_t **covered, size_t *n_windows) {
    return guarded("the density", [&]() -> int { return record_density_impl(h, intervals, n, window, covered, n_windows); });
}

int ribbit_host_record_loci(int64_t length, const int32_t *intervals, size_t n, int32_t gap, RibbitLocus **loci, size_t *n_loci) {
    return guarded("the loci", [&]() -> int { return host_record_loci_impl(length, intervals, n, gap, loci, n_loci); });
}

int ribbit_host_record_density(int64_t length, const int32_t *intervals, size_t n, int32_t window, int32_t **covered, size_t *n_windows) {
    return guarded("the density", [&]() -> int { return host_record_density_impl(length, intervals, n, window, covered, n_windows); });
}

int ribbit_bed_loci_text(const char *name, const char *bed_text, size_t bed_len, const RibbitLocus *loci, size_t n_loci, char **text, size_t *len) {
    return guarded("the loci's text", [&]() -> int { return bed_loci_text_impl(name, bed_text, bed_len, loci, n_loci, text, len); });
}

void ribbit_loci_free(RibbitLocus *loci) { std::free(loci); }

}  // extern "C"
