// api_composition.cpp -- the base counts of every row, of its flanks and of every window of a record (composition.hip); see
// api_internal.h for the map of the files behind include/ribbit_hip.h.  The GPU forms read the bit planes the load packed, not
// the ASCII, and the coverage bitmap the mask builds of the rows (build_coverage, api_mask.cpp), and run on the handle's stream;
// the prefix counts of the planes belong to the record and are kept until the next load.  The host twins count the bytes of the
// sequence with a table, from a sampled prefix, and the coverage by the rows' sorted runs, so that they state the contract a second time
// instead of repeating the kernels; the two texts need no GPU.
#include "bed_text.h"

namespace {

constexpr size_t MAX_ROWS = (size_t)INT32_MAX;
static_assert(sizeof(RibbitRowComposition) == 52 && sizeof(RibbitBaseCounts) == 20, "13 and 5 ints");
std::atomic<int64_t> g_prefix_builds{0};

int check_length(int64_t length) {
    if (length < 0 || length > (int64_t)INT32_MAX) return fail(RIBBIT_E_ARG, "a record of %lld bases", (long long)length);
    return RIBBIT_OK;
}

int check_rows(const int32_t *intervals, size_t n, int32_t flank, const void *out) {
    if ((!intervals && n > 0) || !out) return fail(RIBBIT_E_ARG, "null argument");
    if (n > MAX_ROWS) return fail(RIBBIT_E_ARG, "%zu intervals", n);
    if (flank < 0) return fail(RIBBIT_E_ARG, "flank %d is negative", (int)flank);
    return RIBBIT_OK;
}

int check_window(int32_t window, const void *windows, const size_t *n_windows) {
    if (!windows || !n_windows) return fail(RIBBIT_E_ARG, "null argument");
    if (window < 1) return fail(RIBBIT_E_ARG, "window %d is below 1", (int)window);
    return RIBBIT_OK;
}

int64_t window_count(int64_t length, int64_t window) { return (length + window - 1) / window; }

// the prefix counts of the loaded record (length > 0) in rows.d_comp_sums behind the blocks' counts, enqueued on the handle's
// stream unless they are there already; the caller has sized rows.d_work by `at`, whose scratch region the scan takes.  They count as there
// (prefix_landed) only once the caller's synchronise has come back clean: a call that fails on its way leaves them to be built again.
int ensure_base_prefix(RibbitHandle *h, const rb::CompositionLayout &at) {
    if (h->rec.base_prefix_valid) return RIBBIT_OK;
    RibbitHandle::RowBufs &buf = h->rows;
    const size_t blocks = (size_t)rb::loci_lanes(h->length);
    int rc;
    if ((rc = buf.d_comp_sums.ensure(2 * blocks))) return rc;
    HIP_TRY(rb::launch_composition_prefix(h->planes(), buf.d_comp_sums.p, buf.d_work.p, buf.d_work.cap, at, h->stream));
    ++g_prefix_builds;
    return RIBBIT_OK;
}

void prefix_landed(RibbitHandle *h) { h->rec.base_prefix_valid = true; }

int record_composition_impl(RibbitHandle *h, const int32_t *intervals, size_t n, int32_t flank, const RibbitRowComposition **rows) {
    if (!h) return fail(RIBBIT_E_ARG, "null handle");
    int rc;
    if ((rc = check_rows(intervals, n, flank, rows))) return rc;
    if (!h->loaded) return fail(RIBBIT_E_STATE, "no record loaded");
    RibbitHandle::RowBufs &buf = h->rows;
    if ((rc = buf.h_comp_rows.ensure(std::max<size_t>(n, 1), true))) return rc;
    *rows = buf.h_comp_rows.p;
    if (n == 0) return RIBBIT_OK;
    const int64_t length = h->length;
    if (length == 0) {      // (every row and every flank is empty)
        std::memset(buf.h_comp_rows.p, 0, n * sizeof(RibbitRowComposition));
        return RIBBIT_OK;
    }
    if ((rc = bind_device(h))) return rc;
    const rb::CompositionLayout at = rb::composition_rows_layout((int64_t)n, length);
    if ((rc = buf.d_work.ensure(at.bytes, true))) return rc;
    if ((rc = ensure_base_prefix(h, at))) return rc;
    if ((rc = build_coverage(h, intervals, n))) return rc;
    HIP_TRY(rb::launch_composition_rows(h->planes(), buf.d_comp_sums.p, buf.d_mask_bits.p, buf.d_mask_iv.p, (int64_t)n, flank, buf.d_work.p, buf.d_work.cap, at,
                                        h->stream));
    HIP_TRY(hipMemcpyAsync(buf.h_comp_rows.p, buf.d_work.p + at.out, n * sizeof(RibbitRowComposition), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    prefix_landed(h);
    for (size_t i = 0; i < n; ++i) {
        const RibbitRowComposition &r = buf.h_comp_rows.p[i];
        if ((r.a | r.c | r.g | r.t | r.other | r.left | r.right) < 0 || (int64_t)r.a + r.c + r.g + r.t + r.other > length || (int64_t)r.left_gc + r.left_other > r.left ||
            (int64_t)r.right_gc + r.right_other > r.right || r.left_covered > r.left || r.right_covered > r.right)
            return fail(RIBBIT_E_INTERNAL, "row %zu: the counts the GPU found contradict each other", i);
    }
    return RIBBIT_OK;
}

int record_base_windows_impl(RibbitHandle *h, int32_t window, const RibbitBaseCounts **windows, size_t *n_windows) {
    if (!h) return fail(RIBBIT_E_ARG, "null handle");
    int rc;
    if ((rc = check_window(window, windows, n_windows))) return rc;
    if (!h->loaded) return fail(RIBBIT_E_STATE, "no record loaded");
    static const RibbitBaseCounts kNone{};
    *windows = &kNone;
    *n_windows = 0;
    const int64_t length = h->length;
    if (length == 0) return RIBBIT_OK;
    if ((rc = bind_device(h))) return rc;
    RibbitHandle::RowBufs &buf = h->rows;
    const size_t count = (size_t)window_count(length, window);
    const rb::CompositionLayout at = rb::composition_windows_layout((int64_t)count, length);
    if ((rc = buf.d_work.ensure(at.bytes, true))) return rc;
    if ((rc = buf.h_comp_windows.ensure(count, true))) return rc;
    if ((rc = ensure_base_prefix(h, at))) return rc;
    HIP_TRY(rb::launch_composition_windows(h->planes(), buf.d_comp_sums.p, window, (int64_t)count, buf.d_work.p, buf.d_work.cap, at, h->stream));
    HIP_TRY(hipMemcpyAsync(buf.h_comp_windows.p, buf.d_work.p + at.out, count * sizeof(RibbitBaseCounts), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    prefix_landed(h);
    *windows = buf.h_comp_windows.p;
    *n_windows = count;
    return RIBBIT_OK;
}

// ---- host twins: the bytes themselves
enum : int { KIND_A = 0, KIND_C, KIND_G, KIND_T, KIND_OTHER, KINDS };

struct KindTable {
    uint8_t of[256];
    KindTable() {
        std::memset(of, KIND_OTHER, sizeof of);
        for (const int up : {0, 0x20}) {
            of['A' | up] = KIND_A;
            of['C' | up] = KIND_C;
            of['G' | up] = KIND_G;
            of['T' | up] = KIND_T;
        }
    }
};
const KindTable kKind;

struct Counts {
    int32_t v[KINDS] = {};      // (a record has fewer than 2^31 bases)
    Counts operator-(const Counts &o) const {
        Counts d;
        for (int k = 0; k < KINDS; ++k) d.v[k] = v[k] - o.v[k];
        return d;
    }
};

// The counts of the positions before every multiple of HOST_STEP, and from there byte by byte: a flank of 2^31 bases on every
// row of a chromosome costs no more than a flank of none.
constexpr int64_t HOST_STEP = 256;
struct SequenceCounts {
    const unsigned char *seq;
    std::vector<Counts> at;      // at[j]: the counts of [0, j HOST_STEP)
    SequenceCounts(const char *sequence, int64_t length) : seq(reinterpret_cast<const unsigned char *>(sequence)), at((size_t)(length / HOST_STEP) + 1) {
        Counts run;
        for (int64_t p = 0; p < length; ++p) {
            ++run.v[kKind.of[seq[p]]];
            if ((p + 1) % HOST_STEP == 0) at[(size_t)((p + 1) / HOST_STEP)] = run;
        }
    }
    Counts before(int64_t p) const {
        Counts c = at[(size_t)(p / HOST_STEP)];
        for (int64_t q = p - p % HOST_STEP; q < p; ++q) ++c.v[kKind.of[seq[q]]];
        return c;
    }
};

int host_record_composition_impl(const char *sequence, int64_t length, const int32_t *intervals, size_t n, int32_t flank, RibbitRowComposition **rows) {
    int rc;
    if ((rc = check_rows(intervals, n, flank, rows)) || (rc = check_length(length))) return rc;
    if (!sequence && length > 0) return fail(RIBBIT_E_ARG, "bad sequence");
    const SequenceCounts counts(sequence, length);
    const CoveredRuns runs(clipped_sorted_rows(length, intervals, n));
    Handed<RibbitRowComposition> out;
    if ((rc = hand_out<RibbitRowComposition>(nullptr, n, false, out))) return rc;
    for (size_t i = 0; i < n; ++i) {
        const int64_t s = std::min(std::max<int64_t>(intervals[2 * i], 0), length), e = std::min(std::max<int64_t>(intervals[2 * i + 1], s), length);
        const int64_t lo = std::max<int64_t>(s - flank, 0), hi = std::min<int64_t>(e + flank, length);
        const Counts at_lo = counts.before(lo), at_s = counts.before(s), at_e = counts.before(e), at_hi = counts.before(hi);
        const Counts row = at_e - at_s, left = at_s - at_lo, right = at_hi - at_e;
        RibbitRowComposition &r = out[i];
        r.a = row.v[KIND_A];
        r.c = row.v[KIND_C];
        r.g = row.v[KIND_G];
        r.t = row.v[KIND_T];
        r.other = row.v[KIND_OTHER];
        r.left = (int32_t)(s - lo);
        r.left_gc = left.v[KIND_C] + left.v[KIND_G];
        r.left_other = left.v[KIND_OTHER];
        r.left_covered = (int32_t)(runs.covered_before(s) - runs.covered_before(lo));
        r.right = (int32_t)(hi - e);
        r.right_gc = right.v[KIND_C] + right.v[KIND_G];
        r.right_other = right.v[KIND_OTHER];
        r.right_covered = (int32_t)(runs.covered_before(hi) - runs.covered_before(e));
    }
    *rows = out.release();
    return RIBBIT_OK;
}

int host_record_base_windows_impl(const char *sequence, int64_t length, int32_t window, RibbitBaseCounts **windows, size_t *n_windows) {
    int rc;
    if ((rc = check_window(window, windows, n_windows)) || (rc = check_length(length))) return rc;
    if (!sequence && length > 0) return fail(RIBBIT_E_ARG, "bad sequence");
    const size_t count = (size_t)window_count(length, window);
    Handed<RibbitBaseCounts> out;
    if ((rc = hand_out<RibbitBaseCounts>(nullptr, count, false, out))) return rc;
    const unsigned char *seq = reinterpret_cast<const unsigned char *>(sequence);
    for (size_t k = 0; k < count; ++k) {
        int32_t c[KINDS] = {};
        const int64_t from = (int64_t)k * window, to = std::min<int64_t>(from + window, length);
        for (int64_t p = from; p < to; ++p) ++c[kKind.of[seq[p]]];
        out[k] = RibbitBaseCounts{c[KIND_A], c[KIND_C], c[KIND_G], c[KIND_T], c[KIND_OTHER]};
    }
    *windows = out.release();
    *n_windows = count;
    return RIBBIT_OK;
}

// ---- the two texts
int bed_composition_text_impl(const char *bed, size_t bed_len, const RibbitRowComposition *rows, size_t n, char **text, size_t *len) {
    if (!text || !len || (!bed && bed_len > 0) || (!rows && n > 0)) return fail(RIBBIT_E_ARG, "null argument");
    const size_t parts = bed_text_parts(bed_len);
    BedLines lines;
    int rc;
    if ((rc = lines.find(bed, bed_len, parts))) return rc;
    if (lines.count() != n) return fail(RIBBIT_E_ARG, "the BED text has %zu lines, not the %zu of the rows", lines.count(), n);
    // piece k writes lines [n k / parts, n (k + 1) / parts) where they belong: every line grows by 13 tabs and 13 numbers
    return write_pieces(parts, "the rows' composition", text, len, [&](size_t k, std::string &out) {
        const size_t from = n * k / parts, to = n * (k + 1) / parts;
        out.reserve(lines.start[to] - lines.start[from] + 64 * (to - from));
        for (size_t i = from; i < to; ++i) {
            const RibbitRowComposition &r = rows[i];
            put_field(out, lines[i]);
            for (const int32_t v : {r.a, r.c, r.g, r.t, r.other, r.left, r.left_gc, r.left_other, r.left_covered, r.right, r.right_gc, r.right_other, r.right_covered}) {
                out += '\t';
                put_number(out, v);
            }
            out += '\n';
        }
    });
}

int base_windows_text_impl(const char *name, int64_t length, int32_t window, const RibbitBaseCounts *windows, size_t n_windows, char **text, size_t *len) {
    if (!name || !text || !len || (!windows && n_windows > 0)) return fail(RIBBIT_E_ARG, "null argument");
    if (window < 1) return fail(RIBBIT_E_ARG, "window %d is below 1", (int)window);
    int rc;
    if ((rc = check_length(length))) return rc;
    if (n_windows != (size_t)window_count(length, window))
        return fail(RIBBIT_E_ARG, "%zu windows, not the %lld of a record of %lld bases in windows of %d", n_windows, (long long)window_count(length, window),
                    (long long)length, (int)window);
    const size_t name_len = std::strlen(name), n = n_windows;
    const size_t parts = bed_text_parts(n * 48);
    return write_pieces(parts, "the windows' base counts", text, len, [&](size_t k, std::string &out) {
        const size_t from = n * k / parts, to = n * (k + 1) / parts;
        out.reserve((name_len + 64) * (to - from));
        for (size_t j = from; j < to; ++j) {
            const RibbitBaseCounts &w = windows[j];
            const int64_t start = (int64_t)j * window;
            out.append(name, name_len);
            for (const int64_t v : {start, std::min<int64_t>(start + window, length), (int64_t)w.a, (int64_t)w.c, (int64_t)w.g, (int64_t)w.t, (int64_t)w.other}) {
                out += '\t';
                put_number(out, v);
            }
            out += '\n';
        }
    });
}

}  // namespace

extern "C" {

int ribbit_hip_record_composition(RibbitHandle *h, const int32_t *intervals, size_t n, int32_t flank, const RibbitRowComposition **rows) {
    return guarded("the composition", [&]() -> int { return record_composition_impl(h, intervals, n, flank, rows); });
}

int ribbit_hip_record_base_windows(RibbitHandle *h, int32_t window, const RibbitBaseCounts **windows, size_t *n_windows) {
    return guarded("the windows' base counts", [&]() -> int { return record_base_windows_impl(h, window, windows, n_windows); });
}

int ribbit_host_record_composition(const char *sequence, int64_t length, const int32_t *intervals, size_t n, int32_t flank, RibbitRowComposition **rows) {
    return guarded("the composition", [&]() -> int { return host_record_composition_impl(sequence, length, intervals, n, flank, rows); });
}

int ribbit_host_record_base_windows(const char *sequence, int64_t length, int32_t window, RibbitBaseCounts **windows, size_t *n_windows) {
    return guarded("the windows' base counts", [&]() -> int { return host_record_base_windows_impl(sequence, length, window, windows, n_windows); });
}

void ribbit_composition_free(void *rows_or_windows) { std::free(rows_or_windows); }

int64_t ribbit_debug_composition_prefix_builds(void) { return g_prefix_builds.load(); }

int ribbit_bed_composition_text(const char *bed_text, size_t bed_len, const RibbitRowComposition *rows, size_t n, char **text, size_t *len) {
    return guarded("the rows' composition as text", [&]() -> int { return bed_composition_text_impl(bed_text, bed_len, rows, n, text, len); });
}

int ribbit_base_windows_text(const char *name, int64_t length, int32_t window, const RibbitBaseCounts *windows, size_t n_windows, char **text, size_t *len) {
    return guarded("the windows' base counts as text", [&]() -> int { return base_windows_text_impl(name, length, window, windows, n_windows, text, len); });
}

}  // extern "C"
