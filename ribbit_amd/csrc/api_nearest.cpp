// api_nearest.cpp -- for every interval of one set, the interval of a second set it lies in or overlaps and its neighbours to
// either side (nearest.hip); see api_internal.h for the map of the files behind include/ribbit_hip.h.  The GPU form stages the
// queries and the targets through stage_down, runs on the handle's stream, keeps nothing between calls and synchronises once;
// the host twin sorts the clipped targets twice and does the same four searches per query with the standard library, and is
// tested against the plain statement of the contract, not against the device.  The two texts need no GPU.
#include "bed_text.h"

namespace {

constexpr size_t MAX_INTERVALS = (size_t)INT32_MAX;      // (the indices are int32)
static_assert(sizeof(RibbitNearest) == 24, "six ints per query");
constexpr RibbitNearest NOTHING{RIBBIT_NEAREST_APART, -1, -1, -1, -1, -1};

int check_sets(const int32_t *queries, size_t n, const int32_t *targets, size_t n_targets, const void *out) {
    if ((!queries && n > 0) || (!targets && n_targets > 0) || !out) return fail(RIBBIT_E_ARG, "null argument");
    if (n > MAX_INTERVALS) return fail(RIBBIT_E_ARG, "%zu queries", n);
    if (n_targets > MAX_INTERVALS) return fail(RIBBIT_E_ARG, "%zu targets", n_targets);
    return RIBBIT_OK;
}

int record_nearest_impl(RibbitHandle *h, const int32_t *queries, size_t n, const int32_t *targets, size_t n_targets, const RibbitNearest **out) {
    if (!h) return fail(RIBBIT_E_ARG, "null handle");
    int rc;
    if ((rc = check_sets(queries, n, targets, n_targets, out))) return rc;
    if (!h->loaded) return fail(RIBBIT_E_STATE, "no record loaded");
    RibbitHandle::RowBufs &buf = h->rows;
    if ((rc = buf.h_near.ensure(std::max<size_t>(n, 1), true))) return rc;
    *out = buf.h_near.p;
    if (n == 0) return RIBBIT_OK;
    if (h->length == 0) {      // (every query is empty)
        std::fill(buf.h_near.p, buf.h_near.p + n, NOTHING);
        return RIBBIT_OK;
    }
    if ((rc = bind_device(h))) return rc;
    const rb::NearestLayout at = rb::nearest_layout((int64_t)n, (int64_t)n_targets);
    if ((rc = buf.d_work.ensure(at.bytes, true))) return rc;
    // down: the queries | the targets
    const StageSegment down[2] = {{queries, 2 * n * sizeof(int32_t)}, {targets, 2 * n_targets * sizeof(int32_t)}};
    const uint8_t *d_in[2];
    if ((rc = stage_down(h, down, 2, d_in))) return rc;
    HIP_TRY(rb::launch_nearest(reinterpret_cast<const int32_t *>(d_in[0]), (int64_t)n, reinterpret_cast<const int32_t *>(d_in[1]), (int64_t)n_targets, h->length,
                               buf.d_work.p, buf.d_work.cap, at, h->stream));
    HIP_TRY(hipMemcpyAsync(buf.h_near.p, buf.d_work.p + at.out, n * sizeof(RibbitNearest), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    for (size_t i = 0; i < n; ++i) {
        const RibbitNearest &r = buf.h_near.p[i];
        const int64_t t = (int64_t)n_targets;
        if (r.kind < 0 || r.kind > 2 || r.hit < -1 || r.hit >= t || r.left < -1 || r.left >= t || r.right < -1 || r.right >= t || (r.kind > 0) != (r.hit >= 0))
            return fail(RIBBIT_E_INTERNAL, "query %zu: what the GPU found nearest contradicts itself", i);
    }
    return RIBBIT_OK;
}

// ---- host twin: order A and order B as sorted arrays, M as a running maximum that remembers where it rose
int host_record_nearest_impl(int64_t length, const int32_t *queries, size_t n, const int32_t *targets, size_t n_targets, RibbitNearest **out) {
    int rc;
    if ((rc = check_sets(queries, n, targets, n_targets, out))) return rc;
    if (length < 0 || length > (int64_t)INT32_MAX) return fail(RIBBIT_E_ARG, "a record of %lld bases", (long long)length);
    const std::vector<ClippedRow> a = clipped_sorted_rows(length, targets, n_targets, [](const ClippedRow &x, const ClippedRow &y) {
        return x.s != y.s ? x.s < y.s : x.e != y.e ? x.e < y.e : x.index < y.index;
    });
    const std::vector<ClippedRow> b = clipped_sorted_rows(length, targets, n_targets, [](const ClippedRow &x, const ClippedRow &y) {
        return x.e != y.e ? x.e < y.e : x.s != y.s ? x.s < y.s : x.index < y.index;
    });
    std::vector<int64_t> reach(a.size());      // M[k]
    std::vector<size_t> reach_at(a.size());    // the lowest position that holds it
    for (size_t k = 0; k < a.size(); ++k) {
        const bool rises = k == 0 || a[k].e > reach[k - 1];
        reach[k] = rises ? a[k].e : reach[k - 1];
        reach_at[k] = rises ? k : reach_at[k - 1];
    }
    Handed<RibbitNearest> found;
    if ((rc = hand_out<RibbitNearest>(nullptr, n, false, found))) return rc;
    for (size_t i = 0; i < n; ++i) {
        const int64_t s = std::max<int64_t>(queries[2 * i], 0), e = std::min<int64_t>(queries[2 * i + 1], length);
        RibbitNearest r = NOTHING;
        if (s < e) {
            const size_t pa = (size_t)(std::upper_bound(a.begin(), a.end(), s, [](int64_t v, const ClippedRow &x) { return v < x.s; }) - a.begin());
            const size_t pe = (size_t)(std::lower_bound(a.begin(), a.end(), e, [](const ClippedRow &x, int64_t v) { return x.s < v; }) - a.begin());
            const size_t pb = (size_t)(std::upper_bound(b.begin(), b.end(), s, [](int64_t v, const ClippedRow &x) { return v < x.e; }) - b.begin());
            if (pa > 0 && reach[pa - 1] >= e) {
                r.kind = RIBBIT_NEAREST_INSIDE;
                r.hit = (int32_t)a[reach_at[pa - 1]].index;
            } else {
                const size_t po = (size_t)(std::upper_bound(reach.begin(), reach.begin() + (std::ptrdiff_t)pe, s) - reach.begin());
                if (po < pe) {
                    r.kind = RIBBIT_NEAREST_OVER;
                    r.hit = (int32_t)a[po].index;
                }
            }
            if (pb > 0) {
                r.left = (int32_t)b[pb - 1].index;
                r.left_dist = (int32_t)(s - b[pb - 1].e);
            }
            if (pe < a.size()) {
                r.right = (int32_t)a[pe].index;
                r.right_dist = (int32_t)(a[pe].s - e);
            }
        }
        found[i] = r;
    }
    *out = found.release();
    return RIBBIT_OK;
}

// ---- the two texts
// One set of intervals with their labels, as a text names them: the other file's intervals, or the record's rows with their motifs.
struct Named {
    const int32_t *iv;
    const char *pool;
    const int32_t *offsets;
    size_t n;
    const char *noun;      // what one of them is, in the caller's words
};

int check_named(const Named &t, const char *labels_noun) {
    if ((!t.iv && t.n > 0) || !t.offsets) return fail(RIBBIT_E_ARG, "null argument");
    if (t.n > MAX_INTERVALS) return fail(RIBBIT_E_ARG, "%zu %ss", t.n, t.noun);
    if (t.offsets[0] < 0) return fail(RIBBIT_E_ARG, "the %s' offsets start at %d, below 0", labels_noun, (int)t.offsets[0]);
    for (size_t j = 0; j < t.n; ++j)
        if (t.offsets[j + 1] < t.offsets[j])
            return fail(RIBBIT_E_ARG, "%s %zu: the %s' offsets do not ascend (%d, then %d)", t.noun, j, labels_noun, (int)t.offsets[j], (int)t.offsets[j + 1]);
    if (t.offsets[t.n] > 0 && !t.pool) return fail(RIBBIT_E_ARG, "null argument");
    const size_t pool_len = t.pool ? std::strlen(t.pool) : 0;
    if ((size_t)t.offsets[t.n] > pool_len)
        return fail(RIBBIT_E_ARG, "the %s' offsets end at %d, behind the %zu bytes of their pool", labels_noun, (int)t.offsets[t.n], pool_len);
    return RIBBIT_OK;
}

enum : int { FINE = 0, KIND, HIT, LEFT, RIGHT };      // a refusal's why; a: the query

inline int bad_field(const RibbitNearest &r, size_t n_named) {
    const int64_t t = (int64_t)n_named;
    if (r.kind < 0 || r.kind > 2) return KIND;
    if (r.hit < -1 || r.hit >= t) return HIT;
    if (r.left < -1 || r.left >= t) return LEFT;
    if (r.right < -1 || r.right >= t) return RIGHT;
    return FINE;
}

int word_refusal(const PieceRefusal &b, const RibbitNearest *nearest, const char *query_noun, const Named &t) {
    const RibbitNearest &r = nearest[b.a];
    switch (b.why) {
        case KIND: return fail(RIBBIT_E_ARG, "%s %zu: a kind of %d, not 0, 1 or 2", query_noun, b.a, (int)r.kind);
        case HIT: return fail(RIBBIT_E_ARG, "%s %zu: its hit %d is none of the %zu %ss", query_noun, b.a, (int)r.hit, t.n, t.noun);
        case LEFT: return fail(RIBBIT_E_ARG, "%s %zu: its left neighbour %d is none of the %zu %ss", query_noun, b.a, (int)r.left, t.n, t.noun);
        default: return fail(RIBBIT_E_ARG, "%s %zu: its right neighbour %d is none of the %zu %ss", query_noun, b.a, (int)r.right, t.n, t.noun);
    }
}

inline void put_label(std::string &out, const Named &t, int32_t j) {
    out += '\t';
    if (j < 0) { out += '.'; return; }
    const int32_t from = t.offsets[j], to = t.offsets[j + 1];
    if (to > from) out.append(t.pool + from, (size_t)(to - from)); else out += '.';
}

inline void put_distance(std::string &out, int32_t j, int32_t dist) {
    out += '\t';
    if (j < 0) out += '.'; else put_number(out, dist);
}

// the eight columns, each behind a tab: in | over | ., the hit's label, start and end, the neighbours' labels and distances
void put_nearest(std::string &out, const RibbitNearest &r, const Named &t) {
    out += r.kind == RIBBIT_NEAREST_INSIDE ? "\tin" : r.kind == RIBBIT_NEAREST_OVER ? "\tover" : "\t.";
    put_label(out, t, r.hit);
    for (int k = 0; k < 2; ++k) {
        out += '\t';
        if (r.hit < 0) out += '.'; else put_number(out, t.iv[2 * r.hit + k]);
    }
    put_label(out, t, r.left);
    put_distance(out, r.left, r.left_dist);
    put_label(out, t, r.right);
    put_distance(out, r.right, r.right_dist);
}

int bed_nearest_text_impl(const char *bed, size_t bed_len, const RibbitNearest *nearest, size_t n, const int32_t *targets, const char *labels,
                          const int32_t *label_offsets, size_t n_targets, char **text, size_t *len) {
    if (!text || !len || (!bed && bed_len > 0) || (!nearest && n > 0)) return fail(RIBBIT_E_ARG, "null argument");
    const Named t{targets, labels, label_offsets, n_targets, "interval"};
    int rc;
    if ((rc = check_named(t, "labels"))) return rc;
    const size_t parts = bed_text_parts(bed_len);
    BedLines lines;
    if ((rc = lines.find(bed, bed_len, parts))) return rc;
    if (lines.count() != n) return fail(RIBBIT_E_ARG, "the BED text has %zu lines, not the %zu of the rows", lines.count(), n);
    // piece k writes lines [n k / parts, n (k + 1) / parts): every line grows by eight columns
    return write_pieces(parts, "the rows' nearest intervals", text, len, [&](size_t k, std::string &out) {
        const size_t from = n * k / parts, to = n * (k + 1) / parts;
        out.reserve(lines.start[to] - lines.start[from] + 64 * (to - from));
        for (size_t i = from; i < to; ++i) {
            if (const int why = bad_field(nearest[i], n_targets)) return PieceRefusal{why, i, 0};
            put_field(out, lines[i]);
            put_nearest(out, nearest[i], t);
            out += '\n';
        }
        return PieceRefusal{};
    }, [&](const PieceRefusal &b) { return word_refusal(b, nearest, "row", t); });
}

int nearest_other_text_impl(const char *name, const int32_t *targets, const char *labels, const int32_t *label_offsets, size_t n_targets,
                            const RibbitNearest *nearest, const int32_t *rows, const char *motifs, const int32_t *motif_offsets, size_t n_rows, char **text,
                            size_t *len) {
    if (!name || !text || !len || (!nearest && n_targets > 0)) return fail(RIBBIT_E_ARG, "null argument");
    const Named other{targets, labels, label_offsets, n_targets, "interval"}, t{rows, motifs, motif_offsets, n_rows, "row"};
    int rc;
    if ((rc = check_named(other, "labels")) || (rc = check_named(t, "motifs"))) return rc;
    const size_t name_len = std::strlen(name), n = n_targets;
    const size_t parts = bed_text_parts(n * 64);
    return write_pieces(parts, "the intervals' nearest rows", text, len, [&](size_t k, std::string &out) {
        const size_t from = n * k / parts, to = n * (k + 1) / parts;
        out.reserve((name_len + 96) * (to - from));
        for (size_t j = from; j < to; ++j) {
            if (const int why = bad_field(nearest[j], n_rows)) return PieceRefusal{why, j, 0};
            out.append(name, name_len);
            for (int c = 0; c < 2; ++c) {
                out += '\t';
                put_number(out, targets[2 * j + c]);
            }
            put_label(out, other, (int32_t)j);
            put_nearest(out, nearest[j], t);
            out += '\n';
        }
        return PieceRefusal{};
    }, [&](const PieceRefusal &b) { return word_refusal(b, nearest, "interval", t); });
}

}  // namespace

extern "C" {

int ribbit_hip_record_nearest(RibbitHandle *h, const int32_t *queries, size_t n, const int32_t *targets, size_t n_targets, const RibbitNearest **out) {
    return guarded("the nearest intervals", [&]() -> int { return record_nearest_impl(h, queries, n, targets, n_targets, out); });
}

int ribbit_host_record_nearest(int64_t length, const int32_t *queries, size_t n, const int32_t *targets, size_t n_targets, RibbitNearest **out) {
    return guarded("the nearest intervals", [&]() -> int { return host_record_nearest_impl(length, queries, n, targets, n_targets, out); });
}

void ribbit_nearest_free(RibbitNearest *nearest) { std::free(nearest); }

int ribbit_bed_nearest_text(const char *bed_text, size_t bed_len, const RibbitNearest *nearest, size_t n, const int32_t *targets, const char *labels,
                            const int32_t *label_offsets, size_t n_targets, char **text, size_t *len) {
    return guarded("the rows' nearest intervals as text", [&]() -> int {
        return bed_nearest_text_impl(bed_text, bed_len, nearest, n, targets, labels, label_offsets, n_targets, text, len);
    });
}

int ribbit_nearest_other_text(const char *name, const int32_t *targets, const char *labels, const int32_t *label_offsets, size_t n_targets,
                              const RibbitNearest *nearest, const int32_t *rows, const char *motifs, const int32_t *motif_offsets, size_t n_rows, char **text,
                              size_t *len) {
    return guarded("the intervals' nearest rows as text", [&]() -> int {
        return nearest_other_text_impl(name, targets, labels, label_offsets, n_targets, nearest, rows, motifs, motif_offsets, n_rows, text, len);
    });
}

}  // extern "C"
