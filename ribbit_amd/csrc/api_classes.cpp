// api_classes.cpp -- the rows of a record grouped by canonical motif class (classes.hip); see api_internal.h for the map of the files
// behind include/ribbit_hip.h.  The GPU form stages the rows, the offsets and the motifs through stage_down (it reads no coverage
// bitmap), runs on the handle's stream and keeps nothing between calls; the host twin is written from the
// contract: a least rotation of every motif and of its reverse complement on the host thread team, one sort, one sweep.  The
// motifs of a BED text and the two outputs' texts need no GPU.
#include "bed_text.h"

namespace {

constexpr size_t MAX_ROWS = BED_MAX_ROWS;
constexpr int32_t MAX_MOTIF = 1023;

inline bool is_base(char c) { return c == 'A' || c == 'C' || c == 'G' || c == 'T'; }
inline char complement(char c) { return c == 'A' ? 'T' : c == 'C' ? 'G' : c == 'G' ? 'C' : 'A'; }

// host threads for n rows: one per 64 Ki rows, at most the team's size
unsigned row_threads(size_t n, unsigned asked = 0) { return (unsigned)std::max<size_t>(1, std::min<size_t>(rb::host_thread_count(asked), n >> 16)); }

// what both forms ask of their inputs; the first bad row decides the message
int check_class_args(const int32_t *intervals, size_t n, const char *motifs, const int32_t *offsets, const void *classes, const void *strands,
                     const void *groups, const size_t *n_groups, unsigned threads) {
    if ((!intervals && n > 0) || (!offsets && n > 0) || !classes || !strands || !groups || !n_groups) return fail(RIBBIT_E_ARG, "null argument");
    if (n > MAX_ROWS) return fail(RIBBIT_E_ARG, "%zu rows", n);
    if (n == 0) return RIBBIT_OK;
    if (offsets[0] != 0) return fail(RIBBIT_E_ARG, "the motifs' offsets start at %d, not at 0", (int)offsets[0]);
    // (an int32 offset cannot reach 2^31: a pool of 2^31 bytes or more shows as offsets that do not ascend)
    const unsigned nt = row_threads(n, threads);
    std::vector<size_t> bad(nt, (size_t)-1);
    rb::over_pieces(n, nt, [&](size_t from, size_t to, unsigned t) {
        for (size_t i = from; i < to; ++i) {
            const int64_t k = (int64_t)offsets[i + 1] - offsets[i];
            bool ok = k >= 1 && k <= MAX_MOTIF && motifs;
            for (int64_t j = 0; ok && j < k; ++j) ok = is_base(motifs[offsets[i] + j]);
            if (!ok) { bad[t] = i; return; }
        }
    });
    for (const size_t i : bad) {
        if (i == (size_t)-1) continue;
        const int64_t k = (int64_t)offsets[i + 1] - offsets[i];
        if (!motifs) return fail(RIBBIT_E_ARG, "null argument");
        if (k < 0) return fail(RIBBIT_E_ARG, "row %zu: the motifs' offsets do not ascend (%d, then %d; a pool has fewer than 2^31 bytes)", i, (int)offsets[i], (int)offsets[i + 1]);
        if (k == 0) return fail(RIBBIT_E_ARG, "row %zu: an empty motif", i);
        if (k > MAX_MOTIF) return fail(RIBBIT_E_ARG, "row %zu: a motif of %lld bytes (at most %d)", i, (long long)k, (int)MAX_MOTIF);
        return fail(RIBBIT_E_ARG, "row %zu: a motif with a byte outside ACGT", i);
    }
    return RIBBIT_OK;
}

constexpr size_t HEADER_BYTES = 16;
static_assert(sizeof(rb::ClassHeader) == HEADER_BYTES && sizeof(RibbitMotifClass) == 24, "the groups follow the header in one buffer");

int record_classes_impl(RibbitHandle *h, const int32_t *intervals, size_t n, const char *motifs, const int32_t *offsets, const char **classes,
                        const char **strands, const RibbitMotifClass **groups, size_t *n_groups) {
    if (!h) return fail(RIBBIT_E_ARG, "null handle");
    int rc;
    if ((rc = check_class_args(intervals, n, motifs, offsets, classes, strands, groups, n_groups, h->host_threads))) return rc;
    if (!h->loaded) return fail(RIBBIT_E_STATE, "no record loaded");
    static const char kNoText[1] = {0};
    static const RibbitMotifClass kNoGroups[1] = {};
    *classes = *strands = kNoText;
    *groups = kNoGroups;
    *n_groups = 0;
    if (n == 0) return RIBBIT_OK;
    if ((rc = bind_device(h))) return rc;
    // down: the rows | the offsets | the motifs, each on a 16-byte boundary (the motifs are read in aligned 8-byte words, up to one
    // word past their end); up: the header | n groups of room | the strands | the classes
    const size_t pool = (size_t)offsets[n];
    const size_t out_strands = HEADER_BYTES + n * sizeof(RibbitMotifClass), out_classes = out_strands + round16(n), out_bytes = out_classes + pool;
    RibbitHandle::RowBufs &buf = h->rows;
    const rb::ClassesLayout at = rb::classes_layout((int64_t)n, pool);
    if ((rc = buf.d_work.ensure(at.bytes, true))) return rc;
    if ((rc = buf.h_class.ensure(out_bytes, true))) return rc;
    const StageSegment down[3] = {{intervals, 2 * n * sizeof(int32_t)}, {offsets, (n + 1) * sizeof(int32_t)}, {motifs, pool}};
    const uint8_t *d_in[3];
    if ((rc = stage_down(h, down, 3, d_in))) return rc;
    uint8_t *work = buf.d_work.p, *to = buf.h_class.p;
    HIP_TRY(rb::launch_classes(reinterpret_cast<const int32_t *>(d_in[0]), reinterpret_cast<const int32_t *>(d_in[1]), d_in[2], (int64_t)n, h->length, work,
                               buf.d_work.cap, at, h->stream));
    HIP_TRY(hipMemcpyAsync(to, work + at.header, HEADER_BYTES, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipMemcpyAsync(to + HEADER_BYTES, work + at.groups, n * sizeof(RibbitMotifClass), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipMemcpyAsync(to + out_strands, work + at.strands, n, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipMemcpyAsync(to + out_classes, work + at.classes, pool, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    rb::ClassHeader header;
    std::memcpy(&header, buf.h_class.p, sizeof header);
    if (header.groups == 0 || header.groups > n || header.long_rows > n) return fail(RIBBIT_E_INTERNAL, "the classes' counts contradict each other");
    const char *up = reinterpret_cast<const char *>(buf.h_class.p);
    *classes = up + out_classes;
    *strands = up + out_strands;
    *groups = reinterpret_cast<const RibbitMotifClass *>(up + HEADER_BYTES);
    *n_groups = (size_t)header.groups;
    return RIBBIT_OK;
}

// ---- host twin
// where the least rotation of the k bytes at s starts (the lowest such start), in O(k)
size_t least_rotation(const char *s, size_t k) {
    size_t i = 0, j = 1, l = 0;
    while (i < k && j < k && l < k) {
        const char a = s[(i + l) % k], b = s[(j + l) % k];
        if (a == b) { ++l; continue; }
        if (a > b) i += l + 1; else j += l + 1;
        if (i == j) ++j;
        l = 0;
    }
    return std::min(i, j);
}

int host_record_classes_impl(int64_t length, const int32_t *intervals, size_t n, const char *motifs, const int32_t *offsets, char **classes, char **strands,
                             RibbitMotifClass **groups, size_t *n_groups) {
    int rc;
    if ((rc = check_class_args(intervals, n, motifs, offsets, classes, strands, groups, n_groups, 0))) return rc;
    if (length < 0 || length > (int64_t)INT32_MAX) return fail(RIBBIT_E_ARG, "a record of %lld bases", (long long)length);
    const size_t pool = n ? (size_t)offsets[n] : 0;
    Handed<char> cls, str;
    if ((rc = hand_out<char>(nullptr, pool, true, cls)) || (rc = hand_out<char>(nullptr, n, true, str))) return rc;
    rb::over_pieces(n, row_threads(n), [&](size_t from, size_t to, unsigned) {
        char rc_text[MAX_MOTIF];
        for (size_t i = from; i < to; ++i) {
            const char *u = motifs + offsets[i];
            const size_t k = (size_t)(offsets[i + 1] - offsets[i]);
            for (size_t t = 0; t < k; ++t) rc_text[k - 1 - t] = complement(u[t]);
            const size_t a = least_rotation(u, k), b = least_rotation(rc_text, k);
            int order = 0;
            for (size_t t = 0; t < k && !order; ++t) order = (int)(unsigned char)u[(a + t) % k] - (int)(unsigned char)rc_text[(b + t) % k];
            const char *from_text = order <= 0 ? u : rc_text;
            const size_t at = order <= 0 ? a : b;
            char *out = cls.get() + offsets[i];
            std::memcpy(out, from_text + at, k - at);
            std::memcpy(out + (k - at), from_text, at);
            str[i] = order <= 0 ? '+' : '-';
        }
    });
    std::vector<int32_t> order(n);
    for (size_t i = 0; i < n; ++i) order[i] = (int32_t)i;
    auto compare = [&](int32_t a, int32_t b) {      // < 0, 0, > 0 by (length, class)
        const int32_t ka = offsets[a + 1] - offsets[a], kb = offsets[b + 1] - offsets[b];
        return ka != kb ? (ka < kb ? -1 : 1) : std::memcmp(cls.get() + offsets[a], cls.get() + offsets[b], (size_t)ka);
    };
    std::sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { const int c = compare(a, b); return c ? c < 0 : a < b; });
    std::vector<RibbitMotifClass> found;
    int64_t longest = -1;
    for (size_t j = 0; j < n; ++j) {
        const int32_t i = order[j];
        const int64_t s = std::max<int64_t>(intervals[2 * (size_t)i], 0), e = std::min<int64_t>(intervals[2 * (size_t)i + 1], length);
        const int64_t width = std::max<int64_t>(e - s, 0);
        if (j == 0 || compare(order[j - 1], i) != 0) {
            found.push_back(RibbitMotifClass{0, offsets[i + 1] - offsets[i], 0, i, i});      // (a group's rows come by ascending index)
            longest = -1;
        }
        RibbitMotifClass &g = found.back();
        g.rows += 1;
        g.bases += width;
        if (width > longest) { longest = width; g.longest_row = i; }
    }
    if ((rc = hand_out(found.data(), found.size(), false, groups))) return rc;
    *classes = cls.release();
    *strands = str.release();
    *n_groups = found.size();
    return RIBBIT_OK;
}

// ---- the motifs of a BED text
int bed_motifs_impl(const char *text, size_t len, char **pool, int32_t **offsets, size_t *n) {
    if (!pool || !offsets || !n || (!text && len > 0)) return fail(RIBBIT_E_ARG, "null argument");
    return bed_gather(text, len, "motifs", [](const BedRow &row) {
        const BedField m = row.motif;
        return m.to > m.from && m.to - m.from <= MAX_MOTIF && std::all_of(m.from, m.to, is_base) ? m : BedField{};
    }, [](size_t at) {
        return fail(RIBBIT_E_ARG, "BED text at byte %zu is not a row of 11 tab-separated columns whose motif is 1 .. %d bytes over ACGT", at, (int)MAX_MOTIF);
    }, pool, offsets, n);
}

// ---- the two outputs as text
int bed_class_text_impl(const char *bed, size_t bed_len, const char *classes, const int32_t *offsets, const char *strands, size_t n, char **text, size_t *len) {
    if (!text || !len || (!bed && bed_len > 0) || ((!classes || !offsets || !strands) && n > 0)) return fail(RIBBIT_E_ARG, "null argument");
    const size_t parts = bed_text_parts(bed_len);
    BedLines lines;
    int rc;
    if ((rc = lines.find(bed, bed_len, parts))) return rc;
    if (lines.count() != n) return fail(RIBBIT_E_ARG, "the BED text has %zu lines, not the %zu of the rows", lines.count(), n);
    for (size_t i = 0; i < n; ++i)
        if (offsets[i] < 0 || offsets[i + 1] < offsets[i]) return fail(RIBBIT_E_ARG, "row %zu: the classes' offsets do not ascend", i);
    // piece k writes lines [n k / parts, n (k + 1) / parts): every line grows by two tabs, its class and its strand
    return write_pieces(parts, "the rows' classes", text, len, [&](size_t k, std::string &out) {
        const size_t from = n * k / parts, to = n * (k + 1) / parts;
        out.reserve(lines.start[to] - lines.start[from] + (size_t)(offsets[to] - offsets[from]) + 4 * (to - from));
        for (size_t i = from; i < to; ++i) {
            put_field(out, lines[i]);
            out += '\t';
            out.append(classes + offsets[i], (size_t)(offsets[i + 1] - offsets[i]));
            out += '\t';
            out += strands[i];
            out += '\n';
        }
    });
}

int class_summary_text_impl(const char *name, const int32_t *intervals, size_t n, const char *classes, const int32_t *offsets, const RibbitMotifClass *groups,
                            size_t n_groups, char **text, size_t *len) {
    if (!name || !text || !len || ((!intervals || !classes || !offsets) && n > 0) || (!groups && n_groups > 0)) return fail(RIBBIT_E_ARG, "null argument");
    const size_t name_len = std::strlen(name);
    std::vector<std::string> piece(1);
    std::string &out = piece[0];
    for (size_t g = 0; g < n_groups; ++g) {
        const RibbitMotifClass &c = groups[g];
        if (c.first_row < 0 || (size_t)c.first_row >= n || c.longest_row < 0 || (size_t)c.longest_row >= n)
            return fail(RIBBIT_E_ARG, "group %zu: rows %d and %d of %zu rows", g, (int)c.first_row, (int)c.longest_row, n);
        const int32_t from = offsets[c.first_row], k = offsets[c.first_row + 1] - from;
        if (from < 0 || k != c.length) return fail(RIBBIT_E_ARG, "group %zu: a class of %d bases whose first row's has %d", g, (int)c.length, (int)k);
        out.append(name, name_len);
        out += '\t';
        out.append(classes + from, (size_t)k);
        for (const int64_t v : {(int64_t)c.length, (int64_t)c.rows, c.bases, (int64_t)intervals[2 * (size_t)c.longest_row], (int64_t)intervals[2 * (size_t)c.longest_row + 1]}) {
            out += '\t';
            put_number(out, v);
        }
        out += '\n';
    }
    return join_text(piece, text, len);
}

}  // namespace

extern "C" {

int ribbit_bed_motifs(const char *bed_text, size_t bed_len, char **pool, int32_t **offsets, size_t *n) {
    return guarded("reading the motifs", [&]() -> int { return bed_motifs_impl(bed_text, bed_len, pool, offsets, n); });
}

int ribbit_hip_record_classes(RibbitHandle *h, const int32_t *intervals, size_t n, const char *motifs, const int32_t *offsets, const char **classes,
                              const char **strands, const RibbitMotifClass **groups, size_t *n_groups) {
    return guarded("the motif classes", [&]() -> int { return record_classes_impl(h, intervals, n, motifs, offsets, classes, strands, groups, n_groups); });
}

int ribbit_host_record_classes(int64_t length, const int32_t *intervals, size_t n, const char *motifs, const int32_t *offsets, char **classes, char **strands,
                               RibbitMotifClass **groups, size_t *n_groups) {
    return guarded("the motif classes", [&]() -> int { return host_record_classes_impl(length, intervals, n, motifs, offsets, classes, strands, groups, n_groups); });
}

void ribbit_motif_classes_free(RibbitMotifClass *groups) { std::free(groups); }

int ribbit_bed_class_text(const char *bed_text, size_t bed_len, const char *classes, const int32_t *offsets, const char *strands, size_t n, char **text,
                          size_t *len) {
    return guarded("the rows' classes as text", [&]() -> int { return bed_class_text_impl(bed_text, bed_len, classes, offsets, strands, n, text, len); });
}

int ribbit_class_summary_text(const char *name, const int32_t *intervals, size_t n, const char *classes, const int32_t *offsets, const RibbitMotifClass *groups,
                              size_t n_groups, char **text, size_t *len) {
    return guarded("the classes' summary", [&]() -> int { return class_summary_text_impl(name, intervals, n, classes, offsets, groups, n_groups, text, len); });
}

}  // extern "C"
