// bed_text.h -- the refined BED text as the row outputs read and write it (api_mask.cpp, api_loci.cpp, api_overlap.cpp, api_best.cpp,
// api_classes.cpp, api_compound.cpp, api_interruptions.cpp, api_nearest.cpp, api_repeats.cpp): the row format, the reader that walks a text in
// pieces of whole lines on the host thread team, and the writer that builds a text in pieces and joins them.  No GPU.  What makes a
// field acceptable, and the words of every refusal, stay with the callers.
// Not part of the ABI; nothing outside ribbit_amd/csrc includes it.
#pragma once
#include "api_internal.h"

#include <charconv>

namespace rbapi {

constexpr size_t BED_MAX_ROWS = (size_t)INT32_MAX;      // (row indices are int32)
constexpr size_t BED_MAX_POOL = (size_t)INT32_MAX;      // (and so are the offsets into a pool)

// ---- the row format
// A row is 11 tab-separated columns, read from the right, so that a record name with a tab in it still parses:
//     name | start | end | motif | . | . | units | . | . | . | CIGAR
struct BedField {
    const char *from = nullptr, *to = nullptr;
    size_t size() const { return (size_t)(to - from); }
};
struct BedRow {
    bool ok = false;           // false: fewer than ten tabs, this is not a row
    const char *tail = nullptr;      // the tenth tab from the right: [tail, eol) is the row without its name
    BedField start, end, motif, units, cigar;
};
// the fields of the line [p, eol) (eol: its newline, or the text's end)
inline BedRow bed_row(const char *p, const char *eol) {
    const char *tab[10];       // the last ten tabs, from the right
    const char *q = eol;
    for (int k = 0; k < 10; ++k) {
        q = static_cast<const char *>(memrchr(p, '\t', (size_t)(q - p)));
        if (!q) return BedRow{};
        tab[k] = q;
    }
    BedRow row;
    row.ok = true;
    row.tail = tab[9];
    row.start = BedField{tab[9] + 1, tab[8]};
    row.end = BedField{tab[8] + 1, tab[7]};
    row.motif = BedField{tab[7] + 1, tab[6]};
    row.units = BedField{tab[4] + 1, tab[3]};
    row.cigar = BedField{tab[0] + 1, eol};
    return row;
}

// ---- the reader
// a chromosome's BED is 150-200 MB of text: it is walked in pieces, one thread per piece of at least 4 MB
inline size_t bed_text_parts(size_t len) { return std::max<size_t>(1, std::min<size_t>(std::min(rb::host_thread_count(0), 16u), len >> 22)); }

// What reading came to: the first piece that ran out of memory or met a line its callback refused decides.
struct BedRead {
    bool oom = false;
    const char *bad = nullptr;      // where the refused line starts
};
// The text cut into bed_text_parts(len) pieces of whole lines, one accumulator per piece (acc is sized here); per_line(acc[k],
// row, p, eol) for every line of piece k in order, on the host thread team; it returns false to refuse the line, which ends its piece.
template <typename Acc, typename PerLine>
BedRead bed_read(const char *text, size_t len, std::vector<Acc> &acc, PerLine per_line) {
    const size_t parts = bed_text_parts(len);
    std::vector<const char *> cut(parts + 1, text + len);
    cut[0] = text;
    for (size_t k = 1; k < parts; ++k) {
        const char *at = std::max(cut[k - 1], text + len * k / parts);
        const char *nl = at > text ? static_cast<const char *>(std::memchr(at - 1, '\n', (size_t)(text + len - (at - 1)))) : at - 1;
        cut[k] = nl ? nl + 1 : text + len;
    }
    acc.resize(parts);
    std::vector<BedRead> read(parts);
    rb::on_threads((unsigned)parts, [&](unsigned k) {
        try {
            for (const char *p = cut[k], *end = cut[k + 1]; p < end;) {
                const char *eol = static_cast<const char *>(std::memchr(p, '\n', (size_t)(end - p)));
                if (!eol) eol = end;
                if (!per_line(acc[k], bed_row(p, eol), p, eol)) { read[k].bad = p; return; }
                p = eol + 1;
            }
        } catch (const std::bad_alloc &) { read[k].oom = true; }
    });
    for (const BedRead &r : read)
        if (r.oom || r.bad) return r;
    return BedRead{};
}

// One string field of every line as a pool with n + 1 int32 offsets (malloc memory, the pool zero-terminated).  pick(row) is the
// field, or an empty BedField{} to refuse the line: refuse(byte offset of the line) then words that; `noun` names the fields in
// the two refusals worded here.
template <typename Pick, typename Refuse>
int bed_gather(const char *text, size_t len, const char *noun, Pick pick, Refuse refuse, char **pool, int32_t **offsets, size_t *n) {
    struct Piece { std::string pool; std::vector<int32_t> lens; };
    std::vector<Piece> piece;
    const BedRead read = bed_read(text, len, piece, [&](Piece &a, const BedRow &row, const char *, const char *) {
        const BedField f = row.ok ? pick(row) : BedField{};
        if (!f.from) return false;
        a.pool.append(f.from, f.size());
        a.lens.push_back((int32_t)f.size());
        return true;
    });
    if (read.oom) return fail(RIBBIT_E_NOMEM, "out of host memory reading the %s", noun);
    if (read.bad) return refuse((size_t)(read.bad - text));
    size_t bytes = 0, rows = 0;
    for (const Piece &a : piece) {
        bytes += a.pool.size();
        rows += a.lens.size();
    }
    if (bytes > BED_MAX_POOL || rows > BED_MAX_ROWS) return fail(RIBBIT_E_ARG, "%zu rows with %zu bytes of %s", rows, bytes, noun);
    Handed<char> out;
    int rc;
    if ((rc = hand_out<char>(nullptr, bytes, true, out)) || (rc = hand_out<int32_t>(nullptr, rows + 1, false, offsets))) return rc;
    size_t at = 0, row = 0;
    for (const Piece &a : piece) {
        std::memcpy(out.get() + at, a.pool.data(), a.pool.size());
        for (const int32_t l : a.lens) {
            (*offsets)[row++] = (int32_t)at;
            at += (size_t)l;
        }
    }
    (*offsets)[rows] = (int32_t)at;
    *pool = out.release();
    *n = rows;
    return RIBBIT_OK;
}

// ---- the writer
// where the lines of a BED text start: line i is [start[i], start[i + 1]), its newline included; a last line without its newline
// counts.  Until find() has run there are no lines.
struct BedLines {
    const char *bed = nullptr;
    std::vector<size_t> start{0};
    size_t count() const { return start.size() - 1; }
    // line i without its newline
    BedField operator[](size_t i) const {
        const char *p = bed + start[i], *eol = bed + start[i + 1];
        if (eol > p && eol[-1] == '\n') --eol;
        return BedField{p, eol};
    }
    // the newlines are found in `parts` pieces, one thread per piece
    int find(const char *text, size_t len, size_t parts) {
        bed = text;
        std::vector<std::vector<size_t>> starts(parts);      // per piece: the offsets just behind its newlines
        std::vector<char> oom(parts, 0);
        rb::on_threads((unsigned)parts, [&](unsigned k) {
            try {
                const char *p = text + len * k / parts, *end = text + len * (k + 1) / parts;
                while (p < end && (p = static_cast<const char *>(std::memchr(p, '\n', (size_t)(end - p)))) != nullptr) starts[k].push_back((size_t)(++p - text));
            } catch (const std::bad_alloc &) { oom[k] = 1; }
        });
        start.assign(1, 0);
        for (size_t k = 0; k < parts; ++k) {
            if (oom[k]) return fail(RIBBIT_E_NOMEM, "out of host memory reading BED rows");
            start.insert(start.end(), starts[k].begin(), starts[k].end());
        }
        if (start.back() != len) start.push_back(len);
        return RIBBIT_OK;
    }
};

inline void put_number(std::string &out, int64_t v) {
    char num[24];
    out.append(num, (size_t)(std::to_chars(num, num + sizeof num, v).ptr - num));
}
inline void put_field(std::string &out, BedField f) { out.append(f.from, f.size()); }

// the pieces one behind the other as one zero-terminated text the caller frees
inline int join_text(const std::vector<std::string> &piece, char **text, size_t *len) {
    size_t total = 0;
    for (const std::string &s : piece) total += s.size();
    int rc;
    if ((rc = hand_out<char>(nullptr, total, true, text))) return rc;
    size_t at = 0;
    for (const std::string &s : piece) {
        std::memcpy(*text + at, s.data(), s.size());
        at += s.size();
    }
    *len = total;
    return RIBBIT_OK;
}

// What a piece's body found wrong with its input (why == 0: nothing); the caller gives `why`, `a` and `b` their meaning and words it.
struct PieceRefusal {
    int why = 0;
    size_t a = 0, b = 0;
};
// body(k, out) -> PieceRefusal for every piece k of `parts` on the host thread team, then the pieces joined.  A piece that runs
// out of memory is RIBBIT_E_NOMEM "out of host memory writing <what>"; the first piece with a refusal of its own has it worded by
// refuse(refusal) -> status.
template <typename Body, typename Refuse>
int write_pieces(size_t parts, const char *what, char **text, size_t *len, Body body, Refuse refuse) {
    std::vector<std::string> piece(parts);
    std::vector<PieceRefusal> bad(parts);
    std::vector<char> oom(parts, 0);
    rb::on_threads((unsigned)parts, [&](unsigned k) {
        try { bad[k] = body((size_t)k, piece[k]); } catch (const std::bad_alloc &) { oom[k] = 1; }
    });
    for (size_t k = 0; k < parts; ++k) {
        if (oom[k]) return fail(RIBBIT_E_NOMEM, "out of host memory writing %s", what);
        if (bad[k].why) return refuse(bad[k]);
    }
    return join_text(piece, text, len);
}
// ... for a body that refuses nothing
template <typename Body>
int write_pieces(size_t parts, const char *what, char **text, size_t *len, Body body) {
    return write_pieces(parts, what, text, len, [&](size_t k, std::string &out) { body(k, out); return PieceRefusal{}; },
                        [](const PieceRefusal &) { return (int)RIBBIT_E_INTERNAL; });
}

}  // namespace rbapi
