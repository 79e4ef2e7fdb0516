// primers_host.h -- what the host sides of the primer outputs share (api_primers.cpp, api_primer_pairs.cpp, api_primer_products.cpp,
// api_primer_specific.cpp, api_primer_genome.cpp, api_amplicons.cpp): the checks of RibbitPrimerParams, of a call's arguments and of a
// twin's sequence with their wording, a target's two windows, one candidate judged from the bytes of the sequence letter by letter
// (the five rules and the Tm table as include/ribbit_hip.h states them), the columns of a primer and of a pair as text and the
// writer of the texts that are made of them, and the host code of one twin that another twin calls.  No GPU, and nothing of the
// kernels' packed forms.
// Not part of the ABI; nothing outside ribbit_amd/csrc includes it.
#pragma once
#include <map>
#include <string>

#include "bed_text.h"

namespace rbapi {

constexpr size_t MAX_TARGETS = (size_t)INT32_MAX;
static_assert(sizeof(RibbitRowPrimers) == 56 && sizeof(RibbitPrimer) == 24 && sizeof(RibbitPrimerParams) == 44, "14, 6 and 11 ints");
constexpr RibbitPrimer NO_PRIMER{-1, 0, 0, 0, 0, 0};

inline int check_primer_params(const RibbitPrimerParams *p) {
    if (!p) return fail(RIBBIT_E_ARG, "null argument");
    if (p->flank < 0 || p->flank > RIBBIT_PRIMER_MAX_FLANK) return fail(RIBBIT_E_ARG, "flank %d is outside 0 .. %d", (int)p->flank, RIBBIT_PRIMER_MAX_FLANK);
    if (p->max_length > RIBBIT_PRIMER_MAX_LENGTH) return fail(RIBBIT_E_ARG, "max_length %d is above %d", (int)p->max_length, RIBBIT_PRIMER_MAX_LENGTH);
    if (p->min_length < 2 || p->min_length > p->max_length) return fail(RIBBIT_E_ARG, "min_length %d is outside 2 .. max_length %d", (int)p->min_length, (int)p->max_length);
    if (p->opt_length < p->min_length || p->opt_length > p->max_length)
        return fail(RIBBIT_E_ARG, "opt_length %d is outside min_length %d .. max_length %d", (int)p->opt_length, (int)p->min_length, (int)p->max_length);
    if (p->tm_max > 2000) return fail(RIBBIT_E_ARG, "tm_max %d is above 2000", (int)p->tm_max);
    if (p->tm_opt > p->tm_max) return fail(RIBBIT_E_ARG, "tm_opt %d is above tm_max %d", (int)p->tm_opt, (int)p->tm_max);
    if (p->tm_min < 0 || p->tm_min > p->tm_opt) return fail(RIBBIT_E_ARG, "tm_min %d is outside 0 .. tm_opt %d", (int)p->tm_min, (int)p->tm_opt);
    if (p->gc_max_percent > 100) return fail(RIBBIT_E_ARG, "gc_max_percent %d is above 100", (int)p->gc_max_percent);
    if (p->gc_min_percent < 0 || p->gc_min_percent > p->gc_max_percent)
        return fail(RIBBIT_E_ARG, "gc_min_percent %d is outside 0 .. gc_max_percent %d", (int)p->gc_min_percent, (int)p->gc_max_percent);
    if (p->max_run < 1) return fail(RIBBIT_E_ARG, "max_run %d is below 1", (int)p->max_run);
    if (p->gc_clamp != 0 && p->gc_clamp != 1) return fail(RIBBIT_E_ARG, "gc_clamp %d is neither 0 nor 1", (int)p->gc_clamp);
    return RIBBIT_OK;
}

inline int check_primer_args(const int32_t *intervals, size_t n, const int32_t *targets, size_t n_targets, const RibbitPrimerParams *params, const void *rows) {
    if ((!intervals && n > 0) || (!targets && n_targets > 0) || !rows) return fail(RIBBIT_E_ARG, "null argument");
    if (n > MAX_TARGETS) return fail(RIBBIT_E_ARG, "%zu intervals", n);
    if (n_targets > MAX_TARGETS) return fail(RIBBIT_E_ARG, "%zu targets", n_targets);
    return check_primer_params(params);
}

// a host twin's record
inline int check_sequence(const char *sequence, int64_t length) {
    if (length < 0 || length > (int64_t)INT32_MAX) return fail(RIBBIT_E_ARG, "a record of %lld bases", (long long)length);
    if (!sequence && length > 0) return fail(RIBBIT_E_ARG, "bad sequence");
    return RIBBIT_OK;
}

// the sum of two counts of different records, which stays at the largest int
inline int32_t saturating_sum(int32_t a, int32_t b) { return (int32_t)std::min<int64_t>((int64_t)a + b, INT32_MAX); }

inline bool has_pair(const RibbitRowPrimerPair &r) { return r.left.start >= 0; }

// a target's two windows: the left candidates lie in [lo, s), the right ones in [e, hi)
struct Flanks { int64_t lo, s, e, hi; };
inline Flanks flanks_of(const int32_t *targets, size_t i, int32_t flank, int64_t length) {
    const int64_t s = std::min(std::max<int64_t>(targets[2 * i], 0), length), e = std::min(std::max<int64_t>(targets[2 * i + 1], s), length);
    return Flanks{std::max<int64_t>(s - flank, 0), s, e, std::min<int64_t>(e + flank, length)};
}

// ---- one candidate from the bytes themselves
inline int code_of(unsigned char b) {      // A 0, C 1, G 2, T 3 in either case, -1 for every other byte
    switch (b | 0x20) {
        case 'a': return 0;
        case 'c': return 1;
        case 'g': return 2;
        case 't': return 3;
        default: return -1;
    }
}

inline char letter_at(const unsigned char *seq, int64_t p) {      // the base there in upper case, or 0 for a byte of kind `other`
    const int c = code_of(seq[p]);
    return c < 0 ? 0 : "ACGT"[c];
}
inline std::string reverse_complement(const std::string &o) {      // of letters over ACGT
    std::string q;
    for (size_t j = o.size(); j-- > 0;) q += o[j] == 'A' ? 'T' : o[j] == 'C' ? 'G' : o[j] == 'G' ? 'C' : 'A';
    return q;
}

// SantaLucia 1998 as the contract tabulates it: dH in 100 cal/mol, dS in 0.1 cal/(K mol), by the step's two letters
struct Step { char a, b; int32_t h, s; };
constexpr Step kSteps[16] = {{'A', 'A', -79, -222}, {'T', 'T', -79, -222}, {'A', 'T', -72, -204}, {'T', 'A', -72, -213}, {'C', 'A', -85, -227}, {'T', 'G', -85, -227},
                             {'G', 'T', -84, -224}, {'A', 'C', -84, -224}, {'C', 'T', -78, -210}, {'A', 'G', -78, -210}, {'G', 'A', -82, -222}, {'T', 'C', -82, -222},
                             {'C', 'G', -106, -272}, {'G', 'C', -98, -244}, {'G', 'G', -80, -199}, {'C', 'C', -80, -199}};
inline const Step &step_of(int a, int b) {
    for (const Step &st : kSteps)
        if (st.a == "ACGT"[a] && st.b == "ACGT"[b]) return st;
    return kSteps[0];      // (not reached: the sixteen pairs are all there)
}

struct Candidate { bool ok; int32_t tm; };
// [p, p + k) of the sequence, whose 3' base is the one at `three`
inline Candidate candidate(const unsigned char *seq, const std::vector<uint8_t> &covered, int64_t p, int32_t k, int64_t three, const RibbitPrimerParams &prm) {
    int32_t gc = 0, run = 0, h = 0, s = 0;
    for (int64_t q = p; q < p + k; ++q) {
        const int c = code_of(seq[q]);
        if (c < 0 || covered[(size_t)q]) return {false, 0};
        gc += c == 1 || c == 2;
        run = q > p && c == code_of(seq[q - 1]) ? run + 1 : 1;
        if (run > prm.max_run) return {false, 0};
        if (q > p) {
            const Step &st = step_of(code_of(seq[q - 1]), c);
            h += st.h;
            s += st.s;
        }
        if (q == p || q == p + k - 1) {
            h += c == 1 || c == 2 ? 1 : 23;
            s += c == 1 || c == 2 ? -28 : 41;
        }
    }
    if (100 * gc < prm.gc_min_percent * k || 100 * gc > prm.gc_max_percent * k) return {false, 0};
    const int c3 = code_of(seq[three]);
    if (prm.gc_clamp && c3 != 1 && c3 != 2) return {false, 0};
    s += -11 * (k - 1) - 362;
    const int32_t tm = (int32_t)((10000 * (int64_t)h) / s) - 2732;      // (both negative: the quotient is positive, and / truncates)
    return {tm >= prm.tm_min && tm <= prm.tm_max, tm};
}

// ---- the text
inline void put_tenths(std::string &out, int32_t v) {
    if (v < 0) out += '-';
    const int64_t a = v < 0 ? -(int64_t)v : v;
    put_number(out, a / 10);
    out += '.';
    out += (char)('0' + a % 10);
}

// start, end, sequence 5' to 3' and Tm of one side, or four dots
inline void put_primer(std::string &out, const RibbitPrimer &p, bool reverse) {
    if (p.start < 0) { out += "\t.\t.\t.\t."; return; }
    const uint64_t bases = (uint64_t)(uint32_t)p.bases_hi << 32 | (uint32_t)p.bases_lo;
    out += '\t';
    put_number(out, p.start);
    out += '\t';
    put_number(out, (int64_t)p.start + p.length);
    out += '\t';
    for (int32_t j = 0; j < p.length; ++j) out += reverse ? "TGCA"[(bases >> (2 * (p.length - 1 - j))) & 3] : "ACGT"[(bases >> (2 * j)) & 3];
    out += '\t';
    put_tenths(out, p.tm);
}

// the 21 columns of a row's primer pair, each behind a tab (ribbit_bed_primer_pairs_text, and ribbit_bed_primer_products_text
// before its own six); bad_primer: the primer whose length the text refuses, or null
inline const RibbitPrimer *bad_primer(const RibbitRowPrimerPair &r) {
    if (r.left.start >= 0 && r.right.start >= 0)
        for (const RibbitPrimer *p : {&r.left, &r.right})
            if (p->length < 1 || p->length > RIBBIT_PRIMER_MAX_LENGTH) return p;
    return nullptr;
}
inline void put_pair_columns(std::string &out, const RibbitRowPrimerPair &r) {
    if (r.left.start >= 0 && r.right.start >= 0) {
        put_primer(out, r.left, false);
        put_primer(out, r.right, true);
        out += '\t';
        put_number(out, r.product);
        out += '\t';
        put_tenths(out, r.tm_difference);
        for (const int32_t v : {r.pair_any, r.pair_end, r.left_self_any, r.left_self_end, r.left_hairpin, r.right_self_any, r.right_self_end, r.right_hairpin}) {
            out += '\t';
            put_number(out, v);
        }
    } else {
        for (int c = 0; c < 18; ++c) out += "\t.";
    }
    for (const int32_t v : {r.left_passed, r.right_passed, r.pairs_admissible}) {
        out += '\t';
        put_number(out, v);
    }
}

// the six columns of a pair's products, each behind a tab (ribbit_bed_primer_products_text, and ribbit_bed_primer_specific_text
// before its own four): the four counts, products - own and the shortest other product; dots in the last two when a list is
// longer than max_sites, in all six without a pair
inline void put_product_columns(std::string &out, const RibbitRowPrimerPair &r, const RibbitRowProducts &p) {
    if (r.left.start < 0) {
        for (int c = 0; c < 6; ++c) out += "\t.";
        return;
    }
    for (const int32_t v : {p.left_forward, p.left_reverse, p.right_forward, p.right_reverse}) {
        out += '\t';
        put_number(out, v);
    }
    if (p.products < 0) {
        out += "\t.\t.";
    } else {
        out += '\t';
        put_number(out, p.products - p.own);
        out += '\t';
        put_number(out, p.shortest_other);
    }
}

// The text of n rows' primer pairs (ribbit_bed_primer_pairs_text, ribbit_bed_primer_products_text, ribbit_bed_primer_specific_text):
// every line of the BED text, the 21 columns of its pair, and what columns(out, i) puts behind them.  reserve: what a row's columns
// take at most; what: the text's name in the message of a piece that runs out of memory.  The callers have checked for null.
template <typename Columns>
int bed_pair_rows_text(const char *bed, size_t bed_len, const RibbitRowPrimerPair *pairs, size_t n, const char *what, size_t reserve, char **text, size_t *len,
                       Columns columns) {
    const size_t parts = bed_text_parts(bed_len);
    BedLines lines;
    if (const int rc = lines.find(bed, bed_len, parts)) return rc;
    if (lines.count() != n) return fail(RIBBIT_E_ARG, "the BED text has %zu lines, not the %zu of the rows", lines.count(), n);
    return write_pieces(
        parts, what, text, len,
        [&](size_t k, std::string &out) {
            const size_t from = n * k / parts, to = n * (k + 1) / parts;
            out.reserve(lines.start[to] - lines.start[from] + reserve * (to - from));
            for (size_t i = from; i < to; ++i) {
                if (const RibbitPrimer *bad = bad_primer(pairs[i])) return PieceRefusal{1, i, (size_t)(uint32_t)bad->length};      // (the only refusal)
                put_field(out, lines[i]);
                put_pair_columns(out, pairs[i]);
                columns(out, i);
                out += '\n';
            }
            return PieceRefusal{};
        },
        [](const PieceRefusal &bad) { return fail(RIBBIT_E_ARG, "row %zu: a primer of %d bases, not 1 .. %d", bad.a, (int)(int32_t)(uint32_t)bad.b, RIBBIT_PRIMER_MAX_LENGTH); });
}

// ---- the host code of one twin that another twin calls; each is defined in the file named
// api_primer_pairs.cpp: the check of RibbitPrimerPairParams; the rows' coverage, a byte per position; every admissible pair of a
// target's two shortlists as the record the choice would fill for it, in the order of the choice, and the record of a target without a
// pair; a target's two shortlists as they leave the record; the held places of one side of stored shortlists (those before the first
// empty one); a stored primer's oligo as letters, 5' to 3' (the right one as ordered); the admissible pairs of stored shortlists from
// the lists alone, as host_ordered_pairs gives them from the sequence
int check_primer_pair_params(const RibbitPrimerPairParams *p);
void host_duplex(const std::string &a, const std::string &b, int32_t &any, int32_t &end);      // (the duplex behind ribbit_host_oligo_duplex, of letters over ACGT)
std::vector<uint8_t> host_covered(int64_t length, const int32_t *intervals, size_t n);
void host_ordered_pairs(const unsigned char *seq, const std::vector<uint8_t> &covered, const Flanks &f, const RibbitPrimerParams &prm, const RibbitPrimerPairParams &pair,
                        std::vector<RibbitRowPrimerPair> &ordered, RibbitRowPrimerPair &none);
void host_target_shortlists(const unsigned char *seq, const std::vector<uint8_t> &covered, const Flanks &f, const RibbitPrimerParams &prm, const RibbitPrimerPairParams &pair,
                            RibbitTargetShortlists &out);
int host_held_places(const RibbitPrimer *side);
std::string host_listed_oligo(const RibbitPrimer &p, bool right);
void host_listed_pairs(const RibbitTargetShortlists &lists, const RibbitPrimerPairParams &pair, std::vector<RibbitRowPrimerPair> &ordered, RibbitRowPrimerPair &none);
// api_primer_products.cpp: the check of RibbitProductParams, and of a call's pairs and parameters, with their wording; a pair's two
// oligos as the device takes them, and as letters, 5' to 3'; the sites of an oligo on either strand, ascending; the products of a
// pair among the sites of its two oligos
struct HostSites { std::vector<int32_t> forward, reverse; };
int check_primer_product_params(const RibbitProductParams *p);
int check_product_pairs(const RibbitRowPrimerPair *pairs, size_t n, const RibbitProductParams *params);
void pair_oligos(const RibbitRowPrimerPair &pair, RibbitOligo &a, RibbitOligo &b);
void host_pair_oligos(const RibbitRowPrimerPair &pair, std::string &a, std::string &b);
HostSites host_oligo_sites(const unsigned char *seq, int64_t length, const std::string &oligo, const RibbitProductParams &prm);
RibbitRowProducts host_products_among(const HostSites &a, const HostSites &b, int32_t ka, int32_t kb, int32_t left_start, int32_t right_start, const RibbitProductParams &prm);
// ... and the oligos of a twin whose pairs share them, every distinct one searched once: add() gives an oligo's id, search() finds
// the sites of all that were added on the host thread team, sites() are those of an id
class HostOligoIndex {
public:
    size_t add(const std::string &oligo);
    void search(const unsigned char *seq, int64_t length, const RibbitProductParams &prm);
    const HostSites &sites(size_t id) const { return found[id]; }

private:
    std::map<std::string, size_t> ids;
    std::vector<const std::string *> distinct;      // (a map's keys stay where they are)
    std::vector<HostSites> found;
};

}  // namespace rbapi
