// api_primer_pairs.cpp -- the two primers of every target of a record chosen as one pair, each checked for self-dimers and
// hairpins and the pair for cross-dimers (primer_pairs.hip); see api_internal.h for the map of the files behind
// include/ribbit_hip.h.  The GPU form is ribbit_hip_record_primers' in every step but the kernel: the bit planes the load packed,
// the coverage bitmap of the record's rows (build_coverage: nothing is enqueued for it when the bitmap is that of these rows
// already), the targets through stage_down, the handle's stream, nothing kept between calls.  The host twin works from the bytes of
// the sequence: every candidate judged letter by letter (primers_host.h), every oligo as a string of letters, every placement of
// two oligos walked pair by pair.  It has no packed words and shares nothing with the kernel but the Tm table.  The two oligo
// functions are the twin's own loops, handed out; the text needs no GPU.
#include "primers_host.h"

#include <string>
#include <tuple>

namespace {

static_assert(sizeof(RibbitRowPrimerPair) == 128 && sizeof(RibbitPrimerPairParams) == 28, "32 and 7 ints");
constexpr int32_t MAX_LIMIT = 32, MAX_TM_DIFFERENCE = 2000;

}  // namespace

int rbapi::check_primer_pair_params(const RibbitPrimerPairParams *p) {
    if (!p) return fail(RIBBIT_E_ARG, "null argument");
    if (p->shortlist < 1 || p->shortlist > RIBBIT_PRIMER_PAIR_SHORTLIST) return fail(RIBBIT_E_ARG, "shortlist %d is outside 1 .. %d", (int)p->shortlist, RIBBIT_PRIMER_PAIR_SHORTLIST);
    const struct { const char *name; int32_t value; } limits[] = {{"max_self_any", p->max_self_any}, {"max_self_end", p->max_self_end}, {"max_hairpin", p->max_hairpin},
                                                                   {"max_pair_any", p->max_pair_any}, {"max_pair_end", p->max_pair_end}};
    for (const auto &l : limits)
        if (l.value < 0 || l.value > MAX_LIMIT) return fail(RIBBIT_E_ARG, "%s %d is outside 0 .. %d", l.name, (int)l.value, (int)MAX_LIMIT);
    if (p->max_tm_difference < 0 || p->max_tm_difference > MAX_TM_DIFFERENCE)
        return fail(RIBBIT_E_ARG, "max_tm_difference %d is outside 0 .. %d", (int)p->max_tm_difference, (int)MAX_TM_DIFFERENCE);
    return RIBBIT_OK;
}

namespace {

int check_args(const int32_t *intervals, size_t n, const int32_t *targets, size_t n_targets, const RibbitPrimerParams *params, const RibbitPrimerPairParams *pair,
               const void *rows) {
    if (const int rc = check_primer_args(intervals, n, targets, n_targets, params, rows)) return rc;
    return check_primer_pair_params(pair);
}

// a target without a pair: the six counts stay
RibbitRowPrimerPair no_pair(int32_t left_candidates, int32_t right_candidates, int32_t left_passed, int32_t right_passed, int32_t tried) {
    RibbitRowPrimerPair r{};
    r.left = r.right = NO_PRIMER;
    r.left_candidates = left_candidates;
    r.right_candidates = right_candidates;
    r.left_passed = left_passed;
    r.right_passed = right_passed;
    r.pairs_tried = tried;
    return r;
}

int record_primer_pairs_impl(RibbitHandle *h, const int32_t *intervals, size_t n, const int32_t *targets, size_t n_targets, const RibbitPrimerParams *params,
                             const RibbitPrimerPairParams *pair, const RibbitRowPrimerPair **rows) {
    if (!h) return fail(RIBBIT_E_ARG, "null handle");
    int rc;
    if ((rc = check_args(intervals, n, targets, n_targets, params, pair, rows))) return rc;
    if (!h->loaded) return fail(RIBBIT_E_STATE, "no record loaded");
    RibbitHandle::RowBufs &buf = h->rows;
    if ((rc = buf.h_primer_pairs.ensure(std::max<size_t>(n_targets, 1), true))) return rc;
    *rows = buf.h_primer_pairs.p;
    if (n_targets == 0) return RIBBIT_OK;
    const int64_t length = h->length;
    if (length == 0) {      // (every flank is empty)
        std::fill(buf.h_primer_pairs.p, buf.h_primer_pairs.p + n_targets, no_pair(0, 0, 0, 0, 0));
        return RIBBIT_OK;
    }
    if ((rc = bind_device(h))) return rc;
    const rb::PrimerPairLayout at = rb::primer_pairs_layout((int64_t)n_targets);
    if ((rc = buf.d_work.ensure(at.bytes, true))) return rc;
    const StageSegment down{targets, 2 * n_targets * sizeof(int32_t)};
    const uint8_t *d_targets = nullptr;
    if ((rc = stage_down(h, &down, 1, &d_targets))) return rc;
    if ((rc = build_coverage(h, intervals, n))) return rc;
    HIP_TRY(rb::launch_primer_pairs(h->planes(), buf.d_mask_bits.p, reinterpret_cast<const int32_t *>(d_targets), (int64_t)n_targets, *params, *pair, buf.d_work.p,
                                    buf.d_work.cap, at, h->stream));
    HIP_TRY(hipMemcpyAsync(buf.h_primer_pairs.p, buf.d_work.p + at.out, n_targets * sizeof(RibbitRowPrimerPair), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    for (size_t i = 0; i < n_targets; ++i) {
        const RibbitRowPrimerPair &r = buf.h_primer_pairs.p[i];
        const Flanks f = flanks_of(targets, i, params->flank, length);
        const auto inside = [&](const RibbitPrimer &p, int64_t from, int64_t to) {
            return p.length >= params->min_length && p.length <= params->max_length && p.start >= from && (int64_t)p.start + p.length <= to;
        };
        const bool none = r.left.start == -1 && r.right.start == -1 && r.left.length == 0 && r.right.length == 0 && r.pairs_admissible == 0;
        const bool both = r.left.start >= 0 && r.right.start >= 0 && inside(r.left, f.lo, f.s) && inside(r.right, f.e, f.hi) && r.pairs_admissible >= 1;
        if (!(none || both) || r.left_passed > r.left_candidates || r.right_passed > r.right_candidates || r.pairs_admissible > r.pairs_tried)
            return fail(RIBBIT_E_INTERNAL, "target %zu: a primer pair the GPU found lies outside its flanks", i);
    }
    return RIBBIT_OK;
}

// ---- the duplex and the hairpin, in letters
bool bonded(char x, char y) { return (x == 'A' && y == 'T') || (x == 'T' && y == 'A') || (x == 'C' && y == 'G') || (x == 'G' && y == 'C'); }

struct Duplex { int32_t any, end; };
// a and b over ACGT, 5' to 3'
Duplex duplex(const std::string &a, const std::string &b) {
    const int ka = (int)a.size(), kb = (int)b.size();
    Duplex out{0, 0};
    for (int c = 0; c <= ka + kb - 2; ++c) {
        // the maximal runs of bonded pairs (i, c - i) along i
        int i = std::max(0, c - (kb - 1));
        const int last = std::min(ka - 1, c);
        while (i <= last) {
            if (!bonded(a[(size_t)i], b[(size_t)(c - i)])) { ++i; continue; }
            const int from = i;
            while (i <= last && bonded(a[(size_t)i], b[(size_t)(c - i)])) ++i;
            const int run = i - from;      // the pairs from .. i - 1
            out.any = std::max(out.any, run);
            const bool holds_a3 = i - 1 == ka - 1, holds_b3 = c - from == kb - 1;
            if (holds_a3 || holds_b3) out.end = std::max(out.end, run);
        }
    }
    return out;
}

}  // namespace

void rbapi::host_duplex(const std::string &a, const std::string &b, int32_t &any, int32_t &end) {
    const Duplex d = duplex(a, b);
    any = d.any;
    end = d.end;
}

namespace {

int32_t hairpin(const std::string &a) {
    const int k = (int)a.size();
    int32_t best = 0;
    for (int c = 0; c <= 2 * k - 2; ++c) {
        int run = 0;
        for (int i = std::max(0, c - (k - 1)); i <= std::min(k - 1, c); ++i) {
            const int j = c - i;
            const bool counts = i < j && j - i - 1 >= RIBBIT_PRIMER_HAIRPIN_LOOP && bonded(a[(size_t)i], a[(size_t)j]);
            run = counts ? run + 1 : 0;
            best = std::max(best, run);
        }
    }
    return best;
}

// the letters of an oligo given as text, upper case; false when it is not 1 .. 32 of ACGTacgt
bool oligo_letters(const char *text, std::string &out) {
    out.clear();
    if (!text) return false;
    for (const char *p = text; *p; ++p) {
        const int c = code_of((unsigned char)*p);
        if (c < 0 || out.size() == (size_t)RIBBIT_PRIMER_MAX_LENGTH) return false;
        out += "ACGT"[c];
    }
    return !out.empty();
}

// ---- host twin
struct Listed {
    int32_t penalty, k, tm;
    int64_t distance, p;
    std::string oligo;      // 5' to 3': the left candidate's letters, the right candidate's reverse complement
    Duplex self;
    int32_t hairpin;
    std::tuple<int32_t, int64_t, int32_t> key() const { return std::make_tuple(penalty, distance, k); }
};

std::string oligo_of(const unsigned char *seq, int64_t p, int32_t k, bool right) {
    std::string o;
    for (int32_t j = 0; j < k; ++j) {
        const int c = code_of(seq[right ? p + k - 1 - j : p + j]);
        o += right ? "TGCA"[c] : "ACGT"[c];
    }
    return o;
}

// the passing candidates of the window [from, to), the best `shortlist` of them in order; -> admissible and passing candidates
void side(const unsigned char *seq, const std::vector<uint8_t> &covered, int64_t from, int64_t to, bool right, const RibbitPrimerParams &prm, const RibbitPrimerPairParams &pair,
          std::vector<Listed> &list, int32_t &found, int32_t &passed) {
    list.clear();
    found = passed = 0;
    for (int64_t p = from; p < to; ++p)
        for (int32_t k = prm.min_length; k <= prm.max_length && p + k <= to; ++k) {
            const Candidate c = candidate(seq, covered, p, k, right ? p : p + k - 1, prm);
            if (!c.ok) continue;
            ++found;
            Listed it{std::abs(c.tm - prm.tm_opt) + 10 * std::abs(k - prm.opt_length), k, c.tm, right ? p - from : to - (p + k), p, oligo_of(seq, p, k, right), {0, 0}, 0};
            it.self = duplex(it.oligo, it.oligo);
            it.hairpin = hairpin(it.oligo);
            if (it.self.any > pair.max_self_any || it.self.end > pair.max_self_end || it.hairpin > pair.max_hairpin) continue;
            ++passed;
            // keep the list sorted and no longer than the shortlist
            auto at = list.begin();
            while (at != list.end() && at->key() < it.key()) ++at;
            list.insert(at, std::move(it));
            if (list.size() > (size_t)pair.shortlist) list.pop_back();
        }
}

RibbitPrimer primer_of(const unsigned char *seq, const Listed &it) {
    uint64_t bases = 0;
    for (int32_t j = 0; j < it.k; ++j) bases |= (uint64_t)code_of(seq[it.p + j]) << (2 * j);
    return RibbitPrimer{(int32_t)it.p, it.k, it.tm, it.penalty, (int32_t)(uint32_t)bases, (int32_t)(uint32_t)(bases >> 32)};
}

// every admissible pair of two shortlists, whose primers as records are lp and rp, each as the record the choice would fill for it,
// in the order of step (4); none: the record of a target without a pair (the six counts; pairs_admissible is the others' too)
void pairs_among(const std::vector<Listed> &left, const std::vector<Listed> &right, const std::vector<RibbitPrimer> &lp, const std::vector<RibbitPrimer> &rp,
                 const RibbitPrimerPairParams &pair, std::vector<RibbitRowPrimerPair> &ordered, RibbitRowPrimerPair &none) {
    ordered.clear();
    for (int32_t l = 0; l < (int32_t)left.size(); ++l)
        for (int32_t r = 0; r < (int32_t)right.size(); ++r) {
            const Listed &a = left[(size_t)l], &b = right[(size_t)r];
            const int32_t difference = std::abs(a.tm - b.tm);
            if (difference > pair.max_tm_difference) continue;
            const Duplex d = duplex(a.oligo, b.oligo);
            if (d.any > pair.max_pair_any || d.end > pair.max_pair_end) continue;
            RibbitRowPrimerPair out = none;
            out.left = lp[(size_t)l];
            out.right = rp[(size_t)r];
            out.pair_penalty = a.penalty + b.penalty + difference;
            out.tm_difference = difference;
            out.product = (int32_t)(b.p + b.k - a.p);
            out.left_rank = l;
            out.right_rank = r;
            out.left_self_any = a.self.any;
            out.left_self_end = a.self.end;
            out.left_hairpin = a.hairpin;
            out.right_self_any = b.self.any;
            out.right_self_end = b.self.end;
            out.right_hairpin = b.hairpin;
            out.pair_any = d.any;
            out.pair_end = d.end;
            ordered.push_back(out);
        }
    const auto key = [](const RibbitRowPrimerPair &r) { return std::make_tuple(r.pair_penalty, r.product, r.left_rank, r.right_rank); };
    std::sort(ordered.begin(), ordered.end(), [&](const RibbitRowPrimerPair &x, const RibbitRowPrimerPair &y) { return key(x) < key(y); });
    none.pairs_admissible = (int32_t)ordered.size();
    for (RibbitRowPrimerPair &r : ordered) r.pairs_admissible = none.pairs_admissible;
}

struct Shortlists {
    std::vector<Listed> left, right;
    std::vector<RibbitPrimer> lp, rp;
    RibbitRowPrimerPair none;
};

// a target's two shortlists from the bytes of the sequence
void shortlists_of(const unsigned char *seq, const std::vector<uint8_t> &covered, const Flanks &f, const RibbitPrimerParams &prm, const RibbitPrimerPairParams &pair,
                   Shortlists &s) {
    int32_t n_left, n_right, p_left, p_right;
    side(seq, covered, f.lo, f.s, false, prm, pair, s.left, n_left, p_left);
    side(seq, covered, f.e, f.hi, true, prm, pair, s.right, n_right, p_right);
    s.none = no_pair(n_left, n_right, p_left, p_right, (int32_t)(s.left.size() * s.right.size()));
    s.lp.clear();
    s.rp.clear();
    for (const Listed &it : s.left) s.lp.push_back(primer_of(seq, it));
    for (const Listed &it : s.right) s.rp.push_back(primer_of(seq, it));
}

// a stored primer as the twin lists it: its oligo from its packed bases, the self values from the oligo's letters
Listed listed_of(const RibbitPrimer &p, bool right) {
    const uint64_t bases = (uint64_t)(uint32_t)p.bases_hi << 32 | (uint32_t)p.bases_lo;
    std::string o;
    for (int32_t j = 0; j < p.length; ++j) o += right ? "TGCA"[(bases >> (2 * (p.length - 1 - j))) & 3] : "ACGT"[(bases >> (2 * j)) & 3];
    Listed it{p.penalty, p.length, p.tm, 0, p.start, o, {0, 0}, 0};
    it.self = duplex(it.oligo, it.oligo);
    it.hairpin = hairpin(it.oligo);
    return it;
}

RibbitRowPrimerPair pair_of(const unsigned char *seq, const std::vector<uint8_t> &covered, const Flanks &f, const RibbitPrimerParams &prm, const RibbitPrimerPairParams &pair) {
    std::vector<RibbitRowPrimerPair> ordered;
    RibbitRowPrimerPair none;
    host_ordered_pairs(seq, covered, f, prm, pair, ordered, none);
    if (ordered.empty()) return none;
    return ordered.front();
}

int host_record_primer_pairs_impl(const char *sequence, int64_t length, const int32_t *intervals, size_t n, const int32_t *targets, size_t n_targets,
                                  const RibbitPrimerParams *params, const RibbitPrimerPairParams *pair, RibbitRowPrimerPair **rows) {
    int rc;
    if ((rc = check_args(intervals, n, targets, n_targets, params, pair, rows))) return rc;
    if ((rc = check_sequence(sequence, length))) return rc;
    const unsigned char *seq = reinterpret_cast<const unsigned char *>(sequence);
    const std::vector<uint8_t> covered = host_covered(length, intervals, n);
    Handed<RibbitRowPrimerPair> out;
    if ((rc = hand_out<RibbitRowPrimerPair>(nullptr, n_targets, false, out))) return rc;
    const RibbitPrimerParams prm = *params;
    const RibbitPrimerPairParams prs = *pair;
    const unsigned threads = (unsigned)std::max<size_t>(1, std::min<size_t>(rb::host_thread_count(0), n_targets / 4));
    rb::over_pieces(n_targets, threads, [&](size_t lo, size_t hi, unsigned) {
        for (size_t i = lo; i < hi; ++i) out[i] = pair_of(seq, covered, flanks_of(targets, i, prm.flank, length), prm, prs);
    });
    *rows = out.release();
    return RIBBIT_OK;
}

// ---- the text
int bed_primer_pairs_text_impl(const char *bed, size_t bed_len, const RibbitRowPrimerPair *rows, size_t n, char **text, size_t *len) {
    if (!text || !len || (!bed && bed_len > 0) || (!rows && n > 0)) return fail(RIBBIT_E_ARG, "null argument");
    return bed_pair_rows_text(bed, bed_len, rows, n, "the rows' primer pairs", 192, text, len, [](std::string &, size_t) {});
}

}  // namespace

// ---- what the twins of the specific pairs and of a genome's pairs take from here (primers_host.h)
namespace rbapi {

std::vector<uint8_t> host_covered(int64_t length, const int32_t *intervals, size_t n) {
    std::vector<uint8_t> covered((size_t)length, 0);
    const CoveredRuns runs(clipped_sorted_rows(length, intervals, n));
    for (size_t k = 0; k < runs.start.size(); ++k) std::fill(covered.begin() + runs.start[k], covered.begin() + runs.end[k], 1);
    return covered;
}

void host_ordered_pairs(const unsigned char *seq, const std::vector<uint8_t> &covered, const Flanks &f, const RibbitPrimerParams &prm, const RibbitPrimerPairParams &pair,
                        std::vector<RibbitRowPrimerPair> &ordered, RibbitRowPrimerPair &none) {
    Shortlists s;
    shortlists_of(seq, covered, f, prm, pair, s);
    none = s.none;
    pairs_among(s.left, s.right, s.lp, s.rp, pair, ordered, none);
}

void host_target_shortlists(const unsigned char *seq, const std::vector<uint8_t> &covered, const Flanks &f, const RibbitPrimerParams &prm, const RibbitPrimerPairParams &pair,
                            RibbitTargetShortlists &out) {
    Shortlists s;
    shortlists_of(seq, covered, f, prm, pair, s);
    for (size_t k = 0; k < (size_t)RIBBIT_PRIMER_PAIR_SHORTLIST; ++k) {
        out.left[k] = k < s.lp.size() ? s.lp[k] : NO_PRIMER;
        out.right[k] = k < s.rp.size() ? s.rp[k] : NO_PRIMER;
    }
    out.left_candidates = s.none.left_candidates;
    out.right_candidates = s.none.right_candidates;
    out.left_passed = s.none.left_passed;
    out.right_passed = s.none.right_passed;
}

int host_held_places(const RibbitPrimer *side) {
    int held = 0;
    while (held < RIBBIT_PRIMER_PAIR_SHORTLIST && side[held].start >= 0) ++held;
    return held;
}

std::string host_listed_oligo(const RibbitPrimer &p, bool right) { return listed_of(p, right).oligo; }

void host_listed_pairs(const RibbitTargetShortlists &lists, const RibbitPrimerPairParams &pair, std::vector<RibbitRowPrimerPair> &ordered, RibbitRowPrimerPair &none) {
    Shortlists s;
    const int n_left = host_held_places(lists.left), n_right = host_held_places(lists.right);
    for (int k = 0; k < n_left; ++k) {
        s.lp.push_back(lists.left[k]);
        s.left.push_back(listed_of(lists.left[k], false));
    }
    for (int k = 0; k < n_right; ++k) {
        s.rp.push_back(lists.right[k]);
        s.right.push_back(listed_of(lists.right[k], true));
    }
    none = no_pair(lists.left_candidates, lists.right_candidates, lists.left_passed, lists.right_passed, n_left * n_right);
    pairs_among(s.left, s.right, s.lp, s.rp, pair, ordered, none);
}

}  // namespace rbapi

extern "C" {

void ribbit_primer_pair_params_default(RibbitPrimerPairParams *params) {
    if (params) *params = RibbitPrimerPairParams{RIBBIT_PRIMER_PAIR_SHORTLIST, 4, 3, 3, 4, 3, 30};
}

int ribbit_hip_record_primer_pairs(RibbitHandle *h, const int32_t *intervals, size_t n, const int32_t *targets, size_t n_targets, const RibbitPrimerParams *params,
                                   const RibbitPrimerPairParams *pair_params, const RibbitRowPrimerPair **rows) {
    return guarded("the primer pairs", [&]() -> int { return record_primer_pairs_impl(h, intervals, n, targets, n_targets, params, pair_params, rows); });
}

int ribbit_host_record_primer_pairs(const char *sequence, int64_t length, const int32_t *intervals, size_t n, const int32_t *targets, size_t n_targets,
                                    const RibbitPrimerParams *params, const RibbitPrimerPairParams *pair_params, RibbitRowPrimerPair **rows) {
    return guarded("the primer pairs",
                   [&]() -> int { return host_record_primer_pairs_impl(sequence, length, intervals, n, targets, n_targets, params, pair_params, rows); });
}

void ribbit_primer_pairs_free(RibbitRowPrimerPair *rows) { std::free(rows); }

int ribbit_host_oligo_duplex(const char *a, const char *b, int32_t *any, int32_t *end) {
    return guarded("the duplex of two oligos", [&]() -> int {
        if (!any || !end) return fail(RIBBIT_E_ARG, "null argument");
        std::string la, lb;
        if (!oligo_letters(a, la) || !oligo_letters(b, lb)) return fail(RIBBIT_E_ARG, "an oligo is 1 .. %d letters of ACGTacgt", RIBBIT_PRIMER_MAX_LENGTH);
        const Duplex d = duplex(la, lb);
        *any = d.any;
        *end = d.end;
        return RIBBIT_OK;
    });
}

int ribbit_host_oligo_hairpin(const char *a, int32_t *out) {
    return guarded("the hairpin of an oligo", [&]() -> int {
        if (!out) return fail(RIBBIT_E_ARG, "null argument");
        std::string la;
        if (!oligo_letters(a, la)) return fail(RIBBIT_E_ARG, "an oligo is 1 .. %d letters of ACGTacgt", RIBBIT_PRIMER_MAX_LENGTH);
        *out = hairpin(la);
        return RIBBIT_OK;
    });
}

int ribbit_bed_primer_pairs_text(const char *bed_text, size_t bed_len, const RibbitRowPrimerPair *rows, size_t n, char **text, size_t *len) {
    return guarded("the rows' primer pairs as text", [&]() -> int { return bed_primer_pairs_text_impl(bed_text, bed_len, rows, n, text, len); });
}

}  // extern "C"
