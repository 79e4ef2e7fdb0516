// primer_pairs_host_check.cpp -- a stand-alone run of the host side of the primer pair output (ribbit_host_record_primer_pairs,
// ribbit_host_oligo_duplex, ribbit_host_oligo_hairpin, ribbit_bed_primer_pairs_text) for the sanitizers:
// `make -C ribbit_amd/csrc asan-primer-pairs-check` links it against the library's host code built with
// -fsanitize=address,undefined and runs it on the CPU.  It needs no GPU and prints "ok" when every pair lies in its flanks, spells
// the record's bases there, and has the values that the two oligo functions give for its oligos, within the limits.
#include <algorithm>
#include <cctype>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "ribbit_hip.h"

namespace {

[[noreturn]] void die(const char *what) {
    std::fprintf(stderr, "primer_pairs_host_check: %s: %s\n", what, ribbit_hip_last_error());
    std::exit(1);
}

[[noreturn]] void wrong(const char *what) {
    std::fprintf(stderr, "primer_pairs_host_check: %s\n", what);
    std::exit(1);
}

// the oligo of a primer, 5' to 3', checked against the record
std::string oligo_of(const std::string &seq, const RibbitPrimer &p, bool right) {
    const uint64_t bases = (uint64_t)(uint32_t)p.bases_hi << 32 | (uint32_t)p.bases_lo;
    std::string forward, out;
    for (int32_t j = 0; j < p.length; ++j) forward += "ACGT"[(bases >> (2 * j)) & 3];
    for (int32_t j = 0; j < p.length; ++j)
        if (std::toupper((unsigned char)seq[(size_t)p.start + j]) != forward[(size_t)j]) wrong("a primer that does not spell the record");
    if (!right) return forward;
    for (int32_t j = p.length - 1; j >= 0; --j) out += forward[(size_t)j] == 'A' ? 'T' : forward[(size_t)j] == 'C' ? 'G' : forward[(size_t)j] == 'G' ? 'C' : 'A';
    return out;
}

size_t check_row(const std::string &seq, const RibbitRowPrimerPair &r, int64_t lo, int64_t s, int64_t e, int64_t hi, const RibbitPrimerParams &prm, const RibbitPrimerPairParams &pair) {
    if (r.reserved || r.left_passed > r.left_candidates || r.right_passed > r.right_candidates || r.pairs_admissible > r.pairs_tried ||
        r.pairs_tried != std::min(pair.shortlist, r.left_passed) * std::min(pair.shortlist, r.right_passed))
        wrong("counts that do not fit each other");
    if (r.left.start < 0 || r.right.start < 0) {
        RibbitRowPrimerPair zero{};
        zero.left.start = zero.right.start = -1;
        if (std::memcmp(&r, &zero, 25 * sizeof(int32_t)) != 0 || r.pairs_admissible) wrong("a missing pair with values");
        return 0;
    }
    for (const RibbitPrimer *p : {&r.left, &r.right})
        if (p->length < prm.min_length || p->length > prm.max_length) wrong("a primer of a wrong length");
    if (r.left.start < lo || (int64_t)r.left.start + r.left.length > s || r.right.start < e || (int64_t)r.right.start + r.right.length > hi) wrong("a primer outside its flank");
    const std::string a = oligo_of(seq, r.left, false), b = oligo_of(seq, r.right, true);
    int32_t any = 0, end = 0, stem = 0;
    if (ribbit_host_oligo_duplex(a.c_str(), b.c_str(), &any, &end) != RIBBIT_OK) die("ribbit_host_oligo_duplex");
    if (any != r.pair_any || end != r.pair_end || any > pair.max_pair_any || end > pair.max_pair_end) wrong("a pair with other duplex values");
    if (ribbit_host_oligo_duplex(b.c_str(), a.c_str(), &any, &end) != RIBBIT_OK || any != r.pair_any || end != r.pair_end) wrong("a duplex that is not symmetric");
    if (ribbit_host_oligo_duplex(a.c_str(), a.c_str(), &any, &end) != RIBBIT_OK || ribbit_host_oligo_hairpin(a.c_str(), &stem) != RIBBIT_OK) die("the left oligo");
    if (any != r.left_self_any || end != r.left_self_end || stem != r.left_hairpin || any > pair.max_self_any || end > pair.max_self_end || stem > pair.max_hairpin) wrong("a left primer with other self values");
    if (ribbit_host_oligo_duplex(b.c_str(), b.c_str(), &any, &end) != RIBBIT_OK || ribbit_host_oligo_hairpin(b.c_str(), &stem) != RIBBIT_OK) die("the right oligo");
    if (any != r.right_self_any || end != r.right_self_end || stem != r.right_hairpin || any > pair.max_self_any || end > pair.max_self_end || stem > pair.max_hairpin) wrong("a right primer with other self values");
    if (r.tm_difference != std::abs(r.left.tm - r.right.tm) || r.tm_difference > pair.max_tm_difference || r.pair_penalty != r.left.penalty + r.right.penalty + r.tm_difference ||
        r.product != r.right.start + r.right.length - r.left.start || r.left_rank >= pair.shortlist || r.right_rank >= pair.shortlist || r.pairs_admissible < 1)
        wrong("a pair whose sums do not fit");
    return 1;
}

}  // namespace

int main() {
    std::mt19937 rng(19);
    size_t found = 0, targets_seen = 0;
    RibbitPrimerParams small;
    ribbit_primer_params_default(&small);
    small.min_length = 5; small.max_length = 8; small.opt_length = 6; small.tm_min = 0; small.tm_opt = 150; small.tm_max = 400; small.gc_min_percent = 20; small.gc_max_percent = 80;
    for (const int64_t length : {0, 1, 64, 1000, 4000}) {
        std::string seq;
        for (int64_t i = 0; i < length; ++i) seq += "ACGTacgtACGTacgtACGTacgtNx"[rng() % 26];
        std::vector<int32_t> rows, targets;
        for (int i = 0; i < 10; ++i) {
            const int32_t s = (int32_t)(rng() % (uint32_t)(length + 7)) - 3;
            rows.push_back(s);
            rows.push_back(s + (int32_t)(rng() % 30) - 2);
        }
        for (int i = 0; i < 60; ++i) {
            const int32_t s = (int32_t)(rng() % (uint32_t)(length + 7)) - 3;
            targets.push_back(s);
            targets.push_back(s + (int32_t)(rng() % 40) - 2);
        }
        targets.insert(targets.end(), {INT32_MIN, INT32_MAX, INT32_MAX, INT32_MIN, 0, (int32_t)length, (int32_t)length, (int32_t)length, 0, 0});
        for (const int32_t flank : {0, 17, 200, 1000})
            for (const int variant : {0, 1, 2}) {
                RibbitPrimerParams prm = small;
                RibbitPrimerPairParams pair;
                ribbit_primer_pair_params_default(&pair);
                if (variant == 0) ribbit_primer_params_default(&prm);
                if (variant == 1) pair = RibbitPrimerPairParams{3, 3, 2, 2, 3, 2, 60};
                if (variant == 2) pair = RibbitPrimerPairParams{1, 32, 32, 32, 32, 32, 2000};
                prm.flank = flank;
                RibbitRowPrimerPair *out = nullptr;
                if (ribbit_host_record_primer_pairs(seq.data(), length, rows.data(), rows.size() / 2, targets.data(), targets.size() / 2, &prm, &pair, &out) != RIBBIT_OK)
                    die("ribbit_host_record_primer_pairs");
                for (size_t i = 0; i < targets.size() / 2; ++i) {
                    const int64_t s = std::min(std::max<int64_t>(targets[2 * i], 0), length), e = std::min(std::max<int64_t>(targets[2 * i + 1], s), length);
                    found += check_row(seq, out[i], std::max<int64_t>(s - flank, 0), s, e, std::min<int64_t>(e + flank, length), prm, pair);
                    ++targets_seen;
                }
                ribbit_primer_pairs_free(out);
            }
    }
    if (found < 100) { std::fprintf(stderr, "only %zu pairs\n", found); return 1; }
    // the pinned values, and oligos that are refused
    int32_t any = 0, end = 0, stem = 0;
    if (ribbit_host_oligo_duplex("GATTACAGATTACAGGC", "TTTGCCTGTAATC", &any, &end) != RIBBIT_OK || any != 10 || end != 10) wrong("the duplex of the contract's two oligos");
    if (ribbit_host_oligo_hairpin("CCCCCAAAGGGGG", &stem) != RIBBIT_OK || stem != 5) wrong("the hairpin of the contract's oligo");
    const std::string longest(32, 'g'), too_long(33, 'g');
    if (ribbit_host_oligo_duplex(longest.c_str(), longest.c_str(), &any, &end) != RIBBIT_OK || any != 0) wrong("32 letters");
    if (ribbit_host_oligo_duplex(too_long.c_str(), "ACGT", &any, &end) != RIBBIT_E_ARG || ribbit_host_oligo_hairpin("", &stem) != RIBBIT_E_ARG ||
        ribbit_host_oligo_hairpin("ACGN", &stem) != RIBBIT_E_ARG || ribbit_host_oligo_duplex(nullptr, "ACGT", &any, &end) != RIBBIT_E_ARG)
        wrong("an oligo that should have been refused");
    // enough rows for the BED text to be cut into pieces (4 MB each), and the refusals
    const size_t n = 150000;
    std::string bed;
    std::vector<RibbitRowPrimerPair> rows(n);
    for (size_t i = 0; i < n; ++i) {
        bed += "rec\twith a tab\t" + std::to_string(i) + "\t" + std::to_string(i + 9) + "\tCA\t2|2\t9\t4.5\t0.9\t+\tP\t9=\n";
        RibbitRowPrimerPair &r = rows[i];
        int32_t *fields = reinterpret_cast<int32_t *>(&r);
        for (int j = 12; j < 32; ++j) fields[j] = (int32_t)(rng() >> 1);
        r.left = RibbitPrimer{i % 3 ? (int32_t)i : -1, 1 + (int32_t)(rng() % 32), (int32_t)(rng() % 2001), 0, (int32_t)rng(), (int32_t)rng()};
        r.right = RibbitPrimer{i % 5 ? INT32_MAX - 32 : -1, 1 + (int32_t)(rng() % 32), -(int32_t)(rng() % 2001), 0, (int32_t)rng(), (int32_t)rng()};
    }
    bed.pop_back();      // (a last line without its newline)
    char *text = nullptr, *none = nullptr;
    size_t len = 0;
    if (ribbit_bed_primer_pairs_text(bed.data(), bed.size(), rows.data(), n, &text, &len) != RIBBIT_OK) die("ribbit_bed_primer_pairs_text");
    if ((size_t)std::count(text, text + len, '\n') != n || (size_t)std::count(text, text + len, '\t') != 32 * n) wrong("the text has the wrong shape");
    ribbit_text_free(text);
    rows[n - 1].left = RibbitPrimer{5, 33, 0, 0, 0, 0};
    rows[n - 1].right.start = 7;
    if (ribbit_bed_primer_pairs_text(bed.data(), bed.size(), rows.data(), n, &none, &len) != RIBBIT_E_ARG) die("a primer of 33 bases was taken");
    if (ribbit_bed_primer_pairs_text(bed.data(), bed.size() / 2, rows.data(), n, &none, &len) != RIBBIT_E_ARG) die("half a BED text was taken");
    RibbitPrimerParams prm;
    ribbit_primer_params_default(&prm);
    RibbitPrimerPairParams bad;
    ribbit_primer_pair_params_default(&bad);
    bad.shortlist = RIBBIT_PRIMER_PAIR_SHORTLIST + 1;
    RibbitRowPrimerPair *out = nullptr;
    if (ribbit_host_record_primer_pairs("ACGT", 4, nullptr, 0, nullptr, 0, &prm, &bad, &out) != RIBBIT_E_ARG) die("a shortlist of 9 was taken");
    std::printf("ok: %zu pairs for %zu targets, %zu rows as text\n", found, targets_seen, n);
    return 0;
}
