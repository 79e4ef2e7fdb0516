// primers_host_check.cpp -- a stand-alone run of the host side of the primer output (ribbit_host_record_primers,
// ribbit_bed_primers_text) for the sanitizers: `make -C ribbit_amd/csrc asan-primers-check` links it against the library's host code
// built with -fsanitize=address,undefined and runs it on the CPU.  It needs no GPU and prints "ok" when every primer lies in its
// flank, spells the record's bases there and melts as a second computation of the table says.
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
    std::fprintf(stderr, "primers_host_check: %s: %s\n", what, ribbit_hip_last_error());
    std::exit(1);
}

// Tm of an upper-case oligo over ACGT, from the table of include/ribbit_hip.h by its letters
int32_t melting(const std::string &oligo) {
    static const struct { const char *step; int h, s; } table[] = {{"AA", -79, -222}, {"TT", -79, -222}, {"AT", -72, -204}, {"TA", -72, -213}, {"CA", -85, -227}, {"TG", -85, -227},
                                                                   {"GT", -84, -224}, {"AC", -84, -224}, {"CT", -78, -210}, {"AG", -78, -210}, {"GA", -82, -222}, {"TC", -82, -222},
                                                                   {"CG", -106, -272}, {"GC", -98, -244}, {"GG", -80, -199}, {"CC", -80, -199}};
    long h = 0, s = -11 * ((long)oligo.size() - 1) - 362;
    for (size_t j = 0; j + 1 < oligo.size(); ++j)
        for (const auto &row : table)
            if (oligo.compare(j, 2, row.step) == 0) { h += row.h; s += row.s; }
    for (const char end : {oligo.front(), oligo.back()}) {
        const bool gc = end == 'C' || end == 'G';
        h += gc ? 1 : 23;
        s += gc ? -28 : 41;
    }
    return (int32_t)((10000 * -h) / -s) - 2732;
}

size_t check_side(const std::string &seq, const RibbitPrimer &p, int32_t candidates, int64_t from, int64_t to, const RibbitPrimerParams &prm) {
    if (p.start < 0) {
        if (p.length || p.tm || p.penalty || p.bases_lo || p.bases_hi || candidates) { std::fprintf(stderr, "a missing primer with values\n"); std::exit(1); }
        return 0;
    }
    if (p.start < from || (int64_t)p.start + p.length > to || p.length < prm.min_length || p.length > prm.max_length || candidates < 1) { std::fprintf(stderr, "a primer outside its flank\n"); std::exit(1); }
    const uint64_t bases = (uint64_t)(uint32_t)p.bases_hi << 32 | (uint32_t)p.bases_lo;
    std::string oligo;
    for (int32_t j = 0; j < p.length; ++j) oligo += "ACGT"[(bases >> (2 * j)) & 3];
    for (int32_t j = 0; j < p.length; ++j)
        if (std::toupper((unsigned char)seq[(size_t)p.start + j]) != oligo[j]) { std::fprintf(stderr, "a primer that does not spell the record\n"); std::exit(1); }
    if (melting(oligo) != p.tm || p.tm < prm.tm_min || p.tm > prm.tm_max) { std::fprintf(stderr, "a primer that melts at %d, not %d\n", (int)melting(oligo), (int)p.tm); std::exit(1); }
    return 1;
}

}  // namespace

int main() {
    std::mt19937 rng(17);
    size_t found = 0, sides = 0;
    RibbitPrimerParams small;
    ribbit_primer_params_default(&small);
    small.min_length = 5; small.max_length = 8; small.opt_length = 6; small.tm_min = 0; small.tm_opt = 150; small.tm_max = 400; small.gc_min_percent = 20; small.gc_max_percent = 80;
    for (const int64_t length : {0, 1, 64, 1000, 5000}) {
        std::string seq;
        for (int64_t i = 0; i < length; ++i) seq += "ACGTacgtACGTacgtNx"[rng() % 18];
        std::vector<int32_t> rows, targets;
        for (int i = 0; i < 20; ++i) {
            const int32_t s = (int32_t)(rng() % (uint32_t)(length + 7)) - 3;
            rows.push_back(s);
            rows.push_back(s + (int32_t)(rng() % 30) - 2);
        }
        for (int i = 0; i < 150; ++i) {
            const int32_t s = (int32_t)(rng() % (uint32_t)(length + 7)) - 3;
            targets.push_back(s);
            targets.push_back(s + (int32_t)(rng() % 40) - 2);
        }
        targets.insert(targets.end(), {INT32_MIN, INT32_MAX, INT32_MAX, INT32_MIN, 0, (int32_t)length, (int32_t)length, (int32_t)length, 0, 0});
        for (const int32_t flank : {0, 4, 200, 1000})
            for (const bool defaults : {true, false}) {
                RibbitPrimerParams prm = small;
                if (defaults) ribbit_primer_params_default(&prm);
                prm.flank = flank;
                RibbitRowPrimers *out = nullptr;
                if (ribbit_host_record_primers(seq.data(), length, rows.data(), rows.size() / 2, targets.data(), targets.size() / 2, &prm, &out) != RIBBIT_OK) die("ribbit_host_record_primers");
                for (size_t i = 0; i < targets.size() / 2; ++i) {
                    const int64_t s = std::min(std::max<int64_t>(targets[2 * i], 0), length), e = std::min(std::max<int64_t>(targets[2 * i + 1], s), length);
                    found += check_side(seq, out[i].left, out[i].left_candidates, std::max<int64_t>(s - flank, 0), s, prm);
                    found += check_side(seq, out[i].right, out[i].right_candidates, e, std::min<int64_t>(e + flank, length), prm);
                    sides += 2;
                }
                ribbit_primers_free(out);
            }
    }
    if (found < 100) { std::fprintf(stderr, "only %zu primers\n", found); return 1; }
    // enough rows for the BED text to be cut into pieces (4 MB each), and the refusals
    const size_t n = 150000;
    std::string bed;
    std::vector<RibbitRowPrimers> rows(n);
    for (size_t i = 0; i < n; ++i) {
        bed += "rec\twith a tab\t" + std::to_string(i) + "\t" + std::to_string(i + 9) + "\tCA\t2|2\t9\t4.5\t0.9\t+\tP\t9=\n";
        RibbitRowPrimers &r = rows[i];
        r.left = RibbitPrimer{i % 3 ? (int32_t)i : -1, 1 + (int32_t)(rng() % 32), (int32_t)(rng() % 2001), 0, (int32_t)rng(), (int32_t)rng()};
        r.right = RibbitPrimer{i % 5 ? INT32_MAX - 32 : -1, 1 + (int32_t)(rng() % 32), -(int32_t)(rng() % 2001), 0, (int32_t)rng(), (int32_t)rng()};
        r.left_candidates = (int32_t)(rng() >> 1);
        r.right_candidates = 0;
    }
    bed.pop_back();      // (a last line without its newline)
    char *text = nullptr, *none = nullptr;
    size_t len = 0;
    if (ribbit_bed_primers_text(bed.data(), bed.size(), rows.data(), n, &text, &len) != RIBBIT_OK) die("ribbit_bed_primers_text");
    if ((size_t)std::count(text, text + len, '\n') != n || (size_t)std::count(text, text + len, '\t') != 22 * n) { std::fprintf(stderr, "the text has the wrong shape\n"); return 1; }
    ribbit_text_free(text);
    rows[n - 1].left = RibbitPrimer{5, 33, 0, 0, 0, 0};
    if (ribbit_bed_primers_text(bed.data(), bed.size(), rows.data(), n, &none, &len) != RIBBIT_E_ARG) die("a primer of 33 bases was taken");
    if (ribbit_bed_primers_text(bed.data(), bed.size() / 2, rows.data(), n, &none, &len) != RIBBIT_E_ARG) die("half a BED text was taken");
    RibbitPrimerParams bad;
    ribbit_primer_params_default(&bad);
    bad.flank = RIBBIT_PRIMER_MAX_FLANK + 1;
    RibbitRowPrimers *out = nullptr;
    if (ribbit_host_record_primers("ACGT", 4, nullptr, 0, nullptr, 0, &bad, &out) != RIBBIT_E_ARG) die("a flank of 1001 was taken");
    std::printf("ok: %zu primers on %zu sides, %zu rows as text\n", found, sides, n);
    return 0;
}
