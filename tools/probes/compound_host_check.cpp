// compound_host_check.cpp -- a stand-alone run of the host side of the compound loci (ribbit_host_record_compounds,
// ribbit_class_labels, ribbit_compound_text) for the sanitizers: `make -C ribbit_amd/csrc asan-compound-check` links it against
// the library's host code built with -fsanitize=address,undefined and runs it on the CPU.  It needs no GPU and prints "ok" when
// every result is what a second, naive computation gives.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <set>
#include <string>
#include <vector>

#include "ribbit_hip.h"

namespace {

[[noreturn]] void die(const char *what) {
    std::fprintf(stderr, "compound_host_check: %s: %s\n", what, ribbit_hip_last_error());
    std::exit(1);
}

}  // namespace

int main() {
    std::mt19937 rng(11);
    const char *units[] = {"CA", "AC", "GT", "GA", "AAT", "ATT", "GATA", "TATC", "ACGTT", "A"};
    // enough rows for the BED text to be cut into pieces (4 MB each) and for the chains' lines to be written in pieces
    const size_t n = 150000;
    const int64_t length = 3000000;      // (rows reach past it and start before 0)
    std::string bed;
    for (size_t i = 0; i < n; ++i) {
        const long s = (long)(rng() % 3000200) - 100, e = s + (long)(rng() % 40) - 3;
        bed += "rec\twith a tab\t" + std::to_string(s) + "\t" + std::to_string(e) + "\t" + units[rng() % 10] + "\t2|2\t" + std::to_string(e - s) + "\t" +
               std::to_string((e - s) / 2) + ".5\t0.9\t+\tP\t7=\n";
    }
    bed.pop_back();      // (a last line without its newline)
    char *pool = nullptr, *classes = nullptr, *strands = nullptr;
    int32_t *offsets = nullptr, *iv = nullptr, *labels = nullptr;
    RibbitMotifClass *groups = nullptr;
    size_t rows = 0, n_iv = 0, n_groups = 0;
    if (ribbit_bed_motifs(bed.data(), bed.size(), &pool, &offsets, &rows) != RIBBIT_OK || rows != n) die("ribbit_bed_motifs");
    if (ribbit_bed_intervals(bed.data(), bed.size(), &iv, &n_iv) != RIBBIT_OK || n_iv != n) die("ribbit_bed_intervals");
    if (ribbit_host_record_classes(length, iv, n, pool, offsets, &classes, &strands, &groups, &n_groups) != RIBBIT_OK) die("ribbit_host_record_classes");
    if (ribbit_class_labels(classes, offsets, n, groups, n_groups, &labels) != RIBBIT_OK) die("ribbit_class_labels");
    for (size_t i = 0; i < n; ++i) {
        const RibbitMotifClass &g = groups[labels[i]];
        if (labels[i] < 0 || (size_t)labels[i] >= n_groups || g.length != offsets[i + 1] - offsets[i] ||
            std::memcmp(classes + offsets[i], classes + offsets[g.first_row], (size_t)g.length) != 0) { std::fprintf(stderr, "row %zu: label %d\n", i, (int)labels[i]); return 1; }
    }
    size_t chains_seen = 0;
    for (const int32_t gap : {0, 3, 100, INT32_MAX}) {
        RibbitCompound *chains = nullptr;
        int32_t *members = nullptr;
        size_t n_chains = 0, n_members = 0, len = 0;
        char *text = nullptr;
        if (ribbit_host_record_compounds(length, iv, labels, n, gap, &chains, &n_chains, &members, &n_members) != RIBBIT_OK) die("ribbit_host_record_compounds");
        // naive: every chain's counts again from its members
        size_t at = 0;
        int64_t reach = 0;
        for (size_t c = 0; c < n_chains; ++c) {
            const RibbitCompound &k = chains[c];
            if ((size_t)k.first != at || k.rows < 1 || k.pad != 0) { std::fprintf(stderr, "chain %zu does not follow the one before\n", c); return 1; }
            std::set<int32_t> seen;
            int64_t bases = 0;
            int32_t switches = 0, overlaps = 0;
            for (size_t j = at; j < at + (size_t)k.rows; ++j) {
                const size_t row = (size_t)members[j];
                const int64_t s = std::max<int64_t>(iv[2 * row], 0), e = std::min<int64_t>(iv[2 * row + 1], length);
                if (s >= e) { std::fprintf(stderr, "an empty member\n"); return 1; }
                if (j == at ? (c > 0 && s - reach <= gap) : s - reach > gap) { std::fprintf(stderr, "chain %zu is cut in the wrong place\n", c); return 1; }
                if (j > at) { switches += labels[row] != labels[members[j - 1]]; overlaps += s < reach; }
                reach = j == at && c == 0 ? e : std::max(reach, e);
                if (j == at && s != k.start) { std::fprintf(stderr, "chain %zu starts elsewhere\n", c); return 1; }
                bases += e - s;
                seen.insert(labels[row]);
            }
            if (bases != k.bases || switches != k.switches || overlaps != k.overlaps || (int32_t)seen.size() != k.classes || reach != k.end) {
                std::fprintf(stderr, "chain %zu differs\n", c);
                return 1;
            }
            at += (size_t)k.rows;
        }
        if (at != n_members) { std::fprintf(stderr, "the chains hold %zu of %zu members\n", at, n_members); return 1; }
        if (ribbit_compound_text("rec\twith a tab", bed.data(), bed.size(), length, iv, n, chains, n_chains, members, n_members, &text, &len) != RIBBIT_OK) die("ribbit_compound_text");
        if ((size_t)std::count(text, text + len, '\n') != n_chains || (size_t)std::count(text, text + len, '(') != n_members) { std::fprintf(stderr, "the text has the wrong shape\n"); return 1; }
        // the argument errors
        char *none = nullptr;
        if (n_chains) {
            RibbitCompound bad = chains[n_chains - 1];
            bad.rows += 1;
            if (ribbit_compound_text("r", bed.data(), bed.size(), length, iv, n, &bad, 1, members, n_members, &none, &len) != RIBBIT_E_ARG) die("rows outside members were taken");
            if (ribbit_compound_text("r", bed.data(), bed.size() / 2, length, iv, n, chains, n_chains, members, n_members, &none, &len) != RIBBIT_E_ARG) die("half a BED text was taken");
        }
        chains_seen += n_chains;
        ribbit_text_free(text);
        ribbit_compounds_free(chains);
        ribbit_intervals_free(members);
    }
    RibbitCompound *chains = nullptr;
    int32_t *members = nullptr, *no_labels = nullptr;
    size_t a = 0, b = 0;
    if (ribbit_host_record_compounds(length, iv, labels, n, -1, &chains, &a, &members, &b) != RIBBIT_E_ARG) die("a negative gap was taken");
    if (n_groups > 1 && ribbit_class_labels(classes, offsets, n, groups + 1, n_groups - 1, &no_labels) != RIBBIT_E_ARG) die("a row without a group was taken");
    ribbit_text_free(pool);
    ribbit_text_free(classes);
    ribbit_text_free(strands);
    ribbit_intervals_free(offsets);
    ribbit_intervals_free(iv);
    ribbit_intervals_free(labels);
    ribbit_motif_classes_free(groups);
    std::printf("ok: %zu rows, %zu classes, %zu chains at four gaps\n", n, n_groups, chains_seen);
    return 0;
}
