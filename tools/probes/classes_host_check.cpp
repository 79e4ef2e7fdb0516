// classes_host_check.cpp -- a stand-alone run of the host side of the motif classes (ribbit_bed_motifs, ribbit_host_record_classes,
// ribbit_bed_class_text, ribbit_class_summary_text) for the sanitizers: `make -C ribbit_amd/csrc asan-classes-check` links it
// against the library's host code built with -fsanitize=address,undefined and runs it on the CPU.  It needs no GPU and prints
// "ok" when every result is what a second, naive computation gives.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "ribbit_hip.h"

namespace {

[[noreturn]] void die(const char *what) {
    std::fprintf(stderr, "classes_host_check: %s: %s\n", what, ribbit_hip_last_error());
    std::exit(1);
}

std::string naive_class(const std::string &u, char *strand) {
    std::string rc(u.rbegin(), u.rend());
    for (char &c : rc) c = c == 'A' ? 'T' : c == 'C' ? 'G' : c == 'G' ? 'C' : 'A';
    std::string best = u;
    bool own = true;
    for (int side = 0; side < 2; ++side) {
        const std::string &s = side ? rc : u;
        for (size_t r = 0; r < s.size(); ++r) {
            const std::string t = s.substr(r) + s.substr(0, r);
            if (t < best) { best = t; own = side == 0; }
        }
    }
    *strand = own ? '+' : '-';
    return best;
}

}  // namespace

int main() {
    std::mt19937 rng(7);
    const int lengths[] = {1, 2, 3, 5, 26, 27, 28, 31, 32, 33, 63, 64, 65, 127, 128, 129, 500, 990, 1023};
    std::vector<std::string> units;
    for (const int k : lengths)
        for (int t = 0; t < 3; ++t) {
            std::string u((size_t)k, 'A');
            for (char &c : u) c = "ACGT"[t == 2 ? rng() % 2 : rng() % 4];
            if (t == 1) for (size_t i = 0; i < u.size(); ++i) u[i] = "ACG"[i % 3];      // periodic: every rotation ties
            units.push_back(u);
        }
    // enough rows for the thread team and for the BED text to be cut into pieces (4 MB each)
    const size_t n = 140000;
    std::string bed;
    std::vector<std::string> motifs;
    for (size_t i = 0; i < n; ++i) {
        const std::string &u = i % 50 == 0 ? units[rng() % units.size()] : units[rng() % 12];
        const size_t r = rng() % u.size();
        motifs.push_back(u.substr(r) + u.substr(0, r));
        bed += "rec\twith a tab\t" + std::to_string((long)(i * 7) - 100) + "\t" + std::to_string(i * 7 + rng() % 90) + "\t" + motifs.back() + "\t2|2\t7\t3.5\t0.9\t+\tP\t7=\n";
    }
    bed.pop_back();      // (a last line without its newline)
    char *pool = nullptr, *classes = nullptr, *strands = nullptr, *text = nullptr, *summary = nullptr;
    int32_t *offsets = nullptr, *iv = nullptr;
    RibbitMotifClass *groups = nullptr;
    size_t rows = 0, n_iv = 0, n_groups = 0, len = 0, summary_len = 0;
    if (ribbit_bed_motifs(bed.data(), bed.size(), &pool, &offsets, &rows) != RIBBIT_OK || rows != n) die("ribbit_bed_motifs");
    if (ribbit_bed_intervals(bed.data(), bed.size(), &iv, &n_iv) != RIBBIT_OK || n_iv != n) die("ribbit_bed_intervals");
    const int64_t length = 600000;      // (rows reach past it and start before 0)
    if (ribbit_host_record_classes(length, iv, n, pool, offsets, &classes, &strands, &groups, &n_groups) != RIBBIT_OK) die("ribbit_host_record_classes");
    size_t counted = 0;
    int64_t bases = 0, want_bases = 0;
    for (size_t g = 0; g < n_groups; ++g) { counted += (size_t)groups[g].rows; bases += groups[g].bases; }
    for (size_t i = 0; i < n; ++i) {
        want_bases += std::max<int64_t>(0, std::min<int64_t>(iv[2 * i + 1], length) - std::max<int64_t>(iv[2 * i], 0));
        if (i % 37 && motifs[i].size() > 64) continue;      // (the naive form of a 1023-mer is slow)
        char strand = 0;
        const std::string want = naive_class(motifs[i], &strand);
        if (want != std::string(classes + offsets[i], classes + offsets[i + 1]) || strand != strands[i]) { std::fprintf(stderr, "row %zu differs\n", i); return 1; }
    }
    if (counted != n || bases != want_bases) { std::fprintf(stderr, "the groups hold %zu rows and %lld bases\n", counted, (long long)bases); return 1; }
    if (ribbit_bed_class_text(bed.data(), bed.size(), classes, offsets, strands, n, &text, &len) != RIBBIT_OK) die("ribbit_bed_class_text");
    if (len != bed.size() + 1 + (size_t)offsets[n] + 3 * n) { std::fprintf(stderr, "the class text has %zu bytes\n", len); return 1; }
    if (ribbit_class_summary_text("rec\twith a tab", iv, n, classes, offsets, groups, n_groups, &summary, &summary_len) != RIBBIT_OK) die("ribbit_class_summary_text");
    if ((size_t)std::count(summary, summary + summary_len, '\n') != n_groups) { std::fprintf(stderr, "the summary has the wrong number of lines\n"); return 1; }
    // the argument errors
    const int32_t bad_offsets[3] = {0, 3, 2}, one_motif[2] = {0, 4};
    int32_t *no_offsets = nullptr;
    char *a = nullptr, *b = nullptr;
    RibbitMotifClass *c = nullptr;
    size_t m = 0;
    if (ribbit_host_record_classes(100, iv, 2, "ACGT", bad_offsets, &a, &b, &c, &m) != RIBBIT_E_ARG) die("offsets that do not ascend were taken");
    if (ribbit_host_record_classes(100, iv, 1, "ACNT", one_motif, &a, &b, &c, &m) != RIBBIT_E_ARG) die("a byte outside ACGT was taken");
    if (ribbit_bed_motifs("rec\t1\t2\tAC\n", 11, &a, &no_offsets, &m) != RIBBIT_E_ARG) die("a line of four columns was taken");
    ribbit_text_free(pool);
    ribbit_text_free(classes);
    ribbit_text_free(strands);
    ribbit_text_free(text);
    ribbit_text_free(summary);
    ribbit_intervals_free(offsets);
    ribbit_intervals_free(iv);
    ribbit_motif_classes_free(groups);
    std::printf("ok: %zu rows, %zu classes, %lld bases\n", n, n_groups, (long long)bases);
    return 0;
}
