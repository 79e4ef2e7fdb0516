// alleles_host_check.cpp -- a stand-alone run of the host side of the markers' alleles (ribbit_host_marker_alleles,
// ribbit_pair_amplicon_sizes, ribbit_bed_alleles_text, ribbit_allele_matrix_text) for the sanitizers: `make -C ribbit_amd/csrc
// asan-alleles-check` links it against the library's host code built with -fsanitize=address,undefined and runs it on the CPU.  It
// needs no GPU and prints "ok" when the twin reproduces the pinned values of the contract (include/ribbit_hip.h), a few thousand
// random markers keep the laws every answer has, the cells come out of hand-made amplicons and both texts have their shape.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <random>
#include <string>
#include <vector>

#include "ribbit_hip.h"

namespace {

[[noreturn]] void die(const char *what) {
    std::fprintf(stderr, "alleles_host_check: %s: %s\n", what, ribbit_hip_last_error());
    std::exit(1);
}

[[noreturn]] void wrong(const char *what) {
    std::fprintf(stderr, "alleles_host_check: %s\n", what);
    std::exit(1);
}

// the records of n markers over the S rows of `cells`
std::vector<RibbitRowAlleles> alleles(const std::vector<int32_t> &cells, size_t S, size_t n, const std::vector<int32_t> &designed, const std::vector<int32_t> &steps) {
    RibbitRowAlleles *rows = nullptr;
    if (ribbit_host_marker_alleles(cells.data(), S, n, designed.data(), steps.data(), &rows) != RIBBIT_OK) die("ribbit_host_marker_alleles");
    std::vector<RibbitRowAlleles> out(rows, rows + n);
    ribbit_alleles_free(rows);
    return out;
}

// one marker with designed = 100 and a motif of 2 over these cells
RibbitRowAlleles one(const std::vector<int32_t> &column, int32_t designed = 100) { return alleles(column, column.size(), 1, {designed}, {2})[0]; }

bool is(const RibbitRowAlleles &r, const int32_t (&v)[11], int64_t het, int64_t pic) {
    const int32_t got[11] = {r.typed, r.absent, r.several, r.over, r.alleles, r.min_size, r.max_size, r.major_size, r.major_count, r.same, r.off_step};
    return std::equal(v, v + 11, got) && r.reserved == 0 && r.het_num == het && r.pic_num == pic;
}

RibbitPrimer primer_of(const std::string &forward_bases, int32_t start) {
    uint64_t bases = 0;
    for (size_t j = 0; j < forward_bases.size(); ++j) bases |= (uint64_t)(std::string("ACGT").find(forward_bases[j])) << (2 * j);
    return RibbitPrimer{start, (int32_t)forward_bases.size(), 600, 0, (int32_t)(uint32_t)bases, (int32_t)(uint32_t)(bases >> 32)};
}

}  // namespace

int main() {
    // the pinned values
    if (!is(one({100, 100, 100, 100}), {4, 0, 0, 0, 1, 100, 100, 100, 4, 4, 0}, 0, 0)) wrong("case A");
    if (!is(one({100, 104}), {2, 0, 0, 0, 2, 100, 104, 100, 1, 1, 0}, 2, 6)) wrong("case B");
    if (!is(one({100, 102, 102, 105, 0, -1, -2}), {4, 1, 1, 1, 3, 100, 105, 102, 2, 1, 1}, 10, 142)) wrong("case C");
    if (!is(one({100, 102, 104, 106}), {4, 0, 0, 0, 4, 100, 106, 100, 1, 1, 0}, 12, 180)) wrong("case D");
    if (!is(one({0, 0, 0}), {0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0}, 0, 0)) wrong("case E");
    if (!is(one({100, 102, 0, -1}, -1), {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, 0, 0)) wrong("case F");
    if (!alleles({}, 3, 0, {}, {}).empty()) wrong("no markers");

    // a few thousand random markers on several threads: the laws of every answer, the sums from a count of the sizes
    std::mt19937 rng(11);
    const size_t S = 37, n = 5000;
    std::vector<int32_t> cells(S * n), designed(n), steps(n);
    for (size_t i = 0; i < n; ++i) {
        designed[i] = i % 11 == 10 ? -(int32_t)(rng() % 2) : 80 + (int32_t)(rng() % 300);
        steps[i] = 1 + (int32_t)(rng() % 8);
        const int32_t spread = 1 + (int32_t)(rng() % (i % 3 == 0 ? 3 : 40));
        for (size_t s = 0; s < S; ++s) {
            const unsigned kind = rng() % 20;
            cells[s * n + i] = kind == 0 ? 0 : kind == 1 ? -1 : kind == 2 ? -2 : std::max(designed[i], 100) + steps[i] * (int32_t)(rng() % spread);
        }
    }
    cells[5 * n + 7] = INT32_MAX;
    designed[7] = 100;
    const std::vector<RibbitRowAlleles> rows = alleles(cells, S, n, designed, steps);
    size_t polymorphic = 0;
    for (size_t i = 0; i < n; ++i) {
        const RibbitRowAlleles &r = rows[i];
        if (designed[i] <= 0) {
            const RibbitRowAlleles none{};
            if (std::memcmp(&r, &none, sizeof r) != 0) wrong("a row without a pair is not sixteen zeros");
            continue;
        }
        std::map<int32_t, int64_t> count;
        for (size_t s = 0; s < S; ++s)
            if (cells[s * n + i] > 0) ++count[cells[s * n + i]];
        int64_t t = 0, Q = 0, F = 0, most = 0;
        for (const auto &c : count) {
            t += c.second;
            Q += c.second * c.second;
            F += c.second * c.second * c.second * c.second;
            most = std::max(most, c.second);
        }
        if (r.typed != t || (size_t)(r.typed + r.absent + r.several + r.over) != S || r.reserved != 0) wrong("the kinds do not add up to the samples");
        if ((size_t)r.alleles != count.size() || r.major_count != most || (t > 0 && count[r.major_size] != most)) wrong("the alleles or the most frequent one");
        if (t > 0 && (r.min_size != count.begin()->first || r.max_size != count.rbegin()->first)) wrong("the least or the largest size");
        if (r.het_num != t * t - Q || r.pic_num != t * t * t * t - t * t * Q - Q * Q + F || r.pic_num < 0 || r.pic_num > r.het_num * t * t) wrong("He or PIC");
        polymorphic += r.alleles >= 2;
    }
    if (rows[7].max_size != INT32_MAX || polymorphic < n / 2) wrong("the random markers are not what they were meant to be");

    // a sample's cells from its summed amplicons
    RibbitRowAmplicon typed{}, absent{}, several{}, over{};
    typed.products = 1;
    typed.start = 40;
    typed.end = 165;
    several.products = 3;
    over.products = -1;
    const RibbitRowAmplicon sum[4] = {typed, absent, several, over};
    int32_t row[4] = {9, 9, 9, 9};
    if (ribbit_pair_amplicon_sizes(sum, 4, row) != RIBBIT_OK) die("ribbit_pair_amplicon_sizes");
    if (row[0] != 125 || row[1] != 0 || row[2] != -1 || row[3] != -2) wrong("the cells of four amplicons");
    over.products = -2;
    if (ribbit_pair_amplicon_sizes(&over, 1, row) != RIBBIT_E_ARG) die("products of -2 were taken");

    // the texts: a line per row; 23 columns behind the line, dots without a pair; a header and a field per sample
    const size_t m = 600;
    std::string bed;
    std::vector<RibbitRowPrimerPair> pairs(m);
    for (size_t i = 0; i < m; ++i) {
        bed += "rec\twith a tab\t" + std::to_string(10 * i) + "\t" + std::to_string(10 * i + 9) + "\tCA\t2|2\t9\t4.5\t0.9\t+\tP\t9=\n";
        pairs[i].left = designed[i] > 0 ? primer_of("GATTACAGATTACAGGCT", 5) : RibbitPrimer{-1, 0, 0, 0, 0, 0};
        pairs[i].right = designed[i] > 0 ? primer_of("TTGATCCGAGACTTCAGG", 5 + designed[i] - 18) : RibbitPrimer{-1, 0, 0, 0, 0, 0};
        pairs[i].product = std::max(designed[i], 0);
    }
    bed.pop_back();      // (a last line without its newline)
    std::vector<int32_t> some(S * m), some_designed(designed.begin(), designed.begin() + m), some_steps(steps.begin(), steps.begin() + m);
    for (size_t s = 0; s < S; ++s) std::copy(cells.begin() + s * n, cells.begin() + s * n + m, some.begin() + s * m);
    const std::vector<RibbitRowAlleles> some_rows = alleles(some, S, m, some_designed, some_steps);
    char *text = nullptr, *refused = nullptr;
    size_t len = 0;
    if (ribbit_bed_alleles_text(bed.data(), bed.size(), pairs.data(), some_rows.data(), S, m, &text, &len) != RIBBIT_OK) die("ribbit_bed_alleles_text");
    if ((size_t)std::count(text, text + len, '\n') != m || (size_t)std::count(text, text + len, '\t') != m * (11 + 23)) wrong("the alleles text has the wrong shape");
    if (std::strncmp(text, "rec\twith a tab\t0\t9\tCA\t", 22) != 0) wrong("the alleles text does not start with its row");
    ribbit_text_free(text);
    if (ribbit_bed_alleles_text(bed.data(), bed.size() / 2, pairs.data(), some_rows.data(), S, m, &refused, &len) != RIBBIT_E_ARG) die("half a BED text was taken");
    if (ribbit_bed_alleles_text(bed.data(), bed.size(), pairs.data(), some_rows.data(), 3, m, &refused, &len) != RIBBIT_E_ARG) die("more typed cells than samples were taken");
    std::string names;
    std::vector<int32_t> name_at{0};
    for (size_t s = 0; s < S; ++s) {
        names += "sample " + std::to_string(s);
        name_at.push_back((int32_t)names.size());
    }
    if (ribbit_allele_matrix_text(bed.data(), bed.size(), some.data(), S, m, some_designed.data(), names.data(), name_at.data(), &text, &len) != RIBBIT_OK) die("ribbit_allele_matrix_text");
    if ((size_t)std::count(text, text + len, '\n') != m + 1 || (size_t)std::count(text, text + len, '\t') != 4 + S + m * (5 + S)) wrong("the matrix text has the wrong shape");
    if (std::strncmp(text, "#name\tstart\tend\tmotif\tdesigned\tsample 0\t", 40) != 0) wrong("the matrix text does not start with its header");
    ribbit_text_free(text);
    some[3] = -3;
    if (ribbit_allele_matrix_text(bed.data(), bed.size(), some.data(), S, m, some_designed.data(), names.data(), name_at.data(), &refused, &len) != RIBBIT_E_ARG ||
        !std::strstr(ribbit_hip_last_error(), "cell 3 "))
        die("a cell of -3 was taken by the matrix text");

    // the refusals of the twin
    RibbitRowAlleles *none = nullptr;
    if (ribbit_host_marker_alleles(some.data(), S, m, some_designed.data(), some_steps.data(), &none) != RIBBIT_E_ARG || !std::strstr(ribbit_hip_last_error(), "cell 3 "))
        die("a cell of -3 was taken");
    some_steps[9] = 0;
    if (ribbit_host_marker_alleles(some.data(), S, m, some_designed.data(), some_steps.data(), &none) != RIBBIT_E_ARG || !std::strstr(ribbit_hip_last_error(), "marker 9"))
        die("a motif length of 0 was taken");
    if (ribbit_host_marker_alleles(some.data(), 0, m, some_designed.data(), some_steps.data(), &none) != RIBBIT_E_ARG) die("no samples were taken");
    if (ribbit_host_marker_alleles(some.data(), 1025, 1, some_designed.data(), some_steps.data(), &none) != RIBBIT_E_ARG) die("1025 samples were taken");
    std::printf("ok: the pinned values, %zu random markers over %zu samples (%zu with two alleles or more), %zu lines of each text\n", n, S, polymorphic, m);
    return 0;
}
