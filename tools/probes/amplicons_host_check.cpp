// amplicons_host_check.cpp -- a stand-alone run of the host side of the pairs typed on another record
// (ribbit_host_record_pair_amplicons, ribbit_pair_amplicons_merge, ribbit_bed_marker_text) for the sanitizers:
// `make -C ribbit_amd/csrc asan-amplicons-check` links it against the library's host code built with
// -fsanitize=address,undefined and runs it on the CPU.  It needs no GPU and prints "ok" when the twin reproduces the pinned values
// of the contract (include/ribbit_hip.h), the sum keeps its laws and the text has its shape.
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
    std::fprintf(stderr, "amplicons_host_check: %s: %s\n", what, ribbit_hip_last_error());
    std::exit(1);
}

[[noreturn]] void wrong(const char *what) {
    std::fprintf(stderr, "amplicons_host_check: %s\n", what);
    std::exit(1);
}

std::string reverse_complement(const std::string &o) {
    std::string q;
    for (size_t j = o.size(); j-- > 0;) q += o[j] == 'A' ? 'T' : o[j] == 'C' ? 'G' : o[j] == 'G' ? 'C' : o[j] == 'T' ? 'A' : o[j];
    return q;
}

std::string times(const std::string &unit, int n) {
    std::string out;
    for (int i = 0; i < n; ++i) out += unit;
    return out;
}

RibbitPrimer primer_of(const std::string &forward_bases, int32_t start) {
    uint64_t bases = 0;
    for (size_t j = 0; j < forward_bases.size(); ++j) bases |= (uint64_t)(std::string("ACGT").find(forward_bases[j])) << (2 * j);
    return RibbitPrimer{start, (int32_t)forward_bases.size(), 600, 0, (int32_t)(uint32_t)bases, (int32_t)(uint32_t)(bases >> 32)};
}

const std::string Lp = "GATTACAGATTACAGGCT", Rp = "CCTGAAGTCTCGGATCAA", X = "ACGTTGCATG", Y = "CCATGACTGA";

struct Pinned {
    std::string record, motif;
    int32_t want[15];      // the four counts, products, record, then start .. tract_strand
};

}  // namespace

int main() {
    const std::string rec = Lp + X + times("CA", 10) + Y + Rp;
    std::string lower = rec;
    for (char &c : lower) c = (char)(c | 0x20);
    const int32_t label = 3;
    const std::vector<Pinned> pinned = {
        {rec, "CA", {1, 0, 0, 1, 1, label, 0, 76, 0, 1, 18, 58, 28, 49, 0}},
        {rec, "AC", {1, 0, 0, 1, 1, label, 0, 76, 0, 1, 18, 58, 28, 49, 0}},
        {rec, "TG", {1, 0, 0, 1, 1, label, 0, 76, 0, 1, 18, 58, 28, 49, 1}},
        {reverse_complement(rec), "CA", {0, 1, 1, 0, 1, label, 0, 76, 1, 0, 18, 58, 27, 48, 1}},
        {Lp + X + times("CA", 17) + Y + Rp, "CA", {1, 0, 0, 1, 1, label, 0, 90, 0, 1, 18, 72, 28, 63, 0}},
        {Lp + X + times("CA", 4) + "N" + times("CA", 5) + Y + Rp, "CA", {1, 0, 0, 1, 1, label, 0, 75, 0, 1, 18, 57, 37, 48, 0}},
        {Lp + X + "CA" + Y + Rp, "CA", {1, 0, 0, 1, 1, label, 0, 58, 0, 1, 18, 40, -1, -1, 0}},
        {lower, "CA", {1, 0, 0, 1, 1, label, 0, 76, 0, 1, 18, 58, 28, 49, 0}},
        {rec + "ACGTAGCTAGCTAGGATCGA" + rec, "CA", {2, 0, 0, 2, 3, label, 0, 76, 0, 1, 18, 58, 28, 49, 0}},
        {Lp + times("GATA", 6) + Rp, "ATAG", {1, 0, 0, 1, 1, label, 0, 60, 0, 1, 18, 42, 18, 42, 0}},
        {Lp + X, "CA", {1, 0, 0, 0, 0, -1, -1, -1, 0, 0, -1, -1, -1, -1, 0}},
    };
    RibbitProductParams prm;
    ribbit_product_params_default(&prm);
    // the pair, and a row without one, each with its motif
    RibbitRowPrimerPair pairs[2] = {};
    pairs[0].left = primer_of(Lp, 5);
    pairs[0].right = primer_of(Rp, 63);
    pairs[0].product = 76;
    pairs[1].left = pairs[1].right = RibbitPrimer{-1, 0, 0, 0, 0, 0};
    std::vector<RibbitRowAmplicon> kept;
    for (const Pinned &p : pinned) {
        const std::string pool = p.motif + "ACGT";
        const int32_t offsets[3] = {0, (int32_t)p.motif.size(), (int32_t)pool.size()};
        RibbitRowAmplicon *rows = nullptr;
        if (ribbit_host_record_pair_amplicons(p.record.data(), (int64_t)p.record.size(), pairs, 2, pool.data(), offsets, label, &prm, &rows) != RIBBIT_OK)
            die("ribbit_host_record_pair_amplicons");
        if (std::memcmp(&rows[0], p.want, sizeof p.want) != 0 || rows[0].reserved != 0) wrong("a pinned value is not reproduced");
        const int32_t none[16] = {0, 0, 0, 0, 0, -1, -1, -1, 0, 0, -1, -1, -1, -1, 0, 0};
        if (std::memcmp(&rows[1], none, sizeof none) != 0) wrong("a row without a pair is not sixteen zeros but for the positions");
        kept.push_back(rows[0]);
        ribbit_pair_amplicons_free(rows);
    }
    // an empty record and no pairs
    RibbitRowAmplicon *rows = nullptr;
    const int32_t one_offset[2] = {0, 2};
    if (ribbit_host_record_pair_amplicons("", 0, pairs, 1, "CA", one_offset, 0, &prm, &rows) != RIBBIT_OK || rows[0].products != 0 || rows[0].record != -1) die("an empty record");
    ribbit_pair_amplicons_free(rows);
    if (ribbit_host_record_pair_amplicons(rec.data(), (int64_t)rec.size(), nullptr, 0, nullptr, nullptr, 0, &prm, &rows) != RIBBIT_OK) die("no pairs");
    ribbit_pair_amplicons_free(rows);
    // over at max_sites 1, and a long motif
    RibbitProductParams one_site = prm;
    one_site.max_sites = 1;
    if (ribbit_host_record_pair_amplicons(pinned[8].record.data(), (int64_t)pinned[8].record.size(), pairs, 1, "CA", one_offset, 0, &one_site, &rows) != RIBBIT_OK) die("max_sites 1");
    const RibbitRowAmplicon over = rows[0];
    ribbit_pair_amplicons_free(rows);
    if (over.products != -1 || over.left_forward != 2 || over.record != -1 || over.tract_end != -1) wrong("a list longer than max_sites is not over");
    std::mt19937 rng(7);
    std::string motif;
    for (int j = 0; j < 1023; ++j) motif += "ACGT"[rng() % 4];
    const std::string long_record = Lp + motif.substr(1000) + motif + motif + motif.substr(0, 500) + Rp;
    const int32_t long_offsets[2] = {0, 1023};
    if (ribbit_host_record_pair_amplicons(long_record.data(), (int64_t)long_record.size(), pairs, 1, motif.data(), long_offsets, 0, &prm, &rows) != RIBBIT_OK) die("a motif of 1023 letters");
    if (rows[0].tract_start != 18 || rows[0].tract_end != 18 + 23 + 2046 + 500 || rows[0].tract_strand != 0) wrong("the tract of a motif of 1023 letters");
    ribbit_pair_amplicons_free(rows);

    // the sum: the first record's product stays, -1 wins, the counts saturate
    RibbitRowAmplicon sum[3] = {kept[10], kept[0], kept[0]};
    const RibbitRowAmplicon from[3] = {kept[4], kept[4], over};
    if (ribbit_pair_amplicons_merge(sum, from, 3) != RIBBIT_OK) die("ribbit_pair_amplicons_merge");
    if (sum[0].products != 1 || sum[0].end != 90 || sum[0].left_forward != 2 || sum[0].right_reverse != 1) wrong("a record without a product hides the next one's");
    if (sum[1].products != 2 || sum[1].end != 76 || sum[1].tract_end != 49) wrong("the first record's product is not kept");
    if (sum[2].products != -1 || sum[2].record != -1 || sum[2].start != -1 || sum[2].left_forward != 3) wrong("-1 does not win");
    RibbitRowAmplicon big = kept[0];
    big.left_forward = INT32_MAX - 1;
    big.products = INT32_MAX;
    if (ribbit_pair_amplicons_merge(&big, &kept[8], 1) != RIBBIT_OK || big.left_forward != INT32_MAX || big.products != INT32_MAX || big.end != 76) wrong("the sum does not saturate");

    // the text: enough rows for it to be cut into pieces, every kind of row, and the refusals
    const size_t n = 150000;
    const char names[] = "firstsecond onethird4";
    const int32_t name_offsets[5] = {0, 5, 15, 20, 21};
    std::string bed;
    std::vector<RibbitRowPrimerPair> many(n, pairs[0]);
    std::vector<RibbitRowAmplicon> amplicons(n);
    size_t tabs = 0;
    for (size_t i = 0; i < n; ++i) {
        bed += "rec\twith a tab\t" + std::to_string(i) + "\t" + std::to_string(i + 9) + "\tCA\t2|2\t9\t4.5\t0.9\t+\tP\t9=\n";
        amplicons[i] = i % 7 == 0 ? over : kept[i % pinned.size()];
        if (i % 5 == 4) many[i] = pairs[1];
        tabs += 11 + 20;
    }
    bed.pop_back();      // (a last line without its newline)
    char *text = nullptr, *none = nullptr;
    size_t len = 0;
    if (ribbit_bed_marker_text(bed.data(), bed.size(), many.data(), amplicons.data(), names, name_offsets, 4, n, &text, &len) != RIBBIT_OK) die("ribbit_bed_marker_text");
    if ((size_t)std::count(text, text + len, '\n') != n || (size_t)std::count(text, text + len, '\t') != tabs) wrong("the long text has the wrong shape");
    if (!std::strstr(text, "\t1\t4\t0\t76\t+\t76\t0\t28\t49\t21\t10\n") || !std::strstr(text, "\t1\t4\t0\t76\t-\t76\t0\t27\t48\t21\t10\n") || !std::strstr(text, "\t3\t.\t.\t.\t.\t.\t.\t.\t.\t.\t.\n"))
        wrong("the text does not hold the lines of the pinned values");
    ribbit_text_free(text);
    if (ribbit_bed_marker_text(bed.data(), bed.size(), many.data(), amplicons.data(), names, name_offsets, 3, n, &none, &len) != RIBBIT_E_ARG) die("a record outside the names was taken");
    if (ribbit_bed_marker_text(bed.data(), bed.size() / 2, many.data(), amplicons.data(), names, name_offsets, 4, n, &none, &len) != RIBBIT_E_ARG) die("half a BED text was taken");
    many[n - 2].left.length = 33;      // (a row that has a pair)
    if (ribbit_bed_marker_text(bed.data(), bed.size(), many.data(), amplicons.data(), names, name_offsets, 4, n, &none, &len) != RIBBIT_E_ARG) die("a primer of 33 bases was taken");
    if (ribbit_bed_marker_text("rec\t1\t2\n", 8, pairs, kept.data(), names, name_offsets, 4, 1, &none, &len) != RIBBIT_E_ARG) die("a line that is no row was taken");
    RibbitProductParams bad = prm;
    bad.seed = 17;
    if (ribbit_host_record_pair_amplicons(rec.data(), (int64_t)rec.size(), pairs, 1, "CA", one_offset, 0, &bad, &rows) != RIBBIT_E_ARG) die("a seed of 17 was taken");
    if (ribbit_host_record_pair_amplicons(rec.data(), (int64_t)rec.size(), pairs, 1, "CN", one_offset, 0, &prm, &rows) != RIBBIT_E_ARG) die("a motif with an N was taken");
    if (ribbit_host_record_pair_amplicons(rec.data(), (int64_t)rec.size(), pairs, 1, "CA", one_offset, -1, &prm, &rows) != RIBBIT_E_ARG) die("a negative record was taken");
    std::printf("ok: %zu pinned values, %zu rows as text\n", pinned.size(), n);
    return 0;
}
