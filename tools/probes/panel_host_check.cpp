// panel_host_check.cpp -- a stand-alone run of the host side of the multiplex panels (ribbit_host_panel_pools,
// ribbit_bed_panel_text) for the sanitizers: `make -C ribbit_amd/csrc asan-panel-check` links it against the library's host code
// built with -fsanitize=address,undefined and runs it on the CPU.  It needs no GPU and prints "ok" when the twin reproduces pinned
// values of the contract (include/ribbit_hip.h), a random panel keeps the laws every answer has, and the text has its shape.
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
    std::fprintf(stderr, "panel_host_check: %s: %s\n", what, ribbit_hip_last_error());
    std::exit(1);
}

[[noreturn]] void wrong(const char *what) {
    std::fprintf(stderr, "panel_host_check: %s\n", what);
    std::exit(1);
}

std::string reverse_complement(const std::string &o) {
    std::string q;
    for (size_t j = o.size(); j-- > 0;) q += o[j] == 'A' ? 'T' : o[j] == 'C' ? 'G' : o[j] == 'G' ? 'C' : 'A';
    return q;
}

RibbitPrimer primer_of(const std::string &forward_bases, int32_t start) {
    uint64_t bases = 0;
    for (size_t j = 0; j < forward_bases.size(); ++j) bases |= (uint64_t)(std::string("ACGT").find(forward_bases[j])) << (2 * j);
    return RibbitPrimer{start, (int32_t)forward_bases.size(), 600, 0, (int32_t)(uint32_t)bases, (int32_t)(uint32_t)(bases >> 32)};
}

// the left primer a at `start` and the right primer b (as ordered), the product `product` long
RibbitRowPrimerPair pair_of(const std::string &a, const std::string &b, int32_t start, int32_t product) {
    RibbitRowPrimerPair r{};
    r.left = primer_of(a, start);
    r.right = primer_of(reverse_complement(b), start + product - (int32_t)b.size());
    r.product = product;
    return r;
}

const char *kQuiet[8] = {"TTCAGGACCTAACCTGAG", "TAGCCAAGTTCAACGGCAG", "TGCAACCTAGGGAGAATGTG", "ACATACGCTCTTACTGCGGTC",
                         "CGGAGCATAAATCCCACC", "GAACTAAGTTTGTCGAACC", "GGTAAACGAACCGTTGCG", "AATTTGAAGCAGTGGCCGGG"};
RibbitRowPrimerPair quiet(int k, int32_t start, int32_t product) { return pair_of(kQuiet[2 * k], kQuiet[2 * k + 1], start, product); }

struct Pooled {
    std::vector<RibbitPanelRow> rows;
    int32_t pools = 0;
};
Pooled pooled(const std::vector<RibbitRowPrimerPair> &pairs, const int32_t *extra, const RibbitPanelParams &prm) {
    RibbitPanelRow *rows = nullptr;
    Pooled out;
    if (ribbit_host_panel_pools(pairs.data(), extra, pairs.size(), &prm, &rows, &out.pools) != RIBBIT_OK) die("ribbit_host_panel_pools");
    out.rows.assign(rows, rows + pairs.size());
    ribbit_panel_free(rows);
    return out;
}

bool is(const RibbitPanelRow &r, int32_t pool, int32_t conflicts, int32_t dimer, int32_t size, int32_t near) {
    return r.pool == pool && r.conflicts == conflicts && r.dimer == dimer && r.size == size && r.near == near && r.reserved[0] == 0 && r.reserved[1] == 0 && r.reserved[2] == 0;
}

}  // namespace

int main() {
    RibbitPanelParams prm;
    ribbit_panel_params_default(&prm);
    if (prm.max_cross_any != 6 || prm.max_cross_end != 4 || prm.size_gap != 30 || prm.max_cross_product != 4000 || prm.pool_size != 8) wrong("the defaults");
    // the pinned values
    Pooled p = pooled({quiet(0, 0, 100), quiet(1, 1000, 150)}, nullptr, prm);
    if (p.pools != 1 || !is(p.rows[0], 0, 0, 0, 0, 0) || !is(p.rows[1], 0, 0, 0, 0, 0)) wrong("two pairs without a conflict");
    const std::vector<RibbitRowPrimerPair> dimers = {pair_of("GATTACAGATTACAGGC", kQuiet[0], 0, 100), pair_of(kQuiet[2], "TTTGCCTGTAATC", 0, 200)};
    p = pooled(dimers, nullptr, prm);
    if (p.pools != 2 || !is(p.rows[0], 0, 1, 1, 0, 0) || !is(p.rows[1], 1, 1, 1, 0, 0)) wrong("the dimer of (10, 10)");
    RibbitPanelParams loose = prm;
    loose.max_cross_any = loose.max_cross_end = 32;
    if (pooled(dimers, nullptr, loose).pools != 1) wrong("the limits at 32");
    p = pooled({quiet(0, 0, 100), quiet(1, 0, 129)}, nullptr, prm);
    if (p.pools != 2 || !is(p.rows[1], 1, 1, 0, 1, 0)) wrong("sizes 29 apart");
    if (pooled({quiet(0, 0, 100), quiet(1, 0, 130)}, nullptr, prm).pools != 1) wrong("sizes 30 apart");
    const int32_t one_group[6] = {5, 100, 100, 5, 150, 150}, two_groups[6] = {5, 100, 100, 6, 150, 150};
    p = pooled({quiet(0, 0, 100), quiet(1, 3850, 150)}, one_group, prm);
    if (p.pools != 2 || !is(p.rows[0], 0, 1, 0, 0, 1)) wrong("a hull of 4000");
    if (pooled({quiet(0, 0, 100), quiet(1, 3851, 150)}, one_group, prm).pools != 1) wrong("a hull of 4001");
    if (pooled({quiet(0, 0, 100), quiet(1, 3850, 150)}, two_groups, prm).pools != 1) wrong("two groups");
    const int32_t star[12] = {-1, 100, 100, -1, 200, 200, -1, 300, 300, -1, 90, 310};
    p = pooled({quiet(0, 0, 100), quiet(1, 0, 200), quiet(2, 0, 300), quiet(3, 0, 200)}, star, prm);
    if (p.pools != 2 || !is(p.rows[0], 1, 1, 0, 1, 0) || !is(p.rows[2], 1, 1, 0, 1, 0) || !is(p.rows[3], 0, 3, 0, 3, 0)) wrong("the star: the degree order");
    RibbitRowPrimerPair none{};
    none.left = none.right = RibbitPrimer{-1, 0, 0, 0, 0, 0};
    p = pooled({quiet(0, 0, 100), none, quiet(1, 1000, 150)}, nullptr, prm);
    if (p.pools != 1 || !is(p.rows[1], -1, 0, 0, 0, 0) || !is(p.rows[2], 0, 0, 0, 0, 0)) wrong("a row without a pair");
    if (pooled({}, nullptr, prm).pools != 0) wrong("no pairs");

    // a random panel on several threads: the laws of every answer
    std::mt19937 rng(7);
    const size_t n = 400;
    std::vector<RibbitRowPrimerPair> many;
    std::vector<int32_t> extra;
    for (size_t i = 0; i < n; ++i) {
        std::string a, b;
        for (unsigned j = 0, k = 15 + rng() % 18; j < k; ++j) a += "ACGT"[rng() % 4];
        for (unsigned j = 0, k = 15 + rng() % 18; j < k; ++j) b += "ACGT"[rng() % 4];
        const int32_t product = 80 + (int32_t)(rng() % 400);
        many.push_back(i % 9 == 8 ? none : pair_of(a, b, (int32_t)(rng() % 50000), product));
        extra.insert(extra.end(), {(int32_t)(rng() % 4) - 1, product - (int32_t)(rng() % 10), product + (int32_t)(rng() % 10)});
    }
    RibbitPanelParams five = prm;
    five.pool_size = 5;
    p = pooled(many, extra.data(), five);
    std::vector<int32_t> filled((size_t)p.pools, 0);
    for (size_t i = 0; i < n; ++i) {
        const RibbitPanelRow &r = p.rows[i];
        if (i % 9 == 8) {
            if (!is(r, -1, 0, 0, 0, 0)) wrong("a row without a pair has a pool or a count");
            continue;
        }
        if (r.pool < 0 || r.pool >= p.pools || ++filled[(size_t)r.pool] > 5) wrong("a pool outside the pools, or one with more than pool_size members");
        if (r.conflicts < std::max(r.dimer, std::max(r.size, r.near)) || r.conflicts > r.dimer + r.size + r.near) wrong("the counts of a row do not add up");
    }
    if (std::count(filled.begin(), filled.end(), 0)) wrong("an empty pool");

    // the text: a line per row with its designed product in the ninth of its last 20 columns; only the members, sorted
    std::string marker;
    for (size_t i = 0; i < n; ++i)
        marker += "rec\twith a tab\t" + std::to_string(i) + "\t" + std::to_string(i + 9) + "\tCA\t2|2\t9\t4.5\t0.9\t+\tP\t9=\t5\t23\tACGT\t60.0\t63\t81\tACGT\t60.0\t" +
                  std::to_string(many[i].product) + "\t1\tother\t0\t90\t+\t90\t3\t.\t.\t.\t.\n";
    marker.pop_back();      // (a last line without its newline)
    char *text = nullptr, *refused = nullptr;
    size_t len = 0;
    if (ribbit_bed_panel_text(marker.data(), marker.size(), p.rows.data(), n, &text, &len) != RIBBIT_OK) die("ribbit_bed_panel_text");
    const size_t members = n - (n + 0) / 9;
    if ((size_t)std::count(text, text + len, '\n') != members || (size_t)std::count(text, text + len, '\t') != members * (31 + 5)) wrong("the text has the wrong shape");
    if (std::strncmp(text, "rec\twith a tab\t", 15) != 0 || std::strstr(text, "\t-1\t0\t0\t0\t0\n")) wrong("the text holds a row that has no pool");
    ribbit_text_free(text);
    if (ribbit_bed_panel_text(marker.data(), marker.size() / 2, p.rows.data(), n, &refused, &len) != RIBBIT_E_ARG) die("half a marker text was taken");
    if (ribbit_bed_panel_text("a\tb\n", 4, p.rows.data(), 1, &refused, &len) != RIBBIT_E_ARG) die("a line without a designed product was taken");

    // the refusals
    RibbitPanelRow *rows = nullptr;
    int32_t pools = 0;
    RibbitPanelParams bad = prm;
    bad.pool_size = 0;
    if (ribbit_host_panel_pools(many.data(), nullptr, n, &bad, &rows, &pools) != RIBBIT_E_ARG || !std::strstr(ribbit_hip_last_error(), "pool_size")) die("a pool_size of 0 was taken");
    extra[4] = extra[5] + 1;
    if (ribbit_host_panel_pools(many.data(), extra.data(), n, &prm, &rows, &pools) != RIBBIT_E_ARG || !std::strstr(ribbit_hip_last_error(), "pair 1")) die("size_lo above size_hi was taken");
    many[3].left.length = 33;
    if (ribbit_host_panel_pools(many.data(), nullptr, n, &prm, &rows, &pools) != RIBBIT_E_ARG || !std::strstr(ribbit_hip_last_error(), "pair 3")) die("a primer of 33 bases was taken");
    std::printf("ok: the pinned values, %zu rows in %d pools, %zu lines of text\n", n, (int)p.pools, members);
    return 0;
}
