// primer_products_host_check.cpp -- a stand-alone run of the host side of the in-silico PCR (ribbit_host_record_oligo_sites,
// ribbit_host_record_primer_products, ribbit_bed_primer_products_text) for the sanitizers:
// `make -C ribbit_amd/csrc asan-primer-products-check` links it against the library's host code built with
// -fsanitize=address,undefined and runs it on the CPU.  It needs no GPU and prints "ok" when every site spells its oligo's 3' end in
// the record, every list lies where its record says, and the products fit the sites.
#include <algorithm>
#include <cctype>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include <vector>

#include "ribbit_hip.h"

namespace {

[[noreturn]] void die(const char *what) {
    std::fprintf(stderr, "primer_products_host_check: %s: %s\n", what, ribbit_hip_last_error());
    std::exit(1);
}

[[noreturn]] void wrong(const char *what) {
    std::fprintf(stderr, "primer_products_host_check: %s\n", what);
    std::exit(1);
}

RibbitOligo oligo_of(const std::string &letters) {
    uint64_t bases = 0;
    for (size_t j = 0; j < letters.size(); ++j) bases |= (uint64_t)(std::string("ACGT").find(letters[j])) << (2 * j);
    return RibbitOligo{(int32_t)letters.size(), (int32_t)(uint32_t)bases, (int32_t)(uint32_t)(bases >> 32)};
}

std::string reverse_complement(const std::string &o) {
    std::string q;
    for (size_t j = o.size(); j-- > 0;) q += o[j] == 'A' ? 'T' : o[j] == 'C' ? 'G' : o[j] == 'G' ? 'C' : 'A';
    return q;
}

}  // namespace

int main() {
    std::mt19937 rng(23);
    size_t sites_seen = 0, products_seen = 0;
    for (const int64_t length : {0, 1, 40, 700, 5000}) {
        std::string seq;
        for (int64_t i = 0; i < length; ++i) seq += "ACGTacgtACGTacgtACGTacgtACGTACGTNx"[rng() % 34];
        for (const RibbitProductParams prm : {RibbitProductParams{15, 2, 4000, 64}, RibbitProductParams{6, 32, 200, 3}, RibbitProductParams{16, 0, INT32_MAX, 1024}}) {
            // oligos cut from the record, either strand, some with a base changed
            std::vector<std::string> letters;
            std::vector<RibbitOligo> oligos;
            int64_t before = 0;
            for (int i = 0; i < 60; ++i) {
                const int32_t k = prm.seed + (int32_t)(rng() % (uint32_t)(33 - prm.seed));
                std::string o;
                // an odd one lies 60 bases behind the even one before it and is read from the other strand: the two make a product
                const int64_t at = length <= k ? 0 : i % 2 ? std::min<int64_t>(before + 60, length - k - 1) : (int64_t)(rng() % (uint64_t)(length - k));
                before = at;
                for (int32_t j = 0; j < k; ++j) {
                    const char c = at + j < length ? (char)std::toupper((unsigned char)seq[(size_t)(at + j)]) : 'A';
                    o += std::string("ACGT").find(c) == std::string::npos ? 'A' : c;
                }
                if (rng() % 3 == 0) o[rng() % o.size()] = "ACGT"[rng() % 4];
                if (i % 2) o = reverse_complement(o);
                letters.push_back(o);
                oligos.push_back(oligo_of(o));
            }
            RibbitOligoSites *sites = nullptr;
            int32_t *positions = nullptr;
            size_t n_positions = 0, at = 0;
            if (ribbit_host_record_oligo_sites(seq.data(), length, oligos.data(), oligos.size(), &prm, &sites, &positions, &n_positions) != RIBBIT_OK)
                die("ribbit_host_record_oligo_sites");
            for (size_t i = 0; i < oligos.size(); ++i) {
                const std::string &o = letters[i], q = reverse_complement(o);
                const struct { int32_t count, from; bool reverse; } lists[2] = {{sites[i].forward, sites[i].forward_at, false}, {sites[i].reverse, sites[i].reverse_at, true}};
                for (const auto &l : lists) {
                    if (l.count > prm.max_sites) {
                        if (l.from != -1) wrong("a list that is too long has a place");
                        continue;
                    }
                    if ((size_t)l.from != at) wrong("a list that does not start where the one before ends");
                    for (int32_t j = 0; j < l.count; ++j) {
                        const int32_t x = positions[at + (size_t)j];
                        if (x < 0 || (int64_t)x + (int64_t)o.size() > length || (j > 0 && x <= positions[at + (size_t)j - 1])) wrong("a site outside the record or out of order");
                        // the seed spells the record: the oligo's last bases on the forward strand, its complement's first on the reverse
                        for (int32_t s = 0; s < prm.seed; ++s) {
                            const size_t w = l.reverse ? (size_t)s : o.size() - (size_t)prm.seed + (size_t)s;
                            if (std::toupper((unsigned char)seq[(size_t)x + w]) != (l.reverse ? q[w] : o[w])) wrong("a site whose seed does not spell the record");
                        }
                        ++sites_seen;
                    }
                    at += (size_t)l.count;
                }
            }
            if (at != n_positions) wrong("positions that no list holds");
            // the oligos two by two as pairs (the right primer's record holds its forward-strand bases), the odd ones without a pair
            std::vector<RibbitRowPrimerPair> pairs(oligos.size() / 2);
            for (size_t i = 0; i < pairs.size(); ++i) {
                RibbitRowPrimerPair r{};
                const RibbitOligo a = oligos[2 * i], b = oligo_of(reverse_complement(letters[2 * i + 1]));
                r.left = RibbitPrimer{i % 5 == 4 ? -1 : (int32_t)(rng() % (uint32_t)(length + 1)), a.length, 0, 0, a.bases_lo, a.bases_hi};
                r.right = RibbitPrimer{(int32_t)(rng() % (uint32_t)(length + 1)), b.length, 0, 0, b.bases_lo, b.bases_hi};
                pairs[i] = r;
            }
            RibbitRowProducts *rows = nullptr;
            if (ribbit_host_record_primer_products(seq.data(), length, pairs.data(), pairs.size(), &prm, &rows) != RIBBIT_OK) die("ribbit_host_record_primer_products");
            for (size_t i = 0; i < pairs.size(); ++i) {
                const RibbitRowProducts &r = rows[i];
                const RibbitOligoSites &a = sites[2 * i], &b = sites[2 * i + 1];
                if (pairs[i].left.start < 0) {
                    if (r.left_forward || r.left_reverse || r.right_forward || r.right_reverse || r.products || r.own || r.shortest_other) wrong("products without a pair");
                    continue;
                }
                if (r.left_forward != a.forward || r.left_reverse != a.reverse || r.right_forward != b.forward || r.right_reverse != b.reverse) wrong("a pair's counts are not its oligos'");
                const bool over = std::max(std::max(a.forward, a.reverse), std::max(b.forward, b.reverse)) > prm.max_sites;
                if (over ? r.products != -1 || r.own || r.shortest_other : r.products < r.own || r.own > 1 || r.shortest_other > prm.max_product ||
                               r.products > (a.forward + b.forward) * (a.reverse + b.reverse) || (r.shortest_other > 0) != (r.products > r.own))
                    wrong("products that do not fit the sites");
                products_seen += over ? 0 : (size_t)r.products;
            }
            // the text of these pairs
            std::string bed;
            for (size_t i = 0; i < pairs.size(); ++i) bed += "rec\t" + std::to_string(i) + "\t" + std::to_string(i + 9) + "\tCA\n";
            char *text = nullptr;
            size_t len = 0;
            if (ribbit_bed_primer_products_text(bed.data(), bed.size(), pairs.data(), rows, pairs.size(), &text, &len) != RIBBIT_OK) die("ribbit_bed_primer_products_text");
            if ((size_t)std::count(text, text + len, '\n') != pairs.size() || (size_t)std::count(text, text + len, '\t') != (3 + 27) * pairs.size()) wrong("the text has the wrong shape");
            ribbit_text_free(text);
            ribbit_products_free(rows);
            ribbit_products_free(sites);
            ribbit_products_free(positions);
        }
    }
    if (sites_seen < 100 || products_seen < 5) { std::fprintf(stderr, "only %zu sites and %zu products\n", sites_seen, products_seen); return 1; }
    // enough rows for the BED text to be cut into pieces, and the refusals
    const size_t n = 150000;
    std::string bed;
    std::vector<RibbitRowPrimerPair> pairs(n);
    std::vector<RibbitRowProducts> rows(n);
    for (size_t i = 0; i < n; ++i) {
        bed += "rec\twith a tab\t" + std::to_string(i) + "\t" + std::to_string(i + 9) + "\tCA\t2|2\t9\t4.5\t0.9\t+\tP\t9=\n";
        RibbitRowPrimerPair &r = pairs[i];
        int32_t *fields = reinterpret_cast<int32_t *>(&r);
        for (int j = 12; j < 32; ++j) fields[j] = (int32_t)(rng() >> 1);
        r.left = RibbitPrimer{i % 3 ? (int32_t)i : -1, 1 + (int32_t)(rng() % 32), (int32_t)(rng() % 2001), 0, (int32_t)rng(), (int32_t)rng()};
        r.right = RibbitPrimer{i % 5 ? INT32_MAX - 32 : -1, 1 + (int32_t)(rng() % 32), -(int32_t)(rng() % 2001), 0, (int32_t)rng(), (int32_t)rng()};
        rows[i] = RibbitRowProducts{(int32_t)(rng() >> 1), (int32_t)(rng() >> 1), (int32_t)(rng() >> 1), (int32_t)(rng() >> 1), i % 7 ? (int32_t)(rng() >> 1) : -1, (int32_t)(i % 2),
                                    (int32_t)(rng() >> 1), 0};
    }
    bed.pop_back();      // (a last line without its newline)
    char *text = nullptr, *none = nullptr;
    size_t len = 0;
    if (ribbit_bed_primer_products_text(bed.data(), bed.size(), pairs.data(), rows.data(), n, &text, &len) != RIBBIT_OK) die("ribbit_bed_primer_products_text");
    if ((size_t)std::count(text, text + len, '\n') != n || (size_t)std::count(text, text + len, '\t') != 38 * n) wrong("the long text has the wrong shape");
    ribbit_text_free(text);
    pairs[n - 1].left = RibbitPrimer{5, 33, 0, 0, 0, 0};
    pairs[n - 1].right.start = 7;
    if (ribbit_bed_primer_products_text(bed.data(), bed.size(), pairs.data(), rows.data(), n, &none, &len) != RIBBIT_E_ARG) die("a primer of 33 bases was taken");
    if (ribbit_bed_primer_products_text(bed.data(), bed.size() / 2, pairs.data(), rows.data(), n, &none, &len) != RIBBIT_E_ARG) die("half a BED text was taken");
    RibbitProductParams bad;
    ribbit_product_params_default(&bad);
    bad.seed = 17;
    RibbitRowProducts *out = nullptr;
    if (ribbit_host_record_primer_products("ACGT", 4, pairs.data(), 1, &bad, &out) != RIBBIT_E_ARG) die("a seed of 17 was taken");
    ribbit_product_params_default(&bad);
    RibbitOligoSites *sites = nullptr;
    int32_t *positions = nullptr;
    size_t n_positions = 0;
    const RibbitOligo shorter{14, 0, 0};
    if (ribbit_host_record_oligo_sites("ACGT", 4, &shorter, 1, &bad, &sites, &positions, &n_positions) != RIBBIT_E_ARG) die("an oligo shorter than the seed was taken");
    std::printf("ok: %zu sites, %zu products, %zu rows as text\n", sites_seen, products_seen, n);
    return 0;
}
