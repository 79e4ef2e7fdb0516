// primer_specific_host_check.cpp -- a stand-alone run of the host side of the specific primer pairs
// (ribbit_host_record_specific_primer_pairs, ribbit_bed_primer_specific_text) for the sanitizers:
// `make -C ribbit_amd/csrc asan-primer-specific-check` links it against the library's host code built with
// -fsanitize=address,undefined and runs it on the CPU.  It needs no GPU and prints "ok" when every target's three records fit each
// other, every chosen pair is what ribbit_host_record_primer_pairs chooses where its place is 0, and its products are what
// ribbit_host_record_primer_products counts for it.
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
    std::fprintf(stderr, "primer_specific_host_check: %s: %s\n", what, ribbit_hip_last_error());
    std::exit(1);
}

[[noreturn]] void wrong(const char *what) {
    std::fprintf(stderr, "primer_specific_host_check: %s\n", what);
    std::exit(1);
}

}  // namespace

int main() {
    std::mt19937 rng(29);
    size_t first = 0, later = 0, none_of_some = 0, over = 0;
    for (const int64_t length : {0, 17, 40, 700, 2600}) {
        // mostly bases; the first third of the record a second time behind it, so that pairs there have other products
        std::string seq;
        for (int64_t i = 0; i < length; ++i) seq += "ACGTacgtACGTacgtACGTacgtACGTACGTACGTACGTNx"[rng() % 42];
        if (length >= 700) seq.replace((size_t)(length / 3), (size_t)(length / 3), seq.substr(0, (size_t)(length / 3)));
        std::vector<int32_t> rows, targets;
        for (int i = 0; i < 3; ++i) {
            const int32_t s = (int32_t)(rng() % (uint32_t)(length + 1));
            rows.push_back(s);
            rows.push_back(s + (int32_t)(rng() % 30));
        }
        for (int i = 0; i < 40; ++i) {
            const int32_t s = (int32_t)(rng() % (uint32_t)(length + 40)) - 20;
            targets.push_back(s);
            targets.push_back(s + (int32_t)(rng() % 60) - 3);
        }
        const size_t n_targets = targets.size() / 2;
        for (int variant = 0; variant < 3; ++variant) {
            RibbitPrimerParams prm;
            RibbitPrimerPairParams pair;
            RibbitProductParams product;
            ribbit_primer_params_default(&prm);
            ribbit_primer_pair_params_default(&pair);
            ribbit_product_params_default(&product);
            if (variant == 1) {
                prm.flank = 1000;
                pair.shortlist = 3;
                product.max_sites = 1;
            }
            if (variant == 2) {
                prm.flank = 60;
                pair = RibbitPrimerPairParams{8, 32, 32, 32, 32, 32, 2000};
                product = RibbitProductParams{15, 32, INT32_MAX, 1024};
            }
            RibbitRowPrimerPair *pairs = nullptr, *best = nullptr;
            RibbitRowProducts *products = nullptr, *again = nullptr;
            RibbitRowSpecific *specific = nullptr;
            if (ribbit_host_record_specific_primer_pairs(seq.data(), length, rows.data(), rows.size() / 2, targets.data(), n_targets, &prm, &pair, &product, &pairs, &products,
                                                         &specific) != RIBBIT_OK)
                die("ribbit_host_record_specific_primer_pairs");
            if (ribbit_host_record_primer_pairs(seq.data(), length, rows.data(), rows.size() / 2, targets.data(), n_targets, &prm, &pair, &best) != RIBBIT_OK)
                die("ribbit_host_record_primer_pairs");
            if (ribbit_host_record_primer_products(seq.data(), length, pairs, n_targets, &product, &again) != RIBBIT_OK) die("ribbit_host_record_primer_products");
            for (size_t i = 0; i < n_targets; ++i) {
                const RibbitRowSpecific &s = specific[i];
                const RibbitRowPrimerPair &r = pairs[i];
                if (s.pairs_admissible != s.pairs_specific + s.pairs_over + s.pairs_other || s.pairs_admissible != r.pairs_admissible || s.pairs_admissible > r.pairs_tried ||
                    s.pairs_admissible != best[i].pairs_admissible || s.reserved[0] || s.reserved[1])
                    wrong("counts that do not add up");
                if ((s.place >= 0) != (r.left.start >= 0) || (s.place >= 0) != (s.pairs_specific > 0) || s.place >= s.pairs_admissible) wrong("a place without a pair, or a pair without a place");
                if (std::memcmp(&products[i], &again[i], sizeof(RibbitRowProducts)) != 0) wrong("the products are not those of the chosen pair");
                if (s.place >= 0 && (products[i].products < 0 || products[i].products - products[i].own != 0)) wrong("a chosen pair that is not specific");
                if (s.place == 0 && std::memcmp(&r, &best[i], sizeof(RibbitRowPrimerPair)) != 0) wrong("place 0 is not the best pair");
                if (s.place > 0 && std::memcmp(&r, &best[i], 12 * sizeof(int32_t)) == 0) wrong("a later place holds the best pair");
                first += s.place == 0;
                later += s.place > 0;
                none_of_some += s.place < 0 && s.pairs_admissible > 0;
                over += s.pairs_over > 0;
            }
            std::string bed;
            for (size_t i = 0; i < n_targets; ++i) bed += "rec\t" + std::to_string(i) + "\t" + std::to_string(i + 9) + "\tCA\n";
            char *text = nullptr;
            size_t len = 0;
            if (ribbit_bed_primer_specific_text(bed.data(), bed.size(), pairs, products, specific, n_targets, &text, &len) != RIBBIT_OK) die("ribbit_bed_primer_specific_text");
            if ((size_t)std::count(text, text + len, '\n') != n_targets || (size_t)std::count(text, text + len, '\t') != (3 + 31) * n_targets) wrong("the text has the wrong shape");
            ribbit_text_free(text);
            ribbit_primer_specific_free(pairs);
            ribbit_primer_specific_free(products);
            ribbit_primer_specific_free(specific);
            ribbit_primer_pairs_free(best);
            ribbit_products_free(again);
        }
    }
    if (first < 10 || later + none_of_some < 3 || over < 3) {
        std::fprintf(stderr, "only %zu pairs in place 0, %zu later, %zu targets without a specific pair, %zu with a pair that is over\n", first, later, none_of_some, over);
        return 1;
    }
    // enough rows for the BED text to be cut into pieces, and the refusals
    const size_t n = 150000;
    std::string bed;
    std::vector<RibbitRowPrimerPair> pairs(n);
    std::vector<RibbitRowProducts> rows(n);
    std::vector<RibbitRowSpecific> sums(n);
    for (size_t i = 0; i < n; ++i) {
        bed += "rec\twith a tab\t" + std::to_string(i) + "\t" + std::to_string(i + 9) + "\tCA\t2|2\t9\t4.5\t0.9\t+\tP\t9=\n";
        RibbitRowPrimerPair &r = pairs[i];
        int32_t *fields = reinterpret_cast<int32_t *>(&r);
        for (int j = 12; j < 32; ++j) fields[j] = (int32_t)(rng() >> 1);
        r.left = RibbitPrimer{i % 3 ? (int32_t)i : -1, 1 + (int32_t)(rng() % 32), (int32_t)(rng() % 2001), 0, (int32_t)rng(), (int32_t)rng()};
        r.right = RibbitPrimer{i % 5 ? INT32_MAX - 32 : -1, 1 + (int32_t)(rng() % 32), -(int32_t)(rng() % 2001), 0, (int32_t)rng(), (int32_t)rng()};
        rows[i] = RibbitRowProducts{(int32_t)(rng() >> 1), (int32_t)(rng() >> 1), (int32_t)(rng() >> 1), (int32_t)(rng() >> 1), i % 7 ? (int32_t)(rng() >> 1) : -1, (int32_t)(i % 2),
                                    (int32_t)(rng() >> 1), 0};
        sums[i] = RibbitRowSpecific{i % 4 ? (int32_t)(rng() >> 1) : -1, (int32_t)(rng() >> 1), (int32_t)(rng() >> 1), (int32_t)(rng() >> 1), (int32_t)(rng() >> 1), -1, {0, 0}};
    }
    bed.pop_back();      // (a last line without its newline)
    char *text = nullptr, *none = nullptr;
    size_t len = 0;
    if (ribbit_bed_primer_specific_text(bed.data(), bed.size(), pairs.data(), rows.data(), sums.data(), n, &text, &len) != RIBBIT_OK) die("ribbit_bed_primer_specific_text");
    if ((size_t)std::count(text, text + len, '\n') != n || (size_t)std::count(text, text + len, '\t') != 42 * n) wrong("the long text has the wrong shape");
    ribbit_text_free(text);
    pairs[n - 1].left = RibbitPrimer{5, 33, 0, 0, 0, 0};
    pairs[n - 1].right.start = 7;
    if (ribbit_bed_primer_specific_text(bed.data(), bed.size(), pairs.data(), rows.data(), sums.data(), n, &none, &len) != RIBBIT_E_ARG) die("a primer of 33 bases was taken");
    if (ribbit_bed_primer_specific_text(bed.data(), bed.size() / 2, pairs.data(), rows.data(), sums.data(), n, &none, &len) != RIBBIT_E_ARG) die("half a BED text was taken");
    RibbitPrimerParams prm;
    RibbitPrimerPairParams pair;
    RibbitProductParams product;
    ribbit_primer_params_default(&prm);
    ribbit_primer_pair_params_default(&pair);
    ribbit_product_params_default(&product);
    const int32_t target[2] = {1, 3};
    RibbitRowPrimerPair *p = nullptr;
    RibbitRowProducts *q = nullptr;
    RibbitRowSpecific *s = nullptr;
    prm.min_length = 14;
    if (ribbit_host_record_specific_primer_pairs("ACGT", 4, nullptr, 0, target, 1, &prm, &pair, &product, &p, &q, &s) != RIBBIT_E_ARG) die("a min_length below the seed was taken");
    ribbit_primer_params_default(&prm);
    product.max_sites = 0;
    if (ribbit_host_record_specific_primer_pairs("ACGT", 4, nullptr, 0, target, 1, &prm, &pair, &product, &p, &q, &s) != RIBBIT_E_ARG) die("max_sites 0 was taken");
    std::printf("ok: %zu pairs in place 0, %zu later, %zu targets without a specific pair, %zu rows as text\n", first, later, none_of_some, n);
    return 0;
}
