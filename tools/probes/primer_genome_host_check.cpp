// primer_genome_host_check.cpp -- a stand-alone run of the host side of the genome-wide specific primer pairs
// (ribbit_host_record_primer_shortlists, ribbit_host_record_shortlist_verdicts, ribbit_primer_verdicts_merge,
// ribbit_primer_shortlists_choose, ribbit_bed_primer_specific_text) for the sanitizers:
// `make -C ribbit_amd/csrc asan-primer-genome-check` links it against the library's host code built with
// -fsanitize=address,undefined and runs it on the CPU.  It needs no GPU and prints "ok" when the three genomes whose values
// include/ribbit_hip.h pins (tests/golden/primer_genome_pinned.fa: the home record and the three forms of the other one; found
// beside this file's own path) give those values with either record first, when a genome of one record is
// ribbit_host_record_specific_primer_pairs byte for byte, and when what must be refused is refused.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "ribbit_hip.h"

namespace {

[[noreturn]] void die(const char *what) {
    std::fprintf(stderr, "primer_genome_host_check: %s: %s\n", what, ribbit_hip_last_error());
    std::exit(1);
}

[[noreturn]] void wrong(const char *what) {
    std::fprintf(stderr, "primer_genome_host_check: %s\n", what);
    std::exit(1);
}

struct Params {
    RibbitPrimerParams prm;
    RibbitPrimerPairParams pair;
    RibbitProductParams product;
    Params() {
        ribbit_primer_params_default(&prm);
        ribbit_primer_pair_params_default(&pair);
        ribbit_product_params_default(&product);
    }
};

struct Chosen {
    RibbitRowPrimerPair *pairs = nullptr;
    RibbitRowProducts *products = nullptr;
    RibbitRowSpecific *specific = nullptr;
    ~Chosen() {
        ribbit_primer_genome_free(pairs);
        ribbit_primer_genome_free(products);
        ribbit_primer_genome_free(specific);
    }
};

// twins -> merge -> choose for the targets of records[home]
void genome(const std::vector<std::string> &records, size_t home, const std::vector<int32_t> &targets, const Params &p, RibbitTargetShortlists **lists, Chosen &out) {
    const size_t n = targets.size() / 2;
    if (ribbit_host_record_primer_shortlists(records[home].data(), (int64_t)records[home].size(), nullptr, 0, targets.data(), n, &p.prm, &p.pair, lists) != RIBBIT_OK)
        die("ribbit_host_record_primer_shortlists");
    RibbitTargetVerdicts *sum = nullptr;
    for (size_t k = 0; k < records.size(); ++k) {
        RibbitTargetVerdicts *one = nullptr;
        if (ribbit_host_record_shortlist_verdicts(records[k].data(), (int64_t)records[k].size(), *lists, n, k == home, &p.pair, &p.product, &one) != RIBBIT_OK)
            die("ribbit_host_record_shortlist_verdicts");
        if (!sum) {
            sum = one;
            continue;
        }
        if (ribbit_primer_verdicts_merge(sum, one, n) != RIBBIT_OK) die("ribbit_primer_verdicts_merge");
        ribbit_primer_genome_free(one);
    }
    for (size_t i = 0; i < n; ++i)
        if (sum[i].records != (int32_t)records.size() || sum[i].home_records != 1 || sum[i].reserved != 0) wrong("the records were not counted");
    if (ribbit_primer_shortlists_choose(*lists, sum, n, &p.pair, &out.pairs, &out.products, &out.specific) != RIBBIT_OK) die("ribbit_primer_shortlists_choose");
    ribbit_primer_genome_free(sum);
}

}  // namespace

int main() {
    // the four records of the fixture, which lies two directories above this file and then under tests/golden
    std::string path = __FILE__;
    for (int up = 0; up < 3; ++up) path.erase(path.find_last_of('/'));
    path += "/tests/golden/primer_genome_pinned.fa";
    RibbitFastaReader *reader = nullptr;
    if (ribbit_fasta_open(path.c_str(), 0, &reader) != RIBBIT_OK) {
        std::fprintf(stderr, "primer_genome_host_check: %s\n", ribbit_fasta_last_error());
        return 1;
    }
    std::vector<std::string> records;
    for (;;) {
        const char *name = "", *bases = nullptr;
        int64_t length = 0;
        int is_last = 1;
        const int got = ribbit_fasta_next(reader, &name, &bases, &length, &is_last);
        if (got <= 0) break;
        records.emplace_back(bases, (size_t)length);
        ribbit_fasta_release(reader, bases);
        if (is_last) break;
    }
    ribbit_fasta_close(reader);
    if (records.size() != 4 || records[0].size() != 4000 || records[3].size() != 4000) wrong("the fixture does not hold four records of 4,000 bases");

    const Params p;
    const std::vector<int32_t> target{1500, 1540};
    // (place, pairs_admissible, pairs_specific, pairs_over, pairs_other, first_products), (left start, left length, right start, right length)
    const int32_t pinned[3][10] = {{0, 44, 44, 0, 0, 0, 1304, 22, 1624, 21}, {2, 44, 30, 0, 14, 1, 1304, 22, 1613, 22}, {-1, 44, 0, 0, 44, 1, -1, 0, -1, 0}};
    size_t lines = 0;
    for (int g = 0; g < 3; ++g)
        for (int home = 0; home < 2; ++home) {
            const std::vector<std::string> order = home == 0 ? std::vector<std::string>{records[0], records[1 + g]} : std::vector<std::string>{records[1 + g], records[0]};
            RibbitTargetShortlists *lists = nullptr;
            Chosen c;
            genome(order, (size_t)home, target, p, &lists, c);
            const RibbitRowSpecific &s = c.specific[0];
            const RibbitRowPrimerPair &r = c.pairs[0];
            const int32_t got[10] = {s.place, s.pairs_admissible, s.pairs_specific, s.pairs_over, s.pairs_other, s.first_products, r.left.start, r.left.length, r.right.start, r.right.length};
            if (std::memcmp(got, pinned[g], sizeof got) != 0) wrong("a pinned value is not what the header says");
            if ((s.place >= 0) != (c.products[0].own == 1) || c.products[0].products != c.products[0].own || c.products[0].shortest_other != 0) wrong("the chosen pair's products");
            char *text = nullptr;
            size_t len = 0;
            if (ribbit_bed_primer_specific_text("home\t1500\t1540\tCA", 17, c.pairs, c.products, c.specific, 1, &text, &len) != RIBBIT_OK) die("ribbit_bed_primer_specific_text");
            if (std::count(text, text + len, '\n') != 1 || std::count(text, text + len, '\t') != 3 + 31) wrong("the text has the wrong shape");
            lines += 1;
            ribbit_text_free(text);
            ribbit_primer_genome_free(lists);
        }
    // a genome of one record is the specific primer pairs of that record, byte for byte
    const std::vector<int32_t> targets{1500, 1540, 0, 30, 700, 730, 2600, 2640, 3990, 4000, -5, 3, 3000, 3025};
    const size_t n = targets.size() / 2;
    for (const std::string &record : records)
        for (int variant = 0; variant < 2; ++variant) {
            Params q;
            if (variant == 1) {
                q.prm.flank = 90;
                q.pair.shortlist = 3;
                q.product.max_sites = 1;
            }
            RibbitTargetShortlists *lists = nullptr;
            Chosen c, want;
            genome({record}, 0, targets, q, &lists, c);
            if (ribbit_host_record_specific_primer_pairs(record.data(), (int64_t)record.size(), nullptr, 0, targets.data(), n, &q.prm, &q.pair, &q.product, &want.pairs, &want.products,
                                                         &want.specific) != RIBBIT_OK)
                die("ribbit_host_record_specific_primer_pairs");
            if (std::memcmp(c.pairs, want.pairs, n * sizeof(RibbitRowPrimerPair)) != 0 || std::memcmp(c.products, want.products, n * sizeof(RibbitRowProducts)) != 0 ||
                std::memcmp(c.specific, want.specific, n * sizeof(RibbitRowSpecific)) != 0)
                wrong("a genome of one record is not the specific primer pairs of that record");
            ribbit_primer_genome_free(lists);
        }
    // the refusals
    RibbitTargetShortlists *lists = nullptr;
    if (ribbit_host_record_primer_shortlists(records[0].data(), 4000, nullptr, 0, target.data(), 1, &p.prm, &p.pair, &lists) != RIBBIT_OK) die("ribbit_host_record_primer_shortlists");
    RibbitTargetVerdicts *home = nullptr, *abroad = nullptr, *none = nullptr;
    if (ribbit_host_record_shortlist_verdicts(records[0].data(), 4000, lists, 1, 1, &p.pair, &p.product, &home) != RIBBIT_OK) die("ribbit_host_record_shortlist_verdicts");
    if (ribbit_host_record_shortlist_verdicts(records[1].data(), 4000, lists, 1, 0, &p.pair, &p.product, &abroad) != RIBBIT_OK) die("ribbit_host_record_shortlist_verdicts");
    Chosen refused;
    if (ribbit_primer_shortlists_choose(lists, abroad, 1, &p.pair, &refused.pairs, &refused.products, &refused.specific) != RIBBIT_E_ARG) die("verdicts without a home record were taken");
    RibbitTargetVerdicts twice = *home;
    if (ribbit_primer_verdicts_merge(&twice, home, 1) != RIBBIT_OK) die("ribbit_primer_verdicts_merge");
    if (ribbit_primer_shortlists_choose(lists, &twice, 1, &p.pair, &refused.pairs, &refused.products, &refused.specific) != RIBBIT_E_ARG) die("verdicts of two home records were taken");
    RibbitTargetVerdicts different = *abroad;
    different.admissible ^= 1;
    if (ribbit_primer_verdicts_merge(&twice, &different, 1) != RIBBIT_E_ARG) die("verdicts of other admissible pairs were summed");
    RibbitTargetShortlists gap = lists[0];
    gap.left[1].start = -1;
    if (ribbit_host_record_shortlist_verdicts(records[1].data(), 4000, &gap, 1, 0, &p.pair, &p.product, &none) != RIBBIT_E_ARG) die("a held place behind an empty one was taken");
    gap = lists[0];
    gap.right[0].length = 33;
    if (ribbit_host_record_shortlist_verdicts(records[1].data(), 4000, &gap, 1, 0, &p.pair, &p.product, &none) != RIBBIT_E_ARG) die("a primer of 33 bases was taken");
    ribbit_primer_genome_free(home);
    ribbit_primer_genome_free(abroad);
    ribbit_primer_genome_free(lists);
    std::printf("ok: three pinned genomes with either record first, %zu lines of text, %zu records as genomes of one\n", lines, records.size());
    return 0;
}
