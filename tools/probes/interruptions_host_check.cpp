// interruptions_host_check.cpp -- a stand-alone run of the host side of the CIGAR decode (ribbit_bed_cigars,
// ribbit_host_record_interruptions, ribbit_interruption_text, ribbit_bed_purity_text) for the sanitizers:
// `make -C ribbit_amd/csrc asan-interruptions-check` links it against the library's host code built with
// -fsanitize=address,undefined and runs it on the CPU.  It needs no GPU and prints "ok" when every result is what a second, naive
// computation gives.
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
    std::fprintf(stderr, "interruptions_host_check: %s: %s\n", what, ribbit_hip_last_error());
    std::exit(1);
}

}  // namespace

int main() {
    std::mt19937 rng(17);
    const char *units[] = {"CA", "AAT", "GATA", "ACGTT", "A"};
    const int lens[] = {1, 1, 2, 3, 5, 12, 82, 300};
    // enough rows for the BED text to be cut into pieces (4 MB each) and for both texts to be written in pieces
    const size_t n = 150000;
    const int64_t length = 3000000;      // (rows reach past it and start before 0)
    std::string sequence((size_t)length, 'A'), bed;
    for (char &c : sequence) c = "ACGTNacgtn"[rng() % 10];
    std::vector<int64_t> query(n);
    std::vector<int32_t> ks(n);
    for (size_t i = 0; i < n; ++i) {
        std::string cigar;
        int64_t q = 0;
        for (unsigned ops = rng() % 9; ops > 0; --ops) {
            const int len = lens[rng() % 8];
            const char c = "=X=I=DM"[rng() % 7];
            cigar += std::to_string(len) + c;
            if (c != 'D') q += len;
        }
        const char *unit = units[rng() % 5];
        const long s = (long)(rng() % 3000200) - 100, e = s + q + (rng() % 7 == 0 ? 1 : 0);      // (one row in seven is inconsistent)
        query[i] = q;
        ks[i] = (int32_t)std::strlen(unit);
        bed += "rec\twith a tab\t" + std::to_string(s) + "\t" + std::to_string(e) + "\t" + unit + "\t2|2\t7\t3.5\t0.9\t+\tP\t" + cigar + "\n";
    }
    bed.pop_back();      // (a last line without its newline)
    char *pool = nullptr, *observed = nullptr, *sites_text = nullptr, *rows_text = nullptr;
    int32_t *offsets = nullptr, *iv = nullptr, *observed_offsets = nullptr;
    RibbitRowPurity *rows = nullptr;
    RibbitInterruption *sites = nullptr;
    size_t n_rows = 0, n_iv = 0, n_sites = 0, len = 0, left_out = 0;
    if (ribbit_bed_cigars(bed.data(), bed.size(), &pool, &offsets, &n_rows) != RIBBIT_OK || n_rows != n) die("ribbit_bed_cigars");
    if (ribbit_bed_intervals(bed.data(), bed.size(), &iv, &n_iv) != RIBBIT_OK || n_iv != n) die("ribbit_bed_intervals");
    if (ribbit_host_record_interruptions(sequence.data(), length, iv, ks.data(), n, pool, offsets, &rows, &sites, &n_sites, &observed, &observed_offsets) != RIBBIT_OK)
        die("ribbit_host_record_interruptions");
    // naive: every row's numbers again from its interruptions
    size_t at = 0, inconsistent = 0, lines = 0;
    for (size_t i = 0; i < n; ++i) {
        const RibbitRowPurity &r = rows[i];
        if ((size_t)r.first != at || r.query != query[i]) { std::fprintf(stderr, "row %zu does not follow the one before\n", i); return 1; }
        int64_t x = 0, ins = 0, del = 0, behind = iv[2 * i], longest = 0;
        for (size_t j = at; j < at + (size_t)r.count; ++j) {
            const RibbitInterruption &k = sites[j];
            if ((size_t)k.row != i || k.start < behind || k.end - k.start != k.x + k.ins || k.cigar_at < offsets[i] || k.cigar_at + k.cigar_len > offsets[i + 1]) {
                std::fprintf(stderr, "interruption %zu differs\n", j);
                return 1;
            }
            longest = std::max<int64_t>(longest, k.start - behind);
            const int64_t a = std::min<int64_t>(std::max<int64_t>(k.start, 0), length), b = std::min<int64_t>(std::max<int64_t>(k.end, a), length);
            if (observed_offsets[j + 1] - observed_offsets[j] != b - a || std::memcmp(observed + observed_offsets[j], sequence.data() + a, (size_t)(b - a)) != 0) {
                std::fprintf(stderr, "interruption %zu: other bases\n", j);
                return 1;
            }
            x += k.x; ins += k.ins; del += k.del;
            behind = k.end;
        }
        longest = std::max<int64_t>(longest, iv[2 * i] + query[i] - behind);
        if (x != r.x || ins != r.ins || del != r.del || r.pure_end - r.pure_start != longest) { std::fprintf(stderr, "row %zu differs\n", i); return 1; }
        at += (size_t)r.count;
        const bool ok = (int64_t)iv[2 * i] + query[i] == iv[2 * i + 1];
        inconsistent += !ok;
        if (ok) lines += (size_t)r.count;
    }
    if (at != n_sites) { std::fprintf(stderr, "the rows hold %zu of %zu interruptions\n", at, n_sites); return 1; }
    if (ribbit_interruption_text("rec\twith a tab", bed.data(), bed.size(), iv, n, rows, sites, n_sites, pool, observed, observed_offsets, &sites_text, &len, &left_out) != RIBBIT_OK)
        die("ribbit_interruption_text");
    if (left_out != inconsistent || (size_t)std::count(sites_text, sites_text + len, '\n') != lines) { std::fprintf(stderr, "the interruptions' text has the wrong shape\n"); return 1; }
    if (ribbit_bed_purity_text(bed.data(), bed.size(), iv, ks.data(), rows, n, &rows_text, &len) != RIBBIT_OK) die("ribbit_bed_purity_text");
    if ((size_t)std::count(rows_text, rows_text + len, '\n') != n || (size_t)std::count(rows_text, rows_text + len, '.') < 3 * inconsistent) {
        std::fprintf(stderr, "the rows' text has the wrong shape\n");
        return 1;
    }
    // the argument errors
    char *none = nullptr;
    size_t k = 0;
    if (ribbit_bed_purity_text(bed.data(), bed.size() / 2, iv, ks.data(), rows, n, &none, &k) != RIBBIT_E_ARG) die("half a BED text was taken");
    if (n_sites) {
        RibbitInterruption bad = sites[0];
        bad.cigar_at = offsets[n];
        std::vector<RibbitInterruption> all(sites, sites + n_sites);
        all[0] = bad;
        if (ribbit_interruption_text("r", bed.data(), bed.size(), iv, n, rows, all.data(), n_sites, pool, observed, observed_offsets, &none, &k, &left_out) != RIBBIT_E_ARG)
            die("CIGAR bytes outside the pool were taken");
    }
    const int32_t one_row[2] = {0, 5}, one_k[1] = {2};
    RibbitRowPurity *r2 = nullptr;
    RibbitInterruption *s2 = nullptr;
    char *o2 = nullptr;
    int32_t *f2 = nullptr;
    for (const char *bad : {"5=1Y", "12=5", "=5=1", "00000000001=", "0=1X", "5= 1", "99999999999=", "2147483647=1D"}) {
        const int32_t two_offsets[2] = {0, (int32_t)std::strlen(bad)};
        if (ribbit_host_record_interruptions(sequence.data(), length, one_row, one_k, 1, bad, two_offsets, &r2, &s2, &k, &o2, &f2) != RIBBIT_E_ARG)
            die("a CIGAR that is to be refused was taken");
    }
    ribbit_text_free(pool);
    ribbit_text_free(observed);
    ribbit_text_free(sites_text);
    ribbit_text_free(rows_text);
    ribbit_intervals_free(offsets);
    ribbit_intervals_free(iv);
    ribbit_intervals_free(observed_offsets);
    ribbit_row_purity_free(rows);
    ribbit_interruptions_free(sites);
    std::printf("ok: %zu rows, %zu interruptions, %zu inconsistent rows\n", n, n_sites, inconsistent);
    return 0;
}
