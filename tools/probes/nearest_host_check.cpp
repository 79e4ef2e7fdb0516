// nearest_host_check.cpp -- a stand-alone run of the host side of the nearest intervals (ribbit_host_record_nearest,
// ribbit_bed_nearest_text, ribbit_nearest_other_text) for the sanitizers: `make -C ribbit_amd/csrc asan-nearest-check` links it
// against the library's host code built with -fsanitize=address,undefined and runs it on the CPU.  It needs no GPU and prints
// "ok" when every result is what a second, naive computation gives.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <tuple>
#include <vector>

#include "ribbit_hip.h"

namespace {

[[noreturn]] void die(const char *what) {
    std::fprintf(stderr, "nearest_host_check: %s: %s\n", what, ribbit_hip_last_error());
    std::exit(1);
}

// the contract as two nested loops
RibbitNearest naive(int64_t length, int32_t qs, int32_t qe, const std::vector<int32_t> &targets) {
    RibbitNearest r{RIBBIT_NEAREST_APART, -1, -1, -1, -1, -1};
    const int64_t s = std::max<int64_t>(qs, 0), e = std::min<int64_t>(qe, length);
    if (s >= e) return r;
    using Key = std::tuple<int64_t, int64_t, int64_t>;
    bool holds = false, meets = false, has_left = false, has_right = false;
    Key hold{}, meet{}, left{}, right{};
    for (size_t j = 0; j < targets.size() / 2; ++j) {
        const int64_t ts = std::max<int64_t>(targets[2 * j], 0), te = std::min<int64_t>(targets[2 * j + 1], length);
        if (ts >= te) continue;
        const Key a{ts, te, (int64_t)j}, b{te, ts, (int64_t)j}, reach{-te, ts, (int64_t)j};      // (the furthest end first, then order A)
        if (ts <= s && te >= e && (!holds || reach < hold)) { holds = true; hold = reach; }
        if (ts < e && te > s && (!meets || a < meet)) { meets = true; meet = a; }
        if (te <= s && (!has_left || b > left)) { has_left = true; left = b; }
        if (ts >= e && (!has_right || a < right)) { has_right = true; right = a; }
    }
    if (holds) { r.kind = RIBBIT_NEAREST_INSIDE; r.hit = (int32_t)std::get<2>(hold); }
    else if (meets) { r.kind = RIBBIT_NEAREST_OVER; r.hit = (int32_t)std::get<2>(meet); }
    if (has_left) { r.left = (int32_t)std::get<2>(left); r.left_dist = (int32_t)(s - std::get<0>(left)); }
    if (has_right) { r.right = (int32_t)std::get<2>(right); r.right_dist = (int32_t)(std::get<0>(right) - e); }
    return r;
}

}  // namespace

int main() {
    std::mt19937 rng(13);
    // small sets against the naive loops, at the record lengths of the tests
    size_t compared = 0;
    for (const int64_t length : {0, 1, 64, 1000}) {
        for (const size_t n_targets : {(size_t)0, (size_t)1, (size_t)2, (size_t)300}) {
            std::vector<int32_t> q, t;
            auto fill = [&](std::vector<int32_t> &iv, size_t n) {
                for (size_t i = 0; i < n; ++i) {
                    const int32_t s = (int32_t)(rng() % (uint32_t)(length + 7)) - 3;
                    iv.push_back(s);
                    iv.push_back(s + (int32_t)(rng() % 40) - 2);
                }
            };
            fill(q, 200);
            fill(t, n_targets);
            q.insert(q.end(), {INT32_MIN, INT32_MAX, INT32_MAX, INT32_MIN, 0, (int32_t)length});
            if (n_targets) t.insert(t.end(), {INT32_MIN, INT32_MAX, INT32_MAX, INT32_MIN});
            RibbitNearest *out = nullptr;
            if (ribbit_host_record_nearest(length, q.data(), q.size() / 2, t.data(), t.size() / 2, &out) != RIBBIT_OK) die("ribbit_host_record_nearest");
            for (size_t i = 0; i < q.size() / 2; ++i) {
                const RibbitNearest want = naive(length, q[2 * i], q[2 * i + 1], t);
                if (std::memcmp(&want, out + i, sizeof want) != 0) { std::fprintf(stderr, "length %lld, %zu targets: query %zu differs\n", (long long)length, t.size() / 2, i); return 1; }
                ++compared;
            }
            ribbit_nearest_free(out);
        }
    }
    // enough rows for the BED text to be cut into pieces (4 MB each): both texts, and the refusals
    const size_t n = 150000, m = 5000;
    const int64_t length = 3000000;
    std::string bed, labels;
    std::vector<int32_t> targets, label_at{0};
    for (size_t i = 0; i < n; ++i) {
        const long s = (long)(rng() % 3000200) - 100, e = s + (long)(rng() % 40) - 3;
        bed += "rec\twith a tab\t" + std::to_string(s) + "\t" + std::to_string(e) + "\tCA\t2|2\t" + std::to_string(e - s) + "\t" + std::to_string((e - s) / 2) +
               ".5\t0.9\t+\tP\t7=\n";
    }
    bed.pop_back();      // (a last line without its newline)
    for (size_t j = 0; j < m; ++j) {
        const int32_t s = (int32_t)(rng() % 3000200) - 100;
        targets.push_back(s);
        targets.push_back(s + (int32_t)(rng() % 2000) - 3);
        labels += j % 7 ? "gene " + std::to_string(j) : ".";
        label_at.push_back((int32_t)labels.size());
    }
    int32_t *iv = nullptr, *motif_at = nullptr;
    char *motifs = nullptr, *text = nullptr, *none = nullptr;
    size_t n_iv = 0, n_motifs = 0, len = 0;
    RibbitNearest *near = nullptr, *back = nullptr;
    if (ribbit_bed_intervals(bed.data(), bed.size(), &iv, &n_iv) != RIBBIT_OK || n_iv != n) die("ribbit_bed_intervals");
    if (ribbit_bed_motifs(bed.data(), bed.size(), &motifs, &motif_at, &n_motifs) != RIBBIT_OK || n_motifs != n) die("ribbit_bed_motifs");
    if (ribbit_host_record_nearest(length, iv, n, targets.data(), m, &near) != RIBBIT_OK) die("ribbit_host_record_nearest");
    if (ribbit_host_record_nearest(length, targets.data(), m, iv, n, &back) != RIBBIT_OK) die("ribbit_host_record_nearest, the other way round");
    if (ribbit_bed_nearest_text(bed.data(), bed.size(), near, n, targets.data(), labels.c_str(), label_at.data(), m, &text, &len) != RIBBIT_OK) die("ribbit_bed_nearest_text");
    if ((size_t)std::count(text, text + len, '\n') != n || (size_t)std::count(text, text + len, '\t') != 19 * n) { std::fprintf(stderr, "the rows' text has the wrong shape\n"); return 1; }
    ribbit_text_free(text);
    if (ribbit_nearest_other_text("rec\twith a tab", targets.data(), labels.c_str(), label_at.data(), m, back, iv, motifs, motif_at, n, &text, &len) != RIBBIT_OK)
        die("ribbit_nearest_other_text");
    if ((size_t)std::count(text, text + len, '\n') != m || (size_t)std::count(text, text + len, '\t') != 12 * m) { std::fprintf(stderr, "the intervals' text has the wrong shape\n"); return 1; }
    ribbit_text_free(text);
    // the argument errors
    RibbitNearest bad = near[n - 1];
    std::vector<RibbitNearest> changed(near, near + n);
    bad.hit = (int32_t)m;
    changed[n - 1] = bad;
    if (ribbit_bed_nearest_text(bed.data(), bed.size(), changed.data(), n, targets.data(), labels.c_str(), label_at.data(), m, &none, &len) != RIBBIT_E_ARG) die("a hit outside the targets was taken");
    bad = near[0];
    bad.kind = 3;
    changed[n - 1] = near[n - 1];
    changed[0] = bad;
    if (ribbit_bed_nearest_text(bed.data(), bed.size(), changed.data(), n, targets.data(), labels.c_str(), label_at.data(), m, &none, &len) != RIBBIT_E_ARG) die("a kind of 3 was taken");
    if (ribbit_bed_nearest_text(bed.data(), bed.size() / 2, near, n, targets.data(), labels.c_str(), label_at.data(), m, &none, &len) != RIBBIT_E_ARG) die("half a BED text was taken");
    std::vector<int32_t> beyond = label_at;
    beyond[m] += 1;
    if (ribbit_bed_nearest_text(bed.data(), bed.size(), near, n, targets.data(), labels.c_str(), beyond.data(), m, &none, &len) != RIBBIT_E_ARG) die("offsets that leave the pool were taken");
    if (ribbit_nearest_other_text("r", targets.data(), labels.c_str(), beyond.data(), m, back, iv, motifs, motif_at, n, &none, &len) != RIBBIT_E_ARG) die("offsets that leave the pool were taken");
    ribbit_nearest_free(near);
    ribbit_nearest_free(back);
    ribbit_intervals_free(iv);
    ribbit_intervals_free(motif_at);
    ribbit_text_free(motifs);
    std::printf("ok: %zu queries against the naive loops, %zu rows and %zu intervals as text\n", compared, n, m);
    return 0;
}
