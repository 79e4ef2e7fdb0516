// api_primer_products.cpp -- in-silico PCR on one record: the sites of oligos on either strand and the products of primer pairs
// among them (primer_products.hip); see api_internal.h for the map of the files behind include/ribbit_hip.h.  The GPU form reads
// the bit planes the load packed and nothing else of the record: the oligos go down through stage_down, the work buffer is carved
// by rb::ProductLayout, and two counts the device finds are read in the middle of a call (the unique oligos, which size the
// patterns' lists before the scan; the kept positions, which size what comes back), so those two buffers are the handle's own.
// After the copy back everything the device returned is checked.  search_sites is the site search itself, the one place that
// launches it: the two calls here take it with all of d_work as its room, the specific pairs, the shortlists' verdicts and the
// amplicons with a region of theirs, and site_batch is the rule by which those three cut their work into batches.
// The host twins work from the bytes of the sequence: every window of every oligo judged letter by letter, every pair of sites
// walked.  They have no packed words, do not make the oligos unique and share nothing with the kernels; HostOligoIndex is for the
// twins whose pairs share oligos.  The text needs no GPU.
#include "primers_host.h"

#include <string>

namespace {

static_assert(sizeof(RibbitRowProducts) == 32 && sizeof(RibbitProductParams) == 16 && sizeof(RibbitOligo) == 12 && sizeof(RibbitOligoSites) == 16, "8, 4, 3 and 4 ints");
constexpr int32_t MIN_SEED = 6, MAX_SEED = 16, MAX_MISMATCHES = 32, MAX_SITES = 1024;
constexpr size_t MAX_PAIRS = (size_t)1 << 24, MAX_OLIGO_SITES = (size_t)1 << 29;
constexpr size_t SITE_LIST_BYTES = (size_t)256 << 20, MAX_BATCH_SITES = (size_t)1 << 29;

uint64_t bases_of(int32_t lo, int32_t hi) { return (uint64_t)(uint32_t)hi << 32 | (uint32_t)lo; }

}  // namespace

namespace rbapi {

int check_primer_product_params(const RibbitProductParams *p) {
    if (!p) return fail(RIBBIT_E_ARG, "null argument");
    if (p->seed < MIN_SEED || p->seed > MAX_SEED) return fail(RIBBIT_E_ARG, "seed %d is outside %d .. %d", (int)p->seed, (int)MIN_SEED, (int)MAX_SEED);
    if (p->max_mismatches < 0 || p->max_mismatches > MAX_MISMATCHES) return fail(RIBBIT_E_ARG, "max_mismatches %d is outside 0 .. %d", (int)p->max_mismatches, (int)MAX_MISMATCHES);
    if (p->max_product < 1) return fail(RIBBIT_E_ARG, "max_product %d is below 1", (int)p->max_product);
    if (p->max_sites < 1 || p->max_sites > MAX_SITES) return fail(RIBBIT_E_ARG, "max_sites %d is outside 1 .. %d", (int)p->max_sites, (int)MAX_SITES);
    return RIBBIT_OK;
}

int check_product_pairs(const RibbitRowPrimerPair *pairs, size_t n, const RibbitProductParams *params) {
    if (!pairs && n > 0) return fail(RIBBIT_E_ARG, "null argument");
    if (const int rc = check_primer_product_params(params)) return rc;
    if (n > MAX_PAIRS) return fail(RIBBIT_E_ARG, "%zu pairs", n);
    for (size_t i = 0; i < n; ++i)
        if (has_pair(pairs[i]))
            for (const RibbitPrimer *p : {&pairs[i].left, &pairs[i].right})
                if (p->length < params->seed || p->length > RIBBIT_PRIMER_MAX_LENGTH)
                    return fail(RIBBIT_E_ARG, "pair %zu: a primer of %d bases, not seed %d .. %d", i, (int)p->length, (int)params->seed, RIBBIT_PRIMER_MAX_LENGTH);
    return RIBBIT_OK;
}

// the two oligos of a pair, 5' to 3': the left primer's bases, the reverse complement of the right primer's
void pair_oligos(const RibbitRowPrimerPair &r, RibbitOligo &a, RibbitOligo &b) {
    a = RibbitOligo{r.left.length, r.left.bases_lo, r.left.bases_hi};
    const uint64_t forward = bases_of(r.right.bases_lo, r.right.bases_hi);
    uint64_t q = 0;
    for (int32_t j = 0; j < r.right.length; ++j) q |= (3 - ((forward >> (2 * (r.right.length - 1 - j))) & 3)) << (2 * j);
    b = RibbitOligo{r.right.length, (int32_t)(uint32_t)q, (int32_t)(uint32_t)(q >> 32)};
}

int search_sites(RibbitHandle *h, const RibbitOligo *d_oligos, size_t n_oligos, size_t n_pairs, const RibbitProductParams &prm, uint8_t *product_work, size_t room_bytes,
                 bool use_filter, SiteSearch &out) {
    RibbitHandle::RowBufs &buf = h->rows;
    out.at = rb::products_layout((int64_t)n_oligos, (int64_t)n_pairs);
    if (out.at.bytes > room_bytes) return fail(RIBBIT_E_INTERNAL, "%zu oligos need %zu bytes, not the %zu set aside", n_oligos, out.at.bytes, room_bytes);
    HIP_TRY(rb::launch_product_uniques(d_oligos, (int64_t)n_oligos, prm, product_work, room_bytes, out.at, h->stream));
    HIP_TRY(hipMemcpyAsync(buf.h_product_header.p, product_work + out.at.header, sizeof(rb::ProductHeader), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    out.uniques = reinterpret_cast<const rb::ProductHeader *>(buf.h_product_header.p)->uniques;
    if (out.uniques < 1 || out.uniques > n_oligos) return fail(RIBBIT_E_INTERNAL, "%zu unique oligos of %zu", out.uniques, n_oligos);
    // the lists' room is fixed here, by the patterns, and does not grow with the sites the scan finds
    if (const int rc = buf.d_site_lists.ensure(2 * out.uniques * (size_t)prm.max_sites, true)) return rc;
    HIP_TRY(rb::launch_product_scan(h->planes(), (int64_t)n_oligos, (int64_t)out.uniques, prm, product_work, room_bytes, out.at, buf.d_site_lists.p, use_filter, h->stream));
    return RIBBIT_OK;
}

size_t site_batch(const RibbitHandle *h, size_t oligos_per_item, const RibbitProductParams &prm) {
    const size_t per_item = oligos_per_item * (size_t)prm.max_sites;      // the list slots of an item's patterns of one strand
    const size_t by_rule = std::max<size_t>(1, SITE_LIST_BYTES / (2 * per_item * sizeof(int32_t)));
    return std::min(h->rows.specific_batch ? h->rows.specific_batch : by_rule, std::max<size_t>(1, MAX_BATCH_SITES / per_item));
}

}  // namespace rbapi

namespace {

int check_oligos(const RibbitOligo *oligos, size_t n, const RibbitProductParams *params) {
    if (!oligos && n > 0) return fail(RIBBIT_E_ARG, "null argument");
    if (const int rc = check_primer_product_params(params)) return rc;
    if (n > MAX_OLIGO_SITES / (size_t)params->max_sites) return fail(RIBBIT_E_ARG, "%zu oligos at max_sites %d", n, (int)params->max_sites);
    for (size_t i = 0; i < n; ++i)
        if (oligos[i].length < params->seed || oligos[i].length > RIBBIT_PRIMER_MAX_LENGTH)
            return fail(RIBBIT_E_ARG, "oligo %zu: %d bases, not seed %d .. %d", i, (int)oligos[i].length, (int)params->seed, RIBBIT_PRIMER_MAX_LENGTH);
    return RIBBIT_OK;
}

// ---- the GPU side: the oligos down and searched; -> the layout and the lists, ready for either result
int scan_oligos(RibbitHandle *h, const StageSegment *segs, size_t n_segs, const uint8_t **d_at, size_t n_oligos, size_t n_pairs, const RibbitProductParams &prm, SiteSearch &sc) {
    RibbitHandle::RowBufs &buf = h->rows;
    int rc;
    if ((rc = bind_device(h))) return rc;
    if ((rc = buf.d_work.ensure(rb::products_layout((int64_t)n_oligos, (int64_t)n_pairs).bytes, true))) return rc;
    if ((rc = buf.h_product_header.ensure(sizeof(rb::ProductHeader) / sizeof(uint32_t)))) return rc;
    if ((rc = stage_down(h, segs, n_segs, d_at))) return rc;
    // RIBBIT_PRODUCTS_NO_FILTER=1: the scan without the hashed bitmap in front of the bisection (tools/primer_products_timing.py measures both)
    static const bool no_filter = std::getenv("RIBBIT_PRODUCTS_NO_FILTER") && std::atoi(std::getenv("RIBBIT_PRODUCTS_NO_FILTER")) != 0;
    return search_sites(h, reinterpret_cast<const RibbitOligo *>(d_at[0]), n_oligos, n_pairs, prm, buf.d_work.p, buf.d_work.cap, !no_filter, sc);
}

int record_oligo_sites_impl(RibbitHandle *h, const RibbitOligo *oligos, size_t n, const RibbitProductParams *params, const RibbitOligoSites **sites,
                            const int32_t **positions, size_t *n_positions) {
    if (!h) return fail(RIBBIT_E_ARG, "null handle");
    if (!sites || !positions || !n_positions) return fail(RIBBIT_E_ARG, "null argument");
    int rc;
    if ((rc = check_oligos(oligos, n, params))) return rc;
    if (!h->loaded) return fail(RIBBIT_E_STATE, "no record loaded");
    RibbitHandle::RowBufs &buf = h->rows;
    if ((rc = buf.h_products.ensure(std::max<size_t>(n, 1) * sizeof(RibbitOligoSites), true))) return rc;
    if ((rc = buf.h_site_positions.ensure(1))) return rc;
    RibbitOligoSites *out = reinterpret_cast<RibbitOligoSites *>(buf.h_products.p);
    *sites = out;
    *positions = buf.h_site_positions.p;
    *n_positions = 0;
    if (n == 0) return RIBBIT_OK;
    const int64_t length = h->length;
    if (length == 0) {      // (no window fits)
        std::fill(out, out + n, RibbitOligoSites{0, 0, 0, 0});
        return RIBBIT_OK;
    }
    const StageSegment down{oligos, n * sizeof(RibbitOligo)};
    const uint8_t *d_oligos = nullptr;
    SiteSearch sc;
    if ((rc = scan_oligos(h, &down, 1, &d_oligos, n, 0, *params, sc))) return rc;
    HIP_TRY(rb::launch_oligo_sites((int64_t)n, *params, buf.d_work.p, buf.d_work.cap, sc.at, h->stream));
    HIP_TRY(hipMemcpyAsync(buf.h_product_header.p, buf.d_work.p + sc.at.header, sizeof(rb::ProductHeader), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipMemcpyAsync(out, buf.d_work.p + sc.at.out, n * sizeof(RibbitOligoSites), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    const size_t total = reinterpret_cast<const rb::ProductHeader *>(buf.h_product_header.p)->positions;
    if (total > 2 * n * (size_t)params->max_sites) return fail(RIBBIT_E_INTERNAL, "%zu positions of %zu oligos", total, n);
    if ((rc = buf.h_site_positions.ensure(std::max<size_t>(total, 1), true))) return rc;
    *positions = buf.h_site_positions.p;
    if (total > 0) {
        if ((rc = buf.d_site_flat.ensure(total, true))) return rc;
        rb::launch_site_gather((int64_t)n, *params, buf.d_work.p, sc.at, buf.d_site_lists.p, buf.d_site_flat.p, h->stream);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(buf.h_site_positions.p, buf.d_site_flat.p, total * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));
    }
    // what the device returned: counts, where the lists lie, and every list inside [0, L - k] and ascending
    size_t at = 0;
    for (size_t i = 0; i < n; ++i) {
        const RibbitOligoSites &s = out[i];
        const struct { int32_t count, from; } lists[2] = {{s.forward, s.forward_at}, {s.reverse, s.reverse_at}};
        for (const auto &l : lists) {
            const bool kept = l.count >= 0 && l.count <= params->max_sites;
            if (l.count < 0 || l.count > length || (kept ? (size_t)l.from != at || l.from < 0 : l.from != -1)) return fail(RIBBIT_E_INTERNAL, "oligo %zu: the sites the GPU counted do not add up", i);
            if (!kept) continue;
            for (int32_t j = 0; j < l.count; ++j) {
                const int32_t x = buf.h_site_positions.p[at + (size_t)j];
                if (x < 0 || (int64_t)x + oligos[i].length > length || (j > 0 && x <= buf.h_site_positions.p[at + (size_t)j - 1]))
                    return fail(RIBBIT_E_INTERNAL, "oligo %zu: a site the GPU found lies outside the record or out of order", i);
            }
            at += (size_t)l.count;
        }
    }
    if (at != total) return fail(RIBBIT_E_INTERNAL, "%zu positions, not the %zu of the lists", total, at);
    *n_positions = total;
    return RIBBIT_OK;
}

int record_primer_products_impl(RibbitHandle *h, const RibbitRowPrimerPair *pairs, size_t n, const RibbitProductParams *params, const RibbitRowProducts **rows) {
    if (!h) return fail(RIBBIT_E_ARG, "null handle");
    if (!rows) return fail(RIBBIT_E_ARG, "null argument");
    int rc;
    if ((rc = check_product_pairs(pairs, n, params))) return rc;
    if (!h->loaded) return fail(RIBBIT_E_STATE, "no record loaded");
    RibbitHandle::RowBufs &buf = h->rows;
    if ((rc = buf.h_products.ensure(std::max<size_t>(n, 1) * sizeof(RibbitRowProducts), true))) return rc;
    RibbitRowProducts *out = reinterpret_cast<RibbitRowProducts *>(buf.h_products.p);
    *rows = out;
    if (n == 0) return RIBBIT_OK;
    const int64_t length = h->length;
    // the oligos of the pairs that have any, two each, and for every pair {a's oligo, b's oligo, left.start, right.start}
    std::vector<RibbitOligo> oligos;
    std::vector<int32_t> quads(4 * n, -1);
    for (size_t i = 0; i < n; ++i) {
        if (!has_pair(pairs[i])) continue;
        RibbitOligo a, b;
        pair_oligos(pairs[i], a, b);
        quads[4 * i] = (int32_t)oligos.size();
        quads[4 * i + 1] = (int32_t)oligos.size() + 1;
        quads[4 * i + 2] = pairs[i].left.start;
        quads[4 * i + 3] = pairs[i].right.start;
        oligos.push_back(a);
        oligos.push_back(b);
    }
    if (length == 0 || oligos.empty()) {
        std::fill(out, out + n, RibbitRowProducts{});
        return RIBBIT_OK;
    }
    const StageSegment down[2] = {{oligos.data(), oligos.size() * sizeof(RibbitOligo)}, {quads.data(), quads.size() * sizeof(int32_t)}};
    const uint8_t *d_at[2] = {nullptr, nullptr};
    SiteSearch sc;
    if ((rc = scan_oligos(h, down, 2, d_at, oligos.size(), n, *params, sc))) return rc;
    HIP_TRY(rb::launch_pair_products(reinterpret_cast<const int32_t *>(d_at[1]), (int64_t)n, *params, buf.d_work.p, buf.d_work.cap, sc.at, buf.d_site_lists.p, h->stream));
    HIP_TRY(hipMemcpyAsync(out, buf.d_work.p + sc.at.out, n * sizeof(RibbitRowProducts), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    for (size_t i = 0; i < n; ++i) {
        const RibbitRowProducts &r = out[i];
        bool good = true;
        for (const int32_t c : {r.left_forward, r.left_reverse, r.right_forward, r.right_reverse}) good = good && c >= 0 && c <= length;
        const bool over = std::max(std::max(r.left_forward, r.left_reverse), std::max(r.right_forward, r.right_reverse)) > params->max_sites;
        good = good && r.reserved == 0 && r.own >= 0 && r.own <= 1 && r.shortest_other >= 0 && r.shortest_other <= params->max_product;
        good = good && (over ? r.products == -1 && r.own == 0 && r.shortest_other == 0 : r.products >= r.own && (r.shortest_other > 0) <= (r.products > r.own));
        if (!has_pair(pairs[i])) good = good && r.left_forward + r.left_reverse + r.right_forward + r.right_reverse + r.products == 0;
        if (!good) return fail(RIBBIT_E_INTERNAL, "pair %zu: the products the GPU counted do not add up", i);
    }
    return RIBBIT_OK;
}

// ---- the host twins, in letters
std::string letters_of(const RibbitOligo &o) {
    const uint64_t bases = bases_of(o.bases_lo, o.bases_hi);
    std::string out;
    for (int32_t j = 0; j < o.length; ++j) out += "ACGT"[(bases >> (2 * j)) & 3];
    return out;
}

// pattern at the window [x, x + k): its exact part [from, to) and at most d mismatches elsewhere, no byte of kind `other`
bool window_holds(const unsigned char *seq, int64_t x, const std::string &pattern, size_t from, size_t to, int32_t d) {
    for (size_t j = from; j < to; ++j)
        if (letter_at(seq, x + (int64_t)j) != pattern[j]) return false;
    int32_t mismatches = 0;
    for (size_t j = 0; j < pattern.size(); ++j) {
        if (j >= from && j < to) continue;
        const char c = letter_at(seq, x + (int64_t)j);
        if (!c) return false;
        mismatches += c != pattern[j];
    }
    return mismatches <= d;
}

struct Site { int64_t x, k; bool of_a; };

}  // namespace

namespace rbapi {

void host_pair_oligos(const RibbitRowPrimerPair &pair, std::string &a, std::string &b) {
    RibbitOligo oa, ob;
    pair_oligos(pair, oa, ob);
    a = letters_of(oa);
    b = letters_of(ob);
}

HostSites host_oligo_sites(const unsigned char *seq, int64_t length, const std::string &o, const RibbitProductParams &prm) {
    HostSites out;
    const std::string q = reverse_complement(o);
    const size_t k = o.size(), s = (size_t)prm.seed;
    for (int64_t x = 0; x + (int64_t)k <= length; ++x) {
        if (window_holds(seq, x, o, k - s, k, prm.max_mismatches)) out.forward.push_back((int32_t)x);
        if (window_holds(seq, x, q, 0, s, prm.max_mismatches)) out.reverse.push_back((int32_t)x);
    }
    return out;
}

size_t HostOligoIndex::add(const std::string &oligo) {
    const auto at = ids.emplace(oligo, distinct.size());
    if (at.second) distinct.push_back(&at.first->first);
    return at.first->second;
}

void HostOligoIndex::search(const unsigned char *seq, int64_t length, const RibbitProductParams &prm) {
    found.assign(distinct.size(), HostSites{});
    const unsigned threads = (unsigned)std::max<size_t>(1, std::min<size_t>(rb::host_thread_count(0), distinct.size()));
    rb::over_pieces(distinct.size(), threads, [&](size_t lo, size_t hi, unsigned) {
        for (size_t k = lo; k < hi; ++k) found[k] = host_oligo_sites(seq, length, *distinct[k], prm);
    });
}

// the products among the sites a and b of a pair's two oligos of ka and kb bases, whose own product is (a forward at left_start, b
// reverse at right_start)
RibbitRowProducts host_products_among(const HostSites &a, const HostSites &b, int32_t ka, int32_t kb, int32_t left_start, int32_t right_start, const RibbitProductParams &prm) {
    RibbitRowProducts r{};
    r.left_forward = (int32_t)a.forward.size();
    r.left_reverse = (int32_t)a.reverse.size();
    r.right_forward = (int32_t)b.forward.size();
    r.right_reverse = (int32_t)b.reverse.size();
    if (std::max(std::max(r.left_forward, r.left_reverse), std::max(r.right_forward, r.right_reverse)) > prm.max_sites) {
        r.products = -1;
        return r;
    }
    std::vector<Site> forward, reverse;
    for (const int32_t x : a.forward) forward.push_back(Site{x, ka, true});
    for (const int32_t x : b.forward) forward.push_back(Site{x, kb, false});
    for (const int32_t x : a.reverse) reverse.push_back(Site{x, ka, true});
    for (const int32_t x : b.reverse) reverse.push_back(Site{x, kb, false});
    int64_t shortest = 0;
    for (const Site &f : forward)
        for (const Site &v : reverse) {
            const int64_t size = v.x + v.k - f.x;
            if (f.x + f.k > v.x || size > prm.max_product) continue;
            ++r.products;
            if (f.of_a && !v.of_a && f.x == left_start && v.x == right_start) r.own = 1;
            else if (shortest == 0 || size < shortest) shortest = size;
        }
    r.shortest_other = (int32_t)shortest;
    return r;
}

}  // namespace rbapi

namespace {

int host_record_oligo_sites_impl(const char *sequence, int64_t length, const RibbitOligo *oligos, size_t n, const RibbitProductParams *params, RibbitOligoSites **sites,
                                 int32_t **positions, size_t *n_positions) {
    if (!sites || !positions || !n_positions) return fail(RIBBIT_E_ARG, "null argument");
    int rc;
    if ((rc = check_oligos(oligos, n, params))) return rc;
    if ((rc = check_sequence(sequence, length))) return rc;
    const unsigned char *seq = reinterpret_cast<const unsigned char *>(sequence);
    const RibbitProductParams prm = *params;
    std::vector<HostSites> found(n);
    const unsigned threads = (unsigned)std::max<size_t>(1, std::min<size_t>(rb::host_thread_count(0), n));
    rb::over_pieces(n, threads, [&](size_t lo, size_t hi, unsigned) {
        for (size_t i = lo; i < hi; ++i) found[i] = host_oligo_sites(seq, length, letters_of(oligos[i]), prm);
    });
    Handed<RibbitOligoSites> out;
    if ((rc = hand_out<RibbitOligoSites>(nullptr, n, false, out))) return rc;
    std::vector<int32_t> flat;
    for (size_t i = 0; i < n; ++i) {
        RibbitOligoSites &s = out[i];
        s = RibbitOligoSites{(int32_t)found[i].forward.size(), (int32_t)found[i].reverse.size(), -1, -1};
        if (s.forward <= prm.max_sites) {
            s.forward_at = (int32_t)flat.size();
            flat.insert(flat.end(), found[i].forward.begin(), found[i].forward.end());
        }
        if (s.reverse <= prm.max_sites) {
            s.reverse_at = (int32_t)flat.size();
            flat.insert(flat.end(), found[i].reverse.begin(), found[i].reverse.end());
        }
    }
    Handed<int32_t> pos;
    if ((rc = hand_out<int32_t>(flat.data(), flat.size(), false, pos))) return rc;
    *sites = out.release();
    *positions = pos.release();
    *n_positions = flat.size();
    return RIBBIT_OK;
}

RibbitRowProducts products_of(const unsigned char *seq, int64_t length, const RibbitRowPrimerPair &pair, const RibbitProductParams &prm) {
    if (!has_pair(pair)) return RibbitRowProducts{};
    std::string oa, ob;
    host_pair_oligos(pair, oa, ob);
    return host_products_among(host_oligo_sites(seq, length, oa, prm), host_oligo_sites(seq, length, ob, prm), pair.left.length, pair.right.length, pair.left.start,
                               pair.right.start, prm);
}

int host_record_primer_products_impl(const char *sequence, int64_t length, const RibbitRowPrimerPair *pairs, size_t n, const RibbitProductParams *params,
                                     RibbitRowProducts **rows) {
    if (!rows) return fail(RIBBIT_E_ARG, "null argument");
    int rc;
    if ((rc = check_product_pairs(pairs, n, params))) return rc;
    if ((rc = check_sequence(sequence, length))) return rc;
    const unsigned char *seq = reinterpret_cast<const unsigned char *>(sequence);
    const RibbitProductParams prm = *params;
    Handed<RibbitRowProducts> out;
    if ((rc = hand_out<RibbitRowProducts>(nullptr, n, false, out))) return rc;
    const unsigned threads = (unsigned)std::max<size_t>(1, std::min<size_t>(rb::host_thread_count(0), n));
    rb::over_pieces(n, threads, [&](size_t lo, size_t hi, unsigned) {
        for (size_t i = lo; i < hi; ++i) out[i] = products_of(seq, length, pairs[i], prm);
    });
    *rows = out.release();
    return RIBBIT_OK;
}

// ---- the text
int bed_primer_products_text_impl(const char *bed, size_t bed_len, const RibbitRowPrimerPair *pairs, const RibbitRowProducts *products, size_t n, char **text, size_t *len) {
    if (!text || !len || (!bed && bed_len > 0) || ((!pairs || !products) && n > 0)) return fail(RIBBIT_E_ARG, "null argument");
    return bed_pair_rows_text(bed, bed_len, pairs, n, "the rows' primer products", 256, text, len, [&](std::string &out, size_t i) { put_product_columns(out, pairs[i], products[i]); });
}

}  // namespace

extern "C" {

void ribbit_product_params_default(RibbitProductParams *params) {
    if (params) *params = RibbitProductParams{15, 2, 4000, 64};
}

int ribbit_hip_record_oligo_sites(RibbitHandle *h, const RibbitOligo *oligos, size_t n, const RibbitProductParams *params, const RibbitOligoSites **sites,
                                  const int32_t **positions, size_t *n_positions) {
    return guarded("the oligos' sites", [&]() -> int { return record_oligo_sites_impl(h, oligos, n, params, sites, positions, n_positions); });
}

int ribbit_host_record_oligo_sites(const char *sequence, int64_t length, const RibbitOligo *oligos, size_t n, const RibbitProductParams *params, RibbitOligoSites **sites,
                                   int32_t **positions, size_t *n_positions) {
    return guarded("the oligos' sites", [&]() -> int { return host_record_oligo_sites_impl(sequence, length, oligos, n, params, sites, positions, n_positions); });
}

int ribbit_hip_record_primer_products(RibbitHandle *h, const RibbitRowPrimerPair *pairs, size_t n, const RibbitProductParams *params, const RibbitRowProducts **rows) {
    return guarded("the primer products", [&]() -> int { return record_primer_products_impl(h, pairs, n, params, rows); });
}

int ribbit_host_record_primer_products(const char *sequence, int64_t length, const RibbitRowPrimerPair *pairs, size_t n, const RibbitProductParams *params,
                                       RibbitRowProducts **rows) {
    return guarded("the primer products", [&]() -> int { return host_record_primer_products_impl(sequence, length, pairs, n, params, rows); });
}

void ribbit_products_free(void *from_a_host_twin) { std::free(from_a_host_twin); }

int ribbit_bed_primer_products_text(const char *bed_text, size_t bed_len, const RibbitRowPrimerPair *pairs, const RibbitRowProducts *products, size_t n, char **text,
                                    size_t *len) {
    return guarded("the rows' primer products as text", [&]() -> int { return bed_primer_products_text_impl(bed_text, bed_len, pairs, products, n, text, len); });
}

}  // extern "C"
