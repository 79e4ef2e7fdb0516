// api_panel.cpp -- primer pairs pooled into multiplex PCR panels (panel.hip); see api_internal.h for the map of the files behind
// include/ribbit_hip.h.  The GPU form reads no record and needs none loaded: the pairs and the optional extra ints go down through
// stage_down, three launches fill regions of the handle's work buffer by rb::PanelLayout (the conflict matrix and the degrees, the
// order, the first fit), and only the header and the rows come back; the matrix (512 MiB at the cap) stays on the device, except
// for ribbit_hip_debug_panel_conflicts, which copies a small one to the caller.  After the copy back everything the device
// returned is checked.  With RIBBIT_PROFILE set, HIP events around the three launches are printed.
// The host twin works in letters: the four duplexes of two pairs through the duplex behind ribbit_host_oligo_duplex
// (primers_host.h), a byte per (i, j) and rule, the degrees, a stable sort and the first fit over lists of members.  It shares
// nothing with the kernels.  The text needs no GPU.
#include "primers_host.h"

#include <charconv>
#include <string>

namespace {

static_assert(sizeof(RibbitPanelRow) == 32 && sizeof(RibbitPanelParams) == 20 && sizeof(RibbitRowPrimerPair) == 128, "8, 5 and 32 ints");
constexpr int32_t MAX_LIMIT = 32, MAX_SIZE_GAP = 100000, MAX_CROSS_PRODUCT = 1 << 30, MAX_POOL_SIZE = 65536;
enum : uint8_t { DIMER = 1, SIZE = 2, NEAR = 4 };

int check_params(const RibbitPanelParams *p) {
    if (!p) return fail(RIBBIT_E_ARG, "null argument");
    if (p->max_cross_any < 0 || p->max_cross_any > MAX_LIMIT) return fail(RIBBIT_E_ARG, "max_cross_any %d is outside 0 .. %d", (int)p->max_cross_any, (int)MAX_LIMIT);
    if (p->max_cross_end < 0 || p->max_cross_end > MAX_LIMIT) return fail(RIBBIT_E_ARG, "max_cross_end %d is outside 0 .. %d", (int)p->max_cross_end, (int)MAX_LIMIT);
    if (p->size_gap < 0 || p->size_gap > MAX_SIZE_GAP) return fail(RIBBIT_E_ARG, "size_gap %d is outside 0 .. %d", (int)p->size_gap, (int)MAX_SIZE_GAP);
    if (p->max_cross_product < 0 || p->max_cross_product > MAX_CROSS_PRODUCT)
        return fail(RIBBIT_E_ARG, "max_cross_product %d is outside 0 .. %d", (int)p->max_cross_product, (int)MAX_CROSS_PRODUCT);
    if (p->pool_size < 1 || p->pool_size > MAX_POOL_SIZE) return fail(RIBBIT_E_ARG, "pool_size %d is outside 1 .. %d", (int)p->pool_size, (int)MAX_POOL_SIZE);
    return RIBBIT_OK;
}

int check_args(const RibbitRowPrimerPair *pairs, const int32_t *extra, size_t n, const RibbitPanelParams *params, size_t cap) {
    if (!pairs && n > 0) return fail(RIBBIT_E_ARG, "null argument");
    if (const int rc = check_params(params)) return rc;
    if (n > cap) return fail(RIBBIT_E_ARG, "%zu pairs (at most %zu)", n, cap);
    for (size_t i = 0; i < n; ++i) {
        if (has_pair(pairs[i]))
            for (const RibbitPrimer *p : {&pairs[i].left, &pairs[i].right})
                if (p->length < 1 || p->length > RIBBIT_PRIMER_MAX_LENGTH)
                    return fail(RIBBIT_E_ARG, "pair %zu: a primer of %d bases, not 1 .. %d", i, (int)p->length, RIBBIT_PRIMER_MAX_LENGTH);
        if (!extra) continue;
        if (extra[3 * i] < -1) return fail(RIBBIT_E_ARG, "pair %zu: group %d is below -1", i, (int)extra[3 * i]);
        if (extra[3 * i + 1] > extra[3 * i + 2]) return fail(RIBBIT_E_ARG, "pair %zu: size_lo %d is above size_hi %d", i, (int)extra[3 * i + 1], (int)extra[3 * i + 2]);
    }
    return RIBBIT_OK;
}

struct StageEvents {
    OwnedEvent at[4];
    bool on = false;
    int start() {
        on = rb::profile_on();
        for (OwnedEvent &e : at)
            if (on) HIP_TRY(e.create());
        return RIBBIT_OK;
    }
    int mark(int k, hipStream_t stream) {
        if (on) HIP_TRY(hipEventRecord(at[k], stream));
        return RIBBIT_OK;
    }
    void print(size_t n) {
        if (!on) return;
        float ms[3] = {0, 0, 0};
        for (int k = 0; k < 3; ++k) (void)hipEventElapsedTime(&ms[k], at[k], at[k + 1]);
        std::fprintf(stderr, "[panel] pairs %zu matrix_ms %.3f order_ms %.3f first_fit_ms %.3f\n", n, ms[0], ms[1], ms[2]);
    }
};

// the launches of a panel of n >= 1 pairs on the handle's stream, up to `stages` of the three; -> the layout they filled in rows.d_work
int enqueue_panel(RibbitHandle *h, const RibbitRowPrimerPair *pairs, const int32_t *extra, size_t n, const RibbitPanelParams &prm, int stages, StageEvents &ev,
                  rb::PanelLayout &at) {
    RibbitHandle::RowBufs &buf = h->rows;
    int rc;
    if ((rc = bind_device(h))) return rc;
    at = rb::panel_layout((int64_t)n);
    if ((rc = buf.d_work.ensure(at.bytes, true))) return rc;
    const StageSegment down[2] = {{pairs, n * sizeof(RibbitRowPrimerPair)}, {extra, extra ? 3 * n * sizeof(int32_t) : 0}};
    const uint8_t *d_at[2] = {nullptr, nullptr};
    if ((rc = stage_down(h, down, 2, d_at))) return rc;
    if ((rc = ev.start())) return rc;
    if ((rc = ev.mark(0, h->stream))) return rc;
    HIP_TRY(rb::launch_panel_conflicts(reinterpret_cast<const RibbitRowPrimerPair *>(d_at[0]), extra ? reinterpret_cast<const int32_t *>(d_at[1]) : nullptr, (int64_t)n, prm,
                                       buf.d_work.p, buf.d_work.cap, at, h->stream));
    if ((rc = ev.mark(1, h->stream))) return rc;
    if (stages < 2) return RIBBIT_OK;
    HIP_TRY(rb::launch_panel_order((int64_t)n, buf.d_work.p, buf.d_work.cap, at, h->stream));
    if ((rc = ev.mark(2, h->stream))) return rc;
    HIP_TRY(rb::launch_panel_first_fit((int64_t)n, prm, buf.d_work.p, buf.d_work.cap, at, h->stream));
    return ev.mark(3, h->stream);
}

int panel_pools_impl(RibbitHandle *h, const RibbitRowPrimerPair *pairs, const int32_t *extra, size_t n, const RibbitPanelParams *params, const RibbitPanelRow **rows,
                     int32_t *n_pools) {
    if (!h) return fail(RIBBIT_E_ARG, "null handle");
    if (!rows || !n_pools) return fail(RIBBIT_E_ARG, "null argument");
    *rows = nullptr;      // (both are the answer's only when the call succeeds)
    *n_pools = 0;
    int rc;
    if ((rc = check_args(pairs, extra, n, params, RIBBIT_PANEL_MAX_PAIRS))) return rc;
    RibbitHandle::RowBufs &buf = h->rows;
    const size_t head = sizeof(RibbitPanelRow);      // (the header's room, so that the rows stay aligned)
    static_assert(sizeof(rb::PanelHeader) <= sizeof(RibbitPanelRow), "the header fits a row's room");
    if ((rc = buf.h_panel.ensure(head + std::max<size_t>(n, 1) * sizeof(RibbitPanelRow), true))) return rc;
    RibbitPanelRow *out = reinterpret_cast<RibbitPanelRow *>(buf.h_panel.p + head);
    if (n == 0) {
        *rows = out;
        return RIBBIT_OK;
    }
    StageEvents ev;
    rb::PanelLayout at;
    if ((rc = enqueue_panel(h, pairs, extra, n, *params, 3, ev, at))) return rc;
    HIP_TRY(hipMemcpyAsync(buf.h_panel.p, buf.d_work.p + at.header, sizeof(rb::PanelHeader), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipMemcpyAsync(out, buf.d_work.p + at.rows, n * sizeof(RibbitPanelRow), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    ev.print(n);
    // what the device returned
    const rb::PanelHeader header = *reinterpret_cast<const rb::PanelHeader *>(buf.h_panel.p);
    size_t members = 0;
    bool good = header.pools >= 0 && (size_t)header.pools <= n;
    std::vector<int32_t> filled(good ? (size_t)header.pools : 0, 0);
    for (size_t i = 0; i < n && good; ++i) {
        const RibbitPanelRow &r = out[i];
        good = r.reserved[0] == 0 && r.reserved[1] == 0 && r.reserved[2] == 0 && r.dimer >= 0 && r.size >= 0 && r.near >= 0 &&
               r.conflicts >= std::max(r.dimer, std::max(r.size, r.near)) && (int64_t)r.conflicts <= (int64_t)r.dimer + r.size + r.near && (size_t)r.conflicts < n;
        if (has_pair(pairs[i])) {
            good = good && r.pool >= 0 && r.pool < header.pools && ++filled[(size_t)r.pool] <= params->pool_size;
            ++members;
        } else {
            good = good && r.pool == -1 && r.conflicts == 0;
        }
    }
    for (const int32_t f : filled) good = good && f > 0;
    if (!good || (size_t)header.members != members) return fail(RIBBIT_E_INTERNAL, "the pools the GPU made do not add up");
    *rows = out;
    *n_pools = header.pools;
    return RIBBIT_OK;
}

int debug_conflicts_impl(RibbitHandle *h, const RibbitRowPrimerPair *pairs, const int32_t *extra, size_t n, const RibbitPanelParams *params, uint64_t *words) {
    if (!h) return fail(RIBBIT_E_ARG, "null handle");
    int rc;
    if ((rc = check_args(pairs, extra, n, params, RIBBIT_PANEL_MAX_DEBUG_PAIRS))) return rc;
    if (n == 0) return RIBBIT_OK;
    if (!words) return fail(RIBBIT_E_ARG, "null argument");
    StageEvents ev;
    rb::PanelLayout at;
    if ((rc = enqueue_panel(h, pairs, extra, n, *params, 1, ev, at))) return rc;
    HIP_TRY(hipMemcpyAsync(words, h->rows.d_work.p + at.matrix, n * (size_t)rb::panel_words((int64_t)n) * sizeof(uint64_t), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return RIBBIT_OK;
}

// ---- the host twin, in letters
struct HostPair {
    std::string l, r;
    int64_t start = 0, end = 0, group = -1, lo = 0, hi = 0;
};

uint8_t host_rules(const HostPair &a, const HostPair &b, const RibbitPanelParams &prm) {
    uint8_t rules = 0;
    for (const std::string *x : {&a.l, &a.r})
        for (const std::string *y : {&b.l, &b.r}) {
            int32_t any = 0, end = 0;
            host_duplex(*x, *y, any, end);
            if (any > prm.max_cross_any || end > prm.max_cross_end) rules |= DIMER;
        }
    if (prm.size_gap > 0 && a.lo - b.hi < prm.size_gap && b.lo - a.hi < prm.size_gap) rules |= SIZE;
    if (prm.max_cross_product > 0 && a.group >= 0 && a.group == b.group && std::max(a.end, b.end) - std::min(a.start, b.start) <= prm.max_cross_product) rules |= NEAR;
    return rules;
}

int host_panel_pools_impl(const RibbitRowPrimerPair *pairs, const int32_t *extra, size_t n, const RibbitPanelParams *params, RibbitPanelRow **rows, int32_t *n_pools) {
    if (!rows || !n_pools) return fail(RIBBIT_E_ARG, "null argument");
    int rc;
    if ((rc = check_args(pairs, extra, n, params, RIBBIT_PANEL_MAX_PAIRS))) return rc;
    const RibbitPanelParams prm = *params;
    Handed<RibbitPanelRow> out;
    if ((rc = hand_out<RibbitPanelRow>(nullptr, n, false, out))) return rc;
    // the rows that have a pair, in index order: `at` is a row's place among them
    std::vector<HostPair> all;
    std::vector<size_t> row_of;
    for (size_t i = 0; i < n; ++i) {
        out[i] = RibbitPanelRow{};
        out[i].pool = -1;
        if (!has_pair(pairs[i])) continue;
        HostPair p;
        host_pair_oligos(pairs[i], p.l, p.r);
        p.start = pairs[i].left.start;
        p.end = (int64_t)pairs[i].right.start + pairs[i].right.length;
        p.group = extra ? extra[3 * i] : -1;
        p.lo = extra ? extra[3 * i + 1] : pairs[i].product;
        p.hi = extra ? extra[3 * i + 2] : pairs[i].product;
        all.push_back(p);
        row_of.push_back(i);
    }
    const size_t m = all.size();
    // the rules of every two of them, a byte each: the part above the diagonal is judged, the part below it copied
    std::vector<uint8_t> rules(m * m, 0);
    const unsigned threads = (unsigned)std::max<size_t>(1, std::min<size_t>(rb::host_thread_count(0), m));
    rb::on_threads(threads, [&](unsigned t) {
        for (size_t a = t; a < m; a += threads)      // (dealt out, because place a has m - 1 - a tests)
            for (size_t b = a + 1; b < m; ++b) rules[a * m + b] = host_rules(all[a], all[b], prm);
    });
    for (size_t a = 0; a < m; ++a)
        for (size_t b = 0; b < a; ++b) rules[a * m + b] = rules[b * m + a];
    std::vector<size_t> order(m);
    for (size_t a = 0; a < m; ++a) {
        RibbitPanelRow &r = out[row_of[a]];
        for (size_t b = 0; b < m; ++b) {
            const uint8_t v = rules[a * m + b];
            r.conflicts += v != 0;
            r.dimer += (v & DIMER) != 0;
            r.size += (v & SIZE) != 0;
            r.near += (v & NEAR) != 0;
        }
        order[a] = a;
    }
    std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) { return out[row_of[a]].conflicts > out[row_of[b]].conflicts; });      // (stable: among equals by index)
    std::vector<std::vector<size_t>> pools;
    for (const size_t a : order) {
        size_t p = 0;
        for (; p < pools.size(); ++p) {
            if (pools[p].size() >= (size_t)prm.pool_size) continue;
            bool clash = false;
            for (const size_t b : pools[p]) clash = clash || rules[a * m + b] != 0;
            if (!clash) break;
        }
        if (p == pools.size()) pools.emplace_back();
        pools[p].push_back(a);
        out[row_of[a]].pool = (int32_t)p;
    }
    *n_pools = (int32_t)pools.size();
    *rows = out.release();
    return RIBBIT_OK;
}

// ---- the text
enum : int { BAD_POOL = 1, NO_PRODUCT = 2 };

// the ninth of a marker line's last 20 columns; false when it is no number
bool designed_product(BedField line, int64_t &out) {
    const char *end = line.to;
    for (int tabs = 0; tabs < 11; ++tabs) {      // the eleven columns behind it
        while (end > line.from && end[-1] != '\t') --end;
        if (end == line.from) return false;
        --end;      // (the tab)
    }
    const char *from = end;
    while (from > line.from && from[-1] != '\t') --from;
    if (from == line.from || from == end) return false;
    const auto r = std::from_chars(from, end, out);
    return r.ec == std::errc() && r.ptr == end;
}

int bed_panel_text_impl(const char *marker, size_t marker_len, const RibbitPanelRow *rows, size_t n, char **text, size_t *len) {
    if (!text || !len || (!marker && marker_len > 0) || (!rows && n > 0)) return fail(RIBBIT_E_ARG, "null argument");
    const size_t parts = bed_text_parts(marker_len);
    BedLines lines;
    int rc;
    if ((rc = lines.find(marker, marker_len, parts))) return rc;
    if (lines.count() != n) return fail(RIBBIT_E_ARG, "the marker text has %zu lines, not the %zu of the rows", lines.count(), n);
    struct Member { int32_t pool; int64_t product; size_t i; };
    std::vector<Member> members;
    for (size_t i = 0; i < n; ++i) {
        if (rows[i].pool < 0) continue;
        Member m{rows[i].pool, 0, i};
        if (!designed_product(lines[i], m.product)) return fail(RIBBIT_E_ARG, "line %zu of the marker text has no designed product", i);
        members.push_back(m);
    }
    std::sort(members.begin(), members.end(), [](const Member &a, const Member &b) {
        return a.pool != b.pool ? a.pool < b.pool : a.product != b.product ? a.product < b.product : a.i < b.i;
    });
    const size_t m = members.size();
    return write_pieces(parts, "the panel", text, len, [&](size_t k, std::string &out) {
        for (size_t at = m * k / parts; at < m * (k + 1) / parts; ++at) {
            const size_t i = members[at].i;
            const RibbitPanelRow &r = rows[i];
            put_field(out, lines[i]);
            for (const int32_t v : {r.pool, r.conflicts, r.dimer, r.size, r.near}) {
                out += '\t';
                put_number(out, v);
            }
            out += '\n';
        }
    });
}

}  // namespace

extern "C" {

void ribbit_panel_params_default(RibbitPanelParams *params) {
    if (params) *params = RibbitPanelParams{6, 4, 30, 4000, 8};
}

int ribbit_hip_panel_pools(RibbitHandle *h, const RibbitRowPrimerPair *pairs, const int32_t *extra, size_t n, const RibbitPanelParams *params, const RibbitPanelRow **rows,
                           int32_t *n_pools) {
    return guarded("the panel's pools", [&]() -> int { return panel_pools_impl(h, pairs, extra, n, params, rows, n_pools); });
}

int ribbit_host_panel_pools(const RibbitRowPrimerPair *pairs, const int32_t *extra, size_t n, const RibbitPanelParams *params, RibbitPanelRow **rows, int32_t *n_pools) {
    return guarded("the panel's pools", [&]() -> int { return host_panel_pools_impl(pairs, extra, n, params, rows, n_pools); });
}

void ribbit_panel_free(void *from_the_host_twin) { std::free(from_the_host_twin); }

int ribbit_hip_debug_panel_conflicts(RibbitHandle *h, const RibbitRowPrimerPair *pairs, const int32_t *extra, size_t n, const RibbitPanelParams *params, uint64_t *words) {
    return guarded("the panel's conflicts", [&]() -> int { return debug_conflicts_impl(h, pairs, extra, n, params, words); });
}

int ribbit_bed_panel_text(const char *marker_text, size_t len, const RibbitPanelRow *rows, size_t n, char **text, size_t *out_len) {
    return guarded("the panel as text", [&]() -> int { return bed_panel_text_impl(marker_text, len, rows, n, text, out_len); });
}

}  // extern "C"
