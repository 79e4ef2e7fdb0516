// api_compound.cpp -- the rows of a record chained into compound loci (compound.hip); see api_internal.h for the map of the files
// behind include/ribbit_hip.h.  The GPU form stages the rows and their labels through stage_down (it reads no coverage bitmap), runs on the
// handle's stream and keeps nothing between calls; the host twin is written from the contract, one sort and one sweep; the
// labels of the rows' motif classes and the chains' text need no GPU either.
#include "bed_text.h"

namespace {

constexpr size_t MAX_ROWS = (size_t)INT32_MAX;      // (the indices are int32)
constexpr size_t TOTALS_BYTES = sizeof(rb::CompoundTotals);      // the result on its way up: the totals, then n chains of room, then the members
static_assert(TOTALS_BYTES == 16 && sizeof(RibbitCompound) == 40 && sizeof(rb::CompoundSums) == 24, "the chains follow the totals in one buffer, 8-byte aligned");

int check_compound_args(const int32_t *intervals, const int32_t *labels, size_t n, int32_t gap, const void *compounds, const size_t *n_compounds,
                        const void *members, const size_t *n_members) {
    if (((!intervals || !labels) && n > 0) || !compounds || !n_compounds || !members || !n_members) return fail(RIBBIT_E_ARG, "null argument");
    if (gap < 0) return fail(RIBBIT_E_ARG, "gap %d is negative", (int)gap);
    if (n > MAX_ROWS) return fail(RIBBIT_E_ARG, "%zu intervals", n);
    return RIBBIT_OK;
}

int record_compounds_impl(RibbitHandle *h, const int32_t *intervals, const int32_t *labels, size_t n, int32_t gap, const RibbitCompound **compounds,
                          size_t *n_compounds, const int32_t **members, size_t *n_members) {
    if (!h) return fail(RIBBIT_E_ARG, "null handle");
    int rc;
    if ((rc = check_compound_args(intervals, labels, n, gap, compounds, n_compounds, members, n_members))) return rc;
    if (!h->loaded) return fail(RIBBIT_E_STATE, "no record loaded");
    static const RibbitCompound kNoChains[1] = {};
    static const int32_t kNoMembers[1] = {0};
    *compounds = kNoChains;
    *members = kNoMembers;
    *n_compounds = *n_members = 0;
    const int64_t length = h->length;
    if (length == 0 || n == 0) return RIBBIT_OK;
    if ((rc = bind_device(h))) return rc;
    const size_t out_members = TOTALS_BYTES + n * sizeof(RibbitCompound), out_bytes = out_members + n * sizeof(int32_t);
    RibbitHandle::RowBufs &buf = h->rows;
    const rb::CompoundLayout at = rb::compound_layout((int64_t)n, length);
    if ((rc = buf.d_work.ensure(at.bytes, true))) return rc;
    if ((rc = buf.h_cmp.ensure(out_bytes, true))) return rc;
    const StageSegment down[2] = {{intervals, 2 * n * sizeof(int32_t)}, {labels, n * sizeof(int32_t)}};
    const uint8_t *d_in[2];
    if ((rc = stage_down(h, down, 2, d_in))) return rc;
    uint8_t *work = buf.d_work.p, *up = buf.h_cmp.p;
    HIP_TRY(rb::launch_compounds(reinterpret_cast<const int32_t *>(d_in[0]), reinterpret_cast<const int32_t *>(d_in[1]), (int64_t)n, length, gap, work,
                                 buf.d_work.cap, at, h->stream));
    // the two counts come up first; then the chains and the members there are, not the room they have
    HIP_TRY(hipMemcpyAsync(up, work + at.totals, TOTALS_BYTES, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    rb::CompoundTotals totals;
    std::memcpy(&totals, up, sizeof totals);
    if (totals.rows > n || totals.chains > totals.rows || (totals.chains == 0) != (totals.rows == 0))
        return fail(RIBBIT_E_INTERNAL, "the chains' counts contradict each other (%u chains of %u rows of %zu)", totals.chains, totals.rows, n);
    if (totals.rows == 0) return RIBBIT_OK;      // every row is empty
    HIP_TRY(hipMemcpyAsync(up + TOTALS_BYTES, work + at.compounds, totals.chains * sizeof(RibbitCompound), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipMemcpyAsync(up + out_members, work + at.members, totals.rows * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    const RibbitCompound *found = reinterpret_cast<const RibbitCompound *>(up + TOTALS_BYTES);
    if (found[0].first != 0 || (size_t)found[totals.chains - 1].first + (size_t)found[totals.chains - 1].rows != totals.rows)
        return fail(RIBBIT_E_INTERNAL, "the chains do not tile their %u members", totals.rows);
    *compounds = found;
    *n_compounds = totals.chains;
    *members = reinterpret_cast<const int32_t *>(up + out_members);
    *n_members = totals.rows;
    return RIBBIT_OK;
}

// ---- host twin: the contract as it is written
int host_record_compounds_impl(int64_t length, const int32_t *intervals, const int32_t *labels, size_t n, int32_t gap, RibbitCompound **compounds,
                               size_t *n_compounds, int32_t **members, size_t *n_members) {
    int rc;
    if ((rc = check_compound_args(intervals, labels, n, gap, compounds, n_compounds, members, n_members))) return rc;
    if (length < 0 || length > (int64_t)INT32_MAX) return fail(RIBBIT_E_ARG, "a record of %lld bases", (long long)length);
    using Row = ClippedRow;
    const std::vector<Row> order =
        clipped_sorted_rows(length, intervals, n, [](const Row &a, const Row &b) { return a.s != b.s ? a.s < b.s : a.e != b.e ? a.e < b.e : a.index < b.index; });
    std::vector<RibbitCompound> chains;
    std::vector<int32_t> in_order(order.size()), seen;      // seen: the open chain's labels
    auto close_chain = [&]() {
        if (chains.empty()) return;
        std::sort(seen.begin(), seen.end());
        chains.back().classes = (int32_t)(std::unique(seen.begin(), seen.end()) - seen.begin());
        seen.clear();
    };
    int64_t reach = 0;
    for (size_t k = 0; k < order.size(); ++k) {
        const Row &row = order[k];
        in_order[k] = (int32_t)row.index;
        if (k == 0 || row.s - reach > (int64_t)gap) {
            close_chain();
            chains.push_back(RibbitCompound{0, (int32_t)row.s, 0, 0, 0, 0, 0, (int32_t)k, 0});
            reach = row.e;
        } else {
            RibbitCompound &c = chains.back();
            c.switches += labels[row.index] != labels[order[k - 1].index];
            c.overlaps += row.s < reach;
            reach = std::max(reach, row.e);
        }
        RibbitCompound &c = chains.back();
        c.end = (int32_t)reach;
        c.rows += 1;
        c.bases += row.e - row.s;
        seen.push_back(labels[row.index]);
    }
    close_chain();
    Handed<RibbitCompound> out;
    if ((rc = hand_out(chains.data(), chains.size(), false, out)) || (rc = hand_out(in_order.data(), in_order.size(), false, members))) return rc;
    *compounds = out.release();
    *n_compounds = chains.size();
    *n_members = in_order.size();
    return RIBBIT_OK;
}

// ---- the rows' classes as labels
int class_labels_impl(const char *classes, const int32_t *offsets, size_t n, const RibbitMotifClass *groups, size_t n_groups, int32_t **labels) {
    if (!labels || ((!classes || !offsets) && n > 0) || (!groups && n_groups > 0)) return fail(RIBBIT_E_ARG, "null argument");
    if (n > MAX_ROWS || n_groups > MAX_ROWS) return fail(RIBBIT_E_ARG, "%zu rows in %zu groups", n, n_groups);
    for (size_t i = 0; i < n; ++i)
        if (offsets[i] < 0 || offsets[i + 1] < offsets[i]) return fail(RIBBIT_E_ARG, "row %zu: the classes' offsets do not ascend", i);
    for (size_t g = 0; g < n_groups; ++g) {
        const RibbitMotifClass &c = groups[g];
        if (c.first_row < 0 || (size_t)c.first_row >= n) return fail(RIBBIT_E_ARG, "group %zu: its first row %d is none of %zu rows", g, (int)c.first_row, n);
        if (offsets[c.first_row + 1] - offsets[c.first_row] != c.length)
            return fail(RIBBIT_E_ARG, "group %zu: a class of %d bases whose first row's has %d", g, (int)c.length, (int)(offsets[c.first_row + 1] - offsets[c.first_row]));
    }
    // the groups come in class order (length, then bytes): a row's group is found by bisection
    auto order = [&](int32_t k, const char *text, const RibbitMotifClass &c) {      // < 0, 0, > 0: the class (k, text) against the group's
        return k != c.length ? (k < c.length ? -1 : 1) : std::memcmp(text, classes + offsets[c.first_row], (size_t)k);
    };
    Handed<int32_t> out;
    int rc;
    if ((rc = hand_out<int32_t>(nullptr, n, false, out))) return rc;
    for (size_t i = 0; i < n; ++i) {
        const int32_t k = offsets[i + 1] - offsets[i];
        const char *text = classes + offsets[i];
        size_t lo = 0, hi = n_groups;
        while (lo < hi) {
            const size_t mid = lo + (hi - lo) / 2;
            if (order(k, text, groups[mid]) > 0) lo = mid + 1; else hi = mid;
        }
        if (lo == n_groups || order(k, text, groups[lo]) != 0) return fail(RIBBIT_E_ARG, "row %zu: its class is the class of no group", i);
        out[i] = (int32_t)lo;
    }
    *labels = out.release();
    return RIBBIT_OK;
}

// ---- the chains as text
int compound_text_impl(const char *name, const char *bed, size_t bed_len, int64_t length, const int32_t *intervals, size_t n, const RibbitCompound *compounds,
                       size_t n_compounds, const int32_t *members, size_t n_members, char **text, size_t *len) {
    if (!name || !text || !len || (!bed && bed_len > 0) || (!intervals && n > 0) || (!compounds && n_compounds > 0) || (!members && n_members > 0))
        return fail(RIBBIT_E_ARG, "null argument");
    if (length < 0 || length > (int64_t)INT32_MAX) return fail(RIBBIT_E_ARG, "a record of %lld bases", (long long)length);
    // the BED text's line starts are found in pieces, and the chains' lines are written in as many pieces
    const size_t parts = n_compounds ? bed_text_parts(bed_len) : 1;
    BedLines lines;
    int rc;
    if (n_compounds && (rc = lines.find(bed, bed_len, parts))) return rc;
    const size_t n_lines = lines.count(), name_len = std::strlen(name);
    const size_t out_parts = std::max<size_t>(1, std::min<size_t>(parts, n_compounds >> 12));
    enum : int { FINE = 0, RANGE, MEMBER, EMPTY, LINE };      // a refusal's why; a: the chain, b: its member's position
    return write_pieces(out_parts, "the chains", text, len, [&](size_t t, std::string &out) {
        std::string structure;
        for (size_t c = n_compounds * t / out_parts; c < n_compounds * (t + 1) / out_parts; ++c) {
            const RibbitCompound &k = compounds[c];
            if (k.first < 0 || k.rows < 1 || (size_t)k.first + (size_t)k.rows > n_members) return PieceRefusal{RANGE, c, 0};
            structure.clear();
            int64_t reach = 0;
            for (size_t j = (size_t)k.first; j < (size_t)k.first + (size_t)k.rows; ++j) {
                const int32_t row = members[j];
                if (row < 0 || (size_t)row >= n || (size_t)row >= n_lines) return PieceRefusal{MEMBER, c, j};
                const int64_t s = std::max<int64_t>(intervals[2 * (size_t)row], 0), e = std::min<int64_t>(intervals[2 * (size_t)row + 1], length);
                if (s >= e) return PieceRefusal{EMPTY, c, j};
                const BedField line = lines[(size_t)row];
                const BedRow fields = bed_row(line.from, line.to);
                if (!fields.ok) return PieceRefusal{LINE, c, j};
                if (j > (size_t)k.first) {
                    const int64_t d = s - reach;
                    if (d) {
                        structure += d > 0 ? 'n' : 'o';
                        put_number(structure, d > 0 ? d : -d);
                    }
                }
                structure += '(';
                put_field(structure, fields.motif);
                structure += ')';
                put_field(structure, fields.units);
                reach = j == (size_t)k.first ? e : std::max(reach, e);
            }
            out.append(name, name_len);
            out += '\t';
            put_number(out, k.start);
            out += '\t';
            put_number(out, k.end);
            out += '\t';
            out += k.rows == 1 ? 'p' : k.classes > 1 ? 'c' : 'i';
            if (k.overlaps > 0) out += '*';
            for (const int64_t v : {(int64_t)k.rows, (int64_t)k.classes, k.bases}) {
                out += '\t';
                put_number(out, v);
            }
            out += '\t';
            out += structure;
            out += '\n';
        }
        return PieceRefusal{};
    }, [&](const PieceRefusal &b) {
        switch (b.why) {
            case RANGE:
                return fail(RIBBIT_E_ARG, "chain %zu: members %d .. %lld of %zu", b.a, (int)compounds[b.a].first, (long long)compounds[b.a].first + compounds[b.a].rows,
                            n_members);
            case MEMBER: return fail(RIBBIT_E_ARG, "chain %zu: member %d is no row of %zu with a line of the BED text (%zu lines)", b.a, (int)members[b.b], n, n_lines);
            case EMPTY: return fail(RIBBIT_E_ARG, "chain %zu: member %d is an empty row", b.a, (int)members[b.b]);
            default: return fail(RIBBIT_E_ARG, "chain %zu: line %d of the BED text is not a row of 11 tab-separated columns", b.a, (int)members[b.b]);
        }
    });
}

}  // namespace

extern "C" {

int ribbit_hip_record_compounds(RibbitHandle *h, const int32_t *intervals, const int32_t *labels, size_t n, int32_t gap, const RibbitCompound **compounds,
                                size_t *n_compounds, const int32_t **members, size_t *n_members) {
    return guarded("the compound loci", [&]() -> int { return record_compounds_impl(h, intervals, labels, n, gap, compounds, n_compounds, members, n_members); });
}

int ribbit_host_record_compounds(int64_t length, const int32_t *intervals, const int32_t *labels, size_t n, int32_t gap, RibbitCompound **compounds,
                                 size_t *n_compounds, int32_t **members, size_t *n_members) {
    return guarded("the compound loci", [&]() -> int { return host_record_compounds_impl(length, intervals, labels, n, gap, compounds, n_compounds, members, n_members); });
}

void ribbit_compounds_free(RibbitCompound *compounds) { std::free(compounds); }

int ribbit_class_labels(const char *classes, const int32_t *offsets, size_t n, const RibbitMotifClass *groups, size_t n_groups, int32_t **labels) {
    return guarded("the classes' labels", [&]() -> int { return class_labels_impl(classes, offsets, n, groups, n_groups, labels); });
}

int ribbit_compound_text(const char *name, const char *bed_text, size_t bed_len, int64_t length, const int32_t *intervals, size_t n,
                         const RibbitCompound *compounds, size_t n_compounds, const int32_t *members, size_t n_members, char **text, size_t *len) {
    return guarded("the compound loci's text", [&]() -> int {
        return compound_text_impl(name, bed_text, bed_len, length, intervals, n, compounds, n_compounds, members, n_members, text, len);
    });
}

}  // extern "C"
