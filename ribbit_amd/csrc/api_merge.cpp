// api_merge.cpp -- the anchored stage's merge as device work: what rb::AnchoredDevicePass::run (parallel_merge.h) does on a
// handle.  The ranges, their cuts and starting cursors come from the host's preparation (parallel_merge.cpp); the kept calls
// and the composed planes are in device memory already (window_stage_device, scan_anchored_kernel); the perfect and
// substitution lists travel up (0.1 GB for a chromosome), the ranges' parts of the anchored list and their logs travel down.
#include "api_internal.h"

namespace rbapi {

namespace {

// HIP_TRY returns an int status; inside run() a failure means "the host pass runs"
#define MERGE_TRY(expr) do { const hipError_t e_ = (expr); if (e_ != hipSuccess) { (void)fail(RIBBIT_E_INTERNAL, "%s: %s", #expr, hipGetErrorString(e_)); return false; } } while (0)

// what the pass reads beside the lists and the calls: the composed planes, the motif bounds, and the caps that the production
// pass fixes (defaults: the handle's planes; rb::AM_* of kernels.h) and ribbit_hip_debug_merge_ranges sets
struct DevicePassConfig {
    const uint32_t *d_xa = nullptr;
    int64_t xa_stride = 0;
    int m_lo = 0, m_hi = -1;
    size_t log_cap = 0;                                  // 0: every seed once, a quarter of the calls and 65536 more
    uint32_t head_cap = 1u << 16;
    uint32_t resident_waves = (uint32_t)rb::AM_RESIDENT_WAVES;
    uint32_t max_passes = rb::AM_MAX_PASSES;
};

bool run_device_pass(RibbitHandle *h, const DevicePassConfig &cfg, RibbitCall *d_calls, const int32_t *d_pend, const rb::SeedLists &lists, const rb::KeptCalls &kc,
                     const std::vector<size_t> &first, const std::vector<int> &cut_pos, const std::vector<rb::Cursor2> &start_cursor,
                     const std::vector<uint32_t> &order, size_t device_limit, const std::function<void(uint32_t *, const uint32_t *)> &meanwhile,
                     std::vector<rb::AnchoredDevicePass::RangeResult> &ranges, std::vector<rb::AnchoredDevicePass::LogEntry> &undo,
                     std::vector<rb::AnchoredDevicePass::LogEntry> &reads, std::vector<rb::AnchoredDevicePass::HeadEntry> &heads) {
    const bool profile = rb::profile_on();
    const double t0 = now_ms();
    RibbitHandle::MergeBufs &mg = h->mg;
    const size_t nr = cut_pos.size(), nP = lists.perfect.size(), nS = lists.subst.size(), n = kc.n;
    if (nr < 2 || first.size() != nr + 1 || start_cursor.size() != nr || first[nr] != n || order.size() > nr) return false;      // (the stage passes all nr ranges; fewer only from ribbit_hip_debug_merge_ranges' only_range)
    if (nP >= (1u << 30) || nS >= (1u << 30) || n + nr >= (1ull << 30) || nr >= (1u << 28)) return false;      // (the packing of candidates and log entries)
    if (!cfg.d_xa || cfg.resident_waves < 1 || cfg.resident_waves > (uint32_t)rb::AM_RESIDENT_WAVES || cfg.head_cap < 1) return false;
    if (bind_device(h)) return false;
    const uint32_t head_cap = cfg.head_cap;
    const size_t log_cap = cfg.log_cap ? cfg.log_cap : nP + nS + n / 4 + 65536;
    if (mg.d_perfect.ensure(std::max<size_t>(nP, 1)) || mg.d_subst.ensure(std::max<size_t>(nS, 1)) || mg.d_type0.ensure(nP + nS + 1) ||
        mg.d_own.ensure(n + nr) || mg.d_first.ensure(2 * nr + 1) || mg.d_cuts.ensure(3 * nr) || mg.d_range_out.ensure(nr * rb::AM_RANGE_OUT_WORDS) ||
        mg.d_log.ensure(4 * log_cap) || mg.d_head_log.ensure(8 * (size_t)head_cap) || mg.d_counts.ensure(4) ||
        mg.d_scratch.ensure(64 * (size_t)rb::AM_RESIDENT_WAVES * (size_t)rb::AM_SCRATCH_WORDS) || mg.h_own.ensure(n + nr) || mg.h_range_out.ensure(nr * rb::AM_RANGE_OUT_WORDS) ||
        mg.h_counts.ensure(4) || mg.h_head_log.ensure(8 * (size_t)head_cap))
        return false;
    if (!mg.h_sync.p) {
        if (mg.h_sync.ensure(16)) return false;
        MERGE_TRY(hipHostGetDevicePointer((void **)&mg.h_sync_dev, mg.h_sync.p, 0));
    }
    mg.h_sync.p[0] = (uint32_t)std::min(device_limit, order.size()); mg.h_sync.p[1] = 0;
    // ranges, cuts, cursors
    std::vector<uint32_t> first32(nr + 1);
    for (size_t k = 0; k <= nr; ++k) first32[k] = (uint32_t)first[k];
    std::vector<int32_t> cuts(3 * nr);
    for (size_t k = 0; k < nr; ++k) { cuts[k] = cut_pos[k]; cuts[nr + 2 * k] = start_cursor[k].perfect; cuts[nr + 2 * k + 1] = start_cursor[k].subst; }
    hipStream_t st = h->stream;
    MERGE_TRY(hipMemcpyAsync(mg.d_first.p, first32.data(), (nr + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    MERGE_TRY(hipMemcpyAsync(mg.d_first.p + nr + 1, order.data(), order.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    MERGE_TRY(hipMemsetAsync(mg.d_range_out.p, 0xff, nr * rb::AM_RANGE_OUT_WORDS * sizeof(uint32_t), st));      // (status of a range nobody merged: all ones)
    MERGE_TRY(hipMemcpyAsync(mg.d_cuts.p, cuts.data(), 3 * nr * sizeof(int32_t), hipMemcpyHostToDevice, st));
    if (nP) MERGE_TRY(hipMemcpyAsync(mg.d_perfect.p, lists.perfect.data(), nP * sizeof(RibbitSeed), hipMemcpyHostToDevice, st));
    if (nS) MERGE_TRY(hipMemcpyAsync(mg.d_subst.p, lists.subst.data(), nS * sizeof(RibbitSeed), hipMemcpyHostToDevice, st));
    // (the host threads retire seeds in these lists while the kernel runs: the copies must have left them by then)
    MERGE_TRY(hipStreamSynchronize(st));
    rb::launch_seed_types(mg.d_perfect.p, (uint32_t)nP, mg.d_type0.p, st);
    rb::launch_seed_types(mg.d_subst.p, (uint32_t)nS, mg.d_type0.p + nP, st);
    MERGE_TRY(hipMemsetAsync(mg.d_counts.p, 0, 4 * sizeof(uint32_t), st));
    rb::AnchoredMergeArgs a{};
    a.P = mg.d_perfect.p; a.S = mg.d_subst.p; a.nP = (uint32_t)nP; a.nS = (uint32_t)nS;
    a.P_type0 = mg.d_type0.p; a.S_type0 = mg.d_type0.p + nP;
    a.calls = d_calls; a.pend = d_pend;
    a.first = mg.d_first.p; a.cut_pos = mg.d_cuts.p; a.cur0 = mg.d_cuts.p + nr; a.nr = (uint32_t)nr;
    a.xa = cfg.d_xa; a.xa_stride = cfg.xa_stride; a.length = lists.length; a.m_lo = cfg.m_lo; a.m_hi = cfg.m_hi;
    a.own = mg.d_own.p; a.range_out = mg.d_range_out.p;
    a.log = mg.d_log.p; a.log_count = mg.d_counts.p; a.log_cap = (uint32_t)std::min<size_t>(log_cap, 0xffffffffu);
    a.head_log = mg.d_head_log.p; a.head_count = mg.d_counts.p + 1; a.head_cap = head_cap;
    a.scratch = mg.d_scratch.p; a.next_range = mg.d_counts.p + 2;
    a.order = mg.d_first.p + nr + 1; a.n_order = (uint32_t)order.size(); a.sync = mg.h_sync_dev;
    const double t1 = now_ms();
    a.max_passes = cfg.max_passes;
    rb::launch_anchored_merge(a, (uint32_t)n, cfg.resident_waves, st);
    MERGE_TRY(hipGetLastError());
    meanwhile(mg.h_sync.p, mg.h_sync.p + 1);         // the host threads' share of the ranges, while the kernel runs
    const double t1b = now_ms();
    MERGE_TRY(hipMemcpyAsync(mg.h_counts.p, mg.d_counts.p, 4 * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    MERGE_TRY(hipMemcpyAsync(mg.h_range_out.p, mg.d_range_out.p, nr * rb::AM_RANGE_OUT_WORDS * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    MERGE_TRY(hipMemcpyAsync(mg.h_own.p, mg.d_own.p, (n + nr) * sizeof(RibbitSeed), hipMemcpyDeviceToHost, st));
    MERGE_TRY(hipStreamSynchronize(st));
    const double t2 = now_ms();
    const uint32_t n_log = mg.h_counts.p[0], n_head = mg.h_counts.p[1];
    if (n_log > a.log_cap || n_head > head_cap) return false;            // (every range that met the full log says so too; nothing was applied to the host lists)
    if (mg.h_log.ensure(4 * std::max<size_t>(n_log, 1))) return false;
    if (n_log) MERGE_TRY(hipMemcpyAsync(mg.h_log.p, mg.d_log.p, 4 * (size_t)n_log * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    if (n_head) MERGE_TRY(hipMemcpyAsync(mg.h_head_log.p, mg.d_head_log.p, 8 * (size_t)n_head * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    MERGE_TRY(hipStreamSynchronize(st));
    ranges.resize(nr);
    for (size_t k = 0; k < nr; ++k) {
        const uint32_t *o = mg.h_range_out.p + k * rb::AM_RANGE_OUT_WORDS;
        rb::AnchoredDevicePass::RangeResult &r = ranges[k];
        r.own = mg.h_own.p + first[k] + k;
        r.own_n = o[0]; r.status = o[1];
        if (!r.status && r.own_n > first[k + 1] - first[k] + 1) r.status |= 0x80000000u;
        r.guard_hits = (int64_t)(((uint64_t)o[3] << 32) | o[2]);
        r.cursor.perfect = (int)o[4]; r.cursor.subst = (int)o[5];
        r.head_reads[0] = ((uint64_t)o[7] << 32) | o[6];
        r.head_reads[1] = ((uint64_t)o[9] << 32) | o[8];
    }
    undo.clear(); reads.clear(); heads.clear();
    for (uint32_t i = 0; i < n_log; ++i) {
        const uint32_t *e = mg.h_log.p + 4 * (size_t)i;
        const uint32_t kind = e[0] >> 28, range = e[0] & 0x0fffffffu;
        if (range >= nr) return false;
        const rb::AnchoredDevicePass::LogEntry le{range, e[1] >> 31, e[1] & 0x7fffffffu, (int32_t)e[2]};
        if (le.index >= (le.list ? nS : nP)) return false;
        if (kind == rb::AM_LOG_UNDO) undo.push_back(le);
        else if (kind == rb::AM_LOG_READ) reads.push_back(le);
        else return false;
    }
    for (uint32_t i = 0; i < n_head; ++i) {
        const uint32_t *e = mg.h_head_log.p + 8 * (size_t)i;
        if (e[0] >= nr || e[1] > 1 || e[2] >= (e[1] ? nS : nP)) return false;
        heads.push_back({e[0], e[1], e[2], RibbitSeed{(int32_t)e[3], (int32_t)e[4], (int32_t)e[5], (int32_t)e[6]}, e[7] != 0});
    }
    if (profile) {
        size_t slow_k = 0, merged = 0, too_slow = 0, too_many = 0, calls_on_device = 0;
        uint64_t ticks_sum = 0, passes_sum = 0; uint32_t ticks_max = 0;
        for (size_t k = 0; k < nr; ++k) {
            const uint32_t *o = mg.h_range_out.p + k * rb::AM_RANGE_OUT_WORDS;
            if (o[1] == 0xffffffffu) continue;                     // not the device's
            too_slow += (o[1] & rb::AM_TOO_SLOW) != 0; too_many += (o[1] & rb::AM_SCRATCH_FULL) != 0;
            if (o[1]) continue;
            ++merged; calls_on_device += first[k + 1] - first[k];
            ticks_sum += o[11]; passes_sum += o[10];
            if (o[11] > ticks_max) { ticks_max = o[11]; slow_k = k; }
        }
        std::fprintf(stderr, "[anchored merge on the device] %zu calls in %zu ranges, %zu of them within a lane's reach: lists up and set-up %.1f ms, the host threads' share while the kernel ran %.1f ms, "
                     "%.1f ms more for the kernel and its results, logs %.1f ms (%u entries: %zu retirements, %zu reads left of a range; %u list-head writes).  Merged on the device: %zu ranges, %zu calls; "
                     "left to the host: %zu ranges (%zu over their budget of passes, %zu with more candidates than the LDS holds).  A range took %.2f ms on average (%.0f passes of its lane's loop), the slowest %.2f ms (%zu calls)\n",
                     n, nr, std::min(device_limit, order.size()), t1 - t0, t1b - t1, t2 - t1b, now_ms() - t2, n_log, undo.size(), reads.size(), n_head, merged, calls_on_device, too_slow + too_many, too_slow, too_many,
                     merged ? (double)ticks_sum * 1e-5 / (double)merged : 0.0, merged ? (double)passes_sum / (double)merged : 0.0, ticks_max * 1e-5, first[slow_k + 1] - first[slow_k]);
    }
    return true;
}

}  // namespace

rb::AnchoredDevicePass anchored_device_pass(RibbitHandle *h, RibbitCall *d_calls, const int32_t *d_pend) {
    rb::AnchoredDevicePass p;
    if (const char *e = std::getenv("RIBBIT_DEVICE_MERGE_MIN")) p.min_calls = (size_t)std::strtoull(e, nullptr, 10);        // tuning / tests
    if (const char *e = std::getenv("RIBBIT_DEVICE_MERGE_RANGE")) p.calls_per_range = std::max<size_t>(1, (size_t)std::strtoull(e, nullptr, 10));
    p.run = [h, d_calls, d_pend](const rb::SeedLists &lists, const rb::KeptCalls &kc, const std::vector<size_t> &first, const std::vector<int> &cut_pos,
                                 const std::vector<rb::Cursor2> &start_cursor, const std::vector<uint32_t> &order, size_t device_limit, const std::function<void(uint32_t *, const uint32_t *)> &meanwhile,
                                 std::vector<rb::AnchoredDevicePass::RangeResult> &ranges,
                                 std::vector<rb::AnchoredDevicePass::LogEntry> &undo, std::vector<rb::AnchoredDevicePass::LogEntry> &reads,
                                 std::vector<rb::AnchoredDevicePass::HeadEntry> &heads) {
        if (!h->rec.xa_on_device || !h->d_xa.p) return false;
        DevicePassConfig cfg;
        cfg.d_xa = h->d_xa.p; cfg.xa_stride = h->xa_stride; cfg.m_lo = h->params.min_motif; cfg.m_hi = h->params.max_motif;
        return run_device_pass(h, cfg, d_calls, d_pend, lists, kc, first, cut_pos, start_cursor, order, device_limit, meanwhile, ranges, undo, reads, heads);
    };
    return p;
}

}  // namespace rbapi

using namespace rbapi;

extern "C" {

void ribbit_debug_merge_ranges_free(RibbitDebugMergeRanges *out) {
    if (!out) return;
    std::free(out->cuts); std::free(out->first); std::free(out->cursors0); std::free(out->range); std::free(out->own);
    std::free(out->undo); std::free(out->reads); std::free(out->heads);
    ribbit_seed_lists_free(&out->lists);
    std::memset(out, 0, sizeof *out);
}

int ribbit_hip_debug_merge_ranges(RibbitHandle *h, const RibbitScanParams *params, int64_t length,
                                  const RibbitSeed *perfect, size_t n_perfect, const RibbitSeed *subst, size_t n_subst,
                                  const RibbitCall *calls, size_t n_calls, const uint32_t *xa, size_t xa_stride,
                                  const RibbitDebugMergeKnobs *knobs, RibbitDebugMergeRanges *out) { return guarded("the merge of the ranges", [&]() -> int {
    if (!params || !knobs || !out || !xa || (n_perfect && !perfect) || (n_subst && !subst) || (n_calls && !calls)) return fail(RIBBIT_E_ARG, "null argument");
    const bool lanes = knobs->where == RIBBIT_MERGE_ON_LANES;
    if (!lanes && knobs->where != RIBBIT_MERGE_ON_HOST) return fail(RIBBIT_E_ARG, "where: the lanes (0) or the host workers (1)");
    if (lanes && !h) return fail(RIBBIT_E_ARG, "the lanes need an open handle");
    const int m_lo = params->min_motif, m_hi = params->max_motif;
    if (m_lo < 1 || m_hi < m_lo || length < 1 || length > INT32_MAX - 2 * (int64_t)m_hi - 64) return fail(RIBBIT_E_ARG, "bad motif range or length");
    if (xa_stride < (size_t)(length / 32 + 1)) return fail(RIBBIT_E_ARG, "composed planes (xa) too short");
    if (knobs->calls_per_range < 1 || knobs->resident_waves < 0 || knobs->resident_waves > rb::AM_RESIDENT_WAVES || knobs->max_passes < 0 ||
        knobs->max_passes > (1 << 24) || knobs->head_cap < 0 || knobs->head_cap > (1 << 24) || knobs->log_cap < 0 || knobs->log_cap > (1ll << 28) || knobs->only_range < -1)
        return fail(RIBBIT_E_ARG, "a knob is out of range");
    // nothing the lanes index with may leave the planes: every interval inside the record, every motif size a plane of `xa`
    auto inside = [&](int32_t start, int32_t end, int32_t mlen) { return start >= 0 && start <= end && (int64_t)end <= length && mlen >= m_lo && mlen <= m_hi; };
    for (size_t i = 0; i < n_perfect; ++i) if (!inside(perfect[i].start, perfect[i].end, perfect[i].mlen)) return fail(RIBBIT_E_ARG, "perfect seed %zu lies outside the record or the motif range", i);
    for (size_t i = 0; i < n_subst; ++i) if (!inside(subst[i].start, subst[i].end, subst[i].mlen)) return fail(RIBBIT_E_ARG, "substitution seed %zu lies outside the record or the motif range", i);
    for (size_t i = 0; i < n_calls; ++i) if (!inside(calls[i].start, calls[i].end, calls[i].mlen)) return fail(RIBBIT_E_ARG, "call %zu lies outside the record or the motif range", i);
    // ... and every seed of the type its list holds.  The reference retires a candidate in the list that the candidate's TYPE names
    // (parse_anchored_shiftxor.cpp: `if (last_type == RANK_P) ... else if (last_type == RANK_S || last_type == RANK_Q)`), at the
    // candidate's index: a substitution-list seed typed P, or a perfect-list seed typed S or Q, retires some OTHER seed (or writes
    // beyond the other list), stays live itself, and the call starts again unchanged -- without end on the host, whose merge has no
    // bound on its rounds (the lanes give up after AM_MAX_ROUNDS).  The stages never make such lists.
    for (size_t i = 0; i < n_perfect; ++i)
        if (perfect[i].type != RIBBIT_RANK_P && perfect[i].type != RIBBIT_RANK_N) return fail(RIBBIT_E_ARG, "perfect seed %zu has type %d: the perfect list holds P and N", i, perfect[i].type);
    for (size_t i = 0; i < n_subst; ++i)
        if (subst[i].type != RIBBIT_RANK_S && subst[i].type != RIBBIT_RANK_Q && subst[i].type != RIBBIT_RANK_N)
            return fail(RIBBIT_E_ARG, "substitution seed %zu has type %d: the substitution list holds S, Q and N", i, subst[i].type);
    std::memset(out, 0, sizeof *out);
    const int32_t caps[16] = {rb::AM_PS_CAP, rb::AM_CAND_CAP, rb::AM_PS_SPILL, rb::AM_CAND_SPILL, rb::AM_CHILD_CAP, rb::AM_COV_CAP, rb::AM_RESIDENT_WAVES, (int32_t)rb::AM_MAX_PASSES,
                              (int32_t)rb::AM_SCRATCH_FULL, (int32_t)rb::AM_LOG_FULL, (int32_t)rb::AM_BAD_PLANE, (int32_t)rb::AM_RUNAWAY, (int32_t)rb::AM_TOO_SLOW, 0, 0, 0};
    std::memcpy(out->caps, caps, sizeof caps);

    const size_t nm = (size_t)(m_hi - m_lo + 1);
    rb::HostPlanes hp;
    hp.length = length;
    hp.xa.assign(xa, xa + nm * xa_stride);
    hp.xa_stride = (int64_t)xa_stride; hp.xa_m_lo = m_lo; hp.xa_m_hi = m_hi;
    rb::SeedLists sl;
    sl.length = length; sl.min_motif = m_lo; sl.max_motif = m_hi; sl.min_shift = m_lo > 2 ? m_lo - 2 : 1;
    sl.perfect.assign(perfect, perfect + n_perfect);
    sl.subst.assign(subst, subst + n_subst);
    use_composed_planes(sl, &hp);

    DevBuf<RibbitCall> d_calls;
    DevBuf<int32_t> d_pend;
    DevBuf<uint32_t> d_xa;
    rb::AnchoredDevicePass pass;
    pass.min_calls = 0;
    pass.calls_per_range = (size_t)knobs->calls_per_range;
    if (lanes)
        pass.run = [&](const rb::SeedLists &lists, const rb::KeptCalls &kc, const std::vector<size_t> &first, const std::vector<int> &cut_pos,
                       const std::vector<rb::Cursor2> &start_cursor, const std::vector<uint32_t> &order, size_t device_limit, const std::function<void(uint32_t *, const uint32_t *)> &meanwhile,
                       std::vector<rb::AnchoredDevicePass::RangeResult> &ranges, std::vector<rb::AnchoredDevicePass::LogEntry> &undo, std::vector<rb::AnchoredDevicePass::LogEntry> &reads,
                       std::vector<rb::AnchoredDevicePass::HeadEntry> &heads) {
            if (bind_device(h)) return false;
            if (d_calls.ensure(std::max<size_t>(kc.n, 1)) || d_pend.ensure(std::max<size_t>(kc.n, 1)) || d_xa.ensure(nm * xa_stride)) return false;
            MERGE_TRY(hipMemcpyAsync(d_calls.p, kc.calls, kc.n * sizeof(RibbitCall), hipMemcpyHostToDevice, h->stream));
            if (kc.pend) MERGE_TRY(hipMemcpyAsync(d_pend.p, kc.pend, kc.n * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
            MERGE_TRY(hipMemcpyAsync(d_xa.p, xa, nm * xa_stride * sizeof(uint32_t), hipMemcpyHostToDevice, h->stream));
            MERGE_TRY(hipStreamSynchronize(h->stream));
            DevicePassConfig cfg;
            cfg.d_xa = d_xa.p; cfg.xa_stride = (int64_t)xa_stride; cfg.m_lo = m_lo; cfg.m_hi = m_hi;
            cfg.log_cap = (size_t)knobs->log_cap;
            if (knobs->head_cap) cfg.head_cap = (uint32_t)knobs->head_cap;
            if (knobs->resident_waves) cfg.resident_waves = (uint32_t)knobs->resident_waves;
            if (knobs->max_passes) cfg.max_passes = (uint32_t)knobs->max_passes;
            return run_device_pass(h, cfg, d_calls.p, kc.pend ? d_pend.p : nullptr, lists, kc, first, cut_pos, start_cursor, order, device_limit, meanwhile, ranges, undo, reads, heads);
        };
    else      // the device declines: the host workers merge the ranges, as they do in production for whatever the device leaves
        pass.run = [](const rb::SeedLists &, const rb::KeptCalls &, const std::vector<size_t> &, const std::vector<int> &, const std::vector<rb::Cursor2> &, const std::vector<uint32_t> &, size_t,
                      const std::function<void(uint32_t *, const uint32_t *)> &, std::vector<rb::AnchoredDevicePass::RangeResult> &, std::vector<rb::AnchoredDevicePass::LogEntry> &,
                      std::vector<rb::AnchoredDevicePass::LogEntry> &, std::vector<rb::AnchoredDevicePass::HeadEntry> &) { return false; };
    rb::AnchoredPassProbe probe;
    probe.device_limit = knobs->device_limit < 0 ? SIZE_MAX : (size_t)knobs->device_limit;
    probe.only_range = knobs->only_range;
    probe.stop_after_first_pass = knobs->full == 0;
    probe.host_workers = !lanes;
    rb::MergeStats st;
    const unsigned threads = std::max(2u, rb::host_thread_count(h ? h->host_threads : 0));
    rb::merge_anchored_stage_full(sl, calls, n_calls, threads, &st, &pass, &probe);
    if (lanes) (void)hipStreamSynchronize(h->stream);      // (the buffers above are released on the way out)
    if (!probe.prepared) return fail(RIBBIT_E_STATE, "the calls could not be cut into two ranges or more");
    const size_t nr = probe.cut_pos.size();
    if (knobs->only_range >= (int64_t)nr) return fail(RIBBIT_E_ARG, "only_range %lld of %zu ranges", (long long)knobs->only_range, nr);

    auto words = [](size_t n) { return static_cast<int32_t *>(std::calloc(std::max<size_t>(n, 1), sizeof(int32_t))); };
    out->n_ranges = nr;
    out->cuts = words(nr); out->first = words(nr + 1); out->cursors0 = words(2 * nr); out->range = words(12 * nr);
    if (!out->cuts || !out->first || !out->cursors0 || !out->range) { ribbit_debug_merge_ranges_free(out); return fail(RIBBIT_E_NOMEM, "out of host memory"); }
    for (size_t k = 0; k < nr; ++k) {
        out->cuts[k] = probe.cut_pos[k]; out->first[k] = (int32_t)probe.first[k];
        out->cursors0[2 * k] = probe.start_cursor[k].perfect; out->cursors0[2 * k + 1] = probe.start_cursor[k].subst;
        out->range[12 * k] = -1;
    }
    out->first[nr] = (int32_t)probe.first[nr];
    out->ran = lanes ? (probe.device_ran ? 1 : 0) : 1;
    std::memcpy(out->caps, caps, sizeof caps);
    if (knobs->full) {
        rb::SeedVec no_dispatch;
        const int rc = give_seed_lists(sl, no_dispatch, &out->lists);
        if (rc) { ribbit_debug_merge_ranges_free(out); return rc; }
        const int32_t dm[5] = {(int32_t)st.device_ranges, (int32_t)st.device_bailed, (int32_t)st.device_host_share, (int32_t)st.ranges, (int32_t)st.ranges_redone};
        std::memcpy(out->device_merge, dm, sizeof dm);
        return RIBBIT_OK;
    }
    if (!out->ran || probe.ranges.size() != nr) return RIBBIT_OK;
    size_t n_own = 0, n_undo = 0, n_reads = 0, n_heads = 0;
    for (const rb::AnchoredPassProbe::Range &r : probe.ranges) { n_own += r.own.size(); n_undo += r.undo.size(); n_reads += r.reads.size(); n_heads += r.heads.size(); }
    out->own = static_cast<RibbitSeed *>(std::calloc(std::max<size_t>(n_own, 1), sizeof(RibbitSeed)));
    out->undo = words(4 * n_undo); out->reads = words(4 * n_reads); out->heads = words(8 * n_heads);
    if (!out->own || !out->undo || !out->reads || !out->heads) { ribbit_debug_merge_ranges_free(out); return fail(RIBBIT_E_NOMEM, "out of host memory"); }
    for (size_t k = 0; k < nr; ++k) {
        const rb::AnchoredPassProbe::Range &r = probe.ranges[k];
        int32_t *o = out->range + 12 * k;
        o[0] = (int32_t)r.status; o[1] = (int32_t)out->n_own; o[2] = (int32_t)r.own.size();
        o[3] = (int32_t)(uint32_t)((uint64_t)r.guard_hits & 0xffffffffu); o[4] = (int32_t)(uint32_t)((uint64_t)r.guard_hits >> 32);
        o[5] = r.cursor.perfect; o[6] = r.cursor.subst;
        o[7] = (int32_t)(uint32_t)r.head_reads[0]; o[8] = (int32_t)(uint32_t)(r.head_reads[0] >> 32);
        o[9] = (int32_t)(uint32_t)r.head_reads[1]; o[10] = (int32_t)(uint32_t)(r.head_reads[1] >> 32);
        if (!r.own.empty()) std::memcpy(out->own + out->n_own, r.own.data(), r.own.size() * sizeof(RibbitSeed));
        out->n_own += r.own.size();
        for (const rb::AnchoredDevicePass::LogEntry &e : r.undo) { int32_t *w = out->undo + 4 * out->n_undo++; w[0] = (int32_t)e.range; w[1] = (int32_t)e.list; w[2] = (int32_t)e.index; w[3] = e.value; }
        for (const rb::AnchoredDevicePass::LogEntry &e : r.reads) { int32_t *w = out->reads + 4 * out->n_reads++; w[0] = (int32_t)e.range; w[1] = (int32_t)e.list; w[2] = (int32_t)e.index; w[3] = e.value; }
        for (const rb::AnchoredDevicePass::HeadEntry &e : r.heads) {
            int32_t *w = out->heads + 8 * out->n_heads++;
            w[0] = (int32_t)e.range; w[1] = (int32_t)e.list; w[2] = (int32_t)e.index; w[3] = e.value.start; w[4] = e.value.end; w[5] = e.value.mlen; w[6] = e.value.type; w[7] = e.changed_then ? 1 : 0;
        }
    }
    return RIBBIT_OK;
}); }

}  // extern "C"
