// api_perfect.cpp -- the perfect stage (a3, a4) and its chunk form; see api_internal.h for the map of the files behind include/ribbit_hip.h.
// There is no CPU fallback for any scan anywhere in this library.
#include "api_internal.h"

namespace rbapi {

rb::EventSource event_source(const RibbitHandle *h) {
    rb::EventSource src;
    src.ev = h->h_events.p;
    src.segs = reinterpret_cast<const rb::Seg *>(h->chunk_table.data());
    src.segs_per_motif = h->table_ntile;
    src.nm = (size_t)(h->params.max_motif - h->params.min_motif + 1);
    src.m_lo = h->params.min_motif;
    return src;
}

// Perfect stage on the device end to end: scan kernel -> START/END events (left in their regions, never
// copied to the host) -> pairing kernels -> RibbitRun records ordered by (motif, start) -> one D2H copy
// into pinned memory.  The host only checks the counters and the pairing status.
int perfect_wait(RibbitHandle *h) {
    if (!h->copy_pending) return RIBBIT_OK;
    h->copy_pending = false;
    int rc;
    if ((rc = bind_device(h))) return rc;
    HIP_TRY(hipStreamSynchronize(h->copy_stream));
    return RIBBIT_OK;
}

// The perfect stage in two halves, so that a caller with several handles can keep one record's kernels running
// while another record's results travel to the host (each handle has its own stream):
//   perfect_enqueue: memset + scan + pairing kernels + D2H of counters and status, no synchronisation;
//   perfect_finish:  waits for those, grows the event buffer and repeats on overflow, then copies the run records.
// own_lo/own_hi/pos_offset: see rb::PairLaunch (a whole record is 0, INT64_MAX, 0).
int perfect_enqueue(RibbitHandle *h, size_t cap) {
    int rc;
    if ((rc = bind_device(h))) return rc;
    if ((rc = event_room(h, &cap, &h->pair))) return rc;
    if (h->timing) HIP_TRY(hipEventRecord(h->timers.begin[RIBBIT_TIME_GPU], h->stream));
    if ((rc = zero_counters(h))) return rc;
    const rb::PerfectLaunch pp = scan_launch_args(h, cap, RIBBIT_SCAN_PERFECT);
    if (h->timing) HIP_TRY(hipEventRecord(h->timers.begin[RIBBIT_TIME_SCAN], h->stream));
    h->rec.last_split[RIBBIT_SCAN_PERFECT] = rb::launch_scan_perfect(h->planes(), pp, h->d_events.p, h->pb.d_counters.p, h->stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(h->timers.end[RIBBIT_TIME_SCAN], h->stream));
    // Everything after the scan (nine small, latency-bound launches, later the result copy) runs on the handle's
    // own post stream: on a compute stream shared by several handles the next record's pack and scan start right
    // behind this scan instead of waiting out the pairing chain's launch gaps.
    HIP_TRY(hipStreamWaitEvent(h->copy_stream, h->timers.end[RIBBIT_TIME_SCAN], 0));
    if ((rc = enqueue_pairing(h->pb, h->pair, h->d_events.p, h->d_dense.p, cap, h->copy_stream))) return rc;
    HIP_TRY(hipEventRecord(h->ev_ready, h->copy_stream));
    return RIBBIT_OK;
}

int perfect_begin(RibbitHandle *h, int64_t own_lo, int64_t own_hi, int64_t pos_offset) {
    if (!h->loaded) return fail(RIBBIT_E_STATE, "no record loaded");
    if (h->copy_pending) { int rcw = perfect_wait(h); if (rcw) return rcw; }
    h->rec.runs_valid = h->rec.calls_valid = false;
    h->pair_pending = false;
    int rc;
    if ((rc = pair_prepare(h, h->pb, h->length, own_lo, own_hi, pos_offset, h->pair))) return rc;
    if ((rc = h->h_halves.ensure(2 * (size_t)h->pair.nm))) return rc;
    if ((rc = perfect_enqueue(h, first_event_cap(h, 1)))) return rc;
    h->pair_pending = true;
    return RIBBIT_OK;
}

// the scan in flight is complete on the device: counts known, overflow handled (the scan is run again with more room),
// pairing checked.  The run records are in d_dense, the cut ones in pb.d_halves.
int perfect_collect(RibbitHandle *h) {
    if (!h->pair_pending) return fail(RIBBIT_E_STATE, "no perfect scan in flight on this handle");
    h->pair_pending = false;
    int rc;
    if ((rc = bind_device(h))) return rc;
    Published pub;
    for (int attempt = 0;; ++attempt) {
        // wait for THIS record's kernels only: the stream may be shared with other handles whose kernels come later
        HIP_TRY(hipEventSynchronize(h->ev_ready));
        pub = read_published(h->pb);
        if (pub.worst <= h->pair.region_cap) break;
        size_t cap = 0;
        if ((rc = grow_event_cap(attempt, pub.worst, &cap)) || (rc = perfect_enqueue(h, cap))) return rc;
    }
    h->last_event_count = (int64_t)pub.produced;
    return pairing_verdict(h->pb, pub.produced, "run", &h->n_runs, &h->n_halves);
}

int perfect_finish(RibbitHandle *h, RibbitRun *dst, size_t dst_cap, RibbitRun *half_dst, size_t half_dst_cap, bool wait) {
    int rc = perfect_collect(h);
    if (rc) return rc;
    const rb::PairLaunch &pr = h->pair;
    // everything that can fail is checked before the first copy is enqueued: an error return must not leave a DMA in flight
    // into a buffer the caller may free
    if (half_dst && h->n_halves > half_dst_cap) return fail(RIBBIT_E_OVERFLOW, "%zu half records do not fit the caller's buffer of %zu", h->n_halves, half_dst_cap);
    if (dst && h->n_runs > dst_cap) return fail(RIBBIT_E_OVERFLOW, "%zu run records do not fit the caller's buffer of %zu", h->n_runs, dst_cap);
    const bool whole = pr.own_lo == 0 && pr.own_hi == INT64_MAX && pr.pos_offset == 0 && !dst;
    if (!dst) {
        if ((rc = h->h_runs.ensure(std::max<size_t>(h->n_runs, 1)))) return rc;
        dst = h->h_runs.p;
    }
    if (!half_dst) half_dst = h->h_halves.p;
    if (h->n_halves)
        HIP_TRY(hipMemcpyAsync(half_dst, h->pb.d_halves.p, h->n_halves * sizeof(RibbitRun), hipMemcpyDeviceToHost, h->copy_stream));
    h->copy_pending = h->n_halves != 0;      // from here on a failure leaves the wait to the next call on the handle
    if (h->n_runs)
        HIP_TRY(hipMemcpyAsync(dst, h->d_dense.p, h->n_runs * sizeof(RibbitRun), hipMemcpyDeviceToHost, h->copy_stream));
    if (h->timing) HIP_TRY(hipEventRecord(h->timers.end[RIBBIT_TIME_GPU], h->copy_stream));
    h->timers.have[RIBBIT_TIME_SCAN] = h->timers.have[RIBBIT_TIME_GPU] = h->timing;
    h->host_ms = 0.0;
    h->rec.runs_valid = whole;
    h->copy_pending = true;
    return wait ? perfect_wait(h) : RIBBIT_OK;
}

int run_perfect_scan_range(RibbitHandle *h, int64_t own_lo, int64_t own_hi, int64_t pos_offset, RibbitRun *dst, size_t dst_cap,
                           RibbitRun *half_dst, size_t half_dst_cap) {
    if (!h->loaded) return fail(RIBBIT_E_STATE, "no record loaded");
    const bool whole = own_lo == 0 && own_hi == INT64_MAX && pos_offset == 0 && !dst;
    if (whole && h->rec.runs_valid) return RIBBIT_OK;
    int rc = perfect_begin(h, own_lo, own_hi, pos_offset);
    if (rc) return rc;
    return perfect_finish(h, dst, dst_cap, half_dst, half_dst_cap);
}

int run_perfect_scan(RibbitHandle *h) { return run_perfect_scan_range(h, 0, INT64_MAX, 0, nullptr, 0); }

int build_perfect_calls(RibbitHandle *h) {
    if (h->rec.calls_valid) return RIBBIT_OK;
    int rc = run_perfect_scan(h);
    if (rc) return rc;
    rb::perfect_calls_from_runs(h->h_runs.p, h->n_runs, h->length, h->min_shift, h->perfect_calls);
    h->rec.calls_valid = true;
    return RIBBIT_OK;
}

int advance_to_perfect(RibbitHandle *h) {
    if (h->rec.stage_done >= STAGE_PERFECT) return RIBBIT_OK;
    const double t0 = now_ms();
    int rc = build_perfect_calls(h);
    if (rc) return rc;
    const double t1 = now_ms();
    h->lists.perfect.clear();
    for (const RibbitCall &c : h->perfect_calls) rb::perfect_add(h->lists, c.start, c.end, c.mlen);
    h->rec.stage_done = STAGE_PERFECT;
    const bool profile = rb::profile_on();
    if (profile) std::fprintf(stderr, "[perfect stage] scan, pairing, runs and planes to the host, calls %.1f ms; merge of %zu calls into %zu seeds on one thread %.1f ms\n",
                              t1 - t0, h->perfect_calls.size(), h->lists.perfect.size(), now_ms() - t1);
    return RIBBIT_OK;
}

}  // namespace rbapi

extern "C" {

int ribbit_hip_scan_perfect_runs(RibbitHandle *h, const RibbitRun **out, size_t *n) { return guarded("the perfect stage", [&]() -> int {
    if (!h || !out || !n) return fail(RIBBIT_E_ARG, "null argument");
    h->rec.runs_valid = false;   // an explicit scan call always relaunches the kernel
    h->rec.calls_valid = false;
    int rc = run_perfect_scan(h);
    if (rc) return rc;
    *out = h->h_runs.p;
    *n = h->n_runs;
    return RIBBIT_OK;
}); }

int ribbit_hip_perfect_calls(RibbitHandle *h, const RibbitCall **out, size_t *n) { return guarded("the perfect stage", [&]() -> int {
    if (!h || !out || !n) return fail(RIBBIT_E_ARG, "null argument");
    if (!h->loaded) return fail(RIBBIT_E_STATE, "no record loaded");
    int rc = build_perfect_calls(h);
    if (rc) return rc;
    *out = h->perfect_calls.data();
    *n = h->perfect_calls.size();
    return RIBBIT_OK;
}); }

int ribbit_hip_seeds_perfect(RibbitHandle *h, const RibbitSeed **out, size_t *n) { return guarded("the perfect stage", [&]() -> int {
    if (!h || !out || !n) return fail(RIBBIT_E_ARG, "null argument");
    if (!h->loaded) return fail(RIBBIT_E_STATE, "no record loaded");
    if (h->rec.stage_done > STAGE_PERFECT) return fail(RIBBIT_E_STATE, "a later stage already re-typed the perfect list; reload the record");
    int rc = advance_to_perfect(h);
    if (rc) return rc;
    *out = h->lists.perfect.data();
    *n = h->lists.perfect.size();
    return RIBBIT_OK;
}); }

int ribbit_hip_perfect_runs_partial(RibbitHandle *h, int64_t own_lo, int64_t own_hi, int64_t pos_offset,
                                    const RibbitRun **runs, size_t *n_runs, const uint64_t **halves, size_t *n_halves) { return guarded("the perfect stage", [&]() -> int {
    if (!h || !runs || !n_runs || !halves || !n_halves) return fail(RIBBIT_E_ARG, "null argument");
    if (!h->loaded) return fail(RIBBIT_E_STATE, "no record loaded");
    int rc = collect_perfect_events(h);
    if (rc) return rc;
    h->rec.runs_valid = h->rec.calls_valid = false;
    const double t0 = now_ms();
    std::string why;
    if (!rb::pair_perfect_runs_partial(event_source(h), own_lo, own_hi, pos_offset, h->runs, h->export_events, &why))
        return fail(RIBBIT_E_INTERNAL, "%s", why.c_str());
    h->host_ms = now_ms() - t0;
    *runs = h->runs.data();
    *n_runs = h->runs.size();
    *halves = h->export_events.data();
    *n_halves = h->export_events.size();
    return RIBBIT_OK;
}); }

int ribbit_hip_scan_perfect_chunk(RibbitHandle *h, int64_t own_lo, int64_t own_hi, int64_t pos_offset, RibbitRun *dst, size_t dst_cap,
                                  RibbitRun *half_dst, size_t half_dst_cap, const RibbitRun **out, size_t *n,
                                  const RibbitRun **halves, size_t *n_halves) { return guarded("the perfect stage", [&]() -> int {
    if (!h || !out || !n || !halves || !n_halves) return fail(RIBBIT_E_ARG, "null argument");
    if (own_lo < 0 || own_hi < own_lo) return fail(RIBBIT_E_ARG, "bad own range");
    int rc = run_perfect_scan_range(h, own_lo, own_hi, pos_offset, dst, dst_cap, half_dst, half_dst_cap);
    if (rc) return rc;
    *out = dst ? dst : h->h_runs.p;
    *n = h->n_runs;
    *halves = half_dst ? half_dst : h->h_halves.p;
    *n_halves = h->n_halves;
    return RIBBIT_OK;
}); }

int ribbit_hip_scan_perfect_begin(RibbitHandle *h, int64_t own_lo, int64_t own_hi, int64_t pos_offset) { return guarded("the perfect stage", [&]() -> int {
    if (!h) return fail(RIBBIT_E_ARG, "null argument");
    if (own_lo < 0 || own_hi < own_lo) return fail(RIBBIT_E_ARG, "bad own range");
    return perfect_begin(h, own_lo, own_hi, pos_offset);
}); }

int ribbit_hip_scan_perfect_end_device(RibbitHandle *h, const void **dev_runs, size_t *n, const void **dev_halves, size_t *n_halves) { return guarded("the perfect stage", [&]() -> int {
    if (!h || !dev_runs || !n || !dev_halves || !n_halves) return fail(RIBBIT_E_ARG, "null argument");
    int rc = perfect_collect(h);
    if (rc) return rc;
    h->rec.runs_valid = false;
    h->timers.have[RIBBIT_TIME_SCAN] = h->timing;
    h->timers.have[RIBBIT_TIME_GPU] = false;
    *dev_runs = h->d_dense.p;
    *n = h->n_runs;
    *dev_halves = h->pb.d_halves.p;
    *n_halves = h->n_halves;
    return RIBBIT_OK;
}); }

int ribbit_hip_scan_perfect_wait(RibbitHandle *h) { return guarded("the perfect stage", [&]() -> int {
    if (!h) return fail(RIBBIT_E_ARG, "null argument");
    return perfect_wait(h);
}); }

int ribbit_hip_scan_perfect_end(RibbitHandle *h, RibbitRun *dst, size_t dst_cap, RibbitRun *half_dst, size_t half_dst_cap,
                                int wait, const RibbitRun **out, size_t *n, const RibbitRun **halves, size_t *n_halves) { return guarded("the perfect stage", [&]() -> int {
    if (!h || !out || !n) return fail(RIBBIT_E_ARG, "null argument");
    int rc = perfect_finish(h, dst, dst_cap, half_dst, half_dst_cap, wait != 0);
    if (rc) return rc;
    *out = dst ? dst : h->h_runs.p;
    *n = h->n_runs;
    if (halves) *halves = half_dst ? half_dst : h->h_halves.p;
    if (n_halves) *n_halves = h->n_halves;
    return RIBBIT_OK;
}); }

int ribbit_hip_debug_pair_events(RibbitHandle *h, const uint64_t *events, size_t n, int64_t length, RibbitRun *runs, size_t runs_cap,
                                 size_t *n_runs, uint32_t *flags) { return guarded("the pairing of the events", [&]() -> int {
    if (!h || (n && !events) || !n_runs || !flags || (runs_cap && !runs)) return fail(RIBBIT_E_ARG, "null argument");
    if (length < 0 || n > ((size_t)1 << 24)) return fail(RIBBIT_E_ARG, "bad size");
    int rc;
    if ((rc = bind_device(h))) return rc;
    rb::PairLaunch pr{};
    PairBufs pb;
    if ((rc = pair_prepare(h, pb, length, 0, INT64_MAX, 0, pr))) return rc;
    pr.region_cap = (uint32_t)std::max<size_t>(n, 1);                  // the whole stream sits in region 0
    const size_t cap = (size_t)pr.region_cap * rb::EV_SHARDS;
    DevBuf<uint64_t> d_ev, d_runs;
    if ((rc = d_ev.ensure(cap)) || (rc = d_runs.ensure(cap))) return rc;
    std::vector<uint32_t> counters(rb::EV_COUNTER_WORDS, 0);
    counters[0] = (uint32_t)n;
    if (n) HIP_TRY(hipMemcpy(d_ev.p, events, n * sizeof(uint64_t), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(pb.d_counters.p, counters.data(), counters.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    if ((rc = enqueue_pairing(pb, pr, d_ev.p, d_runs.p, cap, h->stream))) return rc;
    HIP_TRY(hipStreamSynchronize(h->stream));
    const uint32_t *status = pb.h_pub.p + rb::EV_SHARDS;
    *flags = status[rb::PAIR_FLAGS];
    *n_runs = status[rb::PAIR_TOTAL];
    const size_t take = std::min(*n_runs, runs_cap);
    if (take) HIP_TRY(hipMemcpy(runs, d_runs.p, take * sizeof(RibbitRun), hipMemcpyDeviceToHost));
    return RIBBIT_OK;
}); }

int ribbit_hip_debug_pair_events_sharded(RibbitHandle *h, const uint64_t *events, const uint32_t *counters, size_t region_cap,
                                         int64_t length, int64_t own_lo, int64_t own_hi, int64_t pos_offset, RibbitDebugPairing *out) {
    return guarded("the pairing of the events", [&]() -> int {
    if (!h || !events || !counters || !out) return fail(RIBBIT_E_ARG, "null argument");
    if ((out->runs_cap && !out->runs) || (out->halves_cap && !out->halves) || (out->dense_cap && !out->dense) || (out->table_cap && !out->table))
        return fail(RIBBIT_E_ARG, "null argument");
    if (length < 0 || region_cap < 1 || region_cap * rb::EV_SHARDS > ((size_t)1 << 24)) return fail(RIBBIT_E_ARG, "bad size");
    if (own_lo < 0 || own_hi < own_lo) return fail(RIBBIT_E_ARG, "bad own range");
    int rc;
    if ((rc = bind_device(h))) return rc;
    rb::PairLaunch pr{};
    PairBufs pb;
    if ((rc = pair_prepare(h, pb, length, own_lo, own_hi, pos_offset, pr))) return rc;
    pr.region_cap = (uint32_t)region_cap;
    const size_t cap = region_cap * rb::EV_SHARDS, entries = (size_t)pr.nm * pr.ntile;
    DevBuf<uint64_t> d_ev, d_dense;                                     // d_dense: the run records, then the dense stream (as the handle's)
    if ((rc = d_ev.ensure(cap)) || (rc = d_dense.ensure(cap))) return rc;
    std::vector<uint32_t> words(rb::EV_COUNTER_WORDS, 0);
    for (int t = 0; t < rb::EV_SHARDS; ++t) words[(size_t)t * rb::EV_COUNTER_STRIDE] = counters[t];
    HIP_TRY(hipMemcpy(d_ev.p, events, cap * sizeof(uint64_t), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(pb.d_counters.p, words.data(), words.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    if ((rc = enqueue_pairing(pb, pr, d_ev.p, d_dense.p, cap, h->stream))) return rc;
    HIP_TRY(hipStreamSynchronize(h->stream));
    std::copy(pb.h_pub.p, pb.h_pub.p + rb::EV_SHARDS, out->published);
    std::copy(pb.h_pub.p + rb::EV_SHARDS, pb.h_pub.p + rb::EV_SHARDS + 3, out->status);
    const size_t n_runs = std::min({(size_t)out->status[rb::PAIR_TOTAL], out->runs_cap, cap / 2});
    const size_t n_halves = std::min({(size_t)out->status[rb::PAIR_HALVES], out->halves_cap, 2 * (size_t)pr.nm});
    if (n_runs) HIP_TRY(hipMemcpy(out->runs, d_dense.p, n_runs * sizeof(RibbitRun), hipMemcpyDeviceToHost));
    if (n_halves) HIP_TRY(hipMemcpy(out->halves, pb.d_halves.p, n_halves * sizeof(RibbitRun), hipMemcpyDeviceToHost));
    // the legacy pair, as collect_perfect_events runs it
    rb::launch_compact_events(d_ev.p, (uint32_t)cap, pb.d_counters.p, d_dense.p, h->stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(rb::launch_chunk_table(d_dense.p, pb.d_counters.p, pr.m_lo, pr.nm, pr.ntile, pr.tile_bases, pb.d_pair_table.p, pb.d_pair_status.p, h->stream));
    HIP_TRY(hipMemcpyAsync(words.data(), pb.d_counters.p, words.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipMemcpyAsync(&out->table_status, pb.d_pair_status.p, sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    out->summary = words[rb::EV_SUMMARY];
    out->overflow = words[rb::EV_SUMMARY + 1];
    const size_t n_dense = std::min({(size_t)out->summary, out->dense_cap, cap}), n_table = std::min(entries, out->table_cap);
    if (n_dense) HIP_TRY(hipMemcpy(out->dense, d_dense.p, n_dense * sizeof(uint64_t), hipMemcpyDeviceToHost));
    if (n_table) HIP_TRY(hipMemcpy(out->table, pb.d_pair_table.p, n_table * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return RIBBIT_OK;
}); }

int ribbit_host_perfect_runs_from_events(const RibbitScanParams *params, size_t nparts, const uint64_t *events,
                                         const uint64_t *counts, RibbitRun **runs, size_t *n) { return guarded("the pairing of the events", [&]() -> int {
    if (!params || !counts || !runs || !n) return fail(RIBBIT_E_ARG, "null argument");
    const size_t nm = (size_t)(params->max_motif - params->min_motif + 1);
    std::vector<rb::Seg> segs(nm * nparts, rb::Seg{0, 0});
    uint64_t off = 0;
    for (size_t p = 0; p < nparts; ++p)
        for (size_t mi = 0; mi < nm; ++mi) { segs[mi * nparts + p] = rb::Seg{(uint32_t)off, (uint32_t)counts[p * nm + mi]}; off += counts[p * nm + mi]; }
    rb::EventSource src;
    src.ev = events; src.segs = segs.data(); src.segs_per_motif = nparts; src.nm = nm; src.m_lo = params->min_motif;
    std::vector<RibbitRun> out;
    std::string why;
    if (!rb::pair_perfect_runs(src, out, &why)) return fail(RIBBIT_E_INTERNAL, "perfect events: %s", why.c_str());
    *n = out.size();
    *runs = (RibbitRun *)std::malloc(std::max<size_t>(out.size(), 1) * sizeof(RibbitRun));
    if (!*runs) return fail(RIBBIT_E_NOMEM, "out of host memory");
    if (!out.empty()) std::memcpy(*runs, out.data(), out.size() * sizeof(RibbitRun));
    return RIBBIT_OK;
}); }

void ribbit_runs_free(RibbitRun *runs) { std::free(runs); }

}  // extern "C"
