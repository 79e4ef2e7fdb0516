// api_window.cpp -- the substitution and anchored stages (a6-a12); see api_internal.h for the map of the files behind include/ribbit_hip.h.
// There is no CPU fallback for any scan anywhere in this library.
#include "api_internal.h"

namespace rbapi {

// ---- window stages on the device ---------------------------------------------------------------------
// scan kernel -> pass-streak START / END events (left in their regions) -> pairing kernels -> one 16-byte record per
// streak, motif-major by start, in d_dense: the event pass of api_events.cpp around the window scan (1 mismatch) of
// RIBBIT_STAGE_SUBST or the two kernels of RIBBIT_STAGE_ANCHORED.
// filter (anchored scan only): groups of pass-streaks whose call cannot pass min_span leave no events (kernels.hip, "group
// filter"); their ends are left in h->d_dropmap for window_stage_device.
int scan_and_pair_streaks(RibbitHandle *h, int stage, uint32_t *n_streaks, int (*filter_min_span)(int)) {
    int rc;
    if ((rc = bind_device(h))) return rc;
    if (h->copy_pending && (rc = perfect_wait(h))) return rc;      // d_dense / d_events are shared with the perfect stage
    // the anchored stage runs as two kernels: the planes (anchors + composition), then the window scan of the planes (kernels.hip).
    // (The fused form of rounds 1-2 -- 256 VGPRs, two waves per SIMD, 3.3 against 2.3 ms per 100 Mbp -- is gone from the product
    // since round 4; DESIGN.md 4 has its measurements.)
    const bool subst = stage == RIBBIT_STAGE_SUBST;
    RibbitHandle::WindowStage &st = h->win[stage];
    rb::PairLaunch pr{};
    if ((rc = pair_prepare(h, h->pb, h->length, 0, INT64_MAX, 0, pr))) return rc;
    const bool filter = !subst && filter_min_span != nullptr && std::getenv("RIBBIT_NO_GROUP_FILTER") == nullptr;
    // typical event densities on repeat-rich sequence: 0.25 per base (1-mismatch windows); anchored windows 3.7 at 99 motif
    // sizes without the group filter (growing with the motif sizes), and 1.3 (99 sizes) .. 1.6 (499) with it: the filter drops
    // nearly everything the large motifs add.  A too small first guess costs a second launch of the window scan; a too large
    // one costs memory -- until round 4 the filtered scan was sized like the unfiltered one, which at -M 500 meant 2 x 34 GB for
    // 3.3 GB of events, and on a box whose memory had just been used two seconds of the driver clearing it.
    // (1-mismatch windows at 499 motif sizes: 0.49 per base, and the profile of round 4 showed the scan launched twice)
    size_t cap = first_event_cap(h, subst ? std::max<size_t>(2, pr.nm / 100) : filter ? 10 : std::max<size_t>(16, pr.nm / 6));
    const rb::DevicePlanes pl = h->planes();
    Published pub;
    bool first_attempt_fit = false;
    h->dropmap_valid = false;
    if (filter) {
        // positions a group must span for its call to be able to pass: the call's length is the group's span + 7
        std::vector<int32_t> tj(pr.nm);
        for (uint32_t mi = 0; mi < pr.nm; ++mi) {
            const int t = std::min(filter_min_span((int)(pr.m_lo + mi)), rb::GROUP_FILTER_MAX + 7) - 7;
            tj[mi] = t > 1 ? t : 0;
        }
        if ((rc = h->d_tj.ensure(pr.nm)) || (rc = h->d_dropmap.ensure(dropmap_words(h->length)))) return rc;
        HIP_TRY(hipMemcpyAsync(h->d_tj.p, tj.data(), pr.nm * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));       // tj is a local
    }
    for (int attempt = 0;; ++attempt) {
        if ((rc = event_room(h, &cap, &pr))) return rc;
        if (filter) HIP_TRY(hipMemsetAsync(h->d_dropmap.p, 0, dropmap_words(h->length) * sizeof(uint32_t), h->stream));
        HIP_TRY(hipEventRecord(h->timers.begin[RIBBIT_TIME_GPU], h->stream));
        if ((rc = zero_counters(h))) return rc;
        HIP_TRY(hipEventRecord(h->timers.begin[RIBBIT_TIME_SCAN], h->stream));
        // (two-kernel anchored stage: the planes kernel runs on the first attempt only, so the stage's start mark stays where it
        // was put then -- timer RIBBIT_TIME_ANCHORED_SCAN is "both kernels", also when the window scan had to run again with more room)
        if (attempt == 0 || subst) HIP_TRY(hipEventRecord(st.ev_begin, h->stream));
        if (subst) {
            h->rec.last_split[RIBBIT_SCAN_SUBST] = rb::launch_scan_window(pl, scan_launch_args(h, cap, RIBBIT_SCAN_SUBST), 1, h->d_events.p, h->pb.d_counters.p, h->stream);
        } else {
            if (attempt == 0) {          // the planes do not depend on the event capacity: once
                h->rec.last_split[RIBBIT_SCAN_ANCHORED] = rb::launch_scan_anchored(pl, scan_launch_args(h, cap, RIBBIT_SCAN_ANCHORED), h->d_xa.p, h->xa_stride, h->stream);
                HIP_TRY(hipGetLastError());
                HIP_TRY(hipEventRecord(h->ev_planes, h->stream));
            }
            h->rec.last_split[RIBBIT_SCAN_XA_WINDOW] = rb::launch_scan_xa_window(pl, scan_launch_args(h, cap, RIBBIT_SCAN_XA_WINDOW), h->d_xa.p, h->xa_stride, h->d_events.p,
                                                                            h->pb.d_counters.p, filter ? h->d_tj.p : nullptr, filter ? h->d_dropmap.p : nullptr, h->stream);
        }
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(h->timers.end[RIBBIT_TIME_SCAN], h->stream));
        HIP_TRY(hipEventRecord(st.ev_end, h->stream));
        st.have_timing = true;
        if ((rc = enqueue_pairing(h->pb, pr, h->d_events.p, h->d_dense.p, cap, h->stream))) return rc;
        HIP_TRY(hipStreamSynchronize(h->stream));
        pub = read_published(h->pb);
        if (pub.worst <= pr.region_cap) { first_attempt_fit = attempt == 0; break; }
        if ((rc = grow_event_cap(attempt, pub.worst, &cap))) return rc;
    }
    h->timers.have[RIBBIT_TIME_SCAN] = true;
    h->last_event_count = (int64_t)pub.produced;
    size_t n = 0, n_cut = 0;
    if ((rc = pairing_verdict(h->pb, pub.produced, "streak", &n, &n_cut))) return rc;
    if (n_cut) return fail(RIBBIT_E_INTERNAL, "streak cut by the own range of a whole record");
    *n_streaks = (uint32_t)n;
    h->last_streaks = (int64_t)n;
    h->dropmap_valid = filter;
    if (!subst) h->planes_timing_valid = first_attempt_fit;
    return RIBBIT_OK;
}

// The window stage behind the scan and the pairing (window_stage.hip): from the n streak records in d_dense (motif-major by
// start; d_events and d_dense sized by the event pass for them) to the calls on the host.  full: every call, unfiltered;
// otherwise only the calls that pass min_span[motif - min_motif], with their cursor bounds.  cw: chunk mode.  dropmap_valid:
// d_dropmap holds the ends of the groups a filtered scan dropped.  first_edge_cap: first capacity of the edge-call list
// (0: what the list has, 65 536 or a sixteenth of the streaks, whichever is largest); a list that overflows is sized by the
// count and the calls kernel runs again.  scan_ms: what the scan and the pairing took, for the RIBBIT_PROFILE line.
int window_calls_device(RibbitHandle *h, int stage, uint32_t n, bool full, const int32_t *min_span, ChunkWindow *cw, bool dropmap_valid,
                        size_t first_edge_cap, double scan_ms, DeviceCalls *out) {
    int rc;
    PinnedBuf<RibbitCall> &h_calls = h->win[stage].h_calls, &h_flush = h->win[stage].h_flush;
    PinnedBuf<int32_t> &h_pend = h->win[stage].h_pend;
    PinnedBuf<uint32_t> &h_ws = h->win[stage].h_ws;
    const bool profile = rb::profile_on();
    const double t0 = now_ms();
    const uint32_t nm = (uint32_t)(h->params.max_motif - h->params.min_motif + 1);
    const uint32_t n_words = (uint32_t)(h->length / 32 + 1);
    int key_bits = 10;
    while (((int64_t)1 << (key_bits - 10)) <= h->length + 8) ++key_bits;
    size_t scratch = rb::window_stage_scratch_bytes(n, n_words, n, std::max<size_t>(n / 16, (size_t)1 << 16), key_bits);
    if ((rc = h->d_scratch.ensure(scratch))) return rc;
    if ((rc = h->d_word_tmp.ensure(n_words + 1))) return rc;
    if (!h->rec.eval_valid) {
        if ((rc = h->d_eval.ensure(n_words + 1))) return rc;
        if ((rc = h->d_first_rev.ensure(n_words + 1))) return rc;
        HIP_TRY(rb::launch_eval_planes(h->d_brk.p + rb::LEAD_WORDS, n_words, h->d_eval.p, h->d_first_rev.p, h->d_word_tmp.p, h->d_scratch.p, h->d_scratch.cap, h->stream));
        HIP_TRY(hipGetLastError());
        h->rec.eval_valid = true;
    }
    if ((rc = h->d_group.ensure(std::max<size_t>(n, 1)))) return rc;
    const RibbitRun *runs = reinterpret_cast<const RibbitRun *>(h->d_dense.p);
    HIP_TRY(rb::launch_group_starts(runs, n, (uint32_t)h->params.min_motif, h->d_group.p, h->d_scratch.p, h->d_scratch.cap, h->stream));
    HIP_TRY(hipGetLastError());
    // length filter of the stage (seedlen_cutoffs), per motif
    std::vector<int32_t> spans(nm, 0);
    if (!full) spans.assign(min_span, min_span + nm);
    if ((rc = h->d_min_span.ensure(nm))) return rc;
    HIP_TRY(hipMemcpyAsync(h->d_min_span.p, spans.data(), nm * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
    if ((rc = h->d_flush.ensure(nm))) return rc;
    if ((rc = h->d_ws_counters.ensure(rb::WS_WORDS))) return rc;
    if ((rc = h->d_bitmap.ensure(n_words + 1))) return rc;
    if ((rc = h_ws.ensure(rb::WS_WORDS))) return rc;
    if ((rc = h_flush.ensure(nm))) return rc;
    size_t edge_cap = first_edge_cap ? first_edge_cap : std::max<size_t>(h->d_edge_keys.cap, std::max<size_t>((size_t)1 << 16, n / 16));
    // the events are spent: their buffer (2 x 8 bytes per streak at least) receives the unsorted calls
    uint64_t *keys = h->d_events.p, *vals = h->d_events.p + h->d_events.cap / 2;
    uint32_t n_main = 0, n_edge = 0;
    for (int attempt = 0;; ++attempt) {
        if (!full) {
            if ((rc = h->d_edge_keys.ensure(edge_cap)) || (rc = h->d_edge_vals.ensure(edge_cap))) return rc;
            HIP_TRY(hipMemsetAsync(h->d_bitmap.p, 0, ((size_t)n_words + 1) * sizeof(uint32_t), h->stream));
        }
        HIP_TRY(hipMemsetAsync(h->d_flush.p, 0, nm * sizeof(RibbitCall), h->stream));
        HIP_TRY(hipMemsetAsync(h->d_ws_counters.p, 0, rb::WS_WORDS * sizeof(uint32_t), h->stream));
        rb::WindowCallsLaunch w{};
        w.runs = runs; w.n_streaks = n; w.group = h->d_group.p;
        w.eval = h->d_eval.p; w.first_rev = h->d_first_rev.p; w.brk = h->d_brk.p + rb::LEAD_WORDS; w.n_words = n_words;
        w.length = h->length; w.m_lo = (uint32_t)h->params.min_motif; w.nm = nm; w.min_span = h->d_min_span.p; w.full = full ? 1 : 0;
        w.keys = keys; w.vals = vals; w.cap = (uint32_t)(h->d_events.cap / 2);
        w.edge_keys = h->d_edge_keys.p; w.edge_vals = h->d_edge_vals.p; w.edge_cap = full ? 0u : (uint32_t)edge_cap;
        w.flush = h->d_flush.p; w.bitmap = h->d_bitmap.p; w.counters = h->d_ws_counters.p;
        if (cw) { w.own_lo = cw->own_lo; w.own_hi = cw->own_hi; w.z_lo = cw->z_lo; w.keep_flush = cw->keep_flush ? 1 : 0; }
        rb::launch_window_calls(w, h->stream);
        HIP_TRY(hipGetLastError());
        if (dropmap_valid && !full) {
            rb::launch_merge_dropmap(h->d_dropmap.p, (uint32_t)dropmap_words(h->length), n_words, w.own_lo, w.own_hi, h->d_bitmap.p,
                                     h->d_ws_counters.p, h->stream);
            HIP_TRY(hipGetLastError());
        }
        HIP_TRY(hipMemcpyAsync(h_ws.p, h->d_ws_counters.p, rb::WS_WORDS * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipMemcpyAsync(h_flush.p, h->d_flush.p, nm * sizeof(RibbitCall), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));
        n_main = h_ws.p[rb::WS_N_MAIN];
        n_edge = h_ws.p[rb::WS_N_EDGE];
        if (n_edge <= edge_cap || full) break;
        if (attempt == 1) return fail(RIBBIT_E_INTERNAL, "edge-call list overflow");
        edge_cap = (size_t)n_edge + 1024;
    }
    const double t_calls = now_ms();
    uint32_t wflags = h_ws.p[rb::WS_FLAGS];
    if (wflags) return fail(RIBBIT_E_INTERNAL, "window state machine on the device failed (flags 0x%x)", wflags);
    if (cw) cw->inexact = h_ws.p[rb::WS_INEXACT] != 0;
    const int32_t pos_offset = cw ? cw->pos_offset : 0;
    if (n_main > h->d_events.cap / 2) return fail(RIBBIT_E_INTERNAL, "more calls than streaks");
    // call order: scan position major, motif minor
    scratch = rb::window_stage_scratch_bytes(0, n_words, n_main, n_edge, key_bits);
    if ((rc = h->d_scratch.ensure(scratch))) return rc;
    if ((rc = h->d_sort_keys.ensure(std::max<size_t>(n_main, 1))) || (rc = h->d_sort_vals.ensure(std::max<size_t>(n_main, 1)))) return rc;
    HIP_TRY(rb::launch_sort_calls(keys, vals, h->d_sort_keys.p, h->d_sort_vals.p, n_main, key_bits, h->d_scratch.p, h->d_scratch.cap, h->stream));
    HIP_TRY(hipGetLastError());
    const bool bounds = !full && n_edge > 0 && n_main > 0;
    if (bounds) {
        if ((rc = h->d_edge_keys2.ensure(n_edge)) || (rc = h->d_edge_vals2.ensure(n_edge))) return rc;
        if ((rc = h->d_edge_tmp.ensure(n_edge)) || (rc = h->d_edge_end1.ensure(n_edge))) return rc;
        if ((rc = h->d_last_word.ensure(n_words + 1))) return rc;
        if ((rc = h->d_pend.ensure(n_main))) return rc;
        HIP_TRY(rb::launch_sort_calls(h->d_edge_keys.p, h->d_edge_vals.p, h->d_edge_keys2.p, h->d_edge_vals2.p, n_edge, key_bits, h->d_scratch.p, h->d_scratch.cap, h->stream));
        HIP_TRY(hipMemsetAsync(h->d_pend.p, 0xff, (size_t)n_main * sizeof(int32_t), h->stream));
        HIP_TRY(rb::launch_edge_bounds(h->d_edge_keys2.p, h->d_edge_vals2.p, n_edge, h->d_edge_tmp.p, h->d_edge_end1.p, h->d_bitmap.p, h->d_word_tmp.p,
                                       h->d_last_word.p, n_words, h->d_sort_keys.p, n_main, h->d_pend.p, h->d_ws_counters.p, pos_offset, h->d_scratch.p, h->d_scratch.cap, h->stream));
        HIP_TRY(hipGetLastError());
    }
    // 16-byte call records for the host; the streak records are spent, their buffer takes them
    RibbitCall *d_calls = reinterpret_cast<RibbitCall *>(h->d_dense.p);
    rb::launch_assemble_calls(h->d_sort_keys.p, h->d_sort_vals.p, n_main, d_calls, pos_offset, h->stream);
    HIP_TRY(hipGetLastError());
    if ((rc = h_calls.ensure(std::max<size_t>(n_main, 1)))) return rc;
    if (n_main) HIP_TRY(hipMemcpyAsync(h_calls.p, d_calls, (size_t)n_main * sizeof(RibbitCall), hipMemcpyDeviceToHost, h->stream));
    if (bounds) {
        if ((rc = h_pend.ensure(n_main))) return rc;
        HIP_TRY(hipMemcpyAsync(h_pend.p, h->d_pend.p, (size_t)n_main * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipMemcpyAsync(h_ws.p, h->d_ws_counters.p, rb::WS_WORDS * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
    }
    HIP_TRY(hipEventRecord(h->timers.end[RIBBIT_TIME_GPU], h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    h->timers.have[RIBBIT_TIME_GPU] = true;
    wflags = h_ws.p[rb::WS_FLAGS];
    if (wflags) return fail(RIBBIT_E_INTERNAL, "cursor bounds of the edge calls failed (flags 0x%x)", wflags);
    // end-of-sequence calls: at most one per motif, already in motif order; close the gaps
    size_t nf = 0;
    for (uint32_t mi = 0; mi < nm; ++mi)
        if (h_flush.p[mi].mlen != 0) {
            RibbitCall c = h_flush.p[mi];
            c.pos += pos_offset; c.start += pos_offset; c.end += pos_offset;
            h_flush.p[nf++] = c;
        }
    out->calls = h_calls.p;
    out->n = n_main;
    out->pend = bounds ? h_pend.p : nullptr;
    out->tail_pend = h_ws.p[rb::WS_MAX_END] ? (int32_t)h_ws.p[rb::WS_MAX_END] - 1 + pos_offset : -1;
    out->flush = h_flush.p;
    out->n_flush = nf;
    h->last_calls = n_main;
    h->last_edge_calls = n_edge;
    h->host_ms = now_ms() - t0;
    if (profile)
        std::fprintf(stderr, "[window stage %d%s] scan + pairing %.1f ms (%u streaks), group scan + calls kernel %.1f ms, sort + bounds + read-back %.1f ms: "
                     "%u calls, %u edge calls, %zu flush calls\n", stage, full ? " full" : "", scan_ms, n, t_calls - t0, now_ms() - t_calls, n_main, n_edge, nf);
    return RIBBIT_OK;
}

// The whole window stage on the device.  full: every call, unfiltered (the call-list entry points and the parity tests);
// otherwise only the calls that pass min_span, with their cursor bounds.  cw: chunk mode.
int window_stage_device(RibbitHandle *h, int stage, bool full, int (*min_span)(int), DeviceCalls *out, ChunkWindow *cw) {
    int rc;
    uint32_t n = 0;
    const double t_scan = now_ms();
    if ((rc = scan_and_pair_streaks(h, stage, &n, full ? nullptr : min_span))) return rc;
    std::vector<int32_t> spans((size_t)(h->params.max_motif - h->params.min_motif + 1), 0);
    if (!full) for (size_t mi = 0; mi < spans.size(); ++mi) spans[mi] = min_span(h->params.min_motif + (int)mi);
    return window_calls_device(h, stage, n, full, spans.data(), cw, h->dropmap_valid, 0, now_ms() - t_scan, out);
}

void full_calls_from_device(const DeviceCalls &dc, rb::CallVec &calls) {
    calls.resize(dc.n + dc.n_flush);
    if (dc.n) std::memcpy(calls.data(), dc.calls, dc.n * sizeof(RibbitCall));
    if (dc.n_flush) std::memcpy(calls.data() + dc.n, dc.flush, dc.n_flush * sizeof(RibbitCall));
}

// window scan (1 mismatch) + per-motif state machine, both on the device -> the addSeed call list of
// processShiftXORswithSubstitutions (parse_substitute_shiftxor.cpp:430-574)
int build_subst_calls(RibbitHandle *h) {
    if (h->rec.subst_calls_valid) return RIBBIT_OK;
    if (!h->loaded) return fail(RIBBIT_E_STATE, "no record loaded");
    DeviceCalls dc;
    int rc = window_stage_device(h, RIBBIT_STAGE_SUBST, true, nullptr, &dc);
    if (rc) return rc;
    full_calls_from_device(dc, h->subst_calls);
    h->rec.subst_calls_valid = true;
    return RIBBIT_OK;
}

// host half of the substitution stage: the merges of parse_substitute_shiftxor.cpp:18-388 over the stage's calls
void subst_merge(RibbitHandle *h, const DeviceCalls *dc) {
    const rb::HostPlanes *hp = &h->host;
    h->lists.range_count = [hp](int shift, int start, int end) { return hp->range_count(shift, start, end); };
    h->lists.subst.clear();
    const double t0 = now_ms();
    const unsigned threads = rb::host_thread_count(h->host_threads);
    rb::MergeStats st;
    if (dc) rb::merge_subst_stage(h->lists, *dc, threads, &st);
    else rb::merge_subst_stage_full(h->lists, h->subst_calls.data(), h->subst_calls.size(), threads, &st);
    h->merge_ms = now_ms() - t0;
    h->rec.stage_done = STAGE_SUBST;
    const bool profile = rb::profile_on();
    if (profile)
        std::fprintf(stderr, "[subst merge] %zu seeds: %u ranges on %u threads%s, preparation %.1f ms, merges %.1f ms\n", h->lists.subst.size(), st.ranges,
                     st.threads, st.redone_in_order ? " (REDONE IN ORDER)" : "", st.prepare_ms, st.merge_ms);
}

int advance_to_subst(RibbitHandle *h) {
    if (h->rec.stage_done >= STAGE_SUBST) return RIBBIT_OK;
    int rc = advance_to_perfect(h);
    if (rc) return rc;
    if ((rc = ensure_host_planes(h))) return rc;
    DeviceCalls dc;
    const bool full = h->rec.subst_calls_valid;      // the full call list has been asked for (ribbit_hip_subst_calls): replay that
    if (!full && (rc = window_stage_device(h, RIBBIT_STAGE_SUBST, false, rb::subst_seedlen_cutoff, &dc))) return rc;
    subst_merge(h, full ? nullptr : &dc);
    return RIBBIT_OK;
}

// The anchored stage's kernel writes the composed planes XA_m (fasta_utils.cpp:143-161) to HBM: the device-side
// refinement scans read them there, and the host merges' range reads (retainNestedSeedAnchored,
// parse_anchored_shiftxor.cpp:59-84: ~200 K per Mbp, each steering the next decision) read a host copy.  Recomputing
// the slice of a query from the packed planes instead (HostPlanes::xa_slice, what the host-only entry points do when
// they are not given the planes) costs ~0.6 us per query -- 1.4 s per 20 Mbp against 5 ms for the copy, which
// moreover runs behind the substitution stage's merge.
int prepare_anchored(RibbitHandle *h) {
    if (!h->loaded) return fail(RIBBIT_E_STATE, "no record loaded");
    if (h->params.max_motif > rb::ANCHORED_MAX_MOTIF)
        return fail(RIBBIT_E_ARG, "the anchored stage of this build supports max_motif <= %d (got %d)", rb::ANCHORED_MAX_MOTIF, h->params.max_motif);
    const size_t nm = (size_t)(h->params.max_motif - h->params.min_motif + 1);
    // whole tiles of the window kernel that reads the planes back (scan_xa_window_kernel), plus its two words of look-ahead
    h->xa_stride = (h->length / 32 + 1 + rb::TILE_WORDS - 1) / rb::TILE_WORDS * rb::TILE_WORDS + 16;
    return h->d_xa.ensure(nm * (size_t)h->xa_stride);
}

// enqueue the copy of the composed planes on the handle's copy stream (behind everything enqueued on the compute
// stream so far); xa_wait_host() makes them readable
int xa_copy_begin(RibbitHandle *h) {
    int rc;
    const size_t nm = (size_t)(h->params.max_motif - h->params.min_motif + 1);
    if ((rc = h->h_xa.ensure(nm * (size_t)h->xa_stride))) return rc;      // page-locked: the copy runs at link speed
    HIP_TRY(hipEventRecord(h->ev_xa, h->stream));
    HIP_TRY(hipStreamWaitEvent(h->copy_stream, h->ev_xa, 0));
    HIP_TRY(hipMemcpyAsync(h->h_xa.p, h->d_xa.p, nm * (size_t)h->xa_stride * sizeof(uint32_t), hipMemcpyDeviceToHost, h->copy_stream));
    HIP_TRY(hipEventRecord(h->ev_xa, h->copy_stream));
    h->xa_copy_pending = true;
    return RIBBIT_OK;
}

int xa_wait_host(RibbitHandle *h) {
    if (h->xa_copy_pending) {
        HIP_TRY(hipEventSynchronize(h->ev_xa));
        h->xa_copy_pending = false;
    }
    h->host.xa.clear();
    h->host.xa_view = h->h_xa.p;
    h->host.xa_stride = h->xa_stride;
    h->host.xa_m_lo = h->params.min_motif;
    h->host.xa_m_hi = h->params.max_motif;
    return RIBBIT_OK;
}

// fused anchored kernel (anchor planes + composition + 6-of-8 window scan) + state machine, on the device ->
// the addSeed call list of processShiftXORsAnchored (parse_anchored_shiftxor.cpp:580-723)
int build_anchored_calls(RibbitHandle *h) {
    if (h->rec.anchored_calls_valid) return RIBBIT_OK;
    int rc = prepare_anchored(h);
    if (rc) return rc;
    DeviceCalls dc;
    if ((rc = window_stage_device(h, RIBBIT_STAGE_ANCHORED, true, nullptr, &dc))) return rc;
    full_calls_from_device(dc, h->anchored_calls);
    h->rec.xa_on_device = true;
    h->rec.anchored_calls_valid = true;
    return RIBBIT_OK;
}

// processShiftXORswithSubstitutions + processShiftXORsAnchored.  All GPU work of both stages is enqueued before
// either host merge starts, so the copies (kept calls, composed planes) travel while the host merges.
// RIBBIT_PROFILE line of the anchored stage's merge (GPU path and host replay alike)
void print_anchored_merge_profile(size_t seeds, const rb::MergeStats &st, double dispatch_ms, unsigned dispatch_ranges) {
    std::fprintf(stderr, "[anchored merge] %zu seeds: %u ranges on %u threads%s, %u passes, %lld changing head writes, %u ranges done again, preparation %.1f ms (cuts %.1f, cursors %.1f, type snapshots %.1f), merges %.1f ms "
                 "(parallel passes %.1f ms over %u range runs [device pass %.1f ms for %u ranges, the host threads' share meanwhile: %u ranges in %.1f ms; results into the ranges' states %.1f ms; then %u ranges the device left]: the ranges' own times sum to %.1f ms = %.1f ms per thread, longest range %.1f ms; in-order walk %.1f ms; joining the ranges' lists %.1f ms; before the first pass %.1f ms; end-of-sequence calls %.1f ms), dispatch order %.1f ms in %u ranges\n",
                 seeds, st.ranges, st.threads, st.redone_in_order ? " (REDONE IN ORDER)" : (st.head_writes ? " (list-head writes: ranges done again, see passes)" : ""), st.passes, st.head_writes,
                 st.ranges_redone, st.prepare_ms, st.prep_parts[0], st.prep_parts[1] - st.prep_parts[0], st.prep_parts[2] - st.prep_parts[1], st.merge_ms, st.pass_ms, st.ranges_run, st.device_ms, st.device_ranges, st.device_host_share, st.device_meanwhile_ms, st.device_apply_ms, st.device_bailed, st.range_ms_sum, st.range_ms_sum / std::max(1u, st.threads), st.range_ms_max, st.walk_ms, st.concat_ms, st.before_passes_ms, st.flush_ms, dispatch_ms, dispatch_ranges);
}

// from here on "plane m" means the composed plane XA_m (fasta_utils.cpp:159) wherever hp has it: the merges' range reads, and
// the planes they may read word by word when hp stores them
void use_composed_planes(rb::SeedLists &sl, const rb::HostPlanes *hp) {
    sl.range_count = [hp](int shift, int start, int end) {
        return hp->has_xa(shift) ? hp->range_count_xa(shift, start, end) : hp->range_count(shift, start, end);
    };
    if (hp->xa_stored()) { sl.plane_words = hp->xa_words(); sl.plane_stride = hp->xa_stride; sl.plane_lo = hp->xa_m_lo; sl.plane_hi = hp->xa_m_hi; }
}

// ---- what the host-only entry points (ribbit_host_replay_calls, ribbit_host_merge_chunks) share: the caller's planes checked,
// copied into hp with the record's constants in sl, and at the end the lists handed out as malloc memory
int check_caller_planes(const RibbitScanParams *params, int64_t length, const uint32_t *hi, const uint32_t *lo, const uint32_t *brk, size_t nwords, const uint32_t *xa, size_t xa_stride) {
    if (!params || (length > 0 && (!hi || !lo || !brk))) return fail(RIBBIT_E_ARG, "null argument");
    const size_t need = (size_t)(length / 32 + 1) + (size_t)(params->max_motif + 2) / 32 + 2;
    if (nwords < need) return fail(RIBBIT_E_ARG, "planes too short: %zu words, need %zu (zero padding past the record)", nwords, need);
    if (xa && xa_stride < (size_t)(length / 32 + 1)) return fail(RIBBIT_E_ARG, "composed planes (xa) too short");
    return RIBBIT_OK;
}

void lists_over_caller_planes(const RibbitScanParams *params, int64_t length, const uint32_t *hi, const uint32_t *lo, const uint32_t *brk, size_t nwords, rb::HostPlanes &hp, rb::SeedLists &sl) {
    hp.resize(length, nwords);
    std::memcpy(hp.hi.data(), hi, nwords * sizeof(uint32_t));
    std::memcpy(hp.lo.data(), lo, nwords * sizeof(uint32_t));
    std::memcpy(hp.brk.data(), brk, nwords * sizeof(uint32_t));
    sl.length = length;
    sl.min_motif = params->min_motif;
    sl.max_motif = params->max_motif;
    sl.min_shift = (params->min_motif > 2) ? params->min_motif - 2 : 1;
    const rb::HostPlanes *p = &hp;
    sl.range_count = [p](int shift, int start, int end) { return p->range_count(shift, start, end); };
}

int give_seed_lists(const rb::SeedLists &sl, const rb::SeedVec &dispatch, RibbitSeedLists *out) {
    auto give = [](const rb::SeedVec &v, RibbitSeed **p, size_t *n) {
        *n = v.size();
        *p = (RibbitSeed *)std::malloc(std::max<size_t>(v.size(), 1) * sizeof(RibbitSeed));
        if (*p && !v.empty()) std::memcpy(*p, v.data(), v.size() * sizeof(RibbitSeed));
        return *p != nullptr;
    };
    if (!give(sl.perfect, &out->perfect, &out->n_perfect) || !give(sl.subst, &out->subst, &out->n_subst) ||
        !give(sl.anchored, &out->anchored, &out->n_anchored) || !give(dispatch, &out->dispatch, &out->n_dispatch)) {
        ribbit_seed_lists_free(out);
        return fail(RIBBIT_E_NOMEM, "out of host memory");
    }
    out->guard_hits = sl.guard_hits;
    return RIBBIT_OK;
}

int advance_to_anchored(RibbitHandle *h) {
    if (h->rec.stage_done >= STAGE_ANCHORED) return RIBBIT_OK;
    int rc = advance_to_perfect(h);
    if (rc) return rc;
    if ((rc = ensure_host_planes(h))) return rc;
    DeviceCalls dcs, dca;
    const bool subst_todo = h->rec.stage_done < STAGE_SUBST;
    const bool subst_full = h->rec.subst_calls_valid;
    // the full call lists only when they have been asked for (ribbit_hip_*_calls); otherwise the compact form:
    // nine anchored calls in ten fail the length filter and never leave the device
    if (subst_todo && !subst_full && (rc = window_stage_device(h, RIBBIT_STAGE_SUBST, false, rb::subst_seedlen_cutoff, &dcs))) return rc;
    const bool full = h->rec.anchored_calls_valid;
    if (!full) {
        if ((rc = prepare_anchored(h))) return rc;
        if ((rc = window_stage_device(h, RIBBIT_STAGE_ANCHORED, false, rb::anchored_seedlen_cutoff, &dca))) return rc;
        h->rec.xa_on_device = true;
    }
    if ((rc = bind_device(h))) return rc;
    const double tx0 = now_ms();
    if ((rc = xa_copy_begin(h))) return rc;
    const double tx1 = now_ms();
    if (subst_todo) subst_merge(h, subst_full ? nullptr : &dcs);
    const double merge_s = h->merge_ms;
    const double tx2 = now_ms();
    if ((rc = xa_wait_host(h))) return rc;
    const bool profile_xa = rb::profile_on();
    if (profile_xa)
        std::fprintf(stderr, "[composed planes] %.2f GB to the host for the merges' range reads: page-locked room and enqueue %.1f ms, waited %.1f ms for the copy after the substitution merge\n",
                     (double)(h->params.max_motif - h->params.min_motif + 1) * (double)h->xa_stride * 4e-9, tx1 - tx0, now_ms() - tx2);
    use_composed_planes(h->lists, &h->host);
    // (lists.anchored is not cleared here: every path of the stage sets it, and the join reuses what it holds, parallel_merge.cpp)
    const double t0 = now_ms();
    const unsigned threads = rb::host_thread_count(h->host_threads);
    rb::MergeStats st;
    if (full) rb::merge_anchored_stage_full(h->lists, h->anchored_calls.data(), h->anchored_calls.size(), threads, &st);
    else {
        // the first parallel pass as device work for stages of a million calls and more (api_merge.cpp): the kept calls are still
        // where window_stage_device put them (d_dense as 16-byte call records, d_pend)
        const rb::AnchoredDevicePass on_device = anchored_device_pass(h, reinterpret_cast<RibbitCall *>(h->d_dense.p), dca.pend ? h->d_pend.p : nullptr);
        rb::merge_anchored_stage(h->lists, dca, threads, &st, &on_device);
    }
    const double t1 = now_ms();
    const unsigned dispatch_ranges = rb::dispatch_order_ranges(h->lists, st.cut_pos, threads, h->dispatch);
    h->merge_ms = now_ms() - t0;
    const bool profile = rb::profile_on();
    if (profile) print_anchored_merge_profile(h->lists.anchored.size(), st, now_ms() - t1, dispatch_ranges);
    h->subst_merge_ms = subst_todo ? merge_s : 0.0;
    h->rec.stage_done = STAGE_ANCHORED;
    return RIBBIT_OK;
}

}  // namespace rbapi

extern "C" {

int ribbit_hip_subst_calls(RibbitHandle *h, const RibbitCall **out, size_t *n) { return guarded("the substitution stage", [&]() -> int {
    if (!h || !out || !n) return fail(RIBBIT_E_ARG, "null argument");
    int rc = build_subst_calls(h);
    if (rc) return rc;
    *out = h->subst_calls.data();
    *n = h->subst_calls.size();
    return RIBBIT_OK;
}); }

int ribbit_hip_seeds_substitutions(RibbitHandle *h, const RibbitSeed **perfect, size_t *n_perfect,
                                   const RibbitSeed **subst, size_t *n_subst) { return guarded("the substitution stage", [&]() -> int {
    if (!h || !perfect || !n_perfect || !subst || !n_subst) return fail(RIBBIT_E_ARG, "null argument");
    if (!h->loaded) return fail(RIBBIT_E_STATE, "no record loaded");
    if (h->rec.stage_done > STAGE_SUBST) return fail(RIBBIT_E_STATE, "a later stage already re-typed the lists; reload the record");
    int rc = advance_to_subst(h);
    if (rc) return rc;
    *perfect = h->lists.perfect.data();
    *n_perfect = h->lists.perfect.size();
    *subst = h->lists.subst.data();
    *n_subst = h->lists.subst.size();
    return RIBBIT_OK;
}); }

int ribbit_hip_anchored_calls(RibbitHandle *h, const RibbitCall **out, size_t *n) { return guarded("the anchored stage", [&]() -> int {
    if (!h || !out || !n) return fail(RIBBIT_E_ARG, "null argument");
    int rc = build_anchored_calls(h);
    if (rc) return rc;
    *out = h->anchored_calls.data();
    *n = h->anchored_calls.size();
    return RIBBIT_OK;
}); }

int ribbit_hip_debug_window_calls(RibbitHandle *h, int stage, const RibbitDebugWindowStage *in, RibbitChunkCalls *out, uint32_t *n_edge) {
    return guarded("the window stage on caller-made streaks", [&]() -> int {
    if (!h || !in || !out || !n_edge) return fail(RIBBIT_E_ARG, "null argument");
    if (!h->loaded) return fail(RIBBIT_E_STATE, "no record loaded");
    if (h->pair_pending) return fail(RIBBIT_E_STATE, "a perfect scan is in flight on this handle: call ribbit_hip_scan_perfect_end first");
    if (stage != RIBBIT_STAGE_SUBST && stage != RIBBIT_STAGE_ANCHORED) return fail(RIBBIT_E_ARG, "stage must be RIBBIT_STAGE_SUBST or RIBBIT_STAGE_ANCHORED");
    const bool full = in->full != 0;
    if ((in->n_streaks && !in->streaks) || (!full && !in->min_span) || (in->n_dropped && !in->dropped_ends)) return fail(RIBBIT_E_ARG, "null argument");
    const size_t n = in->n_streaks, most = (size_t)1 << 24;
    if (n > most || in->n_dropped > most || in->first_edge_cap > most) return fail(RIBBIT_E_ARG, "bad size");
    const int64_t L = h->length;
    if (in->own_lo < 0 || in->own_hi < in->own_lo || in->z_lo < 0 || in->z_lo > INT32_MAX || in->pos_offset < 0 || in->pos_offset + L > INT32_MAX)
        return fail(RIBBIT_E_ARG, "bad chunk geometry: own [%lld, %lld), first exact position %lld, piece of %lld bases at %lld", (long long)in->own_lo,
                    (long long)in->own_hi, (long long)in->z_lo, (long long)L, (long long)in->pos_offset);
    // everything a kernel indexes with: positions, motifs, the terminator; the order the group scan and the joins rely on
    for (size_t i = 0; i < n; ++i) {
        const RibbitRun &r = in->streaks[i];
        if (r.start < 0 || r.start >= r.end || r.end > L) return fail(RIBBIT_E_ARG, "streak %zu: [%d, %d) is no stretch of a record of %lld bases", i, r.start, r.end, (long long)L);
        if (r.mlen < h->params.min_motif || r.mlen > h->params.max_motif) return fail(RIBBIT_E_ARG, "streak %zu: motif %d outside %d..%d", i, r.mlen, h->params.min_motif, h->params.max_motif);
        if (r.term < RIBBIT_TERM_ZERO || r.term > RIBBIT_TERM_EOS) return fail(RIBBIT_E_ARG, "streak %zu: term %d", i, r.term);
        if (i == 0) continue;
        const RibbitRun &p = in->streaks[i - 1];
        if (r.mlen < p.mlen || (r.mlen == p.mlen && r.start <= p.start)) return fail(RIBBIT_E_ARG, "streak %zu: not in (mlen, start) order", i);
        if (r.mlen == p.mlen && r.start < p.end) return fail(RIBBIT_E_ARG, "streak %zu: overlaps the streak before it", i);
    }
    for (size_t i = 0; i < in->n_dropped; ++i) {
        const int32_t e = in->dropped_ends[i];
        if (e < 0 || e >= L) return fail(RIBBIT_E_ARG, "dropped end %zu: %d outside the record", i, e);
        if (i > 0 && e <= in->dropped_ends[i - 1]) return fail(RIBBIT_E_ARG, "dropped end %zu: not ascending", i);
    }
    int rc;
    if ((rc = bind_device(h))) return rc;
    if (h->copy_pending && (rc = perfect_wait(h))) return rc;          // d_dense / d_events are shared with the perfect stage
    // the buffers the stage inherits from the event pass, sized as that pass sizes them for 2 n events
    size_t cap = std::max<size_t>(2 * n, rb::EV_SHARDS);
    if ((rc = event_room(h, &cap, nullptr))) return rc;
    if (n) HIP_TRY(hipMemcpyAsync(h->d_dense.p, in->streaks, n * sizeof(RibbitRun), hipMemcpyHostToDevice, h->stream));
    const bool dropmap = !full && in->n_dropped > 0;
    std::vector<uint32_t> words;
    if (dropmap) {
        words.assign(dropmap_words(L), 0u);
        for (size_t i = 0; i < in->n_dropped; ++i) words[(size_t)in->dropped_ends[i] >> 5] |= 1u << (in->dropped_ends[i] & 31);
        if ((rc = h->d_dropmap.ensure(words.size()))) return rc;
        HIP_TRY(hipMemcpyAsync(h->d_dropmap.p, words.data(), words.size() * sizeof(uint32_t), hipMemcpyHostToDevice, h->stream));
    }
    HIP_TRY(hipStreamSynchronize(h->stream));      // (the sources are the caller's and a local)
    h->dropmap_valid = false;                      // what a scan left in d_dropmap is gone
    ChunkWindow cw;
    cw.own_lo = (uint32_t)std::min<int64_t>(in->own_lo, 0xffffffffll);
    cw.own_hi = (uint32_t)std::min<int64_t>(in->own_hi, 0xffffffffll);
    cw.z_lo = (uint32_t)in->z_lo;
    cw.keep_flush = in->keep_flush != 0;
    cw.pos_offset = (int32_t)in->pos_offset;
    std::memset(out, 0, sizeof *out);
    out->tail_pend = -1;
    *n_edge = 0;
    DeviceCalls dc;
    rc = window_calls_device(h, stage, (uint32_t)n, full, in->min_span, &cw, dropmap, in->first_edge_cap, 0.0, &dc);
    h->timers.have[RIBBIT_TIME_GPU] = false;       // no scan began that interval
    if (rc) return rc;
    out->calls = dc.calls; out->n = dc.n;
    out->pend = dc.pend;
    out->tail_pend = dc.tail_pend;
    out->flush = dc.flush; out->n_flush = dc.n_flush;
    out->inexact = cw.inexact ? 1 : 0;
    out->dev_calls = h->d_dense.p;
    out->dev_pend = dc.pend ? h->d_pend.p : nullptr;
    out->streaks = (int64_t)n;
    *n_edge = (uint32_t)h->last_edge_calls;
    return RIBBIT_OK;
}); }

int ribbit_hip_seeds_anchored(RibbitHandle *h, const RibbitSeed **perfect, size_t *n_perfect,
                              const RibbitSeed **subst, size_t *n_subst,
                              const RibbitSeed **anchored, size_t *n_anchored) { return guarded("the anchored stage", [&]() -> int {
    if (!h || !perfect || !n_perfect || !subst || !n_subst || !anchored || !n_anchored) return fail(RIBBIT_E_ARG, "null argument");
    if (!h->loaded) return fail(RIBBIT_E_STATE, "no record loaded");
    int rc = advance_to_anchored(h);
    if (rc) return rc;
    *perfect = h->lists.perfect.data();   *n_perfect = h->lists.perfect.size();
    *subst = h->lists.subst.data();       *n_subst = h->lists.subst.size();
    *anchored = h->lists.anchored.data(); *n_anchored = h->lists.anchored.size();
    return RIBBIT_OK;
}); }

int ribbit_hip_dispatch_seeds(RibbitHandle *h, const RibbitSeed **out, size_t *n) { return guarded("the anchored stage", [&]() -> int {
    if (!h || !out || !n) return fail(RIBBIT_E_ARG, "null argument");
    if (!h->loaded) return fail(RIBBIT_E_STATE, "no record loaded");
    int rc = advance_to_anchored(h);
    if (rc) return rc;
    *out = h->dispatch.data();
    *n = h->dispatch.size();
    return RIBBIT_OK;
}); }

void ribbit_debug_set_merge_min_range(size_t calls) { rb::set_merge_min_range(calls); }

int32_t ribbit_debug_last_dispatch_ranges(void) { return (int32_t)rb::last_dispatch_ranges(); }

void ribbit_debug_last_merge(int stage, int32_t out[5]) {
    const rb::MergeStats st = rb::last_merge_stats(stage);
    out[0] = (int32_t)st.ranges; out[1] = (int32_t)std::min(st.ranges_redone, 0xffffu) | (int32_t)(std::min(st.stale_by_sight, 0x7fffu) << 16); out[2] = (st.redone_in_order ? 1 : 0) | (int32_t)(st.ranges_run << 1);
    out[3] = (int32_t)std::min<long long>(st.head_writes, INT32_MAX); out[4] = (st.first_range_empty ? 1 : 0) | (int32_t)(st.passes << 8);
}

void ribbit_debug_last_device_merge(int32_t out[5]) {
    const rb::MergeStats st = rb::last_merge_stats(1);
    out[0] = (int32_t)st.device_ranges; out[1] = (int32_t)st.device_bailed; out[2] = (int32_t)st.device_host_share; out[3] = (int32_t)st.ranges; out[4] = (int32_t)st.ranges_redone;
}

int ribbit_host_replay_calls(const RibbitScanParams *params, int64_t length,
                             const uint32_t *hi, const uint32_t *lo, const uint32_t *brk, size_t nwords,
                             const uint32_t *xa, size_t xa_stride,
                             const RibbitCall *perfect_calls, size_t n_perfect_calls,
                             const RibbitCall *subst_calls, size_t n_subst_calls,
                             const RibbitCall *anchored_calls, size_t n_anchored_calls,
                             RibbitSeedLists *out) { return guarded("the replay of the calls", [&]() -> int {
    if (!params || !out || (length > 0 && (!hi || !lo || !brk))) return fail(RIBBIT_E_ARG, "null argument");
    if ((n_perfect_calls && !perfect_calls) || (n_subst_calls && !subst_calls) || (n_anchored_calls && !anchored_calls))
        return fail(RIBBIT_E_ARG, "null call list");
    if (const int bad = check_caller_planes(params, length, hi, lo, brk, nwords, xa, xa_stride)) return bad;
    std::memset(out, 0, sizeof *out);
    rb::HostPlanes hp;
    rb::SeedLists sl;
    lists_over_caller_planes(params, length, hi, lo, brk, nwords, hp, sl);
    for (size_t i = 0; i < n_perfect_calls; ++i) rb::perfect_add(sl, perfect_calls[i].start, perfect_calls[i].end, perfect_calls[i].mlen);
    rb::merge_subst_stage_full(sl, subst_calls, n_subst_calls, rb::host_thread_count(0));
    // the anchored stage runs when there are anchored calls or composed planes are given; anchored_calls non-null with
    // n == 0 also asks for it (a record whose anchored scan made no call still gets its dispatch list)
    const bool anchored_stage = n_anchored_calls || xa || anchored_calls;
    if (anchored_stage) {
        const size_t nm = (size_t)(params->max_motif - params->min_motif + 1);
        if (xa) hp.xa.assign(xa, xa + nm * xa_stride);        // else: recomputed slice by slice from the packed planes
        hp.xa_stride = xa ? (int64_t)xa_stride : 0;
        hp.xa_m_lo = params->min_motif;
        hp.xa_m_hi = params->max_motif;
        use_composed_planes(sl, &hp);
    }
    rb::SeedVec dispatch;
    if (anchored_stage) {
        rb::MergeStats st;
        // test hook RIBBIT_MERGE_DEVICE_RANGES=<calls per range>: the stage cut as for the GPU's pass of the anchored merge (hundreds of
        // thousands of ranges, prepared on the host threads) with a device that cannot run -- the host threads then merge those ranges
        rb::AnchoredDevicePass no_device;
        const char *fine = std::getenv("RIBBIT_MERGE_DEVICE_RANGES");
        if (fine) {
            no_device.min_calls = 0; no_device.calls_per_range = (size_t)std::max(1, std::atoi(fine));
            // (the "device" takes the lighter half of the ranges and merges none of them)
            no_device.run = [](const rb::SeedLists &, const rb::KeptCalls &, const std::vector<size_t> &, const std::vector<int> &, const std::vector<rb::Cursor2> &, const std::vector<uint32_t> &order, size_t,
                               const std::function<void(uint32_t *, const uint32_t *)> &meanwhile, std::vector<rb::AnchoredDevicePass::RangeResult> &, std::vector<rb::AnchoredDevicePass::LogEntry> &,
                               std::vector<rb::AnchoredDevicePass::LogEntry> &, std::vector<rb::AnchoredDevicePass::HeadEntry> &) {
                uint32_t from_back = (uint32_t)order.size(), from_front = (uint32_t)order.size() / 2;
                meanwhile(&from_back, &from_front);
                return false;
            };
        }
        rb::merge_anchored_stage_full(sl, anchored_calls, n_anchored_calls, rb::host_thread_count(0), &st, fine ? &no_device : nullptr);
        const double td = now_ms();
        const unsigned dispatch_ranges = rb::dispatch_order_ranges(sl, st.cut_pos, rb::host_thread_count(0), dispatch);
        if (rb::profile_on()) print_anchored_merge_profile(sl.anchored.size(), st, now_ms() - td, dispatch_ranges);
    }
    return give_seed_lists(sl, dispatch, out);
}); }

void ribbit_seed_lists_free(RibbitSeedLists *lists) {
    if (!lists) return;
    std::free(lists->perfect); std::free(lists->subst); std::free(lists->anchored); std::free(lists->dispatch);
    std::memset(lists, 0, sizeof *lists);
}

}  // extern "C"
