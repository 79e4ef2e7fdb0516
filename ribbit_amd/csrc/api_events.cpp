// api_events.cpp -- the event pass: what every scan does around its kernel; see api_internal.h for the map of the files behind include/ribbit_hip.h.
// A scan kernel leaves START / END events in EV_SHARDS regions of the event buffer.  Its caller: pair_prepare, first_event_cap, then
// event_room, the kernel with scan_launch_args, enqueue_pairing, read_published and, if a region overflowed, grow_event_cap and round
// again; at last pairing_verdict.  The stages own their streams, their HIP events and their kernels' extras.
#include "api_internal.h"

namespace rbapi {

// pr for a scan of `length` bases with the handle's motifs (own_lo / own_hi / pos_offset: see rb::PairLaunch; a whole record is
// 0, INT64_MAX, 0), pb sized for it, and its page-locked words mapped the first time
int pair_prepare(RibbitHandle *h, PairBufs &pb, int64_t length, int64_t own_lo, int64_t own_hi, int64_t pos_offset, rb::PairLaunch &pr) {
    int rc;
    pr.m_lo = (uint32_t)h->params.min_motif;
    pr.nm = (uint32_t)(h->params.max_motif - h->params.min_motif + 1);
    pr.tile_bases = (uint32_t)rb::TILE_BASES;
    pr.ntile = (uint32_t)(length / rb::TILE_BASES + 1);
    pr.own_lo = own_lo; pr.own_hi = own_hi; pr.pos_offset = pos_offset;
    const size_t entries = (size_t)pr.nm * pr.ntile;
    if (entries > 0xfffffff0u) return fail(RIBBIT_E_ARG, "record too long for %u motif sizes", pr.nm);
    if ((rc = pb.d_counters.ensure(rb::EV_COUNTER_WORDS)) || (rc = pb.d_pair_status.ensure(rb::PAIR_STATUS_WORDS)) ||
        (rc = pb.d_pair_table.ensure(entries)) || (rc = pb.d_run_base.ensure(entries)) || (rc = pb.d_pair_partial.ensure(entries / 1024 + 2)) ||
        (rc = pb.d_halves.ensure(2 * (size_t)pr.nm)))
        return rc;
    if (!pb.h_pub.p) {
        if ((rc = pb.h_pub.ensure(rb::EV_SHARDS + rb::PAIR_STATUS_WORDS))) return rc;
        HIP_TRY(hipHostGetDevicePointer((void **)&pb.h_pub_dev, pb.h_pub.p, 0));
    }
    return RIBBIT_OK;
}

// capacity in events, split evenly over EV_SHARDS regions; per_base_x4: four times the events the stage expects per base.  A too
// small first guess costs a second launch and a second round of allocations.
size_t first_event_cap(const RibbitHandle *h, size_t per_base_x4) {
    if (h->debug_first_cap) return h->debug_first_cap;
    return std::max(std::max<size_t>((size_t)1 << 20, (size_t)h->length * per_base_x4 / 4), h->d_events.cap);
}

static size_t round_event_cap(size_t cap) { return std::min<size_t>((cap + rb::EV_SHARDS - 1) / rb::EV_SHARDS * rb::EV_SHARDS, 0xffffff00u); }

// some region overflowed (its counter says `worst`): size every region for the fullest one, twice at the most
int grow_event_cap(int attempt, uint32_t worst, size_t *cap) {
    const size_t need = (size_t)worst * rb::EV_SHARDS;
    if (attempt == 2 || round_event_cap(need) < need) return fail(RIBBIT_E_OVERFLOW, "event buffer overflow: fullest region needs %u events", worst);
    *cap = ((size_t)worst + 1024) * rb::EV_SHARDS;
    return RIBBIT_OK;
}

// room for *cap events (rounded) and for what the pairing makes of them: cap / 2 records of 16 bytes
int event_room(RibbitHandle *h, size_t *cap, rb::PairLaunch *pr) {
    int rc;
    *cap = round_event_cap(*cap);
    if ((rc = h->d_events.ensure(*cap)) || (rc = h->d_dense.ensure(*cap))) return rc;
    if (pr) pr->region_cap = (uint32_t)(*cap / rb::EV_SHARDS);
    return RIBBIT_OK;
}

int zero_counters(RibbitHandle *h, bool even_if_clean) {
    if (even_if_clean || !h->counters_clean) HIP_TRY(hipMemsetAsync(h->pb.d_counters.p, 0, rb::EV_COUNTER_WORDS * sizeof(uint32_t), h->stream));
    h->counters_clean = false;
    return RIBBIT_OK;
}

rb::PerfectLaunch scan_launch_args(const RibbitHandle *h, size_t cap, int kernel) {
    rb::PerfectLaunch pp;
    pp.m_lo = h->params.min_motif;
    pp.m_hi = h->params.max_motif;
    pp.ev_cap = (uint32_t)cap;
    pp.motifs_per_block = h->debug_split[kernel];
    return pp;
}

int enqueue_pairing(PairBufs &pb, const rb::PairLaunch &pr, const uint64_t *d_events, uint64_t *d_dense, size_t cap, hipStream_t stream) {
    HIP_TRY(rb::launch_pair_runs(d_events, pb.d_counters.p, pr, pb.d_pair_table.p, pb.d_run_base.p, pb.d_pair_partial.p,
                                 d_dense, (uint32_t)(cap / 2), pb.d_halves.p, (uint32_t)(2 * (size_t)pr.nm), pb.d_pair_status.p, stream));
    rb::launch_pair_publish(pb.d_counters.p, pb.d_pair_status.p, pb.h_pub_dev, stream);
    HIP_TRY(hipGetLastError());
    return RIBBIT_OK;
}

Published read_published(const PairBufs &pb) {
    Published pub;
    for (int t = 0; t < rb::EV_SHARDS; ++t) { pub.worst = std::max(pub.worst, pb.h_pub.p[t]); pub.produced += pb.h_pub.p[t]; }
    return pub;
}

// noun: what the pairing makes ("run", "streak")
int pairing_verdict(const PairBufs &pb, uint64_t produced, const char *noun, size_t *n, size_t *n_halves) {
    const uint32_t *status = pb.h_pub.p + rb::EV_SHARDS, flags = status[rb::PAIR_FLAGS];
    if (flags) {
        const std::string s = noun;
        return fail(RIBBIT_E_INTERNAL, "%s pairing failed (flags 0x%x):%s%s%s%s%s", noun, flags,
                    flags & rb::PAIR_BAD_EVENT ? " malformed event;" : "", flags & rb::PAIR_DUP_CHUNK ? " duplicate event chunk;" : "",
                    flags & rb::PAIR_NOT_ALTERNATING ? (" " + s + " starts and ends do not alternate;").c_str() : "",
                    flags & rb::PAIR_UNTERMINATED ? (" unterminated " + s + ";").c_str() : "", flags & rb::PAIR_NO_ROOM ? (" " + s + " buffer too small;").c_str() : "");
    }
    *n = status[rb::PAIR_TOTAL];
    if ((uint64_t)*n * 2 != produced) return fail(RIBBIT_E_INTERNAL, "%llu events but %zu %ss", (unsigned long long)produced, *n, noun);
    *n_halves = status[rb::PAIR_HALVES];
    return RIBBIT_OK;
}

// The legacy form of the perfect scan, whose events travel (ribbit_hip_perfect_runs_partial pairs them on the host): launch the
// kernel, compact its sharded event regions, copy the events back and index the (motif, tile) chunks.
int collect_perfect_events(RibbitHandle *h) {
    int rc;
    if ((rc = bind_device(h))) return rc;
    if ((rc = h->pb.d_counters.ensure(rb::EV_COUNTER_WORDS))) return rc;
    if ((rc = h->h_counters.ensure(rb::EV_COUNTER_WORDS))) return rc;
    size_t cap = first_event_cap(h, 1);      // typical event density of the perfect scan on repeat-rich sequence: 0.07 per base
    uint32_t produced = 0;
    for (int attempt = 0;; ++attempt) {
        if ((rc = event_room(h, &cap, nullptr))) return rc;
        HIP_TRY(hipEventRecord(h->timers.begin[RIBBIT_TIME_GPU], h->stream));
        if ((rc = zero_counters(h, true))) return rc;
        const rb::PerfectLaunch pp = scan_launch_args(h, cap, RIBBIT_SCAN_PERFECT);
        HIP_TRY(hipEventRecord(h->timers.begin[RIBBIT_TIME_SCAN], h->stream));
        h->rec.last_split[RIBBIT_SCAN_PERFECT] = rb::launch_scan_perfect(h->planes(), pp, h->d_events.p, h->pb.d_counters.p, h->stream);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(h->timers.end[RIBBIT_TIME_SCAN], h->stream));
        rb::launch_compact_events(h->d_events.p, pp.ev_cap, h->pb.d_counters.p, h->d_dense.p, h->stream);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(h->h_counters.p, h->pb.d_counters.p, rb::EV_COUNTER_WORDS * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));
        produced = h->h_counters.p[rb::EV_SUMMARY];
        if (!h->h_counters.p[rb::EV_SUMMARY + 1]) break;
        uint32_t worst = 0;
        for (int t = 0; t < rb::EV_SHARDS; ++t) worst = std::max(worst, h->h_counters.p[t * rb::EV_COUNTER_STRIDE]);
        if ((rc = grow_event_cap(attempt, worst, &cap))) return rc;
    }
    h->last_event_count = produced;
    if ((rc = h->h_events.ensure(std::max<size_t>(produced, 1)))) return rc;
    // Events arrive as position-ordered chunks, exactly one per (motif, tile) that has any event.  A kernel indexes
    // them in a direct-address table keyed (motif, tile) -- every event looks at its neighbours -- so the host
    // neither sorts nor walks the events to find the chunks.
    const uint32_t m_lo = (uint32_t)h->params.min_motif;
    const size_t nm = (size_t)(h->params.max_motif - h->params.min_motif + 1);
    const size_t ntile = (size_t)(h->length / rb::TILE_BASES + 1);
    if (nm * ntile > 0xfffffff0u) return fail(RIBBIT_E_ARG, "record too long for %zu motif sizes", nm);
    if ((rc = h->pb.d_pair_table.ensure(nm * ntile))) return rc;
    if ((rc = h->pb.d_pair_status.ensure(rb::PAIR_STATUS_WORDS))) return rc;
    HIP_TRY(rb::launch_chunk_table(h->d_dense.p, h->pb.d_counters.p, m_lo, (uint32_t)nm, (uint32_t)ntile, (uint32_t)rb::TILE_BASES, h->pb.d_pair_table.p, h->pb.d_pair_status.p, h->stream));
    h->chunk_table.resize(nm * ntile);
    h->table_ntile = ntile;
    uint32_t table_status = 0;
    HIP_TRY(hipMemcpyAsync(h->chunk_table.data(), h->pb.d_pair_table.p, nm * ntile * sizeof(uint64_t), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipMemcpyAsync(&table_status, h->pb.d_pair_status.p, sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
    if (produced) {
        HIP_TRY(hipMemcpyAsync(h->h_events.p, h->d_dense.p, (size_t)produced * sizeof(uint64_t), hipMemcpyDeviceToHost, h->stream));
    }
    HIP_TRY(hipEventRecord(h->timers.end[RIBBIT_TIME_GPU], h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    h->timers.have[RIBBIT_TIME_SCAN] = h->timers.have[RIBBIT_TIME_GPU] = true;
    if (table_status & 1u) return fail(RIBBIT_E_INTERNAL, "malformed event (motif or tile outside the launch)");
    if (table_status & 2u) return fail(RIBBIT_E_INTERNAL, "duplicate event chunk");
    // {first + 1, end}  ->  {offset, count}
    struct Chunk { uint32_t off, n; };
    static_assert(sizeof(Chunk) == sizeof(uint64_t), "chunk table entry is one 64-bit word");
    Chunk *table = reinterpret_cast<Chunk *>(h->chunk_table.data());
    for (size_t k = 0; k < nm * ntile; ++k) {
        const uint32_t first1 = table[k].off, end = table[k].n;
        table[k] = first1 ? Chunk{first1 - 1u, end - (first1 - 1u)} : Chunk{0, 0};
    }
    return RIBBIT_OK;
}

}  // namespace rbapi
