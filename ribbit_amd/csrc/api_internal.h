// api_internal.h -- shared by the api_*.cpp files behind the extern "C" boundary of libribbit_hip.so (include/ribbit_hip.h):
// the handle, its device / page-locked buffers, error reporting, and the internal steps that more than one of those files
// takes.  Until round 4 all of this was one 3,200-line api.cpp; it is now
//   api_core.cpp        handles, streams, loading a record (pack), timers, plane queries
//   api_events.cpp      the event pass every scan takes: region sizes, pairing on the device, what it publishes, growth on overflow
//   api_perfect.cpp     the perfect stage: scan, device-side pairing, runs, calls, seeds; its chunk form
//   api_window.cpp      the substitution and anchored stages: scans, streak pairing, window state machines, merges, dispatch order
//   api_chunks.cpp      one chunk of a longer record (window stages) and the merging rank's half
//   api_merge.cpp       the anchored stage's merge on the device: what parallel_merge.h's AnchoredDevicePass does on a handle
//   api_align.cpp       the scans of the dispatched seeds, alignment jobs, batched striped passes and path searches
//   api_refine_bed.cpp  refinement to BED text: the GPU alignment pipeline, the recursion's levels, the host-only form
//   api_mask.cpp        the repeat-masked FASTA body of a record (mask.hip), its host twin, BED rows back to intervals
//   api_repeats.cpp     every row's bases with their flanks as FASTA entries (repeats.hip), in batches of a text budget; its host twin
//   api_loci.cpp        merged, sorted loci and the per-window density of a record (loci.hip), their host twins, the loci as text
//   api_overlap.cpp     the rows of a record against a second set of intervals (overlap.hip), its host twin, the rows' text with the two columns
//   api_best.cpp        the best non-overlapping rows of a record (best.hip), its host twin, the chosen rows' text
//   api_classes.cpp     the rows of a record grouped by canonical motif class (classes.hip), its host twin, the motifs of a BED text, both texts
//   api_compound.cpp    the rows of a record chained into compound loci (compound.hip), its host twin, the classes as labels, the chains' text
//   api_interruptions.cpp  every row's CIGAR decoded into interruptions and the pure stretch (interruptions.hip), its host twin, the CIGARs of a BED text, both texts
//   api_nearest.cpp     the nearest interval of a second set for every row, and the other way round (nearest.hip), its host twin, both texts
//   api_composition.cpp the base counts of every row, its flanks and every window from the bit planes (composition.hip), their host twins, both texts
//   api_primers.cpp     a forward and a reverse primer in the flanks of every target, from the bit planes and the rows' coverage (primers.hip), its host twin, the text
//   api_primer_pairs.cpp  the two primers of every target chosen as a pair and checked for dimers and hairpins (primer_pairs.hip), its host twin, the oligo checks, the text
//   api_primer_products.cpp  the sites of oligos on either strand of the record and the products of primer pairs among them (primer_products.hip), their host twins, the text;
//                            the site search of every in-silico PCR (search_sites) and the rule of its callers' batches (site_batch)
//   api_primer_specific.cpp  the best primer pair of every target that amplifies nothing else in the record (primer_specific.hip, through search_sites), its host twin, the text
//   api_primer_genome.cpp    a target's two shortlists as they leave their record, their pairs judged on any loaded record (primer_specific.hip, through search_sites), the host twins, the sum over records, the choice
//   api_amplicons.cpp        every chosen pair typed on any loaded record: its first product and the repeat tract inside it (amplicons.hip, through search_sites), its host twin, the sum over records, the text
//   api_panel.cpp            primer pairs pooled into multiplex panels: the conflict matrix, the order and the first fit (panel.hip), which read no record; its host twin, the text
//   api_alleles.cpp          the chosen pairs typed on many assemblies: a sample's cells, every marker's alleles, He and PIC over the sample-major matrix (alleles.hip), which reads no record; its host twin, both texts
// The last eighteen are the row outputs: their buffers are the handle's RowBufs `rows`, where all device work of a call is carved from
// one buffer by the layout its .hip file states (kernels.h); best, classes, compound, interruptions, nearest, primers and primer pairs stage their inputs through stage_down, what their host
// sides share is below (hand_out, clipped_sorted_rows), what their kernels share is row_kernels.h, and the BED text they read and
// write (the row format, the reader in pieces, the writer in pieces) is
//   bed_text.h          a row's named fields, bed_read / bed_gather, BedLines, write_pieces / join_text, put_number
//   primers_host.h      what the primer outputs' host sides share: the parameter checks, a target's windows, one candidate from the bytes, a primer's and a pair's columns,
//                       the writer of the pairs' texts, the twins' index of distinct oligos
// Host threads: every team of them, here and in refine.cpp, parallel_merge.cpp and host_planes.cpp, is started by rb::on_threads /
// rb::over_pieces of host_threads.h (part 0 on the caller, a thread that cannot start leaves its part to the caller, all joined, the
// first exception of any part rethrown on the caller: it then meets guarded() below); the thread count rule (the handle's, else
// RIBBIT_THREADS, else min(cores, 16)) is rb::host_thread_count, the RIBBIT_PROFILE switch rb::profile_on, and the threads that
// outlive one loop (feeders, tabler, side, ...) are joined by an rb::JoinOnExit.
// Not part of the ABI; nothing outside ribbit_amd/csrc includes it.
#pragma once
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <condition_variable>
#include <cstring>
#include <deque>
#include <exception>
#include <memory>
#include <mutex>
#include <new>
#include <string>
#include <thread>
#include <vector>

#include "device_planes.h"
#include "event_stream.h"
#include "host_planes.h"
#include "host_threads.h"
#include "kernels.h"
#include "parallel_merge.h"
#include "refine.h"
#include "ssw_exact.h"
#include "ribbit_hip.h"
#include "seed_lists.h"


namespace rbapi {

extern thread_local std::string g_last_error;
int fail(int code, const char *fmt, ...);
// No entry point lets a C++ exception out (the callers are C, ctypes and the command-line tool: an exception that leaves
// extern "C" ends the process).  Every extern "C" function of the api_*.cpp files that returns a status is
//     int ribbit_x(...) { return guarded("x", [&]() -> int {
//         ... the body, indented as a function's ...
//     }); }
// `what` names the operation in the message.  Not guarded, because all they do is check arguments and read or write plain
// fields of the handle or of globals: ribbit_hip_abi_version, ribbit_hip_device_count (a count, not a status), ribbit_hip_set_stream,
// ribbit_hip_set_timing, ribbit_hip_set_host_threads, ribbit_hip_debug_set_event_capacity, ribbit_hip_debug_set_scan_split,
// ribbit_hip_debug_last_scan_split, ribbit_hip_debug_set_repeat_text_budget, ribbit_hip_debug_set_small_record_capacity, ribbit_hip_refine_met_empty_query,
// ribbit_hip_guard_hits, ribbit_host_debug_thread_faults, ribbit_hip_last_event_count, ribbit_hip_plane_words, ribbit_hip_last_error, ribbit_hip_host_free and the
// other *_free functions, ribbit_*_params_default, the ribbit_debug_* counter readers and setters; and ribbit_hip_close, which is
// `delete` (a destructor does not throw).  A team of threads hands an exception of any part to its caller (host_threads.h); the
// threads that outlive one loop keep theirs inside themselves where they are made.
template <typename F>
int guarded(const char *what, F &&body) {
    try { return body(); }
    catch (const std::bad_alloc &) { return fail(RIBBIT_E_NOMEM, "out of host memory in %s", what); }
    catch (const std::exception &e) { return fail(RIBBIT_E_INTERNAL, "%s: %s", what, e.what()); }
    catch (...) { return RIBBIT_E_INTERNAL; }
}
#define HIP_TRY(expr)                                                                              \
    do {                                                                                           \
        hipError_t e_ = (expr);                                                                    \
        if (e_ != hipSuccess)                                                                      \
            return fail(RIBBIT_E_DEVICE, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

// A device buffer that is being replaced by a larger one is released at the next record load or handle close, not on the spot:
// hipFree synchronises with every stream of the device (api_core.cpp).
void device_free_later(void *p);
void pinned_free_later(void *p);
void device_free_pending();      // (both kinds)

template <typename T>
struct DevBuf {
    T *p = nullptr;
    size_t cap = 0;   // elements
    // grows: a buffer that is sized again and again within one call (the alignment batches', slice by slice) asks for half as much
    // again as it has, at least, and a quarter of headroom: it is then released and allocated a few times per record instead of at
    // every slice that is a little larger than the one before.  Everything else is sized exactly: callers derive region sizes
    // from `cap` (a quarter more event capacity is a third off the perfect scan's throughput).
    int ensure(size_t n, bool grows = false) {
        if (n <= cap) return RIBBIT_OK;
        if (grows) n = std::max(n + std::min(n / 4, ((size_t)256 << 20) / sizeof(T)), cap + std::min(cap / 2, ((size_t)1 << 30) / sizeof(T)));
        if (p) { device_free_later(p); p = nullptr; cap = 0; }      // (hipFree waits for the whole device: not while another feeder's kernels run)
        // RIBBIT_PROFILE_MEMORY=<MB>: one line per device allocation of at least that size (which buffers are large, and when)
        static const size_t trace_from = std::getenv("RIBBIT_PROFILE_MEMORY") ? (size_t)std::max(1, std::atoi(std::getenv("RIBBIT_PROFILE_MEMORY"))) << 20 : 0;
        if (trace_from && n * sizeof(T) >= trace_from)
            std::fprintf(stderr, "[device memory] %.2f GB (%zu elements of %zu bytes), called from %p\n", (double)(n * sizeof(T)) * 1e-9, n, sizeof(T), __builtin_return_address(0));
        hipError_t e = hipMalloc((void **)&p, n * sizeof(T));
        if (e != hipSuccess) { device_free_pending(); e = hipMalloc((void **)&p, n * sizeof(T)); }      // (what was put aside may be the room that is missing)
        if (e != hipSuccess) { p = nullptr; return fail(RIBBIT_E_NOMEM, "hipMalloc(%zu bytes) failed: %s", n * sizeof(T), hipGetErrorString(e)); }
        cap = n;
        return RIBBIT_OK;
    }
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { if (p) (void)hipFree(p); }
};

// Page-locked host memory (api_core.cpp).  From PINNED_HUGE_FROM bytes on: anonymous memory advised into 2-MB pages, touched on
// several threads, then registered with the runtime -- measured on the GPU box (tools/probes/pin_probe.hip, 8 GB): 0.05 s against
// 1.27 s for hipHostMalloc, the copies into it at the same 53 GB/s.  The composed planes' host copy is 3 GB for a chromosome at
// -M 100 and 15.5 GB at -M 500 (2.5 s of a 15-s run before).  Falls back to hipHostMalloc wherever a step fails.
int pinned_alloc(size_t bytes, void **out);      // RIBBIT_OK / RIBBIT_E_NOMEM (fail() has the message)
void pinned_free(void *p);

template <typename T>
struct PinnedBuf {
    T *p = nullptr;
    size_t cap = 0;
    int ensure(size_t n, bool grows = false) {
        if (n <= cap) return RIBBIT_OK;
        if (grows) n = std::max(n + std::min(n / 4, ((size_t)256 << 20) / sizeof(T)), cap + std::min(cap / 2, ((size_t)1 << 30) / sizeof(T)));      // (as DevBuf)
        if (p) { pinned_free_later(p); p = nullptr; cap = 0; }
        void *q = nullptr;
        const int rc = pinned_alloc(n * sizeof(T), &q);
        if (rc) return rc;
        p = static_cast<T *>(q);
        cap = n;
        return RIBBIT_OK;
    }
    PinnedBuf() = default;
    PinnedBuf(const PinnedBuf &) = delete;
    PinnedBuf &operator=(const PinnedBuf &) = delete;
    ~PinnedBuf() { pinned_free(p); }
};

// A stream / an event of a handle: created by the handle (OwnedStream::create, OwnedEvent::create), destroyed with it -- a stream
// after what is still enqueued on it.  Both read as the plain HIP type.
struct OwnedStream {
    hipStream_t s = nullptr;
    OwnedStream() = default;
    OwnedStream(const OwnedStream &) = delete;
    OwnedStream &operator=(const OwnedStream &) = delete;
    ~OwnedStream() { if (s) { (void)hipStreamSynchronize(s); (void)hipStreamDestroy(s); } }
    hipError_t create() { return hipStreamCreateWithFlags(&s, hipStreamNonBlocking); }
    operator hipStream_t() const { return s; }
};
struct OwnedEvent {
    hipEvent_t e = nullptr;
    OwnedEvent() = default;
    OwnedEvent(const OwnedEvent &) = delete;
    OwnedEvent &operator=(const OwnedEvent &) = delete;
    ~OwnedEvent() { if (e) (void)hipEventDestroy(e); }
    hipError_t create(unsigned flags = hipEventDefault) { return hipEventCreateWithFlags(&e, flags); }
    operator hipEvent_t() const { return e; }
};
struct FreeDeleter { void operator()(void *p) const { std::free(p); } };

inline double now_ms() {
    using namespace std::chrono;
    return duration<double, std::milli>(steady_clock::now().time_since_epoch()).count();
}

enum Stage { STAGE_NONE = 0, STAGE_PERFECT = 1, STAGE_SUBST = 2, STAGE_ANCHORED = 3 };      // how far the seed lists have come (rec.stage_done)

// What the device-side pairing of one scan's events works in (api_events.cpp: pair_prepare sizes it, enqueue_pairing uses it):
// the handle's, and the own ones of ribbit_hip_debug_pair_events and ribbit_hip_debug_pair_events_sharded.
struct PairBufs {
    DevBuf<uint32_t> d_counters;           // the scan's region counters (also zeroed by the pack kernel)
    DevBuf<uint64_t> d_pair_table;
    DevBuf<uint32_t> d_run_base, d_pair_partial, d_pair_status;
    DevBuf<RibbitRun> d_halves;
    PinnedBuf<uint32_t> h_pub;             // region counters + pairing status, written by the GPU (pair_publish_kernel)
    uint32_t *h_pub_dev = nullptr;         // the same memory as the device sees it
};

// ---- shared by the host sides of the row outputs (api_mask.cpp, api_repeats.cpp, api_loci.cpp, api_overlap.cpp, api_best.cpp, api_classes.cpp, api_compound.cpp,
// api_interruptions.cpp, api_nearest.cpp, api_composition.cpp)

// n elements as malloc memory the caller frees (never a null pointer, whatever n): a copy of src, or for the caller to fill
// when src is null; terminate: a zero element behind them
template <typename T>
int hand_out(const T *src, size_t n, bool terminate, T **out) {
    T *mem = static_cast<T *>(std::malloc((std::max<size_t>(n, 1) + (terminate ? 1 : 0)) * sizeof(T)));
    if (!mem) return fail(RIBBIT_E_NOMEM, "out of host memory");
    if (src && n) std::memcpy(mem, src, n * sizeof(T));
    if (terminate) mem[n] = T();
    *out = mem;
    return RIBBIT_OK;
}
// ... owned here until it is released to the caller (an entry point that hands out several and fails half way frees the first)
template <typename T>
using Handed = std::unique_ptr<T[], FreeDeleter>;
template <typename T>
int hand_out(const T *src, size_t n, bool terminate, Handed<T> &out) {
    T *mem = nullptr;
    const int rc = hand_out(src, n, terminate, &mem);
    out.reset(mem);
    return rc;
}

// the rows clipped to [0, length), the empty ones dropped, sorted by `less`: what the host twins sweep
struct ClippedRow { int64_t s, e; size_t index; };
template <typename Less>
std::vector<ClippedRow> clipped_sorted_rows(int64_t length, const int32_t *intervals, size_t n, Less less) {
    std::vector<ClippedRow> rows;
    rows.reserve(n);
    for (size_t i = 0; i < n; ++i) {
        const int64_t s = std::max<int64_t>(intervals[2 * i], 0), e = std::min<int64_t>(intervals[2 * i + 1], length);
        if (s < e) rows.push_back(ClippedRow{s, e, i});
    }
    std::sort(rows.begin(), rows.end(), less);
    return rows;
}
// ... by start (among equals by index)
inline std::vector<ClippedRow> clipped_sorted_rows(int64_t length, const int32_t *intervals, size_t n) {
    return clipped_sorted_rows(length, intervals, n, [](const ClippedRow &a, const ClippedRow &b) { return a.s != b.s ? a.s < b.s : a.index < b.index; });
}

// ... merged into their runs of covered positions: what the host twins of the overlap and of the composition count coverage with
struct CoveredRuns {
    std::vector<int64_t> start, end, before;      // ascending, disjoint, not abutting; before[k]: covered positions before run k
    int64_t covered = 0;
    explicit CoveredRuns(const std::vector<ClippedRow> &sorted) {
        for (const ClippedRow &r : sorted) {
            if (start.empty() || r.s > end.back()) {
                start.push_back(r.s);
                end.push_back(r.e);
            } else {
                end.back() = std::max(end.back(), r.e);
            }
        }
        for (size_t k = 0; k < start.size(); ++k) {
            before.push_back(covered);
            covered += end[k] - start[k];
        }
    }
    int64_t covered_before(int64_t p) const {
        const size_t k = (size_t)(std::upper_bound(start.begin(), start.end(), p) - start.begin());      // runs that start at or before p
        return k == 0 ? 0 : before[k - 1] + std::min(p, end[k - 1]) - start[k - 1];
    }
    int64_t covered_in(const ClippedRow &r) const { return covered_before(r.e) - covered_before(r.s); }
};

}  // namespace rbapi

using namespace rbapi;

struct RibbitHandle {
    // ORDER MATTERS HERE, and only here: members are destroyed last to first, and the handle gives up its buffers first, then its
    // events, then its streams.  So the streams are declared first, the events second, and everything that owns memory (DevBuf,
    // PinnedBuf, bed_raw; `win`, with the events of its stages) after them.  ~RibbitHandle (api_core.cpp) runs before any member goes: it drains the streams.
    OwnedStream own_stream;
    OwnedStream copy_stream;             // post stream of the perfect scan: pairing kernels and result copies, so that they overlap
                                         // the next record's kernels when several handles share `stream`
    OwnedStream up_stream;               // uploads: the next record's bases travel while this record's kernels run (created by the first upload)
    OwnedEvent ev_ready;                 // pairing done, counters and status on the host
    struct Timers {                      // timers RIBBIT_TIME_PACK, RIBBIT_TIME_SCAN (the last scan's kernel) and RIBBIT_TIME_GPU (its whole GPU side),
        OwnedEvent begin[3], end[3];     // indexed by those ids; have: both events of the interval have been recorded
        bool have[3] = {false, false, false};
    } timers;
    OwnedEvent ev_xa;                    // the copy of the composed planes has landed
    OwnedEvent ev_ssw;                   // orders the longest alignment class (on the copy stream) against the compute stream
    OwnedEvent ev_up, ev_busy;
    OwnedEvent ev_planes;                // between the two kernels of the anchored stage (planes | window scan)

    RibbitHandle() = default;
    RibbitHandle(const RibbitHandle &) = delete;
    RibbitHandle &operator=(const RibbitHandle &) = delete;
    ~RibbitHandle();

    RibbitScanParams params{};
    int device = 0;
    int min_shift = 1, max_shift = 102;
    hipStream_t stream = nullptr;        // own_stream, or the caller's (ribbit_hip_set_stream): not owned
    // everything here is forgotten when a record is loaded; a cached result's flag belongs here
    struct RecordState {
        bool runs_valid = false, calls_valid = false, subst_calls_valid = false, anchored_calls_valid = false;
        bool longest_valid = false, best_rows_valid = false, small_valid = false;
        bool sym_valid = false;               // d_sym holds the loaded record
        bool host_planes_valid = false;
        bool eval_valid = false;              // d_eval / d_first_rev belong to the loaded record
        bool xa_on_device = false;            // the anchored kernel has written the composed planes of the loaded record
        int stage_done = STAGE_NONE;          // how far the seed lists have been advanced
        bool coverage_valid = false;          // rows.d_mask_bits is the coverage of the coverage_n rows in rows.h_mask_iv / d_mask_iv (build_coverage)
        size_t coverage_n = 0;
        bool base_prefix_valid = false;       // rows.d_comp_sums holds the base prefix of the loaded record (api_composition.cpp)
        bool overlap_valid = false;           // rows.h_overlap is the overlap of those rows with the overlap_n intervals in rows.h_overlap_iv (api_overlap.cpp)
        size_t overlap_n = 0;
        rb::ScanSplit last_split[RIBBIT_SCAN_KERNELS];   // the split each scan kernel last ran with on the loaded record
    } rec;
    bool timing = true;           // record the HIP events behind ribbit_hip_last_timing_ms (each costs a barrier packet on the stream)
    double host_ms = 0.0;         // post-processing of the last scan after its pairing (device state machine, sort, read-back), wall clock
    double merge_ms = 0.0;        // sequential host merge of the last window stage, wall clock
    double subst_merge_ms = 0.0;  // ... of the substitution stage when ribbit_hip_seeds_anchored ran both
    unsigned host_threads = 0;    // worker threads of the host stages (0 = RIBBIT_THREADS or min(cores, 16): rb::host_thread_count)

    bool loaded = false;
    int64_t length = 0;
    int64_t ntiles = 0, total_words = 0, tail_words = 0;
    DevBuf<uint8_t> d_ascii;
    DevBuf<uint32_t> d_hi, d_lo, d_brk;
    DevBuf<uint64_t> d_events, d_dense;
    DevBuf<uint32_t> d_query;
    DevBuf<uint32_t> d_xa;             // composed planes XA_m, motif-major
    int64_t xa_stride = 0;
    PinnedBuf<uint64_t> h_events;
    PinnedBuf<uint32_t> h_counters;
    PinnedBuf<uint32_t> h_query;

    // host copy of the packed planes: answers the sparse, latency-bound range reads of the
    // sequential merges (retainNestedSeed & co) without a GPU round trip per query
    rb::HostPlanes host;

    // ordered view of the last event collection
    int64_t last_event_count = 0;
    std::vector<uint64_t> chunk_table;   // (offset, count) per (motif, tile)
    size_t table_ntile = 0;

    std::vector<RibbitRun> runs;          // chunk-local pairing (multi-GPU path)
    // device-side pairing of the perfect scan: scratch + the pinned run list it lands in
    PairBufs pb;
    PinnedBuf<RibbitRun> h_runs, h_halves;
    rb::PairLaunch pair{};                // the perfect scan in flight (perfect_begin .. perfect_finish)
    bool pair_pending = false;
    size_t debug_first_cap = 0;           // ribbit_hip_debug_set_event_capacity: first guess of the event capacity (tests of the overflow path)
    size_t debug_small_record_cap = 0;    // ribbit_hip_debug_set_small_record_capacity: records of the small-motif arena (0 = 4 n + 2^20)
    int32_t debug_split[RIBBIT_SCAN_KERNELS] = {};   // ribbit_hip_debug_set_scan_split: motifs per block of each scan kernel (0 = automatic)
    bool counters_clean = false;          // pb.d_counters zeroed by the pack kernel and not used since
    bool copy_pending = false;            // result copies enqueued but not yet waited for (ribbit_hip_scan_perfect_end with wait = 0)
    size_t n_runs = 0, n_halves = 0;
    // window stages on the device (window_stage.hip): scratch of the streak -> call pipeline and its pinned results
    DevBuf<uint32_t> d_eval, d_first_rev, d_word_tmp, d_last_word, d_bitmap, d_edge_tmp, d_edge_end1, d_ws_counters;
    DevBuf<uint64_t> d_group, d_sort_keys, d_sort_vals, d_edge_keys, d_edge_vals, d_edge_keys2, d_edge_vals2;
    DevBuf<int32_t> d_min_span, d_pend, d_tj;
    DevBuf<uint32_t> d_dropmap;           // group filter of the anchored scan: ends of the groups it dropped
    bool dropmap_valid = false;           // the last anchored scan ran with the filter
    DevBuf<RibbitCall> d_flush;
    DevBuf<uint8_t> d_scratch;
    // per window stage, indexed by RIBBIT_STAGE_SUBST / RIBBIT_STAGE_ANCHORED (entry RIBBIT_STAGE_PERFECT stays empty): its results,
    // page-locked (both stages' kernels run before either merge), and the events around its scan kernel(s)
    struct WindowStage {
        PinnedBuf<RibbitCall> h_calls, h_flush;
        PinnedBuf<int32_t> h_pend;
        PinnedBuf<uint32_t> h_ws;
        OwnedEvent ev_begin, ev_end;
        bool have_timing = false;
    } win[3];
    PinnedBuf<uint32_t> h_xa;          // host copy of the composed planes (rb::HostPlanes::xa_view points here)
    // the anchored stage's merge as device work (api_merge.cpp, anchored_merge.hip): the lists, the ranges and what they leave
    struct MergeBufs {
        DevBuf<RibbitSeed> d_perfect, d_subst, d_own;
        DevBuf<int32_t> d_type0, d_cuts;                // types before the stage (perfect then substitution list); cut_pos | cur0
        DevBuf<uint32_t> d_first, d_range_out, d_log, d_head_log, d_counts, d_scratch;
        PinnedBuf<RibbitSeed> h_own;
        PinnedBuf<uint32_t> h_range_out, h_log, h_head_log, h_counts, h_sync;      // h_sync: read and written by the lanes while the kernel runs
        uint32_t *h_sync_dev = nullptr;
    } mg;
    bool xa_copy_pending = false;
    int64_t last_streaks = 0, last_calls = 0, last_edge_calls = 0;
    rb::CallVec perfect_calls;
    rb::CallVec subst_calls;
    rb::CallVec anchored_calls;
    rb::SeedVec dispatch;
    std::vector<int32_t> longest_runs;
    DevBuf<RibbitSeed> d_seeds;
    DevBuf<RibbitSeed> d_seeds_small;     // the consensus-row scan's jobs (the small-motif scan beside it reads d_seeds: the dispatch list as build_longest_runs left it)
    PinnedBuf<RibbitSeed> h_seed_stage;   // the dispatch list on its way up
    PinnedBuf<int32_t> h_longest_stage;   // ... and the longest runs on their way down
    DevBuf<int32_t> d_longest;
    DevBuf<uint8_t> d_sym;
    DevBuf<uint32_t> d_small_records, d_small_count;        // possibleMotifs of the dispatched seeds (small_motifs.hip)
    DevBuf<int32_t> d_small_head;
    PinnedBuf<int32_t> small_head;                          // 4 per dispatched seed; flags (4 i + 3) != 0: no device result
    PinnedBuf<uint32_t> small_records;
    size_t n_small_records = 0;
    DevBuf<unsigned long long> d_best;
    DevBuf<int32_t> d_slices;
    DevBuf<int32_t> d_ssw_jobs, d_ssw_order, d_ssw_out;   // batched striped passes (ssw_kernels.hip)
    DevBuf<uint8_t> d_ssw_pool;
    DevBuf<int32_t> d_path_items, d_path_result;
    DevBuf<uint64_t> d_path_cell_off, d_path_ops_off;
    DevBuf<uint8_t> d_path_cells;
    DevBuf<uint32_t> d_path_scratch, d_path_ops, d_path_count;
    PinnedBuf<uint32_t> h_path_ops;
    std::vector<rb::SswPath> ssw_paths;                    // per job of h->jobs: the path the GPU found (ops == null: none)
    std::vector<rb::SswEnds> ssw_ends;                     // per job of h->jobs; flag -1 = not computed on the GPU          // {job, first row} per 64-row slice of the long-motif seeds
    std::vector<int32_t> best_rows;       // per dispatch seed: mostFrequentLongerMotif's window start, or -1
    std::vector<RibbitAlignJob> jobs;
    std::string motif_pool;
    std::vector<uint64_t> export_events, export_counts;
    std::string host_ascii;   // the record's bases on the host when they had to be fetched back (refinement slices them for the aligner)
    bool host_ascii_valid = false;
    const char *host_bases = nullptr;     // where refinement reads the bases: the caller's page-locked buffer (load_record_pinned) or host_ascii
    bool planes_timing_valid = false;     // the anchored stage's ev_begin .. ev_planes .. ev_end bracket the two kernels of one run
    const uint8_t *dev_ascii_src = nullptr;
    std::string bed;
    std::unique_ptr<char[], FreeDeleter> bed_raw;   // the text of the last refinement when its pieces were joined (join_pieces: storage the copying threads touch first)
    size_t bed_raw_len = 0, bed_raw_cap = 0;
    bool bed_in_raw = false;              // the last ribbit_hip_refine_bed returned bed_raw, not bed
    rb::SeedLists lists;
    bool refine_met_empty_query = false;  // the last ribbit_hip_refine_bed on this handle met an alignment with an empty query (ribbit_hip_refine_met_empty_query)
    // the row outputs of the loaded record (api_mask.cpp, api_repeats.cpp, api_loci.cpp, api_overlap.cpp, api_best.cpp, api_classes.cpp, api_compound.cpp,
    // api_interruptions.cpp, api_nearest.cpp, api_composition.cpp)
    struct RowBufs {
        // shared by all of them, because every row output ends in a synchronise of the handle's stream and keeps none of the three
        // between calls: the inputs on their way down and on the device (stage_down lays them out), and the one device work buffer.
        // A call sizes d_work once, before it enqueues anything, by the layout its .hip file states (rb::BestLayout and the others,
        // kernels.h): every intermediate array, the result on the device and the temporary storage of the rocPRIM scans, sorts,
        // selects and reductions are regions of it.  The masked text and the density are all of it; the loci and the repeats take
        // only that temporary storage from it.  What is named below is pinned (a result stays valid until the handle's next same
        // call, load or close), or a cache that a later call reads, or a device buffer that is sized by a count the host reads in
        // the middle of a call, when d_work, if it grew, would move what the first half wrote.
        PinnedBuf<uint8_t> h_in;
        DevBuf<uint8_t> d_in, d_work;
        // the masked body of the loaded record (api_mask.cpp): coverage bitmap and intervals (rec.coverage_valid), the text on its way up
        DevBuf<uint32_t> d_mask_bits;
        DevBuf<int32_t> d_mask_iv;
        PinnedBuf<int32_t> h_mask_iv;
        PinnedBuf<char> h_mask_text;
        // the repeat sequences of the loaded record (api_repeats.cpp): the rows with the name behind them, their entry offsets, the
        // first row of every output span, k and the byte count on their way up, the text of one batch (sized by k)
        DevBuf<int32_t> d_rep_iv;
        DevBuf<int64_t> d_rep_off;
        DevBuf<int32_t> d_rep_span_row;
        DevBuf<int64_t> d_rep_pick;
        DevBuf<uint8_t> d_rep_text;
        PinnedBuf<int32_t> h_rep_iv;
        PinnedBuf<int64_t> h_rep_pick;
        PinnedBuf<char> h_rep_text;
        // the loci of the loaded record (api_loci.cpp), from d_mask_bits: the lanes' run ranks, the runs (starts | ends) with the
        // loci's starts and covered prefixes behind them, the join's prefixes with the rows' keys behind them, the loci (all sized
        // by the number of runs) and their number on their way up; the density's windows on their way up
        DevBuf<uint64_t> d_loci_off, d_loci_u64;
        DevBuf<int32_t> d_loci_i32;
        DevBuf<RibbitLocus> d_loci;
        PinnedBuf<uint64_t> h_loci_count;
        PinnedBuf<RibbitLocus> h_loci;
        PinnedBuf<int32_t> h_density;
        // the rows against a second set of intervals (api_overlap.cpp): those intervals as the last call staged them and its result,
        // the totals, then (others, bases) per row (rec.overlap_valid)
        PinnedBuf<int32_t> h_overlap_iv;
        PinnedBuf<int32_t> h_overlap;
        // the results on their way up: the best rows (the totals, then the chosen indices), the motif classes (the header, the
        // groups, the strands, the classes), the compound loci (the counts, the chains, the members), the CIGARs decoded (the counts;
        // the rows, the interruptions, the offsets, the observed bases, which are gathered on the device into d_int_text, sized by
        // the counts), the nearest targets, the base composition of the rows and of the windows
        PinnedBuf<int32_t> h_best;
        PinnedBuf<uint8_t> h_class;
        PinnedBuf<uint8_t> h_cmp;
        PinnedBuf<uint8_t> h_int_totals;
        DevBuf<uint8_t> d_int_text;
        PinnedBuf<uint8_t> h_int;
        PinnedBuf<RibbitNearest> h_near;
        PinnedBuf<RibbitRowComposition> h_comp_rows;
        PinnedBuf<RibbitBaseCounts> h_comp_windows;
        PinnedBuf<RibbitRowPrimers> h_primers;          // the targets' primers on their way up (api_primers.cpp)
        PinnedBuf<RibbitRowPrimerPair> h_primer_pairs;  // the targets' primer pairs on their way up (api_primer_pairs.cpp)
        // the oligos' sites and the pairs' products (api_primer_products.cpp): the patterns' lists, sized by the unique oligos the
        // host reads in the middle of the call, and the kept lists one behind the other, sized by their sum; the header, the
        // records (RibbitOligoSites or RibbitRowProducts) and the positions on their way up
        DevBuf<int32_t> d_site_lists, d_site_flat;
        PinnedBuf<uint32_t> h_product_header;
        PinnedBuf<uint8_t> h_products;
        PinnedBuf<int32_t> h_site_positions;
        // the specific primer pairs (api_primer_specific.cpp): the three records of every target on their way up, one array behind the
        // other; a batch's number of oligos on its way up; the targets or pairs of a batch of every caller of search_sites (0: by the
        // rule of site_batch)
        PinnedBuf<uint8_t> h_specific;
        PinnedBuf<uint32_t> h_specific_header;
        size_t specific_batch = 0;
        // the shortlists that leave the record and their verdicts on a record (api_primer_genome.cpp): the targets' records on their
        // way up, a batch's lists and side counts (or verdicts) as the device holds them behind them
        PinnedBuf<uint8_t> h_shortlists, h_verdicts;
        // the pairs typed on a record (api_amplicons.cpp): one RibbitRowAmplicon per pair on its way up
        PinnedBuf<uint8_t> h_amplicons;
        // the pairs pooled into panels (api_panel.cpp): the header, then one RibbitPanelRow per pair on its way up
        PinnedBuf<uint8_t> h_panel;
        // the markers' alleles over many samples (api_alleles.cpp): one RibbitRowAlleles per marker on its way up
        PinnedBuf<uint8_t> h_alleles;
        // the blocks' base counts | their prefix, which belongs to the record (rec.base_prefix_valid, api_composition.cpp)
        DevBuf<rb::BaseSums> d_comp_sums;
        size_t rep_budget = 0;           // text budget of one batch of repeat sequences in bytes (0: REPEAT_TEXT_BUDGET)
    } rows;
    RibbitHandle *aux = nullptr;          // helper handle of ribbit_hip_refine_bed: streams and buffers of the long alignment batch
    std::vector<RibbitHandle *> feed_aux; // ... and of its further feeders (each takes every n-th slice of the short alignments)

    rb::DevicePlanes planes() const {
        rb::DevicePlanes pl;
        pl.hi = d_hi.p + rb::LEAD_WORDS;
        pl.lo = d_lo.p + rb::LEAD_WORDS;
        pl.brk = d_brk.p + rb::LEAD_WORDS;
        pl.length = length;
        pl.ntiles = ntiles;
        pl.tail_words = tail_words;
        return pl;
    }
};

namespace rbapi {


using DeviceCalls = rb::KeptCalls;      // views of handle-owned page-locked memory


// The loaded record as one chunk (plus halos) of a longer record: which scan positions are this chunk's (piece
// coordinates), from where on the piece's streak events are exact (0: the piece starts where the record starts), whether
// the piece ends where the record ends, and what to add to piece coordinates to get record coordinates.
struct ChunkWindow {
    uint32_t own_lo = 0, own_hi = 0xffffffffu, z_lo = 0;
    bool keep_flush = true;
    int32_t pos_offset = 0;
    bool inexact = false;          // out: an owned call's group reaches the piece's artificial left end
};

// ---- steps shared between the files (each is defined, and described, in the file the list above names)
int bind_device(const RibbitHandle *h);
int is_gfx950(int device);
int pack_loaded_ascii(RibbitHandle *h, const uint8_t *dev_ascii, int64_t length);
int ensure_host_planes(RibbitHandle *h);
// api_events.cpp: the steps of the event pass, in the order a scan takes them
inline size_t dropmap_words(int64_t length) { return (size_t)(length / 32 + 1) + 1024; }      // of the anchored scan's group filter
int pair_prepare(RibbitHandle *h, PairBufs &pb, int64_t length, int64_t own_lo, int64_t own_hi, int64_t pos_offset, rb::PairLaunch &pr);
size_t first_event_cap(const RibbitHandle *h, size_t per_base_x4);
int grow_event_cap(int attempt, uint32_t worst, size_t *cap);
int event_room(RibbitHandle *h, size_t *cap, rb::PairLaunch *pr);
int zero_counters(RibbitHandle *h, bool even_if_clean = false);
rb::PerfectLaunch scan_launch_args(const RibbitHandle *h, size_t cap, int kernel);
int enqueue_pairing(PairBufs &pb, const rb::PairLaunch &pr, const uint64_t *d_events, uint64_t *d_dense, size_t cap, hipStream_t stream);
struct Published { uint32_t worst = 0; uint64_t produced = 0; };
Published read_published(const PairBufs &pb);
int pairing_verdict(const PairBufs &pb, uint64_t produced, const char *noun, size_t *n, size_t *n_halves);
int collect_perfect_events(RibbitHandle *h);
rb::EventSource event_source(const RibbitHandle *h);
int perfect_wait(RibbitHandle *h);
int perfect_enqueue(RibbitHandle *h, size_t cap);
int perfect_begin(RibbitHandle *h, int64_t own_lo, int64_t own_hi, int64_t pos_offset);
int perfect_collect(RibbitHandle *h);
int perfect_finish(RibbitHandle *h, RibbitRun *dst, size_t dst_cap, RibbitRun *half_dst, size_t half_dst_cap, bool wait = true);
int run_perfect_scan_range(RibbitHandle *h, int64_t own_lo, int64_t own_hi, int64_t pos_offset, RibbitRun *dst, size_t dst_cap,
                           RibbitRun *half_dst = nullptr, size_t half_dst_cap = 0);
int run_perfect_scan(RibbitHandle *h);
int build_perfect_calls(RibbitHandle *h);
int advance_to_perfect(RibbitHandle *h);
int scan_and_pair_streaks(RibbitHandle *h, int stage /* RIBBIT_STAGE_SUBST | RIBBIT_STAGE_ANCHORED */, uint32_t *n_streaks, int (*filter_min_span)(int) = nullptr);
int window_stage_device(RibbitHandle *h, int stage, bool full, int (*min_span)(int), DeviceCalls *out, ChunkWindow *cw = nullptr);
// ... its second step, everything behind scan_and_pair_streaks (ribbit_hip_debug_window_calls runs it on caller-made streaks)
int window_calls_device(RibbitHandle *h, int stage, uint32_t n_streaks, bool full, const int32_t *min_span /* per motif */, ChunkWindow *cw,
                        bool dropmap_valid, size_t first_edge_cap /* 0: automatic */, double scan_ms, DeviceCalls *out);
void full_calls_from_device(const DeviceCalls &dc, rb::CallVec &calls);
int build_subst_calls(RibbitHandle *h);
void subst_merge(RibbitHandle *h, const DeviceCalls *dc);
double feeder_phase_ms(int k);      // (profiling: host phases of run_ssw_passes / run_ssw_paths, cumulative)
// api_merge.cpp: the first parallel pass of the anchored stage's merge on the device (d_calls / d_pend: the stage's kept calls as
// window_stage_device left them in device memory, d_pend null when kc.pend is)
rb::AnchoredDevicePass anchored_device_pass(RibbitHandle *h, RibbitCall *d_calls, const int32_t *d_pend);
int advance_to_subst(RibbitHandle *h);
int prepare_anchored(RibbitHandle *h);
int xa_copy_begin(RibbitHandle *h);
int xa_wait_host(RibbitHandle *h);
int build_anchored_calls(RibbitHandle *h);
void print_anchored_merge_profile(size_t seeds, const rb::MergeStats &st, double dispatch_ms, unsigned dispatch_ranges);
int advance_to_anchored(RibbitHandle *h);
// set-up and hand-over of the host-only entry points (ribbit_host_replay_calls, ribbit_host_merge_chunks), api_window.cpp
int check_caller_planes(const RibbitScanParams *params, int64_t length, const uint32_t *hi, const uint32_t *lo, const uint32_t *brk, size_t nwords, const uint32_t *xa, size_t xa_stride);
void lists_over_caller_planes(const RibbitScanParams *params, int64_t length, const uint32_t *hi, const uint32_t *lo, const uint32_t *brk, size_t nwords, rb::HostPlanes &hp, rb::SeedLists &sl);
void use_composed_planes(rb::SeedLists &sl, const rb::HostPlanes *hp);
int give_seed_lists(const rb::SeedLists &sl, const rb::SeedVec &dispatch, RibbitSeedLists *out);
int build_longest_runs(RibbitHandle *h);
int best_rows_of(RibbitHandle *h, const RibbitRefineParams &prm, const rb::SeedVec &seeds, const int32_t *longest, int32_t *best);
int build_best_rows(RibbitHandle *h, const RibbitRefineParams &prm);
int build_small_motifs(RibbitHandle *h, const RibbitRefineParams &prm, hipStream_t stream = nullptr);
int scan_seeds_side_by_side(RibbitHandle *h, const RibbitRefineParams &prm);
void fill_refine_defaults(RibbitRefineParams *p, int min_motif, int max_motif);
int ssw_class(const RibbitAlignJob &jb);
int run_ssw_passes(RibbitHandle *h, const RibbitAlignJob *jobs, size_t n, const char *pool, size_t pool_len, int mask_len,
                          std::vector<rb::SswEnds> &ends, unsigned classes = 0x1fu, bool pool_resident = false);
int run_ssw_paths(RibbitHandle *h, const RibbitAlignJob *jobs, size_t n, const std::vector<rb::SswEnds> &ends, std::vector<rb::SswPath> &paths);
// api_mask.cpp: the coverage bitmap of the loaded record (length > 0) under n rows in rows.d_mask_bits, rb::coverage_words(length)
// words, and the rows in rows.d_mask_iv, enqueued on the handle's stream; nothing is enqueued when the bitmap already is the one of these
// rows (coverage_is)
bool coverage_is(const RibbitHandle *h, const int32_t *intervals, size_t n);
int build_coverage(RibbitHandle *h, const int32_t *intervals, size_t n);
// api_mask.cpp: a row output's inputs on their way down.  The n_segs segments are copied into rows.h_in one behind the other, each
// on a 16-byte boundary, the tail zero-filled to 16 bytes past the last segment (the kernels read pools in aligned words, up to one
// word past their end); one copy to rows.d_in is enqueued on the handle's stream; at[i]: where segment i lies on the device.
// The caller ends in a synchronise of that stream, so the next call finds both buffers free.
inline size_t round16(size_t v) { return (v + 15) & ~(size_t)15; }
struct StageSegment { const void *p; size_t bytes; };
int stage_down(RibbitHandle *h, const StageSegment *segs, size_t n_segs, const uint8_t **at);
// api_primer_products.cpp: the site search of an in-silico PCR (kernels.h, at rb::ProductLayout) for n_oligos >= 1 oligos on the
// device, enqueued on the handle's stream with one synchronise in the middle.  product_work: the search's work buffer of room_bytes,
// the whole of rows.d_work or a region of it, which the caller has sized before its first launch: nothing here grows d_work.  The
// layout is carved for exactly these oligos (and n_pairs records in `out`) and must fit the room; the unique oligos are read back
// into rows.h_product_header (the caller's to size) and size rows.d_site_lists, which the scan fills.
struct SiteSearch {
    rb::ProductLayout at;      // offsets from product_work
    size_t uniques = 0;
};
int search_sites(RibbitHandle *h, const RibbitOligo *d_oligos, size_t n_oligos, size_t n_pairs, const RibbitProductParams &prm, uint8_t *product_work, size_t room_bytes,
                 bool use_filter, SiteSearch &out);
// ... and the items (targets, pairs) of one batch of a call that searches oligos_per_item oligos for each: as many as SITE_LIST_BYTES
// of site lists hold at the worst case of distinct oligos, or what ribbit_hip_debug_set_specific_batch asked for, within what one
// search takes
size_t site_batch(const RibbitHandle *h, size_t oligos_per_item, const RibbitProductParams &prm);

}  // namespace rbapi
