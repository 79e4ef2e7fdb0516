// kernels.h -- host-callable launchers of the gfx950 kernels (implemented in kernels.hip).
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include <algorithm>

#include "device_planes.h"
#include "ribbit_hip.h"

namespace rb {

// fasta_utils.cpp:78-115 -> packed planes.  total_words counts the LEAD padding too; the three
// output pointers are the raw allocations (NOT advanced by LEAD_WORDS).
// zero_words (may be null): n_zero words the kernel also clears (the event counters of the scan that follows).
void launch_pack(const uint8_t *dev_ascii, int64_t length, uint32_t *hi, uint32_t *lo, uint32_t *brk,
                 int64_t total_words, uint32_t *zero_words, int n_zero, hipStream_t stream);

struct PerfectLaunch {
    int m_lo, m_hi;        // motif (== shift) range scanned
    uint32_t ev_cap;       // capacity of the event buffer, in events
    int motifs_per_block = 0;   // split of the motif range over gridDim.y: 0 = the launcher's own choice, n > 0 = n motifs per
                                // block (clamped to the range; ribbit_hip_debug_set_scan_split)
};
// The motif split a scan launcher used: gridDim.y blocks of motifs_per_block motifs each (the last may hold fewer); {0, 0}
// when it launched nothing.
struct ScanSplit {
    int grid_y = 0, motifs_per_block = 0;
};
// parse_perfect_shiftxor.cpp:173-223 hot loop -> run START / END events.
// Events land in EV_SHARDS regions of ev_cap/EV_SHARDS events; counters[] (EV_COUNTER_WORDS words,
// zeroed by the caller) holds one count per region.  A count above the region size = overflow.
ScanSplit launch_scan_perfect(const DevicePlanes &pl, const PerfectLaunch &pp, uint64_t *events, uint32_t *counters,
                              hipStream_t stream);

// Window scan (parse_substitute_shiftxor.cpp:430-532 with allowed_mismatches = 1, i.e. threshold 7;
// parse_anchored_shiftxor.cpp:580-679 with 2, threshold 6) -> pass-streak START / END events at
// window-start positions.  Same event buffer conventions as launch_scan_perfect.
ScanSplit launch_scan_window(const DevicePlanes &pl, const PerfectLaunch &pp, int allowed_mismatches, uint64_t *events,
                             uint32_t *counters, hipStream_t stream);

// generateAnchoredShiftXORs (parse_anchored_shiftxor.cpp:20-56) + the composition of fasta_utils.cpp:143-161: xa receives the
// composed planes XA_m, motif-major, xa_stride words per motif.  Tiles are anchored_tile_words(anchored_halo_lanes(pp.m_hi))
// wide.  Requires pp.m_hi <= ANCHORED_MAX_MOTIF.  launch_scan_xa_window scans the planes.
ScanSplit launch_scan_anchored(const DevicePlanes &pl, const PerfectLaunch &pp, uint32_t *xa, int64_t xa_stride, hipStream_t stream);
// Group filter of the window scan below.  tj_table (may be null: no filter): per motif of the launch, the number of positions a
// group of pass-streaks must span for its call to be able to pass the stage's length filter (<= GROUP_FILTER_MAX; 0: keep every
// group); groups that cannot, and are not kept for another reason (see the kernel), emit no events and leave their end bit in
// dropmap (words 0 .. L/32, zeroed by the caller) instead.
constexpr int GROUP_FILTER_MAX = 16;
// The window scan of processShiftXORsAnchored on composed planes already in HBM (xa, xa_stride words per motif, readable up to
// word ntiles * TILE_WORDS + 2 of every plane): same events and filter as the fused kernel, tiles of TILE_WORDS words.
ScanSplit launch_scan_xa_window(const DevicePlanes &pl, const PerfectLaunch &pp, const uint32_t *xa, int64_t xa_stride, uint64_t *events,
                                uint32_t *counters, const int32_t *tj_table, uint32_t *dropmap, hipStream_t stream);

// Gathers the used part of every region into `dense` (same capacity) in shard order and writes
// counters[EV_SUMMARY] = total events, counters[EV_SUMMARY+1] = 1 if any region overflowed.
void launch_compact_events(const uint64_t *events, uint32_t ev_cap, uint32_t *counters, uint64_t *dense,
                           hipStream_t stream);

// Device-side pairing of the perfect scan's events (still in their EV_SHARDS regions, counters[] as the scan
// left them) into RibbitRun records ordered by (motif, start): parse_perfect_shiftxor.cpp:173-223's run
// bookkeeping.  table: nm*ntile 8-byte entries, run_base: nm*ntile words, partial: nm*ntile/1024+1 words,
// status: PAIR_STATUS_WORDS words (all device scratch, initialised here).  runs holds run_cap records.
struct PairLaunch {
    uint32_t m_lo, nm;        // first motif, number of motifs
    uint32_t ntile;           // tiles of tile_bases positions covering 0..L
    uint32_t tile_bases;      // positions per scan-kernel tile: TILE_BASES, or the anchored kernel's narrower tile
    uint32_t region_cap;      // events per region
    // chunk of a longer record: only runs whose START lies in [own_lo, own_hi) (positions of the loaded piece) are
    // reported, with pos_offset added; a whole record is own_lo = 0, own_hi = INT64_MAX, pos_offset = 0
    int64_t own_lo, own_hi, pos_offset;
};
// halves (half_cap >= 2*nm records) receives the runs cut by the own range, status[PAIR_HALVES] their number.
hipError_t launch_pair_runs(const uint64_t *events, const uint32_t *counters, const PairLaunch &pl, void *table,
                            uint32_t *run_base, uint32_t *partial, void *runs, uint32_t run_cap, void *halves,
                            uint32_t half_cap, uint32_t *status, hipStream_t stream);

// host_words (page-locked, device-visible): [0, EV_SHARDS) the region counters, then PAIR_STATUS_WORDS status words
void launch_pair_publish(const uint32_t *counters, const uint32_t *status, uint32_t *host_words, hipStream_t stream);

// After launch_compact_events: table[(motif - m_lo) * ntile + tile] = {first event index + 1, index past the last event}
// of that (motif, tile) chunk of `dense` (both 0: no chunk); *status != 0: malformed stream.
hipError_t launch_chunk_table(const uint64_t *dense, const uint32_t *counters, uint32_t m_lo, uint32_t nm, uint32_t ntile,
                              uint32_t tile_bases, void *table, uint32_t *status, hipStream_t stream);

// ---- window stages on the device (window_stage.hip): streaks -> addSeed calls -------------------------------
// counters of launch_window_calls (WS_WORDS words, zeroed by the caller)
enum : uint32_t { WS_N_MAIN = 0, WS_N_EDGE = 1, WS_FLAGS = 2, WS_MAX_END = 3 /* largest end + 1 of an in-loop call */,
                  WS_INEXACT = 4 /* != 0: an owned call's group reaches the piece's artificial left end (chunk mode) */, WS_WORDS = 8 };
enum : uint32_t {
    WS_TWO_FLUSH = 1,    // two end-of-sequence calls for one motif
    WS_BAD_MOTIF = 2,    // streak with a motif outside the launch
    WS_NOT_PROMPT = 4,   // an ordinary call whose end is not its position - 8 (would break the bound argument)
    WS_EDGE_LOST = 8,    // a kept edge call is missing from the main list
};
// E plane (bit q: window [q, q+7] is evaluated) and, reversed, the first word >= w that has an evaluated window;
// n_words = L/32 + 1 words each (brk must be readable one word further); word_tmp: n_words words of scratch
hipError_t launch_eval_planes(const uint32_t *brk, uint32_t n_words, uint32_t *eval, uint32_t *first_rev, uint32_t *word_tmp,
                              void *scratch, size_t scratch_bytes, hipStream_t stream);
// group[i] = (motif index << 32) | (start of the group streak i belongs to) + 1, streaks = the run records the
// pairing kernels made of a window scan's events (motif-major, by start)
hipError_t launch_group_starts(const RibbitRun *runs, uint32_t n, uint32_t m_lo, uint64_t *group, void *scratch,
                               size_t scratch_bytes, hipStream_t stream);
struct WindowCallsLaunch {
    const RibbitRun *runs; uint32_t n_streaks;
    const uint64_t *group;
    const uint32_t *eval, *first_rev, *brk; uint32_t n_words;
    int64_t length;
    uint32_t m_lo, nm;
    const int32_t *min_span;           // device, [nm]
    int full;                          // 1: all calls, unfiltered; 0: compact (filtered + bounds)
    uint64_t *keys, *vals; uint32_t cap;              // main list: key = pos << 10 | motif, val = start << 32 | end
    uint64_t *edge_keys, *edge_vals; uint32_t edge_cap;   // compact mode; val bit 63 = passes the filter
    RibbitCall *flush;                 // [nm], zeroed by the caller: the end-of-sequence call of each motif
    uint32_t *bitmap;                  // [n_words + 1], zeroed by the caller
    uint32_t *counters;                // [WS_WORDS], zeroed by the caller
    // chunk mode (the loaded record is a chunk of a longer record plus halos): only calls made at scan positions
    // own_lo <= pos < own_hi are this chunk's; z_lo: first position whose streak events are exact (0: the piece starts
    // where the record starts); keep_flush: the piece ends where the record ends.  Whole record: 0, 0xffffffff, 0, 1.
    uint32_t own_lo = 0, own_hi = 0xffffffffu, z_lo = 0;
    int keep_flush = 1;
};
void launch_window_calls(const WindowCallsLaunch &w, hipStream_t stream);
// after launch_window_calls (compact mode): folds the calls of the groups the anchored scan's filter dropped (dropmap: bit e =
// such a group ends at e; drop_words words) into bitmap[0 .. n_words] and counters[WS_MAX_END], own range only
void launch_merge_dropmap(const uint32_t *dropmap, uint32_t drop_words, uint32_t n_words, uint32_t own_lo, uint32_t own_hi, uint32_t *bitmap,
                          uint32_t *counters, hipStream_t stream);
hipError_t launch_sort_calls(uint64_t *keys_in, uint64_t *vals_in, uint64_t *keys_out, uint64_t *vals_out, uint32_t n, int key_bits,
                             void *scratch, size_t scratch_bytes, hipStream_t stream);
// bounds of the kept edge calls (edge list sorted by key) -> pend[index in the sorted main list]
hipError_t launch_edge_bounds(const uint64_t *edge_keys, const uint64_t *edge_vals, uint32_t n_edge, uint32_t *edge_tmp, uint32_t *edge_end1,
                              const uint32_t *bitmap, uint32_t *word_tmp, uint32_t *last_word1, uint32_t n_words, const uint64_t *main_keys,
                              uint32_t n_main, int32_t *pend, uint32_t *counters, int32_t pos_offset, void *scratch, size_t scratch_bytes,
                              hipStream_t stream);
// pos_offset: added to every coordinate (a chunk's piece coordinates -> record coordinates)
void launch_assemble_calls(const uint64_t *keys, const uint64_t *vals, uint32_t n, RibbitCall *out, int32_t pos_offset, hipStream_t stream);
// bytes of scratch the rocPRIM scans / sorts above need for these sizes
size_t window_stage_scratch_bytes(size_t n_streaks, size_t n_words, size_t n_calls, size_t n_edge, int key_bits);

// X_shift words [w0, w0+nw) -> out_words (device); if count != nullptr also adds the popcount of
// bits in [p0, p1) to *count.
void launch_plane_words(const DevicePlanes &pl, int shift, int64_t w0, int64_t nw, uint32_t *out_words,
                        int64_t p0, int64_t p1, uint32_t *count, hipStream_t stream);

// longestContinuousMatches (parse_seed.cpp:26-44) of n seeds {start,end,mlen,type} on the composed planes
void launch_seed_longest_runs(const uint32_t *xa, int64_t xa_stride, int m_lo, const void *seeds, int64_t n, int32_t *out,
                              hipStream_t stream);

// one byte per base (0..3 = A C G T, 4 = N) from the resident ASCII record
void launch_sym(const uint8_t *ascii, int64_t length, uint8_t *sym, hipStream_t stream);

// small_motifs.hip: possibleMotifs of every dispatched seed with m <= 10 (one wavefront per seed)
struct SmallMotifLimits {
    int32_t first_window[11];      // smallest j - seed_start with j - seed_start >= 0.9 m - 1 (parse_smallmotif_seed.cpp:96)
    int32_t min_length[11];        // MINIMUM_LENGTH[m]
    int32_t min_units[11];         // PERFECT_UNITS[m]
};
// longest != null: `jobs` is the dispatch list on the device ({start, end, m, type}) and longest[i] its seeds' longest runs; the
// kernel then selects the seeds itself (m <= 10, longest[i] >= longest_threshold) and a seed's index is its place in the list
void launch_small_motifs(const uint8_t *sym, int64_t length, const void *jobs, int64_t njobs, const SmallMotifLimits &lim, void *records,
                         uint32_t record_cap, uint32_t *record_count, void *head, hipStream_t stream, const int32_t *longest = nullptr,
                         int32_t longest_threshold = 0);
// mostFrequentLongerMotif's row scores (parse_seed.cpp:165-243) for njobs seeds {seed_start, seed_sequence_length, m, -}:
// best[job] = (best score << 32) | (0xffffffff - first row with that score), 0 when every row scores 0.
// best[] must be zeroed by the caller.  blocks[nblocks] = {job, first row of a 64-row slice of that seed}: every
// seed is covered by ceil(rows / 64) slices, rows = seed_sequence_length - m + 1 (clipped at the record end).
void launch_long_motif_rows(const uint8_t *sym, int64_t length, const void *jobs, int64_t njobs, const void *blocks,
                            int64_t nblocks, unsigned long long *best, hipStream_t stream);

// The two striped Smith-Waterman passes (ssw.c:843-891) of njobs alignment jobs (RibbitAlignJob records, 9 ints each):
// query = record[query_start, +query_length), reference = the job's motif repeated to ppr_length.  Jobs are launched in
// three size classes (order_small / order_big / order_huge: job indices, each list sorted by size); out[8*job .. +8) = score,
// ref_end, query_end, score2, ref_end2, ref_begin, query_begin, flag -- flag -1: too large for its class, not computed.
constexpr int SSW_SMALL_Q = 128, SSW_SMALL_R = 256, SSW_BIG_Q = 512, SSW_BIG_R = 1024, SSW_HUGE_Q = 2048, SSW_HUGE_R = 4096,
              SSW_GIANT_Q = 4096, SSW_GIANT_R = 8192,      // 61.6 KB of LDS per alignment: the most one workgroup gets by default
              SSW_COLOSSAL_Q = 8192, SSW_COLOSSAL_R = 16384;    // 124 KB: asked for with hipFuncAttributeMaxDynamicSharedMemorySize (a
                                                                // workgroup may have all 160 KB of a CU: tools/probes/lds_probe.hip)
// ssw_wave.hip: the same two passes, one wavefront per alignment (queries of 129..qcap bases, reference up to rcap)
void launch_ssw_passes_wave(const uint8_t *ascii, int64_t length, const uint8_t *motif_pool, const int32_t *jobs, const int32_t *order, int n,
                            int mask_len, int qcap, int rcap, int32_t *out, hipStream_t stream);
// ssw_group.hip: the same two passes, one WORKGROUP of `waves` (4, 8 or 16) wavefronts per alignment: a column's stripes dealt to
// the wavefronts, for the long classes.  ssw_group_fits: the class's longest query fits that many wavefronts.
bool ssw_group_fits(int qcap, int waves);
hipError_t launch_ssw_passes_group(const uint8_t *ascii, int64_t length, const uint8_t *motif_pool, const int32_t *jobs, const int32_t *order, int n,
                                   int mask_len, int qcap, int rcap, int waves, int32_t *out, hipStream_t stream);
void launch_ssw_passes(const uint8_t *ascii, int64_t length, const uint8_t *motif_pool, const int32_t *jobs,
                       const int32_t *order_small, int n_small, const int32_t *order_big, int n_big, const int32_t *order_huge, int n_huge,
                       int mask_len, int32_t *out, hipStream_t stream, int huge_group_waves = 0);
// huge_group_waves: 0 = the huge class on one wavefront per alignment (ssw_wave.hip), 4 / 8 = on a workgroup of that many

// The banded path search (ssw.c:590-775) of n_items alignments whose end points are known, one wavefront each (ssw_path.hip).
// items[4*t] = job index, items[4*t+1] = band of this round; cell_off[t] / ops_off[t]: where item t's cell bytes
// ((2*band+1) * read_len) and scratch operations (ref_len + read_len + 2 entries) go; finished paths are appended to
// path_ops (path_cap entries, *path_count their number so far); result[4*job..] = {state, band, first operation in
// path_ops, operations}: state 0 path found, 1 walk failed, 2 band too narrow (run again with twice the band).
// max_band: the largest band among the items (sizes the LDS).
constexpr int SSW_PATH_MAX_BAND = 2048;
constexpr int SSW_PATH_CODE_TABLE = 1024;      // bytes of LDS for the motif's base codes (a longer motif is read from global memory)
void launch_ssw_paths(const uint8_t *ascii, int64_t length, const uint8_t *motif_pool, const int32_t *jobs, const int32_t *ends,
                      const int32_t *items, const uint64_t *cell_off, const uint64_t *ops_off, int n_items, int max_band,
                      uint8_t *cells, uint32_t *ops, uint32_t *path_ops, uint32_t path_cap, uint32_t *path_count, int32_t *result,
                      hipStream_t stream, int n_narrow = 0);
// n_narrow: the first n_narrow items have a band of at most SSW_PATH_NARROW_BAND and run four to a wavefront (ssw_path4_kernel);
// max_band then is the largest band among the OTHERS.
constexpr int SSW_PATH_NARROW_BAND = 7;

// anchored_merge.hip: the anchored stage's seed-list merge (parse_anchored_shiftxor.cpp:113-534, merge_types.cpp:11-189), one lane
// per independent range of the stage's kept calls (parallel_merge.h).  P / S: the perfect and substitution lists on the device (their
// `type` fields change: retirements); *_type0: the types before the stage; first[nr + 1], cut_pos[nr], cur0[2 nr]: the ranges' first
// calls, left cuts and starting cursors; own: n_calls + nr entries, range k's part of the anchored list at first[k] + k (entry 0 of
// every range but the first is the sentinel); range_out[AM_RANGE_OUT_WORDS k ..]: entries in own, status (AM_* bits: the host merges
// the range itself), guard count (2 words), final cursors (2), by-counter head reads (2 x 2), calls taken, the lane's time; log: 4 words per entry
// {kind << 28 | range, list << 31 | index, old type or "was live", 0}; head_log: 8 words per logged list-head write
// {range, list, index, start, end, mlen, type, 0}.
constexpr int AM_PS_CAP = 12, AM_CAND_CAP = 40;      // candidate lists of a call: this much of them in LDS (208 bytes per lane, 13 KB per wavefront) ...
constexpr int AM_CHILD_CAP = 128, AM_COV_CAP = 48, AM_MAX_ROUNDS = 1 << 20;
constexpr int AM_PS_SPILL = 244, AM_CAND_SPILL = 984;      // ... and what a dense locus has beyond, in global memory (256 / 1024 entries in all)
constexpr int AM_SCRATCH_WORDS = 2 * AM_CHILD_CAP + 3 * AM_COV_CAP + AM_PS_SPILL + AM_CAND_SPILL;
constexpr int AM_RANGE_OUT_WORDS = 12;
constexpr int AM_RESIDENT_WAVES = 12 * 256;      // what the chip holds at once: twelve wavefronts per CU (LDS, and three per SIMD by registers)
constexpr uint32_t AM_MAX_PASSES = 12000;        // a range that takes its lane more passes than this (80 ms) is given up: AM_TOO_SLOW
enum : uint32_t { AM_SCRATCH_FULL = 1u, AM_LOG_FULL = 2u, AM_BAD_PLANE = 4u, AM_RUNAWAY = 8u, AM_TOO_SLOW = 16u };
enum : uint32_t { AM_LOG_UNDO = 1u, AM_LOG_READ = 2u };
struct AnchoredMergeArgs {
    RibbitSeed *P, *S;
    uint32_t nP, nS;
    const int32_t *P_type0, *S_type0;
    RibbitCall *calls;                // (their `pos` fields are overwritten with the calls' cursor bounds)
    const int32_t *pend;              // may be null
    const uint32_t *first;
    const int32_t *cut_pos, *cur0;
    uint32_t nr;
    const uint32_t *xa;
    int64_t xa_stride, length;
    int32_t m_lo, m_hi;
    RibbitSeed *own;
    uint32_t *range_out;
    uint32_t *log, *log_count;
    uint32_t log_cap;
    uint32_t *head_log, *head_count;
    uint32_t head_cap;
    uint32_t *scratch;                // AM_SCRATCH_WORDS per LANE of the launch (64 AM_RESIDENT_WAVES at most)
    uint32_t *next_range;             // zero at launch: the lanes take ranges from it, in the order of ...
    const uint32_t *order;            // ... the ranges to merge (n_order of the nr; the others are not touched)
    uint32_t n_order;
    uint32_t *sync;                   // page-locked host memory: [0] entries of `order` left to the lanes (the host threads take from the back), [1] entries the lanes have taken
    uint32_t max_passes;              // a range that needs more passes of its lane's loop than this is left to the host (AM_TOO_SLOW)
};
void launch_anchored_merge(const AnchoredMergeArgs &a, uint32_t n_calls, uint32_t resident_waves /* <= AM_RESIDENT_WAVES */, hipStream_t stream);
void launch_seed_types(const RibbitSeed *seeds, uint32_t n, int32_t *types, hipStream_t stream);      // types[i] = seeds[i].type

// blocks for `items` items, `per_block` of them to a block: at least one, at most `cap` (a striding kernel takes the rest)
inline unsigned grid_for(int64_t items, int per_block, int64_t cap) {
    return (unsigned)std::max<int64_t>(1, std::min<int64_t>((items + per_block - 1) / per_block, cap));
}

// mask.hip: the repeat mask of the loaded record (api_mask.cpp).  bits: length / 32 + 1 words, zeroed by the caller;
// intervals: n (start, end) pairs, clipped to [0, length) on the device.  format: width in 1 .. length (the caller maps
// 0 and anything longer to length), out: out_len = length + ceil(length / width) bytes, rounded up to 16.
void launch_mask_coverage(const int32_t *intervals, int64_t n, int64_t length, uint32_t *bits, hipStream_t stream);
void launch_mask_format(const uint8_t *ascii, int64_t length, const uint32_t *bits, int64_t nwords, int hard, int64_t width,
                        int64_t out_len, uint8_t *out, hipStream_t stream);

// repeats.hip: the repeat sequences of the loaded record with their flanks (api_repeats.cpp).  The format kernel writes
// REPEAT_SPAN output bytes per workgroup; span_row holds the first row of every span.
constexpr int64_t REPEAT_SPAN = 4096;
size_t repeat_scan_scratch_bytes(int64_t m);
// off: m + 1 entry offsets of the m rows of iv (off[0] = 0, off[i + 1] - off[i] = length of entry i); then pick[0] = k, the
// largest k in 1 .. m with off[k] <= budget (1 when there is none), and pick[1] = off[k].  m >= 1.
hipError_t launch_repeat_offsets(const int32_t *iv, int64_t m, int64_t length, int32_t flank, int32_t name_len, int64_t budget,
                                 int64_t *off, int64_t *pick, void *scratch, size_t scratch_bytes, hipStream_t stream);
// the entries of rows [0, k): total = off[k] bytes into out (rounded up to 16; bytes past total are 0); span_row:
// ceil(total / REPEAT_SPAN) + 1 ints.  ascii: the record's bases (any alignment), name: name_len bytes on the device.
void launch_repeat_format(const uint8_t *ascii, int64_t length, const int32_t *iv, const int64_t *off, int64_t k, int64_t total,
                          int32_t flank, const char *name, int32_t name_len, int32_t *span_row, uint8_t *out, hipStream_t stream);

// loci.hip: merged loci and the density track of the loaded record from the mask's coverage bitmap (api_loci.cpp).
// bits: coverage_words(length) words, zeroed and then filled by launch_mask_coverage: padded so that a lane of the run
// kernels reads its LOCI_LANE_WORDS words and the word behind them without a bound check (the padding stays zero).
constexpr int64_t LOCI_LANE_WORDS = 8;
inline int64_t coverage_words(int64_t length) { return ((length / 32 + 1) + LOCI_LANE_WORDS - 1) / LOCI_LANE_WORDS * LOCI_LANE_WORDS + LOCI_LANE_WORDS; }
inline int64_t loci_lanes(int64_t length) { return ((length / 32 + 1) + LOCI_LANE_WORDS - 1) / LOCI_LANE_WORDS; }
size_t loci_scan_scratch_bytes(int64_t items);
// off: loci_lanes(length) + 1 packed ranks, off[t] = (run starts before lane t's words) << 32 | (run ends before them);
// off[lanes] holds the number of runs in both halves
hipError_t launch_run_ranks(const uint32_t *bits, int64_t length, uint64_t *off, void *scratch, size_t scratch_bytes, hipStream_t stream);
// run_start / run_end: the n_runs runs in ascending order, half-open
void launch_run_bounds(const uint32_t *bits, int64_t length, const uint64_t *off, int32_t *run_start, int32_t *run_end, hipStream_t stream);
// The gap join and the rows of every locus.  join: n_runs packed prefixes (locus id + 1) << 32 | covered positions so far;
// locus_start / post: n_runs ints (the loci's starts for the rows' search; covered positions up to each locus's end);
// key: n_runs zeroed words, loci: n_runs zeroed records; count[0] = number of loci.  intervals: the n rows on the device.
hipError_t launch_loci(const int32_t *run_start, const int32_t *run_end, int64_t n_runs, int32_t gap, const int32_t *intervals, int64_t n,
                       int64_t length, uint64_t *join, int32_t *locus_start, int32_t *post, unsigned long long *key, RibbitLocus *loci,
                       uint32_t *count, void *scratch, size_t scratch_bytes, hipStream_t stream);
// covered[k] = covered positions of [k window, min((k + 1) window, length)), k < n_windows = ceil(length / window)
void launch_density(const uint32_t *bits, int64_t length, int64_t window, int64_t n_windows, int32_t *covered, hipStream_t stream);

// ---- the row outputs that carve one device work buffer (overlap.hip, best.hip, classes.hip, compound.hip, interruptions.hip,
// nearest.hip, composition.hip, primers.hip).  Each states its regions once, as a layout of byte offsets made by one function beside its kernels:
// every intermediate array, the result on the device, and one region for the temporary storage of its rocPRIM calls (the most any
// of them asks for these sizes: the function asks them, so it needs the device).  The api file sizes the handle's work buffer by
// `bytes`; launch_* takes that buffer with its size and the layout, derives its pointers from the layout and refuses a buffer
// smaller than `bytes` (hipErrorInvalidValue) before it enqueues anything.
// take(bytes): the offset of the next region.  Regions start on multiples of 256 bytes, hipMalloc's own granularity.
// Every layout ends in the region of rocPRIM's temporary storage: close(at, most) takes it last and sets the buffer's size.
struct WorkLayout {
    size_t scratch, scratch_bytes, bytes;      // rocPRIM's temporary storage, as much as the primitives' queries ask for (no slack); the whole buffer
};
struct WorkCarver {
    size_t end = 0;
    size_t take(size_t bytes) { const size_t from = end; end += (bytes + 255) & ~(size_t)255; return from; }
    void close(WorkLayout &at, size_t scratch_bytes) { at.scratch_bytes = scratch_bytes; at.scratch = take(scratch_bytes); at.bytes = end; }
};
template <typename T>
T *region(uint8_t *work, size_t offset) { return reinterpret_cast<T *>(work + offset); }

// overlap.hip: the rows of the loaded record (length > 0) against a second set of intervals (api_overlap.cpp).  a_bits: the
// coverage bitmap of the n rows as loci.hip takes it; other: the n_other intervals in page-locked host memory, copied down and made
// into their own bitmap by the launch.  totals is zeroed and filled.
struct OverlapLayout : WorkLayout {
    size_t other;        // the second set's intervals, 2 n_other ints
    size_t b_bits;       // their coverage bitmap, coverage_words(length) words
    size_t ranks;        // the blocks' counts | their ranks, loci_lanes(length) words of 64 bits each
    size_t keys;         // the intervals' starts | ends | sorted starts | sorted ends, n_other words each
    size_t totals;       // the result: RibbitOverlapTotals ...
    size_t per_row;      // ... and (others, bases) of every row, 2 n ints
};
OverlapLayout overlap_layout(int64_t n, int64_t n_other, int64_t length);
hipError_t launch_overlap(const uint32_t *a_bits, int64_t length, const int32_t *rows, int64_t n, const int32_t *other, int64_t n_other, uint8_t *work,
                          size_t work_bytes, const OverlapLayout &at, hipStream_t stream);

// best.hip: the best non-overlapping rows of the loaded record (api_best.cpp).  rows: the n >= 1 rows on the device.  totals is
// zeroed and filled.
struct BestTotals {
    unsigned long long selected;      // rows chosen
    unsigned long long bases;         // bases they cover
    uint32_t rows, spare;             // non-empty rows
};
struct BestLayout : WorkLayout {
    size_t keys;         // the rows' keys | the keys sorted, n words of 64 bits each; the first half then holds w << 32 | p per sorted position
    size_t work;         // the row indices | the indices in sorted order | the reversed suffix minimum of s', n ints each; the first third then holds dp
    size_t flags;        // segment heads | take flags, n bytes each
    size_t totals;       // the result: BestTotals ...
    size_t selected;     // ... and the chosen rows' indices by ascending start, totals.selected of them (n ints of room)
};
BestLayout best_layout(int64_t n, int64_t length);
hipError_t launch_best(const int32_t *rows, int64_t n, int64_t length, uint8_t *work, size_t work_bytes, const BestLayout &at, hipStream_t stream);

// classes.hip: the loaded record's rows grouped by canonical motif class (api_classes.cpp).  rows: the n >= 1 rows on the device;
// offsets: n + 1 ascending offsets into pool, every motif 1 .. 1023 bytes over ACGT (the host has checked); pool: 8-byte aligned,
// with 16 readable bytes behind the last motif.  header is zeroed and filled.
struct ClassItem {
    uint64_t key;                     // 10 bits of length, then the first 27 bases of the class, 2 bits each
    uint32_t row, off;                // the row and where its class lies in the pool
};
struct ClassHeader {
    unsigned long long groups;        // classes found
    unsigned long long long_rows;     // rows whose motif has more than 32 bases
};
struct ClassesLayout : WorkLayout {
    size_t items;        // the rows' sort items | the items sorted, n ClassItem each
    size_t agg;          // the groups' aggregates, n of 24 bytes
    size_t heads;        // head flags | group ids, n words each
    size_t long_rows;    // the long rows' list, n ints
    size_t header;       // the result: ClassHeader ...
    size_t groups;       // ... header.groups RibbitMotifClass in class order (n of room) ...
    size_t strands;      // ... n strand bytes ...
    size_t classes;      // ... and the class of row i at offsets[i], as many bytes as the pool
};
ClassesLayout classes_layout(int64_t n, size_t pool_bytes);
hipError_t launch_classes(const int32_t *rows, const int32_t *offsets, const uint8_t *pool, int64_t n, int64_t length, uint8_t *work, size_t work_bytes,
                          const ClassesLayout &at, hipStream_t stream);

// compound.hip: the loaded record's rows chained into compound loci (api_compound.cpp).  rows, labels: the n >= 1 rows and their
// labels on the device.  totals is zeroed and filled.
struct CompoundTotals {
    uint32_t rows, chains;            // non-empty rows, chains
    uint32_t spare[2];
};
struct CompoundSums {                 // what the positions up to one add up to
    unsigned long long bases;
    uint32_t switches, overlaps, classes, spare;
};
struct CompoundLayout : WorkLayout {
    size_t keys;         // the rows' keys, then the (chain, label) keys | the keys sorted | the (chain, label) keys sorted, n words of 64 bits each
    size_t work;         // the row indices, then the chain ids | reach | where every chain starts, n ints each, and r behind the last
    size_t sums;         // n CompoundSums, the prefixes
    size_t flags;        // head, switch and overlap bits, n bytes
    size_t totals;       // the result: CompoundTotals ...
    size_t compounds;    // ... totals.chains RibbitCompound by ascending start (n of room) ...
    size_t members;      // ... and the non-empty rows' indices in (s', e', index) order, totals.rows of them (n ints of room)
};
CompoundLayout compound_layout(int64_t n, int64_t length);
hipError_t launch_compounds(const int32_t *rows, const int32_t *labels, int64_t n, int64_t length, int32_t gap, uint8_t *work, size_t work_bytes,
                            const CompoundLayout &at, hipStream_t stream);

// interruptions.hip: every row's CIGAR decoded into interruptions and the pure stretch (api_interruptions.cpp).  rows, offsets:
// the n >= 1 rows and their n + 1 ascending offsets into pool on the device; pool: 16-byte aligned, zero-filled from its last
// byte to the next multiple of 16 and 16 bytes further.  The ops of a pool of P bytes are at most interruptions_op_cap(P), which
// sizes everything that is per op, per run or per interruption.  launch_interruptions fills totals, the rows' records and the
// sites (with their clipped widths and where their observed bases start); the caller reads totals, refuses what it reports
// (bad_at, bad_row, observed) and, when there are observed bytes, calls launch_interruption_gather for them.
struct InterruptionTotals {
    uint32_t ops, runs, sites;        // ops, runs of ops of one kind (match / not), interruptions
    uint32_t bad_at;                  // the lowest offending byte offset of the pool (the grammar), 0xffffffff: none
    uint32_t bad_row;                 // the lowest row whose sums do not fit, 0xffffffff: none
    uint32_t spare;
    unsigned long long observed;      // observed bytes of all interruptions
};
struct InterruptionSums {             // what the ops up to one add up to
    unsigned long long match, x, ins, del;
    uint32_t runs, sites, row, spare; // run heads and interruption heads so far; the last row head's row + 1
};
struct InterruptionBest {             // a run's stretch key (length << 32 | ~start, 0: no stretch) and whether it is its row's first
    unsigned long long key;
    uint32_t head, spare;
};
struct InterruptionLayout : WorkLayout {
    size_t counts;       // the lanes' op counts, then their prefix: one word per 16 pool bytes and one more
    size_t ops;          // the ops, 64 bits each (cap)
    size_t op_row;       // a row's first op: the row + 1 (cap words)
    size_t first_op;     // the ops before every row, n + 1 words
    size_t sums;         // InterruptionSums up to every op (cap)
    size_t run_head;     // every run's first op, cap + 1 words
    size_t best;         // the runs' keys | the keys scanned, cap InterruptionBest each
    size_t width;        // the interruptions' clipped widths, cap + 1 words
    size_t source;       // where their observed bases start in the record, cap ints
    size_t offsets64;    // the widths' prefix, cap + 1 words of 64 bits
    size_t spans;        // the interruption that holds every 4096th observed byte
    size_t rows;         // the result: n RibbitRowPurity ...
    size_t sites;        // ... totals.sites RibbitInterruption (cap of room) ...
    size_t offsets32;    // ... where each one's observed bases start, and their total behind the last ...
    size_t totals;       // ... and InterruptionTotals
};
constexpr int64_t INTERRUPTION_SPAN = 4096;      // observed bytes one workgroup gathers, 16 per lane
inline size_t interruptions_op_cap(size_t pool_bytes) { return pool_bytes / 2 + 1; }
InterruptionLayout interruptions_layout(int64_t n, size_t pool_bytes);
hipError_t launch_interruptions(const int32_t *rows, const int32_t *offsets, const uint8_t *pool, int64_t n, size_t pool_bytes, int64_t length, uint8_t *work,
                                size_t work_bytes, const InterruptionLayout &at, hipStream_t stream);
hipError_t launch_interruption_gather(const uint8_t *ascii, uint8_t *work, const InterruptionLayout &at, uint32_t sites, int64_t observed, uint8_t *out,
                                      hipStream_t stream);

// nearest.hip: n >= 1 queries of the loaded record against n_targets >= 0 targets (api_nearest.cpp), both on the device.
struct NearestLayout : WorkLayout {
    size_t keys;         // the A keys, then the scan's input | the B keys, then the scanned maxima | the A keys sorted | the B keys sorted, n_targets words of 64 bits each
    size_t order;        // the targets' indices in order A | in order B, n_targets ints each
    size_t out;          // the result: one RibbitNearest per query
};
NearestLayout nearest_layout(int64_t n, int64_t n_targets);
hipError_t launch_nearest(const int32_t *queries, int64_t n, const int32_t *targets, int64_t n_targets, int64_t length, uint8_t *work, size_t work_bytes,
                          const NearestLayout &at, hipStream_t stream);

// composition.hip: base counts of the loaded record (length > 0) from its bit planes (api_composition.cpp).  A block is
// COMP_BLOCK bases, the WORDS_PER_LANE words a lane of the scan tile owns; loci_lanes(length) blocks, the lanes of loci.hip and overlap.hip, hold the positions
// 0 .. length.  sums: two BaseSums per block (the blocks' counts | C, G, T and other of the positions before the block), which belong
// to the record and are no part of the work buffer; launch_composition_prefix makes them with the scratch region of either layout.
// bits: the coverage bitmap of the n >= 1 rows as loci.hip takes it.  n_windows = ceil(length / window) >= 1.
constexpr int COMP_BLOCK_WORDS = 8;
constexpr int COMP_BLOCK = COMP_BLOCK_WORDS * 32;
struct alignas(16) BaseSums { uint32_t c, g, t, other; };
struct CompositionLayout : WorkLayout {
    size_t cover;        // rows: the blocks' covered positions | those before the block, one word per block each
    size_t out;          // the result: one RibbitRowComposition per row, or one RibbitBaseCounts per window
};
CompositionLayout composition_rows_layout(int64_t n, int64_t length);
CompositionLayout composition_windows_layout(int64_t n_windows, int64_t length);
hipError_t launch_composition_prefix(const DevicePlanes &pl, BaseSums *sums, uint8_t *work, size_t work_bytes, const CompositionLayout &at, hipStream_t stream);
hipError_t launch_composition_rows(const DevicePlanes &pl, const BaseSums *sums, const uint32_t *bits, const int32_t *rows, int64_t n, int32_t flank, uint8_t *work,
                                   size_t work_bytes, const CompositionLayout &at, hipStream_t stream);
hipError_t launch_composition_windows(const DevicePlanes &pl, const BaseSums *sums, int64_t window, int64_t n_windows, uint8_t *work, size_t work_bytes,
                                      const CompositionLayout &at, hipStream_t stream);

// primers.hip: a forward primer in the left flank and a reverse primer in the right flank of n_targets >= 1 targets of the loaded
// record (length > 0), from its bit planes (api_primers.cpp; include/ribbit_hip.h has the contract).  bits: the coverage bitmap of
// the record's rows as loci.hip takes it; targets: the (start, end) pairs on the device; prm: checked by the caller.  One wavefront
// per target and side; it has no rocPRIM call, so its scratch region is empty.
struct PrimerLayout : WorkLayout {
    size_t out;          // the result: one RibbitRowPrimers per target
};
PrimerLayout primers_layout(int64_t n_targets);
hipError_t launch_primers(const DevicePlanes &pl, const uint32_t *bits, const int32_t *targets, int64_t n_targets, const RibbitPrimerParams &prm, uint8_t *work,
                          size_t work_bytes, const PrimerLayout &at, hipStream_t stream);

// primer_pairs.hip: the two primers of n_targets >= 1 targets of the loaded record (length > 0) chosen as a pair, each checked for
// self-dimers and hairpins and the pair for cross-dimers (api_primer_pairs.cpp; include/ribbit_hip.h has the contract).  bits,
// targets, prm: as for primers.hip; pair: checked by the caller.  One wavefront per target; no rocPRIM call, so its scratch region
// is empty.
struct PrimerPairLayout : WorkLayout {
    size_t out;          // the result: one RibbitRowPrimerPair per target
};
PrimerPairLayout primer_pairs_layout(int64_t n_targets);
hipError_t launch_primer_pairs(const DevicePlanes &pl, const uint32_t *bits, const int32_t *targets, int64_t n_targets, const RibbitPrimerParams &prm,
                               const RibbitPrimerPairParams &pair, uint8_t *work, size_t work_bytes, const PrimerPairLayout &at, hipStream_t stream);

// primer_products.hip: the sites of n_oligos >= 1 oligos on either strand of the loaded record (length > 0), from its bit planes, and
// the products of n_pairs primer pairs among them (api_primer_products.cpp; include/ribbit_hip.h has the contract).  The first two
// launches are the site search, which every in-silico PCR caller takes through rbapi::search_sites (api_internal.h) and through
// nothing else; the host reads `header` between them, because the size of the lists is a count the device finds:
//   launch_product_uniques   the oligos sorted and made unique; header.uniques = U, copied up, the stream synchronised, 1 <= U <= n_oligos
//   launch_product_scan      the 2 U patterns (an oligo's bases with the seed at the window's end, its reverse complement with the
//                            seed at the window's start) sorted by seed key, one pass over the planes, every kept list sorted.
//                            lists: 2 U max_sites ints, sized by the host from U before the pass and not by what the pass finds;
//                            use_filter: look a position's key up in the hashed bitmap first (false: for measuring what it saves)
// What a caller does with the lists comes behind them: its own kernels (primer_specific.hip, amplicons.hip), or here
//   launch_pair_products     one RibbitRowProducts per pair into `out`, or
//   launch_oligo_sites       one RibbitOligoSites per oligo into `out`; header.positions = P, then
//   launch_site_gather       the kept lists one behind the other into flat (P ints)
struct ProductHeader { uint32_t uniques, positions, spare[2]; };
struct ProductPattern { uint32_t hi, lo, id, k; };      // the k bases in plane form, window base j at bit j; id = 2 unique + strand
struct ProductLayout : WorkLayout {
    size_t items;        // the oligos' sort items | the items sorted, n_oligos of 16 bytes each
    size_t heads;        // head flags | their inclusive sum, n_oligos words each
    size_t unique_of;    // the unique oligo of every oligo, n_oligos words
    size_t uniques;      // the unique oligos {bases, length}, n_oligos of 16 bytes
    size_t keys;         // the patterns' seed keys | their ids | the keys sorted | the ids sorted, 2 n_oligos words each
    size_t patterns;     // the patterns in key order, 2 n_oligos ProductPattern
    size_t counts;       // the sites of every pattern, 2 n_oligos words
    size_t filter;       // a bitmap of the seed keys' hashes in front of the bisection, product_filter_bits(n_oligos) bits
    size_t lens;         // the oligos' kept list lengths | where each list starts in the flat positions, 2 n_oligos words each
    size_t header;       // ProductHeader
    size_t out;          // the result: n_pairs RibbitRowProducts or n_oligos RibbitOligoSites
};
// 16 bits per pattern rounded up to a power of two, 2^15 .. 2^30: of a random record one position in 16 to 32 passes
inline int product_filter_log2(int64_t n_oligos) {
    int bits = 15;
    while (bits < 30 && ((int64_t)1 << bits) < 32 * n_oligos) ++bits;
    return bits;
}
ProductLayout products_layout(int64_t n_oligos, int64_t n_pairs);
hipError_t launch_product_uniques(const RibbitOligo *oligos, int64_t n_oligos, const RibbitProductParams &prm, uint8_t *work, size_t work_bytes, const ProductLayout &at,
                                  hipStream_t stream);
hipError_t launch_product_scan(const DevicePlanes &pl, int64_t n_oligos, int64_t uniques, const RibbitProductParams &prm, uint8_t *work, size_t work_bytes,
                               const ProductLayout &at, int32_t *lists, bool use_filter, hipStream_t stream);
// pairs: four ints per pair on the device, {a's oligo, b's oligo, left.start, right.start}; a's oligo -1: no pair
hipError_t launch_pair_products(const int32_t *pairs, int64_t n_pairs, const RibbitProductParams &prm, uint8_t *work, size_t work_bytes, const ProductLayout &at,
                                const int32_t *lists, hipStream_t stream);
hipError_t launch_oligo_sites(int64_t n_oligos, const RibbitProductParams &prm, uint8_t *work, size_t work_bytes, const ProductLayout &at, hipStream_t stream);
void launch_site_gather(int64_t n_oligos, const RibbitProductParams &prm, uint8_t *work, const ProductLayout &at, const int32_t *lists, int32_t *flat, hipStream_t stream);
// The room of a site search inside another call's work buffer: where the search's own work buffer starts, and its layout (offsets
// from there).  A layout function carves it for the most oligos a batch can have; the api file puts the layout of the batch's own
// oligos, which search_sites hands back, in its place before it launches what reads the search's regions.
struct SiteRoom {
    size_t offset;
    ProductLayout layout;
};
inline SiteRoom site_room(WorkCarver &w, int64_t n_oligos) {
    SiteRoom room{0, products_layout(n_oligos, 0)};
    room.offset = w.take(room.layout.bytes);
    return room;
}

// primer_specific.hip: the best primer pair of every one of n_targets >= 1 targets of the loaded record (length > 0) that
// amplifies nothing else in it (api_primer_specific.cpp; include/ribbit_hip.h has the contract).  bits, targets, prm, pair: as for
// primer_pairs.hip; product: checked by the caller.  The api file serves the targets in batches and sizes the layout by the
// largest.  A batch takes the launches in this order, and the host reads `header` between them:
//   launch_primer_shortlists   the two shortlists of every target (16 RibbitPrimer, four counts), and their primers as oligos one
//                              behind the other, the right ones as ordered; header.oligos = N
//   the site search            of those N oligos in `sites` (ProductLayout above); none when N == 0
//   launch_specific_pairs      one RibbitRowPrimerPair, RibbitRowProducts and RibbitRowSpecific per target
constexpr int SLOTS = 2 * RIBBIT_PRIMER_PAIR_SHORTLIST;      // the places of a target's two shortlists
struct SpecificHeader { uint32_t oligos, spare[3]; };
struct SpecificLayout : WorkLayout {
    size_t lists;         // the shortlists, 16 RibbitPrimer per target: the left side's 8 places, then the right side's (start -1: empty)
    size_t side_counts;   // left_candidates, right_candidates, left_passed, right_passed of every target
    size_t n_oligos;      // the shortlisted primers of every target | their inclusive sum, n_targets words each
    size_t oligos;        // those primers as RibbitOligo, a target's one behind the other, 16 n_targets at most
    size_t header;        // SpecificHeader
    size_t pairs, products, specific;   // the result, n_targets records each
    SiteRoom sites;       // for 16 n_targets oligos
};
SpecificLayout specific_layout(int64_t n_targets);
hipError_t launch_primer_shortlists(const DevicePlanes &pl, const uint32_t *bits, const int32_t *targets, int64_t n_targets, const RibbitPrimerParams &prm,
                                    const RibbitPrimerPairParams &pair, uint8_t *work, size_t work_bytes, const SpecificLayout &at, hipStream_t stream);
// site_lists: what launch_product_scan filled (not read when no target of the batch has an admissible pair)
hipError_t launch_specific_pairs(int64_t n_targets, const RibbitPrimerPairParams &pair, const RibbitProductParams &product, uint8_t *work, size_t work_bytes,
                                 const SpecificLayout &at, const int32_t *site_lists, hipStream_t stream);

// ... and the admissible pairs of n_targets >= 1 targets' uploaded shortlists judged on the loaded record (length > 0), which need
// not be the record they were made on (api_primer_genome.cpp: ribbit_hip_record_shortlist_verdicts).  lists: 16 RibbitPrimer per
// target on the device, as SpecificLayout::lists holds them, checked by the caller (the held places first, 1 .. 32 bases each).  A
// batch takes the launches in this order, and the host reads `header` between them:
//   launch_listed_oligos       the held places of every target counted, and their primers as oligos one behind the other, the right
//                              ones as ordered, without primer_shortlists_kernel; header.oligos = N
//   the site search            as above; none when N == 0
//   launch_shortlist_verdicts  one RibbitTargetVerdicts per target; home: the own product exists on this record
struct VerdictLayout : WorkLayout {
    size_t n_oligos;      // the held places of every target | their inclusive sum, n_targets words each
    size_t n_left;        // the held places of every target's left shortlist
    size_t oligos;        // the held primers as RibbitOligo, a target's one behind the other, 16 n_targets at most
    size_t header;        // SpecificHeader
    size_t verdicts;      // the result, n_targets records
    SiteRoom sites;       // for 16 n_targets oligos
};
VerdictLayout verdict_layout(int64_t n_targets);
hipError_t launch_listed_oligos(const RibbitPrimer *lists, int64_t n_targets, uint8_t *work, size_t work_bytes, const VerdictLayout &at, hipStream_t stream);
// site_lists: what launch_product_scan filled (not read when no target of the batch has an admissible pair)
hipError_t launch_shortlist_verdicts(const RibbitPrimer *lists, int64_t n_targets, bool home, const RibbitPrimerPairParams &pair, const RibbitProductParams &product,
                                     uint8_t *work, size_t work_bytes, const VerdictLayout &at, const int32_t *site_lists, hipStream_t stream);

// amplicons.hip: n_pairs >= 1 primer pairs typed on the loaded record (length > 0), which may be any record
// (api_amplicons.cpp: ribbit_hip_record_pair_amplicons; include/ribbit_hip.h has the contract).  The api file serves the pairs in
// batches and sizes the layout by the largest.  A batch takes the launches in this order:
//   the site search            of the batch's oligos, two per pair that has any, in `sites` (ProductLayout above)
//   launch_pair_amplicons      pair_amplicons_kernel, one lane per pair: the four counts, products and the first product
//                              (product_walk.h); then amplicon_tracts_kernel, one wavefront per pair with a product: the repeat
//                              tract inside it, from the bit planes
struct AmpliconLayout : WorkLayout {
    size_t rows;          // the result, n_pairs RibbitRowAmplicon
    SiteRoom sites;       // for 2 n_pairs oligos
};
AmpliconLayout amplicon_layout(int64_t n_pairs);
// pairs: four ints per pair on the device, {a's oligo, b's oligo, -1, -1}; a's oligo -1: no pair.  pool, offsets: the motifs of
// these pairs on the device, motif i at pool[offsets[i] - offsets[0] ..), 1 .. 1023 letters of ACGT each (checked by the caller).
// site_lists: what launch_product_scan filled.
hipError_t launch_pair_amplicons(const DevicePlanes &pl, const int32_t *pairs, int64_t n_pairs, const uint8_t *pool, const int32_t *offsets, int32_t record,
                                 const RibbitProductParams &prm, uint8_t *work, size_t work_bytes, const AmpliconLayout &at, const int32_t *site_lists,
                                 hipStream_t stream);

// panel.hip: n >= 1 primer pairs pooled into multiplex panels (api_panel.cpp: ribbit_hip_panel_pools; include/ribbit_hip.h has the
// contract).  No record is read.  The launches, in this order, all on one stream:
//   launch_panel_conflicts     panel_items_kernel packs every pair once (both oligos, and both reversed for the placement; the span,
//                              the group, the size range); panel_conflicts_kernel, one wavefront per 64 rows and per chunk of column
//                              words (grid.y): the matrix words by plain stores, the four degrees by vector atomic adds
//   launch_panel_order         the keys ~conflicts << 32 | index (all ones without a pair) and one rocPRIM radix sort of them
//   launch_panel_first_fit     panel_first_fit_kernel, ONE workgroup, n dependent steps; then the records and the number of pools
// PANEL_TILE columns are one LDS tile and one matrix word; panel_chunks(n) column chunks of whole words split the words evenly:
// chunk y holds the words [y words / chunks, (y + 1) words / chunks).
constexpr int PANEL_TILE = 64;
constexpr int64_t PANEL_TARGET_BLOCKS = 2048, PANEL_MIN_CHUNKS = 8;
inline int64_t panel_words(int64_t n) { return (n + PANEL_TILE - 1) / PANEL_TILE; }
inline int64_t panel_chunks(int64_t n) {
    const int64_t words = panel_words(n);
    return std::max<int64_t>(1, std::min(words, std::max(PANEL_MIN_CHUNKS, (PANEL_TARGET_BLOCKS + words - 1) / std::max<int64_t>(words, 1))));
}
struct PanelItem {
    unsigned long long l, r;          // the two oligos 5' to 3', two bits a base (R: the right primer as ordered) ...
    unsigned long long rl, rr;        // ... and their bases in reverse order, as a placement takes its partner
    int32_t kl, kr;                   // their lengths; kl == 0: no pair
    int32_t start, group;             // the span [start, end) = [left.start, right.start + right.length), the end in 64 bits; the record
    int64_t end;
    int32_t size_lo, size_hi;
};
static_assert(sizeof(PanelItem) == 64, "four words of 64 bits and eight ints");
struct PanelHeader { int32_t pools, members; };      // the pools in use; the rows that have a pair
struct PanelLayout : WorkLayout {
    size_t items;         // n PanelItem
    size_t matrix;        // n rows of panel_words(n) words of 64 bits
    size_t counts;        // conflicts, dimer, size, near of every row: 4 n ints, zeroed by the launch
    size_t keys;          // the order's keys | the keys sorted, n words of 64 bits each
    size_t pool_of;       // the pool of every row, -1 until it has one, n ints | the pools' member counts, n ints
    size_t header;        // the result: PanelHeader ...
    size_t rows;          // ... and n RibbitPanelRow
};
PanelLayout panel_layout(int64_t n);
// pairs: the n RibbitRowPrimerPair on the device; extra: 3 n ints on the device, or null
hipError_t launch_panel_conflicts(const RibbitRowPrimerPair *pairs, const int32_t *extra, int64_t n, const RibbitPanelParams &prm, uint8_t *work, size_t work_bytes,
                                  const PanelLayout &at, hipStream_t stream);
hipError_t launch_panel_order(int64_t n, uint8_t *work, size_t work_bytes, const PanelLayout &at, hipStream_t stream);
hipError_t launch_panel_first_fit(int64_t n, const RibbitPanelParams &prm, uint8_t *work, size_t work_bytes, const PanelLayout &at, hipStream_t stream);

// alleles.hip: the records of m >= 1 markers over n_samples samples (api_alleles.cpp: ribbit_hip_marker_alleles; include/ribbit_hip.h
// has the contract).  No record is read, and the work buffer holds only the result: the inputs are read where stage_down put them.
//   launch_marker_alleles      marker_alleles_kernel: a workgroup of four wavefronts per ALLELE_RUN consecutive markers, their cells
//                              transposed into LDS, one wavefront per marker
// cells: n_samples rows of `pitch` ints on the device, pitch >= m, row s holding the m markers' cells of sample s; designed and
// motif_lengths: m ints each.  alleles_keys(S): the sort's keys per marker, a power of two >= 64.
constexpr int ALLELE_RUN = 16;
inline int alleles_keys(int64_t n_samples) {
    int keys = 64;
    while (keys < n_samples) keys <<= 1;
    return keys;
}
struct AllelesLayout : WorkLayout {
    size_t rows;          // the result, m RibbitRowAlleles
};
AllelesLayout alleles_layout(int64_t m);
hipError_t launch_marker_alleles(const int32_t *cells, int64_t pitch, int64_t n_samples, int64_t m, const int32_t *designed, const int32_t *motif_lengths, uint8_t *work,
                                 size_t work_bytes, const AllelesLayout &at, hipStream_t stream);

// profiling aid: reads nwords dwords of src with one coalesced dword per lane (known byte count)
void launch_calib_stream_read(const uint32_t *src, int64_t nwords, uint32_t *sink, hipStream_t stream);

}  // namespace rb
