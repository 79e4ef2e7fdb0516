/*
 * ribbit_hip.h -- C ABI of the MI355X (gfx950) implementation of ribbit's per-sequence
 * shift-XOR tandem-repeat scan.
 *
 * The reference (SowpatiLab/ribbit @ 2024_10_08) has no plugin/FFI interface; its de-facto
 * boundary is the set of free functions processSequence() calls (fasta_utils.cpp:59-250).
 * Every entry point below names the reference interface it replaces.  All functions are
 * plain C: pointers and sizes only, no C++ or torch types.  INTEGRATION.md shows the glue a
 * ribbit maintainer would add to fasta_utils.cpp to call them.
 *
 * Conventions
 *   - every call returns 0 on success or a negative RIBBIT_E_* code; ribbit_hip_last_error()
 *     returns a human-readable message for the last failure on the calling thread;
 *   - no entry point lets a C++ exception out; out of host memory is reported as RIBBIT_E_NOMEM;
 *   - a handle is bound to one GPU and one HIP stream and is single-thread-affine;
 *   - there is NO CPU fallback: if no gfx950 device is usable every call fails loudly;
 *   - host arrays returned through `T **out` are owned by the handle and stay valid until the
 *     next call that produces the same kind of output, or ribbit_hip_close();
 *   - positions are 0-based sequence positions p (the reference stores p at bit L-1-p,
 *     fasta_utils.cpp:93; that reversal is not part of this ABI).
 */
#ifndef RIBBIT_HIP_H
#define RIBBIT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RIBBIT_ABI_VERSION 1

enum {
    RIBBIT_OK = 0,
    RIBBIT_E_ARG = -1,       /* bad argument */
    RIBBIT_E_DEVICE = -2,    /* no usable gfx950 device / HIP runtime error */
    RIBBIT_E_STATE = -3,     /* call made in the wrong order (e.g. scan before load) */
    RIBBIT_E_NOMEM = -4,     /* host or device allocation failed */
    RIBBIT_E_OVERFLOW = -5,  /* event buffer could not be grown far enough */
    RIBBIT_E_INTERNAL = -6
};

/* seed ranks, global_variables.cpp:28-34 */
enum { RIBBIT_RANK_P = 5, RIBBIT_RANK_Q = 4, RIBBIT_RANK_S = 3, RIBBIT_RANK_F = 2,
       RIBBIT_RANK_C = 1, RIBBIT_RANK_A = 0, RIBBIT_RANK_N = -1 };

/* Scan parameters: the reference's process-wide globals that the path reads
 * (global_variables.h:29-34, ribbit.cpp:191,240-243, fasta_utils.cpp:165). */
typedef struct RibbitScanParams {
    int32_t min_motif;        /* MINIMUM_MLEN, -m (default 2) */
    int32_t max_motif;        /* MAXIMUM_MLEN, -M (default 100) */
    int32_t window_length;    /* 8  (ribbit.cpp:191) -- only 8 is supported */
    int32_t subst_threshold;  /* 7  (ribbit.cpp:191) */
    int32_t anchor_threshold; /* 6  (fasta_utils.cpp:165) */
    int32_t anchor_length;    /* 3  (ribbit.cpp:191) */
} RibbitScanParams;

/* The tuple<int,int,int,int> every reference stage exchanges: (start, end, motif length, type). */
typedef struct RibbitSeed { int32_t start, end, mlen, type; } RibbitSeed;

/* One maximal run found by the perfect scan, before addSeedToSeedPositionsPerfect:
 * [start, end) is a run of X_m one-bits over non-N bases; term says what closed it. */
enum { RIBBIT_TERM_ZERO = 0, RIBBIT_TERM_N = 1, RIBBIT_TERM_EOS = 2 };
typedef struct RibbitRun { int32_t start, end, mlen, term; } RibbitRun;

/* One top-level addSeedToSeedPositions* call a reference scanner would make, in call order:
 * pos is the scan position of the call (sequence length for the end-of-sequence flush). */
typedef struct RibbitCall { int32_t pos, mlen, start, end; } RibbitCall;

typedef struct RibbitHandle RibbitHandle;

/* Fills *p with the reference defaults for -m min_motif -M max_motif. */
void ribbit_scan_params_default(RibbitScanParams *p, int32_t min_motif, int32_t max_motif);

const char *ribbit_hip_last_error(void);
int ribbit_hip_abi_version(void);

/* Number of usable gfx950 devices (0 if none; never initialises a device context). */
int ribbit_hip_device_count(void);
/* The PCI bus id of a device ("0000:c1:00.0"), e.g. to find its counters under /sys/class/drm on a host whose other GPUs belong to
 * other jobs (tools/m500_probe.py). */
int ribbit_hip_device_pci_bus_id(int device, char *out, size_t cap);

/* Open a handle on `device`.  Replaces the globals set up in main() (ribbit.cpp:237-243). */
int ribbit_hip_open(const RibbitScanParams *params, int device, RibbitHandle **out);
int ribbit_hip_close(RibbitHandle *h);

/* Use an existing HIP stream (hipStream_t passed as void*) for all work; NULL = handle's own. */
int ribbit_hip_set_stream(RibbitHandle *h, void *hip_stream);

/*
 * Load one FASTA record (ASCII bases, no newlines).  Replaces the 2-bit encode of
 * fasta_utils.cpp:78-115: H2D copy + pack kernel -> device bit planes (left, right, N).
 * Must not be called between ribbit_hip_scan_perfect_begin and _end on the same handle (RIBBIT_E_STATE).
 * The shift-XOR sweep of fasta_utils.cpp:117-122 is never materialised; each scan kernel
 * recomputes X_s words in registers.
 */
int ribbit_hip_load_record(RibbitHandle *h, const char *ascii, int64_t length);
/* Same, but the ASCII bases are already in device memory (length bytes at dev_ascii).  dev_ascii stays the caller's and
 * is READ AGAIN by later calls on this record (the refinement kernels and the fetch of the bases for alignment): it must
 * stay valid and unchanged until the next load on this handle or ribbit_hip_close(). */
int ribbit_hip_load_record_device(RibbitHandle *h, const void *dev_ascii, int64_t length);
/* Same as ribbit_hip_load_record from page-locked host memory (ribbit_hip_host_alloc) that the caller keeps valid and
 * unchanged until the next load on this handle or ribbit_hip_close(): the upload runs asynchronously at link speed on
 * the handle's upload stream (the previous record's kernels keep running), and refinement reads the bases in place --
 * no host copy of the record is made.  This is what a streaming FASTA reader hands over (ribbit.cpp:269-280 is the
 * loop it replaces: getline + string += into one pageable std::string per record). */
int ribbit_hip_load_record_pinned(RibbitHandle *h, const char *pinned_ascii, int64_t length);
/* Page-locked host memory for ribbit_hip_load_record_pinned (hipHostMalloc / hipHostFree). */
int ribbit_hip_host_alloc(size_t bytes, void **out);
int ribbit_hip_host_free(void *p);

/*
 * Device hot loop of processShiftXORsPerfect (parse_perfect_shiftxor.cpp:173-223) without the
 * addSeed merge: all maximal runs with length >= min(cutoff, 32), sorted by (mlen, start).
 */
int ribbit_hip_scan_perfect_runs(RibbitHandle *h, const RibbitRun **out, size_t *n);

/*
 * The addSeedToSeedPositionsPerfect calls processShiftXORsPerfect would make, in its call
 * order (position-major, motif-minor, end-of-sequence flush last; cutoffs of :179,:193,:216).
 */
int ribbit_hip_perfect_calls(RibbitHandle *h, const RibbitCall **out, size_t *n);

/*
 * processShiftXORsPerfect (parse_perfect_shiftxor.h:10; called at fasta_utils.cpp:132):
 * scan + addSeedToSeedPositionsPerfect -> seed_positions_perfect.
 */
int ribbit_hip_seeds_perfect(RibbitHandle *h, const RibbitSeed **out, size_t *n);

/*
 * The addSeedToSeedPositionsSubstitutions calls processShiftXORswithSubstitutions would make
 * (parse_substitute_shiftxor.cpp:430-574), in its call order: window-scan kernel (8-wide window,
 * >= 7 matches) + per-motif state machine replay.
 */
int ribbit_hip_subst_calls(RibbitHandle *h, const RibbitCall **out, size_t *n);

/*
 * processShiftXORswithSubstitutions (parse_substitute_shiftxor.h:9; called at fasta_utils.cpp:136).
 * Runs the perfect stage first if it has not run.  Returns seed_positions_substut and the perfect
 * list as this stage leaves it (entries may have been re-typed to RIBBIT_RANK_N).
 */
int ribbit_hip_seeds_substitutions(RibbitHandle *h, const RibbitSeed **perfect, size_t *n_perfect,
                                   const RibbitSeed **subst, size_t *n_subst);

/*
 * The addSeedToSeedPositionsAnchored calls processShiftXORsAnchored would make
 * (parse_anchored_shiftxor.cpp:580-723), in its call order.  Runs the anchored stage's two kernels: the planes
 * kernel -- generateAnchoredShiftXORs (parse_anchored_shiftxor.h:10, called at fasta_utils.cpp:144) and the plane
 * composition of fasta_utils.cpp:146-160, written to device memory -- and the 6-of-8 window scan of those planes,
 * then the window state machine on the device.  After this call "plane m" means the composed plane for every motif
 * length m (as in the reference, fasta_utils.cpp:159).  Motif sizes up to 990 (the planes kernel widens its per-wave
 * halo with max_motif).
 */
int ribbit_hip_anchored_calls(RibbitHandle *h, const RibbitCall **out, size_t *n);

/*
 * processShiftXORsAnchored (parse_anchored_shiftxor.h:14; called at fasta_utils.cpp:166).  Runs the
 * earlier stages first if needed.  Returns all three seed lists as the stage leaves them.
 */
int ribbit_hip_seeds_anchored(RibbitHandle *h, const RibbitSeed **perfect, size_t *n_perfect,
                              const RibbitSeed **subst, size_t *n_subst,
                              const RibbitSeed **anchored, size_t *n_anchored);

/*
 * The 3-way merge by start of fasta_utils.cpp:187-224: the seeds handed to refinement
 * (processSeedMotifWise / processSeed), in order, RANK_N entries and seeds shorter than 0.9*m dropped.
 */
int ribbit_hip_dispatch_seeds(RibbitHandle *h, const RibbitSeed **out, size_t *n);

/*
 * Refinement of ONE record on several GPUs (fasta_utils.cpp:211-242 handles the dispatched seeds one after the other, and each
 * independently of the others): a handle on another GPU that has the same record loaded takes over a SLICE of the dispatch list --
 * `seeds` = n consecutive entries of the list ribbit_hip_dispatch_seeds returned on the handle that ran the stages (they are
 * copied; they may also be a slice of this handle's own list) -- makes the composed planes on its own device (the planes kernel
 * alone: no scan, no merge) and is then ready for ribbit_hip_refine_bed, whose text is the BED rows of exactly those seeds.  The
 * slices' texts, in order, are the record's BED -- with ONE exception the caller must check: an alignment with an empty query sees
 * the previous seed's CIGAR (the reference's shared Alignment object); inside a slice that is resolved exactly, across a slice's
 * first seed it cannot be, so if ribbit_hip_refine_met_empty_query is 1 for any slice the record is refined again in one piece.
 * After this call the handle's seed lists are not available (ribbit_hip_seeds_* run the stages again from the next load on).
 * The scans of the seeds index the planes and the bases with what a seed says, so every seed of the list must satisfy
 *     0 <= start <= end <= length   and   min_motif <= mlen <= min(max_motif, length)
 * (length = the loaded record's; min_motif, max_motif = the handle's).  Every list ribbit_hip_dispatch_seeds returns does: a seed
 * is made of positions of the record and of a motif length that has a run in it (end + mlen may lie beyond the record; the scans
 * clamp that themselves).  Otherwise the call returns RIBBIT_E_ARG, ribbit_hip_last_error names the first offending index, and
 * the handle keeps the list it had.
 */
int ribbit_hip_adopt_dispatch(RibbitHandle *h, const RibbitSeed *seeds, size_t n);
/* 1 if the last ribbit_hip_refine_bed on this handle met an alignment with an empty query */
int ribbit_hip_refine_met_empty_query(const RibbitHandle *h);

/*
 * Thresholds the refinement scans read from the reference's globals: MINIMUM_LENGTH / PERFECT_UNITS
 * (global_variables.h:36-38, filled at ribbit.cpp:143-174,219-235; index = motif size, 0 = the value
 * operator[] default-inserts for a missing key), PURITY_THRESHOLD (always 0.85, -p is ignored) and
 * cones_threshold (3, ribbit.cpp:191).
 */
#define RIBBIT_TABLE 1024
typedef struct RibbitRefineParams {
    int32_t min_length[RIBBIT_TABLE];
    int32_t perfect_units[RIBBIT_TABLE];
    float purity_threshold;
    int32_t continuous_ones_threshold;
} RibbitRefineParams;
/* defaults for -m min_motif -M max_motif with no -l / --min-units / --perfect-units */
void ribbit_refine_params_default(RibbitRefineParams *p, int32_t min_motif, int32_t max_motif);

/*
 * One Smith-Waterman job as processSeedMotifWise (parse_smallmotif_seed.cpp:255-270) or the first level
 * of processSeed (parse_seed.cpp:379-404) sets it up: query = sequence.substr(query_start, query_length);
 * reference = the motif (motif_pool + motif_offset, `atomicity` characters) repeated until longer than
 * ppr_length; Align(query, ref, ppr_length, filter, &alignment, 15).
 */
typedef struct RibbitAlignJob {
    int32_t seed_index;      /* index into the dispatch list */
    int32_t seed_type, motif_length, atomicity;
    int32_t query_start, query_length, ppr_length;
    int32_t small;           /* 1: processSeedMotifWise (m <= 10); 0: processSeed */
    int32_t motif_offset;
} RibbitAlignJob;

/*
 * What the two striped passes of an alignment determine (ssw.c:843-891: score, end point, second best score outside
 * the mask window, begin point): everything of StripedSmithWaterman::Alignment except the CIGAR.
 * flag: 0 ok, 2 the reverse pass scored less than the forward pass, -1 not computed (job too large for the
 * GPU kernels: query_length > 8192 or ppr_length > 16384) -- align those with ribbit_ssw_align.
 */
typedef struct RibbitSswEnds {
    int32_t score, ref_end, query_end, score2, ref_end2, ref_begin, query_begin, flag;
} RibbitSswEnds;

/* The striped passes of n alignment jobs on the loaded record, batched on the GPU (one alignment per 16-lane DPP
 * row, the library's stripe order: results are the library's, Aligner::Align at parse_seed.cpp:404 /
 * parse_smallmotif_seed.cpp:270 with mask length mask_len).  out[j] belongs to jobs[j]. */
int ribbit_hip_ssw_passes(RibbitHandle *h, const RibbitAlignJob *jobs, size_t n, const char *motif_pool, size_t pool_len,
                          int32_t mask_len, RibbitSswEnds *out);

/* longestContinuousMatches (parse_seed.cpp:26-44; calls at parse_seed.cpp:366, parse_smallmotif_seed.cpp:234)
 * for every dispatched seed at once, on the GPU: out[i] belongs to dispatch seed i. */
int ribbit_hip_seed_longest_runs(RibbitHandle *h, const int32_t **out, size_t *n);

/* mostFrequentLongerMotif's choice (parse_seed.cpp:153-256) for every dispatched seed at once, on the GPU: out[i] = the start of
 * the window of dispatch seed i whose bases become its motif -- the first row with the highest count, 0 (of the RECORD,
 * parse_seed.cpp:169) when no row counts anything -- or -1 for a seed that never gets there (m <= 10, shorter than 0.9 m, longest
 * run below prm's threshold).  What ribbit_hip_refine_jobs / ribbit_hip_refine_bed use for those seeds; valid until the next call
 * on the handle. */
int ribbit_hip_seed_best_rows(RibbitHandle *h, const RibbitRefineParams *prm, const int32_t **out, size_t *n);

/* Host-only twin (no GPU): the same scan over seeds[0..n) of a record given by its packed planes (LSB-first words as
 * ribbit_hip_packed_plane returns them, zero-padded by max_motif/32 + 4 words past word L/32).  The composed planes
 * XA_m (fasta_utils.cpp:143-161; generateAnchoredShiftXORs, parse_anchored_shiftxor.cpp:20-56) are not needed: the slice
 * a seed covers is recomputed from the packed planes, as the host merges of the GPU path do. */
int ribbit_host_longest_runs(const RibbitScanParams *params, int64_t length, const uint32_t *hi, const uint32_t *lo,
                             const uint32_t *brk, size_t nwords, const RibbitSeed *seeds, size_t n, int32_t *out);

/*
 * The refinement scans between dispatch and alignment for every dispatched seed: seed validity,
 * possibleMotifs / calculateRepeatClass / calculateAtomicity (parse_smallmotif_seed.cpp:76-188,
 * bitseq_utils.cpp:139-221) for m <= 10, mostFrequentLongerMotif / calculateAtomicityLongMotif
 * (parse_seed.cpp:153-256, bitseq_utils.cpp:116-137) for m > 10, calculateMotif (bitseq_utils.cpp:14-38).
 * Jobs come in the order the reference would run its alignments (the recursion of processSeed on
 * flanks happens after alignment and is not part of this list).
 */
int ribbit_hip_refine_jobs(RibbitHandle *h, const RibbitRefineParams *prm, const RibbitAlignJob **jobs, size_t *n,
                           const char **motif_pool);

/* Host-only variant (no GPU): same jobs from a dispatch list and host planes (xa may be NULL: recomputed); *jobs and
 * *motif_pool are malloc'ed, release with ribbit_refine_jobs_free(). */
int ribbit_host_refine_jobs(const RibbitScanParams *params, const RibbitRefineParams *prm, int64_t length,
                            const uint32_t *hi, const uint32_t *lo, const uint32_t *brk, size_t nwords,
                            const uint32_t *xa, size_t xa_stride, const RibbitSeed *dispatch, size_t n_dispatch,
                            RibbitAlignJob **jobs, size_t *n_jobs, char **motif_pool, size_t *pool_len);
void ribbit_refine_jobs_free(RibbitAlignJob *jobs, char *motif_pool);

/*
 * The alignment step of refinement: StripedSmithWaterman::Aligner().Align(query, ref, ref_len, Filter(),
 * &alignment, mask_len) as called at parse_seed.cpp:404 and parse_smallmotif_seed.cpp:270 (default scores:
 * match 2, mismatch 2, gap open 3, gap extend 1).  Own implementation with the library's exact results
 * (scores, coordinates, CIGAR with = X I D S).  Host function, no GPU needed.  The CIGAR is written to
 * cigar[0..cap) NUL-terminated; cigar_len receives its full length (> cap-1 means truncated).
 */
typedef struct RibbitAlignment {
    int32_t sw_score, sw_score_next_best;
    int32_t ref_begin, ref_end, query_begin, query_end, ref_end_next_best;
    int32_t mismatches;
    int32_t flag;        /* Align's return value */
    int32_t cigar_len;
} RibbitAlignment;
int ribbit_ssw_align(const char *query, int32_t query_len, const char *ref, int32_t ref_len, int32_t mask_len,
                     RibbitAlignment *out, char *cigar, size_t cap);
/* Test hook, host only: the same alignment against `motif` (atom bases) repeated past ref_len, made the way refinement finishes an
 * alignment whose end points and path come from the GPU -- passes, path as run-length operations, then the finish that reads the
 * reference through the motif's period instead of a spelt-out string.  Must equal ribbit_ssw_align on that string. */
int ribbit_debug_ssw_align_periodic(const char *query, int32_t query_len, const char *motif, int32_t atom, int32_t ref_len, int32_t mask_len,
                                    RibbitAlignment *out, char *cigar, size_t cap);

/* Whole alignments of n jobs on the loaded record with as much on the GPU as it takes (striped passes: ssw_kernels.hip; the
 * banded path search of ssw.c:590-775: ssw_path.hip; the host writes the CIGAR text and aligns what the kernels leave alone):
 * out[j] and the NUL-terminated CIGAR at cigars + cigar_off[j] are Aligner::Align's for jobs[j].  on_gpu[j] (may be NULL):
 * 0 aligned on the host, 1 passes on the GPU, 2 passes and path on the GPU. */
int ribbit_hip_ssw_align_jobs(RibbitHandle *h, const RibbitAlignJob *jobs, size_t n, const char *motif_pool, size_t pool_len, int32_t mask_len,
                              RibbitAlignment *out, char *cigars, size_t cap, int64_t *cigar_off, int32_t *on_gpu);


/*
 * The rest of processSequence (fasta_utils.cpp:211-242): processSeedMotifWise (parse_smallmotif_seed.cpp:190-288)
 * / processSeed (parse_seed.cpp:318-464) for every dispatched seed -- motif discovery, alignment
 * (ribbit_ssw_align), processCIGARMotifWise / processCIGARWithPruning (process_cigar.cpp:126-336),
 * calculateMotifUnits, the recursion on flanks -- and the BED rows they print (11 tab-separated columns,
 * parse_seed.cpp:434-436).  *text points at handle-owned memory holding the rows of this record.
 */
int ribbit_hip_refine_bed(RibbitHandle *h, const RibbitRefineParams *prm, const char *sequence_id,
                          const char **text, size_t *len);


/* Host-only variant (no GPU; xa may be NULL: recomputed); *text is malloc'ed, release with ribbit_text_free(). */
int ribbit_host_refine_bed(const RibbitScanParams *params, const RibbitRefineParams *prm, const char *sequence, int64_t length,
                           const uint32_t *hi, const uint32_t *lo, const uint32_t *brk, size_t nwords,
                           const uint32_t *xa, size_t xa_stride, const RibbitSeed *dispatch, size_t n_dispatch,
                           const char *sequence_id, char **text, size_t *len);
void ribbit_text_free(char *text);

/*
 * ---- repeat-masked FASTA ----------------------------------------------------------------------------------------------
 * The mask of a record is the union of its BED rows' half-open [start, end) (columns 2 and 3), clipped to [0, L); rows with
 * start >= end add nothing.  RIBBIT_MASK_SOFT lowercases masked bytes in A-Z (c | 0x20) and leaves every other byte as it
 * is; RIBBIT_MASK_HARD writes every masked byte as 'N'.  The body is the record's bytes in lines of line_width bytes, each
 * ending in '\n' (the last one may be short; none for an empty record); line_width 0: the whole body on one line.
 */
#define RIBBIT_MASK_SOFT 0
#define RIBBIT_MASK_HARD 1
/* Masked, line-wrapped body of the loaded record (header not included); *text is handle-owned, valid until the
 * handle's next mask call, load or close.  intervals: n pairs (start, end), half-open, any order, clipped to [0, L). */
int ribbit_hip_mask_record(RibbitHandle *h, const int32_t *intervals, size_t n, int32_t mode, int32_t line_width,
                           const char **text, size_t *len);
/* Host-only twin (no GPU): same output for a host sequence; *text malloc'ed, release with ribbit_text_free(). */
int ribbit_host_mask_record(const char *sequence, int64_t length, const int32_t *intervals, size_t n, int32_t mode,
                            int32_t line_width, char **text, size_t *len);
/* (start, end) of every row of BED text as ribbit_hip_refine_bed writes it (host only); *pairs malloc'ed, 2 * *n ints,
 * release with ribbit_intervals_free().  A line that is not such a row: RIBBIT_E_ARG. */
int ribbit_bed_intervals(const char *text, size_t len, int32_t **pairs, size_t *n);
void ribbit_intervals_free(int32_t *pairs);

/*
 * ---- repeat sequences with their flanks (FASTA) ------------------------------------------------------------------------
 * One entry per (start, end) pair, in the order given, also for empty or out-of-range pairs.  With L the record's length
 * and F the flank (0 .. INT32_MAX), in 64-bit arithmetic:
 *   s' = min(max(s, 0), L)    e' = min(max(e, s'), L)    lo = max(s' - F, 0)    hi = min(e' + F, L)
 *   entry = ">" name ":" s' "-" e' " flank=" (s' - lo) "," (hi - e') "\n" bases[lo, hi) "\n"
 * Numbers are plain decimals; the body is the record's bytes as they are, on one line.  name is the record name as the
 * BED writes it (it may be empty).  No pairs: no text.
 */
/* Entries of rows [0, k) of intervals for the loaded record, k >= 1 when n >= 1: the largest k whose text fits the
 * handle's text budget (default 64 MiB), or k = 1 when the first entry alone is larger.  *text is handle-owned, valid
 * until the handle's next repeat-sequence call, load or close; *rows_done = k.  Call again with intervals + 2k, n - k. */
int ribbit_hip_repeat_sequences(RibbitHandle *h, const char *name, const int32_t *intervals, size_t n, int32_t flank,
                                const char **text, size_t *len, size_t *rows_done);
/* Host-only twin (no GPU): the whole text at once; *text malloc'ed, release with ribbit_text_free(). */
int ribbit_host_repeat_sequences(const char *name, const char *sequence, int64_t length, const int32_t *intervals,
                                 size_t n, int32_t flank, char **text, size_t *len);
/* Test hook: the text budget of ribbit_hip_repeat_sequences in bytes (0: the default). */
int ribbit_hip_debug_set_repeat_text_budget(RibbitHandle *h, size_t bytes);

/*
 * ---- merged, sorted loci and a density track -----------------------------------------------------------------------
 * The BED has one row per refined seed, in dispatch order: rows overlap and are not sorted.  With L the record's length,
 * every row (s, e) is clipped as the mask clips it, s' = max(s, 0), e' = min(e, L); a row with s' >= e' is empty: it
 * belongs to no locus and counts nowhere.  A position is covered when a non-empty row holds it; a run is a maximal
 * stretch of covered positions (rows that overlap or abut form one run).
 *   Loci:    consecutive runs are one locus while next.start - previous.end <= gap (gap 0: a locus is a run; this is
 *            `bedtools merge -d gap` of the sorted rows).  Loci come by ascending start.  Every non-empty row lies in
 *            exactly one locus.
 *   Density: window k = [k W, min((k + 1) W, L)) for k = 0 .. ceil(L / W) - 1; its value is the number of covered
 *            positions in it (a count of bases, not a fraction).  L = 0: no windows.
 */
typedef struct {
    int32_t start, end;    /* half-open */
    int32_t rows;          /* non-empty rows inside the locus */
    int32_t covered;       /* covered positions inside it (end - start when gap is 0) */
    int32_t best_row;      /* index into the rows given of the row with the largest e' - s'; among equals the lowest */
} RibbitLocus;
/* Loci of the loaded record under n rows (at most INT32_MAX), on the GPU.  *loci is handle-owned page-locked memory, valid
 * until the handle's next loci call, load or close.  L = 0 or no non-empty row: *n_loci = 0. */
int ribbit_hip_record_loci(RibbitHandle *h, const int32_t *intervals, size_t n, int32_t gap, const RibbitLocus **loci,
                           size_t *n_loci);
/* Covered bases per window of the loaded record, on the GPU; *covered is handle-owned page-locked memory, valid until the
 * handle's next density call, load or close.  When one record gets its mask, loci and density from the same rows, the
 * coverage bitmap behind all three is built once. */
int ribbit_hip_record_density(RibbitHandle *h, const int32_t *intervals, size_t n, int32_t window, const int32_t **covered,
                              size_t *n_windows);
/* Host-only twins (no GPU) for a record of `length` bases (0 <= length < 2^31): *loci malloc'ed, release with
 * ribbit_loci_free(); *covered malloc'ed, release with ribbit_intervals_free(). */
int ribbit_host_record_loci(int64_t length, const int32_t *intervals, size_t n, int32_t gap, RibbitLocus **loci, size_t *n_loci);
int ribbit_host_record_density(int64_t length, const int32_t *intervals, size_t n, int32_t window, int32_t **covered,
                               size_t *n_windows);
void ribbit_loci_free(RibbitLocus *loci);
/* The loci of one record as text (host only), one line per locus, 15 tab-separated columns:
 *   name, start, end, rows, covered, then the last ten columns of row best_row of bed_text, byte for byte (its start, end,
 *   motif, `atomicity | m`, length, units, purity, strand, seed type, CIGAR).
 * bed_text: the record's BED rows as ribbit_hip_refine_bed writes them, row i on line i (the rows the loci were made from);
 * a row's columns are found from the right, so a name with a tab in it works.  A best_row that is no line of bed_text, or
 * a line that is not a row: RIBBIT_E_ARG.  *text malloc'ed, release with ribbit_text_free(). */
int ribbit_bed_loci_text(const char *name, const char *bed_text, size_t bed_len, const RibbitLocus *loci, size_t n_loci,
                         char **text, size_t *len);

/*
 * ---- the rows against a second set of intervals -------------------------------------------------------------------
 * OTHER is a second set of (start, end) intervals on the same record: a truth set, another caller's BED, an annotation.
 * With L the record's length, every interval (s, e), row or OTHER, is clipped as the mask clips it, s' = max(s, 0),
 * e' = min(e, L), in 64-bit; one with s' >= e' is empty.  U_rows and U_other are the sets of positions held by a non-empty
 * row and by a non-empty OTHER interval.
 *   Per row i:  others[i] = the number of non-empty OTHER intervals j with s'_j < e'_i and e'_j > s'_i (duplicates each
 *               count; an abutting interval does not overlap); bases[i] = |[s'_i, e'_i) & U_other|.  An empty row: 0, 0.
 *   Totals:     rows / other = the number of non-empty rows / OTHER intervals; rows_hit = the non-empty rows with
 *               bases > 0; other_hit = the non-empty OTHER intervals that hold a position of U_rows; rows_bases = |U_rows|,
 *               other_bases = |U_other|, both_bases = |U_rows & U_other|.
 * All of them are counts: recall is other_hit / other, precision rows_hit / rows, the base-level Jaccard index
 * both_bases / (rows_bases + other_bases - both_bases).
 */
typedef struct {
    int64_t rows_bases, other_bases, both_bases;
    int32_t rows, rows_hit, other, other_hit;
} RibbitOverlapTotals;
/* The loaded record's n rows against n_other intervals (each at most INT32_MAX), on the GPU.  *per_row: (others, bases) of
 * row i at [2 i] and [2 i + 1], 2 n ints of handle-owned page-locked memory, valid until the handle's next overlap call,
 * load or close.  L = 0, n = 0 and n_other = 0 are no errors.  The coverage bitmap of the rows is the one the mask, the
 * loci and the density use: it is built once for all of them.  A second call with the same rows and the same OTHER on the
 * same loaded record returns what the first one found and gives the GPU nothing to do. */
int ribbit_hip_record_overlap(RibbitHandle *h, const int32_t *rows, size_t n, const int32_t *other, size_t n_other,
                              const int32_t **per_row, RibbitOverlapTotals *totals);
/* Host-only twin (no GPU) for a record of `length` bases (0 <= length < 2^31): *per_row malloc'ed, release with
 * ribbit_intervals_free(). */
int ribbit_host_record_overlap(int64_t length, const int32_t *rows, size_t n, const int32_t *other, size_t n_other,
                               int32_t **per_row, RibbitOverlapTotals *totals);
/* The record's BED rows with the two per-row values appended (host only): line i of bed_text, byte for byte, then a tab,
 * others[i], a tab, bases[i] and a newline: 13 columns.  bed_text: the rows as ribbit_hip_refine_bed writes them, row i on
 * line i (a last line without its newline counts); per_row: 2 n ints as above.  A bed_text that does not have n lines:
 * RIBBIT_E_ARG.  *text malloc'ed, release with ribbit_text_free(). */
int ribbit_bed_overlap_text(const char *bed_text, size_t bed_len, const int32_t *per_row, size_t n, char **text, size_t *len);

/*
 * ---- the best non-overlapping rows --------------------------------------------------------------------------------
 * A non-redundant call set: a subset of the record's own rows in which no two overlap, chosen so that it covers as many
 * bases as any such subset can, by ascending position.  With L the record's length:
 *   Clipping:    every row i = (s, e) is clipped as the mask clips it, s' = max(s, 0), e' = min(e, L), in 64-bit; a row
 *                with s' >= e' is empty and is never selected.
 *   Order:       the non-empty rows ordered by (e', s', i) ascending, at positions k = 1 .. r; w_k = e'_k - s'_k.
 *   Predecessor: p(k) = the number of ordered rows with e' <= s'_k (all of them come before k; an abutting row counts:
 *                abutting rows do not overlap).
 *   Forward:     dp[0] = 0, dp[k] = max(dp[k - 1], w_k + dp[p(k)]).
 *   Backward:    k = r; while k > 0: if w_k + dp[p(k)] > dp[k - 1] (strictly), row k is selected and k = p(k);
 *                otherwise k = k - 1.
 *   Result:      the indices (into the rows given) of the selected rows by ascending s', which is also ascending e';
 *                bases = dp[r], the bases the selection covers.
 * No other set of pairwise non-overlapping rows covers more bases; the rule fixes one optimal set exactly (among
 * identical rows the lowest index is the one selected); dp never exceeds L < 2^31.
 */
/* The selection for the loaded record's n rows (at most INT32_MAX), on the GPU.  *rows: *n_best indices of handle-owned
 * page-locked memory, valid until the handle's next best call, load or close.  L = 0, n = 0 and rows that are all empty
 * are no errors: *n_best = 0, *bases = 0. */
int ribbit_hip_record_best(RibbitHandle *h, const int32_t *intervals, size_t n, const int32_t **rows, size_t *n_best,
                           int64_t *bases);
/* Host-only twin (no GPU) for a record of `length` bases (0 <= length < 2^31): one sort, one forward and one backward
 * sweep.  *rows malloc'ed, release with ribbit_intervals_free(). */
int ribbit_host_record_best(int64_t length, const int32_t *intervals, size_t n, int32_t **rows, size_t *n_best, int64_t *bases);
/* Lines rows[0], rows[1], ... of bed_text (host only), byte for byte, each with its newline: the record's BED rows as
 * ribbit_hip_refine_bed writes them, row i on line i (a last line without its newline counts, and is written with one, as ribbit_bed_overlap_text writes it).
 * An index that is no line of bed_text: RIBBIT_E_ARG.  *text malloc'ed, release with ribbit_text_free(). */
int ribbit_bed_rows_text(const char *bed_text, size_t bed_len, const int32_t *rows, size_t n_rows, char **text, size_t *len);

/*
 * ---- the rows by canonical motif class ----------------------------------------------------------------------------
 * A census of what repeats: CA, AC, TG and GT are one class, and so are GATA, ATAG, TATC and their other rotations.
 *   Motif of a row:  column 4 of the BED row, found from the right (the eighth column from the end, as ribbit_bed_loci_text
 *                    finds columns: a name with a tab in it works).  A non-empty string over A, C, G, T of at most 1023
 *                    bytes (refinement writes nothing else, and -M ends at 990); anything else is RIBBIT_E_ARG.
 *   Class of a motif u of length k: of the 2k strings that are the k cyclic rotations of u and the k cyclic rotations of
 *                    its reverse complement (A<->T, C<->G, reversed) the least in byte order A < C < G < T.  It has length
 *                    k: there is no reduction to a primitive root (ACAC stays a 4-mer class; column 5 tells its atomicity).
 *   Strand:          '+' if the class is a rotation of u itself, '-' otherwise.  A motif whose reverse complement is one of
 *                    its own rotations (AT, ACGT) is '+'.
 *   Order of classes: ascending by length, then by byte order.
 *   Group of a class, within one record of length L: with s' = max(s, 0), e' = min(e, L) (the mask's clipping, in 64-bit)
 *                    and a row's width max(0, e' - s'):
 *                    rows        = the number of the record's rows whose motif has that class; every row counts, an empty
 *                                  one too;
 *                    bases       = the sum of those rows' widths, int64.  NOT a union: rows of one class overlap;
 *                    longest_row = the index of the row of the largest width, among equals the lowest index (empty rows
 *                                  have width 0 and tie with each other);
 *                    first_row   = the lowest row index of the group; the class's text is read from that row.
 * For motifs of at most 10 bases on the '+' strand alone, the least rotation is what the reference's calculateRepeatClass
 * returns (its 2-bit codes order as the letters do).
 */
typedef struct { int64_t bases; int32_t length, rows, first_row, longest_row; } RibbitMotifClass;
/* The motifs of a BED text (host only), concatenated: motif i is pool[offsets[i] .. offsets[i + 1]); offsets has n + 1
 * entries.  A line that is not a row, or a motif that is not as above: RIBBIT_E_ARG.  *pool malloc'ed, release with
 * ribbit_text_free(); *offsets malloc'ed, release with ribbit_intervals_free(). */
int ribbit_bed_motifs(const char *bed_text, size_t bed_len, char **pool, int32_t **offsets, size_t *n);
/* The classes of the loaded record's n rows (at most INT32_MAX), on the GPU.  intervals: (start, end) per row; motifs and
 * offsets as ribbit_bed_motifs hands them out (offsets[0] = 0, a pool below 2^31 bytes).  *classes: the class of row i at offsets[i], as
 * long as its motif; *strands: one byte per row, '+' or '-'; *groups: *n_groups groups in class order.  All three are
 * handle-owned page-locked memory, valid until the handle's next classes call, load or close.  n == 0: no groups.  L == 0
 * is no error: every row is a row of 0 bases.  Offsets that do not ascend, an empty motif or one of more than 1023 bytes,
 * a byte outside ACGT, a pool of 2^31 bytes or more, n > INT32_MAX: RIBBIT_E_ARG.  Before a load: RIBBIT_E_STATE. */
int ribbit_hip_record_classes(RibbitHandle *h, const int32_t *intervals, size_t n, const char *motifs, const int32_t *offsets,
                              const char **classes, const char **strands, const RibbitMotifClass **groups, size_t *n_groups);
/* Host-only twin (no GPU) for a record of `length` bases (0 <= length < 2^31): a least rotation per row, one sort of the
 * rows by (length, class, index), one sweep.  *classes and *strands malloc'ed, release with ribbit_text_free(); *groups
 * malloc'ed, release with ribbit_motif_classes_free(). */
int ribbit_host_record_classes(int64_t length, const int32_t *intervals, size_t n, const char *motifs, const int32_t *offsets,
                               char **classes, char **strands, RibbitMotifClass **groups, size_t *n_groups);
void ribbit_motif_classes_free(RibbitMotifClass *groups);
/* The record's BED rows with class and strand appended (host only): line i of bed_text, byte for byte, then a tab, the
 * class of row i, a tab, its strand and a newline: 13 columns.  bed_text: the rows as ribbit_hip_refine_bed writes them,
 * row i on line i (a last line without its newline counts, and is written with one, as ribbit_bed_overlap_text writes it).
 * A bed_text that does not have n lines, offsets that do not ascend: RIBBIT_E_ARG.  *text malloc'ed, release with
 * ribbit_text_free(). */
int ribbit_bed_class_text(const char *bed_text, size_t bed_len, const char *classes, const int32_t *offsets, const char *strands,
                          size_t n, char **text, size_t *len);
/* One line per group of one record (host only), in class order, seven tab-separated columns: name, class, length, rows,
 * bases, then start and end of longest_row as the BED has them, which are taken from `intervals` (the n rows the groups were
 * made from, unclipped: what ribbit_bed_intervals reads from the record's BED text).  The class's text is read at
 * offsets[first_row].  A first_row or longest_row that is no row, a length that is not the row's: RIBBIT_E_ARG.  *text
 * malloc'ed, release with ribbit_text_free(). */
int ribbit_class_summary_text(const char *name, const int32_t *intervals, size_t n, const char *classes, const int32_t *offsets,
                              const RibbitMotifClass *groups, size_t n_groups, char **text, size_t *len);

/*
 * ---- the rows chained into compound loci --------------------------------------------------------------------------
 * What a locus is made of: one pure stretch (CA)20, the same motif broken by a few bases (CA)12n3(CA)9, or different motifs
 * side by side (CA)12(GA)8 -- the perfect, interrupted and compound repeats of MISA and Krait.  With L the record's length,
 * every row i = (s, e) carries a caller-given int32 label; any value is a label, INT32_MIN and INT32_MAX included (what
 * ribbit_class_labels makes of the rows' motif classes is one choice).
 *   Clipping:  as everywhere, s' = max(s, 0), e' = min(e, L), in 64-bit; a row with s' >= e' is empty: it is in no chain and
 *              counts nowhere.
 *   Order:     the non-empty rows by (s', e', i) ascending, at positions k = 1 .. r.
 *   Reach:     reach_k = max(e'_1 .. e'_k).
 *   Chains:    row 1 starts a chain; row k > 1 starts a new chain iff s'_k - reach_{k-1} > gap, computed in 64-bit, and
 *              otherwise continues the chain of row k - 1.  Chains come by ascending start.  At the same gap, the start, end
 *              and rows of the chains equal those of the loci of ribbit_hip_record_loci.
 *   Per chain: start    = s' of its first member;
 *              end      = reach of its last member;
 *              rows     = the number of members;
 *              bases    = the sum of the members' widths e' - s', int64.  NOT a union;
 *              classes  = the number of distinct labels among the members;
 *              switches = the number of members, not the first, whose label differs from the previous member's;
 *              overlaps = the number of members, not the first, with s'_k < reach_{k-1}: 0 whenever no two of the rows given
 *                         overlap, and then bases equals the locus's covered;
 *              first    = the position of its first member in members.
 *   members:   the r row indices (into the rows given) in the order above; chain c owns members[first .. first + rows).
 *   Kind:      derived by ribbit_compound_text, not stored: p (perfect) when rows == 1, i (interrupted) when rows > 1 and
 *              classes == 1, c (compound) when classes > 1; a * is appended when overlaps > 0.
 * pad is always 0: it keeps sizeof at 40 without hidden tail padding.
 */
typedef struct { int64_t bases; int32_t start, end, rows, classes, switches, overlaps, first, pad; } RibbitCompound;
/* The chains of the loaded record's n rows (at most INT32_MAX) with their labels (n ints), on the GPU.  *compounds:
 * *n_compounds chains; *members: *n_members row indices.  Both are handle-owned page-locked memory, valid until the handle's
 * next compounds call, load or close.  L = 0, n = 0 and rows that are all empty are no errors: no chains, no members.
 * gap < 0, n > INT32_MAX: RIBBIT_E_ARG.  Before a load: RIBBIT_E_STATE. */
int ribbit_hip_record_compounds(RibbitHandle *h, const int32_t *intervals, const int32_t *labels, size_t n, int32_t gap,
                                const RibbitCompound **compounds, size_t *n_compounds, const int32_t **members, size_t *n_members);
/* Host-only twin (no GPU) for a record of `length` bases (0 <= length < 2^31): one sort, one sweep.  *compounds malloc'ed,
 * release with ribbit_compounds_free(); *members malloc'ed, release with ribbit_intervals_free(). */
int ribbit_host_record_compounds(int64_t length, const int32_t *intervals, const int32_t *labels, size_t n, int32_t gap,
                                 RibbitCompound **compounds, size_t *n_compounds, int32_t **members, size_t *n_members);
void ribbit_compounds_free(RibbitCompound *compounds);
/* The rows' motif classes as labels (host only): labels[i] = the index, in class order, of the group whose class is row i's.
 * classes, offsets, groups: what ribbit_hip_record_classes and its host twin hand out for the n rows.  A group whose
 * first_row is no row or whose length is not that row's, a row whose class is no group: RIBBIT_E_ARG.  *labels malloc'ed,
 * release with ribbit_intervals_free(). */
int ribbit_class_labels(const char *classes, const int32_t *offsets, size_t n, const RibbitMotifClass *groups, size_t n_groups,
                        int32_t **labels);
/* The chains of one record as text (host only), one line per chain, eight tab-separated columns:
 *   name, start, end, kind, rows, classes, bases, structure.
 * The structure is built from the chain's members in order: each is written "(MOTIF)UNITS", MOTIF and UNITS being the
 * eighth and the fifth column from the end of the member's line of bed_text, byte for byte (columns are found from the
 * right, as ribbit_bed_loci_text finds them); between two consecutive members, with d = s'_k - reach_{k-1} (the clipping of
 * `length` applied to `intervals`, the n rows the chains were made from): d > 0 writes "n" and d, as in (CA)12n5(GA)8;
 * d == 0 writes nothing; d < 0 writes "o" and -d.  bed_text: row i on line i.  A member that is no row or no line of
 * bed_text or is empty, a first / rows outside members, a line that is not a row: RIBBIT_E_ARG.  *text malloc'ed, release
 * with ribbit_text_free(). */
int ribbit_compound_text(const char *name, const char *bed_text, size_t bed_len, int64_t length, const int32_t *intervals,
                         size_t n, const RibbitCompound *compounds, size_t n_compounds, const int32_t *members,
                         size_t n_members, char **text, size_t *len);

/*
 * ---- every row's CIGAR decoded: interruptions and the pure stretch ----------------------------------------------------
 * Where the imperfections of an imperfect repeat are (the CAA inside a CAG tract), and how long its longest uninterrupted
 * stretch is.  Per row i: (s, e) from columns 2 and 3, k >= 1 the length of the column-4 motif, and the row's CIGAR, column 11,
 * which may be empty.  With L the record's length:
 *   Grammar:      a CIGAR is a sequence of ops; an op is one to ten decimal digits with a value in 1 .. 2^31 - 1 followed by one
 *                 byte of = M X I D (M is a match, as in the reference).  Anything else is RIBBIT_E_ARG, and the error text
 *                 names the byte's offset in the CIGARs given: the offending byte itself; the op letter when its digits are
 *                 missing, more than ten or out of range; the row's end when digits are its last bytes.  An empty CIGAR has
 *                 no ops and is valid.  A row whose op lengths (D included) sum to more than INT32_MAX, or for which
 *                 s + query does not fit int32: RIBBIT_E_ARG.  The first offending row decides, its grammar before its sums.
 *   Offsets:      q_0 = 0; q_{j+1} = q_j + len_j when op_j is not D, otherwise q_j.  query = q after the last op.  The row
 *                 is CONSISTENT iff s + query == e, computed in 64-bit.
 *   Stretch:      a maximal run of consecutive match ops j .. j' (3=2M is one stretch); it spans [s + q_j, s + q_{j'+1}).
 *                 pure_start, pure_end: the longest stretch, the leftmost among equals; (s, s) for a row without a match op.
 *   Interruption: a maximal run of consecutive non-match ops j .. j'.  start = s + q_j, end = s + q_{j'+1} (a run of D alone has
 *                 start == end); x, ins, del: the sums of its lengths by kind; cigar_at, cigar_len: its bytes in the CIGARs
 *                 given, from the first digit of op j through the letter of op j'.
 *   Observed:     with a = min(max(start, 0), L) and b = min(max(end, a), L), the interruption's observed bases are the
 *                 record's bytes [a, b) as loaded (case kept, N kept), concatenated in interruption order behind n_sites + 1
 *                 int32 offsets.  More than INT32_MAX observed bytes: RIBBIT_E_ARG (a pool below 2^31 bytes has fewer than
 *                 2^30 interruptions).
 *   Per row:      first = the number of interruptions of the rows before it; count, x, ins, del: the totals over the row's
 *                 interruptions; then query, pure_start, pure_end.
 *   Order:        interruptions come by row, then in CIGAR order.
 */
typedef struct { int32_t row, start, end, x, ins, del, cigar_at, cigar_len; } RibbitInterruption;   /* 32 bytes */
typedef struct { int32_t first, count, x, ins, del, query, pure_start, pure_end; } RibbitRowPurity; /* 32 bytes */
/* The CIGARs of a BED text (host only), concatenated: CIGAR i is pool[offsets[i] .. offsets[i + 1]); offsets has n + 1
 * entries.  Column 11 is the last one (columns are found from the right: a name with a tab in it works); a last line
 * without its newline counts; the CIGARs' grammar is not looked at.  A line that is not a row of 11 tab-separated columns,
 * 2^31 bytes of CIGARs or more: RIBBIT_E_ARG.  *pool malloc'ed, release with ribbit_text_free(); *offsets malloc'ed, release
 * with ribbit_intervals_free(). */
int ribbit_bed_cigars(const char *bed_text, size_t bed_len, char **pool, int32_t **offsets, size_t *n);
/* The decode for the loaded record's n rows (at most INT32_MAX), on the GPU.  intervals: (start, end) per row;
 * motif_lengths: k per row; cigars and offsets as ribbit_bed_cigars hands them out (offsets[0] = 0, ascending, a pool below
 * 2^31 bytes).  *rows: n records; *sites: *n_sites interruptions; *observed: the observed bases behind *observed_offsets
 * (*n_sites + 1 of them).  All four are handle-owned page-locked memory, valid until the handle's next interruptions call,
 * load or close.  n == 0 and L == 0 are no errors; L == 0: every observed string is empty.  Offsets that do not start at 0
 * or do not ascend, a k below 1, the grammar and the sums above: RIBBIT_E_ARG.  Before a load: RIBBIT_E_STATE. */
int ribbit_hip_record_interruptions(RibbitHandle *h, const int32_t *intervals, const int32_t *motif_lengths, size_t n,
                                    const char *cigars, const int32_t *offsets, const RibbitRowPurity **rows,
                                    const RibbitInterruption **sites, size_t *n_sites, const char **observed,
                                    const int32_t **observed_offsets);
/* Host-only twin (no GPU) for a record of `length` bases (0 <= length < 2^31) at `sequence`: a plain loop over the rows and
 * their ops.  *rows malloc'ed, release with ribbit_row_purity_free(); *sites with ribbit_interruptions_free(); *observed
 * with ribbit_text_free(); *observed_offsets with ribbit_intervals_free(). */
int ribbit_host_record_interruptions(const char *sequence, int64_t length, const int32_t *intervals, const int32_t *motif_lengths,
                                     size_t n, const char *cigars, const int32_t *offsets, RibbitRowPurity **rows,
                                     RibbitInterruption **sites, size_t *n_sites, char **observed, int32_t **observed_offsets);
void ribbit_row_purity_free(RibbitRowPurity *rows);
void ribbit_interruptions_free(RibbitInterruption *sites);
/* One line per interruption of every CONSISTENT row of one record (host only), in order, nine tab-separated columns:
 *   name, start, end, the interruption's ops byte for byte from the CIGAR (1X, 2I1X), the observed bases or "." when there
 *   are none, the row's start and end as the BED has them (from `intervals`), the row's motif byte for byte, and
 *   unit = (start - s) / k, the 0-based repeat unit the site falls in, k being the motif's length.
 * bed_text: row i on line i, the motif its eighth column from the end; cigars: the pool the sites' cigar_at point into,
 * NUL-terminated as ribbit_bed_cigars hands it out.  The interruptions of inconsistent rows are left out;
 * *rows_left_out = the number of inconsistent rows.  A bed_text that does not have n lines or has a line that is not a
 * row, a first / count outside sites, a site whose row is not the row that owns it, a cigar_at / cigar_len outside the
 * pool, observed_offsets that do not start at 0 or do not ascend: RIBBIT_E_ARG.  *text malloc'ed, release with
 * ribbit_text_free(). */
int ribbit_interruption_text(const char *name, const char *bed_text, size_t bed_len, const int32_t *intervals, size_t n,
                             const RibbitRowPurity *rows, const RibbitInterruption *sites, size_t n_sites, const char *cigars,
                             const char *observed, const int32_t *observed_offsets, char **text, size_t *len,
                             size_t *rows_left_out);
/* The record's BED rows with the decode appended (host only): line i of bed_text, byte for byte, then seven more columns, 18
 * in all: count, x, ins, del, pure_start, pure_end and pure_units = (pure_end - pure_start) / k; for an inconsistent row
 * the last three are ".".  bed_text: row i on line i (a last line without its newline counts, and is written with one).  A
 * bed_text that does not have n lines, a k below 1: RIBBIT_E_ARG.  *text malloc'ed, release with ribbit_text_free(). */
int ribbit_bed_purity_text(const char *bed_text, size_t bed_len, const int32_t *intervals, const int32_t *motif_lengths,
                           const RibbitRowPurity *rows, size_t n, char **text, size_t *len);

/*
 * ---- the nearest feature of a second set of intervals ---------------------------------------------------------------
 * Which interval of a second set a row lies in or touches, and which ones are its neighbours to either side: what bedtools
 * closest answers.  The contract is symmetric in QUERIES and TARGETS, two sets of (start, end) intervals on one record: the
 * command-line tool asks with the rows as queries and the other file's intervals as targets, and the other way round.
 * With L the record's length, every interval (s, e), query or target, is clipped as the mask clips it, s' = max(s, 0),
 * e' = min(e, L), in 64-bit; one with s' >= e' is empty.  Empty targets are never named.  j is a target's index as given.
 *   Order A:  the non-empty targets by (s', e', j) ascending.      Order B:  by (e', s', j) ascending.
 * For a non-empty query, (s, e) being its clipped ends:
 *   inside:  C = { j : s'_j <= s and e'_j >= e }.  If C is not empty, kind = RIBBIT_NEAREST_INSIDE and hit is the member of C
 *            with the greatest e', among those the first in order A: the container that reaches furthest; among equals
 *            the one that starts first; then the lowest j.
 *   over:    otherwise O = { j : s'_j < e and e'_j > s } (an abutting interval does not overlap, as in the overlap above).
 *            If O is not empty, kind = RIBBIT_NEAREST_OVER and hit is the first member of O in order A.
 *   apart:   otherwise kind = RIBBIT_NEAREST_APART and hit = -1.
 *   left:    the last in order B of { j : e'_j <= s }, left_dist = s - e'_j (0 when it abuts); none: -1, -1.
 *   right:   the first in order A of { j : s'_j >= e }, right_dist = s'_j - e; none: -1, -1.
 * left and right are reported whatever kind is: a row inside a gene still names its neighbours.
 * An empty query: kind = 0 and -1 in the five other fields.
 */
typedef struct { int32_t kind, hit, left, left_dist, right, right_dist; } RibbitNearest;   /* 24 bytes */
#define RIBBIT_NEAREST_APART 0
#define RIBBIT_NEAREST_OVER 1
#define RIBBIT_NEAREST_INSIDE 2
/* The loaded record's n queries against n_targets targets (each at most INT32_MAX), on the GPU.  *out: n records of
 * handle-owned page-locked memory, valid until the handle's next nearest call, load or close.  L = 0, n = 0 and
 * n_targets = 0 are no errors.  Before a load: RIBBIT_E_STATE. */
int ribbit_hip_record_nearest(RibbitHandle *h, const int32_t *queries, size_t n, const int32_t *targets, size_t n_targets,
                              const RibbitNearest **out);
/* Host-only twin (no GPU) for a record of `length` bases (0 <= length < 2^31): two sorts and the same searches.  *out
 * malloc'ed, release with ribbit_nearest_free(). */
int ribbit_host_record_nearest(int64_t length, const int32_t *queries, size_t n, const int32_t *targets, size_t n_targets,
                               RibbitNearest **out);
void ribbit_nearest_free(RibbitNearest *nearest);
/* The record's BED rows with what is nearest to each appended (host only): line i of bed_text, byte for byte, then eight
 * more columns, 19 in all:
 *   "in", "over" or "."; the hit's label, start and end; the left neighbour's label and left_dist; the right neighbour's
 *   label and right_dist.
 * targets: the n_targets (start, end) pairs the rows were set against, written as given, unclipped; the label of target j is
 * labels[label_offsets[j] .. label_offsets[j + 1]), labels NUL-terminated, n_targets + 1 offsets.  A field with nothing to
 * say (no hit, no neighbour) is ".".  bed_text: row i on line i (a last line without its newline counts, and is written
 * with one).  A bed_text that does not have n lines, a hit, left or right outside [-1, n_targets), a kind outside 0 .. 2,
 * label offsets that are negative, do not ascend or leave the pool: RIBBIT_E_ARG.  *text malloc'ed, release with
 * ribbit_text_free(). */
int ribbit_bed_nearest_text(const char *bed_text, size_t bed_len, const RibbitNearest *nearest, size_t n, const int32_t *targets,
                            const char *labels, const int32_t *label_offsets, size_t n_targets, char **text, size_t *len);
/* The other direction (host only): one line per interval of the second set, in the order given, 12 columns:
 *   name; the interval's start, end and label as given; then the eight columns above with the record's rows as the targets:
 *   a row's label is its motif, motifs[motif_offsets[i] .. motif_offsets[i + 1]) as ribbit_bed_motifs hands them out, its
 *   start and end are rows[2 i] and rows[2 i + 1].
 * nearest: n_targets records, interval j as the query against the n_rows rows.  The refusals are those above, with the
 * rows in the targets' place.  *text malloc'ed, release with ribbit_text_free(). */
int ribbit_nearest_other_text(const char *name, const int32_t *targets, const char *labels, const int32_t *label_offsets,
                              size_t n_targets, const RibbitNearest *nearest, const int32_t *rows, const char *motifs,
                              const int32_t *motif_offsets, size_t n_rows, char **text, size_t *len);

/*
 * ---- base composition of the rows, their flanks and the windows ------------------------------------------------------
 * What the bases are: A/C/G/T beside every repeat, as TRF prints them; for primer design the GC content of either flank,
 * whether it holds an N and whether it runs into another repeat; and the composition per window beside the density track.
 * A byte b of the record is of one of five kinds, by the rule the record is packed with: A, C, G or T if b | 0x20 is 'a',
 * 'c', 'g' or 't', and `other` for everything else (N, the IUPAC letters, any other byte).  Upper and lower case count alike.
 *   Per row:    for a row (s, e) and a flank F (0 .. INT32_MAX), the arithmetic of the repeat sequences above, in 64-bit:
 *                 s' = min(max(s, 0), L)    e' = min(max(e, s'), L)    lo = max(s' - F, 0)    hi = min(e' + F, L)
 *               One record per row, in the order given, also for empty and out-of-range rows.  A position is covered when a
 *               non-empty row of the same call holds it, rows clipped as the mask clips them: left_covered > 0 means the left
 *               flank runs into another repeat (or into a row that overlaps this one).
 *   Per window: the windows of the density track, window k = [k W, min((k + 1) W, L)) for k = 0 .. ceil(L / W) - 1, W in
 *               1 .. INT32_MAX.  L = 0: no windows.
 * Every value is a count of bases.  GC fraction, skew and entropy are one formula away and left to the reader, so that the
 * GPU, the host twin and this statement can be compared exactly.  Lower-case (soft-masked) input is not counted apart.
 */
typedef struct {
    int32_t a, c, g, t, other;                              /* of [s', e'): they sum to e' - s' */
    int32_t left,  left_gc,  left_other,  left_covered;     /* of [lo, s'): its length, its C + G, its `other`, its covered positions */
    int32_t right, right_gc, right_other, right_covered;    /* of [e', hi) likewise */
} RibbitRowComposition;                                     /* 52 bytes */
typedef struct { int32_t a, c, g, t, other; } RibbitBaseCounts;   /* 20 bytes; they sum to the window's length */
/* The loaded record's n rows (at most INT32_MAX) with `flank` bases on either side, on the GPU, from the bit planes the scans
 * read: *rows is n records of handle-owned page-locked memory, valid until the handle's next composition call, load or
 * close.  n = 0 and L = 0 are no errors; flank < 0: RIBBIT_E_ARG; before a load: RIBBIT_E_STATE.  The coverage bitmap of
 * the rows is the one the mask, the loci, the density and the overlap use; the record's prefix counts are built by the first
 * of these two calls after a load and kept until the next load. */
int ribbit_hip_record_composition(RibbitHandle *h, const int32_t *intervals, size_t n, int32_t flank,
                                  const RibbitRowComposition **rows);
/* The loaded record's base counts per window, on the GPU; *windows is handle-owned page-locked memory, valid until the
 * handle's next base-window call, load or close.  window < 1: RIBBIT_E_ARG; before a load: RIBBIT_E_STATE. */
int ribbit_hip_record_base_windows(RibbitHandle *h, int32_t window, const RibbitBaseCounts **windows, size_t *n_windows);
/* Host-only twins (no GPU), counting the bytes of `sequence` (0 <= length < 2^31): *rows and *windows malloc'ed, release
 * with ribbit_composition_free(). */
int ribbit_host_record_composition(const char *sequence, int64_t length, const int32_t *intervals, size_t n, int32_t flank,
                                   RibbitRowComposition **rows);
int ribbit_host_record_base_windows(const char *sequence, int64_t length, int32_t window, RibbitBaseCounts **windows,
                                    size_t *n_windows);
void ribbit_composition_free(void *rows_or_windows);
/* Test hook: how often a handle of this process has built a record's prefix counts on the GPU (once per loaded record
 * that gets either output, however many calls follow). */
int64_t ribbit_debug_composition_prefix_builds(void);
/* The record's BED rows with their composition appended (host only): line i of bed_text, byte for byte, then the 13 values
 * of rows[i] in the struct's order, each behind a tab, and a newline: 24 columns.  bed_text: row i on line i (a last line
 * without its newline counts).  A bed_text that does not have n lines: RIBBIT_E_ARG.  *text malloc'ed, release with
 * ribbit_text_free(). */
int ribbit_bed_composition_text(const char *bed_text, size_t bed_len, const RibbitRowComposition *rows, size_t n, char **text,
                                size_t *len);
/* The windows of one record as text (host only), one line per window, empty ones too, 8 tab-separated columns: name, start,
 * end, A, C, G, T, other.  With equal windows the lines pair one to one with the density track's.  length outside
 * 0 .. INT32_MAX, window < 1 or an n_windows that is not ceil(length / window): RIBBIT_E_ARG.  *text malloc'ed, release with
 * ribbit_text_free(). */
int ribbit_base_windows_text(const char *name, int64_t length, int32_t window, const RibbitBaseCounts *windows, size_t n_windows,
                             char **text, size_t *len);

/*
 * ---- PCR primers in the flanks of chosen rows --------------------------------------------------------------------------
 * For every target (s, e), usually a row of the best selection, a forward primer in the flank to its left and a reverse primer
 * in the flank to its right, each chosen on its own: the candidate oligos of either flank are all of its substrings of
 * min_length .. max_length bases, a candidate is admissible or not, and the admissible one with the least penalty is taken.
 * Everything is integer arithmetic, so that the GPU, the host twin and this statement can be compared exactly.  The pair is
 * not optimised together and nothing is checked for dimers or hairpins (the primer pairs below) or for priming elsewhere (the
 * in-silico PCR below them).
 *   Windows:    the arithmetic of the composition above, in 64-bit, with the flank F = params->flank:
 *                 s' = min(max(s, 0), L)    e' = min(max(e, s'), L)    lo = max(s' - F, 0)    hi = min(e' + F, L)
 *               A left candidate is [p, p + k) with lo <= p and p + k <= s', a right candidate [q, q + k) with e' <= q and
 *               q + k <= hi; min_length <= k <= max_length.  The left primer is the candidate's bases, the right primer their
 *               reverse complement.  All rules below are the same on either strand and are stated on the forward strand; the
 *               3' position of a left candidate is p + k - 1, that of a right candidate is q.
 *   Blocked:    a position is blocked when its byte is of kind `other` (any byte but ACGTacgt) or when a non-empty row of
 *               `intervals`, clipped as the mask clips them, holds it: all rows of the record, not only the targets.
 *   Admissible: (1) no position of the candidate is blocked; (2) with g its C and G bases, 100 g >= gc_min_percent k and
 *               100 g <= gc_max_percent k; (3) no max_run + 1 equal consecutive bases inside it; (4) if gc_clamp is set, the
 *               base at its 3' position is C or G; (5) tm_min <= Tm <= tm_max.
 *   Tm:         SantaLucia's unified nearest-neighbour parameters (1998) in fixed point, dH in 100 cal/mol and dS in
 *               0.1 cal/(K mol), per step of two adjacent bases read 5' to 3' on the forward strand:
 *                 AA TT  -79 -222    AT  -72 -204    TA  -72 -213    CA TG  -85 -227    GT AC  -84 -224
 *                 CT AG  -78 -210    GA TC  -82 -222    CG -106 -272    GC  -98 -244    GG CC  -80 -199
 *               and per terminal base (the first and the last) 23, 41 for A or T and 1, -28 for C or G.  With H and S the
 *               sums over the k - 1 steps and both terminals,
 *                 S' = S - 11 (k - 1) - 362        Tm = (10000 H) / S' - 2732      in tenths of a degree Celsius
 *               -11 per step is the salt correction at 50 mM Na+ (0.368 ln 0.05 = -1.10), -362 is R ln(50 nM / 4) = -36.2.
 *               H and S' are negative for every k >= 2, and the division truncates their positive quotient.
 *   Choice:     penalty = |Tm - tm_opt| + 10 |k - opt_length|.  Of the admissible candidates of a side, the one with the
 *               least (penalty, distance, k) in that order, the distance to the target being s' - (p + k) on the left and
 *               q - e' on the right.  No two candidates of a side share that triple.
 */
#define RIBBIT_PRIMER_MAX_FLANK 1000
#define RIBBIT_PRIMER_MAX_LENGTH 32
typedef struct {
    int32_t flank;                            /* 200;  0 .. RIBBIT_PRIMER_MAX_FLANK */
    int32_t min_length, max_length;           /* 18, 25;  2 <= min_length <= max_length <= RIBBIT_PRIMER_MAX_LENGTH */
    int32_t opt_length;                       /* 20;  min_length .. max_length */
    int32_t tm_min, tm_opt, tm_max;           /* 570, 600, 630, tenths of a degree;  0 <= tm_min <= tm_opt <= tm_max <= 2000 */
    int32_t gc_min_percent, gc_max_percent;   /* 40, 60;  0 <= gc_min_percent <= gc_max_percent <= 100 */
    int32_t max_run;                          /* 4;  1 or more */
    int32_t gc_clamp;                         /* 1;  0 or 1 */
} RibbitPrimerParams;
void ribbit_primer_params_default(RibbitPrimerParams *params);
typedef struct {
    int32_t start, length;                    /* the candidate [start, start + length) on the forward strand; start -1 and */
    int32_t tm, penalty;                      /* every other field 0 when the side has no admissible candidate */
    int32_t bases_lo, bases_hi;               /* its forward-strand bases, A 0, C 1, G 2, T 3: base j at bits 2 j of the 64 bits hi : lo */
} RibbitPrimer;
typedef struct {
    RibbitPrimer left, right;
    int32_t left_candidates, right_candidates;   /* the admissible candidates of either side */
} RibbitRowPrimers;                           /* 56 bytes */
/* The loaded record's n_targets targets (at most INT32_MAX) against the coverage of its n rows `intervals`, on the GPU, from
 * the bit planes the scans read: *rows is one record per target, in the order given, of handle-owned page-locked memory, valid
 * until the handle's next primer call, load or close.  The coverage bitmap of the rows is the one the mask, the loci, the
 * density, the overlap and the composition use.  n_targets = 0, n = 0 and L = 0 are no errors.  A parameter outside its range
 * above: RIBBIT_E_ARG, and the error text names the field; before a load: RIBBIT_E_STATE. */
int ribbit_hip_record_primers(RibbitHandle *h, const int32_t *intervals, size_t n, const int32_t *targets, size_t n_targets,
                              const RibbitPrimerParams *params, const RibbitRowPrimers **rows);
/* Host-only twin (no GPU), from the bytes of `sequence` (0 <= length < 2^31), every candidate computed on its own: *rows
 * malloc'ed, release with ribbit_primers_free(). */
int ribbit_host_record_primers(const char *sequence, int64_t length, const int32_t *intervals, size_t n, const int32_t *targets,
                               size_t n_targets, const RibbitPrimerParams *params, RibbitRowPrimers **rows);
void ribbit_primers_free(RibbitRowPrimers *rows);
/* The targets' BED rows with their primers appended (host only): line i of bed_text, byte for byte, then 11 columns, each
 * behind a tab, and a newline: 22 columns.  The 11 are: the left primer's start, end, sequence 5' to 3' and Tm (tenths as
 * d.d); the right primer's start, end, sequence 5' to 3' (the reverse complement of its forward-strand bases) and Tm; the
 * product's size, right end - left start; the admissible candidates on the left and on the right.  A side without a primer
 * (start < 0) has "." in its four columns, and the product is "." unless both sides have one.  bed_text: row i on line i (a last
 * line without its newline counts).  A bed_text that does not have n lines, a primer of fewer than 1 or more than
 * RIBBIT_PRIMER_MAX_LENGTH bases: RIBBIT_E_ARG.  *text malloc'ed, release with ribbit_text_free(). */
int ribbit_bed_primers_text(const char *bed_text, size_t bed_len, const RibbitRowPrimers *rows, size_t n, char **text, size_t *len);

/*
 * ---- PCR primer pairs, chosen together and checked for dimers and hairpins ---------------------------------------------
 * The same windows, blocked positions, five admissibility rules, Tm and penalty as above, with the same RibbitPrimerParams;
 * on top of them an ungapped model of an oligo that binds to itself or to its partner, and the choice of the two primers of a
 * target as one pair.  Everything is integer arithmetic on the oligos' letters.  Gapped or thermodynamic (dG) dimer models,
 * bounds on the product's size are not part of it; priming elsewhere in the record is the in-silico PCR below, priming in the other
 * records of the input the genome-wide choice behind it.
 *   Oligos:     an oligo is read 5' to 3'.  The left primer is its candidate's forward-strand bases, the right primer the reverse
 *               complement of its candidate's forward-strand bases (the text ribbit_bed_primers_text prints).  Bases x and y are
 *               bonded when y is the complement of x: with the codes A 0, C 1, G 2, T 3, when x ^ y == 3.
 *   Duplex:     of two oligos a (ka bases) and b (kb bases).  A placement is a constant c in 0 .. ka + kb - 2; it pairs a[i] with
 *               b[c - i] for every i for which both exist (antiparallel, ungapped).  any(a, b) is the longest run of consecutive
 *               i whose pairs are all bonded, over all placements; end(a, b) is the longest such run that contains the pair of
 *               a's 3' base (i = ka - 1) or the pair of b's 3' base (c - i = kb - 1), over all placements.  Both are symmetric
 *               in a and b.
 *   Hairpin:    of one oligo a: the placements of a with itself, restricted to the pairs (i, j = c - i) with i < j and
 *               j - i - 1 >= RIBBIT_PRIMER_HAIRPIN_LOOP; hairpin(a) is the longest run of consecutive i whose pairs are bonded,
 *               over all c.
 *   Values:     (any, end) and hairpin of a few oligos, computed from a plain statement of the above:
 *                 ACGT self (4,4)    AAAAAAAA / TTTTTTTT (8,8)    AAAAAAAA self (0,0)    GGGGCCCC self (8,8), hairpin 2
 *                 CCCCCCCCCCCCCCCCCCAT self (2,2)    CAGTCGATCGGATCCATGCA self (6,4), hairpin 3
 *                 ACGTTGCAACGTACGTAGCT self (12,4), hairpin 4; with CAGTCGATCGGATCCATGCA, either order, (4,4)
 *                 GATTACAGATTACAGGC / TTTGCCTGTAATC (10,10)    GCGCGCGCGCGCGCGCGCGC self (20,20), hairpin 8
 *                 hairpins: GGGGAAACCCC 4, GGGGAACCCC 3, GGGCTTTTGCCC 4, GGGCTTTGCCC 4, GGGCTTGCCC 3, CCCCCAAAGGGGG 5
 *   Selection:  per target.  (1) A candidate passes when it is admissible by the five rules and, as an oligo o,
 *               any(o, o) <= max_self_any, end(o, o) <= max_self_end and hairpin(o) <= max_hairpin.  (2) The shortlist of a
 *               side is its first `shortlist` passing candidates in the order (penalty, distance, k) of the choice above; rank
 *               0 is the best.  (3) A pair (l, r) of the two shortlists is admissible when |Tm_l - Tm_r| <= max_tm_difference,
 *               any(l, r) <= max_pair_any and end(l, r) <= max_pair_end.  (4) The chosen pair is the admissible one with the
 *               least (penalty_l + penalty_r + |Tm_l - Tm_r|, product, rank_l, rank_r), the product being the right
 *               candidate's end - the left candidate's start.  (5) There is no fallback to a one-sided answer.
 */
#define RIBBIT_PRIMER_HAIRPIN_LOOP 3
#define RIBBIT_PRIMER_PAIR_SHORTLIST 8
typedef struct {
    int32_t shortlist;                        /* 8;  1 .. RIBBIT_PRIMER_PAIR_SHORTLIST */
    int32_t max_self_any, max_self_end;       /* 4, 3;  0 .. 32 each: at 32 a limit never refuses, an oligo has at most 32 bases */
    int32_t max_hairpin;                      /* 3;  0 .. 32 */
    int32_t max_pair_any, max_pair_end;       /* 4, 3;  0 .. 32 */
    int32_t max_tm_difference;                /* 30, tenths of a degree;  0 .. 2000 */
} RibbitPrimerPairParams;
void ribbit_primer_pair_params_default(RibbitPrimerPairParams *params);
typedef struct {
    RibbitPrimer left, right;                 /* the chosen pair; without an admissible pair both starts are -1 and every */
    int32_t pair_penalty, tm_difference;      /* field is 0 except the six counts below.  penalty_l + penalty_r + |Tm_l - Tm_r|; |Tm_l - Tm_r| */
    int32_t product;                          /* right end - left start */
    int32_t left_rank, right_rank;            /* their places in the shortlists */
    int32_t left_self_any, left_self_end, left_hairpin;
    int32_t right_self_any, right_self_end, right_hairpin;
    int32_t pair_any, pair_end;
    int32_t left_candidates, right_candidates;   /* admissible by the five rules: ribbit_hip_record_primers' counts */
    int32_t left_passed, right_passed;        /* all passing candidates, not only the shortlisted ones */
    int32_t pairs_tried;                      /* min(shortlist, left_passed) * min(shortlist, right_passed) */
    int32_t pairs_admissible;
    int32_t reserved;                         /* 0 */
} RibbitRowPrimerPair;                        /* 32 ints, 128 bytes */
/* The loaded record's n_targets targets (at most INT32_MAX) against the coverage of its n rows `intervals`, on the GPU
 * (primer_pairs.hip): *rows is one record per target, in the order given, of handle-owned page-locked memory, valid until the
 * handle's next primer pair call, load or close.  States and refusals are those of ribbit_hip_record_primers; a field of
 * pair_params outside its range above: RIBBIT_E_ARG, and the error text names the field. */
int ribbit_hip_record_primer_pairs(RibbitHandle *h, const int32_t *intervals, size_t n, const int32_t *targets, size_t n_targets,
                                   const RibbitPrimerParams *params, const RibbitPrimerPairParams *pair_params,
                                   const RibbitRowPrimerPair **rows);
/* Host-only twin (no GPU), from the bytes of `sequence` (0 <= length < 2^31), letter by letter with loops over the placements:
 * *rows malloc'ed, release with ribbit_primer_pairs_free(). */
int ribbit_host_record_primer_pairs(const char *sequence, int64_t length, const int32_t *intervals, size_t n, const int32_t *targets,
                                    size_t n_targets, const RibbitPrimerParams *params, const RibbitPrimerPairParams *pair_params,
                                    RibbitRowPrimerPair **rows);
void ribbit_primer_pairs_free(RibbitRowPrimerPair *rows);
/* any(a, b) and end(a, b), and hairpin(a), of oligos given as text, 5' to 3' (host only): 1 .. 32 letters of ACGTacgt each,
 * anything else is RIBBIT_E_ARG.  For checking a hand-made primer against the limits above. */
int ribbit_host_oligo_duplex(const char *a, const char *b, int32_t *any, int32_t *end);
int ribbit_host_oligo_hairpin(const char *a, int32_t *hairpin);
/* The targets' BED rows with their primer pairs appended (host only): line i of bed_text, byte for byte, then 21 columns, each
 * behind a tab, and a newline: 32 columns.  Columns 1 to 9 are the eight primer columns and the product as
 * ribbit_bed_primers_text writes them; 10 is tm_difference (tenths as d.d); 11 and 12 are pair_any and pair_end; 13 to 18 the
 * left side's, then the right side's, self any, self end and hairpin; 19 to 21 left_passed, right_passed and pairs_admissible.
 * Without a pair the first 18 are ".".  bed_text and the refusals as for ribbit_bed_primers_text.  *text malloc'ed, release
 * with ribbit_text_free(). */
int ribbit_bed_primer_pairs_text(const char *bed_text, size_t bed_len, const RibbitRowPrimerPair *rows, size_t n, char **text, size_t *len);

/*
 * ---- in-silico PCR: where else in the record an oligo primes, and what a primer pair amplifies there ----------------------
 * The check Primer-BLAST, UCSC isPCR, e-PCR and MFEprimer make before a pair is ordered, for the loaded record: every place
 * on either strand where an oligo's 3' end matches exactly and the rest of it nearly, and every two such places of a pair's
 * primers that face each other within a product size.  Everything is integer arithmetic on letters.  Gapped
 * alignments and thermodynamic binding are not part of it; the other records of the input are judged by
 * ribbit_hip_record_shortlist_verdicts, below, with this contract on each.
 *   Letters:    codes A 0, C 1, G 2, T 3, case ignored; any other byte is `other`, as the record is packed (the brk plane).
 *   Oligo:      o has k bases, is read 5' to 3', 1 <= k <= 32; q = revcomp(o), q[j] = 3 - o[k - 1 - j].
 *   Sites:      with s = seed and d = max_mismatches, on the record R[0, L): o has a FORWARD SITE at x when 0 <= x and
 *               x + k <= L, no byte of R[x, x + k) is `other`, R[x + j] == o[j] for k - s <= j < k (the 3' end matches exactly)
 *               and at most d of the j < k - s have R[x + j] != o[j].  o has a REVERSE SITE at x when the same window conditions
 *               hold, R[x + j] == q[j] for j < s, and at most d of the j >= s mismatch q: the oligo's 3' base lies at x.  The
 *               rows' coverage plays no part: a site inside a repeat counts.  A palindromic oligo may have both sites at one x;
 *               both count.
 *   Products:   of a pair.  a is the left primer, its RibbitPrimer's bases as they stand; b is the right primer, the reverse
 *               complement of its RibbitPrimer's forward-strand bases (as ribbit_bed_primer_pairs_text prints it).  F is the
 *               forward sites of a and those of b, V the reverse sites of a and those of b; each site carries its own oligo's
 *               length, and a site of a and a site of b are counted separately even when a == b.  A product is a pair (f, v)
 *               of F x V with f.x + f.k <= v.x (the windows do not overlap) and size = v.x + v.k - f.x <= max_product.
 *               own is 1 when (a forward at left.start, b reverse at right.start) is one of the products, else 0;
 *               shortest_other is the least size among the other products, 0 when there is none.  When any of the four lists
 *               is longer than max_sites: products = -1, own = 0, shortest_other = 0; the four counts are always exact.
 *               A pair is specific in this record when products - own == 0.
 *   Values:     with L = GATTACAGATTACAGGCT, M = ACGTTGCATGCCATGACTGA, R = CCTGAAGTCTCGGATCAA, the pair a = L, b = revcomp(R)
 *               and the defaults, as (left_forward, left_reverse, right_forward, right_reverse, products, own, shortest_other):
 *                 L M R, own (0, 38)                      (1, 0, 0, 1,  1, 1, 0)    max_product 56: the same; 55: (1, 0, 0, 1, 0, 0, 0)
 *                 L's last base T -> A (in the seed)      (0, 0, 0, 1,  0, 0, 0)
 *                 L's first two bases GA -> CT            (1, 0, 0, 1,  1, 1, 0)    first three GAT -> CTA: (0, 0, 0, 1, 0, 0, 0)
 *                 L's first base -> N                     (0, 0, 0, 1,  0, 0, 0)
 *                 L without its first base, own (0, 37)   (0, 0, 0, 1,  0, 0, 0)    R without its last base: (1, 0, 0, 0, 0, 0, 0)
 *                 L R, own (0, 18): abutting              (1, 0, 0, 1,  1, 1, 0)
 *                 GATTACAGATTACAGGC CTGAAGTCTCGGATCAA with a = GATTACAGATTACAGGCC, own (0, 17): one base shared
 *                                                         (1, 0, 0, 1,  0, 0, 0)
 *                 L M revcomp(L) M R, own (0, 76)         (1, 1, 0, 1,  2, 1, 56): a left-left product
 *                 L M L M R, own (0, 76)                  (2, 0, 0, 1,  2, 1, 56)   max_sites 1: (2, 0, 0, 1, -1, 0, 0)
 *                 P = ACGTACGTACGTACGT, a = b = P: on P, own (0, 0)   (1, 1, 1, 1, 0, 0, 0)
 *                                                  on P P, own (0, 16) (5, 5, 5, 5, 4, 1, 32)
 */
typedef struct {
    int32_t seed;                             /* 15;  6 .. 16: the 3' bases that match exactly (isPCR's minPerfect) */
    int32_t max_mismatches;                   /* 2;  0 .. 32 outside the seed (32 never refuses) */
    int32_t max_product;                      /* 4000;  1 .. 2^31 - 1 (isPCR's maxSize) */
    int32_t max_sites;                        /* 64;  1 .. 1024: the longest list of sites that is kept */
} RibbitProductParams;
void ribbit_product_params_default(RibbitProductParams *params);
typedef struct {
    int32_t left_forward, left_reverse, right_forward, right_reverse;   /* the sites of a and of b, exact */
    int32_t products, own, shortest_other, reserved;                    /* reserved 0 */
} RibbitRowProducts;                          /* 32 bytes; eight zeros for a target without a pair (left.start < 0) */
typedef struct {
    int32_t length, bases_lo, bases_hi;       /* 5' to 3', base j at bits 2 j of the 64 bits hi : lo; bits from 2 length on are ignored */
} RibbitOligo;
typedef struct {
    int32_t forward, reverse;                 /* the sites on either strand, exact */
    int32_t forward_at, reverse_at;           /* where the list starts in *positions, ascending window starts x; -1 when the list */
} RibbitOligoSites;                           /* is longer than max_sites (it then takes no room).  16 bytes */
/* The sites of n oligos (n * max_sites at most 2^29) on the loaded record, on the GPU (primer_products.hip): equal oligos are searched once,
 * the record's bit planes are read once.  *sites is one record per oligo in the order given; *positions holds the kept lists one
 * behind the other, oligo by oligo, the forward list before the reverse list, *n_positions values in all.  Both are handle-owned
 * page-locked memory, valid until the handle's next call of either function below, load or close.  n = 0 and L = 0 are no
 * errors.  A field of params outside its range above: RIBBIT_E_ARG, and the error text names the field; an oligo of fewer than
 * `seed` or more than 32 bases: RIBBIT_E_ARG, and the text names its index; before a load: RIBBIT_E_STATE.  Counts and
 * products add up over records, so a genome is answered by loading each record in turn. */
int ribbit_hip_record_oligo_sites(RibbitHandle *h, const RibbitOligo *oligos, size_t n, const RibbitProductParams *params,
                                  const RibbitOligoSites **sites, const int32_t **positions, size_t *n_positions);
/* Host-only twin (no GPU), from the bytes of `sequence` (0 <= length < 2^31), letter by letter: *sites and *positions malloc'ed,
 * release each with ribbit_products_free(). */
int ribbit_host_record_oligo_sites(const char *sequence, int64_t length, const RibbitOligo *oligos, size_t n,
                                   const RibbitProductParams *params, RibbitOligoSites **sites, int32_t **positions, size_t *n_positions);
/* The products of n pairs (at most 2^24: ribbit_hip_record_primer_pairs' rows, or hand-made ones of which only the two primers'
 * start, length and bases are read) on the loaded record, on the GPU: *rows is one record per pair in the order given, of
 * handle-owned page-locked memory as above.  States and refusals as above; a primer of fewer than `seed` or more than 32 bases:
 * RIBBIT_E_ARG, and the text names the pair's index. */
int ribbit_hip_record_primer_products(RibbitHandle *h, const RibbitRowPrimerPair *pairs, size_t n, const RibbitProductParams *params,
                                      const RibbitRowProducts **rows);
/* Host-only twin: *rows malloc'ed, release with ribbit_products_free(). */
int ribbit_host_record_primer_products(const char *sequence, int64_t length, const RibbitRowPrimerPair *pairs, size_t n,
                                       const RibbitProductParams *params, RibbitRowProducts **rows);
void ribbit_products_free(void *from_a_host_twin);
/* The targets' BED rows with their primer pairs and products (host only): the 32 columns of ribbit_bed_primer_pairs_text, then
 * six more, 38 in all: the four counts, products - own, shortest_other.  The last two are "." when products is -1, all six
 * without a pair.  bed_text and the refusals as for ribbit_bed_primer_pairs_text.  *text malloc'ed, release with
 * ribbit_text_free(). */
int ribbit_bed_primer_products_text(const char *bed_text, size_t bed_len, const RibbitRowPrimerPair *pairs, const RibbitRowProducts *products,
                                    size_t n, char **text, size_t *len);

/*
 * ---- the best primer pair of every target that amplifies nothing else in the record ----------------------------------------
 * The two contracts above put together: where ribbit_hip_record_primer_pairs takes the best admissible pair of the two
 * shortlists and ribbit_hip_record_primer_products says what that one pair amplifies, this takes the best admissible pair that
 * is specific.  Everything is integer arithmetic on letters; nothing is added to either contract.  Only the loaded record is
 * searched; the same choice over all records of an input is the section behind this one.
 *   Shortlists: candidates, shortlists and the admissible pairs of a target are exactly steps (1) to (3) of the selection.
 *   Order:      the admissible pairs in the order of step (4)'s key, (penalty_l + penalty_r + |Tm_l - Tm_r|, product, rank_l,
 *               rank_r); no two pairs share a key.  A pair's PLACE is its 0-based position in that order.
 *   Products:   the pair (l, r) is judged by the in-silico PCR contract with a = the left candidate's oligo, b = the right
 *               candidate's oligo as ordered (the reverse complement of its forward-strand bases), and own = (a forward at the
 *               left candidate's start, b reverse at the right candidate's start).
 *   Outcomes:   every admissible pair is exactly one of OVER (products == -1: one of its four site lists is longer than
 *               max_sites), SPECIFIC (not over and products - own == 0, as defined above) and OTHER (neither).
 *   Choice:     the chosen pair is the first specific pair in that order.  There is no fallback: without a specific pair the
 *               target has no pair.
 *   Records:    per target a RibbitRowPrimerPair of the chosen pair, every field as ribbit_hip_record_primer_pairs would fill
 *               it had it chosen that pair (ranks, the five dimer values, the six counts; pairs_admissible counts all admissible
 *               pairs); without a pair both starts are -1 and every field is 0 except the six counts.  Its RibbitRowProducts
 *               (eight zeros without a pair).  And a RibbitRowSpecific, below.
 *   Values:     4,000 random bases with (CA)20 at 1500, the target (1500, 1540), no rows, the defaults
 *               (tests/primer_specific_contract.py builds the records and computes the values from a plain statement of the
 *               above), as (place, pairs_admissible, pairs_specific, pairs_over, pairs_other, first_products) and the chosen
 *               pair's (left start, left length, right start, right length):
 *                 undisturbed                                               (0, 44, 44, 0, 0, 0)     (1304, 22, 1624, 21)
 *                 that pair's two windows copied to 3000 and 60 bases behind (2, 44, 26, 0, 18, 2)    (1304, 22, 1613, 22)
 *                 both flanks of 200 bases copied to 2600 .. 3000           (-1, 44, 0, 0, 44, 2)    no pair
 *                 the left flank alone copied to 2600                       (0, 44, 44, 0, 0, 0)     (1304, 22, 1624, 21)
 *                 the same at max_sites 1                                   (-1, 44, 0, 44, 0, -1)   no pair
 */
typedef struct {
    int32_t place;                            /* of the chosen pair among the admissible pairs; -1: no pair is specific */
    int32_t pairs_admissible;                 /* = pairs_specific + pairs_over + pairs_other */
    int32_t pairs_specific, pairs_over, pairs_other;
    int32_t first_products;                   /* products - own of the pair in place 0 (what ribbit_bed_primer_products_text prints */
    int32_t reserved[2];                      /* beside it): -1 when that pair is over, 0 without an admissible pair.  reserved 0 */
} RibbitRowSpecific;                          /* 32 bytes */
/* The loaded record's n_targets targets (at most INT32_MAX) against the coverage of its n rows, on the GPU (primer_specific.hip):
 * *pairs, *products and *specific are one record per target each, in the order given, of handle-owned page-locked memory, valid
 * until the handle's next call of this function, load or close.  The shortlisted oligos of a batch of targets are searched
 * together, one pass over the record per batch; the result does not depend on the batches.  States and refusals are those of
 * ribbit_hip_record_primer_pairs and ribbit_hip_record_primer_products: a field of any of the three parameter sets outside its
 * range is RIBBIT_E_ARG and the error text names the field, and so is params->min_length below product_params->seed (a
 * shortlisted primer would be shorter than the seed); before a load: RIBBIT_E_STATE.  n_targets = 0 and L = 0 are no errors. */
int ribbit_hip_record_specific_primer_pairs(RibbitHandle *h, const int32_t *intervals, size_t n, const int32_t *targets, size_t n_targets,
                                            const RibbitPrimerParams *params, const RibbitPrimerPairParams *pair_params,
                                            const RibbitProductParams *product_params, const RibbitRowPrimerPair **pairs,
                                            const RibbitRowProducts **products, const RibbitRowSpecific **specific);
/* Host-only twin (no GPU), from the bytes of `sequence` (0 <= length < 2^31), letter by letter: the three arrays malloc'ed, release
 * each with ribbit_primer_specific_free(). */
int ribbit_host_record_specific_primer_pairs(const char *sequence, int64_t length, const int32_t *intervals, size_t n, const int32_t *targets,
                                             size_t n_targets, const RibbitPrimerParams *params, const RibbitPrimerPairParams *pair_params,
                                             const RibbitProductParams *product_params, RibbitRowPrimerPair **pairs,
                                             RibbitRowProducts **products, RibbitRowSpecific **specific);
void ribbit_primer_specific_free(void *from_the_host_twin);
/* For tests: the targets of one batch of ribbit_hip_record_specific_primer_pairs on this handle; 0 restores the rule (as many as
 * 256 MiB of site lists hold with 16 distinct oligos per target: 32,768 at max_sites 64). */
int ribbit_hip_debug_set_specific_batch(RibbitHandle *h, size_t targets);
/* The targets' BED rows with their specific pairs (host only): the 38 columns of ribbit_bed_primer_products_text for the chosen
 * pair, then four more, 42 in all: place, pairs_specific, pairs_over, pairs_other.  Without a pair the first 18 pair columns, the
 * six product columns and place are "."; the counts stay.  bed_text and the refusals as for ribbit_bed_primer_pairs_text.  *text
 * malloc'ed, release with ribbit_text_free(). */
int ribbit_bed_primer_specific_text(const char *bed_text, size_t bed_len, const RibbitRowPrimerPair *pairs, const RibbitRowProducts *products,
                                    const RibbitRowSpecific *specific, size_t n, char **text, size_t *len);

/*
 * ---- the best primer pair of every target that amplifies nothing in any record of a genome ---------------------------------
 * The specific primer pairs above search the record a target lies on.  Here a target's two shortlists leave that record, are
 * judged on every record of the input, and the judgements are summed.  Everything is integer arithmetic on letters; nothing is
 * added to the three contracts above.
 *   Genome:     the records R_0 .. R_{n-1} of the input.  A target belongs to its HOME record R_h.  Home is a matter of position
 *               in the input, not of name: two records with one name are two records.
 *   Shortlists: a target's shortlists, its admissible pairs and their order are exactly steps (1) to (3) of the selection and
 *               the order of the specific contract, made on the home record against the home record's rows.
 *   Judgement:  on one record R_k an admissible pair (l, r) is judged by the in-silico PCR contract on R_k with the same a and b.
 *               Only when k = h does the own product exist (a forward at the left candidate's start, b reverse at the right
 *               candidate's start); on any other record no product is the pair's own.  The pair is OVER on R_k when one of
 *               its four site lists on R_k is longer than max_sites; otherwise its others on R_k are products - own.
 *   Sum:        over all records the pair is OVER when it is over on any record; otherwise OTHER when its others, summed over
 *               the records, are above 0; otherwise SPECIFIC.
 *   Choice:     the chosen pair is the first specific pair in the order.  There is no fallback.
 *   One record: with n = 1 this is the specific primer pair contract, field by field.
 *   max_sites:  holds per record: it is the longest list that is kept on one record, not a limit on a genome's total.  A site
 *               count summed over the records may therefore exceed max_sites without the pair being over.
 *   Values:     R_0 = the undisturbed record of the specific contract's values, the target (1500, 1540), no rows, the defaults;
 *               R_1 = B, 4,000 other random bases (tests/primer_genome_contract.py builds the genomes and computes the values
 *               from a plain statement of the above).  As (place, pairs_admissible, pairs_specific, pairs_over, pairs_other,
 *               first_products) and the chosen pair's (left start, left length, right start, right length):
 *                 R_1 = B                                                      (0, 44, 44, 0, 0, 0)     (1304, 22, 1624, 21)
 *                 B with R_0's best pair's two windows at 3000 and 60 behind   (2, 44, 30, 0, 14, 1)    (1304, 22, 1613, 22)
 *                 B with R_0[1300:1500] at 2600 and R_0[1540:1740] at 2800     (-1, 44, 0, 0, 44, 1)    no pair
 *               Within one record the same two constructions give 18 other and first_products 2: a copy in another record
 *               cannot form a product with the original.
 */
typedef struct {
    RibbitPrimer left[8], right[8];           /* by rank; an empty place has start -1 and zeros; the held places are the first ones */
    int32_t left_candidates, right_candidates, left_passed, right_passed;
} RibbitTargetShortlists;                     /* 100 ints, 400 bytes */
typedef struct {
    uint64_t admissible, over, other, own;    /* bit 8 l + r for the pair (l, r) of the two shortlists */
    int32_t forward[16], reverse[16];         /* the sites of left[0..7], then of right[0..7] as ordered; 0 for an empty place; exact */
    int32_t first_others;                     /* of the pair in place 0: -1 over, else products - own; 0 without an admissible pair */
    int32_t records, home_records;            /* records judged; how many of them as home */
    int32_t reserved;                         /* 0 */
} RibbitTargetVerdicts;                       /* 176 bytes */
/* The two shortlists of the loaded record's n_targets targets against the coverage of its n rows, on the GPU (the lists
 * ribbit_hip_record_specific_primer_pairs makes internally, handed out): *lists is one record per target, in the order given, of
 * handle-owned page-locked memory, valid until the handle's next call of this function, load or close.  States and refusals are
 * those of ribbit_hip_record_primer_pairs.  n_targets = 0 and L = 0 are no errors. */
int ribbit_hip_record_primer_shortlists(RibbitHandle *h, const int32_t *intervals, size_t n, const int32_t *targets, size_t n_targets,
                                        const RibbitPrimerParams *params, const RibbitPrimerPairParams *pair_params,
                                        const RibbitTargetShortlists **lists);
/* Every target's admissible pairs judged on the loaded record, which may be any record, on the GPU (primer_specific.hip):
 * home is 1 when the loaded record is the one the lists were made on, else 0.  `admissible` comes from the lists alone, by
 * step (3); over, other and own are subsets of it; records is 1 and home_records is home.  Targets go in batches by the rule of
 * ribbit_hip_record_specific_primer_pairs (ribbit_hip_debug_set_specific_batch is obeyed); the result does not depend on the
 * batches.  *verdicts is handle-owned page-locked memory, valid until the handle's next call of this function, load or close.
 * Malformed lists (a held place behind an empty one, a length below `seed` or above 32, more held places than
 * pair_params->shortlist) are RIBBIT_E_ARG, and the error text names the target's index; a parameter field outside its range
 * is RIBBIT_E_ARG and the text names the field; before a load: RIBBIT_E_STATE.  n_targets = 0 and L = 0 are no errors: with
 * L = 0 there are no sites, and `admissible` is still filled. */
int ribbit_hip_record_shortlist_verdicts(RibbitHandle *h, const RibbitTargetShortlists *lists, size_t n_targets, int32_t home,
                                         const RibbitPrimerPairParams *pair_params, const RibbitProductParams *product_params,
                                         const RibbitTargetVerdicts **verdicts);
/* Host-only twins (no GPU), from the bytes of `sequence` (0 <= length < 2^31), letter by letter: *lists and *verdicts malloc'ed,
 * release with ribbit_primer_genome_free(). */
int ribbit_host_record_primer_shortlists(const char *sequence, int64_t length, const int32_t *intervals, size_t n, const int32_t *targets,
                                         size_t n_targets, const RibbitPrimerParams *params, const RibbitPrimerPairParams *pair_params,
                                         RibbitTargetShortlists **lists);
int ribbit_host_record_shortlist_verdicts(const char *sequence, int64_t length, const RibbitTargetShortlists *lists, size_t n_targets,
                                          int32_t home, const RibbitPrimerPairParams *pair_params,
                                          const RibbitProductParams *product_params, RibbitTargetVerdicts **verdicts);
/* The sum over records (host only): into[i] becomes the verdicts of into[i]'s and from[i]'s records together.  `admissible` must
 * be equal, else RIBBIT_E_ARG and the text names the index (nothing is changed then); over, other and own are OR-ed; the site
 * counts, records and home_records are added and saturate at INT32_MAX; first_others is -1 if either side's is -1, else the
 * saturating sum. */
int ribbit_primer_verdicts_merge(RibbitTargetVerdicts *into, const RibbitTargetVerdicts *from, size_t n);
/* The choice (host only): per target the admissible pairs of its lists in the order, the first one outside over | other.  *pairs
 * is that pair's record exactly as ribbit_hip_record_specific_primer_pairs would fill it (ranks, the five dimer values, the six
 * counts); *products its four site counts from forward and reverse, own its bit, products equal to own, shortest_other 0 (eight
 * zeros without a pair); *specific the popcounts of the three classes (a pair that is over on one record and other on another is
 * over), place, and first_products = first_others.  Verdicts whose home_records is not 1, whose `admissible` is not that of the
 * lists, and malformed lists are RIBBIT_E_ARG with the target's index.  The three arrays are malloc'ed, release each with
 * ribbit_primer_genome_free(); ribbit_bed_primer_specific_text prints them as they are. */
int ribbit_primer_shortlists_choose(const RibbitTargetShortlists *lists, const RibbitTargetVerdicts *verdicts, size_t n,
                                    const RibbitPrimerPairParams *pair_params, RibbitRowPrimerPair **pairs,
                                    RibbitRowProducts **products, RibbitRowSpecific **specific);
void ribbit_primer_genome_free(void *from_a_host_function);

/*
 * ---- every chosen primer pair typed on another assembly: where its product lies there and how long its repeat is -----------
 * What GMATA calls e-mapping: the chosen pairs of one assembly run against the records of a second one (another individual,
 * strain or haplotype, the previous release), to read off whether the marker transfers and how long its allele is there.
 * Everything is integer arithmetic on letters; nothing is added to the site and product definitions of the in-silico PCR
 * contract above.  Gapped or thermodynamic binding, more than the first product, chunks and several GPUs are not part of it.
 *   Inputs:     all of them refer to the loaded record R[0, L), which may be any record.  n pairs as RibbitRowPrimerPair, of
 *               which only the two primers' length and bases are read (and left.start < 0: a target without a pair); a is the
 *               left primer, b the right primer as ordered; no product is "own".  Per pair a motif w of m letters,
 *               1 <= m <= 1023, letters ACGT, as a pool and int32 offsets exactly as ribbit_bed_motifs hands them out; the
 *               refusals are those of ribbit_hip_record_classes.  A RibbitProductParams.  An int32 `record` label >= 0.
 *   Counts:     the four site counts are exact.  products is as in the product contract, -1 when one of the four lists is
 *               longer than max_sites.
 *   First product:  when products > 0.  Among the products (f, v) the one with the least key (f.x, v.x + v.k, forward_of,
 *               reverse_of), forward_of and reverse_of being 0 for a site of a and 1 for a site of b.  start = f.x,
 *               end = v.x + v.k, inner_start = f.x + f.k, inner_end = v.x.  The inner part may be empty.
 *   Tract:      the longest stretch [s, e) inside [inner_start, inner_end) with e - s >= 2 m (a single unit is no repeat), no
 *               byte of it `other`, and, case ignored, R[s + j] == w[(p + j) mod m] for some phase p and all j (strand 0), or
 *               otherwise the same with revcomp(w) (strand 1).  Of equal lengths the leftmost; when both strands fit one stretch
 *               (a motif whose reverse complement is a rotation of itself) the strand is 0.  Without a tract
 *               tract_start = tract_end = -1 and the strand is 0.
 *               An equivalent form: with ok[x] = (R[x] == R[x - m], both bases, both inside the inner part), the tracts are
 *               the maximal ok stretches [u, v) with v - u >= m, taken as [u - m, v), whose first m letters are a rotation of w
 *               or of revcomp(w).  The kernel works in this form, the host twin in the first.
 *   Record:     with products <= 0, `record` and the six positions are -1 and forward_of, reverse_of, tract_strand are 0; with
 *               products > 0, `record` is the label given.  A pair whose left.start < 0 is sixteen zeros except that `record`
 *               and the positions are -1.
 *   Sum:        over records (ribbit_pair_amplicons_merge): the four counts add and saturate at INT32_MAX; products is -1 if
 *               either is -1, else the saturating sum; when the result is -1 the amplicon fields are the "none" values above,
 *               otherwise they are those of `into` if into.products > 0, else those of `from`: a caller that merges in record
 *               order keeps the first record's product.
 *   Values:     with Lp = GATTACAGATTACAGGCT, Rp = CCTGAAGTCTCGGATCAA, a = Lp, b = revcomp(Rp), X = ACGTTGCATG, Y = CCATGACTGA,
 *               rec = Lp X (CA)10 Y Rp (76 bases) and the defaults (tests/amplicons_contract.py computes them from a plain
 *               statement of the above), as counts, products, (start, end, forward_of, reverse_of, inner_start, inner_end,
 *               tract_start, tract_end, tract_strand):
 *                 rec, CA (and AC)                    (1,0,0,1)  1  (0,76,0,1,18,58,28,49,0)   the tract takes Y's first C
 *                 rec, TG                             (1,0,0,1)  1  the same with strand 1
 *                 revcomp(rec), CA                    (0,1,1,0)  1  (0,76,1,0,18,58,27,48,1)
 *                 Lp X (CA)17 Y Rp, CA                (1,0,0,1)  1  (0,90,0,1,18,72,28,63,0)
 *                 Lp X (CA)4 N (CA)5 Y Rp, CA         (1,0,0,1)  1  (0,75,0,1,18,57,37,48,0)
 *                 Lp X CA Y Rp, CA                    (1,0,0,1)  1  (0,58,0,1,18,40,-1,-1,0)
 *                 rec in lower case, CA               as the first line
 *                 rec ACGTAGCTAGCTAGGATCGA rec, CA    (2,0,0,2)  3  (0,76,0,1,18,58,28,49,0)
 *                 Lp (GATA)6 Rp, ATAG                 (1,0,0,1)  1  (0,60,0,1,18,42,18,42,0)
 *                 Lp X, CA                            (1,0,0,0)  0  none
 */
typedef struct {
    int32_t left_forward, left_reverse, right_forward, right_reverse;   /* the sites of a and of b, exact */
    int32_t products, record;
    int32_t start, end, forward_of, reverse_of, inner_start, inner_end;
    int32_t tract_start, tract_end, tract_strand, reserved;             /* reserved 0 */
} RibbitRowAmplicon;                          /* 16 ints, 64 bytes */
/* The n pairs (at most 2^24) on the loaded record, on the GPU (amplicons.hip): the site scan of ribbit_hip_record_primer_products,
 * one lane per pair for the counts and the first product, one wavefront per pair with a product for the tract.  *rows is one
 * record per pair in the order given, of handle-owned page-locked memory, valid until the handle's next call of this function,
 * load or close.  Only pairs with left.start >= 0 send oligos; pairs go in batches, as many as 256 MiB of site lists hold with
 * 2 oligos per pair (ribbit_hip_debug_set_specific_batch is obeyed, counting pairs); the result does not depend on the batches.
 * n = 0 and L = 0 are no errors.  A field of params outside its range, a primer of fewer than `seed` or more than 32 bases, a
 * bad motif pool, a negative record: RIBBIT_E_ARG with the field or index in the text; before a load: RIBBIT_E_STATE.  A record
 * loaded as one chunk of a longer one is not served as that record: the piece is judged as the record it is. */
int ribbit_hip_record_pair_amplicons(RibbitHandle *h, const RibbitRowPrimerPair *pairs, size_t n, const char *motifs, const int32_t *offsets,
                                     int32_t record, const RibbitProductParams *params, const RibbitRowAmplicon **rows);
/* Host-only twin (no GPU), from the bytes of `sequence` (0 <= length < 2^31), letter by letter in loops, the tract in its first
 * form: *rows malloc'ed, release with ribbit_pair_amplicons_free(). */
int ribbit_host_record_pair_amplicons(const char *sequence, int64_t length, const RibbitRowPrimerPair *pairs, size_t n, const char *motifs,
                                      const int32_t *offsets, int32_t record, const RibbitProductParams *params, RibbitRowAmplicon **rows);
/* The sum over records (host only), as above: into[i] becomes the amplicon of into[i]'s and from[i]'s records together. */
int ribbit_pair_amplicons_merge(RibbitRowAmplicon *into, const RibbitRowAmplicon *from, size_t n);
void ribbit_pair_amplicons_free(void *from_the_host_twin);
/* The targets' BED rows as markers (host only): line i of bed_text, byte for byte, then 20 columns, each behind a tab, and a
 * newline.  1 to 9 are the eight primer columns and the designed product as ribbit_bed_primer_pairs_text writes them; 10 is
 * `products` on the other assembly, "." when it is -1; 11 to 20 are filled only when products == 1, otherwise ".": the record's
 * name (names[name_offsets[record] .. name_offsets[record + 1]), n_records names), start, end, the orientation ("+" for
 * (forward_of, reverse_of) = (0, 1), "-" for (1, 0), "l" for (0, 0), "r" for (1, 1)), the size end - start, the size minus the
 * designed product, tract start, tract end, the tract's bases and its whole units, bases / m with m the length of the row's
 * motif (column 4 of the row); without a tract the last four are ".".  A row without a pair has "." in all 20.  A bed_text that
 * does not have n lines or holds a line that is no row, a primer of fewer than 1 or more than 32 bases, a `record` outside
 * the names where products > 0: RIBBIT_E_ARG.  *text malloc'ed, release with ribbit_text_free(). */
int ribbit_bed_marker_text(const char *bed_text, size_t bed_len, const RibbitRowPrimerPair *pairs, const RibbitRowAmplicon *amplicons,
                           const char *names, const int32_t *name_offsets, size_t n_records, size_t n, char **text, size_t *len);

/*
 * ---- multiplex PCR panels: the markers pooled so that no two members of a pool disturb each other --------------------------
 * What Multiplex Manager, MPprimer and PrimerPooler do behind e-mapping: the markers worth ordering go into pools (tubes, lanes);
 * within a pool no primer may bind a primer of another marker, the products must be tellable apart by size, and two markers
 * that lie close together on one record must not make a product between them.  Everything is integer arithmetic on letters
 * and positions.  dG, gapped dimers, dye colours and an optimal colouring are not part of it: first fit along the degree order
 * is a heuristic, and the rule below is what is pinned.
 *   Inputs:     n pairs as RibbitRowPrimerPair, 0 <= n <= RIBBIT_PANEL_MAX_PAIRS, of which only left and right (start, length,
 *               bases) and product are read; left.start < 0: no pair.  Optionally 3 n int32 `extra`, (group, size_lo, size_hi) per
 *               pair; NULL stands for (-1, product, product) everywhere.  group >= 0 names the record the pair lies on, -1: unknown;
 *               size_lo <= size_hi are the product sizes the marker is expected to show.  A RibbitPanelParams.
 *   Oligos:     those of the pair contract: L is the left primer's forward-strand bases, R the reverse complement of the right
 *               primer's forward-strand bases; any(x, y) and end(x, y) are exactly the pair contract's.
 *   Conflict:   of two different pairs i and j that both have a pair, the OR of three rules.
 *               dimer: for some x in {L_i, R_i} and some y in {L_j, R_j}, any(x, y) > max_cross_any or end(x, y) > max_cross_end.
 *               size:  size_gap > 0, size_lo_i - size_hi_j < size_gap and size_lo_j - size_hi_i < size_gap (the ranges lie less
 *                      than size_gap apart).
 *               near:  max_cross_product > 0, group_i == group_j >= 0, and max(end_i, end_j) - min(start_i, start_j) <=
 *                      max_cross_product, the span of a pair being [left.start, right.start + right.length): the product that L
 *                      of one pair and R of the other can make, which the in-silico PCR contract would count.
 *               The relation is symmetric and has no diagonal; a row without a pair conflicts with nobody.
 *   Degree:     conflicts_i is the number of j in conflict with i; dimer_i, size_i and near_i count each rule on its own (one j
 *               may count in several).  The rows that have a pair are ordered by (conflicts descending, index ascending): the
 *               Welsh-Powell order.
 *   Pools:      first fit along that order: a pair goes into the lowest-numbered pool that has fewer than pool_size members and
 *               no member in conflict with it; if there is none it opens the next pool.  A row without a pair has pool -1 and
 *               counts of 0.  The low-numbered pools fill first, so the first k pools are the natural smaller panel.
 *   Defaults:   the cross limits are 6 and 4, not the pair's own 4 and 3: among random oligos of 18 .. 25 bases at the pair's
 *               own limits three of four pair-to-pair combinations conflict and a pool of eight cannot exist.
 *   Values:     from tests/panel_contract.py, a plain statement of the above.  Q0 .. Q3 are four pairs of eight oligos of which no
 *               two exceed (6, 4) (TTCAGGACCTAACCTGAG / TAGCCAAGTTCAACGGCAG, TGCAACCTAGGGAGAATGTG / ACATACGCTCTTACTGCGGTC,
 *               CGGAGCATAAATCCCACC / GAACTAAGTTTGTCGAACC, GGTAAACGAACCGTTGCG / AATTTGAAGCAGTGGCCGGG), Qk(s, p) with left.start
 *               s and product p; the defaults unless stated; as the pairs' pools, then (conflicts, dimer, size, near) of each:
 *                 Q0(0, 100), Q1(1000, 150)                                  0 0      all (0,0,0,0)
 *                 GATTACAGATTACAGGC / Q0's left, Q1's left / TTTGCCTGTAATC     0 1      both (1,1,0,0): the duplex is (10, 10)
 *                   the same with max_cross_any = max_cross_end = 32         0 0      the dimer rule refuses nothing
 *                 Q0(0, 100), Q1(0, 129)                                     0 1      both (1,0,1,0)    products 130: 0 0
 *                   the same with size_gap 0                                 0 0
 *                 Q0(0, 100), Q1(3850, 150), both in group 5                 0 1      both (1,0,0,1): the hull is 4000
 *                   Q1(3851, 150): hull 4001; or groups 5 and 6; or -1, -1   0 0
 *                 Q0, Q1, Q2 with pool_size 1                                0 1 2
 *                 Q0(0, 100), Q1(0, 200), Q2(0, 300), Q3(0, 200) with sizes 90 .. 310     1 1 1 0
 *                                                                            (1,0,1,0) three times, (3,0,3,0): the degree order
 *                                                                            takes Q3 first; index order would give 0 0 0 1
 *                 Q0, a row without a pair, Q1                               0 -1 0
 */
#define RIBBIT_PANEL_MAX_PAIRS 65536
#define RIBBIT_PANEL_MAX_DEBUG_PAIRS 8192
typedef struct {
    int32_t max_cross_any, max_cross_end;     /* 6, 4;  0 .. 32 each: at 32 the dimer rule never refuses */
    int32_t size_gap;                         /* 30;  0 .. 100000, 0: no size rule */
    int32_t max_cross_product;                /* 4000;  0 .. 2^30, 0: no near rule */
    int32_t pool_size;                        /* 8;  1 .. 65536 */
} RibbitPanelParams;
void ribbit_panel_params_default(RibbitPanelParams *params);
typedef struct {
    int32_t pool;                             /* -1: no pair */
    int32_t conflicts, dimer, size, near;
    int32_t reserved[3];                      /* 0 */
} RibbitPanelRow;                             /* 8 ints, 32 bytes */
/* The n pairs pooled on the GPU (panel.hip): the conflict matrix, one lane per row against tiles of columns in LDS; the degrees;
 * one radix sort for the order; the first fit by a single workgroup, so that the matrix (512 MiB at the cap) never leaves the
 * device.  The call needs a handle and no loaded record: it reads none, and may come before any load.  *rows is one record per
 * pair in the order given, of handle-owned page-locked memory, valid until the handle's next panel call or close; *n_pools the
 * pools in use; on an error *rows is NULL and *n_pools 0.  n = 0 is no error.  A field of params outside its range:
 * RIBBIT_E_ARG, and the text names the field; n above the cap, a primer of fewer than 1 or more than 32 bases, size_lo > size_hi,
 * group < -1: RIBBIT_E_ARG with the index in the text. */
int ribbit_hip_panel_pools(RibbitHandle *h, const RibbitRowPrimerPair *pairs, const int32_t *extra, size_t n,
                           const RibbitPanelParams *params, const RibbitPanelRow **rows, int32_t *n_pools);
/* Host-only twin (no GPU), letter by letter in loops over pairs and placements: *rows malloc'ed, release with ribbit_panel_free().
 * It is the reference for panels of thousands of pairs, not a way to pool at the cap: with m rows that have a pair it holds m^2
 * bytes (4 GiB at 65536; RIBBIT_E_NOMEM when that is not to be had) and makes 2 m^2 duplexes in letters, seconds at m = 4096. */
int ribbit_host_panel_pools(const RibbitRowPrimerPair *pairs, const int32_t *extra, size_t n, const RibbitPanelParams *params,
                            RibbitPanelRow **rows, int32_t *n_pools);
void ribbit_panel_free(void *from_the_host_twin);
/* The conflict matrix itself, as the kernel leaves it (for tests of the kernel apart from the pooling): n rows of (n + 63) / 64
 * words of 64 bits, row-major; bit j % 64 of word j / 64 of row i holds the conflict of i and j.  n above
 * RIBBIT_PANEL_MAX_DEBUG_PAIRS: RIBBIT_E_ARG; everything else as ribbit_hip_panel_pools. */
int ribbit_hip_debug_panel_conflicts(RibbitHandle *h, const RibbitRowPrimerPair *pairs, const int32_t *extra, size_t n,
                                     const RibbitPanelParams *params, uint64_t *words);
/* The panel as text (host only): marker_text holds the n lines that ribbit_bed_marker_text wrote for the same n pairs (a last line
 * without its newline counts).  Only the members (pool >= 0) are written: each its marker line byte for byte, then five columns,
 * each behind a tab: pool, conflicts, dimer, size, near.  The lines are sorted by (pool, designed product size, input order), the
 * designed product being the ninth of a marker line's last 20 columns, so a pool reads like a lane.  A text that does not have n
 * lines, or a member's line that has no number there: RIBBIT_E_ARG.  *text malloc'ed, release with ribbit_text_free(). */
int ribbit_bed_panel_text(const char *marker_text, size_t len, const RibbitPanelRow *rows, size_t n, char **text, size_t *out_len);

/*
 * ---- the chosen pairs typed on many assemblies: the genotype matrix and every marker's alleles, He and PIC -----------------
 * What people who pick SSR markers (GMATA, Krait, QDD, MISA users) rank them by: the polymorphism over a set of individuals.
 * A sample is one assembly; a marker's allele in a sample is the size of its one product there.  Everything is integer
 * arithmetic.  Diploid genotype calls, null-allele estimation and alleles told apart by sequence are not part of it.
 *   Cells:      for pair i and sample s one int32, from the RibbitRowAmplicon of the pair summed over all records of the sample
 *               (what ribbit_pair_amplicons_merge leaves when the records are merged in file order):
 *                 products == 1      end - start    typed; the size is > 0
 *                 products == 0      0              absent
 *                 products >  1      -1             several
 *                 products == -1     -2             over (a primer with more than max_sites sites)
 *               and 0 for a pair without a pair (left.start < 0).  ribbit_pair_amplicon_sizes writes one sample's row.
 *   Matrix:     sample-major, cells[s n + i], 1 <= S <= RIBBIT_ALLELES_MAX_SAMPLES samples, n <= 2^24 markers.  A cell below
 *               -2: RIBBIT_E_ARG, and the text names its index s n + i.
 *   Per marker: designed[i], the designed product (designed[i] <= 0: the row has no pair, its record is sixteen zero ints), and
 *               motif_length[i] >= 1, else RIBBIT_E_ARG with the index.  Over the marker's t typed cells, with every distinct
 *               size counted c_k times, Q = sum c_k^2 and F = sum c_k^4:
 *                 typed, absent, several, over    the cells by kind; they add up to S
 *                 alleles                         the distinct sizes
 *                 min_size, max_size              0 when typed == 0
 *                 major_size, major_count         the most frequent size, of equals the least; 0, 0 when typed == 0
 *                 same                            typed cells equal to designed
 *                 off_step                        typed cells whose size - designed is not divisible by motif_length
 *                 het_num = t^2 - Q               He  = het_num / t^2  (Nei's gene diversity, no t / (t - 1) correction)
 *                 pic_num = t^4 - t^2 Q - Q^2 + F PIC = pic_num / t^4  (Botstein 1980: 1 - sum p^2 - sum_{i<j} 2 p_i^2 p_j^2)
 *               t <= 1024, so t^4 <= 2^40: the device is compared byte for byte.
 *   Values:     with designed = 100 and motif_length = 2 (tests/alleles_contract.py computes them from a plain statement of the
 *               above, in fractions), as typed/absent/several/over, alleles, min, max, major size x count, same, off_step,
 *               het_num, pic_num and the text's He and PIC:
 *                 (100,100,100,100)           4/0/0/0  1  100  100  100x4  4  0   0    0   0.0000  0.0000
 *                 (100,104)                   2/0/0/0  2  100  104  100x1  1  0   2    6   0.5000  0.3750
 *                 (100,102,102,105,0,-1,-2)   4/1/1/1  3  100  105  102x2  1  1  10  142   0.6250  0.5547
 *                 (100,102,104,106)           4/0/0/0  4  100  106  100x1  1  0  12  180   0.7500  0.7031
 *                 (0,0,0)                     0/3/0/0  everything else 0                   .       .
 *                 designed = -1, any cells    sixteen zeros
 */
#define RIBBIT_ALLELES_MAX_SAMPLES 1024
#define RIBBIT_ALLELES_MAX_MARKERS (1 << 24)
typedef struct {
    int32_t typed, absent, several, over;     /* they add up to S */
    int32_t alleles;                          /* distinct sizes among the typed */
    int32_t min_size, max_size;               /* 0 when typed == 0 */
    int32_t major_size, major_count;          /* the most frequent size, the least size among equals; 0, 0 when typed == 0 */
    int32_t same;                             /* typed cells equal to designed */
    int32_t off_step;                         /* typed cells whose size - designed is not divisible by motif_length */
    int32_t reserved;                         /* 0 */
    int64_t het_num;                          /* t^2 - Q */
    int64_t pic_num;                          /* t^4 - t^2 Q - Q^2 + F */
} RibbitRowAlleles;                           /* 64 bytes */
/* One sample's row of cells from its n summed amplicons, as the table above (host only).  products below -1, or one product
 * whose end is not behind its start: RIBBIT_E_ARG with the index.  A row whose pair has no pair sums to products == 0 and so to the cell 0. */
int ribbit_pair_amplicon_sizes(const RibbitRowAmplicon *sum, size_t n, int32_t *cells);
/* The n markers' records on the GPU (alleles.hip): a workgroup takes 16 consecutive markers, reads the samples' rows 64 bytes at a
 * time and transposes them into LDS; one wavefront per marker counts the kinds, sorts the typed sizes (bitonic, in LDS) and
 * reduces the runs of equal sizes.  The call needs a handle and no loaded record.  *rows is one record per marker in the order
 * given, of handle-owned page-locked memory, valid until the handle's next call of this function or close; on an error it is
 * NULL.  Markers go down in batches of a fixed cell budget (ribbit_hip_debug_set_specific_batch is obeyed, counting markers); the
 * result does not depend on the batches.  n = 0 is no error.  n_samples outside 1 .. 1024, n above 2^24, a motif_length below
 * 1, a cell below -2: RIBBIT_E_ARG with the index in the text, checked in this order before anything is launched. */
int ribbit_hip_marker_alleles(RibbitHandle *h, const int32_t *cells, size_t n_samples, size_t n, const int32_t *designed,
                              const int32_t *motif_lengths, const RibbitRowAlleles **rows);
/* Host-only twin (no GPU), plain loops and std::sort: *rows malloc'ed, release with ribbit_alleles_free(). */
int ribbit_host_marker_alleles(const int32_t *cells, size_t n_samples, size_t n, const int32_t *designed, const int32_t *motif_lengths,
                               RibbitRowAlleles **rows);
void ribbit_alleles_free(void *from_the_host_twin);
/* The targets' BED rows with their alleles (host only): line i of bed_text, byte for byte, then 23 columns, each behind a tab,
 * and a newline.  1 to 9 are the eight primer columns and the designed product as ribbit_bed_marker_text writes them; then S,
 * typed, absent, several, over, alleles, min_size, max_size, major_size, major_count, same, off_step, He and PIC.  He and PIC
 * have four decimals, rounded half up in integers: (num 10000 + den / 2) / den with den = typed^2 and typed^4.  With
 * typed == 0 the columns min_size, max_size, major_size, He and PIC are ".".  A row without a pair (left.start < 0 or
 * right.start < 0) has "." in all 23.  A bed_text that does not have n lines, a primer of fewer than 1 or more than 32 bases,
 * n_samples outside 1 .. 1024, a record whose typed is outside 0 .. n_samples: RIBBIT_E_ARG.  *text malloc'ed, release with
 * ribbit_text_free(). */
int ribbit_bed_alleles_text(const char *bed_text, size_t bed_len, const RibbitRowPrimerPair *pairs, const RibbitRowAlleles *rows,
                            size_t n_samples, size_t n, char **text, size_t *len);
/* The genotype matrix as text (host only).  A header line: "#name", "start", "end", "motif", "designed", then the n_samples names
 * (names[name_offsets[s] .. name_offsets[s + 1])), tab-separated.  Then one line per row in the order of bed_text: columns 1 to 4
 * of the row, the designed product ("." when designed[i] <= 0) and one field per sample: the size of a typed cell, "." absent,
 * "+" several, "*" over.  A bed_text that does not have n lines or holds a line that is no row, a cell below -2, n_samples
 * outside 1 .. 1024: RIBBIT_E_ARG.  *text malloc'ed, release with ribbit_text_free(). */
int ribbit_allele_matrix_text(const char *bed_text, size_t bed_len, const int32_t *cells, size_t n_samples, size_t n,
                              const int32_t *designed, const char *names, const int32_t *name_offsets, char **text, size_t *len);

/*
 * ---- streaming FASTA ingest ---------------------------------------------------------------------------------------
 * Replaces the reader loop of ribbit.cpp:269-280 (getline + `sequence += line` into one pageable std::string per
 * record).  The file is read in 16-MB blocks; line bodies are copied once, straight into a page-locked buffer
 * (pinned != 0; plain malloc otherwise, for hosts without a GPU) that ribbit_hip_load_record_pinned uploads from
 * asynchronously and refinement reads in place.  Record boundaries follow the reference loop exactly: a '>' line ends
 * the previous record if it has any bases and names the next one (text up to the first space); other lines are appended
 * without their '\n'; the last record is handed out even when it is empty (*is_last = 1: ribbit.cpp:280 processes it
 * without the "Processing sequence" line).
 * ribbit_fasta_next returns 1 with a record, 0 after the last one, < 0 on error; *bases stays valid until
 * ribbit_fasta_release (any thread) or ribbit_fasta_close; released buffers are reused.
 */
typedef struct RibbitFastaReader RibbitFastaReader;
int ribbit_fasta_open(const char *path, int pinned, RibbitFastaReader **out);
int ribbit_fasta_next(RibbitFastaReader *r, const char **name, const char **bases, int64_t *length, int *is_last);
int ribbit_fasta_release(RibbitFastaReader *r, const char *bases);
int ribbit_fasta_close(RibbitFastaReader *r);
const char *ribbit_fasta_last_error(void);

/* How often the defined-divergence guards fired in the merges of this record (the
 * reference has undefined behaviour there; 0 on ordinary inputs). */
int64_t ribbit_hip_guard_hits(const RibbitHandle *h);

/*
 * Bits [start, end) of shift plane `shift` (X_shift; for a motif length, the composed plane XA_shift once the anchored
 * stage has run on this record -- ribbit_hip_anchored_calls / ribbit_hip_seeds_anchored), one byte per base.  Replaces reads of
 * lshift_xor_bsets[shift-MINIMUM_SHIFT][L-1-p] (fasta_utils.cpp:220-222, parse_seed.cpp:366).
 */
int ribbit_hip_plane_bits(RibbitHandle *h, int32_t shift, int64_t start, int64_t end, uint8_t *out);

/* Popcount of plane `shift` over [start, end): the loop of retainNestedSeed /
 * retainIdenticalSeeds (parse_perfect_shiftxor.cpp:18-43). */
int ribbit_hip_range_popcount(RibbitHandle *h, int32_t shift, int64_t start, int64_t end, int32_t *count);

/* Packed device planes copied back to the host (LSB-first: base p is bit p%32 of word p/32);
 * each array holds ribbit_hip_plane_words() words.  which: 0 left bit, 1 right bit, 2 N mask. */
int64_t ribbit_hip_plane_words(const RibbitHandle *h);
int ribbit_hip_packed_plane(RibbitHandle *h, int which, uint32_t *out_words);

/*
 * Host-only replay of scanner call lists through the order-dependent seed-list merges
 * (addSeedToSeedPositionsPerfect / ...Substitutions).  This is the host half of
 * ribbit_hip_seeds_*: it needs no GPU, only the packed planes (LSB-first words as returned by
 * ribbit_hip_packed_plane, padded with at least max_motif/32 + 4 zero words past word L/32) for
 * the range popcounts of retainNestedSeed / retainIdenticalSeeds.  Used when the call lists come
 * from elsewhere: other ranks in chunk-sharded multi-GPU runs, or the CPU tests of the merges.
 * The arrays in *out are malloc'ed; release them with ribbit_seed_lists_free().
 */
typedef struct RibbitSeedLists {
    RibbitSeed *perfect;  size_t n_perfect;
    RibbitSeed *subst;    size_t n_subst;
    RibbitSeed *anchored; size_t n_anchored;
    RibbitSeed *dispatch; size_t n_dispatch;   /* fasta_utils.cpp:187-224 order */
    int64_t guard_hits;   /* defined-divergence guards that fired */
} RibbitSeedLists;
/* xa: composed planes XA_m for m = min_motif..max_motif, xa_stride words each; may be NULL: the slices the merges
 * read are then recomputed from the packed planes (as in the GPU path, where the composed planes stay in HBM).
 * anchored_calls == NULL and xa == NULL: the anchored stage is not run (no dispatch list). */
int ribbit_host_replay_calls(const RibbitScanParams *params, int64_t length,
                             const uint32_t *hi, const uint32_t *lo, const uint32_t *brk, size_t nwords,
                             const uint32_t *xa, size_t xa_stride,
                             const RibbitCall *perfect_calls, size_t n_perfect_calls,
                             const RibbitCall *subst_calls, size_t n_subst_calls,
                             const RibbitCall *anchored_calls, size_t n_anchored_calls,
                             RibbitSeedLists *out);
void ribbit_seed_lists_free(RibbitSeedLists *lists);

/*
 * ---- chunk-sharded operation: one long record scanned by several GPUs ----------------------------
 * Every scan kernel's output is a stream of events whose values depend on the sequence only within a
 * bounded distance (perfect: 32 + M+2 bases to the right, 33 to the left; window scans: 8 + M+2 / 1;
 * anchored: 4*(M+2) + 16 / 2*(M+2) + 8).  A rank therefore loads its chunk plus halos as a record of
 * its own and runs the whole device side of every stage on it -- scan, pairing of the events, window state
 * machines, length filters -- keeping the run records and the addSeed calls it owns; those sparse 16-byte
 * records are gathered (gather-v over RCCL) and one host runs the order-dependent merges on them exactly
 * as for a single GPU (ribbit_hip_scan_perfect_chunk, ribbit_hip_stage_calls_chunk, ribbit_host_merge_chunks).
 *
 * Events are 64-bit: bits 0-31 position, 32-47 motif length, 48-51 kind (0 START, 1 END closed by a
 * mismatch / failing window, 2 END at an N, 3 END at the end of the loaded record).
 */
#define RIBBIT_EVENT_POS(e)  ((uint32_t)(e))
#define RIBBIT_EVENT_MLEN(e) ((uint32_t)((e) >> 32) & 0xffffu)
#define RIBBIT_EVENT_KIND(e) ((uint32_t)((e) >> 48) & 0xfu)
enum { RIBBIT_STAGE_PERFECT = 0, RIBBIT_STAGE_SUBST = 1, RIBBIT_STAGE_ANCHORED = 2 };

/* Perfect stage of one chunk: scan, keep the events owned ([own_lo, own_hi) local, shifted by pos_offset) and
 * pair them locally.  runs = complete runs; halves = the unmatched events at the chunk's edges (a motif's
 * leading END / trailing START: that run continues in a neighbouring chunk).  After gathering, the halves of
 * all ranks sorted by (motif, position) alternate START, END and pair up into the remaining runs. */
int ribbit_hip_perfect_runs_partial(RibbitHandle *h, int64_t own_lo, int64_t own_hi, int64_t pos_offset,
                                    const RibbitRun **runs, size_t *n_runs, const uint64_t **halves, size_t *n_halves);

/* The same on the device end to end (no event ever reaches the host): scan the loaded piece, pair on the GPU, and
 * deliver one record per run START of the piece, ordered by (motif, start), into dst (caller's buffer of dst_cap
 * records; ideally pinned, see ribbit_hip_host_register) or, when dst is NULL, into handle-owned pinned memory;
 * *out is where they are.  A record is either a complete run owned by this chunk (START in [own_lo, own_hi), END
 * before own_hi; term = RIBBIT_TERM_*) or a place holder to skip (term = RIBBIT_RUN_NOT_OWNED: the run belongs to
 * a neighbour or is cut by the own range).  The cut runs -- at most two per motif -- go to half_dst / *halves:
 *   term RIBBIT_RUN_HALF_START     START owned, the END lies in a later chunk (end = -1);
 *   term RIBBIT_RUN_HALF_END + t   END owned (terminator t), the START lies in an earlier chunk (start = -1).
 * Over all chunks of a record the halves, ordered by (motif, position), pair up START, END into the remaining runs.
 * Positions are shifted by pos_offset.  A whole record is own_lo = 0, own_hi = INT64_MAX, pos_offset = 0: only
 * complete runs, no halves (that is what ribbit_hip_scan_perfect_runs does).
 * Replaces the run bookkeeping of parse_perfect_shiftxor.cpp:173-223 for one chunk of a chunk-sharded record. */
enum { RIBBIT_RUN_NOT_OWNED = -1, RIBBIT_RUN_HALF_START = 3, RIBBIT_RUN_HALF_END = 4 };
int ribbit_hip_scan_perfect_chunk(RibbitHandle *h, int64_t own_lo, int64_t own_hi, int64_t pos_offset,
                                  RibbitRun *dst, size_t dst_cap, RibbitRun *half_dst, size_t half_dst_cap,
                                  const RibbitRun **out, size_t *n, const RibbitRun **halves, size_t *n_halves);

/* The same scan split in two, for callers that keep several handles (each has its own HIP stream) busy: _begin
 * enqueues the load's pack, the scan and the pairing kernels and returns at once; _end waits for them and
 * copies the records down (arguments as for ribbit_hip_scan_perfect_chunk).  With two handles, one record's
 * kernels run while the previous record's runs cross PCIe -- the double-buffered streaming of a multi-record
 * FASTA (ribbit.cpp:269-280 is the loop being pipelined).  A whole record: own_lo 0, own_hi INT64_MAX, offset 0. */
int ribbit_hip_scan_perfect_begin(RibbitHandle *h, int64_t own_lo, int64_t own_hi, int64_t pos_offset);
/* wait != 0: the records are in place when the call returns.  wait == 0: the counts are final but the records are
 * still being copied; ribbit_hip_scan_perfect_wait (or the next _begin on the handle) completes the copy -- lets the
 * caller enqueue the next record's kernels while this one's results cross PCIe. */
int ribbit_hip_scan_perfect_end(RibbitHandle *h, RibbitRun *dst, size_t dst_cap, RibbitRun *half_dst, size_t half_dst_cap,
                                int wait, const RibbitRun **out, size_t *n, const RibbitRun **halves, size_t *n_halves);
int ribbit_hip_scan_perfect_wait(RibbitHandle *h);
/* _end without the copy to the host: the records stay where the pairing kernels wrote them.  *dev_runs / *dev_halves
 * are DEVICE pointers to *n / *n_halves RibbitRun records (complete: the call has waited for the kernels), valid until
 * the next scan on this handle.  For callers that move them on over RCCL / xGMI (the chunks' candidate seed intervals
 * of a chunk-sharded record, gathered to the rank that runs the host merge) instead of through host memory. */
int ribbit_hip_scan_perfect_end_device(RibbitHandle *h, const void **dev_runs, size_t *n, const void **dev_halves, size_t *n_halves);

/*
 * ---- chunk-sharded operation, window stages: only the calls that reach a merge leave a GPU ---------------------
 * The substitution / anchored stage of ONE CHUNK of a longer record, on the device end to end: the loaded record is the
 * chunk plus halos (a "piece", starting pos_offset bases into a record of record_length bases); the window scan, the
 * pairing of its pass-streaks, the per-motif window state machine (parse_substitute_shiftxor.cpp:430-574,
 * parse_anchored_shiftxor.cpp:580-723), the stage's length filter and the call order all run on this GPU, exactly as
 * for a whole record, and the chunk keeps the addSeed calls whose SCAN POSITION it owns: own_lo <= pos - pos_offset <
 * own_hi (piece coordinates; the chunks' own ranges partition 0..record_length, the last one includes record_length,
 * the position of the end-of-sequence calls).  Results are in record coordinates; concatenated over the chunks in order
 * they are the record's kept calls in the reference's call order -- 16 bytes per kept call is all that travels.
 *
 * Exactness.  A call is a function of the sequence between the start of its group of pass-streaks and the first
 * evaluated window behind it -- bounded by the locus, not by a constant.  The piece must reach
 *   right: 4 * (max_motif + 2) + 16 bases beyond own_hi (unless it ends where the record ends): checked, RIBBIT_E_ARG;
 *   left:  far enough that (a) an evaluated window lies between the first exact position (2 * (max_motif + 2) + 8 bases
 *          into the piece) + 16 and own_lo - 8, and (b) no owned call's group starts within 8 positions of that first exact
 *          position; own_lo itself must lie at least 2 * (max_motif + 2) + 8 + 32 + 16 bases into the piece (RIBBIT_E_ARG
 *          otherwise: the last 16 are the span of the anchored scan's group filter, whose dropped groups (b) never sees).
 *          (a) and (b) are CHECKED on every call: *inexact = 1 means a repeat or a block of N reaches further left than
 *          the halo (nothing else can) and the caller loads the chunk again with a longer left halo (the results of such a
 *          call must not be used).  A piece that starts where the record starts (pos_offset == 0) is always exact.
 * calls / pend / flush: handle-owned page-locked memory, valid until the next call for the same stage on this handle;
 * dev_calls / dev_pend: the same arrays in device memory (for RCCL), valid until the next scan on the handle.
 * pend[i] (NULL: none in this chunk): for a kept call made at an N or right behind a blocked stretch, the largest end of
 * any of THIS chunk's calls before it (-1 otherwise); tail_pend: the largest end of any call of this chunk (-1: none).
 * Across chunks the bound of such a call is the larger of pend[i] and the earlier chunks' tail_pend
 * (ribbit_host_merge_chunks does that).  flush: the end-of-sequence calls, last chunk only.
 */
typedef struct RibbitChunkCalls {
    const RibbitCall *calls; size_t n;
    const int32_t *pend;
    int32_t tail_pend;
    int32_t inexact;
    const RibbitCall *flush; size_t n_flush;
    const void *dev_calls, *dev_pend;
    int64_t streaks;          /* pass-streaks the piece's scan found (diagnostic) */
} RibbitChunkCalls;
int ribbit_hip_stage_calls_chunk(RibbitHandle *h, int stage /* RIBBIT_STAGE_SUBST | RIBBIT_STAGE_ANCHORED */, int64_t own_lo, int64_t own_hi,
                                 int64_t pos_offset, int64_t record_length, RibbitChunkCalls *out);

/* Words [word_lo, word_hi) of every composed plane XA_m of the loaded piece into out + motif_index * out_stride: a chunk
 * writes its own words straight into its place in the record's planes (e.g. a page-locked segment every rank of the node
 * maps) -- ribbit_hip_xa_words with a destination stride. */
int ribbit_hip_xa_words_strided(RibbitHandle *h, int64_t word_lo, int64_t word_hi, uint32_t *out, int64_t out_stride);

/* Host-only: the merging rank's half of the chunk-sharded path.  parts[0..nparts) in chunk order: the perfect stage's run
 * records and halves of every chunk (ribbit_hip_scan_perfect_chunk; place holders are skipped, halves paired across
 * chunks) and its kept calls of both window stages (ribbit_hip_stage_calls_chunk; only the host pointers are read).
 * Planes cover the whole record (see ribbit_host_replay_calls); xa is READ IN PLACE (3 GB for a chromosome), it must stay
 * valid during the call.  Runs addSeedToSeedPositionsPerfect / ...Substitutions / ...Anchored + mergeAllLists
 * (parse_perfect_shiftxor.cpp:47-142, parse_substitute_shiftxor.cpp:18-388, parse_anchored_shiftxor.cpp:113-534,
 * merge_types.cpp:11-189) and the dispatch merge of fasta_utils.cpp:187-224 exactly as for one GPU. */
typedef struct RibbitChunkPart {
    const RibbitRun *runs; size_t n_runs;
    const RibbitRun *halves; size_t n_halves;
    RibbitChunkCalls subst, anchored;
} RibbitChunkPart;
int ribbit_host_merge_chunks(const RibbitScanParams *params, int64_t length,
                             const uint32_t *hi, const uint32_t *lo, const uint32_t *brk, size_t nwords,
                             const uint32_t *xa, size_t xa_stride, const RibbitChunkPart *parts, size_t nparts,
                             RibbitSeedLists *out);

/* Test hook: run the device-side pairing on a caller-made event stream of a record of `length` bases,
 * as if one scan had left it in one region.  *flags = 0 for a well-formed stream, otherwise the PAIR_* bits of
 * device_planes.h (1 malformed event, 2 duplicate chunk, 4 starts and ends do not alternate, 8 unterminated run,
 * 16 no room); runs receives min(*n_runs, runs_cap) records. */
int ribbit_hip_debug_pair_events(RibbitHandle *h, const uint64_t *events, size_t n, int64_t length, RibbitRun *runs, size_t runs_cap,
                                 size_t *n_runs, uint32_t *flags);

/* Test hook: the same pairing on events placed where the caller says.  events holds 64 regions of region_cap words each, laid out
 * as a scan leaves them (the chunk of one (motif, tile) contiguous inside one region, chunks in any order); counters holds the 64
 * region counters as the scan would have left them (a value above region_cap means the region overflowed: the kernels read its
 * first region_cap events).  The motif range is the handle's; no record needs to be loaded.  own_lo / own_hi / pos_offset as for
 * ribbit_hip_scan_perfect_chunk.  The caller provides the four buffers of `out`; the call fills
 *   runs       min(status[1], runs_cap, 32 * region_cap) slots, place holders included, ordered by (motif, start);
 *   halves     min(status[2], halves_cap, 2 * motifs) half records, in no particular order;
 *   status     PAIR_FLAGS, PAIR_TOTAL, PAIR_HALVES (device_planes.h);   published: the 64 counters the GPU published;
 * and then, from the same events and counters, what the host-pairing form (ribbit_hip_perfect_runs_partial) works from:
 *   dense      the regions concatenated in region order, each cut at region_cap: min(summary, dense_cap) events;
 *   summary / overflow   the number of events kept, and whether any region overflowed;
 *   table      entry (motif - min_motif) * ntile + tile = {index of the chunk's first event in dense + 1, index past its last},
 *              low word first, 0 = no chunk; ntile = length / 16384 + 1; min(motifs * ntile, table_cap) entries;
 *   table_status         bit 0 malformed event, bit 1 a (motif, tile) with two chunks. */
typedef struct RibbitDebugPairing {
    RibbitRun *runs; size_t runs_cap;
    RibbitRun *halves; size_t halves_cap;
    uint64_t *dense; size_t dense_cap;
    uint64_t *table; size_t table_cap;
    uint32_t status[3];
    uint32_t published[64];
    uint32_t summary, overflow, table_status;
} RibbitDebugPairing;
int ribbit_hip_debug_pair_events_sharded(RibbitHandle *h, const uint64_t *events, const uint32_t *counters, size_t region_cap,
                                         int64_t length, int64_t own_lo, int64_t own_hi, int64_t pos_offset, RibbitDebugPairing *out);

/* Test hook: the window stage behind the scan and the pairing (window_stage.hip: group starts, the calls kernel, the edge list
 * and its retry, the dropmap merge, the sorts, the cursor bounds, the read-back -- the same function the product runs after its
 * scan) on caller-made pass-streaks.  A record must be loaded: it supplies the length and the break plane (where the N are).
 *   stage          RIBBIT_STAGE_SUBST | RIBBIT_STAGE_ANCHORED: whose result buffers the call uses;
 *   streaks        n_streaks records (start = first passing window, end = first window behind it that does not pass, mlen,
 *                  term = RIBBIT_TERM_*), ordered by (mlen, start);
 *   full           1: every call, no length filter, no cursor bounds (min_span may be NULL); 0: the compact form;
 *   min_span       max_motif - min_motif + 1 values: the smallest end - start a call of that motif needs to be kept;
 *   own_lo, own_hi, z_lo, keep_flush, pos_offset   chunk mode as ribbit_hip_stage_calls_chunk derives it from its geometry: the
 *                  owned scan positions (piece coordinates), the first exact position (0: none), whether the end-of-sequence
 *                  calls are this chunk's, what is added to every coordinate of the result;
 *   dropped_ends   n_dropped ascending positions e: a group of pass-streaks that is NOT among the streaks ends at e (the `end`
 *                  of its last streak) and its call, made at e + 15, fails the length filter -- what the anchored scan's group
 *                  filter leaves in its dropmap.  n_dropped = 0: no dropmap.  Ignored with full;
 *   first_edge_cap first capacity of the edge-call list (0 = automatic); a list that overflows is sized by the count and the
 *                  calls kernel runs again.
 * Everything a kernel indexes with is checked first, RIBBIT_E_ARG otherwise and nothing is enqueued: 0 <= start < end <= length,
 * mlen within the handle's motif range, term in 0..2, the order, streaks of one motif that do not overlap, 0 <= e < length,
 * 0 <= own_lo <= own_hi, pos_offset + length <= INT32_MAX, at most 2^24 streaks and edge-list entries.  Streaks that no scan of
 * the loaded record could have produced are answered by the stage's own flags (RIBBIT_E_INTERNAL, e.g. "flags 0x1" for two
 * end-of-sequence calls of one motif), never by a read outside a buffer.
 * out as for ribbit_hip_stage_calls_chunk (inexact: z_lo != 0 and an owned call starts below z_lo + 8; streaks = n_streaks);
 * *n_edge: the edge calls the stage counted. */
typedef struct RibbitDebugWindowStage {
    const RibbitRun *streaks; size_t n_streaks;
    const int32_t *min_span;
    const int32_t *dropped_ends; size_t n_dropped;
    int64_t own_lo, own_hi, z_lo, pos_offset;
    size_t first_edge_cap;
    int32_t full, keep_flush;
} RibbitDebugWindowStage;
int ribbit_hip_debug_window_calls(RibbitHandle *h, int stage, const RibbitDebugWindowStage *in, RibbitChunkCalls *out, uint32_t *n_edge);

/* Test hook: the first guess of the event-buffer capacity of the scans (0 = automatic).  A guess that is too small
 * makes a scan overflow its regions, after which it is sized for the fullest region and run again. */
int ribbit_hip_debug_set_event_capacity(RibbitHandle *h, size_t events);

/* Test hook: how the scan kernels split the motif range over the blocks of a tile (gridDim.y).  kernel selects the
 * perfect scan, the substitution stage's window scan, the anchored stage's planes kernel, its window scan of the composed
 * planes, or all four; motifs_per_block = 0 restores the automatic split (chosen from the record length), n > 0 gives every
 * block n motifs (clamped to the number of motifs), a negative value is RIBBIT_E_ARG.  The output of every stage is the same
 * under every split. */
enum { RIBBIT_SCAN_PERFECT = 0, RIBBIT_SCAN_SUBST = 1, RIBBIT_SCAN_ANCHORED = 2, RIBBIT_SCAN_XA_WINDOW = 3, RIBBIT_SCAN_KERNELS = 4,
       RIBBIT_SCAN_ALL = 4 };
int ribbit_hip_debug_set_scan_split(RibbitHandle *h, int32_t kernel, int32_t motifs_per_block);
/* Test hook: the split one kernel (not RIBBIT_SCAN_ALL) last ran with on the loaded record: gridDim.y and the motifs per block;
 * both 0 when it has not run since the record was loaded. */
int ribbit_hip_debug_last_scan_split(RibbitHandle *h, int32_t kernel, int32_t *grid_y, int32_t *motifs_per_block);

/* Test hook: the window stages' merges run as independent position ranges on host threads (RIBBIT_THREADS, default
 * min(cores, 16)) wherever the call sequence can be cut; this sets the smallest number of calls per range (default 4096). */
void ribbit_debug_set_merge_min_range(size_t calls);
/* Test hook: what the last merge of a stage (0 substitution, 1 anchored) on the calling thread did: out = {ranges, ranges
 * merged again (after validation, or because their writes to list heads change an entry; low 16 bits) | ranges run again
 * behind a list-head change only because the changed entry lay within sight of their walks << 16, whole stage redone in order (0/1)
 * | range runs of the anchored stage's parallel passes, all passes together << 1,
 * list-head writes that changed an entry, first range empty (0/1) | parallel passes of the stage << 8}. */
void ribbit_debug_last_merge(int stage, int32_t out[5]);
/* Test hook: the anchored stage's merge runs its first parallel pass on the GPU for stages of 2^20 kept calls and more
 * (anchored_merge.hip: one lane per range of some 64 calls; environment RIBBIT_DEVICE_MERGE_MIN / RIBBIT_DEVICE_MERGE_RANGE change
 * the two numbers).  The ranges are put in the order of the work they are expected to be: the lanes take them from the light end,
 * and only those expected to need at most 6000 passes of a lane's loop; the host threads take ranges from the heavy end while the
 * kernel runs, until the two meet (api_merge.cpp, parallel_merge.h: AnchoredDevicePass).
 * out = {ranges the device merged, ranges it was given but left to the host threads (candidate lists beyond its scratch, budget of
 * passes), ranges the host threads merged meanwhile, ranges of the stage, ranges merged again by the validation walk} of the
 * calling thread's last anchored merge; the first three are zero when the device pass did not run. */
void ribbit_debug_last_device_merge(int32_t out[5]);

/* Test hook: the first parallel pass of the anchored stage's merge, alone, on lists, planes and calls the caller made.
 * perfect / subst: the two seed lists as they stand before the stage (types P and N in the perfect list, S, Q and N in the
 * substitution list: RIBBIT_E_ARG otherwise -- the reference retires a candidate in the list its TYPE names, so a seed typed for
 * the other list is never retired and its call starts again without end); calls: the full anchored call list in the
 * scanner's order, as ribbit_host_replay_calls takes it (the stage's length filter and cursor bounds apply); xa: the composed
 * planes of min_motif..max_motif, xa_stride words each (at least length / 32 + 1).  Every interval must lie in [0, length] and
 * every motif size in the handle-independent range of `params`: RIBBIT_E_ARG otherwise.
 * The ranges are cut and their start cursors computed as the production device pass prepares them, with knobs.calls_per_range
 * calls to a range.  knobs.where: RIBBIT_MERGE_ON_LANES -- the kernel, with no host thread taking ranges beside it (h: an open
 * handle; a loaded record stays usable, the call uploads into buffers of its own and the handle's merge buffers);
 * RIBBIT_MERGE_ON_HOST -- the host workers (h may be null: no GPU is touched).  Both start from the lists as given.
 * knobs: resident_waves, max_passes, head_cap (0: the production values), log_cap (0: the production formula), device_limit
 * (how many ranges, from the light end of the work order, the lanes may take; < 0: all), only_range (>= 0: only that range
 * runs; -1: all).
 * knobs.full == 0 (raw): stops after the pass.  out->ran: the pass ran at all (0: a log overflowed or the device declined; nothing
 * else but cuts, first and cursors0 is then filled); per range k < n_ranges: cuts[k], first[k] (.. first[n_ranges] = kept
 * calls), cursors0[2k..], and range[12 k ..] = {status (AM_* bits, all ones: not run), offset into own, entries in own (without
 * the sentinel), guard hits low / high, final cursor perfect / subst, head_reads[0] low / high, head_reads[1] low / high, 0};
 * undo / reads: 4 words {range, list (0 perfect, 1 substitution), index, old type / was live}; heads: 8 words {range, list,
 * index, start, end, motif size, type, changed_then}.  The lists are left as given.
 * knobs.full != 0: the stage goes on through the unchanged validation walk, the ranges done again, the join and the flush;
 * out->lists holds the three lists (dispatch empty) and the guard count, out->device_merge what ribbit_debug_last_device_merge
 * reports.
 * out->caps: the kernel's constants {AM_PS_CAP, AM_CAND_CAP, AM_PS_SPILL, AM_CAND_SPILL, AM_CHILD_CAP, AM_COV_CAP,
 * AM_RESIDENT_WAVES, AM_MAX_PASSES, AM_SCRATCH_FULL, AM_LOG_FULL, AM_BAD_PLANE, AM_RUNAWAY, AM_TOO_SLOW, 0, 0, 0}.
 * Release with ribbit_debug_merge_ranges_free. */
enum { RIBBIT_MERGE_ON_LANES = 0, RIBBIT_MERGE_ON_HOST = 1 };
typedef struct RibbitDebugMergeKnobs {
    int32_t where, full;
    int32_t calls_per_range, resident_waves, max_passes, head_cap;
    int64_t log_cap, device_limit, only_range;
} RibbitDebugMergeKnobs;
typedef struct RibbitDebugMergeRanges {
    int32_t ran, reserved;
    int32_t caps[16];
    size_t n_ranges;
    int32_t *cuts, *first, *cursors0, *range;
    RibbitSeed *own; size_t n_own;
    int32_t *undo; size_t n_undo;
    int32_t *reads; size_t n_reads;
    int32_t *heads; size_t n_heads;
    RibbitSeedLists lists;
    int32_t device_merge[5];
} RibbitDebugMergeRanges;
int ribbit_hip_debug_merge_ranges(RibbitHandle *h, const RibbitScanParams *params, int64_t length,
                                  const RibbitSeed *perfect, size_t n_perfect, const RibbitSeed *subst, size_t n_subst,
                                  const RibbitCall *calls, size_t n_calls, const uint32_t *xa, size_t xa_stride,
                                  const RibbitDebugMergeKnobs *knobs, RibbitDebugMergeRanges *out);
void ribbit_debug_merge_ranges_free(RibbitDebugMergeRanges *out);
/* Test hook: in how many independent ranges the calling thread's last dispatch merge (fasta_utils.cpp:187-224) ran; 1 = the
 * sequential merge (no cuts, or a list did not split cleanly at them). */
int32_t ribbit_debug_last_dispatch_ranges(void);
/* Test hook: faults in the teams of host threads the library runs its host stages on (process-wide; -1 turns a mode off).  From
 * the call on, in every team of two parts or more: with refuse_starts_from >= 0 the team's thread start number refuse_starts_from
 * (0 = its first) and every later one fail as a start the system refuses does -- the parts left over run on the calling thread and
 * the result is the same; with throw_in_part >= 0 that part throws std::bad_alloc before its work -- the entry point returns
 * RIBBIT_E_NOMEM with every thread joined.  Returns the number of faults injected since the previous call. */
int64_t ribbit_host_debug_thread_faults(int32_t refuse_starts_from, int32_t throw_in_part);

/* possibleMotifs (parse_smallmotif_seed.cpp:76-188) of every dispatched seed with m <= 10 that reaches it, computed
 * by one GPU launch (small_motifs.hip) -- what ribbit_hip_refine_jobs / ribbit_hip_refine_bed use for those seeds.
 * head: 4 ints per dispatched seed {first record, early reports, classes, flags}; flags != 0: the seed has no device
 * result (m > 10, filtered out by the continuous-ones threshold: -1; more than 64 classes or reports: 1; record arena
 * full: 2) and the library runs the host twin for it.  records: 4 words each {rotation class, first start, last end,
 * units}: a seed's early reports (already filtered by MINIMUM_LENGTH / PERFECT_UNITS, in the reference's push order),
 * then its classes with their final state: all of them in order of first appearance when two or more pass the filters
 * at the seed's end (the reference reports those in its unordered_map's iteration order, which every key determines),
 * otherwise only the one that passes, or none.  Valid until the next call on the handle. */
int ribbit_hip_small_motifs(RibbitHandle *h, const RibbitRefineParams *prm, const int32_t **head, size_t *n_seeds,
                            const uint32_t **records, size_t *n_records);
/* Test hook: the number of records the arena of ribbit_hip_small_motifs holds (0 = automatic: four per dispatched seed and 2^20
 * more).  A seed whose records no longer fit gets flags 2 and is computed by the host twin; the results are the same. */
int ribbit_hip_debug_set_small_record_capacity(RibbitHandle *h, size_t records);
/* Test hook: cumulative, process-wide: small-motif seeds that refinement took from the GPU's table / computed on the host. */
void ribbit_debug_small_motif_counters(int64_t out[2]);
/* Test hook: cumulative, process-wide: alignments refinement made / of them with the striped passes from the GPU / with the
 * path from the GPU (ribbit_hip_refine_bed batches them on the GPU for records with 400,000 dispatched seeds or more;
 * RIBBIT_GPU_SSW=0 / 1 forces it off / on). */
void ribbit_debug_alignment_counters(int64_t out[3]);
/* Test hook: cumulative, process-wide: {levels run, nodes put off, alignments of those nodes} of the level-by-level GPU
 * refinement of long-motif seeds' recursion trees (processSeed's recursion on the flanks, parse_seed.cpp:443-463: nodes of
 * RIBBIT_DEFER_MIN bases and more, default 700, are not refined where they are met but batched on the GPU, level by level). */
void ribbit_debug_level_counters(int64_t out[3]);

/* HIP events behind ribbit_hip_last_timing_ms are recorded by default; every record is a barrier packet between two
 * kernels of the stream (~6 us each on MI355X).  A caller that streams many records can switch them off per handle
 * (ribbit_hip_last_timing_ms then fails with RIBBIT_E_STATE for the pack / scan / GPU-side intervals). */
int ribbit_hip_set_timing(RibbitHandle *h, int32_t enabled);

/* Worker threads the host-side stages of this handle may use (window state machines, refinement);
 * 0 = default (environment RIBBIT_THREADS, else min(cores, 16)).  A caller that keeps several handles busy at
 * once -- ribbit-hip does, one per in-flight FASTA record (ribbit.cpp:269-280 processes them one by one) --
 * divides the cores among them with this. */
int ribbit_hip_set_host_threads(RibbitHandle *h, int32_t threads);

/* Page-lock a host buffer the caller owns (e.g. a shared-memory segment several ranks of one node write their
 * chunk's records into) so that ribbit_hip_scan_perfect_chunk can DMA straight into it.  hipHostRegister. */
int ribbit_hip_host_register(void *p, size_t bytes);
int ribbit_hip_host_unregister(void *p);

/* Words [word_lo, word_hi) of every composed plane XA_m (after the anchored stage's kernel ran),
 * motif-major, into out[(max_motif-min_motif+1) * (word_hi-word_lo)]. */
int ribbit_hip_xa_words(RibbitHandle *h, int64_t word_lo, int64_t word_hi, uint32_t *out);

/* Host-only: pair gathered perfect-stage events into runs (sorted by motif, start); *runs is malloc'ed
 * (release with ribbit_runs_free). */
int ribbit_host_perfect_runs_from_events(const RibbitScanParams *params, size_t nparts, const uint64_t *events,
                                         const uint64_t *counts, RibbitRun **runs, size_t *n);
void ribbit_runs_free(RibbitRun *runs);

/* Timing of the last call, milliseconds.  what: PACK the pack kernel, SCAN the last scan kernel, GPU the GPU side of
 * the last scan (kernel + pairing + state machine + sort + read-back), all by HIP events on the launch stream;
 * HOST everything after the pairing of the last window stage (device state machine, sort, read-back; wall clock);
 * MERGE the host merge of the last window stage (wall clock); SUBST_MERGE that of the substitution stage when
 * ribbit_hip_seeds_anchored ran both stages; SUBST_SCAN / ANCHORED_SCAN the scan kernel of the substitution / anchored stage
 * (HIP events; the anchored stage runs as two kernels, ANCHORED_SCAN is both); ANCHORED_PLANES / ANCHORED_WINDOW its planes
 * kernel (anchors + composition) / its window-scan kernel. */
enum { RIBBIT_TIME_PACK = 0, RIBBIT_TIME_SCAN = 1, RIBBIT_TIME_GPU = 2, RIBBIT_TIME_HOST = 3, RIBBIT_TIME_MERGE = 4, RIBBIT_TIME_SUBST_MERGE = 5,
       RIBBIT_TIME_SUBST_SCAN = 6, RIBBIT_TIME_ANCHORED_SCAN = 7, RIBBIT_TIME_ANCHORED_PLANES = 8, RIBBIT_TIME_ANCHORED_WINDOW = 9 };
int ribbit_hip_last_timing_ms(const RibbitHandle *h, int what, double *ms);
/* Profiling aid (no effect on results): streams `nbytes` of the loaded record's ASCII buffer /
 * planes through calib_stream_read_kernel so that a PMC pass contains a launch with a known byte
 * count in the scan kernels' access shape.  nbytes is clamped to what is resident. */
int ribbit_hip_debug_stream_read(RibbitHandle *h, int64_t nbytes, int64_t *bytes_read);

/* Number of raw device events (run starts + run ends) the last scan produced. */
int64_t ribbit_hip_last_event_count(const RibbitHandle *h);

#ifdef __cplusplus
}
#endif
#endif
