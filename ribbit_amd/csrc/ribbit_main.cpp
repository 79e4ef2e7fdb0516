// ribbit_main.cpp -- command-line front end with ribbit's surface (ribbit.cpp): same options, same
// defaults and quirks, FASTA in, BED out, the reference's progress lines on stderr.  Everything
// between reading a record and writing its BED rows goes through the C ABI of libribbit_hip.so.
//
//   ribbit-hip -i in.fa [-o out.bed] [-m 2] [-M 100] [-p 0.85] [-l N|file] [--min-units N|file] [--perfect-units N|file]
//              [--devices 0,1,...] [--jobs N] [--masked-fasta FILE [--mask soft|hard] [--mask-width N]]
//              [--repeat-fasta FILE [--flank N]] [--loci-bed FILE [--loci-gap D]] [--density-bedgraph FILE [--density-window W]]
//              [--overlap-with OTHER.bed [--overlap-bed FILE] [--overlap-summary FILE]] [--best-bed FILE]
//              [--class-bed FILE] [--motif-summary FILE] [--compound-bed FILE [--compound-gap D]]
//              [--interruption-bed FILE] [--purity-bed FILE]
//              [--overlap-with OTHER.bed [--nearest-bed FILE] [--nearest-other-bed FILE]]
//              [--composition-bed FILE [--composition-flank F]] [--composition-track FILE [--composition-window W]]
//              [--primer-bed FILE [--primer-flank F]]
//              [--primer-pair-bed FILE [--primer-pair-flank F]]
//              [--primer-product-bed FILE [--primer-product-flank F]]
//              [--primer-specific-bed FILE [--primer-specific-flank F]]
//
// Records are independent (ribbit.cpp:269-280 handles them one after the other); here up to --jobs of them are in
// flight at once PER GPU, each on its own handle / HIP streams, so that the upload and GPU scans of one record overlap
// the host merges and refinement of the others (long-read inputs: thousands of 10-100 kb records); with --devices the
// records are dealt over several GPUs, one handle set per device (partitioning by record: no halo, no
// exchange).  Output order is the input order.  The file is read by ribbit_fasta_* (block reads, line bodies copied once into page-locked buffers that
// the GPU uploads from asynchronously and refinement reads in place) instead of getline + string +=.
//
// --masked-fasta writes every record again with its BED rows masked (soft: lowercase, hard: N), on the GPU that refined it
// (ribbit_hip_mask_record), in input order beside the BED.  --repeat-fasta writes every BED row's bases with N flanking bases on
// either side (ribbit_hip_repeat_sequences), the same way.  --loci-bed writes the rows of every record merged into sorted loci
// (ribbit_hip_record_loci, ribbit_bed_loci_text) and --density-bedgraph the covered bases per window (ribbit_hip_record_density),
// the same way again.  --overlap-with reads a second BED file, grouped by record name before the first record is scanned, and
// --overlap-bed / --overlap-summary set every record's rows against its intervals of that file (ribbit_hip_record_overlap): the
// rows again with two columns more (ribbit_bed_overlap_text), and one line of counts per record.  --best-bed writes the rows of
// every record that ribbit_hip_record_best selects, a subset in which no two overlap and which covers the most bases, by ascending
// start (ribbit_bed_rows_text).  --class-bed and --motif-summary group every record's rows by the canonical class of their motif
// (ribbit_bed_motifs, ribbit_hip_record_classes): the rows again with class and strand behind them (ribbit_bed_class_text), and
// one line per class and record (ribbit_class_summary_text).  --compound-bed chains the rows of --best-bed's selection that lie at most
// --compound-gap bases apart (ribbit_hip_record_compounds) and writes one line per chain with its kind -- perfect, interrupted,
// compound -- and its structure, e.g. (CA)12n5(GA)8 (ribbit_class_labels, ribbit_compound_text); the selection and the classes are
// computed once per record, whichever outputs ask for them.  --interruption-bed and --purity-bed decode every row's CIGAR, column 11
// (ribbit_bed_cigars, ribbit_hip_record_interruptions): one line per run of substitutions and indels inside a row, with the bases
// the record has there (ribbit_interruption_text), and the rows again with their interruption counts and their longest
// uninterrupted stretch (ribbit_bed_purity_text); the column-4 motifs are parsed once per record for these and the class outputs.
// --nearest-bed and --nearest-other-bed name, for --overlap-with's file, which interval a row lies in or overlaps and which ones are
// its neighbours to either side, with their distances (ribbit_hip_record_nearest, once per direction): the rows again with eight
// columns more, the intervals by their column-4 labels (ribbit_bed_nearest_text), and one line per interval of the file with the
// rows in the intervals' place, named by their motifs (ribbit_nearest_other_text).  --composition-bed writes every row again with
// its A, C, G, T and other bases and, for --composition-flank bases on either side, the flank's length, C + G, other bases and the
// positions other rows cover (ribbit_hip_record_composition, ribbit_bed_composition_text); --composition-track writes the five
// counts per window, line for line beside --density-bedgraph's (ribbit_hip_record_base_windows, ribbit_base_windows_text); both
// read the bit planes the scans read, whose prefix counts are built once per record.  --primer-bed writes the rows of --best-bed's
// selection again, each with a forward primer in the --primer-flank bases to its left and a reverse primer in those to its right,
// chosen clear of every base that any row of the record covers or that is no A, C, G or T (ribbit_hip_record_primers,
// ribbit_bed_primers_text).  --primer-pair-bed writes the same rows with the two primers chosen together, from the best candidates of
// either flank that are clear of self-dimers and hairpins: the pair that is clear of cross-dimers, melts alike and has the least
// penalty, in --primer-pair-flank bases on either side (ribbit_hip_record_primer_pairs, ribbit_bed_primer_pairs_text).
// --primer-product-bed writes those rows and pairs, chosen in --primer-product-flank bases, with what each pair amplifies in its own
// record: the places on either strand where a primer's 3' end matches exactly and the rest nearly, and the products between two of
// them (ribbit_hip_record_primer_products, ribbit_bed_primer_products_text).
// --primer-specific-bed writes those rows, each with the best pair of --primer-specific-flank bases on either side that amplifies
// nothing else in its own record: all pairs of the two shortlists go through that in-silico PCR, the first specific one in the order
// of the choice is taken (ribbit_hip_record_specific_primer_pairs, ribbit_bed_primer_specific_text).
// --primer-genome-bed writes the same columns with every count and verdict taken over all records of the input.  It is the one
// output that needs the whole input twice: per record only the selected rows' lines and the targets' two shortlists are made, in
// --primer-genome-flank bases on either side (ribbit_hip_record_primer_shortlists), and kept in host memory in input order; after
// the last record the FASTA is read again, every record is loaded without a scan, all targets' pairs are judged on it
// (ribbit_hip_record_shortlist_verdicts, as home for the record's own targets), the judgements are summed
// (ribbit_primer_verdicts_merge), and then the pairs are chosen and written (ribbit_primer_shortlists_choose,
// ribbit_bed_primer_specific_text): write_primer_genome.
// --marker-fasta with --marker-bed types --primer-genome-bed's chosen pairs on a second assembly: the second pass keeps every
// record's chosen pairs and lines; a third pass reads the other FASTA, loads every record of it without a scan, places every pair's
// first product and measures the repeat tract inside it (ribbit_hip_record_pair_amplicons, the record's index as label), sums in
// record order (ribbit_pair_amplicons_merge) and writes the home records' rows in input order (ribbit_bed_marker_text):
// write_markers.  It is no row output of the table: it has two files and no text per record.
// --panel-bed, with both of them, pools the markers worth ordering (one product on the other assembly, of another size than
// designed) into multiplex PCR panels: a fourth pass on the same handle takes write_markers' amplicons and lines, makes the pools on
// the GPU with no record loaded (ribbit_hip_panel_pools) and writes the members' marker lines (ribbit_bed_panel_text): write_panel.
// --population-list with --allele-bed or --allele-matrix types the same chosen pairs on every sample of the list, one assembly after
// the other by the loop that --marker-bed's pass runs on its one (type_on_fasta), keeps one int32 per sample and pair
// (ribbit_pair_amplicon_sizes), counts every marker's alleles on the GPU in one call (ribbit_hip_marker_alleles) and writes the two
// texts (ribbit_bed_alleles_text, ribbit_allele_matrix_text): write_population, the last pass.
// The BED rows are read back once per record, however many of the twenty-one are asked for.
//
// These twenty-one are the ROW OUTPUTS, and each is described once, by its entry of kOutputs below: its file option, its stage (enum
// Stage, with the stage's names beside it), its qualifier options with their ranges and wording (defaults: Settings), and the function that
// makes one record's text from the record's rows.  Parsing, the "needs" checks, opening the files, the sinks of the pipelined
// records and of the last one, --timing and the RIBBIT_PROFILE line are loops over that table.  A twenty-second row output is: a stage in
// the enum and its names, the qualifiers' fields in Settings, a produce function, an entry of kOutputs, and its lines of kHelp.
//
// Reproduced quirks: -p is accepted and ignored (Q1); without -o the BED rows go to
// stderr (Q2); --help exits with status 1 (Q3); the record name ends at the first space and the last
// record is processed even when the file is empty (Q4).
#include <algorithm>
#include <array>
#include <atomic>
#include <cctype>
#include <charconv>
#include <chrono>
#include <condition_variable>
#include <deque>
#include <memory>
#include <mutex>
#include <sstream>
#include <thread>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <fstream>
#include <functional>
#include <iostream>
#include <map>
#include <string>
#include <vector>

#include "ribbit_hip.h"

namespace {

[[noreturn]] void die(const std::string &msg) {        // argument errors: main thread, before any worker exists
    std::cerr << "ribbit-hip: " << msg << "\n";
    std::exit(1);
}

// a failure of the GPU path inside the record pipeline: carried to main(), which lets the workers drain, closes the
// handles and returns 1 (exiting from a worker would run static destructors under live threads)
struct PathError { std::string what; };

void check(int rc) {
    if (rc != RIBBIT_OK) throw PathError{std::string("GPU path failed: ") + ribbit_hip_last_error()};
}

// The stages of a record: the six every record goes through, then one per row output, in the order of kOutputs.
enum Stage { LOAD, PERFECT, SUBSTITUTIONS, ANCHORED, DISPATCH, REFINE_BED, MASK, REPEATS, LOCI, DENSITY, OVERLAP, BEST, CLASSES, COMPOUND, INTERRUPTIONS, NEAREST, COMPOSITION, PRIMERS, PRIMER_PAIRS, PRIMER_PRODUCTS, PRIMER_SPECIFIC, PRIMER_GENOME, MARKERS, PANEL, POPULATION, N_STAGES };
constexpr int N_FIXED_STAGES = MASK;
// a stage's key in --timing's stage_ms_summed_over_records and its label in the RIBBIT_PROFILE line
const struct { const char *key, *label; } kStageNames[N_STAGES] = {
    {"load", "load"}, {"perfect", "perfect"}, {"substitutions", "substitutions"}, {"anchored", "anchored"}, {"dispatch", "dispatch"},
    {"refine_and_bed", "refine+BED"}, {"mask", "mask"}, {"repeats", "repeats"}, {"loci", "loci"}, {"density", "density"}, {"overlap", "overlap"},
    {"best", "best"}, {"classes", "classes"}, {"compound", "compound"}, {"interruptions", "interruptions"}, {"nearest", "nearest"}, {"composition", "composition"}, {"primers", "primers"},
    {"primer_pairs", "primer_pairs"}, {"primer_products", "primer_products"}, {"primer_specific", "primer_specific"}, {"primer_genome", "primer_genome"}, {"markers", "markers"}, {"panel", "panel"}, {"population", "population"}};

// wall time per stage, summed over the records (--timing, RIBBIT_PROFILE=1)
double g_stage_ms[N_STAGES] = {};
std::mutex g_stage_mu;
struct StageClock {
    Stage stage;
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    explicit StageClock(Stage s) : stage(s) {}
    ~StageClock() {
        const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        std::lock_guard<std::mutex> lk(g_stage_mu);
        g_stage_ms[stage] += ms;
    }
};

// ---- the row outputs: what is written from a record's BED rows beside the BED itself
// where an output's text for one record goes: the record's string of the pipeline, or the file itself for the last record
using Sink = std::function<void(const char *, size_t)>;

// --overlap-with: the intervals of a second BED file by record name, each with its column-4 label, and which names have been a
// record of the input
struct OtherBed {
    struct Group {
        std::vector<int32_t> iv;                 // (start, end) per interval, in file order
        std::string labels;                      // the intervals' labels one behind the other ...
        std::vector<int32_t> label_at{0};        // ... label j at [label_at[j], label_at[j + 1])
        bool is_record = false;
        size_t n() const { return iv.size() / 2; }
    };
    std::map<std::string, Group> by_name;
    const Group *of(const std::string &name) const {
        const auto it = by_name.find(name);
        return it == by_name.end() ? nullptr : &it->second;
    }
};

// what the outputs of one record share: the record and its rows in BED order, read back once for all of them
struct RecordRows {
    const std::string &name;
    int64_t length;
    std::vector<int32_t> iv;             // (start, end) per row
    const char *bed_text;                // the record's BED text, row i on line i (handle-owned: valid until the handle's next refinement) ...
    size_t bed_len;
    std::string bed_copy;                // ... or this copy of it, when it came in slices and an output quotes it
    const OtherBed::Group *other;        // the record's intervals of --overlap-with with their labels (null: none)
    // the column-4 motifs of the BED text (owned here), parsed by the first output that asks (motifs_of): the class outputs, the
    // interruption outputs and --nearest-other-bed
    struct Motifs {
        bool have = false;
        char *pool = nullptr;
        int32_t *offsets = nullptr;
        Motifs() = default;
        Motifs(const Motifs &) = delete;
        Motifs &operator=(const Motifs &) = delete;
        ~Motifs() { ribbit_text_free(pool); ribbit_intervals_free(offsets); }
    };
    mutable Motifs motifs;
    // the record's rows by motif class, computed by the first of the outputs that asks (classes_of): the handle's result, which
    // stays valid while the record's outputs are produced
    struct Classes {
        bool have = false;
        const char *motifs = nullptr;        // (RecordRows::motifs')
        const int32_t *offsets = nullptr;
        const char *classes = nullptr, *strands = nullptr;
        const RibbitMotifClass *groups = nullptr;
        size_t n_groups = 0;
    };
    mutable Classes by_class;
    // the record's best non-overlapping rows, computed by the first of the four outputs that asks (best_of): the handle's result,
    // which stays valid while the record's outputs are produced
    struct Best {
        bool have = false;
        const int32_t *chosen = nullptr;
        size_t n = 0;
    };
    mutable Best best;
    // the record's CIGARs decoded, computed by the first of the two outputs that asks (interruptions_of): the CIGARs of the BED text
    // and the motifs' lengths (owned here) and the handle's result, which stays valid while the record's outputs are produced
    struct Interruptions {
        bool have = false;
        char *cigars = nullptr;
        int32_t *offsets = nullptr;
        std::vector<int32_t> motif_lengths;
        const RibbitRowPurity *rows = nullptr;
        const RibbitInterruption *sites = nullptr;
        size_t n_sites = 0;
        const char *observed = nullptr;
        const int32_t *observed_offsets = nullptr;
        Interruptions() = default;
        Interruptions(const Interruptions &) = delete;
        Interruptions &operator=(const Interruptions &) = delete;
        ~Interruptions() { ribbit_text_free(cigars); ribbit_intervals_free(offsets); }
    };
    mutable Interruptions decoded;
    size_t n() const { return iv.size() / 2; }
};

// the qualifiers' values and their defaults
struct Settings {
    int mask_mode = RIBBIT_MASK_SOFT;    // --mask soft|hard
    int mask_width = 60;                 // --mask-width N: bases per line, 0 = one line per record
    int flank = 100;                     // --flank N: bases on either side of a row
    int loci_gap = 0;                    // --loci-gap D: runs at most D bases apart are one locus
    int density_window = 10000;          // --density-window W
    int compound_gap = 100;              // --compound-gap D: rows at most D bases behind what came before them are one chain (MISA's default)
    int composition_flank = 100;         // --composition-flank F: bases on either side of a row
    int composition_window = 10000;      // --composition-window W
    int primer_flank = 200;              // --primer-flank F: bases on either side of a row that a primer may lie in
    int primer_pair_flank = 200;         // --primer-pair-flank F: the same for --primer-pair-bed
    int primer_product_flank = 200;      // --primer-product-flank F: the same for --primer-product-bed
    int primer_specific_flank = 200;     // --primer-specific-flank F: the same for --primer-specific-bed
    int primer_genome_flank = 200;       // --primer-genome-flank F: the same for --primer-genome-bed
    const OtherBed *other = nullptr;         // --overlap-with FILE, read and grouped by name
};

// --name VALUE: a whole number of bases in [lo, hi] of at most max_digits digits (`range`: how the message puts that), or soft|hard
struct Qualifier {
    const char *name;
    enum Kind { BASES, SOFT_HARD } kind;
    int64_t lo, hi;
    size_t max_digits;
    const char *range;
    int Settings::*field;
};
constexpr size_t MAX_QUALIFIERS = 2;

void produce_masked(RibbitHandle *h, const RecordRows &r, const Settings &s, const Sink &write) {      // the header and the masked body
    const char *body = nullptr;
    size_t body_len = 0;
    { StageClock c(MASK); check(ribbit_hip_mask_record(h, r.iv.data(), r.n(), s.mask_mode, s.mask_width, &body, &body_len)); }
    const std::string header = ">" + r.name + "\n";
    write(header.data(), header.size());
    write(body, body_len);
}

void produce_repeats(RibbitHandle *h, const RecordRows &r, const Settings &s, const Sink &write) {
    // in batches of the handle's text budget, each written before the next call reuses the text
    for (size_t done = 0, k = 0; done < r.n(); done += k) {
        const char *text = nullptr;
        size_t len = 0;
        { StageClock c(REPEATS); check(ribbit_hip_repeat_sequences(h, r.name.c_str(), r.iv.data() + 2 * done, r.n() - done, s.flank, &text, &len, &k)); }
        write(text, len);
    }
}

void produce_loci(RibbitHandle *h, const RecordRows &r, const Settings &s, const Sink &write) {
    const RibbitLocus *loci = nullptr;
    size_t n_loci = 0;
    char *text = nullptr;
    size_t len = 0;
    StageClock c(LOCI);
    check(ribbit_hip_record_loci(h, r.iv.data(), r.n(), s.loci_gap, &loci, &n_loci));
    check(ribbit_bed_loci_text(r.name.c_str(), r.bed_text, r.bed_len, loci, n_loci, &text, &len));
    write(text, len);
    ribbit_text_free(text);
}

void produce_density(RibbitHandle *h, const RecordRows &r, const Settings &s, const Sink &write) {
    const int32_t *covered = nullptr;
    size_t n_windows = 0;
    StageClock c(DENSITY);
    check(ribbit_hip_record_density(h, r.iv.data(), r.n(), s.density_window, &covered, &n_windows));
    std::string lines;
    char num[24];
    auto put = [&](int64_t v, char sep) { lines.append(num, (size_t)(std::to_chars(num, num + sizeof num, v).ptr - num)); lines += sep; };
    for (size_t k = 0; k < n_windows; ++k) {
        const int64_t from = (int64_t)k * s.density_window;
        lines += r.name;
        lines += '\t';
        put(from, '\t');
        put(std::min<int64_t>(from + s.density_window, r.length), '\t');
        put(covered[k], '\n');
        if (lines.size() > ((size_t)1 << 20)) { write(lines.data(), lines.size()); lines.clear(); }
    }
    write(lines.data(), lines.size());
}

// both overlap outputs of a record: the second call finds what the first left on the handle and gives the GPU nothing to do
const int32_t *overlap_of(RibbitHandle *h, const RecordRows &r, RibbitOverlapTotals *totals) {
    static const std::vector<int32_t> kNone;
    const std::vector<int32_t> &other = r.other ? r.other->iv : kNone;
    const int32_t *per_row = nullptr;
    check(ribbit_hip_record_overlap(h, r.iv.data(), r.n(), other.data(), other.size() / 2, &per_row, totals));
    return per_row;
}

void produce_overlap_bed(RibbitHandle *h, const RecordRows &r, const Settings &, const Sink &write) {
    RibbitOverlapTotals totals;
    char *text = nullptr;
    size_t len = 0;
    StageClock c(OVERLAP);
    const int32_t *per_row = overlap_of(h, r, &totals);
    check(ribbit_bed_overlap_text(r.bed_text, r.bed_len, per_row, r.n(), &text, &len));
    write(text, len);
    ribbit_text_free(text);
}

void produce_overlap_summary(RibbitHandle *h, const RecordRows &r, const Settings &, const Sink &write) {
    RibbitOverlapTotals t;
    StageClock c(OVERLAP);
    overlap_of(h, r, &t);
    std::string line = r.name;
    char num[24];
    for (const int64_t v : {r.length, (int64_t)t.rows, (int64_t)t.rows_hit, (int64_t)t.other, (int64_t)t.other_hit, t.rows_bases, t.other_bases, t.both_bases}) {
        line += '\t';
        line.append(num, (size_t)(std::to_chars(num, num + sizeof num, v).ptr - num));
    }
    line += '\n';
    write(line.data(), line.size());
}

// the selection of a record, for --best-bed, --compound-bed, --primer-bed, --primer-pair-bed, --primer-product-bed and --primer-specific-bed: a later call finds what the first left in the record's rows
const RecordRows::Best &best_of(RibbitHandle *h, const RecordRows &r) {
    RecordRows::Best &b = r.best;
    if (b.have) return b;
    int64_t bases = 0;
    check(ribbit_hip_record_best(h, r.iv.data(), r.n(), &b.chosen, &b.n, &bases));
    b.have = true;
    return b;
}

void produce_best(RibbitHandle *h, const RecordRows &r, const Settings &, const Sink &write) {
    char *text = nullptr;
    size_t len = 0;
    StageClock c(BEST);
    const RecordRows::Best &b = best_of(h, r);
    check(ribbit_bed_rows_text(r.bed_text, r.bed_len, b.chosen, b.n, &text, &len));
    write(text, len);
    ribbit_text_free(text);
}

// the column-4 motifs of a record's rows: the second call finds what the first left in the record's rows
const RecordRows::Motifs &motifs_of(const RecordRows &r) {
    RecordRows::Motifs &m = r.motifs;
    if (m.have) return m;
    size_t n = 0;
    check(ribbit_bed_motifs(r.bed_text, r.bed_len, &m.pool, &m.offsets, &n));
    if (n != r.n()) throw PathError{"the BED text has " + std::to_string(n) + " motifs for " + std::to_string(r.n()) + " rows"};
    m.have = true;
    return m;
}

// both class outputs of a record: the second call finds what the first left in the record's rows
const RecordRows::Classes &classes_of(RibbitHandle *h, const RecordRows &r) {
    RecordRows::Classes &c = r.by_class;
    if (c.have) return c;
    const RecordRows::Motifs &m = motifs_of(r);
    c.motifs = m.pool;
    c.offsets = m.offsets;
    check(ribbit_hip_record_classes(h, r.iv.data(), r.n(), c.motifs, c.offsets, &c.classes, &c.strands, &c.groups, &c.n_groups));
    c.have = true;
    return c;
}

void produce_class_bed(RibbitHandle *h, const RecordRows &r, const Settings &, const Sink &write) {
    char *text = nullptr;
    size_t len = 0;
    StageClock c(CLASSES);
    const RecordRows::Classes &k = classes_of(h, r);
    check(ribbit_bed_class_text(r.bed_text, r.bed_len, k.classes, k.offsets, k.strands, r.n(), &text, &len));
    write(text, len);
    ribbit_text_free(text);
}

void produce_motif_summary(RibbitHandle *h, const RecordRows &r, const Settings &, const Sink &write) {
    char *text = nullptr;
    size_t len = 0;
    StageClock c(CLASSES);
    const RecordRows::Classes &k = classes_of(h, r);
    check(ribbit_class_summary_text(r.name.c_str(), r.iv.data(), r.n(), k.classes, k.offsets, k.groups, k.n_groups, &text, &len));
    write(text, len);
    ribbit_text_free(text);
}

// the selected rows with the labels of their motif classes, chained; the chains' lines quote the selected rows' lines
void produce_compound(RibbitHandle *h, const RecordRows &r, const Settings &s, const Sink &write) {
    StageClock c(COMPOUND);
    const RecordRows::Best &b = best_of(h, r);
    const RecordRows::Classes &k = classes_of(h, r);
    int32_t *labels = nullptr;
    check(ribbit_class_labels(k.classes, k.offsets, r.n(), k.groups, k.n_groups, &labels));
    std::vector<int32_t> iv(2 * b.n), label(b.n);
    for (size_t j = 0; j < b.n; ++j) {
        const size_t row = (size_t)b.chosen[j];
        iv[2 * j] = r.iv[2 * row];
        iv[2 * j + 1] = r.iv[2 * row + 1];
        label[j] = labels[row];
    }
    ribbit_intervals_free(labels);
    char *lines = nullptr, *text = nullptr;
    size_t lines_len = 0, len = 0, n_chains = 0, n_members = 0;
    const RibbitCompound *chains = nullptr;
    const int32_t *members = nullptr;
    check(ribbit_bed_rows_text(r.bed_text, r.bed_len, b.chosen, b.n, &lines, &lines_len));
    int rc = ribbit_hip_record_compounds(h, iv.data(), label.data(), b.n, s.compound_gap, &chains, &n_chains, &members, &n_members);
    if (rc == RIBBIT_OK) rc = ribbit_compound_text(r.name.c_str(), lines, lines_len, r.length, iv.data(), b.n, chains, n_chains, members, n_members, &text, &len);
    ribbit_text_free(lines);
    check(rc);
    write(text, len);
    ribbit_text_free(text);
}

// both interruption outputs of a record: the second call finds what the first left in the record's rows
const RecordRows::Interruptions &interruptions_of(RibbitHandle *h, const RecordRows &r) {
    RecordRows::Interruptions &d = r.decoded;
    if (d.have) return d;
    const RecordRows::Motifs &m = motifs_of(r);
    d.motif_lengths.resize(r.n());
    for (size_t i = 0; i < r.n(); ++i) d.motif_lengths[i] = m.offsets[i + 1] - m.offsets[i];
    size_t n = 0;
    check(ribbit_bed_cigars(r.bed_text, r.bed_len, &d.cigars, &d.offsets, &n));
    if (n != r.n()) throw PathError{"the BED text has " + std::to_string(n) + " CIGARs for " + std::to_string(r.n()) + " rows"};
    check(ribbit_hip_record_interruptions(h, r.iv.data(), d.motif_lengths.data(), n, d.cigars, d.offsets, &d.rows, &d.sites, &d.n_sites, &d.observed,
                                          &d.observed_offsets));
    d.have = true;
    return d;
}

// rows whose CIGAR does not span them, over all records: their interruptions are not in --interruption-bed
std::atomic<size_t> g_rows_left_out{0};

void produce_interruption_bed(RibbitHandle *h, const RecordRows &r, const Settings &, const Sink &write) {
    char *text = nullptr;
    size_t len = 0, left_out = 0;
    StageClock c(INTERRUPTIONS);
    const RecordRows::Interruptions &d = interruptions_of(h, r);
    check(ribbit_interruption_text(r.name.c_str(), r.bed_text, r.bed_len, r.iv.data(), r.n(), d.rows, d.sites, d.n_sites, d.cigars, d.observed, d.observed_offsets,
                                   &text, &len, &left_out));
    g_rows_left_out += left_out;
    write(text, len);
    ribbit_text_free(text);
}

void produce_purity_bed(RibbitHandle *h, const RecordRows &r, const Settings &, const Sink &write) {
    char *text = nullptr;
    size_t len = 0;
    StageClock c(INTERRUPTIONS);
    const RecordRows::Interruptions &d = interruptions_of(h, r);
    check(ribbit_bed_purity_text(r.bed_text, r.bed_len, r.iv.data(), d.motif_lengths.data(), d.rows, r.n(), &text, &len));
    write(text, len);
    ribbit_text_free(text);
}

// the record's intervals of --overlap-with, or a group without any
const OtherBed::Group &other_of(const RecordRows &r) {
    static const OtherBed::Group kNone;
    return r.other ? *r.other : kNone;
}

// the rows as queries against the file's intervals: every row again, with what is nearest to it
void produce_nearest_bed(RibbitHandle *h, const RecordRows &r, const Settings &, const Sink &write) {
    const OtherBed::Group &other = other_of(r);
    const RibbitNearest *nearest = nullptr;
    char *text = nullptr;
    size_t len = 0;
    StageClock c(NEAREST);
    check(ribbit_hip_record_nearest(h, r.iv.data(), r.n(), other.iv.data(), other.n(), &nearest));
    check(ribbit_bed_nearest_text(r.bed_text, r.bed_len, nearest, r.n(), other.iv.data(), other.labels.c_str(), other.label_at.data(), other.n(), &text, &len));
    write(text, len);
    ribbit_text_free(text);
}

// the file's intervals as queries against the rows: one line per interval of this record, none for a record without any
void produce_nearest_other(RibbitHandle *h, const RecordRows &r, const Settings &, const Sink &write) {
    const OtherBed::Group &other = other_of(r);
    if (other.n() == 0) return;
    const RibbitNearest *nearest = nullptr;
    char *text = nullptr;
    size_t len = 0;
    StageClock c(NEAREST);
    const RecordRows::Motifs &m = motifs_of(r);
    check(ribbit_hip_record_nearest(h, other.iv.data(), other.n(), r.iv.data(), r.n(), &nearest));
    check(ribbit_nearest_other_text(r.name.c_str(), other.iv.data(), other.labels.c_str(), other.label_at.data(), other.n(), nearest, r.iv.data(), m.pool, m.offsets,
                                    r.n(), &text, &len));
    write(text, len);
    ribbit_text_free(text);
}

// every row again, with what its bases and its flanks' bases are
void produce_composition_bed(RibbitHandle *h, const RecordRows &r, const Settings &s, const Sink &write) {
    const RibbitRowComposition *rows = nullptr;
    char *text = nullptr;
    size_t len = 0;
    StageClock c(COMPOSITION);
    check(ribbit_hip_record_composition(h, r.iv.data(), r.n(), s.composition_flank, &rows));
    check(ribbit_bed_composition_text(r.bed_text, r.bed_len, rows, r.n(), &text, &len));
    write(text, len);
    ribbit_text_free(text);
}

// one line per window of the record, as --density-bedgraph has them
void produce_composition_track(RibbitHandle *h, const RecordRows &r, const Settings &s, const Sink &write) {
    const RibbitBaseCounts *windows = nullptr;
    char *text = nullptr;
    size_t n_windows = 0, len = 0;
    StageClock c(COMPOSITION);
    check(ribbit_hip_record_base_windows(h, s.composition_window, &windows, &n_windows));
    check(ribbit_base_windows_text(r.name.c_str(), r.length, s.composition_window, windows, n_windows, &text, &len));
    write(text, len);
    ribbit_text_free(text);
}

// the selected rows as targets: (start, end) of every chosen row
std::vector<int32_t> targets_of(const RecordRows &r, const RecordRows::Best &b) {
    std::vector<int32_t> targets(2 * b.n);
    for (size_t j = 0; j < b.n; ++j) {
        const size_t row = (size_t)b.chosen[j];
        targets[2 * j] = r.iv[2 * row];
        targets[2 * j + 1] = r.iv[2 * row + 1];
    }
    return targets;
}

// the selected rows again, each with a primer in either flank, clear of all rows of the record
void produce_primers(RibbitHandle *h, const RecordRows &r, const Settings &s, const Sink &write) {
    StageClock c(PRIMERS);
    const RecordRows::Best &b = best_of(h, r);
    const std::vector<int32_t> targets = targets_of(r, b);
    RibbitPrimerParams prm;
    ribbit_primer_params_default(&prm);
    prm.flank = s.primer_flank;
    char *lines = nullptr, *text = nullptr;
    size_t lines_len = 0, len = 0;
    const RibbitRowPrimers *primers = nullptr;
    check(ribbit_bed_rows_text(r.bed_text, r.bed_len, b.chosen, b.n, &lines, &lines_len));
    int rc = ribbit_hip_record_primers(h, r.iv.data(), r.n(), targets.data(), b.n, &prm, &primers);
    if (rc == RIBBIT_OK) rc = ribbit_bed_primers_text(lines, lines_len, primers, b.n, &text, &len);
    ribbit_text_free(lines);
    check(rc);
    write(text, len);
    ribbit_text_free(text);
}

// the selected rows again, each with its two primers chosen as a pair and checked for dimers and hairpins
void produce_primer_pairs(RibbitHandle *h, const RecordRows &r, const Settings &s, const Sink &write) {
    StageClock c(PRIMER_PAIRS);
    const RecordRows::Best &b = best_of(h, r);
    const std::vector<int32_t> targets = targets_of(r, b);
    RibbitPrimerParams prm;
    ribbit_primer_params_default(&prm);
    prm.flank = s.primer_pair_flank;
    RibbitPrimerPairParams pair;
    ribbit_primer_pair_params_default(&pair);
    char *lines = nullptr, *text = nullptr;
    size_t lines_len = 0, len = 0;
    const RibbitRowPrimerPair *pairs = nullptr;
    check(ribbit_bed_rows_text(r.bed_text, r.bed_len, b.chosen, b.n, &lines, &lines_len));
    int rc = ribbit_hip_record_primer_pairs(h, r.iv.data(), r.n(), targets.data(), b.n, &prm, &pair, &pairs);
    if (rc == RIBBIT_OK) rc = ribbit_bed_primer_pairs_text(lines, lines_len, pairs, b.n, &text, &len);
    ribbit_text_free(lines);
    check(rc);
    write(text, len);
    ribbit_text_free(text);
}

// the selected rows with their pairs again, chosen at this output's own flank, and what each pair amplifies in the record
void produce_primer_products(RibbitHandle *h, const RecordRows &r, const Settings &s, const Sink &write) {
    StageClock c(PRIMER_PRODUCTS);
    const RecordRows::Best &b = best_of(h, r);
    const std::vector<int32_t> targets = targets_of(r, b);
    RibbitPrimerParams prm;
    ribbit_primer_params_default(&prm);
    prm.flank = s.primer_product_flank;
    RibbitPrimerPairParams pair;
    ribbit_primer_pair_params_default(&pair);
    RibbitProductParams product;
    ribbit_product_params_default(&product);
    char *lines = nullptr, *text = nullptr;
    size_t lines_len = 0, len = 0;
    const RibbitRowPrimerPair *pairs = nullptr;
    const RibbitRowProducts *products = nullptr;
    check(ribbit_bed_rows_text(r.bed_text, r.bed_len, b.chosen, b.n, &lines, &lines_len));
    int rc = ribbit_hip_record_primer_pairs(h, r.iv.data(), r.n(), targets.data(), b.n, &prm, &pair, &pairs);
    if (rc == RIBBIT_OK) rc = ribbit_hip_record_primer_products(h, pairs, b.n, &product, &products);
    if (rc == RIBBIT_OK) rc = ribbit_bed_primer_products_text(lines, lines_len, pairs, products, b.n, &text, &len);
    ribbit_text_free(lines);
    check(rc);
    write(text, len);
    ribbit_text_free(text);
}

// the selected rows again, each with the best pair of its two shortlists that amplifies nothing else in the record
void produce_primer_specific(RibbitHandle *h, const RecordRows &r, const Settings &s, const Sink &write) {
    StageClock c(PRIMER_SPECIFIC);
    const RecordRows::Best &b = best_of(h, r);
    const std::vector<int32_t> targets = targets_of(r, b);
    RibbitPrimerParams prm;
    ribbit_primer_params_default(&prm);
    prm.flank = s.primer_specific_flank;
    RibbitPrimerPairParams pair;
    ribbit_primer_pair_params_default(&pair);
    RibbitProductParams product;
    ribbit_product_params_default(&product);
    char *lines = nullptr, *text = nullptr;
    size_t lines_len = 0, len = 0;
    const RibbitRowPrimerPair *pairs = nullptr;
    const RibbitRowProducts *products = nullptr;
    const RibbitRowSpecific *specific = nullptr;
    check(ribbit_bed_rows_text(r.bed_text, r.bed_len, b.chosen, b.n, &lines, &lines_len));
    int rc = ribbit_hip_record_specific_primer_pairs(h, r.iv.data(), r.n(), targets.data(), b.n, &prm, &pair, &product, &pairs, &products, &specific);
    if (rc == RIBBIT_OK) rc = ribbit_bed_primer_specific_text(lines, lines_len, pairs, products, specific, b.n, &text, &len);
    ribbit_text_free(lines);
    check(rc);
    write(text, len);
    ribbit_text_free(text);
}

// The first pass of --primer-genome-bed over one record: nothing for the file yet.  What goes to the sink is the record's state for the
// second pass (write_primer_genome), which travels in input order as the other outputs' texts do: the number of targets and the
// length of their BED lines (two 64-bit words), the targets' RibbitTargetShortlists, the lines.
void produce_primer_genome(RibbitHandle *h, const RecordRows &r, const Settings &s, const Sink &write) {
    StageClock c(PRIMER_GENOME);
    const RecordRows::Best &b = best_of(h, r);
    const std::vector<int32_t> targets = targets_of(r, b);
    RibbitPrimerParams prm;
    ribbit_primer_params_default(&prm);
    prm.flank = s.primer_genome_flank;
    RibbitPrimerPairParams pair;
    ribbit_primer_pair_params_default(&pair);
    char *lines = nullptr;
    size_t lines_len = 0;
    const RibbitTargetShortlists *lists = nullptr;
    check(ribbit_bed_rows_text(r.bed_text, r.bed_len, b.chosen, b.n, &lines, &lines_len));
    const int rc = ribbit_hip_record_primer_shortlists(h, r.iv.data(), r.n(), targets.data(), b.n, &prm, &pair, &lists);
    if (rc == RIBBIT_OK) {
        const uint64_t head[2] = {(uint64_t)b.n, (uint64_t)lines_len};
        write(reinterpret_cast<const char *>(head), sizeof head);
        write(reinterpret_cast<const char *>(lists), b.n * sizeof(RibbitTargetShortlists));
        write(lines, lines_len);
    }
    ribbit_text_free(lines);
    check(rc);
}

// One entry per row output.  The order is the order of everything that is done for all of them: the "needs" checks, opening the
// files (binary), producing a record's texts, the keys of --timing.
struct Output {
    const char *option;                      // --option FILE
    Stage stage;
    bool quotes_bed;                         // its lines quote the rows' lines or their motifs: it needs RecordRows::bed_text
    void (*produce)(RibbitHandle *, const RecordRows &, const Settings &, const Sink &);      // one record's text for this output
    Qualifier qualifiers[MAX_QUALIFIERS];    // (name null: none)
    bool needs_other;                        // it compares the rows with the intervals of --overlap-with
};
constexpr size_t N_OUTPUTS = 21;
const Output kOutputs[N_OUTPUTS] = {
    {"masked-fasta", MASK, false, produce_masked,
     {{"mask", Qualifier::SOFT_HARD, 0, 0, 0, nullptr, &Settings::mask_mode},
      {"mask-width", Qualifier::BASES, 0, 999999999, 9, "0 or more", &Settings::mask_width}}, false},
    {"repeat-fasta", REPEATS, false, produce_repeats,
     {{"flank", Qualifier::BASES, 0, 999999999, 9, "0 or more, at most 9 digits", &Settings::flank}, {}}, false},
    {"loci-bed", LOCI, true, produce_loci,
     {{"loci-gap", Qualifier::BASES, 0, 2147483647, 10, "0 .. 2147483647", &Settings::loci_gap}, {}}, false},
    {"density-bedgraph", DENSITY, false, produce_density,
     {{"density-window", Qualifier::BASES, 1, 2147483647, 10, "1 .. 2147483647", &Settings::density_window}, {}}, false},
    {"overlap-bed", OVERLAP, true, produce_overlap_bed, {{}, {}}, true},
    {"overlap-summary", OVERLAP, false, produce_overlap_summary, {{}, {}}, true},
    {"best-bed", BEST, true, produce_best, {{}, {}}, false},
    {"class-bed", CLASSES, true, produce_class_bed, {{}, {}}, false},
    {"motif-summary", CLASSES, true, produce_motif_summary, {{}, {}}, false},
    {"compound-bed", COMPOUND, true, produce_compound,
     {{"compound-gap", Qualifier::BASES, 0, 2147483647, 10, "0 .. 2147483647", &Settings::compound_gap}, {}}, false},
    {"interruption-bed", INTERRUPTIONS, true, produce_interruption_bed, {{}, {}}, false},
    {"purity-bed", INTERRUPTIONS, true, produce_purity_bed, {{}, {}}, false},
    {"nearest-bed", NEAREST, true, produce_nearest_bed, {{}, {}}, true},
    {"nearest-other-bed", NEAREST, true, produce_nearest_other, {{}, {}}, true},
    {"composition-bed", COMPOSITION, true, produce_composition_bed,
     {{"composition-flank", Qualifier::BASES, 0, 999999999, 9, "0 or more, at most 9 digits", &Settings::composition_flank}, {}}, false},
    {"composition-track", COMPOSITION, false, produce_composition_track,
     {{"composition-window", Qualifier::BASES, 1, 2147483647, 10, "1 .. 2147483647", &Settings::composition_window}, {}}, false},
    {"primer-bed", PRIMERS, true, produce_primers,
     {{"primer-flank", Qualifier::BASES, 0, RIBBIT_PRIMER_MAX_FLANK, 4, "0 .. 1000", &Settings::primer_flank}, {}}, false},
    {"primer-pair-bed", PRIMER_PAIRS, true, produce_primer_pairs,
     {{"primer-pair-flank", Qualifier::BASES, 0, RIBBIT_PRIMER_MAX_FLANK, 4, "0 .. 1000", &Settings::primer_pair_flank}, {}}, false},
    {"primer-product-bed", PRIMER_PRODUCTS, true, produce_primer_products,
     {{"primer-product-flank", Qualifier::BASES, 0, RIBBIT_PRIMER_MAX_FLANK, 4, "0 .. 1000", &Settings::primer_product_flank}, {}}, false},
    {"primer-specific-bed", PRIMER_SPECIFIC, true, produce_primer_specific,
     {{"primer-specific-flank", Qualifier::BASES, 0, RIBBIT_PRIMER_MAX_FLANK, 4, "0 .. 1000", &Settings::primer_specific_flank}, {}}, false},
    {"primer-genome-bed", PRIMER_GENOME, true, produce_primer_genome,
     {{"primer-genome-flank", Qualifier::BASES, 0, RIBBIT_PRIMER_MAX_FLANK, 4, "0 .. 1000", &Settings::primer_genome_flank}, {}}, false}};
static_assert(RIBBIT_PRIMER_MAX_FLANK == 1000, "the range as --primer-flank's, --primer-pair-flank's, --primer-product-flank's, --primer-specific-flank's and --primer-genome-flank's messages and help put it");
// --primer-genome-bed: what its produce function hands to the sink is not text for the file but the record's state for the second pass
constexpr size_t GENOME_OUTPUT = N_OUTPUTS - 1;

// the row outputs that are on, by stage: an output whose stage an earlier one has already named is left out (--timing, RIBBIT_PROFILE)
std::vector<Stage> stages_on(const std::array<bool, N_OUTPUTS> &on) {
    std::vector<Stage> stages;
    for (size_t k = 0; k < N_OUTPUTS; ++k)
        if (on[k] && std::find(stages.begin(), stages.end(), kOutputs[k].stage) == stages.end()) stages.push_back(kOutputs[k].stage);
    return stages;
}

// which outputs are on for one record, and where each one's text goes (an empty sink: off)
struct RowJobs {
    std::array<Sink, N_OUTPUTS> sink;
    template <typename Make>
    RowJobs(const std::array<bool, N_OUTPUTS> &on, Make make) {
        for (size_t k = 0; k < N_OUTPUTS; ++k)
            if (on[k]) sink[k] = make(k);
    }
    // the first one that is on (the stage clock that pays for reading the rows back is its); quoting: ... and quotes the BED text
    const Output *first(bool quoting = false) const {
        for (size_t k = 0; k < N_OUTPUTS; ++k)
            if (sink[k] && (kOutputs[k].quotes_bed || !quoting)) return &kOutputs[k];
        return nullptr;
    }
    bool any() const { return first() != nullptr; }
};

struct Options {
    std::string fasta, out;
    int min_motif = 2, max_motif = 100;          // global_variables.cpp:21-22
    bool has_min_length = false, has_min_units = false, has_perfect_units = false;
    std::string min_length, min_units, perfect_units;
    int device = 0;
    std::vector<int> devices;                     // --devices / RIBBIT_DEVICES: GPUs the records are dealt over (empty: `device` alone)
    int jobs = 0;                                 // records in flight PER DEVICE; 0 = automatic
    std::string timing;                           // --timing FILE: a JSON record of the run (the reference has cerr progress lines only)
    std::string other_path;                       // --overlap-with FILE: the intervals the overlap and nearest outputs compare the rows with
    std::string marker_fasta, marker_bed;         // --marker-fasta FILE --marker-bed FILE: the second assembly, and the chosen pairs typed on it
    std::string panel_bed;                        // --panel-bed FILE: the markers worth ordering pooled into multiplex panels
    int panel_pool_size = 8, panel_max = 16384;   // --panel-pool-size, --panel-max
    bool panel_pool_size_given = false, panel_max_given = false;
    std::string population_list;                  // --population-list FILE: the samples (name<TAB>path of a FASTA) the chosen pairs are typed on
    std::string allele_bed, allele_matrix;        // --allele-bed FILE, --allele-matrix FILE: every marker's alleles over the samples, and the genotype matrix
    std::array<std::string, N_OUTPUTS> row_path;                  // the row outputs' files, as kOutputs orders them (empty: off)
    std::array<std::array<bool, MAX_QUALIFIERS>, N_OUTPUTS> qualifier_given{};
    Settings settings;
};

const char *kHelp =
    "Below are the running options for the tool.:\n"
    "  -h [ --help ]                 Ribbit tool identifies short tandem repeats with allowed levels of inpurity.\n"
    "  -i [ --input-file ] arg       File path for the input fasta file.\n"
    "  -o [ --output-file ] arg      File path for the input fasta file.\n"
    "  -m [ --min-motif-length ] arg The minimum length of the motif of the repeats to be identified. Default: 2\n"
    "  -M [ --max-motif-length ] arg The maximum length of the motif of the repeats to be identified, Default: 100\n"
    "  -p [ --purity ] arg           Threshold value for cotinuous number of ones found in a seed. Default: 0.85\n"
    "  -l [ --min-length ] arg       The minimum length of the repeat. Default: 12\n"
    "  --min-units arg               The minimum number of units of the repeat. Integer, or a tab separated file\n"
    "                                with the motif size and the unit cutoff. Default: 2\n"
    "  --perfect-units arg           The minimum number of complete units of the repeat. Integer, or a tab\n"
    "                                separated file with the motif size and the unit cutoff. Default: 2\n"
    "  --jobs arg                    (ribbit-hip) FASTA records processed side by side on each GPU. Default: automatic\n"
    "  --device arg                  (ribbit-hip) GPU ordinal. Default: 0\n"
    "  --devices arg                 (ribbit-hip) GPU ordinals, comma separated (or RIBBIT_DEVICES): the records of the\n"
    "                                FASTA are dealt over these GPUs, the longest of the look-ahead first; BED rows\n"
    "                                keep the input order\n"
    "  --timing arg                  (ribbit-hip) write a JSON record of the run to this file: records, bases, wall time and\n"
    "                                the wall time per stage summed over the records\n"
    "  --marker-fasta arg            (ribbit-hip) a second assembly (another individual, strain or haplotype, the previous\n"
    "                                release) that --marker-bed types --primer-genome-bed's chosen pairs on\n"
    "  --marker-bed arg              (ribbit-hip) also write the rows of --primer-genome-bed (chosen with --primer-genome-flank,\n"
    "                                whether or not that file is asked for) to this file with 20 columns: the eight primer\n"
    "                                columns and the designed product; the products the pair has on all records of\n"
    "                                --marker-fasta ('.' where a primer has more than 64 sites on a strand of one record);\n"
    "                                and, only where that is exactly one product: the record's name, start, end, orientation\n"
    "                                (+, -; l, r: one primer with itself), size, size minus the designed product, then start,\n"
    "                                end, bases and whole units of the longest tract of the row's motif inside the product\n"
    "                                ('.' without one). A marker is worth ordering when that difference is not 0. The other\n"
    "                                FASTA is read after the input has been read twice, on the first GPU\n"
    "  --panel-bed arg               (ribbit-hip) with --marker-fasta and --marker-bed: also write the markers worth ordering\n"
    "                                (exactly one product on the other assembly, of another size than designed) to this file,\n"
    "                                pooled into multiplex PCR panels on the GPU: each marker line of --marker-bed with five more\n"
    "                                columns: pool, conflicts, dimer, size, near. Two markers conflict when a primer of one binds\n"
    "                                a primer of the other (ungapped run above 6, or above 4 through a 3' end), when their\n"
    "                                expected product sizes lie less than 30 apart, or when they lie on one record within 4000\n"
    "                                bases; markers are taken by descending conflicts and go into the first pool with room and\n"
    "                                no conflict, so the low-numbered pools fill first. Sorted by pool, then designed product\n"
    "  --panel-pool-size arg         (ribbit-hip) for --panel-bed: the most markers of one pool, 1 .. 65536. Default: 8\n"
    "  --panel-max arg               (ribbit-hip) for --panel-bed: the most markers pooled, 1 .. 65536; of more, those whose size\n"
    "                                differs most from the designed product are taken. Default: 16384\n"
    "  --population-list arg         (ribbit-hip) the samples that --allele-bed and --allele-matrix type --primer-genome-bed's chosen\n"
    "                                pairs on: a file with one sample per line, name<TAB>path of its FASTA (1 .. 1024 samples,\n"
    "                                the names unique; empty lines and lines starting with # are skipped). The input itself is a\n"
    "                                sample only if the list names it. The samples are read one after the other, in list order,\n"
    "                                after every other pass, on the first GPU; one int32 is kept per sample and row\n"
    "  --allele-bed arg              (ribbit-hip) with --population-list: also write the rows of --primer-genome-bed (chosen with\n"
    "                                --primer-genome-flank, whether or not that file is asked for) to this file with 23 columns:\n"
    "                                the eight primer columns and the designed product; then, over the samples, counted on the\n"
    "                                GPU: samples, typed (exactly one product), absent, several, over (a primer with more than 64\n"
    "                                sites), alleles (distinct product sizes), the least, the largest and the most frequent size\n"
    "                                with its count, the samples of the designed size, those whose size is off the motif's step,\n"
    "                                the expected heterozygosity He = 1 - sum p^2 and the polymorphism information content PIC\n"
    "                                (Botstein 1980), four decimals ('.' where no sample is typed)\n"
    "  --allele-matrix arg           (ribbit-hip) with --population-list: also write the genotype matrix to this file: a header\n"
    "                                line (#name, start, end, motif, designed, the samples' names), then per row its first four\n"
    "                                columns, the designed product and per sample the product's size, '.' absent, '+' several,\n"
    "                                '*' over\n"
    "  --masked-fasta arg            (ribbit-hip) also write the records to this FASTA file with the bases of their BED rows\n"
    "                                masked; a header keeps the record name only (the description after the first space\n"
    "                                is not kept)\n"
    "  --mask arg                    (ribbit-hip) soft: masked letters A-Z become lowercase; hard: masked bases become N.\n"
    "                                Default: soft\n"
    "  --mask-width arg              (ribbit-hip) bases per line of the masked FASTA, 0 for one line per record. Default: 60\n"
    "  --repeat-fasta arg            (ribbit-hip) also write every BED row's bases with their flanks to this FASTA file, one\n"
    "                                entry per row in BED order, headed '>name:start-end flank=left,right' (start and end\n"
    "                                clipped to the record; left, right: the flank bases taken on either side)\n"
    "  --flank arg                   (ribbit-hip) bases of the record taken on either side of a row for --repeat-fasta.\n"
    "                                Default: 100\n"
    "  --loci-bed arg                (ribbit-hip) also write the BED rows of every record merged into loci to this file, sorted\n"
    "                                by start: rows that overlap or abut are one locus. 15 columns: name, start, end, rows\n"
    "                                merged, bases covered, then the last ten columns of the locus's longest row\n"
    "  --loci-gap arg                (ribbit-hip) for --loci-bed: stretches of rows at most this many bases apart are one\n"
    "                                locus, as bedtools merge -d. Default: 0\n"
    "  --density-bedgraph arg        (ribbit-hip) also write a bedGraph to this file: one line per window of every record,\n"
    "                                empty windows too: name, start, end, and the NUMBER OF BASES of the window that BED\n"
    "                                rows cover (an exact integer count, not a fraction: divide by end - start for one)\n"
    "  --density-window arg          (ribbit-hip) bases per window of --density-bedgraph, 1 or more. Default: 10000\n"
    "  --overlap-with arg            (ribbit-hip) a second BED file (name, start, end; a truth set, another caller's rows, an\n"
    "                                annotation) that --overlap-bed, --overlap-summary, --nearest-bed and --nearest-other-bed\n"
    "                                compare the BED rows of every record with; a name is matched against the record names;\n"
    "                                column 4, if there is one, is the interval's label in the nearest outputs ('.' without\n"
    "                                one); further columns are ignored\n"
    "  --overlap-bed arg             (ribbit-hip) also write every BED row to this file with two columns appended: the number\n"
    "                                of intervals of --overlap-with that the row overlaps, and the number of the row's bases\n"
    "                                that those intervals cover\n"
    "  --overlap-summary arg         (ribbit-hip) also write one line per record to this file: name, length, rows, rows_hit,\n"
    "                                other, other_hit, rows_bases, other_bases, both_bases (exact counts, not fractions: recall\n"
    "                                is other_hit / other, precision rows_hit / rows, the base-level Jaccard index\n"
    "                                both_bases / (rows_bases + other_bases - both_bases))\n"
    "  --best-bed arg                (ribbit-hip) also write a non-redundant call set to this file: the BED rows of every record\n"
    "                                of which no two overlap and which together cover the most bases, each row as it is in\n"
    "                                the BED, sorted by start\n"
    "  --class-bed arg               (ribbit-hip) also write every BED row to this file with two columns appended: the canonical\n"
    "                                class of its motif (the least of the motif's rotations and of the rotations of its\n"
    "                                reverse complement, so AC, CA, GT and TG are all AC) and '+' if a rotation of the motif\n"
    "                                itself is that class, '-' if only the reverse complement's is\n"
    "  --motif-summary arg           (ribbit-hip) also write a census of what repeats to this file, one line per record and motif\n"
    "                                class, by class length, then alphabetically: name, class, length, rows, bases (the sum of\n"
    "                                the rows' lengths, not their union), start and end of the class's longest row\n"
    "  --compound-bed arg            (ribbit-hip) also write what every locus is made of to this file: the rows of --best-bed's\n"
    "                                selection chained while they lie at most --compound-gap bases apart, one line per chain:\n"
    "                                name, start, end, kind (p perfect: one row; i interrupted: several rows of one motif\n"
    "                                class; c compound: more than one class), rows, classes, bases (the sum of the rows'\n"
    "                                lengths) and the structure, e.g. (CA)12n5(GA)8: motif and units of every row, n5 for 5\n"
    "                                bases between two rows\n"
    "  --compound-gap arg            (ribbit-hip) for --compound-bed: a row at most this many bases behind the rows before it\n"
    "                                continues their chain, 0 .. 2147483647. Default: 100\n"
    "  --interruption-bed arg        (ribbit-hip) also write where the imperfections are to this file, decoded from the CIGAR of\n"
    "                                every BED row: one line per run of substitutions and indels inside a row: name, start,\n"
    "                                end, the run's CIGAR ops (1X, 2I1X, 1D), the bases the record has there ('.' for a\n"
    "                                deletion alone), the row's start, end and motif, and the 0-based repeat unit the run\n"
    "                                falls in. Rows whose CIGAR does not span them are left out and counted on stderr\n"
    "  --purity-bed arg              (ribbit-hip) also write every BED row to this file with seven columns appended: the number\n"
    "                                of such runs, their substituted, inserted and deleted bases, then start, end and whole\n"
    "                                motif units of the row's longest uninterrupted stretch (the leftmost of equals; '.'\n"
    "                                three times for a row whose CIGAR does not span it)\n"
    "  --nearest-bed arg             (ribbit-hip) also write every BED row to this file with eight columns appended, as bedtools\n"
    "                                closest would: 'in' if one interval of --overlap-with holds the whole row, 'over' if one\n"
    "                                overlaps it, '.' if none does; that interval's label, start and end (of several\n"
    "                                containers the one that reaches furthest, else the first overlapping one by start); then\n"
    "                                label and distance in bases of the nearest interval that ends at or before the row's\n"
    "                                start, and of the nearest that starts at or behind its end (0: they abut; '.': none)\n"
    "  --nearest-other-bed arg       (ribbit-hip) also write the other direction to this file, one line per interval of\n"
    "                                --overlap-with that belongs to a record, in the file's order: name, start, end, label,\n"
    "                                then the same eight columns with the record's BED rows in the intervals' place, a row's\n"
    "                                label being its motif: a truth locus that no row meets but that has one 3 bases away\n"
    "                                is a boundary disagreement, not a miss\n"
    "  --composition-bed arg         (ribbit-hip) also write every BED row to this file with 13 columns appended: the row's A, C,\n"
    "                                G, T and other bases (N, IUPAC letters; case is ignored), then for the flank to its left\n"
    "                                its length, its C + G, its other bases and its bases that BED rows cover (more than 0:\n"
    "                                the flank runs into another repeat), then the same four for the flank to its right.\n"
    "                                Exact counts, not fractions: GC content is (C + G) / length\n"
    "  --composition-flank arg       (ribbit-hip) bases of the record taken on either side of a row for --composition-bed, as\n"
    "                                --flank takes them for --repeat-fasta. Default: 100\n"
    "  --composition-track arg       (ribbit-hip) also write one line per window of every record to this file, empty windows\n"
    "                                too: name, start, end, A, C, G, T, other (exact counts of the window's bases; with equal\n"
    "                                windows the lines pair with those of --density-bedgraph)\n"
    "  --composition-window arg      (ribbit-hip) bases per window of --composition-track, 1 or more. Default: 10000\n"
    "  --primer-bed arg              (ribbit-hip) also write the rows of --best-bed's selection to this file with 11 columns\n"
    "                                appended, for typing the loci by PCR: start, end, sequence (5' to 3') and Tm of a forward\n"
    "                                primer in the flank to the row's left, the same four of a reverse primer in the flank to\n"
    "                                its right, the product's size, and the admissible candidates of either flank ('.' where a\n"
    "                                flank has none). 18 .. 25 bases, Tm 57 .. 63 C (nearest neighbour, 50 mM Na+, 50 nM), 40 ..\n"
    "                                60 % GC, a 3' C or G, no base repeated 5 times, no N and no base that a BED row covers.\n"
    "                                Each side is chosen on its own: check the pair for dimers, e.g. Primer3 check_primers;\n"
    "                                --primer-pair-bed is the checked form\n"
    "  --primer-flank arg            (ribbit-hip) bases of the record on either side of a row that --primer-bed may place a\n"
    "                                primer in, 0 .. 1000. Default: 200\n"
    "  --primer-pair-bed arg         (ribbit-hip) also write the rows of --best-bed's selection to this file with 21 columns\n"
    "                                appended: the two primers of --primer-bed's rules chosen together. A candidate must not\n"
    "                                bind to itself (ungapped: at most 4 bonded bases in a row, 3 at a 3' end) nor fold into a\n"
    "                                hairpin (stem of at most 3 around a loop of 3 or more); of the 8 best of either flank the\n"
    "                                pair is taken that does not bind to each other (the same limits), melts within 3 C of\n"
    "                                each other and has the least penalty. Columns: the eight primer columns and the product,\n"
    "                                Tm difference, pair any and end, self any, self end and hairpin of the left and of the\n"
    "                                right primer, passing candidates left and right, admissible pairs ('.' in the first 18\n"
    "                                where no pair is admissible)\n"
    "  --primer-pair-flank arg       (ribbit-hip) bases of the record on either side of a row that --primer-pair-bed may place\n"
    "                                a primer in, 0 .. 1000. Default: 200\n"
    "  --primer-product-bed arg      (ribbit-hip) also write the rows of --best-bed's selection to this file with 27 columns\n"
    "                                appended: the 21 of --primer-pair-bed, then an in-silico PCR of the pair. A primer has a\n"
    "                                site wherever its last 15 bases match the record exactly and at most 2 of its other bases\n"
    "                                differ, on either strand, inside other repeats too; a product is a forward and a reverse\n"
    "                                site of either primer at most 4000 bases apart, end to end. Columns: forward and reverse\n"
    "                                sites of the left primer, of the right primer, products other than the pair's own (0: the\n"
    "                                pair is specific), the shortest of them ('.' in the last two when a primer has more than\n"
    "                                64 sites on a strand, in all six where there is no pair). Only the record itself is\n"
    "                                searched, not the other records of the input: for a genome, ask Scanner.record_oligo_sites\n"
    "                                of the Python package record by record and add up\n"
    "  --primer-product-flank arg    (ribbit-hip) bases of the record on either side of a row that --primer-product-bed may\n"
    "                                place a primer in, 0 .. 1000. Default: 200\n"
    "  --primer-specific-bed arg     (ribbit-hip) also write the rows of --best-bed's selection to this file with 31 columns\n"
    "                                appended: the 27 of --primer-product-bed, but for the best pair that amplifies nothing\n"
    "                                else. All pairs of the 8 best candidates of either flank that --primer-pair-bed would\n"
    "                                admit go through that in-silico PCR, in the order of its choice, and the first one without\n"
    "                                another product is taken; there is no fallback. Then: the place of that pair in the order\n"
    "                                (0: --primer-pair-bed's own pair), the specific pairs, the pairs with a primer of more\n"
    "                                than 64 sites on a strand, the pairs with another product ('.' in the first 18, in the six\n"
    "                                of the PCR and in the place where no pair is specific). Only the record itself is\n"
    "                                searched, not the other records of the input\n"
    "  --primer-specific-flank arg   (ribbit-hip) bases of the record on either side of a row that --primer-specific-bed may\n"
    "                                place a primer in, 0 .. 1000. Default: 200\n"
    "  --primer-genome-bed arg       (ribbit-hip) also write the rows of --best-bed's selection to this file with the 31 columns\n"
    "                                of --primer-specific-bed, every count and verdict taken over ALL records of the input: the\n"
    "                                pairs of a row are those of its own record, and each goes through the in-silico PCR on\n"
    "                                every record. A pair is passed over when a primer has more than 64 sites on a strand of\n"
    "                                any one record, or when it has a product other than its own in any record; the first pair\n"
    "                                left is taken, and there is no fallback. The site counts are sums over the records. The\n"
    "                                input is read a second time after the last record, on the first GPU; the rows' lines and\n"
    "                                about 600 bytes per row stay in memory until then\n"
    "  --primer-genome-flank arg     (ribbit-hip) bases of the record on either side of a row that --primer-genome-bed may place\n"
    "                                a primer in, 0 .. 1000. Default: 200\n";

bool parse_device_list(const std::string &value, std::vector<int> &out) {
    out.clear();
    size_t at = 0;
    while (at <= value.size()) {
        const size_t comma = std::min(value.find(',', at), value.size());
        const std::string item = value.substr(at, comma - at);
        if (item.empty() || !std::all_of(item.begin(), item.end(), [](unsigned char c) { return std::isdigit(c); })) return false;
        out.push_back(std::atoi(item.c_str()));
        at = comma + 1;
    }
    return !out.empty();
}

bool is_number(const std::string &s) { return !s.empty() && std::all_of(s.begin(), s.end(), [](unsigned char c) { return std::isdigit(c); }); }

// returns 0 for --help (the caller exits 1, as the reference does), 1 on success
int parse_arguments(int argc, char **argv, Options &o) {
    static const std::map<std::string, std::string> longs = {
        {"help", "h"}, {"input-file", "i"}, {"output-file", "o"}, {"min-motif-length", "m"}, {"max-motif-length", "M"},
        {"purity", "p"}, {"min-length", "l"}, {"min-units", "U"}, {"perfect-units", "P"}, {"device", "D"}, {"jobs", "J"}, {"devices", "G"}, {"timing", "T"},
        {"overlap-with", "W"}, {"marker-fasta", "F"}, {"marker-bed", "K"}, {"panel-bed", "B"}, {"panel-pool-size", "S"}, {"panel-max", "X"},
        {"population-list", "L"}, {"allele-bed", "A"}, {"allele-matrix", "Y"}};
    bool help = false;
    for (int a = 1; a < argc; ++a) {
        std::string arg = argv[a], key, value;
        bool has_value = false;
        size_t output = N_OUTPUTS, qualifier = MAX_QUALIFIERS;      // a row output's option: --option FILE, or qualifier `qualifier` of it
        if (arg.rfind("--", 0) == 0) {
            const size_t eq = arg.find('=');
            const std::string name = arg.substr(2, eq == std::string::npos ? std::string::npos : eq - 2);
            auto it = longs.find(name);
            for (size_t k = 0; k < N_OUTPUTS; ++k) {
                if (name == kOutputs[k].option) output = k;
                for (size_t q = 0; q < MAX_QUALIFIERS; ++q)
                    if (kOutputs[k].qualifiers[q].name && name == kOutputs[k].qualifiers[q].name) { output = k; qualifier = q; }
            }
            if (it == longs.end() && output == N_OUTPUTS) die("unrecognised option '" + arg + "'");
            if (it != longs.end()) key = it->second;
            if (eq != std::string::npos) { value = arg.substr(eq + 1); has_value = true; }
        } else if (arg.size() >= 2 && arg[0] == '-') {
            key = arg.substr(1, 1);
            if (std::string("hiomMpl").find(key) == std::string::npos) die("unrecognised option '" + arg + "'");
            if (arg.size() > 2) { value = arg.substr(2); has_value = true; }
        } else {
            die("too many positional options have been specified on the command line");
        }
        if (key == "h") { help = true; continue; }
        if (!has_value) {
            if (a + 1 >= argc) die("the required argument for option '" + arg + "' is missing");
            value = argv[++a];
        }
        if (output < N_OUTPUTS && qualifier == MAX_QUALIFIERS) {
            if (value.empty()) die(std::string("--") + kOutputs[output].option + " wants a file name");
            o.row_path[output] = value;
        } else if (output < N_OUTPUTS) {
            const Qualifier &q = kOutputs[output].qualifiers[qualifier];
            if (q.kind == Qualifier::SOFT_HARD) {
                if (value != "soft" && value != "hard") die(std::string("--") + q.name + " wants soft or hard, got '" + value + "'");
                o.settings.*q.field = value == "soft" ? RIBBIT_MASK_SOFT : RIBBIT_MASK_HARD;
            } else {
                if (!is_number(value) || value.size() > q.max_digits || std::atoll(value.c_str()) < q.lo || std::atoll(value.c_str()) > q.hi)
                    die(std::string("--") + q.name + " wants a whole number of bases (" + q.range + "), got '" + value + "'");
                o.settings.*q.field = (int)std::atoll(value.c_str());
            }
            o.qualifier_given[output][qualifier] = true;
        }
        else if (key == "i") o.fasta = value;
        else if (key == "o") o.out = value;
        else if (key == "m") o.min_motif = std::atoi(value.c_str());
        else if (key == "M") o.max_motif = std::atoi(value.c_str());
        else if (key == "p") { /* declared, never read (ribbit.cpp:92) */ }
        else if (key == "l") { o.has_min_length = true; o.min_length = value; }
        else if (key == "U") { o.has_min_units = true; o.min_units = value; }
        else if (key == "P") { o.has_perfect_units = true; o.perfect_units = value; }
        else if (key == "D") o.device = std::atoi(value.c_str());
        else if (key == "J") o.jobs = std::atoi(value.c_str());
        else if (key == "T") o.timing = value;
        else if (key == "W") { if (value.empty()) die("--overlap-with wants a file name"); o.other_path = value; }
        else if (key == "F") { if (value.empty()) die("--marker-fasta wants a file name"); o.marker_fasta = value; }
        else if (key == "K") { if (value.empty()) die("--marker-bed wants a file name"); o.marker_bed = value; }
        else if (key == "B") { if (value.empty()) die("--panel-bed wants a file name"); o.panel_bed = value; }
        else if (key == "L") { if (value.empty()) die("--population-list wants a file name"); o.population_list = value; }
        else if (key == "A") { if (value.empty()) die("--allele-bed wants a file name"); o.allele_bed = value; }
        else if (key == "Y") { if (value.empty()) die("--allele-matrix wants a file name"); o.allele_matrix = value; }
        else if (key == "S" || key == "X") {
            const char *name = key == "S" ? "--panel-pool-size" : "--panel-max";
            if (!is_number(value) || value.size() > 5 || std::atoi(value.c_str()) < 1 || std::atoi(value.c_str()) > 65536)
                die(std::string(name) + " wants a whole number (1 .. 65536), got '" + value + "'");
            (key == "S" ? o.panel_pool_size : o.panel_max) = std::atoi(value.c_str());
            (key == "S" ? o.panel_pool_size_given : o.panel_max_given) = true;
        }
        else if (key == "G") { if (!parse_device_list(value, o.devices)) die("--devices wants a comma separated list of GPU ordinals, got '" + value + "'"); }
    }
    if (help) { std::cerr << kHelp << "\n"; return 0; }                       // ribbit.cpp:114-117
    for (size_t k = 0; k < N_OUTPUTS; ++k)
        for (size_t q = 0; q < MAX_QUALIFIERS && o.row_path[k].empty(); ++q)
            if (o.qualifier_given[k][q]) die(std::string("--") + kOutputs[k].qualifiers[q].name + " needs --" + kOutputs[k].option);
    bool needs_other = false;
    for (size_t k = 0; k < N_OUTPUTS; ++k) needs_other = needs_other || (kOutputs[k].needs_other && !o.row_path[k].empty());
    if (!o.other_path.empty() && !needs_other) die("--overlap-with needs --overlap-bed or --overlap-summary");
    for (size_t k = 0; k < N_OUTPUTS; ++k)
        if (kOutputs[k].needs_other && !o.row_path[k].empty() && o.other_path.empty()) die(std::string("--") + kOutputs[k].option + " needs --overlap-with");
    if (o.panel_bed.empty() && o.panel_pool_size_given) die("--panel-pool-size needs --panel-bed");
    if (o.panel_bed.empty() && o.panel_max_given) die("--panel-max needs --panel-bed");
    if (!o.panel_bed.empty() && (o.marker_fasta.empty() || o.marker_bed.empty())) die("--panel-bed needs --marker-fasta and --marker-bed");
    if (!o.marker_fasta.empty() && o.marker_bed.empty()) die("--marker-fasta needs --marker-bed");
    if (!o.marker_bed.empty() && o.marker_fasta.empty()) die("--marker-bed needs --marker-fasta");
    if (!o.population_list.empty() && o.allele_bed.empty() && o.allele_matrix.empty()) die("--population-list needs --allele-bed or --allele-matrix");
    if (!o.allele_bed.empty() && o.population_list.empty()) die("--allele-bed needs --population-list");
    if (!o.allele_matrix.empty() && o.population_list.empty()) die("--allele-matrix needs --population-list");
    if (o.fasta.empty()) { std::cerr << "ERROR: Please specify an input fasta file!\n"; return 0; }   // :122-126
    return 1;
}

// one decimal field of a BED line; false unless it is [-]digits within int32
bool parse_int32(const char *p, const char *end, int32_t *out) {
    int64_t v = 0;
    const auto r = std::from_chars(p, end, v);
    if (p == end || r.ec != std::errc() || r.ptr != end || v < INT32_MIN || v > INT32_MAX) return false;
    *out = (int32_t)v;
    return true;
}

// --overlap-with FILE: name, start, end, a label if there is a fourth column, and whatever follows, tab separated; empty lines and
// lines that start with '#', "track" or "browser" are skipped.  A name may come anywhere in the file; its intervals keep the file's
// order.
void read_other_bed(const std::string &path, OtherBed &other) {
    std::ifstream in(path, std::ios::binary);
    if (!in) die("--overlap-with: cannot open '" + path + "' for reading");
    std::string line;
    for (size_t k = 1; std::getline(in, line); ++k) {
        if (line.empty() || line[0] == '#' || line.rfind("track", 0) == 0 || line.rfind("browser", 0) == 0) continue;
        const size_t t1 = line.find('\t'), t2 = t1 == std::string::npos ? t1 : line.find('\t', t1 + 1);
        const size_t t3 = t2 == std::string::npos ? t2 : std::min(line.find('\t', t2 + 1), line.size());
        int32_t s = 0, e = 0;
        if (t2 == std::string::npos || !parse_int32(line.data() + t1 + 1, line.data() + t2, &s) || !parse_int32(line.data() + t2 + 1, line.data() + t3, &e))
            die("--overlap-with: line " + std::to_string(k) + " of '" + path + "' is not a BED line (name, start, end)");
        OtherBed::Group &group = other.by_name[line.substr(0, t1)];
        group.iv.push_back(s);
        group.iv.push_back(e);
        // the label: the bytes between the third tab and the next one or the line's end; "." for none
        const size_t from = std::min(t3 + 1, line.size()), to = std::min(line.find('\t', from), line.size());
        if (to > from) group.labels.append(line, from, to - from); else group.labels += '.';
        if (group.labels.size() > (size_t)INT32_MAX) die("--overlap-with: the labels of '" + line.substr(0, t1) + "' in '" + path + "' are 2^31 bytes or more");
        group.label_at.push_back((int32_t)group.labels.size());
    }
}

// parseDualtypeArgs, ribbit.cpp:25-64: one integer for every motif size in range, or a two-column TSV
void dual_type(const std::string &value, std::map<int, int> &table, int m_lo, int m_hi) {
    if (is_number(value)) {
        for (int k = m_lo; k <= m_hi; ++k) table[k] = std::atoi(value.c_str());
        return;
    }
    std::ifstream in(value);
    std::string line;
    while (std::getline(in, line)) {
        const size_t tab = line.find('\t');
        if (tab == std::string::npos) continue;
        table[std::atoi(line.substr(0, tab).c_str())] = std::atoi(line.substr(tab + 1).c_str());
    }
}

// ribbit.cpp:143-174 and the factor completion of :210-235
void build_refine_params(const Options &o, RibbitRefineParams &prm) {
    ribbit_refine_params_default(&prm, o.min_motif, o.max_motif);
    if (!o.has_min_length && !o.has_min_units && !o.has_perfect_units) return;
    std::map<int, int> min_length, min_units, perfect_units;
    if (o.has_min_length) dual_type(o.min_length, min_length, o.min_motif, o.max_motif);
    else if (o.has_min_units) {
        dual_type(o.min_units, min_units, o.min_motif, o.max_motif);
        for (auto &kv : min_units) min_length[kv.first] = kv.first * kv.second;
    } else {
        for (int k = o.min_motif; k <= o.max_motif; ++k) min_length[k] = std::max(12, 2 * k);
    }
    if (o.has_perfect_units) dual_type(o.perfect_units, perfect_units, o.min_motif, o.max_motif);
    else for (int m = 1; m <= o.max_motif; ++m) perfect_units[m] = m == 1 ? 8 : m == 2 ? 4 : m == 3 ? 3 : 2;
    for (int m = o.min_motif; m <= o.max_motif; ++m)
        for (int f = 1; f <= m / 2; ++f) {
            if (m % f) continue;
            if (!min_length.count(f)) min_length[f] = min_length[m];
            if (!perfect_units.count(f)) perfect_units[f] = perfect_units[m] * (m / f);
        }
    std::memset(prm.min_length, 0, sizeof prm.min_length);
    std::memset(prm.perfect_units, 0, sizeof prm.perfect_units);
    for (auto &kv : min_length) if (kv.first >= 0 && kv.first < RIBBIT_TABLE) prm.min_length[kv.first] = kv.second;
    for (auto &kv : perfect_units) if (kv.first >= 0 && kv.first < RIBBIT_TABLE) prm.perfect_units[kv.first] = kv.second;
}

size_t count_failed(const RibbitSeed *s, size_t n) {
    size_t c = 0;
    for (size_t i = 0; i < n; ++i) c += s[i].type == RIBBIT_RANK_N;
    return c;
}

// the (start, end) pairs of a BED text, appended to iv
void append_intervals(const char *text, size_t len, std::vector<int32_t> &iv) {
    int32_t *pairs = nullptr;
    size_t n = 0;
    if (ribbit_bed_intervals(text, len, &pairs, &n) != RIBBIT_OK) throw PathError{std::string("reading the BED rows back failed: ") + ribbit_hip_last_error()};
    iv.insert(iv.end(), pairs, pairs + 2 * n);
    ribbit_intervals_free(pairs);
}

// Refinement of ONE record over several GPUs (ribbit_hip_adopt_dispatch): the dispatched seeds in as many slices as there are
// handles, equal numbers of seeds each (a seed's cost varies by orders of magnitude, but over millions of seeds the slices even
// out); every helper loads the record on its own GPU, makes the composed planes there and refines its slice on its GPU's share of
// the host threads; the texts in order are the record's BED.  An alignment with an empty query in any slice (it would see the
// previous seed's CIGAR, which may be another slice's) makes the record be refined again in one piece, on `h`.
struct Helper { RibbitHandle *h; int host_threads; };
bool refine_over_devices(RibbitHandle *h, const std::vector<Helper> &helpers, const RibbitRefineParams &prm, const std::string &name, const char *bases,
                         int64_t length, const RibbitSeed *d, size_t nd, std::ostream &out, std::ostream &log, std::vector<int32_t> *mask_iv,
                         std::string *bed_copy) {
    const size_t parts = helpers.size() + 1;
    const std::vector<RibbitSeed> all(d, d + nd);          // (`d` is `h`'s own list, which adopting a slice replaces)
    std::vector<std::string> text(parts), error(parts);
    std::vector<int> empty_query(parts, 0);
    auto slice = [&](size_t k, RibbitHandle *hk, bool load) {
        const size_t lo = nd * k / parts, hi = nd * (k + 1) / parts;
        if (load && ribbit_hip_load_record_pinned(hk, bases, length) != RIBBIT_OK) { error[k] = ribbit_hip_last_error(); return; }
        const char *t = nullptr;
        size_t len = 0;
        if (ribbit_hip_adopt_dispatch(hk, all.data() + lo, hi - lo) != RIBBIT_OK || ribbit_hip_refine_bed(hk, &prm, name.c_str(), &t, &len) != RIBBIT_OK) {
            error[k] = ribbit_hip_last_error();
            return;
        }
        text[k].assign(t, len);
        empty_query[k] = ribbit_hip_refine_met_empty_query(hk);
    };
    for (const Helper &hp : helpers) check(ribbit_hip_set_host_threads(hp.h, hp.host_threads));      // (anything that can throw: before the first thread exists)
    std::vector<std::thread> pool;
    pool.reserve(parts);
    try {
        for (size_t k = 1; k < parts; ++k) pool.emplace_back(slice, k, helpers[k - 1].h, true);
    } catch (...) {            // a thread that could not start: its slice and the ones after it run here, one after the other
        for (size_t k = pool.size() + 1; k < parts; ++k) slice(k, helpers[k - 1].h, true);
    }
    slice(0, h, false);
    for (std::thread &t : pool) t.join();
    for (size_t k = 0; k < parts; ++k)
        if (!error[k].empty()) throw PathError{"GPU path failed: " + error[k]};
    bool redo = false;
    for (size_t k = 1; k < parts; ++k) redo = redo || empty_query[k] != 0;
    if (redo) {
        const char *t = nullptr;
        size_t len = 0;
        check(ribbit_hip_adopt_dispatch(h, all.data(), nd));
        check(ribbit_hip_refine_bed(h, &prm, name.c_str(), &t, &len));
        out.write(t, (std::streamsize)len);
        if (mask_iv) append_intervals(t, len, *mask_iv);
        if (bed_copy) bed_copy->assign(t, len);
        log << "[devices] an alignment with an empty query at the head of a slice: the record was refined again in one piece\n";
        return false;
    }
    for (size_t k = 0; k < parts; ++k) out.write(text[k].data(), (std::streamsize)text[k].size());
    if (mask_iv)      // (the rows of all slices: the mask of a record is the union of all of its rows)
        for (size_t k = 0; k < parts; ++k) append_intervals(text[k].data(), text[k].size(), *mask_iv);
    if (bed_copy)     // (the loci's lines quote the rows: the slices' texts as one, row i on line i)
        for (size_t k = 0; k < parts; ++k) bed_copy->append(text[k]);
    return true;
}

// processSequence (fasta_utils.cpp:59-250) through the C ABI, with the reference's progress lines; then the record's text for
// every row output that `jobs` has a sink for, in the order of kOutputs, all on `h`, the handle that loaded it
void process_sequence(RibbitHandle *h, const RibbitRefineParams &prm, const std::string &name, const char *bases, int64_t length,
                      std::ostream &out, std::ostream &log, const Settings &settings, const RowJobs &jobs, const std::vector<Helper> *helpers = nullptr) {
    const time_t t0 = time(0);
    auto secs = [&]() { return difftime(time(0), t0); };
    { StageClock c(LOAD); check(ribbit_hip_load_record_pinned(h, bases, length)); }
    log << "Generated shift XORs!\t Time elapsed:" << secs() << "secs\n";
    const RibbitSeed *p, *s, *a;
    size_t np, ns, na;
    { StageClock c(PERFECT); check(ribbit_hip_seeds_perfect(h, &p, &np)); }
    log << "Total number of perfect seeds: " << np << "\t Time elapsed: " << secs() << "secs\n";
    { StageClock c(SUBSTITUTIONS); check(ribbit_hip_seeds_substitutions(h, &p, &np, &s, &ns)); }
    log << "Total number of seeds considering substitutions: " << np + ns - count_failed(p, np) - count_failed(s, ns)
              << "\t Time elapsed: " << secs() << "secs\n";
    { StageClock c(ANCHORED); check(ribbit_hip_seeds_anchored(h, &p, &np, &s, &ns, &a, &na)); }
    log << "Generated anchored shift XORs!\t Time elapsed: " << secs() << "secs\n";
    log << "Total number of seeds considering indels: "
              << np + ns + na - count_failed(p, np) - count_failed(s, ns) - count_failed(a, na) << "\t Time elapsed: " << secs() << "secs\n";
    const RibbitSeed *d;
    size_t nd;
    { StageClock c(DISPATCH); check(ribbit_hip_dispatch_seeds(h, &d, &nd)); }
    // one record over several GPUs: only worth it from a few hundred thousand seeds on (RIBBIT_SHARD_MIN_SEEDS: a test hook)
    static const size_t shard_min = std::getenv("RIBBIT_SHARD_MIN_SEEDS") ? (size_t)std::atoll(std::getenv("RIBBIT_SHARD_MIN_SEEDS")) : 400000;
    RecordRows rows{name, length, {}, nullptr, 0, {}, settings.other ? settings.other->of(name) : nullptr, {}, {}, {}, {}};
    const bool want_rows = jobs.any();
    if (helpers && !helpers->empty() && nd >= shard_min && nd >= 2 * (helpers->size() + 1)) {
        StageClock c(REFINE_BED);
        const bool sharded = refine_over_devices(h, *helpers, prm, name, bases, length, d, nd, out, log, want_rows ? &rows.iv : nullptr,
                                                 jobs.first(true) ? &rows.bed_copy : nullptr);
        rows.bed_text = rows.bed_copy.data();
        rows.bed_len = rows.bed_copy.size();
        if (std::getenv("RIBBIT_PROFILE"))
            log << "[devices] refinement of " << name << ": " << nd << " dispatched seeds " << (sharded ? "in " : "NOT in ") << helpers->size() + 1 << " slices over as many handles\n";
    } else {
        const char *text;
        size_t len;
        { StageClock c(REFINE_BED); check(ribbit_hip_refine_bed(h, &prm, name.c_str(), &text, &len)); }
        out.write(text, (std::streamsize)len);
        if (want_rows) { StageClock c(jobs.first()->stage); append_intervals(text, len, rows.iv); }
        rows.bed_text = text;
        rows.bed_len = len;
    }
    for (size_t k = 0; k < N_OUTPUTS; ++k)
        if (jobs.sink[k]) kOutputs[k].produce(h, rows, settings, jobs.sink[k]);
    log << "Total number of seeds that are processed for alignment: " << nd << "\t Time elapsed: " << secs() << "secs\n";
}

// The second pass of --primer-genome-bed, after the last record, on the handle h: `states` holds what produce_primer_genome made of
// every record, in input order.  The FASTA is read again; every record is loaded and nothing is scanned; all records' lists are
// judged on it, the record's own as home; the verdicts are summed; then every record's pairs are chosen and its text is written.
// file: --primer-genome-bed's, or null when only --marker-bed asked for the selection; keep: where --marker-bed's pass finds every
// record's chosen pairs and lines (null: not kept).
struct KeptMarkers {
    std::vector<RibbitRowPrimerPair> pairs;      // of all records, in input order ...
    std::vector<size_t> first{0};                // ... record k's are [first[k], first[k + 1])
    std::string lines;                           // their BED lines, one behind the other
    std::vector<size_t> line_at{0};              // record k's lines are lines[line_at[k], line_at[k + 1])
    std::vector<int32_t> record;                 // which record of the input record k is
};
void write_primer_genome(RibbitHandle *h, const std::string &fasta, const std::vector<std::string> &states, std::ostream *file, KeptMarkers *keep) {
    StageClock c(PRIMER_GENOME);
    std::vector<size_t> first(states.size() + 1, 0);      // record k's targets are [first[k], first[k + 1])
    for (size_t k = 0; k < states.size(); ++k) {
        uint64_t head[2];
        std::memcpy(head, states[k].data(), sizeof head);
        first[k + 1] = first[k] + (size_t)head[0];
    }
    const size_t total = first.back();
    if (total == 0) return;      // (no target anywhere: every record's text is empty)
    std::vector<RibbitTargetShortlists> lists(total);
    for (size_t k = 0; k < states.size(); ++k)
        if (first[k + 1] > first[k]) std::memcpy(&lists[first[k]], states[k].data() + 2 * sizeof(uint64_t), (first[k + 1] - first[k]) * sizeof(RibbitTargetShortlists));
    std::vector<RibbitTargetVerdicts> sum(total);
    RibbitPrimerPairParams pair;
    ribbit_primer_pair_params_default(&pair);
    RibbitProductParams product;
    ribbit_product_params_default(&product);
    RibbitFastaReader *reader = nullptr;
    if (ribbit_fasta_open(fasta.c_str(), 1, &reader) != RIBBIT_OK) throw PathError{std::string("--primer-genome-bed: ") + ribbit_fasta_last_error()};
    struct Close { RibbitFastaReader *r; ~Close() { ribbit_fasta_close(r); } } close{reader};
    size_t k = 0;
    for (;; ++k) {
        const char *name = "", *bases = nullptr;
        int64_t length = 0;
        int is_last = 1;
        const int got = ribbit_fasta_next(reader, &name, &bases, &length, &is_last);
        if (got < 0) throw PathError{std::string("--primer-genome-bed: ") + ribbit_fasta_last_error()};
        if (got == 0) break;
        if (k >= states.size()) throw PathError{"--primer-genome-bed: the input has more records than when it was read first"};
        int rc = ribbit_hip_load_record_pinned(h, bases, length);
        // the targets before this record's, its own, those behind them
        const size_t cut[4] = {0, first[k], first[k + 1], total};
        for (int part = 0; part < 3 && rc == RIBBIT_OK; ++part) {
            const size_t from = cut[part], n = cut[part + 1] - from;
            if (n == 0) continue;
            const RibbitTargetVerdicts *verdicts = nullptr;
            rc = ribbit_hip_record_shortlist_verdicts(h, &lists[from], n, part == 1, &pair, &product, &verdicts);
            if (rc != RIBBIT_OK) break;
            if (k == 0) std::memcpy(&sum[from], verdicts, n * sizeof(RibbitTargetVerdicts));
            else rc = ribbit_primer_verdicts_merge(&sum[from], verdicts, n);
        }
        ribbit_fasta_release(reader, bases);
        check(rc);
        if (is_last) { ++k; break; }
    }
    if (k != states.size()) throw PathError{"--primer-genome-bed: the input has fewer records than when it was read first"};
    for (k = 0; k < states.size(); ++k) {
        const size_t n = first[k + 1] - first[k];
        if (n == 0) continue;
        uint64_t head[2];
        std::memcpy(head, states[k].data(), sizeof head);
        const char *lines = states[k].data() + 2 * sizeof(uint64_t) + n * sizeof(RibbitTargetShortlists);
        RibbitRowPrimerPair *pairs = nullptr;
        RibbitRowProducts *products = nullptr;
        RibbitRowSpecific *specific = nullptr;
        char *text = nullptr;
        size_t len = 0;
        int rc = ribbit_primer_shortlists_choose(&lists[first[k]], &sum[first[k]], n, &pair, &pairs, &products, &specific);
        if (rc == RIBBIT_OK && file) rc = ribbit_bed_primer_specific_text(lines, (size_t)head[1], pairs, products, specific, n, &text, &len);
        if (rc == RIBBIT_OK && keep) {
            keep->pairs.insert(keep->pairs.end(), pairs, pairs + n);
            keep->first.push_back(keep->pairs.size());
            keep->lines.append(lines, (size_t)head[1]);
            keep->line_at.push_back(keep->lines.size());
            keep->record.push_back((int32_t)std::min<size_t>(k, (size_t)INT32_MAX));
        }
        ribbit_primer_genome_free(pairs);
        ribbit_primer_genome_free(products);
        ribbit_primer_genome_free(specific);
        check(rc);
        if (file) file->write(text, (std::streamsize)len);
        ribbit_text_free(text);
    }
}

// the column-4 motifs of the kept lines, one per chosen pair (`option` words the refusal)
struct KeptMotifs {
    char *pool = nullptr;
    int32_t *offsets = nullptr;
    KeptMotifs(const KeptMarkers &kept, const char *option) {
        size_t n_motifs = 0;
        check(ribbit_bed_motifs(kept.lines.data(), kept.lines.size(), &pool, &offsets, &n_motifs));
        if (n_motifs != kept.pairs.size()) {
            release();
            throw PathError{std::string(option) + ": the kept lines are not one per chosen pair"};
        }
    }
    KeptMotifs(const KeptMotifs &) = delete;
    KeptMotifs &operator=(const KeptMotifs &) = delete;
    ~KeptMotifs() { release(); }
    void release() { ribbit_text_free(pool); ribbit_intervals_free(offsets); pool = nullptr; offsets = nullptr; }
};

// All kept pairs typed on one assembly, on the handle h: the FASTA is read; every record of it is loaded and nothing is scanned; the
// pairs are typed on it in one call, with the record's index as label; the amplicons are summed in record order into `sum` (one per
// pair), so a pair keeps its first record's product.  names, name_at: the records' names one behind the other (null: not kept).
// What --marker-bed's pass does with the other assembly and --population-list's with every sample; `option` words the refusals.
void type_on_fasta(RibbitHandle *h, const std::string &fasta, const char *option, const KeptMarkers &kept, const KeptMotifs &motifs, std::vector<RibbitRowAmplicon> &sum,
                   std::string *names, std::vector<int32_t> *name_at) {
    const size_t total = kept.pairs.size();
    RibbitProductParams product;
    ribbit_product_params_default(&product);
    RibbitFastaReader *reader = nullptr;
    if (ribbit_fasta_open(fasta.c_str(), 1, &reader) != RIBBIT_OK) throw PathError{std::string(option) + ": " + ribbit_fasta_last_error()};
    struct Close { RibbitFastaReader *r; ~Close() { ribbit_fasta_close(r); } } close{reader};
    for (size_t k = 0;; ++k) {
        const char *name = "", *bases = nullptr;
        int64_t length = 0;
        int is_last = 1;
        const int got = ribbit_fasta_next(reader, &name, &bases, &length, &is_last);
        if (got < 0) throw PathError{std::string(option) + ": " + ribbit_fasta_last_error()};
        if (got == 0) break;
        if (names) {
            *names += name;
            if (names->size() > (size_t)INT32_MAX) throw PathError{std::string(option) + ": the records' names are 2^31 bytes or more"};
            name_at->push_back((int32_t)names->size());
        }
        if (k >= (size_t)INT32_MAX) throw PathError{std::string(option) + ": the records' names are 2^31 bytes or more"};
        const RibbitRowAmplicon *rows = nullptr;
        int rc = ribbit_hip_load_record_pinned(h, bases, length);
        if (rc == RIBBIT_OK) rc = ribbit_hip_record_pair_amplicons(h, kept.pairs.data(), total, motifs.pool, motifs.offsets, (int32_t)k, &product, &rows);
        if (rc == RIBBIT_OK) {
            if (k == 0) std::memcpy(sum.data(), rows, total * sizeof(RibbitRowAmplicon));
            else rc = ribbit_pair_amplicons_merge(sum.data(), rows, total);
        }
        ribbit_fasta_release(reader, bases);
        check(rc);
        if (is_last) break;
    }
}

// The third pass, --marker-bed's, after write_primer_genome, on the handle h: `kept` holds the chosen pairs and the lines of every
// home record that has any, in input order.  All kept pairs are typed on the other FASTA (type_on_fasta); then every home record's
// text is written.
// typed: what --panel-bed's pass takes over (null: not kept): every kept pair's summed amplicon and the marker text, a line per pair
struct TypedMarkers {
    std::vector<RibbitRowAmplicon> amplicons;
    std::string text;
};
void write_markers(RibbitHandle *h, const std::string &fasta, const KeptMarkers &kept, std::ostream &file, TypedMarkers *typed) {
    StageClock c(MARKERS);
    const size_t total = kept.pairs.size();
    if (total == 0) return;      // (no row anywhere: the file stays empty)
    const KeptMotifs motifs(kept, "--marker-bed");
    std::vector<RibbitRowAmplicon> sum(total);
    std::string names;
    std::vector<int32_t> name_at{0};
    type_on_fasta(h, fasta, "--marker-fasta", kept, motifs, sum, &names, &name_at);
    for (size_t k = 0; k + 1 < kept.first.size(); ++k) {
        const size_t from = kept.first[k], n = kept.first[k + 1] - from;
        char *text = nullptr;
        size_t len = 0;
        check(ribbit_bed_marker_text(kept.lines.data() + kept.line_at[k], kept.line_at[k + 1] - kept.line_at[k], &kept.pairs[from], &sum[from], names.data(), name_at.data(),
                                     name_at.size() - 1, n, &text, &len));
        file.write(text, (std::streamsize)len);
        if (typed) typed->text.append(text, len);
        ribbit_text_free(text);
    }
    if (typed) typed->amplicons = std::move(sum);
}

// The fourth pass, --panel-bed's, after write_markers, on the handle h.  The candidates are the kept pairs worth ordering: exactly one
// product over the other assembly, of another size than designed.  Of more than `most`, those with the largest difference are
// taken, among equals the lower pair penalty, then the earlier one; the taken keep the input order.  A candidate's group is its home
// record, its size range the designed and the observed size.  The pools are made on the GPU (ribbit_hip_panel_pools, which needs
// no record loaded) and written by ribbit_bed_panel_text over the candidates' marker lines.
void write_panel(RibbitHandle *h, const KeptMarkers &kept, const TypedMarkers &typed, int pool_size, size_t most, std::ostream &file) {
    StageClock c(PANEL);
    const size_t total = kept.pairs.size();
    if (total == 0) return;
    std::vector<size_t> line_at{0};      // pair i's marker line is typed.text[line_at[i], line_at[i + 1]), its newline included
    for (size_t at = 0; at < typed.text.size(); ++at)
        if (typed.text[at] == '\n') line_at.push_back(at + 1);
    if (line_at.size() != total + 1 || typed.amplicons.size() != total) throw PathError{"--panel-bed: the marker lines are not one per chosen pair"};
    struct Candidate { size_t i; int64_t difference; int32_t group; };
    std::vector<Candidate> taken;
    for (size_t k = 0; k + 1 < kept.first.size(); ++k)
        for (size_t i = kept.first[k]; i < kept.first[k + 1]; ++i) {
            const RibbitRowAmplicon &a = typed.amplicons[i];
            if (kept.pairs[i].left.start < 0 || a.products != 1) continue;
            const int64_t difference = (int64_t)a.end - a.start - kept.pairs[i].product;
            if (difference != 0) taken.push_back(Candidate{i, difference < 0 ? -difference : difference, kept.record[k]});
        }
    if (taken.size() > most) {
        std::sort(taken.begin(), taken.end(), [&](const Candidate &a, const Candidate &b) {
            if (a.difference != b.difference) return a.difference > b.difference;
            if (kept.pairs[a.i].pair_penalty != kept.pairs[b.i].pair_penalty) return kept.pairs[a.i].pair_penalty < kept.pairs[b.i].pair_penalty;
            return a.i < b.i;
        });
        taken.resize(most);
        std::sort(taken.begin(), taken.end(), [](const Candidate &a, const Candidate &b) { return a.i < b.i; });
    }
    if (taken.empty()) return;      // (no marker worth ordering: the file stays empty)
    std::vector<RibbitRowPrimerPair> pairs;
    std::vector<int32_t> extra;
    std::string lines;
    for (const Candidate &t : taken) {
        const RibbitRowAmplicon &a = typed.amplicons[t.i];
        const int32_t designed = kept.pairs[t.i].product, observed = a.end - a.start;
        pairs.push_back(kept.pairs[t.i]);
        extra.insert(extra.end(), {t.group, std::min(designed, observed), std::max(designed, observed)});
        lines.append(typed.text, line_at[t.i], line_at[t.i + 1] - line_at[t.i]);
    }
    RibbitPanelParams params;
    ribbit_panel_params_default(&params);
    params.pool_size = pool_size;
    const RibbitPanelRow *rows = nullptr;
    int32_t pools = 0;
    check(ribbit_hip_panel_pools(h, pairs.data(), extra.data(), pairs.size(), &params, &rows, &pools));
    char *text = nullptr;
    size_t len = 0;
    check(ribbit_bed_panel_text(lines.data(), lines.size(), rows, pairs.size(), &text, &len));
    file.write(text, (std::streamsize)len);
    ribbit_text_free(text);
}

// --population-list: one sample per line, name<TAB>path of its FASTA; empty lines and lines that start with # are skipped.  Read, and
// every path opened, before any file is made and any GPU is touched; a line that will not do ends the run and names itself.
struct Sample { std::string name, path; };
std::vector<Sample> read_population_list(const std::string &path) {
    std::ifstream in(path, std::ios::binary);
    if (!in) die("--population-list: cannot open '" + path + "' for reading");
    std::vector<Sample> samples;
    std::map<std::string, size_t> line_of;
    std::string line;
    for (size_t k = 1; std::getline(in, line); ++k) {
        if (!line.empty() && line.back() == '\r') line.pop_back();
        if (line.empty() || line[0] == '#') continue;
        const std::string where = "--population-list: line " + std::to_string(k) + " of '" + path + "' ";
        const size_t tab = line.find('\t');
        if (tab == std::string::npos) die(where + "is not name<TAB>path");
        if (line.find('\t', tab + 1) != std::string::npos) die(where + "has more than one tab (no name and no path may hold one)");
        Sample sample{line.substr(0, tab), line.substr(tab + 1)};
        if (sample.name.empty()) die(where + "has an empty name");
        if (sample.path.empty()) die(where + "has an empty path");
        if (samples.size() == RIBBIT_ALLELES_MAX_SAMPLES) die(where + "is sample " + std::to_string(RIBBIT_ALLELES_MAX_SAMPLES + 1) + " (at most " + std::to_string(RIBBIT_ALLELES_MAX_SAMPLES) + ")");
        const auto seen = line_of.emplace(sample.name, k);
        if (!seen.second) die(where + "names '" + sample.name + "' again (line " + std::to_string(seen.first->second) + " has it)");
        if (!std::ifstream(sample.path, std::ios::binary)) die(where + "names '" + sample.path + "', which cannot be opened for reading");
        samples.push_back(std::move(sample));
    }
    if (samples.empty()) die("--population-list: '" + path + "' names no sample");
    return samples;
}

// The last pass, --population-list's, after write_primer_genome (and write_markers and write_panel, where they run), on the handle
// h.  Every sample is typed in list order (type_on_fasta) and leaves one int32 per kept pair (ribbit_pair_amplicon_sizes): the
// genotype matrix, sample-major, in host memory.  One call counts every marker's alleles on the GPU (ribbit_hip_marker_alleles,
// which needs no record loaded); then the files are written.
void write_population(RibbitHandle *h, const std::vector<Sample> &samples, const KeptMarkers &kept, std::ostream *allele_file, std::ostream *matrix_file) {
    StageClock c(POPULATION);
    const size_t total = kept.pairs.size(), S = samples.size();
    std::string names;
    std::vector<int32_t> name_at{0};
    for (const Sample &sample : samples) {
        names += sample.name;
        if (names.size() > (size_t)INT32_MAX) throw PathError{"--population-list: the samples' names are 2^31 bytes or more"};
        name_at.push_back((int32_t)names.size());
    }
    std::vector<int32_t> cells(S * total), designed(total), motif_lengths(total);
    const RibbitRowAlleles *rows = nullptr;
    if (total > 0) {
        const KeptMotifs motifs(kept, "--population-list");
        for (size_t i = 0; i < total; ++i) {
            designed[i] = kept.pairs[i].left.start < 0 || kept.pairs[i].right.start < 0 ? 0 : kept.pairs[i].product;
            motif_lengths[i] = motifs.offsets[i + 1] - motifs.offsets[i];
        }
        std::vector<RibbitRowAmplicon> sum(total);
        for (size_t s = 0; s < S; ++s) {
            std::fill(sum.begin(), sum.end(), RibbitRowAmplicon{});
            type_on_fasta(h, samples[s].path, "--population-list", kept, motifs, sum, nullptr, nullptr);
            check(ribbit_pair_amplicon_sizes(sum.data(), total, &cells[s * total]));
        }
        check(ribbit_hip_marker_alleles(h, cells.data(), S, total, designed.data(), motif_lengths.data(), &rows));
    }
    char *text = nullptr;
    size_t len = 0;
    if (allele_file && total > 0) {      // (no row anywhere: the file stays empty)
        check(ribbit_bed_alleles_text(kept.lines.data(), kept.lines.size(), kept.pairs.data(), rows, S, total, &text, &len));
        allele_file->write(text, (std::streamsize)len);
        ribbit_text_free(text);
    }
    if (matrix_file) {      // (the header at least)
        check(ribbit_allele_matrix_text(kept.lines.data(), kept.lines.size(), cells.data(), S, total, designed.data(), names.data(), name_at.data(), &text, &len));
        matrix_file->write(text, (std::streamsize)len);
        ribbit_text_free(text);
    }
}

}  // namespace

int main(int argc, char **argv) {
    Options opt;
    if (!parse_arguments(argc, argv, opt)) return 1;                          // ribbit.cpp:193-195

    OtherBed other;                 // (read before any file is made and any GPU is touched)
    if (!opt.other_path.empty()) {
        read_other_bed(opt.other_path, other);
        opt.settings.other = &other;
    }
    const bool population_on = !opt.population_list.empty();
    std::vector<Sample> samples;      // (read, and every path tried, before any file is made and any GPU is touched)
    if (population_on) samples = read_population_list(opt.population_list);
    std::ofstream file;
    if (!opt.out.empty()) file.open(opt.out);
    std::ostream &out = opt.out.empty() ? std::cerr : file;                   // ribbit.cpp:199-205
    std::array<std::ofstream, N_OUTPUTS> row_file;
    std::array<bool, N_OUTPUTS> row_on;
    for (size_t k = 0; k < N_OUTPUTS; ++k) {
        row_on[k] = !opt.row_path[k].empty();
        if (!row_on[k]) continue;
        row_file[k].open(opt.row_path[k], std::ios::binary);
        if (!row_file[k]) die(std::string("--") + kOutputs[k].option + ": cannot open '" + opt.row_path[k] + "' for writing");
    }

    // --marker-bed and --population-list need --primer-genome-bed's selection, whether or not that file is written: pipe_on says what
    // the records produce
    const bool markers_on = !opt.marker_bed.empty();
    std::array<bool, N_OUTPUTS> pipe_on = row_on;
    pipe_on[GENOME_OUTPUT] = row_on[GENOME_OUTPUT] || markers_on || population_on;
    std::ofstream marker_file;
    if (markers_on) {
        if (!std::ifstream(opt.marker_fasta, std::ios::binary)) die("--marker-fasta: cannot open '" + opt.marker_fasta + "' for reading");
        marker_file.open(opt.marker_bed, std::ios::binary);
        if (!marker_file) die("--marker-bed: cannot open '" + opt.marker_bed + "' for writing");
    }
    const bool panel_on = !opt.panel_bed.empty();
    std::ofstream panel_file;
    if (panel_on) {
        panel_file.open(opt.panel_bed, std::ios::binary);
        if (!panel_file) die("--panel-bed: cannot open '" + opt.panel_bed + "' for writing");
    }
    std::ofstream allele_file, matrix_file;
    if (!opt.allele_bed.empty()) {
        allele_file.open(opt.allele_bed, std::ios::binary);
        if (!allele_file) die("--allele-bed: cannot open '" + opt.allele_bed + "' for writing");
    }
    if (!opt.allele_matrix.empty()) {
        matrix_file.open(opt.allele_matrix, std::ios::binary);
        if (!matrix_file) die("--allele-matrix: cannot open '" + opt.allele_matrix + "' for writing");
    }

    const auto t_run0 = std::chrono::steady_clock::now();
    RibbitRefineParams prm;
    build_refine_params(opt, prm);
    std::cerr << "Minimum motif:\t" << opt.min_motif << "\n";
    std::cerr << "Maximum motif:\t" << opt.max_motif << "\n";
    std::cerr << "Purity threshold: " << 0.85f << "\n";

    RibbitScanParams scan;
    ribbit_scan_params_default(&scan, opt.min_motif, opt.max_motif);
    // GPUs: --devices, else RIBBIT_DEVICES, else --device alone.  Records are independent (ribbit.cpp:269-280 handles them one
    // after the other), so several GPUs simply take different records; a device may be listed twice (two handle sets on it).
    std::vector<int> devices = opt.devices;
    if (devices.empty())
        if (const char *env = std::getenv("RIBBIT_DEVICES"))
            if (!parse_device_list(env, devices)) die(std::string("RIBBIT_DEVICES wants a comma separated list of GPU ordinals, got '") + env + "'");
    if (devices.empty()) devices.push_back(opt.device);
    const int ndev = (int)devices.size();
    RibbitHandle *h = nullptr;
    if (ribbit_hip_open(&scan, devices[0], &h) != RIBBIT_OK) die(std::string("GPU path failed: ") + ribbit_hip_last_error());

    // ---- record pipeline: the reader (this thread) parses records; `jobs` workers per GPU process them on their own
    // handles; results are written in input order.  A record weighs ceil(length / 4 Mbp) of its GPU's `jobs` tokens (at
    // most all of them), so many reads run side by side while a chromosome has one GPU and its share of the host threads
    // to itself.  A free worker takes the LONGEST record of the look-ahead window (the longest-first dealing of
    // independent units over devices, done as the records stream in), but never passes over the oldest record more than
    // 2 x workers times, so the output never waits on a starved record.
    unsigned cores = std::max(1u, std::min(std::thread::hardware_concurrency(), 16u * (unsigned)ndev));
    if (const char *env = std::getenv("RIBBIT_THREADS")) cores = (unsigned)std::max(1, std::atoi(env));
    const unsigned dev_cores = std::max(1u, cores / (unsigned)ndev);      // host threads behind one GPU
    int jobs = (int)std::max(1u, std::min(8u, dev_cores / 2));
    if (const char *env = std::getenv("RIBBIT_JOBS")) jobs = std::max(1, std::atoi(env));
    if (opt.jobs > 0) jobs = opt.jobs;
    jobs = std::min(jobs, 64);
    const int workers = jobs * ndev;
    struct Record { size_t index; std::string name; const char *bases; int64_t length; };
    struct Result { std::string bed, log; std::array<std::string, N_OUTPUTS> rows; };
    std::mutex mu;
    std::condition_variable cv;
    std::deque<Record> queue;
    std::map<size_t, Result> done;
    size_t next_out = 0;
    std::vector<std::string> genome_states;      // --primer-genome-bed: every record's state for the second pass, in input order
    bool reader_done = false;
    bool failed = false;            // some record's GPU path failed: everybody drains
    std::string failure;
    std::vector<int> tokens((size_t)ndev, jobs);
    int front_passed_over = 0;      // how often the oldest queued record has been passed over for a longer one
    std::vector<int64_t> dev_bases((size_t)ndev, 0);      // RIBBIT_PROFILE: bases each GPU has taken
    std::vector<size_t> dev_records((size_t)ndev, 0);
    RibbitFastaReader *reader = nullptr;
    if (ribbit_fasta_open(opt.fasta.c_str(), 1, &reader) != RIBBIT_OK) {
        // the reference's ifstream on a missing file simply yields no lines: one empty, unnamed record (Q4)
        std::cerr << "ribbit-hip: " << ribbit_fasta_last_error() << "\n";
    }

    auto flush_ready = [&]() {                      // call with mu held
        for (auto it = done.find(next_out); it != done.end(); it = done.find(next_out)) {
            std::cerr << it->second.log;
            out.write(it->second.bed.data(), (std::streamsize)it->second.bed.size());
            for (size_t k = 0; k < N_OUTPUTS; ++k) {
                if (k == GENOME_OUTPUT && pipe_on[k]) genome_states.push_back(std::move(it->second.rows[k]));
                else row_file[k].write(it->second.rows[k].data(), (std::streamsize)it->second.rows[k].size());
            }
            done.erase(it);
            ++next_out;
        }
    };
    // heavy: this GPU's first worker.  A record that takes all of a GPU's job tokens runs alone on it, and always on that worker's
    // handle: the buffers of a chromosome (gigabytes of page-locked and device memory, a second to allocate) exist once per
    // GPU, not once per worker (eight handles each meeting their first chromosome cost the whole-genome run 8 of its 83 s).
    auto worker = [&](RibbitHandle *wh, int dev, bool heavy) {
        for (;;) {
            Record rec;
            int weight;
            {
                std::unique_lock<std::mutex> lk(mu);
                size_t pick = 0;
                for (;;) {
                    if (!queue.empty()) {
                        pick = 0;
                        if (front_passed_over < 2 * workers)
                            for (size_t i = 1; i < queue.size() && i < (size_t)workers; ++i)
                                if (queue[i].length > queue[pick].length) pick = i;
                        weight = (int)std::min<size_t>((size_t)jobs, (size_t)queue[pick].length / 4000000 + 1);
                        if (tokens[(size_t)dev] >= weight && (weight < jobs || heavy || jobs == 1)) break;
                    } else if (reader_done) {
                        return;
                    }
                    cv.wait(lk);
                }
                front_passed_over = pick == 0 ? 0 : front_passed_over + 1;
                rec = std::move(queue[pick]);
                queue.erase(queue.begin() + (std::ptrdiff_t)pick);
                tokens[(size_t)dev] -= weight;
                dev_bases[(size_t)dev] += rec.length;
                ++dev_records[(size_t)dev];
            }
            cv.notify_all();
            std::ostringstream bed, log;
            std::array<std::string, N_OUTPUTS> texts;      // (kept in memory until the record's turn to be written)
            const RowJobs row_jobs(pipe_on, [&texts](size_t k) { return [&texts, k](const char *p, size_t n) { texts[k].append(p, n); }; });
            bool ok = true;
            std::string why;
            {
                bool skip;
                { std::lock_guard<std::mutex> lk(mu); skip = failed; }
                if (!skip) {
                    try {
                        check(ribbit_hip_set_host_threads(wh, (int)std::max(1u, dev_cores * (unsigned)weight / (unsigned)jobs)));
                        log << "Processing sequence " << rec.name << "\n";
                        process_sequence(wh, prm, rec.name, rec.bases, rec.length, bed, log, opt.settings, row_jobs);
                    } catch (const PathError &e) { ok = false; why = e.what; }
                }
            }
            ribbit_fasta_release(reader, rec.bases);
            {
                std::lock_guard<std::mutex> lk(mu);
                if (!ok && !failed) { failed = true; failure = why; }
                done[rec.index] = Result{bed.str(), log.str(), std::move(texts)};
                tokens[(size_t)dev] += weight;
                if (!failed) flush_ready();
            }
            cv.notify_all();
        }
    };
    std::vector<RibbitHandle *> handles{h};
    std::vector<int> handle_dev{0};
    for (int j = 1; j < workers; ++j) {
        RibbitHandle *extra = nullptr;
        const int dev = j % ndev;              // worker j serves GPU j mod ndev: every GPU gets `jobs` of them
        if (ribbit_hip_open(&scan, devices[(size_t)dev], &extra) != RIBBIT_OK) { failed = true; failure = std::string("GPU path failed: ") + ribbit_hip_last_error(); break; }
        handles.push_back(extra);
        handle_dev.push_back(dev);
    }
    std::vector<std::thread> pool;
    for (size_t j = 0; j < handles.size(); ++j) pool.emplace_back(worker, handles[j], handle_dev[j], j < (size_t)ndev);      // handles 0 .. ndev-1: one per GPU

    // ribbit.cpp:269-279 -- records as the reference's getline loop delimits them; :280 -- the last record is processed
    // unconditionally and WITHOUT the "Processing sequence" line, also for an empty file (Q4): it bypasses the pipeline
    // once the pipeline has drained
    size_t n_records = 0;
    std::string last_name;
    const char *last_bases = nullptr;
    int64_t last_length = 0;
    for (;;) {
        const char *name = "", *bases = nullptr;
        int64_t length = 0;
        int is_last = 1;
        const int got = reader ? ribbit_fasta_next(reader, &name, &bases, &length, &is_last) : 0;
        if (got < 0) { std::lock_guard<std::mutex> lk(mu); failed = true; failure = ribbit_fasta_last_error(); break; }
        if (got == 0) break;
        if (const auto it = other.by_name.find(name); it != other.by_name.end()) it->second.is_record = true;
        if (is_last) { last_name = name; last_bases = bases; last_length = length; break; }
        std::unique_lock<std::mutex> lk(mu);
        cv.wait(lk, [&] { return queue.size() < (size_t)(2 * workers) || failed; });       // bounded look-ahead
        if (failed) break;
        queue.push_back(Record{n_records++, name, bases, length});
        cv.notify_all();
    }
    {
        std::unique_lock<std::mutex> lk(mu);
        reader_done = true;
        cv.notify_all();
    }
    for (std::thread &t : pool) t.join();
    int status = 0;
    {
        std::lock_guard<std::mutex> lk(mu);
        if (!failed) flush_ready();
    }
    if (!failed) {
        try {
            // The last record runs here, after the workers have gone: every other GPU of --devices is idle by now, so a long last
            // record -- a FASTA with ONE chromosome, above all -- has its refinement dealt over all of them, a slice of the
            // dispatched seeds per GPU with that GPU's share of the host threads (refine_over_devices; scans and merges stay on
            // the first GPU: 0.55 of a chromosome's 2 s).
            std::vector<Helper> helpers;
            for (int d = 1; d < ndev && (size_t)d < handles.size(); ++d) helpers.push_back(Helper{handles[(size_t)d], (int)dev_cores});
            check(ribbit_hip_set_host_threads(h, helpers.empty() ? 0 : (int)dev_cores));
            static const char kNoBases[1] = {0};
            // (every record the reader hands out has its row outputs but the nameless empty one of a file without records, Q4)
            const bool real_last = !(last_name.empty() && last_length == 0);
            std::string last_state;
            const RowJobs row_jobs(real_last ? pipe_on : std::array<bool, N_OUTPUTS>{}, [&row_file, &last_state](size_t k) {
                return [&row_file, &last_state, k](const char *p, size_t n) {
                    if (k == GENOME_OUTPUT) last_state.append(p, n);
                    else row_file[k].write(p, (std::streamsize)n);
                };
            });
            process_sequence(h, prm, last_name, last_bases ? last_bases : kNoBases, last_length, out, std::cerr, opt.settings, row_jobs, &helpers);
            if (pipe_on[GENOME_OUTPUT]) {
                if (real_last) genome_states.push_back(std::move(last_state));
                if (reader) { ribbit_fasta_close(reader); reader = nullptr; }      // (the last record's bases are no longer needed)
                KeptMarkers kept;
                write_primer_genome(h, opt.fasta, genome_states, row_on[GENOME_OUTPUT] ? &row_file[GENOME_OUTPUT] : nullptr, markers_on || population_on ? &kept : nullptr);
                TypedMarkers typed;
                if (markers_on) write_markers(h, opt.marker_fasta, kept, marker_file, panel_on ? &typed : nullptr);
                if (panel_on) write_panel(h, kept, typed, opt.panel_pool_size, (size_t)opt.panel_max, panel_file);
                if (population_on) write_population(h, samples, kept, opt.allele_bed.empty() ? nullptr : &allele_file, opt.allele_matrix.empty() ? nullptr : &matrix_file);
            }
        } catch (const PathError &e) { failed = true; failure = e.what; }
    }
    if (failed) { std::cerr << "ribbit-hip: " << failure << "\n"; status = 1; }
    for (size_t j = 1; j < handles.size(); ++j) ribbit_hip_close(handles[j]);
    ribbit_hip_close(h);
    if (reader) ribbit_fasta_close(reader);
    if (std::getenv("RIBBIT_PROFILE")) {
        char bus[64] = {0};
        for (int d = 0; d < ndev; ++d)
            if (ribbit_hip_device_pci_bus_id(devices[(size_t)d], bus, sizeof bus) == RIBBIT_OK)
                std::cerr << "[device] slot " << d << " is GPU " << devices[(size_t)d] << " at PCI " << bus << "\n";
    }
    if (std::getenv("RIBBIT_PROFILE") && ndev > 1)
        for (int d = 0; d < ndev; ++d)
            std::cerr << "[devices] slot " << d << " (GPU " << devices[(size_t)d] << "): " << dev_records[(size_t)d] << " records, " << dev_bases[(size_t)d] << " bases\n";
    if (!opt.timing.empty()) {
        // (stage times are wall clock per record, summed: with several records in flight their sum exceeds the run's wall time)
        std::ofstream tf(opt.timing);
        const double wall_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_run0).count();
        int64_t total_bases = last_length;
        for (int d = 0; d < ndev; ++d) total_bases += dev_bases[(size_t)d];
        tf << "{\"records\": " << n_records + 1 << ", \"bases\": " << total_bases << ", \"wall_s\": " << wall_s << ", \"status\": " << status
           << ", \"min_motif\": " << opt.min_motif << ", \"max_motif\": " << opt.max_motif << ", \"devices\": " << ndev << ", \"jobs_per_device\": " << jobs
           << ", \"stage_ms_summed_over_records\": {";
        for (int s = 0; s < N_FIXED_STAGES; ++s) tf << (s ? ", \"" : "\"") << kStageNames[s].key << "\": " << g_stage_ms[s];
        for (const Stage s : stages_on(pipe_on)) tf << ", \"" << kStageNames[s].key << "\": " << g_stage_ms[s];
        if (markers_on) tf << ", \"" << kStageNames[MARKERS].key << "\": " << g_stage_ms[MARKERS];
        if (panel_on) tf << ", \"" << kStageNames[PANEL].key << "\": " << g_stage_ms[PANEL];
        if (population_on) tf << ", \"" << kStageNames[POPULATION].key << "\": " << g_stage_ms[POPULATION];
        tf << "}}\n";
    }
    if (std::getenv("RIBBIT_PROFILE")) {
        std::cerr << "[stages, ms over all records]";
        for (int s = 0; s < N_FIXED_STAGES; ++s) std::cerr << (s ? "  " : " ") << kStageNames[s].label << " " << g_stage_ms[s];
        for (const Stage s : stages_on(pipe_on)) std::cerr << "  " << kStageNames[s].label << " " << std::to_string(g_stage_ms[s]);
        if (markers_on) std::cerr << "  " << kStageNames[MARKERS].label << " " << std::to_string(g_stage_ms[MARKERS]);
        if (panel_on) std::cerr << "  " << kStageNames[PANEL].label << " " << std::to_string(g_stage_ms[PANEL]);
        if (population_on) std::cerr << "  " << kStageNames[POPULATION].label << " " << std::to_string(g_stage_ms[POPULATION]);
        std::cerr << "\n";
    }
    size_t ignored = 0, ignored_names = 0;
    for (const auto &group : other.by_name)
        if (!group.second.is_record) { ignored += group.second.n(); ++ignored_names; }
    if (const size_t left_out = g_rows_left_out.load())
        std::cerr << "ribbit-hip: --interruption-bed: " << left_out << " rows whose CIGAR does not span the row were left out\n";
    if (ignored) std::cerr << "ribbit-hip: --overlap-with: " << ignored << " intervals of " << ignored_names << " names that are no record of the input were ignored\n";
    return status;
}
