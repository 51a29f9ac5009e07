/* bsx.h — C ABI of libbsx.so, the MI355X (gfx950) implementation of the BSMAP v2.6 alignment hot path.
 *
 * BSMAP has no plugin/FFI interface; the seam this library replaces is the per-thread C++ object call
 *     a.ImportBatchReads(n, reads); a.Do_Batch(ref);          (reference main.cpp:57-64, :94-102)
 * plus the two start-up calls that produce the data Do_Batch reads:
 *     ref.Run_ConvertBinseq(fin_db); ref.CreateIndex();        (reference main.cpp:462, :174-178)
 * Every entry point below cites the reference interface it stands in for (file:line in the BSMAP
 * v2.6 tree).  Signatures carry plain pointers and sizes only; all device memory is owned by the
 * library behind opaque handles; no call throws or aborts — errors are negative return codes.
 *
 * Host text formatting (SAM/BSP, reference align.cpp:631-765, pairs.cpp:288-498) stays on the host
 * side of this boundary and consumes the numeric records returned here.
 */
#ifndef BSX_H
#define BSX_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define BSX_MAXSNPS 15    /* reference param.h:27 */
#define BSX_MAXHITS 1000  /* reference makefile:4 (-DMAXHITS) */
#define BSX_MAX_READLEN 144 /* reference param.cpp:80 (READ_144) */

enum {
    BSX_OK = 0,
    BSX_ERR_ARG = -1,      /* bad argument / option value (reference: cerr + exit(1), main.cpp:260-265) */
    BSX_ERR_IO = -2,       /* cannot open / parse file (reference main.cpp:457-461) */
    BSX_ERR_NOMEM = -3,    /* host or device allocation failed */
    BSX_ERR_DEVICE = -4,   /* HIP runtime error (see bsx_last_error_detail) */
    BSX_ERR_STATE = -5,    /* call order violated (e.g. align before index build) */
    BSX_ERR_LIMIT = -6,    /* reference limits exceeded (>= 2^32 nt, -v > 15, -w > 1000, -s > 16) */
    BSX_ERR_NODEVICE = -7  /* no usable gfx950 device: the library has NO CPU fallback */
};
const char *bsx_strerror(int code);
const char *bsx_last_error_detail(void); /* thread-local text of the last failing HIP call */

/* ---- parameters: reference class Param (param.h:54-169), option parser main.cpp:234-289 ------- */
typedef struct bsx_params {
    int32_t seed_size;          /* -s  */
    int32_t index_interval;     /* -I  */
    int32_t max_snp_num;        /* -v  */
    int32_t max_num_hits;       /* -w  */
    int32_t chains;             /* -n  */
    int32_t pairend;            /* -b given */
    int32_t min_insert;         /* -m  */
    int32_t max_insert;         /* -x  */
    int32_t report_repeat_hits; /* -r  */
    int32_t randseed;           /* -S  (0 = nondeterministic in the reference; here: treated as seed 0 of the same hash) */
    int32_t qual_threshold;     /* -q  */
    int32_t zero_qual;          /* -z  */
    int32_t max_ns;             /* -f  */
    int32_t max_readlen;        /* -L  */
    int32_t out_sam;            /* affects TrimLowQual's quality rebasing only (align.cpp:64-67) */
    int32_t rrbs;               /* set by bsx_params_set_digest */
    int32_t digest_pos;
    int32_t n_adapter;          /* -A (up to 10) */
    char digest_site[32];
    char adapter[10][128];
    char read_nt, ref_nt;       /* -M */
    char pad_[2];
    /* derived (bsx_params_finish) */
    uint8_t bit_nt[4];          /* 2-bit code of A,C,G,T (Param::SetAlign, param.cpp:187-231) */
    uint8_t profile_a[BSX_MAXSNPS + 1][16]; /* SeedProfile.a (param.cpp:85-93) */
    uint32_t seed_bits;
    int32_t max_seedseg_num;
    uint32_t total_kmers;
} bsx_params;

int bsx_params_default(bsx_params *p);                         /* Param::Param(), param.cpp:6-83 */
int bsx_params_set_digest(bsx_params *p, const char *site);    /* Param::SetDigestionSite, param.cpp:95-106 ("C-CGG") */
int bsx_params_finish(bsx_params *p);                          /* SetAlign + SetSeedSize + InitMapping; validates limits */

/* ---- reference genome: RefSeq::Run_ConvertBinseq (dbseq.cpp:215-282) --------------------------- */
typedef struct bsx_ref bsx_ref;
int bsx_device_count(void);
/* NUMA node the device hangs on (from its PCI address; -1 if unknown): a host program under a CPU quota does well to keep its threads
 * and buffers on that node (bsmap_amd/csrc/bsx_cpus.h) */
int bsx_device_numa_node(int device);
/* parse FASTA text on the host with the reference's tokenisation, pack both strands, upload to `device` */
int bsx_ref_create_from_fasta(const bsx_params *p, const char *text, uint64_t n_bytes, int device, bsx_ref **out);
int bsx_ref_create_from_file(const bsx_params *p, const char *path, int device, bsx_ref **out);
/* deterministic synthetic genome generated ON the device (bench workload) */
int bsx_ref_create_synthetic(const bsx_params *p, uint32_t n_chr, const uint32_t *chr_len, uint64_t seed, int device, bsx_ref **out);
/* text of a synthetic chromosome, positions [from, from+n) (lets tests run the oracle's packer on the same sequence) */
int bsx_synth_chr_text(const bsx_ref *r, uint32_t c, uint32_t from, uint32_t n, char *out);
int bsx_ref_packed_on_device(const bsx_ref *r);   /* 1: the FASTA text was uploaded and packed by kernels (line-regular text of a WGBS reference, csrc/bsx_pack.hip); 0: by the host packer.  Same words either way */
void bsx_ref_destroy(bsx_ref *r);
uint32_t bsx_ref_n_chr(const bsx_ref *r);
uint64_t bsx_ref_n_words(const bsx_ref *r);            /* words per strand copy incl. 2*400 margin (dbseq.h:15) */
uint32_t bsx_ref_n_blocks(const bsx_ref *r);
/* copies out: anchor[n_chr+1], chr_size[n_chr], rc_offset[n_chr]  (RefSeq::ref_anchor, RefTitle, dbseq.h:24-30,113) */
int bsx_ref_info(const bsx_ref *r, uint32_t *anchor, uint32_t *chr_size, uint32_t *rc_offset);
const char *bsx_ref_chr_name(const bsx_ref *r, uint32_t c);
int bsx_ref_blocks(const bsx_ref *r, uint32_t *id, uint32_t *begin, uint32_t *end); /* RefSeq::_blocks, sorted */
int bsx_ref_download_words(const bsx_ref *r, uint32_t *refcat, uint32_t *crefcat);  /* device -> host, n_words each */

/* ---- seed index: RefSeq::CreateIndex (dbseq.cpp:516-539) ---------------------------------------- */
/* (WGBS, -I <= 4: the build can also store, per entry, the 32 reference nt left and right of the entry's seed — the CONTEXT TABLE, 16 bytes per entry,
 *  23.6 GB at hg38 size — for the main kernel's context prefilter, which runs where the work counters are off.  It buys speed, never results, and it must
 *  not take the memory the batches need:
 *    bsx_ref_set_context(r, mode, headroom)  before bsx_index_build.  mode 0: never; 1 (default): only if `headroom` bytes of device memory stay free
 *        behind it (0 = the default, 32 GiB: the fixed part of a 2^22-pair batch — 20.6 GB of per-wave slabs and per-unit arrays — plus the pools'
 *        reserve); 2: whenever it can be allocated, and never dropped.
 *    bsx_ref_context_bytes(r)                what the built index holds (0: none).
 *    bsx_ref_drop_context(r)                 frees it (BSX_ERR_STATE while a batch of the reference exists: a running kernel may hold its address).
 *  In modes 0 / 1 bsx_batch_create itself drops the table and tries once more when the FIRST batch of a reference does not fit beside it.
 *  Test hook: BSX_CTX=0 in the environment builds none.) */
int bsx_ref_set_context(bsx_ref *r, int mode, uint64_t headroom_bytes);
uint64_t bsx_ref_context_bytes(const bsx_ref *r);
int bsx_ref_drop_context(bsx_ref *r);
int bsx_index_build(bsx_ref *r);                        /* built on the GPU; entry order identical to the reference */
uint64_t bsx_index_n_entries(const bsx_ref *r);
/* CSR copy-out: bucket_off[total_kmers+1], bucket_nfwd[total_kmers], entries[n_entries]
 * (WGBS: u32 global positions, RefSeq::index2; RRBS: pairs {tag,loc}, RefSeq::index — 2 words per entry) */
int bsx_index_download(const bsx_ref *r, uint32_t *bucket_off, uint32_t *bucket_nfwd, uint32_t *entries);
uint32_t bsx_ref_n_sites(const bsx_ref *r, uint32_t c);                /* RRBS: RefSeq::CCGG_sites */
int bsx_ref_sites(const bsx_ref *r, uint32_t c, uint32_t *sites);

/* ---- read batches: SingleAlign / PairAlign ImportBatchReads + Do_Batch -------------------------- */
typedef struct bsx_batch bsx_batch;

/* per-read record == what SingleAlign::StringAlign (align.cpp:610-627) hands to the formatter */
typedef struct bsx_hit {
    uint32_t chr;        /* 2*c for the + reference strand copy, 2*c+1 for the - copy (Hit.chr) */
    uint32_t loc;        /* 0-based forward coordinate of the first base (Hit.loc) */
    uint16_t n_best;     /* hits in the best class, both read orientations (<= -w) */
    int8_t best_class;   /* mismatches of the best class; -1 = no hit */
    uint8_t flags;       /* BSX_F_* */
    uint8_t len;         /* read length after trimming (FilterReads) */
    uint8_t max_snp;     /* read_max_snp_num (align.cpp:586) */
    uint8_t seedseg;     /* seedseg_num (align.cpp:440) */
    uint8_t raw_len;     /* length before trimming */
} bsx_hit;
#define BSX_F_FILTERED 1u  /* FilterReads() rejected the read (QC) */
#define BSX_F_CHAIN 2u     /* chosen hit is on the read's reverse-complement orientation (chits) */
#define BSX_F_LIMIT 4u     /* single-end RRBS only: the read matched more than 2^18 distinct places inside the threshold; the set that
                              suppresses duplicate hits overflowed and the record may differ from the reference's */

/* optional per-read class counts: _cur_n_hit[w] / _cur_n_chit[w] (align.h:85-86) */
typedef struct bsx_class_counts { uint16_t n_hit[BSX_MAXSNPS + 1], n_chit[BSX_MAXSNPS + 1]; } bsx_class_counts;

/* per-pair record == PairHit (pairs.h:13-20) chosen by StringAlignPair (pairs.cpp:222-242), plus the
 * two single-mate records StringAlignUnpair (pairs.cpp:244-286) would use */
typedef struct bsx_pair {
    uint32_t a_chr, a_loc, b_chr, b_loc;
    int32_t insert;
    uint16_t n_pairs;    /* pairs in the best pair class */
    int8_t pair_class;   /* na+nb of the best class, -1 none */
    uint8_t chain;       /* PairHit.chain */
    uint8_t na, nb;
    uint8_t paired;      /* PairAlign::RunAlign return value (level+1, 0 = none) */
    uint8_t unpaired_out;/* 1: pair not reported (tmp==1 || paired==0): use a/b below */
    uint32_t pad_;
    bsx_hit a, b;        /* per-mate records; n_best is ma/mb of StringAlignUnpair when unpaired_out */
} bsx_pair;

/* work counters, SURVEY §8(d): 0 n_lookup, 1 n_cand, 2 sum_w (64-bit reference words the reference
 * algorithm touches), 3 n_orient, 4 reads/pairs processed, 5 aligned reads (n_aligned semantics), 6 aligned pairs,
 * 7 candidates evaluated by the scan kernel of the heavy pipeline (k_hscan; a subset of 1 plus the little it evaluates
 * speculatively), 8 their reference words (as 2), 9 / 10 how many of them stopped after the first word / went through all
 * five, 11-14 the share of 0-3 that the main kernel (k_align) did itself — units it did not hand to the heavy pipeline —, so
 * that each kernel's algorithmic bytes can be recomputed from the counters, 15 the part of 7 that was evaluated in groups of two and more
 * tasks over one window and read offset (k_hscan_same: one fetch and shift of the candidates' reference for up to 16 reads), 16 records flagged BSX_F_LIMIT
 * (single-end RRBS reads that matched more than 2^18 distinct places: the one capacity the reference does not have — 0 on every workload seen) */
#define BSX_N_COUNTERS 17

int bsx_batch_create(bsx_ref *r, uint32_t max_units, int paired, bsx_batch **out);
void bsx_batch_destroy(bsx_batch *b);
/* Page-locked host buffers for the arrays handed to bsx_batch_upload_* / bsx_batch_results_*: with them the transfers
 * are plain DMA (the reference has no counterpart: its reads never leave host memory).  Ordinary malloc memory works too. */
int bsx_thread_device(int device);   /* make `device` the calling thread's current GPU (for bsx_pinned_alloc from a helper thread) */
void *bsx_pinned_alloc(size_t bytes);
void bsx_pinned_free(void *p);

/* SoA upload (ImportBatchReads, align.cpp:42-46 / pairs.cpp:27-32): read i = seqs[off[i] .. off[i+1]);
 * quals may be NULL (FASTA input: constant default quality, reads.cpp:108); reads longer than -L are truncated
 * (reads.cpp:115-117).  first_index = ReadInf.index of unit 0 (reads.cpp:97). */
int bsx_batch_upload_se(bsx_batch *b, uint32_t n, const char *seqs, const uint64_t *off, const char *quals, uint32_t first_index);
int bsx_batch_upload_pe(bsx_batch *b, uint32_t n, const char *seqs_a, const uint64_t *off_a, const char *quals_a,
                        const char *seqs_b, const uint64_t *off_b, const char *quals_b, uint32_t first_index);
/* synthetic bisulfite reads sampled ON the device from the resident reference (bench workload) */
int bsx_batch_synth_reads(bsx_batch *b, uint32_t n, uint32_t read_len, uint64_t seed, uint32_t first_index);
/* the same for the other bench workloads: kind 0 plain; 1 trimming workload — qualities with a 3' tail of 10-60 nt
 * at Q2-Q15, 30 % of the fragments 30-149 nt long so that the reads run into the adapter AGATCGGAAGAGC...; 2 RRBS — single
 * reads that start at the digestion sites of an RRBS reference, fragments read_len..220 nt */
int bsx_batch_synth_reads_kind(bsx_batch *b, uint32_t n, uint32_t read_len, uint64_t seed, uint32_t first_index, int kind);
/* Do_Batch (align.cpp:591-606 / pairs.cpp:192-218).  The main kernel is queued on the batch's HIP stream.  Units it hands to the heavy
 * pipeline (reads whose candidate lists run into the tens of thousands) are then taken through passes of control and scan kernels that
 * are chained on the device; the calling thread queues those passes and looks at one counter per two passes to learn when the batch
 * is finished — it SLEEPS on an event meanwhile, it does not spin — so the call returns when the last pass is queued, which for such a
 * batch is close to the end of its device work.  bsx_batch_sync waits for the rest.  To keep a GPU busy through the latency-bound tail
 * of a batch, run two batches per GPU from two host threads (bench.py, the command line): their kernels interleave on the device. */
int bsx_batch_run(bsx_batch *b);
/* the same over units [first_unit, first_unit+n_units) of the uploaded batch (ReadInf.index = first_index + unit) */
int bsx_batch_run_range(bsx_batch *b, uint32_t first_unit, uint32_t n_units);
int bsx_batch_sync(bsx_batch *b);
/* "-p 1 exact" mode (off by default).  The reference never resets SingleAlign::seed_start_offset / seed_array (align.h:82-91):
 * a read with (len - I + 1) % S == 0 is planned with what earlier reads of its stream left there, so with -p 1 its result is a
 * deterministic function of the reads before it (with -p > 1 it depends on thread scheduling).  By default every read starts
 * from zeroed planner state; with this mode on, such reads look their predecessors up — units of the batch,
 * then the history below — and reproduce the single-threaded reference exactly.  History = the reads that precede unit 0 in
 * the input (the tail of the previous batch, up to 65536 reads; quals NULL iff the batch has none). */
int bsx_batch_set_leak_exact(bsx_batch *b, int on);
int bsx_batch_set_history(bsx_batch *b, uint32_t n, const char *seqs_a, const uint64_t *off_a, const char *quals_a, const char *seqs_b,
                          const uint64_t *off_b, const char *quals_b);
/* The same state as an explicit value, for callers that cut an input into batches: `bsx_batch_get_leak_state` returns the planner state
 * behind the last read of the batch's streams (history, then every unit of the batch; a pure function of those reads and of the state
 * before them), `bsx_batch_set_leak_state` makes a state the one before the streams' first read (null: the zero state of a fresh
 * SingleAlign object).  Chaining get -> set from batch to batch reproduces `bsmap -p 1` for any input, however far back the read
 * that set a value lies; no history needs to be attached then.  BSX_LEAK_STATE_BYTES bytes, opaque. */
#define BSX_LEAK_STATE_BYTES 2576
int bsx_batch_set_leak_state(bsx_batch *b, const void *state, size_t bytes);
int bsx_batch_get_leak_state(bsx_batch *b, void *state, size_t bytes);
float bsx_batch_kernel_ms(bsx_batch *b);          /* HIP-event time of the last run's align kernel (after sync) */
/* the scan kernel's launches of the last run: their number and the sum of their HIP-event durations on the stream they
 * were launched on (control kernels of the other unit group may run beside them on another stream).  Passes are queued two
 * chunks ahead of what the host knows (bsx_batch_run), so the count includes the launches queued behind a group's last pass:
 * they find no task, their grids exit at once (tens of microseconds each) and they are part of the sum. */
int bsx_batch_scan_ms(bsx_batch *b, float *total_ms, uint32_t *launches);
/* HIP-event times of the last run by stage, in ms (after sync): out4 = {main kernel k_align (with the exact mode's pre-pass), control kernel k_hctrl summed over
 * its passes, the order kernels between a control pass and its scan, the scan kernel summed over its launches}; each on the stream the kernel is launched on.
 * With ONE batch in flight and one unit group (bench.py's serial replay) no two of them overlap and they add up to the run; with several batches in flight the
 * durations include what ran beside them. */
int bsx_batch_set_stage_timing(bsx_batch *b, int on);   /* off by default: the per-pass events are only recorded for runs queued while it is on */
int bsx_batch_stage_ms(bsx_batch *b, float out4[4], uint32_t *control_passes /* may be NULL */);
int bsx_batch_results_se(bsx_batch *b, bsx_hit *out, bsx_class_counts *counts /* may be NULL */);
int bsx_batch_results_pe(bsx_batch *b, bsx_pair *out, bsx_class_counts *counts_a, bsx_class_counts *counts_b, uint16_t *n_pairs31);
int bsx_batch_counters(bsx_batch *b, uint64_t c[BSX_N_COUNTERS]);   /* accumulated since creation / last reset */
/* Work counters (on by default).  Counters 1-2 and 7-10 count the work the REFERENCE would do on the same reads — candidates, and the
 * 64-bit reference words CountMismatch would touch given its two early-outs (align.h:189-197); SURVEY §8(d)'s algorithmic-byte formula is
 * evaluated with them and the parity suite compares them with the oracle's.  Classifying every candidate of the heavy pipeline's scan by
 * those early-outs is a quarter of the scan kernel's vector instructions and changes no hit: with the counters off the scan kernels skip
 * it (and the control kernel its count-only walks) — every record is identical, counters 0-3 and 7-15 are then incomplete, 4-6 (aligned
 * reads / pairs) stay exact.  The command line runs with them off; bench.py times both and says which is which. */
int bsx_batch_set_work_counters(bsx_batch *b, int on);
int bsx_batch_reset_counters(bsx_batch *b);
/* download the device-resident input reads (for the CPU baseline on device-synthesised input) */
int bsx_batch_download_reads(bsx_batch *b, int mate, char *seqs, uint64_t *off);
int bsx_batch_download_quals(bsx_batch *b, int mate, char *quals);   /* device-synthesised qualities (kind 1), same offsets */
/* test hooks: mode 1 keeps every hit / pair list of every unit (needs max_units small; layout in DESIGN.md);
 * mode 2 records the shader-clock cycles each unit took (diagnostic runs only); 0 switches both off */
int bsx_batch_set_debug(bsx_batch *b, int mode);
int bsx_batch_unit_cycles(bsx_batch *b, uint32_t *cycles_per_unit);
int bsx_batch_ctrl_clocks(bsx_batch *b, uint64_t clocks[24]); /* mode 2: heavy control kernel, wave cycles by category: [0..7] sums, [8..15] longest single span, [16..21] break-down of the longest visit (cycles << 16 | spans) */
int bsx_batch_debug_hits(bsx_batch *b, uint32_t unit, int mate, int orient, int w, uint32_t *chr_loc_pairs, uint32_t cap);
int bsx_batch_debug_pairs(bsx_batch *b, uint32_t unit, int w, uint32_t *pairhits6 /* chain|na<<16|nb<<24, insert, a.chr, a.loc, b.chr, b.loc */, uint32_t cap);
int bsx_batch_debug_plan(bsx_batch *b, uint32_t unit, int mate, int32_t *start_arrays32 /* [2][16] */, int32_t *seedindex32 /* [2][16] */);
/* tuning knob: resident waves per CU for the persistent align kernel (default chosen from register use) */
int bsx_set_waves_per_cu(int waves);
/* tuning knob: candidate-list length (one SnpAlign call, one read orientation) from which a unit is handed to the
 * heavy pipeline (chip-wide scan tasks + resumable control passes); 0 = the library's choice by mode (32768 WGBS, 4096 RRBS),
 * a value no list reaches = never.  Results do not depend on it. */
int bsx_set_heavy_threshold(int n_candidates);
/* pool sizes of the heavy pipeline for batches created afterwards (the defaults follow the batch: bsx_default_heavy_limits returns them — up to 262144 units per round
 * (64 GB of slabs) and 2^22 scan tasks for a 2^22-pair batch —, and bsx_batch_pool_sizes what a batch ended up with); small values only make it take more rounds / passes —
 * used by the tests to exercise those paths; (0, 0) restores the defaults.  The halving below never raises a value set here. */
int bsx_set_heavy_limits(uint32_t units_per_round, uint32_t task_pool);
/* Either way those are STARTING sizes: a batch halves its pools until they fit the device's free memory with a reserve to spare —
 * by default room for one more batch like itself (per-wave slabs + per-unit arrays) plus 4 GB; bsx_set_pool_reserve(bytes) sets the
 * reserve for batches created afterwards (0 = that default).  bsx_batch_pool_sizes returns what a batch ended up with. */
int bsx_set_pool_reserve(uint64_t bytes);
/* the library's own starting sizes for runs of `units` units (a caller whose batches HOLD more units than a run covers — bench.py keeps a ring of
 * steps resident and runs one step at a time with bsx_batch_run_range — passes these to bsx_set_heavy_limits: a batch sizes its pools for the
 * units it was created for) */
int bsx_default_heavy_limits(const bsx_params *p, uint32_t units, int paired, uint32_t *units_per_round, uint32_t *task_pool);
int bsx_batch_pool_sizes(const bsx_batch *b, uint32_t *units_per_round, uint32_t *task_pool);
/* Device bytes a batch of `max_units` will allocate, computed on the host (no device needed): out3 = {per-unit arrays (reads, offsets,
 * records), the main kernel's per-wave slabs for a grid of n_cu x blocks_per_cu blocks, work pools at their starting size}.
 * bench.py checks its whole plan against the device's memory with it before it allocates anything. */
int bsx_batch_plan_bytes(const bsx_params *p, uint32_t max_units, int paired, uint64_t n_entries, uint32_t n_cu, uint32_t blocks_per_cu, uint64_t *out3);
int bsx_batch_last_heavy_units(bsx_batch *b);   /* units the last run handed to the heavy pipeline */
int bsx_batch_last_heavy_list(bsx_batch *b, uint32_t *units, uint32_t cap);   /* their unit numbers inside the batch, in the order the main kernel deferred them (at most cap; returns how many): the tests use it to aim the oracle at them */
int bsx_batch_last_redo_units(bsx_batch *b);    /* of those, units the main kernel had to redo (their duplicate set outgrew the heavy slab; single-end RRBS) */

/* ---- all hits: every equal-best placement of a multi-mapped read or pair ------------------------------------------
 * The record of a read says where ONE of its n_best equal-best placements lies (the reference's formatter prints one, picked by
 * myrand(index) % n_best, align.cpp:610-627).  With a pool attached, the kernel that finishes a unit also copies the best class's
 * whole list out of the unit's slab before the slab is reused — at full batch size, unlike the test hook bsx_batch_set_debug.
 * The records, counts and counters of a run do not depend on the pool in any way; a batch without one allocates nothing for it
 * and its kernels do nothing for it.  (The reference has no counterpart: v2.6 never reports the other placements.)
 *
 * A unit has three spans — [0] the read (single-end) or mate a, [1] mate b, [2] pairs — and emits only what its record does not
 * already say:
 *   single-end read, not filtered, n_best >= 2: span 0 = the best class's forward list, then its reverse-complement list:
 *       n = n_best entries {chr, loc} of two words each, the first n_fwd of them forward; entry myrand(index) % n is the record's
 *       own {chr, loc}, entries from n_fwd on are the ones that carry BSX_F_CHAIN;
 *   reported pair (unpaired_out == 0) with n_pairs >= 2: span 2 = the best pair class's row, n = n_pairs entries of six words
 *       {chain | na<<16 | nb<<24, insert, a.chr, a.loc, b.chr, b.loc} (the layout of bsx_batch_debug_pairs), n_fwd = 0;
 *   pair with unpaired_out == 1: spans 0 / 1 = for each mate that is not filtered and has n_best >= 2, its lists as for a read;
 *   everything else: n = 0.
 * Lists are in the reference's order (what the parity suite compares).  A record flagged BSX_F_LIMIT emits what its lists hold.
 *
 * The pool is one array of 32-bit words that the units of a run share: the wave that finishes a unit reserves the unit's words
 * (all its spans, back to back) from a device-wide cursor.  Which unit lies where depends on scheduling, what a span holds does
 * not: address the pool through the spans only.  A unit whose reservation ends behind the pool is DROPPED: nothing of it is
 * written, its spans have off == BSX_SPAN_DROPPED and still carry n and n_fwd, and the cursor keeps counting — so the need a run
 * reports is exact whatever the pool size.  A caller that sees dropped units sets the pool to the reported words and runs the same
 * units again: results are a pure function of the reads (and of the leak state in exact mode), so that run drops nothing.
 * Needs -r 1 (report_repeat_hits == 1, the default): with -r 0 a scan stops at the second hit of the best class (align.cpp:210)
 * and the list is cut short by design. */
typedef struct bsx_span {
    uint64_t off;    /* first word of the span in the pool, or BSX_SPAN_DROPPED */
    uint32_t n;      /* entries: placements (two words each) in spans 0 and 1, pairs (six words each) in span 2 */
    uint32_t n_fwd;  /* spans 0 and 1: how many of them are on the read's forward orientation (they come first) */
} bsx_span;
#define BSX_SPAN_DROPPED UINT64_MAX   /* value of off: the unit did not fit; n and n_fwd are still right */
/* attach a pool of pool_words words (device memory: 4 bytes per word, plus 48 bytes per unit of the batch for the spans), replace the
 * one attached, or with 0 detach and free it.  BSX_ERR_ARG unless the batch's parameters have -r 1; BSX_ERR_NOMEM */
int bsx_batch_set_all_hits(bsx_batch *b, uint64_t pool_words);
/* after a run (waits for it): the words the last run's units wanted in all — dropped units included —, and how many units it dropped.
 * Spans and cursor start from zero at every bsx_batch_run / bsx_batch_run_range.  BSX_ERR_STATE without a pool or a run */
int bsx_batch_all_hits_need(bsx_batch *b, uint64_t *words, uint32_t *dropped_units);
/* spans[units of the last run][3]; bsx_batch_run_range: entry 0 belongs to its first_unit */
int bsx_batch_all_hits_spans(bsx_batch *b, bsx_span *spans);
/* the used part of the pool: min(need, pool size) words, BSX_ERR_ARG if cap_words is smaller; used_words may be NULL; words NULL: the size only */
int bsx_batch_all_hits_fetch(bsx_batch *b, uint32_t *words, uint64_t cap_words, uint64_t *used_words);

/* ---- measurement aid ("report both peak and a measured ceiling") -----------------------------------
 * Memory rates of `device` in GB/s (1e9 bytes): streaming read of `bytes`, streaming copy (read + write counted), and
 * 16-byte loads at random 4-byte-aligned addresses inside a window of `gather_window_bytes` — the access pattern of the
 * candidate scan (useful bytes = 16 per load; *_Gloads_per_s = 1e9 loads/s).  Not on the alignment path. */
int bsx_probe_memory(int device, uint64_t bytes, uint64_t gather_window_bytes, double *read_GBps, double *copy_GBps, double *gather16_GBps,
                     double *gather16_Gloads_per_s);

/* ---- methylation-ratio pile-up (reference: methratio.py of the BSMAP tree) ---------------------------
 * The reference walks the alignments in Python and increments two per-position counters; here that part runs on the
 * GPU with atomic counters in HBM.  The caller (bsmap_amd/methratio.py) keeps the reference's option parsing, FASTA and
 * BSP/SAM line parsing (get_alignment's filters, methratio.py:31-48) and prints the table (methratio.py:130-151). */
typedef struct bsx_meth bsx_meth;
/* meth/depth arrays for chromosomes of the given lengths (methratio.py:79-83); rm_dup != 0 also allocates the
 * fragment-end table of -r (methratio.py:50-54) */
int bsx_meth_create(uint32_t n_chr, const uint64_t *chr_len, int rm_dup, int device, bsx_meth **out);
/* the same from the reference FASTA (methratio.py:67-77: name = first token of the header, lines stripped and joined, upper case);
 * chroms_csv = the -c list or NULL.  The names are kept: chr_names / order may then be NULL in the calls below. */
int bsx_meth_create_from_fasta(const char *path, const char *chroms_csv, int rm_dup, int device, bsx_meth **out);
uint32_t bsx_meth_n_chr(const bsx_meth *m);
const char *bsx_meth_chr_name(const bsx_meth *m, uint32_t chr);
void bsx_meth_destroy(bsx_meth *m);
int bsx_meth_set_reference(bsx_meth *m, uint32_t chr, const char *upper_seq /* chr_len[chr] letters, upper case */);
/* n alignments in input order: chromosome id, 0-based position, strand code (0 "++", 1 "-+", 2 "+-", 3 "--"), insert size
 * (BSP column 8 / SAM TLEN), cut_at (SAM with insert > 0: PNEXT-1, methratio.py:64; otherwise -1), read letters as
 * concatenated bytes + offsets.  Duplicate removal (first alignment in input order wins), fill-in trimming with
 * trim_fillin, the bounds test and the counter updates of methratio.py:50-63,100-114 happen on the device. */
int bsx_meth_add(bsx_meth *m, uint32_t n, const uint32_t *chr, const int64_t *pos, const uint8_t *strand, const int32_t *insert, const int64_t *cut_at,
                 const char *seqs, const uint64_t *seq_off, uint32_t trim_fillin);
/* the same for a whole BSMAP mapping file (sam = 0 BSP text, 1 SAM text, 2 BAM): the file is memory-mapped and parsed by host
 * threads with get_alignment's filters (NM/QC or unmapped, -u unique, -p pair, chromosome known; methratio.py:31-48), alignments
 * keep the file's order; chr_names[n_chr] in id order */
int bsx_meth_add_file(bsx_meth *m, const char *path, int sam, const char *const *chr_names, int unique, int pair, uint32_t trim_fillin, uint64_t *n_lines);
/* Cycle trimming (extension): in every later bsx_meth_add / bsx_meth_add_file a call at sequencing cycle c (the letter's 0-based index in
 * the untrimmed read of n0 letters in sequencing direction: j for "++" / "--", n0-1-j for "-+" / "+-") is ignored when c < trim5 or
 * c >= n0 - trim3.  Calls only: position, bounds tests, duplicate removal and the count of valid mappings do not change; a letter has
 * to survive trim_fillin and cut_at as well. */
int bsx_meth_set_cycle_trim(bsx_meth *m, uint32_t trim5, uint32_t trim3);
/* M-bias tally (extension): with on != 0 allocates (zeroed) cells[4 strand codes][4 contexts: CG, CHG, CHH, other][BSX_MBIAS_CYCLES][0 unmethylated,
 * 1 methylated] in HBM and every later add counts each call that enters depth / meth in its cell; calls at cycles >= BSX_MBIAS_CYCLES go to one
 * overflow counter.  The tally accumulates over calls and files; bsx_meth_combine_cpg does not touch it.  on == 0 frees it.  BSX_ERR_STATE once
 * alignments have been added. */
#define BSX_MBIAS_CYCLES 1024
int bsx_meth_set_mbias(bsx_meth *m, int on);
/* the tally so far; overflow_calls may be NULL.  BSX_ERR_STATE when the M-bias is off */
int bsx_meth_mbias_fetch(bsx_meth *m, uint64_t *cells /* [4][4][BSX_MBIAS_CYCLES][2] */, uint64_t *overflow_calls);
/* the tally as a tab-separated file: header "strand context cycle meth depth ratio"; rows by strand (++ -+ +- --), context (CG CHG CHH CN) and
 * 1-based cycle up to the last cycle with a call in any group, ratio "%.3f" or NA at depth 0; then "# total <context> <meth> <depth> <ratio>"
 * per context (tab-separated, over the cells) and "# calls beyond cycle 1024: <n>".  BSX_ERR_STATE when the M-bias is off */
int bsx_meth_write_mbias(bsx_meth *m, const char *path);
/* C/T-SNP correction (extension; -i of later BSMAP releases): a genomic C->T SNP looks like an unmethylated C on the strand that carries the C, and
 * the reads of the OTHER reference strand tell the two apart: G over an intact C, A over a SNP.  mode 0 off, 1 correct, 2 skip; another value is
 * BSX_ERR_ARG.  A non-zero mode allocates (zeroed) one uint64 per reference letter — low word rev_GA, high word rev_G — and every later add makes, beside
 * the calls of depth / meth and under the same window and cycle mask, one 64-bit atomic add per opposite-strand letter: a "+?" read over a reference G
 * that shows G adds to rev_G and rev_GA, one that shows A to rev_GA; a "-?" read over a reference C likewise with C and T.  bsx_meth_combine_cpg folds
 * the cells like depth / meth.  Rows (bsx_meth_report_chr, bsx_meth_write_table), tested in this order: depth >= min_depth; the context filter; mode 2
 * drops a position with rev_G != rev_GA, mode 1 one with rev_G == 0 < rev_GA, both one with depth 0; then n_covered += 1 and sum_depth += depth (the raw
 * depth); then methylated > 0 or meth0.  The table gets the columns chr pos strand context ratio eff_CT_count C_count CT_count rev_G_count rev_GA_count
 * CI_lower CI_upper with eff = rev_G != rev_GA ? depth * rev_G / rev_GA : depth ("%.2f"), ratio = min(methylated, eff) / eff and the Wilson interval over
 * eff.  Going between 0 and non-zero is BSX_ERR_STATE once alignments have been added, between 1 and 2 is allowed at any time (the counters are the
 * same: one pile-up can write both tables); BSX_ERR_NOMEM when the array cannot be had; mode 0 before any add frees it. */
int bsx_meth_set_ct_snp(bsx_meth *m, int mode);
/* Context filter (extension; -x of later BSMAP releases) of the later report / write calls, at any time: bit 0 CG, 1 CHG, 2 CHH, 3 other (the classes
 * of the M-bias tally, from the position's own letter: C looks right, G looks left).  A position whose class is not in the mask is not covered: no
 * row, not in n_covered / sum_depth.  0 and 0xF: no filter.  mask > 0xF is BSX_ERR_ARG. */
int bsx_meth_set_contexts(bsx_meth *m, uint32_t mask);
int bsx_meth_combine_cpg(bsx_meth *m);                      /* -g, methratio.py:118-128 */
int bsx_meth_valid_mappings(bsx_meth *m, uint64_t *n);      /* "total %d valid mappings" */
/* rows of one chromosome's table in position order: positions with depth >= min_depth and (methylated > 0 or meth0);
 * n_covered / sum_depth count every position with depth >= min_depth (methratio.py:138-142) */
int bsx_meth_report_chr(bsx_meth *m, uint32_t chr, uint32_t min_depth, int meth0, uint32_t *n_rows, uint64_t *n_covered, uint64_t *sum_depth);
int bsx_meth_fetch_rows(bsx_meth *m, uint32_t *pos0, uint32_t *depth, uint32_t *meth);   /* the rows of the last report_chr */
/* rev_G / rev_GA of the same rows; BSX_ERR_STATE when the C/T-SNP mode is 0 */
int bsx_meth_fetch_rows_snp(bsx_meth *m, uint32_t *rev_g, uint32_t *rev_ga);
/* the whole table file of methratio.py:130-151 (header, chromosomes in the given order — the reference sorts the names —,
 * ratio and Wilson interval with the reference's arithmetic, "%.3f"); returns the counts of the summary line */
int bsx_meth_write_table(bsx_meth *m, const char *path, uint32_t n_order, const uint32_t *order, const char *const *chr_names, uint32_t min_depth, int meth0,
                         uint64_t *n_covered, uint64_t *sum_depth);
/* Pooled methylation per interval and per fixed bin (extensions; -w / -b of later BSMAP releases, and BED intervals), from the counters as they stand,
 * under the handle's current C/T-SNP mode and context mask.  A position is a SITE when the row rule above holds for it (min_depth, the context filter,
 * the SNP tests) and its raw depth is above 0; meth0 plays no part.  Per site, with d the raw depth, m the methylated count, g / ga the rev cells:
 * e = d << 16, or with the mode on and g != ga rint(((double)d * g / ga) * 65536.0) — the table's effective depth in units of 1/65536 —, and
 * mc = min(m << 16, e).  Per interval five uint64 sums over its sites: N (sites), M = sum m, D = sum d, E = sum e, MC = sum mc; the pooled ratio is
 * (double)MC / (double)E and the effective depth E / 65536.0.  Integer sums: the same bits on every call.  The calls change no counter and may be made
 * any number of times, before or after bsx_meth_write_table and bsx_meth_combine_cpg. */
uint32_t bsx_meth_region_tile(void);   /* positions per wave of bsx_meth_regions: a longer interval is cut into tiles of this size (csrc/bsx_meth_tiles.h) */
/* n intervals [start, end) of chromosome chr, 0-based, in any order, overlapping or repeated; end beyond the chromosome is clipped to its length, start
 * then to end.  BSX_ERR_ARG: chr out of range, start > end, a null pointer with n > 0.  n == 0 is BSX_OK.  BSX_ERR_NOMEM */
int bsx_meth_regions(bsx_meth *m, uint32_t n, const uint32_t *chr, const uint32_t *start, const uint32_t *end,
                     uint32_t min_depth, uint64_t *sums /* [n][5]: N, M, D, E, MC */);
/* the bins of one chromosome: bin j holds the positions [j * bin, min((j + 1) * bin, length)), there are length / bin + 1 of them (the last may be
 * empty) and that number comes back in n_bins.  BSX_ERR_ARG: chr out of range, bin == 0, a null m or n_bins; also sums == NULL or n_bins_cap below the
 * number of bins, with n_bins set (a call with sums == NULL asks for the size).  BSX_ERR_NOMEM when the bin array cannot be had on the device */
int bsx_meth_bins(bsx_meth *m, uint32_t chr, uint32_t bin, uint32_t min_depth, uint64_t n_bins_cap,
                  uint64_t *sums /* [n_bins][5] */, uint64_t *n_bins);
/* The intervals of a BED file (columns separated by tabs or spaces: name, start, end, optional label; empty lines and lines that start with '#', "track"
 * or "browser" are skipped; CRLF and a last line without newline are accepted) as a table in the file's order: header
 * "chr start end name n_C methy_C total_C eff_CT ratio CI_lower CI_upper" (tab-separated), then per record the clipped coordinates, the label or ".",
 * N, M, D, E / 65536.0 ("%.2f"), the pooled ratio ("%.3f") and the table's Wilson interval over that depth and ratio; "0 0 0 0.00 NA NA NA" without a
 * site.  A record on a sequence the handle does not hold is dropped and counted in n_dropped.  A line with fewer than three columns, a start or end that
 * is not 1-18 decimal digits, or start > end: BSX_ERR_IO with the line's number in bsx_last_error_detail, and nothing is written.  Needs a handle that
 * knows its names (bsx_meth_create_from_fasta), else BSX_ERR_ARG.  n_written / n_dropped may be NULL. */
int bsx_meth_write_regions(bsx_meth *m, const char *bed_path, const char *out_path, uint32_t min_depth,
                           uint64_t *n_written, uint64_t *n_dropped);
/* A wiggle track of the pooled ratio per bin: "track type=wiggle_0", then for every chromosome in sorted name order (the table's)
 * "variableStep chrom=<name> span=<bin>" and for every bin with a site, ascending, "<j * bin + 1><TAB><ratio %.3f>".  BSX_ERR_ARG for bin == 0 or a
 * handle without names. */
int bsx_meth_write_wig(bsx_meth *m, const char *path, uint32_t bin, uint32_t min_depth);
/* Per-read calls (extensions).  A CALL is what an add puts into depth: a letter of a valid alignment's window over the read strand's own
 * cytosine (reference C under a "+?" read, G under a "-?" read) that shows the unconverted or the converted letter at a cycle that bsx_meth_set_cycle_trim
 * does not mask; the reverse calls of the C/T-SNP mode are none.  Its context class is the M-bias tally's (0 CG, 1 CHG, 2 CHH, 3 other; a chromosome end
 * counts as no letter).  Per valid alignment (per line: the mates of a pair are two reads): n_cg / m_cg = its class-0 calls and the methylated ones among
 * them, n_ch / m_ch = the same over classes 1 and 2 together; class 3 enters nothing.  Three features use these counts, each off by default; with all three
 * off an add does exactly what it did without them.
 *
 * Non-conversion filter (filter_non_conversion of Bismark): with n >= 1 a valid alignment with m_ch >= n in a LATER add is dropped: it adds nothing to depth,
 * meth, the C/T-SNP cells, the M-bias tally or the PDR cells, is not a valid mapping (bsx_meth_valid_mappings) and is counted in bsx_meth_nonconv_dropped.
 * The duplicate filter of rm_dup runs first, on all alignments: a dropped read that owns a fragment end still suppresses its duplicates.  n = 0: off.  May be
 * set at any time. */
int bsx_meth_set_nonconv(bsx_meth *m, uint32_t n);
int bsx_meth_nonconv_dropped(bsx_meth *m, uint64_t *n);
/* Read histogram: with on != 0 allocates (zeroed) the cells below and every later add tallies every valid alignment, those the filter then drops
 * included (the histogram does not depend on the filter's threshold: it is what the threshold is read from).  cg[n][m], 0 <= m <= n <= BSX_RS_CG_MAX:
 * reads with n_cg == n and m_cg == m; ch[k], k = min(m_ch, BSX_RS_CH_MAX): reads by methylated non-CpG calls, the last cell is "BSX_RS_CH_MAX or more";
 * totals: reads, cg_over (reads with n_cg > BSX_RS_CG_MAX, in no cg cell), ch_calls (sum of n_ch), ch_meth (sum of m_ch).  on == 0 frees it.  BSX_ERR_STATE
 * once alignments have been added. */
#define BSX_RS_CG_MAX 31
#define BSX_RS_CH_MAX 63
int bsx_meth_set_read_stats(bsx_meth *m, int on);
/* the histogram so far; every pointer is needed (BSX_ERR_ARG).  BSX_ERR_STATE when the histogram is off */
int bsx_meth_read_stats_fetch(bsx_meth *m, uint64_t *cg /* [BSX_RS_CG_MAX + 1][BSX_RS_CG_MAX + 1] */, uint64_t *ch /* [BSX_RS_CH_MAX + 1] */,
                              uint64_t *totals /* [4]: reads, cg_over, ch_calls, ch_meth */);
/* the histogram as a tab-separated file: header "kind calls meth reads"; "CG <n> <m> <count>" per non-zero cg cell, n then m ascending; "CG >31 . <cg_over>";
 * "CH . <k> <count>" for k = 0..62 and "CH . 63+ <count>", zeros included; then "# reads <reads>", "# CH calls <ch_calls>", "# CH methylated <ch_meth>" and
 * "# CH ratio <ch_meth / ch_calls as %.5f, or NA without a call>".  BSX_ERR_STATE when the histogram is off */
int bsx_meth_write_read_stats(bsx_meth *m, const char *path);
/* Proportion of discordant reads (PDR; Landau et al., Cancer Cell 2014): with min_cpg >= 1 a valid, not dropped alignment with n_cg >= min_cpg is ELIGIBLE,
 * and DISCORDANT when 0 < m_cg < n_cg.  Every CG call of an eligible read adds one to `reads` at the call's reference position (the C under "+?" reads,
 * the G under "-?" reads) and, if the read is discordant, one to `discordant` there.  One zeroed uint64 per reference letter, low word reads, high word
 * discordant, allocated by the first non-zero min_cpg (BSX_ERR_NOMEM when it cannot be had); bsx_meth_combine_cpg folds the cells like depth / meth.
 * min_cpg = 0: off, frees the cells.  Going between 0 and non-zero is BSX_ERR_STATE once alignments have been added; another non-zero value applies to
 * later adds at any time. */
int bsx_meth_set_pdr(bsx_meth *m, uint32_t min_cpg);
/* PDR rows of one chromosome in position order: the positions with reads >= min_reads (min_reads >= 1, else BSX_ERR_ARG), whatever min_depth, the context
 * filter and the C/T-SNP mode are.  BSX_ERR_STATE when PDR is off */
int bsx_meth_pdr_report_chr(bsx_meth *m, uint32_t chr, uint32_t min_reads, uint32_t *n_rows);
int bsx_meth_pdr_fetch_rows(bsx_meth *m, uint32_t *pos0, uint32_t *reads, uint32_t *discordant);   /* the rows of the last pdr_report_chr */
/* the PDR rows of every chromosome in sorted name order (the table's) as a tab-separated file: header "chr pos strand reads discordant PDR", rows with the
 * 1-based position, "+" over a C and "-" over a G, and discordant / reads as "%.3f".  Needs a handle that knows its names, else BSX_ERR_ARG; n_rows may be
 * NULL.  BSX_ERR_STATE when PDR is off */
int bsx_meth_write_pdr(bsx_meth *m, const char *path, uint32_t min_reads, uint64_t *n_rows);

/* Epiallele patterns per window of four neighbouring CpGs (an extension; the input of epipolymorphism, Landan et al. 2012, methylation entropy, Xie et al.
 * 2011, and methclone-style comparisons).  Off by default; with it off bsx_meth_add launches what it launches without it.
 *
 * A reference CpG is a C followed by a G inside one sequence (a C at the end of one sequence and a G at the start of the next are none).  The CpGs of a
 * sequence are numbered 0, 1, .. in position order (the ORDINAL) and identified by the position of their C on both strands.  The CpGs of a read are the
 * reference CpGs whose call position (the C under a "+?" read, the G under a "-?" read) lies in the read's window; the read shows each of them as M (a CG call
 * with the unconverted letter), U (a CG call with the converted letter) or X (anything else: another letter, N, a cycle masked by bsx_meth_set_cycle_trim).
 * A WINDOW is four CpGs with consecutive ordinals o .. o+3 of one sequence.  A valid alignment that the non-conversion filter has not dropped adds one to
 * cell[o][pattern] of every window whose four CpGs are all CpGs of the read and none of them X; bit j of `pattern` (j = 0: the leftmost CpG) is set when
 * CpG o+j is M.  Both strands feed the same cells; mates are two reads.  min_depth, the context filter, the C/T-SNP mode and bsx_meth_combine_cpg do not
 * touch the cells.  Device memory: sixteen uint32 per reference CpG, 4 bytes per CpG for its position and 4 bytes per 64 reference letters for the rank
 * directory, built by kernels at the first add, report or bsx_meth_n_cpg that needs them.  bsx_meth_set_reference after that discards the index AND the
 * cells: set the whole reference before the first add.  The reference must be shorter than 2^33 letters (BSX_ERR_LIMIT).
 *
 * On or off only before the first add, otherwise BSX_ERR_STATE.  Every call below gives BSX_ERR_STATE while it is off, and BSX_ERR_ARG for a null handle
 * or a null out pointer before any device call. */
int bsx_meth_set_epi(bsx_meth *m, int on);
int bsx_meth_n_cpg(bsx_meth *m, uint32_t chr, uint64_t *n);   /* the number of reference CpGs of one sequence */
/* Epiallele rows of one sequence in ordinal order: the windows whose sixteen cells sum to at least min_reads (min_reads >= 1, else BSX_ERR_ARG).  The row
 * buffers are its own: the rows of the last bsx_meth_report_chr and bsx_meth_pdr_report_chr stay fetchable. */
int bsx_meth_epi_report_chr(bsx_meth *m, uint32_t chr, uint32_t min_reads, uint32_t *n_rows);
/* the rows of the last epi_report_chr: pos0[n_rows][4] the 0-based positions of the four Cs, counts[n_rows][16] the cells by pattern */
int bsx_meth_epi_fetch_rows(bsx_meth *m, uint32_t *pos0, uint32_t *counts);
/* The epiallele rows of every sequence in sorted name order (the table's) as a tab-separated file.  Header: "chr pos1 pos2 pos3 pos4 reads meth mean epipoly
 * entropy" and the sixteen patterns as four letters U / M in CpG order, UUUU MUUU UMUU MMUU .. MMMM (pattern 0 .. 15).  A row: the name, the four 1-based
 * positions of the Cs, reads = the sum of the counts, meth = the methylated calls (sum of popcount(k) * n_k), mean = meth / (4 * reads) as "%.3f",
 * epipolymorphism 1 - sum p_k^2 and entropy -1/4 sum p_k log2 p_k as "%.4f" with p_k = n_k / reads in double precision, then the sixteen counts.  A file
 * without rows is the header alone.  Needs a handle that knows its names, else BSX_ERR_ARG; n_rows may be NULL. */
int bsx_meth_write_epi(bsx_meth *m, const char *path, uint32_t min_reads, uint64_t *n_rows);

/* Differential methylation of two samples (an extension).  A and B are two handles on the same device with the same number of sequences and
 * the same length of each (BSX_ERR_ARG otherwise), both with the C/T-SNP mode off (BSX_ERR_STATE otherwise) and with the same context mask (BSX_ERR_ARG
 * otherwise); a == b is allowed.  The letters and the names are A's.  The calls change no counter of either handle and may be made any number of times,
 * before or after bsx_meth_combine_cpg and the table; a process that never makes them runs what it ran without them.
 *
 * Position k is a COMMON SITE when the row rule of bsx_meth_report_chr (min_depth of the call, the context filter) holds for it in A and in B and its raw
 * depth is above 0 in both; its counts are mA, dA, mB, dB (methylated, depth; m <= d).  p is the two-sided Fisher exact test of [[mA, dA - mA], [mB, dB - mB]]
 * with R's rule for ties: over x in [max(0, mA + mB - dB), min(dA, mA + mB)] with w(x) = C(dA, x) C(dB, mA + mB - x),
 * p = sum{w(x) : w(x) <= w(mA) (1 + 1e-7)} / sum w(x), in double precision by the ratio recurrence from the mode (csrc/bsx_meth_diff.h: no lgamma, no
 * floating-point atomics; two calls give the same bits, a support of one table gives exactly 1.0; relative error at most 64 (s + 16) 2^-53 for a support
 * of s tables while p >= 1e-290, and a result in [0, 1e-289] below that).  Per interval five uint64 sums over its common sites: N, MA, DA, MB, DB, and p is
 * the same test on the four sums taken as doubles, NaN where N == 0.
 *
 * Rows of one sequence in position order: the common sites with |mA dB - mB dA| 1000 >= min_delta_permille dA dB (compared as 128-bit integers; 0 keeps
 * every common site, above 1000 is BSX_ERR_ARG).  The row buffers are A's own: the rows of A's other reports stay fetchable. */
int bsx_meth_diff_report_chr(bsx_meth *a, bsx_meth *b, uint32_t chr, uint32_t min_depth, uint32_t min_delta_permille, uint32_t *n_rows);
/* the rows of the last diff_report_chr with `a` as sample A: 0-based positions, counts[n_rows][4] = mA, dA, mB, dB, and p[n_rows] */
int bsx_meth_diff_fetch_rows(bsx_meth *a, uint32_t *pos0, uint32_t *counts, double *p);
/* The rows of every sequence in sorted name order (the table's) as a tab-separated file: header "chr pos strand context C_a CT_a ratio_a C_b CT_b ratio_b
 * delta p"; the 1-based position, "+" over a C and "-" over a G, the context class (CG CHG CHH CN), the counts, the ratios (double)m / d as "%.3f",
 * delta = ratio_b - ratio_a as "%+.3f" and p as "%.4e".  max_p == NULL: every row; otherwise the writer lists the rows with p <= *max_p (the report and
 * the fetch always give every row).  n_rows (may be NULL): the rows written.  Needs a handle `a` that knows its names, else BSX_ERR_ARG. */
int bsx_meth_write_diff(bsx_meth *a, bsx_meth *b, const char *path, uint32_t min_depth, uint32_t min_delta_permille, const double *max_p, uint64_t *n_rows);
/* n intervals under the coordinate rules of bsx_meth_regions (clipping, BSX_ERR_ARG cases, n == 0); sums[n][5] = N, MA, DA, MB, DB and p[n] */
int bsx_meth_diff_regions(bsx_meth *a, bsx_meth *b, uint32_t n, const uint32_t *chr, const uint32_t *start, const uint32_t *end, uint32_t min_depth, uint64_t *sums,
                          double *p);
/* The intervals of a BED file, under the BED rules and the error behaviour of bsx_meth_write_regions, in the file's order: header "chr start end name n_C
 * C_a CT_a ratio_a C_b CT_b ratio_b delta p", the numbers formatted as in bsx_meth_write_diff; a record without a common site is "0 0 0 NA 0 0 NA NA NA". */
int bsx_meth_write_diff_regions(bsx_meth *a, bsx_meth *b, const char *bed_path, const char *out_path, uint32_t min_depth, uint64_t *n_written, uint64_t *n_dropped);
/* The bins [j bin, min((j + 1) bin, length)) of every sequence in sorted name order, as intervals of bsx_meth_diff_regions: the same columns without
 * "name", and only the bins with N > 0; n_rows (may be NULL): the bins written.  bin == 0 is BSX_ERR_ARG. */
int bsx_meth_write_diff_bins(bsx_meth *a, bsx_meth *b, const char *path, uint32_t bin, uint32_t min_depth, uint64_t *n_rows);

/* Benjamini-Hochberg q-values over all rows, and de novo differentially methylated regions (an extension).
 *
 * The FAMILY is every common site (the definition above, under min_depth and the context mask) of every loaded sequence, listed in the writer's sequence
 * order (sorted names as in bsx_meth_write_diff; the ids' order for a handle without names), ascending position within a sequence; n is its size.  No
 * filter of a writer (min_delta_permille, max_p, max_q) shrinks it: filters choose what is written.
 * q: with the family's p-values sorted ascending, p_(1) <= .. <= p_(n), r_k = (p_(k) (double)n) / (double)k (two separately rounded double operations,
 * the product first) and q_(k) = min(1.0, min over j >= k of r_j); a row gets the q of its p, equal p get equal q.  A NaN p (an interval with N == 0) is
 * outside the family: it does not count in n and its q is NaN ("NA" in the files).  Minima are exact in any order and a product followed by a quotient
 * cannot be contracted, so q is bit-identical to the same formula in numpy on the same p, and two calls give the same bits (no floating-point atomics).
 * A CANDIDATE is a row of the family with q <= max_q that passes the delta rule of bsx_meth_diff_report_chr under min_delta_permille and whose direction
 * s = sign(mB dA - mA dB) (64-bit integers) is not 0.  A DMR is a maximal run of candidates that follow one another among the candidates, lie on one
 * sequence, share s, and each lie at most max_gap nt behind the one before (pos[i] - pos[i - 1] <= max_gap).  Common sites that are no candidates do
 * not break a run; strand is ignored (without bsx_meth_combine_cpg the C and the G of a CpG are neighbouring rows).  n_sig is the number of candidates,
 * the span is [start, end) = [pos_first, pos_last + 1), 0-based and half-open; a run is reported when n_sig >= min_sites (min_sites >= 1).  Its sums
 * N, MA, DA, MB, DB and p are what bsx_meth_diff_regions returns for the span under the same min_depth: over ALL common sites of the span (N >= n_sig),
 * and the p is that pooled test, a description of the region and not a corrected value.
 *
 * The core on its own: q[n] of p[n], host arrays, computed on `device` (a radix sort of (bits of p, row index), r, a running minimum, a scatter).
 * Every p is within 0 .. 1 or NaN (BSX_ERR_ARG otherwise); n == 0 is BSX_OK; n >= 2^32 is BSX_ERR_LIMIT. */
int bsx_meth_bh(int device, const double *p, uint64_t n, double *q);
/* Fills the genome-wide store of handle `a`: every row of the family with pos, counts, class byte, p and q (37 bytes a row on the device, in buffers
 * apart from those of bsx_meth_diff_report_chr, whose rows stay fetchable).  n_rows: the family's size.  2^32 rows or more: BSX_ERR_NOMEM with a message.
 * The store stands for (b, min_depth) until the next bsx_meth_diff_report_all on `a`, or until an add, bsx_meth_combine_cpg, bsx_meth_set_reference or
 * bsx_meth_set_contexts on either handle; a handle created after `b` was destroyed is another sample B, also at the same address. */
int bsx_meth_diff_report_all(bsx_meth *a, bsx_meth *b, uint32_t min_depth, uint64_t *n_rows);
/* the store: row_start[n_chr + 1] by rank in the writer's sequence order (the rows of the k-th sequence of that order are [row_start[k], row_start[k + 1])),
 * and per row the 0-based position, counts[4] = mA, dA, mB, dB, the class byte (bits 0-1: CG, CHG, CHH, CN; bit 2 set over a G), p and q.  BSX_ERR_STATE
 * without a store */
int bsx_meth_diff_fetch_all(bsx_meth *a, uint32_t *row_start, uint32_t *pos0, uint32_t *counts, uint8_t *cls, double *p, double *q);
/* The DMRs over the store of the last bsx_meth_diff_report_all(a, b, min_depth): BSX_ERR_STATE when none stands for this b and min_depth.  *max_q within
 * 0 .. 1, min_delta_permille <= 1000, min_sites >= 1, else BSX_ERR_ARG.  n_dmr: how many, in the store's order. */
int bsx_meth_diff_dmrs(bsx_meth *a, bsx_meth *b, uint32_t min_depth, const double *max_q, uint32_t min_delta_permille, uint32_t max_gap, uint32_t min_sites,
                       uint32_t *n_dmr);
/* the DMRs of the last bsx_meth_diff_dmrs: sequence id, start, end, n_sig, sums[n_dmr][5] = N, MA, DA, MB, DB and p[n_dmr] */
int bsx_meth_diff_fetch_dmrs(bsx_meth *a, uint32_t *chr, uint32_t *start, uint32_t *end, uint32_t *n_sig, uint64_t *sums, double *p);
/* bsx_meth_write_diff with a 13th column q ("%.4e"; header "... p q"): formatted from the store (built here unless one stands for b and min_depth).  The
 * rows that pass the delta rule, p <= *max_p and q <= *max_q are written (a NULL pointer: no such filter); the first 12 columns of a written row are what
 * bsx_meth_write_diff writes for it, and no filter changes a printed q.  A limit outside 0 .. 1 (a NaN too) is BSX_ERR_ARG, as in bsx_meth_diff_dmrs.
 * n_rows: the rows written (needed). */
int bsx_meth_write_diff_fdr(bsx_meth *a, bsx_meth *b, const char *path, uint32_t min_depth, uint32_t min_delta_permille, const double *max_p, const double *max_q,
                            uint64_t *n_rows);
/* bsx_meth_write_diff_regions with a column q behind p: Benjamini-Hochberg over the file's intervals with N > 0 (bsx_meth_bh), "NA" for the others.
 * (The bin file has no q form: it is written in pieces of 2^22 bins and q needs all of them.) */
int bsx_meth_write_diff_regions_fdr(bsx_meth *a, bsx_meth *b, const char *bed_path, const char *out_path, uint32_t min_depth, uint64_t *n_written, uint64_t *n_dropped);
/* The DMRs as a file: header "chr start end n_sig n_C C_a CT_a ratio_a C_b CT_b ratio_b delta p", the numbers formatted as in bsx_meth_write_diff.  Uses
 * the store that stands for (b, min_depth) or builds it.  Argument rules of bsx_meth_diff_dmrs; n_rows: the DMRs written (needed). */
int bsx_meth_write_dmrs(bsx_meth *a, bsx_meth *b, const char *path, uint32_t min_depth, const double *max_q, uint32_t min_delta_permille, uint32_t max_gap,
                        uint32_t min_sites, uint64_t *n_rows);

#ifdef __cplusplus
}
#endif
#endif
