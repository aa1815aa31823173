/*
 * pcabi.h -- C ABI of the MI355X adapter-alignment engine (libpcabi.so).
 *
 * Two layers:
 *
 *  1. Drop-in legacy symbols, byte-compatible with the reference's cpp_functions.so
 *     (porechop_abi/include/adapter_align.h:12-16, bound by ctypes in
 *     porechop_abi/cpp_function_wrappers.py:25-39):
 *        char *adapterAlignment(char *readSeq, char *adapterSeq,
 *                               int matchScore, int mismatchScore,
 *                               int gapOpenScore, int gapExtensionScore);
 *        void  freeCString(char *p);
 *     Same argument order (Python passes match, mismatch, gap_open, gap_extend:
 *     cpp_function_wrappers.py:46-51), same malloc'd "rs,re,as,ae,score,pid1,pid2" result
 *     (porechop_abi/src/alignment.cpp:113-120), caller frees with freeCString. Each call runs
 *     on the GPU (one lane); concurrent callers are serialised per device.
 *
 *  2. Batch ABI used by the batched phase drivers (replacing the per-read ThreadPool loops of
 *     porechop_abi/porechop_abi.py:200-245, 359-438, 457-522). Sequences are Dna5 codes
 *     (A=0 C=1 G=2 T/U=3 anything else=4, S/basic/alphabet_residue_tabs.h:113-140) packed in
 *     one byte buffer; a "window" is an (offset, length) view into it (any offset), the
 *     buffer padded with >= 16 readable bytes past the last window. Results are SoA int32,
 *     8 fields x n_results, field order PCABI_F_*.
 *
 * Errors: functions return 0 on success, a negative PCABI_E_* code otherwise;
 * pcabi_last_error() returns a thread-local message. No exceptions cross the ABI.
 * There is no CPU fallback: without a usable gfx950 device every compute entry point fails.
 * The two drop-in symbols have no error channel (the reference's never fail on valid input):
 * when the engine fails under them they print pcabi_last_error() to stderr and abort() rather
 * than return an answer the reference would not give (adapterAlignment's "-1" sentinel would read
 * as "no alignment" and silently change trimming decisions). Empty inputs keep the reference's
 * "-1" result.
 *
 * Lengths: windows / reads of any length up to pcabi_max_window_len(); adapters (and the
 * shorter sequence of a check_compatibility pair) up to pcabi_max_adapter_len() = 65535 bases.
 * Adapters up to 128 bases run register-resident cores; longer ones the striped core
 * (row stripes of 32, the boundary row in stream-ordered device scratch).
 */
#ifndef PCABI_H
#define PCABI_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- result field order (SoA rows) -------------------------------------------------- */
enum {
    PCABI_F_RS = 0,     /* read start (ScoredAlignment::m_readStartPos), -1 = no alignment */
    PCABI_F_RE = 1,     /* read end, inclusive                                          */
    PCABI_F_AS = 2,     /* adapter start                                                */
    PCABI_F_AE = 3,     /* adapter end, inclusive                                       */
    PCABI_F_SCORE = 4,  /* raw DP score                                                 */
    PCABI_F_M = 5,      /* matching columns (numerator of both identities)              */
    PCABI_F_L1 = 6,     /* aligned-region length: pid1 = 100*m/l1 (NaN when l1 == 0)     */
    PCABI_F_L2 = 7,     /* full-adapter span length: pid2 = 100*m/l2                     */
    PCABI_NFIELDS = 8
};

enum {
    PCABI_OK = 0,
    PCABI_E_ARG = -1,      /* bad argument / unsupported size                   */
    PCABI_E_DEVICE = -2,   /* no usable gfx950 device / HIP runtime error       */
    PCABI_E_NOMEM = -3,
    PCABI_E_PARSE = -4     /* malformed FASTA / FASTQ input                     */
};

/* ---- legacy drop-in ------------------------------------------------------------------ */
char *adapterAlignment(char *readSeq, char *adapterSeq, int matchScore, int mismatchScore,
                       int gapOpenScore, int gapExtensionScore);
void freeCString(char *p);

/* ---- housekeeping -------------------------------------------------------------------- */
const char *pcabi_last_error(void);
int pcabi_version(void);                 /* ABI version, currently 1                     */
int pcabi_device_count(void);            /* visible HIP devices (0 if none)              */
int pcabi_max_adapter_len(void);         /* longest adapter the kernels accept (65535)   */
int pcabi_max_window_len(void);          /* longest window / read the kernels accept     */

/* ASCII -> Dna5 codes (host, table lookup). n bytes. */
void pcabi_encode_dna5(const char *ascii, uint8_t *codes, int64_t n);
/* Gathered ASCII -> Dna5 (host, up to 16 threads): codes[dst_off[i] .. + len[i]) = the codes of
 * the len[i] bytes at address src[i]; every byte of codes[0 .. codes_len) outside those segments
 * is set to N (4). dst_off ascending, segments disjoint. The Python drivers pass the addresses of
 * the reads' own str buffers, so windows of 10^5 reads are packed without a slice, a join or an
 * encode (replaces the per-read seq[:end_size] / seq[-end_size:] / trimmed-read slices that
 * nanopore_read.py:181, 203 and porechop_abi.py:495 hand to SeqAn's marshalling). */
void pcabi_encode_dna5_gather(const uint64_t *src, const int64_t *len, const int64_t *dst_off, int64_t n,
                              uint8_t *codes, int64_t codes_len);

/* Identity exactly as Python holds it after the reference's text round trip
 * (alignment.cpp:118-119 "%f", nanopore_read.py:497-498 float()): out[k] = pid6(m[k], l[k]),
 * NaN when l[k] == 0. Host-side formatting helper, same code as the device epilogues. */
void pcabi_pid6_host(const int32_t *m, const int32_t *l, int64_t n, double *out);

/* ---- batch alignment, host buffers ---------------------------------------------------- */
/*
 * Align windows against adapters on `device`.
 *   codes[codes_len]            : Dna5 codes holding every window (padding rules above)
 *   win_off[n_win], win_len[n_win]
 *   adp_codes, adp_off[n_adp], adp_len[n_adp] : adapters (Dna5 codes, any alignment)
 * Work:
 *   task_win == NULL  -> cross product: result (a, w) at index a*n_win + w
 *   task_win != NULL  -> n_task explicit pairs (task_win[t], task_adp[t]); result at index t
 * out: int32[PCABI_NFIELDS * n_results], row f holds field f for every result.
 */
int pcabi_align_host(int device,
                     const uint8_t *codes, int64_t codes_len,
                     const int64_t *win_off, const int32_t *win_len, int64_t n_win,
                     const uint8_t *adp_codes, const int32_t *adp_off, const int32_t *adp_len,
                     int32_t n_adp,
                     const int32_t *task_win, const int32_t *task_adp, int64_t n_task,
                     int match, int mismatch, int gap_open, int gap_extend,
                     int32_t *out);

/* ---- alignment paths and adapter profiles (csrc/pcabi_paths.hip) ------------------------ */
/*
 * The alignment itself, for explicit (window, adapter) pairs: the columns of the gapped rows SeqAn's
 * globalAlignment(..., AlignConfig<1,1,1,1>) leaves in Align (head free-gap columns, the traceback
 * path, tail free-gap columns), left to right, one op per column:
 *   MATCH        both rows hold the same Dna5 code (N against N is a match)
 *   MISMATCH     both rows hold a base, the codes differ
 *   READ_ONLY    a read base against a gap in the adapter row
 *   ADAPTER_ONLY an adapter base against a gap in the read row
 * run-length encoded as uint32 = (run_length << 2) | op, neighbouring runs of different ops. The
 * runs of pair t are runs[run_off[t] .. run_off[t + 1]) (run_off has n_task + 1 entries); a pair with
 * an empty window has none. For any other pair ops 0 + 1 + 2 add up to the window length and ops
 * 0 + 1 + 3 to the adapter length. out (int32[PCABI_NFIELDS * n_task], row f = field f) receives the
 * same eight fields pcabi_align_host returns for the pairs, computed from these columns.
 * Inputs are laid out as for pcabi_align_host (task_win / task_adp are required) and never written.
 * Adapters of 1..pcabi_max_path_adapter_len() = 128 bases, any four-integer scoring. A pair's trace
 * lives in LDS when it fits a wavefront's share and in device scratch otherwise; the pairs run in
 * rounds whose scratch stays within PCABI_PATHS_SCRATCH_MB (default 256), and a pair whose trace
 * alone, (window + adapter / 2) x adapter bytes, exceeds it is refused with PCABI_E_ARG.
 * Both return the total number of runs or a negative PCABI_E_*. When the total exceeds runs_cap, out
 * and run_off are complete and runs is undefined: call again with a larger buffer (the convention of
 * pcabi_middle_scan_dev). Bad arguments are refused before anything is launched.
 *   pcabi_align_paths_host : host buffers.
 *   pcabi_align_paths_dev  : every pointer a device pointer on the current device, queued on
 *                            `stream`, which the call synchronises (twice: it reads the lengths
 *                            and the pairs to plan the rounds, and the total at the end).
 *   pcabi_paths_scratch_pairs : pairs whose trace went to device scratch so far, process-wide.
 */
enum { PCABI_OP_MATCH = 0, PCABI_OP_MISMATCH = 1, PCABI_OP_READ_ONLY = 2, PCABI_OP_ADAPTER_ONLY = 3 };
int pcabi_max_path_adapter_len(void);
int64_t pcabi_paths_scratch_pairs(void);
int64_t pcabi_align_paths_host(int device, const uint8_t *codes, int64_t codes_len, const int64_t *win_off,
                               const int32_t *win_len, int64_t n_win, const uint8_t *adp_codes,
                               const int32_t *adp_off, const int32_t *adp_len, int32_t n_adp,
                               const int32_t *task_win, const int32_t *task_adp, int64_t n_task, int match,
                               int mismatch, int gap_open, int gap_extend, int32_t *out, int64_t *run_off,
                               uint32_t *runs, int64_t runs_cap);
int64_t pcabi_align_paths_dev(const uint8_t *codes, const int64_t *win_off, const int32_t *win_len, int64_t n_win,
                              const uint8_t *adp_codes, const int32_t *adp_off, const int32_t *adp_len,
                              int32_t n_adp, const int32_t *task_win, const int32_t *task_adp, int64_t n_task,
                              int match, int mismatch, int gap_open, int gap_extend, int32_t *out,
                              int64_t *run_off, uint32_t *runs, int64_t runs_cap, void *stream);
/*
 * Per-position pileup of the reads over their adapters, from the run lists above: counts
 * (int64[n_adp * max_adp_len * PCABI_PROFILE_NCOL], row-major) is ADDED to, so batches accumulate.
 * Only the columns of the aligned region count (the region l1 is measured over, alignment.cpp:28-52;
 * free end-gap columns never do). For adapter position i: the read base aligned to it (MATCH and
 * MISMATCH alike) counts under A..N, an ADAPTER_ONLY column under DEL, and every READ_ONLY base
 * under INS at the position of the last adapter base to its left (position 0 if there is none).
 * select (uint8[n_task], NULL = every pair) picks the pairs; res (the rs row of the pairs' results,
 * or NULL) skips pairs without an alignment. Positions >= max_adp_len are dropped.
 *   pcabi_adapter_profile_dev  : device pointers, asynchronous on `stream`.
 *   pcabi_adapter_profile_host : host buffers (windows as for pcabi_align_host).
 */
enum { PCABI_PROFILE_A = 0, PCABI_PROFILE_C = 1, PCABI_PROFILE_G = 2, PCABI_PROFILE_T = 3, PCABI_PROFILE_N = 4,
       PCABI_PROFILE_DEL = 5, PCABI_PROFILE_INS = 6, PCABI_PROFILE_NCOL = 7 };
int pcabi_adapter_profile_dev(const int32_t *res, const int64_t *run_off, const uint32_t *runs,
                              const uint8_t *codes, const int64_t *win_off, const int32_t *win_len,
                              const int32_t *task_win, const int32_t *task_adp, const uint8_t *select,
                              int64_t n_task, int32_t n_adp, int32_t max_adp_len, int64_t *counts, void *stream);
int pcabi_adapter_profile_host(int device, const int32_t *res, const int64_t *run_off, const uint32_t *runs,
                               const uint8_t *codes, int64_t codes_len, const int64_t *win_off,
                               const int32_t *win_len, int64_t n_win, const int32_t *task_win,
                               const int32_t *task_adp, const uint8_t *select, int64_t n_task, int32_t n_adp,
                               int32_t max_adp_len, int64_t *counts);

/* ---- device-resident interface (bench / multi-GPU shards) ------------------------------ */
/* Thin HIP wrappers so hosts without a GPU framework can keep inputs resident in HBM. */
int pcabi_dev_set(int device);
int pcabi_dev_malloc(void **ptr, int64_t bytes);
int pcabi_dev_free(void *ptr);
int pcabi_dev_h2d(void *dst, const void *src, int64_t bytes);
int pcabi_dev_d2h(void *dst, const void *src, int64_t bytes);
int pcabi_dev_memset(void *dst, int value, int64_t bytes);
int pcabi_dev_sync(void);
/* ordered on `stream`; kind 0 = host->device, 1 = device->host, 2 = device->device */
int pcabi_dev_copy_async(void *dst, const void *src, int64_t bytes, int kind, void *stream);
int pcabi_stream_create(void **stream);
int pcabi_stream_destroy(void *stream);
int pcabi_stream_sync(void *stream);
int pcabi_event_create(void **ev);
int pcabi_event_destroy(void *ev);
int pcabi_event_record(void *ev, void *stream);
/* later work on `stream` waits for `ev` (recorded on another stream): fork / join of caller streams */
int pcabi_stream_wait_event(void *stream, void *ev);
int pcabi_event_elapsed_ms(float *ms, void *start, void *stop);

/*
 * Prepared adapter table: adapters re-laid out per register bucket (top-padded, packed codes).
 * Build once per adapter list; reuse across batches.
 */
typedef struct pcabi_adapters pcabi_adapters;
int pcabi_adapters_create(const uint8_t *adp_codes, const int32_t *adp_off, const int32_t *adp_len,
                          int32_t n_adp, pcabi_adapters **out);   /* uploads to current device */
/* Same, with small register buckets merged into larger ones for THIS scoring (fewer, fuller
 * launches; the packed core passes scores through the extra padding rows). The table then
 * serves that scoring only: pcabi_align_cross_dev rejects others. */
int pcabi_adapters_create_scored(const uint8_t *adp_codes, const int32_t *adp_off,
                                 const int32_t *adp_len, int32_t n_adp, int match, int mismatch,
                                 int gap_open, int gap_extend, pcabi_adapters **out);
void pcabi_adapters_destroy(pcabi_adapters *a);

/*
 * Tile layout of a window list, the form the cross-product kernels read:
 * windows [256t, 256t + 256) form tile t; dword (t, q, lane) holds codes 4q..4q+3 of window
 * 256t + lane at tiles[tile_off[t] + 256 q + lane], so a wavefront's load of one 4-column chunk
 * is 256 contiguous bytes. A tile holds ceil(longest window in it / 4) + 2 chunks; sort the
 * windows by length first when they vary (whole reads) to keep tiles dense.
 *   pcabi_tile_layout      : host; fills tile_off[ceil(n_win/256) + 1] (dword offsets) from the
 *                            host copy of win_len and returns the total dword count (< 0 on
 *                            error).
 *   pcabi_tile_windows_dev : device pointers, async on `stream`: writes `tiles` from windows
 *                            laid out as for pcabi_align_host (codes/win_off/win_len);
 *                            max_chunks = largest per-tile chunk count (a launch-shape hint).
 */
int64_t pcabi_tile_layout(const int32_t *win_len, int64_t n_win, int64_t *tile_off);
int pcabi_tile_windows_dev(const uint8_t *codes, const int64_t *win_off, const int32_t *win_len,
                           int64_t n_win, const int64_t *tile_off, int64_t max_chunks,
                           uint32_t *tiles, void *stream);

/*
 * Cross-product alignment, every pointer a DEVICE pointer, asynchronous on `stream`:
 * result (a, w) -> out[f * out_stride + a * n_win + w]. Windows come in tile layout (above);
 * win_len[n_win] is still passed per window. max_win_len (host value) bounds every win_len[w]
 * and must be honest: windows longer than 32k need negative gap costs (the start-column field
 * of the non-packed cores is kept mod 2^16).
 */
int pcabi_align_cross_dev(const uint32_t *tiles, const int64_t *tile_off, const int32_t *win_len,
                          int64_t n_win, int32_t max_win_len, const pcabi_adapters *adps,
                          int match, int mismatch, int gap_open, int gap_extend,
                          int32_t *out, int64_t out_stride, void *stream);
/* Same, and records ev_begin / ev_end (pcabi_event_create; either may be NULL) on `stream`
 * around the launch of the table's largest bucket (adapters x rows), which runs on `stream`
 * while the other buckets run beside it on the device's side streams: the events time that
 * kernel inside a full cross product (bench.py's roofline). */
int pcabi_align_cross_dev_marked(const uint32_t *tiles, const int64_t *tile_off, const int32_t *win_len,
                                 int64_t n_win, int32_t max_win_len, const pcabi_adapters *adps,
                                 int match, int mismatch, int gap_open, int gap_extend,
                                 int32_t *out, int64_t out_stride, void *stream, void *ev_begin,
                                 void *ev_end);
/* Several cross products in one call (r06): region k = (tiles, tile_off, win_len, n_win,
 * max_win_len, adps, out, out_stride) is aligned exactly as pcabi_align_cross_dev would align it
 * (same results, same layout), but the register buckets of ALL regions run as grouped launches: the
 * buckets of one core family -- the run-tagged core (affine, <= 32 rows) and the packed core (affine,
 * 36..64 rows) -- across every region share one launch each (pcabi_kern.h "grouped cross
 * launches"), the other buckets launch on their own. A bucket of one or two adapters (a 400-block
 * grid for 100k windows) is latency-bound alone; grouped with the others its waves fill the SIMDs.
 * The largest launch runs on `stream` (ev_begin / ev_end, either may be NULL, are recorded around
 * it), the others beside it on the side streams when they are on for `stream`. Replaces the
 * per-side calls of porechop_abi.py:359-438's end trim (both read ends in one call). */
typedef struct pcabi_cross_region {
    const uint32_t *tiles;
    const int64_t *tile_off;
    const int32_t *win_len;
    int64_t n_win;
    int32_t max_win_len;
    const pcabi_adapters *adps;
    int32_t *out;
    int64_t out_stride;
} pcabi_cross_region;
int pcabi_align_cross_multi_dev(const pcabi_cross_region *regions, int32_t n_regions, int match, int mismatch,
                                int gap_open, int gap_extend, void *stream, void *ev_begin, void *ev_end);
/* Side streams (process-wide): with on = 1 a cross product (and a middle-scan round) runs its
 * largest register bucket on the caller's stream and the others beside it on the device's side
 * streams; with on = 0 every bucket runs on the caller's stream, one after the other. Side by side
 * pays for ONE cross product at a time (the largest bucket's tail fills with the small ones);
 * callers that run cross products on several streams at once should turn it off: HIP maps the
 * process's streams onto GPU_MAX_HW_QUEUES hardware queues, and a side stream on the queue of
 * another caller stream's large launch waits for it (r04r: the reference job 4.95 -> 4.66 ms
 * off). Initially on. Returns the previous setting; on < 0 only reads it. */
int pcabi_set_side_streams(int on);
/* The same setting for one stream (r05): the cross products and middle-scan rounds queued on `stream`
 * use the side streams when on = 1 and run every bucket on `stream` when on = 0, whatever the
 * process-wide setting; on = -1 removes the stream's entry (it follows pcabi_set_side_streams again).
 * Returns the stream's previous entry (0 / 1) or -1 when it had none. Callers that run cross
 * products on several streams at once set 0 on those streams (r04r: the reference job 4.95 -> 4.66
 * ms), and no other caller of the library is affected. Destroying a stream does not remove its entry:
 * remove it first (a new stream may reuse the handle). */
int pcabi_stream_side_streams(void *stream, int on);

/*
 * End-trim decision epilogue (porechop_abi/nanopore_read.py:175-217), device pointers:
 *   start results: cross product of n_read start windows x n_sa start adapters (layout above)
 *   end results  : cross product of n_read end windows   x n_ea end adapters
 * Identities are compared exactly as the reference does after its text round trip
 * (alignment.cpp:118-119 prints "%f", nanopore_read.py:497-498 parses it back): the device
 * rounds 100*m/l to 6 decimals with round-half-even on the exact double, then to the nearest
 * double (pcabi::pid6). Python's '%f' pins both builds of it: the host build in
 * tests/test_abi.py::test_pid6_host_exact and tests/test_dp_core_cpu.py::
 * test_pid6_matches_text_round_trip, the device build bit for bit in tests/test_gpu_epilogues.py
 * (test_device_pid6_grid, test_device_pid6_ties), each over the lengths whose ties only the exact
 * product decides (64000, 128000, ...).
 * Writes start_trim[n_read], end_trim[n_read] (amounts, same integers as
 * NanoporeRead.start_trim_amount / end_trim_amount) and, when non-NULL, per-pair
 * "alignment recorded" flags (uint8, same layout as the results).
 */
int pcabi_end_trim_dev(const int32_t *start_res, int64_t start_stride, int32_t n_sa,
                       const int32_t *end_res, int64_t end_stride, int32_t n_ea,
                       int64_t n_read, int end_size, int extra_trim, double end_threshold, int min_trim_size,
                       int32_t *start_trim, int32_t *end_trim,
                       uint8_t *start_hit, uint8_t *end_hit, void *stream);

/*
 * The reads with their end adapters trimmed, on the device (nanopore_read.py:44-49,
 * get_seq_with_start_end_adapters_trimmed): view_off = read_off + start_trim, view_len = the
 * length of Python's slice seq[start_trim : read_len - end_trim] -- read_len - start_trim -
 * end_trim while the trims fit; a negative stop (end_trim > read_len) counts from the end, both
 * ends are clipped to the read, never below 0 -- the middle scan's windows straight from
 * pcabi_end_trim_dev's amounts, with no host round trip. Trims are >= 0. Async on `stream`.
 */
int pcabi_trim_views_dev(const int64_t *read_off, const int32_t *read_len, const int32_t *start_trim,
                         const int32_t *end_trim, int64_t n_read, int64_t *view_off, int32_t *view_len, void *stream);

/*
 * End-trim decisions with their alignment lists (porechop_abi/nanopore_read.py:175-217, the loop of
 * find_adapters_at_read_ends, porechop_abi.py:359-438) from HOST buffers, with only the decisions
 * coming back -- never the (read, adapter) result matrix:
 *   codes / s_off, s_len / e_off, e_len : start and end windows of n_read reads (layout of
 *                         pcabi_align_host: one buffer, any offsets, 16 bytes of padding)
 *   sa_* / ea_*         : start and end adapters (Dna5 codes)
 *   start_trim / end_trim[n_read] : NanoporeRead.start_trim_amount / end_trim_amount
 *   start_hits / end_hits : 7 rows x cap int32 -- every alignment find_start_trim / find_end_trim
 *                         record, read-major and in adapter order within a read (the order they
 *                         are appended): read, adapter, rs, re (inclusive), m, l1, l2 (full identity
 *                         = pid6(m, l2), partial = pid6(m, l1)); n_hits[2] receives the two counts,
 *                         and a side whose count exceeds cap is not written (call again, larger cap)
 *   bc_s[n_bc_s], bc_e[n_bc_e] : adapters whose full identity of every read the barcode dicts keep
 *                         (nanopore_read.py:193-195, 215-217); bc_full (double, (n_bc_s + n_bc_e) x
 *                         n_read, start adapters first) receives them when non-NULL
 * The prepared adapter tables are kept per device between calls with the same adapters and scoring.
 *   pcabi_flag_list_dev : the list of one side from device pointers (async on `stream`): flagged
 *                         pairs (k_end_trim's flags, layout of pcabi_end_trim_dev) of a result
 *                         block -> out (7 rows x cap, as above), *n_out (device uint64) = the count;
 *                         when the count exceeds cap, out is not written.
 */
int pcabi_end_decisions_host(int device, const uint8_t *codes, int64_t codes_len, const int64_t *s_off,
                             const int32_t *s_len, const int64_t *e_off, const int32_t *e_len, int64_t n_read,
                             const uint8_t *sa_codes, const int32_t *sa_off, const int32_t *sa_len, int32_t n_sa,
                             const uint8_t *ea_codes, const int32_t *ea_off, const int32_t *ea_len, int32_t n_ea,
                             int match, int mismatch, int gap_open, int gap_extend, int end_size, int extra_trim,
                             double end_threshold, int min_trim_size, int32_t *start_trim, int32_t *end_trim,
                             int32_t *start_hits, int32_t *end_hits, int64_t cap, int64_t *n_hits,
                             const int32_t *bc_s, int32_t n_bc_s, const int32_t *bc_e, int32_t n_bc_e,
                             double *bc_full);
/*
 * pcabi_end_decisions_seqs: the same decisions from the window STRINGS (the reference's
 * seq[:end_size] / seq[-end_size:] slices, nanopore_read.py:181, 203, never made): win[2 n_read]
 * the address of each window's first character (ASCII, one byte per base -- start windows, then
 * end windows), win_len[2 n_read] its length. The library lays them out as pcabi_end_decisions_host's
 * buffer and encodes them itself into pinned staging buffers while earlier chunks copy.
 */
int pcabi_end_decisions_seqs(int device, const char *const *win, const int32_t *win_len, int64_t n_read,
                             const uint8_t *sa_codes, const int32_t *sa_off, const int32_t *sa_len, int32_t n_sa,
                             const uint8_t *ea_codes, const int32_t *ea_off, const int32_t *ea_len, int32_t n_ea,
                             int match, int mismatch, int gap_open, int gap_extend, int end_size, int extra_trim,
                             double end_threshold, int min_trim_size, int32_t *start_trim, int32_t *end_trim,
                             int32_t *start_hits, int32_t *end_hits, int64_t cap, int64_t *n_hits,
                             const int32_t *bc_s, int32_t n_bc_s, const int32_t *bc_e, int32_t n_bc_e,
                             double *bc_full);
int pcabi_flag_list_dev(const uint8_t *flag, int32_t n_adp, int64_t n_read, const int32_t *res, int64_t stride,
                        int32_t *out, int64_t cap, unsigned long long *n_out, void *stream);

/*
 * Middle-adapter scan, round 1 (porechop_abi/nanopore_read.py:219-252): for every window
 * (whole end-trimmed read) the FIRST adapter in list order whose full-adapter identity
 * (pid2, compared after the "%f" round trip like the reference) is not below `threshold`.
 * The reference's masked re-alignment loop hits exactly that adapter first; later rounds
 * re-align the masked read against that adapter and the ones after it (pcabi_align_host pairs).
 * hits: int32 SoA, 5 rows x n_win: adapter index (-1 = none), rs, re (inclusive), m, l2.
 *   pcabi_first_hits_host : host buffers as pcabi_align_host (cross product, tiled on device);
 *                           only the 20 B/read of hits come back over PCIe.
 *   pcabi_first_hit_dev   : epilogue over a device cross-product result block (layout of
 *                           pcabi_align_cross_dev), async on `stream`.
 */
int pcabi_first_hits_host(int device, const uint8_t *codes, int64_t codes_len, const int64_t *win_off,
                          const int32_t *win_len, int64_t n_win, const uint8_t *adp_codes,
                          const int32_t *adp_off, const int32_t *adp_len, int32_t n_adp,
                          int match, int mismatch, int gap_open, int gap_extend, double threshold,
                          int32_t *hits);
int pcabi_first_hit_dev(const int32_t *res, int64_t stride, int64_t n_win, int32_t n_adp,
                        double threshold, int32_t *hits, int64_t hit_stride, void *stream);

/*
 * The whole middle-adapter scan (porechop_abi/nanopore_read.py:219-252, the masked re-alignment
 * loop of find_middle_adapters) for a batch of end-trimmed reads, in rounds on the device:
 * round 1 finds each read's first adapter whose best alignment reaches the threshold -- the pairs
 * that can hit are found first, by exact k-mer seeds (pcabi_seed.hip: seed scan, expansion, banded
 * bounds) or, where seeds do not apply, by a score-only filter, and only those candidates get the
 * attribute DP (in owned-column chunks, planned on the device); every later round masks the new
 * hits (N, the reference's '-') and re-aligns only the reads that just hit, from the adapter that
 * hit onwards, until no read hits (DESIGN.md §4 "Middle scan"). As the reference masks a copy
 * (nanopore_read.py:225,234), the caller's codes are never written: a read's first hit copies it
 * into a shadow arena the scan owns, and later hits mask that copy. Pairs where
 * neither way applies run the full cross product with k_first_hit. Hits are written to `hits`
 * (HOST int32, 6 rows x cap: read, adapter, read_start,
 * read_end (exclusive), m, l2 -- full identity = pid6(m, l2)) in discovery order, which per read
 * is the reference's order. Returns the number of hits (may exceed cap: only the first cap are
 * written) or a negative error. threshold must be > 0 (the reference never terminates otherwise).
 *   pcabi_scan_create / destroy : scratch for one adapter table (current device).
 *   pcabi_middle_scan_dev       : codes/win_off/win_len are DEVICE pointers (codes are read only:
 *                                 byte-identical after the call), h_win_len the host copy of the lengths or NULL (the call
 *                                 then copies them: e.g. views from pcabi_trim_views_dev). When the
 *                                 seeded plan covers the table and scoring, the rounds are queued on
 *                                 the device with their counts there (no host round trip between
 *                                 rounds; PCABI_MIDDLE_DEVROUNDS=0 keeps the host-driven loop).
 *   pcabi_middle_scan_host      : host buffers (as pcabi_align_host), copies in, scans.
 *   pcabi_middle_scan_seqs      : the windows as host strings, seqs[w] its first character and
 *                                 seq_len[w] its length (the char * the reference's ctypes wrapper
 *                                 passes per call, porechop_abi/cpp_function_wrappers.py:42-63):
 *                                 encoded (the Dna5 table of pcabi_encode_dna5) by host threads into
 *                                 pinned staging buffers while earlier chunks copy to the device,
 *                                 then scanned as pcabi_middle_scan_host. Same hits, same returns.
 *   pcabi_middle_seed_runs      : how many round-1 scans took their bounds from exact k-mer seeds
 *                                 (pcabi_seed.hip) instead of the score filter, process-wide.
 *                                 PCABI_MIDDLE_SEEDS=0 / 1 (default, cost model) / 2 (always when
 *                                 the seeds apply) selects; the hits are the same either way.
 *   pcabi_middle_requeues       : queued rounds that overflowed a buffer (raw-hit slabs, band task
 *                                 regions, candidate-DP task slots), were dropped and queued again,
 *                                 process-wide; *flags_seen (optional) = the OR of their flags
 *                                 (1 raw hits, 2 band tasks, 4 task slots, 8 shadow arena). Test knobs:
 *                                 PCABI_MIDDLE_INIT_CAPS="raw,task,slots[,arena]" sizes a new scan's buffers,
 *                                 PCABI_MIDDLE_FAULT="round:bits,..." shrinks one round's buffers.
 *   pcabi_scan_profile          : per-phase profile of this scan's device rounds (a diagnostic: with
 *                                 it on, every queued round is synchronised on its own). mode 1 =
 *                                 reset and on, 0 = off, 2 = read only; out[0..14] (n_out values at
 *                                 most): ms of k_seed_scan, k_seed_expand, the band classes, k_cands,
 *                                 the plan kernels, the candidate DP, the rest; then rounds, reads,
 *                                 bases scanned, raw seed hits, inside / edge band tasks, candidate-DP
 *                                 tasks and cells (columns x adapter rows); out[15] = ms of round 1
 *                                 (its runs, whole); out[16..23] per band class (2) the pinned bands'
 *                                 lane-rows issued, active lane-rows (x (2E + 1) = band cells), tasks
 *                                 and passes (counted by the profiled launches only); out[24..25]
 *                                 the classes' E. Returns 26 or < 0.
 */
typedef struct pcabi_scan pcabi_scan;
int pcabi_scan_create(const pcabi_adapters *adps, pcabi_scan **out);
void pcabi_scan_destroy(pcabi_scan *s);
int64_t pcabi_middle_scan_dev(pcabi_scan *s, const uint8_t *codes, const int64_t *win_off,
                              const int32_t *win_len, const int32_t *h_win_len, int64_t n_win,
                              int match, int mismatch, int gap_open, int gap_extend,
                              double threshold, int32_t *hits, int64_t cap, void *stream);
int64_t pcabi_middle_scan_host(int device, const uint8_t *codes, int64_t codes_len,
                               const int64_t *win_off, const int32_t *win_len, int64_t n_win,
                               const uint8_t *adp_codes, const int32_t *adp_off,
                               const int32_t *adp_len, int32_t n_adp, int match, int mismatch,
                               int gap_open, int gap_extend, double threshold, int32_t *hits,
                               int64_t cap);
/*
 * pcabi_stage_seqs_host: the staging the *_seqs entry points use, on its own -- the n strings
 * (addresses of their first characters, lengths) laid out as SeqPack does (4-aligned starts, N
 * between, 16 N after), carried to the device as 2-bit codes plus an N mask and unpacked there
 * into Dna5 bytes, then copied to out[out_len >= the layout's size] (a check of the staging).
 */
int pcabi_stage_seqs_host(int device, const char *const *seqs, const int32_t *seq_len, int64_t n, uint8_t *out,
                          int64_t out_len);
int64_t pcabi_middle_scan_seqs(int device, const char *const *seqs, const int32_t *seq_len, int64_t n,
                               const uint8_t *adp_codes, const int32_t *adp_off,
                               const int32_t *adp_len, int32_t n_adp, int match, int mismatch,
                               int gap_open, int gap_extend, double threshold, int32_t *hits,
                               int64_t cap);
int64_t pcabi_middle_seed_runs(void);
int64_t pcabi_middle_requeues(int32_t *flags_seen);
int32_t pcabi_scan_profile(pcabi_scan *s, int32_t mode, double *out, int32_t n_out);

/*
 * Adapter-set discovery reduction (porechop_abi/nanopore_read.py:158-173): for each adapter a
 * of a cross-product result block, best[a] = max(best[a], max_w pid2(a, w)).
 */
int pcabi_best_full_identity_dev(const int32_t *res, int64_t stride, int64_t n_win, int32_t n_adp,
                                 double *best, void *stream);
/* The same over windows in host buffers (layout of pcabi_align_host, cross product): the
 * (adapter, window) results stay on the device, only n_adp doubles move. best_on_device != 0:
 * `best` is a device pointer on `device` (e.g. the buffer a collective reduces next; it must be
 * ready when called and is updated when the call returns); else a host array. */
int pcabi_best_full_identity_host(int device, const uint8_t *codes, int64_t codes_len, const int64_t *win_off,
                                  const int32_t *win_len, int64_t n_win, const uint8_t *adp_codes,
                                  const int32_t *adp_off, const int32_t *adp_len, int32_t n_adp, int match,
                                  int mismatch, int gap_open, int gap_extend, double *best, int best_on_device);

/*
 * Middle-adapter trim ranges (porechop_abi/nanopore_read.py:233-250) of a scan's hits: hit k =
 * (read hits[k], adapter hits[stride + k], read_start hits[2 stride + k], read_end (exclusive)
 * hits[3 stride + k]) -- the layout pcabi_middle_scan_* return -- becomes the range
 * [read_start - (bad_start[a] ? bad_side : good_side), read_end + (bad_end[a] ? bad_side : good_side))
 * of NanoporeRead.middle_trim_positions; bad_start / bad_end flag the adapters whose name is a
 * start / end sequence name. Output grouped per read, each read's hits in discovery order:
 * ranges of read r at cuts[2 k], cuts[2 k + 1] for k in [cut_off[r], cut_off[r + 1]) (cut_off has
 * n_reads + 1 entries) -- the cut layout of pcabi_reads_write.
 *   pcabi_middle_cuts_dev  : device pointers, asynchronous on `stream`.
 *   pcabi_middle_cuts_host : host arrays (n_adp flags each).
 */
int pcabi_middle_cuts_dev(const int32_t *hits, int64_t hit_stride, int64_t n_hits, int64_t n_reads,
                          const uint8_t *bad_start, const uint8_t *bad_end, int good_side, int bad_side,
                          int64_t *cut_off, int64_t *cuts, void *stream);
int pcabi_middle_cuts_host(int device, const int32_t *hits, int64_t hit_stride, int64_t n_hits, int64_t n_reads,
                           const uint8_t *bad_start, const uint8_t *bad_end, int32_t n_adp, int good_side,
                           int bad_side, int64_t *cut_off, int64_t *cuts);

/*
 * Barcode demultiplexing call (porechop_abi/nanopore_read.py:408-482, determine_barcode) from
 * the barcode dicts find_start_trim / find_end_trim fill (nanopore_read.py:193-195, 215-217).
 * Replaces the per-read Python loop of porechop_abi.py:359-438 when -b is given.
 *   *_res            : cross-product result blocks (layout of pcabi_align_cross_dev), n_read
 *                      windows x the side's adapters
 *   *_slot_adp[k]    : slot k of the side's dict in insertion order = the adapter (index into the
 *                      side's table) whose full identity is the entry's value (the last adapter of
 *                      that barcode name in set order)
 *   *_slot_name[k]   : the entry's barcode id (ids >= 0, shared by both sides)
 * Identities are pid6(m, l2) (the reference's "%f" round trip), 0.0 for a failed alignment.
 * Writes call[n_read] = barcode id or -1 ('none'); scores (optional, double[4 * n_read]):
 * require_two -> best start, second start, best end, second end; else best, second overall.
 * The albacore cross-check (nanopore_read.py:479-482) stays with the caller.
 *   pcabi_barcode_call_dev  : device pointers, async on `stream`.
 *   pcabi_barcode_call_host : host result arrays int32[PCABI_NFIELDS][n_adp * n_read] per side.
 */
int pcabi_barcode_call_dev(const int32_t *start_res, int64_t start_stride, const int32_t *start_slot_adp,
                           const int32_t *start_slot_name, int32_t n_start_slots, const int32_t *end_res,
                           int64_t end_stride, const int32_t *end_slot_adp, const int32_t *end_slot_name,
                           int32_t n_end_slots, int64_t n_read, double barcode_threshold, double barcode_diff,
                           int require_two, int32_t *call, double *scores, void *stream);
int pcabi_barcode_call_host(int device, const int32_t *start_res, int32_t n_sa, const int32_t *start_slot_adp,
                            const int32_t *start_slot_name, int32_t n_start_slots, const int32_t *end_res,
                            int32_t n_ea, const int32_t *end_slot_adp, const int32_t *end_slot_name,
                            int32_t n_end_slots, int64_t n_read, double barcode_threshold, double barcode_diff,
                            int require_two, int32_t *call, double *scores);

/*
 * Ab-initio adapter clustering link test (porechop_abi/ab_initio_src/compatibility.cpp,
 * compatibility.h:58-60, called all-vs-all by consensus.py:72-100): semi-global alignment
 * (free end gaps, match 2 / mismatch -1 / linear gap -1, SeqAn String<Dna>: anything but
 * ACGTU is A) of the longer sequence against the shorter, then the reference's flag:
 * 0 not compatible, 1 compatible (integer identity of the aligned region >= 87.5), 2 compatible
 * and the shorter lies inside the longer (region more than 3 bases from an end).
 *   check_compatibility : the drop-in symbol of the reference's compatibility.so (current device;
 *       aborts with a message if the engine fails, see Errors above).
 *   pcabi_compat_host   : n_pairs (pair_i[t], pair_j[t]) of n_seq sequences given as Dna codes
 *       (0..3) in one buffer (seq_off / seq_len, 16 bytes of padding), flags[n_pairs]; the
 *       shorter sequence of a pair must be <= pcabi_max_adapter_len() bases. Empty -> 0.
 */
int check_compatibility(char *raw_seq1, char *raw_seq2);
int pcabi_compat_host(int device, const uint8_t *codes, int64_t codes_len, const int64_t *seq_off,
                      const int32_t *seq_len, int64_t n_seq, const int32_t *pair_i, const int32_t *pair_j,
                      int64_t n_pairs, int32_t *flags);
/* consensus.py:72-100 all_vs_all_matrix: mat[n_seq * n_seq] (row-major, -1 on the diagonal,
 * symmetric). Runs every sequence against every sequence in the tiled cross mode (sequences over
 * 128 bases as rows on the striped core) when all are 1..pcabi_max_adapter_len() bases, explicit
 * pairs otherwise. n_seq <= 46340. */
int pcabi_compat_all_vs_all_host(int device, const uint8_t *codes, int64_t codes_len, const int64_t *seq_off,
                                 const int32_t *seq_len, int64_t n_seq, int32_t *mat);

/*
 * Ab-initio k-mer counts (porechop_abi/ab_initio_src/approx_counter.cpp, csrc/pcabi_kmer.hip).
 * Sequences: Dna5 codes (0..4) in one buffer, seq_off / seq_len.
 *   pcabi_kmer_count_host : count_kmers (:487-519): every k-mer (2 <= k <= 32, 2-bit value,
 *       first base in the top bits) without N, not low-complexity (dimer score >= lc_threshold,
 *       :214-234) and not in forbidden_sorted (ascending); writes (k-mer, count) ascending by
 *       k-mer, returns the number of distinct k-mers (if > cap nothing is written: call again
 *       with cap >= the return value) or a negative PCABI_E_*.
 *   pcabi_kmer_approx_host : errorCount (:531-601): counts[q] = sum over sequences of
 *       3 - d for the best substring edit distance d <= 2 of kmers[q] (SeqAn's search at <= 2
 *       errors reports a sequence once at every level from d to 2). Sequences start at 4-aligned
 *       offsets of a buffer whose length is a multiple of 4 (N padding); n_kmers <= 65535 * 64.
 */
int64_t pcabi_kmer_count_host(int device, const uint8_t *codes, int64_t codes_len, const int64_t *seq_off,
                              const int32_t *seq_len, int64_t n_seq, int k, float lc_threshold,
                              const uint64_t *forbidden_sorted, int64_t n_forbidden, uint64_t *kmers,
                              uint32_t *counts, int64_t cap);
/*   pcabi_kmer_top_host : the same counts, sorted by count descending (equal counts k-mer
 *       ascending), only the entries with count >= max(min_count, the top-th largest count)
 *       (top <= 0: no rank cut) -- every k-mer get_most_frequent / get_solid_kmers can keep
 *       (:372-405). Returns the entries written, or the capacity needed when > cap. */
int64_t pcabi_kmer_top_host(int device, const uint8_t *codes, int64_t codes_len, const int64_t *seq_off,
                            const int32_t *seq_len, int64_t n_seq, int k, float lc_threshold,
                            const uint64_t *forbidden_sorted, int64_t n_forbidden, int64_t top, int64_t min_count,
                            uint64_t *kmers, uint32_t *counts, int64_t cap);
/* Host gather of byte segments: dst[dst_off[i] .. + len[i]) = src[src_off[i] .. + len[i]). */
void pcabi_gather_host(const uint8_t *src, const int64_t *src_off, const int32_t *len, int64_t n, uint8_t *dst,
                       const int64_t *dst_off);
int pcabi_kmer_approx_host(int device, const uint8_t *codes, int64_t codes_len, const int64_t *seq_off,
                           const int32_t *seq_len, int64_t n_seq, int k, const uint64_t *kmers, int64_t n_kmers,
                           uint64_t *counts);

/*
 * Sequence files (host code: the reader csrc/pcabi_io.cpp, the writers csrc/pcabi_write.cpp; replaces porechop_abi/misc.py:60-168
 * load_fasta_or_fastq and NanoporeRead's normalisation, nanopore_read.py:31-44, for the batched
 * path, and NanoporeRead.get_fasta / get_fastq, nanopore_read.py:84-156, for output).
 *   pcabi_fastx_open / next / close : streaming reader, plain or gzip, FASTA, FASTQ (by the
 *       first character) or unaligned BAM (first bytes "BAM"; see "unaligned BAM input" below),
 *       the reference's parse rules; next() returns up to max_reads records
 *       (stopping once max_bases sequence bytes are in the batch) as a new pcabi_reads, or a
 *       negative PCABI_E_* (PCABI_E_PARSE for a malformed file); 0 records at end of file.
 *   pcabi_fastx_load : the whole file as one batch.
 *   raw != 0 : keep the file's text (no upper-casing, no U -> T, no quality padding; FASTQ '+'
 *       lines kept in spacer) -- the tuples of misc.load_fasta_or_fastq.
 *   pcabi_reads_views: borrowed pointers into a batch (valid until pcabi_reads_free):
 *       names   : full headers (text after '@' / '>'), name_off[n + 1]
 *       seq     : upper-cased sequences, U -> T for RNA reads (rna[i] = 1), seq_off[n + 1]
 *       qual    : qualities padded with '+' to the sequence length (FASTA: all '+'), qual_off[n + 1]
 *       codes   : Dna5 codes in the engine layout (4-aligned code_off[n], len[n], 16 bytes of
 *                 N padding at the end) -- ready for pcabi_align_host / the device ABI.
 *   pcabi_reads_write: the reference's trimmed output of every read (select[i] != 0 if given):
 *       start_trim / end_trim (NULL = untrimmed), middle cut ranges [cuts[2k], cuts[2k+1]) of the
 *       trimmed sequence for k in [cut_off[i], cut_off[i+1]) (NULL = none; a read with cuts is
 *       written as its split parts, or dropped with discard_middle), FASTA (70-column lines) or
 *       FASTQ, gzip when gz != 0 (2: compressed on the current device, see pcabi_reads_write_dev;
 *       any other value: zlib), appended when append != 0, path "-" = stdout (plain only);
 *       untrimmed != 0 writes reads without cuts whole (split parts still come from the trimmed
 *       sequence, as in the reference). Returns the number of reads that produced output (the
 *       reference's non-empty read strings, porechop_abi.py:598-604), or a negative PCABI_E_*.
 */
enum { PCABI_FASTA = 0, PCABI_FASTQ = 1 };
typedef struct pcabi_fastx pcabi_fastx;
typedef struct pcabi_reads pcabi_reads;
typedef struct pcabi_reads_view {
    int64_t n;
    int32_t type;
    const char *names;
    const int64_t *name_off;
    const char *seq;
    const int64_t *seq_off;
    const char *qual;
    const int64_t *qual_off;
    const uint8_t *rna;
    const char *spacer;
    const int64_t *spacer_off;
    const uint8_t *codes;
    int64_t codes_len;
    const int64_t *code_off;
    const int32_t *len;
} pcabi_reads_view;
int pcabi_fastx_open(const char *path, int raw, pcabi_fastx **out);
/* pcabi_fastx_open for a block-gzipped (BGZF) file read through GPU `device`: the file is mapped and
 * indexed at open (pcabi_gunzip_index); refills then come from groups of members inflated on a
 * stream of the reader's own (the next group while the parser works on the current one) instead of
 * zlib. A member that does not inflate is the reader's read error (PCABI_E_PARSE, "read error:
 * ..."), raised after the records before it. A plain file, a gzip file that is not indexable and
 * device < 0 behave exactly as pcabi_fastx_open. The calling thread's current device may change. */
int pcabi_fastx_open_dev(const char *path, int raw, int device, pcabi_fastx **out);
/* with flags (PCABI_OPEN_GUNZIP_PLAIN): see "gunzip on the device, streams without an index" */
int pcabi_fastx_open_dev2(const char *path, int raw, int device, int flags, pcabi_fastx **out);
int pcabi_fastx_type(const pcabi_fastx *r);
/* Byte-range reading of a plain (not gzip) file, for read shards split by position:
 *   pcabi_fastx_record_start : the first record start at or after `byte` (the file size if
 *       none): a FASTQ header line whose third line is the '+' line; a FASTA header with a name
 *       whose previous header has one too (an empty header's sequence runs on into the next
 *       record). Splitting at record starts gives every record to exactly one range.
 *   pcabi_fastx_set_range    : read only [begin, end) from now on (both record starts, or 0 / the
 *       file size); a fresh reader (no record read yet). */
int64_t pcabi_fastx_record_start(const pcabi_fastx *r, int64_t byte);
int pcabi_fastx_set_range(pcabi_fastx *r, int64_t begin, int64_t end);
/* Bytes of a plain file (or of its set range) not yet parsed; -1 for a gzip input, whose decoded
 * size is unknown. misc.read_batches sizes a pipeline's last batches from it (a ramp-down, so the
 * final write overlaps the trims before it). */
int64_t pcabi_fastx_remaining(const pcabi_fastx *r);
/* Streaming split of any input (gzip included) into spans of decoded text holding whole records,
 * for a distributor that hands spans to other readers (shards.trim_file_sharded): the next span,
 * at least max_bytes long unless the input ends (one record may overshoot), cut where a fresh
 * reader parses the same records as the continuous read -- FASTQ after a record whose successor's
 * first line starts with '@', FASTA before a header with a name whose preceding header has one.
 * *text is valid until the next call on r. Returns 1, 0 at the end of the input, or < 0. */
int pcabi_fastx_next_text(pcabi_fastx *r, int64_t max_bytes, const char **text, int64_t *len);
int64_t pcabi_fastx_next(pcabi_fastx *r, int64_t max_reads, int64_t max_bases, pcabi_reads **out);
void pcabi_fastx_close(pcabi_fastx *r);
int pcabi_fastx_load(const char *path, int raw, pcabi_reads **out);
int64_t pcabi_reads_count(const pcabi_reads *b);
int pcabi_reads_type(const pcabi_reads *b);
int pcabi_reads_views(const pcabi_reads *b, pcabi_reads_view *v);
void pcabi_reads_free(pcabi_reads *b);
int pcabi_reads_write(const pcabi_reads *b, const char *path, int append, int gz, int fasta,
                      const int32_t *start_trim, const int32_t *end_trim, const int64_t *cut_off,
                      const int64_t *cuts, int min_split_read_size, int discard_middle,
                      int untrimmed, const uint8_t *select);
/* Batches of 64 MB and more live in huge-page mappings that freed batches hand to a process-wide
 * cache (PCABI_IO_CACHE_MB, default min(4 GB, RAM / 8)) for the next batch to reuse; this
 * returns every cached mapping to the system. */
void pcabi_io_release_cache(void);
/* pcabi_reads_write with gz = 2, "compress on the device", on device `gzip_device` (-1 = the
 * calling thread's current device; pcabi_reads_write itself uses that for gz = 2). The records are
 * laid out exactly as for a plain file, cut into blocks by pcabi_gzip_plan_lines (PCABI_GZIP_LONG_LINE,
 * blocks up to 65535 bytes), compressed by pcabi_gzip_host and written or appended as gzip members:
 * the file decompresses to the bytes gz = 0 writes. gz = 3: the same through pcabi_bgzf_host, one
 * indexed BGZF member per block of at most 65280 bytes, without the end-of-file marker
 * (pcabi_bgzf_write_eof finishes the file). gz = 0 / 1 behave as in pcabi_reads_write. */
int pcabi_reads_write_dev(const pcabi_reads *b, const char *path, int append, int gz, int fasta,
                          const int32_t *start_trim, const int32_t *end_trim, const int64_t *cut_off,
                          const int64_t *cuts, int min_split_read_size, int discard_middle,
                          int untrimmed, const uint8_t *select, int gzip_device);
/* Seconds the calling thread's last pcabi_reads_write / _dev call spent laying out the records (plain
 * files and gz = 2), compressing on the device (gz = 2) and writing the file (tools/gz_timing.py); after
 * pcabi_reads_write_bam: the part table, side blob and plan (and the host pack when device < 0), the
 * device call or zlib, and writing the file (tools/bam_write_timing.py). */
void pcabi_reads_write_last_times(double *layout, double *compress, double *write);

/* ---- gzip on the device (csrc/pcabi_deflate.hip) ----------------------------------------
 * A gzip stream (RFC 1952 members of RFC 1951 blocks) of a byte buffer, compressed per block with
 * no LZ77 matches: block k = bytes [block_off[k], block_off[k + 1]) (block_off[0] = 0,
 * block_off[n_blocks] = n, every block 1..65535 bytes) becomes one dynamic-Huffman deflate block
 * followed by an empty stored block (so the next block starts on a byte), or one stored block when
 * that is not larger. block_off = NULL: fixed blocks of pcabi_gzip_block_len() bytes (n_blocks is
 * ignored). Blocks are grouped into members, each with the CRC-32 (computed on the device) and
 * ISIZE of its own bytes; the stream is multi-member, an empty input gives one empty member.
 *   pcabi_gzip_bound        : capacity that always suffices (n_blocks = 0: fixed blocks).
 *   pcabi_gzip_scratch_bytes: device scratch pcabi_gzip_dev needs.
 *   pcabi_gzip_dev  : device pointers on the current device, asynchronous on `stream`, no host
 *       synchronisation. *out_len (device) receives the stream length; when it exceeds cap nothing
 *       is written to out; -1 (and nothing written) when the block list is not as described.
 *       Returns 0 or a negative PCABI_E_*.
 *   pcabi_gzip_host : host buffers (pageable), staged through pinned chunks so copies and kernels
 *       overlap. Returns the stream length or a negative PCABI_E_* (a bad block list is refused
 *       before anything is launched). When the length exceeds cap, out[cap..] is untouched and
 *       out[0..cap) undefined: call again with the returned size. device -1 = current device.
 *   pcabi_gzip_plan_lines : the writer's block list for text (host): a block never spans the end
 *       of a line of long_line bytes or more, shorter lines are merged into neighbouring blocks up
 *       to cap bytes, longer spans are cut evenly (long_line <= cap <= 65535). Writes
 *       block_off[0 .. blocks] when blocks + 1 <= off_cap; returns the number of blocks.
 *   pcabi_gzip_tune : test switches, process-wide: fixed block length, blocks per member, bytes per
 *       staged pass of pcabi_gzip_host (0 = the default: 32768, 1024, 64 MiB).
 *   pcabi_gzip_last_times : seconds the last pcabi_gzip_host call spent copying into pinned
 *       memory, waiting for the device, and copying out of pinned memory.
 */
enum { PCABI_GZIP_LONG_LINE = 1024, PCABI_GZIP_BLOCK_CAP = 65535 };
int pcabi_gzip_block_len(void);
int64_t pcabi_gzip_bound(int64_t n, int64_t n_blocks);
int64_t pcabi_gzip_scratch_bytes(int64_t n, int64_t n_blocks);
int pcabi_gzip_tune(int block_len, int64_t member_blocks, int64_t chunk_bytes);
int pcabi_gzip_dev(void *stream, const uint8_t *in, int64_t n, const int64_t *block_off, int64_t n_blocks,
                   uint8_t *out, int64_t cap, int64_t *out_len, void *scratch, int64_t scratch_len);
int64_t pcabi_gzip_host(int device, const uint8_t *in, int64_t n, const int64_t *block_off, int64_t n_blocks,
                        uint8_t *out, int64_t cap);
int64_t pcabi_gzip_plan_lines(const char *text, int64_t n, int64_t long_line, int64_t cap, int64_t *block_off,
                              int64_t off_cap);
void pcabi_gzip_last_times(double *copy_in, double *wait, double *copy_out);
/* BGZF output from the same encoder (opt-in): one gzip member per block, each with the 18-byte BGZF
 * header (1f 8b 08 04, MTIME 0, XFL 0, OS ff, XLEN 6, "BC" 02 00, BSIZE = member bytes - 1), the
 * block encoded exactly as above (its sync marker and the closing empty fixed block included),
 * CRC-32 and ISIZE. Blocks hold 1..PCABI_BGZF_BLOCK_CAP (65280) bytes, so that a stored block with
 * all overhead stays within 65536; block_off = NULL: fixed blocks of min(pcabi_gzip_block_len(),
 * 65280); a longer block is refused like any bad list. Such a stream is indexable: bgzip -d,
 * samtools, htslib and pcabi_gunzip_* read it member by member.
 *   pcabi_bgzf_bound : capacity that always suffices (n_blocks = 0: fixed blocks).
 *   pcabi_bgzf_host  : as pcabi_gzip_host; eof != 0 appends the standard 28-byte end-of-file member
 *       (1f8b08040000000000ff0600424302001b0003000000000000000000). No bytes give no member.
 *   pcabi_bgzf_dev   : as pcabi_gzip_dev (device pointers, asynchronous, no host synchronisation):
 *       in[0, n) in members of block_len (1..65280) bytes, the last one shorter; scratch of
 *       pcabi_bgzf_scratch_bytes(n, block_len). No marker. The BAM writer's encoder entry.
 *   pcabi_bgzf_write_eof : appends that marker to a file.
 *   pcabi_reads_write_dev(..., gz = 3, ...) is the record writer in this mode (blocks planned with cap
 *       65280); it never writes the marker, so appended batches stay one contiguous chain. */
int64_t pcabi_bgzf_bound(int64_t n, int64_t n_blocks, int eof);
int64_t pcabi_bgzf_host(int device, const uint8_t *in, int64_t n, const int64_t *block_off, int64_t n_blocks, int eof,
                        uint8_t *out, int64_t cap);
int64_t pcabi_bgzf_scratch_bytes(int64_t n, int64_t block_len);
int pcabi_bgzf_dev(void *stream, const uint8_t *in, int64_t n, int64_t block_len, uint8_t *out, int64_t cap,
                   int64_t *out_len, void *scratch, int64_t scratch_len);
int pcabi_bgzf_write_eof(const char *path);

/* ---- gunzip on the device (csrc/pcabi_inflate.hip) --------------------------------------
 * Block-gzipped input (BGZF, what bgzip / htslib write): a gzip stream whose every member carries
 * its own compressed size in the header's BC extra subfield and decodes to at most 65536 bytes.
 * The host lists the members without decoding a byte; the device inflates them, one workgroup per
 * member: RFC 1951 in full (stored, fixed and dynamic blocks, LZ77 matches), ISIZE and CRC-32
 * checked. One int32 status per member: 0, or a PCABI_INFLATE_E_* below.
 *   pcabi_gunzip_index : (host) walks the members of z[0, n) by their headers (FEXTRA with any
 *       number of subfields, of which BC with SLEN 2 gives BSIZE = member bytes - 1). Writes
 *       in_off[0..m] (member starts, in_off[m] = n) and out_off[0..m] (prefix sums of ISIZE) when
 *       m + 1 <= cap; returns m. Returns 0, nothing written, when the stream is not indexable (a
 *       member without BC, with CM != 8 or with ISIZE > 65536): use zlib then. PCABI_E_PARSE when
 *       a member does not start with the gzip magic or the chain runs past n (truncated file). The
 *       empty 28-byte end-of-file member is an ordinary member with ISIZE 0, anywhere.
 *   pcabi_gunzip_scratch_bytes : device scratch pcabi_gunzip_dev needs (0 today: the decode tables
 *       live in LDS; scratch may then be NULL).
 *   pcabi_gunzip_dev : device pointers on the current device, asynchronous on `stream`, no host
 *       synchronisation. Member k = z[in_off[k], in_off[k + 1]) decodes into out[out_off[k],
 *       out_off[k + 1]). A member whose status is non-zero leaves its output range undefined and
 *       touches nothing outside it; a member whose ranges do not lie inside [0, n) / [0, out_cap)
 *       (an out_cap too small, for one) gets PCABI_INFLATE_E_OUTPUT / _E_HEADER and writes
 *       nothing. Returns 0 or a negative PCABI_E_* for bad arguments.
 *   pcabi_gunzip_host : host buffers (pageable): indexes, then stages groups of members through
 *       pinned chunks so copies and kernels overlap. Returns the decoded length; the needed length,
 *       with out untouched, when cap is smaller; PCABI_E_PARSE when a member fails (the message
 *       names the first failing member's index, offset and status); PCABI_E_ARG when the stream is
 *       not indexable. device -1 = current device.
 *   pcabi_gunzip_tune : test switch, process-wide: decoded bytes per staged pass of
 *       pcabi_gunzip_host and per refill group of the reader (0 = the default, 32 MiB).
 *   pcabi_gunzip_last_times : seconds the last pcabi_gunzip_host call spent copying into pinned
 *       memory, waiting for the device, and copying out of pinned memory.
 */
enum { PCABI_BGZF_BLOCK_CAP = 65280, PCABI_BGZF_MEMBER_MAX = 65536 };
enum {
    PCABI_INFLATE_E_HEADER = 1,   /* bad gzip or block header                  */
    PCABI_INFLATE_E_CODE = 2,     /* bad Huffman code or symbol                */
    PCABI_INFLATE_E_DIST = 3,     /* distance before the member's first byte   */
    PCABI_INFLATE_E_INPUT = 4,    /* ran out of input                          */
    PCABI_INFLATE_E_OUTPUT = 5,   /* more output than ISIZE                    */
    PCABI_INFLATE_E_LENGTH = 6,   /* less output than ISIZE                    */
    PCABI_INFLATE_E_CRC = 7       /* CRC-32 mismatch                           */
};
int64_t pcabi_gunzip_index(const uint8_t *z, int64_t n, int64_t *in_off, int64_t *out_off, int64_t cap);
int64_t pcabi_gunzip_scratch_bytes(int64_t n_members);
int pcabi_gunzip_dev(void *stream, const uint8_t *z, int64_t n, const int64_t *in_off, const int64_t *out_off,
                     int64_t n_members, uint8_t *out, int64_t out_cap, int32_t *status, void *scratch,
                     int64_t scratch_len);
int64_t pcabi_gunzip_host(int device, const uint8_t *z, int64_t n, uint8_t *out, int64_t cap);
int pcabi_gunzip_tune(int64_t chunk_bytes);
void pcabi_gunzip_last_times(double *copy_in, double *wait, double *copy_out);

/* ---- gunzip on the device, streams without an index (csrc/pcabi_gzstream.hip) ------------
 * Ordinary gzip (what gzip, pigz and the sequencers write: one deflate stream per member, no BC
 * subfield), opt-in. The compressed bytes are processed in spans of span_bytes, each cut at
 * multiples of chunk_bytes: every cut looks for the first place a block may start (a non-final
 * dynamic block header that parses, or a member header), a decoder starts there with the unknown
 * 32768 bytes before it kept as symbolic markers and stops at the first block boundary that is
 * another cut's candidate. The host follows the chain from the span's known start, sizes the
 * chunks on it, and the device hands the windows down the chain, replaces the markers and computes
 * the CRC-32 of every piece; each member's CRC-32 and ISIZE (modulo 2^32) are checked against its
 * trailer. A span with fewer than min_chunks chunks on the chain, or whose chain breaks at its
 * start, goes through zlib's raw inflate from the same bit with the same window. The decoded bytes
 * are zlib's either way; trailing bytes that are no member start are ignored, as gzread does.
 *   pcabi_gunzip_stream_host : host buffers (pageable), any gzip stream, a BGZF one included.
 *       Returns the decoded length; the needed length, with out untouched, when cap is smaller;
 *       PCABI_E_PARSE when the stream is bad (the message names the member's index, its byte offset
 *       and the PCABI_INFLATE_E_* status). An empty input decodes to nothing. device -1 = current.
 *   pcabi_gunzip_stream_tune : test switch, process-wide: compressed bytes per chunk and per span,
 *       and the fewest chunks on a span's chain that keep it on the device (0 = the default of each:
 *       64 KiB, 64 MiB, 1).
 *   pcabi_gunzip_stream_last_stats : s[0..6] of the last pcabi_gunzip_stream_host call, or of the
 *       reader last read from, on this thread: spans, chunk cuts, chunks on the chain, rejected
 *       candidates, members, bytes decoded on the device, bytes decoded by the host fallback.
 *   pcabi_gunzip_stream_last_times : milliseconds from device events, summed since the last call
 *       with reset != 0: ms[0] finder, ms[1] counting pass, ms[2] decode, ms[3] window hand-down,
 *       ms[4] resolve. Events are recorded (and every kernel waited for) only while on = 1; on = 0
 *       turns that off; -1 leaves it.
 *   pcabi_fastx_open_dev2 : pcabi_fastx_open_dev with flags. PCABI_OPEN_GUNZIP_PLAIN: a gzip file
 *       that is not block-gzipped is read through this path, span by span on a stream and a thread
 *       of the reader's own, so the next span inflates while the parser works on the current one. A
 *       BGZF file still takes the indexed path; a BAM file that is not block-gzipped reads through
 *       zlib. Errors are the zlib path's: the records before the bad place, then the read error.
 * There is no entry with device pointers: following the chain and sizing the chunks need the host
 * between the kernels. */
enum { PCABI_OPEN_GUNZIP_PLAIN = 1 };
int64_t pcabi_gunzip_stream_host(int device, const uint8_t *z, int64_t n, uint8_t *out, int64_t cap);
int pcabi_gunzip_stream_tune(int64_t chunk_bytes, int64_t span_bytes, int64_t min_chunks);
void pcabi_gunzip_stream_last_stats(int64_t *s);
void pcabi_gunzip_stream_last_times(int on, int reset, double *ms);

/* ---- unaligned BAM input (csrc/pcabi_bam.h, csrc/pcabi_bam.hip) ------------------------------
 * The reader (pcabi_fastx_open / pcabi_fastx_open_dev) takes a BAM file as a third input type: its
 * first four decoded bytes are "BAM\1". Batches are PCABI_FASTQ batches: name = read name, sequence
 * letters over "=ACMGRSVTWYHKDBN", qualities q + 33 ('+' for every base when they are absent), rna 0,
 * empty spacer; secondary (0x100) and supplementary (0x800) records are skipped, reverse-strand
 * records (0x10) are reverse-complemented, tags are dropped unless pcabi_fastx_keep_aux asks for them. pcabi_fastx_open_dev unpacks the
 * records on the device next to the inflated bytes. pcabi_fastx_remaining returns -1;
 * pcabi_fastx_set_range, pcabi_fastx_record_start and pcabi_fastx_next_text refuse a BAM reader
 * (PCABI_E_ARG). An invalid record, a truncated record chain, a member that does not inflate or
 * "BAM" with another version byte is PCABI_E_PARSE ("read error: ..."), raised by the call after
 * the one that delivered the records before the fault.
 *   pcabi_bam_index : (host) bam[0, n) is a whole inflated BAM file. Skips the header, walks the
 *       record chain and writes the kept records to recs[0, cap) with their output offsets in the
 *       batch layout (sequence and qualities back to back, codes at 4-aligned starts). totals[0..4]
 *       (may be NULL) = sequence bytes, quality bytes, code bytes (16 bytes of tail padding
 *       included), name bytes, tiles. Returns the number of kept records (write again with a larger
 *       cap when it exceeds cap) or PCABI_E_PARSE.
 *   pcabi_bam_unpack_dev : device pointers on the current device, asynchronous on `stream`: the
 *       records of recs[0, n_recs) (a table pcabi_bam_index made, tile0 ascending) from bam[0, n)
 *       into seq / qual / codes. Every record writes its own ranges only: l_seq bytes of seq and
 *       qual, l_seq rounded up to four bytes of codes (padding = 4); codes[tail_off, tail_off + 16)
 *       is filled with 4 when tail_off >= 0. A record that does not lie inside the buffers writes
 *       nothing. Returns 0 or PCABI_E_ARG.
 *   pcabi_bam_unpack_host : the same with host buffers, staged through the device; device < 0 runs
 *       the host build of the same code (no GPU needed). Table entries outside the buffers are
 *       refused (PCABI_E_ARG). On the device every output starts as far off a 16-byte boundary as
 *       the caller's pointer and lies between 64 guard bytes, which are checked after the kernel
 *       (PCABI_E_DEVICE if it wrote outside an output).
 *   pcabi_bam_last_times : milliseconds the device reader spent, from device events, since the last
 *       call with reset != 0: ms[0] k_inflate, ms[1] k_bam_unpack, ms[2] copies to the device,
 *       ms[3] copies from the device; bytes[0] = bytes k_bam_unpack read and wrote. Events are only
 *       recorded while profiling is on (on = 1; on = 0 turns it off; -1 leaves it).
 */
typedef struct pcabi_bam_rec {
    int64_t rec;        /* the record's start (its block_size field) in the inflated bytes   */
    int64_t seq_out;    /* output offsets of base 0: sequence, qualities, codes              */
    int64_t qual_out;
    int64_t code_out;
    int64_t tile0;      /* tiles of the records before this one (16384 bases per tile)        */
    int32_t seq_at;     /* the packed sequence's offset from rec; the qualities follow it    */
    int32_t l_seq;
    int32_t flag;
    int32_t name_len;   /* the name is at rec + 36                                           */
} pcabi_bam_rec;
int64_t pcabi_bam_index(const uint8_t *bam, int64_t n, pcabi_bam_rec *recs, int64_t cap, int64_t *totals);
int pcabi_bam_unpack_dev(void *stream, const uint8_t *bam, int64_t n, const pcabi_bam_rec *recs, int64_t n_recs,
                         int64_t n_tiles, uint8_t *seq, int64_t seq_cap, uint8_t *qual, int64_t qual_cap,
                         uint8_t *codes, int64_t codes_cap, int64_t tail_off);
int pcabi_bam_unpack_host(int device, const uint8_t *bam, int64_t n, const pcabi_bam_rec *recs, int64_t n_recs,
                          uint8_t *seq, int64_t seq_cap, uint8_t *qual, int64_t qual_cap, uint8_t *codes,
                          int64_t codes_cap, int64_t tail_off);
void pcabi_bam_last_times(int on, int reset, double *ms, int64_t *bytes);

/* ---- unaligned BAM output (csrc/pcabi_bam.h, csrc/pcabi_bam.hip, csrc/pcabi_write.cpp) -------
 * The inverse of the unpack: parts of a batch (whole reads, trimmed reads, split pieces) laid out as
 * a chain of unmapped BAM records. One pcabi_bam_part per output record; a record is
 *   block_size | refID -1 | pos -1 | l_read_name = name_len + 1 | mapq 0 | bin 4680 | n_cigar_op 0 |
 *   flag 4 | l_seq | next_refID -1 | next_pos -1 | tlen 0 | name NUL | seq u8[(l_seq + 1) / 2] |
 *   qual u8[l_seq] | aux
 * of 36 + name_len + 1 + (l_seq + 1) / 2 + l_seq + aux_len bytes. Letters become codes over
 * "=ACMGRSVTWYHKDBN" (U -> T, any other byte -> N), the earlier base in the high nibble, the low
 * nibble of an odd last byte 0; qualities are the character - 33 clamped to 0..93, or 0xFF for every
 * base when qual_src < 0. The name and the aux bytes of a part lie back to back in a side blob.
 *   pcabi_bam_pack_plan : (host) fills out / tile0 of parts[0, n_parts) for a chain that starts at
 *       out0 and returns the chain's end; tiles[0] (may be NULL) = the tile count. Every part owns
 *       max(1, ceil(l_seq / 16384)) tiles. PCABI_E_ARG for a negative length or a name over 254 bytes.
 *   pcabi_bam_pack_dev  : device pointers on the current device, asynchronous on `stream`: the parts
 *       (a planned table, tile0 ascending) from seq[0, seq_n) / qual[0, qual_n) / side[0, side_n)
 *       into out[0, out_cap). A part writes its own record's bytes only; a part that does not lie
 *       inside the buffers writes nothing. Returns 0 or PCABI_E_ARG.
 *   pcabi_bam_pack_host : the same with host buffers, staged through the device; device < 0 runs the
 *       host build of the same code (no GPU needed). Table entries outside the buffers, or not
 *       planned, are refused (PCABI_E_ARG). On the device the output starts as far off a 16-byte
 *       boundary as the caller's pointer and lies between 64 guard bytes, which are checked after the
 *       kernel (PCABI_E_DEVICE if it wrote outside). Bytes no part owns keep their values.
 *   pcabi_bam_pack_last_times : milliseconds k_bam_pack took (device events) and the bytes it read
 *       and wrote since the last call with reset != 0, counted while pcabi_bam_last_times' profiling
 *       is on.
 *   pcabi_reads_write_bam : pcabi_reads_write_dev's arguments (without gz and fasta) for a BAM file.
 *       The same parts as the text writers': trims, split parts, "_k" names, min_split_read_size,
 *       discard_middle, untrimmed, select, and the same return value. A record's name is the header
 *       up to its first space or tab (the rest of the header is dropped), cut to 254 bytes, "*" when
 *       empty; an RNA read's bases are written as T; a FASTA batch writes absent qualities (0xFF); a
 *       quality-less FASTQ record's '+' padding is written as Phred 10. append == 0 first writes the
 *       BAM header: "BAM\1", header_text[0, header_len) ("@HD\tVN:1.6\tSO:unknown\n" when NULL),
 *       n_ref = 0. The header and the record chain are one byte stream, cut into BGZF members of
 *       65280 bytes (the last one shorter; records may span members). No end-of-file marker is
 *       written: pcabi_bgzf_write_eof finishes the file, so batches can be appended. device >= 0:
 *       the text, the part table and the side blob go up, k_bam_pack writes the stream into device
 *       memory, the BGZF encoder reads it there and only compressed bytes come back; device < 0: the
 *       host build of the pack and zlib raw deflate per member on the io threads. Both inflate to the
 *       same bytes. keep_aux != 0 writes the aux tags a BAM reader kept (pcabi_fastx_keep_aux): a
 *       part that is its whole read, with the read's bases as stored, gets them verbatim; any other
 *       part gets them without the position-dependent tags MM ML MN Mm Ml mv, which are dropped and
 *       not recomputed. keep_aux = 2 recomputes MM ML MN Mm Ml instead (the block below); mv and
 *       ts are remapped by pcabi_reads_write_bam_tags ("move tables" below), here mv is dropped.
 *   pcabi_fastx_keep_aux : before the first pcabi_fastx_next, on = 1 makes a BAM reader keep every
 *       kept record's aux bytes and whether its bases are stored as written (not reverse-strand); any
 *       other input: no effect (pcabi_fastx_header_tags fills a FASTA / FASTQ batch's). A record whose aux chain does not walk (types A c C s S i I f Z H B)
 *       is then PCABI_E_PARSE, raised after the records before it.
 *   pcabi_reads_aux : a batch's aux bytes: read i's are aux[aux_off[i], aux_off[i + 1]); as_stored[i].
 *       All three NULL when the batch holds none.
 *   pcabi_fastx_bam_header : a BAM reader's header text (valid until close) once a batch was read;
 *       *len = 0 for any other input.
 */
typedef struct pcabi_bam_part {
    int64_t seq_src;    /* base 0 in the sequence buffer (one letter per byte)                   */
    int64_t qual_src;   /* base 0 in the quality buffer (character = q + 33); < 0: absent, 0xFF  */
    int64_t side_off;   /* the name (name_len bytes), then the aux bytes (aux_len), in the blob  */
    int64_t out;        /* the record's start (its block_size field) in the output stream        */
    int64_t tile0;      /* tiles of the parts before this one (16384 bases; at least one a part) */
    int32_t l_seq;
    int32_t name_len;
    int32_t aux_len;
    int32_t reserved;
} pcabi_bam_part;
int64_t pcabi_bam_pack_plan(pcabi_bam_part *parts, int64_t n_parts, int64_t out0, int64_t *tiles);
int pcabi_bam_pack_dev(void *stream, const uint8_t *seq, int64_t seq_n, const uint8_t *qual, int64_t qual_n,
                       const uint8_t *side, int64_t side_n, const pcabi_bam_part *parts, int64_t n_parts,
                       int64_t n_tiles, uint8_t *out, int64_t out_cap);
int pcabi_bam_pack_host(int device, const uint8_t *seq, int64_t seq_n, const uint8_t *qual, int64_t qual_n,
                        const uint8_t *side, int64_t side_n, const pcabi_bam_part *parts, int64_t n_parts,
                        uint8_t *out, int64_t out_cap);
void pcabi_bam_pack_last_times(int reset, double *ms, int64_t *bytes);
int pcabi_reads_write_bam(const pcabi_reads *b, const char *path, int append, const int32_t *start_trim,
                          const int32_t *end_trim, const int64_t *cut_off, const int64_t *cuts,
                          int min_split_read_size, int discard_middle, int untrimmed, const uint8_t *select,
                          const char *header_text, int64_t header_len, int keep_aux, int device);
int pcabi_fastx_keep_aux(pcabi_fastx *r, int on);
int pcabi_reads_aux(const pcabi_reads *b, const uint8_t **aux, const int64_t **aux_off, const uint8_t **as_stored);
int pcabi_fastx_bam_header(const pcabi_fastx *r, const char **text, int64_t *len);

/* ---- base-modification tags remapped onto parts (csrc/pcabi_mods.h, csrc/pcabi_mods.hip) ------
 * MM / ML / MN (SAMtags "Base modifications"; Mm / Ml are the older spellings) count occurrences of a
 * base along the read, so a trimmed read or a split piece needs them recomputed. An MM group
 * `base strand codes [flag] (,count)* ;` marks ordinals o0 = d0, ok = o(k-1) + 1 + dk among the
 * occurrences of its base (U counts T, N counts every base) in the read as the reader returns it (a
 * reverse-strand record already reverse-complemented). For a part [s0, s0 + ns) with c0 occurrences
 * before its start and c1 before its end a group keeps the entries c0 <= ordinal < c1 and is written
 * as its header, verbatim, then the kept counts -- the first as ordinal - c0, the others byte for byte
 * as they stood -- then ';'; a group that keeps nothing is its header and ';'. ML (B:C, one value per
 * entry per code) keeps the kept entries' values and is written whenever the read had one, MN whenever
 * the read had one, as type i with value ns. A part's tag bytes are MM, ML, MN in this order, under
 * the spellings they came in.
 * A read's tags are usable when: the MM text is well formed; it has at most 32 groups; every count
 * fits int32; in every group the last ordinal is below the read's count of that base; ML, if present,
 * holds exactly sum(entries * codes) values; MN, if present, equals the read's length; and the caller
 * found exactly one MM tag, of type Z, no ML without it, ML of type B:C, MN an integer
 * (PCABI_MODS_BAD otherwise). The parts of a read that is not usable get no tag bytes (length 0).
 *   pcabi_mods_read : one read that carries any of the tags. Its letters, its MM text (without the
 *       NUL) and its ML values, as offsets into a sequence buffer and a tag blob; its parts are
 *       parts[part0, part0 + n_parts).
 *   pcabi_mods_part : [s0, s0 + ns) of read `read`; len = the length of its tag bytes, out = where
 *       they go.
 *   pcabi_mods_plan  : fills parts[].len and usable[0, n_reads) (1 usable, 0 not), and adds the reads
 *       to the counters. device >= 0: the letters, the tag blob and the tables go up, the device
 *       parses the MM text into ordinals, counts every group's base up to each part boundary and
 *       selects each part's entries; the lengths and the flags come back. device < 0: the host build
 *       of the same code (no GPU needed). A read or a part that points outside its buffers, or a part
 *       outside its read's range of the table, is refused (PCABI_E_ARG).
 *   pcabi_mods_remap : writes every part's tag bytes to out[part.out, part.out + part.len). parts[]
 *       as pcabi_mods_plan left them, with out set; a len that is not what the plan gives, ranges that
 *       overlap or an out outside out[0, out_cap) are refused (PCABI_E_ARG). On the device the output
 *       lies between 64 guard bytes, checked after the kernel (PCABI_E_DEVICE if it wrote outside).
 *       Bytes no part owns keep their values.
 *   pcabi_mods_counts : reads remapped and reads whose modification tags were dropped (not usable),
 *       as pcabi_mods_plan and pcabi_reads_write_bam(keep_aux = 2) counted them since the last call
 *       with reset != 0.
 *   pcabi_mods_last_times : ms[0..3] = milliseconds k_mods_plan and k_mods_write took (device events,
 *       counted while pcabi_bam_last_times' profiling is on), the wall time of the host build
 *       (device < 0, on the io threads) and the wall time of the device's sizing step (the tag blob
 *       and the tables up, k_mods_plan, the lengths back, and whatever the stream still held);
 *       *bytes = what the two kernels read and wrote; all since the last call with reset != 0.
 * pcabi_reads_write_bam with keep_aux = 2 keeps the tags as keep_aux = 1 does and remaps these: a
 * changed read's part (a trimmed read, a split piece, a read from a reverse-strand record) gets its
 * other tags in file order, then MM, ML, MN by the rule above; a read whose tags are not usable loses
 * MM ML MN Mm Ml from all its parts, as with keep_aux = 1. mv: see "move tables" below. With device >= 0
 * the remap runs there before k_bam_pack, into the device copy of the side blob.
 */
#define PCABI_MODS_OLD_MM 1 /* the MM tag was spelled Mm */
#define PCABI_MODS_BAD 2    /* the caller found the read's tags unusable */
#define PCABI_MODS_OLD_ML 4 /* the ML tag was spelled Ml */
typedef struct pcabi_mods_read {
    int64_t seq_off; /* the read's letters in the sequence buffer, in the reader's orientation */
    int64_t mm_off;  /* the MM text in the tag blob                                            */
    int64_t ml_off;  /* the ML values in the tag blob                                          */
    int64_t part0;   /* its parts in the part table                                            */
    int32_t l_seq;
    int32_t mm_len;  /* < 0: no MM tag                                                         */
    int32_t ml_len;  /* < 0: no ML tag                                                         */
    int32_t mn;      /* < 0: no MN tag                                                         */
    int32_t n_parts;
    int32_t flags;   /* PCABI_MODS_*                                                           */
} pcabi_mods_read;
typedef struct pcabi_mods_part {
    int64_t out; /* where the tag bytes go                 */
    int32_t read;
    int32_t s0, ns;
    int32_t len; /* the tag bytes' length (pcabi_mods_plan) */
} pcabi_mods_part;
int pcabi_mods_plan(int device, const uint8_t *seq, int64_t seq_n, const uint8_t *tags, int64_t tags_n,
                    const pcabi_mods_read *reads, int64_t n_reads, pcabi_mods_part *parts, int64_t n_parts,
                    uint8_t *usable);
int pcabi_mods_remap(int device, const uint8_t *seq, int64_t seq_n, const uint8_t *tags, int64_t tags_n,
                     const pcabi_mods_read *reads, int64_t n_reads, const pcabi_mods_part *parts, int64_t n_parts,
                     uint8_t *out, int64_t out_cap);
void pcabi_mods_counts(int reset, int64_t *remapped, int64_t *dropped);
void pcabi_mods_last_times(int reset, double *ms, int64_t *bytes);

/* ---- move tables remapped onto parts (csrc/pcabi_moves.h, csrc/pcabi_moves.hip) ---------------
 * mv is the basecaller's move table, a B:c array (B:C is accepted): the stride S, then n moves of 0 or
 * 1, each covering S samples of the signal; a 1 starts a base. ts is the number of samples trimmed
 * before the read; the moves count from it. With `ones` the number of 1s, p(k) the index of the k-th 1
 * (from 0) and p(ones) = n, a part [s0, s0 + ns) of the read, in the orientation the reader returns it
 * (nothing is reversed for a reverse-strand record), takes the moves [q0, q1): q0 = 0 when s0 == 0
 * (blocks before the first base stay with a part that starts the read), else p(s0); q1 = p(s0 + ns).
 * Its tag bytes are `mv B c`, the count 1 + q1 - q0, S and the slice byte for byte (subtype c whatever
 * came in), then, when the read had a ts tag, `ts i` with ts + S * q0. Ascending parts that tile the
 * read concatenate to the original moves, and each slice holds ns ones.
 * A read's table is usable when: there is exactly one mv tag, of type B:c or B:C (PCABI_MOVES_BAD
 * otherwise); it has at least one value; 1 <= S <= 127; every move is 0 or 1; ones == l_seq; its ts, if
 * any, is one integer tag (c C s S i I) with a value >= 0 (PCABI_MOVES_BAD otherwise: negative, another
 * type, or twice), and ts + S * q0 <= INT32_MAX for all its parts. The first move need not be 1. The
 * parts of a read that is not usable get no tag bytes (length 0). A table of more than INT32_MAX - 64
 * values is refused (no BAM record holds one).
 * Out of scope: direct-RNA files, whose move tables run against the sequence without the record saying
 * so; the sp and pi tags of split reads. ns (the sample count before
 * trimming) does not depend on the position and stays with the other tags.
 *   pcabi_moves_read : one read with an mv tag: mv_off = the first value of the array (the stride) in
 *       the tag blob, n_vals = how many values (stride included), ts < 0 = no ts tag; its parts are
 *       parts[part0, part0 + n_parts).
 *   pcabi_moves_part : [s0, s0 + ns) of read `read`; len = the length of its tag bytes (mv, then ts),
 *       out = where they go.
 *   pcabi_moves_plan  : fills parts[].len and usable[0, n_reads) and adds the reads to the counters.
 *       device >= 0: the tag blob and the tables go up; k_moves_count counts the ones of fixed 4096-move
 *       segments of all reads (16 bytes a lane a load, any alignment), a device scan turns the counts
 *       into prefixes, k_moves_select finds each part boundary's move (a binary search over the read's
 *       segments, then 64 bytes a pass with a ballot), k_moves_size decides usability and sizes the
 *       parts; 4 bytes a part and one a read come back. device < 0: the host build of the same code (no
 *       GPU needed). Tables that point outside their buffers are refused (PCABI_E_ARG).
 *   pcabi_moves_remap : writes every part's tag bytes to out[part.out, part.out + part.len); refusals
 *       and the 64 guard bytes on the device as for pcabi_mods_remap. Bytes no part owns keep their
 *       values.
 *   pcabi_moves_counts : reads remapped and reads whose mv was dropped (not usable) since the last call
 *       with reset != 0.
 *   pcabi_moves_last_times : ms[0..5] = milliseconds of k_moves_count, the scan, k_moves_select with
 *       k_moves_size, and k_moves_write (device events, counted while pcabi_bam_last_times' profiling
 *       is on), the wall time of the host build (device < 0, on the io threads) and the wall time of
 *       the device's sizing step (blob and tables up, the three stages, the lengths back); *bytes = what
 *       the kernels read and wrote; all since the last call with reset != 0.
 * pcabi_reads_write_bam_tags is pcabi_reads_write_bam with tag_flags: PCABI_BAM_KEEP_MOVES (with
 * keep_aux != 0) gives every changed part of a usable read its mv and its rewritten ts, behind the
 * other tags in file order (without ts when it is rewritten) and behind MM ML MN when keep_aux = 2; a
 * read that is not usable loses mv from its changed parts and keeps ts verbatim. tag_flags = 0 writes
 * what pcabi_reads_write_bam writes. With device >= 0 the move tables are sized in the same round trip
 * as the modification tags and written into the device copy of the side blob before k_bam_pack.
 */
#define PCABI_MOVES_BAD 1      /* the caller found the read's mv or ts unusable */
#define PCABI_BAM_KEEP_MOVES 1 /* pcabi_reads_write_bam_tags tag_flags */
typedef struct pcabi_moves_read {
    int64_t mv_off; /* the array's first value (the stride) in the tag blob */
    int64_t part0;  /* its parts in the part table                          */
    int32_t l_seq;
    int32_t n_vals; /* values of the array, the stride included             */
    int32_t ts;     /* < 0: no ts tag                                       */
    int32_t n_parts;
    int32_t flags;  /* PCABI_MOVES_*                                        */
} pcabi_moves_read;
typedef struct pcabi_moves_part {
    int64_t out; /* where the tag bytes go                  */
    int32_t read;
    int32_t s0, ns;
    int32_t len; /* the tag bytes' length (pcabi_moves_plan) */
} pcabi_moves_part;
int pcabi_moves_plan(int device, const uint8_t *tags, int64_t tags_n, const pcabi_moves_read *reads, int64_t n_reads,
                     pcabi_moves_part *parts, int64_t n_parts, uint8_t *usable);
int pcabi_moves_remap(int device, const uint8_t *tags, int64_t tags_n, const pcabi_moves_read *reads, int64_t n_reads,
                      const pcabi_moves_part *parts, int64_t n_parts, uint8_t *out, int64_t out_cap);
void pcabi_moves_counts(int reset, int64_t *remapped, int64_t *dropped);
void pcabi_moves_last_times(int reset, double *ms, int64_t *bytes);
int pcabi_reads_write_bam_tags(const pcabi_reads *b, const char *path, int append, const int32_t *start_trim,
                               const int32_t *end_trim, const int64_t *cut_off, const int64_t *cuts,
                               int min_split_read_size, int discard_middle, int untrimmed, const uint8_t *select,
                               const char *header_text, int64_t header_len, int keep_aux, int tag_flags, int device);

/* ---- SAM tags in FASTQ / FASTA headers (csrc/pcabi_auxtext.h, csrc/pcabi_auxtext.hip) ----------
 * The text writers can carry a part's aux tags in its header, as `samtools fastq -T` writes them and
 * `minimap2 -y` reads them: tab-separated TG:T:value fields behind the name. The tags are the aux bytes
 * pcabi_reads_write_bam_tags would put into the same part's record (same keep_aux, same tag_flags), so
 * a trimmed read or a split piece carries MM ML MN mv ts remapped exactly as in BAM output.
 * SAM text of an aux chain: per tag a tab, the two name bytes, ':', then by type
 *   A            A: and the byte
 *   c C s S i I  i: and the decimal value
 *   f            f: and C's printf("%g") of the float32 widened to double
 *   Z, H         Z: / H: and the bytes up to the NUL
 *   B            B:, the subtype letter as stored, then ',' and the value per element (an empty array
 *                is TG:B:c with nothing behind it)
 * A chain without tags adds nothing, not even a tab. A tag is left out (and counted) when its name is
 * not [A-Za-z][A-Za-z0-9] or its A / Z / H value holds a byte outside 0x20..0x7E. A chain that does not
 * walk -- an unknown type or subtype, a Z / H without its NUL inside the chain, a value or an array
 * that runs past the end -- has no text: its length is -1 and nothing is written for it.
 *   pcabi_auxtext_part : one chain aux[aux_off, aux_off + aux_len); len = its text's length (leading
 *       tabs included), out = where the text goes.
 *   pcabi_auxtext_plan  : fills parts[].len (-1: the chain does not walk) and adds the tags to the
 *       counters. device >= 0: the blob and the table go up with a table of the floats' texts (the host
 *       prints them, 16 bytes a float), k_auxtext_size walks one chain per wave and 16 bytes a part come
 *       back; device < 0: the host build of the same code (no GPU needed). A part outside the blob is
 *       refused (PCABI_E_ARG).
 *   pcabi_auxtext_write : writes every part's text to out[part.out, part.out + part.len). A len that
 *       is not what the plan gives, ranges that overlap or lie outside out[0, out_cap) are refused
 *       (PCABI_E_ARG). On the device the output lies between 64 guard bytes, checked after the kernel
 *       (PCABI_E_DEVICE if it wrote outside). Bytes no part owns keep their values.
 *   pcabi_auxtext_counts : tags written as text and tags left out, as pcabi_auxtext_plan and
 *       pcabi_reads_write_tags counted them since the last call with reset != 0.
 *   pcabi_fastx_part : one output record. FASTQ: '@' name tag-text '\n' bases '\n' '+' '\n' qualities
 *       '\n'; FASTA: '>' name tag-text '\n', then the bases in lines of 70, each followed by '\n'. The
 *       name and the aux chain lie in a side blob; text_len is the chain's length from the plan (<= 0:
 *       no tag text); PCABI_FASTX_RNA writes T as U.
 *   pcabi_fastx_pack_plan : (host) fills out / tile0 for a chain of records that starts at out0 and
 *       returns its end; tiles[0] (may be NULL) = the tile count. Every part owns max(1, ceil(l_seq /
 *       16384)) tiles.
 *   pcabi_fastx_pack_dev  : device pointers on the current device, asynchronous on `stream`: the parts
 *       (a planned table) written into out[0, out_cap) by k_fastx_pack; the workgroup of a part's first
 *       tile also writes its header. ftext / fslot0 / n_slots: the floats' texts (16-byte slots: the
 *       length, then the characters) and every part's first slot, or NULL / NULL / 0 when no chain
 *       holds a float. A part that does not lie inside the buffers writes nothing.
 *   pcabi_fastx_pack_host : the same with host buffers, staged through the device; device < 0 runs the
 *       host build. Parts outside the buffers, not planned, or with a text_len that is not the plan's
 *       are refused (PCABI_E_ARG). On the device the output lies between 64 guard bytes, checked after
 *       the kernel. Bytes no part owns keep their values.
 *   pcabi_auxtext_last_times : on != 0 makes the device path of pcabi_reads_write_tags time its
 *       kernels with device events; ms[0..1] = milliseconds of k_auxtext_size and k_fastx_pack,
 *       bytes[0..1] = what they read and wrote, since the last call with reset != 0.
 *   pcabi_reads_write_tags : pcabi_reads_write_dev with keep_aux (1, 2), tag_flags
 *       (PCABI_BAM_KEEP_MOVES) and header_tags. header_tags == 0, keep_aux == 0 or a batch without aux
 *       bytes: exactly pcabi_reads_write_dev. Else every record's header is the name as the text writers
 *       write it (for a batch whose tags were parsed from its headers, pcabi_fastx_header_tags: up to
 *       its first tab) followed by the SAM text above of the part's aux bytes. gz = 0 / 1: the host build
 *       builds the text. gz = 2 / 3: on device gzip_device (-1: the current device) the remapped tags
 *       are sized and written into the device copy of the side blob as for BAM output, k_auxtext_size
 *       gives every part's text length, the host plans the records' offsets and the line-aligned
 *       deflate blocks (pcabi_gzip_plan_lines' rules) from the line lengths alone, k_fastx_pack lays the
 *       text out in device memory and the gzip / BGZF encoder compresses it there; only compressed
 *       bytes come back. Both paths decompress to the same bytes.
 * Out of scope: the sp / pi tags of split reads; direct-RNA move tables; escaping the tags that are
 * left out.
 */
#define PCABI_FASTX_RNA 1 /* pcabi_fastx_part flags: T is written as U */
typedef struct pcabi_auxtext_part {
    int64_t aux_off; /* the chain in the aux blob                        */
    int64_t out;     /* where its text goes                              */
    int64_t len;     /* the text's length (pcabi_auxtext_plan), -1: none */
    int32_t aux_len;
    int32_t reserved;
} pcabi_auxtext_part;
typedef struct pcabi_fastx_part {
    int64_t seq_src;  /* base 0 in the sequence buffer                         */
    int64_t qual_src; /* quality 0 in the quality buffer (FASTQ)               */
    int64_t name_off; /* the name (name_len bytes) in the side blob            */
    int64_t aux_off;  /* the aux chain (aux_len bytes) in the side blob        */
    int64_t text_len; /* the chain's text length (pcabi_auxtext_plan); <= 0: none */
    int64_t out;      /* the record's first byte in the output                 */
    int64_t tile0;    /* tiles of the parts before this one                    */
    int32_t l_seq, l_qual, name_len, aux_len;
    int32_t flags;    /* PCABI_FASTX_RNA                                       */
    int32_t reserved;
} pcabi_fastx_part;
int pcabi_auxtext_plan(int device, const uint8_t *aux, int64_t aux_n, pcabi_auxtext_part *parts, int64_t n_parts);
int pcabi_auxtext_write(int device, const uint8_t *aux, int64_t aux_n, const pcabi_auxtext_part *parts, int64_t n_parts,
                        uint8_t *out, int64_t out_cap);
void pcabi_auxtext_counts(int reset, int64_t *tags_written, int64_t *tags_left_out);
void pcabi_auxtext_last_times(int on, int reset, double *ms, int64_t *bytes);
int64_t pcabi_fastx_pack_plan(pcabi_fastx_part *parts, int64_t n_parts, int fasta, int64_t out0, int64_t *tiles);
int pcabi_fastx_pack_dev(void *stream, const uint8_t *seq, int64_t seq_n, const uint8_t *qual, int64_t qual_n,
                         const uint8_t *side, int64_t side_n, const pcabi_fastx_part *parts, int64_t n_parts,
                         int64_t n_tiles, int fasta, const uint8_t *ftext, const int64_t *fslot0, int64_t n_slots,
                         uint8_t *out, int64_t out_cap);
int pcabi_fastx_pack_host(int device, const uint8_t *seq, int64_t seq_n, const uint8_t *qual, int64_t qual_n,
                          const uint8_t *side, int64_t side_n, const pcabi_fastx_part *parts, int64_t n_parts, int fasta,
                          uint8_t *out, int64_t out_cap);
int pcabi_reads_write_tags(const pcabi_reads *b, const char *path, int append, int gz, int fasta,
                           const int32_t *start_trim, const int32_t *end_trim, const int64_t *cut_off,
                           const int64_t *cuts, int min_split_read_size, int discard_middle, int untrimmed,
                           const uint8_t *select, int gzip_device, int keep_aux, int tag_flags, int header_tags);

/* ---- SAM tags read from FASTQ / FASTA headers (csrc/pcabi_auxparse.h, csrc/pcabi_auxparse.hip) ----
 * The other direction: a FASTQ / FASTA file whose headers carry tags as `dorado --emit-fastq`,
 * `samtools fastq -T` and pcabi_reads_write_tags write them. A reader with pcabi_fastx_header_tags parses
 * every header into a chain of BAM aux bytes and puts it where a BAM reader puts a record's
 * (pcabi_reads_aux, as_stored = 1 for every read), so the writers remap MM ML MN mv ts onto trimmed
 * reads and split pieces exactly as for BAM input.
 * The rule. The header is the text after '@' / '>', without the line end. It is split at tabs only.
 * Field 0 is the name and any blank-separated comment; it holds no tags. Every later field is a
 * candidate: a well-formed one appends one tag to the chain, in header order (duplicate names are
 * kept); any other -- an empty field between two tabs or after a trailing tab included -- is left out
 * and counted. A header without a tab gives an empty chain and counts nothing. A candidate is TG:T:V
 * with TG matching [A-Za-z][A-Za-z0-9], and by type T:
 *   A   V exactly one byte 0x20..0x7E                          -> TG A byte
 *   i   V [-+]?[0-9]{1,10} with a value in -2^31 .. 2^32 - 1   -> htslib's smallest type: a leading '-'
 *       selects signed (c >= -128, s >= -32768, else i), otherwise C <= 255, S <= 65535, else I; "-0"
 *       is c 0
 *   f   V SAM's float syntax [-+]?[0-9]*\.?[0-9]+([eE][-+]?[0-9]+)? or [-+]?inf or [-+]?nan, at most
 *       31 bytes                                               -> TG f and the float32 of C's (float)strtod(V)
 *   Z   V any bytes 0x20..0x7E, may be empty                   -> TG Z V NUL
 *   H   V an even number of hex digits, either case            -> TG H V NUL
 *   B   V a subtype letter of cCsSiIf, then zero or more ",element"; an integer element is
 *       [-+]?[0-9]{1,10} inside the subtype's range, a float element as f
 *                                                              -> TG B subtype, the count as u32 LE, the elements LE
 * One bad element leaves the whole field out. Nothing is escaped or repaired.
 * Floats are the host's, as in the writer: the device checks a float's syntax (the field's length
 * depends on it) and leaves a fix-up -- where the text lies, how long it is, where the 4 bytes go; the
 * host fills the fix-ups with strtod once the chains are back and never scans the text itself.
 *   pcabi_auxparse_part : one header text[text_off, text_off + text_len); len = its chain's length, out =
 *       where the chain goes, n_float = the f values and B:f elements in it, tags / left_out = the fields
 *       read and left out.
 *   pcabi_auxparse_plan  : fills parts[].len, n_float, tags and left_out and adds the last two to the
 *       counters. device >= 0: the text and the table go up and k_auxparse_size walks one header per
 *       wave; device < 0: the host build of the same rule (no GPU needed). A part outside the text is
 *       refused (PCABI_E_ARG).
 *   pcabi_auxparse_write : writes every part's chain to out[part.out, part.out + part.len). A len (or
 *       a count) that is not what the plan gives, ranges that overlap or lie outside out[0, out_cap) are refused
 *       (PCABI_E_ARG). device >= 0: k_auxparse_write stores the chains and the floats' fix-up records (a
 *       part's first slot is the host's prefix sum over n_float); the output lies between 64 guard
 *       bytes, checked after the kernel (PCABI_E_DEVICE if it wrote outside). Bytes no part owns keep
 *       their values.
 *   pcabi_auxparse_counts : tags read and fields left out, as pcabi_auxparse_plan and a reader with
 *       pcabi_fastx_header_tags counted them since the last call with reset != 0.
 *   pcabi_auxparse_last_times : on != 0 makes the device paths time their kernels with device events;
 *       ms[0..1] = milliseconds of k_auxparse_size and k_auxparse_write, bytes[0..1] = what they read and
 *       wrote, since the last call with reset != 0.
 *   pcabi_fastx_header_tags : before the first pcabi_fastx_next, on != 0 makes a FASTA / FASTQ reader
 *       fill every batch's aux bytes from its headers. device >= 0: the batch's header blob goes up once,
 *       both kernels run on a stream of the reader's, and the chains and the fix-ups come back; device
 *       < 0: the host build on the io threads. A BAM reader: no effect. A raw reader: PCABI_E_ARG. The
 *       batch remembers that its tags came from its headers: pcabi_reads_write_tags then takes as a
 *       record's name the header up to its first tab (the `_k` of a split piece in front of it, where it
 *       goes today), so the tags that were parsed are not written a second time in front of the new
 *       ones. Every other writer and every other batch is unchanged; the BAM writer's name ends at the
 *       first blank or tab anyway.
 * Out of scope: sharded runs (shards.py) and text_chunks; tags separated by blanks instead of tabs;
 * carrying a left-out field or the free-text comment into BAM (CO); the sp / pi tags of split reads;
 * direct-RNA move tables; keeping the chains on the device for the writer.
 */
typedef struct pcabi_auxparse_part {
    int64_t text_off; /* the header in the text blob                      */
    int64_t out;      /* where its chain goes                             */
    int64_t len;      /* the chain's length (pcabi_auxparse_plan)         */
    int64_t text_len; /* below 2^31                                       */
    int32_t n_float;  /* f values and B:f elements of the chain (plan)    */
    int32_t tags;     /* fields read (plan)                               */
    int32_t left_out; /* fields left out (plan)                           */
    int32_t reserved;
} pcabi_auxparse_part;
int pcabi_auxparse_plan(int device, const uint8_t *text, int64_t text_n, pcabi_auxparse_part *parts, int64_t n_parts);
int pcabi_auxparse_write(int device, const uint8_t *text, int64_t text_n, const pcabi_auxparse_part *parts, int64_t n_parts,
                         uint8_t *out, int64_t out_cap);
void pcabi_auxparse_counts(int reset, int64_t *tags_read, int64_t *fields_left_out);
void pcabi_auxparse_last_times(int on, int reset, double *ms, int64_t *bytes);
int pcabi_fastx_header_tags(pcabi_fastx *r, int on, int device);

/* ---- quality stage: end crop and read filter (csrc/pcabi_qual.h, csrc/pcabi_qual.hip) -----------
 * What the quality filter that follows an adapter trimmer does, on the spans the end trim left: each
 * span is cropped at both ends to its outermost windows of acceptable quality, then the read passes or
 * fails length and mean-quality limits. The caller turns front / tail into trims and the pass bits into
 * its keep mask (pipeline.FileTrimmer), so every writer remaps MM ML MN mv ts for the cropped read as
 * it does for a trimmed one.
 * Qualities. A quality byte c is Phred q = clamp(c - 33, 0, 93): bytes below 33 give 0, above 126 give
 * 93. A read whose quality length differs from its sequence length (FASTA, a BAM record without
 * qualities, a '+'-padded record) is without qualities: the caller passes span_off < 0; it is never
 * cropped and passes the quality test, its length tests apply.
 * The span of read i is the n = span_len[i] bytes qual[span_off[i], span_off[i] + n).
 * The crop. window W (1..64; 0: no crop) and min_window_sum: with S(p) the sum of q over [p, p + W), f
 * the least and g the greatest p in [0, n - W] with S(p) >= min_window_sum, the kept span is
 * [f, g + W): front = f, tail = n - (g + W), kept = g + W - f. No such window, or n < W: front = n,
 * tail = 0, kept = 0.
 * Trims handed on, for a span [a, a + n) of a read of ns bases (a, n from the writers' slice of the
 * adapter trims, pcabi_reads_write): only when front + tail > 0, start_trim' = a + front and
 * end_trim' = ns - (a + n - tail); these are in range, so the writers' slice gives exactly the kept
 * span. Otherwise both trims stay as they are.
 * Sums over the kept span: q_sum = the sum of q; err_sum = the sum of E[q], E[q] = round(2^32 *
 * 10^(-q / 10)) for q = 0..93, 94 constants (pcabi_qual_error_table). A batch holds at most 2^31 bytes,
 * so err_sum stays below 2^63.
 * Flags: PCABI_QUAL_TOO_SHORT kept < min_length; PCABI_QUAL_TOO_LONG max_length > 0 and kept >
 * max_length; PCABI_QUAL_LOW_QUALITY the read has qualities and err_sum > kept * max_mean_err
 * (max_mean_err in [0, 2^32]; 2^32 switches the test off: the mean of the error probabilities, as ONT
 * tools and dorado's qs tag take it); PCABI_QUAL_NO_QUALITIES informational. A read passes when none of
 * the first three is set. Equality passes: a window sum equal to min_window_sum qualifies, err_sum
 * equal to kept * max_mean_err is not LOW_QUALITY.
 *   pcabi_qual_seg_bound     : (host) the segments (4096 bytes each) the uncropped spans would take: the
 *       upper bound pcabi_qual_filter_dev's grid is sized by.
 *   pcabi_qual_scratch_bytes : the scratch pcabi_qual_filter_dev needs for n_reads and that bound.
 *   pcabi_qual_filter_dev    : device pointers on the current device, asynchronous on `stream`; nothing
 *       comes back to the host in between. k_qual_crop, one wave per read, takes 64 window starts a pass
 *       from the front (a wave prefix sum gives the 64 window sums, a ballot the first that qualifies)
 *       and stops at the first pass that holds one, then the same from the tail; a device scan of the
 *       kept spans' segment counts gives every read's first segment; k_qual_sum, one wave per segment,
 *       takes 16-byte loads masked to the segment at both ends (no byte outside a kept span is read)
 *       with E[] in LDS; k_qual_finish adds a read's segments and sets its flags. out[i] is complete
 *       when the stream has run. A span that does not lie inside the blob is treated as a read without
 *       qualities (nothing of it is read). window > 64, max_mean_err > 2^32, a blob over 2^31 bytes or a
 *       scratch buffer that is too small are refused (PCABI_E_ARG) before any launch.
 *   pcabi_qual_filter_host   : host buffers, uploaded and run as above on `device`; device < 0 runs the
 *       host build of the same header on the io threads (no GPU needed). A span outside the blob is
 *       refused as well (PCABI_E_ARG), before any launch.
 *   pcabi_qual_error_table   : E[0..93].
 *   pcabi_qual_last_times    : on != 0 makes pcabi_qual_filter_host time its kernels with device events;
 *       ms[0..3] = milliseconds of k_qual_crop, of k_qual_sum, the wall time of the host build and the
 *       wall time of the device stage behind the uploads (kernels, scan, records back); bytes[0..1] =
 *       the spans' bytes the two kernels were given; all since the last call with reset != 0.
 * The piece stage (csrc/pcabi_pieces.h; pcabi_qual_pieces_*): the stage above sees a chimeric read as one
 * span, middle adapters included, while the writers cut it into pieces. This stage judges the pieces.
 * The pieces of read r, from its trimmed length tl = span_len[r] and its ranges [cuts[2k], cuts[2k + 1])
 * for k in [cut_off[r], cut_off[r + 1]) (positions of the trimmed sequence, in any order; they may
 * overlap, nest, repeat, be empty, begin below 0 or end beyond tl): the read is split when at least one
 * of its ranges is non-empty (end > begin), even if that range lies wholly outside [0, tl) -- the single
 * piece is then [0, tl); the pieces are the maximal runs of positions of [0, tl) that no non-empty range
 * covers, ascending; runs of length 0 do not exist; a read that is not split has no pieces (the stage
 * above has dealt with it). This is the writers' rule (pcabi_reads_write), restated.
 * Each piece (read, begin, end) is a span of its own, span_off[r] + begin of length end - begin (span_off[r]
 * < 0 stays < 0: no qualities), cropped, summed and tested by the same kernels with the same options:
 * one pcabi_qual_read per piece. The result goes to the writers as a new cut layout, cut_off'[r] =
 * cut_off[r] + 2 * piece_off[r]: read r's ranges as they came, in their order, then two ranges a piece:
 * [begin, begin + front) and [end - tail, end) for a piece that passes, [begin, end) and the empty [end,
 * end) for one that fails (TOO_SHORT, TOO_LONG or LOW_QUALITY after its crop). Reads that are not split
 * keep their ranges and get none added. The writers ignore empty ranges, so with (cut_off', cuts') every
 * writer emits exactly the cropped, passing pieces, numbered _1, _2, ... over the pieces written, its
 * min_split_read_size applied to the cropped piece, the MM ML MN mv ts remap following the same cuts.
 *   pcabi_qual_pieces_bound         : (host) upper bounds nothing is read back for: pieces <= ranges + reads
 *       with ranges; segments <= the sum of n_segs(span_len) over the reads with ranges + that piece bound.
 *   pcabi_qual_pieces_scratch_bytes : the scratch pcabi_qual_pieces_dev needs.
 *   pcabi_qual_pieces_dev           : device pointers on the current device, asynchronous on `stream`, no
 *       host round trip: k_piece_keys and a 64-bit radix sort order the ranges by (read, begin), so a read
 *       may have any number of them; k_piece_count, one thread per read, walks them; a device scan gives
 *       piece_off[n_reads + 1]; k_piece_spans writes the pieces and their spans (the slots up to piece_cap
 *       become empty spans); k_qual_crop, the segment scan, k_qual_sum and k_qual_finish run over them;
 *       k_piece_cuts writes cut_off_out[n_reads + 1], cuts_out (cuts_cap ranges, at least n_ranges + 2 *
 *       piece_cap) and the pieces' records. pieces[0, piece_off[n_reads]) are valid. piece_cap and seg_cap
 *       must be the values pcabi_qual_pieces_bound gives for this cut_off (ranges + reads with ranges): the
 *       call sees device pointers and cannot count the reads with ranges, so it can refuse only a
 *       piece_cap below n_ranges + 1; with a cap between that and the bound the kernels write nothing out
 *       of bounds but drop the pieces beyond it, and pieces and cuts_out are undefined (piece_off[n_reads]
 *       > piece_cap tells; pcabi_qual_pieces_host computes the bound itself). Bad options, a blob over
 *       2^31 bytes, such a piece_cap, a cuts_cap or a scratch buffer that is too small are refused
 *       (PCABI_E_ARG) before any launch.
 *   pcabi_qual_pieces_host          : host buffers, uploaded and run as above on `device`; device < 0 runs
 *       the host build of the same headers (no GPU needed): the enumeration, a sort per read and the cut
 *       layout on the calling thread, the crop and sums of the piece spans on the io threads. piece_cap / cuts_cap: the room of pieces /
 *       cuts_out, at least the bound / n_ranges + 2 * piece_cap. cut_off that does not begin at 0 or
 *       descends, and spans outside the blob, are refused as well.
 *   pcabi_qual_pieces_last_times    : as pcabi_qual_last_times, for pcabi_qual_pieces_host: ms[0..5] = the
 *       plan kernels (keys, sort, count, scan, spans), k_qual_crop over the piece spans, k_qual_sum over
 *       them, k_piece_cuts, the wall time of the host build, the wall time of the device stage behind the
 *       uploads; bytes[0..3] = what the first four were given.
 * Out of scope: rewriting dorado's qs tag for a cropped read or piece; sp / pi tags on pieces; running
 * the middle scan again on cropped pieces; fastp's base-by-base trim inside the first good window;
 * windows over 64; sharded runs; qualities kept on the device by the BAM or gunzip readers.
 */
#define PCABI_QUAL_TOO_SHORT 1
#define PCABI_QUAL_TOO_LONG 2
#define PCABI_QUAL_LOW_QUALITY 4
#define PCABI_QUAL_NO_QUALITIES 8
typedef struct pcabi_qual_opts {
    int32_t window; /* W: 1..64, 0 = no crop */
    int32_t reserved;
    int64_t min_window_sum;
    int64_t min_length;
    int64_t max_length;    /* 0 = no limit */
    uint64_t max_mean_err; /* units of 2^-32; 2^32 = no test */
} pcabi_qual_opts;
typedef struct pcabi_qual_read {
    int32_t front, tail; /* bytes cropped from the span's two ends */
    int32_t kept;
    int32_t flags;       /* PCABI_QUAL_* */
    int64_t q_sum;
    uint64_t err_sum;
} pcabi_qual_read;
int64_t pcabi_qual_seg_bound(const int32_t *span_len, int64_t n_reads);
int64_t pcabi_qual_scratch_bytes(int64_t n_reads, int64_t n_segs);
int pcabi_qual_filter_dev(const uint8_t *qual, int64_t qual_n, const int64_t *span_off, const int32_t *span_len,
                          int64_t n_reads, int64_t n_segs, const pcabi_qual_opts *opts, pcabi_qual_read *out,
                          void *scratch, int64_t scratch_len, void *stream);
int pcabi_qual_filter_host(int device, const uint8_t *qual, int64_t qual_n, const int64_t *span_off,
                           const int32_t *span_len, int64_t n_reads, const pcabi_qual_opts *opts,
                           pcabi_qual_read *out);
void pcabi_qual_error_table(uint64_t *table);
void pcabi_qual_last_times(int on, int reset, double *ms, int64_t *bytes);
typedef struct pcabi_qual_piece {
    int64_t read;       /* the read the piece is of */
    int64_t begin, end; /* positions of the trimmed sequence */
    pcabi_qual_read q;  /* over qual[span_off[read] + begin, span_off[read] + end) */
} pcabi_qual_piece;
int pcabi_qual_pieces_bound(const int32_t *span_len, const int64_t *cut_off, int64_t n_reads, int64_t *n_pieces,
                            int64_t *n_segs);
int64_t pcabi_qual_pieces_scratch_bytes(int64_t n_reads, int64_t n_ranges, int64_t piece_cap, int64_t seg_cap);
int pcabi_qual_pieces_dev(const uint8_t *qual, int64_t qual_n, const int64_t *span_off, const int32_t *span_len,
                          int64_t n_reads, const int64_t *cut_off, const int64_t *cuts, int64_t n_ranges,
                          int64_t piece_cap, int64_t seg_cap, const pcabi_qual_opts *opts, int64_t *piece_off,
                          pcabi_qual_piece *pieces, int64_t *cut_off_out, int64_t *cuts_out, int64_t cuts_cap,
                          void *scratch, int64_t scratch_len, void *stream);
int pcabi_qual_pieces_host(int device, const uint8_t *qual, int64_t qual_n, const int64_t *span_off,
                           const int32_t *span_len, int64_t n_reads, const int64_t *cut_off, const int64_t *cuts,
                           const pcabi_qual_opts *opts, int64_t *piece_off, pcabi_qual_piece *pieces,
                           int64_t piece_cap, int64_t *cut_off_out, int64_t *cuts_out, int64_t cuts_cap);
void pcabi_qual_pieces_last_times(int on, int reset, double *ms, int64_t *bytes);

#ifdef __cplusplus
}
#endif
#endif /* PCABI_H */
