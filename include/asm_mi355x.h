/* asm_mi355x.h — C ABI of the MI355X-native batched pair aligner (libasm_mi355x.so).
 *
 * Drop-in boundary for ONE path of GZHoffie/approximate-string-matching: the per-pair work of its benchmark
 * harness, `benchmark::_run_benchmark` (GASMA/benchmark/benchmark_utils.h:231-259), i.e.
 *   NW     `_run_nw_sse`  benchmark_utils.h:130-150  (parasail_nw_trace_striped_sse41_128_16; penalty = -score)
 *   LEAP   `_run_LEAP`    benchmark_utils.h:156-179  (LV::load_reads/reset/run/get_ED, LEAP_SIMD/LV_BAG.cpp:110-245,356)
 *   Greedy `_run_greedy`  benchmark_utils.h:185-201  (hurdle_matrix<int_128bit>::reset/run/get_cost, hurdle_matrix.h:568,625,677)
 * plus the accuracy counters of benchmark_utils.h:249-255, the coverage metric (:214-225,256), the input definition of
 * benchmark_dataset.h, the mapper's per-hit call shape (GASMA/mapper/main.cpp:77-96) and the filtering stage in front of the
 * aligners (bit-parallel LEAP `SIMD_ED` and SHD, GASMA/benchmark/LEAP_SIMD/main.cpp:95-101,186-195).
 * The reference runs these one pair at a time on one CPU thread; this library runs a whole batch of pairs
 * per call on one GPU.  Plain pointers and sizes only; no C++/torch types cross this boundary.
 *
 * Batch layout: `reads`/`refs` = concatenated ASCII (no terminators); `read_off`/`ref_off` = n+1 prefix
 * offsets (uint32); pair i = reads[read_off[i] .. read_off[i+1]) vs refs[ref_off[i] .. ref_off[i+1]).
 *
 * Threading: one handle per GPU; calls on one handle must be serialised by the caller.  Calls are
 * synchronous at return unless the name ends in `_async` (those only enqueue on the handle's stream).
 * Every function returns 0 on success or a negative ASM_E* code; asm_last_error() gives the message.
 * There is NO CPU fallback: without a usable HIP device every compute entry point fails with ASM_ENODEVICE.
 */
#ifndef ASM_MI355X_H
#define ASM_MI355X_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ASM_OK 0
#define ASM_EINVAL (-1)    /* bad argument (k out of range, o < e for LEAP, NULL pointer, ...)            */
#define ASM_ENODEVICE (-2) /* no HIP device / device call failed                                          */
#define ASM_ENOMEM (-3)
#define ASM_EUNSUPPORTED (-4) /* e.g. sequence longer than the kernels' compiled limit                    */

/* aligner ids — the three aligners `_run_benchmark` runs per pair */
#define ASM_NW 0
#define ASM_LEAP 1
#define ASM_GREEDY 2

/* Greedy buffer-tail mode (hurdle_matrix.h:136-137,625-631 + bit_convert.cpp:265-330) */
#define ASM_GREEDY_SEQUENTIAL 0 /* reference as run: stale bytes of earlier pairs flow into later ones   */
#define ASM_GREEDY_CLEAN 1      /* tail bytes are NUL for every pair (order independent)                  */

/* reference limits reproduced here */
#define ASM_GREEDY_MAX_LENGTH 128 /* GASMA/utils.h:23-25 — Greedy aligns the first 128 bases            */
#define ASM_GREEDY_MAX_K 50       /* GASMA/hurdle_matrix.h:8                                             */
#define ASM_LEAP_MAX_LENGTH 256   /* LEAP_SIMD/LV_BAG.h:17-18; longer pairs are undefined in the reference */
#define ASM_LEAP_AF_THRESHOLD 200 /* benchmark_utils.h:289                                               */
#define ASM_MAX_LENGTH 512        /* longest sequence any kernel here accepts                            */

typedef struct asm_handle asm_handle; /* one per GPU: device id, stream, scratch                          */
typedef struct asm_batch asm_batch;   /* a device-resident batch of read pairs (ASCII + packed bit planes) */

/* Scoring and aligner parameters — the constructor arguments of `benchmark` (benchmark_utils.h:263-289)
 * and of hurdle_matrix (hurdle_matrix.h:552-559). */
typedef struct asm_params {
    int32_t k;           /* band half-width (lanes -k..k)                                                 */
    int32_t x, o, e;     /* mismatch, gap-open (first gap base), gap-extend penalties.  NW: all >= 0, and small enough for
                            the batch: 2*(o + (maxlen-1)*e) + o < 30000 (else ASM_EUNSUPPORTED).  LEAP: x >= 1,
                            15 >= o >= e >= 1 (LV_BAG.cpp:165-166).  Greedy: >= 0                                       */
    double p_match;      /* Greedy significance model; defaults 0.80, 0.20/3, 0.40/3                      */
    double p_mismatch;
    double p_indel;
    int32_t alignment_type; /* Greedy: ASM_ALIGN_GLOBAL (default, what the harness uses) or ASM_ALIGN_SEMI_GLOBAL —
                               hurdle_matrix's alignment_type_t (hurdle_matrix.h:477,553; utils.h:554-558); LOCAL is
                               declared but unsupported in the reference (hurdle_matrix.h:467).  NW and LEAP ignore it. */
    int32_t leap_mode;      /* LEAP: LV::init's ED_modes (LEAP_SIMD/LV_BAG.h:38,65) — ASM_LEAP_GLOBAL (default; what the harness
                               passes, benchmark_utils.h:289), ASM_LEAP_LOCAL, ASM_LEAP_SEMI_FREE_BEGIN, ASM_LEAP_SEMI_FREE_END:
                               LOCAL and SEMI_FREE_BEGIN start every lane at generation 0 (LV_BAG.cpp:102-104), LOCAL and
                               SEMI_FREE_END accept any lane that reaches the end (:220-238).  NW and Greedy ignore it.  (This
                               field was `reserved_`, always 0 = GLOBAL.) */
} asm_params;
#define ASM_ALIGN_GLOBAL 0
#define ASM_ALIGN_SEMI_GLOBAL 1
#define ASM_LEAP_GLOBAL 0
#define ASM_LEAP_LOCAL 1
#define ASM_LEAP_SEMI_FREE_BEGIN 2
#define ASM_LEAP_SEMI_FREE_END 3

/* ---- library / handle ------------------------------------------------------------------------------ */
const char* asm_version(void);
void asm_default_params(asm_params* p);          /* x=o=e=1, k=3, default probabilities (benchmark.cpp:22) */
int asm_device_count(void);                       /* number of HIP devices (0 without a GPU; never fails)   */
int asm_create(asm_handle** out, int device);     /* binds the handle to HIP device `device`               */
int asm_destroy(asm_handle* h);
const char* asm_last_error(const asm_handle* h);  /* h may be NULL: last error of the calling thread       */
/* Launch everything on a caller-owned hipStream_t (e.g. torch's current stream).  NULL is HIP's legacy default stream —
 * which is what torch hands out outside a `torch.cuda.stream(...)` context — NOT "no stream": the handle's own stream is
 * non-blocking and never synchronises with the legacy one, so a caller that mixes its own work (a collective, a torch op
 * on d_penalties) with this library's must put both on one stream through this call.  asm_reset_stream goes back to the
 * handle's own stream. */
int asm_set_stream(asm_handle* h, void* hip_stream);
int asm_reset_stream(asm_handle* h);
int asm_synchronize(asm_handle* h);

/* ---- input definition: seeded restatement of `Dataset` (benchmark_dataset.h:61-253) ---- */
#define ASM_GEN_EXACT_ERRORS 0 /* exactly ceil(L*err) edit operations per pair (Dataset exact=true)        */
#define ASM_GEN_PER_BASE 1     /* independent per-base substitution / insertion / deletion (SRR611076-shaped) */
#define ASM_GEN_UP_TO_ERRORS 2 /* Dataset exact=false, the "lt_eq" files (benchmark_dataset.h:153-156,246-250): the number of
                                  edit operations is uniform in 0 .. ceil(L*err) - 1; everything else as ASM_GEN_EXACT_ERRORS */
typedef struct asm_gen_config {
    uint64_t seed;
    int32_t kind;
    int32_t len_lo, len_hi; /* read length uniform in [len_lo, len_hi]                                     */
    float err;              /* ASM_GEN_EXACT_ERRORS: error rate                                           */
    float mismatch_rate;    /* ASM_GEN_EXACT_ERRORS: P(edit is a substitution); Dataset uses 0.96         */
    float p_sub, p_ins, p_del; /* ASM_GEN_PER_BASE rates per base                                         */
} asm_gen_config;
/* Host generator.  Pairs [first, first+n) of the seeded stream (every pair has its own counter-based RNG
 * state, so any slice can be generated independently — this is how shards get their part).
 * With reads == NULL only the offsets are produced (sizing pass). */
int asm_generate_pairs(const asm_gen_config* cfg, int64_t first, int64_t n, uint32_t* read_off,
                       uint32_t* ref_off, char* reads, size_t reads_cap, char* refs, size_t refs_cap);

/* ---- device-resident batches ------------------------------------------------------------------------- */
/* Copies the ASCII batch to the GPU and packs it (pack kernel: ASCII -> 2 bit planes per string, the
 * device counterpart of sse3_convert2bit1, bit_convert.cpp:248-369).  greedy_mode selects what the bit
 * planes hold beyond each string's end (the bytes Greedy's conversion would see). */
int asm_batch_upload(asm_handle* h, int64_t n, const char* reads, const uint32_t* read_off,
                     const char* refs, const uint32_t* ref_off, int greedy_mode, asm_batch** out);
/* Generates pairs [first, first+n) of the seeded stream directly in HBM (device generator; bit-identical
 * to asm_generate_pairs) and packs them: no PCIe traffic. */
int asm_batch_generate(asm_handle* h, const asm_gen_config* cfg, int64_t first, int64_t n, int greedy_mode,
                       asm_batch** out);
/* Seed-hit batches — the shape in which the reference's read mapper calls the Greedy aligner (GASMA/mapper/main.cpp:
 * 67-96): the reference text is uploaded once and stays in HBM; for hit i of read i at 0-based reference position
 * hit_pos[i] the pair is (read i, reference[start, start + len_i + 1)) with start = hit_pos ? hit_pos - 1 : 0, clipped at
 * the reference's end (mapper/main.cpp:79-80).  Windows are gathered on the device.  MAPQ = 60 + Greedy cost (:95). */
typedef struct asm_reference asm_reference;
int asm_reference_upload(asm_handle* h, const char* text, size_t len, asm_reference** out);
int asm_reference_free(asm_handle* h, asm_reference* r);
int asm_batch_from_hits(asm_handle* h, const asm_reference* ref, int64_t n, const char* reads, const uint32_t* read_off,
                        const uint64_t* hit_pos, int greedy_mode, asm_batch** out);
/* Greedy's sequential mode ACROSS batches — shards of one file on several GPUs, or chunks of a streamed file.  The
 * reference's two 128-byte buffers (hurdle_matrix.h:136-137) live on from pair to pair: reset() overwrites their first m / n
 * bytes (:630-631) and every conversion permutes them in place (bit_convert.cpp:265-330), so what pair t sees beyond its
 * strings depends on every earlier pair of the file.  Only the 2-bit codes matter, so the chain's state is 256 codes,
 * state[side*128 + slot], side 0 = read buffer, 1 = reference buffer; a file starts from zeros (NUL bytes).
 *   asm_batch_tail_summary  — what one batch does to the buffers: summary[side*128 + s] = code of the last character the
 *                             batch writes on the trajectory that sits in slot s before its first pair, 0xFF = untouched.
 *                             Works on a batch of either mode; needs no carry-in, so all shards compute it in parallel.
 *   asm_tail_state_advance  — host only, no device: state after a batch of n_pairs = its summary applied to the state
 *                             before it (the permutation has order 10: n_pairs mod 10 decides where trajectories end).
 *   asm_batch_resolve_tails — (re)derives the batch's tails from the given state before its first pair (NULL = zeros),
 *                             switches the batch to ASM_GREEDY_SEQUENTIAL and repacks it.  Enqueue only (the state is
 *                             copied at the call).
 * Shard r of a file: summaries of all shards are exchanged (one all-gather of 256 bytes + the shard sizes), every rank folds
 * the summaries of the shards before its own with asm_tail_state_advance and resolves — the N-GPU result then equals the
 * reference run over the whole file. */
int asm_batch_tail_summary(asm_handle* h, const asm_batch* b, uint8_t* summary /* [256] */);
int asm_tail_state_advance(uint8_t* state /* [256], in/out */, const uint8_t* summary /* [256] */, int64_t n_pairs);
int asm_batch_resolve_tails(asm_handle* h, asm_batch* b, const uint8_t* state /* [256] or NULL */);
int asm_batch_free(asm_handle* h, asm_batch* b); /* the device blocks go back to the pool of the handle that MADE the batch,
                                                    whichever live handle (or NULL) is named here; once that handle has been
                                                    destroyed its device memory went with it and only the record is freed */
int64_t asm_batch_size(const asm_batch* b);
int asm_batch_max_length(const asm_batch* b);
/* bytes of resident ASCII (reads + references) */
int64_t asm_batch_text_bytes(const asm_batch* b);
/* Copies the batch's ASCII form back to the host (buffers sized by the caller from the offsets). */
int asm_batch_download(asm_handle* h, const asm_batch* b, uint32_t* read_off, uint32_t* ref_off,
                       char* reads, size_t reads_cap, char* refs, size_t refs_cap);
/* uint4 entries of the batch's packed planes: all buckets back to back, bucket b a uint4[4][w4][size] block */
int64_t asm_batch_planes_size(const asm_batch* b);
/* Copies the packed form back to the host (synchronizes the handle's stream): planes = 4 * asm_batch_planes_size() uint32
   (planes_cap, in uint32), lens = n words in bucketed order, order = n pair indices in bucketed order (the identity when the
   batch is one bucket).  Any pointer may be NULL. */
int asm_batch_download_planes(asm_handle* h, const asm_batch* b, uint32_t* planes, size_t planes_cap, uint32_t* lens,
                              uint32_t* order);
/* Re-runs only the pack kernel on the batch's resident ASCII (enqueue only). */
int asm_batch_pack_async(asm_handle* h, asm_batch* b);

/* ---- the hot path -------------------------------------------------------------------------------------- */
/* One aligner over a resident batch; d_penalties = DEVICE pointer to n int32 (enqueue only).
 * Replaces, per pair: ASM_NW -> -parasail score (benchmark_utils.h:139-142); ASM_LEAP -> LV::get_ED()
 * (LV_BAG.cpp:356; -1 where no lane passes within 200); ASM_GREEDY -> hurdle_matrix::get_cost()
 * (hurdle_matrix.h:677). */
int asm_align_batch_async(asm_handle* h, const asm_batch* b, int aligner, const asm_params* p,
                          int32_t* d_penalties);
/* Same as asm_align_batch_async with an optional per-pair work estimate (device int32[n], input order; NULL = none).
 * The estimate only steers scheduling — LEAP sorts its pairs by it (inside each workgroup, or over the whole width class with
 * one radix pass for long strings and general penalties) so that the pairs a wave waits for need about the same number of
 * generations — and never changes a result.  `_run_benchmark` passes the NW penalties of the same pairs, or, where NW is
 * not run, the Greedy penalties. */
int asm_align_batch_hinted_async(asm_handle* h, const asm_batch* b, int aligner, const asm_params* p,
                                 const int32_t* d_work_hint, int32_t* d_penalties);
/* Greedy with its CIGAR (hurdle_matrix::get_CIGAR, hurdle_matrix.h:613; built by _update_CIGAR :238-251 — lane switches
 * as nI / nD, runs of matches AND mismatches as nM, and the final hop's run is the hurdle count, :589).  d_ops = device
 * uint16[n][cap], entry = count << 3 | op with op 0 'M', 1 'I', 2 'D' (3 '=' and 4 'X' appear in NW CIGARs only); d_nops = device uint8[n] = entries produced (a
 * value above cap means the row was truncated: only the first cap entries are stored).  The count is a byte and saturates at
 * 255: 255 means "255 or more", so with cap >= 255 a row that reports 255 may be truncated as well.  A row is known to be whole
 * when d_nops[i] <= cap and d_nops[i] < 255.  Enqueue only. */
int asm_greedy_cigar_batch_async(asm_handle* h, const asm_batch* b, const asm_params* p, int32_t* d_penalties,
                                 uint16_t* d_ops, int cap, uint8_t* d_nops);
/* Host helper: formats one encoded row as the reference's string ("22M1D50M1D28M").  Writes the stored entries (the first
 * min(nops, cap)) and returns ASM_EUNSUPPORTED when the row is not known to be whole: nops > cap, or nops == 255 (saturated). */
int asm_cigar_format(const uint16_t* ops, int nops, int cap, char* out, size_t out_cap);
/* The harness's coverage counter (benchmark_utils.h:214-225,256-258; benchmark_coverage.h:26-91): for every pair,
 * does LCM(read, Greedy CIGAR, threshold 1) cover LCM(read, NW CIGAR, threshold 3)?  Needs the Greedy CIGAR rows of
 * asm_greedy_cigar_batch_async.  The NW alignment is traced back on the device with this library's own documented
 * preference (in H the diagonal, then a gap in the read 'D', then a gap in the reference 'I'; inside a gap, extending it —
 * parasail's is internal and unpinned), for any penalties p->x, p->o, p->e the NW aligner accepts.  Unit penalties run a
 * banded bit-parallel pass with `window` = 32 or 64 rows first; pairs it cannot answer (distance above window/2 - 3) and
 * every pair under other penalties go through a full Gotoh matrix with stored directions, so every pair whose Greedy row is
 * whole gets an answer: d_cover[i] = 1 covers / 0 does not.  2 = not determined is produced for exactly one case: the pair's
 * Greedy row is truncated (d_greedy_nops[i] > greedy_cap, or d_greedy_nops[i] == 255, the saturated count), since a verdict from
 * the stored prefix would be a verdict about half an alignment.  d_counters[0] += covered, d_counters[1] += not determined
 * (those pairs; 0 when greedy_cap holds every row).  d_nw_ops (optional) receives the NW CIGAR rows in traceback (reverse)
 * order, entries as above, nw_cap entries per row; d_nw_nops saturates at 255 like d_nops above, and only the first nw_cap
 * entries of a longer row are stored.  Synchronous. */
int asm_coverage(asm_handle* h, const asm_batch* b, const asm_params* p, const uint16_t* d_greedy_ops, int greedy_cap,
                 const uint8_t* d_greedy_nops, int window, uint8_t* d_cover, uint16_t* d_nw_ops, int nw_cap,
                 uint8_t* d_nw_nops, unsigned long long* d_counters);
/* Convenience: host in, host out (upload + pack + align + copy back).  The reference-shaped call:
 * align(read, ref, k) for every pair of the batch. */
int asm_align_batch(asm_handle* h, int aligner, int64_t n, const char* reads, const uint32_t* read_off,
                    const char* refs, const uint32_t* ref_off, const asm_params* p, int greedy_mode,
                    int32_t* penalties);
/* ---- input side: the harness's file format (benchmark_utils.h:325-352) ---------------------------------------------------
 * Line 2i = one marker character + read i, line 2i+1 = one marker character + reference i ('>' and '<' as Dataset writes
 * them, benchmark_dataset.h:229,234; the first character of every line is skipped blindly, :337,:343).
 * asm_batch_from_text: a batch out of such a text held in host memory; the raw bytes go to the GPU as they are and are
 * parsed there (newline index, offsets, gather: csrc/asm_ingest.h). */
int asm_batch_from_text(asm_handle* h, const char* text, size_t nbytes, int greedy_mode, asm_batch** out);
/* asm_stream_seq_file: `read_string_file` + `run` for a file of any size, in chunks of about chunk_bytes (0 = 64 MiB; from 32 MiB
 * on, the first chunk is a sixteenth of that and the chunks double up to it, so that the first transfer starts early): reader
 * threads fill pinned buffers (three in rotation) and cut them at pair boundaries, the raw bytes are copied to HBM on a copy
 * stream while the chunk before is parsed, packed and aligned on the handle's stream, and results of the chunk before that are
 * handed over.  aligner_mask: bit 0 NW, 1 LEAP, 2 Greedy.  nw / leap / greedy: host arrays of out_cap entries (or NULL),
 * pair i of the file at index i.  answers (optional, host, n_answers entries): read_answer_file's integers
 * (benchmark_utils.h:358-368; INT32_MIN = "use the NW penalty").  With ASM_GREEDY_SEQUENTIAL the stale-tail chain of
 * hurdle_matrix.h:136-137 runs through the chunk boundaries, so the result equals the reference run over the whole file.
 * max_pairs > 0 stops after that many pairs (benchmark's max_test_num, benchmark_utils.h:331).  Synchronous. */
typedef struct asm_stream_stats {
    int64_t pairs, chunks, bytes;       /* pairs aligned, chunks shipped, file bytes shipped to the GPU                   */
    unsigned long long counters[4];     /* total_tests, nw_correct, LEAP_correct, greedy_correct (benchmark_utils.h:249-255) */
    double seconds;                     /* wall clock of the whole call                                                  */
    double seconds_read;                /* of which the reader threads were busy (file -> pinned memory, newline count)    */
    int32_t max_length, reserved_;
} asm_stream_stats;
int asm_stream_seq_file(asm_handle* h, const char* path, const asm_params* p, int greedy_mode, int aligner_mask,
                        int64_t chunk_bytes, int64_t max_pairs, int32_t* nw, int32_t* leap, int32_t* greedy, int64_t out_cap,
                        const int32_t* answers, int64_t n_answers, asm_stream_stats* stats);

/* ---- filtering stage in front of the aligners: bit-parallel LEAP (SIMD_ED) and SHD ------------------------------
 * Replaces, per pair of the batch, the stdin filter driver's sequence (GASMA/benchmark/LEAP_SIMD/main.cpp:95-101,
 * 186-195): SIMD_ED::init_levenshtein(ed_threshold, ED_GLOBAL, shd_enable) once, then load_reads(read, ref,
 * min(m, 256)) / calculate_masks() / reset() / run() / check_pass() / get_ED()  (SIMD_ED.h:47-70, SIMD_ED.cpp:269-352,
 * 748-753).  d_ed[i] = get_ED() (converge_ED) when check_pass() holds, -1 otherwise.
 * mode: the reference keeps its verdict state from pair to pair (a pair that never reaches the end inherits the verdict
 * of the last pair that did; an exact pair reports the previous converge_ED) — ASM_FILTER_SEQUENTIAL reproduces that in
 * batch order, starting from state = {final_ED, lane distance, converge_ED} (NULL: zeros; the reference leaves them
 * uninitialised) and writes the state after the last pair back into it, so that a file processed in chunks (BATCH_RUN,
 * main.cpp:20) chains exactly; ASM_FILTER_CLEAN judges every pair on its own (never reached: -1; exact: 0).
 * ed_threshold in [1, 32]; with shd_enable at most 16 (MAX_ERROR_AVX, LEAP_SIMD/mask.h:21).  Enqueue only in clean
 * mode; sequential mode returns after its scans have run. */
#define ASM_FILTER_SEQUENTIAL 0
#define ASM_FILTER_CLEAN 1
int asm_simd_ed_batch_async(asm_handle* h, const asm_batch* b, int ed_threshold, int shd_enable, int mode,
                            int32_t* state, int32_t* d_ed);
/* The same with init_levenshtein's ED_modes argument (SIMD_ED.h:41,49; ed_mode = ASM_LEAP_GLOBAL / LOCAL / SEMI_FREE_BEGIN /
 * SEMI_FREE_END): LOCAL and SEMI_FREE_BEGIN keep every lane live from generation 0 (SIMD_ED.cpp:246-266); LOCAL and
 * SEMI_FREE_END pass exactly when a lane reaches the end, d_ed[i] = final_ED, and neither read nor change `state`
 * (:348-351,748-753 — `mode` makes no difference there); SEMI_FREE_BEGIN follows GLOBAL's rules, carried state included. */
int asm_simd_ed_mode_batch_async(asm_handle* h, const asm_batch* b, int ed_threshold, int shd_enable, int mode, int ed_mode,
                                 int32_t* state, int32_t* d_ed);
/* SIMD_ED in affine mode (LEAP_SIMD/SIMD_ED.h:50, SIMD_ED.cpp:435-616): init_affine(gap_threshold, af_threshold, ED_GLOBAL, x,
 * o, e) then, per pair, load_reads(read, ref, min(m, 256)) / calculate_masks() / reset() / run() / check_pass() / get_ED(), in
 * CLEAN form: every pair starts from the tables init_affine leaves.  (The reference object keeps its I/D/end tables from pair to
 * pair and never clears them, so as run a verdict depends on all pairs seen before; this entry point gives the verdict of the
 * first pair after init_affine.)  d_ed[i] = get_ED() = converge_ED when the pair passes — 1000000 for a pair whose main lane
 * reaches the end at e = 0, as the reference returns it —, -1 when it does not.  gap_threshold in [1, 32], af_threshold in
 * [1, 512], 1 <= e <= o <= 15, 1 <= x <= 15; SHD off (init_affine's default).  Enqueue only. */
int asm_simd_ed_affine_batch_async(asm_handle* h, const asm_batch* b, int gap_threshold, int af_threshold, int x, int o, int e,
                                   int32_t* d_ed);
/* The same with init_affine's SHD_enable = true and SHD_threshold (LEAP_SIMD/SIMD_ED.h:50, SIMD_ED.cpp:445-446,489-492):
 * run_affine starts with bit_vec_filter_avx(hamming_masks + 1, buffer_length, SHD_threshold) — the mask-array SHD
 * (SHD.cpp:334-372) over the first 2*SHD_threshold+1 lane masks, i.e. lanes -gap .. -gap + 2*SHD_threshold (centred on the main
 * lane only when the two thresholds are equal) — and a rejected pair does not pass (d_ed[i] = -1).  shd_threshold in
 * [0, min(16, gap_threshold)]: the reference object holds 2*gap_threshold+1 masks and would read past them.  Enqueue only. */
int asm_simd_ed_affine_shd_batch_async(asm_handle* h, const asm_batch* b, int gap_threshold, int af_threshold, int x, int o, int e,
                                       int shd_threshold, int32_t* d_ed);
/* ... and with init_affine's ED_modes argument (SIMD_ED.h:41,50): mode = ASM_LEAP_GLOBAL / LOCAL / SEMI_FREE_BEGIN / SEMI_FREE_END
 * (the enum is LV's).  LOCAL and SEMI_FREE_BEGIN start every lane at generation 0 (SIMD_ED.cpp:476-478,497-516); LOCAL and
 * SEMI_FREE_END accept any lane that reaches the end and d_ed[i] is final_ED there (:589-610,748-753) — 0, not 1000000, for a
 * pair exact at generation 0.  shd_threshold < 0: SHD off.  Enqueue only. */
int asm_simd_ed_affine_mode_batch_async(asm_handle* h, const asm_batch* b, int gap_threshold, int af_threshold, int x, int o, int e,
                                        int shd_threshold, int mode, int32_t* d_ed);
/* bit_vec_filter_avx(read planes, ref planes, min(m, 256), max_error) (LEAP_SIMD/SHD.h:17-18, SHD.cpp:241-322):
 * d_pass[i] = 1 when the pair survives the shifted-Hamming-distance filter, 0 when it is rejected.  max_error in
 * [0, 16].  Enqueue only. */
int asm_shd_filter_batch_async(asm_handle* h, const asm_batch* b, int max_error, int32_t* d_pass);
/* accuracy counter of benchmark_utils.h:253-255: *d_count += #{i : a[i] == b[i]} (device pointers; enqueue
 * only; the caller zeroes *d_count). */
int asm_count_equal_async(asm_handle* h, const int32_t* d_a, const int32_t* d_b, int64_t n,
                          unsigned long long* d_count);

/* All counters of `_run_benchmark` (benchmark_utils.h:238,249-255) in one pass over device penalty arrays:
 * d_counters[0..3] += {total_tests, nw_correct, LEAP_correct, greedy_correct}; the correct answer of pair i is
 * d_answers[i] when d_answers is given and != INT32_MIN (read_answer_file, benchmark_utils.h:358-368), else the NW
 * penalty.  d_nw / d_leap / d_greedy / d_answers may be NULL; without d_nw a pair has a correct answer only where the
 * answers file gives one, and total_tests counts every pair regardless.  Enqueue only. */
int asm_accuracy_async(asm_handle* h, const int32_t* d_nw, const int32_t* d_leap, const int32_t* d_greedy,
                       const int32_t* d_answers, int64_t n, unsigned long long* d_counters);
/* `_run_benchmark` for a whole resident batch in one call (benchmark_utils.h:231-259): optional re-pack of the
 * resident ASCII, then every aligner whose output pointer is non-NULL, then the counters.  Enqueue only.
 * Order inside the call: Greedy beside the chain NW -> LEAP (LEAP scheduled by the NW penalties); with d_nw NULL and a wide
 * band, Greedy first and LEAP scheduled by its penalties.
 * repack: 0 = use the planes as they are; 1 = pack first, in stream order; 2 = pack first, PIPELINED: the pack of this call
 * fills a second set of planes on its own stream and so overlaps the aligners of the previous call (pack waits on memory for
 * half of its time, the aligners are instruction-bound); this call's aligners wait for it.  With 2 the caller guarantees that
 * nothing it enqueued since the previous call on this batch changes what pack reads.
 * 3 = OVERLAPPED CALLS, the form a caller with a stream of batches (or of passes) wants: as 2, and in addition nothing of this
 * call waits for the previous call's Greedy kernel — consecutive calls form three chains on streams of the library (NW -> LEAP
 * -> counters -> NW ..., Greedy -> Greedy, pack -> pack; a call's counters also wait for its Greedy).  The caller's stream is
 * NOT joined: the
 * outputs and counters of all calls so far are complete on it after asm_pipeline_join_async (asm_synchronize also waits for
 * them).  The caller ALTERNATES between two sets of output arrays from call to call (a set is written again two calls later,
 * when the library has seen its counters finish), and calls asm_pipeline_join_async before it touches the batch or the outputs
 * in any other way.  A later call with repack != 3 joins by itself.  Passing the previous overlapped call's arrays again without a
 * join in between is refused (ASM_EINVAL).  Consecutive calls may name DIFFERENT batches (a caller rotating over several resident
 * batches): they are paced like calls on one batch — the pack of call c starts behind the counters of call c - 2.  A call that
 * cannot overlap (the Greedy-first shape above, an empty batch) runs as repack = 2, ordered behind every earlier call. */
int asm_run_benchmark_async(asm_handle* h, asm_batch* b, const asm_params* p, int repack, int32_t* d_nw,
                            int32_t* d_leap, int32_t* d_greedy, const int32_t* d_answers,
                            unsigned long long* d_counters);

/* Joins the overlapped calls (repack = 3) into the handle's stream: everything they enqueued is ordered before whatever is
 * enqueued on that stream next.  Enqueue only; a no-op when there are none. */
int asm_pipeline_join_async(asm_handle* h);

/* Per-kernel timing INSIDE a caller's timed region: after asm_profile_enable(h, max_calls, kernel_mask) the next max_calls
 * calls of asm_run_benchmark_async bracket the selected kernels (bit 0 pack, 1 NW, 2 LEAP, 3 Greedy) with HIP events
 * recorded on the stream that kernel is launched on (Greedy: the handle's side stream); asm_profile_read synchronises and
 * returns ms[call][4] (-1 where a kernel was not launched or not selected).  An event record keeps the next kernel of its
 * stream from starting early, so bracket only what is needed: all four cost ~8 % of the C2 step, Greedy alone (its own
 * stream) ~1 %.  asm_profile_enable(h, 0, 0) switches it off. */
int asm_profile_enable(asm_handle* h, int max_calls, unsigned kernel_mask);
int asm_profile_read(asm_handle* h, float* ms, int cap_calls, int* n_calls);

/* ---- read mapping: k-mer index, pigeonhole seeding, bit-vector verification, CIGAR, Greedy ----------------------------
 * The counterpart of the reference's read mapper (GASMA/mapper/{indexer,main}.cpp), exact by construction; the full contract is
 * docs/design/mapper.md.  Byte rule: A, C, G, T match only themselves, every other byte mismatches everything (N against N
 * included) — unlike the pack kernel's rule, which Greedy keeps.  Text and reads are taken upper case.
 * Best hit of a read q (1 <= m <= 511): over q_0 = q and, with both_strands, q_1 = reverse complement (A<->T, C<->G), over
 * every sequence r and every T_r[i, j): smallest d = Lev(q_s, T_r[i, j)), then s, then r, then smallest j, then largest i.  The
 * read is mapped when d <= max_errors.  A read is searched only when m >= (max_errors + 1) * k (else flag TOO_SHORT).
 * With max_occ > 0, k-mer buckets above max_occ are skipped (flag SEED_CAPPED; the answer is the best over the candidates seen).
 *
 * asm_index_build: text = the sequences back to back, seq_off = n_seqs + 1 offsets into it (host); k in [8, 14]; total length
 *                  below 2^32, n_seqs in [1, 2^26).  The index ((4^k + 1) uint32 bucket offsets + one uint32 per k-mer) and the
 *                  text stay in HBM.  Synchronous.
 * asm_map_reads:   host in, host out; any n (chunked inside).  out[i] for read i; cigar_ops = [n][cigar_cap] entries count << 3 |
 *                  op (0 M, 1 I, 2 D; I = read base absent from the reference, D = reference base absent from the read),
 *                  cigar_nops[i] = entries of row i (above cigar_cap: truncated, flag CIGAR_TRUNCATED); both may be NULL
 *                  (cigar_cap 0).  Greedy (k = greedy_k, x = o = e = 1, clean tails) runs on (q_s, T_r[w, min(w + m + 1, len_r)))
 *                  with w = pos ? pos - 1 : 0, as mapper/main.cpp:79-95 calls it; MAPQ = min(254, 60 + greedy_cost).
 *                  Unmapped reads: seq_id -1, pos = end = 0, dist -1, greedy_cost -1, cigar_nops 0.  Synchronous.
 * asm_map_reads_all: every locus within max_errors, not only the best hit (SeqAn3's hit_all / hit_all_best / hit_strata).  For
 *                  strand s, sequence r and end j, D(j) = min_i Lev(q_s, T_r[i, j)); a locus is a maximal run of consecutive ends j
 *                  of one (s, r) with D(j) <= max_errors (never across two sequences).  Its d = min D over the run, its end j =
 *                  the smallest end of the run reaching d, its pos = the largest i with Lev(q_s, T_r[i, j)) = d; CIGAR, Greedy and
 *                  MAPQ as for asm_map_reads.  Loci are ranked by (d, s, r, j); with d_best the first one's d, the reported loci are
 *                  those with d <= min(max_errors, d_best + strata), strata in [0, 15] (0: hit_all_best; >= max_errors: hit_all).
 *                  n_hits[i] = how many (uncapped); the first min(n_hits[i], max_hits) are written to out[i][0..], max_hits in
 *                  [1, 256]; cigar_ops = [n][max_hits][cigar_cap], cigar_nops = [n][max_hits].  Rank 0 is, field for field,
 *                  asm_map_reads' record of the read (an unmapped read: n_hits 0 and the unmapped record at rank 0), plus flag
 *                  HITS_TRUNCATED.  Ranks >= 1 carry flag SECONDARY; every record of a read with n_hits > max_hits carries
 *                  HITS_TRUNCATED.  A slot beyond the reported ones: seq_id -1, pos = end = 0, dist -1, greedy_cost -1, flags 0,
 *                  cigar_nops 0 (its cigar_ops row is not written).  Synchronous.
 * asm_map_pairs:   paired-end reads, FR orientation (docs/design/mapper.md, "Paired-end reads").  Mate 1 of pair i is reads1 /
 *                  off1 [i], mate 2 is reads2 / off2 [i], 1 to 511 bytes each; both_strands must be 1.  A mate's loci are those of
 *                  asm_map_reads_all with strata = max_errors.  For loci A (mate 1) and B (mate 2), F = the one with s = 0, R = the
 *                  one with s = 1, m_F = F's mate length: projected span L = j_R - j_F + m_F.  Concordant: same r, s_A != s_B and
 *                  min_insert <= L <= max_insert (0 <= min_insert <= max_insert <= ASM_MAP_MAX_INSERT).  Pair order: (d_A + d_B, s_A,
 *                  r, j_A, j_B); the best concordant pair is reported and n_concordant[i] counts the concordant pairs with its d sum
 *                  (uncapped, saturating).  Without one, and with rescue_errors in [0, 15] (-1: off), each mapped mate X (its best
 *                  hit) is an anchor and its partner b is searched on strand 1 - s_X in T_r over the ends that keep L in range: the
 *                  smallest (D(j), j) with D(j) <= rescue_errors and D(j) < m_b is the rescued locus; of two rescued pairs the smaller
 *                  in pair order is reported.  out = [n][2] records (mate 1, mate 2), cigar_ops = [n][2][cigar_cap], cigar_nops =
 *                  [n][2], tlen[i] = max(end) - min(pos) when both mates map to the same r, else 0.  A proper pair has PROPER_PAIR on
 *                  both records and RESCUED on a rescued one; a non-rescued proper record is, flags apart, asm_map_reads_all's record of
 *                  that locus.  Without a proper pair each record is asm_map_reads' record of that mate.  Synchronous. */
#define ASM_MAP_MAPPED 1
#define ASM_MAP_TOO_SHORT 2
#define ASM_MAP_SEED_CAPPED 4
#define ASM_MAP_CIGAR_TRUNCATED 8
#define ASM_MAP_SECONDARY 16
#define ASM_MAP_HITS_TRUNCATED 32
#define ASM_MAP_PROPER_PAIR 64
#define ASM_MAP_RESCUED 128
#define ASM_MAP_MAX_HITS 256
#define ASM_MAP_MAX_INSERT 8192
#define ASM_MAP_MIN_K 8
#define ASM_MAP_MAX_K 14
#define ASM_MAP_MAX_READ 511
#define ASM_MAP_MAX_ERRORS 15
typedef struct asm_index asm_index;
int asm_index_build(asm_handle* h, const char* text, const uint64_t* seq_off, int32_t n_seqs, int k, asm_index** out);
int asm_index_free(asm_handle* h, asm_index* ix);
typedef struct asm_map_params {
    int32_t max_errors;   /* e in [0, 15]                                                   */
    int32_t both_strands; /* 0: forward only; 1: reverse complement too                      */
    int32_t max_occ;      /* 0 = unlimited                                                   */
    int32_t greedy_k;     /* Greedy's band (the reference mapper uses 3); [0, 50]            */
} asm_map_params;
typedef struct asm_map_hit {
    int32_t seq_id;       /* r, -1 when unmapped                                             */
    uint32_t pos, end;    /* i, j: 0-based, T_r[pos, end)                                    */
    int16_t dist;         /* d, -1 when unmapped                                             */
    uint8_t strand;       /* s: 0 forward, 1 reverse complement                              */
    uint8_t flags;        /* ASM_MAP_*                                                       */
    int32_t greedy_cost;  /* Greedy's cost on the hit's window, -1 when unmapped             */
} asm_map_hit;
int asm_map_reads(asm_handle* h, const asm_index* ix, int64_t n, const char* reads, const uint32_t* read_off,
                  const asm_map_params* p, asm_map_hit* out, uint16_t* cigar_ops, int cigar_cap, uint8_t* cigar_nops);
int asm_map_reads_all(asm_handle* h, const asm_index* ix, int64_t n, const char* reads, const uint32_t* read_off,
                      const asm_map_params* p, int strata, int max_hits, uint32_t* n_hits /* [n] */,
                      asm_map_hit* out /* [n][max_hits] */, uint16_t* cigar_ops /* [n][max_hits][cigar_cap] */, int cigar_cap,
                      uint8_t* cigar_nops /* [n][max_hits] */);
typedef struct asm_pair_params {
    int32_t min_insert;    /* projected span L in [min_insert, max_insert], 0 <= min_insert <= max_insert <= 8192 */
    int32_t max_insert;
    int32_t rescue_errors; /* mate rescue's error bound in [0, 15]; -1 = no rescue                                  */
} asm_pair_params;
int asm_map_pairs(asm_handle* h, const asm_index* ix, int64_t n, const char* reads1, const uint32_t* off1, const char* reads2,
                  const uint32_t* off2, const asm_map_params* p, const asm_pair_params* pp, asm_map_hit* out /* [n][2] */,
                  int32_t* tlen /* [n] */, uint32_t* n_concordant /* [n] */, uint16_t* cigar_ops /* [n][2][cigar_cap] */,
                  int cigar_cap, uint8_t* cigar_nops /* [n][2] */);
/* asm_map_pairs_all: every concordant pair within strata, not only the best (docs/design/mapper.md, "Secondary pairs").  Inputs,
 *                  loci, concordance, pair order, rescue, n_concordant and the tlen rule are asm_map_pairs'.  The eligible pairs are
 *                  the concordant combinations of a mate-1 locus and a mate-2 locus with d_A + d_B <= sum_best + strata (sum_best =
 *                  the smallest sum), strata in [0, 2 * ASM_MAP_MAX_ERRORS] (0: the best sum only; >= 2 max_errors: all of them).
 *                  n_pairs[i] = how many (uncapped, saturating); the first min(n_pairs[i], max_pairs) in pair order are written to
 *                  out[i][0..][0, 1] (mate 1, mate 2), max_pairs in [1, ASM_MAP_MAX_HITS]; tlen = [n][max_pairs], cigar_ops =
 *                  [n][max_pairs][2][cigar_cap], cigar_nops = [n][max_pairs][2].  Rank 0 is, field for field, asm_map_pairs' answer
 *                  (records, tlen, n_concordant, CIGARs; rescued and unpaired fragments too, with n_pairs 0), plus flag
 *                  HITS_TRUNCATED.  A record of rank >= 1 is, flags apart, asm_map_reads_all's record of that locus (strata =
 *                  max_errors) and carries MAPPED | PROPER_PAIR | SECONDARY; tlen[i][rank] = max(end) - min(pos) of that pair.  Every
 *                  record of a fragment with n_pairs > max_pairs carries HITS_TRUNCATED.  An unused slot: the unused record of
 *                  asm_map_reads_all (its cigar_ops row is not written, cigar_nops 0), tlen 0.  Synchronous. */
int asm_map_pairs_all(asm_handle* h, const asm_index* ix, int64_t n, const char* reads1, const uint32_t* off1, const char* reads2,
                      const uint32_t* off2, const asm_map_params* p, const asm_pair_params* pp, int strata, int max_pairs,
                      uint32_t* n_pairs /* [n] */, asm_map_hit* out /* [n][max_pairs][2] */, int32_t* tlen /* [n][max_pairs] */,
                      uint32_t* n_concordant /* [n] */, uint16_t* cigar_ops /* [n][max_pairs][2][cigar_cap] */, int cigar_cap,
                      uint8_t* cigar_nops /* [n][max_pairs][2] */);

/* Mapping quality (docs/design/mapper.md, "Mapping quality"): the model is handle state, like the stream, and all eight mapping
 * calls honour it.  ASM_MAPQ_REFERENCE (the default): MAPQ = min(254, 60 + greedy_cost) of a mapped record.  ASM_MAPQ_GAP: what
 * the exact search proves, T(n, g) with n the loci (or concordant pairs) that tie for the best and g a lower bound on the edit gap to
 * the nearest alternative: T(1, g) = min(60, 20 g), T(2) = 3, T(3..4) = 1, T(>= 5) = 0; at most 20 for a SEED_CAPPED read and for a
 * rescued mate; 0 for a locus or pair that is not the best.  Unmapped records and unused slots have 0 under both.  The records,
 * CIGARs and greedy_cost of every call are the same under both models; under ASM_MAPQ_GAP the best-hit calls take the all-hits
 * path to the loci, which costs time.
 * asm_map_set_mapq_model: a model other than the two is ASM_EINVAL.
 * asm_map_last_mapq: the MAPQ of every record slot of the last successful in-memory mapping call on this handle (asm_map_reads,
 *                  asm_map_reads_all, asm_map_pairs, asm_map_pairs_all), in the layout of that call's `out` array: count must be
 *                  its n, n * max_hits, 2 n or 2 n * max_pairs; any other count, or no earlier call, is ASM_EINVAL.  asm_map_hit
 *                  is a full 20-byte record, so the value travels beside it.  The file calls write it into column 5. */
#define ASM_MAPQ_REFERENCE 0
#define ASM_MAPQ_GAP 1
int asm_map_set_mapq_model(asm_handle* h, int model);
int asm_map_get_mapq_model(const asm_handle* h);
int asm_map_last_mapq(asm_handle* h, uint8_t* dst /* [count] */, int64_t count);

/* Optional SAM tags (docs/design/mapper.md, "MD tag"): a mask on the handle, like the MAPQ model; 0 (the default) leaves every byte
 * of every call as it is.  The four file calls (asm_map_file, asm_map_pairs_file and their _sorted forms) honour it.
 * ASM_SAM_TAG_MD:  every line that shows a CIGAR carries MD:Z:<tag> directly behind XG:i:<n>: primaries, secondaries (SEQ '*'), both
 *                  mates, rescued mates.  A line whose CIGAR is '*' carries none: unmapped lines, an unmapped mate that borrows
 *                  RNAME and POS, a row of more than 64 operations.  The tag walks the CIGAR over the read on the alignment's
 *                  strand against T_r[pos, end) under the byte rule above (N against N mismatches): a number for every run of
 *                  matches (0 included), the reference byte of a mismatch, '^' and the reference bytes of a deletion; insertions
 *                  write nothing.  Reference bytes as the upper-cased text holds them, a byte outside A-Z as 'N'.  Letters in the
 *                  tag plus inserted bases of the CIGAR = dist (NM).  At most 78 bytes (15 single-base deletions, 16 three-digit
 *                  numbers); ASM_MAP_MD_CAP is the row a tag and its NUL always fit.  The tag is built on the device.
 * asm_map_set_sam_tags: a mask with any other bit, or a NULL handle, is ASM_EINVAL; the mask is checked first.
 * asm_md_format:   the same rule on the host, no device: the counterpart of asm_cigar_format for the in-memory calls, whose record
 *                  slots carry no MD.  ops[0, nops) is a CIGAR row (count << 3 | op; M, I and D only), read_on_strand the read as
 *                  the alignment sees it (the reverse complement for strand 1), ref_window T_r[pos, end), e.g. from
 *                  asm_index_get_text; both are upper-cased here.  Returns the tag's length, out NUL-terminated.  ASM_EINVAL: a
 *                  NULL argument, a negative length, a row with another operation or one that does not consume exactly read_len
 *                  read and ref_len reference bases, or out_cap below the tag's length + 1; nothing is written beyond out_cap. */
#define ASM_SAM_TAG_MD 1
#define ASM_MAP_MD_CAP 80
int asm_map_set_sam_tags(asm_handle* h, unsigned mask);
unsigned asm_map_get_sam_tags(const asm_handle* h);
int asm_md_format(const uint16_t* ops, int nops, const char* read_on_strand, int read_len, const char* ref_window, int ref_len,
                  char* out, size_t out_cap);

/* BAM output (docs/design/mapper.md, "BAM output"): the format is handle state, like the MAPQ model and the tag mask; ASM_OUT_SAM (the
 * default) leaves every byte of every call as it is.  Under ASM_OUT_BAM the four file calls (asm_map_file, asm_map_pairs_file and
 * their _sorted forms) write a BAM file to sam_path: the records say what the SAM lines say (SAM spec 4.2; integer tags in the
 * smallest type, SEQ bytes outside =ACMGRSVTWYHKDBN as N, QUAL 0xff when its length is not SEQ's), encoded on the device, in a BGZF
 * container of stored deflate blocks (what `samtools view -u` writes) framed on the device.  The uncompressed stream is the BAM header
 * (magic, `header` as l_text and text, n_ref, the names of seq_names and the lengths of the index) in blocks of its own, then the
 * records cut every ASM_BGZF_PAYLOAD bytes counted from the first record, then the 28-byte EOF block; the file does not depend on
 * chunk_bytes, ASM_MAP_CHUNK or max_device_bytes.  Every other argument, error report and stats field keeps its meaning: bytes_out
 * counts the file's bytes behind the header's blocks (EOF block included), asm_sam_sort_stats.bytes_held the record bytes held.  A
 * QNAME longer than 254 bytes cannot be a BAM record: ASM_EINVAL, asm_last_error names the 1-based record (and the file, for pairs);
 * among the errors of one device chunk it ranks behind a malformed record and before a name mismatch.
 * asm_map_set_output_format: another value, or a NULL handle, is ASM_EINVAL; the value is checked first.
 * asm_map_get_output_format: ASM_OUT_SAM for a NULL handle.
 * asm_bgzf_bound:  the bytes asm_bgzf_frame writes for n input bytes; no device.
 * asm_bgzf_frame:  src[0, n) (host) framed into dst (host) by the device kernel the file calls use: blocks of ASM_BGZF_PAYLOAD bytes,
 *                  the last one shorter, none at all for n = 0; with_eof: the EOF block behind them.  *dst_len = asm_bgzf_bound(n,
 *                  with_eof).  A dst_cap below that is ASM_EINVAL, and nothing is written.  Synchronous.
 * The container's level (docs/design/mapper.md, "Deflate") is handle state too.  ASM_BGZF_STORED (the default) leaves every byte as
 * described above.  Under ASM_BGZF_DEFLATE every block, the header's included, is one deflate block encoded on the device: stored,
 * fixed Huffman or dynamic Huffman, whichever has the fewest bits, so no block is longer than its stored form and an incompressible
 * one is byte for byte the stored one.  The uncompressed stream and its cut are the same, the bytes are a function of that stream
 * alone, and bytes_out counts the bytes really written.  The level has no effect under ASM_OUT_SAM.
 * asm_map_set_bgzf_level: another value, or a NULL handle, is ASM_EINVAL; the value is checked first.
 * asm_map_get_bgzf_level: ASM_BGZF_STORED for a NULL handle.
 * asm_bgzf_compress:      asm_bgzf_frame with a level: dst_cap below asm_bgzf_bound(n, with_eof) is ASM_EINVAL at both levels, and
 *                         *dst_len is what was written.  Level 0 gives asm_bgzf_frame's bytes.
 * asm_bgzf_compress_host: the same bytes from the host build of the same encoder; no device, no handle. */
#define ASM_OUT_SAM 0
#define ASM_OUT_BAM 1
#define ASM_BGZF_PAYLOAD 65280
#define ASM_BGZF_STORED 0
#define ASM_BGZF_DEFLATE 1
int asm_map_set_output_format(asm_handle* h, int format);
int asm_map_get_output_format(const asm_handle* h);
size_t asm_bgzf_bound(size_t n, int with_eof);
int asm_bgzf_frame(asm_handle* h, const void* src, size_t n, int with_eof, void* dst, size_t dst_cap, size_t* dst_len);
int asm_map_set_bgzf_level(asm_handle* h, int level);
int asm_map_get_bgzf_level(const asm_handle* h);
int asm_bgzf_compress(asm_handle* h, const void* src, size_t n, int with_eof, int level, void* dst, size_t dst_cap, size_t* dst_len);
int asm_bgzf_compress_host(const void* src, size_t n, int with_eof, int level, void* dst, size_t dst_cap, size_t* dst_len);

/* The container read back (docs/design/mapper.md, "Compressed input"): a BGZF file is a sequence of gzip members of at most 64 KiB,
 * each with its compressed size (BSIZE) in a BC extra subfield and its CRC-32 and ISIZE (at most 65 536) behind its deflate stream.
 * The host finds every member without decoding; the members are decoded independently, one wavefront each, by a complete RFC 1951
 * decoder (stored, fixed and dynamic blocks, any number of them; zlib's two allowances for the distance code, one code of one bit
 * or none, and no others).  Empty members are allowed anywhere, the EOF block may be missing, an empty input is an empty output.
 * Corrupt input (a bad member header, a member reaching past the end, trailing bytes that are no member, a decoder error, an ISIZE or
 * CRC mismatch) is ASM_EINVAL; asm_last_error names the member's 0-based index, its offset in src and what is wrong; of several bad
 * members the first is named.  A gzip file that is not BGZF (1f 8b, no BC subfield in its first member) is ASM_EUNSUPPORTED, and the
 * message says that bgzip makes it usable.  dst is written only when the whole container is sound.
 *
 * asm_bgzf_decompressed_size: walks and checks the container's headers and sums ISIZE; host only, nothing is decoded.
 * asm_bgzf_decompress:        src (host) decoded into dst (host) by bgzf_inflate_kernel; dst_cap below the size is ASM_EINVAL.
 * asm_bgzf_decompress_host:   the same bytes and the same errors from the host build of the same decoder; no device, no handle.
 * asm_map_file and asm_map_file_sorted read such a file as it is (below, "Compressed input" at asm_map_file). */
int asm_bgzf_decompressed_size(const void* src, size_t n, size_t* out_len);
int asm_bgzf_decompress(asm_handle* h, const void* src, size_t n, void* dst, size_t dst_cap, size_t* dst_len);
int asm_bgzf_decompress_host(const void* src, size_t n, void* dst, size_t dst_cap, size_t* dst_len);

/* asm_map_file:    a FASTQ file in, a SAM file out (docs/design/mapper.md, "Files: FASTQ in, SAM out"); single-end, synchronous.  The
 *                  file is read in chunks of about chunk_bytes (0: 16 MiB) cut at record boundaries; a chunk is parsed, mapped
 *                  and formatted on the device while the next one is read and copied in and the one before is copied out and
 *                  written.  Four-line FASTQ: record i is lines 4i .. 4i+3 by line number alone, lines end in LF or CRLF, the last
 *                  newline may be missing; line 0 starts with '@' and QNAME is its first word, line 2 starts with '+'; SEQ is
 *                  upper-cased, QUAL copied.  Malformed input (line 0 without '@', line 2 without '+', a line count that is not a
 *                  multiple of 4): ASM_EINVAL, asm_last_error names the 1-based record, and what sam_path holds is unspecified.  A
 *                  file starting with '>' (FASTA): ASM_EUNSUPPORTED.  An empty file gives the header alone.  sam_path is created or
 *                  truncated; header (may be NULL) is written first, as it is.  The records are, byte for byte, the lines asm-map
 *                  writes for the same reads: max_hits = 0 asm_map_reads' best hit per read, max_hits in [1, 256] the loci of
 *                  asm_map_reads_all (strata in [0, 15]) in rank order with NH, HI and XH; seq_names = the n_seqs RNAMEs of the index;
 *                  an unmapped, empty or too long (> ASM_MAP_MAX_READ) read gives the unmapped line; CIGAR is '*' above 64
 *                  operations.  The output does not depend on chunk_bytes or ASM_MAP_CHUNK.
 *                  Compressed input (asm_map_file and asm_map_file_sorted only; docs/design/mapper.md, "Compressed input"): a file
 *                  that starts with a BGZF member (what bgzip writes) is inflated on the device, member by member, and its
 *                  concatenated member outputs are the FASTQ text under the contract above.  Empty members are allowed anywhere,
 *                  the EOF block included, and the EOF block may be missing; a file that is only an EOF block is an empty file
 *                  (the header alone is written); CR LF, lines and records may straddle members and chunks.  The SAM or BAM bytes
 *                  equal those of the same call on the inflated text, for every chunk_bytes (which stays text bytes per chunk),
 *                  every ASM_MAP_CHUNK and every way the text was cut into members.  bytes_in stays the FASTQ text bytes; every
 *                  other stats field keeps its meaning.  Corrupt input (a bad member header, a member reaching past the end of the
 *                  file, trailing bytes that are no member, a decoder error, an ISIZE or CRC mismatch): ASM_EINVAL, asm_last_error
 *                  names the member's 0-based index and its file offset and says what is wrong; among the errors of one chunk the
 *                  smallest member is reported, before any record error of that chunk.  A gzip file that is not BGZF (magic 1f 8b,
 *                  no BC subfield in its first member): ASM_EUNSUPPORTED, the message says that the file is plain gzip and that
 *                  bgzip makes it usable.  asm_map_pairs_file* take two such files ("Compressed input" there);
 *                  asm_index_build_file reads plain text only.
 * asm_fastq_cut:   the length of the longest prefix of buf[0, nbytes) made of whole four-line records (every line ending in LF), and
 *                  how many records that is; no device. */
typedef struct asm_map_file_stats {
    int64_t reads, mapped, too_long, records; /* FASTQ records; reads with a mapped primary; longer than ASM_MAP_MAX_READ; SAM lines */
    int64_t chunks, bytes_in, bytes_out;      /* device chunks; FASTQ bytes; SAM bytes without the header */
    double seconds, seconds_read, seconds_write; /* whole call; reader busy; writer busy */
} asm_map_file_stats;
int asm_map_file(asm_handle* h, const asm_index* ix, const char* const* seq_names /* [n_seqs] */, const char* fastq_path,
                 const char* sam_path, const char* header, const asm_map_params* p, int max_hits, int strata, int64_t chunk_bytes,
                 asm_map_file_stats* stats /* may be NULL */);
size_t asm_fastq_cut(const char* buf, size_t nbytes, int64_t* records);

/* asm_map_pairs_file: two FASTQ files in, a paired SAM file out (docs/design/mapper.md, "Files: two FASTQ files in, paired SAM out");
 *                  synchronous.  Record i of fastq1_path and record i of fastq2_path are the mates of pair i; each file follows
 *                  asm_map_file's input contract.  The two files are read in step, about chunk_bytes (0: 16 MiB) of both together
 *                  per chunk, and a chunk is parsed, paired, mapped and formatted on the device while the next one is read and the
 *                  one before is written.  The answer is asm_map_pairs' (best concordant pair, mate rescue; both_strands must be
 *                  1): after `header`, two lines per pair, mate 1 then mate 2, byte for byte the lines asm-map -1 -2 writes.  QNAME
 *                  is the first word without a trailing /1 or /2 and must be the same for both mates.  A pair with an empty or too
 *                  long (> ASM_MAP_MAX_READ) mate gives two unmapped lines.  ASM_EINVAL, naming the 1-based record and the file: a
 *                  malformed or truncated record, files with different numbers of records, mates whose names differ; the first
 *                  device chunk that holds an error reports it, a malformed record of file 1 before one of file 2 before a name,
 *                  each with its smallest record.  ASM_EUNSUPPORTED: a file starting with '>'.  Two empty files give the header
 *                  alone.  The output does not depend on chunk_bytes or ASM_MAP_CHUNK.
 *                  Compressed input (asm_map_pairs_file and asm_map_pairs_file_sorted; docs/design/mapper.md, "Compressed input for
 *                  pairs"): two files that each start with a BGZF member are inflated on the device, each under asm_map_file's
 *                  "Compressed input" contract (empty members anywhere, an optional EOF block, a file that is only an EOF block is
 *                  an empty file), and the concatenated member outputs of file f are its FASTQ text under the contract above (LF or
 *                  CR LF, an optional last newline per file, lines and records straddling members and chunks).  The kind is probed
 *                  from each file's first bytes at open.  The SAM or BAM bytes equal those of the same call on the two inflated
 *                  texts, for every chunk_bytes (which stays text bytes of both files together per chunk), every ASM_MAP_CHUNK and
 *                  every way either text was cut into members, the two files cut differently included; sorted output, BAM at both
 *                  levels, MD, both MAPQ models and rescue run behind the text unchanged.  Both files must be of one kind: one
 *                  BGZF file and one text file is ASM_EUNSUPPORTED, the message says which file is which kind (a file of no bytes
 *                  goes with either).  Plain gzip in either file: ASM_EUNSUPPORTED, asm_map_file's message, naming the file.
 *                  A corrupt container: ASM_EINVAL, "file <1|2>: BGZF member <0-based index> at offset <file offset>: <what>",
 *                  <what> as for asm_map_file.  Of the errors of one chunk: the smallest bad member of file 1, then the smallest
 *                  bad member of file 2, then the record errors in the order above.  The ends of the files are reported with the
 *                  messages and record numbers above (a truncated record of a file read to its end, then a file that holds records
 *                  without a mate), behind the pairs of the chunk that shows them; a missing mate is reported as soon as one file
 *                  is read to its end and holds no further whole record while the other holds one, without reading the longer
 *                  file on.  One difference to text input: line counts are learnt on the device chunk by chunk, so where the longer
 *                  file also ends in a truncated record, the text call may have read that end already and report it, and this call
 *                  reports the missing mate.  bytes_in stays the FASTQ text bytes of both files; carry_peak is the largest sum of
 *                  the two texts' leftovers kept on the device between two chunks, in text bytes, and the one field a failed call
 *                  on compressed input still sets; every other stats field keeps its meaning.  The argument checks come first and
 *                  touch neither device, index nor file; the handle stays usable after an error.
 * asm_fastq_cut_n: asm_fastq_cut bounded to the first max_records records; no device. */
typedef struct asm_map_pairs_file_stats {
    int64_t pairs, proper, rescued, unsent;   /* fragments; proper pairs; rescued mates; pairs with an empty or too long mate */
    int64_t records, chunks, bytes_in, bytes_out, carry_peak; /* SAM lines; device chunks; FASTQ bytes of both files; SAM bytes without
                                                                 the header; the most bytes held back between two chunks: by the reader,
                                                                 or for compressed input on the device (text bytes) */
    double seconds, seconds_read, seconds_write; /* whole call; reader busy; writer busy */
} asm_map_pairs_file_stats;
int asm_map_pairs_file(asm_handle* h, const asm_index* ix, const char* const* seq_names /* [n_seqs] */, const char* fastq1_path,
                       const char* fastq2_path, const char* sam_path, const char* header, const asm_map_params* p,
                       const asm_pair_params* pp, int64_t chunk_bytes, asm_map_pairs_file_stats* stats /* may be NULL */);
size_t asm_fastq_cut_n(const char* buf, size_t nbytes, int64_t max_records, int64_t* records);

/* asm_map_file_sorted, asm_map_pairs_file_sorted: the two file calls with coordinate-sorted output (docs/design/mapper.md, "Sorted
 *                  output"); synchronous.  Input contract, answers, error reports and the first stats struct are those of the
 *                  unsorted call, under the sorted call's name.  The file holds `header` (as it is; the library does not edit it)
 *                  and then the lines the unsorted call writes, byte for byte, in ascending order of (tid, POS) as the line shows
 *                  them: tid = the index of its RNAME in seq_names, n_seqs for '*' (behind everything), POS its POS column.  An
 *                  unmapped mate that borrows RNAME and POS sorts with its mate; secondary lines sort each by its own key.  Lines
 *                  with equal keys keep the unsorted call's order (file order, then rank, then mate 1 before mate 2).  The output
 *                  does not depend on chunk_bytes or ASM_MAP_CHUNK.  The whole SAM text stays on the device until the last chunk is
 *                  formatted and is then sorted there and written in slabs of at most max(chunk_bytes, the longest line) bytes;
 *                  max_device_bytes caps the held text plus the line tables (0: no cap but the device's memory; negative:
 *                  ASM_EINVAL).  When the cap or the allocator says no: ASM_ENOMEM, asm_last_error says that sorted output keeps the
 *                  whole SAM text on the device and names the bytes reached; what sam_path holds is then unspecified and the handle
 *                  stays usable.  2^32 lines or more: ASM_EUNSUPPORTED.  An input error fails the call before any sorted byte is
 *                  written.  An empty input gives the header alone. */
typedef struct asm_sam_sort_stats {
    int64_t lines, bytes_held, slabs;  /* lines sorted; SAM bytes kept on the device; output slabs written */
    double seconds_sort;               /* from the last chunk formatted to the last slab handed to the writer */
} asm_sam_sort_stats;
int asm_map_file_sorted(asm_handle* h, const asm_index* ix, const char* const* seq_names /* [n_seqs] */, const char* fastq_path,
                        const char* sam_path, const char* header, const asm_map_params* p, int max_hits, int strata, int64_t chunk_bytes,
                        int64_t max_device_bytes, asm_map_file_stats* stats /* may be NULL */,
                        asm_sam_sort_stats* sort_stats /* may be NULL */);
int asm_map_pairs_file_sorted(asm_handle* h, const asm_index* ix, const char* const* seq_names /* [n_seqs] */, const char* fastq1_path,
                              const char* fastq2_path, const char* sam_path, const char* header, const asm_map_params* p,
                              const asm_pair_params* pp, int64_t chunk_bytes, int64_t max_device_bytes,
                              asm_map_pairs_file_stats* stats /* may be NULL */, asm_sam_sort_stats* sort_stats /* may be NULL */);

/* BAM index (docs/design/mapper.md, "BAM index"): handle state, like the output format and the container's level.  ASM_BAM_INDEX_NONE
 * (the default) leaves every byte, launch and allocation of every call as it is.  Under ASM_OUT_BAM and ASM_BAM_INDEX_BAI the two sorted
 * file calls write `<sam_path>.bai` (created or truncated) when the BAM file is complete: a BAI index (SAM spec 5.2) in the canonical
 * form of the design document, built on the device from the tables the sort leaves there.  The BAM file is byte for byte the one
 * written without the index, and every argument, error and stats field keeps its meaning.  Under ASM_OUT_SAM and in the unsorted
 * calls the setting has no effect and no `.bai` path is opened.  BAI holds coordinates below 2^29: a sequence of the index of more
 * than 2^29 bases is ASM_EUNSUPPORTED, found with the argument checks before either file is opened; asm_last_error names the sequence
 * and says that such a reference needs a .csi index.  The index tables, the block table and the image are allocations of the sorted
 * call's hold: they count against max_device_bytes, and running out is its ASM_ENOMEM.  A failed write is ASM_EINVAL, "writing the BAM
 * index failed".
 * asm_map_set_bam_index:  another value, or a NULL handle, is ASM_EINVAL; the value is checked first.
 * asm_map_get_bam_index:  ASM_BAM_INDEX_NONE for a NULL handle.
 * asm_map_last_bam_index: of the handle's last sorted BAM call that wrote an index; all zero before one.  bins: the real bins; chunks:
 *                         the chunks of the real bins; intervals: the sum of n_intv; no_coor: n_no_coor; bytes: the index file.
 * asm_bam_index_host:     a whole coordinate-sorted BAM file in memory (any BGZF cut, any number of deflate blocks per member) -> the
 *                         index's bytes, by the host build of the same core; no device, no handle.  dst_cap below the size:
 *                         ASM_EINVAL, *dst_len = the size needed, nothing written.  A corrupt container: asm_bgzf_decompress_host's
 *                         error.  A malformed BAM stream (bad magic, a record reaching past the end, a refID of n_ref or more, a bin
 *                         that is not reg2bin of the record) is ASM_EINVAL and asm_last_error names the 0-based record; records out
 *                         of (refID, pos) order, refID -1 behind everything, are ASM_EINVAL naming the first record below its
 *                         predecessor; a position or end above 2^29 is ASM_EUNSUPPORTED. */
#define ASM_BAM_INDEX_NONE 0
#define ASM_BAM_INDEX_BAI 1
typedef struct asm_bam_index_stats {
    int64_t refs, bins, chunks, intervals, no_coor, bytes;
    double seconds_index; /* from the BAM file complete to the index file written */
} asm_bam_index_stats;
int asm_map_set_bam_index(asm_handle* h, int kind);
int asm_map_get_bam_index(const asm_handle* h);
int asm_map_last_bam_index(asm_handle* h, asm_bam_index_stats* out);
int asm_bam_index_host(const void* bam, size_t n, void* dst, size_t dst_cap, size_t* dst_len);

/* asm_index_build_file: asm_index_build from a FASTA file (docs/design/mapper.md, "Reference: FASTA in, index out"); synchronous.  The
 *                  file is read in chunks of about chunk_bytes (0: 16 MiB) that may end anywhere except inside a header line, so a
 *                  sequence line may have any length; a chunk is parsed on the device while the next one is read and copied in.
 *                  The file: lines end in LF or CRLF, the last newline may be missing.  A line whose first byte is '>' is a header
 *                  line and starts a new sequence; its name is the first word behind the '>' (blanks and tabs are skipped, the word
 *                  ends at a blank, a tab or the line's end without its CR; it may be empty).  Every other line behind the first
 *                  header is a sequence line: all of its bytes go into the text except blank, tab, CR and LF, a-z in upper case,
 *                  every other byte ('N', '*', '-', a '>' inside a line) as it is, for the byte rule above.  Lines before the first
 *                  header are ignored.  A header followed at once by a header or by the end of the file gives a sequence of length
 *                  0.  The sequences lie back to back in file order, seq_off as for asm_index_build.  ASM_EINVAL: a file that cannot
 *                  be opened, a file without a header line ("no sequence in <path>"), 2^26 sequences or more; ASM_EUNSUPPORTED: a
 *                  text of 2^32 - 1 bytes or more.  On an error *out is NULL.  The index does not depend on chunk_bytes.
 * asm_index_n_seqs, asm_index_seq_len, asm_index_seq_name, asm_index_get_text: what an index holds, from either call: its sequences,
 *                  the length of sequence r (0 when r is out of range), its name ("" for an index from asm_index_build or r out of
 *                  range; valid until asm_index_free) and bytes [start, start + n) of the upper-cased text, by global offsets
 *                  (synchronous).
 * asm_fasta_cut:   how much of buf[0, nbytes) the reader ships as one chunk: all of it, unless its last line is a header line still
 *                  without its newline, then the bytes in front of that line; at_line_start: buf[0] begins a line; *ends_in_line:
 *                  the shipped prefix ends inside a line (the next buffer's at_line_start is then 0).  No device.
 * ASM_FASTA_TILE:  the bytes one workgroup of the parser takes, 16 per thread: where the parser's edges are. */
#define ASM_FASTA_TILE 4096
typedef struct asm_index_file_stats {
    int64_t n_seqs, bases, bytes_in, chunks;     /* sequences; text length; file bytes; file chunks */
    double seconds, seconds_read, seconds_index; /* whole call; reader busy; k-mer keys + sort + bucket offsets */
} asm_index_file_stats;
int asm_index_build_file(asm_handle* h, const char* fasta_path, int k, int64_t chunk_bytes, asm_index** out,
                         asm_index_file_stats* stats /* may be NULL */);
int32_t asm_index_n_seqs(const asm_index* ix);
uint64_t asm_index_seq_len(const asm_index* ix, int32_t r);
const char* asm_index_seq_name(const asm_index* ix, int32_t r);
int asm_index_get_text(asm_handle* h, const asm_index* ix, uint64_t start, uint64_t n, char* dst);
size_t asm_fasta_cut(const char* buf, size_t nbytes, int at_line_start, int* ends_in_line);

/* ---- plain device memory helpers (so that non-torch hosts can drive the async API) --------------------- */
int asm_device_malloc(asm_handle* h, size_t bytes, void** d_ptr);
int asm_device_free(asm_handle* h, void* d_ptr);
int asm_memcpy_d2h(asm_handle* h, void* dst, const void* d_src, size_t bytes);
int asm_memcpy_h2d(asm_handle* h, void* d_dst, const void* src, size_t bytes);
int asm_memset_async(asm_handle* h, void* d_ptr, int value, size_t bytes);

/* ---- timing helper: HIP events on the handle's stream (bench.py measures kernels with these) ----------- */
int asm_timer_create(asm_handle* h, void** timer);
int asm_timer_start(asm_handle* h, void* timer);
int asm_timer_stop(asm_handle* h, void* timer);
int asm_timer_elapsed_ms(asm_handle* h, void* timer, float* ms); /* synchronises on the stop event */
int asm_timer_destroy(asm_handle* h, void* timer);

#ifdef __cplusplus
}
#endif
#endif /* ASM_MI355X_H */
