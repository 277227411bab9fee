/*
 * deepmod_hip.h — C ABI of libdeepmod_hip.so: the MI355X (gfx950) implementation of DeepMod's
 * per-read BiLSTM modification-calling hot path and its per-position summary.
 *
 * Plain pointers and sizes only.  Every function returns 0 on success or a negative DM_E* code;
 * the message of the last failure on the calling thread is available from dm_last_error().
 * A handle is single-owner (one process per GPU, as the reference runs one TF session per
 * process: bin/DeepMod_scripts/myDetect.py:948-956, :1177-1180); calls are synchronous on return
 * unless the name says _async.  The caller owns every buffer it passes; the library keeps no host
 * pointer after a call returns.
 *
 * Reference interfaces replaced (all under /root/reference/):
 *   dm_model_create / dm_model_destroy
 *        myMultiBiRNN.mCreateSession            bin/DeepMod_scripts/myMultiBiRNN.py:21-91
 *        tf.Session + Saver.restore             bin/DeepMod_scripts/myDetect.py:950-956
 *   dm_predict_windows
 *        sess.run([mfpred], feed_dict={X, Y})   bin/DeepMod_scripts/myDetect.py:814-820
 *        (graph: myMultiBiRNN.py:38-61; prediction=softmax :59, mfpred=argmax :61)
 *   dm_predict_read
 *        window assembly tx[mind-10:mind+11]    bin/DeepMod_scripts/myDetect.py:794-803
 *        + the sess.run above, fused on device
 *   dm_summary_create / _add / _add_read / _fetch / _destroy
 *        sum_handler's per-base accumulation    bin/DeepMod_scripts/myDetect.py:1089-1100
 *   dm_comm_create / dm_summary_reduce / dm_comm_destroy
 *        cross-process additive merge           DeepMod_tools/sum_chr_mod.py:47-52
 *        (the reference merges BED files of separate runs; here: one RCCL reduce per contig x strand)
 *   dm_cluster_create / _predict / _destroy
 *        cluster MLP sess.run([output])         DeepMod_tools/hm_cluster_predict.py:94-103, :158-164
 *   dm_cluster_sites / _sites_fetch / dm_cluster_bed_format
 *        merged rows with mod > 0               DeepMod_tools/sum_chr_mod.py:37-66
 *        CpG hits of the reference sequence     DeepMod_tools/generate_motif_pos.py:30-72
 *        readpredmod + the 14 features + write  DeepMod_tools/hm_cluster_predict.py:43-72, :128-154, :165-171
 */
#ifndef DEEPMOD_HIP_H
#define DEEPMOD_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DM_OK 0
#define DM_EINVAL (-1)   /* bad argument */
#define DM_EDEVICE (-2)  /* HIP runtime error / no gfx950 device */
#define DM_ENOMEM (-3)   /* allocation failed */
#define DM_ESTATE (-4)   /* handle in wrong state */
#define DM_ERCCL (-5)    /* RCCL could not be loaded or failed */
#define DM_ERANGE (-6)   /* DM_PREC_F16X3 met an input it cannot represent; the call's results are invalid, repeat with DM_PREC_F32 */

/* model geometry fixed by the shipped checkpoints */
#define DM_NFEAT 7
#define DM_HIDDEN 100
#define DM_WINDOW 21
#define DM_LAYERS 3
#define DM_WEIGHT_FLOATS 408402

/* dm_model_set_option keys */
#define DM_OPT_PROFILE 1   /* 1: bracket every kernel launch with HIP events on the model's stream */
#define DM_OPT_PRECISION 2 /* DM_PREC_*; default DM_PREC_F16X3 */
#define DM_OPT_ASYNC 3     /* 1: dm_predict_* with device-resident buffers return after enqueue on the model's stream;
                              wait with dm_model_sync.  Default 0: every call is synchronous on return. */
#define DM_OPT_RESERVED_CUS 4 /* n in [0, CUs / 2]: the classifier's persistent grid uses CUs - n workgroups (one per CU), so that
                              small kernels of OTHER streams (the signal stage of the streaming worker) run beside a classifier
                              launch instead of waiting for it to drain.  Default 0. */
#define DM_OPT_F16X3_SHAPE 5  /* MFMA shape of the DM_PREC_F16X3 / DM_PREC_F16I8 kernels.  16 = the product (v_mfma_f32_16x16x32_f16 and
                              v_mfma_i32_16x16x64_i8, csrc/lstm_f16q.hip.inc); 32 (v_mfma_f32_32x32x16_f16 / v_mfma_i32_32x32x32_i8: the kernels of
                              rounds 2-3, ~8 % / ~5 % slower, tools/experiments/f16s since round 6) exists only in an experiment build
                              (DM_WITH_F16S=1, DM_INFO_HAS_F16S) - a product library answers 32 with DM_EINVAL.  Same arithmetic, another
                              summation order: results differ in the last bits.  A model whose DM_PREC_F16I8 was selected by
                              dm_model_calibrate_i8 goes back to DM_PREC_F16X3 when the shape changes (the gate saw the other kernel). */
#define DM_PREC_F32 0      /* fp32 MFMA (v_mfma_f32_16x16x4_f32): fp32 products, the TF graph's own arithmetic */
#define DM_PREC_F16X3 1    /* split-f16 MFMA: every fp32 operand = hi + lo f16, 3 products per fp32 product, fp32
                              accumulation; max |dp| vs the oracle 1e-6 .. 2e-6 (tolerance of the path: 1e-4), ~3x faster.
                              Step-major kernel: weights and feature rows in, logits out, the state of the three layers never
                              leaves the chip: csrc/lstm_f16q.hip.inc on v_mfma_f32_16x16x32_f16.
                              Range contract (nothing is clamped silently):
                                * weights: every kernel / bias value times its exponent scale (<= 2.886) must be a finite f16
                                  (|w| <~ 22,700).  A model that violates this is created with DM_PREC_F32 as its default and
                                  dm_model_set_option(DM_OPT_PRECISION, DM_PREC_F16X3) returns DM_EINVAL.
                                * inputs: features 0..5 |x| <= 65504; feature 6 (event length, a raw sample count: reference
                                  myDetect.py:894-900) |x| <= 65504 * 2^k, k = DM_INFO_F16_LENGTH_SHIFT (10 for ordinary weights):
                                  beyond 65504 it is fed as x * 2^-k against a weight row stored x 2^k (exact rescale).
                                  An input outside these bounds (or NaN) makes the call fail with DM_ERANGE - synchronous
                                  calls on return, DM_OPT_ASYNC calls at the next dm_model_sync. */
#define DM_PREC_F16X3_ROLES 2 /* EXPERIMENT (round 4, tools/experiments/f16r): the arithmetic of DM_PREC_F16X3, bit for bit, with the work of a
                              SIMD split between a matrix wave and a cell wave (two waves per SIMD, accumulators and h handed over
                              through LDS): 6 % fewer cycles, the same time per launch - the part runs this path at its power limit and
                              gives a saved cycle back as a lower clock (profiles/r04/README.md).  Not part of the product build:
                              selectable only in a library built with -DDM_WITH_F16X3_ROLES (DM_INFO_HAS_F16X3_ROLES), otherwise
                              refused with DM_EINVAL. */
#define DM_PREC_F16I8 3    /* OPT-IN: the step-major kernel with hi*hi in f16 and BOTH cross terms of every product as one int8 MFMA
                              (v_mfma_i32_16x16x64_i8 since round 5, v_mfma_i32_32x32x32_i8 with DM_OPT_F16X3_SHAPE = 32; int32
                              accumulation, folded into the fp32 pre-activations per tile): 2 issued matrix units per product instead
                              of 3, 8-9 % less time per window than the default.  Operands carry ~19 bits instead
                              of 22.  REDUCED PRECISION: on 10^6 windows at weight scale 4 the worst window is 1.1e-4 from the fp32
                              graph, 2 windows exceed the path's 1e-4 tolerance and 99.99 % are below 6.5e-5 (DM_PREC_F16X3: worst
                              9e-6); at weight scale 1: 6e-6.  Documented bound 2e-4; classes equal wherever p1 is further than that
                              from 0.5.  Same range contract as DM_PREC_F16X3 (the raw features never ride the int8 product).
                              Never selected by default - neither by the library nor by the command line; opt-in per model through
                              dm_model_calibrate_i8 below (the command line: DEEPMOD_PRECISION=auto). */
/* dm_model_get_info keys */
#define DM_INFO_PRECISION 1          /* DM_PREC_* in effect */
#define DM_INFO_F16_REPRESENTABLE 2  /* 1 if the weights fit DM_PREC_F16X3 */
#define DM_INFO_F16_LENGTH_SHIFT 3   /* k above */
#define DM_INFO_DEVICE 4
#define DM_INFO_HAS_F16X3_ROLES 5    /* 1 if the library was built with the wave-pair experiment kernel */
#define DM_INFO_HAS_F16S 6           /* 1 if the library was built with the 32x32x16 kernels of rounds 2-3 (experiment builds: DM_WITH_F16S=1) */
#define DM_INFO_GRID_CAP 7           /* most workgroups a classifier launch may use: the device's CUs minus DM_OPT_RESERVED_CUS */
#define DM_INFO_LAST_GRID 8          /* workgroups of the last classifier launch of this model (0 before the first).  A workgroup b of a grid g
                                        over T = ceil(n / 128) tiles runs the work items b, b + g, b + 2 g, ... < 2 T; item w is tile w / 2 in
                                        direction w % 2 (0 forward, 1 backward).  Read-only: what the tests derive items per workgroup from. */

typedef struct dm_model dm_model;
typedef struct dm_summary dm_summary;

const char* dm_last_error(void);
const char* dm_version(void);

/* "experiment=0 switches=0" for the product; "experiment=1 ..." for a library built with -DDM_EXPERIMENT (tools/ablate.py: timing-only
 * kernels).  Any ablation macro without -DDM_EXPERIMENT is a compile error.  dm_version() also names the HIP / clang version the
 * library was compiled with (the hand-scheduled kernels are validated per compiler).  No reference counterpart. */
const char* dm_build_flags(void);

/* number of visible gfx950 devices (0 if none / HIP unusable) */
int dm_device_count(void);
/* PCI bus id ("0000:05:00.0") of HIP device `device` into buf (>= 13 bytes): the key under /sys/bus/pci/devices/ where the driver
 * publishes the device's socket power and clocks (deepmod_amd/powerlog.py, bench.py roofline.power).  No reference counterpart. */
int dm_device_pci_bus_id(int device, char* buf, int len);

/*
 * Build a model on `device` from the canonical flat weight blob (DM_WEIGHT_FLOATS floats, host):
 *   for d in (fw, bw): for l in 0..2: kernel[K_l][400] row-major (K_0 = 107, else 200; columns
 *   i|j|f|o as TF BasicLSTMCell), bias[400];  then head W[200][2], head b[2].
 * The forget bias (+1.0) is NOT pre-added by the caller.  Returns NULL on failure.
 */
dm_model* dm_model_create(int device, const float* weights, size_t n_floats, int n_feat, int hidden,
                          int window, int layers);
void dm_model_destroy(dm_model* m);
int dm_model_set_option(dm_model* m, int key, int64_t value);
int dm_model_get_info(dm_model* m, int key, int64_t* value);
/*
 * Load-time calibration gate of the opt-in int8 mode (round 4; no reference counterpart - the reference runs fp32 TensorFlow kernels,
 * myMultiBiRNN.py:38-61).  Classifies n_windows synthetic windows generated on the device (the same on every box; alternating batches
 * of 65,536: the BASELINE configs[1] distribution, and - round 5 - a read-shaped tail draw: event means over the whole +-5 clip range
 * with 6 % exactly on the clip, standard deviations up to 9x, event lengths log-uniform 1 .. 30,000 samples) with DM_PREC_F32 and with
 * DM_PREC_F16I8 and reports the largest |p(f32) - p(f16i8)| in *max_abs_dp.  If that is <= bound and the model currently runs
 * DM_PREC_F16X3, DM_PREC_F16I8 becomes its precision.  *selected = 1 if the model runs DM_PREC_F16I8 after the call (also when it
 * already did), else 0; a model that does not run it afterwards does not keep the int8 weight pack.  What the mode's error is depends
 * on the weights: 1.2e-5 in the tail of 10^6 windows for weights with trained statistics, 7e-5 - 1.1e-4 for U(-a, a) kernels at scale 4
 * (profiles/r04/i8_tail.txt) - hence a gate per model, never a global default.  10^6 windows take ~0.12 s.  Synchronises the model's stream.
 */
int dm_model_calibrate_i8(dm_model* m, int64_t n_windows, double bound, double* max_abs_dp, int* selected);

/*
 * Classify n windows.  x: [n][21][7] fp32 C-contiguous, host OR device memory (detected).
 * prob: [n][2] fp32 or NULL; cls: [n] u8 (argmax, ties -> 0) or NULL; each may be host or device.
 * n == 0 is a no-op.
 */
int dm_predict_windows(dm_model* m, const float* x, int64_t n, float* prob, uint8_t* cls);

/*
 * Classify `count` consecutive windows of one read: window i is rows[first+i-10 .. first+i+10]
 * of the per-read feature matrix rows [m][7] (fp32, host or device); the caller guarantees
 * first-10 >= 0 and first+count+10 <= m (DeepMod pads 100 rows each side).  Windows are
 * assembled on the device.
 */
int dm_predict_read(dm_model* m, const float* rows, int64_t m_rows, int64_t first, int64_t count,
                    float* prob, uint8_t* cls);

/*
 * Classify `count` windows of the feature-row matrix picked by their CENTRE rows: window i = rows[centre[i]-10 .. centre[i]+10]
 * (10 <= centre[i] < m_rows - 10; checked for host arrays only).  The streaming worker classifies only the windows centred on
 * a base of interest: sum_handler tests refbase == Base before it looks at mod_pred (myDetect.py:1091-1100), so the class of
 * every other window never reaches the BED - on E. coli 5mC that is 3 of 4 windows.  The reference
 * computes them because it stores per-read tables; `--storePred 1` (dm_predict_read) still does.  prob / cls: [count].
 */
int dm_predict_read_at(dm_model* m, const float* rows, int64_t m_rows, const int32_t* centre, int64_t count, float* prob,
                       uint8_t* cls);

/* block until all work queued on the model's stream has finished; reports a pending DM_ERANGE of asynchronous launches */
int dm_model_sync(dm_model* m);

/* profiling (DM_OPT_PROFILE=1): summed HIP-event time and launch count of the BiLSTM kernel since
 * the last reset; dm_profile_get synchronises the stream first. */
int dm_profile_reset(dm_model* m);
int dm_profile_get(dm_model* m, double* kernel_ms, int64_t* launches, int64_t* windows);

/* device-memory helpers so a host language without a HIP binding can keep inputs resident */
void* dm_device_alloc(int device, size_t bytes);
int dm_device_free(int device, void* p);
int dm_memcpy_h2d(int device, void* dst, const void* src, size_t bytes);
int dm_memcpy_d2h(int device, void* dst, const void* src, size_t bytes);
/* host -> device copy queued on the model's stream (ordered with its launches; with DM_OPT_ASYNC a worker refills its
 * staging buffers without waiting for the device).  src must stay valid until the next dm_model_sync. */
int dm_model_h2d_async(dm_model* m, void* dst, const void* src, size_t bytes);
/* The same copy on the model's copy stream: it does NOT wait for the launches already queued (it runs while they compute) and
 * every launch queued after this call waits for it.  The caller guarantees that no queued launch touches dst - in the staging
 * scheme below: dm_model_wait_mark of the set has returned.  src must stay valid until the set's next marker has passed. */
int dm_model_h2d_ahead(dm_model* m, void* dst, const void* src, size_t bytes);
/* Page-locked host staging memory (hipHostMalloc) and stream markers for a pipelined worker: batch k is copied into staging
 * set k % N while the device still works on batch k - 1; dm_model_mark(m, i) records a marker on the model's stream after the
 * launches that read set i, dm_model_wait_mark(m, i) blocks the host until that marker has passed (at once if it was never
 * recorded).  DM_ERANGE is tracked per marker: wait_mark(i) reports exactly the launches queued between the marker recorded before i and
 * marker i - a later batch still in flight is neither reported early nor cleared; dm_model_sync reports everything outstanding.  i in [0, DM_MARKS).
 * A marker recorded again before anybody waited for it leaves its earlier launches to dm_model_sync.  The library tracks 2 DM_MARKS + 2 such ranges: when
 * markers are recorded that often without a wait, a further dm_model_mark(i) still orders host and device, but dm_model_wait_mark(i) reports nothing - the
 * launches before it are reported by a later marker or by dm_model_sync instead, exactly once (tests/test_gpu_range_contract.py).  No reference counterpart:
 * the reference feeds numpy arrays to session.run (myDetect.py:796-822). */
#define DM_MARKS 8
void* dm_host_alloc(int device, size_t bytes);
int dm_host_free(int device, void* p);
int dm_model_mark(dm_model* m, int i);
int dm_model_wait_mark(dm_model* m, int i);

/* ------------------------------------------------------------------ per-position summary -- */
/*
 * Dense per-position counters for one contig x strand of `length` reference positions:
 * touch (rows with refbase == Base: the reference creates the BED key before testing
 * readbase, myDetect.py:1093-1094), cov (readbase != '-'), mod (mod_pred == 1), all int32.
 */
dm_summary* dm_summary_create(int device, int64_t length);
void dm_summary_destroy(dm_summary* s);
int64_t dm_summary_length(const dm_summary* s);

/* flags bit0: refbase == Base (and not '-','N','n'); bit1: readbase != '-'; bit2: mod_pred == 1.
 * pos / flags: [n], host or device. */
int dm_summary_add(dm_summary* s, const int64_t* pos, const uint8_t* flags, int64_t n);
/* same, with bit2 taken from the classifier output cls[i] == 1 (the per-base scatter of
 * myDetect.py:829-831 fused with the accumulation); flags' own bit2 is ignored. */
int dm_summary_add_classified(dm_summary* s, const int64_t* pos, const uint8_t* flags, const uint8_t* cls,
                              int64_t n);
int dm_summary_sync(dm_summary* s);

/* grow the counters to new_length positions (existing counts kept, new positions zero); no-op if not larger */
int dm_summary_grow(dm_summary* s, int64_t new_length);

/* ---- multi-GPU: one process per GPU, a persistent RCCL communicator, one integer reduce per contig x strand -----
 * Reads shard across processes with no data-path collective; the only exchange is the additive merge of the
 * per-position counters at the end (what the reference does across runs with DeepMod_tools/sum_chr_mod.py:47-52).
 *   dm_rccl_unique_id   rank 0 obtains 128 bytes and hands them to the other ranks out of band (deepmod_amd/comm.py:
 *                       a file in the run's output folder; any byte channel works)
 *   dm_comm_create      collective: every rank calls it once with the same id; the communicator lives until
 *                       dm_comm_destroy and serves any number of reduces
 *   dm_summary_reduce   in-place int32 sum of touch|cov|mod over all ranks.  root >= 0: ncclReduce, result valid on
 *                       `root` only; root < 0: ncclAllReduce.  All ranks call it with summaries of equal length, in
 *                       the same order.  Integer sums are order independent: the BED is the same for any GPU count.
 *   dm_comm_max_f64 / dm_comm_barrier   small host-synchronous helpers (timing max over ranks, rendezvous)
 *   dm_comm_stats       collectives issued and bytes reduced by this rank so far
 * The collective library is bound at the first call (dlopen): librccl by soname, or the file DEEPMOD_RCCL_LIBRARY names - a site
 * build of RCCL, or the shared-memory test transport tests/shim/shmccl.cpp that lets several ranks share one device (RCCL refuses
 * that), which is how the N > 1 calls below are tested on a one-GPU box.  A path that cannot be loaded is an error (DM_ERCCL). */
typedef struct dm_comm dm_comm;
int dm_rccl_unique_id(void* out128);
/* the collective library this process bound (path the loader mapped, ncclGetVersion code; loads it on first use) */
int dm_rccl_info(char* path, int path_len, int* version);
dm_comm* dm_comm_create(int device, const void* unique_id128, int rank, int nranks);
void dm_comm_destroy(dm_comm* c);
int dm_comm_rank(const dm_comm* c);
int dm_comm_size(const dm_comm* c);
int dm_comm_barrier(dm_comm* c);
int dm_comm_max_f64(dm_comm* c, double* value);
int dm_comm_stats(const dm_comm* c, int64_t* collectives, int64_t* bytes);
int dm_summary_reduce(dm_summary* s, dm_comm* c, int root);
/*   dm_summary_reduce_scatter   the merge that scales (the reference's per-process BED files + sum_chr_mod.py:47-63 turned
 *                       inside out): positions are cut into nranks slices of ceil(length / nranks); afterwards THIS rank holds the
 *                       all-rank sums of its slice [*first, *first + *count) (count 0 for a rank past the end) - one ncclReduceScatter
 *                       (int32 sum) per counter array.  Each rank then fetches and formats only its slice (dm_summary_fetch_slice,
 *                       dm_bed_format_at) and the parts are concatenated in rank order.  Collective, nranks <= 64.
 *   dm_summary_fetch_slice      that slice: *count int32 each (any may be NULL) */
int dm_summary_reduce_scatter(dm_summary* s, dm_comm* c, int64_t* first, int64_t* count);
int dm_summary_fetch_slice(dm_summary* s, int32_t* touch, int32_t* cov, int32_t* mod);

/* copy counters to host arrays of `length` int32 each (any may be NULL) */
int dm_summary_fetch(dm_summary* s, int32_t* touch, int32_t* cov, int32_t* mod);
/* raw device pointers (3 * length int32: touch | cov | mod) for callers that run their own collective */
void* dm_summary_device_ptr(dm_summary* s);
/* Enqueue this summary's device-resident adds on model m's stream, i.e. in order with its classifier launches (with
 * DM_OPT_ASYNC the host then never waits between classify and accumulate, and the out-of-range check of those adds is
 * reported by the next dm_summary_sync / dm_summary_fetch instead); m = NULL detaches.  Detach or destroy the summary
 * before destroying the model. */
int dm_summary_follow(dm_summary* s, dm_model* m);

/* BED text of one contig x strand from the (host) counters, byte for byte what sum_handler writes (myDetect.py:1107-1120):
 * one line per position with touch > 0, "<chr> <pos> <pos+1> <Base> <min(cov,1000)> <strand> <pos> <pos+1> 0,0,0 <cov> <pct> <mod> \n".
 * Returns the length of the text.  With out == NULL or cap below the safe bound (lines * (strlen(chrom) + 128)) nothing is written and
 * that bound is returned: allocate it and call again. */
int64_t dm_bed_format(const char* chrom, char strand, char base, const int32_t* touch, const int32_t* cov, const int32_t* mod,
                      int64_t length, char* out, int64_t cap);
/* the same for counters of positions [first_pos, first_pos + length): a rank's slice of the text (myDetect.py:1112-1120 is sorted by
 * position, so the ranks' parts concatenated in rank order are the file) */
int64_t dm_bed_format_at(const char* chrom, char strand, char base, int64_t first_pos, const int32_t* touch, const int32_t* cov,
                         const int32_t* mod, int64_t length, char* out, int64_t cap);

/* ------------------------------------------------------------- CpG cluster second stage -- */
/*
 * MLP 14 -> 100 (relu) -> 20 (relu) -> 1 (sigmoid) of DeepMod_tools/hm_cluster_predict.py:94-103,:161
 * (graph nodes X, W_1/b_1, W_2/b_2, W_O/b_O, output; dropout with keep_prob = 1 is the identity).
 * weights: 3541 floats = W_1[14][100], b_1[100], W_2[100][20], b_2[20], W_O[20][1], b_O[1] (host).
 * x: [n][14] fp32, out: [n] fp32; host or device pointers.
 */
#define DM_CLUSTER_WEIGHT_FLOATS 3541
typedef struct dm_cluster dm_cluster;
dm_cluster* dm_cluster_create(int device, const float* weights, size_t n_floats);
void dm_cluster_destroy(dm_cluster* c);
int dm_cluster_predict(dm_cluster* c, const float* x, int64_t n, float* out);

/* The cluster stage of one contig (or one rank's slice of it) from the counters where they are - no BED text in between.  Replaces
 * sum_chr_mod.py:37-66 (rows with mod > 0 of both strands, pct = int(mod * 100 / cov)), generate_motif_pos.py:30-72 (CpG hits: '+' at p where
 * the upper-cased sequence reads "CG" at p, '-' at p + 1) and hm_cluster_predict.py:43-72, :128-154 (the sites = rows on a hit; per site
 * [frac, partner frac, n, 11-bin histogram / n] over the sites within +-25 bp, double arithmetic, cast to fp32), then runs the MLP above
 * on the device feature rows.
 *   plus, minus  the '+' and '-' counters of the contig; either may be NULL (all zero)
 *   from_slice   0: the whole tables; positions [first, first + count) of them are the range (beyond a table's length: zero)
 *                1: each summary's slice after dm_summary_reduce_scatter, which must be [first, first + count)
 *   seq          host bytes of positions [seq_first, seq_first + seq_len), any case; positions outside hold no base.  A slice needs its own
 *                positions +-27
 *   halo         int32 [2 sides][2 strands][cov | mod][26]: the counters of positions first - 26 .. first - 1 (side 0) and
 *                first + count .. first + count + 25 (side 1) - sites there are neighbours and partners, never output.  NULL: whole tables
 *                are read beside the range themselves; beside a slice the counters are zero
 * Returns the number of sites (< 0: error code); *n_plus of them are '+' sites.  Rows are ordered as the reference's file: '+' sites
 * ascending, then '-' sites ascending.  The results stay on the device until the next call:
 *   dm_cluster_sites_fetch   position, cov, mod, new = int(float32 p * 100) (hm_cluster_predict.py:170) and the [n][14] fp32 features per
 *                            site (any may be NULL)
 *   dm_cluster_bed_format    (host) the file's lines for n records of one strand: sum_chr_mod.py:63's row - two spaces after the strand,
 *                            no trailing space - + " <new>\n".  Sized first like dm_bed_format_at; positions < 2^40 */
int64_t dm_cluster_sites(dm_cluster* c, dm_summary* plus, dm_summary* minus, int from_slice, const uint8_t* seq, int64_t seq_first, int64_t seq_len,
                         int64_t first, int64_t count, const int32_t* halo, int64_t* n_plus);
int dm_cluster_sites_fetch(dm_cluster* c, int64_t* pos, int32_t* cov, int32_t* mod, int32_t* new_pct, float* features);
int64_t dm_cluster_bed_format(const char* chrom, char strand, char base, const int64_t* pos, const int32_t* cov, const int32_t* mod,
                              const int32_t* new_pct, int64_t n, char* out, int64_t cap);

/* ---- raw-signal normalisation + per-event statistics ------------------------------------
 * Replaces myDetect.py:266-282 (mnormalized: median / MAD shift-scale over the event-covered slice, second
 * median / MAD, clip to +-5 MAD, round to 3 decimals) and :332-343 (per-event round(np.mean, 3), round(np.std, 3)
 * into the '<f4' fields of m_event).  Results are bit-identical to numpy's (same float64 operations in the same
 * order, including np.add.reduce's 8,192-element buffers and 8-lane pairwise sums).
 *   raw        int16 DAC samples [n_raw] (FAST5 Raw/Reads/.../Signal), host or device (device: 16-byte aligned)
 *   ev_start / ev_length  uint64 [n_events] host arrays (m_event['start'], m_event['length'])
 *   ev_mean / ev_stdv     float [n_events] host outputs; NaN for an event whose slice is empty
 *   norm6      optional double[6]: mshift, mscale, read_med, read_mad, lower_lim, upper_lim
 *   first_empty optional: index of the first event with an empty slice (the reference stops its loop there,
 *              :334-340), n_events if none
 *   normalized optional double [n_raw] (host or device): the normalised signal itself */
typedef struct dm_signal dm_signal;
dm_signal* dm_signal_create(int device);
void dm_signal_destroy(dm_signal* s);
int dm_signal_event_stats(dm_signal* s, const int16_t* raw, int64_t n_raw, const uint64_t* ev_start,
                          const uint64_t* ev_length, int64_t n_events, float* ev_mean, float* ev_stdv, double* norm6,
                          int64_t* first_empty, double* normalized);

/* Many reads per call (a typical 120 k-sample read is launch / latency bound when it travels alone): the reads' samples back to
 * back in raw (read r = raw[raw_off[r] .. raw_off[r+1])), event tables back to back (events of read r = [ev_off[r], ev_off[r+1]),
 * starts relative to the read's first sample); norm6 [n_reads][6] and first_empty [n_reads] optional.  Host arrays only.
 * Bit-identical to n_reads calls of dm_signal_event_stats. */
int dm_signal_event_stats_batch(dm_signal* s, int64_t n_reads, const int16_t* raw, const int64_t* raw_off, const uint64_t* ev_start,
                                const uint64_t* ev_length, const int64_t* ev_off, float* ev_mean, float* ev_stdv, double* norm6,
                                int64_t* first_empty);

/* The RESIDENT form (round 6; SURVEY 8f1 + 8f3: "fuse get_Feature's output rows straight into the kernel"): the per-event statistics never leave the
 * device.  dm_signal_plan_batch (host only, no device call) makes the checks of the batched call and returns first_empty [n_reads] - all a feeder needs
 * from the signal stage before it walks its alignments (myDetect.py:334-340 cuts the event table there).  dm_signal_event_stats_device runs the same
 * four kernels and writes d_ev3 [n_events][3] = (mean, stdv, length) of every merged event of the batch into a device block of the caller - the three
 * values get_Feature (:892-900) copies into a feature row - with the basecaller's values (fb_mean / fb_stdv, host, may be NULL when no read has an empty
 * event) merged in for events at or behind first_empty.  dm_rows_emit_resident's descriptors index that block and dm_rows_assemble reads it in place: no
 * D2H -> feeder -> H2D of the statistics.  The block is complete when the call returns; host arrays should be page-locked (dm_host_alloc).
 * flags (optional): bit 0 = a mean or stdv the call computed (an event before its read's first_empty) is outside the split-f16 kernels' range (the batch
 * then takes DM_PREC_F32).  Lengths and fall-back values are host data: dm_rows_emit_resident's in_range covers them for the events rows show, so an
 * event no row shows decides the kernel in neither form. */
int dm_signal_plan_batch(int64_t n_reads, const int64_t* raw_off, const int64_t* ev_off, const uint64_t* ev_start, const uint64_t* ev_length,
                         int64_t* first_empty);
int dm_signal_event_stats_device(dm_signal* s, int64_t n_reads, const int16_t* raw, const int64_t* raw_off, const uint64_t* ev_start,
                                 const uint64_t* ev_length, const int64_t* ev_off, const int64_t* first_empty, const float* fb_mean, const float* fb_stdv,
                                 float* d_ev3, double* norm6, int32_t* flags);

/* The resident form for reads with MOVE TABLES (detect --move): the event tables are built on the device.  move / mv_off / first as dm_move_events takes
 * them (batch-wide), ev_off [n_reads + 1] = the cumulative Fastq lengths (the event count every read must have).  A segmentation pass (per-chunk boundary
 * counts, a scan per read, one store per boundary) writes the handle's (start, length) tables, then the kernels of dm_signal_event_stats_device run
 * unchanged on the same stream; a read's normalisation slice is [first, samples).  status [n_reads] (host, out) = dm_move_events' status of every read,
 * computed on the device: a read with a non-zero status writes nothing outside its own slots and contributes no statistics (its rows of d_ev3 are
 * NaN, NaN, 0).  Every read needs at least one sample and the batch at least one expected event.  flags: as dm_signal_event_stats_device.
 * dm_signal_move_chunk: table bytes one workgroup of the segmentation kernels takes (a read's chunks start at its table's 16-byte-aligned base). */
int dm_signal_move_stats_device(dm_signal* s, int64_t n_reads, const int16_t* raw, const int64_t* raw_off, const uint8_t* move, const int64_t* mv_off,
                                const int64_t* first, const int64_t* ev_off, float* d_ev3, int32_t* status, double* norm6, int32_t* flags);
int64_t dm_signal_move_chunk(void);

/* ---- SAM record -> per-base alignment table (host code, no GPU needed) ---------------------
 * Replaces the alignment walk of handle_record, myDetect.py:515-714: clip stripping, one row per M/I/D/N/=/X
 * position, first/last-match trimming of table and event slice, '-' strand flip + complement, the CpG gap swap.
 *   flag, pos1, cigar, readseq     fields 2, 4, 6, 10 of the SAM line (pos1 is 1-based)
 *   refseq                         the whole (upper-cased) reference sequence of RNAME
 *   n_events                       len(f5data[readk][1]) (events of the read, one per basecalled base)
 *   refbase/readbase/refbasei/readbasei   caller-allocated columns of base_map_info (dtype :660), cap_rows rows
 *   info[DM_MAP_INFO_LEN]          see DM_MAP_* below
 * Returns 0 and info[DM_MAP_STATUS] = DM_MAP_OK | DM_MAP_NO_MATCH (read skipped, :617-622) | DM_MAP_NEED_ROWS
 * (cap_rows < info[DM_MAP_N_ROWS]; nothing written), or a negative code for a CIGAR that is malformed or runs
 * past the read / reference (the reference raises IndexError there). */
#define DM_MAP_INFO_LEN 16
#define DM_MAP_STATUS 0
#define DM_MAP_N_ROWS 1
#define DM_MAP_LEFTCLIP 2            /* after the strand swap of :667 = start_clip of get_Feature / mPredict1 */
#define DM_MAP_RIGHTCLIP 3           /* = end_clip */
#define DM_MAP_EV_LO 4               /* m_event = events[EV_LO:EV_HI] after both trimming steps */
#define DM_MAP_EV_HI 5
#define DM_MAP_FIRST_MATCH_POS 6
#define DM_MAP_LAST_MATCH_POS 7
#define DM_MAP_NUM_INSERT 8
#define DM_MAP_NUM_DELETE 9
#define DM_MAP_NUM_MISMATCH 10
#define DM_MAP_STRAND 11             /* 0 '+', 1 '-' */
#define DM_MAP_POS_AFTER_CLIP 12     /* 0-based position after the left clip (region filter of :544-553) */
#define DM_MAP_EVENTS_AFTER_CLIP 13  /* len(m_event) at that point */
#define DM_MAP_OK 0
#define DM_MAP_NO_MATCH 1
#define DM_MAP_NEED_ROWS 2
int dm_map_read(int flag, int64_t pos1, const char* cigar, const char* readseq, int64_t readseq_len,
                const char* refseq, int64_t refseq_len, int64_t n_events, char* refbase, char* readbase,
                uint64_t* refbasei, uint64_t* readbasei, int64_t cap_rows, int64_t* info);

/* ---- one worker batch of reads -> the device-ready arrays of the streaming detect (host code) ------------------------------
 * What the streaming worker uploads per batch: feature rows [R][7] fp32 (the reads' matrices back to back, 100 zero rows of
 * padding on both sides of every read - myDetect.py:850-851), per row a reference position and a flag byte (dm_summary_add_classified),
 * and "extra" (position, flag) pairs of table rows that own no window.  Replaces, per batch instead of per read:
 *   dm_events_merge     getEvent, Albacore-2 'simple' branch                           myDetect.py:237-251
 *   dm_rows_add_raw     handle_record's filters + alignment walk + get_Feature         myDetect.py:497-713, :839-903
 *   dm_rows_add_packed  the reads of a feature container (arguments of mPredict1)      myDetect.py:715
 *   dm_rows_info / dm_rows_emit   window <-> base association and per-base flags        myDetect.py:794-803, :824-833, :1089-1100
 * Per-read status codes (read_info[i][0]): */
#define DM_ROWS_OK 0
#define DM_ROWS_LESS_EVENT 1      /* fewer than 50 aligned events (:702-705) */
#define DM_ROWS_INDEX_ERROR 2     /* fewer aligned table rows than aligned events (the reference raises IndexError) */
#define DM_ROWS_NO_MATCH 3        /* no matching base (:617-622) */
#define DM_ROWS_CIGAR_ERROR 4
#define DM_ROWS_FILTERED 5        /* region filter / skipped by the caller */
#define DM_ROWS_NO_REFERENCE 6
#define DM_ROWS_NOT_MATCHING 7    /* raw reads: event bases differ from the table's read bases (:868-874) */
#define DM_ROWS_INFO 8            /* int64 per read: status, contig, strand (0 '+', 1 '-'), windows, rows, table rows, mismatches, extras */
typedef struct dm_rowsbatch dm_rowsbatch;
/* Container tables come from disk: every offset table is checked against the size of the arrays it indexes (n_events, n_tx_rows,
 * n_table_rows below), contigs against n_contigs, strands against {0, 1} - a damaged file is DM_EINVAL, never an out-of-bounds read
 * (tests/test_asan_host.py drives these functions, built with -fsanitize=address, with damaged tables). */
int64_t dm_events_merge(int64_t n_reads, int64_t n_events, const int64_t* ev_off, const double* mean, const double* stdv, const uint64_t* start,
                        const uint64_t* length, const uint32_t* model_state, int32_t ms_width, const int64_t* move, int64_t* mev_off,
                        float* m_mean, float* m_stdv, uint64_t* m_start, uint64_t* m_length, char* m_base);
/* getEvent with --move (myDetect.py:136-153, MoveTable.py:7-54): the event tables of a container's reads from their basecaller move tables (uint8, back
 * to back in `move`, read r = move[mv_off[r] .. mv_off[r+1])).  A boundary is every index i in 1 .. L-1 with move[i] == 1; event 0 starts at first[r]
 * (first_sample_template), boundary i starts the next event at first[r] + 2 i (the reference's stride, :30-33), the last event ends at the read's last
 * sample (raw_off[r+1] - raw_off[r] samples).  m_base is a copy of the Fastq bytes (fq, fq_off); a read has fq_off[r+1] - fq_off[r] events.  status[r]: */
#define DM_MOVE_OK 0
#define DM_MOVE_COUNT 1           /* boundaries != bases - 1: the reference is undefined (IndexError / uninitialised rows); decided first */
#define DM_MOVE_OUTSIDE 2         /* first < 0, first >= samples, or the last boundary at or behind the read's end: an event outside the signal */
/* A read with a non-zero status gets no events (mev_off[r+1] == mev_off[r]).  Outputs are sized for n_fq events.  Offsets are checked against
 * n_move / n_fq before anything is read.  -> events written, or a negative code.  dm_signal_move_stats_device computes the same tables on the device. */
int64_t dm_move_events(int64_t n_reads, int64_t n_move, const uint8_t* move, const int64_t* mv_off, const int64_t* first, const int64_t* raw_off,
                       int64_t n_fq, const char* fq, const int64_t* fq_off, int64_t* mev_off, int32_t* status, uint64_t* m_start, uint64_t* m_length,
                       char* m_base);
dm_rowsbatch* dm_rows_create(char base);
void dm_rows_destroy(dm_rowsbatch* h);
int dm_rows_add_packed(dm_rowsbatch* h, int64_t n_reads, int64_t n_tx_rows, int64_t n_table_rows, int64_t n_events, int32_t n_contigs,
                       const int64_t* row_off, const int64_t* bmi_off, const int64_t* ev_off,
                       const float* tx, const char* refbase, const char* readbase, const int64_t* refbasei, const char* evbase,
                       const int64_t* start_clip, const int64_t* end_clip, const int32_t* contig, const int32_t* strand);
int dm_rows_add_raw(dm_rowsbatch* h, int64_t n_reads, const int32_t* flag, const int64_t* pos1, const char* const* cigar,
                    const char* const* readseq, const int64_t* readseq_len, const int32_t* contig, const int32_t* ev_read,
                    const uint8_t* skip, int32_t n_contigs, const char* const* refseq, const int64_t* refseq_len,
                    int64_t n_event_reads, int64_t n_events, const int64_t* mev_off, const float* m_mean, const float* m_stdv, const uint64_t* m_length, const char* m_base,
                    const float* s_mean, const float* s_stdv, const int64_t* first_empty, int32_t n_region,
                    const int32_t* region_contig, const int64_t* region_lo, const int64_t* region_hi);
/* reads whose alignment table the caller already has (get_Feature's rows are built from the event tables at emit time) */
int dm_rows_add_mapped(dm_rowsbatch* h, int64_t n_reads, int64_t n_table_rows, int64_t n_events, int32_t n_contigs, const int64_t* bmi_off, const char* refbase, const char* readbase,
                       const int64_t* refbasei, const int64_t* start_clip, const int64_t* end_clip, const int32_t* contig,
                       const int32_t* strand, const int64_t* mev_off, const float* m_mean, const float* m_stdv, const uint64_t* m_length,
                       const char* m_base, const float* s_mean, const float* s_stdv, const int64_t* first_empty);
int64_t dm_rows_info(dm_rowsbatch* h, int64_t* n_rows, int64_t* n_pos, int64_t* n_sel, int64_t* read_info, int64_t* mism, int64_t cap_mism,
                     int64_t* n_mism);
#define DM_ROWS_GROUP 8           /* int64 per group: contig, strand, row_lo, row_hi, xlo, xhi, sel_lo, sel_hi */
int64_t dm_rows_emit(dm_rowsbatch* h, const int32_t* contig_rank, float* rows, int32_t* sel_row, int64_t* pos, uint8_t* flags,
                     int64_t* groups, int64_t cap_groups, int64_t* contig_len, int64_t n_contig_len, int32_t* in_range);
/* The DEVICE form of a batch of raw reads (round 5; SURVEY 8f1 "fuse get_Feature's rows into the kernel"): instead of rows [R][7] the host hands over
 * ev3 [E][3] = (mean, stdv, length) of the events the rows cover, code [R] (one-hot class of a row: 0..3 = A, C, G, T, 255 = none) and rdesc [reads][4]
 * = (first row, row -> event shift, first event, end event) - 13 instead of 28 bytes per row, no feature row written or range-scanned on the host -
 * and dm_rows_assemble builds the same [R][7] matrix on the device (get_Feature, myDetect.py:839-903, bit for bit: the values are copied, not computed).
 * dm_rows_device_info (after dm_rows_info): 1 if every emitted read is a raw read, with the sizes E and reads; dm_rows_emit_device: as dm_rows_emit. */
int dm_rows_device_info(dm_rowsbatch* h, int64_t* n_events, int64_t* n_reads);
int64_t dm_rows_emit_device(dm_rowsbatch* h, const int32_t* contig_rank, float* ev3, uint8_t* code, int64_t* rdesc, int32_t* sel_row, int64_t* pos,
                            uint8_t* flags, int64_t* groups, int64_t cap_groups, int64_t* contig_len, int64_t n_contig_len, int32_t* in_range);
/* The RESIDENT form (round 6): reads added by dm_rows_add_raw with s_mean == s_stdv == NULL and first_empty given (dm_signal_plan_batch) - their
 * statistics are the device block of dm_signal_event_stats_device.  No ev3: rdesc's event indices are positions in the batch's merged event tables
 * (= rows of that block); in_range covers the event lengths and the fall-back values, the signal stage reports the range of its own values. */
int64_t dm_rows_emit_resident(dm_rowsbatch* h, const int32_t* contig_rank, uint8_t* code, int64_t* rdesc, int32_t* sel_row, int64_t* pos, uint8_t* flags,
                              int64_t* groups, int64_t cap_groups, int64_t* contig_len, int64_t n_contig_len, int32_t* in_range);
int dm_rows_assemble(dm_model* m, float* d_rows, const uint8_t* d_code, const float* d_ev3, const int64_t* d_rdesc, int64_t n_reads, int64_t n_rows);

/* ------------------------------------------------------------------------- training -- */
/*
 * The other half of the reference: myMultiBiRNN.mCreateSession's loss_op / train_op (bin/DeepMod_scripts/myMultiBiRNN.py:21-91) and the
 * sess.run([train_op, loss_op]) of train_save_model (:190).  fp32 throughout; forward with a tape, backpropagation through the 11 live
 * steps of each direction, TF1 AdamOptimizer (lr 1e-3, beta1 0.9, beta2 0.999, eps 1e-8).  No float atomics: two runs are bit-identical.
 *   weights, grad, m, v   the canonical DM_WEIGHT_FLOATS layout of dm_model_create
 *   x [n][21][7], y [n][2]   host or device memory (detected); n <= max_batch, which sizes the tape once (158,400 B per window)
 *   unbalanced == 1       the loss (only) is taken of logits * [0.1, 0.9] (:64-67); prob stays softmax(logits)
 *   dm_trainer_grad       loss, prob [n][2] and the gradient blob (each of the last two may be NULL); the state does not change
 *   dm_trainer_adam       one Adam step from a caller-supplied gradient blob
 *   dm_trainer_step       grad + adam; nothing is downloaded but the loss
 *   dm_trainer_get_state / _set_state   weights, Adam slots m and v (any may be NULL) and the step count t
 * n == 0 is a no-op.  n > max_batch, NaN / Inf in x or y, or a non-finite loss return DM_EINVAL and leave the state unchanged.
 */
typedef struct dm_trainer dm_trainer;
dm_trainer* dm_trainer_create(int device, const float* weights, size_t n_floats, int n_feat, int hidden, int window, int layers, int64_t max_batch);
void dm_trainer_destroy(dm_trainer* t);
int dm_trainer_grad(dm_trainer* t, const float* x, const float* y, int64_t n, int unbalanced, float* loss, float* prob, float* grad);
int dm_trainer_adam(dm_trainer* t, const float* grad);
int dm_trainer_step(dm_trainer* t, const float* x, const float* y, int64_t n, int unbalanced, float* loss);
int dm_trainer_get_state(dm_trainer* t, float* weights, float* m, float* v, int64_t* step);
int dm_trainer_set_state(dm_trainer* t, const float* weights, const float* m, const float* v, int64_t step);
/* HIP events on the trainer's stream around every dm_trainer_step: reports the time summed and the steps counted since the last call (either may be
 * NULL), then switches the bracketing on or off and clears both (tools/train_rate.py).  No reference counterpart. */
int dm_trainer_profile(dm_trainer* t, int on, double* step_ms, int64_t* steps);

/* ------------------------------------------------------- training the CpG-cluster model -- */
/*
 * The training graph the reference ships with its cluster checkpoint (train_deepmod/na12878_cluster_train_mod-keep_prob0.7-nb25-chr1/
 * Cg.cov5.nb25.meta): the MLP of dm_cluster_predict with TF1 dropout behind both hidden layers (a / keep_prob * floor(keep_prob + U[0,1))),
 * loss = mean((output - y)^2) over the n rows, AdamOptimizer (lr 1e-3, beta1 0.9, beta2 0.999, eps 1e-8).  fp32 throughout, no float atomics: two
 * runs are bit-identical.  The dropout mask is this library's own counter-based generator keyed by (seed, step, row in batch, unit 0..119; units
 * 0..99 = layer 1, 100..119 = layer 2), defined by deepmod_amd/cluster_train.py:dropout_keep; TensorFlow's stream cannot be reproduced.
 *   weights, grad, m, v   the DM_CLUSTER_WEIGHT_FLOATS layout of dm_cluster_create; a dm_cluster can be created from get_state's weights as they are
 *   all pointers          host memory
 *   max_batch             in [1, 65536]; n > max_batch is refused (DM_EINVAL), nothing grows
 *   _set_data             x [n_rows][14], y [n_rows]: one resident copy on the device, replacing the last
 *   _grad                 host rows x [n][14], y [n]; keep: uint8 [n][120] of 0 / 1, or NULL: the mask generated for (seed, step).  loss, out [n]
 *                         and the gradient blob (each may be NULL); the state does not change
 *   _adam                 one Adam step from a caller-supplied gradient blob
 *   _step                 rows ids [n] (int64, each in [0, n_rows), repeats allowed) of the resident data, the mask generated for (seed, the handle's
 *                         step count t), grad + adam: exactly the state of _grad on those rows with that mask followed by _adam.  Three kernel
 *                         launches, nothing is downloaded and the host does not wait; the step's loss is recorded on the device
 *   _losses               the recorded losses of steps [first_step, first_step + count) - step numbers are values of t before the step; the record
 *                         starts at creation and again behind every _set_state and _adam.  Waits for those steps
 *   _mask                 the generated mask uint8 [n][120] (n <= max_batch)
 *   _get_state / _set_state   weights, Adam slots m and v (any may be NULL) and the step count t
 * n == 0 is a no-op.  NaN / Inf in x or y, keep_prob outside (0, 1], an id outside the data, _step before _set_data, or a non-finite loss in _grad
 * return DM_EINVAL with dm_last_error set and leave the state unchanged.  The loss of a _step is looked at only in _losses: it returns DM_EINVAL for
 * a non-finite one (the values are still written), and by then that step and every later one HAVE been applied - the weights are no longer
 * usable; keep a _get_state copy from before (cluster_train.py keeps the last epoch's) to go back to.
 */
typedef struct dm_cluster_trainer dm_cluster_trainer;
dm_cluster_trainer* dm_cluster_trainer_create(int device, const float* weights, size_t n_floats, int64_t max_batch);
void dm_cluster_trainer_destroy(dm_cluster_trainer* t);
int dm_cluster_trainer_set_data(dm_cluster_trainer* t, const float* x, const float* y, int64_t n_rows);
int dm_cluster_trainer_grad(dm_cluster_trainer* t, const float* x, const float* y, int64_t n, float keep_prob, const uint8_t* keep, uint64_t seed,
                            int64_t step, float* loss, float* out, float* grad);
int dm_cluster_trainer_adam(dm_cluster_trainer* t, const float* grad);
int dm_cluster_trainer_step(dm_cluster_trainer* t, const int64_t* ids, int64_t n, float keep_prob, uint64_t seed);
int dm_cluster_trainer_losses(dm_cluster_trainer* t, int64_t first_step, int64_t count, float* losses);
int dm_cluster_trainer_mask(dm_cluster_trainer* t, uint64_t seed, int64_t step, int64_t n, float keep_prob, uint8_t* keep);
int dm_cluster_trainer_get_state(dm_cluster_trainer* t, float* weights, float* m, float* v, int64_t* step);
int dm_cluster_trainer_set_state(dm_cluster_trainer* t, const float* weights, const float* m, const float* v, int64_t step);

/* ---------------------------------------------------------------------- getfeatures -- */
/*
 * The reference's third sub-command (bin/DeepMod_scripts/myGetFeatureBasedPos.py): raw reads + a reference + known positions -> the labelled
 * *.xy.gz text `train` reads.  A matrix row of get_Feature (:355-528) travels as (pos, lab, code) + the event it shows:
 *   pos   int64  column 0, the reference position (0 outside the aligned part)
 *   lab   uint8  0 none | 1 negative (column 1) | 2 positive (column 2)
 *   code  uint8  the one-hot class dm_rows_assemble takes (columns 3..6)
 *   rdesc int64 [reads][4]  dm_rows_assemble's descriptors: columns 7..9 are (mean, stdv, length) of event q + rdesc[1] of the ev3 block
 * HOST (csrc/xyrows.inc):
 *   dm_xy_sites_*   the position lists (fulmodlist / anymodlist / nomodlist, :653-701) as sorted arrays per contig x strand; has_any / has_no:
 *                   the list is not None (--motifORPos 2).  Membership is by (strand, refbasei) value, as in the reference.
 *   dm_xy_labels    the columns dm_map_read writes -> pos / lab / code of the read's matrix rows (n_events - end_clip - start_clip + 200 of them,
 *                   written from index 0 of the arrays) and its descriptor for rows from row0 and events from ev0 of a batch.  motif: NULL
 *                   without a motif (--motifORPos 2), else upper case; posneg as the reference's flag.
 *   dm_xy_read      a SAM record -> the same, through the walk of dm_map_read with the CpG gap swap only for motif "CG" (:302); a base
 *                   mismatch does not end the read (:462-464).  info[DM_XY_STATUS]:
 */
#define DM_XY_OK 0
#define DM_XY_LESS_EVENT 1        /* fewer than 500 aligned events (:321-323) */
#define DM_XY_NO_SITE 2           /* no listed position on the contig (:135-138) */
#define DM_XY_FILTERED 3          /* region filter (:174-181; set by the caller, which knows the names) */
#define DM_XY_NO_MATCH 4          /* no matching base (:245-250) */
#define DM_XY_INDEX_ERROR 5       /* fewer aligned table rows than aligned events (the reference raises IndexError, :455) */
#define DM_XY_NEED_ROWS 6         /* cap_rows < info[DM_XY_N_ROWS]: nothing written */
#define DM_XY_INFO_LEN 8
#define DM_XY_STATUS 0
#define DM_XY_N_ROWS 1
#define DM_XY_STRAND 2
#define DM_XY_START_CLIP 3
#define DM_XY_END_CLIP 4
#define DM_XY_POS_AFTER_CLIP 5
#define DM_XY_EVENTS_AFTER_CLIP 6
typedef struct dm_xysites dm_xysites;
dm_xysites* dm_xy_sites_create(int32_t n_contigs, int has_any, int has_no);
void dm_xy_sites_destroy(dm_xysites* s);
int dm_xy_sites_set(dm_xysites* s, int32_t contig, int strand, int kind, const int64_t* pos, int64_t n);
int dm_xy_labels(const dm_xysites* s, int32_t contig, int strand, const char* motif, int motif_pos, int posneg, const char* refbase, const char* readbase,
                 const uint64_t* refbasei, int64_t n_table_rows, int64_t n_events, int64_t start_clip, int64_t end_clip, int64_t mapped_start_pos,
                 int64_t num_insertions, int64_t* pos, uint8_t* lab, uint8_t* code, int64_t cap_rows, int64_t row0, int64_t ev0, int64_t* rdesc,
                 int64_t* info);
int dm_xy_read(const dm_xysites* s, int32_t contig, int flag, int64_t pos1, const char* cigar, const char* readseq, int64_t readseq_len, const char* refseq,
               int64_t refseq_len, int64_t n_events, const char* motif, int motif_pos, int posneg, int64_t* pos, uint8_t* lab, uint8_t* code,
               int64_t cap_rows, int64_t row0, int64_t ev0, int64_t* rdesc, int64_t* info);
/* The text: np.savetxt(fmt='%.3f') of rows [n][10] doubles - snprintf("%.3f") of the ten values joined by one space, then '\n' ('nan' without a
 * sign).  -> the bytes of the text; written only if cap holds all of them.  dm_xy_rows_host: the device stage below on the host, from host
 * statistics ev3 [n_events][3] (the rows of a batch are never materialised); keep, the offset tables and text are optional, text is written as far
 * as cap reaches. */
int64_t dm_xy_format_host(const double* rows, int64_t n_rows, char* out, int64_t cap);
int64_t dm_xy_rows_host(const int64_t* pos, const uint8_t* lab, const uint8_t* code, const int64_t* rdesc, int64_t n_reads, int64_t n_rows, const float* ev3,
                        int64_t n_events, uint8_t* keep, int64_t* read_row_off, int64_t* read_byte_off, char* text, int64_t cap);
/* DEVICE (csrc/xyrows.hip.inc): row selection (:512-526) and text of a batch, statistics read where the signal stage left them (d_ev3, the block of
 * dm_signal_event_stats_device / dm_signal_move_stats_device, [n_events][3]).  A row is kept if a labelled row of ITS read lies within +-25 rows;
 * a read of n rows with 10 kept > 9 n keeps all, one with none gives nothing.  Plain launches on one stream, no atomics: two calls give the same bytes.
 *   dm_xy_rows        pos / lab / code [n_rows], rdesc [n_reads][4]: host arrays, checked before use.  -> the bytes of the text (< 0: error code).
 *                     *flag = 1: a mean or stdv of a kept row is not finite or >= 2^30 in magnitude, or a length is above 2^24 - the device
 *                     formatter does not take those, and the call has computed the batch through dm_xy_rows_host on the downloaded block
 *                     instead: the result is the reference's bytes either way.
 *   dm_xy_rows_fetch  of the last call: the text, keep [n_rows], read_row_off / read_byte_off [n_reads + 1] (first output row / byte of every read,
 *                     the totals last) - any may be NULL.
 *   dm_xy_times       milliseconds the selection and the text kernels of the last call took on the device (HIP events).
 *   dm_xy_scan        the stage's 64-bit exclusive scan on its own: values [n + 1] (host) <- the prefix sums of values [0 .. n) and their total. */
typedef struct dm_xyrows dm_xyrows;
dm_xyrows* dm_xy_create(int device);
void dm_xy_destroy(dm_xyrows* h);
int64_t dm_xy_rows(dm_xyrows* h, const int64_t* pos, const uint8_t* lab, const uint8_t* code, const int64_t* rdesc, int64_t n_reads, int64_t n_rows,
                   const float* d_ev3, int64_t n_events, int32_t* flag);
int dm_xy_rows_fetch(dm_xyrows* h, char* text, uint8_t* keep, int64_t* read_row_off, int64_t* read_byte_off);
int dm_xy_times(dm_xyrows* h, double* keep_ms, double* text_ms);
int dm_xy_scan(dm_xyrows* h, int64_t* values, int64_t n);

/* -------------------------------------------------------------------------- predict -- */
/*
 * The inverse of the text stage above, for `DeepMod.py predict` (csrc/xyparse.hip.inc): the decompressed bytes of one .xy file -> its table on
 * the device, bit-equal to np.loadtxt(dtype=float32, ndmin=2) of the same bytes (myMultiBiRNN.py:307), and the rows whose windows
 * getDataFromFile_new (:306-343) would return.  The table is kept as head [R][3] (column 0 position, columns 1..2 the labels) and feats [R][7]
 * (columns 3..9, contiguous: the `rows` of dm_predict_read_at).
 * The device parses lines of ten fields -?[0-9]+(\.[0-9]+)? of at most 15 digit characters, separated by one space and ended by '\n' (a missing
 * last '\n' is supplied).  A field is its digits as an integer divided once, in IEEE double, by the exact power of ten of its decimals, then the
 * sign, then the cast to float: the correctly rounded double of strtod, cast as numpy casts it.  Any other line (nan, inf, exponents, '+', tabs,
 * two spaces, '\r', empty lines, '#', nine or eleven fields, 16 digits, '.5', '5.') raises *flag; *first_bad_line is the 1-based number of the
 * first such line (-1: none).  The table of a flagged text is not usable: the caller loads the file on the host and hands the result to
 * dm_xyload_set_table (deepmod_amd/xyload.py does).  Plain launches on one stream, no atomics: two calls on the same bytes give the same bytes.
 *   dm_xyload_parse          text: host bytes.  -> DM_OK, *n_rows = R.  Buffers grow and are kept between files; sizes are checked before a launch.
 *   dm_xyload_parse_host     the same line routine compiled for the host (no GPU needed): table [cap_rows][10] receives the rows below cap_rows
 *                            (a line outside the grammar as zeros).  -> R (< 0: error code).
 *   dm_xyload_set_table      table [n_rows][10] host -> the handle's table, in place of a parse.
 *   dm_xyload_select         kind 0: every labelled row; '-': not those with lo < int(position) < hi; '+': only those (the float32 position
 *                            truncated, as the reference's astype(int)).  A row is labelled unless both labels are below 0.01f.  The selected rows
 *                            in ascending order are centre int32 [n]; label u8 [n] is 1 where int(column 2) == 1 (:407).  -> n, or an error code;
 *                            a selected row with fewer than 10 rows to an edge of the table is DM_EINVAL with *short_row = the first such row.
 *   dm_xyload_set_selection  centre / label [n] host (checked: 10 <= centre < R - 10) in place of a selection: the host loader's rows of a file
 *                            with NaN windows, which the device selection does not look for.
 *   dm_xyload_device         the device addresses dm_predict_read_at takes (d_centre NULL while n <= 0), R and n (-1: no selection).
 *   dm_xyload_fetch          feats [R][7], head [R][3], centre [n], label [n] to host arrays; any may be NULL.
 *   dm_xyload_select_host    the same selection on a host table [n_rows][10], by the routines the kernels run (no GPU needed): centre / label receive
 *                            the rows below cap.  -> n, or an error code with *short_row as above.
 *   dm_xyload_classify       dm_predict_read_at of the model on the handle's table and selection; back come cls u8 [n], prob1 float [n] (the
 *                            probability of class 1, gathered on the device into one contiguous block) and, unless NULL, label u8 [n]: 6 bytes per
 *                            window, nothing of the table.  DM_ERANGE as dm_predict_read_at reports it.
 *   dm_xyload_times          milliseconds between the HIP events around the kernels of the last parse / select (each interval holds one
 *                            8-byte read-back the next launches are sized from); 0 for a call that launched nothing.
 *   dm_xyload_tile_bytes     text bytes per block of the newline kernels; dm_xyload_scan_block: elements per block of the scan.  Tests build
 *                            their boundary cases from them. */
typedef struct dm_xyload dm_xyload;
dm_xyload* dm_xyload_create(int device);
void dm_xyload_destroy(dm_xyload* h);
int dm_xyload_parse(dm_xyload* h, const char* text, int64_t n_bytes, int64_t* n_rows, int32_t* flag, int64_t* first_bad_line);
int64_t dm_xyload_parse_host(const char* text, int64_t n_bytes, float* table, int64_t cap_rows, int32_t* flag, int64_t* first_bad_line);
int dm_xyload_set_table(dm_xyload* h, const float* table, int64_t n_rows);
int64_t dm_xyload_select(dm_xyload* h, int kind, int64_t lo, int64_t hi, int64_t* short_row);
int64_t dm_xyload_select_host(const float* table, int64_t n_rows, int kind, int64_t lo, int64_t hi, int32_t* centre, uint8_t* label, int64_t cap, int64_t* short_row);
int dm_xyload_set_selection(dm_xyload* h, const int32_t* centre, const uint8_t* label, int64_t n);
int dm_xyload_device(dm_xyload* h, const float** d_feats, const int32_t** d_centre, int64_t* n_rows, int64_t* n);
int dm_xyload_fetch(dm_xyload* h, float* feats, float* head, int32_t* centre, uint8_t* label);
int dm_xyload_classify(dm_xyload* h, dm_model* m, float* prob1, uint8_t* cls, uint8_t* label);
int dm_xyload_times(dm_xyload* h, double* parse_ms, double* select_ms);
int dm_xyload_tile_bytes(void);
int dm_xyload_scan_block(void);

/* The RESIDENT SET: the files `train --validate` scores at every checkpoint, kept on the device after one load each.  No reference counterpart
 * (the reference's train never looks at the data --test holds out).  A segment is what dm_xyload holds after a file's parse and selection -
 * feature rows [R][7], centres int32 [n] relative to the segment's first row, labels u8 [n]: 28 bytes per row + 5 per window.
 *   dm_xyset_create    initial_rows sizes the first blocks (rows; one window per eight rows); every block at least doubles when it is full.
 *   dm_xyset_append    the loader's table and selection become the next segment: three device-to-device copies on the set's stream, complete
 *                      on return (the loader may load its next file or be destroyed).  A loader with n == 0 adds no segment.
 *   dm_xyset_segments  -> the number of segments; rows / windows [cap] receive R and n of the segments below cap (either may be NULL).
 *   dm_xyset_classify  one segment as dm_xyload_classify classifies its file: dm_predict_read_at on the segment's rows and centres; prob1 float [n],
 *                      cls u8 [n] and, unless NULL, label u8 [n] come back (host arrays).  DM_ERANGE is the segment's own: the caller repeats that
 *                      segment with DM_PREC_F32, as for a file.  Results equal the loader's byte for byte.
 *   dm_xyset_bytes     28 * (rows of all segments) + 5 * (windows of all segments): what the set keeps for its files. */
typedef struct dm_xyset dm_xyset;
dm_xyset* dm_xyset_create(int device, int64_t initial_rows);
void dm_xyset_destroy(dm_xyset* s);
int dm_xyset_append(dm_xyset* s, dm_xyload* h);
int64_t dm_xyset_segments(dm_xyset* s, int64_t* rows, int64_t* windows, int64_t cap);
int dm_xyset_classify(dm_xyset* s, dm_model* m, int64_t segment, float* prob1, uint8_t* cls, uint8_t* label);
int64_t dm_xyset_bytes(dm_xyset* s);

/* TRAINING FROM THE SET (`train --resident 1`): the training files are segments of a set as well, and a step names its windows by id.  A window's
 * id is its index over the concatenated segments: segment s holds the ids [sum of the windows before s, + its own n), in its centres' order.
 *   dm_xyset_gather      x [n][21][7] (host or device, detected) receives the windows of ids int64 [n] (host or device): the 147 contiguous
 *                        floats feats[(centre - 10) * 7 .. (centre + 11) * 7) of each - what getDataFromFile_new's table[:, 3:][index] holds.
 *                        One kernel on the set's stream resolves every id by a binary search over the segments' window prefix sums.
 *   dm_trainer_step_set  dm_trainer_step whose x is gathered on the device into the trainer's input block: the host sends 8 B of id and 8 B of y
 *   dm_trainer_grad_set  per window.  From the gather on it is dm_trainer_step / dm_trainer_grad's own code: same finite check, same kernels, same
 *                        two host round trips (the id check comes back with the finite check's flag), results bit for bit.  ids and y: host arrays.
 * An id outside [0, windows of the set) returns DM_EINVAL, dm_last_error names the first such id and its position; nothing is launched past
 * the check and the trainer's state is unchanged.  A set on another device than the trainer, n > max_batch and null handles are refused likewise.
 * The set must not be appended to while a call is running on it (one host thread drives both). */
int dm_xyset_gather(dm_xyset* s, const int64_t* ids, int64_t n, float* x);
int dm_trainer_step_set(dm_trainer* t, dm_xyset* s, const int64_t* ids, const float* y, int64_t n, int unbalanced, float* loss);
int dm_trainer_grad_set(dm_trainer* t, dm_xyset* s, const int64_t* ids, const float* y, int64_t n, int unbalanced, float* loss, float* prob, float* grad);

/* ------------------------------------------------------------------------- siteperf -- */
/* Site-level ROC / PR of a run against control runs (DeepMod_tools/cal_EcoliDetPerf.py; csrc/siteperf.hip.inc): BED lines ->
 * hist int64 [category 7][label 2][bucket n_thresholds][percentage 101], the sums tp / fp / tn / fn and line counters.  bucket = (thresholds <=
 * coverage) - 1; a line below the smallest threshold enters the sums only.  One contig at a time, the counters accumulate; integer atomics only:
 * the result is exact and the same on every run.  deepmod_amd/siteperf.py (HostEngine) states the semantics.
 *   create         1 to 8 thresholds, non-negative, strictly ascending.
 *   set_contig     seq: len FASTA bytes (compared case-sensitively); motif: m <= 16 letters as typed, k the modified offset; start / end inclusive,
 *                  negative: none.  Writes the site codes (bit 0 '+', bit 1 '-'; fetch_codes: code [len]) and zeroes the control tables.
 *   add_text       one BED file's bytes, all of contig_name; role 0 run, 1 control.  Device grammar: >= 12 fields of printable bytes, one ' ' or
 *                  '\t' between them, '\n' at the end; field 0 = contig_name; fields 1, 9, 10, 11 of 1 - 10 digits <= 2^31 - 1; position < len,
 *                  percentage <= 100, modified <= coverage; field 3 one byte; field 5 '+' or '-'.  A text with a line outside it sets *flag and
 *                  *first_bad_line (1-based) and is NOT counted: the caller parses it and calls add_records.
 *   add_records    the same counting from host arrays [n] (pos, cov, pct, mod int32; strand u8 0 '+' 1 '-'; base u8), checked before any launch.
 *                  fetch_records: the records of the last add_text / add_records as they lie on the device.
 *   finish_contig  every control (position, strand) -> one label-0 entry, pct = (100 * mod) / cov, base of the first control line (smallest
 *                  file, then line).  Refused: per-file largest coverages of the contig summing to >= 2^31.
 *   fetch          hist, counts [4] = tp, fp, tn, fn; lines handed in, lines outside the region, lines with an unexpected base.
 *   parse_host     the device's line routine compiled for the host (no GPU needed) -> lines.  times: ms of the parse / count kernels (HIP events). */
typedef struct dm_siteperf dm_siteperf;
dm_siteperf* dm_siteperf_create(int device, int n_thresholds, const int32_t* thresholds);
void dm_siteperf_destroy(dm_siteperf* h);
int dm_siteperf_set_contig(dm_siteperf* h, const uint8_t* seq, int64_t len, const char* motif, int m, int k, int64_t start, int64_t end);
int dm_siteperf_fetch_codes(dm_siteperf* h, uint8_t* code);
int dm_siteperf_add_text(dm_siteperf* h, const char* text, int64_t n_bytes, int role, const char* contig_name, int64_t* n_lines, int32_t* flag, int64_t* first_bad_line);
int dm_siteperf_add_records(dm_siteperf* h, int role, int64_t n, const int32_t* pos, const uint8_t* strand, const uint8_t* base, const int32_t* cov, const int32_t* pct,
                            const int32_t* mod);
int dm_siteperf_fetch_records(dm_siteperf* h, int32_t* pos, uint8_t* strand, uint8_t* base, int32_t* cov, int32_t* pct, int32_t* mod);
int dm_siteperf_finish_contig(dm_siteperf* h);
int dm_siteperf_fetch(dm_siteperf* h, int64_t* hist, int64_t* counts, int64_t* lines_seen, int64_t* lines_skipped, int64_t* base_mismatch);
int64_t dm_siteperf_parse_host(const char* text, int64_t n_bytes, const char* contig_name, int64_t contig_len, int32_t* pos, uint8_t* strand, uint8_t* base, int32_t* cov,
                               int32_t* pct, int32_t* mod, int64_t cap, int32_t* flag, int64_t* first_bad_line);
int dm_siteperf_tile_bytes(void);
int dm_siteperf_times(dm_siteperf* h, double* parse_ms, double* count_ms);

/* ---------------------------------------------------------------------------- merge -- */
/* Sum the BED files of several runs of one contig and write the merged file (DeepMod_tools/sum_chr_mod.py; csrc/bedmerge.hip.inc, bedmerge.inc,
 * DESIGN.md 17): lines -> (position, strand, coverage, modified) -> int32 sums in two dm_summary tables (the caller's: '+' and '-', of equal
 * length, at most 2^31 - 1 positions; the handles dm_cluster_sites takes) -> the text, in runs of whole tiles.  Integer atomics for the sums, no
 * atomics in the text: two runs give identical bytes.  merge.merge_beds / merge.save_mod of deepmod_amd/merge.py state the semantics.
 *   open           the tables and the contig's name (1 - 255 printable bytes).  fixed_length != 0: the tables have the contig's length, a line beyond
 *                  it is outside the grammar; 0: the tables are grown (dm_summary_grow) to the largest position + 1 of a text before its adds.
 *   add_text       one BED file's bytes.  Device grammar of a line: fields of printable bytes (0x21 - 0x7e) separated by runs of one or more ' ' /
 *                  '\t', leading and trailing runs allowed, '\n' at the end (a missing last one is supplied); at least 12 fields; field 0 = the
 *                  contig's name byte for byte; fields 1, 9, 11 (position, coverage, modified) of 1 - 10 digits, <= 2^31 - 1; field 5 '+' or '-';
 *                  modified <= coverage; position < the table length when it is fixed, <= 2^31 - 2 otherwise; fields 3 and 10 are not looked at.
 *                  Inside: what detect writes (a space before the newline), what sum_chr_mod.py writes (two spaces after the strand), what
 *                  hm_cluster_predict.py writes (13 fields).  Outside: '\r', a blank line, another contig, a sign, 11 fields, 11 digits.  A text with
 *                  a line outside it sets *flag and *first_bad_line (1-based) and adds NOTHING: the caller parses it and calls add_records.
 *                  Per record: touch += 1, cov += coverage, mod += modified at (strand, position); two records of one text on one key both count.
 *   add_records    the same adds from host arrays [n] (pos, cov, mod int32; strand u8 0 '+' 1 '-'), checked before any launch.
 *                  Both refuse (DM_EINVAL, nothing added) a text or array with which the largest coverages of the contig's texts would sum to
 *                  >= 2^31.  fetch_records: the records of the last add_text / add_records as they lie on the device.
 *   format_begin   lines and bytes of the merged text, and the bytes of its largest tile (dm_bedmerge_tile_positions() positions each).  A line
 *                  '%s %d %d %s %d %s  %d %d 0,0,0 %d %d %d\n' (name, pos, pos + 1, base, min(cov, 1000), strand, pos, pos + 1, cov,
 *                  (100 * mod) / cov, mod) for every (position, strand) with mod > 0, '+' before '-' at one position.
 *   format_next    the next run of whole tiles that fits `cap` bytes -> out, *got bytes; returns 1 while more follows, 0 after the last run,
 *                  < 0 on error: a cap below the next tile's bytes is DM_EINVAL, and dm_last_error names the size needed.  The tables must not
 *                  change between format_begin and the last format_next.
 *   parse_host / format_host   the two line routines compiled for the host (no GPU needed).  parse_host -> lines, records as far as cap reaches
 *                  (table_length < 0: none given).  format_host: tables of positions first_pos .. first_pos + length - 1 (a strand may be NULL) ->
 *                  the bytes of the text; written only if out is given and cap holds them all.
 *   times          ms of the parse / add / format kernels so far (HIP events); a format_begin that finds no line adds nothing. */
typedef struct dm_bedmerge dm_bedmerge;
dm_bedmerge* dm_bedmerge_create(int device);
void dm_bedmerge_destroy(dm_bedmerge* h);
int dm_bedmerge_open(dm_bedmerge* h, dm_summary* plus, dm_summary* minus, const char* contig_name, int fixed_length);
int dm_bedmerge_add_text(dm_bedmerge* h, const char* text, int64_t n_bytes, int64_t* n_lines, int32_t* flag, int64_t* first_bad_line);
int dm_bedmerge_add_records(dm_bedmerge* h, int64_t n, const int32_t* pos, const uint8_t* strand, const int32_t* cov, const int32_t* mod);
int dm_bedmerge_fetch_records(dm_bedmerge* h, int32_t* pos, uint8_t* strand, int32_t* cov, int32_t* mod);
int dm_bedmerge_format_begin(dm_bedmerge* h, char base, int64_t* n_lines, int64_t* n_bytes, int64_t* largest_tile_bytes);
int dm_bedmerge_format_next(dm_bedmerge* h, char* out, int64_t cap, int64_t* got);
int64_t dm_bedmerge_parse_host(const char* text, int64_t n_bytes, const char* contig_name, int64_t table_length, int32_t* pos, uint8_t* strand, int32_t* cov, int32_t* mod,
                               int64_t cap, int32_t* flag, int64_t* first_bad_line);
int64_t dm_bedmerge_format_host(const char* contig_name, char base, int64_t first_pos, int64_t length, const int32_t* cov_plus, const int32_t* mod_plus,
                                const int32_t* cov_minus, const int32_t* mod_minus, char* out, int64_t cap, int64_t* n_lines);
int dm_bedmerge_tile_positions(void);
int dm_bedmerge_times(dm_bedmerge* h, double* parse_ms, double* add_ms, double* format_ms);

/* --------------------------------------------------------------------------- bsperf -- */
/* Score the predicted percentages of a run against whole-genome bisulfite replicates (docs/Reproducibility.md, Example 3, Step 5;
 * csrc/bsperf.hip.inc, bsperf.inc).  The prediction side of a contig are two dm_summary tables (the caller's: the ones dm_bedmerge
 * fills); the truth side are 1 - 4 bedMethyl replicates, parsed in chunks into records that the caller buckets by contig.  Counters, all int64 and
 * accumulating over contigs: hist [kind 2][label 3][bucket T][percentage 101] (sites with truth and a prediction; kind 0 raw, 1 clustered),
 * unpredicted [kind][label][bucket], moments [kind][bucket][6] = n, sum x, sum y, sum xy, sum x^2, sum y^2 over all labels, untruthed [kind],
 * below_threshold [kind].  Per (strand, position): the site has truth if every replicate has a record; m = min coverage, bucket = (thresholds
 * <= m) - 1 (none: below_threshold only); label 1 if every percentage >= methylated, else 0 if every percentage <= unmethylated, else 2;
 * y = the sum of the percentages; predicted if the summed coverage >= pred_cov, x = (100 * mod) / cov in integers (kind 1: a site of add_scores,
 * x its percentage).  Integer atomics only: exact, and the same on every run.  deepmod_amd/bsperf.py (HostEngine) states the semantics.
 *   create         1 - 64 distinct contig names of 1 - 63 printable bytes; lengths: NULL or per contig its positions (< 0: not known, at most
 *                  2^31 - 1 positions); 1 - 8 thresholds >= 1, strictly ascending; 1 - 4 replicates; 0 <= unmethylated < methylated <= 100;
 *                  pred_cov >= 1.
 *   add_truth_text one chunk of a replicate's text, cut at a line end (a missing last '\n' is supplied); is_first_chunk != 0: line 1 is the
 *                  file's first line and is skipped unread.  Rules of a line, in this order: its length without leading and trailing ' ' / '\t'
 *                  is <= 20: skipped.  Grammar: fields of printable bytes (0x21 - 0x7e) separated by runs of one or more ' ' / '\t', leading
 *                  and trailing runs allowed; exactly 11 fields; fields 1, 9, 10 (position, coverage, percentage) of 1 - 10 digits, <= 2^31 - 1;
 *                  percentage <= 100.  Field 5 neither '+' nor '-': skipped.  Field 0 none of the names, byte for byte: skipped.  Position at or
 *                  beyond the contig's length (2^31 - 1 if not known): outside the grammar.  Coverage 0: dropped.  Else a record: position, and
 *                  meta = min(coverage, 65535) | percentage << 16 | strand << 23 | contig index << 24.  Outside the grammar: 10 or 12 fields,
 *                  '\r', a sign, 11 digits, percentage 101.  A chunk with such a line sets *flag and *first_bad_line (1-based) and adds NOTHING:
 *                  the caller parses it and calls add_truth_records.  lines [6]: records, first lines, short lines, other strands, other
 *                  contigs, coverage 0, of this chunk; the handle sums them (fetch).  The records stay on the device, in line order.
 *   add_truth_records  the records (contig index u8, strand u8 0 '+' 1 '-', pos, cov >= 1, pct int32) and the line counters of a chunk the caller
 *                  parsed, checked before any copy; they take the place of the device parser's.
 *   fetch_records  the records of the last add_truth_text / add_truth_records as they lie on the device: pos int32 [n], meta uint32 [n].
 *   open           the open contig: its index and its two tables, of equal length, at most the contig's.  One zeroed 32-bit slot per (replicate,
 *                  strand, position).  close_contig lets go of the tables.
 *   fill           records of the open contig (as fetch_records gave them) into the slots of `replicate`, checked before any launch: another
 *                  contig, a position outside the tables, coverage 0 are DM_EINVAL.  A key that occurs twice in the replicate (in one call or
 *                  in two): DM_EINVAL, *dup_pos / *dup_strand the smallest such key, and the contig cannot be counted any more.
 *   count          kind 0: one sweep over (strand, position) of the open contig, once.  DM_EINVAL: a sum outside 0 <= modified <= coverage.
 *   add_scores     kind 1, once, after count: n distinct sites (pos int32, strand u8, percentage 0 - 100 int32), checked before any launch; every
 *                  other position is unpredicted in kind 1.
 *   fetch          the counters as laid out above, and lines [6] summed over the chunks.
 *   parse_host     the line routine compiled for the host (no GPU needed) -> records, written as far as cap reaches.
 *   times          ms of the parse / fill / count kernels so far (HIP events).  tile_bytes: bytes of one tile of the line splitter. */
typedef struct dm_bsperf dm_bsperf;
dm_bsperf* dm_bsperf_create(int device, int n_contigs, const char* const* names, const int64_t* lengths, int n_thresholds, const int32_t* thresholds, int n_replicates,
                            int methylated, int unmethylated, int pred_cov);
void dm_bsperf_destroy(dm_bsperf* h);
int dm_bsperf_add_truth_text(dm_bsperf* h, int replicate, const char* text, int64_t n_bytes, int is_first_chunk, int64_t* lines, int64_t* n_records, int32_t* flag,
                             int64_t* first_bad_line);
int dm_bsperf_add_truth_records(dm_bsperf* h, int replicate, int64_t n, const uint8_t* contig, const uint8_t* strand, const int32_t* pos, const int32_t* cov,
                                const int32_t* pct, const int64_t* lines);
int dm_bsperf_fetch_records(dm_bsperf* h, int32_t* pos, uint32_t* meta);
int dm_bsperf_open(dm_bsperf* h, int contig_index, dm_summary* plus, dm_summary* minus);
int dm_bsperf_close_contig(dm_bsperf* h);
int dm_bsperf_fill(dm_bsperf* h, int replicate, int64_t n, const int32_t* pos, const uint32_t* meta, int64_t* dup_pos, int32_t* dup_strand);
int dm_bsperf_count(dm_bsperf* h);
int dm_bsperf_add_scores(dm_bsperf* h, int64_t n, const int32_t* pos, const uint8_t* strand, const int32_t* pct);
int dm_bsperf_fetch(dm_bsperf* h, int64_t* hist, int64_t* unpredicted, int64_t* moments, int64_t* untruthed, int64_t* below_threshold, int64_t* lines);
int64_t dm_bsperf_parse_host(const char* text, int64_t n_bytes, int n_contigs, const char* const* names, const int64_t* lengths, int is_first_chunk, int32_t* pos,
                             uint32_t* meta, int64_t cap, int64_t* lines, int32_t* flag, int64_t* first_bad_line);
int dm_bsperf_tile_bytes(void);
int dm_bsperf_times(dm_bsperf* h, double* parse_ms, double* fill_ms, double* count_ms);

/* ------------------------------------------------------------------------- bslabels -- */
/* Training position lists from bisulfite replicates: the fulmod / anymod / nomod files getfeatures --motifORPos 2 reads (`chr strand pos`
 * lines; csrc/bslabels.hip.inc, bslabels.inc).  The truth side is dm_bsperf's, one copy of the code: 1 - 4 bedMethyl replicates,
 * parsed in chunks into records that the caller buckets by contig, then one 32-bit slot per (replicate, strand, position) of the open contig.
 * The reference bytes of the contig give one site code per position (bit 0: the motif lies on '+' with its modified base here, bit 1: on '-';
 * the kernel dm_siteperf_set_contig runs, on the bytes as they are handed over).  Per key (strand, position), one class byte:
 *   0  no replicate has a record                    4  a record somewhere, but the key is no site of the motif (off_motif; in no list)
 *   1  fulmod: every replicate has a record, the smallest coverage is >= cov, every percentage is >= methylated
 *   3  nomod:  every replicate has a record, the smallest coverage is >= cov, every percentage is <= unmethylated
 *   2  anymod: every other site with a record in at least one replicate (partial, disagreeing, low coverage, missing from a replicate)
 * Integer atomics for the counters only, none in the text: two runs give identical bytes.  deepmod_amd/bslabels.py (HostEngine) states the semantics.
 *   create         1 - 64 distinct contig names of 1 - 63 printable bytes; lengths: per contig its positions, every one known, 1 to 2^31 - 1;
 *                  1 - 4 replicates; 1 <= cov <= 65535 (a record's coverage saturates there); 0 <= unmethylated < methylated <= 100.
 *   add_truth_text, add_truth_records, fetch_records   the contracts of the dm_bsperf calls of the same names: grammar, line classes, lines [6],
 *                  a flagged chunk adds nothing.
 *   open           the open contig: its index, its reference bytes (len == the contig's length), the motif (m = 1 - 8 letters of A, C, G, T, either
 *                  case) and the offset k of the modified base in it.  Zeroed slots, the site codes.  DM_ENOMEM, before any launch, with the bytes
 *                  needed if the device cannot hold 8 R + 4 bytes per position.  close_contig ends it.
 *   fill           records of the open contig (as fetch_records gave them) into the slots of `replicate`: the contract of dm_bsperf_fill, the
 *                  duplicate key included; not after classify.
 *   classify       the sweep, once per open; counts [2 strands][5] of this contig alone: fulmod, anymod, nomod, off_motif, sites
 *                  without truth.  DM_EINVAL without an open contig or a second time; DM_ESTATE after a duplicate key.
 *   fetch_classes  cls [2 strands][len] of the classified contig.
 *   format_begin   list 1 fulmod, 2 anymod, 3 nomod: lines and bytes of its text, and the bytes of its largest tile (dm_bslabels_tile_positions()
 *                  positions each).  A line '%s %s %d\n' (name, strand, 0-based position) per key of the class, ascending position, '+' before
 *                  '-' at one position.  An empty list: 0 lines, 0 bytes.
 *   format_next    the next run of whole tiles that fits `cap` bytes -> out, *got bytes; returns 1 while more follows, 0 after the last run (or
 *                  when there is no text), < 0 on error: a cap below the next tile's bytes is DM_EINVAL, and dm_last_error names the size needed.
 *   format_host    the line routine compiled for the host (no GPU needed): class arrays of positions first_pos .. first_pos + length - 1 (a
 *                  strand may be NULL; first_pos + length <= 2^31 - 1) -> the bytes of the list's text; written only if out is given and cap
 *                  holds them all.
 *   times          ms of the parse / fill (with the site codes of open) / class (the sweep) / format kernels so far (HIP events); a format_begin
 *                  of a list without a line adds nothing.
 * Every argument is checked before any launch (DM_EINVAL, dm_last_error names the fault): contig index, replicate, len, motif letters, list. */
typedef struct dm_bslabels dm_bslabels;
dm_bslabels* dm_bslabels_create(int device, int n_contigs, const char* const* names, const int64_t* lengths, int n_replicates, int cov, int methylated, int unmethylated);
void dm_bslabels_destroy(dm_bslabels* h);
int dm_bslabels_add_truth_text(dm_bslabels* h, int replicate, const char* text, int64_t n_bytes, int is_first_chunk, int64_t* lines, int64_t* n_records, int32_t* flag,
                               int64_t* first_bad_line);
int dm_bslabels_add_truth_records(dm_bslabels* h, int replicate, int64_t n, const uint8_t* contig, const uint8_t* strand, const int32_t* pos, const int32_t* cov,
                                  const int32_t* pct, const int64_t* lines);
int dm_bslabels_fetch_records(dm_bslabels* h, int32_t* pos, uint32_t* meta);
int dm_bslabels_open(dm_bslabels* h, int contig_index, const uint8_t* seq, int64_t len, const char* motif, int m, int k);
int dm_bslabels_fill(dm_bslabels* h, int replicate, int64_t n, const int32_t* pos, const uint32_t* meta, int64_t* dup_pos, int32_t* dup_strand);
int dm_bslabels_classify(dm_bslabels* h, int64_t* counts);
int dm_bslabels_fetch_classes(dm_bslabels* h, uint8_t* cls);
int dm_bslabels_format_begin(dm_bslabels* h, int list, int64_t* n_lines, int64_t* n_bytes, int64_t* largest_tile_bytes);
int dm_bslabels_format_next(dm_bslabels* h, char* out, int64_t cap, int64_t* got);
int dm_bslabels_close_contig(dm_bslabels* h);
int64_t dm_bslabels_format_host(const char* name, int list, const uint8_t* cls_plus, const uint8_t* cls_minus, int64_t first_pos, int64_t length, char* out, int64_t cap);
int dm_bslabels_tile_positions(void);
int dm_bslabels_times(dm_bslabels* h, double* parse_ms, double* fill_ms, double* class_ms, double* format_ms);

/* --------------------------------------------------------------------------- motifs -- */
/* De novo modified-motif discovery, the counting half (csrc/motifs.hip.inc, motifs.inc): one sweep over a contig joins the sample's
 * and optionally the pooled controls' tables with the contig's bytes and counts, per oriented sequence context of `up` bases upstream and `down`
 * bases downstream of `base`, the keys (strand, position) that were tested and those called modified.  Per key, the first rule that applies:
 *   1  the oriented letter (seq[p] on '+', its complement on '-') is not `base`: off_base if the sample's coverage is > 0, else ignored
 *   2  an offset of the context ('+': seq[p + j]; '-': the complement of seq[p - j]) is outside the contig or none of A, C, G, T (upper case; the
 *      bytes are taken as handed over): edge
 *   3  sample coverage < cov: shallow             4  controls given and their coverage < cov: no_control
 *   5  tested; modified too if 100 mod / cov (integer division) >= min_pct and (no controls or 100 cmod / ccov <= max_ctrl_pct)
 * The context index has its most significant base-4 digit at offset -up, A < C < G < T.  Everything is an integer sum in 64 bits: exact for
 * coverages and counts up to 2^31 - 1 and for any number of contigs.  deepmod_amd/motifs.py (HostEngine) states the semantics.
 *   create      0 <= up, down, up + down <= 8; base one of A, C, G, T; cov >= 1; 0 <= min_pct, max_ctrl_pct <= 100.  A zeroed histogram.
 *   count       one contig: len bytes (1 to 2^31 - 1), the sample's '+' and '-' tables and the controls' (both or neither), every table on the
 *               handle's device and of exactly len positions.  hist += ; counters [2 strands][5] (tested, modified, shallow, no_control, edge)
 *               and off_base [2] are those of this contig alone.
 *   fetch       hist int64 [4^(up+down)][2] (tested, modified), summed over the contigs since create / reset.      reset   zeroes it.
 *   count_host  the same sweep compiled for the host (no GPU needed), on plain arrays: len >= 0, the four control arrays all given or all null;
 *               hist is added to, counters and off_base are set.
 *   times       ms of the uploads of the contigs' bytes / of the sweeps so far (HIP events).
 * Every argument is checked before any launch (DM_EINVAL, dm_last_error names the fault): null handles, a table on another device or of another
 * length, exactly one control table, options out of range. */
typedef struct dm_motifs dm_motifs;
dm_motifs* dm_motifs_create(int device, int up, int down, char base, int cov, int min_pct, int max_ctrl_pct);
void dm_motifs_destroy(dm_motifs* h);
int dm_motifs_count(dm_motifs* h, const uint8_t* seq, int64_t len, dm_summary* plus, dm_summary* minus, dm_summary* ctrl_plus, dm_summary* ctrl_minus, int64_t* counters,
                    int64_t* off_base);
int dm_motifs_fetch(dm_motifs* h, int64_t* hist);
int dm_motifs_reset(dm_motifs* h);
int dm_motifs_tile_positions(void);
int dm_motifs_times(dm_motifs* h, double* upload_ms, double* count_ms);
int dm_motifs_count_host(int up, int down, char base, int cov, int min_pct, int max_ctrl_pct, const uint8_t* seq, int64_t len, const int32_t* cov_plus,
                         const int32_t* mod_plus, const int32_t* cov_minus, const int32_t* mod_minus, const int32_t* ctrl_cov_plus, const int32_t* ctrl_mod_plus,
                         const int32_t* ctrl_cov_minus, const int32_t* ctrl_mod_minus, int64_t* hist, int64_t* counters, int64_t* off_base);

/* -------------------------------------------------------------------------- diffmod -- */
/* Per-site differential modification of a run against pooled controls (csrc/diffmod.hip.inc, diffmod.inc): one run joins the
 * sample's and the controls' tables of a contig and tests every key (strand, position) that is deep enough in both with Fisher's exact test.
 * With cA, mA the sample's coverage and modified count and cB, mB the controls', the first rule that applies decides:
 *   1  cA == 0 and cB == 0: ignored       2  cA < cov: shallow_sample       3  cB < cov: shallow_control
 *   4  cA + cB > dm_diffmod_max_total() (2^20): too_deep                    5  tested
 * p of a tested key is the two-sided p of R's fisher.test: n1 = cA, n2 = cB, M = mA + mB, N = n1 + n2, x in [max(0, M - n2), min(n1, M)],
 *   L(x) = lf[n1] + lf[n2] + lf[M] + lf[N-M] - lf[N] - lf[x] - lf[n1-x] - lf[M-x] - lf[n2-M+x],   lf[k] = lgamma(k + 1) in fp64,
 *   p = min(1, sum of exp(L(x)) over the x with L(x) <= L(mA) + 1e-7); a support of one table is p = 1.
 * The table lf is computed once on the host and uploaded: the kernels and the host twin read the same doubles.  Within about 1.3e-10 relative of
 * the exact value for N <= 4096 and 6.7e-8 for N <= 2^20; a p that underflows is 0.  deepmod_amd/diffmod.py (HostEngine) states
 * the semantics in exact integers.
 *   create         cov >= 1; 0 < alpha <= 1.  A zeroed p histogram.
 *   run            one contig: the sample's '+' and '-' tables and the controls', all four on the handle's device and of one length.
 *                  counters [2 strands][4] (tested, shallow_sample, shallow_control, too_deep) are those of this contig; the p histogram grows by
 *                  every tested key; *n_records = the tested keys with p <= alpha, held on the device until the next run.
 *   fetch_records  records first .. first + count - 1 of the last run, in key order (ascending position, '+' before '-'): position, strand (0 '+',
 *                  1 '-'), cA, mA, cB, mB, p.
 *   fetch_hist     int64 [20]: bin min(19, int(20 p)) of every key tested since create / reset.      reset   zeroes it.
 *   test_host      the same run compiled for the host (no GPU needed), on plain arrays of len >= 0 entries: counters are set, hist is added to,
 *                  *n_records is the number of records, of which the first cap are written.
 *   times          ms of the select kernels (with their scans) / of the test kernels (with theirs) so far (HIP events).
 *   tile_positions, small_support   positions of a tile of the select kernel; the largest support a 16-lane group sums (above: a workgroup).
 * Every argument is checked before any launch (DM_EINVAL, dm_last_error names the fault): null handles, the controls missing, tables of different
 * lengths or on another device, cov < 1, alpha outside (0, 1]. */
typedef struct dm_diffmod dm_diffmod;
dm_diffmod* dm_diffmod_create(int device, int cov, double alpha);
void dm_diffmod_destroy(dm_diffmod* h);
int dm_diffmod_run(dm_diffmod* h, dm_summary* plus, dm_summary* minus, dm_summary* ctrl_plus, dm_summary* ctrl_minus, int64_t* counters, int64_t* n_records);
int dm_diffmod_fetch_records(dm_diffmod* h, int64_t first, int64_t count, int32_t* pos, uint8_t* strand, int32_t* cA, int32_t* mA, int32_t* cB, int32_t* mB, double* p);
int dm_diffmod_fetch_hist(dm_diffmod* h, int64_t* hist);
int dm_diffmod_reset(dm_diffmod* h);
int dm_diffmod_times(dm_diffmod* h, double* select_ms, double* fisher_ms);
int dm_diffmod_max_total(void);
int dm_diffmod_tile_positions(void);
int dm_diffmod_small_support(void);
int dm_diffmod_test_host(int cov, double alpha, int64_t len, const int32_t* cov_plus, const int32_t* mod_plus, const int32_t* cov_minus, const int32_t* mod_minus,
                         const int32_t* ctrl_cov_plus, const int32_t* ctrl_mod_plus, const int32_t* ctrl_cov_minus, const int32_t* ctrl_mod_minus, int64_t* counters,
                         int64_t* hist, int64_t cap, int32_t* pos, uint8_t* strand, int32_t* cA, int32_t* mA, int32_t* cB, int32_t* mB, double* p, int64_t* n_records);

/* -------------------------------------------------------------------------- diffmod --replicates -- */
/* The replicate-aware per-site test (csrc/diffrep.hip.inc, diffrep.inc): one run joins the tables of n_a sample and n_b control
 * replicates of a contig (1..8 each, 3 or more together) and gives every key (strand, position) the quasi-binomial F test of a two-group
 * logistic model (the McCullagh-Nelder overdispersion correction), in closed form.  A modified count is held to 0..coverage; replicate i is used
 * at the key iff c_i >= cov; nA, nB are the used replicates of either group, C_g and M_g the sums over them.  The first rule that applies decides:
 *   1  every c_i == 0: ignored       2  nA < min_a: shallow_sample       3  nB < min_b: shallow_control
 *   4  C_A + C_B > dm_diffmod_max_total() (2^20, formed in 64 bits): too_deep              5  tested
 * A tested key: nu = nA + nB - 2, C = C_A + C_B, M = M_A + M_B.  M_A C_B == M_B C_A in integers: p = 1 and phi = 1 exactly.  Else, with
 * h(M, C) = M ln(M / C) + (C - M) ln((C - M) / C) (a term whose factor is 0 is 0):
 *   D = max(0, 2 [h(M_A, C_A) + h(M_B, C_B) - h(M, C)]),   X2 = sum over groups and used i of r_i^2 / (c_i M_g (C_g - M_g)),  r_i = m_i C_g - c_i M_g
 *   (a group with M_g in {0, C_g} adds 0),   phi = max(1, X2 / nu),   F = D / phi,   p = I_x(nu / 2, 1 / 2) at x = nu / (nu + F).
 * All in fp64; the incomplete beta is a power series, reflected at x = 1/2, whose terms depend on the key alone, so two runs give the same bits.
 * D is within 18 * 2^-53 * C of its value, phi and the evaluation of p at that D and phi within 2.5e-11 relative.
 * deepmod_amd/diffmod.py (RepHostEngine) states the semantics in integers and 50-digit decimals.
 *   create         cov >= 1; 0 < alpha <= 1; 1 <= min_a, min_b <= 8, min_a + min_b >= 3.  A zeroed p histogram.
 *   run            one contig: plus[j], minus[j] are the tables of replicate j, the n_a sample replicates first, then the n_b control replicates;
 *                  2 (n_a + n_b) different tables on the handle's device and of one length; min_a <= n_a, min_b <= n_b.  counters
 *                  [2 strands][4] (tested, shallow_sample, shallow_control, too_deep) are those of this contig; the p histogram grows by every
 *                  tested key; *n_records = the tested keys with p <= alpha, held on the device until the next run.
 *   fetch_records  records first .. first + count - 1 of the last run, in key order (ascending position, '+' before '-'): position, strand (0 '+',
 *                  1 '-'), cA, mA, cB, mB (the sums over the used replicates), nA, nB, phi, p.
 *   fetch_hist     int64 [20]: bin min(19, int(20 p)) of every key tested since create / reset.      reset   zeroes it.
 *   test_host      the same run compiled for the host (no GPU needed): cov_plus .. mod_minus are n_a + n_b pointers each, sample replicates first,
 *                  to plain arrays of len >= 0 entries; counters are set, hist is added to, *n_records is the number of records, of which the
 *                  first cap are written.
 *   times          ms of the counting pass (with its scan) / of the writing pass so far (HIP events).
 *   max_replicates replicates of a group at most (8).  A tile of the sweep has dm_diffmod_tile_positions() positions.
 * Every argument is checked before any launch (DM_EINVAL, dm_last_error names the fault): null or repeated handles, n_a or n_b outside 1..8,
 * n_a + n_b < 3, least counts outside their ranges, tables of different lengths or on another device, cov < 1, alpha outside (0, 1]. */
typedef struct dm_diffrep dm_diffrep;
dm_diffrep* dm_diffrep_create(int device, int cov, double alpha, int min_a, int min_b);
void dm_diffrep_destroy(dm_diffrep* h);
int dm_diffrep_run(dm_diffrep* h, int n_a, int n_b, dm_summary* const* plus, dm_summary* const* minus, int64_t* counters, int64_t* n_records);
int dm_diffrep_fetch_records(dm_diffrep* h, int64_t first, int64_t count, int32_t* pos, uint8_t* strand, int32_t* cA, int32_t* mA, int32_t* cB, int32_t* mB, uint8_t* nA,
                             uint8_t* nB, double* phi, double* p);
int dm_diffrep_fetch_hist(dm_diffrep* h, int64_t* hist);
int dm_diffrep_reset(dm_diffrep* h);
int dm_diffrep_times(dm_diffrep* h, double* count_ms, double* write_ms);
int dm_diffrep_max_replicates(void);
int dm_diffrep_test_host(int cov, double alpha, int min_a, int min_b, int n_a, int n_b, int64_t len, const int32_t* const* cov_plus, const int32_t* const* mod_plus,
                         const int32_t* const* cov_minus, const int32_t* const* mod_minus, int64_t* counters, int64_t* hist, int64_t cap, int32_t* pos, uint8_t* strand,
                         int32_t* cA, int32_t* mA, int32_t* cB, int32_t* mB, uint8_t* nA, uint8_t* nB, double* phi, double* p, int64_t* n_records);

#ifdef __cplusplus
}
#endif
#endif /* DEEPMOD_HIP_H */
