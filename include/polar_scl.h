/*
 * polar_scl.h -- C ABI of libpolar_mi355x.so, the MI355X (gfx950) polar SC/SCL engine.
 *
 * This is the drop-in boundary for the reference's hot path (heimrih/polar_code,
 * package dl_scl_polar).  The reference has no FFI of its own: it is pure Python/NumPy,
 * so each entry point below replaces a Python function, and the binding a maintainer adds
 * on the reference side is the ctypes stub shown in INTEGRATION.md.
 *
 *   pscl_create / pscl_destroy  <- the implicit per-call setup of decode_scl
 *                                  (info mask scl.py:125-126, CRC poly crc.py:10-16)
 *   pscl_decode                 <- decode_scl(llr, info_set, M, crc, force_info_bits=...)
 *                                  dl_scl_polar/polar/scl.py:108-209, batched over B frames
 *                                  (sc_decode polar.py:130-168 is the M=1 case)
 *   pscl_decode_device          <- same, device-resident buffers, asynchronous; optionally
 *                                  folds the FER/BER counting of run_fer_sweep.py:91-109
 *   pscl_channel_device         <- the per-frame TX chain of run_fer_sweep.py:79-87
 *                                  (payload, attach_crc crc.py:19-37, encode polar.py:106-119,
 *                                  BPSK, AWGN, LLR) with a counter-based Philox stream
 *   pscl_uncoded_device         <- the uncoded BPSK baseline of run_fer_sweep.py:111-121
 *   pscl_dlscl_device           <- decode_with_retries dl_scl_polar/dlscl/flip.py:65-141 over
 *                                  a device batch (+ pscl_set_beta: the beta checkpoint)
 *   pscl_adaptive_device        <- sc_decode (polar.py:130-168) + check_crc (crc.py:40-56) on every
 *                                  frame of a device batch, decode_scl only where that fails
 *   pscl_path_llrs_device       <- best_path_info_llrs / info_llrs of given paths (scl.py:158,166)
 *   pscl_label_device           <- the labelling loop of dl_scl_polar/train/make_dataset.py:52-91 over a
 *                                  device batch: baseline, |L0| order, forced retries, labels
 *   pscl_simulate               <- one SNR point of run_sweep (run_fer_sweep.py:41-191): TX,
 *                                  uncoded baseline, SCL + DL-SCL, counters, in one call
 *
 * Conventions
 *   - Plain pointers and sizes only; no torch/HIP types in signatures (streams are void*).
 *   - Every function returns 0 on success or a negative PSCL_E* code; pscl_last_error()
 *     returns a thread-local message for the last failure.  The Python host layer maps
 *     PSCL_EINVAL to ValueError, PSCL_EPRUNED to RuntimeError (scl.py:171-172), the rest
 *     to RuntimeError.
 *   - Host-buffer calls are synchronous and never retain caller pointers.  Device-buffer
 *     calls are enqueued on the handle's stream (pscl_set_stream) and return immediately.
 *   - Bit vectors crossing the boundary as "words" are little-endian packed uint64:
 *     bit j of a K-bit vector is bit (j & 63) of word (j >> 6); K-bit vectors use
 *     PSCL_WORDS(K) words.
 *   - Arithmetic is IEEE fp64 end to end, like the reference (scl.py:41, polar.py:167); the
 *     path metric reproduces numpy's logaddexp (glibc exp/log1p) bit for bit.
 */
#ifndef POLAR_SCL_H
#define POLAR_SCL_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PSCL_ABI_VERSION 1

#define PSCL_OK 0
#define PSCL_EINVAL -1   /* bad argument (shape, range, list size, force value, CRC length) */
#define PSCL_EDEVICE -2  /* HIP runtime / device failure, or no GPU */
#define PSCL_ENOMEM -3   /* device allocation failed */
#define PSCL_EPRUNED -4  /* "All paths pruned during decoding" (cannot happen for valid input) */
#define PSCL_EUNSUP -5   /* configuration outside what the kernels implement (N, L, CRC degree) */

#define PSCL_MAX_N 1024  /* code length N: power of two, 2..1024 (N <= 128: the specialised kernels,
                            every BASELINE config; 256..1024: one wavefront per frame, global scratch;
                            the decision-LLR replay pscl_path_llrs_device takes every N on float64
                            rows, its float32 form pscl_path_llrs_device_f32 N = 128 only) */
#define PSCL_MAX_L 32    /* list size M/L: 1..32 (2L candidates fit one 64-lane wavefront) */
#define PSCL_MAX_CRC 32  /* CRC degree: 1..32 */
#define PSCL_WORDS(K) (((K) + 63) / 64)

/* decode flags bit layout (pscl_decode_device d_flags[b]) */
#define PSCL_FLAG_CRC_PASS 0x80u  /* best candidate passes the CRC */
#define PSCL_FLAG_IDX_MASK 0x3fu  /* index of the best candidate in the final list */

/* counters accumulated by pscl_decode_device when d_ref_words != NULL (int64[PSCL_NCOUNT]) */
#define PSCL_CNT_FRAMES 0      /* frames decoded */
#define PSCL_CNT_FRAME_ERR 1   /* best candidate fails CRC (run_fer_sweep FER, :92-94) */
#define PSCL_CNT_BIT_ERR 2     /* best bits != reference over all K bits (run_fer_sweep BER, :95-99) */
#define PSCL_CNT_PAYLOAD_ERR 3 /* frames with >=1 error in the first k_payload bits (run_ber_sweep FER) */
#define PSCL_CNT_PAYLOAD_BIT 4 /* payload bit errors (run_ber_sweep BER, :77-82) */
#define PSCL_CNT_RETRIES 5     /* flip re-decodes run by pscl_dlscl_device */
#define PSCL_CNT_ESCALATED 6   /* frames pscl_adaptive_device handed to the list decode */
#define PSCL_NCOUNT 8

typedef struct pscl_handle pscl_handle;

/* Last error message for the calling thread ("" if none). */
const char* pscl_last_error(void);

/* ABI version compiled into the library (PSCL_ABI_VERSION). */
int pscl_abi_version(void);

/* Hash (hex) of the sources and compile flags the library was built from; the build and the
 * Python layer compare it with the sources in the tree, so a stale library is never used. */
const char* pscl_build_hash(void);

/* Number of visible HIP devices (0 when there is no GPU); negative on runtime failure. */
int pscl_device_count(void);

/*
 * Create a decoder for one polar code on one device.
 *   N        code length (power of two, 2..PSCL_MAX_N)
 *   info_set K distinct indices in [0, N), ascending (construct_info_set returns them
 *            sorted, polar.py:103); candidate bit j is u[info_set[j]] (scl.py:183).
 *            Unsorted sets are rejected with PSCL_EUNSUP.
 *   L        list size M (1..PSCL_MAX_L)
 *   crc_poly CRC generator as the integer value of the reference's hex string
 *            (e.g. 0x1864CFB for CRC-24A); 0 = no CRC (decode_scl crc=None)
 */
int pscl_create(pscl_handle** out, int device, int N, const int32_t* info_set, int K, int L,
                uint64_t crc_poly);
int pscl_destroy(pscl_handle* h);

/* Use an external hipStream_t (e.g. torch.cuda.current_stream().cuda_stream); NULL restores
 * the handle's own stream. */
int pscl_set_stream(pscl_handle* h, void* hip_stream);
void* pscl_get_stream(pscl_handle* h);
int pscl_sync(pscl_handle* h);

/*
 * Batched decode_scl on host buffers (synchronous).
 *   llr        [B][N] float64 channel LLRs (not modified)
 *   forced     NULL or [B][K] int8 in {-1,0,1}  (force_info_bits, scl.py:127-131,146-152)
 * Outputs (any may be NULL except n_paths):
 *   n_paths    [B] int32   number of paths in the final list (== min(L, 2^free_info_bits))
 *   best_bits  [B][K] int8 best_path_bits (scl.py:190-201)
 *   crc_pass   [B] uint8   check_crc(best_path_bits) (1 if crc_poly == 0)
 *   best_idx   [B] int32   index of best_path_bits in the candidate list
 *   metrics    [B][L] float64   path metrics in list order (rows >= n_paths untouched)
 *   cands      [B][L][K] int8   candidates in list order
 *   info_llrs  [B][L][K] float64 decision LLRs at info phases (scl.py:158,166)
 */
int pscl_decode(pscl_handle* h, const double* llr, int64_t B, const int8_t* forced, int32_t* n_paths,
                int8_t* best_bits, uint8_t* crc_pass, int32_t* best_idx, double* metrics, int8_t* cands,
                double* info_llrs);

/*
 * Batched sc_decode (dl_scl_polar/polar/polar.py:130-168): successive cancellation with hard
 * decisions u = (llr < 0) at information leaves, on host buffers (synchronous).
 *   bits [B][K] int8 out = u_hat[info_set]
 * The handle's list size and CRC are ignored (one path, no list, no CRC selection).
 */
int pscl_sc_decode(pscl_handle* h, const double* llr, int64_t B, int8_t* bits);

/*
 * Batched decode on device buffers, enqueued on the handle's stream.
 *   d_llr       [B][N] float64
 *   d_force     NULL or [B][2][W] uint64 (W = PSCL_WORDS(K)): force mask words, then
 *               forced-value words, indexed by info position j
 *   d_best      [B][W] uint64 best_path_bits as words (may be NULL)
 *   d_flags     [B] uint8 PSCL_FLAG_* (may be NULL)
 *   d_metrics   NULL or [B][L] float64
 *   d_cands     NULL or [B][L][W] uint64
 *   d_info_llrs NULL or [B][L][K] float64
 *   d_ref       NULL or [B][W] uint64 transmitted message words; when given, the kernel adds
 *               this batch's error statistics into d_counters (int64[PSCL_NCOUNT], device)
 *   k_payload   payload length for the PSCL_CNT_PAYLOAD_* counters (ignored if d_ref NULL)
 */
int pscl_decode_device(pscl_handle* h, const double* d_llr, int64_t B, const uint64_t* d_force,
                       uint64_t* d_best, uint8_t* d_flags, double* d_metrics, uint64_t* d_cands,
                       double* d_info_llrs, const uint64_t* d_ref, int k_payload, int64_t* d_counters);

/*
 * Generate B frames of the reference TX chain on the device (run_fer_sweep.py:79-87):
 *   payload = k_payload uniform bits; msg = attach_crc(payload) (K bits, K = k_payload + deg);
 *   u[info_set] = msg; x = polar transform(u); y = (1 - 2x) + sigma * n; llr = 2 y / sigma^2
 *   with sigma^2 = 1 / (2 * rate * 10^(ebno_db/10)).
 * Randomness: Philox4x32-10, key = (seed, stream_id), counter = (frame index, draw): frame f's
 * samples depend only on (seed, stream_id, f), so sharding frames over GPUs is exact.
 *   d_llr [B][N] float64 out;  d_msg NULL or [B][W] uint64 out (msg words)
 */
int pscl_channel_device(pscl_handle* h, uint64_t seed, uint32_t stream_id, double ebno_db, double rate,
                        int k_payload, int64_t frame0, int64_t B, double* d_llr, uint64_t* d_msg);

/*
 * Caller payloads: the TX chain above on payloads the caller supplies instead of Philox draws.
 *   d_payload [B][Wp] uint64, Wp = PSCL_WORDS(k_payload), k_payload = K - CRC degree (the payload is
 *             the message when the handle has no CRC); bit j of a frame at word j / 64, bit j % 64.
 *             Bits at and above k_payload are ignored.
 * pscl_encode_device writes any subset of (a NULL pointer skips one; all NULL is PSCL_EINVAL):
 *   d_msg   [B][W] uint64: attach_crc(payload), the layout of d_ref / d_best
 *   d_code  [B][PSCL_WORDS(E)] uint64: the transmitted bits in transmission order, E = the
 *           rate-matched length of pscl_set_rate_match or N without it; bit p is
 *           x[order[p % N]] with rate matching (interleave, then truncate or repeat, scl_nr.py:23-35)
 *           and x[p] without; bits past E in the last word are zero
 *   d_sym   [B][E] BPSK symbols 1 - 2 x, float64 (sym_f32 = 0) or float32 (sym_f32 = 1)
 * pscl_channel_payload_device adds pscl_channel_device's AWGN and writes
 *   d_llr   [B][E] LLR rows, float64 (llr_f32 = 0) or float32 (llr_f32 = 1), or NULL
 *   d_msg   as above, or NULL
 * The noise is pscl_channel_device's stream -- key (seed, stream_id), counter (frame0 + frame,
 * pair index) -- and the float64 expression is the same: called with the low k_payload bits of the
 * message words pscl_channel_device writes, it reproduces that call's rows bit for bit.  A float32
 * row is the float64 row rounded once, at the store.
 * Both calls are enqueued on the handle's stream without a host wait; pending pipelined work is
 * ordered first, as for pscl_channel_device.  B = 0 returns PSCL_OK without a launch.  PSCL_EINVAL
 * for a NULL handle or payload, B < 0, frame0 < 0, every output NULL, rate <= 0 and a dtype flag
 * outside {0, 1}; PSCL_EUNSUP for B above 4 * (2^31 - 1) frames, what one launch covers.
 */
int pscl_encode_device(pscl_handle* h, const uint64_t* d_payload, int64_t B, uint64_t* d_msg, uint64_t* d_code,
                       void* d_sym, int sym_f32);
int pscl_channel_payload_device(pscl_handle* h, const uint64_t* d_payload, uint64_t seed, uint32_t stream_id,
                                double ebno_db, double rate, int64_t frame0, int64_t B, void* d_llr, int llr_f32,
                                uint64_t* d_msg);

/*
 * Uncoded BPSK baseline (run_fer_sweep.py:111-121, --include_uncoded) counted on the device:
 * per frame k_payload payload bits (the same Philox payload block as pscl_channel_device),
 * BPSK, AWGN with sigma^2 = 1 / (2 * 10^(ebno_db/10)) (rate 1), hard decision llr < 0.
 * Noise: Philox(frame, draw 0x40000000 + pair), independent of the coded frame's noise.
 * Adds frame errors (>= 1 wrong bit) to d_counters[PSCL_CNT_FRAME_ERR], bit errors to
 * [PSCL_CNT_BIT_ERR] and B to [PSCL_CNT_FRAMES] (int64[PSCL_NCOUNT], device).
 */
int pscl_uncoded_device(pscl_handle* h, uint64_t seed, uint32_t stream_id, double ebno_db, int k_payload,
                        int64_t frame0, int64_t B, int64_t* d_counters);

/*
 * NR rate matching (dl_scl_polar/nr/polar/...): after this call the handle's decode entry
 * points take E received LLRs per frame ([B][E]) and run decode_rate_matched_scl's front end
 * (scl_nr.py:38-57) inside the decode kernel: de-rate-match (rate_match.py:19-39, repeats
 * averaged; E <= N pads with -1.0) then sub-block de-interleave (interleaver.py:26-37).
 * pscl_channel_device then transmits the interleaved, repeated codeword (scl_nr.py:23-35).
 * E = 0 switches rate matching off.  Repetition (E > N) needs N >= 32.
 */
int pscl_set_rate_match(pscl_handle* h, int E);

/*
 * The front end above as a pass of its own, on a handle with pscl_set_rate_match(h, E), E > 0:
 *   d_llr [B][E] float64 received LLRs (rows 8-byte aligned, nothing more; odd E is legal)
 *   d_out [B][N] float64: the decoder-internal rows, subblock_deinterleave(derate_match_polar(row, N), N)
 *         (scl_nr.py:47-48), bit for bit what the decode kernels' fused staging computes: repeats summed
 *         in index order, then 0.0 + s (a -0 sum becomes +0), then the remainder copy, then one division
 *         by the count; E <= N pads with -1.0.  A plain handle (same N, information set, L, CRC) decodes
 *         d_out to the results the rate-matched handle gives on d_llr.
 * One kernel on the handle's stream, no host wait; pending pipelined work is ordered first.  Every N
 * and E pscl_set_rate_match accepts (only the N-vector is staged on chip, never the E-row).  B = 0
 * returns PSCL_OK without a launch.  PSCL_EINVAL for a NULL handle, B < 0, a NULL pointer with B > 0
 * and a handle without rate matching; PSCL_EUNSUP for B above 2^31 - 1, what one launch covers.
 */
int pscl_derate_match_device(pscl_handle* h, const double* d_llr, int64_t B, double* d_out);

/*
 * Staged de-rate-matching (default off).  With enable = 1 and rate matching on, four calls run the
 * pass above once into handle scratch and then the plain-row screening and SC kernels on its rows,
 * where today they refuse a rate-matched handle or fall back to the exact kernels alone:
 *   pscl_decode_device   plain calls (no forced bits, metrics, candidates, decision LLRs) whose
 *                        rate-matching-free twin (same N, information set, L, CRC, screening setting)
 *                        takes a screening kernel -- run-time sets at N = 128 .. 1024, L = 4 .. 32, and
 *                        the compiled-in (128,64) code: the pass, the twin's screening kernel on its
 *                        rows, and the exact re-decode of the deferred frames on the caller's rows, as
 *                        without the mode.  A handle with a rate-matched screening kernel of its own
 *                        (the compiled-in (128,88) code, L = 4, 8) keeps it, and a twin that is exact
 *                        anyway (L <= 2, N < 128, screening off) keeps today's path.
 *   pscl_sc_device       N = 32, 64, 256, 512, 1024: the pass, then the SC kernel (no PSCL_EUNSUP);
 *                        N = 128 keeps its fused kernel.
 *   pscl_escalate_device its dense gathered batch as pscl_decode_device.
 *   pscl_adaptive_async_device  N = 32 .. 1024 (no PSCL_EUNSUP): one pass, the SC stage on its rows,
 *                        stage 2's row-list screening decode on the same rows by row index, the exact
 *                        re-decode (or, where the twin's stage 2 is exact, stage 2 itself) on the
 *                        caller's rows.  On a pipelined handle the staged rows alternate two parities
 *                        with the list and count scratch.  A (128,88) handle at L = 4, 8 keeps today's path.
 * No other call consults the mode: the _f32 forms, the DL-SCL calls, pscl_retry_device,
 * pscl_adaptive_device, pscl_simulate*, pscl_decode and pscl_path_llrs_device behave as with it off.
 * Every output, counter and pscl_screening_count is bit-identical to the mode-off call on the same
 * rows.  The scratch grows to the largest B seen; a later call of the same size allocates nothing.
 * The setter orders pending pipelined work first; it may precede or follow pscl_set_rate_match and
 * has no effect while rate matching is off.
 *
 * pscl_rm_staged_stats: passes launched by those four calls and the rows they staged since the handle
 * was created (or the last reset = 1) -- the outputs being identical, the only sign that the staged
 * route ran.  pscl_derate_match_device is not counted.  Either pointer may be NULL.
 */
int pscl_set_rate_match_staged(pscl_handle* h, int enable);
int pscl_rm_staged_stats(pscl_handle* h, int64_t* passes, int64_t* rows, int reset);

/*
 * Decision LLRs of given paths (scl.py:158,166 info_llrs of a path whose bits are known):
 * for frame b with information bits d_bits[b] (frozen bits 0), the leaf LLR at every
 * information phase, recomputed top-down through the same f/g operations as the decoder
 * (bit-identical to the decoder's info_llrs for that path).  Device buffers, handle stream.
 *   d_llr [B][N] (or [B][E] with rate matching);  d_bits [B][W] uint64;  d_out [B][K] float64
 * Every N the handle takes: N <= 128 on the replay kernel of the DL-SCL post pass, N = 256, 512,
 * 1024 on the long replay kernel (one wavefront per row, the tree level in registers), plain and
 * rate-matched rows alike.  B <= 2^31 - 1; B = 0 returns at once.  The call synchronizes the
 * handle's stream once.  (float32 rows: pscl_path_llrs_device_f32, N = 128 only.)
 *
 * pscl_replay_stats: launches of the long replay kernel and the rows they were sized for since the
 * handle was created (or the last reset = 1), from pscl_path_llrs_device and from the DL-SCL chains
 * under PSCL_TUNE_DL_LONG_REPLAY -- there the only sign that the replay route ran.  Launches at
 * N <= 128 are not counted.  Either pointer may be NULL.
 */
int pscl_path_llrs_device(pscl_handle* h, const double* d_llr, int64_t B, const uint64_t* d_bits, double* d_out);
int pscl_replay_stats(pscl_handle* h, int64_t* launches, int64_t* rows, int reset);

/*
 * DL-SCL flip metric matrix (dl_scl_polar/dlscl/flip.py:104-106, checkpoints/beta_M*.npy):
 * beta [K][K] row-major float64 on the host (the reference's float32 checkpoint widened
 * exactly), or NULL to rank by |L0| alone (flip.py:107).  Applies to pscl_dlscl_device.
 */
int pscl_set_beta(pscl_handle* h, const double* beta);

/*
 * SCL + DL-SCL retries over a device batch: decode_with_retries (flip.py:65-141) for every
 * frame, as run_fer_sweep.py:89-109 uses it (baseline SCL counted, then DL-SCL counted).
 * Baseline SCL decode of all B frames; the frames whose best candidate fails the CRC are
 * retried up to min(retries, K) times, each retry flipping the untried information index
 * with the smallest q = |L0| @ beta (q = |L0| without beta; ties -> lower index), forcing
 * the reference prefix, and re-decoding; the loop stops at the first CRC pass.  L0 and the
 * reference bits follow the latest attempt's best path.  Enqueued on the handle's stream;
 * the call synchronizes once (to size the retry state by the number of failing frames) and
 * returns with the retry rounds queued behind it.
 *   d_best       [B][W] uint64 out: final attempt's best bits (flip.py:126,137)
 *   d_flags      [B] uint8 out: PSCL_FLAG_* of the final attempt
 *   d_attempts   NULL or [B] int32 out: 1 + flips tried
 *   d_tried      NULL or [B][tried_stride] int32 out: flip indices in order, -1 padded
 *   d_ref        NULL or [B][W] transmitted words: baseline statistics are added into
 *                d_counters_scl, final ones into d_counters_dl (both int64[PSCL_NCOUNT],
 *                required with d_ref); PSCL_CNT_RETRIES of d_counters_dl counts re-decodes
 * Requires a CRC (without one every baseline "passes", flip.py:84-86: results = baseline).
 */
int pscl_dlscl_device(pscl_handle* h, const double* d_llr, int64_t B, int retries, uint64_t* d_best,
                      uint8_t* d_flags, int32_t* d_attempts, int32_t* d_tried, int tried_stride,
                      const uint64_t* d_ref, int k_payload, int64_t* d_counters_scl, int64_t* d_counters_dl);

/*
 * Adaptive (list-size-escalating) decode of a device batch: successive cancellation first, the
 * list decoder only where its result fails the CRC.  Per frame
 *   1. u = sc_decode(llr, info_set) (dl_scl_polar/polar/polar.py:130-168: f = sign sign min and
 *      g = b +- a in fp64, frozen leaves 0, information leaves llr < 0); if check_crc(u)
 *      (crc.py:40-56) holds, the result is u with flags PSCL_FLAG_CRC_PASS | 0 and stage 1;
 *   2. otherwise the result is pscl_decode_device's for that frame (decode_scl with the handle's
 *      L and CRC, scl.py:108-209: bits, CRC flag, best index) and the stage is 2.
 * So the result is the composition of the two reference functions, bit for bit; it is not always
 * plain SCL's (an SC result that passes the CRC is kept even where the list would rank another
 * candidate first).  Stage 1 is one lane-parallel SC kernel over all B frames; the escalated rows
 * are gathered densely into handle scratch, decoded by the handle's plain-decode path (screening
 * decode plus exact re-decode) and scattered back.  Enqueued on the handle's stream; the call
 * synchronizes once, after stage 1, to read the escalated count that sizes stage 2 (none is
 * launched for a count of 0), and returns with stage 2 queued.  Pending pipelined work is ordered
 * first; the call itself is not pipelined.
 *   d_best     [B][W] uint64 out;  d_flags [B] uint8 out (both required)
 *   d_stage    NULL or [B] uint8 out: 1 or 2
 *   d_ref      NULL or [B][W] transmitted words: the final outputs' statistics are added into
 *              d_counters as pscl_decode_device adds them, plus the escalated count into
 *              d_counters[PSCL_CNT_ESCALATED] (d_counters is not touched without d_ref)
 *   n_escalated NULL or host out: frames handed to stage 2
 * PSCL_EINVAL without a CRC (every SC result would pass), for B < 0 or d_ref without d_counters;
 * PSCL_EUNSUP for N != 128.  Rate-matched handles take rows of E LLRs.
 */
int pscl_adaptive_device(pscl_handle* h, const double* d_llr, int64_t B, uint64_t* d_best, uint8_t* d_flags,
                         uint8_t* d_stage, const uint64_t* d_ref, int k_payload, int64_t* d_counters,
                         int64_t* n_escalated);

/*
 * The two halves of the adaptive decode as calls of their own, for every code length the SC
 * kernels cover.  A caller that enqueues the next batch's pscl_sc_device before this batch's
 * pscl_escalate_device keeps the device busy across the latter's host wait.
 *
 * pscl_sc_device: sc_decode (polar.py:130-168) + check_crc (crc.py:40-56) on every frame of a
 * device batch, one lane-parallel kernel on the handle's stream, no host wait.  Frame b gets
 * d_best[b] = u[info_set], d_flags[b] = PSCL_FLAG_CRC_PASS | 0 if the CRC holds (always without a
 * CRC, as the plain decode) else 0, d_stage[b] = 1 or 2 (d_stage may be NULL).  With d_ref the SC
 * results' statistics are added into d_counters as pscl_decode_device adds them (the SC baseline
 * curve).  Pending pipelined work is ordered first.
 *   N = 32, 64, 256, 512, 1024: plain rows of N LLRs.  N = 128: plain and rate-matched rows.
 * PSCL_EUNSUP for N < 32, and for a rate-matched handle with N != 128 (unless
 * pscl_set_rate_match_staged is on: the de-rate-matching pass then runs first).
 *
 * pscl_escalate_device: for every frame whose d_flags lacks PSCL_FLAG_CRC_PASS, d_best / d_flags
 * become exactly pscl_decode_device's outputs for that frame and d_stage 2; the other frames are
 * left alone.  The hand-off of pscl_adaptive_device: the failing frames are compacted, the call
 * waits once for their count, their rows are gathered, decoded as a dense plain batch and scattered
 * back.  With d_ref the final outputs of all B frames are counted, and the escalated count is added
 * into d_counters[PSCL_CNT_ESCALATED].  Any N and L pscl_decode_device accepts, rate-matched rows
 * included.  PSCL_EINVAL without a CRC.
 */
int pscl_sc_device(pscl_handle* h, const double* d_llr, int64_t B, uint64_t* d_best, uint8_t* d_flags,
                   uint8_t* d_stage, const uint64_t* d_ref, int k_payload, int64_t* d_counters);
int pscl_escalate_device(pscl_handle* h, const double* d_llr, int64_t B, uint64_t* d_best, uint8_t* d_flags,
                         uint8_t* d_stage, const uint64_t* d_ref, int k_payload, int64_t* d_counters,
                         int64_t* n_escalated);

/*
 * The adaptive decode without the host wait.  Per frame the results are pscl_adaptive_device's
 * (N = 128) and pscl_sc_device followed by pscl_escalate_device's (the other lengths): the
 * composition of sc_decode + check_crc and decode_scl, bit for bit.  Coverage is pscl_sc_device's:
 * N = 32 .. 1024 plain rows, N = 128 rate-matched rows too.
 * Everything is enqueued and the call returns: the SC stage over all B frames; the compaction of
 * the failing frames into a row list and a count in handle scratch; the list decode of "the first
 * count rows of the list, results at their rows", sized on the device -- the row-list screening
 * decode (N = 128 .. 1024, L = 4 .. 32) plus the exact re-decode of the frames it defers, or, where
 * the handle's plain decode is exact (L <= 2, N < 128, screening off), the exact kernel on the same
 * list; with d_ref the statistics of the final outputs of all B frames.  d_stage needs no marking:
 * the SC kernel writes 1 or 2.
 *   d_n_escalated  NULL or a device int32: receives the escalated count
 *   d_counters     with d_ref: the final outputs' statistics are added as pscl_decode_device adds
 *                  them, and the escalated count into d_counters[PSCL_CNT_ESCALATED]
 * Consecutive calls reuse the scratch in stream order.  On a pipelined handle
 * (pscl_set_pipelined >= 1) the SC stage and the compaction stay on the handle's stream, and the
 * rest -- list decode, re-decode, statistics, escalated count -- goes to one of two side streams,
 * where it overlaps the next call's SC stage and the previous call's rest; list and count scratch
 * and the side streams alternate two parities.  The
 * call's input, output and counter buffers then stay in use until pscl_join, pscl_sync, any other
 * entry point on the handle, or the second following pipelined call; consecutive pipelined calls
 * must not write the same output buffers.  Results are bit-identical to the non-pipelined form.
 * PSCL_EINVAL without a CRC, for B < 0, for d_ref without d_counters and for a missing d_llr /
 * d_best / d_flags; PSCL_EUNSUP for N < 32, rate matching at N != 128 (unless
 * pscl_set_rate_match_staged is on) and B > 2^31 - 1.
 */
int pscl_adaptive_async_device(pscl_handle* h, const double* d_llr, int64_t B, uint64_t* d_best, uint8_t* d_flags,
                               uint8_t* d_stage, const uint64_t* d_ref, int k_payload, int64_t* d_counters,
                               int32_t* d_n_escalated);

/*
 * Float32 rows.  The calls below take d_llr as [B][N] (or, on a rate-matched handle, [B][E])
 * float32 and otherwise the arguments of their float64 forms; pscl_decode_device_f32 is the plain
 * decode (no forced bits, metrics, candidates or decision LLRs).  Contract: every output -- d_best,
 * d_flags, d_stage, d_n_escalated, every counter added into d_counters, the deferred-frame count of
 * pscl_screening_count -- equals the float64 form's on the rows widened value by value
 * ((double)row[i], which is exact: float32 subnormals and -0 keep their value and sign), on a
 * pipelined handle too.  Rate-matched values are widened first, then summed and divided in float64;
 * nothing is summed in float32.  d_llr needs 4-byte alignment only (rows of an odd E start on
 * 4-byte boundaries).  Non-finite values are outside the contract, as for float64.  Whether a call's
 * rows are float32 is a property of that call alone: float64 and float32 calls may alternate on one
 * handle, pipelined or not.
 *
 * pscl_f32_available(h) is 1 where pscl_decode_device_f32, pscl_escalate_device_f32 and
 * pscl_adaptive_async_device_f32 have native kernels, else 0 (0 for a NULL handle): N = 128, L = 4 or
 * 8, screening on, the compiled-in (128,64) code on plain rows or the compiled-in (128,88) code on
 * rate-matched rows, PSCL_TUNE_LANE_EXACT at its default.  Where it is 0 those three return
 * PSCL_EUNSUP with a message that names the reason; the argument errors of the float64 forms come
 * first, with the same codes.  pscl_sc_device_f32 is the SC stage alone and takes every N = 128
 * handle (any information set, plain and rate-matched rows); PSCL_EUNSUP for other N.
 */
int pscl_f32_available(pscl_handle* h);
int pscl_decode_device_f32(pscl_handle* h, const float* d_llr, int64_t B, uint64_t* d_best, uint8_t* d_flags,
                           const uint64_t* d_ref, int k_payload, int64_t* d_counters);
int pscl_sc_device_f32(pscl_handle* h, const float* d_llr, int64_t B, uint64_t* d_best, uint8_t* d_flags,
                       uint8_t* d_stage, const uint64_t* d_ref, int k_payload, int64_t* d_counters);
int pscl_escalate_device_f32(pscl_handle* h, const float* d_llr, int64_t B, uint64_t* d_best, uint8_t* d_flags,
                             uint8_t* d_stage, const uint64_t* d_ref, int k_payload, int64_t* d_counters,
                             int64_t* n_escalated);
int pscl_adaptive_async_device_f32(pscl_handle* h, const float* d_llr, int64_t B, uint64_t* d_best, uint8_t* d_flags,
                                   uint8_t* d_stage, const uint64_t* d_ref, int k_payload, int64_t* d_counters,
                                   int32_t* d_n_escalated);

/*
 * One SNR point of a Monte-Carlo sweep with adaptive decoding, for global frames
 * [frame0, frame0 + B): pscl_channel_device (and the optional uncoded baseline) with the Philox
 * stream pscl_simulate uses -- shards add up exactly -- then the SC stage and the escalation of
 * pscl_adaptive_async_device, over chunks of up to 2^20 frames in handle scratch.  Counters are
 * ADDED into int64 [3][PSCL_NCOUNT]: row 0 the SC results of every frame (the SC baseline curve),
 * row 1 the final adaptive outputs with PSCL_CNT_ESCALATED, row 2 uncoded (include_uncoded).
 * The device form makes no host wait: stream-ordered on the handle's stream, d_counters zeroed by
 * the caller and complete once the stream has run.  The host form zeroes, enqueues, waits and
 * copies back.  Errors as pscl_adaptive_async_device's and pscl_channel_device's.
 */
int pscl_simulate_adaptive_device(pscl_handle* h, uint64_t seed, uint32_t stream_id, double ebno_db, double rate,
                                  int k_payload, int64_t frame0, int64_t B, int include_uncoded, int64_t* d_counters);
int pscl_simulate_adaptive(pscl_handle* h, uint64_t seed, uint32_t stream_id, double ebno_db, double rate,
                           int k_payload, int64_t frame0, int64_t B, int include_uncoded, int64_t* counters);

/*
 * Which path pscl_adaptive_async_device / pscl_simulate_adaptive[_device] took since the handle was
 * created (or the last reset = 1): stage-2 launches on a row-list screening kernel, stage-2
 * launches on an exact kernel, and the number of times those entry points blocked the host (a
 * scratch buffer that had to grow while side-stream work was pending; 0 after a warm-up call of
 * the same B).  Any output pointer may be NULL.
 */
int pscl_adaptive_stats(pscl_handle* h, int64_t* screened, int64_t* exact, int64_t* host_waits, int reset);

/*
 * DL-SCL retry rounds on a baseline the caller already holds: flip.py:88-141 for every frame whose
 * d_flags lacks PSCL_FLAG_CRC_PASS, the third building block next to pscl_sc_device and
 * pscl_escalate_device.  Precondition: for every such frame d_best / d_flags hold what the handle's
 * plain list decode returns for it -- pscl_decode_device, pscl_escalate_device and the adaptive
 * calls leave exactly that.  The retry chains are pscl_dlscl_device's (same flip metric, tie rule
 * and beta, pscl_set_beta; N > 128 decodes the listed frames again with decision-LLR history
 * first); a frame with the pass flag never enters one and keeps its d_best / d_flags / d_stage.
 *   d_attempts   NULL or [B] int32 out: 1 + flips tried (1 at the frames that do not enter)
 *   d_tried      NULL or [B][tried_stride] int32 out: flip indices in order, -1 padded
 *   d_stage      NULL or [B] uint8: 3 is written at every frame that enters a chain
 *   d_ref        NULL or [B][W] transmitted words: the final outputs' statistics are added into
 *                d_counters_dl (int64[PSCL_NCOUNT], required with d_ref) with PSCL_CNT_RETRIES
 * Enqueued on the handle's stream; the call synchronizes once, for the failing count that sizes
 * the chains.  On a pipelined handle pending work is ordered first and the call runs
 * stream-ordered.  Any N <= 1024, L and rate matching that pscl_dlscl_device takes.
 * PSCL_EINVAL without a CRC, for tried_stride < min(retries, K) and for d_ref without counters.
 */
int pscl_retry_device(pscl_handle* h, const double* d_llr, int64_t B, int retries, uint64_t* d_best, uint8_t* d_flags,
                      uint8_t* d_stage, int32_t* d_attempts, int32_t* d_tried, int tried_stride, const uint64_t* d_ref,
                      int k_payload, int64_t* d_counters_dl);

/*
 * Three-stage decode of a device batch: SC, the list decoder where SC fails the CRC, DL-SCL flips
 * where the list decoder fails it too.  Per frame
 *   u = sc_decode(llr); if check_crc(u): the result is u, stage 1, attempts 1;
 *   otherwise the result is decode_with_retries(llr) (flip.py:65-141, baseline decode_scl): stage 2
 *   and attempts 1 if that baseline passes the CRC, else stage 3 and attempts = 1 + flips tried.
 * The composition of the two reference functions, bit for bit (best bits, CRC flag, best index of
 * the final attempt, attempts, tried flips in order).  The baseline is pscl_adaptive_async_device's
 * launches, stream-ordered on the handle's stream (no side stream), then pscl_dlscl_device's
 * compaction, its one host wait for the failing count, and its retry chains; on a pipelined
 * handle the chains are deferred and overlap the next call as pscl_dlscl_device's do (same buffer
 * contract).  PSCL_TUNE_DL_CHUNKS does not apply (one chunk).
 *   d_counters     with d_ref, int64 [3][PSCL_NCOUNT], ADDED: row 0 the SC results, row 1 the adaptive
 *                  baseline with PSCL_CNT_ESCALATED, row 2 the final outputs with PSCL_CNT_RETRIES
 *   d_n_escalated  NULL or a device int32: receives the escalated count
 * retries <= 0 gives the adaptive result (stages 1 and 2, attempts 1).  Shapes and errors as
 * pscl_adaptive_async_device's (N = 32 .. 1024, rate-matched rows at N = 128 only, a CRC required),
 * and PSCL_EINVAL for tried_stride < min(retries, K).
 */
int pscl_adaptive_dlscl_device(pscl_handle* h, const double* d_llr, int64_t B, int retries, uint64_t* d_best,
                               uint8_t* d_flags, uint8_t* d_stage, int32_t* d_attempts, int32_t* d_tried,
                               int tried_stride, const uint64_t* d_ref, int k_payload, int64_t* d_counters,
                               int32_t* d_n_escalated);

/*
 * Flip labels of a device batch: the labelling loop of dl_scl_polar/train/make_dataset.py:52-91 for
 * every frame, with the frame's sent message in place of the reference's one all-zero-payload message.
 * It is NOT decode_with_retries: the flip order is fixed once from the baseline, every attempt forces
 * the BASELINE's prefix, and an attempt ends the chain only if it passes the CRC AND equals the sent
 * message.  Per frame
 *   1. the handle's plain list decode (pscl_decode_device's result).  A frame whose best candidate
 *      passes the CRC produces nothing.
 *   2. otherwise the frame is an ENTRY: abs_l0[k] = |(float)L0[k]|, L0 the decision LLRs of the
 *      baseline best path (pscl_path_llrs_device's values, bit for bit), narrowed to float32 once
 *      (round to nearest even) before the absolute value (make_dataset.py:66).
 *   3. the T = min(max_flips, K) information indices of smallest abs_l0, ascending; EQUAL VALUES
 *      RESOLVE TO THE LOWER INDEX.  (The rule is the engine's own: the reference's np.argsort is not
 *      stable, so its order on ties depends on the NumPy build; without ties the two agree.)
 *   4. for t = 0 .. T - 1: decode with the forced bits of flip.py:30-34 for idx_t -- the baseline bits
 *      at the indices below idx_t, the complement at idx_t, the rest free.  The first t whose best
 *      candidate passes the CRC and equals the frame's sent words gives flip = idx_t, rank = t, and
 *      the entry's chain stops.  If no t qualifies, flip = rank = -1.
 *   d_llr        [B][N] (or [B][E] with rate matching) float64
 *   d_sent       the sent message words: [W] with sent_stride = 0 (one message for all frames, the
 *                reference's case) or [B][W] with sent_stride = W (pscl_channel_device's d_msg)
 *   max_flips    1 .. 32 (the reference: 8)
 *   cap          entries the output arrays hold
 *   d_frame      [cap] int64 out: the frame index of entry e
 *   d_abs_l0     [cap][K] float32 out, for labelled and unrepaired entries alike
 *   d_flip       [cap] int32 out: the label, or -1
 *   d_rank       NULL or [cap] int32 out: its rank t, or -1
 *   d_counts     int64[PSCL_NLABEL] out, written (not added): PSCL_LBL_*
 *   n_entries    host out: A, the number of entries
 * Entries e < A are written in unspecified order (the compaction's, not frame order); rows >= A are
 * untouched.  The call makes one host wait, after the compaction, for A (pscl_dlscl_device's wait),
 * and enqueues everything else on the handle's stream without a host trip: the replay of the
 * baseline paths, the ranking, and per round the forced-bit decode of the live entries and the step
 * that labels the hits and builds the next round's force words -- the rounds' lists and counts stay
 * on the device.  If A > cap the call returns PSCL_EINVAL with *n_entries = A and no output written:
 * the caller allocates again and repeats.  On a pipelined handle pending work is ordered first and
 * the call runs stream-ordered, as pscl_retry_device.  Every N <= 1024, L and CRC pscl_dlscl_device
 * takes, rate-matched handles included; float64 rows only.  No knob changes a result.
 * PSCL_EINVAL without a CRC, for max_flips outside 1..32, B < 0, cap < 0, a sent_stride other than 0
 * or W, and a NULL required pointer with B > 0; PSCL_EUNSUP for B > 2^31 - 1.  B = 0 returns PSCL_OK
 * with zero counts and *n_entries = 0.
 */
#define PSCL_LBL_ENTRIES 0     /* frames whose baseline best candidate fails the CRC (A) */
#define PSCL_LBL_LABELLED 1    /* entries with a label */
#define PSCL_LBL_UNREPAIRED 2  /* entries without one (make_dataset's "failures") */
#define PSCL_LBL_DECODES 3     /* forced decodes run, summed over the rounds */
#define PSCL_NLABEL 4
int pscl_label_device(pscl_handle* h, const double* d_llr, int64_t B, const uint64_t* d_sent, int64_t sent_stride,
                      int max_flips, int64_t cap, int64_t* d_frame, float* d_abs_l0, int32_t* d_flip,
                      int32_t* d_rank, int64_t* d_counts, int64_t* n_entries);

/*
 * DL-SCL on float32 rows: the float32 contract above, carried on to the retry chains.  d_llr is
 * [B][N] (or [B][E]) float32, 4-byte aligned; the other arguments are those of the float64 forms.
 * Every output and every counter -- d_best, d_flags, d_stage, d_attempts, d_tried, d_n_escalated, each
 * counter block, d_out -- equals the float64 form's on the rows widened value by value, on a pipelined
 * handle too: a value is widened where a kernel loads it (rate-matched values first, then combined in
 * float64), and flip metric, tie rule (lower index), beta, warm start, stop rule and tried_stride are
 * the float64 forms'.  The row type belongs to the call: it is kept with the call's arguments, so the
 * chains a pipelined call leaves to the next call (or pscl_join) read the rows as their own call gave
 * them, and float64 and float32 calls may alternate on one handle.
 *
 * pscl_dlscl_device_f32, pscl_retry_device_f32 and pscl_adaptive_dlscl_device_f32 are native exactly
 * where pscl_f32_available(h) is 1.  The baseline is the float32 plain decode: pscl_decode_device_f32's
 * launches (at L = 4 too, where PSCL_TUNE_DL_LANE would move the float64 baseline to a kernel without a
 * float32 form; the results are the same by construction), pscl_adaptive_async_device_f32's
 * stream-ordered launches for the three-stage call, the caller's for pscl_retry_device_f32.  The retry
 * rounds are the default chain's instances over float rows: the screened lane-per-path retry decode
 * with its exact side chain ((128,64), plain rows), exact forced-bit rounds ((128,88), rate-matched
 * rows), and the post pass in its wide and narrow forms at 2 and 4 entries per wavefront.
 * PSCL_TUNE_DL_CHUNKS, PSCL_TUNE_DL_SPLIT, PSCL_TUNE_DL_SCREEN (and _MIN), PSCL_TUNE_DL_WARM_APX and
 * PSCL_TUNE_POST_EPW select among those and stay native.  Two knobs select an instance that was not
 * built over float rows and are refused: with PSCL_TUNE_DL_FUSED_POST = 1 or PSCL_TUNE_DL_RETRY_LANE = 2
 * on a (128,64) handle the three calls return PSCL_EUNSUP with a message that names the knob (nothing
 * else runs in its place, so pscl_path_stats stays truthful).  Elsewhere they return PSCL_EUNSUP with
 * pscl_decode_device_f32's message.  The float64 forms' argument errors come first, with the same
 * codes; PSCL_EINVAL without a CRC (pscl_dlscl_device_f32 too: a chain needs one).
 *
 * pscl_path_llrs_device_f32 is the decision-LLR replay from float32 rows; d_out stays float64 and
 * equals pscl_path_llrs_device's on the widened rows bit for bit.  It takes every N = 128 handle (any
 * information set, plain and rate-matched rows), as pscl_sc_device_f32; PSCL_EUNSUP for other N.
 */
int pscl_dlscl_device_f32(pscl_handle* h, const float* d_llr, int64_t B, int retries, uint64_t* d_best,
                          uint8_t* d_flags, int32_t* d_attempts, int32_t* d_tried, int tried_stride,
                          const uint64_t* d_ref, int k_payload, int64_t* d_counters_scl, int64_t* d_counters_dl);
int pscl_retry_device_f32(pscl_handle* h, const float* d_llr, int64_t B, int retries, uint64_t* d_best, uint8_t* d_flags,
                          uint8_t* d_stage, int32_t* d_attempts, int32_t* d_tried, int tried_stride,
                          const uint64_t* d_ref, int k_payload, int64_t* d_counters_dl);
int pscl_adaptive_dlscl_device_f32(pscl_handle* h, const float* d_llr, int64_t B, int retries, uint64_t* d_best,
                                   uint8_t* d_flags, uint8_t* d_stage, int32_t* d_attempts, int32_t* d_tried,
                                   int tried_stride, const uint64_t* d_ref, int k_payload, int64_t* d_counters,
                                   int32_t* d_n_escalated);
int pscl_path_llrs_device_f32(pscl_handle* h, const float* d_llr, int64_t B, const uint64_t* d_bits, double* d_out);

/*
 * One SNR point of a Monte-Carlo sweep with the three-stage decoder, for global frames
 * [frame0, frame0 + B): the TX (and the optional uncoded baseline) with the Philox stream of
 * pscl_simulate and pscl_simulate_adaptive -- shards add up exactly -- then
 * pscl_adaptive_dlscl_device, over chunks of up to 2^20 frames in handle scratch (pscl_simulate's
 * chunking; on a pipelined handle every chunk is one pipelined call).  Counters are ADDED into int64
 * [4][PSCL_NCOUNT]: rows SC, adaptive (PSCL_CNT_ESCALATED), final (PSCL_CNT_RETRIES), uncoded.
 * The device form's counters are zeroed by the caller and complete after pscl_join / pscl_sync; the
 * host form zeroes, enqueues, waits and copies back.
 */
int pscl_simulate_adaptive_dl_device(pscl_handle* h, uint64_t seed, uint32_t stream_id, double ebno_db, double rate,
                                     int k_payload, int64_t frame0, int64_t B, int retries, int include_uncoded,
                                     int64_t* d_counters);
int pscl_simulate_adaptive_dl(pscl_handle* h, uint64_t seed, uint32_t stream_id, double ebno_db, double rate,
                              int k_payload, int64_t frame0, int64_t B, int retries, int include_uncoded,
                              int64_t* counters);

/* Device scratch helpers so that non-torch callers can drive the device path. */
/*
 * One call per SNR point (the frame loop of run_fer_sweep.py:41-191 for global frames
 * [frame0, frame0 + B)): pscl_channel_device, the optional uncoded baseline
 * (pscl_uncoded_device) and SCL + DL-SCL (pscl_dlscl_device, beta from pscl_set_beta) over
 * chunks of up to 2^20 frames in handle scratch, counted on the device.  Synchronous.
 *   counters  out, host int64[3][PSCL_NCOUNT]: rows SCL, DL-SCL, uncoded (PSCL_CNT_* layout)
 * Counts depend only on (seed, stream_id, frame range): shards add up exactly.
 * Rate-matched handles (pscl_set_rate_match(E)) are supported: the TX writes and the decoders read
 * rows of E LLRs, and rate is then k_payload / E.
 */
int pscl_simulate(pscl_handle* h, uint64_t seed, uint32_t stream_id, double ebno_db, double rate, int k_payload,
                  int64_t frame0, int64_t B, int retries, int include_uncoded, int64_t* counters);

/*
 * pscl_simulate without the host round trip: the point is enqueued on the handle's stream and its
 * counters ADDED into d_counters (device int64 [3][PSCL_NCOUNT]: SCL, DL-SCL, uncoded; the caller
 * zeroes them).  On a pipelined handle (pscl_set_pipelined) the point's DL-SCL retry chains
 * overlap the next call's TX and baseline decode (run_fer_sweep's next SNR point); the counters
 * are complete after pscl_join / pscl_sync / any other entry point.  Results equal pscl_simulate's.
 */
int pscl_simulate_device(pscl_handle* h, uint64_t seed, uint32_t stream_id, double ebno_db, double rate, int k_payload,
                         int64_t frame0, int64_t B, int retries, int include_uncoded, int64_t* d_counters);

int pscl_device_alloc(pscl_handle* h, void** d_ptr, int64_t bytes);
/* (pscl_device_free first orders and completes the handle's pending pipelined work, which may
 * still use the buffer) */
int pscl_device_free(pscl_handle* h, void* d_ptr);
int pscl_memcpy_htod(pscl_handle* h, void* d_dst, const void* src, int64_t bytes);
int pscl_memcpy_dtoh(pscl_handle* h, void* dst, const void* d_src, int64_t bytes);
int pscl_memset_device(pscl_handle* h, void* d_dst, int value, int64_t bytes);

/*
 * Screening decode (default on).  Plain decodes (no metrics, candidates, decision LLRs, path
 * counts, forced bits) of the compiled-in N = 128 codes and of the long codes (N = 256..1024 at
 * L = 4, 8) run a screening pass whose path metrics carry a tail log1p(exp(-|v|)) with a
 * measured absolute error bound (fp32 exp2/log2; the bound checked exhaustively over every fp32
 * input on the device); every list ordering it decides must clear a margin of twice the N-term
 * metric error bound, and frames where one does not are re-decoded by the exact kernel.  Decoded
 * bits, CRC flags and best indices are identical to the exact decode (decode_scl,
 * dl_scl_polar/polar/scl.py:108-209).  enable = 0 runs the exact kernel only.
 */
int pscl_set_screening(pscl_handle* h, int enable);

/* Frames the last screening decode on this handle handed to the exact re-decode (synchronizes
 * the stream; 0 if no screening decode ran).  Diagnostic / test hook. */
int pscl_screening_count(pscl_handle* h, int64_t* count);

/*
 * Pipelined plain decodes (throughput mode; the reference's run_sweep frame loop,
 * run_fer_sweep.py:41-191, over a stream of independent batches).  With enable = 1 a plain
 * pscl_decode_device that takes the screening path leaves its exact re-decode of the deferred
 * frames on a second stream, where it overlaps the caller's next decode: when the call returns,
 * that re-decode is not yet ordered into the handle's stream.  Its input rows, output rows and
 * counters stay in use until pscl_join, pscl_sync, any other entry point on the handle (each
 * orders the pending re-decodes into the handle's stream first) or the second following
 * pipelined decode.  Consecutive pipelined decodes must not write the same output buffers.
 * pscl_dlscl_device (one chunk) likewise: a pipelined call enqueues its baseline decode, then the
 * previous pipelined call's retry rounds and DL counters (on high-priority streams, beside this
 * call's baseline), and leaves its own rounds to the next call or the join.  The retry chains of
 * consecutive calls alternate two stream sets, so they run beside each other.  enable = d in
 * 2..4 deepens the DL-SCL pipeline: a pscl_dlscl_device call's input, output and counter buffers
 * are free again at the d-th following pipelined call (enable = 1: the second), so a caller
 * cycling d output buffers lets the chains of up to d - 1 calls run behind the baselines.
 * Results are bit-identical to the non-pipelined form.  enable = 0 (default) restores
 * stream-ordered completion.  Timing (pscl_timing_*) of a pipelined decode covers its
 * screening launch only.  PSCL_EINVAL for enable outside 0..4.
 */
int pscl_set_pipelined(pscl_handle* h, int enable);
/* Order the pending pipelined re-decodes into the handle's stream (no host wait on the plain
 * decodes' re-decodes; a pending pipelined DL-SCL call's chains are enqueued here, which waits for
 * that call's baseline decode on the host to read its failing-frame count). */
int pscl_join(pscl_handle* h);

/*
 * Tuning and test knobs of one handle (value 0 restores the default, which is the measured best
 * schedule).  The library reads no environment variables: a knob changes only
 * the handle it is set on, never a result (every schedule is bit-identical).  Pending pipelined
 * work is ordered first.  PSCL_EINVAL for an unknown knob or a value out of range.
 *   PSCL_TUNE_DL_SCREEN     DL-SCL retry decodes on the forced-bit screening instance (where the
 *                           code has one): 1 always, 2 never, 0 (default) every retry chain, or
 *                           with PSCL_TUNE_DL_SCREEN_MIN set the chains it selects
 *   PSCL_TUNE_DL_CHUNKS     1..64: baseline chunks of a DL-SCL call (default 1)
 *   PSCL_TUNE_DL_SPLIT      1..2: retry chains per chunk (default 2; 1 when pipelined)
 *   PSCL_TUNE_SIDE_PRIORITY 1: a pipelined handle's side streams at normal priority (default high)
 *   PSCL_TUNE_POST_GRID     16..4096: workgroup cap of the DL-SCL post pass (default 512)
 *   PSCL_TUNE_RETRY_WPG     1..4: wavefronts per workgroup of the retry decodes (default: by LDS)
 *   PSCL_TUNE_DL_SCREEN_MIN 1..2^30: with PSCL_TUNE_DL_SCREEN = 0, screen only the retry chains of
 *                           at least this many entries and those beside a later baseline decode (a
 *                           pipelined call's or a chunk's); 0 (default): no threshold
 *   PSCL_TUNE_DL_LANE       1: a DL-SCL baseline decode (N = 128) on the lane-per-path screening
 *                           kernel (default); 2: on the two-lanes-per-path one
 *   PSCL_TUNE_DL_RETRY_LANE 2: screened retry decodes (N = 128) on the two-lanes-per-path forced-
 *                           bit instance instead of the lane-per-path one (default)
 *   PSCL_TUNE_DL_STREAMS    0..3 (bit mask): 1 the side chain on its main chain's stream, 2 one chain
 *                           set (consecutive calls' chains on the same streams, in call order)
 *   PSCL_TUNE_POST_PAIRS    1..32: entry pairs per wavefront the DL-SCL post pass grid is sized for
 *                           (default 2, PSCL_POST_PAIRS in dlscl.hip; capped by PSCL_TUNE_POST_GRID)
 *   PSCL_TUNE_TX_FUSED      pscl_simulate[_device] of the (128,64) code at L = 4, 8: 1 the baseline
 *                           decode draws its channel rows itself (the TX chain fused into the lane
 *                           kernel: no channel_kernel launch, no LLR rows written but those of
 *                           failing or deferred frames), 2 the separate TX launch; 0 (default):
 *                           the measured faster of the two
 *   PSCL_TUNE_DL_FUSED_POST 1: a screened retry round of the (128,64) code at L = 4, 8 runs its post
 *                           pass in the decode kernel (one launch per round; warm-start metrics
 *                           from the screening tail, deferred entries exact from phase 0); 2: the
 *                           separate dl_post_kernel; 0 (default): the measured faster
 *   PSCL_TUNE_POST_EPW      2 or 4: entries a wavefront of the DL-SCL post pass works on at once in
 *                           its narrow form (pipelined calls; 32 or 16 lanes per entry); 0 (default):
 *                           the measured faster
 *   PSCL_TUNE_LANE_EXACT    exact decodes of the (128,64) and NR (128,88) codes at L = 4, 8 -- the
 *                           deferred frames' re-decode and the exact DL-SCL retry rounds: 1 on the
 *                           exact lane-per-path kernel, 2 on the two-lanes-per-path exact kernel;
 *                           3 (tests) also every plain decode, unscreened; 0 (default): the measured
 *                           faster
 *   PSCL_TUNE_DL_WARM_APX   1: the screened DL-SCL chain's warm-start metrics from the screening tail
 *                           (the post pass skips the exact tails; entries its decodes defer start
 *                           the side chain's exact decode at phase 0), 2: exact warm-start metrics;
 *                           0 (default): the measured faster
 *   PSCL_TUNE_DL_TAIL       1: a pipelined DL-SCL call's baseline tail (the re-decode of its deferred
 *                           frames, the compaction of the failing ones) on the handle's stream, before
 *                           the next call's baseline; 0 (default): on a stream of its own beside it
 *   PSCL_TUNE_ADAPT_GRID    1..2^20: workgroup cap of pscl_adaptive_async_device's row-list launch
 *                           (its workgroups then stride over the list); 0 (default): a grid sized
 *                           for B, whose workgroups past the count exit at once -- the measured
 *                           faster
 *   PSCL_TUNE_DL_LONG_REPLAY 1: the long codes' DL-SCL chain (N = 256..1024: pscl_dlscl_device,
 *                           pscl_retry_device, pscl_adaptive_dlscl_device, pscl_simulate*, pipelined
 *                           handles) takes every attempt's L0 from the decision-LLR replay: no second
 *                           baseline decode, and retry decodes without history; 0 (default): the
 *                           decodes with history.  Every output and counter is bit-identical either
 *                           way (pscl_replay_stats tells them apart); no effect at N <= 128
 */
#define PSCL_TUNE_DL_SCREEN 1
#define PSCL_TUNE_DL_CHUNKS 2
#define PSCL_TUNE_DL_SPLIT 3
#define PSCL_TUNE_SIDE_PRIORITY 4
#define PSCL_TUNE_POST_GRID 5
#define PSCL_TUNE_RETRY_WPG 6
#define PSCL_TUNE_DL_LANE 7
#define PSCL_TUNE_DL_SCREEN_MIN 8
#define PSCL_TUNE_DL_RETRY_LANE 9
#define PSCL_TUNE_POST_PAIRS 10
#define PSCL_TUNE_DL_STREAMS 11
#define PSCL_TUNE_TX_FUSED 12
#define PSCL_TUNE_DL_FUSED_POST 13
#define PSCL_TUNE_POST_EPW 14
#define PSCL_TUNE_LANE_EXACT 15
#define PSCL_TUNE_DL_WARM_APX 16
#define PSCL_TUNE_DL_TAIL 17
#define PSCL_TUNE_ADAPT_GRID 18
#define PSCL_TUNE_DL_LONG_REPLAY 19
#define PSCL_TUNE_COUNT 20
int pscl_set_tuning(pscl_handle* h, int knob, int64_t value);

/*
 * Diagnostic: the metric tail log1p(exp(-|v|)) (scl.py:102-105) of n device values, evaluated
 * as the decode kernels do -- d_exact by the bit-exact glibc port, d_apx by the screening
 * decode's bounded-error form.  Device buffers, handle stream.
 */
int pscl_softplus_tails_device(pscl_handle* h, const double* d_v, int64_t n, double* d_exact, double* d_apx);

/*
 * Diagnostic (the screening margin's proof obligation): the absolute error of the screening
 * metric tail against the bit-exact glibc port for every fp32 bit pattern x32 in [lo, hi].
 * d_out[2] (device, zeroed by the caller): d_out[0] = fp64 bits of the largest error, d_out[1]
 * = (its high word << 32) | the x32 bit pattern of the largest error.  Handle stream.
 */
int pscl_tail_abs_scan_device(pscl_handle* h, uint32_t lo, uint32_t hi, uint64_t* d_out);

/*
 * The same scan for the bits form of the screening tail (the lane kernels' plain decodes):
 * max |pscl_tail2_f32(y32) - log1p(exp(-y32 ln 2)) / ln 2| over the fp32 bit patterns [lo, hi],
 * the reference being the bit-exact glibc port in fp64 (glibc_softplus.h).  Same output layout.
 */
int pscl_tail2_scan_device(pscl_handle* h, uint32_t lo, uint32_t hi, uint64_t* d_out);

/*
 * Kernel timing with HIP events recorded on the launch stream around every decode kernel
 * launch (enable = 1 starts a fresh accumulation).  pscl_timing_read returns the number of
 * timed launches and their summed duration in milliseconds (synchronizes the stream).
 */
int pscl_timing_enable(pscl_handle* h, int enable);
int pscl_timing_read(pscl_handle* h, int64_t* launches, double* total_ms);
/* The same, split by stream: launches on the handle's stream (a plain decode's screening pass,
 * a DL-SCL call's baseline decode) and on its side streams (DL-SCL retry decodes).  Side-stream
 * launches overlap main-stream ones, so the two sums are not additive in wall time.  Any output
 * pointer may be NULL. */
int pscl_timing_read_split(pscl_handle* h, int64_t* main_launches, double* main_ms, int64_t* side_launches,
                           double* side_ms);

/*
 * Host-side cost of the DL-SCL calls (pscl_dlscl_device, also through pscl_simulate[_device]):
 * the calls' summed wall time on the host, the part of it spent blocked in the one host wait a
 * call may make (its previous pipelined call's failing-frame count, a finished baseline decode),
 * and the number of calls -- so busy (enqueue) time = call_ms - wait_ms.  reset = 1 zeroes the
 * accumulators after reading.  Any output pointer may be NULL.
 */
int pscl_host_stats(pscl_handle* h, double* call_ms, double* wait_ms, int64_t* calls, int reset);

/*
 * Which schedules this handle has enqueued since it was created (tests assert the path they
 * mean to exercise ran): DL-SCL retry rounds whose post pass ran inside the screened retry
 * decode (PSCL_TUNE_DL_FUSED_POST), rounds with the separate dl_post_kernel, and pscl_simulate
 * blocks whose TX was fused into the baseline decode (PSCL_TUNE_TX_FUSED), dl_post_kernel
 * launches in the 4-entries-per-wavefront form (PSCL_TUNE_POST_EPW), and exact decodes launched on
 * the exact lane-per-path kernel (PSCL_TUNE_LANE_EXACT).  Any pointer may be NULL.
 */
int pscl_path_stats(pscl_handle* h, int64_t* fused_post_rounds, int64_t* post_rounds, int64_t* fused_tx_blocks,
                    int64_t* post_epw4_launches, int64_t* lane_exact_launches);

/*
 * The product's host (CPU) decoder: pscl_decode's contract and outputs (bit-identical) without a
 * GPU or a handle -- decode_scl (dl_scl_polar/polar/scl.py:108-209) for the reference's
 * CPU-only runs (BASELINE config 1: run_fer_sweep on CPU).  Any power-of-two N <= PSCL_MAX_N,
 * 1 <= L <= 255, crc_poly as pscl_create (0 = none); forced as pscl_decode ({-1, 0, 1} per info
 * bit, or NULL); bits, cands as int8 0/1.  Frames are split over `threads` host threads (0 = all
 * hardware threads).  PSCL_EINVAL for invalid arguments.  No HIP call is made.
 */
int pscl_decode_cpu(int N, const int32_t* info_set, int K, int L, uint64_t crc_poly, const double* llr, int64_t B,
                    const int8_t* forced, int32_t* n_paths, int8_t* best_bits, uint8_t* crc_pass, int32_t* best_idx,
                    double* metrics, int8_t* cands, double* info_llrs, int threads);

/*
 * pscl_path_llrs_device on the host, without a GPU or a handle: the decision LLRs out [B][K] of the
 * paths with information bits `bits` [B][K] (int8 0/1; frozen bits 0) on the decoder-internal rows
 * llr [B][N] (the de-rate-matched ones), bit-identical to pscl_decode_cpu's info_llrs of the
 * candidate with those bits.  Any power-of-two N <= PSCL_MAX_N; conventions as pscl_decode_cpu.
 * PSCL_EINVAL for invalid arguments; B = 0 is PSCL_OK.  No HIP call is made.
 */
int pscl_path_llrs_cpu(int N, const int32_t* info_set, int K, const double* llr, int64_t B, const int8_t* bits,
                       double* out, int threads);

/*
 * pscl_label_device's contract on the host, without a GPU or a handle, on pscl_decode_cpu's decoder
 * and pscl_path_llrs_cpu's replay (same narrowing, same order, ties to the lower index).  llr [B][N]
 * decoder-internal rows; sent int8 [K] (sent_stride = 0) or [B][K] (sent_stride = K).  Entries are in
 * frame order and the arrays are sized for B entries: frame [B] int64, abs_l0 [B][K] float32, flip [B]
 * int32, rank NULL or [B] int32 (rows at and above the entry count are untouched); counts
 * int64[PSCL_NLABEL], written.  A CRC is required.  Argument errors as pscl_label_device's
 * (PSCL_EINVAL); conventions as pscl_decode_cpu.  No HIP call is made.
 */
int pscl_label_cpu(int N, const int32_t* info_set, int K, int L, uint64_t crc_poly, const double* llr, int64_t B,
                   const int8_t* sent, int64_t sent_stride, int max_flips, int64_t* frame, float* abs_l0,
                   int32_t* flip, int32_t* rank, int64_t* counts, int threads);

/*
 * pscl_adaptive_device's contract on the host, without a GPU or a handle: sc_decode
 * (polar.py:130-168) + check_crc (crc.py:40-56) per frame, and decode_scl (scl.py:108-209, as
 * pscl_decode_cpu) for the frames that fail.  Any power-of-two N <= PSCL_MAX_N; a CRC is required
 * (PSCL_EINVAL without one).  best_bits [B][K] int8, crc_pass [B], best_idx [B] (0 at stage 1),
 * stage [B] (1 or 2); any output may be NULL.  No HIP call is made.
 */
int pscl_decode_adaptive_cpu(int N, const int32_t* info_set, int K, int L, uint64_t crc_poly, const double* llr,
                             int64_t B, int8_t* best_bits, uint8_t* crc_pass, int32_t* best_idx, uint8_t* stage,
                             int threads);

/*
 * pscl_encode_device's message and code words on the host, without a GPU or a handle: payload
 * [B][PSCL_WORDS(K - CRC degree)] uint64 -> msg [B][W] (attach_crc, crc.py:19-37) and code
 * [B][PSCL_WORDS(E or N)] (polar transform polar.py:17-29,106-119; E > 0: sub-block interleave and
 * rate matching, scl_nr.py:23-35; E = 0: none).  Either output may be NULL, not both.  info_set
 * and crc_poly as pscl_create.  PSCL_EINVAL for invalid arguments, PSCL_EUNSUP for E > N with
 * N < 32 and for a CRC degree above PSCL_MAX_CRC.  No HIP call is made.
 */
int pscl_encode_cpu(int N, const int32_t* info_set, int K, uint64_t crc_poly, int E, const uint64_t* payload,
                    int64_t B, uint64_t* msg, uint64_t* code);

/* Launch geometry used by the decode kernel (for roofline bookkeeping): waves per
 * workgroup, workgroups per launch for B frames, LDS bytes per workgroup. */
int pscl_launch_info(pscl_handle* h, int64_t B, int* waves_per_wg, int64_t* grid, int* lds_bytes);

#ifdef __cplusplus
}
#endif

#endif /* POLAR_SCL_H */
