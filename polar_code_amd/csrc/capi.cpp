// capi.cpp -- C ABI of libpolar_mi355x.so (declared in include/polar_scl.h).
//
// Host side of the engine: validates arguments with the reference's error semantics
// (scl.py:117-131, crc.py:40-49), precomputes the per-code constants (information mask,
// CRC syndrome/remainder columns, glibc exp table), owns device scratch and the stream,
// and launches the kernels in scl_kernels.hip.  Every handle entry point runs on the GPU and
// fails with PSCL_EDEVICE when no GPU is present; the product's host decoder for GPU-less runs
// is the handle-free pscl_decode_cpu (scl_cpu.cpp).
#include <hip/hip_runtime.h>
#include <math.h>

#include <cmath>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <chrono>
#include <string>
#include <utility>
#include <vector>

#include "polar_scl.h"
#include "scl_kernels.h"

namespace {

thread_local std::string g_err;

int fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

#define HIP_TRY(expr)                                                                     \
    do {                                                                                  \
        hipError_t _e = (expr);                                                           \
        if (_e != hipSuccess)                                                             \
            return fail(_e == hipErrorOutOfMemory ? PSCL_ENOMEM : PSCL_EDEVICE, "%s: %s", \
                        #expr, hipGetErrorString(_e));                                    \
    } while (0)

// a kernel-launch wrapper (pscl_launch_*): PSCL_EDEVICE and "<what> launch: <hip error string>"
#define LAUNCH_TRY(what, expr)                                                                               \
    do {                                                                                                     \
        hipError_t _e = (expr);                                                                              \
        if (_e != hipSuccess) return fail(PSCL_EDEVICE, what " launch: %s", hipGetErrorString(_e));          \
    } while (0)

#ifndef PSCL_BUILD_HASH
#define PSCL_BUILD_HASH "unhashed"
#endif
// marker + hash, found in the .so bytes by polar_code_amd/build.py's staleness check
__attribute__((used)) const char kBuildHash[] = "PSCL_BUILD_HASH=" PSCL_BUILD_HASH;

const uint64_t kExpTable[256] = {
#include "exp_table.inc"
};

// MSB-first bits of the polynomial value (crc.py:10-16); returns degree
int poly_degree(uint64_t poly) {
    int len = 0;
    for (uint64_t v = poly; v; v >>= 1) len++;
    return len - 1;
}

// remainder of bits[0..len) after the long division of crc.py (positions 0..len-deg-1
// are divided out); remainder bit i = buffer[len-deg+i]
uint32_t crc_remainder(const std::vector<uint8_t>& in, uint64_t poly, int deg) {
    std::vector<uint8_t> buf(in);
    const int len = (int)buf.size();
    for (int i = 0; i + deg < len; ++i) {
        if (!buf[i]) continue;
        for (int k = 0; k <= deg; ++k) buf[i + k] ^= (uint8_t)((poly >> (deg - k)) & 1);
    }
    uint32_t r = 0;
    for (int i = 0; i < deg; ++i)
        if (buf[len - deg + i]) r |= 1u << i;
    return r;
}

struct DevBuf {
    void* p = nullptr;
    size_t n = 0;
};

// an ordering event, created on first use
int record_event(hipEvent_t& ev, hipStream_t s) {
    if (!ev) HIP_TRY(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    HIP_TRY(hipEventRecord(ev, s));
    return PSCL_OK;
}

// stream `to` continues behind what `from` holds now
int hand_over(hipEvent_t& ev, hipStream_t from, hipStream_t to) {
    const int rc = record_event(ev, from);
    if (rc) return rc;
    HIP_TRY(hipStreamWaitEvent(to, ev, 0));
    return PSCL_OK;
}

// work on a side stream that the handle's stream, or the next user of a scratch parity, must later wait for
struct Pending {
    hipEvent_t ev = nullptr;
    bool on = false;
    int mark(hipStream_t s) {  // the work enqueued on s so far
        const int rc = record_event(ev, s);
        if (!rc) on = true;
        return rc;
    }
    int order(hipStream_t s) {  // s waits for it (no host wait)
        if (on) HIP_TRY(hipStreamWaitEvent(s, ev, 0));
        on = false;
        return PSCL_OK;
    }
    int host_wait() const {  // before the caller regrows a buffer that the work reads
        if (on) HIP_TRY(hipEventSynchronize(ev));
        return PSCL_OK;
    }
};

// depth of the DL-SCL pipeline (pscl_set_pipelined): a pipelined call's compaction output and, for
// pscl_simulate_device, its TX buffers are one of kDlPar sets, rewritten only after the retry chains
// of the call kDlPar back have ended -- the handle's stream runs up to kDlPar - 1 calls ahead of
// the chains (2 measured 175 M frames/s on the config-3 sweep, the stream waiting on chains of the
// low-SNR points)
constexpr int kDlPar = 4;
// retry-chain sets: the chains of consecutive pipelined calls (and of consecutive chunks of one
// call) alternate two sets of streams, events and state, so a call's chains run beside the previous
// call's instead of queueing behind them; each set holds the chain pair of one call (k = 0, 1 at
// index 2 set + k)
constexpr int kChainSets = 2, kChainStreams = 2 * kChainSets;

// The state buffers of one retry chain as (slot field, DlState member, bytes): c the chain's entry
// capacity, R = rounds + 1 lists, NS = PSCL_DL_NSEG buckets, W the message words
#define DL_CHAIN_FIELDS(X)                             \
    X(kChBcnt, bcnt, R * NS * PSCL_DL_CSTRIDE * 4)      \
    X(kChList0, list0, NS * c * 4)                      \
    X(kChList1, list1, NS * c * 4)                      \
    X(kChTried, tried, c * 16)                          \
    X(kChNt, nt, c * 4)                                 \
    X(kChForce, force, c * 2 * W * 8)                   \
    X(kChWarmMetric, warm_metric, c * NS * 8)           \
    X(kChWarmU, warm_u, c * 16)                         \
    X(kChOb, ob, c * W * 8)                             \
    X(kChOf, of, c)                                     \
    X(kChDcnt, dcnt, R * NS * PSCL_DL_CSTRIDE * 4)      \
    X(kChDlist, dlist, R * NS * c * 4)                  \
    X(kChOb2, ob2, c * W * 8)                           \
    X(kChOf2, of2, c)
// and of the long codes' dense-state chain (DlLongState): R2 = rounds + 2 passes, K information bits
#define DL_LONG_FIELDS(X)               \
    X(kLgAct1, act1, c * 8)             \
    X(kLgTried0, tried[0], c * W * 8)   \
    X(kLgTried1, tried[1], c * W * 8)   \
    X(kLgOb, ob, c * W * 8)             \
    X(kLgForce, force, c * 2 * W * 8)   \
    X(kLgNt0, nt[0], c * 4)             \
    X(kLgNt1, nt[1], c * 4)             \
    X(kLgCnt, cnt, R2 * 4)              \
    X(kLgOf, of, c)                     \
    X(kLgL0, l0, c * K * 8)
#define X(field, member, bytes) field,
enum ChainField { DL_CHAIN_FIELDS(X) kChainFields };
enum LongField { DL_LONG_FIELDS(X) kLongFields };
#undef X
enum ScreenField { kScrCount, kScrList, kScreenFields };  // deferred frames of a screening pass: int count, int64 rows
enum IoField { kIoRows, kIoMsg, kIoBest, kIoFlags, kIoFields };  // a simulate block: LLR rows, message and best words, flags
// an adaptive call without a host wait: the counts (deferred frames at int 0, escalated frames at int 16),
// the escalated frames' row list, the deferred frames' row list, the exact long-code kernel's workgroup scratch
enum AdaptField { kAdCounts, kAdEscList, kAdAmbList, kAdLongScratch, kAdaptFields };

// Scratch slots: every device buffer a handle grows on demand (ensure) has one name here, and the
// enum numbers them, so two buffers never share an index.  A family takes a block (first .. last) and
// is reached through its accessor below.  Beside each: who writes it, on which streams it is read,
// and what orders its reuse.  "main" is the handle's stream.
enum Slot : int {
    // decode_host (pscl_decode, pscl_sc_decode): a host call's staged inputs and outputs.  Main only, and the
    // call ends with a host wait.
    kHostLlr, kHostForce, kHostNPaths, kHostBest, kHostFlags, kHostMetrics, kHostCands, kHostInfoLlrs,
    // workgroup scratch of a long-code decode (scl_long.hip) launched on main: stream order
    kLongScratch,
    // ... of the long chain's retry decodes on retry stream 0 (they overlap the next chunk's baseline on
    // main, hence their own slot): that stream's order
    kLongRetryScratch,
    // [parity][ScreenField] a plain decode's screening pass writes them on main; the exact re-decode reads
    // them on main (parity 0) or, pipelined, on pipe_stream: parity p is reused after px[p]
    kScreen, kScreenLast = kScreen + 2 * kScreenFields - 1,
    // [parity][ScreenField] the same for a pipelined DL-SCL baseline, its re-decode on tail_stream: parity q is
    // reused after tail[q]
    kTailScreen, kTailScreenLast = kTailScreen + 2 * kScreenFields - 1,
    // [parity] per-wavefront count partials of a counting decode, zero between uses (the reduce clears
    // them).  0: every counting decode whose reduce follows it on its own stream, and pipelined plain
    // decodes of parity 0; 1: those of parity 1.  A pipelined plain decode's reduce runs on pipe_stream
    // behind its re-decode: parity p is reused after px[p]
    kCountPart, kCountPartLast = kCountPart + 1,
    // [parity] ... of a pipelined DL-SCL baseline, reduced on tail_stream: parity q is reused after tail[q]
    kTailCountPart, kTailCountPartLast = kTailCountPart + 1,
    // fused TX: the uncoded baseline's partials, reduced right behind the screening pass on its stream
    kTxUncPart,
    // escalate_failed (pscl_adaptive_device, pscl_escalate_device): count, frame list, dense rows, dense
    // best words, dense flags.  Main only; the call waits on the host for the count
    kEscCount, kEscList, kEscRows, kEscBest, kEscFlags,
    // pscl_path_llrs_device: the host-staged count and the identity row list.  Main only, host wait at the end
    kPathCount, kPathRows,
    // [parity][AdaptField] adaptive_escalate_enqueue: the compaction writes on main, stage 2 reads and
    // writes on main (unpipelined, parity 0) or on the parity's side stream (0 pipe_stream, 1 ad_stream):
    // parity q is reused after ad[q] (adaptive_begin)
    kAdapt, kAdaptLast = kAdapt + 2 * kAdaptFields - 1,
    // staged de-rate-matching: the decoder-internal rows of a stream-ordered call -- written and read on
    // main only, so one buffer serves a pipelined plain decode of any depth
    kRmRows,
    // [parity] ... of an adaptive call, which its stage 2 reads on the parity's side stream: reused after ad[q]
    kRmAdapt, kRmAdaptLast = kRmAdapt + 1,
    // [compaction parity] a DL-SCL chunk's failing-frame count and frame list: dl_compact writes them on
    // main or tail_stream, the host copy and the chunk's chains (retry streams) read them.  Parity p is
    // reused after dl[p] (pipelined calls, a ring of kDlPar) or ev_retry[p] (the chunks of one call, two)
    kDlCount, kDlCountLast = kDlCount + kDlPar - 1,
    kDlAct, kDlActLast = kDlAct + kDlPar - 1,
    // [chain 2 set + k][ChainField] a retry chain's state, on retry stream and side stream 2 set + k alone
    // (ev_scr / ev_def order the two): calls and chunks that share a set share its streams, in stream order
    kChain, kChainLast = kChain + kChainStreams * kChainFields - 1,
    // [LongField] the long codes' single chain, on retry stream 0: stream order
    kLong, kLongLast = kLong + kLongFields - 1,
    // [DL-SCL call parity][IoField] simulate_enqueue: the TX launch writes rows and messages on main, the
    // baseline (main, tail_stream) and the chains (retry streams) read and write them.  Parity par is
    // reused after dl[par], kDlPar calls later (dl_back = kDlPar for these calls)
    kSim, kSimLast = kSim + kDlPar * kIoFields - 1,
    // [IoField] simulate_adaptive_enqueue: main only, consecutive chunks in stream order
    kSimAd, kSimAdLast = kSimAd + kIoFields - 1,
    // the host forms' device counters (pscl_simulate, pscl_simulate_adaptive, pscl_simulate_adaptive_dl): the
    // call joins the pipelined work and waits on the host before it returns
    kSimCounters, kSimAdCounters, kSimAdDlCounters,
    // pscl_label_device: the baseline's best words and flags, the compaction's count and frame list, the
    // replayed L0 and the flip order by entry, the rounds' dense state (entry ids and LLR rows ping-ponged,
    // force words, result words and flags) and their counts.  Main only, in stream order; sized after the
    // call's host wait, when the stream is idle
    kLblBest, kLblFlags, kLblCount, kLblAct, kLblL0, kLblOrder, kLblEnt0, kLblEnt1, kLblRow0, kLblRow1, kLblForce,
    kLblOb, kLblOf, kLblCnt,
    kSlotCount
};
static_assert(kChainFields == 14 && kLongFields == 10, "a state buffer was added: size it in its table");
static_assert(kTailScreen - kScreen == 2 * kScreenFields && kRmRows - kAdapt == 2 * kAdaptFields, "two parities each");
static_assert(kDlAct - kDlCount == kDlPar && kChain - kDlAct == kDlPar, "one compaction buffer pair per DL-SCL parity");
static_assert(kLong - kChain == kChainStreams * kChainFields, "one state block per retry chain");
static_assert(kSim - kLong == kLongFields && kSimAd - kSim == kDlPar * kIoFields, "one I/O set per DL-SCL parity");
constexpr int slot_screen(bool tail, int parity, int field) { return (tail ? kTailScreen : kScreen) + parity * kScreenFields + field; }
constexpr int slot_count_part(bool tail, int parity) { return (tail ? kTailCountPart : kCountPart) + parity; }
constexpr int slot_adapt(int parity, int field) { return kAdapt + parity * kAdaptFields + field; }
constexpr int slot_rm_adapt(int parity) { return kRmAdapt + parity; }
constexpr int slot_dl_count(int parity) { return kDlCount + parity; }
constexpr int slot_dl_act(int parity) { return kDlAct + parity; }
constexpr int slot_chain(int chain, int field) { return kChain + chain * kChainFields + field; }
constexpr int slot_sim(int parity, int field) { return kSim + parity * kIoFields + field; }

}  // namespace

// the arguments of a pscl_dlscl_device call (kept for a pipelined call's deferred chains)
struct pscl_dl_call {
    const double* d_llr = nullptr;
    int64_t B = 0;
    int rounds = 0;
    uint64_t* d_best = nullptr;
    uint8_t* d_flags = nullptr;
    int32_t* d_attempts = nullptr;
    int32_t* d_tried = nullptr;
    int tried_stride = 0;
    const uint64_t* d_ref = nullptr;
    int k_payload = 0;
    int64_t* d_counters_dl = nullptr;
    int64_t nch = 1, cap = 0;
    int nsplit = 2, pbase = 0;
    bool pipe = false;
    int mode = 0;                 // the baseline (DlBase): 0 the list decode, 1 adaptive, 2 the caller's
    uint8_t* d_stage = nullptr;   // (modes 1, 2) 3 at every frame that enters a chain
    bool row_f32 = false;         // d_llr points at float32 rows (the pscl_*_f32 forms): the type of this
                                  // call's rows, kept with its arguments for the chains enqueued later
};

struct pscl_handle {
    int device = 0;
    int N = 0, n = 0, K = 0, L = 0, W = 1, crc_deg = 0;
    uint64_t crc_poly = 0;
    uint64_t info_mask[2] = {0, 0};   // phases 0..127 (the N <= 128 kernels)
    std::vector<uint64_t> info_words;  // [N/64 or 1] every phase (scl_long.hip)
    uint64_t* d_info_words = nullptr;
    std::vector<int32_t> info_set;
    std::vector<uint32_t> check_cols;   // [K]
    std::vector<uint32_t> attach_cols;  // [K - deg]
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;
    uint32_t* d_check_cols = nullptr;
    uint32_t* d_attach_cols = nullptr;
    int32_t* d_info_set = nullptr;
    uint64_t* d_exp_table = nullptr;
    int rm_E = 0;                     // NR rate matching (0 = off)
    int32_t* d_rm_src = nullptr;      // [N] de-interleave gather index
    int32_t* d_rm_order = nullptr;    // [N] interleaver order
    DevBuf scratch[kSlotCount];       // (enum Slot)
    hipStream_t retry_stream[kChainStreams] = {};  // DL-SCL retry chains: [2 set + k], chain k of a call
    hipStream_t side_stream[kChainStreams] = {};   // their deferred-entry work (PSCL_TUNE_DL_SCREEN)
    // the side streams of the other pipelining mode (their priority differs, create_priority_stream),
    // kept across pscl_set_pipelined switches: a stream creation costs ~0.5 ms of host time
    hipStream_t stash_pipe = nullptr, stash_retry[kChainStreams] = {}, stash_side[kChainStreams] = {};
    hipEvent_t ev_scr[kChainStreams] = {}, ev_def[kChainStreams] = {};
    hipEvent_t ev_base[kDlPar] = {}, ev_retry[kDlPar] = {}, ev_join[kChainSets] = {};
    int32_t* h_count = nullptr;          // pinned: failing-frame counts of the chunk parities
    int32_t* h_adapt = nullptr;          // pinned: escalated-frame count of pscl_adaptive_device
    int32_t* h_label = nullptr;          // pinned: entry count of pscl_label_device
    double* d_beta = nullptr;         // [K][K] DL-SCL flip metric (null = |L0|)
    float* d_beta32g[2] = {nullptr, nullptr};  // K = 64: fp32 beta, [K][G][K / G] for G = 8, 4 (fused post)
    std::vector<float> beta32g_host;
    double beta_absmax = 0.0;         // max |beta| (dl_post_kernel's certificate)
    std::vector<double> beta_host;    // staging of the last pscl_set_beta upload (stream-ordered copy)
    uint64_t* d_epi = nullptr;        // scl128 epilogue tables (gather + syndrome)
    uint64_t* d_xtab = nullptr;       // TX: codeword of each message byte value
    uint32_t* d_crctab = nullptr;     // TX: CRC remainder of each payload byte value
    int epi_words = 0;
    bool timing = false;
    bool screen = true;               // screening decode for plain decodes (pscl_set_screening)
    bool screened = false;            // a screening decode ran (scratch screened_slot holds its count)
    int screened_slot = slot_screen(false, 0, kScrCount);
    // pipelined plain decodes (pscl_set_pipelined): a screening decode's exact re-decode runs on
    // pipe_stream and overlaps the caller's next decode; the two alternate scratch parities, px[p]
    // marks the end of parity p's re-decode, and every other entry point, and pscl_join, order the
    // pending re-decodes back into the handle's stream
    bool pipelined = false;
    hipStream_t pipe_stream = nullptr;
    hipEvent_t ev_pscr[2] = {nullptr, nullptr};
    Pending px[2];
    int pipe_par = 0;
    // pipelined pscl_dlscl_device: the baseline's tail (the exact re-decode of its deferred frames,
    // the compaction of the failing frames and their count for the host) runs on tail_stream, so the
    // next call's baseline starts right after this call's screening pass; two scratch parities,
    // tail[q] marks the end of parity q's tail
    hipStream_t tail_stream = nullptr;
    hipEvent_t ev_tscr[2] = {nullptr, nullptr};
    Pending tail[2];
    // pipelined pscl_dlscl_device: a call's retry chains (and its DL counters) stay on the retry
    // streams and overlap the next call's baseline decode; the calls alternate the compaction
    // parity, dl[p] marks the end of parity p's chains
    Pending dl[kDlPar];
    int dl_par = 0;
    // how many calls back a pipelined call's own buffers may still be in use: for the caller's
    // buffers the depth of pscl_set_pipelined (2 by default: free again at the second following
    // call), kDlPar for pscl_simulate_device's own scratch sets
    int dl_back = 2;
    pscl_dl_call dl_defer;            // the last pipelined call, its chains not yet enqueued
    int dl_last_mode = 0;             // baseline mode of the last DL-SCL call (a change joins everything first)
    bool dl_defer_valid = false;
    std::vector<hipEvent_t> ev_pool;
    std::vector<uint8_t> ev_main;     // per timed launch: 1 if it ran on the handle's stream
    size_t ev_used = 0;
    int64_t tune[PSCL_TUNE_COUNT] = {};  // pscl_set_tuning knobs (0 = the default schedule)
    double host_call_ms = 0.0, host_wait_ms = 0.0;  // pscl_host_stats
    int64_t host_calls = 0;
    int64_t n_fpost_rounds = 0, n_post_rounds = 0, n_fused_tx = 0, n_post_epw4 = 0, n_lane_exact = 0;  // pscl_path_stats
    // pscl_adaptive_async_device on a pipelined handle: stage 2 (the row-list decode, its re-decode, the
    // statistics) runs on a side stream behind ev_adc[q] and overlaps the next call's SC stage; list
    // and count scratch alternate two parities, and so do the side streams (parity 0 pipe_stream,
    // parity 1 ad_stream): the latency-bound re-decode tails of consecutive calls run beside each
    // other, as on two handles.  ad[q] marks the end of parity q's stage 2
    hipStream_t ad_stream = nullptr;
    hipEvent_t ev_adc[2] = {nullptr, nullptr};
    Pending ad[2];
    int ad_par = 0;
    int64_t n_regrow = 0;  // scratch buffers freed and regrown (each drains the side streams on the host)
    int64_t n_ad_screened = 0, n_ad_exact = 0, n_ad_waits = 0;  // pscl_adaptive_stats
    // staged de-rate-matching (pscl_set_rate_match_staged): pscl_decode_device, pscl_sc_device,
    // pscl_escalate_device and pscl_adaptive_async_device write a rate-matched batch's decoder-internal
    // rows once (derate.hip) and run the plain-row screening and SC kernels on them (scratch kRmRows,
    // kRmAdapt)
    bool rm_staged = false;
    int64_t n_rm_passes = 0, n_rm_rows = 0;  // pscl_rm_staged_stats
    int64_t n_replay_launches = 0, n_replay_rows = 0;  // pscl_replay_stats (the long replay kernel)
};

namespace {

// the handle's side streams: the live ones (null where no call has needed one yet), then the stashed
// ones of the other pipelining mode (drained before they were stashed)
constexpr int kLiveStreams = 3 + 2 * kChainStreams, kSideStreams = kLiveStreams + 1 + 2 * kChainStreams;
struct SideStreams {
    hipStream_t* s[kSideStreams];
};
SideStreams side_streams(pscl_handle* h) {
    SideStreams l = {{&h->pipe_stream, &h->tail_stream, &h->ad_stream}};
    int n = 3;
    for (int i = 0; i < kChainStreams; ++i) l.s[n++] = &h->retry_stream[i], l.s[n++] = &h->side_stream[i];
    l.s[n++] = &h->stash_pipe;
    for (int i = 0; i < kChainStreams; ++i) l.s[n++] = &h->stash_retry[i], l.s[n++] = &h->stash_side[i];
    return l;
}

// every stream the handle's pipelined work may still run on, drained (before a scratch buffer is
// freed and regrown)
void quiesce(pscl_handle* h) {
    const SideStreams l = side_streams(h);
    for (int i = 0; i < kLiveStreams; ++i)
        if (*l.s[i]) hipStreamSynchronize(*l.s[i]);
}

// destroy the side streams (after draining them) so the next use creates them with the priority
// the handle's current mode asks for (create_priority_stream)
void drop_side_streams(pscl_handle* h) {
    quiesce(h);
    const SideStreams l = side_streams(h);
    for (hipStream_t* s : l.s) {
        if (*s) hipStreamDestroy(*s);
        *s = nullptr;
    }
}

int ensure(pscl_handle* h, int slot, size_t bytes, void** out) {
    DevBuf& b = h->scratch[slot];
    if (b.n < bytes) {
        if (b.p) {
            quiesce(h);  // (pipelined work may still read it)
            hipFree(b.p);
            h->n_regrow++;
        }
        b.p = nullptr;
        b.n = 0;
        size_t want = bytes + bytes / 2;  // geometric growth: varying batch sizes settle quickly
        if (want < 4096) want = 4096;
        HIP_TRY(hipMalloc(&b.p, want));
        b.n = want;
    }
    *out = b.p;
    return PSCL_OK;
}

template <class T>
int ensure_as(pscl_handle* h, int slot, size_t bytes, T*& out) {
    void* p;
    const int rc = ensure(h, slot, bytes, &p);
    out = (T*)p;
    return rc;
}

int set_device(pscl_handle* h) {
    HIP_TRY(hipSetDevice(h->device));
    return PSCL_OK;
}

// the handle's stream waits for the pending pipelined work (no host wait): what = 1 the plain
// decodes' re-decodes and the adaptive calls' second stages, 2 the DL-SCL retry chains, 3 both;
// + 8: not the adaptive calls' (a pipelined pscl_adaptive_async_device orders those by parity)
// (dl_enqueue_deferred ends in launch_decode, which joins: the one forward declaration)
int dl_enqueue_deferred(pscl_handle* h, bool beside = false);

int join_pipe(pscl_handle* h, int what = 3) {
    int rc;
    if ((what & 2) && (rc = dl_enqueue_deferred(h))) return rc;  // a pipelined DL-SCL call's chains, enqueued first
    if (what & 2)
        for (Pending& m : h->tail)
            if ((rc = m.order(h->stream))) return rc;
    if ((what & 1) && !(what & 8))
        for (Pending& m : h->ad)
            if ((rc = m.order(h->stream))) return rc;
    if (what & 1)
        for (Pending& m : h->px)
            if ((rc = m.order(h->stream))) return rc;
    if (what & 2)
        for (Pending& m : h->dl)
            if ((rc = m.order(h->stream))) return rc;
    return PSCL_OK;
}

// a side stream; on a pipelined handle of the highest priority: latency-bound chains (retry
// rounds, deferred re-decodes) take workgroup slots ahead of the next call's throughput-bound
// baseline decode (measured, config 4 pipelined: 3.55 ms against 4.0 at equal priority).  Not
// otherwise: the FER sweep's two concurrent handles lose from it (4.0 dB point 16.6 -> 25.8 ms)
hipError_t create_priority_stream(pscl_handle* h, hipStream_t* s) {
    int least = 0, greatest = 0;
    if (hipDeviceGetStreamPriorityRange(&least, &greatest) != hipSuccess) greatest = least = 0;
    const bool plain = h->tune[PSCL_TUNE_SIDE_PRIORITY] == 1;  // (tuning knob: normal priority)
    return hipStreamCreateWithPriority(s, hipStreamNonBlocking, h->pipelined && !plain ? greatest : least);
}

// entry points other than a pipelined plain decode: device, then the pending re-decodes
int enter(pscl_handle* h) {
    const int rc = set_device(h);
    return rc ? rc : join_pipe(h);
}

void fill_decode_params(const pscl_handle* h, pscl_decode_params& P, int hist) {
    memset(&P, 0, sizeof(P));
    P.N = h->N;
    P.n = h->n;
    P.K = h->K;
    P.L = h->L;
    P.W = h->W;
    P.info_mask[0] = h->info_mask[0];
    P.info_mask[1] = h->info_mask[1];
    P.info_words = h->d_info_words;
    P.crc_cols = h->d_check_cols;
    P.info_set = h->d_info_set;
    P.has_crc = h->crc_poly != 0;
    P.exp_table = h->d_exp_table;
    P.epi_table = h->d_epi;
    P.epi_words = h->epi_words;
    P.rm_E = h->rm_E;
    P.rm_src = h->d_rm_src;
    pscl_decode_layout(P, hist);
}

// a counting decode (P.ref) whose kernel stores per-wavefront counts: their buffer (scratch kCountPart,
// kTailCountPart)
// A (re)allocated buffer is zeroed on the decode's own stream st: a plain hipMemset runs on the null
// stream, which the handle's non-blocking streams do not wait for -- the decode could store (and its
// reduce read) partials before the zeroing lands (an intermittent counter mismatch)
int with_count_slots(pscl_handle* h, pscl_decode_params& P, int hist, int slot, hipStream_t st) {
    P.cpart = nullptr;
    const int64_t slots = pscl_decode_count_slots(P, hist);
    if (slots <= 0) return PSCL_OK;
    void* d;
    const size_t had = h->scratch[slot].n;
    const int rc = ensure(h, slot, (size_t)slots * 16, &d);
    if (rc) return rc;
    if (h->scratch[slot].n != had) HIP_TRY(hipMemsetAsync(d, 0, h->scratch[slot].n, st));  // (then kept zero by the reduces)
    P.cpart = (int32_t*)d;
    return PSCL_OK;
}

// scr_slot: the scratch buffer of a long-code decode (decodes that may run concurrently on
// different streams need different slots)
// pipe: the caller is a plain pscl_decode_device on a pipelined handle (see pscl_handle)
// exact decodes on the exact lane-per-path instance where it applies (PSCL_TUNE_LANE_EXACT): off by
// default -- these launches are few frames, bound by one wavefront's latency, and one lane per path
// runs each path's tree updates serially where the two-lanes-per-path kernel splits them: re-decode
// 169 us against 99 us per 10^6-frame headline step, side-chain rounds 208 against 182 us
// (profiles/r06r_lane_exact_ab.txt)
#ifndef PSCL_LANE_EXACT_DEFAULT
#define PSCL_LANE_EXACT_DEFAULT 0
#endif
bool lane_exact_on(const pscl_handle* h) {
    const int64_t lx = h->tune[PSCL_TUNE_LANE_EXACT];
    return lx == 1 || lx == 3 || (lx == 0 && PSCL_LANE_EXACT_DEFAULT);
}

// float32 rows (the pscl_*_f32 entry points): why this handle's list decode has no float32 kernels, or
// null where it has -- the handles whose plain decode is the lane-per-path screening kernel plus the
// compiled-in exact re-decode (N = 128, L = 4 or 8, screening on, the (128,64) code on plain rows or the
// (128,88) code on rate-matched rows, no knob that moves a launch to another instance).  The flag that
// marks a launch's rows as float32 is per call (pscl_decode_params::f32; for the SC stage, which of the
// two launch functions is called), never handle state: every kernel argument block is copied when its
// launch is enqueued, so work deferred to a side stream keeps the type of its own call's rows.
const char* f32_unsupported(const pscl_handle* h) {
    if (h->N != PSCL_FAST_N) return "float32 rows are decoded at N = 128 only";
    if (h->L != 4 && h->L != 8) return "float32 rows are decoded at L = 4 and 8 only";
    if (!h->screen) return "float32 rows need the screening decode (pscl_set_screening is off)";
    if (h->tune[PSCL_TUNE_LANE_EXACT] == 3 || lane_exact_on(h))
        return "PSCL_TUNE_LANE_EXACT selects the exact lane-per-path instance, which has no float32 form";
    pscl_decode_params P;
    fill_decode_params(h, P, 0);
    if (!pscl_f32_decode_available(P))
        return h->rm_E ? "float32 rate-matched rows are decoded for the compiled-in (128,88) code only"
                       : "float32 plain rows are decoded for the compiled-in (128,64) code only (runtime information set)";
    return nullptr;
}

// the de-rate-matching pass (derate.hip) of B rate-matched rows on stream st: d_out, or (null) scratch
// slot `slot`, grown to the largest B seen; *rows gets where the [B][N] rows are.  count: one of the
// staged mode's passes (pscl_rm_staged_stats)
int launch_derate(pscl_handle* h, const double* d_llr, int64_t B, double* d_out, int slot, hipStream_t st, bool count,
                  const double** rows) {
    if (B > PSCL_DERATE_MAX_B) return fail(PSCL_EUNSUP, "B exceeds the %lld rows of one de-rate-matching launch", PSCL_DERATE_MAX_B);
    if (!d_out) {
        void* d;
        const int rc = ensure(h, slot, (size_t)B * (size_t)h->N * 8, &d);
        if (rc) return rc;
        d_out = (double*)d;
    }
    pscl_derate_params D;
    memset(&D, 0, sizeof(D));
    D.llr = d_llr;
    D.out = d_out;
    D.B = B;
    D.n = h->n;
    D.E = h->rm_E;
    LAUNCH_TRY("de-rate-matching", pscl_launch_derate(D, st));
    if (count) {
        h->n_rm_passes++;
        h->n_rm_rows += B;
    }
    if (rows) *rows = d_out;
    return PSCL_OK;
}

// the handle's rate-matching-free twin in a block: P on plain rows (layout recomputed)
void plain_twin(pscl_decode_params& P, const double* rows, int hist) {
    P.llr = rows;
    P.rm_E = 0;
    P.rm_src = nullptr;
    pscl_decode_layout(P, hist);
}

// a timed interval of pscl_timing_read_split from ev_pool: its start recorded on st (noted as main or
// side), *e1 for the caller to record at its end; null with timing off
int timed_begin(pscl_handle* h, hipStream_t st, hipEvent_t* e1) {
    *e1 = nullptr;
    if (!h->timing) return PSCL_OK;
    while (h->ev_pool.size() < h->ev_used + 2) {
        hipEvent_t e;
        HIP_TRY(hipEventCreate(&e));
        h->ev_pool.push_back(e);
    }
    if (h->ev_main.size() < h->ev_pool.size() / 2) h->ev_main.resize(h->ev_pool.size() / 2);
    h->ev_main[h->ev_used / 2] = st == h->stream ? 1 : 0;
    *e1 = h->ev_pool[h->ev_used + 1];
    h->ev_used += 2;
    HIP_TRY(hipEventRecord(h->ev_pool[h->ev_used - 2], st));
    return PSCL_OK;
}

// tail (a pipelined DL-SCL baseline, tail_par its scratch parity): the re-decode of the deferred
// frames goes to tail after the screening pass, and the call returns; the caller queues the rest of
// the baseline's tail there and marks it with tail[tail_par]
// rm_stage (pscl_decode_device and pscl_escalate_device on a staged handle): a plain decode of
// rate-matched rows that has no screening kernel of its own, but whose rate-matching-free twin has,
// runs the de-rate-matching pass into scratch and the twin's screening kernel on those rows; the exact
// re-decode of the deferred frames reads the caller's rows with rm_E, as without the mode
int launch_decode(pscl_handle* h, const pscl_decode_params& P0, int hist, hipStream_t st = nullptr, int scr_slot = kLongScratch,
                  bool pipe = false, hipStream_t tail = nullptr, int tail_par = 0, bool rm_stage = false) {
    if (!st) st = h->stream;
    pscl_decode_params P = P0;
    if (P.long_mode) {  // global scratch of every workgroup in flight (scl_long.hip)
        void* d_scr;
        const int rc = ensure(h, scr_slot, (size_t)pscl_decode_grid(P) * (size_t)P.long_block_bytes, &d_scr);
        if (rc) return rc;
        P.long_scratch = (unsigned char*)d_scr;
    }
    int rc;
    hipEvent_t e1;
    if ((rc = timed_begin(h, st, &e1))) return rc;
    // Plain decodes of the compiled-in N = 128 codes (no metrics, candidates, decision LLRs,
    // forced bits or row indirection requested) run as a screening decode plus an exact
    // re-decode of the frames it could not certify; the two launches count as one decode.
    // (long codes: the lane-per-path screening kernel, scl_lane_long.hip, N = 256..1024, L = 4, 8)
    pscl_decode_params T = P;
    T.apx = 1;
    const int64_t lx = h->tune[PSCL_TUNE_LANE_EXACT];  // the exact lane-per-path instance (knob 3: every frame)
    const bool plain = h->screen && lx != 3 && !hist && !P.metrics && !P.cands && !P.force && !P.sc_hard && !P.fidx &&
                       !P.d_count;
    bool screen = plain && (P.fast ? (pscl_screening_available(P) != 0 || pscl_lane_long128_available(T) != 0)
                                   : pscl_lane_long_available(T) != 0);
    bool staged = false;
    if (rm_stage && plain && !screen && h->rm_staged && P.rm_E && !P.f32 && !tail) {
        pscl_decode_params T2 = T;
        plain_twin(T2, nullptr, hist);
        staged = T2.fast ? (pscl_screening_available(T2) != 0 || pscl_lane_long128_available(T2) != 0)
                         : pscl_lane_long_available(T2) != 0;
        screen = staged;
    }
    hipError_t err;
    if (!(screen && pipe) && (rc = join_pipe(h, 1))) return rc;
    if (screen) {
        void *d_cnt, *d_list;
        // pipelined: parity p's list may still be read by the re-decode two calls back
        const int p = pipe ? h->pipe_par : 0;
        const bool tl = tail && !pipe;
        const int s_cnt = slot_screen(tl, tl ? tail_par : p, kScrCount), s_list = slot_screen(tl, tl ? tail_par : p, kScrList);
        if (pipe) {  // (the stream may exist already: a pipelined adaptive call shares it)
            if (!h->pipe_stream) HIP_TRY(create_priority_stream(h, &h->pipe_stream));
            h->pipe_par ^= 1;
        }
        if (tl || pipe) {  // (the parity's previous tail or re-decode still reads its list)
            Pending& prev = tl ? h->tail[tail_par] : h->px[p];
            if (h->scratch[s_list].n < (size_t)P.B * 8 && (rc = prev.host_wait())) return rc;  // (regrown)
            if ((rc = prev.order(st))) return rc;
        }
        if ((rc = ensure(h, s_cnt, 4, &d_cnt))) return rc;
        if ((rc = ensure(h, s_list, (size_t)P.B * 8, &d_list))) return rc;
        HIP_TRY(hipMemsetAsync(d_cnt, 0, 4, st));
        pscl_decode_params S = P;
        S.apx = 1;
        if (staged) {  // the pass, then the twin's screening kernel on its rows
            const double* rows;
            if ((rc = launch_derate(h, P.llr, P.B, nullptr, kRmRows, st, true, &rows))) return rc;
            plain_twin(S, rows, hist);
        }
        pscl_decode_layout(S, hist);  // (no exp table in LDS)
        S.amb_list = (int64_t*)d_list;
        S.amb_count = (int32_t*)d_cnt;
        // (pipelined: the count buffers alternate with the call parity, and the reduce runs on the
        // side stream after the re-decode, off the handle's stream)
        if ((rc = with_count_slots(h, S, hist, slot_count_part(tl, tl ? tail_par : p), st))) return rc;
        S.tx_upart = nullptr;
        if (S.tx && S.tx_unc_counters) {  // fused TX: the uncoded baseline's per-wavefront partials
            const int64_t slots = pscl_decode_count_slots(S, hist);
            void* du;
            const size_t had = h->scratch[kTxUncPart].n;
            if ((rc = ensure(h, kTxUncPart, (size_t)(slots > 0 ? slots : 1) * 16, &du))) return rc;
            if (h->scratch[kTxUncPart].n != had) HIP_TRY(hipMemsetAsync(du, 0, h->scratch[kTxUncPart].n, st));  // (then kept zero by the reduces)
            S.tx_upart = (int32_t*)du;
        }
        err = pscl_launch_decode(S, hist, st);
        if (err == hipSuccess && S.tx_upart)
            err = pscl_launch_count_reduce(S.tx_upart, pscl_decode_count_slots(S, hist), S.tx_unc_counters, st);
        if (err == hipSuccess && S.tx)  // fused TX: the deferred frames' rows, read by the exact re-decode
            err = pscl_launch_tx_rows(S, (const int64_t*)d_list, (const int32_t*)d_cnt, S.B, S.tx_rows, S.tx_frame0, st);
        h->screened = true;
        h->screened_slot = s_cnt;
#ifdef PSCL_APX_ABLATE
        // PSCL_DIAG_SCREEN_ONLY=1: timing diagnostics of the screening pass alone (variant
        // builds only, tools/build_variant.py -DPSCL_APX_ABLATE=..); deferred frames stay undecoded
        static const bool screen_only = getenv("PSCL_DIAG_SCREEN_ONLY") && atoi(getenv("PSCL_DIAG_SCREEN_ONLY")) == 1;
#else
        constexpr bool screen_only = false;  // the shipped library always re-decodes deferred frames
#endif
        if (err == hipSuccess && S.cpart && ((!pipe && !tl) || screen_only))
            err = pscl_launch_count_reduce(S.cpart, pscl_decode_count_slots(S, hist), S.counters, st);
        if (err == hipSuccess && !screen_only) {
            pscl_decode_params X = P;  // exact decode of the listed frames, outputs at their rows
            X.tx = 0;                  // (its rows are in HBM: loaded, or written by tx_rows_kernel)
            X.fidx = (const int64_t*)d_list;
            X.d_count = (const int32_t*)d_cnt;
            X.out_by_row = 1;
            X.lane_exact = lane_exact_on(h) ? 1 : 0;
            // few frames: one resident set of workgroups (4 waves/SIMD on 256 CUs), striding
            // over the listed frames, instead of a grid sized for the whole batch
            X.grid_cap = (int64_t)256 * 16 / (pscl_decode_wpg(X) > 0 ? pscl_decode_wpg(X) : 1);
            if (tl) {  // (the caller's tail stream: this call's baseline tail, off the handle's stream)
                if (e1) HIP_TRY(hipEventRecord(e1, st));
                if ((rc = hand_over(h->ev_tscr[tail_par], st, tail))) return rc;
                if (!hist && pscl_lane_exact_available(X)) h->n_lane_exact++;
                err = pscl_launch_decode(X, hist, tail);
                if (err == hipSuccess && S.cpart)  // (the screening's count partials, kTailCountPart)
                    err = pscl_launch_count_reduce(S.cpart, pscl_decode_count_slots(S, hist), S.counters, tail);
                if (err != hipSuccess) return fail(PSCL_EDEVICE, "decode kernel launch: %s", hipGetErrorString(err));
                return PSCL_OK;
            }
            if (pipe) {
                // the re-decode overlaps the caller's next decode; the timed interval is the
                // screening launch alone
                if (e1) HIP_TRY(hipEventRecord(e1, st));
                if ((rc = hand_over(h->ev_pscr[p], st, h->pipe_stream))) return rc;
                if (!hist && pscl_lane_exact_available(X)) h->n_lane_exact++;
                err = pscl_launch_decode(X, hist, h->pipe_stream);
                if (err == hipSuccess && S.cpart)
                    err = pscl_launch_count_reduce(S.cpart, pscl_decode_count_slots(S, hist), S.counters, h->pipe_stream);
                if (err != hipSuccess) return fail(PSCL_EDEVICE, "decode kernel launch: %s", hipGetErrorString(err));
                return h->px[p].mark(h->pipe_stream);
            }
            if (!hist && pscl_lane_exact_available(X)) h->n_lane_exact++;
            err = pscl_launch_decode(X, hist, st);
        }
    } else {
        if (lx == 3) P.lane_exact = 1;  // (test knob: plain decodes on the exact lane instance)
        if ((rc = with_count_slots(h, P, hist, kCountPart, st))) return rc;
        if (!hist && pscl_lane_exact_available(P)) h->n_lane_exact++;
        err = pscl_launch_decode(P, hist, st);
        if (err == hipSuccess && P.cpart) err = pscl_launch_count_reduce(P.cpart, pscl_decode_count_slots(P, hist), P.counters, st);
        // (no screening pass: the caller's tail follows the decode)
        if (err == hipSuccess && tail && !pipe && (rc = hand_over(h->ev_tscr[tail_par], st, tail))) return rc;
    }
    if (err != hipSuccess) return fail(PSCL_EDEVICE, "decode kernel launch: %s", hipGetErrorString(err));
    if (e1) HIP_TRY(hipEventRecord(e1, st));
    return PSCL_OK;
}

// pscl_decode_device and (f32: d_llr points at float32 rows) pscl_decode_device_f32
int decode_device_impl(pscl_handle* h, const void* d_llr, bool f32, int64_t B, const uint64_t* d_force, uint64_t* d_best,
                       uint8_t* d_flags, double* d_metrics, uint64_t* d_cands, double* d_info_llrs,
                       const uint64_t* d_ref, int k_payload, int64_t* d_counters) {
    if (!h) return fail(PSCL_EINVAL, "NULL handle");
    if (B < 0) return fail(PSCL_EINVAL, "B must be >= 0");
    if (B == 0) return PSCL_OK;
    if (!d_llr) return fail(PSCL_EINVAL, "d_llr is NULL");
    if (d_ref && !d_counters) return fail(PSCL_EINVAL, "d_ref given without d_counters");
    if (k_payload < 0 || k_payload > h->K) return fail(PSCL_EINVAL, "k_payload out of range");
    if (f32) {
        if (const char* why = f32_unsupported(h)) return fail(PSCL_EUNSUP, "%s", why);
    }
    int rc = set_device(h);
    if (rc) return rc;
    const int hist = d_info_llrs != nullptr;
    pscl_decode_params P;
    fill_decode_params(h, P, hist);
    P.llr = (const double*)d_llr;  // (f32: floats; only the float32 instances take the launch)
    P.f32 = f32 ? 1 : 0;
    P.B = B;
    P.force = d_force;
    P.best = d_best;
    P.flags = d_flags;
    P.metrics = d_metrics;
    P.cands = d_cands;
    P.info_llrs = d_info_llrs;
    P.ref = d_ref;
    P.k_payload = k_payload;
    P.counters = d_counters;
    if (pscl_decode_wpg(P) < 1) return fail(PSCL_EUNSUP, "LDS budget exceeded (L=%d, K=%d)", h->L, h->K);
    if (!h->pipelined && (rc = join_pipe(h))) return rc;
    if (h->pipelined && (h->ad[0].on || h->ad[1].on) && (rc = join_pipe(h, 1))) return rc;  // (adaptive calls' stage 2)
    return launch_decode(h, P, hist, nullptr, kLongScratch, h->pipelined, nullptr, 0, !f32);
}

// the SC stage over all B frames as one launch on the handle's stream (sc128_lane.hip at N = 128,
// sc_lane.hip at the other lengths), timed like a decode when timing is on
// f32: d_llr points at float32 rows (N = 128 only; the callers check)
// plain_rows: d_llr points at rows of N values whatever the handle's rate matching (the staged mode:
// the de-rate-matching pass wrote them)
int launch_sc_stage(pscl_handle* h, const double* d_llr, int64_t B, uint64_t* d_best, uint8_t* d_flags, uint8_t* d_stage,
                    bool f32 = false, bool plain_rows = false) {
    hipStream_t s = h->stream;
    hipEvent_t e1;  // (the SC launch is one timed launch on the handle's stream, like a decode)
    if (const int rc = timed_begin(h, s, &e1)) return rc;
    hipError_t e;
    if (h->N == PSCL_FAST_N) {
        pscl_sc_params S;
        memset(&S, 0, sizeof(S));
        S.llr = d_llr;
        S.B = B;
        S.K = h->K;
        S.W = h->W;
        S.info_mask[0] = h->info_mask[0];
        S.info_mask[1] = h->info_mask[1];
        S.epi_table = h->d_epi;
        S.epi_words = h->epi_words;
        S.rm_E = plain_rows ? 0 : h->rm_E;
        S.rm_src = plain_rows ? nullptr : h->d_rm_src;
        S.best = d_best;
        S.flags = d_flags;
        S.stage = d_stage;
        e = f32 ? pscl_launch_sc_lane_f32(S, s) : pscl_launch_sc_lane(S, s);
    } else {
        if (f32) return fail(PSCL_EUNSUP, "float32 rows: the SC stage takes N = %d only (N = %d)", PSCL_FAST_N, h->N);
        if (!pscl_scn_lane_available(h->N) || (h->rm_E && !plain_rows))
            return fail(PSCL_EUNSUP, "no SC kernel for N = %d%s", h->N, h->rm_E ? " with rate matching" : "");
        pscl_scn_params S;
        memset(&S, 0, sizeof(S));
        S.llr = d_llr;
        S.B = B;
        S.N = h->N;
        S.K = h->K;
        S.W = h->W;
        for (size_t k = 0; k < h->info_words.size() && k < 16; ++k) S.info_mask[k] = h->info_words[k];
        S.epi_table = h->d_epi;
        S.epi_words = h->epi_words;
        S.best = d_best;
        S.flags = d_flags;
        S.stage = d_stage;
        e = pscl_launch_scn_lane(S, s);
    }
    LAUNCH_TRY("sc kernel", e);
    if (e1) HIP_TRY(hipEventRecord(e1, s));
    return PSCL_OK;
}

// the hand-off to the list decoder: the frames whose flags lack PSCL_FLAG_CRC_PASS are compacted
// (dl_compact), their rows gathered densely into scratch, decoded by launch_decode as a plain decode
// of that many frames -- the screening path, not a row list, which would land on the exact kernel --
// and scattered back; d_stage (or null) gets 2 at those frames.  Scratch kEscCount .. kEscFlags.  One
// host wait: the count sizes the dense batch.
// f32: d_llr points at float32 rows, widened while they are gathered; the dense batch is doubles
// rm_stage: the dense batch may take the staged de-rate-matching route (launch_decode)
int escalate_failed(pscl_handle* h, const double* d_llr, int64_t B, uint64_t* d_best, uint8_t* d_flags, uint8_t* d_stage,
                    int64_t* n_out, bool f32 = false, bool rm_stage = false) {
    const int W = h->W;
    const int64_t row = h->rm_E ? h->rm_E : h->N;
    hipStream_t s = h->stream;
    int rc;
    if (!h->h_adapt) HIP_TRY(hipHostMalloc((void**)&h->h_adapt, 4, hipHostMallocDefault));
    void *d_cnt, *d_act;
    if ((rc = ensure(h, kEscCount, 4, &d_cnt))) return rc;
    if ((rc = ensure(h, kEscList, (size_t)B * 8, &d_act))) return rc;
    HIP_TRY(hipMemsetAsync(d_cnt, 0, 4, s));
    LAUNCH_TRY("dl_compact", pscl_launch_dl_compact(d_flags, B, 0, (int64_t*)d_act, nullptr, (int32_t*)d_cnt, s));
    HIP_TRY(hipMemcpyAsync(h->h_adapt, d_cnt, 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));  // the call's one host wait
    const int64_t n = *h->h_adapt;
    if (n < 0 || n > B) return fail(PSCL_EDEVICE, "escalated count %lld out of range", (long long)n);
    *n_out = n;
    if (n > 0) {
        // stage 2: a plain decode of the dense batch
        void *d_rows, *d_b2, *d_f2;
        if ((rc = ensure(h, kEscRows, (size_t)n * (size_t)row * 8, &d_rows))) return rc;
        if ((rc = ensure(h, kEscBest, (size_t)n * W * 8, &d_b2))) return rc;
        if ((rc = ensure(h, kEscFlags, (size_t)n, &d_f2))) return rc;
        LAUNCH_TRY("gather", f32 ? pscl_launch_gather_rows_f32((const float*)d_llr, row, (const int64_t*)d_act, n, (double*)d_rows, s)
                                 : pscl_launch_gather_rows(d_llr, row, (const int64_t*)d_act, n, (double*)d_rows, s));
        pscl_decode_params P;
        fill_decode_params(h, P, 0);
        P.llr = (const double*)d_rows;
        P.B = n;
        P.best = (uint64_t*)d_b2;
        P.flags = (uint8_t*)d_f2;
        if (pscl_decode_wpg(P) < 1) return fail(PSCL_EUNSUP, "LDS budget exceeded (L=%d, K=%d)", h->L, h->K);
        if ((rc = launch_decode(h, P, 0, nullptr, kLongScratch, false, nullptr, 0, rm_stage))) return rc;
        LAUNCH_TRY("scatter", pscl_launch_scatter_results((const int64_t*)d_act, n, W, (const uint64_t*)d_b2, (const uint8_t*)d_f2,
                                                          d_best, d_flags, s));
        if (d_stage) LAUNCH_TRY("stage", pscl_launch_mark_stage((const int64_t*)d_act, n, d_stage, s));
    }
    return PSCL_OK;
}

// statistics of the outputs of all B frames, as a plain decode adds them, and the escalated count
int count_final(pscl_handle* h, const uint64_t* d_best, const uint8_t* d_flags, int64_t B, const uint64_t* d_ref,
                int k_payload, int64_t* d_counters, int64_t n_escalated) {
    if (!d_ref) return PSCL_OK;
    LAUNCH_TRY("dl_count", pscl_launch_dl_count(d_best, d_flags, d_ref, B, h->W, k_payload, d_counters, h->stream));
    if (n_escalated > 0) LAUNCH_TRY("counter", pscl_launch_add_counter(d_counters, PSCL_CNT_ESCALATED, n_escalated, h->stream));
    return PSCL_OK;
}

int sc_device_impl(pscl_handle* h, const double* d_llr, bool f32, int64_t B, uint64_t* d_best, uint8_t* d_flags,
                   uint8_t* d_stage, const uint64_t* d_ref, int k_payload, int64_t* d_counters) {
    if (!h) return fail(PSCL_EINVAL, "NULL handle");
    if (B < 0) return fail(PSCL_EINVAL, "B must be >= 0");
    if (d_ref && !d_counters) return fail(PSCL_EINVAL, "d_ref given without d_counters");
    if (k_payload < 0 || k_payload > h->K) return fail(PSCL_EINVAL, "k_payload out of range");
    if (h->N < 32) return fail(PSCL_EUNSUP, "the SC stage is implemented for N = 32 .. %d (N = %d)", PSCL_MAX_N, h->N);
    const bool stage = h->rm_staged && h->rm_E && !f32 && h->N != PSCL_FAST_N;  // (the staged mode: the pass first)
    if (h->rm_E && h->N != PSCL_FAST_N && !stage)
        return fail(PSCL_EUNSUP, "the SC stage takes rate-matched rows at N = %d only (N = %d)", PSCL_FAST_N, h->N);
    if (f32 && h->N != PSCL_FAST_N)
        return fail(PSCL_EUNSUP, "float32 rows: the SC stage takes N = %d only (N = %d)", PSCL_FAST_N, h->N);
    if (B == 0) return PSCL_OK;
    if (!d_llr || !d_best || !d_flags) return fail(PSCL_EINVAL, "d_llr, d_best and d_flags are required");
    int rc = enter(h);  // (pending pipelined work first)
    if (rc) return rc;
    if (stage && (rc = launch_derate(h, d_llr, B, nullptr, kRmRows, h->stream, true, &d_llr))) return rc;
    if ((rc = launch_sc_stage(h, d_llr, B, d_best, d_flags, d_stage, f32, stage))) return rc;
    return count_final(h, d_best, d_flags, B, d_ref, k_payload, d_counters, 0);
}

int escalate_device_impl(pscl_handle* h, const double* d_llr, bool f32, int64_t B, uint64_t* d_best, uint8_t* d_flags,
                         uint8_t* d_stage, const uint64_t* d_ref, int k_payload, int64_t* d_counters,
                         int64_t* n_escalated) {
    if (!h) return fail(PSCL_EINVAL, "NULL handle");
    if (n_escalated) *n_escalated = 0;
    if (B < 0) return fail(PSCL_EINVAL, "B must be >= 0");
    if (!h->crc_poly) return fail(PSCL_EINVAL, "escalation needs a CRC (without one every SC result passes)");
    if (d_ref && !d_counters) return fail(PSCL_EINVAL, "d_ref given without d_counters");
    if (k_payload < 0 || k_payload > h->K) return fail(PSCL_EINVAL, "k_payload out of range");
    if (B == 0) return PSCL_OK;
    if (!d_llr || !d_best || !d_flags) return fail(PSCL_EINVAL, "d_llr, d_best and d_flags are required");
    if (B > INT32_MAX) return fail(PSCL_EUNSUP, "B exceeds 2^31-1");
    if (f32) {
        if (const char* why = f32_unsupported(h)) return fail(PSCL_EUNSUP, "%s", why);
    }
    int rc = enter(h);
    if (rc) return rc;
    int64_t n = 0;
    if ((rc = escalate_failed(h, d_llr, B, d_best, d_flags, d_stage, &n, f32, !f32))) return rc;
    if (n_escalated) *n_escalated = n;
    return count_final(h, d_best, d_flags, B, d_ref, k_payload, d_counters, n);
}

// the start of an adaptive call without a host wait: its scratch parity (pipelined calls alternate),
// and the handle's stream ordered behind the side-stream work that last used that parity -- and the
// caller's buffers of the call two back -- before this call's SC stage writes anything
int adaptive_begin(pscl_handle* h, bool pipe, int* par) {
    const int q = pipe ? h->ad_par : 0;
    if (pipe) {
        if (!h->pipe_stream) HIP_TRY(create_priority_stream(h, &h->pipe_stream));
        if (!h->ad_stream) HIP_TRY(create_priority_stream(h, &h->ad_stream));
        h->ad_par ^= 1;
    }
    *par = q;
    return h->ad[q].order(h->stream);
}

// Stage 2 without the host wait, after the SC stage on the handle's stream: the frames whose flags
// lack PSCL_FLAG_CRC_PASS are compacted into a row list and a device count (dl_compact; no dense
// buffers), and the list decoder runs on "the first count rows of the list, results at their rows":
// the row-list screening launch (pscl_rowlist; its grid is sized for B, never by the count: the
// workgroups past the count exit at once) and the exact re-decode of the frames it defers -- or, where the
// handle's plain decode has no lane-per-path screening kernel, the exact kernel on the list itself.
// Then (d_ref) the statistics of all B final outputs, and the escalated count from device memory.
// pipe: everything after the compaction on parity q's side stream behind ev_adc[q]; ev_ad[q] marks its end.
// f32: d_llr points at float32 rows (a handle with float32 kernels, f32_unsupported; the callers check):
// the row-list launch and the exact re-decode are the float32 instances
// d_stg (the staged mode, or null): the call's rows de-rate-matched by the pass, [B][N].  The row-list
// screening launch is then the rate-matching-free twin's and reads d_stg by the same row indices (no
// second pass, no gather); the exact kernel reads the caller's rows with rm_E, as without the mode
int adaptive_escalate_enqueue(pscl_handle* h, int q, bool pipe, const double* d_llr, int64_t B, uint64_t* d_best,
                              uint8_t* d_flags, const uint64_t* d_ref, int k_payload, int64_t* d_counters,
                              int32_t* d_n_escalated, bool f32 = false, const double* d_stg = nullptr) {
    hipStream_t s = h->stream;
    const int64_t regrown = h->n_regrow;
    int rc;
    void *d_cnt, *d_list, *d_amb;
    if ((rc = ensure(h, slot_adapt(q, kAdCounts), 128, &d_cnt))) return rc;
    if ((rc = ensure(h, slot_adapt(q, kAdEscList), (size_t)B * 8, &d_list))) return rc;
    if ((rc = ensure(h, slot_adapt(q, kAdAmbList), (size_t)B * 8, &d_amb))) return rc;
    int32_t* const amb_cnt = (int32_t*)d_cnt;
    int32_t* const esc_cnt = amb_cnt + 16;
    pscl_decode_params P;
    fill_decode_params(h, P, 0);
    P.llr = d_llr;
    P.B = B;
    P.best = d_best;
    P.flags = d_flags;
    P.fidx = (const int64_t*)d_list;
    P.d_count = esc_cnt;
    P.out_by_row = 1;
    P.f32 = f32 ? 1 : 0;  // (S and X below inherit it)
    if (pscl_decode_wpg(P) < 1) return fail(PSCL_EUNSUP, "LDS budget exceeded (L=%d, K=%d)", h->L, h->K);
    pscl_decode_params S = P;  // the row-list screening launch
    S.apx = 1;
    if (d_stg) plain_twin(S, d_stg, 0);
    pscl_decode_layout(S, 0);
    S.amb_list = (int64_t*)d_amb;
    S.amb_count = amb_cnt;
    S.grid_cap = h->tune[PSCL_TUNE_ADAPT_GRID];  // (0: sized for B -- measured faster than any resident cap)
    const bool screen = h->screen && h->tune[PSCL_TUNE_LANE_EXACT] != 3 &&
                        (S.long_mode ? pscl_lane_long_available(S) != 0
                                     : (pscl_lane_available(S) != 0 || pscl_lane_long128_available(S) != 0));
    pscl_decode_params X = P;  // the exact kernel: on the deferred frames, or on the row list itself
    X.lane_exact = lane_exact_on(h) ? 1 : 0;
    X.grid_cap = (int64_t)256 * 16 / (pscl_decode_wpg(X) > 0 ? pscl_decode_wpg(X) : 1);  // (one resident set, launch_decode)
    if (screen) {
        X.fidx = (const int64_t*)d_amb;
        X.d_count = amb_cnt;
    }
    if (X.long_mode) {
        void* d_scr;
        if ((rc = ensure(h, slot_adapt(q, kAdLongScratch), (size_t)pscl_decode_grid(X) * (size_t)X.long_block_bytes, &d_scr)))
            return rc;
        X.long_scratch = (unsigned char*)d_scr;
    }
    h->n_ad_waits += h->n_regrow - regrown;  // (a regrown buffer drained the side streams on the host)
    HIP_TRY(hipMemsetAsync(d_cnt, 0, 128, s));
    LAUNCH_TRY("dl_compact", pscl_launch_dl_compact(d_flags, B, 0, (int64_t*)d_list, nullptr, esc_cnt, s));
    hipStream_t t = s;
    if (pipe) {
        t = q ? h->ad_stream : h->pipe_stream;
        if ((rc = hand_over(h->ev_adc[q], s, t))) return rc;
    }
    if (screen) {
        LAUNCH_TRY("row-list decode", pscl_launch_decode(S, 0, t));
        h->screened = true;
        h->screened_slot = slot_adapt(q, kAdCounts);
        h->n_ad_screened++;
    } else {
        h->n_ad_exact++;
    }
    if (pscl_lane_exact_available(X)) h->n_lane_exact++;
    LAUNCH_TRY("decode kernel", pscl_launch_decode(X, 0, t));
    if (d_ref) LAUNCH_TRY("dl_count", pscl_launch_dl_count(d_best, d_flags, d_ref, B, h->W, k_payload, d_counters, t));
    if (d_ref || d_n_escalated)
        LAUNCH_TRY("counter", pscl_launch_publish_count(esc_cnt, d_ref ? d_counters : nullptr, PSCL_CNT_ESCALATED, d_n_escalated, t));
    return pipe ? h->ad[q].mark(t) : PSCL_OK;
}

// the argument checks the adaptive calls without a host wait share
// staged: the caller consults the staged mode (pscl_adaptive_async_device), which lifts the refusal
// of rate-matched rows at N != 128
int adaptive_async_args(pscl_handle* h, int64_t B, int k_payload, bool staged = false) {
    if (!h) return fail(PSCL_EINVAL, "NULL handle");
    if (B < 0) return fail(PSCL_EINVAL, "B must be >= 0");
    if (!h->crc_poly) return fail(PSCL_EINVAL, "adaptive decoding needs a CRC (without one every SC result passes)");
    if (k_payload < 0 || k_payload > h->K) return fail(PSCL_EINVAL, "k_payload out of range");
    if (h->N < 32) return fail(PSCL_EUNSUP, "the SC stage is implemented for N = 32 .. %d (N = %d)", PSCL_MAX_N, h->N);
    if (h->rm_E && h->N != PSCL_FAST_N && !(staged && h->rm_staged))
        return fail(PSCL_EUNSUP, "the SC stage takes rate-matched rows at N = %d only (N = %d)", PSCL_FAST_N, h->N);
    if (B > INT32_MAX) return fail(PSCL_EUNSUP, "B exceeds 2^31-1");
    return PSCL_OK;
}

// does pscl_adaptive_async_device take the staged route on this handle: always at N != 128 (the SC
// kernels of those lengths take plain rows only), and at N = 128 where the twin's stage 2 has a
// row-list screening kernel and the handle's own has none (the compiled (128,88) code keeps its own)
bool adaptive_stages(const pscl_handle* h) {
    if (!h->rm_staged || !h->rm_E) return false;
    if (h->N != PSCL_FAST_N) return true;
    if (!h->screen || h->tune[PSCL_TUNE_LANE_EXACT] == 3) return false;
    pscl_decode_params S;
    fill_decode_params(h, S, 0);
    S.apx = 1;
    S.B = 1;
    S.fidx = S.amb_list = reinterpret_cast<int64_t*>(16);  // (a row-list launch's shape; nothing is launched)
    S.d_count = S.amb_count = reinterpret_cast<int32_t*>(16);
    S.out_by_row = 1;
    pscl_decode_layout(S, 0);
    if (pscl_lane_available(S) != 0 || pscl_lane_long128_available(S) != 0) return false;
    plain_twin(S, nullptr, 0);
    return pscl_lane_available(S) != 0 || pscl_lane_long128_available(S) != 0;
}

int adaptive_async_impl(pscl_handle* h, const double* d_llr, bool f32, int64_t B, uint64_t* d_best, uint8_t* d_flags,
                        uint8_t* d_stage, const uint64_t* d_ref, int k_payload, int64_t* d_counters,
                        int32_t* d_n_escalated) {
    int rc = adaptive_async_args(h, B, k_payload, !f32);
    if (rc) return rc;
    if (d_ref && !d_counters) return fail(PSCL_EINVAL, "d_ref given without d_counters");
    if (B > 0 && (!d_llr || !d_best || !d_flags)) return fail(PSCL_EINVAL, "d_llr, d_best and d_flags are required");
    if (f32) {
        if (const char* why = f32_unsupported(h)) return fail(PSCL_EUNSUP, "%s", why);
    }
    const bool pipe = h->pipelined;
    // (pending pipelined work first; a pipelined call orders the earlier adaptive calls by parity)
    if ((rc = set_device(h)) || (rc = join_pipe(h, pipe ? 3 + 8 : 3))) return rc;
    if (B == 0) {
        if (d_n_escalated) HIP_TRY(hipMemsetAsync(d_n_escalated, 0, 4, h->stream));
        return PSCL_OK;
    }
    int q = 0;
    if ((rc = adaptive_begin(h, pipe, &q))) return rc;
    // the staged mode: one pass into parity q's rows (adaptive_begin has ordered the handle's stream
    // behind the parity's previous stage 2, which read them), the SC stage and stage 2's screening on those
    const double* d_stg = nullptr;
    if (!f32 && adaptive_stages(h)) {
        const int64_t regrown = h->n_regrow;
        if ((rc = launch_derate(h, d_llr, B, nullptr, slot_rm_adapt(q), h->stream, true, &d_stg))) return rc;
        h->n_ad_waits += h->n_regrow - regrown;
    }
    if ((rc = launch_sc_stage(h, d_stg ? d_stg : d_llr, B, d_best, d_flags, d_stage, f32, d_stg != nullptr))) return rc;
    return adaptive_escalate_enqueue(h, q, pipe, d_llr, B, d_best, d_flags, d_ref, k_payload, d_counters, d_n_escalated, f32,
                                     d_stg);
}

// pscl_path_llrs_device and (f32: d_llr points at float32 rows) pscl_path_llrs_device_f32
int path_llrs_impl(pscl_handle* h, const void* d_llr, bool f32, int64_t B, const uint64_t* d_bits, double* d_out) {
    if (!h) return fail(PSCL_EINVAL, "NULL handle");
    if (B < 0) return fail(PSCL_EINVAL, "B must be >= 0");
    if (B == 0) return PSCL_OK;
    if (!d_llr || !d_bits || !d_out) return fail(PSCL_EINVAL, "d_llr, d_bits and d_out are required");
    if (f32 && h->N != PSCL_FAST_N)
        return fail(PSCL_EUNSUP, "float32 rows: the decision-LLR replay takes N = %d only (N = %d)", PSCL_FAST_N, h->N);
    if (B > INT32_MAX) return fail(PSCL_EUNSUP, "B exceeds 2^31-1");
    int rc = enter(h);
    if (rc) return rc;
    void *d_cnt, *d_rows;
    if ((rc = ensure(h, kPathCount, 8, &d_cnt))) return rc;
    if ((rc = ensure(h, kPathRows, (size_t)B * 8, &d_rows))) return rc;
    const int32_t nb = (int32_t)B;
    HIP_TRY(hipMemcpyAsync(d_cnt, &nb, 4, hipMemcpyHostToDevice, h->stream));
    LAUNCH_TRY("iota", pscl_launch_iota64((int64_t*)d_rows, B, h->stream));
    pscl_replay_params Rp;
    memset(&Rp, 0, sizeof(Rp));
    Rp.llr = (const double*)d_llr;  // (f32: floats; the float32 instance takes the launch)
    Rp.row_f32 = f32 ? 1 : 0;
    Rp.N = h->N;
    Rp.n = h->n;
    Rp.K = h->K;
    Rp.W = h->W;
    Rp.rm_E = h->rm_E;
    Rp.rm_src = h->d_rm_src;
    Rp.info_mask[0] = h->info_mask[0];
    Rp.info_mask[1] = h->info_mask[1];
    Rp.count = (const int32_t*)d_cnt;
    Rp.act = (const int64_t*)d_rows;
    Rp.bits = d_bits;
    Rp.bits_by_row = 1;
    Rp.out = d_out;
    const bool lng = h->N > PSCL_FAST_N;  // the long replay kernel (replay_long.hip): the mask by words, on the device
    if (lng) {
        h->n_replay_launches++;
        h->n_replay_rows += B;
    }
    LAUNCH_TRY("replay", lng ? pscl_launch_replay_long(Rp, B, h->d_info_words, nullptr, h->stream)
                             : pscl_launch_replay(Rp, B, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));  // d_cnt is a host-staged value
    return PSCL_OK;
}

// retry rounds of one chunk on the retry stream (state sized for the largest chunk)
#ifndef PSCL_DL_FUSED_POST_DEFAULT
#define PSCL_DL_FUSED_POST_DEFAULT 0
#endif
struct DlState {
    int64_t* act;     // [cap] frame index of each entry (a slice of the chunk's dl_compact output)
    int32_t* bcnt;    // [rounds + 1][NSEG * CSTRIDE] bucket counters of each round's list
    int32_t *list0, *list1;  // [NSEG][cap] bucket lists (entry ids), alternating rounds
    uint64_t *tried, *force, *warm_u, *ob;
    int32_t* nt;
    double* warm_metric;
    uint8_t* of;
    int32_t *dcnt, *dlist;   // screening retry decodes: the side chain's bucket lists, one per round
                             // ([rounds + 1][NSEG * CSTRIDE] counts, [rounds + 1][NSEG][cap])
    uint64_t* ob2;           // [cap][W] and [cap]: their exact decode's outputs (the main post pass reads
    uint8_t* of2;            //   `of` concurrently, where the deferred mark must stay)
};

#ifndef PSCL_DL_WARM_APX_DEFAULT
#define PSCL_DL_WARM_APX_DEFAULT 1  // (measured: profiles/r06t_warm_apx_ab.txt)
#endif

// float32 rows in a DL-SCL call (pscl_dlscl_device_f32, pscl_retry_device_f32,
// pscl_adaptive_dlscl_device_f32): why this handle's chains have no float32 kernels, or null where they
// have -- the handles of f32_unsupported, whose default chains are native (the screened lane-per-path
// retry decode with the exact side chain for the (128,64) code, exact retry rounds for the rate-matched
// (128,88) code, the post pass in its wide and narrow forms at 2 and 4 entries per wavefront; chunks,
// splits, PSCL_TUNE_DL_SCREEN and PSCL_TUNE_DL_WARM_APX select among those).  Two knobs select an
// instance that was not built over float rows and are refused by name rather than run as something
// else, which pscl_path_stats would misreport.
const char* f32_chain_unsupported(const pscl_handle* h) {
    if (const char* why = f32_unsupported(h)) return why;
    if (!h->rm_E) {  // (the rate-matched chains screen nothing: the two knobs do not apply)
        const int64_t fk = h->tune[PSCL_TUNE_DL_FUSED_POST];
        if (fk == 1 || (fk == 0 && PSCL_DL_FUSED_POST_DEFAULT))
            return "PSCL_TUNE_DL_FUSED_POST selects the retry decode with the fused post pass, which has no float32 form";
        if (h->tune[PSCL_TUNE_DL_RETRY_LANE] == 2)
            return "PSCL_TUNE_DL_RETRY_LANE = 2 selects the two-lanes-per-path screened retry decode, which has no float32 form";
    }
    return nullptr;
}

hipError_t launch_post(pscl_handle* h, const pscl_post_params& Q, int64_t A, hipStream_t s) {
    if (pscl_post_epw(Q) == 4) h->n_post_epw4++;
    return pscl_launch_dl_post(Q, A, s);
}

int dl_retry_chunk(pscl_handle* h, const DlState& S, int A, int rounds, const double* d_llr, uint64_t* d_best,
                   uint8_t* d_flags, int32_t* d_attempts, int32_t* d_tried, int tried_stride, int64_t* d_cnt_dl,
                   hipStream_t st, hipStream_t side, hipEvent_t& ev_s, hipEvent_t& ev_d, bool narrow, bool beside, bool f32) {
    // f32: d_llr points at float32 rows (a handle with float32 chains, f32_chain_unsupported; the
    // callers check) -- every post pass and every retry decode below is the float32 instance
    const int K = h->K, W = h->W;
    hipError_t e;
    const size_t bstride = (size_t)PSCL_DL_NSEG * PSCL_DL_CSTRIDE;
    HIP_TRY(hipMemsetAsync(S.bcnt, 0, (size_t)(rounds + 1) * bstride * 4, st));
    pscl_post_params Q;
    memset(&Q, 0, sizeof(Q));
    Q.llr = d_llr;
    Q.row_f32 = f32 ? 1 : 0;  // (QD and the launches' copies inherit it)
    Q.N = h->N;
    Q.n = h->n;
    Q.K = K;
    Q.W = W;
    Q.rm_E = h->rm_E;
    Q.rm_src = h->d_rm_src;
    Q.info_mask[0] = h->info_mask[0];
    Q.info_mask[1] = h->info_mask[1];
    Q.info_set = h->d_info_set;
    Q.exp_table = h->d_exp_table;
    Q.rounds = rounds;
    Q.narrow = narrow ? 1 : 0;  // (pipelined calls: beside the next call's baseline)
    Q.grid_cap = h->tune[PSCL_TUNE_POST_GRID];
    Q.pairs = h->tune[PSCL_TUNE_POST_PAIRS];
    Q.epw = (int)h->tune[PSCL_TUNE_POST_EPW];
    Q.cap = A;
    Q.act = S.act;
    Q.tried = S.tried;
    Q.ntried = S.nt;
    Q.beta = h->d_beta;
    Q.beta_absmax = h->beta_absmax;
    Q.force = S.force;
    Q.warm_metric = S.warm_metric;
    Q.warm_u = S.warm_u;
    Q.ob = S.ob;
    Q.of = S.of;
    Q.best = d_best;
    Q.flags = d_flags;
    Q.attempts = d_attempts;
    Q.tried_out = d_tried;
    Q.tried_stride = tried_stride;
    Q.counters = d_cnt_dl;
    int32_t* lists[2] = {S.list0, S.list1};
    // the retry decodes: entries bucket by bucket, LLR rows by indirection, forced prefixes,
    // warm-started past them (the compiled-in FS kernels; others decode from phase 0)
    pscl_decode_params H;
    fill_decode_params(h, H, 0);
    H.llr = d_llr;
    pscl_set_row_type(H, f32);  // (HA and HX inherit it)
    H.B = A;
    H.fidx = S.act;
    H.force = S.force;
    H.best = S.ob;
    H.flags = S.of;
    H.bcap = A;
    H.warm_metric = S.warm_metric;
    H.warm_u = S.warm_u;
    H.wpg_cap = (int)h->tune[PSCL_TUNE_RETRY_WPG];
    H.lane_exact = lane_exact_on(h) ? 1 : 0;  // (exact retry rounds: the lane-per-path instance)
    if (pscl_decode_wpg(H) < 1) return fail(PSCL_EUNSUP, "LDS budget exceeded (L=%d, K=%d)", h->L, h->K);
    int rc;
    // screening retry decodes (measured in DESIGN.md §5.4): the forced-bit screening instance
    // decodes the round's entries and moves the ones it cannot certify to a SIDE CHAIN (flags
    // PSCL_DL_DEFERRED, which the main post pass skips): on the side stream, round r of the side
    // chain decodes its entries exactly (warm-started, as every retry decode) -- the ones round r
    // of the main chain deferred plus the side chain's own survivors -- and its post pass files the
    // survivors in the side chain's list of round r + 1.  An entry stays on the side chain once
    // deferred, at the same attempt index as the main chain's round, so the main chain never waits
    // for the side chain's exact decodes; the chain ends with both.  Each round has its own side
    // list (the side chain may lag the main chain by several rounds).
    // screening retry decodes: always (1), never (2), or by default (0) every chain, unless
    // PSCL_TUNE_DL_SCREEN_MIN sets a size threshold (chains of at least that many entries, and every
    // chain beside a later baseline decode).  With the deferred entries on the side chain the main
    // chain never waits for an exact decode, so screening wins alone too: the standalone config-3
    // 5 dB point (~10^4 entries per round) 4.61-4.62 -> 4.32 ms, the sweep 283.7 -> 285.1 M frames/s
    // (profiles/r05v_screen_ab.txt; round 4, before the side chain, it lost alone: 5.6 -> 6.1 ms)
    const int64_t ds = h->tune[PSCL_TUNE_DL_SCREEN];
    const int64_t ds_min = h->tune[PSCL_TUNE_DL_SCREEN_MIN];
    const bool dl_screen = ds == 1 || (ds == 0 && (!ds_min || A >= ds_min || beside));
    const bool scr = dl_screen && h->screen && S.dcnt && S.ob2 && side && pscl_screening_fs_available(H);
    pscl_decode_params HA, HX;
    pscl_post_params QD;
    bool fpost = false;  // the main chain's post pass inside its screened retry decodes
    if (scr) {
        HA = H;
        HA.apx = 1;
        pscl_decode_layout(HA, 0);  // (no exp table in LDS)
        HA.no_lane = h->tune[PSCL_TUNE_DL_RETRY_LANE] == 2 ? 1 : 0;  // (lane-per-path FS kernel by default)
        const int64_t fk = h->tune[PSCL_TUNE_DL_FUSED_POST];
        pscl_decode_params T = HA;  // (the rounds' launches: bucket lists in and deferred lists out)
        T.elist = lists[0];
        T.bcount = S.bcnt;
        T.amb_elist = S.dlist;
        T.amb_count = S.dcnt;
        fpost = (fk == 1 || (fk == 0 && PSCL_DL_FUSED_POST_DEFAULT)) && !HA.no_lane && pscl_lane_fs_available(T) &&
                h->K == 64 && (!h->d_beta || h->d_beta32g[h->L == 8 ? 0 : 1]);
        if (fpost) {
            HA.fpost = 1;
            HA.fp = Q;
            HA.fp.init = 0;
            HA.fp_beta32g = h->d_beta ? h->d_beta32g[h->L == 8 ? 0 : 1] : nullptr;
        }
        HX = H;
        HX.best = S.ob2;
        HX.flags = S.of2;
        HX.grid_cap = (int64_t)256 * 16 / (pscl_decode_wpg(HX) > 0 ? pscl_decode_wpg(HX) : 1);
        QD = Q;
        QD.init = 0;
        QD.ob = S.ob2;
        QD.of = S.of2;
        HIP_TRY(hipMemsetAsync(S.dcnt, 0, (size_t)(rounds + 1) * bstride * 4, st));
        // the main chain's warm-start metrics from the screening tail (PSCL_TUNE_DL_WARM_APX): its
        // screened decodes certify against margins that cover every increment's tail error, the
        // prefix's too; the entries they defer go to the side chain's bucket 0 (exact from phase 0),
        // whose own posts (QD) keep exact metrics
        // (default: for chains beside a later baseline decode, which are throughput-bound; a chain
        // running alone is latency-bound, and its side chain -- the longer one -- keeps warm starts)
        const int64_t wk = h->tune[PSCL_TUNE_DL_WARM_APX];
        if (!fpost && (wk == 1 || (wk == 0 && PSCL_DL_WARM_APX_DEFAULT && beside))) {
            Q.warm_apx = 1;
            HA.warm_apx = 1;
        }
    }
    // first flips: replay of every baseline best path (flip.py:97-111)
    Q.init = 1;
    Q.in_count = nullptr;
    Q.out_count = S.bcnt;
    Q.out_list = lists[0];
    LAUNCH_TRY("dl_post", launch_post(h, Q, A, st));
    auto side_list = [&](int r) { return S.dlist + (size_t)r * PSCL_DL_NSEG * (size_t)A; };
    auto side_cnt = [&](int r) { return S.dcnt + (size_t)r * bstride; };
    Q.init = 0;
    for (int r = 0; r < rounds; ++r) {  // no host round trips: the counts stay on the device
        H.elist = lists[r & 1];
        H.bcount = S.bcnt + (size_t)r * bstride;
        if (scr) {
            HA.elist = H.elist;
            HA.bcount = H.bcount;
            HA.amb_elist = side_list(r);  // (the side chain's round-r list: appended beside QD(r - 1))
            HA.amb_count = side_cnt(r);
            if (fpost) {  // the round's survivors to the next round's lists, filed by the decode itself
                HA.fp.in_count = H.bcount;
                HA.fp.in_list = lists[r & 1];
                HA.fp.out_count = S.bcnt + (size_t)(r + 1) * bstride;
                HA.fp.out_list = lists[(r + 1) & 1];
            }
            if ((e = pscl_launch_decode(HA, 0, st)) != hipSuccess)
                return fail(PSCL_EDEVICE, "screening retry decode: %s", hipGetErrorString(e));
            // side round r: after the main round's deferrals (ev_s) and side round r - 1 (stream order)
            if ((rc = hand_over(ev_s, st, side))) return rc;
            HX.elist = side_list(r);
            HX.bcount = side_cnt(r);
            if (pscl_lane_exact_available(HX)) h->n_lane_exact++;
            if ((e = pscl_launch_decode(HX, 0, side)) != hipSuccess)
                return fail(PSCL_EDEVICE, "exact retry re-decode: %s", hipGetErrorString(e));
            QD.in_list = side_list(r);
            QD.in_count = side_cnt(r);
            QD.out_list = side_list(r + 1);
            QD.out_count = side_cnt(r + 1);
            LAUNCH_TRY("dl_post", launch_post(h, QD, A, side));
        } else if ((rc = launch_decode(h, H, 0, st))) {
            return rc;
        }
        if (fpost) {  // (the decode ran the main chain's post pass)
            h->n_fpost_rounds++;
            continue;
        }
        h->n_post_rounds++;
        Q.in_count = H.bcount;
        Q.in_list = lists[r & 1];
        Q.out_count = S.bcnt + (size_t)(r + 1) * bstride;
        Q.out_list = lists[(r + 1) & 1];
        LAUNCH_TRY("dl_post", launch_post(h, Q, A, st));
    }
    if (scr && rounds > 0) return hand_over(ev_d, side, st);  // the chain ends with its side chain
    return PSCL_OK;
}

// long codes (N > PSCL_FAST_N): dense entry state, ping-ponged between passes
struct DlLongState {
    int64_t* act1;              // the second entry-frame array (the first is the compaction's)
    uint64_t *tried[2], *ob, *force;
    int32_t *nt[2], *cnt;       // cnt: [rounds + 2] entries of each pass
    uint8_t* of;
    double* l0;
};

// The retry chain of a chunk's A failing frames (act0/cnt0: dl_compact's output) for the long
// codes: the failing frames decoded again with decision-LLR history (the baseline's L0,
// flip.py:97-102; same best bits), a first post pass, then per round a HIST decode of the live
// entries (forced bits, LLR rows by indirection, the live count on the device) and a post pass.
int dl_retry_long(pscl_handle* h, const DlLongState& S, int64_t* act0, const int32_t* cnt0, int A, int rounds,
                  const double* d_llr, uint64_t* d_best, uint8_t* d_flags, int32_t* d_attempts, int32_t* d_tried,
                  int tried_stride, int64_t* d_cnt_dl, hipStream_t st) {
    int rc;
    HIP_TRY(hipMemsetAsync(S.cnt, 0, (size_t)(rounds + 2) * 4, st));
    // PSCL_TUNE_DL_LONG_REPLAY: every attempt's L0 from the long replay kernel (replay_long.hip) -- the
    // baseline's over (act0, d_best by frame), which also copies those bits to S.ob for the first post
    // pass, with no second baseline decode; a round's over (its entries, S.ob by entry) after a retry
    // decode without history.  The same values bit for bit (the replay's contract)
    const bool rpl = h->tune[PSCL_TUNE_DL_LONG_REPLAY] == 1;
    const int hist = rpl ? 0 : 1;
    pscl_replay_params Rp;
    memset(&Rp, 0, sizeof(Rp));
    Rp.llr = d_llr;
    Rp.N = h->N;
    Rp.n = h->n;
    Rp.K = h->K;
    Rp.W = h->W;
    Rp.rm_E = h->rm_E;
    Rp.rm_src = h->d_rm_src;
    Rp.out = S.l0;
    auto replay = [&](const int32_t* count, const int64_t* act, const uint64_t* bits, int by_row, uint64_t* ob_copy) {
        Rp.count = count;
        Rp.act = act;
        Rp.bits = bits;
        Rp.bits_by_row = by_row;
        h->n_replay_launches++;
        h->n_replay_rows += A;
        return pscl_launch_replay_long(Rp, A, h->d_info_words, ob_copy, st);
    };
    pscl_decode_params H;
    fill_decode_params(h, H, hist);
    H.llr = d_llr;
    H.B = A;
    H.fidx = act0;
    H.d_count = cnt0;
    H.best = S.ob;
    H.flags = S.of;
    H.best_info_llrs = rpl ? nullptr : S.l0;
    if (rpl)
        LAUNCH_TRY("replay", replay(cnt0, act0, d_best, 1, S.ob));
    else if ((rc = launch_decode(h, H, 1, st, kLongRetryScratch)))
        return rc;
    pscl_post_long_params Q;
    memset(&Q, 0, sizeof(Q));
    Q.K = h->K;
    Q.W = h->W;
    Q.rounds = rounds;
    Q.cap = A;
    Q.ob = S.ob;
    Q.of = S.of;
    Q.l0 = S.l0;
    Q.force = S.force;
    Q.beta = h->d_beta;
    Q.best = d_best;
    Q.flags = d_flags;
    Q.attempts = d_attempts;
    Q.tried_out = d_tried;
    Q.tried_stride = tried_stride;
    Q.counters = d_cnt_dl;
    int64_t* acts[2] = {act0, S.act1};
    Q.init = 1;
    Q.in_count = cnt0;
    Q.out_count = S.cnt + 1;
    Q.act_in = act0;
    Q.act_out = S.act1;
    Q.tried_w_out = S.tried[1];
    Q.nt_out = S.nt[1];
    LAUNCH_TRY("dl_post_long", pscl_launch_dl_post_long(Q, st));
    Q.init = 0;
    for (int r = 0; r < rounds; ++r) {  // pass r + 1 reads state set (r + 1) & 1
        const int c = (r + 1) & 1;
        H.fidx = acts[c];
        H.d_count = S.cnt + r + 1;
        H.force = S.force;
        if ((rc = launch_decode(h, H, hist, st, kLongRetryScratch))) return rc;
        if (rpl) LAUNCH_TRY("replay", replay(S.cnt + r + 1, acts[c], S.ob, 0, nullptr));
        Q.in_count = S.cnt + r + 1;
        Q.out_count = S.cnt + r + 2;
        Q.act_in = acts[c];
        Q.act_out = acts[c ^ 1];
        Q.tried_in = S.tried[c];
        Q.tried_w_out = S.tried[c ^ 1];
        Q.nt_in = S.nt[c];
        Q.nt_out = S.nt[c ^ 1];
        LAUNCH_TRY("dl_post_long", pscl_launch_dl_post_long(Q, st));
    }
    return PSCL_OK;
}

constexpr int kMinSplit = 2048;

// the retry chains' state (scratch kDlCount, kDlAct, kChain, kLong), sized by dl_setup
struct DlBufs {
    DlState S[kChainStreams];  // chain state (S[2 set + k] on retry stream 2 set + k)
    DlLongState LS = {};  // (long codes)
    int32_t* cnt[kDlPar] = {};  // failing-frame count of the compaction parities
    int64_t* act[kDlPar] = {};  // their frame indices
};

// compaction parity of chunk c: a pipelined call (one chunk) takes the handle's rotating parity,
// the chunks of an unpipelined call alternate two
inline int dl_parity(const pscl_dl_call& a, int64_t c) { return a.pipe ? a.pbase : (int)(c & 1); }

// streams and scratch of a DL-SCL call (everything sized before any work is queued: an allocation
// synchronizes the device)
int dl_setup(pscl_handle* h, const pscl_dl_call& a, DlBufs& b) {
    int rc;
    const size_t K = (size_t)h->K, W = (size_t)h->W, R = (size_t)a.rounds + 1, R2 = R + 1;
    const int64_t cap = a.cap;
    // chain sets: a pipelined call's chains (or an unpipelined call's chunk chains) alternate two
    const int nsets = (h->N <= PSCL_FAST_N && (a.pipe || a.nch >= 2)) ? kChainSets : 1;
    // (only the streams of the chains this call runs: chain i of set s is stream 2 s + i, i < nsplit;
    // every extra stream of the process shifts how the runtime spreads streams over its hardware queues)
    for (int i = 0; i < 2 * nsets; ++i)
        if (!h->retry_stream[i] && (i & 1) < (a.nsplit > 0 ? a.nsplit : 1)) HIP_TRY(create_priority_stream(h, &h->retry_stream[i]));
    for (int i = 0; i < 2 * nsets; ++i)
        if (!h->side_stream[i] && (i & 1) < (a.nsplit > 0 ? a.nsplit : 1)) HIP_TRY(create_priority_stream(h, &h->side_stream[i]));
    if (!h->h_count) HIP_TRY(hipHostMalloc((void**)&h->h_count, 4 * kDlPar, hipHostMallocDefault));
    const size_t NS = PSCL_DL_NSEG;
    for (int i = 0; i < (a.pipe ? kDlPar : (a.nch >= 2 ? 2 : 1)); ++i)
        if ((rc = ensure_as(h, slot_dl_count(i), 4, b.cnt[i])) || (rc = ensure_as(h, slot_dl_act(i), (size_t)cap * 8, b.act[i])))
            return rc;
#define X(field, member, bytes) \
    if ((rc = ensure_as(h, base + field, bytes, T.member))) return rc;
    if (h->N > PSCL_FAST_N) {  // long codes: one chain, dense state (dl_retry_long)
        const size_t c = (size_t)cap;
        const int base = kLong;
        DlLongState& T = b.LS;
        DL_LONG_FIELDS(X)
        pscl_decode_params H;  // the retry decodes' scratch
        fill_decode_params(h, H, 1);
        H.B = cap;
        void* d_scr;
        if ((rc = ensure(h, kLongRetryScratch, (size_t)pscl_decode_grid(H) * (size_t)H.long_block_bytes, &d_scr)))
            return rc;
    }
    for (int j = 0; j < 2 * nsets; ++j) {
        // chain 0 takes every entry of a call that does not split (fewer than 2 kMinSplit
        // failing frames, which may still exceed half the chunk); chain 1 at most half
        const int i = j & 1, set = j >> 1;
        if (i >= a.nsplit) continue;
        const size_t c = (size_t)(i == 0 ? cap : cap - cap / 2);
        const int base = slot_chain(j, 0);
        DlState& T = b.S[2 * set + i];
        DL_CHAIN_FIELDS(X)
    }
#undef X
    return PSCL_OK;
}

// the chain set of chunk c: alternating by call (pipelined) or by chunk; the long codes' single
// dense-state chain keeps set 0
inline int dl_set(const pscl_handle* h, const pscl_dl_call& a, int64_t c) {
    if (h->tune[PSCL_TUNE_DL_STREAMS] & 2) return 0;  // (one set: chains in call order on its streams)
    return h->N > PSCL_FAST_N ? 0 : (a.pipe ? a.pbase : (int)c) & (kChainSets - 1);
}

// the retry chains of chunk c (compaction parity p): the host reads the chunk's failing count
// (waiting for its baseline) and enqueues the rounds on the retry streams of the chunk's set;
// ev_retry[p] marks their end on the set's first retry stream
int dl_chain(pscl_handle* h, const pscl_dl_call& a, const DlBufs& b, int64_t c, bool beside) {
    const int p = dl_parity(a, c);
    const int cs = 2 * dl_set(h, a, c);  // the set's first stream
    const int64_t cap = a.cap;
    const auto w0 = std::chrono::steady_clock::now();
    HIP_TRY(hipEventSynchronize(h->ev_base[p]));
    h->host_wait_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - w0).count();
    const int A = h->h_count[p];
    int64_t* d_cdl = a.d_ref ? a.d_counters_dl : nullptr;
    if (h->N > PSCL_FAST_N) {
        if (A > 0) {
            HIP_TRY(hipStreamWaitEvent(h->retry_stream[0], h->ev_base[p], 0));
            if (a.d_stage) LAUNCH_TRY("stage", pscl_launch_dl_mark_stage(b.act[p], A, a.d_stage, 3, h->retry_stream[0]));
            int r2 = dl_retry_long(h, b.LS, b.act[p], b.cnt[p], A, a.rounds, a.d_llr, a.d_best, a.d_flags, a.d_attempts,
                                   a.d_tried, a.tried_stride, d_cdl, h->retry_stream[0]);
            if (r2) return r2;
        }
        return record_event(h->ev_retry[p], h->retry_stream[0]);
    }
    const int parts = (a.nsplit == 2 && A >= 2 * kMinSplit) ? 2 : 1;
    const int A0 = parts == 2 ? A - A / 2 : A;
    for (int k = 0; k < parts && A > 0; ++k) {
        const int64_t nk = k ? A - A0 : A0, capk = k ? cap - cap / 2 : cap;  // (state sized by dl_setup)
        if (nk > capk)
            return fail(PSCL_EDEVICE, "retry chain %d: %lld entries exceed its state (%lld)", k, (long long)nk,
                        (long long)capk);
        HIP_TRY(hipStreamWaitEvent(h->retry_stream[cs + k], h->ev_base[p], 0));
        DlState T = b.S[cs + k];
        T.act = b.act[p] + (k ? A0 : 0);
        if (a.d_stage) LAUNCH_TRY("stage", pscl_launch_dl_mark_stage(T.act, nk, a.d_stage, 3, h->retry_stream[cs + k]));
        int r2 = dl_retry_chunk(h, T, k ? A - A0 : A0, a.rounds, a.d_llr, a.d_best, a.d_flags, a.d_attempts,
                                a.d_tried, a.tried_stride, d_cdl, h->retry_stream[cs + k],
                                (h->tune[PSCL_TUNE_DL_STREAMS] & 1) ? h->retry_stream[cs + k] : h->side_stream[cs + k],
                                h->ev_scr[cs + k], h->ev_def[cs + k], a.pipe, beside, a.row_f32);
        if (r2) return r2;
    }
    if (parts == 2) {  // both chains done before the parity's indices are reused
        const int rc = hand_over(h->ev_join[cs >> 1], h->retry_stream[cs + 1], h->retry_stream[cs]);
        if (rc) return rc;
    }
    return record_event(h->ev_retry[p], h->retry_stream[cs]);
}

// a pipelined call's retry chains and DL counters, enqueued on the retry streams (ev_dl marks
// their end; join_pipe orders it into the handle's stream); beside: the next call's baseline is on
// the handle's stream, concurrent with them
int dl_enqueue_deferred(pscl_handle* h, bool beside) {
    if (!h->dl_defer_valid) return PSCL_OK;
    h->dl_defer_valid = false;
    const pscl_dl_call a = h->dl_defer;
    DlBufs b;
    int rc = dl_setup(h, a, b);  // (the sizes of the call's own setup: no allocation)
    if (rc) return rc;
    if ((rc = dl_chain(h, a, b, 0, beside))) return rc;
    hipStream_t rs = h->retry_stream[2 * dl_set(h, a, 0)];
    if (a.d_ref) LAUNCH_TRY("dl_count", pscl_launch_dl_count(a.d_best, a.d_flags, a.d_ref, a.B, h->W, a.k_payload, a.d_counters_dl, rs));
    return h->dl[a.pbase].mark(rs);
}

// the fused TX of a pscl_simulate_device block (PSCL_TUNE_TX_FUSED): the baseline decode draws the
// rows it decodes (scl128_lane.hip TXF), writes the message words to d_ref's buffer and the rows of
// failing and deferred frames to d_llr's, and counts the uncoded baseline into unc
struct TxSpec {
    uint32_t k0 = 0, k1 = 0;
    int64_t frame0 = 0;
    double sigma = 0.0, scale = 0.0, unc_sigma = 0.0;
    int kp = 0;
    double* rows = nullptr;
    uint64_t* msg = nullptr;
    int64_t* unc = nullptr;  // [PSCL_NCOUNT] or null
};
// the baseline the retry chains start from.  mode 0: the plain list decode of all B frames
// (pscl_dlscl_device).  mode 1: the adaptive baseline without a host wait, stream-ordered on the
// handle's stream -- the SC stage, its statistics (d_counters_sc), the escalation
// (adaptive_escalate_enqueue; its statistics go where mode 0 counts the baseline, d_counters_scl).
// mode 2: none, the caller's d_best / d_flags are the baseline (pscl_retry_device).  Modes 1 and 2
// run one chunk without the fused TX and mark d_stage 3 over each chain's entry list.
struct DlBase {
    int mode = 0;
    uint8_t* d_stage = nullptr;
    int64_t* d_counters_sc = nullptr;
    int32_t* d_n_escalated = nullptr;
    // d_llr points at float32 rows: the baseline is the float32 plain decode (pscl_decode_device_f32's
    // launches in mode 0, pscl_adaptive_async_device_f32's in mode 1) and the chains the float32 ones
    bool row_f32 = false;
};

#ifndef PSCL_DL_TAIL_STREAM
#define PSCL_DL_TAIL_STREAM 1
#endif

int retry_args(pscl_handle* h, const uint64_t* d_ref, const int64_t* d_counters_dl) {
    if (!h) return fail(PSCL_EINVAL, "NULL handle");
    if (!h->crc_poly) return fail(PSCL_EINVAL, "retry rounds need a CRC (without one every baseline passes)");
    if (d_ref && !d_counters_dl) return fail(PSCL_EINVAL, "d_ref given without d_counters_dl");
    return PSCL_OK;
}

// the checks before dlscl_impl's own; done: B = 0, nothing is left to enqueue
int adaptive_dlscl_args(pscl_handle* h, int64_t B, const uint64_t* d_ref, int k_payload, const int64_t* d_counters,
                        int32_t* d_n_escalated, bool* done) {
    *done = false;
    int rc = adaptive_async_args(h, B, k_payload);
    if (rc) return rc;
    if (d_ref && !d_counters) return fail(PSCL_EINVAL, "d_ref given without d_counters");
    if (B == 0) {
        *done = true;
        if ((rc = enter(h))) return rc;
        if (d_n_escalated) HIP_TRY(hipMemsetAsync(d_n_escalated, 0, 4, h->stream));
    }
    return PSCL_OK;
}

int dlscl_impl(pscl_handle* h, const double* d_llr, int64_t B, int retries, uint64_t* d_best, uint8_t* d_flags,
               int32_t* d_attempts, int32_t* d_tried, int tried_stride, const uint64_t* d_ref, int k_payload,
               int64_t* d_counters_scl, int64_t* d_counters_dl, const TxSpec* tx, const DlBase& base = DlBase()) {
    if (!h) return fail(PSCL_EINVAL, "NULL handle");
    if (B < 0) return fail(PSCL_EINVAL, "B must be >= 0");
    if (B == 0) return PSCL_OK;
    if (!d_llr || !d_best || !d_flags) return fail(PSCL_EINVAL, "d_llr, d_best and d_flags are required");
    const int mode = base.mode;
    if (d_ref && ((!d_counters_scl && mode != 2) || !d_counters_dl)) return fail(PSCL_EINVAL, "d_ref given without both counters");
    if (k_payload < 0 || k_payload > h->K) return fail(PSCL_EINVAL, "k_payload out of range");
    const int rounds = h->crc_poly && retries > 0 ? (retries < h->K ? retries : h->K) : 0;
    if (d_tried && tried_stride < rounds) return fail(PSCL_EINVAL, "tried_stride < min(retries, K)");
    if (B > INT32_MAX) return fail(PSCL_EUNSUP, "B exceeds 2^31-1");
    const bool f32 = base.row_f32;
    if (f32) {
        if (!h->crc_poly) return fail(PSCL_EINVAL, "float32 DL-SCL chains need a CRC (without one every baseline passes)");
        if (const char* why = f32_chain_unsupported(h)) return fail(PSCL_EUNSUP, "%s", why);
    }
    struct HostClock {  // pscl_host_stats: this call's wall time on the host
        pscl_handle* h;
        std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
        ~HostClock() {
            h->host_call_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
            h->host_calls++;
        }
    } host_clock{h};
    int rc = set_device(h);
    if (rc) return rc;
    pscl_dl_call a;
    a.d_llr = d_llr;
    a.B = B;
    a.rounds = rounds;
    a.d_best = d_best;
    a.d_flags = d_flags;
    a.d_attempts = d_attempts;
    a.d_tried = d_tried;
    a.tried_stride = tried_stride;
    a.d_ref = d_ref;
    a.k_payload = k_payload;
    a.d_counters_dl = d_counters_dl;
    a.mode = mode;
    a.row_f32 = f32;
    a.d_stage = mode ? base.d_stage : nullptr;
    // Chunks (tuning knob PSCL_TUNE_DL_CHUNKS, default 1): the baseline decodes run in order on the handle's
    // stream; the retry entries of chunk c are split over two chains, each on its own retry
    // stream with its own state, so the two chains' rounds overlap each other (and chunk c + 1's
    // baseline decode).  A round is latency-bound (a few 10^4 entries per launch), so a second
    // concurrent chain fills what one leaves idle.  PSCL_TUNE_DL_SPLIT (1 or 2) sets the chains per
    // chunk; chunks below 2 * kMinSplit failing frames keep one chain.  The default is 2 for a
    // blocking call and 1 when pipelined: there the previous call's chains already overlap this
    // one's, and a second chain per call only doubles the host's launches (config 4 measured
    // 2.65 -> 2.38 ms/step with one).
    a.nch = 1;
    a.nsplit = h->N > PSCL_FAST_N ? 0 : (h->pipelined ? 1 : 2);
    if (rounds > 0 && h->tune[PSCL_TUNE_DL_CHUNKS] && !mode) a.nch = h->tune[PSCL_TUNE_DL_CHUNKS];
    if (rounds > 0 && h->N <= PSCL_FAST_N && h->tune[PSCL_TUNE_DL_SPLIT]) a.nsplit = (int)h->tune[PSCL_TUNE_DL_SPLIT];
    a.cap = (B + a.nch - 1) / a.nch;
    // Pipelined (pscl_set_pipelined, one chunk): the call enqueues its baseline, then the retry
    // chains of the PREVIOUS pipelined call (whose baseline has ended or is about to: the host
    // waits only for that one), and leaves its own chains to the next call or join -- so the
    // handle's stream holds back-to-back baselines and the chains (high-priority streams) run
    // beside them, the host never waiting for the baseline it has just enqueued.
    a.pipe = h->pipelined && rounds > 0 && a.nch == 1 && mode != 2;  // (pscl_retry_device runs stream-ordered)
    if (h->dl_defer_valid &&
        (!a.pipe || h->dl_defer.B != B || h->dl_defer.rounds != rounds || h->dl_defer.nsplit != a.nsplit)) {
        // (a different shape: the pending chains first, their state sized as they were)
        if ((rc = dl_enqueue_deferred(h))) return rc;
    }
    // (another baseline than the last call's: every pending tail and chain first)
    if ((rc = join_pipe(h, a.pipe && mode == h->dl_last_mode ? 1 : 3))) return rc;
    h->dl_last_mode = mode;
    a.pbase = a.pipe ? h->dl_par : 0;  // compaction parity of chunk 0
    if (a.pipe) {
        // the chains of the call dl_back calls back may still write their call's outputs (and, kDlPar
        // back, read this parity's compaction output): they end before this call starts (the
        // contract of pscl_set_pipelined: a call's buffers are free again at the dl_back-th following
        // call).  Consecutive calls' chains run concurrently (two chain sets, dl_set), so one call's
        // end does not cover another's; the invariant is by induction instead: every call makes the
        // handle's stream wait for the chains dl_back calls back (ev_dl, here), so any call further
        // back was already waited for by an earlier call; and calls whose pbase has the same parity
        // share one set's streams and DlState, which stream order keeps apart.
        // (PSCL_TUNE_DL_STREAMS bit 2 collapses everything to one set: chains then run in call order.)
        const int q = (a.pbase + kDlPar - h->dl_back) % kDlPar;
        if ((rc = h->dl[q].order(h->stream)) || (rc = h->dl[a.pbase].order(h->stream))) return rc;
    }
    const int W = h->W;
    const int64_t row = h->rm_E ? h->rm_E : h->N;
    const int64_t nch = a.nch, cap = a.cap;
    hipStream_t s = h->stream;
    if (d_attempts) HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)d_attempts, 1, (size_t)B, s));
    if (d_tried) HIP_TRY(hipMemsetAsync(d_tried, 0xff, (size_t)B * tried_stride * 4, s));
    DlBufs bufs;
    if (rounds > 0 && (rc = dl_setup(h, a, bufs))) return rc;
    for (int64_t c = 0; c < nch; ++c) {
        const int64_t c0 = c * cap, nc = (B - c0) < cap ? (B - c0) : cap;
        // baseline SCL (flip.py:79-80) of chunk c
        pscl_decode_params P;
        fill_decode_params(h, P, 0);
        P.llr = f32 ? (const double*)((const float*)d_llr + c0 * row) : d_llr + c0 * row;
        pscl_set_row_type(P, f32);
        P.B = nc;
        P.best = d_best + c0 * W;
        P.flags = d_flags + c0;
        P.ref = d_ref ? d_ref + c0 * W : nullptr;
        P.k_payload = k_payload;
        P.counters = d_counters_scl;
        // (N = 128: the DL-SCL baseline's screening kernel, PSCL_TUNE_DL_LANE; by default the
        // lane-per-path one at L = 8 and the two-lanes-per-path one at L = 4, which measured faster
        // beside the retry chains)
        if (rounds > 0) {
            const int64_t dl_lane = h->tune[PSCL_TUNE_DL_LANE] ? h->tune[PSCL_TUNE_DL_LANE]
                                                               : (PSCL_DL_LANE_DEFAULT ? PSCL_DL_LANE_DEFAULT : (h->L == 8 ? 1 : 2));
            // (float32 rows: the lane-per-path kernel at both L -- the two-lanes-per-path screening
            // kernel has no float32 form, and the results are the same by construction)
            P.no_lane = dl_lane != 1 && !f32;
        }
        if (tx) {  // the fused TX: the lane kernel draws the chunk's rows (simulate_enqueue checked it applies)
            P.no_lane = 0;
            P.tx = 1;
            P.tx_k0 = tx->k0;
            P.tx_k1 = tx->k1;
            P.tx_kp = tx->kp;
            P.tx_crc_deg = h->crc_deg;
            P.tx_frame0 = tx->frame0 + c0;
            P.tx_sigma = tx->sigma;
            P.tx_scale = tx->scale;
            P.tx_unc_sigma = tx->unc_sigma;
            P.tx_crctab = h->d_crctab;
            P.tx_xtab = h->d_xtab;
            P.tx_rows = tx->rows + c0 * row;
            P.tx_msg = tx->msg + c0 * W;
            P.tx_unc_counters = tx->unc;
        }
        if (pscl_decode_wpg(P) < 1) return fail(PSCL_EUNSUP, "LDS budget exceeded (L=%d, K=%d)", h->L, h->K);
        // a pipelined call's baseline tail (re-decode, compaction, count) on tail_stream: the next
        // call's baseline follows this one's screening pass directly
        hipStream_t ts = s;
        const int tpar = a.pbase & 1;
        if (a.pipe && !mode && PSCL_DL_TAIL_STREAM && !h->tune[PSCL_TUNE_DL_TAIL]) {
            if (!h->tail_stream) HIP_TRY(create_priority_stream(h, &h->tail_stream));
            ts = h->tail_stream;
        }
        if (mode == 1) {
            int q = 0;
            if ((rc = adaptive_begin(h, false, &q))) return rc;
            if ((rc = launch_sc_stage(h, d_llr, B, d_best, d_flags, base.d_stage, f32))) return rc;
            if (d_ref) LAUNCH_TRY("dl_count", pscl_launch_dl_count(d_best, d_flags, d_ref, B, W, k_payload, base.d_counters_sc, s));
            hipEvent_t t1;  // (stage 2 -- compaction, row-list decode, re-decode, statistics -- as one timed launch)
            if ((rc = timed_begin(h, s, &t1))) return rc;
            if ((rc = adaptive_escalate_enqueue(h, q, false, d_llr, B, d_best, d_flags, d_ref, k_payload, d_counters_scl,
                                                base.d_n_escalated, f32)))
                return rc;
            if (t1) HIP_TRY(hipEventRecord(t1, s));
        } else if (mode == 0) {
            if ((rc = launch_decode(h, P, 0, s, kLongScratch, false, ts != s ? ts : nullptr, tpar))) return rc;
        }
        if (rounds > 0) {
            const int p = dl_parity(a, c);
            if (c >= 2) HIP_TRY(hipStreamWaitEvent(ts, h->ev_retry[p], 0));  // the parity's indices free again
            HIP_TRY(hipMemsetAsync(bufs.cnt[p], 0, 4, ts));
            LAUNCH_TRY("dl_compact", pscl_launch_dl_compact(d_flags + c0, nc, c0, bufs.act[p], nullptr, bufs.cnt[p], ts));
            // fused TX: the failing frames' rows, read by the retry chain (entries hold call-level frame
            // indices c0 + f)
            if (tx) LAUNCH_TRY("tx_rows", pscl_launch_tx_rows(P, bufs.act[p], bufs.cnt[p], nc, tx->rows, tx->frame0, ts));
            HIP_TRY(hipMemcpyAsync(h->h_count + p, bufs.cnt[p], 4, hipMemcpyDeviceToHost, ts));
            if ((rc = record_event(h->ev_base[p], ts))) return rc;
        }
        // the end of the tail: its compaction, or (no rounds) its re-decode
        if (ts != s && (rc = h->tail[tpar].mark(ts))) return rc;
        if (rounds > 0 && c >= 1 && (rc = dl_chain(h, a, bufs, c - 1, true))) return rc;
    }
    if (a.pipe) {
        // the previous call's chains now (its baseline precedes this call's on the stream), this
        // call's at the next call or join
        if ((rc = dl_enqueue_deferred(h, true))) return rc;
        h->dl_defer = a;
        h->dl_defer_valid = true;
        h->dl_par = (h->dl_par + 1) % kDlPar;
        return PSCL_OK;
    }
    if (rounds > 0) {
        if ((rc = dl_chain(h, a, bufs, nch - 1, false))) return rc;
        // (the chunk chains alternate two sets: the last two end every chain)
        HIP_TRY(hipStreamWaitEvent(s, h->ev_retry[dl_parity(a, nch - 1)], 0));
        if (nch >= 2) HIP_TRY(hipStreamWaitEvent(s, h->ev_retry[dl_parity(a, nch - 2)], 0));
    }
    if (d_ref) LAUNCH_TRY("dl_count", pscl_launch_dl_count(d_best, d_flags, d_ref, B, W, k_payload, d_counters_dl, s));
    return PSCL_OK;
}

int decode_host(pscl_handle* h, const double* llr, int64_t B, const int8_t* forced, int32_t* n_paths, int8_t* best_bits,
                uint8_t* crc_pass, int32_t* best_idx, double* metrics, int8_t* cands, double* info_llrs, int sc_hard) {
    if (!h) return fail(PSCL_EINVAL, "NULL handle");
    if (B < 0) return fail(PSCL_EINVAL, "B must be >= 0");
    if (B == 0) return PSCL_OK;
    if (!llr || !n_paths) return fail(PSCL_EINVAL, "llr and n_paths are required");
    const int K = h->K, L = h->L, W = h->W, N = h->N;
    std::vector<uint64_t> hforce;
    if (forced) {
        hforce.assign((size_t)B * 2 * W, 0);
        for (int64_t b = 0; b < B; ++b) {
            uint64_t* fr = &hforce[(size_t)b * 2 * W];
            for (int jj = 0; jj < K; ++jj) {
                int v = forced[b * K + jj];
                if (v == 0 || v == 1) {
                    fr[jj >> 6] |= 1ULL << (jj & 63);
                    if (v) fr[W + (jj >> 6)] |= 1ULL << (jj & 63);
                } else if (v != -1) {
                    return fail(PSCL_EINVAL, "force_info_bits entries must be -1, 0, or 1");
                }
            }
        }
    }
    int rc = enter(h);
    if (rc) return rc;
    void *d_llr, *d_force = nullptr, *d_np, *d_best, *d_flags, *d_met = nullptr, *d_cands = nullptr, *d_illr = nullptr;
    const size_t sz_llr = (size_t)B * (h->rm_E ? h->rm_E : N) * 8;
    if ((rc = ensure(h, kHostLlr, sz_llr, &d_llr))) return rc;
    if (forced && (rc = ensure(h, kHostForce, hforce.size() * 8, &d_force))) return rc;
    if ((rc = ensure(h, kHostNPaths, (size_t)B * 4, &d_np))) return rc;
    if ((rc = ensure(h, kHostBest, (size_t)B * W * 8, &d_best))) return rc;
    if ((rc = ensure(h, kHostFlags, (size_t)B, &d_flags))) return rc;
    if (metrics && (rc = ensure(h, kHostMetrics, (size_t)B * L * 8, &d_met))) return rc;
    if (cands && (rc = ensure(h, kHostCands, (size_t)B * L * W * 8, &d_cands))) return rc;
    if (info_llrs && (rc = ensure(h, kHostInfoLlrs, (size_t)B * L * (K > 0 ? K : 1) * 8, &d_illr))) return rc;
    HIP_TRY(hipMemcpyAsync(d_llr, llr, sz_llr, hipMemcpyHostToDevice, h->stream));
    if (forced) HIP_TRY(hipMemcpyAsync(d_force, hforce.data(), hforce.size() * 8, hipMemcpyHostToDevice, h->stream));
    const int hist = info_llrs != nullptr;
    pscl_decode_params P;
    fill_decode_params(h, P, hist);
    P.llr = (const double*)d_llr;
    P.B = B;
    P.force = (const uint64_t*)d_force;
    P.n_paths = (int32_t*)d_np;
    P.best = (uint64_t*)d_best;
    P.flags = (uint8_t*)d_flags;
    P.metrics = (double*)d_met;
    P.cands = (uint64_t*)d_cands;
    P.info_llrs = (double*)d_illr;
    P.sc_hard = sc_hard;
    if (pscl_decode_wpg(P) < 1) return fail(PSCL_EUNSUP, "LDS budget exceeded (L=%d, K=%d)", h->L, h->K);
    if ((rc = launch_decode(h, P, hist))) return rc;
    std::vector<int32_t> hnp((size_t)B);
    std::vector<uint64_t> hbest((size_t)B * W);
    std::vector<uint8_t> hflags((size_t)B);
    HIP_TRY(hipMemcpyAsync(hnp.data(), d_np, (size_t)B * 4, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipMemcpyAsync(hbest.data(), d_best, (size_t)B * W * 8, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipMemcpyAsync(hflags.data(), d_flags, (size_t)B, hipMemcpyDeviceToHost, h->stream));
    std::vector<uint64_t> hc;
    if (cands) {
        hc.resize((size_t)B * L * W);
        HIP_TRY(hipMemcpyAsync(hc.data(), d_cands, hc.size() * 8, hipMemcpyDeviceToHost, h->stream));
    }
    if (metrics) HIP_TRY(hipMemcpyAsync(metrics, d_met, (size_t)B * L * 8, hipMemcpyDeviceToHost, h->stream));
    if (info_llrs)
        HIP_TRY(hipMemcpyAsync(info_llrs, d_illr, (size_t)B * L * K * 8, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    for (int64_t b = 0; b < B; ++b) {
        n_paths[b] = hnp[(size_t)b];
        if (best_bits)
            for (int jj = 0; jj < K; ++jj)
                best_bits[b * K + jj] = (int8_t)((hbest[(size_t)b * W + (jj >> 6)] >> (jj & 63)) & 1);
        if (crc_pass) crc_pass[b] = (hflags[(size_t)b] & PSCL_FLAG_CRC_PASS) ? 1 : 0;
        if (best_idx) best_idx[b] = (int32_t)(hflags[(size_t)b] & PSCL_FLAG_IDX_MASK);
        if (cands)
            for (int r = 0; r < L; ++r)
                for (int jj = 0; jj < K; ++jj)
                    cands[((size_t)b * L + r) * K + jj] =
                        (int8_t)((hc[((size_t)b * L + r) * W + (jj >> 6)] >> (jj & 63)) & 1);
    }
    return PSCL_OK;
}

int uncoded_launch(pscl_handle* h, uint64_t seed, uint32_t stream_id, double ebno_db, int k_payload, int64_t frame0,
                   int64_t B, int64_t* d_counters, bool no_enter) {
    if (!h) return fail(PSCL_EINVAL, "NULL handle");
    if (B < 0 || frame0 < 0) return fail(PSCL_EINVAL, "B and frame0 must be >= 0");
    if (B == 0) return PSCL_OK;
    if (!d_counters) return fail(PSCL_EINVAL, "d_counters is NULL");
    if (k_payload < 0 || k_payload > PSCL_MAX_N) return fail(PSCL_EINVAL, "k_payload out of range");
    int rc = no_enter ? set_device(h) : enter(h);
    if (rc) return rc;
    pscl_channel_params P;
    memset(&P, 0, sizeof(P));
    P.seed = seed;
    P.stream_id = stream_id;
    P.k_payload = k_payload;
    const double ebno = pow(10.0, ebno_db / 10.0);
    P.noise_var = 1.0 / (2.0 * ebno);  // run_fer_sweep.py:66-67
    P.sigma = sqrt(P.noise_var);
    P.frame0 = frame0;
    P.B = B;
    LAUNCH_TRY("uncoded kernel", pscl_launch_uncoded(P, d_counters, h->stream));
    return PSCL_OK;
}

// the TX launch (pscl_channel_device); d_unc != null also counts the uncoded baseline of the
// same frames (N <= 128: channel_kernel's phase A); no_enter: pending pipelined DL-SCL chains stay
// where they are (pscl_simulate_device: they overlap this TX)
int channel_launch(pscl_handle* h, uint64_t seed, uint32_t stream_id, double ebno_db, double rate, int k_payload,
                   int64_t frame0, int64_t B, double* d_llr, uint64_t* d_msg, int64_t* d_unc, bool no_enter = false) {
    if (!h) return fail(PSCL_EINVAL, "NULL handle");
    if (B < 0 || frame0 < 0) return fail(PSCL_EINVAL, "B and frame0 must be >= 0");
    if (B == 0) return PSCL_OK;
    if (!d_llr) return fail(PSCL_EINVAL, "d_llr is NULL");
    if (!(rate > 0)) return fail(PSCL_EINVAL, "rate must be positive");
    if (k_payload + h->crc_deg != h->K || k_payload < 0)
        return fail(PSCL_EINVAL, "k_payload (%d) + crc degree (%d) must equal K (%d)", k_payload, h->crc_deg, h->K);
    int rc = no_enter ? set_device(h) : enter(h);
    if (rc) return rc;
    pscl_channel_params P;
    memset(&P, 0, sizeof(P));
    P.seed = seed;
    P.stream_id = stream_id;
    P.N = h->N;
    P.K = h->K;
    P.W = h->W;
    P.k_payload = k_payload;
    P.crc_deg = h->crc_deg;
    P.xtab = h->d_xtab;
    P.crctab = h->d_crctab;
    const double ebno = pow(10.0, ebno_db / 10.0);
    P.noise_var = 1.0 / (2.0 * rate * ebno);
    P.sigma = sqrt(P.noise_var);
    P.llr_scale = 2.0 / P.noise_var;
    P.frame0 = frame0;
    P.B = B;
    P.llr = d_llr;
    P.msg = d_msg;
    P.rm_E = h->rm_E;
    P.rm_order = h->d_rm_order;
    if (d_unc) {
        P.unc_counters = d_unc;
        P.unc_sigma = sqrt(1.0 / (2.0 * ebno));  // run_fer_sweep.py:66-67 (uncoded: R = 1)
    }
    LAUNCH_TRY("channel kernel", pscl_launch_channel(P, h->stream));
    return PSCL_OK;
}

#ifndef PSCL_TX_FUSED_DEFAULT
#define PSCL_TX_FUSED_DEFAULT 0
#endif
// whether a pscl_simulate[_device] block takes the fused TX (PSCL_TUNE_TX_FUSED, default
// PSCL_TX_FUSED_DEFAULT): its baseline decode must be the screening lane kernel of the (128,64) code
// on plain rows (L = 4 or 8), which then draws the rows itself
bool tx_fused_applies(const pscl_handle* h, int k_payload) {
    const int64_t k = h->tune[PSCL_TUNE_TX_FUSED];
    if (!(k == 1 || (k == 0 && PSCL_TX_FUSED_DEFAULT))) return false;
    if (h->N != 128 || h->rm_E || !h->screen || (h->L != 8 && h->L != 4) || k_payload + h->crc_deg != h->K) return false;
    pscl_decode_params T;
    fill_decode_params(h, T, 0);
    T.B = 1;
    T.apx = 1;
    return pscl_lane_available(T) != 0;
}

// the four buffers of a simulate block of `chunk` frames (the IoField slots from base on)
int ensure_io(pscl_handle* h, int base, int64_t chunk, int64_t row, void** d_llr, void** d_msg, void** d_best, void** d_flags) {
    int rc;
    if ((rc = ensure(h, base + kIoRows, (size_t)chunk * row * 8, d_llr))) return rc;
    if ((rc = ensure(h, base + kIoMsg, (size_t)chunk * h->W * 8, d_msg))) return rc;
    if ((rc = ensure(h, base + kIoBest, (size_t)chunk * h->W * 8, d_best))) return rc;
    return ensure(h, base + kIoFlags, (size_t)chunk, d_flags);
}

// One SNR point of run_sweep enqueued (pscl_simulate / pscl_simulate_device): chunks of at most
// 2^20 frames through handle scratch (8 bytes per LLR of a row -- N of them, or E on a rate-matched
// handle: about 1 GiB per chunk at N = 128), each = TX (+ the uncoded baseline) +
// pscl_dlscl_device.  On a pipelined handle every chunk is one pipelined DL-SCL call: its retry
// chains overlap the next chunk's (or the next point's) TX and baseline, so kDlPar scratch sets
// rotate with the DL-SCL call parity, and a set is rewritten only after the chains of the call
// kDlPar back that used it have ended.
// adaptive (pscl_simulate_adaptive_dl[_device]): every chunk is a three-stage call instead -- no fused
// TX, and cs has four rows: SC, adaptive baseline, final, uncoded.
int simulate_enqueue(pscl_handle* h, uint64_t seed, uint32_t stream_id, double ebno_db, double rate, int k_payload,
                     int64_t frame0, int64_t B, int retries, int include_uncoded, int64_t* cs, bool adaptive = false) {
    int64_t* const cs_unc = cs + (adaptive ? 3 : 2) * PSCL_NCOUNT;
    const int64_t chunk = B < (1 << 20) ? B : (1 << 20);
    const int N = h->N;
    // (a rate-matched handle: the TX launch writes, and dlscl_impl reads, rows of rm_E doubles; the
    // other scratch of the call -- message and best words, flags, the chains' state -- is per frame)
    const int64_t row = h->rm_E ? h->rm_E : N;
    int rc;
    for (int64_t f = 0; f < B; f += chunk) {
        const int64_t n = B - f < chunk ? B - f : chunk;
        const int par = h->pipelined ? h->dl_par : 0;
        // (the chains that last read this scratch set)
        if (h->pipelined && (rc = h->dl[par].order(h->stream))) return rc;
        void *d_llr, *d_msg, *d_best, *d_flags;
        // (pipelined: every parity's set sized at once, so the first call warms all of them and no
        // later call of a sweep allocates -- ~130 us of hipMalloc on the host per new set)
        for (int q = h->pipelined ? 0 : par; q <= (h->pipelined ? kDlPar - 1 : par); ++q)
            if ((rc = ensure_io(h, slot_sim(q, 0), chunk, row, &d_llr, &d_msg, &d_best, &d_flags))) return rc;
        if ((rc = ensure_io(h, slot_sim(par, 0), chunk, row, &d_llr, &d_msg, &d_best, &d_flags))) return rc;
        // the fused TX (PSCL_TUNE_TX_FUSED): the baseline decode draws the rows itself -- where its
        // screening launch is the lane kernel of the (128,64) code on plain rows
        TxSpec tx;
        const bool fused = !adaptive && tx_fused_applies(h, k_payload);
        if (fused) {
            h->n_fused_tx++;
            tx.k0 = (uint32_t)seed;
            tx.k1 = (uint32_t)(seed >> 32) ^ (stream_id * 0x85EBCA6Bu);  // (channel_kernel's key)
            tx.frame0 = frame0 + f;
            const double ebno = pow(10.0, ebno_db / 10.0);
            const double nv = 1.0 / (2.0 * rate * ebno);  // (channel_launch's parameters)
            tx.sigma = sqrt(nv);
            tx.scale = 2.0 / nv;
            tx.unc_sigma = sqrt(1.0 / (2.0 * ebno));
            tx.kp = k_payload;
            tx.rows = (double*)d_llr;
            tx.msg = (uint64_t*)d_msg;
            tx.unc = include_uncoded ? cs_unc : nullptr;
        } else {
            // N <= 128: the uncoded baseline is counted by the TX launch itself (same payload draw)
            const bool unc_fused = include_uncoded && N <= PSCL_FAST_N;
            if ((rc = channel_launch(h, seed, stream_id, ebno_db, rate, k_payload, frame0 + f, n, (double*)d_llr,
                                     (uint64_t*)d_msg, unc_fused ? cs_unc : nullptr, true)))
                return rc;
            if (include_uncoded && !unc_fused &&
                (rc = uncoded_launch(h, seed, stream_id, ebno_db, k_payload, frame0 + f, n, cs_unc, true)))
                return rc;
        }
        const int back = h->dl_back;
        h->dl_back = kDlPar;  // (its own scratch set: kDlPar sets rotate with the call parity)
        if (adaptive) {
            DlBase base;
            base.mode = 1;
            base.d_counters_sc = cs;
            rc = dlscl_impl(h, (const double*)d_llr, n, retries, (uint64_t*)d_best, (uint8_t*)d_flags, nullptr, nullptr, 0,
                            (const uint64_t*)d_msg, k_payload, cs + PSCL_NCOUNT, cs + 2 * PSCL_NCOUNT, nullptr, base);
        } else {
            rc = dlscl_impl(h, (const double*)d_llr, n, retries, (uint64_t*)d_best, (uint8_t*)d_flags, nullptr, nullptr, 0,
                            (const uint64_t*)d_msg, k_payload, cs, cs + PSCL_NCOUNT, fused ? &tx : nullptr);
        }
        h->dl_back = back;
        if (rc) return rc;
    }
    return PSCL_OK;
}

// pscl_simulate_adaptive[_device]: chunks of at most 2^20 frames through handle scratch (kSimAd:
// rows, messages, best words, flags), each = TX (+ the uncoded baseline), the SC stage,
// its statistics (row 0), and the escalation without a host wait with the final statistics (row 1).
// Stream-ordered on the handle's stream: consecutive chunks reuse the scratch in stream order.
int simulate_adaptive_enqueue(pscl_handle* h, uint64_t seed, uint32_t stream_id, double ebno_db, double rate, int k_payload,
                              int64_t frame0, int64_t B, int include_uncoded, int64_t* cs) {
    const int64_t chunk = B < (1 << 20) ? B : (1 << 20);
    const int W = h->W;
    const int64_t row = h->rm_E ? h->rm_E : h->N;
    const int64_t regrown = h->n_regrow;
    int rc;
    void *d_llr, *d_msg, *d_best, *d_flags;
    if ((rc = ensure_io(h, kSimAd, chunk, row, &d_llr, &d_msg, &d_best, &d_flags))) return rc;
    h->n_ad_waits += h->n_regrow - regrown;
    for (int64_t f = 0; f < B; f += chunk) {
        const int64_t n = B - f < chunk ? B - f : chunk;
        // N <= 128: the uncoded baseline is counted by the TX launch itself (same payload draw)
        const bool unc_fused = include_uncoded && h->N <= PSCL_FAST_N;
        if ((rc = channel_launch(h, seed, stream_id, ebno_db, rate, k_payload, frame0 + f, n, (double*)d_llr,
                                 (uint64_t*)d_msg, unc_fused ? cs + 2 * PSCL_NCOUNT : nullptr, true)))
            return rc;
        if (include_uncoded && !unc_fused &&
            (rc = uncoded_launch(h, seed, stream_id, ebno_db, k_payload, frame0 + f, n, cs + 2 * PSCL_NCOUNT, true)))
            return rc;
        int q = 0;
        if ((rc = adaptive_begin(h, false, &q))) return rc;
        if ((rc = launch_sc_stage(h, (const double*)d_llr, n, (uint64_t*)d_best, (uint8_t*)d_flags, nullptr))) return rc;
        LAUNCH_TRY("dl_count", pscl_launch_dl_count((const uint64_t*)d_best, (const uint8_t*)d_flags, (const uint64_t*)d_msg, n, W,
                                                    k_payload, cs, h->stream));
        if ((rc = adaptive_escalate_enqueue(h, q, false, (const double*)d_llr, n, (uint64_t*)d_best, (uint8_t*)d_flags,
                                            (const uint64_t*)d_msg, k_payload, cs + PSCL_NCOUNT, nullptr)))
            return rc;
    }
    return PSCL_OK;
}

// the launch of the caller-payload TX (encode.hip): every argument is checked before any device call
int encode_launch(pscl_handle* h, const uint64_t* d_payload, int64_t frame0, int64_t B, uint64_t* d_msg, uint64_t* d_code,
                  void* d_rows, int row_mode, int row_f32, uint64_t seed, uint32_t stream_id, double ebno_db, double rate) {
    if (!h) return fail(PSCL_EINVAL, "NULL handle");
    if (!d_payload) return fail(PSCL_EINVAL, "d_payload is NULL");
    if (B < 0 || frame0 < 0) return fail(PSCL_EINVAL, "B and frame0 must be >= 0");
    if (!d_msg && !d_code && !d_rows) return fail(PSCL_EINVAL, "every output is NULL");
    if (row_mode == PSCL_ROWS_LLR && !(rate > 0)) return fail(PSCL_EINVAL, "rate must be positive");
    if (row_f32 != 0 && row_f32 != 1) return fail(PSCL_EINVAL, "the dtype flag must be 0 (float64) or 1 (float32)");
    if (B > PSCL_ENCODE_MAX_B) return fail(PSCL_EUNSUP, "B exceeds the %lld frames of one launch", PSCL_ENCODE_MAX_B);
    if (B == 0) return PSCL_OK;
    const int rc = enter(h);
    if (rc) return rc;
    pscl_encode_params P;
    memset(&P, 0, sizeof(P));
    P.payload = d_payload;
    P.B = B;
    P.frame0 = frame0;
    P.N = h->N;
    P.K = h->K;
    P.W = h->W;
    P.k_payload = h->K - h->crc_deg;
    P.Wp = PSCL_WORDS(P.k_payload);
    P.crc_deg = h->crc_deg;
    P.rm_E = h->rm_E;
    P.row_mode = row_mode;
    P.row_f32 = row_f32;
    P.xtab = h->d_xtab;
    P.crctab = h->d_crctab;
    P.rm_order = h->d_rm_order;
    P.msg = d_msg;
    P.code = d_code;
    P.rows = d_rows;
    if (row_mode == PSCL_ROWS_LLR) {  // (channel_launch's parameters and channel_kernel's key)
        const double nv = 1.0 / (2.0 * rate * pow(10.0, ebno_db / 10.0));
        P.sigma = sqrt(nv);
        P.llr_scale = 2.0 / nv;
        P.k0 = (uint32_t)seed;
        P.k1 = (uint32_t)(seed >> 32) ^ (stream_id * 0x85EBCA6Bu);
    }
    LAUNCH_TRY("encode kernel", pscl_launch_encode(P, h->stream));
    return PSCL_OK;
}

int tail_scan(pscl_handle* h, uint32_t lo, uint32_t hi, uint64_t* d_out, int bits) {
    if (!h) return fail(PSCL_EINVAL, "NULL handle");
    if (!d_out) return fail(PSCL_EINVAL, "d_out is required");
    if (lo > hi) return fail(PSCL_EINVAL, "lo > hi");
    int rc = enter(h);
    if (rc) return rc;
    LAUNCH_TRY("tail scan", pscl_launch_tail_abs_scan(lo, hi, h->d_exp_table, reinterpret_cast<unsigned long long*>(d_out), h->stream, bits));
    return PSCL_OK;
}

}  // namespace

extern "C" {

const char* pscl_last_error(void) { return g_err.c_str(); }

int pscl_abi_version(void) { return PSCL_ABI_VERSION; }

const char* pscl_build_hash(void) { return kBuildHash + 16; }

int pscl_device_count(void) {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e == hipErrorNoDevice) return 0;
    if (e != hipSuccess) return fail(PSCL_EDEVICE, "hipGetDeviceCount: %s", hipGetErrorString(e));
    return n;
}

int pscl_create(pscl_handle** out, int device, int N, const int32_t* info_set, int K, int L, uint64_t crc_poly) {
    if (!out) return fail(PSCL_EINVAL, "out is NULL");
    *out = nullptr;
    if (N <= 1 || (N & (N - 1))) return fail(PSCL_EINVAL, "Channel LLR length must be a power of two");
    if (N > PSCL_MAX_N) return fail(PSCL_EUNSUP, "N=%d exceeds PSCL_MAX_N=%d", N, PSCL_MAX_N);
    if (L <= 0) return fail(PSCL_EINVAL, "List size M must be positive");
    if (L > PSCL_MAX_L) return fail(PSCL_EUNSUP, "list size %d exceeds PSCL_MAX_L=%d", L, PSCL_MAX_L);
    if (K < 0 || K > N || (K > 0 && !info_set)) return fail(PSCL_EINVAL, "info_set must hold 0..N indices");
    pscl_handle tmp;
    tmp.N = N;
    while ((1 << tmp.n) < N) tmp.n++;
    tmp.K = K;
    tmp.L = L;
    tmp.W = K > 64 ? (K + 63) / 64 : 1;
    tmp.crc_poly = crc_poly;
    tmp.info_words.assign((size_t)(N >= 64 ? N / 64 : 1), 0ULL);
    for (int i = 0; i < K; ++i) {
        int p = info_set[i];
        if (p < 0 || p >= N) return fail(PSCL_EINVAL, "info_set indices out of range");
        uint64_t bit = 1ULL << (p & 63);
        if (tmp.info_words[(size_t)(p >> 6)] & bit) return fail(PSCL_EUNSUP, "duplicate info_set index %d", p);
        tmp.info_words[(size_t)(p >> 6)] |= bit;
        if (p < PSCL_FAST_N) tmp.info_mask[p >> 6] |= bit;
        tmp.info_set.push_back(p);
    }
    // The decoder visits info phases in increasing phase order; candidate bit j belongs to
    // info_set[j] (u[info_set], scl.py:183).  Both orders agree only for sorted info sets.
    for (int i = 1; i < K; ++i)
        if (tmp.info_set[i] < tmp.info_set[i - 1]) return fail(PSCL_EUNSUP, "info_set must be sorted ascending");
    tmp.check_cols.assign((size_t)(K > 0 ? K : 1), 0u);
    if (crc_poly) {
        tmp.crc_deg = poly_degree(crc_poly);
        if (tmp.crc_deg <= 0) return fail(PSCL_EINVAL, "Polynomial degree must be positive");
        if (tmp.crc_deg > PSCL_MAX_CRC) return fail(PSCL_EUNSUP, "CRC degree %d > %d", tmp.crc_deg, PSCL_MAX_CRC);
        if (K <= tmp.crc_deg) return fail(PSCL_EINVAL, "Message too short for the provided CRC polynomial");
        for (int jj = 0; jj < K; ++jj) {
            std::vector<uint8_t> e((size_t)K, 0);
            e[(size_t)jj] = 1;
            tmp.check_cols[(size_t)jj] = crc_remainder(e, crc_poly, tmp.crc_deg);
        }
        const int kp = K - tmp.crc_deg;
        tmp.attach_cols.assign((size_t)(kp > 0 ? kp : 1), 0u);
        for (int jj = 0; jj < kp; ++jj) {
            std::vector<uint8_t> e((size_t)(kp + tmp.crc_deg), 0);
            e[(size_t)jj] = 1;
            tmp.attach_cols[(size_t)jj] = crc_remainder(e, crc_poly, tmp.crc_deg);
        }
    } else {
        tmp.attach_cols.assign((size_t)(K > 0 ? K : 1), 0u);
    }
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev == 0)
        return fail(PSCL_EDEVICE, "no HIP device available (%s)", e == hipSuccess ? "0 devices" : hipGetErrorString(e));
    if (device < 0 || device >= ndev) return fail(PSCL_EINVAL, "device %d out of range (%d devices)", device, ndev);
    pscl_handle* h = new pscl_handle(tmp);
    h->device = device;
    int rc = set_device(h);
    if (rc) {
        delete h;
        return rc;
    }
#define CREATE_TRY(expr)                                                         \
    do {                                                                         \
        hipError_t _e = (expr);                                                  \
        if (_e != hipSuccess) {                                                  \
            int _c = fail(PSCL_EDEVICE, "%s: %s", #expr, hipGetErrorString(_e)); \
            pscl_destroy(h);                                                     \
            return _c;                                                           \
        }                                                                        \
    } while (0)
    CREATE_TRY(hipStreamCreateWithFlags(&h->own_stream, hipStreamNonBlocking));
    h->stream = h->own_stream;
    CREATE_TRY(hipMalloc(&h->d_check_cols, h->check_cols.size() * 4));
    CREATE_TRY(hipMalloc(&h->d_attach_cols, h->attach_cols.size() * 4));
    CREATE_TRY(hipMalloc(&h->d_info_set, (size_t)(K > 0 ? K : 1) * 4));
    CREATE_TRY(hipMalloc(&h->d_exp_table, sizeof(kExpTable)));
    CREATE_TRY(hipMalloc(&h->d_info_words, h->info_words.size() * 8));
    CREATE_TRY(hipMemcpy(h->d_info_words, h->info_words.data(), h->info_words.size() * 8, hipMemcpyHostToDevice));
    CREATE_TRY(hipMemcpy(h->d_check_cols, h->check_cols.data(), h->check_cols.size() * 4, hipMemcpyHostToDevice));
    CREATE_TRY(hipMemcpy(h->d_attach_cols, h->attach_cols.data(), h->attach_cols.size() * 4, hipMemcpyHostToDevice));
    if (K > 0) CREATE_TRY(hipMemcpy(h->d_info_set, h->info_set.data(), (size_t)K * 4, hipMemcpyHostToDevice));
    CREATE_TRY(hipMemcpy(h->d_exp_table, kExpTable, sizeof(kExpTable), hipMemcpyHostToDevice));
    {
        // NR sub-block interleaver tables (interleaver.py:10-37: order[k] = (k % 32) nb + k / 32 over
        // nb * 32 positions, the identity when N < 32) -- a function of N alone, so they are uploaded
        // here once; pscl_set_rate_match only switches rate matching on or off (no device write
        // while pipelined work may be reading them)
        std::vector<int32_t> order((size_t)N), src((size_t)N);
        const int nb = (N + 31) / 32;
        for (int k = 0; k < N; ++k) order[(size_t)k] = N >= 32 ? (k % 32) * nb + k / 32 : k;
        for (int k = 0; k < N; ++k) src[(size_t)order[(size_t)k]] = k;
        CREATE_TRY(hipMalloc(&h->d_rm_src, (size_t)N * 4));
        CREATE_TRY(hipMalloc(&h->d_rm_order, (size_t)N * 4));
        CREATE_TRY(hipMemcpy(h->d_rm_src, src.data(), (size_t)N * 4, hipMemcpyHostToDevice));
        CREATE_TRY(hipMemcpy(h->d_rm_order, order.data(), (size_t)N * 4, hipMemcpyHostToDevice));
    }
    {
        // scl128 epilogue: gather[k][v] = the information bits of u-byte k (value v), compacted
        // in index order; syn[m][v] = XOR of the CRC check columns of info bits 4m..4m+3 set in v
        // (N > 128: N / 8 gather tables, scl_lane_long.hip)
        const int k4 = (K + 3) / 4, nby = N > 128 ? N / 8 : 16;
        std::vector<uint8_t> epi((size_t)nby * 256 + (size_t)k4 * 16 * 4, 0);
        for (int k = 0; k < nby; ++k)
            for (int v = 0; v < 256; ++v) {
                int c = 0, cntb = 0;
                for (int t = 0; t < 8; ++t) {
                    const int p = 8 * k + t;
                    if (p < N && ((h->info_words[p >> 6] >> (p & 63)) & 1ULL)) {
                        if ((v >> t) & 1) c |= 1 << cntb;
                        cntb++;
                    }
                }
                epi[(size_t)k * 256 + v] = (uint8_t)c;
            }
        uint32_t* syn = reinterpret_cast<uint32_t*>(epi.data() + (size_t)nby * 256);
        for (int m = 0; m < k4; ++m)
            for (int v = 0; v < 16; ++v) {
                uint32_t acc = 0;
                for (int t = 0; t < 4; ++t)
                    if (4 * m + t < K && ((v >> t) & 1)) acc ^= h->check_cols[(size_t)(4 * m + t)];
                syn[m * 16 + v] = acc;
            }
        epi.resize((epi.size() + 7) & ~(size_t)7, 0);
        h->epi_words = (int)(epi.size() / 8);
        CREATE_TRY(hipMalloc(&h->d_epi, epi.size()));
        CREATE_TRY(hipMemcpy(h->d_epi, epi.data(), epi.size(), hipMemcpyHostToDevice));
    }
    {
        // TX tables: encode and CRC attach are GF(2)-linear, so byte-wise tables give them in
        // ceil(K/8) (resp. ceil(kp/8)) lookups per frame.  Codeword words per entry: 2 for
        // N <= 128 (channel_kernel), N / 64 for the long codes (channel_long_kernel).
        const int nb = (K + 7) / 8, kp = K - h->crc_deg, nbp = (kp + 7) / 8;
        const int XW = N <= PSCL_FAST_N ? 2 : N / 64;
        std::vector<uint64_t> xt((size_t)(nb > 0 ? nb : 1) * 256 * XW, 0);
        std::vector<uint64_t> u(XW);
        for (int k = 0; k < nb; ++k)
            for (int v = 0; v < 256; ++v) {
                std::fill(u.begin(), u.end(), 0ULL);
                for (int t = 0; t < 8; ++t) {
                    const int q = 8 * k + t;
                    if (q < K && ((v >> t) & 1)) {
                        const int pos = h->info_set[(size_t)q];
                        u[pos >> 6] |= 1ULL << (pos & 63);
                    }
                }
                for (int w = 0; w < XW; ++w)  // in-word Arikan stages (polar.py:17-29)
                    for (int st = 1; st < 64; st <<= 1) {
                        uint64_t m = 0;
                        for (int b = 0; b < 64; ++b)
                            if (!(b & st)) m |= 1ULL << b;
                        u[w] ^= (u[w] >> st) & m;
                    }
                for (int sw = 1; 64 * sw < N; sw <<= 1)  // stages of 64 bits and more: whole words
                    for (int w = 0; w < XW; ++w)
                        if (!(w & sw) && w + sw < XW) u[w] ^= u[w + sw];
                for (int w = 0; w < XW; ++w) xt[((size_t)k * 256 + v) * XW + w] = u[w];
            }
        std::vector<uint32_t> ct((size_t)(nbp > 0 ? nbp : 1) * 256, 0);
        for (int k = 0; k < nbp; ++k)
            for (int v = 0; v < 256; ++v) {
                uint32_t r = 0;
                for (int t = 0; t < 8; ++t)
                    if (8 * k + t < kp && ((v >> t) & 1)) r ^= h->attach_cols[(size_t)(8 * k + t)];
                ct[(size_t)k * 256 + v] = r;
            }
        CREATE_TRY(hipMalloc(&h->d_xtab, xt.size() * 8));
        CREATE_TRY(hipMemcpy(h->d_xtab, xt.data(), xt.size() * 8, hipMemcpyHostToDevice));
        CREATE_TRY(hipMalloc(&h->d_crctab, ct.size() * 4));
        CREATE_TRY(hipMemcpy(h->d_crctab, ct.data(), ct.size() * 4, hipMemcpyHostToDevice));
    }
#undef CREATE_TRY
    *out = h;
    return PSCL_OK;
}

int pscl_destroy(pscl_handle* h) {
    if (!h) return PSCL_OK;
    hipSetDevice(h->device);
    if (h->dl_defer_valid) dl_enqueue_deferred(h);  // (a pipelined call's chains complete before the buffers go)
    quiesce(h);
    if (h->own_stream) hipStreamSynchronize(h->own_stream);
    for (auto& b : h->scratch)
        if (b.p) hipFree(b.p);
    for (auto e : h->ev_pool) hipEventDestroy(e);
    if (h->d_check_cols) hipFree(h->d_check_cols);
    if (h->d_attach_cols) hipFree(h->d_attach_cols);
    if (h->d_info_set) hipFree(h->d_info_set);
    if (h->d_exp_table) hipFree(h->d_exp_table);
    if (h->d_info_words) hipFree(h->d_info_words);
    if (h->d_rm_src) hipFree(h->d_rm_src);
    if (h->d_rm_order) hipFree(h->d_rm_order);
    if (h->d_beta) hipFree(h->d_beta);
    for (int i = 0; i < 2; ++i)
        if (h->d_beta32g[i]) hipFree(h->d_beta32g[i]);
    if (h->d_epi) hipFree(h->d_epi);
    if (h->d_xtab) hipFree(h->d_xtab);
    if (h->d_crctab) hipFree(h->d_crctab);
    if (h->h_count) hipHostFree(h->h_count);
    if (h->h_adapt) hipHostFree(h->h_adapt);
    if (h->h_label) hipHostFree(h->h_label);
    auto drop = [](hipEvent_t e) {
        if (e) hipEventDestroy(e);
    };
    for (int i = 0; i < kChainStreams; ++i) drop(h->ev_scr[i]), drop(h->ev_def[i]);
    for (int i = 0; i < kDlPar; ++i) drop(h->ev_base[i]), drop(h->ev_retry[i]), drop(h->dl[i].ev);
    for (int i = 0; i < kChainSets; ++i) drop(h->ev_join[i]);
    for (int i = 0; i < 2; ++i) {
        drop(h->ev_pscr[i]), drop(h->ev_tscr[i]), drop(h->ev_adc[i]);
        drop(h->px[i].ev), drop(h->tail[i].ev), drop(h->ad[i].ev);
    }
    drop_side_streams(h);
    if (h->own_stream) hipStreamDestroy(h->own_stream);
    delete h;
    return PSCL_OK;
}

int pscl_set_stream(pscl_handle* h, void* s) {
    if (!h) return fail(PSCL_EINVAL, "NULL handle");
    int rc = join_pipe(h);  // pending re-decodes ordered before the old stream's later work
    if (rc) return rc;
    h->stream = s ? (hipStream_t)s : h->own_stream;
    return PSCL_OK;
}

void* pscl_get_stream(pscl_handle* h) { return h ? (void*)h->stream : nullptr; }

int pscl_sync(pscl_handle* h) {
    if (!h) return fail(PSCL_EINVAL, "NULL handle");
    HIP_TRY(hipSetDevice(h->device));
    int rc = join_pipe(h);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(h->stream));
    return PSCL_OK;
}

int pscl_decode_device(pscl_handle* h, const double* d_llr, int64_t B, const uint64_t* d_force, uint64_t* d_best,
                       uint8_t* d_flags, double* d_metrics, uint64_t* d_cands, double* d_info_llrs,
                       const uint64_t* d_ref, int k_payload, int64_t* d_counters) {
    return decode_device_impl(h, d_llr, false, B, d_force, d_best, d_flags, d_metrics, d_cands, d_info_llrs, d_ref, k_payload,
                              d_counters);
}

int pscl_decode_device_f32(pscl_handle* h, const float* d_llr, int64_t B, uint64_t* d_best, uint8_t* d_flags,
                           const uint64_t* d_ref, int k_payload, int64_t* d_counters) {
    return decode_device_impl(h, d_llr, true, B, nullptr, d_best, d_flags, nullptr, nullptr, nullptr, d_ref, k_payload,
                              d_counters);
}

int pscl_f32_available(pscl_handle* h) { return h && !f32_unsupported(h) ? 1 : 0; }

// Adaptive decode (include/polar_scl.h): stage 1 is the lane-parallel SC kernel over all B frames
// (launch_sc_stage), stage 2 the hand-off of the frames that fail the CRC (escalate_failed).
int pscl_adaptive_device(pscl_handle* h, const double* d_llr, int64_t B, uint64_t* d_best, uint8_t* d_flags,
                         uint8_t* d_stage, const uint64_t* d_ref, int k_payload, int64_t* d_counters,
                         int64_t* n_escalated) {
    if (!h) return fail(PSCL_EINVAL, "NULL handle");
    if (n_escalated) *n_escalated = 0;
    if (B < 0) return fail(PSCL_EINVAL, "B must be >= 0");
    if (!h->crc_poly) return fail(PSCL_EINVAL, "adaptive decoding needs a CRC (without one every SC result passes)");
    if (d_ref && !d_counters) return fail(PSCL_EINVAL, "d_ref given without d_counters");
    if (k_payload < 0 || k_payload > h->K) return fail(PSCL_EINVAL, "k_payload out of range");
    if (h->N != PSCL_FAST_N)
        return fail(PSCL_EUNSUP, "adaptive decoding is implemented for N = %d only (N = %d)", PSCL_FAST_N, h->N);
    if (B == 0) return PSCL_OK;
    if (!d_llr || !d_best || !d_flags) return fail(PSCL_EINVAL, "d_llr, d_best and d_flags are required");
    if (B > INT32_MAX) return fail(PSCL_EUNSUP, "B exceeds 2^31-1");
    int rc = enter(h);  // (pending pipelined work first; the call runs stream-ordered)
    if (rc) return rc;
    if ((rc = launch_sc_stage(h, d_llr, B, d_best, d_flags, d_stage))) return rc;
    int64_t n = 0;
    if ((rc = escalate_failed(h, d_llr, B, d_best, d_flags, nullptr, &n))) return rc;  // (stage 1 wrote the stages)
    if (n_escalated) *n_escalated = n;
    return count_final(h, d_best, d_flags, B, d_ref, k_payload, d_counters, n);
}

int pscl_sc_device(pscl_handle* h, const double* d_llr, int64_t B, uint64_t* d_best, uint8_t* d_flags,
                   uint8_t* d_stage, const uint64_t* d_ref, int k_payload, int64_t* d_counters) {
    return sc_device_impl(h, d_llr, false, B, d_best, d_flags, d_stage, d_ref, k_payload, d_counters);
}

int pscl_sc_device_f32(pscl_handle* h, const float* d_llr, int64_t B, uint64_t* d_best, uint8_t* d_flags,
                       uint8_t* d_stage, const uint64_t* d_ref, int k_payload, int64_t* d_counters) {
    return sc_device_impl(h, (const double*)d_llr, true, B, d_best, d_flags, d_stage, d_ref, k_payload, d_counters);
}

int pscl_escalate_device(pscl_handle* h, const double* d_llr, int64_t B, uint64_t* d_best, uint8_t* d_flags,
                         uint8_t* d_stage, const uint64_t* d_ref, int k_payload, int64_t* d_counters,
                         int64_t* n_escalated) {
    return escalate_device_impl(h, d_llr, false, B, d_best, d_flags, d_stage, d_ref, k_payload, d_counters, n_escalated);
}

int pscl_escalate_device_f32(pscl_handle* h, const float* d_llr, int64_t B, uint64_t* d_best, uint8_t* d_flags,
                             uint8_t* d_stage, const uint64_t* d_ref, int k_payload, int64_t* d_counters,
                             int64_t* n_escalated) {
    return escalate_device_impl(h, (const double*)d_llr, true, B, d_best, d_flags, d_stage, d_ref, k_payload, d_counters,
                                n_escalated);
}

int pscl_adaptive_async_device(pscl_handle* h, const double* d_llr, int64_t B, uint64_t* d_best, uint8_t* d_flags,
                               uint8_t* d_stage, const uint64_t* d_ref, int k_payload, int64_t* d_counters,
                               int32_t* d_n_escalated) {
    return adaptive_async_impl(h, d_llr, false, B, d_best, d_flags, d_stage, d_ref, k_payload, d_counters, d_n_escalated);
}

int pscl_adaptive_async_device_f32(pscl_handle* h, const float* d_llr, int64_t B, uint64_t* d_best, uint8_t* d_flags,
                                   uint8_t* d_stage, const uint64_t* d_ref, int k_payload, int64_t* d_counters,
                                   int32_t* d_n_escalated) {
    return adaptive_async_impl(h, (const double*)d_llr, true, B, d_best, d_flags, d_stage, d_ref, k_payload, d_counters,
                               d_n_escalated);
}

int pscl_adaptive_stats(pscl_handle* h, int64_t* screened, int64_t* exact, int64_t* host_waits, int reset) {
    if (!h) return fail(PSCL_EINVAL, "NULL handle");
    if (screened) *screened = h->n_ad_screened;
    if (exact) *exact = h->n_ad_exact;
    if (host_waits) *host_waits = h->n_ad_waits;
    if (reset) h->n_ad_screened = h->n_ad_exact = h->n_ad_waits = 0;
    return PSCL_OK;
}

int pscl_join(pscl_handle* h) {
    if (!h) return fail(PSCL_EINVAL, "NULL handle");
    int rc = set_device(h);
    if (rc) return rc;
    return join_pipe(h);
}

int pscl_set_pipelined(pscl_handle* h, int enable) {
    if (!h) return fail(PSCL_EINVAL, "NULL handle");
    int rc = set_device(h);
    if (rc) return rc;
    if ((rc = join_pipe(h))) return rc;
    if (enable < 0 || enable > kDlPar) return fail(PSCL_EINVAL, "pipelined depth %d out of range 0..%d", enable, kDlPar);
    if (h->pipelined != (enable != 0)) {
        // the other mode's streams in, this mode's to the stash (drained first)
        quiesce(h);
        std::swap(h->pipe_stream, h->stash_pipe);
        for (int i = 0; i < kChainStreams; ++i) {
            std::swap(h->retry_stream[i], h->stash_retry[i]);
            std::swap(h->side_stream[i], h->stash_side[i]);
        }
    }
    h->pipelined = enable != 0;
    // DL-SCL calls: a call's buffers are free again at the depth-th following call (1 and 2: the
    // second, the documented default); its chains run up to depth - 1 calls behind the baselines
    h->dl_back = enable >= 2 ? enable : 2;
    return PSCL_OK;
}

int pscl_set_tuning(pscl_handle* h, int knob, int64_t value) {
    if (!h) return fail(PSCL_EINVAL, "NULL handle");
    static const int64_t lim[PSCL_TUNE_COUNT][2] = {{0, 0}, {0, 2}, {0, 64}, {0, 2}, {0, 1}, {0, 4096}, {0, PSCL_MAX_WAVES_PER_WG}, {0, 2},
                                                    {0, (int64_t)1 << 30}, {0, 2}, {0, 32}, {0, 3}, {0, 2}, {0, 2}, {0, 4}, {0, 3}, {0, 2}, {0, 1},
                                                    {0, (int64_t)1 << 20}, {0, 1}};
    if (knob < 1 || knob >= PSCL_TUNE_COUNT) return fail(PSCL_EINVAL, "unknown tuning knob %d", knob);
    if (value < lim[knob][0] || value > lim[knob][1] || (knob == PSCL_TUNE_POST_GRID && value && value < 16))
        return fail(PSCL_EINVAL, "tuning knob %d: value %lld out of range", knob, (long long)value);
    if (knob == PSCL_TUNE_POST_EPW && value != 0 && value != 2 && value != 4)
        return fail(PSCL_EINVAL, "tuning knob %d: value %lld out of range", knob, (long long)value);
    int rc = set_device(h);
    if (rc) return rc;
    if ((rc = join_pipe(h))) return rc;  // (pending work ran under the old schedule)
    if (knob == PSCL_TUNE_SIDE_PRIORITY && h->tune[knob] != value) drop_side_streams(h);
    h->tune[knob] = value;
    return PSCL_OK;
}

int pscl_path_llrs_device(pscl_handle* h, const double* d_llr, int64_t B, const uint64_t* d_bits, double* d_out) {
    return path_llrs_impl(h, d_llr, false, B, d_bits, d_out);
}

int pscl_path_llrs_device_f32(pscl_handle* h, const float* d_llr, int64_t B, const uint64_t* d_bits, double* d_out) {
    return path_llrs_impl(h, d_llr, true, B, d_bits, d_out);
}

// Flip labels of a device batch (include/polar_scl.h): the baseline decode and the compaction of the
// frames that fail the CRC, the call's one host wait for their count A, then -- all enqueued on the
// handle's stream -- the replay of the baseline best paths (L0 by entry), the ranking (label.hip), and
// T rounds of {forced-bit decode of the round's dense list, step}.  A round's decode reads its live
// count on the device (d_count), its LLR rows by indirection (fidx) and one force block per frame, the
// form the long codes' DL-SCL chain drives (dl_retry_long); every code length takes it, and every
// round decodes from phase 0 on the exact forced-bit instance.
int pscl_label_device(pscl_handle* h, const double* d_llr, int64_t B, const uint64_t* d_sent, int64_t sent_stride,
                      int max_flips, int64_t cap, int64_t* d_frame, float* d_abs_l0, int32_t* d_flip, int32_t* d_rank,
                      int64_t* d_counts, int64_t* n_entries) {
    if (!h) return fail(PSCL_EINVAL, "NULL handle");
    if (n_entries) *n_entries = 0;
    if (!h->crc_poly) return fail(PSCL_EINVAL, "labelling needs a CRC (without one every baseline passes)");
    if (max_flips < 1 || max_flips > 32) return fail(PSCL_EINVAL, "max_flips must be 1..32 (got %d)", max_flips);
    if (B < 0) return fail(PSCL_EINVAL, "B must be >= 0");
    if (cap < 0) return fail(PSCL_EINVAL, "cap must be >= 0");
    if (sent_stride != 0 && sent_stride != h->W)
        return fail(PSCL_EINVAL, "sent_stride must be 0 (one message) or W = %d (one per frame)", h->W);
    if (B > 0 && (!d_llr || !d_sent || !d_counts || !n_entries))
        return fail(PSCL_EINVAL, "d_llr, d_sent, d_counts and n_entries are required");
    if (B > 0 && cap > 0 && (!d_frame || !d_abs_l0 || !d_flip))
        return fail(PSCL_EINVAL, "d_frame, d_abs_l0 and d_flip are required");
    if (B > INT32_MAX) return fail(PSCL_EUNSUP, "B exceeds 2^31-1");
    int rc = enter(h);  // (pending pipelined work first; the call runs stream-ordered)
    if (rc) return rc;
    hipStream_t s = h->stream;
    if (B == 0) {
        if (d_counts) HIP_TRY(hipMemsetAsync(d_counts, 0, PSCL_NLABEL * 8, s));
        return PSCL_OK;
    }
    const int K = h->K, W = h->W, T = max_flips < K ? max_flips : K;
    // the baseline: the handle's plain list decode of all B frames into scratch
    uint64_t* d_base;
    uint8_t* d_bflags;
    int32_t* d_cnt;
    int64_t* d_act;
    if ((rc = ensure_as(h, kLblBest, (size_t)B * W * 8, d_base)) || (rc = ensure_as(h, kLblFlags, (size_t)B, d_bflags)) ||
        (rc = ensure_as(h, kLblCount, 4, d_cnt)) || (rc = ensure_as(h, kLblAct, (size_t)B * 8, d_act)))
        return rc;
    if (!h->h_label) HIP_TRY(hipHostMalloc((void**)&h->h_label, 4, hipHostMallocDefault));
    pscl_decode_params P;
    fill_decode_params(h, P, 0);
    P.llr = d_llr;
    P.B = B;
    P.best = d_base;
    P.flags = d_bflags;
    if (pscl_decode_wpg(P) < 1) return fail(PSCL_EUNSUP, "LDS budget exceeded (L=%d, K=%d)", h->L, h->K);
    if ((rc = launch_decode(h, P, 0))) return rc;
    HIP_TRY(hipMemsetAsync(d_cnt, 0, 4, s));
    LAUNCH_TRY("dl_compact", pscl_launch_dl_compact(d_bflags, B, 0, d_act, nullptr, d_cnt, s));
    HIP_TRY(hipMemcpyAsync(h->h_label, d_cnt, 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));  // the call's one host wait
    const int64_t A = *h->h_label;
    if (A < 0 || A > B) return fail(PSCL_EDEVICE, "entry count %lld out of range", (long long)A);
    *n_entries = A;
    if (A > cap)
        return fail(PSCL_EINVAL, "%lld entries exceed cap = %lld: allocate again and repeat", (long long)A, (long long)cap);
    HIP_TRY(hipMemsetAsync(d_counts, 0, PSCL_NLABEL * 8, s));
    if (A == 0) return PSCL_OK;  // (every frame passed: no round is launched)
    double* d_l0;
    int32_t *d_order, *d_ent[2], *d_rcnt;
    int64_t* d_row[2];
    uint64_t *d_force, *d_ob;
    uint8_t* d_of;
    const size_t a = (size_t)A;
    if ((rc = ensure_as(h, kLblL0, a * K * 8, d_l0)) || (rc = ensure_as(h, kLblOrder, a * T * 4, d_order)) ||
        (rc = ensure_as(h, kLblEnt0, a * 4, d_ent[0])) || (rc = ensure_as(h, kLblEnt1, a * 4, d_ent[1])) ||
        (rc = ensure_as(h, kLblRow0, a * 8, d_row[0])) || (rc = ensure_as(h, kLblRow1, a * 8, d_row[1])) ||
        (rc = ensure_as(h, kLblForce, a * 2 * W * 8, d_force)) || (rc = ensure_as(h, kLblOb, a * W * 8, d_ob)) ||
        (rc = ensure_as(h, kLblOf, a, d_of)) || (rc = ensure_as(h, kLblCnt, (size_t)(T + 1) * 4, d_rcnt)))
        return rc;
    // L0 of the baseline best paths, by entry (pscl_path_llrs_device's kernels over the entry list)
    pscl_replay_params Rp;
    memset(&Rp, 0, sizeof(Rp));
    Rp.llr = d_llr;
    Rp.N = h->N;
    Rp.n = h->n;
    Rp.K = K;
    Rp.W = W;
    Rp.rm_E = h->rm_E;
    Rp.rm_src = h->d_rm_src;
    Rp.info_mask[0] = h->info_mask[0];
    Rp.info_mask[1] = h->info_mask[1];
    Rp.count = d_cnt;
    Rp.act = d_act;
    Rp.bits = d_base;
    Rp.bits_by_row = 1;
    Rp.out = d_l0;
    const bool lng = h->N > PSCL_FAST_N;
    if (lng) {
        h->n_replay_launches++;
        h->n_replay_rows += A;
    }
    LAUNCH_TRY("replay", lng ? pscl_launch_replay_long(Rp, A, h->d_info_words, nullptr, s) : pscl_launch_replay(Rp, A, s));
    pscl_label_rank_params R;
    memset(&R, 0, sizeof(R));
    R.l0 = d_l0;
    R.A = A;
    R.K = K;
    R.T = T;
    R.abs_l0 = d_abs_l0;
    R.order = d_order;
    LAUNCH_TRY("label_rank", pscl_launch_label_rank(R, s));
    HIP_TRY(hipMemsetAsync(d_rcnt, 0, (size_t)(T + 1) * 4, s));
    pscl_label_step_params S;
    memset(&S, 0, sizeof(S));
    S.K = K;
    S.W = W;
    S.T = T;
    S.A = A;
    S.ob = d_ob;
    S.of = d_of;
    S.act = d_act;
    S.base = d_base;
    S.sent = d_sent;
    S.sent_stride = sent_stride;
    S.order = d_order;
    S.force_out = d_force;
    S.frame = d_frame;
    S.flip = d_flip;
    S.rank = d_rank;
    S.counts = d_counts;
    S.t = -1;  // the first launch builds round 0
    S.out_count = d_rcnt;
    S.ent_out = d_ent[0];
    S.row_out = d_row[0];
    LAUNCH_TRY("label_step", pscl_launch_label_step(S, s));
    pscl_decode_params H;
    fill_decode_params(h, H, 0);
    H.llr = d_llr;
    H.B = A;
    H.force = d_force;
    H.best = d_ob;
    H.flags = d_of;
    if (pscl_decode_wpg(H) < 1) return fail(PSCL_EUNSUP, "LDS budget exceeded (L=%d, K=%d)", h->L, h->K);
    for (int t = 0; t < T; ++t) {  // no host round trips: the live counts stay on the device
        H.fidx = d_row[t & 1];
        H.d_count = d_rcnt + t;
        if ((rc = launch_decode(h, H, 0))) return rc;
        S.t = t;
        S.in_count = d_rcnt + t;
        S.ent_in = d_ent[t & 1];
        S.out_count = t + 1 < T ? d_rcnt + t + 1 : nullptr;
        S.ent_out = d_ent[(t + 1) & 1];
        S.row_out = d_row[(t + 1) & 1];
        LAUNCH_TRY("label_step", pscl_launch_label_step(S, s));
    }
    return PSCL_OK;
}

int pscl_set_beta(pscl_handle* h, const double* beta) {
    if (!h) return fail(PSCL_EINVAL, "NULL handle");
    int rc = enter(h);
    if (rc) return rc;
    if (!beta) {
        if (h->d_beta) HIP_TRY(hipFree(h->d_beta));
        h->d_beta = nullptr;
        for (int i = 0; i < 2; ++i) {
            if (h->d_beta32g[i]) HIP_TRY(hipFree(h->d_beta32g[i]));
            h->d_beta32g[i] = nullptr;
        }
        return PSCL_OK;
    }
    if (h->K == 0) return fail(PSCL_EINVAL, "beta must be a square matrix matching abs_l0 length");
    const size_t n = (size_t)h->K * h->K;
    if (!h->d_beta) HIP_TRY(hipMalloc(&h->d_beta, n * 8));
    // stream-ordered upload: enter() made the handle's stream wait for every pending pipelined
    // round (which may still read the old matrix), so the copy lands after them and before any
    // later launch; the host staging buffer is rewritten only once the previous upload is done
    HIP_TRY(hipStreamSynchronize(h->stream));
    h->beta_host.assign(beta, beta + n);
    HIP_TRY(hipMemcpyAsync(h->d_beta, h->beta_host.data(), n * 8, hipMemcpyHostToDevice, h->stream));
    if (h->K == 64) {  // the fused post pass's layouts: lane p's candidates p + G i contiguous per row k
        const int K = h->K;
        h->beta32g_host.assign(2 * n, 0.0f);
        for (int gi = 0; gi < 2; ++gi) {
            const int G = gi ? 4 : 8, NC = K / G;
            for (int k = 0; k < K; ++k)
                for (int pp = 0; pp < G; ++pp)
                    for (int i = 0; i < NC; ++i)
                        h->beta32g_host[(size_t)gi * n + ((size_t)k * G + pp) * NC + i] = (float)beta[(size_t)k * K + pp + G * i];
            if (!h->d_beta32g[gi]) HIP_TRY(hipMalloc(&h->d_beta32g[gi], n * 4));
            HIP_TRY(hipMemcpyAsync(h->d_beta32g[gi], h->beta32g_host.data() + (size_t)gi * n, n * 4, hipMemcpyHostToDevice,
                                   h->stream));
        }
    }
    double mx = 0.0;
    bool nan = false;
    for (size_t i = 0; i < n; ++i) {
        const double a = fabs(beta[i]);
        if (std::isnan(a))
            nan = true;
        else if (a > mx)
            mx = a;
    }
    h->beta_absmax = nan ? INFINITY : mx;  // (a NaN entry: every certificate fails, exact sums)
    return PSCL_OK;
}

int pscl_dlscl_device(pscl_handle* h, const double* d_llr, int64_t B, int retries, uint64_t* d_best, uint8_t* d_flags,
                      int32_t* d_attempts, int32_t* d_tried, int tried_stride, const uint64_t* d_ref, int k_payload,
                      int64_t* d_counters_scl, int64_t* d_counters_dl) {
    return dlscl_impl(h, d_llr, B, retries, d_best, d_flags, d_attempts, d_tried, tried_stride, d_ref, k_payload,
                      d_counters_scl, d_counters_dl, nullptr);
}

int pscl_dlscl_device_f32(pscl_handle* h, const float* d_llr, int64_t B, int retries, uint64_t* d_best, uint8_t* d_flags,
                          int32_t* d_attempts, int32_t* d_tried, int tried_stride, const uint64_t* d_ref, int k_payload,
                          int64_t* d_counters_scl, int64_t* d_counters_dl) {
    DlBase base;
    base.row_f32 = true;
    return dlscl_impl(h, (const double*)d_llr, B, retries, d_best, d_flags, d_attempts, d_tried, tried_stride, d_ref,
                      k_payload, d_counters_scl, d_counters_dl, nullptr, base);
}

// Retry rounds on the caller's baseline (include/polar_scl.h): dlscl_impl with the baseline skipped.

int pscl_retry_device(pscl_handle* h, const double* d_llr, int64_t B, int retries, uint64_t* d_best, uint8_t* d_flags,
                      uint8_t* d_stage, int32_t* d_attempts, int32_t* d_tried, int tried_stride, const uint64_t* d_ref,
                      int k_payload, int64_t* d_counters_dl) {
    if (const int rc = retry_args(h, d_ref, d_counters_dl)) return rc;
    DlBase base;
    base.mode = 2;
    base.d_stage = d_stage;
    return dlscl_impl(h, d_llr, B, retries, d_best, d_flags, d_attempts, d_tried, tried_stride, d_ref, k_payload, nullptr,
                      d_counters_dl, nullptr, base);
}

int pscl_retry_device_f32(pscl_handle* h, const float* d_llr, int64_t B, int retries, uint64_t* d_best, uint8_t* d_flags,
                          uint8_t* d_stage, int32_t* d_attempts, int32_t* d_tried, int tried_stride, const uint64_t* d_ref,
                          int k_payload, int64_t* d_counters_dl) {
    if (const int rc = retry_args(h, d_ref, d_counters_dl)) return rc;
    DlBase base;
    base.mode = 2;
    base.d_stage = d_stage;
    base.row_f32 = true;
    return dlscl_impl(h, (const double*)d_llr, B, retries, d_best, d_flags, d_attempts, d_tried, tried_stride, d_ref, k_payload,
                      nullptr, d_counters_dl, nullptr, base);
}

// The three-stage decode (include/polar_scl.h): dlscl_impl on the adaptive baseline.

int pscl_adaptive_dlscl_device(pscl_handle* h, const double* d_llr, int64_t B, int retries, uint64_t* d_best,
                               uint8_t* d_flags, uint8_t* d_stage, int32_t* d_attempts, int32_t* d_tried,
                               int tried_stride, const uint64_t* d_ref, int k_payload, int64_t* d_counters,
                               int32_t* d_n_escalated) {
    bool done;
    const int rc = adaptive_dlscl_args(h, B, d_ref, k_payload, d_counters, d_n_escalated, &done);
    if (rc || done) return rc;
    DlBase base;
    base.mode = 1;
    base.d_stage = d_stage;
    base.d_counters_sc = d_counters;
    base.d_n_escalated = d_n_escalated;
    return dlscl_impl(h, d_llr, B, retries, d_best, d_flags, d_attempts, d_tried, tried_stride, d_ref, k_payload,
                      d_counters ? d_counters + PSCL_NCOUNT : nullptr, d_counters ? d_counters + 2 * PSCL_NCOUNT : nullptr,
                      nullptr, base);
}

int pscl_adaptive_dlscl_device_f32(pscl_handle* h, const float* d_llr, int64_t B, int retries, uint64_t* d_best,
                                   uint8_t* d_flags, uint8_t* d_stage, int32_t* d_attempts, int32_t* d_tried,
                                   int tried_stride, const uint64_t* d_ref, int k_payload, int64_t* d_counters,
                                   int32_t* d_n_escalated) {
    bool done;
    const int rc = adaptive_dlscl_args(h, B, d_ref, k_payload, d_counters, d_n_escalated, &done);
    if (rc || done) return rc;
    DlBase base;
    base.mode = 1;
    base.d_stage = d_stage;
    base.d_counters_sc = d_counters;
    base.d_n_escalated = d_n_escalated;
    base.row_f32 = true;
    return dlscl_impl(h, (const double*)d_llr, B, retries, d_best, d_flags, d_attempts, d_tried, tried_stride, d_ref,
                      k_payload, d_counters ? d_counters + PSCL_NCOUNT : nullptr,
                      d_counters ? d_counters + 2 * PSCL_NCOUNT : nullptr, nullptr, base);
}

int pscl_decode(pscl_handle* h, const double* llr, int64_t B, const int8_t* forced, int32_t* n_paths,
                int8_t* best_bits, uint8_t* crc_pass, int32_t* best_idx, double* metrics, int8_t* cands,
                double* info_llrs) {
    return decode_host(h, llr, B, forced, n_paths, best_bits, crc_pass, best_idx, metrics, cands, info_llrs, 0);
}

int pscl_sc_decode(pscl_handle* h, const double* llr, int64_t B, int8_t* bits) {
    if (!h) return fail(PSCL_EINVAL, "NULL handle");
    if (B <= 0) return B < 0 ? fail(PSCL_EINVAL, "B must be >= 0") : PSCL_OK;
    std::vector<int32_t> np((size_t)B);
    return decode_host(h, llr, B, nullptr, np.data(), bits, nullptr, nullptr, nullptr, nullptr, nullptr, 1);
}

int pscl_uncoded_device(pscl_handle* h, uint64_t seed, uint32_t stream_id, double ebno_db, int k_payload,
                        int64_t frame0, int64_t B, int64_t* d_counters) {
    return uncoded_launch(h, seed, stream_id, ebno_db, k_payload, frame0, B, d_counters, false);
}

int pscl_simulate_device(pscl_handle* h, uint64_t seed, uint32_t stream_id, double ebno_db, double rate, int k_payload,
                         int64_t frame0, int64_t B, int retries, int include_uncoded, int64_t* d_counters) {
    if (!h) return fail(PSCL_EINVAL, "NULL handle");
    if (!d_counters) return fail(PSCL_EINVAL, "d_counters is NULL");
    if (B < 0 || frame0 < 0) return fail(PSCL_EINVAL, "B and frame0 must be >= 0");
    if (B == 0) return PSCL_OK;
    int rc = set_device(h);
    if (rc) return rc;
    if ((rc = join_pipe(h, 1))) return rc;  // (plain decodes' pending re-decodes; DL chains keep overlapping)
    return simulate_enqueue(h, seed, stream_id, ebno_db, rate, k_payload, frame0, B, retries, include_uncoded, d_counters);
}

int pscl_simulate(pscl_handle* h, uint64_t seed, uint32_t stream_id, double ebno_db, double rate, int k_payload,
                  int64_t frame0, int64_t B, int retries, int include_uncoded, int64_t* counters) {
    if (!h) return fail(PSCL_EINVAL, "NULL handle");
    if (!counters) return fail(PSCL_EINVAL, "counters is NULL");
    if (B < 0 || frame0 < 0) return fail(PSCL_EINVAL, "B and frame0 must be >= 0");
    memset(counters, 0, sizeof(int64_t) * 3 * PSCL_NCOUNT);
    if (B == 0) return PSCL_OK;
    int rc = enter(h);
    if (rc) return rc;
    void* d_cnt;
    if ((rc = ensure(h, kSimCounters, sizeof(int64_t) * 3 * PSCL_NCOUNT, &d_cnt))) return rc;
    HIP_TRY(hipMemsetAsync(d_cnt, 0, sizeof(int64_t) * 3 * PSCL_NCOUNT, h->stream));
    if ((rc = simulate_enqueue(h, seed, stream_id, ebno_db, rate, k_payload, frame0, B, retries, include_uncoded,
                               (int64_t*)d_cnt)))
        return rc;
    if ((rc = join_pipe(h))) return rc;  // (a pipelined handle: this call's chains, then the counters)
    HIP_TRY(hipMemcpyAsync(counters, d_cnt, sizeof(int64_t) * 3 * PSCL_NCOUNT, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return PSCL_OK;
}

int pscl_simulate_adaptive_dl_device(pscl_handle* h, uint64_t seed, uint32_t stream_id, double ebno_db, double rate,
                                     int k_payload, int64_t frame0, int64_t B, int retries, int include_uncoded,
                                     int64_t* d_counters) {
    int rc = adaptive_async_args(h, B < 0 ? B : 0, k_payload);  // (any B: the chunks are at most 2^20 frames)
    if (rc) return rc;
    if (!d_counters) return fail(PSCL_EINVAL, "d_counters is NULL");
    if (frame0 < 0) return fail(PSCL_EINVAL, "B and frame0 must be >= 0");
    if (B == 0) return PSCL_OK;
    if ((rc = set_device(h)) || (rc = join_pipe(h, 1))) return rc;  // (DL chains keep overlapping, pscl_simulate_device)
    return simulate_enqueue(h, seed, stream_id, ebno_db, rate, k_payload, frame0, B, retries, include_uncoded, d_counters,
                            true);
}

int pscl_simulate_adaptive_dl(pscl_handle* h, uint64_t seed, uint32_t stream_id, double ebno_db, double rate,
                              int k_payload, int64_t frame0, int64_t B, int retries, int include_uncoded,
                              int64_t* counters) {
    int rc = adaptive_async_args(h, B < 0 ? B : 0, k_payload);
    if (rc) return rc;
    if (!counters) return fail(PSCL_EINVAL, "counters is NULL");
    if (frame0 < 0) return fail(PSCL_EINVAL, "B and frame0 must be >= 0");
    memset(counters, 0, sizeof(int64_t) * 4 * PSCL_NCOUNT);
    if (B == 0) return PSCL_OK;
    if ((rc = enter(h))) return rc;
    void* d_cnt;
    if ((rc = ensure(h, kSimAdDlCounters, sizeof(int64_t) * 4 * PSCL_NCOUNT, &d_cnt))) return rc;
    HIP_TRY(hipMemsetAsync(d_cnt, 0, sizeof(int64_t) * 4 * PSCL_NCOUNT, h->stream));
    if ((rc = simulate_enqueue(h, seed, stream_id, ebno_db, rate, k_payload, frame0, B, retries, include_uncoded,
                               (int64_t*)d_cnt, true)))
        return rc;
    if ((rc = join_pipe(h))) return rc;  // (a pipelined handle: this call's chains, then the counters)
    HIP_TRY(hipMemcpyAsync(counters, d_cnt, sizeof(int64_t) * 4 * PSCL_NCOUNT, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return PSCL_OK;
}

int pscl_simulate_adaptive_device(pscl_handle* h, uint64_t seed, uint32_t stream_id, double ebno_db, double rate,
                                  int k_payload, int64_t frame0, int64_t B, int include_uncoded, int64_t* d_counters) {
    int rc = adaptive_async_args(h, B < 0 ? B : 0, k_payload);  // (any B: the chunks are at most 2^20 frames)
    if (rc) return rc;
    if (!d_counters) return fail(PSCL_EINVAL, "d_counters is NULL");
    if (frame0 < 0) return fail(PSCL_EINVAL, "B and frame0 must be >= 0");
    if (B == 0) return PSCL_OK;
    if ((rc = enter(h))) return rc;
    return simulate_adaptive_enqueue(h, seed, stream_id, ebno_db, rate, k_payload, frame0, B, include_uncoded, d_counters);
}

int pscl_simulate_adaptive(pscl_handle* h, uint64_t seed, uint32_t stream_id, double ebno_db, double rate,
                           int k_payload, int64_t frame0, int64_t B, int include_uncoded, int64_t* counters) {
    int rc = adaptive_async_args(h, B < 0 ? B : 0, k_payload);
    if (rc) return rc;
    if (!counters) return fail(PSCL_EINVAL, "counters is NULL");
    if (frame0 < 0) return fail(PSCL_EINVAL, "B and frame0 must be >= 0");
    memset(counters, 0, sizeof(int64_t) * 3 * PSCL_NCOUNT);
    if (B == 0) return PSCL_OK;
    if ((rc = enter(h))) return rc;
    void* d_cnt;
    if ((rc = ensure(h, kSimAdCounters, sizeof(int64_t) * 3 * PSCL_NCOUNT, &d_cnt))) return rc;
    HIP_TRY(hipMemsetAsync(d_cnt, 0, sizeof(int64_t) * 3 * PSCL_NCOUNT, h->stream));
    if ((rc = simulate_adaptive_enqueue(h, seed, stream_id, ebno_db, rate, k_payload, frame0, B, include_uncoded,
                                        (int64_t*)d_cnt)))
        return rc;
    HIP_TRY(hipMemcpyAsync(counters, d_cnt, sizeof(int64_t) * 3 * PSCL_NCOUNT, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));  // the host form's one wait, at the end
    return PSCL_OK;
}

int pscl_channel_device(pscl_handle* h, uint64_t seed, uint32_t stream_id, double ebno_db, double rate, int k_payload,
                        int64_t frame0, int64_t B, double* d_llr, uint64_t* d_msg) {
    return channel_launch(h, seed, stream_id, ebno_db, rate, k_payload, frame0, B, d_llr, d_msg, nullptr);
}

int pscl_encode_device(pscl_handle* h, const uint64_t* d_payload, int64_t B, uint64_t* d_msg, uint64_t* d_code,
                       void* d_sym, int sym_f32) {
    return encode_launch(h, d_payload, 0, B, d_msg, d_code, d_sym, PSCL_ROWS_SYMBOLS, sym_f32, 0, 0, 0.0, 1.0);
}

int pscl_channel_payload_device(pscl_handle* h, const uint64_t* d_payload, uint64_t seed, uint32_t stream_id,
                                double ebno_db, double rate, int64_t frame0, int64_t B, void* d_llr, int llr_f32,
                                uint64_t* d_msg) {
    return encode_launch(h, d_payload, frame0, B, d_msg, nullptr, d_llr, PSCL_ROWS_LLR, llr_f32, seed, stream_id, ebno_db,
                         rate);
}

int pscl_set_rate_match(pscl_handle* h, int E) {
    if (!h) return fail(PSCL_EINVAL, "NULL handle");
    if (E < 0) return fail(PSCL_EINVAL, "E must be >= 0");
    if (E > 0 && E > h->N && h->N < 32)
        return fail(PSCL_EUNSUP, "repetition (E > N) needs N >= 32 (sub-block interleaver without padding)");
    if (E == h->rm_E) return PSCL_OK;
    // (the interleaver tables depend on N only: uploaded by pscl_create; enqueued launches carry
    // rm_E in their parameter block.  A pipelined DL-SCL call's retry chains are not enqueued yet --
    // they are built from the handle at the next call or join -- so they are enqueued here first,
    // with the rate matching their call's LLR rows were written for)
    const int rc = enter(h);
    if (rc) return rc;
    h->rm_E = E;
    return PSCL_OK;
}

int pscl_derate_match_device(pscl_handle* h, const double* d_llr, int64_t B, double* d_out) {
    if (!h) return fail(PSCL_EINVAL, "NULL handle");
    if (B < 0) return fail(PSCL_EINVAL, "B must be >= 0");
    if (!h->rm_E) return fail(PSCL_EINVAL, "the handle has no rate matching (pscl_set_rate_match)");
    if (B > 0 && (!d_llr || !d_out)) return fail(PSCL_EINVAL, "d_llr and d_out are required");
    if (B > PSCL_DERATE_MAX_B) return fail(PSCL_EUNSUP, "B exceeds the %lld rows of one launch", PSCL_DERATE_MAX_B);
    if (B == 0) return PSCL_OK;
    const int rc = enter(h);
    if (rc) return rc;
    return launch_derate(h, d_llr, B, d_out, kRmRows, h->stream, false, nullptr);  // (d_out given: no scratch is touched)
}

int pscl_set_rate_match_staged(pscl_handle* h, int enable) {
    if (!h) return fail(PSCL_EINVAL, "NULL handle");
    if ((enable != 0) == h->rm_staged) return PSCL_OK;
    const int rc = enter(h);  // (pending pipelined work first, as pscl_set_rate_match)
    if (rc) return rc;
    h->rm_staged = enable != 0;
    return PSCL_OK;
}

int pscl_rm_staged_stats(pscl_handle* h, int64_t* passes, int64_t* rows, int reset) {
    if (!h) return fail(PSCL_EINVAL, "NULL handle");
    if (passes) *passes = h->n_rm_passes;
    if (rows) *rows = h->n_rm_rows;
    if (reset) h->n_rm_passes = h->n_rm_rows = 0;
    return PSCL_OK;
}

int pscl_replay_stats(pscl_handle* h, int64_t* launches, int64_t* rows, int reset) {
    if (!h) return fail(PSCL_EINVAL, "NULL handle");
    if (launches) *launches = h->n_replay_launches;
    if (rows) *rows = h->n_replay_rows;
    if (reset) h->n_replay_launches = h->n_replay_rows = 0;
    return PSCL_OK;
}

int pscl_device_alloc(pscl_handle* h, void** d_ptr, int64_t bytes) {
    if (!h || !d_ptr || bytes < 0) return fail(PSCL_EINVAL, "bad arguments");
    int rc = enter(h);
    if (rc) return rc;
    HIP_TRY(hipMalloc(d_ptr, (size_t)(bytes > 0 ? bytes : 1)));
    return PSCL_OK;
}

int pscl_device_free(pscl_handle* h, void* d_ptr) {
    if (!h) return fail(PSCL_EINVAL, "NULL handle");
    // pending pipelined work may still read or write the buffer (a deferred DL-SCL call's chains
    // hold its LLR, output, reference and counter pointers): enqueue it, then drain every stream
    int rc = enter(h);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(h->stream));
    quiesce(h);
    if (d_ptr) HIP_TRY(hipFree(d_ptr));
    return PSCL_OK;
}

int pscl_memcpy_htod(pscl_handle* h, void* d_dst, const void* src, int64_t bytes) {
    if (!h) return fail(PSCL_EINVAL, "NULL handle");
    int rc = enter(h);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(d_dst, src, (size_t)bytes, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return PSCL_OK;
}

int pscl_memcpy_dtoh(pscl_handle* h, void* dst, const void* d_src, int64_t bytes) {
    if (!h) return fail(PSCL_EINVAL, "NULL handle");
    int rc = enter(h);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(dst, d_src, (size_t)bytes, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return PSCL_OK;
}

int pscl_memset_device(pscl_handle* h, void* d_dst, int value, int64_t bytes) {
    if (!h) return fail(PSCL_EINVAL, "NULL handle");
    int rc = enter(h);
    if (rc) return rc;
    HIP_TRY(hipMemsetAsync(d_dst, value, (size_t)bytes, h->stream));
    return PSCL_OK;
}

int pscl_set_screening(pscl_handle* h, int enable) {
    if (!h) return fail(PSCL_EINVAL, "NULL handle");
    h->screen = enable != 0;
    return PSCL_OK;
}

int pscl_screening_count(pscl_handle* h, int64_t* count) {
    if (!h || !count) return fail(PSCL_EINVAL, "bad arguments");
    *count = 0;
    if (!h->screened || !h->scratch[h->screened_slot].p) return PSCL_OK;
    int rc = enter(h);
    if (rc) return rc;
    int32_t c = 0;
    HIP_TRY(hipMemcpyAsync(&c, h->scratch[h->screened_slot].p, 4, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    *count = c;
    return PSCL_OK;
}

int pscl_softplus_tails_device(pscl_handle* h, const double* d_v, int64_t n, double* d_exact, double* d_apx) {
    if (!h) return fail(PSCL_EINVAL, "NULL handle");
    if (n < 0) return fail(PSCL_EINVAL, "n must be >= 0");
    if (n == 0) return PSCL_OK;
    if (!d_v || !d_exact || !d_apx) return fail(PSCL_EINVAL, "d_v, d_exact and d_apx are required");
    int rc = enter(h);
    if (rc) return rc;
    LAUNCH_TRY("softplus tails", pscl_launch_softplus_tails(d_v, n, h->d_exp_table, d_exact, d_apx, h->stream));
    return PSCL_OK;
}

int pscl_tail_abs_scan_device(pscl_handle* h, uint32_t lo, uint32_t hi, uint64_t* d_out) {
    return tail_scan(h, lo, hi, d_out, 0);
}

int pscl_tail2_scan_device(pscl_handle* h, uint32_t lo, uint32_t hi, uint64_t* d_out) {
    return tail_scan(h, lo, hi, d_out, 1);
}

int pscl_timing_enable(pscl_handle* h, int enable) {
    if (!h) return fail(PSCL_EINVAL, "NULL handle");
    h->timing = enable != 0;
    h->ev_used = 0;
    return PSCL_OK;
}

int pscl_timing_read_split(pscl_handle* h, int64_t* main_launches, double* main_ms, int64_t* side_launches,
                           double* side_ms) {
    if (!h) return fail(PSCL_EINVAL, "NULL handle");
    int rc = enter(h);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(h->stream));
    quiesce(h);
    double tot[2] = {0.0, 0.0};
    int64_t cnt[2] = {0, 0};
    for (size_t i = 0; i + 1 < h->ev_used; i += 2) {
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, h->ev_pool[i], h->ev_pool[i + 1]));
        const int m = h->ev_main[i / 2] ? 0 : 1;
        tot[m] += ms;
        ++cnt[m];
    }
    if (main_launches) *main_launches = cnt[0];
    if (main_ms) *main_ms = tot[0];
    if (side_launches) *side_launches = cnt[1];
    if (side_ms) *side_ms = tot[1];
    return PSCL_OK;
}

int pscl_timing_read(pscl_handle* h, int64_t* launches, double* total_ms) {
    if (!h || !launches || !total_ms) return fail(PSCL_EINVAL, "bad arguments");
    int64_t n0 = 0, n1 = 0;
    double t0 = 0.0, t1 = 0.0;
    const int rc = pscl_timing_read_split(h, &n0, &t0, &n1, &t1);
    if (rc) return rc;
    *launches = n0 + n1;
    *total_ms = t0 + t1;
    return PSCL_OK;
}

int pscl_host_stats(pscl_handle* h, double* call_ms, double* wait_ms, int64_t* calls, int reset) {
    if (!h) return fail(PSCL_EINVAL, "NULL handle");
    if (call_ms) *call_ms = h->host_call_ms;
    if (wait_ms) *wait_ms = h->host_wait_ms;
    if (calls) *calls = h->host_calls;
    if (reset) {
        h->host_call_ms = h->host_wait_ms = 0.0;
        h->host_calls = 0;
    }
    return PSCL_OK;
}

int pscl_path_stats(pscl_handle* h, int64_t* fused_post_rounds, int64_t* post_rounds, int64_t* fused_tx_blocks,
                    int64_t* post_epw4_launches, int64_t* lane_exact_launches) {
    if (!h) return fail(PSCL_EINVAL, "NULL handle");
    if (lane_exact_launches) *lane_exact_launches = h->n_lane_exact;
    if (post_epw4_launches) *post_epw4_launches = h->n_post_epw4;
    if (fused_post_rounds) *fused_post_rounds = h->n_fpost_rounds;
    if (post_rounds) *post_rounds = h->n_post_rounds;
    if (fused_tx_blocks) *fused_tx_blocks = h->n_fused_tx;
    return PSCL_OK;
}

int pscl_launch_info(pscl_handle* h, int64_t B, int* waves_per_wg, int64_t* grid, int* lds_bytes) {
    if (!h) return fail(PSCL_EINVAL, "NULL handle");
    pscl_decode_params P;
    fill_decode_params(h, P, 0);
    P.B = B;
    if (waves_per_wg) *waves_per_wg = pscl_decode_wpg(P);
    if (grid) *grid = pscl_decode_grid(P);
    if (lds_bytes) *lds_bytes = pscl_decode_lds(P, 0);
    return PSCL_OK;
}

}  // extern "C"
