// label.hip -- the chain around the forced decodes of pscl_label_device (flip labels for beta
// training, dl_scl_polar/train/make_dataset.py:52-91 over a device batch).
//
//   label_rank_kernel<MK>   one wavefront per entry over the replayed decision LLRs l0[e][K]: lane l
//                           holds the MK = ceil(K / 64) keys of indices l, l + 64, ..; a key is
//                           (float32 bits of |(float)L0|) << 32 | index (label_rank.h: the bits of a
//                           non-negative float are monotone in it, and the index in the low word makes
//                           equal values resolve to the lower index).  T wave-wide minima -- the lane's
//                           own minimum, four DPP steps inside a 16-lane row, two exchanges across the
//                           rows -- each winner written to order[e][t] and removed (keys are distinct,
//                           so exactly one lane holds it).  The abs_l0 row is stored on the way in.
//   label_step_kernel       one thread per frame of the round just decoded: the stop rule (CRC flag
//                           and result words == sent words), the label of the hits, and for the rest
//                           the next round's dense state -- entry id, LLR row, force words built from
//                           the BASELINE words and order[e][t + 1] -- appended with one atomic per
//                           wavefront.  Counts: one atomic per wavefront and counter.
// The rounds' lists and counts never leave the device; the decodes between the steps are the handle's
// forced-bit kernels (capi.cpp).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "label_rank.h"
#include "scl_device.h"
#include "scl_kernels.h"

namespace {

template <int CTRL>
__device__ __forceinline__ uint32_t lbl_dpp32(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_mov_dpp((int)v, CTRL, 0xF, 0xF, true);
}
template <int CTRL>
__device__ __forceinline__ uint64_t lbl_dpp64(uint64_t v) {
    return ((uint64_t)lbl_dpp32<CTRL>((uint32_t)(v >> 32)) << 32) | lbl_dpp32<CTRL>((uint32_t)v);
}
__device__ __forceinline__ uint64_t min64(uint64_t a, uint64_t b) { return b < a ? b : a; }

// the minimum of v over the wavefront, in every lane (steps as dl_post_kernel's argmin: quad_perm
// xor 1, xor 2, row_half_mirror, row_mirror, then the rows by ds_bpermute)
__device__ __forceinline__ uint64_t wave_min64(uint64_t v, int lane) {
    v = min64(v, lbl_dpp64<0xB1>(v));
    v = min64(v, lbl_dpp64<0x4E>(v));
    v = min64(v, lbl_dpp64<0x141>(v));
    v = min64(v, lbl_dpp64<0x140>(v));
    v = min64(v, pscl::shfl_u64(v, lane ^ 16));
    v = min64(v, pscl::shfl_u64(v, lane ^ 32));
    return v;
}

constexpr int kRankWaves = 4;

template <int MK>
__global__ void __launch_bounds__(kRankWaves * 64) label_rank_kernel(const pscl_label_rank_params R) {
    const int lane = threadIdx.x & 63;
    const int64_t e = (int64_t)blockIdx.x * kRankWaves + (threadIdx.x >> 6);
    if (e >= R.A) return;  // (wave-uniform)
    const int K = R.K;
    const double* src = R.l0 + e * K;
    float* dst = R.abs_l0 + e * K;
    uint64_t key[MK];
#pragma unroll
    for (int m = 0; m < MK; ++m) {
        const int j = lane + 64 * m;
        key[m] = ~0ULL;
        if (j < K) {
            const uint32_t b = pscl_label_abs_bits(src[j]);
            dst[j] = pscl_label_abs_value(b);
            key[m] = pscl_label_key(b, j);
        }
    }
    for (int t = 0; t < R.T; ++t) {
        uint64_t bk = key[0];
#pragma unroll
        for (int m = 1; m < MK; ++m) bk = min64(bk, key[m]);
        bk = wave_min64(bk, lane);
        if (lane == 0) R.order[e * R.T + t] = pscl_label_key_index(bk);
#pragma unroll
        for (int m = 0; m < MK; ++m)
            if (key[m] == bk) key[m] = ~0ULL;
    }
}

constexpr int kStepThreads = 256;

__global__ void __launch_bounds__(kStepThreads) label_step_kernel(const pscl_label_step_params S) {
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * kStepThreads + threadIdx.x;
    const int W = S.W, T = S.T, t = S.t;
    int64_t n = S.A;
    if (t >= 0) {
        const int64_t c = *S.in_count;
        n = c < S.A ? c : S.A;
    }
    if (i == 0) {
        if (t < 0) S.counts[PSCL_LBL_ENTRIES] = S.A;
        else atomicAdd((unsigned long long*)&S.counts[PSCL_LBL_DECODES], (unsigned long long)n);
    }
    const bool live = i < n;
    int64_t e = 0, f = 0;
    bool hit = false;
    if (live) {
        e = t < 0 ? i : (int64_t)S.ent_in[i];
        f = S.act[e];
        if (t < 0) {
            S.frame[e] = f;
        } else {
            hit = (S.of[i] & PSCL_FLAG_CRC_PASS) != 0;
            const uint64_t* got = S.ob + i * W;
            const uint64_t* want = S.sent + f * S.sent_stride;
            for (int w = 0; w < W; ++w) {
                const int bits = S.K - 64 * w;
                const uint64_t m = bits >= 64 ? ~0ULL : ((1ULL << bits) - 1ULL);
                hit = hit && ((got[w] ^ want[w]) & m) == 0;
            }
        }
    }
    const bool last = t + 1 >= T;
    const bool done = live && t >= 0 && (hit || last);
    const bool next = live && !hit && !last;
    if (done) {
        S.flip[e] = hit ? S.order[e * T + t] : -1;
        if (S.rank) S.rank[e] = hit ? t : -1;
    }
    if (t >= 0) {
        const uint64_t mh = __ballot(live && hit), mu = __ballot(done && !hit);
        if (lane == 0) {
            if (mh) atomicAdd((unsigned long long*)&S.counts[PSCL_LBL_LABELLED], (unsigned long long)__popcll(mh));
            if (mu) atomicAdd((unsigned long long*)&S.counts[PSCL_LBL_UNREPAIRED], (unsigned long long)__popcll(mu));
        }
    }
    // the survivors to round t + 1: one atomic per wavefront reserves their places
    const uint64_t mn = __ballot(next);
    if (!mn) return;
    const int leader = __ffsll((unsigned long long)mn) - 1;
    int base = 0;
    if (lane == leader) base = atomicAdd(S.out_count, __popcll(mn));
    base = __shfl(base, leader);
    if (!next) return;
    const int64_t pos = base + __popcll(mn & ((1ULL << lane) - 1ULL));
    if (pos >= S.A) return;  // (cannot happen: a round never holds more frames than entries)
    S.ent_out[pos] = (int32_t)e;
    S.row_out[pos] = f;
    const int idx = S.order[e * T + t + 1];
    const uint64_t* bw = S.base + f * W;
    uint64_t* fr = S.force_out + pos * 2 * W;
    for (int w = 0; w < W; ++w) pscl_label_force_word(bw[w], w, idx, &fr[w], &fr[W + w]);
}

}  // namespace

hipError_t pscl_launch_label_rank(const pscl_label_rank_params& R, hipStream_t s) {
    if (R.A <= 0) return hipSuccess;
    if (R.K < 1 || R.K > PSCL_MAX_N || R.T < 1 || R.T > PSCL_LABEL_MAX_FLIPS || R.T > R.K) return hipErrorInvalidValue;
    const int64_t grid = (R.A + kRankWaves - 1) / kRankWaves;
    if (grid > 0x7fffffffLL) return hipErrorInvalidValue;
    const dim3 g((unsigned)grid), b(kRankWaves * 64);
    const int mk = (R.K + 63) / 64;
    if (mk <= 1) hipLaunchKernelGGL((label_rank_kernel<1>), g, b, 0, s, R);
    else if (mk <= 2) hipLaunchKernelGGL((label_rank_kernel<2>), g, b, 0, s, R);
    else if (mk <= 4) hipLaunchKernelGGL((label_rank_kernel<4>), g, b, 0, s, R);
    else if (mk <= 8) hipLaunchKernelGGL((label_rank_kernel<8>), g, b, 0, s, R);
    else hipLaunchKernelGGL((label_rank_kernel<16>), g, b, 0, s, R);
    return hipGetLastError();
}

hipError_t pscl_launch_label_step(const pscl_label_step_params& S, hipStream_t s) {
    if (S.A <= 0) return hipSuccess;
    if (S.T < 1 || S.t < -1 || S.t >= S.T || S.W < 1) return hipErrorInvalidValue;
    const int64_t grid = (S.A + kStepThreads - 1) / kStepThreads;
    if (grid > 0x7fffffffLL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(label_step_kernel, dim3((unsigned)grid), dim3(kStepThreads), 0, s, S);
    return hipGetLastError();
}
