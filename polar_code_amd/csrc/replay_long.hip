// replay_long.hip -- the decision-LLR replay of the long codes (N = 256, 512, 1024): the leaf LLR at
// every information phase of the path with given information bits (frozen bits 0), recomputed
// top-down through f_minsum / g_node -- dlscl.hip's replay_leaves (N <= 128) at up to 16 words of
// bits.  pscl_path_llrs_device takes it at these lengths, and dl_retry_long under
// PSCL_TUNE_DL_LONG_REPLAY, where it stands in for the history the HIST kernel carries.
//
// One wavefront per entry, the whole tree level in registers: lane l holds elements p = l + 64 r,
// r < R = N / 64.  A level of half-width w maps every pair (q, q + w) to (f, g) in place
// (the g's partial-sum bit is bit q of X, below), so one level buffer suffices:
//   w >= 64   the pair is two registers of one lane: no cross-lane traffic (the first n - 6 levels)
//   w <  64   the pair is one register of lanes l and l ^ w: R independent 64-element problems, the
//             partner's value by DPP (w <= 8) or ds_bpermute (w = 16, 32)
// No LDS is allocated.
//
// Partial sums (replay_leaves' trick): X_m = u after butterfly stages 1, 2, .., 2^(m-1); the g of the
// pair at q on the level of half-width 2^m takes bit q of X_m.  The stages are involutions that
// commute, so one stage per level takes X_m to X_{m-1}.  X is held the way the tree is: lane l keeps
// bit r of one register = bit l + 64 r of X (sixteen 64-bit words in scalar registers left no room:
// 134 spilled at N = 1024).  A stage of 64 D and above is then a shift and a mask within the
// register, a stage below 64 one 32-bit exchange with lane l ^ stage.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "polar_scl.h"
#include "scl_device.h"
#include "scl_kernels.h"

#pragma clang fp contract(off)

namespace {

using pscl::f_minsum;
using pscl::g_node;

template <int CTRL>
__device__ __forceinline__ uint32_t rl_dpp32(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_mov_dpp((int)v, CTRL, 0xF, 0xF, true);
}

// the value of lane (lane ^ S), S = 1..32: quad_perm xor 1 / xor 2, xor 4 as the half-row mirror then
// quad_perm [3,2,1,0], xor 8 as row_ror:8, xor 16 and 32 through ds_bpermute
template <int S>
__device__ __forceinline__ uint32_t rl_xor32(uint32_t v, int lane) {
    if constexpr (S == 1) return rl_dpp32<0xB1>(v);
    else if constexpr (S == 2) return rl_dpp32<0x4E>(v);
    else if constexpr (S == 4) return rl_dpp32<0x1B>(rl_dpp32<0x141>(v));
    else if constexpr (S == 8) return rl_dpp32<0x128>(v);
    else return pscl::bperm32(v, lane ^ S);
}
template <int S>
__device__ __forceinline__ double rl_xor(double x, int lane) {
    const uint64_t v = pscl_asu64(x);
    return pscl_asf64(((uint64_t)rl_xor32<S>((uint32_t)(v >> 32), lane) << 32) | rl_xor32<S>((uint32_t)v, lane));
}

// butterfly stage S of X (bit i with i & S == 0 takes bit i + S) on the lane layout: xb bit r of
// lane l = bit l + 64 r of X
template <int R, int S>
__device__ __forceinline__ uint32_t rl_stage(uint32_t xb, int lane) {
    if constexpr (S >= 64) {
        constexpr int D = S / 64;
        constexpr uint32_t M = D == 1 ? 0x5555u : D == 2 ? 0x3333u : D == 4 ? 0x0f0fu : 0x00ffu;
        return xb ^ ((xb >> D) & M);
    } else {
        const uint32_t oth = rl_xor32<S>(xb, lane);
        return xb ^ ((lane & S) ? 0u : oth);
    }
}

// R = N / 64 (4, 8, 16).  info_words: the R words of the information mask (every phase);
// ob_copy: null, or [entries][W] -- the entry's bit words copied there (dl_retry_long's first post
// pass reads the baseline bits by entry)
template <int R>
__global__ void __launch_bounds__(256) replay_long_kernel(const pscl_replay_params P, int64_t cap,
                                                          const uint64_t* __restrict__ info_words,
                                                          uint64_t* __restrict__ ob_copy) {
    constexpr int N = 64 * R;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t b = (int64_t)blockIdx.x * 4 + wave;
    if (b >= *P.count || b >= cap) return;  // (wave-uniform)
    const int e = P.list ? P.list[b] : (int)b;
    const int64_t row = P.act[e];
    const int W = P.W;
    const uint64_t* bw = P.bits + (P.bits_by_row ? row : b) * W;
    const double* src = P.llr + row * (int64_t)(P.rm_E ? P.rm_E : N);
    double v[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int p = lane + 64 * r;
        v[r] = P.rm_E == 0 ? src[p] : pscl::nr_stage(src, P.rm_src[p], P.rm_E, N);
    }
    if (ob_copy && lane < W) ob_copy[(int64_t)e * W + lane] = bw[lane];
    // the path's bits u at the lane's phases (the information index of phase p: a prefix popcount
    // across the mask words)
    const uint64_t below = (1ULL << lane) - 1ULL;
    uint32_t xb = 0;
    int jbase = 0;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const uint64_t m = info_words[r];
        const bool inf = (m >> lane) & 1ULL;
        const int j = jbase + __popcll(m & below);
        const bool bit = inf && ((bw[inf ? j >> 6 : 0] >> (j & 63)) & 1ULL);  // (j < K where inf)
        xb |= (bit ? 1u : 0u) << r;
        jbase += __popcll(m);
    }
    // X_{n-1}: every stage but the largest (N / 2)
    xb = rl_stage<R, 1>(xb, lane);
    xb = rl_stage<R, 2>(xb, lane);
    xb = rl_stage<R, 4>(xb, lane);
    xb = rl_stage<R, 8>(xb, lane);
    xb = rl_stage<R, 16>(xb, lane);
    xb = rl_stage<R, 32>(xb, lane);
    if constexpr (R >= 4) xb = rl_stage<R, 64>(xb, lane);
    if constexpr (R >= 8) xb = rl_stage<R, 128>(xb, lane);
    if constexpr (R >= 16) xb = rl_stage<R, 256>(xb, lane);
    // levels of half-width w = 64 D >= 64: registers r and r + D of one lane
    auto wide = [&](auto DC) {
        constexpr int D = decltype(DC)::value;
        if constexpr (D >= 1 && D < R) {
#pragma unroll
            for (int r = 0; r < R; ++r)
                if (!(r & D)) {
                    const double a = v[r], bb = v[r + D];
                    v[r] = f_minsum(a, bb);
                    v[r + D] = g_node(a, bb, (xb >> r) & 1u);
                }
            xb = rl_stage<R, 32 * D>(xb, lane);  // X down a level: stage w / 2
        }
    };
    wide(std::integral_constant<int, 8>{});
    wide(std::integral_constant<int, 4>{});
    wide(std::integral_constant<int, 2>{});
    wide(std::integral_constant<int, 1>{});
    // levels of half-width w < 64: lanes l and l ^ w; the pair's first position is the lane without
    // bit w, whose X bits the second one fetches
    auto narrow = [&](auto WC) {
        constexpr int w = decltype(WC)::value;
        const bool hi = (lane & w) != 0;  // (the pair's second position: g, else f)
        const uint32_t xq = rl_xor32<w>(xb, lane);
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const double oth = rl_xor<w>(v[r], lane);
            const double a = hi ? oth : v[r], bb = hi ? v[r] : oth;
            const double gv = g_node(a, bb, (xq >> r) & 1u), fv = f_minsum(a, bb);
            v[r] = hi ? gv : fv;
        }
        if constexpr (w > 1) xb = rl_stage<R, w / 2>(xb, lane);
    };
    narrow(std::integral_constant<int, 32>{});
    narrow(std::integral_constant<int, 16>{});
    narrow(std::integral_constant<int, 8>{});
    narrow(std::integral_constant<int, 4>{});
    narrow(std::integral_constant<int, 2>{});
    narrow(std::integral_constant<int, 1>{});
    double* out = P.out + (int64_t)e * P.K;
    jbase = 0;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const uint64_t m = info_words[r];
        if ((m >> lane) & 1ULL) out[jbase + __popcll(m & below)] = v[r];
        jbase += __popcll(m);
    }
}

}  // namespace

hipError_t pscl_launch_replay_long(const pscl_replay_params& P, int64_t cap, const uint64_t* info_words,
                                   uint64_t* ob_copy, hipStream_t s) {
    if (P.row_f32 || !info_words || P.W < 1 || P.W > 16) return hipErrorInvalidValue;
    if (P.N != 256 && P.N != 512 && P.N != 1024) return hipErrorInvalidValue;
    if (cap <= 0) return hipSuccess;
    const dim3 g((unsigned)((cap + 3) / 4)), b(256);
    if (P.N == 256)
        hipLaunchKernelGGL(replay_long_kernel<4>, g, b, 0, s, P, cap, info_words, ob_copy);
    else if (P.N == 512)
        hipLaunchKernelGGL(replay_long_kernel<8>, g, b, 0, s, P, cap, info_words, ob_copy);
    else
        hipLaunchKernelGGL(replay_long_kernel<16>, g, b, 0, s, P, cap, info_words, ob_copy);
    return hipGetLastError();
}
