// derate.hip -- NR de-rate-matching as a pass of its own (pscl_derate_match_device, and the staged
// mode of pscl_set_rate_match_staged).
//
// out[b][i] = nr_stage(llr + b E, rm_src[i], E, N) (scl_device.h), bit for bit: the E received LLRs
// of frame b de-rate-matched (rate_match.py:19-39: repeats summed in index order, 0.0 + s, the
// remainder copy, one division by the count; E <= N padded with -1.0) and sub-block de-interleaved
// (interleaver.py:26-37).  The decode kernels that read the result are the plain-row instances,
// unchanged: the screening and SC kernels have no register left for a fused gather.
//
//   derate_match_kernel<REP>   one workgroup of 256 threads per tile of 1024 output values =
//                              1024 / N whole frames (one frame at N = 1024, 32 at N = 32).
//     A  thread <-> de-rate-matched position k of a frame (four per thread, 256 apart): the copies
//        src[k + r N] are coalesced loads, the four sums of a thread advance together (four loads in
//        flight); the value goes to LDS.
//     B  thread <-> output position i: the value of k = rm_src[i] from LDS, one coalesced store.
//   The de-interleave is the transpose of an (N / 32) x 32 matrix, k = 32 r + c -> i = c N / 32 + r
//   (interleaver.py:20), computed from i, not loaded.  LDS rows of 32 values are padded to
//   32 + 32 / (N / 32) doubles: the 32 lanes of a ds_read_b64 half-wave read 32 / (N / 32) columns of
//   N / 32 rows (N <= 1024: at most 32 rows), which then fall on 32 distinct 8-byte banks.  N <= 32
//   has no transpose (N < 32: no interleaver at all, the identity).
//   REP = false is E <= N (a copy or the pad, no sum), REP = true is repetition.
// No frame loop: the grid covers the batch (PSCL_DERATE_MAX_B); only the N-vector is staged, never the
// E-row, so E is not bounded by LDS.  Rows need 8-byte alignment only.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "scl_device.h"
#include "scl_kernels.h"

namespace {

using namespace pscl;

constexpr int kTile = 1024;    // output values per workgroup
constexpr int kThreads = 256;
constexpr int kPer = kTile / kThreads;

// LDS index of de-rate-matched position k of a frame (rows of 32, padded; n = log2 N)
__device__ __forceinline__ int lds_index(int k, int n) {
    if (n <= 5) return k;  // (one row or less: no transpose)
    const int pad = 32 >> (n - 5);  // 32 / (N / 32)
    return (k >> 5) * (32 + pad) + (k & 31);
}
// doubles of LDS one frame takes
__device__ __forceinline__ int lds_frame(int n) {
    if (n <= 5) return 1 << n;
    return (1 << (n - 5)) * (32 + (32 >> (n - 5)));
}

template <bool REP>
__global__ void __launch_bounds__(kThreads) derate_match_kernel(const pscl_derate_params P) {
    __shared__ double st[kTile + kTile / 2];  // (the widest padding is N = 64: rows of 48)
    const int n = P.n, N = 1 << n, E = P.E;
    const int t = threadIdx.x;
    const int64_t frame0 = (int64_t)blockIdx.x << (10 - n);  // first frame of the tile
    const int fs = lds_frame(n);
    // ---- A: position k of frame f, four per thread
    double s[kPer];
    const double* src[kPer];
    int k[kPer];
    bool live[kPer];
#pragma unroll
    for (int j = 0; j < kPer; ++j) {
        const int e = t + kThreads * j;
        const int64_t b = frame0 + (e >> n);
        k[j] = e & (N - 1);
        live[j] = b < P.B;
        src[j] = P.llr + (live[j] ? b : 0) * (int64_t)E;
    }
    if (!REP) {
#pragma unroll
        for (int j = 0; j < kPer; ++j) s[j] = (live[j] && k[j] < E) ? src[j][k[j]] : -1.0;
    } else {
        const int reps = E >> n, rem = E - (reps << n);
#pragma unroll
        for (int j = 0; j < kPer; ++j) s[j] = live[j] ? src[j][k[j]] : 0.0;
        for (int r = 1; r < reps; ++r) {
#pragma unroll
            for (int j = 0; j < kPer; ++j) s[j] = s[j] + (live[j] ? src[j][k[j] + (r << n)] : 0.0);
        }
#pragma unroll
        for (int j = 0; j < kPer; ++j) {
            double v = 0.0 + s[j];  // (a -0 sum becomes +0, as numpy's add.at into zeros)
            int cnt = reps;
            if (k[j] < rem) {
                v = v + (live[j] ? src[j][(reps << n) + k[j]] : 0.0);
                ++cnt;
            }
            // (a power-of-two count: the exact reciprocal, the same value as the division)
            if ((cnt & (cnt - 1)) == 0) s[j] = v * pscl_asf64((uint64_t)(1023 - __builtin_ctz((unsigned)cnt)) << 52);
            else s[j] = v / (double)cnt;
        }
    }
#pragma unroll
    for (int j = 0; j < kPer; ++j) {
        const int e = t + kThreads * j;
        st[(e >> n) * fs + lds_index(k[j], n)] = s[j];
    }
    __syncthreads();
    // ---- B: output position i of frame f
#pragma unroll
    for (int j = 0; j < kPer; ++j) {
        const int e = t + kThreads * j;
        const int f = e >> n, i = e & (N - 1);
        // rm_src[i]: i = c (N / 32) + r  <-  k = 32 r + c
        const int kk = n <= 5 ? i : (((i & ((N >> 5) - 1)) << 5) | (i >> (n - 5)));
        const double v = st[f * fs + lds_index(kk, n)];
        if (frame0 + f < P.B) P.out[(frame0 << n) + e] = v;
    }
}

}  // namespace

hipError_t pscl_launch_derate(const pscl_derate_params& P, hipStream_t s) {
    if (P.B <= 0) return hipSuccess;
    if (P.B > PSCL_DERATE_MAX_B || P.n < 1 || P.n > 10 || P.E < 1) return hipErrorInvalidValue;
    const int64_t per = kTile >> P.n;  // frames per workgroup
    const unsigned grid = (unsigned)((P.B + per - 1) / per);
    if (P.E > (1 << P.n)) hipLaunchKernelGGL((derate_match_kernel<true>), dim3(grid), dim3(kThreads), 0, s, P);
    else hipLaunchKernelGGL((derate_match_kernel<false>), dim3(grid), dim3(kThreads), 0, s, P);
    return hipGetLastError();
}
