// encode.hip -- the TX chain on caller payloads (pscl_encode_device, pscl_channel_payload_device).
//
// channel_kernel and channel_long_kernel (scl_kernels.hip) draw each frame's payload from Philox and
// always add AWGN.  The kernels here read the payload from a buffer and write any subset of: the
// message words (attach_crc), the transmitted bits packed in transmission order, and one row per
// frame of either BPSK symbols or LLRs with channel_kernel's noise stream -- in float64 or float32.
// Called with the payloads channel_kernel drew, the LLR rows equal its rows bit for bit (the same
// Philox blocks, bm_pair and fp64 expression; tests/test_gpu_encode.py).
//
//   encode_kernel       N <= 128.  Phase A, one frame per lane: payload -> message -> codeword,
//                       message and code words stored.  Phase B, per frame: the codeword broadcast
//                       with readlane, 64 lanes write the row coalesced.
//   encode_long_kernel  N = 256 .. 1024.  One wavefront per frame; lane w holds message word w and
//                       (w < N / 64) codeword word w.
// Both are compiled per (noise, float32 rows): the symbol instances carry no Philox state.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "scl_device.h"
#include "scl_kernels.h"

namespace {

using namespace pscl;

// payload -> message -> codeword, the first half of the TX chain (run_fer_sweep.py:79-84): the
// payload masked to k_payload bits, the CRC remainder of its bytes (crc.py:19-37; GF(2)-linear, one
// table row per byte) placed at bit k_payload, u[info_set] = msg and x = u G (polar.py:17-29,106-119;
// one table row per message byte).
//   PER_LANE (encode_kernel): the lane holds a whole frame, message words m[0..1], codeword x[0..1].
//   otherwise (encode_long_kernel): the wavefront holds one frame; lane w holds message word w in
//   m[0] (zero from word W on) and codeword word w in x[0] (w < N / 64); every lane takes part.
template <bool PER_LANE>
__device__ __forceinline__ void payload_to_codeword(const pscl_encode_params& P, int lane, uint64_t (&m)[2],
                                                    uint64_t (&x)[2]) {
    constexpr int NH = PER_LANE ? 2 : 1;  // message words this lane holds
    const int kp = P.k_payload, nbp = (kp + 7) >> 3, nb = (P.K + 7) >> 3;
    uint32_t rem = 0;
#pragma unroll
    for (int i = 0; i < NH; ++i) {
        const int w = PER_LANE ? i : lane;
        const int nbits = kp - 64 * w;
        m[i] = nbits >= 64 ? m[i] : (nbits > 0 ? (m[i] & ((1ULL << nbits) - 1)) : 0ULL);
    }
    if (PER_LANE) {
        // (a loop over the table rows, not unrolled: every unrolled row's base is one more SGPR pair)
#pragma unroll 1
        for (int k = 0; k < nbp; ++k)
            rem ^= P.crctab[k * 256 + (uint32_t)(((k < 8 ? m[0] : m[1]) >> (8 * (k & 7))) & 255u)];
    } else {  // lane w's eight bytes, XOR-reduced over the lanes
        for (int t = 0; t < 8; ++t) {
            const int k = 8 * lane + t;
            if (k < nbp) rem ^= P.crctab[k * 256 + (uint32_t)((m[0] >> (8 * t)) & 255u)];
        }
        for (int sft = 1; sft < 64; sft <<= 1) rem ^= (uint32_t)__shfl_xor((int)rem, sft);
    }
    if (P.crc_deg) {  // (the remainder may straddle words w0 and w0 + 1: then o >= 33, the shifts are in range)
        const int w0 = kp >> 6, o = kp & 63;
#pragma unroll
        for (int i = 0; i < NH; ++i) {
            const int w = PER_LANE ? i : lane;
            if (w == w0) m[i] |= (uint64_t)rem << o;
            if (w == w0 + 1 && o + P.crc_deg > 64) m[i] |= (uint64_t)rem >> (64 - o);
        }
    }
    x[0] = x[1] = 0;
    const int NW = P.N >> 6;
    for (int k = 0; k < nb; ++k) {
        const uint64_t mw = PER_LANE ? (k < 8 ? m[0] : m[1]) : shfl_u64(m[0], k >> 3);
        const uint32_t v = (uint32_t)((mw >> (8 * (k & 7))) & 255u);
        if (PER_LANE) {
            x[0] ^= P.xtab[(k * 256 + v) * 2];
            x[1] ^= P.xtab[(k * 256 + v) * 2 + 1];
        } else if (lane < NW) {
            x[0] ^= P.xtab[((size_t)k * 256 + v) * NW + lane];
        }
    }
}

// one row element: the symbol of `bit`, with channel_kernel's noise term when NOISE (its fp64
// expression), rounded once when the rows are float32
template <bool NOISE, bool F32>
__device__ __forceinline__ void store_row(const pscl_encode_params& P, int64_t at, uint32_t bit, double z) {
    const double sym = bit ? -1.0 : 1.0;
    const double v = NOISE ? (sym + P.sigma * z) * P.llr_scale : sym;
    if (F32) static_cast<float*>(P.rows)[at] = (float)v;
    else static_cast<double*>(P.rows)[at] = v;
}

template <bool NOISE, bool F32>
__global__ void __launch_bounds__(256) encode_kernel(const pscl_encode_params P) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int N = P.N, E = P.rm_E ? P.rm_E : N, CW = (E + 63) >> 6;
    const int64_t base = ((int64_t)blockIdx.x * 4 + wave) * 64;  // (one pass: the grid covers the batch)
    if (base >= P.B) return;
    // ---- A: one frame per lane
    const int64_t idx = base + lane;
    uint64_t m[2] = {0, 0}, x[2];
    if (idx < P.B) {
        const uint64_t* src = P.payload + idx * P.Wp;
        if (P.Wp > 0) m[0] = src[0];
        if (P.Wp > 1) m[1] = src[1];
    }
    payload_to_codeword<true>(P, lane, m, x);
    if (P.msg && idx < P.B) {
        P.msg[idx * P.W] = m[0];
        if (P.W > 1) P.msg[idx * P.W + 1] = m[1];
    }
    // the transmitted bits as a sequence of period 128: bit p = y[(p >> 6) & 1] >> (p & 63)
    uint64_t y0 = x[0], y1 = x[1];
    if (P.rm_E) {  // NR: bit p = x[rm_order[p % N]] (interleave, then truncate or repeat)
        y0 = y1 = 0;
        for (int k = 0; k < N; ++k) {
            const int pos = P.rm_order[k];
            const uint64_t b = ((pos < 64 ? x[0] : x[1]) >> (pos & 63)) & 1ULL;
            if (k < 64) y0 |= b << k; else y1 |= b << (k - 64);
        }
        for (int s = N; s < 64; s <<= 1) y0 |= y0 << s;
        if (N <= 64) y1 = y0;
    }
    if (P.code && idx < P.B)
        for (int c = 0; c < CW; ++c) {
            const uint64_t yw = (c & 1) ? y1 : y0;
            const bool part = c == CW - 1 && (E & 63);  // bits past E are zero
            P.code[idx * CW + c] = part ? (yw & ((1ULL << (E & 63)) - 1)) : yw;
        }
    // ---- B: per frame, element p = lane + 64 h + 128 q of its row is bit `lane` of word h
    if (!P.rows) return;
    const int nf = (P.B - base) < 64 ? (int)(P.B - base) : 64;
    for (int j = 0; j < nf; ++j) {
        const uint64_t fj = (uint64_t)(P.frame0 + base + j);
        const uint64_t ya = ((uint64_t)rdl_u32((uint32_t)(y0 >> 32), j) << 32) | rdl_u32((uint32_t)y0, j);
        const uint64_t yb = ((uint64_t)rdl_u32((uint32_t)(y1 >> 32), j) << 32) | rdl_u32((uint32_t)y1, j);
        const int64_t row = (base + j) * E;
        for (int q = 0; q * 128 < E; ++q) {
            double z[2] = {0.0, 0.0};
            if (NOISE) {  // channel_kernel's stream: Philox(frame, pair lane + 64 q)
                const u32x4 rn = philox4x32(u32x4{(uint32_t)fj, (uint32_t)(fj >> 32), (uint32_t)(lane + 64 * q), 0u},
                                            P.k0, P.k1);
                bm_pair(((uint64_t)rn.y << 32) | rn.x, ((uint64_t)rn.w << 32) | rn.z, z[0], z[1]);
            }
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int p = lane + 64 * h + 128 * q;
                if (p < E) store_row<NOISE, F32>(P, row + p, (uint32_t)((h ? yb : ya) >> lane) & 1u, z[h]);
            }
        }
    }
}

template <bool NOISE, bool F32>
__global__ void __launch_bounds__(256) encode_long_kernel(const pscl_encode_params P) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int N = P.N, E = P.rm_E ? P.rm_E : N, CW = (E + 63) >> 6, NW = N >> 6;
    const int64_t idx = (int64_t)blockIdx.x * 4 + wave;  // wave-uniform (one pass: the grid covers the batch)
    if (idx >= P.B) return;
    uint64_t m[2] = {0, 0}, x[2];
    if (lane < P.Wp) m[0] = P.payload[idx * P.Wp + lane];
    payload_to_codeword<false>(P, lane, m, x);
    if (P.msg && lane < P.W) P.msg[idx * P.W + lane] = m[0];
    if (P.code && !P.rm_E) {
        if (lane < NW) P.code[idx * CW + lane] = x[0];  // (CW = N / 64)
    } else if (P.code) {
        // word c of the transmitted bits = the ballot of its 64 bits; lane c keeps it, 64 words per store
        for (int c0 = 0; c0 < CW; c0 += 64) {
            const int cn = CW - c0 < 64 ? CW - c0 : 64;
            uint64_t mine = 0;
            for (int c = 0; c < cn; ++c) {
                const int p = 64 * (c0 + c) + lane;
                const int pos = P.rm_order[p & (N - 1)];
                const uint64_t xw = shfl_u64(x[0], pos >> 6);  // (every lane takes part)
                const uint64_t bal = __ballot(p < E && ((xw >> (pos & 63)) & 1ULL));
                if (lane == c) mine = bal;
            }
            if (lane < cn) P.code[idx * CW + c0 + lane] = mine;
        }
    }
    if (!P.rows) return;
    const uint64_t fr = (uint64_t)(P.frame0 + idx);
    for (int q = 0; q * 128 < E; ++q) {
        double z[2] = {0.0, 0.0};
        if (NOISE) {  // channel_long_kernel's stream: Philox(frame, pair lane + 64 q)
            const u32x4 rn = philox4x32(u32x4{(uint32_t)fr, (uint32_t)(fr >> 32), (uint32_t)(lane + 64 * q), 0u},
                                        P.k0, P.k1);
            bm_pair(((uint64_t)rn.y << 32) | rn.x, ((uint64_t)rn.w << 32) | rn.z, z[0], z[1]);
        }
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int p = lane + 64 * h + 128 * q;
            const int pos = p < E ? (P.rm_E ? P.rm_order[p & (N - 1)] : p) : 0;
            const uint64_t xw = shfl_u64(x[0], pos >> 6);  // (every lane takes part)
            if (p < E) store_row<NOISE, F32>(P, idx * E + p, (uint32_t)(xw >> (pos & 63)) & 1u, z[h]);
        }
    }
}

// One pass, no frame loop in either kernel: the grid covers the batch (PSCL_ENCODE_MAX_B).  With a
// capped grid and a stride loop the compiler keeps every loop-invariant select mask and Philox round
// key live across the loop and parks 17 to 48 SGPRs in VGPR lanes; without it nothing is parked.
template <bool NOISE, bool F32>
void launch(const pscl_encode_params& P, hipStream_t s) {
    if (P.N > PSCL_FAST_N)  // one wavefront per frame, four per workgroup
        hipLaunchKernelGGL((encode_long_kernel<NOISE, F32>), dim3((unsigned)((P.B + 3) / 4)), dim3(256), 0, s, P);
    else  // 64 frames per wavefront
        hipLaunchKernelGGL((encode_kernel<NOISE, F32>), dim3((unsigned)((P.B + 255) / 256)), dim3(256), 0, s, P);
}

}  // namespace

hipError_t pscl_launch_encode(const pscl_encode_params& P, hipStream_t s) {
    if (P.B <= 0) return hipSuccess;
    if (P.B > PSCL_ENCODE_MAX_B) return hipErrorInvalidValue;
    const bool noise = P.rows && P.row_mode == PSCL_ROWS_LLR, f32 = P.rows && P.row_f32;
    if (noise && f32) launch<true, true>(P, s);
    else if (noise) launch<true, false>(P, s);
    else if (f32) launch<false, true>(P, s);
    else launch<false, false>(P, s);
    return hipGetLastError();
}
