// sc128_lane.hip -- lane-parallel successive cancellation of the N = 128 codes for gfx950: stage 1
// of pscl_adaptive_device (sc_decode, dl_scl_polar/polar/polar.py:130-168, plus check_crc,
// crc.py:40-56), and the small kernels of its hand-off to the list decoder.
//
// Layout.  A frame is decoded by the four lanes of one quad, 16 frames per wavefront, the whole
// LLR tree in registers and every cross-lane move a quad_perm DPP (no LDS in the tree, no
// bpermute).  Element i of a tree vector of length M >= 4 lives on lane i & 3 of the quad, slot
// i >> 2: the butterfly partners i and i + M/2 then share a lane down to M = 8, so the levels
// 128 -> 4 are lane-local f/g over M/8 slots.  Below that the vectors are replicated: a length-4
// vector holds element q on lane q, its children come out as element q & 1 on every lane (the
// partner q ^ 2 through quad_perm, f being symmetric), and the leaf value on all four.  The leaf
// decisions are therefore quad-uniform, and every lane keeps the frame's whole u vector and forms
// the partial sums (x = (xl ^ xr, xr), polar.py:163) with plain bit operations.  g on the
// replicated levels flips the sign of whichever operand is `a` on that lane and adds; IEEE
// addition commutes bit for bit, so b + (+-a) is the reference's value on every lane.
//
// The information mask is a kernel argument (SGPRs): a sub-tree whose leaves are all frozen decides
// zeros whatever its LLRs are, so it is skipped by a scalar branch -- its f values are never
// formed, and the parent's g sees x = 0.  The tree is fully unrolled (compile-time register
// indices; a runtime-indexed array would go to scratch), the mask tests are the only branches.
//
// Epilogue: the quad splits the table work of the scl128 epilogue tables (u-byte -> information
// bits, information nibble -> CRC syndrome, staged in LDS once per workgroup): lane q gathers the
// u bytes 4q..4q+3 and the syndrome of information word q, combined over the quad with two DPP
// steps each.  Lane 0 of a quad stores best / flags / stage.
//
// Rate-matched rows (E received LLRs): each lane de-rate-matches the positions 4 j + q from their
// quad-contiguous received values (nr_value), and the sub-block de-interleave, which moves a value to
// another lane, is one pass through 16.5 KB of LDS per wavefront.  (Gathering rm_src[i] straight from
// HBM put every lane of a load on its own cache line: 3.2 ms per 10^6 frames against 0.24 plain.)
//
// Arithmetic is fp64 min, add, compare and sign operations only -- nothing to contract.
#include "scl_device.h"
#include "scl_kernels.h"

using namespace pscl;

// Float32 rows (pscl_sc_device_f32 and the SC stage of the other _f32 calls): sc128_lane_f32.hip compiles
// this file with PSCL_SC128_F32_UNIT and gets the two kernel instances over float rows under a name of
// their own (sc128_lane_kernel_f32<RM>), the float32 twin of the row gather, and their launches -- and
// nothing else, so this file's own code object holds exactly what it held before.  A row element is
// widened as it is loaded (v_cvt_f64_f32, exact; the wave's fp32 denormal mode is IEEE in every
// instance, so subnormals and -0 keep their value and sign); everything after the load is this file's
// fp64 code unchanged.
#ifdef PSCL_SC128_F32_UNIT
using sc_llr_t = float;
#define sc128_lane_kernel sc128_lane_kernel_f32
#else
using sc_llr_t = double;
#endif

namespace {

constexpr int kQuadX1 = 0xB1;  // quad_perm [1,0,3,2]: lane q ^ 1
constexpr int kQuadX2 = 0x4E;  // quad_perm [2,3,0,1]: lane q ^ 2
constexpr int kFramesPerWave = 16;
// wavefronts per workgroup: four, or two for rate-matched rows (their LDS staging rows: 40 KB per
// workgroup with the tables, four workgroups per CU)
constexpr int wavesPerWg(bool rm) { return rm ? 2 : 4; }
// doubles between the LDS staging rows of two frames (rate-matched rows): 128 + 4, so that the quads'
// 32-byte stores of one position fall 8 banks apart
constexpr int kStageStride = 132;

template <int CTRL>
__device__ __forceinline__ uint32_t qdpp32(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_mov_dpp((int)v, CTRL, 0xF, 0xF, true);
}
template <int CTRL>
__device__ __forceinline__ double qdpp64(double v) {
    const uint64_t u = pscl_asu64(v);
    return pscl_asf64(((uint64_t)qdpp32<CTRL>((uint32_t)(u >> 32)) << 32) | qdpp32<CTRL>((uint32_t)u));
}
template <int CTRL>
__device__ __forceinline__ uint64_t qdpp_u64(uint64_t u) {
    return ((uint64_t)qdpp32<CTRL>((uint32_t)(u >> 32)) << 32) | qdpp32<CTRL>((uint32_t)u);
}

// v with its sign flipped where bit 31 of s is set
__device__ __forceinline__ double flip_sign(double v, uint32_t s) {
    const uint64_t u = pscl_asu64(v);
    return pscl_asf64(((uint64_t)((uint32_t)(u >> 32) ^ (s & 0x80000000u)) << 32) | (uint32_t)u);
}

// nr_stage (scl_device.h) with the mean's division by a power-of-two count done as the exact
// multiplication by its reciprocal -- the same correctly rounded value; E = 256 averages pairs, and
// 32 fp64 divisions per lane were most of the rate-matched front end
__device__ __forceinline__ double nr_value(const sc_llr_t* src, int k, int E) {
    constexpr int N = 128;
    if (E <= N) return k < E ? (double)src[k] : -1.0;
    const int reps = E / N, rem = E - reps * N;
    double s = (double)src[k];
    for (int r = 1; r < reps; ++r) s = s + (double)src[k + r * N];
    s = 0.0 + s;
    int cnt = reps;
    if (k < rem) {
        s = s + (double)src[reps * N + k];
        ++cnt;
    }
    if ((cnt & (cnt - 1)) == 0) return s * pscl_asf64((uint64_t)(1023 - __builtin_ctz((unsigned)cnt)) << 52);
    return s / (double)cnt;
}

// per-lane constants of the quad layout and the wave-uniform information mask
struct ScCtx {
    uint64_t mask0, mask1;  // information mask (uniform)
    uint32_t q;             // lane within the quad
    uint32_t low_half;      // all ones on lanes 0, 1 (whose own element is `a` at the 4 -> 2 level)
    uint32_t even;          // all ones on lanes 0, 2 (whose own element is `a` at the 2 -> 1 level)
};

// does the sub-tree of M leaves from phase S hold an information bit (wave-uniform)
template <int M, int S>
__device__ __forceinline__ bool has_info(const ScCtx& c) {
    static_assert(M <= 64 && (S & 63) + M <= 64, "a sub-tree lies in one mask word");
    const uint64_t w = S < 64 ? c.mask0 : c.mask1;
    const uint64_t m = M == 64 ? ~0ULL : ((1ULL << M) - 1ULL);
    return ((w >> (S & 63)) & m) != 0ULL;
}

template <int M>
struct XBits {
    using type = uint32_t;
};
template <>
struct XBits<64> {
    using type = uint64_t;
};

// leaf at phase S (an information bit: the callers test the mask): u = llr < 0 (polar.py:152)
template <int S>
__device__ __forceinline__ uint32_t sc_leaf(double v, uint32_t (&u)[4]) {
    const uint32_t bit = v < 0.0 ? 1u : 0u;
    u[S >> 5] |= bit << (S & 31);
    return bit;
}

// node of 2 leaves: `in` is element q & 1 of its two LLRs
template <int S>
__device__ __forceinline__ uint32_t sc_node2(double in, const ScCtx& c, uint32_t (&u)[4]) {
    const double other = qdpp64<kQuadX1>(in);
    uint32_t xl = 0, xr = 0;
    if (has_info<1, S>(c)) xl = sc_leaf<S>(f_minsum(in, other), u);
    if (has_info<1, S + 1>(c)) {
        const uint32_t sg = xl << 31;  // g = b + (1 - 2 xl) a; `a` is the own value on even lanes
        xr = sc_leaf<S + 1>(flip_sign(in, sg & c.even) + flip_sign(other, sg & ~c.even), u);
    }
    return (xl ^ xr) | (xr << 1);
}

// node of 4 leaves: `in` is element q of its four LLRs; the children hold element q & 1
template <int S>
__device__ __forceinline__ uint32_t sc_node4(double in, const ScCtx& c, uint32_t (&u)[4]) {
    const double other = qdpp64<kQuadX2>(in);
    uint32_t xl = 0, xr = 0;
    if (has_info<2, S>(c)) xl = sc_node2<S>(f_minsum(in, other), c, u);
    if (has_info<2, S + 2>(c)) {
        const uint32_t sg = (xl >> (c.q & 1u)) << 31;  // x bit of element q & 1; `a` is own on lanes 0, 1
        xr = sc_node2<S + 2>(flip_sign(in, sg & c.low_half) + flip_sign(other, sg & ~c.low_half), c, u);
    }
    return (xl ^ xr) | (xr << 2);
}

// node of M >= 8 leaves: `in` holds the lane's M / 4 slots (element 4 j + q in slot j); both
// butterfly operands of an output sit on the same lane
template <int M, int S>
__device__ __forceinline__ typename XBits<M>::type sc_node(const double (&in)[M / 4], const ScCtx& c, uint32_t (&u)[4]) {
    constexpr int H = M / 2, NS = M / 8;
    using XH = typename XBits<H>::type;
    using XM = typename XBits<M>::type;
    XH xl = 0, xr = 0;
    if (has_info<H, S>(c)) {
        if constexpr (H == 4) {
            xl = sc_node4<S>(f_minsum(in[0], in[1]), c, u);
        } else {
            double l[NS];
#pragma unroll
            for (int j = 0; j < NS; ++j) l[j] = f_minsum(in[j], in[j + NS]);
            xl = sc_node<H, S>(l, c, u);
        }
    }
    if (has_info<H, S + H>(c)) {
        const XH xs = xl >> c.q;  // bit 4 j: the partial sum of element 4 j + q
        if constexpr (H == 4) {
            xr = sc_node4<S + H>(g_node_wbit(in[0], in[1], (uint32_t)xs, 0u), c, u);
        } else {
            double r[NS];
#pragma unroll
            for (int j = 0; j < NS; ++j) {
                const uint32_t w = (4 * j) < 32 ? (uint32_t)xs : (uint32_t)((uint64_t)xs >> 32);
                r[j] = g_node_wbit(in[j], in[j + NS], w, (uint32_t)((4 * j) & 31));
            }
            xr = sc_node<H, S + H>(r, c, u);
        }
    }
    return (XM)(xl ^ xr) | ((XM)xr << H);
}

// the root: two 64-leaf halves in the two mask words
__device__ __forceinline__ void sc_root(const double (&in)[32], const ScCtx& c, uint32_t (&u)[4]) {
    constexpr int NS = 16;
    uint64_t xl = 0;
    if (c.mask0) {
        double l[NS];
#pragma unroll
        for (int j = 0; j < NS; ++j) l[j] = f_minsum(in[j], in[j + NS]);
        xl = sc_node<64, 0>(l, c, u);
    }
    if (c.mask1) {
        const uint64_t xs = xl >> c.q;
        double r[NS];
#pragma unroll
        for (int j = 0; j < NS; ++j)
            r[j] = g_node_wbit(in[j], in[j + NS], (4 * j) < 32 ? (uint32_t)xs : (uint32_t)(xs >> 32), (uint32_t)((4 * j) & 31));
        (void)sc_node<64, 64>(r, c, u);
    }
}

template <typename T>
__device__ __forceinline__ T pick4(uint32_t q, T a0, T a1, T a2, T a3) {
    const T lo = (q & 1u) ? a1 : a0, hi = (q & 1u) ? a3 : a2;
    return (q & 2u) ? hi : lo;
}

// (a register budget of three wavefronts per SIMD, 168 VGPRs: the compiler otherwise settles at
// ~190 for two; neither form spills.  The rate-matched instance keeps the budget of two: its LDS
// staging rows admit eight wavefronts per CU anyway, and at 168 it would spill 4 VGPRs)
template <bool RM>
__global__ void __attribute__((amdgpu_waves_per_eu(RM ? 2 : 3))) __launch_bounds__(wavesPerWg(RM) * 64) sc128_lane_kernel(const pscl_sc_params P) {
    constexpr int kFramesPerWg = kFramesPerWave * wavesPerWg(RM);
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    // the epilogue tables, once per workgroup
    {
        uint64_t* dst = reinterpret_cast<uint64_t*>(smem);
        for (int i = threadIdx.x; i < P.epi_words; i += blockDim.x) dst[i] = P.epi_table[i];
    }
    __syncthreads();
    const uint8_t* const GT = smem;                                                // [16][256] u-byte -> info bits
    const uint32_t* const ST = reinterpret_cast<const uint32_t*>(smem + 16 * 256);  // [K4][16] nibble -> syndrome
    const int K4 = (P.K + 3) / 4;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // RM: this wavefront's staging rows, behind the tables
    double* const stage_rows = reinterpret_cast<double*>(smem + (size_t)P.epi_words * 8) + wave * kFramesPerWave * kStageStride;
    ScCtx c;
    c.mask0 = P.info_mask[0];
    c.mask1 = P.info_mask[1];
    c.q = (uint32_t)lane & 3u;
    c.low_half = c.q < 2u ? 0xffffffffu : 0u;
    c.even = (c.q & 1u) ? 0u : 0xffffffffu;
    const uint32_t q = c.q;
    // the information mask as 32-bit words (uniform), this lane's word and the count below it
    const uint32_t mw0 = (uint32_t)c.mask0, mw1 = (uint32_t)(c.mask0 >> 32), mw2 = (uint32_t)c.mask1,
                   mw3 = (uint32_t)(c.mask1 >> 32);
    const uint32_t p0 = __builtin_popcount(mw0), p1 = p0 + __builtin_popcount(mw1), p2 = p1 + __builtin_popcount(mw2);
    const uint32_t mw = pick4<uint32_t>(q, mw0, mw1, mw2, mw3);
    const uint32_t off = pick4<uint32_t>(q, 0u, p0, p1, p2);
    const int64_t rowlen = RM ? (int64_t)P.rm_E : 128;
    for (int64_t g0 = (int64_t)blockIdx.x * kFramesPerWg + wave * kFramesPerWave; g0 < P.B;
         g0 += (int64_t)gridDim.x * kFramesPerWg) {
        const int64_t f = g0 + (lane >> 2);
        const bool valid = f < P.B;
        const sc_llr_t* row = reinterpret_cast<const sc_llr_t*>(P.llr) + (valid ? f : g0) * rowlen;  // (a ragged wave's empty quads decode frame g0 again)
        double ch[32];
        if constexpr (RM) {
            // rate matched: position k = 4 j + q of the de-rate-matched vector is formed from its
            // quad-contiguous received values (as the plain rows load), and the de-interleave --
            // element i is position rm_src[i], another lane's -- goes through the wavefront's LDS rows
            double* const st = stage_rows + (lane >> 2) * kStageStride;
            // (eight positions, 16 loads at E = 256, in flight per lane; fully unrolled the loop takes
            // all 256 VGPRs.  The depth measured no difference: 0.97-1.00 ms per 10^6 frames at 2 and 8)
#pragma unroll 8
            for (int j = 0; j < 32; ++j) st[4 * j + (int)q] = nr_value(row, 4 * j + (int)q, P.rm_E);
            wave_lds_fence();
#pragma unroll
            for (int j = 0; j < 32; ++j) ch[j] = st[P.rm_src[4 * j + (int)q]];
            wave_lds_fence();  // (read before the next iteration's rows overwrite them)
        } else {
            // (float32 rows: one 4-byte load per lane and slot, a quad reading 16 contiguous bytes; 8- and
            // 16-byte loads with a quad_perm exchange measured 1-4 % slower)
#pragma unroll
            for (int j = 0; j < 32; ++j) ch[j] = (double)row[4 * j + (int)q];
        }
        uint32_t u[4] = {0u, 0u, 0u, 0u};
        // (the mask made opaque per iteration: hoisted out of the frame loop, the 255 sub-tree tests
        // would each hold an SGPR across it and spill)
        asm volatile("" : "+s"(c.mask0), "+s"(c.mask1));
        sc_root(ch, c, u);
        // ---- epilogue: u[info_set] as words, CRC syndrome
        const uint32_t uw = pick4<uint32_t>(q, u[0], u[1], u[2], u[3]);
        uint32_t chunk = 0, sh = 0;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            chunk |= (uint32_t)GT[(4 * q + t) * 256 + ((uw >> (8 * t)) & 255u)] << sh;
            sh += __builtin_popcount((mw >> (8 * t)) & 255u);
        }
        // chunk (at most 32 bits) at bit `off` of the 128-bit information vector
        uint64_t ib0, ib1;
        if (off < 64u) {
            ib0 = (uint64_t)chunk << off;
            ib1 = off > 32u ? (uint64_t)chunk >> (64u - off) : 0ULL;
        } else {
            ib0 = 0ULL;
            ib1 = (uint64_t)chunk << (off - 64u);
        }
        ib0 |= qdpp_u64<kQuadX1>(ib0);
        ib1 |= qdpp_u64<kQuadX1>(ib1);
        ib0 |= qdpp_u64<kQuadX2>(ib0);
        ib1 |= qdpp_u64<kQuadX2>(ib1);
        const uint32_t iw = pick4<uint32_t>(q, (uint32_t)ib0, (uint32_t)(ib0 >> 32), (uint32_t)ib1, (uint32_t)(ib1 >> 32));
        uint32_t syn = 0;
#pragma unroll
        for (int t = 0; t < 8; ++t) {
            const int m = 8 * (int)q + t;
            if (m < K4) syn ^= ST[m * 16 + ((iw >> (4 * t)) & 15u)];
        }
        syn ^= qdpp32<kQuadX1>(syn);
        syn ^= qdpp32<kQuadX2>(syn);
        const bool pass = syn == 0u;
        if (valid && q == 0u) {
            P.best[f * P.W] = ib0;
            if (P.W > 1) P.best[f * P.W + 1] = ib1;
            P.flags[f] = pass ? (uint8_t)PSCL_FLAG_CRC_PASS : (uint8_t)0;
            if (P.stage) P.stage[f] = pass ? (uint8_t)1 : (uint8_t)2;
        }
    }
}

#ifdef PSCL_SC128_F32_UNIT
// rows act[i] of the float32 llr, widened, densely: one thread per value
__global__ void __launch_bounds__(256) sc_gather_rows_f32_kernel(const float* __restrict__ llr, int64_t row,
                                                                 const int64_t* __restrict__ act, int64_t n,
                                                                 double* __restrict__ out) {
    const int64_t total = n * row;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = i / row, k = i - r * row;
        out[i] = (double)llr[act[r] * row + k];
    }
}
#else
// rows act[i] of llr, densely: one thread per value
__global__ void __launch_bounds__(256) sc_gather_rows_kernel(const double* __restrict__ llr, int64_t row,
                                                             const int64_t* __restrict__ act, int64_t n,
                                                             double* __restrict__ out) {
    const int64_t total = n * row;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = i / row, k = i - r * row;
        out[i] = llr[act[r] * row + k];
    }
}

// dense results back to their frames' rows
__global__ void __launch_bounds__(256) sc_scatter_results_kernel(const int64_t* __restrict__ act, int64_t n, int W,
                                                                 const uint64_t* __restrict__ best_in,
                                                                 const uint8_t* __restrict__ flags_in,
                                                                 uint64_t* __restrict__ best, uint8_t* __restrict__ flags) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t f = act[i];
        for (int w = 0; w < W; ++w) best[f * W + w] = best_in[i * W + w];
        flags[f] = flags_in[i];
    }
}

__global__ void sc_add_counter_kernel(int64_t* counters, int slot, int64_t v) {
    if (blockIdx.x == 0 && threadIdx.x == 0)
        atomicAdd(reinterpret_cast<unsigned long long*>(counters) + slot, (unsigned long long)v);
}

// the escalated count of pscl_adaptive_async_device, read on the device: counters[slot] += *count
// (counters may be null) and *out = *count (out may be null)
__global__ void sc_publish_count_kernel(const int32_t* __restrict__ count, int64_t* counters, int slot, int32_t* out) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        const int32_t c = *count;
        if (counters && c > 0) atomicAdd(reinterpret_cast<unsigned long long*>(counters) + slot, (unsigned long long)c);
        if (out) *out = c;
    }
}

#endif  // PSCL_SC128_F32_UNIT

}  // namespace

#ifdef PSCL_SC128_F32_UNIT
// (grid, workgroup and LDS as the float64 launch: the staging rows of the rate-matched form hold doubles)
hipError_t pscl_launch_sc_lane_f32(const pscl_sc_params& P, hipStream_t s) {
    if (P.B <= 0) return hipSuccess;
    const dim3 g((unsigned)pscl_sc_lane_grid(P)), b(wavesPerWg(P.rm_E != 0) * 64);
    const size_t lds = (size_t)pscl_sc_lane_lds(P);
    if (P.rm_E)
        hipLaunchKernelGGL(sc128_lane_kernel<true>, g, b, lds, s, P);
    else
        hipLaunchKernelGGL(sc128_lane_kernel<false>, g, b, lds, s, P);
    return hipGetLastError();
}

hipError_t pscl_launch_gather_rows_f32(const float* llr, int64_t row, const int64_t* act, int64_t n, double* out,
                                       hipStream_t s) {
    if (n <= 0) return hipSuccess;
    int64_t grid = (n * row + 255) / 256;
    if (grid > 65536) grid = 65536;
    hipLaunchKernelGGL(sc_gather_rows_f32_kernel, dim3((unsigned)grid), dim3(256), 0, s, llr, row, act, n, out);
    return hipGetLastError();
}
#else

int pscl_sc_lane_lds(const pscl_sc_params& P) {
    return P.epi_words * 8 + (P.rm_E ? wavesPerWg(true) * kFramesPerWave * kStageStride * 8 : 0);
}

// workgroups of 64 (rate matched: 32) frames, capped at eight per CU of a 256-CU device (they
// stride over the rest)
int64_t pscl_sc_lane_grid(const pscl_sc_params& P) {
    const int fpw = kFramesPerWave * wavesPerWg(P.rm_E != 0);
    int64_t grid = (P.B + fpw - 1) / fpw;
    if (grid > 2048) grid = 2048;
    return grid < 1 ? 1 : grid;
}

hipError_t pscl_launch_sc_lane(const pscl_sc_params& P, hipStream_t s) {
    if (P.B <= 0) return hipSuccess;
    const dim3 g((unsigned)pscl_sc_lane_grid(P)), b(wavesPerWg(P.rm_E != 0) * 64);
    const size_t lds = (size_t)pscl_sc_lane_lds(P);
    if (P.rm_E)
        hipLaunchKernelGGL(sc128_lane_kernel<true>, g, b, lds, s, P);
    else
        hipLaunchKernelGGL(sc128_lane_kernel<false>, g, b, lds, s, P);
    return hipGetLastError();
}

hipError_t pscl_launch_gather_rows(const double* llr, int64_t row, const int64_t* act, int64_t n, double* out,
                                   hipStream_t s) {
    if (n <= 0) return hipSuccess;
    int64_t grid = (n * row + 255) / 256;
    if (grid > 65536) grid = 65536;
    hipLaunchKernelGGL(sc_gather_rows_kernel, dim3((unsigned)grid), dim3(256), 0, s, llr, row, act, n, out);
    return hipGetLastError();
}

hipError_t pscl_launch_scatter_results(const int64_t* act, int64_t n, int W, const uint64_t* best_in,
                                       const uint8_t* flags_in, uint64_t* best, uint8_t* flags, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    int64_t grid = (n + 255) / 256;
    if (grid > 4096) grid = 4096;
    hipLaunchKernelGGL(sc_scatter_results_kernel, dim3((unsigned)grid), dim3(256), 0, s, act, n, W, best_in, flags_in,
                       best, flags);
    return hipGetLastError();
}

hipError_t pscl_launch_add_counter(int64_t* counters, int slot, int64_t v, hipStream_t s) {
    hipLaunchKernelGGL(sc_add_counter_kernel, dim3(1), dim3(64), 0, s, counters, slot, v);
    return hipGetLastError();
}

hipError_t pscl_launch_publish_count(const int32_t* count, int64_t* counters, int slot, int32_t* out, hipStream_t s) {
    hipLaunchKernelGGL(sc_publish_count_kernel, dim3(1), dim3(64), 0, s, count, counters, slot, out);
    return hipGetLastError();
}
#endif  // PSCL_SC128_F32_UNIT
