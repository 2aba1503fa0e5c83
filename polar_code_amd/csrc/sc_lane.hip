// sc_lane.hip -- lane-parallel successive cancellation of the codes of length N = 32, 64, 256, 512
// and 1024 for gfx950: pscl_sc_device (sc_decode, dl_scl_polar/polar/polar.py:130-168, plus
// check_crc, crc.py:40-56).  N = 128 stays on sc128_lane.hip, whose quad layout this generalises.
//
// Layout.  A frame is decoded by a group of G = max(4, N / 32) consecutive lanes, 64 / G frames
// per wavefront, the whole LLR tree in registers.  Element i of a tree vector of length M >= G
// lives on lane i & (G - 1) of the group, slot i / G: the butterfly partners i and i + M / 2 share
// a lane down to M = 2 G, so those levels are lane-local f/g over M / (2 G) slots.  From M = G
// down the vectors are replicated: a node of M <= G leaves holds element q & (M - 1) on lane q, the
// partner is lane q ^ (M / 2) -- quad_perm (1, 2), half-row mirror of the quad reverse (4),
// row_ror:8 (8), and for the one level that crosses the DPP rows (16, N = 1024) gfx950's
// v_permlane16_swap and a select -- and the leaf value is on every lane: the decisions are
// group-uniform.
// g on the replicated levels flips the sign of whichever operand is `a` on that lane and adds
// (IEEE addition commutes bit for bit).
//
// Partial sums.  A lane-local node returns only the lane's own positions, bit j = x[G j + q]
// (M / G <= 32 bits), so g takes its bit by a compile-time position; the replicated nodes return
// the group-uniform word of M <= G bits.  The decisions of a 32-leaf sub-tree are collected in
// one uniform word and kept by lane S / 32 of the group: u is distributed by word, one VGPR.
//
// The information mask (N bits, wave-uniform) arrives in the kernel arguments (SGPRs); a sub-tree
// without an information bit is skipped by a scalar branch.  The tree is fully unrolled: every
// register index is a compile-time constant, the mask tests are the only branches.
//
// Epilogue.  Lane w looks up the four bytes of u word w in the handle's gather tables (u byte ->
// information bits) and ORs its chunk, at most 32 bits at the bit offset popcount(mask below word
// w), into the frame's information words in LDS (ds_or: the offsets depend on the code); lane t
// then owns information word t (32 bits): its eight syndrome nibbles, the XOR over the group by
// the cross-lane steps, and the store of its half of a `best` word.  Lane 0 stores flags and stage.
//
// Arithmetic is fp64 min, add, compare and sign operations only -- nothing to contract.
#include "scl_device.h"
#include "scl_kernels.h"

using namespace pscl;

namespace {

// lane ^ 16 (N = 1024, the one level across the DPP rows): 1 gfx950's v_permlane16_swap and a
// select; 0 ds_bpermute, as xrow32 of scl_lane.h.  Measured alternately on the (1024,512) rows of
// tools/bench_staged.py, t_sc 1.676-1.693 ms with the swap against 1.695-1.697 ms
#ifndef PSCL_SC_XROW_SWAP
#define PSCL_SC_XROW_SWAP 1
#endif

constexpr int kWavesPerWg = 4;
// workgroups of a launch (they stride over the rest): four per CU of a 256-CU device
constexpr int kScLaneGridCap = 1024;

constexpr int groupLanes(int N) { return N / 32 > 4 ? N / 32 : 4; }

template <int CTRL>
__device__ __forceinline__ uint32_t xdpp32(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_mov_dpp((int)v, CTRL, 0xF, 0xF, true);
}

// the value of lane ^ X (X = 1 .. 16, a power of two)
template <int X>
__device__ __forceinline__ uint32_t lane_xor32(uint32_t v) {
    if constexpr (X == 1) return xdpp32<0xB1>(v);                      // quad_perm [1,0,3,2]
    else if constexpr (X == 2) return xdpp32<0x4E>(v);                 // quad_perm [2,3,0,1]
    else if constexpr (X == 4) return xdpp32<0x141>(xdpp32<0x1B>(v));  // row_half_mirror of quad_perm [3,2,1,0]
    else if constexpr (X == 8) return xdpp32<0x128>(v);                // row_ror:8
#if PSCL_SC_XROW_SWAP
    else {  // the other DPP row by v_permlane16_swap: the rows 1, 3 of one copy against the rows 0, 2 of the other
        const auto r = __builtin_amdgcn_permlane16_swap(v, v, false, false);
        return (threadIdx.x & 16u) ? r[0] : r[1];
    }
#else
    else return (uint32_t)__shfl_xor((int)v, 16);                      // the other DPP row (ds_bpermute)
#endif
}
template <int X>
__device__ __forceinline__ double lane_xor64(double v) {
    const uint64_t u = pscl_asu64(v);
    return pscl_asf64(((uint64_t)lane_xor32<X>((uint32_t)(u >> 32)) << 32) | lane_xor32<X>((uint32_t)u));
}

// v with its sign flipped where bit 31 of s is set (s holds no other bit)
__device__ __forceinline__ double flip_sign31(double v, uint32_t s) {
    const uint64_t u = pscl_asu64(v);
    return pscl_asf64(((uint64_t)((uint32_t)(u >> 32) ^ s) << 32) | (uint32_t)u);
}

template <int N>
struct ScState {
    static constexpr int NW = N >= 64 ? N / 64 : 1;
    uint64_t mask[NW];  // information mask (uniform)
    uint32_t q;         // lane within the group
    uint32_t ub;        // decisions of the current 32-leaf sub-tree (uniform)
    uint32_t uw;        // u word q of the frame (lanes q < N / 32)
};

// does the sub-tree of M leaves from phase S hold an information bit (wave-uniform)
template <int N, int M, int S>
__device__ __forceinline__ bool has_info(const ScState<N>& c) {
    if constexpr (M >= 64) {
        uint64_t w = 0;
#pragma unroll
        for (int k = 0; k < M / 64; ++k) w |= c.mask[S / 64 + k];
        return w != 0ULL;
    } else {
        return ((c.mask[S >> 6] >> (S & 63)) & ((1ULL << M) - 1ULL)) != 0ULL;
    }
}

// the decisions of the 32-leaf sub-tree at phase S, kept by lane S / 32 of the group
// (q made opaque: the lane compares of all N / 32 sub-trees are otherwise hoisted out of the
// frame loop as 64-bit lane masks, which spills SGPRs at N >= 512)
template <int N, int S>
__device__ __forceinline__ void keep_word(ScState<N>& c) {
    uint32_t q = c.q;
    asm volatile("" : "+v"(q));
    c.uw = q == (uint32_t)(S / 32) ? c.ub : c.uw;
}

// node of M <= G leaves from phase S: `in` is element q & (M - 1) of its LLRs; returns the
// node's partial sums, M bits, group-uniform
template <int N, int M, int S>
__device__ __forceinline__ uint32_t sc_rep_node(double in, ScState<N>& c) {
    if constexpr (M == 32) c.ub = 0u;
    uint32_t x;
    if constexpr (M == 1) {
        x = in < 0.0 ? 1u : 0u;  // an information leaf (the callers test the mask): polar.py:152
        c.ub |= x << (S & 31);
    } else {
        constexpr int H = M / 2;
        const double other = lane_xor64<H>(in);
        uint32_t xl = 0, xr = 0;
        if (has_info<N, H, S>(c)) xl = sc_rep_node<N, H, S>(f_minsum(in, other), c);
        if (has_info<N, H, S + H>(c)) {
            // g = b + (1 - 2 x) a with x the partial sum of element q & (H - 1); `a` is the own value
            // on the lanes whose element lies in the lower half
            const uint32_t t = (xl << (31u - (c.q & (uint32_t)(H - 1)))) & 0x80000000u;
            const uint32_t own = (c.q & (uint32_t)H) ? 0u : t;
            xr = sc_rep_node<N, H, S + H>(flip_sign31(in, own) + flip_sign31(other, own ^ t), c);
        }
        x = (xl ^ xr) | (xr << H);
    }
    if constexpr (M == 32) keep_word<N, S>(c);
    return x;
}

// node of M >= 2 G leaves: `in` holds the lane's M / G slots (element G j + q in slot j), both
// butterfly operands of an output on the same lane; returns the lane's own partial sums (bit j:
// element G j + q)
template <int N, int M, int S>
__device__ __forceinline__ uint32_t sc_node(const double (&in)[M / groupLanes(N)], ScState<N>& c) {
    constexpr int G = groupLanes(N), H = M / 2, NS = H / G;
    if constexpr (M == 32) c.ub = 0u;
    uint32_t xl = 0, xr = 0;
    if (has_info<N, H, S>(c)) {
        if constexpr (H == G) {
            xl = (sc_rep_node<N, H, S>(f_minsum(in[0], in[1]), c) >> c.q) & 1u;
        } else {
            double l[NS];
#pragma unroll
            for (int j = 0; j < NS; ++j) l[j] = f_minsum(in[j], in[j + NS]);
            xl = sc_node<N, H, S>(l, c);
        }
    }
    if (has_info<N, H, S + H>(c)) {
        if constexpr (H == G) {
            xr = (sc_rep_node<N, H, S + H>(g_node_wbit(in[0], in[1], xl, 0u), c) >> c.q) & 1u;
        } else {
            double r[NS];
#pragma unroll
            for (int j = 0; j < NS; ++j) r[j] = g_node_wbit(in[j], in[j + NS], xl, (uint32_t)j);
            xr = sc_node<N, H, S + H>(r, c);
        }
    }
    if constexpr (M == 32) keep_word<N, S>(c);
    return (xl ^ xr) | (xr << NS);
}

// XOR of v over the G lanes of each group
template <int G>
__device__ __forceinline__ uint32_t group_xor(uint32_t v) {
    v ^= lane_xor32<1>(v);
    v ^= lane_xor32<2>(v);
    if constexpr (G >= 8) v ^= lane_xor32<4>(v);
    if constexpr (G >= 16) v ^= lane_xor32<8>(v);
    if constexpr (G >= 32) v ^= lane_xor32<16>(v);
    return v;
}

template <int N>
__global__ void __launch_bounds__(kWavesPerWg * 64) sc_lane_kernel(const pscl_scn_params P) {
    constexpr int G = groupLanes(N), SLOTS = N / G, FPW = 64 / G, NWU = N / 32, NW = ScState<N>::NW;
    constexpr int NBY = N > 128 ? N / 8 : 16;  // gather tables the handle uploads
    constexpr int SW = G + 1;                  // staged information words per frame (one past the chunks' reach)
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    // the epilogue tables, once per workgroup
    {
        uint64_t* dst = reinterpret_cast<uint64_t*>(smem);
        for (int i = threadIdx.x; i < P.epi_words; i += blockDim.x) dst[i] = P.epi_table[i];
    }
    __syncthreads();
    const uint8_t* const GT = smem;                                                   // [NBY][256] u byte -> info bits
    const uint32_t* const ST = reinterpret_cast<const uint32_t*>(smem + NBY * 256);  // [K4][16] nibble -> syndrome
    const int K4 = (P.K + 3) / 4, W2 = 2 * P.W;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t* const iwords = reinterpret_cast<uint32_t*>(smem + (size_t)P.epi_words * 8) + (wave * FPW + lane / G) * SW;
    ScState<N> c;
#pragma unroll
    for (int k = 0; k < NW; ++k) c.mask[k] = P.info_mask[k];
    c.q = (uint32_t)lane & (uint32_t)(G - 1);
    const uint32_t q = c.q;
    // this lane's 32-bit word of the information mask and the information bits below it
    uint32_t mw = 0, off = 0;
#pragma unroll
    for (int v = 0; v < NWU; ++v) {
        const uint32_t m32 = (uint32_t)(c.mask[v >> 1] >> (32 * (v & 1)));
        mw = q == (uint32_t)v ? m32 : mw;
        off += q > (uint32_t)v ? (uint32_t)__builtin_popcount(m32) : 0u;
    }
    constexpr int64_t kFramesPerWg = (int64_t)FPW * kWavesPerWg;
    for (int64_t g0 = (int64_t)blockIdx.x * kFramesPerWg + wave * FPW; g0 < P.B; g0 += (int64_t)gridDim.x * kFramesPerWg) {
        const int64_t f = g0 + lane / G;
        const bool valid = f < P.B;
        const double* row = P.llr + (valid ? f : g0) * N;  // (a ragged wave's empty groups decode frame g0 again)
        double ch[SLOTS];
#pragma unroll
        for (int j = 0; j < SLOTS; ++j) ch[j] = row[G * j + (int)q];
        c.uw = 0u;
        c.ub = 0u;
        // (the mask made opaque per iteration: hoisted out of the frame loop, the sub-tree tests
        // would each hold an SGPR across it and spill)
#pragma unroll
        for (int k = 0; k < NW; ++k) asm volatile("" : "+s"(c.mask[k]));
        (void)sc_node<N, N, 0>(ch, c);
        // ---- epilogue: u[info_set] as words, CRC syndrome
        iwords[q] = 0u;
        if (q == 0u) iwords[G] = 0u;
        uint32_t chunk = 0, sh = 0;
        if (NWU >= G || q < (uint32_t)NWU) {
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                chunk |= (uint32_t)GT[(4 * q + t) * 256 + ((c.uw >> (8 * t)) & 255u)] << sh;
                sh += __builtin_popcount((mw >> (8 * t)) & 255u);
            }
        }
        wave_lds_fence();
        {
            // chunk (sh <= 32 bits) at bit `off` of the information vector
            const uint32_t wi = off >> 5, sb = off & 31u;
            const uint32_t hi = sb ? chunk >> (32u - sb) : 0u;
            atomicOr(&iwords[wi], chunk << sb);
            if (hi) atomicOr(&iwords[wi + 1], hi);  // (a set bit there: wi + 1 <= (K - 1) / 32)
        }
        wave_lds_fence();
        const uint32_t iw = iwords[q];
        wave_lds_fence();  // (read before the next iteration clears the words)
        uint32_t syn = 0;
#pragma unroll
        for (int t = 0; t < 8; ++t) {
            const int m = 8 * (int)q + t;
            if (m < K4) syn ^= ST[m * 16 + ((iw >> (4 * t)) & 15u)];
        }
        syn = group_xor<G>(syn);
        const bool pass = syn == 0u;
        if (valid) {
            if ((int)q < W2) reinterpret_cast<uint32_t*>(P.best)[f * W2 + (int)q] = iw;
            if (q == 0u) {
                P.flags[f] = pass ? (uint8_t)PSCL_FLAG_CRC_PASS : (uint8_t)0;
                if (P.stage) P.stage[f] = pass ? (uint8_t)1 : (uint8_t)2;
            }
        }
    }
}

// stage 2 at the frames act[i] (pscl_escalate_device)
__global__ void __launch_bounds__(256) sc_mark_stage_kernel(const int64_t* __restrict__ act, int64_t n,
                                                            uint8_t* __restrict__ stage) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        stage[act[i]] = (uint8_t)2;
}

template <int N>
hipError_t launch(const pscl_scn_params& P, hipStream_t s) {
    hipLaunchKernelGGL(sc_lane_kernel<N>, dim3((unsigned)pscl_scn_lane_grid(P)), dim3(kWavesPerWg * 64),
                       (size_t)pscl_scn_lane_lds(P), s, P);
    return hipGetLastError();
}

}  // namespace

int pscl_scn_lane_available(int N) { return N == 32 || N == 64 || N == 256 || N == 512 || N == 1024; }

// the tables, then the staged information words of the workgroup's frames
int pscl_scn_lane_lds(const pscl_scn_params& P) {
    const int G = groupLanes(P.N);
    return P.epi_words * 8 + kWavesPerWg * (64 / G) * (G + 1) * 4;
}

int64_t pscl_scn_lane_grid(const pscl_scn_params& P) {
    const int fpw = kWavesPerWg * (64 / groupLanes(P.N));
    int64_t grid = (P.B + fpw - 1) / fpw;
    if (grid > kScLaneGridCap) grid = kScLaneGridCap;
    return grid < 1 ? 1 : grid;
}

hipError_t pscl_launch_scn_lane(const pscl_scn_params& P, hipStream_t s) {
    if (P.B <= 0) return hipSuccess;
    switch (P.N) {
        case 32: return launch<32>(P, s);
        case 64: return launch<64>(P, s);
        case 256: return launch<256>(P, s);
        case 512: return launch<512>(P, s);
        case 1024: return launch<1024>(P, s);
        default: return hipErrorInvalidValue;
    }
}

hipError_t pscl_launch_mark_stage(const int64_t* act, int64_t n, uint8_t* stage, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    int64_t grid = (n + 255) / 256;
    if (grid > 4096) grid = 4096;
    hipLaunchKernelGGL(sc_mark_stage_kernel, dim3((unsigned)grid), dim3(256), 0, s, act, n, stage);
    return hipGetLastError();
}
