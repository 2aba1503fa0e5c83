// scl_lane.h -- cross-lane helpers of the lane-per-path screening decoders (scl128_lane.hip,
// scl_lane_long.hip): one lane per list path, G = L lanes per frame, DPP within a frame's lanes.
#ifndef PSCL_SCL_LANE_H
#define PSCL_SCL_LANE_H

#include "scl128_impl.h"

// the one-swap tier between the keep-the-better-children path and the full ranking
#ifndef PSCL_LANE_SWAP
#define PSCL_LANE_SWAP 1
#endif


// plain decodes compute the LLR tree in units of log2 e and the metrics in bits (the tail without its
// two fp32 multiplies, glibc_softplus.h pscl_softplus_tail2); the N = 128 FS retry decodes, whose
// warm-start metrics come from the post pass in nats, keep the natural-log form
#ifndef PSCL_LANE_BITS
#define PSCL_LANE_BITS 1
#endif

// the partial sums of the first rewritten depth's g nodes at the even non-recompute phases resolved
// at compile time from the information set (the plan below; scl128_lane.hip, plain instances)
#ifndef PSCL_LANE_PSPLAN
#define PSCL_LANE_PSPLAN 1
#endif

namespace {

// ---- The partial-sum plan (plain constexpr: no device code, nothing of HIP).
// At an even phase phi with t = phi mod 16 in {2, .., 14} the first rewritten depth is a row of w =
// t & -t g nodes whose sign bits are the in-word Arikan transform of the window u[phi - w, phi): bit k
// of polar_transform8(window) = the xor of the window bits i with (i & k) == k.  Frozen bits are 0,
// so node k's partial sum is the parity of the window over S_k = {i : i an information bit, (i & k)
// == k}, a set known at compile time: empty (the g node is b + a), the single bit decided at phi - 1,
// or a handful of bits, the same set for several nodes.
constexpr int psplan_width(int phi) { return (phi & 15) & -(phi & 15); }
// the information bits of the window, bit i = position phi - w + i (a window never straddles a byte)
constexpr uint32_t psplan_window(uint64_t info0, uint64_t info1, int phi) {
    const int w = psplan_width(phi), lo = phi - w;
    return (uint32_t)((lo >= 64 ? info1 : info0) >> (lo & 63)) & ((1u << w) - 1u);
}
// S_k as a mask of window positions
constexpr uint32_t psplan_set(uint32_t iw, int w, int k) {
    uint32_t s = 0;
    for (int i = 0; i < w; ++i)
        if (((iw >> i) & 1u) && (i & k) == k) s |= 1u << i;
    return s;
}
// polar_transform8 (scl_device.h) restated as a constant expression: the same three stages
constexpr uint32_t psplan_transform8(uint32_t x) {
    x ^= (x >> 1) & 0x55u;
    x ^= (x >> 2) & 0x33u;
    x ^= (x >> 4) & 0x0fu;
    return x;
}
// the proof: for every window value the frozen pattern allows (at most 2^8), the parity of window &
// S_k is bit k of the transform -- a wrong plan fails the build (static_assert at every planned phase)
constexpr bool psplan_proved(uint32_t iw, int w) {
    for (uint32_t v = 0; v < (1u << w); ++v) {
        if (v & ~iw) continue;
        const uint32_t x = psplan_transform8(v);
        for (int k = 0; k < w; ++k) {
            uint32_t par = 0;
            for (uint32_t m = v & psplan_set(iw, w, k); m; m &= m - 1u) par ^= 1u;
            if (par != ((x >> k) & 1u)) return false;
        }
    }
    return true;
}
// Instruction counts of the two forms of such a phase.  Transform form: extract (shift, and), two per
// transform stage (shift, and-xor), two per node (shift to bit 31, xor).  Planned form, as emitted
// (scl128_lane.hip): one shift per information bit of the window (its bit to bit 31), one xor per
// distinct set of two or more bits that the masks are built through -- a set's mask is the mask of
// the set without its lowest bit, xor that bit's, so sets that share their upper bits share the
// work -- and one sign xor per node with a non-empty set.
constexpr int psplan_cost_transform(int w) { return 2 + 2 * (w == 8 ? 3 : w == 4 ? 2 : 1) + 2 * w; }
constexpr int psplan_cost(uint32_t iw, int w) {
    uint32_t seen[64] = {};
    int nseen = 0, cost = 0;
    for (uint32_t m = iw; m; m &= m - 1u) ++cost;
    for (int k = 0; k < w; ++k) {
        uint32_t s = psplan_set(iw, w, k);
        if (s) ++cost;
        for (; s & (s - 1u); s &= s - 1u) {
            bool dup = false;
            for (int j = 0; j < nseen; ++j) dup = dup || seen[j] == s;
            if (!dup) {
                seen[nseen++] = s;
                ++cost;
            }
        }
    }
    return cost;
}
// a phase keeps the transform where the plan is not cheaper (the densest windows of 8)
constexpr bool psplan_planned(uint32_t iw, int w) { return psplan_cost(iw, w) < psplan_cost_transform(w); }
// an information set's totals over the 56 phases: instructions per wavefront with the plan where it
// is cheaper, and the number of phases that keep the transform
constexpr int psplan_total(uint64_t info0, uint64_t info1) {
    int tot = 0;
    for (int phi = 2; phi < 128; phi += 2) {
        if ((phi & 15) == 0) continue;
        const int w = psplan_width(phi);
        const uint32_t iw = psplan_window(info0, info1, phi);
        tot += psplan_planned(iw, w) ? psplan_cost(iw, w) : psplan_cost_transform(w);
    }
    return tot;
}
constexpr int psplan_kept(uint64_t info0, uint64_t info1) {
    int n = 0;
    for (int phi = 2; phi < 128; phi += 2)
        if ((phi & 15) != 0 && !psplan_planned(psplan_window(info0, info1, phi), psplan_width(phi))) ++n;
    return n;
}
// the compiled-in sets (tests/test_lane_psplan_cpu.py restates the count in Python and reads these
// figures from this file: the two cannot drift apart).  The transform form is 672 for any set.
static_assert(psplan_total(0, 0) == 0 && psplan_kept(0, 0) == 0, "no information bit: every node is b + a");
static_assert(psplan_total(kSpecInfo[1][0], kSpecInfo[1][1]) == 270 && psplan_kept(kSpecInfo[1][0], kSpecInfo[1][1]) == 0,
              "partial-sum plan of the (128,64) set");
static_assert(psplan_total(kSpecInfo[2][0], kSpecInfo[2][1]) == 378 && psplan_kept(kSpecInfo[2][0], kSpecInfo[2][1]) == 1 &&
                  !psplan_planned(psplan_window(kSpecInfo[2][0], kSpecInfo[2][1], 120), 8),
              "partial-sum plan of the (128,88) set: phase 120 keeps the transform");

// intra-frame lane permutations of an 8-lane group (DPP controls): quad_perm xor 1, 2, 3, and the
// half-row mirror (lane i <-> 7 - i), which maps one quad onto the other
constexpr int kQX1 = 0xB1, kQX2 = 0x4E, kQX3 = 0x1B, kQID = 0xE4, kHMIR = 0x141;
// the permutation that maps one quad of an 8-lane frame onto the other: row_half_mirror (0x141,
// lane i <-> 7 - i) for frames of 8 consecutive lanes; row_mirror (0x140, lane i <-> 15 - i) for the
// N = 128 kernel's frames of the outer or the inner two quads of a row (scl128_lane.hip)
#ifndef PSCL_LANE_FRAME_MIRROR
#define PSCL_LANE_FRAME_MIRROR 0x141
#endif
constexpr int kFMIR = PSCL_LANE_FRAME_MIRROR;

template <int CTRL>
__device__ __forceinline__ uint32_t dpp32(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_mov_dpp((int)v, CTRL, 0xF, 0xF, true);
}

// rank counts of this lane's two children against the two children of lane pi(this lane):
// rg += [og < kg] + [ob < kg], rb += [og < kb] + [ob < kb], the other lane's keys read through the
// DPP permutation CTRL of og / ob (hand-scheduled: inline asm is not hazard-checked, so the first
// instruction waits out a VALU write of the key registers)
template <int CTRL>
__device__ __forceinline__ void rank_pair(uint32_t og, uint32_t ob, uint32_t kg, uint32_t kb, uint32_t& rg, uint32_t& rb) {
    uint32_t t;
    asm volatile(
        "s_nop 1\n\t"
        "v_sub_co_u32_dpp %0, vcc, %3, %5 quad_perm:[%7,%8,%9,%10] row_mask:0xf bank_mask:0xf\n\t"
        "v_addc_co_u32 %1, vcc, 0, %1, vcc\n\t"
        "v_sub_co_u32_dpp %0, vcc, %4, %5 quad_perm:[%7,%8,%9,%10] row_mask:0xf bank_mask:0xf\n\t"
        "v_addc_co_u32 %1, vcc, 0, %1, vcc\n\t"
        "v_sub_co_u32_dpp %0, vcc, %3, %6 quad_perm:[%7,%8,%9,%10] row_mask:0xf bank_mask:0xf\n\t"
        "v_addc_co_u32 %2, vcc, 0, %2, vcc\n\t"
        "v_sub_co_u32_dpp %0, vcc, %4, %6 quad_perm:[%7,%8,%9,%10] row_mask:0xf bank_mask:0xf\n\t"
        "v_addc_co_u32 %2, vcc, 0, %2, vcc"
        : "=&v"(t), "+v"(rg), "+v"(rb)
        : "v"(og), "v"(ob), "v"(kg), "v"(kb), "i"(CTRL & 3), "i"((CTRL >> 2) & 3), "i"((CTRL >> 4) & 3),
          "i"((CTRL >> 6) & 3)
        : "vcc");
}

// rank counts for the survivor selection (select_survivors): rg += [og < kg] + [ob < kg] (this
// lane's better child against the other lane's two children), rbb += [ob < kb] (its worse child
// against the other lane's worse child), the other lane read through the DPP permutation CTRL
template <int CTRL>
__device__ __forceinline__ void rank3(uint32_t og, uint32_t ob, uint32_t kg, uint32_t kb, uint32_t& rg, uint32_t& rbb) {
    uint32_t t;
    asm volatile(
        "s_nop 1\n\t"
        "v_sub_co_u32_dpp %0, vcc, %3, %5 quad_perm:[%7,%8,%9,%10] row_mask:0xf bank_mask:0xf\n\t"
        "v_addc_co_u32 %1, vcc, 0, %1, vcc\n\t"
        "v_sub_co_u32_dpp %0, vcc, %4, %5 quad_perm:[%7,%8,%9,%10] row_mask:0xf bank_mask:0xf\n\t"
        "v_addc_co_u32 %1, vcc, 0, %1, vcc\n\t"
        "v_sub_co_u32_dpp %0, vcc, %4, %6 quad_perm:[%7,%8,%9,%10] row_mask:0xf bank_mask:0xf\n\t"
        "v_addc_co_u32 %2, vcc, 0, %2, vcc"
        : "=&v"(t), "+v"(rg), "+v"(rbb)
        : "v"(og), "v"(ob), "v"(kg), "v"(kb), "i"(CTRL & 3), "i"((CTRL >> 2) & 3), "i"((CTRL >> 4) & 3),
          "i"((CTRL >> 6) & 3)
        : "vcc");
}

// lane i <-> 15 - i within a row: maps one 8-lane half of a 16-lane frame (G = 16, a whole row)
// onto the other
constexpr int kRMIR = 0x140;

// max / min / sum of v over the G lanes of each frame (G = 4: two quad_perm steps; G = 8: and
// the half-row mirror; G = 16: and the row mirror)
// the other row of a 32-lane frame (G = 32: two rows; DPP does not cross rows)
__device__ __forceinline__ uint32_t xrow32(uint32_t v) { return (uint32_t)__shfl_xor((int)v, 16); }

template <int G>
__device__ __forceinline__ uint32_t frame_max(uint32_t v) {
    uint32_t o = dpp32<kQX1>(v);
    v = o > v ? o : v;
    o = dpp32<kQX2>(v);
    v = o > v ? o : v;
    if constexpr (G >= 8) {
        o = dpp32<G >= 16 ? kHMIR : kFMIR>(v);
        v = o > v ? o : v;
    }
    if constexpr (G >= 16) {
        o = dpp32<kRMIR>(v);
        v = o > v ? o : v;
    }
    if constexpr (G == 32) {
        o = xrow32(v);
        v = o > v ? o : v;
    }
    return v;
}
template <int G>
__device__ __forceinline__ uint32_t frame_min(uint32_t v) {
    uint32_t o = dpp32<kQX1>(v);
    v = o < v ? o : v;
    o = dpp32<kQX2>(v);
    v = o < v ? o : v;
    if constexpr (G >= 8) {
        o = dpp32<G >= 16 ? kHMIR : kFMIR>(v);
        v = o < v ? o : v;
    }
    if constexpr (G >= 16) {
        o = dpp32<kRMIR>(v);
        v = o < v ? o : v;
    }
    if constexpr (G == 32) {
        o = xrow32(v);
        v = o < v ? o : v;
    }
    return v;
}
template <int G>
__device__ __forceinline__ uint32_t frame_sum(uint32_t v) {
    v += dpp32<kQX1>(v);
    v += dpp32<kQX2>(v);
    if constexpr (G >= 8) v += dpp32<G >= 16 ? kHMIR : kFMIR>(v);
    if constexpr (G >= 16) v += dpp32<kRMIR>(v);
    if constexpr (G == 32) v += xrow32(v);
    return v;
}
template <int G>
__device__ __forceinline__ uint32_t frame_or(uint32_t v) {
    v |= dpp32<kQX1>(v);
    v |= dpp32<kQX2>(v);
    if constexpr (G >= 8) v |= dpp32<G >= 16 ? kHMIR : kFMIR>(v);
    if constexpr (G >= 16) v |= dpp32<kRMIR>(v);
    if constexpr (G == 32) v |= xrow32(v);
    return v;
}

// Survivor selection of a full list (the L smallest of each frame's 2L children): this lane's
// better child key kg and worse child key kb (kb >= kg: the worse child pays |llr| more).  Keys are
// counted strictly below, so with distinct keys keep_g / win_b are exact; equal keys can give a
// wrong count, which the caller's certificate (exactly L survivors, margin between the largest
// survivor and the smallest non-survivor) always rejects.
//   PSCL_LANE_RANK3 = 1: rg = #{children below kg} (2L - 2 compares), d = the frame's number of
//     dropped better children, and a worse child survives iff it is among the d smallest worse
//     children (L - 1 compares): 3 compares per lane permutation.
//   0: both children ranked among all 2L (4 compares per permutation).
#ifndef PSCL_LANE_RANK3
#define PSCL_LANE_RANK3 1
#endif
template <int G, int LMAX>
__device__ __forceinline__ void select_survivors(uint32_t kg, uint32_t kb, bool& keep_g, bool& win_b) {
#if PSCL_LANE_RANK3
    uint32_t rg = 0, rbb = 0;
    rank3<kQX1>(kg, kb, kg, kb, rg, rbb);
    rank3<kQX2>(kg, kb, kg, kb, rg, rbb);
    rank3<kQX3>(kg, kb, kg, kb, rg, rbb);
    if constexpr (G >= 8) {  // the other quad of the frame's 8-lane half, through the half-row mirror
        const uint32_t mkg = dpp32<G >= 16 ? kHMIR : kFMIR>(kg), mkb = dpp32<G >= 16 ? kHMIR : kFMIR>(kb);
        rank3<kQID>(mkg, mkb, kg, kb, rg, rbb);
        rank3<kQX1>(mkg, mkb, kg, kb, rg, rbb);
        rank3<kQX2>(mkg, mkb, kg, kb, rg, rbb);
        rank3<kQX3>(mkg, mkb, kg, kb, rg, rbb);
    }
    // the row's other half (G >= 16): the row mirror (lane 15 - i) and the row mirror of the half-row
    // mirror (lane i + 8 or i - 8), each with the quad permutations; G = 32: then the other row's 16
    // lanes, brought over by a bpermute (xor 16), the same way
    auto quads16 = [&](uint32_t ok, uint32_t ob) {
        rank3<kQID>(ok, ob, kg, kb, rg, rbb);
        rank3<kQX1>(ok, ob, kg, kb, rg, rbb);
        rank3<kQX2>(ok, ob, kg, kb, rg, rbb);
        rank3<kQX3>(ok, ob, kg, kb, rg, rbb);
    };
    if constexpr (G >= 16) {
        quads16(dpp32<kRMIR>(kg), dpp32<kRMIR>(kb));
        quads16(dpp32<kRMIR>(dpp32<kHMIR>(kg)), dpp32<kRMIR>(dpp32<kHMIR>(kb)));
    }
    if constexpr (G == 32) {
        const uint32_t xg = xrow32(kg), xb = xrow32(kb);
        quads16(xg, xb);
        quads16(dpp32<kHMIR>(xg), dpp32<kHMIR>(xb));
        quads16(dpp32<kRMIR>(xg), dpp32<kRMIR>(xb));
        quads16(dpp32<kRMIR>(dpp32<kHMIR>(xg)), dpp32<kRMIR>(dpp32<kHMIR>(xb)));
    }
    keep_g = rg < (uint32_t)LMAX;
    const uint32_t d = frame_sum<G>(keep_g ? 0u : 1u);
    win_b = rbb < d;
#else
    static_assert(G <= 8, "the two-rank selection is built for frames of at most 8 lanes");
    uint32_t rg = 0, rb = kg < kb ? 1u : 0u;
    rank_pair<kQX1>(kg, kb, kg, kb, rg, rb);
    rank_pair<kQX2>(kg, kb, kg, kb, rg, rb);
    rank_pair<kQX3>(kg, kb, kg, kb, rg, rb);
    if constexpr (G == 8) {
        const uint32_t mkg = dpp32<kFMIR>(kg), mkb = dpp32<kFMIR>(kb);
        rank_pair<kQID>(mkg, mkb, kg, kb, rg, rb);
        rank_pair<kQX1>(mkg, mkb, kg, kb, rg, rb);
        rank_pair<kQX2>(mkg, mkb, kg, kb, rg, rb);
        rank_pair<kQX3>(mkg, mkb, kg, kb, rg, rb);
    }
    keep_g = rg < (uint32_t)LMAX;
    win_b = rb < (uint32_t)LMAX;
#endif
}

// The rank counts of select_survivors (PSCL_LANE_RANK3 form) for frames of 4 or 8 lanes, as ONE asm
// statement: rg = #{children of the frame's other lanes below kg}, rbb = #{their worse children below
// kb}.  Inline asm is not hazard-checked, and the DPP-read hazard exists only after a VALU write of a
// register a DPP operand reads: kg / kb are written before the statement (one s_nop 1 waits that out),
// and the mirrored keys mkg / mkb (G = 8: the frame's other quad) are written by the statement's own
// second and third instructions, 18 instructions before their first DPP read -- so one wait serves
// all seven permutations (rank3 waits once per permutation).  Nothing else writes a key register
// inside the statement.  The caller forms keep_g, d and win_b (scl128_lane.hip, the plain tier code).
#define PSCL_RANK3_BLK(OG, OB, QP)                                                                  \
    "v_sub_co_u32_dpp %[t], vcc, " OG ", %[kg] quad_perm:" QP " row_mask:0xf bank_mask:0xf\n\t"          \
    "v_addc_co_u32 %[rg], vcc, 0, %[rg], vcc\n\t"                                                         \
    "v_sub_co_u32_dpp %[t], vcc, " OB ", %[kg] quad_perm:" QP " row_mask:0xf bank_mask:0xf\n\t"          \
    "v_addc_co_u32 %[rg], vcc, 0, %[rg], vcc\n\t"                                                         \
    "v_sub_co_u32_dpp %[t], vcc, " OB ", %[kb] quad_perm:" QP " row_mask:0xf bank_mask:0xf\n\t"          \
    "v_addc_co_u32 %[rbb], vcc, 0, %[rbb], vcc\n\t"
#if PSCL_LANE_FRAME_MIRROR == 0x140
#define PSCL_FRAME_MIRROR_DPP "row_mirror"
#else
#define PSCL_FRAME_MIRROR_DPP "row_half_mirror"
#endif
template <int G>
__device__ __forceinline__ void rank_children(uint32_t kg, uint32_t kb, uint32_t& rg, uint32_t& rbb) {
    static_assert(G == 4 || G == 8, "the fused rank counts are built for frames of 4 or 8 lanes");
    uint32_t t;
    rg = 0;
    rbb = 0;
    if constexpr (G == 4) {
        asm volatile("s_nop 1\n\t"
                     PSCL_RANK3_BLK("%[kg]", "%[kb]", "[1,0,3,2]")
                     PSCL_RANK3_BLK("%[kg]", "%[kb]", "[2,3,0,1]")
                     PSCL_RANK3_BLK("%[kg]", "%[kb]", "[3,2,1,0]")
                     : [t] "=&v"(t), [rg] "+v"(rg), [rbb] "+v"(rbb)
                     : [kg] "v"(kg), [kb] "v"(kb)
                     : "vcc");
    } else {
        uint32_t mkg, mkb;
        asm volatile("s_nop 1\n\t"
                     "v_mov_b32_dpp %[mkg], %[kg] " PSCL_FRAME_MIRROR_DPP " row_mask:0xf bank_mask:0xf\n\t"
                     "v_mov_b32_dpp %[mkb], %[kb] " PSCL_FRAME_MIRROR_DPP " row_mask:0xf bank_mask:0xf\n\t"
                     PSCL_RANK3_BLK("%[kg]", "%[kb]", "[1,0,3,2]")
                     PSCL_RANK3_BLK("%[kg]", "%[kb]", "[2,3,0,1]")
                     PSCL_RANK3_BLK("%[kg]", "%[kb]", "[3,2,1,0]")
                     PSCL_RANK3_BLK("%[mkg]", "%[mkb]", "[0,1,2,3]")
                     PSCL_RANK3_BLK("%[mkg]", "%[mkb]", "[1,0,3,2]")
                     PSCL_RANK3_BLK("%[mkg]", "%[mkb]", "[2,3,0,1]")
                     PSCL_RANK3_BLK("%[mkg]", "%[mkb]", "[3,2,1,0]")
                     : [t] "=&v"(t), [rg] "+v"(rg), [rbb] "+v"(rbb), [mkg] "=&v"(mkg), [mkb] "=&v"(mkb)
                     : [kg] "v"(kg), [kb] "v"(kb)
                     : "vcc");
    }
}
#undef PSCL_RANK3_BLK

// position of the j-th set bit (j < popcount(m)) of a mask of at most 32 bits, branch-free
__device__ __forceinline__ uint32_t nth_set_bit16(uint32_t m, uint32_t j);
__device__ __forceinline__ uint32_t nth_set_bit32(uint32_t m, uint32_t j) {
    const uint32_t c16 = __builtin_popcount(m & 0xffffu);
    const bool h16 = j >= c16;
    return (h16 ? 16u : 0u) + nth_set_bit16(h16 ? (m >> 16) : (m & 0xffffu), h16 ? j - c16 : j);
}

// position of the j-th set bit (j < popcount(m)) of a mask of at most 16 bits, branch-free
__device__ __forceinline__ uint32_t nth_set_bit16(uint32_t m, uint32_t j) {
    const uint32_t c8 = __builtin_popcount(m & 255u);
    const bool h8 = j >= c8;
    j = h8 ? j - c8 : j;
    m = h8 ? (m >> 8) : (m & 255u);
    const uint32_t c4 = __builtin_popcount(m & 15u);
    const bool h4 = j >= c4;
    j = h4 ? j - c4 : j;
    m = h4 ? (m >> 4) : (m & 15u);
    const uint32_t c2 = __builtin_popcount(m & 3u);
    const bool h2 = j >= c2;
    j = h2 ? j - c2 : j;
    m = h2 ? (m >> 2) : m;
    const bool h1 = j >= (m & 1u);
    return (h8 ? 8u : 0u) + (h4 ? 4u : 0u) + (h2 ? 2u : 0u) + (h1 ? 1u : 0u);
}

// position of the j-th set bit (j < popcount(m)) of a mask of at most 8 bits, branch-free
__device__ __forceinline__ uint32_t nth_set_bit8(uint32_t m, uint32_t j) {
    const uint32_t c4 = __builtin_popcount(m & 15u);
    const bool h4 = j >= c4;
    j = h4 ? j - c4 : j;
    m = h4 ? (m >> 4) : (m & 15u);
    const uint32_t c2 = __builtin_popcount(m & 3u);
    const bool h2 = j >= c2;
    j = h2 ? j - c2 : j;
    m = h2 ? (m >> 2) : m;
    const bool h1 = j >= (m & 1u);
    return (h4 ? 4u : 0u) + (h2 ? 2u : 0u) + (h1 ? 1u : 0u);
}

// The ranked tier's winner-to-freed-lane matching for frames of 4 or 8 lanes (the plain tier code of
// scl128_lane.hip): the j-th freed lane of a frame pulls the j-th winner, both counted in lane order.
// One packed word per frame, nibble k = the lane of the k-th winner: a winner of path index p ORs in
// p << 4 r, r = its rank among the winners IN LANE ORDER (the set bits of w8 below p -- not its key
// rank rbb: two winners of equal keys can both survive a passing certificate, and rbb would put both
// in one nibble), over the frame's lanes (frame_or); the j-th freed lane reads nibble j.  Whatever the
// two masks hold (a frame being deferred, a keeper's j past the winners) the lane read lies inside
// the frame: the extract keeps log2 G bits.  (nth_set_bit8 above is the FS branch's form.)
// w8 / win: the frame's winner mask and this lane's bit of it; f8: the frame's freed lanes; p: this
// lane's path index; the result is the path index this lane pulls from if it is freed
template <int G>
__device__ __forceinline__ uint32_t matched_winner(uint32_t f8, uint32_t w8, bool win, uint32_t p) {
    static_assert(G == 4 || G == 8, "the packed matching holds one nibble per lane of a frame of 4 or 8");
    const uint32_t below = (1u << p) - 1u;
    const uint32_t j = __builtin_popcount(f8 & below);
    const uint32_t r = __builtin_popcount(w8 & below);
    const uint32_t W = frame_or<G>(win ? p << (4u * r) : 0u);
    return (W >> (4u * j)) & (uint32_t)(G - 1);
}

// The partial-sum plan's sign mask of the set S (window positions, S != 0) from the per-bit masks
// mb[i] (window bit i at bit 31): the mask of S without its lowest bit, xor that bit's.  Equal
// sub-expressions of a phase's sets are one instruction (psplan_cost counts them so).
template <uint32_t S>
__device__ __forceinline__ uint32_t psplan_mask(const uint32_t (&mb)[8]) {
    static_assert(S != 0 && S < 256u, "a non-empty set of window positions");
    if constexpr ((S & (S - 1u)) == 0)
        return mb[__builtin_ctz(S)];
    else
        return psplan_mask<(S & (S - 1u))>(mb) ^ mb[__builtin_ctz(S)];
}

}  // namespace

#endif
