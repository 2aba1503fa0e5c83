// label_rank.h -- the flip order of the dataset labeller (pscl_label_device, pscl_label_cpu), in one
// place for the device kernel (label.hip) and the host form (scl_cpu.cpp).
//
// make_dataset.py:66,71 of the reference: abs_l0 = |float32(L0)|, order = argsort(abs_l0).  The rule
// here: the decision LLR is narrowed to float32 once (round to nearest even), the sign bit is
// cleared, and candidates are ordered by (that value, information index) -- equal values resolve to
// the LOWER index.  The float32 bits of a non-negative value are monotone in it, so a candidate's key
// is (bits << 32) | index and the order is the keys' ascending order.  (np.argsort's default kind is
// not stable: on ties the reference's order depends on the NumPy build; this rule is the engine's.)
#ifndef PSCL_LABEL_RANK_H
#define PSCL_LABEL_RANK_H

#include <stdint.h>
#include <string.h>

#ifdef __HIPCC__
#define PSCL_LABEL_HD __host__ __device__ inline
#else
#define PSCL_LABEL_HD inline
#endif

#define PSCL_LABEL_MAX_FLIPS 32

// float32 bits of |(float)l0|
PSCL_LABEL_HD uint32_t pscl_label_abs_bits(double l0) {
    const float f = (float)l0;  // round to nearest even, once, before the absolute value
    uint32_t b;
#ifdef __HIP_DEVICE_COMPILE__
    b = (uint32_t)__float_as_uint(f);
#else
    memcpy(&b, &f, 4);
#endif
    return b & 0x7fffffffu;
}

PSCL_LABEL_HD float pscl_label_abs_value(uint32_t bits) {
#ifdef __HIP_DEVICE_COMPILE__
    return __uint_as_float(bits);
#else
    float f;
    memcpy(&f, &bits, 4);
    return f;
#endif
}

PSCL_LABEL_HD uint64_t pscl_label_key(uint32_t abs_bits, int index) { return ((uint64_t)abs_bits << 32) | (uint32_t)index; }
PSCL_LABEL_HD int pscl_label_key_index(uint64_t key) { return (int)(uint32_t)key; }

// Force words of flip.py:30-34 for the flip of information index idx on the bits `base` ([W] words):
// word w of the mask and of the values -- the bits below idx forced to base's, bit idx to its
// complement, the rest free
PSCL_LABEL_HD void pscl_label_force_word(uint64_t base, int w, int idx, uint64_t* mask, uint64_t* value) {
    const int lo = 64 * w;
    if (idx >= lo + 64) {
        *mask = ~0ULL;
        *value = base;
    } else if (idx >= lo) {
        const uint64_t bit = 1ULL << (idx - lo), below = bit - 1ULL;
        *mask = below | bit;
        *value = (base & below) | (~base & bit);
    } else {
        *mask = 0;
        *value = 0;
    }
}

// one thread's form (pscl_label_cpu): abs_out[K] and the T <= K first indices of the order, by repeated
// selection of the smallest remaining key (T <= PSCL_LABEL_MAX_FLIPS, so O(T K))
PSCL_LABEL_HD void pscl_label_rank_host(const double* l0, int K, int T, float* abs_out, int32_t* order) {
    uint64_t last = 0;
    for (int k = 0; k < K; ++k) abs_out[k] = pscl_label_abs_value(pscl_label_abs_bits(l0[k]));
    for (int t = 0; t < T; ++t) {
        uint64_t best = ~0ULL;
        for (int k = 0; k < K; ++k) {
            const uint64_t key = pscl_label_key(pscl_label_abs_bits(l0[k]), k);
            if ((t == 0 || key > last) && key < best) best = key;
        }
        order[t] = pscl_label_key_index(best);
        last = best;
    }
}

#endif
