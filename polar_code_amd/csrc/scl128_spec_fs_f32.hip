// scl128_spec_fs_f32.hip -- the exact forced-bit scl128_kernel instances over float32 rows
// (scl128_fs_kernel_r32<..>: scl128_impl.h with PSCL_SCL128_F32 and PSCL_SCL128_F32_FS; r32 for float32
// rows): the retry decode of a DL-SCL round of a compiled-in code at L = 4 or 8 -- entries by bucket
// list, rows by indirection (P.fidx), forced prefixes, warm-started -- as the side chain of a screened
// chain runs it for the (128,64) code and every round of the rate-matched (128,88) code, which has no
// screened retry decode.  The build compiles this file once per (PSCL_SPEC_CODE, PSCL_SPEC_LMAX) pair,
// as scl128_spec_f32.hip; each object defines pscl_launch_spec_fs_f32_<code>_<lmax>.  Objects of their
// own, not a run-time branch: the exact instances are at their register limit.
#define PSCL_SCL128_F32 1
#define PSCL_SCL128_F32_FS 1
#include "scl128_impl.h"

#ifndef PSCL_SPEC_CODE
#error "PSCL_SPEC_CODE (1 or 2) and PSCL_SPEC_LMAX (4 or 8) must be defined"
#endif

#define PSCL_SPEC_CAT2(a, b, c) pscl_launch_spec_fs_f32_##a##_##b
#define PSCL_SPEC_CAT(a, b) PSCL_SPEC_CAT2(a, b, 0)
#define PSCL_SPEC_FN PSCL_SPEC_CAT(PSCL_SPEC_CODE, PSCL_SPEC_LMAX)

// (128,64) decodes read plain channel rows; (128,88) is the NR code, decoded rate matched
hipError_t PSCL_SPEC_FN(const pscl_decode_params& P, int wpg, int64_t grid, int lds, hipStream_t s) {
    constexpr bool CH = PSCL_SPEC_CODE == 2;
    if (!P.f32 || P.apx || !P.force || P.sc_hard || P.L != PSCL_SPEC_LMAX || (P.rm_E != 0) != CH) return hipErrorInvalidValue;
    hipLaunchKernelGGL((scl128_kernel<PSCL_SPEC_LMAX, false, CH, true, PSCL_SPEC_CODE>), dim3((unsigned)grid),
                       dim3(wpg * 64), lds, s, P);
    return hipGetLastError();
}
