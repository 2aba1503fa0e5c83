// scl128_spec_f32.hip -- the exact scl128_kernel instances over float32 rows (scl128_kernel_f32<..>,
// scl128_impl.h with PSCL_SCL128_F32): the plain exact decode of a compiled-in code at L = 4 or 8, which
// re-decodes the rows a float32 screening launch deferred (rows by P.fidx, the first *P.d_count of
// them, outputs at their rows).  The build compiles this file once per (PSCL_SPEC_CODE,
// PSCL_SPEC_LMAX) pair, as scl128_spec.hip; each object defines pscl_launch_spec_f32_<code>_<lmax>.
// New instances in objects of their own, not a run-time branch: the exact instances are at their
// register limit.
#define PSCL_SCL128_F32 1
#include "scl128_impl.h"

#ifndef PSCL_SPEC_CODE
#error "PSCL_SPEC_CODE (1 or 2) and PSCL_SPEC_LMAX (4 or 8) must be defined"
#endif

#define PSCL_SPEC_CAT2(a, b, c) pscl_launch_spec_f32_##a##_##b
#define PSCL_SPEC_CAT(a, b) PSCL_SPEC_CAT2(a, b, 0)
#define PSCL_SPEC_FN PSCL_SPEC_CAT(PSCL_SPEC_CODE, PSCL_SPEC_LMAX)

// (128,64) decodes read plain channel rows; (128,88) is the NR code, decoded rate matched
hipError_t PSCL_SPEC_FN(const pscl_decode_params& P, int wpg, int64_t grid, int lds, hipStream_t s) {
    constexpr bool CH = PSCL_SPEC_CODE == 2;
    if (!P.f32 || P.apx || P.force || P.sc_hard || P.L != PSCL_SPEC_LMAX || (P.rm_E != 0) != CH) return hipErrorInvalidValue;
    hipLaunchKernelGGL((scl128_kernel<PSCL_SPEC_LMAX, false, CH, false, PSCL_SPEC_CODE>), dim3((unsigned)grid),
                       dim3(wpg * 64), lds, s, P);
    return hipGetLastError();
}
