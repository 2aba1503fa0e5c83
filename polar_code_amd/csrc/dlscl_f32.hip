// dlscl_f32.hip -- the DL-SCL post pass and the decision-LLR replay over float32 rows
// (dl_post_kernel_r32<..> in its wide and narrow forms, replay_kernel_r32; pscl_launch_dl_post_f32,
// pscl_launch_replay_f32) as a translation unit of their own: dlscl.hip compiled with
// PSCL_DLSCL_F32_UNIT gives only those.  The float64 kernels' code object holds exactly what it held
// before.
#define PSCL_DLSCL_F32_UNIT 1
#include "dlscl.hip"
