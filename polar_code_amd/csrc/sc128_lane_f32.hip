// sc128_lane_f32.hip -- the float32-row instances of the lane-parallel SC stage (sc128_lane_kernel_f32<RM>,
// pscl_launch_sc_lane_f32) and the float32 twin of the row gather, as a translation unit of their own:
// sc128_lane.hip compiled with PSCL_SC128_F32_UNIT gives only those.  The float64 kernels' code object
// holds exactly what it held before.
#define PSCL_SC128_F32_UNIT 1
#include "sc128_lane.hip"
