// scl128_lane_f32.hip -- the plain instances of the lane-per-path screening decoder over float32 rows
// (scl_lane_kernel_f32<..>, pscl_launch_lane_f32) as a translation unit of their own: scl128_lane.hip
// compiled with PSCL_LANE_F32_UNIT gives only those.  The code objects of the float64 instances --
// bench.py's headline kernel among them -- hold exactly what they held before.
#define PSCL_LANE_F32_UNIT 1
#include "scl128_lane.hip"
