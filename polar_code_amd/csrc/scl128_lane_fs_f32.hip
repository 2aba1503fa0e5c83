// scl128_lane_fs_f32.hip -- the forced-bit instances of the lane-per-path screening decoder over float32
// rows (scl_lane_fs_kernel_r32<L, 1, true>, pscl_launch_lane_fs_f32: the screened retry rounds of the
// pscl_*_f32 DL-SCL calls) as a translation unit of their own: scl128_lane.hip compiled with
// PSCL_LANE_F32_UNIT and PSCL_LANE_FS_UNIT gives only those.  The code objects of the float64
// instances -- bench.py's headline kernel among them -- hold exactly what they held before.
#define PSCL_LANE_F32_UNIT 1
#define PSCL_LANE_FS_UNIT 1
#include "scl128_lane.hip"
