// scl128_lane_rl.hip -- the row-list instances of the lane-per-path screening decoder (scl_lane_kernel<.., RL>,
// pscl_launch_lane_rowlist) as a translation unit of their own: scl128_lane.hip compiled with
// PSCL_LANE_RL_UNIT gives only those.  The code object of the other instances -- bench.py's headline
// kernel among them -- then holds exactly what it held before the row-list form existed.
#define PSCL_LANE_RL_UNIT 1
#include "scl128_lane.hip"
