// The pose -> network-signal row map (diffusion_model.py:187-212), shared by every kernel that converts a pose row: a3d_pose_to_signal,
// a3d_traj_condition (diffusion.hip) and a3d_traj_pins (traj_pins.hip) include this one definition, so that they produce the same bits.
#pragma once
#include <hip/hip_runtime.h>

namespace a3d {

constexpr int TC_MAX_D = 32;                                      // signal channels a workgroup keeps in LDS (D = Dp + 2)

// r: [xyz | quat (w, x, y, z) | extra..], o: [normalised xyz | first two columns of R(normalise(quat)) | extra..]; bounds: [2][3] or NULL
__device__ __forceinline__ void pose_row_to_signal(const float* __restrict__ r, const float* __restrict__ bounds,
                                                   float* __restrict__ o, int extra) {
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    if (bounds) {
      const float lo = bounds[a], hi = bounds[3 + a];
      o[a] = (r[a] - lo) / (hi - lo) * 2.0f - 1.0f;
    } else {
      o[a] = r[a];
    }
  }
  float w = r[3], x = r[4], y = r[5], z = r[6];
  const float nrm = fmaxf(sqrtf(w * w + x * x + y * y + z * z), 1e-10f);
  w /= nrm; x /= nrm; y /= nrm; z /= nrm;
  const float t = 2.0f / (w * w + x * x + y * y + z * z);
  // first column of R, then the second
  o[3] = 1.0f - t * (y * y + z * z);
  o[4] = t * (x * y + z * w);
  o[5] = t * (x * z - y * w);
  o[6] = t * (x * y - z * w);
  o[7] = 1.0f - t * (x * x + z * z);
  o[8] = t * (y * z + x * w);
  for (int e = 0; e < extra; ++e) o[9 + e] = r[7 + e];
}

}  // namespace a3d
