// Pinned waypoints of a sampling call: more poses for the in-painting seam every sampler step ends with (out[mask] = cond[mask]).
//
//   a3d_traj_pins   after the call's conditioning tensors exist (a3d_traj_condition, or DiffusionPlanner._condition's op-by-op
//                   block), writes up to P pinned poses per scene into cond_data / cond_mask (and the noisy start trajectory) of
//                   all G candidates of the scene, in ONE launch                      diffusion_model.py:131-168
//
// One workgroup row per scene (blockIdx.x = b), its G trajectories b G + g spread over blockIdx.y, as traj_condition_kernel.  Every
// workgroup counts the scene's padding and converts the scene's P pins into LDS itself (pose_row_to_signal, the row map of
// a3d_pose_to_signal: the same bits), then its threads stride over the L D elements of their trajectories and each thread scans the
// P slots for its OWN element, highest slot first: no two threads write one address, the result does not depend on any order, and
// an element no applied pin selects is not written at all.  Plain loads and stores; nothing is exchanged between workgroups.
#include "a3d_common.h"
#include "pose_signal.h"
#include "../../include/act3d_hip.h"

namespace a3d {

constexpr int TP_MAX = A3D_TRAJ_PINS_MAX;

__global__ __launch_bounds__(256) void traj_pins_kernel(
    const float* __restrict__ poses, int ldp, const int* __restrict__ index, const unsigned char* __restrict__ channels,
    const float* __restrict__ bounds, const unsigned char* __restrict__ tmask, const float* __restrict__ init_noise,
    float* __restrict__ cond_data, unsigned char* __restrict__ cond_mask, float* __restrict__ traj,
    unsigned char* __restrict__ applied, int G, int P, int L, int Dp, int use_goal) {
  __shared__ float s_sig[TP_MAX][TC_MAX_D];
  __shared__ int s_row[TP_MAX];                                   // trajectory row of an applied slot, -1 otherwise
  __shared__ unsigned char s_ch[TP_MAX];
  __shared__ int s_cnt[256];
  const int b = blockIdx.x, t = threadIdx.x, D = Dp + 2;
  const unsigned char* mrow = tmask + (size_t)b * L;
  int cnt = 0;
  for (int l = t; l < L; l += 256) cnt += mrow[l] != 0;
  s_cnt[t] = cnt;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (t < s) s_cnt[t] += s_cnt[t + s];
    __syncthreads();
  }
  const int last = L - s_cnt[0] - 1;                              // the scene's last valid row; -1: the whole row is padding
  if (t < P) {
    const size_t slot = (size_t)b * P + t;
    const int row = index[slot];
    const unsigned char ch = channels[slot] & 7;
    const bool ok = ch != 0 && row >= 1 && row <= (use_goal ? last - 1 : last);
    if (ok) pose_row_to_signal(poses + slot * ldp, bounds, s_sig[t], Dp - 7);
    s_row[t] = ok ? row : -1;
    s_ch[t] = ch;
    if (blockIdx.y == 0) applied[slot] = ok ? 1 : 0;
  }
  __syncthreads();
  const int LD = L * D;
  for (int g = blockIdx.y; g < G; g += gridDim.y) {
    const size_t base = ((size_t)b * G + g) * LD;
    for (int i = t; i < LD; i += 256) {
      const int l = i / D, c = i - l * D;
      const unsigned char bit = c < 3 ? 1 : (c < 9 ? 2 : 4);
      for (int p = P - 1; p >= 0; --p) {                          // the higher slot wins
        if (s_row[p] == l && (s_ch[p] & bit)) {
          const float v = s_sig[p][c];
          const size_t j = base + i;
          cond_data[j] = v;
          cond_mask[j] = 1;
          if (traj) traj[j] = init_noise[j] + v;
          break;
        }
      }
    }
  }
}

}  // namespace a3d

using namespace a3d;

extern "C" int a3d_traj_pins(const float* poses, int ldp, const int* index, const unsigned char* channels, const float* bounds,
                             const unsigned char* tmask, const float* init_noise, float* cond_data, unsigned char* cond_mask,
                             float* traj, unsigned char* applied, int B, int G, int P, int L, int Dp, int use_goal, void* stream) {
  const char* me = "a3d_traj_pins";
  if (!poses || !index || !channels || !bounds || !tmask || !cond_data || !cond_mask || !applied) {
    set_error("%s: null pointer (poses, index, channels, bounds, tmask, cond_data, cond_mask and applied are required)", me);
    return A3D_ERR_ARG;
  }
  if (traj && !init_noise) { set_error("%s: traj needs init_noise (traj = init_noise + the pinned signal)", me); return A3D_ERR_ARG; }
  if (B <= 0 || G <= 0 || L <= 0) { set_error("%s: B, G and L must be positive (B=%d G=%d L=%d)", me, B, G, L); return A3D_ERR_ARG; }
  if (P < 1 || P > TP_MAX) { set_error("%s: P=%d pins per scene, the entry serves 1 to %d", me, P, TP_MAX); return A3D_ERR_ARG; }
  if (Dp < 7 || Dp + 2 > TC_MAX_D) { set_error("%s: Dp=%d must lie in [7, %d]", me, Dp, TC_MAX_D - 2); return A3D_ERR_ARG; }
  if (ldp < Dp) { set_error("%s: the leading dimension ldp=%d is smaller than Dp=%d", me, ldp, Dp); return A3D_ERR_ARG; }
  if ((long long)L * (Dp + 2) > 0x7fffffffLL) { set_error("%s: L * D overflows int (L=%d Dp=%d)", me, L, Dp); return A3D_ERR_ARG; }
  hipLaunchKernelGGL(traj_pins_kernel, dim3(B, G < 64 ? G : 64), dim3(256), 0, (hipStream_t)stream, poses, ldp, index, channels,
                     bounds, tmask, init_noise, cond_data, cond_mask, traj, applied, G, P, L, Dp, use_goal ? 1 : 0);
  return check_launch(me);
}
