// Scene clearance of sampled trajectory candidates (trajectory_clearance, rank_trajectories(select={"clearance": ...})): the distance
// of every waypoint to the nearest observed scene point, by brute force, and a hinge term per candidate.  The reference has neither
// a ranking nor a collision term (Actioner.predict, online_evaluation/utils_with_rlbench.py:120-230, executes the one trajectory it
// samples); the cloud is the pcd_obs argument of compute_trajectory, read in place: [B][C][3][n_pix], channel-planar per camera.
//
// Two launches.
//   1  traj_clear_partial<RPT>   the scan of traj_points.h (tc_scan_partial: grid point chunk x row tile x scene, 256 threads, lanes
//      own waypoint rows, the chunk's points staged through LDS 512 at a time) on the rows' xyz as stored, keeping the minimum of
//      d^2 alone.  A masked or non-finite point is staged as [+inf 0 0]: its d^2 is +inf for every finite row and fminf drops it.
//      Partial minima go to ws[chunk][b][g][i].
//   2  traj_clear_final          one workgroup per scene: which rows are scored (a scan over the mask), then per row the minimum
//      over the chunks, ONE square root, the hinge; per candidate the mean, T lanes per candidate striding the rows and a fixed
//      xor tree (the shape depends on (G, L) alone).
// d^2 of a pair is fmaf(dz, dz, fmaf(dy, dy, dx * dx)) of the three differences, written out, with contraction off around it: one
// expression, the same bits wherever it is inlined.  The minimum of a set of floats is exact and does not depend on the order, so
// `nearest` does not depend on the chunking, the tile split or the run.  No atomics.
#include "traj_points.h"
#include "../../include/act3d_hip.h"

namespace a3d {

struct TrajClearArgs : TrajScan {    // ws: the partial minima, then [B][L] ints: 1 = scored row
  const float* poses;              // [B][G][L][Dp]
  float* nearest;                  // [B][R] or NULL
  float* clearance;                // [B][G]
  int Dp;
  float margin;
  int skip_head, skip_tail;
};

template <int RPT>
__global__ __launch_bounds__(TC_THREADS) void traj_clear_partial(const TrajClearArgs a) {
  tc_scan_partial<RPT, false>(a, [&a](int b, int r, float& x, float& y, float& z) {
    const float* p = a.poses + ((size_t)b * (a.G * a.L) + r) * a.Dp;
    x = p[0]; y = p[1]; z = p[2];
  });
}

__global__ __launch_bounds__(TC_THREADS) void traj_clear_final(const TrajClearArgs a) {
  __shared__ int wsum[4];
  __shared__ int carry;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int G = a.G, L = a.L, R = G * L;
  const unsigned char* m = a.tmask + (size_t)b * L;
  int* scored = (int*)(a.ws + (size_t)a.n_chunks * a.B * R) + (size_t)b * L;

  // ---- n = valid rows of the scene
  {
    int cnt = 0;
    for (int i = tid; i < L; i += TC_THREADS) cnt += m[i] ? 0 : 1;
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
    if (lane == 0) wsum[wave] = cnt;
    if (tid == 0) carry = 0;
  }
  __syncthreads();
  const int n = wsum[0] + wsum[1] + wsum[2] + wsum[3];
  __syncthreads();
  // ---- rank j of every valid row among the valid rows (256 rows per pass), scored[i] = skip_head <= j < n - skip_tail
  for (int i0 = 0; i0 < L; i0 += TC_THREADS) {
    const int i = i0 + tid;
    const bool valid = i < L && !m[i];
    const unsigned long long bal = __ballot(valid);
    const int before = __popcll(bal & ((1ull << lane) - 1ull));
    if (lane == 0) wsum[wave] = __popcll(bal);
    __syncthreads();
    int j = carry + before;
    for (int w = 0; w < wave; ++w) j += wsum[w];
    if (i < L) scored[i] = (valid && j >= a.skip_head && j < n - a.skip_tail) ? 1 : 0;
    __syncthreads();
    if (tid == 0) carry += wsum[0] + wsum[1] + wsum[2] + wsum[3];
    __syncthreads();
  }
  // scored[] was written with global stores by other threads of this workgroup: the barrier above orders them

  // ---- per candidate: T lanes stride the rows; all candidates in one pass (T G <= 256)
  int T = 64;
  while (T > 1 && T * G > TC_THREADS) T >>= 1;
  const int sub = tid & (T - 1), g = tid / T;
  const bool act = g < G;
  float sum = 0.f;
  int ns = 0, nbad = 0;
  if (act) {
    const float inv = 1.f / a.margin;
    for (int i = sub; i < L; i += T) {
      const size_t r = (size_t)g * L + i;
      float near = INFINITY;
      if (!m[i]) {
        const float* p = a.poses + ((size_t)b * R + r) * a.Dp;
        if (tc_finite(p[0]) && tc_finite(p[1]) && tc_finite(p[2])) {
          float d2 = INFINITY;
          for (int c = 0; c < a.n_chunks; ++c) d2 = fminf(d2, a.ws[((size_t)c * a.B + b) * R + r]);
          near = sqrtf(d2);
        } else {
          near = NAN;
        }
      }
      if (a.nearest) a.nearest[(size_t)b * R + r] = near;
      if (scored[i]) {
        ++ns;
        if (near != near) ++nbad;
        else sum += fmaxf(0.f, a.margin - near) * inv;
      }
    }
  }
  for (int o = T >> 1; o > 0; o >>= 1) {
    sum += __shfl_xor(sum, o, 64);
    ns += __shfl_xor(ns, o, 64);
    nbad += __shfl_xor(nbad, o, 64);
  }
  if (act && sub == 0) a.clearance[(size_t)b * G + g] = nbad > 0 ? NAN : (ns > 0 ? sum / (float)ns : 0.f);
}

}  // namespace a3d

using namespace a3d;

extern "C" size_t a3d_traj_clearance_ws_floats(int B, int G, int L, int n_points, int n_chunks) {
  const size_t plane = tc_ws_plane(B, G, L, n_points, n_chunks);
  return plane ? plane + (size_t)B * L : 0;
}

extern "C" int a3d_traj_clearance(const float* poses, const unsigned char* tmask, const float* scene, const unsigned char* scene_mask,
                                  int n_cam, int n_pix, float margin, int skip_head, int skip_tail, float* nearest, float* clearance,
                                  float* ws, int n_chunks, int B, int G, int L, int Dp, void* stream) {
  const char* me = "a3d_traj_clearance";
  TrajClearArgs a;
  int rpt;
  unsigned blocks;
  int rc = tc_scan_plan(me, poses && tmask && scene && clearance && ws, "poses, tmask, scene, clearance and ws", &a, &rpt, &blocks, tmask,
                        scene, scene_mask, ws, n_cam, n_pix, margin, skip_head, skip_tail, n_chunks, B, G, L);
  if (rc) return rc;
  if (Dp != 7 && Dp != 8) { set_error("%s: Dp=%d, pose rows have 7 or 8 channels", me, Dp); return A3D_ERR_ARG; }
  a.poses = poses; a.nearest = nearest; a.clearance = clearance; a.Dp = Dp;
  a.margin = margin; a.skip_head = skip_head; a.skip_tail = skip_tail;
  hipStream_t s = (hipStream_t)stream;
  rc = tc_scan_launch(me, rpt, blocks, a, s, traj_clear_partial<1>, traj_clear_partial<2>, traj_clear_partial<4>);
  if (rc) return rc;
  hipLaunchKernelGGL(traj_clear_final, dim3(B), dim3(TC_THREADS), 0, s, a);
  return check_launch(me);
}
