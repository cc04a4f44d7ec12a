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
//   2  traj_clear_final          one workgroup per scene: which rows are scored (tc_rank_rows, a scan over the mask), then per row
//      the minimum over the chunks, ONE square root, the hinge; per candidate the mean (tc_hinge_mean: T lanes per candidate
//      striding the rows and a fixed xor tree, the shape depends on (G, L) alone).
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
  tc_scan_partial<RPT, false, false>(a, [&a](int b, int r, float& x, float& y, float& z) {
    const float* p = a.poses + ((size_t)b * (a.G * a.L) + r) * a.Dp;
    x = p[0]; y = p[1]; z = p[2];
  });
}

__global__ __launch_bounds__(TC_THREADS) void traj_clear_final(const TrajClearArgs a) {
  const int b = blockIdx.x;
  const int G = a.G, L = a.L, R = G * L;
  const unsigned char* m = a.tmask + (size_t)b * L;
  int* scored = (int*)(a.ws + (size_t)a.n_chunks * a.B * R) + (size_t)b * L;
  // rank j of every valid row among the n valid rows: scored[i] = skip_head <= j < n - skip_tail.  scored[] is written with global
  // stores by other threads of this workgroup: the barrier tc_rank_rows ends with orders them
  tc_rank_rows(m, L, [&](int i, bool valid, int j, int n) { scored[i] = (valid && j >= a.skip_head && j < n - a.skip_tail) ? 1 : 0; });
  tc_hinge_mean(m, scored, a.nearest ? a.nearest + (size_t)b * R : nullptr, a.clearance + (size_t)b * G, G, L, a.margin, [&](int g, int i) {
    const size_t r = (size_t)g * L + i;
    const float* p = a.poses + ((size_t)b * R + r) * a.Dp;
    if (!(tc_finite(p[0]) && tc_finite(p[1]) && tc_finite(p[2]))) return NAN;
    float d2 = INFINITY;
    for (int c = 0; c < a.n_chunks; ++c) d2 = fminf(d2, a.ws[((size_t)c * a.B + b) * R + r]);
    return sqrtf(d2);
  });
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
