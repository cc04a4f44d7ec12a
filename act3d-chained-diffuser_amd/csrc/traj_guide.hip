// Clearance guidance of trajectory signals (guide_trajectories, compute_trajectory(guide=...)): after a reverse step of the sampler,
// every free waypoint is pushed out of the margin sphere of its nearest observed scene point and pulled towards the midpoint of its
// neighbours, in place, on the normalised signal.  The reference has no guidance term; the cost is the hinge of traj_clearance.hip,
// the cloud is the pcd_obs argument of compute_trajectory, read in place: [B][C][3][n_pix], channel-planar per camera.
//
// World position of a signal row, ONE fp32 expression, contraction off (tg_world):   p = ((x + 1) * 0.5) * (hi - lo) + lo
// -- two roundings before the scale, the bits of DiffusionPlanner.unnormalize_pos.
//
// Two launches.
//   1  traj_guide_partial<RPT>   the scan of traj_points.h (tc_scan_partial, the decomposition of traj_clear_partial) with two
//      differences: the row's position is unnormalised from the signal on load, and the scan is INDEXED -- a lane keeps (best d^2,
//      index of that point), the lowest index among equal distances stays, and the pair goes to ws: d^2 [chunk][b][g][i] floats,
//      then the indices [chunk][b][g][i] ints (2^31 - 1 = no counted point).
//   2  traj_guide_apply          one workgroup per TRAJECTORY (b, g), thread i = row i (L <= 256).  A ballot scan of the mask gives
//      the rank j of a valid row and, through a rank -> row table in LDS, its valid neighbours; all world positions of the
//      trajectory are put into LDS BEFORE any row is written (Jacobi).  Then per row: the minimum over the chunks (strict <
//      over ascending chunks = ascending indices), ONE square root, s* re-read from the scene by its index, and
//          w = push * (margin - d) / d,  u = w * (p - s*)            when 0 < d < margin, else 0
//          v = smooth * ((p_prev + p_next) * 0.5 - p)                when both neighbours exist and are finite, else 0
//          x' = x + (u + v) * (2 / (hi - lo))                        stored per coordinate, and only where the addend is not 0
//      on the free rows: valid, skip_head <= j < n - skip_tail, cond_mask[row][0] == 0, finite world xyz.  Every other byte of
//      the signal keeps its bits.  nearest[b][g][i] = d before the push (+inf on padded rows and without a counted point, NaN where
//      the row's xyz is not finite).
// d^2 is tc_dist2 of traj_clearance.hip.  The minimum is exact and the tie rule total: the result does not depend on the chunking,
// the tile split or the run.  No atomics.
#include "traj_points.h"
#include "../../include/act3d_hip.h"
#include <math.h>

namespace a3d {

constexpr int TG_MAX_L = TC_THREADS;     // traj_guide_apply: one thread per row

__device__ __forceinline__ float tg_world(float x, float lo, float hi) {
#pragma clang fp contract(off)
  return ((x + 1.f) * 0.5f) * (hi - lo) + lo;
}

struct TrajGuideArgs : TrajScan {    // ws: the partial minima, then [n_chunks][B][R] ints: the point's index
  float* traj;                     // [B][G][L][D] signals, xyz of the free rows updated in place
  const unsigned char* cmask;      // [B G][L][D] or NULL
  const float* bounds;             // [2][3]
  float* nearest;                  // [B][R] or NULL
  int D;
  float margin, push, smooth;
  int skip_head, skip_tail;
};

template <int RPT>
__global__ __launch_bounds__(TC_THREADS) void traj_guide_partial(const TrajGuideArgs a) {
  tc_scan_partial<RPT, true, false>(a, [&a](int b, int r, float& x, float& y, float& z) {
    const float* s = a.traj + ((size_t)b * (a.G * a.L) + r) * a.D;
    x = tg_world(s[0], a.bounds[0], a.bounds[3]);
    y = tg_world(s[1], a.bounds[1], a.bounds[4]);
    z = tg_world(s[2], a.bounds[2], a.bounds[5]);
  });
}

__global__ __launch_bounds__(TC_THREADS) void traj_guide_apply(const TrajGuideArgs a) {
  __shared__ int wsum[4];
  __shared__ int row_of[TG_MAX_L];                 // rank among the valid rows -> row
  __shared__ float P[TG_MAX_L][3];                 // world positions of the trajectory before the update
  __shared__ int fin[TG_MAX_L];
  const int t = blockIdx.x, b = t / a.G, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int L = a.L, R = a.G * a.L, i = tid;
  const size_t r = (size_t)t * L + i;              // row of the whole batch: t = b G + g
  const bool valid = i < L && !a.tmask[(size_t)b * L + i];
  const unsigned long long bal = __ballot(valid);
  if (lane == 0) wsum[wave] = __popcll(bal);
  float lo[3], hi[3], x[3] = {0.f, 0.f, 0.f}, p[3] = {0.f, 0.f, 0.f};
#pragma unroll
  for (int k = 0; k < 3; ++k) { lo[k] = a.bounds[k]; hi[k] = a.bounds[3 + k]; }
  float* xrow = a.traj + r * a.D;
  bool finite = false;
  if (valid) {
#pragma unroll
    for (int k = 0; k < 3; ++k) { x[k] = xrow[k]; p[k] = tg_world(x[k], lo[k], hi[k]); }
    finite = tc_finite(p[0]) && tc_finite(p[1]) && tc_finite(p[2]);
  }
  __syncthreads();
  int j = __popcll(bal & ((1ull << lane) - 1ull));
  for (int w = 0; w < wave; ++w) j += wsum[w];
  const int n = wsum[0] + wsum[1] + wsum[2] + wsum[3];
  if (valid) {
    row_of[j] = i;
    P[i][0] = p[0]; P[i][1] = p[1]; P[i][2] = p[2];
    fin[i] = finite ? 1 : 0;
  }
  __syncthreads();
  if (i >= L) return;

  // ---- the nearest counted point: minimum over the chunks, ascending, strict <
  float d2 = INFINITY;
  int idx = TC_NONE;
  if (valid && finite) {
    const size_t plane = (size_t)a.n_chunks * a.B * R;
    for (int c = 0; c < a.n_chunks; ++c) {
      const float d = a.ws[(size_t)c * a.B * R + r];
      if (d < d2) { d2 = d; idx = ((const int*)(a.ws + plane))[(size_t)c * a.B * R + r]; }
    }
  }
  const float d = sqrtf(d2);
  if (a.nearest) a.nearest[r] = valid ? (finite ? d : NAN) : INFINITY;

  bool free_row = valid && finite && j >= a.skip_head && j < n - a.skip_tail;
  if (free_row && a.cmask && a.cmask[r * a.D]) free_row = false;
  if (!free_row) return;

  float add[3] = {0.f, 0.f, 0.f};
  {
#pragma clang fp contract(off)
    if (a.push > 0.f && idx != TC_NONE && d > 0.f && d < a.margin) {
      const long long c = idx / a.n_pix, q = idx - c * a.n_pix;
      const float* s = a.scene + (size_t)b * a.N * 3 + (size_t)c * 3 * a.n_pix + q;
      const float w = a.push * (a.margin - d) / d;
#pragma unroll
      for (int k = 0; k < 3; ++k) add[k] = w * (p[k] - s[(size_t)k * a.n_pix]);
    }
    if (a.smooth > 0.f && j > 0 && j + 1 < n) {
      const int ip = row_of[j - 1], in = row_of[j + 1];
      if (fin[ip] && fin[in]) {
#pragma unroll
        for (int k = 0; k < 3; ++k) add[k] = add[k] + a.smooth * ((P[ip][k] + P[in][k]) * 0.5f - p[k]);
      }
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const float dx = add[k] * (2.f / (hi[k] - lo[k]));
      if (dx != 0.f) xrow[k] = x[k] + dx;          // a zero addend stores nothing: the row keeps its bits (-0 included)
    }
  }
}

}  // namespace a3d

using namespace a3d;

extern "C" size_t a3d_traj_guide_ws_floats(int B, int G, int L, int n_points, int n_chunks) {
  return 2 * tc_ws_plane(B, G, L, n_points, n_chunks);          // the index plane behind the d^2 plane
}

extern "C" int a3d_traj_guide(float* traj, int D, const unsigned char* tmask, const unsigned char* cond_mask, const float* bounds,
                              const float* scene, const unsigned char* scene_mask, int n_cam, int n_pix, float margin, int skip_head,
                              int skip_tail, float push, float smooth, float* nearest, float* ws, int n_chunks, int B, int G, int L,
                              void* stream) {
  const char* me = "a3d_traj_guide";
  TrajGuideArgs a;
  int rpt;
  unsigned blocks;
  int rc = tc_scan_plan(me, traj && tmask && bounds && scene && ws, "traj, tmask, bounds, scene and ws", &a, &rpt, &blocks, tmask, scene,
                        scene_mask, ws, n_cam, n_pix, margin, skip_head, skip_tail, n_chunks, B, G, L);
  if (rc) return rc;
  if (L > TG_MAX_L) { set_error("%s: L=%d exceeds %d rows per trajectory", me, L, TG_MAX_L); return A3D_ERR_ARG; }
  if (D != 9 && D != 10) { set_error("%s: D=%d, signal rows have 9 or 10 channels", me, D); return A3D_ERR_ARG; }
  if (!(push >= 0.f && push <= 1.f) || !(smooth >= 0.f && smooth <= 1.f)) {
    set_error("%s: push and smooth must lie in [0, 1] (push=%g smooth=%g)", me, (double)push, (double)smooth); return A3D_ERR_ARG;
  }
  if (push == 0.f && smooth == 0.f) { set_error("%s: push and smooth are both 0: nothing to do", me); return A3D_ERR_ARG; }
  a.traj = traj; a.cmask = cond_mask; a.bounds = bounds; a.nearest = nearest; a.D = D;
  a.margin = margin; a.push = push; a.smooth = smooth; a.skip_head = skip_head; a.skip_tail = skip_tail;
  hipStream_t s = (hipStream_t)stream;
  rc = tc_scan_launch(me, rpt, blocks, a, s, traj_guide_partial<1>, traj_guide_partial<2>, traj_guide_partial<4>);
  if (rc) return rc;
  hipLaunchKernelGGL(traj_guide_apply, dim3((unsigned)(B * G)), dim3(TC_THREADS), 0, s, a);
  return check_launch(me);
}
