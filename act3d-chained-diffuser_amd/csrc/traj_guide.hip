// Clearance guidance of trajectory signals (guide_trajectories, compute_trajectory(guide=...)): after a reverse step of the sampler,
// every free waypoint is pushed out of the margin sphere of its nearest observed scene point and pulled towards the midpoint of its
// neighbours, in place, on the normalised signal.  The reference has no guidance term; the cost is the hinge of traj_clearance.hip,
// the cloud is the pcd_obs argument of compute_trajectory, read in place: [B][C][3][n_pix], channel-planar per camera.
//
// World position of a signal row, ONE fp32 expression, contraction off (tg_world):   p = ((x + 1) * 0.5) * (hi - lo) + lo
// -- two roundings before the scale, the bits of DiffusionPlanner.unnormalize_pos.
//
// Two launches.
//   1  traj_guide_partial<RPT>   the decomposition of traj_clear_partial (point chunk x row tile x scene, lanes own rows, 512 points
//      staged through LDS per pass, dropped points staged as +inf; traj_points.h), with two differences: the row's position is
//      unnormalised from the signal on load, and a lane keeps (best d^2, index of that point), replaced on a strict < while it scans
//      its points in ascending order, so the lowest index among equal distances stays.  Where spare waves split the points of a tile
//      (npg point groups) their pairs meet in LDS and are compared as (d^2, index), lexicographically; the same pair goes to
//      ws: d^2 [chunk][b][g][i] floats, then the indices [chunk][b][g][i] ints (2^31 - 1 = no counted point).
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
#include <limits.h>
#include <math.h>

namespace a3d {

constexpr int TG_MAX_L = TC_THREADS;     // traj_guide_apply: one thread per row
constexpr int TG_NONE = INT_MAX;         // index of "no counted point"

__device__ __forceinline__ float tg_world(float x, float lo, float hi) {
#pragma clang fp contract(off)
  return ((x + 1.f) * 0.5f) * (hi - lo) + lo;
}

struct TrajGuideArgs {
  float* traj;                     // [B][G][L][D] signals, xyz of the free rows updated in place
  const unsigned char* tmask;      // [B][L]
  const unsigned char* cmask;      // [B G][L][D] or NULL
  const float* bounds;             // [2][3]
  const float* scene;              // [B][C][3][n_pix]
  const unsigned char* smask;      // [B][C][n_pix] or NULL
  float* ws;                       // [n_chunks][B][R] partial minima of d^2, then [n_chunks][B][R] ints: the point's index
  float* nearest;                  // [B][R] or NULL
  long long N;                     // points per scene = C * n_pix
  int n_pix, n_chunks, chunk_pts, row_tiles, nrg;
  int B, G, L, D;
  float margin, push, smooth;
  int skip_head, skip_tail;
};

template <int RPT>
__global__ __launch_bounds__(TC_THREADS) void traj_guide_partial(const TrajGuideArgs a) {
  __shared__ f32x4 pts[TC_TILE];
  __shared__ float red[TC_THREADS * RPT];          // [npg][nrg 64 RPT]
  __shared__ int redi[TC_THREADS * RPT];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // blockIdx.x = (b * row_tiles + tile) * n_chunks + chunk
  const int chunk = blockIdx.x % a.n_chunks;
  const int bt = blockIdx.x / a.n_chunks;
  const int tile = bt % a.row_tiles, b = bt / a.row_tiles;
  const int R = a.G * a.L;
  const int nrg = a.nrg, npg = 4 / nrg;
  const int rg = wave % nrg, pg = wave / nrg;
  const int RT = nrg * 64 * RPT;                   // row slots of this tile
  const int slot0 = rg * 64 * RPT + lane;          // this lane's slots: slot0 + 64 k
  const int row_base = tile * (TC_THREADS * RPT);

  float px[RPT], py[RPT], pz[RPT], best[RPT];
  int bidx[RPT];
#pragma unroll
  for (int k = 0; k < RPT; ++k) {
    const int r = row_base + slot0 + 64 * k;
    px[k] = py[k] = pz[k] = 0.f;
    best[k] = INFINITY;
    bidx[k] = TG_NONE;
    if (r < R && !a.tmask[(size_t)b * a.L + r % a.L]) {
      const float* x = a.traj + ((size_t)b * R + r) * a.D;
      px[k] = tg_world(x[0], a.bounds[0], a.bounds[3]);
      py[k] = tg_world(x[1], a.bounds[1], a.bounds[4]);
      pz[k] = tg_world(x[2], a.bounds[2], a.bounds[5]);
    }
  }

  const long long first = (long long)chunk * a.chunk_pts;
  const long long last = min(a.N, first + a.chunk_pts);
  const float* S = a.scene + (size_t)b * a.N * 3;
  const unsigned char* M = a.smask ? a.smask + (size_t)b * a.N : nullptr;
  for (long long base = first; base < last; base += TC_TILE) {
    const int cnt = (int)min((long long)TC_TILE, last - base);
    __syncthreads();                               // the previous pass has read pts
    tc_stage_points(pts, S, M, base, cnt, a.n_pix, tid);
    __syncthreads();
    const int cnt_up = (cnt + 3) & ~3;             // whole groups of 4 points; TC_TILE is a multiple of 4 npg for npg <= 4
    const int n0 = (int)base;                      // N < 2^31: a point's index fits an int
    for (int j = pg * 4; j < cnt_up; j += 4 * npg) {
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const f32x4 s = pts[j + u];
#pragma unroll
        for (int k = 0; k < RPT; ++k) {
          const float d2 = tc_dist2(px[k], py[k], pz[k], s);
          const bool lt = d2 < best[k];            // strict, ascending scan: the lowest index of a tie stays; +inf and NaN never win
          best[k] = lt ? d2 : best[k];
          bidx[k] = lt ? n0 + j + u : bidx[k];
        }
      }
    }
  }

#pragma unroll
  for (int k = 0; k < RPT; ++k) {
    red[pg * RT + slot0 + 64 * k] = best[k];
    redi[pg * RT + slot0 + 64 * k] = bidx[k];
  }
  __syncthreads();
  const size_t plane = (size_t)a.n_chunks * a.B * R;
  float* out = a.ws + ((size_t)chunk * a.B + b) * R;
  int* outi = (int*)(a.ws + plane) + ((size_t)chunk * a.B + b) * R;
  for (int s = tid; s < RT; s += TC_THREADS) {
    float m = red[s];
    int mi = redi[s];
    for (int q = 1; q < npg; ++q) {                // the point groups interleave their indices: (d^2, index) lexicographically
      const float d = red[q * RT + s];
      const int di = redi[q * RT + s];
      if (d < m || (d == m && di < mi)) { m = d; mi = di; }
    }
    const int r = row_base + s;
    if (r < R) { out[r] = m; outi[r] = mi; }
  }
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
  int idx = TG_NONE;
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
    if (a.push > 0.f && idx != TG_NONE && d > 0.f && d < a.margin) {
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
  if (B <= 0 || G <= 0 || L <= 0 || n_points <= 0 || n_chunks < 0) return 0;
  const int c = tc_chunks(B, G, L, n_points, n_chunks);
  return 2 * (size_t)c * B * G * L;
}

extern "C" int a3d_traj_guide(float* traj, int D, const unsigned char* tmask, const unsigned char* cond_mask, const float* bounds,
                              const float* scene, const unsigned char* scene_mask, int n_cam, int n_pix, float margin, int skip_head,
                              int skip_tail, float push, float smooth, float* nearest, float* ws, int n_chunks, int B, int G, int L,
                              void* stream) {
  const char* me = "a3d_traj_guide";
  if (!traj || !tmask || !bounds || !scene || !ws) {
    set_error("%s: null pointer (traj, tmask, bounds, scene and ws are required)", me); return A3D_ERR_ARG;
  }
  if (B <= 0 || G <= 0 || L <= 0) { set_error("%s: B, G and L must be positive (B=%d G=%d L=%d)", me, B, G, L); return A3D_ERR_ARG; }
  if (n_cam <= 0 || n_pix <= 0) { set_error("%s: n_cam and n_pix must be positive (n_cam=%d n_pix=%d)", me, n_cam, n_pix); return A3D_ERR_ARG; }
  if (G > TC_MAX_G) { set_error("%s: G=%d exceeds %d candidates per scene", me, G, TC_MAX_G); return A3D_ERR_ARG; }
  if (L > TG_MAX_L) { set_error("%s: L=%d exceeds %d rows per trajectory", me, L, TG_MAX_L); return A3D_ERR_ARG; }
  if (D != 9 && D != 10) { set_error("%s: D=%d, signal rows have 9 or 10 channels", me, D); return A3D_ERR_ARG; }
  if (!(margin > 0.f && margin <= FLT_MAX)) { set_error("%s: margin must be finite and positive", me); return A3D_ERR_ARG; }
  if (skip_head < 0 || skip_tail < 0) { set_error("%s: negative skip (skip_head=%d skip_tail=%d)", me, skip_head, skip_tail); return A3D_ERR_ARG; }
  if (n_chunks < 0) { set_error("%s: n_chunks=%d is negative (0 = chosen by the entry)", me, n_chunks); return A3D_ERR_ARG; }
  if (!(push >= 0.f && push <= 1.f) || !(smooth >= 0.f && smooth <= 1.f)) {
    set_error("%s: push and smooth must lie in [0, 1] (push=%g smooth=%g)", me, (double)push, (double)smooth); return A3D_ERR_ARG;
  }
  if (push == 0.f && smooth == 0.f) { set_error("%s: push and smooth are both 0: nothing to do", me); return A3D_ERR_ARG; }
  const long long N = (long long)n_cam * n_pix, R = (long long)G * L;
  if (N > 0x7fffffffLL) { set_error("%s: n_cam * n_pix overflows int (n_cam=%d n_pix=%d)", me, n_cam, n_pix); return A3D_ERR_ARG; }
  if (B > 65535) { set_error("%s: B=%d exceeds 65535 scenes per call", me, B); return A3D_ERR_ARG; }
  TrajGuideArgs a;
  a.traj = traj; a.tmask = tmask; a.cmask = cond_mask; a.bounds = bounds; a.scene = scene; a.smask = scene_mask; a.ws = ws;
  a.nearest = nearest;
  a.N = N; a.n_pix = n_pix;
  a.n_chunks = tc_chunks(B, G, L, N, n_chunks);
  a.chunk_pts = (int)((N + a.n_chunks - 1) / a.n_chunks);
  int rpt;
  tc_shape(R, &rpt, &a.nrg, &a.row_tiles);
  a.B = B; a.G = G; a.L = L; a.D = D;
  a.margin = margin; a.push = push; a.smooth = smooth; a.skip_head = skip_head; a.skip_tail = skip_tail;
  const long long blocks = (long long)a.n_chunks * a.row_tiles * B;
  if (blocks > 0x7fffffffLL) { set_error("%s: %lld workgroups (n_chunks=%d) exceed the grid", me, blocks, a.n_chunks); return A3D_ERR_ARG; }
  hipStream_t s = (hipStream_t)stream;
  if (rpt == 1) hipLaunchKernelGGL(traj_guide_partial<1>, dim3((unsigned)blocks), dim3(TC_THREADS), 0, s, a);
  else if (rpt == 2) hipLaunchKernelGGL(traj_guide_partial<2>, dim3((unsigned)blocks), dim3(TC_THREADS), 0, s, a);
  else hipLaunchKernelGGL(traj_guide_partial<4>, dim3((unsigned)blocks), dim3(TC_THREADS), 0, s, a);
  const int rc = check_launch(me);
  if (rc) return rc;
  hipLaunchKernelGGL(traj_guide_apply, dim3((unsigned)(B * G)), dim3(TC_THREADS), 0, s, a);
  return check_launch(me);
}
