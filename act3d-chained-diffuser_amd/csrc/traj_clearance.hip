// Scene clearance of sampled trajectory candidates (trajectory_clearance, rank_trajectories(select={"clearance": ...})): the distance
// of every waypoint to the nearest observed scene point, by brute force, and a hinge term per candidate.  The reference has neither
// a ranking nor a collision term (Actioner.predict, online_evaluation/utils_with_rlbench.py:120-230, executes the one trajectory it
// samples); the cloud is the pcd_obs argument of compute_trajectory, read in place: [B][C][3][n_pix], channel-planar per camera.
//
// Two launches.
//   1  traj_clear_partial<RPT>   grid (point chunk x row tile x scene), 256 threads.  Lanes own waypoint rows (RPT rows per lane, their
//      running minima of d^2 in registers); the chunk's points are staged through LDS 512 at a time as [x y z 0] and read back
//      broadcast (one ds_read_b128 per point and wave: every lane reads the same address).  A masked or non-finite point is staged
//      as [+inf 0 0]: its d^2 is +inf for every finite row and fminf drops it -- no divergent branch in the pair loop.  A row tile
//      has 256 RPT row slots; where a scene has fewer than 4 waves' worth of rows the spare waves take every second / fourth point
//      of the tile instead (nrg row groups x npg point groups = 4 waves) and the groups' minima meet in LDS.  Partial minima go to
//      ws[chunk][b][g][i].
//   2  traj_clear_final          one workgroup per scene: which rows are scored (a scan over the mask), then per row the minimum
//      over the chunks, ONE square root, the hinge; per candidate the mean, T lanes per candidate striding the rows and a fixed
//      xor tree (the shape depends on (G, L) alone).
// d^2 of a pair is fmaf(dz, dz, fmaf(dy, dy, dx * dx)) of the three differences, written out, with contraction off around it: one
// expression, the same bits wherever it is inlined.  The minimum of a set of floats is exact and does not depend on the order, so
// `nearest` does not depend on the chunking, the tile split or the run.  No atomics.
#include "traj_points.h"
#include "../../include/act3d_hip.h"

namespace a3d {

struct TrajClearArgs {
  const float* poses;              // [B][G][L][Dp]
  const unsigned char* tmask;      // [B][L]
  const float* scene;              // [B][C][3][n_pix]
  const unsigned char* smask;      // [B][C][n_pix] or NULL
  float* ws;                       // [n_chunks][B][R] partial minima of d^2, then [B][L] ints: 1 = scored row
  float* nearest;                  // [B][R] or NULL
  float* clearance;                // [B][G]
  long long N;                     // points per scene = C * n_pix
  int n_pix, n_chunks, chunk_pts, row_tiles, nrg;
  int B, G, L, Dp;
  float margin;
  int skip_head, skip_tail;
};

template <int RPT>
__global__ __launch_bounds__(TC_THREADS) void traj_clear_partial(const TrajClearArgs a) {
  __shared__ f32x4 pts[TC_TILE];
  __shared__ float red[TC_THREADS * RPT];          // [npg][nrg 64 RPT]
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
#pragma unroll
  for (int k = 0; k < RPT; ++k) {
    const int r = row_base + slot0 + 64 * k;
    px[k] = py[k] = pz[k] = 0.f;
    best[k] = INFINITY;
    if (r < R && !a.tmask[(size_t)b * a.L + r % a.L]) {
      const float* p = a.poses + ((size_t)b * R + r) * a.Dp;
      px[k] = p[0]; py[k] = p[1]; pz[k] = p[2];
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
    for (int j = pg * 4; j < cnt_up; j += 4 * npg) {
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const f32x4 s = pts[j + u];
#pragma unroll
        for (int k = 0; k < RPT; ++k) best[k] = fminf(best[k], tc_dist2(px[k], py[k], pz[k], s));
      }
    }
  }

#pragma unroll
  for (int k = 0; k < RPT; ++k) red[pg * RT + slot0 + 64 * k] = best[k];
  __syncthreads();
  float* out = a.ws + ((size_t)chunk * a.B + b) * R;
  for (int s = tid; s < RT; s += TC_THREADS) {
    float m = red[s];
    for (int q = 1; q < npg; ++q) m = fminf(m, red[q * RT + s]);
    const int r = row_base + s;
    if (r < R) out[r] = m;
  }
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
  if (B <= 0 || G <= 0 || L <= 0 || n_points <= 0 || n_chunks < 0) return 0;
  const int c = tc_chunks(B, G, L, n_points, n_chunks);
  return (size_t)c * B * G * L + (size_t)B * L;
}

extern "C" int a3d_traj_clearance(const float* poses, const unsigned char* tmask, const float* scene, const unsigned char* scene_mask,
                                  int n_cam, int n_pix, float margin, int skip_head, int skip_tail, float* nearest, float* clearance,
                                  float* ws, int n_chunks, int B, int G, int L, int Dp, void* stream) {
  const char* me = "a3d_traj_clearance";
  if (!poses || !tmask || !scene || !clearance || !ws) {
    set_error("%s: null pointer (poses, tmask, scene, clearance and ws are required)", me); return A3D_ERR_ARG;
  }
  if (B <= 0 || G <= 0 || L <= 0) { set_error("%s: B, G and L must be positive (B=%d G=%d L=%d)", me, B, G, L); return A3D_ERR_ARG; }
  if (n_cam <= 0 || n_pix <= 0) { set_error("%s: n_cam and n_pix must be positive (n_cam=%d n_pix=%d)", me, n_cam, n_pix); return A3D_ERR_ARG; }
  if (G > TC_MAX_G) { set_error("%s: G=%d exceeds %d candidates per scene", me, G, TC_MAX_G); return A3D_ERR_ARG; }
  if (Dp != 7 && Dp != 8) { set_error("%s: Dp=%d, pose rows have 7 or 8 channels", me, Dp); return A3D_ERR_ARG; }
  if (!(margin > 0.f && margin <= FLT_MAX)) { set_error("%s: margin must be finite and positive", me); return A3D_ERR_ARG; }
  if (skip_head < 0 || skip_tail < 0) { set_error("%s: negative skip (skip_head=%d skip_tail=%d)", me, skip_head, skip_tail); return A3D_ERR_ARG; }
  if (n_chunks < 0) { set_error("%s: n_chunks=%d is negative (0 = chosen by the entry)", me, n_chunks); return A3D_ERR_ARG; }
  const long long N = (long long)n_cam * n_pix, R = (long long)G * L;
  if (N > 0x7fffffffLL) { set_error("%s: n_cam * n_pix overflows int (n_cam=%d n_pix=%d)", me, n_cam, n_pix); return A3D_ERR_ARG; }
  if (R * 8 > 0x7fffffffLL) { set_error("%s: G * L * 8 overflows int (G=%d L=%d)", me, G, L); return A3D_ERR_ARG; }
  if (B > 65535) { set_error("%s: B=%d exceeds 65535 scenes per call", me, B); return A3D_ERR_ARG; }
  TrajClearArgs a;
  a.poses = poses; a.tmask = tmask; a.scene = scene; a.smask = scene_mask; a.ws = ws; a.nearest = nearest; a.clearance = clearance;
  a.N = N; a.n_pix = n_pix;
  a.n_chunks = tc_chunks(B, G, L, N, n_chunks);
  a.chunk_pts = (int)((N + a.n_chunks - 1) / a.n_chunks);
  int rpt;
  tc_shape(R, &rpt, &a.nrg, &a.row_tiles);
  a.B = B; a.G = G; a.L = L; a.Dp = Dp;
  a.margin = margin; a.skip_head = skip_head; a.skip_tail = skip_tail;
  const long long blocks = (long long)a.n_chunks * a.row_tiles * B;
  if (blocks > 0x7fffffffLL) { set_error("%s: %lld workgroups (n_chunks=%d) exceed the grid", me, blocks, a.n_chunks); return A3D_ERR_ARG; }
  hipStream_t s = (hipStream_t)stream;
  if (rpt == 1) hipLaunchKernelGGL(traj_clear_partial<1>, dim3((unsigned)blocks), dim3(TC_THREADS), 0, s, a);
  else if (rpt == 2) hipLaunchKernelGGL(traj_clear_partial<2>, dim3((unsigned)blocks), dim3(TC_THREADS), 0, s, a);
  else hipLaunchKernelGGL(traj_clear_partial<4>, dim3((unsigned)blocks), dim3(TC_THREADS), 0, s, a);
  const int rc = check_launch(me);
  if (rc) return rc;
  hipLaunchKernelGGL(traj_clear_final, dim3(B), dim3(TC_THREADS), 0, s, a);
  return check_launch(me);
}
