// The brute-force pass over a scene cloud that traj_clearance.hip (the nearest distance) and traj_guide.hip (the nearest point) share:
// the decomposition (point chunk x row tile x scene, lanes own rows), the staging of 512 points through LDS, d^2 of a pair, the scan
// itself (tc_scan_partial) and the host side of its launch: the argument checks, the tile split and the chunking (tc_scan_plan).
#pragma once
#include "a3d_common.h"
#include <float.h>
#include <limits.h>

namespace a3d {

constexpr int TC_THREADS = 256;
constexpr int TC_TILE = 512;            // points staged per pass: 8 KB of LDS
constexpr int TC_MAX_G = 64;
constexpr int TC_TARGET_BLOCKS = 512;   // what the entry aims for when it chooses the chunk count (two workgroups per CU)
constexpr int TC_MAX_CHUNKS = 4096;
constexpr int TC_NONE = INT_MAX;        // index of "no counted point"

// what both argument blocks start with: filled by tc_scan_plan, read by tc_scan_partial
struct TrajScan {
  const unsigned char* tmask;      // [B][L]
  const float* scene;              // [B][C][3][n_pix]
  const unsigned char* smask;      // [B][C][n_pix] or NULL
  float* ws;                       // [n_chunks][B][R] partial minima of d^2, then the entry's own tail
  long long N;                     // points per scene = C * n_pix
  int n_pix, n_chunks, chunk_pts, row_tiles, nrg;
  int B, G, L;
};

__device__ __forceinline__ bool tc_finite(float v) { return fabsf(v) <= FLT_MAX; }

__device__ __forceinline__ float tc_dist2(float px, float py, float pz, const f32x4 s) {
#pragma clang fp contract(off)
  const float dx = px - s[0], dy = py - s[1], dz = pz - s[2];
  return fmaf(dz, dz, fmaf(dy, dy, dx * dx));
}

// Points base .. base + cnt - 1 of one scene ([C][3][n_pix], mask [C][n_pix] or NULL) into pts[TC_TILE] as [x y z 0]; a masked or
// non-finite point and every slot past cnt is staged as [+inf 0 0]: the pair loop needs neither a branch nor a tail.  All
// TC_THREADS threads call it between two barriers of their own.
__device__ __forceinline__ void tc_stage_points(f32x4* pts, const float* S, const unsigned char* M, long long base, int cnt, int n_pix,
                                                int tid) {
  for (int j = tid; j < TC_TILE; j += TC_THREADS) {
    f32x4 v = {INFINITY, 0.f, 0.f, 0.f};
    if (j < cnt) {
      const long long n = base + j;
      const long long c = n / n_pix, p = n - c * n_pix;
      const float* s = S + (size_t)c * 3 * n_pix + p;
      const float x = s[0], y = s[n_pix], z = s[2 * (size_t)n_pix];
      const bool ok = tc_finite(x) && tc_finite(y) && tc_finite(z) && !(M && M[n]);
      if (ok) { v[0] = x; v[1] = y; v[2] = z; }
    }
    pts[j] = v;
  }
}

// The whole body of a partial kernel: grid (point chunk x row tile x scene), TC_THREADS threads.  Lanes own rows (RPT rows per lane,
// their running minima of d^2 in registers); pos(b, r, x, y, z) loads the world position of row r of scene b.  A row tile has
// 256 RPT row slots; where a scene has fewer than 4 waves' worth of rows the spare waves take every second / fourth group of 4 points
// of the tile instead (nrg row groups x npg point groups = 4 waves) and the groups' minima meet in LDS.  Partial minima go to
// ws[chunk][b][r].  INDEXED: a lane keeps (best d^2, index of that point), replaced on a strict < while it scans its points in
// ascending order, so the lowest index among equal distances stays; the point groups' pairs are compared as (d^2, index),
// lexicographically, and the indices go to the plane behind the d^2 plane, [chunk][b][r] ints (TC_NONE = no counted point).
template <int RPT, bool INDEXED, class Pos>
__device__ __forceinline__ void tc_scan_partial(const TrajScan& a, Pos pos) {
  __shared__ f32x4 pts[TC_TILE];
  __shared__ float red[TC_THREADS * RPT];          // [npg][nrg 64 RPT]
  __shared__ int redi[INDEXED ? TC_THREADS * RPT : 1];
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
    bidx[k] = TC_NONE;
    if (r < R && !a.tmask[(size_t)b * a.L + r % a.L]) pos(b, r, px[k], py[k], pz[k]);
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
          if constexpr (INDEXED) {
            const bool lt = d2 < best[k];          // strict, ascending scan: the lowest index of a tie stays; +inf and NaN never win
            best[k] = lt ? d2 : best[k];
            bidx[k] = lt ? n0 + j + u : bidx[k];
          } else {
            best[k] = fminf(best[k], d2);          // a dropped point's +inf never wins: no divergent branch
          }
        }
      }
    }
  }

#pragma unroll
  for (int k = 0; k < RPT; ++k) {
    red[pg * RT + slot0 + 64 * k] = best[k];
    if constexpr (INDEXED) redi[pg * RT + slot0 + 64 * k] = bidx[k];
  }
  __syncthreads();
  float* out = a.ws + ((size_t)chunk * a.B + b) * R;
  int* outi = (int*)(a.ws + (size_t)a.n_chunks * a.B * R) + ((size_t)chunk * a.B + b) * R;
  for (int s = tid; s < RT; s += TC_THREADS) {
    float m = red[s];
    int mi = INDEXED ? redi[s] : 0;
    for (int q = 1; q < npg; ++q) {
      const float d = red[q * RT + s];
      if constexpr (INDEXED) {                     // the point groups interleave their indices: (d^2, index) lexicographically
        const int di = redi[q * RT + s];
        if (d < m || (d == m && di < mi)) { m = d; mi = di; }
      } else {
        m = fminf(m, d);
      }
    }
    const int r = row_base + s;
    if (r < R) {
      out[r] = m;
      if constexpr (INDEXED) outi[r] = mi;
    }
  }
}

// row slots per lane and row groups per workgroup for R rows per scene
static inline void tc_shape(long long R, int* rpt, int* nrg, int* row_tiles) {
  *rpt = R <= 256 ? 1 : (R <= 512 ? 2 : 4);
  const long long per_tile = (long long)TC_THREADS * *rpt;
  *row_tiles = (int)((R + per_tile - 1) / per_tile);
  const long long groups = (R + 64LL * *rpt - 1) / (64LL * *rpt);     // waves' worth of rows, one tile when <= 4
  *nrg = groups >= 3 ? 4 : (int)groups;
}

static inline int tc_chunks(int B, int G, int L, long long N, int n_chunks) {
  if (n_chunks > 0) return n_chunks;
  int rpt, nrg, row_tiles;
  tc_shape((long long)G * L, &rpt, &nrg, &row_tiles);
  const long long per = (long long)B * row_tiles;
  long long c = (TC_TARGET_BLOCKS + per - 1) / per;
  const long long by_points = (N + TC_TILE - 1) / TC_TILE;            // a chunk is at least one staged tile
  if (c > by_points) c = by_points;
  if (c > TC_MAX_CHUNKS) c = TC_MAX_CHUNKS;
  return (int)(c < 1 ? 1 : c);
}

// floats of one [n_chunks][B][G L] plane of the workspace (the partial minima of d^2); 0 for sizes no call takes
static inline size_t tc_ws_plane(int B, int G, int L, int n_points, int n_chunks) {
  if (B <= 0 || G <= 0 || L <= 0 || n_points <= 0 || n_chunks < 0) return 0;
  return (size_t)tc_chunks(B, G, L, n_points, n_chunks) * B * G * L;
}

// The host side of a scan: the checks both entries make, under the name `me` of the entry that was called (have_ptrs: its required
// pointers are all there; `required` names them), then the shared fields of the argument block, the row slots per lane (*rpt) and
// the workgroups of the partial launch (*blocks).  Returns A3D_OK or A3D_ERR_ARG with the message set.
static inline int tc_scan_plan(const char* me, bool have_ptrs, const char* required, TrajScan* a, int* rpt, unsigned* blocks,
                               const unsigned char* tmask, const float* scene, const unsigned char* scene_mask, float* ws, int n_cam,
                               int n_pix, float margin, int skip_head, int skip_tail, int n_chunks, int B, int G, int L) {
  if (!have_ptrs) { set_error("%s: null pointer (%s are required)", me, required); return A3D_ERR_ARG; }
  if (B <= 0 || G <= 0 || L <= 0) { set_error("%s: B, G and L must be positive (B=%d G=%d L=%d)", me, B, G, L); return A3D_ERR_ARG; }
  if (n_cam <= 0 || n_pix <= 0) { set_error("%s: n_cam and n_pix must be positive (n_cam=%d n_pix=%d)", me, n_cam, n_pix); return A3D_ERR_ARG; }
  if (G > TC_MAX_G) { set_error("%s: G=%d exceeds %d candidates per scene", me, G, TC_MAX_G); return A3D_ERR_ARG; }
  if (!(margin > 0.f && margin <= FLT_MAX)) { set_error("%s: margin must be finite and positive", me); return A3D_ERR_ARG; }
  if (skip_head < 0 || skip_tail < 0) { set_error("%s: negative skip (skip_head=%d skip_tail=%d)", me, skip_head, skip_tail); return A3D_ERR_ARG; }
  if (n_chunks < 0) { set_error("%s: n_chunks=%d is negative (0 = chosen by the entry)", me, n_chunks); return A3D_ERR_ARG; }
  const long long N = (long long)n_cam * n_pix, R = (long long)G * L;
  if (N > 0x7fffffffLL) { set_error("%s: n_cam * n_pix overflows int (n_cam=%d n_pix=%d)", me, n_cam, n_pix); return A3D_ERR_ARG; }
  if (R * 8 > 0x7fffffffLL) { set_error("%s: G * L * 8 overflows int (G=%d L=%d)", me, G, L); return A3D_ERR_ARG; }
  if (B > 65535) { set_error("%s: B=%d exceeds 65535 scenes per call", me, B); return A3D_ERR_ARG; }
  a->tmask = tmask; a->scene = scene; a->smask = scene_mask; a->ws = ws;
  a->N = N; a->n_pix = n_pix;
  a->n_chunks = tc_chunks(B, G, L, N, n_chunks);
  a->chunk_pts = (int)((N + a->n_chunks - 1) / a->n_chunks);
  tc_shape(R, rpt, &a->nrg, &a->row_tiles);
  a->B = B; a->G = G; a->L = L;
  const long long nb = (long long)a->n_chunks * a->row_tiles * B;
  if (nb > 0x7fffffffLL) { set_error("%s: %lld workgroups (n_chunks=%d) exceed the grid", me, nb, a->n_chunks); return A3D_ERR_ARG; }
  *blocks = (unsigned)nb;
  return A3D_OK;
}

// the partial launch of a plan: k1 / k2 / k4 are the entry's partial kernel for 1, 2 and 4 rows per lane
template <class Args>
static inline int tc_scan_launch(const char* me, int rpt, unsigned blocks, const Args& a, hipStream_t s, void (*k1)(Args),
                                 void (*k2)(Args), void (*k4)(Args)) {
  hipLaunchKernelGGL(rpt == 1 ? k1 : (rpt == 2 ? k2 : k4), dim3(blocks), dim3(TC_THREADS), 0, s, a);
  return check_launch(me);
}

}  // namespace a3d
