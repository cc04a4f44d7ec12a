// The brute-force pass over a scene cloud that traj_clearance.hip (the nearest distance), traj_guide.hip (the nearest point) and
// traj_body.hip (the nearest distance of swept spheres) share: the decomposition (point chunk x row tile x scene, lanes own rows), the
// staging of 512 points through LDS, d^2 of a pair for the two kinds of row (a point, tc_dist2; a segment, tc_seg_dist2), the scan itself
// (tc_scan_partial) and the host side of its launch: the argument checks, the tile split and the chunking (tc_scan_plan); and what the
// one-workgroup-per-scene stages share: the ranks of the valid rows (tc_rank_rows) and the hinge mean per candidate (tc_hinge_mean).
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
  int B, G, L;                     // G: row groups of L rows per scene (candidates, or candidates x spheres)
};

__device__ __forceinline__ bool tc_finite(float v) { return fabsf(v) <= FLT_MAX; }

__device__ __forceinline__ float tc_dist2(float px, float py, float pz, const f32x4 s) {
#pragma clang fp contract(off)
  const float dx = px - s[0], dy = py - s[1], dz = pz - s[2];
  return fmaf(dz, dz, fmaf(dy, dy, dx * dx));
}

// d^2 of a counted point s and the segment a + t d, t in [0, 1]; inv = 1 / |d|^2, or 0 when |d|^2 == 0 (the segment is the point a:
// t is then 0 or 1, w = u either way, and the result has the bits of tc_dist2).  fminf / fmaxf with the constant as the second operand
// return the constant for a NaN t (a dropped point [+inf 0 0] gives inf * 0), so t is always finite and w[0] = +inf - t d[0] = +inf:
// d^2 of a dropped point is +inf, never NaN.
__device__ __forceinline__ float tc_seg_dist2(float ax, float ay, float az, float dx, float dy, float dz, float inv, const f32x4 s) {
#pragma clang fp contract(off)
  const float ux = s[0] - ax, uy = s[1] - ay, uz = s[2] - az;
  const float t = fmaxf(fminf(fmaf(uz, dz, fmaf(uy, dy, ux * dx)) * inv, 1.f), 0.f);
  const float wx = fmaf(-t, dx, ux), wy = fmaf(-t, dy, uy), wz = fmaf(-t, dz, uz);
  return fmaf(wz, wz, fmaf(wy, wy, wx * wx));
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
// their running minima of d^2 in registers); the kind of row is a point, pos(b, r, x, y, z) loads the world position of row r of scene b, or
// (SEGMENT) a segment, pos(b, r, ax, ay, az, dx, dy, dz, inv) loads its start, its direction and 1 / |d|^2: 7 registers per row slot
// instead of 3, tc_seg_dist2 instead of tc_dist2, everything else is shared.  A row tile has
// 256 RPT row slots; where a scene has fewer than 4 waves' worth of rows the spare waves take every second / fourth group of 4 points
// of the tile instead (nrg row groups x npg point groups = 4 waves) and the groups' minima meet in LDS.  Partial minima go to
// ws[chunk][b][r].  INDEXED: a lane keeps (best d^2, index of that point), replaced on a strict < while it scans its points in
// ascending order, so the lowest index among equal distances stays; the point groups' pairs are compared as (d^2, index),
// lexicographically, and the indices go to the plane behind the d^2 plane, [chunk][b][r] ints (TC_NONE = no counted point).
template <int RPT, bool INDEXED, bool SEGMENT, class Pos>
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
  float qx[SEGMENT ? RPT : 1], qy[SEGMENT ? RPT : 1], qz[SEGMENT ? RPT : 1], qi[SEGMENT ? RPT : 1];      // a segment's d and inv
  int bidx[RPT];
#pragma unroll
  for (int k = 0; k < RPT; ++k) {
    const int r = row_base + slot0 + 64 * k;
    px[k] = py[k] = pz[k] = 0.f;
    best[k] = INFINITY;
    bidx[k] = TC_NONE;
    if constexpr (SEGMENT) {
      qx[k] = qy[k] = qz[k] = qi[k] = 0.f;
      if (r < R && !a.tmask[(size_t)b * a.L + r % a.L]) pos(b, r, px[k], py[k], pz[k], qx[k], qy[k], qz[k], qi[k]);
    } else {
      if (r < R && !a.tmask[(size_t)b * a.L + r % a.L]) pos(b, r, px[k], py[k], pz[k]);
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
          float d2;
          if constexpr (SEGMENT) d2 = tc_seg_dist2(px[k], py[k], pz[k], qx[k], qy[k], qz[k], qi[k], s);
          else d2 = tc_dist2(px[k], py[k], pz[k], s);
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

// The ranks of the valid rows of one mask row m[L], by all TC_THREADS threads of a workgroup: returns n = the valid rows and calls
// each(i, valid, j, n) once for every row i < L with j = its rank among the valid rows (meaningless where !valid), 256 rows per pass.
// Ends with a barrier: what each() stored, LDS or global, is ordered for the whole workgroup.
template <class Each>
__device__ __forceinline__ int tc_rank_rows(const unsigned char* m, int L, Each each) {
  __shared__ int wsum[4];
  __shared__ int carry;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
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
  for (int i0 = 0; i0 < L; i0 += TC_THREADS) {
    const int i = i0 + tid;
    const bool valid = i < L && !m[i];
    const unsigned long long bal = __ballot(valid);
    const int before = __popcll(bal & ((1ull << lane) - 1ull));
    if (lane == 0) wsum[wave] = __popcll(bal);
    __syncthreads();
    int j = carry + before;
    for (int w = 0; w < wave; ++w) j += wsum[w];
    if (i < L) each(i, valid, j, n);
    __syncthreads();
    if (tid == 0) carry += wsum[0] + wsum[1] + wsum[2] + wsum[3];
    __syncthreads();
  }
  return n;
}

// The last stage of a clearance entry, by all TC_THREADS threads of the scene's workgroup: near_of(g, i) is the distance of valid row i
// of candidate g (NaN = not finite); nearest ([G][L] of the scene, or NULL) gets it, +inf on the rows m pads; clearance[g] = the mean
// over the rows with scored[i] of max(0, margin - near) / margin, 0 without one, NaN as soon as one is NaN.  T lanes per candidate
// stride the rows, all candidates in one pass (T G <= 256), then a fixed xor tree: the shape depends on (G, L) alone.
template <class Near>
__device__ __forceinline__ void tc_hinge_mean(const unsigned char* m, const int* scored, float* nearest, float* clearance, int G, int L,
                                              float margin, Near near_of) {
  const int tid = threadIdx.x;
  int T = 64;
  while (T > 1 && T * G > TC_THREADS) T >>= 1;
  const int sub = tid & (T - 1), g = tid / T;
  const bool act = g < G;
  float sum = 0.f;
  int ns = 0, nbad = 0;
  if (act) {
    const float inv = 1.f / margin;
    for (int i = sub; i < L; i += T) {
      const size_t r = (size_t)g * L + i;
      float near = INFINITY;
      if (!m[i]) near = near_of(g, i);
      if (nearest) nearest[r] = near;
      if (scored[i]) {
        ++ns;
        if (near != near) ++nbad;
        else sum += fmaxf(0.f, margin - near) * inv;
      }
    }
  }
  for (int o = T >> 1; o > 0; o >>= 1) {
    sum += __shfl_xor(sum, o, 64);
    ns += __shfl_xor(ns, o, 64);
    nbad += __shfl_xor(nbad, o, 64);
  }
  if (act && sub == 0) clearance[g] = nbad > 0 ? NAN : (ns > 0 ? sum / (float)ns : 0.f);
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
                               int n_pix, float margin, int skip_head, int skip_tail, int n_chunks, int B, int G, int L, int K = 1) {
  if (!have_ptrs) { set_error("%s: null pointer (%s are required)", me, required); return A3D_ERR_ARG; }
  if (B <= 0 || G <= 0 || L <= 0) { set_error("%s: B, G and L must be positive (B=%d G=%d L=%d)", me, B, G, L); return A3D_ERR_ARG; }
  if (n_cam <= 0 || n_pix <= 0) { set_error("%s: n_cam and n_pix must be positive (n_cam=%d n_pix=%d)", me, n_cam, n_pix); return A3D_ERR_ARG; }
  if (G > TC_MAX_G) { set_error("%s: G=%d exceeds %d candidates per scene", me, G, TC_MAX_G); return A3D_ERR_ARG; }
  if (!(margin > 0.f && margin <= FLT_MAX)) { set_error("%s: margin must be finite and positive", me); return A3D_ERR_ARG; }
  if (skip_head < 0 || skip_tail < 0) { set_error("%s: negative skip (skip_head=%d skip_tail=%d)", me, skip_head, skip_tail); return A3D_ERR_ARG; }
  if (n_chunks < 0) { set_error("%s: n_chunks=%d is negative (0 = chosen by the entry)", me, n_chunks); return A3D_ERR_ARG; }
  const long long N = (long long)n_cam * n_pix, R = (long long)G * K * L;
  if (N > 0x7fffffffLL) { set_error("%s: n_cam * n_pix overflows int (n_cam=%d n_pix=%d)", me, n_cam, n_pix); return A3D_ERR_ARG; }
  if (R * 8 > 0x7fffffffLL) {
    if (K == 1) set_error("%s: G * L * 8 overflows int (G=%d L=%d)", me, G, L);
    else set_error("%s: G * K * L * 8 overflows int (G=%d K=%d L=%d)", me, G, K, L);
    return A3D_ERR_ARG;
  }
  if (B > 65535) { set_error("%s: B=%d exceeds 65535 scenes per call", me, B); return A3D_ERR_ARG; }
  a->tmask = tmask; a->scene = scene; a->smask = scene_mask; a->ws = ws;
  a->N = N; a->n_pix = n_pix;
  a->n_chunks = tc_chunks(B, G * K, L, N, n_chunks);
  a->chunk_pts = (int)((N + a->n_chunks - 1) / a->n_chunks);
  tc_shape(R, rpt, &a->nrg, &a->row_tiles);
  a->B = B; a->G = G * K; a->L = L;
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
