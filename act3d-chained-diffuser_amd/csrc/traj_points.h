// What the two brute-force passes over a scene cloud share (traj_clearance.hip: the nearest distance; traj_guide.hip: the nearest
// point): the decomposition (point chunk x row tile x scene, lanes own rows), the staging of 512 points through LDS and d^2 of a pair.
#pragma once
#include "a3d_common.h"
#include <float.h>

namespace a3d {

constexpr int TC_THREADS = 256;
constexpr int TC_TILE = 512;            // points staged per pass: 8 KB of LDS
constexpr int TC_MAX_G = 64;
constexpr int TC_TARGET_BLOCKS = 512;   // what the entry aims for when it chooses the chunk count (two workgroups per CU)
constexpr int TC_MAX_CHUNKS = 4096;

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

}  // namespace a3d
