// Ranking and selection of sampled trajectory candidates (compute_trajectory(num_samples=G, select=...)): one launch, one
// workgroup per scene.  The reference has no ranking: Actioner.predict (online_evaluation/utils_with_rlbench.py:120-230) consumes ONE
// trajectory per scene; the distances follow the conventions of TrajectoryCriterion.compute_metrics (main_trajectory.py:303-343:
// position L2 per step, a sign-invariant quaternion distance, means over the steps of a trajectory).
//
// Terms per candidate (b, g), rows i with tmask[b][i] == 0 only (n = their count):
//   consensus  1 / max(G - 1, 1) * sum_h ( 1 / max(n, 1) * sum_i d(P[b,g,i], P[b,h,i]) ),  d = |p_a - p_b|_2 + rot_weight * rho
//              (a non-finite pair sum with another candidate h != g is left out; the own entry h = g is 0, or NaN)
//   goal       d(P[b,g,i*], goal_b), i* the highest valid row
//   smooth     mean over valid triples (i-1, i, i+1) of |(p_{i+1} - p_i) - (p_i - p_{i-1})|^2
//   length     sum over valid pairs (i, i+1) of |p_{i+1} - p_i|_2
//   bounds     (valid rows with a coordinate outside [lo, hi]) / max(n, 1)
// a3d_traj_rank_extra adds one more term, computed by another launch (the scene clearance of csrc/traj_clearance.hip): extra[b][g],
// weighed by w_extra and added to the score LAST, when and only when w_extra != 0; terms stays [G][5].
// rho(q, r) = 1 - <q, r>^2 for unit quaternions, evaluated by Lagrange's identity as sum_{i<j} (q_i r_j - q_j r_i)^2: the same
// number, an exact 0 for bit-identical rows (no cancellation against 1), relative instead of absolute accuracy near identical rotations.
//
// LDS (dynamic, floats): D [G][G] pair sums | terms [G][5] | score [G] | 16 words of reduction scratch | the scene's candidates
// [G][cstride] as 7 floats per row (xyz, unit quaternion), cstride = (7 L) | 1 (odd: lanes that differ in the candidate hit
// different banks).  G = L = 64: 16 KB + 1.6 KB + 112.25 KB = 129.8 KB of the 160 KB a gfx950 workgroup may hold.  Where that does
// not fit (7 G L floats above ~142 KB) the candidates are read through L2 and normalised on the fly: same arithmetic, same bits.
// d is symmetric, so a pair sum is formed once for h <= g and stored at both places.
// Every reduction has a fixed shape that depends on (G, L) alone: lanes stride over rows, xor-shuffle trees over a power-of-two lane
// group, serial sums in index order over candidates.  No atomics; nothing depends on the grid.
#include "a3d_common.h"
#include "../../include/act3d_hip.h"
#include <float.h>

namespace a3d {

constexpr int TR_THREADS = 256;
constexpr int TR_MAX_G = 64;
constexpr int TR_LDS_CAP = 160 * 1024;

__device__ __forceinline__ void tr_unit_quat(const float* __restrict__ q, float* __restrict__ r) {
  const float den = fmaxf(sqrtf(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]), 1e-10f);
#pragma unroll
  for (int c = 0; c < 4; ++c) r[c] = q[c] / den;
}

// row i of candidate g as [xyz | unit quaternion]: from the staged copy, or from global memory
template <bool STAGED>
__device__ __forceinline__ void tr_row(const float* __restrict__ stage, int cstride, const float* __restrict__ P, int L, int Dp,
                                       int g, int i, float* __restrict__ r) {
  if (STAGED) {
    const float* s = stage + (size_t)g * cstride + i * 7;
#pragma unroll
    for (int c = 0; c < 7; ++c) r[c] = s[c];
  } else {
    const float* p = P + ((size_t)g * L + i) * Dp;
    r[0] = p[0]; r[1] = p[1]; r[2] = p[2];
    tr_unit_quat(p + 3, r + 3);
  }
}
template <bool STAGED>
__device__ __forceinline__ void tr_pos(const float* __restrict__ stage, int cstride, const float* __restrict__ P, int L, int Dp,
                                       int g, int i, float* __restrict__ r) {
  const float* s = STAGED ? stage + (size_t)g * cstride + i * 7 : P + ((size_t)g * L + i) * Dp;
  r[0] = s[0]; r[1] = s[1]; r[2] = s[2];
}

// pose distance of two [xyz | unit quaternion] rows.  The six 2x2 minors are formed without contraction: a fused
// q_i r_j - q_j r_i would round one product only and leave a residue between bit-identical rows.
__device__ __forceinline__ float tr_dist(const float* __restrict__ a, const float* __restrict__ b, float rot_weight) {
  const float dx = a[0] - b[0], dy = a[1] - b[1], dz = a[2] - b[2];
  const float pos = sqrtf(dx * dx + dy * dy + dz * dz);
  float rho = 0.f;
  {
#pragma clang fp contract(off)
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = i + 1; j < 4; ++j) {
        const float m = a[3 + i] * b[3 + j] - a[3 + j] * b[3 + i];
        rho = rho + m * m;
      }
  }
  return pos + rot_weight * rho;
}

// sum over the T consecutive lanes of a group (T a power of two <= 64, groups aligned): a fixed xor tree
__device__ __forceinline__ float tr_group_sum(float v, int T) {
  for (int o = T >> 1; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ int tr_group_sum(int v, int T) {
  for (int o = T >> 1; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

struct TrajRankArgs {
  const float* poses;            // [B][G][L][Dp]
  const unsigned char* tmask;    // [B][L]
  const float* goal;             // [B] rows of ldg floats, or NULL
  const float* bounds;           // [2][3] or NULL
  int* best;                     // [B]
  int* order;                    // [B][G] or NULL
  float* scores;                 // [B][G] or NULL
  float* terms;                  // [B][G][5] or NULL
  float* selected;               // [B][L][Dp] or NULL
  const float* extra;            // [B][G] or NULL: a term computed elsewhere (a3d_traj_rank_extra), added last with weight w_extra
  float w[5];
  float rot_weight, w_extra;
  int ldg, G, L, Dp, cstride;
};

template <bool STAGED>
__global__ __launch_bounds__(TR_THREADS) void traj_rank_kernel(const TrajRankArgs a) {
  extern __shared__ float tr_lds[];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int G = a.G, L = a.L, Dp = a.Dp, cstride = a.cstride;
  float* Dm = tr_lds;                         // [G][G]
  float* tbuf = Dm + G * G;                   // [G][5]
  float* sc = tbuf + G * 5;                   // [G]
  int* red = (int*)(sc + G);                  // [16]: 0-3 valid-row counts per wave, 4-7 highest valid row per wave, 8 best
  float* stage = (float*)(red + 16);          // [G][cstride]
  const float* P = a.poses + (size_t)b * G * L * Dp;
  const unsigned char* m = a.tmask + (size_t)b * L;

  // ---- valid rows: count and highest index (integers: any order gives the same result)
  {
    int cnt = 0, hi = -1;
    for (int i = tid; i < L; i += TR_THREADS)
      if (!m[i]) { ++cnt; hi = i; }
    for (int o = 32; o > 0; o >>= 1) {
      cnt += __shfl_xor(cnt, o, 64);
      hi = max(hi, __shfl_xor(hi, o, 64));
    }
    if ((tid & 63) == 0) { red[tid >> 6] = cnt; red[4 + (tid >> 6)] = hi; }
  }
  if (STAGED) {
    for (int r = tid; r < G * L; r += TR_THREADS) {
      const int g = r / L, i = r - g * L;
      const float* p = P + (size_t)r * Dp;
      float* s = stage + (size_t)g * cstride + i * 7;
      s[0] = p[0]; s[1] = p[1]; s[2] = p[2];
      tr_unit_quat(p + 3, s + 3);
    }
  }
  __syncthreads();
  const int n = red[0] + red[1] + red[2] + red[3];
  const int istar = max(max(red[4], red[5]), max(red[6], red[7]));
  const float nf = (float)max(n, 1);

  // ---- pair sums D[g][h] = D[h][g] = (sum over valid rows of d) / max(n, 1) for h <= g (d is symmetric): T lanes per pair,
  //      256 / T pairs per pass; pair k = g (g + 1) / 2 + h
  {
    const int npair = G * (G + 1) / 2;
    int T = 64;
    while (T > 1 && T * npair > TR_THREADS) T >>= 1;
    const int per_pass = TR_THREADS / T, sub = tid & (T - 1), grp = tid / T;
    for (int base = 0; base < npair; base += per_pass) {
      const int pair = base + grp;
      const bool act = pair < npair;
      int g = 0, h = 0;
      float s = 0.f;
      if (act) {
        g = (int)((sqrtf(8.f * (float)pair + 1.f) - 1.f) * 0.5f);
        while (g * (g + 1) / 2 > pair) --g;                  // the float root may be off by one either way
        while ((g + 1) * (g + 2) / 2 <= pair) ++g;
        h = pair - g * (g + 1) / 2;
        for (int i = sub; i < L; i += T) {
          if (m[i]) continue;
          float x[7], y[7];
          tr_row<STAGED>(stage, cstride, P, L, Dp, g, i, x);
          tr_row<STAGED>(stage, cstride, P, L, Dp, h, i, y);
          s += tr_dist(x, y, a.rot_weight);
        }
      }
      s = tr_group_sum(s, T);
      if (act && sub == 0) { Dm[g * G + h] = s / nf; Dm[h * G + g] = s / nf; }
    }
  }
  __syncthreads();

  // ---- the five terms and the score of candidate g: T lanes per candidate, all candidates in one pass (T G <= 256)
  {
    int T = 64;
    while (T > 1 && T * G > TR_THREADS) T >>= 1;
    const int sub = tid & (T - 1), g = tid / T;
    const bool act = g < G;
    float sm = 0.f, len = 0.f;
    int ntri = 0, nout = 0;
    if (act) {
      float lo[3] = {0.f, 0.f, 0.f}, hi[3] = {0.f, 0.f, 0.f};
      if (a.bounds) {
#pragma unroll
        for (int c = 0; c < 3; ++c) { lo[c] = a.bounds[c]; hi[c] = a.bounds[3 + c]; }
      }
      for (int i = sub; i < L; i += T) {
        if (m[i]) continue;
        float p1[3];
        tr_pos<STAGED>(stage, cstride, P, L, Dp, g, i, p1);
        if (a.bounds && (p1[0] < lo[0] || p1[0] > hi[0] || p1[1] < lo[1] || p1[1] > hi[1] || p1[2] < lo[2] || p1[2] > hi[2])) ++nout;
        if (i + 1 < L && !m[i + 1]) {
          float p2[3];
          tr_pos<STAGED>(stage, cstride, P, L, Dp, g, i + 1, p2);
          const float fx = p2[0] - p1[0], fy = p2[1] - p1[1], fz = p2[2] - p1[2];
          len += sqrtf(fx * fx + fy * fy + fz * fz);
          if (i >= 1 && !m[i - 1]) {
            float p0[3];
            tr_pos<STAGED>(stage, cstride, P, L, Dp, g, i - 1, p0);
            const float ax = fx - (p1[0] - p0[0]), ay = fy - (p1[1] - p0[1]), az = fz - (p1[2] - p0[2]);
            sm += ax * ax + ay * ay + az * az;
            ++ntri;
          }
        }
      }
    }
    sm = tr_group_sum(sm, T);
    len = tr_group_sum(len, T);
    ntri = tr_group_sum(ntri, T);
    nout = tr_group_sum(nout, T);
    if (act && sub == 0) {
      // index order; h = g adds an exact 0 (NaN for a non-finite candidate, which keeps it last); a non-finite pair sum with
      // ANOTHER candidate is left out, so one NaN candidate does not take its whole scene with it
      float cons = 0.f;
      for (int h = 0; h < G; ++h) {
        const float v = Dm[g * G + h];
        if (h == g || fabsf(v) <= FLT_MAX) cons += v;
      }
      cons = cons / (float)max(G - 1, 1);
      float goal = 0.f;
      if (a.goal && n > 0) {
        float x[7], y[7];
        tr_row<STAGED>(stage, cstride, P, L, Dp, g, istar, x);
        const float* gr = a.goal + (size_t)b * a.ldg;
        y[0] = gr[0]; y[1] = gr[1]; y[2] = gr[2];
        tr_unit_quat(gr + 3, y + 3);
        goal = tr_dist(x, y, a.rot_weight);
      }
      const float t[5] = {cons, goal, ntri > 0 ? sm / (float)ntri : 0.f, len, a.bounds ? (float)nout / nf : 0.f};
      float s = 0.f;
#pragma unroll
      for (int k = 0; k < 5; ++k) { tbuf[g * 5 + k] = t[k]; s += a.w[k] * t[k]; }
      if (a.w_extra != 0.f) s += a.w_extra * a.extra[(size_t)b * G + g];   // only when weighed: 0 * NaN would spoil the score
      sc[g] = fabsf(s) <= FLT_MAX ? s : INFINITY;          // NaN and +-inf rank last
    }
  }
  __syncthreads();

  // ---- stable ascending rank; rank 0 is the selected candidate
  if (tid < G) {
    const float s = sc[tid];
    int rank = 0;
    for (int h = 0; h < G; ++h) {
      const float o = sc[h];
      rank += (o < s || (o == s && h < tid)) ? 1 : 0;
    }
    if (a.order) a.order[(size_t)b * G + rank] = tid;
    if (a.scores) a.scores[(size_t)b * G + tid] = s;
    if (rank == 0) { red[8] = tid; a.best[b] = tid; }
  }
  if (a.terms)
    for (int k = tid; k < G * 5; k += TR_THREADS) a.terms[(size_t)b * G * 5 + k] = tbuf[k];
  if (a.selected) {
    __syncthreads();
    const float* src = P + (size_t)red[8] * L * Dp;
    float* dst = a.selected + (size_t)b * L * Dp;
    for (int k = tid; k < L * Dp; k += TR_THREADS) dst[k] = src[k];
  }
}

}  // namespace a3d

using namespace a3d;

static int traj_rank_launch(const char* me, const float* poses, const unsigned char* tmask, const float* goal, int ldg,
                            const float* bounds, float w_consensus, float w_goal, float w_smooth, float w_length, float w_bounds,
                            float rot_weight, int* best, int* order, float* scores, float* terms, float* selected, int B, int G, int L,
                            int Dp, const float* extra, float w_extra, void* stream) {
  if (!poses || !tmask || !best) { set_error("%s: null pointer (poses, tmask and best are required)", me); return A3D_ERR_ARG; }
  if (B <= 0 || G <= 0 || L <= 0) { set_error("%s: B, G and L must be positive (B=%d G=%d L=%d)", me, B, G, L); return A3D_ERR_ARG; }
  if (G > TR_MAX_G) { set_error("%s: G=%d exceeds %d candidates per scene", me, G, TR_MAX_G); return A3D_ERR_ARG; }
  if (Dp != 7 && Dp != 8) { set_error("%s: Dp=%d, pose rows have 7 or 8 channels", me, Dp); return A3D_ERR_ARG; }
  if (goal && ldg < 7) { set_error("%s: goal leading dimension %d is below 7", me, ldg); return A3D_ERR_ARG; }
  const float w[5] = {w_consensus, w_goal, w_smooth, w_length, w_bounds};
  for (int k = 0; k < 5; ++k)
    if (!(w[k] >= 0.f && w[k] <= FLT_MAX)) { set_error("%s: weight %d is negative or not finite", me, k); return A3D_ERR_ARG; }
  if (!(fabsf(rot_weight) <= FLT_MAX)) { set_error("%s: rot_weight is not finite", me); return A3D_ERR_ARG; }
  if (w_goal != 0.f && !goal) { set_error("%s: a goal weight without a goal", me); return A3D_ERR_ARG; }
  if (!(w_extra >= 0.f && w_extra <= FLT_MAX)) { set_error("%s: the extra weight is negative or not finite", me); return A3D_ERR_ARG; }
  if (w_extra != 0.f && !extra) { set_error("%s: an extra weight without an extra term", me); return A3D_ERR_ARG; }
  if (w_bounds != 0.f && !bounds) { set_error("%s: a bounds weight without bounds", me); return A3D_ERR_ARG; }
  if ((long long)G * L * 8 > 0x7fffffffLL) { set_error("%s: G * L * 8 overflows int (G=%d L=%d)", me, G, L); return A3D_ERR_ARG; }
  TrajRankArgs a;
  a.poses = poses; a.tmask = tmask; a.goal = goal; a.bounds = bounds;
  a.best = best; a.order = order; a.scores = scores; a.terms = terms; a.selected = selected;
  for (int k = 0; k < 5; ++k) a.w[k] = w[k];
  a.rot_weight = rot_weight; a.extra = extra; a.w_extra = w_extra;
  a.ldg = goal ? ldg : 0; a.G = G; a.L = L; a.Dp = Dp;
  a.cstride = (7 * L) | 1;
  const size_t fixed = ((size_t)G * G + (size_t)G * 6 + 16) * sizeof(float);
  const size_t staged = fixed + (size_t)G * a.cstride * sizeof(float);
  if (staged <= (size_t)TR_LDS_CAP) {
    static bool once = false;
    if (!once) { (void)hipFuncSetAttribute((const void*)traj_rank_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, TR_LDS_CAP); once = true; }
    hipLaunchKernelGGL(traj_rank_kernel<true>, dim3(B), dim3(TR_THREADS), staged, (hipStream_t)stream, a);
  } else {
    hipLaunchKernelGGL(traj_rank_kernel<false>, dim3(B), dim3(TR_THREADS), fixed, (hipStream_t)stream, a);
  }
  return check_launch(me);
}

extern "C" int a3d_traj_rank(const float* poses, const unsigned char* tmask, const float* goal, int ldg, const float* bounds,
                             float w_consensus, float w_goal, float w_smooth, float w_length, float w_bounds, float rot_weight,
                             int* best, int* order, float* scores, float* terms, float* selected, int B, int G, int L, int Dp,
                             void* stream) {
  return traj_rank_launch("a3d_traj_rank", poses, tmask, goal, ldg, bounds, w_consensus, w_goal, w_smooth, w_length, w_bounds,
                          rot_weight, best, order, scores, terms, selected, B, G, L, Dp, nullptr, 0.f, stream);
}

extern "C" int a3d_traj_rank_extra(const float* poses, const unsigned char* tmask, const float* goal, int ldg, const float* bounds,
                                   float w_consensus, float w_goal, float w_smooth, float w_length, float w_bounds, float rot_weight,
                                   int* best, int* order, float* scores, float* terms, float* selected, int B, int G, int L, int Dp,
                                   const float* extra, float w_extra, void* stream) {
  return traj_rank_launch("a3d_traj_rank_extra", poses, tmask, goal, ldg, bounds, w_consensus, w_goal, w_smooth, w_length, w_bounds,
                          rot_weight, best, order, scores, terms, selected, B, G, L, Dp, extra, w_extra, stream);
}
