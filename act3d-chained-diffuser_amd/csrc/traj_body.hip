// Body-aware swept clearance of sampled trajectory candidates (body_clearance, rank_trajectories(body=...)): the gripper as K <= 8
// spheres in the tool frame, rotated with every waypoint, each swept along the straight segment of its centre to the next valid
// waypoint, against the same cloud and through the same hinge as traj_clearance.hip.  None in the reference.
//
// Three launches, no atomics, no host synchronisation.
//   1  traj_body_rows            one workgroup per scene: the ranks of the valid rows (tc_rank_rows), which rows are scored and the
//      end row of every row (rank j + 1 when sweep is set and j + 1 < n - skip_tail, else the row itself); then per (candidate,
//      row, sphere) the segment record [a | d | inv | bad] of 8 floats: a = p + R(q) o, d = c - a with c the same expression on the
//      end row (d = 0 exactly where the end row is the row itself), inv = 1 / |d|^2 or 0, bad = 1 where a or c is not finite.  The
//      only place with quaternion arithmetic.
//   2  traj_body_partial<RPT>    the scan of traj_points.h (tc_scan_partial) over the G K L segment rows, row kind segment: 7
//      registers per row slot instead of 3.  Partial minima of d^2 go to ws[chunk][b][g][k][i].
//   3  traj_body_final           one workgroup per scene: per row and sphere the minimum over the chunks, ONE square root, minus the
//      radius; the minimum over the spheres is `nearest`; then the hinge and the mean of tc_hinge_mean, as traj_clear_final.
// R(q): the quaternion divided by max(|q|, 1e-10), t = 2 / |q^|^2, the first two columns as pose_row_to_signal (pose_signal.h) emits
// them, the third [t (xz + yw), t (yz - xw), 1 - t (xx + yy)]; written out with contraction off, as the pair expression is: one
// expression, the same bits wherever it is inlined.  The minimum of a set of floats is exact, the square root and the subtraction are
// monotone: `nearest` does not depend on the chunking, the tile split or the run.  With K = 1, o = 0, r = 0 and sweep = 0 every record
// is [p | 0 | 0] and d^2, the minimum, the root and the tree are those of traj_clearance.hip: the same bits.
#include "traj_points.h"
#include "../../include/act3d_hip.h"

namespace a3d {

constexpr int TB_MAX_K = A3D_TRAJ_BODY_MAX_SPHERES;
constexpr int TB_REC = 8;                // floats of a segment record

// ws: the partial minima [n_chunks][B][R] (R = G K L, TrajScan.G = G K), then the records [B][R][8], then 3 [B][L] ints: scored,
// rank of a row (-1 = padded), row of a rank
struct TrajBodyArgs : TrajScan {
  const float* poses;              // [B][G][L][Dp]
  const float* offsets;            // [K][3]
  const float* radii;              // [K]
  float* nearest;                  // [B][G][L] or NULL
  float* clearance;                // [B][G]
  int Gc, K, Dp, sweep;            // Gc: candidates per scene
  float margin;
  int skip_head, skip_tail;
};

__device__ __forceinline__ float* tb_records(const TrajBodyArgs& a) { return a.ws + (size_t)a.n_chunks * a.B * (a.G * a.L); }
__device__ __forceinline__ int* tb_flags(const TrajBodyArgs& a) { return (int*)(tb_records(a) + (size_t)a.B * (a.G * a.L) * TB_REC); }

// the rotation of a pose row's quaternion (w, x, y, z) = q[0..3]: R[row][column]
__device__ __forceinline__ void tb_rotation(const float* q, float R[3][3]) {
#pragma clang fp contract(off)
  float w = q[0], x = q[1], y = q[2], z = q[3];
  const float nrm = fmaxf(sqrtf(w * w + x * x + y * y + z * z), 1e-10f);
  w /= nrm; x /= nrm; y /= nrm; z /= nrm;
  const float t = 2.0f / (w * w + x * x + y * y + z * z);
  R[0][0] = 1.0f - t * (y * y + z * z); R[1][0] = t * (x * y + z * w);        R[2][0] = t * (x * z - y * w);
  R[0][1] = t * (x * y - z * w);        R[1][1] = 1.0f - t * (x * x + z * z); R[2][1] = t * (y * z + x * w);
  R[0][2] = t * (x * z + y * w);        R[1][2] = t * (y * z - x * w);        R[2][2] = 1.0f - t * (x * x + y * y);
}

// c = p + R o
__device__ __forceinline__ void tb_centre(const float* p, const float R[3][3], const float* o, float c[3]) {
#pragma clang fp contract(off)
#pragma unroll
  for (int k = 0; k < 3; ++k) c[k] = p[k] + ((R[k][0] * o[0] + R[k][1] * o[1]) + R[k][2] * o[2]);
}

__global__ __launch_bounds__(TC_THREADS) void traj_body_rows(const TrajBodyArgs a) {
  const int b = blockIdx.x, tid = threadIdx.x;
  const int G = a.Gc, K = a.K, L = a.L;
  const unsigned char* m = a.tmask + (size_t)b * L;
  int* scored = tb_flags(a) + (size_t)b * L;
  int* rank = tb_flags(a) + ((size_t)a.B + b) * L;
  int* row_of = tb_flags(a) + ((size_t)2 * a.B + b) * L;
  const int n = tc_rank_rows(m, L, [&](int i, bool valid, int j, int nv) {
    scored[i] = (valid && j >= a.skip_head && j < nv - a.skip_tail) ? 1 : 0;
    rank[i] = valid ? j : -1;
    if (valid) row_of[j] = i;
  });
  // the three arrays were written with global stores by other threads of this workgroup: tc_rank_rows ended with a barrier
  float* rec = tb_records(a) + (size_t)b * (G * K * L) * TB_REC;
  for (int gi = tid; gi < G * L; gi += TC_THREADS) {
    const int g = gi / L, i = gi - g * L;
    const int j = rank[i];
    if (j < 0) continue;                                       // a padded row: no record, the scan does not load it
    const int e = (a.sweep && j + 1 < n - a.skip_tail) ? row_of[j + 1] : i;
    const float* p = a.poses + (((size_t)b * G + g) * L + i) * a.Dp;
    const float* pe = a.poses + (((size_t)b * G + g) * L + e) * a.Dp;
    float R0[3][3], R1[3][3];
    tb_rotation(p + 3, R0);
    if (e != i) tb_rotation(pe + 3, R1);
    for (int k = 0; k < K; ++k) {
#pragma clang fp contract(off)
      const float o[3] = {a.offsets[3 * k], a.offsets[3 * k + 1], a.offsets[3 * k + 2]};
      float s[3], c[3], d[3] = {0.f, 0.f, 0.f};
      tb_centre(p, R0, o, s);
      bool ok = tc_finite(s[0]) && tc_finite(s[1]) && tc_finite(s[2]);
      if (e != i) {
        tb_centre(pe, R1, o, c);
        ok = ok && tc_finite(c[0]) && tc_finite(c[1]) && tc_finite(c[2]);
        d[0] = c[0] - s[0]; d[1] = c[1] - s[1]; d[2] = c[2] - s[2];
      }
      const float dd = fmaf(d[2], d[2], fmaf(d[1], d[1], d[0] * d[0]));
      float* out = rec + (((size_t)g * K + k) * L + i) * TB_REC;
      out[0] = s[0]; out[1] = s[1]; out[2] = s[2];
      out[3] = d[0]; out[4] = d[1]; out[5] = d[2];
      out[6] = dd == 0.f ? 0.f : 1.f / dd;
      out[7] = ok ? 0.f : 1.f;
    }
  }
}

template <int RPT>
__global__ __launch_bounds__(TC_THREADS) void traj_body_partial(const TrajBodyArgs a) {
  const float* recs = tb_records(a);
  tc_scan_partial<RPT, false, true>(a, [&a, recs](int b, int r, float& ax, float& ay, float& az, float& dx, float& dy, float& dz,
                                                  float& inv) {
    const float* p = recs + ((size_t)b * (a.G * a.L) + r) * TB_REC;
    ax = p[0]; ay = p[1]; az = p[2];
    dx = p[3]; dy = p[4]; dz = p[5];
    inv = p[6];
  });
}

__global__ __launch_bounds__(TC_THREADS) void traj_body_final(const TrajBodyArgs a) {
  const int b = blockIdx.x;
  const int G = a.Gc, K = a.K, L = a.L, R = G * K * L;
  const unsigned char* m = a.tmask + (size_t)b * L;
  const int* scored = tb_flags(a) + (size_t)b * L;
  const float* rec = tb_records(a) + (size_t)b * R * TB_REC;
  tc_hinge_mean(m, scored, a.nearest ? a.nearest + (size_t)b * G * L : nullptr, a.clearance + (size_t)b * G, G, L, a.margin,
                [&](int g, int i) {
    float near = INFINITY;
    bool bad = false;
    for (int k = 0; k < K; ++k) {
      const size_t r = ((size_t)g * K + k) * L + i;
      bad = bad || rec[r * TB_REC + 7] != 0.f;
      float d2 = INFINITY;
      for (int c = 0; c < a.n_chunks; ++c) d2 = fminf(d2, a.ws[((size_t)c * a.B + b) * R + r]);
      near = fminf(near, sqrtf(d2) - a.radii[k]);
    }
    return bad ? NAN : near;
  });
}

}  // namespace a3d

using namespace a3d;

extern "C" size_t a3d_traj_body_clearance_ws_floats(int B, int G, int L, int K, int n_points, int n_chunks) {
  if (G <= 0 || G > TC_MAX_G || K < 1 || K > TB_MAX_K) return 0;
  const size_t plane = tc_ws_plane(B, G * K, L, n_points, n_chunks);
  return plane ? plane + (size_t)B * G * K * L * TB_REC + (size_t)3 * B * L : 0;
}

extern "C" int a3d_traj_body_clearance(const float* poses, const unsigned char* tmask, const float* offsets, const float* radii, int K,
                                       int sweep, const float* scene, const unsigned char* scene_mask, int n_cam, int n_pix, float margin,
                                       int skip_head, int skip_tail, float* nearest, float* clearance, float* ws, int n_chunks, int B,
                                       int G, int L, int Dp, void* stream) {
  const char* me = "a3d_traj_body_clearance";
  TrajBodyArgs a;
  int rpt;
  unsigned blocks;
  const bool k_ok = K >= 1 && K <= TB_MAX_K;
  int rc = tc_scan_plan(me, poses && tmask && offsets && radii && scene && clearance && ws,
                        "poses, tmask, offsets, radii, scene, clearance and ws", &a, &rpt, &blocks, tmask, scene, scene_mask, ws, n_cam,
                        n_pix, margin, skip_head, skip_tail, n_chunks, B, G, L, k_ok ? K : 1);
  if (rc) return rc;
  if (!k_ok) { set_error("%s: K=%d, a body has 1 to %d spheres", me, K, TB_MAX_K); return A3D_ERR_ARG; }
  if (sweep != 0 && sweep != 1) { set_error("%s: sweep=%d must be 0 or 1", me, sweep); return A3D_ERR_ARG; }
  if (Dp != 7 && Dp != 8) { set_error("%s: Dp=%d, pose rows have 7 or 8 channels", me, Dp); return A3D_ERR_ARG; }
  a.poses = poses; a.offsets = offsets; a.radii = radii; a.nearest = nearest; a.clearance = clearance;
  a.Gc = G; a.K = K; a.Dp = Dp; a.sweep = sweep;
  a.margin = margin; a.skip_head = skip_head; a.skip_tail = skip_tail;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(traj_body_rows, dim3(B), dim3(TC_THREADS), 0, s, a);
  rc = check_launch(me);
  if (rc) return rc;
  rc = tc_scan_launch(me, rpt, blocks, a, s, traj_body_partial<1>, traj_body_partial<2>, traj_body_partial<4>);
  if (rc) return rc;
  hipLaunchKernelGGL(traj_body_final, dim3(B), dim3(TC_THREADS), 0, s, a);
  return check_launch(me);
}
