// Elementwise pieces of the ChainedDiffuser DDPM trajectory denoiser (all HBM/latency-bound; they exist so
// that one denoise step is a fixed sequence of stream-ordered launches with no host synchronisation and can be
// captured in a hipGraph).
//
//   a3d_ddpm_add_noise   x_t = sqrt(acp[t]) x0 + sqrt(1-acp[t]) eps, position / rotation channel groups with
//                        their own schedules                                   diffusion_model.py:296-305
//   a3d_ddpm_step        inpaint (out[mask] = cond[mask]) + DDPMScheduler.step with prediction_type="sample",
//                        clip_sample, fixed_small variance                      diffusion_model.py:107-117
//   a3d_ddpm_step_sched  the same update x_prev = c0 clip(x0) + c1 x_t + c2 z on row `row` of tables indexed by step position
//                        (strided DDPM / DDIM sampler schedules), with an explicit terminal flag instead of t == 0
//   a3d_adaln_{fwd,bwd}  x * (1 + scale) + shift                                layers.py:273-290
//   a3d_sinusoidal_emb   [sin(x f_j) | cos(x f_j)]                              position_encodings.py:7-20
//   a3d_silu_{fwd,bwd}   SiLU in AdaLN's modulation                             layers.py:276-278
//   a3d_add_rows         seq + per-position embedding (seq1_sem_pos)            layers.py:104-105,132-133
//   a3d_traj_update      cat(traj_xyz + delta, rot)                             diffusion_head.py:268-272
#include "a3d_common.h"
#include "pose_signal.h"
#include "../../include/act3d_hip.h"

namespace a3d {

__global__ void ddpm_add_noise_kernel(const float* __restrict__ x0, const float* __restrict__ noise,
                                      const long long* __restrict__ t, const float* __restrict__ acp_pos,
                                      const float* __restrict__ acp_rot, float* __restrict__ out, int B, int L, int D,
                                      int npos) {
  const size_t total = (size_t)B * L * D;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int c = (int)(i % D);
    const int b = (int)(i / ((size_t)L * D));
    const float a = (c < npos) ? acp_pos[t[b]] : acp_rot[t[b]];
    out[i] = sqrtf(a) * x0[i] + sqrtf(1.0f - a) * noise[i];
  }
}

// coef tables: [rows][3] = (coef_x0, coef_xt, sigma) per schedule; terminal: the in-painted network output is the result.
// HIST (a3d_ddpm_step_hist): the history term of a multistep schedule, kappa[row] (x0 - hist), added LAST and only where kappa != 0
// (so that a table of zeros gives the bits of the instance without it); every non-terminal step leaves its x0 in hist.
template <bool HIST>
__global__ void ddpm_step_kernel(const float* __restrict__ model_out, const float* __restrict__ sample,
                                 const float* __restrict__ noise, const float* __restrict__ cond_data,
                                 const unsigned char* __restrict__ cond_mask, const float* __restrict__ coef_pos,
                                 const float* __restrict__ coef_rot, float* __restrict__ out, int rows, int D,
                                 int npos, int row, int terminal, float* __restrict__ hist,
                                 const float* __restrict__ kappa_pos, const float* __restrict__ kappa_rot) {
  const size_t total = (size_t)rows * D;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int c = (int)(i % D);
    float mo = model_out[i];
    if (cond_mask && cond_mask[i]) mo = cond_data[i];
    if (terminal) { out[i] = mo; continue; }
    const float* cf = ((c < npos) ? coef_pos : coef_rot) + (size_t)row * 3;
    const float x0 = fminf(fmaxf(mo, -1.0f), 1.0f);
    float prev = cf[0] * x0 + cf[1] * sample[i];
    if (noise) prev += cf[2] * noise[i];
    if (HIST) {
      const float kap = ((c < npos) ? kappa_pos : kappa_rot)[row];
      if (kap != 0.f) prev += kap * (x0 - hist[i]);
      hist[i] = x0;
    }
    out[i] = prev;
  }
}

__global__ void adaln_fwd_kernel(const float* __restrict__ x, const float* __restrict__ mod, float* __restrict__ y,
                                 int B, int L, int E) {
  const size_t total = (size_t)B * L * E;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int c = (int)(i % E);
    const int b = (int)(i / ((size_t)L * E));
    y[i] = x[i] * (1.0f + mod[(size_t)b * 2 * E + c]) + mod[(size_t)b * 2 * E + E + c];
  }
}
// one workgroup per sample; dmod[b] = [sum_l dy*x | sum_l dy]
__global__ __launch_bounds__(256) void adaln_bwd_kernel(const float* __restrict__ x, const float* __restrict__ mod,
                                                        const float* __restrict__ dy, float* __restrict__ dx,
                                                        float* __restrict__ dmod, int L, int E) {
  const int b = blockIdx.x;
  for (int c = threadIdx.x; c < E; c += blockDim.x) {
    const float sc = 1.0f + mod[(size_t)b * 2 * E + c];
    float ds = 0.f, dh = 0.f;
    for (int l = 0; l < L; ++l) {
      const size_t i = ((size_t)b * L + l) * E + c;
      const float g = dy[i];
      ds += g * x[i];
      dh += g;
      dx[i] = g * sc;
    }
    dmod[(size_t)b * 2 * E + c] = ds;
    dmod[(size_t)b * 2 * E + E + c] = dh;
  }
}

// The same with the rows of a sample split over gridDim.x workgroups and float4 lanes (E % 4 == 0, E <= 1024): E / 4 lanes per row,
// 256 / (E / 4) rows per pass, the per-workgroup column sums reduced in LDS and added to dmod (zeroed by the launcher) with one
// atomic per column and workgroup.  The kernel above walks ALL L rows of a sample with E of its 256 threads in ONE workgroup --
// B = 22 workgroups on 256 CUs, 3074 dependent-latency steps for the trajectory model's context rows (22 us average, 0.7 ms of a
// diffusion training step).
__global__ __launch_bounds__(256) void adaln_bwd_split_kernel(const float* __restrict__ x, const float* __restrict__ mod,
                                                              const float* __restrict__ dy, float* __restrict__ dx,
                                                              float* __restrict__ dmod, int L, int E, int rows_per_wg) {
  extern __shared__ float red_ad[];                               // [rows per pass][2 E]
  const int b = blockIdx.y, t = threadIdx.x;
  const int lpr = E >> 2, rpp = 256 / lpr;                        // lanes per row, rows per pass
  const int rg = t / lpr, l4 = t - rg * lpr;                      // row group, float4 column
  const bool act = rg < rpp;
  const int c = l4 * 4;
  float4 ds = make_float4(0.f, 0.f, 0.f, 0.f), dh = ds;
  if (act) {
    const float4 m = *reinterpret_cast<const float4*>(mod + (size_t)b * 2 * E + c);
    const float4 sc = make_float4(1.0f + m.x, 1.0f + m.y, 1.0f + m.z, 1.0f + m.w);
    const int l_beg = blockIdx.x * rows_per_wg, l_end = min(L, l_beg + rows_per_wg);
    for (int l = l_beg + rg; l < l_end; l += rpp) {
      const size_t i = ((size_t)b * L + l) * E + c;
      const float4 g = *reinterpret_cast<const float4*>(dy + i);
      const float4 xv = *reinterpret_cast<const float4*>(x + i);
      ds.x += g.x * xv.x; ds.y += g.y * xv.y; ds.z += g.z * xv.z; ds.w += g.w * xv.w;
      dh.x += g.x; dh.y += g.y; dh.z += g.z; dh.w += g.w;
      *reinterpret_cast<float4*>(dx + i) = make_float4(g.x * sc.x, g.y * sc.y, g.z * sc.z, g.w * sc.w);
    }
    float* r = red_ad + (size_t)rg * 2 * E;
    *reinterpret_cast<float4*>(r + c) = ds;
    *reinterpret_cast<float4*>(r + E + c) = dh;
  }
  __syncthreads();
  for (int j = t; j < 2 * E; j += 256) {
    float a = 0.f;
    for (int u = 0; u < rpp; ++u) a += red_ad[(size_t)u * 2 * E + j];
    if (gridDim.x == 1) dmod[(size_t)b * 2 * E + j] = a;
    else atomicAdd(&dmod[(size_t)b * 2 * E + j], a);
  }
}

__global__ void sinusoidal_kernel(const float* __restrict__ x, float* __restrict__ out, int n, int E) {
  const int half = E / 2;
  const size_t total = (size_t)n * half;
  const float step = 9.210340371976184f / (float)(half - 1);
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int j = (int)(i % half);
    const size_t r = i / half;
    const float f = expf((float)j * -step);
    const float a = x[r] * f;
    out[r * E + j] = sinf(a);
    out[r * E + half + j] = cosf(a);
  }
}

__global__ void silu_fwd_kernel(const float* __restrict__ x, float* __restrict__ y, size_t n) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const float v = x[i];
    y[i] = v / (1.0f + expf(-v));
  }
}
__global__ void silu_bwd_kernel(const float* __restrict__ x, const float* __restrict__ dy, float* __restrict__ dx,
                                size_t n) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const float v = x[i];
    const float s = 1.0f / (1.0f + expf(-v));
    dx[i] = dy[i] * s * (1.0f + v * (1.0f - s));
  }
}

__global__ void add_rows_kernel(const float* __restrict__ x, const float* __restrict__ r, float* __restrict__ y, int B,
                                int L, int E) {
  const size_t total = (size_t)B * L * E;
  const size_t le = (size_t)L * E;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x)
    y[i] = x[i] + r[i % le];
}

// backward of the broadcast add w.r.t. the shared rows: dr[l][e] = sum_b dy[b][l][e]
__global__ void add_rows_bwd_kernel(const float* __restrict__ dy, float* __restrict__ dr, int B, int LE) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= LE) return;
  float acc = 0.f;
  for (int b = 0; b < B; ++b) acc += dy[(size_t)b * LE + i];
  dr[i] = acc;
}

__global__ void traj_update_kernel(const float* __restrict__ traj, const float* __restrict__ upd, float* __restrict__ out,
                                   int rows, int D, int npos) {
  const size_t total = (size_t)rows * D;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int c = (int)(i % D);
    out[i] = (c < npos) ? traj[i] + upd[i] : upd[i];
  }
}

// ---------------------------------------------------------------- pose <-> network signal (one launch each way)
// diffusion_model.py:187-230: workspace normalisation of xyz to [-1, 1] and the quaternion <-> 6D rotation change of
// variables (model/utils/utils.py:51-52,117-139 and the quaternion <-> matrix maps of utils/pytorch3d_transforms.py),
// written from the closed forms: R(q) for a unit quaternion (w, x, y, z); 6D = the first two columns of R; back:
// Gram-Schmidt of the two 3-vectors, then the quaternion from the best-conditioned of the four trace identities.
// One thread per pose row; rows carry `extra` trailing channels that pass through.
// pose_row_to_signal is the row map itself (pose_signal.h), shared with traj_condition_kernel and traj_pins_kernel so that all
// three produce the same bits.
__global__ void pose_to_signal_kernel(const float* __restrict__ in, const float* __restrict__ bounds,
                                      float* __restrict__ out, int n, int extra) {
  const int Din = 7 + extra, Dout = 9 + extra;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
    pose_row_to_signal(in + (size_t)i * Din, bounds, out + (size_t)i * Dout, extra);
}

// ---------------------------------------------------------------- conditioning of a sampling call in one launch
// diffusion_model.py:131-168: the start / goal poses as network signals, the in-painting data and mask (start pose on row 0, goal
// pose on row L - pad - 1 and the mask from there on, pad = the number of padded steps of the scene) and the noisy start
// trajectory.  One workgroup row per scene (blockIdx.x = b); its G trajectories b G + g are spread over blockIdx.y.  Every
// workgroup converts the scene's two poses and counts its padding itself (a few hundred flops), so there is no second launch
// and nothing is exchanged through memory.
__global__ __launch_bounds__(256) void traj_condition_kernel(
    const float* __restrict__ curr, int ldc, const float* __restrict__ goal, int ldg, const float* __restrict__ bounds,
    const unsigned char* __restrict__ tmask, const float* __restrict__ init_noise, float* __restrict__ cg,
    float* __restrict__ gg, float* __restrict__ cond_data, unsigned char* __restrict__ cond_mask,
    unsigned char* __restrict__ kmask, float* __restrict__ traj, int G, int L, int Dp, int use_goal) {
  __shared__ float s_sig[2][TC_MAX_D];
  __shared__ int s_cnt[256];
  const int b = blockIdx.x, t = threadIdx.x, D = Dp + 2;
  const unsigned char* mrow = tmask + (size_t)b * L;
  if (t < 2) pose_row_to_signal(t == 0 ? curr + (size_t)b * ldc : goal + (size_t)b * ldg, bounds, s_sig[t], Dp - 7);
  int cnt = 0;
  for (int l = t; l < L; l += 256) cnt += mrow[l] != 0;
  s_cnt[t] = cnt;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (t < s) s_cnt[t] += s_cnt[t + s];
    __syncthreads();
  }
  const int gidx = L - s_cnt[0] - 1;                              // -1: the whole row is padding -- all masked, no goal row
  if (blockIdx.y == 0 && t < 2 * D) {
    if (t < D) cg[(size_t)b * D + t] = s_sig[0][t];
    else gg[(size_t)b * D + (t - D)] = s_sig[1][t - D];
  }
  const int LD = L * D;
  for (int g = blockIdx.y; g < G; g += gridDim.y) {
    const size_t row = (size_t)b * G + g;
    for (int i = t; i < LD; i += 256) {
      const int l = i / D, c = i - l * D;
      const float v = (use_goal && l == gidx) ? s_sig[1][c] : (l == 0 ? s_sig[0][c] : 0.0f);
      const size_t j = row * LD + i;
      cond_data[j] = v;
      cond_mask[j] = (l == 0 || (use_goal && l >= gidx)) ? 1 : 0;
      if (traj) traj[j] = init_noise[j] + v;
    }
    for (int l = t; l < L; l += 256) kmask[row * L + l] = mrow[l] != 0 ? 1 : 0;
  }
}

__global__ void signal_to_pose_kernel(const float* __restrict__ in, const float* __restrict__ bounds,
                                      float* __restrict__ out, int n, int extra) {
  const int Din = 9 + extra, Dout = 7 + extra;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const float* r = in + (size_t)i * Din;
    float* o = out + (size_t)i * Dout;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      if (bounds) {
        const float lo = bounds[a], hi = bounds[3 + a];
        o[a] = (r[a] + 1.0f) / 2.0f * (hi - lo) + lo;
      } else {
        o[a] = r[a];
      }
    }
    // orthonormal frame (c0, c1, c2) from the two raw 3-vectors: c0 = a / |a|, c2 = (c0 x b) / |c0 x b|, c1 = c2 x c0
    float c0[3] = {r[3], r[4], r[5]};
    const float n0 = fmaxf(sqrtf(c0[0] * c0[0] + c0[1] * c0[1] + c0[2] * c0[2]), 1e-8f);
    c0[0] /= n0; c0[1] /= n0; c0[2] /= n0;
    float c2[3] = {c0[1] * r[8] - c0[2] * r[7], c0[2] * r[6] - c0[0] * r[8], c0[0] * r[7] - c0[1] * r[6]};
    const float n2 = fmaxf(sqrtf(c2[0] * c2[0] + c2[1] * c2[1] + c2[2] * c2[2]), 1e-8f);
    c2[0] /= n2; c2[1] /= n2; c2[2] /= n2;
    const float c1[3] = {c2[1] * c0[2] - c2[2] * c0[1], c2[2] * c0[0] - c2[0] * c0[2], c2[0] * c0[1] - c2[1] * c0[0]};
    // R[row][col] = c_col[row]
    const float r00 = c0[0], r10 = c0[1], r20 = c0[2], r01 = c1[0], r11 = c1[1], r21 = c1[2], r02 = c2[0], r12 = c2[1], r22 = c2[2];
    // 4 w^2 = 1 + tr, 4 x^2 = 1 + r00 - r11 - r22, ...: take the largest component as the pivot
    const float d[4] = {1.0f + r00 + r11 + r22, 1.0f + r00 - r11 - r22, 1.0f - r00 + r11 - r22, 1.0f - r00 - r11 + r22};
    float mag[4];
    int piv = 0;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      mag[c] = d[c] > 0.f ? sqrtf(d[c]) : 0.f;
      if (mag[c] > mag[piv]) piv = c;
    }
    const float den = 2.0f * fmaxf(mag[piv], 0.1f);
    float q[4];
    if (piv == 0) { q[0] = mag[0] * mag[0]; q[1] = r21 - r12; q[2] = r02 - r20; q[3] = r10 - r01; }
    else if (piv == 1) { q[0] = r21 - r12; q[1] = mag[1] * mag[1]; q[2] = r10 + r01; q[3] = r02 + r20; }
    else if (piv == 2) { q[0] = r02 - r20; q[1] = r10 + r01; q[2] = mag[2] * mag[2]; q[3] = r12 + r21; }
    else { q[0] = r10 - r01; q[1] = r20 + r02; q[2] = r21 + r12; q[3] = mag[3] * mag[3]; }
#pragma unroll
    for (int c = 0; c < 4; ++c) o[3 + c] = q[c] / den;
    for (int e = 0; e < extra; ++e) o[7 + e] = r[9 + e];
  }
}

// per-trajectory error columns of TrajectoryCriterion.compute_metrics (main_trajectory.py:303-343); one wave per sample.
// cols[b] = { mean_l pos_l2, mean_l [pos_l2 < 0.01], mean_l rot_l1, mean_l [rot_l1 < 0.025], mean_{l,c} (pred - gt)^2,
//             and the same four position / rotation figures at the last step }, rot_l1 = min(|q - g|_1, |q + g|_1)
__global__ __launch_bounds__(64) void traj_errors_kernel(const float* __restrict__ pred, const float* __restrict__ gt,
                                                         float* __restrict__ cols, int L, int D) {
  const int b = blockIdx.x, lane = threadIdx.x;
  float s_pos = 0.f, s_pacc = 0.f, s_rot = 0.f, s_racc = 0.f, s_sq = 0.f;
  float last[4] = {0.f, 0.f, 0.f, 0.f};
  for (int l = lane; l < L; l += 64) {
    const float* p = pred + ((size_t)b * L + l) * D;
    const float* g = gt + ((size_t)b * L + l) * D;
    float d2 = 0.f, a = 0.f, a_neg = 0.f, sq = 0.f;
    for (int c = 0; c < D; ++c) {
      const float e = p[c] - g[c];
      sq += e * e;
      if (c < 3) d2 += e * e;
      else if (c < 7) { a += fabsf(e); a_neg += fabsf(p[c] + g[c]); }
    }
    const float pos = sqrtf(d2), rot = fminf(a, a_neg);
    s_pos += pos; s_pacc += pos < 0.01f ? 1.f : 0.f;
    s_rot += rot; s_racc += rot < 0.025f ? 1.f : 0.f;
    s_sq += sq;
    if (l == L - 1) { last[0] = pos; last[1] = pos < 0.01f ? 1.f : 0.f; last[2] = rot; last[3] = rot < 0.025f ? 1.f : 0.f; }
  }
  s_pos = wave_sum(s_pos); s_pacc = wave_sum(s_pacc); s_rot = wave_sum(s_rot); s_racc = wave_sum(s_racc); s_sq = wave_sum(s_sq);
#pragma unroll
  for (int c = 0; c < 4; ++c) last[c] = wave_sum(last[c]);
  if (lane == 0) {
    float* o = cols + (size_t)b * 9;
    o[0] = s_pos / L; o[1] = s_pacc / L; o[2] = s_rot / L; o[3] = s_racc / L; o[4] = s_sq / ((float)L * D);
    o[5] = last[0]; o[6] = last[1]; o[7] = last[2]; o[8] = last[3];
  }
}

}  // namespace a3d

using namespace a3d;
static inline int gsz(size_t n) { return (int)std::min<size_t>((n + 255) / 256, 4096); }

extern "C" int a3d_ddpm_add_noise(const float* x0, const float* noise, const long long* t, const float* acp_pos,
                                  const float* acp_rot, float* out, int B, int L, int D, int npos, void* stream) {
  if (!x0 || !noise || !t || !acp_pos || !acp_rot || !out || B <= 0 || L <= 0 || D <= 0) { set_error("a3d_ddpm_add_noise: bad argument"); return A3D_ERR_ARG; }
  hipLaunchKernelGGL(ddpm_add_noise_kernel, dim3(gsz((size_t)B * L * D)), dim3(256), 0, (hipStream_t)stream, x0, noise, t, acp_pos, acp_rot, out, B, L, D, npos);
  return check_launch("a3d_ddpm_add_noise");
}
extern "C" int a3d_ddpm_step(const float* model_out, const float* sample, const float* noise, const float* cond_data,
                             const unsigned char* cond_mask, const float* coef_pos, const float* coef_rot, float* out,
                             int rows, int D, int npos, int t, void* stream) {
  if (!model_out || !sample || !coef_pos || !coef_rot || !out || rows <= 0 || D <= 0 || t < 0 || (cond_mask && !cond_data)) { set_error("a3d_ddpm_step: bad argument"); return A3D_ERR_ARG; }
  hipLaunchKernelGGL(ddpm_step_kernel<false>, dim3(gsz((size_t)rows * D)), dim3(256), 0, (hipStream_t)stream, model_out, sample, noise, cond_data, cond_mask, coef_pos, coef_rot, out, rows, D, npos, t, t == 0, nullptr, nullptr, nullptr);
  return check_launch("a3d_ddpm_step");
}
extern "C" int a3d_ddpm_step_sched(const float* model_out, const float* sample, const float* noise, const float* cond_data,
                                   const unsigned char* cond_mask, const float* coef_pos, const float* coef_rot, float* out,
                                   int rows, int D, int npos, int row, int terminal, void* stream) {
  if (!model_out || !sample || !coef_pos || !coef_rot || !out || rows <= 0 || D <= 0 || row < 0 || (terminal != 0 && terminal != 1) ||
      (cond_mask && !cond_data)) { set_error("a3d_ddpm_step_sched: bad argument"); return A3D_ERR_ARG; }
  hipLaunchKernelGGL(ddpm_step_kernel<false>, dim3(gsz((size_t)rows * D)), dim3(256), 0, (hipStream_t)stream, model_out, sample, noise, cond_data, cond_mask, coef_pos, coef_rot, out, rows, D, npos, row, terminal, nullptr, nullptr, nullptr);
  return check_launch("a3d_ddpm_step_sched");
}
extern "C" int a3d_ddpm_step_hist(const float* model_out, const float* sample, const float* noise, const float* cond_data,
                                  const unsigned char* cond_mask, const float* coef_pos, const float* coef_rot, float* out,
                                  int rows, int D, int npos, int row, int terminal, float* hist, const float* kappa_pos,
                                  const float* kappa_rot, void* stream) {
  if (!model_out || !sample || !coef_pos || !coef_rot || !out || rows <= 0 || D <= 0 || row < 0 || (terminal != 0 && terminal != 1) ||
      (cond_mask && !cond_data)) { set_error("a3d_ddpm_step_hist: bad argument"); return A3D_ERR_ARG; }
  if (!hist || !kappa_pos || !kappa_rot) {
    set_error("a3d_ddpm_step_hist: the history term needs hist, kappa_pos and kappa_rot (got %s%s%s)", hist ? "hist " : "",
              kappa_pos ? "kappa_pos " : "", kappa_rot ? "kappa_rot" : "");
    return A3D_ERR_ARG;
  }
  hipLaunchKernelGGL(ddpm_step_kernel<true>, dim3(gsz((size_t)rows * D)), dim3(256), 0, (hipStream_t)stream, model_out, sample, noise, cond_data, cond_mask, coef_pos, coef_rot, out, rows, D, npos, row, terminal, hist, kappa_pos, kappa_rot);
  return check_launch("a3d_ddpm_step_hist");
}
extern "C" int a3d_adaln_fwd(const float* x, const float* mod, float* y, int B, int L, int E, void* stream) {
  if (!x || !mod || !y || B <= 0 || L <= 0 || E <= 0) { set_error("a3d_adaln_fwd: bad argument"); return A3D_ERR_ARG; }
  hipLaunchKernelGGL(adaln_fwd_kernel, dim3(gsz((size_t)B * L * E)), dim3(256), 0, (hipStream_t)stream, x, mod, y, B, L, E);
  return check_launch("a3d_adaln_fwd");
}
extern "C" int a3d_adaln_bwd(const float* x, const float* mod, const float* dy, float* dx, float* dmod, int B, int L,
                             int E, void* stream) {
  if (!x || !mod || !dy || !dx || !dmod || B <= 0 || L <= 0 || E <= 0) { set_error("a3d_adaln_bwd: bad argument"); return A3D_ERR_ARG; }
  if ((E & 3) == 0 && E <= 1024 && ((((uintptr_t)x) | ((uintptr_t)mod) | ((uintptr_t)dy) | ((uintptr_t)dx)) & 15) == 0) {
    const int rpp = 256 / (E / 4);
    // rows per workgroup: at least 4 passes each, at most ~2 workgroups per CU over the batch
    int nsplit = std::max(1, std::min(cdiv(L, 4 * rpp), cdiv(512, B)));
    const int rows_per_wg = cdiv(cdiv(L, nsplit), rpp) * rpp;
    nsplit = cdiv(L, rows_per_wg);
    if (nsplit > 1) {
      // a kernel node, not a memset node: this call sits inside the captured diffusion training step (engine.GraphedStep)
      const int zrc = zero_words(dmod, (size_t)B * 2 * E * sizeof(float), (hipStream_t)stream, "a3d_adaln_bwd(zero)");
      if (zrc) return zrc;
    }
    hipLaunchKernelGGL(adaln_bwd_split_kernel, dim3(nsplit, B), dim3(256), (size_t)rpp * 2 * E * sizeof(float), (hipStream_t)stream, x, mod, dy,
                       dx, dmod, L, E, rows_per_wg);
    return check_launch("a3d_adaln_bwd");
  }
  hipLaunchKernelGGL(adaln_bwd_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, x, mod, dy, dx, dmod, L, E);
  return check_launch("a3d_adaln_bwd");
}
extern "C" int a3d_sinusoidal_emb(const float* x, float* out, int n, int E, void* stream) {
  if (!x || !out || n <= 0 || E < 4 || (E & 1)) { set_error("a3d_sinusoidal_emb: bad argument"); return A3D_ERR_ARG; }
  hipLaunchKernelGGL(sinusoidal_kernel, dim3(gsz((size_t)n * E / 2)), dim3(256), 0, (hipStream_t)stream, x, out, n, E);
  return check_launch("a3d_sinusoidal_emb");
}
extern "C" int a3d_silu_fwd(const float* x, float* y, size_t n, void* stream) {
  if (!x || !y) { set_error("a3d_silu_fwd: null pointer"); return A3D_ERR_ARG; }
  if (!n) return A3D_OK;
  hipLaunchKernelGGL(silu_fwd_kernel, dim3(gsz(n)), dim3(256), 0, (hipStream_t)stream, x, y, n);
  return check_launch("a3d_silu_fwd");
}
extern "C" int a3d_silu_bwd(const float* x, const float* dy, float* dx, size_t n, void* stream) {
  if (!x || !dy || !dx) { set_error("a3d_silu_bwd: null pointer"); return A3D_ERR_ARG; }
  if (!n) return A3D_OK;
  hipLaunchKernelGGL(silu_bwd_kernel, dim3(gsz(n)), dim3(256), 0, (hipStream_t)stream, x, dy, dx, n);
  return check_launch("a3d_silu_bwd");
}
extern "C" int a3d_add_rows(const float* x, const float* r, float* y, int B, int L, int E, void* stream) {
  if (!x || !r || !y || B <= 0 || L <= 0 || E <= 0) { set_error("a3d_add_rows: bad argument"); return A3D_ERR_ARG; }
  hipLaunchKernelGGL(add_rows_kernel, dim3(gsz((size_t)B * L * E)), dim3(256), 0, (hipStream_t)stream, x, r, y, B, L, E);
  return check_launch("a3d_add_rows");
}
extern "C" int a3d_add_rows_bwd(const float* dy, float* dr, int B, int L, int E, void* stream) {
  if (!dy || !dr || B <= 0 || L <= 0 || E <= 0) { set_error("a3d_add_rows_bwd: bad argument"); return A3D_ERR_ARG; }
  hipLaunchKernelGGL(add_rows_bwd_kernel, dim3((L * E + 255) / 256), dim3(256), 0, (hipStream_t)stream, dy, dr, B, L * E);
  return check_launch("a3d_add_rows_bwd");
}
extern "C" int a3d_traj_update(const float* traj, const float* upd, float* out, int rows, int D, int npos, void* stream) {
  if (!traj || !upd || !out || rows <= 0 || D <= 0) { set_error("a3d_traj_update: bad argument"); return A3D_ERR_ARG; }
  hipLaunchKernelGGL(traj_update_kernel, dim3(gsz((size_t)rows * D)), dim3(256), 0, (hipStream_t)stream, traj, upd, out, rows, D, npos);
  return check_launch("a3d_traj_update");
}

extern "C" int a3d_pose_to_signal(const float* pose, const float* bounds, float* out, int n, int extra, void* stream) {
  if (!pose || !out || n <= 0 || extra < 0) { set_error("a3d_pose_to_signal: bad argument"); return A3D_ERR_ARG; }
  hipLaunchKernelGGL(pose_to_signal_kernel, dim3(gsz((size_t)n)), dim3(256), 0, (hipStream_t)stream, pose, bounds, out, n, extra);
  return check_launch("a3d_pose_to_signal");
}
extern "C" int a3d_signal_to_pose(const float* signal, const float* bounds, float* out, int n, int extra, void* stream) {
  if (!signal || !out || n <= 0 || extra < 0) { set_error("a3d_signal_to_pose: bad argument"); return A3D_ERR_ARG; }
  hipLaunchKernelGGL(signal_to_pose_kernel, dim3(gsz((size_t)n)), dim3(256), 0, (hipStream_t)stream, signal, bounds, out, n, extra);
  return check_launch("a3d_signal_to_pose");
}
extern "C" int a3d_traj_condition(const float* curr, int ldc, const float* goal, int ldg, const float* bounds,
                                  const unsigned char* tmask, const float* init_noise, float* cg, float* gg, float* cond_data,
                                  unsigned char* cond_mask, unsigned char* kmask, float* traj, int B, int G, int L, int Dp,
                                  int use_goal, void* stream) {
  if (!curr || !goal || !bounds || !tmask || !cg || !gg || !cond_data || !cond_mask || !kmask) {
    set_error("a3d_traj_condition: null pointer"); return A3D_ERR_ARG;
  }
  if ((init_noise == nullptr) != (traj == nullptr)) {
    set_error("a3d_traj_condition: init_noise and traj go together (both or neither)"); return A3D_ERR_ARG;
  }
  if (B <= 0 || G <= 0 || L <= 0) { set_error("a3d_traj_condition: B, G and L must be positive"); return A3D_ERR_ARG; }
  if (Dp < 7 || Dp + 2 > a3d::TC_MAX_D) { set_error("a3d_traj_condition: Dp must lie in [7, 30]"); return A3D_ERR_ARG; }
  if (ldc < Dp || ldg < Dp) { set_error("a3d_traj_condition: a leading dimension is smaller than Dp"); return A3D_ERR_ARG; }
  if ((long long)L * (Dp + 2) > 0x7fffffffLL) { set_error("a3d_traj_condition: L * D overflows int"); return A3D_ERR_ARG; }
  hipLaunchKernelGGL(traj_condition_kernel, dim3(B, G < 64 ? G : 64), dim3(256), 0, (hipStream_t)stream, curr, ldc, goal, ldg,
                     bounds, tmask, init_noise, cg, gg, cond_data, cond_mask, kmask, traj, G, L, Dp, use_goal ? 1 : 0);
  return check_launch("a3d_traj_condition");
}
extern "C" int a3d_traj_errors(const float* pred, const float* gt, float* cols, int B, int L, int D, void* stream) {
  if (!pred || !gt || !cols || B <= 0 || L <= 0 || D < 7) { set_error("a3d_traj_errors: bad argument (B=%d L=%d D=%d, D >= 7)", B, L, D); return A3D_ERR_ARG; }
  hipLaunchKernelGGL(traj_errors_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream, pred, gt, cols, L, D);
  return check_launch("a3d_traj_errors");
}
