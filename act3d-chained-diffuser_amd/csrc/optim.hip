// Optimizer-side kernels on the flat parameter buffer (engine.FlatParams): the fused AdamW step that also maintains an exponential
// moving average (EMA) of the weights, and the in-place exchange that lets evaluation / sampling / deployment read the averages
// through the SAME storage every captured graph and pointer table already addresses.
//
//   a3d_adamw_ema_step : a3d_adamw_step (heads.hip: the same two launches, the same expression sequence) + per element
//                            ema <- ema + w (p_new - ema)
//                        for the elements of parameters that are active this step.  w lives on the device (ema_state[0]) and is
//                        advanced by the prepare launch from the EMA's own update count (ema_state[1]): the warm-up needs no host
//                        sync and nothing step-dependent is frozen into a captured graph.
//   a3d_swap_f32       : a <-> b in one pass.
#include "a3d_common.h"
#include "../../include/act3d_hip.h"
#include <algorithm>

namespace a3d {

// The two kernels below are heads.hip's adamw_prepare_kernel / adamw_kernel statement for statement (the per-parameter table, the
// skip rule and the update are described there), with the EMA lines added: a3d_adamw_ema_step must leave p, m, v, step and seg_state
// bit for bit as a3d_adamw_step does (tests/test_ema_gpu.py compares the two entries after every step).  A change to the
// arithmetic of one is a change to both.
constexpr int ADAMW_LDS_SEGS = 4096;

// One workgroup per parameter; the thread that counts the optimizer step also advances the EMA:
//   t = updates + 1;  w = 1 - min(decay, (1 + t) / (warmup + t)) = max(1 - decay, (warmup - 1) / (warmup + t))      (warmup >= 1)
//   w = 1 - decay                                                                                                   (warmup == 0)
__global__ __launch_bounds__(256) void adamw_ema_prepare_kernel(const float* __restrict__ g, const long long* __restrict__ seg_off,
                                                                float* __restrict__ seg_state, float* __restrict__ step,
                                                                float* __restrict__ ema_state, float lr, float beta1, float beta2,
                                                                float ema_decay, float ema_warmup) {
  const int seg = blockIdx.x;
  float* st = seg_state + (size_t)seg * 4;
  const long long a = seg_off[seg], b = seg_off[seg + 1];
  int in_graph = st[0] > 0.0f;
  if (!in_graph) {
    int nz = 0;
    for (long long i = a + threadIdx.x; i < b; i += blockDim.x) nz |= (g[i] != 0.0f);
    in_graph = __syncthreads_or(nz);
  }
  if (threadIdx.x == 0) {
    if (in_graph) {
      const float t = st[0] + 1.0f;
      st[0] = t;
      st[1] = 1.0f;
      st[2] = lr / (1.0f - powf(beta1, t));
      st[3] = sqrtf(1.0f - powf(beta2, t));
    } else {
      st[1] = 0.0f;
    }
    if (seg == 0) {
      step[0] += 1.0f;
      const float t = ema_state[1] + 1.0f;
      float w = 1.0f - ema_decay;
      if (ema_warmup >= 1.0f) w = fmaxf(w, (ema_warmup - 1.0f) / (ema_warmup + t));
      ema_state[0] = w;
      ema_state[1] = t;
    }
  }
}

// The average is updated from the p the thread has just formed: 5 loads + 4 stores per element instead of the 4 + 3 of the plain
// step followed by a 2 + 1 lerp launch.
__global__ __launch_bounds__(256) void adamw_ema_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                        float* __restrict__ v, float* __restrict__ ema,
                                                        const long long* __restrict__ seg_off, const float* __restrict__ seg_state,
                                                        const float* __restrict__ ema_state, int nseg, size_t n, size_t n_nodecay,
                                                        float lr, float beta1, float beta2, float eps, float wd0, float wd1,
                                                        float gscale) {
  __shared__ long long offS[ADAMW_LDS_SEGS + 1];
  const bool staged = nseg <= ADAMW_LDS_SEGS;
  if (staged) {
    for (int i = threadIdx.x; i <= nseg; i += blockDim.x) offS[i] = seg_off[i];
    __syncthreads();
  }
  const long long* off = staged ? offS : seg_off;
  const float w = ema_state[0];
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    int lo = 0, hi = nseg - 1;                 // largest seg with off[seg] <= i
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if ((size_t)off[mid] <= i) lo = mid; else hi = mid - 1;
    }
    const float* st = seg_state + (size_t)lo * 4;
    if (st[1] == 0.0f) continue;               // parameter not in the graph: p, m, v AND ema are left alone
    const float step_size = st[2], bc2s = st[3];
    const float gi = g[i] * gscale;
    const float wd = (i < n_nodecay) ? wd0 : wd1;
    float pi = p[i] * (1.0f - lr * wd);
    const float mi = beta1 * m[i] + (1.0f - beta1) * gi;
    const float vi = beta2 * v[i] + (1.0f - beta2) * gi * gi;
    const float denom = sqrtf(vi) / bc2s + eps;
    pi -= step_size * (mi / denom);
    p[i] = pi; m[i] = mi; v[i] = vi;
    const float ei = ema[i];
    ema[i] = ei + w * (pi - ei);
  }
}

// a[i] <-> b[i].  When a and b sit at the same offset inside a 16-byte line the middle goes as float4 (body = a + head is then
// 16-byte aligned for both), with a scalar head of `head` < 4 elements and a scalar tail; otherwise head = n and all is scalar.
__global__ __launch_bounds__(256) void swap_f32_kernel(float* __restrict__ a, float* __restrict__ b, size_t n, size_t head,
                                                       size_t nvec) {
  const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x, nthr = (size_t)gridDim.x * blockDim.x;
  f32x4* av = reinterpret_cast<f32x4*>(a + head);
  f32x4* bv = reinterpret_cast<f32x4*>(b + head);
  for (size_t i = tid; i < nvec; i += nthr) {
    const f32x4 x = av[i], y = bv[i];
    av[i] = y; bv[i] = x;
  }
  const size_t tail = head + nvec * 4;        // scalar elements: [0, head) and [tail, n)
  for (size_t i = tid; i < head + (n - tail); i += nthr) {
    const size_t j = i < head ? i : tail + (i - head);
    const float x = a[j], y = b[j];
    a[j] = y; b[j] = x;
  }
}

}  // namespace a3d

using namespace a3d;

extern "C" int a3d_adamw_ema_step(float* p, const float* g, float* m, float* v, float* ema, float* step, const long long* seg_off,
                                  float* seg_state, float* ema_state, int nseg, size_t n, size_t n_nodecay, float lr, float beta1,
                                  float beta2, float eps, float wd_nodecay, float wd_decay, float grad_scale, float ema_decay,
                                  float ema_warmup, void* stream) {
  if (!p || !g || !m || !v || !ema || !step || !seg_off || !seg_state || !ema_state) {
    set_error("a3d_adamw_ema_step: null pointer");
    return A3D_ERR_ARG;
  }
  if (nseg <= 0) {
    set_error("a3d_adamw_ema_step: the flat buffer needs at least one parameter segment (nseg = %d)", nseg);
    return A3D_ERR_ARG;
  }
  if (!(ema_decay >= 0.0f && ema_decay < 1.0f)) {               // NaN fails both comparisons
    set_error("a3d_adamw_ema_step: ema_decay = %g is outside [0, 1)", (double)ema_decay);
    return A3D_ERR_ARG;
  }
  if (!(ema_warmup == 0.0f || (ema_warmup >= 1.0f && std::isfinite(ema_warmup)))) {
    set_error("a3d_adamw_ema_step: ema_warmup = %g must be 0 (off) or a finite value >= 1", (double)ema_warmup);
    return A3D_ERR_ARG;
  }
  if (n == 0) return A3D_OK;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(adamw_ema_prepare_kernel, dim3(nseg), dim3(256), 0, s, g, seg_off, seg_state, step, ema_state, lr, beta1, beta2,
                     ema_decay, ema_warmup);
  int rc = check_launch("a3d_adamw_ema_step(prepare)");
  if (rc) return rc;
  const int grid = (int)std::min<size_t>((n + 255) / 256, 2048);
  hipLaunchKernelGGL(adamw_ema_kernel, dim3(grid), dim3(256), 0, s, p, g, m, v, ema, seg_off, seg_state, ema_state, nseg, n, n_nodecay,
                     lr, beta1, beta2, eps, wd_nodecay, wd_decay, grad_scale);
  return check_launch("a3d_adamw_ema_step");
}

extern "C" int a3d_swap_f32(float* a, float* b, size_t n, void* stream) {
  if (n == 0) return A3D_OK;
  if (!a || !b) { set_error("a3d_swap_f32: null pointer"); return A3D_ERR_ARG; }
  const uintptr_t ua = (uintptr_t)a, ub = (uintptr_t)b;
  if ((ua | ub) & 3u) { set_error("a3d_swap_f32: pointers must be 4-byte aligned"); return A3D_ERR_ARG; }
  if (n > SIZE_MAX / sizeof(float)) { set_error("a3d_swap_f32: n = %zu overflows a byte count", n); return A3D_ERR_ARG; }
  const uintptr_t bytes = (uintptr_t)n * sizeof(float);
  if (ua < ub ? ub - ua < bytes : ua - ub < bytes) {
    set_error("a3d_swap_f32: the two ranges of %zu floats overlap", n);
    return A3D_ERR_ARG;
  }
  size_t head = n, nvec = 0;
  if ((ua & 15u) == (ub & 15u)) {
    head = std::min<size_t>(((16u - (ua & 15u)) & 15u) / 4u, n);
    nvec = (n - head) / 4;
  }
  const size_t work = std::max<size_t>(nvec, n - nvec * 4);     // threads wanted: vector body vs scalar head + tail
  const int grid = (int)std::min<size_t>((work + 255) / 256, 2048);
  hipLaunchKernelGGL(swap_f32_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, a, b, n, head, nvec);
  return check_launch("a3d_swap_f32");
}
