// Optimizer-side kernels on the flat parameter buffer (engine.FlatParams): the fused AdamW step, optionally with an exponential
// moving average (EMA) of the weights and with global gradient-norm clipping, and the in-place exchange that lets evaluation /
// sampling / deployment read the averages through the SAME storage every captured graph and pointer table already addresses.
//
//   a3d_adamw_step      : torch.optim.AdamW update on the flat parameter buffer (engine.py:89-102): prepare + update launch.
//   a3d_adamw_ema_step  : the same two launches + per element
//                             ema <- ema + w (p_new - ema)
//                         for the elements of parameters that are active this step.  w lives on the device (ema_state[0]) and is
//                         advanced by the prepare launch from the EMA's own update count (ema_state[1]): the warm-up needs no host
//                         sync and nothing step-dependent is frozen into a captured graph.
//   a3d_adamw_clip_step : a norm launch in front of the same two: sum g^2 in double -> one partial per workgroup; the prepare launch
//                         combines the partials, decides {skip, clip coefficient} on the device and leaves the effective gradient
//                         scale in clip_state[0], which the update launch reads in place of the host's grad_scale.  EMA optional.
//   a3d_adamw_sched_step: any of the above with the learning rate taken from a warm-up + decay schedule that is evaluated on the
//                         device: the prepare launch derives lr_t from the position and the base rate in lr_state and leaves it
//                         in lr_state[0], the update launch reads it there and advances the position.  Nothing rate-dependent
//                         is a kernel argument, so a captured graph follows the schedule and a changed base rate.
//   a3d_swap_f32        : a <-> b in one pass.
#include "a3d_common.h"
#include "../../include/act3d_hip.h"
#include <algorithm>
#include <cmath>

namespace a3d {

// torch.optim.AdamW decides PER PARAMETER: a parameter whose .grad is None is skipped (no decay, no moment update, its own
// `step` does not advance -- engine.py:121-124 find_unused_parameters: the FPN blocks / embeddings a configuration never
// reads), every other parameter is updated in full, zero-gradient elements (dead ReLU rows, pad channels) included, with the
// bias correction of ITS OWN step count.  The flat buffer has no None: seg_off [nseg + 1] delimits the parameters, and
// seg_state [nseg][4] = {step, active, lr / bc1, sqrt(bc2)} carries the per-parameter state.  A parameter is "in the graph"
// from the first step in which any element of its gradient segment is non-zero, and stays in (which tensors a model's
// forward reaches is structural); adamw_prepare_kernel (one workgroup per parameter; the scan only runs until the parameter
// is in) advances the step counts and leaves the coefficients for adamw_kernel, whose threads find their element's parameter
// by bisection of the LDS-staged offsets.  Elements [0, n_nodecay) use weight decay wd0, the rest wd1.
//
// ONE prepare kernel and ONE update kernel serve the four entries: <EMA, CLIP, SCHED> only add statements (if constexpr), so the
// arithmetic of p, m, v, step and seg_state is the same expression sequence everywhere -- a3d_adamw_ema_step leaves them bit for bit
// as a3d_adamw_step does, a3d_adamw_clip_step as either of them called with grad_scale = clip_state[0], and a3d_adamw_sched_step
// as any of the three called with lr = lr_state[0] (tests/test_ema_gpu.py, tests/test_grad_clip_gpu.py, tests/test_lr_schedule_gpu.py
// compare the entries after every step).
constexpr int ADAMW_LDS_SEGS = 4096;
constexpr int CLIP_PARTS = A3D_ADAMW_CLIP_WS_DOUBLES;       // workgroups of the norm pass = partials in clip_ws
static_assert(CLIP_PARTS == 256, "clip_decide reads one partial per thread of a 256-thread workgroup");

// Sum of one double per thread over a 256-thread workgroup, returned to EVERY thread with the same bits: an xor butterfly inside
// the wave (lane i adds x[i ^ k], its partner the same two numbers the other way round: a + b == b + a), the four wave sums
// through LDS, added in one fixed order.  No atomics, so the result depends on the inputs only.
__device__ __forceinline__ double block_sum_f64(double x, double* wsum) {
#pragma unroll
  for (int k = 32; k >= 1; k >>= 1) x += __shfl_xor(x, k, 64);
  __syncthreads();                             // wsum may still be read from a previous call
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = x;
  __syncthreads();
  return (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]);
}

// Norm pass: partial[blockIdx.x] = sum over this workgroup's grid-stride share of g[i]^2, squares and sums in double (the square of
// an fp32 value is exact in double, and the sum of n < 2^64 of them cannot overflow).  The middle of g goes as float4 (g + head is
// 16-byte aligned), the `head` < 4 leading and the < 4 trailing elements as scalars, as swap_f32_kernel does it.
__global__ __launch_bounds__(256) void grad_sqnorm_kernel(const float* __restrict__ g, size_t n, size_t head, size_t nvec,
                                                          double* __restrict__ partial) {
  __shared__ double wsum[4];
  const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x, nthr = (size_t)gridDim.x * blockDim.x;
  const f32x4* gv = reinterpret_cast<const f32x4*>(g + head);
  double acc = 0.0;
  for (size_t i = tid; i < nvec; i += nthr) {
    const f32x4 x = gv[i];
    const double a = x[0], b = x[1], c = x[2], d = x[3];
    acc += (a * a + b * b) + (c * c + d * d);
  }
  const size_t tail = head + nvec * 4;        // scalar elements: [0, head) and [tail, n)
  for (size_t i = tid; i < head + (n - tail); i += nthr) {
    const double a = g[i < head ? i : tail + (i - head)];
    acc += a * a;
  }
  const double s = block_sum_f64(acc, wsum);
  if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

// The decision of a clipped step, derived by every workgroup that needs it from the same `nparts` partials with the same code,
// hence with the same bits: norm = fp32(|gscale| sqrt(sum)), coef = min(1, max_norm / (norm + 1e-6)) (torch's clip_grad_norm_),
// e = gscale * coef; a non-finite norm (a NaN / inf gradient element, or an fp32 overflow of the norm) skips the step.
struct ClipDecision {
  float e, norm, coef;
  bool skip;
};
__device__ __forceinline__ ClipDecision clip_decide(const double* __restrict__ partial, int nparts, float gscale, float max_norm,
                                                    double* wsum) {
  const double sum = block_sum_f64((int)threadIdx.x < nparts ? partial[threadIdx.x] : 0.0, wsum);
  ClipDecision d;
  d.norm = (float)(fabs((double)gscale) * sqrt(sum));
  d.skip = !isfinite(d.norm);
  d.coef = d.skip ? 0.0f : fminf(1.0f, max_norm / (d.norm + 1e-6f));
  d.e = d.skip ? 0.0f : gscale * d.coef;
  return d;
}

// The rate of a scheduled step (tests/lr_schedule_ref.py is the float64 statement): t = lr_state[1] scheduled steps applied so
// far, base = lr_state[3];
//   t < W: f = t / W;   else constant: f = 1;   linear: f = 1 - (1 - r) u;   cosine: f = r + (1 - r) (1 + cos(pi u)) / 2
//   u = min(1, (t - W) / (N - W));   lr_t = fp32(base f), everything before that rounding in double.
// Derived by one thread of every prepare workgroup from the same two words with the same code, hence with the same bits.
struct SchedArgs {
  double warmup, total, min_ratio;
  int kind;
};
struct SchedRate {
  float lr, f;
};
__device__ __forceinline__ SchedRate sched_rate(const float* __restrict__ lr_state, const SchedArgs& sc) {
  const double t = lr_state[1], base = lr_state[3];
  double f = 1.0;
  if (t < sc.warmup) {
    f = t / sc.warmup;
  } else if (sc.kind != A3D_LR_CONSTANT) {
    const double u = fmin(1.0, (t - sc.warmup) / (sc.total - sc.warmup)), r = sc.min_ratio;
    f = sc.kind == A3D_LR_LINEAR ? 1.0 - (1.0 - r) * u : r + (1.0 - r) * (1.0 + cos(3.14159265358979323846 * u)) / 2.0;
  }
  return {(float)(base * f), (float)f};
}

// One workgroup per parameter; the thread that counts the optimizer step also advances the EMA:
//   t = updates + 1;  w = 1 - min(decay, (1 + t) / (warmup + t)) = max(1 - decay, (warmup - 1) / (warmup + t))      (warmup >= 1)
//   w = 1 - decay                                                                                                   (warmup == 0)
// CLIP: every workgroup first derives the decision; workgroup 0 records it in clip_state (the only writer, and nobody reads
// clip_state in this launch), and on a skip every workgroup leaves before it has written anything.
// SCHED: thread 0 of every workgroup derives the step's rate from lr_state[1] and [3]; workgroup 0 records it in lr_state[0] and
// [2] (the only writer, and nobody reads those two words in this launch; [1] is advanced by the update launch).
template <bool EMA, bool CLIP, bool SCHED>
__global__ __launch_bounds__(256) void adamw_prepare_kernel(const float* __restrict__ g, const long long* __restrict__ seg_off,
                                                            float* __restrict__ seg_state, float* __restrict__ step,
                                                            float* __restrict__ ema_state, float* __restrict__ clip_state,
                                                            const double* __restrict__ clip_ws, int clip_parts, float lr, float beta1,
                                                            float beta2, float ema_decay, float ema_warmup, float gscale,
                                                            float max_norm, float* __restrict__ lr_state, SchedArgs sched) {
  const int seg = blockIdx.x;
  if constexpr (CLIP) {
    __shared__ double wsum[4];
    const ClipDecision d = clip_decide(clip_ws, clip_parts, gscale, max_norm, wsum);
    if (seg == 0 && threadIdx.x == 0) {
      clip_state[0] = d.e;
      clip_state[1] = d.norm;
      clip_state[2] = d.coef;
      if (!d.skip && d.coef < 1.0f) clip_state[3] += 1.0f;
      if (d.skip) clip_state[4] += 1.0f;
      clip_state[5] = d.skip ? 1.0f : 0.0f;
      clip_state[6] = 0.0f;
      clip_state[7] = 0.0f;
    }
    if (d.skip) return;
  }
  float* st = seg_state + (size_t)seg * 4;
  const long long a = seg_off[seg], b = seg_off[seg + 1];
  int in_graph = st[0] > 0.0f;
  if (!in_graph) {
    int nz = 0;
    for (long long i = a + threadIdx.x; i < b; i += blockDim.x) nz |= (g[i] != 0.0f);
    in_graph = __syncthreads_or(nz);
  }
  if (threadIdx.x == 0) {
    if constexpr (SCHED) {
      const SchedRate r = sched_rate(lr_state, sched);
      lr = r.lr;
      if (seg == 0) {
        lr_state[0] = r.lr;
        lr_state[2] = r.f;
      }
    }
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
      step[0] += 1.0f;                         // completed optimizer steps (the value torch keeps for every updated parameter)
      if constexpr (EMA) {
        const float t = ema_state[1] + 1.0f;
        float w = 1.0f - ema_decay;
        if (ema_warmup >= 1.0f) w = fmaxf(w, (ema_warmup - 1.0f) / (ema_warmup + t));
        ema_state[0] = w;
        ema_state[1] = t;
      }
    }
  }
}

// EMA: the average is updated from the p the thread has just formed: 5 loads + 4 stores per element instead of the 4 + 3 of the
// plain step followed by a 2 + 1 lerp launch.  CLIP: the gradient scale is the e the prepare launch left in clip_state[0]; on a
// skipped step (clip_state[5]) nothing is read or written.  SCHED: the rate is the lr_t the prepare launch left in lr_state[0], and
// one thread counts the applied step in lr_state[1] (its only writer; nobody reads it in this launch).
template <bool EMA, bool CLIP, bool SCHED>
__global__ __launch_bounds__(256) void adamw_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                    float* __restrict__ v, float* __restrict__ ema,
                                                    const long long* __restrict__ seg_off, const float* __restrict__ seg_state,
                                                    const float* __restrict__ ema_state, const float* __restrict__ clip_state,
                                                    int nseg, size_t n, size_t n_nodecay, float lr, float beta1, float beta2, float eps,
                                                    float wd0, float wd1, float gscale, float* __restrict__ lr_state) {
  if constexpr (CLIP) {
    if (clip_state[5] != 0.0f) return;
    gscale = clip_state[0];
  }
  if constexpr (SCHED) {
    lr = lr_state[0];
    if (blockIdx.x == 0 && threadIdx.x == 0) lr_state[1] += 1.0f;
  }
  __shared__ long long offS[ADAMW_LDS_SEGS + 1];
  const bool staged = nseg <= ADAMW_LDS_SEGS;
  if (staged) {
    for (int i = threadIdx.x; i <= nseg; i += blockDim.x) offS[i] = seg_off[i];
    __syncthreads();
  }
  const long long* off = staged ? offS : seg_off;
  float w = 0.0f;
  if constexpr (EMA) w = ema_state[0];
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    int lo = 0, hi = nseg - 1;                 // largest seg with off[seg] <= i
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if ((size_t)off[mid] <= i) lo = mid; else hi = mid - 1;
    }
    const float* st = seg_state + (size_t)lo * 4;
    if (st[1] == 0.0f) continue;               // parameter not in the graph: left alone (p, m, v AND ema), as torch skips .grad is None
    const float step_size = st[2], bc2s = st[3];
    const float gi = g[i] * gscale;
    const float wd = (i < n_nodecay) ? wd0 : wd1;
    float pi = p[i] * (1.0f - lr * wd);
    const float mi = beta1 * m[i] + (1.0f - beta1) * gi;
    const float vi = beta2 * v[i] + (1.0f - beta2) * gi * gi;
    const float denom = sqrtf(vi) / bc2s + eps;
    pi -= step_size * (mi / denom);
    p[i] = pi; m[i] = mi; v[i] = vi;
    if constexpr (EMA) {
      const float ei = ema[i];
      ema[i] = ei + w * (pi - ei);
    }
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

// The parameters of one step, shared by the four entries (absent parts null / 0).
struct AdamWArgs {
  float *p, *m, *v, *ema, *step, *seg_state, *ema_state, *clip_state;
  const float* g;
  const long long* seg_off;
  double* clip_ws;
  int nseg, clip_parts;
  size_t n, n_nodecay;
  float lr, beta1, beta2, eps, wd0, wd1, gscale, ema_decay, ema_warmup, max_norm;
  float* lr_state = nullptr;
  SchedArgs sched = {0.0, 0.0, 0.0, A3D_LR_CONSTANT};
};

template <bool EMA, bool CLIP, bool SCHED = false>
static int launch_adamw(const AdamWArgs& a, hipStream_t s, const char* prepare_name, const char* name) {
  hipLaunchKernelGGL((adamw_prepare_kernel<EMA, CLIP, SCHED>), dim3(a.nseg), dim3(256), 0, s, a.g, a.seg_off, a.seg_state, a.step, a.ema_state,
                     a.clip_state, a.clip_ws, a.clip_parts, a.lr, a.beta1, a.beta2, a.ema_decay, a.ema_warmup, a.gscale, a.max_norm,
                     a.lr_state, a.sched);
  int rc = check_launch(prepare_name);
  if (rc) return rc;
  const int grid = (int)std::min<size_t>((a.n + 255) / 256, 2048);
  hipLaunchKernelGGL((adamw_kernel<EMA, CLIP, SCHED>), dim3(grid), dim3(256), 0, s, a.p, a.g, a.m, a.v, a.ema, a.seg_off, a.seg_state, a.ema_state,
                     a.clip_state, a.nseg, a.n, a.n_nodecay, a.lr, a.beta1, a.beta2, a.eps, a.wd0, a.wd1, a.gscale, a.lr_state);
  return check_launch(name);
}

// The norm pass of a clipped step; *parts = the partials it leaves in clip_ws.
static int launch_grad_sqnorm(const float* g, size_t n, double* clip_ws, hipStream_t s, const char* name, int* parts) {
  const size_t head = std::min<size_t>(((16u - ((uintptr_t)g & 15u)) & 15u) / 4u, n);
  const size_t nvec = (n - head) / 4;
  // always CLIP_PARTS workgroups would leave most of them idle on a small buffer; the idle ones' partials are simply not written and
  // not read: the prepare launch is told how many there are
  *parts = (int)std::min<size_t>(std::max<size_t>((nvec + 255) / 256, 1), CLIP_PARTS);
  hipLaunchKernelGGL(grad_sqnorm_kernel, dim3(*parts), dim3(256), 0, s, g, n, head, nvec, clip_ws);
  return check_launch(name);
}

static int check_max_norm(const char* who, float max_norm) {
  if (!(max_norm > 0.0f)) {                                     // NaN fails the comparison; +inf is legal (measure only)
    set_error("%s: max_norm = %g must be > 0 (+inf: measure the norm, never clip)", who, (double)max_norm);
    return A3D_ERR_ARG;
  }
  return A3D_OK;
}

static int check_ema_ranges(const char* who, float ema_decay, float ema_warmup) {
  if (!(ema_decay >= 0.0f && ema_decay < 1.0f)) {               // NaN fails both comparisons
    set_error("%s: ema_decay = %g is outside [0, 1)", who, (double)ema_decay);
    return A3D_ERR_ARG;
  }
  if (!(ema_warmup == 0.0f || (ema_warmup >= 1.0f && std::isfinite(ema_warmup)))) {
    set_error("%s: ema_warmup = %g must be 0 (off) or a finite value >= 1", who, (double)ema_warmup);
    return A3D_ERR_ARG;
  }
  return A3D_OK;
}

}  // namespace a3d

using namespace a3d;

extern "C" int a3d_adamw_step(float* p, const float* g, float* m, float* v, float* step, const long long* seg_off,
                              float* seg_state, int nseg, size_t n, size_t n_nodecay, float lr, float beta1, float beta2, float eps,
                              float wd_nodecay, float wd_decay, float grad_scale, void* stream) {
  if (!p || !g || !m || !v || !step || !seg_off || !seg_state) { set_error("a3d_adamw_step: null pointer"); return A3D_ERR_ARG; }
  if (n == 0) return A3D_OK;
  if (nseg <= 0) { set_error("a3d_adamw_step: the flat buffer needs at least one parameter segment (nseg = %d)", nseg); return A3D_ERR_ARG; }
  const AdamWArgs a = {p, m, v, nullptr, step, seg_state, nullptr, nullptr, g, seg_off, nullptr, nseg, 0, n, n_nodecay,
                       lr, beta1, beta2, eps, wd_nodecay, wd_decay, grad_scale, 0.0f, 0.0f, 0.0f};
  return launch_adamw<false, false>(a, (hipStream_t)stream, "a3d_adamw_step(prepare)", "a3d_adamw_step");
}

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
  if (check_ema_ranges("a3d_adamw_ema_step", ema_decay, ema_warmup)) return A3D_ERR_ARG;
  if (n == 0) return A3D_OK;
  const AdamWArgs a = {p, m, v, ema, step, seg_state, ema_state, nullptr, g, seg_off, nullptr, nseg, 0, n, n_nodecay,
                       lr, beta1, beta2, eps, wd_nodecay, wd_decay, grad_scale, ema_decay, ema_warmup, 0.0f};
  return launch_adamw<true, false>(a, (hipStream_t)stream, "a3d_adamw_ema_step(prepare)", "a3d_adamw_ema_step");
}

extern "C" int a3d_adamw_clip_step(float* p, const float* g, float* m, float* v, float* ema, float* step, const long long* seg_off,
                                   float* seg_state, float* ema_state, float* clip_state, double* clip_ws, int nseg, size_t n,
                                   size_t n_nodecay, float lr, float beta1, float beta2, float eps, float wd_nodecay, float wd_decay,
                                   float grad_scale, float ema_decay, float ema_warmup, float max_norm, void* stream) {
  if (!p || !g || !m || !v || !step || !seg_off || !seg_state || !clip_state || !clip_ws) {
    set_error("a3d_adamw_clip_step: null pointer");
    return A3D_ERR_ARG;
  }
  if ((ema == nullptr) != (ema_state == nullptr)) {
    set_error("a3d_adamw_clip_step: ema and ema_state must both be given or both be null");
    return A3D_ERR_ARG;
  }
  if (nseg <= 0) {
    set_error("a3d_adamw_clip_step: the flat buffer needs at least one parameter segment (nseg = %d)", nseg);
    return A3D_ERR_ARG;
  }
  if (check_max_norm("a3d_adamw_clip_step", max_norm)) return A3D_ERR_ARG;
  if (ema && check_ema_ranges("a3d_adamw_clip_step", ema_decay, ema_warmup)) return A3D_ERR_ARG;
  if (n == 0) return A3D_OK;
  hipStream_t s = (hipStream_t)stream;
  int parts = 0;
  int rc = launch_grad_sqnorm(g, n, clip_ws, s, "a3d_adamw_clip_step(norm)", &parts);
  if (rc) return rc;
  const AdamWArgs a = {p, m, v, ema, step, seg_state, ema_state, clip_state, g, seg_off, clip_ws, nseg, parts, n, n_nodecay,
                       lr, beta1, beta2, eps, wd_nodecay, wd_decay, grad_scale, ema_decay, ema_warmup, max_norm};
  return ema ? launch_adamw<true, true>(a, s, "a3d_adamw_clip_step(prepare)", "a3d_adamw_clip_step")
             : launch_adamw<false, true>(a, s, "a3d_adamw_clip_step(prepare)", "a3d_adamw_clip_step");
}

extern "C" int a3d_adamw_sched_step(float* p, const float* g, float* m, float* v, float* ema, float* step, const long long* seg_off,
                                    float* seg_state, float* ema_state, float* clip_state, double* clip_ws, float* lr_state, int nseg,
                                    size_t n, size_t n_nodecay, int decay_kind, double warmup_steps, double total_steps,
                                    double min_ratio, float beta1, float beta2, float eps, float wd_nodecay, float wd_decay,
                                    float grad_scale, float ema_decay, float ema_warmup, float max_norm, void* stream) {
  const char* who = "a3d_adamw_sched_step";
  if (!p || !g || !m || !v || !step || !seg_off || !seg_state || !lr_state) { set_error("%s: null pointer", who); return A3D_ERR_ARG; }
  if ((ema == nullptr) != (ema_state == nullptr)) {
    set_error("%s: ema and ema_state must both be given or both be null", who);
    return A3D_ERR_ARG;
  }
  if ((clip_state == nullptr) != (clip_ws == nullptr)) {
    set_error("%s: clip_state and clip_ws must both be given or both be null", who);
    return A3D_ERR_ARG;
  }
  if (nseg <= 0) {
    set_error("%s: the flat buffer needs at least one parameter segment (nseg = %d)", who, nseg);
    return A3D_ERR_ARG;
  }
  if (decay_kind != A3D_LR_CONSTANT && decay_kind != A3D_LR_LINEAR && decay_kind != A3D_LR_COSINE) {
    set_error("%s: unknown decay_kind %d", who, decay_kind);
    return A3D_ERR_ARG;
  }
  const double limit = 16777216.0;                              // the position is an fp32 counter: exact below 2^24
  if (!(warmup_steps >= 0.0 && warmup_steps < limit && warmup_steps == std::floor(warmup_steps))) {   // NaN fails the comparisons
    set_error("%s: warmup_steps = %g must be an integer value in [0, 2^24)", who, warmup_steps);
    return A3D_ERR_ARG;
  }
  if (decay_kind != A3D_LR_CONSTANT &&
      !(total_steps > warmup_steps && total_steps < limit && total_steps == std::floor(total_steps))) {
    set_error("%s: total_steps = %g must be an integer value in (warmup_steps = %g, 2^24) for a decaying schedule", who, total_steps,
              warmup_steps);
    return A3D_ERR_ARG;
  }
  if (!(min_ratio >= 0.0 && min_ratio <= 1.0)) {
    set_error("%s: min_ratio = %g is outside [0, 1]", who, min_ratio);
    return A3D_ERR_ARG;
  }
  if (clip_state && check_max_norm(who, max_norm)) return A3D_ERR_ARG;
  if (ema && check_ema_ranges(who, ema_decay, ema_warmup)) return A3D_ERR_ARG;
  if (n == 0) return A3D_OK;
  hipStream_t s = (hipStream_t)stream;
  int parts = 0;
  if (clip_state) {
    int rc = launch_grad_sqnorm(g, n, clip_ws, s, "a3d_adamw_sched_step(norm)", &parts);
    if (rc) return rc;
  }
  AdamWArgs a = {p, m, v, ema, step, seg_state, ema_state, clip_state, g, seg_off, clip_ws, nseg, parts, n, n_nodecay,
                 0.0f, beta1, beta2, eps, wd_nodecay, wd_decay, grad_scale, ema_decay, ema_warmup, max_norm};
  a.lr_state = lr_state;
  a.sched = {warmup_steps, total_steps, min_ratio, decay_kind};
  const char* prep = "a3d_adamw_sched_step(prepare)";
  if (clip_state) return ema ? launch_adamw<true, true, true>(a, s, prep, who) : launch_adamw<false, true, true>(a, s, prep, who);
  return ema ? launch_adamw<true, false, true>(a, s, prep, who) : launch_adamw<false, false, true>(a, s, prep, who);
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
