// BatchNorm statistics of a 1x1 convolution's OUTPUT from its INPUT (CLIP ModifiedResNet bottleneck conv3 + bn3,
// model/utils/clip.py:28-43; the frozen backbone runs in train() mode, so bn3 normalises with batch statistics).
// With a [M][K] the bf16 operand the GEMM multiplies and o = a w^T:
//   sum_m o[m][c]   = w_c . (sum_m a[m][:])          sum_m o[m][c]^2 = w_c^T (a^T a) w_c
// so a K x K Gram matrix of the input -- a quarter the bytes of the output at K -> 4 K -- gives scale / shift of bn3 BEFORE conv3
// runs, and conv3's epilogue (a3d_conv1x1_bn_residual_fwd) can apply them: the raw conv3 map is never written.
//   a3d_bn_gram        per-slab partial Gram matrices + column sums (bf16 MFMA, fp32 accumulate)            1 read of x
//   a3d_bn_gram_stats  slabs reduced in double in a fixed order; per output channel the two forms in double -> [1][2][N] fp32
//                      (sum, sum of squares), the record a3d_bn_finalize reduces with nslab = 1
#include "a3d_common.h"
#include "attn_ring.h"
#include "../../include/act3d_hip.h"

namespace a3d {

// rows of a chunk: 16 KB of the input whatever K (four 16-byte loads per thread)
static constexpr int gram_chunk_rows(int K) { return 8192 / K; }

// lane (li, g) <- column col0 + li of rows row0 + 8 g .. + 7 of a row-major [rows][LD] tile: an MFMA fragment whose contraction
// index is the ROW (fs_tr_frag of fpn_sparse.hip with the row stride as a parameter)
template <int LD>
__device__ __forceinline__ s16x8 gram_tr_frag(const unsigned short* tile, int row0, int col0, int li, int g) {
  const unsigned short* p = tile + (row0 + g * 8 + (li >> 2)) * LD + col0 + (li & 3) * 4;
  const s16x4_ a = lds_tr16(p), b = lds_tr16(p + 4 * LD);
  return s16x8{a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
}

// grid nslab persistent workgroups; chunks of CH rows are dealt round-robin (workgroup i takes chunks i, i + nslab, ...: at any
// moment the grid reads one contiguous stretch of x, as bn_stats_kernel does) and fetched two chunks ahead into registers.  A thread
// owns one 16-byte column segment of the rows it stages, so the producer's scale / shift of its 8 channels and its 8 column sums
// live in registers.  Wave w owns rows 16 TR w .. of the Gram matrix (TR x K/16 MFMA tiles).  Fixed assignment, no atomics.
// Registers (hipcc 164 / 324 for K = 64 / 128, no spill): three / one workgroups per CU, which the 512 / 256 slabs of a3d_bn_gram_nslab
// need two / one of; capping K = 128 at 256 registers spills.
template <int K>
__global__ __launch_bounds__(256) void bn_gram_kernel(const unsigned short* __restrict__ x, const float* __restrict__ in_scale,
                                                      const float* __restrict__ in_shift, int in_relu, float* __restrict__ gpart,
                                                      float* __restrict__ spart, long long M, int nslab) {
  constexpr int SEGS = K / 8, RP = 256 / SEGS, U = 4, CH = RP * U;
  constexpr int LD = K == 64 ? 72 : 144;                         // halfs: the 4 rows of a transposed read on distinct banks
  constexpr int TR = K / 64, TC = K / 16;
  static_assert(CH == gram_chunk_rows(K), "chunk rows");
  __shared__ __attribute__((aligned(16))) unsigned short Xs[CH * LD];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int li = lane & 15, g = lane >> 4;
  const int seg = t % SEGS, r0 = t / SEGS;
  const long long nchunk = (M + CH - 1) / CH;
  float sc[8], sh[8], cs[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    sc[j] = in_scale ? in_scale[seg * 8 + j] : 1.f;
    sh[j] = in_scale ? in_shift[seg * 8 + j] : 0.f;
    cs[j] = 0.f;
  }
  const float relu_lo = in_relu ? 0.f : -INFINITY;
  f32x4 acc[TR][TC];
#pragma unroll
  for (int i = 0; i < TR; ++i)
#pragma unroll
    for (int c = 0; c < TC; ++c) acc[i][c] = f32x4{0.f, 0.f, 0.f, 0.f};
  auto load = [&](long long ch, uint4 (&r)[U]) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const long long row = ch * CH + u * RP + r0;
      const long long m = row < M ? row : M - 1;                  // clamped: tail rows are zeroed at the stage
      r[u] = *reinterpret_cast<const uint4*>(x + (size_t)m * K + seg * 8);
    }
  };
  auto stage = [&](long long ch, const uint4 (&r)[U]) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const long long row = ch * CH + u * RP + r0;
      unsigned int w[4] = {r[u].x, r[u].y, r[u].z, r[u].w};
      if (in_scale) {                                             // the A-operand staging of conv1x1_stream_kernel, bit for bit
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          float a = __uint_as_float(w[j] << 16) * sc[2 * j] + sh[2 * j];
          float b = __uint_as_float(w[j] & 0xFFFF0000u) * sc[2 * j + 1] + sh[2 * j + 1];
          a = fmaxf(a, relu_lo);
          b = fmaxf(b, relu_lo);
          w[j] = pk_bf16(a, b);
        }
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (row >= M) w[j] = 0u;                                  // AFTER the prologue: a padded row contributes nothing
        cs[2 * j] += __uint_as_float(w[j] << 16);
        cs[2 * j + 1] += __uint_as_float(w[j] & 0xFFFF0000u);
      }
      *reinterpret_cast<uint4*>(&Xs[(u * RP + r0) * LD + seg * 8]) = make_uint4(w[0], w[1], w[2], w[3]);
    }
  };
  auto mma = [&]() {
#pragma unroll
    for (int ks = 0; ks < CH / 32; ++ks) {
      s16x8 a[TR];
#pragma unroll
      for (int i = 0; i < TR; ++i) a[i] = gram_tr_frag<LD>(Xs, ks * 32, (wave * TR + i) * 16, li, g);
#pragma unroll
      for (int c = 0; c < TC; ++c) {
        const s16x8 b = gram_tr_frag<LD>(Xs, ks * 32, c * 16, li, g);
#pragma unroll
        for (int i = 0; i < TR; ++i) acc[i][c] = mfma_bf16_16x16x32(a[i], b, acc[i][c]);
      }
    }
  };
  uint4 ra[U], rb[U];
  long long ch = blockIdx.x;
  if (ch < nchunk) load(ch, ra);
  if (ch + nslab < nchunk) load(ch + nslab, rb);
  while (ch < nchunk) {                                           // every condition below is workgroup-uniform
    __syncthreads();                                              // the previous chunk's fragment reads are done
    stage(ch, ra);
    if (ch + 2ll * nslab < nchunk) load(ch + 2ll * nslab, ra);
    __syncthreads();
    mma();
    ch += nslab;
    if (ch >= nchunk) break;
    __syncthreads();
    stage(ch, rb);
    if (ch + 2ll * nslab < nchunk) load(ch + 2ll * nslab, rb);
    __syncthreads();
    mma();
    ch += nslab;
  }
  // lane (li, g) register r of tile (i, c): Gram row (wave TR + i) 16 + 4 g + r, column 16 c + li
  float* out = gpart + (size_t)blockIdx.x * K * K;
#pragma unroll
  for (int i = 0; i < TR; ++i)
#pragma unroll
    for (int c = 0; c < TC; ++c)
#pragma unroll
      for (int r = 0; r < 4; ++r) out[((wave * TR + i) * 16 + g * 4 + r) * K + c * 16 + li] = acc[i][c][r];
  // column sums: the RP row-groups of the workgroup added in a fixed order
  __syncthreads();
  float* red = reinterpret_cast<float*>(Xs);                      // [256][8] floats = 8 KB of the 18 KB tile
#pragma unroll
  for (int j = 0; j < 8; ++j) red[t * 8 + j] = cs[j];
  __syncthreads();
  if (t < K) {
    const int sg = t >> 3, j = t & 7;
    float s = 0.f;
    for (int r = 0; r < RP; ++r) s += red[(r * SEGS + sg) * 8 + j];
    spart[(size_t)blockIdx.x * K + t] = s;
  }
}

// grid K K / 16 + K / 16 workgroups of 16 elements x 16 slab-groups: element e of the Gram matrix (then of the column sums) over the
// slabs in double, a fixed order; four independent loads in flight per thread (one thread walking every slab is a latency chain)
__global__ __launch_bounds__(256) void bn_gram_reduce_kernel(const float* __restrict__ gpart, const float* __restrict__ spart, int nslab,
                                                             int K, double* __restrict__ work) {
  __shared__ double red[16][16];
  const int e = threadIdx.x & 15, sg = threadIdx.x >> 4;
  const int ng = K * K / 16;
  const bool is_g = (int)blockIdx.x < ng;
  const int e0 = (is_g ? (int)blockIdx.x : (int)blockIdx.x - ng) * 16 + e;
  const float* src = (is_g ? gpart : spart) + e0;
  const size_t stride = is_g ? (size_t)K * K : (size_t)K;
  double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
  int i = sg;
  for (; i + 48 < nslab; i += 64) {
    a0 += (double)src[(size_t)i * stride];
    a1 += (double)src[(size_t)(i + 16) * stride];
    a2 += (double)src[(size_t)(i + 32) * stride];
    a3 += (double)src[(size_t)(i + 48) * stride];
  }
  for (; i < nslab; i += 16) a0 += (double)src[(size_t)i * stride];
  red[sg][e] = (a0 + a1) + (a2 + a3);
  __syncthreads();
  if (sg == 0) {
    double s = 0.0;
#pragma unroll
    for (int u = 0; u < 16; ++u) s += red[u][e];
    work[(is_g ? 0 : K * K) + e0] = s;
  }
}

// grid N / 4: one wave per output channel c.  Lane k forms t_k = sum_l G[l][k] w_l (G is symmetric: the column walk is the coalesced
// one), the wave adds w_k t_k and w_k s_k -- all in double.
__global__ __launch_bounds__(256) void bn_gram_quad_kernel(const double* __restrict__ work, const unsigned short* __restrict__ w, int K, int N,
                                                           float* __restrict__ out) {
  __shared__ double wS[4][128];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c = blockIdx.x * 4 + wave;
  for (int k = lane; k < K; k += 64) wS[wave][k] = (double)bf2f(w[(size_t)c * K + k]);
  __syncthreads();
  const double* G = work;
  const double* s = work + (size_t)K * K;
  double q = 0.0, sm = 0.0;
  for (int k = lane; k < K; k += 64) {
    double t0 = 0.0, t1 = 0.0, t2 = 0.0, t3 = 0.0;
#pragma unroll 4
    for (int l = 0; l < K; l += 4) {
      t0 = fma(G[(size_t)l * K + k], wS[wave][l], t0);
      t1 = fma(G[(size_t)(l + 1) * K + k], wS[wave][l + 1], t1);
      t2 = fma(G[(size_t)(l + 2) * K + k], wS[wave][l + 2], t2);
      t3 = fma(G[(size_t)(l + 3) * K + k], wS[wave][l + 3], t3);
    }
    q = fma(wS[wave][k], (t0 + t1) + (t2 + t3), q);
    sm = fma(wS[wave][k], s[k], sm);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { q += __shfl_xor(q, o, 64); sm += __shfl_xor(sm, o, 64); }
  if (lane == 0) { out[c] = (float)sm; out[N + c] = (float)q; }
}

}  // namespace a3d

using namespace a3d;

static bool gram_serves(int K) { return K == 64 || K == 128; }

extern "C" int a3d_bn_gram_nslab(size_t M, int K) {
  if (M == 0 || !gram_serves(K)) return 0;
  // 16 KB (K = 64) / 64 KB (K = 128) of partials per slab: 8 / 16 MB at the cap, against the 134 / 67 MB the 256-image maps hold
  const size_t ch = (size_t)gram_chunk_rows(K), nchunk = (M + ch - 1) / ch;
  return (int)std::min<size_t>(nchunk, K == 64 ? 512 : 256);
}

extern "C" int a3d_bn_gram(const void* x, const float* in_scale, const float* in_shift, int in_relu, float* gpart, float* spart, size_t M,
                           int K, int nslab, void* stream) {
  if (!x || !gpart || !spart || M == 0 || !gram_serves(K) || nslab != a3d_bn_gram_nslab(M, K) || (in_scale && !in_shift) ||
      ((((uintptr_t)x | (uintptr_t)gpart | (uintptr_t)spart) & 15) != 0)) {
    set_error("a3d_bn_gram: bad argument (M=%zu K=%d nslab=%d; K in {64, 128}, nslab = a3d_bn_gram_nslab(M, K), in_shift with in_scale, "
              "16-byte aligned operands)", M, K, nslab);
    return A3D_ERR_ARG;
  }
  hipStream_t s = (hipStream_t)stream;
  if (K == 64)
    hipLaunchKernelGGL(bn_gram_kernel<64>, dim3(nslab), dim3(256), 0, s, (const unsigned short*)x, in_scale, in_shift, in_relu, gpart, spart,
                       (long long)M, nslab);
  else
    hipLaunchKernelGGL(bn_gram_kernel<128>, dim3(nslab), dim3(256), 0, s, (const unsigned short*)x, in_scale, in_shift, in_relu, gpart, spart,
                       (long long)M, nslab);
  return check_launch("a3d_bn_gram");
}

extern "C" int a3d_bn_gram_stats(const float* gpart, const float* spart, int nslab, const void* w, int K, int N, double* work, float* stats,
                                 void* stream) {
  if (!gpart || !spart || !w || !work || !stats || nslab < 1 || !gram_serves(K) || N <= 0 || (N % 4) != 0 || (((uintptr_t)work) & 7) != 0) {
    set_error("a3d_bn_gram_stats: bad argument (nslab=%d K=%d N=%d; K in {64, 128}, N a multiple of 4, work = K K + K doubles)", nslab, K, N);
    return A3D_ERR_ARG;
  }
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(bn_gram_reduce_kernel, dim3(K * K / 16 + K / 16), dim3(256), 0, s, gpart, spart, nslab, K, work);
  hipLaunchKernelGGL(bn_gram_quad_kernel, dim3(N / 4), dim3(256), 0, s, (const double*)work, (const unsigned short*)w, K, N, stats);
  return check_launch("a3d_bn_gram_stats");
}
