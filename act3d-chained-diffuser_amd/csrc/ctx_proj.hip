// Context K/V projections of up to two attention layers that read ONE context, in one wave-local launch.
//
// The ghost-point stream runs two RelativeCrossAttentionLayers per pyramid level on the same context rows X [B][N][60]
// (act3d.py ghost_point_cross_attn_pyramid -> layers.py:293-310 on MultiheadCustomAttention, multihead_custom_attention.py:251-275:
// key is value, packed k,v projection).  Per layer that is proj_rope_split_kernel<4,60,true> with grid (Npad/64, 2, B): the K block and
// the V block are different workgroups that each stage the same 64 rows of X, re-stage their weight block from L2 and walk five
// workgroup barriers per tile -- X is read four times per level and the kernel is bound by neither HBM nor the matrix pipe.
//
// Here (the restructuring single_query_wave.hip applied to the query stream's key pass):
//   * persistent workgroups, grid (nsplit, B): the 2 nl weight blocks (W_k | W_v of each layer, 60 x 60 fp32) and their biases are
//     staged in LDS ONCE per workgroup;
//   * a WAVE owns 16 keys end to end, no __syncthreads() in the key loop.  Every product is formed transposed,
//         T^T[c][key] = sum_cin W[c][cin] X[key][cin]      (A = W rows from LDS, B = X rows straight from global memory),
//     so an MFMA lane (li = lane & 15, g = lane >> 4) holds, for key li, the 16 channels ct * 16 + g * 4 + r of a block: both
//     channels of every RoPE pair sit in one lane and the rotation is register arithmetic;
//   * X is read ONCE for all 2 nl blocks, the next group's rows are in flight while the current one computes; the 8 sincos per lane
//     depend only on xyz and are shared by the nl K blocks (V blocks are not rotated);
//   * the contraction is 15 k-steps per 16-channel tile, not 16: channels 0-47 arrive as three float4 per lane (k-step members
//     s * 16 + 4 g' + e over the four lane groups g'), channels 48-59 as three scalars 48 + 4 j + g -- 4 x 60 MFMAs per 16 keys;
//   * a lane's 16 channels straddle heads (head width 15): one wave-private LDS round trip (wavefront-scope fence, no s_barrier) puts
//     a key's 16 head-dim values side by side; a lane then splits eight of them and writes the 16-byte hi and lo segments of the key's
//     64-byte rows16 record hi(16) | lo(16) -- the 16 keys of one head are 1 KB contiguous.
// Arithmetic: exact-f32 MFMA 16x16x4 from a zero accumulator, then acc + bias (scale = 1 for k and v), then y0 cs - y1 sn,
// y1 cs + y0 sn, then rp_split_f16's hi / lo -- the function a3d_proj_rope_split16 computes, with the k-steps of the contraction in
// another order.  Output conventions are write_operand_formats16's (rope.hip): rows n in [N, Npad) zero in channels 0-14, channel 15
// of the K hi part 0, of the V hi part 1.0 on every row below Npad, all lo pads 0, nothing outside [0, Npad) written.
// E = 60, H = 4 only (the E = 120 model's eight blocks do not fit LDS).
#include "a3d_common.h"
#include "../../include/act3d_hip.h"
#include <algorithm>

namespace a3d {

constexpr int CP_E = 60, CP_H = 4;
constexpr int CP_THREADS = 512, CP_WAVES = CP_THREADS / 64;   // one workgroup per CU: 2 waves per SIMD
constexpr int CP_LD = 68;     // row stride (floats) of the LDS weight blocks [64][CP_LD] and of the wave-private tiles [16][CP_LD]
constexpr int CP_MAX_BLOCKS = 4;

struct CtxProjBlocks {        // block 2 l = K of layer l, 2 l + 1 = V of layer l
  const float* W[CP_MAX_BLOCKS];          // [60][ldw]
  const float* bias[CP_MAX_BLOCKS];       // [60] or null
  unsigned short* out[CP_MAX_BLOCKS];     // rows16 [B][H][Npad][32]
};

// as single_query_wave.hip's sqw_opaque_zero / sqw_wave_sync: an integer that is new in every loop iteration (LDS addresses derived
// from it are not loop-invariant, so the weight fragments are re-read per step instead of being hoisted into 64 VGPRs per block), and
// the ordering of one wave's LDS writes before its reads of other lanes' data
__device__ __forceinline__ int cp_opaque_zero() {
  int z = 0;
  asm volatile("" : "+v"(z));
  return z;
}
__device__ __forceinline__ void cp_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// rope.hip's rp_split_f16: hi = RNE fp16 pair, lo = fp16(x - hi) in one rounding (x * 1.0 - hi is exact in fp32), subnormals kept
__device__ __forceinline__ void cp_split_f16(float a, float b, unsigned int& hi, unsigned int& lo) {
  typedef __attribute__((ext_vector_type(2))) float cp_f32x2;
  typedef __attribute__((ext_vector_type(2))) _Float16 cp_h16x2;
  hi = __builtin_bit_cast(unsigned int, __builtin_convertvector((cp_f32x2){a, b}, cp_h16x2));
#ifdef A3D_NO_FMA_MIX
  const cp_h16x2 hh = __builtin_bit_cast(cp_h16x2, hi);
  lo = __builtin_bit_cast(unsigned int, __builtin_convertvector((cp_f32x2){a - (float)hh[0], b - (float)hh[1]}, cp_h16x2));
#else
  asm("v_fma_mixlo_f16 %0, %1, 1.0, -%3 op_sel:[0,0,0] op_sel_hi:[0,0,1]\n\t"
      "v_fma_mixhi_f16 %0, %2, 1.0, -%3 op_sel:[0,0,1] op_sel_hi:[0,0,1]"
      : "=&v"(lo)
      : "v"(a), "v"(b), "v"(hi));
#endif
}

// the lane's key row in B-operand order: x[s] = X[n][s * 16 + g * 4 .. + 3] (s < 3), t[j] = X[n][48 + 4 j + g]; zero for n >= N
struct CpKey { float4 x[3]; float t[3]; float px, py, pz; };
__device__ __forceinline__ CpKey cp_load_key(const float* __restrict__ X, int ldx, const float* __restrict__ xyz, int b, int n, int N,
                                             int g) {
  CpKey k;
  const bool valid = n < N;
  const float* row = X + ((size_t)b * N + (valid ? n : 0)) * ldx;
#pragma unroll
  for (int s = 0; s < 3; ++s) {
    k.x[s] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (valid) k.x[s] = *reinterpret_cast<const float4*>(row + s * 16 + g * 4);
  }
#pragma unroll
  for (int j = 0; j < 3; ++j) k.t[j] = valid ? row[48 + 4 * j + g] : 0.f;
  k.px = k.py = k.pz = 0.f;
  if (xyz && valid) {
    const float* p = xyz + ((size_t)b * N + n) * 3;
    k.px = p[0]; k.py = p[1]; k.pz = p[2];
  }
  return k;
}

// acc[ct][r] = sum_cin W[ct * 16 + g * 4 + r][cin] X[key li][cin]: 15 k-steps per 16-channel tile.  The weight fragments are double
// buffered by hand (the next 16 input channels' four float4 are in flight while the current sixteen MFMAs issue); the scheduling
// barriers keep the compiler from hoisting all of them in front of the MFMAs.
__device__ __forceinline__ void cp_project(const float* Wb, const CpKey& k, int li, int g, f32x4 (&acc)[4]) {
#pragma unroll
  for (int ct = 0; ct < 4; ++ct) acc[ct] = f32x4{0.f, 0.f, 0.f, 0.f};
  float4 a[4], an[4];
#pragma unroll
  for (int ct = 0; ct < 4; ++ct) a[ct] = *reinterpret_cast<const float4*>(&Wb[(ct * 16 + li) * CP_LD + g * 4]);
#pragma unroll
  for (int s = 0; s < 3; ++s) {
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) an[ct] = *reinterpret_cast<const float4*>(&Wb[(ct * 16 + li) * CP_LD + (s + 1) * 16 + g * 4]);
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) acc[ct] = mfma_f32_16x16x4(a[ct].x, k.x[s].x, acc[ct]);
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) acc[ct] = mfma_f32_16x16x4(a[ct].y, k.x[s].y, acc[ct]);
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) acc[ct] = mfma_f32_16x16x4(a[ct].z, k.x[s].z, acc[ct]);
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) acc[ct] = mfma_f32_16x16x4(a[ct].w, k.x[s].w, acc[ct]);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) a[ct] = an[ct];
  }
  // input channels 48 + 4 j + g: the block's columns 48-63 are stored as [g][j], so the lane's three weights are one float4 again
#pragma unroll
  for (int ct = 0; ct < 4; ++ct) acc[ct] = mfma_f32_16x16x4(a[ct].x, k.t[0], acc[ct]);
#pragma unroll
  for (int ct = 0; ct < 4; ++ct) acc[ct] = mfma_f32_16x16x4(a[ct].y, k.t[1], acc[ct]);
#pragma unroll
  for (int ct = 0; ct < 4; ++ct) acc[ct] = mfma_f32_16x16x4(a[ct].z, k.t[2], acc[ct]);
}

// grid (nsplit, B), 512 threads.  NL layers -> 2 NL blocks.
template <int NL>
__global__ __launch_bounds__(CP_THREADS) void ctx_kv_proj_kernel(const float* __restrict__ X, int ldx, const float* __restrict__ xyz,
                                                                 CtxProjBlocks blk, int ldw, const float* __restrict__ freq, int N,
                                                                 int Npad, int nsplit) {
  constexpr int NB = 2 * NL, E = CP_E, H = CP_H;
  typedef __attribute__((ext_vector_type(4))) unsigned int cp_u32x4;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* Ws = smem;                                   // [NB][64][CP_LD], zero beyond row / column 60
  float* Bs = Ws + NB * 64 * CP_LD;                   // [NB][64]
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  float* Tw = Bs + NB * 64 + wave * 16 * CP_LD;       // this wave's [16 keys][CP_LD] tile
  const int li = lane & 15, g = lane >> 4;
  const int b = blockIdx.y, sp = blockIdx.x;
  const bool rotate = xyz != nullptr;
  // 16-key groups of this workgroup; a workgroup without one stages nothing
  const int ngroups = Npad >> 4;
  const int g_beg = (int)((long long)ngroups * sp / nsplit), g_end = (int)((long long)ngroups * (sp + 1) / nsplit);
  if (g_beg >= g_end) return;
  CpKey cur;
  int grp = g_beg + wave;
  if (grp < g_end) cur = cp_load_key(X, ldx, xyz, b, grp * 16 + li, N, g);
  // parameters living in a flat optimizer buffer are only 4-byte aligned: scalar loads.  All of a thread's 8 NB weights are in flight
  // before the first LDS write (one L2 round trip for the whole stage, not one per element): thread t holds column t & 63 of rows
  // (t >> 6) + 8 i.  Columns 48 + 4 j + g are stored at 48 + 4 g + j (cp_project's last step).
  {
    constexpr int PER = 64 * 64 / CP_THREADS;
    const int c = t & 63, r0 = t >> 6, cc = c - 48;
    const int col = c < 48 ? c : 48 + (cc & 3) * 4 + (cc >> 2);
    float wv[NB][PER];
#pragma unroll
    for (int j = 0; j < NB; ++j)
#pragma unroll
      for (int i = 0; i < PER; ++i) {
        const int r = r0 + (CP_THREADS / 64) * i;
        wv[j][i] = (r < E && c < E) ? blk.W[j][(size_t)r * ldw + c] : 0.f;
      }
    float bv = 0.f;
#pragma unroll
    for (int j = 0; j < NB; ++j)
      if ((t >> 6) == j && c < E && blk.bias[j]) bv = blk.bias[j][c];
#pragma unroll
    for (int j = 0; j < NB; ++j)
#pragma unroll
      for (int i = 0; i < PER; ++i) Ws[(j * 64 + r0 + (CP_THREADS / 64) * i) * CP_LD + col] = wv[j][i];
    if (t < NB * 64) Bs[t] = bv;
  }
  // the lane's RoPE constants: pair (ct, j) = channels c, c + 1 with c = ct * 16 + g * 4 + 2 j -> axis c / 20, frequency (c % 20) / 2
  float fq[4][2];
  int axis[4][2];
#pragma unroll
  for (int ct = 0; ct < 4; ++ct)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int c = ct * 16 + g * 4 + 2 * j;
      fq[ct][j] = 0.f;
      axis[ct][j] = 0;
      if (rotate && c < E) {
        axis[ct][j] = c / (E / 3);
        fq[ct][j] = freq[(c - axis[ct][j] * (E / 3)) >> 1];
      }
    }
  // the wave-private tile holds a key's row head-major: channel c = 15 h + d at column (d >> 3) * 32 + h * 8 + (d & 7), so the eight
  // values of a (key, head, half) item are two aligned float4, and a 16-lane read group (8 keys x 2 halves) touches 64 distinct
  // banks.  The lane's channels 60-63 (ct = 3, g = 3: zero weight rows) go to the four d = 15 slots, which the readers replace.
  int wcol[4][4];
#pragma unroll
  for (int ct = 0; ct < 4; ++ct)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int c = ct * 16 + g * 4 + r;
      const int h = c < E ? c / HD : c - E, d = c < E ? c - h * HD : HD;
      wcol[ct][r] = li * CP_LD + (d >> 3) * 32 + h * 8 + (d & 7);
    }
  __syncthreads();
  // the lane's two (key, head, half) items per block: lanes 2 k, 2 k + 1 hold the halves of key k; heads 2 i + (lane >> 5)
  const int wkey = (lane >> 1) & 15, whalf = lane & 1, whsel = lane >> 5;
  for (; grp < g_end; grp += CP_WAVES) {
    const int n = grp * 16 + li;
    CpKey nxt = cur;
    if (grp + CP_WAVES < g_end) nxt = cp_load_key(X, ldx, xyz, b, n + CP_WAVES * 16, N, g);   // one step ahead: hides the HBM round trip
    const bool live = grp * 16 < N;                    // wave-uniform: a group of pad rows only is written without being computed
    const bool valid = n < N;
    float cs[4][2], sn[4][2];
    if (rotate && live) {
#pragma unroll
      for (int ct = 0; ct < 4; ++ct)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const float p = axis[ct][j] == 0 ? cur.px : (axis[ct][j] == 1 ? cur.py : cur.pz);
          fast_sincos(p * fq[ct][j], &sn[ct][j], &cs[ct][j]);
        }
    }
    const int oz = cp_opaque_zero();
#pragma unroll
    for (int j = 0; j < NB; ++j) {
      f32x4 acc[4];
      if (live) {
        cp_project(Ws + j * 64 * CP_LD + oz, cur, li, g, acc);
#pragma unroll
        for (int ct = 0; ct < 4; ++ct) {
          const float4 bv = *reinterpret_cast<const float4*>(&Bs[j * 64 + ct * 16 + g * 4 + oz]);
          acc[ct] = f32x4{acc[ct][0] + bv.x, acc[ct][1] + bv.y, acc[ct][2] + bv.z, acc[ct][3] + bv.w};
          if (rotate && !(j & 1)) {
#pragma unroll
            for (int p = 0; p < 2; ++p) {
              const float y0 = acc[ct][2 * p], y1 = acc[ct][2 * p + 1];
              acc[ct][2 * p] = y0 * cs[ct][p] - y1 * sn[ct][p];
              acc[ct][2 * p + 1] = y1 * cs[ct][p] + y0 * sn[ct][p];
            }
          }
          if (!valid) acc[ct] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
      } else {
#pragma unroll
        for (int ct = 0; ct < 4; ++ct) acc[ct] = f32x4{0.f, 0.f, 0.f, 0.f};
      }
      cp_wave_sync();                                   // the previous block's tile reads come before these writes
#pragma unroll
      for (int ct = 0; ct < 4; ++ct)
#pragma unroll
        for (int r = 0; r < 4; ++r) Tw[wcol[ct][r]] = acc[ct][r];
      cp_wave_sync();
      const float pad = (j & 1) ? 1.0f : 0.f;          // channel 15 of the hi part: the value rows' ones channel
      unsigned short* __restrict__ out = blk.out[j];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int h = 2 * i + whsel;
        const float* src = &Tw[wkey * CP_LD + whalf * 32 + h * 8];
        const float4 v0 = *reinterpret_cast<const float4*>(src), v1 = *reinterpret_cast<const float4*>(src + 4);
        unsigned int ohi[4], olo[4];
        cp_split_f16(v0.x, v0.y, ohi[0], olo[0]);
        cp_split_f16(v0.z, v0.w, ohi[1], olo[1]);
        cp_split_f16(v1.x, v1.y, ohi[2], olo[2]);
        cp_split_f16(v1.z, whalf ? pad : v1.w, ohi[3], olo[3]);
        unsigned short* dst = out + (((size_t)b * H + h) * Npad + grp * 16 + wkey) * 32 + whalf * 8;
        *reinterpret_cast<cp_u32x4*>(dst) = cp_u32x4{ohi[0], ohi[1], ohi[2], ohi[3]};
        *reinterpret_cast<cp_u32x4*>(dst + 16) = cp_u32x4{olo[0], olo[1], olo[2], olo[3]};
      }
    }
    cur = nxt;
  }
}

}  // namespace a3d

using namespace a3d;

extern "C" int a3d_ctx_kv_proj16_splits(int B, int Npad) {
  static int cus = 0;
  if (cus == 0) {
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0)
      n = 256;
    cus = n;
  }
  if (B <= 0 || Npad <= 0) return 1;
  // one workgroup per CU; every wave of a workgroup gets at least one 16-key group
  const int want = cdiv(cus, B), most = std::max(1, (Npad >> 4) / CP_WAVES);
  return std::max(1, std::min(want, most));
}

extern "C" int a3d_ctx_kv_proj16(const float* X, int ldx, const float* xyz, const float* W0, const float* bias0, void* Krows0,
                                 void* Vrows0, const float* W1, const float* bias1, void* Krows1, void* Vrows1, int ldw,
                                 const float* freq, int nl, int B, int N, int Npad, int E, int H, int nsplit, void* stream) {
  const char* fn = "a3d_ctx_kv_proj16";
  if (nl < 1 || nl > 2 || E != CP_E || H != CP_H) {
    set_error("%s: serves 1 or 2 layers of the E = 60, H = 4 model (nl=%d E=%d H=%d)", fn, nl, E, H);
    return A3D_ERR_ARG;
  }
  if (B <= 0 || B > 65535 || N <= 0 || Npad < N || (Npad % 64) != 0 || nsplit < 0 || nsplit > 65535) {
    set_error("%s: bad argument (B=%d N=%d Npad=%d nsplit=%d; need Npad %% 64 == 0, Npad >= N, B and nsplit <= 65535)", fn, B, N, Npad,
              nsplit);
    return A3D_ERR_ARG;
  }
  if (!X || (((uintptr_t)X) & 15) || (ldx & 3) || ldx < E || ldw < E) {
    set_error("%s: X must be 16-byte aligned with ldx %% 4 == 0, ldx >= E, ldw >= E (ldx=%d ldw=%d)", fn, ldx, ldw);
    return A3D_ERR_ARG;
  }
  if (!W0 || !Krows0 || !Vrows0 || (nl == 2 && (!W1 || !Krows1 || !Vrows1)) || (xyz && !freq)) {
    set_error("%s: null pointer (weights and both outputs of every layer are required; xyz needs freq)", fn);
    return A3D_ERR_ARG;
  }
  if (((((uintptr_t)Krows0) | ((uintptr_t)Vrows0) | ((uintptr_t)Krows1) | ((uintptr_t)Vrows1)) & 15) ||
      ((((uintptr_t)W0) | ((uintptr_t)W1) | ((uintptr_t)bias0) | ((uintptr_t)bias1) | ((uintptr_t)xyz) | ((uintptr_t)freq)) & 3)) {
    set_error("%s: outputs must be 16-byte aligned, fp32 inputs 4-byte aligned", fn);
    return A3D_ERR_ARG;
  }
  CtxProjBlocks blk;
  const float* Wl[2] = {W0, W1};
  const float* bl[2] = {bias0, bias1};
  void* Kl[2] = {Krows0, Krows1};
  void* Vl[2] = {Vrows0, Vrows1};
  for (int l = 0; l < 2; ++l) {
    const bool on = l < nl;
    blk.W[2 * l] = on ? Wl[l] : nullptr;
    blk.W[2 * l + 1] = on ? Wl[l] + (size_t)E * ldw : nullptr;
    blk.bias[2 * l] = on ? bl[l] : nullptr;
    blk.bias[2 * l + 1] = (on && bl[l]) ? bl[l] + E : nullptr;
    blk.out[2 * l] = on ? (unsigned short*)Kl[l] : nullptr;
    blk.out[2 * l + 1] = on ? (unsigned short*)Vl[l] : nullptr;
  }
  if (nsplit == 0) nsplit = a3d_ctx_kv_proj16_splits(B, Npad);
  const size_t lds = ((size_t)2 * nl * 64 * CP_LD + 2 * nl * 64 + CP_WAVES * 16 * CP_LD) * sizeof(float);
  static bool attr_set = false;
  if (!attr_set) {
    (void)hipFuncSetAttribute((const void*)ctx_kv_proj_kernel<1>, hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024);
    (void)hipFuncSetAttribute((const void*)ctx_kv_proj_kernel<2>, hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024);
    attr_set = true;
  }
  const dim3 grid(nsplit, B);
  if (nl == 1)
    hipLaunchKernelGGL(ctx_kv_proj_kernel<1>, grid, dim3(CP_THREADS), lds, (hipStream_t)stream, X, ldx, xyz, blk, ldw, freq, N, Npad, nsplit);
  else
    hipLaunchKernelGGL(ctx_kv_proj_kernel<2>, grid, dim3(CP_THREADS), lds, (hipStream_t)stream, X, ldx, xyz, blk, ldw, freq, N, Npad, nsplit);
  return check_launch(fn);
}
