// Host-side launch plan of the attention cores (attention.hip, attention_bwd.hip, attention16.hip, attention8.hip): what every
// launcher does before it names its kernel.  Each entry validates in ONE order -- shapes, dropout arguments, pointers, then whatever
// is its own -- and launches nothing before all of that has passed; messages carry the name of the entry that was called.
#pragma once
#include "a3d_common.h"
#include <stdio.h>
#include <stdlib.h>
#include <type_traits>

namespace a3d {

// qmod: modulus of Lqp (16 for the forwards, 64 for the backwards); sp_max: largest Sp the kernel's key bitmask holds (0: no limit)
static inline int attn_check_shapes(const char* fn, int B, int H, int Lq, int Lqp, int S, int Sp, int nsplit, int qmod, int sp_max) {
  if (B <= 0 || H <= 0 || Lq <= 0 || Lqp < Lq || (Lqp % qmod) != 0 || S <= 0 || Sp < S || (Sp % 64) != 0 || nsplit < 1 ||
      nsplit > 64 || (sp_max && Sp > sp_max)) {
    char lim[32] = "";
    if (sp_max) snprintf(lim, sizeof(lim), ", Sp <= %d", sp_max);
    set_error("%s: bad argument (B=%d H=%d Lq=%d Lqp=%d S=%d Sp=%d nsplit=%d; need Lqp %% %d == 0, Sp %% 64 == 0%s)", fn, B, H, Lq,
              Lqp, S, Sp, nsplit, qmod, lim);
    return A3D_ERR_ARG;
  }
  return A3D_OK;
}

// Dropout of the attention weights as the kernels take it.  Off (no state, or p == 0) is (nullptr, 0, 0, 1.0f); a state with p outside
// [0, 1) is refused.  `required`: the entry exists for dropout only (the bf16x3 _dropout entries) and refuses a NULL state.
struct AttnDrop {
  const unsigned long long* state = nullptr;
  unsigned int site = 0u, thr = 0u;
  float scale = 1.0f;
};
static inline int attn_drop_decode(const char* fn, const unsigned long long* state, unsigned int site, float p, bool required,
                                   AttnDrop* d) {
  *d = AttnDrop{};
  if (!state) {
    if (required) { set_error("%s: null dropout state", fn); return A3D_ERR_ARG; }
    return A3D_OK;
  }
  uint32_t thr;
  float scale;
  const int rc = drop_params(fn, p, &thr, &scale);
  if (rc == A3D_OK && p > 0.f) *d = AttnDrop{state, site, thr, scale};
  return rc;
}

// Tiles per wave and the two grids, from the shapes alone.  QT: two 16-query tiles per wave (128 queries per workgroup; forward, dQ)
// once the query set fills them.  KT: two key tiles per wave (dK / dV) when enough 128-key workgroups are left to fill the chip.
struct AttnTiles {
  int QT, KT;
  dim3 gq, gk;        // forward / dQ grid (query tiles x key splits), dK / dV grid (key tiles)
};
static inline AttnTiles attn_tiles(int B, int H, int Lq, int Lqp, int Sp, int nsplit) {
  AttnTiles t;
  t.QT = Lq > 64 ? 2 : 1;
  t.KT = ((size_t)B * H * (Sp / 128) >= 1024 && Lq > 16) ? 2 : 1;
  t.gq = dim3(xcd_grid(B * H, cdiv(Lqp, 64 * t.QT) * nsplit));
  t.gk = dim3(xcd_grid(B * H, cdiv(Sp, 64 * t.KT)));
  return t;
}

// Split workspace Op [nsplit][rows][HDP] | Mp [nsplit][rows] | Lp [nsplit][rows], rows = B * H * Lqp: the size query
// (a3d_attn_fwd_ws_floats) and the carve read the same offsets.
struct AttnWsPlan { size_t mp, lp, floats; };       // float offsets of Mp and Lp (Op at 0), and the total
static inline AttnWsPlan attn_ws_plan(int B, int H, int Lqp, int nsplit) {
  const size_t n = (size_t)nsplit * B * H * Lqp;
  return AttnWsPlan{n * HDP, n * HDP + n, n * HDP + 2 * n};
}
struct AttnWs { float *Op, *Mp, *Lp; };
static inline AttnWs attn_ws_carve(float* ws, int B, int H, int Lqp, int nsplit) {
  const AttnWsPlan p = attn_ws_plan(B, H, Lqp, nsplit);
  return AttnWs{ws, ws ? ws + p.mp : nullptr, ws ? ws + p.lp : nullptr};
}

// Run-time flag -> template argument: f is a generic lambda and receives a std::bool_constant / std::integral_constant, so a
// launcher names its kernel once, as kernel<decltype(flag)::value, ...>.  with_int<2, 1>(QT, f) passes 2 if QT == 2 and 1 otherwise
// (the last value listed is the default).
template <class F>
static inline void with_bool(bool v, F&& f) {
  if (v) f(std::true_type{}); else f(std::false_type{});
}
template <int V0, int... Vs, class F>
static inline void with_int(int v, F&& f) {
  if constexpr (sizeof...(Vs) == 0) f(std::integral_constant<int, V0>{});
  else if (v == V0) f(std::integral_constant<int, V0>{});
  else with_int<Vs...>(v, f);
}

// A3D_ATTN_FAST=1: the single-part P / G kernels of the split-fp16 family (read once)
static inline bool attn_fast() {
  static const bool fast = getenv("A3D_ATTN_FAST") && atoi(getenv("A3D_ATTN_FAST")) != 0;
  return fast;
}

}  // namespace a3d
