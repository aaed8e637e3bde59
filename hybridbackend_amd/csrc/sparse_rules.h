// The arithmetic of the sparse optimizer steps: one rule functor per optimizer and the small helpers they
// use.  Included by sparse_apply.hip, whose one row walk (slot_task) steps fp32 tables (the apply launches of
// the slot entries, the clip pass, hbk_sparse_apply_slices_n) and bf16 / fp16 tables (hbk_lowp_apply_slices_n)
// with these formulas, in this rounding and operation order; only how a table row is read and written (the
// walk's table policy) differs between the two.
#ifndef HBK_CSRC_SPARSE_RULES_H_
#define HBK_CSRC_SPARSE_RULES_H_

#include "common.h"
#include "lookup_common.h"

namespace hbk {
namespace {

__device__ inline float sqrt_v(float a) { return sqrtf(a); }
__device__ inline f32x4 sqrt_v(f32x4 a) { return f32x4{sqrtf(a.x), sqrtf(a.y), sqrtf(a.z), sqrtf(a.w)}; }

// one stepped chunk of a row: the new weights and slots
template <typename V>
struct Stepped {
  V w, s0, s1;
};

// A rule is the arithmetic of one optimizer.  Rule::setup(p) runs on wave 0 lane 0 of every
// workgroup before the barrier, Rule::state() on every thread after it; every task builds its
// Rule(p, state), and rule(w, s0, s1, g) steps one chunk of a row in place.

// Lazy Adam (s0 = m, s1 = v): the bias-corrected rate lr_t, computed once per workgroup from the
// device beta powers, is its state (one LDS word)
struct AdamParams {
  const float* powers;
  float lr, beta1, beta2, eps;
};
struct AdamRule {
  using Params = AdamParams;
  using State = float;
  static constexpr int kSlots = 2;
  static constexpr bool kStep = true;
  static constexpr bool kRowwise = false;
  float lr_t, beta1, beta2, eps;

  __device__ static float& lds_lr_t() {
    __shared__ float s_lr_t;
    return s_lr_t;
  }
  __device__ static void setup(const AdamParams& p) {
    const float b1p = p.powers[0], b2p = p.powers[1];
    lds_lr_t() = (p.lr * sqrtf(1.0f - b2p)) / (1.0f - b1p);
  }
  __device__ static float state() { return lds_lr_t(); }
  __device__ AdamRule(const AdamParams& p, float lr_t_)
      : lr_t(lr_t_), beta1(p.beta1), beta2(p.beta2), eps(p.eps) {}
  template <typename V>
  __device__ Stepped<V> operator()(V& w, V& m, V& v, V g) const {
    const float one_m_b1 = 1.0f - beta1, one_m_b2 = 1.0f - beta2;
    const V mk = beta1 * m + one_m_b1 * g;
    const V vk = beta2 * v + one_m_b2 * (g * g);
    return Stepped<V>{w - (lr_t * mk) / (sqrt_v(vk) + eps), mk, vk};
  }
};

// FTRL-Proximal (s0 = accum, s1 = linear): TF 1.15 SparseApplyFtrl[V2] on every element, each op a
// separately rounded fp32 op in TF's order; kPow: lr_power != -0.5 (powf), else sqrtf
struct FtrlParams {
  float lr, l1, two_l2, two_shrinkage, neg_lr_power;   // (2 * l2, 2 * l2_shrinkage, -lr_power: exact)
};
template <bool kPow>
struct FtrlRule {
  using Params = FtrlParams;
  struct State {};
  static constexpr int kSlots = 2;
  static constexpr bool kStep = true;
  static constexpr bool kRowwise = false;
  const FtrlParams& a;

  __device__ static void setup(const FtrlParams&) {}
  __device__ static State state() { return State{}; }
  __device__ FtrlRule(const FtrlParams& p, State) : a(p) {}
  __device__ void elem(float& w, float& acc, float& z, float g) const {
    const float gs = a.two_shrinkage == 0.0f ? g : g + a.two_shrinkage * w;
    const float na = acc + g * g;
    const float pn = kPow ? powf(na, a.neg_lr_power) : sqrtf(na);
    const float po = kPow ? powf(acc, a.neg_lr_power) : sqrtf(acc);
    const float zn = z + (gs - ((pn - po) / a.lr) * w);
    const float y = pn / a.lr + a.two_l2;
    w = (fmaxf(fminf(zn, a.l1), -a.l1) - zn) / y;
    acc = na;
    z = zn;
  }
  __device__ Stepped<float> operator()(float& w, float& acc, float& z, float g) const {
    elem(w, acc, z, g);
    return Stepped<float>{w, acc, z};
  }
  __device__ Stepped<f32x4> operator()(f32x4& w, f32x4& acc, f32x4& z, f32x4 g) const {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      float wi = w[i], ai = acc[i], zi = z[i];
      elem(wi, ai, zi, g[i]);
      w[i] = wi;
      acc[i] = ai;
      z[i] = zi;
    }
    return Stepped<f32x4>{w, acc, z};
  }
};

// The rules of the clip pass (hbk_group_lookup_bwd_apply_clipped): SGD and Adagrad with the arithmetic
// of the fused reduce's step (step_row, lookup_bwd.hip), so that a row with g' == g gets the same bits.
struct LrParams {
  float lr;
};
struct SgdRule {
  using Params = LrParams;
  struct State {};
  static constexpr int kSlots = 0;
  static constexpr bool kStep = true;
  static constexpr bool kRowwise = false;
  float lr;

  __device__ static void setup(const LrParams&) {}
  __device__ static State state() { return State{}; }
  __device__ SgdRule(const LrParams& p, State) : lr(p.lr) {}
  template <typename V>
  __device__ Stepped<V> operator()(V& w, V& s0, V& s1, V g) const {
    return Stepped<V>{w - lr * g, s0, s1};
  }
};

__device__ inline float rsqrt_v(float a) { return 1.0f / sqrtf(a); }
__device__ inline f32x4 rsqrt_v(f32x4 a) {
  return f32x4{1.0f / sqrtf(a.x), 1.0f / sqrtf(a.y), 1.0f / sqrtf(a.z), 1.0f / sqrtf(a.w)};
}

// s0 = the accumulator
struct AdagradRule {
  using Params = LrParams;
  struct State {};
  static constexpr int kSlots = 1;
  static constexpr bool kStep = true;
  static constexpr bool kRowwise = false;
  float lr;

  __device__ static void setup(const LrParams&) {}
  __device__ static State state() { return State{}; }
  __device__ AdagradRule(const LrParams& p, State) : lr(p.lr) {}
  template <typename V>
  __device__ Stepped<V> operator()(V& w, V& s0, V& s1, V g) const {
    const V acc = s0 + g * g;
    return Stepped<V>{w - (lr * g) * rsqrt_v(acc), acc, s1};
  }
};

// Row-wise Adagrad (include/hbk.h, hbk_group_lookup_bwd_rowwise_adagrad): ONE accumulator word per row, fp32
// [rows, 1] (no pitch: word r belongs to row r).  kRowwise: the row walk reads that word once per row, sums
// g * g over the row's lane group (the clip prologue's order) and hands the rule the row's sum; the rule
// returns the new accumulator and the row's one rate.
struct RowwiseParams {
  float lr, eps;
};
struct RowwiseAdagradRule {
  using Params = RowwiseParams;
  struct State {};
  static constexpr int kSlots = 0;   // (no slot of the table's shape)
  static constexpr bool kStep = true;
  static constexpr bool kRowwise = true;
  float lr, eps;

  __device__ static void setup(const RowwiseParams&) {}
  __device__ static State state() { return State{}; }
  __device__ RowwiseAdagradRule(const RowwiseParams& p, State) : lr(p.lr), eps(p.eps) {}
  // a: the row's accumulator, s: the sum of g * g over the row, dim as a float; *rate: lr / (sqrt(a') + eps)
  __device__ float row(float a, float s, float fdim, float* rate) const {
    const float na = a + s / fdim;
    *rate = lr / (sqrtf(na) + eps);
    return na;
  }
};

// The clip prologue (include/hbk.h, hbk_group_lookup_fwd_clipped): the sums of a row over its lane
// group, each lane's chunk in element order, then a butterfly over the group's lanes (xor 1, 2, 4, ..):
// both lanes of a pair add the same two values, so every lane of the group ends with the same bits.
__device__ inline float chunk_sum(float a) { return a; }
__device__ inline float chunk_sum(f32x4 a) { return ((a.x + a.y) + a.z) + a.w; }
__device__ inline float group_sum(float s, int lpr_log2) {
  for (int o = 1; o < (1 << lpr_log2); o <<= 1) s = s + __shfl_xor(s, o, kWave);
  return s;
}

}  // namespace
}  // namespace hbk

#endif  // HBK_CSRC_SPARSE_RULES_H_
