// Sparse optimizer steps with two slots per row after the grouped backward: Lazy Adam
// (tf.contrib.opt.LazyAdamOptimizer's sparse apply, TF 1.15; hbk_group_lookup_bwd_adam) and FTRL-Proximal
// (SparseApplyFtrl[V2], TF 1.15; hbk_group_lookup_bwd_ftrl).
//
// Two phases.  (1) The backward in its emit form (hbk_group_lookup_bwd_apply, apply_lr = 0) writes every
// column's distinct rows, their summed gradient rows and n_unique -- into the caller's buffers or, step
// only, into buffers carved from this call's workspace.  Every reduce plan, the deterministic modes,
// weighted columns and segmented inputs come from there unchanged, and so does the guarantee that each
// distinct row appears exactly once (Adam is not additive: a row stepped twice would decay its moments
// twice; FTRL would add g^2 to its accumulator twice).  (2) ONE apply launch for up to kSlotMaxCols
// columns: sparse_adam_apply_kernel or sparse_ftrl_apply_kernel.
//
// Both optimizers share everything but their arithmetic: one kernel body (slot_apply_body), one row
// walk (slot_task) and one host driver (slot_apply); a rule (AdamRule, FtrlRule) holds what differs.
// Work is counted in wave tasks: a task is kSlotItems rows per lane group of one column, a lane group
// holds one row (f32x4 chunks when dim % 4 == 0 and every address is 16-byte aligned, scalar chunks
// otherwise -- the reduce's rule, make_rowshape).  Wave 0 of every workgroup reads the columns'
// n_unique from the device and scans their task counts into LDS; the grid is sized from the
// host-known capacities only and walks the tasks grid-stride, so the call needs no host sync and can
// be captured in a graph.  A lane issues the w / slot / slot / g loads of all its kSlotItems rows
// before any arithmetic: random rows are bound by the request rate (~49 G requests/s), so
// what matters is how many are in flight.  grad_rows and unique_rows are read once (non-temporal).
// Adam's bias-corrected rate lr_t is computed once per workgroup from the device beta powers; the
// powers advance after the apply, in stream order (adam_finish_kernel), when the call asks for it.
// FTRL has no device state besides its slots; its lr_power != -0.5 form (powf) is a separate
// instantiation, so the default form carries no powf code.
//
// Row-wise Adagrad (hbk_group_lookup_bwd_rowwise_adagrad) rides the same walk with ONE slot of another
// shape: an fp32 [rows, 1] accumulator.  Its rule (RowwiseAdagradRule, kRowwise) is not element-wise:
// slot_task loads the row's accumulator word with the task's other loads (every lane of the row's group
// reads the same address: one request), sums g * g over the lane group in the clip prologue's order
// (chunk_sum, then the group_sum butterfly), and lane 0 of the group stores the word back.  Everything
// kRowwise adds sits under `if constexpr`, so the other instantiations are the instructions they were.
//
// The walk is also parameterised by a table policy: how a lane chunk of a table row is read and written.
// Fp32Rows is the plain load and store of every kernel above (SlotCol, SlotArgs; their instructions did not
// change when the policy came).  LowpRows (LowpCol, LowpArgs; hbk_lowp_apply_slices_n, lowp_apply_kernel<Rule>)
// reads bf16 / fp16 rows upcast exactly and rounds the stepped row back -- to nearest even, or for bf16
// stochastically with noise keyed by (seed, step, column, row, element); the element helpers are lowp_elems.h's,
// which the 16-bit forward (lowp_tables.hip) shares.  It has no clip, no pitch and no emit rule.  The two slice
// entries share the rule dispatch (dispatch_rule), the launch packer (launch_slices over fill_slot_cols) and the
// checks both word alike; each keeps the refusals of its own.
#include <string.h>

#include <algorithm>
#include <vector>

#include "common.h"
#include "lookup_common.h"
#include "lowp_elems.h"
#include "sparse_rules.h"

namespace hbk {
namespace {

constexpr int kSlotMaxCols = 64;    // columns per apply launch (kernarg: 64 descriptors)
constexpr int kSlotBlock = 256;
constexpr int kSlotWaves = kSlotBlock / kWave;
constexpr int kSlotItems = 4;       // rows per lane group in flight
constexpr int kSlotBlocksPerCU = 8;
static_assert(kSlotMaxCols <= kWave, "one lane per column in the task scan");

// one column of a two-slot apply: Adam's (m, v) or FTRL's (accum, linear) in s0 / s1
struct SlotCol {
  float* w;
  float* s0;
  float* s1;
  const int64_t* urows;
  const float* grows;       // [cap, dim] contiguous
  const int32_t* nu;
  int64_t rows;
  int32_t cap;              // n_ids: n_unique never exceeds it
  int32_t dim;
  int32_t pitch;            // floats between rows of w, s0 and s1
  int32_t lpr_log2;
  int32_t vec4;
  float max_norm;           // > 0: the clip pass's c (clip kernels only; 0: the column is not clipped)
};

// the kernel arguments of one apply launch: the columns and the rule's parameters P
template <typename P>
struct SlotArgs {
  SlotCol c[kSlotMaxCols];
  P p;
  int32_t n_cols;
};

// one column of a 16-bit apply (hbk_lowp_apply_slices_n): rows of bf16 / fp16 elements, dim apart; fp32 slots
struct LowpCol {
  uint16_t* w;
  float* s0;
  float* s1;
  const int64_t* urows;
  const float* grows;   // [cap, dim] contiguous
  const int32_t* nu;
  int64_t rows;
  int32_t cap;
  int32_t dim;
  int32_t index;        // the column's index in the CALL (the noise is keyed by it)
  uint8_t lpr_log2;
  uint8_t vec4;
  uint8_t bf16;
};

struct LowpRound {
  const uint32_t* step;   // NULL: round to nearest even
  uint32_t seed;
};

template <typename P>
struct LowpArgs {
  LowpCol c[kSlotMaxCols];
  P p;
  LowpRound round;
  int32_t n_cols;
};

// The table policies: how the walk reads and writes a lane chunk of a table row.  A policy names its column and
// its kernel arguments, is built once per thread from the arguments (after the barrier), and builds a Task once
// per task.  load(c, off, V()) reads the chunk at element `off` of c.w as fp32; task.row(r) is row r's word of
// rounding noise and task.store(x, p, that word, k0) writes x at p as elements k0 .. of the row.  Fp32Rows holds
// nothing and compiles to the plain loads and stores -- to the very instructions of the kernels before the
// policies, which is why store takes the value first (an assignment evaluates its right side first) and row takes
// the row by reference (an argument passed by value is marked as defined, and that alone reorders the FTRL kernels).
struct Fp32Rows {
  using Col = SlotCol;
  template <typename P>
  using Args = SlotArgs<P>;
  template <typename P>
  __device__ explicit Fp32Rows(const SlotArgs<P>&) {}
  __device__ static int32_t pitch(const SlotCol& c) { return c.pitch; }
  template <typename V>
  __device__ static V load(const SlotCol& c, int64_t off, V) { return *reinterpret_cast<const V*>(c.w + off); }
  struct Task {
    __device__ Task(const Fp32Rows&, const SlotCol&) {}
    template <typename V>
    __device__ void store(V x, float* p, uint32_t, int) const { *reinterpret_cast<V*>(p) = x; }
    __device__ uint32_t row(const int64_t&) const { return 0u; }
  };
};

// 16-bit rows: upcast on the load; on the store round to nearest even or, for bf16, stochastically with the noise
// of include/hbk.h, keyed by (seed, step, the column's index, the row, the element).  The step word is read once
// per thread, behind the barrier and so before the advance launch -- behind the apply in stream order -- writes it.
struct LowpRows {
  using Col = LowpCol;
  template <typename P>
  using Args = LowpArgs<P>;
  bool stochastic;
  uint32_t seed, step;
  template <typename P>
  __device__ explicit LowpRows(const LowpArgs<P>& a)
      : stochastic(a.round.step != nullptr), seed(a.round.seed), step(stochastic ? *a.round.step : 0u) {}
  __device__ static int32_t pitch(const LowpCol& c) { return c.dim; }
  template <typename V>
  __device__ static V load(const LowpCol& c, int64_t off, V) { return load_w(c.w + off, c.bf16 != 0, V()); }
  struct Task {
    bool bf16, stochastic;
    uint32_t nbase;
    __device__ Task(const LowpRows& t, const LowpCol& c)
        : bf16(c.bf16 != 0), stochastic(t.stochastic),
          nbase(stochastic ? noise_base(t.seed, t.step, c.index) : 0u) {}
    template <typename V>
    __device__ void store(V x, uint16_t* p, uint32_t rowh, int k0) const {
      store_w(p, x, bf16, stochastic, rowh, k0);
    }
    __device__ uint32_t row(const int64_t& r) const { return stochastic ? noise_row(nbase, r) : 0u; }
  };
};

// The rules (sparse_rules.h): AdamRule, FtrlRule<>, SgdRule, AdagradRule,
// RowwiseAdagradRule, their Params, Stepped<> and the sums chunk_sum / group_sum.  A rule is the arithmetic
// of one optimizer: Rule::setup(p) runs on wave 0 lane 0 of every workgroup before the barrier,
// Rule::state() on every thread after it; every task builds its Rule(p, state), and rule(w, s0, s1, g)
// steps one chunk of a row in place.

// TF's _finish: beta1^t, beta2^t -> beta1^(t+1), beta2^(t+1), one fp32 product each
__global__ void adam_finish_kernel(float* powers, float beta1, float beta2) {
  if (threadIdx.x == 0) {
    powers[0] = powers[0] * beta1;
    powers[1] = powers[1] * beta2;
  }
}

// The clip pass (hbk_group_lookup_bwd_apply_clipped) steps with SgdRule / AdagradRule -- the arithmetic of
// the fused reduce's step (step_row, lookup_bwd.hip), so that a row with g' == g gets the same bits -- or
// with the emit rule, which steps nothing and writes g' back over the gradient row.
struct EmitRule {
  using Params = LrParams;
  struct State {};
  static constexpr int kSlots = 0;
  static constexpr bool kStep = false;
  static constexpr bool kRowwise = false;

  __device__ static void setup(const LrParams&) {}
  __device__ static State state() { return State{}; }
  __device__ EmitRule(const LrParams&, State) {}
};

// Row-wise Adagrad (RowwiseAdagradRule): the row's ONE accumulator word sits in SlotCol::s0 as fp32 [rows, 1].

// g' of one lane chunk from the pre-step row chunk x and the summed gradient chunk g (TF's clip_by_norm
// differentiated once per distinct row).  Every lane of the group takes part (lanes without a row
// pass zeros).
template <typename V>
__device__ inline V clip_grad(V x, V g, float c, int lpr_log2) {
  const float s = group_sum(chunk_sum(x * x), lpr_log2);
  const float n = s > 0.0f ? sqrtf(s) : 0.0f;
  const float m = fmaxf(n, c);
  // d = sum_k G_k * ((x_k * c) / m) / m: every term rounded on its own, then summed as s is
  const float d = group_sum(chunk_sum((g * ((x * c) / m)) / m), lpr_log2);
  const V tangent = (g / m) * c;
  if (!(s > 0.0f && n >= c)) return tangent;
  const float ds = (-d * 0.5f) / n;
  return tangent + (2.0f * ds) * x;
}

// one task: rows base + k * groups + grp (k < kSlotItems) of column c; W floats per lane chunk.
// Rule::kSlots slots are read and written; Rule::kStep false: nothing is stepped.  CLIP: the rows of a
// column with max_norm > 0 step with clip_grad's g', which is written back over the gradient row in
// every form (the IndexedSlices of a clipped column are the gradient its rows were stepped with).
// Rule::kRowwise: c.s0 is one word per row -- every lane of the row's group loads that same word with the
// task's other loads, the group sums g * g (after the clip: g' * g'), lane 0 of the group stores the word.
// Table: the rows' policy (the 16-bit one has no clip, no emit rule and no pitch of its own).
template <typename V, int W, typename Rule, bool CLIP, typename Table>
__device__ inline void slot_task(const Table& table, const typename Table::Col& c, int64_t base, int64_t n,
                                 const Rule& rule) {
  const int lane = lane_id();
  const int lpr = c.lpr_log2;
  const int grp = lane >> lpr;
  const int sub = lane & ((1 << lpr) - 1);
  const int groups = kWave >> lpr;
  const bool lane_on = sub * W < c.dim;
  int64_t r[kSlotItems];
  bool on[kSlotItems];
#pragma unroll
  for (int k = 0; k < kSlotItems; ++k) {
    const int64_t u = base + (int64_t)k * groups + grp;
    on[k] = lane_on && u < n;
    r[k] = on[k] ? __builtin_nontemporal_load(c.urows + u) : 0;
    on[k] = on[k] && (uint64_t)r[k] < (uint64_t)c.rows;   // (the reduce only emits rows of the table)
  }
  V w[kSlotItems], s0[kSlotItems], s1[kSlotItems], g[kSlotItems];
  if constexpr (CLIP || Rule::kSlots < 2) {
#pragma unroll
    for (int k = 0; k < kSlotItems; ++k) w[k] = s0[k] = s1[k] = g[k] = zero_v<V>();
  }
  float acc[Rule::kRowwise ? kSlotItems : 1], sq[Rule::kRowwise ? kSlotItems : 1];
  if constexpr (Rule::kRowwise) {
#pragma unroll
    for (int k = 0; k < kSlotItems; ++k) acc[k] = 0.0f;
  }
#pragma unroll
  for (int k = 0; k < kSlotItems; ++k) {
    if (!on[k]) continue;
    const int64_t u = base + (int64_t)k * groups + grp;
    const int64_t off = r[k] * Table::pitch(c) + sub * W;
    if constexpr (Rule::kStep || CLIP) w[k] = Table::load(c, off, V());
    if constexpr (Rule::kSlots >= 1) s0[k] = *reinterpret_cast<const V*>(c.s0 + off);
    if constexpr (Rule::kSlots >= 2) s1[k] = *reinterpret_cast<const V*>(c.s1 + off);
    if constexpr (Rule::kRowwise) acc[k] = c.s0[r[k]];
    g[k] = __builtin_nontemporal_load(reinterpret_cast<const V*>(c.grows + u * c.dim + sub * W));
  }
  if constexpr (CLIP) {
    if (c.max_norm != 0.0f) {   // (uniform: one column per task)
#pragma unroll
      for (int k = 0; k < kSlotItems; ++k) g[k] = clip_grad<V>(w[k], g[k], c.max_norm, lpr);
    }
  }
  if constexpr (Rule::kRowwise) {
    // every lane of the wave takes part (lanes without a row or past dim pass +0.0f)
#pragma unroll
    for (int k = 0; k < kSlotItems; ++k) sq[k] = group_sum(chunk_sum(g[k] * g[k]), lpr);
  }
  const typename Table::Task rows(table, c);
#pragma unroll
  for (int k = 0; k < kSlotItems; ++k) {
    if (!on[k]) continue;
    if constexpr (CLIP) {
      if (c.max_norm != 0.0f) {
        const int64_t u = base + (int64_t)k * groups + grp;
        *reinterpret_cast<V*>(const_cast<float*>(c.grows) + u * c.dim + sub * W) = g[k];
      }
    }
    const uint32_t rowh = rows.row(r[k]);
    if constexpr (Rule::kRowwise) {
      float rate;
      const float na = rule.row(acc[k], sq[k], (float)c.dim, &rate);
      if (sub == 0) c.s0[r[k]] = na;
      const int64_t off = r[k] * Table::pitch(c) + sub * W;
      rows.store(w[k] - rate * g[k], c.w + off, rowh, sub * W);
    } else if constexpr (Rule::kStep) {
      const int64_t off = r[k] * Table::pitch(c) + sub * W;
      const Stepped<V> o = rule(w[k], s0[k], s1[k], g[k]);
      if constexpr (Rule::kSlots >= 1) *reinterpret_cast<V*>(c.s0 + off) = o.s0;
      if constexpr (Rule::kSlots >= 2) *reinterpret_cast<V*>(c.s1 + off) = o.s1;
      rows.store(o.w, c.w + off, rowh, sub * W);
    }
  }
}

// wave 0 of a workgroup: the columns' n_unique (clamped to the capacity) into s_n and the inclusive
// prefix of their task counts into s_end
template <typename Col>
__device__ inline void scan_tasks(const Col* cols, int n_cols, int lane, int64_t* s_end, int64_t* s_n) {
  int64_t tasks = 0;
  if (lane < n_cols) {
    const Col& c = cols[lane];
    const int64_t n = min(max(__builtin_nontemporal_load(c.nu), 0), c.cap);
    const int64_t rpt = (int64_t)(kWave >> c.lpr_log2) * kSlotItems;
    tasks = (n + rpt - 1) / rpt;
    s_n[lane] = n;
  }
#pragma unroll
  for (int d = 1; d < kWave; d <<= 1) {
    const int64_t t = __shfl_up(tasks, d, kWave);
    if (lane >= d) tasks += t;
  }
  if (lane < n_cols) s_end[lane] = tasks;
}

// every wave: the tasks of the scan, grid-stride; task(col, first row, n_unique) runs one
template <typename Col, typename Task>
__device__ inline void walk_tasks(const Col* cols, int n_cols, const int64_t* s_end, const int64_t* s_n,
                                  Task task) {
  const int64_t total = s_end[n_cols - 1];
  int c = 0;
  for (int64_t t = (int64_t)blockIdx.x * kSlotWaves + threadIdx.x / kWave; t < total;
       t += (int64_t)gridDim.x * kSlotWaves) {
    while (s_end[c] <= t) ++c;   // (t only grows: the column only moves forward)
    const Col& col = cols[c];
    const int64_t t0 = c == 0 ? 0 : s_end[c - 1];
    const int64_t base = (t - t0) * ((int64_t)(kWave >> col.lpr_log2) * kSlotItems);
    task(col, base, s_n[c]);
  }
}

// the body of every apply kernel: the scan, the rule's setup, the barrier, the walk
template <typename Rule, bool CLIP = false, typename Table = Fp32Rows>
__device__ inline void slot_apply_body(const typename Table::template Args<typename Rule::Params>& a) {
  __shared__ int64_t s_end[kSlotMaxCols];   // inclusive prefix of the columns' task counts
  __shared__ int64_t s_n[kSlotMaxCols];     // their n_unique (clamped to the capacity)
  if (threadIdx.x < kWave) {
    const int lane = (int)threadIdx.x;
    scan_tasks(a.c, a.n_cols, lane, s_end, s_n);
    if (lane == 0) Rule::setup(a.p);
  }
  __syncthreads();
  const typename Rule::State st = Rule::state();
  const Table table(a);
  walk_tasks(a.c, a.n_cols, s_end, s_n, [&](const typename Table::Col& col, int64_t base, int64_t n) {
    if (col.vec4) {
      slot_task<f32x4, 4, Rule, CLIP>(table, col, base, n, Rule(a.p, st));
    } else {
      slot_task<float, 1, Rule, CLIP>(table, col, base, n, Rule(a.p, st));
    }
  });
}

__global__ __launch_bounds__(kSlotBlock) void sparse_adam_apply_kernel(SlotArgs<AdamParams> a) {
  slot_apply_body<AdamRule>(a);
}

template <bool kPow>
__global__ __launch_bounds__(kSlotBlock) void sparse_ftrl_apply_kernel(SlotArgs<FtrlParams> a) {
  slot_apply_body<FtrlRule<kPow>>(a);
}

// the clip pass: the walk of the two-slot kernels with the clip prologue in front of the rule
__global__ __launch_bounds__(kSlotBlock) void sparse_adam_clip_kernel(SlotArgs<AdamParams> a) {
  slot_apply_body<AdamRule, true>(a);
}

template <bool kPow>
__global__ __launch_bounds__(kSlotBlock) void sparse_ftrl_clip_kernel(SlotArgs<FtrlParams> a) {
  slot_apply_body<FtrlRule<kPow>, true>(a);
}

__global__ __launch_bounds__(kSlotBlock) void sparse_sgd_clip_kernel(SlotArgs<LrParams> a) {
  slot_apply_body<SgdRule, true>(a);
}

__global__ __launch_bounds__(kSlotBlock) void sparse_adagrad_clip_kernel(SlotArgs<LrParams> a) {
  slot_apply_body<AdagradRule, true>(a);
}

__global__ __launch_bounds__(kSlotBlock) void sparse_emit_clip_kernel(SlotArgs<LrParams> a) {
  slot_apply_body<EmitRule, true>(a);
}

__global__ __launch_bounds__(kSlotBlock) void sparse_rowwise_adagrad_apply_kernel(SlotArgs<RowwiseParams> a) {
  slot_apply_body<RowwiseAdagradRule>(a);
}

__global__ __launch_bounds__(kSlotBlock) void sparse_rowwise_adagrad_clip_kernel(SlotArgs<RowwiseParams> a) {
  slot_apply_body<RowwiseAdagradRule, true>(a);
}

// the walk over 16-bit rows (hbk_lowp_apply_slices_n), every rule
template <typename Rule>
__global__ __launch_bounds__(kSlotBlock) void lowp_apply_kernel(LowpArgs<typename Rule::Params> a) {
  slot_apply_body<Rule, false, LowpRows>(a);
}

// the step counter of the stochastic rounding, behind the apply in stream order
__global__ void lowp_advance_kernel(uint32_t* step) {
  if (threadIdx.x == 0) step[0] = step[0] + 1u;
}

inline size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

// the step-only buffers of column c (unique_rows, grad_rows) behind the emit-form workspace
size_t slot_bytes(const hbk_lookup_grad_column_t& h) {
  if (h.grad_rows != nullptr || h.n_ids <= 0) return 0;
  return align256((size_t)h.n_ids * 8) + align256((size_t)h.n_ids * h.dim * 4);
}

// the columns as the emit form sees them: step-only columns get (non-NULL, aligned) stand-ins so the
// query counts the emitting reduce, not the step-only one
std::vector<hbk_lookup_grad_column_t> emit_form(int32_t n_cols, const hbk_lookup_grad_column_t* cols) {
  std::vector<hbk_lookup_grad_column_t> e(cols, cols + n_cols);
  for (hbk_lookup_grad_column_t& h : e) {
    if (h.grad_rows == nullptr) {
      h.unique_rows = reinterpret_cast<int64_t*>((uintptr_t)256);
      h.grad_rows = reinterpret_cast<float*>((uintptr_t)256);
    }
    h.accum = nullptr;
  }
  return e;
}

// every host check of a one-slot call's columns (nm.s1 == NULL: row-wise Adagrad's accumulators, fp32
// [rows, 1] in s0), before any device work; the apply's row shapes.  The accumulator is one 4-byte word
// per row: it does not enter the alignment bits of the row shape (table, grad_rows and the pitch do).
int check_row_slot_columns(const SlotNames& nm, int32_t n_cols, const hbk_lookup_grad_column_t* cols,
                           float* const* s0, std::vector<RowShape>* shapes) {
  const char* who = nm.who;
  HBK_REQUIRE(n_cols == 0 || cols != nullptr, "%s: cols is NULL", who);
  HBK_REQUIRE(n_cols == 0 || s0 != nullptr, "%s: the %s array is NULL", who, nm.s0);
  std::vector<uintptr_t> seen;
  seen.reserve((size_t)n_cols * 2);
  shapes->assign((size_t)n_cols, RowShape{});
  for (int32_t c = 0; c < n_cols; ++c) {
    const hbk_lookup_grad_column_t& h = cols[c];
    HBK_REQUIRE(s0[c] != nullptr, "%s: column %d: %s is NULL", who, c, nm.s0);
    HBK_REQUIRE(((uintptr_t)s0[c] & 3) == 0, "%s: column %d: %s must be 4-byte aligned", who, c, nm.s0);
    HBK_REQUIRE(s0[c] != h.table, "%s: column %d: %s is the table", who, c, nm.s0);
    HBK_REQUIRE(h.accum == nullptr, "%s: column %d: accum must be NULL (%s's slot is the %s array)", who, c,
                nm.opt, nm.s0);
    HBK_REQUIRE(h.n_ids == 0 || h.table != nullptr, "%s: column %d: table is NULL", who, c);
    HBK_REQUIRE(h.n_ids < (1ll << 30), "%s: column %d: more than 2^30-1 ids", who, c);
    HBK_REQUIRE(h.dim >= 1, "%s: column %d: dim must be >= 1", who, c);
    HBK_REQUIRE(h.table_pitch == 0 || h.table_pitch >= h.dim,
                "%s: column %d: table_pitch %d is smaller than dim %d", who, c, h.table_pitch, h.dim);
    HBK_REQUIRE(h.n_ids == 0 || (h.unique_rows != nullptr) == (h.grad_rows != nullptr),
                "%s: column %d: unique_rows and grad_rows go together", who, c);
    const int32_t pitch = h.table_pitch > 0 ? h.table_pitch : h.dim;
    HBK_REQUIRE(h.n_ids <= 0 ||
                    make_rowshape(h.dim,
                                  (uintptr_t)h.table | (uintptr_t)h.grad_rows | ((uintptr_t)(uint32_t)pitch * 4),
                                  &(*shapes)[(size_t)c]),
                "%s: column %d: dim %d needs more than 64 lanes per row (at most 256 with 16-byte "
                "aligned table / grad_rows / pitch, 64 otherwise)", who, c, h.dim);
    if (h.table != nullptr) seen.push_back((uintptr_t)h.table);
    seen.push_back((uintptr_t)s0[c]);
  }
  std::sort(seen.begin(), seen.end());
  HBK_REQUIRE(std::adjacent_find(seen.begin(), seen.end()) == seen.end(),
              "%s: two columns name the same table or %s (%s is not additive: a row stepped twice "
              "in one call would race)", who, nm.s0, nm.opt);
  return HBK_OK;
}

// every host check of a two-slot call's columns, before any device work; the apply's row shapes
int check_slot_columns(const SlotNames& nm, int32_t n_cols, const hbk_lookup_grad_column_t* cols,
                       float* const* s0, float* const* s1, std::vector<RowShape>* shapes) {
  const char* who = nm.who;
  HBK_REQUIRE(n_cols == 0 || cols != nullptr, "%s: cols is NULL", who);
  HBK_REQUIRE(n_cols == 0 || (s0 != nullptr && s1 != nullptr), "%s: the %s / %s arrays are NULL", who,
              nm.s0, nm.s1);
  std::vector<uintptr_t> seen;
  seen.reserve((size_t)n_cols * 3);
  shapes->assign((size_t)n_cols, RowShape{});
  for (int32_t c = 0; c < n_cols; ++c) {
    const hbk_lookup_grad_column_t& h = cols[c];
    HBK_REQUIRE(s0[c] != nullptr, "%s: column %d: %s is NULL", who, c, nm.s0);
    HBK_REQUIRE(s1[c] != nullptr, "%s: column %d: %s is NULL", who, c, nm.s1);
    HBK_REQUIRE(s0[c] != s1[c], "%s: column %d: %s and %s are the same buffer", who, c, nm.s0, nm.s1);
    HBK_REQUIRE(s0[c] != h.table, "%s: column %d: %s is the table", who, c, nm.s0);
    HBK_REQUIRE(s1[c] != h.table, "%s: column %d: %s is the table", who, c, nm.s1);
    HBK_REQUIRE(h.accum == nullptr, "%s: column %d: accum must be NULL (%s's slots are the %s / %s arrays)",
                who, c, nm.opt, nm.s0, nm.s1);
    HBK_REQUIRE(h.n_ids == 0 || h.table != nullptr, "%s: column %d: table is NULL", who, c);
    HBK_REQUIRE(h.n_ids < (1ll << 30), "%s: column %d: more than 2^30-1 ids", who, c);
    HBK_REQUIRE(h.dim >= 1, "%s: column %d: dim must be >= 1", who, c);
    HBK_REQUIRE(h.table_pitch == 0 || h.table_pitch >= h.dim,
                "%s: column %d: table_pitch %d is smaller than dim %d", who, c, h.table_pitch, h.dim);
    HBK_REQUIRE(h.n_ids == 0 || (h.unique_rows != nullptr) == (h.grad_rows != nullptr),
                "%s: column %d: unique_rows and grad_rows go together", who, c);
    // the apply's row shape, checked here -- before the reduce runs -- with the alignment phase 2
    // sees (step-only slices are carved 256-byte aligned from the workspace: they add no bits)
    const int32_t pitch = h.table_pitch > 0 ? h.table_pitch : h.dim;
    HBK_REQUIRE(h.n_ids <= 0 ||
                    make_rowshape(h.dim,
                                  (uintptr_t)h.table | (uintptr_t)s0[c] | (uintptr_t)s1[c] |
                                      (uintptr_t)h.grad_rows | ((uintptr_t)(uint32_t)pitch * 4),
                                  &(*shapes)[(size_t)c]),
                "%s: column %d: dim %d needs more than 64 lanes per row (at most 256 with 16-byte "
                "aligned table / %s / %s / grad_rows / pitch, 64 otherwise)", who, c, h.dim, nm.s0, nm.s1);
    if (h.table != nullptr) seen.push_back((uintptr_t)h.table);
    seen.push_back((uintptr_t)s0[c]);
    seen.push_back((uintptr_t)s1[c]);
  }
  std::sort(seen.begin(), seen.end());
  HBK_REQUIRE(std::adjacent_find(seen.begin(), seen.end()) == seen.end(),
              "%s: two columns name the same table, %s or %s (%s is not additive: a row stepped twice "
              "in one call would race)", who, nm.s0, nm.s1, nm.opt);
  return HBK_OK;
}

// workspace of a two-slot call: the emit form's reduce, then the step-only slices (256-byte aligned
// each).  The backward's size query runs once per call: `slots` is where the slices begin.
struct SlotLayout {
  size_t slots, total;
};
SlotLayout slot_layout(int32_t n_cols, const hbk_lookup_grad_column_t* cols) {
  SlotLayout l = {0, 0};
  if (n_cols <= 0 || cols == nullptr) return l;
  const std::vector<hbk_lookup_grad_column_t> e = emit_form(n_cols, cols);
  l.slots = align256(hbk_group_lookup_bwd_workspace_bytes(n_cols, e.data()));
  l.total = l.slots;
  for (int32_t c = 0; c < n_cols; ++c) l.total += slot_bytes(cols[c]);
  if (l.total != 0) l.total += 256;
  return l;
}
size_t slot_workspace_bytes(int32_t n_cols, const hbk_lookup_grad_column_t* cols) {
  return slot_layout(n_cols, cols).total;
}

// phase 1: the reduce in its emit form (validates the rest of the columns); *e: the columns as the
// apply reads them (step-only slices carved from the workspace)
int run_emit_form(const char* who, int32_t n_cols, const hbk_lookup_grad_column_t* cols,
                  void* workspace, size_t workspace_bytes, hbk_stream_t stream_,
                  std::vector<hbk_lookup_grad_column_t>* e) {
  const SlotLayout l = slot_layout(n_cols, cols);
  const size_t need = l.total;
  HBK_REQUIRE(need == 0 || (workspace != nullptr && workspace_bytes >= need),
              "%s: workspace too small: need %zu bytes, got %zu", who, need, workspace_bytes);
  HBK_REQUIRE(((uintptr_t)workspace & 7) == 0, "%s: workspace must be 8-byte aligned", who);
  e->assign(cols, cols + n_cols);
  char* const base = reinterpret_cast<char*>(((uintptr_t)workspace + 255) & ~(uintptr_t)255);
  char* slot = base + l.slots;
  for (int32_t c = 0; c < n_cols; ++c) {
    hbk_lookup_grad_column_t& h = (*e)[(size_t)c];
    h.accum = nullptr;
    if (h.grad_rows == nullptr && h.n_ids > 0) {
      h.unique_rows = reinterpret_cast<int64_t*>(slot);
      slot += align256((size_t)h.n_ids * 8);
      h.grad_rows = reinterpret_cast<float*>(slot);
      slot += align256((size_t)h.n_ids * h.dim * 4);
    }
  }
  if (n_cols == 0) return HBK_OK;
  return hbk_group_lookup_bwd_apply(n_cols, e->data(), HBK_APPLY_SGD, 0.0f, base,
                                    workspace_bytes - (size_t)(base - (char*)workspace), stream_);
}

// what a descriptor takes from the host column of its table kind: the capacity, and the table's own fields
inline int64_t capacity_of(const hbk_lookup_grad_column_t& h) { return h.n_ids; }
inline int64_t capacity_of(const hbk_lowp_slices_column_t& h) { return h.capacity; }
inline void set_table(SlotCol& d, const hbk_lookup_grad_column_t& h, int32_t c, const float* max_norms) {
  d.w = h.table;
  d.pitch = h.table_pitch > 0 ? h.table_pitch : h.dim;
  d.max_norm = max_norms != nullptr ? max_norms[c] : 0.0f;
}
inline void set_table(LowpCol& d, const hbk_lowp_slices_column_t& h, int32_t c, const float*) {
  d.w = static_cast<uint16_t*>(h.table);
  d.index = c;
  d.bf16 = h.table_dtype == HBK_LOWP_BF16;
}

// phase 2's descriptors of columns c0 .. c1 (those with rows to step) into out; the number of them
// and the grid the launch needs.  s0 / s1: NULL where the rule has no such slot.
template <typename Col, typename HostCol>
int fill_slot_cols(const HostCol* e, const std::vector<RowShape>& shapes, float* const* s0, float* const* s1,
                   int32_t c0, int32_t c1, Col* out, unsigned* blocks, const float* max_norms = nullptr) {
  int64_t tasks = 0;
  int k = 0;
  for (int32_t c = c0; c < c1; ++c) {
    const HostCol& h = e[c];
    const int64_t cap = capacity_of(h);
    if (cap <= 0 || h.rows <= 0) continue;
    Col& d = out[k];
    set_table(d, h, c, max_norms);
    d.s0 = s0 != nullptr ? s0[c] : nullptr;
    d.s1 = s1 != nullptr ? s1[c] : nullptr;
    d.urows = h.unique_rows;
    d.grows = h.grad_rows;
    d.nu = h.n_unique;
    d.rows = h.rows;
    d.cap = (int32_t)cap;
    d.dim = h.dim;
    const RowShape& shape = shapes[(size_t)c];   // (validated before the reduce)
    d.lpr_log2 = shape.lpr_log2;
    d.vec4 = shape.vec4;
    const int64_t rpt = (int64_t)(kWave >> shape.lpr_log2) * kSlotItems;
    tasks += (std::min<int64_t>(cap, h.rows) + rpt - 1) / rpt;
    ++k;
  }
  const int64_t want = (tasks + kSlotWaves - 1) / kSlotWaves;
  *blocks = (unsigned)std::max<int64_t>(
      1, std::min<int64_t>(want, (int64_t)device_cus() * kSlotBlocksPerCU));
  return k;
}

// one slot call (two slots, or nm.s1 == s1 == NULL: one): every host check (n_cols, check() for the hyperparameters, the columns), the
// emit-form reduce, then one apply launch per kSlotMaxCols columns -- launch(args, blocks, stream)
// sets args.p and launches the rule's kernel.  run_empty: go on with n_cols = 0 (what follows the
// apply still has to run)
// max_norms: NULL, or the clip of every column (the apply is then a clip kernel)
template <typename P, typename Check, typename Launch>
int slot_apply(const SlotNames& nm, Check check, bool run_empty, int32_t n_cols,
               const hbk_lookup_grad_column_t* cols, float* const* s0, float* const* s1, Launch launch,
               void* workspace, size_t workspace_bytes, hbk_stream_t stream_,
               const float* max_norms = nullptr) {
  HBK_REQUIRE(n_cols >= 0, "%s: n_cols must be >= 0, got %d", nm.who, n_cols);
  int rc = check();
  if (rc != HBK_OK) return rc;
  std::vector<RowShape> shapes;
  rc = nm.s1 != nullptr ? check_slot_columns(nm, n_cols, cols, s0, s1, &shapes)
                        : check_row_slot_columns(nm, n_cols, cols, s0, &shapes);
  if (rc != HBK_OK) return rc;
  if (n_cols == 0 && !run_empty) return HBK_OK;
  std::vector<hbk_lookup_grad_column_t> e;
  rc = run_emit_form(nm.who, n_cols, cols, workspace, workspace_bytes, stream_, &e);
  if (rc != HBK_OK) return rc;
  hipStream_t stream = as_stream(stream_);
  for (int32_t c0 = 0; c0 < n_cols; c0 += kSlotMaxCols) {
    SlotArgs<P> a;
    memset(&a, 0, sizeof(a));
    unsigned blocks = 0;
    a.n_cols = fill_slot_cols(e.data(), shapes, s0, s1, c0, std::min(n_cols, c0 + kSlotMaxCols), a.c, &blocks,
                              max_norms);
    if (a.n_cols == 0) continue;
    launch(a, blocks, stream);
    HBK_HIP_OK(hipGetLastError());
  }
  return HBK_OK;
}

}  // namespace
}  // namespace hbk

namespace hbk {
// the hyperparameters of a Lazy Adam call (host only; shared with the sharded backward, which checks
// them before its exchanges)
int adam_check(const hbk_adam_t* adam, float lr, const char* who) {
  HBK_REQUIRE(adam != nullptr, "%s: adam is NULL", who);
  HBK_REQUIRE(adam->beta1 >= 0.0f && adam->beta1 < 1.0f,
              "%s: beta1 must be in [0, 1), got %g", who, (double)adam->beta1);
  HBK_REQUIRE(adam->beta2 >= 0.0f && adam->beta2 < 1.0f,
              "%s: beta2 must be in [0, 1), got %g", who, (double)adam->beta2);
  HBK_REQUIRE(adam->epsilon >= 0.0f && adam->epsilon <= 3.402823466e38f,
              "%s: epsilon must be finite and >= 0, got %g", who, (double)adam->epsilon);
  HBK_REQUIRE(adam->beta_powers != nullptr && ((uintptr_t)adam->beta_powers & 3) == 0,
              "%s: beta_powers must be a device fp32 [2]", who);
  HBK_REQUIRE(lr != 0.0f, "%s: lr must be != 0 (the emit form alone is hbk_group_lookup_bwd with "
              "apply_lr = 0)", who);
  return HBK_OK;
}

// the hyperparameters of an FTRL call, refused as TF's kernel refuses them (host only; shared with the
// sharded backward)
int ftrl_check(const hbk_ftrl_t* ftrl, float lr, const char* who) {
  constexpr float kMax = 3.402823466e38f;
  HBK_REQUIRE(ftrl != nullptr, "%s: ftrl is NULL", who);
  HBK_REQUIRE(lr > 0.0f && lr <= kMax, "%s: lr must be finite and > 0, got %g", who, (double)lr);
  HBK_REQUIRE(ftrl->l1 >= 0.0f && ftrl->l1 <= kMax, "%s: l1 must be finite and >= 0, got %g", who,
              (double)ftrl->l1);
  HBK_REQUIRE(ftrl->l2 >= 0.0f && ftrl->l2 <= kMax, "%s: l2 must be finite and >= 0, got %g", who,
              (double)ftrl->l2);
  HBK_REQUIRE(ftrl->l2_shrinkage >= 0.0f && ftrl->l2_shrinkage <= kMax,
              "%s: l2_shrinkage must be finite and >= 0, got %g", who, (double)ftrl->l2_shrinkage);
  HBK_REQUIRE(ftrl->lr_power <= 0.0f && ftrl->lr_power >= -kMax,
              "%s: lr_power must be finite and <= 0, got %g", who, (double)ftrl->lr_power);
  return HBK_OK;
}

// the hyperparameters of a row-wise Adagrad call (host only; shared with the sharded backward)
int rowwise_adagrad_check(const hbk_rowwise_adagrad_t* opt, float lr, const char* who) {
  constexpr float kMax = 3.402823466e38f;
  HBK_REQUIRE(opt != nullptr, "%s: rowwise_adagrad is NULL", who);
  HBK_REQUIRE(lr != 0.0f && lr >= -kMax && lr <= kMax, "%s: lr must be finite and != 0, got %g", who,
              (double)lr);
  HBK_REQUIRE(opt->epsilon >= 0.0f && opt->epsilon <= kMax, "%s: epsilon must be finite and >= 0, got %g",
              who, (double)opt->epsilon);
  return HBK_OK;
}
}  // namespace hbk

namespace hbk {
namespace {
// The clip of a call (max_norms[c] of hbk_group_lookup_bwd_*_clipped): 0 or a finite c > 0 per column,
// refused otherwise.  *any: some column is clipped.
int check_max_norms(const char* who, int32_t n_cols, const float* max_norms, bool* any) {
  *any = false;
  HBK_REQUIRE(n_cols <= 0 || max_norms != nullptr, "%s: max_norms is NULL", who);
  for (int32_t c = 0; c < n_cols; ++c) {
    const float x = max_norms[c];
    HBK_REQUIRE(x >= 0.0f && x <= 3.402823466e38f,
                "%s: column %d: max_norm must be 0 (no clip) or finite and > 0, got %g", who, c, (double)x);
    *any = *any || x > 0.0f;
  }
  return HBK_OK;
}

int adam_call(int32_t n_cols, const hbk_lookup_grad_column_t* cols, const float* clip, float* const* m,
              float* const* v, const hbk_adam_t* adam, float lr, void* workspace, size_t workspace_bytes,
              hbk_stream_t stream_) {
  static const SlotNames kNames = {"group_lookup_bwd_adam", "Adam", "m", "v"};
  const int rc = slot_apply<AdamParams>(
      kNames, [&] { return adam_check(adam, lr, kNames.who); }, adam != nullptr && adam->finish,
      n_cols, cols, m, v,
      [&](SlotArgs<AdamParams>& a, unsigned blocks, hipStream_t stream) {
        a.p = AdamParams{adam->beta_powers, lr, adam->beta1, adam->beta2, adam->epsilon};
        if (clip != nullptr) {
          hipLaunchKernelGGL(sparse_adam_clip_kernel, dim3(blocks), dim3(kSlotBlock), 0, stream, a);
        } else {
          hipLaunchKernelGGL(sparse_adam_apply_kernel, dim3(blocks), dim3(kSlotBlock), 0, stream, a);
        }
      },
      workspace, workspace_bytes, stream_, clip);
  if (rc != HBK_OK || !adam->finish) return rc;
  hipLaunchKernelGGL(adam_finish_kernel, dim3(1), dim3(kWave), 0, as_stream(stream_), adam->beta_powers,
                     adam->beta1, adam->beta2);
  HBK_HIP_OK(hipGetLastError());
  return HBK_OK;
}

int ftrl_call(int32_t n_cols, const hbk_lookup_grad_column_t* cols, const float* clip, float* const* accum,
              float* const* linear, const hbk_ftrl_t* ftrl, float lr, void* workspace,
              size_t workspace_bytes, hbk_stream_t stream_) {
  static const SlotNames kNames = {"group_lookup_bwd_ftrl", "FTRL", "accum", "linear"};
  return slot_apply<FtrlParams>(
      kNames, [&] { return ftrl_check(ftrl, lr, kNames.who); }, false, n_cols, cols, accum, linear,
      [&](SlotArgs<FtrlParams>& a, unsigned blocks, hipStream_t stream) {
        a.p = FtrlParams{lr, ftrl->l1, 2.0f * ftrl->l2, 2.0f * ftrl->l2_shrinkage, -ftrl->lr_power};
        // lr_power = -0.5 (TF's default) takes the sqrtf instantiation, any other the powf one
        if (clip != nullptr) {
          if (ftrl->lr_power != -0.5f) {
            hipLaunchKernelGGL(sparse_ftrl_clip_kernel<true>, dim3(blocks), dim3(kSlotBlock), 0, stream, a);
          } else {
            hipLaunchKernelGGL(sparse_ftrl_clip_kernel<false>, dim3(blocks), dim3(kSlotBlock), 0, stream, a);
          }
        } else if (ftrl->lr_power != -0.5f) {
          hipLaunchKernelGGL(sparse_ftrl_apply_kernel<true>, dim3(blocks), dim3(kSlotBlock), 0, stream,
                             a);
        } else {
          hipLaunchKernelGGL(sparse_ftrl_apply_kernel<false>, dim3(blocks), dim3(kSlotBlock), 0, stream,
                             a);
        }
      },
      workspace, workspace_bytes, stream_, clip);
}

int rowwise_adagrad_call(int32_t n_cols, const hbk_lookup_grad_column_t* cols, const float* clip,
                         float* const* accum, const hbk_rowwise_adagrad_t* opt, float lr, void* workspace,
                         size_t workspace_bytes, hbk_stream_t stream_) {
  static const SlotNames kNames = {"group_lookup_bwd_rowwise_adagrad", "row-wise Adagrad", "accum", nullptr};
  return slot_apply<RowwiseParams>(
      kNames, [&] { return rowwise_adagrad_check(opt, lr, kNames.who); }, false, n_cols, cols, accum,
      nullptr,
      [&](SlotArgs<RowwiseParams>& a, unsigned blocks, hipStream_t stream) {
        a.p = RowwiseParams{lr, opt->epsilon};
        if (clip != nullptr) {
          hipLaunchKernelGGL(sparse_rowwise_adagrad_clip_kernel, dim3(blocks), dim3(kSlotBlock), 0, stream,
                             a);
        } else {
          hipLaunchKernelGGL(sparse_rowwise_adagrad_apply_kernel, dim3(blocks), dim3(kSlotBlock), 0, stream,
                             a);
        }
      },
      workspace, workspace_bytes, stream_, clip);
}

// The columns of a clipped SGD / Adagrad / emit call, split: `plain` keeps the route of
// hbk_group_lookup_bwd_apply (the fused step), `clipped` runs the emit form and the clip pass.
struct ClipSplit {
  std::vector<hbk_lookup_grad_column_t> plain, clipped;
  std::vector<float> c;   // the clipped columns' max_norm
};
ClipSplit clip_split(int32_t n_cols, const hbk_lookup_grad_column_t* cols, const float* max_norms) {
  ClipSplit s;
  for (int32_t c = 0; c < n_cols; ++c) {
    if (max_norms[c] > 0.0f) {
      s.clipped.push_back(cols[c]);
      s.c.push_back(max_norms[c]);
    } else {
      s.plain.push_back(cols[c]);
    }
  }
  return s;
}

// the workspace of a split call: the plain columns' reduce, then the clipped columns' emit form and
// step-only slices
size_t clip_workspace_bytes(const ClipSplit& s) {
  const size_t plain = hbk_group_lookup_bwd_workspace_bytes((int32_t)s.plain.size(), s.plain.data());
  const size_t clipped = slot_workspace_bytes((int32_t)s.clipped.size(), s.clipped.data());
  return align256(plain) + clipped;
}
}  // namespace
}  // namespace hbk

extern "C" size_t hbk_group_lookup_bwd_apply_clipped_workspace_bytes(int32_t n_cols,
                                                                    const hbk_lookup_grad_column_t* cols,
                                                                    const float* max_norms) {
  using namespace hbk;
  bool any = false;
  if (n_cols <= 0 || cols == nullptr || check_max_norms("", n_cols, max_norms, &any) != HBK_OK || !any) {
    return hbk_group_lookup_bwd_workspace_bytes(n_cols, cols);
  }
  return clip_workspace_bytes(clip_split(n_cols, cols, max_norms));
}

extern "C" int hbk_group_lookup_bwd_apply_clipped(int32_t n_cols, const hbk_lookup_grad_column_t* cols,
                                                  const float* max_norms, int32_t apply, float apply_lr,
                                                  void* workspace, size_t workspace_bytes,
                                                  hbk_stream_t stream_) {
  using namespace hbk;
  static const char* kWho = "group_lookup_bwd_apply_clipped";
  HBK_REQUIRE(n_cols >= 0, "%s: n_cols must be >= 0, got %d", kWho, n_cols);
  HBK_REQUIRE(n_cols == 0 || cols != nullptr, "%s: cols is NULL", kWho);
  bool any = false;
  int rc = check_max_norms(kWho, n_cols, max_norms, &any);
  if (rc != HBK_OK) return rc;
  if (!any) {
    return hbk_group_lookup_bwd_apply(n_cols, cols, apply, apply_lr, workspace, workspace_bytes, stream_);
  }
  // every check of both halves before the first launch: a refused call steps and writes nothing
  if ((rc = bwd_check(n_cols, cols, apply, apply_lr)) != HBK_OK) return rc;
  const ClipSplit s = clip_split(n_cols, cols, max_norms);
  const int32_t nc = (int32_t)s.clipped.size();
  {
    const std::vector<hbk_lookup_grad_column_t> q = emit_form(nc, s.clipped.data());
    if ((rc = bwd_check(nc, q.data(), HBK_APPLY_SGD, 0.0f)) != HBK_OK) return rc;
  }
  const bool stepping = apply_lr != 0.0f;
  const bool adagrad = stepping && apply == HBK_APPLY_ADAGRAD;
  std::vector<RowShape> shapes((size_t)nc);
  std::vector<float*> s0((size_t)nc, nullptr), s1((size_t)nc, nullptr);
  for (int32_t k = 0; k < nc; ++k) {
    const hbk_lookup_grad_column_t& h = s.clipped[(size_t)k];
    if (h.n_ids <= 0) continue;
    HBK_REQUIRE(h.table != nullptr, "%s: clipped column %d: table is NULL (the clip reads the rows)", kWho,
                k);
    const int32_t pitch = h.table_pitch > 0 ? h.table_pitch : h.dim;
    if (adagrad) s0[(size_t)k] = h.accum;
    HBK_REQUIRE(make_rowshape(h.dim,
                              (uintptr_t)h.table | (uintptr_t)h.grad_rows | (adagrad ? (uintptr_t)h.accum : 0) |
                                  ((uintptr_t)(uint32_t)pitch * 4),
                              &shapes[(size_t)k]),
                "%s: clipped column %d: dim %d needs more than 64 lanes per row (at most 256 with 16-byte "
                "aligned table / accum / grad_rows / pitch, 64 otherwise)", kWho, k, h.dim);
  }
  if (stepping) {
    // the clip reads every row as it was before this call's step: a table stepped by a clipped column
    // may not be named by any other column of the call
    for (int32_t a = 0; a < n_cols; ++a) {
      if (max_norms[a] <= 0.0f || cols[a].n_ids <= 0) continue;
      for (int32_t b = 0; b < n_cols; ++b) {
        if (b == a || cols[b].n_ids <= 0) continue;
        HBK_REQUIRE(cols[b].table != cols[a].table && cols[b].accum != cols[a].table &&
                        (cols[a].accum == nullptr ||
                         (cols[b].table != cols[a].accum && cols[b].accum != cols[a].accum)),
                    "%s: columns %d and %d share a table or accumulator; a clipped column's table may "
                    "not be named twice in a stepping call", kWho, a, b);
      }
    }
  }
  const size_t plain_ws = hbk_group_lookup_bwd_workspace_bytes((int32_t)s.plain.size(), s.plain.data());
  const size_t need = clip_workspace_bytes(s);
  HBK_REQUIRE(need == 0 || (workspace != nullptr && workspace_bytes >= need),
              "%s: workspace too small: need %zu bytes, got %zu", kWho, need, workspace_bytes);
  HBK_REQUIRE(((uintptr_t)workspace & 7) == 0, "%s: workspace must be 8-byte aligned", kWho);
  // (1) the plain columns on their own route
  if (!s.plain.empty()) {
    rc = hbk_group_lookup_bwd_apply((int32_t)s.plain.size(), s.plain.data(), apply, apply_lr, workspace,
                                    workspace_bytes, stream_);
    if (rc != HBK_OK) return rc;
  }
  // (2) the clipped columns' emit form behind them in the workspace, (3) the clip pass
  char* const ws = reinterpret_cast<char*>(workspace) + align256(plain_ws);
  std::vector<hbk_lookup_grad_column_t> e;
  rc = run_emit_form(kWho, nc, s.clipped.data(), ws, workspace_bytes - align256(plain_ws), stream_, &e);
  if (rc != HBK_OK) return rc;
  hipStream_t stream = as_stream(stream_);
  for (int32_t c0 = 0; c0 < nc; c0 += kSlotMaxCols) {
    SlotArgs<LrParams> a;
    memset(&a, 0, sizeof(a));
    unsigned blocks = 0;
    a.n_cols = fill_slot_cols(e.data(), shapes, s0.data(), s1.data(), c0, std::min(nc, c0 + kSlotMaxCols), a.c,
                              &blocks, s.c.data());
    if (a.n_cols == 0) continue;
    a.p = LrParams{apply_lr};
    if (!stepping) {
      hipLaunchKernelGGL(sparse_emit_clip_kernel, dim3(blocks), dim3(kSlotBlock), 0, stream, a);
    } else if (adagrad) {
      hipLaunchKernelGGL(sparse_adagrad_clip_kernel, dim3(blocks), dim3(kSlotBlock), 0, stream, a);
    } else {
      hipLaunchKernelGGL(sparse_sgd_clip_kernel, dim3(blocks), dim3(kSlotBlock), 0, stream, a);
    }
    HBK_HIP_OK(hipGetLastError());
  }
  return HBK_OK;
}

extern "C" size_t hbk_group_lookup_bwd_adam_clipped_workspace_bytes(int32_t n_cols,
                                                                   const hbk_lookup_grad_column_t* cols,
                                                                   const float* max_norms) {
  (void)max_norms;
  return hbk::slot_workspace_bytes(n_cols, cols);
}

extern "C" int hbk_group_lookup_bwd_adam_clipped(int32_t n_cols, const hbk_lookup_grad_column_t* cols,
                                                 const float* max_norms, float* const* m, float* const* v,
                                                 const hbk_adam_t* adam, float lr, void* workspace,
                                                 size_t workspace_bytes, hbk_stream_t stream_) {
  using namespace hbk;
  bool any = false;
  const int rc = check_max_norms("group_lookup_bwd_adam_clipped", n_cols, max_norms, &any);
  if (rc != HBK_OK) return rc;
  return adam_call(n_cols, cols, any ? max_norms : nullptr, m, v, adam, lr, workspace, workspace_bytes,
                   stream_);
}

extern "C" size_t hbk_group_lookup_bwd_ftrl_clipped_workspace_bytes(int32_t n_cols,
                                                                   const hbk_lookup_grad_column_t* cols,
                                                                   const float* max_norms) {
  (void)max_norms;
  return hbk::slot_workspace_bytes(n_cols, cols);
}

extern "C" int hbk_group_lookup_bwd_ftrl_clipped(int32_t n_cols, const hbk_lookup_grad_column_t* cols,
                                                 const float* max_norms, float* const* accum,
                                                 float* const* linear, const hbk_ftrl_t* ftrl, float lr,
                                                 void* workspace, size_t workspace_bytes,
                                                 hbk_stream_t stream_) {
  using namespace hbk;
  bool any = false;
  const int rc = check_max_norms("group_lookup_bwd_ftrl_clipped", n_cols, max_norms, &any);
  if (rc != HBK_OK) return rc;
  return ftrl_call(n_cols, cols, any ? max_norms : nullptr, accum, linear, ftrl, lr, workspace,
                   workspace_bytes, stream_);
}

extern "C" size_t hbk_group_lookup_bwd_adam_workspace_bytes(int32_t n_cols,
                                                            const hbk_lookup_grad_column_t* cols) {
  return hbk::slot_workspace_bytes(n_cols, cols);
}

extern "C" int hbk_group_lookup_bwd_adam(int32_t n_cols, const hbk_lookup_grad_column_t* cols,
                                         float* const* m, float* const* v, const hbk_adam_t* adam,
                                         float lr, void* workspace, size_t workspace_bytes,
                                         hbk_stream_t stream_) {
  return hbk::adam_call(n_cols, cols, nullptr, m, v, adam, lr, workspace, workspace_bytes, stream_);
}

extern "C" size_t hbk_group_lookup_bwd_ftrl_workspace_bytes(int32_t n_cols,
                                                            const hbk_lookup_grad_column_t* cols) {
  return hbk::slot_workspace_bytes(n_cols, cols);
}

extern "C" int hbk_group_lookup_bwd_ftrl(int32_t n_cols, const hbk_lookup_grad_column_t* cols,
                                         float* const* accum, float* const* linear,
                                         const hbk_ftrl_t* ftrl, float lr, void* workspace,
                                         size_t workspace_bytes, hbk_stream_t stream_) {
  return hbk::ftrl_call(n_cols, cols, nullptr, accum, linear, ftrl, lr, workspace, workspace_bytes,
                        stream_);
}

extern "C" size_t hbk_group_lookup_bwd_rowwise_adagrad_workspace_bytes(int32_t n_cols,
                                                                       const hbk_lookup_grad_column_t* cols) {
  return hbk::slot_workspace_bytes(n_cols, cols);
}

extern "C" int hbk_group_lookup_bwd_rowwise_adagrad(int32_t n_cols, const hbk_lookup_grad_column_t* cols,
                                                    float* const* accum, const hbk_rowwise_adagrad_t* opt,
                                                    float lr, void* workspace, size_t workspace_bytes,
                                                    hbk_stream_t stream_) {
  return hbk::rowwise_adagrad_call(n_cols, cols, nullptr, accum, opt, lr, workspace, workspace_bytes,
                                   stream_);
}

extern "C" size_t hbk_group_lookup_bwd_rowwise_adagrad_clipped_workspace_bytes(
    int32_t n_cols, const hbk_lookup_grad_column_t* cols, const float* max_norms) {
  (void)max_norms;
  return hbk::slot_workspace_bytes(n_cols, cols);
}

extern "C" int hbk_group_lookup_bwd_rowwise_adagrad_clipped(int32_t n_cols,
                                                            const hbk_lookup_grad_column_t* cols,
                                                            const float* max_norms, float* const* accum,
                                                            const hbk_rowwise_adagrad_t* opt, float lr,
                                                            void* workspace, size_t workspace_bytes,
                                                            hbk_stream_t stream_) {
  using namespace hbk;
  bool any = false;
  const int rc = check_max_norms("group_lookup_bwd_rowwise_adagrad_clipped", n_cols, max_norms, &any);
  if (rc != HBK_OK) return rc;
  return rowwise_adagrad_call(n_cols, cols, any ? max_norms : nullptr, accum, opt, lr, workspace,
                              workspace_bytes, stream_);
}

// ------------------------------------------------------------------------------------------------------------
// hbk_sparse_apply_slices_n (include/hbk.h): the apply launches above on IndexedSlices the caller holds.  Host
// code only: the slices become the descriptors phase 2 reads (n_ids = the capacity), the column checks of the
// slot entries run on them, and the rule's kernel is launched once per kSlotMaxCols columns.  SGD and Adagrad
// take the clip pass's kernels with every max_norm 0, which makes them plain slice applies with the fused
// step's arithmetic.
namespace hbk {
namespace {

// every host check of an SGD / Adagrad slice call's columns (accum == NULL: SGD); the apply's row shapes
int check_lr_slices(const char* who, int32_t n_cols, const hbk_lookup_grad_column_t* e, float* const* accum,
                    std::vector<RowShape>* shapes) {
  std::vector<uintptr_t> seen;
  seen.reserve((size_t)n_cols * 2);
  shapes->assign((size_t)n_cols, RowShape{});
  for (int32_t c = 0; c < n_cols; ++c) {
    const hbk_lookup_grad_column_t& h = e[c];
    float* const a = accum != nullptr ? accum[c] : nullptr;
    HBK_REQUIRE(accum == nullptr || a != nullptr, "%s: column %d: the accumulator is NULL", who, c);
    HBK_REQUIRE(a == nullptr || a != h.table, "%s: column %d: the accumulator is the table", who, c);
    const int32_t pitch = h.table_pitch > 0 ? h.table_pitch : h.dim;
    HBK_REQUIRE(h.n_ids <= 0 ||
                    make_rowshape(h.dim,
                                  (uintptr_t)h.table | (uintptr_t)a | (uintptr_t)h.grad_rows |
                                      ((uintptr_t)(uint32_t)pitch * 4),
                                  &(*shapes)[(size_t)c]),
                "%s: column %d: dim %d needs more than 64 lanes per row (at most 256 with 16-byte "
                "aligned table / accum / grad_rows / pitch, 64 otherwise)", who, c, h.dim);
    if (h.table != nullptr) seen.push_back((uintptr_t)h.table);
    if (a != nullptr) seen.push_back((uintptr_t)a);
  }
  std::sort(seen.begin(), seen.end());
  HBK_REQUIRE(std::adjacent_find(seen.begin(), seen.end()) == seen.end(),
              "%s: two columns name the same table or accumulator (a row stepped twice in one call would "
              "race)", who);
  return HBK_OK;
}

// what both slice entries refuse first, in the same words
int check_slices_call(const char* who, int32_t n_cols, const void* cols, int32_t apply) {
  HBK_REQUIRE(n_cols >= 0, "%s: n_cols must be >= 0, got %d", who, n_cols);
  HBK_REQUIRE(n_cols == 0 || cols != nullptr, "%s: cols is NULL", who);
  HBK_REQUIRE(apply == HBK_APPLY_SGD || apply == HBK_APPLY_ADAGRAD || apply == HBK_APPLY_LAZY_ADAM ||
                  apply == HBK_APPLY_FTRL || apply == HBK_APPLY_ROWWISE_ADAGRAD,
              "%s: apply must be HBK_APPLY_SGD, _ADAGRAD, _LAZY_ADAM, _FTRL or _ROWWISE_ADAGRAD, got %d", who,
              apply);
  return HBK_OK;
}

// the sizes of slice column c, and its slices when it has any (S: hbk_slices_column_t or hbk_lowp_slices_column_t)
template <typename S>
int check_slice_sizes(const char* who, int32_t c, const S& s) {
  HBK_REQUIRE(s.capacity >= 0 && s.capacity < (1ll << 30), "%s: column %d: capacity %lld must be in [0, 2^30)",
              who, c, (long long)s.capacity);
  HBK_REQUIRE(s.rows >= 0, "%s: column %d: rows must be >= 0, got %lld", who, c, (long long)s.rows);
  HBK_REQUIRE(s.dim >= 1, "%s: column %d: dim must be >= 1", who, c);
  return HBK_OK;
}
template <typename S>
int check_slice_buffers(const char* who, int32_t c, const S& s) {
  HBK_REQUIRE(s.unique_rows != nullptr && ((uintptr_t)s.unique_rows & 7) == 0,
              "%s: column %d: unique_rows must be a device int64 [capacity]", who, c);
  HBK_REQUIRE(s.grad_rows != nullptr && ((uintptr_t)s.grad_rows & 3) == 0,
              "%s: column %d: grad_rows must be a device fp32 [capacity, dim]", who, c);
  HBK_REQUIRE(s.n_unique != nullptr && ((uintptr_t)s.n_unique & 3) == 0,
              "%s: column %d: n_unique must be a device int32 [1]", who, c);
  return HBK_OK;
}

// a rule as the argument of dispatch_rule's callback
template <typename R>
struct RuleOf {
  using Rule = R;
};

// The one rule dispatch of the slice entries: the apply code's hyperparameter check (the lr's own for SGD and
// Adagrad), then run(RuleOf<Rule>(), the names the rule's refusals use, the rule's Params) -- where the caller
// checks its columns and launches the kernel of its table policy -- and Adam's finish launch behind it.
template <typename Run>
int dispatch_rule(const char* who, int32_t apply, const void* params, float lr, hipStream_t stream, Run run) {
  int rc = HBK_OK;
  if (apply == HBK_APPLY_LAZY_ADAM) {
    const hbk_adam_t* adam = static_cast<const hbk_adam_t*>(params);
    if ((rc = adam_check(adam, lr, who)) != HBK_OK) return rc;
    rc = run(RuleOf<AdamRule>(), SlotNames{who, "Adam", "m", "v"},
             AdamParams{adam->beta_powers, lr, adam->beta1, adam->beta2, adam->epsilon});
    if (rc != HBK_OK || !adam->finish) return rc;
    hipLaunchKernelGGL(adam_finish_kernel, dim3(1), dim3(kWave), 0, stream, adam->beta_powers, adam->beta1,
                       adam->beta2);
    HBK_HIP_OK(hipGetLastError());
    return HBK_OK;
  }
  if (apply == HBK_APPLY_FTRL) {
    const hbk_ftrl_t* ftrl = static_cast<const hbk_ftrl_t*>(params);
    if ((rc = ftrl_check(ftrl, lr, who)) != HBK_OK) return rc;
    const SlotNames nm = {who, "FTRL", "accum", "linear"};
    const FtrlParams p = {lr, ftrl->l1, 2.0f * ftrl->l2, 2.0f * ftrl->l2_shrinkage, -ftrl->lr_power};
    // lr_power = -0.5 (TF's default) takes the sqrtf instantiation, any other the powf one
    return ftrl->lr_power != -0.5f ? run(RuleOf<FtrlRule<true>>(), nm, p) : run(RuleOf<FtrlRule<false>>(), nm, p);
  }
  if (apply == HBK_APPLY_ROWWISE_ADAGRAD) {
    const hbk_rowwise_adagrad_t* opt = static_cast<const hbk_rowwise_adagrad_t*>(params);
    if ((rc = rowwise_adagrad_check(opt, lr, who)) != HBK_OK) return rc;
    return run(RuleOf<RowwiseAdagradRule>(), SlotNames{who, "row-wise Adagrad", "accum", nullptr},
               RowwiseParams{lr, opt->epsilon});
  }
  HBK_REQUIRE(lr != 0.0f && lr >= -3.402823466e38f && lr <= 3.402823466e38f,
              "%s: lr must be finite and != 0, got %g", who, (double)lr);
  const SlotNames nm = {who, apply == HBK_APPLY_ADAGRAD ? "Adagrad" : "SGD", "the accumulator", nullptr};
  return apply == HBK_APPLY_ADAGRAD ? run(RuleOf<AdagradRule>(), nm, LrParams{lr})
                                    : run(RuleOf<SgdRule>(), nm, LrParams{lr});
}

// the launches of one slice call over either kind of table: launch(args, blocks) sets what args holds besides
// the columns and launches the rule's kernel
template <typename Table, typename P, typename HostCol, typename Launch>
int launch_slices(int32_t n_cols, const HostCol* cols, const std::vector<RowShape>& shapes, float* const* s0,
                  float* const* s1, Launch launch) {
  for (int32_t c0 = 0; c0 < n_cols; c0 += kSlotMaxCols) {
    typename Table::template Args<P> a;
    memset(&a, 0, sizeof(a));
    unsigned blocks = 0;
    a.n_cols = fill_slot_cols(cols, shapes, s0, s1, c0, std::min(n_cols, c0 + kSlotMaxCols), a.c, &blocks);
    if (a.n_cols == 0) continue;
    launch(a, blocks);
    HBK_HIP_OK(hipGetLastError());
  }
  return HBK_OK;
}

// the fp32 slice kernel of a rule: SGD and Adagrad take the clip pass's kernels (every max_norm is 0)
inline auto fp32_slices_kernel(RuleOf<SgdRule>) { return sparse_sgd_clip_kernel; }
inline auto fp32_slices_kernel(RuleOf<AdagradRule>) { return sparse_adagrad_clip_kernel; }
inline auto fp32_slices_kernel(RuleOf<AdamRule>) { return sparse_adam_apply_kernel; }
template <bool kPow>
inline auto fp32_slices_kernel(RuleOf<FtrlRule<kPow>>) { return sparse_ftrl_apply_kernel<kPow>; }
inline auto fp32_slices_kernel(RuleOf<RowwiseAdagradRule>) { return sparse_rowwise_adagrad_apply_kernel; }

int sparse_apply_slices(int32_t n_cols, const hbk_slices_column_t* cols, int32_t apply, float* const* slot0,
                        float* const* slot1, const void* params, float lr, hbk_stream_t stream_) {
  static const char* kWho = "sparse_apply_slices_n";
  int rc = check_slices_call(kWho, n_cols, cols, apply);
  if (rc != HBK_OK) return rc;
  // the slices as the descriptors the apply reads
  std::vector<hbk_lookup_grad_column_t> e((size_t)n_cols);
  for (int32_t c = 0; c < n_cols; ++c) {
    const hbk_slices_column_t& s = cols[c];
    if ((rc = check_slice_sizes(kWho, c, s)) != HBK_OK) return rc;
    HBK_REQUIRE(s.table_pitch == 0 || s.table_pitch >= s.dim,
                "%s: column %d: table_pitch %d is smaller than dim %d", kWho, c, s.table_pitch, s.dim);
    if (s.capacity > 0) {
      HBK_REQUIRE(s.table != nullptr && ((uintptr_t)s.table & 3) == 0,
                  "%s: column %d: table must be a device fp32 buffer", kWho, c);
      if ((rc = check_slice_buffers(kWho, c, s)) != HBK_OK) return rc;
    }
    hbk_lookup_grad_column_t& h = e[(size_t)c];
    memset(&h, 0, sizeof(h));
    h.table = s.table;
    h.rows = s.rows;
    h.dim = s.dim;
    h.table_pitch = s.table_pitch;
    h.n_ids = s.capacity;
    h.unique_rows = const_cast<int64_t*>(s.unique_rows);
    h.grad_rows = const_cast<float*>(s.grad_rows);
    h.n_unique = const_cast<int32_t*>(s.n_unique);
  }
  hipStream_t stream = as_stream(stream_);
  return dispatch_rule(kWho, apply, params, lr, stream, [&](auto rule, const SlotNames& nm, const auto& p) {
    using Rule = typename decltype(rule)::Rule;
    using P = typename Rule::Params;
    // the column checks of the rule's slot entry (SGD and Adagrad: their own)
    float* const* const s0 = Rule::kSlots >= 1 || Rule::kRowwise ? slot0 : nullptr;
    float* const* const s1 = Rule::kSlots >= 2 ? slot1 : nullptr;
    std::vector<RowShape> shapes;
    int rc = HBK_OK;
    if constexpr (Rule::kRowwise) {
      rc = check_row_slot_columns(nm, n_cols, e.data(), s0, &shapes);
    } else if constexpr (Rule::kSlots == 2) {
      rc = check_slot_columns(nm, n_cols, e.data(), s0, s1, &shapes);
    } else {
      HBK_REQUIRE(Rule::kSlots == 0 || n_cols == 0 || s0 != nullptr, "%s: the accumulator array (slot0) is NULL",
                  kWho);
      rc = check_lr_slices(kWho, n_cols, e.data(), s0, &shapes);
    }
    if (rc != HBK_OK) return rc;
    return launch_slices<Fp32Rows, P>(n_cols, e.data(), shapes, s0, s1, [&](SlotArgs<P>& a, unsigned blocks) {
      a.p = p;
      hipLaunchKernelGGL(fp32_slices_kernel(rule), dim3(blocks), dim3(kSlotBlock), 0, stream, a);
    });
  });
}

// ------------------------------------------------------------------------------------------------------------
// hbk_lowp_apply_slices_n (include/hbk.h): the same step on tables of bf16 / fp16 rows -- the same dispatch, the
// same launches, lowp_apply_kernel<Rule> in the place of the fp32 kernels.

// every host check of a 16-bit slice call's slots and columns (n_slots table-shaped slots, or the row-wise
// accumulator in slot0; n0 / n1: their names); the apply's row shapes
int check_lowp_columns(const char* who, int32_t n_cols, const hbk_lowp_slices_column_t* cols, int n_slots,
                       bool rowwise, const char* n0, const char* n1, float* const* slot0, float* const* slot1,
                       bool stochastic, std::vector<RowShape>* shapes) {
  HBK_REQUIRE(n_cols == 0 || (n_slots < 1 && !rowwise) || slot0 != nullptr, "%s: the %s array (slot0) is NULL", who,
              n0);
  HBK_REQUIRE(n_cols == 0 || n_slots < 2 || slot1 != nullptr, "%s: the %s array (slot1) is NULL", who, n1);
  shapes->assign((size_t)n_cols, RowShape{});
  std::vector<uintptr_t> seen;
  seen.reserve((size_t)n_cols * 3);
  int rc = HBK_OK;
  for (int32_t c = 0; c < n_cols; ++c) {
    const hbk_lowp_slices_column_t& s = cols[c];
    HBK_REQUIRE(s.table_dtype == HBK_LOWP_BF16 || s.table_dtype == HBK_LOWP_FP16,
                "%s: column %d: table_dtype must be HBK_LOWP_BF16 or HBK_LOWP_FP16, got %d", who, c, s.table_dtype);
    HBK_REQUIRE(!stochastic || s.table_dtype == HBK_LOWP_BF16,
                "%s: column %d: stochastic rounding is defined for bf16 tables only", who, c);
    if ((rc = check_slice_sizes(who, c, s)) != HBK_OK) return rc;
    HBK_REQUIRE(((uintptr_t)s.table & 1) == 0, "%s: column %d: table must be 2-byte aligned", who, c);
    float* const a0 = (n_slots >= 1 || rowwise) ? slot0[c] : nullptr;
    float* const a1 = n_slots >= 2 ? slot1[c] : nullptr;
    HBK_REQUIRE(!(n_slots >= 1 || rowwise) || (a0 != nullptr && ((uintptr_t)a0 & 3) == 0),
                "%s: column %d: %s must be a device fp32 buffer", who, c, n0);
    HBK_REQUIRE(n_slots < 2 || (a1 != nullptr && ((uintptr_t)a1 & 3) == 0),
                "%s: column %d: %s must be a device fp32 buffer", who, c, n1);
    if (s.capacity > 0) {
      HBK_REQUIRE(s.table != nullptr, "%s: column %d: table is NULL", who, c);
      if ((rc = check_slice_buffers(who, c, s)) != HBK_OK) return rc;
      // the row shape of the fp32 entry: the table's bytes count twice (an 8-byte chunk where fp32 has 16), the
      // row-wise word does not enter
      const uintptr_t bits = ((uintptr_t)s.table * 2) | (uintptr_t)s.grad_rows |
                             (n_slots >= 1 ? (uintptr_t)a0 : 0) | (uintptr_t)a1;
      HBK_REQUIRE(make_rowshape(s.dim, bits, &(*shapes)[(size_t)c]),
                  "%s: column %d: dim %d: at most 256 when dim %% 4 == 0, the table is 8-byte and the slots and "
                  "grad_rows are 16-byte aligned, 64 otherwise", who, c, s.dim);
    }
    if (s.table != nullptr) seen.push_back((uintptr_t)s.table);
    if (a0 != nullptr) seen.push_back((uintptr_t)a0);
    if (a1 != nullptr) seen.push_back((uintptr_t)a1);
  }
  std::sort(seen.begin(), seen.end());
  HBK_REQUIRE(std::adjacent_find(seen.begin(), seen.end()) == seen.end(),
              "%s: two columns name the same table or slot (a row stepped twice in one call would race)", who);
  return HBK_OK;
}

int lowp_apply_slices(int32_t n_cols, const hbk_lowp_slices_column_t* cols, int32_t apply, float* const* slot0,
                      float* const* slot1, const void* params, float lr, const hbk_lowp_rounding_t* rounding,
                      hbk_stream_t stream_) {
  static const char* kWho = "lowp_apply_slices_n";
  int rc = check_slices_call(kWho, n_cols, cols, apply);
  if (rc != HBK_OK) return rc;
  const int32_t mode = rounding != nullptr ? rounding->mode : HBK_LOWP_ROUND_NEAREST;
  HBK_REQUIRE(mode == HBK_LOWP_ROUND_NEAREST || mode == HBK_LOWP_ROUND_STOCHASTIC,
              "%s: rounding mode must be HBK_LOWP_ROUND_NEAREST or HBK_LOWP_ROUND_STOCHASTIC, got %d", kWho, mode);
  const bool stochastic = mode == HBK_LOWP_ROUND_STOCHASTIC;
  HBK_REQUIRE(!stochastic || (rounding->step != nullptr && ((uintptr_t)rounding->step & 3) == 0),
              "%s: stochastic rounding needs a device uint32 [1] step counter", kWho);
  const LowpRound round = {stochastic ? rounding->step : nullptr, stochastic ? rounding->seed : 0u};
  hipStream_t stream = as_stream(stream_);
  rc = dispatch_rule(kWho, apply, params, lr, stream, [&](auto rule, const SlotNames& nm, const auto& p) {
    using Rule = typename decltype(rule)::Rule;
    using P = typename Rule::Params;
    float* const* const s0 = Rule::kSlots >= 1 || Rule::kRowwise ? slot0 : nullptr;
    float* const* const s1 = Rule::kSlots >= 2 ? slot1 : nullptr;
    std::vector<RowShape> shapes;
    const int rc = check_lowp_columns(kWho, n_cols, cols, Rule::kSlots, Rule::kRowwise,
                                      Rule::kSlots == 2 ? nm.s0 : "the accumulator", nm.s1, s0, s1, stochastic,
                                      &shapes);
    if (rc != HBK_OK) return rc;
    return launch_slices<LowpRows, P>(n_cols, cols, shapes, s0, s1, [&](LowpArgs<P>& a, unsigned blocks) {
      a.p = p;
      a.round = round;
      hipLaunchKernelGGL(lowp_apply_kernel<Rule>, dim3(blocks), dim3(kSlotBlock), 0, stream, a);
    });
  });
  if (rc != HBK_OK) return rc;
  if (stochastic && rounding->advance != 0) {
    hipLaunchKernelGGL(lowp_advance_kernel, dim3(1), dim3(kWave), 0, stream, rounding->step);
    HBK_HIP_OK(hipGetLastError());
  }
  return HBK_OK;
}

}  // namespace
}  // namespace hbk

extern "C" int hbk_sparse_apply_slices_n(int32_t n_cols, const hbk_slices_column_t* cols, int32_t apply,
                                         float* const* slot0, float* const* slot1, const void* params,
                                         float lr, hbk_stream_t stream) {
  return hbk::sparse_apply_slices(n_cols, cols, apply, slot0, slot1, params, lr, stream);
}

extern "C" int hbk_lowp_apply_slices_n(int32_t n_cols, const hbk_lowp_slices_column_t* cols, int32_t apply,
                                       float* const* slot0, float* const* slot1, const void* params, float lr,
                                       const hbk_lowp_rounding_t* rounding, hbk_stream_t stream) {
  return hbk::lowp_apply_slices(n_cols, cols, apply, slot0, slot1, params, lr, rounding, stream);
}
