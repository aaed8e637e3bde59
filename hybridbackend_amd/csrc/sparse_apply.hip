// Sparse optimizer steps with two slots per row after the grouped backward: Lazy Adam
// (tf.contrib.opt.LazyAdamOptimizer's sparse apply, TF 1.15; hbk_group_lookup_bwd_adam) and FTRL-Proximal
// (SparseApplyFtrl[V2], TF 1.15; hbk_group_lookup_bwd_ftrl).
//
// Two phases.  (1) The backward in its emit form (hbk_group_lookup_bwd_apply, apply_lr = 0) writes every
// column's distinct rows, their summed gradient rows and n_unique -- into the caller's buffers or, step
// only, into buffers carved from this call's workspace.  Every reduce plan, the deterministic modes,
// weighted columns and segmented inputs come from there unchanged, and so does the guarantee that each
// distinct row appears exactly once (Adam is not additive: a row stepped twice would decay its moments
// twice; FTRL would add g^2 to its accumulator twice).  (2) ONE apply launch for up to kAdamMaxCols
// columns: sparse_adam_apply_kernel or sparse_ftrl_apply_kernel.
//
// The apply kernels share their scheduling (scan_tasks, walk_tasks).  Work is counted in wave tasks:
// a task is kAdamItems rows per lane group of one column, a lane group holds one row (f32x4 chunks
// when dim % 4 == 0 and every address is 16-byte aligned, scalar chunks otherwise -- the reduce's
// rule, make_rowshape).  Wave 0 of every workgroup
// reads the columns' n_unique from the device and scans their task counts into LDS; the grid is sized
// from the host-known capacities only and walks the tasks grid-stride, so the call needs no host sync
// and can be captured in a graph.  A lane issues the w / slot / slot / g loads of all its kAdamItems rows
// before any arithmetic: random rows are bound by the request rate (~49 G requests/s), so
// what matters is how many are in flight.  grad_rows and unique_rows are read once (non-temporal).
// The bias-corrected rate lr_t is computed once per workgroup from the device beta powers; the
// powers advance after the apply, in stream order (adam_finish_kernel), when the call asks for it.
// FTRL has no device state besides its slots; its lr_power != -0.5 form (powf) is a separate
// instantiation, so the default form carries no powf code.
#include <string.h>

#include <algorithm>
#include <mutex>
#include <vector>

#include "common.h"
#include "lookup_common.h"

namespace hbk {
namespace {

constexpr int kAdamMaxCols = 64;    // columns per apply launch (kernarg: 64 descriptors)
constexpr int kAdamBlock = 256;
constexpr int kAdamWaves = kAdamBlock / kWave;
constexpr int kAdamItems = 4;       // rows per lane group in flight
constexpr int kAdamBlocksPerCU = 8;
static_assert(kAdamMaxCols <= kWave, "one lane per column in the task scan");

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
  int32_t pad;
};

struct AdamArgs {
  SlotCol c[kAdamMaxCols];
  const float* powers;
  float lr, beta1, beta2, eps;
  int32_t n_cols;
};
static_assert(sizeof(AdamArgs) <= 8192, "kernarg budget");

__device__ inline float sqrt_v(float a) { return sqrtf(a); }
__device__ inline f32x4 sqrt_v(f32x4 a) { return f32x4{sqrtf(a.x), sqrtf(a.y), sqrtf(a.z), sqrtf(a.w)}; }

// one task: rows base + k * groups + grp (k < kAdamItems) of column c; W floats per lane chunk
template <typename V, int W>
__device__ inline void adam_task(const SlotCol& c, int64_t base, int64_t n, float lr_t, float beta1,
                                 float beta2, float eps) {
  const int lane = lane_id();
  const int lpr = c.lpr_log2;
  const int grp = lane >> lpr;
  const int sub = lane & ((1 << lpr) - 1);
  const int groups = kWave >> lpr;
  const bool lane_on = sub * W < c.dim;
  int64_t r[kAdamItems];
  bool on[kAdamItems];
#pragma unroll
  for (int k = 0; k < kAdamItems; ++k) {
    const int64_t u = base + (int64_t)k * groups + grp;
    on[k] = lane_on && u < n;
    r[k] = on[k] ? __builtin_nontemporal_load(c.urows + u) : 0;
    on[k] = on[k] && (uint64_t)r[k] < (uint64_t)c.rows;   // (the reduce only emits rows of the table)
  }
  V w[kAdamItems], m[kAdamItems], v[kAdamItems], g[kAdamItems];
#pragma unroll
  for (int k = 0; k < kAdamItems; ++k) {
    if (!on[k]) continue;
    const int64_t u = base + (int64_t)k * groups + grp;
    const int64_t off = r[k] * c.pitch + sub * W;
    w[k] = *reinterpret_cast<const V*>(c.w + off);
    m[k] = *reinterpret_cast<const V*>(c.s0 + off);
    v[k] = *reinterpret_cast<const V*>(c.s1 + off);
    g[k] = __builtin_nontemporal_load(reinterpret_cast<const V*>(c.grows + u * c.dim + sub * W));
  }
  const float one_m_b1 = 1.0f - beta1, one_m_b2 = 1.0f - beta2;
#pragma unroll
  for (int k = 0; k < kAdamItems; ++k) {
    if (!on[k]) continue;
    const int64_t off = r[k] * c.pitch + sub * W;
    const V mk = beta1 * m[k] + one_m_b1 * g[k];
    const V vk = beta2 * v[k] + one_m_b2 * (g[k] * g[k]);
    const V wk = w[k] - (lr_t * mk) / (sqrt_v(vk) + eps);
    *reinterpret_cast<V*>(c.s0 + off) = mk;
    *reinterpret_cast<V*>(c.s1 + off) = vk;
    *reinterpret_cast<V*>(c.w + off) = wk;
  }
}

// wave 0 of a workgroup: the columns' n_unique (clamped to the capacity) into s_n and the inclusive
// prefix of their task counts into s_end
__device__ inline void scan_tasks(const SlotCol* cols, int n_cols, int lane, int64_t* s_end,
                                  int64_t* s_n) {
  int64_t tasks = 0;
  if (lane < n_cols) {
    const SlotCol& c = cols[lane];
    const int64_t n = min(max(__builtin_nontemporal_load(c.nu), 0), c.cap);
    const int64_t rpt = (int64_t)(kWave >> c.lpr_log2) * kAdamItems;
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
template <typename Task>
__device__ inline void walk_tasks(const SlotCol* cols, int n_cols, const int64_t* s_end,
                                  const int64_t* s_n, Task task) {
  const int64_t total = s_end[n_cols - 1];
  int c = 0;
  for (int64_t t = (int64_t)blockIdx.x * kAdamWaves + threadIdx.x / kWave; t < total;
       t += (int64_t)gridDim.x * kAdamWaves) {
    while (s_end[c] <= t) ++c;   // (t only grows: the column only moves forward)
    const SlotCol& col = cols[c];
    const int64_t t0 = c == 0 ? 0 : s_end[c - 1];
    const int64_t base = (t - t0) * ((int64_t)(kWave >> col.lpr_log2) * kAdamItems);
    task(col, base, s_n[c]);
  }
}

__global__ __launch_bounds__(kAdamBlock) void sparse_adam_apply_kernel(AdamArgs a) {
  __shared__ int64_t s_end[kAdamMaxCols];   // inclusive prefix of the columns' task counts
  __shared__ int64_t s_n[kAdamMaxCols];     // their n_unique (clamped to the capacity)
  __shared__ float s_lr_t;
  if (threadIdx.x < kWave) {
    const int lane = (int)threadIdx.x;
    scan_tasks(a.c, a.n_cols, lane, s_end, s_n);
    if (lane == 0) {
      const float b1p = a.powers[0], b2p = a.powers[1];
      s_lr_t = (a.lr * sqrtf(1.0f - b2p)) / (1.0f - b1p);
    }
  }
  __syncthreads();
  const float lr_t = s_lr_t;
  walk_tasks(a.c, a.n_cols, s_end, s_n, [&](const SlotCol& col, int64_t base, int64_t n) {
    if (col.vec4) {
      adam_task<f32x4, 4>(col, base, n, lr_t, a.beta1, a.beta2, a.eps);
    } else {
      adam_task<float, 1>(col, base, n, lr_t, a.beta1, a.beta2, a.eps);
    }
  });
}

// TF's _finish: beta1^t, beta2^t -> beta1^(t+1), beta2^(t+1), one fp32 product each
__global__ void adam_finish_kernel(float* powers, float beta1, float beta2) {
  if (threadIdx.x == 0) {
    powers[0] = powers[0] * beta1;
    powers[1] = powers[1] * beta2;
  }
}

struct FtrlArgs {
  SlotCol c[kAdamMaxCols];   // s0 = accum, s1 = linear
  float lr, l1, two_l2, two_shrinkage, neg_lr_power;   // (2 * l2, 2 * l2_shrinkage, -lr_power: exact)
  int32_t n_cols;
};
static_assert(sizeof(FtrlArgs) <= 8192, "kernarg budget");

struct FtrlOut {
  float w, acc, z;
};

// TF 1.15 SparseApplyFtrl[V2] on one element, every op a separately rounded fp32 op in TF's order;
// kPow: lr_power != -0.5 (powf), else sqrtf
template <bool kPow>
__device__ inline FtrlOut ftrl_elem(float w, float acc, float z, float g, const FtrlArgs& a) {
  const float gs = a.two_shrinkage == 0.0f ? g : g + a.two_shrinkage * w;
  const float na = acc + g * g;
  const float pn = kPow ? powf(na, a.neg_lr_power) : sqrtf(na);
  const float po = kPow ? powf(acc, a.neg_lr_power) : sqrtf(acc);
  const float zn = z + (gs - ((pn - po) / a.lr) * w);
  const float y = pn / a.lr + a.two_l2;
  return FtrlOut{(fmaxf(fminf(zn, a.l1), -a.l1) - zn) / y, na, zn};
}

template <bool kPow>
__device__ inline void ftrl_v(float& w, float& acc, float& z, float g, const FtrlArgs& a) {
  const FtrlOut o = ftrl_elem<kPow>(w, acc, z, g, a);
  w = o.w;
  acc = o.acc;
  z = o.z;
}
template <bool kPow>
__device__ inline void ftrl_v(f32x4& w, f32x4& acc, f32x4& z, f32x4 g, const FtrlArgs& a) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const FtrlOut o = ftrl_elem<kPow>(w[i], acc[i], z[i], g[i], a);
    w[i] = o.w;
    acc[i] = o.acc;
    z[i] = o.z;
  }
}

// one task of FTRL: adam_task's rows and loads, accum / linear in place of m / v
template <typename V, int W, bool kPow>
__device__ inline void ftrl_task(const SlotCol& c, int64_t base, int64_t n, const FtrlArgs& a) {
  const int lane = lane_id();
  const int lpr = c.lpr_log2;
  const int grp = lane >> lpr;
  const int sub = lane & ((1 << lpr) - 1);
  const int groups = kWave >> lpr;
  const bool lane_on = sub * W < c.dim;
  int64_t r[kAdamItems];
  bool on[kAdamItems];
#pragma unroll
  for (int k = 0; k < kAdamItems; ++k) {
    const int64_t u = base + (int64_t)k * groups + grp;
    on[k] = lane_on && u < n;
    r[k] = on[k] ? __builtin_nontemporal_load(c.urows + u) : 0;
    on[k] = on[k] && (uint64_t)r[k] < (uint64_t)c.rows;   // (the reduce only emits rows of the table)
  }
  V w[kAdamItems], acc[kAdamItems], z[kAdamItems], g[kAdamItems];
#pragma unroll
  for (int k = 0; k < kAdamItems; ++k) {
    if (!on[k]) continue;
    const int64_t u = base + (int64_t)k * groups + grp;
    const int64_t off = r[k] * c.pitch + sub * W;
    w[k] = *reinterpret_cast<const V*>(c.w + off);
    acc[k] = *reinterpret_cast<const V*>(c.s0 + off);
    z[k] = *reinterpret_cast<const V*>(c.s1 + off);
    g[k] = __builtin_nontemporal_load(reinterpret_cast<const V*>(c.grows + u * c.dim + sub * W));
  }
#pragma unroll
  for (int k = 0; k < kAdamItems; ++k) {
    if (!on[k]) continue;
    const int64_t off = r[k] * c.pitch + sub * W;
    ftrl_v<kPow>(w[k], acc[k], z[k], g[k], a);
    *reinterpret_cast<V*>(c.s0 + off) = acc[k];
    *reinterpret_cast<V*>(c.s1 + off) = z[k];
    *reinterpret_cast<V*>(c.w + off) = w[k];
  }
}

template <bool kPow>
__global__ __launch_bounds__(kAdamBlock) void sparse_ftrl_apply_kernel(FtrlArgs a) {
  __shared__ int64_t s_end[kAdamMaxCols];
  __shared__ int64_t s_n[kAdamMaxCols];
  if (threadIdx.x < kWave) scan_tasks(a.c, a.n_cols, (int)threadIdx.x, s_end, s_n);
  __syncthreads();
  walk_tasks(a.c, a.n_cols, s_end, s_n, [&](const SlotCol& col, int64_t base, int64_t n) {
    if (col.vec4) {
      ftrl_task<f32x4, 4, kPow>(col, base, n, a);
    } else {
      ftrl_task<float, 1, kPow>(col, base, n, a);
    }
  });
}

int adam_cus() {
  static std::mutex mu;
  static int cache[64] = {0};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 256;
  std::lock_guard<std::mutex> lock(mu);
  if (cache[dev] == 0) {
    int n = 0;
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
    cache[dev] = n;
  }
  return cache[dev];
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


// the names a two-slot call's refusals use
struct SlotNames {
  const char* who;   // "group_lookup_bwd_adam"
  const char* opt;   // "Adam"
  const char* s0;    // "m"
  const char* s1;    // "v"
};

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

size_t slot_workspace_bytes(int32_t n_cols, const hbk_lookup_grad_column_t* cols) {
  if (n_cols <= 0 || cols == nullptr) return 0;
  const std::vector<hbk_lookup_grad_column_t> e = emit_form(n_cols, cols);
  size_t total = align256(hbk_group_lookup_bwd_workspace_bytes(n_cols, e.data()));
  for (int32_t c = 0; c < n_cols; ++c) total += slot_bytes(cols[c]);
  return total == 0 ? 0 : total + 256;
}

// phase 1: the reduce in its emit form (validates the rest of the columns); *e: the columns as the
// apply reads them (step-only slices carved from the workspace)
int run_emit_form(const char* who, int32_t n_cols, const hbk_lookup_grad_column_t* cols,
                  void* workspace, size_t workspace_bytes, hbk_stream_t stream_,
                  std::vector<hbk_lookup_grad_column_t>* e) {
  const size_t need = slot_workspace_bytes(n_cols, cols);
  HBK_REQUIRE(need == 0 || (workspace != nullptr && workspace_bytes >= need),
              "%s: workspace too small: need %zu bytes, got %zu", who, need, workspace_bytes);
  HBK_REQUIRE(((uintptr_t)workspace & 7) == 0, "%s: workspace must be 8-byte aligned", who);
  e->assign(cols, cols + n_cols);
  char* const base = reinterpret_cast<char*>(((uintptr_t)workspace + 255) & ~(uintptr_t)255);
  {
    const std::vector<hbk_lookup_grad_column_t> q = emit_form(n_cols, cols);
    char* slot = base + align256(hbk_group_lookup_bwd_workspace_bytes(n_cols, q.data()));
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
  }
  if (n_cols == 0) return HBK_OK;
  return hbk_group_lookup_bwd_apply(n_cols, e->data(), HBK_APPLY_SGD, 0.0f, base,
                                    workspace_bytes - (size_t)(base - (char*)workspace), stream_);
}

// phase 2's descriptors of columns c0 .. c1 (those with rows to step) into out; the number of them
// and the grid the launch needs
int fill_slot_cols(const std::vector<hbk_lookup_grad_column_t>& e, const std::vector<RowShape>& shapes,
                   float* const* s0, float* const* s1, int32_t c0, int32_t c1, SlotCol* out,
                   unsigned* blocks) {
  int64_t tasks = 0;
  int k = 0;
  for (int32_t c = c0; c < c1; ++c) {
    const hbk_lookup_grad_column_t& h = e[(size_t)c];
    if (h.n_ids <= 0 || h.rows <= 0) continue;
    SlotCol& d = out[k];
    d.w = h.table;
    d.s0 = s0[c];
    d.s1 = s1[c];
    d.urows = h.unique_rows;
    d.grows = h.grad_rows;
    d.nu = h.n_unique;
    d.rows = h.rows;
    d.cap = (int32_t)h.n_ids;
    d.dim = h.dim;
    d.pitch = h.table_pitch > 0 ? h.table_pitch : h.dim;
    const RowShape& shape = shapes[(size_t)c];   // (validated before the reduce)
    d.lpr_log2 = shape.lpr_log2;
    d.vec4 = shape.vec4;
    const int64_t rpt = (int64_t)(kWave >> shape.lpr_log2) * kAdamItems;
    tasks += (std::min<int64_t>(h.n_ids, h.rows) + rpt - 1) / rpt;
    ++k;
  }
  const int64_t want = (tasks + kAdamWaves - 1) / kAdamWaves;
  *blocks = (unsigned)std::max<int64_t>(1, std::min<int64_t>(want, (int64_t)adam_cus() * kAdamBlocksPerCU));
  return k;
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
}  // namespace hbk

extern "C" size_t hbk_group_lookup_bwd_adam_workspace_bytes(int32_t n_cols,
                                                            const hbk_lookup_grad_column_t* cols) {
  return hbk::slot_workspace_bytes(n_cols, cols);
}

extern "C" int hbk_group_lookup_bwd_adam(int32_t n_cols, const hbk_lookup_grad_column_t* cols,
                                         float* const* m, float* const* v, const hbk_adam_t* adam,
                                         float lr, void* workspace, size_t workspace_bytes,
                                         hbk_stream_t stream_) {
  using namespace hbk;
  static const SlotNames kNames = {"group_lookup_bwd_adam", "Adam", "m", "v"};
  HBK_REQUIRE(n_cols >= 0, "group_lookup_bwd_adam: n_cols must be >= 0, got %d", n_cols);
  int rc = adam_check(adam, lr, kNames.who);
  if (rc != HBK_OK) return rc;
  std::vector<RowShape> shapes;
  if ((rc = check_slot_columns(kNames, n_cols, cols, m, v, &shapes)) != HBK_OK) return rc;
  if (n_cols == 0 && !adam->finish) return HBK_OK;
  std::vector<hbk_lookup_grad_column_t> e;
  rc = run_emit_form(kNames.who, n_cols, cols, workspace, workspace_bytes, stream_, &e);
  if (rc != HBK_OK) return rc;
  hipStream_t stream = as_stream(stream_);

  // phase 2: the apply, kAdamMaxCols columns per launch
  for (int32_t c0 = 0; c0 < n_cols; c0 += kAdamMaxCols) {
    AdamArgs a;
    memset(&a, 0, sizeof(a));
    unsigned blocks = 0;
    a.n_cols = fill_slot_cols(e, shapes, m, v, c0, std::min(n_cols, c0 + kAdamMaxCols), a.c, &blocks);
    if (a.n_cols == 0) continue;
    a.powers = adam->beta_powers;
    a.lr = lr;
    a.beta1 = adam->beta1;
    a.beta2 = adam->beta2;
    a.eps = adam->epsilon;
    hipLaunchKernelGGL(sparse_adam_apply_kernel, dim3(blocks), dim3(kAdamBlock), 0, stream, a);
    HBK_HIP_OK(hipGetLastError());
  }
  if (adam->finish) {
    hipLaunchKernelGGL(adam_finish_kernel, dim3(1), dim3(kWave), 0, stream, adam->beta_powers,
                       adam->beta1, adam->beta2);
    HBK_HIP_OK(hipGetLastError());
  }
  return HBK_OK;
}

extern "C" size_t hbk_group_lookup_bwd_ftrl_workspace_bytes(int32_t n_cols,
                                                            const hbk_lookup_grad_column_t* cols) {
  return hbk::slot_workspace_bytes(n_cols, cols);
}

extern "C" int hbk_group_lookup_bwd_ftrl(int32_t n_cols, const hbk_lookup_grad_column_t* cols,
                                         float* const* accum, float* const* linear,
                                         const hbk_ftrl_t* ftrl, float lr, void* workspace,
                                         size_t workspace_bytes, hbk_stream_t stream_) {
  using namespace hbk;
  static const SlotNames kNames = {"group_lookup_bwd_ftrl", "FTRL", "accum", "linear"};
  HBK_REQUIRE(n_cols >= 0, "group_lookup_bwd_ftrl: n_cols must be >= 0, got %d", n_cols);
  int rc = ftrl_check(ftrl, lr, kNames.who);
  if (rc != HBK_OK) return rc;
  std::vector<RowShape> shapes;
  if ((rc = check_slot_columns(kNames, n_cols, cols, accum, linear, &shapes)) != HBK_OK) return rc;
  if (n_cols == 0) return HBK_OK;
  std::vector<hbk_lookup_grad_column_t> e;
  rc = run_emit_form(kNames.who, n_cols, cols, workspace, workspace_bytes, stream_, &e);
  if (rc != HBK_OK) return rc;
  hipStream_t stream = as_stream(stream_);

  // phase 2: the apply, kAdamMaxCols columns per launch; lr_power = -0.5 (TF's default) takes the
  // sqrtf instantiation, any other the powf one
  const bool use_pow = ftrl->lr_power != -0.5f;
  for (int32_t c0 = 0; c0 < n_cols; c0 += kAdamMaxCols) {
    FtrlArgs a;
    memset(&a, 0, sizeof(a));
    unsigned blocks = 0;
    a.n_cols = fill_slot_cols(e, shapes, accum, linear, c0, std::min(n_cols, c0 + kAdamMaxCols), a.c,
                              &blocks);
    if (a.n_cols == 0) continue;
    a.lr = lr;
    a.l1 = ftrl->l1;
    a.two_l2 = 2.0f * ftrl->l2;
    a.two_shrinkage = 2.0f * ftrl->l2_shrinkage;
    a.neg_lr_power = -ftrl->lr_power;
    if (use_pow) {
      hipLaunchKernelGGL(sparse_ftrl_apply_kernel<true>, dim3(blocks), dim3(kAdamBlock), 0, stream, a);
    } else {
      hipLaunchKernelGGL(sparse_ftrl_apply_kernel<false>, dim3(blocks), dim3(kAdamBlock), 0, stream, a);
    }
    HBK_HIP_OK(hipGetLastError());
  }
  return HBK_OK;
}
