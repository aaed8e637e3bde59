// Lazy Adam sparse optimizer step (tf.contrib.opt.LazyAdamOptimizer's sparse apply, TF 1.15) after the
// grouped backward: hbk_group_lookup_bwd_adam.
//
// Two phases.  (1) The backward in its emit form (hbk_group_lookup_bwd_apply, apply_lr = 0) writes every
// column's distinct rows, their summed gradient rows and n_unique -- into the caller's buffers or, step
// only, into buffers carved from this call's workspace.  Every reduce plan, the deterministic modes,
// weighted columns and segmented inputs come from there unchanged, and so does the guarantee that each
// distinct row appears exactly once (Adam is not additive: a row stepped twice would decay its moments
// twice).  (2) ONE apply launch for up to kAdamMaxCols columns: sparse_adam_apply_kernel.
//
// The apply kernel.  Work is counted in wave tasks: a task is kAdamItems rows per lane group of one
// column, a lane group holds one row (f32x4 chunks when dim % 4 == 0 and every address is 16-byte
// aligned, scalar chunks otherwise -- the reduce's rule, make_rowshape).  Wave 0 of every workgroup
// reads the columns' n_unique from the device and scans their task counts into LDS; the grid is sized
// from the host-known capacities only and walks the tasks grid-stride, so the call needs no host sync
// and can be captured in a graph.  A lane issues the w / m / v / g loads of all its kAdamItems rows
// before any arithmetic: random rows are bound by the request rate (~49 G requests/s), so
// what matters is how many are in flight.  grad_rows and unique_rows are read once (non-temporal).
// The bias-corrected rate lr_t is computed once per workgroup from the device beta powers; the
// powers advance after the apply, in stream order (adam_finish_kernel), when the call asks for it.
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

struct AdamCol {
  float* w;
  float* m;
  float* v;
  const int64_t* urows;
  const float* grows;       // [cap, dim] contiguous
  const int32_t* nu;
  int64_t rows;
  int32_t cap;              // n_ids: n_unique never exceeds it
  int32_t dim;
  int32_t pitch;            // floats between rows of w, m and v
  int32_t lpr_log2;
  int32_t vec4;
  int32_t pad;
};

struct AdamArgs {
  AdamCol c[kAdamMaxCols];
  const float* powers;
  float lr, beta1, beta2, eps;
  int32_t n_cols;
};
static_assert(sizeof(AdamArgs) <= 8192, "kernarg budget");

__device__ inline float sqrt_v(float a) { return sqrtf(a); }
__device__ inline f32x4 sqrt_v(f32x4 a) { return f32x4{sqrtf(a.x), sqrtf(a.y), sqrtf(a.z), sqrtf(a.w)}; }

// one task: rows base + k * groups + grp (k < kAdamItems) of column c; W floats per lane chunk
template <typename V, int W>
__device__ inline void adam_task(const AdamCol& c, int64_t base, int64_t n, float lr_t, float beta1,
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
    m[k] = *reinterpret_cast<const V*>(c.m + off);
    v[k] = *reinterpret_cast<const V*>(c.v + off);
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
    *reinterpret_cast<V*>(c.m + off) = mk;
    *reinterpret_cast<V*>(c.v + off) = vk;
    *reinterpret_cast<V*>(c.w + off) = wk;
  }
}

__global__ __launch_bounds__(kAdamBlock) void sparse_adam_apply_kernel(AdamArgs a) {
  __shared__ int64_t s_end[kAdamMaxCols];   // inclusive prefix of the columns' task counts
  __shared__ int64_t s_n[kAdamMaxCols];     // their n_unique (clamped to the capacity)
  __shared__ float s_lr_t;
  if (threadIdx.x < kWave) {
    const int lane = (int)threadIdx.x;
    int64_t tasks = 0;
    if (lane < a.n_cols) {
      const AdamCol& c = a.c[lane];
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
    if (lane < a.n_cols) s_end[lane] = tasks;
    if (lane == 0) {
      const float b1p = a.powers[0], b2p = a.powers[1];
      s_lr_t = (a.lr * sqrtf(1.0f - b2p)) / (1.0f - b1p);
    }
  }
  __syncthreads();
  const int64_t total = s_end[a.n_cols - 1];
  const float lr_t = s_lr_t;
  int c = 0;
  for (int64_t t = (int64_t)blockIdx.x * kAdamWaves + threadIdx.x / kWave; t < total;
       t += (int64_t)gridDim.x * kAdamWaves) {
    while (s_end[c] <= t) ++c;   // (t only grows: the column only moves forward)
    const AdamCol& col = a.c[c];
    const int64_t t0 = c == 0 ? 0 : s_end[c - 1];
    const int64_t base = (t - t0) * ((int64_t)(kWave >> col.lpr_log2) * kAdamItems);
    if (col.vec4) {
      adam_task<f32x4, 4>(col, base, s_n[c], lr_t, a.beta1, a.beta2, a.eps);
    } else {
      adam_task<float, 1>(col, base, s_n[c], lr_t, a.beta1, a.beta2, a.eps);
    }
  }
}

// TF's _finish: beta1^t, beta2^t -> beta1^(t+1), beta2^(t+1), one fp32 product each
__global__ void adam_finish_kernel(float* powers, float beta1, float beta2) {
  if (threadIdx.x == 0) {
    powers[0] = powers[0] * beta1;
    powers[1] = powers[1] * beta2;
  }
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
}  // namespace hbk

extern "C" size_t hbk_group_lookup_bwd_adam_workspace_bytes(int32_t n_cols,
                                                            const hbk_lookup_grad_column_t* cols) {
  using namespace hbk;
  if (n_cols <= 0 || cols == nullptr) return 0;
  const std::vector<hbk_lookup_grad_column_t> e = emit_form(n_cols, cols);
  size_t total = align256(hbk_group_lookup_bwd_workspace_bytes(n_cols, e.data()));
  for (int32_t c = 0; c < n_cols; ++c) total += slot_bytes(cols[c]);
  return total == 0 ? 0 : total + 256;
}

extern "C" int hbk_group_lookup_bwd_adam(int32_t n_cols, const hbk_lookup_grad_column_t* cols,
                                         float* const* m, float* const* v, const hbk_adam_t* adam,
                                         float lr, void* workspace, size_t workspace_bytes,
                                         hbk_stream_t stream_) {
  using namespace hbk;
  HBK_REQUIRE(n_cols >= 0, "group_lookup_bwd_adam: n_cols must be >= 0, got %d", n_cols);
  {
    const int rc = adam_check(adam, lr, "group_lookup_bwd_adam");
    if (rc != HBK_OK) return rc;
  }
  HBK_REQUIRE(n_cols == 0 || cols != nullptr, "group_lookup_bwd_adam: cols is NULL");
  HBK_REQUIRE(n_cols == 0 || (m != nullptr && v != nullptr),
              "group_lookup_bwd_adam: the m / v arrays are NULL");
  std::vector<uintptr_t> seen;
  seen.reserve((size_t)n_cols * 3);
  std::vector<RowShape> shapes((size_t)n_cols);
  for (int32_t c = 0; c < n_cols; ++c) {
    const hbk_lookup_grad_column_t& h = cols[c];
    HBK_REQUIRE(m[c] != nullptr, "group_lookup_bwd_adam: column %d: m is NULL", c);
    HBK_REQUIRE(v[c] != nullptr, "group_lookup_bwd_adam: column %d: v is NULL", c);
    HBK_REQUIRE(m[c] != v[c], "group_lookup_bwd_adam: column %d: m and v are the same buffer", c);
    HBK_REQUIRE(m[c] != h.table, "group_lookup_bwd_adam: column %d: m is the table", c);
    HBK_REQUIRE(v[c] != h.table, "group_lookup_bwd_adam: column %d: v is the table", c);
    HBK_REQUIRE(h.accum == nullptr,
                "group_lookup_bwd_adam: column %d: accum must be NULL (Adam's slots are m and v)", c);
    HBK_REQUIRE(h.n_ids == 0 || h.table != nullptr, "group_lookup_bwd_adam: column %d: table is NULL", c);
    HBK_REQUIRE(h.n_ids < (1ll << 30), "group_lookup_bwd_adam: column %d: more than 2^30-1 ids", c);
    HBK_REQUIRE(h.dim >= 1, "group_lookup_bwd_adam: column %d: dim must be >= 1", c);
    HBK_REQUIRE(h.table_pitch == 0 || h.table_pitch >= h.dim,
                "group_lookup_bwd_adam: column %d: table_pitch %d is smaller than dim %d", c,
                h.table_pitch, h.dim);
    HBK_REQUIRE(h.n_ids == 0 || (h.unique_rows != nullptr) == (h.grad_rows != nullptr),
                "group_lookup_bwd_adam: column %d: unique_rows and grad_rows go together", c);
    // the apply's row shape, checked here -- before the reduce runs -- with the alignment phase 2
    // sees (step-only slices are carved 256-byte aligned from the workspace: they add no bits)
    const int32_t pitch = h.table_pitch > 0 ? h.table_pitch : h.dim;
    HBK_REQUIRE(h.n_ids <= 0 ||
                    make_rowshape(h.dim,
                                  (uintptr_t)h.table | (uintptr_t)m[c] | (uintptr_t)v[c] |
                                      (uintptr_t)h.grad_rows | ((uintptr_t)(uint32_t)pitch * 4),
                                  &shapes[(size_t)c]),
                "group_lookup_bwd_adam: column %d: dim %d needs more than 64 lanes per row (at most "
                "256 with 16-byte aligned table / m / v / grad_rows / pitch, 64 otherwise)", c, h.dim);
    if (h.table != nullptr) seen.push_back((uintptr_t)h.table);
    seen.push_back((uintptr_t)m[c]);
    seen.push_back((uintptr_t)v[c]);
  }
  std::sort(seen.begin(), seen.end());
  HBK_REQUIRE(std::adjacent_find(seen.begin(), seen.end()) == seen.end(),
              "group_lookup_bwd_adam: two columns name the same table, m or v (Adam is not "
              "additive: a row stepped twice in one call would race)");
  if (n_cols == 0 && !adam->finish) return HBK_OK;
  const size_t need = hbk_group_lookup_bwd_adam_workspace_bytes(n_cols, cols);
  HBK_REQUIRE(need == 0 || (workspace != nullptr && workspace_bytes >= need),
              "group_lookup_bwd_adam: workspace too small: need %zu bytes, got %zu", need,
              workspace_bytes);
  HBK_REQUIRE(((uintptr_t)workspace & 7) == 0, "group_lookup_bwd_adam: workspace must be 8-byte aligned");
  hipStream_t stream = as_stream(stream_);

  // phase 1: the reduce in its emit form (validates the rest of the columns)
  std::vector<hbk_lookup_grad_column_t> e(cols, cols + n_cols);
  char* const base = reinterpret_cast<char*>(((uintptr_t)workspace + 255) & ~(uintptr_t)255);
  {
    const std::vector<hbk_lookup_grad_column_t> q = emit_form(n_cols, cols);
    char* slot = base + align256(hbk_group_lookup_bwd_workspace_bytes(n_cols, q.data()));
    for (int32_t c = 0; c < n_cols; ++c) {
      hbk_lookup_grad_column_t& h = e[(size_t)c];
      h.accum = nullptr;
      if (h.grad_rows == nullptr && h.n_ids > 0) {
        h.unique_rows = reinterpret_cast<int64_t*>(slot);
        slot += align256((size_t)h.n_ids * 8);
        h.grad_rows = reinterpret_cast<float*>(slot);
        slot += align256((size_t)h.n_ids * h.dim * 4);
      }
    }
  }
  if (n_cols > 0) {
    const int rc = hbk_group_lookup_bwd_apply(n_cols, e.data(), HBK_APPLY_SGD, 0.0f, base,
                                              workspace_bytes - (size_t)(base - (char*)workspace),
                                              stream_);
    if (rc != HBK_OK) return rc;
  }

  // phase 2: the apply, kAdamMaxCols columns per launch
  const int cap_blocks = adam_cus() * kAdamBlocksPerCU;
  for (int32_t c0 = 0; c0 < n_cols; c0 += kAdamMaxCols) {
    const int32_t c1 = std::min(n_cols, c0 + kAdamMaxCols);
    AdamArgs a;
    memset(&a, 0, sizeof(a));
    a.powers = adam->beta_powers;
    a.lr = lr;
    a.beta1 = adam->beta1;
    a.beta2 = adam->beta2;
    a.eps = adam->epsilon;
    int64_t tasks = 0;
    int k = 0;
    for (int32_t c = c0; c < c1; ++c) {
      const hbk_lookup_grad_column_t& h = e[(size_t)c];
      if (h.n_ids <= 0 || h.rows <= 0) continue;
      AdamCol& d = a.c[k];
      d.w = h.table;
      d.m = m[c];
      d.v = v[c];
      d.urows = h.unique_rows;
      d.grows = h.grad_rows;
      d.nu = h.n_unique;
      d.rows = h.rows;
      d.cap = (int32_t)h.n_ids;
      d.dim = h.dim;
      d.pitch = h.table_pitch > 0 ? h.table_pitch : h.dim;
      const RowShape& shape = shapes[(size_t)c];   // (validated above)
      d.lpr_log2 = shape.lpr_log2;
      d.vec4 = shape.vec4;
      const int64_t rpt = (int64_t)(kWave >> shape.lpr_log2) * kAdamItems;
      tasks += (std::min<int64_t>(h.n_ids, h.rows) + rpt - 1) / rpt;
      ++k;
    }
    if (k == 0) continue;
    a.n_cols = k;
    const int64_t want = (tasks + kAdamWaves - 1) / kAdamWaves;
    const unsigned blocks = (unsigned)std::max<int64_t>(1, std::min<int64_t>(want, cap_blocks));
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
