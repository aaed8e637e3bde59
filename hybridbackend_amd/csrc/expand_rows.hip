// Key-deduplicated features (include/hbk.h, "Key-deduplicated features"): rows that are the same for many
// samples of a batch are looked up once per distinct key and EXPANDED to the batch on the device, and the
// batch gradient is REDUCED back to one row per key before the backward of the lookup runs.
//
//   hbk_expand_rows_n        out[b, :] = src[idx[b], :], a zero row for an index outside [0, n_keys).  A bit
//                            copy of 4-byte elements.  One launch per 64 columns; a lane group per output
//                            row, sized from the width (a power of two up to a wave); a group covers kFwdU
//                            chunks per lane, their loads issued together, and rows wider than that are tiled
//                            over more workgroups.
//   hbk_expand_index_build   the inverse of idx: order / splits (a CSR of the samples by key, ascending b
//                            inside a key) and the count of indices outside [0, n_keys).  A key kernel, the
//                            stable LSD sort of det_prims.hip, one lower bound per key.
//   hbk_expand_rows_grad_n   out[u, :] = src[order[splits[u]], :] + src[order[splits[u] + 1], :] + ..., one
//                            sequential fp32 chain per element: a lane group per (key, width tile), kAhead
//                            rows of the list loaded ahead of the adds.  Every row of out is written.
//
// Plain loads and vector stores, no atomics anywhere.  A column takes 16-byte chunks when its width, both
// strides and both addresses allow it, else 4-byte chunks: the host decides per column.  An index is checked
// against [0, n_keys) -- and order / splits against [0, n_samples) -- before any address is formed from it.
#include <algorithm>
#include <utility>
#include <vector>

#include "lookup_common.h"

namespace hbk {

size_t det_sort_temp_bytes(size_t n, int end_bit);
int det_sort_pairs(void* temp, size_t temp_bytes, const uint64_t* keys_in, uint64_t* keys_out,
                   const uint32_t* vals_in, uint32_t* vals_out, size_t n, int end_bit, hipStream_t stream);

namespace {

constexpr int kBlock = 256;            // 4 waves
constexpr int kFwdU = 4;               // chunks per lane of the forward: independent loads in flight
constexpr int kAhead = 8;              // rows of a key's list the transpose loads ahead of its adds
constexpr int kMaxColsPerLaunch = 64;  // one ballot finds the column; ExpandArgs travels by value

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

struct ExpandCol {
  const uint32_t* src;
  uint32_t* out;
  int64_t src_stride;   // elements
  int64_t out_stride;
  int32_t chunks;       // per row: width / 4 (16-byte chunks) or width
  int32_t wtiles;       // workgroup tiles over the width
  int32_t g_log2;       // lanes of a row's lane group: 2^g_log2 <= 64
  int32_t vec4;
};

struct ExpandArgs {
  int32_t n_cols;
  int32_t n_samples;
  int32_t n_keys;
  int32_t idx64;
  const void* idx;          // forward; NULL: identity
  const int32_t* order;     // transpose
  const int32_t* splits;
  int32_t tile_start[kMaxColsPerLaunch + 1];
  ExpandCol col[kMaxColsPerLaunch];
};
static_assert(sizeof(ExpandArgs) <= 4096, "kernarg budget");

template <typename V>
__device__ inline V zero_bits();
template <>
__device__ inline u32x4 zero_bits<u32x4>() { return u32x4{0u, 0u, 0u, 0u}; }
template <>
__device__ inline uint32_t zero_bits<uint32_t>() { return 0u; }

template <typename V>
__device__ inline void expand_rows_col(const ExpandArgs& a, const ExpandCol& c, int local) {
  constexpr int kElems = (int)(sizeof(V) / sizeof(uint32_t));
  const int g = 1 << c.g_log2;
  const int rows = kBlock >> c.g_log2;            // output rows per workgroup
  const int rt = local / c.wtiles, wt = local - rt * c.wtiles;
  const int64_t b = (int64_t)rt * rows + (int64_t)(threadIdx.x >> c.g_log2);
  const int sub = (int)threadIdx.x & (g - 1);
  if (b >= (int64_t)a.n_samples) return;
  int64_t v = b;
  bool ok = true;
  if (a.idx != nullptr) {
    v = load_id(a.idx, a.idx64 != 0, b);
    ok = v >= 0 && v < (int64_t)a.n_keys;         // (checked before an address is formed from it)
  }
  const int64_t ch0 = (int64_t)wt * g * kFwdU + sub;
  const uint32_t* from = c.src + (ok ? v : 0) * c.src_stride;
  uint32_t* to = c.out + b * c.out_stride;
  V r[kFwdU];
#pragma unroll
  for (int k = 0; k < kFwdU; ++k) {
    const int64_t ch = ch0 + (int64_t)k * g;
    r[k] = zero_bits<V>();
    if (ok && ch < (int64_t)c.chunks) r[k] = *reinterpret_cast<const V*>(from + ch * kElems);
  }
#pragma unroll
  for (int k = 0; k < kFwdU; ++k) {
    const int64_t ch = ch0 + (int64_t)k * g;
    if (ch < (int64_t)c.chunks) *reinterpret_cast<V*>(to + ch * kElems) = r[k];
  }
}

__global__ __launch_bounds__(kBlock) void expand_rows_kernel(const ExpandArgs a) {
  const int b = (int)blockIdx.x;
  const int ci = column_of(a.tile_start, a.n_cols, b, lane_id());
  const ExpandCol& c = a.col[ci];
  const int local = b - a.tile_start[ci];
  if (c.vec4) {
    expand_rows_col<u32x4>(a, c, local);
  } else {
    expand_rows_col<uint32_t>(a, c, local);
  }
}

// The sequential sum of a key's list, first term first: acc = x_0, then acc = acc + x_j.  (Not 0 + x_0: that
// would turn a -0 into +0.)  kAhead rows of the list are loaded before they are added, in order.
template <typename V>
__device__ inline void expand_grad_col(const ExpandArgs& a, const ExpandCol& c, int local) {
  constexpr int kElems = (int)(sizeof(V) / sizeof(float));
  const int g = 1 << c.g_log2;
  const int keys = kBlock >> c.g_log2;            // keys per workgroup
  const int kt = local / c.wtiles, wt = local - kt * c.wtiles;
  const int64_t u = (int64_t)kt * keys + (int64_t)(threadIdx.x >> c.g_log2);
  const int64_t ch = (int64_t)wt * g + ((int)threadIdx.x & (g - 1));
  if (u >= (int64_t)a.n_keys || ch >= (int64_t)c.chunks) return;
  int32_t beg = a.splits[u], end = a.splits[u + 1];
  beg = beg < 0 ? 0 : beg;
  end = end > a.n_samples ? a.n_samples : end;
  const float* from = reinterpret_cast<const float*>(c.src) + ch * kElems;
  V acc = zero_v<V>();
  for (int32_t j0 = beg; j0 < end; j0 += kAhead) {
    V r[kAhead];
    bool has[kAhead];
#pragma unroll
    for (int k = 0; k < kAhead; ++k) {
      has[k] = false;
      r[k] = zero_v<V>();
      if (j0 + k < end) {
        const int32_t s = a.order[j0 + k];
        has[k] = (uint32_t)s < (uint32_t)a.n_samples;   // (what the build wrote always is)
        if (has[k]) r[k] = *reinterpret_cast<const V*>(from + (int64_t)s * c.src_stride);
      }
    }
#pragma unroll
    for (int k = 0; k < kAhead; ++k) {
      if (has[k]) acc = (j0 + k == beg) ? r[k] : acc + r[k];
    }
  }
  *reinterpret_cast<V*>(reinterpret_cast<float*>(c.out) + u * c.out_stride + ch * kElems) = acc;
}

__global__ __launch_bounds__(kBlock) void expand_rows_grad_kernel(const ExpandArgs a) {
  const int b = (int)blockIdx.x;
  const int ci = column_of(a.tile_start, a.n_cols, b, lane_id());
  const ExpandCol& c = a.col[ci];
  const int local = b - a.tile_start[ci];
  if (c.vec4) {
    expand_grad_col<f32x4>(a, c, local);
  } else {
    expand_grad_col<float>(a, c, local);
  }
}

// (idx[b] valid ? idx[b] : n_keys, b): the pairs the stable sort takes
__global__ __launch_bounds__(kBlock) void expand_index_keys_kernel(const void* idx, int idx64, int32_t n_samples,
                                                                   int32_t n_keys, uint64_t* keys, uint32_t* vals) {
  const int64_t b = (int64_t)blockIdx.x * kBlock + (int64_t)threadIdx.x;
  if (b >= (int64_t)n_samples) return;
  const int64_t v = load_id(idx, idx64 != 0, b);
  keys[b] = (v >= 0 && v < (int64_t)n_keys) ? (uint64_t)v : (uint64_t)n_keys;
  vals[b] = (uint32_t)b;
}

// splits[u] = the first position of the sorted keys that holds a key >= u, u in [0, n_keys]; the samples in no
// list are those behind splits[n_keys]
__global__ __launch_bounds__(kBlock) void expand_index_splits_kernel(const uint64_t* sorted, int32_t n_samples,
                                                                     int32_t n_keys, int32_t* splits,
                                                                     int32_t* invalid) {
  const int64_t u = (int64_t)blockIdx.x * kBlock + (int64_t)threadIdx.x;
  if (u > (int64_t)n_keys) return;
  int32_t lo = 0, hi = n_samples;
  while (lo < hi) {
    const int32_t mid = lo + ((hi - lo) >> 1);
    if (sorted[mid] < (uint64_t)u) {
      lo = mid + 1;
    } else {
      hi = mid;
    }
  }
  splits[u] = lo;
  if (u == (int64_t)n_keys) invalid[0] = n_samples - lo;
}

inline int lane_group_log2(int64_t chunks) {
  int l = 0;
  while (l < 6 && (1ll << l) < chunks) ++l;
  return l;
}

inline size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

// bits [0, end_bit) hold every key the sort sees: 0 .. n_keys (the value of a sample in no list)
inline int index_end_bit(int64_t n_keys) {
  int bits = 1;
  while (bits < 63 && (1ll << bits) <= n_keys) ++bits;
  return bits;
}

struct IndexLayout {
  size_t keys, sorted, vals, temp, temp_bytes, total;
};

inline IndexLayout index_layout(int64_t n_samples, int64_t n_keys) {
  IndexLayout l;
  const size_t n = (size_t)n_samples;
  size_t at = 0;
  l.keys = at;
  at = align256(at + n * sizeof(uint64_t));
  l.sorted = at;
  at = align256(at + n * sizeof(uint64_t));
  l.vals = at;
  at = align256(at + n * sizeof(uint32_t));
  l.temp = at;
  l.temp_bytes = n > 0 ? det_sort_temp_bytes(n, index_end_bit(n_keys)) : 0;
  l.total = at + align256(l.temp_bytes);
  return l;
}

inline bool sizes_ok(int64_t n_samples, int64_t n_keys) {
  return n_samples >= 0 && n_keys >= 0 && n_samples < (1ll << 31) && n_keys < (1ll << 31);
}

// what both row launches check of their columns; `reads` / `writes`: the call has rows to read from src / to
// write to out (without them a NULL pointer is fine)
int check_columns(const char* who, int32_t n_cols, const hbk_expand_column_t* cols, int64_t n_samples,
                  int64_t n_keys, bool reads, bool writes) {
  HBK_REQUIRE(n_cols >= 0, "%s: n_cols must be >= 0, got %d", who, n_cols);
  HBK_REQUIRE(n_cols == 0 || cols != nullptr, "%s: cols is NULL", who);
  HBK_REQUIRE(sizes_ok(n_samples, n_keys), "%s: n_samples (%lld) and n_keys (%lld) must be in [0, 2^31)", who,
              (long long)n_samples, (long long)n_keys);
  std::vector<std::pair<uintptr_t, int32_t>> outs;
  for (int32_t c = 0; c < n_cols; ++c) {
    const hbk_expand_column_t& h = cols[c];
    HBK_REQUIRE(h.width >= 1, "%s: column %d: width must be >= 1, got %d", who, c, h.width);
    HBK_REQUIRE(h.src_stride == 0 || h.src_stride >= (int64_t)h.width,
                "%s: column %d: src_stride %lld is below the width %d (0: contiguous)", who, c,
                (long long)h.src_stride, h.width);
    HBK_REQUIRE(h.out_stride == 0 || h.out_stride >= (int64_t)h.width,
                "%s: column %d: out_stride %lld is below the width %d (0: contiguous)", who, c,
                (long long)h.out_stride, h.width);
    HBK_REQUIRE(!reads || h.src != nullptr, "%s: column %d: src is NULL with rows to read", who, c);
    HBK_REQUIRE(!writes || h.out != nullptr, "%s: column %d: out is NULL with rows to write", who, c);
    if (h.out != nullptr) outs.emplace_back(reinterpret_cast<uintptr_t>(h.out), c);
  }
  std::sort(outs.begin(), outs.end());
  for (size_t i = 1; i < outs.size(); ++i) {
    HBK_REQUIRE(outs[i].first != outs[i - 1].first, "%s: column %d: names the same out as column %d", who,
                outs[i].second, outs[i - 1].second);
  }
  return HBK_OK;
}

// k columns as launch arguments; rows_out: the rows every column writes, `per_lane`: the chunks of a row one
// lane covers.  Returns the workgroups of the launch, -1 when they pass 2^31.
int64_t fill_columns(ExpandArgs* args, const hbk_expand_column_t* cols, int32_t k, int64_t rows_out, int per_lane) {
  int64_t groups = 0;
  args->n_cols = k;
  args->tile_start[0] = 0;
  for (int32_t i = 0; i < k; ++i) {
    const hbk_expand_column_t& h = cols[i];
    ExpandCol& d = args->col[i];
    d.src = static_cast<const uint32_t*>(h.src);
    d.out = static_cast<uint32_t*>(h.out);
    d.src_stride = h.src_stride != 0 ? h.src_stride : (int64_t)h.width;
    d.out_stride = h.out_stride != 0 ? h.out_stride : (int64_t)h.width;
    const uintptr_t bits = reinterpret_cast<uintptr_t>(h.src) | reinterpret_cast<uintptr_t>(h.out);
    d.vec4 = (h.width % 4 == 0 && d.src_stride % 4 == 0 && d.out_stride % 4 == 0 && bits % 16 == 0) ? 1 : 0;
    d.chunks = d.vec4 ? h.width / 4 : h.width;
    d.g_log2 = lane_group_log2(d.chunks);
    const int64_t span = (int64_t)per_lane << d.g_log2;
    d.wtiles = (int32_t)((d.chunks + span - 1) / span);
    const int64_t rows_per_group = kBlock >> d.g_log2;
    groups += (rows_out + rows_per_group - 1) / rows_per_group * d.wtiles;
    if (groups >= (1ll << 31)) return -1;
    args->tile_start[i + 1] = (int32_t)groups;
  }
  return groups;
}

int expand_rows(int32_t n_cols, const hbk_expand_column_t* cols, const void* idx, int32_t idx_dtype,
                int64_t n_samples, int64_t n_keys, hbk_stream_t stream) {
  const char* who = "expand_rows_n";
  HBK_REQUIRE(idx == nullptr || idx_dtype == HBK_INT32 || idx_dtype == HBK_INT64,
              "%s: idx must be int32 or int64, got dtype %d", who, idx_dtype);
  const bool identity = idx == nullptr;
  if (int rc = check_columns(who, n_cols, cols, n_samples, n_keys, n_samples > 0 && (identity || n_keys > 0),
                             n_samples > 0)) {
    return rc;
  }
  if (n_samples == 0) return HBK_OK;
  hipStream_t s = as_stream(stream);
  for (int32_t c0 = 0; c0 < n_cols; c0 += kMaxColsPerLaunch) {
    ExpandArgs args;
    const int32_t k = n_cols - c0 < kMaxColsPerLaunch ? n_cols - c0 : kMaxColsPerLaunch;
    const int64_t groups = fill_columns(&args, cols + c0, k, n_samples, kFwdU);
    HBK_REQUIRE(groups >= 0, "%s: grid too large", who);
    args.n_samples = (int32_t)n_samples;
    args.n_keys = (int32_t)n_keys;
    args.idx = idx;
    args.idx64 = idx_dtype == HBK_INT64;
    args.order = nullptr;
    args.splits = nullptr;
    hipLaunchKernelGGL(expand_rows_kernel, dim3((unsigned)groups), dim3(kBlock), 0, s, args);
    HBK_HIP_OK(hipGetLastError());
  }
  return HBK_OK;
}

int expand_rows_grad(int32_t n_cols, const hbk_expand_column_t* cols, const int32_t* order, const int32_t* splits,
                     int64_t n_samples, int64_t n_keys, hbk_stream_t stream) {
  const char* who = "expand_rows_grad_n";
  if (int rc = check_columns(who, n_cols, cols, n_samples, n_keys, n_samples > 0 && n_keys > 0, n_keys > 0)) {
    return rc;
  }
  HBK_REQUIRE(n_keys == 0 || splits != nullptr, "%s: splits is NULL", who);
  HBK_REQUIRE(n_keys == 0 || n_samples == 0 || order != nullptr, "%s: order is NULL", who);
  if (n_keys == 0) return HBK_OK;
  hipStream_t s = as_stream(stream);
  for (int32_t c0 = 0; c0 < n_cols; c0 += kMaxColsPerLaunch) {
    ExpandArgs args;
    const int32_t k = n_cols - c0 < kMaxColsPerLaunch ? n_cols - c0 : kMaxColsPerLaunch;
    const int64_t groups = fill_columns(&args, cols + c0, k, n_keys, 1);
    HBK_REQUIRE(groups >= 0, "%s: grid too large", who);
    args.n_samples = (int32_t)n_samples;
    args.n_keys = (int32_t)n_keys;
    args.idx = nullptr;
    args.idx64 = 0;
    args.order = order;
    args.splits = splits;
    hipLaunchKernelGGL(expand_rows_grad_kernel, dim3((unsigned)groups), dim3(kBlock), 0, s, args);
    HBK_HIP_OK(hipGetLastError());
  }
  return HBK_OK;
}

int expand_index_build(const void* idx, int32_t idx_dtype, int64_t n_samples, int64_t n_keys, int32_t* order,
                       int32_t* splits, int32_t* invalid, void* workspace, size_t workspace_bytes,
                       hbk_stream_t stream) {
  const char* who = "expand_index_build";
  HBK_REQUIRE(sizes_ok(n_samples, n_keys), "%s: n_samples (%lld) and n_keys (%lld) must be in [0, 2^31)", who,
              (long long)n_samples, (long long)n_keys);
  HBK_REQUIRE(idx_dtype == HBK_INT32 || idx_dtype == HBK_INT64, "%s: idx must be int32 or int64, got dtype %d",
              who, idx_dtype);
  HBK_REQUIRE(n_samples == 0 || idx != nullptr, "%s: idx is NULL", who);
  HBK_REQUIRE(n_samples == 0 || order != nullptr, "%s: order is NULL", who);
  HBK_REQUIRE(splits != nullptr && invalid != nullptr, "%s: splits and invalid are written whatever the sizes, "
              "and one of them is NULL", who);
  const IndexLayout l = index_layout(n_samples, n_keys);
  HBK_REQUIRE(l.total <= workspace_bytes && (l.total == 0 || workspace != nullptr),
              "%s: a workspace of %zu bytes is too small: %zu bytes are needed (hbk_expand_index_workspace_bytes)",
              who, workspace != nullptr ? workspace_bytes : (size_t)0, l.total);
  hipStream_t s = as_stream(stream);
  char* ws = static_cast<char*>(workspace);
  uint64_t* sorted = reinterpret_cast<uint64_t*>(ws + l.sorted);
  if (n_samples > 0) {
    uint64_t* keys = reinterpret_cast<uint64_t*>(ws + l.keys);
    uint32_t* vals = reinterpret_cast<uint32_t*>(ws + l.vals);
    const unsigned tiles = (unsigned)((n_samples + kBlock - 1) / kBlock);
    hipLaunchKernelGGL(expand_index_keys_kernel, dim3(tiles), dim3(kBlock), 0, s, idx, idx_dtype == HBK_INT64,
                       (int32_t)n_samples, (int32_t)n_keys, keys, vals);
    HBK_HIP_OK(hipGetLastError());
    if (int rc = det_sort_pairs(ws + l.temp, l.temp_bytes, keys, sorted, vals, reinterpret_cast<uint32_t*>(order),
                                (size_t)n_samples, index_end_bit(n_keys), s)) {
      return rc;
    }
  }
  const unsigned tiles = (unsigned)((n_keys + 1 + kBlock - 1) / kBlock);
  hipLaunchKernelGGL(expand_index_splits_kernel, dim3(tiles), dim3(kBlock), 0, s, sorted, (int32_t)n_samples,
                     (int32_t)n_keys, splits, invalid);
  HBK_HIP_OK(hipGetLastError());
  return HBK_OK;
}

}  // namespace
}  // namespace hbk

extern "C" int hbk_expand_rows_n(int32_t n_cols, const hbk_expand_column_t* cols, const void* idx,
                                 int32_t idx_dtype, int64_t n_samples, int64_t n_keys, hbk_stream_t stream) {
  return hbk::expand_rows(n_cols, cols, idx, idx_dtype, n_samples, n_keys, stream);
}

extern "C" size_t hbk_expand_index_workspace_bytes(int64_t n_samples, int64_t n_keys) {
  if (!hbk::sizes_ok(n_samples, n_keys)) return 0;
  return hbk::index_layout(n_samples, n_keys).total;
}

extern "C" int hbk_expand_index_build(const void* idx, int32_t idx_dtype, int64_t n_samples, int64_t n_keys,
                                      int32_t* order, int32_t* splits, int32_t* invalid, void* workspace,
                                      size_t workspace_bytes, hbk_stream_t stream) {
  return hbk::expand_index_build(idx, idx_dtype, n_samples, n_keys, order, splits, invalid, workspace,
                                 workspace_bytes, stream);
}

extern "C" int hbk_expand_rows_grad_n(int32_t n_cols, const hbk_expand_column_t* cols, const int32_t* order,
                                      const int32_t* splits, int64_t n_samples, int64_t n_keys,
                                      hbk_stream_t stream) {
  return hbk::expand_rows_grad(n_cols, cols, order, splits, n_samples, n_keys, stream);
}
