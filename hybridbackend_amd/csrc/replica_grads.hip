// Gradients of replicated tables across ranks in their dense form (include/hbk.h, "Gradients of REPLICATED
// tables"): a table kept on every rank has at most max(batch, W) rows, so its dense gradient is no larger than
// the gradient block the backward already reads, and one allreduce of one bucket replaces two gathers per column.
//
//   hbk_replica_grads_pack_n   clears the bucket (a memset on the stream), then scatters every column's
//                              IndexedSlices into its block: block[r, :] = grad_rows[u, :], touched[r] = 1.0f.
//                              One launch per 64 columns; a lane group per slice row, sized from the width (a
//                              power of two up to a wave, one chunk per lane: the apply's row shape).
//   hbk_replica_grads_rows_n   after the allreduce: urows[r] = touched[r] != 0 ? r : -1, a thread per row.
//
// Bandwidth kernels: plain loads and vector stores, no LDS, no atomics (the rows of a column's slices are
// distinct).  A column takes 16-byte lanes when its width and both addresses allow it, else 4-byte lanes: the
// host decides per column (make_rowshape, the rule of expand_rows.hip and of the apply).  n_unique is read on
// the device and clamped to the capacity; a row number is checked against [0, rows) before any address is
// formed from it; the slices are read once (non-temporal).  The grid is sized from the host-known capacities, so
// neither call reads device memory on the host and both can be captured.
#include <algorithm>
#include <utility>
#include <vector>

#include "lookup_common.h"

namespace hbk {
namespace {

constexpr int kBlock = 256;            // 4 waves
constexpr int kMaxColsPerLaunch = 64;  // one ballot finds the column; the arguments travel by value

struct ReplicaCol {
  const int64_t* urows_in;
  const float* grows;
  const int32_t* nu;
  float* block;
  float* touched;
  int64_t* urows_out;
  int64_t rows;
  int32_t cap;
  int32_t dim;
  int32_t chunks;     // per row: dim / 4 (16-byte lanes) or dim
  int32_t lpr_log2;   // lanes of a row's lane group: 2^lpr_log2 >= chunks, <= 64
  int32_t vec4;
};

struct ReplicaArgs {
  int32_t n_cols;
  int32_t tile_start[kMaxColsPerLaunch + 1];
  ReplicaCol col[kMaxColsPerLaunch];
};
static_assert(sizeof(ReplicaArgs) <= 8192, "kernarg budget");

// slice row u of column c: lane `sub` of the row's group copies chunk `sub`, lane 0 marks the row
template <typename V, int W>
__device__ inline void pack_row(const ReplicaCol& c, int64_t u, int sub) {
  const int64_t n = min(max(__builtin_nontemporal_load(c.nu), 0), c.cap);
  if (u >= n || sub >= c.chunks) return;
  const int64_t r = __builtin_nontemporal_load(c.urows_in + u);
  if ((uint64_t)r >= (uint64_t)c.rows) return;   // (-1 and rows outside the table store nothing)
  const V g = __builtin_nontemporal_load(reinterpret_cast<const V*>(c.grows + u * c.dim + sub * W));
  *reinterpret_cast<V*>(c.block + r * c.dim + sub * W) = g;
  if (sub == 0) c.touched[r] = 1.0f;
}

__global__ __launch_bounds__(kBlock) void replica_pack_kernel(const ReplicaArgs a) {
  const int b = (int)blockIdx.x;
  const int ci = column_of(a.tile_start, a.n_cols, b, lane_id());
  const ReplicaCol& c = a.col[ci];
  const int local = b - a.tile_start[ci];
  const int64_t u = (int64_t)local * (kBlock >> c.lpr_log2) + (int64_t)(threadIdx.x >> c.lpr_log2);
  const int sub = (int)threadIdx.x & ((1 << c.lpr_log2) - 1);
  if (c.vec4) {
    pack_row<f32x4, 4>(c, u, sub);
  } else {
    pack_row<float, 1>(c, u, sub);
  }
}

__global__ __launch_bounds__(kBlock) void replica_rows_kernel(const ReplicaArgs a) {
  const int b = (int)blockIdx.x;
  const int ci = column_of(a.tile_start, a.n_cols, b, lane_id());
  const ReplicaCol& c = a.col[ci];
  const int64_t r = (int64_t)(b - a.tile_start[ci]) * kBlock + (int64_t)threadIdx.x;
  if (r >= c.rows) return;
  // (the word holds the number of ranks that touched the row times the allreduce's scale, which may be negative)
  c.urows_out[r] = c.touched[r] != 0.0f ? r : (int64_t)-1;
}

// workgroups of the pack over `capacity` slice rows of one column
inline int64_t pack_groups(int64_t capacity, const RowShape& shape) {
  const int64_t rows_per_group = kBlock >> shape.lpr_log2;
  return (capacity + rows_per_group - 1) / rows_per_group;
}

// what both calls check of a column's table side
int check_table_side(const char* who, int32_t c, const hbk_replica_column_t& h) {
  HBK_REQUIRE(h.rows >= 0 && h.rows < (1ll << 31), "%s: column %d: rows %lld must be in [0, 2^31)", who, c,
              (long long)h.rows);
  HBK_REQUIRE(h.rows == 0 || (h.touched != nullptr && ((uintptr_t)h.touched & 3) == 0),
              "%s: column %d: touched must be a device fp32 [rows]", who, c);
  return HBK_OK;
}

int replica_pack(int32_t n_cols, const hbk_replica_column_t* cols, float* bucket, int64_t bucket_floats,
                 hbk_stream_t stream) {
  const char* who = "replica_grads_pack_n";
  HBK_REQUIRE(n_cols >= 0, "%s: n_cols must be >= 0, got %d", who, n_cols);
  HBK_REQUIRE(n_cols == 0 || cols != nullptr, "%s: cols is NULL", who);
  HBK_REQUIRE(bucket != nullptr && ((uintptr_t)bucket & 3) == 0, "%s: bucket must be a device fp32 buffer", who);
  HBK_REQUIRE(bucket_floats > 0 && bucket_floats < (1ll << 31),
              "%s: bucket_floats %lld must be in [1, 2^31)", who, (long long)bucket_floats);
  std::vector<RowShape> shapes((size_t)n_cols);
  std::vector<std::pair<int64_t, int64_t>> ranges;   // [first, end) in floats from the bucket
  const uintptr_t lo = (uintptr_t)bucket;
  const uintptr_t hi = lo + (uintptr_t)bucket_floats * 4;
  int64_t launch_groups = 0;   // workgroups of the launch column c belongs to
  for (int32_t c = 0; c < n_cols; ++c) {
    const hbk_replica_column_t& h = cols[c];
    if (int rc = check_table_side(who, c, h)) return rc;
    HBK_REQUIRE(h.capacity >= 0 && h.capacity < (1ll << 30), "%s: column %d: capacity %lld must be in [0, 2^30)",
                who, c, (long long)h.capacity);
    HBK_REQUIRE(h.dim >= 1, "%s: column %d: dim must be >= 1, got %d", who, c, h.dim);
    if (h.capacity > 0) {
      HBK_REQUIRE(h.unique_rows != nullptr && ((uintptr_t)h.unique_rows & 7) == 0,
                  "%s: column %d: unique_rows must be a device int64 [capacity]", who, c);
      HBK_REQUIRE(h.grad_rows != nullptr && ((uintptr_t)h.grad_rows & 3) == 0,
                  "%s: column %d: grad_rows must be a device fp32 [capacity, dim]", who, c);
      HBK_REQUIRE(h.n_unique != nullptr && ((uintptr_t)h.n_unique & 3) == 0,
                  "%s: column %d: n_unique must be a device int32 [1]", who, c);
    }
    HBK_REQUIRE(h.rows == 0 || (h.block != nullptr && ((uintptr_t)h.block & 3) == 0),
                "%s: column %d: block must be a device fp32 [rows, dim] inside the bucket", who, c);
    HBK_REQUIRE(make_rowshape(h.dim, (uintptr_t)h.grad_rows | (uintptr_t)h.block, &shapes[(size_t)c]),
                "%s: column %d: dim %d needs more than 64 lanes per row (at most 256 with dim %% 4 == 0 and "
                "16-byte aligned grad_rows / block, 64 otherwise)", who, c, h.dim);
    if (c % kMaxColsPerLaunch == 0) launch_groups = 0;
    if (h.capacity > 0 && h.rows > 0) launch_groups += pack_groups(h.capacity, shapes[(size_t)c]);
    HBK_REQUIRE(launch_groups < (1ll << 31), "%s: grid too large", who);
    if (h.rows == 0) continue;
    // (rows < 2^31 and dim <= 256: the sizes cannot overflow)
    const uintptr_t firsts[2] = {(uintptr_t)h.block, (uintptr_t)h.touched};
    const uintptr_t sizes[2] = {(uintptr_t)h.rows * (uintptr_t)h.dim * 4, (uintptr_t)h.rows * 4};
    for (int k = 0; k < 2; ++k) {
      HBK_REQUIRE(firsts[k] >= lo && firsts[k] <= hi && sizes[k] <= hi - firsts[k],
                  "%s: column %d: the bucket of %lld floats is too small: its %s leaves it", who, c,
                  (long long)bucket_floats, k == 0 ? "block" : "touched words");
      ranges.emplace_back((int64_t)((firsts[k] - lo) / 4), (int64_t)((firsts[k] - lo + sizes[k]) / 4));
    }
  }
  std::sort(ranges.begin(), ranges.end());
  for (size_t i = 1; i < ranges.size(); ++i) {
    HBK_REQUIRE(ranges[i].first >= ranges[i - 1].second,
                "%s: two blocks or touched ranges overlap inside the bucket (floats [%lld, %lld) and [%lld, %lld))",
                who, (long long)ranges[i - 1].first, (long long)ranges[i - 1].second, (long long)ranges[i].first,
                (long long)ranges[i].second);
  }
  hipStream_t s = as_stream(stream);
  HBK_HIP_OK(hipMemsetAsync(bucket, 0, (size_t)bucket_floats * 4, s));
  for (int32_t c0 = 0; c0 < n_cols; c0 += kMaxColsPerLaunch) {
    ReplicaArgs args;
    int k = 0;
    int64_t groups = 0;
    args.tile_start[0] = 0;
    for (int32_t c = c0; c < std::min(n_cols, c0 + kMaxColsPerLaunch); ++c) {
      const hbk_replica_column_t& h = cols[c];
      if (h.capacity == 0 || h.rows == 0) continue;
      const RowShape& shape = shapes[(size_t)c];
      ReplicaCol& d = args.col[k];
      d.urows_in = h.unique_rows;
      d.grows = h.grad_rows;
      d.nu = h.n_unique;
      d.block = h.block;
      d.touched = h.touched;
      d.urows_out = nullptr;
      d.rows = h.rows;
      d.cap = (int32_t)h.capacity;
      d.dim = h.dim;
      d.chunks = shape.chunks;
      d.lpr_log2 = shape.lpr_log2;
      d.vec4 = shape.vec4;
      groups += pack_groups(h.capacity, shape);   // (below 2^31: checked above)
      args.tile_start[++k] = (int32_t)groups;
    }
    if (k == 0) continue;
    args.n_cols = k;
    hipLaunchKernelGGL(replica_pack_kernel, dim3((unsigned)groups), dim3(kBlock), 0, s, args);
    HBK_HIP_OK(hipGetLastError());
  }
  return HBK_OK;
}

int replica_rows(int32_t n_cols, const hbk_replica_column_t* cols, hbk_stream_t stream) {
  const char* who = "replica_grads_rows_n";
  HBK_REQUIRE(n_cols >= 0, "%s: n_cols must be >= 0, got %d", who, n_cols);
  HBK_REQUIRE(n_cols == 0 || cols != nullptr, "%s: cols is NULL", who);
  for (int32_t c = 0; c < n_cols; ++c) {
    const hbk_replica_column_t& h = cols[c];
    if (int rc = check_table_side(who, c, h)) return rc;
    HBK_REQUIRE(h.rows == 0 || (h.urows != nullptr && ((uintptr_t)h.urows & 7) == 0),
                "%s: column %d: urows must be a device int64 [rows]", who, c);
  }
  hipStream_t s = as_stream(stream);
  for (int32_t c0 = 0; c0 < n_cols; c0 += kMaxColsPerLaunch) {
    ReplicaArgs args;
    int k = 0;
    int64_t groups = 0;
    args.tile_start[0] = 0;
    for (int32_t c = c0; c < std::min(n_cols, c0 + kMaxColsPerLaunch); ++c) {
      const hbk_replica_column_t& h = cols[c];
      if (h.rows == 0) continue;
      ReplicaCol& d = args.col[k];
      d = ReplicaCol{};
      d.touched = h.touched;
      d.urows_out = h.urows;
      d.rows = h.rows;
      groups += (h.rows + kBlock - 1) / kBlock;   // (64 columns of < 2^31 rows: below 2^29)
      args.tile_start[++k] = (int32_t)groups;
    }
    if (k == 0) continue;
    args.n_cols = k;
    hipLaunchKernelGGL(replica_rows_kernel, dim3((unsigned)groups), dim3(kBlock), 0, s, args);
    HBK_HIP_OK(hipGetLastError());
  }
  return HBK_OK;
}

}  // namespace
}  // namespace hbk

extern "C" int hbk_replica_grads_pack_n(int32_t n_cols, const hbk_replica_column_t* cols, float* bucket,
                                        int64_t bucket_floats, hbk_stream_t stream) {
  return hbk::replica_pack(n_cols, cols, bucket, bucket_floats, stream);
}

extern "C" int hbk_replica_grads_rows_n(int32_t n_cols, const hbk_replica_column_t* cols, hbk_stream_t stream) {
  return hbk::replica_rows(n_cols, cols, stream);
}
