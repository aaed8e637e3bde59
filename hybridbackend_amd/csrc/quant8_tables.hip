// 8-bit tables (include/hbk.h, "8-bit tables"): rows of int8 codes in offset binary with one fp32 scale per row,
// fp32 sums, fp32 optimizer slots.
//
//   hbk_quant8_rows_n / hbk_dequant8_rows_n   fp32 / bf16 / fp16 [rows, dim] -> the table and back; one launch for
//                                up to 64 tables.  A row is owned by LPR = pow2(dim4 / 4) adjacent lanes of 4
//                                elements each; the row's amax is a butterfly maximum over those lanes, the codes of a
//                                lane leave as ONE 4-byte store (the padding between dim and dim4 inside it), the scale
//                                word and the zeros behind it are written by the row's lanes.
//   hbk_quant8_lookup_fwd        the forward: designed around the request count.  A row of dim <= 124 codes and its
//                                scale are one 128-byte request when they share a line, and a lane asks for 4 bytes of
//                                it: ONE 4-byte load per lane whatever the row's alignment (base and pitch are multiples
//                                of 4 and nothing else), the scale word read by every lane of the row from the same
//                                line, the four codes unpacked by the byte-to-float conversions, one multiply each, and
//                                the lane's four sums leave as ONE 16-byte (fp32) or 8-byte (bf16 / fp16, rounded once)
//                                store.  Rows that cannot (dim % 4 != 0, an output block off its boundary) take one
//                                code per lane and element-sized stores.  Ids and weights are read once per wave,
//                                non-temporally, and handed to a row's lanes by shuffle; a one-id-per-segment lane
//                                issues kFwdU row loads before its first store; a ragged lane group fetches the next
//                                chunk of ids while this chunk's rows are in flight.  The sums are those of
//                                lowp_tables.hip's forward, expression for expression.
//   hbk_quant8_apply_slices_n    the split step: a walk of its own over IndexedSlices (the task scan and the
//                                grid-stride walk of sparse_apply.hip's, whose kernels stay what they are) that
//                                dequantises a row, steps it with the rule functors of sparse_rules.h -- unchanged, all
//                                five --, finds the new row's amax with a butterfly over the row's lanes in which every
//                                lane of the wave takes part (as group_sum), requantises to nearest or stochastically
//                                and writes codes and scale.  Slots are fp32 and are written as the fp32 walk writes
//                                them.
//
// Compiled as lookup_out16.hip is (no packed fp32 operations, no contraction): every product, quotient and sum is
// one scalar correctly rounded operation, so a numpy fp32 restatement reproduces every bit.
#include <string.h>

#include <algorithm>
#include <vector>

#include "common.h"
#include "lookup_common.h"
#include "lowp_elems.h"
#include "sparse_rules.h"

namespace hbk {
namespace {

constexpr float kQuantTiny = 0x1p-100f;   // a row whose amax is below this is a zero row

__device__ inline float up16(uint32_t h, int dtype) { return dtype == HBK_LOWP_BF16 ? up_bf16(h) : up_fp16(h); }

// code c of a row with `scale`: (c - 128) * scale
__device__ inline float decode(uint32_t c, float scale) { return ((float)c - 128.0f) * scale; }
// the four codes of a word (the shifts and masks become the byte-to-float conversions)
__device__ inline f32x4 decode4(uint32_t p, float scale) {
  return f32x4{decode(p & 0xffu, scale), decode((p >> 8) & 0xffu, scale), decode((p >> 16) & 0xffu, scale),
               decode(p >> 24, scale)};
}

__device__ inline float chunk_amax(float a) { return fabsf(a); }
__device__ inline float chunk_amax(f32x4 a) {
  return fmaxf(fmaxf(fmaxf(fabsf(a.x), fabsf(a.y)), fabsf(a.z)), fabsf(a.w));
}
// the maximum over a row's lane group: a butterfly (xor 1, 2, 4, ..) in which every lane of the wave takes part
__device__ inline float group_max(float m, int lpr_log2) {
  for (int o = 1; o < (1 << lpr_log2); o <<= 1) m = fmaxf(m, __shfl_xor(m, o, kWave));
  return m;
}

// how a row is rounded: the scale of its amax, and element k's code
struct RowQuant {
  float scale;
  bool zero;
  __device__ explicit RowQuant(float amax) : scale(0.0f), zero(amax < kQuantTiny) {
    if (!zero) scale = amax / 127.0f;
  }
  __device__ uint32_t code(float v, bool stochastic, uint32_t rowh, int k) const {
    if (zero) return 128u;
    const float t = v / scale;
    float q;
    if (stochastic) {
      const float u = (float)(noise_elem(rowh, k) & 0xffffu);
      q = floorf(t + u * 0x1p-16f);
    } else {
      q = rintf(t);
    }
    q = fminf(fmaxf(q, -127.0f), 127.0f);   // (a NaN lands on a bound: nothing leaves the byte)
    return (uint32_t)((int)q + 128);
  }
  __device__ uint32_t code4(f32x4 v, bool stochastic, uint32_t rowh, int k0) const {
    return code(v.x, stochastic, rowh, k0) | (code(v.y, stochastic, rowh, k0 + 1) << 8) |
           (code(v.z, stochastic, rowh, k0 + 2) << 16) | (code(v.w, stochastic, rowh, k0 + 3) << 24);
  }
};

// the rounding of a launch: step == NULL: to nearest
struct Round8 {
  const uint32_t* step;
  uint32_t seed;
};

__global__ void quant8_advance_kernel(uint32_t* step) {
  if (threadIdx.x == 0) step[0] = step[0] + 1u;
}

constexpr int kMaxCols = 64;   // columns per launch (one lane per column in the tile search / task scan)
constexpr int kBlock = 256;
constexpr int kWaves = kBlock / kWave;

inline int32_t round_up4(int32_t d) { return (d + 3) & ~3; }

// what every entry asks of a table's layout; *pitch: the pitch in bytes (0 = the default)
int check_layout(const char* who, int32_t c, const void* table, int32_t dim, int32_t pitch_in, int32_t max_dim,
                 int32_t* pitch) {
  HBK_REQUIRE(dim >= 1 && dim <= max_dim, "%s: column %d: dim must be in [1, %d], got %d", who, c, max_dim, dim);
  const int32_t dim4 = round_up4(dim);
  *pitch = pitch_in == 0 ? dim4 + 4 : pitch_in;
  HBK_REQUIRE(*pitch % 4 == 0 && *pitch >= dim4 + 4,
              "%s: column %d: pitch %d must be a multiple of 4 and >= round_up(dim, 4) + 4 = %d", who, c, *pitch,
              dim4 + 4);
  HBK_REQUIRE(((uintptr_t)table & 3) == 0, "%s: column %d: table must be 4-byte aligned", who, c);
  return HBK_OK;
}

int check_rounding(const char* who, const hbk_lowp_rounding_t* rounding, Round8* round) {
  const int32_t mode = rounding != nullptr ? rounding->mode : HBK_LOWP_ROUND_NEAREST;
  HBK_REQUIRE(mode == HBK_LOWP_ROUND_NEAREST || mode == HBK_LOWP_ROUND_STOCHASTIC,
              "%s: rounding mode must be HBK_LOWP_ROUND_NEAREST or HBK_LOWP_ROUND_STOCHASTIC, got %d", who, mode);
  const bool stochastic = mode == HBK_LOWP_ROUND_STOCHASTIC;
  HBK_REQUIRE(!stochastic || (rounding->step != nullptr && ((uintptr_t)rounding->step & 3) == 0),
              "%s: stochastic rounding needs a device uint32 [1] step counter", who);
  round->step = stochastic ? rounding->step : nullptr;
  round->seed = stochastic ? rounding->seed : 0u;
  return HBK_OK;
}

int advance(const hbk_lowp_rounding_t* rounding, const Round8& round, hipStream_t stream) {
  if (round.step != nullptr && rounding->advance != 0) {
    hipLaunchKernelGGL(quant8_advance_kernel, dim3(1), dim3(kWave), 0, stream, rounding->step);
    HBK_HIP_OK(hipGetLastError());
  }
  return HBK_OK;
}

// ---------------------------------------------------------------------------------------------------------
// quantise / dequantise whole tables

constexpr int kRowsU = 4;   // rows per lane group and wave

struct RowsCol {
  uint8_t* table;
  void* rows_f;
  int64_t rows;
  int32_t dim;
  int32_t dim4;
  int32_t pitch;
  int32_t index;     // the column's index in the CALL (the noise is keyed by it)
  uint8_t lpr_log2;
  uint8_t src_dtype;
};

struct RowsArgs {
  int32_t n_cols;
  int32_t tile_start[kMaxCols + 1];
  RowsCol col[kMaxCols];
  Round8 round;
};
static_assert(sizeof(RowsArgs) <= 16384, "kernarg budget");

// element k of source row r as fp32 (0 past dim)
__device__ inline float load_src(const RowsCol& c, int64_t r, int k) {
  if (k >= c.dim) return 0.0f;
  const int64_t at = r * c.dim + k;
  if (c.src_dtype == HBK_QUANT8_SRC_FP32) return __builtin_nontemporal_load(static_cast<const float*>(c.rows_f) + at);
  return up16(__builtin_nontemporal_load(static_cast<const uint16_t*>(c.rows_f) + at), c.src_dtype);
}

template <bool QUANT>
__global__ __launch_bounds__(kBlock) void quant8_rows_kernel(const RowsArgs a) {
  const int b = (int)blockIdx.x;
  const int lane = lane_id();
  const int ci = column_of(a.tile_start, a.n_cols, b, lane);
  const RowsCol& c = a.col[ci];
  const int64_t tile = b - a.tile_start[ci];
  const int lpr_log2 = c.lpr_log2;
  const int lpr = 1 << lpr_log2;
  const int rpi = kWave >> lpr_log2;
  const int sub = lane & (lpr - 1);
  const int grp = lane >> lpr_log2;
  const int k0 = sub * 4;
  const int64_t row0 = (tile * kWaves + (int64_t)(threadIdx.x >> 6)) * (kRowsU * rpi);
  if (row0 >= c.rows) return;
  const bool lane_on = k0 < c.dim4;
  if constexpr (QUANT) {
    const bool stochastic = a.round.step != nullptr;
    const uint32_t nbase = stochastic ? noise_base(a.round.seed, *a.round.step, c.index) : 0u;
    f32x4 v[kRowsU];
#pragma unroll
    for (int u = 0; u < kRowsU; ++u) {
      const int64_t r = row0 + u * rpi + grp;
      v[u] = zero_v<f32x4>();
      if (lane_on && r < c.rows) {
        v[u] = f32x4{load_src(c, r, k0), load_src(c, r, k0 + 1), load_src(c, r, k0 + 2), load_src(c, r, k0 + 3)};
      }
    }
#pragma unroll
    for (int u = 0; u < kRowsU; ++u) {
      const int64_t r = row0 + u * rpi + grp;
      // every lane of the wave takes part (lanes without a row pass +0)
      const RowQuant rq(group_max(chunk_amax(v[u]), lpr_log2));
      if (r >= c.rows) continue;
      uint8_t* const row = c.table + r * (int64_t)c.pitch;
      if (lane_on) {
        const uint32_t rowh = stochastic ? noise_row(nbase, r) : 0u;
        uint32_t p = 0;   // (a code past dim stays 0: the padding)
        const float e[4] = {v[u].x, v[u].y, v[u].z, v[u].w};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          if (k0 + i < c.dim) p |= rq.code(e[i], stochastic, rowh, k0 + i) << (8 * i);
        }
        *reinterpret_cast<uint32_t*>(row + k0) = p;
      }
      if (sub == 0) *reinterpret_cast<float*>(row + c.dim4) = rq.scale;
      for (int o = c.dim4 + 4 + k0; o < c.pitch; o += lpr * 4) *reinterpret_cast<uint32_t*>(row + o) = 0u;
    }
  } else {
    uint32_t p[kRowsU];
    float scale[kRowsU];
#pragma unroll
    for (int u = 0; u < kRowsU; ++u) {
      const int64_t r = row0 + u * rpi + grp;
      p[u] = 0u;
      scale[u] = 0.0f;
      if (lane_on && r < c.rows) {
        const uint8_t* const row = c.table + r * (int64_t)c.pitch;
        p[u] = *reinterpret_cast<const uint32_t*>(row + k0);
        scale[u] = *reinterpret_cast<const float*>(row + c.dim4);
      }
    }
#pragma unroll
    for (int u = 0; u < kRowsU; ++u) {
      const int64_t r = row0 + u * rpi + grp;
      if (!lane_on || r >= c.rows) continue;
      const f32x4 x = decode4(p[u], scale[u]);
      const float e[4] = {x.x, x.y, x.z, x.w};
      float* const out = static_cast<float*>(c.rows_f) + r * c.dim;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        if (k0 + i < c.dim) __builtin_nontemporal_store(e[i], out + k0 + i);
      }
    }
  }
}

template <bool QUANT>
int quant8_rows(const char* kWho, int32_t n_cols, const hbk_quant8_rows_column_t* cols,
                const hbk_lowp_rounding_t* rounding, hbk_stream_t stream_) {
  HBK_REQUIRE(n_cols >= 0, "%s: n_cols must be >= 0, got %d", kWho, n_cols);
  HBK_REQUIRE(n_cols == 0 || cols != nullptr, "%s: cols is NULL", kWho);
  Round8 round = {nullptr, 0u};
  int rc = QUANT ? check_rounding(kWho, rounding, &round) : HBK_OK;
  if (rc != HBK_OK) return rc;
  std::vector<int32_t> pitch((size_t)std::max(n_cols, 1));
  for (int32_t c = 0; c < n_cols; ++c) {
    const hbk_quant8_rows_column_t& h = cols[c];
    if ((rc = check_layout(kWho, c, h.table, h.dim, h.pitch, 256, &pitch[(size_t)c])) != HBK_OK) return rc;
    HBK_REQUIRE(h.rows >= 0 && h.rows < (1ll << 31), "%s: column %d: rows must be in [0, 2^31), got %lld", kWho, c,
                (long long)h.rows);
    HBK_REQUIRE(h.reserved == 0, "%s: column %d: the reserved word must be 0, got %d", kWho, c, h.reserved);
    const bool f32 = !QUANT || h.src_dtype == HBK_QUANT8_SRC_FP32;
    HBK_REQUIRE(f32 || h.src_dtype == HBK_LOWP_BF16 || h.src_dtype == HBK_LOWP_FP16,
                "%s: column %d: src_dtype must be HBK_QUANT8_SRC_FP32, HBK_LOWP_BF16 or HBK_LOWP_FP16, got %d", kWho, c,
                h.src_dtype);
    HBK_REQUIRE(QUANT || h.src_dtype == 0, "%s: column %d: src_dtype must be 0, got %d", kWho, c, h.src_dtype);
    HBK_REQUIRE(((uintptr_t)h.rows_f & (f32 ? 3 : 1)) == 0, "%s: column %d: rows_f must be aligned to its element",
                kWho, c);
    HBK_REQUIRE(h.rows == 0 || (h.table != nullptr && h.rows_f != nullptr), "%s: column %d: table or rows_f is NULL",
                kWho, c);
  }
  hipStream_t stream = as_stream(stream_);
  for (int32_t c0 = 0; c0 < n_cols; c0 += kMaxCols) {
    RowsArgs args;
    int32_t k = 0;
    int64_t tiles = 0;
    args.tile_start[0] = 0;
    args.round = round;
    for (int32_t c = c0; c < std::min(n_cols, c0 + kMaxCols); ++c) {
      const hbk_quant8_rows_column_t& h = cols[c];
      if (h.rows == 0) continue;
      RowsCol& d = args.col[k];
      d.table = static_cast<uint8_t*>(h.table);
      d.rows_f = h.rows_f;
      d.rows = h.rows;
      d.dim = h.dim;
      d.dim4 = round_up4(h.dim);
      d.pitch = pitch[(size_t)c];
      d.index = c;
      d.lpr_log2 = (uint8_t)ceil_log2_u32((uint32_t)(d.dim4 / 4));
      d.src_dtype = (uint8_t)h.src_dtype;
      const int64_t per_block = (int64_t)kWaves * (kWave >> d.lpr_log2) * kRowsU;
      tiles += (h.rows + per_block - 1) / per_block;
      HBK_REQUIRE(tiles < (1ll << 31), "%s: grid too large", kWho);
      args.tile_start[++k] = (int32_t)tiles;
    }
    if (k == 0) continue;
    args.n_cols = k;
    hipLaunchKernelGGL(quant8_rows_kernel<QUANT>, dim3((unsigned)tiles), dim3(kBlock), 0, stream, args);
    HBK_HIP_OK(hipGetLastError());
  }
  return QUANT ? advance(rounding, round, stream) : HBK_OK;
}

// ---------------------------------------------------------------------------------------------------------
// forward

constexpr int kFwdU = 4;          // independent row loads per lane (one id per segment)
constexpr int kFwdSegIters = 4;   // segments per lane group and wave (ragged)

struct FwdCol {
  const uint8_t* table;
  const void* ids;
  const int32_t* splits;
  const float* weights;
  void* out;
  int64_t n_seg;
  IdMap map;
  int32_t dim4;         // byte offset of the scale word
  int32_t pitch;        // bytes between rows
  int32_t chunks;       // lane chunks per row
  int32_t out_stride;   // elements between output rows
  uint8_t lpr_log2;
  uint8_t ids64;
  uint8_t combiner;
  uint8_t out_bf16;
};

struct FwdArgs {
  int32_t n_cols;
  int32_t tile_start[kMaxCols + 1];
  FwdCol col[kMaxCols];
};
static_assert(sizeof(FwdArgs) <= 16384, "kernarg budget");

// lane chunk `sub` of row r, decoded: W = 4: one 4-byte load of codes, W = 1: one byte; the scale word beside them
template <int W>
__device__ inline void load_codes(const FwdCol& c, uint64_t r, int sub, float (&v)[W]) {
  const uint8_t* const row = c.table + r * (uint64_t)(uint32_t)c.pitch;
  const float scale = *reinterpret_cast<const float*>(row + c.dim4);
  if constexpr (W == 4) {
    const f32x4 x = decode4(*reinterpret_cast<const uint32_t*>(row + sub * 4), scale);
    v[0] = x.x;
    v[1] = x.y;
    v[2] = x.z;
    v[3] = x.w;
  } else {
    v[0] = decode(row[sub], scale);
  }
}

__device__ inline uint32_t round16(float x, bool bf16) { return bf16 ? bf16_nearest(x) : fp16_nearest(x); }

// W sums stored at element `off` as one store, streamed: O16 false: fp32 (W = 4: 16 bytes), true: rounded once to
// bf16 / fp16 (W = 4: 8 bytes, pairs packed in registers); W = 1: one element, no neighbouring byte touched
template <int W, bool O16>
__device__ inline void store_sums(void* out, int64_t off, bool bf16, const float (&v)[W]) {
  if constexpr (!O16) {
    float* const o = static_cast<float*>(out) + off;
    if constexpr (W == 1) {
      __builtin_nontemporal_store(v[0], o);
    } else {
      const f32x4 x = {v[0], v[1], v[2], v[3]};
      __builtin_nontemporal_store(x, reinterpret_cast<f32x4*>(o));
    }
  } else {
    uint16_t* const o = static_cast<uint16_t*>(out) + off;
    if constexpr (W == 1) {
      __builtin_nontemporal_store((uint16_t)round16(v[0], bf16), o);
    } else {
      u32x2 p;
#pragma unroll
      for (int i = 0; i < 2; ++i) p[i] = round16(v[2 * i], bf16) | (round16(v[2 * i + 1], bf16) << 16);
      __builtin_nontemporal_store(p, reinterpret_cast<u32x2*>(o));
    }
  }
}

// one id per segment: out[s, :] = decode(table[row(ids[s]), :]), times the segment's weight when weighted
// (lowp_gather_rows of lowp_tables.hip: the same expressions in the same order)
template <int W, bool O16>
__device__ inline void q8_gather_rows(const FwdCol& c, int64_t wave_row0) {
  const int lane = lane_id();
  const int lpr_log2 = c.lpr_log2;
  const int rpi = kWave >> lpr_log2;   // rows per wave instruction
  const int sub = lane & ((1 << lpr_log2) - 1);
  const int grp = lane >> lpr_log2;
  const int64_t n_seg = c.n_seg;
  const bool wgt = c.weights != nullptr;   // (uniform: one column per wave)
  const bool obf16 = c.out_bf16 != 0;

  // ids: slot q (0 <= q < U * rpi) lives in register q >> 6 of lane q & 63
  uint64_t rowreg[kFwdU];
  float wreg[kFwdU];
  const int n_slots = kFwdU * rpi;
#pragma unroll
  for (int k = 0; k < kFwdU; ++k) {
    rowreg[k] = kNoRow;
    wreg[k] = 0.f;
    const int q = k * kWave + lane;
    const int64_t s = wave_row0 + q;
    if (q < n_slots && s < n_seg) {
      rowreg[k] = id_to_row(c.map, load_id(c.ids, c.ids64, s));
      if (wgt) wreg[k] = __builtin_nontemporal_load(c.weights + s);
    }
  }
  float v[kFwdU][W];
  const bool live = sub < c.chunks;
  // every row load of the lane is issued before the first store
#pragma unroll
  for (int u = 0; u < kFwdU; ++u) {
    const int q0 = u * rpi;   // a multiple of rpi (a power of two <= 64): q0 >> 6 is uniform
    const int k = q0 >> 6;
    uint64_t src = rowreg[0];
#pragma unroll
    for (int kk = 1; kk < kFwdU; ++kk) src = (k == kk) ? rowreg[kk] : src;
    const uint64_t r = shfl_u64(src, (q0 & (kWave - 1)) + grp);
#pragma unroll
    for (int i = 0; i < W; ++i) v[u][i] = 0.f;
    if (live && r != kNoRow) load_codes<W>(c, r, sub, v[u]);
    if (wgt) {
      float w = wreg[0];
#pragma unroll
      for (int kk = 1; kk < kFwdU; ++kk) w = (k == kk) ? wreg[kk] : w;
      w = __shfl(w, (q0 & (kWave - 1)) + grp, kWave);
      const float div = c.combiner == HBK_COMBINER_MEAN    ? w
                        : c.combiner == HBK_COMBINER_SQRTN ? sqrtf(w * w)
                                                           : 1.f;
      if (r != kNoRow && div != 0.f) {
#pragma unroll
        for (int i = 0; i < W; ++i) {
          v[u][i] = v[u][i] * w;
          if (c.combiner != HBK_COMBINER_SUM) v[u][i] = v[u][i] / div;
        }
      } else {
#pragma unroll
        for (int i = 0; i < W; ++i) v[u][i] = 0.f;
      }
    }
  }
#pragma unroll
  for (int u = 0; u < kFwdU; ++u) {
    const int64_t s = wave_row0 + u * rpi + grp;
    if (live && s < n_seg) store_sums<W, O16>(c.out, s * (int64_t)c.out_stride + (int64_t)sub * W, obf16, v[u]);
  }
}

// ragged segments: out[s, :] = combine_j decode(table[row(ids[j]), :]) in id order, from +0 (lowp_combine_segments
// of lowp_tables.hip: the same expressions in the same order).  Lane `sub` of a group owns id j0 + sub of the
// group's segment; the next chunk of ids is fetched while this chunk's rows are in flight.
template <int W, bool O16>
__device__ inline void q8_combine_segments(const FwdCol& c, int64_t wave_seg0) {
  const int lane = lane_id();
  const int lpr_log2 = c.lpr_log2;
  const int lpr = 1 << lpr_log2;
  const int rpi = kWave >> lpr_log2;
  const int sub = lane & (lpr - 1);
  const int grp = lane >> lpr_log2;
  const int grp_lane0 = grp << lpr_log2;
  const int64_t n_seg = c.n_seg;
  const bool live = sub < c.chunks;
  const bool wgt = c.weights != nullptr;
  const bool obf16 = c.out_bf16 != 0;

  for (int it = 0; it < kFwdSegIters; ++it) {
    const int64_t s = wave_seg0 + (int64_t)it * rpi + grp;
    int32_t beg = 0, end = 0;
    if (s < n_seg) {
      beg = c.splits[s];
      end = c.splits[s + 1];
    }
    float acc[W];
#pragma unroll
    for (int i = 0; i < W; ++i) acc[i] = 0.f;
    float wsum = 0.f;   // weighted: W_s or Q_s
    int32_t j0 = beg;
    uint64_t myrow = kNoRow;
    float myw = 0.f;
    if (j0 + sub < end) {
      myrow = id_to_row(c.map, load_id(c.ids, c.ids64, j0 + sub));
      if (wgt) myw = __builtin_nontemporal_load(c.weights + j0 + sub);
    }
    while (__any(j0 < end)) {
      uint64_t nextrow = kNoRow;
      float nextw = 0.f;
      const int32_t j1 = j0 + lpr;
      if (j1 + sub < end) {
        nextrow = id_to_row(c.map, load_id(c.ids, c.ids64, j1 + sub));
        if (wgt) nextw = __builtin_nontemporal_load(c.weights + j1 + sub);
      }
      const int32_t cnt = end - j0;   // ids of this group still to add (may be <= 0)
      for (int t0 = 0; t0 < lpr; t0 += 4) {
        float v[4][W];
        bool p[4];
        float w[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          const int tt = t0 + t;
          const uint64_t r = shfl_u64(myrow, grp_lane0 + (tt & (lpr - 1)));
          p[t] = tt < lpr && tt < cnt;
          w[t] = 0.f;
          if (wgt) {
            w[t] = __shfl(myw, grp_lane0 + (tt & (lpr - 1)), kWave);
            p[t] = p[t] && r != kNoRow;   // an invalid row adds neither term nor weight
          }
#pragma unroll
          for (int i = 0; i < W; ++i) v[t][i] = 0.f;
          if (p[t] && live && r != kNoRow) load_codes<W>(c, r, sub, v[t]);
        }
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          if (!p[t]) continue;
          if (wgt) {
#pragma unroll
            for (int i = 0; i < W; ++i) acc[i] = acc[i] + v[t][i] * w[t];
            wsum = wsum + (c.combiner == HBK_COMBINER_SQRTN ? w[t] * w[t] : w[t]);
          } else {
#pragma unroll
            for (int i = 0; i < W; ++i) acc[i] = acc[i] + v[t][i];
          }
        }
      }
      myrow = nextrow;
      myw = nextw;
      j0 = j1;
    }
    const int32_t n = end - beg;
    if (wgt) {
      if (c.combiner != HBK_COMBINER_SUM) {
        const float div = c.combiner == HBK_COMBINER_MEAN ? wsum : sqrtf(wsum);
#pragma unroll
        for (int i = 0; i < W; ++i) acc[i] = div != 0.f ? acc[i] / div : 0.f;
      }
    } else if (n > 0 && c.combiner == HBK_COMBINER_MEAN) {
      const float fn = (float)n;
#pragma unroll
      for (int i = 0; i < W; ++i) acc[i] = acc[i] / fn;
    } else if (n > 0 && c.combiner == HBK_COMBINER_SQRTN) {
      const float fn = sqrtf((float)n);
#pragma unroll
      for (int i = 0; i < W; ++i) acc[i] = acc[i] / fn;
    }
    if (live && s < n_seg) store_sums<W, O16>(c.out, s * (int64_t)c.out_stride + (int64_t)sub * W, obf16, acc);
  }
}

// one kernel per kind (one id per segment: CSR = false; ragged), lane width and output size
template <bool CSR, int W, bool O16>
__global__ __launch_bounds__(kBlock) void quant8_lookup_fwd_kernel(const FwdArgs a) {
  const int b = (int)blockIdx.x;
  const int ci = column_of(a.tile_start, a.n_cols, b, lane_id());
  const int64_t tile = b - a.tile_start[ci];
  const FwdCol& c = a.col[ci];
  const int wave = (int)(threadIdx.x >> 6);
  const int rpi = kWave >> c.lpr_log2;
  const int64_t first = (tile * kWaves + wave) * (int64_t)((CSR ? kFwdSegIters : kFwdU) * rpi);
  if (first >= c.n_seg) return;
  if constexpr (CSR) {
    q8_combine_segments<W, O16>(c, first);
  } else {
    q8_gather_rows<W, O16>(c, first);
  }
}

template <bool CSR, bool O16>
void launch_fwd(int w, const FwdArgs& a, unsigned tiles, hipStream_t stream) {
  if (w == 4) {
    hipLaunchKernelGGL((quant8_lookup_fwd_kernel<CSR, 4, O16>), dim3(tiles), dim3(kBlock), 0, stream, a);
  } else {
    hipLaunchKernelGGL((quant8_lookup_fwd_kernel<CSR, 1, O16>), dim3(tiles), dim3(kBlock), 0, stream, a);
  }
}

int quant8_lookup_fwd(int32_t n_cols, const hbk_quant8_lookup_column_t* cols, hbk_stream_t stream_) {
  static const char* kWho = "quant8_lookup_fwd";
  HBK_REQUIRE(n_cols >= 0, "%s: n_cols must be >= 0, got %d", kWho, n_cols);
  HBK_REQUIRE(n_cols == 0 || cols != nullptr, "%s: cols is NULL", kWho);
  // every column is checked and classified before the first launch: codes per lane (1, 4) and kind
  struct Classified {
    int w;   // 0: nothing to do (no segments)
    int pitch;
  };
  std::vector<Classified> cls((size_t)std::max(n_cols, 1));
  for (int32_t c = 0; c < n_cols; ++c) {
    const hbk_quant8_lookup_column_t& h = cols[c];
    const int rc = check_layout(kWho, c, h.table, h.dim, h.pitch, 256, &cls[(size_t)c].pitch);
    if (rc != HBK_OK) return rc;
    const bool o16 = h.out_dtype != HBK_QUANT8_OUT_FP32;
    HBK_REQUIRE(!o16 || h.out_dtype == HBK_LOWP_BF16 || h.out_dtype == HBK_LOWP_FP16,
                "%s: column %d: out_dtype must be HBK_QUANT8_OUT_FP32, HBK_LOWP_BF16 or HBK_LOWP_FP16, got %d", kWho, c,
                h.out_dtype);
    HBK_REQUIRE(h.rows >= 0 && h.n_ids >= 0 && h.n_segments >= 0, "%s: column %d: negative size", kWho, c);
    HBK_REQUIRE(h.ids_dtype == HBK_INT32 || h.ids_dtype == HBK_INT64, "%s: column %d: ids must be int32 or int64",
                kWho, c);
    HBK_REQUIRE(h.bucket >= 0, "%s: column %d: bucket must be >= 0", kWho, c);
    HBK_REQUIRE(h.divisor >= 1, "%s: column %d: divisor must be >= 1", kWho, c);
    HBK_REQUIRE(h.combiner >= HBK_COMBINER_SUM && h.combiner <= HBK_COMBINER_SQRTN,
                "%s: column %d: unknown combiner %d", kWho, c, h.combiner);
    HBK_REQUIRE(h.chunk_elems == 0 || h.chunk_elems == 4, "%s: column %d: chunk_elems must be 0 or 4, got %d", kWho, c,
                h.chunk_elems);
    HBK_REQUIRE(h.row_splits != nullptr || h.n_segments == h.n_ids,
                "%s: column %d: n_segments (%lld) must equal n_ids (%lld) when row_splits is NULL", kWho, c,
                (long long)h.n_segments, (long long)h.n_ids);
    HBK_REQUIRE(h.n_ids < (1ll << 31) && h.n_segments < (1ll << 31),
                "%s: column %d: more than 2^31-1 ids/segments", kWho, c);
    HBK_REQUIRE(h.out_stride == 0 || h.out_stride >= h.dim, "%s: column %d: out_stride %d is smaller than dim %d",
                kWho, c, h.out_stride, h.dim);
    const int esize = o16 ? 2 : 4;
    HBK_REQUIRE(((uintptr_t)h.out & (uintptr_t)(esize - 1)) == 0, "%s: column %d: out must be aligned to its element",
                kWho, c);
    cls[(size_t)c].w = 0;
    if (h.n_segments == 0) continue;
    HBK_REQUIRE(h.table != nullptr || h.rows == 0, "%s: column %d: table is NULL", kWho, c);
    HBK_REQUIRE(h.out != nullptr, "%s: column %d: out is NULL", kWho, c);
    HBK_REQUIRE(h.ids != nullptr || h.n_ids == 0, "%s: column %d: ids is NULL", kWho, c);
    // the store side decides: one 16-byte (fp32) or 8-byte (16-bit) store per lane needs out and its pitch there
    const uintptr_t out_bits = (uintptr_t)h.out | ((uintptr_t)(uint32_t)h.out_stride * (uintptr_t)esize);
    const int w = h.dim % 4 == 0 && out_bits % (uintptr_t)(4 * esize) == 0 ? 4 : 1;
    HBK_REQUIRE(h.dim <= (w == 4 ? 256 : 64),
                "%s: column %d: dim %d: at most 256 when dim %% 4 == 0 and out and its stride are 16-byte (fp32) or "
                "8-byte (16-bit) aligned, 64 otherwise", kWho, c, h.dim);
    cls[(size_t)c].w = w;
  }
  hipStream_t stream = as_stream(stream_);
  for (int kind = 0; kind < 8; ++kind) {
    const bool csr = (kind & 1) != 0, o16 = (kind & 2) != 0;
    const int w = (kind & 4) != 0 ? 1 : 4;
    int32_t c0 = 0;
    while (c0 < n_cols) {
      FwdArgs args;
      int32_t k = 0;
      int64_t tiles = 0;
      args.tile_start[0] = 0;
      for (; c0 < n_cols && k < kMaxCols; ++c0) {
        const hbk_quant8_lookup_column_t& h = cols[c0];
        if (cls[(size_t)c0].w != w || (h.row_splits != nullptr) != csr ||
            (h.out_dtype != HBK_QUANT8_OUT_FP32) != o16) {
          continue;
        }
        FwdCol& d = args.col[k];
        d.table = static_cast<const uint8_t*>(h.table);
        d.ids = h.ids;
        d.splits = h.row_splits;
        d.weights = h.id_weights;
        d.out = h.out;
        d.n_seg = h.n_segments;
        d.map = make_idmap(h.bucket, h.divisor, h.rows);
        d.dim4 = round_up4(h.dim);
        d.pitch = cls[(size_t)c0].pitch;
        d.chunks = h.dim / w;
        d.out_stride = h.out_stride > 0 ? h.out_stride : h.dim;
        d.lpr_log2 = (uint8_t)ceil_log2_u32((uint32_t)d.chunks);
        d.ids64 = h.ids_dtype == HBK_INT64;
        d.combiner = (uint8_t)h.combiner;
        d.out_bf16 = h.out_dtype == HBK_LOWP_BF16;
        const int64_t rpi = kWave >> d.lpr_log2;
        const int64_t per_block = kWaves * rpi * (csr ? kFwdSegIters : kFwdU);
        tiles += (h.n_segments + per_block - 1) / per_block;
        HBK_REQUIRE(tiles < (1ll << 31), "%s: grid too large", kWho);
        args.tile_start[++k] = (int32_t)tiles;
      }
      if (k == 0) continue;
      args.n_cols = k;
      if (csr) {
        o16 ? launch_fwd<true, true>(w, args, (unsigned)tiles, stream)
            : launch_fwd<true, false>(w, args, (unsigned)tiles, stream);
      } else {
        o16 ? launch_fwd<false, true>(w, args, (unsigned)tiles, stream)
            : launch_fwd<false, false>(w, args, (unsigned)tiles, stream);
      }
      HBK_HIP_OK(hipGetLastError());
    }
  }
  return HBK_OK;
}

// ---------------------------------------------------------------------------------------------------------
// the split step

constexpr int kStepItems = 4;       // rows per lane group in flight
constexpr int kStepBlocksPerCU = 8;

struct StepCol {
  uint8_t* w;
  float* s0;
  float* s1;
  const int64_t* urows;
  const float* grows;   // [cap, dim] contiguous
  const int32_t* nu;
  int64_t rows;
  int32_t cap;
  int32_t dim;
  int32_t dim4;
  int32_t pitch;
  int32_t index;        // the column's index in the CALL (the noise is keyed by it)
  uint8_t lpr_log2;
  uint8_t vec4;
};

template <typename P>
struct StepArgs {
  StepCol c[kMaxCols];
  P p;
  Round8 round;
  int32_t n_cols;
};

__device__ inline f32x4 load_row_chunk8(const uint8_t* row, int sub, float scale, f32x4) {
  return decode4(*reinterpret_cast<const uint32_t*>(row + sub * 4), scale);
}
__device__ inline float load_row_chunk8(const uint8_t* row, int sub, float scale, float) {
  return decode(row[sub], scale);
}
__device__ inline void store_row_chunk8(uint8_t* row, int sub, f32x4 x, const RowQuant& rq, bool stochastic,
                                        uint32_t rowh) {
  *reinterpret_cast<uint32_t*>(row + sub * 4) = rq.code4(x, stochastic, rowh, sub * 4);
}
__device__ inline void store_row_chunk8(uint8_t* row, int sub, float x, const RowQuant& rq, bool stochastic,
                                        uint32_t rowh) {
  row[sub] = (uint8_t)rq.code(x, stochastic, rowh, sub);
}

// one task: rows base + k * groups + grp (k < kStepItems) of column c; W elements per lane.  A lane issues the
// codes / scale / slot / gradient loads of all its rows before any arithmetic; lanes without a row (past n, an
// entry outside the table, past dim) pass +0 to the butterflies, in which every lane of the wave takes part.
template <typename V, int W, typename Rule>
__device__ inline void q8_step_task(const StepCol& c, int64_t base, int64_t n, const Rule& rule, bool stochastic,
                                    uint32_t nbase) {
  const int lane = lane_id();
  const int lpr = c.lpr_log2;
  const int grp = lane >> lpr;
  const int sub = lane & ((1 << lpr) - 1);
  const int groups = kWave >> lpr;
  const bool lane_on = sub * W < c.dim;
  int64_t r[kStepItems];
  bool on[kStepItems];
#pragma unroll
  for (int k = 0; k < kStepItems; ++k) {
    const int64_t u = base + (int64_t)k * groups + grp;
    on[k] = lane_on && u < n;
    r[k] = on[k] ? __builtin_nontemporal_load(c.urows + u) : 0;
    on[k] = on[k] && (uint64_t)r[k] < (uint64_t)c.rows;
  }
  V w[kStepItems], s0[kStepItems], s1[kStepItems], g[kStepItems];
  float acc[kStepItems];
#pragma unroll
  for (int k = 0; k < kStepItems; ++k) {
    w[k] = s0[k] = s1[k] = g[k] = zero_v<V>();
    acc[k] = 0.0f;
    if (!on[k]) continue;
    const int64_t u = base + (int64_t)k * groups + grp;
    const uint8_t* const row = c.w + r[k] * (int64_t)c.pitch;
    const int64_t off = r[k] * c.dim + sub * W;
    w[k] = load_row_chunk8(row, sub, *reinterpret_cast<const float*>(row + c.dim4), V());
    if constexpr (Rule::kSlots >= 1) s0[k] = *reinterpret_cast<const V*>(c.s0 + off);
    if constexpr (Rule::kSlots >= 2) s1[k] = *reinterpret_cast<const V*>(c.s1 + off);
    if constexpr (Rule::kRowwise) acc[k] = c.s0[r[k]];
    g[k] = __builtin_nontemporal_load(reinterpret_cast<const V*>(c.grows + u * c.dim + sub * W));
  }
  float sq[kStepItems];
  if constexpr (Rule::kRowwise) {
#pragma unroll
    for (int k = 0; k < kStepItems; ++k) sq[k] = group_sum(chunk_sum(g[k] * g[k]), lpr);
  }
  V x[kStepItems];
#pragma unroll
  for (int k = 0; k < kStepItems; ++k) {
    x[k] = zero_v<V>();
    if (!on[k]) continue;
    if constexpr (Rule::kRowwise) {
      float rate;
      const float na = rule.row(acc[k], sq[k], (float)c.dim, &rate);
      if (sub == 0) c.s0[r[k]] = na;
      x[k] = w[k] - rate * g[k];
    } else {
      const int64_t off = r[k] * c.dim + sub * W;
      const Stepped<V> o = rule(w[k], s0[k], s1[k], g[k]);
      if constexpr (Rule::kSlots >= 1) *reinterpret_cast<V*>(c.s0 + off) = o.s0;
      if constexpr (Rule::kSlots >= 2) *reinterpret_cast<V*>(c.s1 + off) = o.s1;
      x[k] = o.w;
    }
  }
#pragma unroll
  for (int k = 0; k < kStepItems; ++k) {
    const RowQuant rq(group_max(chunk_amax(x[k]), lpr));
    if (!on[k]) continue;
    uint8_t* const row = c.w + r[k] * (int64_t)c.pitch;
    store_row_chunk8(row, sub, x[k], rq, stochastic, stochastic ? noise_row(nbase, r[k]) : 0u);
    if (sub == 0) *reinterpret_cast<float*>(row + c.dim4) = rq.scale;
  }
}

// the body of every step kernel: wave 0 reads the columns' n_unique and scans their task counts into LDS, the
// rule's setup, the barrier, then the tasks grid-stride (the grid comes from the host-known capacities only)
template <typename Rule>
__global__ __launch_bounds__(kBlock) void quant8_apply_kernel(StepArgs<typename Rule::Params> a) {
  __shared__ int64_t s_end[kMaxCols];   // inclusive prefix of the columns' task counts
  __shared__ int64_t s_n[kMaxCols];     // their n_unique (clamped to the capacity)
  if (threadIdx.x < kWave) {
    const int lane = (int)threadIdx.x;
    int64_t tasks = 0;
    if (lane < a.n_cols) {
      const StepCol& c = a.c[lane];
      const int64_t n = min(max(__builtin_nontemporal_load(c.nu), 0), c.cap);
      const int64_t rpt = (int64_t)(kWave >> c.lpr_log2) * kStepItems;
      tasks = (n + rpt - 1) / rpt;
      s_n[lane] = n;
    }
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {
      const int64_t t = __shfl_up(tasks, d, kWave);
      if (lane >= d) tasks += t;
    }
    if (lane < a.n_cols) s_end[lane] = tasks;
    if (lane == 0) Rule::setup(a.p);
  }
  __syncthreads();
  const typename Rule::State st = Rule::state();
  // the step word is read behind the barrier and so before the advance launch -- behind this one in stream
  // order -- writes it
  const bool stochastic = a.round.step != nullptr;
  const uint32_t step = stochastic ? *a.round.step : 0u;
  const int64_t total = s_end[a.n_cols - 1];
  int ci = 0;
  for (int64_t t = (int64_t)blockIdx.x * kWaves + threadIdx.x / kWave; t < total;
       t += (int64_t)gridDim.x * kWaves) {
    while (s_end[ci] <= t) ++ci;   // (t only grows: the column only moves forward)
    const StepCol& col = a.c[ci];
    const int64_t t0 = ci == 0 ? 0 : s_end[ci - 1];
    const int64_t base = (t - t0) * ((int64_t)(kWave >> col.lpr_log2) * kStepItems);
    const uint32_t nbase = stochastic ? noise_base(a.round.seed, step, col.index) : 0u;
    if (col.vec4) {
      q8_step_task<f32x4, 4, Rule>(col, base, s_n[ci], Rule(a.p, st), stochastic, nbase);
    } else {
      q8_step_task<float, 1, Rule>(col, base, s_n[ci], Rule(a.p, st), stochastic, nbase);
    }
  }
}

// TF's _finish: beta1^t, beta2^t -> beta1^(t+1), beta2^(t+1), one fp32 product each
__global__ void quant8_adam_finish_kernel(float* powers, float beta1, float beta2) {
  if (threadIdx.x == 0) {
    powers[0] = powers[0] * beta1;
    powers[1] = powers[1] * beta2;
  }
}

// every check of the columns for a rule with n_slots table-shaped slots (or the row-wise word in slot0), then one
// launch per kMaxCols columns
template <typename Rule>
int step_columns(const char* who, int32_t n_cols, const hbk_quant8_slices_column_t* cols, const char* n0,
                 const char* n1, float* const* slot0, float* const* slot1, const typename Rule::Params& p,
                 const Round8& round, hipStream_t stream) {
  constexpr int n_slots = Rule::kSlots;
  constexpr bool rowwise = Rule::kRowwise;
  HBK_REQUIRE(n_cols == 0 || (n_slots < 1 && !rowwise) || slot0 != nullptr, "%s: the %s array (slot0) is NULL", who,
              n0);
  HBK_REQUIRE(n_cols == 0 || n_slots < 2 || slot1 != nullptr, "%s: the %s array (slot1) is NULL", who, n1);
  std::vector<StepCol> out((size_t)std::max(n_cols, 1));
  std::vector<uintptr_t> seen;
  seen.reserve((size_t)n_cols * 3);
  for (int32_t c = 0; c < n_cols; ++c) {
    const hbk_quant8_slices_column_t& s = cols[c];
    StepCol& d = out[(size_t)c];
    memset(&d, 0, sizeof(d));
    const int rc = check_layout(who, c, s.table, s.dim, s.pitch, 256, &d.pitch);
    if (rc != HBK_OK) return rc;
    HBK_REQUIRE(s.capacity >= 0 && s.capacity < (1ll << 30), "%s: column %d: capacity %lld must be in [0, 2^30)", who,
                c, (long long)s.capacity);
    HBK_REQUIRE(s.rows >= 0, "%s: column %d: rows must be >= 0, got %lld", who, c, (long long)s.rows);
    float* const a0 = (n_slots >= 1 || rowwise) ? slot0[c] : nullptr;
    float* const a1 = n_slots >= 2 ? slot1[c] : nullptr;
    HBK_REQUIRE(!(n_slots >= 1 || rowwise) || (a0 != nullptr && ((uintptr_t)a0 & 3) == 0),
                "%s: column %d: %s must be a device fp32 buffer", who, c, n0);
    HBK_REQUIRE(n_slots < 2 || (a1 != nullptr && ((uintptr_t)a1 & 3) == 0),
                "%s: column %d: %s must be a device fp32 buffer", who, c, n1);
    if (s.capacity > 0) {
      HBK_REQUIRE(s.table != nullptr, "%s: column %d: table is NULL", who, c);
      HBK_REQUIRE(s.unique_rows != nullptr && ((uintptr_t)s.unique_rows & 7) == 0,
                  "%s: column %d: unique_rows must be a device int64 [capacity]", who, c);
      HBK_REQUIRE(s.grad_rows != nullptr && ((uintptr_t)s.grad_rows & 3) == 0,
                  "%s: column %d: grad_rows must be a device fp32 [capacity, dim]", who, c);
      HBK_REQUIRE(s.n_unique != nullptr && ((uintptr_t)s.n_unique & 3) == 0,
                  "%s: column %d: n_unique must be a device int32 [1]", who, c);
      // the row shape of the fp32 entry over the fp32 buffers (the table's words are 4-byte aligned at any row)
      RowShape shape;
      const uintptr_t bits = (uintptr_t)s.grad_rows | (n_slots >= 1 ? (uintptr_t)a0 : 0) | (uintptr_t)a1;
      HBK_REQUIRE(make_rowshape(s.dim, bits, &shape),
                  "%s: column %d: dim %d: at most 256 when dim %% 4 == 0 and the slots and grad_rows are 16-byte "
                  "aligned, 64 otherwise", who, c, s.dim);
      d.lpr_log2 = shape.lpr_log2;
      d.vec4 = shape.vec4;
    }
    d.w = static_cast<uint8_t*>(s.table);
    d.s0 = a0;
    d.s1 = a1;
    d.urows = s.unique_rows;
    d.grows = s.grad_rows;
    d.nu = s.n_unique;
    d.rows = s.rows;
    d.cap = (int32_t)s.capacity;
    d.dim = s.dim;
    d.dim4 = round_up4(s.dim);
    d.index = c;
    if (s.table != nullptr) seen.push_back((uintptr_t)s.table);
    if (a0 != nullptr) seen.push_back((uintptr_t)a0);
    if (a1 != nullptr) seen.push_back((uintptr_t)a1);
  }
  std::sort(seen.begin(), seen.end());
  HBK_REQUIRE(std::adjacent_find(seen.begin(), seen.end()) == seen.end(),
              "%s: two columns name the same table or slot (a row stepped twice in one call would race)", who);
  for (int32_t c0 = 0; c0 < n_cols; c0 += kMaxCols) {
    StepArgs<typename Rule::Params> a;
    memset(&a, 0, sizeof(a));
    int64_t tasks = 0;
    int k = 0;
    for (int32_t c = c0; c < std::min(n_cols, c0 + kMaxCols); ++c) {
      const StepCol& d = out[(size_t)c];
      if (d.cap <= 0 || d.rows <= 0) continue;
      a.c[k++] = d;
      const int64_t rpt = (int64_t)(kWave >> d.lpr_log2) * kStepItems;
      tasks += (std::min<int64_t>(d.cap, d.rows) + rpt - 1) / rpt;
    }
    if (k == 0) continue;
    a.n_cols = k;
    a.p = p;
    a.round = round;
    const int64_t want = (tasks + kWaves - 1) / kWaves;
    const unsigned blocks =
        (unsigned)std::max<int64_t>(1, std::min<int64_t>(want, (int64_t)device_cus() * kStepBlocksPerCU));
    hipLaunchKernelGGL(quant8_apply_kernel<Rule>, dim3(blocks), dim3(kBlock), 0, stream, a);
    HBK_HIP_OK(hipGetLastError());
  }
  return HBK_OK;
}

int quant8_apply_slices(int32_t n_cols, const hbk_quant8_slices_column_t* cols, int32_t apply, float* const* slot0,
                        float* const* slot1, const void* params, float lr, const hbk_lowp_rounding_t* rounding,
                        hbk_stream_t stream_) {
  static const char* kWho = "quant8_apply_slices_n";
  HBK_REQUIRE(n_cols >= 0, "%s: n_cols must be >= 0, got %d", kWho, n_cols);
  HBK_REQUIRE(n_cols == 0 || cols != nullptr, "%s: cols is NULL", kWho);
  HBK_REQUIRE(apply == HBK_APPLY_SGD || apply == HBK_APPLY_ADAGRAD || apply == HBK_APPLY_LAZY_ADAM ||
                  apply == HBK_APPLY_FTRL || apply == HBK_APPLY_ROWWISE_ADAGRAD,
              "%s: apply must be HBK_APPLY_SGD, _ADAGRAD, _LAZY_ADAM, _FTRL or _ROWWISE_ADAGRAD, got %d", kWho, apply);
  Round8 round;
  int rc = check_rounding(kWho, rounding, &round);
  if (rc != HBK_OK) return rc;
  hipStream_t stream = as_stream(stream_);
  if (apply == HBK_APPLY_LAZY_ADAM) {
    const hbk_adam_t* adam = static_cast<const hbk_adam_t*>(params);
    if ((rc = adam_check(adam, lr, kWho)) != HBK_OK) return rc;
    rc = step_columns<AdamRule>(kWho, n_cols, cols, "m", "v", slot0, slot1,
                                AdamParams{adam->beta_powers, lr, adam->beta1, adam->beta2, adam->epsilon}, round,
                                stream);
    if (rc != HBK_OK) return rc;
    if (adam->finish) {
      hipLaunchKernelGGL(quant8_adam_finish_kernel, dim3(1), dim3(kWave), 0, stream, adam->beta_powers, adam->beta1,
                         adam->beta2);
      HBK_HIP_OK(hipGetLastError());
    }
  } else if (apply == HBK_APPLY_FTRL) {
    const hbk_ftrl_t* ftrl = static_cast<const hbk_ftrl_t*>(params);
    if ((rc = ftrl_check(ftrl, lr, kWho)) != HBK_OK) return rc;
    const FtrlParams p = {lr, ftrl->l1, 2.0f * ftrl->l2, 2.0f * ftrl->l2_shrinkage, -ftrl->lr_power};
    // lr_power = -0.5 (TF's default) takes the sqrtf instantiation, any other the powf one
    rc = ftrl->lr_power != -0.5f
             ? step_columns<FtrlRule<true>>(kWho, n_cols, cols, "accum", "linear", slot0, slot1, p, round, stream)
             : step_columns<FtrlRule<false>>(kWho, n_cols, cols, "accum", "linear", slot0, slot1, p, round, stream);
    if (rc != HBK_OK) return rc;
  } else if (apply == HBK_APPLY_ROWWISE_ADAGRAD) {
    const hbk_rowwise_adagrad_t* opt = static_cast<const hbk_rowwise_adagrad_t*>(params);
    if ((rc = rowwise_adagrad_check(opt, lr, kWho)) != HBK_OK) return rc;
    rc = step_columns<RowwiseAdagradRule>(kWho, n_cols, cols, "the accumulator", nullptr, slot0, nullptr,
                                          RowwiseParams{lr, opt->epsilon}, round, stream);
    if (rc != HBK_OK) return rc;
  } else {
    HBK_REQUIRE(lr != 0.0f && lr >= -3.402823466e38f && lr <= 3.402823466e38f,
                "%s: lr must be finite and != 0, got %g", kWho, (double)lr);
    rc = apply == HBK_APPLY_ADAGRAD
             ? step_columns<AdagradRule>(kWho, n_cols, cols, "the accumulator", nullptr, slot0, nullptr, LrParams{lr},
                                         round, stream)
             : step_columns<SgdRule>(kWho, n_cols, cols, "the accumulator", nullptr, nullptr, nullptr, LrParams{lr},
                                     round, stream);
    if (rc != HBK_OK) return rc;
  }
  return advance(rounding, round, stream);
}

}  // namespace
}  // namespace hbk

extern "C" int hbk_quant8_rows_n(int32_t n_cols, const hbk_quant8_rows_column_t* cols,
                                 const hbk_lowp_rounding_t* rounding, hbk_stream_t stream) {
  return hbk::quant8_rows<true>("quant8_rows_n", n_cols, cols, rounding, stream);
}

extern "C" int hbk_dequant8_rows_n(int32_t n_cols, const hbk_quant8_rows_column_t* cols, hbk_stream_t stream) {
  return hbk::quant8_rows<false>("dequant8_rows_n", n_cols, cols, nullptr, stream);
}

extern "C" int hbk_quant8_lookup_fwd(int32_t n_cols, const hbk_quant8_lookup_column_t* cols, hbk_stream_t stream) {
  return hbk::quant8_lookup_fwd(n_cols, cols, stream);
}

extern "C" int hbk_quant8_apply_slices_n(int32_t n_cols, const hbk_quant8_slices_column_t* cols, int32_t apply,
                                         float* const* slot0, float* const* slot1, const void* params, float lr,
                                         const hbk_lowp_rounding_t* rounding, hbk_stream_t stream) {
  return hbk::quant8_apply_slices(n_cols, cols, apply, slot0, slot1, params, lr, rounding, stream);
}
