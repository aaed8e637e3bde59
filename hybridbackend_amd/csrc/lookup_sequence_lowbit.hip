// Sequence lookups over low-bit tables, fused (include/hbk.h: hbk_sequence_lookup_fwd_lowbit and
// hbk_sequence_lowbit_lane_elems): the padded [B, T, dim] rows of lookup_sequence.hip read from bf16 / fp16 rows or
// from int8 codes with a row scale, written as fp32, bf16 or fp16, with the grid and the lengths from the same
// launch.  The positions are sequence_position.h's -- the code the fp32 kernel runs -- so pad rule, truncation,
// bucket, divisor and grid words cannot differ.
//
// What was chosen, and why:
//
//   a lane owns the elements of ONE output store.  A sequence lookup is the one-id-per-segment case, and there the
//     store side decides (profiles/quant8_tables.txt): a lane that stores 16 contiguous bytes makes a wave
//     instruction write whole lines, a lane that stores 32 or 64 bytes as several instructions writes a part of
//     every line each time.  So W = 8 elements with 16-bit outputs and W = 4 with fp32 outputs, whatever the table
//     holds; the load is what follows from W: 16, 8 or 4 bytes.  16-bit outputs that cannot take W = 8 (dim % 8 != 0,
//     a block on 8 bytes) keep 4 elements per lane with one 8-byte store before they fall to W = 1, so that every
//     dim the apply kernels step (256, or 64 when dim % 4 != 0) is served.
//   rows stay packed.  A lane keeps a row chunk as it was loaded -- four, two or one 32-bit words, and the scale of an
//     8-bit row -- while the loads of its other rows are in flight, and upcasts / decodes and rounds it only when it
//     stores it (quant8_wide.hip's rule).  kU = 4 rows in flight then cost at most 16 registers where decoded rows
//     would cost 32.  A row that is not looked up is never loaded: it is the words 0 (16-bit: +0) or 0x80808080 with
//     scale 0 (8-bit: (128 - 128) * 0 = +0).
//   the wave shape of the fp32 kernel.  A wave takes kU * rpi consecutive positions (rpi = 64 >> lpr_log2 rows per
//     instruction); slot q lives in register q >> 6 of lane q & 63; ids and row splits are read once per wave and
//     reach a row's lanes by shuffle; every row load of a lane is issued before its first store; grid words and
//     outputs leave non-temporally.  Neighbouring lane groups write neighbouring rows of a sample.
//   no LDS.  Nothing is read twice by a wave: ids, splits and rows each have one reader, and the shuffle hands them
//     on.  Staging would add a round trip and buy nothing.
//
// The decode is quant8_tables.hip's ((float)code - 128.f) * scale, the upcast lowp_elems.h's, the rounding its
// bf16_nearest / fp16_nearest: one correctly rounded operation each, nothing to contract (-ffp-contract=off) and
// nothing a packed fp32 instruction would round differently, so this object carries no flag of its own.
#include <vector>

#include "common.h"
#include "lookup_common.h"
#include "lowp_elems.h"
#include "sequence_position.h"

namespace hbk {
namespace {

constexpr int kBlock = 256;   // 4 waves
constexpr int kWaves = kBlock / kWave;
constexpr int kMaxCols = 64;  // one ballot finds the column
constexpr int kU = 4;         // rows in flight per lane
constexpr uint32_t kZeroCodes = 0x80808080u;   // four codes of q = 0

struct LowbitCol {
  const uint8_t* table;
  const void* ids;
  const int32_t* splits;   // NULL: one id per sample
  void* out;
  int64_t* grid;           // NULL: not wanted
  int32_t* lengths;        // NULL: not wanted
  int64_t n_pos;           // B * T
  int64_t n_ids;
  IdMap map;
  FastDiv max_len;         // T
  uint64_t pad_row;        // what a padding position looks up (kNoRow: nothing, a zero row)
  int64_t pad_grid;        // and its grid word (-1: nothing)
  int64_t out_stride;      // elements between samples (>= T * dim)
  int32_t dim;
  int32_t chunks;          // live lanes per row (dim / W)
  int32_t pitch;           // bytes between rows
  int32_t dim4;            // 8-bit: byte offset of the scale word
  uint8_t lpr_log2;
  uint8_t ids64;
  uint8_t bf16;            // 16-bit table: its elements are bf16 (else fp16)
  uint8_t out_bf16;        // 16-bit outputs: bf16 (else fp16)
  uint8_t one_load;        // W = 8: table and pitch allow ONE 16-byte (16-bit) / 8-byte (8-bit) load per chunk
};

struct LowbitArgs {
  int32_t n_cols;
  int32_t tile_start[kMaxCols + 1];
  LowbitCol col[kMaxCols];
};
static_assert(sizeof(LowbitArgs) <= 16384, "kernarg budget");

// 32-bit words a lane keeps of a row: W 16-bit elements, or W codes
constexpr int words_of(bool q8, int w) { return q8 ? (w + 3) / 4 : (w + 1) / 2; }

// a row before it is loaded, and a row that never is
template <bool Q8, int W>
__device__ inline void zero_packed(uint32_t (&p)[words_of(Q8, W)], float& scale) {
#pragma unroll
  for (int i = 0; i < words_of(Q8, W); ++i) p[i] = Q8 ? kZeroCodes : 0u;
  scale = 0.f;
}

// lane chunk `sub` of row r, packed, and (8-bit) the row's scale
template <bool Q8, int W>
__device__ inline void load_packed(const LowbitCol& c, uint64_t r, int sub, uint32_t (&p)[words_of(Q8, W)],
                                   float& scale) {
  const uint8_t* const row = c.table + r * (uint64_t)(uint32_t)c.pitch;
  if constexpr (Q8) {
    const uint8_t* const at = row + sub * W;
    if constexpr (W == 8) {
      if (c.one_load) {   // (uniform: one column per wave)
        const u32x2 x = *reinterpret_cast<const u32x2*>(at);
        p[0] = x[0];
        p[1] = x[1];
      } else {
        p[0] = *reinterpret_cast<const uint32_t*>(at);
        p[1] = *reinterpret_cast<const uint32_t*>(at + 4);
      }
    } else if constexpr (W == 4) {
      p[0] = *reinterpret_cast<const uint32_t*>(at);
    } else {
      p[0] = *at;
    }
    scale = *reinterpret_cast<const float*>(row + c.dim4);
  } else {
    const uint8_t* const at = row + sub * (2 * W);
    if constexpr (W == 8) {
      if (c.one_load) {
        const u32x4 x = *reinterpret_cast<const u32x4*>(at);
#pragma unroll
        for (int i = 0; i < 4; ++i) p[i] = x[i];
      } else {
        const u32x2 x = *reinterpret_cast<const u32x2*>(at), y = *reinterpret_cast<const u32x2*>(at + 8);
        p[0] = x[0];
        p[1] = x[1];
        p[2] = y[0];
        p[3] = y[1];
      }
    } else if constexpr (W == 4) {
      const u32x2 x = *reinterpret_cast<const u32x2*>(at);
      p[0] = x[0];
      p[1] = x[1];
    } else {
      p[0] = *reinterpret_cast<const uint16_t*>(at);
    }
  }
}

// element i of a packed chunk as fp32: the exact upcast, or quant8_tables.hip's decode
template <bool Q8>
__device__ inline float elem_of(const uint32_t* p, int i, float scale, bool bf16) {
  if constexpr (Q8) {
    const uint32_t code = (p[i >> 2] >> (8 * (i & 3))) & 0xffu;
    return ((float)code - 128.0f) * scale;
  } else {
    return upcast((p[i >> 1] >> (16 * (i & 1))) & 0xffffu, bf16);
  }
}

__device__ inline uint32_t round16(float x, bool bf16) { return bf16 ? bf16_nearest(x) : fp16_nearest(x); }

// the lane's W elements as ONE streamed store at element `off` of out
template <int W, bool O16>
__device__ inline void store_elems(void* out, int64_t off, bool obf16, const float (&v)[W]) {
  if constexpr (!O16) {
    float* const o = static_cast<float*>(out) + off;
    if constexpr (W == 4) {
      const f32x4 x = {v[0], v[1], v[2], v[3]};
      __builtin_nontemporal_store(x, reinterpret_cast<f32x4*>(o));
    } else {
      static_assert(W == 1, "fp32 outputs: 4 elements per lane or one");
      __builtin_nontemporal_store(v[0], o);
    }
  } else {
    uint16_t* const o = static_cast<uint16_t*>(out) + off;
    if constexpr (W == 1) {
      __builtin_nontemporal_store((uint16_t)round16(v[0], obf16), o);
    } else {
      uint32_t w[W / 2];
#pragma unroll
      for (int k = 0; k < W / 2; ++k) w[k] = round16(v[2 * k], obf16) | (round16(v[2 * k + 1], obf16) << 16);
      if constexpr (W == 8) {
        const u32x4 x = {w[0], w[1], w[2], w[3]};
        __builtin_nontemporal_store(x, reinterpret_cast<u32x4*>(o));
      } else {
        const u32x2 x = {w[0], w[1]};
        __builtin_nontemporal_store(x, reinterpret_cast<u32x2*>(o));
      }
    }
  }
}

// kU * rpi consecutive positions per wave: slot q lives in register q >> 6 of lane q & 63
template <bool Q8, int W, bool O16>
__global__ __launch_bounds__(kBlock) void sequence_lowbit_fwd_kernel(const LowbitArgs a) {
  constexpr int NW = words_of(Q8, W);
  const int b = (int)blockIdx.x;
  const int lane = lane_id();
  const int ci = column_of(a.tile_start, a.n_cols, b, lane);
  const LowbitCol& c = a.col[ci];
  const int wave = (int)(threadIdx.x >> 6);
  const int lpr_log2 = c.lpr_log2;
  const int rpi = kWave >> lpr_log2;  // rows per wave instruction
  const int sub = lane & ((1 << lpr_log2) - 1);
  const int grp = lane >> lpr_log2;
  const int n_slots = kU * rpi;
  const int64_t pos0 = ((int64_t)(b - a.tile_start[ci]) * kWaves + wave) * (int64_t)n_slots;
  if (pos0 >= c.n_pos) return;   // (wave-uniform)

  uint64_t rowreg[kU];
#pragma unroll
  for (int k = 0; k < kU; ++k) {
    const int q = k * kWave + lane;
    const int64_t p = pos0 + q;
    rowreg[k] = seq_position(c, p, q < n_slots && p < c.n_pos);
  }

  uint32_t packed[kU][NW];
  float scale[kU];
  const bool live = sub < c.chunks;
  // every row load of the lane is issued before the first store
#pragma unroll
  for (int u = 0; u < kU; ++u) {
    const int q0 = u * rpi;  // a multiple of rpi (a power of two <= 64): q0 >> 6 is uniform
    const int k = q0 >> 6;
    uint64_t src = rowreg[0];
#pragma unroll
    for (int kk = 1; kk < kU; ++kk) src = (k == kk) ? rowreg[kk] : src;
    const uint64_t r = shfl_u64(src, (q0 & (kWave - 1)) + grp);
    zero_packed<Q8, W>(packed[u], scale[u]);
    if (live && r != kNoRow) load_packed<Q8, W>(c, r, sub, packed[u], scale[u]);
  }
  const int64_t T = (int64_t)c.max_len.d;
  const bool bf16 = c.bf16 != 0, obf16 = c.out_bf16 != 0;
#pragma unroll
  for (int u = 0; u < kU; ++u) {
    const int64_t p = pos0 + u * rpi + grp;
    if (live && p < c.n_pos) {
      float v[W];
#pragma unroll
      for (int i = 0; i < W; ++i) v[i] = elem_of<Q8>(packed[u], i, scale[u], bf16);
      const int64_t s = (int64_t)fastdiv((uint64_t)p, c.max_len);
      const int64_t off = s * c.out_stride + (p - s * T) * (int64_t)c.dim + (int64_t)sub * W;
      store_elems<W, O16>(c.out, off, obf16, v);
    }
  }
}

template <bool Q8, int W, bool O16>
void launch_lowbit(const LowbitArgs& args, unsigned tiles, hipStream_t stream) {
  hipLaunchKernelGGL((sequence_lowbit_fwd_kernel<Q8, W, O16>), dim3(tiles), dim3(kBlock), 0, stream, args);
}

inline int32_t round_up4(int32_t d) { return (d + 3) & ~3; }
inline bool is_q8(const hbk_sequence_lowbit_column_t& h) { return h.row_format == HBK_ROWS_INT8; }
inline bool format_ok(const hbk_sequence_lowbit_column_t& h) {
  return h.row_format == HBK_LOWP_BF16 || h.row_format == HBK_LOWP_FP16 || h.row_format == HBK_ROWS_INT8;
}
inline bool out_dtype_ok(const hbk_sequence_lowbit_column_t& h) {
  return h.out_dtype == HBK_QUANT8_OUT_FP32 || h.out_dtype == HBK_LOWP_BF16 || h.out_dtype == HBK_LOWP_FP16;
}
inline int esize_of(const hbk_sequence_lowbit_column_t& h) { return h.out_dtype == HBK_QUANT8_OUT_FP32 ? 4 : 2; }
inline int32_t pitch_of(const hbk_sequence_lowbit_column_t& h) {
  return h.pitch != 0 ? h.pitch : (is_q8(h) ? round_up4(h.dim) + 4 : 2 * h.dim);
}
// table and pitch together: what every row's base is a multiple of
inline uintptr_t table_bits(const hbk_sequence_lowbit_column_t& h) {
  return (uintptr_t)h.table | (uintptr_t)(uint32_t)pitch_of(h);
}

// the elements a lane of this column moves: 8, 4 or 1 (an out_stride of 0 is T * dim, a multiple of whatever dim is)
int lane_elems_of(const hbk_sequence_lowbit_column_t& h) {
  const uintptr_t esize = (uintptr_t)esize_of(h);
  const uintptr_t out_bits = (uintptr_t)h.out | ((uintptr_t)h.out_stride * esize);
  // a 16-bit row chunk is read as 8-byte pieces at least; codes as 4-byte words, which the layout promises
  const bool table_ok = is_q8(h) || table_bits(h) % 8 == 0;
  if (!table_ok || h.dim > 256) return 1;
  if (esize == 2 && h.dim % 8 == 0 && out_bits % 16 == 0) return 8;
  if (h.dim % 4 == 0 && out_bits % (esize == 2 ? 8 : 16) == 0) return 4;
  return 1;
}

int sequence_lookup_fwd_lowbit(int32_t n_cols, const hbk_sequence_lowbit_column_t* cols, const hbk_sequence_t* seq,
                               hbk_stream_t stream_) {
  static const char* kWho = "sequence_lookup_fwd_lowbit";
  HBK_REQUIRE(n_cols >= 0, "%s: n_cols must be >= 0, got %d", kWho, n_cols);
  HBK_REQUIRE(n_cols == 0 || cols != nullptr, "%s: cols is NULL", kWho);
  HBK_REQUIRE(n_cols == 0 || seq != nullptr, "%s: seq is NULL", kWho);
  // kinds: 8-bit table * 5 + {W8 / 16-bit out, W4 / 16-bit, W1 / 16-bit, W4 / fp32, W1 / fp32}
  constexpr int kKinds = 10;
  std::vector<int> kind_of((size_t)(n_cols > 0 ? n_cols : 1), -1);   // -1: nothing to do (no samples)
  std::vector<int> width((size_t)(n_cols > 0 ? n_cols : 1), 0);
  bool kinds_present[kKinds] = {};
  for (int32_t c = 0; c < n_cols; ++c) {
    const hbk_sequence_lowbit_column_t& h = cols[c];
    const hbk_sequence_t& q = seq[c];
    HBK_REQUIRE(format_ok(h),
                "%s: column %d: row_format must be HBK_LOWP_BF16, HBK_LOWP_FP16 or HBK_ROWS_INT8, got %d", kWho, c,
                h.row_format);
    HBK_REQUIRE(out_dtype_ok(h),
                "%s: column %d: out_dtype must be HBK_QUANT8_OUT_FP32, HBK_LOWP_BF16 or HBK_LOWP_FP16, got %d", kWho, c,
                h.out_dtype);
    HBK_REQUIRE(q.max_len >= 1, "%s: column %d: max_len must be >= 1, got %d", kWho, c, q.max_len);
    HBK_REQUIRE(h.dim >= 1 && h.dim <= 256, "%s: column %d: dim must be in [1, 256], got %d", kWho, c, h.dim);
    const int32_t pitch = pitch_of(h);
    if (is_q8(h)) {
      const int32_t dim4 = round_up4(h.dim);
      HBK_REQUIRE(pitch % 4 == 0 && pitch >= dim4 + 4,
                  "%s: column %d: pitch %d must be a multiple of 4 and >= round_up(dim, 4) + 4 = %d", kWho, c, pitch,
                  dim4 + 4);
      HBK_REQUIRE(((uintptr_t)h.table & 3) == 0, "%s: column %d: an 8-bit table must be 4-byte aligned", kWho, c);
    } else {
      HBK_REQUIRE(pitch % 2 == 0 && pitch >= 2 * h.dim,
                  "%s: column %d: pitch %d must be even and >= 2 * dim = %d bytes", kWho, c, pitch, 2 * h.dim);
      HBK_REQUIRE(((uintptr_t)h.table & 1) == 0, "%s: column %d: a 16-bit table must be 2-byte aligned", kWho, c);
    }
    HBK_REQUIRE(h.rows >= 0 && h.n_ids >= 0 && h.n_segments >= 0, "%s: column %d: negative size", kWho, c);
    HBK_REQUIRE(h.ids_dtype == HBK_INT32 || h.ids_dtype == HBK_INT64, "%s: column %d: ids must be int32 or int64",
                kWho, c);
    HBK_REQUIRE(h.bucket >= 0, "%s: column %d: bucket must be >= 0", kWho, c);
    HBK_REQUIRE(h.divisor >= 1, "%s: column %d: divisor must be >= 1", kWho, c);
    HBK_REQUIRE(h.row_splits != nullptr || h.n_segments == h.n_ids,
                "%s: column %d: n_segments (%lld) must equal n_ids (%lld) when row_splits is NULL", kWho, c,
                (long long)h.n_segments, (long long)h.n_ids);
    HBK_REQUIRE(h.n_ids < (1ll << 31), "%s: column %d: more than 2^31-1 ids", kWho, c);
    HBK_REQUIRE(h.n_segments < (1ll << 31) && h.n_segments * (int64_t)q.max_len < (1ll << 31),
                "%s: column %d: B * T = %lld x %d positions, must stay below 2^31", kWho, c, (long long)h.n_segments,
                q.max_len);
    const int64_t sample = (int64_t)q.max_len * h.dim;
    HBK_REQUIRE(sample < (1ll << 31) && (h.out_stride == 0 || h.out_stride >= sample),
                "%s: column %d: out_stride %lld is smaller than max_len * dim = %lld elements (or that exceeds "
                "2^31-1)", kWho, c, (long long)h.out_stride, (long long)sample);
    HBK_REQUIRE(h.out_stride < (1ll << 40), "%s: column %d: out_stride %lld is out of range", kWho, c,
                (long long)h.out_stride);
    HBK_REQUIRE(((uintptr_t)h.out & (uintptr_t)(esize_of(h) - 1)) == 0,
                "%s: column %d: out must be aligned to its element", kWho, c);
    const int w = lane_elems_of(h);
    HBK_REQUIRE(w > 1 || h.dim <= 64,
                "%s: column %d: dim %d: at most 256 when dim %% 4 == 0 and the table rows, out and its sample stride "
                "are on the lane's boundary, 64 otherwise", kWho, c, h.dim);
    if (h.n_segments == 0) continue;
    HBK_REQUIRE(h.table != nullptr || h.rows == 0, "%s: column %d: table is NULL", kWho, c);
    HBK_REQUIRE(h.out != nullptr, "%s: column %d: out is NULL", kWho, c);
    HBK_REQUIRE(h.ids != nullptr || h.n_ids == 0, "%s: column %d: ids is NULL", kWho, c);
    width[(size_t)c] = w;
    const bool o16 = esize_of(h) == 2;
    kind_of[(size_t)c] = (is_q8(h) ? 5 : 0) + (o16 ? (w == 8 ? 0 : w == 4 ? 1 : 2) : (w == 4 ? 3 : 4));
    kinds_present[kind_of[(size_t)c]] = true;
  }
  hipStream_t stream = as_stream(stream_);
  for (int kind = 0; kind < kKinds; ++kind) {
    if (!kinds_present[kind]) continue;
    int32_t c0 = 0;
    while (c0 < n_cols) {
      LowbitArgs args;
      int32_t k = 0;
      int64_t tiles = 0;
      args.tile_start[0] = 0;
      while (c0 < n_cols && k < kMaxCols) {
        const int32_t ci = c0++;
        if (kind_of[(size_t)ci] != kind) continue;
        const hbk_sequence_lowbit_column_t& h = cols[ci];
        const hbk_sequence_t& q = seq[ci];
        const int w = width[(size_t)ci];
        LowbitCol& d = args.col[k];
        d.table = static_cast<const uint8_t*>(h.table);
        d.ids = h.ids;
        d.splits = h.row_splits;
        d.out = h.out;
        d.grid = q.row_grid;
        d.lengths = q.lengths;
        d.n_pos = h.n_segments * (int64_t)q.max_len;
        d.n_ids = h.n_ids;
        d.map = make_idmap(h.bucket, h.divisor, h.rows);
        d.max_len = make_fastdiv((uint64_t)q.max_len);
        d.pad_row = kNoRow;
        d.pad_grid = -1;
        if (q.has_pad != 0) d.pad_row = seq_map(d.map, q.pad_id, &d.pad_grid);
        d.out_stride = h.out_stride > 0 ? h.out_stride : (int64_t)q.max_len * h.dim;
        d.dim = h.dim;
        d.chunks = h.dim / w;
        d.pitch = pitch_of(h);
        d.dim4 = round_up4(h.dim);
        d.lpr_log2 = (uint8_t)ceil_log2_u32((uint32_t)d.chunks);
        d.ids64 = h.ids_dtype == HBK_INT64;
        d.bf16 = h.row_format == HBK_LOWP_BF16;
        d.out_bf16 = h.out_dtype == HBK_LOWP_BF16;
        d.one_load = table_bits(h) % (is_q8(h) ? 8 : 16) == 0;
        const int64_t per_block = (int64_t)kWaves * (kWave >> d.lpr_log2) * kU;
        tiles += (d.n_pos + per_block - 1) / per_block;
        HBK_REQUIRE(tiles < (1ll << 31), "%s: grid too large", kWho);
        args.tile_start[++k] = (int32_t)tiles;
      }
      if (k == 0) continue;
      args.n_cols = k;
      const unsigned t = (unsigned)tiles;
      switch (kind) {
        case 0: launch_lowbit<false, 8, true>(args, t, stream); break;
        case 1: launch_lowbit<false, 4, true>(args, t, stream); break;
        case 2: launch_lowbit<false, 1, true>(args, t, stream); break;
        case 3: launch_lowbit<false, 4, false>(args, t, stream); break;
        case 4: launch_lowbit<false, 1, false>(args, t, stream); break;
        case 5: launch_lowbit<true, 8, true>(args, t, stream); break;
        case 6: launch_lowbit<true, 4, true>(args, t, stream); break;
        case 7: launch_lowbit<true, 1, true>(args, t, stream); break;
        case 8: launch_lowbit<true, 4, false>(args, t, stream); break;
        default: launch_lowbit<true, 1, false>(args, t, stream); break;
      }
      HBK_HIP_OK(hipGetLastError());
    }
  }
  return HBK_OK;
}

}  // namespace
}  // namespace hbk

extern "C" int hbk_sequence_lookup_fwd_lowbit(int32_t n_cols, const hbk_sequence_lowbit_column_t* cols,
                                              const hbk_sequence_t* seq, hbk_stream_t stream) {
  return hbk::sequence_lookup_fwd_lowbit(n_cols, cols, seq, stream);
}

extern "C" int32_t hbk_sequence_lowbit_lane_elems(const hbk_sequence_lowbit_column_t* col) {
  if (col == nullptr || !hbk::format_ok(*col) || !hbk::out_dtype_ok(*col) || col->dim < 1) return 0;
  return hbk::lane_elems_of(*col);
}
