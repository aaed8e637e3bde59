// 8-bit tables, the forward with lanes of 8 or 16 codes (include/hbk.h, "8-bit tables": hbk_quant8_lookup_fwd_wide
// and hbk_quant8_lookup_lane_codes).  quant8_tables.hip's forward gives a lane 4 codes: one 4-byte load, one 16-byte
// (fp32) or 8-byte (16-bit) store.  Here a row is owned by LPR = pow2(dim / L) adjacent lanes of L = 8 or 16
// consecutive codes, so that a wave instruction covers 2x / 4x the rows and a lane's store is one (L = 8) or two
// (L = 16) 16-byte stores of 16-bit elements, or L / 4 of fp32.  The sums are those of quant8_tables.hip expression
// for expression -- the same id map and decode, in-order fp32 sums from +0, the same weighted forms and zero rules,
// one rounding to nearest even -- so no bit depends on the lane width.
//
// What was chosen, and why:
//
//   codes stay packed until they are needed.  A lane keeps a row as its L / 4 code words, the scale and (weighted)
//     the weight -- at most 6 registers -- while the loads of its other rows are in flight, and decodes a row only
//     when it stores it (one id per segment) or adds it (ragged).  4 rows in flight per lane therefore cost 24
//     registers at L = 16 where 4 decoded rows would cost 64, and kWideU stays 4 at both widths without a spill.
//     A row that is not loaded (an invalid id, a lane past dim) is the words 0x80808080 with scale 0, which decode
//     to +0 exactly: the zero row of the narrow kernels.
//   two forms of the code load, chosen by the host per column and uniform in a wave: L / 4 loads of 4 bytes at
//     consecutive words (all the layout promises: base and pitch multiples of 4), or ONE 8- / 16-byte load when the
//     table's base and pitch are multiples of L.  The scale word is one 4-byte load per row and lane.  (Global
//     memory on gfx950 takes a multi-word load at any 4-byte boundary, and the compiler knows it: it merges the
//     consecutive 4-byte loads of the first form into the instruction of the second.  Measured, the forms differ
//     by what the wider pitch costs or saves -- under 2 % with one id per segment -- and not by the instruction;
//     profiles/quant8_tables.txt.)
//   one id per segment: the skeleton of the narrow kernel.  Ids and weights are read once per wave, non-temporally,
//     slot q in register q >> 6 of lane q & 63, and handed to a row's lanes by shuffle; every row load of a lane is
//     issued before its first store.
//   ragged: the id chunk is decoupled from LPR.  The narrow kernel's lane group fetches LPR ids per chunk, which at
//     L = 16 and dim 64 would be 4 and at dim 16 ONE: a serial chain of memory round trips per id.  Here a lane
//     group always prefetches max(LPR, K) ids per chunk, K = 64 / L (8 at L = 8, 4 at L = 16, where a lane's 16 sums
//     leave fewer registers): slot t of a chunk lives in register t / LPR of lane t % LPR of the group (R = K / LPR
//     registers per lane for LPR < K), the next chunk is fetched while this chunk's rows are in flight, and the rows
//     of a chunk are loaded four at a time and added in id order, from +0.  LPR < K is a template parameter, picked
//     per column inside the kernel, so a slot's register is a constant and a group of one lane shuffles nothing.
//     The price is registers: 99 - 114 against the narrow kernel's 66, 4 waves per SIMD against 7.
//
// What it measured (profiles/quant8_tables.txt): the store side decides.  With 16-bit outputs a lane of 8 codes
// stores 16 contiguous bytes and a wave instruction whole lines: 6 - 19 % faster than 4 codes per lane with one id per
// segment.  A lane of 16 codes, and any wide lane with fp32 outputs, stores its 32 or 64 bytes as two or four
// instructions each of which writes a part of every line: up to 3x SLOWER with one id per segment.  Ragged at dim 64,
// where stores are one in nine accesses, 8 codes win 9 - 10 % and 16 codes 27 % (16-bit outputs); ragged at dim 16
// every width loses 14 % or more.  `lane_codes='auto'` (embedding/quant8.py) names a width only where it won.
//
// Columns that cannot take L codes per lane (dim % L != 0, an output block or stride off its 16-byte boundary) are
// handed, in the same call and behind the wide launches, to hbk_quant8_lookup_fwd, which runs them at 4 or 1 codes
// per lane as it always has.  No LDS, no atomics, no workspace, no host read: the call can be captured.
//
// Compiled as quant8_tables.hip is (no packed fp32 operations, no contraction).
#include <algorithm>
#include <vector>

#include "common.h"
#include "lookup_common.h"
#include "lowp_elems.h"

namespace hbk {
namespace {

constexpr int kMaxCols = 64;   // columns per launch
constexpr int kBlock = 256;
constexpr int kWaves = kBlock / kWave;
constexpr int kWideU = 4;          // rows in flight per lane (one id per segment), at both widths
constexpr int kWideSegIters = 4;   // segments per lane group and wave (ragged)
// ids a lane group of fewer lanes than this prefetches per chunk (ragged): 8 at L = 8, 4 at L = 16, where a lane's 16
// sums and its rows in flight leave fewer registers for ids
template <int L>
constexpr int kIdChunk = 64 / L;
constexpr uint32_t kZeroCodes = 0x80808080u;   // four codes of q = 0

struct WideCol {
  const uint8_t* table;
  const void* ids;
  const int32_t* splits;
  const float* weights;
  void* out;
  int64_t n_seg;
  IdMap map;
  int32_t dim4;         // byte offset of the scale word
  int32_t pitch;        // bytes between rows
  int32_t chunks;       // live lanes per row (dim / L)
  int32_t out_stride;   // elements between output rows
  uint8_t lpr_log2;
  uint8_t ids64;
  uint8_t combiner;
  uint8_t out_bf16;
  uint8_t one_load;     // base and pitch are multiples of L: one L-byte load of codes per row and lane
};

struct WideArgs {
  int32_t n_cols;
  int32_t tile_start[kMaxCols + 1];
  WideCol col[kMaxCols];
};
static_assert(sizeof(WideArgs) <= 16384, "kernarg budget");

// code c of a row with `scale`: (c - 128) * scale (quant8_tables.hip's decode)
__device__ inline float decode(uint32_t c, float scale) { return ((float)c - 128.0f) * scale; }
__device__ inline float decode_at(const uint32_t* p, int i, float scale) {
  return decode((p[i >> 2] >> (8 * (i & 3))) & 0xffu, scale);
}
__device__ inline uint32_t round16(float x, bool bf16) { return bf16 ? bf16_nearest(x) : fp16_nearest(x); }

// a row before it is loaded, and a row that never is: L codes of q = 0 with scale 0
template <int L>
__device__ inline void zero_codes(uint32_t (&p)[L / 4], float& scale) {
#pragma unroll
  for (int i = 0; i < L / 4; ++i) p[i] = kZeroCodes;
  scale = 0.f;
}

// lane chunk `sub` of row r, packed, and the row's scale
template <int L, bool ONE>
__device__ inline void load_codes(const WideCol& c, uint64_t r, int sub, uint32_t (&p)[L / 4], float& scale) {
  const uint8_t* const row = c.table + r * (uint64_t)(uint32_t)c.pitch;
  const uint8_t* const at = row + sub * L;
  if constexpr (!ONE) {
#pragma unroll
    for (int i = 0; i < L / 4; ++i) p[i] = *reinterpret_cast<const uint32_t*>(at + 4 * i);
  } else if constexpr (L == 8) {
    const u32x2 x = *reinterpret_cast<const u32x2*>(at);
    p[0] = x[0];
    p[1] = x[1];
  } else {
    const u32x4 x = *reinterpret_cast<const u32x4*>(at);
#pragma unroll
    for (int i = 0; i < 4; ++i) p[i] = x[i];
  }
  scale = *reinterpret_cast<const float*>(row + c.dim4);
}

// L sums stored at element `off`, streamed: fp32 as L / 4 16-byte stores, 16-bit (rounded once) as L / 8
template <int L, bool O16>
__device__ inline void store_sums(void* out, int64_t off, bool bf16, const float (&v)[L]) {
  if constexpr (!O16) {
    f32x4* const o = reinterpret_cast<f32x4*>(static_cast<float*>(out) + off);
#pragma unroll
    for (int i = 0; i < L / 4; ++i) {
      const f32x4 x = {v[4 * i], v[4 * i + 1], v[4 * i + 2], v[4 * i + 3]};
      __builtin_nontemporal_store(x, o + i);
    }
  } else {
    u32x4* const o = reinterpret_cast<u32x4*>(static_cast<uint16_t*>(out) + off);
#pragma unroll
    for (int i = 0; i < L / 8; ++i) {
      u32x4 x;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        x[k] = round16(v[8 * i + 2 * k], bf16) | (round16(v[8 * i + 2 * k + 1], bf16) << 16);
      }
      __builtin_nontemporal_store(x, o + i);
    }
  }
}

// register k (uniform) of a lane's N: a chain of selects that folds when k is a constant
template <int N, typename T>
__device__ inline T pick(const T (&reg)[N], int k) {
  T x = reg[0];
#pragma unroll
  for (int kk = 1; kk < N; ++kk) x = (k == kk) ? reg[kk] : x;
  return x;
}

// one id per segment: out[s, :] = decode(table[row(ids[s]), :]), times the segment's weight when weighted
// (q8_gather_rows of quant8_tables.hip: the same expressions in the same order)
template <int L, bool O16, bool ONE>
__device__ inline void wide_gather_rows(const WideCol& c, int64_t wave_row0) {
  const int lane = lane_id();
  const int lpr_log2 = c.lpr_log2;
  const int rpi = kWave >> lpr_log2;   // rows per wave instruction
  const int sub = lane & ((1 << lpr_log2) - 1);
  const int grp = lane >> lpr_log2;
  const int64_t n_seg = c.n_seg;
  const bool wgt = c.weights != nullptr;   // (uniform: one column per wave)
  const bool obf16 = c.out_bf16 != 0;

  // ids: slot q (0 <= q < U * rpi) lives in register q >> 6 of lane q & 63
  uint64_t rowreg[kWideU];
  float wreg[kWideU];
  const int n_slots = kWideU * rpi;
#pragma unroll
  for (int k = 0; k < kWideU; ++k) {
    rowreg[k] = kNoRow;
    wreg[k] = 0.f;
    const int q = k * kWave + lane;
    const int64_t s = wave_row0 + q;
    if (q < n_slots && s < n_seg) {
      rowreg[k] = id_to_row(c.map, load_id(c.ids, c.ids64, s));
      if (wgt) wreg[k] = __builtin_nontemporal_load(c.weights + s);
    }
  }
  uint32_t p[kWideU][L / 4];
  float scale[kWideU], w[kWideU];
  bool valid[kWideU];
  const bool live = sub < c.chunks;
  // every row load of the lane is issued before the first store
#pragma unroll
  for (int u = 0; u < kWideU; ++u) {
    const int q0 = u * rpi;   // a multiple of rpi (a power of two <= 64): q0 >> 6 is uniform
    const int src = (q0 & (kWave - 1)) + grp;
    const int k = q0 >> 6;
    uint64_t rsrc = rowreg[0];
#pragma unroll
    for (int kk = 1; kk < kWideU; ++kk) rsrc = (k == kk) ? rowreg[kk] : rsrc;
    const uint64_t r = shfl_u64(rsrc, src);
    valid[u] = r != kNoRow;
    zero_codes<L>(p[u], scale[u]);
    if (live && valid[u]) load_codes<L, ONE>(c, r, sub, p[u], scale[u]);
    w[u] = 0.f;
    if (wgt) {
      float wsrc = wreg[0];
#pragma unroll
      for (int kk = 1; kk < kWideU; ++kk) wsrc = (k == kk) ? wreg[kk] : wsrc;
      w[u] = __shfl(wsrc, src, kWave);
    }
  }
#pragma unroll
  for (int u = 0; u < kWideU; ++u) {
    float v[L];
#pragma unroll
    for (int i = 0; i < L; ++i) v[i] = decode_at(p[u], i, scale[u]);
    if (wgt) {
      const float div = c.combiner == HBK_COMBINER_MEAN    ? w[u]
                        : c.combiner == HBK_COMBINER_SQRTN ? sqrtf(w[u] * w[u])
                                                           : 1.f;
      if (valid[u] && div != 0.f) {
#pragma unroll
        for (int i = 0; i < L; ++i) {
          v[i] = v[i] * w[u];
          if (c.combiner != HBK_COMBINER_SUM) v[i] = v[i] / div;
        }
      } else {
#pragma unroll
        for (int i = 0; i < L; ++i) v[i] = 0.f;
      }
    }
    const int64_t s = wave_row0 + u * rpi + grp;
    if (live && s < n_seg) store_sums<L, O16>(c.out, s * (int64_t)c.out_stride + (int64_t)sub * L, obf16, v);
  }
}

// ragged segments: out[s, :] = combine_j decode(table[row(ids[j]), :]) in id order, from +0 (q8_combine_segments of
// quant8_tables.hip: the same expressions in the same order).  LG >= 0: the group has 2^LG < K lanes (K =
// kIdChunk<L>) and fetches K ids per chunk, R = K >> LG per lane; LG < 0: the group has LPR >= K lanes and fetches
// LPR ids per chunk, one per lane.  Slot t of a chunk is id j0 + t, held in register t / LPR of lane t % LPR.
template <int L, bool O16, bool ONE, int LG>
__device__ inline void wide_combine_segments(const WideCol& c, int64_t wave_seg0) {
  constexpr int K = kIdChunk<L>;
  constexpr int R = LG >= 0 ? (K >> LG) : 1;
  static_assert(R >= 1 && (LG < 0 || R > 1), "a group of K or more lanes holds one id per lane");
  const int lane = lane_id();
  const int lpr_log2 = LG >= 0 ? LG : (int)c.lpr_log2;
  const int lpr = 1 << lpr_log2;
  const int chunk = R * lpr;   // LG >= 0: K
  const int rpi = kWave >> lpr_log2;
  const int sub = lane & (lpr - 1);
  const int grp = lane >> lpr_log2;
  const int grp_lane0 = grp << lpr_log2;
  const int64_t n_seg = c.n_seg;
  const bool live = sub < c.chunks;
  const bool wgt = c.weights != nullptr;
  const bool obf16 = c.out_bf16 != 0;

  for (int it = 0; it < kWideSegIters; ++it) {
    const int64_t s = wave_seg0 + (int64_t)it * rpi + grp;
    int32_t beg = 0, end = 0;
    if (s < n_seg) {
      beg = c.splits[s];
      end = c.splits[s + 1];
    }
    float acc[L];
#pragma unroll
    for (int i = 0; i < L; ++i) acc[i] = 0.f;
    float wsum = 0.f;   // weighted: W_s or Q_s
    int32_t j0 = beg;
    uint64_t myrow[R];
    float myw[R];
#pragma unroll
    for (int k = 0; k < R; ++k) {
      myrow[k] = kNoRow;
      myw[k] = 0.f;
      const int32_t j = j0 + k * lpr + sub;
      if (j < end) {
        myrow[k] = id_to_row(c.map, load_id(c.ids, c.ids64, j));
        if (wgt) myw[k] = __builtin_nontemporal_load(c.weights + j);
      }
    }
    while (__any(j0 < end)) {
      uint64_t nextrow[R];
      float nextw[R];
      const int32_t j1 = j0 + chunk;
#pragma unroll
      for (int k = 0; k < R; ++k) {
        nextrow[k] = kNoRow;
        nextw[k] = 0.f;
        const int32_t j = j1 + k * lpr + sub;
        if (j < end) {
          nextrow[k] = id_to_row(c.map, load_id(c.ids, c.ids64, j));
          if (wgt) nextw[k] = __builtin_nontemporal_load(c.weights + j);
        }
      }
      const int32_t cnt = end - j0;   // ids of this group still to add (may be <= 0)
      // slots t0 .. t0 + 3 of the chunk: four row loads in flight, then added in id order
      auto add4 = [&](int t0) {
        uint32_t p[4][L / 4];
        float scale[4], w[4];
        bool on[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          const int tt = t0 + t;
          const int k = LG >= 0 ? tt >> lpr_log2 : 0;   // (LG >= 0: a constant once add4 is unrolled)
          uint64_t r = pick(myrow, k);
          w[t] = wgt ? pick(myw, k) : 0.f;
          if constexpr (LG != 0) {   // (a group of one lane holds its own ids)
            const int src = grp_lane0 + (tt & (lpr - 1));
            r = shfl_u64(r, src);
            if (wgt) w[t] = __shfl(w[t], src, kWave);
          }
          on[t] = tt < cnt;
          if (wgt) on[t] = on[t] && r != kNoRow;   // an invalid row adds neither term nor weight
          zero_codes<L>(p[t], scale[t]);
          if (on[t] && live && r != kNoRow) load_codes<L, ONE>(c, r, sub, p[t], scale[t]);
        }
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          if (!on[t]) continue;
          if (wgt) {
#pragma unroll
            for (int i = 0; i < L; ++i) acc[i] = acc[i] + decode_at(p[t], i, scale[t]) * w[t];
            wsum = wsum + (c.combiner == HBK_COMBINER_SQRTN ? w[t] * w[t] : w[t]);
          } else {
#pragma unroll
            for (int i = 0; i < L; ++i) acc[i] = acc[i] + decode_at(p[t], i, scale[t]);
          }
        }
      };
      if constexpr (LG >= 0) {
#pragma unroll
        for (int t0 = 0; t0 < K; t0 += 4) add4(t0);
      } else {
        for (int t0 = 0; t0 < lpr; t0 += 4) add4(t0);
      }
#pragma unroll
      for (int k = 0; k < R; ++k) {
        myrow[k] = nextrow[k];
        myw[k] = nextw[k];
      }
      j0 = j1;
    }
    const int32_t n = end - beg;
    if (wgt) {
      if (c.combiner != HBK_COMBINER_SUM) {
        const float div = c.combiner == HBK_COMBINER_MEAN ? wsum : sqrtf(wsum);
#pragma unroll
        for (int i = 0; i < L; ++i) acc[i] = div != 0.f ? acc[i] / div : 0.f;
      }
    } else if (n > 0 && c.combiner == HBK_COMBINER_MEAN) {
      const float fn = (float)n;
#pragma unroll
      for (int i = 0; i < L; ++i) acc[i] = acc[i] / fn;
    } else if (n > 0 && c.combiner == HBK_COMBINER_SQRTN) {
      const float fn = sqrtf((float)n);
#pragma unroll
      for (int i = 0; i < L; ++i) acc[i] = acc[i] / fn;
    }
    if (live && s < n_seg) store_sums<L, O16>(c.out, s * (int64_t)c.out_stride + (int64_t)sub * L, obf16, acc);
  }
}

// the instantiation of a column's lane group (uniform: one column per block)
template <int L, bool O16, bool ONE>
__device__ inline void wide_combine_by_lanes(const WideCol& c, int64_t first) {
  const int lg = c.lpr_log2;
  if (lg == 0) {
    wide_combine_segments<L, O16, ONE, 0>(c, first);
  } else if (lg == 1) {
    wide_combine_segments<L, O16, ONE, 1>(c, first);
  } else {
    if constexpr (kIdChunk<L> > 4) {
      if (lg == 2) return wide_combine_segments<L, O16, ONE, 2>(c, first);
    }
    wide_combine_segments<L, O16, ONE, -1>(c, first);
  }
}

// one kernel per kind (one id per segment: CSR = false; ragged), lane width and output size
template <bool CSR, int L, bool O16>
__global__ __launch_bounds__(kBlock) void quant8_wide_fwd_kernel(const WideArgs a) {
  const int b = (int)blockIdx.x;
  const int ci = column_of(a.tile_start, a.n_cols, b, lane_id());
  const int64_t tile = b - a.tile_start[ci];
  const WideCol& c = a.col[ci];
  const int wave = (int)(threadIdx.x >> 6);
  const int rpi = kWave >> c.lpr_log2;
  const int64_t first = (tile * kWaves + wave) * (int64_t)((CSR ? kWideSegIters : kWideU) * rpi);
  if (first >= c.n_seg) return;
  if constexpr (CSR) {
    c.one_load ? wide_combine_by_lanes<L, O16, true>(c, first) : wide_combine_by_lanes<L, O16, false>(c, first);
  } else {
    c.one_load ? wide_gather_rows<L, O16, true>(c, first) : wide_gather_rows<L, O16, false>(c, first);
  }
}

template <bool CSR, bool O16>
void launch_wide(int lane_codes, const WideArgs& a, unsigned tiles, hipStream_t stream) {
  if (lane_codes == 8) {
    hipLaunchKernelGGL((quant8_wide_fwd_kernel<CSR, 8, O16>), dim3(tiles), dim3(kBlock), 0, stream, a);
  } else {
    hipLaunchKernelGGL((quant8_wide_fwd_kernel<CSR, 16, O16>), dim3(tiles), dim3(kBlock), 0, stream, a);
  }
}

inline int32_t round_up4(int32_t d) { return (d + 3) & ~3; }
inline int esize_of(const hbk_quant8_lookup_column_t& h) { return h.out_dtype != HBK_QUANT8_OUT_FP32 ? 2 : 4; }
inline int32_t pitch_of(const hbk_quant8_lookup_column_t& h) { return h.pitch == 0 ? round_up4(h.dim) + 4 : h.pitch; }

// the codes a lane of this column moves when the call asks for `want` (8 or 16; 0 or 4: hbk_quant8_lookup_fwd's rule)
int lane_codes_of(const hbk_quant8_lookup_column_t& h, int want) {
  const uintptr_t esize = (uintptr_t)esize_of(h);
  const uintptr_t out_bits = (uintptr_t)h.out | ((uintptr_t)(uint32_t)h.out_stride * esize);
  if (want >= 8 && h.dim % want == 0 && h.dim <= 256 && out_bits % 16 == 0) return want;
  return h.dim % 4 == 0 && out_bits % (4 * esize) == 0 ? 4 : 1;
}

int quant8_lookup_fwd_wide(int32_t n_cols, const hbk_quant8_lookup_column_t* cols, int32_t lane_codes,
                           hbk_stream_t stream_) {
  static const char* kWho = "quant8_lookup_fwd_wide";
  HBK_REQUIRE(n_cols >= 0, "%s: n_cols must be >= 0, got %d", kWho, n_cols);
  HBK_REQUIRE(n_cols == 0 || cols != nullptr, "%s: cols is NULL", kWho);
  HBK_REQUIRE(lane_codes == 8 || lane_codes == 16, "%s: lane_codes must be 8 or 16, got %d", kWho, lane_codes);
  // every column is checked and classified before the first launch: hbk_quant8_lookup_fwd's checks, so that the
  // columns handed on to it cannot be refused behind the wide launches
  std::vector<int> width((size_t)std::max(n_cols, 1));   // 0: nothing to do (no segments)
  std::vector<hbk_quant8_lookup_column_t> narrow;
  for (int32_t c = 0; c < n_cols; ++c) {
    const hbk_quant8_lookup_column_t& h = cols[c];
    HBK_REQUIRE(h.dim >= 1 && h.dim <= 256, "%s: column %d: dim must be in [1, %d], got %d", kWho, c, 256, h.dim);
    const int32_t dim4 = round_up4(h.dim), pitch = pitch_of(h);
    HBK_REQUIRE(pitch % 4 == 0 && pitch >= dim4 + 4,
                "%s: column %d: pitch %d must be a multiple of 4 and >= round_up(dim, 4) + 4 = %d", kWho, c, pitch,
                dim4 + 4);
    HBK_REQUIRE(((uintptr_t)h.table & 3) == 0, "%s: column %d: table must be 4-byte aligned", kWho, c);
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
    HBK_REQUIRE(h.chunk_elems == 0, "%s: column %d: chunk_elems must be 0 (lane_codes sets the width), got %d", kWho,
                c, h.chunk_elems);
    HBK_REQUIRE(h.row_splits != nullptr || h.n_segments == h.n_ids,
                "%s: column %d: n_segments (%lld) must equal n_ids (%lld) when row_splits is NULL", kWho, c,
                (long long)h.n_segments, (long long)h.n_ids);
    HBK_REQUIRE(h.n_ids < (1ll << 31) && h.n_segments < (1ll << 31),
                "%s: column %d: more than 2^31-1 ids/segments", kWho, c);
    HBK_REQUIRE(h.out_stride == 0 || h.out_stride >= h.dim, "%s: column %d: out_stride %d is smaller than dim %d",
                kWho, c, h.out_stride, h.dim);
    HBK_REQUIRE(((uintptr_t)h.out & (uintptr_t)(esize_of(h) - 1)) == 0,
                "%s: column %d: out must be aligned to its element", kWho, c);
    width[(size_t)c] = 0;
    if (h.n_segments == 0) continue;
    HBK_REQUIRE(h.table != nullptr || h.rows == 0, "%s: column %d: table is NULL", kWho, c);
    HBK_REQUIRE(h.out != nullptr, "%s: column %d: out is NULL", kWho, c);
    HBK_REQUIRE(h.ids != nullptr || h.n_ids == 0, "%s: column %d: ids is NULL", kWho, c);
    const int w = lane_codes_of(h, lane_codes);
    HBK_REQUIRE(h.dim <= (w >= 4 ? 256 : 64),
                "%s: column %d: dim %d: at most 256 when dim %% 4 == 0 and out and its stride are 16-byte (fp32) or "
                "8-byte (16-bit) aligned, 64 otherwise", kWho, c, h.dim);
    width[(size_t)c] = w;
    if (w < 8) narrow.push_back(h);
  }
  hipStream_t stream = as_stream(stream_);
  for (int kind = 0; kind < 4; ++kind) {
    const bool csr = (kind & 1) != 0, o16 = (kind & 2) != 0;
    int32_t c0 = 0;
    while (c0 < n_cols) {
      WideArgs args;
      int32_t k = 0;
      int64_t tiles = 0;
      args.tile_start[0] = 0;
      for (; c0 < n_cols && k < kMaxCols; ++c0) {
        const hbk_quant8_lookup_column_t& h = cols[c0];
        if (width[(size_t)c0] < 8 || (h.row_splits != nullptr) != csr || (h.out_dtype != HBK_QUANT8_OUT_FP32) != o16) {
          continue;
        }
        WideCol& d = args.col[k];
        d.table = static_cast<const uint8_t*>(h.table);
        d.ids = h.ids;
        d.splits = h.row_splits;
        d.weights = h.id_weights;
        d.out = h.out;
        d.n_seg = h.n_segments;
        d.map = make_idmap(h.bucket, h.divisor, h.rows);
        d.dim4 = round_up4(h.dim);
        d.pitch = pitch_of(h);
        d.chunks = h.dim / lane_codes;
        d.out_stride = h.out_stride > 0 ? h.out_stride : h.dim;
        d.lpr_log2 = (uint8_t)ceil_log2_u32((uint32_t)d.chunks);
        d.ids64 = h.ids_dtype == HBK_INT64;
        d.combiner = (uint8_t)h.combiner;
        d.out_bf16 = h.out_dtype == HBK_LOWP_BF16;
        d.one_load = (((uintptr_t)h.table | (uintptr_t)(uint32_t)d.pitch) % (uintptr_t)lane_codes) == 0;
        const int64_t rpi = kWave >> d.lpr_log2;
        const int64_t per_block = kWaves * rpi * (csr ? kWideSegIters : kWideU);
        tiles += (h.n_segments + per_block - 1) / per_block;
        HBK_REQUIRE(tiles < (1ll << 31), "%s: grid too large", kWho);
        args.tile_start[++k] = (int32_t)tiles;
      }
      if (k == 0) continue;
      args.n_cols = k;
      if (csr) {
        o16 ? launch_wide<true, true>(lane_codes, args, (unsigned)tiles, stream)
            : launch_wide<true, false>(lane_codes, args, (unsigned)tiles, stream);
      } else {
        o16 ? launch_wide<false, true>(lane_codes, args, (unsigned)tiles, stream)
            : launch_wide<false, false>(lane_codes, args, (unsigned)tiles, stream);
      }
      HBK_HIP_OK(hipGetLastError());
    }
  }
  // the columns that cannot take the width: the narrow forward, behind the wide launches
  if (!narrow.empty()) return hbk_quant8_lookup_fwd((int32_t)narrow.size(), narrow.data(), stream_);
  return HBK_OK;
}

}  // namespace
}  // namespace hbk

extern "C" int hbk_quant8_lookup_fwd_wide(int32_t n_cols, const hbk_quant8_lookup_column_t* cols, int32_t lane_codes,
                                          hbk_stream_t stream) {
  return hbk::quant8_lookup_fwd_wide(n_cols, cols, lane_codes, stream);
}

extern "C" int32_t hbk_quant8_lookup_lane_codes(const hbk_quant8_lookup_column_t* col, int32_t lane_codes) {
  if (col == nullptr || !(lane_codes == 0 || lane_codes == 4 || lane_codes == 8 || lane_codes == 16)) return 0;
  return hbk::lane_codes_of(*col, lane_codes);
}
