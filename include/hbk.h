/*
 * hbk.h -- C ABI of libhbk_core.so: the MI355X (gfx950) sharded-embedding engine that
 * sits behind HybridBackend's TensorFlow custom-op surface.
 *
 * This is the drop-in boundary (DESIGN.md "Boundary").  Every entry point replaces the
 * device side of one reference op family; the citation after each declaration is the
 * reference interface it stands in for (paths relative to the reference tree,
 * hbtf/ = hybridbackend/tensorflow/).  INTEGRATION.md shows the REGISTER_OP /
 * REGISTER_KERNEL_BUILDER shim a maintainer adds on the TensorFlow side.
 *
 * Conventions (mirroring the reference's):
 *   - extern "C", plain pointers and sizes; no TF / torch / HIP types in signatures.
 *     `hbk_stream_t` is a hipStream_t passed as void* (NULL = the default stream).
 *   - The caller owns every buffer (TF: ctx->allocate_output / allocate_temp); the
 *     library never frees caller memory.  Scratch is a caller-provided workspace whose
 *     size comes from the matching hbk_*_workspace_bytes() query.
 *   - All device work is enqueued on the given stream and returns without a host
 *     sync unless the entry point's comment says otherwise.
 *   - Return value: 0 (HBK_OK) or a TensorFlow error code (the reference maps
 *     CUDA/NCCL failures to errors::Internal and shape violations to
 *     errors::InvalidArgument: hbtf/common/host_functions.h:37-42,
 *     hbtf/distribute/partition/partition_by_modulo_ops.cc:81-83).
 *     hbk_last_error() returns the calling thread's last message.  Never throws.
 *   - Re-entrant: compute entry points keep no global mutable state.  One communicator
 *     is one ordered queue; the caller issues collective calls in the same order on
 *     every rank (the reference guarantees this with graph linearisation,
 *     hbtf/graph/common/linearization.cc:42-82).
 */
#ifndef HBK_H_
#define HBK_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* hbk_stream_t;

/* status = TensorFlow error codes */
#define HBK_OK 0
#define HBK_INVALID_ARGUMENT 3
#define HBK_UNIMPLEMENTED 12
#define HBK_INTERNAL 13

/* dtypes: the list HbNcclAlltoallv accepts (hbtf/distribute/nccl/types.h:59-67) */
#define HBK_INT8 0
#define HBK_UINT8 1
#define HBK_INT32 2
#define HBK_UINT32 3
#define HBK_INT64 4
#define HBK_UINT64 5
#define HBK_HALF 6
#define HBK_FLOAT 7
#define HBK_DOUBLE 8

/* combiner of tf.nn.embedding_lookup_sparse (None => mean) */
#define HBK_COMBINER_SUM 0
#define HBK_COMBINER_MEAN 1
#define HBK_COMBINER_SQRTN 2

/* hbtf/distribute/ops.py:34-39, hbtf/distribute/collective.h:52-56 */
#define HBK_TOPOLOGY_ALL 0
#define HBK_TOPOLOGY_INTRA_NODE 1
#define HBK_TOPOLOGY_INTER_NODE 2

const char* hbk_last_error(void);
/* "hbk <version> gfx950"; "hbk 0.2.0 gfx950" since the lookup column structs end in id_weights */
const char* hbk_version(void);

/* Table memory (optional; tables stay caller-owned): one slab for N tables, each at a 2 MB-aligned
 * offset -- the policy that was fastest in every run of tools/placement_probe
 * (profiles/r05_placement.txt).  hbk_tables_layout only computes the offsets (returns the slab size)
 * for callers that carve their own memory (a TF allocator, torch); hbk_tables_alloc does it with
 * hipMalloc; hbk_tables_free releases the slab. */
size_t hbk_tables_layout(int32_t n, const size_t* bytes, size_t* offsets);
int hbk_tables_alloc(int32_t n, const size_t* bytes, void** tables, void** slab);
int hbk_tables_free(void* slab);
/* Tuning / diagnostic options of the library, process wide.  Defaults come from the environment
 * once, when the library is first used (HBK_BWD_LOG2P, HBK_BWD_TARGET, HBK_BWD_SPLIT,
 * HBK_BWD_ONEPASS, HBK_BWD_GROUP_COLS, HBK_UNIQUE_LOG2P, HBK_UNIQUE_ONEPASS, HBK_PART_SUB, HBK_PART_FIXED,
 * HBK_PART_ONEPASS, HBK_SHARDED_GROUPS, HBK_SHARDED_ID64, HBK_SHARDED_COPY_SELF,
 * HBK_SHARDED_TRACE); no entry point reads the environment per call.
 * Names: bwd_buckets_log2, bwd_bucket_pairs, bwd_split_pairs, bwd_onepass, bwd_group_cols, bwd_dense, bwd_wide, bwd_xcd, fwd_xcd, fwd_interleave, fwd_hot_rows,
 * bwd_deterministic (1 or 2: the duplicate-row reduction sums every row's terms in ID ORDER by one lane group, so IndexedSlices and stepped
 * tables are bit-identical from run to run and equal to the sequential fp32 sum (TF's CPU UnsortedSegmentSum), and rows leave ascending;
 * 1: columns whose row range fits the row-sorted jobs take those jobs' in-order form -- a row's pairs ordered by gradient row inside the
 * job, output ranges in bucket order, no bucket split over workgroups -- and the other columns the sort of 2; 2: a stable sort of the
 * batch's (row, gradient row) pairs and a sequential walk for every column; the reproducibility mode, TF_DETERMINISTIC_OPS' analogue),
 * bwd_pairs_packed, bwd_seg_inline, bwd_scale_fused, bwd_simple (0: the general instantiation of the grouping kernels for every launch group), fwd_d16 (0: the general gather for columns of 16 floats too), bwd_weights_lds (0: the weight gradient's segments of more than LPR ids all take the second sweep in memory), bwd_scatter_staged, bwd_rowsort_pos, bwd_rowsort_ratio (round 5: x 4 for dim <= 32),
 * bwd_streams (launch groups of > 64 columns rotate over this many library streams; 0: the caller's), bwd_large_first,
 * bwd_trace (the launch groups of every backward call on stderr), bwd_lds_pad (a probe), sharded_p2p,
 * sharded_p2p_test_refuse (test hook: the rank whose hbk_sharded_p2p_bind behaves as if a peer's memory could not be mapped),
 * unique_buckets_log2,
 * unique_onepass, partition_sub_tiles (held to 8), partition_fixed_max (held to 64, the lanes of a wave), partition_onepass, sharded_groups,
 * sharded_id64, sharded_copy_self, sharded_trace, sharded_inline, sharded_wire_fused, sharded_pack_early (the sharded_* ones are taken by
 * hbk_sharded_create), sync_wait_ms, sync_onepass_off, sync_test_withhold.
 * *_onepass (default 1): small calls of partition / unique / the backward group their ids in ONE
 * launch whose tiles wait for each other; 0 keeps the multi-launch forms.  The
 * waits are bounded (sync_wait_ms, default 2000).  A launch that gave up (never seen outside the
 * test hook sync_test_withhold) poisons its call: the call's later kernels leave without touching
 * anything, its outputs are not valid, and the failure is reported ONCE as HBK_INTERNAL -- by the
 * sharded step in the call that suffered it (it synchronises anyway), else by the next call of
 * these entries ON THE SAME STREAM or by hbk_sync_check[_stream]() -- after which the library takes the multi-launch forms
 * (sync_onepass_off = 1; writable).  The one-launch forms are also not taken when the device
 * cannot hold a whole column's workgroups at once (partitioned modes, small devices; a CU mask set
 * on one stream is not seen by the occupancy query -- there the bounded wait applies).  The words the
 * tiles poll live in buffers the library keeps per (device, stream): calls that share a stream
 * are ordered, which is all these entries ask of the caller. */
int hbk_set_option(const char* name, int32_t value);
int hbk_get_option(const char* name, int32_t* value);
/* HBK_OK, or once per timed-out one-launch wait HBK_INTERNAL (see above).  Callers that read
 * the outputs of hbk_partition_* / hbk_unique_n / hbk_group_lookup_bwd* after their own stream
 * synchronisation call this behind it to learn of a failed call before using its outputs. */
int hbk_sync_check(void);
/* The same for ONE stream of the current device (round 5): the status word of a timed-out wait is
 * kept per (device, stream) -- the stream the failed call was made on -- so a failure on stream A
 * is reported to the next entry call on A (or to this function with A) and is neither seen nor
 * consumed by calls on stream B.  hbk_sync_check() above reports -- and clears -- whatever any
 * stream has raised.
 * Key semantics: a status word (one 64-byte line of pinned memory) and the poll buffers belong to
 * the PAIR (device, hipStream_t value) and live as long as the process: the library cannot see a
 * stream being destroyed.  A new stream that the runtime gives the handle value of a destroyed one
 * inherits that key -- including a failure the destroyed stream never had reported -- so a caller
 * that destroys streams calls hbk_sync_check_stream(stream) (or hbk_sync_check()) before
 * hipStreamDestroy; frameworks with a fixed set of compute streams (TensorFlow, torch) never get
 * there.  The stream to name is the one the failed ENTRY CALL was made on: work the library put on
 * its own helper streams (the backward's launch groups, the sharded plan's prefetch) reports to
 * that caller stream, and asking with any other stream reports nothing. */
int hbk_sync_check_stream(hbk_stream_t stream);
/* the kernels' divide-free floor-mod / floor-div (multiply-high by a
 * host-computed magic) evaluated on the host, so the integer arithmetic can be checked
 * against Python's % and // without a GPU.  d > 0. */
int64_t hbk_host_floormod_i64(int64_t v, int64_t d);
uint64_t hbk_host_fastdiv_u64(uint64_t n, uint64_t d);
/* the block -> work item mapping of the XCD-aware launches (every XCD takes one contiguous range
 * of a launch's work items; block b is observed to run on XCD b % 8), evaluated on the host: a
 * bijection of [0, n_blocks) for every n_blocks. */
int32_t hbk_host_xcd_contiguous(int32_t block, int32_t n_blocks);
/* CRC-32C (Castagnoli) of n host bytes, continuing from crc (0 starts a message): the checksum
 * of TensorFlow's tensor-bundle checkpoints (per tensor and per index block), for the host-side
 * reader / writer of that format (hybridbackend_amd/training/tf_bundle.py; the reference saves
 * through TF's bundle writer, hbtf/training/saver.py:97-185).  "123456789" -> 0xe3069283. */
uint32_t hbk_host_crc32c(uint32_t crc, const void* data, int64_t n);

/* ------------------------------------------------------------------------------------
 * R1  bucketize `feature % embedding_size` (TF FloorMod), N columns in one launch.
 *     docs/tutorial/ranking/data.py:179,186.  dtype HBK_INT32 | HBK_INT64.
 *     out may alias in.  buckets[c] > 0. */
int hbk_floormod_n(int32_t n_cols, int32_t dtype, const void* const* inputs,
                   const int64_t* lens, const int64_t* buckets, void* const* outputs,
                   hbk_stream_t stream);

/* ------------------------------------------------------------------------------------
 * R2  HbPartitionByModulo / HbPartitionByModuloN
 *     ops: hbtf/distribute/partition/partition_by_modulo_ops.cc:46-60, :124-143
 *     semantics = the CPU functor (STABLE counting sort), partition_by_modulo_functors.cc:39-70:
 *       shard = ((v % P) + P) % P;  outputs[c] = ids grouped by shard, input order kept
 *       inside a shard;  sizes[c][p] = count;  indices[c][i] = position of inputs[c][i]
 *       in outputs[c]  (so outputs[c][indices[c]] == inputs[c]).
 *     dtype: HBK_INT32 | HBK_INT64 | HBK_UINT32 | HBK_UINT64.  n_cols = 1 covers the
 *     non-N op.  lens[c] < 2^31 (indices are int32, as in the reference).
 *     1 <= num_partitions <= 16384. */
size_t hbk_partition_workspace_bytes(int32_t n_cols, const int64_t* lens,
                                     int32_t num_partitions);
int hbk_partition_by_modulo_n(int32_t n_cols, int32_t dtype, int32_t num_partitions,
                              const void* const* inputs, const int64_t* lens,
                              void* const* outputs, int32_t* const* sizes,
                              int32_t* const* indices, void* workspace,
                              size_t workspace_bytes, hbk_stream_t stream);

/* R3  HbPartitionByDualModuloStage{One,Two}[N]
 *     ops: hbtf/distribute/partition/partition_by_dual_modulo_ops.cc:46-61,132-147,184-204,278-298
 *     functor: partition_by_dual_modulo_functors.cc:37-91
 *       pre = ((v % (P*M)) + P*M) % (P*M);  stage 1: shard = pre % P;  stage 2: shard = pre / M
 *     stage is 1 or 2; modulus >= 1. */
int hbk_partition_by_dual_modulo_n(int32_t n_cols, int32_t dtype, int32_t num_partitions,
                                   int32_t modulus, int32_t stage,
                                   const void* const* inputs, const int64_t* lens,
                                   void* const* outputs, int32_t* const* sizes,
                                   int32_t* const* indices, void* workspace,
                                   size_t workspace_bytes, hbk_stream_t stream);
/* Host-memory twins (all buffers in host memory, no workspace, no stream): the CPU kernels of
 * the non-N ops, which the reference registers for DEVICE_CPU
 * (partition_by_modulo_ops.cc:62-101, partition_by_dual_modulo_ops.cc:62-130; the N-ary CPU form
 * is Unimplemented there, partition_by_modulo_functors.cc:84-85 -- here it simply loops).  Same
 * results as the device entries, bit for bit. */
int hbk_partition_by_modulo_host(int32_t n_cols, int32_t dtype, int32_t num_partitions,
                                 const void* const* inputs, const int64_t* lens,
                                 void* const* outputs, int32_t* const* sizes,
                                 int32_t* const* indices);
int hbk_partition_by_dual_modulo_host(int32_t n_cols, int32_t dtype, int32_t num_partitions,
                                      int32_t modulus, int32_t stage,
                                      const void* const* inputs, const int64_t* lens,
                                      void* const* outputs, int32_t* const* sizes,
                                      int32_t* const* indices);

/* ------------------------------------------------------------------------------------
 * R6  fp32 <-> fp16 wire casts, N tensors in one launch.
 *     hbtf/common/cast.h:40-54, cast.cu.cc:37-42,60-65,84-95,287 (functor::Cast / CastN).
 *     (src,dst) = (HBK_FLOAT,HBK_HALF) round-to-nearest-even, or (HBK_HALF,HBK_FLOAT). */
int hbk_cast_n(int32_t n, int32_t src_dtype, int32_t dst_dtype, const void* const* inputs,
               const int64_t* lens, void* const* outputs, hbk_stream_t stream);

/* ------------------------------------------------------------------------------------
 * R7  owner-side unique (TF `array_ops.unique`, hbtf/embedding/sharding.py:186):
 *     unique_out[c] = distinct ids in FIRST-OCCURRENCE order, index_out[c][i] = position of
 *     inputs[c][i] in unique_out[c], n_unique[c] (device int32) = number of distinct ids.
 *     ids int64.  unique_out[c] has capacity lens[c]. */
size_t hbk_unique_workspace_bytes(int32_t n_cols, const int64_t* lens);
int hbk_unique_n(int32_t n_cols, const int64_t* const* inputs, const int64_t* lens,
                 int64_t* const* unique_out, int32_t* const* index_out,
                 int32_t* const* n_unique, void* workspace, size_t workspace_bytes,
                 hbk_stream_t stream);

/* ------------------------------------------------------------------------------------
 * R1+R7+R8+R9 fused:  HbGroupLookup (new, additive op; N-ary conventions of the
 * reference's Hb...N ops so Pack-style grouping can target it).  Per column c
 *     row(j)   = ids[j]                       (bucket == 0)
 *              = floormod(ids[j], bucket)     (bucket  > 0)            -- R1
 *     row(j)   = row(j) / divisor             (owner-side `// W`, sharding.py:189)
 *     out[s,:] = combine_{j in [row_splits[s], row_splits[s+1])} table[row(j), :]
 *   row_splits == NULL means one id per segment (Criteo scalar columns; the combiner is
 *   then the identity and out = table[row(ids)]).  Rows outside [0, rows) contribute
 *   zeros (TF GPU GatherV2 behaviour).  The unique/restore pair of the reference
 *   (sharding.py:186,193) is value-transparent in the forward and is not materialised.
 *   replaces: tf.nn.embedding_lookup_sparse as patched by
 *   hbtf/embedding/sharding.py:171-205 (local part) and docs/tutorial/ranking/data.py:179-193.
 *   fp32 tables, fixed in-order accumulation over j.                                   */
typedef struct {
  const float* table;        /* device [rows, dim] row-major */
  int64_t rows;
  int32_t dim;
  int32_t ids_dtype;         /* HBK_INT32 | HBK_INT64 */
  const void* ids;           /* device [n_ids] */
  int64_t n_ids;
  const int32_t* row_splits; /* device [n_segments + 1] or NULL */
  int64_t n_segments;        /* == n_ids when row_splits == NULL */
  int64_t bucket;            /* 0 = ids are row numbers already */
  int32_t divisor;           /* >= 1 */
  int32_t combiner;          /* HBK_COMBINER_* */
  float* out;                /* device [n_segments, dim] */
  /* optional segmented table (n_runs > 0): logical rows [run_start[k], run_start[k+1]) live
   * at table + run_base[k] floats (run_start[0] = 0).  Lets the stitch of the sharded
   * pipeline read the peer-major exchange buffer in place.  Device arrays [n_runs]. */
  const int64_t* run_start;
  const int64_t* run_base;
  int32_t n_runs;
  /* row stride of `out` in floats; 0 = dim.  Lets N columns write their blocks of one
   * concatenated [segments, sum of dims] tensor (hb.feature_column.DenseFeatures) in place.
   * Rows move in 16-byte chunks when dim % 4 == 0 and table, out and the stride are 16-byte aligned
   * (8 bytes for fp16 rows), else in 4-byte chunks of one lane each, which hold at most 64 floats:
   * a column of dim > 64 whose block is not 16-byte aligned is refused (INVALID_ARGUMENT).
   * DenseFeatures looks such a column up into a tensor of its own and copies it into the block. */
  int32_t out_stride;
  /* 1: skewed ids expected (Zipf heads): wide one-id-per-segment columns (dim >= 64, 16-byte
   * chunks, plain table of < 2^32 rows) go through 256-segment tiles that fetch every row
   * repeated inside a tile once and serve the repeats from LDS (config 4: 239 -> 215 us; on
   * uniform ids the tiles cost 15 %, hence a hint and not the default).  Option fwd_hot_rows = 1
   * sets it for every eligible column.  Other columns ignore it. */
  int32_t hot_rows;
  /* fp16 rows on one side (the embedding exchange's wire format fused into the kernels around
   * it; replaces the reference's separate cast passes, hbtf/common/cast.cu.cc:84-285):
   * HBK_LOOKUP_OUT_HALF: `out` holds fp16 rows (fp32 -> fp16 round to nearest even); one id per
   * segment, plain table.  HBK_LOOKUP_TABLE_HALF: `table` holds fp16 rows (sums stay fp32);
   * segmented tables only (n_runs > 0).  Offsets, strides and run bases count elements. */
  int32_t half_io;
  /* optional output permutation (round 5): segment s is written to row out_slots[s] of `out`
   * instead of row s (device int32 [n_segments]; one id per segment, plain table, fp32 rows).
   * The owner gather of the sharded step's p2p form stores every row straight into its place in
   * the requester's output this way.  NULL: rows in segment order. */
  const int32_t* out_slots;
  /* optional per-id weights (tf.nn.embedding_lookup_sparse's sp_weights; version 0.2.0): device
   * fp32 [n_ids], one weight per id.  NULL: unweighted (the code path and results of 0.1.0).  With
   * weights w_j and rows e_j of the segment's ids, in id order, plain fp32 adds of separately
   * rounded products:
   *   sum:   out[s] = sum_j w_j e_j
   *   mean:  out[s] = (sum_j w_j e_j) / W_s,         W_s = sum_j w_j
   *   sqrtn: out[s] = (sum_j w_j e_j) / sqrtf(Q_s),  Q_s = sum_j w_j * w_j
   * (one id per segment included: mean gives (w e) / w).  Ids whose row falls outside [0, rows)
   * contribute neither term nor weight.  A segment whose divisor W_s / Q_s is 0 (empty, or weights
   * that cancel) gives a ZERO row where TensorFlow divides and gives non-finite values.  Negative
   * weights are legal and nothing is pruned.  Refused with out_slots and HBK_LOOKUP_OUT_HALF (the
   * owner gather of the sharded step is never weighted); hot_rows is ignored. */
  const float* id_weights;
} hbk_lookup_column_t;
#define HBK_LOOKUP_OUT_HALF 1
#define HBK_LOOKUP_TABLE_HALF 2

int hbk_group_lookup_fwd(int32_t n_cols, const hbk_lookup_column_t* cols,
                         hbk_stream_t stream);

/* R10  HbGroupLookupGrad: backward of the above up to the IndexedSlices the optimizer
 *   gets (SparseSegment*Grad -> UnsortedSegmentSum dup-reduction):
 *     unique_rows[c][u]  = the distinct row(j) of the column, in unspecified order   (int64)
 *     grad_rows[c][u,:]  = sum_{j: row(j) == unique_rows[u]} scale(seg(j)) * grad_out[seg(j),:]
 *     n_unique[c]        = u   (device int32; stays on the device, no host sync)
 *   scale = 1 (sum), 1/count (mean), 1/sqrt(count) (sqrtn).  unique_rows / grad_rows have
 *   capacity n_ids; rows >= n_unique are untouched.  Ids that map outside [0, rows) contribute
 *   nothing.  No global atomics on the data path: ids are grouped by a hash of their row and
 *   each group is reduced by one workgroup (LDS hash table of the distinct rows, sums in
 *   registers; a group holding a hot row is split over several workgroups and merged), so the
 *   summation order is not fixed: tolerance 1e-5 relative (option bwd_deterministic fixes it: every
 *   row's terms in id order, bit-equal to the sequential fp32 sum, unique_rows ascending -- see
 *   hbk_set_option).  unique_rows[c][0..u) are DISTINCT
 *   whatever the column holds: a group with more distinct rows than the workgroup's LDS table
 *   takes further passes over its pairs (rows handled in one pass are struck out), so every row
 *   is emitted -- and stepped by the fused optimizer -- exactly once.
 *   apply_lr != 0 additionally performs the sparse SGD update on the shard in the same
 *   pass: table[unique_rows[u],:] -= apply_lr * grad_rows[u,:] (sharded variables skip
 *   cross-rank aggregation, hbtf/training/gradient.py:193-217).  With apply_lr != 0 a column
 *   may pass unique_rows = grad_rows = NULL ("step only"): the rows are stepped where their sums
 *   sit in registers and no IndexedSlices are written (a third of the traffic, and no output range
 *   to claim); n_unique still receives the number of distinct rows.  The workspace query must be
 *   made with the same NULL / non-NULL pointers as the call.                            */
typedef struct {
  float* table;              /* device [rows, dim]; only touched when apply_lr != 0 */
  int64_t rows;
  int32_t dim;
  int32_t ids_dtype;
  const void* ids;
  int64_t n_ids;
  const int32_t* row_splits;
  int64_t n_segments;
  int64_t bucket;
  int32_t divisor;
  int32_t combiner;
  const float* grad_out;     /* device [n_segments, dim] */
  int64_t* unique_rows;      /* device [n_ids] */
  float* grad_rows;          /* device [n_ids, dim] */
  int32_t* n_unique;         /* device [1] */
  /* optional segmented inputs (n_runs > 0; row_splits must be NULL): ids j in
   * [run_start[k], run_start[k+1]) live at ids + run_ids[k] (elements) and their gradient rows
   * at grad_out + run_grads[k] (floats, 16-byte aligned).  Lets the owner side of the sharded
   * backward read the peer-major exchange buffers in place.  Device arrays [n_runs]. */
  const int64_t* run_start;
  const int64_t* run_ids;
  const int64_t* run_grads;
  int32_t n_runs;
  /* row stride of grad_out in floats; 0 = dim, else >= dim.  The 16-byte / 4-byte chunk rule of
   * out_stride holds over grad_out, grad_rows and the stride (and table, accum and table_pitch with a
   * step); the deterministic sort path walks up to 256 floats as 4-byte chunks.  Every column is
   * checked before the call's first launch: a refused call steps and writes nothing. */
  int32_t grad_stride;
  float* accum;              /* Adagrad accumulator [rows, dim] (HBK_APPLY_ADAGRAD), else NULL */
  /* floats between consecutive rows of `table` AND of `accum` (round 6); 0 = dim.  Lets a caller
   * keep weights and accumulator interleaved row by row (table = buf, accum = buf + dim,
   * table_pitch = 2 dim): a dim-16 row's weights and accumulator then share ONE 128-byte line, the
   * Adagrad step fetches it with one request instead of two.  Only the optimizer step reads it
   * (the forward takes contiguous rows): measured on the config-5 shape in DESIGN.md 4.4. */
  int32_t table_pitch;
  /* HBK_GRAD_DETERMINISTIC: this column's rows are summed in id order -- what option
   * bwd_deterministic = 1 does for every column of every call (and the option, when set, still does):
   * the reproducible mode chosen per call instead of per process.  Other bits: 0. */
  int32_t flags;
  /* per-id weights of the forward (hbk_lookup_column_t.id_weights; NULL: unweighted).  The
   * gradient term of id j is  t_j = (grad_out[s] / W_s) * w_j  (mean),  (grad_out[s] / sqrtf(Q_s))
   * * w_j  (sqrtn),  grad_out[s] * w_j  (sum), each a separately rounded fp32 op in that order;
   * the ids of a zero-divisor segment get t_j = 0.  grad_rows[u] sums the t_j of row u (in id
   * order under HBK_GRAD_DETERMINISTIC).  The gradient of the weights themselves is a call of its own,
   * hbk_group_lookup_bwd_weights (below), made before a stepping call.  The call writes
   * every t_j to an [n_ids, dim] fp32 buffer inside the workspace and reduces that as a column of
   * one id per segment with the SUM combiner.  Refused with segmented inputs (n_runs > 0). */
  const float* id_weights;
} hbk_lookup_grad_column_t;
#define HBK_GRAD_DETERMINISTIC 1

size_t hbk_group_lookup_bwd_workspace_bytes(int32_t n_cols,
                                            const hbk_lookup_grad_column_t* cols);
int hbk_group_lookup_bwd(int32_t n_cols, const hbk_lookup_grad_column_t* cols,
                         float apply_lr, void* workspace, size_t workspace_bytes,
                         hbk_stream_t stream);
/* The same with the optimizer named: HBK_APPLY_SGD (above), or HBK_APPLY_ADAGRAD =
 *   accum[row,:] += g * g;  table[row,:] -= apply_lr * g * (1 / sqrt(accum[row,:]))
 * on the deduplicated gradient g of every touched row -- tf.train.AdagradOptimizer's sparse
 * apply, the optimizer of the reference's Taobao tutorials (docs/tutorial/ranking/taobao/
 * train.py:115); cols[c].accum holds the accumulator (initial_accumulator_value filled in by
 * the caller). */
#define HBK_APPLY_SGD 0
#define HBK_APPLY_ADAGRAD 2
int hbk_group_lookup_bwd_apply(int32_t n_cols, const hbk_lookup_grad_column_t* cols,
                               int32_t apply, float apply_lr, void* workspace,
                               size_t workspace_bytes, hbk_stream_t stream);

/* Lazy Adam: tf.contrib.opt.LazyAdamOptimizer's sparse apply (TF 1.15) on the deduplicated gradient
 * g of every distinct row r of the call, each a separately rounded fp32 op in this order:
 *     lr_t = (lr * sqrtf(1 - beta_powers[1])) / (1 - beta_powers[0])
 *     m[r] = beta1 * m[r] + (1 - beta1) * g
 *     v[r] = beta2 * v[r] + (1 - beta2) * (g * g)
 *     w[r] = w[r] - (lr_t * m[r]) / (sqrtf(v[r]) + epsilon)
 * Rows that do not occur are not touched (tf.train.AdamOptimizer's own sparse path decays and moves
 * every row: a full-table pass, not provided).  Two phases: the backward in its emit form
 * (hbk_group_lookup_bwd, apply_lr = 0: every distinct row exactly once, deterministic modes and
 * weights as there), then one apply launch that reads each column's n_unique on the device (no host
 * sync; capturable).  cols[c].table is the weights, m[c] / v[c] the first / second moments, all three
 * with the row pitch cols[c].table_pitch (so [w | m | v | pad] may be interleaved per row);
 * cols[c].accum must be NULL.  unique_rows / grad_rows may both be NULL (step only: they then live in
 * the workspace, which the query sizes from the same pointers).  beta_powers is a device fp32 [2]
 * (beta1^t, beta2^t; start at beta1, beta2), read by the apply; finish != 0 multiplies it by
 * (beta1, beta2) in fp32 after this call's step, in stream order (TF's _finish).  Adam is not
 * additive: no table, m or v may appear twice in one call.  Dims: those the backward takes -- at most
 * 256 when table, m, v, grad_rows and the pitch are 16-byte aligned and dim % 4 == 0 (f32x4 chunks),
 * at most 64 otherwise (scalar chunks); larger dims are refused before any device work.  Detected by
 * the presence of the symbol. */
typedef struct {
  float beta1, beta2, epsilon;
  float* beta_powers;   /* device [2]: beta1^t, beta2^t */
  int32_t finish;       /* != 0: advance beta_powers after this call's step */
} hbk_adam_t;
size_t hbk_group_lookup_bwd_adam_workspace_bytes(int32_t n_cols,
                                                 const hbk_lookup_grad_column_t* cols);
int hbk_group_lookup_bwd_adam(int32_t n_cols, const hbk_lookup_grad_column_t* cols,
                              float* const* m, float* const* v, const hbk_adam_t* adam, float lr,
                              void* workspace, size_t workspace_bytes, hbk_stream_t stream);

/* FTRL-Proximal: TF 1.15 SparseApplyFtrl / SparseApplyFtrlV2 on the deduplicated gradient g of every
 * distinct row r of the call, each a separately rounded fp32 op in this order (a = accum[r],
 * z = linear[r], w = weights[r], the old values):
 *     gs = l2_shrinkage == 0 ? g : g + (2 * l2_shrinkage) * w
 *     na = a + g * g
 *     p(x) = lr_power == -0.5 ? sqrtf(x) : powf(x, -lr_power)
 *     z  = z + (gs - ((p(na) - p(a)) / lr) * w)
 *     y  = p(na) / lr + (2 * l2)
 *     w  = (clamp(z, -l1, l1) - z) / y;   a = na
 * Rows that do not occur are not touched.  The phases, the pitch (cols[c].table_pitch for weights,
 * accum[c] and linear[c]: [w | accum | linear | pad] may be interleaved), step only, the dim limits and
 * the refusal of a table or slot named twice are hbk_group_lookup_bwd_adam's; cols[c].accum must be
 * NULL.  Refused before any device work: lr <= 0 or not finite; l1, l2 or l2_shrinkage < 0 or not
 * finite; lr_power > 0 or not finite.  lr_power = -0.5 (TF's default) runs an instantiation without
 * powf; powf is not correctly rounded, so other powers may differ from a host powf in the last bit.
 * Detected by the presence of the symbol. */
typedef struct {
  float l1, l2, l2_shrinkage, lr_power;
} hbk_ftrl_t;
size_t hbk_group_lookup_bwd_ftrl_workspace_bytes(int32_t n_cols,
                                                 const hbk_lookup_grad_column_t* cols);
int hbk_group_lookup_bwd_ftrl(int32_t n_cols, const hbk_lookup_grad_column_t* cols,
                              float* const* accum, float* const* linear, const hbk_ftrl_t* ftrl,
                              float lr, void* workspace, size_t workspace_bytes, hbk_stream_t stream);

/* Row-wise Adagrad ("exact row-wise Adagrad" of sparse embedding engines): ONE fp32 accumulator per row.
 * For every distinct row r of the call with its deduplicated gradient g[0..dim) (after the clip: g'), each
 * a separately rounded fp32 op in this order:
 *     s    = sum_k g_k * g_k
 *     a'   = a[r] + s / (float)dim
 *     m    = lr / (sqrtf(a') + epsilon)
 *     w_k  = w_k - m * g_k        (every k)
 *     a[r] = a'
 * The order of s is the clip's (hbk_group_lookup_fwd_clipped): the row is split over its lanes (chunks of 4
 * floats when dim % 4 == 0 and table, grad_rows and the pitch are 16-byte aligned, else of 1 float; L = the
 * power of two >= chunks), a lane sums its chunk in element order (((g0 g0 + g1 g1) + g2 g2) + g3 g3), lanes
 * without a chunk give +0, and the L partial sums meet in the butterfly p[i] = p[i] + p[i ^ o], o = 1, 2, 4,
 * .. < L.  accum[c] is a device fp32 [rows, 1], contiguous (word r belongs to row r whatever table_pitch is);
 * being one 4-byte word per row it does not decide the row shape.  Rows that do not occur, rows outside the
 * table and -1 touch nothing.  A row with a' == 0 and epsilon == 0 computes 0 / 0: start the accumulator
 * above 0 or keep epsilon > 0.  The phases (emit-form reduce, then one apply launch per 64 columns that reads
 * n_unique on the device: no host sync, capturable), step only (unique_rows = grad_rows = NULL) and the
 * workspace query are hbk_group_lookup_bwd_adam's.  Refused before any device work (HBK_INVALID_ARGUMENT): a
 * NULL or misaligned accum[c]; accum[c] equal to the table; a table or accumulator named by two columns (the
 * step is not additive); cols[c].accum != NULL; dim > 256 (> 64 as 4-byte chunks); lr 0 or not finite;
 * epsilon < 0 or not finite.  The _clipped pair differentiates through max_norm as the other optimizers'
 * (g' replaces g everywhere, and grad_rows end as g').  Detected by the presence of the symbols; the
 * structs above and the version are those of 0.2.0. */
typedef struct {
  float epsilon;
} hbk_rowwise_adagrad_t;
size_t hbk_group_lookup_bwd_rowwise_adagrad_workspace_bytes(int32_t n_cols,
                                                            const hbk_lookup_grad_column_t* cols);
int hbk_group_lookup_bwd_rowwise_adagrad(int32_t n_cols, const hbk_lookup_grad_column_t* cols,
                                         float* const* accum, const hbk_rowwise_adagrad_t* rowwise_adagrad,
                                         float lr, void* workspace, size_t workspace_bytes,
                                         hbk_stream_t stream);

/* The gradient of the per-id weights (tf.nn.embedding_lookup_sparse is differentiable in
 * sp_weights.values).  grad_weights[c] is a device fp32 [n_ids of column c], or NULL = not wanted;
 * max_norms is NULL or a HOST float[n_cols] as in the clipped entries (0 = not clipped).  Reads
 * cols[c].{table, rows, dim, table_pitch, ids, ids_dtype, n_ids, row_splits, n_segments, bucket, divisor,
 * combiner, grad_out, grad_stride, id_weights} as hbk_group_lookup_bwd does and writes grad_weights only: no
 * workspace, no atomics, one launch per kind of column (ragged or not, 16-byte or 4-byte chunks).  Per id
 * j of segment s, with e_j = table[row(j)] after the column's clip (hbk_group_lookup_fwd_clipped's y), w_j
 * its weight and G_s = grad_out[s]:
 *     d_j = sum_k G_sk * e_jk      A_s = sum_i w_i * d_i      W_s = sum_i w_i      Q_s = sum_i w_i * w_i
 *     sum:    dw_j = d_j
 *     mean:   dw_j = (d_j - A_s / W_s) / W_s
 *     sqrtn:  r = sqrtf(Q_s);  dw_j = d_j / r - (w_j * A_s) / (Q_s * r)
 * each a separately rounded fp32 op in that order.  A_s, W_s and Q_s run over the segment's ids that map
 * inside [0, rows), in id order (A = A + w_i * d_i, ...), as the forward sums its divisor.  The order of
 * d_j: the row is split over its lanes as the clip's s is (chunks of 4 floats when dim % 4 == 0 and table,
 * grad_out, the pitch and the stride are 16-byte aligned, else of 1 float; L = the power of two >= chunks);
 * a lane sums its chunk in element order (((G0 e0 + G1 e1) + G2 e2) + G3 e3), lanes without a chunk give 0,
 * and the L partial sums meet in the butterfly p[i] = p[i] + p[i ^ o], o = 1, 2, 4, .. < L.  Nothing
 * depends on scheduling: two runs give the same bits.  dw_j = 0 for an id that maps outside [0, rows), for
 * the ids of a segment whose divisor (W_s, sqrtf(Q_s)) is 0 and for ids in no segment; every position
 * [0, n_ids) is written.  row_splits = NULL (one id per segment) is legal: A = w d, W = w, Q = w w.  A
 * lane group owns a segment whatever its length (no chunked path: a segment of 10^5 ids is walked by one
 * group); a segment of more than L and at most 8 L ids parks d_j, w_j and the validity in LDS until A_s is
 * known, a longer one writes d_j to grad_weights first and fixes it up in a second sweep over its own ids
 * (the same arithmetic and bits either way; option bwd_weights_lds = 0: the second sweep for both).
 * The rows are read as they are when the call runs: call it BEFORE a stepping backward of the same step,
 * as the clip's gradient reads the rows before the step.  Refused (HBK_INVALID_ARGUMENT) before any
 * launch: segmented inputs (n_runs > 0), a wanted gradient on a column without id_weights, a max_norm
 * that is negative, NaN or infinite, a row the gather cannot take (dim > 256, or > 64 as 4-byte chunks).
 * Detected by the presence of the symbol; the structs and the version are those of 0.2.0. */
int hbk_group_lookup_bwd_weights(int32_t n_cols, const hbk_lookup_grad_column_t* cols,
                                 const float* max_norms, float* const* grad_weights,
                                 hbk_stream_t stream);

/* max_norm: TF 1.15's embedding_lookup[_sparse](..., max_norm=) / embedding_column(max_norm=) -- every
 * gathered row clipped to an L2 norm of at most c before its weight and the combine, and the gradient
 * taken through the clip.  max_norms is a HOST float[n_cols]: 0 = the column is not clipped, c > 0
 * finite = clipped; negative, NaN or infinite values are refused (HBK_INVALID_ARGUMENT) before any
 * launch.  With every value 0 each entry is its unclipped twin, bit for bit.  Detected by the presence
 * of the symbols; the column structs and the version are those of 0.2.0.
 *
 * Forward.  For each gathered fp32 row x of `dim` elements, each a separately rounded fp32 op:
 *     s   = sum_k x_k * x_k
 *     n   = s > 0 ? sqrtf(s) : 0
 *     m   = fmaxf(n, c)
 *     y_k = (x_k * c) / m            (every row, rows inside the ball included)
 * y then replaces x in the weighted / unweighted sum, mean and sqrtn formulas above.  The order of s:
 * the row is split over its lanes as the gather splits it (chunks of 4 floats when dim % 4 == 0 and the
 * buffers are 16-byte aligned, else of 1 float; lanes per row L = the power of two >= chunks); every
 * lane sums its chunk in element order (((x0 x0 + x1 x1) + x2 x2) + x3 x3), lanes without a chunk give
 * 0, then the L partial sums meet in a butterfly: for o = 1, 2, 4, .. < L, p[i] = p[i] + p[i ^ o].
 * The order depends on the row shape only, never on a reduce plan: results are bit-reproducible.
 * Refused for a clipped column: HBK_LOOKUP_TABLE_HALF rows, out_slots.  HBK_LOOKUP_OUT_HALF clips in
 * fp32, then rounds.  hot_rows is ignored for clipped columns.
 * Consequence: with c a power of two and every row norm < c (zero rows included), y == x bit for bit. */
int hbk_group_lookup_fwd_clipped(int32_t n_cols, const hbk_lookup_column_t* cols,
                                 const float* max_norms, hbk_stream_t stream);
/* Backward through the clip.  TF clips every DISTINCT row once, so the Jacobian applies to the row's
 * summed gradient G (grad_rows of the unclipped backward: weights, combiner scale and the
 * deterministic modes included), with x = the table row BEFORE this call's step:
 *     if s > 0 and n >= c:    (the tie n == c included: TF's Maximum gradient uses >=)
 *         d    = sum_k G_k * ((x_k * c) / m) / m
 *         ds   = (-d * 0.5f) / n
 *         g'_k = (G_k / m) * c + (2 * ds) * x_k
 *     else:
 *         g'_k = (G_k / m) * c
 * Every term of d, G_k * ((x_k * c) / m) / m, is rounded on its own; the terms are then summed in the
 * order of the forward's s (per lane in element order, then the butterfly), over the row shape of the
 * step (the table, the accumulator or slots, grad_rows and the pitch decide 4-float chunks).  Every
 * optimizer steps with g'.
 * Two phases: the clipped columns' backward in its emit form (into grad_rows, or for step-only columns
 * into workspace slices), then one clip pass per 64 columns that reads x, forms g' and steps the row
 * (SGD / Adagrad with the fused step's arithmetic, Lazy Adam, FTRL).  In every form grad_rows of a
 * clipped column end as g', the gradient its rows were stepped with (G for unclipped columns).
 * Unclipped columns of hbk_group_lookup_bwd_apply_clipped keep the fused route of
 * hbk_group_lookup_bwd_apply (their bits are that call's); in the Adam / FTRL entries every column
 * runs the two phases as in the unclipped entries.  Refused before any launch: a clipped column whose
 * table is named by another column (table or accum) of a stepping call (the clip must see the pre-step
 * row; the emit form may repeat tables); a clipped column without a table.  Workspace: the matching
 * query, made with the same pointers and max_norms. */
size_t hbk_group_lookup_bwd_apply_clipped_workspace_bytes(int32_t n_cols,
                                                          const hbk_lookup_grad_column_t* cols,
                                                          const float* max_norms);
int hbk_group_lookup_bwd_apply_clipped(int32_t n_cols, const hbk_lookup_grad_column_t* cols,
                                       const float* max_norms, int32_t apply, float apply_lr,
                                       void* workspace, size_t workspace_bytes, hbk_stream_t stream);
size_t hbk_group_lookup_bwd_adam_clipped_workspace_bytes(int32_t n_cols,
                                                         const hbk_lookup_grad_column_t* cols,
                                                         const float* max_norms);
int hbk_group_lookup_bwd_adam_clipped(int32_t n_cols, const hbk_lookup_grad_column_t* cols,
                                      const float* max_norms, float* const* m, float* const* v,
                                      const hbk_adam_t* adam, float lr, void* workspace,
                                      size_t workspace_bytes, hbk_stream_t stream);
size_t hbk_group_lookup_bwd_ftrl_clipped_workspace_bytes(int32_t n_cols,
                                                         const hbk_lookup_grad_column_t* cols,
                                                         const float* max_norms);
int hbk_group_lookup_bwd_ftrl_clipped(int32_t n_cols, const hbk_lookup_grad_column_t* cols,
                                      const float* max_norms, float* const* accum,
                                      float* const* linear, const hbk_ftrl_t* ftrl, float lr,
                                      void* workspace, size_t workspace_bytes, hbk_stream_t stream);
size_t hbk_group_lookup_bwd_rowwise_adagrad_clipped_workspace_bytes(int32_t n_cols,
                                                                    const hbk_lookup_grad_column_t* cols,
                                                                    const float* max_norms);
int hbk_group_lookup_bwd_rowwise_adagrad_clipped(int32_t n_cols, const hbk_lookup_grad_column_t* cols,
                                                 const float* max_norms, float* const* accum,
                                                 const hbk_rowwise_adagrad_t* rowwise_adagrad, float lr,
                                                 void* workspace, size_t workspace_bytes,
                                                 hbk_stream_t stream);

/* The optimizer step on IndexedSlices the CALLER holds: what the second phase of the entries above does,
 * without the reduce in front of it.  For every u < n_unique[0] (read on the device, clamped to
 * [0, capacity]; entries at or after it are not read) with r = unique_rows[u] inside [0, rows), row r of the
 * table and of its slots is stepped with g = grad_rows[u, :]; any other entry (-1 included) touches nothing, so
 * slices may have holes.  The rows must be DISTINCT: no step but SGD's is additive, and a row named twice
 * races.  This is documented, not checked.  `apply` names the rule, and formulas, rounding and operation
 * order are exactly those of the entry it belongs to:
 *     HBK_APPLY_SGD              table -= lr * g                                   (hbk_group_lookup_bwd_apply)
 *     HBK_APPLY_ADAGRAD          slot0 = the accumulator                           (hbk_group_lookup_bwd_apply)
 *     HBK_APPLY_LAZY_ADAM        slot0 = m, slot1 = v, params = hbk_adam_t         (hbk_group_lookup_bwd_adam)
 *     HBK_APPLY_FTRL             slot0 = accum, slot1 = linear, params = hbk_ftrl_t (hbk_group_lookup_bwd_ftrl)
 *     HBK_APPLY_ROWWISE_ADAGRAD  slot0 = accum [rows, 1], params = hbk_rowwise_adagrad_t
 *                                                                       (hbk_group_lookup_bwd_rowwise_adagrad)
 * slot0 / slot1 are arrays of n_cols device pointers (NULL where the rule has no such slot), params is NULL
 * for SGD and Adagrad.  Table and table-shaped slots share table_pitch (0 = dim).  hbk_adam_t.finish advances
 * the beta powers after the step, in stream order, also with n_cols == 0.  The gradient is not clipped.
 * One launch per 64 columns, no workspace, no host read of device memory: the call can be captured.  Refused
 * before the first launch (HBK_INVALID_ARGUMENT): an unknown rule; a NULL table, unique_rows, grad_rows,
 * n_unique or needed slot of a column with capacity > 0; capacity < 0 or >= 2^30; dim < 1, or > 256 (> 64
 * unless dim % 4 == 0 and table, slots, grad_rows and the pitch are 16-byte aligned); a table or slot named
 * twice; the hyperparameters and the lr the rule's own entry refuses (lr == 0 for every rule; a non-finite lr
 * but for Lazy Adam; FTRL: lr <= 0).  Detected by the presence of the symbol; the structs above and the
 * version are those of 0.2.0. */
#define HBK_APPLY_LAZY_ADAM 3
#define HBK_APPLY_FTRL 4
#define HBK_APPLY_ROWWISE_ADAGRAD 5
typedef struct {
  float* table;                /* device [rows, dim], table_pitch floats between rows */
  int64_t rows;
  int32_t dim;
  int32_t table_pitch;         /* 0 = dim */
  const int64_t* unique_rows;  /* device [capacity] */
  const float* grad_rows;      /* device [capacity, dim], contiguous */
  const int32_t* n_unique;     /* device [1] */
  int64_t capacity;
} hbk_slices_column_t;
int hbk_sparse_apply_slices_n(int32_t n_cols, const hbk_slices_column_t* cols, int32_t apply,
                              float* const* slot0, float* const* slot1, const void* params, float lr,
                              hbk_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Low-precision tables: rows stored as bf16 or fp16 (2 bytes per element), every sum and every optimizer
 * slot fp32.  Two entries, both detected by the presence of the symbol (the structs above and the version
 * are those of 0.2.0): a forward of its own and the optimizer step on IndexedSlices the caller holds.  The
 * backward between them is hbk_group_lookup_bwd_apply in its emit form (apply_lr = 0), which never reads the
 * table (hbk_lookup_grad_column_t.table: "only touched when apply_lr != 0") and so serves a table of any
 * element type.  NEVER hand a 16-bit table to an entry that steps (apply_lr != 0, the slot entries,
 * hbk_sparse_apply_slices_n): they read and write `table` as fp32.
 *
 * Element types (hbk_lowp_*_column_t.table_dtype; a call may mix them):
 *     HBK_LOWP_BF16   1 sign, 8 exponent, 7 fraction bits: the upper half of the fp32 pattern
 *     HBK_LOWP_FP16   IEEE binary16
 *   upcast(x) is exact for both: bf16 bits << 16 as an fp32 pattern; (float)(_Float16)x, subnormals included.
 *
 * FORWARD  hbk_lowp_lookup_fwd: per column, with e_j = upcast(table[row(j), :]) and row(j) as in
 *   hbk_group_lookup_fwd (bucket: floormod; divisor; rows outside [0, rows) are zero rows),
 *     row_splits == NULL:                 out[s] = e_s                                  (the combiner is ignored)
 *       with id_weights:   sum   out[s] = w_s e_s
 *                          mean  out[s] = (w_s e_s) / w_s
 *                          sqrtn out[s] = (w_s e_s) / sqrtf(w_s * w_s)
 *                          an invalid row or a zero divisor gives a zero row
 *     row_splits != NULL:  acc = +0; for j in id order: acc = acc + e_j              (n = all ids of the segment)
 *                          sum   out[s] = acc;  mean acc / (float)n;  sqrtn acc / sqrtf((float)n);  n == 0: zeros
 *       with id_weights:   acc = acc + e_j * w_j, W = W + w_j (sqrtn: Q = Q + w_j * w_j), ids of VALID rows only
 *                          sum   out[s] = acc;  mean acc / W;  sqrtn acc / sqrtf(Q);  a zero divisor: zeros
 *   every product and sum a separately rounded fp32 operation.  This is hbk_group_lookup_fwd on the table upcast
 *   to fp32, bit for bit; per-element sums are independent, so the lane layout cannot change a bit.
 *   Rows move as chunks of 4 elements (8 bytes) per lane -- or 8 elements (16 bytes) where dim % 8 == 0 and the
 *   table is 16-byte aligned: by default (chunk_elems = 0) from dim 64 on, with chunk_elems = 8 wherever possible,
 *   with chunk_elems = 4 never -- when dim % 4 == 0, the table is 8-byte aligned and `out` and its stride are
 *   16-byte aligned: dim <= 256.  Otherwise one element per lane: dim <= 64 -- or, with wide_rows = 1 (the field
 *   that was reserved; 0 changes nothing), dim <= 256 here too: such a row is served as column blocks of 64 elements,
 *   each a column of its own to the kernel, 64 columns and blocks per launch; no bit depends on the split.
 *   One launch per 64 columns and kind (one id per segment / ragged), plain loads and stores, no atomics, no
 *   workspace, no host read: the call can be captured.  There is no max_norm, no segmented table, no output
 *   permutation and no fp16 output here.  Refused before the first launch (HBK_INVALID_ARGUMENT, the column
 *   named): an unknown table_dtype, ids_dtype or combiner; chunk_elems not 0, 4 or 8; wide_rows not 0 or 1; dim < 1
 *   or beyond the bounds above; a table at an odd address or an `out` not 4-byte aligned; a NULL table (rows > 0), ids
 *   (n_ids > 0) or out of a column with segments; negative sizes, >= 2^31 ids or segments; bucket < 0;
 *   divisor < 1; out_stride != 0 and < dim; n_segments != n_ids without row_splits.  n_cols == 0 answers OK. */
#define HBK_LOWP_BF16 1
#define HBK_LOWP_FP16 2
typedef struct {
  const void* table;         /* device [rows, dim] of 2-byte elements, contiguous rows */
  int32_t table_dtype;       /* HBK_LOWP_BF16 | HBK_LOWP_FP16 */
  int32_t dim;
  int64_t rows;
  const void* ids;           /* device [n_ids] */
  int32_t ids_dtype;         /* HBK_INT32 | HBK_INT64 */
  int32_t combiner;          /* HBK_COMBINER_* */
  int64_t n_ids;
  const int32_t* row_splits; /* device [n_segments + 1] or NULL */
  int64_t n_segments;        /* == n_ids when row_splits == NULL */
  int64_t bucket;            /* 0 = ids are row numbers already */
  int32_t divisor;           /* >= 1 */
  int32_t out_stride;        /* floats between rows of `out`; 0 = dim */
  float* out;                /* device fp32 [n_segments, dim] */
  const float* id_weights;   /* device fp32 [n_ids] or NULL */
  int32_t chunk_elems;       /* 0 = the default (8 from dim 64 on, else 4); 4 or 8: elements per lane where the column allows it */
  int32_t wide_rows;         /* 0; 1: one-element-per-lane rows up to dim 256, in blocks of 64 (the reserved word) */
} hbk_lowp_lookup_column_t;
int hbk_lowp_lookup_fwd(int32_t n_cols, const hbk_lowp_lookup_column_t* cols, hbk_stream_t stream);

/* APPLY  hbk_lowp_apply_slices_n: the contract of hbk_sparse_apply_slices_n (distinct rows; an entry outside
 *   [0, rows), -1 included, touches nothing; n_unique read on the device and clamped to [0, capacity]; the five
 *   rules; one launch per 64 columns, no workspace, no host read; hbk_adam_t.finish advances the beta powers
 *   behind the step, also with n_cols == 0) on tables of 2-byte elements with contiguous rows.  For a stepped
 *   row r:
 *       w32          = upcast(table[r, :])
 *       (w32', s')   = rule(w32, slots[r], g)      formulas, rounding and operation order of the fp32 entry
 *       slots[r]     = s'                          fp32, stored as the fp32 entry stores them
 *       table[r, :]  = round(w32')
 *   so that with rounding 0 the table equals the fp32 entry's result on upcast(table), cast, bit for bit.
 *   A row is split over lanes as in the fp32 entry: 4 elements per lane when dim % 4 == 0, the table is 8-byte
 *   and the slots and grad_rows are 16-byte aligned (dim <= 256), else one element per lane (dim <= 64).  Row-wise
 *   Adagrad's sum of g * g follows that layout (each lane's chunk in element order, then the butterfly), as there.
 *
 *   round, HBK_LOWP_ROUND_NEAREST (0): round to nearest, ties to even.  bf16, on the fp32 pattern u of w32':
 *       a NaN stays a NaN (0x7FC0 today; the payload is not specified); otherwise
 *       out = (u + 0x7FFF + ((u >> 16) & 1)) >> 16      (infinities stay; a carry out of the largest finite value
 *                                                        gives infinity)
 *     fp16: the (_Float16) conversion.
 *   round, HBK_LOWP_ROUND_STOCHASTIC (1): bf16 only (refused with an fp16 column).
 *       exponent field of u all ones: as NEAREST; otherwise  out = (u + (noise_k & 0xFFFF)) >> 16
 *     (no wrap-around is possible there).  It rounds in magnitude, is unbiased for both signs, and an exactly
 *     representable value never moves.  A carry into the exponent, infinity at the very top included, is
 *     correct behaviour.  noise_k is a pure function of the call's seed, the step counter, the column's index c in
 *     the call, the row r (int64) and the element index k in the row, all arithmetic modulo 2^32:
 *       fmix32(h): h ^= h >> 16; h *= 0x85EBCA6B; h ^= h >> 13; h *= 0xC2B2AE35; h ^= h >> 16   (murmur3's finalizer)
 *       base    = fmix32(seed ^ fmix32(step + 0x9E3779B9 * (c + 1)))
 *       rowh    = fmix32(fmix32(base ^ lo32(r)) ^ hi32(r))
 *       noise_k = fmix32(rowh + 0x9E3779B9 * (k + 1))
 *     step = rounding->step[0], a device uint32 the call reads ON THE DEVICE; with rounding->advance != 0 a
 *     one-thread launch behind the apply adds 1 to it in stream order (also with n_cols == 0), so replays of a
 *     captured graph draw fresh noise and a run is reproducible.  NEAREST never reads or writes the counter.
 *   rounding == NULL means NEAREST.
 *   Refused before the first launch (HBK_INVALID_ARGUMENT): what hbk_sparse_apply_slices_n refuses (an unknown
 *   rule; a NULL table, unique_rows, grad_rows, n_unique or needed slot of a column with capacity > 0;
 *   capacity < 0 or >= 2^30; dim < 1 or beyond the bounds above; a table or slot named twice; lr == 0 and the
 *   hyperparameters the rule's own entry refuses), an unknown table_dtype or rounding mode, a table at an odd
 *   address, STOCHASTIC with an fp16 column, STOCHASTIC with a NULL or misaligned step counter. */
#define HBK_LOWP_ROUND_NEAREST 0
#define HBK_LOWP_ROUND_STOCHASTIC 1
typedef struct {
  void* table;                 /* device [rows, dim] of 2-byte elements, contiguous rows */
  int32_t table_dtype;         /* HBK_LOWP_BF16 | HBK_LOWP_FP16 */
  int32_t dim;
  int64_t rows;
  const int64_t* unique_rows;  /* device [capacity] */
  const float* grad_rows;      /* device fp32 [capacity, dim], contiguous */
  const int32_t* n_unique;     /* device [1] */
  int64_t capacity;
} hbk_lowp_slices_column_t;
typedef struct {
  int32_t mode;                /* HBK_LOWP_ROUND_* */
  uint32_t seed;
  uint32_t* step;              /* device uint32 [1]; STOCHASTIC only */
  int32_t advance;             /* != 0: step[0] += 1 behind the apply (STOCHASTIC only) */
  int32_t reserved;            /* 0 */
} hbk_lowp_rounding_t;
int hbk_lowp_apply_slices_n(int32_t n_cols, const hbk_lowp_slices_column_t* cols, int32_t apply,
                            float* const* slot0, float* const* slot1, const void* params, float lr,
                            const hbk_lowp_rounding_t* rounding, hbk_stream_t stream);

/* The two sides of a 16-bit wire (the sharded step over 16-bit shards, hbk_sharded_set_table_dtypes): rows travel
 * in the table's own 2 bytes per element and are upcast by the requester, so nothing is rounded on the way -- the
 * result stays hbk_group_lookup_fwd over the upcast table, bit for bit, at half the wire bytes.  Both detected by
 * the presence of the symbol; the structs above and the version stay those of 0.2.0.
 *
 * OWNER GATHER  hbk_lowp_gather_rows_n: per column, one id per segment, no weights, no combiner:
 *       out[s, :] = table[row(ids[s]), :]   copied as 16-bit patterns
 *   with row() the id map of hbk_lowp_lookup_fwd (bucket: floormod; divisor; rows).  A row outside [0, rows) gives
 *   0x0000 elements: +0 in bf16 and in fp16, what the upcast forward writes for it.  Nothing is converted, so the
 *   entry does not ask whether the bits are bf16 or fp16 (NaN payloads, infinities, subnormals and -0 arrive as
 *   they are).  out_stride counts ELEMENTS between rows of `out` (0 = dim).
 *   A lane moves 8 elements (16 bytes) when dim % 8 == 0 and table, out and the stride in bytes are 16-byte
 *   aligned, 4 elements (8 bytes) when dim % 4 == 0 and they are 8-byte aligned: dim <= 256; otherwise one element:
 *   dim <= 64.  Ids are read once per wave and handed to a row's lanes by shuffle; a lane issues its 4 independent
 *   row loads before it stores.  One launch per 64 columns and lane width (a call with more columns splits), plain
 *   loads, non-temporal stores, no atomics, no workspace, no host read: capturable.
 *   Refused before the first launch (HBK_INVALID_ARGUMENT, the column named): dim < 1 or beyond the bounds above;
 *   an unknown ids_dtype; negative sizes or >= 2^31 ids; bucket < 0; divisor < 1; out_stride != 0 and < dim; a
 *   table or out at an odd address; a NULL table (rows > 0), ids or out of a column with ids.  n_cols == 0: OK. */
typedef struct {
  const void* table;         /* device [rows, dim] of 2-byte elements, contiguous rows */
  int32_t dim;
  int32_t ids_dtype;         /* HBK_INT32 | HBK_INT64 */
  int64_t rows;
  const void* ids;           /* device [n_ids] */
  int64_t n_ids;
  int64_t bucket;            /* 0 = ids are row numbers already */
  int32_t divisor;           /* >= 1 */
  int32_t out_stride;        /* ELEMENTS between rows of `out`; 0 = dim */
  void* out;                 /* device [n_ids, dim] of 2-byte elements */
} hbk_lowp_gather_column_t;
int hbk_lowp_gather_rows_n(int32_t n_cols, const hbk_lowp_gather_column_t* cols, hbk_stream_t stream);

/* REQUESTER STITCH  hbk_lowp_lookup_fwd_runs: hbk_lowp_lookup_fwd -- ragged segments, the three combiners,
 *   id_weights, the zero-row rules, out_stride, fp32 output, fp32 sums in id order from +0 -- over a SEGMENTED
 *   table as in hbk_lookup_column_t: logical rows [run_start[k], run_start[k + 1]) (the last run ends at
 *   col.rows) live at col.table + run_base[k] ELEMENTS; run_start[0] = 0; device int64 arrays [n_runs], n_runs >= 1;
 *   a base may be negative.  table_dtype is per column: one call may mix bf16 and fp16 columns.  The result is
 *   hbk_group_lookup_fwd over the same runs of the upcast fp32 buffer, bit for bit.
 *   Lane widths as hbk_lowp_lookup_fwd, with one difference: a lane moves 4 elements by default at every dim
 *   (the run bases must then be multiples of 4 elements, which hbk_sharded_layout's padding gives) and 8 only
 *   with col.chunk_elems = 8 (the caller then promises bases that are multiples of 8 elements).
 *   Refused as hbk_lowp_lookup_fwd refuses, plus n_runs < 1 or a NULL run array. */
typedef struct {
  hbk_lowp_lookup_column_t col;
  const int64_t* run_start;  /* device [n_runs] */
  const int64_t* run_base;   /* device [n_runs], elements */
  int32_t n_runs;            /* >= 1 */
  int32_t reserved;          /* 0 */
} hbk_lowp_lookup_runs_column_t;
int hbk_lowp_lookup_fwd_runs(int32_t n_cols, const hbk_lowp_lookup_runs_column_t* cols, hbk_stream_t stream);

/* Gradients of REPLICATED tables across ranks, in their dense form (the reference's
 * TRAINABLE_REPLICATED_SMALL, training/gradient.py:131-141): every rank scatters its IndexedSlices into one
 * bucket, ONE allreduce sums the buckets, and each table's block of the bucket is then read back as
 * IndexedSlices with holes -- which hbk_sparse_apply_slices_n takes as they are.
 *
 * The bucket is one contiguous fp32 buffer of bucket_floats floats that the caller lays out: per table a
 * block [rows, dim] (contiguous rows; start every block on a 16-byte boundary to keep 16-byte lanes) and,
 * behind all blocks, per table `touched`, one fp32 word per row.  cols[c].block and cols[c].touched point into
 * it; no two of these ranges may overlap.
 *
 * hbk_replica_grads_pack_n: clears the whole bucket to +0.0f on the stream (a memset node: capturable), then,
 * one launch per 64 columns, for every u < n_unique[0] (read on the device, clamped to [0, capacity]) with
 * r = unique_rows[u] inside [0, rows):
 *     block[r, :] = grad_rows[u, :]        touched[r] = 1.0f
 * A bit copy: rows are distinct (not checked), so these are plain stores, no atomics.  Entries at or after
 * n_unique are not read; an entry outside [0, rows) stores nothing.  A lane group per slice row, sized from the
 * width: 16-byte lanes when dim % 4 == 0 and grad_rows and block are 16-byte aligned, else 4-byte lanes.
 * Refused before the memset: a NULL unique_rows, grad_rows or n_unique of a column with capacity > 0; a NULL
 * block or touched of a column with rows > 0; capacity < 0 or >= 2^30; rows < 0 or >= 2^31; dim < 1 or beyond
 * the apply's limits (256 as 16-byte lanes, 64 as 4-byte lanes); a NULL bucket; bucket_floats <= 0 or
 * >= 2^31; a block or touched range that is misaligned, leaves the bucket or overlaps another.
 *
 * After the allreduce (SUM, in place; a row is touched when any rank touched it):
 * hbk_replica_grads_rows_n, one launch per 64 columns:
 *     urows[r] = touched[r] != 0 ? r : -1     for every r in [0, rows)
 * (urows int64 [rows]; the word holds the number of ranks that touched row r times the scale the allreduce
 * applied to the whole bucket: > 0 for a mean or a sum, < 0 under a negative scale).  With a device int32 that holds `rows` as n_unique, (urows, block, rows) is table c's
 * IndexedSlices with holes: no compaction, no copy.  Reads touched, writes urows; block, unique_rows, grad_rows
 * and n_unique are not looked at.  Detected by the presence of the symbols. */
typedef struct {
  const int64_t* unique_rows;  /* device [capacity] */
  const float* grad_rows;      /* device [capacity, dim], contiguous */
  const int32_t* n_unique;     /* device [1] */
  int64_t capacity;
  int64_t rows;
  int32_t dim;
  float* block;                /* inside the bucket: [rows, dim] */
  float* touched;              /* inside the bucket, behind the blocks: [rows] */
  int64_t* urows;              /* device [rows]: written by hbk_replica_grads_rows_n */
} hbk_replica_column_t;
int hbk_replica_grads_pack_n(int32_t n_cols, const hbk_replica_column_t* cols, float* bucket,
                             int64_t bucket_floats, hbk_stream_t stream);
int hbk_replica_grads_rows_n(int32_t n_cols, const hbk_replica_column_t* cols, hbk_stream_t stream);

/* Sequence lookups: a ragged id list WITHOUT a combiner -- the padded [batch, max_len, dim] rows an
 * attention layer reads (DIN / DIEN / BST): docs/tutorial/ranking/data.py:195-224
 * (transform_categorical_non_pooling: tf.sparse.slice to max_varlength ids, tf.sparse.to_dense(default_value=),
 * then the lookup of the [batch, max_varlength] grid), or TF's sequence_categorical_column_* + embedding_column
 * + SequenceFeatures (zero rows past a sample's length, and a sequence_length vector).
 * seq is an array of n_cols entries, one per column.  Per column, with B = n_segments, T = seq[c].max_len,
 * len_b = row_splits[b + 1] - row_splits[b] (1 when row_splits == NULL) and L_b = min(len_b, T), for every
 * position p = b * T + t of the flattened [B * T] grid:
 *     t <  L_b            id(p) = ids[row_splits[b] + t]     (the sample's FIRST T ids; later ones are never read)
 *     t >= L_b, has_pad   id(p) = pad_id
 *     t >= L_b, no pad    nothing is looked up: out[b, t, :] = 0, row_grid[p] = -1
 *     g(p)        = floormod(id(p), bucket)   (bucket > 0)
 *                 = id(p)                     (bucket == 0; id(p) < 0: nothing is looked up, zero row, -1)
 *     row_grid[p] = g(p)
 *     out[b, t, :] = table[g(p) / divisor, :]                (rows outside [0, rows) read as zeros)
 *     lengths[b]  = L_b
 * cols[c].out is [B, T, dim] fp32; cols[c].out_stride counts the floats between SAMPLES (0 = T * dim, else
 * >= T * dim); a sample's T rows are contiguous.  The 16-byte / 4-byte chunk rule of out_stride holds over
 * table, out and that stride.  max_norms (NULL, or a HOST float[n_cols], 0 = not clipped) clips every
 * looked-up row, pad rows included, as hbk_group_lookup_fwd_clipped does (same formulas and order of s).
 * lengths and row_grid may be NULL (not wanted: the inference form writes neither).  cols[c].combiner and
 * hot_rows are ignored.  Refused (HBK_INVALID_ARGUMENT) before any device work: seq == NULL, max_len < 1,
 * id_weights, out_slots, half_io, n_runs > 0, B * T >= 2^31, a bad max_norm, a row the gather cannot take.
 * No workspace, no host synchronisation, no device-to-host copy: capturable.  One launch per kind of column
 * (16-byte or 4-byte chunks, clipped or not).
 *
 * The backward needs no entry of its own.  row_grid is bucketized already, so a column of ONE id per
 * segment with
 *     ids = row_grid (HBK_INT64), n_ids = n_segments = B * T, row_splits = NULL, bucket = 0,
 *     the same divisor / rows / table, grad_out = the [B, T, dim] gradient in place, grad_stride = dim
 * (a gradient with a sample stride other than T * dim: one contiguous copy first) handed to
 * hbk_group_lookup_bwd* IS the backward of the sequence lookup: a negative id with bucket == 0 maps to no
 * row, so padding without pad_id and truncated ids (which are not in the grid at all) reach no reduce, no
 * unique_rows and no optimizer slot, while pad_id's row collects the gradient of every padding position.
 * The emit form, apply_lr, Adagrad, Lazy Adam, FTRL, the _clipped entries (with the forward's max_norms),
 * HBK_GRAD_DETERMINISTIC (the order is position order, b-major) and table_pitch apply unchanged.
 * Detected by the presence of the symbols; the structs above and the version are those of 0.2.0. */
typedef struct {
  int32_t max_len;     /* T >= 1 */
  int32_t has_pad;     /* 0: padding positions are zero rows, -1 in the grid */
  int64_t pad_id;      /* has_pad != 0: mapped like any id of the column */
  int32_t* lengths;    /* device [n_segments] or NULL */
  int64_t* row_grid;   /* device [n_segments * max_len] or NULL (inference) */
} hbk_sequence_t;
int hbk_group_lookup_fwd_sequence(int32_t n_cols, const hbk_lookup_column_t* cols,
                                  const hbk_sequence_t* seq, const float* max_norms,
                                  hbk_stream_t stream);
/* row_grid and lengths alone, by the same arithmetic: one thread per position, reads ids and row_splits
 * only (cols[c].table and cols[c].out may be NULL; dim and out_stride are not looked at).  With
 * hbk_group_lookup_fwd over the grid (the column of the recipe above, out viewed [B * T, dim]) this is the
 * two-launch form of the sequence lookup: the same bits as the fused entry. */
int hbk_sequence_row_grid_n(int32_t n_cols, const hbk_lookup_column_t* cols,
                            const hbk_sequence_t* seq, hbk_stream_t stream);
/* The RAW-id grid: what a sharded hash-keyed sequence column hands the sharded step as B * T ids of one sample
 * each.  hbk_sequence_row_grid_n with bucket == 0 writes -1 for every negative id and every padding position,
 * and -1 is an ordinary key of a hash table (see hbk_hash_translate_sequence_n); here the effective ids
 * themselves are written.  With B, T, len_b and L_b as above, for every position p = b * T + t:
 *     row_grid[p] = ids[row_splits[b] + t]   (t <  L_b; sign-extended from int32 ids, NEVER bucketized, negative
 *                                             ids kept; an index outside [0, n_ids) is not read: pad_id)
 *                 = pad_id                   (t >= L_b)
 *     lengths[b]  = L_b                      (lengths may be NULL)
 * row_splits == NULL: one id per sample.  Only ids and row_splits are read, and never an id past a sample's first
 * T: cols[c].table, out, bucket, divisor, rows, dim and every other field of the column are ignored.
 * Refused (HBK_INVALID_ARGUMENT) before any device work: seq == NULL, has_pad == 0 (there is no "nothing" value
 * among raw ids), row_grid == NULL (also with B == 0), max_len < 1, B * T >= 2^31.  One launch for up to 64 columns, one thread per
 * position, 8-byte coalesced stores; no workspace, no atomics, no host synchronisation: capturable.
 * Detected by the presence of the symbol; the structs and the version are those of 0.2.0. */
int hbk_sequence_id_grid_n(int32_t n_cols, const hbk_lookup_column_t* cols,
                           const hbk_sequence_t* seq, hbk_stream_t stream);
/* The PACKED form of a zero-padded sequence column: what a sharded sequence column WITHOUT a pad id hands the
 * sharded step.  Neither grid above can say "nothing" to that step (it bucketizes a -1 into row bucket - 1, and
 * among raw ids every int64 is a key), but the step takes ragged columns, and with combiner sum an empty segment
 * is a zero row that reaches no gradient.  A zero-padded sequence column is such a column: B * T segments, one
 * per position, each holding exactly one id where the position holds one and none where it is padding; the ids
 * are the effective ids packed back to back.  Padding is in no list: it is never sent, looked up or stepped.
 * Per column, with B = n_segments, T = seq[c].max_len:
 *     len_b            = row_splits ? row_splits[b + 1] - row_splits[b] : 1      (a negative value counts as 0)
 *     l_b              = min(len_b, T)
 *     sample_splits[b] = sum over b' < b of l_b'          sample_splits[B] = total
 *     lengths[b]       = l_b                                                     int32 [B]   (seq[c].lengths)
 *     pos_splits[b * T + t] = sample_splits[b] + min(t, l_b)   pos_splits[B * T] = total     int32 [B * T + 1]
 *     packed[sample_splits[b] + t] = (int64) ids[row_splits[b] + t]   for t < l_b            int64
 *     total[0]         = sample_splits[B]                                                    int32 [1]
 * sample_splits (int32 [B + 1]) is the CSR of the packed ids by sample, pos_splits their CSR by position.  Packed
 * ids are RAW: sign-extended from int32 ids, negative ids kept, nothing bucketized (the sharded step floormods a
 * bucketed column itself; a hash column wants the raw id).  Never read: an id past a sample's first T.  Never
 * written: an element of packed at or past total.  An id index row_splits[b] + t outside [0, n_ids) follows
 * hbk_sequence_id_grid_n's rule: it is not read -- where the grid holds the pad id, the packed element, which has
 * none to hold, holds 0.  No contents of row_splits make the kernels read or write out of bounds: with row
 * splits that are no CSR of the ids total may exceed packed_capacity, and the elements at or past
 * packed_capacity are then not written either (compare total with the capacity).
 * The id side of cols[c] (ids, ids_dtype, n_ids, row_splits, n_segments) is read as hbk_sequence_id_grid_n reads
 * it; every other field of the column is ignored.  Of seq[c]: max_len and lengths; has_pad must be 0; row_grid
 * and pad_id are ignored.  Refused (HBK_INVALID_ARGUMENT) before any launch, the column named: max_len < 1,
 * B * T >= 2^31, n_ids >= 2^31, n_segments != n_ids with row_splits == NULL, a NULL output (all five are
 * written, also with B == 0), packed_capacity < min(n_ids, B * T), has_pad != 0 (a pad id belongs to the grid
 * ops), a workspace smaller than hbk_sequence_pack_workspace_bytes answers (the message states the size).
 * n_cols == 0, B == 0 and all-empty samples are fine.
 * Three launches per 64 columns -- the clamped lengths of every tile of 256 samples summed into the workspace;
 * one workgroup per column scans its tile sums and writes total; every tile scans its own samples, writes lengths
 * and sample_splits and covers its positions (pos_splits, packed) -- of plain loads and vector stores, 8 bytes
 * wide to packed, no atomics.  No host read, no device-to-host copy, and no scratch that has to be cleared
 * (every workspace word is written before it is read): capturable and replayable.  The caller that narrows
 * packed to total elements reads total himself.
 * Detected by the presence of the symbols; the structs above and the version are those of 0.2.0. */
typedef struct {
  int64_t* packed;           /* device [packed_capacity] */
  int64_t packed_capacity;   /* >= min(n_ids, B * T) */
  int32_t* pos_splits;       /* device [B * T + 1] */
  int32_t* sample_splits;    /* device [B + 1] */
  int32_t* total;            /* device [1] */
} hbk_sequence_pack_t;
size_t hbk_sequence_pack_workspace_bytes(int32_t n_cols, const hbk_lookup_column_t* cols);
int hbk_sequence_pack_n(int32_t n_cols, const hbk_lookup_column_t* cols, const hbk_sequence_t* seq,
                        const hbk_sequence_pack_t* pack, void* workspace, size_t workspace_bytes,
                        hbk_stream_t stream);

/* Key-deduplicated features: rows that are the same for many samples of a batch (the user side of a click log;
 * the reference's hb.data.deduplicate, data/dataframe.py:301-392, restores the IDS to batch length before the
 * lookup) are looked up ONCE per distinct key and expanded to the batch on the device.  n_keys = U rows are
 * produced by whatever lookup runs underneath; idx (int32 or int64, [n_samples]) names, per sample, the row it
 * takes.  A column is rows of `width` 4-byte elements, any width >= 1; strides count elements, 0 = contiguous.
 *
 * hbk_expand_rows_n -- the forward.  For every column and every b < n_samples:
 *     out[b, :] = src[idx[b], :]      if 0 <= idx[b] < n_keys
 *               = a zero row          otherwise (also: every row when n_keys == 0)
 * a pure copy of bits (fp32 rows, or int32 rows such as sequence lengths).  idx == NULL is the identity,
 * out[b, :] = src[b, :] for every b < n_samples (src holds n_samples rows and n_keys is not read): a plain block
 * placed by the same kind of launch.  An index is compared with [0, n_keys) before any address is formed from it.
 * One launch per 64 columns; a lane group per output row sized from the width, 16-byte lanes where width, both
 * strides and both addresses are multiples of 4 elements / 16 bytes, else 4-byte lanes (chosen per column by the
 * host); wider rows are tiled.  Plain loads and vector stores, no atomics, no workspace, no host read: capturable.
 *
 * hbk_expand_index_build -- the inverse of idx, built once per key field and step and shared by its columns:
 *     order[splits[u] .. splits[u + 1])  = the samples b with idx[b] == u, in ASCENDING b     (u < n_keys)
 *     invalid[0]                         = the number of samples with idx[b] outside [0, n_keys): in no list
 * order is int32 [n_samples] (its elements at or past splits[n_keys] hold the samples in no list), splits int32
 * [n_keys + 1], invalid int32 [1]; splits and invalid are written whatever the sizes.  A key kernel writes the
 * pairs (idx[b] valid ? idx[b] : n_keys, b), a stable LSD radix sort (rocPRIM) orders them by key, one lower bound
 * per key writes splits: no atomics, so the order does not depend on the run.  No host read and no allocation;
 * capture of this call is not promised.  The workspace holds the pairs and the sort's scratch.
 *
 * hbk_expand_rows_grad_n -- the transpose.  src is the gradient [n_samples, width] (typically a column block of
 * the batch gradient), out is [n_keys, width]:
 *     out[u, :] = src[order[splits[u]], :] + src[order[splits[u] + 1], :] + ...      (fp32, in this order)
 * one sequential chain per element that STARTS FROM ITS FIRST TERM (not from 0) and adds the following terms one
 * by one; a key with an empty list gets a zero row; every row of out is written, nothing needs clearing.  One lane
 * group per (key, width tile), several rows of the list loaded ahead of the adds; no atomics: the same bits on
 * every run.  An element of order outside [0, n_samples) is skipped, splits are clamped to [0, n_samples].  A key
 * that owns thousands of samples is one latency-bound chain (long lists are not split).  Capturable.
 *
 * Refused (HBK_INVALID_ARGUMENT) before any device work, the column named: a NULL src or out with rows to move,
 * width < 1, a stride below the width, n_samples or n_keys negative or >= 2^31, an id dtype that is neither int32
 * nor int64, a workspace smaller than hbk_expand_index_workspace_bytes answers (the message states the size),
 * more than one column naming the same out.  n_cols == 0, n_samples == 0 and n_keys == 0 are fine.
 * Bytes moved per column: 4 * width * (n_samples + n_keys) + the index forward; 4 * width * (n_samples + n_keys)
 * + 4 * n_samples + 4 * n_keys backward.
 * Detected by the presence of the symbols; the structs above and the version are those of 0.2.0. */
typedef struct {
  const void* src;      /* device [rows, src_stride]: n_keys rows (forward), n_samples rows (transpose, identity) */
  void* out;            /* device [rows, out_stride]: n_samples rows (forward), n_keys rows (transpose) */
  int64_t src_stride;   /* elements between rows; 0 = width */
  int64_t out_stride;
  int32_t width;        /* 4-byte elements per row, >= 1 */
} hbk_expand_column_t;
int hbk_expand_rows_n(int32_t n_cols, const hbk_expand_column_t* cols, const void* idx, int32_t idx_dtype,
                      int64_t n_samples, int64_t n_keys, hbk_stream_t stream);
size_t hbk_expand_index_workspace_bytes(int64_t n_samples, int64_t n_keys);
int hbk_expand_index_build(const void* idx, int32_t idx_dtype, int64_t n_samples, int64_t n_keys, int32_t* order,
                           int32_t* splits, int32_t* invalid, void* workspace, size_t workspace_bytes,
                           hbk_stream_t stream);
int hbk_expand_rows_grad_n(int32_t n_cols, const hbk_expand_column_t* cols, const int32_t* order,
                           const int32_t* splits, int64_t n_samples, int64_t n_keys, hbk_stream_t stream);

/* R10 (sharded form)  d(stitch + combiner): the transpose of the requester-side
 *   `gather(embeddings, shard_index)` + combiner (hbtf/embedding/sharding.py:200; TF emits
 *   SparseSegment*Grad followed by an UnsortedSegmentSum over a permutation):
 *     grad_rows[index[j], :] = scale(seg(j)) * grad_out[seg(j), :]
 *   `index` = the `indices` output of the forward partition (a permutation of 0..n_ids-1), so
 *   each row of grad_rows [n_ids, dim] is written exactly once.  The result is what travels
 *   back through the reverse alltoallv (hbtf/distribute/collective.py:334-347).            */
typedef struct {
  int32_t dim;
  int32_t combiner;
  int64_t n_ids;
  const int32_t* index;       /* device [n_ids] */
  const int32_t* row_splits;  /* device [n_segments + 1] or NULL */
  int64_t n_segments;
  const float* grad_out;      /* device [n_segments, dim] */
  float* grad_rows;           /* device [n_ids, dim] */
  /* optional segmented destination (n_runs > 0): rows [run_start[k], run_start[k+1]) of
   * grad_rows live at grad_rows + run_base[k] floats (the peer-major send buffer of the
   * reverse exchange; same tables as the forward's hbk_lookup_column_t runs).  Device arrays. */
  const int64_t* run_start;
  const int64_t* run_base;
  int32_t n_runs;
  int32_t grad_stride;        /* row stride of grad_out in floats; 0 = dim */
  /* per-id weights of the forward's stitch (device fp32 [n_ids], NULL: unweighted):
   * grad_rows[index[j], :] = t_j as in hbk_lookup_grad_column_t.id_weights */
  const float* id_weights;
} hbk_stitch_grad_column_t;

int hbk_group_stitch_bwd(int32_t n_cols, const hbk_stitch_grad_column_t* cols,
                         hbk_stream_t stream);

/* ------------------------------------------------------------------------------------
 * R11 HbLookup: cache probe.  op hbtf/embedding/lookup_ops.cc:38-58; kernel
 *     hbtf/embedding/lookup_functors.cu.cc:54-149; hash hybridbackend/common/murmur3.cu.h:32-77.
 *     slab = murmur3_hash32(key) % slab_count; a slab is `slab_size` consecutive int64 keys
 *     (the reference fixes 32 = its warp; here 1..64, one wave64 probes a slab with one
 *     ballot); first matching slot -> hit; an EMPTY (INT64_MIN) slot in the slab -> miss;
 *     else next slab (linear, wrapping).
 *     hit_slot[i] = cache index (slab*slab_size+slot) or -1 for a miss -- a per-key result
 *     in key order (the reference's compacted hit/miss lists follow from it; its own
 *     slicing is inconsistent).  n_miss: device int32, may be NULL.          */
int hbk_cache_probe(const int64_t* keys_cache, int64_t slab_count, int32_t slab_size,
                    const int64_t* keys, int64_t n_keys, int64_t* hit_slot,
                    int32_t* n_miss, hbk_stream_t stream);
/* The op's four outputs (lookup_ops.cc:38-58), key order kept inside each list (the reference
 * fills them through atomic counters, i.e. in no particular order):
 *   hit_keys_indices[h]  = i of the h-th key found        hit_cache_indices[h] = its cache index
 *   miss_keys_indices[m] = i of the m-th key not found    miss_keys[m]         = keys[i]
 * All four have capacity n_keys; counts (device int32[2]) = {n_hit, n_miss}.  The op sizes its
 * outputs from counts after one host sync (lookup_ops.cc:118-121); the C ABI leaves that to the
 * caller. */
size_t hbk_cache_lookup_workspace_bytes(int64_t n_keys);
int hbk_cache_lookup(const int64_t* keys_cache, int64_t slab_count, int32_t slab_size,
                     const int64_t* keys, int64_t n_keys, int32_t* hit_keys_indices,
                     int64_t* hit_cache_indices, int32_t* miss_keys_indices, int64_t* miss_keys,
                     int32_t* counts, void* workspace, size_t workspace_bytes,
                     hbk_stream_t stream);
/* test hook: murmur3_hash32<int64, 0> of each key, on device */
int hbk_murmur3_hash32(const int64_t* keys, int64_t n_keys, uint32_t* out,
                       hbk_stream_t stream);

/* Hash-keyed tables: device find-or-insert, the WRITER of the slab key cache hbk_cache_probe reads.  Raw
 * int64 ids become row numbers of a fixed-capacity table (capacity = slab_count * slab_size rows), so two
 * ids never share a row as they do under floormod(id, num_buckets) (DeepRec's EmbeddingVariable; the
 * reference's EmbeddingService in miniature, whose own placement -- where(cache_keys == EMPTY)[:n_miss],
 * hbtf/embedding/service.py:212-218 -- is not where its probe looks).  One launch serves all
 * columns (64 per launch).
 *
 * Placement rule, per key (EMPTY = INT64_MIN; keys_cache starts all EMPTY):
 *     slab = murmur3_hash32(key) % slab_count
 *     the slab holds the key                 -> slots[i] = slab * slab_size + its slot
 *     else the slab has EMPTY slots          -> the FIRST of them is claimed (64-bit agent-scope
 *                                               compare-and-swap EMPTY -> key); a claim lost to the same key
 *                                               is a hit on that slot, a claim lost to another key reads the
 *                                               same slab again (match first, then its first EMPTY slot)
 *     else (the slab is full)                -> the next slab, wrapping; after slab_count slabs slots[i] = -1
 * Slots only ever go EMPTY -> key, so a key never sits behind a slab that still has an EMPTY slot: every key
 * this entry placed is found by hbk_cache_probe / hbk_cache_lookup on the same array, and by insert = 0.
 * key == EMPTY is never stored and gives -1.  Retries are bounded by slab_size per slab and slab_count slabs
 * per key; no workgroup waits for another.
 *
 * Row initialisation.  The call that inserts a key writes its row, table[slot * pitch + j] for j < dim:
 *     r      = murmur3_hash32(key ^ (int64)((uint64)(seed + j + 1) * 0x9E3779B97F4A7C15))
 *     row[j] = ((float)(r >> 8) * 2^-23 - 1.0f) * init_scale          (uniform in [-init_scale, init_scale))
 * exact in fp32 up to the final multiply; init_scale == 0 stores +0.0f; table == NULL writes nothing; rows of
 * keys already present are not touched.  A row's start depends on its key, never on the slot it got.
 *
 * Counters.  counts (device int32[2] or NULL; the CALLER zeroes it, calls add to it): {n_inserted, n_failed}.
 * n_inserted counts keys stored by this call (a key repeated in the call counts once); n_failed counts key
 * OCCURRENCES whose slot is -1.  One atomic per wave and counter.
 *
 * Reproducible between runs: every key's row contents; which keys are stored when no key fails; the SET of
 * keys of every slab when no slab overflows into its neighbour.  NOT reproducible: slot numbers (the order
 * inside a slab, and which keys spill once a slab is full, depend on which workgroup claims first), hence
 * not which keys fail in a table that fills up.
 *
 * insert == 0: a pure find -- no compare-and-swap, no row is written, plain loads; n_failed counts the
 * misses.  The results are hbk_cache_probe's (except key == EMPTY: -1 here), for N columns in one launch.
 *
 * Refused (HBK_INVALID_ARGUMENT) before any device work: slab_size outside [1, 64], slab_count < 1, NULL
 * keys_cache / keys / slots with n_keys > 0, n_keys outside [0, 2^31), dim < 1 with a table, table_pitch
 * non-zero and < dim, init_scale negative, NaN or infinite.  No workspace, no host synchronisation:
 * capturable.  The row numbers feed hbk_group_lookup_fwd* / hbk_group_lookup_bwd* as int64 ids with
 * bucket = 0 (a -1 looks nothing up and reaches no gradient row).  Detected by the presence of the symbol;
 * the structs above and the version are those of 0.2.0. */
typedef struct {
  int64_t* keys_cache;    /* device [slab_count * slab_size], 8-byte aligned */
  int64_t slab_count;
  int32_t slab_size;      /* 1..64 */
  const int64_t* keys;    /* device [n_keys] */
  int64_t n_keys;
  int64_t* slots;         /* device [n_keys]: row number or -1 */
  int32_t* counts;        /* device int32[2] {n_inserted, n_failed}, added to; or NULL */
  float* table;           /* device, slab_count * slab_size rows; NULL: new rows are not initialised */
  int32_t dim;
  int32_t table_pitch;    /* floats between rows; 0 = dim */
  float init_scale;       /* finite, >= 0 */
  int64_t seed;
} hbk_hash_column_t;
int hbk_hash_insert_n(int32_t n_cols, const hbk_hash_column_t* cols, int32_t insert,
                      hbk_stream_t stream);

/* Expiring hash tables: last-seen steps, an eviction sweep and slot reuse (DeepRec's steps_to_live).  A table
 * that cannot forget has a fixed lifetime: new ids arrive for ever.  An expiring table is an hbk_hash_column_t
 * table plus per-slot metadata, translated by hbk_hash_insert_expiring_n and swept by hbk_hash_evict_n;
 * hbk_hash_insert_n above and the tables it serves are unchanged (INT64_MIN + 1 stays an ordinary key there).
 *
 * Sentinels.  EMPTY = INT64_MIN as above and TOMBSTONE = INT64_MIN + 1.  Eviction turns key -> TOMBSTONE, never
 * -> EMPTY: a slab without an EMPTY slot stays without one, so every live key is still found by the walk of
 * hbk_cache_probe / hbk_cache_lookup (to them a tombstone is a key nobody asks for).  The ids EMPTY and
 * TOMBSTONE are never stored; they translate to -1 and count in n_failed.  EMPTY slots come back only by
 * rebuilding the table (hbk_hash_rehash_n below; HashTable.compact in Python is the same in torch ops).
 *
 * Placement rule of the expiring insert, per key:
 *     walk the slabs from murmur3_hash32(key) % slab_count, wrapping, at most slab_count slabs:
 *         the slab holds the key             -> slots[i] = its slot, done
 *         remember the FIRST TOMBSTONE slot seen on the walk (slab order, then slot order)
 *         the slab has an EMPTY slot         -> stop walking here
 *     claim the remembered TOMBSTONE (compare-and-swap TOMBSTONE -> key) if there is one, else the stopping
 *     slab's first EMPTY slot (EMPTY -> key), else slots[i] = -1
 *     a claim lost to the same key is a hit on that slot; a claim lost to another key walks again from the
 *     home slab
 * The walk goes past a tombstone to the stopping slab before it claims: a key that spilled into the next slab
 * while its home slab was full is still there after a slot of the home slab was evicted, and must be found,
 * not stored a second time.  Concurrent inserters of one key end in one slot (the argument is in
 * csrc/hash_insert.hip).  Retries are bounded: a walk reads at most slab_count slabs, and each new walk is a
 * free slot that somebody else filled; no workgroup waits for another.  With no tombstone in the table the
 * results are those of hbk_hash_insert_n: the same slab sets, the same counters.  The winner writes the row as
 * above, a function of (key, seed, j).
 *
 * Metadata, written by the translate launch itself.  last_seen, freq: device int32 [slab_count * slab_size];
 * step: a device int32 scalar the caller keeps current (on the device so that replayed launches and captured
 * graphs see it).  With insert != 0 every id OCCURRENCE that resolves to a slot >= 0 stores last_seen[slot] =
 * *step and adds 1 to freq[slot] (relaxed agent-scope atomic); the add is skipped once the value read is
 * >= 2^30, and n_keys >= 2^30 per column is refused, so the counter never wraps: it saturates somewhere in
 * [2^30, 2^31).  A find (insert == 0) and an occurrence answered -1 touch neither array.
 *
 * Counters.  counts as above ({n_inserted, n_failed}; a key stored into a reused slot counts in n_inserted).
 * stats (device int32[2] or NULL, zeroed by the caller, added to): {n_evicted, n_reused}.  n_reused counts the
 * keys stored into a TOMBSTONE slot, n_evicted is the sweep's.  Live keys = n_inserted - n_evicted.
 *
 * hbk_hash_evict_n: one streaming pass over the slots of N tables.  A slot whose key is neither EMPTY nor
 * TOMBSTONE is evicted iff
 *     steps_to_live > 0  and  (int64)*step - last_seen[slot] >= steps_to_live
 *     and (keep_freq == 0  or  freq[slot] < keep_freq)
 * (idle ids expire unless they were seen often enough to be kept for good; steps_to_live == 0 evicts
 * nothing).  For an evicted slot: key = TOMBSTONE, freq = last_seen = 0, and for each of the n_fills companion
 * arrays (the optimizer slots, which the next id to get the row must not inherit: Adagrad's accumulator ->
 * initial_accumulator_value, Adam's m / v -> 0, FTRL's accum / linear -> theirs) base[slot * pitch + j] =
 * value for j < dim; the padding up to pitch is not written.  The embedding row is left as it is: the next
 * inserter writes it.  The sweep must be stream-ordered against the translate launches of its tables, never
 * concurrent with one (its accesses to the key array are plain).  It reads 16 bytes per slot.
 *
 * Reproducible between runs: the evicted SET (a function of the arrays alone), n_evicted, every row's
 * contents, freq and last_seen per key.  NOT reproducible: which of several free slots a key gets under
 * concurrency beyond what is stated for hbk_hash_insert_n, hence n_reused once keys of different home slabs
 * compete for the same tombstones (exact for one slab, or one key at a time).
 *
 * Refused (HBK_INVALID_ARGUMENT) before any device work: everything hbk_hash_insert_n refuses; NULL last_seen,
 * freq or step where there is work (n_keys > 0; always for the sweep, which also needs keys_cache); n_keys
 * >= 2^30; steps_to_live < 0 or keep_freq < 0; n_fills outside [0, 4]; a fill with NULL base, dim < 1, a
 * non-zero pitch < dim or a non-finite value.  No workspace, no host synchronisation: both are capturable.
 * Detected by the presence of the symbols; the version stays that of 0.2.0. */
typedef struct {
  int32_t* last_seen;     /* device int32 [slab_count * slab_size] */
  int32_t* freq;          /* device int32 [slab_count * slab_size] */
  const int32_t* step;    /* device int32 scalar: the current step */
  int32_t* stats;         /* device int32[2] {n_evicted, n_reused}, added to; or NULL */
} hbk_hash_expiry_t;
/* exp[c] belongs to cols[c] */
int hbk_hash_insert_expiring_n(int32_t n_cols, const hbk_hash_column_t* cols, const hbk_hash_expiry_t* exp,
                               int32_t insert, hbk_stream_t stream);

#define HBK_HASH_MAX_FILLS 4
typedef struct {
  float* base;            /* device, slab_count * slab_size rows */
  int32_t pitch;          /* floats between rows; 0 = dim */
  int32_t dim;
  float value;            /* finite */
} hbk_hash_fill_t;
typedef struct {
  int64_t* keys_cache;    /* device [slab_count * slab_size], 8-byte aligned */
  int64_t slab_count;
  int32_t slab_size;      /* 1..64 */
  hbk_hash_expiry_t exp;
  int64_t steps_to_live;  /* >= 0; 0: nothing expires */
  int32_t keep_freq;      /* >= 0; 0: frequency keeps nothing */
  int32_t n_fills;        /* 0..HBK_HASH_MAX_FILLS */
  hbk_hash_fill_t fills[HBK_HASH_MAX_FILLS];
} hbk_hash_evict_column_t;
int hbk_hash_evict_n(int32_t n_cols, const hbk_hash_evict_column_t* cols, hbk_stream_t stream);

/* Bounded tables: evict the oldest keys down to a size bound (the reference's EmbeddingService removes the
 * num_removes entries with the oldest step: hybridbackend/tensorflow/embedding/service.py:180-210).
 * hbk_hash_evict_n asks for an age threshold in advance; hbk_hash_evict_to_n finds it on the device.  Per table:
 *     live      = the slots that hold a key (neither EMPTY nor TOMBSTONE), L = |live|
 *     evictable = the live slots with  keep_freq == 0  or  freq[slot] < keep_freq    (hbk_hash_evict_n's guard)
 *     need      = L - max_size;  need <= 0: nothing is written to the table's arrays, they stay bit-identical
 *     cut       = the smallest v with  #{evictable : last_seen <= v} >= need,  last_seen compared as SIGNED int32;
 *                 fewer than `need` evictable slots: cut = INT32_MAX (every evictable slot goes, and the table
 *                 stays above the bound)
 * and every evictable slot with last_seen <= cut is evicted exactly as hbk_hash_evict_n evicts: key = TOMBSTONE,
 * freq = last_seen = 0, the rows of the n_fills companion arrays = their value, stats[0] += the slots evicted.
 * *step is not read: the order is last_seen itself.
 *
 * WHOLE STEPS LEAVE TOGETHER.  Keys last seen at the same step are equally old, so all of them go: the size
 * after the call is <= max_size (unless the frequency guard kept it above) and undershoots the bound by less
 * than the keys of one step -- those with last_seen == cut.  There is no tie-break: the evicted set is a
 * function of the table's arrays alone, the same on every run and whatever slots the keys sit in (the
 * reference's top_k picks arbitrarily among ties).  Not an exact size.  This entry orders by age alone and
 * keep_freq is its only use of freq; hbk_hash_evict_to_lfu_n (below) orders by (freq, last_seen).
 *
 * report (device int32[4] or NULL), written by the call: {live_before, need, cut, n_evicted}; cut is 0 when
 * need <= 0.
 *
 * One call serves N tables of any capacities (more than 32: several launches each).  The selection is a radix
 * select over last_seen ^ 0x80000000, most significant digit first, 11 / 11 / 10 bits: per digit one streaming
 * histogram pass over the slots (16 bytes per slot; per-workgroup histogram in LDS, a wave's hits on its leading
 * lane's bin added once, non-zero bins added to the table's histogram with integer atomics -- an
 * order-independent sum) and one small kernel per table that picks the bin the remaining need falls into; then
 * the sweep.  The passes after the first leave at once for a table with need <= 0.  No host read anywhere:
 * everything is stream-ordered device work, and the call clears its workspace on the stream itself, so it can
 * be captured into a graph and replayed.  Stream-ordered against the translate launches of its tables, never
 * beside one, as the sweep.
 *
 * workspace: device memory of hbk_hash_evict_to_workspace_bytes(n_cols) bytes, 4-byte aligned; contents are
 * scratch.  Refused (HBK_INVALID_ARGUMENT) before any device work: what hbk_hash_evict_n refuses of keys_cache,
 * slab_count, slab_size and the fills; NULL last_seen or freq; max_size < 0; keep_freq < 0; a table of 2^31
 * slots or more (the counters are int32); a NULL or too small workspace where n_cols > 0.  exp.step may be
 * NULL. */
typedef struct {
  int64_t* keys_cache;    /* device [slab_count * slab_size], 8-byte aligned */
  int64_t slab_count;
  int32_t slab_size;      /* 1..64 */
  hbk_hash_expiry_t exp;  /* step is not read */
  int64_t max_size;       /* >= 0: the keys that may stay */
  int32_t keep_freq;      /* >= 0; 0: frequency keeps nothing */
  int32_t n_fills;        /* 0..HBK_HASH_MAX_FILLS */
  hbk_hash_fill_t fills[HBK_HASH_MAX_FILLS];
  int32_t* report;        /* device int32[4] {live_before, need, cut, n_evicted}, or NULL */
} hbk_hash_evict_to_column_t;
size_t hbk_hash_evict_to_workspace_bytes(int32_t n_cols);
int hbk_hash_evict_to_n(int32_t n_cols, const hbk_hash_evict_to_column_t* cols, void* workspace,
                        size_t workspace_bytes, hbk_stream_t stream);

/* The selection alone: hbk_hash_evict_to_n without its sweep.  Same struct, same argument checks and refusal texts
 * (under the name hash_evict_to_select_n), same workspace (hbk_hash_evict_to_workspace_bytes), the same clear
 * launch and three digit passes -- and no sweep: the table's arrays, its stats and its companions are NOT WRITTEN
 * (the fills are checked and not used).  report is required here (NULL is refused) and receives
 *     {live_before, need, cut, n_selected}
 * live_before, need and cut as above (cut = 0 when need <= 0, INT32_MAX when fewer than `need` slots are
 * evictable); n_selected is the exact number of slots the sweep of hbk_hash_evict_to_n would evict from the table
 * as it is: 0 when need <= 0, else the evictable slots with last_seen <= cut -- all evictable slots when cut =
 * INT32_MAX.  It falls out of the select: the need consumed before the last chosen bin plus that bin's count.  No
 * host read, capturable; the report is what hbk_hash_spill_n (below, behind the export) takes as its selection.
 * hbk_hash_evict_to_n itself is unchanged: the fourth word of its report stays the sweep's own count. */
int hbk_hash_evict_to_select_n(int32_t n_cols, const hbk_hash_evict_to_column_t* cols, void* workspace,
                               size_t workspace_bytes, hbk_stream_t stream);

/* Bounded tables in LFU order: the LEAST FREQUENTLY USED keys leave first (DeepRec's multi-tier EmbeddingVariable
 * offers LRU and LFU caches).  hbk_hash_evict_to_n orders by last_seen alone; hbk_hash_evict_to_lfu_n orders by the
 * pair (freq, last_seen): least frequent first, among equally frequent keys the oldest first, both fields compared
 * as SIGNED int32 (an import may carry any value).  As one 64-bit key
 *     k(slot) = ((uint64)(freq ^ 0x80000000) << 32) | (uint32)(last_seen ^ 0x80000000)
 * Per table, live, evictable (the keep_freq guard) and need = L - max_size are hbk_hash_evict_to_n's, and
 *     cut       = the smallest k with  #{evictable : k(slot) <= cut} >= need;  fewer than `need` evictable slots:
 *                 every evictable slot goes, the table stays above the bound, and the report says
 *                 cut_freq = cut_last_seen = INT32_MAX
 * and every evictable slot with k(slot) <= cut leaves exactly as the other sweeps make a key leave: key = TOMBSTONE,
 * last_seen = freq = 0, the rows of the n_fills companion arrays = their value (the padding up to the pitch not
 * written), stats[0] += the slots evicted.  need <= 0: nothing is written to the table's arrays.  *step is not
 * read.
 *
 * WHOLE CLASSES LEAVE TOGETHER.  Keys with equal (freq, last_seen) are equally cold, so all of them go: the size
 * after the call is <= max_size (unless the frequency guard kept it above) and undershoots the bound by less than
 * one such class -- the slots with k == cut.  There is no tie-break by slot: the evicted set is a function of the
 * table's arrays alone, the same on every run.
 *
 * report (device int32[8] or NULL -- EIGHT words, not the four of hbk_hash_evict_to_n), written by the call:
 *     {live_before, need, cut_freq, cut_last_seen, n_evicted, 0, 0, 0}
 * both cuts are 0 when need <= 0.
 *
 * The selection is the radix select of hbk_hash_evict_to_n carried over k: SIX digits, most significant first,
 * 11 / 11 / 10 bits over freq, then 11 / 11 / 10 over last_seen; per digit one streaming histogram pass (16 bytes
 * per slot; per-workgroup LDS histogram, a wave's hits on its leading lane's bin added once -- real counts pile up
 * on 1 and 2 --, integer atomics into the table's histogram: an order-independent sum) and one pick kernel per
 * table that carries the 64-bit prefix and the need that remains; a slot takes part in a digit only if its higher
 * digits equal the prefix.  Then the sweep.  The passes after the first leave at once for a table with need <= 0.
 * 32 tables per launch, more are chunked.  No host read anywhere; the call clears its workspace on the stream, so
 * it can be captured into a graph and replayed.
 *
 * Same struct as hbk_hash_evict_to_n (report -> int32[8]), the same argument checks and refusal texts under the
 * names hash_evict_to_lfu_n / hash_evict_to_lfu_select_n, refused before any device work; workspace: device memory
 * of hbk_hash_evict_to_lfu_workspace_bytes(n_cols) bytes, 4-byte aligned, contents scratch.
 *
 * hbk_hash_evict_to_lfu_select_n is the selection alone -- the clear launch and the six digit passes, no sweep,
 * nothing of the table written, report required -- and writes {live_before, need, cut_freq, cut_last_seen,
 * n_selected, 0, 0, 0}: n_selected is the exact number of slots the sweep would evict, as it falls out of the
 * select.  Its report is what hbk_hash_spill_lfu_n takes as its selection.
 *
 * freq saturates at 2^30 and otherwise never forgets; callers let old popularity fade by shifting freq right in
 * place between calls (Python: HashTable.age_freq).  Detected by the presence of the symbols; the version stays
 * that of 0.2.0. */
size_t hbk_hash_evict_to_lfu_workspace_bytes(int32_t n_cols);
int hbk_hash_evict_to_lfu_n(int32_t n_cols, const hbk_hash_evict_to_column_t* cols, void* workspace,
                            size_t workspace_bytes, hbk_stream_t stream);
int hbk_hash_evict_to_lfu_select_n(int32_t n_cols, const hbk_hash_evict_to_column_t* cols, void* workspace,
                                   size_t workspace_bytes, hbk_stream_t stream);

/* Removal by id: the keys the caller names leave (tf.lookup's mutable tables have remove; the reference's
 * EmbeddingService removes entries by index: hybridbackend/tensorflow/embedding/service.py:180-210).  The sweeps
 * above decide by age; hbk_hash_remove_n takes a list.  Expiring tables only: a plain table has no TOMBSTONE, and
 * INT64_MIN + 1 is an ordinary key there.  Per table:
 *     slots[i] = the slot keys[i] held BEFORE the call, or -1 -- for every occurrence, duplicates included; the ids
 *                EMPTY and TOMBSTONE give -1
 *     every distinct id that was found leaves exactly as hbk_hash_evict_n makes a key leave: key = TOMBSTONE (never
 *     EMPTY: the probe's invariant holds, keys that spilled past the slot's slab are still found), last_seen =
 *     freq = 0, and for each of the n_fills companion arrays base[slot * pitch + j] = value for j < dim, the
 *     padding up to pitch not written.  The embedding row is left as it is: the next inserter writes it.
 *     stats[0] and *n_removed (device int32 or NULL; the CALLER zeroes it, the call adds to it) grow by the number
 *     of DISTINCT ids removed: live keys = n_inserted - n_evicted stays right.  counts, an admission sketch and
 *     stats[1] are not touched.
 * Every array, both counters and slots are functions of the inputs alone: the same on every run.
 *
 * Two launches per 32 columns on the call's stream.  The first is the pure find of the expiring kind
 * (hbk_hash_insert_expiring_n with insert == 0: plain loads, no counter; a column of 2^30 keys or more goes
 * through it in parts) and writes slots.  The second is tiled over the occurrences: a lane with slots[i] >= 0
 * swaps keys[slot]: id -> TOMBSTONE with a 64-bit agent-scope compare-and-swap; of the occurrences of an id
 * exactly one wins, stores the metadata zeros, and the wave fills its winners' companion rows with lane groups of
 * pow2(dim) lanes; one atomic per wave and counter.  The kernel boundary between the two is what makes slots
 * deterministic: in one fused kernel a duplicate that walks after the winner's swap would answer -1.  Which
 * occurrence wins is not fixed, and nothing written depends on it.
 *
 * Stream-ordered against the translates, sweeps and backwards of its tables, never beside one.  No workspace, no
 * host synchronisation: capturable.  It reads, per occurrence, the 8-byte id, the slabs of its walk and writes an
 * 8-byte slot; per removed key the 8-byte swap, 8 bytes of metadata and the fills' rows.
 *
 * Refused (HBK_INVALID_ARGUMENT) before any device work, naming the column and the field: what hbk_hash_evict_n
 * refuses of keys_cache, slab_count, slab_size and the fills; a table of 2^31 slots or more (the counters are
 * int32); NULL last_seen or freq; NULL keys or slots with n_keys > 0; n_keys outside [0, 2^31); 32 consecutive
 * columns whose find would need a grid of 2^31 tiles (only at slab_size above 32, with nearly 2^31 ids in each).  More
 * than 32 columns with keys run as groups of 32, a group's find and erase before the next group's.  exp.step is not
 * read and may be NULL.  Detected by the presence of the symbol; the version stays that of 0.2.0. */
typedef struct {
  int64_t* keys_cache;    /* device [slab_count * slab_size], 8-byte aligned */
  int64_t slab_count;
  int32_t slab_size;      /* 1..64 */
  hbk_hash_expiry_t exp;  /* last_seen, freq and stats are used; step is not read */
  const int64_t* keys;    /* device [n_keys]: the ids to remove */
  int64_t n_keys;
  int64_t* slots;         /* device [n_keys], written: the slot every id held before the call, or -1 */
  int32_t* n_removed;     /* device int32, added to: the distinct ids removed; or NULL */
  int32_t n_fills;        /* 0..HBK_HASH_MAX_FILLS */
  hbk_hash_fill_t fills[HBK_HASH_MAX_FILLS];
} hbk_hash_remove_column_t;
int hbk_hash_remove_n(int32_t n_cols, const hbk_hash_remove_column_t* cols, hbk_stream_t stream);

/* Admission filter: a count-min sketch gates new ids (DeepRec's CounterFilter / CBFFilter beside
 * steps_to_live).  Most distinct ids of a click log occur once or twice; unfiltered, each of them claims a row,
 * its optimizer slots and a key slot at first sight.  A filtered table stores an id once it was seen min_freq
 * times; until then it translates to -1: a zero row that reaches no gradient and no optimizer slot (DeepRec reads
 * its default-value row there).  The counters are a sketch per table, not per-id counters in the key array: an
 * exact counter would spend a key slot on every rare id.  hbk_hash_insert_n and hbk_hash_insert_expiring_n are
 * unchanged.
 *
 * sketch: device int32 [depth * width], zero at start, row r at sketch + r * width.  The cell of key k in row r:
 *     cell(k, r) = murmur3_hash32(k ^ (int64)((uint64)(seed + r + 1) * 0x9E3779B97F4A7C15)) % width
 * (the mix of the row initialisation above).
 *
 * A call with insert != 0 is COUNT, THEN ADMIT: two kernels on the call's stream.
 *   1. count.  Every occurrence is looked for by its table's own walk (the plain rule, or the rule with
 *      tombstones).  Found: that slot is the answer (an expiring table's last_seen / freq are written as above)
 *      and the sketch is not touched -- a batch of resident ids issues no atomic.  Not found and not a sentinel
 *      of that table kind (those are -1, counted in n_failed): 1 is added to each of its depth cells, a relaxed
 *      agent-scope atomic add skipped when the value read is already >= 2^30 (the ceiling rule of freq; n_keys
 *      >= 2^30 per column is refused, so a counter cannot wrap).
 *   2. admit.  For an occurrence not found in 1: estimate = min over r of sketch[r][cell(k, r)], read after
 *      ALL of 1.  estimate >= min_freq: the find-or-insert of that table kind -- the same compare-and-swap rules,
 *      the row written by the one winner, the same counts / stats, last_seen / freq for every occurrence that
 *      resolved to a slot.  Otherwise slots[i] = -1, *filtered grows by one per occurrence and nothing else is
 *      written: not the key array, not counts, not last_seen / freq.
 * Between the two kernels slots[] holds a provisional value (-2) for the unresolved occurrences; none survives
 * the call.  When the columns need several launches (more than 64 columns) or two columns name one table, every
 * counting launch of the call runs before any admitting launch.
 *
 * What follows.  The decision depends on the sketch after phase 1 alone, so every occurrence of an id in one
 * call gets the same answer, and an id seen min_freq times inside one batch is admitted by that batch.  Which
 * ids are admitted, the sketch, filtered, n_inserted and n_failed are the same on every run and equal to a
 * sequential restatement (phase 1 over all keys, then phase 2 in key order); slot numbers stay run-dependent as
 * above.  Collisions only add: estimate >= the true count, an id is admitted early, never late.  An admitted id
 * that finds the table full is -1 counted in n_failed, not in filtered.  insert == 0 is the find of the entry
 * without a filter and never touches the sketch.
 *
 * The sketch is never decremented.  An id evicted from an expiring table is therefore admitted again at once
 * unless the caller cleared the sketch or aged it (halved every counter): both are plain array operations, not
 * entries of this ABI (HashTable.clear_filter / age_filter in Python).
 *
 * Refused (HBK_INVALID_ARGUMENT) before any device work: everything the entry without a filter refuses; NULL
 * adm; NULL sketch with n_keys > 0; width outside [1, 2^31), depth outside [1, 8], min_freq outside [1, 2^30];
 * n_keys >= 2^30; a sketch that is not 4-byte aligned.  No workspace, no host synchronisation: capturable.
 * Detected by the presence of the symbols; the structs above and the version are those of 0.2.0. */
#define HBK_HASH_MAX_SKETCH_DEPTH 8
typedef struct {
  int32_t* sketch;        /* device int32 [depth * width] */
  int64_t width;          /* 1 .. 2^31 - 1 */
  int32_t depth;          /* 1 .. HBK_HASH_MAX_SKETCH_DEPTH */
  int32_t min_freq;       /* 1 .. 2^30 */
  int64_t seed;
  int32_t* filtered;      /* device int32: occurrences the filter answered -1, added to; or NULL */
} hbk_hash_admission_t;
/* adm[c] (and exp[c]) belongs to cols[c] */
int hbk_hash_insert_admit_n(int32_t n_cols, const hbk_hash_column_t* cols, const hbk_hash_admission_t* adm,
                            int32_t insert, hbk_stream_t stream);
int hbk_hash_insert_expiring_admit_n(int32_t n_cols, const hbk_hash_column_t* cols,
                                     const hbk_hash_expiry_t* exp, const hbk_hash_admission_t* adm,
                                     int32_t insert, hbk_stream_t stream);

/* Hash-keyed 16-bit tables: the translate entries over tables whose rows are bf16 / fp16 ("Low-precision
 * tables" above).  exp / adm select the table kind for ALL columns of the call, as for hbk_hash_translate_runs_n
 * below: (NULL, NULL) = hbk_hash_insert_n, (exp, NULL) = hbk_hash_insert_expiring_n,
 * (NULL, adm) = hbk_hash_insert_admit_n, (exp, adm) = hbk_hash_insert_expiring_admit_n -- and the call IS that
 * entry: placement, tombstone reuse,
 * last_seen / freq, the sketch's two phases, the counters and insert == 0 are unchanged, the same kernels walk the
 * slabs.  The one difference is the row the inserting call writes.  cols[c].table points at 2-byte elements of
 * table_dtypes[c] (host int32 [n_cols], HBK_LOWP_BF16 or HBK_LOWP_FP16); dim and table_pitch count ELEMENTS;
 *     row[j] = round_to_nearest_even(v_j),   v_j = the fp32 value of "Row initialisation" above
 * with the rounding of the low-precision apply (bf16: the bits of a float32 -> bfloat16 cast; fp16: the hardware
 * conversion); init_scale == 0 stores 0x0000.  A row depends on (key, seed, j, dtype) alone, never on the slot;
 * there is no stochastic initialisation.  The winning lane group writes whole 4-byte words -- word w holds element
 * 2w in its low and 2w + 1 in its high half -- so nothing outside [row, row + dim) is written and the padding up to
 * table_pitch keeps what it held.  Every other per-slot array (rows moved by hbk_hash_rehash_n, hbk_hash_export_n,
 * hbk_hash_store_rows_n, hbk_hash_spill_n) travels as 4-byte words already: a 16-bit row of even dim is dim / 2 of
 * them.  The optimizer slots of such a table stay fp32.
 *
 * Refused (HBK_INVALID_ARGUMENT) before any device work, with the entry, the column and the field named: everything
 * the matching fp32 entry refuses; NULL table_dtypes with n_cols > 0; a code other than HBK_LOWP_BF16 /
 * HBK_LOWP_FP16; with a table: an odd dim, an odd non-zero table_pitch, a table that is not 4-byte aligned;
 * HBK_LOWP_FP16 with init_scale > 65504 (a start value would round to infinity).  n_cols == 0 returns HBK_OK without
 * touching a device.  No workspace, no host synchronisation: capturable.  Keys that arrive as runs or sequences go
 * through hbk_hash_translate_runs_lowp_n / hbk_hash_translate_sequence_lowp_n below (hbk_hash_translate_runs_n and
 * hbk_hash_translate_sequence_n write fp32 rows).  Detected by the presence of the symbol; the structs and the version
 * are those of 0.2.0. */
int hbk_hash_insert_lowp_n(int32_t n_cols, const hbk_hash_column_t* cols,
                           const hbk_hash_expiry_t* exp    /* NULL: plain tables */,
                           const hbk_hash_admission_t* adm /* NULL: no filter */,
                           const int32_t* table_dtypes     /* [n_cols]: HBK_LOWP_BF16 / HBK_LOWP_FP16 */,
                           int32_t insert, hbk_stream_t stream);

/* Keys that arrive as runs.  On the owner of a sharded hash table (hbk_sharded_set_hash_tables below) the ids of
 * one column are W separate arrays, one per requester, each with its own place for the answers.  Handing them
 * to the four entries above as W virtual columns costs one 64-column launch per 64 runs (26 columns x 8 peers:
 * 4 launches, 8 for filtered tables) and grows with W.  hbk_hash_translate_runs_n takes the runs as they lie.
 *
 * cols[c] describes table c as above; its keys, slots and n_keys are IGNORED: runs[c][0 .. n_runs[c]) are
 * column c's keys and slots.  exp and adm are each NULL or hold one record per column, and name the table kind
 * of ALL columns of the call: (NULL, NULL) = hbk_hash_insert_n, (exp, NULL) = hbk_hash_insert_expiring_n,
 * (NULL, adm) = hbk_hash_insert_admit_n, (exp, adm) = hbk_hash_insert_expiring_admit_n.
 *
 * Semantics: exactly those of the matching entry called ONCE on the concatenation of column c's runs --
 * placement, row initialisation, counts, stats, last_seen, freq and the sketch.  n_inserted counts a key once
 * even when it appears in several runs (one compare-and-swap wins).  For filtered tables the counting phase
 * covers all runs of all columns before any admitting launch starts: an id seen once in each of two runs, with
 * min_freq = 2, is admitted by the call.  insert == 0 is the find of the entry without a filter.
 *
 * Launches: one per call, two for filtered tables (count, admit), while the non-empty runs number at most
 * HBK_HASH_MAX_RUNS_PER_LAUNCH and the columns at most 64 (26 columns x 8 runs = 208 fit).  The kernels are
 * those of the four entries with another way to find a tile's work: the tile's RUN is found with up to four
 * 64-wide ballots over the runs' first tiles, and the run names its column.  Beyond the limits the call is
 * chunked, every counting launch still before any admitting one.
 *
 * Refused (HBK_INVALID_ARGUMENT) before any device work: everything the matching entry refuses of a column;
 * NULL n_runs or runs with n_cols > 0; n_runs[c] < 0; NULL runs[c] with n_runs[c] > 0; a run with n_keys < 0, or
 * with n_keys > 0 and NULL keys or slots; a column whose runs sum to >= 2^31 keys (>= 2^30 with exp or adm: a
 * counter must not wrap).  Zero runs and zero-length runs are fine.  No workspace, no host synchronisation:
 * capturable.  Detected by the presence of the symbol; the version stays that of 0.2.0. */
#define HBK_HASH_MAX_RUNS_PER_LAUNCH 256
typedef struct {
  const int64_t* keys;    /* device [n_keys] */
  int64_t* slots;         /* device [n_keys]: row number or -1 */
  int64_t n_keys;
} hbk_hash_run_t;
int hbk_hash_translate_runs_n(int32_t n_cols, const hbk_hash_column_t* cols,
                              const hbk_hash_expiry_t* exp,      /* NULL, or [n_cols] */
                              const hbk_hash_admission_t* adm,   /* NULL, or [n_cols] */
                              const int32_t* n_runs, const hbk_hash_run_t* const* runs,
                              int32_t insert, hbk_stream_t stream);

/* Runs over 16-bit tables: hbk_hash_translate_runs_n for tables whose rows are bf16 / fp16, what the owner of a
 * sharded 16-bit hash table calls.  The call IS hbk_hash_translate_runs_n with the same cols, exp, adm, n_runs and runs
 * -- placement, tombstone reuse, last_seen / freq, the two phases of a filtered table, the counters, how a tile finds
 * its run, the chunking beyond HBK_HASH_MAX_RUNS_PER_LAUNCH runs or 64 columns -- except for the row the inserting
 * launch writes, which is hbk_hash_insert_lowp_n's: cols[c].table points at 2-byte elements of table_dtypes[c] (host
 * int32 [n_cols], HBK_LOWP_BF16 or HBK_LOWP_FP16), dim and table_pitch count ELEMENTS, row[j] is the fp32 start value
 * rounded to nearest even, stored as whole 4-byte words, a function of (key, seed, j, dtype) alone; the padding up to
 * table_pitch keeps what it held.  Only the inserting launches are other kernels (the LOWP instantiations over the
 * runs); insert == 0 and the counting phase of a filtered table write no row and are the launches of
 * hbk_hash_translate_runs_n as they are.
 *
 * Refused (HBK_INVALID_ARGUMENT) before any device work, with the entry, the column and the field named: everything
 * hbk_hash_translate_runs_n refuses; NULL table_dtypes with n_cols > 0; a code other than HBK_LOWP_BF16 /
 * HBK_LOWP_FP16; with a table: an odd dim, an odd non-zero table_pitch, a table that is not 4-byte aligned;
 * HBK_LOWP_FP16 with init_scale > 65504.  n_cols == 0 returns HBK_OK without touching a device.  No workspace, no host
 * synchronisation: capturable.  Detected by the presence of the symbol; the structs and the version are those of
 * 0.2.0. */
int hbk_hash_translate_runs_lowp_n(int32_t n_cols, const hbk_hash_column_t* cols,
                                   const hbk_hash_expiry_t* exp,      /* NULL, or [n_cols] */
                                   const hbk_hash_admission_t* adm,   /* NULL, or [n_cols] */
                                   const int32_t* table_dtypes        /* [n_cols]: HBK_LOWP_BF16 / HBK_LOWP_FP16 */,
                                   const int32_t* n_runs, const hbk_hash_run_t* const* runs,
                                   int32_t insert, hbk_stream_t stream);

/* Hash-keyed sequence lookups: the first T ids of every sample translated into a slot grid.  The behaviour
 * histories of DIN / DIEN / BST (item and shop ids: an open vocabulary) are the columns that most need a raw-id
 * table, and hbk_group_lookup_fwd_sequence above reads ids only through floormod(id, bucket).  The existing calls
 * do not compose: hbk_sequence_row_grid_n with bucket == 0 maps every negative id to -1 and writes -1 at padding
 * positions, and -1 is an ordinary key of a hash table (translated, it would be inserted once per padding position,
 * bump its freq and count in the sketch); translating the whole ragged list inserts the ids past T, which the
 * sequence lookup promises are never read -- they would claim a key slot, a row and its optimizer slots for ever
 * and stay fresh in an expiring table without ever being trained; padding with INT64_MIN gives -1 but counts
 * every padding position in n_failed.  hbk_hash_translate_sequence_n reads ids the way the sequence lookup does.
 *
 * exp and adm name the table kind of ALL columns as for hbk_hash_translate_runs_n.  cols[c] describes table c;
 * cols[c].keys / n_keys are the flat int64 ids of the column and cols[c].slots is the SLOT GRID, int64 [B * T]
 * with B = seq[c].n_segments and T = seq[c].max_len.  len_b = row_splits[b + 1] - row_splits[b] (1 when
 * row_splits == NULL) and L_b = min(len_b, T).  The EFFECTIVE ID LIST E_c of a column is, sample after sample,
 * the sample's first L_b ids, followed by T - L_b copies of pad_id when has_pad.
 *   - The call does to the table, its counters, stats, last_seen, freq and the sketch exactly what the matching
 *     existing entry does when called ONCE on E_c.
 *   - The answer for position p = b * T + t is written to slots[p].
 *   - A padding position (t >= L_b) without has_pad gets slots[p] = -1 and touches nothing else: no walk, no
 *     n_failed, no filtered, no sketch cell, no freq.
 *   - lengths[b] = L_b (lengths may be NULL: not wanted).
 *   - Ids at positions >= T of a sample are never read.
 *   - An id equal to INT64_MIN in the data behaves as it does everywhere: -1, counted in n_failed; in an expiring
 *     table INT64_MIN + 1 behaves the same way.  "Nothing here" is a state of its own in the kernel, not the
 *     EMPTY sentinel by value.
 *   - insert == 0 is a pure find (of the entry without a filter: no sketch is touched).
 *   - For filtered tables every counting launch of the call runs before any admitting launch.
 * A row_splits entry that points outside [0, n_keys) names no id: such a position is padding.
 *
 * Kernel: those of the four entries with a third way to find a tile's work, by POSITION.  A tile covers
 * positions of one column; a position finds its sample by a fast division by T, reads the two row_splits
 * entries and takes its key, the pad id or nothing; the walk runs unchanged.  One launch per call (two for
 * filtered tables) up to 64 columns, chunked beyond.
 *
 * Recipe.  The slot grid is what hbk_group_lookup_fwd_sequence's row_grid is to a bucketed column:
 *     forward   hbk_group_lookup_fwd[_clipped] over a column of ONE id per segment with ids = the slot grid
 *               (HBK_INT64), n_ids = n_segments = B * T, row_splits = NULL, bucket = 0, table = the hash table's
 *               rows, out = the [B, T, dim] output viewed [B * T, dim]: a -1 reads a zero row
 *     backward  the same column handed to hbk_group_lookup_bwd* (the recipe of hbk_group_lookup_fwd_sequence)
 * The translate and the gather are two launches on purpose: a concurrent duplicate of a new id can hit the freshly
 * claimed slot before the winner has written its row, so the row write and the gather need a kernel boundary
 * between them.
 *
 * Refused (HBK_INVALID_ARGUMENT) before any device work: everything the matching entry refuses of a column (with
 * B * T in the place of n_keys), of expiry and of admission; seq == NULL with n_cols > 0; max_len < 1;
 * n_segments < 0; B * T >= 2^31 (>= 2^30 with exp or adm: a counter must not wrap); NULL slots with B * T > 0;
 * n_keys outside [0, 2^31); NULL keys with n_keys > 0; row_splits == NULL with n_keys != n_segments; has_pad with
 * pad_id == INT64_MIN, and in an expiring table also pad_id == INT64_MIN + 1.  n_cols == 0, B == 0 and a column
 * of only empty samples are fine.  No workspace, no host synchronisation: capturable.  Detected by the presence of
 * the symbol; the structs above and the version are those of 0.2.0. */
typedef struct {
  const int32_t* row_splits;   /* device int32 [n_segments + 1], or NULL: one id per sample */
  int64_t n_segments;          /* B >= 0 */
  int32_t max_len;             /* T >= 1 */
  int32_t has_pad;             /* 0: padding positions are -1 in the grid and touch nothing */
  int64_t pad_id;              /* has_pad != 0: a RAW id, any value the table can store */
  int32_t* lengths;            /* device int32 [n_segments], or NULL */
} hbk_hash_sequence_t;
/* seq[c] (and exp[c], adm[c]) belongs to cols[c] */
int hbk_hash_translate_sequence_n(int32_t n_cols, const hbk_hash_column_t* cols,
                                  const hbk_hash_expiry_t* exp,      /* NULL, or [n_cols] */
                                  const hbk_hash_admission_t* adm,   /* NULL, or [n_cols] */
                                  const hbk_hash_sequence_t* seq,    /* [n_cols] */
                                  int32_t insert, hbk_stream_t stream);

/* Sequences over 16-bit tables: hbk_hash_translate_sequence_n for tables whose rows are bf16 / fp16.  The call IS
 * hbk_hash_translate_sequence_n with the same cols, exp, adm and seq -- the effective id list, the slot grid, lengths,
 * the "nothing" state of a padding position without a pad id, the rule that ids at positions >= T are never read,
 * placement, metadata, the sketch's two phases, the counters -- except for the row the inserting launch writes, which
 * is hbk_hash_insert_lowp_n's (see hbk_hash_translate_runs_lowp_n above: table_dtypes[c], nearest even, whole 4-byte
 * words, a function of (key, seed, j, dtype) alone).  Only the inserting launches are other kernels; insert == 0 and
 * the counting phase of a filtered table are the launches of hbk_hash_translate_sequence_n as they are.  The recipe
 * above holds with the 16-bit gathers in the place of hbk_group_lookup_fwd: hbk_lowp_lookup_fwd over ids = the slot
 * grid, bucket = 0; a -1 reads a zero row.
 *
 * Refused (HBK_INVALID_ARGUMENT) before any device work, with the entry, the column and the field named: everything
 * hbk_hash_translate_sequence_n refuses; NULL table_dtypes with n_cols > 0; a code other than HBK_LOWP_BF16 /
 * HBK_LOWP_FP16; with a table: an odd dim, an odd non-zero table_pitch, a table that is not 4-byte aligned;
 * HBK_LOWP_FP16 with init_scale > 65504.  n_cols == 0 returns HBK_OK without touching a device.  No workspace, no host
 * synchronisation: capturable.  Detected by the presence of the symbol; the structs and the version are those of
 * 0.2.0. */
int hbk_hash_translate_sequence_lowp_n(int32_t n_cols, const hbk_hash_column_t* cols,
                                       const hbk_hash_expiry_t* exp,      /* NULL, or [n_cols] */
                                       const hbk_hash_admission_t* adm,   /* NULL, or [n_cols] */
                                       const int32_t* table_dtypes        /* [n_cols]: HBK_LOWP_BF16 / HBK_LOWP_FP16 */,
                                       const hbk_hash_sequence_t* seq,    /* [n_cols] */
                                       int32_t insert, hbk_stream_t stream);

/* Missing ids: the distinct ids of N id lists that their tables do not hold -- what a fault-in asks the host tier
 * for (HashTable.fault_in composed it from a find, a boolean index and a sort per table, with two host
 * synchronisations each).  Expiring tables only, as fault-in.  seq == NULL: the id list E of a column is keys[0 ..
 * n_keys) and slots is int64 [n_keys].  seq != NULL ([n_cols]): E is the EFFECTIVE ID LIST exactly as
 * hbk_hash_translate_sequence_n defines it above -- per sample its first min(len, T) ids, then the pad id T - L_b
 * times when has_pad; padding without a pad id is "nothing here"; ids past T are never read; a row_splits entry
 * that points outside [0, n_keys) names no id -- and slots is the [B * T] grid.  positions = n_keys or B * T.
 *   - slots[p] is the pure find's answer for position p (with seq: -1 at a padding position without a pad id;
 *     seq[c].lengths is written as the translate writes it, or NULL).
 *   - out_ids[0 .. min(*count, out_capacity)) holds the distinct ids of E that the table does not hold, in the
 *     order of their FIRST OCCURRENCE in E.  *count is their number even when it exceeds out_capacity; writes stop
 *     at out_capacity, nothing is written behind it.
 *   - An id equal to INT64_MIN or INT64_MIN + 1 is never reported: no store can hold it.  A TOMBSTONE slot holds no
 *     key, so an evicted id is reported.
 *   - The table is NOT written: keys, rows, last_seen, freq, counts, stats and the sketch are bit for bit what
 *     they were.  Nothing is inserted, nothing past T is looked at.
 *   - slots, out_ids[0 .. count) and *count are functions of the inputs alone: the same on every run.
 *
 * Launches, on the call's stream: one clear of the workspace per call, then per 32 columns (more columns run as
 * groups of 32, as hbk_hash_remove_n) the find -- hbk_hash_insert_expiring_n or hbk_hash_translate_sequence_n with
 * insert == 0, called as it is --, a claim launch tiled over the positions and the count, scan and write of the
 * export's stream compaction.  The claim: a lane whose position holds an id with slots[p] < 0 and no sentinel puts
 * the id into a scratch set of the column -- open addressing over S = pow2 >= 2 * positions cells (at least 64),
 * EMPTY = INT64_MIN, home cell murmur3_hash32(id) & (S - 1), linear probing, cells claimed with a 64-bit agent-scope
 * compare-and-swap -- and does atomicMin(first[cell], p) on an int32 array pre-set to INT32_MAX; a lane that finds
 * its id in a cell does only the atomicMin (skipped when the value it reads there is already below p: first[]
 * only falls).  The probe reads at most S cells and no lane waits for another: there is no spin loop.  A wave whose positions all hit leaves after reading slots: a batch of resident ids issues no
 * atomic.  The compaction selects position p iff it missed and first[cell(id)] == p, in position order.
 *
 * Workspace: hbk_hash_missing_workspace_bytes(n_cols, cols, seq) bytes, 16-byte aligned: 12 bytes per cell and 8
 * bytes per 256 positions, so about 24 bytes per position.  Only the id counts, n_segments and max_len are read to
 * size it (a column whose counts are out of range adds nothing; the call refuses it).  The call clears what it
 * uses on the stream before it reads it: the workspace needs no preparation, there is no host read, and a captured
 * call replays on whatever the id buffers then hold.  Stream-ordered against the translates, sweeps and backwards
 * of its tables, never beside one.
 *
 * Refused (HBK_INVALID_ARGUMENT) before any device work, naming the column and the field: what hbk_hash_remove_n
 * refuses of keys_cache, slab_count and slab_size; NULL last_seen or freq; NULL count; out_capacity < 0; NULL
 * out_ids with out_capacity > 0; n_keys outside [0, 2^31) (positions >= 2^31); NULL keys with n_keys > 0; NULL
 * slots with positions > 0; with seq everything hbk_hash_translate_sequence_n refuses of an expiring table's
 * column (max_len < 1, n_segments < 0, B * T >= 2^30, row_splits == NULL with n_keys != n_segments, a sentinel
 * pad_id); 32 consecutive columns whose find would need a grid of 2^31 tiles; a NULL, misaligned or too small
 * workspace where one is needed, with the size needed.  n_cols == 0, n_keys == 0, B == 0 and all-empty samples are
 * fine (*count = 0).  exp.step is not read and may be NULL; exp.stats is not touched.  Detected by the presence of
 * the symbol; the structs above and the version are those of 0.2.0. */
typedef struct {
  const int64_t* keys_cache;   /* device [slab_count * slab_size], 8-byte aligned: read only */
  int64_t slab_count;
  int32_t slab_size;           /* 1..64 */
  hbk_hash_expiry_t exp;       /* last_seen and freq name an expiring table; nothing of it is written */
  const int64_t* keys;         /* device [n_keys]: the ids */
  int64_t n_keys;
  int64_t* slots;              /* device [n_keys], or [B * T] with seq; written: the find's answers */
  int64_t* out_ids;            /* device [out_capacity]; written: the distinct missed ids, first occurrence first */
  int64_t out_capacity;
  int64_t* count;              /* device int64 [1]; written: the distinct missed ids */
} hbk_hash_missing_column_t;
int hbk_hash_missing_n(int32_t n_cols, const hbk_hash_missing_column_t* cols,
                       const hbk_hash_sequence_t* seq,   /* NULL: flat id lists; else [n_cols] */
                       void* workspace, size_t workspace_bytes, hbk_stream_t stream);
size_t hbk_hash_missing_workspace_bytes(int32_t n_cols, const hbk_hash_missing_column_t* cols,
                                        const hbk_hash_sequence_t* seq);

/* Missing ids over runs.  On the owner of a sharded hash table the ids of one column are W separate arrays, one per
 * requester, each with its own place for the answers -- what hbk_hash_translate_runs_n reads where it lies.
 * hbk_hash_missing_runs_n is hbk_hash_missing_n for ids in that form: what the owner asks its host tier for before
 * the translate would insert a fresh row for a spilled id.  Expiring tables only.
 *
 * cols[c] describes table c and the outputs; runs[c][0 .. n_runs[c]) are column c's ids and the places for the
 * find's answers.  Semantics: exactly those of hbk_hash_missing_n called ONCE on E_c, the concatenation of column
 * c's runs in run order --
 *   - runs[c][q].slots holds the pure find's answers for that run;
 *   - out_ids[0 .. min(*count, out_capacity)) holds the distinct ids of E_c that the table does not hold, in the
 *     order of their FIRST OCCURRENCE in E_c: an id in two runs is reported once, at its earlier run.  *count is
 *     their number even when it exceeds out_capacity; nothing is written behind out_capacity;
 *   - INT64_MIN and INT64_MIN + 1 are never reported; a TOMBSTONE slot holds no key, so an evicted id is reported;
 *   - the table is NOT written: keys, rows, last_seen, freq, counts, stats and the sketch are bit for bit what they
 *     were;
 *   - slots, out_ids[0 .. count) and *count are functions of the inputs alone: the same on every run.
 *
 * Positions: every run is padded up to whole tiles of 256 positions, so that no tile straddles a run; the positions
 * behind a run's n_keys hold nothing, and positions stay monotone in the order of E_c.  Launches, on the call's
 * stream: one clear of the workspace per call, then per launch group -- up to 32 columns and
 * HBK_HASH_MAX_RUNS_PER_LAUNCH non-empty runs, a column's runs never split (26 columns x 8 runs fit one group) --
 * the find (hbk_hash_translate_runs_n with insert == 0, called as it is), a claim launch -- a workgroup
 * takes up to 1024 positions of one run, a wave walking four 64-position chunks in order as hbk_hash_missing_n's
 * claim does -- and the count, scan and write of the export's stream compaction.  A claim workgroup finds its run as
 * the runs translate does, with up to four 64-wide ballots over the runs' first claim tiles, and records it for the
 * count and write of its tiles; the scratch
 * set, the compare-and-swap, atomicMin(first[cell], p) with the load before it, and the selection are those of
 * hbk_hash_missing_n.  No lane waits for another: there is no spin loop.  A wave whose positions all hit issues no
 * atomic.
 *
 * Workspace: hbk_hash_missing_runs_workspace_bytes(n_cols, n_runs, runs) bytes, 16-byte aligned: 12 bytes per cell
 * (S = pow2 >= 2 * ids of the column, at least 64) and 12 bytes per tile.  Only the runs' n_keys are read to size it
 * (a column whose counts are out of range adds nothing; the call refuses it).  The call clears what it uses on the
 * stream before it reads it: there is no host read, and a captured call replays on whatever the id buffers then
 * hold.  Stream-ordered against the translates, sweeps and backwards of its tables, never beside one.
 *
 * Refused (HBK_INVALID_ARGUMENT) before any device work, naming the column and the field: what hbk_hash_missing_n
 * refuses of keys_cache, slab_count, slab_size, last_seen, freq, count, out_capacity and out_ids; what
 * hbk_hash_translate_runs_n refuses of an expiring table's runs (NULL n_runs or runs with n_cols > 0; n_runs[c] < 0;
 * NULL runs[c] with n_runs[c] > 0; a run with n_keys outside [0, 2^31), or with n_keys > 0 and NULL keys or slots; a
 * column whose runs sum to >= 2^30 keys); a column whose padded positions reach 2^31 (below 2^30 keys and at most
 * HBK_HASH_MAX_RUNS_PER_LAUNCH runs they cannot); a column with more than HBK_HASH_MAX_RUNS_PER_LAUNCH non-empty
 * runs; a launch group whose find would need a grid of 2^31 tiles; a NULL, misaligned or too small workspace where
 * one is needed, with the size needed.  n_cols == 0, zero runs and empty runs are fine (*count = 0).  exp.step is
 * not read and may be NULL; exp.stats is not touched.  Detected by the presence of the symbol; the structs above and
 * the version are those of 0.2.0. */
typedef struct {
  const int64_t* keys_cache;   /* device [slab_count * slab_size], 8-byte aligned: read only */
  int64_t slab_count;
  int32_t slab_size;           /* 1..64 */
  hbk_hash_expiry_t exp;       /* last_seen and freq name an expiring table; nothing of it is written */
  int64_t* out_ids;            /* device [out_capacity]; written: the distinct missed ids, first occurrence first */
  int64_t out_capacity;
  int64_t* count;              /* device int64 [1]; written: the distinct missed ids */
} hbk_hash_missing_runs_column_t;
int hbk_hash_missing_runs_n(int32_t n_cols, const hbk_hash_missing_runs_column_t* cols,
                            const int32_t* n_runs, const hbk_hash_run_t* const* runs,
                            void* workspace, size_t workspace_bytes, hbk_stream_t stream);
size_t hbk_hash_missing_runs_workspace_bytes(int32_t n_cols, const int32_t* n_runs,
                                             const hbk_hash_run_t* const* runs);

/* Rehash: growth and tombstone compaction on the device.  A full table answers -1 for ever, and an expiring
 * table's probes get longer with every tombstone; both are cured by moving every live key into a fresh key
 * array -- of a larger geometry, or of the same one -- with its rows.  hbk_hash_rehash_n does that for N tables
 * per launch (32 per launch) without a host round trip: one streaming pass over the source key array and one
 * insert into the destination per live key, the rows moving along.
 *
 * Source.  src_keys [src_slab_count * src_slab_size] is read with plain loads, 64 consecutive slots per wave;
 * nobody may write it during the call.  A slot holds a key unless it is EMPTY, or TOMBSTONE with expiring != 0
 * (expiring == 0: INT64_MIN + 1 is an ordinary key, as for hbk_hash_insert_n).  The keys of the source are
 * taken to be distinct, as the keys of a table are.
 *
 * Placement, per live key (dst_keys must be all EMPTY on entry: the caller's contract, not checked):
 *     slab = murmur3_hash32(key) % dst_slab_count
 *     the slab has EMPTY slots  -> the FIRST of them is claimed (64-bit agent-scope compare-and-swap EMPTY -> key);
 *                                  a claim lost (to another key: the source keys are distinct) reads the same
 *                                  slab again
 *     else (the slab is full)   -> the next slab, wrapping; after dst_slab_count slabs the key did not fit
 * the rule of hbk_hash_insert_n bit for bit, so hbk_cache_probe and every translate entry find each key where
 * this entry put it.  The destination holds no tombstone: the one rule serves plain and expiring tables.
 * Inside the kernel every read of dst_keys is a relaxed agent-scope 8-byte atomic load and every write the
 * compare-and-swap; no fences.  Retries are bounded by dst_slab_size per slab and dst_slab_count slabs per key;
 * no workgroup waits for another.  With dst capacity >= the live keys every key fits: the walk covers all slabs.
 *
 * Moves.  Each of the n_moves per-slot arrays (the embedding rows, optimizer slots, last_seen, freq) is an
 * array of rows of `words` 4-byte words, copied bit for bit: for a key that went from source slot s to
 * destination slot d, dst[d * dst_pitch + j] = src[s * src_pitch + j] for j < words, plain stores by the lane
 * group that won the slot; the padding between words and the pitch is not written, and neither are the rows of
 * destination slots no key took (the caller pre-fills them).  Rows whose bases, pitches and width are all
 * multiples of 16 bytes travel in 16-byte accesses.
 *
 * Results.  new_slots (device int64 [src capacity] or NULL): new_slots[s] = the destination slot of the key of
 * source slot s; -1 where s holds no key and where the key did not fit.  counts (device int32[2] or NULL, added
 * to): {n_moved, n_failed}, one atomic per wave and counter.  Reproducible between runs: the SET of keys of
 * every destination slab when no slab overflows, every row's contents per key, the counters.  NOT reproducible:
 * slot numbers.
 *
 * What a rehash invalidates: every slot number handed out before it, and -- the arrays being new -- every
 * address derived from the old ones (descriptors, captured graphs).
 *
 * Refused (HBK_INVALID_ARGUMENT) before any device work: n_cols < 0; NULL cols with n_cols > 0; a slab size
 * outside [1, 64] or a slab count < 1 or > 2^62 / 64 on either side; NULL or not 8-byte aligned src_keys /
 * dst_keys; src_keys == dst_keys; n_moves outside [0, 8]; a move with words < 1, a non-zero pitch < words, a NULL
 * or not 4-byte aligned src / dst, or src == dst.  n_cols == 0 returns HBK_OK without touching a device.  No
 * workspace, no host synchronisation: capturable.  Detected by the presence of the symbol; the version stays
 * that of 0.2.0. */
#define HBK_HASH_MAX_MOVES 8
typedef struct {            /* one per-slot array that travels with its key, in 4-byte words */
  const void* src;
  void* dst;
  int32_t words;            /* >= 1: words per row (fp32 rows, int32 metadata: copied bit for bit) */
  int32_t src_pitch;        /* words between rows; 0 = words */
  int32_t dst_pitch;
} hbk_hash_move_t;
typedef struct {
  const int64_t* src_keys;  /* device [src_slab_count * src_slab_size], 8-byte aligned */
  int64_t src_slab_count;
  int32_t src_slab_size;    /* 1..64 */
  int64_t* dst_keys;        /* device [dst_slab_count * dst_slab_size], 8-byte aligned, all EMPTY on entry */
  int64_t dst_slab_count;
  int32_t dst_slab_size;    /* 1..64 */
  int32_t expiring;         /* != 0: a TOMBSTONE in src is skipped; 0: INT64_MIN + 1 is an ordinary key */
  int32_t n_moves;          /* 0..HBK_HASH_MAX_MOVES */
  hbk_hash_move_t moves[HBK_HASH_MAX_MOVES];
  int64_t* new_slots;       /* device int64 [src capacity] or NULL */
  int32_t* counts;          /* device int32[2] {n_moved, n_failed}, added to; or NULL */
} hbk_hash_rehash_column_t;
int hbk_hash_rehash_n(int32_t n_cols, const hbk_hash_rehash_column_t* cols, hbk_stream_t stream);

/* Export and import: a table leaves the device whole and comes back whole.  A table's keys with their rows are
 * not the table: the optimizer slots of every key, and an expiring table's last_seen and freq, are state too.
 * hbk_hash_export_n packs the keys a table holds -- all of them, or those touched since a step -- with every
 * per-slot array named in the call into dense arrays of a geometry-free form; hbk_hash_store_rows_n is the
 * second half of the way back (the first half, placing the keys, is the table's own translate entry).
 *
 * hbk_hash_export_n, N tables per call (32 per launch), three launches per 32 tables on the call's stream.
 *
 * Selection.  Source slot s of column c is exported iff it holds a key -- keys[s] is not EMPTY, and not
 * TOMBSTONE when expiring != 0 (expiring == 0: INT64_MIN + 1 is an ordinary key, as for hbk_hash_rehash_n) --
 * and, in addition, since <= 0 or last_seen[s] >= since.  last_seen[s] is the step of the slot's last training
 * translate, and that step's backward is the only thing that writes the slot's row and optimizer slots: with
 * since = s0 + 1 the export holds exactly the keys whose payload may have changed after step s0 (a delta).
 * last_seen is read only when since > 0.
 *
 * Order.  The exported keys appear in ASCENDING SOURCE-SLOT ORDER, packed from position 0: the p-th exported
 * slot goes to position p.  No ticket atomic and no look-back between tiles -- no workgroup waits for another:
 *   1. count: every 256-slot tile writes its number of matches into the workspace;
 *   2. scan:  one workgroup per column turns the tile counts into exclusive offsets and writes the total to count;
 *   3. write: every tile evaluates the same predicate again and places its matches behind its offset.
 * The table's arrays must not be written during the call (launch 3 must see what launch 1 saw).
 *
 * Moves.  As for hbk_hash_rehash_n, each of the n_moves arrays is rows of `words` 4-byte words copied bit for
 * bit: for the key of source slot s at position p, dst[p * dst_pitch + j] = src[s * src_pitch + j] for j <
 * words; the padding between words and the pitch is not written.  Rows whose bases, pitches and width are all
 * multiples of 16 bytes travel in 16-byte accesses.  The embedding rows, last_seen, freq and the optimizer slots
 * are all just moves.
 *
 * Results.  out_keys[p] = the key, out_slots[p] (if not NULL) = its source slot, for p < min(count,
 * out_capacity).  *count ALWAYS receives the total number of matches; nothing is written at positions >=
 * out_capacity -- keys, slots and rows alike -- and the caller compares the two.  Positions in [count,
 * out_capacity) are not written.
 *
 * Memory rules.  Plain loads and plain vector stores only; no atomics.  Reproducible between runs: everything
 * -- the output is a function of the table's arrays alone.  What is NOT reproducible is inherited from the
 * table: which slot a key got when it was inserted, hence the order of the keys of two tables that hold the
 * same set.
 *
 * Workspace: hbk_hash_export_workspace_bytes(n_cols, cols, &bytes) reads the geometry of the columns only (8
 * bytes per 256 slots); one device pointer, 8-byte aligned, not kept after the call.  No host synchronisation:
 * capturable.
 *
 * Refused (HBK_INVALID_ARGUMENT) before any device work: everything hbk_hash_rehash_n refuses of a source
 * geometry and of a move; NULL count; NULL out_keys with out_capacity > 0; out_capacity < 0; since > 0 with NULL
 * last_seen; a NULL (or not 8-byte aligned) workspace with n_cols > 0.  n_cols == 0 returns HBK_OK without
 * touching a device.
 *
 * hbk_hash_store_rows_n, N columns per launch (32 per launch).  For every i < n with 0 <= slots[i] < dst_rows
 * and every move: dst[slots[i] * dst_pitch + j] = src[i * src_pitch + j] for j < words, one lane group per row,
 * the 16-byte rule as above; entries with slots[i] < 0 (a key that did not fit) or >= dst_rows are skipped.
 * Here src is the packed array (an export's) and dst the per-slot array of the table.  An import is an upsert:
 * the caller translates the imported keys with its table's own entry (insert != 0, table == NULL: rows not
 * initialised; an expiring table reuses tombstones by its own walk) and hands the slots to this entry.
 * last_seen and freq travel as moves and overwrite what the expiring insert just stamped, so an imported key
 * keeps its age and count.  Distinct keys have distinct slots, so no two rows race; duplicate slots[] entries
 * are the caller's contract (which of the duplicates' rows stays is then run-dependent, word by word).  Plain
 * loads and stores, no atomics, no workspace, no host synchronisation: capturable.  Refused: n_cols < 0; NULL
 * cols with n_cols > 0; n < 0; NULL slots with n > 0; slots not 8-byte aligned; dst_rows < 0; everything
 * hbk_hash_rehash_n refuses of a move.  n_cols == 0 returns HBK_OK without touching a device.
 *
 * Both entries are detected by the presence of the symbol; the version stays that of 0.2.0. */
typedef struct {
  const int64_t* keys;      /* device [slab_count * slab_size], 8-byte aligned */
  int64_t slab_count;
  int32_t slab_size;        /* 1..64 */
  int32_t expiring;         /* != 0: a TOMBSTONE is skipped; 0: INT64_MIN + 1 is an ordinary key */
  const int32_t* last_seen; /* device int32 [slab_count * slab_size]; may be NULL when since <= 0 */
  int32_t since;            /* <= 0: every key; > 0: the keys with last_seen >= since */
  int32_t n_moves;          /* 0..HBK_HASH_MAX_MOVES */
  hbk_hash_move_t moves[HBK_HASH_MAX_MOVES];   /* src: the per-slot array; dst: the packed array */
  int64_t* out_keys;        /* device int64 [out_capacity] */
  int64_t* out_slots;       /* device int64 [out_capacity] or NULL */
  int64_t out_capacity;     /* >= 0: rows of out_keys, out_slots and every move's dst */
  int64_t* count;           /* device int64[1]: the total number of matches */
} hbk_hash_export_column_t;
int hbk_hash_export_workspace_bytes(int32_t n_cols, const hbk_hash_export_column_t* cols, size_t* bytes);
int hbk_hash_export_n(int32_t n_cols, const hbk_hash_export_column_t* cols, void* workspace, hbk_stream_t stream);

typedef struct {
  const int64_t* slots;     /* device int64 [n]: destination row of packed row i; outside [0, dst_rows): skipped */
  int64_t n;
  int64_t dst_rows;         /* rows of every move's dst */
  int32_t n_moves;          /* 0..HBK_HASH_MAX_MOVES */
  hbk_hash_move_t moves[HBK_HASH_MAX_MOVES];   /* src: the packed array; dst: the per-slot array */
} hbk_hash_store_column_t;
int hbk_hash_store_rows_n(int32_t n_cols, const hbk_hash_store_column_t* cols, hbk_stream_t stream);

/* Spilling: export exactly the keys an eviction removes, then remove them (the reference's EmbeddingService keeps a
 * device cache in front of a larger store and pushes out what it evicts: service.py:153-283).  The evicted keys
 * leave with their rows, their age and count and their optimizer slots, for a host tier to keep; a later import
 * (the table's translate entry and hbk_hash_store_rows_n) brings them back as they left.
 *
 * hbk_hash_spill_n, N expiring tables per call (32 per launch), four launches per 32 tables on the call's stream.
 *
 * Selection.  `selection` is a device int32[4] as hbk_hash_evict_to_select_n writes it: {live_before, need, cut,
 * n_selected}.  It is READ FROM DEVICE MEMORY by the launches: there is no host read anywhere in the call, and it
 * may be stream-ordered right behind the select.  Slot s is SELECTED iff ALL of
 *     keys_cache[s] holds a key (neither EMPTY nor TOMBSTONE)
 *     keep_freq == 0  or  freq[s] < keep_freq
 *     selection[1] > 0            (the need: with need <= 0 the report's cut is 0 and last_seen may well be <= 0,
 *                                  so the need is tested and not only the cut)
 *     last_seen[s] <= selection[2]   as SIGNED int32
 * -- with the keep_freq of the select, exactly the slots hbk_hash_evict_to_n would evict.  selection[0] and [3] are
 * not read.
 *
 * Launches 1-3 are the count, scan and write of hbk_hash_export_n with this predicate, and the contract is that
 * entry's: the selected keys in ASCENDING SOURCE-SLOT ORDER packed from position 0, out_slots (if not NULL) their
 * source slots, every move a bit-for-bit copy (dst[p * dst_pitch + j] = src[s * src_pitch + j], the 16-byte rule
 * as there), nothing written at positions >= out_capacity, *count = the total number of selected slots whatever
 * the capacity; plain loads and stores, no atomics.  *n_evicted (if not NULL) is zeroed by the scan launch, so a
 * captured call replays.
 *
 * Launch 4 is the eviction sweep with the same predicate: what hbk_hash_evict_to_n's sweep does -- key =
 * TOMBSTONE, last_seen = freq = 0, the rows of the n_fills companions = their value, stats[0] (if not NULL) and
 * *n_evicted (if not NULL) += the slots evicted.  ALL OR NOTHING per table: the sweep is guarded by
 * *count <= out_capacity.  A table whose selected keys do not all fit its output is left completely untouched and
 * its n_evicted stays 0: nothing leaves the table that was not exported in full.  The kernel boundary between
 * launches 3 and 4 orders the copies before the resets; a move's src may therefore be a fill's array (an
 * optimizer slot is exported, then reset).
 *
 * If the table changed between the select and the spill the call is still self-consistent -- it evicts exactly
 * what it exports -- just a different set than the select counted: *count says how many.  The table's arrays must
 * not be written by anyone else during the call.
 *
 * Workspace: hbk_hash_spill_workspace_bytes(n_cols, cols, &bytes) reads the geometry of the columns only (8 bytes
 * per 256 slots); one device pointer, 8-byte aligned, not kept after the call.  No host synchronisation:
 * capturable.
 *
 * Refused (HBK_INVALID_ARGUMENT) before any device work: what hbk_hash_evict_to_n refuses of keys_cache,
 * slab_count, slab_size (a table of 2^31 slots or more included) and the fills; NULL last_seen, freq, selection or
 * count; keep_freq < 0; everything hbk_hash_rehash_n refuses of a move; out_capacity < 0; NULL out_keys with
 * out_capacity > 0; a NULL (or not 8-byte aligned) workspace with n_cols > 0.  exp.step is not read, exp.stats may
 * be NULL.  n_cols == 0 returns HBK_OK without touching a device.  Detected by the presence of the symbols; the
 * version stays that of 0.2.0. */
typedef struct {
  int64_t* keys_cache;      /* device [slab_count * slab_size], 8-byte aligned */
  int64_t slab_count;
  int32_t slab_size;        /* 1..64 */
  hbk_hash_expiry_t exp;    /* last_seen and freq are required; step is not read; stats may be NULL */
  const int32_t* selection; /* device int32[4] {live_before, need, cut, n_selected} of hbk_hash_evict_to_select_n */
  int32_t keep_freq;        /* >= 0; 0: frequency keeps nothing.  The select's */
  int32_t n_moves;          /* 0..HBK_HASH_MAX_MOVES */
  hbk_hash_move_t moves[HBK_HASH_MAX_MOVES];   /* src: the per-slot array; dst: the packed array */
  int32_t n_fills;          /* 0..HBK_HASH_MAX_FILLS */
  hbk_hash_fill_t fills[HBK_HASH_MAX_FILLS];   /* the companions the sweep resets */
  int64_t* out_keys;        /* device int64 [out_capacity] */
  int64_t* out_slots;       /* device int64 [out_capacity] or NULL */
  int64_t out_capacity;     /* >= 0: rows of out_keys, out_slots and every move's dst */
  int64_t* count;           /* device int64[1]: the total number of selected slots */
  int32_t* n_evicted;       /* device int32[1]: the slots the sweep evicted (0 when the guard held it back); or NULL */
} hbk_hash_spill_column_t;
int hbk_hash_spill_workspace_bytes(int32_t n_cols, const hbk_hash_spill_column_t* cols, size_t* bytes);
int hbk_hash_spill_n(int32_t n_cols, const hbk_hash_spill_column_t* cols, void* workspace, hbk_stream_t stream);

/* Spilling in LFU order: hbk_hash_spill_n with the selection of hbk_hash_evict_to_lfu_select_n.  Same struct;
 * `selection` points at that entry's device int32[8] {live_before, need, cut_freq, cut_last_seen, n_selected, ...},
 * read from device memory by every launch.  Slot s is SELECTED iff ALL of
 *     keys_cache[s] holds a key;   keep_freq == 0  or  freq[s] < keep_freq;   selection[1] > 0;
 *     (freq[s], last_seen[s]) <= (selection[2], selection[3])   as a pair of SIGNED int32, freq first
 * -- with the keep_freq of the select, exactly the slots hbk_hash_evict_to_lfu_n would evict.  Everything else is
 * hbk_hash_spill_n's contract: count, scan and write of the export with this predicate (ascending source-slot
 * order, packed from 0, nothing behind out_capacity, *count = the total), then the sweep, ALL OR NOTHING per table
 * (guarded by *count <= out_capacity); *n_evicted zeroed by the scan launch; 32 tables per launch; no host read,
 * capturable.  Workspace: hbk_hash_spill_workspace_bytes (the geometry alone decides).  The argument checks and
 * refusal texts are hbk_hash_spill_n's under the name hash_spill_lfu_n, before any device work. */
int hbk_hash_spill_lfu_n(int32_t n_cols, const hbk_hash_spill_column_t* cols, void* workspace, hbk_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Communicator lifecycle: HbGetNcclId / HbCreateNcclCollective /
 * HbIsNcclCollectiveInitialized / async-error polling.
 *     hbtf/distribute/nccl/nccl_get_id.cc:35-62, nccl_create.cc:45-132,
 *     nccl_collective.cc:434-465.  RCCL over xGMI; one communicator + one private comm
 *     stream per handle (hbtf/distribute/nccl/collective.h:41-126).
 *     The 128-byte id travels between ranks by whatever the host has (the reference uses
 *     a TF gRPC broadcast, hbtf/distribute/rpc.py:88-124).                              */
typedef struct hbk_comm* hbk_comm_t;
#define HBK_COMM_ID_BYTES 128
int hbk_comm_get_id(uint8_t id[HBK_COMM_ID_BYTES]);
/* RCCL version codes (major * 10000 + minor * 100 + patch): the headers the library was built
 * against and the RCCL the process actually runs (a framework may have loaded its own first).
 * hbk_comm_create refuses a different MAJOR version; minor skew is fine for the calls used. */
int hbk_comm_rccl_versions(int32_t* built, int32_t* runtime);
int hbk_comm_create(hbk_comm_t* comm, const uint8_t id[HBK_COMM_ID_BYTES],
                    int32_t world_size, int32_t local_size, int32_t rank);
int hbk_comm_destroy(hbk_comm_t comm);
/* 0 = healthy; on an async RCCL error aborts the communicator and returns HBK_INTERNAL */
int hbk_comm_check_async(hbk_comm_t comm);
int hbk_comm_world_size(hbk_comm_t comm);
int hbk_comm_rank(hbk_comm_t comm);
/* ncclCommCount of the RCCL communicator behind the handle: the ranks RCCL itself connected
 * (0: custom transport, -1: error).  Reported by bench.py as `rccl_ranks_seen`. */
int hbk_comm_rccl_ranks(hbk_comm_t comm);
/* the communicator's private stream (a hipStream_t) */
hbk_stream_t hbk_comm_stream(hbk_comm_t comm);
/* R4  Collective::compute_active_ranks, hbtf/distribute/collective.h:80-112.
 *     Writes the peer list for `topology`, returns its length (<= world_size). */
int hbk_comm_active_ranks(hbk_comm_t comm, int32_t topology, int32_t* ranks_out);

/* R5  HbNcclAlltoall / HbNcclAlltoallN (equal split; also the sizes exchange that precedes
 *     every Alltoallv): hbtf/distribute/nccl/nccl_alltoall.cc:169-180,242-258,
 *     nccl_collective.cc:112-248.  counts[c] elements per tensor, divisible by the active
 *     size.  Enqueued on the communicator's stream, fenced after `compute_stream`'s
 *     current tail and before its future work (hbtf/common/stream.cc:83-142).          */
int hbk_alltoall_n(hbk_comm_t comm, int32_t n, int32_t dtype, int32_t topology,
                   const void* const* inputs, const int64_t* counts, void* const* outputs,
                   hbk_stream_t compute_stream);

/* R5/R6  HbNcclAlltoallv / HbNcclAlltoallvN payload exchange.
 *     ops hbtf/distribute/nccl/nccl_alltoallv.cc:200-223,359-387; arithmetic
 *     nccl_collective.cc:250-384: chunk i of inputs[c] starts at
 *     sum_{j<i} send_sizes[c][j]*common_sizes[c] elements, the chunk from peer i lands at
 *     sum_{j<i} recv_sizes[c][j]*common_sizes[c].  Offsets are 64-bit here (the reference's
 *     int32 byte offsets overflow past 2 GiB, nccl_collective.cc:261-262).
 *     send_sizes / recv_sizes are HOST arrays [n][active] (rows); recv_sizes must already
 *     be known (use hbk_alltoall_n on the sizes first -- once for all columns -- as
 *     HbNcclAlltoallvN does, nccl_alltoallv.cc:418-564).
 *     wire_dtype HBK_HALF with dtype HBK_FLOAT casts to fp16 before the send and back
 *     after the receive (collective.py:291-296); `wire_ws` then needs
 *     hbk_alltoallv_wire_workspace_bytes().  wire_dtype == dtype otherwise.             */
size_t hbk_alltoallv_wire_workspace_bytes(int32_t n, const int64_t* common_sizes,
                                          const int32_t* send_sizes,
                                          const int32_t* recv_sizes, int32_t active);
int hbk_alltoallv_n(hbk_comm_t comm, int32_t n, int32_t dtype, int32_t wire_dtype,
                    int32_t topology, const int64_t* common_sizes,
                    const void* const* inputs, const int32_t* send_sizes,
                    void* const* outputs, const int32_t* recv_sizes, void* wire_ws,
                    size_t wire_ws_bytes, hbk_stream_t compute_stream);

/* ------------------------------------------------------------------------------------
 * SURVEY 8f-1  aggregation of replicated gradients (hbtf/training/gradient.py:119-177):
 *   HbNcclAllreduce / HbNcclAllreduceN / HbNcclAllreduceMergedN  (nccl_allreduce.cc:31-260)
 *     outputs[c] = reduce over ranks of inputs[c] (reduce_op 0 SUM, 1 PROD, 2 MAX, 3 MIN), then
 *     multiplied by `scale` (fp32 only; 1/W = the `_mean` of gradient.py:77-99 fused in).  The N
 *     tensors travel as ONE bucket (pack -> one ncclAllReduce -> unpack); in place allowed.
 *   HbNcclAllgatherv  (nccl_allgatherv.cc:31-120)
 *     output = inputs of ranks 0..W-1 concatenated; counts[r] (host, elements) = what rank r
 *     contributes.  The reference op exchanges the counts itself and syncs the host; here the
 *     caller obtains them (one hbk_alltoall_n of its own count). */
size_t hbk_allreduce_workspace_bytes(int32_t n, const int64_t* counts, int32_t dtype);
int hbk_allreduce_n(hbk_comm_t comm, int32_t n, int32_t dtype, int32_t reduce_op,
                    const void* const* inputs, const int64_t* counts, void* const* outputs,
                    float scale, void* workspace, size_t workspace_bytes,
                    hbk_stream_t compute_stream);
int hbk_allgatherv(hbk_comm_t comm, int32_t dtype, const void* input, const int64_t* counts,
                   void* output, hbk_stream_t compute_stream);
/* HbNcclBroadcast (hbtf/distribute/nccl/nccl_broadcast.cc:31-92): every rank ends with the root's
 * `count` elements in `output`; `input` is read on the root only (input == output is allowed).
 * HbNcclAllgather (nccl_allgather.cc:31-101, equal counts) is hbk_allgatherv with every count the
 * same. */
int hbk_broadcast(hbk_comm_t comm, int32_t dtype, const void* input, void* output, int64_t count,
                  int32_t root, hbk_stream_t compute_stream);

/* A communicator over a caller-provided transport instead of RCCL (the reference's Collective is
 * an abstract class with NCCL as one implementation, hbtf/distribute/collective.h:70-201).  Every
 * collective above, and the sharded pipeline below, then moves its data through these callbacks
 * with the same chunk / offset arithmetic as over RCCL:
 *   exchange   chunk k of sendbuf (send_off[k], send_len[k] elements of esize bytes) goes to
 *              ranks[k], the chunk from ranks[k] lands at recv_off[k] elements of recvbuf; all on
 *              `stream`; with skip_self the chunk for `rank` itself is left alone
 *   allreduce  out[i] = reduce over the world's ranks of in[i]  (may be NULL: no allreduce)
 *   destroy    called by hbk_comm_destroy (may be NULL)
 * tests/support builds an in-process world on it (host threads sharing one GPU, device copies);
 * that code is not part of this library. */
typedef struct {
  void* ctx;
  int (*exchange)(void* ctx, int32_t rank, const int32_t* ranks, int32_t n_ranks,
                  const void* sendbuf, const int64_t* send_off, const int64_t* send_len,
                  void* recvbuf, const int64_t* recv_off, size_t esize, int32_t skip_self,
                  hbk_stream_t stream);
  int (*allreduce)(void* ctx, int32_t rank, int32_t world_size, int32_t dtype, int32_t reduce_op,
                   const void* in, void* out, int64_t count, hbk_stream_t stream);
  void (*destroy)(void* ctx);
} hbk_transport_t;
int hbk_comm_create_custom(hbk_comm_t* comm, const hbk_transport_t* transport,
                           int32_t world_size, int32_t local_size, int32_t rank);

/* ------------------------------------------------------------------------------------
 * R12  The whole sharded pipeline of hbtf/embedding/sharding.py:171-205 for N columns in one
 *   call per direction (what the reference's Pack pass + executor run as ~10 ops per column):
 *     forward : bucketize -> partition by id mod W -> alltoallv(ids) -> owner gather (`// W`)
 *               -> alltoallv(rows, fp32 | fp16 wire) -> stitch + combiner
 *     backward: d(stitch+combiner) -> reverse alltoallv (forward's sizes,
 *               hbtf/distribute/collective.py:334-347) -> duplicate-row reduction on the owner
 *               (+ fused SGD on the shard when apply_lr != 0)
 *   One [N x W] size exchange and ONE host sync per forward for all columns (the reference
 *   syncs once per op: nccl_alltoallv.cc:316,533); none in the backward.  Every exchange
 *   is one message per peer (all columns of a peer travel together).  Exchange buffers whose
 *   size depends on the peers are owned by the plan and grow on demand.
 *   ids are int64.  outs[c] is [n_segments[c], dim] ([n_ids[c], dim] when row_splits[c] is
 *   NULL).  The backward differentiates the LAST forward of the plan; its outputs need
 *   capacity hbk_sharded_owned_ids(plan, c) rows (known after that forward).              */
typedef struct {
  const float* shard;   /* device [rows_local, dim]: rows r, r+W, r+2W.. of the logical table */
  int64_t rows_local;
  int32_t dim;
  int32_t combiner;
  int64_t bucket;       /* >0: ids are taken modulo this before the partition (R1) */
  float* accum;         /* Adagrad accumulator of the shard [rows_local, dim], or NULL */
  int32_t hot_rows;     /* != 0: skewed ids expected: the owner gather stages the rows repeated in a
                           tile in LDS (hbk_lookup_column_t.hot_rows; wide columns only) */
  int32_t dedup;        /* != 0: requester-side dedup -- every DISTINCT id of the column's batch is
                           sent once (the reference's tutorials do it in user code in front of the
                           lookup, docs/tutorial/ranking/data.py:180-182): unique over the partitioned
                           ids, exchanges sized by the distinct ids, the stitch reads the received
                           rows through inverse o shard_index, and the backward sums duplicate
                           positions on the requester before the reverse exchange.  Pays when ids
                           repeat inside a batch (Zipf) and the step is link-bound; costs the unique. */
} hbk_sharded_column_t;

/* Host arithmetic of the peer-major exchange buffers (pure host code, no device work): S is
 * [n_cols][world] (rows this rank requests from owner q), R is [world][n_cols] (rows requester q
 * asked this rank for).  Any output pointer may be NULL.  Offsets are in ids / floats. */
int hbk_sharded_layout(int32_t n_cols, int32_t world, const int32_t* dims, const int32_t* S,
                       const int32_t* R, int32_t* ids_send_peer, int32_t* ids_recv_peer,
                       int32_t* rows_send_peer, int32_t* rows_recv_peer, int64_t* req_id_off,
                       int64_t* req_row_off, int64_t* own_id_off, int64_t* own_row_off,
                       int64_t* col_shard_off);

typedef struct hbk_sharded* hbk_sharded_t;
int hbk_sharded_create(hbk_sharded_t* plan, hbk_comm_t comm, int32_t n_cols,
                       const hbk_sharded_column_t* cols, int32_t wire_dtype);
/* Replaces the hot_rows hints of the plan's columns (hbk_sharded_column_t.hot_rows, [n_cols]);
 * the next forward reads them.  (The host side derives them from the distinct rows / ids of the
 * last backward: hybridbackend_amd/embedding/sharded.py.) */
int hbk_sharded_set_hot_rows(hbk_sharded_t plan, const int32_t* hot_rows);
/* max_norm of the plan's columns (host float[n_cols], the values of hbk_group_lookup_fwd_clipped; NULL: no
 * column clipped); kept by the plan until set again.  As in the reference, the OWNER clips: its gather
 * clips every row in fp32 before the wire (and the fp16 cast), the requester's stitch applies the
 * weights; the owner-side backward runs the reduce in its emit form and the clip pass on its shard
 * rows (every optimizer; unique_rows / grad_rows as in hbk_group_lookup_bwd_apply_clipped).  A
 * p2p-bound plan (hbk_sharded_p2p_bind) refuses a forward with a clipped column: HBK_UNIMPLEMENTED
 * before any exchange.  Values are refused as in the clipped entries. */
int hbk_sharded_set_max_norms(hbk_sharded_t plan, const float* max_norms);
/* 16-bit shards (plan state like the max_norms; a new symbol, the structs and the version stay those of 0.2.0).
 * dtypes: host int32 [n_cols], every entry HBK_LOWP_BF16 or HBK_LOWP_FP16 -- cols[c].shard then points at
 * [rows_local, dim] rows of 2-byte elements -- or NULL: the plan is an fp32 plan again, as created.  All or nothing:
 * a plan has 16-bit shards in every column or in none.  `wire` names what crosses the link in the forward:
 *   HBK_LOWP_WIRE_TABLE  the rows in the table's own 16 bits: the owner gather is hbk_lowp_gather_rows_n into the
 *                        send buffer (the element offsets of the fp32 layout, two bytes each, as the fused fp16
 *                        wire addresses it), the row exchange moves 2-byte elements, the stitch is
 *                        hbk_lowp_lookup_fwd_runs over the received rows; the own slice stays in place.  Half the
 *                        wire bytes of fp32 and, unlike the fp16 wire, nothing is rounded.
 *   HBK_LOWP_WIRE_FLOAT  the owner gather is hbk_lowp_lookup_fwd (one id per segment, sum, divisor = W, fp32 out)
 *                        and everything behind it the fp32 path: the twin the 16-bit wire is compared against.
 * Both give hbk_sharded_lookup_fwd over fp32 shards holding the upcast values, bit for bit.  Requester-side dedup,
 * column groups, inline and hopped exchanges, weighted forwards and the prefetch work unchanged; hot_rows hints
 * are ignored; the gradient exchange stays fp32.
 *
 * THE BACKWARD.  hbk_sharded_lookup_bwd[_apply] with apply_lr == 0 (the emit form, which never reads the shard)
 * works unchanged and returns LOCAL row numbers; the caller steps its shards with hbk_lowp_apply_slices_n.  Every
 * entry that steps reads and writes `shard` as fp32 rows of 4 * dim bytes and would run past a 2-byte shard, so on
 * a 16-bit plan each of them is refused by name before any launch or exchange: hbk_sharded_lookup_bwd[_apply] with
 * apply_lr != 0, hbk_sharded_lookup_bwd_adam, _ftrl and _rowwise_adagrad, and hbk_sharded_set_adam_slots,
 * _ftrl_slots and _rowwise_adagrad_slots (HBK_UNIMPLEMENTED).  Also refused on a 16-bit plan:
 * hbk_sharded_lookup_bwd_weights (the received rows are 16-bit), hbk_sharded_p2p_bind, a non-zero max_norm
 * (hbk_sharded_set_max_norms) and a hash column (hbk_sharded_set_hash_tables), each HBK_UNIMPLEMENTED; and this
 * setter itself on a plan created with wire_dtype == HBK_HALF, on a plan with a non-zero max_norm, a hash column
 * or a p2p bind (HBK_UNIMPLEMENTED), with an unknown dtype or wire (HBK_INVALID_ARGUMENT).
 *
 * Stochastic rounding over shards: hbk_lowp_apply_slices_n keys its noise by (seed, step, column, row, element),
 * and the row is the LOCAL row, so two ranks with one seed would round local row r alike.  A caller that steps the
 * shards of rank k seeds that rank with  rank_seed = (seed + 0x9E3779B9 * k) mod 2^32  (what
 * hb.embedding.LowpShardedGroupLookup does). */
#define HBK_LOWP_WIRE_TABLE 0
#define HBK_LOWP_WIRE_FLOAT 1
int hbk_sharded_set_table_dtypes(hbk_sharded_t plan, const int32_t* dtypes /* [n_cols] or NULL */, int32_t wire);
/* Sharded hash tables: columns of the plan whose shard is a hash-keyed table (hbk_hash_column_t above) keyed by
 * the RAW id.  owner = floormod(id, W) as for every column (the partition uses floormod: negative ids have an
 * owner); what changes is the owner's side: instead of row = id // W in a dense shard, the owner TRANSLATES the
 * ids it received into row numbers of its table -- hbk_hash_translate_runs_n over the W runs of the column
 * exactly where the gather would read its ids (the own slice in the outgoing buffer when it stays in place),
 * one call per table kind (and insert flag) present in a column group -- into a plan-owned int64 slot buffer
 * laid out as the received ids.  The owner gather then reads ids = slots, divisor = 1, rows = capacity (a -1
 * reads a zero row), and the owner reduce of the backward (every optimizer) reads the same slots with divisor
 * = 1: unique_rows are SLOT numbers, keys_cache[unique_rows] names the ids, Adagrad / Adam / FTRL slots are
 * [capacity, dim].  The slot buffer lives until the next forward, as the received ids do.
 *
 * tables: host [n_cols], copied; NULL, or all keys_cache NULL: no hash column (today's step, no extra work).
 * tables[c].keys_cache == NULL: column c is an ordinary column.  Otherwise column c's shard is the table's
 * rows ([slab_count * slab_size, dim], dense), and counts, init_scale, seed, exp (exp.last_seen == NULL: not
 * expiring), adm (adm.sketch == NULL: no filter) and insert (0: a pure find, inference) are what the translate
 * call is handed.  Plan state like the max_norms: plan creation is local, every rank sets it for itself, and
 * after a rehash of a table (new arrays) the plan is made again.  Requester-side dedup, the fp16 wire,
 * max_norms, hot_rows, column groups, inline or hopped exchanges and prefetch work unchanged.
 *
 * Refused (HBK_INVALID_ARGUMENT): a hash column with rows_local != slab_count * slab_size, with bucket != 0
 * (ids must reach the owner raw, as int64), with slab_size outside [1, 64] or slab_count < 1, or with
 * exp.last_seen set and exp.freq or exp.step NULL.  HBK_UNIMPLEMENTED: a p2p-bound plan; and
 * hbk_sharded_p2p_bind on a plan with a hash column.  hbk_sharded_lookup_fwd_weighted's rule that a weighted
 * column needs a bucket stands, so id_weights on a hash column are refused. */
typedef struct {
  int64_t* keys_cache;          /* NULL: column c is an ordinary column */
  int64_t slab_count; int32_t slab_size;
  int32_t* counts; float init_scale; int64_t seed;
  hbk_hash_expiry_t exp;        /* exp.last_seen == NULL: not expiring */
  hbk_hash_admission_t adm;     /* adm.sketch == NULL: no filter */
  int32_t insert;               /* 0: pure find (inference) */
} hbk_sharded_hash_t;
int hbk_sharded_set_hash_tables(hbk_sharded_t plan, const hbk_sharded_hash_t* tables /* [n_cols] or NULL */);
/* 16-bit sharded hash tables: hash columns whose tables hold bf16 / fp16 rows.  The two setters above refuse each
 * other -- hbk_sharded_set_hash_tables on a 16-bit plan, hbk_sharded_set_table_dtypes on a plan with a hash column,
 * both as before -- so this ONE setter registers both pieces of state or neither.  Plan state, set right after
 * creation by every rank for itself.
 *   dtypes, wire  as hbk_sharded_set_table_dtypes: all or nothing, every entry HBK_LOWP_BF16 / HBK_LOWP_FP16;
 *                 HBK_LOWP_WIRE_TABLE or HBK_LOWP_WIRE_FLOAT.  The plan becomes a 16-bit plan: everything a 16-bit
 *                 plan refuses stays refused (the stepping entries, the slot setters, hbk_sharded_lookup_bwd_weights,
 *                 hbk_sharded_p2p_bind, a non-zero max_norm; HBK_UNIMPLEMENTED).
 *   tables        as hbk_sharded_set_hash_tables; tables[c].keys_cache == NULL: column c is an ordinary 16-bit
 *                 bucketed column.
 *   tables == NULL or dtypes == NULL: the plan is the fp32 plan without hash columns that it was created as.
 *   (hbk_sharded_set_table_dtypes(plan, NULL, .) on such a plan drops its hash columns with the 16-bit state.)
 * Stage C of the forward: the hash columns of a group are translated by hbk_hash_translate_runs_lowp_n, one call per
 * table kind and insert flag as before, the columns' element codes beside them -- a new row is the fp32 start row
 * rounded to nearest even -- and the virtual columns go to the gathers of the 16-bit plan: hbk_lowp_gather_rows_n
 * onto the 16-bit wire, hbk_lowp_lookup_fwd for HBK_LOWP_WIRE_FLOAT, a hash column with ids = the translated slots,
 * HBK_INT64, divisor = 1.  A -1 slot is a zero row on both wires.  The emit backward (slot numbers; nothing is sent
 * for -1), the split forward _ids / _gather / _end and hbk_sharded_hash_missing (whose find writes no row) are
 * unchanged; the caller steps the tables with hbk_lowp_apply_slices_n over [capacity, dim] fp32 slots.
 *
 * Refused before the plan changes.  HBK_UNIMPLEMENTED: a plan created with wire_dtype == HBK_HALF, a plan with a
 * non-zero max_norm, a p2p-bound plan.  HBK_INVALID_ARGUMENT: an unknown dtype or wire, a shard that is not 2-byte
 * aligned; everything hbk_sharded_set_hash_tables refuses of a hash column; and of a hash column also an odd dim (new
 * rows are whole 4-byte words), dim > 64 with dim % 4 != 0 (the bound of the 16-bit gathers without wide_rows), a
 * shard that is not 4-byte aligned, HBK_LOWP_FP16 with init_scale > 65504.  Detected by the presence of the symbol;
 * the structs and the version are those of 0.2.0. */
int hbk_sharded_set_lowp_hash_tables(hbk_sharded_t plan, const hbk_sharded_hash_t* tables /* [n_cols] or NULL */,
                                     const int32_t* dtypes /* [n_cols] or NULL */, int32_t wire);
int hbk_sharded_destroy(hbk_sharded_t plan);
/* out_strides / grad_strides: NULL, or per column the row stride in floats of outs[c] /
 * grads[c] (0 = dim): the columns' blocks of one concatenated [segments, sum of dims] tensor. */
int hbk_sharded_lookup_fwd(hbk_sharded_t plan, const int64_t* const* ids, const int64_t* n_ids,
                           const int32_t* const* row_splits, const int64_t* n_segments,
                           float* const* outs, const int32_t* out_strides, hbk_stream_t stream);
/* The weighted forward (tf.nn.embedding_lookup_sparse's sp_weights; hbk_lookup_column_t.id_weights):
 * id_weights[c] is column c's device fp32 [n_ids[c]] (one weight per id) or NULL (unweighted); a NULL
 * array = hbk_sharded_lookup_fwd.  Weights never cross the wire: the owners gather plain rows and the
 * requester's stitch applies them.  The plan keeps the pointers for hbk_sharded_lookup_bwd[_apply]
 * (its stitch backward writes the weighted per-id terms; under dedup the duplicate positions sum
 * those), so the caller keeps them valid and unchanged until that backward, as with the ids; a plain
 * hbk_sharded_lookup_fwd (or _begin) clears them.  The stitch sees the received rows, not the owners'
 * range checks, so a weighted column needs a bucket (hbk_sharded_column_t.bucket > 0: every id then
 * names a row of its owner's shard, and the results equal hbk_group_lookup_fwd's over the logical
 * table); a weighted column without one is refused with HBK_INVALID_ARGUMENT before any exchange.
 * A p2p-bound plan (hbk_sharded_p2p_bind) has no stitch: HBK_UNIMPLEMENTED on every rank, before any
 * exchange, when some weight pointer is non-NULL.  _begin / _end take no weights. */
int hbk_sharded_lookup_fwd_weighted(hbk_sharded_t plan, const int64_t* const* ids,
                                    const int64_t* n_ids, const int32_t* const* row_splits,
                                    const int64_t* n_segments, const float* const* id_weights,
                                    float* const* outs, const int32_t* out_strides,
                                    hbk_stream_t stream);
/* The forward in two halves (round 5).  _begin: everything up to and including the owner-side
 * gather (the partition or its prefetched result, the step's one host wait, the id exchange, the
 * gather into the reply buffer -- in the p2p form into the requesters' outputs).  _end: rows
 * exchange + stitch + combiner into `outs`.  hbk_sharded_lookup_fwd = _begin + _end.  Two plans
 * over ONE communicator that alternate  begin(B, step i + 1); end(A, step i)  put the ids of step
 * i + 1 on the wire AHEAD of the rows of step i: B gathers while A's rows travel, A stitches while
 * B's travel -- exchanges overlapped with the local gather across steps (hb.embedding.
 * PipelinedLookup).  Forward-only use: nothing may change the tables between a step's _begin and
 * its _end; every rank makes the same calls in the same order. */
int hbk_sharded_lookup_fwd_begin(hbk_sharded_t plan, const int64_t* const* ids,
                                 const int64_t* n_ids, const int32_t* const* row_splits,
                                 const int64_t* n_segments, hbk_stream_t stream);
int hbk_sharded_lookup_fwd_end(hbk_sharded_t plan, float* const* outs, const int32_t* out_strides,
                               hbk_stream_t stream);
/* The first half in two parts, so that the owner of a bounded hash table gets its chance between them:
 * hbk_sharded_lookup_fwd_begin = hbk_sharded_lookup_fwd_ids + hbk_sharded_lookup_fwd_gather, the same launches and
 * exchanges in the same order and the same host-time report.
 *   _ids     everything through the id exchanges of all column groups: partition or a matching prefetch, the
 *            step's one host wait, layouts, run tables, pack, exchanges.  hbk_sharded_owned_ids(plan, c) is valid
 *            from here on.
 *   _gather  the owner side: the translate of the hash columns, the owner gather and, where the exchanges run on
 *            the communicator's stream, the events.
 * hbk_sharded_hash_missing is valid only between the two.  For every column c with want[c] != 0 -- a hash column
 * with an expiring table -- it runs hbk_hash_missing_runs_n over the W runs of ids this rank received for the
 * column, peer after peer, where the translate would read them (the own slice in the outgoing buffer when it stayed
 * in place): out_ids[c][0 .. min(counts[c], out_capacity[c])) holds the distinct received ids the table does not
 * hold, first occurrence first, and counts[c] (device int64 [n_cols]; written for wanted columns only) their number.
 * The find's answers go to the plan's slot buffer, which the translate overwrites; the workspace is the plan's.
 * Where the exchanges run on the communicator's stream, `stream` first waits for the id exchange of the wanted
 * columns' groups.  No host synchronisation.  out_ids, out_capacity and counts are read only at wanted columns.
 *
 * Between _ids and _gather the caller may change the tables in ways that move no tensor (hbk_hash_store_rows_n
 * behind an insert: bringing spilled rows back), stream-ordered on the step's stream: the translate then finds
 * the rows instead of inserting fresh ones.  Nothing here is a collective beyond what _begin is: ranks need not
 * agree on whether anything was missed.
 *
 * Refused, naming the call: _gather or hbk_sharded_hash_missing without an open _ids step; _end before _gather;
 * want[c] != 0 on a column that is not a hash column with an expiring table (HBK_INVALID_ARGUMENT); _ids and
 * hbk_sharded_hash_missing on a p2p-bound plan (HBK_UNIMPLEMENTED).  A new _ids, _begin or hbk_sharded_lookup_fwd
 * drops an open step.  Detected by the presence of the symbols; the version stays that of 0.2.0. */
int hbk_sharded_lookup_fwd_ids(hbk_sharded_t plan, const int64_t* const* ids, const int64_t* n_ids,
                               const int32_t* const* row_splits, const int64_t* n_segments,
                               hbk_stream_t stream);
int hbk_sharded_lookup_fwd_gather(hbk_sharded_t plan, hbk_stream_t stream);
int hbk_sharded_hash_missing(hbk_sharded_t plan, const uint8_t* want /* [n_cols] */, int64_t* const* out_ids,
                             const int64_t* out_capacity, int64_t* counts /* device [n_cols] */,
                             hbk_stream_t stream);
/* Optional pipelining hint: partition + size exchange (stages 1-2) of a FUTURE step on the plan's
 * own stream, overlapping what the last forward still has in flight (its exchanges, gather and
 * stitch).  The next hbk_sharded_lookup_fwd with the same id pointers and counts uses it and
 * skips its own stages 1-2; any other forward drops it.  All ranks must prefetch the same steps;
 * the ids must stay valid and unchanged until that forward. */
int hbk_sharded_prefetch(hbk_sharded_t plan, const int64_t* const* ids, const int64_t* n_ids,
                         void* ids_ready_event /* hipEvent_t recorded after the ids were written,
                                                  or NULL when they are complete already */);
/* The same on a stream of the caller's (round 5): no stream of the plan is involved; the caller
 * enqueues it behind the end of the step BEFORE the last one begun on this plan (stream order is
 * the only protection the overwritten partition state gets).  Used by hb.embedding.PipelinedLookup
 * right behind a step's _begin. */
int hbk_sharded_prefetch_on(hbk_sharded_t plan, const int64_t* const* ids, const int64_t* n_ids,
                            hbk_stream_t stream);
int64_t hbk_sharded_owned_ids(hbk_sharded_t plan, int32_t column);

/* The p2p form of the forward (round 5).  hbk_sharded_p2p_bind registers this rank's N output
 * tensors ([n_ids[c], dim] fp32, out_strides as in hbk_sharded_lookup_fwd; NULL = dense) -- a
 * COLLECTIVE over the plan's communicator: every rank calls it with its own tensors, the addresses
 * are exchanged once and mapped into every peer (ranks of one process -- told apart by pid + host
 * boot id + a per-process random number, since pids repeat across containers: the pointer itself,
 * with hipDeviceEnablePeerAccess when they sit on different devices; other processes of the same
 * host: hipIpcGetMemHandle / hipIpcOpenMemHandle).  out_rows[c] = rows of outs[c]: a later forward
 * with more ids than that is refused (remote owners would store outside the tensor).  From then on hbk_sharded_lookup_fwd --
 * which must be handed exactly these tensors, one id per segment -- sends (id, output row) pairs and
 * the owner-side gather stores every row straight into its place in the requester's output: no
 * reply buffer, no rows Alltoallv, no stitch (one random-row pass instead of two; the rows cross the
 * link as the gather's own stores, so the gather IS the exchange); the ids still travel through the
 * communicator, and a one-int token per peer orders the requester behind the owners' stores.  The
 * exchange form stays the contract default (hbtf/embedding/sharding.py:171-205 composes the same
 * result); requester-side dedup and the fp16 wire are not available in this form.  The backward is
 * unchanged.  HBK_UNIMPLEMENTED on every rank when some peer's memory cannot be mapped; the plan
 * then keeps the exchange form.  hbk_sharded_p2p_unbind returns to it (not collective). */
int hbk_sharded_p2p_bind(hbk_sharded_t plan, float* const* outs, const int32_t* out_strides,
                         const int64_t* out_rows, hbk_stream_t stream);
int hbk_sharded_p2p_unbind(hbk_sharded_t plan);
/* diagnostics: host time of the plan's last forward in microseconds -- [0] enqueueing the
 * partition and the size exchange, [1] waiting for the sizes (the device, not host work),
 * [2] enqueueing everything else */
int hbk_sharded_last_host_us(hbk_sharded_t plan, float* out3);
/* The gradient of the per-id weights of the last hbk_sharded_lookup_fwd_weighted, computed on the requester
 * (the weights never cross the wire) by hbk_group_lookup_bwd_weights' kernel over the rows this rank
 * RECEIVED: e_j is exactly what the forward's stitch multiplied -- clipped by its owner, rounded to fp16 on
 * an fp16 wire -- found through the stitch's index, so duplicate positions of a deduplicated column share
 * one received row.  grad_weights[c]: device fp32 [n_ids of column c] or NULL = not wanted; grads /
 * grad_strides as in hbk_sharded_lookup_bwd.  The received rows live in the plan's exchange buffer until
 * the next forward (_begin) lays it out again or the row backward writes the gradient rows over them; a
 * prefetch does not touch them.  So the call is made after the forward and BEFORE the row backward of the
 * same step; anywhere else it is refused (HBK_INVALID_ARGUMENT), nothing is copied and nothing is kept
 * for a plan that never asks (no opt-in switch is needed).  Local work: no exchange, ranks need not agree on
 * which columns they ask for.  Refused before any launch: a p2p-bound plan (HBK_UNIMPLEMENTED on every
 * rank: no stitch), a wanted column the last forward gave no weights, no forward before it. */
int hbk_sharded_lookup_bwd_weights(hbk_sharded_t plan, const float* const* grads,
                                   const int32_t* grad_strides, float* const* grad_weights,
                                   hbk_stream_t stream);
int hbk_sharded_lookup_bwd(hbk_sharded_t plan, const float* const* grads,
                           const int32_t* grad_strides, float apply_lr,
                           int64_t* const* unique_rows, float* const* grad_rows,
                           int32_t* const* n_unique, hbk_stream_t stream);
/* the same with the optimizer named (HBK_APPLY_SGD | HBK_APPLY_ADAGRAD, see
 * hbk_group_lookup_bwd_apply); Adagrad uses the columns' `accum` shards.  unique_rows and grad_rows
 * may both be NULL when apply_lr != 0 (step only: no IndexedSlices are written). */
int hbk_sharded_lookup_bwd_apply(hbk_sharded_t plan, const float* const* grads,
                                 const int32_t* grad_strides, int32_t apply, float apply_lr,
                                 int64_t* const* unique_rows, float* const* grad_rows,
                                 int32_t* const* n_unique, hbk_stream_t stream);
/* Lazy Adam on the shards (hbk_group_lookup_bwd_adam): hbk_sharded_set_adam_slots registers every
 * column's first / second moment shard ([rows_local, dim], as the column's shard; the columns' accum
 * must be NULL), then hbk_sharded_lookup_bwd_adam runs the owner-side reduce in its emit form and the
 * apply, launch group by launch group; only the last group finishes the powers.  unique_rows and
 * grad_rows may both be NULL (step only). */
int hbk_sharded_set_adam_slots(hbk_sharded_t plan, float* const* m, float* const* v);
int hbk_sharded_lookup_bwd_adam(hbk_sharded_t plan, const float* const* grads,
                                const int32_t* grad_strides, const hbk_adam_t* adam, float lr,
                                int64_t* const* unique_rows, float* const* grad_rows,
                                int32_t* const* n_unique, hbk_stream_t stream);
/* FTRL on the shards (hbk_group_lookup_bwd_ftrl), as the Lazy Adam pair: hbk_sharded_set_ftrl_slots
 * registers every column's accum / linear shard ([rows_local, dim], as the column's shard; the
 * columns' accum must be NULL), then hbk_sharded_lookup_bwd_ftrl runs the owner-side reduce in its emit
 * form and the apply, launch group by launch group.  unique_rows and grad_rows may both be NULL (step
 * only). */
int hbk_sharded_set_ftrl_slots(hbk_sharded_t plan, float* const* accum, float* const* linear);
int hbk_sharded_lookup_bwd_ftrl(hbk_sharded_t plan, const float* const* grads,
                                const int32_t* grad_strides, const hbk_ftrl_t* ftrl, float lr,
                                int64_t* const* unique_rows, float* const* grad_rows,
                                int32_t* const* n_unique, hbk_stream_t stream);
/* Row-wise Adagrad on the shards (hbk_group_lookup_bwd_rowwise_adagrad), as the Lazy Adam pair:
 * hbk_sharded_set_rowwise_adagrad_slots registers every column's accumulator shard ([rows_local, 1]; the
 * columns' accum must be NULL), then hbk_sharded_lookup_bwd_rowwise_adagrad runs the owner-side reduce in its
 * emit form and the apply, launch group by launch group.  Hash plans and max_norms as there; unique_rows and
 * grad_rows may both be NULL (step only). */
int hbk_sharded_set_rowwise_adagrad_slots(hbk_sharded_t plan, float* const* accum);
int hbk_sharded_lookup_bwd_rowwise_adagrad(hbk_sharded_t plan, const float* const* grads,
                                           const int32_t* grad_strides,
                                           const hbk_rowwise_adagrad_t* rowwise_adagrad, float lr,
                                           int64_t* const* unique_rows, float* const* grad_rows,
                                           int32_t* const* n_unique, hbk_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* HBK_H_ */
