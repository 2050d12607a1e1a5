/*
 * gpuq.h — C-ABI of the MI355X-native columnar execution engine (libgpuq.so).
 *
 * This is the drop-in boundary beneath Spark's columnar plugin API: a Scala
 * host layer (SparkSessionExtensions.injectColumnar + ColumnarRule,
 * sql/core/src/main/scala/org/apache/spark/sql/SparkSessionExtensions.scala:168
 * and sql/core/.../execution/Columnar.scala:36-50) binds these entry points
 * over JNI and swaps SortExec / HashAggregateExec / ShuffledHashJoinExec /
 * ShuffleExchangeExec for GPU exec nodes whose doExecuteColumnar() calls
 * land here. The JNI stub a Spark maintainer would add is shown in
 * INTEGRATION.md; in this repo the same ABI is driven by the Python host
 * mirror (spark_amd/) used for tests and benchmarks.
 *
 * Conventions:
 *  - all device pointers are raw HIP device pointers on the CALLER's current
 *    HIP device; `stream` is a hipStream_t (pass 0 for the default stream).
 *    One executor task = one stream; calls are thread-safe per stream.
 *  - the caller owns every buffer, including scratch workspaces, sized via
 *    the gpuq_*_workspace_bytes() helpers. No allocation inside libgpuq.
 *  - column buffers follow the Arrow layout used by Spark's ColumnVector
 *    API (sql/catalyst/src/main/java/org/apache/spark/sql/vectorized/
 *    ColumnVector.java:58-366): a dense data buffer plus an optional
 *    validity bitmap (1 bit/row, LSB-first; NULL bitmap ptr = no nulls).
 *  - return value: 0 on success, non-zero error code; gpuq_last_error()
 *    returns a thread-local message (mapped to exceptions by the host,
 *    mirroring SparkOutOfMemoryError semantics for device OOM).
 */
#ifndef GPUQ_H
#define GPUQ_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- error handling ---- */
#define GPUQ_OK 0
#define GPUQ_ERR_HIP 1          /* underlying HIP call failed           */
#define GPUQ_ERR_INVALID 2      /* bad argument / unsupported combo     */
#define GPUQ_ERR_OVERFLOW 3     /* hash table or output buffer overflow */

const char* gpuq_last_error(void);
int gpuq_device_count(void);

/* ---- optional per-kernel profiling (bench roofline evidence) ----
 * When enabled, each kernel launch is bracketed by HIP events on its own
 * stream; gpuq_kernel_stats synchronizes pending events and returns the
 * accumulated GPU time and launch count for a kernel tag (e.g.
 * "radix_scatter", "radix_hist", "agg_build", "join_probe"). */
void gpuq_profiling(int enable);
void gpuq_kernel_stats_reset(void);
int gpuq_kernel_stats(const char* name, double* total_ms, long long* count);

/* ---- dtypes ---- */
#define GPUQ_INT64 0
#define GPUQ_FLOAT64 1
#define GPUQ_INT32 2

/* One column of a ColumnarBatch (ColumnarBatch.java:61-123 access contract,
 * device-resident). */
typedef struct gpuq_col {
  void* data;                 /* device ptr to dense values              */
  const uint8_t* validity;    /* device ptr to Arrow validity bitmap or NULL */
  int32_t dtype;              /* GPUQ_* */
} gpuq_col;

/* ---------------------------------------------------------------- */
/* Synthetic data generation (bench only; bit-identical to the CPU  */
/* oracle's splitmix64 generator — DESIGN.md §data).                 */
/* ---------------------------------------------------------------- */
int gpuq_gen_i64_range(void* stream, uint64_t seed, uint64_t start,
                       int64_t nrows, uint64_t range, int64_t* out);
int gpuq_gen_f64_unit(void* stream, uint64_t seed, uint64_t start,
                      int64_t nrows, double* out);

/* RangeExec scan feed (basicPhysicalOperators.scala:630):
 * out[i] = start + i*step */
int gpuq_range_i64(void* stream, int64_t nrows, int64_t start, int64_t step,
                   int64_t* out);

/* ---------------------------------------------------------------- */
/* SORT — replaces SortExec (execution/SortExec.scala:75-126): the   */
/* radix-eligible single-key path (canUseRadixSort, SortExec.scala   */
/* :82-83) over an int64 or float64 key column. Produces the sorted  */
/* row permutation; gather materializes payload columns.             */
/* Key encoding on device matches PrefixComparators.java:66-83       */
/* (double bijection) / SignedPrefixComparator (int64); sort is an   */
/* LSB radix over 8-bit digits with the reference's skip-uniform-    */
/* byte optimization (RadixSort.java:108-139) and is STABLE (ties    */
/* keep row order, as the reference's (prefix,pointer) sort does).   */
/* NULL keys are placed per nulls_first in input order               */
/* (SortOrder.scala:35-45 defaults: asc=>first, desc=>last).         */
/* ---------------------------------------------------------------- */

/* workspace bytes for gpuq_sort_perm at nrows (nrows < 2^32) */
int64_t gpuq_sort_workspace_bytes(int64_t nrows);

/* Sort one key column; writes the sorted permutation (row ids into the
 * input) to out_perm[nrows] (uint32) and, if out_keys != NULL, the sorted
 * key column. With key.validity set, NULL rows are placed per nulls_first
 * in input order and out_keys carries the input's raw values at those
 * positions (callers track NULL-ness via the permuted validity).
 * The key column is read more than once during the call (a histogram
 * pre-pass, then the first radix pass, and again if the sort redoes itself),
 * so it must not change until the work this call put on the stream has
 * finished; it is never written. An
 * out_keys that overlaps the key column is allowed: it selects the path that
 * first materialises an encoded copy of the keys in the workspace. */
int gpuq_sort_perm(void* stream, int64_t nrows, gpuq_col key,
                   int32_t desc, int32_t nulls_first,
                   uint32_t* out_perm, void* out_keys,
                   void* workspace, int64_t workspace_bytes);

/* Pass plan of the last gpuq_sort_perm on the calling thread. With wide keys
 * the sort radixes only the leading window of active key bytes (enough
 * changed bits to almost totally order nrows) and resolves the remaining
 * ties in one streaming pass: window_passes is the number of radix passes
 * that plan ran and deferred_bytes the number of active low bytes it left to
 * the tie-fix. deferred_bytes == 0 means the classic all-active-bytes plan
 * ran (window_passes is 0 then). fell_back == 1 means the tie-fix met an
 * unsorted run longer than its limit and the sort was redone with the
 * classic plan; window_passes/deferred_bytes then describe the plan that was
 * tried. GPUQ_SORT_NO_PREFIX (env, read per call) forces the classic plan.
 * Any pointer may be NULL. */
void gpuq_sort_last_plan(int* window_passes, int* deferred_bytes, int* fell_back);

/* ---------------------------------------------------------------- */
/* TOP-K — the selection under TakeOrderedAndProjectExec             */
/* (execution/limit.scala): the rows of the first k positions of the */
/* sort order, found by an MSB radix select over the sort's own key  */
/* encodings instead of a full sort. Let S be the stable order       */
/* gpuq_sort_perm(key, desc, nulls_first) produces (float64: -0.0 == */
/* 0.0, all NaNs equal and greatest; NULLs one group, first or last  */
/* per nulls_first) and T the group of rows equal in that order that */
/* holds position min(k, nrows) - 1 of S. T may be the NULL group.   */
/* ---------------------------------------------------------------- */

/* workspace bytes for gpuq_topk_candidates at nrows; pure arithmetic */
int64_t gpuq_topk_workspace_bytes(int64_t nrows);

/* Writes the candidate row ids to out_rids in ASCENDING row-id (input)
 * order, so a stable sort of the gathered candidates reproduces the head of
 * S exactly, and sets out_counts = {n_cand, n_before, n_tie} (HOST int64[3]):
 * n_before rows sort strictly before T, n_tie = |T|.
 *  - keep_ties == 0: the n_before rows before T plus the first
 *    min(k, nrows) - n_before rows of T in input order, so n_cand ==
 *    min(k, nrows) and the candidates are exactly the rows of S[:k].
 *  - keep_ties == 1: the rows before T plus all of T, n_cand == n_before +
 *    n_tie (for callers whose further sort keys break the tie).
 * out_counts is always set. If n_cand > out_capacity nothing is written and
 * GPUQ_ERR_OVERFLOW is returned (call again with n_cand entries), the
 * convention of gpuq_join_probe_keys; the counts are known on the host
 * before the emit kernels are launched. k <= 0 or nrows == 0 gives {0,0,0}
 * and GPUQ_OK with nothing launched. nrows > 0xFFFFFFFF, a dtype other than
 * int64/float64 or a short workspace return GPUQ_ERR_INVALID before anything
 * is launched.
 * The key column (and its validity bitmap) is read several times during the
 * call — once per select level until the surviving bucket has been copied to
 * the workspace, then twice by the emit — with host synchronisations in
 * between, so it must not change until the call returns; it is never
 * written. */
int gpuq_topk_candidates(void* stream, int64_t nrows, gpuq_col key,
                         int32_t desc, int32_t nulls_first, int64_t k,
                         int32_t keep_ties,
                         uint32_t* out_rids, int64_t out_capacity,
                         int64_t* out_counts /* HOST int64[3] */,
                         void* workspace, int64_t workspace_bytes);

/* out[i] = col[perm[i]] — payload materialization after sort/partition. */
int gpuq_gather(void* stream, int64_t nrows, gpuq_col col,
                const uint32_t* perm, void* out);

/* two 8-byte columns through one permutation in one kernel */
int gpuq_gather2_i64(void* stream, int64_t nrows, const void* a, const void* b,
                     const uint32_t* perm, void* out_a, void* out_b);

/* two 8-byte columns through one permutation via an interleaved staging
 * buffer (scratch: nrows * 16 B device): one streaming interleave pass,
 * then ONE random b128 load per row serving both columns — halves the
 * random-request count and line amplification of the plain two-column
 * gather. */
int gpuq_gather2_i64_fast(void* stream, int64_t nrows, const void* a,
                          const void* b, const uint32_t* perm,
                          void* out_a, void* out_b, void* scratch);

/* the two halves separately: the interleave depends only on the payload
 * columns, so a host can run it on a SIDE stream concurrently with the
 * sort passes and hide it entirely (event-sync before the pairs gather) */
int gpuq_interleave2_i64(void* stream, int64_t nrows, const void* a,
                         const void* b, void* pairs);
int gpuq_gather2_pairs(void* stream, int64_t nrows, const void* pairs,
                       const uint32_t* perm, void* out_a, void* out_b);

/* ---------------------------------------------------------------- */
/* HASH AGGREGATE — replaces HashAggregateExec                       */
/* (execution/aggregate/HashAggregateExec.scala:99-151) for          */
/* GROUP BY int64 key -> SUM(float64) / COUNT. Open-address table    */
/* (the GPU analog of BytesToBytesMap, core/.../unsafe/map/          */
/* BytesToBytesMap.java:50-56) keyed by Murmur3(key,42), linear      */
/* probe, device-scope atomics. SUM accumulation order is device     */
/* order => float64 parity within 1e-6 relative (north star); keys   */
/* and COUNT bit-exact. NULL keys form one group; NULL values are    */
/* skipped (Sum.scala:113-141).                                      */
/* ---------------------------------------------------------------- */

/* capacity must be a power of two >= 2 * expected distinct groups.   */
int64_t gpuq_hash_agg_workspace_bytes(int64_t capacity);

/* aggregate ops bitmask */
#define GPUQ_AGG_SUM 1
#define GPUQ_AGG_COUNT 2

/* Aggregate nrows of (key,val) into the workspace table, then compact:
 * writes ngroups rows of (key, key_valid, sum, sum_valid, count) into the
 * caller's output arrays (each sized for max possible groups) and returns
 * the group count via *out_ngroups. Emission order is nondeterministic
 * (the parity checker is order-insensitive, as QueryTest.checkAnswer is).
 * Multiple (key,val) batches can be accumulated before compaction:
 * pass finalize=0 to accumulate only, finalize=1 to also compact.
 * ops: GPUQ_AGG_* bitmask; SUM-only mode (no COUNT) requires non-null
 * values (sum NULL-ness tracking needs COUNT) and allows out_counts=NULL. */
int gpuq_hash_agg_i64_f64(void* stream, int64_t nrows,
                          gpuq_col key, gpuq_col val,
                          void* workspace, int64_t capacity, int32_t first_batch,
                          int32_t finalize, int32_t ops,
                          int64_t* out_keys, uint8_t* out_key_valid,
                          double* out_sums, uint8_t* out_sum_valid,
                          int64_t* out_counts, int64_t* out_ngroups);

/* Partitioned aggregation: same results contract as gpuq_hash_agg_i64_f64
 * for a single batch with NON-NULL values — rows are bucket-partitioned
 * by 13 Murmur bits in ONE non-stable pass (histogram + per-block range
 * reservation + contiguous per-bucket runs), then each 16 K-row chunk
 * aggregates in an LDS table that flushes to the global table mid-chunk
 * if a skewed/boundary chunk overflows it; sidesteps the global-atomic
 * throughput wall at mid/high cardinality and never needs a fallback. */
int64_t gpuq_hash_agg_part_workspace_bytes(int64_t nrows, int64_t capacity);
int gpuq_hash_agg_partitioned(void* stream, int64_t nrows,
                              gpuq_col key, gpuq_col val,
                              void* workspace, int64_t capacity, int32_t ops,
                              int64_t* out_keys, uint8_t* out_key_valid,
                              double* out_sums, uint8_t* out_sum_valid,
                              int64_t* out_counts, int64_t* out_ngroups);

/* Multi-aggregate: one pass computing up to 12 accumulator words per group
 * (HashAggregateExec evaluates a list of aggregate expressions,
 * HashAggregateExec.scala:68-76 — e.g. TPC-H Q1's 8 aggregates).
 * spec_ops[j]: 0=SUM(float64 col), 1=COUNT(col), 2=COUNT(*),
 * 3=SUM(int64 col) -> int64 (Sum.scala LongType result; non-ansi
 * overflow wraps), 4=MIN(int64), 5=MAX(int64), 6=MIN(float64),
 * 7=MAX(float64) (Min/Max.scala; float64 order = the sort's and the window
 * functions': NaN greatest and all NaNs equal, -0.0 == 0.0; a zero result
 * is emitted as +0.0 and a NaN result as the canonical NaN. This deviates
 * from Spark's Double.compare, which puts -0.0 below 0.0: a group whose
 * extreme is -0.0 returns +0.0 here and -0.0 in Spark);
 * up to 12 specs; spec_cols[j] indexes vals[] (ignored for COUNT(*)). out_accs[j] is a
 * device array per spec: f64 for SUM_F64/MIN_F64/MAX_F64, i64 otherwise.
 * Small tables (cap*(1+nspecs)*8 <= 64 KB) aggregate per-block in LDS
 * first. Value ops skip NULL rows; an all-NULL group emits the op's
 * neutral init (0 for SUM/COUNT, extremes for MIN/MAX) — pair with a
 * COUNT spec to realize SQL NULL results (Sum.scala: NULL iff no
 * non-null input).
 *
 * Exact decimal SUM (Sum.scala's Decimal path for decimal(p<=18,s) carried
 * as scaled int64; result decimal(min(38,p+10),s)): a 128-bit accumulator
 * held in TWO adjacent specs, so each decimal sum costs 2 of the 12 specs.
 *   8=SUM_DEC128(int64 col): the lo word; must be followed immediately by 9.
 *   9=DEC128_HI: the hi word of the preceding spec (8 or 10); its own
 *     update is a no-op. After op 8 its spec_cols entry is ignored.
 *  10=MERGE_DEC128: final-mode merge of 128-bit partials; spec_cols[j] is
 *     the partial lo column (int64 bits) and the following op 9's
 *     spec_cols[j+1] is the partial hi column (int64).
 * out_accs[j] receives lo as int64 bits and out_accs[j+1] hi as signed
 * int64: value = (hi << 64) | (uint64)lo, two's complement, wrapping only
 * at 2^127. NULL rows are skipped by the validity bitmap of the op-8 column
 * (op 10: of the partial lo column); an all-NULL group emits (0, 0) — pair
 * with a COUNT spec as for the other ops. A pairing violation (8/10 last or
 * not followed by 9, 9 not preceded by 8/10) or a non-int64 column returns
 * GPUQ_ERR_INVALID before anything is launched. */
int64_t gpuq_hash_agg_multi_workspace_bytes(int64_t capacity, int32_t nspecs);
int gpuq_hash_agg_multi(void* stream, int64_t nrows, gpuq_col key,
                        const gpuq_col* vals, const int32_t* spec_ops,
                        const int32_t* spec_cols, int32_t nspecs,
                        void* workspace, int64_t capacity,
                        int32_t first_batch, int32_t finalize,
                        int64_t* out_keys, uint8_t* out_key_valid,
                        void* const* out_accs, int64_t* out_ngroups);

/* Composite-key aggregate: GROUP BY (k1..kK), K <= 4 int64 columns with
 * independent NULLability (the reference groups by an UnsafeRow key tuple,
 * UnsafeFixedWidthAggregationMap.java:39). Slots claim by CAS + publish;
 * tuple equality is verified against stored keys, so the full domain is
 * exact. out_keys[c]: device i64 array per key column; out_kmask: one byte
 * per group, bit c = key column c non-NULL. Same spec_ops as
 * gpuq_hash_agg_multi. */
int64_t gpuq_hash_agg_keys_workspace_bytes(int64_t capacity, int32_t nkeys,
                                           int32_t nspecs);
int gpuq_hash_agg_keys(void* stream, int64_t nrows,
                       const gpuq_col* key_cols, int32_t nkeys,
                       const gpuq_col* vals, const int32_t* spec_ops,
                       const int32_t* spec_cols, int32_t nspecs,
                       void* workspace, int64_t capacity,
                       int32_t first_batch, int32_t finalize,
                       void* const* out_keys, uint8_t* out_kmask,
                       void* const* out_accs, int64_t* out_ngroups);

/* ---------------------------------------------------------------- */
/* PARTITION — replaces ShuffleExchangeExec's partition-id + write   */
/* path (exchange/ShuffleExchangeExec.scala:357-470 +                */
/* core/src/main/java/.../shuffle/sort/UnsafeShuffleWriter.java):    */
/* pid = Pmod(Murmur3Hash(key,42), n) (partitioning.scala:328-330),  */
/* stable radix-partition into per-partition contiguous runs. The    */
/* cross-GPU exchange itself is RCCL all-to-all over xGMI, driven by */
/* the host layer (torch.distributed / ncclGroup of send-recv) on    */
/* the per-partition runs this produces.                             */
/* ---------------------------------------------------------------- */

int64_t gpuq_partition_workspace_bytes(int64_t nrows, int32_t num_parts);

/* Computes the stable permutation that groups rows by partition id and the
 * per-partition row counts. out_perm[nrows] (uint32), out_counts[num_parts]
 * (int64, device). Gather columns with gpuq_gather afterwards.
 * num_parts <= 65536 (two radix passes above 256). */
int gpuq_partition_perm(void* stream, int64_t nrows, gpuq_col key,
                        int32_t num_parts, uint32_t* out_perm,
                        int64_t* out_counts,
                        void* workspace, int64_t workspace_bytes);

/* Multi-column partition keys: pid = Pmod(Murmur3Hash(k1..kK, 42), n)
 * with the hash seed-chained column-wise and NULL columns passing the
 * running seed through (hash.scala:849-860 HashExpression.eval;
 * partitioning.scala:328). nkeys <= 4, each int64. */
int gpuq_partition_perm_multi(void* stream, int64_t nrows,
                              const gpuq_col* key_cols, int32_t nkeys,
                              int32_t num_parts, uint32_t* out_perm,
                              int64_t* out_counts,
                              void* workspace, int64_t workspace_bytes);

/* Range partition (global ORDER BY across GPUs): bin = first bound >=
 * key in the sort order (RangePartitioning, ShuffleExchangeExec.scala:
 * 379-400 — the host layer samples keys and picks quantile bounds);
 * NULL keys go to the first/last partition per nulls_first. bounds:
 * device array of nbounds entries, same dtype as the key; out_counts:
 * nbounds+1 entries. Stable, like the hash partition. */
int gpuq_range_partition_perm(void* stream, int64_t nrows, gpuq_col key,
                              int32_t desc, int32_t nulls_first,
                              const void* bounds, int32_t nbounds,
                              uint32_t* out_perm, int64_t* out_counts,
                              void* workspace, int64_t workspace_bytes);

/* ---------------------------------------------------------------- */
/* HASH JOIN — replaces ShuffledHashJoinExec inner join              */
/* (joins/ShuffledHashJoinExec.scala:103-132; build side analog of   */
/* LongHashedRelation, joins/HashedRelation.scala:993 — duplicates   */
/* chained per key). NULL keys never match. Emission order is        */
/* nondeterministic (checker sorts, as QueryTest does).              */
/* ---------------------------------------------------------------- */

int64_t gpuq_join_build_workspace_bytes(int64_t build_rows, int64_t capacity);
/* The probe needs no workspace of its own: always 0 (kept for the ABI). */
int64_t gpuq_join_probe_workspace_bytes(int64_t probe_rows);

/* Build the hash table over the build-side key column. capacity: power of
 * two >= ~1.6*build_rows. The workspace holds the table + chains and must
 * stay alive through probes. */
int gpuq_join_build_i64(void* stream, int64_t build_rows, gpuq_col build_key,
                        void* workspace, int64_t capacity);

/* Probe: emits matching (probe_rid, build_rid) uint32 pairs into the
 * caller's buffers (out_cap entries each); *out_nmatches returns the total
 * match count. If the count exceeds out_cap, returns GPUQ_ERR_OVERFLOW
 * after setting *out_nmatches (call again with bigger buffers).
 * probe_workspace / probe_workspace_bytes are accepted and ignored (they
 * fed a hash-ordered probe stream that was retired); pass NULL and 0. */
/* join_type (ShuffledHashJoinExec.scala joinType dispatch): 0=Inner,
 * 1=probe-side Outer (unmatched probe rows pair with build rid 0xFFFFFFFF
 * => NULL build columns; gather with gpuq_gather_nullable), 2=LeftSemi
 * (probe row once iff matched; out_b = 0xFFFFFFFF), 3=LeftAnti (iff
 * unmatched; NULL probe keys emit — the non-null-aware anti). */
int gpuq_join_probe_i64_typed(void* stream, int64_t probe_rows, gpuq_col probe_key,
                              const void* workspace, int64_t capacity,
                              int64_t build_rows, void* probe_workspace,
                              int64_t probe_workspace_bytes, int32_t join_type,
                              uint32_t* out_probe_rid, uint32_t* out_build_rid,
                              int64_t out_capacity, int64_t* out_nmatches);

/* inner-join compatibility wrapper (join_type = 0) */
int gpuq_join_probe_i64(void* stream, int64_t probe_rows, gpuq_col probe_key,
                        const void* workspace, int64_t capacity, int64_t build_rows,
                        void* probe_workspace, int64_t probe_ws_bytes,
                        uint32_t* out_probe_rid, uint32_t* out_build_rid,
                        int64_t out_cap, int64_t* out_nmatches);

/* ---------------------------------------------------------------- */
/* COMPOSITE-KEY HASH JOIN — equi-join on a key tuple, the general   */
/* HashJoin case (joins/HashJoin.scala leftKeys/rightKeys:           */
/* Seq[Expression]); the single-key entry points above are its       */
/* LongHashedRelation special case. 1 <= nkeys <= 4; every key       */
/* column is GPUQ_INT64 with optional validity. A row with a NULL in */
/* ANY key column never matches (no null-safe <=>). -1, 0 and        */
/* INT64_MIN are ordinary key values. Emission order is              */
/* nondeterministic.                                                 */
/* ---------------------------------------------------------------- */

/* Table + chains + matched bits for build_rows rows at the given capacity.
 * Pure arithmetic (no device query); 0 for arguments out of range. The
 * workspace must be 64-byte aligned and stay alive through the probes. */
int64_t gpuq_join_keys_workspace_bytes(int64_t build_rows, int64_t capacity, int32_t nkeys);

/* Build the table over the build-side key columns: one slot per distinct
 * tuple, duplicates chained. capacity: a power of two GREATER than the
 * number of distinct non-NULL build tuples (callers use >= 2*build_rows);
 * build_rows <= 0x7FFFFFFE. A table that cannot seat every tuple gives up
 * after `capacity` slot visits and returns GPUQ_ERR_OVERFLOW (bounded, no
 * hang); the workspace is then unusable until rebuilt. Bad nkeys, a
 * non-power-of-two capacity or a non-int64 key return GPUQ_ERR_INVALID
 * before anything is launched. Resets the matched bits. */
int gpuq_join_build_keys(void* stream, int64_t build_rows,
                         const gpuq_col* build_keys, int32_t nkeys,
                         void* workspace, int64_t capacity);

/* Probe one batch: emits (probe_rid, build_rid) uint32 pairs exactly as
 * gpuq_join_probe_i64_typed does — *out_nmatches is always set; if it
 * exceeds out_capacity nothing is written past out_capacity and
 * GPUQ_ERR_OVERFLOW is returned (call again with bigger buffers; setting
 * matched bits twice is harmless). join_type: 0=Inner, 1=probe-side Outer,
 * 2=LeftSemi, 3=LeftAnti, 4=FullOuter probe half (as 1, and sets the
 * matched bit of every build row it pairs). Type 4 does NOT emit unmatched
 * build rows: a probe side arriving in several batches calls this once per
 * batch and gpuq_join_keys_unmatched_build once at the end. Type 5
 * (null-aware anti) is single-key only (isNullAwareAntiJoin requires
 * leftKeys.length == 1) and returns GPUQ_ERR_INVALID, like every other bad
 * argument, before anything is launched. */
int gpuq_join_probe_keys(void* stream, int64_t probe_rows,
                         const gpuq_col* probe_keys, int32_t nkeys,
                         void* workspace, int64_t capacity, int64_t build_rows,
                         int32_t join_type,
                         uint32_t* out_probe_rid, uint32_t* out_build_rid,
                         int64_t out_capacity, int64_t* out_nmatches);

/* Probe with a residual join condition — the non-equi remainder of the ON
 * clause that HashJoin.scala keeps as boundCondition (`l.k = r.k AND
 * l.ship < r.cutoff`: the equality is the key, the rest is the condition).
 * Same table (gpuq_join_build_keys), same workspace and same pair output as
 * gpuq_join_probe_keys; no new build, and gpuq_join_keys_unmatched_build is
 * used unchanged.
 *
 * cond_cols[ncond_cols] are the columns the condition reads; cond_sides[c]
 * says which side cond_cols[c] belongs to: a probe-side column is indexed by
 * the probe row id, a build-side column by the build row id. prog is exactly
 * a gpuq_filter_expr program over cond_cols (HOST array, copied into the
 * kernel arguments): the same eight opcodes, the same GPUQ_PRED_MAX_* caps,
 * the same comparison rules (total order on float64, -0.0 == 0.0, NaN == NaN
 * and greatest) and the same Kleene tables. CMP_COL may compare a probe
 * column with a build column of equal dtype.
 *
 * A candidate pair (all keys equal, no NULL in any key column) PASSES iff
 * the program evaluates to TRUE for it; FALSE and NULL both fail. The join
 * types are those of gpuq_join_probe_keys with "match" read as "passing
 * pair":
 *   0 Inner      every passing pair;
 *   1 Outer      every passing pair; a probe row without one — NULL key, no
 *                key match, or a key match whose candidates all fail — emits
 *                (i, 0xFFFFFFFF) once;
 *   2 LeftSemi   the probe row once iff at least one pair passes;
 *   3 LeftAnti   the probe row once iff no pair passes (NULL-key rows and
 *                rows whose candidates all fail included);
 *   4 FullOuter  probe half: as 1, and sets the matched bit of exactly the
 *                build rows that appear in a passing pair. Key-equal build
 *                rows whose pairs all fail stay unmatched and come out of
 *                gpuq_join_keys_unmatched_build;
 *   5            GPUQ_ERR_INVALID: Spark requires an empty condition for the
 *                null-aware anti join.
 * As for gpuq_join_probe_keys: *out_nmatches is always set; if it exceeds
 * out_capacity nothing is written past out_capacity and GPUQ_ERR_OVERFLOW is
 * returned (call again with bigger buffers; setting matched bits twice is
 * harmless); emission order is nondeterministic; probe_rows == 0 launches
 * nothing.
 * Returned as GPUQ_ERR_INVALID before anything is launched: everything
 * gpuq_join_probe_keys rejects; ncond_cols outside 1..GPUQ_PRED_MAX_COLS; a
 * NULL cond_cols, cond_sides or prog; a side other than 0 or 1; ninsns
 * outside 1..GPUQ_PRED_MAX_INSNS; and every program error gpuq_filter_expr
 * rejects — a bad opcode, comparison code or CONST value, a column index out
 * of range, a column whose dtype is not int64 / float64, CMP_COL over two
 * dtypes, a stack that underflows, grows past GPUQ_PRED_MAX_DEPTH or does
 * not end at depth exactly 1. */
#define GPUQ_JOIN_SIDE_PROBE 0
#define GPUQ_JOIN_SIDE_BUILD 1

struct gpuq_pred_insn;   /* defined with gpuq_filter_expr below */

int gpuq_join_probe_keys_cond(void* stream, int64_t probe_rows,
                              const gpuq_col* probe_keys, int32_t nkeys,
                              void* workspace, int64_t capacity, int64_t build_rows,
                              int32_t join_type,
                              const gpuq_col* cond_cols, const int32_t* cond_sides,
                              int32_t ncond_cols,
                              const struct gpuq_pred_insn* prog /* HOST */, int32_t ninsns,
                              uint32_t* out_probe_rid, uint32_t* out_build_rid,
                              int64_t out_capacity, int64_t* out_nmatches);

/* FullOuter second half: one (0xFFFFFFFF, build_rid) pair per build row
 * whose matched bit is clear after the type-4 probes so far — NULL-key
 * build rows included (never inserted, so never matched). Same overflow
 * contract as the probe; build_rows entries always suffice. */
int gpuq_join_keys_unmatched_build(void* stream, void* workspace, int64_t capacity,
                                   int64_t build_rows, int32_t nkeys,
                                   uint32_t* out_probe_rid, uint32_t* out_build_rid,
                                   int64_t out_capacity, int64_t* out_nrows);

/* ---------------------------------------------------------------- */
/* FILTER / PROJECT — SURVEY §8(f).2: FilterExec / ProjectExec on    */
/* columnar batches, so multi-operator plans stay on-device.         */
/* Filter: single comparison col OP literal (gpuq_filter_cmp) or a   */
/* compound predicate (gpuq_filter_expr); WHERE keeps only TRUE      */
/* (a NULL result drops the row). Stable compaction: the             */
/* first *out_count entries of out_perm are the passing rows in      */
/* input order. Project: elementwise a OP b (column or literal), or  */
/* a list of compound expressions in one pass (gpuq_project_expr).   */
/* ---------------------------------------------------------------- */

/* Comparison rules (Spark, non-ANSI):
 *  - a NULL input row never passes, GPUQ_CMP_NE included;
 *  - float64 uses Spark's total order (SQLOrderingUtil.compareDoubles), the
 *    one the sort and MIN/MAX already follow: -0.0 == 0.0, NaN == NaN, and
 *    NaN is greater than every other value, +inf included. So `x > 0.5` and
 *    `x >= 0.5` keep NaN rows, and a NaN literal is legal: `x == NaN` keeps
 *    exactly the NaN rows, `x < NaN` every other valid row;
 *  - int64 compares exactly against lit_i64 (lit_f64 is ignored). */
#define GPUQ_CMP_EQ 0
#define GPUQ_CMP_LT 1
#define GPUQ_CMP_LE 2
#define GPUQ_CMP_GT 3
#define GPUQ_CMP_GE 4
#define GPUQ_CMP_NE 5

int64_t gpuq_filter_workspace_bytes(int64_t nrows);
int gpuq_filter_cmp(void* stream, int64_t nrows, gpuq_col col, int32_t op,
                    double lit_f64, int64_t lit_i64,
                    uint32_t* out_perm, int64_t* out_count /* device, u64 */,
                    void* workspace, int64_t workspace_bytes);

/* Compound WHERE predicate in one fused pass: a postfix program over up to
 * GPUQ_PRED_MAX_COLS columns, evaluated per row on a stack of three-valued
 * (TRUE / FALSE / NULL) slots. The host layer lowers And / Or / Not / In /
 * Between / IsNull / IsNotNull and the binary comparisons to it; the kernel
 * knows only the eight opcodes below.
 *
 * Semantics (Spark, non-ANSI):
 *  - CMP_LIT (cols[col_a] OP literal; lit_f64 for a float64 column, lit_i64
 *    for an int64 one) and CMP_COL (cols[col_a] OP cols[col_b], equal
 *    dtypes): NULL if an operand row is NULL, else exactly the comparison
 *    rules above — total order on float64, -0.0 == 0.0, NaN == NaN and
 *    greatest;
 *  - IS_NULL / IS_NOT_NULL push TRUE or FALSE, never NULL;
 *  - CONST pushes cmp: 0 = FALSE, 1 = TRUE, 2 = NULL;
 *  - AND pops two: FALSE if either is FALSE, else NULL if either is NULL,
 *    else TRUE. OR is its dual: TRUE if either is TRUE, else NULL if either
 *    is NULL, else FALSE. NOT pops one: NOT NULL is NULL;
 *  - a row passes iff the value left on the stack is TRUE. */
#define GPUQ_PRED_CMP_LIT 0
#define GPUQ_PRED_CMP_COL 1
#define GPUQ_PRED_IS_NULL 2
#define GPUQ_PRED_IS_NOT_NULL 3
#define GPUQ_PRED_CONST 4
#define GPUQ_PRED_AND 5
#define GPUQ_PRED_OR 6
#define GPUQ_PRED_NOT 7

#define GPUQ_PRED_FALSE 0
#define GPUQ_PRED_TRUE 1
#define GPUQ_PRED_NULL 2

#define GPUQ_PRED_MAX_INSNS 32
#define GPUQ_PRED_MAX_COLS 8
#define GPUQ_PRED_MAX_DEPTH 16

typedef struct gpuq_pred_insn {
  int32_t opcode;   /* GPUQ_PRED_* */
  int32_t cmp;      /* GPUQ_CMP_* for CMP_LIT / CMP_COL; 0/1/2 = FALSE/TRUE/NULL for CONST */
  int32_t col_a;    /* index into cols[] */
  int32_t col_b;    /* CMP_COL only */
  int64_t lit_i64;
  double lit_f64;
} gpuq_pred_insn;

/* workspace bytes for gpuq_filter_expr at nrows; pure arithmetic */
int64_t gpuq_filter_expr_workspace_bytes(int64_t nrows);

/* The first *out_count entries of out_perm[nrows] are the row ids for which
 * the program evaluates to TRUE, in ascending (input) order; entries past
 * *out_count are unspecified (gpuq_filter_cmp writes all nrows, this does
 * not). prog is a HOST array, copied into the kernel arguments. Each
 * referenced column (and bitmap) is read once and never written. nrows == 0
 * sets *out_count to 0 and launches nothing. Returned as GPUQ_ERR_INVALID
 * before anything is launched: nrows > 0xFFFFFFFF; ncols outside
 * 0..GPUQ_PRED_MAX_COLS (a CONST-only program reads no column; cols may be
 * NULL then) or ninsns outside 1..GPUQ_PRED_MAX_INSNS; a bad
 * opcode, comparison code or CONST value; a column index out of range; a
 * column whose dtype is not int64 / float64; CMP_COL over two dtypes; a
 * short workspace; a program whose stack underflows, grows past
 * GPUQ_PRED_MAX_DEPTH or does not end at depth exactly 1. */
int gpuq_filter_expr(void* stream, int64_t nrows,
                     const gpuq_col* cols, int32_t ncols,
                     const gpuq_pred_insn* prog /* HOST */, int32_t ninsns,
                     uint32_t* out_perm, int64_t* out_count /* device, u64 */,
                     void* workspace, int64_t workspace_bytes);

#define GPUQ_BINOP_ADD 0
#define GPUQ_BINOP_SUB 1
#define GPUQ_BINOP_MUL 2
#define GPUQ_BINOP_DIV 3
#define GPUQ_BINOP_RSUB 4  /* out = b - a (literal - column) */

/* Arithmetic rules (Spark, non-ANSI): int64 + - * wrap modulo 2^64; int64 /
 * truncates toward zero and INT64_MIN / -1 == INT64_MIN (Java long); float64
 * is the IEEE result of the single operation.
 *
 * gpuq_project_binop tracks no NULLs: a.validity must be NULL, the caller
 * owns validity (AVG = sum / count derives it from the count) and an
 * integral zero divisor yields 0. b is read with a's dtype. */
int gpuq_project_binop(void* stream, int64_t nrows, gpuq_col a,
                       const void* b /* second column's data or NULL for literal */,
                       double lit_f64, int64_t lit_i64, int32_t op, void* out);

/* NULL-aware projection. b.data == NULL makes b the literal (lit_f64 for a
 * float64 a, lit_i64 for an int64 a; b.validity must then be NULL); otherwise
 * b.dtype must equal a.dtype. Output row i is valid iff a and b are valid at
 * i and the op is not a division by zero: x / 0 is NULL (for float64, 0.0
 * and -0.0 alike; a NaN divisor is not zero). NULL output rows hold 0.
 * out_validity_bits: (nrows + 7) / 8 bytes; may be NULL only when nothing
 * can be NULL (no input bitmap and op != GPUQ_BINOP_DIV). */
int gpuq_project_binop_nullable(void* stream, int64_t nrows, gpuq_col a,
                                gpuq_col b, double lit_f64, int64_t lit_i64,
                                int32_t op, void* out,
                                uint8_t* out_validity_bits);

/* Compound SELECT-list expressions in one fused pass: a typed postfix program
 * over up to GPUQ_EXPR_MAX_COLS columns, evaluated once per row on a stack of
 * at most GPUQ_EXPR_MAX_DEPTH slots, producing up to GPUQ_EXPR_MAX_OUTS output
 * columns from ONE read of each referenced input column. The host layer
 * (spark_amd/expression.py) lowers arithmetic trees, casts, comparisons used
 * as values, If / CaseWhen and Coalesce to it.
 *
 * Every instruction states its operand type in `dtype`; the host decides all
 * typing and the entry point checks it with a stack simulation, so the kernel
 * tracks no types at run time. Stack types are GPUQ_INT64, GPUQ_FLOAT64 and
 * the stack-only GPUQ_EXPR_BOOL. A slot is a 64-bit payload plus a NULL flag;
 * BOOL is payload 0 / 1; the payload of a NULL slot is unspecified.
 *
 * Semantics (Spark, non-ANSI):
 *  COL     push cols[arg]; NULL where its bitmap says so. dtype = its dtype.
 *  LIT     push the literal of type dtype (lit_f64 for float64, lit_i64 for
 *          int64 and for BOOL, which takes 0 / 1). arg == 1: the typed NULL
 *          literal; arg must be 0 or 1.
 *  REF     push the value and NULL-ness OUT arg already produced for the row.
 *  ARITH   arg = GPUQ_BINOP_ADD / SUB / MUL / DIV. Pops b (top), then a, and
 *          pushes a OP b by the arithmetic rules of
 *          gpuq_project_binop_nullable: int64 + - * wrap, / truncates toward
 *          zero, INT64_MIN / -1 == INT64_MIN; float64 is the IEEE result of
 *          that single operation (nothing is contracted across instructions).
 *          NULL if an operand is NULL or the op is / and the divisor is zero
 *          (float64: 0.0 and -0.0).
 *  NEG ABS int64 wraps: -INT64_MIN == abs(INT64_MIN) == INT64_MIN. float64
 *          flips / clears the sign bit (NaN included). NULL stays NULL.
 *  CAST    dtype = source type, arg = target type: int64 -> float64 (round to
 *          nearest even), float64 -> int64 (Java's (long) d: truncates toward
 *          zero, NaN -> 0, values at or beyond +/-2^63 saturate to INT64_MAX /
 *          INT64_MIN), BOOL -> int64 (0 / 1). NULL stays NULL.
 *  CMP     arg = GPUQ_CMP_*. Pops b then a of equal int64 / float64 type and
 *          pushes BOOL by exactly the comparison rules above (total order on
 *          float64, -0.0 == 0.0, NaN == NaN and greatest). NULL if an operand
 *          is NULL.
 *  IS_NULL / IS_NOT_NULL  pop one value of any type (dtype = its type), push
 *          a BOOL that is never NULL.
 *  AND OR NOT  Kleene logic on BOOL, the truth tables of gpuq_filter_expr.
 *  SELECT  pops cond (top, BOOL), then `then`, then `else` (equal types,
 *          dtype = that type). Pushes `then` iff cond is TRUE, otherwise
 *          `else` — a NULL cond picks `else`, as Spark's If / CaseWhen do —
 *          with the chosen branch's NULL-ness. Both branches are evaluated;
 *          a division by zero in the branch not taken is a discarded NULL.
 *  COALESCE  pops b (top), then a, of equal types: a if a is non-NULL, else b.
 *  OUT     pops the top (int64 / float64, == out_dtypes[arg] == dtype), writes
 *          it to outs[arg] (0 where the row is NULL) and, when
 *          out_validity_bits[arg] is non-NULL, the row's validity bit. */
#define GPUQ_EXPR_BOOL 3   /* stack-only type; not a column dtype */

#define GPUQ_EXPR_COL 0
#define GPUQ_EXPR_LIT 1
#define GPUQ_EXPR_REF 2
#define GPUQ_EXPR_ARITH 3
#define GPUQ_EXPR_NEG 4
#define GPUQ_EXPR_ABS 5
#define GPUQ_EXPR_CAST 6
#define GPUQ_EXPR_CMP 7
#define GPUQ_EXPR_IS_NULL 8
#define GPUQ_EXPR_IS_NOT_NULL 9
#define GPUQ_EXPR_AND 10
#define GPUQ_EXPR_OR 11
#define GPUQ_EXPR_NOT 12
#define GPUQ_EXPR_SELECT 13
#define GPUQ_EXPR_COALESCE 14
#define GPUQ_EXPR_OUT 15

#define GPUQ_EXPR_MAX_INSNS 48
#define GPUQ_EXPR_MAX_COLS 8
#define GPUQ_EXPR_MAX_OUTS 4
#define GPUQ_EXPR_MAX_DEPTH 8

typedef struct gpuq_expr_insn {
  int32_t opcode;   /* GPUQ_EXPR_* */
  int32_t arg;      /* column / output index, binop, comparison, cast target, NULL-literal flag */
  int32_t dtype;    /* operand type: GPUQ_INT64 / GPUQ_FLOAT64 / GPUQ_EXPR_BOOL */
  int32_t pad;      /* ignored */
  int64_t lit_i64;
  double lit_f64;
} gpuq_expr_insn;

/* Needs no workspace and never synchronises with the host. prog is a HOST
 * array, copied into the kernel arguments. outs[k] is nrows 8-byte values of
 * out_dtypes[k]; out_validity_bits[k] is (nrows + 7) / 8 bytes (spare bits of
 * the last byte come out zero, nothing past it is written, no alignment is
 * required) or NULL, by which the caller asserts that output k cannot be NULL:
 * nothing is recorded for it then. Every referenced column (and bitmap) is
 * read once and never written. Outputs and their bitmaps must not overlap an
 * input or each other. nrows == 0 returns GPUQ_OK with nothing launched.
 * Returned as GPUQ_ERR_INVALID before any HIP call: nrows < 0 or
 * > 0xFFFFFFFF; ncols outside 0..GPUQ_EXPR_MAX_COLS, ninsns outside
 * 1..GPUQ_EXPR_MAX_INSNS, nouts outside 1..GPUQ_EXPR_MAX_OUTS; a column or
 * output dtype other than int64 / float64; a bad opcode, binop (RSUB
 * included), comparison, cast pair or NULL-literal flag; a column, output or
 * REF index out of range; a REF to an output not yet written; an output
 * written twice or never; a declared dtype that differs from the type the
 * stack simulation infers; operand types that differ; BOOL given to ARITH,
 * NEG, ABS, CMP or OUT; non-BOOL given to AND, OR, NOT or as a SELECT
 * condition; stack underflow; depth over GPUQ_EXPR_MAX_DEPTH; a program that
 * does not end at depth 0; a NULL outs[k] with nrows > 0. */
int gpuq_project_expr(void* stream, int64_t nrows,
                      const gpuq_col* cols, int32_t ncols,
                      const gpuq_expr_insn* prog /* HOST */, int32_t ninsns,
                      void* const* outs, uint8_t* const* out_validity_bits,
                      const int32_t* out_dtypes, int32_t nouts);

/* int64 -> float64 cast (AVG evaluation: sum / cast(count)) */
int gpuq_cast_i64_f64(void* stream, int64_t nrows, const int64_t* in, double* out);

/* ---------------------------------------------------------------- */
/* VALIDITY BITMAP UTILITIES — move Arrow validity bitmaps           */
/* (LSB-first, ColumnVector null contract, ColumnVector.java:58-366) */
/* through permutations and across the RCCL exchange (bitmaps travel */
/* as u8 columns: all-to-all row splits are not byte-aligned).       */
/* ---------------------------------------------------------------- */

/* out bit i = src bit perm[i] (permute a validity bitmap alongside its
 * data column) */
int gpuq_gather_bits(void* stream, int64_t nrows, const uint8_t* src_bits,
                     const uint32_t* perm, uint8_t* out_bits);

/* bitmap <-> one-byte-per-row (exchange transport form) */
int gpuq_bits_to_u8(void* stream, int64_t nrows, const uint8_t* bits,
                    uint8_t* out);
int gpuq_u8_to_bits(void* stream, int64_t nrows, const uint8_t* u8,
                    uint8_t* out_bits);

/* out[i] = col[perm[i]], with perm[i] == 0xFFFFFFFF producing NULL (the
 * outer-join build side); out_bits = src validity AND not-NIL. */
int gpuq_gather_nullable(void* stream, int64_t nrows, gpuq_col col,
                         const uint32_t* perm, void* out, uint8_t* out_bits);

/* validity bitmap for key column `bit` of a composite-key result:
 * out bit i = (mask[i] >> bit) & 1 (see gpuq_hash_agg_keys out_kmask) */
int gpuq_maskbit_to_bits(void* stream, int64_t nrows, const uint8_t* mask,
                         int32_t bit, uint8_t* out_bits);

/* bit i = (in[i] != 0): merged-COUNT column -> NULL-ness of merged
 * SUM/MIN/MAX results (final-mode aggregation, Sum.scala merge) */
int gpuq_nonzero_to_bits(void* stream, int64_t nrows, const int64_t* in,
                         uint8_t* out_bits);

/* Decimal-overflow-to-NULL for 128-bit sums (Sum.scala, non-ANSI): clears
 * validity bit i (Arrow LSB order, in/out) when |(hi[i],lo[i])| >=
 * 10^result_precision, 1 <= result_precision <= 38; bits already clear stay
 * clear. (lo, hi) as emitted by spec ops 8/9/10 above. */
int gpuq_dec128_overflow_to_null(void* stream, int64_t nrows, const int64_t* lo,
                                 const int64_t* hi, int32_t result_precision,
                                 uint8_t* validity_bits);

/* min/max/valid-count reduction of an int64 column. out_dev: device u64[3]
 * = {min encoded (encode_i64), max encoded, count of valid rows}. */
int gpuq_minmax_i64(void* stream, int64_t nrows, gpuq_col col,
                    unsigned long long* out_dev);

/* Pack two narrow int64 key columns into one: out = (a - a_bias) << shift
 * | (b - b_bias). Caller proves the ranges via gpuq_minmax_i64 first.
 * Feeds composite GROUP BY keys into the single-key fast path (per-block
 * LDS tables at low cardinality). */
int gpuq_pack2_i64(void* stream, int64_t nrows, const int64_t* a,
                   const int64_t* b, int64_t a_bias, int64_t b_bias,
                   int32_t shift, int64_t* out);
int gpuq_unpack2_i64(void* stream, int64_t nrows, const int64_t* in,
                     int64_t a_bias, int64_t b_bias, int32_t shift,
                     int64_t* out_a, int64_t* out_b);

/* ---------------------------------------------------------------- */
/* WINDOW — the device side of WindowExec (execution/window/         */
/* WindowExec.scala): row_number / rank / dense_rank, running and    */
/* per-partition COUNT / SUM / MIN / MAX (the frames of              */
/* WindowFunctionFrame.scala's UnboundedPrecedingWindowFunctionFrame */
/* and UnboundedWindowFunctionFrame) and lag / lead                  */
/* (FrameLessOffsetWindowFunctionFrame), as segmented scans.         */
/* The input batch is ALREADY SORTED by (partition keys, then order  */
/* keys) — the SortExec EnsureRequirements puts below a WindowExec;  */
/* nothing here sorts. Partition and peer-group starts are carried   */
/* as two bitmaps of 8 * ceil(nrows / 64) bytes, LSB-first (byte-    */
/* compatible with the Arrow validity layout), bits at and above     */
/* nrows zero. One call computes one window expression; a node       */
/* computes the bitmaps once and shares them.                        */
/* ---------------------------------------------------------------- */

/* bit i of out_part_start: i == 0 or some partition key differs between rows
 * i-1 and i. bit i of out_peer_start: the part_start bit, or some order key
 * differs (a new peer group). keys[0..npart) are the partition columns,
 * keys[npart..nkeys) the order columns; 0 <= npart <= nkeys <= 8, each int64
 * or float64 with optional validity. Equality is the sort's: NULL == NULL,
 * NULL != value, int64 exact, float64 by the sort-key encoding (so -0.0 ==
 * 0.0 and every NaN equals every NaN). nkeys == 0 gives one partition of one
 * peer group. Each key column is read once and never written. No workspace.
 * nrows == 0 returns GPUQ_OK with nothing launched; nrows > 0xFFFFFFFF,
 * nkeys / npart out of range or a dtype other than int64 / float64 return
 * GPUQ_ERR_INVALID before anything is launched. */
int gpuq_window_boundaries(void* stream, int64_t nrows, const gpuq_col* keys,
                           int32_t nkeys, int32_t npart,
                           uint64_t* out_part_start, uint64_t* out_peer_start);

#define GPUQ_WIN_ROW_NUMBER 0   /* int64 out; val ignored; frame must be ROWS */
#define GPUQ_WIN_RANK       1   /* 1 + rows of the partition before the row's peer group */
#define GPUQ_WIN_DENSE_RANK 2   /* peer groups of the partition up to and including the row's */
#define GPUQ_WIN_COUNT      3   /* int64 out, never NULL; val.data == NULL means COUNT(*) */
#define GPUQ_WIN_SUM        4   /* int64 -> int64 wrapping; float64 -> float64 */
#define GPUQ_WIN_MIN        5   /* order of the aggregate's MIN/MAX (spec ops 4-7):   */
#define GPUQ_WIN_MAX        6   /* encode_i64 / encode_f64, NaN greatest, zero emitted as +0.0 */

#define GPUQ_FRAME_ROWS      0  /* ROWS  BETWEEN UNBOUNDED PRECEDING AND CURRENT ROW */
#define GPUQ_FRAME_RANGE     1  /* RANGE BETWEEN UNBOUNDED PRECEDING AND CURRENT ROW: peers share the value at the last row of their group */
#define GPUQ_FRAME_PARTITION 2  /* UNBOUNDED PRECEDING .. UNBOUNDED FOLLOWING: every row gets the partition's value */

/* workspace bytes for gpuq_window_scan / gpuq_window_shift at nrows; pure
 * arithmetic (a few words per 2048-row tile) */
int64_t gpuq_window_workspace_bytes(int64_t nrows);

/* out[i] = op over the rows of i's frame, given the bitmaps
 * gpuq_window_boundaries produced for the same rows. out is nrows 8-byte
 * values: int64 for the rank ops, COUNT and int64 SUM / MIN / MAX, float64
 * for float64 SUM / MIN / MAX.
 * NULL rules (Sum.scala / Min / Max, as the hash aggregate states them): SUM
 * / MIN / MAX skip NULL rows; a row's result is NULL iff its frame holds no
 * non-NULL value, and NULL result rows hold 0. MIN / MAX of float64 return
 * the canonical NaN for any NaN and +0.0 for either zero. A float64 SUM adds
 * in tile order, not row order: exact while every partial sum is exactly
 * representable, otherwise within the usual reordering error; a sum over
 * zeros only is +0.0.
 * out_validity_bits is (nrows + 7) / 8 bytes, spare bits of the last byte
 * zero. It may be NULL for the rank ops, for COUNT (when given it comes out
 * all valid) and for SUM / MIN / MAX over a column without a bitmap.
 * RANGE and PARTITION frames run the ROWS scan and then copy, in place, the
 * value at the last row of each peer group / partition to its rows.
 * val (and its bitmap) and the two boundary bitmaps are read twice on the
 * stream and never written; out must not overlap them.
 * GPUQ_ERR_INVALID before anything is launched: nrows > 0xFFFFFFFF; a bad op
 * or frame; a rank op (0-2) with a frame other than ROWS; a value column
 * whose dtype is not int64 / float64; SUM / MIN / MAX with val.data == NULL
 * (and nrows > 0: an empty column's pointer may be NULL); SUM / MIN / MAX
 * over a column with a bitmap and no out_validity_bits; a short workspace.
 * nrows == 0 returns GPUQ_OK with nothing launched. */
int gpuq_window_scan(void* stream, int64_t nrows, int32_t op, int32_t frame, gpuq_col val,
                     const uint64_t* part_start, const uint64_t* peer_start,
                     void* out, uint8_t* out_validity_bits,
                     void* workspace, int64_t workspace_bytes);

/* LAG (offset < 0) / LEAD (offset > 0): out[i] = val[i + offset] if that row
 * lies in i's partition (it keeps its own NULL-ness: ignoreNulls = false).
 * Otherwise out[i] is the default (lit_f64 / lit_i64 by val.dtype) when
 * has_default, else NULL. offset == 0 copies. NULL rows hold 0.
 * out_validity_bits ((nrows + 7) / 8 bytes) is required; out must not overlap
 * val. Same workspace as gpuq_window_scan. GPUQ_ERR_INVALID before anything
 * is launched: nrows > 0xFFFFFFFF, a dtype other than int64 / float64, a
 * short workspace, val.data or out_validity_bits NULL. nrows == 0 returns
 * GPUQ_OK with nothing launched. */
int gpuq_window_shift(void* stream, int64_t nrows, gpuq_col val, int64_t offset,
                      int32_t has_default, double lit_f64, int64_t lit_i64,
                      const uint64_t* part_start, void* out, uint8_t* out_validity_bits,
                      void* workspace, int64_t workspace_bytes);

/* Sliding ROWS BETWEEN frames (WindowFunctionFrame.scala's
 * SlidingWindowFunctionFrame and UnboundedPrecedingWindowFunctionFrame) and
 * first_value / last_value. */
#define GPUQ_WIN_FIRST_VALUE 7   /* gpuq_window_slide only */
#define GPUQ_WIN_LAST_VALUE  8   /* gpuq_window_slide only */
#define GPUQ_WIN_UNBOUNDED_PRECEDING INT64_MIN
#define GPUQ_WIN_UNBOUNDED_FOLLOWING INT64_MAX
#define GPUQ_WIN_SLIDE_MAX_SPAN 2048   /* hi - lo of a two-sided bounded frame */

/* workspace bytes for gpuq_window_slide at (nrows, lo, hi): the scan's
 * workspace, plus nrows 8-byte words and a bitmap when lo is unbounded. Pure
 * arithmetic; 0 for arguments gpuq_window_slide would refuse. */
int64_t gpuq_window_slide_workspace_bytes(int64_t nrows, int64_t lo, int64_t hi);

/* out[i] = op over the frame ROWS BETWEEN lo AND hi of row i, given the
 * partition bitmap gpuq_window_boundaries produced for the same rows.
 * Frame: row i lies in the partition [pb, pe] (inclusive row positions); its
 * frame is the rows first..last with first = max(pb, i + lo) and last =
 * min(pe, i + hi), and it is EMPTY when first > last. lo ==
 * GPUQ_WIN_UNBOUNDED_PRECEDING means first = pb, hi ==
 * GPUQ_WIN_UNBOUNDED_FOLLOWING means last = pe. Finite offsets are signed row
 * counts (negative PRECEDING, 0 CURRENT ROW, positive FOLLOWING) that fit
 * int32, with lo <= hi.
 * Accepted shapes: (a) both finite with hi - lo <= GPUQ_WIN_SLIDE_MAX_SPAN,
 * at any distance from the row (5000 FOLLOWING .. 5002 FOLLOWING is legal);
 * (b) lo unbounded with hi finite or unbounded. A finite lo with an unbounded
 * hi is refused (it needs a backward scan).
 * Ops: COUNT (val.data == NULL: COUNT(*)), SUM, MIN, MAX, FIRST_VALUE,
 * LAST_VALUE; out is nrows 8-byte values typed as gpuq_window_scan's, and as
 * val for FIRST / LAST.
 * Results follow gpuq_window_scan's NULL / NaN rules: SUM / MIN / MAX skip
 * NULL rows; a row's result is NULL iff its frame holds no non-NULL value (an
 * empty frame is such a frame); NULL rows hold 0; COUNT is never NULL and is
 * 0 for an empty frame; int64 SUM wraps; float64 MIN / MAX order by the
 * sort-key encoding and return the canonical NaN and +0.0. FIRST_VALUE /
 * LAST_VALUE (ignoreNulls = false) copy the value and NULL-ness of row first
 * / last and give NULL for an empty frame.
 * float64 SUM, shape (a): acc = +0.0, then acc += v for the non-NULL rows
 * first..last in ascending row order, plain IEEE adds: the result equals that
 * expression bit for bit (any NaN counts as NaN). No prefix differences are
 * taken, so nothing cancels, inf - inf does not arise and a NaN reaches only
 * the frames that hold it. Shape (b) runs gpuq_window_scan's ROWS scan and
 * inherits its tile-order sum and reordering error.
 * out_validity_bits ((nrows + 7) / 8 bytes) is required for FIRST / LAST, and
 * for SUM / MIN / MAX when the column has a bitmap or the frame can be empty
 * (lo > 0 or hi < 0). It is optional for COUNT; when given it comes out all
 * valid.
 * val (and its bitmap) and part_start are read on the stream and never
 * written; out must not overlap them or the workspace.
 * GPUQ_ERR_INVALID before anything is launched: nrows < 0 or > 0xFFFFFFFF; a
 * bad op; a dtype other than int64 / float64; val.data == NULL for any op but
 * COUNT (and nrows > 0); lo > hi; a finite offset outside int32; a span over
 * the cap; a finite lo with an unbounded hi; a missing required
 * out_validity_bits (and nrows > 0); a short workspace. nrows == 0 returns
 * GPUQ_OK with nothing launched. */
int gpuq_window_slide(void* stream, int64_t nrows, int32_t op, gpuq_col val,
                      int64_t lo, int64_t hi, const uint64_t* part_start,
                      void* out, uint8_t* out_validity_bits,
                      void* workspace, int64_t workspace_bytes);

#ifdef __cplusplus
}
#endif
#endif /* GPUQ_H */
