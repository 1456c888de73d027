/*
 * tsamd.h -- C-ABI of the MI355X (gfx950) sparse-matmul hot path.
 *
 * This is the drop-in boundary: plain pointers + sizes, no torch types.  Every
 * entry point replaces one L0 function (or one ATen composition) of
 * rusty1s/pytorch_sparse; the reference interface it stands in for is cited
 * next to it as `path:line` relative to the reference tree.
 *
 * Conventions (all entry points):
 *   - all pointers are DEVICE pointers unless the name ends in `_host`;
 *   - index arrays are int64 (reference contract: storage.py:52,85,92 and
 *     csrc/cpu/spmm_cpu.cpp:39-40);
 *   - dense operands are row-major and contiguous ([B, rows, K]);
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream);
 *     nothing synchronises, nothing allocates, inputs are never written;
 *   - scratch memory is caller-provided: ask `*_workspace_bytes`, pass a
 *     device buffer of at least that size (256-byte aligned);
 *   - the return value is a tsamd_status; TSAMD_ERR_HIP means a HIP runtime
 *     call failed (tsamd_last_hip_error() returns the hipError_t).
 */
#ifndef TSAMD_H_
#define TSAMD_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
  TSAMD_OK = 0,
  TSAMD_ERR_INVALID = 1,     /* bad argument (null pointer, negative size, ...) */
  TSAMD_ERR_UNSUPPORTED = 2, /* dtype / reduce / size not implemented           */
  TSAMD_ERR_HIP = 3,         /* HIP runtime error, see tsamd_last_hip_error()   */
  TSAMD_ERR_WORKSPACE = 4    /* workspace missing or too small                  */
} tsamd_status;

/* Element types of `value` / `mat` / `out`.  Mirrors the dtypes the
 * reference tests sweep (torch_sparse/testing.py:7-14). */
typedef enum {
  TSAMD_F32 = 0,
  TSAMD_F64 = 1,
  TSAMD_F16 = 2,
  TSAMD_BF16 = 3,
  TSAMD_I32 = 4,
  TSAMD_I64 = 5,
  /* SpMM forward only (the reference dispatches AT_DISPATCH_ALL_TYPES_AND2, csrc/cpu/spmm_cpu.cpp:47):
   * sums wrap like the C++ type, mean divides the wrapped sum by the count cast to the type */
  TSAMD_U8 = 6,
  TSAMD_I8 = 7,
  TSAMD_I16 = 8
} tsamd_dtype;

/* Reductions reachable from the registered ops (csrc/spmm.cpp:82,145,195,255;
 * csrc/cpu/reducer.h:6-11 also lists mul/div, which no op can reach). */
typedef enum { TSAMD_SUM = 0, TSAMD_MEAN = 1, TSAMD_MIN = 2, TSAMD_MAX = 3 } tsamd_reduce;

/* Library / runtime identification.  Replaces torch_sparse::cuda_version
 * (csrc/version.cpp:26-41): returns HIP_VERSION the library was built with. */
int64_t tsamd_hip_version(void);
/* Build flags of the library; always 0 (no flag is defined).  Kept for ABI stability.  (No reference
 * counterpart: csrc/version.cpp:26-41 only reports the toolkit version.) */
int tsamd_build_flags(void);
/* Last hipError_t observed by this library on the calling thread. */
int tsamd_last_hip_error(void);
/* Human-readable string for a tsamd_status. */
const char *tsamd_status_string(int status);

/* ------------------------------------------------------------------------ *
 * CSR SpMM forward.   Replaces spmm_cuda / spmm_cpu
 * (csrc/cuda/spmm_cuda.cu:92-155, csrc/cpu/spmm_cpu.cpp:8-101).
 *
 *   out[b, m, :] = REDUCE_{e in [rowptr[m], rowptr[m+1])} value[e] * mat[b, col[e], :]
 *
 *   rowptr  [M+1] int64, col [E] int64 (0 <= col < N, not validated),
 *   value   [E] dtype or NULL (treated as all-ones),
 *   mat     [B, N, K] dtype,   out [B, M, K] dtype,
 *   arg_out [B, M, K] int64, required for MIN/MAX, ignored otherwise:
 *           edge id of the winning entry, first occurrence on ties
 *           (csrc/cpu/reducer.h:63-67); rows without entries get out = 0 and
 *           arg_out = E (csrc/cpu/spmm_cpu.cpp:35, reducer.h:76-82).
 *   MEAN divides by max(row length, 1) (reducer.h:73-74).
 *
 * f16/bf16 SUM/MEAN accumulate in fp32 and round once (the reference CPU
 * path accumulates in the narrow type); MIN/MAX compare the products rounded
 * to the narrow type exactly as the reference does.
 * ------------------------------------------------------------------------ */
size_t tsamd_spmm_workspace_bytes(int dtype, int reduce, int64_t B, int64_t M,
                                  int64_t N, int64_t K, int64_t E);

/* Hot rows (inspection and tests; no device work).  Sums / means of one floating-point matrix whose column ids camp copy
 * only the rows that a sample of `col` names into a side table inside the workspace.  Returns 1 when tsamd_spmm with
 * these operands and this workspace takes that route once its probe flags the graph, and fills layout[0..3]: byte
 * offsets in `workspace` of the N flag bytes (1 = hot), of the lookup words (per 32 ids: {flags, slot of the first
 * hot id}) and of the table (hot rows in id order), and the table's distance from `mat` in rows.  Returns 0 when the
 * call keeps the full copy of `mat`. */
int tsamd_spmm_hot_rows_layout(int dtype, int reduce, int64_t B, int64_t M, int64_t N, int64_t K, int64_t E,
                               const void *mat, const void *out, void *workspace, int64_t *layout);

/* Hot blocks (inspection and tests; no device work): the same scope from N = 65536 on, where the unit of the side table
 * is the block of 64 consecutive ids (a call takes one of the two routes, never both: for these shapes
 * tsamd_spmm_hot_rows_layout returns 0, for smaller N this function does).  A block is selected when at least
 * tsamd_spmm_hot_block_min() of its ids are flagged.  Returns 1 and fills layout[0..3]: byte offsets in `workspace` of
 * the N flag bytes, of the block words (uint32 per block: rank + 1 among the selected blocks in block order, 0 = not
 * selected) and of the table, and the table's distance from `mat` in rows.  Id i of the block of rank r sits in table
 * row r * 64 + ((i + rot(r)) & 63), rot(r) = ((uint32_t)(r * 0x9E3779B1u)) >> 26; rows of ids >= N are not written. */
int tsamd_spmm_hot_blocks_layout(int dtype, int reduce, int64_t B, int64_t M, int64_t N, int64_t K, int64_t E,
                                 const void *mat, const void *out, void *workspace, int64_t *layout);
int tsamd_spmm_hot_block_min(void);

/* tsamd_spmm_route (inspection and tests): what tsamd_spmm -- with arg32 != 0: tsamd_spmm_minmax_arg32 -- decides for
 * these operands before it launches anything.  Host arithmetic only -- no HIP call, no device: the driver plans every
 * call as one piece of data (plan_spmm, csrc/spmm_kernels.h) and then launches what that plan names; this entry, the two
 * layouts above and tsamd_spmm_order_layout make the same plan and copy words out of it.  Pointers count for their
 * alignment and for the offsets only; mat / out / arg_out == NULL mean "aligned", workspace == NULL leaves the four
 * offsets 0.
 *   route[0] family   merge instantiation: 0 nothing is launched (B * M * K == 0), 1 short rows side by side (lgG >= 3),
 *                     2 cooperative, 3 cooperative over the hot-row table, 4 over the hot-block table, 5 / 6 = 1 / 2 with
 *                     int32 winner ids, 7 the reference-order mode (tsamd_spmm_reference_order; nothing else is filled)
 *   route[1] vec      elements per lane packet; route[2] slots = ceil(K / vec) packets per row; route[3] lpr lanes per
 *                     row (a power of two <= 64); route[4] lgG (2^lgG rows side by side); route[5] ktiles (feature
 *                     tiles of 64 packets; gridDim.y = route[17] = B * ktiles)
 *   route[6] P, route[7] items   partitions and (row end + entry) items per partition; route[8] snap: min / max
 *                     boundaries that fall into the first `snap` entries of a row move back to its start (0: sums)
 *   route[9] relabel  0 no copy of mat, 2 decided on the device by the probe of `col` (1: never for this entry)
 *   route[10] copy    what a flagged call copies: 0 nothing, 1 all of mat, 2 the hot-row table, 3 the hot-block table
 *   route[11] fixup   1 when the fix-up kernel launches (P > 1)
 *   route[12..15]     byte offsets in `workspace` of table ([P + 1] {row, entry}), tail_row [P], head_row [P] (int64)
 *                     and of the probe's four int counters {-, ids with 3 low zero bits, with 6, samples}
 *   route[16] records arg32 only: the record-writing instantiation tsamd_spmm_minmax_records takes for this shape
 *                     (1: 97..128 features, 2: the others), 0 when its records come from the ids
 *   route[18]         tsamd_spmm_workspace_bytes of the shape; route[19..23] are 0.
 * TSAMD_ERR_INVALID for a negative size or route == NULL; TSAMD_ERR_UNSUPPORTED where the entry point refuses (dtype,
 * reduce, N >= 2^32, K >= 2^31, B * ceil(K / 64) >= 65536; arg32 for sum / mean, integer types or E >= 2^31);
 * TSAMD_ERR_WORKSPACE for a workspace off a 256-byte boundary. */
int tsamd_spmm_route(int dtype, int reduce, int64_t B, int64_t M, int64_t N, int64_t K, int64_t E, const void *mat,
                     const void *out, const void *arg_out, int arg32, void *workspace, int64_t route[24]);

int tsamd_spmm(int dtype, int reduce, const int64_t *rowptr, const int64_t *col,
               const void *value, const void *mat, void *out, int64_t *arg_out,
               int64_t B, int64_t M, int64_t N, int64_t K, int64_t E,
               void *workspace, size_t workspace_bytes, void *stream);
/* Verification mode: set = 1 makes tsamd_spmm / tsamd_spmm_cached / tsamd_spmm_minmax_arg32 (and every torch op on
 * top of them) compute in the ORDER OF OPERATIONS of the reference CPU kernel (csrc/cpu/spmm_cpu.cpp:61-87,
 * csrc/cpu/reducer.h:43-84: a row's entries one after the other, product and sum rounded separately in the element
 * type, mean = sum / (scalar_t)count), one thread per output element: results BIT-IDENTICAL to the reference for every
 * dtype and reduction, at a fraction of the speed.  set = 0 back to the product kernels, anything else: query.
 * Returns the mode in force.  Process-wide; the backward kernels are not affected. */
int tsamd_spmm_reference_order(int set);

/* Column order of the merge kernel.  Sums / means over rows of >= 256 bytes run their partitions in an order built on
 * the device in every call: the partitions that lie wholly inside one row ("single-row": table[p].row < M,
 * table[p].entry > rowptr[row], table[p + 1].row == row) go behind all others, sorted by
 * (col[e0] + col[e1 - 1], p), so that the waves in flight gather the same rows of `mat` at the same time.  Only the
 * order of execution changes: results are bit-identical with every setting.
 *   tsamd_spmm_column_order(set): 0 off, 1 auto (the default: calls with E >= 2^20, N >= 4096, E >= 8 N and
 *   power-of-two rows, when the device counts at least layout[5] single-row partitions that are at least an eighth of
 *   all), 2 on for every call in scope; anything else: query.  Returns the setting in force.  Process-wide.
 *   tsamd_spmm_order_layout (inspection and tests; no device work): 0 when tsamd_spmm with these operands keeps
 *   slot = partition, else the mode (1 auto, 2 forced) and
 *     layout[0]  byte offset in `workspace` of the header (uint32): [0] 1 = the order is in force for this call (auto
 *                engaged, or forced; 0 also when one of the builder's key buckets held more than layout[6] keys),
 *                [1] the number of single-row partitions, [2] the largest bucket
 *     layout[1]  byte offset of the slot -> partition map (uint32 [layout[2]], layout[2] = P): the other partitions in
 *                ascending order, then the single-row ones by (key, p); written only when the order is in force
 *     layout[3]  byte offset of the keys (uint32 [P], 0xFFFFFFFF = not single-row)
 *     layout[4]  the builder's bucket of a key is key >> layout[4] (buckets only bound its work; the order is exact). */
int tsamd_spmm_column_order(int set);
int tsamd_spmm_order_layout(int dtype, int reduce, int64_t B, int64_t M, int64_t N, int64_t K, int64_t E,
                            const void *mat, const void *out, void *workspace, int64_t *layout);

/* The same product with the entries of the CSR taken through a permutation: entry e is
 * (col[perm[e]], value[perm[e]]), perm [E] int64.  With (rowptr, col, perm) = (colptr, row, csr2csc)
 * this multiplies by the TRANSPOSE of a matrix straight from its COO/CSR arrays -- the
 * grad_mat = A^T * grad_out of SPMMSum::backward (csrc/spmm.cpp:100-108), where the reference first
 * materialises row.index_select(0, csr2csc) and value.index_select(0, csr2csc).  arg_out (MIN/MAX)
 * holds positions in the permuted order (e, not perm[e]).  Workspace: tsamd_spmm_workspace_bytes. */
int tsamd_spmm_permuted(int dtype, int reduce, const int64_t *rowptr, const int64_t *col,
                        const void *value, const int64_t *perm, const void *mat, void *out,
                        int64_t *arg_out, int64_t B, int64_t M, int64_t N, int64_t K, int64_t E,
                        void *workspace, size_t workspace_bytes, void *stream);

/* Partial product of ONE COLUMN BLOCK of a matrix, combined into the result of the blocks before it -- the
 * building block of the overlapped all-gather of the row-sharded SpMM (pytorch_sparse_amd/parallel.py, SURVEY.md
 * section 8e: "pre-split each rank's CSR into column blocks by owner, run block p's partial SpMM as soon as
 * shard p lands"; the reference has no distributed code, its slicing primitives are torch_sparse/narrow.py:15-42
 * and cat.py:60-114).  (rowptr, col, value) is the CSR of the block's entries only (col = positions in `mat`,
 * the buffer the block's rows of X landed in).  Never copies `mat` (no relabelling), otherwise the kernels of
 * tsamd_spmm.
 *   accumulate = 0   first block: out / arg_out are overwritten;
 *   accumulate = 1   out / arg_out hold the result of the earlier blocks:
 *       SUM       out += block product (accumulator precision, one rounding per block for f16 / bf16);
 *       MEAN      out = (out + block product) / max(deg_rowptr[m + 1] - deg_rowptr[m], 1): pass SUM for every block
 *                 but the last and MEAN with the WHOLE matrix's rowptr (deg_rowptr, required) for the last one;
 *       MIN/MAX   (out, arg_out) = better of the two, ties to the smaller entry id -- the first occurrence in
 *                 the whole row, as csrc/cpu/reducer.h:63-67 -- whatever order the blocks come in.
 *   arg_map  [E] block entry -> entry id of the whole matrix (NULL: identity), reported in arg_out;
 *   arg_none the whole matrix's "no winner" id (its number of entries): rows without entries so far hold
 *            (0, arg_none), rows whose entries so far all lost against the init value (NaN only) hold
 *            (init, arg_none) -- the same final states as tsamd_spmm.
 * After the last block out / arg_out equal tsamd_spmm on the whole matrix: exactly for MIN / MAX, up to the
 * association of the partial sums for SUM / MEAN.  Workspace: tsamd_spmm_partial_workspace_bytes. */
size_t tsamd_spmm_partial_workspace_bytes(int dtype, int reduce, int64_t B, int64_t M, int64_t N, int64_t K,
                                          int64_t E);
int tsamd_spmm_partial(int dtype, int reduce, const int64_t *rowptr, const int64_t *col, const void *value,
                       const void *mat, void *out, int64_t *arg_out, int64_t B, int64_t M, int64_t N, int64_t K,
                       int64_t E, const int64_t *arg_map, int64_t arg_none, int accumulate,
                       const int64_t *deg_rowptr, void *workspace, size_t workspace_bytes, void *stream);

/* Operand cache.  On Kronecker-like graphs tsamd_spmm copies `mat` to hashed row positions before the
 * gather (channel camping, see below) -- 15 % of a north-star call.  A caller that multiplies by the SAME
 * dense operand again (inference with fixed features, the first layer of every training epoch) can keep
 * that copy: tsamd_spmm_cached takes a caller-owned device buffer of tsamd_spmm_operand_cache_bytes()
 * bytes (0 = this product never copies its operand; 256-byte aligned) that holds the copy, the verdict of
 * the camping probe and a fingerprint of `mat` (64 x 256 sampled 16-byte packets).
 *   cache_valid = 0: fill the buffer (the same work as tsamd_spmm);
 *   cache_valid = 1: the buffer was filled by a call with the same (col, E, N, K, dtype, reduce class): the
 *     fingerprint of `mat` is recomputed (microseconds) and the copy kernel returns at once when it still
 *     matches; when it does not, the copy is redone -- the decision is taken on the device, no sync.
 * The CALLER decides whether `mat` can still be the same matrix (the torch glue keys on storage identity,
 * data pointer, version counter, shape and stream); the fingerprint is the second line of defence for writes
 * that bypass such bookkeeping.  Results are bit-identical to tsamd_spmm.  The workspace
 * (tsamd_spmm_cached_workspace_bytes) no longer contains the copy. */
size_t tsamd_spmm_operand_cache_bytes(int dtype, int reduce, int64_t B, int64_t M, int64_t N, int64_t K,
                                      int64_t E);
size_t tsamd_spmm_cached_workspace_bytes(int dtype, int reduce, int64_t B, int64_t M, int64_t N, int64_t K,
                                         int64_t E);
int tsamd_spmm_cached(int dtype, int reduce, const int64_t *rowptr, const int64_t *col, const void *value,
                      const void *mat, void *out, int64_t *arg_out, int64_t B, int64_t M, int64_t N,
                      int64_t K, int64_t E, void *workspace, size_t workspace_bytes, void *cache,
                      size_t cache_bytes, int cache_valid, void *stream);

/* Pattern hints.  Most of what tsamd_spmm does in front of its merge kernel depends on (rowptr, col) alone: the
 * probe's verdict, which 64-id blocks are hot and their ranks, the slot -> partition map of the column order.  A caller
 * that multiplies by the same pattern again keeps those in a device buffer of tsamd_spmm_hints_bytes() bytes (256-byte
 * aligned; 0 = the call is out of scope: only the shapes of the hot-block route -- sum / mean, B = 1, N >= 65536 -- are
 * in it, TSAMD_ERR_UNSUPPORTED otherwise).
 *   state = 1  build: the kernels of tsamd_spmm, writing those arrays into `hints`;
 *   state = 2  reuse: the partition kernel (the table only), the copy of the hot blocks (it reads `mat`), the merge
 *              kernel and the fix-up.  No probe, mark, bits, scatter or rank kernel and no memset.
 * The hints are ADVISORY: they choose addresses and the order of execution, never a value.  `hints` must have been
 * filled by a state-1 call with the same dtype, reduce class, B, M, N, K and E -- that alone makes it fit (block words
 * for N ids, a permutation of the P partitions); what rowptr / col held then, or hold now, does not matter: results are
 * bit-identical to tsamd_spmm with ANY such buffer, a stale one only costs time.  Nothing on the device re-validates it.
 * A build call that takes neither route (narrow packets, column order switched off, verification mode) leaves the
 * verdict "no" for the route it did not build.  Workspace: tsamd_spmm_workspace_bytes, unchanged.
 *   tsamd_spmm_hints_layout (inspection and tests; no device work): 0 out of scope, else 1 and layout[0..7] = byte
 *   offsets in `hints` of the probe's four int counters, the order header (as tsamd_spmm_order_layout, layout[0]), the
 *   128 chunk totals, the block words (as tsamd_spmm_hot_blocks_layout), the per-chunk lists of selected blocks and the
 *   slot -> partition map; then P and the size in bytes. */
size_t tsamd_spmm_hints_bytes(int dtype, int reduce, int64_t B, int64_t M, int64_t N, int64_t K, int64_t E);
int tsamd_spmm_hints_layout(int dtype, int reduce, int64_t B, int64_t M, int64_t N, int64_t K, int64_t E,
                            int64_t *layout);
int tsamd_spmm_hinted(int dtype, int reduce, const int64_t *rowptr, const int64_t *col, const void *value,
                      const void *mat, void *out, int64_t *arg_out, int64_t B, int64_t M, int64_t N, int64_t K,
                      int64_t E, void *workspace, size_t workspace_bytes, void *hints, int state, void *stream);

/* Measurement aid (bench.py): same as tsamd_spmm, but brackets the three
 * kernels of the launch sequence (merge-path partition, merge, carry fix-up)
 * with hipEvents on `stream`, waits for the last one and writes their
 * durations in milliseconds to kernel_ms_host[0..2] (host memory). */
int tsamd_spmm_profiled(int dtype, int reduce, const int64_t *rowptr,
                        const int64_t *col, const void *value, const void *mat,
                        void *out, int64_t *arg_out, int64_t B, int64_t M, int64_t N,
                        int64_t K, int64_t E, void *workspace, size_t workspace_bytes,
                        void *stream, float *kernel_ms_host);

/* ------------------------------------------------------------------------ *
 * Relabelled ("channel-camping free") layout, end to end.  tsamd_spmm fixes the camping of
 * Kronecker-like graphs by copying `mat` to hashed row positions on EVERY call (15 % of a
 * north-star step).  A caller that runs many products with the same matrix (every layer / epoch
 * of a GNN) can instead keep its dense matrices in that layout for good:
 *
 *   position of row i of a [n, K] matrix = tsamd_relabel_ids(i, n)   (a bijection on [0, n))
 *
 *   tsamd_relabel_ids       out[j] = position(ids[j]) (ids == NULL: ids[j] = j, i.e. the whole map);
 *                           ids outside [0, n) are passed through (the reference's "E = no winner").
 *   tsamd_spmm_relabelled   same arithmetic as tsamd_spmm -- bit-identical values -- with
 *                           col_h = position(col) (computed once per matrix), mat_h in relabelled
 *                           row order (positions over N) and out_h / arg_out_h written in
 *                           relabelled row order (positions over M): no probe, no copy, and the
 *                           result feeds the next product as it is.  arg_out_h holds the ORIGINAL
 *                           entry ids (E for "no winner").
 * ------------------------------------------------------------------------ */
int tsamd_relabel_ids(const int64_t *ids, int64_t count, int64_t n, int64_t *out, void *stream);
size_t tsamd_spmm_relabelled_workspace_bytes(int dtype, int reduce, int64_t B, int64_t M,
                                             int64_t N, int64_t K, int64_t E);
int tsamd_spmm_relabelled(int dtype, int reduce, const int64_t *rowptr, const int64_t *col_h,
                          const void *value, const void *mat_h, void *out_h, int64_t *arg_out_h,
                          int64_t B, int64_t M, int64_t N, int64_t K, int64_t E, void *workspace,
                          size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------ *
 * Row gather of a dense row-major matrix: dst[i, :] = src[idx[i], :], rows of `row_bytes` bytes
 * (any element type).  The pack step in front of the row exchange of the sharded SpMM
 * (pytorch_sparse_amd/parallel.py; no reference counterpart: the reference has no distributed code).
 * idx in [-n_src, n_src); negative ids wrap like torch indexing.
 * ------------------------------------------------------------------------ */
int tsamd_gather_rows(const void *src, const int64_t *idx, void *dst, int64_t n, int64_t n_src,
                      int64_t row_bytes, void *stream);

/* ------------------------------------------------------------------------ *
 * Legacy functional SpMM on a SMALL, UNSORTED COO in one launch.  Replaces the
 * ATen composition of torch_sparse/spmm.py:25-31
 *   (matrix.index_select(-2, col) * value.unsqueeze(-1)  ->  scatter_add over row)
 * where launch latency is all that counts (BASELINE.json configs[0]).
 *
 *   out[r, :] = sum over entries e with row[e] == r of value[e] * mat[col[e], :]
 *
 *   row, col [E] int64 in any order, duplicates add up; value [E] dtype (required);
 *   mat [N, K] dtype; out [M, K] dtype, fully written (rows without entries = 0).
 * No workspace, no host sync, no pre-zeroed output.  fp sums are formed in
 * arrival order (like a device scatter_add); integer sums are exact (wrapping).
 * tsamd_spmm_coo_small_supported(...) == 0: use the sorted route (tsamd_sort_coo*
 * + tsamd_ind2ptr + tsamd_spmm); the entry point itself then returns
 * TSAMD_ERR_UNSUPPORTED.
 * ------------------------------------------------------------------------ */
int tsamd_spmm_coo_small_supported(int dtype, int64_t E, int64_t M, int64_t K);
int tsamd_spmm_coo_small(int dtype, const int64_t *row, const int64_t *col,
                         const void *value, const void *mat, void *out,
                         int64_t E, int64_t M, int64_t N, int64_t K, void *stream);

/* ------------------------------------------------------------------------ *
 * Gradient of SUM/MEAN SpMM w.r.t. the sparse values (an SDDMM over the
 * pattern).  Replaces spmm_value_bw_cuda / spmm_value_bw_cpu
 * (csrc/cuda/spmm_cuda.cu:196-237, csrc/cpu/spmm_cpu.cpp:103-152).
 *
 *   out[e] = sum_b sum_k mat[b, col[e], k] * grad[b, row(e), k]
 *            ( / max(deg(row(e)), 1) for MEAN )
 *
 * The reference takes both the COO `row` and `rowptr`; only `rowptr` is
 * needed here (row(e) is implied by the CSR segment), `row` may be NULL.
 * reduce must be TSAMD_SUM or TSAMD_MEAN.  out is [E] dtype, fully written.
 * ------------------------------------------------------------------------ */
int tsamd_spmm_value_bw(int dtype, int reduce, const int64_t *row,
                        const int64_t *rowptr, const int64_t *col,
                        const void *mat, const void *grad, void *out, int64_t B,
                        int64_t M, int64_t N, int64_t K, int64_t E, void *stream);

/* ------------------------------------------------------------------------ *
 * Backward of MIN/MAX SpMM.  Replaces the ATen composition in
 * SPMMMin/SPMMMax::backward (csrc/spmm.cpp:204-242, 264-302):
 *
 *   for every (b, m, k) with a = arg_out[b,m,k] != E:
 *     grad_value[a]            += mat[b, col[a], k] * grad_out[b,m,k]
 *     grad_mat[b, col[a], k]   += value[a] * grad_out[b,m,k]   (value==NULL: 1)
 *
 * grad_value ([E] dtype) and grad_mat ([B,N,K] dtype) may each be NULL (not
 * requested).  Both are fully defined on return (zero where nothing lands).
 *
 * rowptr [M+1] is the CSR pointer of the forward call (the reference's backward does
 * not need it; here it lets grad_value be accumulated per row in LDS and written with
 * plain stores -- no atomics, no memset).  It may be NULL when grad_value is NULL.
 * grad_mat is accumulated with hardware atomics (it is a scatter into the transposed
 * pattern, which this op does not receive): fp32 / fp64 global_atomic_add; f16 / bf16
 * packed global_atomic_pk_add on the final buffer, i.e. one rounding per addition like the
 * reference's own narrow-type scatter_add_, in a non-deterministic order.  Odd K
 * accumulates narrow types in an fp32 workspace instead and
 * rounds once; tsamd_spmm_minmax_bw_workspace_bytes() says how much that takes (0
 * otherwise).
 * ------------------------------------------------------------------------ */
size_t tsamd_spmm_minmax_bw_workspace_bytes(int dtype, int64_t B, int64_t N,
                                            int64_t K, int64_t E);
int tsamd_spmm_minmax_bw(int dtype, const int64_t *rowptr, const int64_t *col,
                         const void *value, const void *mat, const void *grad_out,
                         const int64_t *arg_out, void *grad_value, void *grad_mat,
                         int64_t B, int64_t M, int64_t N, int64_t K, int64_t E,
                         void *workspace, size_t workspace_bytes, void *stream);

/* The same backward as a PULL over the transposed pattern, for callers that hold the CSC arrays
 * (SparseTensor.matmul does: the sum backward uses the same three, csrc/spmm.cpp:84,100-108):
 *   colptr [N+1], csr2csc [E] (CSC position -> CSR entry), row [E] (COO rows of the CSR order).
 * grad_mat is produced column-parallel without atomics:
 *   1. one pass over arg_out writes a winner mask per entry (ceil(K/32) words, bit k = "entry e is the
 *      arg of feature k of its row");
 *   2. the merge-path SpMM kernel runs on (colptr, row, value) through csr2csc with that mask as a
 *      per-(entry, feature) predicate:  grad_mat[b, n, k] = sum_{e in column n, bit k set}
 *      round_T(value[e] * grad_out[b, row[e], k]), accumulated in fp32 (fp64 for f64), rounded once.
 * Deterministic (fixed summation order), every element of grad_mat written exactly once (no memset of
 * the result), the device-scope atomics of tsamd_spmm_minmax_bw are gone.  grad_value: beside grad_mat, a masked
 * SDDMM over the same masks when K * element size is a multiple of 16 and mat and grad_out are 16-byte aligned;
 * otherwise the row-parallel kernel of tsamd_spmm_minmax_bw (no global atomics either).  Either output may be
 * NULL.  Replaces the same ATen composition (csrc/spmm.cpp:204-242, 264-302).
 * Status, in this order, before anything is launched (all three _bw_csc* entries; tests/test_cabi_minmax_bw.py):
 *   INVALID      a negative size; on a non-empty output (B * M * K > 0) a NULL rowptr, col, mat, grad_out or
 *                arg_out; grad_mat wanted, E > 0 and a NULL colptr, csr2csc or row
 *   UNSUPPORTED  a dtype that is not f32 / f64 / f16 / bf16; N, M or E >= 2^32 or K >= 2^31 (32-bit ids inside the
 *                kernels) -- nothing else: this entry serves every combination of outputs and alignments
 *   WORKSPACE    grad_mat wanted on a non-empty problem and the workspace is NULL, smaller than
 *                tsamd_spmm_minmax_bw_csc_workspace_bytes() or not 256-byte aligned */
size_t tsamd_spmm_minmax_bw_csc_workspace_bytes(int dtype, int64_t B, int64_t M, int64_t N, int64_t K,
                                                int64_t E);
int tsamd_spmm_minmax_bw_csc(int dtype, const int64_t *rowptr, const int64_t *col, const void *value,
                             const void *mat, const void *grad_out, const int64_t *arg_out,
                             const int64_t *colptr, const int64_t *csr2csc, const int64_t *row,
                             void *grad_value, void *grad_mat, int64_t B, int64_t M, int64_t N, int64_t K,
                             int64_t E, void *workspace, size_t workspace_bytes, void *stream);

/* min / max whose winners stay inside the caller (SparseTensor.matmul(x, 'min' | 'max') returns `out` only and
 * keeps arg_out for its own backward, torch_sparse/matmul.py:60-77, csrc/spmm.cpp:183-203): the same entry ids as
 * arg_out in 32-bit words -- half the bytes in the forward's store and in the backward's read of them (configs[2]:
 * 1.07 -> 0.54 GB each way).  E < 2^31 ("no winner" = E as in tsamd_spmm).
 *   tsamd_spmm_minmax_arg32: tsamd_spmm / tsamd_spmm_cached (cache == NULL: stateless) for reduce = MIN | MAX with
 *     arg_out32 [B, M, K] int32; workspace = tsamd_spmm_workspace_bytes / tsamd_spmm_cached_workspace_bytes.
 *   tsamd_spmm_minmax_bw_csc_arg32: tsamd_spmm_minmax_bw_csc on those ids, same workspace.  TSAMD_ERR_UNSUPPORTED,
 *     besides what that entry returns it for: E >= 2^31 (checked first of all); grad_value wanted and not computable
 *     as the masked SDDMM, i.e. grad_mat is NULL, K * element size is no multiple of 16, or mat or grad_out is not
 *     16-byte aligned (the row-parallel kernel reads int64 ids: widen them and take tsamd_spmm_minmax_bw / _csc).
 *     A NULL arg_out32 on a non-empty output is INVALID before the dtype is looked at. */
int tsamd_spmm_minmax_arg32(int dtype, int reduce, const int64_t *rowptr, const int64_t *col, const void *value,
                            const void *mat, void *out, int32_t *arg_out32, int64_t B, int64_t M, int64_t N,
                            int64_t K, int64_t E, void *workspace, size_t workspace_bytes, void *cache,
                            size_t cache_bytes, int cache_valid, void *stream);
int tsamd_spmm_minmax_bw_csc_arg32(int dtype, const int64_t *rowptr, const int64_t *col, const void *value,
                                   const void *mat, const void *grad_out, const int32_t *arg_out32,
                                   const int64_t *colptr, const int64_t *csr2csc, const int64_t *row,
                                   void *grad_value, void *grad_mat, int64_t B, int64_t M, int64_t N, int64_t K,
                                   int64_t E, void *workspace, size_t workspace_bytes, void *stream);

/* min / max whose forward leaves the WINNER RECORDS of the pull backward instead of the winner ids (round 6): for a
 * caller that keeps the winners only for its own backward (SparseTensor.matmul(x, 'max') with x.requires_grad:
 * torch_sparse/matmul.py:60-77 -> csrc/spmm.cpp:183-242) the backward's first step -- re-reading the ids and writing one
 * 32-byte record per entry, 0.30 of the 1.36 ms at configs[2] -- is done by the forward where the winners still sit in
 * registers: at the end of every row that one wave finishes by itself it writes the row's records and does not store
 * the ids at all; rows cut between waves get theirs from the ids right behind the forward (a pass that skips every
 * 64-entry chunk without such a row).  Same records bit for bit as tsamd_spmm_minmax_winrec makes from the ids, hence
 * the same gradients bit for bit.  The forward writes records itself for f16 / bf16 rows of 33..256 features and f32 rows
 * of 65..256 (multiples of 4; 97..128 features -- 32-byte records -- have their own, faster kernel instantiation); any other
 * float shape works too (ids to the workspace, then every record from them).
 *   tsamd_spmm_minmax_records_bytes        size of `records` ([B][E] records of 8..  32-bit words, see csrc/spmm_internal.h)
 *   tsamd_spmm_minmax_records              out [B, M, K] and records; row [E] = COO row ids; E < 2^31
 *   tsamd_spmm_minmax_winrec               records from int32 ids (what tsamd_spmm_minmax_bw_csc_arg32 does first)
 *   tsamd_spmm_minmax_bw_csc_records       tsamd_spmm_minmax_bw_csc on such records; has_value: the matrix had values
 *                                          (they are in the records).  TSAMD_ERR_UNSUPPORTED, besides what that entry
 *                                          returns it for: grad_mat is NULL (checked first of all: grad_value alone
 *                                          reads ids); E >= 2^31; grad_value wanted and K * element size no multiple
 *                                          of 16, or mat or grad_out not 16-byte aligned -- there is no id to fall back
 *                                          on.  NULL records with E > 0 on a non-empty output: INVALID, checked second.
 *                                          Workspace: tsamd_spmm_minmax_bw_csc_records_workspace_bytes(), which is the
 *                                          _csc figure less tsamd_spmm_minmax_records_bytes() */
int tsamd_spmm_minmax_records_in_forward(int dtype, int64_t B, int64_t M, int64_t K, int64_t E); /* 1: the merge kernel writes them */
size_t tsamd_spmm_minmax_records_bytes(int64_t B, int64_t K, int64_t E);
size_t tsamd_spmm_minmax_records_workspace_bytes(int dtype, int reduce, int64_t B, int64_t M, int64_t N, int64_t K,
                                                 int64_t E);
int tsamd_spmm_minmax_records(int dtype, int reduce, const int64_t *rowptr, const int64_t *col, const void *value,
                              const void *mat, void *out, const int64_t *row, uint32_t *records, int64_t B, int64_t M,
                              int64_t N, int64_t K, int64_t E, void *workspace, size_t workspace_bytes, void *stream);
int tsamd_spmm_minmax_winrec(int dtype, const int64_t *row, const void *value, const int32_t *arg_out32,
                             uint32_t *records, int64_t B, int64_t M, int64_t K, int64_t E, void *stream);
size_t tsamd_spmm_minmax_bw_csc_records_workspace_bytes(int dtype, int64_t B, int64_t M, int64_t N, int64_t K,
                                                        int64_t E);
int tsamd_spmm_minmax_bw_csc_records(int dtype, const int64_t *rowptr, const int64_t *col, int has_value,
                                     const void *mat, const void *grad_out, const uint32_t *records,
                                     const int64_t *colptr, const int64_t *csr2csc, const int64_t *row,
                                     void *grad_value, void *grad_mat, int64_t B, int64_t M, int64_t N, int64_t K,
                                     int64_t E, void *workspace, size_t workspace_bytes, void *stream);

/* tsamd_spmm_minmax_bw_route (inspection and tests): what a min / max backward call decides before it launches anything.
 * Host arithmetic only -- no HIP call, no device -- through the very plan functions the four entries run.
 *   winners   0 int64 ids (tsamd_spmm_minmax_bw_csc), 1 int32 ids (_arg32), 2 records (_records), 3 none: the bare
 *             scatter entry tsamd_spmm_minmax_bw
 *   want_value / want_mat   whether grad_value / grad_mat are asked for
 *   mat, grad_out, grad_mat count for their alignment only (NULL: aligned); every array the query does not take is
 *             taken as present, the workspace as large enough and 256-byte aligned.
 *   route[0]  status  the TSAMD_* status the entry answers; when it is not TSAMD_OK the other words are 0
 *   route[1]  value   how grad_value is made: 0 not at all, 1 zero fill, 2 masked SDDMM over the records, 3 the
 *                     row-parallel kernel (spmm_minmax_bw_kernel<.., GVAL>: LDS sums)
 *   route[2]  sddmm   masked SDDMM only: 1 spmm_value_bw_masked_kernel (pipelined, <= 64 packets per row),
 *                     2 spmm_value_bw_kernel<.., true>; route[3] its lgG (2^lgG entries side by side)
 *   route[4]  mat     how grad_mat is made: 0 not at all, 1 zero fill, 2 pull (masked sum), 3 scatter (atomics)
 *   route[5]  write_records  pull only: 1 when minmax_winrec_kernel writes the records first (winners 0 and 1)
 *   route[6..8] W, S, has_z  pull only: mask words and stride of a record in 32-bit words, and whether the masked sum
 *                     reads word W + 3 as the non-zero-word bitmap (the padding leaves it and W <= 32)
 *   route[9]  lgG, route[10] cap   scatter / row-parallel kernel: 2^lgG rows side by side, LDS sums per row and pass
 *                     (rows of more than `cap` entries take several passes)
 *   route[11] packed  scatter of grad_mat: 0 per-element atomics (fp32, fp64, or the fp32 shadow), 1 packed f16 / bf16
 *                     atomics whose word mates are lanes (2j, 2j + 1) of a row (even K), 2 packed with the half chosen by
 *                     the element's index (odd K)
 *   route[12] shadow  1 when f16 / bf16 grad_mat goes through an fp32 shadow and narrow_from_f32_kernel (grad_mat not
 *                     4-byte aligned, or B * N * K odd); route[13] the workspace bytes it needs
 *   route[14] items, route[15] P, route[16] fixup, route[17] relabel, route[18] copy, route[19] vec, route[20] lpr,
 *   route[21] lgG, route[22] ktiles, route[24] family   pull only: the words of tsamd_spmm_route for the masked sum --
 *                     the SUM of the transposed problem (N rows, M columns, `grad_out` gathered, `grad_mat` written)
 *                     with relabel 1 in place of 2: no probe of the ids, the copy of grad_out wherever it is possible.
 *                     family is what is launched: 2 (cooperative) at every lgG, also where the plain sum would say 1
 *                     (lgG >= 3) -- the masked kernel has no side-by-side form
 *   route[23]       pull only: the entry's workspace bytes; the other words are 0.
 * TSAMD_ERR_INVALID for route == NULL or winners outside 0 .. 3, TSAMD_OK otherwise. */
int tsamd_spmm_minmax_bw_route(int winners, int dtype, int64_t B, int64_t M, int64_t N, int64_t K, int64_t E,
                               int want_value, int want_mat, const void *mat, const void *grad_out, const void *grad_mat,
                               int64_t route[32]);

/* ------------------------------------------------------------------------ *
 * COO row ids <-> CSR row pointer.  Replace ind2ptr_cuda / ptr2ind_cuda
 * (csrc/cuda/convert_cuda.cu:26-67, csrc/cpu/convert_cpu.cpp:7-57).
 *   ind2ptr: ind [E] sorted ascending, values in [0, M) -> out [M+1];
 *            E == 0 gives all zeros (convert_cpu.cpp:15-16).
 *   ptr2ind: ptr [M+1] -> out [E].
 * ------------------------------------------------------------------------ */
int tsamd_ind2ptr(const int64_t *ind, int64_t M, int64_t E, int64_t *out,
                  void *stream);
int tsamd_ptr2ind(const int64_t *ptr, int64_t M, int64_t E, int64_t *out,
                  void *stream);

/* ------------------------------------------------------------------------
 * Entry-balanced segmented reduction (csrc/segreduce.hip): same result as tsamd_segment_reduce,
 * for segments that may be very long (rows / columns of a power-law matrix:
 * SparseTensor.sum/mean/min/max(dim), torch_sparse/reduce.py:8-67 -> torch_scatter.segment_csr).
 * Work is split by entries, not by segments; deterministic, no atomics; fp32 partial sums of a
 * segment that spans several chunks fold in fp64.  Needs seg_ptr[0] = 0 and seg_ptr[nseg] = E.
 * ------------------------------------------------------------------------ */
size_t tsamd_segment_reduce_balanced_workspace_bytes(int dtype, int64_t E, int64_t D);
int tsamd_segment_reduce_balanced(int dtype, int reduce, const void *value, const int64_t *perm,
                                  const int64_t *seg_ptr, int64_t nseg, int64_t E, int64_t D,
                                  void *out, void *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------
 * Entry-balanced segmented softmax and its backward (csrc/softmax.hip): SparseTensor.softmax(dim), the
 * normalisation of attention layers over the stored entries of every row (perm = NULL, seg_ptr = rowptr) or
 * column (perm = csr2csc, seg_ptr = colptr).  Entry i of the segmented order is element perm ? perm[i] : i of
 * value / y / grad / out / grad_value, each [E, D] contiguous; the output is written in the input's own order.
 *   forward   out = exp(value - m) / s, m and s the maximum and the sum of exp(value - m) of the entry's segment
 *             and head (column of D); a segment alone behaves as torch.softmax does on it: -inf gives 0, a
 *             segment of -inf only, or one that holds +inf or a NaN, is all NaN; other segments and heads are
 *             not touched by it.  Empty segments write nothing.
 *   backward  grad_value = y * (grad - sum over the segment of grad * y), from the forward's output y.
 * float32 / float16 / bfloat16 accumulate in fp32, float64 in fp64; one rounding on the store.  Work is split by
 * entries; deterministic, no atomics, no host sync.  Needs seg_ptr[0] = 0 and seg_ptr[nseg] = E.
 * Status, in this order: a negative size TSAMD_ERR_INVALID; a non-floating dtype or D > 65535
 * TSAMD_ERR_UNSUPPORTED; E == 0 or D == 0 TSAMD_OK without a launch; a null pointer (or nseg == 0)
 * TSAMD_ERR_INVALID; a missing or short workspace TSAMD_ERR_WORKSPACE.
 *   tsamd_segment_softmax_route (host arithmetic only): out[0] entries per wave chunk, out[1] entries per
 *   workgroup tile, out[2] the largest number of segments a tile stages in LDS, out[3] tail records one fix-up
 *   round folds per wave, out[4..7] = 0.
 *   workspace = 3 * align256(2 * acc * D * nchunks) + 2 * align256(8 * nchunks), nchunks = ceil(E / out[0]),
 *   acc = 8 for float64, else 4 (0 for a dtype that is not supported).
 * ------------------------------------------------------------------------ */
int tsamd_segment_softmax_route(int64_t out[8]);
size_t tsamd_segment_softmax_workspace_bytes(int dtype, int64_t E, int64_t D);
int tsamd_segment_softmax(int dtype, const void *value, const int64_t *perm, const int64_t *seg_ptr,
                          int64_t nseg, int64_t E, int64_t D, void *out, void *workspace,
                          size_t workspace_bytes, void *stream);
int tsamd_segment_softmax_bw(int dtype, const void *y, const void *grad, const int64_t *perm,
                             const int64_t *seg_ptr, int64_t nseg, int64_t E, int64_t D, void *grad_value,
                             void *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------
 * Sparse attention over a pattern (csrc/sddmm.hip, csrc/spmm_heads.hip): the scores before and the aggregation
 * after SparseTensor.softmax, with H heads side by side.  (ptr, ind) is a segmented order of the E entries: the
 * rows through (rowptr, col) with perm = NULL, the columns through (colptr, row) with perm = csr2csc.  Entry i of
 * that order is element p(i) = perm ? perm[i] : i of the [E, H] array (out of the SDDMM, value of the SpMM); its
 * segment is s(i) (ptr[s] <= i < ptr[s + 1]), its source ind[i].  All arrays are contiguous; float32, float64,
 * float16 and bfloat16; float32 / float16 / bfloat16 accumulate in fp32, float64 in fp64, one rounding on the
 * store.  Work is split by entries, never by segments; deterministic (two calls give the same bits), no
 * floating-point atomics, no host sync.  Needs ptr[0] = 0 and ptr[nseg] = E.
 *
 *   tsamd_sddmm_heads   out[p(i), h] = scale * sum_d q[s(i), h, d] * k[ind[i], h, d];  q [nseg, H, D],
 *                       k [nsrc, H, D].  row [E] holds s(i) in the segmented order, or is NULL: then s(i) is
 *                       searched in ptr (one of row / ptr may be NULL, not both).  One launch, no workspace.  A
 *                       non-finite element of q (k) reaches the scores of its head on its row (column) only.
 *   tsamd_spmm_heads    out[s, h, :] = sum over i in [ptr[s], ptr[s+1]) of value[p(i), h] * x[ind[i], h, :];
 *                       x [nsrc, H, D], out [nseg, H, D], value NULL = all ones.  out is zeroed first: segments
 *                       without entries are zeros and out is fully defined on return.  A segment cut by a chunk
 *                       boundary leaves head / tail records (accumulator rows of H * D) that one fix-up launch
 *                       adds in chunk order (fp32 records fold in fp64): a fixed combine tree.  A non-finite
 *                       product reaches the outputs of the segment that holds the entry, in that head, only.
 *
 * Status, in this order: a negative size TSAMD_ERR_INVALID; a non-floating dtype, or nseg / nsrc / H / D /
 * H * D above 2^31 - 1 (the SpMM: H * D above 65535 * 64), or an E whose byte offsets leave int64,
 * TSAMD_ERR_UNSUPPORTED; then
 *   SDDMM: E == 0, H == 0 or D == 0 TSAMD_OK without a launch; a null out / ind / q / k, row and ptr both null,
 *          or nseg == 0 / nsrc == 0 TSAMD_ERR_INVALID;
 *   SpMM:  nseg * H * D == 0 TSAMD_OK (out has no element); a null out TSAMD_ERR_INVALID; E == 0 TSAMD_OK with
 *          out zero-filled; a null ptr / ind / x or nsrc == 0 TSAMD_ERR_INVALID; a missing or short workspace
 *          TSAMD_ERR_WORKSPACE.  Every one of these is decided on the host before the first device call.
 *
 * The *_route calls are host arithmetic only, through the functions the drivers plan with; a null route array or
 * a negative size is TSAMD_ERR_INVALID, a non-floating dtype TSAMD_ERR_UNSUPPORTED.  Only the alignment of the
 * pointers is looked at (NULL counts as aligned).
 *   tsamd_sddmm_heads_route: out[0] route: 0 packets (16-byte loads; D * itemsize a multiple of 16, packets per head
 *   a power of two, q and k on a 16-byte boundary), 1 generic (element loads, any D >= 1); out[1] elements per
 *   load; out[2] lanes per head (the butterfly runs over these); out[3] entries side by side in a wave; out[4]
 *   heads side by side in a group of lanes (H above it takes several passes); out[5] entries per wave window
 *   (64); out[6] entries per workgroup (256); out[7] the most heads a pass holds (16).
 *   tsamd_spmm_heads_route: out[0] route: 0 packets (D * itemsize a multiple of 16, x and out on a 16-byte
 *   boundary), 1 generic; out[1] elements per lane; out[2] lanes per row; out[3] groups (chunks) side by side in a
 *   wave; out[4] entries per chunk = 8 * out[2] (a function of dtype, H, D alone); out[5] entries per workgroup
 *   tile (2048); out[6] the largest number of segments a tile stages in LDS; out[7] column blocks.
 *   workspace = 2 * align256(acc * nchunks * H * D) + 2 * align256(8 * nchunks), nchunks = ceil(E / out[4]),
 *   acc = 8 for float64, else 4 (0 bytes for a dtype or a size that is not supported).
 * ------------------------------------------------------------------------ */
int tsamd_sddmm_heads_route(int dtype, int64_t H, int64_t D, const void *q, const void *k, int64_t out[8]);
int tsamd_sddmm_heads(int dtype, const int64_t *row, const int64_t *ptr, const int64_t *ind, const int64_t *perm,
                      const void *q, const void *k, double scale, void *out, int64_t nseg, int64_t nsrc,
                      int64_t H, int64_t D, int64_t E, void *stream);
int tsamd_spmm_heads_route(int dtype, int64_t H, int64_t D, const void *x, const void *out, int64_t out_route[8]);
size_t tsamd_spmm_heads_workspace_bytes(int dtype, int64_t nseg, int64_t H, int64_t D, int64_t E);
int tsamd_spmm_heads(int dtype, const int64_t *ptr, const int64_t *ind, const int64_t *perm, const void *value,
                     const void *x, void *out, int64_t nseg, int64_t nsrc, int64_t H, int64_t D, int64_t E,
                     void *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------
 * Fused attention over a pattern (csrc/attention.hip): scores, softmax over the row and aggregation in one pass.
 * (rowptr, col) is the CSR order of the E entries; q [nseg, H, D], k and v [nsrc, H, D], out [nseg, H, D],
 * lse [nseg, H] in the accumulator type (float, double for float64).  bias is NULL or holds one element of the
 * operands' dtype per entry (bias_heads = 1, shared by the heads) or per entry and head (bias_heads = H, [E, H]).
 * All arrays are contiguous; float32, float64, float16 and bfloat16; fp32 accumulators (fp64 for float64), one
 * rounding on the store.  Work is split by entries, never by rows; deterministic (two calls give the same bits), no
 * atomics, no host sync.  Needs rowptr[0] = 0 and rowptr[nseg] = E.
 *
 *   tsamd_attention_heads     s(i, h) = scale * <q[r, h, :], k[col[i], h, :]> + bias for the entries i of row r;
 *                             out[r, h, :] = sum_i softmax_i(s(., h)) * v[col[i], h, :], lse[r, h] = log sum_i
 *                             exp(s(i, h)).  The softmax is online (running maximum, e = __expf in fp32, exp in
 *                             fp64); nothing of size E is written.  out is zeroed and lse set to -inf first: rows
 *                             without entries are zeros.  A row cut by a chunk boundary leaves head / tail records
 *                             ((m, l) per head and an accumulator row of H * D) that one fix-up launch folds in
 *                             chunk order, every piece rescaled to the running maximum.  At most three launches
 *                             (fill, tile, fix-up).  A NaN or +inf score makes its row and head NaN (lse NaN), a row
 *                             of -inf scores only is NaN with lse = -inf, -inf beside finite scores weighs zero;
 *                             nothing else is touched.
 *   tsamd_attention_heads_bw  per entry i of row r and head h, from the forward's out and lse:
 *                             p = e(s(i, h) - lse[r, h]), ds = p * (<grad_out[r, h], v[col[i], h]> -
 *                             <grad_out[r, h], out[r, h]>), both [E, H] of the operands' dtype in storage order.
 *                             lse[r, h] not finite: p = ds = NaN; s = -inf: p = ds = 0.  row [E] holds the row ids
 *                             or is NULL (then they are searched in rowptr; not both NULL).  One launch, no
 *                             workspace.  The gradients follow through tsamd_spmm_heads: grad_q = scale *
 *                             spmm(rows; ds, k), grad_k = scale * spmm(columns; ds, q), grad_v = spmm(columns; p,
 *                             grad_out), grad_bias = ds.
 *
 * Status, in this order: a negative size TSAMD_ERR_INVALID; a non-floating dtype, or nseg / nsrc / H / D / H * D
 * above 2^31 - 1, more than 65535 column blocks, an out above 2^39 elements, or an E whose byte offsets leave int64,
 * TSAMD_ERR_UNSUPPORTED; a bias with bias_heads other than 1 or H TSAMD_ERR_INVALID; then
 *   forward:  nseg * H * D == 0 TSAMD_OK, nothing is written (D == 0 leaves lse undefined); a null out / lse
 *             TSAMD_ERR_INVALID; E == 0 TSAMD_OK with out zero-filled and lse = -inf; a null rowptr / col / q / k / v
 *             or nsrc == 0 TSAMD_ERR_INVALID; a missing or short workspace TSAMD_ERR_WORKSPACE;
 *   backward: E == 0 or H == 0 TSAMD_OK without a launch; D == 0, a null array (row and rowptr both), nseg == 0 or
 *             nsrc == 0 TSAMD_ERR_INVALID.
 * Every one of these is decided on the host before the first device call.
 *
 * tsamd_attention_heads_route is host arithmetic only, through the function the driver plans with; a null route
 * array or a negative size is TSAMD_ERR_INVALID, a non-floating dtype TSAMD_ERR_UNSUPPORTED.  Only the alignment of
 * the pointers is looked at (NULL counts as aligned).  out[0] route: 0 packets (16-byte loads and stores;
 * D * itemsize a multiple of 16 and q, k, v, out on a 16-byte boundary), 1 generic (element loads, any D >= 1);
 * out[1] elements per load; out[2] lanes per head (the butterfly runs over these; a lane covers 16 / itemsize
 * adjacent features on both routes); out[3] heads side by side in a group of lanes; out[4] column blocks =
 * ceil(H / out[3]) * out[7]; out[5] entries per chunk = 8 * out[2] * out[3]; out[6] entries per workgroup tile
 * (2048), also the largest number of rows a tile stages in LDS; out[7] feature blocks of a head (1 unless
 * D * itemsize > 1024).  out[2..7] -- hence the workspace -- are a function of (dtype, H, D) alone.
 *   workspace = 2 * align256(acc * nchunks * H * D) + 2 * align256(2 * acc * nchunks * H) + 2 * align256(8 * nchunks),
 *   nchunks = ceil(E / out[5]), acc = 8 for float64, else 4 (0 bytes for a dtype or a size that is not supported).
 * ------------------------------------------------------------------------ */
int tsamd_attention_heads_route(int dtype, int64_t H, int64_t D, const void *q, const void *k, const void *v,
                                const void *out, int64_t out_route[8]);
size_t tsamd_attention_heads_workspace_bytes(int dtype, int64_t H, int64_t D, int64_t E);
int tsamd_attention_heads(int dtype, const int64_t *rowptr, const int64_t *col, const void *bias,
                          int64_t bias_heads, const void *q, const void *k, const void *v, double scale, void *out,
                          void *lse, int64_t nseg, int64_t nsrc, int64_t H, int64_t D, int64_t E, void *workspace,
                          size_t workspace_bytes, void *stream);
int tsamd_attention_heads_bw(int dtype, const int64_t *row, const int64_t *rowptr, const int64_t *col,
                             const void *bias, int64_t bias_heads, const void *q, const void *k, const void *v,
                             const void *out, const void *lse, const void *grad_out, double scale, void *p_out,
                             void *ds_out, int64_t nseg, int64_t nsrc, int64_t H, int64_t D, int64_t E,
                             void *stream);

/* ------------------------------------------------------------------------
 * Fused additive (GAT) attention over a pattern (csrc/attention.hip, the kernels above in their additive score
 * mode): the score of an entry is a sum of one scalar per node and head inside a leaky ReLU, not a dot product.
 * (rowptr, col) is the CSR order of the E entries; a_dst [nseg, H], a_src [nsrc, H], v [nsrc, H, D], out
 * [nseg, H, D], lse [nseg, H] in the accumulator type A (float, double for float64); nseg != nsrc is allowed.  bias
 * is NULL or holds one element of the operands' dtype per entry (bias_heads = 1) or per entry and head (bias_heads =
 * H, [E, H]).  All arrays are contiguous and share one dtype (float32, float64, float16, bfloat16).
 *
 *   tsamd_gat_attention_heads     for the entries i of row r and head h, in A:
 *                                   z(i, h) = a_dst[r, h] + a_src[col[i], h] (+ bias[i] or bias[i, h])
 *                                   s(i, h) = z > 0 ? z : negative_slope * z     (torch's leaky_relu, also at z == 0
 *                                                                                 and for NaN)
 *                                   out[r, h, :] = sum_i softmax_i(s(., h)) * v[col[i], h, :]
 *                                   lse[r, h]    = log sum_i exp(s(i, h)).
 *                                 The bias goes INSIDE the activation (where GATConv puts its edge term), unlike the
 *                                 bias of tsamd_attention_heads, which is added to the finished score.
 *                                 negative_slope is any finite double (0.2 in GATConv).  Rows without entries are
 *                                 zeros with lse = -inf.  Non-finite scores as in tsamd_attention_heads: a NaN or
 *                                 +inf score makes its row and head NaN (lse NaN), a row of -inf scores only is NaN
 *                                 with lse = -inf, -inf beside finite scores weighs zero.  A -inf bias masks its
 *                                 entry only for negative_slope > 0: with a slope of 0 the IEEE product 0 * -inf is
 *                                 NaN (and a negative slope turns it into +inf); this is not special-cased.
 *                                 a_dst and a_src are read by element loads and need no alignment; the packet route
 *                                 needs D * itemsize a multiple of 16 and v and out on a 16-byte boundary.  Lane
 *                                 map, chunk, records and workspace are those of tsamd_attention_heads:
 *                                 tsamd_attention_heads_route(dtype, H, D, NULL, NULL, v, out, route) and
 *                                 tsamd_attention_heads_workspace_bytes(dtype, H, D, E) serve this call.  Three
 *                                 launches (fill, tile, fix-up), deterministic, no atomics, no host sync, nothing
 *                                 of size E written.
 *   tsamd_gat_attention_heads_bw  per entry i of row r and head h, from the forward's out and lse:
 *                                   p  = e(s(i, h) - lse[r, h])
 *                                   ds = p * (<grad_out[r, h], v[col[i], h]> - <grad_out[r, h], out[r, h]>)
 *                                   dz = ds * (z > 0 ? 1 : negative_slope)
 *                                 p and dz are stored as [E, H] of the operands' dtype in storage order.  lse[r, h]
 *                                 not finite: p = dz = NaN; s = -inf: p = dz = 0.  row [E] holds the row ids or is
 *                                 NULL (then they are searched in rowptr; not both NULL).  One launch, no workspace.
 *                                 The gradients follow: grad_a_dst[r, h] = the sum of dz over the row, grad_a_src[n,
 *                                 h] = the sum of dz over the column (tsamd_segment_reduce), grad_bias = dz (summed
 *                                 over the heads for a [E] bias), grad_v = spmm(columns; p, grad_out)
 *                                 (tsamd_spmm_heads).
 *
 * Status: as tsamd_attention_heads and tsamd_attention_heads_bw, case for case and in their order, with a_dst for
 * q and a_src for k.  Every one is decided on the host before the first device call.
 * ------------------------------------------------------------------------ */
int tsamd_gat_attention_heads(int dtype, const int64_t *rowptr, const int64_t *col, const void *bias,
                              int64_t bias_heads, const void *a_dst, const void *a_src, const void *v,
                              double negative_slope, void *out, void *lse, int64_t nseg, int64_t nsrc, int64_t H,
                              int64_t D, int64_t E, void *workspace, size_t workspace_bytes, void *stream);
int tsamd_gat_attention_heads_bw(int dtype, const int64_t *row, const int64_t *rowptr, const int64_t *col,
                                 const void *bias, int64_t bias_heads, const void *a_dst, const void *a_src,
                                 const void *v, const void *out, const void *lse, const void *grad_out,
                                 double negative_slope, void *p_out, void *dz_out, int64_t nseg, int64_t nsrc,
                                 int64_t H, int64_t D, int64_t E, void *stream);

/* ------------------------------------------------------------------------
 * Dropout on the probabilities of the two fused calls (csrc/attention.hip, the DROP instantiations of the same
 * kernels).  Each entry has the signature of its plain twin with `double dropout, uint64_t seed` after the scalar.
 *
 * The mask is a pure function of (seed, e, h), e the entry's position in CSR storage order and h its head:
 *     thr  = (uint32) floor(dropout * 2^32)
 *     r    = philox(seed, c_lo = e >> 2, c2 = (uint32) h, c3 = 0xD20B)       Philox4x32-10, key = (lo32, hi32) of seed
 *     keep = (r.x, r.y, r.z, r.w)[e & 3] >= thr
 *     c    = 1 / (1 - dropout)          computed in double, used in the accumulator type
 * It does not depend on the route, the lane map, the chunking, the feature block or the dtype; forward and backward
 * recompute it and nothing of size E is stored for it.
 *
 *   forward   out[r, h, :] = sum_i softmax_i(s(., h)) * keep(i, h) * c * v[col[i], h, :].  The softmax itself is the
 *             plain call's -- a dropped entry still counts in the denominator -- so lse is the plain call's lse bit
 *             for bit and out is NaN exactly where the plain call's is; records, fix-up, fill, workspace and
 *             tsamd_attention_heads_route are unchanged.
 *   backward  with p = e(s - lse), dp = <grad_out[r, h], v[col[i], h]>, delta = <grad_out[r, h], out[r, h]> (out is the
 *             forward's out WITH dropout): p_out = pt = p * keep * c and ds = p * (keep * c * dp - delta) (dz = ds *
 *             (z > 0 ? 1 : negative_slope) for the additive call).  lse not finite: NaN both; s = -inf: 0 both.  The
 *             gradients follow as for the plain calls with pt in the place of p: grad_v = spmm(columns; pt, grad_out).
 *
 * Status: a dropout that is NaN, negative or >= 1 is TSAMD_ERR_INVALID, before every other case; then the twin's cases
 * in the twin's order.  dropout == 0 runs the twin's kernels and gives the twin's bits.
 *
 * tsamd_attention_dropout_mask is host arithmetic only, through the function the kernels compile: keep[(e - e0) * H +
 * h] = 1 where entry e in [e0, e0 + n) keeps head h, else 0.  A null array, a negative e0, n or H, or a rate that is
 * NaN or outside [0, 1) is TSAMD_ERR_INVALID.
 * ------------------------------------------------------------------------ */
int tsamd_attention_heads_dropout(int dtype, const int64_t *rowptr, const int64_t *col, const void *bias,
                                  int64_t bias_heads, const void *q, const void *k, const void *v, double scale,
                                  double dropout, uint64_t seed, void *out, void *lse, int64_t nseg, int64_t nsrc,
                                  int64_t H, int64_t D, int64_t E, void *workspace, size_t workspace_bytes,
                                  void *stream);
int tsamd_attention_heads_dropout_bw(int dtype, const int64_t *row, const int64_t *rowptr, const int64_t *col,
                                     const void *bias, int64_t bias_heads, const void *q, const void *k,
                                     const void *v, const void *out, const void *lse, const void *grad_out,
                                     double scale, double dropout, uint64_t seed, void *p_out, void *ds_out,
                                     int64_t nseg, int64_t nsrc, int64_t H, int64_t D, int64_t E, void *stream);
int tsamd_gat_attention_heads_dropout(int dtype, const int64_t *rowptr, const int64_t *col, const void *bias,
                                      int64_t bias_heads, const void *a_dst, const void *a_src, const void *v,
                                      double negative_slope, double dropout, uint64_t seed, void *out, void *lse,
                                      int64_t nseg, int64_t nsrc, int64_t H, int64_t D, int64_t E, void *workspace,
                                      size_t workspace_bytes, void *stream);
int tsamd_gat_attention_heads_dropout_bw(int dtype, const int64_t *row, const int64_t *rowptr, const int64_t *col,
                                         const void *bias, int64_t bias_heads, const void *a_dst, const void *a_src,
                                         const void *v, const void *out, const void *lse, const void *grad_out,
                                         double negative_slope, double dropout, uint64_t seed, void *p_out,
                                         void *dz_out, int64_t nseg, int64_t nsrc, int64_t H, int64_t D, int64_t E,
                                         void *stream);
int tsamd_attention_dropout_mask(uint64_t seed, double rate, int64_t e0, int64_t n, int64_t H, uint8_t *keep);

/* ------------------------------------------------------------------------ *
 * COO ordering / sorting / coalescing. Replace the Python + ATen +
 * torch_scatter compositions of SparseStorage (torch_sparse/storage.py):
 *
 *   tsamd_coo_order      the `(idx[1:] < idx[:-1]).any()` / `mask.all()` probes
 *                        (storage.py:150-154, 431-441): counts_out[0] = number of
 *                        positions where key decreases, counts_out[1] = number of
 *                        adjacent duplicates, key = row * N + col.  counts_out is
 *                        a DEVICE int64[2]; reading it is the caller's one sync.
 *   tsamd_sort_coo       sort-on-construct (storage.py:149-162, utils.py:14-21):
 *                        stable radix sort by (row, col) -- the order of row * N + col (one most-significant-digit
 *                        scatter + one in-LDS sort per bucket, or one-sweep LSD passes when a bucket overflows);
 *                        E < 2^32 and bits(M) + bits(N) <= 64, else TSAMD_ERR_UNSUPPORTED; writes the sorted
 *                        row / col (either may be NULL) and the permutation.
 *                        Called with (col, row, E, N, M, NULL, NULL, perm) it
 *                        yields csr2csc (storage.py:407-416).
 *   tsamd_coalesce_index adjacent-duplicate compaction of SORTED (row, col)
 *                        (storage.py:436-447): unique pairs to row_out/col_out
 *                        (capacity E), seg_ptr[j] = first input position of
 *                        unique pair j, seg_ptr[nnz] = E (capacity E + 1),
 *                        *nnz_out (device) = number of unique pairs.
 *   tsamd_segment_reduce torch_scatter.segment_csr (storage.py:448-451):
 *                        out[j, :] = REDUCE_{i in [seg_ptr[j], seg_ptr[j+1])}
 *                        value[perm ? perm[i] : i, :], value is [*, D] row-major.
 *                        MEAN on integer types floors, like torch_scatter.
 * ------------------------------------------------------------------------ */
int tsamd_coo_order(const int64_t *row, const int64_t *col, int64_t E, int64_t N,
                    int64_t *counts_out, void *stream);
/* The same probe plus the range check of the constructor (storage.py:113-129: `row.max() < M`, `col.max() < N`)
 * in one pass: counts_out[0..3] = (#descents, #adjacent duplicates, max row id, max col id) -- one transfer
 * instead of three.  The order is taken lexicographically on (row, col), so the number of columns need not be
 * known yet (the constructor may still have to infer it from max col id). */
int tsamd_coo_check(const int64_t *row, const int64_t *col, int64_t E, int64_t *counts_out, void *stream);
/* tsamd_sort_coo decided ON THE DEVICE (no host sync): probes the order into counts_out[0..1] as
 * tsamd_coo_order does; when the input has no descent the radix passes return at once and the outputs are
 * (row, col, identity), otherwise they are those of tsamd_sort_coo.  Same workspace. */
int tsamd_sort_coo_auto(const int64_t *row, const int64_t *col, int64_t E, int64_t M, int64_t N,
                        int64_t *row_out, int64_t *col_out, int64_t *perm_out, int64_t *counts_out,
                        void *workspace, size_t workspace_bytes, void *stream);
/* The same with the order already probed: descents[0] (DEVICE) = #descents of the input, e.g. counts_out[0] of
 * tsamd_coo_check.  Lets a caller enqueue check, sort and the gathers through the permutation back to back
 * and read the check's result only once everything is in flight. */
int tsamd_sort_coo_probed(const int64_t *row, const int64_t *col, int64_t E, int64_t M, int64_t N,
                          int64_t *row_out, int64_t *col_out, int64_t *perm_out, const int64_t *descents,
                          void *workspace, size_t workspace_bytes, void *stream);
/* The three sorts above behind one entry, with the entries' values riding along: mode 0 = tsamd_sort_coo, 1 =
 * tsamd_sort_coo_auto (counts [2] written), 2 = tsamd_sort_coo_probed (counts[0] read), 3 = tsamd_coo_check +
 * tsamd_sort_coo_probed in one go: counts [4] = (#descents, #adjacent duplicates, max row id, max col id) written, the
 * check riding in the sort's first pass over (row, col).  value / value_out
 * (both or neither): arrays of E elements of value_bytes = 4 or 8 bytes; value_out[i] = value[perm_out[i]] is
 * written by the last radix pass (the `value.index_select(0, perm)` of torch_sparse/storage.py:160-161 without a
 * second pass over the permutation).  E < 2^32, bits(M) + bits(N) <= 64. */
int tsamd_sort_coo_values(int mode, const int64_t *row, const int64_t *col, int64_t E, int64_t M, int64_t N,
                          int64_t *row_out, int64_t *col_out, int64_t *perm_out, int64_t *counts,
                          const void *value, void *value_out, int64_t value_bytes, void *workspace,
                          size_t workspace_bytes, void *stream);
/* How the radix kernels rank equal digits (what makes the sorts STABLE, i.e. what fixes the permutation the
 * reference gets from its sort in torch_sparse/storage.py:152-162, 407-416 and the order in which coalesce,
 * storage.py:431-466, reduces duplicates): 0 = one returning LDS atomic per entry -- a stable rank as long as the
 * LDS unit serves the lanes of one instruction in ascending order, which a device-side self-test checks the first
 * time a sort runs in the process -- 1 = ballot matching, independent of that order (slower).  set: -1 = query (runs
 * the self-test if no sort has run yet: one synchronising round trip of 4 bytes; call it once before capturing a
 * stream), 0 / 1 = force a mode, 2 = forget the decision and run the self-test again.  Returns the mode in force. */
int tsamd_sort_rank_mode(int set);
/* tsamd_sort_route: what the sorts above (coalesce = 0) and tsamd_sort_coalesce* (coalesce = 1) decide from the sizes
 * alone, for E entries of an M x N matrix with a riding value of value_bytes = 0 (none), 4 or 8 bytes.  Host
 * arithmetic only -- no HIP call, no device -- through the very functions the driver plans with.
 *   out[0] route   1 = the one-launch sort in LDS (1 <= E <= 8192, 0 < N < 2^32 and max(M, 1) * N <= 2^32; tried
 *                  first), else 0 = nothing to order (E <= 1 or keys of zero bits: a copy + the identity) or 2 = the
 *                  general path
 *   out[1] key_bits, out[2] idx_bits, out[3] packed (position in the key's word), out[4] passes (8-bit one-sweep
 *                  passes).  Route 1: the bits of M * N, 0, 0 and the passes of the one-launch kernel.
 *   out[5] ride    a 4-byte value travels through the one-sweep passes (else the last pass gathers it)
 *   out[6] tiles   workgroups of a one-sweep pass
 *   out[7..15]     the bucket plan: on, levels, strip, bits, bits1, kshift, shift, nb, cap (all 0 when off: below 2^17
 *                  entries, no plan within 14 bucket bits, or a compacting sort whose full-word buckets would cut
 *                  through a key)
 * Routes 0 and 1 leave out[5..15] = 0.  Whether the bucket path or the passes then sort an input of route 2 is
 * decided on the device (a bucket beyond `cap` falls back).  TSAMD_ERR_UNSUPPORTED where the sorts refuse the sizes,
 * TSAMD_ERR_INVALID for negative sizes, a value_bytes other than 0 / 4 / 8 or out == NULL. */
int tsamd_sort_route(int64_t E, int64_t M, int64_t N, int value_bytes, int coalesce, int64_t out[16]);
/* tsamd_sort_header: where a sort of route 2 (and route 0 beyond the one-launch sizes) leaves what it decided on the
 * device, for a caller that owns the workspace and reads it back after the call -- host arithmetic only, from the carve
 * the driver itself uses.  The header is an array of 64-bit words inside the workspace of the sorts above
 * (coalesce = 0, tsamd_sort_coo_workspace_bytes) or of tsamd_sort_coalesce* (coalesce = 1,
 * tsamd_sort_coalesce_workspace_bytes), zeroed by the call's first fill:
 *   out[0] byte offset of the header in that workspace
 *   out[1] word index of the probe's #descents (probing sorts with a bucket plan, and the counts of every probing sort)
 *   out[2] word index of the fast word: 1 = the bucket path sorted this input (and, for a compacting sort, wrote the
 *          compacted outputs itself), 0 = the one-sweep passes did -- a bucket beyond the plan's capacity, an input
 *          without descents, no bucket plan, or an id that does not fit the bit width of its size (an untrusted COO
 *          never reaches the bucket kernels)
 *   out[3] word index of the error word (a look-back that gave up; the launch is aborted then)
 * The one-launch sort (route 1) has no header.  TSAMD_ERR_INVALID for E < 0 or out == NULL. */
int tsamd_sort_header(int64_t E, int coalesce, int64_t out[4]);
size_t tsamd_sort_coo_workspace_bytes(int64_t E);
int tsamd_sort_coo(const int64_t *row, const int64_t *col, int64_t E, int64_t M,
                   int64_t N, int64_t *row_out, int64_t *col_out, int64_t *perm_out,
                   void *workspace, size_t workspace_bytes, void *stream);
/* tsamd_sort_coo_auto + tsamd_coalesce_index in one call -- the functional coalesce / transpose of
 * torch_sparse/coalesce.py:5-25, transpose.py:39-62 (storage.py:149-162 + 431-447 behind them): the distinct
 * (row, col) pairs in row-major order to row_u / col_u (capacity E), the start of every run of equal pairs in the
 * SORTED order to seg_ptr (capacity E + 1, seg_ptr[nnz] = E), counts[0..2] (DEVICE) = (#descents of the input,
 * #adjacent duplicates of the input, #distinct pairs); value_out (nullable, with value: E elements of value_bytes = 4
 * or 8) = the values in sorted order, ready for tsamd_segment_reduce(..., perm = NULL, seg_ptr, ...).  When the bucket
 * path sorts the input the compaction happens while the last kernel writes its output (the sorted ids are never
 * written); otherwise row_tmp / col_tmp (capacity E each) receive the sorted ids and a compaction kernel follows.
 * No host sync; reading counts is the caller's one. */
size_t tsamd_sort_coalesce_workspace_bytes(int64_t E);
int tsamd_sort_coalesce(const int64_t *row, const int64_t *col, int64_t E, int64_t M, int64_t N, int64_t *row_tmp,
                        int64_t *col_tmp, int64_t *row_u, int64_t *col_u, int64_t *seg_ptr, int64_t *counts,
                        const void *value, void *value_out, int64_t value_bytes, void *workspace,
                        size_t workspace_bytes, void *stream);
/* tsamd_sort_coalesce with the reduction of the duplicates' values fused into the bucket sort (round 6) -- the whole
 * of torch_sparse/coalesce.py:5-25 (storage.py:431-466: `segment_csr(value, ptr, reduce)`) behind ONE read of the
 * input: `value` is an [E] array of dtype TSAMD_F32 or TSAMD_I32, `reduce` one of TSAMD_SUM .. TSAMD_MAX.  When the
 * bucket path sorts the input, value_u[p] (capacity E) = REDUCE over the p-th run of equal pairs, taken in sorted
 * (= stable input) order in the accumulator type of tsamd_segment_reduce -- the same bits -- counts[3] (DEVICE) = 1,
 * and NEITHER seg_ptr NOR value_out is written.  Otherwise counts[3] = 0 and the call leaves exactly what
 * tsamd_sort_coalesce leaves (seg_ptr, value_out = the values in sorted order): the caller reduces them with
 * tsamd_segment_reduce once it has read counts.  counts has FOUR entries here.  value / value_out / value_u may be
 * NULL together: index only (the common `coalesce(edge_index)` of a graph without edge attributes) -- counts[3] = 0
 * and the bucket route writes NO seg_ptr (8 bytes per entry nobody would read).  Workspace: tsamd_sort_coalesce's. */
int tsamd_sort_coalesce_reduce(const int64_t *row, const int64_t *col, int64_t E, int64_t M, int64_t N,
                               int64_t *row_tmp, int64_t *col_tmp, int64_t *row_u, int64_t *col_u, int64_t *seg_ptr,
                               int64_t *counts, int dtype, int reduce, const void *value, void *value_out,
                               void *value_u, void *workspace, size_t workspace_bytes, void *stream);
size_t tsamd_coalesce_workspace_bytes(int64_t E);
int tsamd_coalesce_index(const int64_t *row, const int64_t *col, int64_t E,
                         int64_t *row_out, int64_t *col_out, int64_t *seg_ptr,
                         int64_t *nnz_out, void *workspace, size_t workspace_bytes,
                         void *stream);
int tsamd_segment_reduce(int dtype, int reduce, const void *value, const int64_t *perm,
                         const int64_t *seg_ptr, int64_t nseg, int64_t D, void *out,
                         void *stream);

/* Device-wide exclusive scan of int64 (building block, exported for tests and hosts):
 * out[i] = sum_{j<i} in[j]; in == out allowed; *total (device, nullable) = sum of all. */
size_t tsamd_exclusive_scan_workspace_bytes(int64_t n);
int tsamd_exclusive_scan_i64(const int64_t *in, int64_t *out, int64_t n, int64_t *total,
                             void *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------ *
 * SpSpMM  C = A * B  (CSR x CSR -> CSR, sum).  Replaces the torch.sparse.mm
 * call behind spspmm_sum (torch_sparse/matmul.py:94-111) and therefore the
 * functional spspmm (torch_sparse/spspmm.py:6-33).  Result contract = what the
 * reference relies on (matmul.py:104-111): every row of C sorted by column,
 * duplicates summed, explicit zeros kept.  fp32 / fp64 only (torch.sparse.mm
 * rejects the other dtypes too).  Count first, write once -- the host allocates between the
 * stages:
 *
 *   1. tsamd_spspmm_plan      prod[M] = products per row of A (sum of the lengths of the B rows
 *        it references); bins[2*M] = ids of the rows with more than 512 products by size class
 *        (medium <= 4096 | large, M slots each; rows of <= 512 products are not listed, their
 *        kernels run over all rows in natural order); stats (DEVICE int64[8]): [2]=#medium
 *        [3]=#large  [4]=products in large rows  [5]=products of the largest row (must be < 2^31: the
 *        per-(row, column range) counters of stage 2 are 32-bit; the caller rejects bigger rows).  colB32 [nnz(B)] = the column ids of B as 32-bit
 *        words (caller-allocated): stages 2 and 4 gather short B rows from all over the array and read
 *        this copy (half the lines per row).
 *        --> host reads stats (sync 1: grid sizes and the workspace of the large rows).
 *   2. tsamd_spspmm_symbolic  nnzC[i] = exact number of entries of row i of C (LDS hash sets for
 *        small / medium rows; large rows: products binned by column range into `workspace`
 *        -- 4 + sizeof(value) bytes per product, which stage 4 reuses -- and counted with LDS
 *        bitmaps).  nnzC has M entries, all written.  `dtype` is the value type of stage 4 (it
 *        fixes the width of a column range).  bin_values != 0: the products of the large rows are
 *        binned together with their values (valA / valB of type `dtype`, either may be NULL = ones),
 *        and stage 4 is then called with values_binned = 1 and does not expand those rows again;
 *        with bin_values = 0 (structure only, or values not known yet) valA / valB are ignored.
 *   3. host: rowptrC = exclusive scan of nnzC over M + 1 entries (tsamd_exclusive_scan_i64, entry
 *        M = 0), reads nnz(C) (sync 2), allocates colC / valC at their FINAL size.
 *   4. tsamd_spspmm_numeric   every row is expanded, sorted by column (registers / LDS), its equal
 *        columns summed in product order (large rows: in a fixed order too up to 2048 column ranges; beyond
 *        that -- tsamd_spspmm_route: sub = 1 -- in atomic order, values not bit-reproducible), and
 *        stored at rowptrC[i].  valA / valB may be NULL (all ones); valC may be NULL (structure
 *        only).  `workspace` is the one stage 2 filled.
 * M < 2^31, N < 2^32 - 1.
 *
 * tsamd_spspmm_route: which kernels stages 2 and 4 take for B with N columns and values of `dtype`
 * (host arithmetic only, no HIP call, no device needed).  out[0] = log2 of the columns per range of
 * the large-row path; [1] = number of ranges; [2] = wave segments per (row, range) bin: 4 = the
 * sums of the large rows are bit-reproducible run to run, 1 = bins above 1024 products are summed
 * in atomic order (more than 2048 ranges: N > 2^24 fp32, N > 2^23 fp64); [3] = 1 when the bin
 * kernel keeps its segment offsets in LDS, 0 = read from global memory; [4] = small rows: 0 =
 * register sort of 32-bit (column, index) keys, 1 = one-wave radix sort of (column, value) pairs
 * (N > 2^23); [5] = 8-bit radix passes of that sort; [6] = 1 when the symbolic hash sets use the
 * 24-bit multiply (N <= 2^24); [7] = 1 when rows of more than 1024 products are supported (at most
 * 8192 ranges: N <= 2^26 fp32, N <= 2^25 fp64), 0 = tsamd_spspmm_symbolic returns
 * TSAMD_ERR_UNSUPPORTED for an operand that has such a row.  N outside [0, 2^32 - 1) or a dtype
 * other than fp32 / fp64: TSAMD_ERR_UNSUPPORTED.
 * ------------------------------------------------------------------------ */
int tsamd_spspmm_route(int dtype, int64_t N, int64_t out[8]);
int tsamd_spspmm_plan(const int64_t *rowptrA, const int64_t *colA, const int64_t *rowptrB,
                      const int64_t *colB, int64_t nnzB, int64_t M, int64_t *prod, int64_t *bins,
                      uint32_t *colB32, int64_t *stats, void *stream);
size_t tsamd_spspmm_workspace_bytes(int dtype, int64_t n_large, int64_t P_large, int64_t N);
int tsamd_spspmm_symbolic(int dtype, const int64_t *rowptrA, const int64_t *colA, const void *valA,
                          const int64_t *rowptrB, const uint32_t *colB32, const void *valB, int bin_values,
                          int64_t M, int64_t N, const int64_t *prod, const int64_t *bins, int64_t n_medium,
                          int64_t n_large, int64_t P_large, int64_t *nnzC, void *workspace,
                          size_t workspace_bytes, void *stream);
int tsamd_spspmm_numeric(int dtype, const int64_t *rowptrA, const int64_t *colA, const void *valA,
                         const int64_t *rowptrB, const uint32_t *colB32, const void *valB, int64_t M,
                         int64_t N, const int64_t *prod, const int64_t *bins, int64_t n_medium,
                         int64_t n_large, int64_t P_large, const int64_t *rowptrC, int64_t *colC,
                         void *valC, int values_binned, void *workspace, size_t workspace_bytes,
                         void *stream);

/* ------------------------------------------------------------------------ *
 * SpSpMM value gradients (csrc/spspmm_bw.hip).  Serves the autograd node of tsamd::spspmm
 * (csrc/ops_spspmm.cpp), i.e. SparseTensor @ SparseTensor (pytorch_sparse_amd/matmul.py) and the
 * functional spspmm (pytorch_sparse_amd/spspmm.py); the reference's torch.sparse.mm is differentiable
 * in both value tensors but torch_sparse/matmul.py:102 drops the graph at C._values().
 * With C = A * B as tsamd_spspmm_numeric leaves it (structural pattern, rows sorted by column, explicit
 * zeros kept), gC the gradient of valC and pos(i, j) the index of (i, j) in C:
 *
 *   gA[e] = sum_{p in row k of B}    vB[p] * gC[pos(i, colB[p])]      e = (i, k) of A
 *   gB[p] = sum_{e in column k of A} vA[e] * gC[pos(row(e), j)]       p = (k, j) of B
 *
 * Both are one computation -- a SEGMENT (entry of A | entry of B) owns a LIST (row k of B | column k of A),
 * one of (row, col) of the looked-up entry of C is fixed per segment, the other comes from the list -- so
 * the entries take the operands in that generic form (a deviation from one signature per side):
 *
 *              segptr[nrows + 1]  segind[nseg]  listptr          list_ind             list_val
 *   side 0 gA  rowptrA, M         colA, nnzA    rowptrB [K + 1]  colB                 valB | NULL
 *   side 1 gB  rowptrB, K         colB, nnzB    colptrA [K + 1]  rowA in column order valA in column order | NULL
 *
 * list_val NULL = all ones.  fp32 / fp64 only (TSAMD_ERR_UNSUPPORTED otherwise).  Work is balanced by
 * products: tiles of out[0] consecutive products, sums in a fixed order, no atomics -- two calls return the
 * same bits.  No buffer proportional to the number of products P beyond two carry records per tile.
 *
 *   tsamd_spspmm_bw_route   host arithmetic only.  out[0] = products per tile; out[1] = the largest number
 *        of segments a tile may intersect and still stage their pointers in LDS (a tile over more segments
 *        -- long runs of segments with empty lists -- searches global memory: the one further route);
 *        out[2] = products per wave; out[3] = carry records per tile; the rest 0.
 *   tsamd_spspmm_bw_plan    ptr[nseg + 1] = exclusive scan of the list lengths; stats (DEVICE int64[2]):
 *        [0] = bytes of workspace tsamd_spspmm_value_bw needs, [1] = P.  P does not depend on the side.
 *        workspace: tsamd_spspmm_bw_plan_workspace_bytes(nseg).
 *        --> host reads stats (the one sync: the grid and the carry records are sized by P).
 *   tsamd_spspmm_value_bw   grad[nseg], every element written (zeroed inside the call, segments with an
 *        empty list stay 0).  workspace: tsamd_spspmm_bw_workspace_bytes(dtype, P) = stats[0].
 *        nseg = 0 or P = 0: TSAMD_OK, zeros written.  An entry of the product pattern that is missing
 *        in C contributes 0 (never an out-of-range read).
 * ------------------------------------------------------------------------ */
int tsamd_spspmm_bw_route(int dtype, int64_t out[8]);
size_t tsamd_spspmm_bw_plan_workspace_bytes(int64_t nseg);
size_t tsamd_spspmm_bw_workspace_bytes(int dtype, int64_t P);
int tsamd_spspmm_bw_plan(int dtype, int side, const int64_t *segptr, int64_t nrows, const int64_t *segind,
                         int64_t nseg, const int64_t *listptr, int64_t *ptr, int64_t *stats, void *workspace,
                         size_t workspace_bytes, void *stream);
int tsamd_spspmm_value_bw(int dtype, int side, const int64_t *ptr, int64_t P, const int64_t *segptr,
                          int64_t nrows, const int64_t *segind, int64_t nseg, const int64_t *listptr,
                          const int64_t *list_ind, const void *list_val, const int64_t *rowptrC,
                          const int64_t *colC, const void *gC, void *grad, void *workspace,
                          size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------
 * Sub-matrix extraction (the callers either side of the sharded
 * SpMM path).  Pure index work on a sorted pattern; order preserving.
 *
 * select -- pick K segments (rows of a CSR, or columns of a CSC) by id, duplicates and
 * negative (wrapping) ids allowed.  Replaces torch_sparse/index_select.py:13-68 (rowcount[idx],
 * cumsum, repeat_interleave, torch_scatter.gather_csr, fancy-index gathers).
 *   1. tsamd_select_plan: out_ptr[K+1] = exclusive scan of the picked segment lengths;
 *        info[0] = total entries, info[1] = number of ids outside [-S, S)  (device, 2 int64).
 *   2. host reads info (the one sync: the output size is data dependent), allocates.
 *   3. tsamd_select_fill: for output entry e of output segment i:
 *        seg_out[e] = i, ind_out[e] = ind[src], pos_out[e] = src  with
 *        src = ptr[idx[i]] + (e - out_ptr[i]).  Any of the three outputs may be NULL.
 *
 * filter -- keep the entries of a COO list that satisfy a predicate.  Replaces the
 * boolean-mask compositions of torch_sparse/narrow.py:44-50, masked_select.py:15-90 and
 * diag.py:10-17 (compare -> nonzero -> gathers).
 *   1. tsamd_filter_plan: pos[n+1] = exclusive scan of the keep flags, *count = kept entries.
 *        pred TSAMD_KEEP_COL_RANGE: a <= col < a + b      TSAMD_KEEP_OFF_DIAG: row != col - a
 *        TSAMD_KEEP_MASK: mask[i]   TSAMD_KEEP_MASK_ROW: mask[row[i]]   TSAMD_KEEP_MASK_COL:
 *        mask[col[i]]   (mask = one byte per element, non-zero keeps)   TSAMD_KEEP_COL_MAPPED:
 *        map[col[i]] >= 0  (map = int64 per column id).  With TSAMD_KEEP_MASK and
 *        row = col = NULL, pos is the rank of every set mask byte (new id of a kept row/column).
 *   2. host reads *count, allocates.
 *   3. tsamd_filter_apply: kept entry i goes to slot pos[i]:
 *        row_out = (row_map ? row_map[row] : row) - row_shift, same for col, src_out = i.
 * ------------------------------------------------------------------------ */
enum {
  TSAMD_KEEP_COL_RANGE = 0,
  TSAMD_KEEP_OFF_DIAG = 1,
  TSAMD_KEEP_MASK = 2,
  TSAMD_KEEP_MASK_ROW = 3,
  TSAMD_KEEP_MASK_COL = 4,
  TSAMD_KEEP_COL_MAPPED = 5
};
/* tsamd_index_route: host arithmetic only.  The sizes at which the index kernels (exclusive scan, ind2ptr /
 * ptr2ind, select, filter) change route: out[0] = entries per scan tile (one more scan level for every factor
 * of it); out[1] = entries per tile of ptr2ind / select_fill, also the most segments a tile may intersect and
 * still stage their pointers in LDS (more: it searches global memory in place); out[2] = entries per tile of
 * filter_count / filter_write; out[3] = entries per slice of such a tile; out[4] = ind2ptr: a boundary whose
 * row pointers span this many rows or more is resolved by the long-run kernel; the rest 0. */
int tsamd_index_route(int64_t out[8]);
size_t tsamd_select_workspace_bytes(int64_t K);
int tsamd_select_plan(const int64_t *ptr, int64_t S, const int64_t *idx, int64_t K,
                      int64_t *out_ptr, int64_t *info, void *workspace, size_t workspace_bytes,
                      void *stream);
int tsamd_select_fill(const int64_t *ptr, int64_t S, const int64_t *ind, const int64_t *idx,
                      int64_t K, const int64_t *out_ptr, int64_t total, int64_t *seg_out,
                      int64_t *ind_out, int64_t *pos_out, void *stream);
size_t tsamd_filter_workspace_bytes(int64_t n);
int tsamd_filter_plan(int pred, const int64_t *row, const int64_t *col, const uint8_t *mask,
                      const int64_t *map, int64_t n, int64_t a, int64_t b, int64_t *pos,
                      int64_t *count, void *workspace, size_t workspace_bytes, void *stream);
int tsamd_filter_apply(const int64_t *pos, const int64_t *row, const int64_t *col, int64_t n,
                       const int64_t *row_map, const int64_t *col_map, int64_t row_shift,
                       int64_t col_shift, int64_t *row_out, int64_t *col_out, int64_t *src_out,
                       void *stream);

/* The same filter in two passes over the INPUTS instead of flags + positions per entry (what
 * filter_coo uses; tsamd_filter_plan / _apply stay for callers that need the positions themselves:
 * the mask rank map and the fused set_diag):
 *   tsamd_filter_count  kept entries per 2048-entry tile -> exclusive scan in `workspace`, *count.
 *   host reads *count, allocates.
 *   tsamd_filter_write  re-evaluates the predicate (same arguments!) and writes the kept entries in
 *                       input order at tile offset + rank inside the tile. */
size_t tsamd_filter_tiles_workspace_bytes(int64_t n);
int tsamd_filter_count(int pred, const int64_t *row, const int64_t *col, const uint8_t *mask,
                       const int64_t *map, int64_t n, int64_t a, int64_t b, int64_t *count,
                       void *workspace, size_t workspace_bytes, void *stream);
int tsamd_filter_write(int pred, const int64_t *row, const int64_t *col, const uint8_t *mask,
                       const int64_t *map, int64_t n, int64_t a, int64_t b, const void *workspace,
                       const int64_t *row_map, const int64_t *col_map, int64_t row_shift,
                       int64_t col_shift, int64_t *row_out, int64_t *col_out, int64_t *src_out,
                       void *stream);

/* Column-wise concatenation without a sort (replaces the cat + re-sort of
 * torch_sparse/cat.py:117-165): entry i of one operand goes to slot i + delta[row[i]] of the
 * row-interleaved output, with  delta[r] = out_rowptr[r] + (entries of earlier operands in
 * row r) - rowptr[r];  row_out = row, col_out = col + col_shift, src_out = src_offset + i.
 * Called once per operand on the same output arrays. */
int tsamd_scatter_rows(const int64_t *row, const int64_t *col, int64_t n, const int64_t *delta,
                       int64_t col_shift, int64_t src_offset, int64_t *row_out, int64_t *col_out,
                       int64_t *src_out, void *stream);

/* ------------------------------------------------------------------------
 * Diagonal insertion into a sorted pattern WITHOUT entries on the k-th diagonal.
 * tsamd_num_diag        = length of the k-th diagonal of an M x N matrix.
 * tsamd_non_diag_mask   replaces non_diag_mask_cpu / non_diag_mask_cuda
 *                       (csrc/cpu/diag_cpu.cpp:5-47, csrc/cuda/diag_cuda.cu:9-62):
 *                       mask[E + num_diag] (bytes) is 1 at the slots the existing entries keep
 *                       once the full diagonal is merged in, 0 at the diagonal's slots.
 * tsamd_insert_diag     does the merge itself (replaces the mask + four boolean-mask scatters of
 *                       torch_sparse/diag.py:37-79): row_out/col_out[E + num_diag] is the merged
 *                       sorted pattern, src_out[p] = old position of an existing entry, or
 *                       E + j for the j-th diagonal entry (one gather assembles the values).
 * ------------------------------------------------------------------------ */
int64_t tsamd_num_diag(int64_t M, int64_t N, int64_t k);
int tsamd_non_diag_mask(const int64_t *row, const int64_t *col, int64_t E, int64_t M, int64_t N,
                        int64_t k, uint8_t *mask, void *stream);
int tsamd_insert_diag(const int64_t *row, const int64_t *col, int64_t E, int64_t M, int64_t N,
                      int64_t k, int64_t *row_out, int64_t *col_out, int64_t *src_out, void *stream);
/* Fused remove + insert (set_diag / fill_diag in one pass over a pattern that may still have
 * entries on the k-th diagonal): pos[E + 1] from tsamd_filter_plan(TSAMD_KEEP_OFF_DIAG, ..., a = k);
 * outputs have pos[E] + tsamd_num_diag(M, N, k) entries; src_out[p] = input position of a kept
 * entry, or E + j for the j-th diagonal entry. */
int tsamd_set_diag_apply(const int64_t *pos, const int64_t *row, const int64_t *col, int64_t E,
                         int64_t M, int64_t N, int64_t k, int64_t *row_out, int64_t *col_out,
                         int64_t *src_out, void *stream);

/* ------------------------------------------------------------------------
 * Mini-batch producers.  CPU-only in the reference except the walk.
 *
 * tsamd_random_walk   replaces random_walk_cpu / random_walk_cuda (csrc/cpu/rw_cpu.cpp:5-45,
 *                     csrc/cuda/rw_cuda.cu:10-53).  rand[n, L] are the uniform floats in [0, 1)
 *                     the reference draws with torch::rand; out[n, L + 1], out[w, 0] = start[w],
 *                     out[w, l + 1] = col[rowptr[cur] + int64(rand[w, l] * deg(cur))].
 *                     A node without neighbours keeps the walk where it is.
 *
 * sample_adj (csrc/cpu/sample_cpu.cpp:10-140) = plan + draw + relabel + a per-row sort:
 *   tsamd_sample_plan   out_ptr[n + 1] = exclusive scan of the per-row sample counts
 *                       (num_neighbors < 0: all; with replacement: num_neighbors if deg > 0;
 *                       else min(deg, num_neighbors)); info[0] = total, info[1] = #bad ids.
 *   tsamd_sample_draw   num_neighbors >= 0: e_id[t] = position of the drawn entry, nbr[t] = its
 *                       column.  Without replacement the draws of a row are distinct (keyed
 *                       bijection of [0, deg) evaluated at 0..k-1, see csrc/sample.hip).
 *                       (num_neighbors < 0 is tsamd_select_fill with ind_out = nbr, pos_out = e_id.)
 *                       Every draw is a pure function of (seed, i, j, deg): i = position of the row in idx (NOT the
 *                       node id), j = index of the draw, k = num_neighbors, p = the drawn position in the row,
 *                       e_id = rowptr[idx[i]] + p.  Philox(seed; c_lo, c2, c3) is Philox4x32-10 with counter words
 *                       (lo32(c_lo), hi32(c_lo), c2, c3) and key words (lo32(seed), hi32(seed)); u = x | y << 32 of its
 *                       output (x, y, z, w); mulhi(a, b) = the high 64 bits of the 128-bit product.
 *                         with replacement       p = mulhi(u, deg), u of Philox(seed; i, lo32(j), 0xD4A3 ^ hi32(j))
 *                         deg <= k               p = j (the whole row in stored order)
 *                         k < deg <= 64          Floyd: used = {}; for t = deg - k .. deg - 1, in this order of emission:
 *                                                pick = mulhi(u, t + 1), u of Philox(seed; i, t, 0xF10D); if pick is in
 *                                                used, pick = t; used += pick; the next draw of the row is pick
 *                         deg > 64               p = pi(j): b = bits of deg - 1, h = (b + 1) / 2, keys K[0..5] = x, y,
 *                                                z, w of Philox(seed; i, 0, 0x5A17) then x, y of Philox(seed; i, 1,
 *                                                0x5A17); v = j; repeat { L = v >> h, R = v & (2^h - 1); six rounds r:
 *                                                (L, R) = (R, (L ^ (fmix32(lo32(R * 0x9E3779B1 + K[r])) >> (32 - h)))
 *                                                & (2^h - 1)); v = L << h | R } until v < deg; fmix32 = MurmurHash3's
 *                                                32-bit finaliser
 *                       tsamd_temporal_redraw: pick j of node i copies its (mulhi(u, cnt))-th draw with keep = 1 in
 *                       stored order, cnt = their number, u of Philox(seed; i, lo32(j), 0x7E4D ^ hi32(j)).
 *                       oracle/np_draws.py restates all of it in numpy; docs/design/oracle_parity.md has the seeds.
 *   tsamd_relabel_plan / _apply   replaces the std::unordered_map walk of relabel_cpu /
 *                       relabel_one_hop_cpu / sample_adj_cpu (csrc/cpu/relabel_cpu.cpp:5-155):
 *                       ids in idx[n] keep local id = their position, every other id in nbr[T]
 *                       gets n + (rank of its first occurrence in nbr order).  slot[M] (M = number
 *                       of node ids) and rank[T + 1] are scratch the caller provides; info[0] =
 *                       number of new nodes, info[1] = #ids outside [0, M).  _apply writes
 *                       local[T] and n_id[n + info[0]] (either may be NULL).
 * tsamd_relabel_seed / _extend   the same numbering for MULTI-HOP samplers (neighbor_sample_cpu.cpp:23-133,
 *                       135-400: one std::unordered_map per node type that lives across hops and relations):
 *                       slot[M] is set up ONCE per call and node type (_seed: seeds idx[n] hold -(i + 1), *count
 *                       (device) = n, *err (device) = #ids outside [0, M); a seed listed twice keeps its FIRST position
 *                       with first_wins = 1 -- the map insert of neighbor_sample_cpu.cpp:31, 195 -- else its last); every _extend numbers the ids of
 *                       nbr[T] that are new (n_id[*count + rank] = id, first-occurrence order), turns their slots
 *                       into -(id + 1), writes local[T] (may be NULL) and adds the number of new nodes to *count --
 *                       all on the device: n_id is a buffer of `capacity` ids (the caller knows *count + T as an
 *                       upper bound), *err counts bad ids and appends beyond the capacity.  No host read-back, no
 *                       M-sized fill and no re-seeding per hop.  rank[T + 1] scratch, workspace as _relabel_plan.
 * tsamd_temporal_*    the building blocks of hetero_temporal_neighbor_sample (neighbor_sample_cpu.cpp:222-340: one
 *                     computation tree per root, nodes are (node, root) PAIRS, a neighbour v may be drawn for a node of
 *                     root time t only if node_time[v] <= t).  The constraint is a FLAG per draw (keep[T], int64 0 / 1)
 *                     until the end; one size read-back (info) per relation and hop.
 *   _mark             keep[t] = src_time[nbr[t]] <= f_time[seg[t]] (src_time == NULL: 1); seg[t] = frontier node of draw t.
 *   _redraw           sampling WITH replacement (:268-300): k uniform picks per frontier node among its draws with
 *                     keep = 1 (nbr / e / keep list ALL its neighbours, out_ptr[F + 1] delimits them) -> nbr2, e2, seg2,
 *                     keep2 of F * k entries (keep2 = 0 for a node without a valid neighbour).
 *   _relabel          first-occurrence numbering of the pairs (nbr[t], f_root[seg[t]]) with keep[t] = 1 behind the n pairs
 *                     (old_node, old_root) already numbered (distinct): local[T] (undefined where keep = 0),
 *                     keep_rank[T + 1] / open_rank[T + 1] = exclusive ranks of the kept draws / of the draws that open a new
 *                     pair, info[0] = #kept, info[1] = #new pairs (device).  One stable sort of n + T pairs
 *                     (tsamd_sort_coo); node ids < num_nodes, roots < num_roots.
 *   _emit             after the caller has read info: rows / cols / edges [info[0]] = (local, seg + begin, e) of the kept
 *                     draws, node_out / root_out / time_out [info[1]] = (nbr, f_root[seg], f_time[seg]) of the new pairs.
 * tsamd_subset_assoc  assoc[M] = position of every node in idx, -1 elsewhere (the association
 *                     array of subgraph_cpu, csrc/cpu/saint_cpu.cpp:17-18); *err = #bad ids.
 *                     SAINT sub-graphs are then select + filter(TSAMD_KEEP_COL_MAPPED).
 *
 * ego_k_hop_sample_adj (csrc/cpu/ego_sample_cpu.cpp, CPU-only in the reference): one sub-graph per seed g = idx[g]
 * (duplicates included, each independent).  Every function below ADDS the number of ids outside [0, M) it meets to
 * *err (device, the caller zeroes it once per call) and uses node 0 in their place, so nothing reads out of bounds.
 *   tsamd_ego_seeds     seg_out[g] = g, node_out[g] = idx[g]: the pairs (seed, node) the node sets start from.
 *   tsamd_ego_plan      one hop: out_ptr[F + 1] = exclusive scan of the draws per frontier entry -- the whole row when
 *                       deg <= num_neighbors (both replace modes), else num_neighbors; nothing when num_neighbors < 0;
 *                       *total (device) = number of draws.
 *   tsamd_ego_draw      the T draws of that hop (one lane per draw): nbr[t] = the drawn column, seg_out[t] = fseg of its
 *                       frontier entry.  Without replacement a uniform subset (Floyd up to deg 64, the keyed bijection
 *                       above), with it uniform picks -- tsamd_sample_draw's draws, keyed by (seed, frontier position,
 *                       j).  The next frontier is (nbr, seg_out), duplicates included.
 *   node sets           tsamd_sort_coalesce_reduce, index only, of the pairs (seg, node) of the seeds and all draws with
 *                       sizes (n, M): col_u = n_id (ascending inside a seed), row_u = its seed, ind2ptr(row_u, n) = ptr.
 *   tsamd_ego_roots     root_n_id[g] = position of idx[g] in n_id[ptr[g] : ptr[g + 1]], plus ptr[g].
 *   tsamd_ego_induced_count / _write   the induced sub-graphs.  vptr[D + 1] / V = tsamd_select_plan(rowptr, M, n_id,
 *                       D): virtual entry x (of V) is stored entry e of row n_id[i] in (i, e) order.  _count: *count
 *                       (device) = number of entries whose column lies in the node set of the row's seed n_seg[i];
 *                       _write (same inputs, the workspace of _count): for those, in virtual-entry order, row_out = i,
 *                       col_out = position of the column in n_id, e_id_out = e.  ind2ptr(row_out, D) = the rowptr.
 *
 * hgt_sample (csrc/cpu/hgt_sample_cpu.cpp, CPU-only in the reference): HGT budget sampling.  Per node type ONE 64-bit
 * word per id, alive for the whole call: 0 = untouched, all-ones = seen (listed), anything else = the budget in fixed
 * point (units of 2^-32), and a list of the ids that ever received budget (the candidates).  See csrc/hgt_sample.hip.
 *   tsamd_hgt_seen        word[ids[i]] = seen; *err (device, the caller zeroes it) += #ids outside [0, M).
 *   tsamd_hgt_budget_add  out_ptr[F + 1] / nbr = a tsamd_sample_plan / _draw pair with num_neighbors =
 *                         TSAMD_HGT_MAX_NEIGHBORS, replace = 0 over the new nodes of the destination type.  Every draw
 *                         of a column with c draws adds floor(2^32 / c) to the word of its source unless that is seen
 *                         (one integer atomic: the sums do not depend on the order of arrival); a source whose word was
 *                         0 is appended to cand (order arbitrary).  state[0] (device) = length of cand, state[1] +=
 *                         #ids outside [0, M) + appends beyond `capacity`.
 *   tsamd_hgt_select      k <= #live candidates draws WITHOUT replacement, sequentially proportional to budget^2, as an
 *                         exponential race: key = -log(u) / budget^2, u = Philox(seed, id, hop, type_tag) in (0, 1], the
 *                         k smallest (key as float32, then id) win: out[k] in ascending key order, their words turn
 *                         seen.  Candidates that are seen already (drawn earlier) take no part.  A pure function of
 *                         (seed, hop, type_tag) and the words, whatever the order of cand.  *err += winners asked for
 *                         beyond the live candidates (their out entry is -1).
 *   tsamd_hgt_keys / tsamd_hgt_commit   the two halves of tsamd_hgt_select around its sort, for a caller that sorts the
 *                         candidates of SEVERAL types at once: _keys writes key[C] = (type_tag << 32) | float32 bits of
 *                         the race key (all-ones for a dead entry) and id[C]; after ONE tsamd_sort_coo of the
 *                         concatenated (key, id) arrays with M = (largest tag + 1) << 32, N = largest id space, type
 *                         t's segment starts at the sum of the C of the types with a smaller tag; _commit takes the
 *                         first k entries of that segment (*err += entries that are dead or not of type_tag).  type_tag < 2^16.
 *   tsamd_hgt_check_ids   ids outside [0, M) are counted in *err and replaced by 0 (before a dense array is indexed).
 * ------------------------------------------------------------------------ */
int tsamd_random_walk(const int64_t *rowptr, const int64_t *col, const int64_t *start,
                      const float *rand, int64_t n, int64_t walk_length, int64_t *out,
                      void *stream);
size_t tsamd_sample_workspace_bytes(int64_t n);
int tsamd_sample_plan(const int64_t *rowptr, int64_t M, const int64_t *idx, int64_t n,
                      int64_t num_neighbors, int replace, int64_t *out_ptr, int64_t *info,
                      void *workspace, size_t workspace_bytes, void *stream);
int tsamd_sample_draw(const int64_t *rowptr, const int64_t *col, const int64_t *idx, int64_t n,
                      int64_t num_neighbors, int replace, uint64_t seed, const int64_t *out_ptr,
                      int64_t *e_id, int64_t *nbr, void *stream);
size_t tsamd_relabel_workspace_bytes(int64_t T);
int tsamd_relabel_plan(const int64_t *idx, int64_t n, const int64_t *nbr, int64_t T, int64_t M,
                       int64_t *slot, int64_t *rank, int64_t *info, void *workspace,
                       size_t workspace_bytes, void *stream);
int tsamd_relabel_apply(const int64_t *idx, int64_t n, const int64_t *nbr, int64_t T, int64_t M,
                        const int64_t *slot, const int64_t *rank, int64_t *local, int64_t *n_id,
                        void *stream);
int tsamd_relabel_seed(const int64_t *idx, int64_t n, int64_t M, int64_t *slot, int64_t *count,
                       int64_t *err, int first_wins, void *stream);
int tsamd_relabel_extend(const int64_t *nbr, int64_t T, int64_t M, int64_t *slot, int64_t *rank,
                         int64_t *count, int64_t *local, int64_t *n_id, int64_t capacity, int64_t *err,
                         void *workspace, size_t workspace_bytes, void *stream);
int tsamd_temporal_mark(const int64_t *nbr, const int64_t *seg, int64_t T, const int64_t *src_time,
                        const int64_t *f_time, int64_t *keep, void *stream);
size_t tsamd_temporal_redraw_workspace_bytes(int64_t T);
int tsamd_temporal_redraw(const int64_t *out_ptr, int64_t F, int64_t T, int64_t k, uint64_t seed,
                          const int64_t *nbr, const int64_t *e, const int64_t *keep, int64_t *nbr2, int64_t *e2,
                          int64_t *seg2, int64_t *keep2, void *workspace, size_t workspace_bytes, void *stream);
size_t tsamd_temporal_relabel_workspace_bytes(int64_t n, int64_t T);
int tsamd_temporal_relabel(const int64_t *old_node, const int64_t *old_root, int64_t n, const int64_t *nbr,
                           const int64_t *seg, const int64_t *f_root, const int64_t *keep, int64_t T,
                           int64_t num_nodes, int64_t num_roots, int64_t *local, int64_t *keep_rank,
                           int64_t *open_rank, int64_t *info, void *workspace, size_t workspace_bytes, void *stream);
int tsamd_temporal_emit(const int64_t *nbr, const int64_t *e, const int64_t *seg, const int64_t *f_root,
                        const int64_t *f_time, const int64_t *keep_rank, const int64_t *open_rank,
                        const int64_t *local, int64_t T, int64_t begin, int64_t *rows, int64_t *cols, int64_t *edges,
                        int64_t *node_out, int64_t *root_out, int64_t *time_out, void *stream);
int tsamd_subset_assoc(const int64_t *idx, int64_t n, int64_t M, int64_t *assoc, int64_t *err,
                       void *stream);
int tsamd_ego_seeds(const int64_t *idx, int64_t n, int64_t M, int64_t *seg_out, int64_t *node_out, int64_t *err,
                    void *stream);
size_t tsamd_ego_plan_workspace_bytes(int64_t F);
int tsamd_ego_plan(const int64_t *rowptr, int64_t M, const int64_t *frontier, int64_t F, int64_t num_neighbors,
                   int64_t *out_ptr, int64_t *total, int64_t *err, void *workspace, size_t workspace_bytes, void *stream);
int tsamd_ego_draw(const int64_t *rowptr, const int64_t *col, int64_t M, const int64_t *frontier, const int64_t *fseg,
                   int64_t F, int64_t num_neighbors, int replace, uint64_t seed, const int64_t *out_ptr, int64_t T,
                   int64_t *nbr, int64_t *seg_out, int64_t *err, void *stream);
int tsamd_ego_roots(const int64_t *idx, int64_t n, const int64_t *ptr, const int64_t *n_id, int64_t *root_n_id,
                    void *stream);
size_t tsamd_ego_induced_workspace_bytes(int64_t V);
int tsamd_ego_induced_count(const int64_t *rowptr, const int64_t *col, int64_t M, const int64_t *n_id,
                            const int64_t *n_seg, int64_t D, const int64_t *ptr, const int64_t *vptr, int64_t V,
                            int64_t *count, int64_t *err, void *workspace, size_t workspace_bytes, void *stream);
int tsamd_ego_induced_write(const int64_t *rowptr, const int64_t *col, int64_t M, const int64_t *n_id,
                            const int64_t *n_seg, int64_t D, const int64_t *ptr, const int64_t *vptr, int64_t V,
                            const void *workspace, int64_t *row_out, int64_t *col_out, int64_t *e_id_out, void *stream);
#define TSAMD_HGT_MAX_NEIGHBORS 50
int tsamd_hgt_seen(const int64_t *ids, int64_t n, int64_t M, uint64_t *word, int64_t *err, void *stream);
int tsamd_hgt_budget_add(const int64_t *out_ptr, int64_t F, const int64_t *nbr, int64_t M, uint64_t *word,
                         int64_t *cand, int64_t capacity, int64_t *state, void *stream);
size_t tsamd_hgt_select_workspace_bytes(int64_t C);
int tsamd_hgt_select(const int64_t *cand, int64_t C, uint64_t *word, int64_t M, int64_t k, uint64_t seed,
                     int64_t hop, int64_t type_tag, int64_t *out, int64_t *err, void *workspace,
                     size_t workspace_bytes, void *stream);
int tsamd_hgt_keys(const int64_t *cand, int64_t C, const uint64_t *word, int64_t M, uint64_t seed, int64_t hop,
                   int64_t type_tag, int64_t *key, int64_t *id, void *stream);
int tsamd_hgt_commit(const int64_t *key_sorted, const int64_t *id_sorted, int64_t k, uint64_t *word, int64_t M,
                     int64_t type_tag, int64_t *out, int64_t *err, void *stream);
int tsamd_hgt_check_ids(int64_t *ids, int64_t n, int64_t M, int64_t *err, void *stream);

/* ------------------------------------------------------------------------ *
 * Multilevel k-way graph partitioning (csrc/partition.hip, docs/design/partition.md).  Stands in for the METIS calls
 * behind torch_sparse::partition / partition2 / mt_partition (csrc/metis.cpp:18-64 -> csrc/cpu/metis_cpu.cpp:9-113,
 * METIS_PartGraphKway / METIS_PartGraphRecursive / mtmetis on the CPU; the reference refuses device tensors,
 * csrc/metis.cpp:21-26).  It is a partitioner of its own behind that interface, not a port: no METIS exists for this
 * build.  The entries below are the phases; the level loop with its allocations and read-backs lives in the caller
 * (csrc/ops_partition.cpp).  The working graph is a symmetric CSR (rowptr [n + 1], row / col / weight [E]) without
 * self-loops or duplicates, int64 edge weights >= 0, int64 vertex weights; n and k < 2^31.
 *
 *   tsamd_partition_edges            the entry list of a level: entry e -> (cmap[row], cmap[col], weight) (cmap NULL:
 *        identity, weight NULL: ones), with mirror != 0 its transpose at slot E + e as well (outputs of 2 E entries:
 *        A + A^T, what METIS expects the caller to pass, metis_cpu.cpp:36-42); an entry whose ends coincide is parked
 *        on the key (n_key, 0) with weight 0.  Sorting + coalescing the list (tsamd_sort_coalesce) and summing the
 *        duplicates (tsamd_segment_reduce, TSAMD_I64) gives the level's CSR, the parked entries last.  info (DEVICE
 *        int64[4], zeroed by the caller) += (low 32 bits, high 32 bits of the kept weights, #entries out of range or
 *        negative, #parked entries).
 *   tsamd_partition_vertex_weights   vweight_c[c] = sum of vweight[v] over cmap[v] == c.
 *   tsamd_partition_match            `rounds` handshake rounds of heavy-edge matching: an unmatched vertex proposes to
 *        its heaviest unmatched neighbour u with vweight[v] + vweight[u] <= cap, ties by the larger hash(round, u), then
 *        the smaller u; mutual proposals match.  match[v] = partner or -1; cmap[v] = rank of the pair's leader (the
 *        smaller id; an unmatched vertex leads itself) among the leaders; *n_coarse (DEVICE) = number of leaders.
 *   tsamd_partition_bfs_init / _seed / _step / tsamd_partition_assign      the initial partition: a level-synchronous
 *        BFS, cl[v] = component << 31 | level (-1 unvisited; vertices without edges form one last component).
 *        _init marks the isolated vertices and finds the start (minimum degree, then id); _seed starts component
 *        `component` there (first != 0) or at the smallest unvisited id, state[2] = 1 if there was one; _step adds the
 *        unvisited neighbours of (component, level) at level + 1, state[3] = 1 if any.  state is a DEVICE int64[4]; the
 *        caller reads state[2] / state[3] (one 8-byte read-back per BFS level and per component).  _assign sorts by
 *        (component, level, id), scans vweight in that order and sets part = min(k - 1, floor((prefix + w / 2) k / W)).
 *   tsamd_partition_part_weights     pweight[p] = sum of vweight over part == p (k entries).
 *   tsamd_partition_conn             per vertex, the best ELIGIBLE other part among those it has an edge to: largest
 *        summed weight, ties to the smaller id; eligible = it has room (pweight + vweight[v] <= cap) and lies above
 *        (mode 0) / below (mode 1) the own part, or anywhere (mode 2).  gain = weight to it - weight to the own part.
 *        Modes 0 / 1 keep it (dest[v], gain[v]) when gain > 0 or the own part is over cap, else dest = -1.  Mode 2
 *        (rebalance) reports only for vertices of parts over cap, and falls back to part *lightest (DEVICE, nullable)
 *        with gain = -(weight to the own part) when no adjacent part has room.  Rows of up to 32 entries take a lane,
 *        longer ones a wave with a 128-slot LDS hash, rows touching more parts than that a dense table of k counters
 *        per workgroup in the workspace (64 * k words: nothing is n x k).
 *   tsamd_partition_recount          drops candidates whose gain is no longer positive once the neighbours that move
 *        first (higher gain, then smaller id) are counted at their destinations; acc [n] is scratch.
 *   tsamd_partition_commit           select = 0: sorts the candidates by (dest, gain descending, id), takes a segmented
 *        prefix sum of their weights and resets dest to -1 where the prefix no longer fits cap - pweight[dest];
 *        select = 1: the same by (own part, ...) over the candidates of parts over cap, keeping only the prefix that
 *        covers the part's excess.
 *   tsamd_partition_apply            part[v] = dest[v] where dest[v] >= 0, pweight updated, *moved (DEVICE) += #moves.
 *   tsamd_partition_cut              *cut (DEVICE) = summed weight of the entries whose ends differ (twice the cut).
 *   tsamd_partition_keep_better      cuts (DEVICE int64[2]) = (before, after): when after > before and *over == 0 the
 *        round is undone (part / pweight restored); then cuts[0] = the cut in force, cuts[1] = 0.
 *   tsamd_partition_balance          balance (DEVICE int64[3]) = (#parts over cap, smallest part weight, its smallest id).
 * ------------------------------------------------------------------------ */
int tsamd_partition_edges(const int64_t *row, const int64_t *col, const int64_t *weight, const int64_t *cmap, int64_t E,
                          int64_t n, int64_t n_key, int mirror, int64_t *row_out, int64_t *col_out, int64_t *weight_out,
                          int64_t *info, void *stream);
int tsamd_partition_vertex_weights(const int64_t *vweight, const int64_t *cmap, int64_t n, int64_t n_c,
                                   int64_t *vweight_c, void *stream);
size_t tsamd_partition_match_workspace_bytes(int64_t n);
int tsamd_partition_match(const int64_t *rowptr, const int64_t *col, const int64_t *weight, const int64_t *vweight,
                          int64_t n, int64_t cap, int64_t rounds, int64_t *match, int64_t *cmap, int64_t *n_coarse,
                          void *workspace, size_t workspace_bytes, void *stream);
int tsamd_partition_bfs_init(const int64_t *rowptr, int64_t n, int64_t *cl, int64_t *state, void *stream);
int tsamd_partition_bfs_seed(int64_t *cl, int64_t n, int64_t component, int first, int64_t *state, void *stream);
int tsamd_partition_bfs_step(const int64_t *rowptr, const int64_t *col, int64_t n, int64_t *cl, int64_t component,
                             int64_t level, int64_t *state, void *stream);
size_t tsamd_partition_assign_workspace_bytes(int64_t n);
int tsamd_partition_assign(const int64_t *cl, const int64_t *vweight, int64_t n, int64_t k, int64_t *part,
                           void *workspace, size_t workspace_bytes, void *stream);
int tsamd_partition_part_weights(const int64_t *part, const int64_t *vweight, int64_t n, int64_t k, int64_t *pweight,
                                 void *stream);
size_t tsamd_partition_conn_workspace_bytes(int64_t n, int64_t k);
int tsamd_partition_conn(const int64_t *rowptr, const int64_t *col, const int64_t *weight, const int64_t *vweight,
                         const int64_t *part, const int64_t *pweight, int64_t n, int64_t k, int64_t cap, int mode,
                         const int64_t *lightest, int64_t *dest, int64_t *gain, void *workspace, size_t workspace_bytes,
                         void *stream);
int tsamd_partition_recount(const int64_t *row, const int64_t *col, const int64_t *weight, const int64_t *part,
                            const int64_t *pweight, const int64_t *gain, int64_t n, int64_t E, int64_t cap, int64_t *dest,
                            int64_t *acc, void *stream);
size_t tsamd_partition_commit_workspace_bytes(int64_t n, int64_t k);
int tsamd_partition_commit(int64_t *dest, const int64_t *gain, const int64_t *vweight, const int64_t *part,
                           const int64_t *pweight, int64_t n, int64_t k, int64_t cap, int select, void *workspace,
                           size_t workspace_bytes, void *stream);
int tsamd_partition_apply(const int64_t *dest, const int64_t *vweight, int64_t n, int64_t k, int64_t *part,
                          int64_t *pweight, int64_t *moved, void *stream);
int tsamd_partition_cut(const int64_t *row, const int64_t *col, const int64_t *weight, const int64_t *part, int64_t E,
                        int64_t *cut, void *stream);
int tsamd_partition_keep_better(int64_t *cuts, const int64_t *over, const int64_t *part_old, const int64_t *pweight_old,
                                int64_t n, int64_t k, int64_t *part, int64_t *pweight, void *stream);
int tsamd_partition_balance(const int64_t *pweight, int64_t k, int64_t cap, int64_t *balance, void *stream);

/* ------------------------------------------------------------------------ *
 * Reverse Cuthill-McKee ordering (csrc/rcm.hip).  Replaces the scipy call of reverse_cuthill_mckee
 * (torch_sparse/bandwidth.py:8-20: `sp.csgraph.reverse_cuthill_mckee(sp_src, symmetric_mode=True)` on the host) and
 * returns the same permutation bit for bit when seeded in scipy's order; docs/design/rcm.md has the scheme.  The
 * building blocks of the host driver (csrc/ops_rcm.cpp); n < 2^31.
 *
 *   tsamd_rcm_limits        out[0..2] = (largest node capacity of the one-workgroup route, its capacity in frontier
 *        entries, the levels one of its launches may run under tsamd::rcm).
 *   tsamd_rcm_degree        deg[i] = rowptr[i + 1] - rowptr[i], plus one where row i holds its own diagonal (scipy's
 *        degree; a repeated diagonal counts once).  Balanced by entries.
 *   tsamd_rcm_relabel       out[i] = table[idx[i]]; an id outside [0, n) gives 0 and state[7] = max(state[7], 1).
 *   tsamd_rcm_begin         by_rank [n] = the nodes in stable (degree, id) order, seeds [n] = the order in which nodes are
 *        tried as component seeds -> rank (the inverse of by_rank), seeds_r[i] = rank[seeds[i]], pos = -1, owner = max.
 *        state[7] = 2 when seeds is not a permutation of [0, n).  scratch: n words.
 *   state (DEVICE int64[8], zeroed by the caller): [0] lo and [1] hi, the frontier is order[lo, hi); [2] the seed
 *        cursor; [3] why the last one-workgroup launch ended: 0 everything is ordered, 1 the frontier exceeds the
 *        route's capacity, 2 level budget, 3 seed-search budget; [4] levels (non-empty frontiers); [5] components;
 *        [6] entries of the frontier's rows (written by _level_plan); [7] input errors.
 *   tsamd_rcm_small         ONE workgroup on the RELABELLED graph (node = rank, rows sorted): runs levels -- claim by
 *        min, flag, scan, write -- and, when a frontier empties, takes the next unvisited node of seeds_r (isolated
 *        seeds in batches), until the frontier exceeds cap_nodes nodes (clamped to the limit; 0: seed search only) or the
 *        entry capacity, everything is ordered, or `budget` levels have run.  The caller reads state and relaunches.
 *        With state[7] != 0 (bad input) the launch returns at once with reason 0; no position >= n is ever written.
 *   tsamd_rcm_level_plan / _level_run      one level on the whole device, work divided by frontier ENTRIES: _plan
 *        scans the row lengths of the nf = hi - lo frontier nodes into fptr [nf + 1] and state[6] = T; the caller reads
 *        T; _run(T, n) claims, flags, scans and writes (ej, ep, off: T words each) and advances lo / hi / levels.
 *        Workspace of both: tsamd_rcm_level_workspace_bytes(count) with count = nf resp. T.
 *   tsamd_rcm_finish        perm[i] = by_rank[order[n - 1 - i]].
 * ------------------------------------------------------------------------ */
int tsamd_rcm_limits(int64_t out[3]);
int tsamd_rcm_degree(const int64_t *rowptr, const int64_t *col, int64_t n, int64_t E, int64_t *deg, void *stream);
int tsamd_rcm_relabel(const int64_t *idx, const int64_t *table, int64_t count, int64_t n, int64_t *out, int64_t *state,
                      void *stream);
int tsamd_rcm_begin(const int64_t *by_rank, const int64_t *seeds, int64_t n, int64_t *rank, int64_t *seeds_r,
                    int64_t *pos, int64_t *owner, int64_t *scratch, int64_t *state, void *stream);
int tsamd_rcm_small(const int64_t *rowptr, const int64_t *col, const int64_t *seeds_r, int64_t n, int64_t cap_nodes,
                    int64_t budget, int64_t *pos, int64_t *owner, int64_t *order, int64_t *state, void *stream);
size_t tsamd_rcm_level_workspace_bytes(int64_t count);
int tsamd_rcm_level_plan(const int64_t *rowptr, const int64_t *order, int64_t nf, int64_t *fptr, int64_t *state,
                         void *workspace, size_t workspace_bytes, void *stream);
int tsamd_rcm_level_run(const int64_t *rowptr, const int64_t *col, const int64_t *fptr, int64_t T, int64_t n, int64_t *pos,
                        int64_t *owner, int64_t *order, int64_t *ej, int64_t *ep, int64_t *off, int64_t *state,
                        void *workspace, size_t workspace_bytes, void *stream);
int tsamd_rcm_finish(const int64_t *order, const int64_t *by_rank, int64_t n, int64_t *perm, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* TSAMD_H_ */
