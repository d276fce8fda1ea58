/*
 * sgp_amd.h -- C ABI of libsgp_amd.so: the MI355X (gfx950) device side of SGP's
 * training-free spatiotemporal encoder.
 *
 * The reference (Graph-Machine-Learning-Group/sgp) is pure Python; the native work on its
 * hot path is done by third-party ops.  Each entry point below replaces one of
 * those call sites (paths relative to the reference repo root):
 *
 *   sgp_spmm_csr_f32 / sgp_spmm_tiled_f32
 *       lib/sgp_preprocessing.py:202   `x = adj @ x`
 *       (torch_sparse SparseTensor.__matmul__ -> spmm_sum(row,rowptr,col,value,colptr,csr2csc,mat))
 *   sgp_reservoir_f32
 *       lib/nn/reservoir/reservoir.py:77-81 (ReservoirLayer.forward: 2x F.linear, act, leak)
 *       driven by the Python time loop at lib/nn/reservoir/reservoir.py:170-183
 *   sgp_node_mean_bcast_f32
 *       lib/nn/encoders/sgp_spatial_encoder.py:32-34 (`ones_like(x) * x.mean(-2, keepdim=True)`)
 *   sgp_copy_rows_f32
 *       lib/sgp_preprocessing.py:200,217 + sgp_spatial_encoder.py:35 (`torch.cat(out, -1)`) --
 *       only needed when a caller hands over a tensor that is not already in the
 *       output slot; the fused path writes slots in place and never concatenates.
 *   sgp_gather_rows_f32
 *       lib/datasets/iid_dataset.py:57-99 (IID (t, n) row gather of the embedding; "next" row f1)
 *   sgp_pack_rows_16, sgp_gather_rows_16
 *       the same embedding kept in bf16 / fp16 (no counterpart in the reference: lib/utils.py:24-35 holds float32)
 *   sgp_window_gather
 *       tsl/data/spatiotemporal_dataset.py (window / horizon indexing of a sample) and
 *       lib/dataloader/subgraph_dataloader.py:31-34 (node slices of a batch), one launch per tensor and batch
 *   sgp_window_hop_f32
 *       lib/nn/models/sgp_online.py:55-61 (rearrange 'b t n f -> b n (t f)', sgp_spatial_embedding, torch.cat)
 *   sgp_grouped_linear_f32
 *       lib/nn/models/sgp_model.py:41-52 (decoder input encoder: grouped Conv1d + activation; f4)
 *   sgp_grouped_linear_fwd_16, sgp_grouped_linear_wgrad_16
 *       the same layer, forward and weight gradient, reading the bf16 / fp16 embedding in place
 *
 * Conventions
 *   - All pointers are DEVICE pointers owned by the caller (e.g. the PyTorch
 *     allocator) unless stated otherwise; nothing is allocated inside.
 *   - Strides are in ELEMENTS (floats), not bytes.
 *   - Kernels are enqueued asynchronously on `stream` (a hipStream_t passed as
 *     void*; NULL = the default stream).
 *   - Every function returns 0 on success, a negative SGP_E* code on a bad
 *     argument, or a positive hipError_t if the runtime refused the launch.
 *     Nothing throws.  sgp_last_error() returns a thread-local description.
 */
#ifndef SGP_AMD_H
#define SGP_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 4: decoder_mlp.hip's one-workgroup MaskedMAE pair (forward, backward) removed; MaskedMAE is kind 0 of
 * sgp_masked_loss_f32 / _bwd_f32.
 * 3 (round 6): the launch predicate became the explicit trailing (pred, run_if) pair of every sgp_spmm_*_f32 entry
 * (sgp_launch_predicate removed); host-side planner sgp_split_plan_deal / sgp_split_plan_fill, the time-piece
 * reservoir entry sgp_reservoir_pieces_f32 and the wide split hop sgp_spmm_split_wide_f32 added.
 * 2 (round 5): sgp_spmm_split_f32 takes per-column scale tables and a per-row plan array; sgp_col_stats_f32,
 * sgp_split_prepare_f32, sgp_launch_predicate added; round 4 had already removed sgp_spmm_mfma / pipe / blk_*, widened
 * sgp_spmm_colblock_f32 by the halo arguments and grown sgp_reservoir_workspace_bytes (bf16-piece fragments). */
/* (within 3: sgp_spmm_split_banded_f32 / _wide_banded_f32 and sgp_split_plan_bands were added, and the two planner
 * entries sgp_split_plan_deal / _fill gained `nnz` behind `col` -- their only caller is sgp_amd/splitplan.py) */
#define SGP_ABI_VERSION 4

#define SGP_EINVAL   (-1)  /* bad size / null pointer / misaligned stride */
#define SGP_EUNSUP   (-2)  /* shape outside what the kernels are built for */
#define SGP_ENOMEM   (-3)  /* a host-side planner ran out of memory */

/* activations of lib/nn/reservoir/reservoir.py:37-41 */
#define SGP_ACT_TANH      0
#define SGP_ACT_RELU      1
#define SGP_ACT_SELF_NORM 2
#define SGP_ACT_IDENTITY  3
/* tanh evaluated with RELATIVE accuracy (an odd polynomial below |x| = 0.25; SGP_ACT_TANH is accurate to 3e-7 absolute,
 * 6 instead of 14 instructions per value): for layers whose bias and input scaling are so small that their states are
 * far below 1 -- sgp_amd's Python layer selects it when max |bias| < 0.25 */
#define SGP_ACT_TANH_REL  4

typedef void* sgp_stream_t;

int sgp_abi_version(void);
const char* sgp_last_error(void);
/* Name of the gfx target the device code was compiled for ("gfx950"). */
const char* sgp_build_arch(void);

/* The library's view of the ONE debug / tuning hook, the environment variable SGP_TUNE = "key=value,key=value"
 * (keys: sgp_amd/tune.py): the integer value of `key`, `dflt` when the variable or the key is absent.  Most keys
 * are read once per process by the kernel launchers; this entry parses the variable anew on every call. */
int64_t sgp_tune_value(const char* key, int64_t dflt);

/* ------------------------------------------------------------------ SpMM ---
 * Y[b, i, 0:feat] = sum_{e in [rowptr[i], rowptr[i+1])} val[e] * X[b, col[e], 0:feat]
 * for b in [0, batch), i in [0, n_rows).  X and Y may alias the same
 * allocation as long as the [feat]-wide column ranges do not overlap
 * (hop k reads slot k-1 and writes slot k of the [T, N, D_out] output).
 *
 * Columns >= n_own (when X_halo != NULL) are read from the halo buffer:
 *   X_halo[b, col - n_own, :]   (rows received from peer GPUs between hops)
 * Pass X_halo = NULL, n_own = n_cols for the single-GPU case.
 */
int sgp_spmm_csr_f32(const int32_t* rowptr, const int32_t* col, const float* val,
                     const float* X, int64_t x_row_stride, int64_t x_batch_stride,
                     const float* X_halo, int64_t xh_row_stride, int64_t xh_batch_stride,
                     int32_t n_own,
                     float* Y, int64_t y_row_stride, int64_t y_batch_stride,
                     int32_t n_rows, int32_t n_cols, int32_t batch, int32_t feat,
                     const int32_t* pred, int32_t run_if, sgp_stream_t stream);

/* LDS-staged variant for graphs with locality.  Rows are grouped into tiles of at most
 * `tile_rows` consecutive rows (tile k = rows tile_row_ptr[k] .. tile_row_ptr[k+1]); for
 * tile k the host supplies the sorted list of distinct source rows it references
 * (ucol[uptr[k] .. uptr[k+1])) and every edge carries the index of its column inside
 * that list.  Edge lists are padded per row to a multiple of 16 with (lcol = 0, val = 0):
 *   erow[i] .. erow[i+1]  = padded edge range of row i (multiple of 16 long)
 *   ecol[e] (uint16)      = index into the tile's ucol list
 *   eval[e]               = weight
 * max_union = largest per-tile list length, max_row_edges = largest padded per-row
 * edge count (host-side facts about the plan; they select the kernel variant).
 * Tiles of more than 128 rows (up to sgp_spmm_tiled_max_tile_rows() = 384; rows with at most 32
 * edges) take the tall form: the edge records live in LDS behind the stage, which must then hold
 * ceil(max_union / 64) * 16 KiB + 6 bytes per padded edge slot of 256 / 384 rows within 160 KiB
 * (small sparse graphs as ONE tile: every source row is staged once per step).
 * Returns SGP_EUNSUP if the plan exceeds the limits reported below.
 */
int sgp_spmm_tiled_f32(const int32_t* tile_row_ptr, const int32_t* uptr, const int32_t* ucol,
                       const int32_t* erow, const uint16_t* ecol, const float* eval,
                       int32_t tile_rows, int32_t n_tiles,
                       int32_t max_union, int32_t max_row_edges,
                       const float* X, int64_t x_row_stride, int64_t x_batch_stride,
                       const float* X_halo, int64_t xh_row_stride, int64_t xh_batch_stride,
                       int32_t n_own,
                       float* Y, int64_t y_row_stride, int64_t y_batch_stride,
                       int32_t n_rows, int32_t n_cols, int32_t batch, int32_t feat,
                       const int32_t* pred, int32_t run_if, sgp_stream_t stream);
/* Row-group kernel on the fp32 matrix cores, exact fp32 (lib/sgp_preprocessing.py:200-203, `x = adj @ x` per hop).
 * Tiles of at most 64 rows and their distinct-column lists as above; every tile is cut into 16 groups of 4
 * rows (slots 4g .. 4g+3 of the tile, see rowmap).  A group's sorted column union is dealt round-robin to 4
 * classes q; super-step s handles the s-th column of every class with one v_mfma_f32_4x4x1_16b_f32 per
 * feature.  The stream is stored 4 super-steps ("quad") at a time.  The tile's distinct-column list is cut
 * at usplit[k] (a multiple of 4) into segment A (list positions < usplit[k]) and segment B; a group's quads
 * are stored A-part first and never mix the segments: gptr[2 (16 k + g)] .. gptr[2 (16 k + g) + 1] = quads
 * on segment A, .. gptr[2 (16 k + g) + 2] = quads on segment B.  Per time step the kernel refills one
 * segment of the LDS stage by LDS-DMA (global_load_lds_dwordx4) while the matrix cores consume the other.
 *   gw  [quad][q][super-step s][row i]  float  weight of row i for class q's column in super-step s of the
 *                                        quad (0 = row lacks the column / padding); the MFMA of super-step s
 *                                        broadcasts block s of its class (cbsz = 2 / abid = s)
 *   gidx[quad][q][4]          int32   256 * index of that column in the tile's ucol list, i.e. the byte
 *                                     offset of its staged row in LDS (0 = padding)
 *   gsup[2 (16 k + g) + s]    int32   ceil(columns of that range / 4): the padding of a range's last quad is
 *                                     skipped in units of one super-step
 *   rowmap[64 * k + 4 g + i]  int32   output row of slot i of group g of tile k, -1 = empty (the host may
 *                                     permute rows inside a tile so that the 4 rows of a group share columns)
 * uptr / ucol list segment A first (padded to a multiple of 4 entries), then segment B.  A group's weights
 * and the per-lane LDS addresses of its staged rows are loaded once per workgroup into VGPRs, so a super-step
 * is one ds_read_b128 + 4 MFMAs with no VALU address arithmetic and no stream reads from LDS (ranges longer
 * than the resident super-steps continue from an LDS copy of the stream).  Limits: sgp_spmm_res_max_union()
 * staged rows and sgp_spmm_res_max_quads() quads per tile.  sgp_spmm_res_tune(cfg): 0 = 16 waves x 1 group
 * per workgroup, 1 = 8 waves x 2 groups (process-wide).
 * (Round 4 retired this kernel's predecessors sgp_spmm_mfma_f32 / sgp_spmm_pipe_f32 and the row-block form
 * sgp_spmm_blk_f32 -- superseded on every measured workload; their sources are kept under tools/experiments/.) */
int sgp_spmm_res_f32(const int32_t* uptr, const int32_t* ucol, const int32_t* usplit,
                     const int32_t* gptr, const int32_t* gsup, const int32_t* gidx, const float* gw,
                     const int32_t* rowmap,
                     int32_t n_tiles, int32_t max_union, int32_t max_tile_quads,
                     const float* X, int64_t x_row_stride, int64_t x_batch_stride,
                     const float* X_halo, int64_t xh_row_stride, int64_t xh_batch_stride,
                     int32_t n_own,
                     float* Y, int64_t y_row_stride, int64_t y_batch_stride,
                     int32_t n_rows, int32_t n_cols, int32_t batch, int32_t feat,
                     const int32_t* pred, int32_t run_if, sgp_stream_t stream);
int32_t sgp_spmm_res_max_union(void);
int32_t sgp_spmm_res_max_quads(void);
int sgp_spmm_res_tune(int32_t cfg);

/* Mixed dense / sparse form of the row-group product (lib/sgp_preprocessing.py:200-203, `x = adj @ x`
 * per hop; plan: sgp_amd/mixplan.py).  Tiles, staged rows, two-phase LDS-DMA staging and the
 * 4-row-group stream (uptr .. rowmap, gptr .. gw) are those of sgp_spmm_res_f32, but the 16 groups of
 * a tile form 4 blocks of 16 rows (tile slot = 16 block + 4 group + row), and the columns shared by
 * (nearly) all groups of a block are taken out of the group streams and multiplied by
 * v_mfma_f32_16x16x4_f32 instead (16 rows x 4 columns x 16 features per instruction):
 *   dptr[2 * 4 * n_tiles + 1]   first dense instruction of (tile, block, segment)
 *   didx[n_dense][4]            LDS byte offsets (staged row * 256) of the instruction's 4 columns
 *   dw[n_dense][64]             its A operand in lane order: lane 16 k + i = weight of (row i of the
 *                               block, column k), 0 where the row does not use the column
 * max_dense = longest (block, segment) list, at most sgp_spmm_mix_max_dense(halo != 0) (the lists
 * live in registers).  Wave w of a workgroup owns sparse group w and the dense part of block w / 4
 * for the feature quarter w % 4; dense sums reach the storing wave through a 16 KB LDS slab.
 * Arithmetic: exact fp32 FMAs; a row's sum is (sparse part, k order of its group stream) + (dense
 * part, k order of the block's list) -- another summation order than sgp_spmm_res_f32, same values
 * to rounding.  X / X_halo / Y as in sgp_spmm_tiled_f32. */
int sgp_spmm_mix_f32(const int32_t* uptr, const int32_t* ucol, const int32_t* usplit,
                     const int32_t* gptr, const int32_t* gsup, const int32_t* gidx, const float* gw,
                     const int32_t* rowmap,
                     const int32_t* dptr, const int32_t* didx, const float* dw,
                     int32_t n_tiles, int32_t max_union, int32_t max_dense,
                     const float* X, int64_t x_row_stride, int64_t x_batch_stride,
                     const float* X_halo, int64_t xh_row_stride, int64_t xh_batch_stride,
                     int32_t n_own,
                     float* Y, int64_t y_row_stride, int64_t y_batch_stride,
                     int32_t n_rows, int32_t n_cols, int32_t batch, int32_t feat,
                     const int32_t* pred, int32_t run_if, sgp_stream_t stream);
int32_t sgp_spmm_mix_max_union(void);
int32_t sgp_spmm_mix_max_dense(int32_t halo);

/* out[0] = max |X| over a strided [batch, n_rows, feat] view (device scalar; non-finite inputs give a
 * non-finite value).  Serves callers of sgp_spmm_split_f32 that have no analytic bound on their operand
 * (`sgp_spatial_embedding` on arbitrary [B, N, F] batches, lib/nn/models/sgp_model.py:169-181; relu
 * reservoirs).  Widths that are multiples of 4 need 16-byte aligned rows. */
int sgp_abs_max_f32(const float* X, int64_t x_row_stride, int64_t x_batch_stride,
                    int32_t n_rows, int32_t batch, int32_t feat, float* out, sgp_stream_t stream);

/* Launch predicate of the hop entries (the trailing `pred, run_if` pair of every sgp_spmm_*_f32): with pred != NULL (a
 * DEVICE word) the launch runs only if *pred == run_if when its kernel starts on the stream, and is a no-op otherwise
 * (every workgroup exits at its first instruction).  This is how a hop chooses between the split-fp16 kernel and the
 * exact-fp32 kernels ON THE DEVICE: sgp_split_prepare_f32 writes the flag, the caller enqueues sgp_spmm_split_f32 with
 * run_if = 1 and its exact kernel with run_if = 0 behind it (no host round trip, legal under stream capture).
 * pred = NULL: unconditional.  (ABI 2 carried this as thread-local state set by sgp_launch_predicate(); ABI 3 made it
 * an argument so that nothing armed by one call can reach another.) */

/* Per-column statistics of a strided [batch, n_rows, feat] view over the steps 0, t_stride, 2 t_stride, ... and the rows
 * 0, r_stride, 2 r_stride, ...: stats[0 : feat] = max |x[:, c]| (bit pattern of the float; NaN / inf win),
 * stats[feat : 2 feat] = sum of squares.  accumulate = 0 clears stats first; 1 adds a second source (the halo rows of
 * a node partition) to it.  feat % 4 == 0, feat <= 1024, 16-byte aligned rows. */
int sgp_col_stats_f32(const float* X, int64_t x_row_stride, int64_t x_batch_stride,
                      int32_t n_rows, int32_t batch, int32_t feat, int32_t t_stride, int32_t r_stride, int32_t accumulate,
                      float* stats, sgp_stream_t stream);

/* Scales, next bound and admission flag of the split-fp16 hop, on the device.  Per column c the bound B_c >= max
 * |x[:, c]| is bound_in[c] (device) if given, else bound_scalar if > 0, else the measured maximum (needs full = 1:
 * statistics over EVERY row).  An a-priori bound is never replaced by a measurement: the scales of a bounded operand
 * do not depend on how the caller cuts the time axis (bit-identical results per time chunk).  x_tab[c] = 2^e with
 * B_c 2^e in [2^13, 2^14] (B_c = 0: scale 1, the column is identically zero), x_tab[feat + c] = 2^-e,
 * bound_out[c] = B_c * norm_inf * (1 + 1e-6) (the bound of A x for ||A||_inf = norm_inf; may be NULL).
 * flag[0] = 1 iff every bound is finite, covers the sampled data, and -- when statistics are given -- satisfies
 *     B_c * sqrt(s_eff) <= 2^16 * sqrt(ssq_c / n_samples)           for every column with B_c > 0
 * (n_samples = rows behind the sums, s_eff = rows of the operand / rows sampled >= 1: a strided sample overstates a
 * mean square by at most that factor).  Why: the split kernel represents |x| >= 2^-16 B_c to 2^-23 relative and
 * everything smaller to 2^-38 B_c ABSOLUTE; the test keeps that absolute term below 2^-22 of the column's RMS,
 * i.e. at fp32's own level.  stats = NULL: no test, the caller vouches for the bound (flag = bounds finite). */
int sgp_split_prepare_f32(const float* stats, double n_samples, double s_eff, int32_t full,
                          const float* bound_in, float bound_scalar, float norm_inf, int32_t feat,
                          float* x_tab, float* bound_out, int32_t* flag, sgp_stream_t stream);

/* Split-fp16 hop (lib/sgp_preprocessing.py:200-203, `x = adj @ x` per hop; plan: sgp_amd/splitplan.py;
 * kernel: csrc/spmm_split.hip).  Every operand value is carried as two fp16 pieces of its scaled self
 * (v * scale = hi + lo, 22 significant bits) and every product as hi*hi + hi*lo + lo*hi accumulated in fp32
 * by v_mfma_f32_16x16x32_f16, at 16x the fp32 matrix rate, which pays for dense 16 x 32 blocks of A and 256-row
 * tiles (3.2 staged source rows per result row instead of 5.8).
 * ERROR MODEL.  x is scaled per feature column (x_tab, from sgp_split_prepare_f32), A per row (plan), so the
 * result is invariant to rescaling a column of x or a row of A, like fp32.  Within 2^16 of its column's bound a
 * value keeps 22 bits (relative 2^-23); below that the error is absolute, <= 2^-38 x the column's bound.  The
 * products are exact, sums are fp32.  The kernel is therefore fp32-equivalent exactly where
 * sgp_split_prepare_f32 sets its flag, and callers launch it under that predicate with an exact kernel behind it.
 * Arrays:
 *   hdr[n_tiles][64]                         [W : 2 W] rows of each of the W waves, [2 W] staged rows U
 *   rowid[n_tiles][W][16]                    result row of every slot of every wave, -1 = empty
 *   ucol[n_tiles][max_union]                 source row staged at position s (-1 beyond U)
 *   afr[n_tiles][W][chunks][2][64][8] fp16   A fragments in lane order (piece 0 | 1) of a[i, :] * 2^e_i
 *   adr[n_tiles][W][chunks][64]              per-lane byte addresses of the two transpose reads, a0 | a1 << 16
 *   rinv[n_tiles][W][16]                     2^-e_i of every slot's row (0 for empty slots)
 * with W = sgp_spmm_split_waves() waves of sgp_spmm_split_rows_per_wave() = 16 rows, the k-slots of a chunk in any
 * order (the planner picks one that keeps the rows a transpose read fetches together on different LDS banks),
 * chunks = sgp_spmm_split_chunks(), max_union = sgp_spmm_split_max_union().  feat % 16 == 0, feat <=
 * sgp_spmm_split_max_feat().  X / X_halo / n_own as in sgp_spmm_tiled_f32 (columns >= n_own address the halo rows
 * a node partition received).  x_tab: device [2][feat], scale then inverse, |x[:, c]| * x_tab[c] < 65504.
 * NON-FINITE OPERANDS.  The kernel multiplies dense 16 x 32 blocks: padded and zero entries form 0 * x, so a NaN /
 * inf in a source row (or a value that overflows fp16 after scaling: |x| above its column's bound by 4x) reaches EVERY
 * result row of every wave that stages that row, not only the row's graph neighbours as in a sparse fp32 product.
 * sgp_split_prepare_f32's admission test sees non-finite values only in the rows and steps its statistics read: all of
 * them when the bound is measured (full = 1), a sample (~8 steps, every r-th row, plus every row of the last step -- where
 * a value that entered a recurrence earlier still is) when the caller supplies an a-priori bound.  A caller that passes a bound therefore vouches for finiteness and for the bound on the unsampled part
 * (sgp_amd's encoders pass one only for states their own bounded-activation reservoir kernels wrote).
 * accumulate != 0: Y += A X (the later passes of an operator whose rows were cut into column segments).
 * t_chunk = time steps per workgroup (0 = chosen here). */
int sgp_spmm_split_f32(const int32_t* hdr, const int32_t* rowid, const int32_t* ucol, const void* afr,
                       const int32_t* adr, const float* rinv, int32_t n_tiles,
                       const float* X, int64_t x_row_stride, int64_t x_batch_stride,
                       const float* X_halo, int64_t xh_row_stride, int64_t xh_batch_stride, int32_t n_own,
                       float* Y, int64_t y_row_stride, int64_t y_batch_stride,
                       int32_t n_rows, int32_t n_cols, int32_t batch, int32_t feat,
                       const float* x_tab, int32_t accumulate, int32_t t_chunk, const int32_t* pred, int32_t run_if, sgp_stream_t stream);
int32_t sgp_spmm_split_chunks(void);
int32_t sgp_spmm_split_max_union(void);
int32_t sgp_spmm_split_waves(void);
int32_t sgp_spmm_split_rows_per_wave(void);
int32_t sgp_spmm_split_max_feat(void);

/* The same hop with the caller's choice of WALK, the mapping from workgroup to (tile, time chunk) -- the arithmetic of
 * a result element does not depend on it, so every walk gives the same bits.  walk = 0: chosen here, exactly
 * sgp_spmm_split_f32; 1: tile-major (an XCD walks its own tiles over all time); 2: time-major (an XCD walks ITS time
 * chunks, chunk % 8 == xcd, over all tiles: operators whose source rows of one step fit an L2); 3: BANDED time-major
 * (DESIGN 4.2e): band_first[n_bands + 1] (DEVICE memory; strictly increasing tile indices from 0 to n_tiles, made by
 * sgp_split_plan_bands) cuts the plan's tile list into bands of consecutive tiles whose distinct staged rows of one step
 * fit an L2; inside a band the XCDs walk time-major over the band's tiles, the bands follow each other in workgroup
 * order inside the one launch, in workgroups of at most 32 steps unless t_chunk names a length.  band_first is read for
 * walk = 3 only. */
int sgp_spmm_split_banded_f32(const int32_t* hdr, const int32_t* rowid, const int32_t* ucol, const void* afr,
                              const int32_t* adr, const float* rinv, int32_t n_tiles,
                              const float* X, int64_t x_row_stride, int64_t x_batch_stride,
                              const float* X_halo, int64_t xh_row_stride, int64_t xh_batch_stride, int32_t n_own,
                              float* Y, int64_t y_row_stride, int64_t y_batch_stride,
                              int32_t n_rows, int32_t n_cols, int32_t batch, int32_t feat,
                              const float* x_tab, int32_t accumulate, int32_t t_chunk,
                              int32_t walk, const int32_t* band_first, int32_t n_bands,
                              const int32_t* pred, int32_t run_if, sgp_stream_t stream);

/* The same kernel in its WIDE form (csrc/spmm_split_wide.hip): 8 waves x 16 rows x 14 chunks -- 448 columns per wave, two
 * waves per SIMD.  For operators whose rows exceed the standard form's 224 columns (the reference's full large-scale
 * graphs, config/largescale/sgp_pv.yaml / sgp_cer.yaml with experiments/run_largescale_sgp.py:167-170: ~740 / ~495
 * entries per row): half as many accumulating passes and less than half the staged rows per result row.  Same arguments,
 * array formats and error model as sgp_spmm_split_f32, with W = sgp_spmm_split_wide_waves(), chunks =
 * sgp_spmm_split_wide_chunks(), max_union = sgp_spmm_split_wide_max_union(). */
int sgp_spmm_split_wide_f32(const int32_t* hdr, const int32_t* rowid, const int32_t* ucol, const void* afr,
                            const int32_t* adr, const float* rinv, int32_t n_tiles,
                            const float* X, int64_t x_row_stride, int64_t x_batch_stride,
                            const float* X_halo, int64_t xh_row_stride, int64_t xh_batch_stride, int32_t n_own,
                            float* Y, int64_t y_row_stride, int64_t y_batch_stride,
                            int32_t n_rows, int32_t n_cols, int32_t batch, int32_t feat,
                            const float* x_tab, int32_t accumulate, int32_t t_chunk, const int32_t* pred, int32_t run_if, sgp_stream_t stream);
int sgp_spmm_split_wide_banded_f32(const int32_t* hdr, const int32_t* rowid, const int32_t* ucol, const void* afr,
                                   const int32_t* adr, const float* rinv, int32_t n_tiles,
                                   const float* X, int64_t x_row_stride, int64_t x_batch_stride,
                                   const float* X_halo, int64_t xh_row_stride, int64_t xh_batch_stride, int32_t n_own,
                                   float* Y, int64_t y_row_stride, int64_t y_batch_stride,
                                   int32_t n_rows, int32_t n_cols, int32_t batch, int32_t feat,
                                   const float* x_tab, int32_t accumulate, int32_t t_chunk,
                                   int32_t walk, const int32_t* band_first, int32_t n_bands,
                                   const int32_t* pred, int32_t run_if, sgp_stream_t stream);
int32_t sgp_spmm_split_wide_chunks(void);
int32_t sgp_spmm_split_wide_max_union(void);
int32_t sgp_spmm_split_wide_waves(void);
int32_t sgp_spmm_split_wide_rows_per_wave(void);
int32_t sgp_spmm_split_wide_max_feat(void);

/* Host-side planner of sgp_spmm_split_f32 (csrc/plan_split.hip; HOST pointers, no GPU needed; the encoder builds the
 * plan once per graph in front of `x = adj @ x`, lib/sgp_preprocessing.py:188-203).
 * sgp_split_plan_deal: rows -- in `order` (n_order entries) or 0 .. n_rows - 1 when order = NULL -- are dealt greedily to
 * waves of at most rows_per_wave rows touching at most 32 * chunks distinct columns, waves to tiles of at most `waves`
 * waves touching at most max_union distinct columns.  Writes wave_of_row / slot_of_row [n_rows] (-1 for rows outside
 * the order) and tile_of_wave / rows_of_wave (capacity n_rows); returns the number of waves, -2 when a single row
 * exceeds a wave's budget (no one-pass plan), -1 on a bad argument.
 * sgp_split_plan_fill: the kernel's arrays (formats: sgp_spmm_split_f32 above) for that deal, tiles in parallel on
 * `threads` host threads (0 = all); stats[8] = tiles, waves, rows per wave, rows per tile, staged rows per result row,
 * chunk fill, largest staged-row count, ||A||_inf.
 * sgp_split_plan_bands: cuts the tile list (ucol[n_tiles][max_union] of a filled plan, host memory) into bands of
 * consecutive tiles for sgp_spmm_split_banded_f32: a band closes when the next tile would take its distinct staged
 * rows over col_budget (a tile beyond the budget on its own is a band of one).  Writes band_first (capacity
 * n_tiles + 1): first tile of every band, then n_tiles; returns the number of bands.
 * sgp_split_plan_order: a dealing order for a SQUARE operator's rows (row ids = column ids) worked out from the graph
 * alone: tiles are grown from the lowest-numbered unplaced row by adding, among the unplaced rows the tile's staged
 * columns name, the one that brings the fewest new columns (ties: most columns already staged, then lowest number) until
 * max_union columns or waves * rows_per_wave rows are reached; the tile's rows are cut into waves of at most
 * rows_per_wave rows / 32 * chunks columns by the same rule, waves beyond `waves` go back to the unplaced rows.  Writes
 * the permutation order[n_rows] (tiles in the order of their seeds, so the sequence keeps the numbering's locality
 * for the banded walk); returns 0.  Single-threaded and deterministic.
 * All four check their CSR (rowptr[0] == 0, non-decreasing, rowptr[n_rows] <= nnz = the length of col / val) and
 * let no C++ exception out: SGP_EINVAL / SGP_ENOMEM instead. */
int sgp_split_plan_order(const int64_t* rowptr, const int64_t* col, int64_t nnz, int64_t n_rows, int64_t n_cols,
                         int32_t waves, int32_t chunks, int32_t max_union, int32_t rows_per_wave, int64_t* order);
int64_t sgp_split_plan_deal(const int64_t* rowptr, const int64_t* col, int64_t nnz, int64_t n_rows, int64_t n_cols,
                            const int64_t* order, int64_t n_order,
                            int32_t waves, int32_t chunks, int32_t max_union, int32_t rows_per_wave,
                            int64_t* wave_of_row, int64_t* slot_of_row, int64_t* tile_of_wave, int64_t* rows_of_wave);
int sgp_split_plan_fill(const int64_t* rowptr, const int64_t* col, const float* val, int64_t nnz, int64_t n_rows, int64_t n_cols,
                        const int64_t* wave_of_row, const int64_t* slot_of_row, const int64_t* tile_of_wave,
                        const int64_t* rows_of_wave, int64_t n_waves, int64_t n_tiles,
                        int32_t waves, int32_t chunks, int32_t max_union,
                        int32_t* hdr, int32_t* rowid, int32_t* ucol, void* afr, int32_t* adr, float* rinv,
                        double* stats, int32_t threads);
int64_t sgp_split_plan_bands(const int32_t* ucol, int64_t n_tiles, int32_t max_union, int64_t n_cols,
                             int64_t col_budget, int32_t* band_first);

/* Column-blocked hop for graphs without locality (lib/sgp_preprocessing.py:202, `x = adj @ x`; plan:
 * sgp_amd/colblock.py).  The columns are cut into n_blocks blocks of consecutive columns whose source
 * rows fit the L2 of an XCD; n_wg persistent workgroups (16 waves) each own a contiguous range of at
 * most sgp_spmm_colblock_rows_cap() rows for all time steps and sweep the blocks in the same order, so
 * every gather of a sweep is served by the L2; partial sums of a step stay in LDS.  Arrays:
 *   plan[n_entries][2]            {column | (row - wg_row0[wg]) << 23, weight bits}: the edges of a
 *                                 (workgroup, block) segment row by row, padded with weight-0 entries
 *                                 to a multiple of 64 * sgp_spmm_colblock_round_pad()
 *   segptr[n_wg * n_blocks + 1]   first ROUND (64 entries) of segment (wg, block)
 *   wg_row0[n_wg + 1]             first row of every workgroup
 * feat must be a multiple of 64 (one launch dimension per 64 features), n_cols < 2^22.  X_halo / n_own as in
 * sgp_spmm_tiled_f32: columns >= n_own address the halo rows a node partition received (round 4).  The sums of a row meet through LDS float
 * atomics: their order, hence the last bits of a result, may differ between runs. */
int sgp_spmm_colblock_f32(const int32_t* plan, const int32_t* segptr, const int32_t* wg_row0,
                          int32_t n_wg, int32_t n_blocks,
                          const float* X, int64_t x_row_stride, int64_t x_batch_stride,
                          const float* X_halo, int64_t xh_row_stride, int64_t xh_batch_stride, int32_t n_own,
                          float* Y, int64_t y_row_stride, int64_t y_batch_stride,
                          int32_t n_rows, int32_t n_cols, int32_t batch, int32_t feat,
                          const int32_t* pred, int32_t run_if, sgp_stream_t stream);
int32_t sgp_spmm_colblock_rows_cap(void);
int32_t sgp_spmm_colblock_round_pad(void);

/* Limits of the tiled kernel: largest per-tile distinct-column count it can stage for
 * `feat` (0 = feat unsupported; feat must be a multiple of 64), largest tile height and
 * largest padded per-row edge count. */
int32_t sgp_spmm_tiled_max_union(int32_t feat);
int32_t sgp_spmm_tiled_max_tile_rows(void);
int32_t sgp_spmm_tiled_max_row_edges(void);

/* Which kernel form a launch takes -- host-only queries; the entries dispatch on these same answers.
 * sgp_spmm_tiled_form: rows per edge group (1, 2, or 4 / 6 for tall tiles) and 16-edge batches per row (1, 2, 8) of a
 * plan with the given tallest tile and largest padded per-row edge count (NULL outputs are skipped).  Returns 0, or
 * SGP_EUNSUP where sgp_spmm_tiled_f32 has no kernel: beyond the limits above, or 8 batches with more than one row per
 * group.
 * sgp_spmm_csr_form: lanes per source-row chunk of the generic rows kernel (4, 8, 16, 32, 64) for `feat`-wide operands,
 * or 0 = the scalar kernel (feat % 4 != 0, or aligned == 0: a stride that is no multiple of 4 floats / a pointer off a
 * 16-byte boundary).  predicated != 0 names the bounded-grid form of the same lane count. */
int sgp_spmm_tiled_form(int32_t tile_rows, int32_t max_row_edges, int32_t* rows_per_group, int32_t* batches);
int32_t sgp_spmm_csr_form(int32_t feat, int32_t aligned, int32_t predicated);

/* ------------------------------------------------------------- Reservoir ---
 * One leaky-ESN layer over the whole sequence (time loop on the device):
 *   h[t] = (1 - alpha) * h[t-1] + alpha * act(x[t] W_ih^T + b + h[t-1] W_hh^T)
 * x:   [T, N, F] with strides (x_step_stride, x_row_stride, 1)
 * out: [T, N, R] with strides (out_step_stride, out_row_stride, 1)
 * w_ih [R, F], w_hh [R, R], b [R]: row-major device arrays, exactly the
 *   reference's parameters (lib/nn/reservoir/reservoir.py:43-52).
 * h_state: optional [N, R] contiguous; if non-NULL it is the initial state and
 *   receives the final one (T-chunked streaming / resume); NULL = zeros.
 * workspace: device scratch of sgp_reservoir_workspace_bytes(F, R) bytes
 *   (weights re-laid out in MFMA fragment order); contents need not persist.
 * Multi-layer reservoirs (reservoir.py:174-176) are run layer by layer: layer
 * l > 0 reads layer l-1's slot of the output as its x.
 * Arithmetic: fp32 products on the fp32 matrix cores (v_mfma_f32_16x16x4_f32), fp32 accumulation.  Layers with
 * R = 32 or 64 and F = 16, 32 or 64, and large layers with R = 256 and F = 32, 64 or 128 (16-byte aligned rows)
 * take csrc/reservoir_bf3.h instead: every operand as
 * three bf16 pieces (24 bits, no scale, no bound on the values), six piece products per product on
 * v_mfma_f32_16x16x32_bf16, fp32 accumulation -- as close to the fp64 result as a CPU fp32 evaluation
 * (tests/test_gpu_reservoir_bf3.py); SGP_TUNE=res_bf3=0 keeps the fp32 matrix cores for them too.
 * Small problems (<= 512 tiles of 16 nodes, 32 < R <= 128, F <= 64: csrc/reservoir_splitj_bf3.h) form the same
 * three-piece products, except the RECURRENT ones under act = SGP_ACT_TANH: there the state lies in [-1, 1] (a convex
 * combination of the old state and a tanh) and is cut into two fp16 pieces of 2^14 h, row j of w_hh into two fp16
 * pieces under its own power-of-two scale (largest entry at 2^13 .. 2^14); hi hi + hi lo + lo hi on
 * v_mfma_f32_16x16x32_f16, fp32 accumulation, the row sum scaled back exactly.  Per operand: relative 2^-23 down to
 * 2^-16 of its bound (1 for the state, the row's largest |w|), absolute 2^-38 of the bound below -- far under the
 * 3e-7 absolute accuracy of SGP_ACT_TANH itself.  A workgroup (16 nodes) whose INITIAL h_state has an entry outside
 * [-1, 1] (or NaN) runs the three-piece loop instead, decided on the device; the other activations always do.
 * The large-N forms (R = 32 / 64 with F = 16 / 32 / 64; R = 256 with F = 32 / 64 / 128, >= 2048 node tiles) do the same under SGP_ACT_TANH (pack_weights_bf3h / pack_weights_sbf3h: the row scale
 * 2^(e_j + 14) is folded into the bias and the input fragments, so the accumulator carries it as a whole and is scaled
 * back once, exactly): launched alone when h_state is NULL; with an h_state, a test kernel writes "some entry lies outside
 * [-1, 1] or is NaN" into a device word and the two-piece instance runs under word == 0, the three-piece instance
 * under word == 1 behind it (whole launch; no host round trip).
 * All of this only for 0 <= alpha <= 1 (the leak is convex); any other leaking rate keeps three bf16 pieces.
 * SGP_TUNE=res_h16=0 keeps three bf16 pieces for the bounded state too.
 */
int64_t sgp_reservoir_workspace_bytes(int32_t F, int32_t R);
int sgp_reservoir_f32(const float* x, int64_t x_row_stride, int64_t x_step_stride,
                      const float* w_ih, const float* w_hh, const float* b,
                      double alpha, int32_t act,
                      float* out, int64_t out_row_stride, int64_t out_step_stride,
                      float* h_state, void* workspace,
                      int32_t T, int32_t N, int32_t F, int32_t R,
                      sgp_stream_t stream);

/* The same layer over n_pieces TIME PIECES side by side (small graphs: the sequential chain of
 * lib/nn/reservoir/reservoir.py:170-183 runs on ceil(N / 16) workgroups -- 21 of 256 CUs at N = 325 -- so the time axis
 * is the only parallelism left).  Workgroup (node tile, p) runs t_piece steps (the last piece: t_last <= t_piece) of
 *     x + p * x_piece_stride, out + p * out_piece_stride, h_state + p * N * R        (strides in floats)
 * from the state h_state[p] and leaves its final state there; no_store != 0 writes no output rows (a piece's WARM-UP:
 * started from zero some hundred steps early, a contractive recurrence arrives at the true state).  The recurrence
 * itself is not changed: what makes the pieces a valid evaluation of the sequence is the caller's comparison of every
 * piece's end state with its successor's warmed-up start (sgp_amd/nn/reservoir/reservoir.py::run_time_parallel, on the
 * device) and the sequential launch -- this entry with n_pieces = 1 under `pred` -- that repairs a rejected splice.
 * pred / run_if: launch predicate as on the hop entries.  Served by the split-J bf16-piece kernel only
 * (csrc/reservoir_splitj_bf3.h: 32 < R <= 128, F <= 64, <= 512 node tiles); anything else returns SGP_EUNSUP. */
int sgp_reservoir_pieces_f32(const float* x, int64_t x_row_stride, int64_t x_step_stride,
                             const float* w_ih, const float* w_hh, const float* b,
                             double alpha, int32_t act,
                             float* out, int64_t out_row_stride, int64_t out_step_stride,
                             float* h_state, void* workspace,
                             int32_t t_piece, int32_t t_last, int32_t n_pieces,
                             int64_t x_piece_stride, int64_t out_piece_stride, int32_t no_store,
                             int32_t N, int32_t F, int32_t R,
                             const int32_t* pred, int32_t run_if, sgp_stream_t stream);

/* Which kernels the two entries above launch for such a call, from the planner they run (plan_reservoir,
 * csrc/reservoir.hip); host only, no device pointers.  has_state / has_pred: h_state / pred would be non-NULL
 * (n_pieces = 1, no_store = 0, has_pred = 0: sgp_reservoir_f32); x_align / out_align: the pointers' address modulo 16.
 * Writes one JSON object per line into text, in launch order: {"kernel": name} for every weight pack and the
 * initial-state test, then per layer-kernel launch its name with template arguments, node range, grid (x, y), workgroup
 * size, dynamic LDS bytes, predicate (none / caller / state_inside / state_outside: the word "some initial state lies
 * outside [-1, 1]" == 0 / == 1) and lane (main / side).  A request the entries refuse returns their error. */
int sgp_reservoir_describe(int32_t F, int32_t R, int32_t N, int32_t T, int32_t act, double alpha, int32_t has_state,
                           int32_t n_pieces, int32_t no_store, int32_t has_pred,
                           int64_t x_row_stride, int64_t x_step_stride, int32_t x_align,
                           int64_t out_row_stride, int64_t out_step_stride, int32_t out_align,
                           char* text, int64_t capacity);

/* All L layers of a narrow stacked reservoir in ONE launch (lib/nn/reservoir/reservoir.py:170-180:
 * the reference steps every layer inside one time step, layer l consuming layer l-1's new state).
 * The layers are pipelined as a wavefront over the waves of a workgroup (layer l on step t while
 * layer l+1 is on step t-1, hand-off through LDS), layer inputs never travel through HBM.
 *   w_ih / w_hh / b / alpha: HOST arrays of length L; w_ih[l] ([R, F] for l = 0, else [R, R]),
 *        w_hh[l] ([R, R]), b[l] ([R]) are DEVICE pointers to the reference's parameters
 *        (reservoir.py:42-52), alpha[l] the layer's leaking rate (reservoir.py:109-123)
 *   out: [T, N, >= L*R] strides (out_step_stride, out_row_stride, 1); layer l fills columns
 *        l*R .. (l+1)*R-1 of every step (the layer-major order of reservoir.py:181-183)
 *   h_state: optional [L, N, R] contiguous, initial states in / final states out; NULL = zeros
 *   workspace: sgp_reservoir_fused_workspace_bytes(F, R, L) bytes of device scratch, 16-byte aligned
 * Built for F <= 64, R <= 64, 2 <= L <= 16 with all layers' weights in LDS
 * (sgp_reservoir_fused_supported); other shapes: SGP_EUNSUP, run sgp_reservoir_f32 per layer.
 * Same exact-fp32 MFMA products as sgp_reservoir_f32; deeper layers sum their input part in the
 * k order of the recurrent part, so results agree to rounding, not bitwise. */
int64_t sgp_reservoir_fused_workspace_bytes(int32_t F, int32_t R, int32_t L);
int32_t sgp_reservoir_fused_supported(int32_t F, int32_t R, int32_t L);
int sgp_reservoir_fused_f32(const float* x, int64_t x_row_stride, int64_t x_step_stride,
                            const float* const* w_ih, const float* const* w_hh, const float* const* b,
                            const double* alpha, int32_t act,
                            float* out, int64_t out_row_stride, int64_t out_step_stride,
                            float* h_state, void* workspace,
                            int32_t T, int32_t N, int32_t F, int32_t R, int32_t L,
                            sgp_stream_t stream);
/* Same, and the column sums of the produced states per node tile of 16:
 *   tile_sums[ceil(N / 16)][T][L*R] (contiguous, 16-byte aligned), entry (k, t, :) = sum over the
 *   nodes 16 k .. 16 k + 15 (< N) of out[t, node, :L*R].
 * The global_attr block of lib/nn/encoders/sgp_spatial_encoder.py:32-34 is the mean over nodes of
 * exactly this tensor: summing the tiles (sgp_node_mean_bcast_f32 with Y = NULL over the [T, tiles, D]
 * view) replaces a second pass over the whole block.  NULL = sgp_reservoir_fused_f32. */
int sgp_reservoir_fused_sums_f32(const float* x, int64_t x_row_stride, int64_t x_step_stride,
                                 const float* const* w_ih, const float* const* w_hh, const float* const* b,
                                 const double* alpha, int32_t act,
                                 float* out, int64_t out_row_stride, int64_t out_step_stride,
                                 float* h_state, void* workspace, float* tile_sums,
                                 int32_t T, int32_t N, int32_t F, int32_t R, int32_t L,
                                 sgp_stream_t stream);

/* Windowed reservoir, LAST STATE ONLY: the call shape of the echo-state baseline (lib/nn/models/esn_model.py:41-43:
 * maybe_cat_exog, then lib/nn/reservoir/reservoir.py:158-186 with return_last_state=True).  For M = B * N independent
 * sequences of S steps and L layers
 *     h_l[t] = (1 - a_l) h_l[t-1] + a_l act(W_ih,l x_l[t] + b_l + W_hh,l h_l[t-1]),  x_0[t] = [x[t] | u[t]],  x_l[t] = h_{l-1}[t]
 * only h_l[S-1] is written: out[(b * N + n) * out_row_stride + l * R + j] (the layer-major order of reservoir.py:181-183).
 *   x: element (b, t, n, k) at x[b * x_batch_stride + (start_b + t) * x_step_stride + n * x_node_stride + k], k < Fx
 *      (the reference's [b, s, n, f] batch is read where it lies; no `s (b n) f` copy)
 *   u: optional second source with its own strides: features Fx .. Fx + Fu - 1 of layer 0 (NULL with Fu = 0: none).
 *      Node stride 0 is the global exogenous series of maybe_cat_exog (tsl/nn/utils/utils.py:56-75, u [b, s, f]);
 *      no concatenated tensor is built.
 *   step_start: optional [B] int32, start_b above (NULL: 0).  With batch stride 0 the windows of a resident series
 *      [T, N, F] are read in place, for x and u alike; the caller keeps start_b + S <= T.
 *   w_ih / w_hh / b / alpha: HOST arrays of length L as for sgp_reservoir_fused_f32 (w_ih[0]: [R, Fx + Fu])
 *   h0: optional [L, M, R] contiguous initial states, read only; NULL = zeros (reservoir.py:162-164)
 *   workspace: sgp_reservoir_window_workspace_bytes(Fx + Fu, R, L, S, M) bytes, 16-byte aligned.  Its head is the
 *      weights in fragment order: packed != 0 says an earlier call with the same weights and (Fx + Fu, R, L) left them
 *      there and skips the packing (w_ih / w_hh / b may then be NULL).
 * sgp_reservoir_window_supported: 0 = outside the domain (Fx + Fu <= 256, R <= 256, L <= 8: SGP_EUNSUP, run the
 * sequence entries); 1 = all layers in ONE launch, every state in registers for the whole window, nothing of size
 * S * M * R in memory (always when L * R <= 256, and for any single layer); 2 = layer by layer with one [S, M, R]
 * intermediate in the workspace that layer l + 1 overwrites row by row with its own states (L > 1 with L * R > 256
 * beyond 24 register tiles of 16 features).
 * A wave owns 16 sequences; weights in LDS for R <= 64 while the pack fits it, else streamed from the packed buffer
 * through L2.  Any M, S >= 1,
 * every activation code, any alpha.  Arithmetic: exact fp32 products (v_mfma_f32_16x16x4_f32), fp32 accumulation. */
int32_t sgp_reservoir_window_supported(int32_t F, int32_t R, int32_t L);
int64_t sgp_reservoir_window_workspace_bytes(int32_t F, int32_t R, int32_t L, int32_t S, int64_t M);
int sgp_reservoir_window_f32(const float* x, int64_t x_batch_stride, int64_t x_step_stride, int64_t x_node_stride, int32_t Fx,
                             const float* u, int64_t u_batch_stride, int64_t u_step_stride, int64_t u_node_stride, int32_t Fu,
                             const int32_t* step_start,
                             const float* const* w_ih, const float* const* w_hh, const float* const* b,
                             const double* alpha, int32_t act,
                             const float* h0, float* out, int64_t out_row_stride,
                             void* workspace, int32_t packed,
                             int32_t B, int32_t N, int32_t S, int32_t R, int32_t L, sgp_stream_t stream);

/* --------------------------------------------------------------- DynGESN ---
 * The graph echo-state baseline (lib/nn/reservoir/graph_reservoir.py:85-93, stepped by
 * tsl/nn/blocks/encoders/gcrnn.py:67-93):
 *     h' = (1 - alpha) h + alpha * act( x W_ih^T + b + A_hat (h W_hh^T) )
 * sgp_gesn_f32 runs a whole sequence through all L layers (the _GraphRNN loop of gcrnn.py:67-93
 * with _cat_states_layers): two launches per (time step, layer), issued from C:
 *   x:   [T, N, F] strides (x_step_stride, x_row_stride, 1)
 *   out: [T, N, L*R] strides (out_step_stride, out_row_stride, 1); layer i fills columns
 *        i*R .. (i+1)*R-1 of every step
 *   w_ih / w_hh / b / alpha: HOST arrays of length L; w_ih[i] ([R, F] for i = 0, else [R, R]),
 *        w_hh[i] ([R, R]) and b[i] ([R]) are DEVICE pointers to the reference's parameters
 *        (graph_reservoir.py:44-52), alpha[i] the layer's leaking rate
 *   h_state: [L, N, R] contiguous, initial states in, final states out (zeros = cold start)
 *   workspace: sgp_gesn_workspace_bytes(N, R, L) bytes of device scratch, 16-byte aligned
 *   rowptr / col / val: the normalised operator in CSR, rows = targets (N rows)
 * Building blocks, also exported (one cell step = graph_reservoir.py:85-93):
 *   sgp_gemm_nt_f32      C[m, n] = sum_k A[m, k] W[n, k] (+ bias[n])   (F.linear; fp32 MFMA)
 *   sgp_gesn_update_f32  h_out[i, :] = (1 - alpha) h_in[i, :]
 *                                     + alpha * act(p[i, :] + sum_e val[e] z[col[e], :])
 *                        (torch_sparse matmul of :91 fused with activation and leak; also
 *                        writes the row into out_row[i * out_stride + 0:R], the step's slot of
 *                        the [T, N, L*R] embedding).  z, p, h_in, h_out: contiguous [N, R].
 */
int64_t sgp_gesn_workspace_bytes(int32_t N, int32_t R, int32_t L);
/* sgp_gesn_tune(persistent): 1 (default, also SGP_TUNE=gesn_persistent=1) lets sgp_gesn_f32 run the
 * sequence in ONE cooperative launch per 256 steps when the shape allows it (R % 16 == 0, R <= 384,
 * L <= 8, not R = 144 .. 256 with L > 1, the (layer, column group, row tile) items fit one workgroup per CU; csrc/gesn_persist.hip:
 * layers as a wavefront, weights in registers, one grid barrier per step); 0 = always two launches
 * per (step, layer); < 0 = query.  Returns the setting. */
int sgp_gesn_tune(int32_t persistent);
/* Two read-only queries on which path sgp_gesn_f32 takes (tests/gesn_forms.py).  Why the persistent kernel does not
 * serve a shape or a call: */
#define SGP_GESN_WHY_TUNE_OFF    1  /* sgp_gesn_tune(0) / SGP_TUNE=gesn_persistent=0 */
#define SGP_GESN_WHY_R_MOD_16    2  /* R is no multiple of 16 */
#define SGP_GESN_WHY_R_ABOVE_384 3
#define SGP_GESN_WHY_LAYERS      4  /* L > 8 */
#define SGP_GESN_WHY_ITEMS       5  /* more (layer, column group, row tile group) items than CUs at every LDS carve-up */
#define SGP_GESN_WHY_OUT_ALIGN   6  /* sgp_gesn_last_run only: `out` rows cannot take 16-byte stores */
#define SGP_GESN_WHY_SCRATCH     7  /* sgp_gesn_last_run only: this build of the kernel uses scratch memory */
#define SGP_GESN_WHY_LAUNCH      8  /* the runtime refused: the cooperative launch, or no device to plan for */
#define SGP_GESN_WHY_FORM_OFF    9  /* an instantiation that is switched off: R = 144 .. 256 with L > 1 (gesn_persist.hip) */
/* sgp_gesn_plan: what sgp_gesn_f32 does for [N nodes, R units, L layers] on a device of `cus` compute units (cus <= 0:
 * the current device's; with cus > 0 no device call is made), from the functions the launches themselves go through.
 * out[8] (int64):
 *   0: 1 = the persistent kernel serves the shape   1: else why not (SGP_GESN_WHY_*), 0 when served
 *   2: KSB of gesn_persistent<KSB> (2, 4, 6)   3: row tiles of 16 nodes per workgroup (1 .. 4)
 *   4: workgroups   5: dynamic LDS bytes                                  (2 .. 5: 0 when not served)
 *   6: NV of the stepwise gesn_update_kernel<NV> (1, 2, 4, 6, 8)
 *   7: 1 = the stepwise GEMM on the states takes its 16-byte (VEC) form, for a 16-byte aligned h_state
 * sgp_gesn_edge_cap: adjacency entries a workgroup of the persistent kernel keeps in LDS; a workgroup whose rows hold
 * more reads col / val from global memory.
 * sgp_gesn_last_run: what the last sgp_gesn_f32 call of this process did.  out[3] (int64): steps run by the persistent
 * kernel, steps run stepwise, and why (SGP_GESN_WHY_*) the persistent kernel did not serve the latter (0 if it served all). */
int sgp_gesn_plan(int32_t N, int32_t R, int32_t L, int32_t cus, int64_t* out);
int sgp_gesn_edge_cap(void);
int sgp_gesn_last_run(int64_t* out);
int sgp_gesn_f32(const int32_t* rowptr, const int32_t* col, const float* val,
                 const float* x, int64_t x_row_stride, int64_t x_step_stride,
                 const float* const* w_ih, const float* const* w_hh, const float* const* b,
                 const double* alpha, int32_t act,
                 float* out, int64_t out_row_stride, int64_t out_step_stride,
                 float* h_state, void* workspace,
                 int32_t T, int32_t N, int32_t F, int32_t R, int32_t L, sgp_stream_t stream);
int sgp_gemm_nt_f32(const float* A, int64_t lda, const float* W, int64_t ldw, const float* bias,
                    float* C, int64_t ldc, int32_t M, int32_t N, int32_t K, sgp_stream_t stream);
int sgp_gesn_update_f32(const int32_t* rowptr, const int32_t* col, const float* val,
                        const float* z, const float* p, const float* h_in,
                        double alpha, int32_t act,
                        float* h_out, float* out_row, int64_t out_stride,
                        int32_t n_nodes, int32_t R, sgp_stream_t stream);

/* ------------------------------------------------------------ Node mean ----
 * Y[b, i, 0:feat] = (1 / n_rows) * sum_j X[b, j, 0:feat]   for every i.
 * With partial != NULL the kernel instead writes the un-normalised column sums
 * to partial[b, 0:feat] (contiguous) and leaves Y alone (multi-GPU: all-reduce
 * the partial sums, then call sgp_bcast_rows_f32).
 */
int sgp_node_mean_bcast_f32(const float* X, int64_t x_row_stride, int64_t x_batch_stride,
                            float* Y, int64_t y_row_stride, int64_t y_batch_stride,
                            float* partial,
                            int32_t n_rows, int32_t batch, int32_t feat,
                            sgp_stream_t stream);
/* Y[b, i, 0:feat] = scale * src[b, 0:feat]  for i in [0, n_rows). */
int sgp_bcast_rows_f32(const float* src, float scale,
                       float* Y, int64_t y_row_stride, int64_t y_batch_stride,
                       int32_t n_rows, int32_t batch, int32_t feat,
                       sgp_stream_t stream);

/* --------------------------------------------------------- Copy / gather ---
 * Y[b, i, 0:feat] = X[b, i, 0:feat] (strided block copy into an output slot). */
int sgp_copy_rows_f32(const float* X, int64_t x_row_stride, int64_t x_batch_stride,
                      float* Y, int64_t y_row_stride, int64_t y_batch_stride,
                      int32_t n_rows, int32_t batch, int32_t feat,
                      sgp_stream_t stream);
/* out[k, 0:feat] = X[step[k], node[k], 0:feat]   (IID sampling of the embedding).
 * Also used to pack halo rows: step = NULL gathers node[k] for every b:
 *   out[b, k, :] = X[b, node[k], :]. */
int sgp_gather_rows_f32(const float* X, int64_t x_row_stride, int64_t x_batch_stride,
                        const int32_t* step, const int32_t* node, int32_t n_index,
                        float* out, int64_t out_row_stride, int64_t out_batch_stride,
                        int32_t batch, int32_t feat, sgp_stream_t stream);

/* ------------------------------------------------- 16-bit embedding store ---
 * embed_store.hip.  The encoders' product can be kept in 16 bits: packed after the hops have written
 * their fp32 slots, widened again by the samplers' gather.  Strides of a 16-bit view are in 16-bit ELEMENTS.
 *
 * sgp_pack_rows_16: Y[b, i, 0:feat] = X[b, i, 0:feat] rounded to nearest-even in format `fmt`, bit-equal to the IEEE
 * conversion (fp16: subnormals, underflow to signed zero, overflow to infinity; NaN stays NaN -- bf16 writes the quiet
 * NaN 0x7FC0).  overflow_count (optional, fp16 only, device int64, 8-byte aligned) is INCREMENTED by the number of
 * finite inputs that became infinite: summed per workgroup, at most one atomic per workgroup, exact.  It is ignored for
 * bf16, whose exponent range is fp32's.  feat % 8 == 0 with strides that are multiples of 8 and 16-byte aligned bases
 * takes two 16-byte loads and one 16-byte store per thread; everything else (any feat and stride, X on 4 and Y on 2
 * bytes) the element-wise kernel.  An empty shape returns 0 without a launch.
 *
 * sgp_gather_rows_16: sgp_gather_rows_f32 over a 16-bit source -- out[k, 0:feat] = X[step[k], node[k], 0:feat], or with
 * step = NULL out[b, k, :] = X[b, node[k], :]; out is fp32 and may be a slot of a wider buffer.  Widening is exact.
 * The same two paths as the pack entry. */
#define SGP_STORE_BF16 1
#define SGP_STORE_F16  2
int sgp_pack_rows_16(const float* X, int64_t x_row_stride, int64_t x_batch_stride,
                     int32_t batch, int32_t n_rows, int32_t feat, int32_t fmt,
                     void* Y, int64_t y_row_stride, int64_t y_batch_stride,
                     int64_t* overflow_count, sgp_stream_t stream);
int sgp_gather_rows_16(const void* X, int64_t x_row_stride, int64_t x_batch_stride,
                       const int32_t* step, const int32_t* node, int32_t n_index, int32_t fmt,
                       float* out, int64_t out_row_stride, int64_t out_batch_stride,
                       int32_t batch, int32_t feat, sgp_stream_t stream);

/* ------------------------------------------------- Window gather of the data module ---
 * window_gather.hip.  Replaces tsl/data/spatiotemporal_dataset.py's window / horizon indexing of a
 * sample (one fancy index per item and tensor, then a collate) and lib/dataloader/subgraph_dataloader.py:31-34 (the
 * node slice of inputs, targets and mask): ONE launch builds one registered tensor of a whole batch,
 *
 *   out[b, j, k, 0:feat] = T( X[start[b] + offset + lag * j, node(b, k), 0:feat] ),   b < batch, j < count, k < n_out.
 *
 * X: a resident [n_steps, n_nodes, feat] series, fp32 (src_fmt 0) or SGP_STORE_BF16 / SGP_STORE_F16 (widened
 * exactly), unit feature stride, step and node strides in ELEMENTS (a slot of a wider buffer is a legal source).  A
 * "t f" tensor is n_nodes = 1, node = NULL.  start: DEVICE int32 [batch].  (offset, count, lag) is (0, window, 1) for
 * inputs and (window + delay, len(range(0, horizon, horizon_lag)), horizon_lag) for targets and the mask.
 * node: NULL (all nodes, n_out = n_nodes), int32 [n_out] shared by the batch (node_batch_stride 0) or int32
 * [batch, n_out] (node_batch_stride n_out).  out: contiguous [batch, count, n_out, feat], fp32, or bool bytes under
 * SGP_WINDOW_MASK.
 *
 * T (mode): SGP_WINDOW_IDENTITY; SGP_WINDOW_SCALE, (x - bias) / scale + 5e-8 in the operations and order of
 * sgp_scaler_apply_f32 (bit-equal to gather-then-transform), bias / scale device fp32 [param_nodes, param_feat] with
 * param_nodes in {1, n_nodes}, param_feat in {1, feat}, indexed by the GLOBAL node id; SGP_WINDOW_MASK, x != 0.
 *
 * Bounds are judged in the kernel before any access: a start whose first or last row
 * (start + offset + lag * (count - 1)) lies outside [0, n_steps) sets SGP_WINDOW_ERR_START in the caller's device word
 * *err (an atomic or; the caller zeroes and reads it), a node id outside [0, n_nodes) sets SGP_WINDOW_ERR_NODE; the
 * rows concerned are written as zeros and nothing is read out of range.
 * feat % 4 == 0 (fp32) or feat % 8 == 0 (16-bit) with 16-byte aligned X and out and strides that are such multiples
 * moves 16 source bytes per lane; everything else runs element-wise with the lanes along the nodes.  An empty shape
 * returns 0 without a launch; a null pointer or a negative size is SGP_EINVAL. */
#define SGP_WINDOW_IDENTITY 0
#define SGP_WINDOW_SCALE    1
#define SGP_WINDOW_MASK     2
#define SGP_WINDOW_ERR_START 1
#define SGP_WINDOW_ERR_NODE  2
int sgp_window_gather(const void* X, int32_t src_fmt, int64_t x_step_stride, int64_t x_node_stride,
                      int32_t n_steps, int32_t n_nodes, int32_t feat,
                      const int32_t* start, int32_t batch, int32_t offset, int32_t count, int32_t lag,
                      const int32_t* node, int32_t n_out, int64_t node_batch_stride,
                      int32_t mode, const float* bias, const float* scale, int32_t param_nodes, int32_t param_feat,
                      void* out, int32_t* err, sgp_stream_t stream);

/* ------------------------------------------------- Window hops of SGPOnlineModel ---
 * window_hops.hip.  Replaces lib/nn/models/sgp_online.py:55-61: rearrange(x, 'b t n f -> b n (t f)'),
 * sgp_spatial_embedding (k hops forward, k hops backward) and torch.cat(x, -1).  ONE launch is one hop of one direction
 * for the whole batch over a CSR operator (int32 rowptr / col, fp32 val; indices are trusted), into block dst_block of
 *
 *   out[b, i, n_blocks * W],  W = steps * feat,  block j = columns j W .. (j + 1) W - 1,  contiguous.
 *
 * Source: src_block < 0 reads the raw window where it lies, element (b, t, c, k) at
 * x[b * x_batch_stride + t * x_step_stride + c * x_node_stride + k] (strides in floats, k stride 1), as column
 * t * feat + k of node c; src_block >= 0 reads that block of `out` (x is not read).  write_block0 != 0 (window source
 * only) also writes block 0, the flattened window, for the launch's own rows.  rowptr == NULL with write_block0 writes
 * block 0 alone (k = 0).
 *
 * Every output element is accumulated in fp32 in the order the generic CSR kernel takes for a W-wide slot of an
 * aligned buffer (sgp_spmm_csr_form(W, 1, 0) lanes per row chunk for W % 4 == 0, one chain in CSR order otherwise), so
 * the result is bit-equal to sgp_copy_rows_f32 + sgp_spmm_csr_f32 on the flattened window.  Rows without entries are
 * written as zeros.  For W % 4 == 0 `out` has to be 16-byte aligned.
 *
 * form: 0 = the one sgp_window_hop_form names; SGP_WINDOW_HOP_DIRECT gathers the source per element / per 16 bytes
 * from memory; SGP_WINDOW_HOP_PLANES (window source, steps > 1, n * feat <= 16384) stages the [n, feat] planes of one
 * step for up to 4 batch items in LDS and gathers there.  Asking for PLANES outside its domain is SGP_EUNSUP.  An empty
 * shape returns 0 without a launch.
 *
 * sgp_window_hop_plan (host only) answers with the function the entry launches from what a launch of that shape and
 * `form` does, as out[0..9]: the form taken; the kernel (0 = window_hop_rows, 1 = window_hop_scalar, 2 =
 * window_hop_planes); its lanes (lanes per row chunk for rows, lanes per row for planes, 0 for scalar); grid x, y, z;
 * the batch items of one workgroup (4 for rows, 256 / W clamped to 1 .. batch for scalar, the staged planes' count for
 * planes); rows per workgroup and trips of its row loop (planes; otherwise 0 and 1); dynamic LDS bytes.  It refuses
 * with the entry's codes what the entry refuses from these arguments: a bad size, a window too wide, an unknown form,
 * PLANES outside its domain, a grid y or z above 65535.  An empty shape gives a grid of 0 x 0 x 0. */
#define SGP_WINDOW_HOP_DIRECT 1
#define SGP_WINDOW_HOP_PLANES 2
int32_t sgp_window_hop_form(int32_t from_window, int32_t has_operator, int32_t steps, int32_t n, int32_t feat);
int sgp_window_hop_plan(int32_t from_window, int32_t has_operator, int32_t batch, int32_t steps, int32_t n,
                        int32_t feat, int32_t form, int64_t* out);
int sgp_window_hop_f32(const int32_t* rowptr, const int32_t* col, const float* val,
                       const float* x, int64_t x_batch_stride, int64_t x_step_stride, int64_t x_node_stride,
                       float* out, int32_t src_block, int32_t dst_block, int32_t write_block0,
                       int32_t batch, int32_t steps, int32_t n, int32_t feat, int32_t n_blocks,
                       int32_t form, sgp_stream_t stream);

/* ------------------------------------------------- Decoder first layer ("next" row f4) ---
 * Grouped 1x1 convolution of lib/nn/models/sgp_model.py:41-52 (nn.Conv1d(input_size, out_channels,
 * kernel_size=1, groups) between two Rearranges, then the activation): for every row
 *   out[row, g*oc + o] = act(bias[g*oc + o] + sum_i W[g*oc + o, i] * X_row[g*ic + i]),  g < groups.
 * Row k is X[k, :] (x_row_stride) or, when step / node are given, X[step[k], node[k], :] -- the IID
 * gather of lib/datasets/iid_dataset.py:66-69 fused in, so the sampled batch never exists in HBM.
 * W is Conv1d's weight [groups*oc, ic] (trailing kernel axis of size 1 dropped), handed over in the
 * fragment order produced by sgp_grouped_linear_pack_f32 (sgp_grouped_linear_packed_floats floats).
 * act: 0 = none, 1 = relu, 2 = silu.  fp32 MFMA (v_mfma_f32_16x16x4_f32), exact products. */
int64_t sgp_grouped_linear_packed_floats(int32_t groups, int32_t ic, int32_t oc);
int sgp_grouped_linear_pack_f32(const float* w, float* packed, int32_t groups, int32_t ic, int32_t oc,
                                sgp_stream_t stream);
int sgp_grouped_linear_f32(const float* X, int64_t x_row_stride, int64_t x_batch_stride,
                           const int32_t* step, const int32_t* node,
                           const float* w_packed, const float* bias, int32_t act,
                           float* out, int64_t out_row_stride,
                           int32_t n_rows, int32_t groups, int32_t ic, int32_t oc,
                           sgp_stream_t stream);
/* Training the decoder (sgp_model.py:41-52 is a trained layer): the same forward that also writes the
 * pre-activation values `pre[n_rows, groups*oc]` (NULL = sgp_grouped_linear_f32), and the three pieces
 * of its backward pass.  With z = W x + b, y = act(z), incoming gradient dy:
 *   sgp_grouped_linear_dact_f32       dz = dy * act'(z)            (dz, pre contiguous [n_rows, width])
 *   sgp_grouped_linear_transpose_f32  W [groups*oc, ic] -> W^T laid out as the weight [groups*ic, oc] of
 *                                     the layer with ic and oc exchanged: dx = that layer (packed with
 *                                     sgp_grouped_linear_pack_f32, zero bias, act 0) applied to dz
 *   sgp_grouped_linear_wgrad_f32      dW[g*oc + o, i] = sum_row dz[row, g*oc + o] * X_row[g*ic + i]
 *                                     (rows as in the forward, IID gather included; fp32 MFMA with the
 *                                     rows as contraction index, row slices meet through float atomics)
 *   db = column sums of dz (sgp_node_mean_bcast_f32 with Y = NULL).
 * Dropout(p) behind the activation (sgp_model.py:50; training mode only): `dropout_p` in [0, 1) and a
 * 64-bit `seed` per call; element (row, column) is kept and scaled by 1 / (1 - p) when word 0 of
 * Philox4x32-10(key = seed, counter = row * width + column) >= p * 2^32.  The forward applies the factor
 * to `out` (not to `pre`), sgp_grouped_linear_dact_f32 with the same (p, seed) to dz. */
int sgp_grouped_linear_fwd_f32(const float* X, int64_t x_row_stride, int64_t x_batch_stride,
                               const int32_t* step, const int32_t* node,
                               const float* w_packed, const float* bias, int32_t act,
                               float* out, int64_t out_row_stride, float* pre,
                               double dropout_p, uint64_t seed,
                               int32_t n_rows, int32_t groups, int32_t ic, int32_t oc,
                               sgp_stream_t stream);
int sgp_grouped_linear_dact_f32(const float* dy, int64_t dy_row_stride, const float* pre, int32_t act,
                                double dropout_p, uint64_t seed,
                                float* dz, int64_t n_rows, int32_t width, sgp_stream_t stream);
int sgp_grouped_linear_transpose_f32(const float* w, float* wt, int32_t groups, int32_t ic, int32_t oc,
                                     sgp_stream_t stream);
int sgp_grouped_linear_wgrad_f32(const float* X, int64_t x_row_stride, int64_t x_batch_stride,
                                 const int32_t* step, const int32_t* node,
                                 const float* dz, float* dw,
                                 int32_t n_rows, int32_t groups, int32_t ic, int32_t oc,
                                 sgp_stream_t stream);
/* Which kernel form a launch takes -- host-only queries; the entries dispatch on these same answers (NULL outputs are
 * skipped; SGP_EINVAL on a bad size).
 * sgp_grouped_linear_form: jtc = 16-channel output tiles a wave accumulates together (1, 2, or 4: oc <= 16, <= 32,
 * more -- above 64 channels the wave makes further trips of 4 tiles, the last one partial when ceil(oc / 16) % 4 != 0;
 * above ic = 128 it makes further trips of 8 k-blocks); xvec = 1 when a lane reads its row piece with one 16-byte load:
 * ic % 4 == 0, both strides multiples of 4 floats and x_aligned16 (X on a 16-byte boundary), 0 = four scalar loads.
 * sgp_grouped_linear_wgrad_form: the row slices of sgp_grouped_linear_wgrad_f32 (slices = ceil(n_rows / rows_per_slice),
 * 0 without rows; every slice but the last has rows_per_slice rows, a multiple of 16 that is at least 64). */
int sgp_grouped_linear_form(int32_t ic, int32_t oc, int64_t x_row_stride, int64_t x_batch_stride, int32_t x_aligned16,
                            int32_t* jtc, int32_t* xvec);
int sgp_grouped_linear_wgrad_form(int32_t n_rows, int32_t groups, int32_t ic, int32_t oc,
                                  int32_t* rows_per_slice, int32_t* slices);
/* The same layer fed from the 16-bit embedding store: X holds bfloat16 / float16 elements (`fmt` =
 * SGP_STORE_BF16 / SGP_STORE_F16, anything else SGP_EINVAL), 2-byte aligned, strides in 16-bit ELEMENTS; every other
 * argument, the row sources (step / node, or step = NULL: plain rows X[row]), pre, dropout, activation and
 * out_row_stride are sgp_grouped_linear_fwd_f32's and sgp_grouped_linear_wgrad_f32's.  The kernels are the fp32 ones
 * instantiated for the source type: an element is widened to fp32 in registers (bf16: shift left by 16; fp16: the
 * hardware convert -- both exact) and enters the same v_mfma_f32_16x16x4_f32 chain in the same order, so
 *   sgp_grouped_linear_fwd_16(X16) is BIT-EQUAL to sgp_grouped_linear_fwd_f32(widened X16), out and pre, and
 *   sgp_grouped_linear_wgrad_16 is bit-equal to sgp_grouped_linear_wgrad_f32 wherever that one is deterministic (one
 *   row slice); with several slices both meet in dW through float atomics in no fixed order.
 * Weights, bias, dz, out, pre and dW stay fp32; no gradient exists for X.  n_rows == 0: success without a launch (the
 * wgrad entry still zeroes dW).
 * sgp_grouped_linear_form_16: jtc as sgp_grouped_linear_form; xvec = 1 when a lane reads the 4 elements of a k-block
 * with one 8-byte load: ic % 4 == 0, both strides multiples of 4 elements and x_aligned8 (X on an 8-byte boundary);
 * 0 = one element at a time (any ic, any stride, 2-byte alignment). */
int sgp_grouped_linear_fwd_16(const void* X, int32_t fmt, int64_t x_row_stride, int64_t x_batch_stride,
                              const int32_t* step, const int32_t* node,
                              const float* w_packed, const float* bias, int32_t act,
                              float* out, int64_t out_row_stride, float* pre,
                              double dropout_p, uint64_t seed,
                              int32_t n_rows, int32_t groups, int32_t ic, int32_t oc,
                              sgp_stream_t stream);
int sgp_grouped_linear_wgrad_16(const void* X, int32_t fmt, int64_t x_row_stride, int64_t x_batch_stride,
                                const int32_t* step, const int32_t* node,
                                const float* dz, float* dw,
                                int32_t n_rows, int32_t groups, int32_t ic, int32_t oc,
                                sgp_stream_t stream);
int sgp_grouped_linear_form_16(int32_t ic, int32_t oc, int64_t x_row_stride, int64_t x_batch_stride, int32_t x_aligned8,
                               int32_t* jtc, int32_t* xvec);

/* ---------------------------------------------------------- Ridge readout ---
 * The closed-form baseline's readout (experiments/run_closed_form.py:169-247): sklearn Ridge(alpha) fitted once per
 * lag on a host copy of [data | encoded_x].  Here the design matrix is VIRTUAL and never materialised: row
 * r = s * n_nodes + n (s < n_steps) is node n at step steps[s] (int32, device, any order), and its columns are up to 8
 * SEGMENTS laid side by side.  `segs` is a HOST table of n_segs x 6 int64:
 *   (device pointer, step stride, node stride, width, step offset, reps)
 * and column q * width + c of a segment (c < width, q < reps) is
 *   base[(steps[s] + offset + q) * step_stride + n * node_stride + c]
 * (fp32; node stride 0 broadcasts a global [T, c] series over the nodes; offset 1 with reps H is the target of lags
 * 1 .. H as one segment).  The caller guarantees
 * that every steps[s] + offset addresses a step of the tensor (sgp_amd/readout.py checks it before any device work).
 * All reductions are fp64 in a fixed order, without atomics: results are bit-identical run to run.
 *
 * Workspace sizes (bytes, -1 on a bad size): which = 0 colmeans, 1 Gram (n_cols counts the ones column), 2 predict
 * (n_out = horizon x channels).  n_rows = n_steps x n_nodes. */
int64_t sgp_ridge_workspace_bytes(int32_t which, int64_t n_rows, int32_t n_cols, int32_t n_out);
/* The launch regime of the three entries for these sizes -- a host-only query (no device call, no stream) computed by
 * the functions the entries launch with; same arguments as sgp_ridge_workspace_bytes.  out[] (int64):
 *   which = 0: {row slices, rows per slice}
 *   which = 1: {nt1 = ceil(n_cols / 128), upper-triangle tiles, row slices, rows per slice (the last slices may be
 *              short or empty), the most fp32 partials (one per 256 rows) a slice adds into its fp64 slab}
 *   which = 2: {NT = ceil(n_out / 16), workgroups, the most 64-row blocks a workgroup walks, 32-column panels,
 *              dynamic LDS bytes}
 * SGP_EINVAL on a size the entry refuses; SGP_EUNSUP (out[] still filled) where sgp_ridge_predict_score_f32 answers
 * SGP_EUNSUP: the dynamic LDS plus the kernel's 768 static bytes exceed 160 KiB. */
int sgp_ridge_form(int32_t which, int64_t n_rows, int32_t n_cols, int32_t n_out, int64_t* out);

/* means[c] = column means of the virtual matrix (fp64; the fp32 values are summed in fp64).
 *   replaces the centring inside sklearn Ridge.fit (run_closed_form.py:195, _preprocess_data) */
int sgp_ridge_colmeans_f32(const int64_t* segs, int32_t n_segs, const int32_t* steps, int64_t n_steps,
                           int64_t n_nodes, double* means, void* work, int64_t work_bytes, sgp_stream_t stream);

/* gram[i * ldg + j] (fp64, both triangles) = Zc^T Zc for Zc = [Z - shift | 1]: shift[c] (fp32, device; NULL = no
 * shift) is subtracted in fp32, the ones column is appended when ones = 1.  EXACT-FP32 contract: the products are
 * v_mfma_f32_32x32x2_f32 (one fp32 rounding per product-add, no reduced-precision inputs) over at most 256 rows, and
 * each such partial is added into fp64.  Only upper-triangle 128 x 128 tiles are computed.  Products of two
 * node-invariant columns (segments of node stride 0, the ones column) would add one value n_nodes times in a row, each
 * addition rounding the same way; with n_nodes > 1 and such a segment they are n_nodes x the fp64 sum over the steps.
 *   replaces the X^T X + X^T y of the 12 Ridge.fit calls at run_closed_form.py:191-196 (one Gram for every lag: the
 *   targets are columns of the same matrix) */
int sgp_ridge_gram_f32(const int64_t* segs, int32_t n_segs, const int32_t* steps, int64_t n_steps, int64_t n_nodes,
                       const float* shift, int32_t ones, double* gram, int64_t ldg, void* work, int64_t work_bytes,
                       sgp_stream_t stream);

/* One pass over the rows for all H x C outputs: yhat = X W + b with W [D, H*C] (fp32, column l * C + c = lag l + 1,
 * channel c) held in LDS and b [H*C] fp64; products v_mfma_f32_16x16x4_f32 over 64-column partials added in fp64.
 * scale / bias (NULL = none; element (n, c) at n * sc_node_stride + c) apply tsl's inverse_transform
 * yhat * (scale + 5e-8) + bias.  With y (raw target, (t, n, c) at t * y_ss + n * y_ns + c) the masked sums of tsl's
 * numpy_metrics against the target at step steps[s] + l + 1 and mask (uint8, NULL = all valid) go to sums[H][4] =
 * (sum |e|, sum e^2, sum |e / (y + 5e-8)|, count).  yhat [S, H, N, C] fp32 is written when not NULL.
 * SGP_EUNSUP when W does not fit in LDS (D rounded up to 32, times H*C rounded up to 16, times 4 bytes, plus about
 * 8 KiB + 512 bytes per output column within 160 KiB); H * C <= 64.
 *   replaces Ridge.predict + inverse_transform + masked_mae / mse / mape of run_closed_form.py:199-247 */
int sgp_ridge_predict_score_f32(const int64_t* segs, int32_t n_segs, const int32_t* steps, int64_t n_steps,
                                int64_t n_nodes, const float* W, const double* b, int32_t horizon, int32_t channels,
                                const float* scale, const float* bias, int64_t sc_node_stride,
                                const float* y, int64_t y_ss, int64_t y_ns,
                                const uint8_t* mask, int64_t m_ss, int64_t m_ns, int64_t m_cs,
                                float* yhat, double* sums, void* work, int64_t work_bytes, sgp_stream_t stream);

/* The same pass for a PATH of n_alphas = G regularisation strengths solved from one Gram: W [D, G*H*C] fp32 row-major,
 * column (g * H + l) * C + c = alpha g, lag l + 1, channel c; b [G*H*C] fp64; yhat [G, S, H, N, C] or NULL; sums
 * [G, H, 4] fp64 or NULL.  The kernel ADDS into sums (the caller zeroes it; chunks staged from the host accumulate).
 * Segments, steps, scaler, y and mask as in sgp_ridge_predict_score_f32, and so is the arithmetic of every output
 * column: v_mfma_f32_16x16x4_f32 with the same k per lane in the same panel order, fp32 partials over at most 64
 * feature columns added in fp64, the bias in fp64, the inverse transform with scale + 5e-8f in fp32, y + 5e-8f in
 * fp32; with the g-th column block of W and b the single-alpha entry writes the same yhat bit for bit.  W is not held
 * in LDS but streamed: per 32-column K panel one X stage [64 x 32] and one W stage [32 x 16 TP], the columns walked in
 * passes of TP <= 8 16-column tiles (a row block with several passes stages X again).  There is no LDS refusal.  The
 * masked sums go through one slab per workgroup in `work` and a final kernel, in a fixed order, without atomics.
 * Limits (SGP_EINVAL): G 1 .. 64, H*C 1 .. 256, G*H*C <= 4096, n_cols <= 16384.
 * sgp_ridge_path_form -- host only, computed by the functions the entry launches with -- fills out[] (int64) with
 *   {16-column tiles = ceil(G*H*C / 16), tiles per pass TP, passes, workgroups, the most 64-row blocks a workgroup
 *    walks, 32-column K panels, dynamic LDS bytes (the kernel adds 768 static bytes)}
 * and sgp_ridge_path_workspace_bytes is what the entry needs (-1 on a bad size): workgroups x passes x TP x 16 x 32. */
int64_t sgp_ridge_path_workspace_bytes(int64_t n_rows, int32_t n_cols, int32_t n_out, int32_t n_alphas);
int sgp_ridge_path_form(int64_t n_rows, int32_t n_cols, int32_t n_out, int32_t n_alphas, int64_t* out);
int sgp_ridge_predict_score_path_f32(const int64_t* segs, int32_t n_segs, const int32_t* steps, int64_t n_steps,
                                     int64_t n_nodes, const float* W, const double* b, int32_t n_alphas,
                                     int32_t horizon, int32_t channels,
                                     const float* scale, const float* bias, int64_t sc_node_stride,
                                     const float* y, int64_t y_ss, int64_t y_ns,
                                     const uint8_t* mask, int64_t m_ss, int64_t m_ns, int64_t m_cs,
                                     float* yhat, double* sums, void* work, int64_t work_bytes, sgp_stream_t stream);


/* ------------------------------------------------ Decoder MLP and readout -----
 * The trained layers of SGPModel after its input layer (decoder_mlp.hip), forward and backward.  EXACT-FP32
 * contract: every product is a v_mfma_f32_16x16x4_f32 (no reduced-precision inputs).
 *
 * Packed weights: the matrix M[n_out, k] of a layer (transpose = 0: M[j][i] = w[j * w_row_stride + i], an nn.Linear
 * weight; transpose = 1: M[j][i] = w[i * w_row_stride + j], its transpose for dX) in the fragment order of the dense
 * kernel, sgp_dense_packed_floats(n_out, k) floats, 16-byte aligned. */
int64_t sgp_dense_packed_floats(int32_t n_out, int32_t k);
int sgp_dense_pack_f32(const float* w, int64_t w_row_stride, int32_t transpose, int32_t n_out, int32_t k,
                       float* packed, sgp_stream_t stream);

/* out = epilogue(X M^T) over n_rows rows.  Row r of X is X[src(r) * x_row_stride + 0 .. k-1] with
 * src(r) = gather[r % row_mod] (gather != NULL; row_mod = 0: r) or r % row_mod (gather == NULL).  Epilogue of
 * column c < n_out, v = (X M^T)[r, c] (+ bias[c]):
 *   dmode = 0, c < n_act:  pre[r * pre_row_stride + c] = v (pre != NULL);  v = act(v) * keep(r, c)
 *   dmode = 1, c < n_act:  v = v * act'(dpre[r * dpre_row_stride + c]) * keep(r, c)      (the backward pass)
 *   then v += add[r * add_row_stride + c] (add != NULL), stored at
 *   out[(r / m0) m1 + (r % m0) m2 + (c / m3) m4 + (c % m3) m5] with out_map = {m0, .., m5} (host array).
 * act: 0 linear, 1 relu, 2 silu, 3 elu (alpha 1: v > 0 ? v : expm1(v), act' = z > 0 ? 1 : exp(z); this entry and
 * sgp_grouped_linear_dact_f32 only); keep(r, c) = the Philox dropout factor of decoder.hip at flat index
 * r * drop_width + c (1 when dropout_p = 0, 0 when dropout_p = 1).
 *   replaces nn.Linear + activation + Dropout of tsl Dense (tsl/nn/base/dense.py:19-23), the stacked Linear1 / skip
 *   of ResidualMLP (tsl/nn/blocks/encoders/mlp.py:86-111), lin_emb + the positional add (sgp_model.py:76,97), the
 *   readout and its Rearrange (tsl/nn/blocks/decoders/linear_readout.py:23-26), and every dX of their backward */
int sgp_dense_f32(const float* X, int64_t x_row_stride, const int32_t* gather, int64_t row_mod,
                  const float* w_packed, const float* bias, int32_t n_rows, int32_t k, int32_t n_out,
                  int32_t act, int32_t n_act, int32_t dmode, const float* dpre, int64_t dpre_row_stride,
                  float* pre, int64_t pre_row_stride, double dropout_p, uint64_t seed, int64_t drop_width,
                  const float* add, int64_t add_row_stride,
                  float* out, const int64_t* out_map, sgp_stream_t stream);
/* The form sgp_dense_f32 launches for these sizes -- a host-only query; the entry dispatches on this same answer (NULL
 * outputs are skipped; SGP_EINVAL on a bad size).  rows_per_wg: 128 when ceil(n_rows / 128) * ceil(n_out / 64) >= 512
 * workgroups (two per CU), 64 otherwise; xvec = 1 when a lane reads its row piece with one 16-byte load: k % 4 == 0,
 * x_row_stride % 4 == 0 and x_aligned16 (X on a 16-byte boundary), 0 = four scalar loads. */
int sgp_dense_form(int32_t n_rows, int32_t n_out, int32_t k, int64_t x_row_stride, int32_t x_aligned16,
                   int32_t* rows_per_wg, int32_t* xvec);

/* dw[o * dw_row_stride + i] = sum_r dZ[r * dz_row_stride + o] * X_row(r)[i] and (db != NULL) db[o] = sum_r dZ[r, o],
 * X_row as in sgp_dense_f32.  Row slices write partials into `work` (sgp_dense_wgrad_workspace_floats floats,
 * with_bias = db != NULL), added in slice order in fp64: no float atomics, bit-identical from run to run.  With
 * kp = k + with_bias there are workspace_floats / (n_out * kp) slices of rows_per_slice =
 * max(64, ceil(n_rows / max(1, 2048 / (ceil(n_out / 64) * ceil(kp / 64))))) rows rounded up to a multiple of 16
 * (integer divisions; the last slice may be shorter; one empty slice without rows).
 *   replaces the weight / bias gradients autograd forms for every nn.Linear of the decoder */
int64_t sgp_dense_wgrad_workspace_floats(int64_t n_rows, int32_t n_out, int32_t k, int32_t with_bias);
int sgp_dense_wgrad_f32(const float* dZ, int64_t dz_row_stride, const float* X, int64_t x_row_stride,
                        const int32_t* gather, int64_t row_mod, int32_t n_rows, int32_t n_out, int32_t k,
                        float* dw, int64_t dw_row_stride, float* db, float* work, int64_t work_floats,
                        sgp_stream_t stream);

/* out[n_seg, width] = per-node sums of the rows of g, in a fixed order (fp64):
 *   perm == NULL: out[n] = sum_b g[b * n_seg + n]   (n_rows a multiple of n_seg)
 *   otherwise keys = the rows' node ids stably sorted, perm = the row of each sorted position; out[keys[p]] = sum of
 *   g[perm[p]] over the run of p (nodes without rows: 0).
 *   replaces the node_emb.emb gradient of the embedding lookup (tsl/nn/base/embedding.py:93, sgp_model.py:97) */
int sgp_row_segsum_f32(const float* g, int64_t g_row_stride, int64_t n_rows, int32_t width,
                       const int32_t* perm, const int32_t* keys, int32_t n_seg, float* out, sgp_stream_t stream);


/* ------------------------------------------------ Training step: optimizer, losses, metrics -----
 * train.hip.  Every reduction adds fixed partials in a fixed order in fp64: no float atomics, bit-identical from
 * run to run.
 *
 * Chunk table (device memory, int64 [n_chunks][3]): (tensor id, element offset, length).  A chunk lies inside one
 * tensor; tensor t's base addresses are params[t], grads[t], exp_avg[t], exp_avg_sq[t] of four DEVICE pointer arrays.
 * The kernels take any chunk length (sgp_amd/optim.py cuts 2048 elements) and any 4-byte aligned base: a chunk is a
 * head of up to 3 scalars, 16-byte vectors, and a tail.
 *
 * norm_f32[0] (and norm_f64[0] when not NULL) = sqrt(sum of g^2 over every chunk): one workgroup per chunk writes
 * partial[chunk] (fp64, n_chunks doubles), one workgroup adds them.  0 without chunks.
 *   replaces the norm of torch.nn.utils.clip_grad_norm_ (gradient_clip_val of the reference's trainers) */
int sgp_multi_sqnorm_f32(const int64_t* table, int64_t n_chunks, const float* const* grads, double* partial,
                         float* norm_f32, double* norm_f64, sgp_stream_t stream);

/* One Adam step (torch.optim.adam._single_tensor_adam, no amsgrad, no maximize) over the table, one launch:
 *   max_norm > 0:  g *= min(1, max_norm / (norm[0] + 1e-6)) -- clip_grad_norm_'s coefficient, read from the device;
 *                  a non-finite norm propagates as in torch.  The clipped gradient is NOT written back.
 *                  max_norm <= 0: no clip, norm may be NULL.
 *   decoupled = 0: g += weight_decay * p (Adam);  decoupled = 1: p *= 1 - lr * weight_decay (AdamW)
 *   m += (1 - beta1) (g - m);  v = beta2 v + (1 - beta2) g^2
 *   p -= lr / (1 - beta1^step) * m / (sqrt(v) / sqrt(1 - beta2^step) + eps),  step >= 1 the number of THIS step.
 * Every hyper-parameter is passed by value (a scheduler needs no device write).
 *   replaces torch.optim.Adam.step and the in-place scaling of clip_grad_norm_ */
int sgp_adam_step_f32(const int64_t* table, int64_t n_chunks, float* const* params, const float* const* grads,
                      float* const* exp_avg, float* const* exp_avg_sq, const float* norm, double max_norm,
                      double lr, double beta1, double beta2, double eps, double weight_decay, int64_t step,
                      int32_t decoupled, sgp_stream_t stream);

/* state[h][0..5] += per horizon step h of contiguous y_hat, y [batch, horizon, nodes, channels] (mask: uint8 of the
 * same shape, NULL = all valid), with d = y_hat' - y and y_hat' = y_hat * (scale + 5e-8) + bias (scale, bias NULL =
 * y_hat; element (n, c) at n * sc_node_stride + c -- tsl ScalerModule.inverse_transform_tensor):
 *   0: sum |d|   1: their number   2: sum d^2 (over the elements of 1)   5: sum y (over the elements of 1)
 *   3: sum |d / y|   4: their number
 * An element enters 0 / 1 / 2 / 5 when the mask keeps it and, with mask_nans, |d| is not NaN and, with mask_inf, not
 * infinite; it enters 3 / 4 when the mask keeps it, |d / y| is finite-or-NaN (MaskedMAPE: mask_inf always) and, with
 * mask_nans, not NaN -- MaskedMetric._check_mask on the metric's own value.  `work`: at least
 * sgp_masked_metrics_workspace_doubles doubles (per-unit partials: 2048 elements of one horizon step each); a second
 * launch of one workgroup per step adds them into `state` ([horizon][6] fp64, persistent: the caller zeroes it).
 *   replaces MaskedMAE / MaskedMSE / MaskedMAPE / MaskedMRE .update, with and without at= (tsl/nn/metrics) */
int64_t sgp_masked_metrics_workspace_doubles(int64_t batch, int32_t horizon, int64_t nodes, int32_t channels);
int sgp_masked_metrics_f32(const float* y_hat, const float* y, const uint8_t* mask, int64_t batch, int32_t horizon,
                           int64_t nodes, int32_t channels, const float* scale, const float* bias,
                           int64_t sc_node_stride, int32_t mask_nans, int32_t mask_inf, double* work,
                           int64_t work_doubles, double* state, sgp_stream_t stream);

/* loss[0] = sum of f(y_hat, y) over the counted elements / their number (count[0]; the plain sum, 0, when nothing
 * counts), over contiguous [batch, horizon, row]; kind 0: f = |d|, 1: d^2, 2: |d / y| (infinite values never count);
 * at >= 0: horizon step `at` only, -1: all.  grad[e] = grad_out[0] / count[0] * df/dy_hat on the counted elements
 * (sign(d), 2 d, sign(d) / |y|), 0 elsewhere.  `work`: sgp_masked_loss_workspace_doubles doubles.
 *   replaces MaskedMAE / MaskedMSE / MaskedMAPE (tsl/nn/metrics/metric_base.py:79-96) as the loss of every training
 *   loop and as loss_fn of the reference's Predictor */
int64_t sgp_masked_loss_workspace_doubles(int64_t batch, int32_t horizon, int64_t row, int32_t at);
int sgp_masked_loss_f32(const float* y_hat, const float* y, const uint8_t* mask, int64_t batch, int32_t horizon,
                        int64_t row, int32_t kind, int32_t at, int32_t mask_nans, double* work, int64_t work_doubles,
                        float* loss, double* count, sgp_stream_t stream);
int sgp_masked_loss_bwd_f32(const float* y_hat, const float* y, const uint8_t* mask, int64_t batch, int32_t horizon,
                            int64_t row, int32_t kind, int32_t at, int32_t mask_nans, const float* grad_out,
                            const double* count, float* grad, sgp_stream_t stream);

/* The loss and the metrics on the ROOT NODES of a sampled batch.  y_hat is contiguous [batch, horizon, nodes_all,
 * channels] (the model's output on every node of the subgraph); y and mask are [batch, horizon, roots, channels] and
 * root j is node target_nodes[j] of y_hat (int32 or int64, index_bytes = 4 or 8, device).  The forward entries walk the
 * units of sgp_masked_loss_f32 / sgp_masked_metrics_f32 over the sliced index space and add the same partials in the
 * same order: loss, count and state are bit-equal to those entries on y_hat[..., target_nodes, :].contiguous().
 * err (int32, device, persistent: the caller zeroes it, the kernels only OR into it): bit 0 an id outside
 * [0, nodes_all) -- compared (unsigned) before it indexes anything; such an element contributes nothing -- bit 1 a
 * node named twice.
 *
 * sgp_target_nodes_table: inv[nodes_all] (int32) with inv[target_nodes[j]] = j and -1 elsewhere (a memset and one
 * launch; a repeated node is seen by the integer atomicMax that writes the table and keeps its larger j).
 * sgp_masked_loss_nodes_bwd_f32: the FULL gradient [batch, horizon, nodes_all, channels] in one launch -- row n with
 * inv[n] = j >= 0 gets what sgp_masked_loss_bwd_f32 writes for sliced row j, every other row +0; every element is
 * written exactly once (no memset before it, no atomics), 16 bytes per lane when grad is 16-byte aligned.
 * sgp_masked_metrics_nodes_f32: scale / bias are addressed by the ROOT position j (element (j, c) at
 * j * sc_node_stride + c): the sampler slices the target's scaler with the roots.
 *   replaces y_hat[..., batch.target_nodes, :] and the loss_fn / metrics.update calls on it, and the zero fill +
 *   index_put of its backward (lib/predictors/subgraph_predictor.py:14-15,25,28; 42-43,53,56; 66-67,70,73) */
int sgp_target_nodes_table(const void* target_nodes, int32_t index_bytes, int64_t roots, int64_t nodes_all,
                           int32_t* inv, int32_t* err, sgp_stream_t stream);
int sgp_masked_loss_nodes_f32(const float* y_hat, const float* y, const uint8_t* mask, const void* target_nodes,
                              int32_t index_bytes, int64_t batch, int32_t horizon, int64_t nodes_all, int64_t roots,
                              int32_t channels, int32_t kind, int32_t at, int32_t mask_nans, int32_t* err, double* work,
                              int64_t work_doubles, float* loss, double* count, sgp_stream_t stream);
int sgp_masked_loss_nodes_bwd_f32(const float* y_hat, const float* y, const uint8_t* mask, const int32_t* inv,
                                  int64_t batch, int32_t horizon, int64_t nodes_all, int64_t roots, int32_t channels,
                                  int32_t kind, int32_t at, int32_t mask_nans, const float* grad_out,
                                  const double* count, float* grad, sgp_stream_t stream);
int sgp_masked_metrics_nodes_f32(const float* y_hat, const float* y, const uint8_t* mask, const void* target_nodes,
                                 int32_t index_bytes, int64_t batch, int32_t horizon, int64_t nodes_all, int64_t roots,
                                 int32_t channels, const float* scale, const float* bias, int64_t sc_node_stride,
                                 int32_t mask_nans, int32_t mask_inf, int32_t* err, double* work, int64_t work_doubles,
                                 double* state, sgp_stream_t stream);
/* The launch regime of the four entries above -- a host-only query computed by the functions the entries launch with.
 * The workspaces are those of sgp_masked_loss_workspace_doubles(batch, horizon, roots * channels, at) and
 * sgp_masked_metrics_workspace_doubles(batch, horizon, roots, channels).  out[7] (int64):
 *   0: units (2048 sliced elements each) of the loss -- over the whole sliced tensor, or over step `at`
 *   1: units per horizon step of the metrics
 *   2: workgroups of the backward (at most 2048)   3: its grid-stride trips (the most any thread makes)
 *   4: elements per lane of the backward: 4 (grad_aligned16 and at least 4 elements), else 1
 *   5: 1 = the int64 index kernels, 0 = int32   6: workgroups of the table launch */
int sgp_masked_nodes_form(int64_t batch, int32_t horizon, int64_t nodes_all, int64_t roots, int32_t channels,
                          int32_t at, int32_t index_bytes, int32_t grad_aligned16, int64_t* out);


/* ------------------------------------------------ Gated graph network: edges -----
 * The per-edge MLP, gate and sum of a GatedGraphNetwork layer (gated_gn.hip), forward and backward, for the same
 * edge list in every batch item.  EXACT-FP32 contract as above: every product is a v_mfma_f32_16x16x4_f32.
 * H = the layer's output width (even, 16..256), Hm = H / 2; act: 1 relu, 2 silu.  PQ [b * n, 2 Hm] holds the node
 * projection P = X Wa^T + b1 | Q = X Wb^T of msg_mlp.0's weight W1 = [Wa | Wb] (sgp_dense_f32).  An edge (j -> i) is
 *   z1 = P[i] + Q[j], a1 = act(z1), z2 = W2 a1 + b2, m = act(z2), g = sigmoid(wg . m + bg), agg[i] += g m.
 * Edge tables (int32, device), built once per edge list (sgp_amd/nn/layers/gated_gn.py, edge_plan):
 *   src[n_edges]      source of every edge, edges stably sorted by target
 *   chunks[n_chunks][4] = (target, first edge, end edge, partial row or -1): at most sgp_gated_gn_chunk_edges() edges
 *                     of one target; every target has at least one chunk (an empty one when nothing enters it), a
 *                     target with more edges has several, which write partial rows (n_parts in all, per batch item)
 *   fix[n_fix][3]     = (target, first partial row, count) of the split targets: their partials are added in chunk order
 *   src_ptr[n + 1], src_pos[n_edges]   the inverted index: positions in the target-sorted list of the edges OUT OF
 *                     each node, edges stably sorted by source
 * w2_packed / w2t_packed: sgp_dense_pack_f32 of msg_mlp.2's weight [H, Hm] with transpose = 0 (n_out = H, k = Hm) / 1
 * (n_out = Hm, k = H); b2 [H]; wg [H], bg [1] = gate_mlp.0 (device pointers).  Sizes outside the domain: SGP_EUNSUP;
 * sgp_gated_gn_supported returns 0 for them and leaves the reason in sgp_last_error.
 * Workspace bytes (-1 on a bad size): forward b * n_parts * H floats; backward the dz1 rows of a slice of batch items
 * (at most SGP_TUNE gated_gn_ws_mb = 256 MiB, one item at least) + partial rows + per-workgroup weight partials. */
int32_t sgp_gated_gn_supported(int32_t H, int32_t act);
int32_t sgp_gated_gn_chunk_edges(void);
int64_t sgp_gated_gn_workspace_bytes(int32_t backward, int64_t b, int64_t n_edges, int64_t n_chunks, int32_t n_parts,
                                     int32_t H);

/* agg [b * n, H]: every row written (no incoming edge: zeros); nothing of size n_edges is written.
 *   replaces propagate() of tsl/nn/layers/graph_convs/gated_gn.py:56 = message() of lines 62-64 (cat([x_i, x_j]),
 *   msg_mlp.1-3, gate_mlp, the product) and torch_geometric's gather and scatter-add around it */
int sgp_gated_gn_edge_f32(const float* PQ, int64_t pq_row_stride, int32_t b, int32_t n, int32_t H, int32_t act,
                          const int32_t* chunks, int32_t n_chunks, const int32_t* src, int64_t n_edges,
                          const int32_t* fix, int32_t n_fix, int32_t n_parts,
                          const float* w2_packed, const float* b2, const float* wg, const float* bg,
                          float* agg, int64_t agg_row_stride, void* work, int64_t work_bytes, sgp_stream_t stream);

/* Recomputes z1 .. g per edge from PQ; with dm = dAgg[i] g + (dAgg[i] . m) g (1 - g) wg, dz2 = dm act'(z2),
 * dz1 = (W2^T dz2) act'(z1):  dPQ[i, 0 .. Hm) = sum of dz1 over the edges INTO i, dPQ[j, Hm .. 2 Hm) = over the edges
 * OUT OF j, dW2 [H, Hm] = sum dz2 a1^T, db2 [H] = sum dz2, dwg [H] = sum (dAgg[i] . m) g (1 - g) m, dbg [1].
 * No float atomics; bit-identical from run to run.
 *   replaces what autograd derives for the lines above (the saved [b, E, .] tensors of message() included) */
int sgp_gated_gn_edge_bwd_f32(const float* PQ, int64_t pq_row_stride, const float* dAgg, int64_t dagg_row_stride,
                              int32_t b, int32_t n, int32_t H, int32_t act,
                              const int32_t* chunks, int32_t n_chunks, const int32_t* src, int64_t n_edges,
                              const int32_t* fix, int32_t n_fix, int32_t n_parts,
                              const int32_t* src_ptr, const int32_t* src_pos,
                              const float* w2_packed, const float* w2t_packed, const float* b2, const float* wg,
                              const float* bg, float* dPQ, int64_t dpq_row_stride, float* dW2, float* db2, float* dwg,
                              float* dbg, void* work, int64_t work_bytes, sgp_stream_t stream);

/* ------------------------------------------------ Trained recurrent baselines: LSTM / GRU window -----
 * The gated recurrence of one torch.nn.LSTM / torch.nn.GRU layer (batch_first = False, zero initial state) over a
 * window of S steps for M independent sequences (rnn_window.hip), forward and backward through time.  EXACT-FP32
 * contract as above: every product is a v_mfma_f32_16x16x4_f32; no float atomics, bit-identical from run to run.
 * cell: 0 lstm (gates i, f, g, o), 1 gru (gates r, z, n; n = tanh(W_in x + b_in + r (W_hn h + b_hn)),
 * h' = (1 - z) n + z h).  H: a multiple of 16 in 16 .. 256; S, M >= 1; anything else returns SGP_EUNSUP with the reason
 * in sgp_last_error (sgp_rnn_window_supported answers without a GPU).
 * gates [S][M][4 H] (sgp_rnn_window_workspace_bytes): on entry the input projection W_ih x_t + b_ih (+ b_hh; GRU:
 * blocks 0 .. 2, with b_hr and b_hz but NOT b_hn folded in), one sgp_dense_f32 launch for all S M rows.
 * packed: sgp_rnn_window_packed_floats floats, W_hh [G H, H] in the fragment order of both directions. */
int32_t sgp_rnn_window_supported(int32_t cell, int32_t H);
int64_t sgp_rnn_window_packed_floats(int32_t cell, int32_t H);
int64_t sgp_rnn_window_workspace_bytes(int32_t cell, int32_t H, int32_t S, int64_t M);
int sgp_rnn_window_pack_f32(const float* w_hh, int32_t cell, int32_t H, float* packed, sgp_stream_t stream);

/* One launch for the whole window.  save != 0 (training): the gate buffer is overwritten with what backward reads
 * (LSTM: the activated i, f, g, o; GRU: r, z, n and W_hn h + b_hn in block 3), h_seq [S][M][H] and, for the LSTM,
 * c_seq [S][M][H] are stored.  h_seq (any mode, may be NULL): every step's state; h_last (may be NULL) [M][H]: the
 * last one.  h_drop (may be NULL) [S][M][H]: h times the Philox dropout factor of decoder.hip at flat index
 * (t M + m) H + column (0 < dropout_p <= 1; p = 1: zeros), the next layer's input.
 *   replaces self.rnn(x) of tsl/nn/blocks/encoders/rnn.py:57 (torch.nn.LSTM / GRU: the recurrent half of every cell
 *   step, the cell update and the dropout between layers) and x[:, -1] of line 61 */
int sgp_rnn_window_fwd_f32(int32_t cell, int32_t H, int32_t S, int64_t M, float* gates, const float* packed,
                           const float* b_hn, float* h_seq, float* c_seq, float* h_drop, double dropout_p, uint64_t seed,
                           float* h_last, int32_t save, sgp_stream_t stream);

/* Time reversed; dh and dc never leave the chip.  dy: the cotangent of h, [M][H] for the last step only
 * (dy_full = 0) or [S][M][H] (dy_full = 1).  The saved gates are overwritten in place with the gradients of the
 * pre-activations: LSTM the 4 blocks; GRU [dr, dz, dn, dn r] -- the input side (dW_ih, db_ih, dx) reads blocks 0 .. 2,
 * the hidden side (dW_hh, db_hh) blocks 0, 1 and 3.  Weight gradients: sgp_dense_wgrad_f32 on slices of this buffer.
 *   replaces what autograd derives for the lines above (cuDNN-style BPTT of torch.nn.LSTM / GRU) */
int sgp_rnn_window_bwd_f32(int32_t cell, int32_t H, int32_t S, int64_t M, float* gates, const float* packed,
                           const float* h_seq, const float* c_seq, const float* dy, int32_t dy_full,
                           sgp_stream_t stream);

/* ------------------------------------------------ RNN imputers: the fill-in GRU recurrence -----
 * rnn_impute.hip: the time loop of RNNImputerModel (tsl/nn/models/imputation/rnni_models.py:74-96) for M independent
 * sequences of S steps with D fed-back columns,
 *   h_0 given (NULL: zeros),  p_s = W_r h_s + b_r,  xp_s = m_s ? x_s : p_s,  h_{s+1} = GRUCell([xp_s | u_s | m_s], h_s)
 * for s = 0 .. S-2 (x_{S-1} is never an input).  EXACT-FP32 contract as above: every product is a
 * v_mfma_f32_16x16x4_f32, one k-ordered chain per output, no float atomics, bit-identical from run to run and
 * independent of the tile a sequence falls into.  h and the backward carries stay on chip for the whole window.
 * Domain: GRU; H a multiple of 16 in 16 .. 256; D in 1 .. 512; S, M >= 1; anything else returns SGP_EUNSUP with the
 * reason in sgp_last_error (sgp_rnn_impute_supported answers without a GPU).
 * Rows.  mask, xp, p, dP and gx lie in the window's own order: row (m / inner) * S * inner + t * inner + m % inner for
 * step t of sequence m -- [b, s, n, c] read in place with inner = n (independent nodes, D = c) or inner = 1 (joint,
 * D = n c).  gates, h_seq, dH and dp are [S][M][.].  reverse != 0 walks the window from its last step to its first and
 * reads and writes rows at S-1-t, which is a forward run on the time-flipped window, flipped back.
 * gates [S][M][4 H] (sgp_rnn_impute_workspace_bytes): on entry blocks 0 .. 2 hold the state-free part
 * W_x (m . x) + W_u u + W_m m + b_ih (+ b_hr, b_hz; NOT b_hn) of all S M rows, one sgp_dense_f32 launch.
 * packed: sgp_rnn_impute_packed_floats floats; W_hh [3 H, H], W_x = weight_ih[:, :D] and W_r [D, H] in the fragment
 * order of both directions, zero padded to whole tiles of 16 along D. */
int32_t sgp_rnn_impute_supported(int32_t H, int32_t D);
int64_t sgp_rnn_impute_packed_floats(int32_t H, int32_t D);
int64_t sgp_rnn_impute_workspace_bytes(int32_t H, int32_t D, int32_t S, int64_t M);
int sgp_rnn_impute_pack_f32(const float* w_ih, int64_t w_ih_row_stride, const float* w_hh, const float* w_r, int32_t H,
                            int32_t D, float* packed, sgp_stream_t stream);

/* The launch form for these sizes (host only): plan[0] column tiles of 16 per wave (1, 2 or 4), [1] waves per
 * workgroup, [2] tiles of 16 along D (1: every D tile is wave 0's; more: dealt round robin over the waves),
 * [3] workgroups (16 sequences each), [4] / [5] bytes of LDS of the forward / backward launch. */
int sgp_rnn_impute_plan(int32_t H, int32_t D, int64_t M, int32_t* plan);

/* One launch for the whole window: p (every step's prediction) and h_seq (h_0 .. h_{S-1}) are stored.  mask: 0 / 1
 * floats.  save != 0 (training): the gate buffer is overwritten with what backward reads (r, z, n and W_hn h + b_hn in
 * block 3) and xp -- on entry m . x, the operand the state-free part was computed from -- receives p_s at the missing
 * entries of steps 0 .. S-2, which makes it the merged input, the weight-gradient operand of W_x.
 *   replaces the loop of tsl/nn/models/imputation/rnni_models.py:83-96 (init_hidden_state aside): readout,
 *   _preprocess_input (lines 62-72), rnn_cell and the two stacks */
int sgp_rnn_impute_fwd_f32(int32_t H, int32_t D, int32_t S, int64_t M, int64_t inner, int32_t reverse, float* gates,
                           const float* packed, const float* b_hn, const float* b_r, const float* h0, const float* mask,
                           int64_t mask_row_stride, float* xp, int64_t xp_row_stride, float* p, float* h_seq,
                           int32_t save, sgp_stream_t stream);

/* Time reversed, one launch.  dP: the cotangent of p; dH (may be NULL) [S][M][H]: the cotangent of h_seq (the Bi
 * model's read_out).  The saved gates are overwritten in place with the gradients of the pre-activations
 * [dr, dz, dn, dn r] (the input side reads blocks 0 .. 2, the hidden side 0, 1 and 3; the row of the last step is
 * zeroed, so weight gradients run over all S M rows and S = 1 gives exact zeros).  dp [S][M][D]: the total
 * dp_s = dP_s + (1 - m_s) . W_x^T dgates_s (detach != 0: dP_s alone), the operand of dW_r, db_r.  gx (may be NULL):
 * m_s . W_x^T dgates_s, exactly zero at missing entries and at step S-1.
 *   replaces what autograd derives for rnni_models.py:83-96 (detach_input: line 64) */
int sgp_rnn_impute_bwd_f32(int32_t H, int32_t D, int32_t S, int64_t M, int64_t inner, int32_t reverse, int32_t detach,
                           float* gates, const float* packed, const float* h_seq, const float* mask,
                           int64_t mask_row_stride, const float* dP, const float* dH, float* dp, float* gx,
                           sgp_stream_t stream);

/* ------------------------------------------------ GRIN: the stages around the cells of one GRIL step -----
 * grin.hip (tsl/nn/layers/graph_convs/grin_cell.py:200-227, SpatialDecoder.forward :82-104).  With hT the top layer's
 * state entering the step, m the mask, R = b n rows, H hidden, C input and U exogenous columns:
 *   stage 1  p1 = W_fs hT + b_fs,  x1 = m ? x : p1,  z = W_in [x1 | m | hT | u] + b_in  -> slot 0 of dec [R, 3 H]
 *   (one sgp_diffuse_f32 launch: slots 1, 2 = A_f z, A_b z on the graph without self loops)
 *   stage 2  g = W_f [A_f z | A_b z] + b_f,  o = PReLU(W_o [g | hT] + b_o),  repr = [o | hT],  p2 = W_ro repr + b_ro,
 *            x2 = m ? x : p2,  [x2 | m | u] -> the leading columns of cell_in
 * EXACT-FP32 contract as above: v_mfma_f32_16x16x4_f32, one k-ordered chain per output, no atomics, bit-identical
 * from run to run and independent of the tile a row falls into; x is selected by the mask and never multiplied.
 * Domain: H a multiple of 16 in 16 .. 128, C in 1 .. 16, U in 0 .. 64, k as sgp_dcrnn_supported; anything else
 * returns SGP_EUNSUP with the reason in sgp_last_error (sgp_grin_supported answers without a GPU).
 * Rows.  x, mask (0 / 1 floats), p1, p2, dP1, dP2, gx [., C] and u, gu [., U] are contiguous and lie in the
 * window's own [b, S, n, .] order: row (r / inner) S inner + tt inner + r % inner for row r, inner = n, tt = t or, with
 * reverse != 0, S - 1 - t.  repr / dRepr rows lie in the same order, repr_row_stride floats apart.  hT, dec, cell_in,
 * the save buffers, ddec, carry, dp1 and dp2 [R][C] are rows of this step.
 * packed: sgp_grin_packed_floats floats; first_stage.weight [C, H], lin_in.weight [H, 2 C + H + U],
 * graph_conv.filters.weight [H, 2 H], lin_out.weight [H, 2 H], read_out.weight [C, 2 H] (all contiguous) in fragment
 * order, then their transposes. */
int32_t sgp_grin_supported(int32_t H, int32_t C, int32_t U, int32_t k);
int64_t sgp_grin_packed_floats(int32_t H, int32_t C, int32_t U);
int sgp_grin_pack_f32(const float* w_fs, const float* w_in, const float* w_f, const float* w_o, const float* w_ro,
                      int32_t H, int32_t C, int32_t U, float* packed, sgp_stream_t stream);

/* The launch form (host only): plan[0] tiles of 16 along H, [1] rounds of the 4 waves over them, [2] tiles of 16 along
 * 2 C + H + U, [3] workgroups (16 rows each), [4] .. [7] bytes of LDS of stage 1, stage 2, stage 2 backward and
 * stage 1 backward. */
int sgp_grin_plan(int32_t H, int32_t C, int32_t U, int64_t R, int32_t* plan);

/* save_in (may be NULL) [R][2 C + H + U]: the merged operand row of lin_in. */
int sgp_grin_stage1_f32(int32_t H, int32_t C, int32_t U, int64_t R, int64_t inner, int32_t S, int32_t t, int32_t reverse,
                        const float* packed, const float* b_fs, const float* b_in, const float* hT, int64_t h_row_stride,
                        const float* x, const float* mask, const float* u, float* p1, float* dec, int64_t dec_row_stride,
                        float* save_in, sgp_stream_t stream);

/* slope: the PReLU weight, read on the device.  repr may be NULL (nothing reads the representations).  save_pre [R][H] and save_cat [R][2 H] (both or neither): the
 * pre-activation of lin_out and its operand [g | hT]. */
int sgp_grin_stage2_f32(int32_t H, int32_t C, int32_t U, int64_t R, int64_t inner, int32_t S, int32_t t, int32_t reverse,
                        const float* packed, const float* b_f, const float* b_o, const float* b_ro, const float* slope,
                        const float* dec, int64_t dec_row_stride, const float* hT, int64_t h_row_stride, const float* x,
                        const float* mask, const float* u, float* p2, float* repr, int64_t repr_row_stride,
                        float* cell_in, int64_t cell_row_stride, float* save_pre, float* save_cat, sgp_stream_t stream);

/* dcell (may be NULL): the cotangent of cell_in.  dp2 = dP2 + (1 - m) dx2 (stored: the operand of read_out's weight
 * gradient), gx = m dx2 (gx may be NULL); pre is overwritten with the cotangent of lin_out's pre-activation, dg [R][H]
 * receives that of g; ddec [R, 3 H]: slots 1, 2 = W_f^T dg, slot 0 zeroed for the adjoint hop; carry [R][H] += the
 * cotangent of hT; slope_partial [workgroups]: per-workgroup sums of the slope's gradient (fixed order, fp64 inside).
 *   replaces what autograd derives for SpatialDecoder.forward :100-104 and grin_cell.py:216 */
int sgp_grin_stage2_bwd_f32(int32_t H, int32_t C, int32_t U, int64_t R, int64_t inner, int32_t S, int32_t t,
                            int32_t reverse, const float* packed, const float* slope, const float* mask, const float* dP2,
                            const float* dRepr, int64_t drepr_row_stride, const float* dcell, int64_t cell_row_stride,
                            float* pre, float* dg, float* ddec, int64_t ddec_row_stride, float* carry, float* gx,
                            float* dp2, float* slope_partial, sgp_stream_t stream);

/* After the adjoint hop: d[x1 | m | hT | u] = W_in^T (slot 0 of ddec); dp1 = dP1 + (1 - m) dx1 (stored), gx += m dx1,
 * gu = du + the u columns of dcell, carry += W_fs^T dp1 + dhT.
 *   replaces what autograd derives for grin_cell.py:206-208 and SpatialDecoder.forward :86-90 */
int sgp_grin_stage1_bwd_f32(int32_t H, int32_t C, int32_t U, int64_t R, int64_t inner, int32_t S, int32_t t,
                            int32_t reverse, const float* packed, const float* mask, const float* dP1, const float* dcell,
                            int64_t cell_row_stride, const float* ddec, int64_t ddec_row_stride, float* carry, float* gx,
                            float* dp1, float* gu, sgp_stream_t stream);

/* ------------------------------------------------ DCRNN baseline: diffusion convolution and its GRU cell -----
 * dcrnn.hip.  EXACT-FP32 contract as above: v_mfma_f32_16x16x4_f32 in the matrix kernels, plain FMAs in CSR order in
 * the hop; no float atomics, bit-identical from run to run; no persistent kernel and no barrier between workgroups (a
 * hop that needs its neighbours' previous hop is the next launch in stream order).
 * The filters' input cat([x | h], A_f [x | h], .., A_b^k [x | h]) is kept as two "concat buffers" of 2 k + 1 slots:
 * the x side [S R, (2 k + 1) Fin] for all steps at once, whose product with the stacked x columns of the three
 * filters (one sgp_dense_f32 launch, biases folded in) is G [S R, 3 H] = (r | u | c); and the h side [R, (2 k + 1) H]
 * per step.  Slot 0 is the value itself, slots 1 .. k its A_f powers, k + 1 .. 2 k its A_b powers.
 * Domain: H a multiple of 16 in 16 .. 128, k >= 1; anything else returns SGP_EUNSUP with the reason in sgp_last_error
 * (sgp_dcrnn_supported answers without a GPU). */
int32_t sgp_dcrnn_supported(int32_t H, int32_t k);

/* One hop order of one or two supports (rowptr1 = NULL: one) given as CSR tables over n rows (int32 / fp32, columns in
 * [0, n)): for each support s, Y[b, i, ycol_s : ycol_s + feat] (= | += with accumulate) sum_e val_s[e] *
 * X[b, col_s[e], xcol_s : xcol_s + feat].  Strides in floats; X and Y may be the same allocation when the column
 * ranges read and written differ.  One wave owns a destination row and walks its supports in order, so two supports
 * may accumulate into the same destination columns.
 *   replaces one self.propagate(sup_index, x=x_sup, weight=sup_weights) per support of
 *   tsl/nn/layers/graph_convs/diff_conv.py:98-102 (message(), line 72, summed at the targets), and with the tables of
 *   the transposed supports what autograd derives for it */
int sgp_diffuse_f32(const int32_t* rowptr0, const int32_t* col0, const float* val0, int64_t xcol0, int64_t ycol0,
                    const int32_t* rowptr1, const int32_t* col1, const float* val1, int64_t xcol1, int64_t ycol1,
                    const float* X, int64_t x_row_stride, int64_t x_batch_stride,
                    float* Y, int64_t y_row_stride, int64_t y_batch_stride,
                    int32_t n, int32_t batch, int32_t feat, int32_t accumulate, sgp_stream_t stream);

/* [r | u] = sigmoid(Dh Wh_ru^T + G[:, 0 : 2 H]) over R rows; Dh [R, (2 k + 1) H] with h in slot 0; w_ru_packed:
 * sgp_dense_pack_f32 of the h columns of forget_gate and update_gate stacked, [2 H, (2 k + 1) H].  Stores r and u into
 * ruc [R, 3 H] (columns 0 .. 2 H) and r * h into slot 0 of Drh.
 *   replaces the h half of forget_gate / update_gate's filters, the sigmoids and r * h of
 *   tsl/nn/blocks/encoders/gcrnn.py:14-17 (filters: diff_conv.py:105) */
int sgp_dcrnn_gates_f32(const float* Dh, int64_t d_row_stride, const float* w_ru_packed,
                        const float* G, int64_t g_row_stride, float* ruc, int64_t ruc_row_stride,
                        float* Drh, int64_t drh_row_stride, int64_t R, int32_t H, int32_t k, sgp_stream_t stream);

/* c = tanh(Drh Wh_c^T + G[:, 2 H : 3 H]), h' = u h_prev + (1 - u) c.  c goes to ruc[:, 2 H : 3 H]; h' to h_seq_t
 * [R, H] (may be NULL), to the leading H columns of dh_next (slot 0 of the next step's Dh, may be NULL, may be the
 * buffer h_prev points into) and to h_last [R, H] (may be NULL).
 *   replaces the h half of candidate_gate's filters, the tanh and the state update of gcrnn.py:18-19 */
int sgp_dcrnn_update_f32(const float* Drh, int64_t d_row_stride, const float* w_c_packed,
                         const float* G, int64_t g_row_stride, float* ruc, int64_t ruc_row_stride,
                         const float* h_prev, int64_t h_row_stride, float* h_seq_t, float* dh_next,
                         int64_t dh_next_row_stride, float* h_last, int64_t R, int32_t H, int32_t k,
                         sgp_stream_t stream);

/* The elementwise half of one reversed step; dh [R, H] is the carried cotangent of h_t, updated in place; dz [R, 3 H]
 * = (dzr | dzu | dzc), the gradients of the pre-activations.
 *   phase 1: dzc = dh (1 - u)(1 - c^2), dzu = dh (h_prev - c) u (1 - u), dh <- dh u
 *   phase 2: with dDrh (slot 0 of the cotangent of Drh): dzr = dDrh h_prev r (1 - r), dh += dDrh r
 * ruc and dz may be the same allocation with the same row stride (dz then overwrites r | u | c in place): element
 * (row, col) of each of the three blocks is read and written by one thread, which loads all it needs before it stores.
 *   replaces what autograd derives for gcrnn.py:15-19 */
int sgp_dcrnn_bwd_f32(int32_t phase, float* dh, const float* ruc, int64_t ruc_row_stride,
                      const float* h_prev, int64_t h_row_stride, const float* dDrh, int64_t ddrh_row_stride,
                      float* dz, int64_t dz_row_stride, int64_t R, int32_t H, sgp_stream_t stream);

/* ------------------------------------------------ Graph WaveNet baseline: gated TCN, dense learned adjacency, norm -----
 * gwnet.hip.  EXACT-FP32 contract as above (v_mfma_f32_16x16x4_f32 in the matrix kernels), no float atomics, every sum
 * in one fixed order: bit-identical from run to run and independent of the row or batch item a value falls into.
 * Activations are time-major [S, M, H] (M = b n): tap j of the temporal convolution is the row offset j d M.
 * Domain of the model: H a multiple of 16 in 16 .. 128, Kt in 1 .. 4; anything else returns SGP_EUNSUP with the reason
 * in sgp_last_error (sgp_gwnet_supported answers without a GPU). */
int32_t sgp_gwnet_supported(int32_t H, int32_t Kt);

/* y[r] = tanh(a) * sigmoid(g), [a | g] = sum_j W_j x[r + j tap_rows] + bias for n_rows output rows; X has x_rows rows
 * (n_rows + (Kt - 1) tap_rows <= x_rows is checked).  w_packed: sgp_dense_pack_f32 of the conv weight [2 H, H, 1, Kt]
 * rearranged tap-major to [2 H, Kt H]; bias [2 H].  act (may be NULL): [n_rows, 2 H] = [tanh a | sigmoid g] for the
 * backward pass.  Row strides in floats, multiples of 4; buffers 16-byte aligned.
 *   replaces self.conv(x) of tsl/nn/base/temporal_conv.py:54 (Conv2d(H, 2 H, (1, Kt), dilation (1, d)), no padding:
 *   tsl/nn/blocks/encoders/tcn.py:60-68 with causal_padding False) and gated_tanh of temporal_conv.py:88 */
int sgp_gwnet_tconv_f32(const float* X, int64_t x_row_stride, int64_t x_rows, int64_t tap_rows,
                        const float* w_packed, const float* bias, float* Y, int64_t y_row_stride,
                        float* act, int64_t act_row_stride, int64_t n_rows, int32_t H, int32_t Kt,
                        sgp_stream_t stream);

/* dz = [dy s (1 - t^2) | dy t s (1 - s)] written over act = [t | s] of the forward pass (which therefore runs once).
 *   replaces what autograd derives for gated_tanh (temporal_conv.py:88); the convolution's own gradients are
 *   sgp_dense_wgrad_f32 / sgp_dense_f32 per tap on time-major slices */
int sgp_gwnet_tconv_bwd_f32(const float* dY, int64_t dy_row_stride, float* act, int64_t act_row_stride,
                            int64_t n_rows, int32_t H, sgp_stream_t stream);

/* Y[i, w, ycol : ycol + feat] (= | += with accumulate) sum_v A[w, v] X[i, v, xcol : xcol + feat] for every batch item i
 * (transpose: A[v, w]).  A: dense fp32 [n, n] with a row stride, shared by all items; X and Y may be column slots of one
 * concat buffer when the column ranges differ.  feat a multiple of 16; strides and column offsets multiples of 4.
 *   replaces torch.einsum('ncvl, wv -> ncwl', (x1, a)) of tsl/nn/layers/graph_convs/dense_spatial_conv.py:81, and with
 *   transpose what autograd derives for it with respect to x1 */
int sgp_adj_apply_f32(const float* A, int64_t a_row_stride, int32_t transpose,
                      const float* X, int64_t xcol, int64_t x_row_stride, int64_t x_batch_stride,
                      float* Y, int64_t ycol, int64_t y_row_stride, int64_t y_batch_stride,
                      int32_t n, int32_t batch, int32_t feat, int32_t accumulate, sgp_stream_t stream);

/* dA[w, v] (= | +=) sum_i sum_f dY[i, w, dycol + f] X[i, v, xcol + f], the items in order.  A small operator splits
 * the items into slices with one partial each (work, sgp_adj_grad_workspace_floats; 0: none needed), added in slice
 * order in fp64.
 *   replaces what autograd derives for dense_spatial_conv.py:81 with respect to a */
int64_t sgp_adj_grad_workspace_floats(int32_t n, int32_t batch);
int sgp_adj_grad_f32(const float* dY, int64_t dycol, int64_t dy_row_stride, int64_t dy_batch_stride,
                     const float* X, int64_t xcol, int64_t x_row_stride, int64_t x_batch_stride,
                     float* dA, int64_t da_row_stride, int32_t n, int32_t batch, int32_t feat, int32_t accumulate,
                     float* work, int64_t work_floats, sgp_stream_t stream);

/* A[r, :] = softmax(L[r, :]) with the row maximum subtracted; dL = A (dA - sum_j dA A) where L > 0, else 0 (the relu of
 * the logits folded into the backward pass; dL may be dA).
 *   replaces torch.softmax(logits, dim=1) of lib/nn/models/gwnet_model.py:12 and what autograd derives for lines 10-12 */
int sgp_row_softmax_f32(const float* L, int64_t l_row_stride, float* A, int64_t a_row_stride, int32_t n_rows, int32_t n,
                        sgp_stream_t stream);
int sgp_row_softmax_bwd_f32(const float* A, int64_t a_row_stride, const float* dA, int64_t da_row_stride,
                            const float* L, int64_t l_row_stride, float* dL, int64_t dl_row_stride,
                            int32_t n_rows, int32_t n, sgp_stream_t stream);

/* z = dropout(Y) + res (res may be NULL), out = norm(z) over R rows of H <= 256 columns.  kind 0: none; 1: batch
 * (training: statistics over all rows, biased variance, running buffers updated with the unbiased one; else the
 * running buffers); 2: layer, (z - mean) / (std + eps) with the population std, then the affine.  Dropout is the Philox
 * scheme of sgp_dense_f32 at index row * H + col.  z_save [R, H] (may be NULL) and stats (batch: mean | rstd | low part of the mean [3 H],
 * required; layer: (mean, 1 / (std + eps)) [R, 2], may be NULL) are what the backward pass reads.  work: batch
 * training only, sgp_gwnet_norm_workspace_doubles.
 *   replaces self.dropout(x), x + res[:, -x.size(1):] and norm(x) of graph_wavenet_model.py:157-160
 *   (tsl/nn/layers/norm/batch_norm.py:35-37, layer_norm.py:40-46) */
int64_t sgp_gwnet_norm_workspace_doubles(int64_t R, int32_t H);
int sgp_gwnet_norm_f32(int32_t kind, int32_t training, const float* Y, int64_t y_row_stride,
                       const float* res, int64_t res_row_stride, double dropout_p, uint64_t seed,
                       const float* weight, const float* bias, float* running_mean, float* running_var,
                       double momentum, double eps, float* z_save, float* stats,
                       float* out, int64_t out_row_stride, int64_t R, int32_t H,
                       double* work, int64_t work_doubles, sgp_stream_t stream);

/* dY = dz * keep, dRes = dz (may be NULL), dweight = column sums of dOut * xhat, dbias of dOut (fp64 over row slices,
 * slice order), with dz the cotangent of z.
 *   replaces what autograd derives for graph_wavenet_model.py:157-160 */
int sgp_gwnet_norm_bwd_f32(int32_t kind, int32_t training, const float* dOut, int64_t dout_row_stride,
                           const float* z, const float* stats, const float* weight, double dropout_p, uint64_t seed,
                           double eps, float* dY, int64_t dy_row_stride, float* dRes, int64_t dres_row_stride,
                           float* dweight, float* dbias, int64_t R, int32_t H,
                           double* work, int64_t work_doubles, sgp_stream_t stream);

/* ------------------------------------------- k-hop subgraph sampling ---
 * The batch construction of lib/dataloader/subgraph_dataloader.py on a device-resident int32 edge list.  Node sets
 * and flag arrays are BIT arrays in 64-bit words (bit i of word i / 64); bits at and beyond the stated length are
 * ignored.  Every size may be up to 2^31 - 1; all launches are grid-stride.  Ids outside [0, n_nodes) are never
 * followed: they are skipped, and where an `err` word is given it is set to 1 (it is never cleared here).
 *
 * sgp_subgraph_mark: set the bits of ids[0 .. n_ids) in mask (atomic OR; the caller cleared the mask).
 *   replaces `subsets = [node_idx]` / `node_mask[subsets[-1]] = True` of torch_geometric.utils.k_hop_subgraph, called
 *   at subgraph_dataloader.py:159 */
int sgp_subgraph_mark(const int32_t* ids, int64_t n_ids, uint64_t* mask, int64_t n_nodes, int32_t* err,
                      sgp_stream_t stream);
/* One hop: mask_out = mask_in | { dst[e] : src[e] in mask_in }.  mask_out is first overwritten with a copy of
 * mask_in; the two must be different buffers (a node reached in this hop must not expand in it).
 *   replaces one turn of `torch.index_select(node_mask, 0, row, out=edge_mask); subsets.append(col[edge_mask])` in
 *   k_hop_subgraph(flow='target_to_source') (subgraph_dataloader.py:159-161: row = edge_index[0], col = edge_index[1]) */
int sgp_subgraph_expand(const int32_t* src, const int32_t* dst, int64_t n_edges, const uint64_t* mask_in,
                        uint64_t* mask_out, int64_t n_nodes, sgp_stream_t stream);
/* flags bit e = mask[src[e]] & mask[dst[e]] (ceil(n_edges / 64) words, all written); edge_mask (may be NULL): the same
 * as one byte per edge, the `edge_mask` k_hop_subgraph returns.
 *   replaces `edge_mask = node_mask[row] & node_mask[col]` of k_hop_subgraph (subgraph_dataloader.py:159-162) */
int sgp_subgraph_edge_flags(const int32_t* src, const int32_t* dst, int64_t n_edges, const uint64_t* mask,
                            int64_t n_nodes, uint64_t* flags, uint8_t* edge_mask, sgp_stream_t stream);

/* Ordered compaction of an n-bit array: the indices of the set bits ascending, and each one's exclusive rank.
 * Three passes, no workgroup waits for another: sgp_compact_count writes the set bits of every tile of 16 384 flags to
 * tile_offsets[sgp_compact_tiles(n)], scans them in place (exclusive, one workgroup) and writes the number of set bits
 * to the device word `total`; sgp_compact_scatter then writes, for the r-th set bit i: idx32[r] = idx64[r] = i and
 * rank[i] = r (each may be NULL; idx* hold n_set entries, rank n, entries of clear bits untouched).  n_set is the total
 * the caller read back.  sgp_compact_pack_u8 turns one byte per flag (non-zero = set) into the bit array.
 *   replaces `torch.cat(subsets).unique(return_inverse=True)` and `node_idx[subset] = torch.arange(subset.size(0))` of
 *   k_hop_subgraph (sorted node ids, relabel table) and, on edge flags, the positions that `edge_index[:, edge_mask]`
 *   keeps (subgraph_dataloader.py:159-164) */
int64_t sgp_compact_tiles(int64_t n);
int sgp_compact_pack_u8(const uint8_t* flags, int64_t n, uint64_t* bits, sgp_stream_t stream);
int sgp_compact_count(const uint64_t* bits, int64_t n, int32_t* tile_offsets, int32_t* total, sgp_stream_t stream);
int sgp_compact_scatter(const uint64_t* bits, int64_t n, const int32_t* tile_offsets, int64_t n_set, int32_t* idx32,
                        int64_t* idx64, int32_t* rank, sgp_stream_t stream);
/* The compaction's scatter on edge flags, writing the edge itself: for the r-th surviving edge e
 *   out_src[r] = relabel[src[e]], out_dst[r] = relabel[dst[e]], out_weight[r] = weight[e] (weight pair may be NULL).
 *   replaces `edge_index = edge_index[:, edge_mask]; edge_index = node_idx[edge_index]` of k_hop_subgraph and
 *   `edge_weight = edge_weight[edge_mask]` (subgraph_dataloader.py:159-164) */
int sgp_subgraph_edges(const uint64_t* flags, int64_t n_edges, const int32_t* tile_offsets, int64_t n_set,
                       const int32_t* src, const int32_t* dst, const float* weight, const int32_t* relabel,
                       int64_t n_nodes, int64_t* out_src, int64_t* out_dst, float* out_weight, sgp_stream_t stream);
/* The edge cap: out[j] = edge pos[keep[j]], relabelled, j < n_keep, in keep's order.  pos [n_pos]: positions of the
 * surviving edges (sgp_compact_scatter's idx32; NULL: every edge, n_pos = n_edges); keep NULL: j itself; relabel NULL:
 * ids as they are.  A keep entry outside [0, n_pos) writes -1 and sets err.
 *   replaces `edge_index = edge_index[:, keep_edges]; edge_weight = edge_weight[keep_edges]`
 *   (subgraph_dataloader.py:184-186) */
int sgp_subgraph_take_edges(const int32_t* src, const int32_t* dst, const float* weight, int64_t n_edges,
                            const int32_t* pos, int64_t n_pos, const int64_t* keep, int64_t n_keep,
                            const int32_t* relabel, int64_t n_nodes, int64_t* out_src, int64_t* out_dst,
                            float* out_weight, int32_t* err, sgp_stream_t stream);

/* ------------------------------------------- graph construction ---
 * Row-wise selection over an N x N similarity that is either never formed (geographic) or given (dense).  Entry A[i, j]
 * of row i, column j.  `threshold`: entries whose value is below it are dropped (-inf: none); `binary`: kept values
 * become 1 (knn) or `sim > 0` (no knn); an entry whose value rounds to 0 in fp32 is no entry.  Values come out in fp64
 * (the caller rounds once, after its O(E) post-processing).
 *
 * knn entries: per row the k best candidates by (value descending, column ascending), the diagonal excluded unless
 * include_self.  out_col / out_val [n, k]: the row's kept entries; a slot whose entry was dropped holds value 0.
 * 1 <= k <= n; k above sgp_conn_max_knn() (512) is SGP_EUNSUP.
 *
 * rows entries (no knn): called twice.  With row_count [n] given: the number of entries of every row.  With row_count
 * NULL: rowptr [n + 1] (the caller's exclusive scan of the counts, int64) and out_col / out_val [rowptr[n]] receive the
 * rows, columns ascending.
 *
 * Geographic source: unit [3, n] fp64 unit vectors (x | y | z) of the nodes; the value of (i, j) is
 * exp(-(scale asin(min(1, |u_i - u_j| / 2)))^2) with scale = 2 R / theta, evaluated for kept entries only: knn selects
 * on min(|u_i - u_j|^2, chord_zero) (chord_zero: the squared chord from which the fp64 value is exactly 0, so those
 * tie), rows tests the squared chord against [chord_lo, chord_hi] (below: kept; above: dropped; inside: the value
 * itself is tested).
 *   replaces geographical_distance + gaussian_kernel (tsl/ops/similarities.py:58-101, lib/datasets/pv.py:88-95) and,
 *   for both sources, top_k (similarities.py:104-122), `adj[adj < threshold] = 0`, `fill_diagonal` and the non-zero
 *   scan of adj_to_edge_index / csr_matrix in get_connectivity (tsl/datasets/prototypes/dataset.py:411-433)
 * Dense source: sim [n, n] fp32 (is_f64 = 0) or fp64 with the given element strides; fp64 is compared as fp64. */
int32_t sgp_conn_max_knn(void);
int sgp_conn_geo_knn_f64(const double* unit, int64_t n, int32_t k, int32_t include_self, int32_t binary,
                         double threshold, double chord_zero, double scale, int32_t* out_col, double* out_val,
                         sgp_stream_t stream);
int sgp_conn_geo_rows_f64(const double* unit, int64_t n, int32_t include_self, int32_t binary, double threshold,
                          double chord_lo, double chord_hi, double scale, int32_t* row_count, const int64_t* rowptr,
                          int32_t* out_col, double* out_val, sgp_stream_t stream);
int sgp_conn_dense_knn(const void* sim, int32_t is_f64, int64_t row_stride, int64_t col_stride, int64_t n, int32_t k,
                       int32_t include_self, int32_t binary, double threshold, int32_t* out_col, double* out_val,
                       sgp_stream_t stream);
int sgp_conn_dense_rows(const void* sim, int32_t is_f64, int64_t row_stride, int64_t col_stride, int64_t n,
                        int32_t include_self, int32_t binary, double threshold, int32_t* row_count,
                        const int64_t* rowptr, int32_t* out_col, double* out_val, sgp_stream_t stream);
/* out[a, b] = mean over chunks c < n_chunks of exp(-gamma max(0, n_c[a] + n_c[b] - 2 <x_c[:, a], x_c[:, b]>)), chunk c =
 * rows [c period, (c + 1) period) of x [>= n_chunks period, n]; the diagonal is exactly 1.  The Gram tiles run on the
 * exact-fp32 matrix-core form; norms [n_chunks, n] is scratch (the chunks' squared column norms).
 *   replaces the `rbf_kernel(xi, gamma=gamma)` loop of CEREn.compute_similarity (lib/datasets/cer_en.py:153-164) */
int sgp_correntropy_f32(const float* x, int64_t x_row_stride, int32_t n, int32_t period, int32_t n_chunks, double gamma,
                        float* norms, float* out, int64_t out_row_stride, sgp_stream_t stream);

/* --------------------------------------------------------- scalers ---
 * Fits of tsl's StandardScaler / MinMaxScaler / RobustScaler and the fused transform.  x is a row-major fp32 [m, g]
 * matrix: m reduced rows, g groups (one bias / scale each).  mask: NULL or bytes (non-zero = counts), indexed as
 * flat_index / mask_div (mask_div divides g: 1 = a mask of x's shape, C = tsl's [T, N, 1] mask over C channels).  An
 * element counts iff its mask byte is set and it is not NaN.
 *
 * Launch regime (sgp_amd.scalers.launch_plan): regime 0 "long" (g <= 8): rows_per_wg rows per workgroup, fp64 partials
 * added by a second stage in a fixed order, global integer histograms; needs ws of sgp_scaler_workspace_bytes.
 * regime 1 "many": a workgroup owns tile_cols (16 | 32 | 64) adjacent columns, everything in LDS; ws may be NULL.
 *
 * moments: stats [6, g] fp64 = count | mean | sum of squared deviations from the mean (want_var; else 0) | min | max |
 *   1 where an unmasked NaN was seen.  Two passes (the second for want_var); no float atomics, fixed summation order.
 * select: exact order statistics ostat [g, 6] = the elements of rank floor / ceil of the virtual indices
 *   q / 100 * (count - 1) for q = q_lo, q_mid, q_hi (numpy's linear method), the count taken from stats on the device.
 *   Radix select on order-preserving keys: 4 passes of 8-bit digits (long) or 8 of 4-bit digits (many).
 * finish: kind 0 standard (bias = mean, scale = population std), 1 min-max (p0 < p1: the output range), 2 robust
 *   (p0, p1: the quantile range given to select, bias = median; adjust: 0 or the unit-variance divisor); fp64, rounded
 *   to fp32 once; |scale| <= 10 * 2^-23 becomes 1; an empty group, or without a mask (has_mask = 0) a group that held a
 *   NaN, gets bias = scale = NaN.  bias / scale: [g] fp32.
 * apply: out[i] = (x[i] - bias[i % n_params]) / scale[i % n_params] + 5e-8, or with `inverse`
 *   x[i] * (scale[..] + 5e-8) + bias[..]; unfused fp32 with IEEE division (bit-equal to torch's evaluation); out may
 *   be x.
 *   replaces Scaler.transform / inverse_transform and the numpy fits of tsl/data/preprocessing/scalers.py:114-283 */
int64_t sgp_scaler_workspace_bytes(int64_t m, int64_t g, int32_t regime, int64_t rows_per_wg);
int sgp_scaler_moments_f32(const float* x, const uint8_t* mask, int64_t mask_div, int64_t m, int64_t g, int32_t want_var,
                           int32_t regime, int64_t rows_per_wg, int32_t tile_cols, double* stats, void* ws,
                           int64_t ws_bytes, sgp_stream_t stream);
int sgp_scaler_select_f32(const float* x, const uint8_t* mask, int64_t mask_div, int64_t m, int64_t g, const double* stats,
                          double q_lo, double q_mid, double q_hi, int32_t regime, int64_t rows_per_wg, int32_t tile_cols,
                          float* ostat, void* ws, int64_t ws_bytes, sgp_stream_t stream);
int sgp_scaler_finish_f32(int32_t kind, const double* stats, const float* ostat, int64_t g, int32_t has_mask, double p0,
                          double p1, double adjust, float* bias, float* scale, sgp_stream_t stream);
int sgp_scaler_apply_f32(const float* x, float* out, const float* bias, const float* scale, int64_t n, int64_t n_params,
                         int32_t inverse, sgp_stream_t stream);

/* ------------------------------------------- per-batch edge tables ---
 * The tables every model derives from an edge list, built on the stream: a stable sort of the list by node, the
 * segment offsets, ordered degree sums, CSR gathers and the chunk tables of the gated graph network.  Edge endpoints
 * come as int32 (flag 0) or int64 (flag 1) and are narrowed on the device.  No workgroup waits for another; integer
 * arithmetic decides every position, so two runs give identical tables.
 *
 * sgp_edge_sort: LSD radix sort, 8-bit digits, sgp_edge_sort_passes(n_nodes) = max(1, ceil(bits(n_nodes - 1) / 8))
 *   passes of three launches (tile histogram, scan, scatter) over tiles of sgp_edge_sort_tile() items.  Item i of the
 *   list has the key keys[i], or keys[payload_in[i]] when payload_in is given (n_keys entries behind keys; the second
 *   sort of an already sorted list: edge_plan's src_pos).  order[n_items]: the positions of the stable sort,
 *   torch.sort(list, stable=True)[1]; ptr[n_nodes + 1]: the segment offsets, cumsum(bincount(list)), found from the
 *   key boundaries of the sorted list.  A key outside [0, n_nodes) or a payload_in entry outside [0, n_keys) is
 *   compared unsigned before it indexes anything, sets *err = 1 (the caller cleared it) and is dropped: ptr then
 *   describes the remaining items and the tail of order is not written.  ws: sgp_edge_sort_workspace_bytes(n_items)
 *   bytes (a pure function of n_items; sgp_amd.edgetables.sort_plan computes the same number).
 *   replaces the stable torch.sort / bincount / cumsum of gated_gn.edge_plan and diff_conv._csr
 * sgp_edge_segment_sum_f32: deg[k] = weight[order[ptr[k]]] + ... + weight[order[ptr[k + 1] - 1]] added one after the
 *   other from 0 in fp32 (weight NULL: ones) -- the host's scatter_add_ in edge order, bit for bit, because the sort
 *   is stable.  One thread per segment: a hub row is slow and correct.
 *   replaces the host-side scatter_add_ of diff_conv.diffusion_plan (tsl/ops/connectivity.py:200-227)
 * sgp_edge_gather_f32: with o = order[e]: col[e] = other[o], val_a[e] = weight[o] / deg_a[idx_a[o]], val_b likewise
 *   (IEEE division; weight NULL: ones; deg_x NULL: val_x[e] = weight[o]; col, val_a, val_b may each be NULL).  An o
 *   outside the list gives 0.
 * sgp_edge_chunk_tables: from ptr (the target sort) and chunk, edge_plan's chunks[C][4] = (target, first, end, partial
 *   row or -1) and fix[F][3] = (target, first partial row, count), and counts[0 .. 3) = (C, F, n_parts).  scan: 3 *
 *   n_nodes int32 of scratch.  Rows at and beyond max_chunks / max_fix are not written (C <= n_nodes + n_edges /
 *   chunk, F <= n_edges / chunk).  The caller keeps the sort's err word at counts[3]: one host read returns all four. */
int32_t sgp_edge_sort_tile(void);
int32_t sgp_edge_sort_passes(int64_t n_nodes);
int64_t sgp_edge_sort_workspace_bytes(int64_t n_items);
int sgp_edge_sort(const void* keys, int32_t keys64, int64_t n_keys, const int32_t* payload_in, int64_t n_items,
                  int64_t n_nodes, int32_t* order, int32_t* ptr, int32_t* err, void* ws, int64_t ws_bytes,
                  sgp_stream_t stream);
int sgp_edge_segment_sum_f32(const int32_t* ptr, const int32_t* order, const float* weight, int64_t n_nodes,
                             int64_t n_items, float* deg, sgp_stream_t stream);
int sgp_edge_gather_f32(const int32_t* order, int64_t n_items, const void* other, int32_t other64, const float* weight,
                        const void* idx_a, const float* deg_a, const void* idx_b, const float* deg_b, int32_t idx64,
                        int64_t n_nodes, int32_t* col, float* val_a, float* val_b, sgp_stream_t stream);
int sgp_edge_chunk_tables(const int32_t* ptr, int64_t n_nodes, int32_t chunk, int32_t* scan, int32_t* counts,
                          int32_t* chunks, int64_t max_chunks, int32_t* fix, int64_t max_fix, sgp_stream_t stream);

/* ------------------------------------- graph-shift operator from an edge list ---
 * The normalised operator of SGP's spatial embedding, built on the stream from a device-resident edge list, bit for
 * bit what sgp_amd.graph.ShiftOperator.from_edges builds on the host (shift_operator.hip).  A[i, j] is the weight of
 * edge j -> i: row = dst, column = src; SGP_SHIFT_TRANSPOSE swaps them; SGP_SHIFT_UNDIRECTED appends the swapped list
 * behind the original one (n_items = 2 n_edges, else n_edges).  The items are sorted stably by (row, column) with two
 * chained sgp_edge_sort passes (by column, then by row through the first order); a run of equal (row, column) becomes
 * one entry whose value is +0.0f + w_1 + w_2 + ... in list order (weight NULL: ones), added by the head of the run;
 * the positions come from a scan of the head flags (tile counts, one scan over the tiles, a scan inside each tile).
 * SGP_SHIFT_SET_DIAG / SGP_SHIFT_REMOVE_DIAG drop the coalesced entries with row == column; SET_DIAG (it wins) gives
 * every row one diagonal entry of value 1 at its sorted column position.  deg[i] = the fp32 sum of row i's values in
 * column order from +0.0f; d = 1 / deg, or 1 / sqrt(deg) with SGP_SHIFT_GCN_NORM (correctly rounded division and
 * square root; +inf becomes 0, NaN stays); val = d[row] * val, then * d[column] with GCN_NORM, in that order.
 *
 * Outputs: rowptr[n_nodes + 1], col / val of `capacity` >= n_items + (SET_DIAG ? n_nodes : 0) entries, of which the
 * first rowptr[n_nodes] are written, *nnz = rowptr[n_nodes], and *err = 1 (the caller cleared it) for an endpoint
 * outside [0, n_nodes): such an edge is dropped before it indexes anything and nothing is written outside the buffers.
 * ws: sgp_shift_operator_workspace_bytes(n_items, n_nodes) bytes.  No host read, no workgroup waits for another.
 *   replaces to_undirected / SparseTensor(...).set_diag / remove_diag / the degree normalisation of preprocess_adj
 *   (lib/sgp_preprocessing.py:67-105) and of sgp_spatial_embedding (:177-192, :205-216) */
#define SGP_SHIFT_GCN_NORM    1
#define SGP_SHIFT_SET_DIAG    2
#define SGP_SHIFT_REMOVE_DIAG 4
#define SGP_SHIFT_UNDIRECTED  8
#define SGP_SHIFT_TRANSPOSE   16
int64_t sgp_shift_operator_workspace_bytes(int64_t n_items, int64_t n_nodes);
int sgp_shift_operator_f32(const void* src, const void* dst, int32_t idx64, const float* weight, int64_t n_edges,
                           int64_t n_nodes, int32_t flags, int32_t* rowptr, int32_t* col, float* val, int64_t capacity,
                           int32_t* nnz, int32_t* err, void* ws, int64_t ws_bytes, sgp_stream_t stream);

/* ------------------------------------- product and row subset of CSR operators ---
 * The explicit supports of SGP's on-the-fly path for operators that live on the device (spgemm.hip).  An operand is
 * CSR as sgp_shift_operator_f32 leaves it: rowptr int32 [rows + 1], col int32 / val fp32 of `capacity` >= 1 entries of
 * which the first rowptr[rows] count, columns ascending and unique within a row.
 *
 * sgp_spgemm_f32: C = A B for A [n_rows, n_mid] and B [n_mid, n_cols] (A and B may be the same arrays), bit for bit
 *   scipy's fp32 product with sorted indices: C[i, j] = +0.0f + a[i, k1] b[k1, j] + a[i, k2] b[k2, j] + ... in
 *   ascending k, one fp32 multiply and one fp32 add per term (no fused multiply-add); columns ascending within a row;
 *   an entry whose sum compares equal to zero (either sign) is absent, NaN stays.  One wave per output row keeps a
 *   band of sgp_spgemm_form's width of columns as fp32 sums and touched flags in LDS, walks row i of A in order with
 *   the lanes striding over the rows of B, and scans the flags; columns beyond the band follow in further bands (only
 *   bands that hold an entry are walked).  A hub row is slow and correct.
 *   phase: SGP_SPGEMM_COUNT counts the entries of every row into ws, SGP_SPGEMM_EMIT scans the counts (one workgroup,
 *   64-bit sums) into rowptr and writes col / val; both bits: one call.  COUNT alone also scans (against a capacity of
 *   2^31 - 1) and so leaves the exact size in *nnz for a caller that allocates between the two phases; EMIT alone
 *   needs the ws of a COUNT call on the same operands.
 *     replaces the scipy SpGEMM of sgp_spatial_support (lib/sgp_preprocessing.py:143-145)
 * sgp_csr_take_rows_f32: row t of the result is row index[t] of A (index int32 / int64 by idx64, unsorted, repeats
 *   allowed), n_index rows, A's columns: row lengths, the same scan, a copy by one wave per row.  Same phases.
 *     replaces adj.index_select(0, node_index) (lib/datasets/iid_dataset.py:111-114; the product at
 *     lib/sgp_preprocessing.py:143-145 is applied to these rows)
 * Outputs of both: rowptr [rows + 1], the first rowptr[rows] entries of col / val, *nnz = rowptr[rows], and *err (the
 * caller cleared it; bits are OR-ed in).  SGP_SPGEMM_ERR_CAPACITY: the result has more than `capacity` (or 2^31 - 1)
 * entries; rowptr is then clamped to the capacity -- monotone, the rows that fit are complete, the rest cut short.
 * SGP_SPGEMM_ERR_INDEX: a rowptr entry of an operand outside [0, capacity] or decreasing, a column of A outside
 * [0, n_mid), a column of B outside [0, n_cols), an index outside [0, n_rows): compared unsigned before it indexes
 * anything, then skipped (an empty row).  Nothing is written outside the buffers.  ws: sgp_spgemm_workspace_bytes(rows
 * of the result) bytes.  No host read, no workgroup waits for another.
 * sgp_spgemm_form (host only): out[0] = the band width, out[1] = the bands that cover n_cols, out[2] = the regime:
 *   0 nothing to do, 1 one band, 2 banded; out[3] = workgroups (one wave each). */
#define SGP_SPGEMM_COUNT 1
#define SGP_SPGEMM_EMIT  2
#define SGP_SPGEMM_ERR_CAPACITY 1
#define SGP_SPGEMM_ERR_INDEX    2
int64_t sgp_spgemm_workspace_bytes(int64_t n_rows);
int sgp_spgemm_form(int64_t n_rows, int64_t n_cols, int64_t* out);
int sgp_spgemm_f32(const int32_t* a_rowptr, const int32_t* a_col, const float* a_val, int64_t a_capacity, int64_t n_rows,
                   int64_t n_mid, const int32_t* b_rowptr, const int32_t* b_col, const float* b_val, int64_t b_capacity,
                   int64_t n_cols, int32_t phase, int32_t* rowptr, int32_t* col, float* val, int64_t capacity,
                   int32_t* nnz, int32_t* err, void* ws, int64_t ws_bytes, sgp_stream_t stream);
int sgp_csr_take_rows_f32(const int32_t* a_rowptr, const int32_t* a_col, const float* a_val, int64_t a_capacity,
                          int64_t n_rows, const void* index, int32_t idx64, int64_t n_index, int32_t phase,
                          int32_t* rowptr, int32_t* col, float* val, int64_t capacity, int32_t* nnz, int32_t* err, void* ws,
                          int64_t ws_bytes, sgp_stream_t stream);

/* ------------------------------------- AZ-whiteness test of residuals ---
 * The integer core of tsl's az_whiteness_test (whiteness.hip).  x is an fp32 series [steps, nodes, feat] with unit
 * feature stride and the given step / node strides (in elements); mask: NULL (all valid) or bytes of the same shape
 * with strides of their own (non-zero = valid).  A masked-out entry is never looked at; a NaN / inf under a valid one
 * is counted into *nonfinite.  The prepared edge list (edge_u < edge_v, int32, sorted) comes from
 * sgp_amd.whiteness.prepare_graph; an endpoint outside [0, nodes) is compared unsigned and skipped.  Every sum is an
 * int64 that the entries ADD to (the caller zeroes the state once; consecutive time chunks accumulate); integer
 * atomics only, so the state does not depend on the launch shape or the run.
 *
 * sgp_az_pack_f32: planes [3, feat, nodes, words] uint64, words = ceil(steps / 64): bit b of word w describes step
 *   64 w + b: plane 0 negative (the sign bit), 1 non-zero and valid, 2 valid; the high bits of a ragged last word are
 *   zero.  The same launch adds the temporal sums st[f] = sum sgn(x[t] x[t - 1]) and mt[f] = #{both valid} over the
 *   pairs inside the chunk (each word against itself shifted by one bit, the bit shifted in being the step below the
 *   word) and, with carry_in, the pair across the chunk boundary.  carry_in / carry_out: NULL or [nodes * feat] bytes,
 *   bit 0 | 1 | 2 = the three planes' bit of the step before this chunk / of its last step (two different buffers).
 * sgp_az_edge_counts: s[e, f] += sum_t sgn(x[t, u, f] x[t, v, f]) = popc(nz) - 2 popc((neg_u ^ neg_v) & nz) with
 *   nz = nz_u & nz_v, and m[e, f] += popc(valid_u & valid_v), over the `words` words of the planes.  regime 0 "words":
 *   a wave per (edge, feature), lanes along the words; regime 1 "edges": a lane per (feature, edge) walks its words
 *   (sgp_amd.whiteness.launch_plan chooses).
 * sgp_az_direct_f32: the general form, no planes.  multivariate != 0: s[e] += sum_t sgn(sum_f x[t, u, f] x[t, v, f])
 *   with masked-out entries as 0, the dot product in fp64 (f ascending; fp32 products are exact there), m[e] += #{t:
 *   some feature of u and some feature of v valid}, st[0] / mt[0] likewise over (t - 1, t) with mt counting valid
 *   pairs over the features as well (the reference's count).  multivariate == 0: one test per feature, s / m
 *   [n_edges, feat], st / mt [feat]: the integers of the bit-plane path.  A lane owns an edge (edge, feature) over a
 *   slab of `slab` steps; node tiles behind the edge tiles take the temporal pairs.  prev_x [nodes, feat] fp32 /
 *   prev_mask bytes (contiguous): the step before this chunk, or NULL.
 * sgp_az_finish: rec [n_tests, 5] fp64 = Ct_s = sum_e w_e s[e, k] | W_s = sum_e w_e^2 m[e, k] | st[k] | mt[k] |
 *   *nonfinite, the fp64 sums in one fixed order (thread-strided partials, then a halving tree).  The host reads rec
 *   once and forms the statistic.
 *   replaces az_whiteness_test / _az_whiteness_test (tsl/ops/test.py:81-288) */
int sgp_az_pack_f32(const float* x, int64_t x_step_stride, int64_t x_node_stride, const uint8_t* mask,
                    int64_t mask_step_stride, int64_t mask_node_stride, int64_t steps, int64_t nodes, int32_t feat,
                    const uint8_t* carry_in, uint8_t* carry_out, uint64_t* planes, int64_t* st, int64_t* mt,
                    int64_t* nonfinite, sgp_stream_t stream);
int sgp_az_edge_counts(const uint64_t* planes, const int32_t* edge_u, const int32_t* edge_v, int64_t n_edges, int64_t nodes,
                       int32_t feat, int64_t words, int32_t regime, int64_t* s, int64_t* m, sgp_stream_t stream);
int sgp_az_direct_f32(const float* x, int64_t x_step_stride, int64_t x_node_stride, const uint8_t* mask,
                      int64_t mask_step_stride, int64_t mask_node_stride, const float* prev_x, const uint8_t* prev_mask,
                      int64_t steps, int64_t nodes, int32_t feat, int32_t multivariate, const int32_t* edge_u,
                      const int32_t* edge_v, int64_t n_edges, int32_t slab, int64_t* s, int64_t* m, int64_t* st, int64_t* mt,
                      int64_t* nonfinite, sgp_stream_t stream);
int sgp_az_finish(const int64_t* s, const int64_t* m, const double* weight, int64_t n_edges, int32_t n_tests,
                  const int64_t* st, const int64_t* mt, const int64_t* nonfinite, double* rec, sgp_stream_t stream);

/* ------------------------------------- preparing a raw series ---
 * The arithmetic between a dataset reader and the window data module (series.hip): temporal resampling, node groups
 * and time encodings of an fp32 series.  Every tensor is contiguous.  A NaN in the source is skipped by every
 * operation, as pandas' skipna=True skips it: sum = the sum of the others (0 if there are none), mean = that sum over
 * their count, min / max over the others, and NaN for mean / min / max where nothing is left.  Sums are accumulated in
 * fp64 in row (node) order and rounded to fp32 once; the mean is divided in fp64 by the count and then rounded.  All
 * offsets are 64-bit: rows x cols beyond 2^31 elements is served by construction.
 *
 * sgp_series_resample_f32: x [rows, cols] (cols = nodes x feat), bin_ptr [bins + 1] int32: bin b holds the source rows
 *   bin_ptr[b] .. bin_ptr[b + 1] - 1 (the rows are sorted by time, so a bin is a row range; entries are clamped to
 *   [0, rows] before they index anything).  y [bins, cols] = op over the bin's rows, one thread per output element
 *   walking its rows in order.  An empty bin gives 0 (sum) or NaN (mean, min, max).  op SGP_SERIES_TAKE: y[b] = row
 *   src_row[b] of x (int32 [bins]; outside [0, rows), -1 by convention: NaN) -- asfreq and `nearest`, whose row choice
 *   is host work; bin_ptr is then read for the mask only and may be NULL without one.
 *   mask: NULL, or bytes [rows, cols] (mask_per_node == 0) or [rows, cols / feat] (mask_per_node != 0); mask_out has
 *   the same columns and `bins` rows: (double) valid / (double) count >= 1.0 - mask_tol over the bin's rows, compared in
 *   fp64; an empty bin is invalid.  The aggregation of x does not read the mask.
 *   flags SGP_SERIES_NAN_TO_MASK (op TAKE, no mask): mask_out [bins, cols] = the value is not NaN, and a NaN is stored
 *   as 0 (CEREn.load's mask = ~isnan, fillna(0)).
 *     replaces PandasDataset.resample_ (tsl/datasets/prototypes/pd_dataset.py:117-150) and df.asfreq in CEREn.load
 *     (lib/datasets/cer_en.py:120-124)
 * sgp_series_group_f32: x [steps, nodes, feat], groups as a CSR over the nodes: grp_ptr [groups + 1], grp_node [nodes]
 *   int32 (ascending within a group; pointers are clamped to [0, nodes], a node id outside [0, nodes) is skipped).
 *   y [steps, groups, feat] = op over the group's nodes (SUM .. MAX); mask / mask_out as above with [steps, nodes(,
 *   feat)] -> [steps, groups(, feat)].  regime 0: a thread per output walks its group in node order; regime 1: a
 *   workgroup per (step, group), thread k takes the group's nodes k, k + 256, .. in order into fp64 partials and wg.h's
 *   halving tree folds the 256 partials.  Both orders are fixed: the result does not change from run to run (it may
 *   differ between the regimes in the last bit of a sum).  sgp_amd.series.launch_plan chooses.
 *     replaces TabularDataset.aggregate_ (tsl/datasets/prototypes/tabular_dataset.py:329-375; CEREn.aggregate,
 *     cluster_'s aggregation step)
 * sgp_datetime_encode_f32: out [steps, 2 units] = sin | cos of 2 pi r / period per unit with r = index_ns mod
 *   period_ns reduced in int64 (floored: 0 <= r < period, also before 1970), the angle and sin / cos in fp64, rounded
 *   once.  period_ns [units] int64, each positive.
 *     replaces TemporalFeaturesMixin.datetime_encoded (tsl/datasets/prototypes/mixin.py:97-115), whose fp64 product
 *     index_nano * (2 pi / period) carries ~1e-11 of argument error at present-day timestamps */
#define SGP_SERIES_SUM  0
#define SGP_SERIES_MEAN 1
#define SGP_SERIES_MIN  2
#define SGP_SERIES_MAX  3
#define SGP_SERIES_TAKE 4
#define SGP_SERIES_NAN_TO_MASK 1
int sgp_series_resample_f32(const float* x, int64_t rows, int64_t cols, int32_t feat, const uint8_t* mask,
                            int32_t mask_per_node, const int32_t* bin_ptr, const int32_t* src_row, int64_t bins, int32_t op,
                            int32_t flags, double mask_tol, float* y, uint8_t* mask_out, sgp_stream_t stream);
int sgp_series_group_f32(const float* x, int64_t steps, int64_t nodes, int32_t feat, const uint8_t* mask,
                         int32_t mask_per_node, const int32_t* grp_ptr, const int32_t* grp_node, int64_t groups, int32_t op,
                         int32_t regime, double mask_tol, float* y, uint8_t* mask_out, sgp_stream_t stream);
int sgp_datetime_encode_f32(const int64_t* index_ns, int64_t steps, const int64_t* period_ns, int32_t units, float* out,
                            sgp_stream_t stream);

/* ------------------------------------------------------------ Attention -----
 * Multi-head scaled dot-product attention, forward and backward (attention.hip).  EXACT-FP32 contract as
 * the decoder section: every product is a v_mfma_f32_16x16x4_f32, no 16-bit operand, softmax statistics in fp32 with
 * the row maximum subtracted and the library's exp.
 *
 * For every sequence s < n_seq and head h < heads: O = softmax(Q K^T / sqrt(d) + mask) V over L tokens.  Q, K, V, O
 * (and dO, dQ, dK, dV) are separate pointers with their own row strides in floats, so they may be column ranges of one
 * [rows, 3 heads d] projection buffer; head h owns columns [h d, (h + 1) d).  Token t of sequence s is row
 *     (s / inner) * outer_rows + (s % inner) * inner_rows + t * tok_rows
 * of every operand: attention over the steps and over the nodes of a [b, s, n, .] tensor read the rows where they lie.
 * causal = 1: key j is visible to query i iff j <= i.  Only the queries q_first .. L - 1 are computed: the forward
 * leaves the rows below q_first of O untouched, the backward ignores those rows of dO and writes zeros to those of dQ
 * (dK, dV cover every key).  lse [n_seq, heads, L] (forward: may be NULL) is the log-sum-exp of a query's scaled
 * scores; the backward recomputes the probabilities from it.  work: sgp_attention_workspace_bytes (the row sums of
 * dO * O).  No float atomics: every output tile has one owner and sums run in tile order, so results are bit-identical
 * from run to run and a sequence computed alone has the bits it has in a batch.
 *
 * Domain: d a multiple of 8 in 8 .. 128, heads * d <= 256, L >= 1 (no upper bound: keys are streamed with the online
 * softmax), n_seq >= 1 with n_seq * heads * ceil(L / 16) < 2^31, 0 <= q_first < L; outside it SGP_EUNSUP with the
 * reason.  Pointers 16-byte aligned, row strides multiples of 4 (SGP_EINVAL otherwise).
 * sgp_attention_plan (host only; the entries dispatch on the same answer) fills plan[8]:
 *   [0] form = channel tiles a wave's registers are built for: 1 (d <= 16), 2 (d <= 32), 4 (d <= 64), 8 (d <= 128)
 *   [1] ceil(d / 16)   [2] query tiles ceil((L - q_first) / 16)   [3] key tiles ceil(L / 16)   [4] waves per workgroup
 *   [5] workgroups of the forward and of the dQ pass   [6] workgroups of the dK / dV pass   [7] 0
 *   replaces F.multi_head_attention_forward's bmm / softmax / bmm called by nn.MultiheadAttention.forward under
 *   tsl/nn/base/attention/attention.py:131-137 (with the causal mask of lines 14-19 and 125-130 and the rearranges of
 *   lines 122-123 and 138), and what autograd derives for them */
int sgp_attention_plan(int32_t L, int32_t d, int32_t heads, int64_t n_seq, int32_t causal, int32_t q_first, int32_t* plan);
int64_t sgp_attention_workspace_bytes(int32_t L, int32_t heads, int64_t n_seq);
int sgp_attention_fwd_f32(const float* Q, int64_t q_row_stride, const float* K, int64_t k_row_stride,
                          const float* V, int64_t v_row_stride, float* O, int64_t o_row_stride, float* lse,
                          int32_t L, int32_t d, int32_t heads, int64_t n_seq,
                          int64_t inner, int64_t outer_rows, int64_t inner_rows, int64_t tok_rows,
                          int32_t causal, int32_t q_first, sgp_stream_t stream);
int sgp_attention_bwd_f32(const float* dO, int64_t do_row_stride, const float* Q, int64_t q_row_stride,
                          const float* K, int64_t k_row_stride, const float* V, int64_t v_row_stride,
                          const float* O, int64_t o_row_stride, const float* lse,
                          float* dQ, int64_t dq_row_stride, float* dK, int64_t dk_row_stride,
                          float* dV, int64_t dv_row_stride, void* work, int64_t work_bytes,
                          int32_t L, int32_t d, int32_t heads, int64_t n_seq,
                          int64_t inner, int64_t outer_rows, int64_t inner_rows, int64_t tok_rows,
                          int32_t causal, int32_t q_first, sgp_stream_t stream);

/* -------------------------------------------------------------- Timing -----
 * HIP-event helpers so that Python can time kernels on the stream they were
 * launched on without importing a HIP binding. */
int sgp_event_create(void** ev);
int sgp_event_destroy(void* ev);
int sgp_event_record(void* ev, sgp_stream_t stream);
int sgp_event_elapsed_ms(void* start, void* stop, float* ms); /* synchronises on stop */

#ifdef __cplusplus
}
#endif
#endif /* SGP_AMD_H */
