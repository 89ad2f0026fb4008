/*
 * sassd.h -- C ABI of the MI355X-native SA-SSD hot path (libsassd.so, gfx950 only).
 *
 * This is the drop-in boundary.  Every entry point replaces one operator surface of the reference
 * (skyhehe123/SA-SSD; file:line relative to /root/reference) -- the reference binds those through pybind11 /
 * numba / the spconv Python package; a maintainer binds these through ctypes.
 *
 * Conventions
 *   - plain C types only: device pointers, sizes, a `void* stream` that is a hipStream_t (NULL = default).
 *   - return 0 on success, negative SASSD_E* otherwise.  No function allocates, frees or synchronises:
 *     the caller owns every buffer (use the *_workspace_bytes queries) and every count that is data
 *     dependent lives in DEVICE memory (int32 scalars), so a whole frame is a fixed launch sequence
 *     (hipGraph-capturable).  The reference, by contrast, exit()s on CUDA errors (iou3d.cpp:13-21) and
 *     syncs on every boolean index (ssd_rotate_head.py:336-356).
 *   - "cap" arguments are row capacities of caller buffers; if a device count exceeds its capacity the
 *     kernel clamps, and sets bit i of the int32 at `status` (see SASSD_ST_*) when a status pointer is given.
 *   - all floating point is IEEE fp32; all index math int32 (linear voxel indices must fit 2^32-2).
 */
#ifndef SASSD_H
#define SASSD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SASSD_OK       0
#define SASSD_EINVAL  -1   /* bad argument / unsupported configuration   */
#define SASSD_ENOSPC  -2   /* caller workspace or capacity too small     */
#define SASSD_EHIP    -3   /* HIP runtime / launch error (sassd_last_hip_error) */

#define SASSD_ST_VOXEL_OVERFLOW   1   /* more rows than an output capacity      */
#define SASSD_ST_HASH_FULL        2   /* hash table probe exhausted             */
#define SASSD_ST_BOX_OVERFLOW     4   /* more candidate boxes than capK / capD  */
#define SASSD_ST_GRID_SYNC        8   /* an in-launch grid barrier timed out (persistent rulebook pyramid) */
#define SASSD_ST_POINT_OVERFLOW  16   /* more points than a point capacity (sassd_crop_polytope_dev, sassd_merge_sweeps_dev) */

#define SASSD_MAX_POINTS_PER_VOXEL 64  /* max_points supported by sassd_voxelize (reference default: 35) */

const char *sassd_version(void);
int sassd_last_hip_error(void);
const char *sassd_last_hip_error_string(void);

/* Kernel selection is PER CALL (round 6; rounds 1-5 had process-wide sassd_debug_set_* switches, which a hipGraph capture
 * could bake in by accident -- none is left): the sparse-conv and Winograd entry points take an `int cfg`, 0 in production; the
 * direct and the bf16 convolution have `_cfg` twins of their entry points for their ablation switches.
 *   sparse conv (sassd_spconv_fwd / _bwd_data / _bwd_weight)   low 16 bits = ablation flags (tools/ablate_spconv.py): bit2 no
 *     MFMA, bit5 every gather reads row 0 (weight gradient: the tile-per-wave formulation), bit6 one weight image for every
 *     offset (bits 5 / 6 keep the number of loads in flight unchanged), bit8 the register-stationary kernel everywhere.
 *     Bits 16+: workgroup geometry -- 0 the per-shape, per-capacity default; 1 / 5 = spconv_gs_kernel on 4 / 8 waves, 8 / 9 =
 *     the balanced kernel spconv_gq_kernel with 4x4x1 quads / 16x16x4 tiles (the four the default picks from), 10 = the
 *     round-3 default (1 or 5 by capacity) for every layer; any other value returns SASSD_EINVAL.
 *   Winograd (sassd_conv2d_wino4_fwd / _chain, sassd_conv1x1_gemm_fwd)   bits 0-7 = GEMM geometry: 0 split operands on the
 *     bf16 MFMA, 128 x 128 workgroups (default); 1 = the fp32 MFMA (v_mfma_f32_32x32x2_f32) at its picked width; 2..6 = fp32
 *     MFMA with 32 cfg tile columns; 11..14 = split with other workgroup shapes (12 = the 128 x 128 workgroup by number); 15 /
 *     16 = split, 256 channels x 192 / 256 columns per workgroup on 128-row wave tiles.  All split geometries give bit-identical
 *     results.  Bits 8+: bit0 stage only the first chunk,
 *     bit1 no MFMA (fp32 geometries), bit2 no split arithmetic, bits 4 / 5 / 6 / 7 skip the input transform / GEMM / output
 *     transform / fused transform (per-kernel timing on live buffers, bench.py).  Chained calls must agree on the geometry.
 * The Python binding reads SASSD_SPCONV_DEBUG / SASSD_WINO4_CFG once as the DEFAULT cfg its wrappers pass. */

/* hipGraph capture of a launch sequence issued through this ABI (the reference has no counterpart: its frame is
 * ~10^2 host-issued launches with >= 6 host syncs).  begin -> any sassd_* calls on `stream` (streams
 * joined to it through events are captured too) -> end returns an executable graph; launch replays it. */
int sassd_graph_begin(void *stream);
int sassd_graph_end(void *stream, void **graph_exec);
int sassd_graph_launch(void *graph_exec, void *stream);
int sassd_graph_destroy(void *graph_exec);

/* ------------------------------------------------------------------------------------------------
 * (a1+a2) Hard voxelisation + per-voxel mean.
 * Replaces mmdet/ops/points_op/points_ops.py:104-164 `points_to_voxel` (numba kernel :5-50, zyx order) and
 * mmdet/models/backbones/vxnet.py:110-116 `SimpleVoxel.forward`.  Bit-exact with the serial reference:
 * voxels in first-touch order, <= max_points points per voxel in arrival order, the max_voxels `break`.
 *   points      [n_points, ndim] f32 (ndim >= 3; xyz first)            device
 *   voxel_size  3 f32, coors_range 6 f32                               HOST
 *   voxels      [cap, max_points, ndim] f32 zero padded, or NULL
 *   coors       [cap, coors_cols] i32; coors_cols 3 -> (z,y,x); 4 -> (batch_idx,z,y,x)
 *   num_points  [cap] i32, or NULL
 *   mean        [cap, nfeat] f32 (nfeat <= ndim), or NULL
 *   row_offset  device int32[2] or NULL: rows are written starting at row_offset[0] (0 if NULL) and
 *               row_offset[1] = row_offset[0] + voxel_num is written back (batch concatenation,
 *               detectors/single_stage.py:52-73 merge_second_batch).
 *   voxel_num   device int32 scalar: number of voxels of THIS cloud
 *   workspace   16-byte aligned (its tables are cleared by 16-byte stores; SASSD_EINVAL otherwise)
 * ---------------------------------------------------------------------------------------------- */
size_t sassd_voxelize_workspace_bytes(int n_points, int max_points);
int sassd_voxelize(const float *points, int n_points, int ndim, const float *voxel_size,
                   const float *coors_range, int max_points, int max_voxels, int batch_idx,
                   float *voxels, int32_t *coors, int coors_cols, int32_t *num_points, float *mean,
                   int nfeat, int32_t *row_offset, int32_t *voxel_num, int cap, int32_t *status,
                   void *workspace, size_t workspace_bytes, void *stream);

/* The same with the point count in DEVICE memory: `points` has room for points_cap rows, min(*n_points_dev, points_cap)
 * of them are valid.  The launch sequence depends on points_cap only, so a frame that starts at the raw point cloud
 * can be captured in a hipGraph and replayed for clouds of any size (workspace: sassd_voxelize_workspace_bytes(points_cap, ..)). */
int sassd_voxelize_dev(const float *points, int points_cap, const int32_t *n_points_dev, int ndim,
                       const float *voxel_size, const float *coors_range, int max_points, int max_voxels,
                       int batch_idx, float *voxels, int32_t *coors, int coors_cols, int32_t *num_points,
                       float *mean, int nfeat, int32_t *row_offset, int32_t *voxel_num, int cap, int32_t *status,
                       void *workspace, size_t workspace_bytes, void *stream);

/* SimpleVoxel.forward alone (vxnet.py:110-116): mean[v,f] = sum_t voxels[v,t,f] / num_points[v]. */
int sassd_voxel_mean(const float *voxels, const int32_t *num_points, int m, int max_points, int ndim,
                     int nfeat, float *mean, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Frustum crop: the FIRST nodes of a captured frame that starts at a raw 360-degree sweep.  Stable compaction of a point
 * cloud to one convex polytope -- the camera-2 viewing frustum of `remove_outside_points` (geometry.py:50-61, the
 * velodyne -> velodyne_reduced step of tools/create_data.py) -- with the point count in device memory on both sides, so
 * that sassd_voxelize_dev can follow it in the same graph.
 *
 * CONTRACT
 *   points     [cap_in, ndim] f32 device (ndim >= 3, xyz first);  n = min(*n_in_dev, cap_in) rows are the cloud (a
 *              negative count reads as 0).  Nothing is read past cap_in rows.
 *   planes     [6][4] f64 device: (nx, ny, nz, d) per face, as sassd_points_in_polytopes takes them; f32_math likewise.
 *   kept       row i < n is kept iff no face gives n.p + d >= 0 (a point ON a face is outside) -- the same device
 *              function sassd_points_in_polytopes evaluates (inside_polytope, csrc/augment_core.h: float64, or float32
 *              with f32_math, products and sums rounded separately).
 *   out        [cap_out, ndim] f32 device: the kept rows in ASCENDING i (stable), all ndim floats copied bit for bit.
 *              *n_out_dev = min(kept, cap_out); rows of `out` at and beyond *n_out_dev are not written.
 *   overflow   kept > cap_out: the first cap_out kept rows are written and SASSD_ST_POINT_OVERFLOW is OR-ed into *status.
 *              The same flag is set when *n_in_dev > cap_in.  `status` is only ever OR-ed into.
 *   workspace  sassd_crop_polytope_workspace_bytes(cap_in) bytes, 4-byte aligned: one int32 count per 256 rows of
 *              cap_in.  Every count is rewritten by every call (a replay with a smaller n sees no stale count).
 *   launches   two kernels, a grid of ceil(cap_in / 1024) workgroups each (one for cap_in == 0): the shape depends on
 *              cap_in only.  No host sync, no allocation, no memset, no atomics but the OR into `status`, and no
 *              workgroup waits for another inside a launch.  ndim == 4 with 16-byte aligned points / out moves rows as
 *              16-byte vectors; any other ndim (or alignment) takes a strided path with the same result.
 *   errors     SASSD_EINVAL before any HIP call: a NULL pointer (every pointer is required), ndim < 3, cap_in < 0,
 *              cap_out < 1, planes not 8-byte aligned, points / out / workspace not 4-byte aligned, workspace_bytes
 *              below the query.
 * ---------------------------------------------------------------------------------------------- */
size_t sassd_crop_polytope_workspace_bytes(int cap_in);
int sassd_crop_polytope_dev(const float *points, int cap_in, const int32_t *n_in_dev, int ndim,
                            const double *planes, int f32_math, float *out, int cap_out, int32_t *n_out_dev,
                            int32_t *status, void *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Multi-sweep merge: the FIRST node of a captured frame whose cloud is the current sweep plus up to 15 earlier sweeps,
 * each moved into the current sensor frame by its ego-pose transform, the time lag as an optional last feature (the
 * nuScenes / Waymo multi-sweep input; the reference, a KITTI project, has no counterpart).  The sweeps stay in a device
 * ring that the caller fills, one upload per sweep; a frame names the ring slots it reads through S descriptor entries
 * in device memory, so that sassd_voxelize_dev can follow in the same graph.
 *
 * CONTRACT
 *   ring       [R, sweep_cap, ndim_in] f32 device (ndim_in >= 3, xyz first).
 *   slot, count, xform   [S] i32 device;  T [S][3][4] f64 device (row major, the fourth column the translation);  dt [S]
 *              f32 device.  S is 1..16.  (sassd.stream.stage_layout keeps them in the frame's staging block.)
 *   out        [cap_out, ndim_out] f32 device, ndim_out = ndim_in + (time_feature ? 1 : 0).
 *   rows       entry s contributes c_s = clamp(count[s], 0, sweep_cap) rows, rows 0 .. c_s - 1 of ring slot slot[s].  A
 *              slot outside [0, R) is absent: it contributes 0 rows.  Nothing is ever read outside the ring.
 *   order      output rows in ENTRY order, entry 0 first; within an entry in ascending row order.  (The voxelizer keeps
 *              the first max_points arrivals per voxel: the entry listed first -- the current sweep -- wins.)
 *   transform  xform[s] == 0: all ndim_in floats of a row are copied bit for bit (the current sweep; an identity matrix
 *              would turn -0.0 into +0.0).  xform[s] != 0: x, y, z are replaced, per row i of T[s], by
 *                  float32(((T[s][i][0] * x + T[s][i][1] * y) + T[s][i][2] * z) + T[s][i][3])
 *              evaluated in float64, every product and sum rounded separately in exactly this order (no fused
 *              multiply-add, as inside_polytope of csrc/augment_core.h); the other columns are copied bit for bit.
 *              With time_feature the last output column of every row of entry s is dt[s].
 *   count      *n_out_dev = min(sum_s c_s, cap_out); rows of `out` at and beyond *n_out_dev are not written.
 *   overflow   sum_s c_s > cap_out, or any count[s] > sweep_cap: SASSD_ST_POINT_OVERFLOW is OR-ed into *status; the
 *              first cap_out rows are still written.  `status` is only ever OR-ed into.
 *   launches   one kernel, a grid of ceil(sweep_cap / 256) x S workgroups: the shape depends on (S, sweep_cap) only.
 *              Every thread derives its entry's first output row from the S <= 16 counts.  No host sync, no
 *              allocation, no memset, no atomics but the OR into `status`, and no workgroup waits for another.
 *              ndim_in == 4 without time_feature and with 16-byte aligned ring / out moves rows as 16-byte vectors;
 *              every other case takes a strided path with the same result.
 *   errors     SASSD_EINVAL before any HIP call: a NULL pointer (every pointer is required), S outside 1..16, R < 1,
 *              sweep_cap < 1, cap_out < 1, ndim_in < 3, T not 8-byte aligned, another pointer not 4-byte aligned.
 * ---------------------------------------------------------------------------------------------- */
int sassd_merge_sweeps_dev(const float *ring, int R, int sweep_cap, int ndim_in, const int32_t *slot,
                           const int32_t *count, const int32_t *xform, const double *T, const float *dt, int S,
                           int time_feature, float *out, int cap_out, int32_t *n_out_dev, int32_t *status, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Test-time augmentation: the detector runs on V views of every cloud inside ONE captured frame, and the candidates of
 * the views are suppressed together.  Two kernels frame the unchanged detector, which runs an inner batch of b * V samples
 * (inner sample s * V + v is view v of user sample s): sassd_tta_views_dev in front of the voxelizer, sassd_tta_pool
 * between sassd_pswarp_sample and sassd_rescore_nms, which then runs with batch = b and capK = capP.  (The reference's
 * BaseDetector.forward_test dispatches to an aug_test hook that its 3-D detector never implements.)
 *
 * CONTRACT
 *   view       (flip, angle, scale): flip 0 / 1 (y -> -y), angle in radians, scale > 0.  A call takes V = 1..8 views as
 *              HOST arrays read before it returns: flip [V] i32, rot_sin [V] = float32(sin(angle)), rot_cos [V] =
 *              float32(cos(angle)), scale [V] = float32(scale) and, for the pool, angle [V] = float32(angle).  View 0 is the
 *              identity: flip 0, rot_sin 0, rot_cos 1, scale 1 (angle 0).
 *   forward    sassd_tta_views_dev: src [cap, ndim] f32 device and its device count *n_src_dev are view 0, as they are.
 *              dst[v - 1] ([cap_dst, ndim] f32 device) and *n_dst_dev[v - 1], v = 1 .. V - 1 (HOST arrays of V - 1 device
 *              pointers) receive view v: n = clamp(*n_src_dev, 0, cap) rows and the count n.  x, y, z of a row are
 *              global_point of csrc/augment_core.h -- flip, then rotate, then scale; float32, every product and sum rounded
 *              on its own (no fused multiply-add) -- and every further column is copied bit for bit.  Rows of a
 *              destination at and beyond n are not written.  V == 1 launches nothing.
 *   inverse    a candidate box (x, y, z, w, l, h, yaw) of view v >= 1 returns to the sensor frame by unview_box of
 *              csrc/tta_core.h: float32, no fused multiply-add, each product, quotient and sum rounded on its own, in this
 *              order: (1) the first six fields are divided by scale; (2) x = x' * c - y' * s, y = x' * s + y' * c,
 *              yaw -= angle; (3) with flip: y = -y, yaw = -yaw + float32(pi).  Boxes of view 0 are copied bit for bit.
 *   pool       sassd_tta_pool: guided [b * V, capK, 7] f32, logits [b * V, capK] f32, labels [b * V, capK] i32, counts
 *              [b * V] i32 (the buffers of sassd_decode_filter / sassd_pswarp_sample at the inner batch) -> guided_p
 *              [b, capP, 7], logits_p [b, capP], labels_p [b, capP], counts_p [b].  The pooled rows of a sample are
 *              VIEW-MAJOR: view v contributes its first c_v = clamp(counts[s * V + v], 0, capK) rows in their order, boxes
 *              through the inverse, logits and labels copied.  counts_p[s] = min(sum_v c_v, capP); rows at and beyond it
 *              are not written.  (sassd_rescore_nms sorts stably: among equal scores the identity view wins.)
 *   overflow   sum_v c_v > capP: the rows past capP are dropped and SASSD_ST_BOX_OVERFLOW is OR-ed into *status, which is
 *              only ever OR-ed into.  A plan uses capP = min(V * capK, 4096), the most sassd_rescore_nms takes.
 *   launches   one kernel each, no workspace: views (ceil(cap * ndim / 256), V - 1) workgroups, one thread per output
 *              float; pool (ceil(capP / 256), b) workgroups, one thread per pooled row.  No host sync, no allocation, no
 *              memset, no atomics but the OR into `status`, no workgroup waits for another.
 *   errors     SASSD_EINVAL before any HIP call: V outside 1..8, ndim < 3, cap / batch / capK / capP < 1, capP > 4096, a
 *              NULL or misaligned (4 bytes) pointer, a destination that is the source, a view 0 that is not the identity,
 *              a flip that is not 0 / 1, a scale that is not positive and finite, a sine or cosine outside [-1, 1], an
 *              angle that is not finite.  SASSD_ENOSPC: cap_dst < cap (a destination cannot hold the source); capP <
 *              min(capK, 4096) (the pool cannot hold the identity view whole).
 * ---------------------------------------------------------------------------------------------- */
int sassd_tta_views_dev(const float *src, int cap, const int32_t *n_src_dev, int ndim, int V, const int32_t *flip,
                        const float *rot_sin, const float *rot_cos, const float *scale, float *const *dst,
                        int32_t *const *n_dst_dev, int cap_dst, void *stream);
int sassd_tta_pool(const float *guided, const float *logits, const int32_t *labels, const int32_t *counts, int batch,
                   int V, int capK, const int32_t *flip, const float *rot_sin, const float *rot_cos, const float *scale,
                   const float *angle, float *guided_p, float *logits_p, int32_t *labels_p, int32_t *counts_p, int capP,
                   int32_t *status, void *stream);

/* ------------------------------------------------------------------------------------------------
 * (a5) Rulebook build.  Replaces spconv v1.0 `get_indice_pairs` as invoked by SubMConv3d / SparseConv3d
 * (call sites mmdet/models/necks/cmn.py:147-173).  The rulebook is a gather table
 *   nbr[row_out, 27]  = input row feeding output row_out through kernel offset k=(kz*3+ky)*3+kx, or -1
 * (each (out,k) has at most one input); sassd_rulebook_pairs converts it to spconv's
 * indice_pairs[27,2,P] / indice_pair_num[27] form (pairs in ascending out row).
 *   indices [n,4] i32 (batch,z,y,x); n_ptr device int32 row count; cap = row capacity of indices/nbr.
 * ---------------------------------------------------------------------------------------------- */
size_t sassd_hash_bytes(int cap_rows);                 /* table for cap_rows keys                      */
int sassd_hash_build(const int32_t *indices, const int32_t *n_ptr, int cap, int D, int H, int W,
                     int batch_size, void *table, size_t table_bytes, int32_t *status, void *stream);
int sassd_rulebook_subm(const int32_t *indices, const int32_t *n_ptr, int cap, int D, int H, int W,
                        int batch_size, const void *table, size_t table_bytes, int32_t *nbr,
                        void *stream);
/* SparseConv3d(k=3, s=2, p=1): out dims (in+2-2-1)/2+1; out rows ascending in linear (b,z,y,x). */
size_t sassd_rulebook_conv_workspace_bytes(int D, int H, int W, int batch_size);
int sassd_rulebook_conv(const int32_t *in_indices, const int32_t *n_in_ptr, int cap_in, int D, int H,
                        int W, int batch_size, const void *in_table, size_t in_table_bytes,
                        int32_t *out_indices, int32_t *n_out_ptr, int cap_out, int32_t *nbr,
                        int32_t *status, void *workspace, size_t workspace_bytes, void *stream);
int sassd_rulebook_pairs(const int32_t *nbr, const int32_t *n_out_ptr, int cap_out, int K,
                         int32_t *pairs /*[K,2,cap_out]*/, int32_t *pair_num /*[K]*/, void *stream);

/* Fused rulebook PYRAMID: all gather tables of a stack of `levels` resolutions (level l: SubMConv3d k=3 rulebook,
 * indice_key "subm<l>"; l-1 -> l: SparseConv3d(k=3,s=2,p=1) rulebook + output coordinates) -- the seven
 * get_indice_pairs calls of VxNet (cmn.py:147-173, 197-206) in one fill + 2 launches per level (9 for VxNet; the
 * per-op chain above takes 30), or in one fill + ONE persistent launch (flags).
 *   indices[l]  [caps[l],4] i32 (b,z,y,x): level 0 is the input, levels >= 1 are written (ascending linear order)
 *   n_ptrs[l]   device int32 row counts: level 0 is the input, levels >= 1 are written
 *   D,H,W       spatial shape of level 0; level l+1 = (dim-1)/2+1 per axis
 *   nbr_subm[l] [caps[l],27] or NULL;  nbr_down[l] (l >= 1) [caps[l],27]: strided table from level l-1 into level l
 *   level_begin/level_end   build levels [begin, end) only (a caller that overlaps the tables with the convolutions
 *               issues one call per level and records an event after each); begin = 0 also resets the workspace.
 *   flags       SASSD_PYRAMID_PERSISTENT: all phases in ONE launch separated by agent-scope grid barriers (needs
 *               level_begin = 0, level_end = levels; bits 8..15 = workgroups per compute unit, 0 = default 2, max 4;
 *               a barrier that times out sets SASSD_ST_GRID_SYNC).  Per call, no process-wide state.
 *   workspace   16-byte aligned (cleared by 16-byte stores).
 * All pointer arrays are HOST arrays of device pointers. */
#define SASSD_PYRAMID_PERSISTENT 1
size_t sassd_rulebook_pyramid_workspace_bytes(int levels, const int *caps, int D, int H, int W, int batch_size);
int sassd_rulebook_pyramid(int levels, int32_t *const *indices, int32_t *const *n_ptrs, const int *caps,
                           int D, int H, int W, int batch_size, int32_t *const *nbr_subm,
                           int32_t *const *nbr_down, int level_begin, int level_end, int flags, int32_t *status,
                           void *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------------------------------
 * (a6+a7) Sparse convolution forward with fused per-channel affine (folded eval BatchNorm1d) + ReLU.
 * Replaces spconv `indice_conv_fp32` (+ nn.BatchNorm1d + nn.ReLU, cmn.py:138-173,208-212).
 *   y[o,:] = act( (sum_k x[nbr[o,k],:] @ w[k]) * scale + shift )
 *   w        [K, Cin, Cout] f32 (spconv layout [kz,ky,kx,Cin,Cout] flattened) -> pack once with
 *            sassd_spconv_pack_weight (sassd_spconv_packed_floats floats; an opaque image -- since round 4
 *            [K][Cin/4][Cout][4], four consecutive input channels of one output channel per 16-byte piece).
 *   nbr NULL = identity rulebook with K=1 (the 1x1x1 `extra_conv` shortcut, cmn.py:208-212).
 *   scale/shift may be NULL (1 / 0).  (Cin,Cout) in {(4,16),(16,16),(16,32),(32,32),(32,64),(64,64)}.
 * ---------------------------------------------------------------------------------------------- */
size_t sassd_spconv_packed_floats(int K, int Cin, int Cout);
int sassd_spconv_pack_weight(const float *w, int K, int Cin, int Cout, float *packed, void *stream);
int sassd_spconv_fwd(const float *x, const int32_t *nbr, const int32_t *n_out_ptr, int cap_out,
                     const float *w_packed, int K, int Cin, int Cout, const float *scale,
                     const float *shift, int relu, float *y, int cfg, void *stream);

/* (a15) Sparse convolution backward (training; replaces spconv `indice_conv_backward_fp32`).
 *   sassd_rulebook_transpose   nbrT[i,k] = o  for every rulebook entry nbr[o,k] = i  (-1 elsewhere); nbrT [cap_in,27]
 *   sassd_spconv_pack_weight_t forward weight w [K,Cin,Cout] -> packed image of W[k]^T for the data gradient
 *   sassd_spconv_bwd_data      dx[i,:] = sum_k dy[nbrT[i,k],:] @ W[k]^T       (dx [cap_in,Cin], dy [cap_out,Cout])
 *                              (nbrT NULL + K = 1: the 1x1x1 layer)
 *   sassd_spconv_bwd_weight    dw[k] (+)= sum_{o: nbr[o,k]>=0} x[nbr[o,k],:]^T (x) dy[o,:]   (dw [K,Cin,Cout];
 *                              deterministic two-stage reduction through the caller's workspace)
 * Gradients w.r.t. the fused scale/shift/ReLU epilogue are the caller's (elementwise). */
int sassd_rulebook_transpose(const int32_t *nbr, const int32_t *n_out_ptr, int cap_out, int32_t *nbrT,
                             int cap_in, void *stream);
int sassd_spconv_pack_weight_t(const float *w, int K, int Cin, int Cout, float *packed, void *stream);
int sassd_spconv_bwd_data(const float *dy, const int32_t *nbrT, const int32_t *n_in_ptr, int cap_in,
                          const float *wT_packed, int K, int Cin, int Cout, float *dx, int cfg, void *stream);
size_t sassd_spconv_bwd_weight_workspace_bytes(int cap_out, int K, int Cin, int Cout);
int sassd_spconv_bwd_weight(const float *x, const float *dy, const int32_t *nbr, const int32_t *n_out_ptr,
                            int cap_out, int K, int Cin, int Cout, float *dw, int accumulate, int cfg,
                            void *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Sparse input layer: SubMConv3d(Cin, 16, 3) for 3 <= Cin <= 8 features per voxel (csrc/spconv_in.hip).  The reference
 * cannot run a width other than 4 (cmn.py:104-106 writes voxel_features[:, :3] into a zeros_like(voxel_features)[:, 1:]);
 * the semantics are those of the project's oracle, oracle.nets.sparse_conv.  fp32 operands, K = 27.  The entry points of the
 * block above keep (4, 16) and still answer SASSD_EINVAL for every other narrow width; a caller with Cin != 4 calls these.
 * Cin = 4 is accepted here too and computes, bit for bit, what sassd_spconv_fwd computes for (4, 16).
 *   sassd_spconv_in_supported      1 iff K == 27, 3 <= Cin <= 8 and Cout == 16.
 *   sassd_spconv_in_pack_weight    w [K, Cin, Cout] -> an opaque image of sassd_spconv_in_packed_floats floats (0: unsupported),
 *                                  16-byte aligned: [K][CP/4][Cout][4] with CP = Cin rounded up to a multiple of 4 and zeros
 *                                  in the padding (at Cin = 4 the image of sassd_spconv_pack_weight).  The pack only moves
 *                                  words.  The FEATURES are never padded: x keeps the voxelizer's row stride of Cin floats.
 *   sassd_spconv_in_fwd            y[o, co] = act(acc * scale[co] + shift[co]) with the summation order part of the contract:
 *                                      acc = 0;  for k = 0..26: if nbr[o, k] >= 0: for c = 0..Cin-1:
 *                                          acc = fmaf(x[nbr[o, k]][c], w[k][c][co], acc)
 *                                  then the epilogue of sassd_spconv_fwd (one fused multiply-add, scale / shift NULL = 1 / 0,
 *                                  max(., 0) when relu).  y fp32 [cap_out, 16], or with y_bf16 != 0 bf16 [cap_out, 16]: the fp32
 *                                  result rounded to bf16, nearest even, at the store (the first layer of the bf16 sparse plans).
 *                                  The row count is read from n_out_ptr on the device, rows n..cap_out-1 of y are not written;
 *                                  one kernel launch, no memset: capturable into a frame graph.  x and w_packed 16-byte aligned.
 *   sassd_spconv_in_bwd_weight     dw[k][c][co] (+)= sum_{o: nbr[o,k] >= 0} x[nbr[o,k]][c] * dy[o][co]  (dw [K, Cin, Cout], dy
 *                                  [cap_out, 16] fp32): per-workgroup partial sums over ascending rows in the caller's workspace
 *                                  (sassd_spconv_in_bwd_weight_workspace_bytes bytes; 0: unsupported), added in a fixed order by
 *                                  a second kernel -- two calls on the same inputs agree bit for bit.  x 16-byte aligned.
 *                                  There is no data gradient: the input layer has none.
 * Every entry point returns SASSD_EINVAL before any launch for a NULL pointer, an unsupported (K, Cin, Cout), a misaligned image
 * and a workspace smaller than the size above.
 * ---------------------------------------------------------------------------------------------- */
int sassd_spconv_in_supported(int K, int Cin, int Cout);
size_t sassd_spconv_in_packed_floats(int K, int Cin, int Cout);
int sassd_spconv_in_pack_weight(const float *w, int K, int Cin, int Cout, float *packed, void *stream);
int sassd_spconv_in_fwd(const float *x, const int32_t *nbr, const int32_t *n_out_ptr, int cap_out, const float *w_packed, int K,
                        int Cin, int Cout, const float *scale, const float *shift, int relu, void *y, int y_bf16, void *stream);
size_t sassd_spconv_in_bwd_weight_workspace_bytes(int cap_out, int K, int Cin, int Cout);
int sassd_spconv_in_bwd_weight(const float *x, const float *dy, const int32_t *nbr, const int32_t *n_out_ptr, int cap_out, int K,
                               int Cin, int Cout, float *dw, int accumulate, void *workspace, size_t workspace_bytes,
                               void *stream);

/* (a8) SparseConvTensor.dense() + view (cmn.py:112-114): out [B, C*D, H, W] f32, zero filled here.
 * channel_order 0: channel = c*D + d (reference); 1: channel = d*C + c (internal, conv0 weights permuted). */
int sassd_densify(const float *feats, const int32_t *indices, const int32_t *n_ptr, int cap, int C,
                  int D, int H, int W, int batch_size, int channel_order, float *out, void *stream);
/* The same map as bf16 (each feature rounded to nearest even: the operand BEV conv0 rounds) for InferencePlan(precision="bf16"):
 * out [B, C*D, H, W] bf16, 16-byte aligned, cleared by a fill kernel (never hipMemsetAsync: no memset node in a captured frame).
 * Supported: H*W % 8 == 0; else SASSD_EINVAL before any launch. */
int sassd_densify_bf16_supported(int C, int D, int H, int W);
int sassd_densify_bf16(const float *feats, const int32_t *indices, const int32_t *n_ptr, int cap, int C, int D, int H, int W,
                       int batch_size, int channel_order, void *out, void *stream);

/* ------------------------------------------------------------------------------------------------
 * bf16 sparse backbone, inference (InferencePlan(sparse_precision="bf16"), test_cfg['sparse_precision']).  Chosen per plan
 * and per call -- no process-wide switch.  (Training has its own opt-in mode and contract: "bf16 sparse backbone, training"
 * below.)  Arithmetic contract:
 *   first layer (Cin = 4, the voxel means in metres: a bf16 ulp at 70 m is 0.5 m against a 0.05 m voxel)  x fp32 and the fp32
 *            weights, fp32 accumulation, relu(acc * scale + shift) in fp32, the result stored rounded to bf16 (nearest even);
 *   every other layer (submanifold, strided, the 1x1x1 `extra_conv`)  x bf16 as stored; the raw weights rounded once to bf16
 *            by the pack (BatchNorm is NOT folded into them); products of two bf16 values accumulated in fp32; epilogue
 *            relu(acc * scale + shift) in fp32 (scale / shift of the folded eval BatchNorm, NULL = 1 / 0); bf16 store;
 *   summation order a function of the rulebook only (no float atomics, no hipMemsetAsync: the calls are captured into the
 *            frame's hipGraph); two runs on the same inputs agree bit for bit.
 * sassd_spconv_bf16_supported       (K, Cin, Cout) in {(27,4,16), (27|1, 16,16), (27|1, 16,32), (27|1, 32,32), (27|1, 32,64),
 *                                   (27|1, 64,64)} and 0 < cap < 2^25 (every layer of the trunk at car batch 1, multi_cfg batch 8
 *                                   and Waymo-scale batch 4).
 * sassd_spconv_bf16_pack_weight     w [K,Cin,Cout] fp32 -> an opaque image of sassd_spconv_bf16_packed_bytes bytes (0: no kernel
 *                                   for the shape), 16-byte aligned: bf16 for Cin >= 16, the fp32 image of
 *                                   sassd_spconv_pack_weight for Cin = 4.
 * sassd_spconv_fwd_bf16             y_bf16 [cap_out, Cout] = the layer above; x bf16 [rows, Cin], or fp32 [rows, 4] with
 *                                   x_is_f32 = 1 (legal, and required, for Cin = 4 only); nbr NULL = identity rulebook with K = 1.
 *                                   x, w_packed, scale, shift 16-byte, y 8-byte aligned.  cfg is reserved (0): the fp32 kernel
 *                                   selection words do not apply.
 * sassd_densify_from_bf16           densify of bf16 features [rows, C]: the bits copied into a bf16 map (out_is_bf16 = 1) or
 *                                   widened exactly into an fp32 map; supported as sassd_densify_bf16, out 16-byte aligned,
 *                                   cleared by a fill kernel.
 * Every entry point returns SASSD_EINVAL for a NULL / misaligned pointer or an unsupported shape before it touches the device.
 * ---------------------------------------------------------------------------------------------- */
int sassd_spconv_bf16_supported(int K, int Cin, int Cout, int cap);
size_t sassd_spconv_bf16_packed_bytes(int K, int Cin, int Cout);
int sassd_spconv_bf16_pack_weight(const float *w, int K, int Cin, int Cout, void *packed, void *stream);
int sassd_spconv_fwd_bf16(const void *x, int x_is_f32, const int32_t *nbr, const int32_t *n_out_ptr, int cap_out,
                          const void *w_packed, int K, int Cin, int Cout, const float *scale, const float *shift, int relu,
                          void *y_bf16, int cfg, void *stream);
int sassd_densify_from_bf16(const void *feats, const int32_t *indices, const int32_t *n_ptr, int cap, int C, int D, int H, int W,
                            int batch_size, int channel_order, void *out, int out_is_bf16, void *stream);

/* ------------------------------------------------------------------------------------------------
 * bf16 sparse backbone, training (opt-in: sassd.autograd.set_sparse_precision("bf16") or train_cfg['sparse_precision'] = 'bf16';
 * off by default, and with the mode off every launch of a training step is what it was).  Every tensor a sparse kernel GATHERS is
 * stored bf16; what is read contiguously or feeds statistics stays fp32.  Arithmetic contract:
 *   first layer (Cin = 4, voxel means in metres)  forward and weight gradient on the fp32 kernels with fp32 operands
 *            (sassd_spconv_fwd / sassd_spconv_bwd_weight); it has no data gradient.
 *   every other sparse conv (submanifold, strided, the 1x1x1 `extra_conv`)
 *     forward          x bf16 as stored; the fp32 master weight rounded once to bf16 by the pack; products exact in fp32, fp32
 *                      accumulation; the RAW result stored fp32 -- no epilogue; BatchNorm statistics are taken on fp32.
 *     data gradient    the same kernel on dy (bf16 as stored) with the bf16 image of W[k]^T: on the transposed table, or, for a
 *                      submanifold layer, on the forward table with the offset-reversed image (the rule of the fp32 path);
 *                      dx fp32.
 *     weight gradient  x bf16 (the saved forward operand) and dy bf16, fp32 accumulation, the deterministic two-stage reduction
 *                      through the caller's workspace (the partial-sum layout and reduce kernel of sassd_spconv_bwd_weight);
 *                      dw fp32.  An offset without a pair gives exactly 0.
 *   training BatchNorm1d + ReLU between the layers  arithmetic and running statistics bit-identical to sassd_bn_relu_fwd /
 *            _bwd; only the store changes: the forward writes its output rounded to bf16 (nearest even) -- the next conv's
 *            operand, saved for the backward at half the bytes -- and the backward writes the gradient of the raw conv output
 *            rounded to bf16 -- what the data gradient gathers and the weight gradient reads.  Behind the fp32 first layer the
 *            backward writes fp32 (sassd_bn_relu_bwd).
 *   downstream  the auxiliary head's three feature scales and the dense map receive the bf16 features widened exactly to fp32;
 *            master weights, Adam state and gradients stay fp32.  A conv that is not followed by the fused BatchNorm + ReLU
 *            rounds its fp32 incoming gradient to bf16 once; fp32 features entering the trunk behind the first layer likewise.
 *   no float atomics and no hipMemsetAsync in any entry point below; the summation order is a function of the rulebook alone:
 *            two calls on the same inputs agree bit for bit.
 * sassd_spconv_train_bf16_supported   (Cin, Cout) in {(16,16), (16,32), (32,32), (32,64), (64,64)} and the transposed pairs of
 *                                     the data gradients {(32,16), (64,32)}, K = 27 or 1, 0 < cap < 2^25.
 * sassd_spconv_train_bf16_pack_weight w [K,Cin,Cout] fp32 -> bf16 [K][Cout][Cin] (sassd_spconv_train_bf16_packed_bytes bytes; 0:
 *                                     no kernel), the pack kernel of sassd_spconv_bf16_pack_weight over the training shape list.
 *                                     The image of a data gradient is this pack fed W[k]^T ([K,Cout,Cin]; offsets flipped for
 *                                     the forward-table form) with (Cout, Cin) as its (Cin, Cout).  packed 16-byte aligned.
 * sassd_spconv_fwd_bf16_raw           y fp32 [cap_out, Cout] = sum_k x[nbr[:,k]] . W[k]: forward and data gradient.  nbr NULL =
 *                                     identity rulebook with K = 1.  x, w_packed, y 16-byte aligned; cfg is reserved (0).  Rows
 *                                     past the count are not written.
 * sassd_spconv_bwd_weight_bf16        dw [27,Cin,Cout] fp32 (+= with accumulate) for the forward pairs; workspace of
 *                                     sassd_spconv_bwd_weight_bf16_workspace_bytes bytes (0: no kernel), 16-byte aligned like x
 *                                     and dy; cfg is reserved (0).  SASSD_ENOSPC for a short workspace.
 * sassd_bn_relu_fwd_bf16out / _bwd_bf16out   sassd_bn_relu_fwd / _bwd with y / dx bf16 [n, C] (8-byte aligned; x and dy 16-byte).
 * Every entry point returns SASSD_EINVAL for a NULL / misaligned pointer or an unsupported shape before it touches the device.
 * ---------------------------------------------------------------------------------------------- */
int sassd_spconv_train_bf16_supported(int K, int Cin, int Cout, int cap);
size_t sassd_spconv_train_bf16_packed_bytes(int K, int Cin, int Cout);
int sassd_spconv_train_bf16_pack_weight(const float *w, int K, int Cin, int Cout, void *packed, void *stream);
int sassd_spconv_fwd_bf16_raw(const void *x_bf16, const int32_t *nbr, const int32_t *n_out_ptr, int cap_out, const void *w_packed,
                              int K, int Cin, int Cout, float *y, int cfg, void *stream);
size_t sassd_spconv_bwd_weight_bf16_workspace_bytes(int cap_out, int K, int Cin, int Cout);
int sassd_spconv_bwd_weight_bf16(const void *x_bf16, const void *dy_bf16, const int32_t *nbr, const int32_t *n_out_ptr, int cap_out,
                                 int K, int Cin, int Cout, float *dw, int accumulate, int cfg, void *workspace,
                                 size_t workspace_bytes, void *stream);
int sassd_bn_relu_fwd_bf16out(const float *x, int n, int C, const float *gamma, const float *beta, float *running_mean,
                              float *running_var, float momentum, float eps, void *y_bf16, float *save_mean, float *save_invstd,
                              void *workspace, size_t workspace_bytes, void *stream);
int sassd_bn_relu_bwd_bf16out(const float *x, const float *dy, int n, int C, const float *gamma, const float *beta,
                              const float *save_mean, const float *save_invstd, void *dx_bf16, float *dgamma, float *dbeta,
                              void *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------------------------------
 * (a9,a10,a12) Dense 2-D convolution (3x3 pad 1 or 1x1), NCHW fp32, on fp32 MFMA (v_mfma_f32_32x32x2_f32),
 * fused per-channel affine (folded BatchNorm2d / bias) + optional ReLU.  Replaces torch.nn.Conv2d +
 * BatchNorm2d + ReLU in BEVNet (cmn.py:233-282), SSDRotateHead (ssd_rotate_head.py:120-125) and
 * PSWarpHead.convs (:424-429).   w torch layout [Cout,Cin,k,k]; pack once.
 * ---------------------------------------------------------------------------------------------- */
size_t sassd_conv2d_packed_floats(int Cin, int Cout, int ksize);
int sassd_conv2d_pack_weight(const float *w, int Cout, int Cin, int ksize, float *packed, void *stream);
int sassd_conv2d_fwd(const float *x, const float *w_packed, const float *scale, const float *shift,
                     int relu, float *y, int batch, int Cin, int Cout, int H, int W, int ksize,
                     void *stream);
/* ... with a per-call `cfg` word (0 = sassd_conv2d_fwd): ablation switches of tools/run_conv.py -- 1 = no staging DMA after the
 * first chunk, 2 = no chunk barrier. */
int sassd_conv2d_fwd_cfg(const float *x, const float *w_packed, const float *scale, const float *shift, int relu, float *y,
                         int batch, int Cin, int Cout, int H, int W, int ksize, int cfg, void *stream);

/* 1x1 convolution with <= 32 output channels (the fused SSD head, ssd_rotate_head.py:120-125; the second conv of the
 * part-sensitive head, :424-429) as an HBM stream on the vector ALU: same contract as sassd_conv2d_fwd with ksize 1, but
 * the weights are handed over TRANSPOSED and zero-padded, wT [Cin][CO] fp32, CO = sassd_conv1x1_narrow_pad(Cout), 16-byte
 * aligned. */
int sassd_conv1x1_narrow_supported(int Cin, int Cout);
int sassd_conv1x1_narrow_pad(int Cout);
int sassd_conv1x1_narrow_fwd(const float *x, const float *wT, const float *scale, const float *shift, int relu,
                             float *y, int batch, int Cin, int Cout, int H, int W, void *stream);

/* Winograd F(2x2,3x3) variant of the 3x3 / stride 1 / pad 1 convolution (the BEVNet layers cmn.py:240-262): 2.25x
 * fewer multiplications on the fp32 MFMA, transforms fused (nothing but x, packed weights and y touches HBM).  Same
 * epilogue as sassd_conv2d_fwd (y = relu?(conv * scale[co] + shift[co]), NULL scale/shift = 1/0).  Requires
 * Cin % 32 == 0, Cout % 32 == 0, even H, W % 4 == 0 and W >= 64 (sassd_conv2d_wino_supported; anything else takes
 * sassd_conv2d_fwd); relative error ~1e-6 vs the direct kernel. */
int sassd_conv2d_wino_supported(int Cin, int Cout, int H, int W);
size_t sassd_conv2d_wino_packed_floats(int Cin, int Cout);
int sassd_conv2d_wino_pack_weight(const float *w, int Cout, int Cin, float *packed, void *stream);
int sassd_conv2d_wino_fwd(const float *x, const float *w_packed, const float *scale, const float *shift, int relu,
                          float *y, int batch, int Cin, int Cout, int H, int W, void *stream);

/* The same layers through Winograd F(4x4,3x3) as THREE launches: input transform -> 36 GEMMs
 * (Cout x Cin x tiles) -> output transform with the folded BatchNorm / bias / ReLU epilogue.  4x fewer multiplications
 * than the direct convolution (1.78x fewer than F(2x2)); fp32 rounding error ~6x the direct kernel's (2.4e-6 relative after
 * seven layers).  The GEMMs compute their fp32 products on the bf16 MFMA over operands split exactly into three bf16
 * pieces in registers (eight of the nine piece products, fp32 accumulation: the error of the fp32 MFMA at half its
 * cycles); tensors, packed weights and workspace stay fp32.  Needs Cin % 32 == 0, Cout % 256 == 0, H % 4 == 0,
 * W % 4 == 0 and a caller workspace (transformed input + product tensors, 36 planes each). */
int sassd_conv2d_wino4_supported(int Cin, int Cout, int H, int W);
size_t sassd_conv2d_wino4_packed_floats(int Cin, int Cout);
int sassd_conv2d_wino4_pack_weight(const float *w /*[Cout,Cin,3,3]*/, int Cout, int Cin, float *packed, void *stream);
size_t sassd_conv2d_wino4_workspace_bytes(int batch, int Cin, int Cout, int H, int W);
int sassd_conv2d_wino4_fwd(const float *x, const float *w_packed, const float *scale, const float *shift, int relu,
                           float *y, int batch, int Cin, int Cout, int H, int W, int cfg, void *workspace,
                           size_t workspace_bytes, void *stream);

/* Chained 3x3 layers with the activation map between them kept in the transform domain: one call = one layer,
 *   src_products == 0: V = input transform of the NCHW map x (as sassd_conv2d_wino4_fwd);
 *   src_products != 0: V = fused output->input transform of the products the PREVIOUS chain call left in `workspace`
 *                      (that call's Cout = this call's Cin, same batch / H / W / cmax; its folded BatchNorm / ReLU passed
 *                      here as prev_scale / prev_shift / prev_relu) -- the map between the two layers is never written to
 *                      HBM (cmn.py:240-262: conv0 .. conv6 of the BEV stack);
 *   then the 36 GEMMs; y != NULL: output transform + scale / shift / relu into the NCHW map y, y == NULL: the products
 *   stay in the workspace for the next call.  cmax >= every Cin / Cout of the chain fixes the workspace layout
 *   (sassd_conv2d_wino4_chain_workspace_bytes(batch, cmax, H, W)).  sassd_conv2d_wino4_chain_supported: the fused
 *   transform keeps one (H + 2) x (W + 2) plane in LDS (<= 160 KB).  src_products = 1 additionally requires that this
 *   layer and the previous one (whose Cout is this Cin) pad their tile count to the same plane stride -- true whenever
 *   both have the same Cout; SASSD_EINVAL otherwise. */
int sassd_conv2d_wino4_chain_supported(int Cin, int Cout, int H, int W);
size_t sassd_conv2d_wino4_chain_workspace_bytes(int batch, int cmax, int H, int W);
int sassd_conv2d_wino4_chain(const float *x, int src_products, const float *prev_scale, const float *prev_shift,
                             int prev_relu, const float *w_packed, const float *scale, const float *shift, int relu,
                             float *y, int batch, int Cin, int Cout, int cmax, int H, int W, const int32_t *tile_map,
                             const int32_t *prev_tile_map, int cfg, void *workspace, size_t workspace_bytes,
                             void *stream);
/* A NARROW layer (<= 64 output channels) at the end of a chain: the part-sensitive head's 3x3 conv 256 -> 28
 * (ssd_rotate_head.py:424-429) on conv6's products.  One call = the fused transform of the previous call's products (prev_* = that
 * layer's folded BatchNorm / ReLU; y_prev, optional: its NCHW activation map, stored from the LDS plane for its other readers --
 * BEVNet conv7, cmn.py:262), the 36 GEMMs on a 64-channel block, the output transform + scale / shift / relu into y [B,Cout,H,W].
 * Weights: sassd_conv2d_wino4_pack_weight_narrow ([36][Cin][64], zero padded).  cfg: the geometry of the chain's other calls; this
 * layer runs 128-column blocks on their planes, and a geometry whose plane stride is no multiple of 128 is SASSD_EINVAL. */
size_t sassd_conv2d_wino4_narrow_packed_floats(int Cin);
int sassd_conv2d_wino4_pack_weight_narrow(const float *w /*[Cout,Cin,3,3]*/, int Cout, int Cin, float *packed, void *stream);
int sassd_conv2d_wino4_chain_tail(const float *prev_scale, const float *prev_shift, int prev_relu, float *y_prev,
                                  const float *w_packed64, const float *scale, const float *shift, int relu, float *y,
                                  int batch, int Cin, int Cout, int cmax, int H, int W, const int32_t *prev_tile_map, int cfg,
                                  void *workspace, size_t workspace_bytes, void *stream);

/* Active-tile map of a SPARSE input map (BEVNet conv0 reads SparseConvTensor.dense(), cmn.py:112-114,240: 56 % of the 4x4
 * tiles of a KITTI frame have an occupied pixel in their 6x6 patch).  indices [cap,4] (b, z, y, x) = the sparse rows that
 * were densified.  A chain call with `tile_map` (src_products == 0) transforms and multiplies the active tiles only
 * (compacted columns); the NEXT chain call passes the same map as `prev_tile_map` (or this call, with y != NULL, its own):
 * an inactive tile's products are exactly zero, so the result is bit-identical to the dense launch.  NULL = all tiles.
 * tile_map: sassd_wino4_tile_map_ints(batch, H, W) int32, 16-byte aligned like `indices` (0 = unsupported: more than 2^24
 * tiles): [0] active tiles, [1] tiles, [2..3] 0, tpos[T] (column of tile t or -1), tlist[T] (tile of column j, ascending), then
 * the call's own tile flags.  Two grid-wide launches behind one fill kernel. */
size_t sassd_wino4_tile_map_ints(int batch, int H, int W);
int sassd_wino4_tile_map(const int32_t *indices, const int32_t *n_ptr, int cap, int batch, int H, int W,
                         int32_t *tile_map, void *stream);

/* BEVNet conv0 straight from the sparse tensor: the first layer of a chain WITHOUT the dense [B, C D, H, W] map in between.
 *   sassd_wino4_sparse_prepare   per frame, from the level-3 coordinates alone (indices [cap,4] (b, z, y, x), rows past
 *                                min(*n_ptr, cap) ignored, rows unique per coordinate): the tile map above AND the pixel -> row
 *                                index grid, int32 [B][D][H][W] (sassd_wino4_sparse_grid_ints, -1 = empty), cleared by a fill
 *                                kernel and filled one thread per row -- no memset node, no atomics.
 *   sassd_conv2d_wino4_chain_sparse   = sassd_densify(channel_order 1) + sassd_conv2d_wino4_chain(x, src_products 0, tile_map)
 *                                bit for bit: the input transform gathers feats [rows, C] (fp32, 16-byte aligned rows: C % 4 == 0)
 *                                through the grid into V[p][d C + c][column of the tile], then the same 36 GEMMs on the active
 *                                columns and, with y != NULL, the same output transform; y == NULL leaves the products for the
 *                                next sassd_conv2d_wino4_chain call (prev_tile_map = this tile_map).
 * SASSD_EINVAL before any launch: C * D != Cin, Cin % 32 != 0, D > 8 (documented precondition of the grid), C % 4 != 0, no
 * tile_map, a shape sassd_conv2d_wino4_supported refuses, a pointer that is not 16-byte aligned; SASSD_ENOSPC: workspace below
 * sassd_conv2d_wino4_chain_workspace_bytes(batch, cmax, H, W). */
size_t sassd_wino4_sparse_grid_ints(int batch, int D, int H, int W);
int sassd_wino4_sparse_prepare(const int32_t *indices, const int32_t *n_ptr, int cap, int batch, int D, int H, int W,
                               int32_t *grid, int32_t *tile_map, void *stream);
int sassd_conv2d_wino4_chain_sparse(const float *feats, int C, int D, const int32_t *grid, const float *w_packed,
                                    const float *scale, const float *shift, int relu, float *y, int batch, int Cin, int Cout,
                                    int cmax, int H, int W, const int32_t *tile_map, int cfg, void *workspace,
                                    size_t workspace_bytes, void *stream);

/* 1x1 convolution with >= 128 output channels (BEVNet conv7, cmn.py:262) as a plain fp32-MFMA GEMM over the NCHW
 * tensor (y[b] [Cout x HW] = W [Cout x Cin] . x[b] [Cin x HW]) with the folded BatchNorm / bias / ReLU epilogue; the
 * kernel of the Winograd F(4x4) products with one problem per image.  Needs Cin % 32 == 0, Cout % 128 == 0 and H*W
 * divisible by one of 64 / 96 / 128 / 160 / 192; weights packed [Cin][Cout] (Cin*Cout floats). */
int sassd_conv1x1_gemm_supported(int Cin, int Cout, int H, int W);
int sassd_conv1x1_gemm_pack_weight(const float *w /*[Cout,Cin,1,1]*/, int Cout, int Cin, float *packed, void *stream);
int sassd_conv1x1_gemm_fwd(const float *x, const float *w_packed, const float *scale, const float *shift, int relu,
                           float *y, int batch, int Cin, int Cout, int H, int W, int cfg, void *stream);

/* BASELINE configs[2] (bf16 training): the 3x3 pad-1 BEV convolutions (cmn.py:240-262) with bf16 MFMA operands --
 * direct implicit GEMM on v_mfma_f32_32x32x16_bf16, fp32 accumulation, NCHW fp32 activations in and out, optional
 * per-channel bias.  Weights are packed once per update ([Cout,Cin,3,3] fp32 -> bf16 [tap][Cin32/8][Cout][8],
 * sassd_conv2d_bf16_packed_elems 16-bit elements).  The data gradient is the same call on dy with the weights
 * transposed and the taps mirrored.  Supported: Cout % 32 == 0, W >= 16 and W % 4 == 0 (the last 16-column tile may be partial: the 188-wide Waymo-scale map; else SASSD_EINVAL; the caller keeps the
 * fp32 kernels); Cin is padded to a multiple of 32 with zero weights inside the pack. */
int sassd_conv2d_bf16_supported(int Cin, int Cout, int H, int W);
size_t sassd_conv2d_bf16_packed_elems(int Cin, int Cout);
int sassd_conv2d_bf16_pack_weight(const float *w, int Cout, int Cin, void *packed, void *stream);
int sassd_conv2d_bf16_fwd(const float *x, const void *w_packed, const float *shift, float *y, int batch, int Cin,
                          int Cout, int H, int W, void *stream);
/* ... with a per-call `cfg` word (0 = sassd_conv2d_bf16_fwd; tools / tests only): low byte = compile-time ablation variant of the
 * kernel (tools/run_bf16_conv.py), bits 8-15 = forced workgroup count (long runs of tiles), 0x10000 / 0x20000 / 0x40000 =
 * wave-priority and loader-order A/B switches, 0x80000 = Cout = 320 on 128-cout instead of 160-cout workgroups. */
int sassd_conv2d_bf16_fwd_cfg(const float *x, const void *w_packed, const float *shift, float *y, int batch, int Cin,
                              int Cout, int H, int W, int cfg, void *stream);
/* The same convolution over relu(batchnorm(x)), the normalisation applied by the kernel's loader waves (round 6): x is the RAW
 * output of the previous convolution, in_affine [3][Cin] = mean | invstd * gamma | beta as sassd_bn2d_stats writes it.  The
 * operand that reaches the MFMA is bit-identical to the one sassd_bn2d_relu_fwd + sassd_conv2d_bf16_fwd produce, and the
 * normalised map (cmn.py:236-237 between two BEV layers) is never written to HBM.  Cin <= 1024. */
int sassd_conv2d_bf16_bnrelu_fwd(const float *x, const float *in_affine, const void *w_packed, const float *shift, float *y,
                                 int batch, int Cin, int Cout, int H, int W, void *stream);

/* 1x1 convolution on the bf16 MFMA (round 6; same arithmetic contract as sassd_conv2d_bf16_fwd: weights rounded to bf16 at pack
 * time, activations on their way into the MFMA, fp32 accumulation, fp32 NCHW tensors in and out): BEVNet's conv7 (cmn.py:262),
 * its data gradient, and the data gradient of the SSD head's 1x1 convs (ssd_rotate_head.py:120-125) under
 * set_bev_precision("bf16") -- HBM streams of 144 MB that took 150 us each on the fp32-MFMA kernel.  x [B,Cin,HW] -> y
 * [B,Cout,HW] (+ shift[Cout], may be NULL).  Cin <= 256 (padded inside the pack), any Cout (64-channel groups, the last
 * one masked), HW % 4 == 0; x 8-byte, y and the pack 16-byte aligned.  pack_weight: w fp32 [Cout][Cin], or -- transposed = 1 --
 * the [Cin][Cout] array of the forward layer read as its transpose (the data gradient's weights, no host-side transpose);
 * sassd_conv1x1_bf16_packed_elems 16-bit elements. */
int sassd_conv1x1_bf16_supported(int Cin, int Cout, int HW);
size_t sassd_conv1x1_bf16_packed_elems(int Cin, int Cout);
int sassd_conv1x1_bf16_pack_weight(const float *w, int Cout, int Cin, int transposed, void *packed, void *stream);
int sassd_conv1x1_bf16_fwd(const float *x, const void *w_packed, const float *shift, float *y, int batch, int Cin, int Cout,
                           int HW, void *stream);

/* bf16 inference (InferencePlan(precision="bf16")): every dense conv of the frame on bf16 operands with fp32 accumulation.
 * x is a bf16 NCHW map (rounded by its producer: rounding at the store gives the operand rounding at the load would), the
 * weights are the RAW conv weights rounded once at pack time (BatchNorm is not folded into them), and the epilogue applies the
 * eval BatchNorm + ReLU in fp32 to the accumulator -- relu(acc * scale[co] + shift[co]) (relu = 0: no ReLU; scale = NULL:
 * acc + shift[co], shift may be NULL too) -- and stores bf16 (y_bf16 = 1: the map of the next conv, rounded to nearest even)
 * or fp32.  Caller-owned buffers, no allocation, no host sync; SASSD_EINVAL on NULL pointers, misalignment or unsupported
 * shapes before anything touches the device.
 * 3x3 pad 1 (BEV conv0-conv6, the part-sensitive 256 -> 28 conv): the implicit GEMM of sassd_conv2d_bf16_fwd with a bf16
 * loader.  Weights [Cout,Cin,3,3] fp32 packed at Cout rounded up to 32 (zero rows; sassd_conv2d_bf16_infer_packed_elems 16-bit
 * elements); y [B,Cout,H,W] holds only the Cout real maps.  Supported: W >= 16, W % 4 == 0.  x 8-byte, the pack 16-byte,
 * y 8-byte (bf16) / 16-byte (fp32) aligned. */
int sassd_conv2d_bf16_infer_supported(int Cin, int Cout, int H, int W);
size_t sassd_conv2d_bf16_infer_packed_elems(int Cin, int Cout);
int sassd_conv2d_bf16_infer_pack_weight(const float *w, int Cout, int Cin, void *packed, void *stream);
int sassd_conv2d_bf16_infer_fwd(const void *x, const void *w_packed, const float *scale, const float *shift, int relu, void *y,
                                int y_bf16, int batch, int Cin, int Cout, int H, int W, void *stream);
/* 1x1 (BEV conv7: BatchNorm + ReLU, bf16 out; the fused SSD head: bias, fp32 out; the part-sensitive 28 -> 28 conv: fp32 out)
 * on the kernel of sassd_conv1x1_bf16_fwd, weights from sassd_conv1x1_bf16_pack_weight.  Supported shapes are those of
 * sassd_conv1x1_bf16_supported.  x 4-byte, the pack 16-byte, y 8-byte (bf16) / 16-byte (fp32) aligned. */
int sassd_conv1x1_bf16_infer_supported(int Cin, int Cout, int HW);
int sassd_conv1x1_bf16_infer_fwd(const void *x, const void *w_packed, const float *scale, const float *shift, int relu, void *y,
                                 int y_bf16, int batch, int Cin, int Cout, int HW, void *stream);

/* Training: weight gradient of the same convolutions (autograd of nn.Conv2d at cmn.py:240-262 and
 * ssd_rotate_head.py:120-125,424-429; cuDNN in the reference).  x [B,Cin,H,W], dy [B,Cout,H,W] NCHW fp32 ->
 * dw [Cout,Cin,k,k] (torch layout), overwritten or accumulated.  Split-K over pixels with a deterministic second-stage
 * reduction; workspace from sassd_conv2d_wgrad_workspace_bytes.  The data gradient is sassd_conv2d_fwd on dy with the
 * weights transposed and the taps mirrored (sassd.autograd.Conv2dFn). */
size_t sassd_conv2d_wgrad_workspace_bytes(int batch, int Cin, int Cout, int H, int W, int ksize);
int sassd_conv2d_bwd_weight(const float *x, const float *dy, float *dw, int batch, int Cin, int Cout, int H, int W,
                            int ksize, int accumulate, void *workspace, size_t workspace_bytes, void *stream);
/* BASELINE configs[2] (bf16 training): the same contraction with x and dy rounded to bf16 (round-to-nearest-even) on
 * their way into LDS, multiplied on v_mfma_f32_32x32x16_bf16 with fp32 accumulation; dw stays fp32.  W must be even
 * (SASSD_EINVAL otherwise).  What the reference gets from cuDNN under torch autocast / apex O1. */
int sassd_conv2d_bwd_weight_bf16(const float *x, const float *dy, float *dw, int batch, int Cin, int Cout, int H, int W,
                                 int ksize, int accumulate, void *workspace, size_t workspace_bytes, void *stream);
/* ... with the X operand = relu(batchnorm(x)) applied on the way into LDS (x_affine as above; 3x3 only): the weight gradient of
 * a layer whose input map was never materialised (sassd_conv2d_bf16_bnrelu_fwd). */
int sassd_conv2d_bwd_weight_bf16_bnrelu(const float *x, const float *x_affine, const float *dy, float *dw, int batch, int Cin,
                                        int Cout, int H, int W, int ksize, int accumulate, void *workspace,
                                        size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------------------------------
 * (f-3 / a18) fused training targets and RPN loss.
 *
 * sassd_assign_targets: mmdet/core/bbox3d/target_ops.py:139-277 (create_target_np) for a whole batch in two launches.
 *   anchors [A,7] (anchors_per_sample = 0) or [B,A,7]; anchor_mask [B,A] u8 or NULL; ground truths of all samples
 *   concatenated: gt_boxes [T,7], gt_classes [T] i64 or NULL (all 1), gt_ok [T] u8 or NULL, gt_offsets [B+1] i32
 *   (device).  Similarity = NearestIouSimilarity (iou3d_utils.py:163-183) computed in the kernel, or -- overlaps != NULL
 *   -- a precomputed row-major [A, G_b] matrix per sample starting at overlaps + overlap_offsets[b] (i64, device).
 *   Outputs: labels i64 (-1 ignore / 0 negative / class), targets (second_box_encode, ssd_rotate_head.py:15-50, zero
 *   for non-positives), best_overlap (or NULL), each with out_sample_stride anchors between samples (>= A: lets
 *   several classes write interleaved [B, classes, A] tensors); num_pos[b] += positives (zeroed first when
 *   zero_num_pos).  Workspace: sassd_assign_targets_workspace_bytes.
 * sassd_rpn_loss: ssd_rotate_head.py:128-314 loss() in one pass: loss_sums[3] = (smooth-L1 with sin-difference, sigmoid
 *   focal, direction cross-entropy) with NormByNumPositives weights, and the gradients of those three sums with
 *   respect to box_preds [B,A,7], cls_preds [B,A,num_class], dir_preds [B,A,2] (dir_preds may be NULL). */
size_t sassd_assign_targets_workspace_bytes(int batch, int n_anchors, int total_gt);
int sassd_assign_targets(const float *anchors, int anchors_per_sample, const uint8_t *anchor_mask, int n_anchors,
                         int batch, const float *gt_boxes, const int64_t *gt_classes, const uint8_t *gt_ok,
                         const int32_t *gt_offsets, int total_gt, const float *overlaps, const int64_t *overlap_offsets,
                         float matched_threshold, float unmatched_threshold, int64_t *labels, float *targets,
                         float *best_overlap, size_t out_sample_stride, int32_t *num_pos, int zero_num_pos,
                         void *workspace, size_t workspace_bytes, void *stream);
/* Guided-anchor selection for training (ssd_rotate_head.py:316-388) without a host round trip: ascending indices of the
 * anchors with anchor_mask set (NULL = all) and sigmoid(max_c cls_preds[b,a,c]) > score_thr go to sel[b][0..counts[b]) of
 * a fixed-capacity [B,cap] int64 buffer (remaining entries p -> p: valid, distinct indices); *overflow is set (never cleared) when a sample had more
 * than cap (the surplus is dropped).  Workspace: sassd_guided_select_workspace_bytes. */
size_t sassd_guided_select_workspace_bytes(int batch, int n_anchors);
int sassd_guided_select(const float *cls_preds, const uint8_t *anchor_mask, int n_anchors, int batch, int num_class,
                        float score_thr, int cap, int64_t *sel, int32_t *counts, int32_t *overflow, void *workspace,
                        size_t workspace_bytes, void *stream);
size_t sassd_rpn_loss_workspace_bytes(int batch, int n_anchors);
int sassd_rpn_loss(const float *box_preds, const float *cls_preds, const float *dir_preds, int num_class,
                   const int64_t *labels, const float *targets, const float *anchors, int anchors_per_sample,
                   const int32_t *num_pos, int n_anchors, int batch, float *grad_box, float *grad_cls, float *grad_dir,
                   float *loss_sums, void *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------------------------------
 * (f-1) anchors_mask: mmdet/datasets/kitti.py:333-343 with geometry.py:676-710
 * (sparse_sum_for_anchors_mask -> cumsum -> fused_get_anchors_area > area_threshold).
 *   coors [n,4] (b,z,y,x) rows of ONE batch element are selected by batch_idx
 *   anchors_bv [A,4] f32 (xmin,ymin,xmax,ymax); mask [A] u8
 * ---------------------------------------------------------------------------------------------- */
size_t sassd_anchor_mask_workspace_bytes(int H0, int W0);
int sassd_anchor_mask(const int32_t *coors, const int32_t *row_begin_ptr, const int32_t *row_end_ptr,
                      int H0, int W0, const float *anchors_bv, int n_anchors, const float *voxel_size,
                      const float *coors_range, float area_threshold, uint8_t *mask, void *workspace,
                      size_t workspace_bytes, void *stream);
/* The same for `batch` samples in one launch sequence: sample b owns the coordinate rows [row_offsets[b],
 * row_offsets[b+1]) (device int32[batch+1], what sassd_voxelize's row_offset chain leaves behind), mask[b*n_anchors..]
 * and one sassd_anchor_mask_workspace_bytes slice of the workspace (batch slices in total). */
int sassd_anchor_mask_batch(const int32_t *coors, const int32_t *row_offsets, int batch, int H0, int W0,
                            const float *anchors_bv, int n_anchors, const float *voxel_size,
                            const float *coors_range, float area_threshold, uint8_t *mask, void *workspace,
                            size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------------------------------
 * (a11) get_guided_anchors, test path (ssd_rotate_head.py:307-372) + second_box_decode (:53-91).
 *   box/cls/dir: raw conv outputs [B, ncls*A*7 | ncls*A*ncls | ncls*A*2, H, W] (NCHW), channel strides
 *   given in floats via *_batch_stride (lets the three heads live in one fused conv output).
 *   anchors [Atot,7] (Atot = ncls*H*W*A), mask [B,Atot] u8.  Keeps anchors with mask && max-class
 *   sigmoid score > thr, in ascending anchor order; applies the direction flip.
 *   out: guided [B,capK,7], labels [B,capK] i32, scores [B,capK] f32 (rpn score, extra), counts [B] i32.
 * ---------------------------------------------------------------------------------------------- */
size_t sassd_decode_filter_workspace_bytes(int batch, int n_anchors_total);
int sassd_decode_filter(const float *box, const float *cls, const float *dir, size_t batch_stride,
                        int batch, int num_class, int anchors_per_loc, int H, int W,
                        const float *anchors, const uint8_t *mask, float thr, float *guided,
                        int32_t *labels, float *scores, int32_t *counts, int capK, int32_t *status,
                        void *workspace, size_t workspace_bytes, void *stream);

/* (a12) PSWarpHead sampling (ssd_rotate_head.py:374-414,438-442): feat [B,parts,H,W] (parts = 4*7),
 * guided [B,capK,7], counts [B] -> logits [B,capK] = mean_k bilinear(feat[k], grid point k). */
int sassd_pswarp_sample(const float *feat, int batch, int H, int W, const float *guided,
                        const int32_t *counts, int capK, float grid_off_x, float grid_off_y,
                        float spatial_scale, float *logits, void *stream);

/* The part-sensitive head at the pixels sassd_pswarp_sample reads, and nowhere else.
 *
 * sassd_ps_pixel_list: the set of pixels sassd_pswarp_sample(guided, counts, capK, offsets, scale) would read from a
 *   [B,28,H,W] map -- for every box < min(counts[b], capK) and grid point k < 28 the in-map ones of its four bilinear
 *   neighbours, by the same device function as the sampler (bit-equal geometry).  `list` is int32, 16-byte aligned,
 *   sassd_ps_pixel_list_ints(B, H, W) ints (0: unsupported shape), laid out as
 *     [0, B)                       the number of listed pixels per sample,
 *     [HEAD, HEAD + B H W)         HEAD = B rounded up to 4: per sample H W slots, the first count[b] of them the listed
 *                                  linear pixels y W + x in ascending order (the others keep stale values),
 *     behind, 4-int aligned        B x (H W rounded up to 16) flag bytes: 1 at a listed pixel, 0 elsewhere.
 *   Deterministic; three kernel launches (fill, mark, compact), no memset node, no host read; every call clears the flags
 *   itself, so nothing of an earlier call survives in counts, in the listed prefix or in the flags.
 * sassd_ps_head_sampled: y[b, :, p] = conv1x1(relu?(conv3x3(x) * scale0 + shift0)) * scale1 + shift1 at every listed pixel p
 *   of `list` (the layout above; only counts and lists are read; entries outside [0, H W) are skipped), all other pixels of
 *   y [B,parts,H,W] untouched.  x [B,Cin,H,W] fp32, w_packed from sassd_conv2d_pack_weight(ksize 3), wT the transposed
 *   [parts][CO] image of sassd_conv1x1_narrow_fwd; scale / shift pointers may be NULL (1 / 0).  The stored values are
 *   BIT-IDENTICAL to sassd_conv2d_fwd(ksize 3) followed by sassd_conv1x1_narrow_fwd at those pixels (both summation orders
 *   are repeated: csrc/conv2d.hip).  Needs Cin % 32 == 0 and parts <= 32 (sassd_ps_head_sampled_supported), list 16-byte
 *   aligned.  One launch whose grid covers the worst case, every pixel listed; no fall-back to the dense kernels. */
size_t sassd_ps_pixel_list_ints(int batch, int H, int W);
int sassd_ps_pixel_list(const float *guided, const int32_t *counts, int capK, int batch, int H, int W,
                        float grid_off_x, float grid_off_y, float spatial_scale, int32_t *list, void *stream);
int sassd_ps_head_sampled_supported(int Cin, int parts);
int sassd_ps_head_sampled(const float *x, const float *w_packed, const float *scale0, const float *shift0, int relu0,
                          const float *wT, const float *scale1, const float *shift1, int relu1, const int32_t *list,
                          float *y, int batch, int Cin, int parts, int H, int W, void *stream);

/* backward of sassd_pswarp_sample (training, PSWarpHead.loss): dlogits [B,capK] -> ACCUMULATES into dfeat [B,28,H,W]
 * (caller zeroes; float atomics) and writes dguided [B,capK,7] (d/d x,y,w,l,r; z,h columns zero; may be NULL) --
 * torch.nn.functional.grid_sample differentiates w.r.t. both input and grid (ssd_rotate_head.py:400-414). */
int sassd_pswarp_sample_bwd(const float *feat, int batch, int H, int W, const float *guided,
                            const int32_t *counts, int capK, float grid_off_x, float grid_off_y,
                            float spatial_scale, const float *dlogits, float *dfeat, float *dguided,
                            void *stream);

/* (a13+a14) get_rescore_bboxes (ssd_rotate_head.py:487-533): sigmoid, > score_thr, BEV boxes
 * (iou3d_utils.py:47-60), stable descending sort, rotated NMS (iou3d_kernel.cu:250-292 + iou3d.cpp:100-116).
 *   out_boxes [B,capD,7], out_scores [B,capD], out_labels [B,capD] i32, out_counts [B] i32. */
size_t sassd_rescore_nms_workspace_bytes(int batch, int capK);
int sassd_rescore_nms(const float *guided, const float *logits, const int32_t *labels,
                      const int32_t *counts, int batch, int capK, float score_thr, float iou_thr,
                      float *out_boxes, float *out_scores, int32_t *out_labels, int32_t *out_counts,
                      int capD, int32_t *status, void *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Box fusion (opt-in): behind sassd_rescore_nms every detection becomes the score-weighted mean of the candidates it
 * stands for -- its own box and the overlapping boxes of its label that NMS dropped -- instead of the single survivor.
 * Under test-time augmentation the candidate list is the pool of all views, so the views' boxes are averaged.  Scores,
 * labels, counts and the order of the detections are not touched; only boxes move.  (The reference keeps the survivor.)
 *
 * CONTRACT  (the rule is csrc/box_fuse_core.h; its numpy statement is sassd.fuse.fuse_host)
 *   inputs     the candidate buffers exactly as handed to sassd_rescore_nms: guided [B,capK,7] f32, logits [B,capK] f32,
 *              labels [B,capK] i32, counts [B] i32, score_thr; and the buffers it left behind: det_boxes [B,capD,7] f32,
 *              det_labels [B,capD] i32, det_counts [B] i32.  Detection d of sample b is row t < clamp(det_counts[b], 0,
 *              capD) with box B_d and label l_d; candidate j is row j < clamp(counts[b], 0, capK) with score
 *              s_j = sigmoidf(logits[j]) (csrc/sigmoid.h, the fp32 function sassd_rescore_nms thresholds and sorts by).
 *   member     candidate j is a member of d when s_j > score_thr, labels[j] == l_d and
 *              iou3d::iou_bev(bev(B_d), bev(box_j)) >= fuse_iou -- the detection first, the candidate second, bev(g) =
 *              (x - w/2, y - l/2, x + w/2, y + l/2, yaw) as sassd_rescore_nms builds it.  A NaN IoU is not a member.
 *   sums       float64, over the members in ASCENDING j, every product, quotient and sum rounded on its own (no fused
 *              multiply-add); the sum of one term is that term.  W = sum s_j;  F_q = sum s_j * f_jq for q in x, y, z, w, l,
 *              h (each product is exact);  delta_j = d - pi * floor(d / pi + 0.5) with d = yaw_j - yaw_d and float64 pi,
 *              so delta_j lies in [-pi/2, pi/2) and a candidate pointing the opposite way (a flipped view's) does not drag
 *              the heading round;  D = sum s_j * delta_j.
 *   result     fused_q = float32(F_q / W), fused_yaw = float32(double(yaw_d) + D / W).  Without a member, or when W is not a
 *              positive finite number, fused row = B_d bit for bit.  A detection whose only member is itself comes out bit
 *              for bit too, by arithmetic ((s * f) / s == f), except that a yaw of -0.0 becomes +0.0.
 *   output     fused [B,capD,7] f32, a buffer of its own (det_boxes stays readable); rows at and past the detection count
 *              are not written.
 *   launches   one kernel, no workspace: (ceil(capD / 4), B) workgroups of 4 waves, one wave per detection; the lanes take
 *              the candidates 64 at a time and ballot the members, whose terms are then added serially, lowest row first --
 *              the result is a pure function of the inputs.  No host sync, no allocation, no memset, no atomics, no
 *              workgroup waits for another.
 *   errors     SASSD_EINVAL before any HIP call: a NULL or misaligned (4 bytes) pointer, batch / capK / capD < 1, batch >
 *              65535, capK > 4096, fuse_iou not inside (0, 1) or not finite, fused overlapping det_boxes.
 * sassd_candidate_scores: scores[i] = sigmoidf(logits[i]) for i < n -- the s_j above as a tensor, for callers that state
 * the rule on the host (one kernel, one thread per element; n == 0 launches nothing).
 * ---------------------------------------------------------------------------------------------- */
int sassd_box_fuse(const float *guided, const float *logits, const int32_t *labels, const int32_t *counts, int batch,
                   int capK, float score_thr, float fuse_iou, const float *det_boxes, const int32_t *det_labels,
                   const int32_t *det_counts, int capD, float *fused, void *stream);
int sassd_candidate_scores(const float *logits, long long n, float *scores, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Tracking (opt-in): identity across the frames of a stream.  A greedy centre-distance tracker of the CenterPoint kind
 * runs as ONE kernel per frame behind the frame's detections; the tracks of every sample live in device memory between
 * the calls.  (The reference detects on single frames and has no counterpart.)
 *
 * CONTRACT  (the rule is csrc/track_core.h; its numpy statement is sassd.track.track_host)
 *   state      per sample `cap` slots (1..1024) of SASSD_TRACK_SLOT_WORDS = 14 32-bit words -- id i32 (-1: free) | label i32
 *              | box[7] f32 | vel[2] f32 (m/s, sensor frame) | hits i32 | misses i32 | score f32 -- as slots [B,cap,14], and
 *              next_id [B] i32.  The caller owns both and hands them to every call; ids are never reused, not even after
 *              a reset, as long as next_id is kept.
 *   descriptor one per sample and frame, made on the host (120 bytes, 8-byte aligned): T[3,4] f64, the transform of the
 *              previous sensor frame into the current one (exactly [I|0] without ego motion); dyaw f64 = atan2(T[1,0],
 *              T[0,0]) (exactly 0.0 for the identity); dt f64 = time_now - time_prev; flags i32, bit 0: reset; one pad word.
 *   inputs     the detection buffers a frame leaves behind: det_boxes [B,capD,7] f32, det_scores [B,capD] f32, det_labels
 *              [B,capD] i32, det_counts [B] i32, and the words at `seq` and `status`.
 *   arithmetic float64 on the float32 fields, every product, quotient and sum rounded on its own (no fused multiply-add),
 *              results stored as float32.
 *   1 reset    with flag bit 0 every slot's id becomes -1.
 *   2 predict  every live slot: px = x + vx * dt, py = y + vy * dt, pz = z;  x' = f32(((T00 px + T01 py) + T02 pz) + T03), y'
 *              and z' alike;  yaw' = f32(double(yaw) + dyaw);  v' = (f32(T00 vx + T01 vy), f32(T10 vx + T11 vy)); the sizes
 *              stay.  When the status word is not 0 the step ENDS here: the tracks have been carried into the current sensor
 *              frame, nothing else changes, every output row is empty and the count written is 0.
 *   3 match    D = clamp(det_counts[b], 0, capD).  For d = 0 .. D-1 in the detector's order: slot i is eligible when its id
 *              >= 0, it is not yet matched in this frame, its label equals the detection's, the label lies in [0, n_labels)
 *              and c_i = dx * dx + dy * dy <= double(max_dist[label])^2 with dx = double(det.x) - double(x'_i), dy alike.  A
 *              NaN cost is not eligible.  The match is the eligible slot of least cost, on equal cost the lowest slot.
 *   4 update   a matched slot: g = 1 when hits == 1, else alpha.  When dt is finite and > 0: vx = f32(double(vx') + g *
 *              ((double(det.x) - double(x')) / dt)), vy alike; otherwise the velocity stays v'.  The box and the score become
 *              the detection's, bit for bit; hits = min(hits + 1, 1 << 30), misses = 0.
 *   5 age      every live slot that was not matched: misses += 1, and id = -1 when misses > max_age.
 *   6 births   every unmatched detection with score >= birth_score, in order, takes the lowest free slot (slots freed in
 *              step 5 count): id = next_id++, the detection's box, label and score, vel = 0, hits = 1, misses = 0.  When no
 *              slot is free the detection keeps id -1 and the sample's `dropped` goes up by one.
 *   record     32-bit words, SASSD_TRACK_HEADER_WORDS = 8 in front: SASSD_TRACK_MAGIC, the word at `seq`, the status word
 *              seen, B, capD, cap, 0, 0; then count [B] (the D used), dropped [B], next_id [B], det_id [B,capD] i32, det_hits
 *              [B,capD] i32, det_vel [B,capD,2] f32, and the whole slot table [B,cap,14] after the step.  A detection's
 *              values are those of its slot after the step; rows at and past D, and detections without a track, hold
 *              -1 / 0 / (0, 0).  sassd.track.track_record_layout is the Python statement of these offsets.
 *   launches   one kernel, no workspace: B workgroups of 256 threads, the sample's table in LDS, the detections staged there 64
 *              at a time.  Per detection a block arg-min: per-thread scan, wave64 shuffle reduction, the four waves through
 *              LDS, one barrier.  Births by two
 *              block scans.  No host sync, no allocation, no memset, no atomics, no workgroup waits for another.
 *   errors     SASSD_EINVAL before any HIP call: a NULL or misaligned pointer (4 bytes; desc 8), batch / capD / cap < 1,
 *              batch > 65535, capD > 16384, cap > 1024, n_labels outside 1..8, alpha outside (0, 1], a max_dist that is
 *              negative or not finite, a negative max_age, a NaN birth_score.  SASSD_ENOSPC: record_bytes below
 *              sassd_track_record_bytes(batch, capD, cap) (0 for shapes the step refuses).  max_dist is a HOST array of
 *              n_labels floats.
 * ---------------------------------------------------------------------------------------------- */
#define SASSD_TRACK_MAGIC 0x53540001
#define SASSD_TRACK_HEADER_WORDS 8
#define SASSD_TRACK_SLOT_WORDS 14
#define SASSD_TRACK_DESC_BYTES 120
size_t sassd_track_record_bytes(int batch, int capD, int cap);
int sassd_track_step(const float *det_boxes, const float *det_scores, const int32_t *det_labels, const int32_t *det_counts,
                     int batch, int capD, const int32_t *seq, const int32_t *status, const void *desc, int32_t *slots,
                     int32_t *next_id, int cap, const float *max_dist, int n_labels, int max_age, double alpha,
                     float birth_score, void *record, size_t record_bytes, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Frame record: the LAST node of a captured frame.  sassd_frame_seal copies the detection buffers sassd_rescore_nms
 * left behind into ONE fixed-size, self-describing device record, so that a frame leaves the GPU in one asynchronous
 * copy (sassd.stream.FrameStream; the reference reads its detections with three blocking copies per sample,
 * ssd_rotate_head.py:529-531).  One kernel launch, grid sized by batch * capD, plain loads and vector stores: no
 * atomics, no memset -- a frame that ends in it still holds kernel nodes only.  It READS boxes / scores / labels /
 * counts, the word at `seq` and the word at `status`, and writes nothing but `record`.
 *
 * CONTRACT -- the record, in 32-bit little-endian words (sassd.stream.record_layout returns the same byte offsets):
 *   word 0            magic/version  SASSD_FRAME_MAGIC
 *   word 1            seq            the int32 at `seq` when the kernel ran (a captured graph bakes its kernel
 *                                    arguments, so the sequence number is staged in device memory with the inputs)
 *   word 2            status         the int32 at `status` (SASSD_ST_* bits) at the end of this frame
 *   word 3            B              batch
 *   word 4            capD
 *   words 5 .. 5+B-1  counts[B]      counts[b] clamped to 0 .. capD
 *   (zero words up to H = SASSD_FRAME_HEADER_WORDS(B) = 5 + B rounded up to a multiple of 4: the body is 16-byte
 *    aligned in a 16-byte aligned record)
 *   words H ..        boxes  [B][capD][7] f32, then scores [B][capD] f32, then labels [B][capD] i32
 * Every row at or past counts[b] is written as zero words, so the record is a pure function of the frame: two runs of
 * the same frame give the same bytes.  sassd_frame_record_bytes = 4 * (H + 9 * B * capD), 0 for an impossible shape.
 * `record` must be 4-byte aligned and record_bytes at least that size (SASSD_ENOSPC otherwise).
 * ---------------------------------------------------------------------------------------------- */
#define SASSD_FRAME_MAGIC 0x53460001                       /* 'S' 'F', layout version 1 */
#define SASSD_FRAME_HEADER_WORDS(B) ((5 + (B) + 3) / 4 * 4)
size_t sassd_frame_record_bytes(int batch, int capD);
int sassd_frame_seal(const float *boxes, const float *scores, const int32_t *labels, const int32_t *counts,
                     int batch, int capD, const int32_t *seq, const int32_t *status, void *record,
                     size_t record_bytes, void *stream);

/* ------------------------------------------------------------------------------------------------
 * KITTI annotations: what kitti_common.kitti_bbox2results computes per frame on the host -- the camera-frame result
 * annotation of every detection whose projection meets the image -- as one more kernel node of the captured frame.
 * sassd_frame_annos READS boxes [B][capD][7] f32 (x, y, z, w, l, h, yaw; lidar frame), counts [B] and the calibration
 * block, and writes nothing but `annos`.  One launch, one workgroup per sample, plain loads and vector stores: no
 * atomics, no memset.
 *
 * Calibration block: per sample 36 float64 -- Tr_velo_to_cam [3][4], R0_rect [3][3], P2 [3][4], img_w, img_h, one pad.
 *
 * ARITHMETIC (csrc/kitti_anno_core.h states it once, for the kernel and for the CPU harness of the tests; products are
 * rounded separately, every sum is associated left to right):
 *   yaw'        = yaw - floor(yaw / 2pi + 0.5) * 2pi                      float32, 2pi rounded to float32
 *   location    = R0 . (V2C . [x y z 1])                                  float64, rounded to float32
 *   dimensions  = (l, h, w);  rotation_y = yaw'
 *   corners     = ((+-0.5, {-1, 0}, +-0.5) * (l, h, w)) rotated about the camera y axis by yaw' (float32 sin / cos),
 *                 plus the float32 location                               float32
 *   (u, v, w)   = P2 . [X Y Z 1] per corner, u / w and v / w              float64
 *   bbox        = min u, min v, max u, max v over the eight corners       float64
 *   alpha       = -atan2(-y, x) + yaw'                                    float32
 *   keep        = !(x1 > img_w || y1 > img_h || x2 < 0 || y2 < 0)
 *   clip        = x1, y1 to >= 0;  x2 to <= img_w;  y2 to <= img_h
 * A box with corners at or behind the image plane gets NO special case: the formula is applied as written, as the host
 * function applies it (a negative w mirrors the corner, w == 0 gives an infinite coordinate).  The min / max are plain
 * comparisons, so a NaN coordinate (non-finite input) is ignored where numpy would propagate it.
 *
 * CONTRACT -- the annotation block, in 32-bit words from its 8-byte aligned start, n = B * capD:
 *   kept  [B] i32          annotation rows of sample b; one zero word follows when B is odd
 *   index [B][capD] i32    the detection row each annotation row came from, ascending (stable compaction: score order)
 *   cam   [B][capD][7] f32 x, y, z, l, h, w, rotation_y
 *   alpha [B][capD] f32    one zero word follows when n is odd, so that
 *   bbox  [B][capD][4] f64 is 8-byte aligned
 * counts[b] is clamped to 0 .. capD as in the frame record; every row at or past kept[b] is written as zero words, so the
 * block is a pure function of the frame.  sassd_frame_annos_bytes is its size, 0 for an impossible shape.  `calib` and
 * `annos` must be 8-byte aligned, boxes / counts 4-byte aligned (SASSD_EINVAL); annos_bytes at least the size
 * (SASSD_ENOSPC).
 *
 * Frame record, layout version 2 (additive; version 1 is unchanged): SASSD_FRAME_MAGIC_KITTI in word 0, the version 1
 * header and body as above, zero bytes up to the next 8-byte boundary, then the annotation block -- one buffer, one
 * copy to the host.  sassd_frame_seal_kitti writes it (two kernel launches: the seal, then sassd_frame_annos on the same
 * boxes / counts); `record` must be 8-byte aligned and record_bytes at least sassd_frame_record_kitti_bytes
 * (= sassd_frame_record_bytes rounded up to 8, plus sassd_frame_annos_bytes).
 * ---------------------------------------------------------------------------------------------- */
#define SASSD_FRAME_MAGIC_KITTI 0x53460002                 /* 'S' 'F', layout version 2 */
size_t sassd_frame_annos_bytes(int batch, int capD);
int sassd_frame_annos(const float *boxes, const int32_t *counts, int batch, int capD, const double *calib,
                      void *annos, size_t annos_bytes, void *stream);
size_t sassd_frame_record_kitti_bytes(int batch, int capD);
int sassd_frame_seal_kitti(const float *boxes, const float *scores, const int32_t *labels, const int32_t *counts,
                           int batch, int capD, const int32_t *seq, const int32_t *status, const double *calib,
                           void *record, size_t record_bytes, void *stream);

/* ------------------------------------------------------------------------------------------------
 * iou3d_cuda operator surface (mmdet/ops/iou3d/src/iou3d.cpp:31,52,73; kernels iou3d_kernel.cu:223-292).
 * boxes (x1,y1,x2,y2,ry) f32.  nms: boxes sorted by descending score; keep [n] i64 and num_keep are DEVICE
 * buffers (the reference fills a CPU LongTensor after a blocking D2H of the mask, iou3d.cpp:92-94).
 * ---------------------------------------------------------------------------------------------- */
int sassd_boxes_overlap_bev(const float *boxes_a, int num_a, const float *boxes_b, int num_b,
                            float *ans_overlap, void *stream);
int sassd_boxes_iou_bev(const float *boxes_a, int num_a, const float *boxes_b, int num_b,
                        float *ans_iou, void *stream);
size_t sassd_nms_workspace_bytes(int n);
int sassd_nms_gpu(const float *boxes, int n, float thresh, int64_t *keep, int32_t *num_keep,
                  void *workspace, size_t workspace_bytes, void *stream);
/* iou3d_cuda.nms_normal_gpu (iou3d.cpp:123-172, iou3d_kernel.cu:295-348): the same greedy suppression over the
 * axis-aligned IoU of the (x1,y1,x2,y2) rectangles, rotation ignored.  Same arguments / workspace as sassd_nms_gpu. */
int sassd_nms_normal_gpu(const float *boxes_sorted, int n, float thresh, int64_t *keep, int32_t *num_keep,
                         void *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------------------------------
 * (a16, a17) training-side point operators of the auxiliary network.
 * pointnet2_cuda (mmdet/ops/pointnet2/src/interpolate.cpp:13,25,40; kernels interpolate_gpu.cu:9-146):
 *   three_nn            unknown [N,4] (b,x,y,z), known [M,4] -> dist2 [N,3] f32 (squared), idx [N,3] i32: the three
 *                       nearest known points of the same batch index, first index wins ties
 *   three_interpolate   points [M,C], idx, weight [N,3] -> out [N,C]
 *   three_interpolate_grad  grad_out [N,C] -> ACCUMULATES into grad_points [M,C] (caller zeroes it; float atomics,
 *                       like the reference interpolate_gpu.cu:143-145)
 * points_op_cpu (mmdet/ops/points_op/src/points_op.cpp:107-144):
 *   pts_in_boxes3d      pts [N,3], boxes3d [M,7] -> pts_flag [M,N] i32 (fully written), reg_target [N,3] f32
 *                       (only rows of points inside a box are written: caller zeroes, as points_op/__init__.py:8-9)
 * ---------------------------------------------------------------------------------------------- */
int sassd_three_nn(int n, int m, const float *unknown, const float *known, float *dist2, int32_t *idx,
                   void *stream);
/* Exact accelerated variant: the known points are counting-sorted into a uniform BEV grid (batch, y, x) of
 * `cell`-sized columns starting at (x0, y0) with nx * ny cells per batch element (coordinates outside are clamped
 * into the border cells), and each query scans rings of cells until its 3rd best distance is provably final.
 * Results are bit-identical to sassd_three_nn for ANY inputs (same ranking by (distance,row), same fp32 distance
 * arithmetic); cost ~O((N+M) * points-per-neighbourhood) instead of O(N*M).  Batch indices must be 0..batch_size-1;
 * nx*ny*batch_size <= 2^20. */
size_t sassd_three_nn_binned_workspace_bytes(int m, int nx, int ny, int batch_size);
int sassd_three_nn_binned(int n, int m, const float *unknown, const float *known, float x0, float y0, float cell,
                          int nx, int ny, int batch_size, float *dist2, int32_t *idx, void *workspace,
                          size_t workspace_bytes, void *stream);
int sassd_three_interpolate(int c, int m, int n, const float *points, const int32_t *idx, const float *weight,
                            float *out, void *stream);
int sassd_three_interpolate_grad(int c, int n, int m, const float *grad_out, const int32_t *idx,
                                 const float *weight, float *grad_points, void *stream);
int sassd_pts_in_boxes3d(const float *pts, int n, const float *boxes3d, int m, int32_t *pts_flag,
                         float *reg_target, void *stream);

/* ------------------------------------------------------------------------------------------------
 * (f-2) KITTI-evaluation rotated IoU.  Replaces `rotate_iou_gpu_eval(boxes, query_boxes, criterion, device_id)` of
 * mmdet/core/post_processing/rotate_nms_gpu.py:594-627 (numba.cuda kernel :548-591, device functions :153-388), called
 * by mmdet/core/evaluation/kitti_eval.py for the BEV / 3-D overlap matrices.
 *   boxes [n,5], query_boxes [k,5] f32 device: (cx, cy, x_dim, y_dim, angle);  iou [n,k] f32 device
 *   iou[i][j] = inter / (area_q + area_b - inter)  (criterion -1),  inter / area(query j) (0),  inter / area(box i) (1),
 *               inter (anything else) -- the reference's argument order devRotateIoUEval(query, box).
 * ---------------------------------------------------------------------------------------------- */
int sassd_rotate_iou_eval(const float *boxes, int n, const float *query_boxes, int k, int criterion, float *iou,
                          void *stream);

/* (f-2) KITTI-evaluation matching statistics -- HOST function (no device memory, no stream): the greedy
 * ground-truth <-> detection assignment is sequential per image and negligible next to the overlap matrices above.
 * Replaces `compute_statistics_jit` (mmdet/core/evaluation/kitti_eval.py:165-283, numba CPU) and the loop over images x
 * score thresholds `fused_compute_statistics` (:296-343) for ONE part of the image list (eval_class_v3 :598-648).
 *   overlaps [sum dt, ld] f64 host, row-major: overlap of detection j with ground truth i; image p owns the block
 *            rows [sum_{q<p} dt_nums[q], +dt_nums[p]) x columns [sum_{q<p} gt_nums[q], +gt_nums[p]);  ld >= sum gt
 *   gt_datas [sum gt,5] (bbox x1 y1 x2 y2, alpha)   dt_datas [sum dt,6] (bbox, alpha, score)   dontcares [sum dc,4]
 *   ignored_gts [sum gt] / ignored_dets [sum dt] int64: 0 counted, 1 neutral, -1 other class (clean_data :39-93)
 *   metric 0 image bbox (detections inside DontCare boxes are not false positives), 1 BEV, 2 3-D
 *   n_thr == 0: first pass (compute_fp=False, thresh 0): tp_scores[<= sum gt] receives the score of every matched
 *               detection in image order, *n_tp_scores their count;  pr (optional, [4]) += (tp, 0, fn, 0)
 *   n_thr  > 0: pr [n_thr,4] f64 += (tp, fp, fn, sum over true positives of (1+cos(alpha_gt-alpha_dt))/2 when
 *               compute_aos) per threshold; detections scoring under thresholds[t] are left out
 * Returns SASSD_EINVAL for negative counts, metric outside 0..2, ld < sum gt or a missing output array. */
int sassd_kitti_eval_statistics(const double *overlaps, int64_t ld, int n_img, const int64_t *gt_nums,
                                const int64_t *dt_nums, const int64_t *dc_nums, const double *gt_datas,
                                const double *dt_datas, const double *dontcares, const int64_t *ignored_gts,
                                const int64_t *ignored_dets, int metric, double min_overlap, const double *thresholds,
                                int n_thr, int compute_aos, double *pr, double *tp_scores, int64_t *n_tp_scores);

/* ------------------------------------------------------------------------------------------------
 * (f-4) Training-side augmentation and offline data preparation.  The reference runs these as numba CPU loops inside
 * DataLoader workers (mmdet/core/point_cloud/point_augmentor.py, mmdet/core/bbox3d/geometry.py, tools/create_data.py).
 * Device entry points work in place on a point cloud that is already in HBM ([n, stride] f32 rows, xyz first).
 * ---------------------------------------------------------------------------------------------- */

/* `points_in_convex_polygon_3d_jit(points, surfaces)` geometry.py:189-227, the core of `points_in_rbbox` (:63-74, called
 * from kitti.py:222, create_data.py:43,221) and of `remove_outside_points` (:50-61, camera-frustum reduction).
 *   planes [m,6,4] f64 device: (nx, ny, nz, d) of each polytope's 6 surfaces, as `surface_equ_3d_jit` (:176-186) gives
 *   them -- the caller builds them from the box / frustum corners with the reference's own numpy arithmetic;
 *   f32_math != 0: the plane values are float32 numbers (float32 boxes) and the sign is evaluated in float32, as the
 *   reference's dtype rules make it;  mask [n,m] u8 device: 1 when no surface gives n.p + d >= 0. */
int sassd_points_in_polytopes(const float *points, int n, int stride, const double *planes, int m, int f32_math,
                              uint8_t *mask, void *stream);

/* `points_transform_(points, centers, point_masks, loc_transform, rot_transform, valid_mask)` point_augmentor.py:44-62:
 * every point inside a valid box is rotated about that box's centre and shifted with it (first such box wins).
 *   mask [n,m] u8, valid [m] u8, centers [m,3] f32, rot_sin / rot_cos [m] f32 (float64 sine / cosine of the accepted yaw
 *   noise rounded to float32, the entries of the reference's float32 rotation matrix), loc [m,3] f64 -- all device. */
int sassd_points_transform(float *points, int n, int stride, const uint8_t *mask, int m, const uint8_t *valid,
                           const float *centers, const float *rot_sin, const float *rot_cos, const double *loc,
                           void *stream);

/* `random_flip` + `global_rotation` + `global_scaling` on the points, one pass (point_augmentor.py:279-303):
 * y -> -y if flip; [x y z] @ [[c,-s,0],[s,c,0],[0,0,1]]; xyz *= scale. */
int sassd_points_global_transform(float *points, int n, int stride, int flip, float rot_sin, float rot_cos, float scale,
                                  void *stream);

/* The points of the sampled ground-truth objects (`PointAugmentor.sample_all` point_augmentor.py:232-242: np.fromfile
 * per object, += box centre, -= road-plane correction) gathered from a database that is RESIDENT IN HBM.
 *   db_points [P,4] f32;  src_start [n_obj] i64 first database row of object k;  out_start [n_obj+1] i64 prefix sums of
 *   the objects' point counts (out_start[n_obj] == n_out);  shift [n_obj,3] f64;  lower [n_obj] f64 or NULL;
 *   out [n_out,4] f32 -- all device. */
int sassd_paste_objects(const float *db_points, const int64_t *src_start, const int64_t *out_start, int n_obj,
                        int64_t n_out, const double *shift, const double *lower, float *out, void *stream);

/* The same gather for a database of `ndim` floats per point, ndim 3..8 (clouds with a time column, extra returns, ...):
 *   db_points [P,ndim] f32 and out [n_out,ndim] f32, both dense (row stride = ndim floats); every other argument as above.
 * Columns 0..2 are (float)((double)src + shift[k][c]), and column 2 is rounded a second time as
 * (float)((double)z - lower[k]) when `lower` is given -- the arithmetic of sassd_paste_objects; columns 3..ndim-1 are
 * copied bit for bit (NaN payloads, -0.0 and denormals included).  At ndim == 4 the output bytes are those of
 * sassd_paste_objects.  An object of zero points repeats its out_start; row r belongs to the largest k with
 * out_start[k] <= r.  The caller guarantees src_start[k] + count_k <= P.
 * Returns SASSD_EINVAL for a negative count, ndim outside 3..8 or a missing array, SASSD_OK without a launch when
 * n_obj == 0 or n_out == 0 -- all decided before anything is launched. */
int sassd_paste_objects_nd(const float *db_points, int ndim, const int64_t *src_start, const int64_t *out_start,
                           int n_obj, int64_t n_out, const double *shift, const double *lower, float *out, void *stream);

/* HOST functions (no device memory, no stream): the sequential O(boxes^2 x tries) decisions.
 * `box_collision_test(boxes, qboxes)` geometry.py:593-672: boxes [n,4,2], qboxes [k,4,2] corner arrays (float64 when
 * is_f64, else float32) -> out [n,k] u8; edge crossings and full containment both count (numba evaluates the
 * reference's `ret[i, j] is False` as an equality test).
 * `noise_per_box(boxes, valid_mask, loc_noises, rot_noises)` point_augmentor.py:73-105: boxes [n,5] f32 (x, y, w, l, yaw),
 * valid [n] u8, loc_noises [n,num_try,3] f64, rot_noises [n,num_try] f64 -> success [n] i64: index of the first draw
 * that keeps box i clear of all others (accepted draws move the box for the later tests), -1 if none / not valid. */
int sassd_box_collision_test(const void *boxes, int n, const void *qboxes, int k, int is_f64, uint8_t *out);
int sassd_noise_per_box(const float *boxes, const uint8_t *valid, const double *loc_noises, const double *rot_noises,
                        int n, int num_try, int64_t *success);

/* ---- training: parameter update ------------------------------------------------------------------------------------
 * Replaces tools/train_utils/__init__.py:57-61 (clip_grad_norm_ + optimizer.step) for optimizer type 'adam_onecycle'
 * (tools/train_utils/optimization/__init__.py:17-30, fastai_optim.py:132-148): decoupled weight decay on every
 * parameter, then Adam(betas=(mom, 0.99), eps, weight_decay=0) -- over one flat fp32 buffer.
 * sassd_grad_sumsq: out[0] = sum(grad^2) (device float, zeroed by the call).
 * sassd_adam_step:  g' = grad * grad_scale * min(1, max_norm / (sqrt(sumsq) * grad_scale + 1e-6)) when grad_sumsq is
 *                   non-NULL and max_norm > 0 (torch clip_grad_norm_ semantics), else grad * grad_scale;
 *                   p *= 1 - wd*lr; m,v Adam moments; p -= lr/(1-b1^t) * m / (sqrt(v)/sqrt(1-b2^t) + eps).
 *                   `step` is t >= 1.  All pointers 16-byte aligned.
 * The other two optimizer types of optimization/__init__.py:9-16 take the same g' (the clip acts on the raw gradient,
 * before weight decay, as clip_grad_norm_ does in front of optimizer.step()) over the same flat buffers:
 * sassd_adam_l2_step: 'adam' = torch Adam(weight_decay): g = g' + wd*p; m, v, and the bias-corrected update as above
 *                   on g; there is no p *= 1 - wd*lr.  Same arguments and checks as sassd_adam_step.
 * sassd_sgd_step:   'sgd' = torch SGD(momentum, weight_decay), no dampening, no Nesterov: g = g' + wd*p;
 *                   buf = momentum*buf + g; p -= lr*buf.  A zero-initialised buffer gives torch's first step
 *                   (buf = g).  12 B read + 8 B written per element.
 * Both: SASSD_EINVAL for a NULL or not 16-byte aligned param / grad / state pointer and for n < 0. */
/* Training-mode BatchNorm1d + ReLU of the sparse blocks (cmn.py:147-173: SubMConv3d / SparseConv3d -> BatchNorm1d(eps
 * 1e-3, momentum 0.01) -> ReLU) over features x [n, C] row-major, two launches each way instead of torch's six.
 *   fwd: y = relu((x - mean) * invstd * gamma + beta) with batch statistics (biased variance); save_mean / save_invstd [C]
 *        are kept for the backward pass; running_mean / running_var (both or neither) are updated like torch (momentum,
 *        unbiased variance).
 *   bwd: dx, dgamma, dbeta from dy (gradient with respect to y) and the saved statistics.
 * C % 4 == 0, 256 % C == 0.  Deterministic: block partials in double, reduced in a fixed order by every block of the
 * second launch (no inter-workgroup hand-off inside a launch).  Workspace: sassd_bn_relu_workspace_bytes(C). */
size_t sassd_bn_relu_workspace_bytes(int C);
int sassd_bn_relu_fwd(const float *x, int n, int C, const float *gamma, const float *beta, float *running_mean,
                      float *running_var, float momentum, float eps, float *y, float *save_mean, float *save_invstd,
                      void *workspace, size_t workspace_bytes, void *stream);
int sassd_bn_relu_bwd(const float *x, const float *dy, int n, int C, const float *gamma, const float *beta,
                      const float *save_mean, const float *save_invstd, float *dx, float *dgamma, float *dbeta,
                      void *workspace, size_t workspace_bytes, void *stream);

/* Training-mode BatchNorm2d + ReLU over NCHW maps x [B, C, H*W] (the BEV stack cmn.py:233-282 and the part-sensitive head
 * ssd_rotate_head.py:424-429: Conv2d -> BatchNorm2d(eps 1e-3, momentum 0.01) -> ReLU), replacing torch's MIOpen BatchNorm +
 * clamp / threshold_backward + MIOpen backward (four passes over the map each way) by two launches each way; same
 * contract as sassd_bn_relu_* with the channel as the SECOND dimension.  HW % 4 == 0, 16-byte aligned tensors.
 * Deterministic (double partials per (channel, split), added in a fixed order by every block of the second launch).
 * Workspace: sassd_bn2d_relu_workspace_bytes(C). */
size_t sassd_bn2d_relu_workspace_bytes(int C);
int sassd_bn2d_relu_fwd(const float *x, int B, int C, int HW, const float *gamma, const float *beta, float *running_mean,
                        float *running_var, float momentum, float eps, float *y, float *save_mean, float *save_invstd,
                        void *workspace, size_t workspace_bytes, void *stream);
/* Statistics only: mean / invstd / running statistics exactly as sassd_bn2d_relu_fwd computes them, plus the affine triple
 * [3][C] = mean | invstd * gamma | beta for consumers that apply BatchNorm + ReLU themselves (sassd_conv2d_bf16_bnrelu_fwd,
 * sassd_conv2d_bwd_weight_bf16_bnrelu); the backward is sassd_bn2d_relu_bwd on the raw map. */
int sassd_bn2d_stats(const float *x, int B, int C, int HW, const float *gamma, const float *beta, float *running_mean,
                     float *running_var, float momentum, float eps, float *save_mean, float *save_invstd, float *affine,
                     void *workspace, size_t workspace_bytes, void *stream);
int sassd_bn2d_relu_bwd(const float *x, const float *dy, int B, int C, int HW, const float *gamma, const float *beta,
                        const float *save_mean, const float *save_invstd, float *dx, float *dgamma, float *dbeta,
                        void *workspace, size_t workspace_bytes, void *stream);

/* The guided-anchor / rescoring tail of the training step on padded tensors with device counts (train_heads.hip):
 *   sassd_guided_decode_fwd  ssd_rotate_head.py:316-388 (train mode): guided[b] = [ground truth of sample b (gt_boxes rows
 *                            gt_off[b] .. gt_off[b+1]); decoded + direction-flipped boxes of the anchors sel[b][0 .. sel_count[b])
 *                            (second_box_decode :53-91, flip :352-356); zeros] as [B, gmax + cap, 7]; counts[b] = G_b +
 *                            min(sel_count[b], cap).  anchors [A,7] (anchors_per_sample 0) or [B,A,7] (1); dir_preds may be NULL.
 *   sassd_guided_decode_bwd  dbox [B,A,7] (zeroed here) <- dguided through the decode (selected anchors only).
 *   sassd_boxes_iou3d_batch  iou3d_utils.py:79-111 boxes_iou3d_gpu of boxes [B, rows, 7] (rows < counts[b] valid, the rest
 *                            give 0) against each sample's ground truth; sample b's [rows, G_b] matrix starts at element
 *                            ov_off[b] of `overlaps` (the layout sassd_assign_targets takes as `overlaps`).
 *   sassd_focal_loss         losses.py:35-62 sigmoid focal loss (gamma 2, alpha .25) of logits [n] against labels [n]
 *                            (-1 ignore / 0 / > 0), weight 1 / max(sum(num_pos[0..nb)), 1): loss_sum[0] and grad [n]. */
int sassd_guided_decode_fwd(const float *box_preds, const float *dir_preds, const float *anchors, int anchors_per_sample,
                            const int64_t *sel, const int32_t *sel_count, const float *gt_boxes, const int32_t *gt_off,
                            int A, int B, int cap, int gmax, float *guided, int32_t *counts, void *stream);
int sassd_guided_decode_bwd(const float *box_preds, const float *anchors, int anchors_per_sample, const int64_t *sel,
                            const int32_t *sel_count, const int32_t *gt_off, int A, int B, int cap, int gmax,
                            const float *dguided, float *dbox, void *stream);
int sassd_boxes_iou3d_batch(const float *boxes, const int32_t *counts, int B, int rows, const float *gt_boxes,
                            const int32_t *gt_off, int gmax, const int64_t *ov_off, float *overlaps, void *stream);
size_t sassd_focal_loss_workspace_bytes(int n);
int sassd_focal_loss(const float *logits, const int64_t *labels, int n, const int32_t *num_pos, int nb, float *loss_sum,
                     float *grad, void *workspace, size_t workspace_bytes, void *stream);

/* The auxiliary point-wise head of SpMiddleFHD in training, fused (cmn.py:27-29 point_fc / point_cls / point_reg, :45-72
 * build_aux_target, :74-104 aux_loss, :121-135,175-189 nearest_neighbor_interpolate, transforms.py:218-223 tensor2points):
 *   sassd_aux_prepare   points [N,4] = (b, voxel mean xyz); voxel centres known[s] [M_s,4] of the three middle tensors
 *                       (indices [M_s,4] (b,z,y,x); centre = idx * vs_s + offset + vs_s / 2 with vs_s = 2, 4, 8 x voxel_size,
 *                       evaluated in the reference's fp32 order); per-point label (inside any ground-truth box of the
 *                       point's own sample: points_op.cpp:92-144 semantics, gt_boxes [T,7] + gt_off [B+1]) and centre
 *                       offsets of the LAST containing box; npos[0] = number of positive points.
 *   (the three 3-NN searches between points and known[s] stay sassd_three_nn_binned calls)
 *   sassd_aux_head_fwd  per point: inverse-distance weights from nn_d2[s] [N,3], interpolation of feats[s] [M_s, C_s]
 *                       (C = 32, 64, 64) at nn_idx[s] [N,3], h = f W1^T (W1 [64,160]), out = h W2^T (W2 [4,64]: point_cls
 *                       row, then the three point_reg rows); loss_sums[0] = sum of the sigmoid focal terms / max(npos, 1),
 *                       loss_sums[1] = sum over positives of smooth-L1(beta 1/9) / max(npos, 1); gout [N,4] = their
 *                       gradients with respect to out.  Keeps wgt [N,9], h [N,64] for the backward pass.
 *   sassd_aux_head_bwd  grad_sums [2] (device) = upstream gradients of the two sums -> grad_feats[s] [M_s, C_s]
 *                       (zeroed here, accumulated with float atomics like the reference's three_interpolate_grad),
 *                       dw1 [64,160], dw2 [4,64] (per-workgroup partials, fixed-order reduction).
 * Workspace (both): sassd_aux_head_workspace_bytes(N). */
size_t sassd_aux_head_workspace_bytes(int N);
int sassd_aux_prepare(const float *voxel_feats, int vstride, const int32_t *coors, int N, const int32_t *const *indices,
                      const int *M, const float *voxel_size, const float *offset, const float *gt_boxes,
                      const int32_t *gt_off, int B, float *points, float *const *known, uint8_t *label, float *target,
                      int *npos, void *stream);
int sassd_aux_head_fwd(int N, const float *const *feats, const int32_t *const *nn_idx, const float *const *nn_d2,
                       const float *w1, const float *w2, const uint8_t *label, const float *target, const int *npos,
                       float *wgt, float *h, float *out, float *gout, float *loss_sums, void *workspace,
                       size_t workspace_bytes, void *stream);
int sassd_aux_head_bwd(int N, const float *const *feats, const int *M, const int32_t *const *nn_idx, const float *w1,
                       const float *w2, const float *wgt, const float *h, const float *gout, const float *grad_sums,
                       float *const *grad_feats, float *dw1, float *dw2, void *workspace, size_t workspace_bytes,
                       void *stream);

/* dst[i] = map[i] >= 0 ? src[map[i]] : 0 for i < n; dst fp32, or bf16 (round-to-nearest-even) when bf16 != 0: every
 * kernel-layout weight image is a permutation (+ zero padding) of the flat parameter buffer, so ONE gather re-packs all
 * of them after an optimizer step (sassd.train.PackPlan). */
int sassd_gather_pack(const float *src, const int32_t *map, void *dst, long n, int bf16, void *stream);
int sassd_grad_sumsq(const float *grad, long n, float *out, void *stream);
int sassd_adam_step(float *param, const float *grad, float *exp_avg, float *exp_avg_sq, long n,
                    const float *grad_sumsq, float lr, float beta1, float beta2, float eps, float weight_decay,
                    int step, float max_norm, float grad_scale, void *stream);
int sassd_adam_l2_step(float *param, const float *grad, float *exp_avg, float *exp_avg_sq, long n,
                       const float *grad_sumsq, float lr, float beta1, float beta2, float eps, float weight_decay,
                       int step, float max_norm, float grad_scale, void *stream);
int sassd_sgd_step(float *param, const float *grad, float *momentum_buf, long n, const float *grad_sumsq, float lr,
                   float momentum, float weight_decay, float max_norm, float grad_scale, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Deterministic training (opt-in: train_cfg['deterministic'] or torch.use_deterministic_algorithms(True)).
 * The default training path sums four gradients with float atomics, so two runs of the same seeded workload differ in
 * the last bits and drift apart over many steps.  These `_det` twins fix every summation order, so that a step is
 * bit-reproducible and a CPU model can recompute their results bit for bit.  The mode switches exactly these launches:
 * the aux-head scatter (sassd_aux_head_bwd), the PSWarp backward (sassd_pswarp_sample_bwd), the gradient-norm square
 * sum of the clip (sassd_grad_sumsq) and the reference-surface three_interpolate_grad.  Everything else on the training
 * path already reduces in a fixed order.  The twins contain no float atomics; their integer atomics only count list
 * lengths or place entries that are sorted afterwards.  They issue no hipMemsetAsync (capture-safe).
 *
 * 3-NN interpolation gradient (sassd_three_interpolate_grad_det; sassd_aux_head_bwd_det per level):
 *   grad[r, ch] = the value on entry (0 for the aux head, grad_points as passed for three_interpolate_grad), then
 *   t = fl(g[p, ch] * w[p, j]) added one at a time, fl(acc + t), for every (p, j) with idx[p, j] == r in ascending
 *   (p, j) order.  fp32, each product rounded before it is added (no FMA contraction).  Each (row, channel) sum is
 *   sequential; only rows and channels run in parallel.  Entries with idx outside [0, m) are ignored.  For the aux head,
 *   g = d(interpolated features) of the point pass and w the interpolation weights of the forward.  dw1 / dw2 of
 *   sassd_aux_head_bwd_det are bit-identical to sassd_aux_head_bwd's (already a fixed-order reduction).
 * PSWarp backward (sassd_pswarp_sample_bwd_det): dfeat[b, k, y, x] = its value on entry, then the tap values of
 *   sassd_pswarp_sample_bwd for that pixel (go * wx * wy, evaluated left to right) added in ascending box index over
 *   boxes < min(counts[b], capK).  dguided is bit-identical to sassd_pswarp_sample_bwd's.  Any capK (the taps are sorted
 *   in LDS 512 boxes at a time); the workspace query returns 0 today and ws may then be NULL.
 * Gradient square sum (sassd_grad_sumsq_det): the summation order depends on n only (not on CU count, occupancy or
 *   launch timing): min(1024, max(1, ceil(n / 1024))) block partials in fp32 (optim.hip spells out the order), summed
 *   by one workgroup in double.  *out is WRITTEN, not accumulated.  Within 1e-6 relative of a float64 sum.
 * Workspaces are caller-owned, sized by the queries (host arithmetic; 0 for impossible shapes); short -> SASSD_ENOSPC. */
size_t sassd_three_interpolate_grad_det_workspace_bytes(int n, int m);
int sassd_three_interpolate_grad_det(int c, int n, int m, const float *grad_out, const int32_t *idx,
                                     const float *weight, float *grad_points, void *ws, size_t ws_bytes, void *stream);
size_t sassd_aux_head_bwd_det_workspace_bytes(int N, const int *M);
int sassd_aux_head_bwd_det(int N, const float *const *feats, const int *M, const int32_t *const *nn_idx,
                           const float *w1, const float *w2, const float *wgt, const float *h, const float *gout,
                           const float *grad_sums, float *const *grad_feats, float *dw1, float *dw2, void *workspace,
                           size_t workspace_bytes, void *stream);
size_t sassd_pswarp_sample_bwd_det_workspace_bytes(int batch, int capK);
int sassd_pswarp_sample_bwd_det(const float *feat, int batch, int H, int W, const float *guided,
                                const int32_t *counts, int capK, float grid_off_x, float grid_off_y,
                                float spatial_scale, const float *dlogits, float *dfeat, float *dguided, void *ws,
                                size_t ws_bytes, void *stream);
size_t sassd_grad_sumsq_det_workspace_bytes(long n);
int sassd_grad_sumsq_det(const float *grad, long n, float *out, void *ws, size_t ws_bytes, void *stream);

/* Hardware self-test helper used by tests: D = A(32x2k) * B(2k x32) through v_mfma_f32_32x32x2_f32 and
 * D = A(16x4k) * B(4k x16) through v_mfma_f32_16x16x4_f32 with the lane maps the kernels assume. */
int sassd_mfma_probe(const float *a32, const float *b32, float *d32, const float *a16, const float *b16,
                     float *d16, int ksteps, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SASSD_H */
