/*
 * unidistill_hip.h -- C ABI of libunidistill_hip.so (MI355X / gfx950).
 *
 * One shared library sits underneath the Python names the UniDistill reference
 * imports for its BEV feature-extraction + distillation hot path.  Every entry
 * point takes plain device pointers + sizes + a hipStream_t, never a torch type,
 * returns 0 on success or a negative UD_ERR_* code, and never throws.
 * All pointers are DEVICE pointers unless a parameter is documented "host".
 * Kernels are enqueued on `stream`; nothing in here synchronises the device.
 *
 * Reference interface each group replaces (paths relative to the reference tree,
 * /root/reference/unidistill/...):
 *
 *   ud_bev_pool_*      voxel_pooling_ext.voxel_pooling_forward_wrapper
 *                      layers/blocks_3d/mmdet3d/lss_fpn.py:48-59 (fwd), :64-79 (bwd)
 *   ud_lss_*           LSSFPN.get_geometry / binning / lift
 *                      layers/blocks_3d/mmdet3d/lss_fpn.py:200-240, :289-316
 *   ud_voxelize*       spconv.pytorch.utils.PointToVoxel.__call__ + MeanVFE.forward
 *                      data/det3d/preprocess/voxelization.py:31-38,54
 *                      layers/blocks_3d/det3d/vfe/mean_vfe.py:14-34
 *   ud_spconv_*        spconv.pytorch.{SubMConv3d,SparseConv3d,SparseConvTensor.dense}
 *                      layers/blocks_3d/det3d/spconv_backbone.py:21-48,71-92,259-340
 *                      layers/blocks_2d/det3d/map_to_bev/height_compression.py:19-22
 *   ud_distill_*       FeatureDistillLoss / BEVDistillLoss / ResponseDistillLoss
 *                      exps/.../BEVFusion_nuscenes_centerhead_camera_exp_distill_lidar.py
 *                      :196-245, :248-323, :326-385, gaussian mask :100-178
 */
#ifndef UNIDISTILL_HIP_H
#define UNIDISTILL_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* hipStream_t is an opaque pointer; spelled void* so this header needs no HIP include. */
typedef void* ud_stream_t;

#define UD_OK 0
#define UD_ERR_INVALID_ARG (-1)
#define UD_ERR_WORKSPACE (-2) /* workspace pointer NULL or too small */
#define UD_ERR_HIP (-3)       /* a HIP runtime call / launch failed    */
#define UD_ERR_UNSUPPORTED (-4)

/* Library identity: returns "unidistill_hip <abi-version> gfx950". */
const char* ud_version(void);
/* ABI version integer; bumped whenever a signature in this header changes. */
int ud_abi_version(void);
/* Human-readable text for a UD_ERR_* code. */
const char* ud_error_string(int code);

/*
 * Optional profiler: when enabled, the library brackets its dominant kernels with hipEvents on
 * the launch stream.  ud_prof_read(name) waits for those events and returns the summed kernel
 * time in ms and the number of launches (names: "bev_pool.k_pool", "bev_pool.k_bwd", ...).
 */
void ud_prof_enable(int on);
int ud_prof_read(const char* name, double* total_ms, int* calls, int reset);

/* HBM calibration: mode 0 = streaming read of src (dst only keeps the loads alive), mode 1 = copy
 * src -> dst; n_floats elements.  Timed through ud_prof ("bench.stream_read" / "bench.stream_copy"). */
int ud_bench_stream(const float* src, float* dst, size_t n_floats, int mode, ud_stream_t stream);

/* ------------------------------------------------------------------------- */
/* BEV pool (camera LSS splat)                                               */
/* ------------------------------------------------------------------------- */

/* flags for ud_bev_pool_fwd */
#define UD_POOL_ACCUMULATE 0u /* out += pooled sums; caller pre-zeroed out (reference contract, lss_fpn.py:43-47) */
#define UD_POOL_OVERWRITE 1u  /* every cell of out is written (empty cells get 0); no pre-zero needed             */

/* Bytes of scratch ud_bev_pool_fwd needs for these sizes (0 on invalid sizes). */
size_t ud_bev_pool_workspace_bytes(int B, int N, int C, int nx, int ny, int nz);

/*
 * out[b, y, x, :] (+)= sum over points n of batch b with geom[b,n]=(x,y,z) inside
 * 0<=x<nx, 0<=y<ny, 0<=z<nz of feat[b,n,:];  pos[b,n,:] = (b,y,x) for kept points,
 * (-1,-1,-1) otherwise.  Sums run in ascending point index n (deterministic; the
 * reference CUDA op used unordered atomicAdd).
 *   geom  i32[B,N,3]   feat f32[B,N,C]   out f32[B,ny,nx,C]   pos i32[B,N,3]
 */
int ud_bev_pool_fwd(const int32_t* geom, const float* feat, float* out, int32_t* pos,
                    int B, int N, int C, int nx, int ny, int nz, unsigned flags,
                    void* workspace, size_t workspace_bytes, ud_stream_t stream);

/*
 * gfeat[b,n,:] = gout[b,:,y,x] for pos[b,n]=(b,y,x) != -1, else 0   (lss_fpn.py:64-79).
 * gout is addressed through element strides (sb, sc, sy, sx) so both the NCHW grad the
 * reference produces and an NHWC (channels-last) grad are accepted; NHWC (sc == 1) is the
 * fast path, anything else is transposed into `workspace` first
 * (ud_bev_pool_bwd_workspace_bytes).
 */
size_t ud_bev_pool_bwd_workspace_bytes(int B, int C, int nx, int ny, int64_t sc);
int ud_bev_pool_bwd(const float* gout, int64_t sb, int64_t sc, int64_t sy, int64_t sx,
                    const int32_t* pos, float* gfeat, int B, int N, int C, int nx, int ny,
                    void* workspace, size_t workspace_bytes, ud_stream_t stream);

/* ------------------------------------------------------------------------- */
/* Camera lift-splat (LSS): geometry, depth softmax, lift, fused lift+splat  */
/* ------------------------------------------------------------------------- */

/*
 * mats[b*ncam+cam] = { inverse(ida), sensor2ego @ inverse(intrin), bda }  f32[B*ncam,3,16]
 * (lss_fpn.py:221-222,233,235-239).  sensor2ego/intrin/ida f32[B,ncam,4,4]; bda f32[B,4,4] or NULL.
 * ida_inv / intrin_inv f32[B,ncam,4,4]: the fp32 inverses as the caller's torch.inverse produced
 * them (the reference's own call; its rounding depends on the LAPACK/solver backend), or NULL for
 * the correctly rounded inverse computed in fp64 in the kernel.  Every product is evaluated as the
 * reference's CPU path does (acc = 0; acc += a[k]*b[k], fp32, no FMA), so with the reference's
 * inverses the ego coordinates and bins of ud_lss_geometry are bit-identical to its CPU output.
 */
int ud_lss_prepare_mats(const float* sensor2ego, const float* intrin, const float* ida,
                        const float* bda, const float* ida_inv, const float* intrin_inv, int B,
                        int ncam, float* mats, ud_stream_t stream);

/*
 * LSSFPN.get_geometry + binning (lss_fpn.py:200-240, :311-313) for every frustum point
 * (b, cam, d, h, w): geom f32[B,ncam,D,fH,fW,3] (optional, NULL to skip) and
 * bins i32[B,ncam,D,fH,fW,3] = ((geom - lo) / size).int()  with host lo/size f32[3]
 * (lo = voxel_coord - voxel_size/2 evaluated in fp32 by the caller).  frustum_u[fW], frustum_v[fH],
 * frustum_d[D] are the device vectors of create_frustum (lss_fpn.py:173-198).
 */
int ud_lss_geometry(const float* mats, const float* frustum_u, const float* frustum_v,
                    const float* frustum_d, int B, int ncam, int D, int fH, int fW,
                    const float* lo, const float* size, int has_bda, float* geom, int32_t* bins,
                    ud_stream_t stream);

/*
 * depth_feature f32[BN, D+C, fH, fW] addressed by element strides (sn, sc, sh, sw) ->
 *   prob   f32[BN, D, fH*fW]   softmax over the first D channels (lss_fpn.py:289)
 *   ctx_pm f32[BN, fH*fW, C]   context channels D..D+C, pixel-major
 */
int ud_lss_depth_ctx(const float* depth_feature, int64_t sn, int64_t sc, int64_t sh, int64_t sw,
                     int BN, int D, int C, int fH, int fW, float* prob, float* ctx_pm,
                     ud_stream_t stream);

/* Materialised lift (reference boundary, lss_fpn.py:290-310):
 * lifted f32[BN, D, fH*fW, C] = prob (x) ctx  == img_feat_with_depth.permute(0,1,3,4,5,2). */
int ud_lss_lift_fwd(const float* prob, const float* ctx_pm, float* lifted, int BN, int D, int C,
                    int fH, int fW, ud_stream_t stream);

/*
 * Fused lift + splat forward (a7-a9): out[b,y,x,:] = sum over points of prob[point] *
 * ctx_pm[pixel(point), :], in ascending point order; the [B,N,C] tensor is never formed.
 * geom i32[B,N,3] with N = ncam*D*fH*fW; out f32[B,ny,nx,C] (every cell written);
 * pos i32[B,N,3] as ud_bev_pool_fwd.  Workspace: ud_bev_pool_workspace_bytes(B,N,C,nx,ny,nz).
 */
int ud_lss_splat_fwd(const int32_t* geom, const float* prob, const float* ctx_pm, float* out,
                     int32_t* pos, int B, int ncam, int D, int fH, int fW, int C, int nx, int ny,
                     int nz, void* workspace, size_t workspace_bytes, ud_stream_t stream);

/*
 * ud_lss_splat_fwd with the binning computed from the frustum inside the list-building kernel (the arithmetic of
 * ud_lss_geometry: mats / frustum axes / lo / size / has_bda as there): what LSSFPN._forward_single_sweep
 * (lss_fpn.py:277-319) needs from get_geometry is only the bins, so the training step never materialises them.
 * out, pos and the workspace as ud_lss_splat_fwd; bit-identical to ud_lss_geometry followed by ud_lss_splat_fwd.
 */
int ud_lss_splat_geom_fwd(const float* mats, const float* frustum_u, const float* frustum_v,
                          const float* frustum_d, const float* lo, const float* size, int has_bda,
                          const float* prob, const float* ctx_pm, float* out, int32_t* pos, int B, int ncam,
                          int D, int fH, int fW, int C, int nx, int ny, int nz, void* workspace,
                          size_t workspace_bytes, ud_stream_t stream);

/*
 * Backward of softmax (x) context.  pos == NULL: gsrc is the dense grad of the materialised
 * lifted tensor f32[BN, D, fH*fW, C].  pos != NULL (fused splat backward): gsrc is the dense NHWC
 * BEV grad f32[B, ny, nx, C] and each point gathers its cell's row through pos i32[B*N,3].
 * Writes g_depth_feature f32[BN, D+C, fH, fW] through element strides (sn, sc, sh, sw).
 */
size_t ud_lss_lift_bwd_workspace_bytes(int BN, int D, int C, int fH, int fW);
int ud_lss_lift_bwd(const float* gsrc, const int32_t* pos, const float* prob, const float* ctx_pm,
                    float* g_depth_feature, int64_t sn, int64_t sc, int64_t sh, int64_t sw, int BN,
                    int ncam, int D, int C, int fH, int fW, int nx, int ny, void* workspace,
                    size_t workspace_bytes, ud_stream_t stream);

/* ------------------------------------------------------------------------- */
/* LiDAR voxelization (+ fused MeanVFE)                                      */
/* ------------------------------------------------------------------------- */

/*
 * Replaces spconv.pytorch.utils.PointToVoxel.__call__ (voxelization.py:31-38,54) for a whole
 * collated batch and, optionally fused, MeanVFE.forward (mean_vfe.py:14-34).
 *   points      f32[B,N,F]  (F >= 3: x,y,z first; clouds padded to a common N like collate_fn)
 *   voxel_size  host f32[3] (x,y,z);  range host f32[6] (xmin,ymin,zmin,xmax,ymax,zmax)
 *   P           max points kept per voxel;  max_voxels  cap PER SAMPLE
 * Outputs hold ud_voxelize_capacity(B,N,max_voxels) rows; rows [0, m_out[B]) are valid:
 *   voxels      f32[cap,P,F] zero padded, or NULL to skip materialising it (fused path)
 *   coords      i32[cap,4]  (b, z, y, x)
 *   num_points  i32[cap] or NULL;  mean_feats f32[cap,F] or NULL (sum over slots / max(num,1))
 *   m_out       i32[B+2]    voxels per sample, then the total, then the overflow word (device memory)
 *   algo        0: hash partition + per-partition LDS sort, no global atomics (the fast path; if one partition
 *                  receives more than 3 072 points -- thousands of points in a single voxel -- it sets the overflow
 *                  word m_out[B+1] = 1, the outputs are then invalid and the call must be repeated with algo 1);
 *               1: open-addressing hash with device-scope atomics (any input).  Both give the same bits.
 * Deterministic: voxel order = first appearance in the point list, kept points = the first P in
 * input order, no voxel created beyond max_voxels per sample (oracle/ud_oracle.c:oracle_voxelize).
 */
size_t ud_voxelize_workspace_bytes(int B, int N, int P, int max_voxels);
int ud_voxelize_capacity(int B, int N, int max_voxels);
int ud_voxelize(const float* points, int B, int N, int F, const float* voxel_size,
                const float* range, int P, int max_voxels, float* voxels, int32_t* coords,
                int32_t* num_points, float* mean_feats, int32_t* m_out, void* workspace,
                size_t workspace_bytes, int algo, ud_stream_t stream);

/* ------------------------------------------------------------------------- */
/* Sparse 3-D convolution (spconv boundary) + densify                        */
/* ------------------------------------------------------------------------- */

/*
 * Site index of one level: a rank bitmap over the (B, Dz, Hy, Wx) voxel grid (spconv_index.hip).
 * coords are i32[M,4] = (b, z, y, x) like SparseConvTensor.indices (spconv_backbone.py:354-359).
 * rows_sorted != 0 promises that row i is the i-th site in ascending (b,z,y,x) order (true for
 * the outputs of ud_spconv_down_outputs); otherwise a rank->row permutation is built.
 */
size_t ud_spconv_index_bytes(int B, int Dz, int Hy, int Wx, int M);
int ud_spconv_build_index(const int32_t* coords, int M, int B, int Dz, int Hy, int Wx,
                          int rows_sorted, void* index, size_t index_bytes, ud_stream_t stream);

/* SubMConv3d rulebook (odd kernel, implicit padding k/2): nbr i32[M, kz*ky*kx] = row of the
 * active site at coord + (k - centre) or -1.  Offsets enumerate z slowest, x fastest. */
int ud_spconv_subm_rulebook(const void* index, int rows_sorted, const int32_t* coords, int M,
                            int B, int Dz, int Hy, int Wx, int kz, int ky, int kx, int32_t* nbr,
                            ud_stream_t stream);

/*
 * SparseConv3d(kernel, stride, padding) output sites = every cell reachable from an active
 * input; ksize/stride/pad are host int[3] in (z, y, x) order; the output grid is
 * floor((in + 2p - k)/s) + 1 per axis.  Builds the OUTPUT level's index (rows sorted), writes
 * out_coords i32[out_cap,4] in ascending (b,z,y,x) order and the count into m_out (device int).
 */
int ud_spconv_down_outputs(const int32_t* in_coords, int Min, int B, int Dz, int Hy, int Wx,
                           const int* ksize, const int* stride, const int* pad, void* out_index,
                           size_t out_index_bytes, int32_t* out_coords, int out_cap,
                           int32_t* m_out, ud_stream_t stream);
/* Device-count variants: the row count of the input site set is read from device memory (the launches cover the upper
 * bound M_cap / Min_cap), so ud_voxelize -> level index -> the four down-sampling levels of VoxelResBackBone8x
 * (spconv_backbone.py:279-340) chain without a host read in between; ONE read of all counts sizes the tensors afterwards. */
int ud_spconv_build_index_dev(const int32_t* coords, const int32_t* m_dev, int M_cap, int B, int Dz, int Hy, int Wx,
                              int rows_sorted, void* index, size_t index_bytes, ud_stream_t stream);
int ud_spconv_down_outputs_dev(const int32_t* in_coords, const int32_t* min_dev, int Min_cap, int B, int Dz, int Hy,
                               int Wx, const int* ksize, const int* stride, const int* pad, void* out_index,
                               size_t out_index_bytes, int32_t* out_coords, int out_cap, int32_t* m_out,
                               ud_stream_t stream);

/* out_nbr i32[Mout,K]: input row at o*s - p + k or -1; in_nbr i32[Min,K] (optional, for dgrad):
 * output row that input i feeds through offset k, or -1. */
int ud_spconv_down_rulebook(const void* in_index, int in_rows_sorted, int Min, int B, int Dz,
                            int Hy, int Wx, const int* ksize, const int* stride, const int* pad,
                            const int32_t* out_coords, int Mout, int32_t* out_nbr,
                            int32_t* in_nbr, ud_stream_t stream);

/*
 * out f32[Mout,Cout] = bias + sum_k sum_c in[nbr[o][k], c] * W[n*w_sn + k*w_sk + c*w_sc].
 * Forward with spconv-2.x KRSC weights [Cout,K,Cin]: (w_sn, w_sk, w_sc) = (K*Cin, Cin, 1).
 * Input gradient: in := gout, nbr := in_nbr (strided conv) or the subm rulebook with mirror = 1,
 * (w_sn, w_sk, w_sc) = (1, Cin, K*Cin), Cin/Cout swapped.  Exact-fp32 MFMA, deterministic.
 * algo 0 = auto (128-row MFMA kernel), 1 = generic VALU kernel (any channel counts),
 * 2 = first-generation 64-row MFMA kernel, 3 = bf16-input MFMA with fp32 accumulation
 * (mixed-precision mode: operands are rounded to bf16 in LDS; tensors in HBM stay fp32).
 * Fused epilogue (MFMA kernel, algo 0): y = relu?((conv + bias) * ep_scale + ep_shift + ep_residual)
 * with ep_scale/ep_shift f32[Cout] (a folded eval-mode BatchNorm1d; both or neither),
 * ep_residual f32[Mout,Cout] (a SparseBasicBlock skip), ep_relu 0/1; pass NULL/0 to disable.
 * row_order (optional, may be NULL): a permutation i32[Mout] of the output rows; tiles are formed
 * over row_order so rows with similar neighbour masks share a tile (same results, fewer active
 * kernel offsets per tile; only the wide-channel MFMA kernel uses it).
 * Size limit: `in` must be smaller than 4 GiB - 64 KiB (0xFFFF0000 bytes): the 64 / 128-channel fp32 kernel addresses the gathered
 * rows with 32-bit byte offsets through a buffer descriptor (the entry point is not told the input's row count).
 */
int ud_spconv_conv(const float* in, const int32_t* nbr, const float* W, int64_t w_sn, int64_t w_sk,
                   int64_t w_sc, int mirror, const float* bias, float* out, int Mout, int K,
                   int Cin, int Cout, int algo, const int32_t* row_order, const float* ep_scale,
                   const float* ep_shift, const float* ep_residual, int ep_relu, ud_stream_t stream);

/* gW f32[Cout,K,Cin] = sum_o gout[o,n] * in[nbr[o][k], c]  (ordered partial sums, deterministic). */
/* Mixed-precision weight gradient (training under bf16 autocast): operands rounded to bf16 when the
 * 64-row tiles are staged, fp32 accumulation on v_mfma_f32_16x16x32_bf16, ordered reduction of the row
 * chunks (deterministic).  row_order (optional) is the forward kernel's row permutation; tiles that
 * have no pair for an offset are skipped.  K <= 32.  gW f32[Cout,K,Cin].  io_bf16 bit 0: `in` and `gout`
 * already hold bf16 rows (Cin, Cout % 8 == 0); otherwise they are fp32.  Bit 1 (with bit 0, row_order and
 * tile_masks; Cin, Cout in {32, 64, 128}, else UD_ERR_UNSUPPORTED): `nbr` and `tile_masks` are ALREADY permuted
 * into row_order and row_order only locates the gout rows -- spares the caller a gather pass over gout. */
size_t ud_spconv_wgrad_bf16_workspace_bytes(int Mout, int K, int Cin, int Cout);
int ud_spconv_wgrad_bf16(const void* in, const int32_t* nbr, const void* gout, float* gW, int Mout,
                         int K, int Cin, int Cout, int io_bf16, const int32_t* row_order,
                         const unsigned* tile_masks, void* workspace, size_t workspace_bytes,
                         ud_stream_t stream);
/* tile_masks (optional, u32[ceil(Mout/64)]): bit k set iff some row of the 64-row tile (in row_order) has
 * a pair at offset k; computed internally when NULL.  It depends on the rulebook only. */
int ud_spconv_tile_masks(const int32_t* nbr, int Mout, int K, const int32_t* row_order, unsigned* masks,
                         ud_stream_t stream);
/* Row order of a rulebook for the kernels above (`row_order`): rows sorted (stable) by their neighbour bit mask, the bit of
 * offset k weighted by its rarity among ~4 096 sampled rows (rarest on top).  order: i32[Mout].  K <= 31. */
size_t ud_spconv_mask_order_workspace_bytes(int Mout, int K);
int ud_spconv_mask_order(const int32_t* nbr, int Mout, int K, int32_t* order, void* workspace, size_t workspace_bytes,
                         ud_stream_t stream);
/* Mixed-precision inference variant: the bf16-operand MFMA kernel (algo 3 above) with bf16 tensors in
 * HBM so the gather moves half the bytes.  io_flags bit 0: `in` is bf16 [*, Cin] (Cin % 4 == 0);
 * bit 1: `out` and `ep_residual` are bf16 [Mout, Cout]; bit 2: `W` is bf16 (w_sc == 1).  K <= 32. */
int ud_spconv_conv_bf16io(const void* in, const int32_t* nbr, const void* W, int64_t w_sn,
                          int64_t w_sk, int64_t w_sc, int mirror, const float* bias, void* out,
                          int Mout, int K, int Cin, int Cout, int io_flags, const int32_t* row_order,
                          const float* ep_scale, const float* ep_shift, const void* ep_residual,
                          int ep_relu, ud_stream_t stream);
size_t ud_spconv_wgrad_workspace_bytes(int Mout, int K, int Cin, int Cout);
int ud_spconv_wgrad(const float* in, const int32_t* nbr, const float* gout, float* gW, int Mout,
                    int K, int Cin, int Cout, int algo, void* workspace, size_t workspace_bytes,
                    ud_stream_t stream);

/* SparseConvTensor.dense() (height_compression.py:19): dense f32[B,C,Dz,Hy,Wx], every element written
 * once (feature or zero; the caller need not clear it), and its backward gather
 * gfeat[row,:] = gdense[b,:,z,y,x].  workspace: ud_sparse_bev_workspace_bytes(B,Dz,Hy,Wx) (cell -> row map).
 * B*Dz*Hy <= 65535. */
int ud_sparse_to_dense(const float* feat, const int32_t* coords, int M, int C, int B, int Dz,
                       int Hy, int Wx, float* dense, void* workspace, size_t workspace_bytes,
                       ud_stream_t stream);
int ud_dense_to_sparse(const float* gdense, const int32_t* coords, int M, int C, int B, int Dz,
                       int Hy, int Wx, float* gfeat, void* workspace, size_t workspace_bytes,
                       ud_stream_t stream);
/* HeightCompression in the mixed-precision path (reference layers/blocks_2d/det3d/map_to_bev/
 * height_compression.py:19-22: dense() then view(N, C*D, H, W)): bev bf16[B,Hy,Wx,C*Dz] (channels-last,
 * channel = c*Dz + z) straight from feat bf16[M,C], zeros where no voxel; and its backward. (C*Dz) % 4 == 0. */
size_t ud_sparse_bev_workspace_bytes(int B, int Dz, int Hy, int Wx);
int ud_sparse_to_bev_bf16(const void* feat, const int32_t* coords, int M, int C, int B, int Dz, int Hy,
                          int Wx, void* bev, void* workspace, size_t workspace_bytes, ud_stream_t stream);
int ud_bev_to_sparse_bf16(const void* gbev, const int32_t* coords, int M, int C, int B, int Dz, int Hy,
                          int Wx, void* gfeat, void* workspace, size_t workspace_bytes, ud_stream_t stream);
/* fp32 twin (the reference's arithmetic): the channels-last fp32 BEV map in one pass instead of dense() + an NCHW -> NHWC copy. */
int ud_sparse_to_bev_f32(const float* feat, const int32_t* coords, int M, int C, int B, int Dz, int Hy, int Wx, float* bev,
                         void* workspace, size_t workspace_bytes, ud_stream_t stream);
int ud_bev_to_sparse_f32(const float* gbev, const int32_t* coords, int M, int C, int B, int Dz, int Hy, int Wx, float* gfeat,
                         void* workspace, size_t workspace_bytes, ud_stream_t stream);

/* ------------------------------------------------------------------------- */
/* Distillation losses (feature / relation / response) + gaussian box mask   */
/* ------------------------------------------------------------------------- */

/*
 * training_step's box prep on the device (distill_lidar.py:449-455, :466-483, :73-97):
 * gt f32[B,M,S>=7] (x,y,z,dx,dy,dz,yaw,...) -> corners_px f32[B,M,4,2] = rotated BEV corners in
 * BEV pixels ((corner - pc_min) / pixel), valid u8[B,M] = 1 for rows up to the last non-zero row.
 */
int ud_distill_box_corners(const float* gt, int B, int M, int S, double pc_min_x, double pc_min_y,
                           double pixel_x, double pixel_y, float* corners_px, unsigned char* valid,
                           ud_stream_t stream);

/*
 * kind 0 = FeatureDistillLoss (distill_lidar.py:196-245), kind 1 = BEVDistillLoss (:248-323).
 * s / t: student / teacher BEV maps [B,C,H,W] addressed through host element strides
 * int64[4] = (sb, sc, sy, sx).  Forward writes box_loss f32[B,M] (per-box loss, 0 for invalid boxes;
 * the scalar loss is sum(box_loss) / (reduce_mean(n_valid) + 1e-4)).  Backward writes
 * (*gscale) * d sum(box_loss)/ds into the pre-zeroed gs (gscale: DEVICE scalar): per-(box, key point, channel) gradients
 * into `workspace` (>= ud_distill_box_bwd_workspace_bytes), then a sorted, atomic-free scatter of the overlapping bilinear
 * footprints (fixed summation order: bitwise reproducible).  M <= 56.
 */
int ud_distill_box_fwd(int kind, const float* s, const int64_t* s_strides, const float* t,
                       const int64_t* t_strides, const float* corners_px,
                       const unsigned char* valid, int B, int M, int C, int H, int W,
                       float* box_loss, ud_stream_t stream);
size_t ud_distill_box_bwd_workspace_bytes(int B, int M, int C);
int ud_distill_box_bwd(int kind, const float* s, const int64_t* s_strides, const float* t,
                       const int64_t* t_strides, const float* corners_px,
                       const unsigned char* valid, int B, int M, int C, int H, int W,
                       const float* gscale, float* gs, const int64_t* gs_strides,
                       void* workspace, size_t workspace_bytes, ud_stream_t stream);
/* ud_distill_box_bwd ADDED to gs instead of written into a zeroed gs: gs already holds the gradient the feature map received from
 * its other consumer; only the pixels the boxes touch are read and written (deterministic).  Replaces the zero fill + autograd's
 * dense add of the two maps in the student's backward. */
int ud_distill_box_bwd_acc(int kind, const float* s, const int64_t* s_strides, const float* t,
                           const int64_t* t_strides, const float* corners_px,
                           const unsigned char* valid, int B, int M, int C, int H, int W,
                           const float* gscale, float* gs, const int64_t* gs_strides,
                           void* workspace, size_t workspace_bytes, ud_stream_t stream);

/* calculate_box_mask_gaussian (distill_lidar.py:100-178) on the device: mask f32[B,H,W]. */
size_t ud_distill_mask_workspace_bytes(int B, int M);
int ud_distill_gaussian_mask(const float* gt, int B, int M, int S, double pc_min_x,
                             double pc_min_y, double pixel_x, double pixel_y, int H, int W,
                             float* mask, void* workspace, size_t workspace_bytes,
                             ud_stream_t stream);

/*
 * ResponseDistillLoss (distill_lidar.py:326-385).  HOST arrays of DEVICE pointers: n_hm heat-map
 * tensors [B,hm_ch[i],H,W] (student: probabilities as produced by the head's clamped sigmoid;
 * teacher: logits, turned into clamp(sigmoid(x/2), lo, hi)) and n_reg regression tensors
 * [B,reg_ch[i],H,W], all dense NCHW.  Forward: partial f32[B*ceil(H*W/256), 2] per-workgroup sums
 * of (|max_c s - max_c t| * mask, mean_c|s - t| * mask).  Backward writes every element of the
 * student-side grads; gscale_* are device scalars.
 */
int ud_distill_resp_fwd(const float* const* s_hm, const float* const* t_hm, const int* hm_ch,
                        int n_hm, const float* const* s_reg, const float* const* t_reg,
                        const int* reg_ch, int n_reg, const float* mask, int B, int H, int W,
                        float clamp_lo, float clamp_hi, float* partial, ud_stream_t stream);
int ud_distill_resp_bwd(const float* const* s_hm, const float* const* t_hm, float* const* g_hm,
                        const int* hm_ch, int n_hm, const float* const* s_reg,
                        const float* const* t_reg, float* const* g_reg, const int* reg_ch,
                        int n_reg, const float* mask, int B, int H, int W, float clamp_lo,
                        float clamp_hi, const float* gscale_cls, const float* gscale_reg,
                        ud_stream_t stream);
/* The same two passes with every tensor read / written in place through an (sb, sc, sp) element-stride triple (batch, channel,
 * linearised pixel; stride(H) == W * stride(W)): channels-last maps and channel slices of the packed CenterHead output need no dense
 * NCHW copies.  *_st: host int64[n][3]. */
int ud_distill_resp_fwd_strided(const float* const* s_hm, const int64_t* s_hm_st, const float* const* t_hm,
                                const int64_t* t_hm_st, const int* hm_ch, int n_hm, const float* const* s_reg,
                                const int64_t* s_reg_st, const float* const* t_reg, const int64_t* t_reg_st, const int* reg_ch,
                                int n_reg, const float* mask, int B, int H, int W, float clamp_lo, float clamp_hi, float* partial,
                                ud_stream_t stream);
int ud_distill_resp_bwd_strided(const float* const* s_hm, const int64_t* s_hm_st, const float* const* t_hm,
                                const int64_t* t_hm_st, float* const* g_hm, const int64_t* g_hm_st, const int* hm_ch, int n_hm,
                                const float* const* s_reg, const int64_t* s_reg_st, const float* const* t_reg,
                                const int64_t* t_reg_st, float* const* g_reg, const int64_t* g_reg_st, const int* reg_ch,
                                int n_reg, const float* mask, int B, int H, int W, float clamp_lo, float clamp_hi,
                                const float* gscale_cls, const float* gscale_reg, ud_stream_t stream);

/* ---- Detection-head tail: BatchNorm -> ReLU -> per-head 3x3 conv (64 -> k) --------------------------
 * Replaces modules 1..3 of every SepHead stack (reference unidistill/layers/head/det3d/
 * center_head.py:311-362: nn.Sequential(Conv 64->64, BatchNorm2d, ReLU, Conv 64->k)) for all
 * G = tasks x heads packed heads at once, on the hidden tensor produced by the packed first conv.
 *   y, dy : [B][H][W][G*64] bf16, channels-last.          z, dz : [B][G*kmax][H][W] fp32.
 *   w2, dw2 : [G][kmax][9][64] fp32 (tap = ky*3 + kx), rows j >= a head's real k are zero.
 *   per-channel vectors (gamma, beta, mean, var, invstd, scale, shift, dgamma, dbeta): fp32 [G*64].
 * kmax <= 3 (UD_ERR_UNSUPPORTED otherwise).  BN + ReLU are applied while tiles are staged, the conv
 * multiplies bf16 operands with fp32 accumulation (same arithmetic as the bf16 autocast library path).
 *   ud_head_tail_stats : training-mode batch statistics of y -> mean, biased var, invstd and the
 *                        folded scale = gamma*invstd, shift = beta - mean*scale.  When running_mean /
 *                        running_var are given (both or neither) they are updated in place like
 *                        nn.BatchNorm2d does: r = (1-momentum)*r + momentum*{mean, unbiased var};
 *                        batches_tracked (optional, int64 on the device) is incremented by one.
 *   ud_head_tail_fwd   : z = conv(relu(y*scale + shift), w2) + b2   (any scale/shift: batch or running).
 *   ud_head_tail_bwd   : training-mode backward through conv, ReLU and BatchNorm: dy, dw2, dgamma,
 *                        dbeta (db2 = sum of dz is left to the caller).  Deterministic. */
size_t ud_head_tail_workspace_bytes(int G);
int ud_head_tail_stats(const void* y, int B, int H, int W, int G, const float* gamma,
                       const float* beta, float eps, float* mean, float* var, float* invstd,
                       float* scale, float* shift, float* running_mean, float* running_var,
                       float momentum, long long* batches_tracked, void* workspace,
                       size_t workspace_bytes, ud_stream_t stream);
int ud_head_tail_fwd(const void* y, const float* scale, const float* shift, const float* w2,
                     const float* b2, float* z, int B, int H, int W, int G, int kmax,
                     ud_stream_t stream);
int ud_head_tail_bwd(const void* y, const float* dz, const float* w2, const float* scale,
                     const float* shift, const float* mean, const float* invstd, void* dy,
                     float* dw2, float* dgamma, float* dbeta, int B, int H, int W, int G, int kmax,
                     void* workspace, size_t workspace_bytes, ud_stream_t stream);

/* fp32 mode (the reference's arithmetic) of the second SepHead convolutions (center_head.py:311-362): a grouped
 * 3x3 / pad-1 convolution with 64 inputs and KM <= 4 outputs per group on channels-last fp32 tensors, exact fp32
 * FMAs, HBM-bound streaming kernels (the libraries run it as a 42x padded block-diagonal conv).
 *   a  f32 [B][H][W][G*64]   hidden tensor after BatchNorm + ReLU        w  f32 [G][KM][9][64] (tap = ky*3+kx)
 *   z  f32 [B][H][W][G*KM]   = bias[G*KM] + conv                          dz same layout as z
 *   dgrad: da [B][H][W][G*64];  wgrad: dw [G][KM][9][64], fixed-order slice reduction (deterministic). */
int ud_head_tail_f32_fwd(const float* a, const float* w, const float* bias, float* z, int B, int H, int W, int G,
                         int KM, ud_stream_t stream);
int ud_head_tail_f32_dgrad(const float* dz, const float* w, float* da, int B, int H, int W, int G, int KM,
                           ud_stream_t stream);
size_t ud_head_tail_f32_wgrad_workspace_bytes(int B, int H, int W, int G, int KM);
int ud_head_tail_f32_wgrad(const float* a, const float* dz, float* dw, int B, int H, int W, int G, int KM,
                           void* workspace, size_t workspace_bytes, ud_stream_t stream);
/* The same second convolutions reading the first convolution's RAW output: relu(a * scale + shift) -- the BatchNorm of the SepHead
 * (center_head.py:341-350) folded per channel [G*64] -- is applied to every piece as it is loaded, in the forward and in the weight
 * gradient; the normalised 1.39 GB hidden tensor is never written or read back. */
int ud_head_tail_f32_bn_fwd(const float* a, const float* bn_scale, const float* bn_shift, const float* w, const float* bias,
                            float* z, int B, int H, int W, int G, int KM, ud_stream_t stream);
int ud_head_tail_f32_bn_wgrad(const float* a, const float* bn_scale, const float* bn_shift, const float* dz, float* dw, int B,
                              int H, int W, int G, int KM, void* workspace, size_t workspace_bytes, ud_stream_t stream);
/* ud_head_tail_f32_bn_fwd for a consumer that weights every site by mask f32 [B][H][W] (the frozen distillation teacher): z is
 * the dense result where mask > 0 and exactly 0 elsewhere.  strip_rows [strips][2] = the (first, end) image rows of each strip
 * (16 columns x ud_head_tail_f32_strip_rows rows, index (b * strips_down + sy) * strips_across + sx) that hold a site, end <=
 * first for none, from ud_head_sites_build: a workgroup walks those rows only and writes zeros to the rest of its strip without
 * reading a.  Of a, only the sites with mask > 0 and their eight neighbours are needed. */
int ud_head_tail_f32_strip_rows(int B, int H, int W, int G, int KM);
int ud_head_tail_f32_bn_fwd_sites(const float* a, const float* bn_scale, const float* bn_shift, const float* w, const float* bias,
                                  float* z, int B, int H, int W, int G, int KM, const float* mask, const int* strip_rows,
                                  ud_stream_t stream);
/* One launch: mask f32 [B][H][W] -> the work lists of the two launches above, on the device, in ascending index order.
 *   conv_units  i32 [1 + blocks]   count, then the blk_w x blk_h pixel blocks whose rectangle, grown by one pixel (the tail is a
 *                                  3x3 convolution), holds a site with mask > 0
 *   tail_strips i32 [1 + strips]   count, then the strip_w x strip_h pixel strips that hold such a site
 *   tail_rows   i32 [strips][2]    (first, end) image rows of those sites per strip, (0, 0) for none
 *   scratch     i32 [1 + blocks + strips], zero on entry */
int ud_head_sites_build(const float* mask, int B, int H, int W, int blk_w, int blk_h, int strip_w, int strip_h, int* conv_units,
                        int* tail_strips, int* tail_rows, int* scratch, ud_stream_t stream);
/* Backward of relu(bn(y)) -> second convolutions down to y in two passes that RECOMPUTE the tail's data gradient instead of
 * storing it: dgamma / dbeta [G*64] (training-mode statistics: mean / invstd of y, folded scale / shift) and dy [B, H, W, G*64].
 * dy_colsum (optional, [G*64]): the per-channel sums of the dy values stored, in a fixed order -- the bias gradient of the
 * convolution that produced y (center_head.py:339 bias=True), emitted by the pass that writes dy instead of a third pass over it. */
size_t ud_head_tail_f32_bn_bwd_workspace_bytes(int B, int H, int W, int G, int KM);
int ud_head_tail_f32_bn_bwd(const float* dz, const float* w, const float* y, const float* bn_scale, const float* bn_shift,
                            const float* mean, const float* invstd, float* dy, float* dgamma, float* dbeta, float* dy_colsum,
                            int B, int H, int W, int G, int KM, void* workspace, size_t workspace_bytes, ud_stream_t stream);
/* Column sums of a channels-last tensor, out[c] = sum_p x[p * ld + c] (ld >= C elements between rows): the bias gradient of a
 * convolution = the sum of its output gradient over batch and pixels (reference: autograd of nn.Conv2d(bias=True),
 * center_head.py:64,339,353; lss_fpn.py:160 depth net).  Two HBM-rate passes, fixed summation order (deterministic); any C
 * (16-byte vector loads when C % 8 == 0 and the rows are 16-byte aligned). */
size_t ud_colsum_workspace_bytes(int C);
int ud_colsum_f32(const float* x, long long P, int C, long long ld, float* out, void* workspace, size_t workspace_bytes,
                  ud_stream_t stream);
int ud_colsum_bf16(const void* x, long long P, int C, long long ld, float* out, void* workspace, size_t workspace_bytes,
                   ud_stream_t stream);

/* ---- Dense 3x3 / stride 1 / pad 1 convolution, channels-last bf16 (BEV trunk + head convs) ----------
 * Replaces nn.Conv2d(k=3, s=1, p=1) of BaseBEVBackbone (reference unidistill/layers/blocks_2d/det3d/
 * base_bev_backbone.py:30-110) and CenterHead.shared_conv (layers/head/det3d/center_head.py:408-420)
 * when tensors are bf16 channels-last: x [B][H][W][Cin], w [Cout][9][Cin] (tap = ky*3+kx),
 * y [B][H][W][Cout]; fp32 accumulation on the MFMA pipe.  Optional fused epilogue, in this order:
 * + bias[Cout], * scale + shift (folded eval BatchNorm), + residual (bf16, y's layout), ReLU.
 * Cin % 64 == 0 and Cout % 8 == 0, else UD_ERR_UNSUPPORTED.  The data gradient of the convolution is
 * the same call on dy with w' [Cin][9][Cout], w'[c][8 - tap][n] = w[n][tap][c] -- or with the un-flipped
 * w'[c][tap][n] = w[n][tap][c] and bit 1 of `relu` set (walk the taps in reverse).  `relu`: bit 0 = ReLU. */
int ud_conv3x3_nhwc_bf16(const void* x, const void* w, void* y, int B, int H, int W, int Cin, int Cout,
                         const float* bias, const float* scale, const float* shift,
                         const void* residual, int relu, ud_stream_t stream);
/* 1x1 / stride-1 convolution (the ResNet bottleneck 1x1 convs of the reference's image branch) on the same
 * kernel family: x [P][Cin] bf16 (P = B*H*W channels-last pixels), w [Cout][Cin] bf16, y [P][Cout] bf16,
 * same fused epilogue (bit 0 of `relu` only).  The data gradient is the same call on dy with w^T
 * [Cin][Cout].  Cin % 64 == 0, Cout % 8 == 0, else UD_ERR_UNSUPPORTED. */
int ud_conv1x1_nhwc_bf16(const void* x, const void* w, void* y, int64_t P, int Cin, int Cout,
                         const float* bias, const float* scale, const float* shift,
                         const void* residual, int relu, ud_stream_t stream);
/* fp32 twins (the reference trains in fp32: exps/base_cli.py:40-45 has no precision flag): channels-last
 * FP32 x / w / y, exact fp32 products and fp32 accumulation on v_mfma_f32_16x16x4_f32.  Same argument
 * meaning and fused epilogue as the bf16 calls (residual is fp32, y's layout); `flags` bit 0 = ReLU, bit 1 =
 * walk the taps in reverse (data gradient on un-flipped transposed weights).  Cin % 32 == 0, Cout % 4 == 0. */
int ud_conv3x3_nhwc_f32(const float* x, const float* w, float* y, int B, int H, int W, int Cin, int Cout,
                        const float* bias, const float* scale, const float* shift, const float* residual,
                        int flags, ud_stream_t stream);
int ud_conv1x1_nhwc_f32(const float* x, const float* w, float* y, int64_t P, int Cin, int Cout,
                        const float* bias, const float* scale, const float* shift, const float* residual,
                        int flags, ud_stream_t stream);
/* Convolution (+ bias) fused with the FIRST pass of the training-mode BatchNorm that follows it in the reference's
 * Conv2d -> BatchNorm2d -> ReLU links (base_bev_backbone.py:48-66, center_head.py:408-420, the mmdet ResNet
 * bottlenecks): besides y, every workgroup writes partial[tile][Cout][2] = (sum, sum of squares) of the values it
 * stored (for bf16 the rounded ones: what a separate statistics pass would read back).  `partial_bytes` >=
 * ud_conv{3x3,1x1}_bnstats_bytes(...) (an upper bound: the tile height is chosen per launch); *slices (host int) =
 * number of tiles written.  Finish with ud_bn_stats_from_partials.  Same shape rules as the plain calls. */
size_t ud_conv3x3_bnstats_bytes(int B, int H, int W, int Cout);
size_t ud_conv1x1_bnstats_bytes(int64_t P, int Cout);
int ud_conv3x3_bnstats_nhwc_bf16(const void* x, const void* w, void* y, int B, int H, int W, int Cin, int Cout,
                                 const float* bias, float* partial, size_t partial_bytes, int* slices,
                                 ud_stream_t stream);
int ud_conv1x1_bnstats_nhwc_bf16(const void* x, const void* w, void* y, int64_t P, int Cin, int Cout,
                                 const float* bias, float* partial, size_t partial_bytes, int* slices,
                                 ud_stream_t stream);
int ud_conv3x3_bnstats_nhwc_f32(const float* x, const float* w, float* y, int B, int H, int W, int Cin, int Cout,
                                const float* bias, float* partial, size_t partial_bytes, int* slices,
                                ud_stream_t stream);
int ud_conv1x1_bnstats_nhwc_f32(const float* x, const float* w, float* y, int64_t P, int Cin, int Cout,
                                const float* bias, float* partial, size_t partial_bytes, int* slices,
                                ud_stream_t stream);
/* Weight gradient of the same convolution: dw [Cout][9][Cin] fp32 = sum over pixels of
 * dy [B][H][W][Cout] (bf16) x shifted x [B][H][W][Cin] (bf16); fp32 accumulation, fixed-order
 * reduction of pixel slices (deterministic).  Cin % 64 == 0, Cout % 8 == 0. */
size_t ud_conv3x3_wgrad_workspace_bytes(int B, int H, int W, int Cin, int Cout);
int ud_conv3x3_wgrad_nhwc_bf16(const void* x, const void* dy, float* dw, int B, int H, int W, int Cin,
                               int Cout, void* workspace, size_t workspace_bytes, ud_stream_t stream);
/* Weight gradient of a 1x1 / stride-1 convolution (reference: the ResNet bottleneck and neck 1x1 convs,
 * nn.Conv2d backward): dw [Cout][Cin] fp32 = sum over the P = B*H*W pixels of dy [P][Cout] (bf16) x
 * x [P][Cin] (bf16), channels-last rows.  Pixel-sliced MFMA GEMM with a fixed-order reduction of the
 * slices (deterministic).  Cin % 64 == 0, Cout % 8 == 0, else UD_ERR_UNSUPPORTED. */
size_t ud_conv1x1_wgrad_workspace_bytes(int64_t P, int Cin, int Cout);
int ud_conv1x1_wgrad_nhwc_bf16(const void* x, const void* dy, float* dw, int64_t P, int Cin, int Cout,
                               void* workspace, size_t workspace_bytes, ud_stream_t stream);

/* The convolutions whose im2col is a pure permutation, on the same 1x1 kernels through a pixel-address map
 * {mode, s, Ho, Wo, H, W, C, a, b} (9 ints, HOST; NULL = plain [P][K] rows; a = b = 0 unless stated):
 *   mode 1: row p = (b, oy, ox) of the virtual matrix is the s x s block of the channels-last tensor [B,H,W,C] at
 *           (s*oy, s*ox), its K = s*s*C elements ordered (dy, dx, c)  -- conv k = s / stride s (neck levels, reference
 *           lss_fpn.py:143-149 / SECONDFPN) on the input side, transposed conv k = s / stride s (BaseBEVBackbone
 *           deblocks, base_bev_backbone.py:67-92; neck) on the output side;  (s*C) % 64 == 0 on an input side;
 *   mode 2: row p = pixel (s*oy + a, s*ox + b), K = C -- the stride-s 1x1 shortcut convs of the ResNet stages;
 *   mode 3 (input / x side only): im2col of a 3x3 / pad 1 / stride s convolution, K = 9*C ordered (tap, c), zeros
 *           outside the tensor -- the stride-2 3x3 convs of the ResNet stages and of BaseBEVBackbone's second level
 *           (forward and weight gradient; C % 64 == 0);
 *   mode 4 (input side only, s = 2): the data gradient of that convolution for the input pixels of parity class
 *           (a, b): row p = (batch, i, j) is pixel (2i + a, 2j + b) (written through a mode-2 output map with the same
 *           (a, b)), K = (1 + a)(1 + b) * C gathered from dy -- four launches cover the tensor with exactly the
 *           multiply-adds of the convolution (no zero-stuffed taps).  With a mode-4 input map `w` is the whole
 *           transposed tap-major weight [Cin][3][3][Cout] of the convolution (the kernel picks the class's taps).
 * Forward and data gradient are ud_conv1x1_mapped_nhwc_bf16 with the map on the input or the output (a data gradient
 * through a mode-2 output map writes only the sampled pixels: clear dx first); weight gradients are
 * ud_conv1x1_wgrad_mapped_nhwc_bf16 with the map on x or dy.  w / dw as in the unmapped calls: [Cout][K] / [Cout][Cin]. */
int ud_conv1x1_mapped_nhwc_bf16(const void* x, const void* w, void* y, int64_t P, int Cin, int Cout,
                                const int* in_map, const int* out_map, ud_stream_t stream);
/* fp32 twin (the reference's arithmetic): forward and data gradient of the strided / transposed convolutions of the fp32
 * mode on v_mfma_f32_16x16x4_f32; map channels % 4 == 0, Cin % 32 == 0, Cout % 4 == 0, a 32-channel slice inside one tap. */
int ud_conv1x1_mapped_nhwc_f32(const float* x, const float* w, float* y, int64_t P, int Cin, int Cout,
                               const int* in_map, const int* out_map, ud_stream_t stream);
/* Persistent form of the fp32 1x1 family (plain and mapped, csrc/conv2d_f32_1x1p.hip; the same layers as ud_conv1x1_nhwc_f32 /
 * ud_conv1x1_mapped_nhwc_f32): 512 resident workgroups walk (128-pixel tile, 64-channel block) units data parallel + a stream-K
 * tail of 32-channel slices (pieces of a cut unit are summed in slice order by a fix-up launch: deterministic), slices flowing
 * through a three-stage LDS ring two ahead of the MFMAs, epilogue (bias, folded BN, residual, ReLU if flags & 1) from registers.
 * partial != NULL: BatchNorm partial sums [*slices = ceil(P / 128)][Cout][2] (ud_conv1x1_bnstats_bytes).  in_map / out_map as in
 * ud_conv1x1_mapped_nhwc_f32 (NULL = plain; mapped launches take no epilogue inputs); x_elems = elements of the mapped input
 * tensor, y_elems of the mapped output tensor (ignored for plain sides).  workspace (ud_conv1x1p_f32_workspace_bytes) enables the stream-K tail.  Tensors < 4 GB.
 * ud_conv1x1_f32_persistent(mode): -1 default (UD_F32_1X1P or 1), 0 = callers use the grid-per-tile kernels, 1 = this one. */
size_t ud_conv1x1p_f32_workspace_bytes(void);
void ud_conv1x1_f32_persistent(int mode);
void ud_conv1x1p_stream_k(int mode);   /* tests / tuning: -1 default (the launcher's cost model), 0 whole units only, 2 cut every tail that can be cut */
int ud_conv1x1_f32_persistent_enabled(void);
int ud_conv1x1p_nhwc_f32(const float* x, const float* w, float* y, int64_t P, int Cin, int Cout, const float* bias,
                         const float* scale, const float* shift, const float* residual, int flags, float* partial,
                         size_t partial_bytes, int* slices, const int* in_map, const int* out_map, size_t x_elems,
                         size_t y_elems, void* workspace, size_t workspace_bytes, ud_stream_t stream);
int ud_conv1x1_wgrad_mapped_nhwc_bf16(const void* x, const void* dy, float* dw, int64_t P, int Cin, int Cout,
                                      const int* x_map, const int* dy_map, void* workspace,
                                      size_t workspace_bytes, ud_stream_t stream);
/* fp32 weight gradients (the reference's arithmetic; replaces nn.Conv2d's backward-weights pass of the BEV trunk,
 * base_bev_backbone.py:38-115, the CenterHead convolutions, center_head.py:58-99,311-355, and the image branch) on
 * v_mfma_f32_16x16x4_f32, exact fp32 products; pixel slices reduced in a fixed order (deterministic, no atomics).
 *   3x3 / stride 1 / pad 1: x [B][H][W][Cin], dy [B][H][W][Cout] -> dw [Cout][3][3][Cin];
 *   1x1 over pixel maps (NULL = plain rows; maps as above, on x or dy): dw [Cout][Cin'].
 * Cin % 4 == 0, Cout % 4 == 0 (and map channels % 4 == 0), else UD_ERR_UNSUPPORTED. */
size_t ud_conv3x3_wgrad_f32_workspace_bytes(int B, int H, int W, int Cin, int Cout);
int ud_conv3x3_wgrad_nhwc_f32(const float* x, const float* dy, float* dw, int B, int H, int W, int Cin, int Cout,
                              void* workspace, size_t workspace_bytes, ud_stream_t stream);
size_t ud_conv1x1_wgrad_f32_workspace_bytes(int64_t P, int Cin, int Cout);
int ud_conv1x1_wgrad_mapped_nhwc_f32(const float* x, const float* dy, float* dw, int64_t P, int Cin, int Cout,
                                     const int* x_map, const int* dy_map, void* workspace, size_t workspace_bytes,
                                     ud_stream_t stream);

/* fp32 3x3 / stride 1 / pad 1 as Winograd F(2x2, 3x3) on the fp32 MFMA pipe (2.25x fewer matrix flops than the direct form;
 * same layers as ud_conv3x3_nhwc_f32: base_bev_backbone.py:30-110, center_head.py:311-420, lss_fpn.py:143-149; the framework the
 * reference runs on picks the same algorithm family for fp32 3x3 layers).  Weights are transformed once per weight version:
 *   ud_conv3x3_wino_f32_weights(w, strides of (n, c, ky, kx) in elements, N, C, flip, U): U = G g G^T of g[n][ky][kx][c]; the forward
 *   pass uses (n, c) = (Cout, Cin), the data gradient (n, c) = (Cin, Cout) with flip = 1 (taps reversed);
 *   U holds ud_conv3x3_wino_f32_weight_bytes(C, N) bytes.
 * ud_conv3x3_wino_nhwc_f32: y = conv(x) (+ bias) (* scale + shift: folded eval-mode BatchNorm, both or NULL) (+ residual) (ReLU if flags & 1); partial != NULL also returns the per-workgroup
 * BatchNorm partial sums [*slices][Cout][2] (ud_conv3x3_wino_bnstats_bytes).  Cin % 8 == 0, Cout % 4 == 0. */
size_t ud_conv3x3_wino_f32_weight_bytes(int Cin, int Cout);
size_t ud_conv3x3_wino_bnstats_bytes(int B, int H, int W, int Cout);
int ud_conv3x3_wino_f32_blocks(int H, int W);   /* 64-tile blocks per image of the launch plan (fill = ceil(H/2) ceil(W/2) / (64 blocks)) */
int ud_conv3x3_wino_f32_weights(const float* w, int64_t s_n, int64_t s_c, int64_t s_y, int64_t s_x, int N, int C, int flip,
                                float* U, ud_stream_t stream);
int ud_conv3x3_wino_nhwc_f32(const float* x, const float* U, float* y, int B, int H, int W, int Cin, int Cout,
                             const float* bias, const float* scale, const float* shift, const float* residual, int flags,
                             float* partial, size_t partial_bytes, int* slices, ud_stream_t stream);

/* The same layers as Winograd F(4x4, 3x3) (csrc/conv2d_f32_wino4.hip): 36 multiplications per 4 x 4 outputs, 4x fewer matrix flops than
 * the direct form and 1.78x fewer than F(2x2, 3x3); rounding 3-5e-6 of the output's max against fp64 (tested per layer shape).  Same
 * contract as the ud_conv3x3_wino_* entry points; U from ud_conv3x3_wino4_f32_weights (ud_conv3x3_wino4_f32_weight_bytes(C, N) bytes);
 * ud_conv3x3_wino4_f32_blocks: 32-tile blocks per image of the launch plan (fill = ceil(H/4) ceil(W/4) / (32 blocks)).
 * Cin % 8 == 0, Cout % 4 == 0. */
size_t ud_conv3x3_wino4_f32_weight_bytes(int Cin, int Cout);
size_t ud_conv3x3_wino4_bnstats_bytes(int B, int H, int W, int Cout);
int ud_conv3x3_wino4_f32_blocks(int H, int W);
int ud_conv3x3_wino4_f32_weights(const float* w, int64_t s_n, int64_t s_c, int64_t s_y, int64_t s_x, int N, int C, int flip,
                                 float* U, ud_stream_t stream);
size_t ud_conv3x3_wino4_f32_workspace_bytes(int B, int H, int W, int Cin, int Cout);   /* stream-K partial tiles (optional: NULL = whole units only) */
void ud_conv3x3_wino4_stream_k(int mode);   /* schedule rule: -1 default (= 2), 0 whole units only, 1 stream-K tail when Cin >= 256, 2 every tail that beats one more round */
int ud_conv3x3_wino4_nhwc_f32(const float* x, const float* U, float* y, int B, int H, int W, int Cin, int Cout,
                              const float* bias, const float* scale, const float* shift, const float* residual, int flags,
                              float* partial, size_t partial_bytes, int* slices, void* workspace, size_t workspace_bytes,
                              ud_stream_t stream);
/* The same launch restricted to a device-side list of its pixel units (32-tile blocks, index (b * by + iy) * bx + ix of the plan's
 * bx x by blocks per image; ud_conv3x3_wino4_f32_block_shape = (tiles across << 8) | tiles down of a block): unit_list holds
 * *unit_count block indices in ascending order.  The grid is the dense launch's; the persistent workgroups read the count and
 * walk (listed block, output-channel block) units only -- whole units, stream-K tail and fix-up as in the dense schedule.  Blocks
 * that are not listed are neither read nor written: their part of y keeps what it held.  Inference only (no BatchNorm sums). */
int ud_conv3x3_wino4_f32_block_shape(int H, int W);
int ud_conv3x3_wino4_units_nhwc_f32(const float* x, const float* U, float* y, int B, int H, int W, int Cin, int Cout,
                                    const float* bias, const float* scale, const float* shift, const float* residual, int flags,
                                    const int* unit_list, const int* unit_count, void* workspace, size_t workspace_bytes,
                                    ud_stream_t stream);

/* Weight gradient of the same layers through the Winograd form (gradient of ud_conv3x3_wino_nhwc_f32: 16 instead of 36 multiplications
 * per 2 x 2 tile and (n, c)); same contract as ud_conv3x3_wgrad_nhwc_f32: dw [Cout][3][3][Cin], tile slices reduced in a fixed order. */
size_t ud_conv3x3_wino_wgrad_f32_workspace_bytes(int B, int H, int W, int Cin, int Cout);
int ud_conv3x3_wino_wgrad_nhwc_f32(const float* x, const float* dy, float* dw, int B, int H, int W, int Cin, int Cout,
                                   void* workspace, size_t workspace_bytes, ud_stream_t stream);

/* ... and through the F(4x4, 3x3) form (csrc/conv2d_f32_wino4_wgrad.hip: 36 multiplications per 16 output pixels and (n, c) instead of
 * 64): same contract; Cin % 32 == 0, Cout % 64 == 0, both tensors below 2 GB, else UD_ERR_UNSUPPORTED. */
size_t ud_conv3x3_wino4_wgrad_f32_workspace_bytes(int B, int H, int W, int Cin, int Cout);
int ud_conv3x3_wino4_wgrad_nhwc_f32(const float* x, const float* dy, float* dw, int B, int H, int W, int Cin, int Cout,
                                    void* workspace, size_t workspace_bytes, ud_stream_t stream);

/* ---- LiDAR input side ------------------------------------------------------------------
 * Replaces the numpy point transforms of the reference's data pipeline:
 * CollectLidarSweeps.forward (unidistill/data/multisensorfusion/transforms3d.py:379-414) and the point part
 * of BevAffineTransformation.forward (:417-443).  in/out f32 [rows][D] (D >= 3; in == out allowed); seg:
 * S+1 ascending row offsets (device, int64); mats: S row-major 4x4 float64 matrices (device); segment s
 * gets xyz <- (mats[s] @ [x y z 1]^T)[:3] evaluated in float64 in numpy's order and rounded to float32
 * (bit-identical to the reference), columns 3.. copied, and, when `last` (device, f32[S]) is given and
 * last[s] is not NaN, column D-1 <- last[s] (the sweep's time lag).  max_rows = longest segment. */
int ud_points_transform(const float* in, float* out, const int64_t* seg, const double* mats, const float* last,
                        int S, int D, int64_t max_rows, ud_stream_t stream);

/* ---- camera input side + collate ------------------------------------------------------
 * ImageNormalize.forward (data/multisensorfusion/transforms3d.py:350-368 -> mmcv.imnormalize, third party:
 * float32(img) [channel order reversed when to_rgb] - float32(mean), * float32(1 / float64(std))) fused with the
 * dataset's HWC -> CHW permute + stack (nuscenes_multimodal.py:262-293).  img u8 [NI][H][W][3] (device), out f32
 * [NI][3][H][W], or [NI][H][W][3] memory when out_channels_last (a channels-last view for the NHWC model);
 * mean/std: HOST float[3]. */
int ud_image_normalize(const unsigned char* img, float* out, const float* mean, const float* std, int to_rgb,
                       int NI, int H, int W, int out_channels_last, ud_stream_t stream);
/* collate_fn.fill_batch_tensor for ragged samples (nuscenes_multimodal.py:441-463): out f32 [B][L][W] (device),
 * out[b, :rows[b]] = samples[b] (device pointers, HOST array of B), zero rows up to L.  rows: HOST int64[B]. */
int ud_collate_pad(const float* const* samples, const int64_t* rows, int B, int64_t L, int W, float* out,
                   ud_stream_t stream);

/* ---- camera augmentation ---------------------------------------------------------------
 * ImageAffineTransformation.forward (data/multisensorfusion/transforms3d.py:298-347 -> functional.img_transform,
 * functional.py:560-592): PIL resize (BICUBIC) -> crop (zero fill) -> optional FLIP_LEFT_RIGHT -> rotate (NEAREST,
 * centre, black fill) of N uint8 RGB frames, bit-exact to Pillow, each frame with its own parameters.  The host
 * (ops/input_prep.py plan_frames) fills one record per frame, every field int64:
 *   src_off    byte offset in img of the frame's first stored source row, src_row0 = that row's index,
 *              src_rows = rows stored (a frame may ship only the row band its crop needs); row_stride bytes apart
 *   ws_off     byte offset of the frame's horizontal-pass rows in the workspace (16-aligned)
 *   htab/vtab  device addresses of the int32 resampling tables (W -> rw, H -> rh): rows of (lo, count,
 *              hk / vk weights in 22-bit fixed point), Pillow's precompute_coeffs + normalize_coeffs_8bpc
 *   rw, rh     resized size; cx, cy: crop origin in the resized image
 *   col0/ncols resized columns inside the crop; band0/band_rows: source rows the crop rows' vertical taps touch
 *   flip       FLIP_LEFT_RIGHT of the crop; rotate: 1 = output (x, y) reads crop pixel ((a2 + a1 y + a0 x) >> 16,
 *              (a5 + a4 y + a3 x) >> 16) or the fill when outside (Pillow's 16.16 NEAREST affine), 0 = copy
 * img u8 [.][H][W][3] (device, img_bytes long); out_mode 0: out u8 [N][fH][fW][3]; 1: f32 [N][3][fH][fW] and 2: f32
 * [N][fH][fW][3], both through ud_image_normalize's arithmetic (mean/std: HOST float[3], ignored for mode 0).
 * frames_host / frames_dev: the same N records on the host (validated, launch geometry) and on the device.
 * Workspace: ud_image_affine_workspace_bytes(frames_host, N) bytes (a pure function of the records). */
typedef struct UdImageAffineFrame {
  int64_t src_off, src_row0, src_rows, ws_off, htab, vtab, hk, vk, rw, rh, cx, cy;
  int64_t col0, ncols, band0, band_rows, flip, rotate, a0, a1, a2, a3, a4, a5;
} UdImageAffineFrame;
size_t ud_image_affine_workspace_bytes(const UdImageAffineFrame* frames_host, int N);
/* The launcher's bounds check of the records, as a pure host function: UD_OK, UD_ERR_INVALID_ARG (a band not stored or
 * outside img_bytes, crop columns outside the resized image, bad sizes) or UD_ERR_WORKSPACE (workspace_bytes too small). */
int ud_image_affine_check(const UdImageAffineFrame* frames_host, int N, int64_t img_bytes, int H, int W,
                          int64_t row_stride, int fH, int fW, size_t workspace_bytes);
int ud_image_affine(const unsigned char* img, int64_t img_bytes, int H, int W, int64_t row_stride,
                    const UdImageAffineFrame* frames_host, const UdImageAffineFrame* frames_dev, int N, int fH, int fW,
                    int out_mode, void* out, const float* mean, const float* std, int to_rgb, void* workspace,
                    size_t workspace_bytes, ud_stream_t stream);

/* ---- LiDAR input chain after collate -------------------------------------------------------
 * CollectLidarSweeps -> BevAffineTransformation -> ObjectRangeFilter (data/multisensorfusion/transforms3d.py:379-443,
 * :242-287) on the points, then collate_fn's zero-padded stack (nuscenes_multimodal.py:441-463), for a whole batch.
 * pts f32 [rows][D] (device): S segments, segment s = rows seg[s] .. seg[s+1]; sample b = segments
 * sample_seg[b] .. sample_seg[b+1] (key frame first, then its sweeps; at most UD_LIDAR_MAX_SEGMENTS).  seg / sample_seg
 * are given on the host (validation, launch geometry) and on the device.  Per row:
 *   xyz = the segment's matrix applied in float64, rounded to float32 (seg_par[s][17] != 0), else copied;
 *   then the sample's BDA matrix applied the same way to that float32 result (smp_par[b][22] != 0);
 *   column D-1 <- seg_par[s][16] when D > 3 and that value is not NaN (time lag; 0 for the key frame when D == 5);
 *   kept when x >= r0 && x <= r3 && y >= r1 && y <= r4 in float32 (smp_par[b][23] != 0; NaN fails), else always.
 * Kept rows keep their order.  seg_par f64 [S][UD_LIDAR_SEG_PAR] = matrix (16, row major), last, transform flag;
 * smp_par f64 [B][UD_LIDAR_SMP_PAR] = BDA matrix (16), range (6 float32 values), has_bda, has_range (device).
 *   ud_lidar_prep_count   : counts (device int64[B]) <- kept rows per sample
 *   ud_lidar_prep_compact : with counts_host = those counts read back; compact == 0: out f32 [B][nmax][D], rows
 *                           counts[b] .. nmax zero (nmax >= every count, out_rows >= B * nmax); compact == 1: the
 *                           samples' kept rows back to back (out_rows >= their sum).  Same plan as the count call.
 * Both validate the plan on the host first (UD_ERR_INVALID_ARG: offsets not ascending, D < 3, a NULL pointer with a
 * non-zero size, too many segments in a sample, B > 65535) and launch nothing when it fails.
 * Workspace: ud_lidar_prep_workspace_bytes(seg_host, sample_seg_host, S, B), the same buffer for both calls. */
#define UD_LIDAR_MAX_SEGMENTS 64
#define UD_LIDAR_SEG_PAR 18
#define UD_LIDAR_SMP_PAR 24
size_t ud_lidar_prep_workspace_bytes(const int64_t* seg_host, const int64_t* sample_seg_host, int S, int B);
int ud_lidar_prep_count(const float* pts, int64_t rows, int D, const int64_t* seg_host, const int64_t* sample_seg_host,
                        int S, int B, const int64_t* seg_dev, const int64_t* sample_seg_dev, const double* seg_par,
                        const double* smp_par, int64_t* counts, void* workspace, size_t workspace_bytes,
                        ud_stream_t stream);
int ud_lidar_prep_compact(const float* pts, int64_t rows, int D, const int64_t* seg_host,
                          const int64_t* sample_seg_host, int S, int B, const int64_t* seg_dev,
                          const int64_t* sample_seg_dev, const double* seg_par, const double* smp_par,
                          const int64_t* counts_host, const int64_t* counts, int64_t nmax, int compact, float* out,
                          int64_t out_rows, void* workspace, size_t workspace_bytes, ud_stream_t stream);

/* ---- JPEG decode after collate -------------------------------------------------------------
 * The reference reads every camera frame with skimage_io.imread (nuscenes_multimodal.py:171-177, :197), i.e. Pillow's
 * libjpeg-turbo.  Baseline / extended-sequential Huffman JPEGs (SOF0 / SOF1), 8-bit, three components YCbCr in one
 * interleaved scan, luma sampling 1x1, 2x1 or 2x2 and chroma 1x1, with or without restart intervals, decode here bit for
 * bit as Pillow decodes them: ISLOW IDCT, fancy upsampling, jdcolor's fixed-point YCbCr -> RGB.
 *   ud_jpeg_parse  : HOST only.  Reads the markers of one file into a record (geometry, quantisation tables in natural
 *                    order, per component the DC / AC Huffman lookups, the entropy-coded segment's byte range).
 *                    UD_JPEG_OK, or UD_JPEG_UNSUPPORTED (progressive, lossless, arithmetic, 12-bit, grayscale, CMYK,
 *                    RGB, 4:4:0 or other sampling, multi-scan), UD_JPEG_TRUNCATED (the file ends early, no EOI) or
 *                    UD_JPEG_CORRUPT (inconsistent headers, oversubscribed Huffman tables); nothing is launched for
 *                    such a file.  The scan's bytes are taken to the end of the data: the decode ends the scan at its
 *                    first marker other than RSTn (normally EOI; bytes after it are ignored).
 *   ud_jpeg_plan   : HOST only.  With src_off set by the caller (the file's offset in the packed input), fills each
 *                    record's out_off (frames back to back, uint8 [H][W][3] each) and workspace offsets; returns the
 *                    workspace bytes ud_jpeg_decode needs (0 when a record is not a parsed one).
 *   ud_jpeg_decode : N frames, any mix of sizes and sampling modes, in four launches: destuff + split at RSTn,
 *                    self-synchronising parallel Huffman decode (UD_JPEG_SUB_BITS-bit subsequences), dequantise + IDCT
 *                    into component planes, upsample + colour convert into out.  status int32[N] (device) <- 0 or
 *                    UD_JPEG_ST_* bits; a failed frame's pixels are zeros and the other frames are unaffected.  iters
 *                    int32[N] (device, may be NULL) <- the synchronisation rounds the Huffman decode needed.
 * Every bitstream read is clamped to the frame's own entropy-coded bytes; the host checks the records (geometry
 * consistent with the sizes, regions inside src / out / workspace) before anything is launched. */
#define UD_JPEG_OK 0
#define UD_JPEG_UNSUPPORTED 1
#define UD_JPEG_TRUNCATED 2
#define UD_JPEG_CORRUPT 3
#define UD_JPEG_LOOKAHEAD 9
#define UD_JPEG_SUB_BITS 1024
#define UD_JPEG_ST_MARKER 1 /* restart numbers out of order or miscounted (the scan ends at its first other marker) */
#define UD_JPEG_ST_CODE 2   /* an invalid Huffman code or a coefficient index past 63 */
#define UD_JPEG_ST_LENGTH 4 /* a segment holds fewer or more bytes than its MCUs need */
typedef struct UdJpegHuff {
  uint16_t look[1 << UD_JPEG_LOOKAHEAD]; /* code length << 8 | symbol for codes of <= LOOKAHEAD bits, else 0 */
  int32_t maxcode[18];                   /* largest code of each length, -1 when none */
  int32_t valoff[18];                    /* index of a length's first symbol minus its first code */
  uint8_t vals[256];
} UdJpegHuff;
typedef struct UdJpegFrame {
  int32_t width, height, hmax, vmax, mcus_x, mcus_y, bpm, restart, nseg, reserved0;
  int32_t comp_id[3], h[3], v[3], cw[3], ch[3], reserved1;
  int64_t ecs_off, ecs_bytes;                           /* entropy-coded segment, relative to the file's first byte */
  int64_t src_off, out_off, ws_ecs, ws_seg, ws_sub, ws_state, ws_scan, ws_coef, ws_plane[3], nsub_max, total_blocks;
  uint16_t qt[3][64];                                   /* per component, natural order */
  UdJpegHuff huff[6];                                   /* component c: [2c] DC, [2c + 1] AC */
} UdJpegFrame;
int ud_jpeg_parse(const unsigned char* bytes, int64_t nbytes, UdJpegFrame* out);
size_t ud_jpeg_plan(UdJpegFrame* frames, int N);
int ud_jpeg_decode(const unsigned char* src, int64_t src_bytes, const UdJpegFrame* frames_host,
                   const UdJpegFrame* frames_dev, int N, unsigned char* out, int64_t out_bytes, int32_t* status,
                   int32_t* iters, void* workspace, size_t workspace_bytes, ud_stream_t stream);

/* ---- frozen ResNet stem (image branch) ----------------------------------------------------------------
 * conv1 (7x7 / stride 2 / pad 3, 3 -> 64, no bias) + bn1 (eval mode, folded to scale / shift) + ReLU, then max-pool 3x3 /
 * stride 2 / pad 1, of the mmdet ResNet-50 the reference builds in unidistill/layers/blocks_3d/mmdet3d/lss_fpn.py:143-149 with
 * frozen_stages = 0 (exps/.../BEVFusion_nuscenes_centerhead_fusion_exp.py:24-31).  Forward only (the stem takes no gradient).
 *   ud_stem_pack_weights     : HOST helper: w = host pointer to the [64][3][7][7] filters (strides in floats) ->
 *                              packed f32[7*6*4*16*4] in the kernel's MFMA operand order (once per frozen filter)
 *   ud_stem_conv7x7_bn_relu  : x f32 [B][3][H][W] through its strides in floats (NCHW planes or channels-last memory),
 *                              packed_w / scale[64] / shift[64] device f32 -> y [B][OH][OW][64] channels-last, f32 or bf16
 *                              (OH = (H - 1) / 2 + 1, same for OW); fp32 MFMA, exact products
 *   ud_maxpool3x3s2_nhwc     : x [B][H][W][C] -> y [B][(H - 1) / 2 + 1][(W - 1) / 2 + 1][C], f32 (C % 4 == 0) or bf16 (C % 8 == 0) */
int ud_stem_pack_weights(const float* w, int64_t sn, int64_t sc, int64_t sky, int64_t skx, float* packed);
int ud_stem_conv7x7_bn_relu(const float* x, int64_t sb, int64_t sc, int64_t sy, int64_t sx, int B, int H, int W,
                            const float* packed_w, const float* scale, const float* shift, void* y, int out_bf16,
                            ud_stream_t stream);
int ud_maxpool3x3s2_nhwc(const void* x, void* y, int B, int H, int W, int C, int is_bf16, ud_stream_t stream);

/* ---- BatchNorm2d (+ residual) (+ ReLU), channels-last bf16 ------------------------------------------
 * The Conv2d -> BatchNorm2d -> ReLU links of the reference's dense layers (base_bev_backbone.py:48-66,
 * center_head.py:408-420, the mmdet ResNet bottlenecks) as HBM-bound streaming kernels over
 * x [P rows][C] bf16 -- P = B*H*W pixels of a channels-last map, or the active voxels of a sparse tensor
 * (the BatchNorm1d of the reference's sparse blocks, spconv_backbone.py:10-113).
 *   ud_bn_stats   : training-mode batch statistics -> mean, biased var, invstd, folded scale/shift;
 *                   running_mean / running_var (optional, both or neither) are updated in place like
 *                   nn.BatchNorm does (unbiased variance); batches_tracked (optional device int64) += 1.
 *                   C % 16 == 0.
 *   ud_bn_act_fwd : y = act(x * scale + shift (+ residual)), scale = gamma*invstd, shift = beta - mean*scale
 *                   (batch statistics in training, running statistics in eval).  C % 8 == 0.
 *   ud_bn_act_bwd : training-mode backward: dx (bf16), dgamma, dbeta [C] and, when `dresidual` is given,
 *                   the masked gradient for the residual branch.  Pass `y` (the saved output) when a
 *                   residual took part in the forward, NULL otherwise (the ReLU mask is then recomputed
 *                   from x).  C % 16 == 0.  Deterministic two-stage reductions. */
size_t ud_bn_act_workspace_bytes(int C);
int ud_bn_stats(const void* x, long long P, int C, const float* gamma, const float* beta, float eps,
                float* mean, float* var, float* invstd, float* scale, float* shift, float* running_mean,
                float* running_var, float momentum, long long* batches_tracked, void* workspace,
                size_t workspace_bytes, ud_stream_t stream);
int ud_bn_act_fwd(const void* x, const void* residual, const float* scale, const float* shift, void* y,
                  long long P, int C, int relu, ud_stream_t stream);
int ud_bn_act_bwd(const void* x, const void* y, const void* dy, const float* scale, const float* shift,
                  const float* mean, const float* invstd, void* dx, void* dresidual, float* dgamma,
                  float* dbeta, long long P, int C, int relu, void* workspace, size_t workspace_bytes,
                  ud_stream_t stream);
/* ud_bn_stats for a tensor whose first statistics pass came out of a convolution epilogue
 * (ud_conv*_bnstats_nhwc_*): partial [slices][C][2] per-tile (sum, sum of squares) over the P rows, reduced in slice
 * order (deterministic); outputs and running-statistics update exactly as ud_bn_stats. */
int ud_bn_stats_from_partials(const float* partial, int slices, long long P, int C, const float* gamma,
                              const float* beta, float eps, float* mean, float* var, float* invstd, float* scale,
                              float* shift, float* running_mean, float* running_var, float momentum,
                              long long* batches_tracked, ud_stream_t stream);
/* fp32 twins for the fp32 (reference-arithmetic) mode: x / residual / y / dy / dx are FP32 rows, everything
 * else as above (C % 16 == 0). */
int ud_bn_stats_f32(const float* x, long long P, int C, const float* gamma, const float* beta, float eps,
                    float* mean, float* var, float* invstd, float* scale, float* shift, float* running_mean,
                    float* running_var, float momentum, long long* batches_tracked, void* workspace,
                    size_t workspace_bytes, ud_stream_t stream);
int ud_bn_act_fwd_f32(const float* x, const float* residual, const float* scale, const float* shift, float* y,
                      long long P, int C, int relu, ud_stream_t stream);
int ud_bn_act_bwd_f32(const float* x, const float* y, const float* dy, const float* scale, const float* shift,
                      const float* mean, const float* invstd, float* dx, float* dresidual, float* dgamma,
                      float* dbeta, long long P, int C, int relu, void* workspace, size_t workspace_bytes,
                      ud_stream_t stream);
/* y (forward) / dy (backward) as a CHANNEL SLICE of a wider channels-last map: rows of C elements every `ld` elements
 * (ld >= C, ld % 8 == 0, the slice's first element 16-byte aligned); everything else as the functions above.  The upsampling
 * heads of the BEV trunk (reference base_bev_backbone.py:117-141: `torch.cat(ups, dim=1)` over the deblocks' BatchNorm + ReLU
 * outputs) write straight into the concatenated map and read its gradient in place: no cat kernel forward, no strided-slice
 * copies backward. */
int ud_bn_act_fwd_ld(const void* x, const void* residual, const float* scale, const float* shift, void* y,
                     long long P, int C, long long y_ld, int relu, ud_stream_t stream);
int ud_bn_act_fwd_ld_f32(const float* x, const float* residual, const float* scale, const float* shift, float* y,
                         long long P, int C, long long y_ld, int relu, ud_stream_t stream);
int ud_bn_act_bwd_ld(const void* x, const void* y, const void* dy, long long dy_ld, const float* scale, const float* shift,
                     const float* mean, const float* invstd, void* dx, void* dresidual, float* dgamma,
                     float* dbeta, long long P, int C, int relu, void* workspace, size_t workspace_bytes,
                     ud_stream_t stream);
int ud_bn_act_bwd_ld_f32(const float* x, const float* y, const float* dy, long long dy_ld, const float* scale,
                         const float* shift, const float* mean, const float* invstd, float* dx, float* dresidual,
                         float* dgamma, float* dbeta, long long P, int C, int relu, void* workspace,
                         size_t workspace_bytes, ud_stream_t stream);
/* Backward through FROZEN statistics: an eval-mode BatchNorm inside a training graph (the reference's frozen_bn /
 * frozen_encoder, models/multisensor_fusion/base.py:50-67; mmdet's norm_eval).  scale / shift / mean / invstd are the vectors
 * folded from the running buffers; the shape rules are those of ud_bn_act_bwd_ld* (C % 16 == 0, dy a channel slice with row
 * stride dy_ld, y the saved output when a residual took part).
 *   dx = scale * dr, dresidual (optional) = dr, dr = dy under the ReLU mask of the training-mode kernels.
 *   dgamma, dbeta: both given -> dbeta = sum dr, dgamma = invstd * sum dr (x - mean): the pass that writes dx leaves per-slice
 *     partial sums, a fixed-order kernel adds them (two launches, no atomics, bitwise reproducible; workspace of
 *     ud_bn_act_workspace_bytes(C)).  Both NULL (frozen affine parameters) -> ONE launch, no reduction; mean, invstd and the
 *     workspace are not read and may be NULL / 0. */
int ud_bn_act_bwd_frozen_ld(const void* x, const void* y, const void* dy, long long dy_ld, const float* scale,
                            const float* shift, const float* mean, const float* invstd, void* dx, void* dresidual,
                            float* dgamma, float* dbeta, long long P, int C, int relu, void* workspace,
                            size_t workspace_bytes, ud_stream_t stream);
int ud_bn_act_bwd_frozen_ld_f32(const float* x, const float* y, const float* dy, long long dy_ld, const float* scale,
                                const float* shift, const float* mean, const float* invstd, float* dx, float* dresidual,
                                float* dgamma, float* dbeta, long long P, int C, int relu, void* workspace,
                                size_t workspace_bytes, ud_stream_t stream);

/* ---- Proposal layer: rotated-BEV IoU + greedy NMS -----------------------------------------------------
 * Replaces `iou3d_nms_cuda.nms_gpu(boxes, keep, thresh)` (reference layers/head/det3d/generate_proposals/
 * centerpoint_gen_proposals.py:85-105; OpenPCDet iou3d_nms, binary absent from the tree).
 * boxes f32[N,7] = (x, y, z, dx, dy, dz, heading) sorted by descending score.  keep i64[N] receives the
 * kept indices in order (rest = -1), *num_keep (device int) their count; nothing synchronises with the
 * host.  N <= 16384.  ud_boxes_iou_bev: iou f32[Na,Nb] of the BEV footprints. */
size_t ud_nms_bev_workspace_bytes(int N);
int ud_nms_rotated_bev(const float* boxes, int N, float thresh, long long* keep, int* num_keep,
                       void* workspace, size_t workspace_bytes, ud_stream_t stream);
int ud_boxes_iou_bev(const float* a, int Na, const float* b, int Nb, float* iou, ud_stream_t stream);

/* ---- Proposal layer on the device: top-K decode + IoU-aware score + filters + rotated NMS + roi packing ----
 * Replaces IouAwareGenProposals / CenterPointGenProposals.generate_predicted_boxes (reference layers/head/
 * det3d/generate_proposals/iou_aware_gen_proposals.py:43-139, centerpoint_gen_proposals.py:66-105,232-340)
 * for all T <= 8 tasks and B samples in three launches; nothing synchronises with the host.
 *   heads   HOST array [T*7] of device pointers: hm, reg, height, dim, rot, vel, iou of task t (raw head
 *           outputs, fp32, logical shape [B, c, H, W]); vel may be NULL when box_dim == 7, iou when iou_alpha
 *           is NULL (plain CenterPoint: NMS ranks by the heat-map score).
 *   strides HOST array [T*7*3]: (batch, channel, pixel) strides in elements of each tensor (NCHW planes:
 *           (c*H*W, H*W, 1); channel slices of a channels-last packed map: (H*W*Ctot, 1, Ctot)).
 *   num_classes / class_offsets / iou_alpha  HOST arrays [T]: classes of the task's heat map, number of
 *           classes of the tasks before it (labels are 1-based global ids), IoU-aware exponent a
 *           (NMS score = score^(1-a) * clamp(iou/2+0.5, 0, 1)^a).
 *   K = nms_pre_max_size (<= 2048), post_max = nms_post_max_size (<= 512); box = (x, y, z, dx, dy, dz, rot
 *   [, vx, vy]); dx..dz = clamp(exp(dim), 0.001, 30) unless no_log; x = (col + reg.x) * out_size_factor *
 *   voxel_x + pc_x (same fp32 operation order as the reference); kept iff center_range[0:3] <= (x,y,z) <=
 *   center_range[3:6] (HOST array [6]) and score > score_threshold.
 * Outputs: rois f32[B, T*post_max, box_dim], roi_scores f32[B, T*post_max], roi_labels i64[B, T*post_max]
 * (tasks back to back, each in NMS order, zero padded), num_boxes i32[B] = rows in use per sample. */
size_t ud_proposal_workspace_bytes(int B, int T, int K);
int ud_proposal_layer(const float* const* heads, const long long* strides, const int* num_classes,
                      const int* class_offsets, const float* iou_alpha, int B, int T, int H, int W, int K,
                      int post_max, int box_dim, int no_log, float out_size_factor, float voxel_x,
                      float voxel_y, float pc_x, float pc_y, const float* center_range, float score_threshold,
                      float nms_threshold, float* rois, float* roi_scores, long long* roi_labels,
                      int* num_boxes, void* workspace, size_t workspace_bytes, ud_stream_t stream);

/* ---- Detection loss of the CenterPoint heads (focal + gathered regression / IoU terms) ------------------
 * CenterHeadIouAware.get_loss (reference layers/head/det3d/center_head_iou_aware.py:55-298, losses/det3d.py:
 * 287-421) for all T <= 8 tasks at once.  Head tensors are given as device-pointer tables (any
 * [B, c, H, W] fp32 tensors with contiguous H*W planes; *_bstride = elements between batch entries).
 *   ud_det_focal_fwd : prob [T,B,ncm,HW] = clamp(sigmoid(hm), 1e-4, 1-1e-4) (0 in padded channels),
 *                      pos_neg [T,2] = (sum log(p)(1-p)^g a [gt==1], sum log(1-p+1e-4) p^g (1-a) [gt==0]).
 *   ud_det_focal_bwd : dlogit [T,B,ncm,HW] from g_prob (optional), g_pos [T], g_neg [T].
 *   ud_det_reg_fwd   : head[t*11+j] = plane of gathered value j (reg.x reg.y height dim0..2 rot.sin rot.cos
 *                      vel.x vel.y iou); ind i64 / mask u8 / tgt f32 [T,B,K(,tgt_dim)], num_obj f32 [T];
 *                      losses [T,12] = box L1 per code dim (10), IoU loss, IoU-aware L1, all normalised;
 *                      loc [T,B,K,17] = local derivatives kept for the backward.  nb = 10 (nuScenes codes).
 *   ud_det_reg_bwd   : dhead [T,B,11,HW] (caller zero-fills) += scaled local derivatives at the slots.
 *   ud_det_reg_fwd_rot / ud_det_reg_bwd_rot : the same pair (same arguments, same box L1) with the rotated 3-D IoU
 *                       of the decoded prediction and target in both IoU terms: IoU loss
 *                      sum (1 - clamp(IoU,0,1)) / max(num_obj,1) with derivatives for reg, height, dim AND rot, IoU-aware
 *                      target 2 (IoU - 0.5).  loc [T,B,K,19] (10 box, 8 IoU-loss, 1 aware).
 *   ud_rot_iou3d_pairs : iou [N] = IoU3D_rot(a[i], b[i]) of boxes [N,7] = x y z dx dy dz yaw (rotated-rectangle
 *                      intersection x z-overlap over the union, floor 1e-8); diou_da [N,7] = d iou[i] / d a[i], or NULL.
 * Ordered two-stage reductions; no host synchronisation. */
size_t ud_det_loss_workspace_bytes(int T);
int ud_det_focal_fwd(const float* const* hm, const long long* hm_bstride, const int* ncls, int T, int B,
                     int ncm, int HW, const float* gt, float alpha, float gamma, float* prob,
                     float* pos_neg, void* workspace, size_t workspace_bytes, ud_stream_t stream);
int ud_det_focal_bwd(const int* ncls, int T, int B, int ncm, int HW, const float* gt, const float* prob,
                     const float* g_prob, const float* g_pos, const float* g_neg, float alpha,
                     float gamma, float* dlogit, ud_stream_t stream);
int ud_det_reg_fwd(const float* const* head, const long long* head_bstride, int T, int B, int K, int HW,
                   int nb, const long long* ind, const unsigned char* mask, const float* tgt, int tgt_dim,
                   const float* num_obj, float sx, float sy, float* losses, float* loc, void* workspace,
                   size_t workspace_bytes, ud_stream_t stream);
int ud_det_reg_bwd(int T, int B, int K, int HW, int nb, const long long* ind, const unsigned char* mask,
                   const float* loc, const float* g_box, const float* g_iou, const float* g_aw,
                   float* dhead, ud_stream_t stream);
int ud_det_reg_fwd_rot(const float* const* head, const long long* head_bstride, int T, int B, int K, int HW,
                       int nb, const long long* ind, const unsigned char* mask, const float* tgt, int tgt_dim,
                       const float* num_obj, float sx, float sy, float* losses, float* loc, void* workspace,
                       size_t workspace_bytes, ud_stream_t stream);
int ud_det_reg_bwd_rot(int T, int B, int K, int HW, int nb, const long long* ind, const unsigned char* mask,
                       const float* loc, const float* g_box, const float* g_iou, const float* g_aw,
                       float* dhead, ud_stream_t stream);
int ud_rot_iou3d_pairs(const float* a, const float* b, int N, float* iou, float* diou_da, ud_stream_t stream);

/* ---- FCOS-style target assignment of the CenterPoint heads -----------------------------------
 * FCOSAssigner.assign_targets (reference layers/head/det3d/target_assigner/fcos_assigner.py:73-285) for all
 * T tasks and B samples in one launch.  gt f32[B,M,cols] (x y z dx dy dz yaw [extra...] class(1-based));
 * task_of / off_of: HOST int8 tables indexed by class id (task of the class or -1, offset inside the task).
 * Outputs: hm f32[T,B,ncm,h*w] one-hot class map of the positive anchors, ind i64 / mask u8 / cat i64
 * [T,B,K] (positives in ascending anchor order), enc f32[T,B,K,enc_dim] box encoding relative to the
 * anchor (log sizes, sin/cos yaw; +-inf for zero-size boxes like the reference).  topk <= 9, M <= 512,
 * grid <= 180 x 180, else UD_ERR_UNSUPPORTED. */
int ud_assign_targets(const float* gt, int B, int M, int cols, const signed char* task_of,
                      const signed char* off_of, int n_classes, int T, int ncm, int w, int h, int K,
                      int topk, int enc_dim, float osf, float pc0, float pc1, float vs0, float vs1,
                      float* hm, long long* ind, unsigned char* mask, long long* cat, float* enc,
                      ud_stream_t stream);

/* ---- nuScenes detection metric, detection_cvpr_2019 ------------------------------------------
 * The reference's validation_epoch_end -> NuscenesMultiModalData.evaluation (nuscenes_multimodal.py:336-393,
 * eval_utils.py) ends in the nuScenes devkit's DetectionEval; tests/nus_eval_reference.py restates it in numpy.
 *   ud_nus_pred_to_global : per prediction row (boxes f32 [n][ncol], ncol 7 or 9 = x y z dx dy dz rot [vx vy], scores
 *                   f32 [n], labels int64 [n] starting at 1) of a batch whose sample b owns rows batch_off[b] ..
 *                   batch_off[b+1] (int32, device): the global-frame record rec f64 [n][UD_NUS_PRED_COLS] =
 *                   x y z w l h yaw vx vy score through the sample's LiDAR->global matrix l2g f64 [B][4][4] (row
 *                   major), cls int32 = label - 1 and attr int32 (eval_utils' rule from the per-class tables
 *                   attr_moving / attr_still, -1 = '').  A label outside 1 .. num_classes sets UD_NUS_ST_CLASS in
 *                   *status (device, OR-ed) and gives cls -1.
 *   ud_nus_eval   : the metric's curves.  One workgroup per sample: the class-range / num_pts / keep filters, the
 *                   sample's kept predictions in (class, descending score, descending box) order, greedy matching at
 *                   the four thresholds (TP flags, matched GT, the five TP errors at dist_th_tp); a stable radix sort
 *                   of (class, descending score) over the predictions laid out in (sample, box) order and reversed;
 *                   per (class, threshold) the integer TP cumsum, per (class, error) the NaN-aware cummean over the
 *                   matches; numpy.interp of precision, confidence and the errors onto the recall points.
 * Host-checked (UD_ERR_INVALID_ARG, nothing launched): sizes, NULL pointers, num_classes, dist_th_tp_index.  Device
 * checks set status bits: UD_NUS_ST_CLASS, UD_NUS_ST_SIZE (a matched pair with a size <= 0), UD_NUS_ST_COUNT (more
 * than UD_NUS_MAX_BOXES boxes of one sample).  Workspace: ud_nus_eval_workspace_bytes(P, num_classes). */
#define UD_NUS_MAX_CLASSES 15
#define UD_NUS_PRED_COLS 10
#define UD_NUS_GT_COLS 9
#define UD_NUS_MAX_BOXES 1024 /* predictions, and ground-truth boxes, of one sample */
#define UD_NUS_POINTS 101
#define UD_NUS_ST_CLASS 1
#define UD_NUS_ST_SIZE 2
#define UD_NUS_ST_COUNT 4

typedef struct {
  int num_classes;
  int dist_th_tp_index;                       /* which of dist_th is dist_th_tp */
  int pi_period_class;                        /* class whose yaw period is pi (barrier), -1 = none */
  int pad_;
  double class_range[UD_NUS_MAX_CLASSES];
  double dist_th[4];
  double rec_pts[UD_NUS_POINTS];              /* numpy.linspace(0, 1, 101) */
} UdNusCfg;

typedef struct {
  /* predictions: rows of ud_nus_pred_to_global, each sample's rows contiguous, samples in any order */
  const double* pred_rec;                     /* [rows][UD_NUS_PRED_COLS] */
  const int32_t* pred_cls;                    /* [rows], -1 = invalid */
  const int32_t* pred_attr;                   /* [rows] */
  const int64_t* pred_src;                    /* [S] first row of sample s */
  const int64_t* pred_off;                    /* [S + 1] sample s = (sample, box) positions pred_off[s] .. pred_off[s+1] */
  /* ground truth, samples in order: sample s = rows gt_off[s] .. gt_off[s+1] */
  const double* gt_rec;                       /* [G][UD_NUS_GT_COLS] x y z w l h yaw vx vy */
  const int32_t* gt_cls;
  const int32_t* gt_attr;                     /* -1 = '' */
  const int32_t* gt_num_pts;
  const uint8_t* gt_keep;                     /* caller's mask (bike racks) */
  const int64_t* gt_off;
  const double* ego;                          /* [S][3] ego translation, global frame */
  /* outputs */
  double* prec;                               /* [C][4][101] */
  double* conf;                               /* [C][4][101] */
  double* tp_err;                             /* [C][5][101] trans scale orient vel attr */
  uint8_t* tp;                                /* [4][P] per (sample, box) position; 0 for a filtered prediction */
  int32_t* match_gt;                          /* [P] GT row matched at dist_th_tp, -1 */
  int32_t* order;                             /* [P] (sample, box) position of each sorted prediction, by class */
  int32_t* counts;                            /* [2][C] kept predictions, kept GT (npos) */
  int32_t* status;                            /* OR-ed UD_NUS_ST_* bits */
} UdNusEvalIo;

int ud_nus_pred_to_global(const float* boxes, int64_t n, int ncol, const float* scores, const int64_t* labels,
                          const int32_t* batch_off, int B, const double* l2g, int num_classes,
                          const int32_t* attr_moving_host, const int32_t* attr_still_host, double* rec, int32_t* cls,
                          int32_t* attr, int32_t* status, ud_stream_t stream);
size_t ud_nus_eval_workspace_bytes(int64_t P, int num_classes);
int ud_nus_eval(const UdNusCfg* cfg_host, const UdNusEvalIo* io_host, int S, int64_t P, void* workspace,
                size_t workspace_bytes, ud_stream_t stream);

/* ---- optimizer: gradient-norm clip + decoupled-weight-decay AdamW in two launches (csrc/optim.hip) ----
 * The parameter set is cut into chunks of ud_optim_chunk_elems() elements; a chunk lies inside one tensor (the last
 * chunk of a tensor is short).  One workgroup per chunk; nothing in the grid depends on the data.
 *   ud_optim_sqnorm      partial[c] = sum of g*g over chunk c (0 for a tensor whose gradient pointer is NULL), in a fixed
 *                        order that depends on the position inside the chunk only; workgroup 0 also latches
 *                        state[STEP] into state[STEP_IN].
 *   ud_optim_clip_adamw  every workgroup sums the partials in the same order, so all of them hold the same total:
 *                        total_norm = sqrt(sum), coef = min(1, max_norm / (total_norm + 1e-6)), then AdamW on its own
 *                        chunk with g' = coef * g applied on the fly (gradients are never written).  With skip_nonfinite
 *                        and a non-finite total_norm nothing is written to params / exp_avg / exp_avg_sq, STEP stays and
 *                        SKIPPED is incremented.  Workgroup 0 writes STEP, NORM, COEF, SKIPPED, FINITE.
 *   ud_optim_clip_adamw_ema  the same step (bit for bit) with a fifth row of tensors, ema: after an element's new p is
 *                        formed, ema = lerp(ema, p, w) in torch's form (ema + w * (p - ema) for w < 0.5, p - (p - ema) *
 *                        (1 - w) otherwise), w = (float)(1 - d), d = ema_decay for ema_ramp <= 0 and ema_decay *
 *                        (1 - exp(-n / ema_ramp)) otherwise, n = the number of applied steps including this one (STEP
 *                        after the call).  A skipped step leaves ema untouched and does not advance n.  A tensor whose
 *                        gradient pointer is NULL is not stepped, but its ema is still lerped towards its value.
 *   ud_optim_swap        exchanges a_ptrs[t][i] and b_ptrs[t][i] for every element of the table, bit for bit.
 * params / exp_avg / exp_avg_sq / ema / grads are DEVICE arrays of per-tensor device pointers (fp32 data, each tensor's
 * elements in the same storage order in all of them).  state is UD_OPTIM_STATE_DOUBLES doubles on the device. */
typedef struct {
  int64_t offset;                             /* first element of the chunk inside its tensor */
  int32_t tensor;                             /* index into the pointer arrays */
  int32_t length;                             /* 1 .. ud_optim_chunk_elems() */
} UdOptimChunk;
#define UD_OPTIM_ST_LR 0                      /* written by the host */
#define UD_OPTIM_ST_STEP 1                    /* completed (not skipped) steps */
#define UD_OPTIM_ST_STEP_IN 2                 /* STEP as latched by ud_optim_sqnorm */
#define UD_OPTIM_ST_NORM 3                    /* total_norm of the last call */
#define UD_OPTIM_ST_COEF 4                    /* clip coefficient of the last call */
#define UD_OPTIM_ST_SKIPPED 5                 /* calls skipped by the guard */
#define UD_OPTIM_ST_FINITE 6                  /* 1 if the last total_norm was finite */
#define UD_OPTIM_STATE_DOUBLES 8
int ud_optim_chunk_elems(void);
int ud_optim_sqnorm(const UdOptimChunk* chunks, int n_chunks, const float* const* grads, double* partial,
                    double* state, ud_stream_t stream);
int ud_optim_clip_adamw(const UdOptimChunk* chunks, int n_chunks, float* const* params, float* const* exp_avg,
                        float* const* exp_avg_sq, const float* const* grads, const double* partial, double* state,
                        double beta1, double beta2, double eps, double weight_decay, double max_norm,
                        int skip_nonfinite, ud_stream_t stream);
int ud_optim_clip_adamw_ema(const UdOptimChunk* chunks, int n_chunks, float* const* params, float* const* exp_avg,
                            float* const* exp_avg_sq, float* const* ema, const float* const* grads,
                            const double* partial, double* state, double beta1, double beta2, double eps,
                            double weight_decay, double max_norm, int skip_nonfinite, double ema_decay, double ema_ramp,
                            ud_stream_t stream);
int ud_optim_swap(const UdOptimChunk* chunks, int n_chunks, float* const* a_ptrs, float* const* b_ptrs,
                  ud_stream_t stream);

/* ---- LiDAR depth supervision of the camera student's lift (csrc/depth_sup.hip) ---------------------------
 * The BEVDepth recipe: the collated cloud is projected into the key frame's images, every feature cell keeps its
 * MINIMUM depth, the depth net's softmax is trained against that cell's depth bin with binary cross entropy.
 *   ud_depth_labels    points f32[B, Nmax, >= 3] (element strides stride_b, stride_n; x y z contiguous), the post-BDA
 *                      cloud.  sensor2ego / intrin / ida f32[B, ncam, 4, 4] of the key frame, bda f32[B, 4, 4] or NULL.
 *                      Per sample and camera, in fp64:  q = (bda . sensor2ego)^-1 . (x, y, z, 1);  (x', y', w) = upper
 *                      3x3 of intrin . q;  (u, v, d, 1) = ida . (x' / w, y' / w, q.z, 1).  A point counts when x, y, z,
 *                      u, v, d are finite, d_lo <= d < d_hi, 0 <= u < W, 0 <= v < H; rows with x == y == z == 0 are
 *                      padding.  Cell (floor(v / downsample), floor(u / downsample)) keeps the minimum of (float)d.
 *                      dmin f32[B, ncam, H / downsample, W / downsample] (+inf where empty), label i32 of that shape =
 *                      floor((dmin - d_lo) / d_step) when inside [0, D), else -1.  Independent of the order of the
 *                      points, bitwise reproducible.  Three launches (two when Nmax == 0).
 *   ud_depth_loss_fwd  logits f32[BN, D, fH, fW] through element strides (sn, sc, sh, sw), D <= 256; label i32[BN, fH,
 *                      fW].  p = softmax over D, t = onehot(label), fg = label in [0, D):
 *                      result[0] = sum over fg pixels and bins of BCE(p, t) / max(1, |fg|) with both logs clamped at
 *                      -100 (torch's binary_cross_entropy), result[1] = |fg|.  Ordered reduction: bitwise
 *                      reproducible; exactly 0 without a foreground pixel.  Two launches.
 *   ud_depth_loss_bwd  dx (strides dn, dc, dh, dw) = grad_out[0] * d result[0] / d logits, with torch's
 *                      dBCE/dp = (p - t) / max((1 - p) p, 1e-12); exact zeros at pixels without a label.  One launch.
 * No host synchronisation, no allocation; scratch from the caller. */
size_t ud_depth_labels_workspace_bytes(int B, int ncam);
int ud_depth_labels(const float* points, int64_t stride_b, int64_t stride_n, int B, int Nmax, const float* sensor2ego,
                    const float* intrin, const float* ida, const float* bda, int ncam, int H, int W, int downsample,
                    double d_lo, double d_hi, double d_step, int D, float* dmin, int32_t* label, void* workspace,
                    size_t workspace_bytes, ud_stream_t stream);
size_t ud_depth_loss_workspace_bytes(int BN, int fH, int fW);
int ud_depth_loss_fwd(const float* logits, int64_t sn, int64_t sc, int64_t sh, int64_t sw, const int32_t* label, int BN,
                      int D, int fH, int fW, float* result, void* workspace, size_t workspace_bytes, ud_stream_t stream);
int ud_depth_loss_bwd(const float* logits, int64_t sn, int64_t sc, int64_t sh, int64_t sw, const int32_t* label,
                      const float* result, const float* grad_out, float* dx, int64_t dn, int64_t dc, int64_t dh,
                      int64_t dw, int BN, int D, int fH, int fW, ud_stream_t stream);

/* ---- GT-sampling (database paste) in the LiDAR input chain (csrc/gt_paste.hip, csrc/lidar_prep.hip) ----
 * OpenPCDet's DataBaseSampler as the reference's GTSampling configures it (transforms3d.py:162-207), between
 * CollectLidarSweeps and BevAffineTransformation: database objects that collide with nothing are pasted into the scene,
 * the scene's points inside their (enlarged) boxes are removed.
 *   ud_gt_paste_select   Per sample b: scene boxes gt f32 [gt_off[b] .. gt_off[b+1])[7] (x, y, z, dx, dy, dz, yaw; before
 *                        BDA), candidates cand f32 [cand_off[b] .. cand_off[b+1])[7] with cand_group i32 (ascending; a
 *                        group is a run of equal ids), at most UD_GT_PASTE_MAX_CAND per sample.  accept u8
 *                        [B][accept_stride] (accept_stride >= every sample's candidates; bytes past them are 0).  Groups
 *                        in order; a candidate is accepted iff its rotated-BEV IoU (ud_boxes_iou_bev's arithmetic) is
 *                        exactly 0 with every scene box, with every ACCEPTED candidate of an earlier group and with every
 *                        OTHER candidate of its own group (two colliding candidates of a group are both dropped; not a
 *                        greedy NMS).  A candidate with a non-finite entry is rejected and blocks nobody; a non-finite
 *                        scene box collides with nobody.  One workgroup per sample, one launch, no atomics; the offsets
 *                        are given on the host (validation) and on the device.
 *   ud_lidar_paste_count / ud_lidar_paste_compact   ud_lidar_prep_count / _compact (same plan, same kernels, same
 *                        workspace and output contract) with, per segment, seg_paste[s] (device, or NULL for none):
 *                          src    the segment's rows are read from src (row 0 = the segment's first) instead of pts;
 *                                 pts may be NULL when every segment has one (rows = seg_host[S] then);
 *                          gate   when not NULL and *gate == 0 every row of the segment is dropped;
 *                          object != 0: an object segment, never tested against the removal boxes;
 *                        and per sample the removal boxes rm_boxes f32 [rm_off[b] .. rm_off[b+1])[7] (at most
 *                        UD_GT_PASTE_MAX_CAND; rm_off NULL on host and device: none), box j active when
 *                        rm_accept[b * rm_stride + j] != 0.  A row of a scene segment is dropped when its float32
 *                        position after the segment transform, BEFORE the BDA, lies inside an active box:
 *                          sx = x - cx, sy = y - cy;   |z - cz| <= dz / 2;
 *                          lx = sx * cos(yaw) + sy * sin(yaw),   ly = -sx * sin(yaw) + sy * cos(yaw);
 *                          |lx| < dx / 2 + 1e-5  and  |ly| < dy / 2 + 1e-5
 *                        all in float32 (OpenPCDet's check_pt_in_box3d).  BDA, range test, stable compaction and both
 *                        output layouts are those of ud_lidar_prep_*, for object rows too.  Object clouds are ordinary
 *                        segments placed ahead of the key frame: gate = the candidate's accept byte, matrix = the
 *                        translation by its box centre (database clouds are box-centred), last = NaN.
 *                        UD_ERR_INVALID_ARG, nothing launched: everything ud_lidar_prep_* rejects (more than
 *                        UD_LIDAR_MAX_SEGMENTS segments in a sample: 1 + sweeps + candidates > 64), more than
 *                        UD_GT_PASTE_MAX_CAND removal boxes in a sample, rm_stride below a sample's boxes. */
#define UD_GT_PASTE_MAX_CAND 63
typedef struct {
  const float* src;
  const uint8_t* gate;
  int64_t object;
} UdLidarPasteSeg;
int ud_gt_paste_select(const float* gt, const int64_t* gt_off_host, const int64_t* gt_off_dev, const float* cand,
                       const int32_t* cand_group, const int64_t* cand_off_host, const int64_t* cand_off_dev, int B,
                       uint8_t* accept, int64_t accept_stride, ud_stream_t stream);
int ud_lidar_paste_count(const float* pts, int64_t rows, int D, const int64_t* seg_host, const int64_t* sample_seg_host,
                         int S, int B, const int64_t* seg_dev, const int64_t* sample_seg_dev, const double* seg_par,
                         const double* smp_par, const UdLidarPasteSeg* seg_paste, const float* rm_boxes,
                         const int64_t* rm_off_host, const int64_t* rm_off_dev, const uint8_t* rm_accept,
                         int64_t rm_stride, int64_t* counts, void* workspace, size_t workspace_bytes, ud_stream_t stream);
int ud_lidar_paste_compact(const float* pts, int64_t rows, int D, const int64_t* seg_host,
                           const int64_t* sample_seg_host, int S, int B, const int64_t* seg_dev,
                           const int64_t* sample_seg_dev, const double* seg_par, const double* smp_par,
                           const UdLidarPasteSeg* seg_paste, const float* rm_boxes, const int64_t* rm_off_host,
                           const int64_t* rm_off_dev, const uint8_t* rm_accept, int64_t rm_stride,
                           const int64_t* counts_host, const int64_t* counts, int64_t nmax, int compact, float* out,
                           int64_t out_rows, void* workspace, size_t workspace_bytes, ud_stream_t stream);

/* ---- Building the GT-sampling object database (csrc/gt_database.hip) ---------------------------------
 * OpenPCDet's create_groundtruth_database on the device: which box owns each point of whole scenes, then every box's
 * points as a box-centred cloud.  The scenes lie back to back: pts f32, row i at pts + i * pts_stride (floats,
 * pts_stride >= D >= 3; columns 0..2 are x, y, z), seg[B + 1] row offsets with seg[0] == 0 and seg[B] == rows; boxes
 * f32, box g at boxes + g * box_stride (box_stride >= W >= 7; x, y, z, dx, dy, dz, yaw, the rest not read),
 * box_off[B + 1] with box_off[0] == 0; n_boxes = box_off[B] <= 262 144.  Offsets are given on the host (validation,
 * grid size) and on the device.
 *   ud_points_in_boxes   owner i32 [rows]: the index WITHIN ITS SAMPLE of the lowest-numbered box that contains the row,
 *                        or -1 (points_in_boxes_gpu, whose loop leaves at the first hit).  The inside test is the paste's
 *                        (ud_lidar_paste_*, above), float32.  A box with a non-finite entry among its first 7 contains
 *                        nothing; a row with a non-finite x, y or z gets -1.  One launch, any number of boxes per sample.
 *   ud_gt_db_count       counts i64 [n_boxes + 1] (device): rows owned by each box, in (sample, box) order, and their
 *                        total in counts[n_boxes].  An owner outside its sample's boxes counts as -1.  Leaves the hit list
 *                        in the workspace for ud_gt_db_extract: same workspace, same stream, nothing in between.
 *   ud_gt_db_extract     counts_host = counts read back.  out f32 [total][D], dense: the boxes' clouds back to back in
 *                        (sample, box) order, inside a box ascending by input row (a stable partition); columns 0..2 are
 *                        x - cx, y - cy, z - cz, one float32 subtraction each, every other column is copied bit for bit.
 *                        No row at or beyond out_rows is written.
 *   Three launches for the count, three per 9 key bits (stable radix sort of the hits by box) plus one for the extract.
 *   Integer counting only, every output element written once: bitwise reproducible.  ud_gt_db_workspace_bytes(rows,
 *   n_boxes) -> bytes (0 for rows == 0 or an invalid size).
 *   UD_ERR_INVALID_ARG, nothing launched: D < 3, W < 7, a stride below D / W, offsets that descend or do not span
 *   0 .. rows, rows >= 2^31, too many boxes, counts_host negative / not summing to counts_host[n_boxes] / above rows,
 *   out_rows below the total, a NULL pointer to something non-empty.  All sizes zero: UD_OK, nothing done. */
int ud_points_in_boxes(const float* pts, int64_t rows, int D, int64_t pts_stride, const int64_t* seg_host,
                       const int64_t* seg_dev, const float* boxes, int W, int64_t box_stride,
                       const int64_t* box_off_host, const int64_t* box_off_dev, int B, int32_t* owner,
                       ud_stream_t stream);
size_t ud_gt_db_workspace_bytes(int64_t rows, int64_t n_boxes);
int ud_gt_db_count(const int32_t* owner, int64_t rows, const int64_t* seg_host, const int64_t* seg_dev,
                   const int64_t* box_off_host, const int64_t* box_off_dev, int B, int64_t* counts, void* workspace,
                   size_t workspace_bytes, ud_stream_t stream);
int ud_gt_db_extract(const float* pts, int64_t rows, int D, int64_t pts_stride, const float* boxes, int W,
                     int64_t box_stride, int64_t n_boxes, const int64_t* counts_host, float* out, int64_t out_rows,
                     void* workspace, size_t workspace_bytes, ud_stream_t stream);

/* ---- Depth metric of the camera student's lift (csrc/depth_metric.hip) ------------------------------
 * The monocular-depth figures of the lift against the LiDAR minimum depth, accumulated on the device.
 *   logits f32[BN, D, fH, fW] through element strides (sn, sc, sh, sw), D <= 256: NCHW or the channels-last slice
 *   depth_feature[:, :D], no copy.  dmin f32[BN, fH, fW] as ud_depth_labels writes it (+inf = no LiDAR return).
 *   A pixel is labelled when dmin is finite and b = floor(((double)dmin - d_lo) / d_step) lies in [0, D): ud_depth_labels'
 *   own expression, so the pixel set is its label >= 0 bit for bit.  Per labelled pixel, in fp32 (the two sums over D are
 *   carried in fp64 and rounded to fp32 once): p = softmax over D with the maximum subtracted;  dhat = sum_j p_j * (d_lo + (j + 0.5) * d_step), the expectation over the bin CENTRES (label
 *   bin j covers [d_lo + j * d_step, d_lo + (j + 1) * d_step));  ahat = the arg-max bin, the lowest index on a tie.
 *   With d = dmin and e = dhat - d, in fp64 from the fp32 dhat, the T = 12 terms in this order:
 *     0 count   1 sum |e|   2 sum |e| / d   3 sum e^2 / d   4 sum e^2   5 sum (ln dhat - ln d)^2
 *     6..8 #[max(dhat / d, d / dhat) < 1.25^k], k = 1, 2, 3   9 #[ahat == b]   10 #[|ahat - b| <= 1]
 *     11 sum -ln max(p_b, 1e-44)
 *   Group g = n mod ncam_groups (ncam for a per-camera breakdown of [B * ncam] images, 1 for none); range bucket r = the
 *   first r with range_edges[r] <= d < range_edges[r + 1] (range_edges: n_ranges + 1 strictly ascending doubles on the
 *   HOST, read before the call returns; 1 <= n_ranges <= 8); a labelled pixel outside every bucket is counted in none.
 *   state f64[ncam_groups, n_ranges, 12] += this call (the caller zeroes it once).  Every 64 consecutive pixels of an
 *   image make one fp64 partial row in the workspace, a second launch adds the rows in a fixed order: no floating-point
 *   atomics, bitwise reproducible, the partition a function of the shape alone.  Two launches, no host
 *   synchronisation, no allocation.  UD_ERR_INVALID_ARG with nothing launched: D outside 1..256, n_ranges outside
 *   1..8, edges that do not ascend, ncam_groups < 1, BN % ncam_groups != 0, a negative size.  BN == 0 or fH * fW == 0: UD_OK, nothing done. */
size_t ud_depth_metric_workspace_bytes(int BN, int fH, int fW);
int ud_depth_metric_accumulate(const float* logits, int64_t sn, int64_t sc, int64_t sh, int64_t sw, const float* dmin,
                               int BN, int D, int fH, int fW, int ncam_groups, double d_lo, double d_step,
                               const double* range_edges, int n_ranges, double* state, void* workspace,
                               size_t workspace_bytes, ud_stream_t stream);

/* ---- Flip test-time augmentation: merge of the head maps of V flipped views (csrc/tta_merge.hip) -----
 * One launch for all T <= 8 tasks and their seven heads; nothing synchronises with the host, no workspace, no atomics,
 * bitwise reproducible.
 *   heads / strides      HOST arrays [T*7] / [T*7*3] as for ud_proposal_layer (hm, reg, height, dim, rot, vel, iou; fp32,
 *                        logical shape [V*B, c, H, W]; (batch, channel, pixel) element strides: NCHW planes or channel slices
 *                        of a channels-last map).  View v of sample b is row v * B + b.  A NULL pointer: the head is absent
 *                        and nothing is written for it; hm must be present.  c = num_classes[t] for hm, else 2 1 3 2 2 1.
 *   outs / out_strides   the same two tables for the outputs, logical shape [B, c, H, W] (strides below 2^31).
 *   flips                HOST int [V*2]: (flip_dx, flip_dy) of each view, 1 <= V <= 4, any combinations in any order.
 * Output pixel (y, x) reads pixel (flip_dy ? H-1-y : y, flip_dx ? W-1-x : x) of view v; flip_dx mirrors the x axis.  The
 * un-flipped terms are added for v = 0 .. V-1 in that order, starting from view 0's term, and the sum is multiplied by the
 * fp32 value 1 / V.  Terms: reg[0]: flip_dx ? 1 - r : r; reg[1]: flip_dy ? 1 - r : r; rot[0] (sin) and vel[1]: negated under
 * flip_dy; rot[1] (cos) and vel[0]: negated under flip_dx; height, iou: as they are; dim: as it is when no_log, else exp(d),
 * and the output is log(mean), not clamped; hm: sigmoid(h) = 1 / (1 + exp(-h)), and the output is logit(mean) = log(m) -
 * log1p(-m): -inf when the mean rounds to 0, +inf when it rounds to 1, never NaN for finite inputs.  The sums of hm and of
 * a logarithmic dim, and their way back, are carried in double and rounded to fp32 once; all other heads are fp32 throughout.
 * The rules are exact for a BEV range that is symmetric about 0 on each flipped axis (the caller's check).
 * UD_ERR_INVALID_ARG with nothing launched: V outside 1..4, B, T, H, W out of range, a missing table, hm or output pointer,
 * a negative stride; UD_ERR_UNSUPPORTED: more than 256 channels in all, or B*H*W*channels >= 2^31. */
int ud_tta_merge(const float* const* heads, const long long* strides, float* const* outs, const long long* out_strides,
                 const int* num_classes, const int* flips, int V, int B, int T, int H, int W, int no_log,
                 ud_stream_t stream);

/* ---- Rotation / scale / flip test-time augmentation: resampling merge of V views (csrc/tta_merge_affine.hip)
 * The tables heads / strides / outs / out_strides / num_classes, the view-major rows, the layouts and the output are those
 * of ud_tta_merge (every stride below 2^31 here); one launch, no workspace, no atomics, bitwise reproducible.
 *   view_params          HOST double [V*11], 1 <= V <= 16, per view: T (row-major 2x3), Ti (row-major 2x2), s.  Cell (x, y)
 *                        covers [x, x+1) x [y, y+1) in cell units u; T takes original-frame u to view-frame u
 *                        (T = C^-1 A_v C with A_v = F S R of the view, C: u -> u * cell + range_min), Ti is the inverse of
 *                        T's linear part, s > 0 the view's scale.  All finite.  View 0 maps the grid onto itself: s = 1 and
 *                        per axis (1, 0) or (-1, size) as (linear entry, offset), the cross entries 0.
 *   cell_ratio           cell_x / cell_y, > 0: metres L^-1_ij = Ti_ij * cell_i / cell_j.
 * Output pixel p samples view v at q = T (p + 1/2): g = q - 1/2, i0 = floor(g), f = g - i0, neighbours i0 and i0 + 1 per
 * axis with weights 1 - f and f, all in double.  A view contributes at p only if every neighbour of non-zero weight lies inside
 * the map; the blended terms of the contributing views are added in the views' order and divided by their number n(p) >= 1.
 * Terms, per neighbour n, brought into the original frame before the blend: hm: sigmoid(h), the output logit(min(mean, 1)) =
 * log m - log1p(-m), never NaN; dim: exp(d) / s and the output log(mean), under no_log d / s; height: z / s; iou: as it is;
 * reg: Ti (n + reg - T's offset) - p, the offset of the predicted centre from the output cell's corner (1 - r for a flip);
 * vel: L^-1 v; rot (sin, cos): the vector (cos, sin) multiplied by s L^-1, not renormalised.  hm and a logarithmic dim are
 * carried in double, weights included, and rounded to fp32 once; the other heads are fp32 one operation at a time with
 * fp32-rounded weights and coefficients (tests/tta_affine_reference.py: merge32 restates the order).
 * UD_ERR_INVALID_ARG with nothing launched: V outside 1..16, B, T, H, W out of range, a missing table, hm or output pointer,
 * a negative stride, a non-finite parameter, s <= 0, cell_ratio <= 0, a view 0 that does not map the grid onto itself;
 * UD_ERR_UNSUPPORTED: a stride >= 2^31, more than 256 channels in all, or B*H*W*channels >= 2^31. */
int ud_tta_merge_affine(const float* const* heads, const long long* strides, float* const* outs,
                        const long long* out_strides, const int* num_classes, const double* view_params, double cell_ratio,
                        int V, int B, int T, int H, int W, int no_log, ud_stream_t stream);

/* ---- Box-level fusion (weighted box fusion) of TTA views and ensembles (csrc/box_fusion.hip) -----------------
 * Fuses the decoded boxes of S sources (views or models) per sample.  Three launches; nothing synchronises with the host, no
 * allocation, no floating-point atomics, bitwise reproducible.
 *   rois / scores / labels / num   DEVICE f32[S*B, R, box_dim] / f32[S*B, R] / i64[S*B, R] / i32[S*B]: ud_proposal_layer's padded
 *                        outputs, read in place; source s of sample b is row s * B + b; rows at or beyond num (clamped to 0..R)
 *                        are never read.  box_dim 7 or 9: (x, y, z, dx, dy, dz, yaw[, vx, vy]).
 *   views                HOST double [S*6], per source: rot_deg, scale > 0, flip_dx, flip_dy, sin, cos of the rotation (the
 *                        caller's: ops.tta._sincos, exact at multiples of 90 degrees; sin^2 + cos^2 = 1 within 1e-12).
 *   weights              HOST double [S], each > 0.
 * Un-view (double, from the fp32 inputs; A_v = F S R): (x, y) = R^T F (x', y') / s, z = z' / s, dims = dims' / s, (vx, vy) =
 * R^T F (vx', vy') / s; yaw = yaw' - rot | -yaw' - rot (flip_dy) | pi - yaw' - rot (flip_dx) | pi + yaw' - rot (both), rot =
 * rot_deg / 180 * pi.  A box is valid iff every entry and the score are finite, score > score_threshold and 0 <= label <= 65535;
 * others count nowhere.  Order per sample: (label ascending, score descending, source ascending, row ascending).  Clusters: greedy
 * NMS within a label on the un-viewed boxes rounded to fp32, ud_boxes_iou_bev's arithmetic with the earlier box first, strict
 * IoU > iou_threshold; an unsuppressed box is an anchor, a suppressed box joins the first anchor in order that suppresses it,
 * suppressed boxes suppress nobody.  Fusion in double over the un-viewed values, members in order, anchor first, c_i = w_s(i) *
 * score_i: centre, dims, velocity = sum c_i v_i / sum c_i; yaw = yaw_a + sum c_i d_i / sum c_i wrapped into [-pi, pi), d_i =
 * yaw_i - yaw_a wrapped to (-pi, pi] and folded by -+pi into [-pi/2, pi/2]; score = sum c_i / max(sum_i w_s(i), sum_s w_s);
 * each rounded to fp32 once.
 * Outputs (DEVICE): out_rois f32[B, max_out, box_dim], out_scores f32[B, max_out], out_labels i64[B, max_out], zero padded, the
 * clusters by fused fp32 score descending, ties in anchor order, cut at max_out; out_num i32[B]; status i32[B]: 1 for a sample
 * with more than 16384 valid boxes (possible only when S * R > 16384), which is not fused: its out_num is 0.  Optional (NULL
 * to skip) out_anchor i32[B, max_out]: s * R + r of each cluster's anchor (-1 in the padding), out_members i32[B, max_out]: its
 * member count.
 * UD_ERR_INVALID_ARG with nothing launched: B outside 1..65535, S outside 1..16, R < 1, S * R > 2^24, box_dim not 7 or 9,
 * max_out < 1, a non-finite iou_threshold, a NaN score_threshold, a non-finite view entry, scale or weight <= 0, a missing
 * pointer; UD_ERR_WORKSPACE: less than ud_box_fusion_workspace_bytes(B, S, R) (0 for sizes out of range). */
size_t ud_box_fusion_workspace_bytes(int B, int S, int R);
int ud_box_fusion(const float* rois, const float* scores, const long long* labels, const int* num, int B, int S, int R,
                  int box_dim, const double* views, const double* weights, float iou_threshold, float score_threshold,
                  int max_out, float* out_rois, float* out_scores, long long* out_labels, int* out_num, int* status,
                  int* out_anchor, int* out_members, void* workspace, size_t workspace_bytes, ud_stream_t stream);

/* ---- Multi-object tracking of the validation predictions (csrc/track.hip) -----------------------------------
 * CenterPoint's greedy, velocity-compensated centre association over the rows of ud_nus_pred_to_global, every scene in one
 * launch (one workgroup per scene, its frames in order); tests/tracking_reference.py restates it in numpy.  Nothing
 * synchronises with the host, no allocation, no floating-point atomics, bitwise reproducible.
 *   rec / cls            DEVICE f64[num_rows][UD_NUS_PRED_COLS] / i32[num_rows]: the evaluator's prediction rows.
 *   row_start / row_count  DEVICE i64[num_samples]: sample s owns rows row_start[s] .. + row_count[s] (samples in any order).
 *   frame_sample         DEVICE i64[num_frames]: the sample of every frame, scene after scene, each scene's frames in time order.
 *   scene_off            DEVICE i64[num_scenes + 1]: scene k = frames scene_off[k] .. scene_off[k + 1].
 *   frame_dt             DEVICE f64[num_frames]: seconds since the scene's previous frame, 0 for its first.
 * Per scene: no tracks, id counter 0.  Per frame: (1) candidates = rows with track_class[cls] and score >= score_threshold, by
 * descending score, equal scores by ascending row; such a row with a non-finite translation, velocity or score sets
 * UD_TRACK_ST_NONFINITE and is no candidate.  (2) every track coasts: ct = ct + v * dt in x and y, a rounded multiply then a
 * rounded add.  (3) candidates in order: among the unclaimed tracks of the candidate's class, d2 = dx * dx + dy * dy to the
 * coasted centre; the smallest d2 wins, the lowest slot on a tie, and is claimed if d2 <= max_dist[cls] * max_dist[cls].
 * (4) the new list: one entry per candidate in order (a match keeps the id, hits = hits + 1 if the track was seen in the
 * previous frame and 1 otherwise; no match: the next id, from 1 per scene, hits = 1; centre, velocity and class of the
 * detection, age 0), then the unclaimed tracks in their old order with age + 1, dropped when that reaches max_age.
 * Outputs (DEVICE, i32[num_rows]): track_id (0: the row is no candidate of a listed frame) and track_hits; *status i32, OR-ed:
 * UD_TRACK_ST_NONFINITE; UD_TRACK_ST_COUNT (a frame with more than UD_NUS_MAX_BOXES rows: treated as empty); UD_TRACK_ST_RANGE
 * (a frame's sample, a sample's rows or a scene's frames outside the inputs: treated as empty).
 * UD_ERR_INVALID_ARG with nothing launched: num_scenes < 1, max_age outside 1 .. UD_TRACK_MAX_AGE, num_classes outside 1 ..
 * UD_NUS_MAX_CLASSES, num_rows >= 2^31, a NaN threshold, a NaN or negative max_dist of a tracked class, a missing pointer;
 * UD_ERR_WORKSPACE: less than ud_track_workspace_bytes(num_scenes, max_age) (0 for sizes out of range). */
#define UD_TRACK_MAX_AGE 8
#define UD_TRACK_ST_NONFINITE 1
#define UD_TRACK_ST_COUNT 2
#define UD_TRACK_ST_RANGE 4

typedef struct {
  int num_classes;
  int max_age;
  int64_t num_rows, num_samples, num_frames, num_scenes;
  double score_threshold;
  double max_dist[UD_NUS_MAX_CLASSES];        /* metres, per class */
  uint8_t track_class[UD_NUS_MAX_CLASSES + 1]; /* non-zero: the class is tracked */
} UdTrackCfg;

size_t ud_track_workspace_bytes(int64_t num_scenes, int max_age);
int ud_track_scenes(const double* rec, const int32_t* cls, const int64_t* row_start, const int64_t* row_count,
                    const int64_t* frame_sample, const int64_t* scene_off, const double* frame_dt,
                    const UdTrackCfg* cfg_host, int32_t* track_id, int32_t* track_hits, int32_t* status, void* workspace,
                    size_t workspace_bytes, ud_stream_t stream);

/* ---- The nuScenes tracking metric (csrc/track_metric.hip) -----------------------------------------------------
 * AMOTA, AMOTP, MOTA, IDS and the other figures of the devkit's TrackingEval over the rows and ids of ud_track_scenes, scored as
 * given (no interpolation of tracks); tests/track_metric_reference.py restates it in float64 Python with scipy's assignment.
 * Everything is enqueued on `stream` without a host wait; no allocation, no floating-point atomics, bitwise reproducible.
 *   pred_rec / pred_cls / track_id   DEVICE f64[num_rows][UD_NUS_PRED_COLS] / i32 / i32: the evaluator's rows and their ids.
 *   row_start / row_count            DEVICE i64[num_samples]: the prediction rows of sample s.
 *   gt_xyz / gt_cls / gt_num_pts / gt_keep / gt_inst   DEVICE f64[num_gt][3] / i32 / i32 / u8 / i32, sorted by sample:
 *                                    gt_inst numbers the object densely within its (scene, class), below max_instances; an
 *                                    object appears at most once per sample.  gt_off DEVICE i64[num_samples + 1].
 *   ego                              DEVICE f64[num_samples][3]; frame_sample / scene_off as for ud_track_scenes.
 *   recall                           DEVICE f64[num_thresholds]: the recall thresholds r_k.
 * ROWS.  A GT row is kept iff gt_keep, gt_num_pts > 0, its class is tracked and sqrt(dx * dx + dy * dy) to its sample's ego
 * translation is <= class_range.  A prediction row is kept iff track_id > 0, its class is tracked and it passes the same test.
 * A non-finite translation (or score) sets UD_TM_ST_NONFINITE and drops the row; a sample with more than max_boxes_per_sample
 * kept predictions sets UD_TM_ST_BOXES; a kept row whose id exceeds max_scene_rows sets UD_TM_ST_ID and is dropped.
 * TRACK SCORE.  A kept prediction row's score is the mean detection score over the kept rows of its (scene, id), summed in
 * (frame, row) order, then divided.
 * ONE PASS = (class c, scene, threshold theta or "all boxes"); its state m: GT instance -> track id last matched, empty at the
 * scene's first frame, kept through frames that miss the object.  Per frame, in (timestamp, sample) order:
 *   1 hypotheses = kept prediction rows of class c with score >= theta, objects = kept GT rows of class c; a frame with neither
 *     is skipped and not counted.  d(o, h) = sqrt(dx * dx + dy * dy); a pair is admissible iff d < dist_th_tp (tested on d).
 *   2 objects in GT row order: if m[o] exists and an unclaimed hypothesis with that id is admissible (the first such in row
 *     order), the pair is a MATCH and both leave.
 *   3 among the rest: the matching over admissible pairs with the most pairs, and among those the least sum of d.  A pair is a
 *     SWITCH if m[o] exists and differs from the hypothesis' id, else a MATCH; m[o] = id.  Solver: objects and hypotheses
 *     without an admissible partner leave; the smaller side becomes the rows of a shortest-augmenting-path assignment (rows in
 *     order, forbidden pairs cost UD_TM_MAX_FRAME_ROWS * dist_th_tp + 1); equal reduced costs go to the lowest column.  Where
 *     several matchings are optimal this fixes one, the same in every run.
 *   4 unmatched objects are MISS, unmatched hypotheses FP.
 * Per pass and scene: the UD_TM_COUNTS integers frames, objects, matches, switches, fp, miss, mt (tracked / appearances >= 0.8
 * per instance), ml (< 0.2), frag (MISS after a tracked appearance, later tracked again: once per gap), tid (frames of the
 * scene's list from the first to the first tracked appearance) and lgd (longest run of MISS appearances), both summed over the
 * instances tracked at least once, and that instance count; dist_sum = the sum of d over MATCH and SWITCH pairs in (frame, GT
 * row) order.  Scenes are then added in scene order (integers and dist_sum alike).
 * THRESHOLDS.  s = the scores of the all-boxes pass's MATCH hypotheses, descending, n of them; P = objects; rec[i] = (i + 1) / P;
 * theta_k = s[0] where r_k <= rec[0], s[j] at a knot, else s[j] + ((s[j+1] - s[j]) / (rec[j+1] - rec[j])) * (r_k - rec[j]) with
 * rec[j] < r_k < rec[j+1]; NaN where r_k > n / P, P = 0 or n = 0: that pass is not run (valid = 0, zeros).
 * Outputs (DEVICE): counts i64[T][num_thresholds + 1][UD_TM_COUNTS], dist_sum f64 and valid i32 [T][num_thresholds + 1] (T =
 * tracked classes in class order; entry 0 = all boxes), thresholds f64[T][num_thresholds], num_scores i64[T] (n); with
 * events_pass >= -1 (-1 = all boxes, k = threshold k, -2 = off) events_type i32[num_gt] (-1 not kept, 0 MISS, 1 MATCH, 2
 * SWITCH) and events_row (the matched prediction row or -1) of that pass; *status i32, OR-ed (also UD_TM_ST_RANGE: a layout
 * entry outside the inputs, treated as empty; UD_TM_ST_INTERNAL: the solver's guard).
 * UD_ERR_INVALID_ARG with nothing launched: classes outside 1 .. UD_NUS_MAX_CLASSES or none tracked, num_thresholds outside
 * 1 .. UD_TM_MAX_THRESHOLDS, max_frame_rows (the most GT or prediction rows of one sample) above UD_TM_MAX_FRAME_ROWS,
 * max_instances above UD_TM_MAX_INSTANCES, a missing pointer, a bad dist_th_tp or range; UD_ERR_WORKSPACE as usual. */
#define UD_TM_MAX_FRAME_ROWS 512
#define UD_TM_MAX_INSTANCES 4096
#define UD_TM_MAX_THRESHOLDS 64
#define UD_TM_COUNTS 12
#define UD_TM_ST_NONFINITE 1
#define UD_TM_ST_BOXES 2
#define UD_TM_ST_RANGE 4
#define UD_TM_ST_ID 8
#define UD_TM_ST_INTERNAL 16

typedef struct {
  int num_classes;
  int num_thresholds;
  int max_boxes_per_sample;
  int events_pass;       /* -2 off, -1 the all-boxes pass, k the pass of threshold k */
  int max_frame_rows;    /* the most GT rows, or prediction rows, of one sample */
  int max_instances;     /* the most GT instances of one (scene, class) */
  int64_t num_rows, num_gt, num_samples, num_frames, num_scenes;
  int64_t max_scene_rows; /* the most prediction rows of one scene: ids lie in 1 .. max_scene_rows */
  double dist_th_tp;
  double class_range[UD_NUS_MAX_CLASSES];
  int64_t class_gt[UD_NUS_MAX_CLASSES];        /* GT rows per class */
  uint8_t track_class[UD_NUS_MAX_CLASSES + 1]; /* non-zero: the class is tracked */
} UdTrackMetricCfg;

size_t ud_track_metric_workspace_bytes(const UdTrackMetricCfg* cfg);
int ud_track_metric(const double* pred_rec, const int32_t* pred_cls, const int32_t* track_id, const int64_t* row_start,
                    const int64_t* row_count, const double* gt_xyz, const int32_t* gt_cls, const int32_t* gt_num_pts,
                    const uint8_t* gt_keep, const int32_t* gt_inst, const int64_t* gt_off, const double* ego,
                    const int64_t* frame_sample, const int64_t* scene_off, const double* recall,
                    const UdTrackMetricCfg* cfg_host, int64_t* counts, double* dist_sum, int32_t* valid, double* thresholds,
                    int64_t* num_scores, int32_t* events_type, int32_t* events_row, int32_t* status, void* workspace,
                    size_t workspace_bytes, ud_stream_t stream);

/* ---- Interpolation of tracks across missed frames (csrc/track_interp.hip) -------------------------------------
 * What the devkit's tracking evaluation does to every ground-truth track and every predicted track after its filters and before
 * it scores them; tests/track_interp_reference.py restates it in float64 Python.  Two calls, because the size of the output
 * depends on the data: ud_track_interp_count (counts), then -- after the caller has read the counts and laid the output out --
 * ud_track_interp_fill (rows).  Integer counting only, no floating-point atomics, every interpolated value is written by one
 * thread from its two endpoints, bitwise reproducible, independent of what the workspace held before.
 * A SIDE is the predictions or the ground truth.  Each side has rows in the evaluator's layout (float64 columns, cls, per sample
 * a first row and a row count), an int32 track key per row (predictions: the tracker's track_id; GT: a number dense within the
 * scene, below UD_TI_MAX_GT_KEYS, that the host derives from the instance), the frames of ud_track_scenes (frame_sample /
 * scene_off) and frame_ts DEVICE i64[num_frames]: the timestamp in microseconds of every frame, strictly ascending in a scene.
 *   1 KEPT ROWS.  A row is kept by exactly the rule of ud_track_metric, section ROWS (csrc/track_kept.h holds it, once):
 *     predictions track_id > 0, class tracked, xy distance to the sample's ego translation <= class_range; GT gt_keep,
 *     gt_num_pts > 0, class tracked, the same range test.  Such a row with a non-finite column (predictions: all
 *     UD_NUS_PRED_COLS, GT: the translation) sets UD_TI_ST_NONFINITE and is dropped.  A kept row whose key lies outside
 *     1 .. max_scene_rows (predictions) or 0 .. max_gt_keys - 1 (GT) sets UD_TI_ST_KEY and is dropped.  A sample with more
 *     than max_boxes_per_sample kept predictions (the devkit's cap, tested here before interpolation) sets UD_TI_ST_BOXES.
 *   2 TRACKS.  A track is the set of kept rows of one (scene, key).  A key may occur at most once per frame; a second
 *     occurrence sets UD_TI_ST_DUPLICATE (the caller raises).
 *   3 HOLES.  For every frame f of the scene strictly between a track's first and last kept appearance in which the track has no
 *     kept row -- frames without any rows and frames whose own row of the track was dropped in step 1 included -- one
 *     interpolated row is made from the nearest kept appearance before (L) and after (R).  Nothing is extrapolated before the
 *     first or after the last appearance.  Holes have no length bound.
 *   4 WEIGHT.  mode UD_TI_MODE_DEVKIT: w = double(t_R - t_f) / double(t_R - t_L); UD_TI_MODE_LINEAR: w = double(t_f - t_L) /
 *     double(t_R - t_L); the timestamps are subtracted as int64 before the conversion.  The result is (1 - w) * L + w * R.  The
 *     devkit mode restates the devkit's interpolate_tracks as recalled (the ratio from the right timestamp, applied to the right
 *     box, which mirrors time inside a hole); that recollection is unverified, hence the second mode.  The two agree where the
 *     hole is one frame in the middle of its neighbours.
 *   5 COLUMNS.  Translation (3), size (3), velocity (2) and score are each (1 - w) * a + w * b in float64: 1 - w rounded, two
 *     rounded products, one rounded sum, never a fused multiply-add.  Yaw is yaw_L + w * remainder(yaw_R - yaw_L, 2 pi) with
 *     the IEEE remainder (the slerp of two z-axis quaternions along the shorter arc), not re-wrapped.  GT rows carry only the
 *     translation.  An interpolated row takes the class of R and the key of the track; predictions take the interpolated score.
 *   6 OUTPUT.  Each side's output holds only the kept original rows, in their original order, and after them each sample's
 *     interpolated rows in ascending key.  (The order is part of the definition: the metric's dist_sum and the track mean score
 *     are float sums in (frame, row) order.)
 * ud_track_interp_count writes counts DEVICE i64[2 * num_samples + 2 + UD_NUS_MAX_CLASSES]: the output rows of every sample
 * (predictions, then GT), the interpolated rows of the two sides, the GT output rows per class; and ORs into *status.
 * ud_track_interp_fill takes, per side, out_start / out_count DEVICE i64[num_samples] (the caller's layout of exactly those
 * counts; num_out_pred / num_out_gt rows in all) and writes out_rec f64[num_out_pred][UD_NUS_PRED_COLS] / out_xyz
 * f64[num_out_gt][3], out_cls, out_key and out_src i32 (the original row, -1 for an interpolated row).  Inputs that give other
 * counts than the layout holds set UD_TI_ST_RANGE; nothing is written outside a sample's out_count rows.
 * UD_ERR_INVALID_ARG with nothing launched: classes outside 1 .. UD_NUS_MAX_CLASSES or none tracked, num_scenes < 1, more than
 * UD_TM_MAX_FRAME_ROWS rows in a sample, max_gt_keys above UD_TI_MAX_GT_KEYS, a mode other than the two, a bad range or
 * max_boxes_per_sample, a missing pointer; UD_ERR_WORKSPACE: less than ud_track_interp_workspace_bytes (0 for sizes out of
 * range; it depends on num_out_pred / num_out_gt, which are 0 for the count call). */
#define UD_TI_MAX_GT_KEYS 4096 /* = UD_TM_MAX_INSTANCES: the GT keys of the output serve ud_track_metric as gt_inst */
#define UD_TI_MODE_DEVKIT 0
#define UD_TI_MODE_LINEAR 1
#define UD_TI_ST_NONFINITE 1
#define UD_TI_ST_BOXES 2
#define UD_TI_ST_RANGE 4
#define UD_TI_ST_KEY 8
#define UD_TI_ST_DUPLICATE 16

typedef struct {
  int num_classes;
  int mode;                 /* UD_TI_MODE_* */
  int max_boxes_per_sample;
  int max_frame_rows;       /* the most GT rows, or prediction rows, of one sample */
  int64_t num_rows, num_gt, num_samples, num_frames, num_scenes;
  int64_t max_scene_rows;   /* the most prediction rows of one scene: prediction keys lie in 1 .. max_scene_rows */
  int64_t max_gt_keys;      /* GT keys lie in 0 .. max_gt_keys - 1 */
  int64_t num_out_pred, num_out_gt; /* rows of the two outputs: 0 for the count call */
  double class_range[UD_NUS_MAX_CLASSES];
  uint8_t track_class[UD_NUS_MAX_CLASSES + 1]; /* non-zero: the class is tracked */
} UdTrackInterpCfg;

size_t ud_track_interp_workspace_bytes(const UdTrackInterpCfg* cfg);
int ud_track_interp_count(const double* pred_rec, const int32_t* pred_cls, const int32_t* track_id, const int64_t* row_start,
                          const int64_t* row_count, const double* gt_xyz, const int32_t* gt_cls, const int32_t* gt_num_pts,
                          const uint8_t* gt_keep, const int32_t* gt_key, const int64_t* gt_off, const double* ego,
                          const int64_t* frame_sample, const int64_t* scene_off, const int64_t* frame_ts,
                          const UdTrackInterpCfg* cfg_host, int64_t* counts, int32_t* status, void* workspace,
                          size_t workspace_bytes, ud_stream_t stream);
int ud_track_interp_fill(const double* pred_rec, const int32_t* pred_cls, const int32_t* track_id, const int64_t* row_start,
                         const int64_t* row_count, const double* gt_xyz, const int32_t* gt_cls, const int32_t* gt_num_pts,
                         const uint8_t* gt_keep, const int32_t* gt_key, const int64_t* gt_off, const double* ego,
                         const int64_t* frame_sample, const int64_t* scene_off, const int64_t* frame_ts,
                         const UdTrackInterpCfg* cfg_host, const int64_t* pred_out_start, const int64_t* pred_out_count,
                         const int64_t* gt_out_start, const int64_t* gt_out_count, double* out_rec, int32_t* out_pred_cls,
                         int32_t* out_pred_key, int32_t* out_pred_src, double* out_xyz, int32_t* out_gt_cls,
                         int32_t* out_gt_key, int32_t* out_gt_src, int32_t* status, void* workspace, size_t workspace_bytes,
                         ud_stream_t stream);

/* ------------------------------------------------------------------------- */
/* PointPillars encoder: PillarVFE (one PFNLayer, use_norm, last_layer) +     */
/* PointPillarScatter -- csrc/pillars.hip, DESIGN 2.26                        */
/*   layers/blocks_3d/det3d/vfe/pillar_vfe.py:8-145                           */
/*   layers/blocks_2d/det3d/map_to_bev/pointpillar_scatter.py:5-40            */
/* ------------------------------------------------------------------------- */

/*
 * Inputs of all three passes: the voxelizer's output on a one-cell-high grid,
 *   voxels f32[M,P,F] (rows >= num[m] zero)   coords i32[M,4] (b,z,y,x)   num i32[M]   weight f32[C,K]
 * The K row features are never stored: the raw row (its columns 3.. only without UD_PILLAR_ABS_XYZ), xyz - mean_xyz (sum over
 * the P rows / num), xyz - cell centre (coords * voxel_size + offset, fp32), ||xyz|| with UD_PILLAR_DISTANCE; all times
 * (row < num).  K = F + 6 (F + 3 without UD_PILLAR_ABS_XYZ) (+ 1).  geom: HOST f32[6] = voxel_size xyz, offset xyz
 * (voxel_size / 2 + range minimum, evaluated in double by the caller as the reference does).
 * Supported: C % 32 == 0, C <= 256; 3 <= F <= 8; 1 <= P <= 64.  fp32, no float atomics, every sum in a fixed order.
 */
#define UD_PILLAR_ABS_XYZ 1u
#define UD_PILLAR_DISTANCE 2u

/* Scratch of ud_pillar_stats / ud_pillar_bwd for these sizes; 0 for unsupported sizes. */
size_t ud_pillar_workspace_bytes(int M, int P, int F, int C, unsigned flags);

/*
 * Training statistics of z = weight . feat over ALL M * P rows (padded rows count, with z = 0: what the reference's
 * BatchNorm1d sees): stats f32[4,C] = mean, invstd (biased variance + eps), scale = gamma * invstd, shift = beta - mean * scale.
 * running_mean / running_var (NULL to skip): (1 - momentum) * old + momentum * (mean | unbiased variance, n = M * P).
 */
int ud_pillar_stats(const float* voxels, const int32_t* coords, const int32_t* num, int M, int P, int F,
                    const float* weight, int C, unsigned flags, const float* geom, const float* gamma, const float* beta,
                    float eps, float momentum, float* running_mean, float* running_var, float* stats, void* workspace,
                    size_t workspace_bytes, ud_stream_t stream);

/*
 * out[m,c] = max over the P rows of relu(z * scale[c] + shift[c]) (padded rows give relu(shift[c])), written to
 * bev f32[B,ny,nx,C] at (coords b, y, x); bev is zero-filled here first.  pillars f32[M,C] and argmax u8[M,C] (the first row
 * that attains the maximum) are optional (NULL).  A pillar whose coordinates fall outside the map is not written.
 */
int ud_pillar_apply(const float* voxels, const int32_t* coords, const int32_t* num, int M, int P, int F,
                    const float* weight, int C, unsigned flags, const float* geom, const float* scale, const float* shift,
                    int B, int ny, int nx, float* bev, float* pillars, uint8_t* argmax, ud_stream_t stream);

/*
 * Backward of the two passes above for dbev f32[B,ny,nx,C] (plus dpillars f32[M,C], the gradient of the optional pillars
 * output, or NULL): dweight f32[C,K], dgamma / dbeta f32[C] (each NULL to skip).
 * stats / argmax: what the forward used (frozen != 0: stats = running mean, 1 / sqrt(running var + eps), folded scale, shift,
 * and dz = scale * dy on the argmax rows only; otherwise the batch-statistics backward, whose dz is non-zero on every row).
 */
int ud_pillar_bwd(const float* voxels, const int32_t* coords, const int32_t* num, int M, int P, int F, const float* weight,
                  int C, unsigned flags, const float* geom, const float* dbev, const float* dpillars, int B, int ny, int nx,
                  const uint8_t* argmax, const float* stats, int frozen, float* dweight, float* dgamma, float* dbeta, void* workspace,
                  size_t workspace_bytes, ud_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* UNIDISTILL_HIP_H */
