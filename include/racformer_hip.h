/*
 * racformer_hip.h -- C-ABI of libracformer_hip.so (MI355X / gfx950 only).
 *
 * Drop-in boundary for RaCFormer's query-decoder hot path.  Plain pointers and sizes, no torch
 * types, no exceptions across the ABI.  Every entry point returns 0 on success, a negative
 * RAC_E_* code for argument errors (nothing launched) or a positive hipError_t value if the HIP
 * runtime refused the launch; rac_last_error() gives the message for the calling thread.
 * All device pointers must be valid on the current HIP device; kernels are enqueued on `stream`
 * (a hipStream_t; NULL = the legacy default stream, which is what the reference's launcher used,
 * models/csrc/msmv_sampling/msmv_sampling_forward.cu:359).  No allocation, no synchronisation:
 * every call is hipGraph-capturable.
 *
 * Reference interfaces replaced (paths relative to the reference root):
 *   rac_msmv_fwd      <- _ms_deform_attn_cuda_{c45,c2345,c23456}_forward
 *                        models/csrc/msmv_sampling/msmv_sampling.cpp:132-184 (+ :186-236, :238-300),
 *                        pybind at :499-506; Python caller models/csrc/wrapper.py:78-153
 *   rac_msda_fwd      <- mmcv-full 1.6.0 `_ext.ms_deform_attn_forward`, call site
 *                        models/multi_scale_deformable_attn_function.py:118-124
 *   rac_regroup_fwd   <- the channel-last regroup in RaCFormerTransformerDecoder.forward,
 *                        models/racformer_transformer.py:112-124
 *   rac_box_prep_fwd  <- decode_bbox(theta_d2xy_coods(.)) models/bbox/utils.py:66-90 (shared prologue)
 *   rac_sampling4d_fwd<- RaCFormerSampling.inner_forward + sampling_4d + msmv op, fused
 *                        models/racformer_transformer.py:361-419, models/sparsebev_sampling.py:28-134
 *   rac_msmv_bwd / rac_msda_bwd <- the two operators' backward entry points (row f4)
 *   rac_msmv_bwd_ex / rac_msmv_v2_bwd_ex <- the same backwards reading the gradient in sampling_4d's [B,Q,G,T*P,C] layout
 *   rac_msmv_v2_fwd / rac_msmv_v2_bwd <- msmv_sampling_v2 (torch only in the reference: msmv_sampling_pytorch_v2,
 *                        models/csrc/wrapper.py:41-76), called by sampling_4d(aggregate=False), models/sparsebev_sampling.py:122-134
 *   rac_bev_pool_v2_fwd/_bwd <- bev_pool_v2_ext (models/csrc/bev_pool_v2/src/bev_pool.cpp:40-111), row f2
 *   rac_add_ln_fwd    <- residual add + nn.LayerNorm (+ReLU) groups, models/racformer_transformer.py:170-258
 *   rac_layer_boundary_fwd <- rac_refine_fwd + rac_box_prep_fwd + rac_pe_head_fwd of consecutive layers, one launch
 *   rac_head_finish_fwd <- nan_to_num of the decoder outputs + box denormalisation, models/racformer_transformer.py:58, models/racformer_head.py:124-131
 *   rac_refine_fwd    <- refine_bbox + velocity scaling + theta_d2xy_coods of the outputs
 *                        models/racformer_transformer.py:230-236,265-269,134
 *   rac_mixing_fwd    <- AdaptiveMixing.inner_forward's matmul / layer_norm / relu chain
 *                        models/racformer_transformer.py:589-603
 *   rac_mixing_bwd    <- autograd of the same chain (the reference checkpoints it: models/racformer_transformer.py:612-616)
 *   rac_sasa_fwd      <- ScaleAdaptiveSelfAttention.inner_forward's mask + attention product
 *                        models/racformer_transformer.py:296-335
 *   rac_sasa_fwd_ex / rac_sasa_bwd <- the same forward saving each row's log-sum-exp, and its backward (autograd of the
 *                        reference's float-mask nn.MultiheadAttention in q, k, v and tau; the distances are no_grad there)
 *   rac_sasa_fwd_mask / rac_sasa_bwd_mask <- the same pair with the boolean [Q,Q] attn_mask of query denoising
 *                        (models/racformer_head.py:220-232, models/racformer_transformer.py:311-312), bit-packed
 *   rac_decode_fwd    <- NMSFreeCoder.decode_single + get_bboxes, models/bbox/coders/nms_free_coder.py:37-88,
 *                        models/racformer_head.py:488-507
 *   rac_outproj_fwd / rac_gemm_split_pack_fwd <- AdaptiveMixing.out_proj (nn.Linear 32768 -> 256), models/racformer_transformer.py:566,606
 *   rac_value_proj_fwd <- BEVSelfAttention.value_proj over the BEV maps, models/bev_self_attention.py:162-174
 *   rac_generator_fwd <- AdaptiveMixing.parameter_generator (nn.Linear 256 -> 65536), models/racformer_transformer.py:565,589
 *   rac_rowgemm_fwd   <- nn.Linear + its preceding add / LayerNorm / ReLU groups, models/racformer_transformer.py:170-177, 243-269
 *   rac_gru_gate_fwd / rac_upsample2x_fwd <- ConvGRUCell.forward's element-wise tail, nn.Upsample
 *                        models/racformer_transformer.py:705-720, :633-636
 *   rac_absmax_fwd / rac_conv_pack_fwd / rac_conv3x3_fwd <- RadarBEVTemporalEncoder.temporal_fusion (nn.Conv2d 3x3)
 *                        models/racformer_transformer.py:631,655
 *   rac_linear_pack_act / rac_linear_pack_wt / rac_generator_ds_fwd / rac_linear_reduce / rac_linear_wgrad <- autograd of
 *     AdaptiveMixing.parameter_generator and out_proj (models/racformer_transformer.py:565-566): forward and data gradients on
 *     rac_generator_fwd's and rac_outproj_fwd's kernels, the weight gradients on a kernel of their own
 *   rac_conv_pack_cl_fwd / rac_conv3x3_wgrad <- autograd of the same convolution: the data gradient is rac_conv3x3_fwd on an
 *                        image of the output gradient with transposed, flipped weights; the weight gradient is a kernel of its own
 *   rac_bev_sampling_fwd <- BEVSampling keypoints + BEVSelfAttention's MSDA + frame fusion, fused
 *                        models/racformer_transformer.py:490-529, models/bev_self_attention.py:176-213
 *   rac_bev_sampling_bwd <- autograd of the same chain (keypoints, MSDA, frame fusion) in one launch
 *   rac_bev_sampling_bwd_batch <- the same for B >= 1, with the frame / batch pairing of models/bev_self_attention.py:162-218
 *   rac_sampling4d_bwd <- autograd of RaCFormerSampling.inner_forward + sampling_4d + msmv op in one launch
 *   rac_regroup_bwd / rac_regroup_multi_bwd <- autograd of the regroup's permute().contiguous(), models/racformer_transformer.py:112-124
 *   rac_refine_bwd    <- autograd of refine_bbox + velocity scaling + theta_d2xy_coods (the ops rac_refine_fwd replaces)
 *   rac_match_cost_fwd <- the cost matrix of PolarHungarianAssigner3D / HungarianAssigner3D.assign
 *                        models/bbox/assigners/polar_hungarian_assigner_3d.py:56-78, models/bbox/match_costs/match_cost.py
 *   rac_lsap_fwd / rac_lsap_host <- scipy.optimize.linear_sum_assignment as the assigners call it (:84)
 *   rac_det_loss_fwd  <- the targets, FocalLoss and L1Loss of loss_single / dn_loss_single with their autograd backwards
 *                        models/racformer_head.py:264-300, 326-427
 *   rac_conv_small_* / rac_depthnet_* <- DepthNet.forward (use_dcn=False), models/necks/view_transformer_racformer.py:329-567
 *   rac_fpn_lateral_fwd / rac_conv3x3_cf_fwd <- the lateral convolutions, top-down merge and output convolutions of the image necks
 *                        (mmdet FPN as img_neck, CustomFPN as img_lss_neck), models/necks/fpn.py:159-180, models/racformer.py:107-126
 *   rac_fpn_merge_bwd / rac_fpn_lateral_dgrad / rac_fpn_lateral_wgrad <- autograd of the same lateral stage (stop_prev_grad=0 trains
 *                        through the necks, models/racformer.py:300)
 *   rac_resnet_stem_fwd / rac_resnet_absmax_fwd / rac_resnet_conv_fwd <- img_backbone, mmdet ResNet(depth=50, style='pytorch',
 *                        norm_eval=True) (configs/racformer_r50_nuimg_704x256_f8.py:67-76, models/racformer.py:107-126) and the
 *                        input normalisation of models/racformer.py:202-212
 *   rac_resnet_conv_dgrad / rac_resnet_conv_wgrad / rac_resnet_relu_bwd <- autograd of the same Bottleneck stages (frozen_stages=1,
 *                        norm_eval=True: the stem and layer1 need no backward, the BatchNorms stay folded)
 *   rac_pillar_train_fwd / rac_pillar_train_bwd / rac_bn_train_* <- extract_pts_feat on frame 0 in training mode under autograd
 *                        (models/racformer.py:316-331): the PFN layer and radar_bev_conv on batch statistics, forward and backward
 *   rac_image_aug_fwd <- the image preparation of extract_feat in a training step: GpuPhotoMetricDistortion, img_norm_cfg, pad_multiple
 *                        and GridMask (models/utils.py:8-45, :104-120, :219-305; models/racformer.py:108-109, :198-224)
 *   rac_adamw_step    <- the optimizer and grad_clip of the training recipe (AdamW through mmcv's optimizer hook,
 *                        configs/racformer_r50_nuimg_704x256_f8.py:282-296): clip_grad_norm_ + torch.optim.AdamW.step
 *   rac_point_maps_radar_fwd / rac_point_maps_lidar_fwd <- RadarPointToMultiViewDepth and PointToMultiViewDepth of the data pipeline
 *                        (loaders/pipelines/loading.py:470-600): the radar_depth / radar_rcs maps and gt_depth from the clouds
 *   rac_image_geom_fwd <- RandomTransformImage of the data pipeline (loaders/pipelines/transforms.py:219-342): Pillow's bicubic
 *                        Image.resize, crop and left-right flip of the raw camera frames
 *   rac_bev_aug_fwd   <- RaCGlobalRotScaleTransImage of the data pipeline (loaders/pipelines/transforms.py:398-464): the rotation about
 *                        z and the isotropic scaling of the lidar cloud, the radar clouds and the ground-truth boxes
 */
#ifndef RACFORMER_HIP_H
#define RACFORMER_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RAC_ABI_VERSION 37
#define RAC_MAX_LEVELS 8
#define RAC_MAX_POINTS 128 /* same limit as the reference, msmv_sampling_forward.cu:21 */

enum { RAC_F32 = 0, RAC_BF16 = 1, RAC_I16 = 2 /* int16 block storage of a BEV value stream: rac_quant_i16_fwd */ };

enum {
    RAC_E_ARG = -1,      /* bad size / null pointer */
    RAC_E_UNSUPPORTED = -2,
};

/* Output layouts of rac_msmv_fwd / rac_msmv_v2_fwd; gradient layouts of rac_msmv_bwd_ex / rac_msmv_v2_bwd_ex. */
enum {
    RAC_OUT_SQCP = 0,  /* [S,Q,C,P]      -- the reference op's layout (msmv_sampling.cpp:170)      */
    RAC_OUT_BQGTPC = 1 /* [B,Q,G,T*P,C]  -- what sampling_4d returns after its regroup
                          (sparsebev_sampling.py:128-131), written directly; slot s=(b*T+t)*G+g */
};

int rac_abi_version(void);
const char *rac_last_error(void);

/* Multi-scale multi-view sampling, forward.
 *   feats[l] : device ptr, [S, N, H_l, W_l, C] channel-last, dtype `dtype`
 *   hw       : HOST ptr, L x (H_l, W_l) int32
 *   loc      : device f32 [S,Q,P,3] = (u, v, view/(N-1)), u,v normalised to [0,1]
 *   w        : device f32 [S,Q,P,L] per-level weights
 *   out      : device f32, layout `out_layout`; every element is written (no pre-zeroing needed)
 *   T,G      : only used by RAC_OUT_BQGTPC (S must be a multiple of T*G); pass 1,1 otherwise
 * out[s,q,c,p] = sum_l w[s,q,p,l] * bilinear0(feats[l][s, round(view*(N-1))], u*(W_l-1), v*(H_l-1)) */
int rac_msmv_fwd(const void *const *feats, const int32_t *hw, int L, const float *loc,
                 const float *w, float *out, int S, int N, int Q, int P, int C, int dtype,
                 int out_layout, int T, int G, void *stream);

/* Feature layouts of rac_msmv_v2_fwd / rac_msmv_v2_bwd. */
enum {
    RAC_FEAT_CL = 0, /* [S,N,H,W,C] channel-last -- the package's pyramid (rac_regroup_fwd), what rac_msmv_fwd takes  */
    RAC_FEAT_CF = 1  /* [S,C,N,H,W] channel-first -- what the reference's torch path hands grid_sample (fp32 only)  */
};

/* Hard-level multi-scale multi-view sampling (msmv_sampling_v2), forward: the level with the largest weight alone.
 *   feats[l] : device ptr, layout `feat_layout`, dtype `dtype` (RAC_BF16: channel-last only)
 *   hw, loc, w, out, T, G: as rac_msmv_fwd (w is only read to pick the level)
 * out[s,q,c,p] = bilinear0(feats[l*][s, round(view*(N-1))], u*(W_l*-1), v*(H_l*-1)), NOT multiplied by the weight, where
 *   l* = argmax_l w[s,q,p,l] as torch.argmax: ties to the first index, a NaN counts as maximal (the first NaN wins),
 *        an all -inf row gives 0.  Only level l*'s four taps are read. */
int rac_msmv_v2_fwd(const void *const *feats, const int32_t *hw, int L, const float *loc, const float *w, float *out,
                    int S, int N, int Q, int P, int C, int dtype, int feat_layout, int out_layout, int T, int G,
                    void *stream);

/* Multi-scale deformable attention, forward (Deformable-DETR semantics, align_corners=False).
 *   value  : device, [bs, keys, heads, dim], dtype `dtype`
 *   shapes : HOST int64 [L,2] (h,w);  starts: HOST int64 [L]
 *   loc    : device f32 [bs,Q,heads,L,P,2] (x,y) in [0,1];  attn: device f32 [bs,Q,heads,L,P]
 *   out    : device f32 [bs,Q,heads*dim] */
int rac_msda_fwd(const void *value, const int64_t *shapes, const int64_t *starts, const float *loc,
                 const float *attn, float *out, int bs, int keys, int heads, int dim, int Q, int L,
                 int P, int dtype, void *stream);

/* Pyramid regroup: in [B, T*N, G*C, H, W] f32 -> out [B*T*G, N, H, W, C] (dtype out_dtype). */
int rac_regroup_fwd(const float *in, void *out, int B, int T, int N, int G, int C, int H, int W,
                    int out_dtype, void *stream);

/* The same regroup for all L levels of the pyramid in ONE launch (16-byte accesses on both sides): ins / outs HOST arrays
 * of L device pointers, hw HOST L x (H, W); C % 4 == 0 and H*W % 4 == 0 on every level. */
int rac_regroup_multi_fwd(int L, const float *const *ins, void *const *outs, const int32_t *hw, int B, int T, int N, int G,
                          int C, int out_dtype, void *stream);

/* Backward of the regroup, the inverse transposition: grad_out [B*T*G, N, H, W, C] f32 -> grad_in [B, T*N, G*C, H, W] f32.
 * A pure permutation: every element of grad_in is written exactly once (no pre-zeroing, no atomics), bit-exact. */
int rac_regroup_bwd(const float *grad_out, float *grad_in, int B, int T, int N, int G, int C, int H, int W, void *stream);

/* The same backward for L levels in ONE launch (16-byte accesses on both sides): grad_outs / grad_ins HOST arrays of L device
 * pointers, hw HOST L x (H, W); C % 4 == 0 and H*W % 4 == 0 on every level.  The caller lists only the levels that need a
 * gradient. */
int rac_regroup_multi_bwd(int L, const float *const *grad_outs, float *const *grad_ins, const int32_t *hw, int B, int T, int N,
                          int G, int C, void *stream);

/* Per-query box constants shared by the fused sampling kernels: table[b,q] = (cx, cy, cz, w, l, h,
 * cos yaw, sin yaw) = decode_bbox(theta_d2xy_coods(query_bbox)) (models/bbox/utils.py:66-90), once per
 * query and layer instead of once per keypoint.  query_bbox device f32 [n,10], table device f32 [n,8]. */
int rac_box_prep_fwd(const float *query_bbox, float *table, int num_boxes, const float *pc_range, void *stream);

/* Adaptive 4D sampling of one decoder layer, fully fused (keypoints -> projection -> first-valid-view
 * -> multi-scale gather).  Replaces RaCFormerSampling.inner_forward + sampling_4d + the msmv op
 * (models/racformer_transformer.py:361-419, models/sparsebev_sampling.py:28-134).
 *   feats[l]     : device [B*T*G, N, H_l, W_l, 64] (dtype), hw HOST L x (H,W)
 *   query_bbox   : device f32 [B,Q,10] polar boxes (theta, d, z, log w, log l, log h, sin, cos, vx, vy)
 *   box_table    : device f32 [B,Q,8] written by rac_box_prep_fwd for the same boxes
 *   offsets      : device f32, row (b,q) at offsets + (b*Q+q)*ld_off, G*NP*D*3 values (sampling_offset Linear)
 *   ray_logits   : device f32, rows of D values, stride ld_ray          (ray_points_offset Linear)
 *   scale_logits : device f32, rows of G*T*NP*D*L values, stride ld_scale (scale_weights Linear, softmax over L here)
 *   time_diff    : device f32 [B,T];  lidar2img: device f32 [B,T*N,4,4]
 *   out          : device f32 [B,Q,G,T*NP*D,64]
 *   loc_out,w_out: optional debug outputs [S,Q,P,3] (u,v,view/(N-1)) and [S,Q,P,L] (NULL,NULL to skip)
 *   view_in      : optional device u8 [S,Q,P]: the camera index to sample each point in, INSTEAD of the first valid view
 *                  (sparsebev_sampling.py:97-110).  NULL on the product path; parity tests pass the reference's own
 *                  choices to take the path's one discontinuous step out of a comparison.  loc_out then still reports
 *                  the kernel's OWN choice in its third component (and the imposed view's u, v).
 *   pc_range (6), depth_base (D = torch.linspace(-d_region,d_region,D)): HOST pointers
 *   limits       : NP*D <= 128 points per (slot, query); the kernel takes 8 queries per workgroup, fewer where their tap table
 *                  (queries * NP*D * L * 32 bytes) would exceed 64 KB of LDS (NP*D = 64, L = 4: four); 64 channels per group
 *   compact      : 1 = the variant that sets points without any tap aside (rigs that do not cover the full circle), 0 = plain,
 *                  -1 = decide by the number of cameras (<= 3).  Same results either way. */
int rac_sampling4d_fwd(const void *const *feats, const int32_t *hw, int L, const float *query_bbox,
                       const float *box_table, const float *offsets, const float *ray_logits, const float *scale_logits,
                       const float *time_diff, const float *lidar2img, float *out, float *loc_out,
                       float *w_out, const unsigned char *view_in, int ld_off, int ld_ray, int ld_scale, int B, int T, int N,
                       int G, int Q,
                       int NP, int D, int C, const float *pc_range, const float *depth_base, float d_region,
                       float image_h, float image_w, float eps, int dtype, int compact, void *stream);

/* Backward of rac_sampling4d_fwd in one launch: float32 features, 64 channels per group.  Nothing of the forward is saved:
 * location, camera choice, level weights and bilinear taps are recomputed from the forward's inputs with the forward's own
 * device functions (the same bits).  Inputs as rac_sampling4d_fwd (the same pointers, row strides and host arrays, view_in
 * included), plus
 *   grad_out     : device f32 [B,Q,G,T*NP*D,64]
 * Outputs, all device f32:
 *   grad_feats[l]: HOST array of L device pointers, each of the shape of feats[l], ZERO-FILLED BY THE CALLER; float atomics
 *                  (sums in arrival order).  NULL array: no feature gradient wanted, the scatter is skipped.
 *   grad_offsets : rows of G*NP*D*3 (stride gld_off);  grad_ray: rows of D (gld_ray);
 *   grad_scale   : rows of G*T*NP*D*L (gld_scale): gradient of the LOGITS (softmax backward over L), written at the (g', t')
 *                  slot the forward reads a keypoint's weights from (sparsebev_sampling.py:113-120; a bijection)
 *                  -- the three may be column slices of one gradient of a fused Linear output
 *   grad_box     : [B,Q,8] gradient of all eight box-table entries (z, h and the rotation act through the projection)
 *   grad_loc_out, grad_w_out : optional debug outputs [S,Q,P,2] / [S,Q,P,L] (NULL to skip): per keypoint the gradient of its
 *                  image location (u, v) and of its softmaxed level weights, before the chain tail
 *   loc_out, w_out : optional debug outputs [S,Q,P,3] / [S,Q,P,L] (NULL, NULL to skip): the keypoints as THIS kernel recomputed
 *                  them, in the forward's loc_out / w_out format (bit-equal to the forward's)
 * Every element of every output except grad_feats has one writer and a fixed summation order (bit-reproducible).  homo passes
 * the gradient where homo > eps; the two clamps to [0,1] inside [0,1] inclusive; a point no camera sees is sampled (and
 * differentiated) in camera 0, as in the reference; velocity, time_diff and lidar2img get no gradient.  Refused before any
 * launch: dtype other than RAC_F32, C != 64, L outside {1, 2, 4, 5}, NP*D > 128, T*G*NP*D keypoints per query beyond the 64 KB
 * LDS staging ((5 + 2 L) floats each). */
int rac_sampling4d_bwd(const void *const *feats, const int32_t *hw, int L, const float *query_bbox,
                       const float *box_table, const float *offsets, const float *ray_logits,
                       const float *scale_logits, const float *time_diff, const float *lidar2img,
                       const unsigned char *view_in, const float *grad_out, void *const *grad_feats,
                       float *grad_offsets, float *grad_ray, float *grad_scale, float *grad_box, float *grad_loc_out,
                       float *grad_w_out, float *loc_out, float *w_out, int ld_off, int ld_ray, int ld_scale,
                       int gld_off, int gld_ray, int gld_scale, int B, int T, int N, int G, int Q, int NP, int D, int C,
                       const float *pc_range, const float *depth_base, float d_region, float image_h, float image_w,
                       float eps, int dtype, void *stream);

/* BEV deformable cross-attention of one decoder layer, fully fused (keypoints -> per-frame
 * deformable attention -> softmax-over-frames fusion).  Replaces BEVSampling.inner_forward's keypoint
 * chain, the MSDA op and the frame fusion (models/racformer_transformer.py:490-529,
 * models/bev_self_attention.py:176-213); output_proj + identity stay outside.
 *   value        : device [B*T, H*W, heads, 64] (dtype) -- hoisted value_proj(bev + pos)
 *   offsets      : rows of heads*NP*D*2 values (stride ld_off); ray_logits rows of D (ld_ray);
 *   scale_logits : rows of heads*NP*D (ld_scale, softmax over the NP*D points of a head here);
 *   queue_logits : rows of T (ld_queue, softmax over frames here)
 *   out          : device f32 [B,Q,heads*64];  loc_out: optional [B,Q,heads,T,NP*D,2] or NULL */
int rac_bev_sampling_fwd(const void *value, const float *query_bbox, const float *box_table, const float *offsets,
                         const float *ray_logits, const float *scale_logits, const float *queue_logits,
                         const float *time_diff, float *out, float *loc_out, int ld_off, int ld_ray,
                         int ld_scale, int ld_queue, int B, int T, int Q, int heads, int NP, int D, int H, int W,
                         int dim, const float *pc_range, const float *depth_base, float d_region, int dtype,
                         void *stream);

/* Backward of rac_bev_sampling_fwd in one launch: float32 value stream, B == 1, 64 channels per head.  Nothing of the forward
 * is saved: keypoints, softmaxes and bilinear footprints are recomputed from the forward's inputs with the forward's own
 * device functions.  Inputs as rac_bev_sampling_fwd (the same pointers and row strides), plus
 *   grad_out     : device f32 [B,Q,heads*64]
 * Outputs, all device f32:
 *   grad_value   : [B*T, H*W, heads, 64], ZERO-FILLED BY THE CALLER; float atomics (sums in arrival order)
 *   grad_offsets : rows of heads*NP*D*2 (stride gld_off);  grad_ray: rows of D (gld_ray);
 *   grad_scale   : rows of heads*NP*D (gld_scale): gradient of the LOGITS (softmax backward over the points of a head);
 *   grad_queue   : rows of T (gld_queue): gradient of the frame logits (softmax backward over T)
 *                  -- the four may be column slices of one gradient of a fused Linear output
 *   grad_box     : [B,Q,8] gradient of the box-table entries the forward reads (0, 1, 3, 4, 6, 7; 2 and 5 are written as 0)
 *   grad_loc_out, grad_attn_out : optional debug outputs [B,Q,heads,T,NP*D,2] / [B,Q,heads,T,NP*D] (NULL, NULL to skip): per
 *                  keypoint the gradient of its location (x, y in [0,1], its weight included) and of its combined weight
 *                  softmax_P * softmax_T, before the chain tail -- the counterpart of the forward's loc_out
 * Every element of every output except grad_value has one writer and a fixed summation order (bit-reproducible).  The clamp
 * to [0,1] passes the gradient inside [0,1] inclusive; a keypoint outside the map contributes nothing; velocity and
 * time_diff get no gradient.  A non-finite logit reaches grad_value at the pixels its keypoints tap, as in autograd; a
 * non-finite box row samples nothing.  Refused before any launch: dtype other than RAC_F32, B > 1, T or NP*D above 64,
 * heads*T*NP*D keypoints per query beyond the 64 KB LDS staging (about 2,600). */
int rac_bev_sampling_bwd(const void *value, const float *query_bbox, const float *box_table, const float *offsets,
                         const float *ray_logits, const float *scale_logits, const float *queue_logits,
                         const float *time_diff, const float *grad_out, float *grad_value, float *grad_offsets,
                         float *grad_ray, float *grad_scale, float *grad_queue, float *grad_box, float *grad_loc_out,
                         float *grad_attn_out, int ld_off, int ld_ray, int ld_scale, int ld_queue, int gld_off,
                         int gld_ray, int gld_scale, int gld_queue, int B, int T, int Q, int heads, int NP, int D, int H,
                         int W, int dim, const float *pc_range, const float *depth_base, float d_region, int dtype,
                         void *stream);

/* rac_bev_sampling_bwd for batches: the same arguments and outputs, any B >= 1 (B = 0 is refused), float32 values, dim == 64.
 * (One kernel source serves both: here B is read at run time, rac_bev_sampling_bwd's instantiation fixes it at 1.)
 * For B > 1 the forward pairs row r = 0 .. B*T-1 of the value frames -- frame and output slot (b_o, t_o) = (r / T, r % T), whose
 * frame weight and grad_out row it takes -- with the keypoints and point weights of (b_l, t_l) = (r % B, r / B)
 * (models/bev_self_attention.py:162-218); the gradients of (b_l, q)'s offsets, ray and scale logits and box table collect terms
 * from several output rows, and the softmax-over-T backward of (b_o, q) the rows of several b_l.  One workgroup takes query
 * index q of all B samples, so every output except grad_value keeps one writer and a fixed summation order.  time_diff is
 * [B,T]; the optional debug outputs are indexed by the output slot, as the forward's loc_out.  At B == 1 every output except
 * grad_value equals rac_bev_sampling_bwd's bit for bit.  Refused before any launch: what rac_bev_sampling_bwd refuses except
 * B > 1, and B * (heads*T*NP*D) keypoints per query index beyond the 160 KB LDS of a workgroup (about 19 KB per sample at
 * heads 4, T 8, NP*D 20). */
int rac_bev_sampling_bwd_batch(const void *value, const float *query_bbox, const float *box_table, const float *offsets,
                               const float *ray_logits, const float *scale_logits, const float *queue_logits,
                               const float *time_diff, const float *grad_out, float *grad_value, float *grad_offsets,
                               float *grad_ray, float *grad_scale, float *grad_queue, float *grad_box, float *grad_loc_out,
                               float *grad_attn_out, int ld_off, int ld_ray, int ld_scale, int ld_queue, int gld_off,
                               int gld_ray, int gld_scale, int gld_queue, int B, int T, int Q, int heads, int NP, int D, int H,
                               int W, int dim, const float *pc_range, const float *depth_base, float d_region, int dtype,
                               void *stream);

/* The same kernel for the BEV streams of one decoder layer (radar, LSS) in ONE launch: same queries, boxes and time_diff,
 * per stream its own value maps, Linear outputs (same row strides) and output.  HOST arrays of nstreams (1..2) device
 * pointers.  The second stream's workgroups start as the first one's drain and its keypoint prologue runs under the first
 * stream's gathers (models/racformer_transformer.py:246-249 runs the two modules back to back). */
int rac_bev_sampling_multi_fwd(int nstreams, const void *const *values, const float *const *offsets,
                               const float *const *ray_logits, const float *const *scale_logits,
                               const float *const *queue_logits, float *const *outs, const float *query_bbox,
                               const float *box_table, const float *time_diff, int ld_off, int ld_ray, int ld_scale,
                               int ld_queue, int B, int T, int Q, int heads, int NP, int D, int H, int W, int dim,
                               const float *pc_range, const float *depth_base, float d_region, int dtype, void *stream);

/* Opt-in 16-bit BLOCK storage of a hoisted BEV value stream (round 4; the default keeps fp32): values [blocks][64] f32 -- one
 * block = the 64 channels of one head at one pixel of one frame, i.e. the unit one tap of the BEV kernel reads -- become int16
 * mantissas q [blocks][64] and one power-of-two scale per block, value = q * scale[block] (14-15 significant bits relative to
 * the block's largest value).  Not a reference interface: the reference keeps fp32 value maps (bev_self_attention.py:162-174);
 * this is the storage format of rac_bev_sampling_multi_q16_fwd below. */
int rac_quant_i16_fwd(const float *values, void *q, float *scale, int64_t blocks, void *stream);

/* rac_bev_sampling_multi_fwd over int16 block-stored value streams: values[i] int16 [B*T, H*W, heads, 64], value_scales[i] f32
 * [B*T, H*W, heads] from rac_quant_i16_fwd; everything else as above (same arithmetic in fp32; each tap's scale is folded into
 * its bilinear weight).  Halves the bytes the kernel gathers. */
int rac_bev_sampling_multi_q16_fwd(int nstreams, const void *const *values, const float *const *value_scales,
                                   const float *const *offsets, const float *const *ray_logits,
                                   const float *const *scale_logits, const float *const *queue_logits, float *const *outs,
                                   const float *query_bbox, const float *box_table, const float *time_diff, int ld_off,
                                   int ld_ray, int ld_scale, int ld_queue, int B, int T, int Q, int heads, int NP, int D,
                                   int H, int W, int dim, const float *pc_range, const float *depth_base, float d_region,
                                   void *stream);

/* Scale-adaptive self-attention core (QK^T + distance mask + softmax + AV), one kernel.
 * Replaces calc_bbox_dists, the [B*heads,Q,Q] mask and nn.MultiheadAttention's attention product
 * (models/racformer_transformer.py:296-335); in_proj / out_proj remain library GEMMs.
 *   qkv : device f32, token row (b,q) at qkv + (b*Q+q)*ld_qkv holding q|k|v, each [heads, dim]
 *   tau : device f32, rows of `heads` values, stride ld_tau (gen_tau Linear output)
 *   box_table : optional device f32 [B,Q,8] from rac_box_prep_fwd for the same boxes (NULL: centres computed here)
 *   out : device f32 [B,Q,heads*dim];  pc_range: HOST (6).  dim must be 32.  Q <= 1024: QK^T and PV run on
 *   v_mfma_f32_16x16x4_f32 (exact fp32); larger Q: an LDS-tiled fp32 VALU kernel. */
int rac_sasa_fwd(const float *qkv, const float *tau, const float *query_bbox, const float *box_table, float *out,
                 int ld_qkv, int ld_tau, int B, int Q, int heads, int dim, const float *pc_range, void *stream);

/* rac_sasa_fwd that also writes lse : device f32 [B,heads,Q], the log-sum-exp m + log(l) of every query row's logits
 * (NULL: nothing more is written).  `out` is bit-identical to rac_sasa_fwd's with or without lse. */
int rac_sasa_fwd_ex(const float *qkv, const float *tau, const float *query_bbox, const float *box_table, float *out,
                    float *lse, int ld_qkv, int ld_tau, int B, int Q, int heads, int dim, const float *pc_range, void *stream);

/* Backward of rac_sasa_fwd in qkv and tau (none for query_bbox: the reference forms the distances under no_grad).
 * qkv, tau, query_bbox, box_table, pc_range, B, Q, heads, dim: as given to rac_sasa_fwd_ex; out [B,Q,heads*dim] and
 * lse [B,heads,Q]: what it wrote; grad_out: device f32 [B,Q,heads*dim] (contiguous).
 *   grad_qkv : device f32, token row (b,q) at grad_qkv + (b*Q+q)*ld_grad_qkv receiving dq|dk|dv ([heads, dim] each; even ld)
 *   grad_tau : device f32, token row at grad_tau + (b*Q+q)*ld_grad_tau receiving the `heads` values of dtau
 * The two may be column slices of one [B,Q,3*heads*dim+heads] buffer (the gradient of the in_proj + gen_tau GEMM output).
 * Every element of the two is written once (no accumulation, no atomics: bit-reproducible); S is recomputed from lse,
 * nothing of size Q x Q is stored.  dim must be 32, Q <= 6144.  No host synchronisation, no allocation. */
int rac_sasa_bwd(const float *qkv, const float *tau, const float *query_bbox, const float *box_table, const float *out,
                 const float *lse, const float *grad_out, float *grad_qkv, float *grad_tau, int ld_qkv, int ld_tau,
                 int ld_grad_qkv, int ld_grad_tau, int B, int Q, int heads, int dim, const float *pc_range, void *stream);

/* rac_sasa_fwd_ex / rac_sasa_bwd under a boolean attention mask shared by all batches and heads (the reference's
 * pre_attn_mask: mask[:, :, attn_mask] = -inf, models/racformer_transformer.py:311-312).  All other arguments as above.
 *   mask_bits : device uint32 words [Q][ld_mask], ld_mask >= ceil(Q/32): bit (j & 31) of word [i][j >> 5] set = query i
 *               does not attend to key j.  Bits at j >= Q are ignored.
 * A blocked pair has logit -inf: probability exactly 0 and exactly 0 in dq, dk, dv and dtau; lse is over the allowed keys.
 * Forward: Q <= 1024 the register-resident matrix-core kernel of rac_sasa_fwd_ex (with an all-zero mask, out and lse are
 * bit-identical to it); larger Q (up to 6144) a streaming matrix-core kernel with online softmax -- box_table is honoured at
 * every Q.  Backward: the two-role kernel of rac_sasa_bwd with the mask in both roles, one writer per element, no atomics
 * (bit-reproducible; with an all-zero mask bit-identical to rac_sasa_bwd where the two read the same centres).  A 16 x 16 tile
 * without an allowed pair is skipped whole (no loads, no MFMAs); the results do not depend on that.  Nothing of size Q x Q
 * beyond the Q*ld_mask mask words is read or written.
 * A query row with every key blocked has no softmax: its out row and the gradients it would contribute to are unspecified
 * (NaN where the tile is computed) and its lse is -inf or NaN.  The query-denoising layout has no such row. */
int rac_sasa_fwd_mask(const float *qkv, const float *tau, const float *query_bbox, const float *box_table, float *out,
                      float *lse, int ld_qkv, int ld_tau, int B, int Q, int heads, int dim, const float *pc_range, void *stream,
                      const uint32_t *mask_bits, int ld_mask);

int rac_sasa_bwd_mask(const float *qkv, const float *tau, const float *query_bbox, const float *box_table, const float *out,
                      const float *lse, const float *grad_out, float *grad_qkv, float *grad_tau, int ld_qkv, int ld_tau,
                      int ld_grad_qkv, int ld_grad_tau, int B, int Q, int heads, int dim, const float *pc_range, void *stream,
                      const uint32_t *mask_bits, int ld_mask);

/* Layouts of the f16 hi / lo activation images that rac_add_ln_fwd and rac_rowgemm_fwd can emit beside their fp32 rows */
enum {
    RAC_SPLIT_KCAT = 0,    /* rows [hi dim | hi dim | lo dim | pad]: A operand of a K-concatenated library GEMM */
    RAC_SPLIT_LINES = 1    /* rows [dim/32 lines][hi 32 | lo 32]: X image of rac_generator_fwd (dim = 256: 1 KB per row) */
};

/* Row-wise  out = [relu]( LayerNorm( a_scale * sum_{s<num_partials} a[s] + residual + bias ) * gamma + beta ) [+ post_residual].
 * Replaces the add / bias / split-K reduce + nn.LayerNorm (+ ReLU) (+ add) launch groups of the decoder layer
 * (models/racformer_transformer.py:170-177, 199-205, 243-258).  a: device f32, row r of partial s at
 * a + s*partial_stride + r*ld_a; residual / post_residual [rows][dim], bias [dim]: optional (NULL); out row r at
 * out + r*ld_out (so results can land in a column slice of a wider buffer); dim % 4 == 0, <= 1024.
 * split_out (optional, NULL to skip): device f16 [rows][3*dim + split_pad] = [hi | hi | lo | pad] with
 * out*split_scale = hi + lo -- the K-concatenated A operand of a 3-product split GEMM (hi*Whi + hi*Wlo + lo*Whi,
 * fp32 accumulate) on the f16 matrix cores, for the Linear layers that consume this row (split_scale: a power of
 * two).  split_layout = RAC_SPLIT_LINES instead writes the line image [rows][dim/32][hi 32 | lo 32] (split_pad 0).
 * split_pad (0 or a multiple of 4) extra columns: the first two hold split_scale (the activation 1.0, which
 * meets [bias_hi | bias_lo] in the weight image, so the GEMM adds the bias itself), the others 0. */
int rac_add_ln_fwd(const float *a, int num_partials, int64_t partial_stride, int ld_a, float a_scale, const float *residual,
                   const float *bias, const float *gamma, const float *beta, const float *post_residual,
                   float *out, int ld_out, int rows, int dim, float eps, int relu, void *split_out,
                   float split_scale, int split_pad, int split_layout, void *stream);

/* The element-wise tail of the head over the stacked decoder outputs, one launch: cls <- nan_to_num(cls) in place
 * (RaCFormerTransformer.forward, models/racformer_transformer.py:58) and box <- nan_to_num(xy) with the centre scaled to
 * metres and the columns reordered to (x, y, w, l, z, h, sin, cos, vx, vy) (RaCFormer_head.forward,
 * models/racformer_head.py:124-131).  cls: device f32 [n_cls]; xy, box: device f32 [rows][10], distinct buffers;
 * pc_range: HOST float[6]. */
int rac_head_finish_fwd(float *cls, int64_t n_cls, const float *xy, float *box, int64_t rows, int code_size,
                        const float *pc_range, void *stream);

/* Position-encoder head  out = relu(LayerNorm(W x + b))  for the 3-wide box input
 * (models/racformer_transformer.py:170-173); x row r at x + r*ld_x (3 values), weight [256,3], out [rows,256]. */
int rac_pe_head_fwd(const float *x, int ld_x, const float *weight, const float *bias, const float *gamma,
                    const float *beta, float *out, int rows, int dim, float eps, void *stream);

/* Box refinement tail of a decoder layer: refine_bbox + velocity / time_diff + theta_d2xy of the emitted
 * boxes (models/racformer_transformer.py:230-236, :265-269, :134; models/bbox/utils.py:82-90).
 *   proposal [B*Q,10] (this layer's input boxes), delta [B*Q,10] (reg_branch output),
 *   time_diff_safe [B,T] (time_diff with values < 1e-5 replaced by 1)  ->
 *   bbox_pred [B*Q,10] (polar, next layer's input), bbox_xy [B*Q,10] (normalised xy, the layer's output). */
int rac_refine_fwd(const float *proposal, const float *delta, const float *time_diff_safe, float *bbox_pred,
                   float *bbox_xy, int B, int Q, int T, float num_ray, void *stream);

/* Backward of rac_refine_fwd, closed form, the forward quantities recomputed from its inputs:
 *   grad_pred [B*Q,10], grad_xy [B*Q,10] (gradients of bbox_pred / bbox_xy; either may be NULL = absent, it is then not read)  ->
 *   grad_delta [B*Q,10], grad_proposal [B*Q,10] (every element written; components 3..9 of grad_proposal are zero).
 * Gates as torch's autograd of the reference's ops: clamp passes the gradient on the closed interval and blocks it outside
 * (the [0,1] clamp of theta_d2xy_coods and of inverse_sigmoid); inverse_sigmoid's clamp(min=eps) of x and of 1-x each gate their
 * own factor; the velocity division by time_diff_safe[:,1] applies only when T > 1; theta receives gradient from bbox_pred[0]
 * and, through cos / sin, from bbox_xy[0:2]. */
int rac_refine_bwd(const float *proposal, const float *delta, const float *time_diff_safe, const float *grad_pred,
                   const float *grad_xy, float *grad_delta, float *grad_proposal, int B, int Q, int T, float num_ray,
                   void *stream);

/* Boundary between two decoder layers in one launch: rac_refine_fwd for the finished layer and, for the boxes it produces,
 * the first two launches of the next layer -- rac_box_prep_fwd (box_table [B*Q,8]) and rac_pe_head_fwd (pe_out [B*Q,256]
 * = relu(LayerNorm(pe_weight (theta,d,z) + pe_bias))).  Same arithmetic as the three separate entry points. */
int rac_layer_boundary_fwd(const float *proposal, const float *delta, const float *time_diff_safe, float *bbox_pred,
                           float *bbox_xy, float *box_table, const float *pc_range, const float *pe_weight,
                           const float *pe_bias, const float *pe_gamma, const float *pe_beta, float *pe_out, int B, int Q,
                           int T, int dim, float num_ray, float eps, void *stream);

/* Matrix-core arithmetic of rac_mixing_fwd. */
enum {
    RAC_MIX_F32 = 0,   /* v_mfma_f32_16x16x4_f32: f32 in, f32 accumulate (bit-for-bit an fmaf chain) */
    RAC_MIX_F16X3 = 1  /* 16-bit matrix cores on split operands, f32 accumulate, fp32-GEMM accuracy: x @ M as three
                          bf16 terms each (6 products, truncation 2^-23, any fp32 magnitude), S @ Y as two f16 terms
                          each (3 products, truncation 2^-22; needs |S * param_scale| < 6e4) */
};

/* AdaptiveMixing core on the matrix cores: per (query, group) item
 *   Y = relu(LN_{[P,64]}(x @ M)),  Z = relu(LN_{[128,64]}(S @ Y))
 * Replaces the two batched matmuls, two layer norms and two ReLUs of AdaptiveMixing.inner_forward
 * (models/racformer_transformer.py:589-603); out_proj consumes its output image through rac_outproj_fwd.
 *   x      : device f32 [num_query, groups, in_points, 64]    (sampled features, B folded into num_query)
 *   params : device f32, row q at params + q*ld_params, per group [64*64 (M, in x out) | 128*in_points (S)];
 *            every value is multiplied by param_scale on load (1.0, or the power-of-two alpha of a split GEMM)
 *   out    : device f32 [num_query, groups, 128, 64] (NULL to skip when out_split is given)
 *   out_split : optional device f16 line image [num_query][groups*256][hi 32 | lo 32] of the flattened output row
 *            (K order group, out point, channel) with out*split_scale = hi + lo -- the A operand of rac_outproj_fwd
 *            (NULL to skip) */
int rac_mixing_fwd(const float *x, const float *params, float param_scale, float *out, void *out_split,
                   float split_scale, int ld_params, int num_query, int groups, int in_points, int channels, int out_points,
                   float eps, int mfma_mode, void *stream);

/* rac_mixing_fwd with a parameter row period: item row q reads the parameter row at params + (q % period)*ld_params.  For
 * item rows whose parameters repeat -- B batch elements generated from the same queries -- the parameter block is held
 * once ([period] rows) instead of B times.  period divides num_query; period == num_query is rac_mixing_fwd, address for
 * address.  Every other argument as for rac_mixing_fwd. */
int rac_mixing_period_fwd(const float *x, const float *params, float param_scale, float *out, void *out_split,
                          float split_scale, int ld_params, int period, int num_query, int groups, int in_points, int channels,
                          int out_points, float eps, int mfma_mode, void *stream);

/* Backward of rac_mixing_fwd in RAC_MIX_F32 mode with param_scale 1 (the training forward): given dZ, the gradients in x and
 * in the generated parameters.  x, params, ld_params, num_query, groups, in_points, channels, out_points, eps: as given to
 * rac_mixing_fwd (channels 64, out_points 128, in_points 1..96; ld_params a multiple of 4).
 *   grad_out    : device f32 [num_query, groups, 128, 64] (contiguous), dZ
 *   grad_x      : device f32 [num_query, groups, in_points, 64] receiving dx
 *   grad_params : device f32, row q at grad_params + q*ld_grad_params, laid out as params: per group [dM 64*64 | dS 128*in_points];
 *                 every one of a row's groups*(64*64+128*in_points) columns is written (ld_grad_params >= that width)
 *   z_out       : optional device f32 [num_query, groups, 128, 64] receiving the recomputed Z (NULL: not written); bit for bit
 *                 rac_mixing_fwd's RAC_MIX_F32 output
 * One workgroup per item recomputes the forward with its own arithmetic (so the ReLU masks are the forward's) and forms
 *   g2 = dZ [B^ > 0],  dB = r2 (g2 - mean g2 - B^ mean(g2 B^)),  dS = dB Y^T,  dY = S^T dB,
 *   g1 = dY [A^ > 0],  dA = r1 (g1 - mean g1 - A^ mean(g1 A^)),  dM = x^T dA, dx = dA M^T
 * (A = x M, A^ = LN(A), B = S Y, B^ = LN(B); means over the P*64 / 128*64 elements).  Every output element has one writer (no
 * accumulation, no atomics: bit-reproducible).  No host synchronisation, no allocation. */
int rac_mixing_bwd(const float *x, const float *params, int ld_params, const float *grad_out, float *grad_x, float *grad_params,
                   int ld_grad_params, float *z_out, int num_query, int groups, int in_points, int channels, int out_points,
                   float eps, void *stream);

/* Split-precision GEMM operand image: nn.Linear weight [N][K] f32 -> f16 [N][K/32][hi 32 | lo 32] of weight * scale
 * (per 32 values of K one 128-byte line; hi + lo carry 22 significant bits).  Packed once per set of weights. */
int rac_gemm_split_pack_fwd(const float *weight, void *image, int N, int K, float scale, void *stream);

/* AdaptiveMixing.out_proj (nn.Linear(groups*128*64 -> 256), models/racformer_transformer.py:566,606) as a hand-written
 * split-K GEMM on the f16 matrix cores at fp32-GEMM accuracy (three products hi*hi + hi*lo + lo*hi, fp32 accumulate):
 *   partials[s][m][n] = sum_{k in slice s} Z[m][k] * W[n][k]        (unscaled: the consumer applies both powers of two)
 *   z_image : device f16 line image [M][K/32][hi 32 | lo 32]   (rac_mixing_fwd's out_split)
 *   w_image : device f16 line image [N][K/32][hi 32 | lo 32]   (rac_gemm_split_pack_fwd)
 *   partials: device f32 [slices][M][N];  K % (32 * slices) == 0 (N % 4 == 0 gives aligned 16-byte stores; other N work through
 *             unaligned stores, slower).  rac_add_ln_fwd sums the slices. */
int rac_outproj_fwd(const void *z_image, const void *w_image, float *partials, int M, int N, int K, int slices, void *stream);

/* AdaptiveMixing.parameter_generator (nn.Linear(256 -> groups*(64*64 + 128*in_points)), models/racformer_transformer.py:565,589)
 * on the same hand-written kernel:  out[m][n] = alpha * sum_k X[m][k] * W[n][k] + bias[n]   (alpha undoes the two powers of two
 * of the images).  One workgroup per 256 features walks all rows: the weights cross the fabric once.  Also the eleven Linears
 * of the three sampling modules (256 -> 2189, models/racformer_transformer.py:361-366, 490-500): for narrow outputs the rows
 * are cut into chunks so that feature blocks x chunks covers the CUs.
 *   x_image : device f16 line image [M][K/32][hi 32 | lo 32]   (rac_rowgemm_fwd's split_out, split_layout = RAC_SPLIT_LINES)
 *   w_image : device f16 line image [N][K/32][hi 32 | lo 32]   (rac_gemm_split_pack_fwd);  bias device f32 [N] or NULL
 *   out     : device f32, row m at out + m*ld_out;  K % 32 == 0, ld_out % 4 == 0, N % 4 == 0 unless K == 256 */
int rac_generator_fwd(const void *x_image, const void *w_image, const float *bias, float alpha, float *out, int64_t ld_out, int M,
                      int N, int K, void *stream);

/* BEVSelfAttention.value_proj over a whole BEV stream (nn.Linear(256 -> 256) on every pixel of every frame,
 * models/bev_self_attention.py:162-174) read straight from the channel-first maps:
 *     out[f*HW + p][n] = sum_c x[f][c][p] * W[n][c] + add[p][n]        (add NULL: + bias[n], bias NULL: nothing)
 *   x       : device f32 [frames][256][HW] (the reference's [B*T, C, H, W]);  HW % 32 == 0
 *   w_image : device f16 line image [256][8][hi 32 | lo 32] (rac_gemm_split_pack_fwd with scale 2^s); w_alpha = 2^-s
 *   add     : device f32 [HW][256] -- the frame-independent term value_proj(pos) + bias -- or NULL;  bias: device f32 [256] or NULL
 *   out     : device f32 [frames*HW][256] (= [B*T, H*W, heads, 64], the value operand of rac_bev_sampling_fwd)
 * Split-precision f16 MFMA (hi / lo per operand, fp32 accumulate), activation scale per pixel.  16-byte aligned pointers. */
int rac_value_proj_fwd(const float *x, const void *w_image, float w_alpha, const float *add, const float *bias, float *out,
                       int frames, int channels, int HW, int features, void *stream);
/* rac_value_proj_fwd writing the int16 block storage of rac_quant_i16_fwd (q [frames*HW][256] int16, scale [frames*HW][4] f32):
 * bit for bit rac_quant_i16_fwd(rac_value_proj_fwd(...)); the LSS BEV value stream of rac_bev_sampling_multi_q16_fwd. */
int rac_value_proj_q16_fwd(const float *x, const void *w_image, float w_alpha, const float *add, const float *bias, void *q,
                           float *scale, int frames, int channels, int HW, int features, void *stream);

/* The temporal-fusion convolution of RadarBEVTemporalEncoder (3x3, stride 1, pad 1, Cin -> 256; the 193-GFLOP
 * nn.Conv2d of models/racformer_transformer.py:631,655) as an implicit GEMM on the f16 matrix cores with
 * hi/lo-split operands (3 products, fp32 accumulate: fp32-convolution accuracy).  Three calls:
 *   rac_absmax_fwd    amax_out[0] = max(floor_value, max |v| over `num` device arrays) (srcs / counts: HOST arrays;
 *                     16-byte aligned sources); a one-thread launch sets amax_out to floor_value first.  Fixes the activations'
 *                     power-of-two scale; floor_value >= 0 covers sources whose bound is known without reading them.
 *   rac_conv_pack_fwd src [N,C,H,W] f32 -> channel range [c_offset, c_offset+C) of the kernel's activation image
 *                     xs = f16 [N][H+2][W+2][c_total/32][2][32] (per pixel and 32-channel chunk: hi, then lo, of
 *                     v * 2^e; e from *amax).  Only interior pixels are written: the caller zeroes xs once (border =
 *                     the convolution's zero padding).  Any H, W (16-byte loads when W % 4 == 0); channel counts multiples of 32.
 *   rac_conv3x3_fwd   out [N,H,W,256] f32 (channel-last) = conv3x3(xs) * w_alpha / 2^e + bias[c] (or + pixel_bias[h*W+w][c]
 *                     if pixel_bias != NULL: a per-pixel additive map shared by the N images), with
 *                     ws = f16 [9 taps (ky*3+kx)][Cin/32][256][2][32] holding hi / lo of weight[co][ci][ky][kx] / w_alpha
 *                     (w_alpha a power of two chosen by the packer).  Any H*W (tiles of 256 pixels, the last one of an image
 *                     ragged); a pixel_bias map needs H*W to be a multiple of 256. */
/* rac_conv3x3_relu_cf_fwd: the same kernel with another epilogue: out [N][256][H*W] f32 CHANNEL-FIRST = relu(conv3x3(xs) + bias[c])
 * -- Conv2d(3x3, pad 1, bias=False) + BatchNorm2d (folded into ws and bias by the host) + ReLU, the last ConvModule of radar_bev_conv
 * (models/racformer.py:81-99).  The image's scale is act_scale(scale_mul * (*amax) + scale_add) as in rac_cd_scale (amax: device
 * word or NULL), so an image written by rac_conv_direct_fwd can be read as it is.  Cout = 256, Cin a multiple of 32, any H*W. */
int rac_conv3x3_relu_cf_fwd(const void *xs, const void *ws, const float *bias, const float *amax, float scale_mul, float scale_add,
                            float w_alpha, float *out, int N, int H, int W, int Cin, int Cout, void *stream);
/* rac_conv3x3_cf_fwd: rac_conv3x3_fwd storing CHANNEL-FIRST, out [N][256][H*W] f32 = conv3x3(xs) * w_alpha / 2^e + bias[c] with no
 * activation (the image's scale from *amax, as rac_conv3x3_fwd): bit for bit rac_conv3x3_fwd's channel-last result transposed.
 * The output convolutions of the image necks (racformer_amd/necks.py).  Cout = 256, Cin a multiple of 32, any H*W; bias may be NULL. */
int rac_conv3x3_cf_fwd(const void *xs, const void *ws, const float *bias, const float *amax, float w_alpha, float *out, int N, int H,
                       int W, int Cin, int Cout, void *stream);
int rac_absmax_fwd(const float *const *srcs, const int64_t *counts, int num, float floor_value, float *amax_out,
                   void *stream);
int rac_conv_pack_fwd(const float *src, const float *amax, void *xs, int N, int C, int H, int W, int c_total,
                      int c_offset, void *stream);
/* rac_conv_pack_fwd with a per-channel bias [C] (or NULL) added before the split, for an image whose N frames come in groups
 * of frames_per_group of which only the first live_per_group exist in src ([N / frames_per_group * live_per_group, C, H, W]):
 * the other frames are the bias alone.  (The hidden half of the temporal-fusion input: the ConvGRU leaves the frames t >= 4 at
 * zero, so after the resize and the last convolution they are exactly that convolution's bias, racformer_transformer.py:674-693.) */
int rac_conv_pack_bias_fwd(const float *src, const float *bias, const float *amax, void *xs, int N, int C, int H, int W,
                           int c_total, int c_offset, int frames_per_group, int live_per_group, void *stream);
int rac_conv3x3_fwd(const void *xs, const void *ws, const float *bias, const float *pixel_bias, const float *amax,
                    float w_alpha, float *out, int N, int H, int W, int Cin, int Cout, void *stream);
/* rac_conv3x3_fwd whose epilogue writes the int16 block storage of rac_quant_i16_fwd instead of fp32 (the radar BEV value stream,
 * value_proj composed into the weights: the convolution's result IS the stream rac_bev_sampling_multi_q16_fwd reads):
 *   q [N*H*W][256] int16, scale [N*H*W][4] f32 -- bit for bit rac_quant_i16_fwd(rac_conv3x3_fwd(...)), without the fp32 stream. */
int rac_conv3x3_q16_fwd(const void *xs, const void *ws, const float *bias, const float *pixel_bias, const float *amax,
                        float w_alpha, void *q, float *scale, int N, int H, int W, int Cin, int Cout, void *stream);

/* Producer-side pyramid layout: the last stage of the image neck -- the per-level 3x3 / pad 1 /
 * Cin -> 256 output convolution of the FPN (mmdet 2.28.2 FPN.fpn_convs[i], the same structure as the in-tree CustomFPN,
 * models/necks/fpn.py:109-132,180) -- writing the layout the decoder samples from directly, so that the reshape / permute copy
 * of models/racformer_transformer.py:112-124 (1.47 GB of traffic per sample at f8) never runs:
 *   xs / ws / amax / w_alpha : as for rac_conv3x3_fwd (activation image of the laterals [num_images, Cin, H, W], image index
 *                              (b*T + t) * num_cams + cam; packed weights [9][Cin/32][256][2][32])
 *   out : device f32 [num_images / num_cams * 4][num_cams][H][W][64]: slot (b*T + t) * 4 + g holds output channels g*64..g*64+63
 *         of the num_cams images of (b, t), channel-last -- the `feats` operand of rac_sampling4d_fwd / rac_msmv_fwd.
 * bias: device f32 [256] or NULL.  num_images % num_cams == 0; any H, W. */
int rac_fpn_conv_fwd(const void *xs, const void *ws, const float *bias, const float *amax, float w_alpha, float *out,
                     int num_images, int H, int W, int Cin, int num_cams, void *stream);

/* The lateral 1x1 convolution of an image-neck level with the top-down merge (mmdet FPN / CustomFPN: ConvModule(Cin, 256, 1) with
 * bias, no norm, no activation, then laterals[i] += F.interpolate(laterals[i + 1], size=(H, W), mode='nearest');
 * models/necks/fpn.py:159-176), read straight from the channel-first backbone map:
 *     out[n][co][p] = sum_ci W[co][ci] * x[n][ci][p] + bias[co] + (top ? top[n][co][src(p)] : 0)
 *   x       : device f32 [N][Cin][H*W] (the backbone stage's [B*T*N, Cin, H, W]);  Cin a multiple of 32, any H, W >= 1
 *   w_image : device f16 line image [256][Cin/32][hi 32 | lo 32] (rac_gemm_split_pack_fwd with scale 2^s); w_alpha = 2^-s
 *   bias    : device f32 [256] or NULL
 *   top     : device f32 [N][256][top_h*top_w] -- the coarser level's merged lateral, i.e. the previous call's out -- or NULL;
 *             1 <= top_h <= H, 1 <= top_w <= W.  src(p) of p = h*W + w is the legacy 'nearest' rule, per axis
 *             min((int)floorf(dst * ((float)in / out)), in - 1) in float32 (not 'nearest-exact')
 *   out     : device f32 [N][256][H*W], channel-first: the next finer level's top and the source of rac_absmax_fwd / rac_conv_pack_fwd
 * Split-precision f16 MFMA (hi / lo per operand, three products, fp32 accumulate), activation scale per pixel.  No atomics; the
 * grid depends on the shapes alone.  Cout = 256.  w_image / bias 16-byte aligned (16-byte loads of x when it is aligned and
 * H*W % 4 == 0, 4-byte loads otherwise). */
int rac_fpn_lateral_fwd(const float *x, const void *w_image, float w_alpha, const float *bias, const float *top, float *out, int N,
                        int Cin, int H, int W, int top_h, int top_w, int Cout, void *stream);

/* Backward of the lateral stage, level by level from the finest to the coarsest (racformer_amd/necks.py walks them).  No atomics, fixed
 * summation orders, grids from the shapes alone, nothing read back; Cout = 256, Cin a multiple of 32 from 32 to 2048, any H, W >= 1.
 *
 *   rac_fpn_merge_bwd     G[n][c][p] = A[n][c][p] + sum over q with src(q) == p of Gfine[n][c][q]: the gradient of a level's merged
 *                         lateral.  a [N][C][H*W] (what the level's own 3x3 convolution sends back) or NULL; gfine [N][C][fine_h*fine_w]
 *                         (the finer level's G) or NULL, not both NULL; fine_h >= H, fine_w >= W.  row_start [H + 1] / col_start
 *                         [W + 1]: device int32, the fine rows / columns whose src is i are [start[i], start[i + 1]) (src is
 *                         non-decreasing; built on the host with the forward's float32 arithmetic).  Children are added to A
 *                         row-major, in exact float32; ranges are clamped to the fine map.
 *   rac_fpn_lateral_dgrad dx[n][ci][p] = sum_co W[co][ci] * g[n][co][p]: the forward's kernel with K = 256 and Cin output channels.
 *                         wt_image: f16 line image of W^T, [Cin rounded up to a multiple of 256][8][hi 32 | lo 32] -- rac_linear_pack_wt
 *                         of W [256][Cin] with scale 2^s into its first Cin rows, the rows behind them allocated (they are read, their
 *                         products are not stored); w_alpha = 2^-s.  Scale of g per pixel, as the forward's of x.  16-byte aligned
 *                         image; 16-byte loads of g when it is aligned and H*W % 4 == 0.
 *   rac_fpn_lateral_wgrad dw[co][ci] = sum_{n,p} g[n][co][p] * x[n][ci][p] and, db != NULL, db[co] = sum_{n,p} g[n][co][p].  K is cut
 *                         into units of 32 pixels of one image (N * ceil(H*W / 32) of them) and the units into k_splits contiguous
 *                         ranges of ceil(units / k_splits), none empty; workspace f32 [k_splits][256][Cin] + [k_splits][256] holds the
 *                         ranges' partial sums, which a second launch adds in ascending order.  Split f16 operands with one
 *                         power-of-two scale per channel and range (it factors out of a sum over pixels; a per-pixel scale does not). */
int rac_fpn_merge_bwd(const float *a, const float *gfine, const int *row_start, const int *col_start, float *g, int N, int C, int H,
                      int W, int fine_h, int fine_w, void *stream);
int rac_fpn_lateral_dgrad(const float *g, const void *wt_image, float w_alpha, float *dx, int N, int Cin, int H, int W, int Cout,
                          void *stream);
int rac_fpn_lateral_wgrad(const float *g, const float *x, float *workspace, float *dw, float *db, int N, int Cin, int H, int W,
                          int Cout, int k_splits, void *stream);

/* Element-wise pieces of RadarBEVTemporalEncoder (models/racformer_transformer.py:618-720).
 *   rac_gru_gate_fwd   ConvGRUCell update after the gates convolution (:705-720): gates [B,3C,H,W] (z | r | cand),
 *                      h_prev [B,C,H,W] (batch stride h_prev_bstride floats) -> h_out (batch stride h_out_bstride):
 *                      h = (1 - sigmoid(z)) * h_prev + sigmoid(z) * tanh(cand + sigmoid(r) * h_prev);
 *                      bias_map (optional [3C,H,W]) is added to the gates first; h_out2 (optional) receives h as well
 *   rac_upsample2x_fwd nn.Upsample(scale_factor=2, bilinear, align_corners=True) (:633-636) on `planes` = N*C maps
 *                      [h,w] -> [2h,2w] */
int rac_gru_gate_fwd(const float *gates, const float *h_prev, int64_t h_prev_bstride, float *h_out, int64_t h_out_bstride,
                     const float *bias_map, float *h_out2, int64_t h_out2_bstride, int B, int C, int HW, void *stream);
int rac_upsample2x_fwd(const float *src, float *dst, int64_t planes, int h, int w, void *stream);

/* The small dense layers of a decoder layer with their surrounding row-wise work in one launch
 * (models/racformer_transformer.py:170-177, 243-269: nn.Linear + the add / split-K sum / nn.LayerNorm / ReLU before it):
 *   X   = per 256-wide segment s:  [relu]( LN( a_scale * sum_p a[p] + bias0 + residual ) * gamma + beta ) [+ post]
 *   out = [relu on columns >= relu_from]( X @ w^T + b ),   w [N][256*num_seg] (torch Linear layout), exact-fp32 MFMA.
 * Segment sources are rows of 256 floats: row r of partial p at a + p*partial_stride + r*ld_a; residual / post / x_out
 * rows at their own strides; gamma == NULL skips the LayerNorm (relu / post still apply).  x_out (optional) receives
 * the finished segment; split_out (optional) its f16 [hi | hi | lo | pad] image (layout of rac_add_ln_fwd's split_out).
 * Up to RAC_ROWGEMM_MAX_BATCH independent GEMMs over the same `rows` share the launch (descs: HOST array). */
#define RAC_ROWGEMM_MAX_BATCH 3
typedef struct {
    const float *a;
    int64_t partial_stride;
    const float *bias0, *residual, *gamma, *beta, *post;
    float *x_out;
    void *split_out;
    int ld_a, num_partials, ld_res, ld_post, ld_xout, relu, split_pad, split_layout;
    float a_scale, eps, split_scale;
} rac_rowseg;
typedef struct {
    rac_rowseg seg[3];
    const float *w, *b;
    float *out;
    int num_seg, N, ld_out, relu_from;
} rac_rowgemm;
int rac_rowgemm_fwd(const rac_rowgemm *descs, int num, int rows, void *stream);

/* The downsample convolution of RadarBEVTemporalEncoder (3x3, stride 2, pad 1, Cin -> 64; models/racformer_transformer.py:632,646)
 * on the activation image of rac_conv_pack_fwd (its first Cin channels; the image holds Cin_image >= Cin channels) with the
 * arithmetic of rac_conv3x3_fwd.  ws = f16 [9 taps][Cin/32][64][2][32];  out: channels 0..63 of an NCHW f32 buffer
 * [N, out_channels_total, H/2, W/2] (64 for a plain output);  (H/2)*(W/2) % 128 == 0. */
int rac_conv3x3s2_fwd(const void *xs, const void *ws, const float *bias, const float *amax, float w_alpha, float *out,
                      int out_channels_total, int N, int H, int W, int Cin, int Cin_image, int Cout, void *stream);

/* NMS-free decode of one sample in one launch: sigmoid, top-max_num of the num_query x num_classes scores (sorted by
 * score, ties by flat index), label = idx % C, query = idx / C, denormalize_bbox (exp of the log sizes, atan2 of sin / cos),
 * centre-range and score masks, z moved to the box bottom.  Replaces NMSFreeCoder.decode_single + the reshuffle of
 * get_bboxes (models/bbox/coders/nms_free_coder.py:37-88, models/bbox/utils.py:26-46, models/racformer_head.py:488-507).
 *   cls_scores [Q,C] logits, bbox_preds [Q,10] = (cx, cy, log w, log l, cz, log h, sin, cos, vx, vy) of the last layer
 *   out [max_num,11] = (x, y, z_bottom, w, l, h, yaw, vx, vy, score, label); masked rows carry score = -1
 *   post_center_range: HOST (6);  Q*C <= 16384, max_num <= 512 */
int rac_decode_fwd(const float *cls_scores, const float *bbox_preds, float *out, int num_query, int num_classes,
                   int max_num, const float *post_center_range, float score_threshold, int use_threshold, void *stream);

/* Backward of the two gather operators (SURVEY.md section 8 "next" row f4; fp32 features only).
 * rac_msmv_bwd  <- _ms_deform_attn_cuda_{c45,c2345,c23456}_backward, models/csrc/msmv_sampling/msmv_sampling.cpp:302-497
 *                  (kernels msmv_sampling_backward.cu:108-440): grad_out [S,Q,C,P]; grad_feats[l] like feats[l] and
 *                  ZERO-FILLED by the caller; grad_loc [S,Q,P,3] (view component = 0), grad_w [S,Q,P,L] overwritten.
 * rac_msda_bwd  <- mmcv `_ext.ms_deform_attn_backward`, call site models/multi_scale_deformable_attn_function.py:148-158:
 *                  grad_out [bs,Q,heads*dim]; grad_value like value, ZERO-FILLED by the caller; grad_loc / grad_attn
 *                  like loc / attn, overwritten.
 * grad_loc / grad_w / grad_attn have one writer per element (deterministic); the feature / value scatter uses float
 * atomics, so those two gradients can differ in the last bits from run to run (as in the reference). */
int rac_msmv_bwd(const float *grad_out, const void *const *feats, const int32_t *hw, int L, const float *loc,
                 const float *w, void *const *grad_feats, float *grad_loc, float *grad_w, int S, int N, int Q,
                 int P, int C, void *stream);
/* Backward of rac_msmv_v2_fwd (fp32 features, either layout; grad_out [S,Q,C,P]).  grad_feats[l] like feats[l] and
 * ZERO-FILLED by the caller: only level l* of each point receives its scatter (float atomics, last bits may vary from run to
 * run).  grad_loc [S,Q,P,3] overwritten, one writer per element (deterministic): (u, v) = (W_l*-1 | H_l*-1) *
 * sum_c grad_out[c] * d bilinear / d(w | h), view component 0 (as rac_msmv_bwd).  The weights get no gradient (argmax). */
int rac_msmv_v2_bwd(const float *grad_out, const void *const *feats, const int32_t *hw, int L, const float *loc,
                    const float *w, void *const *grad_feats, float *grad_loc, int S, int N, int Q, int P, int C,
                    int feat_layout, void *stream);
/* rac_msmv_bwd / rac_msmv_v2_bwd with grad_out in layout `grad_layout` (T, G as rac_msmv_fwd): RAC_OUT_SQCP [S,Q,C,P], or
 * RAC_OUT_BQGTPC [B,Q,G,T*P,C], slot s = (b*T+t)*G+g -- the tensor rac_msmv_fwd / rac_msmv_v2_fwd write for sampling_4d, read
 * as it lies (no permute copy; at C = 64 a point's channels are one contiguous 256-byte row).  T >= 1 and G >= 1 always;
 * under RAC_OUT_BQGTPC S must be a multiple of T*G.  Every other argument, and every result, as the entry point without _ex:
 * grad_loc / grad_w bit-identical between the two layouts.  rac_msmv_bwd(...) is rac_msmv_bwd_ex(grad_out, RAC_OUT_SQCP, 1, 1,
 * ...), likewise for v2. */
int rac_msmv_bwd_ex(const float *grad_out, int grad_layout, int T, int G, const void *const *feats, const int32_t *hw, int L,
                    const float *loc, const float *w, void *const *grad_feats, float *grad_loc, float *grad_w, int S, int N,
                    int Q, int P, int C, void *stream);
int rac_msmv_v2_bwd_ex(const float *grad_out, int grad_layout, int T, int G, const void *const *feats, const int32_t *hw,
                       int L, const float *loc, const float *w, void *const *grad_feats, float *grad_loc, int S, int N, int Q,
                       int P, int C, int feat_layout, void *stream);
int rac_msda_bwd(const float *grad_out, const float *value, const int64_t *shapes, const int64_t *starts,
                 const float *loc, const float *attn, float *grad_value, float *grad_loc, float *grad_attn,
                 int bs, int keys, int heads, int dim, int Q, int L, int P, void *stream);

/* BEVPoolv2 (Lift-Splat-Shoot voxel pooling) -- SURVEY.md section 8 "next" row f2.  Replaces
 * bev_pool_v2_forward / bev_pool_v2_backward of models/csrc/bev_pool_v2/src/bev_pool.cpp:40-111
 * (kernels bev_pool_cuda.cu:21-136); argument order follows those entry points.
 *   depth [b,n,d,h,w] f32, feat [b,n,h,w,c] f32, out [b,z,y,x,c] f32 (pre-zeroed by the caller, as in
 *   bev_pool.py:29), ranks_* int32 [n_points], interval_* int32 [n_intervals]; all device pointers.
 * Backward expects the intervals regrouped by ranks_feat (bev_pool.py:50-63) and depth_grad / feat_grad
 * pre-zeroed.  Deterministic: one writer per output element, no atomics. */
int rac_bev_pool_v2_fwd(const float *depth, const float *feat, float *out, const int32_t *ranks_depth,
                        const int32_t *ranks_feat, const int32_t *ranks_bev, const int32_t *interval_lengths,
                        const int32_t *interval_starts, int c, int n_intervals, void *stream);
int rac_bev_pool_v2_bwd(const float *out_grad, float *depth_grad, float *feat_grad, const float *depth,
                        const float *feat, const int32_t *ranks_depth, const int32_t *ranks_feat,
                        const int32_t *ranks_bev, const int32_t *interval_lengths, const int32_t *interval_starts,
                        int c, int n_intervals, void *stream);

/* ---- Round 5: the ConvGRU branch of RadarBEVTemporalEncoder without library convolutions -------------------------------------
 * (models/racformer_transformer.py:645-656 inner_forward, :674-693 ConvGRU, :705-720 ConvGRUCell)
 *
 * rac_conv_direct_fwd: a 3x3 convolution (stride 1 or 2, pad 1) for the SMALL maps of that branch (64 x 64 x 64 channels, one
 * frame at a time through the recurrence), with the split-precision arithmetic of rac_conv3x3_fwd (three f16 MFMA products of
 * hi / lo operands, fp32 accumulate: fp32-convolution accuracy).  The WEIGHTS of a workgroup's output-channel block pass through
 * an LDS double buffer, one 32-channel chunk (9 taps) per buffer (108 KB for 48-channel blocks, 144 KB for 64-channel ones), with
 * one workgroup barrier per chunk; the PIXELS never do: every lane loads its MFMA fragments straight from the activation image
 * (L2-resident at these sizes) through a register ring three K steps ahead -- these launches are latency-bound chains, not
 * throughput kernels.  The chunk count is a template parameter (the K loop is straight-line code); instantiated are
 *   stride 2, RAC_CD_IMAGE: chunks 2 | 3 | 8;   stride 1, RAC_CD_IMAGE and RAC_CD_IMAGE_RELU: chunks 2;
 *   RAC_CD_F32: chunks 1 | 2 | 4;   RAC_CD_F32_CF_RELU: chunks 2;   RAC_CD_GRU: chunks 0 | 2
 * and any other count is an argument error.  bias, pixel_map, out_f32, xpart, h_prev and h_out must be 16-byte aligned.
 * A frame map carries no frame count: that every frame(n), n < N, lies inside its buffer is the caller's responsibility.
 *
 *   in_img   f16 [frames][H+2][W+2][in_chunks_total][hi 32 | lo 32]  zero border; K runs over chunks in_chunk0 .. +chunks-1
 *            (chunks == 0: no convolution, the accumulators stay zero -- the recurrence's first step, h_0 = 0)
 *   ws       f16 [9 taps][chunks][Cout][hi 32 | lo 32]  (racformer_amd.fused.pack_conv3x3_weight), w_alpha = its 2^-s
 *   scales   an image's power-of-two scale is rac's act_scale(bound) with bound = mul * (*amax) + add  (amax may be NULL):
 *            a DEVICE word plus host constants, so that a bound derived from the weights follows the measured input maximum
 *   frame maps  frame(n) = (n / live) * stride + n % live + first:  the n-th processed frame inside a [groups][stride] stack
 * mode RAC_CD_IMAGE : out_img <- (conv + bias) as an activation image [frames][OH+2][OW+2][out_chunks_total][hi|lo], channels
 *                     out_chunk0 * 32 .. (interior pixels only; the caller zeroed the border once)
 * mode RAC_CD_F32   : out_f32 [N][OH*OW][Cout] channel-last <- conv + bias + pixel_map[OH*OW][Cout] (either may be NULL)
 * mode RAC_CD_GRU   : Cout = 3 * 64 gate channels (z | r | candidate); pre = conv(h_prev image) + xpart[frame][pixel][192];
 *                     z = sigmoid, r = sigmoid, cand = tanh(pre_c + r * h_prev), h = (1 - z) h_prev + z cand  (:714-720);
 *                     h -> h_out f32 [frames][OH*OW][64] AND out_img (the next step's convolution input); h_prev NULL = zeros
 * mode RAC_CD_IMAGE_RELU   : RAC_CD_IMAGE with out_img <- relu(conv + bias); stride 1, chunks = 2 (64 input channels)
 * mode RAC_CD_F32_CF_RELU  : out_f32 [N][Cout][OH*OW] CHANNEL-FIRST <- relu(conv + bias); stride 1, chunks = 2, no pixel_map.
 *                     These two are Conv2d(3x3, pad 1, bias=False) + BatchNorm2d (folded into weights and bias by the host) + ReLU
 *                     of radar_bev_conv (models/racformer.py:81-99); the modes 0..2 are unchanged by them, bit for bit.
 */
enum { RAC_CD_IMAGE = 0, RAC_CD_F32 = 1, RAC_CD_GRU = 2, RAC_CD_IMAGE_RELU = 3, RAC_CD_F32_CF_RELU = 4 };
typedef struct {
    const float *amax;     /* device word or NULL */
    float mul, add;
} rac_cd_scale;
typedef struct {
    int live, stride, first;
} rac_cd_frames;
typedef struct {
    int mode, conv_stride;           /* RAC_CD_*, 1 | 2 */
    int N, H, W;                     /* frames processed; INPUT map size (output = H / conv_stride x W / conv_stride) */
    const void *in_img;
    int in_chunks_total, in_chunk0, chunks;
    rac_cd_frames in_frames;
    rac_cd_scale in_scale;
    const void *ws;
    float w_alpha;
    int Cout;
    const float *bias;               /* [Cout] or NULL (IMAGE, F32) */
    void *out_img;                   /* IMAGE, GRU */
    int out_chunks_total, out_chunk0;
    rac_cd_frames out_frames;
    rac_cd_scale out_scale;
    float *out_f32;                  /* F32 */
    const float *pixel_map;          /* F32: [OH*OW][Cout] or NULL */
    const float *xpart;              /* GRU: [frames][OH*OW][192] */
    rac_cd_frames xpart_frames;
    const float *h_prev;             /* GRU: [frames][OH*OW][64] or NULL */
    rac_cd_frames h_prev_frames;
    float *h_out;                    /* GRU */
    rac_cd_frames h_out_frames;
} rac_conv_direct;
int rac_conv_direct_fwd(const rac_conv_direct *desc, void *stream);

/* nn.Upsample(scale_factor=2, bilinear, align_corners=True) (models/racformer_transformer.py:633-636) of channel-last maps
 * src f32 [frames][h*w][C] straight into an activation image f16 [frames][2h+2][2w+2][C/32][hi 32 | lo 32] (interior pixels)
 * with the scale act_scale(bound); C % 32 == 0. */
int rac_upsample2x_image_fwd(const float *src, void *img, int frames, int h, int w, int C, float bound, void *stream);

/* rac_conv3x3_fwd / rac_conv3x3_q16_fwd for a stack of [groups][frames_per_group] images of which only the first live_per_group
 * of a group carry all Cin channels: the others' last Cin - Cin_dead channels are a per-channel constant (the ConvGRU leaves
 * frames >= 4 at zero, so their hidden half is the bias of the convolution behind the resize, :674-693), whose contribution
 * the caller has folded into THEIR per-pixel map (border-aware: composed through the zero padding) -- those images run
 * Cin_dead / 32 chunks per tap and add pixel_bias_dead instead of pixel_bias_live.  Exactly one of out / (q, scale). */
int rac_conv3x3_temporal_fwd(const void *xs, const void *ws, const float *pixel_bias_live, const float *pixel_bias_dead,
                             const float *amax, float w_alpha, float *out, void *q, float *scale, int N, int H, int W, int Cin,
                             int Cin_dead, int frames_per_group, int live_per_group, void *stream);

/* ---- backward of the 3x3 / stride 1 / pad 1 convolution of rac_conv3x3_fwd (the temporal-fusion convolution under autograd) ----
 * Same arithmetic as the forward: hi / lo split operands, three f16 MFMA products, fp32 accumulate.
 *
 * Data gradient: dX = conv3x3(dY, W') with W'[ci][co][ky][kx] = W[co][ci][2-ky][2-kx] is rac_conv3x3_fwd itself (bias NULL) on
 * an activation image of dY (256 channels, its scale from rac_absmax_fwd) and a weight image packed from W'
 * (racformer_amd.fused.pack_conv3x3_dgrad_weight: 256 input channels of W at a time, zero output columns where fewer remain).
 *
 *   rac_conv_pack_cl_fwd  rac_conv_pack_fwd for a channel-LAST source: src [N,H,W,C] f32 (contiguous, 16-byte aligned) -> channel
 *                         range [c_offset, c_offset+C) of the image xs f16 [N][H+2][W+2][c_total/32][hi 32 | lo 32] (interior
 *                         pixels; the border must be zero).  C, c_total, c_offset multiples of 32.
 *   rac_conv3x3_wgrad     dw [256][Cin][3][3] f32 = sum_{n,h,w} dY[n,co,h,w] X[n,ci,h+ky-1,w+kx-1] from the two images
 *                         xs (X: Cin channels, scale amax_x) and gs (dY: 256 channels, scale amax_g).  The N*H image rows are
 *                         split into k_splits contiguous ranges (1 <= k_splits <= N*H) whose partial sums go to
 *                         workspace [k_splits][9][256][Cin] f32 and are added in ascending order by a second launch: no float
 *                         atomics, bitwise reproducible for equal k_splits.  Cin a multiple of 32, Cout == 256, any H, W. */
int rac_conv_pack_cl_fwd(const float *src, const float *amax, void *xs, int N, int C, int H, int W, int c_total, int c_offset,
                         void *stream);
int rac_conv3x3_wgrad(const void *xs, const void *gs, const float *amax_x, const float *amax_g, float *workspace, float *dw, int N,
                      int H, int W, int Cin, int Cout, int k_splits, void *stream);

/* ---- the two big Linears of AdaptiveMixing under autograd (y = x W^T + b: x [M][K], W [N][K], g = dy [M][N]) ----
 * Same arithmetic as the forward kernels: hi / lo split operands, three f16 MFMA products, fp32 accumulate; no float atomics,
 * fixed summation orders (bitwise reproducible); no host synchronisation and no allocation in any of them.
 * Activations and gradients carry a DEVICE-side scale: amax (device f32[1], from rac_absmax_fwd) is read by the kernels, the
 * image holds v * rac_act_scale(amax) with the scale a power of two that brings amax into [2^13, 2^14) (1 for amax == 0).
 *
 *   rac_linear_pack_act   src f32 rows [M][K], row m at src + m*ld_src -> image f16 [M][K/32][hi 32 | lo 32] (the X / Z image of
 *                         rac_generator_fwd / rac_outproj_fwd).  K % 32 == 0, ld_src % 4 == 0, 16-byte aligned.  Rows past M
 *                         are never read; amax == 0 gives an all-zero image.
 *   rac_linear_pack_wt    weight f32 [N][K] (contiguous) -> the line image of its TRANSPOSE, f16 [K][N/32][hi 32 | lo 32] of
 *                         weight * scale (host float): the W operand of a data gradient dX = g W.  N, K multiples of 32.
 *   rac_generator_ds_fwd  rac_generator_fwd's K == 256 weights-stationary kernel for an X image with a device-side scale:
 *                         out[m][n] = alpha / rac_act_scale(*amax) * sum_k X[m][k] W[n][k] + bias[n]  (bias NULL: none).
 *                         The generator forward (X: pack of the query) and out_proj's data gradient dZ (X: pack of g, W: the
 *                         transposed image of W_out).  A second instantiation: rac_generator_fwd's own code is unchanged.
 *   rac_linear_reduce     out[m][n] = bias[n] + alpha / rac_act_scale(*amax) * sum_s partials[s][m][n], s ASCENDING: the slices
 *                         of rac_outproj_fwd in true units -- the out_proj forward (Z image: pack of Z) and the generator's data
 *                         gradient dquery (Z image: pack of dP, W image: the transposed image of W_gen).  N, ld_out % 4 == 0.
 *   rac_linear_wgrad      C[a][b] = sum_m A[m][a] * Bm[m][b] over all M rows in ascending order, one workgroup per 128 columns b,
 *                         every output element written once.  A, the narrow operand (`narrow` == 256 columns), comes as its
 *                         line image [M][8][hi 32 | lo 32] packed with amax_narrow; Bm, the wide one (`wide_cols` a multiple of
 *                         128), as fp32 rows (row m at wide + m*ld_wide, ld_wide % 4 == 0), split in the kernel with amax_wide
 *                         (which must bound it: rac_absmax_fwd over the same tensor).
 *                         wide_major == 0: out f32 [256][wide_cols]   (dW_out: narrow = g, wide = Z)
 *                         wide_major != 0: out f32 [wide_cols][256]   (dW_gen: narrow = query, wide = dP)
 *                         colsum (f32 [wide_cols] or NULL) receives sum_m Bm[m][b] in fp32, rows added in a fixed order (the
 *                         generator's bias gradient).  Other shapes are refused (RAC_E_ARG). */
int rac_linear_pack_act(const float *src, int64_t ld_src, const float *amax, void *image, int M, int K, void *stream);
int rac_linear_pack_wt(const float *weight, void *image, int N, int K, float scale, void *stream);
int rac_generator_ds_fwd(const void *x_image, const void *w_image, const float *bias, float alpha, const float *amax, float *out,
                         int64_t ld_out, int M, int N, int K, void *stream);
int rac_linear_reduce(const float *partials, const float *bias, const float *amax, float alpha, float *out, int64_t ld_out, int slices,
                      int M, int N, void *stream);
int rac_linear_wgrad(const void *narrow_image, const float *amax_narrow, const float *wide, int64_t ld_wide, const float *amax_wide,
                     float *out, float *colsum, int M, int narrow, int wide_cols, int wide_major, void *stream);

/* ---- the head loss: match costs, assignment, focal + L1 (batched over P = num_layers * batch problems) ----
 * Ground truth: ONE concatenated table gt_boxes [sum G, 9] (x, y, z, w, l, h, yaw, vx, vy; gravity centre), gt_labels [sum G]
 * and offsets [batch + 1] (offsets[0] = 0; sample b owns rows offsets[b] .. offsets[b+1]).  offsets is a HOST array, built
 * from the lengths of the ground-truth lists; batch <= 64.
 *
 * rac_match_cost_fwd: cost [P, gmax, qpad] fp32, the query index fastest; entry (p = l * batch + b, g, q) for g < G_b, q < Q:
 *   FocalLossCost(alpha 0.25, gamma 2, eps 1e-12) * cls_weight
 *   + sum_k |pred_k cw_k - normalize_bbox(gt)_k cw_k| * reg_weight              (all 10 columns)
 *   + (polar) |remainder(|theta(pred) - theta(gt)| + 0.5, 1) - 0.5| * theta_weight, theta from the code-weighted x, y through
 *     ThetaL1Cost's own pc_range (-51.2 .. 51.2) and xy2theta_d_coods(norm=True)
 *   then nan_to_num(nan = 100, posinf = 100, neginf = -100).  Entries with g >= G_b or q >= Q are left as they are.
 *   cls_scores [L,B,Q,C], bbox_preds [L,B,Q,10], code_weights [10] (device) */
int rac_match_cost_fwd(const float *cls_scores, const float *bbox_preds, const float *gt_boxes, const int32_t *gt_labels,
                       const int32_t *offsets, const float *code_weights, float *cost, int num_layers, int batch, int num_query,
                       int num_classes, int gmax, int qpad, float cls_weight, float reg_weight, float theta_weight, int polar,
                       void *stream);

/* rac_lsap_fwd: the P rectangular assignment problems of a cost tensor laid out as above, on the device: every ground-truth box
 * gets one distinct query at minimum total cost (shortest augmenting paths, duals and path lengths in float64, the cost widened
 * on read; one wave64 per problem; ties of a step's minimum go to the smaller query index).  Entries with g >= G_b or
 * q >= num_query are never read.
 *   matched_query [P, gmax]  the query of box g (-1 for g >= G_b)
 *   assigned_gt   [P, Q]     offsets[b] + g for a matched query (an index into the concatenated table), -1 for background
 *   u [P, gmax], v [P, Q]    float64 duals: u_g + v_q <= cost everywhere, equal on matched pairs, v <= 0, v = 0 when unmatched
 *   steps [P] or NULL        Dijkstra steps taken (at most G (G + 1) / 2); negative if the problem was given up
 * A problem whose costs leave no finite path (NaN, +inf) is given up: all background, duals 0.
 * num_query <= 2048 and gmax <= num_query, else RAC_E_UNSUPPORTED (rac_lsap_host takes those). */
int rac_lsap_fwd(const float *cost, const int32_t *offsets, int32_t *matched_query, int32_t *assigned_gt, double *u, double *v,
                 int32_t *steps, int num_layers, int batch, int num_query, int gmax, int qpad, void *stream);

/* rac_lsap_host: ONE problem on the host in plain C++, the same algorithm and arithmetic, any num_gt and num_query (it iterates
 * over the smaller side).  cost(g, q) = cost[g * gt_stride + q * query_stride] (HOST memory).
 *   matched_query [num_gt] (-1: unmatched, possible when num_gt > num_query), matched_gt [num_query] (-1: background)
 *   u [num_gt], v [num_query] float64 duals; steps: one counter or NULL.  RAC_E_UNSUPPORTED if no finite assignment exists. */
int rac_lsap_host(const float *cost, int64_t gt_stride, int64_t query_stride, int num_gt, int num_query, int32_t *matched_query,
                  int32_t *matched_gt, double *u, double *v, int64_t *steps);

/* rac_det_loss_fwd: sigmoid focal loss + code-weighted L1 of rows [num_layers, rows], forward sums and unit gradients in one pass.
 *   target [L, rows]: index into the ground-truth table, -1 = background (label num_classes, no box term); NULL: row r takes
 *   entry r mod num_gt (the denoising rows).  A positive row whose normalize_bbox(gt) has a non-finite entry has no box term.
 *   sums [L, 2] = (sum of focal terms, sum of |pred - target| * code_weights) -- raw, not averaged
 *   grad_logits [L, rows, C], grad_boxes [L, rows, 10]: d sums[l,0] / d logits, d sums[l,1] / d boxes
 * Fixed-order reduction (no float atomics): bitwise reproducible. */
int rac_det_loss_fwd(const float *logits, const float *boxes, const int32_t *target, const float *gt_boxes, const int32_t *gt_labels,
                     const float *code_weights, float *sums, float *grad_logits, float *grad_boxes, int num_layers, int rows,
                     int num_classes, int num_gt, float alpha, float gamma, void *stream);

/* ---- Lift-Splat view transform around the splat (models/necks/view_transformer_racformer.py:112-295), forward and backward -------
 * Frustum point p = ((bn * D + d) * H + h) * W + w of camera bn = b * N + n (the flat index in [B,N,D,H,W] = ranks_depth);
 * pixel = bn * H * W + h * W + w (= ranks_feat); cell = ((b * Z + z) * Y + y) * X + x (= ranks_bev).  All pointers are device
 * pointers, all tables int32.  No launch is sized by a count read back and nothing floating-point is accumulated atomically:
 * the operator can be captured into a graph and is bitwise reproducible.
 *
 * rac_lss_cells_fwd: cells [B*N*D*H*W] = the point's cell, or -1 if dropped.
 *   img2lidar [B*N,4,4] row-major f32 (the host's inverse of lidar2img, cast to f32); depth_tab [D], v_tab [H], u_tab [W]: the
 *   frustum's three axes as the module's constructor built them.  point = M . (u * max(d, 1e-5), v * max(d, 1e-5), d, 1);
 *   scaled = (point - lower) / interval in true f32 division; cell index = trunc toward zero per axis; kept when
 *   0 <= index < size on all three axes -- so a scaled coordinate in (-1, 0) lands in cell 0 and IS kept (the reference's .long()).
 *
 * rac_lss_tables_fwd: cells -> ranks_bev / ranks_depth / ranks_feat [n_points], interval_starts / interval_lengths
 *   [min(n_cells, n_points)], counts [2] = (kept points, occupied cells).  Points sorted by cell, ascending ranks_depth inside a
 *   cell (histogram, one-workgroup scan, unordered fill, then each point placed by the number of smaller indices in its cell).
 *   Padding past the counts: -1 in the three rank tables, start 0 / length 0 in the interval tables (trim to the counts before
 *   handing the tables to rac_bev_pool_v2_fwd).  workspace: 3 * n_cells + n_points int32.
 *
 * rac_lss_softmax_stats_fwd: stats [B*N*H*W, 2] = (max, 1 / sum exp(x - max)) of each pixel's D logits; logits [B*N, D, H*W]
 *   (channel-first, stride H*W).  The probabilities themselves are never written.
 *
 * rac_lss_transpose_fwd: dst [batch, cols, rows] from src [batch, rows, cols]: the layout pass between channel-first tensors and
 *   channel-last rows (features [B*N, C, H*W] -> [B*N*H*W, C]; the incoming gradient [B*Z, C, Y*X] -> cell-major
 *   [B*Z*Y*X, C]; grad_feat back to channel-first).
 *
 * rac_lss_splat_fwd: out [B, Z*C, Y, X] (channel-first, channel index z * C + c -- the order of voxel_pooling_v2's
 *   torch.cat(bev_feat.unbind(dim=2), 1); fully written, empty cells zero)
 *   = sum over a cell's points of softmax_D(logits)[ranks_depth] * feat[ranks_feat, :]; feat is CHANNEL-LAST [B*N*H*W, C].
 *   The sorted points are cut into chunks of 64; one wave sums a chunk and writes one partial row per (chunk, cell) segment,
 *   row index chunk + interval index; a second kernel adds each cell's rows in chunk order and writes runs of 16 x cells through
 *   LDS.  cell_interval: B*Z*Y*X int32 scratch; partial: (ceil(n_points / 64) + min(n_cells, n_points)) * C f32 scratch.
 *   C: multiples of 4 up to 320, anything else is RAC_E_ARG and nothing is launched.
 *
 * rac_lss_view_bwd: grad_cell [B*Z*Y*X, C] (the incoming gradient, cell-major), feat channel-last ->
 *   grad_feat [B*N*H*W, C] (channel-last) = sum_d p_d * g[cell(d)] over the pixel's kept bins, and
 *   grad_logits [B*N, D, H*W] = p_d * (s_d - sum_d' p_d' s_d') with s_d = <g[cell(d)], feat[pixel]> for kept bins and 0 for
 *   dropped ones (which therefore still get a gradient).  One wave per pixel, gather only, one writer per element; D <= 256. */
int rac_lss_cells_fwd(const float *img2lidar, const float *depth_tab, const float *v_tab, const float *u_tab, int32_t *cells,
                      int BN, int N, int D, int H, int W, float lower_x, float lower_y, float lower_z, float interval_x,
                      float interval_y, float interval_z, int X, int Y, int Z, void *stream);
int rac_lss_tables_fwd(const int32_t *cells, int32_t *ranks_bev, int32_t *ranks_depth, int32_t *ranks_feat,
                       int32_t *interval_starts, int32_t *interval_lengths, int32_t *counts, int32_t *workspace,
                       int n_points, int n_cells, int D, int HW, void *stream);
int rac_lss_softmax_stats_fwd(const float *logits, float *stats, int BN, int D, int HW, void *stream);
int rac_lss_transpose_fwd(const float *src, float *dst, int batch, int rows, int cols, void *stream);
int rac_lss_splat_fwd(const float *logits, const float *stats, const float *feat, const int32_t *ranks_depth,
                      const int32_t *ranks_feat, const int32_t *ranks_bev, const int32_t *interval_starts,
                      const int32_t *interval_lengths, const int32_t *counts, int32_t *cell_interval, float *partial,
                      float *out, int n_points, int B, int C, int X, int Y, int Z, void *stream);
int rac_lss_view_bwd(const float *grad_cell, const float *logits, const float *stats, const float *feat,
                     const int32_t *cells, float *grad_feat, float *grad_logits, int BN, int C, int D, int HW, void *stream);

/* ---- LSS depth branch: radar depth / RCS priors and the depth loss (models/necks/view_transformer_racformer.py:593-699
 * get_downsampled_depth / get_downsampled_rcs / get_depth_loss / forward, models/necks/focalloss.py:114-125) ------------------
 * Maps are [BN, H, W] f32, feature pixels [BN, h, w] with h = H / ds, w = W / ds; index maps int32.  All pointers are device
 * pointers.  Every launch is sized by shapes, nothing is read back, no floating-point sum is atomic: capturable into a graph and
 * bitwise reproducible.
 *
 * rac_lss_pool_bins_fwd: one pass over the full-resolution maps, each value read once from the [BN, H, W] layout.
 *   depth (or NULL) -> pooled [BN,h,w] f32: min over the ds x ds block with zeros replaced by 1e5; NaN if any element is NaN
 *                      bins   [BN,h,w]: idx = -0.5 + 0.5 sqrt(1 + 8 (d - depth_lo) / depth_bin_size) in IEEE f32 (true division,
 *                      correctly rounded square root), truncated toward zero; depth_bins where idx < 0, idx > depth_bins or idx
 *                      is not finite.  depth_bin_size = float(2 (hi - lo) / (n (n + 1))), computed in double by the caller.
 *   rcs (or NULL)   -> rcs_class [BN,h,w]: m = max over the block with values < rcs_lo replaced by -1e5 (NaN wins);
 *                      r = (m - rcs_offset) / rcs_bin_size with rcs_offset = float(lo - bin), rcs_bin_size = float(bin);
 *                      class max(trunc(r) - 1, -1) for -1 <= r < rcs_bins + 1, else -1.  Class -1 (an all-below-range block, a
 *                      maximum >= hi, NaN) is "no class": an all-zero one-hot row, where the reference's F.one_hot raises.
 *   H % ds == 0, W % ds == 0, 1 <= ds <= 1024 (RAC_E_UNSUPPORTED beyond).
 *
 * rac_lss_prior_fwd: out [BN, (D+1)+E, hw], the tensor DepthNet.forward concatenates behind its features (:558):
 *   channels 0..D   the one-hot radar depth grid: 1 where bins == channel (rad_dep_grids, :690-693)
 *   channels D+1..  weight[e, class] + bias[e], bias[e] alone for class -1: the 1x1 rcs_embedding of the one-hot RCS map,
 *                   which is never built.  weight [E, n_rcs], bias [E].
 *
 * rac_lss_prior_bwd: grad_out [BN, (D+1)+E, hw] -> grad_weight [E, n_rcs] (sum over the pixels of each class), grad_bias [E]
 *   (sum over all pixels); both fully written.  The pixels are cut into up to 32 contiguous runs (8 segments of 4), each summed
 *   in ascending pixel order, the runs added in ascending order (a second launch adds the segments); grad_bias is the sum of a
 *   run's class sums in a fixed tree.  The one-hot channels carry no gradient.  workspace: 8 * E * (n_rcs + 1) f32 scratch.
 *   n_rcs <= 256.
 *
 * rac_lss_depth_loss_fwd: logits [BN, D, hw] (channel-first), labels [BN*hw] (foreground: 0 <= label < D) ->
 *   per foreground pixel l = sum_c (onehot_c + 1e-6) (-alpha) (1 - p_c)^2 log p_c on softmax / log-softmax (focalloss.py with
 *   its one_hot(eps = 1e-6)); gamma must be 2 (RAC_E_UNSUPPORTED otherwise).
 *   grad_unit [BN, D, hw] = dl / dlogits, unscaled; zeros at background pixels
 *   pixel_loss [BN*hw] or NULL: l itself, 0 at background pixels
 *   partial   [ceil(BN*hw / 64), 2] scratch: (sum of l, foreground count) per workgroup, combined in index order by a second launch
 *   loss [1]  = weight * sum / max(1, count);   scale [1] = weight / max(1, count)
 *
 * rac_lss_depth_loss_bwd: grad_logits [n] = grad_unit * (scale[0] * grad_loss[0]); the three operands stay on the device. */
int rac_lss_pool_bins_fwd(const float *depth, const float *rcs, float *pooled, int32_t *bins, int32_t *rcs_class, int BN, int H,
                          int W, int ds, float depth_lo, float depth_bin_size, int depth_bins, float rcs_lo, float rcs_offset,
                          float rcs_bin_size, int rcs_bins, void *stream);
int rac_lss_prior_fwd(const int32_t *bins, const int32_t *rcs_class, const float *weight, const float *bias, float *out, int BN,
                      int hw, int D, int E, int n_rcs, void *stream);
int rac_lss_prior_bwd(const float *grad_out, const int32_t *rcs_class, float *workspace, float *grad_weight, float *grad_bias, int BN,
                      int hw, int D, int E, int n_rcs, void *stream);
int rac_lss_depth_loss_fwd(const float *logits, const int32_t *labels, float *partial, float *grad_unit, float *pixel_loss,
                           float *loss, float *scale, int BN, int D, int hw, float alpha, float gamma, float weight, void *stream);
int rac_lss_depth_loss_bwd(const float *grad_unit, const float *scale, const float *grad_loss, float *grad_logits, int64_t n,
                           void *stream);

/* ---- Image preparation of a training step (models/racformer.py:198-224, :108-109; models/utils.py:8-45, :219-305) ----------------
 * rac_image_aug_fwd: img [n, 3, H, W] f32 (device, the loader's BGR image) -> out [n, 3, Hp, Wp] f32 (device), Hp >= H, Wp >= W, in
 *   one launch; img is only read.  Per pixel, float32 with the reference's operations one by one (IEEE division, no contraction):
 *     working R, G, B = input channels 2, 1, 0
 *     where the image's table row has colour != 0 (GpuPhotoMetricDistortion): + delta; * alpha0; rgb_to_hsv (/255, eps 1e-8, deltac == 0
 *       -> 1, hue from the first maximal channel, (h / 6) floor-mod 1, * 360); s * sat; h + hue, then h - 360 where h > 360, then
 *       h + 360 where h < 0; hsv_to_rgb (floor(6h) floor-mod 6, the 18-entry table, * 255); * alpha1.  No clipping.
 *     output channel k = working[map[k]]: the random channel permutation, the flip back to BGR and to_rgb folded into one map
 *     (x - mean[k]) / std[k] unless mean and std are NULL
 *     0 at pixels outside the grid mask's bands (GridMask keeps the bands and zeroes the rest) and in the pad rows and columns
 *   table: device f32 [n][9] = colour, delta, alpha0, sat, hue, alpha1, map[0], map[1], map[2] (the map as 0.0 / 1.0 / 2.0).
 *   mean, std: HOST pointers to 3 floats each, or both NULL.
 *   grid mask: grid_d == 0 for none; else the four integers GridMask draws and derives (d >= 2, 1 <= l < d, 0 <= st_h, st_w < d) on
 *   the canvas int(1.5 Hp) x int(1.5 Wp) with the centre crop; no mask tensor is built.
 *   A lane owns four pixels of a row: 16-byte loads and stores where W % 4 == 0, Wp % 4 == 0 and both pointers are 16-byte aligned,
 *   scalar accesses otherwise.  No atomics, nothing read back: capturable, two runs give the same bits. */
int rac_image_aug_fwd(const float *img, const float *table, float *out, int n, int H, int W, int Hp, int Wp, const float *mean,
                      const float *stdv, int grid_d, int grid_l, int grid_st_h, int grid_st_w, void *stream);

/* ---- Radar pillar encoder: point clouds to the BEV canvas (models/racformer.py:130-177 extract_pts_feat / radar_voxelize; mmcv 1.6.0
 * Voxelization (hard), mmdet3d 1.0.0rc6 PillarFeatureNet and PointPillarsScatter; configs/racformer_r50_nuimg_704x256_f8.py:122-139) ----
 * All clouds of a call are packed: points [n_points][C] f32, cloud_offsets [n_clouds + 1] int32 (cloud c = rows offsets[c] ..
 * offsets[c+1] - 1; offsets[n_clouds] <= n_points, rows past it belong to no cloud), both on the device.  Launches are sized by
 * n_points and n_clouds * cells; nothing is read back, no float atomics (integer min / max only): capturable, bitwise reproducible.
 *
 * rac_pillar_voxelize_fwd: hard voxelization in the one deterministic order (mmcv's CPU path / deterministic=True): walking a
 *   cloud's points in input order, c_j = floor((p_j - lo_j) / vs_j) in IEEE f32 (true division); a point outside [0, grid_j) on any
 *   axis is skipped; a new cell gets the next pillar index while fewer than max_voxels exist (afterwards its points are skipped,
 *   points of registered cells are still taken); a pillar keeps its first max_num_points points.
 *     voxels      f32 [n_points][max_num_points][C]   pillar i of cloud c is row offsets[c] + i; zero-padded
 *     coors       int32 [n_points][4] = (cloud, c_z, c_y, c_x); -1 in rows that hold no pillar
 *     num_points  int32 [n_points]; 0 in rows that hold no pillar
 *     counts      int32 [n_clouds]: pillars per cloud
 *     amax        f32 [1]: max |value| over the in-range points (0 if none) -- the device word of the activation image's scale
 *     workspace   int32 [2 * n_clouds * cells + n_points]
 *   Limits: 4 <= C <= 16, 1 <= max_num_points <= 32, n_clouds * cells < 2^30, n_points * max_num_points * C < 2^31.
 *
 * rac_pillar_encode_fwd: PillarFeatureNet (one PFN layer, 64 channels, with_cluster_center, with_voxel_center, legacy=False, no
 *   distance) + PointPillarsScatter in one launch per destination set.  Per pillar: mean = sum of the rows' xyz / num_points;
 *   features [C raw | xyz - mean | x - (c_x vs_x + center_x), y and z alike] (C + 6); y = relu(wt^T f + shift) per row, wt f32 [C+6][64]
 *   and shift [64] holding the Linear with the BatchNorm1d folded in; max over the max_num_points rows, rows >= num_points taking
 *   part with relu(shift) (the reference zeroes their features and still runs them through Linear / BN / ReLU / max).  A NaN among
 *   a pillar's candidates wins the maximum, as torch.relu and torch.max have it: a NaN point feature gives NaN in that pillar's
 *   channels (feats, canvas and image), and no other pillar changes.
 *     canvas  f32 [n_clouds][64][H][W] (PointPillarsScatter's result: canvas[cloud, :, c_y, c_x]) or NULL
 *     image   f16 [n_clouds][H+2][W+2][2][hi 32 | lo 32] activation image of rac_conv_direct_fwd or NULL, with the scale
 *             act_scale(bound_mul * (*amax) + bound_add) (amax may be NULL)
 *     feats   f32 [n_rows][64]: the pillar features themselves (PillarFeatureNet.forward's result), rows without a pillar are
 *             not written; or NULL
 *   Any subset, at least one; canvas and image are cleared on the stream first (the image's border included), so cells without a
 *   pillar read as zero on every call.  n_rows = rows of voxels / coors / num_points; rows whose coors are -1 are skipped.  H = grid_y, W = grid_x. */
int rac_pillar_voxelize_fwd(const float *points, const int32_t *cloud_offsets, float *voxels, int32_t *coors, int32_t *num_points,
                            int32_t *counts, float *amax, int32_t *workspace, int n_points, int n_clouds, int C, float lo_x,
                            float lo_y, float lo_z, float vs_x, float vs_y, float vs_z, int grid_x, int grid_y, int grid_z,
                            int max_num_points, int max_voxels, void *stream);
int rac_pillar_encode_fwd(const float *voxels, const int32_t *coors, const int32_t *num_points, const float *wt, const float *shift,
                          const float *amax, float bound_mul, float bound_add, float *canvas, void *image, float *feats, int n_rows,
                          int n_clouds,
                          int C, int max_num_points, int F, float vs_x, float vs_y, float vs_z, float center_x, float center_y,
                          float center_z, int H, int W, void *stream);

/* ---- Training through the radar pillar branch (models/racformer.py:316-331: frame 0 runs extract_pts_feat in training mode under
 * autograd; csrc/radar_pillars.hip, csrc/batchnorm_train.hip).  The BatchNorm1d of the PFN layer and the BatchNorm2d of the three
 * radar_bev_conv layers use BATCH statistics and update their running statistics; the convolutions between them are
 * rac_resnet_conv_fwd / _dgrad / _wgrad.  No float atomics, every sum float64 in one fixed order, launch geometry from the shapes
 * alone, nothing read back (the number of pillars stays on the device): capturable, bitwise reproducible.  Every argument is checked
 * before any launch.  Points get no gradient (the voxelization is no_grad in the reference too).
 *
 * rac_pillar_train_fwd: per real point row x = W f (the decoration and the fma chain of rac_pillar_encode_fwd, W the RAW Linear weight);
 *   per channel mean and biased variance over all n = M * P rows of the call, M = rows with num_points > 0 and coors[0] >= 0, P =
 *   max_num_points >= 2 -- the padded rows count, they are exactly 0 and add nothing to the sums;
 *   y = relu((x - mean) * invstd * gamma + beta); feature = max over the P slots, a padded slot taking part with
 *   relu((0 - mean) * invstd * gamma + beta); canvas[cloud, :, c_y, c_x] = feature, the rest of the canvas cleared first.
 *     wt          f32 [C + 6][64], the Linear's weight transposed;  gamma, beta f32 [64]
 *     running_mean, running_var f32 [64], num_batches_tracked int64 [1]: updated as nn.BatchNorm1d does in training mode (momentum;
 *                 the unbiased n / (n - 1) variance; += 1), all three or none (NULL)
 *     xbuf        f32 [n_rows][P][64]: x of the real rows (the rest is not written), for the backward
 *     workspace   f64 [n_rows][2][64]
 *     stat        f32 [128] = mean | invstd;  n_total int32 [1] = n
 *     feats       f32 [n_rows][64], slots int32 [n_rows][64]: the winning value and its slot -- the FIRST maximum in slot order, -1 for a
 *                 padded slot (it comes after the real ones); 0 / -1 in rows without a pillar.  torch may pick another of several tied
 *                 slots: tied rows are identical inputs (duplicate radar returns), all padded, or both at the ReLU's zero, and in each
 *                 case every parameter gradient is the same.  A NaN among the candidates wins (torch.max); the slot saved for it is
 *                 unspecified.
 *     canvas      f32 [n_clouds][64][H][W], 16-byte aligned
 *   Sums: a pillar's rows in slot order, the pillars of each of 16 contiguous row ranges (ceil(n_rows / 16) rows) ascending, the ranges
 *   ascending.  No pillar at all: canvas 0, stat 0, n_total 0, the running statistics untouched.
 * rac_pillar_train_bwd: from dcanvas [n_clouds][64][H][W]: gm = dcanvas at the pillar's cell where the saved feature > 0, routed to the
 *   saved slot; dbeta = sum gm, dgamma = sum gm * xhat (xhat of a padded winner = (0 - mean) * invstd);
 *   dx = gamma * invstd * (gm - dbeta / n - xhat * dgamma / n) on every real row; dw [64][C + 6] = sum over the real rows of dx f^T (padded
 *   rows have f = 0; they still count in n).  dw may be NULL (only dgamma / dbeta).
 *     workspace   f64 [n_rows][2][64] + [ceil(n_rows / 64)][C + 6][64]
 *   Sums: dgamma / dbeta as the forward's; dw: 64 pillar rows per workgroup (a wave takes 16 in ascending order, the four waves added in
 *   ascending order), the workgroups in ascending order.  n_total = 0: all three gradients are 0.
 *
 * Training-mode BatchNorm (+ ReLU) on channel-first f32 maps [N][C][HW]: C a multiple of 64 (at most 4096), any N, HW with N * HW >= 2.
 * A channel's N * HW values in (image, pixel) order are cut into chunks of 4096; a workgroup sums a chunk (a thread's 16 values
 * ascending, lanes by butterfly, the 4 waves ascending), a second launch adds the chunks in ascending order.  float64 sums of x and x^2
 * (exact squares): var = sum x^2 / n - mean^2 keeps 10 digits at |mean| = 1e3 std.  workspace: f64 [C][ceil(N * HW / 4096)][2].
 * rac_bn_train_stats_fwd: mean, invstd = 1 / sqrt(biased var + eps) f32 [C]; the same launch that finishes them updates running_mean
 *   and running_var (momentum; unbiased n / (n - 1)) and num_batches_tracked (int64 [1], += 1) -- all three or none (NULL).
 * rac_bn_train_apply_fwd: y = [relu]((x - mean) * invstd * gamma + beta), left to right in f32 (a NaN stays a NaN).
 * rac_bn_train_bwd: from g = dL/dy and the saved x, y, mean, invstd: gm = g where y > 0 (y NULL: gm = g -- no ReLU, or the decision
 *   was already applied, e.g. by rac_resnet_conv_dgrad's mask), xhat = (x - mean) * invstd;  dbeta = sum gm, dgamma = sum gm * xhat,
 *   dx = gamma * invstd * (gm - dbeta / n - xhat * dgamma / n).  dx may be NULL (only dgamma / dbeta); it must not alias an input. */
int rac_pillar_train_fwd(const float *voxels, const int32_t *coors, const int32_t *num_points, const float *wt, const float *gamma,
                         const float *beta, float *running_mean, float *running_var, int64_t *num_batches_tracked, float *xbuf,
                         double *workspace, float *stat, int32_t *n_total, float *feats, int32_t *slots, float *canvas, int n_rows,
                         int n_clouds, int C, int max_num_points, int F, float eps, float momentum, float vs_x, float vs_y, float vs_z,
                         float center_x, float center_y, float center_z, int H, int W, void *stream);
int rac_pillar_train_bwd(const float *dcanvas, const float *voxels, const int32_t *coors, const int32_t *num_points, const float *gamma,
                         const float *xbuf, const float *stat, const int32_t *n_total, const float *feats, const int32_t *slots,
                         double *workspace, float *dw, float *dgamma, float *dbeta, int n_rows, int n_clouds, int C, int max_num_points,
                         int F, float vs_x, float vs_y, float vs_z, float center_x, float center_y, float center_z, int H, int W,
                         void *stream);
int rac_bn_train_stats_fwd(const float *x, double *workspace, float *mean, float *invstd, float *running_mean, float *running_var,
                           int64_t *num_batches_tracked, int N, int C, int HW, float eps, float momentum, void *stream);
int rac_bn_train_apply_fwd(const float *x, const float *mean, const float *invstd, const float *gamma, const float *beta, float *y,
                           int N, int C, int HW, int relu, void *stream);
int rac_bn_train_bwd(const float *g, const float *x, const float *y, const float *mean, const float *invstd, const float *gamma,
                     double *workspace, float *dgamma, float *dbeta, float *dx, int N, int C, int HW, void *stream);

/* ---- DepthNet (models/necks/view_transformer_racformer.py:329-567, use_dcn=False), eval mode, BatchNorms folded by the caller:
 * a convolution for many small maps and the per-image vectors around it (csrc/depth_net.hip).  Activations between layers are
 * channel-last f32 rows: pixel (n, p) of a [BN, h, w] batch is row n * hw + p of ld floats.  All arithmetic is fp32 (the f32-input
 * MFMA: an fmaf chain over each 32 input channels of a tap, the chains added in ascending (tap, channel) order); every sum has one fixed order, nothing is atomic, nothing is read back: capturable, bitwise reproducible.
 *
 * rac_conv_small_pack_fwd: src [BN, C, hw] channel-first -> dst rows of ld_dst floats, channels c_off .. c_off + C - 1, and zeros in
 *   the c_pad channels behind them (padding a concatenation to the convolution's multiple of 32).  c_off + C + c_pad <= ld_dst.
 *
 * rac_conv_small_fwd: out = epilogue(conv(gate * in)) for one layer, described by rac_conv_small:
 *   in, ld_in      channel-last rows, the first Cin channels of each are read; ld_in >= Cin, a multiple of 4, in 16-byte aligned
 *   BN, H, W       maps and their size; a workgroup owns 64 pixels of one map x 64 output channels
 *   Cin            a multiple of 32, up to 4096 (ASPP.conv1 reads its 1024 concatenated channels in one pass)
 *   ksize          1, or 3 with padding = dilation (dilation >= 1); a tap whose offset is >= H rows or >= W columns is skipped
 *   w, ld_w        f32 [ksize * ksize][Cin][ld_w], tap ky * 3 + kx, element [tap][ci][co] = weight[co][ci][ky][kx]; ld_w a multiple
 *                  of 64 >= Cout (columns >= Cout are read and must exist; zeros by convention), 16-byte aligned
 *   Cout           output channels (any count >= 1)
 *   gate           NULL or f32 [BN][gate_channels]: input channel c < gate_channels of map n is multiplied by gate[n][c] while it is
 *                  staged (SE gating without per-image weights); gate_channels a multiple of 32 <= Cin
 *   epilogue, in this order, each part optional (NULL):  + bias[co]  + img_bias[n][co]  + bins_table[bins[pix]][co] for
 *                  0 <= bins[pix] < n_bins (table [n_bins][Cout]: a one-hot input's 1x1 term as a column lookup)
 *                  + cls_table[cls[pix] + 1][co], row 0 for a class outside 0 .. n_cls - 1 (table [n_cls + 1][Cout])
 *                  + residual[pix][co] (channel-last rows of ld_res floats)   then ReLU if relu != 0; a NaN stays a NaN
 *                  (as torch.relu keeps it)
 *   out            RAC_CS_CHANNEL_LAST: rows of ld_out floats, channels c_off .. c_off + Cout - 1 (the next layer's operand: a
 *                  concatenation is written in place, never copied);  RAC_CS_CHANNEL_FIRST: [BN][ld_out][hw], channels from c_off
 *   Any violation is RAC_E_ARG before any launch.
 *
 * rac_depthnet_gates_fwd: gates [branches][BN][C] = sigmoid(We relu(Wr (W2 relu(W1 x + b1) + b2) + br) + be) for x = mlp_input[n]
 *   (f32 [BN][9]; the BatchNorm1d in front folded into W1, b1): Mlp and the SE tail of one DepthNet branch per params block
 *   (a NaN passes both ReLUs: a NaN in mlp_input[n] makes every gate of map n NaN)
 *   w1t [9][C] | b1 [C] | w2t [C][C] | b2 [C] | wrt [C][C] | br [C] | wet [C][C] | be [C], matrices [in][out]; C <= 1024.
 *
 * rac_depthnet_pool_bias_fwd: ASPP's image-pool branch as a per-image bias of ASPP.conv1: m = mean over the hw rows of map n of x
 *   (channel-last rows of ld floats, C channels; up to 1024 / C pixel segments summed in ascending order, then added in ascending
 *   order), y = relu(wpool_t^T m + bpool) (a NaN stays a NaN), img_bias[n][co] = sum_k wbias_t[k][co] y[k].  wpool_t [C][C],
 *   wbias_t [C][Cout], [in][out]; C <= 1024. */
enum { RAC_CS_CHANNEL_LAST = 0, RAC_CS_CHANNEL_FIRST = 1 };
typedef struct {
    const float *in;
    const float *w;
    const float *bias;
    const float *img_bias;
    const float *gate;
    const float *residual;
    const int32_t *bins;
    const float *bins_table;
    const int32_t *cls;
    const float *cls_table;
    float *out;
    int BN, H, W, Cin, Cout, ksize, dilation;
    int ld_in, ld_w, gate_channels, ld_res, n_bins, n_cls, relu, out_layout, ld_out, c_off;
} rac_conv_small;
int rac_conv_small_pack_fwd(const float *src, float *dst, int BN, int C, int hw, int ld_dst, int c_off, int c_pad, void *stream);
int rac_conv_small_fwd(const rac_conv_small *d, void *stream);
int rac_depthnet_gates_fwd(const float *mlp_input, const float *params, float *gates, int BN, int C, int branches, void *stream);
int rac_depthnet_pool_bias_fwd(const float *x, const float *wpool_t, const float *bpool, const float *wbias_t, float *img_bias, int BN,
                               int hw, int ld, int C, int Cout, void *stream);

/* ---- The image backbone: mmdet ResNet with Bottleneck blocks (depth 50 / 101 / 152, style 'pytorch'), eval mode, BatchNorms folded
 * by the caller (csrc/resnet.hip).  Every tensor is channel-first f32; no atomics, every sum in one fixed order, nothing read back,
 * launch geometry from the shapes alone: capturable, bitwise reproducible.
 *
 * rac_resnet_stem_fwd: out = maxpool3x3/2/1(relu(conv7x7/2/3(norm(img)) + bias)), exact fp32 (an fmaf chain over (ci, ky, kx)).
 *   img     device f32 [N][3][H][W], any H, W >= 1
 *   w       device f32 [147][64]: element [(ci * 7 + ky) * 7 + kx][co] = folded weight[co][ci][ky][kx]; 16-byte aligned
 *   bias    device f32 [64], the folded BatchNorm shift
 *   norm    != 0: the convolution reads (img[:, perm[c]] - mean[c]) / std[c] as its channel c (subtract, then an IEEE float32 division,
 *           element by element; the zero padding stays zero)
 *   conv    device f32 scratch [N][64][Hc][Wc], Hc = (H + 6 - 7) / 2 + 1 (the convolution's output; two launches)
 *   out     device f32 [N][64][Hp][Wp], Hp = (Hc + 2 - 3) / 2 + 1; a pool window over the border takes the maximum of its valid pixels
 *
 * rac_resnet_absmax_fwd: parts[n][0..63] = maxima of |x| over 64 slices of image n (x: [N] images of per_image floats).  Fixes the
 *   power-of-two activation scale of rac_resnet_conv_fwd, which combines the 64 values itself.
 *
 * rac_resnet_conv_fwd: one convolution of a Bottleneck with its folded BatchNorm and epilogue,
 *     out[n][co][q] = [relu]( sum W[co][ci][ky][kx] * in[n][ci][stride * q + (ky, kx) - pad] + bias[co] [+ residual[n][co][q]] )
 *   ksize 1 (pad 0) or 3 (pad 1); stride 1 or 2; Cin a multiple of 32, Cout a multiple of 64, both at most 2048; any H, W >= 1,
 *   Ho = (H + 2 pad - ksize) / stride + 1
 *   in         device f32 [N][Cin][H*W];  out, residual (or NULL): device f32 [N][Cout][Ho*Wo]
 *   w_image    device f16 line image [Cout][ksize*ksize*Cin/32][hi 32 | lo 32] of weight * 2^s (rac_gemm_split_pack_fwd on the weight
 *              as [Cout][K], K index = (ky * ksize + kx) * Cin + ci); w_alpha = 2^-s; 16-byte aligned
 *   bias       device f32 [Cout] or NULL;  amax_parts: rac_resnet_absmax_fwd of `in` (it must bound every image)
 *   Split-precision f16 MFMA (hi / lo per operand, three products, fp32 accumulate), activation scale per image. */
typedef struct {
    const float *img;
    const float *w;
    const float *bias;
    float *conv;
    float *out;
    int N, H, W, norm;
    int perm[3];
    float mean[3];
    float std[3];
} rac_resnet_stem;
typedef struct {
    const float *in;
    const void *w_image;
    const float *bias;
    const float *residual;
    const float *amax_parts;
    float *out;
    float w_alpha;
    int N, H, W, Cin, Cout, ksize, stride, relu;
} rac_resnet_conv;
int rac_resnet_stem_fwd(const rac_resnet_stem *d, void *stream);
int rac_resnet_absmax_fwd(const float *x, float *parts, int N, int64_t per_image, void *stream);
int rac_resnet_conv_fwd(const rac_resnet_conv *d, void *stream);

/* ---- Backward of one Bottleneck convolution (csrc/resnet_bwd.hip): what training through the backbone needs behind the frozen stem.
 * BatchNorms stay folded (norm_eval: the forward under autograd is the folded convolution); W below is the FOLDED weight, the caller
 * turns dW / db into the gradients of the convolution weight and the BatchNorm affine (resnet.fold_bn_backward).  Channel-first f32, no
 * float atomics, every sum in one fixed order, launch geometry from the shapes alone, nothing read back; every argument is checked
 * before any launch.  Sizes: H x W is the convolution's INPUT map, Ho x Wo its output, Ho = (H + 2 pad - ksize) / stride + 1 (both are
 * arguments and must agree: 7 and 8 both map to 4); ksize 1 (pad 0) or 3 (pad 1); stride 1 or 2; any H, W >= 1.
 *
 * rac_resnet_conv_dgrad: the data gradient with the backward's element-wise work in its epilogue,
 *     out[n][ci][p] = M( sum_{co,ky,kx} W[co][ci][ky][kx] * g[n][co][q] [+ add[n][ci][p]] ),  stride * q + (ky, kx) - pad == p
 *   Cin a multiple of 64, Cout a multiple of 32, both at most 2048
 *   g          device f32 [N][Cout][Ho*Wo];  out, add (or NULL), mask (or NULL): device f32 [N][Cin][H*W]
 *   w_image    device f16 line image [Cin][ksize*ksize*Cout/32][hi 32 | lo 32] of W^T * 2^s: rac_gemm_split_pack_fwd on [Cin][K] with
 *              K index = ((ksize - 1 - ky) * ksize + (ksize - 1 - kx)) * Cout + co (the taps flipped); w_alpha = 2^-s; 16-byte aligned
 *   amax_parts rac_resnet_absmax_fwd of g (one power-of-two scale per image, as in the forward)
 *   add        the identity branch or an outside gradient, added before the mask
 *   mask       the convolution's own post-ReLU input: an element with mask <= 0 is +0 exactly (the ReLU backward of the layer in front)
 *   Split-precision f16 MFMA (hi / lo per operand, three products, fp32 accumulate).
 *
 * rac_resnet_conv_wgrad: dW[co][ci][ky][kx] = sum_{n,q} g[n][co][q] * x[n][ci][stride * q + (ky, kx) - pad],  db[co] = sum_{n,q} g[n][co][q]
 *   Cout a multiple of 64, Cin a multiple of 32, both at most 2048
 *   g          device f32 [N][Cout][Ho*Wo];  x device f32 [N][Cin][H*W]
 *   dw         device f32 [Cout][Cin][ksize][ksize];  db device f32 [Cout] or NULL
 *   k_splits   K = N * Ho * Wo in units of 32 pixels of one image (N * ceil(Ho * Wo / 32) units) is cut into k_splits contiguous
 *              ranges of ceil(units / k_splits) units; 1 <= k_splits <= units and no range may be empty
 *   workspace  device f32 [k_splits][ksize*ksize][Cout][Cin] + [k_splits][Cout]: the ranges' partial sums, added in ascending range
 *              order by a second launch.  Bitwise reproducible for equal k_splits.
 *   Both operands split f16, one power-of-two scale per channel and K range.
 *
 * rac_resnet_relu_bwd: out[i] = y[i] > 0 ? a[i] [+ b[i]] : +0 for count elements (b may be NULL; out may alias a or b). */
typedef struct {
    const float *g;
    const void *w_image;
    const float *add;
    const float *mask;
    const float *amax_parts;
    float *out;
    float w_alpha;
    int N, H, W, Ho, Wo, Cin, Cout, ksize, stride;
} rac_resnet_dgrad;
int rac_resnet_conv_dgrad(const rac_resnet_dgrad *d, void *stream);
int rac_resnet_conv_wgrad(const float *g, const float *x, float *workspace, float *dw, float *db, int N, int Cin, int H, int W, int Cout,
                          int Ho, int Wo, int ksize, int stride, int k_splits, void *stream);
int rac_resnet_relu_bwd(const float *y, const float *a, const float *b, float *out, int64_t count, void *stream);

/* The streaming detector's window gather (csrc/frames.hip; racformer_amd/detector.py, RaCFormer.simple_test_online): the front end's
 * per-frame outputs live in one ring of n_slots frames per tensor kind, the decoder reads T frames of every kind as one contiguous
 * window.  For every tensor k < n_tensors and frame t < T:
 *     outs[k][t * frame_bytes[k] ..] = rings[k][slots[t] * frame_bytes[k] ..]          (frame_bytes[k] bytes)
 *   rings, outs : HOST arrays of n_tensors device pointers, 16-byte aligned; ring k holds n_slots frames, out k holds T frames
 *   frame_bytes : HOST int64 [n_tensors], positive multiples of 16 (a frame of the pyramid in the sampling layout at B = 1 is one
 *                 contiguous block [G, N, H, W, 64] of rac_fpn_conv_fwd's output; a BEV frame is [C, Y, X])
 *   slots       : HOST int32 [T], each in [0, n_slots); repeated slots are allowed
 * All tables travel as kernel arguments: no device table, no upload, no synchronisation, no allocation -- capturable.  One launch for
 * all tensors, 16 bytes per lane on both sides, workgroups divided among the tensors in proportion to their bytes.
 * Limits: n_tensors <= 8, T <= 16.  Refused with RAC_E_ARG before any HIP call: a null pointer, a frame_bytes that is not a positive
 * multiple of 16, a misaligned pointer, a slot outside [0, n_slots), n_tensors or T out of range. */
int rac_frames_gather(int n_tensors, const void *const *rings, void *const *outs, const int64_t *frame_bytes, const int32_t *slots,
                      int T, int n_slots, void *stream);

/* The training step's parameter update (csrc/optimizer.hip; racformer_amd/optim.py, FusedAdamW): torch.optim.AdamW (amsgrad=False,
 * maximize=False) after clip_grad_norm_(norm_type=2) over a list of float32 tensors, in three launches on `stream` -- no atomics, no
 * grid-wide barrier, no read-back, no allocation: capturable, and bitwise reproducible wherever the tensors lie.
 *
 * A CHUNK is RAC_OPT_CHUNK consecutive elements of one tensor (a tensor's last chunk is short; no chunk spans two tensors).  The
 * constant is part of the definition of the norm's summation order: per chunk a fixed tree in float64 (squares of float32 are exact
 * there), then the chunks' partial sums in index order in a fixed tree.  Neither depends on the grid, the device or the alignment.
 *   tensors  : DEVICE [n_tensors] rac_opt_tensor -- the tensors that take part in this step: p (updated), g (read only, left
 *              unclipped), m / v (exp_avg / exp_avg_sq, updated), numel >= 1, and `row`, the tensor's row in hyper / steps / scalars
 *              (rows are distinct; a tensor keeps its row from step to step whether or not it takes part).  Pointers are 4-byte
 *              aligned; accesses are 16 bytes wide where a pointer is 16-byte aligned, scalar otherwise and at a tensor's tail
 *   chunks   : DEVICE [n_chunks] rac_opt_chunk -- tensor index and start element (a multiple of RAC_OPT_CHUNK, below numel) of
 *              every chunk, tensors in table order, chunks of a tensor in ascending order
 *   hyper    : DEVICE double [rows, RAC_OPT_HYPER] -- lr, weight_decay, beta1, beta2, eps, 0 per row; read by the finish launch of
 *              every step, so a scheduler changes a learning rate by writing here
 *   steps    : DEVICE float [rows] -- per-tensor step counters (torch keeps them as float32 too); + 1 for the present tensors
 *              unless the step is skipped
 *   scalars  : DEVICE float [rows, RAC_OPT_SCALARS] -- written by the finish launch for the present tensors, each computed in
 *              float64 and rounded once: 1 - lr wd, lr / (1 - beta1^t), sqrt(1 - beta2^t), 1 - beta1, beta2, 1 - beta2, eps, 0
 *   partials : DEVICE double [n_chunks] scratch
 *   record   : DEVICE rac_opt_record -- total_sq (sum of the squares of all gradients), total_norm (its root), clip_coef =
 *              min(1, max_norm / (total_norm + 1e-6)) (1 when max_norm < 0: no clipping), skip = the total is not finite.  When
 *              skip is set nothing else is written: no counter, no scalar, no element of p, m or v
 *   phases   : mask of RAC_OPT_NORM | RAC_OPT_FINISH | RAC_OPT_UPDATE, the launches to enqueue (a step is RAC_OPT_ALL; single
 *              phases are for timing)
 * Per element (every operation rounded once, division and square root correctly rounded), with the row's scalars:
 *     g' = g clip_coef;  p = p (1 - lr wd);  m = m + (g' - m)(1 - beta1);  v = beta2 v + ((1 - beta2) g') g'
 *     p = p - (lr / bc1) (m / (sqrt(v) / sqrt(bc2) + eps))
 * Departure from torch: the clip is folded into the update, g itself is not written.
 * Refused with RAC_E_ARG before any HIP call: a null or misaligned table pointer, n_tensors < 1, n_chunks < n_tensors, phases out
 * of range, max_norm nan.  The tables' CONTENTS are the caller's responsibility (device memory is not inspected). */
#define RAC_OPT_CHUNK 16384
#define RAC_OPT_HYPER 6
#define RAC_OPT_SCALARS 8
enum { RAC_OPT_NORM = 1, RAC_OPT_FINISH = 2, RAC_OPT_UPDATE = 4, RAC_OPT_ALL = 7 };
typedef struct {
    float *p;
    const float *g;
    float *m;
    float *v;
    int64_t numel;
    int32_t row;
    int32_t reserved;
} rac_opt_tensor;
typedef struct {
    int64_t start;
    int32_t tensor;
    int32_t reserved;
} rac_opt_chunk;
typedef struct {
    double total_sq;
    double total_norm;
    float clip_coef;
    int32_t skip;
} rac_opt_record;
int rac_adamw_step(const rac_opt_tensor *tensors, int n_tensors, const rac_opt_chunk *chunks, int n_chunks, const double *hyper,
                   float *steps, float *scalars, double *partials, rac_opt_record *record, float max_norm, int phases, void *stream);

/* Point clouds to per-view maps (csrc/point_maps.hip; racformer_amd/point_maps.py): what the reference's data pipeline
 * makes on the CPU -- radar_depth / radar_rcs from the radar clouds, gt_depth from the lidar cloud -- made on the device from the
 * packed clouds of the radar pillar ABI.  Nothing is read back, launches are sized by the shapes alone, no allocation: capturable;
 * winners are chosen by 64-bit integer atomic min / max, so two runs give the same bits.
 *   points        : DEVICE float [n_points, C], C >= 3: x, y, z and further columns
 *   cloud_offsets : DEVICE int32 [n_clouds + 1], ascending from 0 to n_points (rac_pillar_voxelize_fwd's table)
 *   mats          : DEVICE float [n_clouds * n_views, 12]: rows 0..2 of the 4x4 lidar2img of map m = cloud * n_views + view
 *   H, W, ds      : the image size and the downsample; the map is hm x wm = H / ds x W / ds (integer division)
 *   Hp, Wp        : the outputs' row count and row length, Hp >= hm, Wp >= wm; outputs are [n_clouds * n_views, Hp, Wp], every element
 *                   is written, rows >= hm and columns >= wm as +0.0.  Outputs are 4-byte aligned; stores are 16 bytes wide where
 *                   the address allows it, scalar otherwise
 *   scratch       : DEVICE uint64 [scratch_words], 8-byte aligned, contents arbitrary before and after.  Needed: radar
 *                   2 * n_clouds * n_views * wm words, lidar n_clouds * n_views * hm * wm words
 * Per cloud and view (float32, every operation rounded once, left to right, IEEE division):
 *   p_i = x M[i][0] + y M[i][1] + z M[i][2] + M[i][3];  u = p_0 / p_2, v = p_1 / p_2, d = p_2;  cx = rint(u / ds), cy = rint(v / ds)
 *   kept: 0 <= cx < wm, 0 <= cy < hm, lo <= d < hi (NaN, inf and p_2 = 0 fail);  key k = (cx + cy wm) + d / 100
 *   a pixel's winner is the kept point with the smallest (k, index in the cloud)
 *   lidar: gt_depth[cy][cx] = d of the pixel's winner, 0 elsewhere
 *   radar: every row of column cx = the value of the column's pixel winner with the largest cy, 0 for a column without one;
 *          radar_depth gets the winner's d, radar_rcs gets points[s][rcs_col] where s is the winner's POSITION AMONG THE CLOUD'S KEPT
 *          POINTS for this view in input order (the reference's indexing, kept as it is); either output may be NULL
 * RAC_E_ARG before any HIP call: a null or misaligned pointer, C < 3, ds < 1, H < ds or W < ds, Hp < hm or Wp < wm, rcs_col outside
 * [0, C), a scratch that is too small, more than 65535 maps.  RAC_E_UNSUPPORTED before any HIP call: hm * wm > 2^18, hi > 99 or
 * lo <= 0 (the key's rounding could reach the next pixel's rank, or a key could be negative), n_points >= 2^20, hm > 4096. */
int rac_point_maps_radar_fwd(const float *points, const int32_t *cloud_offsets, const float *mats, float *radar_depth, float *radar_rcs,
                             uint64_t *scratch, int64_t scratch_words, int n_points, int n_clouds, int n_views, int C, int rcs_col, int H,
                             int W, int Hp, int Wp, int ds, float lo, float hi, void *stream);
int rac_point_maps_lidar_fwd(const float *points, const int32_t *cloud_offsets, const float *mats, float *gt_depth, uint64_t *scratch,
                             int64_t scratch_words, int n_points, int n_clouds, int n_views, int C, int H, int W, int Hp, int Wp, int ds,
                             float lo, float hi, void *stream);

/* Raw camera frames to the detector's images (csrc/image_geom.hip; racformer_amd/image_geom.py): the resize, crop and
 * left-right flip of the reference's RandomTransformImage as Pillow's 8-bit bicubic resampler computes them, for all images of all
 * samples in ONE launch.  Integer arithmetic only, nothing read back, sized by the shapes, no atomics, no allocation: capturable, the
 * same bits on every run.  raw is only read; every output element is written exactly once.
 *   raw         : DEVICE uint8 [n_images, Hr, Wr, 3], any byte alignment
 *   group       : consecutive images that share one table (one sample's draw); n_images is a multiple of it
 *   tables      : DEVICE int32 [n_images / group, words], 4-byte aligned; tables_host: the same words in HOST memory, read before the
 *                 call returns (every bound is checked there, so the kernel cannot read outside raw).  With ntx = ceil(fW / 64) and
 *                 nty = ceil(fH / 16), one group's words are, in this order:
 *                   column bounds [fW][2]   : output column ox reads raw columns [first, first + count); count = 0: it is 0
 *                   row bounds    [fH][2]   : the same for output row oy and raw rows
 *                   column spans  [ntx][2]  : [lo, hi) covers the reads of output columns 64 i .. 64 i + 63 (0, 0 for none)
 *                   row spans     [nty][2]  : the same for output rows 16 i .. 16 i + 15
 *                   column weights [fW][ksize], row weights [fH][ksize] : 22-bit fixed point, entries past the count unused
 *   out         : DEVICE, out_kind RAC_IG_F32_CHW: float [n_images, 3, fH, fW], the integers 0 .. 255; RAC_IG_U8_HWC: uint8
 *                 [n_images, fH, fW, 3].  The channel order is raw's.
 * Per channel: h(r, ox) = clip8((2^21 + sum_t raw[r][first_x + t] * wx[ox][t]) >> 22) for the raw rows r an output row reads, then
 * out(oy, ox) = clip8((2^21 + sum_t h(first_y + t, ox) * wy[oy][t]) >> 22); int32 sums (the caller's weights keep them below 2^31).
 * RAC_E_ARG before any HIP call: a null pointer, a misaligned table or float output, a size <= 0, n_images > 65535 or not a multiple of
 * group, a bound outside raw or outside its tile's span, a count above ksize.  RAC_E_UNSUPPORTED before any HIP call, nothing is
 * launched: ksize > 16, a column span above 212 raw columns or a row span above 64 raw rows (the LDS tile chosen at compile time; a
 * down-scale by more than about 3). */
enum { RAC_IG_F32_CHW = 0, RAC_IG_U8_HWC = 1 };
int rac_image_geom_fwd(const uint8_t *raw, const int32_t *tables, const int32_t *tables_host, void *out, int n_images, int group, int Hr,
                       int Wr, int fH, int fW, int ksize, int out_kind, void *stream);

/* The scene's rotation about z and isotropic scaling (csrc/bev_aug.hip; racformer_amd/bev_aug.py): what the reference's
 * RaCGlobalRotScaleTransImage does to the lidar cloud, the radar clouds and the ground-truth boxes through mmdet3d's rotate / scale,
 * for all samples of a step in ONE launch.  No trigonometric function on the device, nothing read back, the grid sized by the chunk
 * table, no atomics, no allocation: capturable, the same bits on every run and at every address.
 *   segs    : DEVICE [n_segs] rac_bev_seg -- src (read) and dst (written) float [rows, cols], rows back to back, 4-byte aligned; kind
 *             RAC_BEV_POINTS (3 <= cols <= RAC_BEV_MAX_COLS) or RAC_BEV_BOXES (cols 7 or 9: x, y, z of the bottom centre, w, l, h, yaw
 *             and, with 9, vx, vy); sample: the row of `draws` the segment uses.  rows may be 0.  dst == src is allowed (a lane reads its
 *             row whole before it writes it); any other overlap of a dst with a src or with another dst is refused
 *   chunks  : DEVICE [n_chunks] rac_bev_chunk -- segment and first row of every RAC_BEV_CHUNK rows of every segment, segments in
 *             table order, a segment's chunks ascending (the last one short); one workgroup per chunk, one row per lane
 *   segs_host, chunks_host : the same tables in HOST memory, read before the call returns: everything below is checked there, so the
 *             kernel cannot touch a row no segment names
 *   draws   : DEVICE float [n_samples, 4] -- c, s, a, r per sample: cos and sin of the angle as the host computed them, the angle and
 *             the scale ratio, all float32.  Read by the launch, so a captured launch takes new draws from a rewritten table
 * Per row, float32, every operation rounded once, nothing contracted into a fused multiply-add, left to right:
 *   points: x' = ((x c + y (-s)) + z 0) r;  y' = ((x s + y c) + z 0) r;  z' = ((x 0 + y 0) + z 1) r;  columns >= 3 copied bit for bit
 *           (the products by 0 stay: they carry a NaN or inf coordinate into the other two, as the reference's matmul does)
 *   boxes : the centre as a point; w, l, h times r; yaw' = yaw + a (not re-limited); vx' = (vx c + vy (-s)) r, vy' = (vx s + vy c) r
 * n_chunks == 0 (every segment empty) launches nothing.  RAC_E_ARG before any HIP call: a null or misaligned pointer, n_segs outside
 * [1, 1024], n_samples < 1, rows < 0, rows * cols >= 2^31, cols or kind or sample out of range, overlapping segments, a chunk table that
 * is not the one described above. */
enum { RAC_BEV_POINTS = 0, RAC_BEV_BOXES = 1 };
#define RAC_BEV_CHUNK 256
#define RAC_BEV_MAX_COLS 16
typedef struct {
    const float *src;
    float *dst;
    int32_t rows;
    int32_t cols;
    int32_t kind;
    int32_t sample;
} rac_bev_seg;
typedef struct {
    int32_t seg;
    int32_t row0;
} rac_bev_chunk;
int rac_bev_aug_fwd(const rac_bev_seg *segs, const rac_bev_chunk *chunks, const rac_bev_seg *segs_host, const rac_bev_chunk *chunks_host,
                    const float *draws, int n_segs, int n_chunks, int n_samples, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* RACFORMER_HIP_H */
