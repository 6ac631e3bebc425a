/* libdynaboa_hip.so - C ABI of the MI355X (gfx950) kernels behind DynaBOA's per-frame adaptation
 * hot path.
 *
 * The reference (syguan96/DynaBOA) has no FFI: its boundary for this path is the Python object
 * surface (hmr()/HMR.forward, SMPL.forward, MAML.clone/adapt, torch.optim.Adam, BaseAdaptor.*;
 * SURVEY.md 8b).  dynaboa_amd/ reproduces that surface in Python and calls down into the entry
 * points below; each one names the reference code whose arithmetic it replaces.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer to fp32 unless stated otherwise; the library never
 *     allocates, frees or retains caller memory; scratch is passed in (`ws`, size from the
 *     matching *_workspace_bytes);
 *   - everything is enqueued on `stream` in order; no call synchronises the host - with ONE exception, stated where it occurs:
 *     dyb_stepper_adapt_frame_full / _frames_full with the dynamic-BOA gate on poll device-written pinned memory once per gate
 *     check (the reference's `.item()`, dynaboa_benchmark.py:165) to decide which sequences take a further step;
 *   - return value: 0 = ok, -1 bad argument, -2 launch failure, -3 unsupported shape,
 *     -4 workspace too small;
 *   - one host thread per GPU process; re-entrant across different streams + workspaces.
 *   - `const T* const*` arguments are HOST arrays of device pointers;
 *   - activations are NHWC, conv weights [R][S][Cin][Cout] (Cin padded to >= 4), linear weights
 *     (out, in) row-major with the row stride padded to a multiple of 4 floats.
 */
#ifndef DYNABOA_HIP_H
#define DYNABOA_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ihipStream_t* dyb_stream_t; /* == hipStream_t */

/* ---- convolution (implicit GEMM on fp32 MFMA) ------------------------------------------------
 * replaces nn.Conv2d(bias=False) forward and its autograd in the ResNet-50 backbone:
 * reference model/hmr.py:28-33,40-56 (Bottleneck), :70,110-114,138 (stem / downsample). */
size_t dyb_conv2d_workspace_bytes(int N, int H, int W, int C, int K, int R, int S, int stride, int pad);
int dyb_conv2d_nhwc_fwd(const float* x, const float* w, float* y, int N, int H, int W, int C, int K, int R, int S,
                        int stride, int pad, void* ws, size_t ws_bytes, dyb_stream_t stream);
int dyb_conv2d_nhwc_dgrad(const float* dy, const float* w, float* dx, const float* addend, int N, int H, int W, int C,
                          int K, int R, int S, int stride, int pad, void* ws, size_t ws_bytes, dyb_stream_t stream);
int dyb_conv2d_nhwc_wgrad(const float* x, const float* dy, float* dw, int N, int H, int W, int C, int K, int R, int S,
                          int stride, int pad, void* ws, size_t ws_bytes, dyb_stream_t stream);

/* ---- GroupNorm(4 groups, eps 1e-5) + optional residual add + optional ReLU --------------------
 * replaces nn.GroupNorm(32//8, C) (reference model/hmr.py:14-18), nn.ReLU and `out += residual`
 * (:43-58).  `slabs`/`nslabs` let the kernel fold split-K partial sums of the preceding conv.
 * stats = [N][4][2] (mean, rstd) saved for backward. */
size_t dyb_groupnorm_workspace_bytes(int N, int HW, int C);
int dyb_groupnorm_fwd(const float* slabs, int nslabs, float* y, const float* gamma, const float* beta,
                      const float* residual, float* out, float* stats, int N, int HW, int C, int relu, void* ws,
                      size_t ws_bytes, dyb_stream_t stream);
int dyb_groupnorm_bwd(const float* dout, const float* out, const float* y, const float* stats, const float* gamma,
                      float* dy, float* dres, float* dgamma, float* dbeta, int N, int HW, int C, int relu, void* ws,
                      size_t ws_bytes, dyb_stream_t stream);

/* as dyb_groupnorm_bwd, but the incoming gradient is sum_z dout_slabs[z*slab_stride + .] (+ addend),
 * i.e. the un-folded split-K slabs of the data-gradient convolution that produced it plus the
 * residual-edge gradient; the sum is formed once inside the reduce kernel and written to `folded`. */
int dyb_groupnorm_bwd_fold(const float* dout_slabs, int nslabs, size_t slab_stride, const float* addend, float* folded,
                           const float* out, const float* y, const float* stats, const float* gamma, float* dy,
                           float* dres, float* dgamma, float* dbeta, int N, int HW, int C, int relu, void* ws,
                           size_t ws_bytes, dyb_stream_t stream);

/* One-pass GroupNorm backward of ONE image (the throughput schedule's form: one image per sequence replica; replaces
 * nn.GroupNorm's autograd, reference model/hmr.py:14-18): every input is read once and every output written once - a workgroup
 * keeps its rows of an (image, group) slab in registers between the sums and the apply; slabs beyond `cap` float4 per workgroup
 * (0: the policy's, 2048) are cut into up to 32 row chunks whose workgroups meet on a counter inside `ws`.  Incoming gradient = sum_z
 * dout_slabs[z*slab_stride + .] (+ addend); out = the saved activation (ReLU mask) or NULL: the mask is recomputed from y
 * (beta required); dm (may be NULL) receives the masked gradient.  DYB_ERR_UNSUPPORTED when the shape does not qualify
 * (C a power of two in 64..2048, a slab of at most 32 chunks). */
size_t dyb_groupnorm_bwd_onepass_workspace_bytes(int HW, int C);
int dyb_groupnorm_bwd_onepass(const float* dout_slabs, int nslabs, size_t slab_stride, const float* addend, const float* out,
                              const float* y, const float* stats, const float* gamma, const float* beta, float* dm, float* dy,
                              float* dgamma, float* dbeta, int HW, int C, int relu, int cap, void* ws, size_t ws_bytes,
                              dyb_stream_t stream);

/* GroupNorm backward split for consumers that form dy on the fly: the reduce half alone.  dm = dout
 * masked by the ReLU (relu == 0: pass dm == dout, nothing is copied); `part`
 * (dyb_groupnorm_bwd_partial_floats floats) receives the per-channel / per-group partial sums.  The
 * two convolution gradients below consume (dm, y_gn, stats, part, gamma) in their operand loaders -
 * dy = rstd*(gamma*dm - c1 - xhat*c2) never exists in memory - and the weight-gradient launch also
 * writes dgamma / dbeta.  Same autograd as dyb_groupnorm_bwd + dyb_conv2d_nhwc_dgrad/_wgrad, one
 * dependent launch less per layer (the engine's critical chain is launch-latency-bound at batch 1). */
size_t dyb_groupnorm_bwd_partial_floats(int N, int HW, int C);
int dyb_groupnorm_bwd_reduce(const float* dout, const float* out, const float* y, const float* stats,
                             const float* gamma, const float* beta, float* dm, float* part, int N, int HW, int C,
                             int relu, dyb_stream_t stream);
int dyb_conv2d_nhwc_dgrad_gn(const float* dm, const float* y_gn, const float* stats, const float* part,
                             const float* gamma, const float* w, float* dx, const float* addend, int N, int H, int W,
                             int C, int K, int R, int S, int stride, int pad, void* ws, size_t ws_bytes,
                             dyb_stream_t stream);
int dyb_conv2d_nhwc_wgrad_gn(const float* x, const float* dm, const float* y_gn, const float* stats, const float* part,
                             const float* gamma, float* dw, float* dgamma, float* dbeta, int N, int H, int W, int C,
                             int K, int R, int S, int stride, int pad, void* ws, size_t ws_bytes, dyb_stream_t stream);

/* GroupNorm forward split the same way.  dyb_groupnorm_stats: the statistics half alone (partials =
 * dyb_groupnorm_workspace_bytes(N,HW,C) bytes).  dyb_groupnorm_apply: the apply half; its residual may be
 * NULL, plain, or (res_partials != NULL) the GroupNorm without ReLU of a raw conv output - the
 * shortcut branch's downsample.1 (model/hmr.py:66-70) - normalised on the fly.
 * dyb_conv2d_nhwc_fwd_gnin: y = conv(relu?(gn(y_prev))) with the producer's GroupNorm applied in the
 * operand loader from its partials (inside a bottleneck, model/hmr.py:43-52, bn1/bn2 outputs have a
 * single consumer and are never written); dyb_conv2d_nhwc_wgrad_gn_gnin is the matching weight gradient. */
int dyb_groupnorm_stats(const float* slabs, int nslabs, float* y, float* partials, int N, int HW, int C,
                        dyb_stream_t stream);
int dyb_groupnorm_apply(const float* y, const float* partials, const float* gamma, const float* beta,
                        const float* residual, const float* res_partials, const float* res_gamma, const float* res_beta,
                        float* res_stats, float* out, float* stats, int N, int HW, int C, int relu, dyb_stream_t stream);
int dyb_conv2d_nhwc_fwd_gnin(const float* y_prev, const float* part_prev, const float* gamma_prev, const float* beta_prev,
                             int relu_prev, float* stats_prev_out, const float* w, float* y, int N, int H, int W, int C,
                             int K, int R, int S, int stride, int pad, void* ws, size_t ws_bytes, dyb_stream_t stream);
int dyb_conv2d_nhwc_wgrad_gn_gnin(const float* y_prev, const float* stats_prev, const float* gamma_prev,
                                  const float* beta_prev, int relu_prev, const float* dm, const float* y_gn,
                                  const float* stats, const float* part, const float* gamma, float* dw, float* dgamma,
                                  float* dbeta, int N, int H, int W, int C, int K, int R, int S, int stride, int pad,
                                  void* ws, size_t ws_bytes, dyb_stream_t stream);

/* Measurement aid for bench.py's roofline leg: between _begin and _end every convolution kernel launched
 * from the calling thread is timed on its own dispatch (start/stop events on the launch, no extra stream
 * packets).  _end (after a device synchronise) returns the summed kernel time, the launch count and the
 * algorithmic flop / bytes those launches stand for. */
int dyb_conv_timing_begin(int max_launches);
int dyb_conv_timing_end(double* ms_total, long long* launches, double* flop, double* bytes);
/* Per-shape breakdown of the scope closed last, as CSV text (header line first; kind f/d/w (t/u/v: throughput form) = tiled forward / data gradient /
 * weight gradient kernel, F/D = the single-launch 1x1 kernels).  Copies at most cap-1 bytes + terminator into buf; returns
 * the size needed.  tools/conv_table.py prints it. */
size_t dyb_conv_timing_table(char* buf, size_t cap);
double dyb_conv_timing_union_ms(void); /* of the scope closed last: time during which at least one timed launch was executing */
/* Diagnostic: while set (buf != NULL), launches of the throughput-form conv kernel whose mode (0 forward, 1 data gradient,
 * 2 weight gradient) and layer (H, C, K, R) match write per-wave phase clocks into buf ([workgroup][4 waves][8] 64-bit words,
 * cap_wgs workgroups of room; layout in igemm_conv.hip).  bench.py --probe / tools/tp_probe.py read it.  buf = NULL clears. */
int dyb_conv_probe_set(void* buf, long cap_wgs, int mode, int H, int C, int K, int R);

/* ---- second-order building blocks (exact Hessian-vector products, hvp_kernels.hip / hvp_engine.inc) ----
 * Tangent ("t" prefix = directional derivative along a parameter direction) of GroupNorm(4, C)(+ReLU)(+residual) and of its
 * backward; NHWC [N][HW][C]; stats = the forward's [N][4][2] (mean, rstd); tstats [N][4][2] receives / supplies the tangent
 * statistics.  out may be NULL.  ty2 (may be NULL): a second half of the tangent, added into ty first (the two halves of a
 * convolution's tangent).  dyb_gn_jvp_bwd: dout / tdout = gradient w.r.t. the layer's output and its tangent, out_mask =
 * the primal output (ReLU mask, relu = 1); writes the masked gradients (dm, tdm; may be NULL), the gradient w.r.t. y and its
 * tangent (dy, tdy) and the tangents of dgamma / dbeta ([C]).  scratch: dyb_gn_jvp_scratch_floats(N, HW, C) floats, 8-byte aligned
 * (each (image, group) slab is cut into row chunks, one workgroup each; partial sums meet there).  Not replica-aware. */
size_t dyb_gn_jvp_scratch_floats(int N, int HW, int C);
int dyb_gn_jvp_fwd(const float* y, float* ty, const float* ty2, const float* stats, const float* gamma, const float* beta,
                   const float* tgamma, const float* tbeta, const float* res, const float* tres, float* out, float* tout, float* tstats,
                   float* scratch, int N, int HW, int C, int relu, dyb_stream_t stream);
int dyb_gn_jvp_bwd(const float* dout, const float* tdout, const float* out_mask, const float* y, const float* ty, const float* stats,
                   const float* tstats, const float* gamma, const float* tgamma, float* dm, float* tdm, float* dy, float* tdy,
                   float* scratch, float* tdgamma, float* tdbeta, int N, int HW, int C, int relu, dyb_stream_t stream);
/* The same two as ONE launch each (the chunks of a slab meet on an arrival counter inside the launch instead of between two launches):
 * sync = dyb_gn_jvp_sync_words(N) 32-bit words - an error word, then one counter per (image, group) slab - zero on entry and private to
 * the call until it has finished on the stream.  A wait that lasts 0.2 s raises sync[0] and goes on (results then wrong). */
size_t dyb_gn_jvp_sync_words(int N);
int dyb_gn_jvp_fwd_onepass(const float* y, float* ty, const float* ty2, const float* stats, const float* gamma, const float* beta,
                           const float* tgamma, const float* tbeta, const float* res, const float* tres, float* out, float* tout,
                           float* tstats, float* scratch, unsigned* sync, int N, int HW, int C, int relu, dyb_stream_t stream);
int dyb_gn_jvp_bwd_onepass(const float* dout, const float* tdout, const float* out_mask, const float* y, const float* ty,
                           const float* stats, const float* tstats, const float* gamma, const float* tgamma, float* dm, float* tdm,
                           float* dy, float* tdy, float* scratch, unsigned* sync, float* tdgamma, float* tdbeta, int N, int HW, int C,
                           int relu, dyb_stream_t stream);
/* Exact Hessian-vector product through HMR, forward-over-reverse (hvp_engine.inc).  acts = the arena dyb_hmr_forward filled at
 * (params, image); tparams = the direction v (parameter arena layout); dual = scratch of dyb_hmr_hvp_dual_floats floats shared by
 * the two passes.  _jvp_forward leaves the tangent of the regressor's final state [B][160] at dual + dyb_hmr_hvp_offset_tstate;
 * the caller differentiates the head (rot6d -> SMPL -> losses) along it; _jvp_backward takes the head's gradient w.r.t. that state
 * (d_state, rot6d folded in) and its tangent (td_state) and writes hv = H v in the parameter arena layout (tensor spans only: zero
 * hv first).  Eval mode, fp32, one sequence per call.  aux (may be NULL): a side stream; the halves of every tangent pair that
 * are off the dependency chain (conv(x, tw), the weight-gradient pairs, dgrad(dy, tw)) are issued there, ordered by events, and
 * everything has joined `stream` again when a call returns. */
size_t dyb_hmr_hvp_dual_floats(const void* plan);
long long dyb_hmr_hvp_offset_tstate(const void* plan);
int dyb_hmr_jvp_forward(void* plan, const float* params, const float* tparams, const float* acts, float* dual, int n_iter, void* ws,
                        size_t ws_bytes, dyb_stream_t stream, dyb_stream_t aux);
int dyb_hmr_jvp_backward(void* plan, const float* params, const float* tparams, const float* acts, float* dual, const float* d_state,
                         const float* td_state, int n_iter, float* hv, void* ws, size_t ws_bytes, dyb_stream_t stream, dyb_stream_t aux);
/* tangent of MaxPool2d(3,2,1): ty = tx gathered at the tap indices dyb_maxpool3x3s2_fwd stored */
int dyb_maxpool3x3s2_jvp(const float* tx, const uint32_t* idx, float* ty, int N, int H, int W, int C, dyb_stream_t stream);

/* One forward layer = conv + the GroupNorm statistics of its output (what the engine issues per layer): y and *nchunks
 * partial records [G][2] in `partials` (>= dyb_groupnorm_workspace_bytes(N, Ho*Wo, K) and >= 4*(Ho*Wo/32+1)*(K/32)*8
 * bytes).  part_prev != NULL: x is the producer's raw output, normalised in the loader from its nch_prev partials.
 * Small 1x1 layers at batch 1 run as ONE launch (statistics in the conv epilogue); dyb_groupnorm_apply_n is
 * dyb_groupnorm_apply with the partial counts given explicitly. */
int dyb_conv2d_nhwc_fwd_gnstats(const float* x, const float* part_prev, int nch_prev, const float* gamma_prev,
                                const float* beta_prev, int relu_prev, float* stats_prev_out, const float* w, float* y,
                                float* partials, int* nchunks, int N, int H, int W, int C, int K, int R, int S, int stride,
                                int pad, void* ws, size_t ws_bytes, dyb_stream_t stream);
int dyb_groupnorm_apply_n(const float* y, const float* partials, int nch, const float* gamma, const float* beta,
                          const float* residual, const float* res_partials, int res_nch, const float* res_gamma,
                          const float* res_beta, float* res_stats, float* out, float* stats, int N, int HW, int C, int relu,
                          dyb_stream_t stream);

/* Backward mirror of dyb_conv2d_nhwc_fwd_gnstats: the data gradient of a conv fused with the GroupNorm-backward reduce
 * of the PRODUCER of its input (GroupNorm over [N][H*W][C]): dm_p and the partial block part_p
 * (dyb_groupnorm_bwd_partial_floats(N, H*W, C) floats) come out, *nch_p / *ncolb_p give part_p's layout; dx itself only
 * exists in dx_scratch (or not at all).  With DYB_K4_BWD=1 small 1x1 layers at batch 1 are ONE launch; otherwise it is
 * dyb_conv2d_nhwc_dgrad_gn + dyb_groupnorm_bwd_reduce.  (nch, ncolb) describe `part` of THIS conv's GroupNorm (0, 0 = the
 * dyb_groupnorm_bwd_reduce layout).  The _n gradients take such an explicit layout; in dyb_conv2d_nhwc_wgrad_gn_n the
 * conv input is x, or - x == NULL - relu(gn(y_prev)) formed in the loader. */
int dyb_conv2d_nhwc_dgrad_gn_reduce(const float* dm, const float* y_gn, const float* stats, const float* part, int nch,
                                    int ncolb, const float* gamma, const float* w, const float* addend, const float* y_p,
                                    const float* out_p, const float* stats_p, const float* gamma_p, const float* beta_p,
                                    float* dm_p, float* part_p, int* nch_p, int* ncolb_p, float* dx_scratch, int N, int H,
                                    int W, int C, int K, int R, int S, int stride, int pad, void* ws, size_t ws_bytes,
                                    dyb_stream_t stream);
int dyb_conv2d_nhwc_dgrad_gn_n(const float* dm, const float* y_gn, const float* stats, const float* part, int nch, int ncolb,
                               const float* gamma, const float* w, float* dx, const float* addend, int N, int H, int W, int C,
                               int K, int R, int S, int stride, int pad, void* ws, size_t ws_bytes, dyb_stream_t stream);
int dyb_conv2d_nhwc_wgrad_gn_n(const float* x, const float* y_prev, const float* stats_prev, const float* gamma_prev,
                               const float* beta_prev, const float* dm, const float* y_gn, const float* stats,
                               const float* part, int nch, int ncolb, const float* gamma, float* dw, float* dgamma,
                               float* dbeta, int N, int H, int W, int C, int K, int R, int S, int stride, int pad, void* ws,
                               size_t ws_bytes, dyb_stream_t stream);

/* ---- pooling / layout: nn.MaxPool2d(3,2,1), nn.AvgPool2d(7) (reference model/hmr.py:73,78,142,155)
 * and the NCHW(3) -> NHWC(4) repack of the dataloader image (boa_dataset/pw3d.py:115). */
int dyb_nchw3_to_nhwc4(const float* x, float* y, int N, int H, int W, dyb_stream_t stream);
int dyb_maxpool3x3s2_fwd(const float* x, float* y, uint32_t* idx, int N, int H, int W, int C, dyb_stream_t stream);
int dyb_maxpool3x3s2_bwd(const float* dy, const uint32_t* idx, float* dx, int N, int H, int W, int C,
                         dyb_stream_t stream);
int dyb_avgpool_fwd(const float* x, float* const* dsts, int ndst, int ld, int N, int HW, int C, dyb_stream_t stream);
int dyb_avgpool_bwd(const float* dxf, int ld, float* dx, int N, int HW, int C, dyb_stream_t stream);

/* ---- linear layers of the iterative regressor: nn.Linear fc1/fc2/decpose/decshape/deccam
 * (reference model/hmr.py:82-90,161-172) and their autograd. */
int dyb_linear_fwd(const float* x, int ldx, const float* w, int ldw, const float* bias, const float* res, int ldres,
                   float* y, int ldy, int B, int I, int O, dyb_stream_t stream);
size_t dyb_linear_bwd_workspace_bytes(int B, int I, int O);
int dyb_linear_bwd_dx(const float* dy, int lddy, const float* w, int ldw, int B, int I, int O, float* dstA, int ldA,
                      int accA, int split_col, float* dstB, int ldB, const float* addB, int ldaddB, void* ws,
                      size_t ws_bytes, dyb_stream_t stream);
int dyb_linear_bwd_dw(const float* const* dys, const int* lddys, const float* const* xs, const int* ldxs, int T, int B,
                      int I, int O, float* dw, int ldw, float* db, dyb_stream_t stream);

/* ---- rotation maps: utils/geometry.py:47-61 (rot6d_to_rotmat) and :184-306
 * (rotation_matrix_to_angle_axis), forward and backward. */
int dyb_rot6d_fwd(const float* x6, int ldx, float* rotmat, int B, dyb_stream_t stream);
int dyb_rot6d_bwd(const float* x6, int ldx, const float* drotmat, float* dx6, int lddx, int B, dyb_stream_t stream);
/* smplx.lbs.batch_rodrigues (pose2rot=True path of SMPL.forward; metric ground truth only) */
int dyb_rodrigues_fwd(const float* axis_angle, float* rotmat, int n, dyb_stream_t stream);
int dyb_rotmat_to_aa_fwd(const float* R, float* aa, int n, dyb_stream_t stream);
int dyb_rotmat_to_aa_bwd(const float* R, const float* daa, float* dR, int n, dyb_stream_t stream);

/* ---- SMPL forward/backward: smplx lbs + vertex joints + J_regressor_extra + 49-joint gather
 * (reference model/smpl.py:25-37).
 * tables_f = {v_template[6890*3], shapedirs[6890*3][10], posedirs[207][6890*3], weights_t[24][6890],
 *             j_template[24*3], j_shapedirs[72][10], j_extra[9][6890]}
 * tables_i = {parents[24], vertex_joint_ids[21], joint_map[49]}        (device int32) */
size_t dyb_lbs_saved_floats(int B);
size_t dyb_lbs_bwd_workspace_bytes(int B);
int dyb_lbs_fwd(const float* const* tables_f, const int* const* tables_i, const float* betas, int ldb,
                const float* rotmat, float* verts, float* joints49, float* saved, int B, dyb_stream_t stream);
int dyb_lbs_bwd(const float* const* tables_f, const int* const* tables_i, const float* rotmat, const float* saved,
                const float* djoints49, const float* dverts, float* drot, float* dbetas, int lddb, int B, void* ws,
                size_t ws_bytes, dyb_stream_t stream);
/* J_regressor_h36m @ vertices of the metric path (reference dynaboa_benchmark.py:220-233) */
int dyb_regress_joints(const float* reg, const float* verts, float* out, int nj, int B, dyb_stream_t stream);

/* ---- losses: BaseAdaptor.projection (base_adaptor.py:160-170) and the frame-loss block of
 * lower/upper_level_adaptation (:229-240 / :279-289 with cal_shape_prior :401, cal_pose_prior :405,
 * MaxMixturePrior.merged_log_likelihood utils/smplify/prior.py:181-196).  dyb_frame_losses returns
 * the three loss values + weighted total AND the gradient of the total in one launch. */
int dyb_projection_fwd(const float* cam, int ldc, const float* p3, float* p2, int B, int np, dyb_stream_t stream);
int dyb_projection_bwd(const float* cam, int ldc, const float* p3, const float* g2, float* dp3, float* dcam, int lddc,
                       int B, int np, dyb_stream_t stream);
/* utils/geometry.py:63-91 perspective_projection(points (B,N,3), rotation (B,3,3), translation (B,3), focal_length, camera_center
 * (B,2)) -> (B,N,2) and its gradient w.r.t. points and translation; focal: per sample with stride ldf floats (0: one value). */
int dyb_perspective_projection_fwd(const float* points, const float* rotation, const float* translation, const float* focal, int ldf,
                                   const float* center, float* out, int B, int np, dyb_stream_t stream);
int dyb_perspective_projection_bwd(const float* points, const float* rotation, const float* translation, const float* focal, int ldf,
                                   const float* g2, float* dpoints, float* dtranslation, int B, int np, dyb_stream_t stream);
/* MaxMixturePrior.forward / merged_log_likelihood (utils/smplify/prior.py:181-196) on an axis-angle body pose [B][69]: out[B] =
 * per-sample min over the 8 Gaussians, dpose69 (may be NULL) = its gradient. */
int dyb_gmm_prior(const float* pose69, const float* gmm_means, const float* gmm_prec, const float* gmm_logw, float* out,
                  float* dpose69, int B, dyb_stream_t stream);
int dyb_frame_losses(const float* rotmat, const float* shape, int lds, const float* cam, int ldc, const float* joints49,
                     const float* kp2d, const float* gmm_means, const float* gmm_prec, const float* gmm_logw, float w2d,
                     float wshape, float wpose, float* losses_out, float* drot, float* dshape, int ldds, float* dcam,
                     int lddc, float* djoints49, int B, void* ws, size_t ws_bytes, dyb_stream_t stream);
/* Keypoint sets: the window of the 49-joint convention that the 2-D keypoint term of the frame head and the motion term supervise.
 * The keypoint array keeps its [B][49][3] layout for both.
 *   DYB_KP_GT24 (0): joints 25..48, mean over B * 24 * 2 - the ground-truth style joints of dynaboa_benchmark.py (base_adaptor.py:229,234)
 *   DYB_KP_OP25 (1): joints  0..24, mean over B * 25 * 2 - OpenPose BODY_25 detections in slots 0..24, the online path of
 *                    dynaboa_webcam.py (:164-182 cal_motion_loss, :206 / :248 the frame term on [:, :25])
 * dyb_frame_losses_kp is dyb_frame_losses with the set as an argument (value, the four gradients and the per-sample camera sum all
 * follow the window; dyb_frame_losses forwards with DYB_KP_GT24 and its results are unchanged bit for bit).  An unknown set returns
 * DYB_ERR_ARG before anything is launched. */
#define DYB_KP_GT24 0
#define DYB_KP_OP25 1
int dyb_frame_losses_kp(const float* rotmat, const float* shape, int lds, const float* cam, int ldc, const float* joints49,
                        const float* kp2d, const float* gmm_means, const float* gmm_prec, const float* gmm_logw, float w2d,
                        float wshape, float wpose, float* losses_out, float* drot, float* dshape, int ldds, float* dcam,
                        int lddc, float* djoints49, int B, int kp_set, void* ws, size_t ws_bytes, dyb_stream_t stream);

/* ---- closed-form second derivative of the frame-loss head (--hvp exact --hvp_head closed).
 * Every *_jvp entry point computes what its sibling computes AND, in the same launches, the directional derivative along the
 * t-prefixed inputs; a t-prefixed array has the shape and leading dimension of its value array.  The table sweeps (posedirs) are
 * read once for value and tangent.  The value arrays are the sibling's in the same arithmetic, equal to rounding but not bit for bit
 * (the compiler contracts the two instantiations differently).  Single sequence only: inside a replica scope they return
 * DYB_ERR_UNSUPPORTED.
 *   dyb_rot6d_jvp / dyb_rot6d_bwd_jvp : rot6d -> R along tx6; its gradient along (tx6, tdrotmat)
 *   dyb_lbs_jvp                       : SMPL forward along (trotmat, tbetas); tsaved (dyb_lbs_saved_floats) = tangents of `saved`
 *   dyb_frame_losses_jvp              : tangent of the four gradients of dyb_frame_losses, inside the quaternion branch and the
 *                                       mixture component the value selects
 *   dyb_lbs_bwd_jvp                   : full tangent of the SMPL backward (its action on tdjoints49 + its own derivative with
 *                                       respect to pose and shape); ws >= 2 * dyb_lbs_bwd_workspace_bytes(B)
 *   dyb_head_hvp                      : the whole head on a regressor state [B][ld] (pose6d 144 | shape 10 | cam 3 | pad):
 *                                       d_state = gradient of w2d * kp2d + wshape * shape prior + wpose * pose prior, bit for bit
 *                                       what the five calls rot6d_fwd, lbs_fwd, frame_losses, lbs_bwd + head_grad_combine,
 *                                       rot6d_bwd give (it runs them after the tangent pass);
 *                                       td_state = H_head(state) . tstate; columns 157.. of both are written as zero (ldd >= 157);
 *                                       losses4 (may be NULL) as dyb_frame_losses; ws 16-byte aligned. */
int dyb_rot6d_jvp(const float* x6, const float* tx6, int ldx, float* rotmat, float* trotmat, int B, dyb_stream_t stream);
int dyb_rot6d_bwd_jvp(const float* x6, const float* tx6, int ldx, const float* drotmat, const float* tdrotmat, float* dx6,
                      float* tdx6, int lddx, int B, dyb_stream_t stream);
int dyb_lbs_jvp(const float* const* tables_f, const int* const* tables_i, const float* betas, const float* tbetas, int ldb,
                const float* rotmat, const float* trotmat, float* verts, float* tverts, float* joints49, float* tjoints49,
                float* saved, float* tsaved, int B, dyb_stream_t stream);
int dyb_lbs_bwd_jvp(const float* const* tables_f, const int* const* tables_i, const float* rotmat, const float* trotmat,
                    const float* saved, const float* tsaved, const float* djoints49, const float* tdjoints49, float* drot,
                    float* tdrot, float* dbetas, float* tdbetas, int lddb, int B, void* ws, size_t ws_bytes, dyb_stream_t stream);
int dyb_frame_losses_jvp(const float* rotmat, const float* trotmat, const float* shape, const float* tshape, int lds,
                         const float* cam, const float* tcam, int ldc, const float* joints49, const float* tjoints49,
                         const float* kp2d, const float* gmm_means, const float* gmm_prec, const float* gmm_logw, float w2d,
                         float wshape, float wpose, float* losses_out, float* drot, float* tdrot, float* dshape, float* tdshape,
                         int ldds, float* dcam, float* tdcam, int lddc, float* djoints49, float* tdjoints49, int B, void* ws,
                         size_t ws_bytes, dyb_stream_t stream);
size_t dyb_head_hvp_workspace_bytes(int B);
int dyb_head_hvp(const float* const* tables_f, const int* const* tables_i, const float* state, const float* tstate, int ld,
                 const float* kp2d, const float* gmm_means, const float* gmm_prec, const float* gmm_logw, float w2d, float wshape,
                 float wpose, float* losses4, float* d_state, float* td_state, int ldd, int B, void* ws, size_t ws_bytes,
                 dyb_stream_t stream);

/* The other terms of the level losses, value + gradient in one launch each (B <= 16): mode 0 mean-teacher consistency
 * (reference base_adaptor.py:320-343: 5 mse(s2d) + 5 mse(s3d) + 0.001 mse(shape) + mse(rotmat) against the teacher's outputs
 * rot2 / shape2 / cam2 / joints2), mode 1 motion (:379-398: confidence-masked mse of the projected-keypoint motion between the
 * frame and the history frame - cam2 / joints2 are the history pass's outputs, kp / kp2 the two frames' keypoints), mode 2
 * labelled exemplar (:346-376 with the hip-centred 3-D loss of :412-422; kp / gt_rot / gt_betas / gt_s3d [B][24][4] are the
 * exemplar's annotations).  s2d is the normalised projection (:160-170) formed inside.  Gradients of weight * term w.r.t. the
 * student pass's rotmat [B][216] / shape [B][10] / cam [B][3] / joints49 [B][147] (accumulate != 0: added) and, mode 1, w.r.t.
 * the history pass's cam / joints49.  vals5 = {s2d, s3d, shape, pose, loss} un-weighted (mode 1: {motion, 0, 0, 0, motion}). */
int dyb_aux_loss_terms(int mode, int B, int accumulate, float weight, const float* rot, const float* shape, int lds,
                       const float* cam, int ldc, const float* joints49, const float* rot2, const float* shape2, int lds2,
                       const float* cam2, int ldc2, const float* joints2, const float* kp, const float* kp2,
                       const float* gt_rot, const float* gt_betas, const float* gt_s3d, float* vals5, float* d_rot,
                       float* d_shape, float* d_cam, float* d_joints49, float* d_cam2, float* d_joints2, dyb_stream_t stream);
/* The same with a keypoint set (see dyb_frame_losses_kp) for the motion term: both passes' projections, the mask "both frames'
 * confidences are 1", the mean over B * count * 2 and the gradients to the student and the history pass are restricted to the
 * window.  Modes 0 and 2 do not read it (an unknown set is DYB_ERR_ARG for every mode).  dyb_aux_loss_terms forwards with DYB_KP_GT24. */
int dyb_aux_loss_terms_kp(int mode, int B, int accumulate, float weight, const float* rot, const float* shape, int lds,
                          const float* cam, int ldc, const float* joints49, const float* rot2, const float* shape2, int lds2,
                          const float* cam2, int ldc2, const float* joints2, const float* kp, const float* kp2,
                          const float* gt_rot, const float* gt_betas, const float* gt_s3d, float* vals5, float* d_rot,
                          float* d_shape, float* d_cam, float* d_joints49, float* d_cam2, float* d_joints2, int kp_set,
                          dyb_stream_t stream);
/* tests / lab: the two windowed heads for nrep sequence replicas in one launch, each replica with its own inputs and outputs in its
 * slice of `blob` ([nrep][blob_floats]; per-replica layouts in csrc/losses.hip).  Results per replica are those of the call on that
 * replica alone. */
int dyb_debug_frame_losses_kp_replicas(float* blob, size_t blob_floats, int nrep, const float* gmm_means, const float* gmm_prec,
                                       const float* gmm_logw, float w2d, float wshape, float wpose, int B, int kp_set,
                                       dyb_stream_t stream);
int dyb_debug_motion_term_kp_replicas(float* blob, size_t blob_floats, int nrep, int B, int accumulate, float weight, int kp_set,
                                      dyb_stream_t stream);

/* Gradient assembly of the fused HMR + SMPL + frame-loss node (one autograd node per adaptation level instead
 * of three plus glue): out = g*a (+ ext) with g a device scalar (NULL = 1), and the d_rotmat / d_state inputs of
 * dyb_hmr_backward from the dyb_frame_losses pieces (scaled by g), the dyb_lbs_bwd pieces and optional external
 * gradients on rotmat / shape / cam (teacher, motion and label terms attach there). */
int dyb_scale_add(const float* g, const float* a, const float* ext, float* out, size_t n, dyb_stream_t stream);
int dyb_head_grad_combine(const float* g, const float* drot_loss, const float* drot_smpl, const float* drot_ext,
                          const float* dshape_loss, const float* dbetas_smpl, const float* dshape_ext,
                          const float* dcam_loss, const float* dcam_ext, float* d_rot, float* d_state, int B,
                          dyb_stream_t stream);

/* PA-MPJPE on the device: compute_similarity_transform(_batch) of reference utils/pose_utils.py:9-64 (centre, K = X1^T X2,
 * 3x3 SVD, reflection fix, scale, translation) + the mean per-joint error of dynaboa_benchmark.py:236-240, one sample per
 * thread, so that the metric path ships scalars instead of joint sets.  aligned (optional) receives the aligned prediction. */
int dyb_pa_mpjpe(const float* pred, const float* gt, float* out, float* aligned, int n, int J, dyb_stream_t stream);

/* Sequence metrics (csrc/seq_metrics.hip; reference utils/pose_utils.py:66-144: compute_pck, reconstruction_error, compute_error_accel)
 * over n frames cut into n_seq sequences: one launch over the frames, one reduction per sequence, stream ordered, no synchronisation.
 * pred, gt [n][J][3] in one unit (root-aligned by the caller); seq_offsets [n_seq + 1] on the device, ascending, [0] = 0,
 * [n_seq] = n (a sequence of length 0 is legal); valid (may be NULL = all valid) [n]: the reference's `vis`; frame_id (may be
 * NULL) [n]: the frame's number in its video; thresholds [n_thr] on the device, n_thr in 0..64: the AUC thresholds.
 * frame_out [n][DYB_SEQM_FRAME_FLOATS], the columns below.  PCK = mean_j(|p_j - g_j| < pck_thr) and AUC = the mean of the PCKs over
 * `thresholds` (0 for n_thr = 0) are taken on the pair as given, NOT after alignment - what the reference computes.  The
 * acceleration error of centre frame i is mean_j |(p[i-1] - 2 p[i] + p[i+1]) - (g[i-1] - 2 g[i] + g[i+1])|; the triple counts iff its
 * three frames lie in one sequence, all three are valid and, with frame_id, their ids are f, f + 1, f + 2; otherwise both columns
 * are 0.  seq_out [n_seq + 1][DYB_SEQM_SEQ_FLOATS]: per sequence the frame count, the means of columns 0..3 over its frames, the
 * mean acceleration error over its counted triples (0 when none) and their count; row n_seq the same over all frames; an empty
 * sequence is a row of zeros.  Sums are taken in double in an order fixed by the sequence's length: no floating-point atomics, two
 * calls return equal bytes, and a sequence's row does not depend on its place in the batch.  DYB_ERR_ARG (nothing written): a NULL
 * required pointer (pred, gt and frame_out are required when n > 0), J < 3, n < 0, n_seq < 1, n_thr outside 0..64. */
#define DYB_SEQM_MPJPE 0
#define DYB_SEQM_PAMPJPE 1          /* the arithmetic of dyb_pa_mpjpe */
#define DYB_SEQM_PCK 2
#define DYB_SEQM_AUC 3
#define DYB_SEQM_ACCEL 4
#define DYB_SEQM_ACCEL_COUNTED 5    /* 1.0 if the triple centred on the frame counts, else 0.0 (column 4 is then 0.0) */
#define DYB_SEQM_FRAME_FLOATS 6
#define DYB_SEQM_SEQ_FRAMES 0
#define DYB_SEQM_SEQ_MPJPE 1
#define DYB_SEQM_SEQ_PAMPJPE 2
#define DYB_SEQM_SEQ_PCK 3
#define DYB_SEQM_SEQ_AUC 4
#define DYB_SEQM_SEQ_ACCEL 5
#define DYB_SEQM_SEQ_TRIPLES 6
#define DYB_SEQM_SEQ_FLOATS 7
int dyb_seq_metrics(const float* pred, const float* gt, const int* seq_offsets, int n_seq, const unsigned char* valid,
                    const int* frame_id, float pck_thr, const float* thresholds, int n_thr, float* frame_out, float* seq_out, int n,
                    int J, dyb_stream_t stream);

/* Temporal smoothing of a predicted sequence (csrc/smooth.hip; the reference has no smoother - the rules below are the definition, and
 * tests/smooth_cases.py restates them in fp64 NumPy).  n frames cut into n_seq sequences as for dyb_seq_metrics: seq_offsets
 * [n_seq + 1] on the device, valid [n] (NULL = all valid), frame_id [n] (NULL = consecutive).  Frames i and i + 1 are LINKED iff both
 * lie in one sequence, both are valid and, with frame_id, frame_id[i + 1] == frame_id[i] + 1; a RUN is a maximal chain of linked frames.
 * dyb_smooth_sequences, the non-causal window: weights_host [2 half_window + 1] is HOST memory, read before the launch and passed by
 * value; weights_host[k + half_window] weighs tap k = -half_window .. half_window.  Only the taps inside the centre's run count.
 * rotmat [n][J][9], per joint: q_k = the quaternion of R[i + k] (the four-branch formula of csrc/dyb_quat.h); a tap whose quaternion
 * is not finite is left out; a tap is negated when dot(q_k, q_0) < 0; s = sum_k w_k q_k in fp32, taps in ascending k; the output is
 * the rotation matrix of s / |s| (the weighted chordal mean) - or the centre's nine floats, copied, when |s|^2 < 1e-12 or the centre's
 * own quaternion is not finite.  betas [n][nb] and cam [n][nc] (each may be NULL: not smoothed): sum_k w_k x_k / sum_k w_k per channel.
 * Byte copies of the input: everything when half_window == 0, invalid frames, frames whose run has length 1.  An invalid frame is
 * never read as a tap.  One launch, no floating-point atomics, an order of operations that depends on the frame's place in its run
 * alone: two calls return equal bytes and a sequence's output does not depend on where it lies in the batch.  Stream ordered, no
 * synchronisation.  DYB_ERR_ARG (nothing written): NULL rotmat, rotmat_out, seq_offsets or weights_host with n > 0; betas without
 * betas_out or cam without cam_out; an output overlapping its input; half_window outside 0 .. DYB_SMOOTH_MAX_HALF_WINDOW; a weight
 * that is not finite or < 0, or a centre weight that is not > 0; J < 1, n < 0, n_seq < 1, nb < 0 or nc < 0.
 * dyb_one_euro_step, the causal form: one One-Euro filter step for R sequences in one launch.  state [R][dyb_one_euro_state_floats(J,
 * nb, nc)]: per row a `started` float, then x-hat (J x 4 quaternion components | nb | nc floats), then dx-hat of the same size; a
 * zeroed row is a reset filter.  Groups are each joint's quaternion, each beta, each camera scalar.  Per group, x the new sample,
 * alpha(c) = 1 / (1 + (1 / (2 pi c)) / te): with started == 0, x-hat = x, dx-hat = 0, started is set and the outputs are byte copies
 * of the inputs; otherwise x is negated if dot(x, x-hat) < 0 (quaternions), dx = (x - x-hat) / te, dx-hat = alpha(d_cutoff) dx +
 * (1 - alpha(d_cutoff)) dx-hat, cutoff = min_cutoff + beta |dx-hat| (the norm over the group), x-hat = alpha(cutoff) x +
 * (1 - alpha(cutoff)) x-hat; a quaternion is then normalised, stored normalised, and its rotation matrix is the output.  active [R]
 * (NULL = all): the state and outputs of a sequence with active == 0 are not touched.  DYB_ERR_ARG (nothing written): a NULL state,
 * rotmat or rotmat_out with R > 0; nb > 0 without betas and betas_out, nc > 0 without cam and cam_out; an output overlapping its
 * input; te, min_cutoff or d_cutoff <= 0 or not finite, beta < 0 or not finite; J < 1, R < 0, nb < 0 or nc < 0
 * (dyb_one_euro_state_floats returns DYB_ERR_ARG for the same sizes). */
#define DYB_SMOOTH_MAX_HALF_WINDOW 32
int dyb_smooth_sequences(const float* rotmat, const float* betas, int nb, const float* cam, int nc, const int* seq_offsets, int n_seq,
                         const unsigned char* valid, const int* frame_id, const float* weights_host, int half_window,
                         float* rotmat_out, float* betas_out, float* cam_out, int n, int J, dyb_stream_t stream);
int dyb_one_euro_state_floats(int J, int nb, int nc);
int dyb_one_euro_step(float* state, const float* rotmat, const float* betas, int nb, const float* cam, int nc,
                      const unsigned char* active, float te, float min_cutoff, float beta, float d_cutoff, float* rotmat_out,
                      float* betas_out, float* cam_out, int R, int J, dyb_stream_t stream);

/* Person ids for detections that come without them (csrc/track.hip; the reference has no tracker and leaves association to external
 * tools - the rule below is the definition, and tests/track_cases.py restates it in fp64 NumPy).  A batch of V videos: video v owns
 * frames frame_offsets[v] .. frame_offsets[v + 1] of F, frame f owns detections det_offsets[f] .. det_offsets[f + 1] of n (both on the
 * device, ascending, from 0; empty frames and empty videos are legal); kp [n][K][3] = (x, y, confidence) in pixels, 1 <= K <=
 * DYB_TRACK_MAX_KP; frame_id [F] (NULL = the frame's position in its video), trusted to increase strictly within a video.
 * A joint is VISIBLE iff its confidence is > c_min.  A detection with fewer than min_common visible joints is UNTRACKABLE: it gets
 * track -1, matches nothing and starts nothing.  A detection's AREA is (max x - min x) * (max y - min y) over its visible joints.
 * A video has at most DYB_TRACK_MAX_PEOPLE live tracks; a live track has an id, the keypoints, visibility and area of the last
 * detection matched to it, and that detection's frame id `last`.  Per frame f, in this order:
 *  1. retire: every track with frame_id[f] - last > max_age is retired;
 *  2. score: for every live track t and trackable detection d among the frame's first DYB_TRACK_MAX_PEOPLE, with `common` the joints
 *     visible in both: s = 0 if |common| < min_common, otherwise s = (sum over common, ascending k, of
 *     expf(-(dx_k^2 + dy_k^2) / (2 kappa^2 A))) / |common| with A = max((area_t + area_d) / 2, 1), all in fp32;
 *  3. greedy assignment: among the pairs with both sides free and s >= s_min take the largest s - ties go to the lower track id, then
 *     to the lower detection index - assign it, and repeat until no pair is left;
 *  4. update: a matched track takes the detection's keypoints, visibility, area and frame id whole;
 *  5. new tracks: every unmatched trackable detection among the first DYB_TRACK_MAX_PEOPLE, in index order, starts a track with the
 *     video's next id (ids count from 0 per video in order of creation) while fewer than DYB_TRACK_MAX_PEOPLE tracks are live;
 *     otherwise it gets -1.  Detections past the DYB_TRACK_MAX_PEOPLE-th of a frame are not looked at and get -1.
 * No constant-velocity prediction, no appearance term, no gap filling: a person lost for more than max_age frame ids comes back under
 * a new id.  track_out [n]: the id or -1; sim_out [n] (may be NULL): the s a detection was matched with, 0 for one that started a
 * track, -1 for one left without; video_out [V][DYB_TRACK_VIDEO_INTS]: tracks started, untrackable detections (among the frames' first
 * DYB_TRACK_MAX_PEOPLE), detections left for lack of a slot (those past the DYB_TRACK_MAX_PEOPLE-th included), reserved 0.  One
 * launch, one workgroup per video, nothing shared between them: two calls return equal bytes and a video's outputs do not depend on
 * where it lies in the batch.  Stream ordered, no synchronisation.  DYB_ERR_ARG (nothing written): NULL kp or track_out with n > 0;
 * NULL det_offsets, frame_offsets or video_out; K outside 1 .. DYB_TRACK_MAX_KP; kappa <= 0; s_min outside (0, 1]; max_age < 0;
 * min_common < 1; a float that is not finite; n < 0, F < 0 or V < 1. */
#define DYB_TRACK_MAX_PEOPLE 64
#define DYB_TRACK_MAX_KP 32
#define DYB_TRACK_VIDEO_INTS 4
int dyb_track_videos(const float* kp, const int* det_offsets, const int* frame_offsets, const int* frame_id, int K, float c_min,
                     float kappa, float s_min, int max_age, int min_common, int* track_out, float* sim_out, int* video_out, int n, int F,
                     int V, dyb_stream_t stream);

/* ---- flat-arena updates: learn2learn MAML.adapt (call sites dynaboa_benchmark.py:136,140),
 * torch.optim.Adam (base_adaptor.py:126; dynaboa_benchmark.py:149-151), update_teacher
 * (base_adaptor.py:193-201), cal_feature_diff's cosine (:211-219). n = float count, multiple of 4. */
int dyb_fastweight_update(const float* p, const float* g, float* out, float lr, size_t n, dyb_stream_t stream);
int dyb_adam_step(float* p, const float* g, float* m, float* v, float beta1, float beta2, float step_size,
                  float bc2_sqrt, float eps, size_t n, dyb_stream_t stream);
/* Adam on the gradient g - alpha * h: the second-order path's last accumulation (v - lr * H v) fused into the optimiser step */
int dyb_adam_step_accum(float* p, const float* g, const float* h, float alpha, float* m, float* v, float beta1, float beta2,
                        float step_size, float bc2_sqrt, float eps, size_t n, dyb_stream_t stream);
int dyb_ema_update(float* teacher, const float* p, float alpha, size_t n, dyb_stream_t stream);
int dyb_axpby(const float* x, float* y, float a, float b, size_t n, dyb_stream_t stream);
int dyb_cosine_sim(const float* a, const float* b, size_t n, float eps, float* out, dyb_stream_t stream);

/* run-time switches of the dispatch policy (A/B runs, tests).  Read from the environment (DYB_K4, DYB_K4_BWD,
 * DYB_K4_BATCH, DYB_K4_MAXC) once at first use - never on the dispatch path - and changed here afterwards.
 * names: "k4" single-launch 1x1 forward conv + statistics; "k4_bwd" 1x1 data gradient carrying the producer's
 * GroupNorm-backward reduce; "k4_batch" both at batch > 1; "k4_maxc" their channel limit. */
/* Diagnostic: one convolution mode (0 forward, 1 data gradient, 2 weight gradient) for `nrep` sequence replicas in one launch -
 * x / w / dy / out are [nrep][...] stacks, every replica with its own weights (what the native stepper's launches look like); used by
 * tools/tp_lab.py to time a layer's kernels alone. */
int dyb_debug_conv_replicas(int mode, const float* x, const float* w, const float* dy, float* out, int nrep, int N, int H, int W, int C,
                            int K, int R, int S, int stride, int pad, void* ws, size_t ws_bytes, dyb_stream_t stream);
/* diagnostic (tools/gn_lab.py): dyb_groupnorm_bwd_onepass for nrep replicas in one launch; blob = [nrep] x { din | y | out | dm | dy |
 * stats(8) | dgamma | dbeta | workspace }, blob_floats per replica; mode bit 0: mask from the saved activation, bit 1: write dm */
int dyb_debug_gn_onepass_replicas(float* blob, size_t blob_floats, int nrep, const float* gamma, const float* beta, int HW, int C, int relu,
                                  int mode, dyb_stream_t stream);
/* diagnostic / tests: the operand-pair convolution the tangent passes of the exact Hessian-vector product are made of (latency form,
 * csrc/hvp_engine.inc): out = op(a1, b1) + op(a2, b2) (+ addend; data gradient only) as ONE launch with a K loop over both pairs.
 * mode 0 forward (a = x [N][H][W][C], b = w [R][S][C][K]), 1 data gradient (a = dy [N][Ho][Wo][K], b = w), 2 weight gradient (a = x,
 * b = dy).  DYB_ERR_UNSUPPORTED where the throughput schedule or the bf16 form is in force (option "conv_pair" = 0 turns pairs off). */
int dyb_debug_conv_pair(int mode, const float* a1, const float* b1, const float* a2, const float* b2, float* out, const float* addend,
                        int N, int H, int W, int C, int K, int R, int S, int stride, int pad, void* ws, size_t ws_bytes,
                        dyb_stream_t stream);
/* In-kernel hand-offs (one-pass GroupNorm backward: the workgroups of a slab meet on a counter) give up after ~0.2 s and go on with
 * incomplete sums rather than block the queue.  This returns how many did since the library was loaded; it waits for `stream`.
 * The reference has no counterpart (PyTorch kernels do not rendezvous); the drivers check it at their metric flush and raise. */
int dyb_sync_error_count(unsigned* count_host, dyb_stream_t stream);
/* tests / lab: counter region (nwords zeroed 32-bit words, device memory) for the in-kernel split-K fold of the calling thread's plain
 * conv calls, until reset with (NULL, 0).  With a region in scope a split launch's last-arriving workgroup per tile adds the slabs
 * itself (csrc/igemm_tp.inc); the engine passes its own regions per pass.  Option "stat_folds" counts such launches. */
int dyb_debug_set_conv_sync(unsigned* ctr, int nwords);
/* tests / lab ("fuse_fast", round 6): while set, a weight gradient of the calling thread whose result would land inside [grads, grads + bytes)
 * writes p_next[off] = p_cur[off] - lr * g instead of g - from its accumulators when it runs unsplit, from the fold launch that adds its
 * slabs when it splits (not with the throughput kernel's in-kernel fold), in the latency form's fp32 kernel too - the MAML
 * fast-weight step (learn2learn MAML.adapt: p' = p - lr * dL/dp; reference dynaboa_benchmark.py:136,140) fused into the convolution's
 * epilogue.  Reset with grads = NULL.  dyb_debug_wgrad_update_spans: how many launches took that form since the scope was set.  The frame
 * stepper opens such a scope around every lower level's backward (csrc/adapt_step.hip). */
int dyb_debug_set_wgrad_update(const float* grads, size_t bytes, const float* p_cur, float* p_next, float lr);
int dyb_debug_wgrad_update_spans(void);
/* the same for Adam ("fuse_adam"): an unsplit throughput-form weight gradient whose result would land inside [grads, grads + bytes) applies
 * torch.optim.Adam's single-tensor step (reference base_adaptor.py:126, dynaboa_benchmark.py:149-151) to theta / m / v IN PLACE at the same
 * offset from its accumulators; sc = device pointer to (step_size = lr / (1 - beta1^t), bc2_sqrt = sqrt(1 - beta2^t)).  Reset with
 * dyb_debug_set_wgrad_update(NULL, ...).  Only the pipelined loop forms carry that epilogue: with tp_kernel 1, a phase probe armed or a map
 * too small for the pipelined pixel walk the scope is declined - the plain gradient is written, no span counted.  The frame stepper opens
 * such a scope around the outer level's backward of a replica group. */
int dyb_debug_set_wgrad_adam(const float* grads, size_t bytes, float* theta, float* m, float* v, const float* sc, float beta1, float beta2,
                             float eps);
int dyb_set_option(const char* name, int value);
int dyb_get_option(const char* name, int* value);

/* diagnostic: n dependent launches of a trivial kernel (per-launch floor of a kernel chain) */
int dyb_debug_launch_chain(float* scratch, int n, int blocks, dyb_stream_t stream);

/* ---- native HMR engine: HMR.forward (reference model/hmr.py:127-181) and its backward over a
 * static plan.  Parameter / activation arena layouts are queried from the plan. */
int dyb_hmr_plan_create(int B, int H, int W, void** plan);
void dyb_hmr_plan_destroy(void* plan);
size_t dyb_hmr_param_floats(const void* plan);
size_t dyb_hmr_act_floats(const void* plan);
size_t dyb_hmr_workspace_bytes(const void* plan);
int dyb_hmr_num_tensors(const void* plan);
/* kind: 0 conv weight, 1 norm weight, 2 norm bias, 3 fc weight, 4 fc bias, 5 fused decoder weight
 * [160][1024] (decpose 0..143 | decshape 144..153 | deccam 154..156), 6 fused decoder bias */
int dyb_hmr_tensor_info(const void* plan, int i, char* name, int name_cap, int* kind, long long* offset, int* dims4,
                        int* cin_pad);
int dyb_hmr_feature_info(const void* plan, int which, long long* offset, int* dims4, int* row_stride);
long long dyb_hmr_act_offset_rotmat(const void* plan); /* [B][24][9] */
long long dyb_hmr_act_offset_state(const void* plan);  /* [B][160] pose|shape|cam|pad */
/* graph mode: whole forward / backward calls are captured into hipGraphs keyed by their pointer
 * arguments (second sighting of a key) and replayed; results are those of the eager path. */
int dyb_hmr_set_graph_mode(void* plan, int on);
/* bf16-MFMA variant of the plan's convolutions (BASELINE configs[4]; never the parity default): fp32 master weights, fp32
 * activations / GroupNorm statistics / accumulators, operand tiles rounded to bf16 (nearest even) as they are staged for
 * v_mfma_f32_32x32x16_bf16.  The option "bf16" (dyb_set_option) does the same for direct calls of the conv entry points. */
int dyb_hmr_set_bf16(void* plan, int on);
int dyb_hmr_graph_stats(const void* plan, long long* stats10); /* replays, eager, captures, fwd keys, bwd keys, 5 failure counters */
int dyb_hmr_forward(void* plan, const float* params, const float* image_nchw, const float* init_state, int n_iter,
                    float* acts, void* ws, size_t ws_bytes, dyb_stream_t stream);
/* aux_stream (may be NULL): second stream for the weight-gradient convolutions, which are off the
 * critical path; `stream` waits for them before the call returns control of ordering. */
int dyb_hmr_backward(void* plan, const float* params, const float* acts, const float* d_rotmat, const float* d_state,
                     int n_iter, float* grads, void* ws, size_t ws_bytes, dyb_stream_t stream, dyb_stream_t aux_stream);

/* ---- frame preprocessing: bounding-box crop + anti-aliased bilinear resize + /255 + Normalize + HWC->CHW ----------------
 * reference utils/dataprocess.py:48-96 crop() (test-time path: rot = 0) as called by boa_dataset/pw3d.py:131-136 and
 * base_adaptor.py:529-533, with skimage.transform.resize 0.17.2 semantics (Gaussian anti-aliasing sigma = (in/out - 1)/2,
 * 'mirror' boundary, bilinear warp at (j + 0.5) * in/out - 0.5), then pw3d.py:121-123.  img: decoded frame [H][W][3] uint8
 * RGB (device); (ul, br): box corners in frame pixels as the reference's transform(..., invert=1) gives them (may lie
 * outside the frame: zero fill); out: [3][res][res] fp32.  ws: dyb_crop_workspace_bytes(br_y - ul_y, br_x - ul_x). */
size_t dyb_crop_workspace_bytes(int box_h, int box_w);
int dyb_crop_resize_normalize(const uint8_t* img, int H, int W, int ul_x, int ul_y, int br_x, int br_y, float* out, int res,
                              float mean0, float mean1, float mean2, float std0, float std1, float std2, void* ws,
                              size_t ws_bytes, dyb_stream_t stream);
/* The same for n crops in one call (1 <= n <= 64), ragged: crop i has its own frame imgs[i] of H[i] x W[i], box corners and output
 * outs[i]; several crops may name one frame.  imgs / outs are HOST arrays of n device pointers, the int arguments HOST arrays of n.
 * Three launches and one host-to-device copy whatever n is, no host synchronisation; every output equals, bit for bit, what
 * dyb_crop_resize_normalize writes for that crop alone.  All crops are checked first: on an error return (n out of range, an empty
 * box, a tap table over the limit, a short buffer) nothing has been enqueued.
 * staging: dyb_crop_many_staging_bytes(n) bytes of host memory of the caller's (pinned, for the copy to be asynchronous).  The
 * stream reads it AFTER the call returns: do not pass the same block to a later call, or write to it, before the stream has passed
 * this call (an event recorded on `stream` after the call tells) - callers keep a small ring of blocks.
 * ws: dyb_crop_many_workspace_bytes(n, box_h, box_w) bytes of device memory; calls on one stream may share it. */
size_t dyb_crop_many_staging_bytes(int n);
size_t dyb_crop_many_workspace_bytes(int n, const int* box_h, const int* box_w);
int dyb_crop_resize_normalize_many(int n, const uint8_t* const* imgs, const int* H, const int* W, const int* ul_x, const int* ul_y,
                                   const int* br_x, const int* br_y, float* const* outs, int res, float mean0, float mean1,
                                   float mean2, float std0, float std1, float std2, void* staging, size_t staging_bytes, void* ws,
                                   size_t ws_bytes, dyb_stream_t stream);

/* ---- mesh overlay: N meshes rasterised over their frames in one call ---------------------------------------------------
 * Stands where the reference renders one frame at a time through pyrender (render_demo.py:58-134, called from
 * base_adaptor.py:429-443).  verts [N][V][3] fp32; faces [F][3] int32, shared by the N meshes; (adj_ptr [V+1], adj_idx [3F]):
 * vertex -> incident faces as CSR, ascending face index per vertex (the vertex normals are gathered in that order);
 * cam [N][4] = (sx, sy, tx, ty); background [N][H][W][3] uint8 RGB or NULL (black); out [N][H][W][3] uint8;
 * face_id [N][H][W] int32 (-1 = not covered) and depth [N][H][W] fp32 (+inf = not covered) are optional (NULL).
 * Image position u = W/2 (1 + sx (X + tx)), v = H/2 (1 + sy (Y + ty)), pixel centres at (i + 0.5, j + 0.5), depth = Z (smaller
 * is nearer, no clipping planes).  Coverage is exact: positions snapped to 1/256 pixel, int64 edge functions, top-left rule;
 * faces whose normal (v1 - v0) x (v2 - v0) has Z >= 0 after snapping are culled, and so is a face with a corner beyond 2^22
 * pixels.  Nearest face wins, ties to the lower index; the result does not depend on scheduling (two calls give equal bytes).
 * Smooth shading with the reference's ambient 0.3 and three light positions; pyrender's own material model is not
 * reproduced (csrc/render.hip).  N <= 64, H and W <= 4096 (DYB_ERR_UNSUPPORTED beyond).  ws: dyb_render_workspace_bytes(N, V, F);
 * after the call its first N * V * 3 floats hold the vertex normals.  Nothing is written when an error code is returned. */
size_t dyb_render_workspace_bytes(int N, int V, int F);
int dyb_render_meshes(const float* verts, const int* faces, const int* adj_ptr, const int* adj_idx, const float* cam,
                      const uint8_t* background, float col_r, float col_g, float col_b, uint8_t* out, int* face_id,
                      float* depth, int N, int V, int F, int H, int W, void* ws, size_t ws_bytes, dyb_stream_t stream);
/* The ragged form: up to 64 meshes in one call, each over a frame of its own size.  desc: HOST table of N entries - verts [V][3]
 * (device; the rows of different meshes need not be contiguous: they may point into result-ring rows of different replicas),
 * background [H][W][3] uint8 (device) or NULL (black), out [H][W][3] uint8 (device), H, W <= 4096.  The table and the prefix of
 * the meshes' tile counts travel as kernel arguments: no allocation, no copy, no host wait; the table may be reused when the
 * call returns.  cam [N][4] stays a device array.  Mesh i equals, byte for byte, dyb_render_meshes called alone with that mesh,
 * H_i, W_i (the same kernels: a mesh of this call is a scene of one mesh).  One workgroup per mesh first reduces the faces' pixel boxes to the mesh's own box
 * (integer min / max in LDS: deterministic); the tile grid is flat over all meshes and a tile outside its mesh's box copies the
 * frame without streaming the face list (flags bit 0 set: no box, every tile streams - same bytes, for measurements; other bits 0).
 * A mesh with no drawn face has an empty box: its picture is the frame.  DYB_ERR_ARG: NULL table / verts / out, non-positive size;
 * DYB_ERR_UNSUPPORTED: N > 64, H or W > 4096; DYB_ERR_WORKSPACE: ws_bytes < dyb_render_var_workspace_bytes(N, V, F).  Nothing is
 * written when an error code is returned. */
typedef struct dyb_render_desc {
  const float* verts;
  const uint8_t* background;
  uint8_t* out;
  int H, W;
} dyb_render_desc;
size_t dyb_render_var_workspace_bytes(int N, int V, int F);
int dyb_render_meshes_var(const dyb_render_desc* desc, const int* faces, const int* adj_ptr, const int* adj_idx, const float* cam,
                          float col_r, float col_g, float col_b, int N, int V, int F, int flags, void* ws, size_t ws_bytes,
                          dyb_stream_t stream);
/* Scenes: several meshes over ONE frame (all tracked people of a video frame in one overlay), up to 64 scenes and 64 meshes in
 * one call.  Every mesh has its own weak-perspective camera, so depths of different meshes are not comparable and there is NO
 * depth test between meshes - the painter rule instead: within a mesh the nearest face wins (ties: lower face index), between
 * meshes the one listed LATER wins wherever it covers a pixel, whatever its Z.  A scene equals, byte for byte, the chain
 * img = frame; for i in its range: img = dyb_render_meshes(mesh i over img, colour i) - the same kernels, in one pass: one workgroup per tile
 * walks the scene's meshes from the last to the first, skips a mesh whose pixel box misses the tile, stops testing a pixel once a
 * mesh has claimed it, leaves when every pixel of the tile is decided and shades each pixel once; the frame is read and written once.
 * scenes: HOST table of nscenes entries - background [H][W][3] uint8 (device) or NULL (black), out [H][W][3] uint8 (device),
 * mesh_id / face_id [H][W] int32 (device, optional: NULL): the winning mesh's position in the scene's own list and its face, -1
 * where nothing is drawn; [mesh_begin, mesh_end): the scene's meshes in the call's mesh list - the ranges tile 0 .. nmeshes in scene
 * order, a scene may be empty (its picture is its frame, or black).  mesh_verts: HOST table of nmeshes device pointers to [V][3]
 * fp32 rows (views into different buffers are fine); mesh_scene: HOST table, the scene of each mesh (must agree with the ranges);
 * cam [nmeshes][4] = (sx, sy, tx, ty) and colors [nmeshes][3] fp32 are DEVICE arrays.  A mesh is set up on its scene's H, W.  The
 * tables travel as kernel arguments: no allocation, no copy, no host wait; they may be reused when the call returns.  flags bit 0
 * set: no per-mesh pixel box (same bytes, for measurements); other bits 0.  With nmeshes == 0 mesh_verts, mesh_scene, cam, colors
 * and ws may be NULL.  DYB_ERR_ARG: a NULL required argument, nscenes <= 0, nmeshes < 0, non-positive size, ranges that do not
 * tile the list or disagree with mesh_scene; DYB_ERR_UNSUPPORTED: nscenes or nmeshes > 64, H or W > 4096; DYB_ERR_WORKSPACE:
 * ws_bytes < dyb_render_scenes_workspace_bytes(nmeshes, V, F).  Everything is checked before the first launch: nothing is written
 * when an error code is returned. */
typedef struct dyb_render_scene {
  const uint8_t* background;
  uint8_t* out;
  int* mesh_id;
  int* face_id;
  int H, W;
  int mesh_begin, mesh_end;
} dyb_render_scene;
size_t dyb_render_scenes_workspace_bytes(int nmeshes, int V, int F);
int dyb_render_scenes(const dyb_render_scene* scenes, int nscenes, const float* const* mesh_verts, const int* mesh_scene,
                      const float* cam, const float* colors, const int* faces, const int* adj_ptr, const int* adj_idx, int nmeshes,
                      int V, int F, int flags, void* ws, size_t ws_bytes, dyb_stream_t stream);
/* Side views and wireframe: the three entries again with one more argument, opts (HOST; NULL = the plain entry, which forwards here).
 * model: DEVICE array [meshes][9] fp32, one row-major 3x3 matrix per mesh of the call (NULL: identity), applied to the mesh in the
 * raw model space of these entries - x' = (m0 x + m1 y) + m2 z, likewise y', z', one rounding per operation - before anything reads
 * a position: normals, face set-up, depth and shading.  The reference's side view (render_demo.py:96-98: the mesh turned by Rx,
 * 180 degrees about X, then by R(angle, axis)) is model = Rx R Rx, as Rx is folded into the image coordinates here.  A call with
 * matrices equals, byte for byte, the plain call on the output of dyb_render_transform_verts (model NULL there: a copy).  It needs
 * dyb_render_model_workspace_bytes(meshes, V) MORE workspace than its entry's own size (the turned rows lie behind it) and, to check
 * the matrices before it launches anything, copies them to the host and waits for the stream: DYB_ERR_ARG for an entry that is
 * not finite, nothing written.  (Hence no stream capture with matrices; calls without matrices never wait.)
 * wireframe != 0: a face gives a fragment at a pixel centre iff the centre is inside it by the coverage rule AND for at least one
 * of its edges e  w_e < 256 max(|dx_e|, |dy_e|)  (w_e: the non-negative int64 edge function at the centre, dx_e / dy_e: the edge's
 * snapped extents in 1/256 pixel): the centre is within one pixel of the edge along its minor axis.  Nearest fragment wins (ties:
 * lower face index), depth and shading as for the solid mesh; a pixel without a fragment keeps the frame, or falls through to the
 * mesh beneath in a scene, with face_id -1 and depth +inf - OpenGL's line polygon mode (RenderFlags.ALL_WIREFRAME): only line
 * fragments take part in the depth test.  Unpinned against pyrender, like the shading. */
typedef struct dyb_render_opts {
  const float* model;
  int wireframe;
} dyb_render_opts;
size_t dyb_render_model_workspace_bytes(int N, int V);
int dyb_render_transform_verts(const float* verts, const float* model, float* out, int N, int V, dyb_stream_t stream);
int dyb_render_meshes_opt(const float* verts, const int* faces, const int* adj_ptr, const int* adj_idx, const float* cam,
                          const uint8_t* background, float col_r, float col_g, float col_b, uint8_t* out, int* face_id,
                          float* depth, int N, int V, int F, int H, int W, void* ws, size_t ws_bytes, dyb_stream_t stream,
                          const dyb_render_opts* opts);
int dyb_render_meshes_var_opt(const dyb_render_desc* desc, const int* faces, const int* adj_ptr, const int* adj_idx, const float* cam,
                              float col_r, float col_g, float col_b, int N, int V, int F, int flags, void* ws, size_t ws_bytes,
                              dyb_stream_t stream, const dyb_render_opts* opts);
int dyb_render_scenes_opt(const dyb_render_scene* scenes, int nscenes, const float* const* mesh_verts, const int* mesh_scene,
                          const float* cam, const float* colors, const int* faces, const int* adj_ptr, const int* adj_idx, int nmeshes,
                          int V, int F, int flags, void* ws, size_t ws_bytes, dyb_stream_t stream, const dyb_render_opts* opts);

/* ---- baseline JPEG of device pictures (csrc/jpeg.hip; dynaboa_amd/jpeg.py adds the header, EOI and the Motion-JPEG writer) --------
 * Up to 64 pictures of any sizes in one call.  desc: HOST table of N entries - rgb [H][W][3] uint8 (device: what the render entries
 * write), out (device) receives the entropy-coded scan ONLY - stuffed, padded, no markers - of at most `capacity` bytes;
 * 1 <= H, W <= 8192.  lengths [N] (device, int64) is ALWAYS the number of bytes the scan needs; where lengths[i] > capacity nothing
 * at or beyond out + capacity is written, that picture's bytes are unspecified and the other pictures are unaffected.  Stream
 * ordered, no host wait, no allocation: the table and the prefixes of the pictures' block counts travel as kernel arguments (the
 * table may be reused when the call returns), six launches whatever N.  No atomics: two calls return equal bytes, and a picture's
 * bytes do not depend on its place or company in the batch.
 * The arithmetic is libjpeg's, all integer (tests/jpeg_cases.py restates it in NumPy and is pinned to PIL's files):
 *   colour   Y = (19595 R + 38470 G + 7471 B + 32768) >> 16, Cb = (-11059 R - 21709 G + 32768 B + 8388608 + 32767) >> 16,
 *            Cr = (32768 R - 27439 G - 5329 B + 8388608 + 32767) >> 16, then - 128
 *   444      every plane repeats its last column and row up to multiples of 8; blocks in the order Y Cb Cr per 8 x 8 MCU
 *   420      16 x 16 MCUs, Y00 Y01 Y10 Y11 Cb Cr.  Chroma: the full plane repeats its last column up to 16 x MCUs and ONE row if H
 *            is odd, (a + b + c + d + bias) >> 2 with bias 1 on even output columns and 2 on odd ones, then the DOWNSAMPLED plane
 *            repeats its last row.  A Y block beyond ceil(W / 8) columns or ceil(H / 8) rows is a dummy: no AC, the quantised DC of
 *            the block coded just before it
 *   DCT      the Independent JPEG Group's accurate integer form (13-bit constants, rows then columns, 8 x the true DCT)
 *   quant    Annex K.1 / K.2 scaled by s = 5000 / Q (Q < 50) or 200 - 2 Q: q = clamp((base s + 50) / 100, 1, 255);
 *            c -> sign(c) ((|c| + 4 q) / (8 q))
 *   entropy  the four Annex K.3 tables, zig-zag order, DC differences per component, no restart markers, 1-bits fill the last
 *            byte, 0x00 behind every 0xFF
 * ws: dyb_jpeg_workspace_bytes(desc, N, subsampling) bytes (0 for a table the encode call refuses): per block 134 bytes
 * (coefficients, DC, bit offset), per picture min(capacity, 208 x blocks) bytes of unstuffed stream, 12 bytes per 1024 blocks and
 * per 1024 worst-case stream bytes.  DYB_ERR_ARG: NULL table, rgb, out or lengths, N < 1, non-positive size, negative capacity,
 * quality outside 1 .. 100; DYB_ERR_UNSUPPORTED: N > 64, H or W > 8192, subsampling other than 444 or 420; DYB_ERR_WORKSPACE.
 * Everything is checked before the first launch: nothing is written when an error code is returned. */
typedef struct dyb_jpeg_desc {
  const uint8_t* rgb;
  uint8_t* out;
  int H, W;
  long long capacity;
} dyb_jpeg_desc;
size_t dyb_jpeg_workspace_bytes(const dyb_jpeg_desc* desc, int N, int subsampling);
int dyb_jpeg_encode_many(const dyb_jpeg_desc* desc, int N, int quality, int subsampling, long long* lengths, void* ws,
                         size_t ws_bytes, dyb_stream_t stream);

/* ---- native frame stepper: Adaptor.adaptation (reference dynaboa_benchmark.py:126-193) as ONE call per frame --------
 * The first-order bilevel schedule with the frame-loss set - clone, inner_step x [lower-level loss
 * (base_adaptor.py:222-268) -> learner.adapt -> inference], upper-level loss (:270-317) through the fast weights,
 * zero_grad / backward / Adam.step, inference (:204-262) - issued from C++ over the entry points above: same kernels, same
 * order and operands as the Python composition (dynaboa_amd/benchmark.py), hence identical weights and Adam state, at
 * ~2.5 us of host time per launch instead of ~5.  A stepper owns no memory: theta / Adam moments / tables are the
 * caller's (dyb_stepper_set_p), scratch is one blob (dyb_stepper_workspace_bytes -> dyb_stepper_bind_workspace).
 * Steppers are independent: several may run on different streams from different host threads (sequence replicas
 * sharing one GPU).  Keys: csrc/dyb_stepper_options.h lists every option once - key, type (set_i / set_f / set_p), environment
 * variable, whether it is locked once the workspace is bound ("replicas", "fuse_fast", "full": DYB_ERR_ARG afterwards), meaning;
 * get_i / get_f return any int / double option by its key.  With code of their own:
 *   set_i: adam_step, adam_step_<replica>, replicas (1..64), logs_bytes, drop_seed, drop_offset, bank_seed, bank_draw_<replica>
 *   set_p: smpl_{neutral,male,female}_{0..6} and smpli_{...}_{0..2} (the table order of dyb_lbs_fwd)
 *   get_i: adam_step, adam_step_<replica>, bank_seed, bank_draw_<replica>, drop_used, slots_per_frame, result_floats (floats per row of the result ring), record_floats (floats per metric record: pred14 [B][14][3] |
 *          gt14 [B][14][3] | mpjpe [B] | pve), loss_floats (floats per frame in loss_log: (inner_step + 1) x {s2d, shape prior, pose
 *          prior, weighted total}; full term set: 16 per level, + optim_steps levels with the dynamic loop)
 * Unknown keys are errors.
 * Exemplar bank (full term set, batch 1): with the ten "bank_*" pointers and bank_items / bank_clusters / bank_members /
 * bank_pick_capacity set (and "bank_on_device" 1, the default), a level with a labelled term runs dyb_retrieve_select on the
 * chain's stream behind its forward - every replica of the launch from its own pooled feature, draw index bank_draw_<replica>,
 * seed bank_seed - and dyb_exemplar_gather into the replicas' exemplar inputs on the stream of the exemplar pass, behind an
 * event: no host callback, the parallel passes stay on, the exemplar entries of `inputs` stay NULL.  bank_draw_<replica> advances
 * by one per labelled level of that replica (not at all when the frame step returns an error); row (draw mod bank_pick_capacity)
 * of bank_picks[replica] receives (cluster, item), item -1 if the nearest cluster was empty (the replica's exemplar inputs are
 * then not rewritten).  A bank together with retrieve_fn / retrieve_rep_fn is DYB_ERR_ARG.
 * dyb_stepper_adapt_frame: gender is int64 [B]; gt_* / gender may be NULL with metrics = 0.  Records go to slots
 * record_slot.. (one per inner step when eval_lower, then the final one).  `aux`: weight-gradient stream (may be NULL);
 * `side`: stream for the final no-grad forward + its metrics (may be NULL), overlapped with the next frame.
 * dyb_stepper_join makes `stream` wait for the side stream's tail; dyb_stepper_output: 0 rotmat, 1 state, 2 vertices,
 * 3 joints49 of the last final inference. */
int dyb_stepper_create(void* plan, int B, int H, int W, void** stepper);
void dyb_stepper_destroy(void* stepper);
int dyb_stepper_set_i(void* stepper, const char* key, long long value);
int dyb_stepper_set_f(void* stepper, const char* key, double value);
int dyb_stepper_set_p(void* stepper, const char* key, const void* ptr);
long long dyb_stepper_get_i(const void* stepper, const char* key);
/* host issue time in ms accumulated over "host_frames" frame steps, by section: host_ms_forward / _backward / _head (loss head
 * + records) / _update (fast weights) / _tail (Adam + final inference) / _total */
double dyb_stepper_get_f(const void* stepper, const char* key);
size_t dyb_stepper_workspace_bytes(void* stepper);
int dyb_stepper_bind_workspace(void* stepper, void* ws, size_t bytes, dyb_stream_t stream);
int dyb_stepper_adapt_frame(void* stepper, const float* image, const float* kp2d, const float* gt_pose, const float* gt_betas,
                            const long long* gender, int record_slot, int loss_slot, dyb_stream_t stream, dyb_stream_t aux,
                            dyb_stream_t side);
/* The same step for `replicas` (set_i key, 1..64, before sizing the workspace) independent sequences in lockstep: every
 * launch of the chain covers all replicas (replica = a grid dimension; pointer arguments inside a replica's arenas are
 * rebased in the kernels), each replica with its own weights / Adam moments / workspace / records: theta, adam_m, adam_v are
 * [replicas][param floats], records [replicas][record_capacity][record_floats], loss_log [replicas][loss_capacity]
 * [loss_floats].  inputs: HOST array of 5 x replicas device pointers, kind-major: image[r], kp2d[r], gt_pose[r],
 * gt_betas[r], gender[r].  Results per replica are those of dyb_stepper_adapt_frame on that replica alone. */
int dyb_stepper_adapt_frames(void* stepper, const void* const* inputs, int record_slot, int loss_slot, dyb_stream_t stream,
                             dyb_stream_t aux, dyb_stream_t side);
/* The reference's FULL term set (its default flags) as one call per frame: per level the frame losses + (upper level) the
 * mean-teacher term with a no-grad teacher forward + the motion term with a second forward of the history frame + the
 * labelled-exemplar term with a forward of the retrieved exemplars (dyb_aux_loss_terms), gradients of the passes summed, Adam,
 * teacher EMA, final inference, and the dynamic-BOA loop (dynaboa_benchmark.py:161-192): the 15 feature cosines come from one
 * launch that also writes them to device-visible pinned host memory, which the call polls - its only host wait, no stream
 * synchronise - to decide on up to optim_steps further upper-level steps.  Enable with set_i "full" = 1 before sizing the
 * workspace; further keys: set_i temporal_lower/upper, use_teacher, use_motion, interval, mix_lower/upper, dynamic, optim_steps;
 * set_f teacherloss_weight, motionloss_weight, labelloss_weight, alpha, cos_sim_threshold; set_p teacher (parameter arena),
 * gate_host (16 floats, pinned), gate_log ([loss_capacity][1 + optim_steps][16]), feat5_out ([2048]), retrieve_fn / retrieve_user
 * (int fn(void* user, int level, const void** ex5): host retrieval of exemplars from feat5_out, batch 1).  inputs: HOST array of
 * 12 device pointers: image, kp2d, gt_pose, gt_betas, gender, hist_image, hist_kp2d (NULL: no motion term), ex_img, ex_kp,
 * ex_pose, ex_betas, ex_pose3d (NULL with a retrieval callback).  loss_log rows are 16 floats per level (adapt_step.hip). */
int dyb_stepper_adapt_frame_full(void* stepper, const void* const* inputs, int record_slot, int loss_slot, int* extra_steps,
                                 dyb_stream_t stream, dyb_stream_t aux);
/* The full term set for the stepper's sequence replicas in lockstep (round 3; reference dynaboa_benchmark.py:126-193 per sequence):
 * every launch - teacher forward, history-frame pass, exemplar pass, the feature cosines - covers all active replicas.  The
 * dynamic-BOA gate is decided PER replica: a replica whose feature 12 has stopped moving leaves the launch set of the remaining
 * iterations, so replicas take different numbers of Adam steps (per-replica step counts: get_i "adam_step_<r>").  inputs: HOST
 * array of 12 x replicas device pointers, kind-major - inputs[kind * replicas + r] in the order of dyb_stepper_adapt_frame_full,
 * r the physical replica (entries of inactive replicas ignored; the history pair present for all active replicas or none;
 * exemplars NULL with the per-replica callback set_p "retrieve_rep_fn": int fn(void* user, int level, int replica, const void**
 * ex5)).  teacher / gate_log / feat5_out are [replicas][...] like theta; gate_host 16 floats per replica.  extra_steps: `replicas`
 * ints.  A launch scope holds at most 8 per-replica arenas (workspace, theta, adam_m, adam_v, teacher + the logs): with replicas
 * the four log buffers (records, loss_log, gate_log, feat5_out) must be sub-buffers of ONE per-replica block registered with
 * set_p "logs_base" / set_i "logs_bytes" (replica r's block at logs_base + r * logs_bytes); with separate log pointers the call
 * returns DYB_ERR_UNSUPPORTED rather than alias replicas.  dyb_stepper_adapt_frames (replicas > 1) with "use_side" and
 * "group_side" issues the frame's final inference on `side` itself, from its own copy of the staged inputs, and orders `stream` behind
 * the whole weight update (read outputs / records / result rows behind dyb_stepper_join); the full term set takes no side stream
 * (DYB_ERR_UNSUPPORTED).  dyb_stepper_set_active: the replicas following
 * frame steps cover (ascending physical indices; n = 0: all) - sequences of
 * different lengths: a replica whose stream has ended leaves the set, its weights / Adam state / records stay as they are. */
int dyb_stepper_adapt_frames_full(void* stepper, const void* const* inputs, int record_slot, int loss_slot, int* extra_steps,
                                  dyb_stream_t stream, dyb_stream_t aux);
int dyb_stepper_set_active(void* stepper, const int* idx, int n);
int dyb_stepper_join(void* stepper, dyb_stream_t stream);
const float* dyb_stepper_output(const void* stepper, int which);
/* Result ring (set_p "results", set_i "result_capacity"; get_i "result_floats" = B * 20900 floats per row): with `results` set, every
 * final inference of a frame step - the one behind the optimiser step, each step of the dynamic loop (under the scope of the
 * replicas still adapting), the owed one on the side stream - is packed into row `loss_slot mod result_capacity` of each replica
 * of that launch's scope, stream-ordered behind the inference it copies (no allocation, no synchronisation, no new stream; works
 * with metrics = 0).  Later steps of the frame overwrite: what stays is each replica's own last inference, whichever activation
 * arena it lived in; an inactive replica or one that has left the dynamic loop is not written.  results is [replicas]
 * [result_capacity][result_floats]; with replicas > 1 it must be a FIFTH sub-buffer of the one per-replica logs block (a launch
 * scope holds at most 8 arenas): outside it the step returns DYB_ERR_UNSUPPORTED, and results with result_capacity <= 0 is
 * DYB_ERR_ARG, both before any launch.  Read a row after dyb_stepper_join when a side stream is in use.
 * dyb_result_pack packs one inference into one row by one kernel: per sample verts [6890][3] | rotmat [24][9] | beta [10] | cam [3]
 * (s, tx, ty) | 1 pad float that is never written (20900 floats, a multiple of 16 bytes).  rotmat [B][24][9], state [B][160] (shape
 * at 144, cam at 154), verts [B][6890][3] (8-byte aligned), out [B][20900] (16-byte aligned). */
int dyb_result_pack(const float* rotmat, const float* state, const float* verts, float* out, int B, dyb_stream_t stream);

/* Device-resident exemplar bank (csrc/retrieval.hip; reference base_adaptor.py:82-96 without the host): dyb_retrieve_select picks,
 * for each of nrows feature rows of 2048 floats, the centre with the largest cos_k = dot(x, c_k) * center_inv_norm[k] (ties: the
 * LOWEST index; independent of `chunk`, the centres per workgroup, <= 0 = 16) and draws a member of that cluster:
 * w = first word of philox4x32_10(counter = (draw lo, draw hi, sample, 0), key = (seed lo, seed hi)),
 * item = member_idx[member_ptr[c] + mulhi32(w, member_ptr[c + 1] - member_ptr[c])].  Row i belongs to "physical replica" rows[i]
 * (HOST array, 0 .. 63, nrows <= 64): its feature is at feat + rows[i] * feat_stride BYTES (16-byte aligned), its draw index
 * draws[rows[i]] (HOST array indexed by replica), its pick log at picks + rows[i] * picks_stride bytes - [pick_capacity][2] int32,
 * row (draw mod pick_capacity) receives (cluster, item).  No allocation; stream ordered; check == 0 never synchronises and an empty
 * nearest cluster (or tables pointing outside the bank) leaves item -1 in the log; check != 0 waits for the stream and returns
 * DYB_ERR_ARG for such a row.  K <= 0, n_items <= 0, more than 64 rows: DYB_ERR_ARG.
 * dyb_exemplar_gather copies, for each row, bank item picks[r][draws[r] mod pick_capacity][1] into the replica's five exemplar
 * inputs: dst5 / dst_stride5 are HOST arrays of replica 0's destinations (img [3][224][224], keypoints [49][3], pose [72], betas
 * [10], pose_3d [24][4]; img 16-byte aligned) and the bytes between consecutive replicas.  Rows whose logged item is outside
 * [0, n_items) are left untouched. */
size_t dyb_retrieve_workspace_bytes(int rows, int K, int chunk);
int dyb_retrieve_select(const float* feat, size_t feat_stride, const int* rows, int nrows, const float* centers,
                        const float* center_inv_norm, int K, const int* member_ptr, const int* member_idx, int n_members,
                        int n_items, const unsigned long long* draws, unsigned long long seed, int sample, int* picks,
                        size_t picks_stride, int pick_capacity, int chunk, int check, void* ws, size_t ws_bytes,
                        dyb_stream_t stream);
int dyb_exemplar_gather(const int* picks, size_t picks_stride, int pick_capacity, const int* rows, int nrows,
                        const unsigned long long* draws, const float* img, const float* kp, const float* pose, const float* betas,
                        const float* pose3d, int n_items, float* const* dst5, const size_t* dst_stride5, dyb_stream_t stream);

/* Spherical k-means for building the retrieval index (csrc/kmeans.hip; dynaboa_amd/retrieval_index.py drives the Lloyd loop).
 * x: N rows of D floats, row i at x + i * x_stride_bytes (16-byte aligned base and pitch, pitch >= 4 D); centers [K][D] contiguous,
 * un-normalised.  Shapes: N >= 1, D a multiple of 32, 1 <= K <= 1024 - otherwise DYB_ERR_UNSUPPORTED (D, K) or DYB_ERR_ARG, before
 * any launch and with every output untouched; a workspace smaller than the matching *_workspace_bytes is DYB_ERR_WORKSPACE.  No
 * allocation, stream ordered, no synchronisation.
 * dyb_rows_inv_norm: inv_norm[i] = 1 / max(|x_i|, 1e-8), the clamp of torch.cosine_similarity.
 * dyb_kmeans_assign: assign[i] = the centre of highest cosine (dot(x_i, c_k) * x_inv_norm[i]) * center_inv_norm[k], ties to the
 * LOWEST index (the rule of dyb_retrieve_select); best[i] = that cosine; changed[0] = rows whose assign differs from the value
 * passed in (assign is read and rewritten: fill it with -1 before the first call); counts[k] = members of k; ws = one fp64 partial
 * sum of best per 128 rows (ceil(N / 128) doubles, rows in order): the host adds them in index order for the objective.
 * dyb_kmeans_update: centers[k] = (sum over members of x_i * x_inv_norm[i]) / counts[k]; counts[k] <= 0 leaves row k as it is.  No
 * floating-point atomics: the summation order depends on (N, D, K) only, two calls return equal bytes.  counts must match assign
 * (the host may have corrected both for empty clusters); entries of assign outside 0 .. K - 1 belong to no cluster. */
int dyb_rows_inv_norm(const float* x, size_t x_stride_bytes, int N, int D, float* inv_norm, dyb_stream_t stream);
size_t dyb_kmeans_assign_workspace_bytes(int N, int D, int K);
int dyb_kmeans_assign(const float* x, size_t x_stride_bytes, const float* x_inv_norm, int N, int D, const float* centers,
                      const float* center_inv_norm, int K, int* assign, float* best, int* changed, int* counts, void* ws,
                      size_t ws_bytes, dyb_stream_t stream);
size_t dyb_kmeans_update_workspace_bytes(int N, int D, int K);
int dyb_kmeans_update(const float* x, size_t x_stride_bytes, const float* x_inv_norm, int N, int D, const int* assign,
                      const int* counts, int K, float* centers, void* ws, size_t ws_bytes, dyb_stream_t stream);

/* HMR in train() mode: nn.Dropout(p) after fc1 / fc2 of every regressor iteration (reference model/hmr.py:84,86,165,169 -
 * the reference's mean teacher runs like this, base_adaptor.py:151-158 never calls teacher.eval()).  Masks are
 * counter-based (Philox-4x32-10) functions of (seed, offset, iteration, element): a backward regenerates them from the same
 * pair.  dyb_hmr_feature_info_ex(train = 1) locates the post-dropout hidden vectors (features 7+3t). */
int dyb_hmr_forward_train(void* plan, const float* params, const float* image_nchw, const float* init_state, int n_iter,
                          float* acts, void* ws, size_t ws_bytes, unsigned long long seed, unsigned long long offset, float p,
                          dyb_stream_t stream);
int dyb_hmr_backward_train(void* plan, const float* params, const float* acts, const float* d_rotmat, const float* d_state,
                           int n_iter, float* grads, void* ws, size_t ws_bytes, unsigned long long seed,
                           unsigned long long offset, float p, dyb_stream_t stream, dyb_stream_t aux_stream);
int dyb_hmr_feature_info_ex(const void* plan, int which, int train, long long* offset, int* dims4, int* row_stride);

/* ---- SMPLify (reference utils/smplify/): the optimisation-based fitter on the device (csrc/smplify.hip).  One workgroup per sample,
 * fixed reduction order; nothing couples the samples of a batch.  kp2d is [B][49][3] = (x, y, confidence) in pixels.
 * dyb_rodrigues_bwd: the gradient of dyb_rodrigues_fwd exactly as that kernel is written (angle = ||r + 1e-8||, un-normalised axis
 * r / angle), finite and equal to autograd of the formula at r = 0. */
int dyb_rodrigues_bwd(const float* axis_angle, const float* drotmat, float* daxis_angle, int n, dyb_stream_t stream);
/* camera_fitting_loss (utils/smplify/losses.py:83-113; defaults focal 5000, depth_weight 100): loss [B], djoints49 [B][49][3],
 * dcam_t [B][3].  The OpenPose torso joints are used when all four of their confidences are > 0, else the ground-truth-style ones. */
int dyb_smplify_camera_loss(const float* joints49, const float* cam_t, const float* cam_t_est, const float* center, const float* kp2d,
                            float focal, float depth_weight, float* loss, float* djoints49, float* dcam_t, int B, dyb_stream_t stream);
/* body_fitting_loss (losses.py:49-81; defaults focal 5000, sigma 100, weights 4.78 / 5 / 15.2): parts [B][5] = (reprojection sum,
 * pose prior, angle prior, shape prior, total), reproj [B][49] (what output='reprojection' returns), total_out [B] (may be NULL);
 * gradients djoints49 [B][49][3], dpose69 [B][lddp], dbetas [B][lddb], dcam_t [B][3] (may be NULL).  ignore != 0: the five joints of
 * smplify.py:31 count with confidence 0 (kp2d itself is never written). */
int dyb_smplify_body_loss(const float* pose69, int ldp, const float* betas, int ldb, const float* joints49, const float* cam_t,
                          const float* center, const float* kp2d, const float* gmm_means, const float* gmm_prec, const float* gmm_logw,
                          float focal, float sigma, float pose_prior_weight, float shape_prior_weight, float angle_prior_weight, int ignore,
                          float* parts, float* reproj, float* total_out, float* djoints49, float* dpose69, int lddp, float* dbetas, int lddb,
                          float* dcam_t, int B, dyb_stream_t stream);
/* torch.optim.Adam over the per-sample vector pose 72 | betas 10 | camera 3.  group 1: global orientation + camera (stage 1),
 * group 2: body pose + betas + global orientation (stage 2).  A gradient is g (+ its *_extra where given).  state (m | v | step
 * count per sample) is dyb_smplify_adam_state_bytes(B); restart != 0 starts from zero moments and step 0. */
size_t dyb_smplify_adam_state_bytes(int B);
int dyb_smplify_adam(float* pose, int ldp, float* betas, int ldb, float* cam_t, const float* dpose, const float* dbody_extra, int lddx,
                     const float* dbetas, const float* dbetas_extra, int lddbx, const float* dcam_t, void* state, size_t state_bytes,
                     int group, int restart, double lr, double beta1, double beta2, double eps, int B, dyb_stream_t stream);
/* SMPLify.__call__ (smplify.py:43-139) in one call on one stream, no host synchronisation: num_iters iterations of the camera loss
 * over {global orientation, camera}, num_iters of the body loss over {body pose, betas, global orientation} (camera fixed, five
 * joints ignored), a final forward.  Per iteration: rodrigues, LBS forward, loss head, LBS backward (joints only), rodrigues
 * backward, Adam.  Outputs verts [B][6890][3], joints49, pose [B][72], betas [B][10], cam_t [B][3], reproj [B][49]; loss_log (may be
 * NULL) [2 * num_iters][B] per-sample totals, each evaluated before its step.  num_iters = 0 evaluates the initial values.  The
 * loss weights are the reference's defaults. */
size_t dyb_smplify_fit_workspace_bytes(int B);
int dyb_smplify_fit(const float* const* tables_f, const int* const* tables_i, const float* gmm_means, const float* gmm_prec,
                    const float* gmm_logw, const float* init_pose, const float* init_betas, const float* init_cam_t, const float* center,
                    const float* kp2d, int num_iters, double lr, float focal, float* verts, float* joints49, float* pose, float* betas,
                    float* cam_t, float* reproj, float* loss_log, int B, void* ws, size_t ws_bytes, dyb_stream_t stream);

/* ---- 3DPW extraction (reference utils/data_preprocess/pw3d.py; csrc/pw3d_extract.hip): the annotations of n person-frames in one
 * launch.  Inputs: joints49 fp32 [n][49][3] (SMPL joints, world coordinates, before translation), trans fp64 [n][3], cam_pose fp64
 * [n][4][4], cam_intrinsics fp64 [3][3], root_aa fp32 [n][3] (the global orientation as the sequence file stores it).  Outputs:
 * j2d fp64 [n][49][3] = (u, v, 1) with p = (float)((double)joint + trans) rounded once to fp32 and everything after it in fp64
 * (q = cam_pose[:3, :] . (p, 1), q /= q.z, uv = (K . q).xy; no special case for q.z <= 0); center fp64 [n][2] and scale fp64 [n] of
 * the box of the 49 projections (midpoint; max(width, height) / 200); root_aligned fp32 [n][3] =
 * rotation_matrix_to_angle_axis(fp32(cam_pose[:3, :3]) . batch_rodrigues(root_aa)), both through the quaternion forms of
 * utils/geometry.py, in fp32.  DYB_ERR_ARG for a null pointer or n <= 0. */
int dyb_pw3d_annotate(const float* joints49, const double* trans, const double* cam_pose, const double* cam_intrinsics,
                      const float* root_aa, double* j2d, double* center, double* scale, float* root_aligned, int n,
                      dyb_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
