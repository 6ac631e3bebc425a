// Native frame stepper: ONE C call per adapted frame.
//
// The per-frame bilevel schedule of reference dynaboa_benchmark.py:126-193 (Adaptor.adaptation) - clone, inner_step x
// [lower-level loss -> learner.adapt -> inference], upper-level loss through the fast weights, zero_grad / backward /
// Adam.step, inference - issued from C++ over the engine (hmr_engine.hip), the SMPL kernels (smpl_lbs.hip), the loss
// head (losses.hip) and the flat-arena updates (optim.hip).  The Python Adaptor (dynaboa_amd/benchmark.py) stays the
// surface; in the configurations this file covers it forwards a frame here instead of walking the same ~1700 launches
// through torch.autograd + ctypes (9 ms of host time per frame there, ~2.5 us per launch here).  One stepper can also
// advance up to DYB_MAX_REPLICAS independent sequences in lockstep ("replicas", dyb_common.h): every launch of the chain
// then covers all of them.  dyb_stepper_* are re-entrant per stepper (own workspace, events, stream ordering).
//
// Same kernels, same order, same operands as the Python path => identical weights / Adam state (tests assert
// bit-equality); the metric reductions (MPJPE / PVE means) are this file's own kernels and agree to rounding.
//
// First-order MAML only (reference base_adaptor.py:119 first_order=True): theta_fast_{k+1} = theta_fast_k - fastlr*g_k,
// outer gradient = gradient of the upper-level loss AT the last fast weights (learn2learn clone() + adapt() with
// first_order=True: SURVEY Appendix B).
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <string>
#include <vector>

#include "dyb_common.h"
#include "dyb_stepper_options.h"

extern "C" {
size_t dyb_hmr_param_floats(const void*);
size_t dyb_hmr_act_floats(const void*);
size_t dyb_hmr_workspace_bytes(const void*);
int dyb_hmr_forward_train(void*, const float*, const float*, const float*, int, float*, void*, size_t, unsigned long long, unsigned long long, float,
                          hipStream_t);
long long dyb_hmr_act_offset_rotmat(const void*);
long long dyb_hmr_act_offset_state(const void*);
size_t dyb_lbs_saved_floats(int);
size_t dyb_lbs_bwd_workspace_bytes(int);
int dyb_lbs_fwd(const float* const*, const int* const*, const float*, int, const float*, float*, float*, float*, int, hipStream_t);
int dyb_lbs_bwd(const float* const*, const int* const*, const float*, const float*, const float*, const float*, float*, float*, int,
                int, void*, size_t, hipStream_t);
int dyb_regress_joints(const float*, const float*, float*, int, int, hipStream_t);
int dyb_rodrigues_fwd(const float*, float*, int, hipStream_t);
int dyb_frame_losses_kp(const float*, const float*, int, const float*, int, const float*, const float*, const float*, const float*,
                        const float*, float, float, float, float*, float*, float*, int, float*, int, float*, int, int, void*, size_t,
                        hipStream_t);
int dyb_scale_add(const float*, const float*, const float*, float*, size_t, hipStream_t);
int dyb_head_grad_combine(const float*, const float*, const float*, const float*, const float*, const float*, const float*,
                          const float*, const float*, float*, float*, int, hipStream_t);
int dyb_fastweight_update(const float*, const float*, float*, float, size_t, hipStream_t);
int dyb_adam_step(float*, const float*, float*, float*, float, float, float, float, float, size_t, hipStream_t);
int dyb_ema_update(float*, const float*, float, size_t, hipStream_t);
int dyb_axpby(const float*, float*, float, float, size_t, hipStream_t);
int dyb_aux_loss_terms_kp(int, int, int, float, const float*, const float*, int, const float*, int, const float*, const float*,
                          const float*, int, const float*, int, const float*, const float*, const float*, const float*, const float*,
                          const float*, float*, float*, float*, float*, float*, float*, float*, int, hipStream_t);
int dyb_hmr_feature_info(const void*, int, long long*, int*, int*);
size_t dyb_retrieve_workspace_bytes(int, int, int);
int dyb_retrieve_select(const float*, size_t, const int*, int, const float*, const float*, int, const int*, const int*, int, int,
                        const unsigned long long*, unsigned long long, int, int*, size_t, int, int, int, void*, size_t, hipStream_t);
int dyb_exemplar_gather(const int*, size_t, int, const int*, int, const unsigned long long*, const float*, const float*, const float*,
                        const float*, const float*, int, float* const*, const size_t*, hipStream_t);
}
int dyb_adam_step_rep(float*, const float*, float*, float*, float, float, const float*, const float*, float, size_t, hipStream_t);   // optim.hip
int dyb_adam_step_rep3(float*, const float*, const float*, const float*, float*, float*, float, float, const float*, const float*, float, size_t,
                       hipStream_t);
int dyb_fastweight_update3(const float*, const float*, const float*, const float*, float*, float, size_t, hipStream_t);
int dyb_fastweight_update_segs(const float*, const float*, float*, float, const DybFwSegs&, hipStream_t);       // optim.hip
int dyb_adam_step_rep3_ema(float*, const float*, const float*, const float*, float*, float*, float, float, const float*, const float*, float, size_t,
                           float*, float, hipStream_t);
int dyb_adam_step_segs(float*, const float*, float*, float*, float, float, const float*, const float*, float, const DybFwSegs&, hipStream_t);
int dyb_adam_write_scalars(float*, const float*, const float*, hipStream_t);

#define STATE_LD 160
#define NV 6890
#define NJ 49
#define RUN(x)                       \
  do {                               \
    int rc__ = (x);                  \
    if (rc__ != DYB_OK) return rc__; \
  } while (0)
#define HIPOK(x)                                  \
  do {                                            \
    if ((x) != hipSuccess) return DYB_ERR_LAUNCH; \
  } while (0)

// ---- metric record of one inference() (reference dynaboa_benchmark.py:204-262) ----------------------------------------
// pred17 / gt17m / gt17f: J_regressor_h36m @ vertices [B][17][3]; rec = pred14[B][14][3] | gt14[B][14][3] | mpjpe[B] | pve.
// pred14 = joints[H36M_TO_J14] - joints[0] (pelvis), gt from the male or the female mesh by gender (:221-233);
// mpjpe = mean_j |pred14 - gt14| (:236), pve = mean over batch and vertices of |gt_neutral - pred| (:244).
// PA-MPJPE needs an SVD per sample and is evaluated over all records at once (dyb_pa_mpjpe) when they are read.
__global__ __launch_bounds__(256) void metric_record_kernel(const float* __restrict__ pred17, const float* __restrict__ gt17m,
                                                            const float* __restrict__ gt17f, const long long* __restrict__ gender,
                                                            const int* __restrict__ j14, const float* __restrict__ pverts,
                                                            const float* __restrict__ gverts, float* __restrict__ rec, int B,
                                                            DybRep Rp) {
  DYB_REP_PROLOGUE(Rp);
  DYB_RB(Rp, pred17); DYB_RB(Rp, gt17m); DYB_RB(Rp, gt17f); DYB_RB(Rp, gender); DYB_RB(Rp, pverts); DYB_RB(Rp, gverts); DYB_RB(Rp, rec);
  __shared__ float s_err[64 * 14];
  __shared__ float s_red[4];
  const int t = threadIdx.x;
  float* pred14 = rec;
  float* gt14 = rec + (size_t)B * 42;
  float* mpjpe = rec + (size_t)B * 84;
  float* pve = mpjpe + B;
  for (int i = t; i < B * 14; i += 256) {
    const int b = i / 14, j = i - b * 14, src = j14[j];
    const float* g17 = (gender[b] == 1 ? gt17f : gt17m) + (size_t)b * 51;
    const float* p17 = pred17 + (size_t)b * 51;
    float e2 = 0.f;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float p = p17[src * 3 + c] - p17[c], g = g17[src * 3 + c] - g17[c];
      pred14[i * 3 + c] = p;
      gt14[i * 3 + c] = g;
      e2 += (p - g) * (p - g);
    }
    s_err[i] = sqrtf(e2);
  }
  float acc = 0.f;
  const int nv = B * NV;
  for (int i = t; i < nv; i += 256) {
    const float dx = gverts[i * 3] - pverts[i * 3], dy = gverts[i * 3 + 1] - pverts[i * 3 + 1], dz = gverts[i * 3 + 2] - pverts[i * 3 + 2];
    acc += sqrtf(dx * dx + dy * dy + dz * dz);
  }
  acc = dyb_wave_sum(acc);
  if ((t & 63) == 0) s_red[t >> 6] = acc;
  __syncthreads();
  if (t < B) {
    float s = 0.f;
    for (int j = 0; j < 14; ++j) s += s_err[t * 14 + j];
    mpjpe[t] = s / 14.f;
  }
  if (t == 0) pve[0] = ((s_red[0] + s_red[1]) + (s_red[2] + s_red[3])) / (float)nv;
}

// dst[0..3] = src[0..3] (a level's loss 4-vector into the frame's log row; replica-aware, unlike a device-to-device memcpy)
__global__ void copy4_kernel(const float* __restrict__ src, float* __restrict__ dst, DybRep Rp) {
  DYB_REP_PROLOGUE(Rp);
  DYB_RB(Rp, src); DYB_RB(Rp, dst);
  if (threadIdx.x < 4) dst[threadIdx.x] = src[threadIdx.x];
}
// the 16-float log row of one level of the full loss set: frame {s2d, shape prior, pose prior, total} | teacher {s2d, s3d, shape,
// pose, loss} | motion | labelled {s2d, s3d, shape, pose, loss} | level total = frame + wt*teacher + wm*motion + wl*labelled
__global__ void level_log_kernel(const float* __restrict__ frame4, const float* __restrict__ teach5, const float* __restrict__ motion5,
                                 const float* __restrict__ label5, float wt, float wm, float wl, float* __restrict__ row16, DybRep Rp) {
  DYB_REP_PROLOGUE(Rp);
  DYB_RB(Rp, frame4); DYB_RB(Rp, teach5); DYB_RB(Rp, motion5); DYB_RB(Rp, label5); DYB_RB(Rp, row16);
  if (threadIdx.x != 0) return;
  float total = frame4[3];
  for (int i = 0; i < 4; ++i) row16[i] = frame4[i];
  for (int i = 0; i < 5; ++i) row16[4 + i] = teach5 ? teach5[i] : 0.f;
  row16[9] = motion5 ? motion5[4] : 0.f;
  for (int i = 0; i < 5; ++i) row16[10 + i] = label5 ? label5[i] : 0.f;
  if (teach5) total += wt * teach5[4];
  if (motion5) total += wm * motion5[4];
  if (label5) total += wl * label5[4];
  row16[15] = total;
}
// cal_feature_diff (reference base_adaptor.py:211-219): cosine of each of the 15 feature pairs (flattened), one workgroup per
// feature; out[f] = cos_f, and - workgroup 12, the gate feature - the sequence number `seq` into out[15] AFTER its cosine, so a
// host that polls out[15] (device-visible pinned memory) reads a complete out[12].
struct FeatCosArgs {
  long long off[15];
  int rows[15], cols[15], ld[15];
};
__global__ __launch_bounds__(1024) void feat_cos_kernel(const float* __restrict__ A, const float* __restrict__ Bp, FeatCosArgs fa,
                                                        float eps, float* __restrict__ out_dev, volatile float* out_host, float seq,
                                                        DybRep Rp) {
  DYB_REP_PROLOGUE(Rp);
  DYB_RB(Rp, A); DYB_RB(Rp, Bp); DYB_RB(Rp, out_dev);
  if (out_host) out_host += 16 * dyb_rep;             // pinned host memory: 16 floats per physical replica
  // The three sums are accumulated in double (round 6): 1 - cos of feature 12 is ~1e-4 and the gate compares it with a threshold to a
  // few per cent, i.e. cos must be good to ~1e-6 - an fp32 sum over 2e5 ... 8e5 elements is not (torch's own fp32 evaluation returns
  // 1.000017 for feature 0: tests compare against the float64 evaluation of the reference's features, golden key gate_cos64)
  __shared__ double sm[16][3];
  const int f = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const float* a = A + fa.off[f];
  const float* b = Bp + fa.off[f];
  const long long n = (long long)fa.rows[f] * fa.cols[f];
  double ab = 0.0, aa = 0.0, bb = 0.0;
  for (long long i = t; i < n; i += 1024) {
    const long long r = i / fa.cols[f], c = i - r * fa.cols[f];
    const double x = (double)a[r * fa.ld[f] + c], y = (double)b[r * fa.ld[f] + c];
    ab += x * y; aa += x * x; bb += y * y;
  }
  for (int m = 32; m >= 1; m >>= 1) { ab += __shfl_xor(ab, m); aa += __shfl_xor(aa, m); bb += __shfl_xor(bb, m); }
  if (lane == 0) { sm[wave][0] = ab; sm[wave][1] = aa; sm[wave][2] = bb; }
  __syncthreads();
  if (t == 0) {
    double x = 0.0, y = 0.0, z = 0.0;
    for (int w = 0; w < 16; ++w) { x += sm[w][0]; y += sm[w][1]; z += sm[w][2]; }
    // torch cosine_similarity: x.y / (max(|x|, eps) max(|y|, eps)), rounded to fp32 once
    const float cs = (float)(x / (fmax(sqrt(y), (double)eps) * fmax(sqrt(z), (double)eps)));
    out_dev[f] = cs;
    if (out_host) {
      out_host[f] = cs;
      if (f == 12) {
        __threadfence_system();
        out_host[15] = seq;
      }
    }
  }
}

// ---- result ring: one final inference packed into one row ------------------------------------------------------------------
// Row layout per sample (RESULT_FLOATS = 20900 floats, a multiple of 16 bytes): verts [6890][3] | rotmat [24][9] | beta [10] | cam [3]
// (s, tx, ty) | 1 pad float (never written).  One launch covers every sample and every replica of the launch scope (rotmat / state /
// verts lie in the replicas' workspaces, `out` in their log blocks: rebased like every other pointer).  The vertex body moves as
// 16-byte stores fed by 16-byte loads where the sample's vertices are 16-byte aligned (even samples: a sample's vertices start at
// b * 20670 floats) and by two 8-byte loads otherwise; the 232-float tail (2 vertex floats, rotmat, beta, cam) goes float by float.
#define RESULT_FLOATS 20900
#define RESULT_BODY4 5167                   // float4 units of the vertex block (20668 of its 20670 floats)
__global__ __launch_bounds__(256) void result_pack_kernel(const float* __restrict__ rotmat, const float* __restrict__ state,
                                                          const float* __restrict__ verts, float* __restrict__ out, DybRep Rp) {
  DYB_REP_PROLOGUE(Rp);
  DYB_RB(Rp, rotmat); DYB_RB(Rp, state); DYB_RB(Rp, verts); DYB_RB(Rp, out);
  const int b = blockIdx.y;
  const float* v = verts + (size_t)b * NV * 3;
  float* o = out + (size_t)b * RESULT_FLOATS;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < RESULT_BODY4) {
    float4 x;
    if (((uintptr_t)v & 15) == 0) {
      x = reinterpret_cast<const float4*>(v)[i];
    } else {
      const float2 lo = reinterpret_cast<const float2*>(v)[2 * i], hi = reinterpret_cast<const float2*>(v)[2 * i + 1];
      x = make_float4(lo.x, lo.y, hi.x, hi.y);
    }
    reinterpret_cast<float4*>(o)[i] = x;
  } else if (i < RESULT_BODY4 + 231) {
    const int k = i - RESULT_BODY4;            // 0, 1: the last two vertex floats | 2 .. 217 rotmat | 218 .. 227 beta | 228 .. 230 cam
    float x;
    if (k < 2) x = v[4 * RESULT_BODY4 + k];
    else if (k < 218) x = rotmat[(size_t)b * 216 + (k - 2)];
    else x = state[(size_t)b * STATE_LD + 144 + (k - 218)];       // shape at 144 .. 153, cam at 154 .. 156
    o[4 * RESULT_BODY4 + k] = x;
  }
}
// rotmat [B][24][9], state [B][160] (shape at 144, cam at 154), verts [B][6890][3] -> out [B][20900]; verts 8-byte, out 16-byte aligned
extern "C" int dyb_result_pack(const float* rotmat, const float* state, const float* verts, float* out, int B, hipStream_t st) {
  DYB_REQUIRE(rotmat && state && verts && out && B > 0 && B <= 64, DYB_ERR_ARG);
  DYB_REQUIRE(((uintptr_t)verts & 7) == 0 && ((uintptr_t)out & 15) == 0, DYB_ERR_ARG);
  const DybRep& Rp = dyb_rep_current();
  hipLaunchKernelGGL(result_pack_kernel, dim3(dyb_cdiv(RESULT_BODY4 + 231, 256), B, Rp.n), dim3(256), 0, st, rotmat, state, verts, out, Rp);
  DYB_CHECK_LAUNCH();
  return DYB_OK;
}

// replica r's frame inputs (separate caller tensors) into its staging area inside the workspace, one launch for all replicas
struct GatherArgs {
  const float* src[5][DYB_MAX_REPLICAS];     // up to five inputs per launch, per PHYSICAL replica (e.g. image, kp2d, gt_pose, gt_betas,
                                             // gender - int64 viewed as 2 floats); NULL: nothing to copy
  float* dst[5];                             // replica 0's staging buffers
  unsigned n[5];                             // floats per input
};
__global__ __launch_bounds__(256) void gather_inputs_kernel(GatherArgs a, DybRep Rp) {
  DYB_REP_PROLOGUE(Rp);
  const int k = blockIdx.y;
  const float* src = a.src[k][dyb_rep];
  if (!src) return;
  float* dst = a.dst[k];
  DYB_RB(Rp, dst);
  for (unsigned i = blockIdx.x * 256 + threadIdx.x; i < a.n[k]; i += gridDim.x * 256) dst[i] = src[i];
}

// ---- one forward (+ backward) of HMR -> SMPL -> loss head ---------------------------------------------------------------
struct Pass {
  float* acts;
  char* ws;                 // engine workspace of the chain this pass runs on
  float *verts, *joints, *saved;
  float *losses, *drot_l, *dshape_l, *dcam_l, *djoints_l, *lws;      // dyb_frame_losses outputs
  float *djoints, *drot_s, *dbetas_s;                                // gradient assembly
  char* lbs_ws;
  float *d_rot, *d_state;
  float* pred17;
};

struct Stepper {
  void* plan = nullptr;
  int B = 1, H = 224, W = 224;
  size_t n_params = 0, act_floats = 0, ws_bytes = 0, off_rot = 0, off_state = 0, lbs_saved = 0, lbs_wsb = 0;
  // options (doubles: the Python floats, so host-side scalars round exactly as in dynaboa_amd/optim.py / maml.py)
  int n_iter = 3, inner_step = 1, eval_lower = 1, use_side = 0, metrics = 1;
  // the full loss set (reference defaults): teacher / motion / labelled-exemplar terms, dynamic-BOA gate
  int full = 0, temporal_lower = 0, temporal_upper = 1, use_teacher = 1, use_motion = 1, interval = 5, mix_lower = 1, mix_upper = 1,
      dynamic = 1, optim_steps = 7;
  int kp_set = 0;                     // keypoint window of the frame head's 2-D term and of the motion term: 0 gt24 | 1 op25 (losses.hip)
  double teacher_w = 0.1, motion_w = 0.8, label_w = 0.1, alpha = 0.1, cos_thr = 3.1e-4;
  float* teacher = nullptr;           // teacher parameter arena (caller's)
  // train-mode teacher (the reference never calls teacher.eval(): base_adaptor.py:151-158 - its teacher forwards run with live
  // nn.Dropout(0.5) after fc1 / fc2, model/hmr.py:84,86): every teacher forward of a frame draws the masks of (drop_seed, drop_off + k),
  // k = teacher forwards issued since "drop_offset" was set - the same counter-based keys dynaboa_amd.hmr hands the autograd path
  int teacher_train = 0;
  unsigned long long drop_seed = 0, drop_off = 0;
  long long drop_used = 0;
  double drop_p = 0.5;
  volatile float* gate_host = nullptr;   // 16 floats of device-visible pinned host memory (caller's): 15 cosines + sequence number
  float* gate_log = nullptr;          // device: [loss_capacity][1 + optim_steps][16] cosines of every gate evaluation
  float* feat5_out = nullptr;         // [B][2048] the level's pooled feature for the retrieval callback
  int (*retrieve)(void*, int, const void**) = nullptr;
  int (*retrieve_rep)(void*, int, int, const void**) = nullptr;     // replica groups: (user, level, physical replica, out[5])
  void* retrieve_user = nullptr;
  // Exemplar bank (retrieval.hip): the whole retrieval set resident on the device (caller's tables).  Bound (all pointers set,
  // "bank_on_device" 1), a level with a labelled term selects each replica's nearest cluster from its own pooled feature on the chain,
  // draws a member and gathers that exemplar into the replica's exemplar staging - no host callback, so the parallel passes stay on.
  // The draw index is host state: bank_draw[r] counts the labelled levels issued for physical replica r (the dynamic gate is a host
  // poll, so the host knows), handed to the kernels as arguments and logged in bank_picks row (draw mod bank_pick_capacity).
  const float *bank_img = nullptr, *bank_kp = nullptr, *bank_pose = nullptr, *bank_betas = nullptr, *bank_pose3d = nullptr;
  const float *bank_centers = nullptr, *bank_inv_norm = nullptr;
  const int *bank_member_ptr = nullptr, *bank_member_idx = nullptr;
  int* bank_picks = nullptr;
  int bank_items = 0, bank_clusters = 0, bank_members = 0, bank_pick_capacity = 0, bank_on_device = 1;
  unsigned long long bank_seed = 0;
  unsigned long long bank_draw[DYB_MAX_REPLICAS] = {};
  char* retr_ws = nullptr;            // select partials (replica 0's blob: sized for every replica of the handle)
  FeatCosArgs fca{};
  float gate_seq = 0.f;
  Pass lvl0{}, ex{}, hist{}, teach{};
  float *grads2 = nullptr, *grads3 = nullptr, *zeros = nullptr, *ex_rot = nullptr;
  const float *lvl_g2 = nullptr, *lvl_g3 = nullptr;      // the current level's further gradient arenas (history pass, exemplar pass): summed by the update
  float *ext_rot = nullptr, *ext_shape = nullptr, *ext_cam = nullptr, *ext_joints = nullptr;     // aux-term gradients on the image pass
  float *exg_rot = nullptr, *exg_shape = nullptr, *exg_cam = nullptr, *exg_joints = nullptr;     // ... on the exemplar pass
  float *hg_cam = nullptr, *hg_joints = nullptr;                                                 // ... on the history pass
  float *vals_t = nullptr, *vals_m = nullptr, *vals_l = nullptr;
  int nrep = 1;                       // sequence replicas stepped in lockstep by every launch (dyb_common.h)
  int active[DYB_MAX_REPLICAS] = {};  // the replicas the next frame step covers (physical indices, ascending); default: all
  int nactive = 0;                    // 0 = all
  long long adam_t_rep[DYB_MAX_REPLICAS] = {};   // Adam steps taken, per replica (they differ once the dynamic loop or ragged streams do)
  size_t blob = 0;                    // workspace bytes of ONE replica
  float* in_stage[12] = {};           // staging of the frame inputs, in IN_* order (replica 0): all kinds for nrep > 1; one sequence: only
                                      // the exemplar kinds, and only with an exemplar bank set before the workspace is sized
  float* in_stage_alt[5] = {};        // replica groups, frame-loss set: the second copy of the first five kinds.  Every call stages into
                                      // the copy the previous call did not use: a final inference on the side stream ("group_side") keeps
                                      // reading its own frame
  double lr = 3e-6, beta1 = 0.5, beta2 = 0.9, eps = 1e-8, fastlr = 8e-6, w2d = 10.0, wshape = 2e-6, wpose = 1e-4;
  long long adam_t = 0;
  // caller-owned state and tables (device pointers)
  float *theta = nullptr, *adam_m = nullptr, *adam_v = nullptr;
  const float* init_state = nullptr;
  const float* smpl_f[3][7] = {};         // neutral, male, female: the dyb_lbs_fwd table order
  const int* smpl_i[3][3] = {};
  const float *gmm_means = nullptr, *gmm_prec = nullptr, *gmm_logw = nullptr, *j_h36m = nullptr;
  const int* j14 = nullptr;
  float *records = nullptr, *loss_log = nullptr;
  const char* logs_base = nullptr;    // replica 0's block holding records | loss_log | gate_log | feat5_out (one replica arena for all four)
  size_t logs_bytes = 0;
  int record_capacity = 0, loss_capacity = 0;
  // result ring (caller's; with replicas a fifth sub-buffer of the logs block): every final inference of a frame step is packed into
  // row `loss_slot mod result_capacity` of each replica in that launch's scope, stream-ordered behind the inference - later steps of
  // the frame overwrite, so what stays is each replica's own LAST inference, whichever activation arena it lived in
  float* results = nullptr;
  int result_capacity = 0;
  // workspace
  char* wsp = nullptr;
  bool bound = false;
  Pass main{}, fin{};
  float *theta_fast = nullptr, *grads = nullptr;
  // "fuse_fast" (round 6; frame-loss path): a lower level's unsplit throughput-form weight gradients write theta_next = theta_cur - fastlr * g
  // straight from their accumulators (DybWgradUpdateScope, igemm_conv.hip) - those spans never see a gradient in HBM nor the streaming
  // fast-weight pass, which covers what is left (fused_spans -> upd_spans).  theta_cur and theta_next must then be different buffers (a
  // layer's data gradient reads theta_cur on the chain while its weight gradient writes on the auxiliary stream): the levels ping-pong
  // between theta_fast and theta_fast2.
  float* theta_fast2 = nullptr;
  int fuse_fast = 1;
  std::vector<DybSpan> fused_spans, upd_spans;
  // "fuse_adam" (round 6; frame-loss path, replica groups, inner_step >= 1): the OUTER level's unsplit throughput-form weight gradients apply
  // Adam to theta / exp_avg / exp_avg_sq in place from their accumulators (igemm_tp.inc; the level is differentiated at the fast weights,
  // nobody reads theta meanwhile); the streaming Adam pass covers what is left.  The step's bias corrections are fixed BEFORE that
  // backward (adam_prepare) and live, per replica, in adam_sc (two floats of every replica's workspace copy).
  int fuse_adam = 1;
  int fuse_ema = 1;                // the teacher's EMA inside the Adam pass (default term set)
  float* adam_sc = nullptr;
  bool adam_prepared = false;
  float pre_ss[DYB_MAX_REPLICAS], pre_bc[DYB_MAX_REPLICAS];
  float *gt_rot = nullptr, *gt_verts[3] = {}, *gt_joints = nullptr, *gt_saved = nullptr, *gt17[2] = {};
  DybEvents* ev = nullptr;
  hipEvent_t e_theta = nullptr, e_side = nullptr, e_gt = nullptr;
  hipEvent_t e_stage = nullptr;       // replica groups with a side stream: the frame's inputs are staged (on the chain's stream)
  // weight updates by arena ranges beside the next forward ("upd_overlap", replica groups): the fast-weight steps and Adam are
  // streaming passes over [replicas] x 108 MB that nothing overlapped - now the range a forward needs first (stem .. layer2, 5 % of
  // the parameters) is updated on the main stream and the rest (layer3 | layer4 + regressor) on the auxiliary stream while the
  // forward's first layers run; the forward waits for each range right before its first reader (DybFwdGates)
  int upd_overlap = 1;
  // one sequence, full term set: the history pass and the exemplar pass of a level are independent of the frame pass until their gradients
  // are summed - they run on two streams of the stepper's own beside the chain ("par_passes"; batch-1 kernels fill a fraction of the chip)
  int par_passes = 1, par_max_replicas = DYB_MAX_REPLICAS;   // measured up to 32 per launch: 16: 290 -> 316, 32: 362 -> 377 frames/s (s30)
  hipStream_t par_stream[2] = {nullptr, nullptr};                                 // history pass | exemplar pass.  (A third stream for the teacher's
  // forward was measured and removed: 75.7 - 76.9 frames/s against 89.4 - 92.3 with two, profiles/r05_sessions.txt s25.)
  hipEvent_t par_ev[9] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};   // fork | hist fwd | hist head grads | hist bwd | label term | exemplar bwd | error-path tails of the two pass streams | bank select
  bool out_in_main = false;        // where the latest final inference lives (dyb_stepper_output): fin, or main after an odd number of shared steps
  int share_dyn_fwd = 1;           // dynamic loop: an extra step's upper level reuses the previous step's final inference as its forward
  hipEvent_t e_upd = nullptr;
  DybFwdGates gates{};
  bool gates_pending = false;
  // "wgrad_defer" (round 8; wherever the ranged update applies): a chain backward leaves the weight gradients of layer4 (but block 0's
  // conv1 / downsample) and of the regressor - HBM streams with a short matrix prologue - behind its join on the auxiliary stream,
  // where they run beside the NEXT forward's stem .. layer3 instead of beside this backward's GroupNorm backward / data gradients
  // (DybEvents, hmr_engine.hip backward_body).  The events S.ev->l4 / reg order their readers: the consuming forward
  // (gates.l4 / reg) or settle_update for every other consumer.  0 = the issue order of round 7 exactly.  Measured at 32 sequences, three
  // alternating pairs in one session: 493.7 - 495.1 -> 499.8 - 500.9 frames/s (profiles/r08_wgrad_defer_bench.txt).
  int wgrad_defer = 1;
  bool defer_pending = false;      // a deferred set has been issued that no consumer has been ordered behind yet
  int n_deferred = 0;              // launches issued behind a backward's join so far (get_f "deferred_launches": what the tests count)
  int upd_late = 1;                // the last range (layer4 + regressor, 68 % of the parameters) is issued when the forward reaches layer3
  // "group_side" (round 18; replica groups, frame-loss set, with "use_side" and a side stream): the frame's final inference
  // at the updated weights - a whole forward that nothing on the chain consumes - leaves the chain: frame_step issues forward + record +
  // result row on the side stream, where they run beside the end of the outer update and the NEXT frame's first level, and the chain's
  // stream only waits for the update itself (see frame_step; read the outputs behind dyb_stepper_join).  0 = the tail in line, the
  // issue order of round 8 exactly.  Same kernels, same inputs, same split
  // depths either way: the results are the same bits.  Measured at 32 sequences, three alternating runs per arm in one session: 502.5 -
  // 504.0 -> 509.2 - 509.8 frames/s; 8 sequences 276.7 -> 283.8, 64 sequences 556.1 -> 560.9; two groups in one process (six streams on
  // four hardware queues) lost, 459.4 - 460.7 -> 455.4 - 456.4: the Python handle switches it off there (profiles/r18_group_side_bench.txt).
  int group_side = 1;
  // one weight update: the fast-weight step out = p - fastlr * g (adam = false), or Adam in place on theta [+ the teacher's EMA]
  struct Upd {
    bool adam = false, ema = false;
    const float *g2 = nullptr, *g3 = nullptr;      // the level's further gradient arenas, summed by the pass
    const float* p = nullptr;
    float* out = nullptr;
    float ss[DYB_MAX_REPLICAS] = {}, bc[DYB_MAX_REPLICAS] = {};     // Adam's bias corrections by physical replica
  };
  struct LateUpd {                 // what gates.late needs to issue it
    Upd u;
    hipStream_t aux = nullptr;
    DybRep scope{};
  } late;
  size_t grp_bounds[2] = {0, 0};
  bool side_pending = false;
  // the final inference of a frame (side stream) is issued by the NEXT call, behind that frame's first level: the host cannot
  // run far ahead of the GPU (launches block when the queue is full), so issuing ~130 side-stream launches right after Adam
  // left the main queue empty for ~1 ms per frame (profiles/r02_s2_frame_timeline_S1.txt)
  struct Tail {
    bool on = false;
    const float* image = nullptr;
    const long long* gender = nullptr;
    int slot = 0;
    bool metrics = false;
    int loss_slot = -1;
  } tail;
  struct GtJob {
    bool on = false;
    const float *pose = nullptr, *betas = nullptr;
    bool staged = false;           // pose / betas are staged copies written on the chain's stream (e_stage), not the caller's tensors
  } gtjob;
  hipStream_t tail_stream = nullptr;
  std::string err;
  // host-side issue time by section (always on: two clock reads per section), read back through dyb_stepper_get_f
  double h_fwd = 0, h_bwd = 0, h_head = 0, h_update = 0, h_tail = 0, h_total = 0;
  long long h_frames = 0;
};
struct HostTimer {
  double& acc;
  std::chrono::steady_clock::time_point t0;
  explicit HostTimer(double& a) : acc(a), t0(std::chrono::steady_clock::now()) {}
  ~HostTimer() { acc += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); }
};

static size_t a64(size_t v) { return (v + 63) & ~(size_t)63; }
#define BANK_MAX_CHUNKS 256           // select partials per replica: the centres go to at most this many workgroups per replica
static bool bank_bound(const Stepper& S) { return S.bank_img && S.bank_on_device; }
static const char* opt_env(const char* name) { return name ? getenv(name) : nullptr; }

// carve (or, with base == nullptr, size) the workspace
static size_t carve(Stepper& S, char* base) {
  size_t off = 0;
  auto take_f = [&](size_t nfloats) -> float* {
    float* p = base ? reinterpret_cast<float*>(base + off) : nullptr;
    off += a64(nfloats) * sizeof(float);
    return p;
  };
  auto take_b = [&](size_t nbytes) -> char* {
    char* p = base ? base + off : nullptr;
    off += a64((nbytes + 3) / 4) * sizeof(float);
    return p;
  };
  const size_t B = (size_t)S.B;
  auto pass = [&](Pass& P, bool with_grad) {
    P.acts = take_f(S.act_floats);
    P.ws = take_b(S.ws_bytes);
    P.verts = take_f(B * NV * 3);
    P.joints = take_f(B * NJ * 3);
    P.saved = take_f(S.lbs_saved);
    P.pred17 = take_f(B * 51);
    if (with_grad) {
      P.losses = take_f(4);
      P.drot_l = take_f(B * 216);
      P.dshape_l = take_f(B * 10);
      P.dcam_l = take_f(B * 3);
      P.djoints_l = take_f(B * NJ * 3);
      P.lws = take_f(B * 4);
      P.djoints = take_f(B * NJ * 3);
      P.drot_s = take_f(B * 216);
      P.dbetas_s = take_f(B * 10);
      P.lbs_ws = take_b(S.lbs_wsb);
      P.d_rot = take_f(B * 216);
      P.d_state = take_f(B * STATE_LD);
    }
  };
  pass(S.main, true);
  pass(S.fin, false);
  S.theta_fast = take_f(S.n_params);
  S.theta_fast2 = S.fuse_fast ? take_f(S.n_params) : nullptr;
  S.adam_sc = take_f(64);
  S.grads = take_f(S.n_params);
  S.gt_rot = take_f(B * 24 * 9);
  for (int i = 0; i < 3; ++i) S.gt_verts[i] = take_f(B * NV * 3);
  S.gt_joints = take_f(B * NJ * 3);
  S.gt_saved = take_f(S.lbs_saved);
  S.gt17[0] = take_f(B * 51);
  S.gt17[1] = take_f(B * 51);
  if (S.full) {
    S.lvl0 = S.main;                           // level 0 keeps its own activation arena: its features gate the dynamic loop
    S.lvl0.acts = take_f(S.act_floats);
    pass(S.ex, true);
    pass(S.hist, true);
    pass(S.teach, false);
    S.grads2 = take_f(S.n_params);
    S.grads3 = take_f(S.n_params);
    S.zeros = take_f(B * 216);
    S.ex_rot = take_f(B * 216);
    S.ext_rot = take_f(B * 216); S.ext_shape = take_f(B * 10); S.ext_cam = take_f(B * 3); S.ext_joints = take_f(B * NJ * 3);
    S.exg_rot = take_f(B * 216); S.exg_shape = take_f(B * 10); S.exg_cam = take_f(B * 3); S.exg_joints = take_f(B * NJ * 3);
    S.hg_cam = take_f(B * 3); S.hg_joints = take_f(B * NJ * 3);
    S.vals_t = take_f(8); S.vals_m = take_f(8); S.vals_l = take_f(8);
  }
  if (S.nrep > 1) {
    S.in_stage[0] = take_f(B * 3 * (size_t)S.H * S.W);
    S.in_stage[1] = take_f(B * NJ * 3);
    S.in_stage[2] = take_f(B * 72);
    S.in_stage[3] = take_f(B * 10);
    S.in_stage[4] = take_f(B * 2);
    if (!S.full) {                               // "group_side": the copy the side stream still reads while the next call stages (see adapt)
      S.in_stage_alt[0] = take_f(B * 3 * (size_t)S.H * S.W);
      S.in_stage_alt[1] = take_f(B * NJ * 3);
      S.in_stage_alt[2] = take_f(B * 72);
      S.in_stage_alt[3] = take_f(B * 10);
      S.in_stage_alt[4] = take_f(B * 2);
    }
    if (S.full) {                                // history frame (image, kp2d) and the labelled exemplars (img, kp, pose, betas, pose_3d)
      S.in_stage[5] = take_f(B * 3 * (size_t)S.H * S.W);
      S.in_stage[6] = take_f(B * NJ * 3);
      S.in_stage[7] = take_f(B * 3 * (size_t)S.H * S.W);
      S.in_stage[8] = take_f(B * NJ * 3);
      S.in_stage[9] = take_f(B * 72);
      S.in_stage[10] = take_f(B * 10);
      S.in_stage[11] = take_f(B * 24 * 4);
    }
  } else if (S.full && S.bank_img) {             // one sequence: only the exemplar bank's gather writes staged inputs
    S.in_stage[7] = take_f(B * 3 * (size_t)S.H * S.W);
    S.in_stage[8] = take_f(B * NJ * 3);
    S.in_stage[9] = take_f(B * 72);
    S.in_stage[10] = take_f(B * 10);
    S.in_stage[11] = take_f(B * 24 * 4);
  }
  // (the bank's pointers are set before the workspace is sized; without a bank the layout is what it was)
  S.retr_ws = (S.full && S.bank_img) ? take_b(dyb_retrieve_workspace_bytes(S.nrep, BANK_MAX_CHUNKS, 1)) : nullptr;
  return off;
}

extern "C" int dyb_stepper_create(void* plan, int B, int H, int W, void** out) {
  DYB_REQUIRE(plan && out && B > 0 && B <= 64, DYB_ERR_ARG);
  Stepper* S = new Stepper();
  S->plan = plan; S->B = B; S->H = H; S->W = W;
  S->n_params = dyb_hmr_param_floats(plan);
  S->act_floats = dyb_hmr_act_floats(plan);
  S->ws_bytes = dyb_hmr_workspace_bytes(plan);
  S->off_rot = (size_t)dyb_hmr_act_offset_rotmat(plan);
  S->off_state = (size_t)dyb_hmr_act_offset_state(plan);
  S->lbs_saved = dyb_lbs_saved_floats(B);
  S->lbs_wsb = dyb_lbs_bwd_workspace_bytes(B);
  S->ev = dyb_hmr_events_create(plan);
  dyb_hmr_param_groups(plan, S->grp_bounds);
  // (A/B runs; a set_i of the same option afterwards wins)
#define DYB_OPT_ENV_(member, name, env, type, locked, doc) \
  if (const char* e = opt_env(env)) S->member = atoi(e);
  DYB_STEPPER_OPTIONS_I(DYB_OPT_ENV_)
#undef DYB_OPT_ENV_
  if (!S->ev || hipEventCreateWithFlags(&S->e_theta, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&S->e_side, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&S->e_gt, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&S->e_stage, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&S->e_upd, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&S->gates.ev[0], hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&S->gates.ev[1], hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&S->gates.mid, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&S->ev->l4, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&S->ev->reg, hipEventDisableTiming) != hipSuccess) {
    delete S;
    return DYB_ERR_LAUNCH;
  }
  *out = S;
  return DYB_OK;
}
extern "C" void dyb_stepper_destroy(void* stepper) {
  Stepper* S = reinterpret_cast<Stepper*>(stepper);
  if (!S) return;
  dyb_hmr_events_destroy(S->ev);
  if (S->e_theta) (void)hipEventDestroy(S->e_theta);
  if (S->e_side) (void)hipEventDestroy(S->e_side);
  if (S->e_gt) (void)hipEventDestroy(S->e_gt);
  if (S->e_stage) (void)hipEventDestroy(S->e_stage);
  if (S->e_upd) (void)hipEventDestroy(S->e_upd);
  if (S->gates.ev[0]) (void)hipEventDestroy(S->gates.ev[0]);
  if (S->gates.ev[1]) (void)hipEventDestroy(S->gates.ev[1]);
  if (S->gates.mid) (void)hipEventDestroy(S->gates.mid);
  for (int i = 0; i < 9; ++i) if (S->par_ev[i]) (void)hipEventDestroy(S->par_ev[i]);
  for (int i = 0; i < 2; ++i) if (S->par_stream[i]) (void)hipStreamDestroy(S->par_stream[i]);
  delete S;
}

// ---- string-keyed options: dyb_stepper_options.h is the list (unknown key => DYB_ERR_ARG); below it the keys with code of their own ------
extern "C" int dyb_stepper_set_i(void* stepper, const char* key, long long v) {
  Stepper* S = reinterpret_cast<Stepper*>(stepper);
  DYB_REQUIRE(S && key, DYB_ERR_ARG);
  const std::string k(key);
#define DYB_OPT_SET_I_(member, name, env, type, locked, doc) \
  if (k == name) {                                           \
    DYB_REQUIRE(!(locked) || !S->bound, DYB_ERR_ARG);        \
    S->member = (int)v;                                      \
    return DYB_OK;                                           \
  }
  DYB_STEPPER_OPTIONS_I(DYB_OPT_SET_I_)
#undef DYB_OPT_SET_I_
  if (k == "adam_step") {
    S->adam_t = v;
    for (int r = 0; r < DYB_MAX_REPLICAS; ++r) S->adam_t_rep[r] = v;
  }
  else if (k.compare(0, 10, "adam_step_") == 0) {     // "adam_step_<replica>": replicas may join with different histories
    const int r = atoi(k.c_str() + 10);
    DYB_REQUIRE(r >= 0 && r < DYB_MAX_REPLICAS, DYB_ERR_ARG);
    S->adam_t_rep[r] = v;
    S->adam_t = 0;                                    // "adam_step" reports the largest count among the handle's replicas
    for (int q = 0; q < S->nrep || q <= r; ++q)
      if (S->adam_t_rep[q] > S->adam_t) S->adam_t = S->adam_t_rep[q];
  }
  else if (k == "bank_seed") S->bank_seed = (unsigned long long)v;
  else if (k.compare(0, 10, "bank_draw_") == 0) {     // "bank_draw_<replica>": labelled levels issued so far = the next draw index
    const int r = atoi(k.c_str() + 10);
    DYB_REQUIRE(r >= 0 && r < DYB_MAX_REPLICAS, DYB_ERR_ARG);
    S->bank_draw[r] = (unsigned long long)v;
  }
  else if (k == "drop_seed") S->drop_seed = (unsigned long long)v;
  else if (k == "drop_offset") { S->drop_off = (unsigned long long)v; S->drop_used = 0; }
  else if (k == "replicas") {
    DYB_REQUIRE(v >= 1 && v <= DYB_MAX_REPLICAS && !S->bound, DYB_ERR_ARG);
    S->nrep = (int)v;
  }
  else if (k == "logs_bytes") S->logs_bytes = (size_t)v;
  else return DYB_ERR_ARG;
  return DYB_OK;
}
extern "C" int dyb_stepper_set_f(void* stepper, const char* key, double v) {
  Stepper* S = reinterpret_cast<Stepper*>(stepper);
  DYB_REQUIRE(S && key, DYB_ERR_ARG);
  const std::string k(key);
  if (k == "drop_p") DYB_REQUIRE(v >= 0.0 && v < 1.0, DYB_ERR_ARG);
#define DYB_OPT_SET_F_(member, name, env, type, locked, doc) \
  if (k == name) {                                           \
    S->member = v;                                           \
    return DYB_OK;                                           \
  }
  DYB_STEPPER_OPTIONS_F(DYB_OPT_SET_F_)
#undef DYB_OPT_SET_F_
  return DYB_ERR_ARG;
}
// "smpl_<neutral|male|female>_<0..6>" = the seven float tables of dyb_lbs_fwd, "smpli_<...>_<0..2>" the three int tables
extern "C" int dyb_stepper_set_p(void* stepper, const char* key, const void* p) {
  Stepper* S = reinterpret_cast<Stepper*>(stepper);
  DYB_REQUIRE(S && key, DYB_ERR_ARG);
  const std::string k(key);
#define DYB_OPT_SET_P_(member, name, env, type, locked, doc) \
  if (k == name) {                                           \
    S->member = (decltype(S->member))p;                      \
    return DYB_OK;                                           \
  }
  DYB_STEPPER_OPTIONS_P(DYB_OPT_SET_P_)
#undef DYB_OPT_SET_P_
  static const char* const which[3] = {"neutral", "male", "female"};
  for (int g = 0; g < 3; ++g) {
    const std::string pf = std::string("smpl_") + which[g] + "_", pi = std::string("smpli_") + which[g] + "_";
    if (k.compare(0, pf.size(), pf) == 0 && k.size() == pf.size() + 1 && k.back() >= '0' && k.back() <= '6') {
      S->smpl_f[g][k.back() - '0'] = (const float*)p;
      return DYB_OK;
    }
    if (k.compare(0, pi.size(), pi) == 0 && k.size() == pi.size() + 1 && k.back() >= '0' && k.back() <= '2') {
      S->smpl_i[g][k.back() - '0'] = (const int*)p;
      return DYB_OK;
    }
  }
  return DYB_ERR_ARG;
}
// every int option of the list by its key, and the derived values below
extern "C" long long dyb_stepper_get_i(const void* stepper, const char* key) {
  const Stepper* S = reinterpret_cast<const Stepper*>(stepper);
  if (!S || !key) return -1;
  const std::string k(key);
#define DYB_OPT_GET_(member, name, env, type, locked, doc) \
  if (k == name) return S->member;
  DYB_STEPPER_OPTIONS_I(DYB_OPT_GET_)
  if (k == "adam_step") return S->adam_t;
  if (k.compare(0, 10, "adam_step_") == 0) {          // "adam_step_<replica>"
    const int r = atoi(k.c_str() + 10);
    return (r >= 0 && r < S->nrep) ? S->adam_t_rep[r] : -1;
  }
  if (k == "bank_seed") return (long long)S->bank_seed;
  if (k.compare(0, 10, "bank_draw_") == 0) {
    const int r = atoi(k.c_str() + 10);
    return (r >= 0 && r < S->nrep) ? (long long)S->bank_draw[r] : -1;
  }
  if (k == "drop_used") return S->drop_used;
  if (k == "result_floats") return (long long)S->B * RESULT_FLOATS;
  if (k == "record_floats") return (long long)a64((size_t)S->B * 85 + 1);
  if (k == "loss_floats") return (S->full ? 16 : 4) * (long long)(S->inner_step + 1 + (S->full && S->dynamic ? S->optim_steps : 0));
  if (k == "slots_per_frame") return (S->eval_lower ? S->inner_step : 0) + 1 + (S->full && S->dynamic ? S->optim_steps : 0);
  return -1;
}
// every double option of the list by its key; host issue time (ms, accumulated over "host_frames" frame steps) by section:
// "host_ms_forward", "host_ms_backward", "host_ms_head", "host_ms_update", "host_ms_tail", "host_ms_total"; "deferred_launches"
extern "C" double dyb_stepper_get_f(const void* stepper, const char* key) {
  const Stepper* S = reinterpret_cast<const Stepper*>(stepper);
  if (!S || !key) return -1.0;
  const std::string k(key);
  DYB_STEPPER_OPTIONS_F(DYB_OPT_GET_)
#undef DYB_OPT_GET_
  if (k == "host_ms_forward") return S->h_fwd;
  if (k == "host_ms_backward") return S->h_bwd;
  if (k == "host_ms_head") return S->h_head;
  if (k == "host_ms_update") return S->h_update;
  if (k == "host_ms_tail") return S->h_tail;
  if (k == "host_ms_total") return S->h_total;
  if (k == "host_frames") return (double)S->h_frames;
  if (k == "deferred_launches") return (double)S->n_deferred;     // "wgrad_defer": launches issued behind a backward's join
  return -1.0;
}
extern "C" size_t dyb_stepper_workspace_bytes(void* stepper) {
  Stepper* S = reinterpret_cast<Stepper*>(stepper);
  if (!S) return 0;
  Stepper tmp = *S;
  return a64(carve(tmp, nullptr) / 4) * 4 * (size_t)S->nrep;
}
// `ws` must stay valid (and untouched by others) while the stepper lives; its gradient staging is zeroed here, on `stream`.
extern "C" int dyb_stepper_bind_workspace(void* stepper, void* ws, size_t bytes, hipStream_t st) {
  Stepper* S = reinterpret_cast<Stepper*>(stepper);
  DYB_REQUIRE(S && ws, DYB_ERR_ARG);
  S->blob = a64(carve(*S, nullptr) / 4) * 4;
  DYB_REQUIRE(bytes >= S->blob * (size_t)S->nrep, DYB_ERR_WORKSPACE);
  S->wsp = reinterpret_cast<char*>(ws);
  carve(*S, S->wsp);                 // replica 0's pointers; replica r's = + r * blob (resolved inside the kernels)
  // the engine overwrites every tensor span of the gradient arena and only columns 144..156 of d_state: pads stay zero
  for (int r = 0; r < S->nrep; ++r) {
    HIPOK(hipMemsetAsync(reinterpret_cast<char*>(S->grads) + (size_t)r * S->blob, 0, S->n_params * sizeof(float), st));
    HIPOK(hipMemsetAsync(reinterpret_cast<char*>(S->main.d_state) + (size_t)r * S->blob, 0, (size_t)S->B * STATE_LD * sizeof(float), st));
  }
  if (S->full) {
    for (int r = 0; r < S->nrep; ++r) {
      auto at = [&](float* p0) { return reinterpret_cast<char*>(p0) + (size_t)r * S->blob; };
      HIPOK(hipMemsetAsync(at(S->zeros), 0, (size_t)S->B * 216 * sizeof(float), st));
      HIPOK(hipMemsetAsync(at(S->grads2), 0, S->n_params * sizeof(float), st));
      HIPOK(hipMemsetAsync(at(S->grads3), 0, S->n_params * sizeof(float), st));
      HIPOK(hipMemsetAsync(at(S->ex.d_state), 0, (size_t)S->B * STATE_LD * sizeof(float), st));
      HIPOK(hipMemsetAsync(at(S->hist.d_state), 0, (size_t)S->B * STATE_LD * sizeof(float), st));
    }
    for (int f = 0; f < 15; ++f) {
      long long off = 0;
      int dims[4] = {0, 0, 0, 0}, rs = 0;
      RUN(dyb_hmr_feature_info(S->plan, f, &off, dims, &rs));
      S->fca.off[f] = off;
      if (dims[2] > 0) {                                  // [B][H][W][C] dense
        S->fca.rows[f] = 1; S->fca.cols[f] = dims[0] * dims[1] * dims[2] * dims[3]; S->fca.ld[f] = S->fca.cols[f];
      } else {                                            // [B][cols] with a row stride
        S->fca.rows[f] = dims[0]; S->fca.cols[f] = dims[1]; S->fca.ld[f] = rs;
      }
    }
  }
  S->bound = true;
  return DYB_OK;
}

static int check_ready(const Stepper& S) {
  DYB_REQUIRE(S.bound && S.theta && S.adam_m && S.adam_v && S.init_state && S.gmm_means && S.gmm_prec && S.gmm_logw, DYB_ERR_ARG);
  for (int i = 0; i < 7; ++i) DYB_REQUIRE(S.smpl_f[0][i], DYB_ERR_ARG);
  for (int i = 0; i < 3; ++i) DYB_REQUIRE(S.smpl_i[0][i], DYB_ERR_ARG);
  if (S.metrics) {
    DYB_REQUIRE(S.j_h36m && S.j14 && S.records, DYB_ERR_ARG);
    for (int g = 1; g < 3; ++g) {
      for (int i = 0; i < 7; ++i) DYB_REQUIRE(S.smpl_f[g][i], DYB_ERR_ARG);
      for (int i = 0; i < 3; ++i) DYB_REQUIRE(S.smpl_i[g][i], DYB_ERR_ARG);
    }
  }
  DYB_REQUIRE(S.inner_step >= 0 && S.inner_step <= 16 && S.n_iter >= 1 && S.n_iter <= 3, DYB_ERR_UNSUPPORTED);
  DYB_REQUIRE(!S.results || S.result_capacity > 0, DYB_ERR_ARG);
  DYB_REQUIRE(S.kp_set == 0 || S.kp_set == 1, DYB_ERR_ARG);       // (the setter stores any value: refused here, before the first launch)
  if (bank_bound(S)) {
    // a bank and a retrieval callback are two answers to one question: refused rather than ranked
    DYB_REQUIRE(!S.retrieve && !S.retrieve_rep, DYB_ERR_ARG);
    DYB_REQUIRE(S.full && S.B == 1, DYB_ERR_UNSUPPORTED);         // feature-driven retrieval is batch 1
    DYB_REQUIRE(S.bank_kp && S.bank_pose && S.bank_betas && S.bank_pose3d && S.bank_centers && S.bank_inv_norm && S.bank_member_ptr &&
                S.bank_member_idx && S.bank_picks, DYB_ERR_ARG);
    DYB_REQUIRE(S.bank_items > 0 && S.bank_clusters > 0 && S.bank_members > 0 && S.bank_pick_capacity > 0, DYB_ERR_ARG);
    DYB_REQUIRE(S.retr_ws && S.in_stage[7], DYB_ERR_WORKSPACE);          // "bank_img" was set after the workspace had been sized
  }
  return DYB_OK;
}

static int settle_update(Stepper& S, hipStream_t st);
// HMR forward at `theta` -> rotmat / shape / cam in the pass's arena -> SMPL (neutral) vertices + 49 joints
static int pass_forward(Stepper& S, Pass& P, const float* theta, const float* image, hipStream_t st, bool chain = true) {
  // (a ranged weight update may still be running on the auxiliary stream: this forward - the first reader of the new weights -
  // waits for each range where it first reads it).  chain = false: a forward on the side stream or a pass stream
  // that must leave the chain's gate state alone (a group's final inference on the side stream IS its update's consuming forward:
  // frame_step calls it with chain = true)
  const DybFwdGates* gates = (chain && S.gates_pending) ? &S.gates : nullptr;
  {
    const int rc = dyb_hmr_forward_plain(S.plan, theta, image, S.init_state, S.n_iter, P.acts, P.ws, S.ws_bytes, st, gates);
    if (rc != DYB_OK) {
      // the forward may have stopped before it waited for / issued the later ranges: make the stream wait for the whole update so
      // that nothing stale is read by whatever the caller does next, then report the failure
      if (gates) (void)settle_update(S, st);
      return rc;
    }
    // consumed: every range's gate was waited for inside the forward (the deferred one issued there)
    if (gates) { DYB_REQUIRE(!S.gates.late, DYB_ERR_LAUNCH); S.gates_pending = false; S.defer_pending = false; }
  }
  const float* rot = P.acts + S.off_rot;
  const float* state = P.acts + S.off_state;
  return dyb_lbs_fwd(S.smpl_f[0], S.smpl_i[0], state + 144, STATE_LD, rot, P.verts, P.joints, P.saved, S.B, st);
}
// frame-loss head (reference base_adaptor.py:229-240 / :279-289): value + gradient in one launch
static int pass_frame_head(Stepper& S, Pass& P, const float* kp2d, hipStream_t st) {
  const float* rot = P.acts + S.off_rot;
  const float* state = P.acts + S.off_state;
  return dyb_frame_losses_kp(rot, state + 144, STATE_LD, state + 154, STATE_LD, P.joints, kp2d, S.gmm_means, S.gmm_prec, S.gmm_logw,
                             (float)S.w2d, (float)S.wshape, (float)S.wpose, P.losses, P.drot_l, P.dshape_l, 10, P.dcam_l, 3, P.djoints_l,
                             S.B, S.kp_set, P.lws, (size_t)S.B * 16, st);
}
// where a weight update goes by arena ranges (weight_update) - and a chain backward may defer weight gradients ("wgrad_defer")
static bool ranged_form(const Stepper& S, hipStream_t st, hipStream_t aux) {
  return S.upd_overlap && S.nrep > 1 && aux && aux != st && S.grp_bounds[0] > 0 && S.grp_bounds[1] > S.grp_bounds[0] &&
         S.grp_bounds[1] < S.n_params;
}
// the engine's backward on the stepper's event set; with "wgrad_defer" in the ranged form it leaves the deferred set in flight on `aux`
// (never captured: dyb_hmr_backward_ev has no graph cache)
static int engine_backward(Stepper& S, Pass& P, const float* theta, float* grads, hipStream_t st, hipStream_t aux) {
  const bool defer = S.wgrad_defer && ranged_form(S, st, aux) && S.ev->l4 && S.ev->reg;
  if (defer) S.defer_pending = true;           // (also when the call fails half-way: settle_update then waits for what was issued)
  return dyb_hmr_backward_ev(S.plan, theta, P.acts, P.d_rot, P.d_state, S.n_iter, grads, P.ws, S.ws_bytes, st, aux, S.ev, defer, &S.n_deferred);
}
// ground-truth side of the metrics (depends on the batch only): male / female / neutral meshes from the axis-angle pose
static int gt_meshes(Stepper& S, const float* gt_pose, const float* gt_betas, hipStream_t st) {
  RUN(dyb_rodrigues_fwd(gt_pose, S.gt_rot, S.B * 24, st));
  for (int g = 0; g < 3; ++g)
    RUN(dyb_lbs_fwd(S.smpl_f[g], S.smpl_i[g], gt_betas, 10, S.gt_rot, S.gt_verts[g], S.gt_joints, S.gt_saved, S.B, st));
  RUN(dyb_regress_joints(S.j_h36m, S.gt_verts[1], S.gt17[0], 17, S.B, st));
  return dyb_regress_joints(S.j_h36m, S.gt_verts[2], S.gt17[1], 17, S.B, st);
}
static int record_metrics(Stepper& S, Pass& P, const long long* gender, int slot, hipStream_t st) {
  DYB_REQUIRE(slot >= 0 && slot < S.record_capacity, DYB_ERR_ARG);
  RUN(dyb_regress_joints(S.j_h36m, P.verts, P.pred17, 17, S.B, st));
  float* rec = S.records + (size_t)slot * a64((size_t)S.B * 85 + 1);
  const DybRep& Rp = dyb_rep_current();
  hipLaunchKernelGGL(metric_record_kernel, dim3(1, 1, Rp.n), dim3(256), 0, st, P.pred17, S.gt17[0], S.gt17[1], gender, S.j14, P.verts,
                     S.gt_verts[0], rec, S.B, Rp);
  DYB_CHECK_LAUNCH();
  return DYB_OK;
}

// the final inference in pass P -> row `loss_slot mod result_capacity` of the result ring, for every replica of the current scope
static int pack_result(Stepper& S, Pass& P, int loss_slot, hipStream_t st) {
  if (!S.results || loss_slot < 0) return DYB_OK;
  float* row = S.results + (size_t)(loss_slot % S.result_capacity) * S.B * RESULT_FLOATS;
  return dyb_result_pack(P.acts + S.off_rot, P.acts + S.off_state, P.verts, row, S.B, st);
}

// issue what the side stream owes: the previous frame's final forward + record (one sequence), then this frame's ground-truth meshes
static int issue_side_work(Stepper& S, hipStream_t side) {
  if (S.tail.on) {
    HIPOK(hipStreamWaitEvent(side, S.e_theta, 0));
    RUN(pass_forward(S, S.fin, S.theta, S.tail.image, side, false));
    if (S.tail.metrics) RUN(record_metrics(S, S.fin, S.tail.gender, S.tail.slot, side));
    RUN(pack_result(S, S.fin, S.tail.loss_slot, side));
    HIPOK(hipEventRecord(S.e_side, side));
    S.side_pending = true;
    S.tail.on = false;
  }
  if (S.gtjob.on) {
    if (S.gtjob.staged) HIPOK(hipStreamWaitEvent(side, S.e_stage, 0));
    RUN(gt_meshes(S, S.gtjob.pose, S.gtjob.betas, side));
    HIPOK(hipEventRecord(S.e_gt, side));
    S.gtjob.on = false;
  }
  return DYB_OK;
}
// ---- weight updates ---------------------------------------------------------------------------------------------------
static bool spans_touch(const Stepper& S, size_t lo, size_t hi) {
  for (const DybSpan& sp : S.upd_spans)
    if (sp.off < hi && sp.off + sp.n > lo) return true;
  return false;
}
// [lo, hi) minus the spans the level's weight gradients updated themselves (S.upd_spans, sorted): the gaps between them as float4
// segments, handed to `emit` in batches of up to DYB_FW_MAX_SEGS
template <class Emit>
static int walk_gaps(const Stepper& S, size_t lo, size_t hi, Emit emit) {
  DYB_REQUIRE(lo % 4 == 0 && hi % 4 == 0, DYB_ERR_UNSUPPORTED);
  DybFwSegs t{};
  auto flush = [&]() -> int {
    if (t.n == 0) return DYB_OK;
    const int rc = emit(t);
    t.n = 0;
    return rc;
  };
  auto add = [&](size_t a, size_t b) -> int {
    if (a >= b) return DYB_OK;
    DYB_REQUIRE(a % 4 == 0 && b % 4 == 0 && (b - a) / 4 < 0xffffffffull && a / 4 < 0xffffffffull, DYB_ERR_UNSUPPORTED);
    if (t.n == DYB_FW_MAX_SEGS) RUN(flush());
    t.start4[t.n] = (unsigned)(a / 4); t.count4[t.n] = (unsigned)((b - a) / 4); ++t.n;
    return DYB_OK;
  };
  size_t at = lo;
  for (const DybSpan& sp : S.upd_spans) {
    if (sp.off + sp.n <= at) continue;
    if (sp.off >= hi) break;
    DYB_REQUIRE(sp.off >= lo && sp.off + sp.n <= hi, DYB_ERR_UNSUPPORTED);     // a tensor never straddles a range boundary
    RUN(add(at, sp.off));
    at = sp.off + sp.n;
  }
  RUN(add(at, hi));
  return flush();
}
// out[lo, hi) = p - fastlr * (grads [+ g2 + g3]) minus the fused spans
static int fastweight_range(Stepper& S, const float* p, float* out, const float* g2, const float* g3, size_t lo, size_t hi, hipStream_t s) {
  if (!spans_touch(S, lo, hi))
    return dyb_fastweight_update3(p + lo, S.grads + lo, g2 ? g2 + lo : nullptr, g3 ? g3 + lo : nullptr, out + lo, (float)S.fastlr, hi - lo, s);
  DYB_REQUIRE(!g2 && !g3, DYB_ERR_UNSUPPORTED);     // (the fused form exists for single-pass levels only)
  return walk_gaps(S, lo, hi, [&](const DybFwSegs& t) { return dyb_fastweight_update_segs(p, S.grads, out, (float)S.fastlr, t, s); });
}
// Adam over [lo, hi) minus the fused spans (ema: the teacher's EMA of the range in the same pass - "fuse_ema", default term set)
static int adam_range(Stepper& S, const float* g2, const float* g3, const float* ss, const float* bc, size_t lo, size_t hi, hipStream_t s,
                      bool ema) {
  if (!spans_touch(S, lo, hi))
    return dyb_adam_step_rep3_ema(S.theta + lo, S.grads + lo, g2 ? g2 + lo : nullptr, g3 ? g3 + lo : nullptr, S.adam_m + lo, S.adam_v + lo,
                                  (float)S.beta1, (float)S.beta2, ss, bc, (float)S.eps, hi - lo, ema ? S.teacher + lo : nullptr, (float)S.alpha, s);
  DYB_REQUIRE(!ema && !g2 && !g3, DYB_ERR_UNSUPPORTED);
  return walk_gaps(S, lo, hi, [&](const DybFwSegs& t) {
    return dyb_adam_step_segs(S.theta, S.grads, S.adam_m, S.adam_v, (float)S.beta1, (float)S.beta2, ss, bc, (float)S.eps, t, s);
  });
}
// this step's Adam bias corrections of every replica of the current scope, by physical replica (each has its own step count, which
// advances HERE; adam_t keeps the largest)
static void adam_corrections(Stepper& S, float* ss, float* bc) {
  const DybRep& R = dyb_rep_current();
  for (int r = 0; r < DYB_MAX_REPLICAS; ++r) { ss[r] = 0.f; bc[r] = 1.f; }
  for (int i = 0; i < R.n; ++i) {
    const int r = dyb_rep_phys(R, i);
    const double t = (double)(++S.adam_t_rep[r]);
    ss[r] = (float)(S.lr / (1.0 - pow(S.beta1, t)));
    bc[r] = (float)sqrt(1.0 - pow(S.beta2, t));
    if (S.adam_t_rep[r] > S.adam_t) S.adam_t = S.adam_t_rep[r];
  }
}
// the corrections fixed BEFORE the outer backward: kept for weight_update(adam) and written into each replica's adam_sc on `st` for the
// weight-gradient epilogues that apply Adam themselves ("fuse_adam")
static int adam_prepare(Stepper& S, hipStream_t st) {
  adam_corrections(S, S.pre_ss, S.pre_bc);
  S.adam_prepared = true;
  return dyb_adam_write_scalars(S.adam_sc, S.pre_ss, S.pre_bc, st);
}
// one arena range of the weight update U on stream `s`
static int update_range(Stepper& S, const Stepper::Upd& U, size_t lo, size_t hi, hipStream_t s) {
  if (!U.adam) return fastweight_range(S, U.p, U.out, U.g2, U.g3, lo, hi, s);
  // update_teacher (base_adaptor.py:193-201) of the same range: inside the Adam pass ("fuse_ema"), or right behind it
  const bool fe = U.ema && S.fuse_ema;
  RUN(adam_range(S, U.g2, U.g3, U.ss, U.bc, lo, hi, s, fe));
  if (U.ema && !fe) RUN(dyb_ema_update(S.teacher + lo, S.theta + lo, (float)S.alpha, hi - lo, s));
  return DYB_OK;
}
// the deferred last range of a ranged weight update (see weight_update): issued from inside the consuming forward at layer3
static int late_update(void* user) {
  Stepper& S = *reinterpret_cast<Stepper*>(user);
  Stepper::LateUpd& L = S.late;
  DybRepScope scope(L.scope);
  HIPOK(hipStreamWaitEvent(L.aux, S.gates.mid, 0));
  RUN(update_range(S, L.u, S.grp_bounds[1], S.n_params, L.aux));
  HIPOK(hipEventRecord(S.gates.ev[1], L.aux));
  S.gates.late = nullptr;
  return DYB_OK;
}
// One weight update over the whole arena - the fast-weight step out = p - fastlr * grads (adam = false) or Adam in place on theta, each
// replica of the launch scope with its own bias corrections -
// as one launch on `st`, or (upd_overlap, replica groups with an auxiliary stream) by arena ranges: [0, layer3) on `st`, [layer3,
// layer4) and [layer4, end) on `aux` behind everything `st` has issued, each followed by its gate event; the next pass_forward waits
// for them where it first reads those weights.
static int weight_update(Stepper& S, bool adam, const float* p, float* out, hipStream_t st, hipStream_t aux, bool ema = false) {
  // a ranged update nobody consumed (no chain forward followed it) must not be overtaken: its tail range would stay un-issued and
  // its events would satisfy later waits with stale weights - settle it first
  if (S.gates_pending) RUN(settle_update(S, st));
  DYB_REQUIRE(!S.gates.late, DYB_ERR_LAUNCH);
  Stepper::Upd U;
  U.adam = adam; U.ema = ema; U.p = p; U.out = out;
  U.g2 = S.lvl_g2; U.g3 = S.lvl_g3;                  // further gradient arenas of the level just differentiated (full term set), consumed here
  S.lvl_g2 = S.lvl_g3 = nullptr;
  // the spans this level's weight gradients turned into fast weights themselves ("fuse_fast"): taken over, sorted, for this update only
  S.upd_spans.clear();
  S.upd_spans.swap(S.fused_spans);
  std::sort(S.upd_spans.begin(), S.upd_spans.end(), [](const DybSpan& a, const DybSpan& b) { return a.off < b.off; });
  S.fused_spans.clear();
  if (adam && S.adam_prepared) {                       // fixed before the outer backward (adam_prepare): the epilogues used the same numbers
    for (int r = 0; r < DYB_MAX_REPLICAS; ++r) { U.ss[r] = S.pre_ss[r]; U.bc[r] = S.pre_bc[r]; }
    S.adam_prepared = false;
  } else if (adam) {
    adam_corrections(S, U.ss, U.bc);
  }
  if (!ranged_form(S, st, aux)) {
    if (S.defer_pending) {         // (a switch flipped between the backward and its update) the pass reads / rewrites what the deferred set writes
      HIPOK(hipStreamWaitEvent(st, S.ev->l4, 0));
      HIPOK(hipStreamWaitEvent(st, S.ev->reg, 0));
      S.defer_pending = false;
    }
    return update_range(S, U, 0, S.n_params, st);
  }
  // the consuming forward waits for the level's deferred weight gradients too.  The ranged pass of [layer4, end) below / in late_update
  // writes the spans of that arena range those launches did NOT update themselves (and, without fused epilogues, reads their gradients):
  // it is issued on `aux`, an in-order stream, behind them - keep it there.
  S.gates.l4 = S.defer_pending ? S.ev->l4 : nullptr;
  S.gates.reg = S.defer_pending ? S.ev->reg : nullptr;
  RUN(update_range(S, U, 0, S.grp_bounds[0], st));
  HIPOK(hipEventRecord(S.e_upd, st));                 // the gradients' main-stream writers (and the first range) are behind this point
  HIPOK(hipStreamWaitEvent(aux, S.e_upd, 0));
  RUN(update_range(S, U, S.grp_bounds[0], S.grp_bounds[1], aux));
  HIPOK(hipEventRecord(S.gates.ev[0], aux));
  if (S.upd_late) {
    // the last range waits until the forward that consumes it reaches layer3 (gates.late, called from inside that forward)
    S.late.u = U; S.late.aux = aux; S.late.scope = dyb_rep_current();
    S.gates.late = &late_update;
    S.gates.user = &S;
  } else {
    S.gates.late = nullptr;
    RUN(update_range(S, U, S.grp_bounds[1], S.n_params, aux));
    HIPOK(hipEventRecord(S.gates.ev[1], aux));
  }
  S.gates_pending = true;
  return DYB_OK;
}
// make `st` wait for a ranged update nobody has consumed yet (a consumer other than a forward follows)
static int settle_update(Stepper& S, hipStream_t st) {
  if (S.defer_pending && !S.gates_pending) {         // a backward deferred weight gradients and no update followed it (it failed half-way)
    HIPOK(hipStreamWaitEvent(st, S.ev->l4, 0));
    HIPOK(hipStreamWaitEvent(st, S.ev->reg, 0));
    S.defer_pending = false;
  }
  if (!S.gates_pending) return DYB_OK;
  if (S.gates.late) {                               // nobody's forward will call it: issue the deferred range now
    HIPOK(hipEventRecord(S.gates.mid, st));
    RUN(late_update(&S));
  }
  HIPOK(hipStreamWaitEvent(st, S.gates.ev[0], 0));
  HIPOK(hipStreamWaitEvent(st, S.gates.ev[1], 0));
  if (S.defer_pending) {                            // the deferred weight gradients of the level this update belongs to
    HIPOK(hipStreamWaitEvent(st, S.ev->l4, 0));
    HIPOK(hipStreamWaitEvent(st, S.ev->reg, 0));
    S.defer_pending = false;
  }
  S.gates_pending = false;
  return DYB_OK;
}
// ---- the full loss set -------------------------------------------------------------------------------------------------
// gradient of (frame loss [+ external terms]) or of external terms alone w.r.t. theta through pass P
static int pass_backward_ext(Stepper& S, Pass& P, const float* theta, float* grads, bool frame_loss, const float* e_rot,
                             const float* e_shape, const float* e_cam, const float* e_joints, hipStream_t st, hipStream_t aux) {
  const size_t nj = (size_t)S.B * NJ * 3;
  if (frame_loss) RUN(dyb_scale_add(nullptr, P.djoints_l, e_joints, P.djoints, nj, st));
  else RUN(dyb_scale_add(nullptr, e_joints, nullptr, P.djoints, nj, st));
  RUN(dyb_lbs_bwd(S.smpl_f[0], S.smpl_i[0], P.acts + S.off_rot, P.saved, P.djoints, nullptr, P.drot_s, P.dbetas_s, 10, S.B, P.lbs_ws,
                  S.lbs_wsb, st));
  const float* z = S.zeros;
  RUN(dyb_head_grad_combine(nullptr, frame_loss ? P.drot_l : z, P.drot_s, e_rot, frame_loss ? P.dshape_l : z, P.dbetas_s, e_shape,
                            frame_loss ? P.dcam_l : z, e_cam, P.d_rot, P.d_state, S.B, st));
  return engine_backward(S, P, theta, grads, st, aux);
}
enum { IN_IMAGE = 0, IN_KP, IN_GT_POSE, IN_GT_BETAS, IN_GENDER, IN_HIST_IMAGE, IN_HIST_KP, IN_EX_IMG, IN_EX_KP, IN_EX_POSE,
       IN_EX_BETAS, IN_EX_POSE3D, IN_COUNT };
// copy `nk` inputs (kinds k0 .. k0+nk-1 in IN_* order) of every replica of the current scope from the callers' separate tensors
// into the replicas' staging areas, one launch: src[(kind - k0) * ld + physical replica] (NULL: nothing to copy)
static int stage_inputs(Stepper& S, const void* const* src, int ld, int k0, int nk, hipStream_t st);
// what the levels of one frame step share
struct LevelCtx {
  const void* in[IN_COUNT];   // the frame's inputs: the callers' tensors (one sequence) or the staging areas; NULL = absent
  float* losslog;             // this frame's log rows (NULL: not logged)
  hipStream_t side;           // the side stream this frame step uses (frame-loss set, one sequence), or NULL
  // the main stream waits for the ground-truth meshes only where it first reads them (the record after inner step 0): at the top of
  // the frame the side stream is still busy with the previous frame's final forward, and waiting there stalled the main
  // chain for that whole tail (1.1 ms per frame in the kernel trace)
  bool gt_waited;
};
// A level that forked onto the pass streams and fails before its joins must not return with work still queued there against the
// stepper's arenas: the caller's stream is ordered behind the CURRENT tails of both pass streams on every early return, so a
// retry or a free on that stream cannot race them.  Disarmed once the regular joins (par_ev[3] / par_ev[5]) have been issued.
struct ParTailGuard {
  hipStream_t st, sB, sC;
  hipEvent_t eB, eC;
  bool armed;
  ~ParTailGuard() {
    if (!armed) return;
    if (sB != st && hipEventRecord(eB, sB) == hipSuccess) (void)hipStreamWaitEvent(st, eB, 0);
    if (sC != st && hipEventRecord(eC, sC) == hipSuccess) (void)hipStreamWaitEvent(st, eC, 0);
  }
};
// Exemplar bank: every replica of the current scope picks (nearest centre of its pooled feature in pass P, member draw bank_draw[r]) on
// `sel` - the stream P's forward was issued on - and the chosen exemplars are gathered into the replicas' exemplar staging on `gat`, the
// stream the exemplar pass runs on, behind the event `ev` when the two differ.  The staging's previous readers (the last level's
// exemplar forward / backward) are ordered before the gather: on `gat` itself, or - they ran on another stream - by that level's join
// (par_ev[5]) and this level's fork (par_ev[0]).  C.in[IN_EX_*] become the staging areas; the draw indices advance.
static int bank_retrieve(Stepper& S, LevelCtx& C, Pass& P, hipStream_t sel, hipStream_t gat, hipEvent_t ev) {
  const DybRep& R = dyb_rep_current();
  int rows[DYB_MAX_REPLICAS];
  for (int i = 0; i < R.n; ++i) rows[i] = S.nrep == 1 ? 0 : dyb_rep_phys(R, i);
  const int K = S.bank_clusters, cap = S.bank_pick_capacity;
  const int chunk = std::max(16, dyb_cdiv(K, BANK_MAX_CHUNKS));
  RUN(dyb_retrieve_select(P.acts + S.fca.off[5], S.blob, rows, R.n, S.bank_centers, S.bank_inv_norm, K, S.bank_member_ptr, S.bank_member_idx,
                          S.bank_members, S.bank_items, S.bank_draw, S.bank_seed, 0, S.bank_picks, (size_t)cap * 2 * sizeof(int), cap, chunk, 0,
                          S.retr_ws, dyb_retrieve_workspace_bytes(S.nrep, BANK_MAX_CHUNKS, 1), sel));
  if (gat != sel) {
    HIPOK(hipEventRecord(ev, sel));
    HIPOK(hipStreamWaitEvent(gat, ev, 0));
  }
  float* dst[5];
  size_t stride[5];
  for (int k = 0; k < 5; ++k) {
    DYB_REQUIRE(S.in_stage[IN_EX_IMG + k], DYB_ERR_ARG);
    dst[k] = S.in_stage[IN_EX_IMG + k];
    stride[k] = S.blob;
  }
  RUN(dyb_exemplar_gather(S.bank_picks, (size_t)cap * 2 * sizeof(int), cap, rows, R.n, S.bank_draw, S.bank_img, S.bank_kp, S.bank_pose,
                          S.bank_betas, S.bank_pose3d, S.bank_items, dst, stride, gat));
  for (int k = 0; k < 5; ++k) C.in[IN_EX_IMG + k] = S.in_stage[IN_EX_IMG + k];
  for (int i = 0; i < R.n; ++i) ++S.bank_draw[rows[i]];
  return DYB_OK;
}
// the weight gradients' fused update epilogues ("fuse_fast", "fuse_adam") exist for single-pass levels: never with the full term set
static bool fused_epilogues(const Stepper& S) { return !S.full; }
// One level (reference base_adaptor.py:222-317 lower / upper_level_adaptation) at weights `cur` through pass P: forward, frame head,
// the metric record of the inference this forward stands for (record_slot >= 0), the terms of the full set that are enabled, the log
// row (frame-loss set: the head's 4 floats; full set: 16), and the gradient of the level total w.r.t. `cur` in S.grads (+ S.lvl_g2 /
// lvl_g3, which the weight update that follows sums).  With no term enabled these are the launches of the frame-loss set exactly.
// nxt: where a lower level's fused epilogues write the next fast weights.
// have_fwd: P already holds the forward of (cur, this frame's image) - the dynamic loop hands the previous step's final inference on
static int level(Stepper& S, LevelCtx& C, Pass& P, const float* cur, float* nxt, bool upper, int level_index, int record_slot, hipStream_t st,
                 hipStream_t aux, bool have_fwd = false) {
  const int B = S.B;
  const float* image = (const float*)C.in[IN_IMAGE];
  const float* kp = (const float*)C.in[IN_KP];
  const bool temporal = S.full && (upper ? S.temporal_upper != 0 : S.temporal_lower != 0);
  const bool teacher = temporal && S.use_teacher && S.teacher;
  const bool motion = temporal && S.use_motion && C.in[IN_HIST_IMAGE] && C.in[IN_HIST_KP];
  const bool label = S.full && (upper ? S.mix_upper : S.mix_lower) != 0;
  // One sequence: the history pass and the exemplar pass go to streams of their own.  Dependencies (events par_ev[]): both wait for
  // the weights (0: recorded on the chain where the level starts); the motion term (chain) needs the history forward (1) and leaves
  // the history pass's head gradients (2) for its backward; the chain's log row reads the label term's values (4); the weight update
  // that follows the level reads all three gradient arenas (3, 5).  Their backwards run without an auxiliary stream (weight gradients
  // in line: the engine's per-plan event set serves one two-stream backward at a time - the chain's).  Retrieval by callback
  // synchronises with the level's own forward on the host: sequential as before.
  // For replica groups too (up to par_max_replicas per launch, default: all): default term set, frames/s sequential -> parallel passes at
  // 1: 65 -> 78 (89 with 8 hardware queues), 2: 93 -> 107, 3: 116 -> 129, 4: 131 -> 145, 5: 154 -> 182, 8: 205 -> 232, 16: 290 -> 316,
  // 32: 362 -> 377 (profiles/r05_sessions.txt s29 / s30) - a level's three passes fill each other's ramps and tails.
  const bool par = S.par_passes && dyb_rep_current().n <= S.par_max_replicas && !S.retrieve && !S.retrieve_rep && (motion || label);
  // a ranged weight update may still be in flight (replica groups): the chain's forward waits for each range where it first reads it,
  // the pass streams read every weight - they wait for both range events, which exist once the chain's forward has been issued
  const bool ranged_before = par && S.gates_pending && !have_fwd;
  hipStream_t sB = st, sC = st;
  if (par) {
    for (int i = 0; i < 2; ++i)
      if (!S.par_stream[i]) HIPOK(hipStreamCreateWithFlags(&S.par_stream[i], hipStreamNonBlocking));
    for (int i = 0; i < 9; ++i)
      if (!S.par_ev[i]) HIPOK(hipEventCreateWithFlags(&S.par_ev[i], hipEventDisableTiming));
    sB = S.par_stream[0]; sC = S.par_stream[1];
    HIPOK(hipEventRecord(S.par_ev[0], st));
    if (motion) HIPOK(hipStreamWaitEvent(sB, S.par_ev[0], 0));
    if (label) HIPOK(hipStreamWaitEvent(sC, S.par_ev[0], 0));
  }
  ParTailGuard tails{st, sB, sC, S.par_ev[6], S.par_ev[7], par};
  if (!have_fwd) {
    HostTimer t(S.h_fwd);
    RUN(pass_forward(S, P, cur, image, st));
  }
  {
    HostTimer th(S.h_head);
    RUN(pass_frame_head(S, P, kp, st));
    if (C.losslog && !S.full) {
      hipLaunchKernelGGL(copy4_kernel, dim3(1, 1, dyb_rep_current().n), dim3(64), 0, st, (const float*)P.losses, C.losslog + 4 * level_index,
                         dyb_rep_current());
      DYB_CHECK_LAUNCH();
    }
    // inference() after the previous inner step = this level's forward (same weights, same image: dynaboa_benchmark.py:142); the record
    // only reads the pass's forward products, which nothing later in the level writes
    if (record_slot >= 0) {
      if (!C.gt_waited) {
        HIPOK(hipStreamWaitEvent(st, S.e_gt, 0));
        C.gt_waited = true;
      }
      RUN(record_metrics(S, P, (const long long*)C.in[IN_GENDER], record_slot, st));
    }
  }
  const float* rot = P.acts + S.off_rot;
  const float* state = P.acts + S.off_state;
  if (ranged_before) {
    DYB_REQUIRE(!S.gates_pending && !S.gates.late, DYB_ERR_LAUNCH);            // consumed by the chain's forward above
    for (int k = 0; k < 2; ++k) {
      if (motion) HIPOK(hipStreamWaitEvent(sB, S.gates.ev[k], 0));
      if (label) HIPOK(hipStreamWaitEvent(sC, S.gates.ev[k], 0));
    }
    for (hipEvent_t e : {S.gates.l4, S.gates.reg}) {     // ... and for the deferred weight gradients that wrote layer4 / the regressor
      if (e && motion) HIPOK(hipStreamWaitEvent(sB, e, 0));
      if (e && label) HIPOK(hipStreamWaitEvent(sC, e, 0));
    }
  }
  if (par && motion) {
    RUN(pass_forward(S, S.hist, cur, (const float*)C.in[IN_HIST_IMAGE], sB, false));
    HIPOK(hipEventRecord(S.par_ev[1], sB));
  }
  auto label_pass_forward_and_term = [&](hipStream_t s, bool chain) -> int {
    RUN(pass_forward(S, S.ex, cur, (const float*)C.in[IN_EX_IMG], s, chain));
    RUN(dyb_rodrigues_fwd((const float*)C.in[IN_EX_POSE], S.ex_rot, B * 24, s));          // utils/geometry.py:9-24 on the exemplar pose
    const float* es = S.ex.acts + S.off_state;
    return dyb_aux_loss_terms_kp(2, B, 0, (float)S.label_w, S.ex.acts + S.off_rot, es + 144, STATE_LD, es + 154, STATE_LD, S.ex.joints, nullptr,
                                 nullptr, 0, nullptr, 0, nullptr, (const float*)C.in[IN_EX_KP], nullptr, S.ex_rot,
                                 (const float*)C.in[IN_EX_BETAS], (const float*)C.in[IN_EX_POSE3D], S.vals_l, S.exg_rot, S.exg_shape, S.exg_cam,
                                 S.exg_joints, nullptr, nullptr, 0, s);
  };
  if (par && label) {
    // exemplar bank: select on the chain right behind the level's forward, gather + labelled pass on the exemplar stream behind it
    if (bank_bound(S)) RUN(bank_retrieve(S, C, P, st, sC, S.par_ev[8]));
    DYB_REQUIRE(C.in[IN_EX_IMG] && C.in[IN_EX_KP] && C.in[IN_EX_POSE] && C.in[IN_EX_BETAS] && C.in[IN_EX_POSE3D], DYB_ERR_ARG);
    RUN(label_pass_forward_and_term(sC, false));
    HIPOK(hipEventRecord(S.par_ev[4], sC));
    RUN(pass_backward_ext(S, S.ex, cur, S.grads3, false, S.exg_rot, S.exg_shape, S.exg_cam, S.exg_joints, sC, nullptr));
    HIPOK(hipEventRecord(S.par_ev[5], sC));
  }
  bool ext = false;
  if (teacher) {
    // teacher forward (no gradient): reference base_adaptor.py:324-329
    if (S.teacher_train) {
      // (by now the chain's own forward has consumed the gates of a ranged update: the teacher's ranges are complete on `st`)
      DYB_REQUIRE(!S.gates_pending, DYB_ERR_LAUNCH);
      RUN(dyb_hmr_forward_train(S.plan, S.teacher, image, S.init_state, S.n_iter, S.teach.acts, S.teach.ws, S.ws_bytes, S.drop_seed,
                                S.drop_off + (unsigned long long)S.drop_used, (float)S.drop_p, st));
      ++S.drop_used;
      const float* tstate = S.teach.acts + S.off_state;
      RUN(dyb_lbs_fwd(S.smpl_f[0], S.smpl_i[0], tstate + 144, STATE_LD, S.teach.acts + S.off_rot, S.teach.verts, S.teach.joints,
                      S.teach.saved, S.B, st));
    } else {
      RUN(pass_forward(S, S.teach, S.teacher, image, st));
    }
    const float* ts = S.teach.acts + S.off_state;
    RUN(dyb_aux_loss_terms_kp(0, B, 0, (float)S.teacher_w, rot, state + 144, STATE_LD, state + 154, STATE_LD, P.joints,
                              S.teach.acts + S.off_rot, ts + 144, STATE_LD, ts + 154, STATE_LD, S.teach.joints, nullptr, nullptr, nullptr,
                              nullptr, nullptr, S.vals_t, S.ext_rot, S.ext_shape, S.ext_cam, S.ext_joints, nullptr, nullptr, 0, st));
    ext = true;
  }
  if (motion) {
    // the history frame through the SAME weights, with gradient (base_adaptor.py:380-386)
    if (par) HIPOK(hipStreamWaitEvent(st, S.par_ev[1], 0));
    else RUN(pass_forward(S, S.hist, cur, (const float*)C.in[IN_HIST_IMAGE], st));
    const float* hs = S.hist.acts + S.off_state;
    RUN(dyb_aux_loss_terms_kp(1, B, ext ? 1 : 0, (float)S.motion_w, rot, state + 144, STATE_LD, state + 154, STATE_LD, P.joints, nullptr,
                              nullptr, 0, hs + 154, STATE_LD, S.hist.joints, kp, (const float*)C.in[IN_HIST_KP], nullptr, nullptr, nullptr,
                              S.vals_m, S.ext_rot, S.ext_shape, S.ext_cam, S.ext_joints, S.hg_cam, S.hg_joints, S.kp_set, st));
    ext = true;
    if (par) {
      HIPOK(hipEventRecord(S.par_ev[2], st));
      HIPOK(hipStreamWaitEvent(sB, S.par_ev[2], 0));
      RUN(pass_backward_ext(S, S.hist, cur, S.grads2, false, nullptr, nullptr, S.hg_cam, S.hg_joints, sB, nullptr));
      HIPOK(hipEventRecord(S.par_ev[3], sB));
    }
  }
  if (label && !par) {
    // retrieval (base_adaptor.py:82-96): the exemplar bank's two kernels in line, or on the host - hand it the pooled feature of this
    // level's forward
    if (bank_bound(S)) {
      RUN(bank_retrieve(S, C, P, st, st, nullptr));
    } else if (S.nrep > 1 && S.retrieve_rep) {
      DYB_REQUIRE(S.feat5_out, DYB_ERR_ARG);
      const DybRep& R = dyb_rep_current();
      RUN(dyb_scale_add(nullptr, P.acts + S.fca.off[5], nullptr, S.feat5_out, (size_t)B * 2048, st));     // every replica's feature, one launch
      const void* exin[5 * DYB_MAX_REPLICAS];
      for (int k = 0; k < 5 * DYB_MAX_REPLICAS; ++k) exin[k] = nullptr;
      for (int i = 0; i < R.n; ++i) {
        const int r = dyb_rep_phys(R, i);
        const void* one[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
        if (S.retrieve_rep(S.retrieve_user, level_index, r, one) != 0) return DYB_ERR_ARG;
        for (int k = 0; k < 5; ++k) {
          DYB_REQUIRE(one[k], DYB_ERR_ARG);
          exin[k * DYB_MAX_REPLICAS + r] = one[k];
        }
      }
      RUN(stage_inputs(S, exin, DYB_MAX_REPLICAS, IN_EX_IMG, 5, st));
      for (int k = 0; k < 5; ++k) C.in[IN_EX_IMG + k] = S.in_stage[IN_EX_IMG + k];
    } else if (S.retrieve) {
      DYB_REQUIRE(S.feat5_out && S.nrep == 1, DYB_ERR_ARG);
      RUN(dyb_scale_add(nullptr, P.acts + S.fca.off[5], nullptr, S.feat5_out, (size_t)0 + (size_t)B * 2048, st));   // B == 1: contiguous
      const void* exin[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
      if (S.retrieve(S.retrieve_user, level_index, exin) != 0) return DYB_ERR_ARG;
      for (int k = 0; k < 5; ++k) C.in[IN_EX_IMG + k] = exin[k];
    }
    DYB_REQUIRE(C.in[IN_EX_IMG] && C.in[IN_EX_KP] && C.in[IN_EX_POSE] && C.in[IN_EX_BETAS] && C.in[IN_EX_POSE3D], DYB_ERR_ARG);
    RUN(label_pass_forward_and_term(st, true));
  }
  if (C.losslog && S.full) {
    if (par && label) HIPOK(hipStreamWaitEvent(st, S.par_ev[4], 0));          // the row reads the label term's values
    hipLaunchKernelGGL(level_log_kernel, dim3(1, 1, dyb_rep_current().n), dim3(64), 0, st, (const float*)P.losses,
                       teacher ? (const float*)S.vals_t : nullptr, motion ? (const float*)S.vals_m : nullptr,
                       label ? (const float*)S.vals_l : nullptr, (float)S.teacher_w, (float)S.motion_w, (float)S.label_w,
                       C.losslog + 16 * level_index, dyb_rep_current());
    DYB_CHECK_LAUNCH();
  }
  // gradient of the level total: image pass (+ its external terms), history pass, exemplar pass
  {
    HostTimer t(S.h_bwd);
    // The weight gradients' fused update epilogues (DybWgradUpdateScope, igemm_conv.hip).  Lower level, "fuse_fast": theta_next = cur -
    // fastlr * g straight from the accumulators.  Upper level, "fuse_adam": it is
    // differentiated at the fast weights, so theta has no reader until the final inference - Adam may be applied layer by layer as the
    // weight gradients finish (replica groups; a previous frame's tail on the side stream is waited for first)
    S.fused_spans.clear();
    DybWgradUpdate upd{};
    if (fused_epilogues(S) && !upper && S.fuse_fast && S.theta_fast2) {
      upd = DybWgradUpdate{S.grads, S.n_params * sizeof(float), cur, nxt, (float)S.fastlr, &S.fused_spans};
    } else if (fused_epilogues(S) && upper && S.fuse_adam && cur != S.theta && S.nrep > 1) {
      // ("group_side") the previous frame's final inference may still read theta on the side stream: every writer of theta, the moments and
      // adam_sc below is on `st` or ordered behind it - the auxiliary stream's weight gradients wait for per-block events recorded on
      // `st` behind this point, the deferred set is issued behind them on the same in-order stream
      if (S.side_pending) {
        HIPOK(hipStreamWaitEvent(st, S.e_side, 0));
        S.side_pending = false;
      }
      RUN(adam_prepare(S, st));
      upd = DybWgradUpdate{S.grads, S.n_params * sizeof(float), S.theta, S.theta, 0.f, &S.fused_spans};
      upd.adam_m = S.adam_m; upd.adam_v = S.adam_v; upd.adam_sc = S.adam_sc;
      upd.b1 = (float)S.beta1; upd.b2 = (float)S.beta2; upd.eps = (float)S.eps;
    }
    DybWgradUpdateScope fuse(upd);
    RUN(pass_backward_ext(S, P, cur, S.grads, true, ext ? S.ext_rot : nullptr, ext ? S.ext_shape : nullptr, ext ? S.ext_cam : nullptr,
                          ext ? S.ext_joints : nullptr, st, aux));
  }
  // (the level's gradient = (image pass + history pass) + exemplar pass: the passes keep their own arenas and the weight update that
  // follows every level adds them while it reads them - no accumulation passes)
  S.lvl_g2 = S.lvl_g3 = nullptr;
  if (motion) {
    if (par) HIPOK(hipStreamWaitEvent(st, S.par_ev[3], 0));
    else RUN(pass_backward_ext(S, S.hist, cur, S.grads2, false, nullptr, nullptr, S.hg_cam, S.hg_joints, st, aux));
    S.lvl_g2 = S.grads2;
  }
  if (label) {
    if (par) HIPOK(hipStreamWaitEvent(st, S.par_ev[5], 0));
    else RUN(pass_backward_ext(S, S.ex, cur, S.grads3, false, S.exg_rot, S.exg_shape, S.exg_cam, S.exg_joints, st, aux));
    if (S.lvl_g2) S.lvl_g3 = S.grads3;
    else S.lvl_g2 = S.grads3;
  }
  tails.armed = false;                                    // both pass streams have been joined above
  return DYB_OK;
}
// optimizer.step() on every replica of the launch scope, then the teacher's EMA (full set; base_adaptor.py:193-201)
static int outer_update(Stepper& S, hipStream_t st, hipStream_t aux) {
  return weight_update(S, true, nullptr, nullptr, st, aux, S.full && S.use_teacher && S.teacher);
}
// features of two forwards -> 15 cosines per replica of the current scope (device log row + host-visible copy); cos12[r] (indexed
// by PHYSICAL replica) = cos[12] read from the host copy
static int gate_cosine(Stepper& S, const float* actsA, const float* actsB, float* log_row, float* cos12, hipStream_t st) {
  DYB_REQUIRE(S.gate_host, DYB_ERR_ARG);
  const DybRep& R = dyb_rep_current();
  S.gate_seq += 1.f;
  hipLaunchKernelGGL(feat_cos_kernel, dim3(15, 1, R.n), dim3(1024), 0, st, actsA, actsB, S.fca, 1e-12f, log_row, S.gate_host, S.gate_seq, R);
  DYB_CHECK_LAUNCH();
  // the one host wait of the dynamic loop (the reference's `.item()`, dynaboa_benchmark.py:165): a poll of pinned memory the
  // kernel writes, no stream synchronise / device-to-host copy call
  for (int i = 0; i < R.n; ++i) {
    const int r = dyb_rep_phys(R, i);
    long spins = 0;
    while (S.gate_host[16 * r + 15] != S.gate_seq) {
      if (++spins > 2000000000L) return DYB_ERR_LAUNCH;
      __builtin_ia32_pause();
    }
    cos12[r] = S.gate_host[16 * r + 12];
  }
  return DYB_OK;
}
static int stage_inputs(Stepper& S, const void* const* src, int ld, int k0, int nk, hipStream_t st) {
  DYB_REQUIRE(nk >= 1 && nk <= 5 && S.nrep > 1, DYB_ERR_ARG);
  const DybRep& R = dyb_rep_current();
  const size_t B = (size_t)S.B, img = B * 3 * (size_t)S.H * S.W;
  const size_t cnt[IN_COUNT] = {img, B * NJ * 3, B * 72, B * 10, B * 2, img, B * NJ * 3, img, B * NJ * 3, B * 72, B * 10, B * 24 * 4};
  GatherArgs g{};
  for (int k = 0; k < nk; ++k) {
    DYB_REQUIRE(S.in_stage[k0 + k], DYB_ERR_ARG);
    g.dst[k] = S.in_stage[k0 + k];
    g.n[k] = (unsigned)cnt[k0 + k];
    for (int i = 0; i < R.n; ++i) g.src[k][dyb_rep_phys(R, i)] = reinterpret_cast<const float*>(src[(size_t)k * ld + dyb_rep_phys(R, i)]);
  }
  hipLaunchKernelGGL(gather_inputs_kernel, dim3(64, nk, R.n), dim3(256), 0, st, g, R);
  DYB_CHECK_LAUNCH();
  return DYB_OK;
}
// The launch scope of a set of physical replicas: every per-replica arena of the stepper, map = the set.  DYB_ERR_UNSUPPORTED when
// the stepper's arenas do not fit the scope's DYB_MAX_ARENAS slots: with the full term set and replicas the separate records /
// loss_log / gate_log / feat5_out pointers are one too many - pass them as sub-buffers of ONE per-replica block through
// "logs_base" / "logs_bytes" (what the Python driver does); an arena silently left out would alias every replica onto replica 0's.
static int make_scope(const Stepper& S, const int* idx, int n, DybRep* out) {
  DybRep R{};
  dyb_rep_identity(R);
  dyb_rep_set_map(R, idx, n);
  bool overflow = false;
  auto arena = [&](const void* lo, size_t bytes) {
    if (!lo || !bytes) return;
    if (R.narenas >= DYB_MAX_ARENAS) { overflow = true; return; }
    R.lo[R.narenas] = reinterpret_cast<const char*>(lo);
    R.span[R.narenas] = bytes;
    R.stride[R.narenas] = bytes;
    ++R.narenas;
  };
  const int rows = S.inner_step + 1 + (S.full && S.dynamic ? S.optim_steps : 0);
  arena(S.wsp, S.blob);
  arena(S.theta, S.n_params * sizeof(float));
  arena(S.adam_m, S.n_params * sizeof(float));
  arena(S.adam_v, S.n_params * sizeof(float));
  if (S.full) arena(S.teacher, S.n_params * sizeof(float));
  if (S.results) {
    // the ring would be one arena too many on its own: a fifth sub-buffer of the ONE per-replica block, or refused
    const char *r0 = reinterpret_cast<const char*>(S.results), *r1 = r0 + (size_t)(S.result_capacity > 0 ? S.result_capacity : 0) * S.B * RESULT_FLOATS * sizeof(float);
    DYB_REQUIRE(S.logs_base && S.logs_bytes && r0 >= S.logs_base && r1 <= S.logs_base + S.logs_bytes, DYB_ERR_UNSUPPORTED);
  }
  if (S.logs_base && S.logs_bytes) {
    arena(S.logs_base, S.logs_bytes);              // records, loss_log, gate_log, feat5_out, results: sub-buffers of one per-replica block
  } else {
    arena(S.records, (size_t)S.record_capacity * a64((size_t)S.B * 85 + 1) * sizeof(float));
    arena(S.loss_log, (size_t)S.loss_capacity * (S.full ? 16 : 4) * rows * sizeof(float));
    if (S.full) {
      arena(S.gate_log, (size_t)S.loss_capacity * (1 + S.optim_steps) * 16 * sizeof(float));
      arena(S.feat5_out, (size_t)S.B * 2048 * sizeof(float));
    }
  }
  DYB_REQUIRE(!overflow, DYB_ERR_UNSUPPORTED);
  *out = R;
  return DYB_OK;
}
// the replicas the next frame step covers (ascending physical indices; n = 0: all).  Sequences of different lengths: a replica
// whose stream has ended simply leaves the set - its weights, Adam state and records stay as they are.
extern "C" int dyb_stepper_set_active(void* stepper, const int* idx, int n) {
  Stepper* S = reinterpret_cast<Stepper*>(stepper);
  DYB_REQUIRE(S && n >= 0 && n <= S->nrep && (n == 0 || idx), DYB_ERR_ARG);
  for (int i = 0; i < n; ++i) DYB_REQUIRE(idx[i] >= 0 && idx[i] < S->nrep && (i == 0 || idx[i] > idx[i - 1]), DYB_ERR_ARG);
  S->nactive = n;
  for (int i = 0; i < n; ++i) S->active[i] = idx[i];
  return DYB_OK;
}
static int active_set(const Stepper& S, int* idx) {
  if (S.nactive > 0) {
    for (int i = 0; i < S.nactive; ++i) idx[i] = S.active[i];
    return S.nactive;
  }
  for (int i = 0; i < S.nrep; ++i) idx[i] = i;
  return S.nrep;
}

// One adapted frame - Adaptor.adaptation (reference dynaboa_benchmark.py:126-193) - for every replica of the current launch scope (one
// replica without a scope), with the frame-loss set or, S.full, the reference's full term set.  C.in: the frame's inputs; gt_pose
// [B][72] / gt_betas [B][10] / gender [B] (int64) feed the metric records only (NULL with metrics = 0).  Records: inner_step
// (eval_lower) + 1 slots from record_slot in schedule order - after inner step 0, 1, ..., then the final one (+ one per step of the
// dynamic loop); loss rows: one per level at loss_slot (4 floats {s2d, shape prior, pose prior, weighted total}, full set: 16).
// side (frame-loss set, one sequence; may be NULL): stream for the final no-grad forward and its metrics, overlapped with the next
// frame's first level; the call orders the weight hazards itself.
// extra[r] (physical replica) receives the number of dynamic-loop iterations replica r took: the gate is evaluated per replica,
// and a replica whose feature 12 has stopped moving LEAVES the launch set of the remaining iterations (the others are not held
// back by it, and it does not take Adam steps the reference would not have taken).
static int frame_step(Stepper& S, LevelCtx& C, int record_slot, int loss_slot, int* extra, hipStream_t st, hipStream_t aux, hipStream_t side) {
  const bool metrics = S.metrics != 0;
  DYB_REQUIRE(C.in[IN_IMAGE] && C.in[IN_KP], DYB_ERR_ARG);
  DYB_REQUIRE(!metrics || (C.in[IN_GT_POSE] && C.in[IN_GT_BETAS] && C.in[IN_GENDER]), DYB_ERR_ARG);
  S.out_in_main = false;                                  // this frame's final inference goes to `fin` (reset at every entry point)
  if (!S.use_side || side == st) side = nullptr;
  // a tail owed by a call that had a side stream, and none now: nobody would issue it before this frame's update rewrites theta
  if (!side && (S.tail.on || S.gtjob.on) && S.tail_stream && S.tail_stream != st) RUN(issue_side_work(S, S.tail_stream));
  const float* image = (const float*)C.in[IN_IMAGE];
  const long long* gender = (const long long*)C.in[IN_GENDER];
  const int K = S.inner_step;
  const int rows = K + 1 + (S.full && S.dynamic ? S.optim_steps : 0);
  C.losslog = (S.loss_log && loss_slot >= 0 && loss_slot < S.loss_capacity) ? S.loss_log + (size_t)loss_slot * (S.full ? 16 : 4) * rows : nullptr;
  C.side = side;
  int slot = record_slot;
  const DybRep outer = dyb_rep_current();                 // (copy: nested scopes below replace the thread's current one)
  for (int i = 0; i < outer.n; ++i) extra[dyb_rep_phys(outer, i)] = 0;
  if (metrics) {
    // the ground-truth meshes only feed metric kernels: on the side stream when there is one, behind the previous frame's
    // tail (which still reads the buffers) - both are issued below, once this frame's first level is in the main queue
    if (side) {
      S.gtjob.on = true; S.gtjob.pose = (const float*)C.in[IN_GT_POSE]; S.gtjob.betas = (const float*)C.in[IN_GT_BETAS];
      S.gtjob.staged = S.nrep > 1;
    } else {
      if (S.side_pending) {                      // (the option was switched off between two frames) the last tail's record still reads them
        HIPOK(hipStreamWaitEvent(st, S.e_side, 0));
        S.side_pending = false;
      }
      RUN(gt_meshes(S, (const float*)C.in[IN_GT_POSE], (const float*)C.in[IN_GT_BETAS], st));
    }
  }
  C.gt_waited = !(metrics && side);
  HostTimer t_all(S.h_total);
  ++S.h_frames;
  const float* cur = S.theta;                    // clone(): the learner starts as an alias of theta
  for (int i = 0; i <= K; ++i) {                 // i < K: lower level + adapt; i == K: upper level
    Pass& P = (i == 0 && S.full && S.dynamic) ? S.lvl0 : S.main;     // level 0's features gate the dynamic loop
    // the next level's weights: the other fast buffer when the weight gradients may write them while data gradients still read `cur`
    float* nxt = (fused_epilogues(S) && S.fuse_fast && S.theta_fast2 && cur == S.theta_fast) ? S.theta_fast2 : S.theta_fast;
    RUN(level(S, C, P, cur, nxt, i == K, i, (metrics && S.eval_lower && i > 0) ? slot++ : -1, st, aux));
    if (i == 0 && side) {
      HostTimer t(S.h_tail);
      RUN(issue_side_work(S, side));
    }
    if (i < K) {
      HostTimer t(S.h_update);
      RUN(weight_update(S, false, cur, nxt, st, aux));
      cur = nxt;
    }
  }
  {
    HostTimer t_tail(S.h_tail);
    // optimizer.step(): theta is about to change in place - the previous frame's tail on the side stream reads it
    if (S.side_pending) {
      HIPOK(hipStreamWaitEvent(st, S.e_side, 0));
      S.side_pending = false;
    }
    RUN(outer_update(S, st, (side && S.nrep == 1) ? nullptr : aux));
    // final inference() with the updated weights (dynaboa_benchmark.py:156): in line, or - with a side stream - owed to the
    // next call / dyb_stepper_join (the caller keeps this frame's inputs alive until then)
    if (side && S.nrep > 1) {
      // "group_side": the final inference leaves the chain for the side stream, issued HERE, under this frame's launch scope and from
      // this frame's copy of the staged inputs.  Whoever reads theta / the moments on the chain's stream after this call (the caller,
      // the next frame's first level) must find the whole update done, so the chain's stream waits for every part of it that runs
      // elsewhere: the last range is issued now rather than from inside a forward, and the waits for the two ranges and the deferred
      // layer4 / regressor weight gradients are the chain's last commands of the frame.  The side forward is that update's consuming
      // forward: it takes the gates (behind e_theta: the fused epilogues the backward joined and the first range), so its stem ..
      // layer3 run while the auxiliary stream finishes, and the rest of it beside the next frame's first level.  Frame f + 1's outer
      // level waits for e_side before anything writes theta, the moments or adam_sc (level(), outer_update above); its lower levels'
      // weight gradients write the fast buffers and the gradient arena, never theta.  S.fin shares nothing with the chain or the
      // auxiliary stream's jobs: its own activation arena, engine workspace (split-K slabs, GroupNorm partials, both conv counter
      // regions), SMPL outputs and pred17; the ground-truth meshes it reads are written on the side stream itself (gtjob).
      hipEvent_t done[4] = {nullptr, nullptr, nullptr, nullptr};
      if (S.gates_pending) {
        if (S.gates.late) {
          HIPOK(hipEventRecord(S.gates.mid, st));
          RUN(late_update(&S));
        }
        done[0] = S.gates.ev[0]; done[1] = S.gates.ev[1]; done[2] = S.gates.l4; done[3] = S.gates.reg;
      }
      HIPOK(hipEventRecord(S.e_theta, st));
      for (hipEvent_t e : done)
        if (e) HIPOK(hipStreamWaitEvent(st, e, 0));
      HIPOK(hipStreamWaitEvent(side, S.e_theta, 0));
      RUN(pass_forward(S, S.fin, S.theta, image, side));
      RUN(settle_update(S, side));                       // (consumed by the forward above; a no-op unless that changes)
      if (metrics) RUN(record_metrics(S, S.fin, gender, slot++, side));
      RUN(pack_result(S, S.fin, loss_slot, side));
      HIPOK(hipEventRecord(S.e_side, side));
      S.side_pending = true;
      S.tail_stream = side;
      return DYB_OK;
    }
    if (side) {
      HIPOK(hipEventRecord(S.e_theta, st));
      S.tail.on = true; S.tail.image = image; S.tail.gender = gender; S.tail.slot = slot++; S.tail.metrics = metrics;
      S.tail.loss_slot = loss_slot;
      S.tail_stream = side;
      return DYB_OK;
    }
    RUN(pass_forward(S, S.fin, S.theta, image, st));
    RUN(settle_update(S, st));                         // (consumed by the forward above; a no-op unless that changes)
    if (metrics) RUN(record_metrics(S, S.fin, gender, slot++, st));
    RUN(pack_result(S, S.fin, loss_slot, st));
  }
  if (!(S.full && S.dynamic)) return DYB_OK;
  // dynaboa_benchmark.py:161-192: compare features of the un-adapted and the adapted forward; while feature 12 still
  // moves, repeat the upper level on the model itself (at most optim_steps times)
  float* glog = (S.gate_log && loss_slot >= 0 && loss_slot < S.loss_capacity) ? S.gate_log + (size_t)loss_slot * (1 + S.optim_steps) * 16 : nullptr;
  DYB_REQUIRE(glog, DYB_ERR_ARG);
  float cos12[DYB_MAX_REPLICAS];
  RUN(gate_cosine(S, S.lvl0.acts, S.fin.acts, glog, cos12, st));     // (inner_step 0: the upper level's own forward is lvl0)
  int cont[DYB_MAX_REPLICAS], ncont = 0;
  for (int i = 0; i < outer.n; ++i)
    if (1.f - cos12[dyb_rep_phys(outer, i)] > (float)S.cos_thr) cont[ncont++] = dyb_rep_phys(outer, i);
  int step = 0;
  Pass* post = &S.fin;                                   // where the latest final inference lives
  while (ncont > 0) {
    ++step;
    if (step > S.optim_steps) {
      for (int i = 0; i < ncont; ++i) extra[cont[i]] = S.optim_steps + 1;
      break;
    }
    {
      // the replicas still adapting get a scope of their own (one replica without replica machinery: the scope it came with)
      DybRep sub = outer;
      dyb_rep_set_map(sub, cont, ncont);
      DybRepScope scope(sub);
      // The upper level of this step starts with a forward at (theta, this image) - exactly the final inference the previous step
      // ended with (same weights, same image, deterministic kernels): it is not repeated.  `up` = that forward's products with the
      // chain's gradient buffers; the new final inference goes to the other activation arena (the gate compares the two), and the
      // two arenas swap roles every step ("share_dyn_fwd"; 0: the literal two forwards per step, main then fin).
      Pass up = S.main;
      Pass* nxt = &S.fin;
      if (S.share_dyn_fwd) {
        up.acts = post->acts; up.verts = post->verts; up.joints = post->joints; up.saved = post->saved; up.pred17 = post->pred17;
        nxt = (post == &S.fin) ? &S.main : &S.fin;
      }
      RUN(level(S, C, up, S.theta, nullptr, true, K + step, -1, st, aux, S.share_dyn_fwd != 0));
      RUN(outer_update(S, st, aux));
      RUN(pass_forward(S, *nxt, S.theta, image, st));
      RUN(gate_cosine(S, up.acts, nxt->acts, glog + 16 * step, cos12, st));
      if (metrics) RUN(record_metrics(S, *nxt, gender, slot, st));
      RUN(pack_result(S, *nxt, loss_slot, st));            // under the sub-scope: only the replicas still adapting overwrite their row
      post = nxt;
      S.out_in_main = (post == &S.main);
    }
    ++slot;
    int m = 0;
    for (int i = 0; i < ncont; ++i) {
      extra[cont[i]] = step;
      if (1.f - cos12[cont[i]] > (float)S.cos_thr) cont[m++] = cont[i];
    }
    ncont = m;
  }
  return DYB_OK;
}
// The frame step behind the four exported entry points.  inputs: HOST array of nk x replicas device pointers, kind-major -
// inputs[kind * replicas + r], r the PHYSICAL replica (entries of inactive replicas are ignored) - in IN_* order: nk = 5 kinds with
// the frame-loss set, 12 with the full term set.  One sequence: the step reads the callers' tensors; replicas (the active set,
// dyb_stepper_set_active): every launch of the chain covers all of them, their inputs are staged into the workspace first, and
// the terms must be alike for every active replica (lockstep).  extra_steps (may be NULL): `replicas` ints.
static int adapt(Stepper& S, const void* const* inputs, int nk, int record_slot, int loss_slot, int* extra_steps, hipStream_t st,
                 hipStream_t aux, hipStream_t side) {
  RUN(check_ready(S));
  DYB_REQUIRE((nk == IN_COUNT) == (S.full != 0) && (!S.full || S.B <= 16), DYB_ERR_UNSUPPORTED);
  // a frame step that fails must leave the bank's draw indices where they were: a retry draws the same members (ADVICE: stale state
  // survives an error return)
  struct DrawGuard {
    Stepper& S;
    unsigned long long saved[DYB_MAX_REPLICAS];
    bool ok = false;
    explicit DrawGuard(Stepper& s) : S(s) { memcpy(saved, S.bank_draw, sizeof saved); }
    ~DrawGuard() { if (!ok) memcpy(S.bank_draw, saved, sizeof saved); }
  } draws(S);
  const int n = S.nrep;
  int extra[DYB_MAX_REPLICAS] = {};
  LevelCtx C{};
  int rc;
  if (n == 1) {
    for (int k = 0; k < nk; ++k) C.in[k] = inputs[k];
    rc = frame_step(S, C, record_slot, loss_slot, extra, st, aux, side);
  } else {
    // replicas + side stream ("group_side"): the final inference of frame f on the side stream must not read staging buffers the next
    // call has refilled, nor run under the next frame's launch scope.  Frame-loss set: it reads its own copy of the
    // staged inputs (two copies, used in turn: the copy of frame f is staged into again by frame f + 2, whose chain has waited for
    // e_side at frame f + 1's outer level).  It is issued by its own call, under its own scope (frame_step).  The full term set and
    // the dynamic loop keep their tail in line and refuse a side stream.
    DYB_REQUIRE(!(S.use_side && side && side != st && S.full), DYB_ERR_UNSUPPORTED);
    if (!S.group_side) side = nullptr;
    if (S.in_stage_alt[0])
      for (int k = 0; k < 5; ++k) std::swap(S.in_stage[k], S.in_stage_alt[k]);
    int act[DYB_MAX_REPLICAS];
    const int na = active_set(S, act);
    auto have = [&](int r, int k0, int k1) {
      for (int k = k0; k <= k1; ++k)
        if (k >= nk || !inputs[k * n + r]) return false;
      return true;
    };
    const bool have_gt = have(act[0], IN_GT_POSE, IN_GENDER), have_hist = have(act[0], IN_HIST_IMAGE, IN_HIST_KP),
               have_ex = have(act[0], IN_EX_IMG, IN_EX_POSE3D);
    for (int i = 0; i < na; ++i) {
      DYB_REQUIRE(have(act[i], IN_IMAGE, IN_KP), DYB_ERR_ARG);
      DYB_REQUIRE(have(act[i], IN_GT_POSE, IN_GENDER) == have_gt && have(act[i], IN_HIST_IMAGE, IN_HIST_KP) == have_hist &&
                  have(act[i], IN_EX_IMG, IN_EX_POSE3D) == have_ex, DYB_ERR_UNSUPPORTED);     // lockstep: the same terms for every replica
    }
    DybRep R{};
    RUN(make_scope(S, act, na, &R));
    DybRepScope scope(R);
    RUN(stage_inputs(S, inputs, n, IN_IMAGE, 5, st));
    if (side && side != st) HIPOK(hipEventRecord(S.e_stage, st));      // the side stream's ground-truth meshes read the staged pose / betas
    if (have_hist) RUN(stage_inputs(S, inputs + (size_t)IN_HIST_IMAGE * n, n, IN_HIST_IMAGE, 2, st));
    if (have_ex) RUN(stage_inputs(S, inputs + (size_t)IN_EX_IMG * n, n, IN_EX_IMG, 5, st));
    for (int k = 0; k < nk; ++k) {
      const bool on = k <= IN_KP || (k <= IN_GENDER ? have_gt : k <= IN_HIST_KP ? have_hist : have_ex);
      C.in[k] = on ? S.in_stage[k] : nullptr;
    }
    rc = frame_step(S, C, record_slot, loss_slot, extra, st, aux, side);
  }
  if (extra_steps)
    for (int r = 0; r < n; ++r) extra_steps[r] = extra[r];
  draws.ok = rc == DYB_OK;
  return rc;
}
// One sequence, frame-loss set: image [B][3][H][W], kp2d [B][49][3]; gt_pose / gt_betas / gender may be NULL with metrics = 0.
extern "C" int dyb_stepper_adapt_frame(void* stepper, const float* image, const float* kp2d, const float* gt_pose,
                                       const float* gt_betas, const long long* gender, int record_slot, int loss_slot,
                                       hipStream_t st, hipStream_t aux, hipStream_t side) {
  Stepper* S = reinterpret_cast<Stepper*>(stepper);
  DYB_REQUIRE(S && image && kp2d && S->nrep == 1, DYB_ERR_ARG);
  const void* inputs[5] = {image, kp2d, gt_pose, gt_betas, gender};
  return adapt(*S, inputs, 5, record_slot, loss_slot, nullptr, st, aux, side);
}
// The same for the stepper's replicas: theta, adam_m, adam_v are [replicas][param floats], records [replicas][record_capacity]
// [record_floats], loss_log [replicas][loss_capacity][loss_floats], the workspace `replicas` blobs.  inputs: 5 x replicas pointers -
// image[r], kp2d[r], gt_pose[r], gt_betas[r], gender[r].
extern "C" int dyb_stepper_adapt_frames(void* stepper, const void* const* inputs, int record_slot, int loss_slot, hipStream_t st,
                                        hipStream_t aux, hipStream_t side) {
  Stepper* S = reinterpret_cast<Stepper*>(stepper);
  DYB_REQUIRE(S && inputs, DYB_ERR_ARG);
  return adapt(*S, inputs, 5, record_slot, loss_slot, nullptr, st, aux, side);
}
// One sequence, full term set: inputs = 12 pointers (image, kp2d, gt_pose, gt_betas, gender, hist_image, hist_kp, ex_img, ex_kp,
// ex_pose, ex_betas, ex_pose3d; the history pair NULL while there is no frame `interval` steps back, the exemplar five NULL when a
// retrieval callback is set).  *extra_steps receives the number of dynamic-loop iterations taken.
extern "C" int dyb_stepper_adapt_frame_full(void* stepper, const void* const* inputs, int record_slot, int loss_slot, int* extra_steps,
                                            hipStream_t st, hipStream_t aux) {
  Stepper* S = reinterpret_cast<Stepper*>(stepper);
  DYB_REQUIRE(S && inputs && extra_steps, DYB_ERR_ARG);
  DYB_REQUIRE(S->nrep == 1, DYB_ERR_UNSUPPORTED);
  return adapt(*S, inputs, IN_COUNT, record_slot, loss_slot, extra_steps, st, aux, nullptr);
}
// The same for the stepper's replicas, teacher / history / exemplar passes included: 12 x replicas pointers; the history pair must be
// present for all active replicas or for none; the exemplar five may be NULL when a per-replica retrieval callback
// ("retrieve_rep_fn") is set.  teacher is [replicas][param floats], gate_log [replicas][...], gate_host 16 floats per replica,
// feat5_out [replicas][B][2048].  extra_steps: `replicas` ints.
extern "C" int dyb_stepper_adapt_frames_full(void* stepper, const void* const* inputs, int record_slot, int loss_slot, int* extra_steps,
                                             hipStream_t st, hipStream_t aux) {
  Stepper* S = reinterpret_cast<Stepper*>(stepper);
  DYB_REQUIRE(S && inputs && extra_steps, DYB_ERR_ARG);
  return adapt(*S, inputs, IN_COUNT, record_slot, loss_slot, extra_steps, st, aux, nullptr);
}
// make `st` wait for everything the stepper has in flight on its side stream (before reading records / the final prediction)
extern "C" int dyb_stepper_join(void* stepper, hipStream_t st) {
  Stepper* S = reinterpret_cast<Stepper*>(stepper);
  DYB_REQUIRE(S, DYB_ERR_ARG);
  if ((S->tail.on || S->gtjob.on) && S->tail_stream) RUN(issue_side_work(*S, S->tail_stream));      // the last frame's final inference
  // (every frame step ends with a forward that consumed them; only a step that failed after its backward leaves deferred weight gradients behind)
  if (S->defer_pending && !S->gates_pending) RUN(settle_update(*S, st));
  if (S->side_pending) {
    HIPOK(hipStreamWaitEvent(st, S->e_side, 0));
    S->side_pending = false;
  }
  return DYB_OK;
}
// device locations of the last final-inference outputs: which = 0 rotmat [B][24][9], 1 state [B][160] (shape 144.., cam 154..),
// 2 vertices [B][6890][3], 3 joints [B][49][3]
extern "C" const float* dyb_stepper_output(const void* stepper, int which) {
  const Stepper* S = reinterpret_cast<const Stepper*>(stepper);
  if (!S || !S->bound) return nullptr;
  // (the dynamic loop's steps alternate between the two activation arenas, "share_dyn_fwd": the last launch's final inference - for a
  // replica that left the loop a step earlier than the last one, read its prediction from its row of the result ring, "results")
  const Pass& F = (S->out_in_main ? S->main : S->fin);
  switch (which) {
    case 0: return F.acts + S->off_rot;
    case 1: return F.acts + S->off_state;
    case 2: return F.verts;
    case 3: return F.joints;
    default: return nullptr;
  }
}
