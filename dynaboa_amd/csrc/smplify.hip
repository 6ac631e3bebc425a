// SMPLify (reference utils/smplify/): the optimisation-based fitter beside the regressor, on the device.
//   dyb_rodrigues_bwd          the gradient of rodrigues_kernel (smpl_lbs.hip): what lets an axis-angle pose be optimised at all
//   dyb_smplify_camera_loss    camera_fitting_loss (utils/smplify/losses.py:83-113), value and gradient per sample
//   dyb_smplify_body_loss      body_fitting_loss (losses.py:49-81), value, parts, [B][49] reprojection terms and gradient per sample
//   dyb_smplify_adam           torch.optim.Adam over the per-sample vector pose 72 | betas 10 | camera 3, one group of it at a time
//   dyb_smplify_fit            SMPLify.__call__ (utils/smplify/smplify.py:43-139): 2 x num_iters iterations issued by ONE call on one
//                              stream, no host synchronisation - per iteration rodrigues, LBS forward (3 launches), loss head, LBS
//                              backward (3), rodrigues backward, Adam: ten launches
// Latency class: one workgroup per sample, 49 joints in one wave, a 69-dimensional pose.  Samples never meet: the reference sums the
// loss over the batch and Adam is element-wise, so every kernel here reads and writes its own sample only, with a fixed reduction
// order (wave butterfly, no atomics) - two runs return equal bytes and sample b of a batch equals the run of sample b alone.
#include "dyb_common.h"
#include "dyb_gmm.h"

#define NJ49 49
#define NPOSE 72
#define NBODY 69
#define NBETA 10
#define NPARAM 85               // pose 72 | betas 10 | camera translation 3

// joints of the 49-joint convention by name (dynaboa_amd/constants.py JOINT_NAMES)
#define J_OP_NECK 1
#define J_OP_RSHO 2
#define J_OP_LSHO 5
#define J_OP_RHIP 9
#define J_OP_LHIP 12
#define J_GT_RHIP 27
#define J_GT_LHIP 28
#define J_GT_RSHO 33
#define J_GT_LSHO 34
// smplify.py:31  ign_joints = OP Neck, OP RHip, OP LHip, Right Hip, Left Hip
__device__ __forceinline__ bool smplify_ignored(int j) {
  return j == J_OP_NECK || j == J_OP_RHIP || j == J_OP_LHIP || j == J_GT_RHIP || j == J_GT_LHIP;
}

extern "C" int dyb_rodrigues_fwd(const float* aa, float* rotmat, int n, hipStream_t st);
extern "C" size_t dyb_lbs_saved_floats(int B);
extern "C" size_t dyb_lbs_bwd_workspace_bytes(int B);
extern "C" int dyb_lbs_fwd(const float* const* tables_f, const int* const* tables_i, const float* betas, int ldb, const float* rotmat,
                           float* verts, float* joints49, float* saved, int B, hipStream_t st);
extern "C" int dyb_lbs_bwd(const float* const* tables_f, const int* const* tables_i, const float* rotmat, const float* saved,
                           const float* djoints49, const float* dverts, float* drot, float* dbetas, int lddb, int B, void* ws,
                           size_t ws_bytes, hipStream_t st);

// ------------------------------------------------------------------------------------------
// gradient of rodrigues_kernel (smpl_lbs.hip), exactly as that kernel is written:
//   e = r + 1e-8, a = |e|, k = r / a (NOT e / a: the axis is un-normalised by up to 1e-8 / a), s = sin a, c1 = 1 - cos a,
//   R = I + s K(k) + c1 (k k^T - |k|^2 I).
// With G = dL/dR:   w = (G21 - G12, G02 - G20, G10 - G01),  dL/ds = k.w,  dL/dc1 = k^T G k - |k|^2 tr G,
//   dL/dk = s w + c1 ((G + G^T) k - 2 k tr G),   dL/da = dL/ds cos a + dL/dc1 sin a,
//   dL/dr = dL/dk / a + (dL/da - dL/dk . k / a) e / a          (k = r / a carries both the 1 / a and the a(r) dependence).
// At r = 0 exactly: k = 0, a = sqrt(3) 1e-8, and what is left is (sin a / a) w = w - finite, the generators' contraction, which is
// also what autograd of the formula returns there (the reference starts body poses at zero and lives by this gradient).
// c1 is formed as 2 sin^2(a / 2) here: 1 - cosf(a) is 0 below a = 3e-4 and dL/dk / a would lose c1 / a, up to 1e-4 of the gradient.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void rodrigues_bwd_kernel(const float* __restrict__ aa, const float* __restrict__ dR,
                                                           float* __restrict__ daa, int n) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  const float r[3] = {aa[(size_t)i * 3], aa[(size_t)i * 3 + 1], aa[(size_t)i * 3 + 2]};
  const float e[3] = {r[0] + 1e-8f, r[1] + 1e-8f, r[2] + 1e-8f};
  const float a = sqrtf(e[0] * e[0] + e[1] * e[1] + e[2] * e[2]);
  const float k[3] = {r[0] / a, r[1] / a, r[2] / a};
  const float s = sinf(a), c = cosf(a), sh = sinf(0.5f * a), c1 = 2.f * sh * sh;
  const float* G = dR + (size_t)i * 9;
  const float w[3] = {G[7] - G[5], G[2] - G[6], G[3] - G[1]};
  const float tr = G[0] + G[4] + G[8];
  const float k2 = k[0] * k[0] + k[1] * k[1] + k[2] * k[2];
  float Gk[3], Gtk[3];
  for (int p = 0; p < 3; ++p) {
    Gk[p] = G[p * 3] * k[0] + G[p * 3 + 1] * k[1] + G[p * 3 + 2] * k[2];
    Gtk[p] = G[p] * k[0] + G[3 + p] * k[1] + G[6 + p] * k[2];
  }
  const float g_s = k[0] * w[0] + k[1] * w[1] + k[2] * w[2];
  const float g_c1 = k[0] * Gk[0] + k[1] * Gk[1] + k[2] * Gk[2] - k2 * tr;
  float gk[3];
  for (int p = 0; p < 3; ++p) gk[p] = s * w[p] + c1 * (Gk[p] + Gtk[p] - 2.f * k[p] * tr);
  const float g_a = g_s * c + g_c1 * s;
  const float radial = (g_a - (gk[0] * k[0] + gk[1] * k[1] + gk[2] * k[2]) / a) / a;
  for (int p = 0; p < 3; ++p) daa[(size_t)i * 3 + p] = gk[p] / a + radial * e[p];
}
extern "C" int dyb_rodrigues_bwd(const float* aa, const float* drotmat, float* daa, int n, hipStream_t st) {
  DYB_REQUIRE(aa && drotmat && daa && n > 0, DYB_ERR_ARG);
  DYB_REQUIRE(dyb_rep_current().n == 1, DYB_ERR_UNSUPPORTED);
  hipLaunchKernelGGL(rodrigues_bwd_kernel, dim3(dyb_cdiv(n, 64)), dim3(64), 0, st, aa, drotmat, daa, n);
  DYB_CHECK_LAUNCH();
  return DYB_OK;
}

// perspective_projection (utils/geometry.py:63-91) with the identity rotation: p = f (x / z, y / z) + centre of one joint.
// The two heads evaluate a sample's 49 joints in DOUBLE on the float inputs and round each output once (the cost is nothing at this
// size).  In float, z = j_z + t_z rounds at the camera depth (half an ulp of 40 is 1.9e-6) and p at the pixel coordinate (of 150:
// 7.6e-6 px); behind f / z = 125 that is as much again as the error of the fp32 joints themselves (1e-7: 1.2e-5 px), and all of it
// lands, through the residual of a few pixels, in the gradients Adam normalises.
struct SmplifyProj {
  double x, y, z, px, py;
};
__device__ __forceinline__ SmplifyProj smplify_project(const float* __restrict__ j3, const float* __restrict__ t, double f,
                                                       const float* __restrict__ cen) {
  SmplifyProj P;
  P.x = (double)j3[0] + (double)t[0]; P.y = (double)j3[1] + (double)t[1]; P.z = (double)j3[2] + (double)t[2];
  P.px = f * (P.x / P.z) + (double)cen[0];
  P.py = f * (P.y / P.z) + (double)cen[1];
  return P;
}
// 64-lane butterfly sum of a double (the order of dyb_wave_sum)
__device__ __forceinline__ double smplify_wave_sum(double v) {
  v += __shfl_xor(v, 32);
  v += __shfl_xor(v, 16);
  v += __shfl_xor(v, 8);
  v += __shfl_xor(v, 4);
  v += __shfl_xor(v, 2);
  v += __shfl_xor(v, 1);
  return v;
}

// ------------------------------------------------------------------------------------------
// camera_fitting_loss (losses.py:83-113), one 64-lane workgroup per sample:
//   sum over the four torso joints of |kp - proj|^2  +  depth_w^2 (t_z - t_z_est)^2
// torso = the OpenPose hips / shoulders when all four of their confidences are > 0, else the ground-truth-style ones; per sample.
// kp [B][49][3] = (x, y, confidence).  loss [B], djoints [B][49][3] (zero outside the selected four), dcam_t [B][3].
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void smplify_camera_loss_kernel(const float* __restrict__ joints, const float* __restrict__ cam_t,
                                                                 const float* __restrict__ cam_t_est, const float* __restrict__ center,
                                                                 const float* __restrict__ kp, float focal, float depth_w,
                                                                 float* __restrict__ loss, float* __restrict__ djoints,
                                                                 float* __restrict__ dcam_t) {
  const int b = blockIdx.x, t = threadIdx.x;
  const float* K = kp + (size_t)b * NJ49 * 3;
  const float* T = cam_t + (size_t)b * 3;
  const float cmin = fminf(fminf(K[J_OP_RHIP * 3 + 2], K[J_OP_LHIP * 3 + 2]), fminf(K[J_OP_RSHO * 3 + 2], K[J_OP_LSHO * 3 + 2]));
  const bool op = cmin > 0.f;
  double l = 0.0, gx = 0.0, gy = 0.0, gz = 0.0;
  if (t < NJ49) {
    const bool sel = op ? (t == J_OP_RHIP || t == J_OP_LHIP || t == J_OP_RSHO || t == J_OP_LSHO)
                        : (t == J_GT_RHIP || t == J_GT_LHIP || t == J_GT_RSHO || t == J_GT_LSHO);
    if (sel) {
      const SmplifyProj P = smplify_project(joints + ((size_t)b * NJ49 + t) * 3, T, (double)focal, center + (size_t)b * 2);
      const double ex = P.px - (double)K[t * 3], ey = P.py - (double)K[t * 3 + 1];
      l = ex * ex + ey * ey;
      gx = 2.0 * ex * (double)focal / P.z;
      gy = 2.0 * ey * (double)focal / P.z;
      gz = -(gx * P.x + gy * P.y) / P.z;
    }
    float* d = djoints + ((size_t)b * NJ49 + t) * 3;
    d[0] = (float)gx; d[1] = (float)gy; d[2] = (float)gz;
  }
  l = smplify_wave_sum(l); gx = smplify_wave_sum(gx); gy = smplify_wave_sum(gy); gz = smplify_wave_sum(gz);
  if (t == 0) {
    const double dz = (double)T[2] - (double)cam_t_est[(size_t)b * 3 + 2], w2 = (double)depth_w * (double)depth_w;
    loss[b] = (float)(l + w2 * (dz * dz));
    dcam_t[(size_t)b * 3] = (float)gx;
    dcam_t[(size_t)b * 3 + 1] = (float)gy;
    dcam_t[(size_t)b * 3 + 2] = (float)(gz + 2.0 * w2 * dz);
  }
}
extern "C" int dyb_smplify_camera_loss(const float* joints49, const float* cam_t, const float* cam_t_est, const float* center,
                                       const float* kp2d, float focal, float depth_weight, float* loss, float* djoints49,
                                       float* dcam_t, int B, hipStream_t st) {
  DYB_REQUIRE(joints49 && cam_t && cam_t_est && center && kp2d && loss && djoints49 && dcam_t && B > 0, DYB_ERR_ARG);
  DYB_REQUIRE(dyb_rep_current().n == 1, DYB_ERR_UNSUPPORTED);
  hipLaunchKernelGGL(smplify_camera_loss_kernel, dim3(B), dim3(64), 0, st, joints49, cam_t, cam_t_est, center, kp2d, focal, depth_weight,
                     loss, djoints49, dcam_t);
  DYB_CHECK_LAUNCH();
  return DYB_OK;
}

// ------------------------------------------------------------------------------------------
// body_fitting_loss (losses.py:49-81), one 256-thread workgroup per sample:
//   reproj[j] = conf_j^2 (gmof(px - kx) + gmof(py - ky)),  gmof(d) = sigma^2 d^2 / (sigma^2 + d^2)
//   total = sum_j reproj[j] + wp^2 gmm(pose) + wa^2 sum exp(+-pose[52, 55, 9, 12])^2 + ws^2 |betas|^2
// ignore != 0: the five joints of smplify.py:31 count with confidence 0 (the caller's keypoints are not written).
// parts [B][5] = (reprojection sum, pose prior, angle prior, shape prior, total), the priors weighted; total_out [B] (may be NULL)
// receives the total as well (the fit's loss log).  dcam_t may be NULL (stage 2 of the fit holds the camera fixed).
// ------------------------------------------------------------------------------------------
struct SmplifyBodyArgs {
  const float *pose69, *betas, *joints, *cam_t, *center, *kp, *means, *prec, *logw;
  int ldp, ldb, ignore;
  float focal, sigma, w_pose, w_shape, w_angle;
  float *parts, *reproj, *total_out, *djoints, *dpose69, *dbetas, *dcam_t;
  int lddp, lddb;
};
__global__ __launch_bounds__(256) void smplify_body_loss_kernel(SmplifyBodyArgs a) {
  __shared__ DybGmmShared S;
  __shared__ double sRed[4];
  const int b = blockIdx.x, t = threadIdx.x;
  const float* pose = a.pose69 + (size_t)b * a.ldp;
  if (t < 64) {                                     // wave 0: the 49 joints
    double l = 0.0, gx = 0.0, gy = 0.0, gz = 0.0;
    if (t < NJ49) {
      const float* K = a.kp + ((size_t)b * NJ49 + t) * 3;
      const double conf = (a.ignore && smplify_ignored(t)) ? 0.0 : (double)K[2];
      const SmplifyProj P = smplify_project(a.joints + ((size_t)b * NJ49 + t) * 3, a.cam_t + (size_t)b * 3, (double)a.focal,
                                            a.center + (size_t)b * 2);
      const double s2 = (double)a.sigma * (double)a.sigma, c2 = conf * conf;
      const double dx = P.px - (double)K[0], dy = P.py - (double)K[1];
      const double qx = s2 + dx * dx, qy = s2 + dy * dy;
      l = c2 * ((s2 * (dx * dx)) / qx + (s2 * (dy * dy)) / qy);
      const double hx = c2 * 2.0 * dx * (s2 / qx) * (s2 / qx), hy = c2 * 2.0 * dy * (s2 / qy) * (s2 / qy);     // d gmof / d d = 2 d s2^2 / q^2
      gx = hx * (double)a.focal / P.z;
      gy = hy * (double)a.focal / P.z;
      gz = -(gx * P.x + gy * P.y) / P.z;
      a.reproj[(size_t)b * NJ49 + t] = (float)l;
      float* d = a.djoints + ((size_t)b * NJ49 + t) * 3;
      d[0] = (float)gx; d[1] = (float)gy; d[2] = (float)gz;
    }
    l = smplify_wave_sum(l); gx = smplify_wave_sum(gx); gy = smplify_wave_sum(gy); gz = smplify_wave_sum(gz);
    if (t == 0) { sRed[0] = l; sRed[1] = gx; sRed[2] = gy; sRed[3] = gz; }
  }
  dyb_gmm_eval<256>(pose, a.means, a.prec, a.logw, S, t);          // (its barriers also publish sRed)
  const double wp2 = (double)a.w_pose * (double)a.w_pose, wa2 = (double)a.w_angle * (double)a.w_angle, ws2 = (double)a.w_shape * (double)a.w_shape;
  if (t < NBODY) {
    double g = wp2 * (double)dyb_gmm_grad(S, t);
    // angle_prior (losses.py:19-24): exp(pose[52]), exp(-pose[55]), exp(-pose[9]), exp(-pose[12]), each squared
    if (t == 52 || t == 55 || t == 9 || t == 12) {
      const double sg = t == 52 ? 1.0 : -1.0, ex = exp(sg * (double)pose[t]);
      g += wa2 * 2.0 * sg * (ex * ex);
    }
    a.dpose69[(size_t)b * a.lddp + t] = (float)g;
  } else if (t >= 128 && t < 128 + NBETA) {
    a.dbetas[(size_t)b * a.lddb + (t - 128)] = (float)(2.0 * ws2 * (double)a.betas[(size_t)b * a.ldb + (t - 128)]);
  }
  if (t == 0) {
    const double e0 = exp((double)pose[52]), e1 = exp(-(double)pose[55]), e2 = exp(-(double)pose[9]), e3 = exp(-(double)pose[12]);
    const double ang = wa2 * (e0 * e0 + e1 * e1 + e2 * e2 + e3 * e3);
    double sb = 0.0;
    for (int l = 0; l < NBETA; ++l) { const double v = (double)a.betas[(size_t)b * a.ldb + l]; sb += v * v; }
    const double shp = ws2 * sb, pri = wp2 * (double)S.Q[S.best];
    const double tot = sRed[0] + pri + ang + shp;
    float* o = a.parts + (size_t)b * 5;
    o[0] = (float)sRed[0]; o[1] = (float)pri; o[2] = (float)ang; o[3] = (float)shp; o[4] = (float)tot;
    if (a.total_out) a.total_out[b] = (float)tot;
    if (a.dcam_t) { a.dcam_t[(size_t)b * 3] = (float)sRed[1]; a.dcam_t[(size_t)b * 3 + 1] = (float)sRed[2]; a.dcam_t[(size_t)b * 3 + 2] = (float)sRed[3]; }
  }
}
extern "C" int dyb_smplify_body_loss(const float* pose69, int ldp, const float* betas, int ldb, const float* joints49, const float* cam_t,
                                     const float* center, const float* kp2d, const float* gmm_means, const float* gmm_prec,
                                     const float* gmm_logw, float focal, float sigma, float pose_prior_weight, float shape_prior_weight,
                                     float angle_prior_weight, int ignore, float* parts, float* reproj, float* total_out, float* djoints49,
                                     float* dpose69, int lddp, float* dbetas, int lddb, float* dcam_t, int B, hipStream_t st) {
  DYB_REQUIRE(pose69 && betas && joints49 && cam_t && center && kp2d && gmm_means && gmm_prec && gmm_logw, DYB_ERR_ARG);
  DYB_REQUIRE(parts && reproj && djoints49 && dpose69 && dbetas && B > 0, DYB_ERR_ARG);
  DYB_REQUIRE(ldp >= NBODY && ldb >= NBETA && lddp >= NBODY && lddb >= NBETA, DYB_ERR_ARG);
  DYB_REQUIRE(dyb_rep_current().n == 1, DYB_ERR_UNSUPPORTED);
  SmplifyBodyArgs a;
  a.pose69 = pose69; a.betas = betas; a.joints = joints49; a.cam_t = cam_t; a.center = center; a.kp = kp2d;
  a.means = gmm_means; a.prec = gmm_prec; a.logw = gmm_logw;
  a.ldp = ldp; a.ldb = ldb; a.ignore = ignore;
  a.focal = focal; a.sigma = sigma; a.w_pose = pose_prior_weight; a.w_shape = shape_prior_weight; a.w_angle = angle_prior_weight;
  a.parts = parts; a.reproj = reproj; a.total_out = total_out; a.djoints = djoints49; a.dpose69 = dpose69; a.dbetas = dbetas;
  a.dcam_t = dcam_t; a.lddp = lddp; a.lddb = lddb;
  hipLaunchKernelGGL(smplify_body_loss_kernel, dim3(B), dim3(256), 0, st, a);
  DYB_CHECK_LAUNCH();
  return DYB_OK;
}

// ------------------------------------------------------------------------------------------
// torch.optim.Adam (no amsgrad, no weight decay) over the per-sample vector  pose 72 | betas 10 | camera translation 3, one
// 128-thread workgroup per sample.  group 1 = {global orientation, camera translation} (elements 0..2, 82..84: stage 1 of the fit),
// group 2 = {global orientation, body pose, betas} (elements 0..81: stage 2); the other elements and their moments are left alone.
// The gradient of an element is g (+ g_extra where given: the body loss's direct gradient to the body pose / betas, beside the one
// that arrives through LBS).  state = m [B][85] | v [B][85] | step [B] (int): dyb_smplify_adam_state_bytes(B).  restart != 0: the
// step starts from zero moments and step count 0 whatever the state holds (a new optimiser: each stage of the fit).
// Arithmetic order of dyb_adam_one (dyb_common.h), with the weights 1 - beta formed in double and rounded once, as torch passes them
// (1.f - 0.999f is 1.3e-5 away from float(1 - 0.999), and v carries that factor into the very first step).
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ void smplify_adam_one(float& p, float g, float& m, float& v, float omb1, float b2, float omb2, float step_size,
                                                 float bc2_sqrt, float eps) {
#pragma clang fp contract(off)
  m = fmaf(omb1, g - m, m);
  const float g1 = omb2 * g;
  v = fmaf(g1, g, v * b2);
  const float denom = sqrtf(v) / bc2_sqrt + eps;
  p = fmaf(-step_size, m / denom, p);
}
struct SmplifyAdamArgs {
  float *pose, *betas, *cam_t;
  const float *dpose, *dbody_extra, *dbetas, *dbetas_extra, *dcam_t;
  float *m, *v;
  int* step;
  int ldp, ldb, lddx, lddbx, group, restart;
  double lr, beta1, beta2, eps;
};
__global__ __launch_bounds__(128) void smplify_adam_kernel(SmplifyAdamArgs a) {
  const int b = blockIdx.x, t = threadIdx.x;
  const int step = (a.restart ? 0 : a.step[b]) + 1;
  __syncthreads();                                   // every work-item has read the count before it is advanced
  if (t == 0) a.step[b] = step;
  const bool live = a.group == 1 ? (t < 3 || (t >= NPOSE + NBETA && t < NPARAM)) : (t < NPOSE + NBETA);
  if (!live) return;
  float* p;
  float g;
  if (t < NPOSE) {
    p = a.pose + (size_t)b * a.ldp + t;
    g = a.dpose[(size_t)b * NPOSE + t];
    if (a.dbody_extra && t >= 3) g += a.dbody_extra[(size_t)b * a.lddx + (t - 3)];
  } else if (t < NPOSE + NBETA) {
    p = a.betas + (size_t)b * a.ldb + (t - NPOSE);
    g = a.dbetas[(size_t)b * NBETA + (t - NPOSE)];
    if (a.dbetas_extra) g += a.dbetas_extra[(size_t)b * a.lddbx + (t - NPOSE)];
  } else {
    p = a.cam_t + (size_t)b * 3 + (t - NPOSE - NBETA);
    g = a.dcam_t[(size_t)b * 3 + (t - NPOSE - NBETA)];
  }
  const double bc1 = 1.0 - pow(a.beta1, (double)step), bc2 = 1.0 - pow(a.beta2, (double)step);
  const float step_size = (float)(a.lr / bc1), bc2_sqrt = (float)sqrt(bc2);
  const size_t i = (size_t)b * NPARAM + t;
  float pv = *p, m = a.restart ? 0.f : a.m[i], v = a.restart ? 0.f : a.v[i];
  smplify_adam_one(pv, g, m, v, (float)(1.0 - a.beta1), (float)a.beta2, (float)(1.0 - a.beta2), step_size, bc2_sqrt, (float)a.eps);
  *p = pv; a.m[i] = m; a.v[i] = v;
}
extern "C" size_t dyb_smplify_adam_state_bytes(int B) { return (size_t)B * (2 * NPARAM * sizeof(float) + sizeof(int)); }
// pose [B][ldp] (72 used), betas [B][ldb] (10 used), cam_t [B][3]; dpose [B][72], dbetas [B][10], dcam_t [B][3] (may be NULL for group 2);
// dbody_extra [B][lddx] (69 used) and dbetas_extra [B][lddbx] may be NULL.
extern "C" int dyb_smplify_adam(float* pose, int ldp, float* betas, int ldb, float* cam_t, const float* dpose, const float* dbody_extra,
                                int lddx, const float* dbetas, const float* dbetas_extra, int lddbx, const float* dcam_t, void* state,
                                size_t state_bytes, int group, int restart, double lr, double beta1, double beta2, double eps, int B,
                                hipStream_t st) {
  DYB_REQUIRE(pose && betas && cam_t && dpose && state && B > 0 && (group == 1 || group == 2), DYB_ERR_ARG);
  DYB_REQUIRE(group == 1 ? dcam_t != nullptr : dbetas != nullptr, DYB_ERR_ARG);
  DYB_REQUIRE(ldp >= NPOSE && ldb >= NBETA && (!dbody_extra || lddx >= NBODY) && (!dbetas_extra || lddbx >= NBETA), DYB_ERR_ARG);
  DYB_REQUIRE(state_bytes >= dyb_smplify_adam_state_bytes(B), DYB_ERR_WORKSPACE);
  DYB_REQUIRE(dyb_rep_current().n == 1, DYB_ERR_UNSUPPORTED);
  SmplifyAdamArgs a;
  a.pose = pose; a.betas = betas; a.cam_t = cam_t;
  a.dpose = dpose; a.dbody_extra = dbody_extra; a.dbetas = dbetas; a.dbetas_extra = dbetas_extra; a.dcam_t = dcam_t;
  a.m = reinterpret_cast<float*>(state);
  a.v = a.m + (size_t)B * NPARAM;
  a.step = reinterpret_cast<int*>(a.v + (size_t)B * NPARAM);
  a.ldp = ldp; a.ldb = ldb; a.lddx = lddx; a.lddbx = lddbx; a.group = group; a.restart = restart;
  a.lr = lr; a.beta1 = beta1; a.beta2 = beta2; a.eps = eps;
  hipLaunchKernelGGL(smplify_adam_kernel, dim3(B), dim3(128), 0, st, a);
  DYB_CHECK_LAUNCH();
  return DYB_OK;
}

// ------------------------------------------------------------------------------------------
// SMPLify.__call__ (smplify.py:43-139) in one call.  The optimised values live in the OUTPUT arrays (pose, betas, cam_t), which
// start as copies of the initial ones; the caller's keypoints are read only (the reference zeroes the ignored confidences in place).
// ------------------------------------------------------------------------------------------
#define SMPLIFY_SIGMA 100.f                 // the defaults of losses.py:49-53, :83-84 - what SMPLify.__call__ runs with
#define SMPLIFY_W_POSE 4.78f
#define SMPLIFY_W_SHAPE 5.f
#define SMPLIFY_W_ANGLE 15.2f
#define SMPLIFY_W_DEPTH 100.f
static inline size_t smplify_pad(size_t floats) { return (floats + 63) / 64 * 64; }
struct SmplifyWs {
  float *rot, *saved, *drot, *djoints, *dpose, *dbody, *dbetas, *dbetas_x, *dcam, *parts, *loss, *state, *lbs_ws;
  size_t lbs_ws_bytes, total_floats;
};
static SmplifyWs smplify_carve(float* base, int B) {
  SmplifyWs w;
  size_t o = 0;
  auto take = [&](size_t n) { float* p = base ? base + o : nullptr; o += smplify_pad(n); return p; };
  w.rot = take((size_t)B * 216);
  w.saved = take(dyb_lbs_saved_floats(B));
  w.drot = take((size_t)B * 216);
  w.djoints = take((size_t)B * NJ49 * 3);
  w.dpose = take((size_t)B * NPOSE);
  w.dbody = take((size_t)B * NBODY);
  w.dbetas = take((size_t)B * NBETA);
  w.dbetas_x = take((size_t)B * NBETA);
  w.dcam = take((size_t)B * 3);
  w.parts = take((size_t)B * 5);
  w.loss = take((size_t)B);
  w.state = take((dyb_smplify_adam_state_bytes(B) + 3) / 4);
  w.lbs_ws_bytes = dyb_lbs_bwd_workspace_bytes(B);
  w.lbs_ws = take((w.lbs_ws_bytes + 3) / 4);
  w.total_floats = o;
  return w;
}
extern "C" size_t dyb_smplify_fit_workspace_bytes(int B) { return B > 0 ? smplify_carve(nullptr, B).total_floats * sizeof(float) : 0; }

// init_pose [B][72] axis-angle, init_betas [B][10], init_cam_t [B][3], center [B][2], kp2d [B][49][3] (x, y, confidence).
// Outputs: verts [B][6890][3], joints49 [B][49][3], pose [B][72], betas [B][10], cam_t [B][3], reproj [B][49] (the final
// body_fitting_loss(output='reprojection') with the five joints ignored); loss_log (may be NULL) [2 * num_iters][B]: the per-sample
// total each iteration evaluated BEFORE its step - rows 0..num_iters-1 the camera loss, the rest the body loss.  num_iters = 0
// evaluates the initial values.  Adam: lr, betas (0.9, 0.999), eps 1e-8, a new optimiser per stage.
extern "C" int dyb_smplify_fit(const float* const* tables_f, const int* const* tables_i, const float* gmm_means, const float* gmm_prec,
                               const float* gmm_logw, const float* init_pose, const float* init_betas, const float* init_cam_t,
                               const float* center, const float* kp2d, int num_iters, double lr, float focal, float* verts,
                               float* joints49, float* pose, float* betas, float* cam_t, float* reproj, float* loss_log, int B, void* ws,
                               size_t ws_bytes, hipStream_t st) {
  DYB_REQUIRE(tables_f && tables_i && gmm_means && gmm_prec && gmm_logw && init_pose && init_betas && init_cam_t && center && kp2d, DYB_ERR_ARG);
  DYB_REQUIRE(verts && joints49 && pose && betas && cam_t && reproj && ws && B > 0 && num_iters >= 0, DYB_ERR_ARG);
  DYB_REQUIRE(ws_bytes >= dyb_smplify_fit_workspace_bytes(B), DYB_ERR_WORKSPACE);
  DYB_REQUIRE(dyb_rep_current().n == 1, DYB_ERR_UNSUPPORTED);
  const SmplifyWs w = smplify_carve(reinterpret_cast<float*>(ws), B);
  const size_t state_bytes = dyb_smplify_adam_state_bytes(B);
  if (hipMemcpyAsync(pose, init_pose, (size_t)B * NPOSE * sizeof(float), hipMemcpyDeviceToDevice, st) != hipSuccess) return DYB_ERR_LAUNCH;
  if (hipMemcpyAsync(betas, init_betas, (size_t)B * NBETA * sizeof(float), hipMemcpyDeviceToDevice, st) != hipSuccess) return DYB_ERR_LAUNCH;
  if (hipMemcpyAsync(cam_t, init_cam_t, (size_t)B * 3 * sizeof(float), hipMemcpyDeviceToDevice, st) != hipSuccess) return DYB_ERR_LAUNCH;
  int rc;
#define SMPLIFY_TRY(call) \
  do {                    \
    rc = (call);          \
    if (rc != DYB_OK) return rc; \
  } while (0)
  for (int stage = 1; stage <= 2; ++stage) {
    for (int it = 0; it < num_iters; ++it) {
      float* log = loss_log ? loss_log + ((size_t)(stage - 1) * num_iters + it) * B : nullptr;
      SMPLIFY_TRY(dyb_rodrigues_fwd(pose, w.rot, B * 24, st));
      SMPLIFY_TRY(dyb_lbs_fwd(tables_f, tables_i, betas, NBETA, w.rot, verts, joints49, w.saved, B, st));
      if (stage == 1)
        SMPLIFY_TRY(dyb_smplify_camera_loss(joints49, cam_t, init_cam_t, center, kp2d, focal, SMPLIFY_W_DEPTH, log ? log : w.loss, w.djoints,
                                            w.dcam, B, st));
      else
        SMPLIFY_TRY(dyb_smplify_body_loss(pose + 3, NPOSE, betas, NBETA, joints49, cam_t, center, kp2d, gmm_means, gmm_prec, gmm_logw, focal,
                                          SMPLIFY_SIGMA, SMPLIFY_W_POSE, SMPLIFY_W_SHAPE, SMPLIFY_W_ANGLE, 1, w.parts, reproj, log, w.djoints,
                                          w.dbody, NBODY, w.dbetas_x, NBETA, nullptr, B, st));
      SMPLIFY_TRY(dyb_lbs_bwd(tables_f, tables_i, w.rot, w.saved, w.djoints, nullptr, w.drot, w.dbetas, NBETA, B, w.lbs_ws, w.lbs_ws_bytes, st));
      SMPLIFY_TRY(dyb_rodrigues_bwd(pose, w.drot, w.dpose, B * 24, st));
      if (stage == 1)
        SMPLIFY_TRY(dyb_smplify_adam(pose, NPOSE, betas, NBETA, cam_t, w.dpose, nullptr, 0, w.dbetas, nullptr, 0, w.dcam, w.state, state_bytes,
                                     1, it == 0, lr, 0.9, 0.999, 1e-8, B, st));
      else
        SMPLIFY_TRY(dyb_smplify_adam(pose, NPOSE, betas, NBETA, cam_t, w.dpose, w.dbody, NBODY, w.dbetas, w.dbetas_x, NBETA, nullptr, w.state,
                                     state_bytes, 2, it == 0, lr, 0.9, 0.999, 1e-8, B, st));
    }
  }
  // the final forward and the reprojection terms it is judged by
  SMPLIFY_TRY(dyb_rodrigues_fwd(pose, w.rot, B * 24, st));
  SMPLIFY_TRY(dyb_lbs_fwd(tables_f, tables_i, betas, NBETA, w.rot, verts, joints49, w.saved, B, st));
  SMPLIFY_TRY(dyb_smplify_body_loss(pose + 3, NPOSE, betas, NBETA, joints49, cam_t, center, kp2d, gmm_means, gmm_prec, gmm_logw, focal,
                                    SMPLIFY_SIGMA, SMPLIFY_W_POSE, SMPLIFY_W_SHAPE, SMPLIFY_W_ANGLE, 1, w.parts, reproj, nullptr, w.djoints, w.dbody,
                                    NBODY, w.dbetas_x, NBETA, nullptr, B, st));
#undef SMPLIFY_TRY
  return DYB_OK;
}
