// The frame-loss head and its second derivative along a state tangent in one call (--hvp exact --hvp_head closed).
//
//   state [B][157] -> rot6d -> SMPL -> projection / priors -> loss;     d_state = gradient,   td_state = H_head(state) . tstate
//
// Forward-over-reverse, like the backbone (hvp_engine.inc): the tangent of the forward chain first (rot6d, LBS), then the tangent of
// every backward stage (loss gradients, LBS backward, combine, rot6d backward).  Each stage is the (value, tangent) instantiation of
// the kernel that computes the gradient (dyb_dual.h): one sweep over the tables yields value and tangent, 12 launches.
// The value half of that pass is the gradient in the same arithmetic, but not in the same bits: hipcc contracts multiply-adds of the
// two instantiations differently (on the MI355X the last bit of a few percent of the elements differs; on a host build without fused
// multiply-add they are identical).  d_state is promised to be the first-order head's gradient bit for bit, so it is produced by
// the float kernels themselves in a second, value-only pass (11 launches) that overwrites the first pass's value half.
// No host arithmetic in between.  Single sequence (no replica scope).
#include "dyb_common.h"

// the stage entry points (smpl_lbs.hip, losses.hip; declared for callers in include/dynaboa_hip.h)
extern "C" {
int dyb_rot6d_fwd(const float* x6, int ldx, float* rotmat, int B, hipStream_t st);
int dyb_rot6d_bwd(const float* x6, int ldx, const float* drotmat, float* dx6, int lddx, int B, hipStream_t st);
int dyb_lbs_fwd(const float* const* tables_f, const int* const* tables_i, const float* betas, int ldb, const float* rotmat, float* verts,
                float* joints49, float* saved, int B, hipStream_t st);
int dyb_lbs_bwd(const float* const* tables_f, const int* const* tables_i, const float* rotmat, const float* saved,
                const float* djoints49, const float* dverts, float* drot, float* dbetas, int lddb, int B, void* ws, size_t ws_bytes,
                hipStream_t st);
int dyb_frame_losses(const float* rotmat, const float* shape, int lds, const float* cam, int ldc, const float* joints49,
                     const float* kp2d, const float* gmm_means, const float* gmm_prec, const float* gmm_logw, float w2d, float wshape,
                     float wpose, float* losses_out, float* drot, float* dshape, int ldds, float* dcam, int lddc, float* djoints49, int B,
                     void* ws, size_t ws_bytes, hipStream_t st);
size_t dyb_lbs_saved_floats(int B);
size_t dyb_lbs_bwd_workspace_bytes(int B);
int dyb_rot6d_jvp(const float* x6, const float* tx6, int ldx, float* rotmat, float* trotmat, int B, hipStream_t st);
int dyb_rot6d_bwd_jvp(const float* x6, const float* tx6, int ldx, const float* drotmat, const float* tdrotmat, float* dx6,
                      float* tdx6, int lddx, int B, hipStream_t st);
int dyb_lbs_jvp(const float* const* tables_f, const int* const* tables_i, const float* betas, const float* tbetas, int ldb,
                const float* rotmat, const float* trotmat, float* verts, float* tverts, float* joints49, float* tjoints49,
                float* saved, float* tsaved, int B, hipStream_t st);
int dyb_lbs_bwd_jvp(const float* const* tables_f, const int* const* tables_i, const float* rotmat, const float* trotmat,
                    const float* saved, const float* tsaved, const float* djoints49, const float* tdjoints49, float* drot,
                    float* tdrot, float* dbetas, float* tdbetas, int lddb, int B, void* ws, size_t ws_bytes, hipStream_t st);
int dyb_frame_losses_jvp(const float* rotmat, const float* trotmat, const float* shape, const float* tshape, int lds,
                         const float* cam, const float* tcam, int ldc, const float* joints49, const float* tjoints49,
                         const float* kp2d, const float* gmm_means, const float* gmm_prec, const float* gmm_logw, float w2d,
                         float wshape, float wpose, float* losses_out, float* drot, float* tdrot, float* dshape, float* tdshape,
                         int ldds, float* dcam, float* tdcam, int lddc, float* djoints49, float* tdjoints49, int B, void* ws,
                         size_t ws_bytes, hipStream_t st);
}

#define HH_NV 6890
#define HH_STATE 157

// d_rot = drot_l + drot_s; d_state[144..153] = dshape_l + dbetas_s; d_state[154..156] = dcam_l; d_state[157..ldd) = 0 - for the
// value arrays (blockIdx.y 0) and the tangent arrays (1) alike: the combination is linear.  Rounds as head_grad_kernel does with
// g = NULL and no external terms (1 * a + b + 0: one rounding however the multiply-add is contracted).
struct HeadHvpCombineArgs {
  const float *drot_l[2], *drot_s[2], *dshape_l[2], *dbetas_s[2], *dcam_l[2];
  float *d_rot[2], *d_state[2];
  int B, ldd;
};
__global__ __launch_bounds__(256) void head_hvp_combine_kernel(HeadHvpCombineArgs a) {
  const int per = 216 + (a.ldd - 144);
  const int which = blockIdx.y;
  const float *drot_l = which ? a.drot_l[1] : a.drot_l[0], *drot_s = which ? a.drot_s[1] : a.drot_s[0];
  const float *dshape_l = which ? a.dshape_l[1] : a.dshape_l[0], *dbetas_s = which ? a.dbetas_s[1] : a.dbetas_s[0];
  const float* dcam_l = which ? a.dcam_l[1] : a.dcam_l[0];
  float *d_rot = which ? a.d_rot[1] : a.d_rot[0], *d_state = which ? a.d_state[1] : a.d_state[0];
  for (int i = blockIdx.x * 256 + threadIdx.x; i < a.B * per; i += gridDim.x * 256) {
    const int b = i / per, j = i % per;
    if (j < 216) {
      const int o = b * 216 + j;
      d_rot[o] = 1.f * drot_l[o] + drot_s[o] + 0.f;
    } else if (j < 226) {
      const int c = j - 216;
      d_state[(size_t)b * a.ldd + 144 + c] = 1.f * dshape_l[b * 10 + c] + dbetas_s[b * 10 + c] + 0.f;
    } else if (j < 229) {
      const int c = j - 226;
      d_state[(size_t)b * a.ldd + 154 + c] = 1.f * dcam_l[b * 3 + c] + 0.f;
    } else {
      d_state[(size_t)b * a.ldd + 157 + (j - 229)] = 0.f;
    }
  }
}

namespace {
struct HeadHvpWs {
  float *rot[2], *verts[2], *joints[2], *saved[2], *drot_l[2], *dshape_l[2], *dcam_l[2], *djoints_l[2], *drot_s[2], *dbetas_s[2],
      *d_rot[2];
  float *loss_parts, *losses;
  void* lbs_ws;
  size_t lbs_ws_bytes, total_bytes;
};
// every block starts on a 16-byte boundary
HeadHvpWs head_hvp_carve(char* base, int B) {
  HeadHvpWs w;
  size_t off = 0;
  auto take = [&](size_t floats) {
    float* p = reinterpret_cast<float*>(base + off);
    off += ((floats * sizeof(float) + 15) / 16) * 16;
    return p;
  };
  const size_t nb = (size_t)B;
  for (int k = 0; k < 2; ++k) {
    w.rot[k] = take(nb * 216);
    w.verts[k] = take(nb * HH_NV * 3);
    w.joints[k] = take(nb * 49 * 3);
    w.saved[k] = take(dyb_lbs_saved_floats(B));
    w.drot_l[k] = take(nb * 216);
    w.dshape_l[k] = take(nb * 10);
    w.dcam_l[k] = take(nb * 3);
    w.djoints_l[k] = take(nb * 49 * 3);
    w.drot_s[k] = take(nb * 216);
    w.dbetas_s[k] = take(nb * 10);
    w.d_rot[k] = take(nb * 216);
  }
  w.loss_parts = take(nb * 4);
  w.losses = take(4);
  w.lbs_ws_bytes = 2 * dyb_lbs_bwd_workspace_bytes(B);
  w.lbs_ws = take(w.lbs_ws_bytes / sizeof(float));
  w.total_bytes = off;
  return w;
}
}  // namespace

extern "C" size_t dyb_head_hvp_workspace_bytes(int B) { return B > 0 ? head_hvp_carve(nullptr, B).total_bytes : 0; }

extern "C" int dyb_head_hvp(const float* const* tables_f, const int* const* tables_i, const float* state, const float* tstate, int ld,
                            const float* kp2d, const float* gmm_means, const float* gmm_prec, const float* gmm_logw, float w2d,
                            float wshape, float wpose, float* losses4, float* d_state, float* td_state, int ldd, int B, void* ws,
                            size_t ws_bytes, hipStream_t st) {
  DYB_REQUIRE(tables_f && tables_i && state && tstate && kp2d && gmm_means && gmm_prec && gmm_logw, DYB_ERR_ARG);
  DYB_REQUIRE(d_state && td_state && ws && B > 0 && ld >= HH_STATE && ldd >= HH_STATE, DYB_ERR_ARG);
  DYB_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 15) == 0, DYB_ERR_ARG);
  DYB_REQUIRE(ws_bytes >= dyb_head_hvp_workspace_bytes(B), DYB_ERR_WORKSPACE);
  DYB_REQUIRE(dyb_rep_current().n == 1, DYB_ERR_UNSUPPORTED);
  const HeadHvpWs w = head_hvp_carve(reinterpret_cast<char*>(ws), B);
  const float *shape = state + 144, *tshape = tstate + 144, *cam = state + 154, *tcam = tstate + 154;
  int rc;
  if ((rc = dyb_rot6d_jvp(state, tstate, ld, w.rot[0], w.rot[1], B, st)) != DYB_OK) return rc;
  if ((rc = dyb_lbs_jvp(tables_f, tables_i, shape, tshape, ld, w.rot[0], w.rot[1], w.verts[0], w.verts[1], w.joints[0], w.joints[1],
                        w.saved[0], w.saved[1], B, st)) != DYB_OK)
    return rc;
  if ((rc = dyb_frame_losses_jvp(w.rot[0], w.rot[1], shape, tshape, ld, cam, tcam, ld, w.joints[0], w.joints[1], kp2d, gmm_means, gmm_prec,
                                 gmm_logw, w2d, wshape, wpose, w.losses, w.drot_l[0], w.drot_l[1], w.dshape_l[0],
                                 w.dshape_l[1], 10, w.dcam_l[0], w.dcam_l[1], 3, w.djoints_l[0], w.djoints_l[1], B, w.loss_parts,
                                 (size_t)B * 4 * sizeof(float), st)) != DYB_OK)
    return rc;
  if ((rc = dyb_lbs_bwd_jvp(tables_f, tables_i, w.rot[0], w.rot[1], w.saved[0], w.saved[1], w.djoints_l[0], w.djoints_l[1], w.drot_s[0],
                            w.drot_s[1], w.dbetas_s[0], w.dbetas_s[1], 10, B, w.lbs_ws, w.lbs_ws_bytes, st)) != DYB_OK)
    return rc;
  HeadHvpCombineArgs a;
  for (int k = 0; k < 2; ++k) {
    a.drot_l[k] = w.drot_l[k]; a.drot_s[k] = w.drot_s[k]; a.dshape_l[k] = w.dshape_l[k]; a.dbetas_s[k] = w.dbetas_s[k];
    a.dcam_l[k] = w.dcam_l[k]; a.d_rot[k] = w.d_rot[k];
  }
  a.d_state[0] = d_state; a.d_state[1] = td_state;
  a.B = B; a.ldd = ldd;
  hipLaunchKernelGGL(head_hvp_combine_kernel, dim3(dyb_cdiv(B * (216 + ldd - 144), 256), 2), dim3(256), 0, st, a);
  DYB_CHECK_LAUNCH();
  if ((rc = dyb_rot6d_bwd_jvp(state, tstate, ld, w.d_rot[0], w.d_rot[1], d_state, td_state, ldd, B, st)) != DYB_OK) return rc;
  // the value-only pass: the float kernels' own gradient over the value half (see the head of this file)
  if ((rc = dyb_rot6d_fwd(state, ld, w.rot[0], B, st)) != DYB_OK) return rc;
  if ((rc = dyb_lbs_fwd(tables_f, tables_i, shape, ld, w.rot[0], w.verts[0], w.joints[0], w.saved[0], B, st)) != DYB_OK) return rc;
  if ((rc = dyb_frame_losses(w.rot[0], shape, ld, cam, ld, w.joints[0], kp2d, gmm_means, gmm_prec, gmm_logw, w2d, wshape, wpose,
                             losses4 ? losses4 : w.losses, w.drot_l[0], w.dshape_l[0], 10, w.dcam_l[0], 3, w.djoints_l[0], B, w.loss_parts,
                             (size_t)B * 4 * sizeof(float), st)) != DYB_OK)
    return rc;
  if ((rc = dyb_lbs_bwd(tables_f, tables_i, w.rot[0], w.saved[0], w.djoints_l[0], nullptr, w.drot_s[0], w.dbetas_s[0], 10, B, w.lbs_ws,
                        w.lbs_ws_bytes, st)) != DYB_OK)
    return rc;
  hipLaunchKernelGGL(head_hvp_combine_kernel, dim3(dyb_cdiv(B * (216 + ldd - 144), 256), 1), dim3(256), 0, st, a);
  DYB_CHECK_LAUNCH();
  return dyb_rot6d_bwd(state, ld, w.d_rot[0], d_state, ldd, B, st);
}
