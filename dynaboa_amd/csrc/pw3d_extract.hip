// 3DPW extraction (dynaboa_amd/pw3d_extract.py): the per-frame annotations the reference's utils/data_preprocess/pw3d.py derives
// from a sequence file, for n person-frames in one launch.  Restated from what that file's NumPy does:
//   projection (:24-30)   p = (float)((double)joint + trans): the in-place += on the float32 joints rounds ONCE to fp32; from there
//                         on fp64: q = cam_pose[:3, :] . (p, 1), q /= q.z, uv = (K . q).xy, confidence 1.  No special case for
//                         q.z <= 0 (the reference has none; IEEE division decides).
//   get_bbox (:48-53)     min / max of u and v over the 49 joints, centre = midpoint, scale = max(width, height) / 200.
//   root alignment (:128-133), fp32: R = batch_rodrigues(root) through the unit quaternion (utils/geometry.py:9-45, NOT smplx's
//                         Rodrigues), Rs = fp32(cam_pose[:3, :3]) . R, root_aligned = rotation_matrix_to_angle_axis(Rs) (dyb_quat.h).
// One wave per frame, PW_WAVES frames per workgroup: lanes 0..48 take one joint each, lanes 49..63 repeat joint 48 (their loads stay
// in bounds and a repeated value cannot move an extremum; they store nothing), the four extrema are 64-lane butterflies on doubles
// (fmin / fmax: a NaN coordinate is skipped, where Python's min / max would depend on its position), lane 0 does the alignment.
// The kernel is a few hundred bytes per frame and bound by its launch; nothing here is tuned beyond a grid that covers n.
#include <math.h>

#include "dyb_common.h"
#include "dyb_quat.h"

#define PW_WAVES 4                 // frames per workgroup
#define PW_NJ 49

__device__ __forceinline__ double pw_wave_min(double v) {
  for (int m = 32; m >= 1; m >>= 1) v = fmin(v, __shfl_xor(v, m));
  return v;
}
__device__ __forceinline__ double pw_wave_max(double v) {
  for (int m = 32; m >= 1; m >>= 1) v = fmax(v, __shfl_xor(v, m));
  return v;
}

// utils/geometry.py:9-45 in fp32: axis-angle -> unit quaternion (1e-8 added before the norm) -> rotation matrix
__device__ __forceinline__ void pw_rodrigues_quat(const float* aa, float* R) {
  const float e0 = aa[0] + 1e-8f, e1 = aa[1] + 1e-8f, e2 = aa[2] + 1e-8f;
  const float angle = sqrtf(e0 * e0 + e1 * e1 + e2 * e2);
  const float half = angle * 0.5f, c = cosf(half), s = sinf(half);
  const float q0 = c, q1 = s * (aa[0] / angle), q2 = s * (aa[1] / angle), q3 = s * (aa[2] / angle);
  const float qn = sqrtf(q0 * q0 + q1 * q1 + q2 * q2 + q3 * q3);
  const float w = q0 / qn, x = q1 / qn, y = q2 / qn, z = q3 / qn;
  const float w2 = w * w, x2 = x * x, y2 = y * y, z2 = z * z;
  const float wx = w * x, wy = w * y, wz = w * z, xy = x * y, xz = x * z, yz = y * z;
  R[0] = w2 + x2 - y2 - z2; R[1] = 2.f * xy - 2.f * wz;   R[2] = 2.f * wy + 2.f * xz;
  R[3] = 2.f * wz + 2.f * xy; R[4] = w2 - x2 + y2 - z2;   R[5] = 2.f * yz - 2.f * wx;
  R[6] = 2.f * xz - 2.f * wy; R[7] = 2.f * wx + 2.f * yz; R[8] = w2 - x2 - y2 + z2;
}

__global__ __launch_bounds__(64 * PW_WAVES) void pw3d_annotate_kernel(const float* __restrict__ joints49, const double* __restrict__ trans,
                                                                      const double* __restrict__ cam_pose,
                                                                      const double* __restrict__ cam_intrinsics,
                                                                      const float* __restrict__ root_aa, double* __restrict__ j2d,
                                                                      double* __restrict__ center, double* __restrict__ scale,
                                                                      float* __restrict__ root_aligned, int n) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long f = (long long)blockIdx.x * PW_WAVES + wave;
  if (f >= n) return;                                       // whole waves leave together; there is no workgroup barrier below
  const int j = lane < PW_NJ ? lane : PW_NJ - 1;
  const float* jp = joints49 + ((size_t)f * PW_NJ + j) * 3;
  const double* t = trans + (size_t)f * 3;
  const double* P = cam_pose + (size_t)f * 16;
  const double* K = cam_intrinsics;

  const double p0 = (double)(float)((double)jp[0] + t[0]);
  const double p1 = (double)(float)((double)jp[1] + t[1]);
  const double p2 = (double)(float)((double)jp[2] + t[2]);
  const double qx = P[0] * p0 + P[1] * p1 + P[2] * p2 + P[3];
  const double qy = P[4] * p0 + P[5] * p1 + P[6] * p2 + P[7];
  const double qz = P[8] * p0 + P[9] * p1 + P[10] * p2 + P[11];
  const double hx = qx / qz, hy = qy / qz, hz = qz / qz;
  const double u = K[0] * hx + K[1] * hy + K[2] * hz;
  const double v = K[3] * hx + K[4] * hy + K[5] * hz;
  if (lane < PW_NJ) {
    double* o = j2d + ((size_t)f * PW_NJ + lane) * 3;
    o[0] = u; o[1] = v; o[2] = 1.0;
  }
  const double ulo = pw_wave_min(u), uhi = pw_wave_max(u), vlo = pw_wave_min(v), vhi = pw_wave_max(v);
  if (lane == 0) {
    center[(size_t)f * 2] = (uhi + ulo) / 2.0;
    center[(size_t)f * 2 + 1] = (vhi + vlo) / 2.0;
    scale[f] = fmax(uhi - ulo, vhi - vlo) / 200.0;

    float R[9], Rs[9], q_aa[3];
    pw_rodrigues_quat(root_aa + (size_t)f * 3, R);
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 3; ++c)
        Rs[3 * r + c] = (float)P[4 * r] * R[c] + (float)P[4 * r + 1] * R[3 + c] + (float)P[4 * r + 2] * R[6 + c];
    const QuatFwd q = rot_to_quat(Rs);
    quat_to_aa(q.q, q_aa);
    for (int i = 0; i < 3; ++i) root_aligned[(size_t)f * 3 + i] = q_aa[i];
  }
}

extern "C" int dyb_pw3d_annotate(const float* joints49, const double* trans, const double* cam_pose, const double* cam_intrinsics,
                                 const float* root_aa, double* j2d, double* center, double* scale, float* root_aligned, int n,
                                 hipStream_t st) {
  DYB_REQUIRE(joints49 && trans && cam_pose && cam_intrinsics && root_aa && j2d && center && scale && root_aligned && n > 0,
              DYB_ERR_ARG);
  hipLaunchKernelGGL(pw3d_annotate_kernel, dim3(dyb_cdiv(n, PW_WAVES)), dim3(64 * PW_WAVES), 0, st, joints49, trans, cam_pose,
                     cam_intrinsics, root_aa, j2d, center, scale, root_aligned, n);
  DYB_CHECK_LAUNCH();
  return DYB_OK;
}
