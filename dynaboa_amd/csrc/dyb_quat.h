// rotation matrix -> quaternion -> axis-angle as the reference's rotation_matrix_to_angle_axis does it (utils/geometry.py:184-306,
// kornia-derived 4-branch quaternion formula, NaN -> 0).  Shared by the loss head (losses.hip) and the 3DPW extraction
// (pw3d_extract.hip).
#pragma once
#include "dyb_common.h"

struct QuatFwd {
  int branch;
  float t;        // selected trace term
  float u[4];     // un-normalised quaternion (one component equals t)
  float q[4];     // 0.5*u/sqrt(t)
};
__device__ __forceinline__ QuatFwd rot_to_quat(const float* R) {
  const float eps = 1e-6f;
  float r00 = R[0], r01 = R[1], r02 = R[2], r10 = R[3], r11 = R[4], r12 = R[5], r20 = R[6], r21 = R[7], r22 = R[8];
  bool d2 = r22 < eps, d01 = r00 > r11, d0n1 = r00 < -r11;
  QuatFwd f;
  if (d2 && d01) {
    f.branch = 0; f.t = 1.f + r00 - r11 - r22;
    f.u[0] = r21 - r12; f.u[1] = f.t; f.u[2] = r10 + r01; f.u[3] = r02 + r20;
  } else if (d2) {
    f.branch = 1; f.t = 1.f - r00 + r11 - r22;
    f.u[0] = r02 - r20; f.u[1] = r10 + r01; f.u[2] = f.t; f.u[3] = r21 + r12;
  } else if (d0n1) {
    f.branch = 2; f.t = 1.f - r00 - r11 + r22;
    f.u[0] = r10 - r01; f.u[1] = r02 + r20; f.u[2] = r21 + r12; f.u[3] = f.t;
  } else {
    f.branch = 3; f.t = 1.f + r00 + r11 + r22;
    f.u[0] = f.t; f.u[1] = r21 - r12; f.u[2] = r02 - r20; f.u[3] = r10 - r01;
  }
  float k = 0.5f / sqrtf(f.t);
  for (int i = 0; i < 4; ++i) f.q[i] = f.u[i] * k;
  return f;
}
__device__ __forceinline__ void quat_to_aa(const float* q, float* aa) {
  float w = q[0];
  float s2 = q[1] * q[1] + q[2] * q[2] + q[3] * q[3];
  float s = sqrtf(s2);
  float tt = 2.f * (w < 0.f ? atan2f(-s, -w) : atan2f(s, w));
  float k = s2 > 0.f ? tt / s : 2.f;
  for (int i = 0; i < 3; ++i) {
    float v = q[1 + i] * k;
    aa[i] = (v != v) ? 0.f : v;
  }
}
