// Temporal smoothing of a predicted pose sequence (dynaboa_amd/smooth.py).  The reference has no smoother: this is the project's own
// procedure, pinned to the rules of include/dynaboa_hip.h and to their fp64 NumPy restatement in tests/smooth_cases.py.
//
// smooth_window_kernel   the offline, non-causal form.  One thread per (frame, group): groups 0 .. J - 1 are the joints, group J the
//                        betas and camera channels of the frame.  A thread finds how far its frame's run reaches inside the window
//                        (links as seq_frame_kernel of seq_metrics.hip counts its triples: one sequence, both frames valid,
//                        consecutive frame ids), then walks the taps in ascending order: a joint's rotation becomes a quaternion,
//                        takes the centre's hemisphere and enters a weighted sum that is normalised at the end - the weighted chordal
//                        mean; a channel enters a plain weighted mean.  Every tap is converted again by every centre that reads it
//                        (2 h + 1 times): at 35 000 frames x 24 joints that is a few MFLOP on data that stays in L2, and it keeps the
//                        order of operations a function of the frame's place in its run alone - no LDS tile, no atomics, equal bytes
//                        from two calls and wherever the sequence lies in the batch.
// one_euro_kernel        the live, causal form: one workgroup per sequence, a thread per group (joint quaternion, beta, camera
//                        scalar).  `started` is read by every thread before the barrier and written by thread 0 after it.
#include <math.h>

#include "dyb_common.h"
#include "dyb_quat.h"

#define SM_MAX_HALF 32             // DYB_SMOOTH_MAX_HALF_WINDOW of include/dynaboa_hip.h
#define SM_TAPS (2 * SM_MAX_HALF + 1)
#define SM_MIN_NORM2 1e-12f

struct SmWeights {
  float w[SM_TAPS];                // w[k + h], k = -h .. h
};

__device__ __forceinline__ bool sm_finite(float v) { return fabsf(v) <= 3.4028235e38f; }      // false for NaN and the infinities
__device__ __forceinline__ bool sm_finite4(const float* q) { return sm_finite(q[0]) && sm_finite(q[1]) && sm_finite(q[2]) && sm_finite(q[3]); }

// unit quaternion (w, x, y, z) -> rotation matrix, the standard formula
__device__ __forceinline__ void sm_quat_to_rot(const float* q, float* R) {
  const float w = q[0], x = q[1], y = q[2], z = q[3];
  R[0] = 1.f - 2.f * (y * y + z * z); R[1] = 2.f * (x * y - w * z);       R[2] = 2.f * (x * z + w * y);
  R[3] = 2.f * (x * y + w * z);       R[4] = 1.f - 2.f * (x * x + z * z); R[5] = 2.f * (y * z - w * x);
  R[6] = 2.f * (x * z - w * y);       R[7] = 2.f * (y * z + w * x);       R[8] = 1.f - 2.f * (x * x + y * y);
}

__device__ __forceinline__ void sm_copy_words(const float* src, float* dst, int n) {
  const unsigned* s = reinterpret_cast<const unsigned*>(src);
  unsigned* d = reinterpret_cast<unsigned*>(dst);
  for (int c = 0; c < n; ++c) d[c] = s[c];
}

// frames a and a + 1 are linked (first <= a, a + 1 < end: the sequence of both)
__device__ __forceinline__ bool sm_linked(int a, const unsigned char* valid, const int* frame_id) {
  if (valid && !(valid[a] && valid[a + 1])) return false;
  if (frame_id && frame_id[a + 1] != frame_id[a] + 1) return false;
  return true;
}

__global__ __launch_bounds__(256) void smooth_window_kernel(const float* __restrict__ rotmat, const float* __restrict__ betas, int nb,
                                                            const float* __restrict__ cam, int nc, const int* __restrict__ seq_offsets,
                                                            int n_seq, const unsigned char* __restrict__ valid,
                                                            const int* __restrict__ frame_id, SmWeights W, int h,
                                                            float* __restrict__ rotmat_out, float* __restrict__ betas_out,
                                                            float* __restrict__ cam_out, int n, int J) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  const int G = J + 1;
  if (e >= (long long)n * G) return;
  const int i = (int)(e / G), g = (int)(e - (long long)i * G);

  // the taps of frame i: i - back .. i + fwd, the part of its run inside the window
  int back = 0, fwd = 0;
  if (h > 0 && (!valid || valid[i])) {
    int lo = 0, hi = n_seq;                                          // the sequence of frame i, as seq_frame_kernel finds it
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (seq_offsets[mid] <= i) lo = mid; else hi = mid;
    }
    int first = seq_offsets[lo], end = seq_offsets[lo + 1];
    first = first < 0 ? 0 : first;
    end = end > n ? n : end;
    while (back < h && i - back - 1 >= first && sm_linked(i - back - 1, valid, frame_id)) ++back;
    while (fwd < h && i + fwd + 1 < end && sm_linked(i + fwd, valid, frame_id)) ++fwd;
  }
  const bool copy = back + fwd == 0;                                 // h = 0, an invalid frame, a run of one frame

  if (g < J) {
    const float* Rc = rotmat + ((size_t)i * J + g) * 9;
    float* Ro = rotmat_out + ((size_t)i * J + g) * 9;
    if (copy) { sm_copy_words(Rc, Ro, 9); return; }
    const QuatFwd qc = rot_to_quat(Rc);
    if (!sm_finite4(qc.q)) { sm_copy_words(Rc, Ro, 9); return; }
    float s[4] = {0.f, 0.f, 0.f, 0.f};
    for (int k = -back; k <= fwd; ++k) {
      const QuatFwd qk = rot_to_quat(Rc + (long long)k * J * 9);
      if (!sm_finite4(qk.q)) continue;
      const float d = qk.q[0] * qc.q[0] + qk.q[1] * qc.q[1] + qk.q[2] * qc.q[2] + qk.q[3] * qc.q[3];
      const float w = d < 0.f ? -W.w[k + h] : W.w[k + h];
      for (int c = 0; c < 4; ++c) s[c] += w * qk.q[c];
    }
    const float n2 = s[0] * s[0] + s[1] * s[1] + s[2] * s[2] + s[3] * s[3];
    if (!(n2 >= SM_MIN_NORM2)) { sm_copy_words(Rc, Ro, 9); return; }
    const float inv = 1.f / sqrtf(n2);
    float q[4], R[9];
    for (int c = 0; c < 4; ++c) q[c] = s[c] * inv;
    sm_quat_to_rot(q, R);
    for (int c = 0; c < 9; ++c) Ro[c] = R[c];
    return;
  }

  // group J: the plain weighted mean of every betas and camera channel
  for (int part = 0; part < 2; ++part) {
    const float* src = part == 0 ? betas : cam;
    float* dst = part == 0 ? betas_out : cam_out;
    const int nch = part == 0 ? nb : nc;
    if (!src || nch <= 0) continue;
    const float* xc = src + (size_t)i * nch;
    float* xo = dst + (size_t)i * nch;
    if (copy) { sm_copy_words(xc, xo, nch); continue; }
    float wsum = 0.f;
    for (int k = -back; k <= fwd; ++k) wsum += W.w[k + h];
    for (int c = 0; c < nch; ++c) {
      float acc = 0.f;
      for (int k = -back; k <= fwd; ++k) acc += W.w[k + h] * xc[(long long)k * nch + c];
      xo[c] = acc / wsum;
    }
  }
}

static bool sm_overlap(const void* a, size_t na, const void* b, size_t nb) {
  const char *pa = static_cast<const char*>(a), *pb = static_cast<const char*>(b);
  return a && b && pa < pb + nb && pb < pa + na;
}

extern "C" int dyb_smooth_sequences(const float* rotmat, const float* betas, int nb, const float* cam, int nc, const int* seq_offsets,
                                    int n_seq, const unsigned char* valid, const int* frame_id, const float* weights_host,
                                    int half_window, float* rotmat_out, float* betas_out, float* cam_out, int n, int J, hipStream_t st) {
  DYB_REQUIRE(J >= 1 && n >= 0 && n_seq >= 1 && nb >= 0 && nc >= 0, DYB_ERR_ARG);
  DYB_REQUIRE(half_window >= 0 && half_window <= SM_MAX_HALF, DYB_ERR_ARG);
  DYB_REQUIRE(n == 0 || (rotmat && rotmat_out && seq_offsets && weights_host), DYB_ERR_ARG);
  DYB_REQUIRE((!betas || betas_out) && (!cam || cam_out), DYB_ERR_ARG);
  const size_t rot_bytes = (size_t)n * J * 9 * sizeof(float), b_bytes = (size_t)n * nb * sizeof(float),
               c_bytes = (size_t)n * nc * sizeof(float);
  DYB_REQUIRE(!sm_overlap(rotmat, rot_bytes, rotmat_out, rot_bytes), DYB_ERR_ARG);
  DYB_REQUIRE(!sm_overlap(betas, b_bytes, betas_out, b_bytes) && !sm_overlap(cam, c_bytes, cam_out, c_bytes), DYB_ERR_ARG);
  SmWeights W;
  for (int k = 0; k < SM_TAPS; ++k) W.w[k] = 0.f;
  if (weights_host) {
    for (int k = 0; k <= 2 * half_window; ++k) {
      const float w = weights_host[k];
      DYB_REQUIRE(std::isfinite(w) && w >= 0.f, DYB_ERR_ARG);
      W.w[k] = w;
    }
    DYB_REQUIRE(W.w[half_window] > 0.f, DYB_ERR_ARG);
  }
  if (n == 0) return DYB_OK;
  const long long blocks = ((long long)n * (J + 1) + 255) / 256;
  DYB_REQUIRE(blocks <= 0x7fffffffLL, DYB_ERR_UNSUPPORTED);
  hipLaunchKernelGGL(smooth_window_kernel, dim3((unsigned)blocks), dim3(256), 0, st, rotmat, betas, nb, cam, nc, seq_offsets, n_seq, valid,
                     frame_id, W, half_window, rotmat_out, betas_out, cam_out, n, J);
  DYB_CHECK_LAUNCH();
  return DYB_OK;
}

// ---- One-Euro filter (Casiez, Roussel, Vogel 2012) over quaternions and scalars ---------------------------------------------------
__device__ __forceinline__ float oe_alpha(float cutoff, float te) {
  const float tau = 1.f / (6.2831853071795864769f * cutoff);
  return 1.f / (1.f + tau / te);
}

// one group of D components: x the new sample (already in x-hat's hemisphere), xh / dxh the state; -> xh updated (not normalised)
template <int D>
__device__ __forceinline__ void oe_group(const float* x, float* xh, float* dxh, float te, float min_cutoff, float beta, float a_d) {
  float n2 = 0.f;
  for (int c = 0; c < D; ++c) {
    const float dx = (x[c] - xh[c]) / te;
    dxh[c] = a_d * dx + (1.f - a_d) * dxh[c];
    n2 += dxh[c] * dxh[c];
  }
  const float a = oe_alpha(min_cutoff + beta * sqrtf(n2), te);
  for (int c = 0; c < D; ++c) xh[c] = a * x[c] + (1.f - a) * xh[c];
}

__global__ __launch_bounds__(64) void one_euro_kernel(float* __restrict__ state, const float* __restrict__ rotmat,
                                                      const float* __restrict__ betas, int nb, const float* __restrict__ cam, int nc,
                                                      const unsigned char* __restrict__ active, float te, float min_cutoff, float beta,
                                                      float d_cutoff, float* __restrict__ rotmat_out, float* __restrict__ betas_out,
                                                      float* __restrict__ cam_out, int J) {
  const int r = blockIdx.x;
  if (active && !active[r]) return;                                  // the whole workgroup leaves: no barrier is left waiting
  const int X = 4 * J + nb + nc;
  float* row = state + (size_t)r * (1 + 2 * X);
  float *xh = row + 1, *dxh = row + 1 + X;
  const bool started = row[0] != 0.f;
  __syncthreads();
  if (threadIdx.x == 0) row[0] = 1.f;
  const float a_d = oe_alpha(d_cutoff, te);
  for (int g = threadIdx.x; g < J + nb + nc; g += 64) {
    if (g < J) {
      const float* Rin = rotmat + ((size_t)r * J + g) * 9;
      float* Ro = rotmat_out + ((size_t)r * J + g) * 9;
      const QuatFwd qf = rot_to_quat(Rin);
      float* qh = xh + 4 * g;
      float* dqh = dxh + 4 * g;
      if (!started) {
        for (int c = 0; c < 4; ++c) { qh[c] = qf.q[c]; dqh[c] = 0.f; }
        sm_copy_words(Rin, Ro, 9);
        continue;
      }
      float x[4], q[4], R[9];
      for (int c = 0; c < 4; ++c) q[c] = qh[c];
      const float d = qf.q[0] * q[0] + qf.q[1] * q[1] + qf.q[2] * q[2] + qf.q[3] * q[3];
      for (int c = 0; c < 4; ++c) x[c] = d < 0.f ? -qf.q[c] : qf.q[c];
      oe_group<4>(x, q, dqh, te, min_cutoff, beta, a_d);
      const float inv = 1.f / sqrtf(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
      for (int c = 0; c < 4; ++c) { q[c] *= inv; qh[c] = q[c]; }
      sm_quat_to_rot(q, R);
      for (int c = 0; c < 9; ++c) Ro[c] = R[c];
    } else {
      const int c = g - J;                                           // betas first, then the camera
      const float* src = c < nb ? betas + (size_t)r * nb + c : cam + (size_t)r * nc + (c - nb);
      float* dst = c < nb ? betas_out + (size_t)r * nb + c : cam_out + (size_t)r * nc + (c - nb);
      float* sh = xh + 4 * J + c;
      float* dsh = dxh + 4 * J + c;
      if (!started) {
        *sh = *src; *dsh = 0.f;
        sm_copy_words(src, dst, 1);
        continue;
      }
      const float x = *src;
      float v = *sh;
      oe_group<1>(&x, &v, dsh, te, min_cutoff, beta, a_d);
      *sh = v;
      *dst = v;
    }
  }
}

extern "C" int dyb_one_euro_state_floats(int J, int nb, int nc) {
  if (J < 1 || nb < 0 || nc < 0) return DYB_ERR_ARG;
  return 1 + 2 * (4 * J + nb + nc);
}

extern "C" int dyb_one_euro_step(float* state, const float* rotmat, const float* betas, int nb, const float* cam, int nc,
                                 const unsigned char* active, float te, float min_cutoff, float beta, float d_cutoff, float* rotmat_out,
                                 float* betas_out, float* cam_out, int R, int J, hipStream_t st) {
  DYB_REQUIRE(J >= 1 && R >= 0 && nb >= 0 && nc >= 0, DYB_ERR_ARG);
  DYB_REQUIRE(te > 0.f && min_cutoff > 0.f && d_cutoff > 0.f && std::isfinite(te) && std::isfinite(min_cutoff) && std::isfinite(d_cutoff) &&
                  std::isfinite(beta) && beta >= 0.f, DYB_ERR_ARG);
  DYB_REQUIRE(R == 0 || (state && rotmat && rotmat_out), DYB_ERR_ARG);
  DYB_REQUIRE((nb == 0 || (betas && betas_out)) && (nc == 0 || (cam && cam_out)), DYB_ERR_ARG);
  const size_t rot_bytes = (size_t)R * J * 9 * sizeof(float), b_bytes = (size_t)R * nb * sizeof(float),
               c_bytes = (size_t)R * nc * sizeof(float);
  DYB_REQUIRE(!sm_overlap(rotmat, rot_bytes, rotmat_out, rot_bytes), DYB_ERR_ARG);
  DYB_REQUIRE(!sm_overlap(betas, b_bytes, betas_out, b_bytes) && !sm_overlap(cam, c_bytes, cam_out, c_bytes), DYB_ERR_ARG);
  if (R == 0) return DYB_OK;
  hipLaunchKernelGGL(one_euro_kernel, dim3(R), dim3(64), 0, st, state, rotmat, betas, nb, cam, nc, active, te, min_cutoff, beta, d_cutoff,
                     rotmat_out, betas_out, cam_out, J);
  DYB_CHECK_LAUNCH();
  return DYB_OK;
}
