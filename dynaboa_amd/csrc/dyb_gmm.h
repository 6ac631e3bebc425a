// MaxMixturePrior.merged_log_likelihood (utils/smplify/prior.py:181-196) on one axis-angle body pose, evaluated by one workgroup:
// ONE definition for dyb_gmm_prior (losses.hip) and the SMPLify body loss (smplify.hip) - the two must select the same component
// and round alike.  (The frame-loss head of losses.hip keeps its own copy: it is templated over dual numbers.)
#pragma once
#include "dyb_common.h"

#define DYB_GMM_NG 8
#define DYB_GMM_ND 69

struct DybGmmShared {
  float D[DYB_GMM_NG][DYB_GMM_ND], Row[DYB_GMM_NG][DYB_GMM_ND], Col[DYB_GMM_NG][DYB_GMM_ND], Q[DYB_GMM_NG];
  int best;
};
// Called by all NT work-items of the workgroup (t = threadIdx.x), S in shared memory.  On return (after its last barrier) S.best is
// the component with the smallest 0.5 d^T P d - log w (the first of equals), S.Q[S.best] that value and dyb_gmm_grad(S, k) its gradient.
template <int NT>
__device__ __forceinline__ void dyb_gmm_eval(const float* __restrict__ pose69, const float* __restrict__ means,
                                             const float* __restrict__ prec, const float* __restrict__ logw, DybGmmShared& S, int t) {
  constexpr int NG = DYB_GMM_NG, ND = DYB_GMM_ND;
  for (int i = t; i < NG * ND; i += NT) S.D[i / ND][i % ND] = pose69[i % ND] - means[i];
  __syncthreads();
  for (int i = t; i < NG * ND; i += NT) {
    const int m = i / ND, k = i % ND;
    const float* P = prec + (size_t)m * ND * ND;
    float r = 0.f, c = 0.f;
    for (int j = 0; j < ND; ++j) {
      const float d = S.D[m][j];
      r += P[k * ND + j] * d;
      c += P[j * ND + k] * d;
    }
    S.Row[m][k] = r;
    S.Col[m][k] = c;
  }
  __syncthreads();
  if (t < NG) {
    float q = 0.f;
    for (int k = 0; k < ND; ++k) q += S.Row[t][k] * S.D[t][k];
    S.Q[t] = 0.5f * q - logw[t];
  }
  __syncthreads();
  if (t == 0) {
    int best = 0;
    for (int m = 1; m < NG; ++m)
      if (S.Q[m] < S.Q[best]) best = m;
    S.best = best;
  }
  __syncthreads();
}
__device__ __forceinline__ float dyb_gmm_grad(const DybGmmShared& S, int k) { return 0.5f * (S.Row[S.best][k] + S.Col[S.best][k]); }
