// (value, tangent) pairs for the closed-form second derivative of the frame-loss head (--hvp_head closed).
//
// The head's gradient kernels (smpl_lbs.hip, losses.hip) are templates on a scalar type S.  S = float is the code the library has
// always run: every helper below is the identity on it, so that instantiation is the same arithmetic in the same order.  S = dualf
// carries the directional derivative along the state tangent next to the value: the value half repeats the float arithmetic, the
// tangent half is the product / quotient rule of each operation, so one pass over the tables (the 17.1 MB posedirs sweep above all)
// yields the gradient AND its tangent.  Values and tangents live in separate float arrays (value array laid out exactly as before,
// tangent array of the same shape); DybIO pairs them at the loads and stores.  Table entries (SMPL, GMM prior, key points) stay float.
#pragma once
#include "dyb_common.h"

template <class F>
struct DybDual {
  F v, t;
};
typedef DybDual<float> dualf;
typedef DybDual<double> duald;

#define DD __host__ __device__ __forceinline__
template <class F> DD DybDual<F> dyb_mk(F v, F t) { DybDual<F> r; r.v = v; r.t = t; return r; }
template <class F> DD DybDual<F> operator+(DybDual<F> a, DybDual<F> b) { return dyb_mk<F>(a.v + b.v, a.t + b.t); }
template <class F> DD DybDual<F> operator-(DybDual<F> a, DybDual<F> b) { return dyb_mk<F>(a.v - b.v, a.t - b.t); }
template <class F> DD DybDual<F> operator*(DybDual<F> a, DybDual<F> b) { return dyb_mk<F>(a.v * b.v, a.v * b.t + a.t * b.v); }
template <class F> DD DybDual<F> operator/(DybDual<F> a, DybDual<F> b) {
  const F q = a.v / b.v;
  return dyb_mk<F>(q, (a.t - q * b.t) / b.v);
}
template <class F> DD DybDual<F> operator-(DybDual<F> a) { return dyb_mk<F>(-a.v, -a.t); }
template <class F> DD DybDual<F> operator+(DybDual<F> a, F c) { return dyb_mk<F>(a.v + c, a.t); }
template <class F> DD DybDual<F> operator+(F c, DybDual<F> a) { return dyb_mk<F>(c + a.v, a.t); }
template <class F> DD DybDual<F> operator-(DybDual<F> a, F c) { return dyb_mk<F>(a.v - c, a.t); }
template <class F> DD DybDual<F> operator-(F c, DybDual<F> a) { return dyb_mk<F>(c - a.v, -a.t); }
template <class F> DD DybDual<F> operator*(DybDual<F> a, F c) { return dyb_mk<F>(a.v * c, a.t * c); }
template <class F> DD DybDual<F> operator*(F c, DybDual<F> a) { return dyb_mk<F>(c * a.v, c * a.t); }
template <class F> DD DybDual<F> operator/(DybDual<F> a, F c) { return dyb_mk<F>(a.v / c, a.t / c); }
template <class F> DD DybDual<F> operator/(F c, DybDual<F> a) {
  const F q = c / a.v;
  return dyb_mk<F>(q, -q * a.t / a.v);
}
template <class F> DD DybDual<F>& operator+=(DybDual<F>& a, DybDual<F> b) { a = a + b; return a; }
template <class F> DD DybDual<F>& operator-=(DybDual<F>& a, DybDual<F> b) { a = a - b; return a; }
template <class F> DD DybDual<F>& operator*=(DybDual<F>& a, F c) { a = a * c; return a; }

// value of a scalar, a literal as a scalar
DD float dyb_val(float x) { return x; }
DD float dyb_val(dualf x) { return x.v; }
template <class S> DD S dyb_lit(float c);
template <> DD float dyb_lit<float>(float c) { return c; }
template <> DD dualf dyb_lit<dualf>(float c) { return dyb_mk<float>(c, 0.f); }

// sqrt; max against a constant floor (tangent of the argument where the floor is inactive, zero where it is active)
// (dyb_sqrt of an exact 0 hands on a tangent of 0/0 or t/0; the only callers clamp the root with dyb_maxc, whose active branch
// replaces the whole pair by (c, 0) and so never looks at it - keep the two together)
DD float dyb_sqrt(float x) { return sqrtf(x); }
DD dualf dyb_sqrt(dualf x) { const float s = sqrtf(x.v); return dyb_mk<float>(s, x.t / (2.f * s)); }
DD duald dyb_sqrt(duald x) { const double s = sqrt(x.v); return dyb_mk<double>(s, x.t / (2.0 * s)); }
DD float dyb_maxc(float x, float c) { return fmaxf(x, c); }
DD dualf dyb_maxc(dualf x, float c) { return x.v > c ? x : dyb_mk<float>(c, 0.f); }

template <class S> struct DybIO;
template <> struct DybIO<float> {
  static constexpr bool dual = false;
  static DD float ld(const float* p, const float*, size_t i) { return p[i]; }
  static DD void st(float* p, float*, size_t i, float x) { p[i] = x; }
};
template <> struct DybIO<dualf> {
  static constexpr bool dual = true;
  static DD dualf ld(const float* p, const float* tp, size_t i) { return dyb_mk<float>(p[i], tp[i]); }
  static DD void st(float* p, float* tp, size_t i, dualf x) { p[i] = x.v; tp[i] = x.t; }
};
#undef DD

// wave-wide exchange and butterfly sum of a scalar
__device__ __forceinline__ float dyb_shx(float v, int m) { return __shfl_xor(v, m); }
__device__ __forceinline__ dualf dyb_shx(dualf v, int m) { return dyb_mk<float>(__shfl_xor(v.v, m), __shfl_xor(v.t, m)); }
__device__ __forceinline__ dualf dyb_wave_sum(dualf v) { return dyb_mk<float>(dyb_wave_sum(v.v), dyb_wave_sum(v.t)); }
