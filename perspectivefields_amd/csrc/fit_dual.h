// Shared pieces of the camera fits (fit_camera.hip: pinhole, fit_camera_usm.hip: Unified Spherical Model, fit_camera_fisheye.hip: fisheye
// lenses): forward-mode dual numbers, the wave-uniform mark, the Huber / L2 loss and the wave reduction.  Everything is __forceinline__ and internal to the including unit.
#pragma once

#include <math.h>

#include "pf_kernels.h"

namespace pf {

namespace {

constexpr float kRad2Deg = 57.29577951308232f;

// ---------------------------------------------------------------- forward-mode dual numbers, N derivatives
template <int N>
struct Dual {
  float v;
  float d[N];
};
template <int N>
__device__ __forceinline__ Dual<N> dconst(float v) {
  Dual<N> r;
  r.v = v;
#pragma unroll
  for (int k = 0; k < N; ++k) r.d[k] = 0.f;
  return r;
}
template <int N>
__device__ __forceinline__ Dual<N> dvar(float v, int k0) {
  Dual<N> r = dconst<N>(v);
  if (k0 < N) r.d[k0] = 1.f;
  return r;
}
template <int N>
__device__ __forceinline__ Dual<N> operator+(const Dual<N>& a, const Dual<N>& b) {
  Dual<N> r;
  r.v = a.v + b.v;
#pragma unroll
  for (int k = 0; k < N; ++k) r.d[k] = a.d[k] + b.d[k];
  return r;
}
template <int N>
__device__ __forceinline__ Dual<N> operator-(const Dual<N>& a, const Dual<N>& b) {
  Dual<N> r;
  r.v = a.v - b.v;
#pragma unroll
  for (int k = 0; k < N; ++k) r.d[k] = a.d[k] - b.d[k];
  return r;
}
template <int N>
__device__ __forceinline__ Dual<N> operator-(const Dual<N>& a) {
  Dual<N> r;
  r.v = -a.v;
#pragma unroll
  for (int k = 0; k < N; ++k) r.d[k] = -a.d[k];
  return r;
}
template <int N>
__device__ __forceinline__ Dual<N> operator*(const Dual<N>& a, const Dual<N>& b) {
  Dual<N> r;
  r.v = a.v * b.v;
#pragma unroll
  for (int k = 0; k < N; ++k) r.d[k] = fmaf(a.v, b.d[k], a.d[k] * b.v);
  return r;
}
template <int N>
__device__ __forceinline__ Dual<N> operator*(const Dual<N>& a, float s) {
  Dual<N> r;
  r.v = a.v * s;
#pragma unroll
  for (int k = 0; k < N; ++k) r.d[k] = a.d[k] * s;
  return r;
}
template <int N>
__device__ __forceinline__ Dual<N> operator+(const Dual<N>& a, float s) {
  Dual<N> r = a;
  r.v += s;
  return r;
}
// a * s + b for a float s: the per-pixel affine forms
template <int N>
__device__ __forceinline__ Dual<N> fma_s(const Dual<N>& a, float s, const Dual<N>& b) {
  Dual<N> r;
  r.v = fmaf(a.v, s, b.v);
#pragma unroll
  for (int k = 0; k < N; ++k) r.d[k] = fmaf(a.d[k], s, b.d[k]);
  return r;
}
__device__ __forceinline__ float fma_s(float a, float s, float b) { return fmaf(a, s, b); }
template <int N>
__device__ __forceinline__ Dual<N> recip(const Dual<N>& a) {
  Dual<N> r;
  r.v = 1.0f / a.v;
  const float g = -r.v * r.v;
#pragma unroll
  for (int k = 0; k < N; ++k) r.d[k] = a.d[k] * g;
  return r;
}
__device__ __forceinline__ float recip(float a) { return 1.0f / a; }
template <int N>
__device__ __forceinline__ Dual<N> dsqrt(const Dual<N>& a) {
  Dual<N> r;
  r.v = sqrtf(a.v);
  const float g = 0.5f / r.v;
#pragma unroll
  for (int k = 0; k < N; ++k) r.d[k] = a.d[k] * g;
  return r;
}
__device__ __forceinline__ float dsqrt(float a) { return sqrtf(a); }
template <int N>
__device__ __forceinline__ Dual<N> drsqrt(const Dual<N>& a) {
  Dual<N> r;
  r.v = 1.0f / sqrtf(a.v);
  const float g = -0.5f * r.v * r.v * r.v;
#pragma unroll
  for (int k = 0; k < N; ++k) r.d[k] = a.d[k] * g;
  return r;
}
__device__ __forceinline__ float drsqrt(float a) { return 1.0f / sqrtf(a); }
template <int N>
__device__ __forceinline__ Dual<N> datan2(const Dual<N>& y, const Dual<N>& x) {
  Dual<N> r;
  r.v = atan2f(y.v, x.v);
  const float q = 1.0f / (x.v * x.v + y.v * y.v);
  const float gy = x.v * q, gx = -y.v * q;
#pragma unroll
  for (int k = 0; k < N; ++k) r.d[k] = fmaf(gy, y.d[k], gx * x.d[k]);
  return r;
}
__device__ __forceinline__ float datan2(float y, float x) { return atan2f(y, x); }
template <int N>
__device__ __forceinline__ Dual<N> dasin(const Dual<N>& a) {
  Dual<N> r;
  r.v = asinf(a.v);
  const float g = 1.0f / sqrtf(1.0f - a.v * a.v);
#pragma unroll
  for (int k = 0; k < N; ++k) r.d[k] = a.d[k] * g;
  return r;
}
__device__ __forceinline__ float dasin(float a) { return asinf(a); }
template <int N>
__device__ __forceinline__ Dual<N> datan(const Dual<N>& a) {
  Dual<N> r;
  r.v = atanf(a.v);
  const float g = 1.0f / fmaf(a.v, a.v, 1.0f);
#pragma unroll
  for (int k = 0; k < N; ++k) r.d[k] = a.d[k] * g;
  return r;
}
__device__ __forceinline__ float datan(float a) { return atanf(a); }
template <int N>
__device__ __forceinline__ void dsincos(const Dual<N>& a, Dual<N>* s, Dual<N>* c) {
  float sv, cv;
  sincosf(a.v, &sv, &cv);
  s->v = sv;
  c->v = cv;
#pragma unroll
  for (int k = 0; k < N; ++k) {
    s->d[k] = cv * a.d[k];
    c->d[k] = -sv * a.d[k];
  }
}
__device__ __forceinline__ void dsincos(float a, float* s, float* c) { sincosf(a, s, c); }
__device__ __forceinline__ float val(float a) { return a; }
template <int N>
__device__ __forceinline__ float val(const Dual<N>& a) { return a.v; }

// A value that every lane of the block computed from the same inputs: said so, it lives in a scalar register.  The parameter-only
// quantities of the USM and fisheye models are 13 to 17 dual numbers; in vector registers they alone would take most of the budget of Dual<6>.
__device__ __forceinline__ float uni(float v) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v))); }
template <int N>
__device__ __forceinline__ Dual<N> uni(const Dual<N>& a) {
  Dual<N> r;
  r.v = uni(a.v);
#pragma unroll
  for (int k = 0; k < N; ++k) r.d[k] = uni(a.d[k]);
  return r;
}

// Huber by IRLS: weight of a residual of norm r, and rho(r)
__device__ __forceinline__ void loss_of(float r, int huber, float delta, float* w, float* rho) {
  if (huber && r > delta) {
    *w = delta / r;
    *rho = delta * (r - 0.5f * delta);
  } else {
    *w = 1.f;
    *rho = 0.5f * r * r;
  }
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

}  // namespace

}  // namespace pf
