// Perspective fields -> camera parameters of the pinhole model of pf_fields_from_params (include/pf_hip.h pf_fit_camera, DESIGN.md
// section 10): the camera model and its per-pixel sums.  The batched per-image Levenberg-Marquardt fit around them (start, accumulate and
// solve kernels, launchers) is fit_lm.h, instantiated here over PinholeFit.  VALU and memory bound, no MFMA.
#include "fit_lm.h"
namespace pf {

namespace {

// ---------------------------------------------------------------- the model, ONE source for T = float and T = Dual<N>
// Every quantity is affine in (col, row) with coefficients that depend on the parameters only, so the per-block
// constructor does all trig of the parameters, and a pixel costs five affine forms (two for the up vector, three for the
// world ray), one rsqrt, one sqrt and the atan2 of the latitude.
template <class T>
struct CamModel {
  T ka, kb, sp;                                   // up: a = ka + sp px, b = kb + sp py; u = -(a, b) / |(a, b)|
  T xw0, xwc, xwr, yw0, ywc, ywr, zw0, zwc, zwr;  // world ray at (col, row): w = w0 + wc col + wr row
  __device__ CamModel(const T& roll, const T& pitch, const T& f, const T& cx, const T& cy, int H, int W) {
    T sr, cr, cp;
    dsincos(roll, &sr, &cr);
    dsincos(pitch, &sp, &cp);
    const T F = f * (float)H;
    const T Cx = (cx + 0.5f) * (float)W, Cy = (cy + 0.5f) * (float)H;
    const T cpF = cp * F;
    ka = sr * cpF - sp * Cx;
    kb = cr * cpF - sp * Cy;
    // the reference's latitude grid: linspace(-C, size - C, size), spacing size / (size - 1)
    const T invF = recip(F);
    const T x1 = invF * ((float)W / (float)(W - 1)), y1 = invF * ((float)H / (float)(H - 1));
    const T x0 = -(Cx * invF), y0 = -(Cy * invF);
    // x_w = x cr - y sr;  y_w = cp (x sr + y cr) - sp;  z_w = sp (x sr + y cr) + cp
    xw0 = x0 * cr - y0 * sr;
    xwc = x1 * cr;
    xwr = -(y1 * sr);
    const T t0 = x0 * sr + y0 * cr, tc = x1 * sr, tr = y1 * cr;
    yw0 = cp * t0 - sp;
    ywc = cp * tc;
    ywr = cp * tr;
    zw0 = sp * t0 + cp;
    zwc = sp * tc;
    zwr = sp * tr;
  }
  // up vector and latitude (degrees) of pixel (row, col); ok_up / ok_lat = false where the model itself is undefined
  // (at the vanishing point of the verticals, at the zenith)
  __device__ __forceinline__ void eval(float col, float row, T& ux, T& uy, T& lat, bool& ok_up, bool& ok_lat) const {
    const T a = fma_s(sp, col + 0.5f, ka), b = fma_s(sp, row + 0.5f, kb);
    const T n2 = a * a + b * b;
    ok_up = val(n2) > 0.f;
    const T inv = drsqrt(n2);
    ux = -(a * inv);
    uy = -(b * inv);
    const T xw = fma_s(xwr, row, fma_s(xwc, col, xw0));
    const T yw = fma_s(ywr, row, fma_s(ywc, col, yw0));
    const T zw = fma_s(zwr, row, fma_s(zwc, col, zw0));
    const T h2 = xw * xw + zw * zw;
    ok_lat = val(h2) > 0.f;
    lat = -(datan2(yw, dsqrt(h2)) * kRad2Deg);
  }
};

}  // namespace

struct PinholeFit {
  static constexpr int NTH = 5, STATE = FIT_STATE, REC = FIT_REC, COLS = PF_FIT_COLS;

  template <int NP>
  static __device__ __forceinline__ constexpr int theta_of(int k) { return k; }

  static __device__ __forceinline__ void clamp_theta(double* th) {
    th[1] = fmin(fmax(th[1], -kPitchMax), kPitchMax);
    th[2] = fmax(th[2], kFocalMin);
  }

  // the parameters as duals: derivative k of parameter k for k < NP, constants beyond
  template <int NP>
  static __device__ __forceinline__ CamModel<Dual<NP>> model_at(const double* th, int H, int W) {
    return CamModel<Dual<NP>>(dvar<NP>((float)th[0], 0), dvar<NP>((float)th[1], 1), dvar<NP>((float)th[2], 2), dvar<NP>((float)th[3], 3),
                              dvar<NP>((float)th[4], 4), H, W);
  }

  // the three residual rows of a pixel enter the sums in one fused expression
  template <int NP>
  static __device__ __forceinline__ void accum_pixel(const CamModel<Dual<NP>>& m, float col, float row, float pux, float puy, float plat,
                                                     const FitParams& prm, float* acc) {
    using R = Rec<NP>;
    if (!(isfinite(pux) && isfinite(puy) && isfinite(plat))) return;  // also the padding of a last partial chunk (NaN)
    Dual<NP> ux, uy, lat;
    bool ok_up, ok_lat;
    m.eval(col, row, ux, uy, lat, ok_up, ok_lat);
    const float rx = (ux.v - pux) * kRad2Deg, ry = (uy.v - puy) * kRad2Deg, rl = lat.v - plat;
    const float nu = sqrtf(rx * rx + ry * ry), nl = fabsf(rl);
    float wu, rhou, wl, rhol;
    loss_of(nu, prm.loss, prm.huber_delta, &wu, &rhou);
    loss_of(nl, prm.loss, prm.huber_delta, &wl, &rhol);
    wu = ok_up ? wu * prm.w_up : 0.f;
    wl = ok_lat ? wl * prm.w_lat : 0.f;
    float jx[NP], jy[NP], jl[NP];
#pragma unroll
    for (int k = 0; k < NP; ++k) {
      jx[k] = ok_up ? ux.d[k] * kRad2Deg : 0.f;
      jy[k] = ok_up ? uy.d[k] * kRad2Deg : 0.f;
      jl[k] = ok_lat ? lat.d[k] : 0.f;
    }
    int t = 0;
#pragma unroll
    for (int i = 0; i < NP; ++i) {
      const float ax = wu * jx[i], ay = wu * jy[i], al = wl * jl[i];
#pragma unroll
      for (int j = i; j < NP; ++j) acc[t++] += fmaf(ax, jx[j], fmaf(ay, jy[j], al * jl[j]));
      acc[R::G + i] += fmaf(ax, rx, fmaf(ay, ry, al * rl));
    }
    acc[R::COST] += (ok_up ? prm.w_up * rhou : 0.f) + (ok_lat ? prm.w_lat * rhol : 0.f);
    acc[R::UP2] += ok_up ? nu * nu : 0.f;
    acc[R::LAT2] += ok_lat ? rl * rl : 0.f;
    acc[R::CNT] += 1.f;
  }

  static __device__ __forceinline__ float start_focal(int c) { return start_focal_vfov(c); }

  static __device__ __forceinline__ CamModel<float> start_model(const double* th, float f, int H, int W) {
    return CamModel<float>((float)th[0], (float)th[1], f, 0.f, 0.f, H, W);
  }

  static __device__ __forceinline__ void start_cost(const CamModel<float>& m, float col, float row, float pux, float puy, float pl, const FitParams& prm,
                                                    float& cost) {
    float ux, uy, l, w, rho;
    bool ok_up, ok_lat;
    m.eval(col, row, ux, uy, l, ok_up, ok_lat);
    const float rx = (ux - pux) * kRad2Deg, ry = (uy - puy) * kRad2Deg;
    if (ok_up) {
      loss_of(sqrtf(rx * rx + ry * ry), prm.loss, prm.huber_delta, &w, &rho);
      cost += prm.w_up * rho;
    }
    if (ok_lat) {
      loss_of(fabsf(l - pl), prm.loss, prm.huber_delta, &w, &rho);
      cost += prm.w_lat * rho;
    }
  }
};

template void launch_fit_init<PinholeFit>(const FitBatch&, const FitParams&, hipStream_t);
template void launch_fit_iteration<PinholeFit>(const FitBatch&, const FitParams&, hipStream_t);
template void launch_fit_shared_start<PinholeFit>(const FitGroups&, hipStream_t);
template void launch_fit_shared_accum<PinholeFit>(const FitBatch&, const FitParams&, double*, hipStream_t);
template void launch_fit_shared_solve<PinholeFit>(const FitGroups&, const FitParams&, hipStream_t);

}  // namespace pf
