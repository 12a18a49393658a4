// Perspective fields -> a fisheye lens (include/pf_hip.h pf_fit_fisheye): the lens model of fisheye_target.hip in the other
// direction, its inverse projection and label formulas over dual numbers and their per-pixel sums, fitted by the Levenberg-Marquardt driver of
// fit_lm.h (instantiated here over FisheyeFit<KIND, POLY>).  VALU and memory bound; plain C++, no MFMA, no atomics.
// Model, theta = (roll r, pitch p, f, cx, cy, k1, k2), at the pixel centre (a, b) = (col + 1/2, row + 1/2) for both labels:
//   F = f H, Cx = (cx + 1/2) W, Cy = (cy + 1/2) H; dx = a - Cx, dy = b - Cy, r = hypot(dx, dy), rho = r / F, (c, s) = (dx, dy) / r
//   theta_d = rho^-1(rho); theta = theta_d without a polynomial, else PF_FISHEYE_NEWTON_STEPS clamped Newton steps in plain floats; its derivatives
//   from the implicit function: d theta = (d theta_d - theta^3 d k1 - theta^5 d k2) / P'(theta)
//   the pixel has a model value iff r > PF_FISHFIT_R_MIN, 0 < theta < theta_max (FitParams::theta_max) and, with a polynomial, the iteration ended at a
//   root (|P(theta) - theta_d| <= PF_FISHFIT_ROOT_TOL) on a rising branch (P'(theta) >= PF_FISHFIT_SLOPE_MIN); the equisolid kind needs rho < 2
//   X = (sin theta c, sin theta s, cos theta); g = R^T (0, -1, 0) = (-cos p sin r, -cos p cos r, sin p), R = R_pitch R_roll as in fit_camera_usm.hip
//   lat = -atan2(W.y, hypot(W.x, W.z)) degrees, W = R X
//   up ~ m' ge (c, s) + (rho / sin theta) gp (-s, c) normalised, ge = g . e_theta, gp = g . e_phi, m' = rho'(theta_d) P'(theta); the up rows are off
//   where ge^2 + gp^2 < PF_PANO_UP_MIN_T2
// fit_lm.h comes first: the templates of fisheye_model.h find the float overloads of fit_dual.h where they are defined, the dual ones where T is.
#include "fit_lm.h"

#include "fisheye_model.h"

namespace pf {

namespace {

// theta as a number of the model's type from the root t that the float iteration found: the implicit function's derivatives
__device__ __forceinline__ float implicit_theta(float, float, float, float t, float) { return t; }
template <int N>
__device__ __forceinline__ Dual<N> implicit_theta(const Dual<N>& td, const Dual<N>& k1, const Dual<N>& k2, float t, float slope) {
  Dual<N> r;
  r.v = t;
  const float inv = 1.0f / slope, t3 = t * t * t, t5 = t3 * t * t;
#pragma unroll
  for (int k = 0; k < N; ++k) r.d[k] = (td.d[k] - t3 * k1.d[k] - t5 * k2.d[k]) * inv;
  return r;
}

// an image point with a model value
template <class T>
struct LensPoint {
  T c, s;      // cosine and sine of its azimuth about the lens axis
  T st, ct;    // of theta
  T rho, ms;   // r / F; m' = rho'(theta_d) P'(theta)
};

// ---------------------------------------------------------------- the model, ONE source for T = float and T = Dual<N>
// The constructor does everything that depends on the parameters only (trig, g, the rows of R, 1 / F, the centre); the polynomial's coefficients
// are wave-uniform floats for the Newton iteration and numbers of the model's type for the derivatives.
template <int KIND, class T>
struct FisheyeModel {
  T gx, gy, gz;    // g; R's second row is -g
  T cr, sr;        // R's first row (cr, -sr, 0)
  T r20, r21, cp;  // R's third row (sp sr, sp cr, cp)
  T invF, Cx, Cy;
  T k1, k2;
  float k1v, k2v;
  bool poly;       // k1 != 0 or k2 != 0
  bool live;       // every parameter is finite; otherwise no pixel has a model value
  __device__ FisheyeModel(const T& roll, const T& pitch, const T& f, const T& cx, const T& cy, const T& k1_, const T& k2_, int H, int W) {
    T s_r, c_r, s_p, c_p;
    dsincos(roll, &s_r, &c_r);
    dsincos(pitch, &s_p, &c_p);
    sr = uni(s_r);
    cr = uni(c_r);
    cp = uni(c_p);
    gz = uni(s_p);
    gx = uni(-(c_p * s_r));
    gy = uni(-(c_p * c_r));
    r20 = uni(s_p * s_r);
    r21 = uni(s_p * c_r);
    invF = uni(recip(f * (float)H));
    Cx = uni((cx + 0.5f) * (float)W);
    Cy = uni((cy + 0.5f) * (float)H);
    k1 = uni(k1_);
    k2 = uni(k2_);
    k1v = val(k1);
    k2v = val(k2);
    poly = k1v != 0.f || k2v != 0.f;
    live = isfinite(val(roll)) && isfinite(val(pitch)) && isfinite(val(f)) && isfinite(val(Cx)) && isfinite(val(Cy)) && isfinite(k1v) && isfinite(k2v);
  }

  // the inverse projection of pixel (row, col); false: the pixel has no model value
  __device__ __forceinline__ bool point_at(float col, float row, float tmax, LensPoint<T>& p) const {
    if (!live) return false;
    const T dx = -(Cx + -(col + 0.5f)), dy = -(Cy + -(row + 0.5f));
    const T r2 = dx * dx + dy * dy;
    const T ir = drsqrt(r2);
    const T r = r2 * ir;
    if (!(val(r) - PF_FISHFIT_R_MIN > 0.f)) return false;
    p.rho = r * invF;
    if (KIND == PF_FISHEYE_EQUISOLID && !(2.f - val(p.rho) > 0.f)) return false;
    const T td = fisheye_rho_inverse<KIND>(p.rho);
    float t = val(td), slope = 1.f;
    if (poly) {
      t = fminf(t, tmax);
      for (int s = 0; s < PF_FISHEYE_NEWTON_STEPS; ++s) {
        const float e = fisheye_poly(t, k1v, k2v, 0.f, 0.f) - val(td);
        t = fminf(fmaxf(t - e / fisheye_poly_slope(t, k1v, k2v, 0.f, 0.f), 0.f), tmax);
      }
      slope = fisheye_poly_slope(t, k1v, k2v, 0.f, 0.f);
      if (!(slope >= PF_FISHFIT_SLOPE_MIN && fabsf(fisheye_poly(t, k1v, k2v, 0.f, 0.f) - val(td)) <= PF_FISHFIT_ROOT_TOL)) return false;
    }
    if (!(tmax - t > 0.f && t > 0.f)) return false;  // t = 0: the iteration was clamped at the axis (theta_d within the root tolerance); 1 / sin theta
    const T th = implicit_theta(td, k1, k2, t, slope);
    p.c = dx * ir;
    p.s = dy * ir;
    dsincos(th, &p.st, &p.ct);
    p.ms = fisheye_poly_slope(th, k1, k2);
    if constexpr (KIND != PF_FISHEYE_EQUIDISTANT) p.ms = p.ms * fisheye_rho_slope<KIND>(td);
    return true;
  }
  // up vector; ok = false where the pixel looks at the zenith or the nadir
  __device__ __forceinline__ void up_at(const LensPoint<T>& p, T& ux, T& uy, bool& ok) const {
    const T ge = p.ct * (gx * p.c + gy * p.s) - gz * p.st;
    const T gp = gy * p.c - gx * p.s;
    ok = val(ge) * val(ge) + val(gp) * val(gp) >= PF_PANO_UP_MIN_T2;
    const T A = p.ms * ge, B = p.rho * recip(p.st) * gp;
    const T px = A * p.c - B * p.s, py = A * p.s + B * p.c;
    const T in = drsqrt(px * px + py * py);
    ux = px * in;
    uy = py * in;
  }
  // latitude (degrees); ok = false at the zenith and the nadir
  __device__ __forceinline__ void lat_at(const LensPoint<T>& p, T& lat, bool& ok) const {
    const T Xx = p.st * p.c, Xy = p.st * p.s;
    const T yw = -(Xx * gx + Xy * gy + p.ct * gz);
    const T xw = Xx * cr - Xy * sr;
    const T zw = Xx * r20 + Xy * r21 + p.ct * cp;
    const T h2 = xw * xw + zw * zw;
    ok = val(h2) > 0.f;
    lat = -(datan2(yw, dsqrt(h2)) * kRad2Deg);
  }
};

constexpr double kPolyMax = 0.5;

}  // namespace

// KIND: PF_FISHEYE_*.  POLY: k1 and k2 are free.  The free sets: without POLY (r, p, f) and (r, p, f, cx, cy), with it (r, p, f, k1, k2) and all seven;
// FitParams::free_pp selects the larger of a pair.
template <int KIND, bool POLY>
struct FisheyeFit {
  static constexpr int NTH = 7, STATE = FISHFIT_STATE, REC = FISHFIT_REC, COLS = PF_FISHFIT_COLS;
  static constexpr int NP_PP = POLY ? 7 : 5, NP_HELD = POLY ? 5 : 3;  // free parameters with and without the principal point

  // free parameter k of the NP-parameter fit -> its place in theta
  template <int NP>
  static __device__ __forceinline__ constexpr int theta_of(int k) { return (POLY && NP == NP_HELD && k >= 3) ? k + 2 : k; }

  // by comparisons, not fmin / fmax: a non-finite start stays what it is, and the model then has no value anywhere
  static __device__ __forceinline__ double clamp1(double v, double lo, double hi) { return v < lo ? lo : v > hi ? hi : v; }
  static __device__ __forceinline__ void clamp_theta(double* th) {
    th[0] = remainder(th[0], 2.0 * kPi);
    th[1] = clamp1(th[1], -kPitchMax, kPitchMax);
    th[2] = th[2] < kFocalMin ? kFocalMin : th[2];
    th[5] = clamp1(th[5], -kPolyMax, kPolyMax);
    th[6] = clamp1(th[6], -kPolyMax, kPolyMax);
  }

  // the parameters as duals: derivative k of free parameter k, constants for the held ones
  template <int NP>
  static __device__ __forceinline__ FisheyeModel<KIND, Dual<NP>> model_at(const double* th, int H, int W) {
    static_assert(NP == NP_PP || NP == NP_HELD, "not a free set of this fit");
    constexpr int kc = NP == NP_PP ? 3 : NP;              // cx (cy follows); NP: held
    constexpr int kk = !POLY ? NP : NP == NP_PP ? 5 : 3;  // k1 (k2 follows)
    return FisheyeModel<KIND, Dual<NP>>(dvar<NP>((float)th[0], 0), dvar<NP>((float)th[1], 1), dvar<NP>((float)th[2], 2), dvar<NP>((float)th[3], kc),
                                        dvar<NP>((float)th[4], kc + (kc < NP ? 1 : 0)), dvar<NP>((float)th[5], kk), dvar<NP>((float)th[6], kk + (kk < NP ? 1 : 0)),
                                        H, W);
  }

  // The up and the latitude contributions of a pixel go into the sums one after the other, so that one set of duals is live.
  template <int NP>
  static __device__ __forceinline__ void accum_pixel(const FisheyeModel<KIND, Dual<NP>>& m, float col, float row, float pux, float puy, float plat,
                                                     const FitParams& prm, float* acc) {
    using R = Rec<NP>;
    if (!(isfinite(pux) && isfinite(puy) && isfinite(plat))) return;  // also the padding of a last partial chunk (NaN)
    LensPoint<Dual<NP>> p;
    if (!m.point_at(col, row, prm.theta_max, p)) return;  // no model value
    {
      Dual<NP> ux, uy;
      bool ok;
      m.up_at(p, ux, uy, ok);
      const float rx = (ux.v - pux) * kRad2Deg, ry = (uy.v - puy) * kRad2Deg;
      const float nu = sqrtf(rx * rx + ry * ry);
      float w, rho;
      loss_of(nu, prm.loss, prm.huber_delta, &w, &rho);
      w = ok ? w * prm.w_up : 0.f;
      add_row<NP>(acc, ux, ok, kRad2Deg, w, rx);
      add_row<NP>(acc, uy, ok, kRad2Deg, w, ry);
      acc[R::COST] += ok ? prm.w_up * rho : 0.f;
      acc[R::UP2] += ok ? nu * nu : 0.f;
    }
    {
      Dual<NP> lat;
      bool ok;
      m.lat_at(p, lat, ok);
      const float rl = lat.v - plat;
      float w, rho;
      loss_of(fabsf(rl), prm.loss, prm.huber_delta, &w, &rho);
      w = ok ? w * prm.w_lat : 0.f;
      add_row<NP>(acc, lat, ok, 1.f, w, rl);
      acc[R::COST] += ok ? prm.w_lat * rho : 0.f;
      acc[R::LAT2] += ok ? rl * rl : 0.f;
    }
    acc[R::CNT] += 1.f;
  }

  // candidate c of the start search: the half field of view h_c = (20 + 7 c) degrees over half the height, f = 0.5 / rho(h_c)
  static __device__ __forceinline__ float start_focal(int c) {
    const double h = (20.0 + 7.0 * c) * (kPi / 180.0);
    const double rho = KIND == PF_FISHEYE_EQUIDISTANT ? h : KIND == PF_FISHEYE_EQUISOLID ? 2.0 * sin(0.5 * h) : 2.0 * tan(0.5 * h);
    return (float)(0.5 / rho);
  }

  // At the circle centre up = (-sin r, -cos r) and lat = p for every kind; the candidates are searched with the centre in the middle and no polynomial.
  static __device__ __forceinline__ FisheyeModel<KIND, float> start_model(const double* th, float f, int H, int W) {
    return FisheyeModel<KIND, float>((float)th[0], (float)th[1], f, 0.f, 0.f, 0.f, 0.f, H, W);
  }

  static __device__ __forceinline__ void start_cost(const FisheyeModel<KIND, float>& m, float col, float row, float pux, float puy, float pl,
                                                    const FitParams& prm, float& cost) {
    LensPoint<float> p;
    if (!m.point_at(col, row, prm.theta_max, p)) return;
    float ux, uy, l, w, rho;
    bool ok;
    m.up_at(p, ux, uy, ok);
    const float rx = (ux - pux) * kRad2Deg, ry = (uy - puy) * kRad2Deg;
    if (ok) {
      loss_of(sqrtf(rx * rx + ry * ry), prm.loss, prm.huber_delta, &w, &rho);
      cost += prm.w_up * rho;
    }
    m.lat_at(p, l, ok);
    if (ok) {
      loss_of(fabsf(l - pl), prm.loss, prm.huber_delta, &w, &rho);
      cost += prm.w_lat * rho;
    }
  }
};

// One accumulate + solve pair over this model's free sets: NP_PP or NP_HELD parameters, where the driver's own launcher takes NTH or NTH - 2.
template <class Fit>
static void fisheye_iteration(const FitBatch& fb, const FitParams& prm, hipStream_t s) {
  int mx = 1;
  for (int k = 0; k < fb.n; ++k) mx = std::max(mx, fb.nblk[k]);
  if (prm.free_pp) {
    hipLaunchKernelGGL((fit_accum_kernel<Fit, Fit::NP_PP>), dim3(mx, fb.n), dim3(256), 0, s, fb, prm);
    hipLaunchKernelGGL((fit_solve_kernel<Fit, Fit::NP_PP>), dim3(fb.n), dim3(64), 0, s, fb);
  } else {
    hipLaunchKernelGGL((fit_accum_kernel<Fit, Fit::NP_HELD>), dim3(mx, fb.n), dim3(256), 0, s, fb, prm);
    hipLaunchKernelGGL((fit_solve_kernel<Fit, Fit::NP_HELD>), dim3(fb.n), dim3(64), 0, s, fb);
  }
}

#define PF_FISHEYE_FIT(KIND, POLY)                                                                                               \
  template <>                                                                                                                    \
  void launch_fit_iteration<FisheyeFit<KIND, POLY>>(const FitBatch& fb, const FitParams& prm, hipStream_t s) {                   \
    fisheye_iteration<FisheyeFit<KIND, POLY>>(fb, prm, s);                                                                       \
  }                                                                                                                              \
  template void launch_fit_init<FisheyeFit<KIND, POLY>>(const FitBatch&, const FitParams&, hipStream_t);
PF_FISHEYE_FIT(PF_FISHEYE_EQUIDISTANT, false)
PF_FISHEYE_FIT(PF_FISHEYE_EQUIDISTANT, true)
PF_FISHEYE_FIT(PF_FISHEYE_EQUISOLID, false)
PF_FISHEYE_FIT(PF_FISHEYE_EQUISOLID, true)
PF_FISHEYE_FIT(PF_FISHEYE_STEREOGRAPHIC, false)
PF_FISHEYE_FIT(PF_FISHEYE_STEREOGRAPHIC, true)
#undef PF_FISHEYE_FIT

}  // namespace pf
