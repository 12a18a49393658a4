// Perspective fields <-> camera parameters of the Unified Spherical Model (include/pf_hip.h pf_fit_camera_usm /
// pf_fields_from_params_usm): the camera model with the mirror parameter xi and its per-pixel sums, fitted by
// the Levenberg-Marquardt driver of fit_lm.h (instantiated here over UsmFit), and the forward direction of the same model.  VALU and
// memory bound; plain C++, no MFMA, no atomics.
//   fields_usm_kernel     theta [6] in device memory -> up [2][H][W], lat [H][W]; the label formulas of cam_model.h
// Model, theta = (roll r, pitch p, f, cx, cy, xi) -- pf_pano_crop's intrinsics, ray, rotation and labels:
//   x = (a - Cx) / F, y = (b - Cy) / F, F = f H, Cx = (cx + 1/2) W, Cy = (cy + 1/2) H
//   rho^2 = x^2 + y^2, disc = 1 + (1 - xi^2) rho^2, eta = (xi + sqrt(disc)) / (1 + rho^2), X = (eta x, eta y, eta - xi)
//   g = R^T (0, -1, 0) = (-cos p sin r, -cos p cos r, sin p); the second row of R = R_pitch R_roll is -g, so X_w.y = -(X . g)
//   up at (col + 1/2, row + 1/2): s = g_z + xi (X . g); (g_x D - X_x s, g_y D - X_y s) with D = X_z + xi = eta, and eta > 0 for every
//       xi in the fit's range [-0.5, 2], so the direction is (g_x - x s, g_y - y s), normalised
//   lat (degrees) of X_w at the linspace point (col W / (W - 1), row H / (H - 1))
//   disc < 0 at either point: the pixel is skipped (no weight, not counted)
#include "cam_model.h"
#include "fit_lm.h"

namespace pf {

namespace {

// ---------------------------------------------------------------- the model, ONE source for T = float and T = Dual<N>
// The constructor does everything that depends on the parameters only (trig, g, the rows of R, 1 / F, the affine coefficients
// of x and y on both grids).  A pixel costs two unprojections (one sqrt and one reciprocal each), one rsqrt, one sqrt and
// the atan2 of the latitude.
template <class T>
struct UsmModel {
  T gx, gy, gz;          // g; R's second row is -g
  T cr, sr;              // R's first row (cr, -sr, 0)
  T r20, r21, cp;        // R's third row (sp sr, sp cr, cp)
  T xi, om;              // om = 1 - xi^2
  T xc0, yc0, inv;       // pixel centres: x = xc0 + inv col, y = yc0 + inv row
  T xl0, yl0, xl1, yl1;  // the reference's latitude grid, linspace(-C, size - C, size): x = xl0 + xl1 col, y = yl0 + yl1 row
  __device__ UsmModel(const T& roll, const T& pitch, const T& f, const T& cx, const T& cy, const T& xi_, int H, int W) {
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
    xi = uni(xi_);
    om = uni(-(xi_ * xi_) + 1.0f);
    const T invF = recip(f * (float)H);
    const T Cx = (cx + 0.5f) * (float)W, Cy = (cy + 0.5f) * (float)H;
    inv = uni(invF);
    xc0 = uni(-((Cx + -0.5f) * invF));
    yc0 = uni(-((Cy + -0.5f) * invF));
    xl0 = uni(-(Cx * invF));
    yl0 = uni(-(Cy * invF));
    xl1 = uni(invF * ((float)W / (float)(W - 1)));
    yl1 = uni(invF * ((float)H / (float)(H - 1)));
  }
  __device__ __forceinline__ void centre_point(float col, float row, T& x, T& y) const {
    x = fma_s(inv, col, xc0);
    y = fma_s(inv, row, yc0);
  }
  __device__ __forceinline__ void linspace_point(float col, float row, T& x, T& y) const {
    x = fma_s(xl1, col, xl0);
    y = fma_s(yl1, row, yl0);
  }
  // rho^2 and disc of an image point; the point has a ray where val(disc) >= 0
  __device__ __forceinline__ void disc_at(const T& x, const T& y, T& rho2, T& disc) const {
    rho2 = x * x + y * y;
    disc = om * rho2 + 1.0f;
  }
  __device__ __forceinline__ T eta_of(const T& rho2, const T& disc) const { return (xi + dsqrt(disc)) * recip(rho2 + 1.0f); }
  // up vector at a pixel centre (x, y); ok = false at the vanishing point of the verticals
  __device__ __forceinline__ void up_at(const T& x, const T& y, const T& rho2, const T& disc, T& ux, T& uy, bool& ok) const {
    const T eta = eta_of(rho2, disc);
    const T Xg = eta * (x * gx + y * gy + gz) - xi * gz;
    const T s = gz + xi * Xg;
    const T a = gx - x * s, b = gy - y * s;
    const T n2 = a * a + b * b;
    ok = val(n2) > 0.f;
    const T in = drsqrt(n2);
    ux = a * in;
    uy = b * in;
  }
  // latitude (degrees) of the ray of a linspace point (x, y); ok = false at the zenith
  __device__ __forceinline__ void lat_at(const T& x, const T& y, const T& rho2, const T& disc, T& lat, bool& ok) const {
    const T eta = eta_of(rho2, disc);
    const T Xx = eta * x, Xy = eta * y, Xz = eta - xi;
    const T yw = -(Xx * gx + Xy * gy + Xz * gz);
    const T xw = Xx * cr - Xy * sr;
    const T zw = Xx * r20 + Xy * r21 + Xz * cp;
    const T h2 = xw * xw + zw * zw;
    ok = val(h2) > 0.f;
    lat = -(datan2(yw, dsqrt(h2)) * kRad2Deg);
  }
};

constexpr double kXiMin = -0.5, kXiMax = 2.0;

}  // namespace

struct UsmFit {
  static constexpr int NTH = 6, STATE = USMFIT_STATE, REC = USMFIT_REC, COLS = PF_USMFIT_COLS;

  // free parameter k of the NP-parameter fit -> its place in theta: (r, p, f, xi) or all six
  template <int NP>
  static __device__ __forceinline__ constexpr int theta_of(int k) { return NP == 6 ? k : (k < 3 ? k : 5); }

  // roll is periodic: a long early step may land turns away from the start, so it is brought back into [-pi, pi]
  static __device__ __forceinline__ void clamp_theta(double* th) {
    th[0] = remainder(th[0], 2.0 * kPi);
    th[1] = fmin(fmax(th[1], -kPitchMax), kPitchMax);
    th[2] = fmax(th[2], kFocalMin);
    th[5] = fmin(fmax(th[5], kXiMin), kXiMax);
  }

  // the parameters as duals: derivative k of free parameter k, constants for the held ones
  template <int NP>
  static __device__ __forceinline__ UsmModel<Dual<NP>> model_at(const double* th, int H, int W) {
    constexpr int kc = NP == 6 ? 3 : NP;  // rel_cx / rel_cy are free in the 6-parameter fit only
    return UsmModel<Dual<NP>>(dvar<NP>((float)th[0], 0), dvar<NP>((float)th[1], 1), dvar<NP>((float)th[2], 2), dvar<NP>((float)th[3], kc),
                              dvar<NP>((float)th[4], kc + (NP == 6 ? 1 : 0)), dvar<NP>((float)th[5], NP - 1), H, W);
  }

  // The up and the latitude contributions of a pixel go into the sums one after the other, so that one set of duals is live.
  template <int NP>
  static __device__ __forceinline__ void accum_pixel(const UsmModel<Dual<NP>>& m, float col, float row, float pux, float puy, float plat,
                                                     const FitParams& prm, float* acc) {
    using R = Rec<NP>;
    if (!(isfinite(pux) && isfinite(puy) && isfinite(plat))) return;  // also the padding of a last partial chunk (NaN)
    Dual<NP> x, y, rho2, disc, xl, yl, rho2l, discl;
    m.centre_point(col, row, x, y);
    m.disc_at(x, y, rho2, disc);
    m.linspace_point(col, row, xl, yl);
    m.disc_at(xl, yl, rho2l, discl);
    if (!(disc.v >= 0.f && discl.v >= 0.f)) return;  // no ray: no model value
    {
      Dual<NP> ux, uy;
      bool ok;
      m.up_at(x, y, rho2, disc, ux, uy, ok);
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
      m.lat_at(xl, yl, rho2l, discl, lat, ok);
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

  static __device__ __forceinline__ float start_focal(int c) { return start_focal_vfov(c); }

  // The centre ray is (0, 0, 1) for every xi, so the start of the pinhole fit holds here too; its candidates are searched at xi = 0.
  static __device__ __forceinline__ UsmModel<float> start_model(const double* th, float f, int H, int W) {
    return UsmModel<float>((float)th[0], (float)th[1], f, 0.f, 0.f, 0.f, H, W);
  }

  static __device__ __forceinline__ void start_cost(const UsmModel<float>& m, float col, float row, float pux, float puy, float pl, const FitParams& prm,
                                                    float& cost) {
    float x, y, rho2, disc, ux, uy, l, w, rho;
    bool ok;
    m.centre_point(col, row, x, y);
    m.disc_at(x, y, rho2, disc);
    m.up_at(x, y, rho2, disc, ux, uy, ok);
    const float rx = (ux - pux) * kRad2Deg, ry = (uy - puy) * kRad2Deg;
    if (ok) {
      loss_of(sqrtf(rx * rx + ry * ry), prm.loss, prm.huber_delta, &w, &rho);
      cost += prm.w_up * rho;
    }
    m.linspace_point(col, row, x, y);
    m.disc_at(x, y, rho2, disc);
    m.lat_at(x, y, rho2, disc, l, ok);
    if (ok) {
      loss_of(fabsf(l - pl), prm.loss, prm.huber_delta, &w, &rho);
      cost += prm.w_lat * rho;
    }
  }
};

template void launch_fit_init<UsmFit>(const FitBatch&, const FitParams&, hipStream_t);
template void launch_fit_iteration<UsmFit>(const FitBatch&, const FitParams&, hipStream_t);
template void launch_fit_shared_start<UsmFit>(const FitGroups&, hipStream_t);
template void launch_fit_shared_accum<UsmFit>(const FitBatch&, const FitParams&, double*, hipStream_t);
template void launch_fit_shared_solve<UsmFit>(const FitGroups&, const FitParams&, hipStream_t);

// ---------------------------------------------------------------- theta -> fields
// One thread per 4 consecutive pixels of the flattened image.  xi == 0: pinhole_fields_at, the bits of pf_fields_from_params;
// otherwise usm_up_of_ray / usm_lat_of_ray, the bits of pf_pano_crop's labels.  NaN where a point has no ray.
__global__ __launch_bounds__(256) void fields_usm_kernel(const float* __restrict__ cam, int H, int W, float* __restrict__ up, float* __restrict__ lat,
                                                         int vec) {
  const long n = (long)H * W, nchunk = (n + 3) >> 2;
  const float roll = cam[0], pitch = cam[1], f = cam[2], rcx = cam[3], rcy = cam[4], xi = cam[5];
  const PinholeFields pin = pinhole_fields_setup(roll, pitch, f, rcx, rcy, H, W);
  float sr, cr, sp, cp, R[9];
  sincosf(roll, &sr, &cr);
  sincosf(pitch, &sp, &cp);
  cam_rotation(sr, cr, sp, cp, R);
  const float g[3] = {-R[3], -R[4], -R[5]};
  const float F = f * (float)H, invF = 1.f / F, Cx = (rcx + 0.5f) * (float)W, Cy = (rcy + 0.5f) * (float)H;
  const float sx = W > 1 ? (float)W / (float)(W - 1) : 0.f, sy = H > 1 ? (float)H / (float)(H - 1) : 0.f;
  for (long q = (long)blockIdx.x * 256 + threadIdx.x; q < nchunk; q += (long)gridDim.x * 256) {
    const long p0 = q << 2;
    int row = (int)(p0 / W), col = (int)(p0 - (long)row * W);
    float ux[4], uy[4], la[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      ux[k] = uy[k] = la[k] = __builtin_nanf("");
      if (p0 + k < n) {
        if (xi == 0.f) {
          const FieldsPixel o = pinhole_fields_at(pin, row, col);
          ux[k] = o.ux;
          uy[k] = o.uy;
          la[k] = o.lat;
        } else {
          {
            const float x = ((float)col + 0.5f - Cx) * invF, y = ((float)row + 0.5f - Cy) * invF;
            float r2, X[3];
            const float disc = usm_disc(x, y, xi, &r2);
            if (disc >= 0.f) {
              usm_ray_of(x, y, xi, r2, disc, X);
              usm_up_of_ray(X, g, xi, &ux[k], &uy[k]);
            }
          }
          {
            const float x = ((float)col * sx - Cx) / F, y = ((float)row * sy - Cy) / F;
            float r2, X[3];
            const float disc = usm_disc(x, y, xi, &r2);
            if (disc >= 0.f) {
              usm_ray_of(x, y, xi, r2, disc, X);
              la[k] = usm_lat_of_ray(X, R);
            }
          }
        }
      }
      if (++col == W) { col = 0; ++row; }
    }
    if (vec) {  // n % 4 == 0 and 16-byte aligned planes
      *reinterpret_cast<float4*>(up + p0) = make_float4(ux[0], ux[1], ux[2], ux[3]);
      *reinterpret_cast<float4*>(up + n + p0) = make_float4(uy[0], uy[1], uy[2], uy[3]);
      *reinterpret_cast<float4*>(lat + p0) = make_float4(la[0], la[1], la[2], la[3]);
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (p0 + k < n) {
          up[p0 + k] = ux[k];
          up[n + p0 + k] = uy[k];
          lat[p0 + k] = la[k];
        }
      }
    }
  }
}

void launch_fields_usm(const float* cam6, int H, int W, float* up, float* lat, hipStream_t s) {
  const long n = (long)H * W;
  long blocks = ((n + 3) / 4 + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  const int vec = (n & 3) == 0 && ((reinterpret_cast<uintptr_t>(up) | reinterpret_cast<uintptr_t>(lat)) & 15) == 0;
  hipLaunchKernelGGL(fields_usm_kernel, dim3((unsigned)blocks), dim3(256), 0, s, cam6, H, W, up, lat, vec);
}

}  // namespace pf
