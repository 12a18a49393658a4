// Perspective fields <-> camera parameters of the Unified Spherical Model (include/pf_hip.h pf_fit_camera_usm /
// pf_fields_from_params_usm): the fit of fit_camera.hip with the mirror parameter xi as one more unknown,
// and the forward direction of the same model.  VALU and memory bound; plain C++, no MFMA, no atomics.
//   usmfit_init_kernel    one wave per image: start parameters (xi = 0, the rest as the pinhole fit) or the caller's, state reset
//   usmfit_accum_kernel   grid (blocks per image) x (images): model + Jacobian per pixel by forward-mode dual numbers, upper
//                         triangle of J^T W J, J^T W r, cost and rms sums per block -> one partial record per block
//   usmfit_solve_kernel   one wave per image: partials summed in block order in fp64, LM accept / reject, damped Cholesky
//   fields_usm_kernel     theta [6] in device memory -> up [2][H][W], lat [H][W]; xi == 0: the pinhole path of cam_model.h
// Model, theta = (roll r, pitch p, f, cx, cy, xi) -- pf_pano_crop's intrinsics, ray, rotation and labels:
//   x = (a - Cx) / F, y = (b - Cy) / F, F = f H, Cx = (cx + 1/2) W, Cy = (cy + 1/2) H
//   rho^2 = x^2 + y^2, disc = 1 + (1 - xi^2) rho^2, eta = (xi + sqrt(disc)) / (1 + rho^2), X = (eta x, eta y, eta - xi)
//   g = R^T (0, -1, 0) = (-cos p sin r, -cos p cos r, sin p); the second row of R = R_pitch R_roll is -g, so X_w.y = -(X . g)
//   up at (col + 1/2, row + 1/2): s = g_z + xi (X . g); (g_x D - X_x s, g_y D - X_y s) with D = X_z + xi = eta, and eta > 0 for every
//       xi in the fit's range [-0.5, 2], so the direction is (g_x - x s, g_y - y s), normalised
//   lat (degrees) of X_w at the linspace point (col W / (W - 1), row H / (H - 1))
//   disc < 0 at either point: the pixel is skipped (no weight, not counted)
#include <math.h>
#include <stdint.h>

#include <algorithm>

#include "../../include/pf_hip.h"
#include "cam_model.h"
#include "fit_dual.h"
#include "pf_kernels.h"

namespace pf {

namespace {

// A value that every lane of the block computed from the same inputs: said so, it lives in a scalar register.  The model's
// parameter-only quantities are 17 dual numbers; in vector registers they alone would take most of the budget of Dual<6>.
__device__ __forceinline__ float uni(float v) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v))); }
template <int N>
__device__ __forceinline__ Dual<N> uni(const Dual<N>& a) {
  Dual<N> r;
  r.v = uni(a.v);
#pragma unroll
  for (int k = 0; k < N; ++k) r.d[k] = uni(a.d[k]);
  return r;
}

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

// per-block record (USMFIT_REC doubles): [0, NH) upper triangle of J^T W J row by row, [NH, NH + NP) J^T W r, then the cost,
// sum |r_up|^2, sum r_lat^2 and the valid pixels
template <int NP>
struct Rec {
  static constexpr int NH = NP * (NP + 1) / 2;
  static constexpr int G = NH, COST = NH + NP, UP2 = COST + 1, LAT2 = COST + 2, CNT = COST + 3, NV = COST + 4;
};
static_assert(Rec<6>::NV <= USMFIT_REC, "record too small");

// state of one image (USMFIT_STATE doubles)
enum : int {
  NTH = 6,
  S_CUR = 0,     // [6] accepted parameters (roll, pitch, f, cx, cy, xi)
  S_TRIAL = 6,   // [6] parameters the next accumulate pass evaluates
  S_COST = 12,   // cost at S_CUR
  S_LAMBDA = 13,
  S_NEV = 14,    // evaluations so far
  S_CONV = 15,   // 0: running; 1: converged; 2: no finite cost at the start.  Accumulate and solve return at once when != 0
  S_UP2 = 16, S_LAT2 = 17, S_CNT = 18,  // rms sums and valid pixels at S_CUR
  S_HG = 19,     // [NH + NP] J^T W J and J^T W r at S_CUR
  S_END = S_HG + Rec<6>::NH + 6
};
static_assert(S_END <= USMFIT_STATE, "state too small");

constexpr double kPi = 3.14159265358979323846;
constexpr double kPitchMax = 89.9 * kPi / 180.0, kFocalMin = 1e-3, kXiMin = -0.5, kXiMax = 2.0;

// roll is periodic: a long early step may land turns away from the start, so it is brought back into [-pi, pi]
__device__ __forceinline__ void clamp_theta(double* th) {
  th[0] = remainder(th[0], 2.0 * kPi);
  th[1] = fmin(fmax(th[1], -kPitchMax), kPitchMax);
  th[2] = fmax(th[2], kFocalMin);
  th[5] = fmin(fmax(th[5], kXiMin), kXiMax);
}

// free parameter k of the NP-parameter fit -> its place in theta: (r, p, f, xi) or all six
template <int NP>
__device__ __forceinline__ constexpr int theta_of(int k) { return NP == 6 ? k : (k < 3 ? k : 5); }

// the parameters as duals: derivative k of free parameter k, constants for the held ones
template <int NP>
__device__ __forceinline__ UsmModel<Dual<NP>> model_at(const double* th, int H, int W) {
  constexpr int kc = NP == 6 ? 3 : NP;  // rel_cx / rel_cy are free in the 6-parameter fit only
  return UsmModel<Dual<NP>>(dvar<NP>((float)th[0], 0), dvar<NP>((float)th[1], 1), dvar<NP>((float)th[2], 2), dvar<NP>((float)th[3], kc),
                            dvar<NP>((float)th[4], kc + (NP == 6 ? 1 : 0)), dvar<NP>((float)th[5], NP - 1), H, W);
}

__device__ void write_out(float* o, const double* st) {
  const double r2d = 180.0 / kPi;
  const double* th = st + S_CUR;
  const double f = th[2], cx = th[3], cy = th[4];
  const double P = f * f + cx * cx + (cy + 0.5) * (cy + 0.5), Q = f * f + cx * cx + (cy - 0.5) * (cy - 0.5);
  const double n = st[S_CNT];
  o[PF_USMFIT_COL_ROLL] = (float)(th[0] * r2d);
  o[PF_USMFIT_COL_PITCH] = (float)(th[1] * r2d);
  o[PF_USMFIT_COL_VFOV] = (float)(2.0 * atan(0.5 / f) * r2d);
  o[PF_USMFIT_COL_REL_FOCAL] = (float)f;
  o[PF_USMFIT_COL_GENERAL_VFOV] = (float)(acos(fmin(fmax((P + Q - 1.0) / (2.0 * sqrt(P * Q)), -1.0), 1.0)) * r2d);
  o[PF_USMFIT_COL_REL_CX] = (float)cx;
  o[PF_USMFIT_COL_REL_CY] = (float)cy;
  o[PF_USMFIT_COL_RMS_UP] = (float)sqrt(st[S_UP2] / n);
  o[PF_USMFIT_COL_RMS_LAT] = (float)sqrt(st[S_LAT2] / n);
  o[PF_USMFIT_COL_COST] = (float)st[S_COST];
  o[PF_USMFIT_COL_ITERATIONS] = (float)fmax(st[S_NEV] - 1.0, 0.0);
  o[PF_USMFIT_COL_CONVERGED] = st[S_CONV] == 1.0 ? 1.f : 0.f;
  o[PF_USMFIT_COL_VALID_PIXELS] = (float)n;
  o[PF_USMFIT_COL_XI] = (float)th[5];
}

// one residual row into the sums: Jacobian row m.d * scale (0 where the model is undefined), residual r, weight w
template <int NP>
__device__ __forceinline__ void add_row(float* acc, const Dual<NP>& m, bool ok, float scale, float w, float r) {
  using R = Rec<NP>;
  float j[NP];
#pragma unroll
  for (int k = 0; k < NP; ++k) j[k] = ok ? m.d[k] * scale : 0.f;
  int t = 0;
#pragma unroll
  for (int i = 0; i < NP; ++i) {
    const float a = w * j[i];
#pragma unroll
    for (int jj = i; jj < NP; ++jj, ++t) acc[t] = fmaf(a, j[jj], acc[t]);
    acc[R::G + i] = fmaf(a, r, acc[R::G + i]);
  }
}

// The up and the latitude contributions of a pixel go into the sums one after the other, so that one set of duals is live.
template <int NP>
__device__ __forceinline__ void accum_pixel(const UsmModel<Dual<NP>>& m, float col, float row, float pux, float puy, float plat, const FitParams& prm,
                                            float* acc) {
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

}  // namespace

// ---------------------------------------------------------------- init: one wave per image
// The centre ray is (0, 0, 1) for every xi, so roll from the up vector and pitch from the latitude at the image centre as in
// the pinhole fit (4 x 4 pixels); xi = 0; f from the best of 16 vFoV candidates in [15, 150] deg by the cost on a 32 x 32
// subsample.  With fb.init: the caller's [6] parameters instead.
__global__ __launch_bounds__(64) void usmfit_init_kernel(const FitBatch fb, const FitParams prm) {
  const int img = blockIdx.x, lane = threadIdx.x;
  if (img >= fb.n) return;
  const int H = fb.H[img], W = fb.W[img];
  const long n = (long)H * W;
  const float* up = fb.up[img];
  const float* lat = fb.lat[img];
  double* st = fb.state + (long)img * USMFIT_STATE;
  double th[NTH];
  if (fb.init) {
    for (int k = 0; k < NTH; ++k) th[k] = (double)fb.init[img * NTH + k];
  } else {
    float sx = 0.f, sy = 0.f, sl = 0.f, cu = 0.f, cl = 0.f;
    if (lane < 16) {
      const int row = H / 2 - 2 + (lane >> 2), col = W / 2 - 2 + (lane & 3);
      const long i = (long)row * W + col;
      const float ux = up[i], uy = up[n + i], l = lat[i];
      if (isfinite(ux) && isfinite(uy)) { sx = ux; sy = uy; cu = 1.f; }
      if (isfinite(l)) { sl = l; cl = 1.f; }
    }
    sx = wave_sum(sx); sy = wave_sum(sy); sl = wave_sum(sl); cu = wave_sum(cu); cl = wave_sum(cl);
    th[0] = cu > 0.f ? atan2(-(double)sx, -(double)sy) : 0.0;
    th[1] = cl > 0.f ? (double)(sl / cl) * (kPi / 180.0) : 0.0;
    th[2] = 1.0;
    th[3] = th[4] = th[5] = 0.0;
    clamp_theta(th);
    // the 32 x 32 subsample, 16 pixels per lane, loaded once for all candidates
    float sux[16], suy[16], sla[16];
    int srow[16], scol[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const int s = lane + 64 * j;
      srow[j] = min((int)(((s >> 5) + 0.5f) * (float)H / 32.f), H - 1);
      scol[j] = min((int)(((s & 31) + 0.5f) * (float)W / 32.f), W - 1);
      const long i = (long)srow[j] * W + scol[j];
      sux[j] = up[i];
      suy[j] = up[n + i];
      sla[j] = lat[i];
    }
    float best = INFINITY;
    for (int c = 0; c < 16; ++c) {
      const double vfov = (15.0 + 9.0 * c) * (kPi / 180.0);
      const float f = (float)(0.5 / tan(0.5 * vfov));
      const UsmModel<float> m((float)th[0], (float)th[1], f, 0.f, 0.f, 0.f, H, W);
      float cost = 0.f;
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const float pux = sux[j], puy = suy[j], pl = sla[j];
        if (!(isfinite(pux) && isfinite(puy) && isfinite(pl))) continue;
        float x, y, rho2, disc, ux, uy, l, w, rho;
        bool ok;
        m.centre_point((float)scol[j], (float)srow[j], x, y);
        m.disc_at(x, y, rho2, disc);
        m.up_at(x, y, rho2, disc, ux, uy, ok);
        const float rx = (ux - pux) * kRad2Deg, ry = (uy - puy) * kRad2Deg;
        if (ok) {
          loss_of(sqrtf(rx * rx + ry * ry), prm.loss, prm.huber_delta, &w, &rho);
          cost += prm.w_up * rho;
        }
        m.linspace_point((float)scol[j], (float)srow[j], x, y);
        m.disc_at(x, y, rho2, disc);
        m.lat_at(x, y, rho2, disc, l, ok);
        if (ok) {
          loss_of(fabsf(l - pl), prm.loss, prm.huber_delta, &w, &rho);
          cost += prm.w_lat * rho;
        }
      }
      cost = wave_sum(cost);
      if (cost < best) { best = cost; th[2] = (double)f; }
    }
  }
  clamp_theta(th);
  if (lane == 0) {
    for (int k = 0; k < NTH; ++k) { st[S_CUR + k] = th[k]; st[S_TRIAL + k] = th[k]; }
    st[S_COST] = INFINITY;
    st[S_LAMBDA] = 1e-3;
    st[S_NEV] = 0.0;
    st[S_CONV] = 0.0;
    st[S_UP2] = st[S_LAT2] = st[S_CNT] = 0.0;
    write_out(fb.out + (long)img * PF_USMFIT_COLS, st);
  }
}

// ---------------------------------------------------------------- accumulate: grid (blocks per image) x (images), 256 threads
template <int NP>
__global__ __launch_bounds__(256) void usmfit_accum_kernel(const FitBatch fb, const FitParams prm) {
  using R = Rec<NP>;
  const int img = blockIdx.y, tid = threadIdx.x;
  if (img >= fb.n || (int)blockIdx.x >= fb.nblk[img]) return;
  const double* st = fb.state + (long)img * USMFIT_STATE;
  if (st[S_CONV] != 0.0) return;
  const int H = fb.H[img], W = fb.W[img];
  const long n = (long)H * W;
  const float* up = fb.up[img];
  const float* lat = fb.lat[img];
  const UsmModel<Dual<NP>> m = model_at<NP>(st + S_TRIAL, H, W);
  float acc[R::NV];
#pragma unroll
  for (int k = 0; k < R::NV; ++k) acc[k] = 0.f;
  // chunks of 4 consecutive pixels; 16-byte loads when all three planes are 16-byte aligned
  const bool vec = (n & 3) == 0 && ((reinterpret_cast<uintptr_t>(up) | reinterpret_cast<uintptr_t>(lat)) & 15) == 0;
  const long nchunk = (n + 3) >> 2, stride = (long)fb.nblk[img] * 256;
  for (long q = (long)blockIdx.x * 256 + tid; q < nchunk; q += stride) {
    const long p0 = q << 2;
    float vx[4], vy[4], vl[4];
    if (vec) {
      const float4 a = *reinterpret_cast<const float4*>(up + p0);
      const float4 b = *reinterpret_cast<const float4*>(up + n + p0);
      const float4 c = *reinterpret_cast<const float4*>(lat + p0);
      vx[0] = a.x; vx[1] = a.y; vx[2] = a.z; vx[3] = a.w;
      vy[0] = b.x; vy[1] = b.y; vy[2] = b.z; vy[3] = b.w;
      vl[0] = c.x; vl[1] = c.y; vl[2] = c.z; vl[3] = c.w;
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const bool in = p0 + k < n;
        vx[k] = in ? up[p0 + k] : NAN;
        vy[k] = in ? up[n + p0 + k] : NAN;
        vl[k] = in ? lat[p0 + k] : NAN;
      }
    }
    int row = (int)(p0 / W), col = (int)(p0 - (long)row * W);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      accum_pixel<NP>(m, (float)col, (float)row, vx[k], vy[k], vl[k], prm, acc);
      if (++col == W) { col = 0; ++row; }
    }
  }
  // wave sums in fp32, then the 4 waves in fp64 in a fixed order
  __shared__ double red[4][R::NV];
  const int wave = tid >> 6, lane = tid & 63;
#pragma unroll
  for (int k = 0; k < R::NV; ++k) {
    const float s = wave_sum(acc[k]);
    if (lane == 0) red[wave][k] = (double)s;
  }
  __syncthreads();
  if (tid < R::NV) {
    double* part = fb.part[img] + (long)blockIdx.x * USMFIT_REC;
    part[tid] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
  }
}

// ---------------------------------------------------------------- solve: one wave per image
// The accept / reject rule, damping and stopping rule of fit_solve_kernel (fit_camera.hip), over the free parameters of theta.
template <int NP>
__global__ __launch_bounds__(64) void usmfit_solve_kernel(const FitBatch fb) {
  using R = Rec<NP>;
  const int img = blockIdx.x, lane = threadIdx.x;
  if (img >= fb.n) return;
  double* st = fb.state + (long)img * USMFIT_STATE;
  if (st[S_CONV] != 0.0) return;
  __shared__ double sum[R::NV];
  if (lane < R::NV) {
    // 8 loads in flight, added in block order
    const double* part = fb.part[img] + lane;
    const int nb = fb.nblk[img];
    double s = 0.0;
    for (int b0 = 0; b0 < nb; b0 += 8) {
      double v[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) v[k] = b0 + k < nb ? part[(long)(b0 + k) * USMFIT_REC] : 0.0;
#pragma unroll
      for (int k = 0; k < 8; ++k) s += v[k];
    }
    sum[lane] = s;
  }
  __syncthreads();
  if (lane != 0) return;
  const double cost_t = sum[R::COST], cost_c = st[S_COST];
  const int nev = (int)st[S_NEV];
  double lambda = st[S_LAMBDA];
  double conv = 0.0;
  if (isfinite(cost_t) && (nev == 0 || cost_t < cost_c)) {  // accept the trial
    for (int k = 0; k < NTH; ++k) st[S_CUR + k] = st[S_TRIAL + k];
    for (int k = 0; k < R::NH + NP; ++k) st[S_HG + k] = sum[k];
    st[S_COST] = cost_t;
    st[S_UP2] = sum[R::UP2];
    st[S_LAT2] = sum[R::LAT2];
    st[S_CNT] = sum[R::CNT];
    if (nev > 0) {
      if (cost_c - cost_t <= 1e-10 * cost_c) conv = 1.0;
      lambda = fmax(lambda * 0.1, 1e-12);
    }
    if (cost_t == 0.0) conv = 1.0;
  } else if (nev == 0) {
    conv = 2.0;  // no finite cost at the start (no valid pixel): the output row keeps the start parameters
    st[S_CNT] = sum[R::CNT];
  } else {  // reject: more damping, same linearisation
    lambda *= 10.0;
    if (lambda > 1e16) conv = 1.0;
  }
  st[S_NEV] = (double)(nev + 1);
  if (conv == 0.0) {
    // (H + lambda diag(H)) delta = -g by Cholesky in fp64
    double A[NP][NP], b[NP];
    const double* hg = st + S_HG;
    int t = 0;
#pragma unroll
    for (int i = 0; i < NP; ++i)
#pragma unroll
      for (int j = i; j < NP; ++j) { A[i][j] = hg[t]; A[j][i] = hg[t]; ++t; }
#pragma unroll
    for (int i = 0; i < NP; ++i) { A[i][i] *= 1.0 + lambda; b[i] = -hg[R::NH + i]; }
    bool pd = true;
#pragma unroll
    for (int j = 0; j < NP; ++j) {
      double d = A[j][j];
#pragma unroll
      for (int k = 0; k < j; ++k) d -= A[j][k] * A[j][k];
      pd = pd && d > 0.0;
      d = sqrt(fmax(d, 1e-300));
      A[j][j] = d;
#pragma unroll
      for (int i = j + 1; i < NP; ++i) {
        double v = A[i][j];
#pragma unroll
        for (int k = 0; k < j; ++k) v -= A[i][k] * A[j][k];
        A[i][j] = v / d;
      }
    }
    if (!pd) {
      conv = 1.0;  // singular normal equations: the data determine no step
    } else {
#pragma unroll
      for (int i = 0; i < NP; ++i) {
        double v = b[i];
#pragma unroll
        for (int k = 0; k < i; ++k) v -= A[i][k] * b[k];
        b[i] = v / A[i][i];
      }
#pragma unroll
      for (int i = NP - 1; i >= 0; --i) {
        double v = b[i];
#pragma unroll
        for (int k = i + 1; k < NP; ++k) v -= A[k][i] * b[k];
        b[i] = v / A[i][i];
      }
      double th[NTH];
      for (int k = 0; k < NTH; ++k) th[k] = st[S_CUR + k];
#pragma unroll
      for (int k = 0; k < NP; ++k) th[theta_of<NP>(k)] += b[k];
      clamp_theta(th);
      double step = 0.0;
      for (int k = 0; k < NTH; ++k) {
        step = fmax(step, fabs(th[k] - st[S_CUR + k]));
        st[S_TRIAL + k] = th[k];
      }
      if (step < 1e-9) conv = 1.0;
    }
  }
  st[S_LAMBDA] = lambda;
  st[S_CONV] = conv;
  write_out(fb.out + (long)img * PF_USMFIT_COLS, st);
}

// ---------------------------------------------------------------- theta -> fields
// One thread per 4 consecutive pixels of the flattened image.  xi == 0: pinhole_fields_at, the bits of pf_fields_from_params;
// otherwise pf_pano_crop's label formulas in the same fp32 operations.  NaN where a point has no ray.
__global__ __launch_bounds__(256) void fields_usm_kernel(const float* __restrict__ cam, int H, int W, float* __restrict__ up, float* __restrict__ lat,
                                                         int vec) {
  const long n = (long)H * W, nchunk = (n + 3) >> 2;
  const float roll = cam[0], pitch = cam[1], f = cam[2], rcx = cam[3], rcy = cam[4], xi = cam[5];
  const PinholeFields pin = pinhole_fields_setup(roll, pitch, f, rcx, rcy, H, W);
  float sr, cr, sp, cp;
  sincosf(roll, &sr, &cr);
  sincosf(pitch, &sp, &cp);
  const float R[9] = {cr, -sr, 0.f, cp * sr, cp * cr, -sp, sp * sr, sp * cr, cp};
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
            const float r2 = x * x + y * y, disc = 1.f + (1.f - xi * xi) * r2;
            if (disc >= 0.f) {
              const float eta = (xi + sqrtf(disc)) / (1.f + r2);
              const float X0 = eta * x, X1 = eta * y, X2 = eta - xi;
              const float D = X2 + xi;
              const float s = g[2] + xi * (X0 * g[0] + X1 * g[1] + X2 * g[2]);
              const float a = g[0] * D - X0 * s, b = g[1] * D - X1 * s;
              const float in = 1.f / sqrtf(a * a + b * b);
              ux[k] = a * in;
              uy[k] = b * in;
            }
          }
          {
            const float x = ((float)col * sx - Cx) / F, y = ((float)row * sy - Cy) / F;
            const float r2 = x * x + y * y, disc = 1.f + (1.f - xi * xi) * r2;
            if (disc >= 0.f) {
              const float eta = (xi + sqrtf(disc)) / (1.f + r2);
              const float X0 = eta * x, X1 = eta * y, X2 = eta - xi;
              const float xw = R[0] * X0 + R[1] * X1 + R[2] * X2;
              const float yw = R[3] * X0 + R[4] * X1 + R[5] * X2;
              const float zw = R[6] * X0 + R[7] * X1 + R[8] * X2;
              la[k] = -atan2f(yw, sqrtf(xw * xw + zw * zw)) * kRad2Deg;
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

void launch_usmfit_init(const FitBatch& fb, const FitParams& prm, hipStream_t s) {
  hipLaunchKernelGGL(usmfit_init_kernel, dim3(fb.n), dim3(64), 0, s, fb, prm);
}

void launch_usmfit_iteration(const FitBatch& fb, const FitParams& prm, hipStream_t s) {
  int mx = 1;
  for (int k = 0; k < fb.n; ++k) mx = std::max(mx, fb.nblk[k]);
  if (prm.free_pp) {
    hipLaunchKernelGGL(usmfit_accum_kernel<6>, dim3(mx, fb.n), dim3(256), 0, s, fb, prm);
    hipLaunchKernelGGL(usmfit_solve_kernel<6>, dim3(fb.n), dim3(64), 0, s, fb);
  } else {
    hipLaunchKernelGGL(usmfit_accum_kernel<4>, dim3(mx, fb.n), dim3(256), 0, s, fb, prm);
    hipLaunchKernelGGL(usmfit_solve_kernel<4>, dim3(fb.n), dim3(64), 0, s, fb);
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
