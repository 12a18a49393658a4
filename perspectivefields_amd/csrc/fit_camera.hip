// Perspective fields -> camera parameters: a batched per-image Levenberg-Marquardt fit of the model of
// pf_fields_from_params (include/pf_hip.h pf_fit_camera).  VALU and memory bound, no MFMA.
//   fit_init_kernel    one wave per image: start parameters (or a copy of the caller's), state reset
//   fit_accum_kernel   grid (blocks per image) x (images): model + Jacobian per pixel by forward-mode dual numbers,
//                      upper triangle of J^T W J, J^T W r, cost and the rms sums per block -> one partial record per block
//                      (no atomics: the result is the same on every run and does not depend on the batch an image is in)
//   fit_solve_kernel   one wave per image: partials summed in a fixed order in fp64, LM accept / reject, damped
//                      Cholesky solve in fp64, next trial parameters, per-image convergence flag, output row
#include <math.h>

#include <algorithm>

#include "../../include/pf_hip.h"
#include "fit_dual.h"
#include "pf_kernels.h"

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

// per-block record (FIT_REC doubles): [0, NH) upper triangle of J^T W J row by row, [NH, NH + NP) J^T W r, then the cost,
// sum |r_up|^2, sum r_lat^2 and the valid pixels
template <int NP>
struct Rec {
  static constexpr int NH = NP * (NP + 1) / 2;
  static constexpr int G = NH, COST = NH + NP, UP2 = COST + 1, LAT2 = COST + 2, CNT = COST + 3, NV = COST + 4;
};
static_assert(Rec<5>::NV <= FIT_REC, "record too small");

// the parameters as duals: derivative k of parameter k for k < NP, constants beyond
template <int NP>
__device__ __forceinline__ CamModel<Dual<NP>> model_at(const double* th, int H, int W) {
  return CamModel<Dual<NP>>(dvar<NP>((float)th[0], 0), dvar<NP>((float)th[1], 1), dvar<NP>((float)th[2], 2), dvar<NP>((float)th[3], 3),
                            dvar<NP>((float)th[4], 4), H, W);
}

template <int NP>
__device__ __forceinline__ void accum_pixel(const CamModel<Dual<NP>>& m, float col, float row, float pux, float puy, float plat, const FitParams& prm,
                                            float* acc) {
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

// state of one image (FIT_STATE doubles)
enum : int {
  S_CUR = 0,     // [5] accepted parameters
  S_TRIAL = 5,   // [5] parameters the next accumulate pass evaluates
  S_COST = 10,   // cost at S_CUR
  S_LAMBDA = 11,
  S_NEV = 12,    // evaluations so far
  S_CONV = 13,   // 0: running; 1: converged; 2: no finite cost at the start.  Accumulate and solve return at once when != 0
  S_UP2 = 14, S_LAT2 = 15, S_CNT = 16,  // rms sums and valid pixels at S_CUR
  S_HG = 17,     // [NH + NP] J^T W J and J^T W r at S_CUR
  S_END = S_HG + 20
};
static_assert(S_END <= FIT_STATE, "state too small");

constexpr double kPi = 3.14159265358979323846;
constexpr double kPitchMax = 89.9 * kPi / 180.0, kFocalMin = 1e-3;

__device__ __forceinline__ void clamp_theta(double* th) {
  th[1] = fmin(fmax(th[1], -kPitchMax), kPitchMax);
  th[2] = fmax(th[2], kFocalMin);
}

__device__ void write_out(float* o, const double* st) {
  const double r2d = 180.0 / kPi;
  const double* th = st + S_CUR;
  const double f = th[2], cx = th[3], cy = th[4];
  const double P = f * f + cx * cx + (cy + 0.5) * (cy + 0.5), Q = f * f + cx * cx + (cy - 0.5) * (cy - 0.5);
  const double n = st[S_CNT];
  o[PF_FIT_COL_ROLL] = (float)(th[0] * r2d);
  o[PF_FIT_COL_PITCH] = (float)(th[1] * r2d);
  o[PF_FIT_COL_VFOV] = (float)(2.0 * atan(0.5 / f) * r2d);
  o[PF_FIT_COL_REL_FOCAL] = (float)f;
  o[PF_FIT_COL_GENERAL_VFOV] = (float)(acos(fmin(fmax((P + Q - 1.0) / (2.0 * sqrt(P * Q)), -1.0), 1.0)) * r2d);
  o[PF_FIT_COL_REL_CX] = (float)cx;
  o[PF_FIT_COL_REL_CY] = (float)cy;
  o[PF_FIT_COL_RMS_UP] = (float)sqrt(st[S_UP2] / n);
  o[PF_FIT_COL_RMS_LAT] = (float)sqrt(st[S_LAT2] / n);
  o[PF_FIT_COL_COST] = (float)st[S_COST];
  o[PF_FIT_COL_ITERATIONS] = (float)fmax(st[S_NEV] - 1.0, 0.0);
  o[PF_FIT_COL_CONVERGED] = st[S_CONV] == 1.0 ? 1.f : 0.f;
  o[PF_FIT_COL_VALID_PIXELS] = (float)n;
}

}  // namespace

// ---------------------------------------------------------------- init: one wave per image
// roll from the up vector and pitch from the latitude at the image centre (there u = (-sin r, -cos r) and lat = pitch
// whatever the other parameters), averaged over the 4 x 4 pixels around it; f from the best of 16 vFoV candidates in
// [15, 150] deg by the cost on a 32 x 32 subsample.  With fb.init: the caller's parameters instead.
__global__ __launch_bounds__(64) void fit_init_kernel(const FitBatch fb, const FitParams prm) {
  const int img = blockIdx.x, lane = threadIdx.x;
  if (img >= fb.n) return;
  const int H = fb.H[img], W = fb.W[img];
  const long n = (long)H * W;
  const float* up = fb.up[img];
  const float* lat = fb.lat[img];
  double* st = fb.state + (long)img * FIT_STATE;
  double th[5];
  if (fb.init) {
    for (int k = 0; k < 5; ++k) th[k] = (double)fb.init[img * 5 + k];
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
    th[3] = th[4] = 0.0;
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
      const CamModel<float> m((float)th[0], (float)th[1], f, 0.f, 0.f, H, W);
      float cost = 0.f;
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const float pux = sux[j], puy = suy[j], pl = sla[j];
        if (!(isfinite(pux) && isfinite(puy) && isfinite(pl))) continue;
        float ux, uy, l, w, rho;
        bool ok_up, ok_lat;
        m.eval((float)scol[j], (float)srow[j], ux, uy, l, ok_up, ok_lat);
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
      cost = wave_sum(cost);
      if (cost < best) { best = cost; th[2] = (double)f; }
    }
  }
  clamp_theta(th);
  if (lane == 0) {
    for (int k = 0; k < 5; ++k) { st[S_CUR + k] = th[k]; st[S_TRIAL + k] = th[k]; }
    st[S_COST] = INFINITY;
    st[S_LAMBDA] = 1e-3;
    st[S_NEV] = 0.0;
    st[S_CONV] = 0.0;
    st[S_UP2] = st[S_LAT2] = st[S_CNT] = 0.0;
    write_out(fb.out + (long)img * PF_FIT_COLS, st);
  }
}

// ---------------------------------------------------------------- accumulate: grid (blocks per image) x (images), 256 threads
template <int NP>
__global__ __launch_bounds__(256) void fit_accum_kernel(const FitBatch fb, const FitParams prm) {
  using R = Rec<NP>;
  const int img = blockIdx.y, tid = threadIdx.x;
  if (img >= fb.n || (int)blockIdx.x >= fb.nblk[img]) return;
  const double* st = fb.state + (long)img * FIT_STATE;
  if (st[S_CONV] != 0.0) return;
  const int H = fb.H[img], W = fb.W[img];
  const long n = (long)H * W;
  const float* up = fb.up[img];
  const float* lat = fb.lat[img];
  const CamModel<Dual<NP>> m = model_at<NP>(st + S_TRIAL, H, W);
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
    double* part = fb.part[img] + (long)blockIdx.x * FIT_REC;
    part[tid] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
  }
}

// ---------------------------------------------------------------- solve: one wave per image
template <int NP>
__global__ __launch_bounds__(64) void fit_solve_kernel(const FitBatch fb) {
  using R = Rec<NP>;
  const int img = blockIdx.x, lane = threadIdx.x;
  if (img >= fb.n) return;
  double* st = fb.state + (long)img * FIT_STATE;
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
      for (int k = 0; k < 8; ++k) v[k] = b0 + k < nb ? part[(long)(b0 + k) * FIT_REC] : 0.0;
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
    for (int k = 0; k < 5; ++k) st[S_CUR + k] = st[S_TRIAL + k];
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
      double th[5];
      for (int k = 0; k < 5; ++k) th[k] = st[S_CUR + k];
      for (int k = 0; k < NP; ++k) th[k] += b[k];
      clamp_theta(th);
      double step = 0.0;
      for (int k = 0; k < 5; ++k) {
        step = fmax(step, fabs(th[k] - st[S_CUR + k]));
        st[S_TRIAL + k] = th[k];
      }
      if (step < 1e-9) conv = 1.0;
    }
  }
  st[S_LAMBDA] = lambda;
  st[S_CONV] = conv;
  write_out(fb.out + (long)img * PF_FIT_COLS, st);
}

int fit_blocks_per_image(int H, int W) {
  const long n = (long)H * W;
  return (int)std::min<long>(std::max<long>((n + 4095) / 4096, 1), 256);
}

void launch_fit_init(const FitBatch& fb, const FitParams& prm, hipStream_t s) {
  hipLaunchKernelGGL(fit_init_kernel, dim3(fb.n), dim3(64), 0, s, fb, prm);
}

void launch_fit_iteration(const FitBatch& fb, const FitParams& prm, hipStream_t s) {
  int mx = 1;
  for (int k = 0; k < fb.n; ++k) mx = std::max(mx, fb.nblk[k]);
  if (prm.free_pp) {
    hipLaunchKernelGGL(fit_accum_kernel<5>, dim3(mx, fb.n), dim3(256), 0, s, fb, prm);
    hipLaunchKernelGGL(fit_solve_kernel<5>, dim3(fb.n), dim3(64), 0, s, fb);
  } else {
    hipLaunchKernelGGL(fit_accum_kernel<3>, dim3(mx, fb.n), dim3(256), 0, s, fb, prm);
    hipLaunchKernelGGL(fit_solve_kernel<3>, dim3(fb.n), dim3(64), 0, s, fb);
  }
}

}  // namespace pf
