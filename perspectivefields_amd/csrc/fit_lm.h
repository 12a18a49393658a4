// The Levenberg-Marquardt driver of the camera fits (fit_camera.hip: pinhole, fit_camera_usm.hip: Unified Spherical Model; DESIGN.md
// sections 10, 14 and 15): everything that does not depend on the camera model, once.
//   fit_init_kernel<Fit>        one wave per image: start parameters (or a copy of the caller's), state reset
//   fit_accum_kernel<Fit, NP>   grid (blocks per image) x (images): model + Jacobian per pixel by forward-mode dual numbers,
//                               upper triangle of J^T W J, J^T W r, cost and the rms sums per block -> one partial record per block
//                               (no atomics: the result is the same on every run and does not depend on the batch an image is in)
//   fit_solve_kernel<Fit, NP>   one wave per image: partials summed in a fixed order in fp64, LM accept / reject, damped
//                               Cholesky solve in fp64, next trial parameters, per-image convergence flag, output row
// A model is a traits type Fit in namespace pf (it is part of the kernels' names) with
//   NTH, STATE, REC, COLS       parameters in theta; doubles of one image's state and of one partial record; floats of an output row
//   theta_of<NP>(k)             place in theta of free parameter k of the NP-parameter fit
//   clamp_theta(th)             theta back into the model's range
//   model_at<NP>(th, H, W)      the model over Dual<NP>: derivative k of free parameter k, constants for the held parameters
//   accum_pixel<NP>(m, col, row, pux, puy, plat, prm, acc)   one pixel into the block's fp32 sums, laid out as Rec<NP>
//   start_model(th, f, H, W)    the model over float at (th[0], th[1], f) and zeros: a candidate of the start search
//   start_cost(m, col, row, pux, puy, plat, prm, cost)       one pixel's cost at a candidate, added to cost term by term
// The per-pixel accumulation stays with the model on purpose: the two models add their residual rows in different fp32 orders.
#pragma once

#include <math.h>
#include <stdint.h>

#include <algorithm>

#include "../../include/pf_hip.h"
#include "fit_dual.h"
#include "pf_kernels.h"

namespace pf {

// Internal to the including unit, like fit_dual.h.  The kernels below have external names and use these, so every <Fit, NP> must be
// instantiated in ONE unit only: the one that defines Fit and instantiates its launcher pair.
namespace {

// per-block record (Fit::REC doubles): [0, NH) upper triangle of J^T W J row by row, [NH, NH + NP) J^T W r, then the cost,
// sum |r_up|^2, sum r_lat^2 and the valid pixels
template <int NP>
struct Rec {
  static constexpr int NH = NP * (NP + 1) / 2;
  static constexpr int G = NH, COST = NH + NP, UP2 = COST + 1, LAT2 = COST + 2, CNT = COST + 3, NV = COST + 4;
};

// state of one image (Fit::STATE doubles)
template <class Fit>
struct St {
  static constexpr int CUR = 0,                 // [NTH] accepted parameters
                       TRIAL = Fit::NTH,        // [NTH] parameters the next accumulate pass evaluates
                       COST = 2 * Fit::NTH,     // cost at CUR
                       LAMBDA = COST + 1,
                       NEV = COST + 2,          // evaluations so far
                       CONV = COST + 3,         // 0: running; 1: converged; 2: no finite cost at the start.  Accumulate and solve return at once when != 0
                       UP2 = COST + 4, LAT2 = COST + 5, CNT = COST + 6,  // rms sums and valid pixels at CUR
                       HG = COST + 7,           // [NH + NP] J^T W J and J^T W r at CUR
                       END = HG + Rec<Fit::NTH>::NH + Fit::NTH;
  static_assert(END <= Fit::STATE, "state too small");
  static_assert(Rec<Fit::NTH>::NV <= Fit::REC, "record too small");
};

constexpr double kPi = 3.14159265358979323846;
constexpr double kPitchMax = 89.9 * kPi / 180.0, kFocalMin = 1e-3;

// the thirteen columns that both row formats share
static_assert(PF_USMFIT_COL_ROLL == PF_FIT_COL_ROLL && PF_USMFIT_COL_PITCH == PF_FIT_COL_PITCH && PF_USMFIT_COL_VFOV == PF_FIT_COL_VFOV &&
                  PF_USMFIT_COL_REL_FOCAL == PF_FIT_COL_REL_FOCAL && PF_USMFIT_COL_GENERAL_VFOV == PF_FIT_COL_GENERAL_VFOV &&
                  PF_USMFIT_COL_REL_CX == PF_FIT_COL_REL_CX && PF_USMFIT_COL_REL_CY == PF_FIT_COL_REL_CY && PF_USMFIT_COL_RMS_UP == PF_FIT_COL_RMS_UP &&
                  PF_USMFIT_COL_RMS_LAT == PF_FIT_COL_RMS_LAT && PF_USMFIT_COL_COST == PF_FIT_COL_COST &&
                  PF_USMFIT_COL_ITERATIONS == PF_FIT_COL_ITERATIONS && PF_USMFIT_COL_CONVERGED == PF_FIT_COL_CONVERGED &&
                  PF_USMFIT_COL_VALID_PIXELS == PF_FIT_COL_VALID_PIXELS && PF_USMFIT_COL_XI == PF_FIT_COLS && PF_USMFIT_COLS == PF_FIT_COLS + 1,
              "the USM output row is the pinhole row, then xi");

template <class Fit>
__device__ void write_out(float* o, const double* st) {
  using S = St<Fit>;
  const double r2d = 180.0 / kPi;
  const double* th = st + S::CUR;
  const double f = th[2], cx = th[3], cy = th[4];
  const double P = f * f + cx * cx + (cy + 0.5) * (cy + 0.5), Q = f * f + cx * cx + (cy - 0.5) * (cy - 0.5);
  const double n = st[S::CNT];
  o[PF_FIT_COL_ROLL] = (float)(th[0] * r2d);
  o[PF_FIT_COL_PITCH] = (float)(th[1] * r2d);
  o[PF_FIT_COL_VFOV] = (float)(2.0 * atan(0.5 / f) * r2d);
  o[PF_FIT_COL_REL_FOCAL] = (float)f;
  o[PF_FIT_COL_GENERAL_VFOV] = (float)(acos(fmin(fmax((P + Q - 1.0) / (2.0 * sqrt(P * Q)), -1.0), 1.0)) * r2d);
  o[PF_FIT_COL_REL_CX] = (float)cx;
  o[PF_FIT_COL_REL_CY] = (float)cy;
  o[PF_FIT_COL_RMS_UP] = (float)sqrt(st[S::UP2] / n);
  o[PF_FIT_COL_RMS_LAT] = (float)sqrt(st[S::LAT2] / n);
  o[PF_FIT_COL_COST] = (float)st[S::COST];
  o[PF_FIT_COL_ITERATIONS] = (float)fmax(st[S::NEV] - 1.0, 0.0);
  o[PF_FIT_COL_CONVERGED] = st[S::CONV] == 1.0 ? 1.f : 0.f;
  o[PF_FIT_COL_VALID_PIXELS] = (float)n;
  if constexpr (Fit::NTH == 6) o[PF_USMFIT_COL_XI] = (float)th[5];
}

}  // namespace

// ---------------------------------------------------------------- init: one wave per image
// roll from the up vector and pitch from the latitude at the image centre (there u = (-sin r, -cos r) and lat = pitch
// whatever the other parameters), averaged over the 4 x 4 pixels around it; f from the best of 16 vFoV candidates in
// [15, 150] deg by the cost on a 32 x 32 subsample; zeros beyond.  With fb.init: the caller's [NTH] parameters instead.
template <class Fit>
__global__ __launch_bounds__(64) void fit_init_kernel(const FitBatch fb, const FitParams prm) {
  using S = St<Fit>;
  constexpr int NTH = Fit::NTH;
  const int img = blockIdx.x, lane = threadIdx.x;
  if (img >= fb.n) return;
  const int H = fb.H[img], W = fb.W[img];
  const long n = (long)H * W;
  const float* up = fb.up[img];
  const float* lat = fb.lat[img];
  double* st = fb.state + (long)img * Fit::STATE;
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
    for (int k = 3; k < NTH; ++k) th[k] = 0.0;
    Fit::clamp_theta(th);
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
      const auto m = Fit::start_model(th, f, H, W);
      float cost = 0.f;
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const float pux = sux[j], puy = suy[j], pl = sla[j];
        if (!(isfinite(pux) && isfinite(puy) && isfinite(pl))) continue;
        Fit::start_cost(m, (float)scol[j], (float)srow[j], pux, puy, pl, prm, cost);
      }
      cost = wave_sum(cost);
      if (cost < best) { best = cost; th[2] = (double)f; }
    }
  }
  Fit::clamp_theta(th);
  if (lane == 0) {
    for (int k = 0; k < NTH; ++k) { st[S::CUR + k] = th[k]; st[S::TRIAL + k] = th[k]; }
    st[S::COST] = INFINITY;
    st[S::LAMBDA] = 1e-3;
    st[S::NEV] = 0.0;
    st[S::CONV] = 0.0;
    st[S::UP2] = st[S::LAT2] = st[S::CNT] = 0.0;
    write_out<Fit>(fb.out + (long)img * Fit::COLS, st);
  }
}

// ---------------------------------------------------------------- accumulate: grid (blocks per image) x (images), 256 threads
template <class Fit, int NP>
__global__ __launch_bounds__(256) void fit_accum_kernel(const FitBatch fb, const FitParams prm) {
  using R = Rec<NP>;
  using S = St<Fit>;
  const int img = blockIdx.y, tid = threadIdx.x;
  if (img >= fb.n || (int)blockIdx.x >= fb.nblk[img]) return;
  const double* st = fb.state + (long)img * Fit::STATE;
  if (st[S::CONV] != 0.0) return;
  const int H = fb.H[img], W = fb.W[img];
  const long n = (long)H * W;
  const float* up = fb.up[img];
  const float* lat = fb.lat[img];
  const auto m = Fit::template model_at<NP>(st + S::TRIAL, H, W);
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
      Fit::template accum_pixel<NP>(m, (float)col, (float)row, vx[k], vy[k], vl[k], prm, acc);
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
    double* part = fb.part[img] + (long)blockIdx.x * Fit::REC;
    part[tid] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
  }
}

// ---------------------------------------------------------------- solve: one wave per image
template <class Fit, int NP>
__global__ __launch_bounds__(64) void fit_solve_kernel(const FitBatch fb) {
  using R = Rec<NP>;
  using S = St<Fit>;
  constexpr int NTH = Fit::NTH;
  const int img = blockIdx.x, lane = threadIdx.x;
  if (img >= fb.n) return;
  double* st = fb.state + (long)img * Fit::STATE;
  if (st[S::CONV] != 0.0) return;
  __shared__ double sum[R::NV];
  if (lane < R::NV) {
    // 8 loads in flight, added in block order
    const double* part = fb.part[img] + lane;
    const int nb = fb.nblk[img];
    double s = 0.0;
    for (int b0 = 0; b0 < nb; b0 += 8) {
      double v[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) v[k] = b0 + k < nb ? part[(long)(b0 + k) * Fit::REC] : 0.0;
#pragma unroll
      for (int k = 0; k < 8; ++k) s += v[k];
    }
    sum[lane] = s;
  }
  __syncthreads();
  if (lane != 0) return;
  const double cost_t = sum[R::COST], cost_c = st[S::COST];
  const int nev = (int)st[S::NEV];
  double lambda = st[S::LAMBDA];
  double conv = 0.0;
  if (isfinite(cost_t) && (nev == 0 || cost_t < cost_c)) {  // accept the trial
    for (int k = 0; k < NTH; ++k) st[S::CUR + k] = st[S::TRIAL + k];
    for (int k = 0; k < R::NH + NP; ++k) st[S::HG + k] = sum[k];
    st[S::COST] = cost_t;
    st[S::UP2] = sum[R::UP2];
    st[S::LAT2] = sum[R::LAT2];
    st[S::CNT] = sum[R::CNT];
    if (nev > 0) {
      if (cost_c - cost_t <= 1e-10 * cost_c) conv = 1.0;
      lambda = fmax(lambda * 0.1, 1e-12);
    }
    if (cost_t == 0.0) conv = 1.0;
  } else if (nev == 0) {
    conv = 2.0;  // no finite cost at the start (no valid pixel): the output row keeps the start parameters
    st[S::CNT] = sum[R::CNT];
  } else {  // reject: more damping, same linearisation
    lambda *= 10.0;
    if (lambda > 1e16) conv = 1.0;
  }
  st[S::NEV] = (double)(nev + 1);
  if (conv == 0.0) {
    // (H + lambda diag(H)) delta = -g by Cholesky in fp64
    double A[NP][NP], b[NP];
    const double* hg = st + S::HG;
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
      for (int k = 0; k < NTH; ++k) th[k] = st[S::CUR + k];
#pragma unroll
      for (int k = 0; k < NP; ++k) th[Fit::template theta_of<NP>(k)] += b[k];
      Fit::clamp_theta(th);
      double step = 0.0;
      for (int k = 0; k < NTH; ++k) {
        step = fmax(step, fabs(th[k] - st[S::CUR + k]));
        st[S::TRIAL + k] = th[k];
      }
      if (step < 1e-9) conv = 1.0;
    }
  }
  st[S::LAMBDA] = lambda;
  st[S::CONV] = conv;
  write_out<Fit>(fb.out + (long)img * Fit::COLS, st);
}

// ---------------------------------------------------------------- launchers (declared in pf_kernels.h; each model's unit instantiates its pair)
template <class Fit>
void launch_fit_init(const FitBatch& fb, const FitParams& prm, hipStream_t s) {
  hipLaunchKernelGGL(fit_init_kernel<Fit>, dim3(fb.n), dim3(64), 0, s, fb, prm);
}

// FitParams::free_pp: all NTH parameters are free; otherwise NTH - 2, with rel_cx / rel_cy held at their start values
template <class Fit>
void launch_fit_iteration(const FitBatch& fb, const FitParams& prm, hipStream_t s) {
  int mx = 1;
  for (int k = 0; k < fb.n; ++k) mx = std::max(mx, fb.nblk[k]);
  if (prm.free_pp) {
    hipLaunchKernelGGL((fit_accum_kernel<Fit, Fit::NTH>), dim3(mx, fb.n), dim3(256), 0, s, fb, prm);
    hipLaunchKernelGGL((fit_solve_kernel<Fit, Fit::NTH>), dim3(fb.n), dim3(64), 0, s, fb);
  } else {
    hipLaunchKernelGGL((fit_accum_kernel<Fit, Fit::NTH - 2>), dim3(mx, fb.n), dim3(256), 0, s, fb, prm);
    hipLaunchKernelGGL((fit_solve_kernel<Fit, Fit::NTH - 2>), dim3(fb.n), dim3(64), 0, s, fb);
  }
}

}  // namespace pf
