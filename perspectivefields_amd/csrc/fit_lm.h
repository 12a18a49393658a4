// The Levenberg-Marquardt driver of the camera fits (fit_camera.hip: pinhole, fit_camera_usm.hip: Unified Spherical Model,
// fit_camera_fisheye.hip: fisheye lenses; DESIGN.md sections 10, 14, 15 and 37): everything that does not depend on the camera model, once.
//   fit_init_kernel<Fit>        one wave per image: start parameters (or a copy of the caller's), state reset
//   fit_accum_kernel<Fit, NP>   grid (blocks per image) x (images): model + Jacobian per pixel by forward-mode dual numbers,
//                               upper triangle of J^T W J, J^T W r, cost and the rms sums per block -> one partial record per block
//                               (no atomics: the result is the same on every run and does not depend on the batch an image is in)
//   fit_solve_kernel<Fit, NP>   one wave per image: partials summed in a fixed order in fp64, LM accept / reject, damped
//                               Cholesky solve in fp64, next trial parameters, per-image convergence flag, output row
// The fit with intrinsics shared across the images of a camera group (pf_fit_camera_shared) keeps init and accumulate
// and replaces the solve by a pair, because a group may hold any number of images anywhere in the batch:
//   fit_shared_start_kernel<Fit>       one wave per group, after init: the group's f = exp(mean log f), cx, cy, xi = the means of its members' starts
//   fit_shared_reduce_kernel<Fit, NP>  one wave per image: the partials summed as fit_solve_kernel sums them -> rec [B][Fit::REC]
//   fit_shared_solve_kernel<Fit, NP>   one wave per group: accept / reject on the group's cost, every member's 2 x 2 (roll, pitch) block eliminated
//                                      from the damped block-arrow system, the shared NP - 2 parameters by Cholesky in fp64, back-substitution
// A model is a traits type Fit in namespace pf (it is part of the kernels' names) with
//   NTH, STATE, REC, COLS       parameters in theta; doubles of one image's state and of one partial record; floats of an output row
//   theta_of<NP>(k)             place in theta of free parameter k of the NP-parameter fit
//   clamp_theta(th)             theta back into the model's range
//   model_at<NP>(th, H, W)      the model over Dual<NP>: derivative k of free parameter k, constants for the held parameters
//   accum_pixel<NP>(m, col, row, pux, puy, plat, prm, acc)   one pixel into the block's fp32 sums, laid out as Rec<NP>
//   start_focal(c)              the focal length of candidate c = 0 ... 15 of the start search
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
                       END = HG + Rec<Fit::NTH>::NH + Fit::NTH,
                       GCONV = END;             // shared fit only: the group's flag, the same in every member (CONV of a member without a valid pixel stays 2)
  static_assert(GCONV < Fit::STATE, "state too small");
  static_assert(Rec<Fit::NTH>::NV <= Fit::REC, "record too small");
};

// one residual row into a block's sums (the models that add their rows one after the other: USM, fisheye): Jacobian row m.d * scale (0 where the model is undefined), residual r, weight w
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
  if constexpr (Fit::NTH == 7) {
    o[PF_FISHFIT_COL_K1] = (float)th[5];
    o[PF_FISHFIT_COL_K2] = (float)th[6];
    if (!(n > 0.0)) o[PF_FISHFIT_COL_CONVERGED] = 0.f;  // a cost of 0 over no pixel at all met no tolerance
  }
}

// candidate c of 16 of the start search of a camera with a vertical field of view: vFoV in [15, 150] deg
__device__ __forceinline__ float start_focal_vfov(int c) {
  const double vfov = (15.0 + 9.0 * c) * (kPi / 180.0);
  return (float)(0.5 / tan(0.5 * vfov));
}

}  // namespace

// ---------------------------------------------------------------- init: one wave per image
// roll from the up vector and pitch from the latitude at the image centre (there u = (-sin r, -cos r) and lat = pitch
// whatever the other parameters), averaged over the 4 x 4 pixels around it; f from the best of the model's 16 candidates
// (Fit::start_focal) by the cost on a 32 x 32 subsample; zeros beyond.  With fb.init: the caller's [NTH] parameters instead.
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
      const float f = Fit::start_focal(c);
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

// ================================================================ intrinsics shared across the images of a group
// place of element (i, j), i <= j, in the row-by-row upper triangle of an NP x NP matrix
template <int NP>
__device__ __forceinline__ constexpr int tri(int i, int j) { return i * NP - i * (i - 1) / 2 + (j - i); }

// ---------------------------------------------------------------- group start: one wave per group
template <class Fit>
__global__ __launch_bounds__(64) void fit_shared_start_kernel(const FitGroups fg) {
  using S = St<Fit>;
  constexpr int NTH = Fit::NTH, NS = NTH - 2;
  const int g = blockIdx.x, lane = threadIdx.x;
  if (g >= fg.n) return;
  const int i0 = fg.start[g], n = fg.size[g];
  __shared__ double red[64][NS];
  double acc[NS];
#pragma unroll
  for (int k = 0; k < NS; ++k) acc[k] = 0.0;
  for (int i = lane; i < n; i += 64) {
    const double* st = fg.state + (long)(i0 + i) * Fit::STATE;
    acc[0] += log(st[S::CUR + 2]);
#pragma unroll
    for (int k = 1; k < NS; ++k) acc[k] += st[S::CUR + 2 + k];
  }
#pragma unroll
  for (int k = 0; k < NS; ++k) red[lane][k] = acc[k];
  __syncthreads();
  // every lane adds the 64 lane sums in lane order: the same bits in all of them
  double sh[NS];
#pragma unroll
  for (int k = 0; k < NS; ++k) {
    double s = 0.0;
    for (int l = 0; l < 64; ++l) s += red[l][k];
    sh[k] = s / (double)n;
  }
  sh[0] = exp(sh[0]);
  for (int i = lane; i < n; i += 64) {
    double* st = fg.state + (long)(i0 + i) * Fit::STATE;
    double th[NTH];
    th[0] = st[S::CUR];
    th[1] = st[S::CUR + 1];
#pragma unroll
    for (int k = 0; k < NS; ++k) th[2 + k] = sh[k];
    Fit::clamp_theta(th);
    for (int k = 0; k < NTH; ++k) { st[S::CUR + k] = th[k]; st[S::TRIAL + k] = th[k]; }
    st[S::GCONV] = 0.0;
    write_out<Fit>(fg.out + (long)(i0 + i) * Fit::COLS, st);
  }
}

// ---------------------------------------------------------------- per-image reduction: one wave per image
template <class Fit, int NP>
__global__ __launch_bounds__(64) void fit_shared_reduce_kernel(const FitBatch fb, double* __restrict__ rec) {
  using R = Rec<NP>;
  using S = St<Fit>;
  const int img = blockIdx.x, lane = threadIdx.x;
  if (img >= fb.n) return;
  if (fb.state[(long)img * Fit::STATE + S::CONV] != 0.0) return;
  if (lane < R::NV) {
    // 8 loads in flight, added in block order (as fit_solve_kernel)
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
    rec[(long)img * Fit::REC + lane] = s;
  }
}

// (A + lambda diag A)^-1 of a member's (roll, pitch) block as (i00, i01, i11); false when the damped block is not positive definite
template <int NP>
__device__ __forceinline__ bool inv_own_block(const double* hg, double lambda, double* inv) {
  const double a00 = hg[tri<NP>(0, 0)] * (1.0 + lambda), a01 = hg[tri<NP>(0, 1)], a11 = hg[tri<NP>(1, 1)] * (1.0 + lambda);
  const double det = a00 * a11 - a01 * a01;
  const bool pd = a00 > 0.0 && det > 0.0;
  const double r = 1.0 / (pd ? det : 1.0);
  inv[0] = a11 * r;
  inv[1] = -(a01 * r);
  inv[2] = a00 * r;
  return pd;
}

// ---------------------------------------------------------------- shared solve: one wave per group
// Lane l owns members l, l + 64, ...  Sums over the group: per lane in member order, then over the lanes in lane order, in fp64 -- the
// bits of a group depend on nothing but its own members.  What follows a group sum is computed by every lane from the same numbers.
template <class Fit, int NP>
__global__ __launch_bounds__(64) void fit_shared_solve_kernel(const FitGroups fg) {
  using R = Rec<NP>;
  using S = St<Fit>;
  constexpr int NTH = Fit::NTH, NS = NP - 2, NT = NS * (NS + 1) / 2;
  constexpr int RT = 0, RD = NT, RB = NT + NS, RBAD = NT + 2 * NS, NRED = RBAD + 1;  // C - B^T A^-1 B, diag C, b, members with a singular block
  static_assert(NRED >= 3 && NRED <= 64, "reduction width");
  const int g = blockIdx.x, lane = threadIdx.x;
  if (g >= fg.n) return;
  const int i0 = fg.start[g], n = fg.size[g];
  double* const st0 = fg.state + (long)i0 * Fit::STATE;
  if (st0[S::GCONV] != 0.0) return;  // the whole block
  const int nev = (int)st0[S::NEV];
  double lambda = st0[S::LAMBDA];
  __shared__ double red[64][NRED];
  __shared__ double tot[NRED];

  // ---- the group's cost at the trial and at the accepted parameters; at the first evaluation, the members without a valid pixel leave
  double acc[NRED];
#pragma unroll
  for (int k = 0; k < NRED; ++k) acc[k] = 0.0;
  for (int i = lane; i < n; i += 64) {
    double* st = fg.state + (long)(i0 + i) * Fit::STATE;
    const double* rc = fg.rec + (long)(i0 + i) * Fit::REC;
    if (nev == 0 && !(rc[R::CNT] > 0.0 && isfinite(rc[R::COST]))) {
      st[S::CONV] = 2.0;
      st[S::COST] = rc[R::COST];
      st[S::CNT] = rc[R::CNT];
    }
    if (st[S::CONV] != 0.0) continue;
    acc[0] += rc[R::COST];
    acc[1] += st[S::COST];
    acc[2] += 1.0;
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) red[lane][k] = acc[k];
  __syncthreads();
  if (lane < 3) {
    double s = 0.0;
    for (int l = 0; l < 64; ++l) s += red[l][lane];
    tot[lane] = s;
  }
  __syncthreads();
  const double cost_t = tot[0], cost_c = tot[1];
  const bool any = tot[2] > 0.0;
  __syncthreads();  // tot and red are written again below
  const bool accept = any && isfinite(cost_t) && (nev == 0 || cost_t < cost_c);
  double conv = 0.0;
  if (accept) {
    if (nev > 0) {
      if (cost_c - cost_t <= 1e-10 * cost_c) conv = 1.0;
      lambda = fmax(lambda * 0.1, 1e-12);
    }
    if (cost_t == 0.0) conv = 1.0;
  } else if (nev == 0) {
    conv = 2.0;  // no member has a valid pixel: every output row keeps the start parameters
  } else {  // reject: more damping, same linearisation
    lambda *= 10.0;
    if (lambda > 1e16) conv = 1.0;
  }

  // ---- accept, then every member's (roll, pitch) block out of the damped system
#pragma unroll
  for (int k = 0; k < NRED; ++k) acc[k] = 0.0;
  for (int i = lane; i < n; i += 64) {
    double* st = fg.state + (long)(i0 + i) * Fit::STATE;
    const bool live = st[S::CONV] == 0.0;
    if (accept) {
      for (int k = 0; k < NTH; ++k) st[S::CUR + k] = st[S::TRIAL + k];  // a member without a valid pixel follows the group's shared parameters
      if (live) {
        const double* rc = fg.rec + (long)(i0 + i) * Fit::REC;
        for (int k = 0; k < R::NH + NP; ++k) st[S::HG + k] = rc[k];
        st[S::COST] = rc[R::COST];
        st[S::UP2] = rc[R::UP2];
        st[S::LAT2] = rc[R::LAT2];
        st[S::CNT] = rc[R::CNT];
      }
    }
    if (!live || conv != 0.0) continue;
    const double* hg = st + S::HG;
    double inv[3];
    if (!inv_own_block<NP>(hg, lambda, inv)) acc[RBAD] += 1.0;
    const double ga0 = hg[R::NH], ga1 = hg[R::NH + 1];
    const double v0 = inv[0] * ga0 + inv[1] * ga1, v1 = inv[1] * ga0 + inv[2] * ga1;  // A^-1 g_a
    double B0[NS], B1[NS], w0[NS], w1[NS];                                           // B, A^-1 B
#pragma unroll
    for (int k = 0; k < NS; ++k) {
      B0[k] = hg[tri<NP>(0, 2 + k)];
      B1[k] = hg[tri<NP>(1, 2 + k)];
      w0[k] = inv[0] * B0[k] + inv[1] * B1[k];
      w1[k] = inv[1] * B0[k] + inv[2] * B1[k];
    }
    int t = 0;
#pragma unroll
    for (int k = 0; k < NS; ++k) {
#pragma unroll
      for (int l = k; l < NS; ++l, ++t) acc[RT + t] += hg[tri<NP>(2 + k, 2 + l)] - (B0[k] * w0[l] + B1[k] * w1[l]);
      acc[RD + k] += hg[tri<NP>(2 + k, 2 + k)];
      acc[RB + k] += hg[R::NH + 2 + k] - (B0[k] * v0 + B1[k] * v1);
    }
  }
#pragma unroll
  for (int k = 0; k < NRED; ++k) red[lane][k] = acc[k];
  __syncthreads();
  if (lane < NRED) {
    double s = 0.0;
    for (int l = 0; l < 64; ++l) s += red[l][lane];
    tot[lane] = s;
  }
  __syncthreads();

  // ---- S delta_s = -b by Cholesky in fp64, S = sum (C - B^T A^-1 B) + lambda diag(sum C)
  double ds[NS];
#pragma unroll
  for (int k = 0; k < NS; ++k) ds[k] = 0.0;
  if (conv == 0.0) {
    double A[NS][NS];
    int t = 0;
#pragma unroll
    for (int i = 0; i < NS; ++i)
#pragma unroll
      for (int j = i; j < NS; ++j) { A[i][j] = tot[RT + t]; A[j][i] = tot[RT + t]; ++t; }
#pragma unroll
    for (int i = 0; i < NS; ++i) { A[i][i] += lambda * tot[RD + i]; ds[i] = -tot[RB + i]; }
    bool pd = tot[RBAD] == 0.0;
#pragma unroll
    for (int j = 0; j < NS; ++j) {
      double d = A[j][j];
#pragma unroll
      for (int k = 0; k < j; ++k) d -= A[j][k] * A[j][k];
      pd = pd && d > 0.0;
      d = sqrt(fmax(d, 1e-300));
      A[j][j] = d;
#pragma unroll
      for (int i = j + 1; i < NS; ++i) {
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
      for (int i = 0; i < NS; ++i) {
        double v = ds[i];
#pragma unroll
        for (int k = 0; k < i; ++k) v -= A[i][k] * ds[k];
        ds[i] = v / A[i][i];
      }
#pragma unroll
      for (int i = NS - 1; i >= 0; --i) {
        double v = ds[i];
#pragma unroll
        for (int k = i + 1; k < NS; ++k) v -= A[k][i] * ds[k];
        ds[i] = v / A[i][i];
      }
    }
  }

  // ---- back-substitution: delta_a = -A^-1 (g_a + B delta_s); next trial parameters; the group's longest step
  double step = 0.0;
  if (conv == 0.0) {
    for (int i = lane; i < n; i += 64) {
      double* st = fg.state + (long)(i0 + i) * Fit::STATE;
      const bool live = st[S::CONV] == 0.0;
      double th[NTH];
      for (int k = 0; k < NTH; ++k) th[k] = st[S::CUR + k];
      if (live) {
        const double* hg = st + S::HG;
        double inv[3];
        inv_own_block<NP>(hg, lambda, inv);
        double r0 = hg[R::NH], r1 = hg[R::NH + 1];
#pragma unroll
        for (int k = 0; k < NS; ++k) {
          r0 += hg[tri<NP>(0, 2 + k)] * ds[k];
          r1 += hg[tri<NP>(1, 2 + k)] * ds[k];
        }
        th[Fit::template theta_of<NP>(0)] -= inv[0] * r0 + inv[1] * r1;
        th[Fit::template theta_of<NP>(1)] -= inv[1] * r0 + inv[2] * r1;
      }
#pragma unroll
      for (int k = 0; k < NS; ++k) th[Fit::template theta_of<NP>(2 + k)] += ds[k];
      Fit::clamp_theta(th);
      for (int k = 0; k < NTH; ++k) {
        if (live) step = fmax(step, fabs(th[k] - st[S::CUR + k]));
        st[S::TRIAL + k] = th[k];
      }
    }
  }
  red[lane][0] = step;
  __syncthreads();
  if (conv == 0.0) {
    double m = 0.0;
    for (int l = 0; l < 64; ++l) m = fmax(m, red[l][0]);
    if (m < 1e-9) conv = 1.0;
  }

  // ---- state and output rows
  for (int i = lane; i < n; i += 64) {
    double* st = fg.state + (long)(i0 + i) * Fit::STATE;
    st[S::LAMBDA] = lambda;
    st[S::NEV] = (double)(nev + 1);
    st[S::GCONV] = conv;
    if (st[S::CONV] == 0.0) st[S::CONV] = conv;
    write_out<Fit>(fg.out + (long)(i0 + i) * Fit::COLS, st);
  }
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

template <class Fit>
void launch_fit_shared_start(const FitGroups& fg, hipStream_t s) {
  hipLaunchKernelGGL(fit_shared_start_kernel<Fit>, dim3(fg.n), dim3(64), 0, s, fg);
}

// the existing accumulate kernel, then the per-image reduction into rec (this launch group's first record)
template <class Fit>
void launch_fit_shared_accum(const FitBatch& fb, const FitParams& prm, double* rec, hipStream_t s) {
  int mx = 1;
  for (int k = 0; k < fb.n; ++k) mx = std::max(mx, fb.nblk[k]);
  if (prm.free_pp) {
    hipLaunchKernelGGL((fit_accum_kernel<Fit, Fit::NTH>), dim3(mx, fb.n), dim3(256), 0, s, fb, prm);
    hipLaunchKernelGGL((fit_shared_reduce_kernel<Fit, Fit::NTH>), dim3(fb.n), dim3(64), 0, s, fb, rec);
  } else {
    hipLaunchKernelGGL((fit_accum_kernel<Fit, Fit::NTH - 2>), dim3(mx, fb.n), dim3(256), 0, s, fb, prm);
    hipLaunchKernelGGL((fit_shared_reduce_kernel<Fit, Fit::NTH - 2>), dim3(fb.n), dim3(64), 0, s, fb, rec);
  }
}

template <class Fit>
void launch_fit_shared_solve(const FitGroups& fg, const FitParams& prm, hipStream_t s) {
  if (prm.free_pp)
    hipLaunchKernelGGL((fit_shared_solve_kernel<Fit, Fit::NTH>), dim3(fg.n), dim3(64), 0, s, fg);
  else
    hipLaunchKernelGGL((fit_shared_solve_kernel<Fit, Fit::NTH - 2>), dim3(fg.n), dim3(64), 0, s, fg);
}

}  // namespace pf
