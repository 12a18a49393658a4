// Relative yaw of camera views of one centre (include/pf_hip.h pf_yaw_moments): for ordered pairs (a, b) of views and a list of
// candidate turns, the six moments from which the zero-mean normalised cross-correlation of the two pictures on their overlap follows.  VALU and
// memory bound, no MFMA, no atomics, no inline assembly; every offset is 64-bit.
//   yaw_luminance_kernel<T>  grid (blocks of 256 pixels) x (views of the launch).  L = 0.299 c0 + 0.587 c1 + 0.114 c2 - c of every pixel as an fp32
//                            plane: each view is converted once, whatever number of pairs it is in, and a tap of the moments pass is one float.
//   yaw_moments_kernel       grid (tiles) x (pairs of the launch) x (candidate chunks), 64 threads.  A block owns (pair, tile of <= 1024 samples of b,
//                            chunk of 64 candidates).  Lane 0 puts the constants of a and b in LDS; the block puts (W, y) of the tile's samples in
//                            LDS, 16 bytes each, so the ray of b is computed once per block and not once per candidate.  Then one lane owns one
//                            candidate: cos and sin of its turn and six fp32 sums in registers, a walk over the tile in sample order (every lane
//                            reads the same LDS address: a broadcast), rotate, test, project, sample.  Neighbouring lanes are neighbouring
//                            candidates, so their taps lie close together in a.  No cross-lane reduction, no barrier per candidate.  The six sums
//                            go to part[tile][candidate][6] as three 8-byte stores.
//   yaw_sum_kernel           one thread per (pair, candidate): the tiles' records added in tile order in fp64 -> moments[pair][candidate][6].
// A store pass and a sum pass, so the bits depend on the pair's two views, their cameras, the candidate and the stride only: not on the launch, the
// other pairs or the way the candidates are chunked.
// Model (the contract; tests/test_yaw_align_ref.py states it in fp64).  Cameras are pf_reproject's without the yaw.  Samples of (a, b) at stride s: the
// pixels of b with row % s == 0 and col % s == 0, in row-major order.
//   X_b = usm_ray((col + 1/2 - Cx_b) / F_b, (row + 1/2 - Cy_b) / F_b, xi_b); a pixel without a ray is no sample.  W = R_b X_b
//   X_a = R_a^T Y(D) W for the candidate D = yaw_b - yaw_a (pf_reproject's M with a as the source at yaw 0 and b as the destination at yaw D)
//   visible iff X_a.z > z_min(xi_a); (p, q) = F_a (X_a.x, X_a.y) / (X_a.z + xi_a |X_a|) + (Cx_a, Cy_a)
//   covered iff visible and p > 0, Ws_a - p > 0, q > 0, Hs_a - q > 0: positive comparisons, so a NaN covers nothing and issues no load
//   y = L_b at the pixel, x = L_a bilinear at (p - 1/2, q - 1/2) with clamped taps (gather.h sample_clamped_plane)
//   moments over the covered samples: n, sum x, sum y, sum x^2, sum y^2, sum xy
// A sample without a ray, or of a view with non-finite parameters, is stored as NaN and fails the first comparison for every candidate.
#include <math.h>
#include <stdint.h>

#include <algorithm>

#include "../../include/pf_hip.h"
#include "cam_model.h"
#include "gather.h"

namespace pf {

namespace {

struct YawConsts {
  float RaT[9];  // world -> camera a, row major
  float Rb[9];   // camera b -> world
  float Fa, Cxa, Cya, xia, zmin, wmax, hmax;
  float invFb, Cxb, Cyb, xib;
};

}  // namespace

template <typename T>
__global__ __launch_bounds__(256) void yaw_luminance_kernel(YawLum yl) {
  const int v = blockIdx.y;
  const size_t npx = (size_t)yl.src.H[v] * yl.src.W[v];
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= npx) return;
  const T* __restrict__ src = static_cast<const T*>(yl.src.p[v]);
  yl.out[v][i] = 0.299f * texel(src, 3 * i) + 0.587f * texel(src, 3 * i + 1) + 0.114f * texel(src, 3 * i + 2) - yl.c;
}

__global__ __launch_bounds__(YawBatch::CHUNK) void yaw_moments_kernel(YawBatch yb) {
  __shared__ YawConsts cc;
  __shared__ float4 tile[YawBatch::TILE];
  const YawPair& pr = yb.pr[blockIdx.y];
  const int t = blockIdx.x;
  if (t >= pr.tiles) return;  // the whole block
  const int Hb = pr.Hb, Wb = pr.Wb, Ha = pr.Ha, Wa = pr.Wa, stride = yb.stride;
  if (threadIdx.x == 0) {
    const float* ca = yb.cam + (size_t)pr.a * 6;
    const float* cb = yb.cam + (size_t)pr.b * 6;
    float Ra[9];
    cam_rotation(ca[0], ca[1], Ra);
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) cc.RaT[3 * i + j] = Ra[3 * j + i];
    cam_rotation(cb[0], cb[1], cc.Rb);
    cc.Fa = ca[2] * (float)Ha;
    cc.Cxa = (ca[3] + 0.5f) * (float)Wa;
    cc.Cya = (ca[4] + 0.5f) * (float)Ha;
    cc.xia = ca[5];
    cc.zmin = usm_z_min(ca[5]);
    cc.wmax = (float)Wa;
    cc.hmax = (float)Ha;
    cc.invFb = 1.f / (cb[2] * (float)Hb);
    cc.Cxb = (cb[3] + 0.5f) * (float)Wb;
    cc.Cyb = (cb[4] + 0.5f) * (float)Hb;
    cc.xib = cb[5];
  }
  __syncthreads();
  const int cols = (Wb + stride - 1) / stride, rows = (Hb + stride - 1) / stride;  // samples across and down
  const int total = rows * cols;                                                   // < 2^31: checked on the host
  const int s0 = t * YawBatch::TILE, cnt = min(total - s0, (int)YawBatch::TILE);
  const float* __restrict__ Lb = pr.Lb;
  const float nan = __builtin_nanf("");
  for (int i = threadIdx.x; i < cnt; i += YawBatch::CHUNK) {
    const int sr = (s0 + i) / cols, sc = (s0 + i) - sr * cols;
    const int row = sr * stride, col = sc * stride;  // inside b: sr < rows, sc < cols
    float X[3], Wd[3] = {nan, nan, nan};
    if (usm_ray(((float)col + 0.5f - cc.Cxb) * cc.invFb, ((float)row + 0.5f - cc.Cyb) * cc.invFb, cc.xib, X)) to_world(cc.Rb, X, Wd);
    tile[i] = make_float4(Wd[0], Wd[1], Wd[2], Lb[(size_t)row * Wb + col]);
  }
  __syncthreads();

  const int k = blockIdx.z * YawBatch::CHUNK + threadIdx.x;
  if (k >= yb.n_cand) return;  // after the last barrier
  float sd, cd;
  sincosf(yb.cand[k], &sd, &cd);
  const float* __restrict__ La = pr.La;
  const float Fa = cc.Fa, Cxa = cc.Cxa, Cya = cc.Cya, xia = cc.xia, zmin = cc.zmin, wmax = cc.wmax, hmax = cc.hmax;
  float M[9];
#pragma unroll
  for (int i = 0; i < 9; ++i) M[i] = cc.RaT[i];
  float n = 0.f, sx = 0.f, sy = 0.f, sxx = 0.f, syy = 0.f, sxy = 0.f;
  for (int i = 0; i < cnt; ++i) {
    const float4 w = tile[i];
    const float V[3] = {cd * w.x + sd * w.z, w.y, cd * w.z - sd * w.x};  // Y(D) W
    float Xa[3];
    to_world(M, V, Xa);
    if (!(Xa[2] > zmin)) continue;
    float xs, ys;
    usm_project(Xa, xia, &xs, &ys);
    const float p = Fa * xs + Cxa, q = Fa * ys + Cya;
    const float rp = wmax - p, rq = hmax - q;
    if (!(p > 0.f && rp > 0.f && q > 0.f && rq > 0.f)) continue;  // false for NaN and infinities: no load without a point inside a
    const float x = sample_clamped_plane(La, Ha, Wa, p - 0.5f, q - 0.5f), y = w.w;
    n += 1.f;
    sx += x;
    sy += y;
    sxx = fmaf(x, x, sxx);
    syy = fmaf(y, y, syy);
    sxy = fmaf(x, y, sxy);
  }
  float2* __restrict__ out = reinterpret_cast<float2*>(yb.part + ((size_t)(pr.tile0 + (unsigned)t) * yb.n_cand + k) * 6);
  out[0] = make_float2(n, sx);
  out[1] = make_float2(sy, sxx);
  out[2] = make_float2(syy, sxy);
}

__global__ __launch_bounds__(256) void yaw_sum_kernel(YawBatch yb) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= yb.n_cand) return;
  const YawPair& pr = yb.pr[blockIdx.y];
  double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int t = 0; t < pr.tiles; ++t) {
    const float2* __restrict__ in = reinterpret_cast<const float2*>(yb.part + ((size_t)(pr.tile0 + (unsigned)t) * yb.n_cand + k) * 6);
    const float2 a = in[0], b = in[1], c = in[2];
    acc[0] += (double)a.x; acc[1] += (double)a.y;
    acc[2] += (double)b.x; acc[3] += (double)b.y;
    acc[4] += (double)c.x; acc[5] += (double)c.y;
  }
  double2* __restrict__ out = reinterpret_cast<double2*>(yb.moments + ((size_t)blockIdx.y * yb.n_cand + k) * 6);
  out[0] = make_double2(acc[0], acc[1]);
  out[1] = make_double2(acc[2], acc[3]);
  out[2] = make_double2(acc[4], acc[5]);
}

void launch_yaw_luminance(const YawLum& yl, int dtype, hipStream_t s) {
  size_t npx = 0;
  for (int v = 0; v < yl.n; ++v) npx = std::max(npx, (size_t)yl.src.H[v] * yl.src.W[v]);
  const dim3 grid((unsigned)((npx + 255) / 256), (unsigned)yl.n), block(256);
  if (dtype == PF_PANO_U8) hipLaunchKernelGGL(yaw_luminance_kernel<uint8_t>, grid, block, 0, s, yl);
  else hipLaunchKernelGGL(yaw_luminance_kernel<float>, grid, block, 0, s, yl);
}

void launch_yaw_moments(const YawBatch& yb, hipStream_t s) {
  const dim3 grid((unsigned)yb.max_tiles, (unsigned)yb.n, (unsigned)((yb.n_cand + YawBatch::CHUNK - 1) / YawBatch::CHUNK)), block(YawBatch::CHUNK);
  hipLaunchKernelGGL(yaw_moments_kernel, grid, block, 0, s, yb);
}

void launch_yaw_sum(const YawBatch& yb, hipStream_t s) {
  const dim3 grid((unsigned)((yb.n_cand + 255) / 256), (unsigned)yb.n), block(256);
  hipLaunchKernelGGL(yaw_sum_kernel, grid, block, 0, s, yb);
}

}  // namespace pf
