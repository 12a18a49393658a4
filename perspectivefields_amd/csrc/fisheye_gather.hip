// Fisheye and dual-fisheye frames as a source: camera views and equirectangular panoramas out of one or two lenses of a frame (include/pf_hip.h
// pf_fisheye_crop / pf_fisheye_to_pano): two more image gathers of gather.h.  VALU and memory bound, no MFMA, no atomics, no
// workspace.
//   fisheye_crop_kernel<T>     views of cameras (roll, pitch, yaw, rel_focal, rel_cx, rel_cy, xi): pf_pano_crop's ray C, world direction D = Qc C with
//                              Qc = Y(yaw) R_pitch R_roll, the frame's value in D
//   fisheye_to_pano_kernel<T>  panoramas: pf_pano_rotate's pixel -> direction D0 and D = A D0, the frame's value in D
//       both: grid (tiles per output) x (outputs of the group), 256 threads, a 64 x 16 pixel tile, 4 adjacent pixels of a row per thread, lane 0
//       computes the output's constants into LDS once per block (per lens M = Ql^T Qc or Ql^T A, so that a sample goes from the camera ray or the
//       panorama direction into the lens in one 3 x 3 product, and the lens' intrinsics), 64-bit offsets, vector stores with GatherDims::vec.
//       `samples` = S is a run-time loop as in gather_ss.hip: the fp32 sum of the valid sub-samples at offsets (i + 1/2) / S, i-major then j, from
//       -0, divided by their count; `fill` without one.  The projection kind is a block-uniform run-time switch.
// The value of a frame in a direction (the contract; tests/test_fisheye_ref.py states it in fp64), per lens l = 0, 1 in that order:
//   angle    X = M v, h = sqrt(fma(X0, X0, X1 X1)), t = atan2f(h, X2)
//   point    td = t * fma(t2, fma(t2, fma(t2, fma(t2, k4, k3), k2), k1), 1) with t2 = t t;  r = F rho(td), rho = td | 2 sinf(td / 2) | 2 tanf(td / 2);
//            s = r / h;  (a, b) = (fma(s, X0, Cx), fma(s, X1, Cy)), (Cx, Cy) where h == 0
//   covered  the lens is on (its 12 entries finite, theta_max > 0) and theta_max - t > 0 and 0 <= a <= Ws and 0 <= b <= Hs: positive comparisons
//            only, so that a NaN covers nothing and no load is issued without a point inside the frame
//   weight   w = fminf((theta_max - t) / band, 1) for band > 0, else 1
//   colour   c = sample_clamped at (a - 1/2, b - 1/2)
//   S = S + w, C = fma(w, c, C) from 0; valid iff S > 0, value C / S.
// Every rounding step of the setup and of the per-sample function is spelled out (contraction off, fmaf where a fused step is meant).
#include <math.h>
#include <stdint.h>

#include "../../include/pf_hip.h"
#include "cam_model.h"
#include "gather.h"

namespace pf {

namespace {

constexpr float kPi = 3.14159265358979323846f;

// Q = Y(yaw) R_pitch(pitch) R_roll(roll), row major: pano_rotate.hip's lines
__device__ __forceinline__ void world_rotation(float roll, float pitch, float yaw, float* Q) {
#pragma clang fp contract(off)
  float R[9], sy, cy;
  cam_rotation(roll, pitch, R);
  sincosf(yaw, &sy, &cy);
  for (int k = 0; k < 3; ++k) {
    Q[k] = fmaf(cy, R[k], sy * R[6 + k]);
    Q[3 + k] = R[3 + k];
    Q[6 + k] = fmaf(cy, R[6 + k], -(sy * R[k]));
  }
}

// offset of sub-sample k of S inside its pixel: 1/2 exactly at S = 1
__device__ __forceinline__ float sub_offset(int k, float fS) { return ((float)k + 0.5f) / fS; }

struct LensConsts {
  float M[9];  // camera ray or panorama direction -> lens coordinates, row major
  float F, Cx, Cy, tmax, k1, k2, k3, k4, band;
  int on;      // 0: a non-finite entry or theta_max <= 0: the lens covers nothing
};

struct FisheyeConsts {
  LensConsts lens[PF_FISHEYE_MAX_LENSES];
  float invF, Cx, Cy, xi;  // the view's camera (fisheye_crop_kernel)
  int ok;                  // 0: a non-finite camera or angle entry
};

// the constants of lens l of output out_i: M = Ql^T A for the 3 x 3 matrix A (row major) that takes the sample's vector into the world
__device__ __forceinline__ void lens_setup(const float* __restrict__ lens, const float* A, LensConsts* c) {
#pragma clang fp contract(off)
  float Q[9];
  world_rotation(lens[0], lens[1], lens[2], Q);
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) c->M[3 * i + j] = fmaf(Q[6 + i], A[6 + j], fmaf(Q[3 + i], A[3 + j], Q[i] * A[j]));
  c->F = lens[3]; c->Cx = lens[4]; c->Cy = lens[5]; c->tmax = lens[6];
  c->k1 = lens[7]; c->k2 = lens[8]; c->k3 = lens[9]; c->k4 = lens[10];
  c->band = lens[11];
  bool fin = true;
  for (int k = 0; k < PF_FISHEYE_LENS_FLOATS; ++k) fin = fin && isfinite(lens[k]);
  c->on = (fin && lens[6] > 0.f) ? 1 : 0;
}

// the frame's value in the direction whose vector is v (a camera ray or a panorama direction): false where no lens covers it
template <typename T>
__device__ __forceinline__ bool fisheye_sample(const T* __restrict__ src, int Hs, int Ws, int kind, const LensConsts* lens, float v0, float v1, float v2,
                                               float* out) {
#pragma clang fp contract(off)
  const float wmax = (float)Ws, hmax = (float)Hs;
  float S = 0.f, C[3] = {0.f, 0.f, 0.f};
#pragma unroll
  for (int l = 0; l < PF_FISHEYE_MAX_LENSES; ++l) {
    const LensConsts& c = lens[l];
    if (!c.on) continue;
    const float X0 = fmaf(c.M[2], v2, fmaf(c.M[1], v1, c.M[0] * v0));
    const float X1 = fmaf(c.M[5], v2, fmaf(c.M[4], v1, c.M[3] * v0));
    const float X2 = fmaf(c.M[8], v2, fmaf(c.M[7], v1, c.M[6] * v0));
    const float h = sqrtf(fmaf(X0, X0, X1 * X1));
    const float t = atan2f(h, X2);
    const float margin = c.tmax - t;
    if (!(margin > 0.f)) continue;
    const float t2 = t * t;
    const float td = t * fmaf(t2, fmaf(t2, fmaf(t2, fmaf(t2, c.k4, c.k3), c.k2), c.k1), 1.f);
    const float rho = kind == PF_FISHEYE_EQUIDISTANT ? td : kind == PF_FISHEYE_EQUISOLID ? 2.f * sinf(td * 0.5f) : 2.f * tanf(td * 0.5f);
    const float s = c.F * rho / h;
    const float a = h > 0.f ? fmaf(s, X0, c.Cx) : c.Cx, b = h > 0.f ? fmaf(s, X1, c.Cy) : c.Cy;
    if (!(a >= 0.f && a <= wmax && b >= 0.f && b <= hmax)) continue;  // false for NaN and infinities: no load without a point inside the frame
    const float w = c.band > 0.f ? fminf(margin / c.band, 1.f) : 1.f;
    float px[3];
    sample_clamped(src, Hs, Ws, a - 0.5f, b - 0.5f, px);
    S = S + w;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) C[ch] = fmaf(w, px[ch], C[ch]);
  }
  if (!(S > 0.f)) return false;
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) out[ch] = C[ch] / S;
  return true;
}

// the image and the mask of 4 adjacent pixels of a row, each the mean of its n summed samples (`fill` without one): 12 / 48 image bytes and 4 mask
// bytes with `vec`, otherwise store_px and single bytes for the pixels inside the row
template <typename T>
__device__ __forceinline__ void store_means(T* __restrict__ out, uint8_t* __restrict__ valid, int vec, int col0, int W, const float (*acc)[3], const int* n,
                                            float fill) {
  float img[4][3];
  uint32_t ok[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const float fn = (float)n[k];
    ok[k] = n[k] > 0 ? 1u : 0u;
#pragma unroll
    for (int c = 0; c < 3; ++c) img[k][c] = n[k] > 0 ? acc[k][c] / fn : fill;
  }
  if (vec) {
    if constexpr (sizeof(T) == 1) {
      uint32_t w[3] = {0u, 0u, 0u};
#pragma unroll
      for (int e = 0; e < 12; ++e) w[e / 4] |= round_u8(img[e / 3][e % 3]) << (8 * (e % 4));
      uint32_t* o = reinterpret_cast<uint32_t*>(out);
      o[0] = w[0]; o[1] = w[1]; o[2] = w[2];
    } else {
      store_rgb4(out, img);
    }
    if (valid) *reinterpret_cast<uint32_t*>(valid) = ok[0] | ok[1] << 8 | ok[2] << 16 | ok[3] << 24;
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (col0 + k >= W) break;
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) store_px(out + 3 * k + ch, img[k][ch]);
      if (valid) valid[k] = (uint8_t)ok[k];
    }
  }
}

}  // namespace

template <typename T>
__global__ __launch_bounds__(256) void fisheye_crop_kernel(FisheyeCropBatch fb) {
#pragma clang fp contract(off)
  __shared__ FisheyeConsts fc;
  const int out_i = blockIdx.y;
  const int H = fb.d.H, W = fb.d.W;
  if (threadIdx.x == 0) {
    const float* cam = fb.cam + (size_t)out_i * 7;
    const float roll = cam[0], pitch = cam[1], yaw = cam[2], f = cam[3], rcx = cam[4], rcy = cam[5], xi = cam[6];
    float Q[9];
    world_rotation(roll, pitch, yaw, Q);
    for (int l = 0; l < PF_FISHEYE_MAX_LENSES; ++l)
      lens_setup(fb.lens + ((size_t)out_i * PF_FISHEYE_MAX_LENSES + l) * PF_FISHEYE_LENS_FLOATS, Q, &fc.lens[l]);
    fc.invF = 1.f / (f * (float)H);
    fc.Cx = (rcx + 0.5f) * (float)W;
    fc.Cy = (rcy + 0.5f) * (float)H;
    fc.xi = xi;
    fc.ok = (isfinite(roll) && isfinite(pitch) && isfinite(yaw) && isfinite(f) && isfinite(rcx) && isfinite(rcy) && isfinite(xi)) ? 1 : 0;
  }
  __syncthreads();
  const int tpr = fb.d.tpr;  // threads per tile row; the tile is (4 tpr) x (256 / tpr) pixels
  const int tile_x = blockIdx.x % fb.d.tiles_x, tile_y = blockIdx.x / fb.d.tiles_x;
  const int row = tile_y * (256 / tpr) + threadIdx.x / tpr;
  const int col0 = tile_x * 4 * tpr + (threadIdx.x % tpr) * 4;
  if (row >= H || col0 >= W) return;
  const T* __restrict__ src = static_cast<const T*>(fb.src.p[out_i]);
  const int Hs = fb.src.H[out_i], Ws = fb.src.W[out_i];
  const int kind = fb.kind;
  const float xi = fc.xi, k1 = 1.f - xi * xi;
  const int S = fc.ok ? fb.samples : 0;  // a non-finite parameter: no sub-sample, no load
  const float fS = (float)fb.samples;

  float acc[4][3];
  int n[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    acc[k][0] = acc[k][1] = acc[k][2] = -0.f;
    n[k] = 0;
  }
  for (int i = 0; i < S; ++i) {
    const float y = ((float)row + sub_offset(i, fS) - fc.Cy) * fc.invF;
    for (int j = 0; j < S; ++j) {
      const float oj = sub_offset(j, fS);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int col = col0 + k;
        if (col >= W) continue;
        // pf_pano_crop's ray: rho^2, disc, eta, C = (eta x, eta y, eta - xi)
        const float x = ((float)col + oj - fc.Cx) * fc.invF;
        const float r2 = fmaf(x, x, y * y);
        const float disc = fmaf(k1, r2, 1.f);
        if (!(disc >= 0.f)) continue;
        const float eta = (xi + sqrtf(disc)) / (1.f + r2);
        float px[3];
        if (!fisheye_sample(src, Hs, Ws, kind, fc.lens, eta * x, eta * y, eta - xi, px)) continue;
        acc[k][0] += px[0]; acc[k][1] += px[1]; acc[k][2] += px[2];
        ++n[k];
      }
    }
  }
  const size_t pix = (size_t)out_i * ((size_t)H * W) + (size_t)row * W + col0;
  store_means(static_cast<T*>(fb.img) + pix * 3, fb.valid ? fb.valid + pix : nullptr, fb.d.vec, col0, W, acc, n, fb.fill);
}

template <typename T>
__global__ __launch_bounds__(256) void fisheye_to_pano_kernel(FisheyePanoBatch fb) {
#pragma clang fp contract(off)
  __shared__ FisheyeConsts fc;
  const int out_i = blockIdx.y;
  const int H = fb.d.H, W = fb.d.W;
  if (threadIdx.x == 0) {
    const float* rot = fb.rot + (size_t)out_i * 3;
    float Q[9], A[9];
    world_rotation(rot[0], rot[1], rot[2], Q);
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) A[3 * i + j] = fb.inverse ? Q[3 * j + i] : Q[3 * i + j];
    for (int l = 0; l < PF_FISHEYE_MAX_LENSES; ++l)
      lens_setup(fb.lens + ((size_t)out_i * PF_FISHEYE_MAX_LENSES + l) * PF_FISHEYE_LENS_FLOATS, A, &fc.lens[l]);
    fc.ok = (isfinite(rot[0]) && isfinite(rot[1]) && isfinite(rot[2])) ? 1 : 0;
  }
  __syncthreads();
  const int tpr = fb.d.tpr;  // threads per tile row; the tile is (4 tpr) x (256 / tpr) pixels
  const int tile_x = blockIdx.x % fb.d.tiles_x, tile_y = blockIdx.x / fb.d.tiles_x;
  const int row = tile_y * (256 / tpr) + threadIdx.x / tpr;
  const int col0 = tile_x * 4 * tpr + (threadIdx.x % tpr) * 4;
  if (row >= H || col0 >= W) return;
  const T* __restrict__ src = static_cast<const T*>(fb.src.p[out_i]);
  const int Hs = fb.src.H[out_i], Ws = fb.src.W[out_i];
  const int kind = fb.kind;
  const int S = fc.ok ? fb.samples : 0;  // a non-finite angle: no sub-sample, no load
  const float fS = (float)fb.samples;

  float acc[4][3];
  int n[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    acc[k][0] = acc[k][1] = acc[k][2] = -0.f;
    n[k] = 0;
  }
  for (int i = 0; i < S; ++i) {
    float sl, cl;  // pf_pano_rotate's direction of a pixel: the row's latitude once per i
    sincosf((0.5f - ((float)row + sub_offset(i, fS)) / (float)H) * kPi, &sl, &cl);
    for (int j = 0; j < S; ++j) {
      const float oj = sub_offset(j, fS);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int col = col0 + k;
        if (col >= W) continue;
        float so, co;
        sincosf((((float)col + oj) / (float)W - 0.5f) * (2.f * kPi), &so, &co);
        float px[3];
        if (!fisheye_sample(src, Hs, Ws, kind, fc.lens, cl * so, -sl, cl * co, px)) continue;
        acc[k][0] += px[0]; acc[k][1] += px[1]; acc[k][2] += px[2];
        ++n[k];
      }
    }
  }
  const size_t pix = (size_t)out_i * ((size_t)H * W) + (size_t)row * W + col0;
  store_means(static_cast<T*>(fb.img) + pix * 3, fb.valid ? fb.valid + pix : nullptr, fb.d.vec, col0, W, acc, n, fb.fill);
}

void launch_fisheye_crop(const FisheyeCropBatch& fb, int dtype, hipStream_t s) {
  const dim3 grid((unsigned)(fb.d.tiles_x * fb.d.tiles_y), (unsigned)fb.d.n), block(256);
  if (dtype == PF_PANO_U8) hipLaunchKernelGGL(fisheye_crop_kernel<uint8_t>, grid, block, 0, s, fb);
  else hipLaunchKernelGGL(fisheye_crop_kernel<float>, grid, block, 0, s, fb);
}

void launch_fisheye_to_pano(const FisheyePanoBatch& fb, int dtype, hipStream_t s) {
  const dim3 grid((unsigned)(fb.d.tiles_x * fb.d.tiles_y), (unsigned)fb.d.n), block(256);
  if (dtype == PF_PANO_U8) hipLaunchKernelGGL(fisheye_to_pano_kernel<uint8_t>, grid, block, 0, s, fb);
  else hipLaunchKernelGGL(fisheye_to_pano_kernel<float>, grid, block, 0, s, fb);
}

}  // namespace pf
