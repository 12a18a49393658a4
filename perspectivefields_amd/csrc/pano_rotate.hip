// Equirectangular panorama -> rotated equirectangular panorama, and the perspective fields of a panoramic camera (include/pf_hip.h pf_pano_rotate /
// pf_pano_fields): the third image gather of gather.h.  VALU and memory bound, no MFMA, no atomics.
//   pano_rotate_kernel<T, LABELS>  grid (tiles per output) x (outputs of the group), 256 threads.  Each block owns a compact 2-D tile of output pixels
//                                  (GatherDims::tpr threads x 4 pixels across, 256 / tpr rows; 64 x 16 as launched).  Lane 0 computes the output's
//                                  constants (A, g, the two pixel scales) into LDS once per block; a thread takes the sine and cosine of its row's
//                                  latitude once and of its four longitudes.
//   pano_fields_kernel             the labels alone, no source: the same per-pixel function (rot_pixel), so the same bits as the LABELS path.
// Model (the contract; tests/test_pano_rotate_ref.py states it in fp64):
//   lon = ((col + 1/2) / W - 1/2) 2 pi, lat = (1/2 - (row + 1/2) / H) pi, D = (cos lat sin lon, -sin lat, cos lat cos lon)
//   Q = Y(yaw) R_pitch(p) R_roll(r), A = Q or (inverse) Q^T; X = A D
//   lat_s = -atan2(X.y, hypot(X.x, X.z)), lon_s = atan2(X.x, X.z); u = (lon_s / 2 pi + 1/2) Ws - 1/2, v = (1/2 - lat_s / pi) Hs - 1/2
//   image = `sample` (gather.h: bilinear, columns wrap, rows clamp) of the source at (u, v); uint8 through round_u8
//   labels: latitude = lat_s in degrees; g = A^T (0, -1, 0), a = g . e_lon, b = g . e_lat with e_lon = (cos lon, 0, -sin lon),
//       e_lat = (-sin lat sin lon, -cos lat, -sin lat cos lon) (so t = g - (g . D) D = a e_lon + b e_lat, |t|^2 = a^2 + b^2),
//       up ~ (W / (2 pi) a / cos lat, -H / pi b) normalised; NaN where a^2 + b^2 < PF_PANO_UP_MIN_T2
//   non-finite roll, pitch or yaw: image 0, labels NaN, no load is issued (as pano_crop's pixels without a ray)
// Every rounding step of the setup and of rot_pixel is spelled out (contraction off, fmaf where a fused step is meant): the bits must not depend on
// the kernel they are inlined into.
#include <math.h>
#include <stdint.h>

#include "../../include/pf_hip.h"
#include "cam_model.h"
#include "gather.h"

namespace pf {

namespace {

constexpr float kInv2Pi = 0.15915494309189535f, kInvPi = 0.3183098861837907f, kPi = 3.14159265358979323846f, kRad2Deg = 57.29577951308232f;

struct RotConsts {
  float A[9];    // output direction -> source (world) direction, row major
  float g[3];    // world up (0, -1, 0) in the output camera's coordinates: A^T (0, -1, 0)
  float kx, ky;  // W / (2 pi), H / pi: pixels per radian of longitude and of latitude
  int ok;        // 0: a non-finite angle
};

// rot = {roll, pitch, yaw} radians
__device__ __forceinline__ void rot_setup(const float* rot, int inverse, int H, int W, RotConsts* c) {
#pragma clang fp contract(off)
  const float roll = rot[0], pitch = rot[1], yaw = rot[2];
  pano_rotation(rot, inverse, c->A);
  c->g[0] = -c->A[3]; c->g[1] = -c->A[4]; c->g[2] = -c->A[5];
  c->kx = (float)W * kInv2Pi;
  c->ky = (float)H * kInvPi;
  c->ok = (isfinite(roll) && isfinite(pitch) && isfinite(yaw)) ? 1 : 0;
}

__device__ __forceinline__ void row_sincos(int row, int H, float* sl, float* cl) {
#pragma clang fp contract(off)
  sincosf((0.5f - ((float)row + 0.5f) / (float)H) * kPi, sl, cl);
}

struct RotPixel {
  float ts, tl;      // longitude and latitude of the source point as fractions: lon_s / 2 pi + 1/2 and 1/2 - lat_s / pi
  float ux, uy, lat; // the labels (LABELS only)
};

// pixel (row, col) of an H x W output whose row has latitude sine / cosine (sl, cl)
template <bool LABELS>
__device__ __forceinline__ RotPixel rot_pixel(const RotConsts& c, float sl, float cl, int col, int W) {
#pragma clang fp contract(off)
  float so, co;
  sincosf((((float)col + 0.5f) / (float)W - 0.5f) * (2.f * kPi), &so, &co);
  const float D0 = cl * so, D1 = -sl, D2 = cl * co;
  const float X0 = fmaf(c.A[2], D2, fmaf(c.A[1], D1, c.A[0] * D0));
  const float X1 = fmaf(c.A[5], D2, fmaf(c.A[4], D1, c.A[3] * D0));
  const float X2 = fmaf(c.A[8], D2, fmaf(c.A[7], D1, c.A[6] * D0));
  const float nlat = atan2f(X1, sqrtf(fmaf(X0, X0, X2 * X2)));  // -lat_s
  RotPixel o;
  o.ts = fmaf(atan2f(X0, X2), kInv2Pi, 0.5f);
  o.tl = fmaf(nlat, kInvPi, 0.5f);
  if (LABELS) {
    o.lat = -nlat * kRad2Deg;
    const float a = fmaf(c.g[0], co, -(c.g[2] * so));
    const float b = -fmaf(c.g[1], cl, sl * fmaf(c.g[0], so, c.g[2] * co));
    const float t2 = fmaf(a, a, b * b);
    const float px = c.kx * a / cl, py = -(c.ky * b);
    const float n = sqrtf(fmaf(px, px, py * py));  // divisions, not a reciprocal: an upright camera gives (0, -1) exactly
    const bool has = t2 >= PF_PANO_UP_MIN_T2;
    o.ux = has ? px / n : __builtin_nanf("");
    o.uy = has ? py / n : __builtin_nanf("");
  }
  return o;
}

// the labels of 4 adjacent pixels of output `out_i`: 16-byte vectors with `vec`, otherwise scalars for the pixels inside the row
__device__ __forceinline__ void store_labels(float* up, float* lat, int vec, int out_i, int H, int W, int row, int col0, const float* ux, const float* uy,
                                             const float* la) {
  const size_t npx = (size_t)H * W, l = (size_t)out_i * npx + (size_t)row * W + col0;
  if (vec) {
    *reinterpret_cast<float4*>(up + l + (size_t)out_i * npx) = make_float4(ux[0], ux[1], ux[2], ux[3]);
    *reinterpret_cast<float4*>(up + l + (size_t)out_i * npx + npx) = make_float4(uy[0], uy[1], uy[2], uy[3]);
    *reinterpret_cast<float4*>(lat + l) = make_float4(la[0], la[1], la[2], la[3]);
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (col0 + k >= W) break;
      up[l + k + (size_t)out_i * npx] = ux[k];
      up[l + k + (size_t)out_i * npx + npx] = uy[k];
      lat[l + k] = la[k];
    }
  }
}

}  // namespace

template <typename T, bool LABELS>
__global__ __launch_bounds__(256) void pano_rotate_kernel(PanoRotBatch rb) {
  __shared__ RotConsts rc;
  const int out_i = blockIdx.y;
  const int H = rb.d.H, W = rb.d.W;
  if (threadIdx.x == 0) rot_setup(rb.rot + (size_t)out_i * 3, rb.inverse, H, W, &rc);
  __syncthreads();
  const int tpr = rb.d.tpr;  // threads per tile row; the tile is (4 tpr) x (256 / tpr) pixels
  const int tile_x = blockIdx.x % rb.d.tiles_x, tile_y = blockIdx.x / rb.d.tiles_x;
  const int row = tile_y * (256 / tpr) + threadIdx.x / tpr;
  const int col0 = tile_x * 4 * tpr + (threadIdx.x % tpr) * 4;
  if (row >= H || col0 >= W) return;
  const T* __restrict__ src = static_cast<const T*>(rb.src.p[out_i]);
  const int Hs = rb.src.H[out_i], Ws = rb.src.W[out_i];
  float sl, cl;
  row_sincos(row, H, &sl, &cl);

  float img[4][3], ux[4], uy[4], lat[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int col = col0 + k;
    img[k][0] = img[k][1] = img[k][2] = 0.f;
    ux[k] = uy[k] = lat[k] = __builtin_nanf("");
    if (col >= W || !rc.ok) continue;
    const RotPixel o = rot_pixel<LABELS>(rc, sl, cl, col, W);
    sample(src, Hs, Ws, fmaf(o.ts, (float)Ws, -0.5f), fmaf(o.tl, (float)Hs, -0.5f), img[k]);
    if (LABELS) { ux[k] = o.ux; uy[k] = o.uy; lat[k] = o.lat; }
  }

  const size_t npx = (size_t)H * W, pix = (size_t)out_i * npx + (size_t)row * W + col0;
  T* __restrict__ out = static_cast<T*>(rb.img) + pix * 3;
  if (rb.d.vec) {  // W % 4 == 0 and aligned outputs: the 4 pixels are 12 / 48 image bytes
    if constexpr (sizeof(T) == 1) {
      uint32_t w[3] = {0u, 0u, 0u};
#pragma unroll
      for (int e = 0; e < 12; ++e) w[e / 4] |= round_u8(img[e / 3][e % 3]) << (8 * (e % 4));
      uint32_t* o = reinterpret_cast<uint32_t*>(out);
      o[0] = w[0]; o[1] = w[1]; o[2] = w[2];
    } else {
      store_rgb4(out, img);
    }
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (col0 + k >= W) break;
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) store_px(out + 3 * k + ch, img[k][ch]);
    }
  }
  if (LABELS) store_labels(rb.up, rb.lat, rb.d.vec, out_i, H, W, row, col0, ux, uy, lat);
}

__global__ __launch_bounds__(256) void pano_fields_kernel(PanoFieldsBatch fb) {
  __shared__ RotConsts rc;
  const int out_i = blockIdx.y;
  const int H = fb.d.H, W = fb.d.W;
  if (threadIdx.x == 0) rot_setup(fb.rot + (size_t)out_i * 3, fb.inverse, H, W, &rc);
  __syncthreads();
  const int tpr = fb.d.tpr;  // threads per tile row; the tile is (4 tpr) x (256 / tpr) pixels
  const int tile_x = blockIdx.x % fb.d.tiles_x, tile_y = blockIdx.x / fb.d.tiles_x;
  const int row = tile_y * (256 / tpr) + threadIdx.x / tpr;
  const int col0 = tile_x * 4 * tpr + (threadIdx.x % tpr) * 4;
  if (row >= H || col0 >= W) return;
  float sl, cl;
  row_sincos(row, H, &sl, &cl);
  float ux[4], uy[4], lat[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    ux[k] = uy[k] = lat[k] = __builtin_nanf("");
    if (col0 + k >= W || !rc.ok) continue;
    const RotPixel o = rot_pixel<true>(rc, sl, cl, col0 + k, W);
    ux[k] = o.ux; uy[k] = o.uy; lat[k] = o.lat;
  }
  store_labels(fb.up, fb.lat, fb.d.vec, out_i, H, W, row, col0, ux, uy, lat);
}

void launch_pano_rotate(const PanoRotBatch& rb, int dtype, hipStream_t s) {
  const dim3 grid((unsigned)(rb.d.tiles_x * rb.d.tiles_y), (unsigned)rb.d.n), block(256);
  const bool labels = rb.up != nullptr;
  if (dtype == PF_PANO_U8) {
    if (labels) hipLaunchKernelGGL((pano_rotate_kernel<uint8_t, true>), grid, block, 0, s, rb);
    else hipLaunchKernelGGL((pano_rotate_kernel<uint8_t, false>), grid, block, 0, s, rb);
  } else {
    if (labels) hipLaunchKernelGGL((pano_rotate_kernel<float, true>), grid, block, 0, s, rb);
    else hipLaunchKernelGGL((pano_rotate_kernel<float, false>), grid, block, 0, s, rb);
  }
}

void launch_pano_fields(const PanoFieldsBatch& fb, hipStream_t s) {
  const dim3 grid((unsigned)(fb.d.tiles_x * fb.d.tiles_y), (unsigned)fb.d.n), block(256);
  hipLaunchKernelGGL(pano_fields_kernel, grid, block, 0, s, fb);
}

}  // namespace pf
