// Equirectangular panorama -> camera views (pinhole or Unified Spherical Model) and their ground-truth perspective fields
// (include/pf_hip.h pf_pano_crop): the reference's PanoCam.get_image / crop_equi / crop_distortion and
// get_up_general / get_lat_general (utils/panocam.py) as one batched gather.  VALU and memory bound, no MFMA, no atomics.
//   pano_crop_kernel<T, LABELS>  grid (tiles per crop) x (crops of the group), 256 threads.  Each block owns a compact 2-D tile of
//                                output pixels (GatherDims::tpr threads x 4 pixels across, 256 / tpr rows; 64 x 16 as launched), so
//                                its bilinear gathers stay in a small region of the panorama.  Lane 0 computes the crop's constants (R, g, F, Cx, Cy,
//                                xi) into LDS once per block.  Every output value depends on its own crop's parameters and
//                                panorama only: the same bits in any batch and on every run.
// Model (the contract; tests/test_pano_crop_ref.py states it in fp64):
//   x = (a - Cx) / F, y = (b - Cy) / F with F = f H, Cx = (cx + 1/2) W, Cy = (cy + 1/2) H
//   ray X = (eta x, eta y, eta - xi), rho^2 = x^2 + y^2, disc = 1 + (1 - xi^2) rho^2, eta = (xi + sqrt(disc)) / (1 + rho^2);
//       disc < 0: no ray (image 0, labels NaN)
//   X_w = R_pitch(p) R_roll(r) X; lat = -atan2(X_w.y, hypot(X_w.x, X_w.z)), lon = wrap(yaw + atan2(X_w.x, X_w.z)) into [-pi, pi)
//   u = (lon / 2 pi + 1/2) Wp - 1/2, v = (1/2 - lat / pi) Hp - 1/2; bilinear, columns wrap modulo Wp, rows clamp to [0, Hp - 1]
//   image sampled at (a, b) = (col + 1/2, row + 1/2); uint8 = the fp32 value rounded half up, clamped to [0, 255]
//   labels: xi == 0 -> cam_model.h (the bits of pf_fields_from_params); otherwise up at pixel centres
//       g = R^T (0, -1, 0), D = X_z + xi, s = g_z + xi (X . g), up ~ (g_x D - X_x s, g_y D - X_y s), and lat (degrees) of the ray
//       at the linspace point (a, b) = (col W / (W - 1), row H / (H - 1)); yaw does not enter
// Loads: 3-byte uint8 and 12-byte fp32 texels are read channel by channel (every address inside the panorama, 64-bit offsets).
#include <math.h>
#include <stdint.h>

#include "../../include/pf_hip.h"
#include "cam_model.h"
#include "gather.h"

namespace pf {

namespace {

constexpr float kInv2Pi = 0.15915494309189535f, kInvPi = 0.3183098861837907f;

struct CropConsts {
  float R[9];  // camera -> world, row major
  float g[3];  // world up (0, -1, 0) in camera coordinates
  float F, invF, Cx, Cy, xi, yaw_t, sx, sy;
  PinholeFields pin;  // the xi == 0 labels
};

}  // namespace

template <typename T, bool LABELS>
__global__ __launch_bounds__(256) void pano_crop_kernel(PanoBatch pb) {
  __shared__ CropConsts cc;
  const int crop = blockIdx.y;
  const int H = pb.d.H, W = pb.d.W;
  if (threadIdx.x == 0) {
    const float* cam = pb.cam + (size_t)crop * 7;
    const float roll = cam[0], pitch = cam[1], yaw = cam[2], f = cam[3], rcx = cam[4], rcy = cam[5], xi = cam[6];
    float sr, cr, sp, cp, R[9];
    sincosf(roll, &sr, &cr);
    sincosf(pitch, &sp, &cp);
    cam_rotation(sr, cr, sp, cp, R);
    for (int k = 0; k < 9; ++k) cc.R[k] = R[k];
    cc.g[0] = -R[3]; cc.g[1] = -R[4]; cc.g[2] = -R[5];
    cc.F = f * (float)H;
    cc.invF = 1.f / cc.F;
    cc.Cx = (rcx + 0.5f) * (float)W;
    cc.Cy = (rcy + 0.5f) * (float)H;
    cc.xi = xi;
    cc.yaw_t = yaw * kInv2Pi + 0.5f;
    cc.sx = W > 1 ? (float)W / (float)(W - 1) : 0.f;
    cc.sy = H > 1 ? (float)H / (float)(H - 1) : 0.f;
    if (LABELS) cc.pin = pinhole_fields_setup(roll, pitch, f, rcx, rcy, H, W);
  }
  __syncthreads();
  const int tpr = pb.d.tpr;  // threads per tile row; the tile is (4 tpr) x (256 / tpr) pixels
  const int tile_x = blockIdx.x % pb.d.tiles_x, tile_y = blockIdx.x / pb.d.tiles_x;
  const int row = tile_y * (256 / tpr) + threadIdx.x / tpr;
  const int col0 = tile_x * 4 * tpr + (threadIdx.x % tpr) * 4;
  if (row >= H || col0 >= W) return;
  const T* __restrict__ pano = static_cast<const T*>(pb.src.p[crop]);
  const int Hp = pb.src.H[crop], Wp = pb.src.W[crop];
  const float xi = cc.xi;

  float img[4][3], ux[4], uy[4], lat[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int col = col0 + k;
    img[k][0] = img[k][1] = img[k][2] = 0.f;
    ux[k] = uy[k] = lat[k] = __builtin_nanf("");
    if (col >= W) continue;
    float X[3];
    if (usm_ray(((float)col + 0.5f - cc.Cx) * cc.invF, ((float)row + 0.5f - cc.Cy) * cc.invF, xi, X)) {
      float Xw[3];
      to_world(cc.R, X, Xw);
      float t = cc.yaw_t + atan2f(Xw[0], Xw[2]) * kInv2Pi;
      t -= floorf(t);
      const float u = t * (float)Wp - 0.5f;
      const float v = (0.5f + atan2f(Xw[1], sqrtf(Xw[0] * Xw[0] + Xw[2] * Xw[2])) * kInvPi) * (float)Hp - 0.5f;
      sample(pano, Hp, Wp, u, v, img[k]);
      if (LABELS && xi != 0.f) usm_up_of_ray(X, cc.g, xi, &ux[k], &uy[k]);
    }
    if (LABELS) {
      if (xi == 0.f) {
        const FieldsPixel o = pinhole_fields_at(cc.pin, row, col);
        ux[k] = o.ux;
        uy[k] = o.uy;
        lat[k] = o.lat;
      } else if (usm_ray(((float)col * cc.sx - cc.Cx) / cc.F, ((float)row * cc.sy - cc.Cy) / cc.F, xi, X)) {
        lat[k] = usm_lat_of_ray(X, cc.R);
      }
    }
  }

  const size_t npx = (size_t)H * W, pix = (size_t)crop * npx + (size_t)row * W + col0;
  T* __restrict__ out = static_cast<T*>(pb.img) + pix * 3;
  if (pb.d.vec) {  // W % 4 == 0 and aligned outputs: the 4 pixels are whole 16-byte label vectors and 12 / 48 image bytes
    if constexpr (sizeof(T) == 1) {
      uint32_t w[3] = {0u, 0u, 0u};
#pragma unroll
      for (int e = 0; e < 12; ++e) w[e / 4] |= round_u8(img[e / 3][e % 3]) << (8 * (e % 4));
      uint32_t* o = reinterpret_cast<uint32_t*>(out);
      o[0] = w[0]; o[1] = w[1]; o[2] = w[2];
    } else {
      store_rgb4(out, img);
    }
    if (LABELS) {
      const size_t l = (size_t)crop * npx + (size_t)row * W + col0;
      *reinterpret_cast<float4*>(pb.up + l + (size_t)crop * npx) = make_float4(ux[0], ux[1], ux[2], ux[3]);
      *reinterpret_cast<float4*>(pb.up + l + (size_t)crop * npx + npx) = make_float4(uy[0], uy[1], uy[2], uy[3]);
      *reinterpret_cast<float4*>(pb.lat + l) = make_float4(lat[0], lat[1], lat[2], lat[3]);
    }
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (col0 + k >= W) break;
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) store_px(out + 3 * k + ch, img[k][ch]);
      if (LABELS) {
        const size_t l = (size_t)crop * npx + (size_t)row * W + col0 + k;
        pb.up[l + (size_t)crop * npx] = ux[k];
        pb.up[l + (size_t)crop * npx + npx] = uy[k];
        pb.lat[l] = lat[k];
      }
    }
  }
}

void launch_pano_crop(const PanoBatch& pb, int dtype, hipStream_t s) {
  const dim3 grid((unsigned)(pb.d.tiles_x * pb.d.tiles_y), (unsigned)pb.d.n), block(256);
  const bool labels = pb.up != nullptr;
  if (dtype == PF_PANO_U8) {
    if (labels) hipLaunchKernelGGL((pano_crop_kernel<uint8_t, true>), grid, block, 0, s, pb);
    else hipLaunchKernelGGL((pano_crop_kernel<uint8_t, false>), grid, block, 0, s, pb);
  } else {
    if (labels) hipLaunchKernelGGL((pano_crop_kernel<float, true>), grid, block, 0, s, pb);
    else hipLaunchKernelGGL((pano_crop_kernel<float, false>), grid, block, 0, s, pb);
  }
}

}  // namespace pf
