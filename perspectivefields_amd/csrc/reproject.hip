// Image of one camera -> image of another camera of the same centre (include/pf_hip.h pf_reproject): upright
// rectification, undistortion of a Unified Spherical Model view, a change of focal length, principal point or size, as one batched
// gather.  VALU and memory bound, no MFMA, no atomics.
//   reproject_kernel<T, EXTRAS>  grid (tiles per output) x (outputs of the group), 256 threads.  Each block owns a compact 2-D tile of
//                                output pixels (GatherDims::tpr threads x 4 pixels across, 256 / tpr rows; 64 x 16 as launched), so its
//                                bilinear gathers stay in a small region of the source.  Lane 0 computes the output's constants (M, both
//                                intrinsics, both xi, z_min) into LDS once per block.  EXTRAS: the mask and / or the map are written.
//                                Every output value depends on its own two cameras and its own source only: the same bits in any
//                                batch and on every run.
// Model (the contract; tests/test_reproject_ref.py states it in fp64), cameras theta_d (output, H x W) and theta_s (source, Hs x Ws):
//   x = (col + 1/2 - Cx_d) / F_d, y = (row + 1/2 - Cy_d) / F_d; X_d = usm_ray(x, y, xi_d); no ray (disc < 0): invalid
//   X_s = M X_d, M = R_s^T Y(yaw_d - yaw_s) R_d, R = R_pitch R_roll, Y(t) = [[cos t, 0, sin t], [0, 1, 0], [-sin t, 0, cos t]]
//   visible iff X_s.z > z_min(xi_s) (usm_z_min); a_s = F_s X_s.x / D + Cx_s, b_s = F_s X_s.y / D + Cy_s, D = X_s.z + xi_s |X_s|
//   valid iff visible and 0 <= a_s <= Ws and 0 <= b_s <= Hs; bilinear at (a_s - 1/2, b_s - 1/2), the four taps clamped into the source
//   uint8 = the fp32 value rounded half up, clamped to [0, 255]; invalid: fill in the image, 0 in the mask; map = (a_s, b_s), NaN where not visible
// Every comparison is a positive one: a NaN or infinite coordinate (non-finite parameters) is invalid and issues no load, and the tap
// indices are clamped whatever the parameters.  Loads: channel by channel, every address inside the source, 64-bit offsets.
#include <math.h>
#include <stdint.h>

#include "../../include/pf_hip.h"
#include "cam_model.h"
#include "gather.h"

namespace pf {

namespace {

struct ReprojConsts {
  float M[9];  // destination camera -> source camera, row major
  float invFd, Cxd, Cyd, xid;
  float Fs, Cxs, Cys, xis, zmin;
};

}  // namespace

template <typename T, bool EXTRAS>
__global__ __launch_bounds__(256) void reproject_kernel(ReprojBatch rb) {
  __shared__ ReprojConsts cc;
  const int o = blockIdx.y;
  const int H = rb.d.H, W = rb.d.W;
  const int Hs = rb.src.H[o], Ws = rb.src.W[o];
  if (threadIdx.x == 0) {
    const float* cs = rb.cam_src + (size_t)o * 7;
    const float* cd = rb.cam_dst + (size_t)o * 7;
    float Rs[9], Rd[9], sy, cy;
    cam_rotation(cs[0], cs[1], Rs);
    cam_rotation(cd[0], cd[1], Rd);
    sincosf(cd[2] - cs[2], &sy, &cy);
    float Tm[9];  // Y(yaw_d - yaw_s) R_d
    for (int j = 0; j < 3; ++j) {
      Tm[j] = cy * Rd[j] + sy * Rd[6 + j];
      Tm[3 + j] = Rd[3 + j];
      Tm[6 + j] = cy * Rd[6 + j] - sy * Rd[j];
    }
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) cc.M[3 * i + j] = Rs[i] * Tm[j] + Rs[3 + i] * Tm[3 + j] + Rs[6 + i] * Tm[6 + j];
    cc.invFd = 1.f / (cd[3] * (float)H);
    cc.Cxd = (cd[4] + 0.5f) * (float)W;
    cc.Cyd = (cd[5] + 0.5f) * (float)H;
    cc.xid = cd[6];
    cc.Fs = cs[3] * (float)Hs;
    cc.Cxs = (cs[4] + 0.5f) * (float)Ws;
    cc.Cys = (cs[5] + 0.5f) * (float)Hs;
    cc.xis = cs[6];
    cc.zmin = usm_z_min(cs[6]);
  }
  __syncthreads();
  const int tpr = rb.d.tpr;  // threads per tile row; the tile is (4 tpr) x (256 / tpr) pixels
  const int tile_x = blockIdx.x % rb.d.tiles_x, tile_y = blockIdx.x / rb.d.tiles_x;
  const int row = tile_y * (256 / tpr) + threadIdx.x / tpr;
  const int col0 = tile_x * 4 * tpr + (threadIdx.x % tpr) * 4;
  if (row >= H || col0 >= W) return;
  const T* __restrict__ src = static_cast<const T*>(rb.src.p[o]);
  const float fill = rb.fill, wmax = (float)Ws, hmax = (float)Hs;

  float img[4][3], ma[4], mb[4];
  uint32_t ok[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int col = col0 + k;
    img[k][0] = img[k][1] = img[k][2] = fill;
    ma[k] = mb[k] = __builtin_nanf("");
    ok[k] = 0u;
    if (col >= W) continue;
    float X[3];
    if (!usm_ray(((float)col + 0.5f - cc.Cxd) * cc.invFd, ((float)row + 0.5f - cc.Cyd) * cc.invFd, cc.xid, X)) continue;
    float Xs[3];
    to_world(cc.M, X, Xs);
    if (!(Xs[2] > cc.zmin)) continue;
    float xs, ys;
    usm_project(Xs, cc.xis, &xs, &ys);
    const float a = cc.Fs * xs + cc.Cxs, b = cc.Fs * ys + cc.Cys;
    ma[k] = a;
    mb[k] = b;
    if (a >= 0.f && a <= wmax && b >= 0.f && b <= hmax) {  // false for NaN and infinities: no load without a point inside the source
      ok[k] = 1u;
      sample_clamped(src, Hs, Ws, a - 0.5f, b - 0.5f, img[k]);
    }
  }

  const size_t npx = (size_t)H * W, pix = (size_t)o * npx + (size_t)row * W + col0;
  T* __restrict__ out = static_cast<T*>(rb.img) + pix * 3;
  if (rb.d.vec) {  // W % 4 == 0 and aligned outputs: 12 / 48 image bytes, 4 mask bytes and two 16-byte map vectors
    if constexpr (sizeof(T) == 1) {
      uint32_t w[3] = {0u, 0u, 0u};
#pragma unroll
      for (int e = 0; e < 12; ++e) w[e / 4] |= round_u8(img[e / 3][e % 3]) << (8 * (e % 4));
      uint32_t* p = reinterpret_cast<uint32_t*>(out);
      p[0] = w[0]; p[1] = w[1]; p[2] = w[2];
    } else {
      store_rgb4(out, img);
    }
    if (EXTRAS) {
      if (rb.valid) *reinterpret_cast<uint32_t*>(rb.valid + pix) = ok[0] | ok[1] << 8 | ok[2] << 16 | ok[3] << 24;
      if (rb.map) {
        float* m = rb.map + pix + (size_t)o * npx;  // [n][2][H][W]
        *reinterpret_cast<float4*>(m) = make_float4(ma[0], ma[1], ma[2], ma[3]);
        *reinterpret_cast<float4*>(m + npx) = make_float4(mb[0], mb[1], mb[2], mb[3]);
      }
    }
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (col0 + k >= W) break;
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) store_px(out + 3 * k + ch, img[k][ch]);
      if (EXTRAS) {
        if (rb.valid) rb.valid[pix + k] = (uint8_t)ok[k];
        if (rb.map) {
          rb.map[pix + (size_t)o * npx + k] = ma[k];
          rb.map[pix + (size_t)o * npx + npx + k] = mb[k];
        }
      }
    }
  }
}

void launch_reproject(const ReprojBatch& rb, int dtype, hipStream_t s) {
  const dim3 grid((unsigned)(rb.d.tiles_x * rb.d.tiles_y), (unsigned)rb.d.n), block(256);
  const bool extras = rb.valid != nullptr || rb.map != nullptr;
  if (dtype == PF_PANO_U8) {
    if (extras) hipLaunchKernelGGL((reproject_kernel<uint8_t, true>), grid, block, 0, s, rb);
    else hipLaunchKernelGGL((reproject_kernel<uint8_t, false>), grid, block, 0, s, rb);
  } else {
    if (extras) hipLaunchKernelGGL((reproject_kernel<float, true>), grid, block, 0, s, rb);
    else hipLaunchKernelGGL((reproject_kernel<float, false>), grid, block, 0, s, rb);
  }
}

}  // namespace pf
