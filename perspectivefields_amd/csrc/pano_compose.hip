// Camera views of one centre -> equirectangular panoramas (include/pf_hip.h pf_pano_compose): the inverse direction of
// pano_crop.hip, several views blended per output pixel, as one batched gather.  VALU and memory bound, no MFMA, no atomics.
//   pano_compose_kernel<T, FEATHER>  grid (tiles per panorama) x (panoramas of the launch), 256 threads.  Each block owns a 2-D tile of panorama
//                                    pixels (GatherDims::tpr threads x 4 pixels across, 256 / tpr rows; 64 x 16 as launched).  Threads v < count
//                                    compute the constants of view v of the block's panorama (M, F, Cx, Cy, xi, z_min, the size, the weight scale)
//                                    into LDS once per block.  A thread takes sincosf of its row's latitude and of its four columns' longitudes
//                                    once, then loops over the views in the caller's order with (C, S) of its four pixels in registers.
//                                    Every output value depends on its own panorama's views, their order and the options only: the same bits
//                                    in any batch and on every run.
// Model (the contract; tests/test_pano_compose_ref.py states it in fp64), panorama Hp x Wp, view i with camera theta_i and image Hs_i x Ws_i:
//   lon = ((col + 1/2) / Wp - 1/2) 2 pi, lat = (1/2 - (row + 1/2) / Hp) pi, D = (cos lat sin lon, -sin lat, cos lat cos lon): pano_crop.hip's sphere
//   X = M_i D, M_i = R_i^T Y(-yaw_i); visible iff X.z > z_min(xi_i); (a, b) = F_i (X.x, X.y) / (X.z + xi_i |X|) + (Cx_i, Cy_i)
//   d = min(a, Ws_i - a, b, Hs_i - b); the view covers the pixel iff visible and d > 0
//   w_i = min(2 d / min(Hs_i, Ws_i), 1) (FEATHER) or 1 (MEAN); c_i = bilinear at (a - 1/2, b - 1/2), taps clamped into the view (gather.h sample_clamped)
//   S = sum w_i, C = sum w_i c_i in fp32 in view order; pixel = C / S where S > 0, else fill; uint8 rounded half up and clamped; weight output = S
// Every comparison is a positive one: a NaN or infinite coordinate (non-finite parameters) covers nothing and issues no load, and the tap
// indices are clamped whatever the parameters.  Loads: channel by channel, every address inside its view, 64-bit offsets.
// A panorama of more than ComposeBatch::MAX views takes one launch per MAX views: a carry_out launch writes (C, S) to the fp32 accumulator
// instead of the image, a carry_in launch starts from it.  The same thread owns the same pixel in every launch and fp32 store / reload is
// exact, so the bits are those of one loop over all views.
#include <math.h>
#include <stdint.h>

#include "../../include/pf_hip.h"
#include "cam_model.h"
#include "gather.h"

namespace pf {

namespace {

constexpr float kTwoPi = 6.283185307179586f, kPi = 3.141592653589793f;

struct ViewConsts {
  float M[9];  // world (yaw 0) -> the view's camera, row major
  float F, Cx, Cy, xi, zmin;
  float wmax, hmax;  // the view's size
  float wscale;      // 2 / min(Hs, Ws)
};

}  // namespace

template <typename T, bool FEATHER>
__global__ __launch_bounds__(256) void pano_compose_kernel(ComposeBatch cb) {
  __shared__ ViewConsts vc[ComposeBatch::MAX];
  const int p = blockIdx.y;
  const int H = cb.d.H, W = cb.d.W;
  const int first = cb.first[p], count = min(cb.count[p], (int)ComposeBatch::MAX);
  if ((int)threadIdx.x < count) {
    const int v = first + (int)threadIdx.x;
    const float* cam = cb.cam + (size_t)v * 7;
    const int Hs = cb.src.H[v], Ws = cb.src.W[v];
    ViewConsts& c = vc[threadIdx.x];
    float R[9], sy, cy;
    cam_rotation(cam[0], cam[1], R);
    sincosf(0.f - cam[2], &sy, &cy);
    for (int i = 0; i < 3; ++i) {  // M = R^T Y(-yaw), Y(t) = [[cos t, 0, sin t], [0, 1, 0], [-sin t, 0, cos t]]
      c.M[3 * i] = R[i] * cy - R[6 + i] * sy;
      c.M[3 * i + 1] = R[3 + i];
      c.M[3 * i + 2] = R[i] * sy + R[6 + i] * cy;
    }
    c.F = cam[3] * (float)Hs;
    c.Cx = (cam[4] + 0.5f) * (float)Ws;
    c.Cy = (cam[5] + 0.5f) * (float)Hs;
    c.xi = cam[6];
    c.zmin = usm_z_min(cam[6]);
    c.wmax = (float)Ws;
    c.hmax = (float)Hs;
    c.wscale = 2.f / (float)min(Hs, Ws);
  }
  __syncthreads();
  const int tpr = cb.d.tpr;  // threads per tile row; the tile is (4 tpr) x (256 / tpr) pixels
  const int tile_x = blockIdx.x % cb.d.tiles_x, tile_y = blockIdx.x / cb.d.tiles_x;
  const int row = tile_y * (256 / tpr) + threadIdx.x / tpr;
  const int col0 = tile_x * 4 * tpr + (threadIdx.x % tpr) * 4;
  if (row >= H || col0 >= W) return;
  const size_t npx = (size_t)H * W, pix = (size_t)p * npx + (size_t)row * W + col0;
  float4* __restrict__ acc = reinterpret_cast<float4*>(cb.acc) + pix;  // touched only under the carry flags

  float sl, cl;
  sincosf((0.5f - ((float)row + 0.5f) / (float)H) * kPi, &sl, &cl);
  float D[4][3], C[4][3], S[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    float sn, cs;
    sincosf((((float)(col0 + k) + 0.5f) / (float)W - 0.5f) * kTwoPi, &sn, &cs);
    D[k][0] = cl * sn;
    D[k][1] = 0.f - sl;
    D[k][2] = cl * cs;
    C[k][0] = C[k][1] = C[k][2] = S[k] = 0.f;
  }
  if (cb.carry_in >> p & 1u) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (col0 + k >= W) break;
      const float4 a = acc[k];
      C[k][0] = a.x; C[k][1] = a.y; C[k][2] = a.z; S[k] = a.w;
    }
  }

  for (int i = 0; i < count; ++i) {
    const ViewConsts& c = vc[i];
    const T* __restrict__ src = static_cast<const T*>(cb.src.p[first + i]);
    const int Hs = cb.src.H[first + i], Ws = cb.src.W[first + i];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (col0 + k >= W) continue;
      float X[3];
      to_world(c.M, D[k], X);
      if (!(X[2] > c.zmin)) continue;
      float xs, ys;
      usm_project(X, c.xi, &xs, &ys);
      const float a = c.F * xs + c.Cx, b = c.F * ys + c.Cy;
      const float ra = c.wmax - a, rb = c.hmax - b;
      if (!(a > 0.f && ra > 0.f && b > 0.f && rb > 0.f)) continue;  // d > 0; false for NaN and infinities: no load without a point inside the view
      const float w = FEATHER ? fminf(fminf(fminf(a, ra), fminf(b, rb)) * c.wscale, 1.f) : 1.f;
      float px[3];
      sample_clamped(src, Hs, Ws, a - 0.5f, b - 0.5f, px);
      S[k] += w;
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) C[k][ch] = fmaf(w, px[ch], C[k][ch]);
    }
  }

  if (cb.carry_out >> p & 1u) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (col0 + k >= W) break;
      acc[k] = make_float4(C[k][0], C[k][1], C[k][2], S[k]);
    }
    return;
  }
  const float fill = cb.fill;
  float img[4][3];
#pragma unroll
  for (int k = 0; k < 4; ++k)
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) img[k][ch] = S[k] > 0.f ? C[k][ch] / S[k] : fill;

  T* __restrict__ out = static_cast<T*>(cb.img) + pix * 3;
  if (cb.d.vec) {  // W % 4 == 0 and aligned outputs: 12 / 48 image bytes and one 16-byte weight vector
    if constexpr (sizeof(T) == 1) {
      uint32_t w[3] = {0u, 0u, 0u};
#pragma unroll
      for (int e = 0; e < 12; ++e) w[e / 4] |= round_u8(img[e / 3][e % 3]) << (8 * (e % 4));
      uint32_t* o = reinterpret_cast<uint32_t*>(out);
      o[0] = w[0]; o[1] = w[1]; o[2] = w[2];
    } else {
      store_rgb4(out, img);
    }
    if (cb.weight) *reinterpret_cast<float4*>(cb.weight + pix) = make_float4(S[0], S[1], S[2], S[3]);
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (col0 + k >= W) break;
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) store_px(out + 3 * k + ch, img[k][ch]);
      if (cb.weight) cb.weight[pix + k] = S[k];
    }
  }
}

void launch_pano_compose(const ComposeBatch& cb, int dtype, int blend, hipStream_t s) {
  const dim3 grid((unsigned)(cb.d.tiles_x * cb.d.tiles_y), (unsigned)cb.d.n), block(256);
  const bool feather = blend == PF_BLEND_FEATHER;
  if (dtype == PF_PANO_U8) {
    if (feather) hipLaunchKernelGGL((pano_compose_kernel<uint8_t, true>), grid, block, 0, s, cb);
    else hipLaunchKernelGGL((pano_compose_kernel<uint8_t, false>), grid, block, 0, s, cb);
  } else {
    if (feather) hipLaunchKernelGGL((pano_compose_kernel<float, true>), grid, block, 0, s, cb);
    else hipLaunchKernelGGL((pano_compose_kernel<float, false>), grid, block, 0, s, cb);
  }
}

}  // namespace pf
