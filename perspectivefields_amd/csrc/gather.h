// What the batched image gathers (pano_crop.hip, reproject.hip, pano_compose.hip, pano_rotate.hip) share on the device: the bilinear blend of four taps, the uint8 rounding rule and
// the stores of the RGB epilogue.  Each kernel keeps its camera model and its index policy (which taps); the blend's order of operations and the
// rounding are here alone, so that every gather gives the same bits for the same taps.  The launch's shape is GatherDims (pf_kernels.h).
// yaw_align.hip samples one-channel fp32 planes with the same tap rule and blend order (sample_clamped_plane).
// Two pieces stay in the kernels because no helper form of them compiled to the kernels' instructions: the four lines of
// block -> (row, col0) arithmetic and the packing of 4 uint8 pixels into three 4-byte words.
#pragma once

#include <stdint.h>

#include "pf_kernels.h"

namespace pf {

__device__ __forceinline__ float texel(const uint8_t* p, size_t i) { return (float)p[i]; }
__device__ __forceinline__ float texel(const float* p, size_t i) { return p[i]; }

// bilinear blend of the taps (r0 | r1, c0 | c1) of channel-interleaved (., Ws, 3) texels, fu / fv the weights of c1 / r1; the caller has forced
// the four indices into the image.  Loads channel by channel, 64-bit offsets
template <typename T>
__device__ __forceinline__ void bilerp_rgb(const T* __restrict__ src, int Ws, int r0, int r1, int c0, int c1, float fu, float fv, float* out) {
  const size_t i00 = ((size_t)r0 * Ws + c0) * 3, i01 = ((size_t)r0 * Ws + c1) * 3;
  const size_t i10 = ((size_t)r1 * Ws + c0) * 3, i11 = ((size_t)r1 * Ws + c1) * 3;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float top = (1.f - fu) * texel(src, i00 + k) + fu * texel(src, i01 + k);
    const float bot = (1.f - fu) * texel(src, i10 + k) + fu * texel(src, i11 + k);
    out[k] = (1.f - fv) * top + fv * bot;
  }
}

// bilinear sample of channel-interleaved (Hs, Ws, 3) texels at (u, v), pixel centres at integers; the taps clamp into the image
template <typename T>
__device__ __forceinline__ void sample_clamped(const T* __restrict__ src, int Hs, int Ws, float u, float v, float* out) {
  const float uf = floorf(u), vf = floorf(v);
  const float fu = u - uf, fv = v - vf;
  const int c = (int)uf, r = (int)vf;
  const int c0 = min(max(c, 0), Ws - 1), c1 = min(max(c + 1, 0), Ws - 1);
  const int r0 = min(max(r, 0), Hs - 1), r1 = min(max(r + 1, 0), Hs - 1);
  bilerp_rgb(src, Ws, r0, r1, c0, c1, fu, fv, out);
}

// bilinear sample of channel-interleaved (Hp, Wp, 3) texels at (u, v): columns wrap, rows clamp, every index is forced into the panorama
template <typename T>
__device__ __forceinline__ void sample(const T* __restrict__ pano, int Hp, int Wp, float u, float v, float* out) {
  const float uf = floorf(u), vf = floorf(v);
  const float fu = u - uf, fv = v - vf;
  int c0 = (int)uf;
  c0 = c0 < 0 ? c0 + Wp : c0;
  c0 = c0 >= Wp ? c0 - Wp : c0;
  c0 = (unsigned)c0 >= (unsigned)Wp ? 0 : c0;
  const int c1 = c0 + 1 == Wp ? 0 : c0 + 1;
  const int r = (int)vf;
  const int r0 = min(max(r, 0), Hp - 1), r1 = min(max(r + 1, 0), Hp - 1);
  bilerp_rgb(pano, Wp, r0, r1, c0, c1, fu, fv, out);
}

// the one-channel form: bilinear sample of an (Hs, Ws) fp32 plane at (u, v) with the tap rule and the blend order of sample_clamped
__device__ __forceinline__ float sample_clamped_plane(const float* __restrict__ src, int Hs, int Ws, float u, float v) {
  const float uf = floorf(u), vf = floorf(v);
  const float fu = u - uf, fv = v - vf;
  const int c = (int)uf, r = (int)vf;
  const int c0 = min(max(c, 0), Ws - 1), c1 = min(max(c + 1, 0), Ws - 1);
  const int r0 = min(max(r, 0), Hs - 1), r1 = min(max(r + 1, 0), Hs - 1);
  const size_t o0 = (size_t)r0 * Ws, o1 = (size_t)r1 * Ws;
  const float top = (1.f - fu) * src[o0 + c0] + fu * src[o0 + c1];
  const float bot = (1.f - fu) * src[o1 + c0] + fu * src[o1 + c1];
  return (1.f - fv) * top + fv * bot;
}

// uint8 of an fp32 value: rounded half up, clamped to [0, 255]
__device__ __forceinline__ uint32_t round_u8(float v) { return (uint32_t)fminf(fmaxf(floorf(v + 0.5f), 0.f), 255.f); }

// 4 fp32 RGB pixels as three 16-byte stores; out aligned to 16 bytes (GatherDims::vec)
__device__ __forceinline__ void store_rgb4(float* out, const float (*img)[3]) {
  float4* o = reinterpret_cast<float4*>(out);
  o[0] = make_float4(img[0][0], img[0][1], img[0][2], img[1][0]);
  o[1] = make_float4(img[1][1], img[1][2], img[2][0], img[2][1]);
  o[2] = make_float4(img[2][2], img[3][0], img[3][1], img[3][2]);
}

// one channel of one pixel in the image's type: any alignment
__device__ __forceinline__ void store_px(uint8_t* out, float v) { *out = (uint8_t)round_u8(v); }
__device__ __forceinline__ void store_px(float* out, float v) { *out = v; }

}  // namespace pf
