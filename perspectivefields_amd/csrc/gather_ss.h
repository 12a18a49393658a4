// The sample loop of the supersampled gathers, stated once (DESIGN.md sections 25 and 31): gather_ss.hip, cube_gather.hip and fisheye_gather.hip plug
// their seven models into gather_ss<M>.  An output pixel is the mean of the valid ones of S x S sub-samples, S = `samples` in
// [1, PF_GATHER_MAX_SAMPLES]; sub-sample (i, j) of pixel (row, col) sits at (col + (j + 1/2) / S, row + (i + 1/2) / S).  What holds for every model by
// construction: the fp32 sum runs over the valid sub-samples only, i-major, then j, from -0 (so that one sample is itself, whatever its sign); the
// pixel is sum / (float)n, or the model's `empty` value without a valid sub-sample; what describes the pixel and not its footprint (labels, map) is
// computed after the loop, at the pixel centre, by the model's finish(); a non-finite parameter row (ok() false) runs no sub-sample and issues no load.
// The shape is the parents' (gather.h): grid (tiles per output) x (outputs of the group), 256 threads, a 64 x 16 tile, 4 adjacent pixels of a row per
// thread, lane 0 computes the output's constants into LDS once per block, 64-bit offsets, vector stores with GatherDims::vec.  S is a run-time loop: i
// outermost (the row's term once per i), then j (the column offset once per j), then the thread's 4 pixels unrolled, so one kernel serves every S.
// A model M supplies
//   M::Texel, M::Batch, M::Consts                       uint8_t | float, the kernel's argument (pf_kernels.h), the output's constants in LDS
//   static void setup(const Batch&, int out_i, Consts*)  lane 0
//   M(const Batch&, const Consts&, int out_i)            what a thread keeps in registers: the source, its size, loop invariants
//   bool ok()                                            false: a non-finite parameter row
//   R row_term(int row, float off)                       once per i: what depends on the sub-sample's row alone
//   bool sample(const R&, int col, float off, float* px) the model's value at sub-sample column col + off, false where it has none
//   float empty()                                        0 or `fill`
//   void finish(int row, int col0, size_t pix, const int* n)   the stores beside the image: labels, mask, map (store_labels, store_mask, store_plane4)
// The kernels stay named __global__ functions whose body is the one call of gather_ss<M>, so the block -> (row, col0) lines are kernel text after
// inlining, as gather.h requires of them.
// pano_crop_ss_kernel (gather_ss.hip) is not a model: as one it gave the parent's bits only with its blend spelled out and was then 15 - 20 % slower on
// the crop workload of scripts/time_gather_samples.py.  It keeps its loop in its own text and calls the helpers below.
#pragma once

#include <stdint.h>

#include "../../include/pf_hip.h"
#include "gather.h"

namespace pf {

// offset of sub-sample k of S inside its pixel: 1/2 exactly at S = 1
__device__ __forceinline__ float sub_offset(int k, float fS) { return ((float)k + 0.5f) / fS; }

// the mean of n >= 1 summed samples, or `empty`
__device__ __forceinline__ void mean_of(const float* acc, int n, float empty, float* out) {
  const float fn = (float)n;
#pragma unroll
  for (int c = 0; c < 3; ++c) out[c] = n > 0 ? acc[c] / fn : empty;
}

// the image of 4 adjacent pixels of a row: 12 / 48 bytes with `vec` (W % 4 == 0 and aligned outputs), otherwise store_px for the pixels inside the row
template <typename T>
__device__ __forceinline__ void store_image(T* __restrict__ out, int vec, int col0, int W, const float (*img)[3]) {
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
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (col0 + k >= W) break;
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) store_px(out + 3 * k + ch, img[k][ch]);
    }
  }
}

// 4 adjacent values of a row of an fp32 plane: one 16-byte vector with `vec`, otherwise scalars for the pixels inside the row
__device__ __forceinline__ void store_plane4(float* p, int vec, int col0, int W, const float* v) {
  if (vec) {
    *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (col0 + k >= W) break;
      p[k] = v[k];
    }
  }
}

// the labels of the 4 pixels at `pix` of output `out_i`: up [n][2][H][W], lat [n][H][W]
__device__ __forceinline__ void store_labels(float* up, float* lat, int vec, int out_i, size_t npx, size_t pix, int col0, int W, const float* ux,
                                             const float* uy, const float* la) {
  store_plane4(up + pix + (size_t)out_i * npx, vec, col0, W, ux);
  store_plane4(up + pix + (size_t)out_i * npx + npx, vec, col0, W, uy);
  store_plane4(lat + pix, vec, col0, W, la);
}

// the mask of 4 adjacent pixels, 1 where a sub-sample was valid: 4 bytes with `vec`, otherwise single bytes for the pixels inside the row
__device__ __forceinline__ void store_mask(uint8_t* valid, int vec, int col0, int W, const int* n) {
  uint32_t ok[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) ok[k] = n[k] > 0 ? 1u : 0u;
  if (vec) {
    *reinterpret_cast<uint32_t*>(valid) = ok[0] | ok[1] << 8 | ok[2] << 16 | ok[3] << 24;
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (col0 + k >= W) break;
      valid[k] = (uint8_t)ok[k];
    }
  }
}

template <class M>
__device__ __forceinline__ void gather_ss(const typename M::Batch& b) {
  using T = typename M::Texel;
  __shared__ typename M::Consts cc;
  const int out_i = blockIdx.y;
  const int H = b.d.H, W = b.d.W;
  if (threadIdx.x == 0) M::setup(b, out_i, &cc);
  __syncthreads();
  const int tpr = b.d.tpr;  // threads per tile row; the tile is (4 tpr) x (256 / tpr) pixels
  const int tile_x = blockIdx.x % b.d.tiles_x, tile_y = blockIdx.x / b.d.tiles_x;
  const int row = tile_y * (256 / tpr) + threadIdx.x / tpr;
  const int col0 = tile_x * 4 * tpr + (threadIdx.x % tpr) * 4;
  if (row >= H || col0 >= W) return;
  const M m(b, cc, out_i);
  const int S = m.ok() ? b.samples : 0;  // a non-finite parameter row: no sub-sample, no load
  const float fS = (float)b.samples;

  float acc[4][3];
  int n[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    acc[k][0] = acc[k][1] = acc[k][2] = -0.f;
    n[k] = 0;
  }
  for (int i = 0; i < S; ++i) {
    const auto rt = m.row_term(row, sub_offset(i, fS));
    for (int j = 0; j < S; ++j) {
      const float oj = sub_offset(j, fS);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int col = col0 + k;
        if (col >= W) continue;
        float px[3];
        if (!m.sample(rt, col, oj, px)) continue;
        acc[k][0] += px[0]; acc[k][1] += px[1]; acc[k][2] += px[2];
        ++n[k];
      }
    }
  }

  float img[4][3];
#pragma unroll
  for (int k = 0; k < 4; ++k) mean_of(acc[k], n[k], m.empty(), img[k]);
  const size_t pix = (size_t)out_i * ((size_t)H * W) + (size_t)row * W + col0;
  store_image(static_cast<T*>(b.img) + pix * 3, b.d.vec, col0, W, img);
  m.finish(row, col0, pix, n);
}

// the launch of one instantiation and the dtype half of the ladder dtype x flag -> instantiation: every launcher of these units ends here; one with
// a flag (labels, extras) picks its pair of instantiations with one if / else first
template <class Batch>
void launch_ss(void (*u8)(Batch), void (*f32)(Batch), const Batch& b, int dtype, hipStream_t s) {
  const dim3 grid((unsigned)(b.d.tiles_x * b.d.tiles_y), (unsigned)b.d.n), block(256);
  hipLaunchKernelGGL(dtype == PF_PANO_U8 ? u8 : f32, grid, block, 0, s, b);
}

}  // namespace pf
