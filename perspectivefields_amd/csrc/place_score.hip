// Perspective-field discrepancy of an object's fields against a background's at every placement (include/pf_hip.h pf_place_scores):
// for (background, object) pairs and a stride, per placement the sum of the up-vector angles, the sum of the latitude differences and the number of
// valid pixel pairs.  VALU and memory bound, no MFMA, no atomics, no inline assembly; every offset into a plane is 64-bit.
//   place_pack_kernel   grid (blocks of 256 pixels) x (fields of the launch).  (up, lat) of every pixel -> one 8-byte record (theta, lat), theta =
//                       atan2f(u_y, u_x) in degrees clamped to [-180, 180]; both NaN where the pixel is invalid.  Every field is packed once per call,
//                       whatever number of pairs it is in, and a pixel pair of the score pass costs no atan2f.
//   place_score_kernel  grid (tiles) x (chunks) x (pairs of the launch), 256 threads.  A block owns (pair, tile of 256 placements in row-major order,
//                       chunk of <= 1024 object pixels in row-major order).  The block puts the chunk's records and their offsets r * W + c in the
//                       background in LDS.  Then one thread owns one placement: the offset of its corner (j * stride) * W + i * stride and three fp32
//                       sums in registers, a walk over the chunk in pixel order, four pixels at a time so that four loads are in flight.  Every lane
//                       reads the same LDS address (a broadcast, taken to scalar registers), so four invalid object pixels in a row are skipped by the
//                       whole wavefront and an invalid one among valid ones adds 0; the background record is one 8-byte load per lane at corner +
//                       offset: neighbouring lanes are neighbouring placements of a row, 8 * stride bytes apart.  No cross-lane reduction.  The three
//                       sums go to part[chunk][placement][3].
//   place_sum_kernel    one thread per (pair, placement): the chunks' records added in chunk order in fp64 -> out[pair][placement][3].
// A store pass and a sum pass, so the bits depend on the pair's two fields and the stride only: not on the launch, the other pairs or the run.
// Model (the contract; tests/test_placement_ref.py states it in fp64).  A pixel is valid iff its latitude is finite and the fp32 squared length of its up
// vector, fmaf(u_x, u_x, u_y * u_y), is >= 1e-12 and finite.  For the placement (j, i) the object's pixel (r, c) lies on the background's
// (j * stride + r, i * stride + c); where both are valid
//   e_up = min(d, 360 - d) with d = |theta_bg - theta_obj|: the angle between the two up vectors, 0 for equal vectors, the small angle across +-180
//   e_lat = |lat_bg - lat_obj|
// and (S_up, S_lat, n) are the sums over the valid pairs.
#include <math.h>
#include <stdint.h>

#include <algorithm>

#include "../../include/pf_hip.h"
#include "pf_kernels.h"

namespace pf {

namespace {

__device__ __forceinline__ float uniform(float v) { return __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, v))); }

}  // namespace

__global__ __launch_bounds__(256) void place_pack_kernel(PlacePack pp) {
  const int f = blockIdx.y;
  const size_t npx = (size_t)pp.npx[f];
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= npx) return;
  const float* __restrict__ up = pp.up[f];
  const float ux = up[i], uy = up[npx + i], la = pp.lat[f][i];
  const float l2 = fmaf(ux, ux, uy * uy);
  // a finite squared length means finite components
  const bool valid = l2 >= 1e-12f && l2 < INFINITY && fabsf(la) < INFINITY;
  // fp32 pi * 180 / pi may round above 180; inside [-180, 180] d below stays in [0, 360] and e_up in [0, 180]
  const float th = fminf(fmaxf(atan2f(uy, ux) * 57.29577951308232f, -180.f), 180.f);
  pp.out[f][i] = valid ? make_float2(th, la) : make_float2(NAN, NAN);
}

__global__ __launch_bounds__(PlaceBatch::TILE) void place_score_kernel(PlaceBatch pb) {
  __shared__ float2 rec[PlaceBatch::CHUNK];
  __shared__ int off[PlaceBatch::CHUNK];
  const PlacePair& pr = pb.pr[blockIdx.z];
  const int np = pr.np, ch = blockIdx.y;
  if ((size_t)blockIdx.x * PlaceBatch::TILE >= (size_t)np || ch >= pr.chunks) return;  // the whole block
  const int W = pr.W, w = pr.w, Q = pr.Q, stride = pb.stride;
  const int q0 = ch * PlaceBatch::CHUNK, cnt = min(pr.obj_px - q0, (int)PlaceBatch::CHUNK);
  const float2* __restrict__ obj = pr.obj;
  const int cnt4 = (cnt + 3) & ~3;  // the walk below takes four pixels at a time: the chunk is filled up with invalid ones
  for (int k = threadIdx.x; k < cnt4; k += PlaceBatch::TILE) {
    const int q = min(q0 + k, pr.obj_px - 1), r = q / w, c = q - r * w;
    rec[k] = k < cnt ? obj[(size_t)q] : make_float2(NAN, NAN);
    off[k] = r * W + c;  // < H * W < 2^31: checked on the host
  }
  __syncthreads();

  const int p = blockIdx.x * PlaceBatch::TILE + threadIdx.x;
  const bool mine = p < np;
  const int pc = mine ? p : 0;  // a lane past the last placement walks placement 0 and stores nothing
  const int j = pc / Q, i = pc - j * Q;
  const float2* __restrict__ bg = pr.bg + ((size_t)j * stride * W + (size_t)i * stride);
  float su = 0.f, sl = 0.f, n = 0.f;
  for (int k = 0; k < cnt4; k += 4) {
    float oth[4], ola[4];
    int o[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      oth[u] = uniform(rec[k + u].x);
      ola[u] = uniform(rec[k + u].y);
      o[u] = __builtin_amdgcn_readfirstlane(off[k + u]);
    }
    if (oth[0] != oth[0] && oth[1] != oth[1] && oth[2] != oth[2] && oth[3] != oth[3]) continue;  // the same for every lane
    float2 g[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) g[u] = bg[(size_t)o[u]];  // four loads in flight; an invalid pixel's offset is inside the object all the same
#pragma unroll
    for (int u = 0; u < 4; ++u) {  // in pixel order
      const bool v = oth[u] == oth[u] && g[u].x == g[u].x;
      const float d = fabsf(g[u].x - oth[u]);
      const float e = fminf(d, 360.f - d);
      const float dl = fabsf(g[u].y - ola[u]);
      su += v ? e : 0.f;
      sl += v ? dl : 0.f;
      n += v ? 1.f : 0.f;
    }
  }
  if (!mine) return;  // after the last barrier
  float* __restrict__ out = pb.part + (pr.part0 + (size_t)ch * np + p) * 3;
  out[0] = su;
  out[1] = sl;
  out[2] = n;
}

__global__ __launch_bounds__(256) void place_sum_kernel(PlaceBatch pb) {
  const PlacePair& pr = pb.pr[blockIdx.y];
  const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= (size_t)pr.np) return;
  double acc[3] = {0.0, 0.0, 0.0};
  for (int ch = 0; ch < pr.chunks; ++ch) {
    const float* __restrict__ in = pb.part + (pr.part0 + (size_t)ch * pr.np + p) * 3;
    acc[0] += (double)in[0];
    acc[1] += (double)in[1];
    acc[2] += (double)in[2];
  }
  double* __restrict__ out = pb.out + (pr.out0 + p) * 3;
  out[0] = acc[0];
  out[1] = acc[1];
  out[2] = acc[2];
}

void launch_place_pack(const PlacePack& pp, hipStream_t s) {
  int npx = 0;
  for (int f = 0; f < pp.n; ++f) npx = std::max(npx, pp.npx[f]);
  const dim3 grid((unsigned)(((size_t)npx + 255) / 256), (unsigned)pp.n), block(256);
  hipLaunchKernelGGL(place_pack_kernel, grid, block, 0, s, pp);
}

void launch_place_score(const PlaceBatch& pb, hipStream_t s) {
  const dim3 grid((unsigned)pb.max_tiles, (unsigned)pb.max_chunks, (unsigned)pb.n), block(PlaceBatch::TILE);
  hipLaunchKernelGGL(place_score_kernel, grid, block, 0, s, pb);
}

void launch_place_sum(const PlaceBatch& pb, hipStream_t s) {
  const dim3 grid((unsigned)pb.max_tiles, (unsigned)pb.n), block(256);
  hipLaunchKernelGGL(place_sum_kernel, grid, block, 0, s, pb);
}

}  // namespace pf
