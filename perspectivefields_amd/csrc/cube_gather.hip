// Cube maps as a source: camera views and equirectangular panoramas out of six faces (include/pf_hip.h pf_cube_crop / pf_cube_to_pano, DESIGN.md
// section 28): two more image gathers of gather.h.  VALU and memory bound, no MFMA, no atomics, no workspace.
//   cube_crop_kernel<T>     views of cameras (roll, pitch, yaw, rel_focal, rel_cx, rel_cy, xi): pf_pano_crop's ray, turned into the world by
//                           Q = Y(yaw) R_pitch R_roll, sampled in the cube
//   cube_to_pano_kernel<T>  panoramas: pf_pano_rotate's pixel -> direction X = A D, sampled in the cube
//       both: grid (tiles per output) x (outputs of the group), 256 threads, a 64 x 16 pixel tile, 4 adjacent pixels of a row per thread, lane 0
//       computes the output's constants into LDS once per block, 64-bit offsets, vector stores with GatherDims::vec.  `samples` = S is a run-time loop
//       as in gather_ss.hip: the fp32 sum of the valid sub-samples at offsets (i + 1/2) / S, i-major then j, from -0, divided by their count.
// The sampler (the contract; tests/test_cubemap_ref.py states it in fp64).  A cube is (6, N, N, 3); face k has the frame (r, d, n) of kFace:
//   face    |z| >= |x| and |z| >= |y|: front (z >= 0) or back; else |x| >= |y|: right (x > 0) or left; else up (y < 0) or down
//   point   a = (X . r) / (X . n), b = (X . d) / (X . n); u = fma(a, N / 2, N / 2 - 1/2), v likewise: in [-1/2, N - 1/2], texel centres at integers
//   taps    (floor v, floor v + 1) x (floor u, floor u + 1), indices in [-1, N]; -1 and N are the ring
//   ring    one index in the ring: the texel of the face beyond that edge, unfolded flat around the edge (kRing: the face, and per index of that face
//           one of 0, N - 1, t, N - 1 - t with t the tap's index along the edge).  Both in the ring (a corner): (T0 + Ta + Tb) * (1/3) in fp32, T0 the
//           face's own corner texel, Ta the ring texel beside it across the column edge, Tb across the row edge
//   blend   bilerp_rgb's order of operations on the four values
// Only the taps of a sample next to an edge take the ring path (about 4 / N of the samples): the branch diverges along the seams alone.
// Every rounding step of the setup and of the per-sample function is spelled out (contraction off, fmaf where a fused step is meant).
#include <math.h>
#include <stdint.h>

#include "../../include/pf_hip.h"
#include "cam_model.h"
#include "gather.h"

namespace pf {

namespace {

constexpr float kPi = 3.14159265358979323846f, kThird = 1.f / 3.f;

// the face frames: right r, down d, forward n of face k = front, right, back, left, up, down (include/pf_hip.h)
struct Frame { int r[3], d[3], n[3]; };
constexpr Frame kFace[6] = {{{1, 0, 0}, {0, 1, 0}, {0, 0, 1}},  {{0, 0, -1}, {0, 1, 0}, {1, 0, 0}},  {{-1, 0, 0}, {0, 1, 0}, {0, 0, -1}},
                            {{0, 0, 1}, {0, 1, 0}, {-1, 0, 0}}, {{1, 0, 0}, {0, 0, 1}, {0, -1, 0}},  {{1, 0, 0}, {0, 0, -1}, {0, 1, 0}}};

constexpr int dot3(const int* a, const int* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }

// How an index of the neighbour follows from the ring tap: the neighbour's axis is the face's forward axis n (the first row or column inwards: N - 1
// along +n, 0 along -n) or the edge's axis o (the tap's index t along +o, N - 1 - t along -o)
enum : uint32_t { RING_ZERO = 0, RING_LAST = 1, RING_SAME = 2, RING_FLIP = 3 };
constexpr uint32_t ring_code(const int* axis, const int* n, const int* o) {
  return dot3(axis, n) == 1 ? RING_LAST : dot3(axis, n) == -1 ? RING_ZERO : dot3(axis, o) == 1 ? RING_SAME : RING_FLIP;
}
// the ring of face k beyond its edge `side` (0: col = N, +r; 1: col = -1, -r; 2: row = N, +d; 3: row = -1, -d): the texel whose direction is
// e + (1 - 1/N) n + t o lies on the face whose forward axis is e.  bits 0-2 the face, 3-4 the code of its column, 5-6 of its row
constexpr uint32_t ring_entry(int k, int side) {
  const Frame& f = kFace[k];
  const int sgn = (side & 1) ? -1 : 1;
  const int* ea = side < 2 ? f.r : f.d;
  const int* o = side < 2 ? f.d : f.r;
  const int e[3] = {sgn * ea[0], sgn * ea[1], sgn * ea[2]};
  int k2 = 0;
  for (int j = 0; j < 6; ++j)
    if (dot3(kFace[j].n, e) == 1) k2 = j;
  return (uint32_t)k2 | ring_code(kFace[k2].r, f.n, o) << 3 | ring_code(kFace[k2].d, f.n, o) << 5;
}
struct RingTable { uint32_t e[24]; };
constexpr RingTable make_ring() {
  RingTable t{};
  for (int k = 0; k < 6; ++k)
    for (int s = 0; s < 4; ++s) t.e[4 * k + s] = ring_entry(k, s);
  return t;
}
__constant__ RingTable kRing = make_ring();

__device__ __forceinline__ int ring_index(uint32_t code, int t, int N) {
  return code == RING_ZERO ? 0 : code == RING_LAST ? N - 1 : code == RING_SAME ? t : N - 1 - t;
}

// one tap (row, col) of face k with at most ONE index in the ring, the other inside the face: its three channels
template <typename T>
__device__ __forceinline__ void tap_or_ring(const T* __restrict__ cube, int N, int k, int row, int col, float* out) {
  int f = k, r = row, c = col;
  if (col < 0 || col >= N || row < 0 || row >= N) {
    const int side = col >= N ? 0 : col < 0 ? 1 : row >= N ? 2 : 3;
    const int t = side < 2 ? row : col;
    const uint32_t e = kRing.e[4 * k + side];
    f = (int)(e & 7u);
    c = ring_index((e >> 3) & 3u, t, N);
    r = ring_index((e >> 5) & 3u, t, N);
  }
  const size_t i = (((size_t)f * N + r) * N + c) * 3;
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) out[ch] = texel(cube, i + ch);
}

// any tap of face k, indices in [-1, N]
template <typename T>
__device__ __forceinline__ void tap_any(const T* __restrict__ cube, int N, int k, int row, int col, float* out) {
#pragma clang fp contract(off)
  const bool ring_r = row < 0 || row >= N, ring_c = col < 0 || col >= N;
  if (ring_r && ring_c) {  // a corner: no texel
    const int ir = min(max(row, 0), N - 1), ic = min(max(col, 0), N - 1);
    float t0[3], ta[3], tb[3];
    tap_or_ring(cube, N, k, ir, ic, t0);
    tap_or_ring(cube, N, k, ir, col, ta);
    tap_or_ring(cube, N, k, row, ic, tb);
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) out[ch] = ((t0[ch] + ta[ch]) + tb[ch]) * kThird;
  } else {
    tap_or_ring(cube, N, k, row, col, out);
  }
}

// the cube's value in the direction X: face, point, taps, blend
template <typename T>
__device__ __forceinline__ void cube_sample(const T* __restrict__ cube, int N, float X0, float X1, float X2, float* out) {
#pragma clang fp contract(off)
  const float ax = fabsf(X0), ay = fabsf(X1), az = fabsf(X2);
  int k;
  float xr, xd, xn;
  if (az >= ax && az >= ay) {
    k = X2 < 0.f ? 2 : 0;
    xr = X2 < 0.f ? -X0 : X0; xd = X1; xn = az;
  } else if (ax >= ay) {
    k = X0 > 0.f ? 1 : 3;
    xr = X0 > 0.f ? -X2 : X2; xd = X1; xn = ax;
  } else {
    k = X1 < 0.f ? 4 : 5;
    xr = X0; xd = X1 < 0.f ? X2 : -X2; xn = ay;
  }
  const float hN = (float)N * 0.5f, off = hN - 0.5f;
  const float u = fmaf(xr / xn, hN, off), v = fmaf(xd / xn, hN, off);
  const float uf = floorf(u), vf = floorf(v);
  const float fu = u - uf, fv = v - vf;
  // every index in [-1, N], also for a non-finite direction: fmaxf drops a NaN, and the integer clamp covers an N that fp32 rounds up
  const float top_f = (float)(N - 1);
  const int c0 = min(max((int)fminf(fmaxf(uf, -1.f), top_f), -1), N - 1), r0 = min(max((int)fminf(fmaxf(vf, -1.f), top_f), -1), N - 1);
  float t00[3], t01[3], t10[3], t11[3];
  if (c0 >= 0 && c0 + 1 < N && r0 >= 0 && r0 + 1 < N) {
    const size_t i00 = (((size_t)k * N + r0) * N + c0) * 3, i10 = i00 + (size_t)N * 3;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      t00[ch] = texel(cube, i00 + ch); t01[ch] = texel(cube, i00 + 3 + ch);
      t10[ch] = texel(cube, i10 + ch); t11[ch] = texel(cube, i10 + 3 + ch);
    }
  } else {
    tap_any(cube, N, k, r0, c0, t00);
    tap_any(cube, N, k, r0, c0 + 1, t01);
    tap_any(cube, N, k, r0 + 1, c0, t10);
    tap_any(cube, N, k, r0 + 1, c0 + 1, t11);
  }
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {  // bilerp_rgb's order
    const float top = (1.f - fu) * t00[ch] + fu * t01[ch];
    const float bot = (1.f - fu) * t10[ch] + fu * t11[ch];
    out[ch] = (1.f - fv) * top + fv * bot;
  }
}

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

// the image of 4 adjacent pixels of a row, each the mean of its n summed samples (0 without one): 12 / 48 bytes with `vec`, otherwise store_px
template <typename T>
__device__ __forceinline__ void store_means(T* __restrict__ out, int vec, int col0, int W, const float (*acc)[3], const int* n) {
  float img[4][3];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const float fn = (float)n[k];
#pragma unroll
    for (int c = 0; c < 3; ++c) img[k][c] = n[k] > 0 ? acc[k][c] / fn : 0.f;
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
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (col0 + k >= W) break;
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) store_px(out + 3 * k + ch, img[k][ch]);
    }
  }
}

struct CubeCropConsts {
  float Q[9];  // camera -> world, row major
  float invF, Cx, Cy, xi;
  int ok;      // 0: a non-finite parameter
};

struct CubePanoConsts {
  float A[9];  // output direction -> world direction, row major
  int ok;      // 0: a non-finite angle
};

}  // namespace

template <typename T>
__global__ __launch_bounds__(256) void cube_crop_kernel(CubeCropBatch cb) {
#pragma clang fp contract(off)
  __shared__ CubeCropConsts cc;
  const int out_i = blockIdx.y;
  const int H = cb.d.H, W = cb.d.W;
  if (threadIdx.x == 0) {
    const float* cam = cb.cam + (size_t)out_i * 7;
    const float roll = cam[0], pitch = cam[1], yaw = cam[2], f = cam[3], rcx = cam[4], rcy = cam[5], xi = cam[6];
    world_rotation(roll, pitch, yaw, cc.Q);
    cc.invF = 1.f / (f * (float)H);
    cc.Cx = (rcx + 0.5f) * (float)W;
    cc.Cy = (rcy + 0.5f) * (float)H;
    cc.xi = xi;
    cc.ok = (isfinite(roll) && isfinite(pitch) && isfinite(yaw) && isfinite(f) && isfinite(rcx) && isfinite(rcy) && isfinite(xi)) ? 1 : 0;
  }
  __syncthreads();
  const int tpr = cb.d.tpr;  // threads per tile row; the tile is (4 tpr) x (256 / tpr) pixels
  const int tile_x = blockIdx.x % cb.d.tiles_x, tile_y = blockIdx.x / cb.d.tiles_x;
  const int row = tile_y * (256 / tpr) + threadIdx.x / tpr;
  const int col0 = tile_x * 4 * tpr + (threadIdx.x % tpr) * 4;
  if (row >= H || col0 >= W) return;
  const T* __restrict__ cube = static_cast<const T*>(cb.src.p[out_i]);
  const int N = cb.src.H[out_i];
  const float xi = cc.xi, k1 = 1.f - xi * xi;
  const int S = cc.ok ? cb.samples : 0;  // a non-finite parameter: no sub-sample, no load
  const float fS = (float)cb.samples;

  float acc[4][3];
  int n[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    acc[k][0] = acc[k][1] = acc[k][2] = -0.f;
    n[k] = 0;
  }
  for (int i = 0; i < S; ++i) {
    const float y = ((float)row + sub_offset(i, fS) - cc.Cy) * cc.invF;
    for (int j = 0; j < S; ++j) {
      const float oj = sub_offset(j, fS);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int col = col0 + k;
        if (col >= W) continue;
        // pf_pano_crop's ray: rho^2, disc, eta, X = (eta x, eta y, eta - xi)
        const float x = ((float)col + oj - cc.Cx) * cc.invF;
        const float r2 = fmaf(x, x, y * y);
        const float disc = fmaf(k1, r2, 1.f);
        if (!(disc >= 0.f)) continue;
        const float eta = (xi + sqrtf(disc)) / (1.f + r2);
        const float C0 = eta * x, C1 = eta * y, C2 = eta - xi;
        const float X0 = fmaf(cc.Q[2], C2, fmaf(cc.Q[1], C1, cc.Q[0] * C0));
        const float X1 = fmaf(cc.Q[5], C2, fmaf(cc.Q[4], C1, cc.Q[3] * C0));
        const float X2 = fmaf(cc.Q[8], C2, fmaf(cc.Q[7], C1, cc.Q[6] * C0));
        float px[3];
        cube_sample(cube, N, X0, X1, X2, px);
        acc[k][0] += px[0]; acc[k][1] += px[1]; acc[k][2] += px[2];
        ++n[k];
      }
    }
  }
  const size_t pix = (size_t)out_i * ((size_t)H * W) + (size_t)row * W + col0;
  store_means(static_cast<T*>(cb.img) + pix * 3, cb.d.vec, col0, W, acc, n);
}

template <typename T>
__global__ __launch_bounds__(256) void cube_to_pano_kernel(CubePanoBatch cb) {
#pragma clang fp contract(off)
  __shared__ CubePanoConsts cc;
  const int out_i = blockIdx.y;
  const int H = cb.d.H, W = cb.d.W;
  if (threadIdx.x == 0) {
    const float* rot = cb.rot + (size_t)out_i * 3;
    float Q[9];
    world_rotation(rot[0], rot[1], rot[2], Q);
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) cc.A[3 * i + j] = cb.inverse ? Q[3 * j + i] : Q[3 * i + j];
    cc.ok = (isfinite(rot[0]) && isfinite(rot[1]) && isfinite(rot[2])) ? 1 : 0;
  }
  __syncthreads();
  const int tpr = cb.d.tpr;  // threads per tile row; the tile is (4 tpr) x (256 / tpr) pixels
  const int tile_x = blockIdx.x % cb.d.tiles_x, tile_y = blockIdx.x / cb.d.tiles_x;
  const int row = tile_y * (256 / tpr) + threadIdx.x / tpr;
  const int col0 = tile_x * 4 * tpr + (threadIdx.x % tpr) * 4;
  if (row >= H || col0 >= W) return;
  const T* __restrict__ cube = static_cast<const T*>(cb.src.p[out_i]);
  const int N = cb.src.H[out_i];
  const int S = cc.ok ? cb.samples : 0;  // a non-finite angle: no sub-sample, no load
  const float fS = (float)cb.samples;

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
        const float D0 = cl * so, D1 = -sl, D2 = cl * co;
        const float X0 = fmaf(cc.A[2], D2, fmaf(cc.A[1], D1, cc.A[0] * D0));
        const float X1 = fmaf(cc.A[5], D2, fmaf(cc.A[4], D1, cc.A[3] * D0));
        const float X2 = fmaf(cc.A[8], D2, fmaf(cc.A[7], D1, cc.A[6] * D0));
        float px[3];
        cube_sample(cube, N, X0, X1, X2, px);
        acc[k][0] += px[0]; acc[k][1] += px[1]; acc[k][2] += px[2];
        ++n[k];
      }
    }
  }
  const size_t pix = (size_t)out_i * ((size_t)H * W) + (size_t)row * W + col0;
  store_means(static_cast<T*>(cb.img) + pix * 3, cb.d.vec, col0, W, acc, n);
}

void launch_cube_crop(const CubeCropBatch& cb, int dtype, hipStream_t s) {
  const dim3 grid((unsigned)(cb.d.tiles_x * cb.d.tiles_y), (unsigned)cb.d.n), block(256);
  if (dtype == PF_PANO_U8) hipLaunchKernelGGL(cube_crop_kernel<uint8_t>, grid, block, 0, s, cb);
  else hipLaunchKernelGGL(cube_crop_kernel<float>, grid, block, 0, s, cb);
}

void launch_cube_to_pano(const CubePanoBatch& cb, int dtype, hipStream_t s) {
  const dim3 grid((unsigned)(cb.d.tiles_x * cb.d.tiles_y), (unsigned)cb.d.n), block(256);
  if (dtype == PF_PANO_U8) hipLaunchKernelGGL(cube_to_pano_kernel<uint8_t>, grid, block, 0, s, cb);
  else hipLaunchKernelGGL(cube_to_pano_kernel<float>, grid, block, 0, s, cb);
}

}  // namespace pf
