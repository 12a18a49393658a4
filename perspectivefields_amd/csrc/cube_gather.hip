// Cube maps as a source: camera views and equirectangular panoramas out of six faces (include/pf_hip.h pf_cube_crop / pf_cube_to_pano, DESIGN.md
// section 28): two more image gathers of gather.h.  VALU and memory bound, no MFMA, no atomics, no workspace.
//   cube_crop_kernel<T>     views of cameras (roll, pitch, yaw, rel_focal, rel_cx, rel_cy, xi): pf_pano_crop's ray, turned into the world by
//                           Q = Y(yaw) R_pitch R_roll, sampled in the cube
//   cube_to_pano_kernel<T>  panoramas: pf_pano_rotate's pixel -> direction X = A D, sampled in the cube
//       both are models of gather_ss.h, which owns the launch shape, the `samples` loop, the mean and the stores; the ray, the rotation and the
//       pixel -> direction are cam_model.h's.
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
#include "gather_ss.h"

// every rounding step of this unit's setup and per-sample functions is spelled out: no contraction in what follows, fmaf where a fused step is meant
#pragma clang fp contract(off)

namespace pf {

namespace {

constexpr float kThird = 1.f / 3.f;

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

// ---------------------------------------------------------------- the two models of gather_ss.h: an empty pixel is 0, nothing is stored beside the image
template <typename T>
struct CubeSource {  // what both keep per thread
  const T* __restrict__ cube;
  const int N;
  template <class Batch>
  __device__ __forceinline__ CubeSource(const Batch& b, int i) : cube(static_cast<const T*>(b.src.p[i])), N(b.src.H[i]) {}
  __device__ __forceinline__ float empty() const { return 0.f; }
  __device__ __forceinline__ void finish(int, int, size_t, const int*) const {}
};

struct CubeCropConsts {
  float Q[9];  // camera -> world, row major
  float invF, Cx, Cy, xi;
  int ok;      // 0: a non-finite parameter
};

// views of cameras: pf_pano_crop's ray (usm_ray_exact), turned into the world by Q
template <typename T>
struct CubeCrop : CubeSource<T> {
  using Texel = T;
  using Batch = CubeCropBatch;
  using Consts = CubeCropConsts;

  static __device__ __forceinline__ void setup(const Batch& cb, int out_i, Consts* c) {
    const float* cam = cb.cam + (size_t)out_i * 7;
    world_rotation(cam[0], cam[1], cam[2], c->Q);
    c->invF = 1.f / (cam[3] * (float)cb.d.H);
    c->Cx = (cam[4] + 0.5f) * (float)cb.d.W;
    c->Cy = (cam[5] + 0.5f) * (float)cb.d.H;
    c->xi = cam[6];
    c->ok = all_finite(cam, 7) ? 1 : 0;
  }

  const Consts& cc;
  const float xi, k1;
  __device__ __forceinline__ CubeCrop(const Batch& b, const Consts& c, int i) : CubeSource<T>(b, i), cc(c), xi(c.xi), k1(1.f - c.xi * c.xi) {}

  __device__ __forceinline__ bool ok() const { return cc.ok != 0; }
  __device__ __forceinline__ float row_term(int row, float off) const { return ((float)row + off - cc.Cy) * cc.invF; }
  __device__ __forceinline__ bool sample(float y, int col, float off, float* px) const {
    float C[3], X[3];
    if (!usm_ray_exact(((float)col + off - cc.Cx) * cc.invF, y, xi, k1, C)) return false;
    rotate_exact(cc.Q, C[0], C[1], C[2], X);
    cube_sample(this->cube, this->N, X[0], X[1], X[2], px);
    return true;
  }
};

struct CubePanoConsts {
  float A[9];  // output direction -> world direction, row major
  int ok;      // 0: a non-finite angle
};

// panoramas: pf_pano_rotate's pixel -> direction (pano_row, pano_direction), X = A D
template <typename T>
struct CubePano : CubeSource<T> {
  using Texel = T;
  using Batch = CubePanoBatch;
  using Consts = CubePanoConsts;

  static __device__ __forceinline__ void setup(const Batch& cb, int out_i, Consts* c) {
    const float* rot = cb.rot + (size_t)out_i * 3;
    pano_rotation(rot, cb.inverse, c->A);
    c->ok = all_finite(rot, 3) ? 1 : 0;
  }

  const Consts& cc;
  const int H, W;
  __device__ __forceinline__ CubePano(const Batch& b, const Consts& c, int i) : CubeSource<T>(b, i), cc(c), H(b.d.H), W(b.d.W) {}

  __device__ __forceinline__ bool ok() const { return cc.ok != 0; }
  __device__ __forceinline__ PanoRow row_term(int row, float off) const { return pano_row(row, off, H); }
  __device__ __forceinline__ bool sample(const PanoRow& r, int col, float off, float* px) const {
    float so, co, D[3], X[3];
    pano_direction(r, col, off, W, D, &so, &co);
    rotate_exact(cc.A, D[0], D[1], D[2], X);
    cube_sample(this->cube, this->N, X[0], X[1], X[2], px);
    return true;
  }
};

}  // namespace

template <typename T>
__global__ __launch_bounds__(256) void cube_crop_kernel(CubeCropBatch cb) { gather_ss<CubeCrop<T>>(cb); }

template <typename T>
__global__ __launch_bounds__(256) void cube_to_pano_kernel(CubePanoBatch cb) { gather_ss<CubePano<T>>(cb); }

void launch_cube_crop(const CubeCropBatch& cb, int dtype, hipStream_t s) { launch_ss(cube_crop_kernel<uint8_t>, cube_crop_kernel<float>, cb, dtype, s); }

void launch_cube_to_pano(const CubePanoBatch& cb, int dtype, hipStream_t s) {
  launch_ss(cube_to_pano_kernel<uint8_t>, cube_to_pano_kernel<float>, cb, dtype, s);
}

}  // namespace pf
