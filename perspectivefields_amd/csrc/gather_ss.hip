// The supersampled forms of the three one-source gathers (include/pf_hip.h pf_pano_crop_ss / pf_reproject_ss / pf_pano_rotate_ss, DESIGN.md
// section 25): antialiasing for crops, re-projections and rotations that minify.  VALU and memory bound, no MFMA, no atomics.
// An output pixel is the mean of the valid ones of S x S sub-samples, S = `samples` in [1, PF_GATHER_MAX_SAMPLES].  Sub-sample (i, j) of pixel (row, col)
// sits at (a, b) = (col + (j + 1/2) / S, row + (i + 1/2) / S) and is its gather's per-sample model at that point, unchanged: ray, validity, source
// coordinate, tap rule and blend order are those of pano_crop.hip, reproject.hip and pano_rotate.hip, whose few lines per sample are restated here
// (their text does not change).  The fp32 sum runs over the valid sub-samples i-major, then j, from -0 (so that one sample is itself, whatever its sign),
// and is divided by their count as sum / (float)n; a pixel without a valid sub-sample is 0 (crop, rotation) or `fill` (re-projection).  At S = 1 the
// offsets are 1/2 exactly and every kernel gives the bits of its parent (tests/test_gpu_gather_samples.py).
// What describes the pixel and not its footprint is taken at the pixel centre with the parent's code: the labels of the crop and of the rotation, the
// map of the re-projection.  With an even S the centre is not itself a sub-sample.  The mask of the re-projection is 1 iff a sub-sample is valid.
//   pano_crop_ss_kernel<T, LABELS>, reproject_ss_kernel<T, EXTRAS>, pano_rotate_ss_kernel<T, LABELS>
//       the parents' shape: grid (tiles per output) x (outputs of the group), 256 threads, a 64 x 16 tile, 4 adjacent pixels of a row per thread, lane 0
//       computes the output's constants into LDS once per block, 64-bit offsets, every tap index forced into the source, vector stores with
//       GatherDims::vec.  S is a run-time loop: i outermost (the row's terms once per i), then j (the column offset once per j), then the thread's 4
//       pixels unrolled as in the parents, so that the body is the parents' body and one kernel serves every S (DESIGN.md section 25 says why).
#include <math.h>
#include <stdint.h>

#include "../../include/pf_hip.h"
#include "cam_model.h"
#include "gather.h"

namespace pf {

namespace {

constexpr float kInv2Pi = 0.15915494309189535f, kInvPi = 0.3183098861837907f, kPi = 3.14159265358979323846f, kRad2Deg = 57.29577951308232f;

// offset of sub-sample k of S inside its pixel: 1/2 exactly at S = 1
__device__ __forceinline__ float sub_offset(int k, float fS) { return ((float)k + 0.5f) / fS; }

// the mean of n >= 1 summed samples, or `empty`
__device__ __forceinline__ void mean_of(const float* acc, int n, float empty, float* out) {
  const float fn = (float)n;
#pragma unroll
  for (int c = 0; c < 3; ++c) out[c] = n > 0 ? acc[c] / fn : empty;
}

// the image of 4 adjacent pixels of a row: 12 / 48 bytes with `vec`, otherwise store_px for the pixels inside the row
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

// ---------------------------------------------------------------- pano_crop.hip's constants
struct CropConsts {
  float R[9];  // camera -> world, row major
  float g[3];  // world up (0, -1, 0) in camera coordinates
  float F, invF, Cx, Cy, xi, yaw_t, sx, sy;
  PinholeFields pin;  // the xi == 0 labels
};

// ---------------------------------------------------------------- reproject.hip's constants
struct ReprojConsts {
  float M[9];  // destination camera -> source camera, row major
  float invFd, Cxd, Cyd, xid;
  float Fs, Cxs, Cys, xis, zmin;
};

// ---------------------------------------------------------------- pano_rotate.hip's constants and per-pixel function, the pixel centre's 1/2 a parameter
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
  float R[9], sy, cy, Q[9];
  cam_rotation(roll, pitch, R);
  sincosf(yaw, &sy, &cy);
  // Y(yaw) R, Y = [[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]
  for (int k = 0; k < 3; ++k) {
    Q[k] = fmaf(cy, R[k], sy * R[6 + k]);
    Q[3 + k] = R[3 + k];
    Q[6 + k] = fmaf(cy, R[6 + k], -(sy * R[k]));
  }
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) c->A[3 * i + j] = inverse ? Q[3 * j + i] : Q[3 * i + j];
  c->g[0] = -c->A[3]; c->g[1] = -c->A[4]; c->g[2] = -c->A[5];
  c->kx = (float)W * kInv2Pi;
  c->ky = (float)H * kInvPi;
  c->ok = (isfinite(roll) && isfinite(pitch) && isfinite(yaw)) ? 1 : 0;
}

// sine and cosine of the latitude of the point `off` below the top of row `row`
__device__ __forceinline__ void row_sincos(int row, float off, int H, float* sl, float* cl) {
#pragma clang fp contract(off)
  sincosf((0.5f - ((float)row + off) / (float)H) * kPi, sl, cl);
}

struct RotPixel {
  float ts, tl;      // longitude and latitude of the source point as fractions: lon_s / 2 pi + 1/2 and 1/2 - lat_s / pi
  float ux, uy, lat; // the labels (LABELS only)
};

// the point `off` right of the left side of pixel `col` of an H x W output, on a row whose latitude has sine / cosine (sl, cl)
template <bool LABELS>
__device__ __forceinline__ RotPixel rot_pixel(const RotConsts& c, float sl, float cl, int col, float off, int W) {
#pragma clang fp contract(off)
  float so, co;
  sincosf((((float)col + off) / (float)W - 0.5f) * (2.f * kPi), &so, &co);
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

}  // namespace

template <typename T, bool LABELS>
__global__ __launch_bounds__(256) void pano_crop_ss_kernel(PanoSsBatch pb) {
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
  const int S = pb.samples;
  const float fS = (float)S;

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
        float X[3];
        if (usm_ray(((float)col + oj - cc.Cx) * cc.invF, y, xi, X)) {
          float Xw[3], px[3];
          to_world(cc.R, X, Xw);
          float t = cc.yaw_t + atan2f(Xw[0], Xw[2]) * kInv2Pi;
          t -= floorf(t);
          const float u = t * (float)Wp - 0.5f;
          const float v = (0.5f + atan2f(Xw[1], sqrtf(Xw[0] * Xw[0] + Xw[2] * Xw[2])) * kInvPi) * (float)Hp - 0.5f;
          sample(pano, Hp, Wp, u, v, px);
          acc[k][0] += px[0]; acc[k][1] += px[1]; acc[k][2] += px[2];
          ++n[k];
        }
      }
    }
  }

  float img[4][3], ux[4], uy[4], lat[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int col = col0 + k;
    mean_of(acc[k], n[k], 0.f, img[k]);
    ux[k] = uy[k] = lat[k] = __builtin_nanf("");
    if (!LABELS || col >= W) continue;
    float X[3];  // the labels are the pixel's: pano_crop.hip's at (col + 1/2, row + 1/2) and at the linspace point
    if (xi == 0.f) {
      const FieldsPixel o = pinhole_fields_at(cc.pin, row, col);
      ux[k] = o.ux;
      uy[k] = o.uy;
      lat[k] = o.lat;
    } else {
      if (usm_ray(((float)col + 0.5f - cc.Cx) * cc.invF, ((float)row + 0.5f - cc.Cy) * cc.invF, xi, X)) usm_up_of_ray(X, cc.g, xi, &ux[k], &uy[k]);
      if (usm_ray(((float)col * cc.sx - cc.Cx) / cc.F, ((float)row * cc.sy - cc.Cy) / cc.F, xi, X)) lat[k] = usm_lat_of_ray(X, cc.R);
    }
  }

  const size_t npx = (size_t)H * W, pix = (size_t)crop * npx + (size_t)row * W + col0;
  store_image(static_cast<T*>(pb.img) + pix * 3, pb.d.vec, col0, W, img);
  if (LABELS) store_labels(pb.up, pb.lat, pb.d.vec, crop, H, W, row, col0, ux, uy, lat);
}

template <typename T, bool EXTRAS>
__global__ __launch_bounds__(256) void reproject_ss_kernel(ReprojSsBatch rb) {
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
  const float wmax = (float)Ws, hmax = (float)Hs;
  const int S = rb.samples;
  const float fS = (float)S;

  float acc[4][3];
  int n[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    acc[k][0] = acc[k][1] = acc[k][2] = -0.f;
    n[k] = 0;
  }
  for (int i = 0; i < S; ++i) {
    const float y = ((float)row + sub_offset(i, fS) - cc.Cyd) * cc.invFd;
    for (int j = 0; j < S; ++j) {
      const float oj = sub_offset(j, fS);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int col = col0 + k;
        if (col >= W) continue;
        float X[3];
        if (!usm_ray(((float)col + oj - cc.Cxd) * cc.invFd, y, cc.xid, X)) continue;
        float Xs[3];
        to_world(cc.M, X, Xs);
        if (!(Xs[2] > cc.zmin)) continue;
        float xs, ys;
        usm_project(Xs, cc.xis, &xs, &ys);
        const float a = cc.Fs * xs + cc.Cxs, b = cc.Fs * ys + cc.Cys;
        if (a >= 0.f && a <= wmax && b >= 0.f && b <= hmax) {  // false for NaN and infinities: no load without a point inside the source
          float px[3];
          sample_clamped(src, Hs, Ws, a - 0.5f, b - 0.5f, px);
          acc[k][0] += px[0]; acc[k][1] += px[1]; acc[k][2] += px[2];
          ++n[k];
        }
      }
    }
  }

  float img[4][3], ma[4], mb[4];
  uint32_t ok[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    mean_of(acc[k], n[k], rb.fill, img[k]);
    ok[k] = n[k] > 0 ? 1u : 0u;
    ma[k] = mb[k] = __builtin_nanf("");
  }
  if (EXTRAS && rb.map) {  // the map is the pixel centre's: reproject.hip's steps at (col + 1/2, row + 1/2)
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int col = col0 + k;
      if (col >= W) continue;
      float X[3];
      if (!usm_ray(((float)col + 0.5f - cc.Cxd) * cc.invFd, ((float)row + 0.5f - cc.Cyd) * cc.invFd, cc.xid, X)) continue;
      float Xs[3];
      to_world(cc.M, X, Xs);
      if (!(Xs[2] > cc.zmin)) continue;
      float xs, ys;
      usm_project(Xs, cc.xis, &xs, &ys);
      ma[k] = cc.Fs * xs + cc.Cxs;
      mb[k] = cc.Fs * ys + cc.Cys;
    }
  }

  const size_t npx = (size_t)H * W, pix = (size_t)o * npx + (size_t)row * W + col0;
  store_image(static_cast<T*>(rb.img) + pix * 3, rb.d.vec, col0, W, img);
  if (EXTRAS) {
    if (rb.d.vec) {  // 4 mask bytes and two 16-byte map vectors
      if (rb.valid) *reinterpret_cast<uint32_t*>(rb.valid + pix) = ok[0] | ok[1] << 8 | ok[2] << 16 | ok[3] << 24;
      if (rb.map) {
        float* m = rb.map + pix + (size_t)o * npx;  // [n][2][H][W]
        *reinterpret_cast<float4*>(m) = make_float4(ma[0], ma[1], ma[2], ma[3]);
        *reinterpret_cast<float4*>(m + npx) = make_float4(mb[0], mb[1], mb[2], mb[3]);
      }
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (col0 + k >= W) break;
        if (rb.valid) rb.valid[pix + k] = (uint8_t)ok[k];
        if (rb.map) {
          rb.map[pix + (size_t)o * npx + k] = ma[k];
          rb.map[pix + (size_t)o * npx + npx + k] = mb[k];
        }
      }
    }
  }
}

template <typename T, bool LABELS>
__global__ __launch_bounds__(256) void pano_rotate_ss_kernel(PanoRotSsBatch rb) {
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
  const int S = rc.ok ? rb.samples : 0;  // a non-finite angle: no sub-sample, no load
  const float fS = (float)rb.samples;

  float acc[4][3];
  int n[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    acc[k][0] = acc[k][1] = acc[k][2] = -0.f;
    n[k] = 0;
  }
  for (int i = 0; i < S; ++i) {
    float sl, cl;
    row_sincos(row, sub_offset(i, fS), H, &sl, &cl);
    for (int j = 0; j < S; ++j) {
      const float oj = sub_offset(j, fS);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int col = col0 + k;
        if (col >= W) continue;
        const RotPixel o = rot_pixel<false>(rc, sl, cl, col, oj, W);
        float px[3];
        sample(src, Hs, Ws, fmaf(o.ts, (float)Ws, -0.5f), fmaf(o.tl, (float)Hs, -0.5f), px);
        acc[k][0] += px[0]; acc[k][1] += px[1]; acc[k][2] += px[2];
        ++n[k];
      }
    }
  }

  float img[4][3], ux[4], uy[4], lat[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    mean_of(acc[k], n[k], 0.f, img[k]);
    ux[k] = uy[k] = lat[k] = __builtin_nanf("");
  }
  if (LABELS && rc.ok) {  // the labels are the pixel centre's: pano_rotate.hip's
    float sl, cl;
    row_sincos(row, 0.5f, H, &sl, &cl);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (col0 + k >= W) continue;
      const RotPixel o = rot_pixel<true>(rc, sl, cl, col0 + k, 0.5f, W);
      ux[k] = o.ux; uy[k] = o.uy; lat[k] = o.lat;
    }
  }

  const size_t npx = (size_t)H * W, pix = (size_t)out_i * npx + (size_t)row * W + col0;
  store_image(static_cast<T*>(rb.img) + pix * 3, rb.d.vec, col0, W, img);
  if (LABELS) store_labels(rb.up, rb.lat, rb.d.vec, out_i, H, W, row, col0, ux, uy, lat);
}

template <class Batch>
static dim3 ss_grid(const Batch& b) { return dim3((unsigned)(b.d.tiles_x * b.d.tiles_y), (unsigned)b.d.n); }

void launch_pano_crop_ss(const PanoSsBatch& pb, int dtype, hipStream_t s) {
  const dim3 grid = ss_grid(pb), block(256);
  const bool labels = pb.up != nullptr;
  if (dtype == PF_PANO_U8) {
    if (labels) hipLaunchKernelGGL((pano_crop_ss_kernel<uint8_t, true>), grid, block, 0, s, pb);
    else hipLaunchKernelGGL((pano_crop_ss_kernel<uint8_t, false>), grid, block, 0, s, pb);
  } else {
    if (labels) hipLaunchKernelGGL((pano_crop_ss_kernel<float, true>), grid, block, 0, s, pb);
    else hipLaunchKernelGGL((pano_crop_ss_kernel<float, false>), grid, block, 0, s, pb);
  }
}

void launch_reproject_ss(const ReprojSsBatch& rb, int dtype, hipStream_t s) {
  const dim3 grid = ss_grid(rb), block(256);
  const bool extras = rb.valid != nullptr || rb.map != nullptr;
  if (dtype == PF_PANO_U8) {
    if (extras) hipLaunchKernelGGL((reproject_ss_kernel<uint8_t, true>), grid, block, 0, s, rb);
    else hipLaunchKernelGGL((reproject_ss_kernel<uint8_t, false>), grid, block, 0, s, rb);
  } else {
    if (extras) hipLaunchKernelGGL((reproject_ss_kernel<float, true>), grid, block, 0, s, rb);
    else hipLaunchKernelGGL((reproject_ss_kernel<float, false>), grid, block, 0, s, rb);
  }
}

void launch_pano_rotate_ss(const PanoRotSsBatch& rb, int dtype, hipStream_t s) {
  const dim3 grid = ss_grid(rb), block(256);
  const bool labels = rb.up != nullptr;
  if (dtype == PF_PANO_U8) {
    if (labels) hipLaunchKernelGGL((pano_rotate_ss_kernel<uint8_t, true>), grid, block, 0, s, rb);
    else hipLaunchKernelGGL((pano_rotate_ss_kernel<uint8_t, false>), grid, block, 0, s, rb);
  } else {
    if (labels) hipLaunchKernelGGL((pano_rotate_ss_kernel<float, true>), grid, block, 0, s, rb);
    else hipLaunchKernelGGL((pano_rotate_ss_kernel<float, false>), grid, block, 0, s, rb);
  }
}

}  // namespace pf
