// Perspective fields drawn over their images (include/pf_hip.h pf_draw_fields): a latitude tint, iso-latitude lines and up
// arrows, composed onto the picture in one pass.  VALU and memory bound, no MFMA, no atomics, no inline assembly; every offset into an image or a
// plane is 64-bit.
//   draw_arrows_kernel     grid (blocks of 256 anchors) x (images of the launch).  One thread per anchor: it reads the anchor's field pixel and writes
//                          one 64-byte record -- (a, u), (tip, valid, -), (the two barb directions), (the padded bounding box) -- written once per
//                          call and read by every tile the arrow can reach.  An anchor without an arrow has a NaN box, which meets nothing.
//   draw_fields_kernel<T>  grid (tiles of the largest image) x (images of the launch), 256 threads, a 64 x 16 tile, a thread owns 4 adjacent pixels of
//                          a row (reproject_kernel's shape; the images of a launch may differ in size, a block past its image's tiles leaves).
//                          1. every thread: its pixels, the tint and the iso-line from its own latitudes and their four neighbours (plain
//                             global loads: the neighbours hit L1 / L2);
//                          2. the block: the anchors whose pixel lies within `reach` of the tile, a rectangle of the anchor grid found by integer
//                             arithmetic, in batches of DrawBatch::CAP = 128: thread c of the batch fetches candidate c's record into LDS slot c,
//                             with a NaN box where its box misses the tile, and after a barrier every thread walks the slots -- a broadcast read of
//                             the box, a reject against its four pixels, a reject per pixel -- keeping per pixel the smallest squared distance
//                             to a segment.  clamp(c - sqrt(.)) does not increase with the distance, so the largest coverage over all arrows and
//                             segments is the coverage of the smallest distance, bit for bit: one sqrtf per pixel, any visiting order.
//                             The slots are not compacted: a tile at the default density has a dozen candidates, and a rejected one costs a
//                             walker one LDS read and four compares.  Candidates per tile: ((64 + 2 reach) / s + 1) x ((16 + 2 reach) / s + 1), any
//                             number of batches, so spacing 1 (an anchor per pixel) is a loop and not a cap;
//                          3. the store: 4-pixel vector stores where W % 4 == 0 and image and output are aligned, scalars otherwise.
// Segments are (start, unit direction, length) and not two end points: the distance then needs no division, and the three lengths are per-image
// constants.  Every validity test is a positive comparison, so NaN fails it.  Every output pixel depends on its own image and fields only.
#include <math.h>
#include <stdint.h>

#include <algorithm>

#include "../../include/pf_hip.h"
#include "gather.h"

namespace pf {

namespace {

__device__ __forceinline__ bool is_finite(float x) { return fabsf(x) < INFINITY; }

// one component of the latitude gradient: central where both neighbours are finite (outside the image: NaN), else one-sided, else 0
__device__ __forceinline__ float lat_diff(float prev, float cur, float next) {
  const bool hp = is_finite(prev), hn = is_finite(next);
  return hp && hn ? (next - prev) * 0.5f : hn ? next - cur : hp ? cur - prev : 0.f;
}

// squared distance of p to the segment that starts at b and runs the length l along the unit vector e
__device__ __forceinline__ float seg_dist2(float px, float py, float bx, float by, float ex, float ey, float l) {
  const float rx = px - bx, ry = py - by;
  const float t = fminf(fmaxf(rx * ex + ry * ey, 0.f), l);
  const float dx = rx - t * ex, dy = ry - t * ey;
  return dx * dx + dy * dy;
}

__device__ __forceinline__ void over(float* v, float cov, const float* c) {
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) v[ch] = (1.f - cov) * v[ch] + cov * c[ch];
}

}  // namespace

__global__ __launch_bounds__(256) void draw_arrows_kernel(DrawBatch db) {
  const int o = blockIdx.y;
  const int nx = db.nx[o], na = nx * db.ny[o];  // < 2^31: at most the image's pixels
  const int a = blockIdx.x * 256 + threadIdx.x;
  if (a >= na) return;
  const int s = db.spacing, W = db.W[o];
  const int j = a / nx, i = a - j * nx;
  const int pr = j * s + s / 2, pc = i * s + s / 2;  // inside the image: the host counted nx and ny so
  const size_t npx = (size_t)db.H[o] * W, idx = (size_t)pr * W + pc;
  const float ux = db.up[o][idx], uy = db.up[o][npx + idx], la = db.lat[o][idx];
  const float l2 = fmaf(ux, ux, uy * uy);
  float4* __restrict__ r = db.rec[o] + (size_t)a * DrawBatch::REC;
  if (!(l2 >= 1e-12f && l2 < INFINITY && is_finite(la))) {
    r[0] = r[1] = r[2] = make_float4(0.f, 0.f, 0.f, 0.f);
    r[3] = make_float4(NAN, NAN, NAN, NAN);
    return;
  }
  const float inv = 1.f / sqrtf(l2);
  const float ex = ux * inv, ey = uy * inv;
  const float ax = (float)pc + 0.5f, ay = (float)pr + 0.5f;
  const float L = db.len[o], Lb = PF_DRAW_HEAD_RATIO * L;
  const float tx = ax + L * ex, ty = ay + L * ey;
  const float cs = PF_DRAW_HEAD_COS, sn = PF_DRAW_HEAD_SIN;
  const float mx = -ex, my = -ey;
  const float e1x = mx * cs - my * sn, e1y = mx * sn + my * cs;  // R(+angle)(-u)
  const float e2x = mx * cs + my * sn, e2y = my * cs - mx * sn;  // R(-angle)(-u)
  const float b1x = tx + Lb * e1x, b1y = ty + Lb * e1y, b2x = tx + Lb * e2x, b2y = ty + Lb * e2y;
  const float pad = 0.5f * db.line_width + 1.f;  // coverage ends at line_width / 2 + 1/2 from a segment: half a pixel to spare
  r[0] = make_float4(ax, ay, ex, ey);
  r[1] = make_float4(tx, ty, 1.f, 0.f);
  r[2] = make_float4(e1x, e1y, e2x, e2y);
  r[3] = make_float4(fminf(fminf(ax, tx), fminf(b1x, b2x)) - pad, fminf(fminf(ay, ty), fminf(b1y, b2y)) - pad,
                     fmaxf(fmaxf(ax, tx), fmaxf(b1x, b2x)) + pad, fmaxf(fmaxf(ay, ty), fmaxf(b1y, b2y)) + pad);
}

template <typename T>
__global__ __launch_bounds__(256) void draw_fields_kernel(DrawBatch db) {
  __shared__ float4 rec[DrawBatch::CAP][DrawBatch::REC];
  const int o = blockIdx.y;
  const int H = db.H[o], W = db.W[o];
  const int tiles_x = (W - 1) / 64 + 1, tiles_y = (H - 1) / 16 + 1;
  if (blockIdx.x >= (unsigned)(tiles_x * tiles_y)) return;  // the whole block: a smaller image of the launch
  const int tile_x = blockIdx.x % tiles_x, tile_y = blockIdx.x / tiles_x;
  const int row = tile_y * 16 + threadIdx.x / 16;
  const int col0 = tile_x * 64 + (threadIdx.x % 16) * 4;
  const bool active = row < H && col0 < W;  // an idle thread loads and stores nothing and keeps to the barriers
  const bool vec = db.vec[o] != 0;
  const size_t npx = (size_t)H * W, pix = (size_t)row * W + col0;

  float v[4][3];
#pragma unroll
  for (int k = 0; k < 4; ++k) v[k][0] = v[k][1] = v[k][2] = 0.f;
  if (active) {
    const T* img = static_cast<const T*>(db.img[o]) + pix * 3;  // may be the output: a thread reads its own pixels before it writes them
    if (vec) {
      if constexpr (sizeof(T) == 1) {
        const uint32_t* p = reinterpret_cast<const uint32_t*>(img);
        const uint32_t w[3] = {p[0], p[1], p[2]};
#pragma unroll
        for (int e = 0; e < 12; ++e) v[e / 3][e % 3] = (float)((w[e / 4] >> (8 * (e % 4))) & 255u);
      } else {
        const float4* p = reinterpret_cast<const float4*>(img);
        const float4 q0 = p[0], q1 = p[1], q2 = p[2];
        v[0][0] = q0.x; v[0][1] = q0.y; v[0][2] = q0.z; v[1][0] = q0.w;
        v[1][1] = q1.x; v[1][2] = q1.y; v[2][0] = q1.z; v[2][1] = q1.w;
        v[2][2] = q2.x; v[3][0] = q2.y; v[3][1] = q2.z; v[3][2] = q2.w;
      }
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (col0 + k >= W) break;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) v[k][ch] = texel(img, (size_t)(3 * k + ch));
      }
    }
  }

  if (active && (db.layers & PF_DRAW_LAT)) {
    const float* __restrict__ lat = db.lat[o];
    const float* __restrict__ up = db.up[o];
    constexpr float ramp[5][3] = PF_DRAW_RAMP;
    constexpr float line[3] = PF_DRAW_LINE_RGB;
    const float step = db.lat_step, alpha = db.alpha, lw = db.line_width;
    float lc[6], lu[4], ld[4];  // this row at the columns col0 - 1 ... col0 + 4, the rows above and below; NaN outside the image
    float ux4[4], uy4[4];
    if (db.fvec[o]) {  // W % 4 == 0 and aligned planes: five 16-byte loads and the two neighbours of the row
      const float4 nan4 = make_float4(NAN, NAN, NAN, NAN);
      const float4 c4 = *reinterpret_cast<const float4*>(lat + pix);
      const float4 u4 = row > 0 ? *reinterpret_cast<const float4*>(lat + pix - W) : nan4;
      const float4 d4 = row + 1 < H ? *reinterpret_cast<const float4*>(lat + pix + W) : nan4;
      const float4 x4 = *reinterpret_cast<const float4*>(up + pix), y4 = *reinterpret_cast<const float4*>(up + npx + pix);
      lc[0] = col0 > 0 ? lat[pix - 1] : NAN;
      lc[5] = col0 + 4 < W ? lat[pix + 4] : NAN;
      lc[1] = c4.x; lc[2] = c4.y; lc[3] = c4.z; lc[4] = c4.w;
      lu[0] = u4.x; lu[1] = u4.y; lu[2] = u4.z; lu[3] = u4.w;
      ld[0] = d4.x; ld[1] = d4.y; ld[2] = d4.z; ld[3] = d4.w;
      ux4[0] = x4.x; ux4[1] = x4.y; ux4[2] = x4.z; ux4[3] = x4.w;
      uy4[0] = y4.x; uy4[1] = y4.y; uy4[2] = y4.z; uy4[3] = y4.w;
    } else {
#pragma unroll
      for (int q = 0; q < 6; ++q) {
        const int c = col0 - 1 + q;
        lc[q] = (c >= 0 && c < W) ? lat[pix + q - 1] : NAN;
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const bool in = col0 + k < W;
        lu[k] = (in && row > 0) ? lat[pix - W + k] : NAN;
        ld[k] = (in && row + 1 < H) ? lat[pix + W + k] : NAN;
        ux4[k] = in ? up[pix + k] : 0.f;
        uy4[k] = in ? up[npx + pix + k] : 0.f;
      }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (col0 + k >= W) break;
      const float la = lc[k + 1], ux = ux4[k], uy = uy4[k];
      const float l2 = fmaf(ux, ux, uy * uy);
      if (!(l2 >= 1e-12f && l2 < INFINITY && is_finite(la))) continue;
      const float t = fminf(fmaxf((la + 90.f) / 45.f, 0.f), 4.f);
      const float fi = fminf(floorf(t), 3.f), f = t - fi;
      float c[3];
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) {
        const float lo = fi == 0.f ? ramp[0][ch] : fi == 1.f ? ramp[1][ch] : fi == 2.f ? ramp[2][ch] : ramp[3][ch];
        const float hi = fi == 0.f ? ramp[1][ch] : fi == 1.f ? ramp[2][ch] : fi == 2.f ? ramp[3][ch] : ramp[4][ch];
        c[ch] = (1.f - f) * lo + f * hi;
      }
      over(v[k], alpha, c);
      const float gx = lat_diff(lc[k], la, lc[k + 2]), gy = lat_diff(lu[k], la, ld[k]);
      const float g = sqrtf(gx * gx + gy * gy);
      if (g >= PF_DRAW_GRAD_FLOOR) {
        const float level = step * rintf(la / step);
        const float d = fabsf(la - level) / g;
        const float wl = level == 0.f ? 2.f * lw : lw;
        over(v[k], fminf(fmaxf(0.5f + 0.5f * wl - d, 0.f), 1.f), line);
      }
    }
  }

  const int nx = db.nx[o], ny = db.ny[o];
  if ((db.layers & PF_DRAW_UP) && nx > 0 && ny > 0) {  // the same for the whole block
    const int s = db.spacing;
    const long long reach = db.reach[o], half = s / 2;
    const int x0 = tile_x * 64, x1 = min(x0 + 64, W), y0 = tile_y * 16, y1 = min(y0 + 16, H);  // the tile's pixels [x0, x1) x [y0, y1)
    // anchor pixels i s + half in [x0 - reach, x1 - 1 + reach], likewise down: those further away draw nothing in the tile
    const long long lo_x = x0 - reach - half, hi_x = x1 - 1 + reach - half, lo_y = y0 - reach - half, hi_y = y1 - 1 + reach - half;
    const int i_lo = lo_x <= 0 ? 0 : (int)min((lo_x + s - 1) / s, (long long)nx);
    const int j_lo = lo_y <= 0 ? 0 : (int)min((lo_y + s - 1) / s, (long long)ny);
    const int i_hi = hi_x < 0 ? -1 : (int)min(hi_x / s, (long long)nx - 1);
    const int j_hi = hi_y < 0 ? -1 : (int)min(hi_y / s, (long long)ny - 1);
    const int ni = max(i_hi - i_lo + 1, 0), nj = max(j_hi - j_lo + 1, 0);
    const int ncand = ni * nj;  // <= nx ny < 2^31
    const float fx0 = (float)x0, fx1 = (float)x1, fy0 = (float)y0, fy1 = (float)y1;
    const float py = (float)row + 0.5f, pxmin = (float)col0 + 0.5f, pxmax = (float)col0 + 3.5f;
    const float L = db.len[o], Lb = PF_DRAW_HEAD_RATIO * L;
    float best[4] = {INFINITY, INFINITY, INFINITY, INFINITY};  // smallest squared distance to a segment of an arrow
    for (int base = 0; base < ncand; base += DrawBatch::CAP) {
      const int cnt = min((int)DrawBatch::CAP, ncand - base);
      __syncthreads();  // the previous batch has been walked
      if ((int)threadIdx.x < cnt) {
        const int c = base + threadIdx.x, jj = c / ni, ii = c - jj * ni;
        const float4* __restrict__ r = db.rec[o] + ((size_t)(j_lo + jj) * nx + (size_t)(i_lo + ii)) * DrawBatch::REC;
        const float4 box = r[3];
        if (box.x <= fx1 && box.z >= fx0 && box.y <= fy1 && box.w >= fy0) {  // false for the NaN box of an anchor without an arrow
          rec[threadIdx.x][0] = r[0];
          rec[threadIdx.x][1] = r[1];
          rec[threadIdx.x][2] = r[2];
          rec[threadIdx.x][3] = box;
        } else {
          rec[threadIdx.x][3] = make_float4(NAN, NAN, NAN, NAN);
        }
      }
      __syncthreads();
      if (active) {
        for (int q = 0; q < cnt; ++q) {
          const float4 box = rec[q][3];
          if (!(box.x <= pxmax && box.z >= pxmin && box.y <= py && box.w >= py)) continue;
          const float4 a = rec[q][0], tp = rec[q][1], e = rec[q][2];
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            const float px = pxmin + (float)k;
            if (!(px >= box.x && px <= box.z)) continue;
            const float d2 = fminf(seg_dist2(px, py, a.x, a.y, a.z, a.w, L),
                                   fminf(seg_dist2(px, py, tp.x, tp.y, e.x, e.y, Lb), seg_dist2(px, py, tp.x, tp.y, e.z, e.w, Lb)));
            best[k] = fminf(best[k], d2);
          }
        }
      }
    }
    const float c0 = 0.5f + 0.5f * db.line_width;
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (best[k] < INFINITY) over(v[k], fminf(fmaxf(c0 - sqrtf(best[k]), 0.f), 1.f), db.rgb);
  }

  if (!active) return;  // after the last barrier
  T* out = static_cast<T*>(db.out[o]) + pix * 3;
  if (vec) {
    if constexpr (sizeof(T) == 1) {
      uint32_t w[3] = {0u, 0u, 0u};
#pragma unroll
      for (int e = 0; e < 12; ++e) w[e / 4] |= round_u8(v[e / 3][e % 3]) << (8 * (e % 4));
      uint32_t* p = reinterpret_cast<uint32_t*>(out);
      p[0] = w[0]; p[1] = w[1]; p[2] = w[2];
    } else {
      store_rgb4(out, v);
    }
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (col0 + k >= W) break;
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) store_px(out + 3 * k + ch, v[k][ch]);
    }
  }
}

void launch_draw_fields(const DrawBatch& db, int dtype, hipStream_t s) {
  const dim3 block(256);
  if ((db.layers & PF_DRAW_UP) && db.max_anchors > 0)
    hipLaunchKernelGGL(draw_arrows_kernel, dim3((unsigned)(((size_t)db.max_anchors + 255) / 256), (unsigned)db.n), block, 0, s, db);
  const dim3 grid((unsigned)db.max_tiles, (unsigned)db.n);
  if (dtype == PF_PANO_U8) hipLaunchKernelGGL(draw_fields_kernel<uint8_t>, grid, block, 0, s, db);
  else hipLaunchKernelGGL(draw_fields_kernel<float>, grid, block, 0, s, db);
}

}  // namespace pf
