// Objects pasted into background pictures under a similarity and a placement read from device memory (include/pf_hip.h pf_composite, DESIGN.md
// section 29).  Memory bound -- most of a launch is a copy --, no MFMA, no LDS, no atomics, no inline assembly; every offset into an image or a
// plane is 64-bit.
//   composite_prep_kernel   one thread per job of the launch: the job's row of d_place -> a CompositeJob record in the workspace: the activity flag,
//                           cos phi and sin phi (fp64 from remainder(phi, 360), exactly 0 or +-1 at the multiples of 90) and 1 / s rounded to fp32
//                           once, the integer box and the box clipped to the background.  The trigonometry runs once per job, not per pixel.
//   composite_kernel<T>     grid (blocks of 256 threads) x (jobs of the launch).  The contiguous image is a flat array of pixels and a thread owns
//                           four consecutive ones: 12 bytes (uint8: three 4-byte words) or 48 bytes (fp32: three 16-byte words) that it moves as raw
//                           bits, so that a pixel nothing covers keeps the background's bits, NaN payloads included.  A pixel inside the job's
//                           clipped box runs the S x S sub-sample loop and replaces its bits where the coverage is not 0.  A job whose image and
//                           output are not aligned for the wide accesses, and the last thread of an image whose pixels are no multiple of 4, move
//                           their pixels channel by channel.
// Model (the contract; tests/test_composite_ref.py states it in fp64).  Background (H, W), object (h, w) with alpha in [0, 1] (NULL: 1; NaN: 0), row
// (s, phi, row, col, h', w').  Output pixel (R, C), r' = R - row, c' = C - col; outside [0, h') x [0, w') the background.  Inside, sub-sample (a, b),
// a-major: d = (c' + (b + 1/2) / S - w'/2, r' + (a + 1/2) / S - h'/2), source position (x, y) = (w/2, h/2) + R(-phi) d / s - (1/2, 1/2) in fp32 with
// field_xform_kernel's three fmaf; four bilinear taps; a tap outside the array is transparent (kept in the mean as nothing), a tap whose alpha is 0 is
// skipped; A_ab = sum w_k alpha_k, P_ab = sum (w_k alpha_k) c_k in fp64; A and P their means over the S^2 sub-samples.  Soft edge:
// cov = opacity A, out = bg (1 - cov) + opacity P.  Hard edge: where A >= 1/2, cov = opacity and out = bg (1 - opacity) + opacity P / A, else cov = 0.
// cov = 0: the background's bits.  The blend is fp64 and rounded once: to fp32, or half up and clamped to uint8 (gather.h round_u8's rule).
#include <math.h>
#include <stdint.h>

#include <algorithm>

#include "../../include/pf_hip.h"
#include "gather.h"

namespace pf {

namespace {

// uint8 of an fp64 value: round_u8's rule -- half up, clamped to [0, 255] -- without a rounding to fp32 before it
__device__ __forceinline__ uint32_t round_u8(double v) { return (uint32_t)fmin(fmax(floor(v + 0.5), 0.0), 255.0); }

__device__ __forceinline__ bool whole(double v) { return v == floor(v); }  // false for NaN

// the premultiplied colour P[3] and the alpha A of one output pixel of the box: the means over the S x S sub-samples
template <typename T>
__device__ __forceinline__ void composite_sample(const T* __restrict__ obj, const float* __restrict__ alpha, int h, int w, const CompositeJob& j, float fr, float fc,
                                                 int S, double* A_out, double* P_out) {
  const float fS = (float)S;
  const float hx = 0.5f * (float)j.wb, hy = 0.5f * (float)j.hb;
  const float cx = 0.5f * (float)w - 0.5f, cy = 0.5f * (float)h - 0.5f;
  double A = 0.0, P[3] = {0.0, 0.0, 0.0};
  for (int a = 0; a < S; ++a) {
    const float dy = (fr + ((float)a + 0.5f) / fS) - hy;
    for (int b = 0; b < S; ++b) {
      const float dx = (fc + ((float)b + 0.5f) / fS) - hx;
      // R(-phi) d = (cos dx + sin dy, cos dy - sin dx)
      const float px = fmaf(j.c, dx, j.s * dy), py = fmaf(j.c, dy, -(j.s * dx));
      const float x = fmaf(px, j.inv, cx), y = fmaf(py, j.inv, cy);
      if (!(x > -1.f && x < (float)w && y > -1.f && y < (float)h)) continue;  // every tap is outside: transparent (and a NaN position)
      const float xf = floorf(x), yf = floorf(y);
      const float ax = x - xf, ay = y - yf;  // exact
      const int x0 = (int)xf, y0 = (int)yf;  // in [-1, w - 1], [-1, h - 1]
      const float wx[2] = {1.f - ax, ax}, wy[2] = {1.f - ay, ay};
#pragma unroll
      for (int ty = 0; ty < 2; ++ty) {
#pragma unroll
        for (int tx = 0; tx < 2; ++tx) {
          const int xi = x0 + tx, yi = y0 + ty;
          if (!(xi >= 0 && xi < w && yi >= 0 && yi < h)) continue;
          const size_t q = (size_t)yi * w + xi;
          float al = alpha ? alpha[q] : 1.f;
          al = al > 0.f ? fminf(al, 1.f) : 0.f;  // NaN -> 0
          if (!(al > 0.f)) continue;             // the colour under a zero alpha is never read
          const double wa = (double)(wy[ty] * wx[tx]) * (double)al;  // exact: two fp32 factors
          A += wa;
#pragma unroll
          for (int ch = 0; ch < 3; ++ch) P[ch] += wa * (double)texel(obj, q * 3 + ch);
        }
      }
    }
  }
  const double n = (double)(S * S);
  *A_out = A / n;
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) P_out[ch] = P[ch] / n;
}

}  // namespace

__global__ __launch_bounds__(CompositeBatch::MAX) void composite_prep_kernel(CompositeBatch cb) {
  const int k = threadIdx.x;
  if (k >= cb.n) return;
  const double* __restrict__ p = cb.place + (size_t)(cb.first + k) * 6;
  const double s = p[0], phi = p[1], row = p[2], col = p[3], hb = p[4], wb = p[5];
  CompositeJob j;
  // every test is a positive comparison, so NaN fails it
  const bool active = s > 0.0 && s < INFINITY && fabs(phi) < INFINITY && fabs(row) < 0x1p30 && fabs(col) < 0x1p30 && whole(row) && whole(col) &&
                      hb >= 1.0 && hb < 0x1p31 && wb >= 1.0 && wb < 0x1p31 && whole(hb) && whole(wb);
  j.active = active ? 1 : 0;
  j.c = 1.f; j.s = 0.f; j.inv = 1.f;
  j.row = j.col = 0; j.hb = j.wb = 1;
  j.r0 = j.r1 = j.c0 = j.c1 = 0;  // an empty box: every pixel is the background's
  if (active) {
    const double a = remainder(phi, 360.0);  // exact, in [-180, 180]
    const double q = a / 90.0;
    double c, sn;
    if (q == floor(q)) {
      const int i = (int)q + 2;  // 0 ... 4
      c = i == 2 ? 1.0 : (i == 0 || i == 4) ? -1.0 : 0.0;
      sn = i == 1 ? -1.0 : i == 3 ? 1.0 : 0.0;
    } else {
      const double rad = a * (M_PI / 180.0);
      c = cos(rad); sn = sin(rad);
    }
    j.c = (float)c; j.s = (float)sn; j.inv = (float)(1.0 / s);
    const long long r = (long long)row, cc = (long long)col, H = cb.H[k], W = cb.W[k];
    j.row = (int)r; j.col = (int)cc; j.hb = (int)hb; j.wb = (int)wb;
    j.r0 = (int)min(max(r, 0LL), H); j.r1 = (int)min(max(r + (long long)hb, 0LL), H);
    j.c0 = (int)min(max(cc, 0LL), W); j.c1 = (int)min(max(cc + (long long)wb, 0LL), W);
  }
  cb.rec[cb.first + k] = j;
}

template <typename T>
__global__ __launch_bounds__(256) void composite_kernel(CompositeBatch cb) {
  constexpr int NW = sizeof(T) == 1 ? 3 : 12;  // 4-byte words of four pixels
  const int k = blockIdx.y;
  const int H = cb.H[k], W = cb.W[k];
  const size_t npx = (size_t)H * W;
  const size_t p0 = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4;
  if (p0 >= npx) return;
  const int cnt = (int)min((size_t)4, npx - p0);
  const bool vec = cb.vec[k] != 0 && cnt == 4;
  const T* __restrict__ bg = static_cast<const T*>(cb.bg[k]) + p0 * 3;
  T* __restrict__ out = static_cast<T*>(cb.out[k]) + p0 * 3;
  const CompositeJob j = cb.rec[cb.first + k];

  uint32_t wd[NW];
#pragma unroll
  for (int e = 0; e < NW; ++e) wd[e] = 0u;
  if (vec) {
    if constexpr (sizeof(T) == 1) {
      const uint32_t* p = reinterpret_cast<const uint32_t*>(bg);
      wd[0] = p[0]; wd[1] = p[1]; wd[2] = p[2];
    } else {
      const uint4* p = reinterpret_cast<const uint4*>(bg);
      const uint4 q0 = p[0], q1 = p[1], q2 = p[2];
      wd[0] = q0.x; wd[1] = q0.y; wd[2] = q0.z; wd[3] = q0.w;
      wd[4] = q1.x; wd[5] = q1.y; wd[6] = q1.z; wd[7] = q1.w;
      wd[8] = q2.x; wd[9] = q2.y; wd[10] = q2.z; wd[11] = q2.w;
    }
  } else {
#pragma unroll
    for (int e = 0; e < 12; ++e) {
      if (e < 3 * cnt) {
        if constexpr (sizeof(T) == 1) wd[e / 4] |= (uint32_t)bg[e] << (8 * (e % 4));
        else wd[e] = reinterpret_cast<const uint32_t*>(bg)[e];
      }
    }
  }

  float cov4[4] = {0.f, 0.f, 0.f, 0.f};
  const int R0 = (int)(p0 / (size_t)W), C0 = (int)(p0 - (size_t)R0 * W);
  // the four pixels lie in the rows R0 ... R0 + 3 at most (W >= 1); none of them meets an empty box
  const bool near = j.active && R0 < j.r1 && R0 >= j.r0 - 3;
  if (near) {
    int R = R0, C = C0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      if (q < cnt && R >= j.r0 && R < j.r1 && C >= j.c0 && C < j.c1) {
        double A, P[3];
        composite_sample(static_cast<const T*>(cb.obj[k]), cb.alpha[k], cb.h[k], cb.w[k], j, (float)(R - j.row), (float)(C - j.col), cb.samples, &A, P);
        double cov, keep;
        if (cb.hard) {
          const bool on = A >= 0.5;
          cov = on ? cb.opacity : 0.0;
          const double g = on ? cb.opacity / A : 0.0;
#pragma unroll
          for (int ch = 0; ch < 3; ++ch) P[ch] *= g;
        } else {
          cov = cb.opacity * A;
#pragma unroll
          for (int ch = 0; ch < 3; ++ch) P[ch] *= cb.opacity;
        }
        keep = 1.0 - cov;
        if (cov > 0.0) {
          cov4[q] = (float)cov;
#pragma unroll
          for (int ch = 0; ch < 3; ++ch) {
            const int e = 3 * q + ch;
            if constexpr (sizeof(T) == 1) {
              const double b = (double)((wd[e / 4] >> (8 * (e % 4))) & 255u);
              const uint32_t v = round_u8(b * keep + P[ch]);
              wd[e / 4] = (wd[e / 4] & ~(255u << (8 * (e % 4)))) | (v << (8 * (e % 4)));
            } else {
              wd[e] = __float_as_uint((float)((double)__uint_as_float(wd[e]) * keep + P[ch]));
            }
          }
        }
      }
      if (++C == W) { C = 0; ++R; }
    }
  }

  if (vec) {
    if constexpr (sizeof(T) == 1) {
      uint32_t* p = reinterpret_cast<uint32_t*>(out);
      p[0] = wd[0]; p[1] = wd[1]; p[2] = wd[2];
    } else {
      uint4* p = reinterpret_cast<uint4*>(out);
      p[0] = make_uint4(wd[0], wd[1], wd[2], wd[3]);
      p[1] = make_uint4(wd[4], wd[5], wd[6], wd[7]);
      p[2] = make_uint4(wd[8], wd[9], wd[10], wd[11]);
    }
  } else {
#pragma unroll
    for (int e = 0; e < 12; ++e) {
      if (e < 3 * cnt) {
        if constexpr (sizeof(T) == 1) out[e] = (uint8_t)((wd[e / 4] >> (8 * (e % 4))) & 255u);
        else reinterpret_cast<uint32_t*>(out)[e] = wd[e];
      }
    }
  }
  if (cb.cov[k]) {
    float* __restrict__ cv = cb.cov[k] + p0;
    if (cb.cvec[k] && cnt == 4) {
      *reinterpret_cast<float4*>(cv) = make_float4(cov4[0], cov4[1], cov4[2], cov4[3]);
    } else {
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if (q < cnt) cv[q] = cov4[q];
    }
  }
}

void launch_composite(const CompositeBatch& cb, int dtype, hipStream_t s) {
  hipLaunchKernelGGL(composite_prep_kernel, dim3(1), dim3(CompositeBatch::MAX), 0, s, cb);
  size_t npx = 0;
  for (int k = 0; k < cb.n; ++k) npx = std::max(npx, (size_t)cb.H[k] * cb.W[k]);
  const dim3 grid((unsigned)((npx + 1023) / 1024), (unsigned)cb.n), block(256);
  if (dtype == PF_PANO_U8) hipLaunchKernelGGL(composite_kernel<uint8_t>, grid, block, 0, s, cb);
  else hipLaunchKernelGGL(composite_kernel<float>, grid, block, 0, s, cb);
}

}  // namespace pf
