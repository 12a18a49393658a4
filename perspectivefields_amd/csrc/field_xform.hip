// Similarity transforms of perspective fields, and the best placement over (variant, offset) (include/pf_hip.h pf_fields_transform and pf_place_search,
// DESIGN.md section 26).  Memory bound, no MFMA, no atomics, no inline assembly; every offset into a plane is 64-bit.
//   field_xform_kernel      grid (blocks of 256 output pixels) x (jobs of the launch), one thread per output pixel.  The source position in fp32 from
//                           the job's cos phi, sin phi and 1 / s in the kernel arguments; four taps, each dropped when outside the array or invalid; the
//                           values in fp64 -- the products of fp32 weights and fp32 taps are exact there -- and rounded to fp32 once.
//   place_count_kernel      one block of 1024 threads per packed plane (place_pack_kernel's records): its valid pixels, an integer.
//   place_best_tile_kernel  grid (tiles of 256 placements) x (entries of the launch); an entry is the score map of one (pair, variant).  One thread per
//                           placement: the means and the pfd in fp64, +inf below the threshold; the block's lowest (pfd, placement) in lexicographic
//                           order by an LDS tree -> tile[]; block 0 of an entry also writes its BestHead.  A skipped variant has one tile of +inf.
//   place_best_pair_kernel  one block per pair: variant by variant the lowest of the variant's tiles -> d_var, the first lowest variant -> d_best.
// The order (pfd, placement) is total, so a minimum does not depend on the shape of the reduction: the bits depend on the pair's fields, the variants,
// the stride, the threshold and the weights only.
// Model of the transform (the contract; tests/test_placement_search_ref.py states it in fp64).  Source (h, w), variant (s, phi), output (h', w').  Output
// pixel (r', c'): d = (c' + 1/2 - w'/2, r' + 1/2 - h'/2); source position (x, y) = (w/2, h/2) + R(-phi) d / s - (1/2, 1/2) in pixel-centre
// coordinates; taps (floor y + {0, 1}, floor x + {0, 1}) with the bilinear weights, products of (1 - a_x, a_x) and (1 - a_y, a_y).  A tap counts when it
// is inside the array and valid by pf_place_scores' rule.  W_v = the weights of the taps that count; the pixel is valid iff W_v >= 1/2 and the mix
// m = sum w_k u_k, rounded to fp32, passes the length rule.  lat' = sum w_k lat_k / W_v; up' = R(phi) m scaled to unit length, and left as it is where
// its squared length is within 2^-22 of 1 already: a unit vector in fp32 keeps its bits, so s = 1, phi = 0 copies such a field.  Invalid: NaN x 3.
#include <math.h>
#include <stdint.h>

#include <algorithm>

#include "../../include/pf_hip.h"
#include "pf_kernels.h"

namespace pf {

namespace {

struct Best { double pfd; long long at; };
__device__ __forceinline__ bool before(const Best& a, const Best& b) { return a.pfd < b.pfd || (a.pfd == b.pfd && a.at < b.at); }

// the first of the block's 256 records in the order `before`, valid in thread 0; ends with a barrier, so the LDS can be used again
__device__ __forceinline__ Best block_first(Best v, double* sp, long long* sa) {
  const int t = threadIdx.x;
  sp[t] = v.pfd;
  sa[t] = v.at;
  __syncthreads();
  for (int half = 128; half > 0; half >>= 1) {
    if (t < half) {
      const Best a{sp[t], sa[t]}, b{sp[t + half], sa[t + half]};
      if (before(b, a)) { sp[t] = b.pfd; sa[t] = b.at; }
    }
    __syncthreads();
  }
  const Best r{sp[0], sa[0]};
  __syncthreads();
  return r;
}

}  // namespace

__global__ __launch_bounds__(256) void field_xform_kernel(FieldXform fx) {
  const int f = blockIdx.y;
  const int ho = fx.ho[f], wo = fx.wo[f];
  const size_t npo = (size_t)ho * wo;
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= npo) return;
  const int h = fx.h[f], w = fx.w[f];
  const size_t npx = (size_t)h * w;
  const float* __restrict__ up = fx.up[f];
  const float* __restrict__ lat = fx.lat[f];
  const int r = (int)(i / (size_t)wo), c = (int)(i - (size_t)r * wo);
  // exact for sides below 2^23: half-integers
  const float dx = ((float)c + 0.5f) - 0.5f * (float)wo, dy = ((float)r + 0.5f) - 0.5f * (float)ho;
  const float cs = fx.c[f], sn = fx.s[f], inv = fx.inv[f];
  // R(-phi) d = (cos dx + sin dy, cos dy - sin dx)
  const float px = fmaf(cs, dx, sn * dy), py = fmaf(cs, dy, -(sn * dx));
  const float x = fmaf(px, inv, 0.5f * (float)w - 0.5f), y = fmaf(py, inv, 0.5f * (float)h - 0.5f);
  float o_ux = NAN, o_uy = NAN, o_la = NAN;
  if (x > -1.f && x < (float)w && y > -1.f && y < (float)h) {  // otherwise every tap is outside (and a NaN position is invalid)
    const float xf = floorf(x), yf = floorf(y);
    const float ax = x - xf, ay = y - yf;  // exact
    const int x0 = (int)xf, y0 = (int)yf;  // in [-1, w - 1], [-1, h - 1]
    const float wx[2] = {1.f - ax, ax}, wy[2] = {1.f - ay, ay};
    double Wv = 0.0, mx = 0.0, my = 0.0, ml = 0.0;
#pragma unroll
    for (int ty = 0; ty < 2; ++ty) {
#pragma unroll
      for (int tx = 0; tx < 2; ++tx) {
        const int xi = x0 + tx, yi = y0 + ty;
        const bool inside = xi >= 0 && xi < w && yi >= 0 && yi < h;
        const size_t q = inside ? (size_t)yi * w + xi : 0;
        const float ux = up[q], uy = up[npx + q], la = lat[q];
        const float l2 = fmaf(ux, ux, uy * uy);
        const bool valid = inside && l2 >= 1e-12f && l2 < INFINITY && fabsf(la) < INFINITY;
        const double wk = (double)(wy[ty] * wx[tx]);
        if (valid) {  // in tap order; a product of two fp32 numbers is exact in fp64
          Wv += wk;
          mx += wk * (double)ux;
          my += wk * (double)uy;
          ml += wk * (double)la;
        }
      }
    }
    const float mxf = (float)mx, myf = (float)my;
    const float m2 = fmaf(mxf, mxf, myf * myf);
    if (Wv >= 0.5 && m2 >= 1e-12f && m2 < INFINITY) {
      const double rx = (double)cs * mx - (double)sn * my, ry = (double)sn * mx + (double)cs * my;  // R(phi) m; exact for (cos, sin) in {0, +-1}
      const double l2 = rx * rx + ry * ry;
      const double k = fabs(l2 - 1.0) <= 0x1p-22 ? 1.0 : 1.0 / sqrt(l2);
      o_ux = (float)(rx * k);
      o_uy = (float)(ry * k);
      o_la = (float)(ml / Wv);
    }
  }
  float* __restrict__ ou = fx.out_up[f];
  ou[i] = o_ux;
  ou[npo + i] = o_uy;
  fx.out_lat[f][i] = o_la;
}

__global__ __launch_bounds__(1024) void place_count_kernel(BestCount bc) {
  __shared__ int sc[1024];
  const int f = blockIdx.x, t = threadIdx.x;
  const float2* __restrict__ pl = bc.plane[f];
  const size_t npx = (size_t)bc.npx[f];
  int n = 0;
#pragma unroll 4
  for (size_t i = t; i < npx; i += 1024) {  // one block per plane: 1024 threads and four loads in flight each, as latency is all there is to hide
    const float th = pl[i].x;
    n += th == th ? 1 : 0;
  }
  sc[t] = n;
  __syncthreads();
  for (int half = 512; half > 0; half >>= 1) {
    if (t < half) sc[t] += sc[t + half];
    __syncthreads();
  }
  if (t == 0) *bc.cnt[f] = sc[0];
}

__global__ __launch_bounds__(BestBatch::TILE) void place_best_tile_kernel(BestBatch bb) {
  __shared__ double sp[BestBatch::TILE];
  __shared__ long long sa[BestBatch::TILE];
  const BestEntry& e = bb.e[blockIdx.y];
  const int tiles = max(1, (int)(((long long)e.np + BestBatch::TILE - 1) / BestBatch::TILE));
  if ((int)blockIdx.x >= tiles) return;  // the whole block
  const int cnt = *e.cnt;
  const long long p = (long long)blockIdx.x * BestBatch::TILE + threadIdx.x;
  Best b{INFINITY, -1};
  if (p < (long long)e.np) {  // np = 0 for a skipped variant
    const double* __restrict__ m = e.map + (size_t)p * 3;
    const double n = m[2];
    const double um = m[0] / n, lm = m[1] / n;
    // three roundings, as the composition of separate tensor operations has them: no contraction
    const double v = __dadd_rn(__dmul_rn(bb.w_up, um), __dmul_rn(bb.w_lat, lm));
    if (n >= __dmul_rn(bb.min_valid, (double)cnt) && n > 0.0 && v < INFINITY) b = Best{v, p};
  }
  b = block_first(b, sp, sa);
  if (threadIdx.x == 0) {
    bb.tile[(size_t)e.tile0 + blockIdx.x] = BestTile{b.pfd, b.at};
    if (blockIdx.x == 0) bb.head[e.head] = BestHead{e.map, e.tile0, tiles, e.Q, cnt, e.ho, e.wo};
  }
}

__global__ __launch_bounds__(256) void place_best_pair_kernel(int n_var, int stride, const BestHead* __restrict__ head, const BestTile* __restrict__ tile,
                                                              double* __restrict__ d_best, double* __restrict__ d_var) {
  __shared__ double sp[256];
  __shared__ long long sa[256];
  const int pair = blockIdx.x;
  Best best{INFINITY, -1};  // used by thread 0
  int best_v = -1;
  for (int v = 0; v < n_var; ++v) {
    const BestHead hd = head[(size_t)pair * n_var + v];
    Best b{INFINITY, -1};
    for (int t = threadIdx.x; t < hd.tiles; t += 256) {
      const BestTile bt = tile[(size_t)hd.tile0 + t];
      const Best c{bt.pfd, bt.at};
      if (before(c, b)) b = c;
    }
    b = block_first(b, sp, sa);
    if (threadIdx.x == 0) {
      double* __restrict__ o = d_var + ((size_t)pair * n_var + v) * 6;
      const long long j = b.at < 0 ? -1 : b.at / hd.Q, i = b.at < 0 ? -1 : b.at - j * hd.Q;
      o[0] = b.pfd;
      o[1] = b.at < 0 ? -1.0 : (double)(j * stride);
      o[2] = b.at < 0 ? -1.0 : (double)(i * stride);
      o[3] = (double)hd.cnt;
      o[4] = (double)hd.ho;
      o[5] = (double)hd.wo;
      if (b.pfd < best.pfd) { best = b; best_v = v; }  // strictly: the lowest variant of equal ones stays
    }
  }
  if (threadIdx.x != 0) return;
  double* __restrict__ o = d_best + (size_t)pair * 7;
  if (best_v < 0) {
    o[0] = INFINITY; o[1] = NAN; o[2] = NAN; o[3] = 0.0; o[4] = -1.0; o[5] = -1.0; o[6] = -1.0;
    return;
  }
  const BestHead hd = head[(size_t)pair * n_var + best_v];
  const double* __restrict__ m = hd.map + (size_t)best.at * 3;
  const long long j = best.at / hd.Q, i = best.at - j * hd.Q;
  o[0] = best.pfd;
  o[1] = m[0] / m[2];
  o[2] = m[1] / m[2];
  o[3] = m[2];
  o[4] = (double)best_v;
  o[5] = (double)(j * stride);
  o[6] = (double)(i * stride);
}

void launch_field_xform(const FieldXform& fx, hipStream_t s) {
  size_t npo = 0;
  for (int f = 0; f < fx.n; ++f) npo = std::max(npo, (size_t)fx.ho[f] * fx.wo[f]);
  const dim3 grid((unsigned)((npo + 255) / 256), (unsigned)fx.n), block(256);
  hipLaunchKernelGGL(field_xform_kernel, grid, block, 0, s, fx);
}

void launch_place_count(const BestCount& bc, hipStream_t s) {
  hipLaunchKernelGGL(place_count_kernel, dim3((unsigned)bc.n), dim3(1024), 0, s, bc);
}

void launch_place_best_tiles(const BestBatch& bb, hipStream_t s) {
  const dim3 grid((unsigned)bb.max_tiles, (unsigned)bb.n), block(BestBatch::TILE);
  hipLaunchKernelGGL(place_best_tile_kernel, grid, block, 0, s, bb);
}

void launch_place_best_pairs(int n_pair, int n_var, int stride, const BestHead* head, const BestTile* tile, double* d_best, double* d_var, hipStream_t s) {
  hipLaunchKernelGGL(place_best_pair_kernel, dim3((unsigned)n_pair), dim3(256), 0, s, n_var, stride, head, tile, d_best, d_var);
}

}  // namespace pf
