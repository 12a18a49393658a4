// Transport of perspective fields between cameras of one centre and onto equirectangular panoramas (include/pf_hip.h pf_reproject_fields /
// pf_compose_fields): the field counterparts of reproject.hip and pano_compose.hip.  Latitude is a property of the ray, so it is
// resampled; an up vector is a tangent direction, so it is lifted to the sphere at the source, rotated, and pushed to the destination's image plane
// through the closed-form differential of field_transport.h.  Gravity does not enter: only the relative rotation M that reproject.hip builds.
// VALU and memory bound, no MFMA, no atomics, no inline assembly; plain C++ stores; every offset into a plane is 64-bit.
//   reproject_fields_kernel       grid (tiles per output) x (outputs of the group), 256 threads, a thread owns 4 adjacent pixels of a 64 x 16 tile
//                                 (GatherDims).  Lane 0 computes the output's constants (M, both intrinsics, both xi, z_min, the linspace scales, the
//                                 finiteness of the 14 parameters) into LDS once per block.
//   compose_fields_kernel<FEATHER> grid (tiles per panorama) x (panoramas of the launch).  Threads v < count compute the constants of view v of the
//                                 block's panorama into LDS once per block; a thread keeps (S, L, U) of its 4 pixels in registers over the views.
// Model (the contract; tests/test_field_transport_ref.py states it in fp64).  Taps: a sample at (u, v) in index units reads (floor v + {0, 1},
// floor u + {0, 1}) with the bilinear weights; a tap counts when it is inside the array and valid by pf_place_scores' rule (finite latitude,
// 1e-12 <= |u|^2 < inf); taps are not clamped; W = the weights that count, sums in tap order (row-major) in fp32.
//   views -> views, destination pixel (row, col):
//     up   steps 1-5 of pf_reproject at (col + 1/2, row + 1/2): X_d, X_s = M X_d, (a_s, b_s); taps at (a_s - 1/2, b_s - 1/2): W_u, m = sum w_k u_k;
//          valid iff step 5, W_u >= 1/2, |m|^2 >= 1e-12; t = usm_lift(X_s, m, xi_s), up' = normalise(usm_push(X_d, M^T t, xi_d))
//     lat  the same steps at the linspace point (col W / (W - 1), row H / (H - 1)); taps at (a_s (Ws - 1) / Ws, b_s (Hs - 1) / Hs): W_l;
//          valid iff step 5 and W_l >= 1/2; lat' = sum w_k lat_k / W_l
//     the pixel is written iff both are valid, else NaN x 3; a non-finite camera parameter makes the whole output NaN
//   views -> panorama, pixel (row, col), D / lon / lat of pf_pano_compose; view i in the caller's order: steps 1-5 of pf_pano_compose give X, (a, b),
//     d > 0, w_i; up taps at (a - 1/2, b - 1/2), latitude taps at (a (Ws - 1) / Ws, b (Hs - 1) / Hs); t = M_i^T usm_lift(X, m, xi_i),
//     p = (Wp / (2 pi) (t . e_lon) / cos lat, -Hp / pi (t . e_lat)), u_i = p / |p|; the view contributes iff covered, W_u >= 1/2, W_l >= 1/2,
//     |m|^2 >= 1e-12 and 1e-12 <= |p|^2 < inf.  S = sum w_i, L = sum w_i lat_i, U = sum w_i u_i in fp32 in view order; lat = L / S,
//     up = U / |U| where S > 0 and |U|^2 >= 1e-12, else NaN x 3; the weight output holds S.  A view with a non-finite parameter contributes nothing.
// Every comparison is a positive one: a NaN or infinite coordinate issues no load.  Every value depends on its own output's cameras and sources
// only: the same bits in any batch and on every run.
#include <math.h>
#include <stdint.h>

#include "../../include/pf_hip.h"
#include "cam_model.h"
#include "field_transport.h"
#include "pf_kernels.h"

namespace pf {

namespace {

constexpr float kTwoPi = 6.283185307179586f, kPi = 3.141592653589793f, kInv2Pi = 0.15915494309189535f, kInvPi = 0.3183098861837907f;
constexpr float kMinLen2 = 1e-12f;  // pf_place_scores' length rule

struct FieldReprojConsts {
  float M[9];  // destination camera -> source camera, row major
  float invFd, Cxd, Cyd, xid;
  float Fs, Cxs, Cys, xis, zmin;
  float sxd, syd;  // W / (W - 1), H / (H - 1): index -> pixel-edge units of the destination's latitude grid
  float sxs, sys;  // (Ws - 1) / Ws, (Hs - 1) / Hs: pixel-edge units -> index of the source's latitude grid
  int ok;          // 0: a non-finite camera parameter
};

struct FieldViewConsts {
  float M[9];  // world (yaw 0) -> the view's camera, row major
  float F, Cx, Cy, xi, zmin;
  float wmax, hmax;  // the view's size
  float wscale;      // 2 / min(Hs, Ws)
  float sxs, sys;    // (Ws - 1) / Ws, (Hs - 1) / Hs
  int ok;
};

struct TapSums { float W, mx, my, ml; };

// the four taps of a sample at (u, v), index units, of the planes up [2][Hs][Ws] and lat [Hs][Ws].  The caller has (u, v) inside [-1, Ws] x [-1, Hs];
// a tap outside the array reads element 0 and does not count
__device__ __forceinline__ TapSums field_taps(const float* __restrict__ up, const float* __restrict__ lat, int Hs, int Ws, float u, float v) {
  const float uf = floorf(u), vf = floorf(v);
  const float au = u - uf, av = v - vf;
  const int c = (int)uf, r = (int)vf;
  const size_t npx = (size_t)Hs * Ws;
  const float wx[2] = {1.f - au, au}, wy[2] = {1.f - av, av};
  TapSums s{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int ty = 0; ty < 2; ++ty) {
#pragma unroll
    for (int tx = 0; tx < 2; ++tx) {
      const int ci = c + tx, ri = r + ty;
      const bool inside = ci >= 0 && ci < Ws && ri >= 0 && ri < Hs;
      const size_t q = inside ? (size_t)ri * Ws + ci : 0;
      const float ux = up[q], uy = up[npx + q], la = lat[q];
      const float l2 = fmaf(ux, ux, uy * uy);
      const bool valid = inside && l2 >= kMinLen2 && l2 < INFINITY && fabsf(la) < INFINITY;
      const float wk = wy[ty] * wx[tx];
      if (valid) {
        s.W += wk;
        s.mx = fmaf(wk, ux, s.mx);
        s.my = fmaf(wk, uy, s.my);
        s.ml = fmaf(wk, la, s.ml);
      }
    }
  }
  return s;
}

// steps 1 to 5 of pf_reproject for the destination point (pa, pb) in pixel-edge units: false where the point is invalid
__device__ __forceinline__ bool reproj_point(const FieldReprojConsts& cc, float pa, float pb, float wmax, float hmax, float* Xd, float* Xs, float* a,
                                             float* b) {
  if (!usm_ray((pa - cc.Cxd) * cc.invFd, (pb - cc.Cyd) * cc.invFd, cc.xid, Xd)) return false;
  to_world(cc.M, Xd, Xs);
  if (!(Xs[2] > cc.zmin)) return false;
  float xs, ys;
  usm_project(Xs, cc.xis, &xs, &ys);
  *a = cc.Fs * xs + cc.Cxs;
  *b = cc.Fs * ys + cc.Cys;
  return *a >= 0.f && *a <= wmax && *b >= 0.f && *b <= hmax;  // false for NaN and infinities
}

// (ux, uy, lat) of 4 adjacent pixels of output `o`: 16-byte vectors with `vec`, otherwise scalars for the pixels inside the row
__device__ __forceinline__ void store_fields(float* __restrict__ up, float* __restrict__ lat, int vec, int o, int H, int W, int row, int col0,
                                             const float* ux, const float* uy, const float* la) {
  const size_t npx = (size_t)H * W, l = (size_t)o * npx + (size_t)row * W + col0;
  float* __restrict__ u0 = up + l + (size_t)o * npx;  // [n][2][H][W]
  if (vec) {
    *reinterpret_cast<float4*>(u0) = make_float4(ux[0], ux[1], ux[2], ux[3]);
    *reinterpret_cast<float4*>(u0 + npx) = make_float4(uy[0], uy[1], uy[2], uy[3]);
    *reinterpret_cast<float4*>(lat + l) = make_float4(la[0], la[1], la[2], la[3]);
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (col0 + k >= W) break;
      u0[k] = ux[k];
      u0[npx + k] = uy[k];
      lat[l + k] = la[k];
    }
  }
}

}  // namespace

__global__ __launch_bounds__(256) void reproject_fields_kernel(FieldReprojBatch rb) {
  __shared__ FieldReprojConsts cc;
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
    cc.sxd = (float)W / (float)(W - 1);
    cc.syd = (float)H / (float)(H - 1);
    cc.sxs = (float)(Ws - 1) / (float)Ws;
    cc.sys = (float)(Hs - 1) / (float)Hs;
    cc.ok = (all_finite(cs, 7) && all_finite(cd, 7)) ? 1 : 0;
  }
  __syncthreads();
  const int tpr = rb.d.tpr;  // threads per tile row; the tile is (4 tpr) x (256 / tpr) pixels
  const int tile_x = blockIdx.x % rb.d.tiles_x, tile_y = blockIdx.x / rb.d.tiles_x;
  const int row = tile_y * (256 / tpr) + threadIdx.x / tpr;
  const int col0 = tile_x * 4 * tpr + (threadIdx.x % tpr) * 4;
  if (row >= H || col0 >= W) return;
  const float* __restrict__ sup = rb.src.up[o];
  const float* __restrict__ slat = rb.src.lat[o];
  const float wmax = (float)Ws, hmax = (float)Hs;
  const float pb_c = (float)row + 0.5f, pb_l = (float)row * cc.syd;

  float ux[4], uy[4], la[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int col = col0 + k;
    ux[k] = uy[k] = la[k] = __builtin_nanf("");
    if (col >= W || !cc.ok) continue;
    float Xd[3], Xs[3], a, b;
    if (!reproj_point(cc, (float)col + 0.5f, pb_c, wmax, hmax, Xd, Xs, &a, &b)) continue;
    const TapSums su = field_taps(sup, slat, Hs, Ws, a - 0.5f, b - 0.5f);
    const float m2 = su.mx * su.mx + su.my * su.my;
    if (!(su.W >= 0.5f && m2 >= kMinLen2)) continue;
    float Yd[3], Ys[3], a2, b2;
    if (!reproj_point(cc, (float)col * cc.sxd, pb_l, wmax, hmax, Yd, Ys, &a2, &b2)) continue;
    const TapSums sl = field_taps(sup, slat, Hs, Ws, a2 * cc.sxs, b2 * cc.sys);
    if (!(sl.W >= 0.5f)) continue;
    float t[3], td[3], px, py;
    usm_lift(Xs, su.mx, su.my, cc.xis, t);
    rotate_t(cc.M, t, td);  // M^T: source camera -> destination camera
    usm_push(Xd, td, cc.xid, &px, &py);
    const float inv = 1.f / sqrtf(px * px + py * py);
    ux[k] = px * inv;
    uy[k] = py * inv;
    la[k] = sl.ml / sl.W;
  }
  store_fields(rb.up, rb.lat, rb.d.vec, o, H, W, row, col0, ux, uy, la);
}

template <bool FEATHER>
__global__ __launch_bounds__(256) void compose_fields_kernel(FieldComposeBatch cb) {
  __shared__ FieldViewConsts vc[FieldComposeBatch::MAX];
  const int p = blockIdx.y;
  const int H = cb.d.H, W = cb.d.W;
  const int first = cb.first[p], count = min(cb.count[p], (int)FieldComposeBatch::MAX);
  if ((int)threadIdx.x < count) {
    const int v = first + (int)threadIdx.x;
    const float* cam = cb.cam + (size_t)v * 7;
    const int Hs = cb.src.H[v], Ws = cb.src.W[v];
    FieldViewConsts& c = vc[threadIdx.x];
    float R[9], sy, cy;
    cam_rotation(cam[0], cam[1], R);
    sincosf(0.f - cam[2], &sy, &cy);
    for (int i = 0; i < 3; ++i) {  // M = R^T Y(-yaw)
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
    c.sxs = (float)(Ws - 1) / (float)Ws;
    c.sys = (float)(Hs - 1) / (float)Hs;
    c.ok = all_finite(cam, 7) ? 1 : 0;
  }
  __syncthreads();
  const int tpr = cb.d.tpr;  // threads per tile row; the tile is (4 tpr) x (256 / tpr) pixels
  const int tile_x = blockIdx.x % cb.d.tiles_x, tile_y = blockIdx.x / cb.d.tiles_x;
  const int row = tile_y * (256 / tpr) + threadIdx.x / tpr;
  const int col0 = tile_x * 4 * tpr + (threadIdx.x % tpr) * 4;
  if (row >= H || col0 >= W) return;

  float sl, cl;
  sincosf((0.5f - ((float)row + 0.5f) / (float)H) * kPi, &sl, &cl);
  const float kx = (float)W * kInv2Pi / cl, ky = (float)H * kInvPi;  // pixels per radian of longitude (on this row) and of latitude
  float so[4], co[4], S[4], L[4], Ux[4], Uy[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    sincosf((((float)(col0 + k) + 0.5f) / (float)W - 0.5f) * kTwoPi, &so[k], &co[k]);
    S[k] = L[k] = Ux[k] = Uy[k] = 0.f;
  }

  for (int i = 0; i < count; ++i) {
    const FieldViewConsts& c = vc[i];
    if (!c.ok) continue;
    const float* __restrict__ sup = cb.src.up[first + i];
    const float* __restrict__ slat = cb.src.lat[first + i];
    const int Hs = cb.src.H[first + i], Ws = cb.src.W[first + i];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (col0 + k >= W) continue;
      const float D[3] = {cl * so[k], 0.f - sl, cl * co[k]};
      float X[3];
      to_world(c.M, D, X);
      if (!(X[2] > c.zmin)) continue;
      float xs, ys;
      usm_project(X, c.xi, &xs, &ys);
      const float a = c.F * xs + c.Cx, b = c.F * ys + c.Cy;
      const float ra = c.wmax - a, rb = c.hmax - b;
      if (!(a > 0.f && ra > 0.f && b > 0.f && rb > 0.f)) continue;  // d > 0; false for NaN and infinities: no load without a point inside the view
      const float w = FEATHER ? fminf(fminf(fminf(a, ra), fminf(b, rb)) * c.wscale, 1.f) : 1.f;
      const TapSums su = field_taps(sup, slat, Hs, Ws, a - 0.5f, b - 0.5f);
      const float m2 = su.mx * su.mx + su.my * su.my;
      if (!(su.W >= 0.5f && m2 >= kMinLen2)) continue;
      const TapSums sv = field_taps(sup, slat, Hs, Ws, a * c.sxs, b * c.sys);
      if (!(sv.W >= 0.5f)) continue;
      float t[3], tw[3];
      usm_lift(X, su.mx, su.my, c.xi, t);
      rotate_t(c.M, t, tw);  // M^T: the view's camera -> world
      const float ta = tw[0] * co[k] - tw[2] * so[k];                         // t . e_lon
      const float tb = -(tw[1] * cl + sl * (tw[0] * so[k] + tw[2] * co[k]));  // t . e_lat
      const float px = kx * ta, py = -(ky * tb);
      const float p2 = px * px + py * py;
      if (!(p2 >= kMinLen2 && p2 < INFINITY)) continue;
      const float inv = 1.f / sqrtf(p2);
      S[k] += w;
      L[k] = fmaf(w, sv.ml / sv.W, L[k]);
      Ux[k] = fmaf(w, px * inv, Ux[k]);
      Uy[k] = fmaf(w, py * inv, Uy[k]);
    }
  }

  float ux[4], uy[4], la[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const float u2 = Ux[k] * Ux[k] + Uy[k] * Uy[k];
    const bool has = S[k] > 0.f && u2 >= kMinLen2;
    const float inv = 1.f / sqrtf(u2);
    ux[k] = has ? Ux[k] * inv : __builtin_nanf("");
    uy[k] = has ? Uy[k] * inv : __builtin_nanf("");
    la[k] = has ? L[k] / S[k] : __builtin_nanf("");
  }
  store_fields(cb.up, cb.lat, cb.d.vec, p, H, W, row, col0, ux, uy, la);
  if (cb.weight) {
    const size_t pix = (size_t)p * H * W + (size_t)row * W + col0;
    if (cb.d.vec) {
      *reinterpret_cast<float4*>(cb.weight + pix) = make_float4(S[0], S[1], S[2], S[3]);
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (col0 + k >= W) break;
        cb.weight[pix + k] = S[k];
      }
    }
  }
}

void launch_reproject_fields(const FieldReprojBatch& rb, hipStream_t s) {
  const dim3 grid((unsigned)(rb.d.tiles_x * rb.d.tiles_y), (unsigned)rb.d.n), block(256);
  hipLaunchKernelGGL(reproject_fields_kernel, grid, block, 0, s, rb);
}

void launch_compose_fields(const FieldComposeBatch& cb, int blend, hipStream_t s) {
  const dim3 grid((unsigned)(cb.d.tiles_x * cb.d.tiles_y), (unsigned)cb.d.n), block(256);
  if (blend == PF_BLEND_FEATHER) hipLaunchKernelGGL((compose_fields_kernel<true>), grid, block, 0, s, cb);
  else hipLaunchKernelGGL((compose_fields_kernel<false>), grid, block, 0, s, cb);
}

}  // namespace pf
