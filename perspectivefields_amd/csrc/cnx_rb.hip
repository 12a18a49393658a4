// Row-block fused ConvNeXt block MLP for the 384- / 768-channel stages on gfx950 (convnext.py:49-58):
//     y += ls * pwconv2( GELU( pwconv1( LayerNorm(d) ) ) )
// cnx_mlp.hip keeps a wave's rows and its y accumulators in registers, which ends at C = 192 (96 + 96 registers).  Here a BLOCK owns the rows, in the row-block form
// of rb_common.h: 64 rows (C = 384) or 32 rows (C = 768) are LayerNorm'ed while staged and stay in LDS as split-f16 fragments (A1) for the whole kernel; the hidden
// map is produced 128 columns at a time and never leaves the CU:
//   GEMM 1  RbGeo<1, false, RT>, K = C: every wave owns one 32-column tile of the hidden chunk; in the transposed accumulators a lane holds 16 hidden values of its
//           own row(s) -> weight scale, bias, erf-GELU, fp16 split, written as the A fragments of this chunk (A2, 8 k16 chunks);
//   barrier
//   GEMM 2  RbGeo<C / 128, false, RT>, K = 128: all C output columns, y^T accumulated in registers over all hidden chunks (6 accumulators per wave);
//   barrier (in front of the NEXT chunk's A2 writes, i.e. behind its GEMM 1: nobody waits there for long).
// One weight stream in execution order, [chunk t: W1 pass (C/16 steps of 4 tiles), W2 K-slice (8 steps of C/32 tiles)] ..., read by two register rings (the two GEMMs
// have different tile counts per step): each ring skips the other GEMM's part of the stream, and its look-ahead for chunk t + 1 is issued in the last RB_D steps of
// its GEMM of chunk t, so the loads are in flight through the other GEMM, the GELU phase and the barriers.  The K loops have no barrier and no LDS write.
// LDS: A1 99 840 / 101 376 B, A2 33 280 / 16 896 B, tables (inv1, b1 [4C], inv2, b2 [C]) 15 360 / 30 720 B = 148 480 / 148 992 B of 160 KB.  The epilogue's
// transposition scratch (4 KB per wave) is the dead A2 region.
// No atomics on results, fixed summation order; a row's result does not depend on its position in the block or on the other rows.
#include <stdlib.h>

#include "rb_common.h"

namespace pf {

template <int C>
__global__ __launch_bounds__(256, 1) void cnx_rb_kernel(const CnxRbArgs p) {
  static_assert(C == 384 || C == 768, "geometry: 64 x 384 or 32 x 768 row blocks");
  constexpr int RT = C == 384 ? 2 : 1, ROWS = 32 * RT;
  using G1 = RbGeo<1, false, RT>;
  using G2 = RbGeo<C / 128, false, RT>;
  constexpr int H = 4 * C, HC = G1::COLS, NCH = H / HC, KC = C / 16, KC2 = HC / 16;
  constexpr int CHS = G1::CHS;
  constexpr int TPR = 256 / ROWS;  // staging threads per row (thread = row tid / TPR, chunks (tid % TPR) + TPR i)
  constexpr int CPT = KC / TPR;
  constexpr int TAB = 2 * H + 2 * C, TAB4 = TAB / 4, NTL = (TAB4 + 255) / 256;
  constexpr int D1 = C == 384 ? 2 * RB_D : RB_D;  // ring depth of GEMM 1: its steps are 3 RT MFMAs short, RB_D of them cover 770 cycles at RT = 2 (C = 768 has no registers left)
  constexpr unsigned W1_BYTES = KC * G1::STEP_BYTES, W2_BYTES = KC2 * G2::STEP_BYTES;
  static_assert(HC == 128 && G2::COLS == C && G2::CHS == CHS && KC % TPR == 0 && KC % D1 == 0 && D1 % 2 == 0 && KC2 == 2 * RB_D, "geometry");
  static_assert(KC2 * CHS >= 4 * 4096, "the epilogue's scratch lives in the A2 region");
  static_assert(G1::RT == G2::RT && !G1::EXTRA && !G2::EXTRA && sizeof(RbA<G1>) == sizeof(RbA<G2>),
                "GEMM 2's last look-ahead is handed to GEMM 1 register by register: RbA<G1> and RbA<G2> must be the same fragments");
  __shared__ __attribute__((aligned(16))) unsigned char As1[KC * CHS];
  __shared__ __attribute__((aligned(16))) unsigned char As2[KC2 * CHS];
  __shared__ __attribute__((aligned(16))) float tabs[TAB];  // inv1 [H], b1 [H], inv2 [C], b2 [C]
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l31 = lane & 31, hi = lane >> 5;
  const int m0 = blockIdx.x * ROWS;
  const int nrows = min(ROWS, p.M - m0);

  RbW<G1, D1> W1;
  RbW<G2> W2;
  W1.init(p.w, p.w_bytes, wave, lane);
  W2.init(p.w, p.w_bytes, wave, lane);
  W2.voff += W1_BYTES;

  {  // ---- rows -> LayerNorm (passes over the registers, like F.layer_norm: mean, then the variance of the centred row; gamma / beta applied here) -> split-f16 fragments
    const int r = tid / TPR, q = tid % TPR;
    const float* xr = p.d + (size_t)(m0 + min(r, nrows - 1)) * C;  // rows past the block's end: a valid row, never stored
    float4 v[CPT][4];
#pragma unroll
    for (int i = 0; i < CPT; ++i)
#pragma unroll
      for (int e = 0; e < 4; ++e) v[i][e] = *reinterpret_cast<const float4*>(xr + 16 * (q + TPR * i) + 4 * e);
    // everything the block needs first is in flight at once: its rows, the per-channel tables, the first steps of GEMM 1's ring
    float4 tv[NTL];
#pragma unroll
    for (int j = 0; j < NTL; ++j) tv[j] = reinterpret_cast<const float4*>(p.tab)[min(tid + 256 * j, TAB4 - 1)];
    W1.prologue();
    // mean in two steps: the rounding error of the first (a sum of C values of the row's magnitude) is taken out by the mean of the centred row, so a constant row
    // is centred to exactly zero and a row with a large common offset keeps its small deviations (1 / sqrt(var + 1e-6) amplifies what is left by up to 1000)
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < CPT; ++i)
#pragma unroll
      for (int e = 0; e < 4; ++e) s += (v[i][e].x + v[i][e].y) + (v[i][e].z + v[i][e].w);
#pragma unroll
    for (int o = 1; o < TPR; o *= 2) s += __shfl_xor(s, o);
    const float mu0 = s / (float)C;
    float s1 = 0.f;
#pragma unroll
    for (int i = 0; i < CPT; ++i)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        v[i][e] = make_float4(v[i][e].x - mu0, v[i][e].y - mu0, v[i][e].z - mu0, v[i][e].w - mu0);
        s1 += (v[i][e].x + v[i][e].y) + (v[i][e].z + v[i][e].w);
      }
#pragma unroll
    for (int o = 1; o < TPR; o *= 2) s1 += __shfl_xor(s1, o);
    const float mu = s1 / (float)C;
    float ss = 0.f;
#pragma unroll
    for (int i = 0; i < CPT; ++i)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        v[i][e] = make_float4(v[i][e].x - mu, v[i][e].y - mu, v[i][e].z - mu, v[i][e].w - mu);
        ss = fmaf(v[i][e].x, v[i][e].x, fmaf(v[i][e].y, v[i][e].y, fmaf(v[i][e].z, v[i][e].z, fmaf(v[i][e].w, v[i][e].w, ss))));
      }
#pragma unroll
    for (int o = 1; o < TPR; o *= 2) ss += __shfl_xor(ss, o);
    const float rs = 1.0f / sqrtf(ss * (1.0f / C) + p.ln_eps);
#pragma unroll
    for (int i = 0; i < CPT; ++i) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float4 g = *reinterpret_cast<const float4*>(p.ln_g + 16 * (q + TPR * i) + 4 * e), b = *reinterpret_cast<const float4*>(p.ln_b + 16 * (q + TPR * i) + 4 * e);
        v[i][e] = make_float4(fmaf(v[i][e].x * rs, g.x, b.x), fmaf(v[i][e].y * rs, g.y, b.y), fmaf(v[i][e].z * rs, g.z, b.z), fmaf(v[i][e].w * rs, g.w, b.w));
      }
      rb_store_chunk(As1 + (q + TPR * i) * CHS, r, v[i]);
    }
#pragma unroll
    for (int j = 0; j < NTL; ++j)
      if (tid + 256 * j < TAB4) reinterpret_cast<float4*>(tabs)[tid + 256 * j] = tv[j];
  }
  W2.prologue();  // first used behind GEMM 1 of chunk 0; issued with the rows it would be 192 more live registers in the staging phase at C = 768 (spills)
  __syncthreads();

  f32x16 acc2[G2::NACC];
#pragma unroll
  for (int i = 0; i < G2::NACC; ++i)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc2[i][e] = 0.f;
  RbA<G1> A1[2];
  RbA<G2> A2[2];
  A1[0].read(As1, lane, 0);
#pragma unroll 1
  for (int t = 0; t < NCH; ++t) {
    // ---- GEMM 1: hidden chunk t (128 columns) of the resident rows
    f32x16 acc1[G1::NACC];
#pragma unroll
    for (int i = 0; i < G1::NACC; ++i)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc1[i][e] = 0.f;
#pragma unroll 1
    for (int s = 0; s < KC; s += D1) {
      if (s == KC - D1) W1.voff += W2_BYTES;  // the ring's next D1 steps belong to chunk t + 1: behind this chunk's W2 slice
#pragma unroll
      for (int d = 0; d < D1; ++d) {
        const int nx = s + d + 1 == KC ? 0 : s + d + 1;
        rb_step<G1>(acc1, W1, d, A1[d & 1], A1[(d + 1) & 1], As1 + nx * CHS, lane, 0);
      }
    }
    __syncthreads();  // every wave is behind GEMM 2 of chunk t - 1: A2 may be overwritten
    // ---- weight scale, bias, GELU, split: lane = row rt 32 + l31, register 4 g + e of tile rt = hidden column 32 wave + 8 g + 4 hi + e of the chunk
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int n = t * HC + wave * 32 + 8 * g + 4 * hi;
        const float4 iv = *reinterpret_cast<const float4*>(tabs + n), bb = *reinterpret_cast<const float4*>(tabs + H + n);
        const float4 hv = make_float4(gelu_erf(fmaf(acc1[rt][4 * g], iv.x, bb.x)), gelu_erf(fmaf(acc1[rt][4 * g + 1], iv.y, bb.y)),
                                      gelu_erf(fmaf(acc1[rt][4 * g + 2], iv.z, bb.z)), gelu_erf(fmaf(acc1[rt][4 * g + 3], iv.w, bb.w)));
        uint2 h, l;
        split4_f16(hv, h, l);
        unsigned char* dst = As2 + (2 * wave + (g >> 1)) * CHS + rt * 2048 + (l31 + 32 * (g & 1)) * 16 + 8 * hi;
        *reinterpret_cast<uint2*>(dst) = h;
        *reinterpret_cast<uint2*>(dst + 1024) = l;
      }
    __syncthreads();
    // ---- GEMM 2: y^T += W2[:, chunk t] hidden^T
    A2[0].read(As2, lane, 0);
#pragma unroll
    for (int s = 0; s < KC2; ++s) {
      if (s == KC2 - RB_D) W2.voff += W1_BYTES;  // chunk t + 1's slice lies behind its W1 pass
      rb_step<G2>(acc2, W2, s % RB_D, A2[s & 1], A2[(s + 1) & 1], s + 1 < KC2 ? As2 + (s + 1) * CHS : As1, lane, 0);
    }
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
      for (int pl = 0; pl < 2; ++pl) A1[0].a[rt][pl] = A2[0].a[rt][pl];  // the last step's look-ahead read chunk 0 of the resident rows
  }
  __syncthreads();  // A2 is dead: the epilogue's scratch

  // ---- epilogue: every 32 x 32 tile takes a turn through 4 KB of wave-private LDS and leaves as full 128-byte lines (rb_gemm.hip rb_epilogue_store); inv2, b2,
  // residual, saturation watch on the row-major side.  y is read and written by the same thread at the same place.
  {
    float* scratch = reinterpret_cast<float*>(As2) + wave * 1024;
    const float* tinv = tabs + 2 * H;
    const float* tb = tabs + 2 * H + C;
    const int rrow = lane >> 3, c4 = lane & 7;
    float4 rr[G2::NACC][4];
#pragma unroll
    for (int idx = 0; idx < G2::NACC; ++idx) {
      int rt, ct;
      bool own;
      rb_tile_of<G2>(idx, wave, rt, ct, own);
#pragma unroll
      for (int i = 0; i < 4; ++i) rr[idx][i] = *reinterpret_cast<const float4*>(p.y + (size_t)(m0 + min(rt * 32 + rrow + 8 * i, nrows - 1)) * C + ct * 32 + c4 * 4);
    }
#pragma unroll
    for (int idx = 0; idx < G2::NACC; ++idx) {
      int rt, ct;
      bool own;
      rb_tile_of<G2>(idx, wave, rt, ct, own);
#pragma unroll
      for (int g = 0; g < 4; ++g)
        *reinterpret_cast<float4*>(scratch + l31 * 32 + (((2 * g + hi) ^ (l31 & 7)) << 2)) = make_float4(acc2[idx][4 * g], acc2[idx][4 * g + 1], acc2[idx][4 * g + 2], acc2[idx][4 * g + 3]);
      __builtin_amdgcn_wave_barrier();
      const int n = ct * 32 + c4 * 4;
      const float4 iv = *reinterpret_cast<const float4*>(tinv + n), bb = *reinterpret_cast<const float4*>(tb + n);
      float4 v[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int row = rrow + 8 * i;
        v[i] = *reinterpret_cast<const float4*>(scratch + row * 32 + ((c4 ^ (row & 7)) << 2));
      }
      __builtin_amdgcn_wave_barrier();  // the next tile's writes stay behind this tile's reads
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int ml = rt * 32 + rrow + 8 * i;
        const float4 w = make_float4(fmaf(v[i].x, iv.x, bb.x) + rr[idx][i].x, fmaf(v[i].y, iv.y, bb.y) + rr[idx][i].y, fmaf(v[i].z, iv.z, bb.z) + rr[idx][i].z,
                                     fmaf(v[i].w, iv.w, bb.w) + rr[idx][i].w);
        if (own && ml < nrows) {
          if (p.sat) sat_watch4(p.sat, p.sat_limit, w.x, w.y, w.z, w.w);  // the residual stream feeds the next block's depthwise conv (ConvParams::sat)
          *reinterpret_cast<float4*>(p.y + (size_t)(m0 + ml) * C + n) = w;
        }
      }
    }
  }
}

bool cnx_rb_supported(int C) { return C == 384 || C == 768; }
int cnx_rb_rows(int C) { return C == 384 ? 64 : 32; }

void launch_cnx_rb(const CnxRbArgs& a, int C, hipStream_t s) {
  const int rows = cnx_rb_rows(C);
  const dim3 grid((unsigned)((a.M + rows - 1) / rows)), block(256);
  if (C == 384) hipLaunchKernelGGL((cnx_rb_kernel<384>), grid, block, 0, s, a);
  else if (C == 768) hipLaunchKernelGGL((cnx_rb_kernel<768>), grid, block, 0, s, a);
}

}  // namespace pf
