// Internal kernel-launcher interface of libpf_hip.so (gfx950 / CDNA4 only).
// All activations are NHWC in HBM, fp32 or (inputs of the split-bf16 GEMMs) three exact bf16 planes (sb_split.h); "tokens (B,N,C)" of the reference's MiT
// blocks are the same memory as NHWC maps, so none of the reference's ~200
// NCHW<->NLC round trips (mix_transformers.py:117-118,246,458,504-506) exist here.
#pragma once
#include <vector>
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace pf {

enum Act { ACT_NONE = 0, ACT_RELU = 1, ACT_GELU = 2 };
#if defined(__HIPCC__)
// saturation watch of a producer (ConvParams::sat): one v_max3 / v_max / compare per 4 outputs, an atomic only when the window is left.  NaN-aware: fmaxf drops a
// NaN operand, so the sum of the four values is tested too (NaN if any of them is NaN, or inf - inf) -- this is the form of every epilogue that is not at its
// register cap (Winograd, row-block layers, fused block MLPs): a Winograd layer whose clamp-free split (wino.hip split2_f16_nc) met a value beyond its window
// produces inf / NaN outputs, and those are counted HERE, at that layer's own output
__device__ __forceinline__ void sat_watch4(unsigned* sat, float limit, float a, float b, float c, float d) {
  const float mx = fmaxf(fmaxf(fabsf(a), fabsf(b)), fmaxf(fabsf(c), fabsf(d)));
  const float s = (a + b) + (c + d);
  if (!(mx <= limit) || s != s) atomicAdd(sat, 1u);
}
// the same with ONE running maximum per thread (two v_max3_f32 per 4 outputs, no temporaries: the epilogues of the GEMM tiles sit at their register caps) ...
__device__ __forceinline__ float sat_acc4(float amax, float a, float b, float c, float d) {
  return __builtin_fmaxf(__builtin_fmaxf(__builtin_fmaxf(amax, __builtin_fabsf(a)), __builtin_fabsf(b)), __builtin_fmaxf(__builtin_fabsf(c), __builtin_fabsf(d)));
}
// ... and one compare at the kernel's end.  SATURATION ONLY: a NaN output is dropped by fmaxf (+-inf is counted).  A NaN can only reach these tiles from a producer
// that was itself counted (an inf beyond every window, or the Winograd epilogue's NaN test above); non-finite values are otherwise the debug forward's business
__device__ __forceinline__ void sat_flush(unsigned* sat, float limit, float amax) {
  if (sat && amax > limit) atomicAdd(sat, 1u);
}
#endif
// Packed fp32 (v_pk_*_f32) whose LOW lane reads the HIGH half of src1 -- hipcc's horizontal reductions `v_pk_add_f32 d, x, x op_sel:[0,1] op_sel_hi:[1,0]`, packed scalar
// FMAs -- was exact alone and wrong in lanes 48..63 on MI355X while this library's kernels ran on another stream (profiles/r04_dw7_packed.md,
// profiles/r05_pk_opsel_beside.txt), which is what every forward with the deferred ParamNet branch is.  tests/test_host_logic.py scans the built library and allows NO such
// form anywhere.  Two remedies: translation units whose kernels hipcc packed that way (cnx_mlp / mit_mlp / rb_gemm / rb_chain) are compiled without the feature
// (build.py NO_PK_F32_FLAGS: every function of the unit, so inlining stays legal -- a per-kernel attribute left the device helpers outlined and their arrays in
// scratch); a single stand-alone kernel without helpers may carry this attribute instead.
#if defined(__HIP_DEVICE_COMPILE__)
#define PF_NO_PK_F32 __attribute__((target("no-packed-fp32-ops")))
#else
#define PF_NO_PK_F32  // host pass: the x86 target has no such feature
#endif
static constexpr int NT_F16X3 = 23;  // ConvParams::nterms value of the split-f16 scheme
// Split-plane tensors: every `plane` stride argument is (elements between consecutive planes, always even) | format bit:
// 0 = three exact bf16 planes (x == h + m + l), SB_FMT_F16 = the two fp16 planes of the split-f16 scheme (sb_split.h)
static constexpr size_t SB_FMT_F16 = 1;

// Implicit-GEMM convolution / GEMM on v_mfma_f32_32x32x2_f32.
//   y[m][n] = post( act( sum_k A[m][k] * Wp[n][k] + bias[n] ) + res1[m][n] + res2[m][n] )
// m = (b, oy, ox) output pixel, k = (ky, kx, ci) with ci fastest, A gathered on the fly
// from one NHWC tensor or from the channel-concat of two (x: C1 channels, x2: C2).
struct ConvPtrs {
  const float* x = nullptr;
  const float* x2 = nullptr;        // nullptr unless channel-concat input
  const float* w = nullptr;         // packed [Cout][KH][KWCp], KWCp = roundup(KW*Cin, 32), zero padded
  const unsigned short* w_sb = nullptr;  // same weights as 5 bf16 planes [5][Cout][KH][KWCp]: exact split h, m, l (h + m + l == w), then
                                         // round-to-nearest bf16(w) and round-to-nearest m for the reduced-precision modes
  // split-f16 scheme (sb_split.h NT_F16X3): weights scaled per output channel by a power of two (row maximum in
  // [2^13, 2^14)) as two fp16 planes [2][Cout][KH][KWCp]: wh = fp16(w S), wl = fp16(w S - wh); w_h16_inv_scale = 1 / S
  const unsigned short* w_h16 = nullptr;
  const float* w_h16_inv_scale = nullptr;  // [Cout]: applied to the accumulators before the bias
  // Winograd F(2x2, 3x3) form of a 3x3 / stride-1 conv (wino.hip): U = G g G^T, per-channel power-of-two scale, two fp16 planes in MFMA fragment order
  const unsigned short* w_wino = nullptr;
  const float* w_wino_inv = nullptr;       // [Cout]
  const float* bias = nullptr;      // [Cout] or nullptr
  const float* bias_tab = nullptr;  // [9][Cout]: bias per 3x3 border case (folded Linear->conv), overrides bias
  const float* res1 = nullptr;      // [M][Cout] or nullptr (may alias y)
  const float* res2 = nullptr;      // [M][Cout] or nullptr
  float* y = nullptr;               // [M][ldy], or nullptr when only the split planes are wanted
  // Fused regression prediction head (Cout == 32, tiles with BN == 32 only): instead of storing the 32-channel map, the
  // epilogue applies the 1x1 head to every pixel -- kind 1: linear_pred_gravity (32 -> 2) + F.normalize (gravity_head.py:117,
  // 190-193), kind 2: linear_pred_latitude (32 -> 1) + clamp(-1, 1) (latitude_head.py:118,189-192) -- and writes the NCHW
  // API output head_out plus its components of the ParamNet input head_pn ([M] float4: g0, g1, lat, 0; may be nullptr)
  // Fused LayerNorm of the INPUT rows (ConvParams::ln, 1x1 layers whose K loop covers the whole row): the weights carry the LayerNorm
  // gamma (W'[n][k] = W[n][k] gamma[k]), bias = b + W beta, and ln_colsum[n] = sum_k W'[n][k]; the kernel contracts the raw rows,
  // accumulates their mean / variance while staging them and applies  y = rstd (acc - mean colsum) + bias  in the epilogue
  const float* ln_colsum = nullptr; // [Cout]
  float* partial = nullptr;         // split-K: [splitk][M][ldy] raw partial sums (fp32 scratch owned by the caller)
  int head_kind = 0;
  const float* head_w = nullptr;    // [nout][32]
  const float* head_b = nullptr;    // [nout]
  float* head_out = nullptr;        // [B][nout][Ho*Wo]
  float* head_pn = nullptr;
  // split-bf16 activation format (sb_split.h): plane 0 of the same NHWC tensors as three exact bf16 planes.  When x_sb
  // is set the split-bf16 kernel copies its A operand instead of splitting it (x / x2 may then be nullptr).
  const unsigned short* x_sb = nullptr;
  const unsigned short* x2_sb = nullptr;
  unsigned short* y_sb = nullptr;   // additional (or only) output in split planes
};
struct ConvParams {
  ConvPtrs g[2];   // grouped launch: `groups` problems of identical shape (the two decoder heads) in one grid
  int groups = 1;
  int B, H, W, C1, C2, Cin;
  int KH, KW, stride, pad;
  int Ho, Wo, Cout;
  int KWC, KWCp;
  int M;
  int act;        // Act applied to (acc + bias)
  int post_relu;  // relu after the residual adds
  int ldy;        // row stride of y / res1 / res2 in floats (normally Cout)
  int nchw_out;   // 1: store y as [B][Cout][Ho*Wo] (API-visible logits), residuals unsupported
  int splitk = 1; // > 1: K is contracted in `splitk` slices by separate blocks (linear split tiles only) into g[].partial, then reduced with
                  // the epilogue (scale, bias, activation, res1, post_relu) by splitk_reduce_kernel -- deterministic (fixed summation order)
  int ups = 0;    // 1: x is stored at half resolution [B][H/2][W/2][C1]; the conv runs on its bilinear x2 up-sampling, interpolated
                  // while the input halo is staged (3x3 halo tiles of the split-f16 scheme only; x2, if any, is at full resolution)
  int ln = 0;     // 1: LayerNorm over the Cin input channels fused into this 1x1 layer (ConvPtrs::ln_colsum; linear split tiles, fp32 input,
                  // no concat, no split-K): mix_transformers.py:200 (norm2 -> fc1), :123-126 (sr norm -> kv), convnext.py:50-51 (norm -> pwconv1)
  float ln_eps = 0.f;
  int nterms = 6; // split kernels: partial products per element product -- NT_F16X3 (23): 2-way fp16 split, 3 products, fp32-class accuracy;
                  // 6: exact 3-way bf16 split, 6 products (fp32-accurate); 3 (bf16, ~16-bit operands); 1 (plain bf16)
  unsigned x_bytes, x2_bytes, w_bytes;  // buffer sizes for the hardware range check (< 2 GiB each)
  unsigned w_sb_plane_bytes;            // bytes of one bf16 weight plane
  size_t x_sb_plane = 0, x2_sb_plane = 0, y_sb_plane = 0;  // elements between consecutive planes of x_sb / x2_sb / y_sb
  // Always-on saturation watch (the engine's counter; in the op entry points what pf_op_set_saturation_watch set, nullptr by default): every producer of a tensor that a
  // split-f16 contraction will read counts the 16-byte groups of its output with an element beyond sat_limit (or NaN) into *sat -- one compare per group and, in a
  // healthy network, no atomic ever.  The limit is the CONSUMER's window: 65504, 65504 / 4 in front of a Winograd conv (wino.hip), 8188 / 4094 for the attention
  // operands q / kv (attn.hip).  A split-K launch is watched by its reduce kernel (igemm_sb.hip splitk_reduce_kernel), which writes the finished output.
  unsigned* sat = nullptr;
  float sat_limit = 65504.f;
  int wino_half = 1;  // Winograd launches: non-zero = the half-patch geometry where it applies (wino.hip), 0 = square patches always (PF_WINO_HALF: the engine sets what its
                      // pf_create read, the conv op entry points what conv_wino_half_env() says at the call)
  unsigned long long* stamps = nullptr;  // timing aid (wino.hip, PF_WINO_STAMPS=1 in pf_op_conv2d_bench): s_memtime stamps of block 17, [wave][128]
  // fills the derived fields (Ho, Wo, M, Cin, *_bytes) from the primary ones
  void finish() {
    Cin = C1 + C2;
    Ho = (H + 2 * pad - KH) / stride + 1;
    Wo = (W + 2 * pad - KW) / stride + 1;
    M = B * Ho * Wo;
    x_bytes = (unsigned)((size_t)B * (ups ? H / 2 : H) * (ups ? W / 2 : W) * C1 * 4);
    x2_bytes = (unsigned)((size_t)B * H * W * C2 * 4);
    w_bytes = (unsigned)((size_t)Cout * KH * KWCp * 4);
    w_sb_plane_bytes = (unsigned)((size_t)Cout * KH * KWCp * 2);
    ldy = Cout;
  }
};

void launch_conv(const ConvParams& p, hipStream_t s);
// tile choice is exposed for tests / tuning: -1 = auto
void launch_conv_tile(const ConvParams& p, int tile_id, hipStream_t s);
int conv_num_tiles();
int conv_tile_bm(int tile_id);
int conv_tile_bn(int tile_id);
bool conv_tile_is_sb(int tile_id);
bool conv_tile_usable(const ConvParams& p, int tile_id);
int conv_default_tile(const ConvParams& p);  // static choice (cost model) among the usable tiles  // split-bf16 tiles need pre-split weights and Cin % 32 == 0
// split-bf16 kernel family (igemm_sb.hip)
int conv_sb_num_tiles();
const char* conv_sb_tile_name(int id);
int conv_sb_tile_bm(int id);
int conv_sb_tile_bn(int id);
bool conv_sb_eligible(const ConvParams& p);
bool conv_sb_tile_ok(const ConvParams& p, int sb_tile);  // per-tile restrictions (the pipelined "sbd" tiles: fp32 operands, fp32-accurate mode)
int conv_sb_default_tile(const ConvParams& p);
void launch_conv_sb(const ConvParams& p, int sb_tile, hipStream_t s);
// split-K factor for a launch (1 = none): deep-K shapes whose 64x64 tiling gives too few blocks for 256 CUs (the MiT spatial-
// reduction convs: 3 200 rows, K up to 4 096); the caller allocates g[].partial = splitk * M * ldy floats and sets ConvParams::splitk
int conv_splitk_factor(const ConvParams& p);
int conv_splitk_factor(const ConvParams& p, int mode);  // the same with the caller's mode in place of PF_SPLITK (mode as in conv_splitk_shape)
int conv_splitk_shape(long M, int Cout, int KH, int KWCp, int groups, int mode);  // its shape-only part; mode = PF_SPLITK (conv_splitk_env): -1 default, 0 never, N > 1 forces the factor
int conv_wino_half_env();  // PF_WINO_HALF (default 1) as the environment has it NOW
int conv_splitk_env();  // PF_SPLITK as the environment has it NOW (pf_create reads it per engine, the op entry points per call: tests switch it inside one process)
// What the launchers of this thread really did (plain host increments, no device work): the decisions taken below the engine -- split-K after launch_conv_sb's
// own checks, the Winograd geometry -- for the engine's dispatch report (pf_last_dispatch), which takes the difference over one forward
struct LaunchCounts { long splitk = 0, splitk_max = 0, wino = 0, wino_half = 0; };
extern thread_local LaunchCounts g_launch_counts;
const char* conv_tile_name(int tile_id);
// Winograd F(2x2, 3x3) kernel (wino.hip; tiles "wino256x64d" / "wino256x64c" of the split family)
bool conv_wino_ok(const ConvParams& p);
void launch_conv_wino(const ConvParams& p, hipStream_t s, int variant = 0);  // 0: "wino256x64c", 1: "wino256x64d"
int conv_wino_blocks(const ConvParams& p);   // grid size of the shipped Winograd kernel for this launch (all groups; the half-patch geometry where it applies)
void wino_pack_weights(const float* packed /*[Cout][3][KWCp], k = (kx, ci)*/, int Cout, int Cin, int KWCp, std::vector<unsigned short>* planes, std::vector<float>* inv_scale);

// rows x C LayerNorm (biased variance), y may alias x
// Optional split-plane output (sb_split.h) of the elementwise / attention kernels: y_sb != nullptr writes the result as
// three bf16 planes `sb_plane` elements apart (in addition to y, or instead of it when y == nullptr).
void launch_layernorm(const float* x, const float* g, const float* b, float* y, long rows, int C, float eps, hipStream_t s,
                      unsigned short* y_sb = nullptr, size_t sb_plane = 0);

// depthwise 3x3 (pad 1) + bias + exact-erf GELU, NHWC, w packed [9][C]
void launch_dwconv3x3_gelu(const float* x, const float* w9c, const float* bias, float* y, int B, int H, int W, int C, hipStream_t s,
                           unsigned short* y_sb = nullptr, size_t sb_plane = 0);
void launch_dwconv3x3_gelu_variant(int variant, const float* x, const float* w9c, const float* bias, float* y, int B, int H, int W, int C, hipStream_t s,
                                   unsigned short* y_sb = nullptr, size_t sb_plane = 0);
// depthwise 7x7 (pad 3) + bias, NHWC, w packed [49][C]
void launch_dwconv7x7(const float* x, const float* w49c, const float* bias, float* y, int B, int H, int W, int C, hipStream_t s);
// variant 3 = column-blocked streaming kernel with nc columns per thread (4 / 2), nb row buffers (2 / 3), strips of th rows (0 = automatic); 2 = one column per lane
void launch_dwconv7x7_cfg(int variant, int nc, int nb, int th, const float* x, const float* w49c, const float* bias, float* y, int B, int H, int W, int C, hipStream_t s);

// spatial-reduction attention: q [B][N][C], kv [B][M][2C] (k | v), out [B][N][C]; head_dim 64, M <= 128
void launch_sr_attention(const float* q, const float* kv, float* out, int B, int N, int M, int heads, hipStream_t s,
                         unsigned short* out_sb = nullptr, size_t sb_plane = 0);

// variant 1: split-f16 MFMA (default); 0: exact fp32 MFMA
void launch_sr_attention_variant(int variant, const float* q, const float* kv, float* out, int B, int N, int M, int heads, hipStream_t s,
                                 unsigned short* out_sb = nullptr, size_t sb_plane = 0);

// The attention half of a one-head, 64-channel MiT block as one kernel (attn_block.hip): y = x + proj(softmax((LN1(x) Wq^T + bq) K^T / 8) V); y may alias x
struct MitAttn64Args {
  const float* x = nullptr;            // [B][N][64] token rows
  const float* kv = nullptr;           // [B][M][128] keys | values of the spatially reduced tokens
  float* y = nullptr;                  // [B][N][64]
  const unsigned short* wfr = nullptr; // attn64_pack: q and proj fragments
  const float* tab = nullptr;          // attn64_pack: LayerNorm-1 gamma / beta, inverse scales, biases
  int B = 0, N = 0, M = 0, QT = 1;
  float ln_eps = 1e-6f;
  unsigned* sat = nullptr;             // saturation watch: q against the attention window (8188), y against sat_limit
  float sat_limit = 65504.f;
};
bool mit_attn64_supported(int C, int heads, int kv_rows);
void launch_mit_attn64(const MitAttn64Args& a, int num_cus, hipStream_t s);
void attn64_pack(const float* ln_g, const float* ln_b, const float* q_w, const float* q_b, const float* p_w, const float* p_b, std::vector<unsigned short>* wfr, std::vector<float>* tab);

// The two 7 x 7 convolutions on the normalised image (stem7.hip): conv 7x7 / stride 2 or 4 / pad 3, 3 (stored as 4) -> 64 channels, + bias (folded BatchNorm), + ReLU or
// + LayerNorm over the 64 channels, one kernel
struct Stem7Args {
  const float* x = nullptr;            // [B][H][W][4] normalised image (channel 3 = 0)
  float* y = nullptr;                  // [B][Ho][Wo][64]
  const unsigned short* wfr = nullptr; // stem7x7_pack: weight fragments
  const float* tab = nullptr;          // stem7x7_pack: inverse scales, bias, LayerNorm gamma / beta
  int B = 0, H = 0, W = 0, Ho = 0, Wo = 0, stride = 2, relu = 0, ln = 0, QT = 1;
  float ln_eps = 1e-5f;
  unsigned* sat = nullptr;
  float sat_limit = 65504.f;
};
bool stem7x7_supported(int Cin, int Cout, int K, int stride, int pad);
void launch_stem7x7(const Stem7Args& a, int num_cus, hipStream_t s);
void stem7x7_pack(const float* w, const double* out_scale, const float* bias, const float* ln_g, const float* ln_b, std::vector<unsigned short>* wfr, std::vector<float>* tab);

// y = x W^T + b (+ res) for 128 -> 128 layers over many rows (thin_linear.hip): weights in LDS, rows as the MFMA's B operand, register epilogue; y may alias res
struct ThinLinArgs {
  const float* x = nullptr;            // [M][128]
  const float* res = nullptr;          // [M][128] or nullptr
  float* y = nullptr;                  // [M][128]
  const unsigned short* wfr = nullptr; // thin128_pack
  const float* tab = nullptr;
  long M = 0;
  int QT = 1;
  unsigned* sat = nullptr;
  float sat_limit = 65504.f;
};
bool thin128_supported(int K, int N);
void launch_thin128(const ThinLinArgs& a, int num_cus, hipStream_t s);
void thin128_pack(const float* w, const float* bias, std::vector<unsigned short>* wfr, std::vector<float>* tab);

// bilinear x2 (align_corners=False), NHWC
void launch_upsample2x(const float* x, float* y, int B, int H, int W, int C, hipStream_t s, unsigned short* y_sb = nullptr, size_t sb_plane = 0);

// fp32 [n] <-> three exact bf16 planes (n a multiple of 4)
void launch_split_planes(const float* x, unsigned short* y_sb, size_t sb_plane, long n, hipStream_t s);
void launch_merge_planes(const unsigned short* x_sb, size_t sb_plane, float* y, long n, hipStream_t s);
void launch_fill_random(float* p, long n, unsigned seed, float scale, hipStream_t s);
void launch_range_stats(const float* x, long n, float* out4 /*zeroed: max |x|, sum x^2, saturated, non-finite*/, hipStream_t s);

// input normalisation: uint8 NHWC BGR [B][320][320][3] or fp32 NCHW [B][3][320][320] -> fp32 NHWC4 (x-mean)/std, ch3=0
void launch_prep_u8(const uint8_t* in, float* out, long npix, const float* mean3, const float* std3, hipStream_t s);
void launch_prep_f32_nchw(const float* in, float* out, int B, int HW, const float* mean3, const float* std3, hipStream_t s);

// bit-exact PIL antialiased bilinear resize of one uint8 HxWx3 image to OHxOWx3 (two integer passes; tables from the host)
void launch_resize_u8(const uint8_t* in, int H, int W, uint8_t* tmp, uint8_t* out, int OH, int OW, const int* bh, const int* kh, int ksh,
                      const int* bv, const int* kv, int ksv, hipStream_t s);

// the same for up to ResizeBatch::MAX images in one launch pair (per-image pointers / sizes / tables in the kernel arguments)
struct ResizeBatch {
  static constexpr int MAX = 32;
  int n;
  int H[MAX], W[MAX], ksh[MAX], ksv[MAX];
  const uint8_t* in[MAX];
  uint8_t* tmp[MAX];
  uint8_t* out[MAX];
  const int* bh[MAX]; const int* kh[MAX];
  const int* bv[MAX]; const int* kv[MAX];
};
void launch_resize_batch_u8(const ResizeBatch& rb, int OH, int OW, hipStream_t s);

// regression prediction heads: 1x1 (32->2) + L2-normalise, 1x1 (32->1) + clamp; writes NCHW API outputs and the NHWC4 ParamNet input
void launch_pred_regression(const float* tg, const float* tl, const float* wg, const float* bg, const float* wl, const float* bl,
                            float* pred_g_nchw, float* pred_l_nchw, float* pn_in_nhwc4, int B, int HW, hipStream_t s);

// classification decode: argmax over channels of NCHW logits -> decoded fields (gravity (2,HW), latitude degrees (1,HW))
void launch_decode_cls(const float* logit_g, int ng, const float* logit_l, int nl, float* dec_g, float* dec_l, int B, int HW, hipStream_t s);

// post-process one image: gravity (2,h,w)*scale -> bilinear (H,W) -> normalise; latitude bilinear -> (asin->deg)
void launch_postprocess(const float* g2, const float* l1, int h, int w, float* up_out, float* lat_out, int H, int W, int lat_is_sin, hipStream_t s);

// the same for up to PostBatch::MAX images in one launch (per-image sizes / pointers in the kernel arguments)
struct PostBatch {
  static constexpr int MAX = 32;
  int n;
  int H[MAX], W[MAX];
  float rh[MAX], rw[MAX], sxs[MAX], sys[MAX];  // filled by launch_postprocess_batch
  const float* g2[MAX];
  const float* l1[MAX];
  float* up[MAX];
  float* lat[MAX];
};
void launch_postprocess_batch(PostBatch& pb, int h, int w, int lat_is_sin, hipStream_t s);

// nearest resize NHWC4 (ParamNetConvNextRegress input, param_network.py:197)
void launch_nearest_nhwc4(const float* x, float* y, int B, int H, int W, int Ho, int Wo, hipStream_t s);

// ConvNeXt tail: global average pool -> LN(C) -> Linear(C->nout); out [B][nout]
// Fused ConvNeXt block MLP (cnx_mlp.hip): y += ls * pwconv2(GELU(pwconv1(LayerNorm(d)))) for C = 96 / 192, hidden map in registers only.
// wpk / tab: packed by cnx_mlp_pack (host_pack.h)
bool cnx_mlp_supported(int C);
bool cnx_mlp_preferred(int C);  // the stages where the engine uses it
void launch_cnx_mlp(const float* d, float* y, const unsigned short* wpk, const float* tab, long M, int C, float eps, hipStream_t s, unsigned* sat = nullptr, float sat_limit = 65504.f);
// Row-block fused ConvNeXt block MLP (cnx_rb.hip, rb_common.h): the same block for C = 384 / 768 on blocks of 64 / 32 rows, hidden map in LDS only; d and y are
// different buffers.  w / tab: packed by cnx_rb_pack (host_pack.h); LayerNorm gamma / beta are applied while the rows are staged
struct CnxRbArgs {
  const float* d;            // [M][C] depthwise conv output
  float* y;                  // [M][C] residual stream, in and out
  const unsigned short* w;   // weight stream: [hidden chunk of 128: W1 pass, W2 K-slice] ...
  size_t w_bytes;
  const float* tab;          // inv1 [4C], b1 [4C], inv2 [C], b2 [C] (layer scale folded)
  const float* ln_g;
  const float* ln_b;
  float ln_eps;
  int M;
  unsigned* sat = nullptr;   // saturation watch of the residual stream (ConvParams::sat)
  float sat_limit = 65504.f;
};
bool cnx_rb_supported(int C);
int cnx_rb_rows(int C);      // rows per block
void launch_cnx_rb(const CnxRbArgs& a, int C, hipStream_t s);
// Fused MiT block Mlp (mit_mlp.hip): y = x + fc2(GELU(dwconv3x3(fc1(LayerNorm(x))))) for C = 64 / 128; x and y are different buffers.
// wpk / tab2: packed by mit_mlp_pack (host_pack.h), one chunk of mit_mlp_chunk_bytes(C) per 32 hidden units
bool mit_mlp_supported(int C);
bool mit_mlp_preferred(int C, int with128);  // the stages for which the engine builds its weights (with128 = Engine::mit_mlp128: smallest batch that takes the C = 128 form, 0 = never)
int mit_mlp_chunk_bytes(int C);
void launch_mit_mlp(const float* x, float* y, const unsigned short* wpk, const float* tab2, int B, int Hs, int Ws, int C, float eps, hipStream_t s, unsigned* sat = nullptr, float sat_limit = 65504.f);
// Row-block linear layers (rb_gemm.hip, rb_common.h): blocks of 64 token rows of one image, weights streamed from L2 into registers in MFMA fragment order
struct RbLinArgs {
  const float* x;            // [M][K] fp32 rows
  const float* ln_g;         // LayerNorm over K (nullptr: none)
  const float* ln_b;
  float ln_eps;
  const unsigned short* w;   // weight stream (rb_pack_w), N / COLS passes of K / 16 steps
  size_t w_bytes;
  const float* inv;          // [N] inverse weight scales
  const float* bias;         // [N]
  const float* res;          // [M][N] or nullptr (may alias y)
  float* y;                  // [M][N]
  int M, tokens, bpi;        // rows, tokens per image, blocks per image = ceil(tokens / 64)
  int N, act;
  // saturation watch of y against sat_limit (ConvParams::sat)
  unsigned* sat = nullptr;
  float sat_limit = 65504.f;
  unsigned long long* stamps = nullptr;  // timing aid (scripts/tune_rb.py, PF_RB_STAMPS=1): s_memtime stamps of block 17, [wave][64]
};
bool rb_linear_supported(int K, int N);
// The key / value branch of a MiT block with 2 x 2 spatial reduction in one launch (rb_chain.hip): kv = Linear(LN_sr(Conv2x2s2(LN_1(x)))), mix_transformers.py:119-127
struct RbSrKvArgs {
  const float* x;             // [B][2 Hr][2 Wr][C] token map (pre-norm1)
  const float* ln1_g; const float* ln1_b; float ln1_eps;
  const unsigned short* w;    // weight stream: the conv as a GEMM over K = (ky, kx, ci) (80 steps), then the kv layer's two 320-column passes (2 x 20 steps), RB_D pad steps
  size_t w_bytes;
  const float* sr_inv; const float* sr_bias;   // [C]
  const float* srn_g; const float* srn_b; float srn_eps;
  const float* kv_inv; const float* kv_bias;   // [2 C]
  float* kv;                  // [B][Hr Wr][2 C]
  int B, Hr, Wr, bpi;         // bpi = ceil(Hr Wr / 32) blocks per image
  unsigned* sat = nullptr;    // saturation watch of kv (ConvParams::sat; the attention kernel's window for k / v: 4094)
};
bool rb_srkv_supported(int C, int sr);
// The seam between the attention half and the Mlp half of a MiT block in one launch (rb_chain.hip): x += proj(attn_out); hidden = fc1(LayerNorm_2(x))
struct RbProjFc1Args {
  const float* attn;          // [M][C] attention output
  float* x;                   // [M][C] token stream: residual in, x1 out (in place)
  const unsigned short* w;    // weight stream: proj (C / 16 steps), then fc1's four 320-column passes, RB_D pad steps
  size_t w_bytes;
  const float* proj_inv; const float* proj_bias;   // [C]
  const float* ln2_g; const float* ln2_b; float ln2_eps;
  const float* fc1_inv; const float* fc1_bias;     // [4 C]
  float* hidden;              // [M][4 C]
  int B, tokens, bpi;         // bpi = ceil(tokens / 64)
  unsigned* sat = nullptr;    // saturation watch of x1 (against sat_limit) and hidden (against hidden_limit: the depthwise conv's input window), ConvParams::sat
  float sat_limit = 65504.f, hidden_limit = 65504.f;
};
void launch_rb_proj_fc1(const RbProjFc1Args& a, int C, hipStream_t s);
void launch_rb_srkv(const RbSrKvArgs& a, int C, hipStream_t s);
void launch_rb_linear(const RbLinArgs& a, int K, hipStream_t s);
void launch_gap_ln_head(const float* x, const float* g, const float* b, const float* w, const float* hb, float* out, int B, int HW, int C, int nout, float eps, hipStream_t s);

// camera parameters {roll, elevation (rad), focal_rel, cx_rel, cy_rel} (device) -> up [2][H][W], latitude [H][W] degrees
// (PanoCam.get_up_general / get_lat_general, utils/panocam.py:451-556)
void launch_fields_from_params(const float* cam5, int H, int W, float* up, float* lat, hipStream_t s);

// ParamNet scalar formulas (param_network.py:62-67): raw [B][nraw] -> [B][8] (layout: include/pf_hip.h)
void launch_paramnet_scalars(const float* raw, int nraw, float* out8, int B, int mode, hipStream_t s);

// perspective fields -> camera parameters: one Levenberg-Marquardt driver (fit_lm.h) over two camera models, each a traits type Fit.
//   PinholeFit (fit_camera.hip, include/pf_hip.h pf_fit_camera): theta [5] = roll, pitch, f, cx, cy; out [n][PF_FIT_COLS]
//   UsmFit (fit_camera_usm.hip, pf_fit_camera_usm): theta [6], the Unified Spherical Model's xi as one more parameter; out [n][PF_USMFIT_COLS]
// FitParams::free_pp selects the fit of all of theta (otherwise cx, cy are held: 3 / 4 parameters).  Up to FitBatch::MAX images per launch,
// per-image sizes and pointers in the kernel arguments; the strides of part, state, out and init are the model's
//   FisheyeFit<KIND, POLY> (fit_camera_fisheye.hip, pf_fit_fisheye): theta [7], a fisheye lens of the compile-time projection KIND with k1, k2; POLY: k1, k2 are
//   free, otherwise held: 3 / 5 parameters without POLY, 5 / 7 with it; out [n][PF_FISHFIT_COLS]
struct PinholeFit;
struct UsmFit;
template <int KIND, bool POLY>
struct FisheyeFit;
constexpr int FIT_STATE = 40, USMFIT_STATE = 48, FISHFIT_STATE = 64;  // Fit::STATE: doubles of per-image LM state
constexpr int FIT_REC = 24, USMFIT_REC = 32, FISHFIT_REC = 40;        // Fit::REC: doubles of one accumulate block's partial record
struct FitParams {
  int free_pp, loss;
  float huber_delta, w_up, w_lat;
  float theta_max;  // the fisheye fit alone: the widest half field of view with a model value, radians; behind the fields every fit reads
};
struct FitBatch {
  static constexpr int MAX = 32;
  int n;
  int H[MAX], W[MAX], nblk[MAX];
  const float* up[MAX];   // [2][H][W]
  const float* lat[MAX];  // [H][W] degrees
  double* part[MAX];      // [nblk][Fit::REC]
  double* state;          // [n][Fit::STATE]
  float* out;             // [n][Fit::COLS]
  const float* init;      // NULL or [n][Fit::NTH]
};
// accumulate blocks (= partial records) of an image: one per 4096 pixels, at most 256
inline int fit_blocks_per_image(int H, int W) {
  const long nb = ((long)H * W + 4095) / 4096;
  return (int)(nb < 1 ? 1 : nb > 256 ? 256 : nb);
}
template <class Fit>
void launch_fit_init(const FitBatch& fb, const FitParams& prm, hipStream_t s);
template <class Fit>
void launch_fit_iteration(const FitBatch& fb, const FitParams& prm, hipStream_t s);  // one accumulate + solve pair
// The fit with intrinsics shared across the images of a camera group (include/pf_hip.h pf_fit_camera_shared): init and accumulate as above over
// launch groups of FitBatch::MAX images, a per-image reduction into rec, then one solve per camera group.  Camera groups are consecutive images
// anywhere in the batch, of any length; up to FitGroups::MAX of them per launch, state / rec / out are those of the whole batch
struct FitGroups {
  static constexpr int MAX = 128;
  int n;
  int start[MAX], size[MAX];  // first image and number of images of each camera group
  double* state;              // [B][Fit::STATE]
  const double* rec;          // [B][Fit::REC]: every image's summed record at its trial parameters
  float* out;                 // [B][Fit::COLS]
};
template <class Fit>
void launch_fit_shared_start(const FitGroups& fg, hipStream_t s);  // after launch_fit_init: the group's shared start
template <class Fit>
void launch_fit_shared_accum(const FitBatch& fb, const FitParams& prm, double* rec, hipStream_t s);  // accumulate + reduction; rec: of fb's first image
template <class Fit>
void launch_fit_shared_solve(const FitGroups& fg, const FitParams& prm, hipStream_t s);
// camera parameters {roll, pitch (rad), focal_rel, cx_rel, cy_rel, xi} (device) -> up [2][H][W], latitude [H][W] degrees, NaN without a ray
void launch_fields_usm(const float* cam6, int H, int W, float* up, float* lat, hipStream_t s);

// The batched image gathers (gather.h): up to GatherSources::MAX outputs of one size per launch, grid (tiles per output) x (outputs), per-output source
// pointers and sizes in the kernel arguments.  Both arguments begin with the launch's shape
struct GatherDims {
  int n, H, W;                // outputs of this launch, their size
  int tpr, tiles_x, tiles_y;  // threads per tile row (the tile is 4 tpr x 256 / tpr pixels), tiles per output
  int vec;                    // 1: W % 4 == 0 and every output aligned for the 4-pixel vector stores (uint8 image and mask 4 bytes, the rest 16)
};
struct GatherSources {  // of each output of the launch
  static constexpr int MAX = 32;
  const void* p[MAX];  // (H, W, 3) uint8 or fp32
  int H[MAX], W[MAX];
};

// equirectangular panorama -> camera views + ground-truth fields (pano_crop.hip, include/pf_hip.h pf_pano_crop)
struct PanoBatch {
  static constexpr int MAX = GatherSources::MAX;
  GatherDims d;
  GatherSources src;  // the panoramas (Hp, Wp, 3)
  const float* cam;  // [n][7]: roll, pitch, yaw (radians), rel_focal, rel_cx, rel_cy, xi
  void* img;         // [n][H][W][3], the panorama's type
  float* up;         // NULL (no labels) or [n][2][H][W]
  float* lat;        // NULL or [n][H][W] degrees
};
void launch_pano_crop(const PanoBatch& pb, int dtype, hipStream_t s);

// image of one camera -> image of another camera of the same centre (reproject.hip, include/pf_hip.h pf_reproject)
struct ReprojBatch {
  static constexpr int MAX = GatherSources::MAX;
  GatherDims d;
  float fill;         // value of a pixel that sees nothing of its source
  GatherSources src;  // (Hs, Ws, 3)
  const float* cam_src;  // [n][7]: roll, pitch, yaw (radians), rel_focal, rel_cx, rel_cy, xi
  const float* cam_dst;  // [n][7]
  void* img;             // [n][H][W][3], the sources' type
  uint8_t* valid;        // NULL or [n][H][W]
  float* map;            // NULL or [n][2][H][W]: (a_s, b_s), NaN where not visible
};
void launch_reproject(const ReprojBatch& rb, int dtype, hipStream_t s);
// the kernel-argument layout both gathers were measured with
static_assert(sizeof(PanoBatch) == 576 && offsetof(PanoBatch, src) == 32, "PanoBatch layout");
static_assert(sizeof(ReprojBatch) == 584 && offsetof(ReprojBatch, fill) == 28 && offsetof(ReprojBatch, src) == 32, "ReprojBatch layout");

// equirectangular panorama -> rotated equirectangular panorama + the fields of the panoramic camera (pano_rotate.hip, include/pf_hip.h pf_pano_rotate)
struct PanoRotBatch {
  static constexpr int MAX = GatherSources::MAX;
  GatherDims d;
  int inverse;        // 0: A = Q = Y(yaw) R(roll, pitch); otherwise A = Q^T
  GatherSources src;  // the source panoramas (Hs, Ws, 3)
  const float* rot;   // [n][3]: roll, pitch, yaw (radians)
  void* img;          // [n][H][W][3], the sources' type
  float* up;          // NULL (no labels) or [n][2][H][W]
  float* lat;         // NULL or [n][H][W] degrees
};
void launch_pano_rotate(const PanoRotBatch& rb, int dtype, hipStream_t s);
static_assert(sizeof(PanoRotBatch) == 576 && offsetof(PanoRotBatch, inverse) == 28 && offsetof(PanoRotBatch, src) == 32, "PanoRotBatch layout");
// the labels alone (pf_pano_fields): no source
struct PanoFieldsBatch {
  static constexpr int MAX = GatherSources::MAX;
  GatherDims d;
  int inverse;
  const float* rot;  // [n][3]
  float* up;         // [n][2][H][W]
  float* lat;        // [n][H][W] degrees
};
void launch_pano_fields(const PanoFieldsBatch& fb, hipStream_t s);

// The supersampled forms of the three one-source gathers (gather_ss.hip, include/pf_hip.h pf_pano_crop_ss / pf_reproject_ss / pf_pano_rotate_ss):
// every output pixel is the mean of the valid ones of samples x samples sub-samples.  Arguments of their own, so that the layouts above stay as they
// were measured: the launch's shape, `samples` in the word behind it, the sources at offset 32, then what the parent's struct holds
struct PanoSsBatch {
  static constexpr int MAX = GatherSources::MAX;
  GatherDims d;
  int samples;        // S in [1, PF_GATHER_MAX_SAMPLES]
  GatherSources src;  // the panoramas (Hp, Wp, 3)
  const float* cam;   // [n][7], as PanoBatch
  void* img;
  float* up;
  float* lat;
};
void launch_pano_crop_ss(const PanoSsBatch& pb, int dtype, hipStream_t s);
struct ReprojSsBatch {
  static constexpr int MAX = GatherSources::MAX;
  GatherDims d;
  int samples;
  GatherSources src;  // (Hs, Ws, 3)
  float fill;
  const float* cam_src;  // [n][7], as ReprojBatch
  const float* cam_dst;
  void* img;
  uint8_t* valid;  // NULL or [n][H][W]: 1 where a sub-sample is valid
  float* map;      // NULL or [n][2][H][W]: (a_s, b_s) of the pixel centre
};
void launch_reproject_ss(const ReprojSsBatch& rb, int dtype, hipStream_t s);
struct PanoRotSsBatch {
  static constexpr int MAX = GatherSources::MAX;
  GatherDims d;
  int samples;
  GatherSources src;  // the source panoramas (Hs, Ws, 3)
  int inverse;
  const float* rot;  // [n][3], as PanoRotBatch
  void* img;
  float* up;
  float* lat;
};
void launch_pano_rotate_ss(const PanoRotSsBatch& rb, int dtype, hipStream_t s);
static_assert(offsetof(PanoSsBatch, samples) == 28 && offsetof(PanoSsBatch, src) == 32, "PanoSsBatch layout");
static_assert(offsetof(ReprojSsBatch, samples) == 28 && offsetof(ReprojSsBatch, src) == 32, "ReprojSsBatch layout");
static_assert(offsetof(PanoRotSsBatch, samples) == 28 && offsetof(PanoRotSsBatch, src) == 32, "PanoRotSsBatch layout");

// cube maps -> camera views and equirectangular panoramas (cube_gather.hip, include/pf_hip.h pf_cube_crop / pf_cube_to_pano): the sources are cubes
// (6, N, N, 3), src.H = src.W = N; `samples` as in the supersampled gathers
struct CubeCropBatch {
  static constexpr int MAX = GatherSources::MAX;
  GatherDims d;
  int samples;        // S in [1, PF_GATHER_MAX_SAMPLES]
  GatherSources src;  // the cubes
  const float* cam;   // [n][7], as PanoBatch
  void* img;          // [n][H][W][3], the cubes' type
};
void launch_cube_crop(const CubeCropBatch& cb, int dtype, hipStream_t s);
struct CubePanoBatch {
  static constexpr int MAX = GatherSources::MAX;
  GatherDims d;
  int samples;
  GatherSources src;  // the cubes
  int inverse;        // as PanoRotBatch
  const float* rot;   // [n][3]: roll, pitch, yaw (radians)
  void* img;
};
void launch_cube_to_pano(const CubePanoBatch& cb, int dtype, hipStream_t s);
static_assert(offsetof(CubeCropBatch, samples) == 28 && offsetof(CubeCropBatch, src) == 32, "CubeCropBatch layout");
static_assert(offsetof(CubePanoBatch, samples) == 28 && offsetof(CubePanoBatch, src) == 32, "CubePanoBatch layout");

// fisheye and dual-fisheye frames -> camera views and equirectangular panoramas (fisheye_gather.hip, include/pf_hip.h pf_fisheye_crop /
// pf_fisheye_to_pano): the sources are frames (Hs, Ws, 3), each output reads up to PF_FISHEYE_MAX_LENSES lenses of its one frame; `samples` as in
// the supersampled gathers
struct FisheyeCropBatch {
  static constexpr int MAX = GatherSources::MAX;
  GatherDims d;
  int samples;        // S in [1, PF_GATHER_MAX_SAMPLES]
  GatherSources src;  // the frames
  int kind;           // PF_FISHEYE_EQUIDISTANT | PF_FISHEYE_EQUISOLID | PF_FISHEYE_STEREOGRAPHIC
  float fill;         // value of a pixel that no lens covers
  const float* lens;  // [n][PF_FISHEYE_MAX_LENSES][PF_FISHEYE_LENS_FLOATS]
  const float* cam;   // [n][7], as PanoBatch
  void* img;          // [n][H][W][3], the frames' type
  uint8_t* valid;     // NULL or [n][H][W]: 1 where a sub-sample is covered
};
void launch_fisheye_crop(const FisheyeCropBatch& fb, int dtype, hipStream_t s);
struct FisheyePanoBatch {
  static constexpr int MAX = GatherSources::MAX;
  GatherDims d;
  int samples;
  GatherSources src;  // the frames
  int kind;
  float fill;
  int inverse;        // as PanoRotBatch
  const float* lens;  // [n][PF_FISHEYE_MAX_LENSES][PF_FISHEYE_LENS_FLOATS]
  const float* rot;   // [n][3]: roll, pitch, yaw (radians)
  void* img;
  uint8_t* valid;
};
void launch_fisheye_to_pano(const FisheyePanoBatch& fb, int dtype, hipStream_t s);
static_assert(offsetof(FisheyeCropBatch, samples) == 28 && offsetof(FisheyeCropBatch, src) == 32, "FisheyeCropBatch layout");
static_assert(offsetof(FisheyePanoBatch, samples) == 28 && offsetof(FisheyePanoBatch, src) == 32, "FisheyePanoBatch layout");

// equirectangular panoramas -> fisheye and dual-fisheye frames + the perspective fields of the fisheye camera (fisheye_target.hip, include/pf_hip.h
// pf_pano_to_fisheye / pf_fisheye_fields): the outputs are frames (H, W, 3), each with its PF_FISHEYE_MAX_LENSES lens rows; `samples` as in the
// supersampled gathers
struct PanoToFisheyeBatch {
  static constexpr int MAX = GatherSources::MAX;
  GatherDims d;
  int samples;        // S in [1, PF_GATHER_MAX_SAMPLES]
  GatherSources src;  // the panoramas (Hp, Wp, 3)
  int kind;           // PF_FISHEYE_EQUIDISTANT | PF_FISHEYE_EQUISOLID | PF_FISHEYE_STEREOGRAPHIC
  float fill;         // value of a pixel that no lens owns
  const float* lens;  // [n][PF_FISHEYE_MAX_LENSES][PF_FISHEYE_LENS_FLOATS]
  void* img;          // [n][H][W][3], the panoramas' type
  uint8_t* valid;     // NULL or [n][H][W]: 1 where a sub-sample has an owner
  float* up;          // NULL (no labels) or [n][2][H][W]
  float* lat;         // NULL or [n][H][W] degrees
};
void launch_pano_to_fisheye(const PanoToFisheyeBatch& fb, int dtype, hipStream_t s);
// the labels alone (pf_fisheye_fields): no source
struct FisheyeFieldsBatch {
  static constexpr int MAX = GatherSources::MAX;
  GatherDims d;
  int kind;
  const float* lens;  // [n][PF_FISHEYE_MAX_LENSES][PF_FISHEYE_LENS_FLOATS]
  float* up;          // [n][2][H][W]
  float* lat;         // [n][H][W] degrees
};
void launch_fisheye_fields(const FisheyeFieldsBatch& fb, hipStream_t s);
static_assert(offsetof(PanoToFisheyeBatch, samples) == 28 && offsetof(PanoToFisheyeBatch, src) == 32, "PanoToFisheyeBatch layout");
static_assert(offsetof(FisheyeFieldsBatch, kind) == 28 && offsetof(FisheyeFieldsBatch, lens) == 32, "FisheyeFieldsBatch layout");

// camera views of one centre -> equirectangular panoramas (pano_compose.hip, include/pf_hip.h pf_pano_compose): the outputs of a launch are up to MAX
// panoramas, its sources up to MAX views; panorama k blends the views [first[k], first[k] + count[k]) of the launch in that order
struct ComposeBatch {
  static constexpr int MAX = GatherSources::MAX;
  GatherDims d;       // n panoramas of Hp x Wp
  float fill;         // value of a pixel that no view covers
  GatherSources src;  // the launch's views (Hs, Ws, 3)
  const float* cam;   // [views of the launch][7]: roll, pitch, yaw (radians), rel_focal, rel_cx, rel_cy, xi
  int first[MAX], count[MAX];
  uint32_t carry_in, carry_out;  // bit k: panorama k starts from / ends in the accumulator (a panorama of more than MAX views, one launch per MAX views)
  void* img;      // [n][Hp][Wp][3], the views' type
  float* weight;  // NULL or [n][Hp][Wp]: the summed weight S
  float* acc;     // NULL or [n][Hp][Wp][4]: (C.r, C.g, C.b, S) between the launches of one panorama
};
void launch_pano_compose(const ComposeBatch& cb, int dtype, int blend, hipStream_t s);
static_assert(offsetof(ComposeBatch, d) == 0 && offsetof(ComposeBatch, src) == 32, "ComposeBatch layout");

// perspective fields transported between cameras of one centre and onto panoramas (field_transport.hip, include/pf_hip.h pf_reproject_fields /
// pf_compose_fields): the gathers above with field planes as the sources
struct FieldSources {  // of each output (pf_reproject_fields) or of each view of the launch (pf_compose_fields)
  static constexpr int MAX = GatherSources::MAX;
  const float* up[MAX];   // [2][Hs][Ws]
  const float* lat[MAX];  // [Hs][Ws] degrees
  int H[MAX], W[MAX];
};
struct FieldReprojBatch {
  static constexpr int MAX = FieldSources::MAX;
  GatherDims d;
  FieldSources src;
  const float* cam_src;  // [n][7]: roll, pitch, yaw (radians), rel_focal, rel_cx, rel_cy, xi
  const float* cam_dst;  // [n][7]
  float* up;             // [n][2][H][W]
  float* lat;            // [n][H][W]
};
void launch_reproject_fields(const FieldReprojBatch& rb, hipStream_t s);
struct FieldComposeBatch {
  static constexpr int MAX = FieldSources::MAX;  // views of a launch, and of one panorama: there is no accumulator path
  GatherDims d;       // n panoramas of Hp x Wp
  FieldSources src;   // the launch's views
  const float* cam;   // [views of the launch][7]
  int first[MAX], count[MAX];
  float* up;      // [n][2][Hp][Wp]
  float* lat;     // [n][Hp][Wp]
  float* weight;  // NULL or [n][Hp][Wp]: the summed weight S
};
void launch_compose_fields(const FieldComposeBatch& cb, int blend, hipStream_t s);
static_assert(sizeof(FieldReprojBatch) <= 4096 && sizeof(FieldComposeBatch) <= 4096, "the field batches fit the kernel arguments");

// relative yaw of views of one centre (yaw_align.hip, include/pf_hip.h pf_yaw_moments): the luminance planes of up to YawLum::MAX views per launch, then
// the moments of up to YawBatch::MAX ordered pairs (a, b) per launch
struct YawLum {
  static constexpr int MAX = GatherSources::MAX;
  int n;              // views of this launch
  float c;            // the constant taken off the luminance: 127.5 (uint8), 0.5 (fp32)
  GatherSources src;  // (H, W, 3)
  float* out[MAX];    // (H, W) fp32 planes
};
void launch_yaw_luminance(const YawLum& yl, int dtype, hipStream_t s);
struct YawPair {
  const float *La, *Lb;  // luminance planes of a (sampled) and b (whose grid gives the samples)
  int Ha, Wa, Hb, Wb;
  int a, b;              // rows of `cam`
  unsigned tile0;        // the pair's first tile in `part`
  int tiles;             // ceil(samples of b / TILE)
};
struct YawBatch {
  static constexpr int MAX = 64;     // pairs per launch (the kernel arguments hold them: 48 bytes each)
  static constexpr int TILE = 1024;  // samples of b per block, 16 bytes of LDS each
  static constexpr int CHUNK = 64;   // candidates per block: one wavefront, one candidate per lane
  int n, n_cand, stride, max_tiles;  // pairs of this launch; candidates; sample stride; largest `tiles` of the launch
  const float* cam;   // [n_view][6]: roll, pitch (radians), rel_focal, rel_cx, rel_cy, xi
  const float* cand;  // [n_cand] radians
  float* part;        // [tile][n_cand][6] fp32: n, sum x, sum y, sum x^2, sum y^2, sum xy of one tile
  double* moments;    // [n][n_cand][6] of this launch's pairs
  YawPair pr[MAX];
};
void launch_yaw_moments(const YawBatch& yb, hipStream_t s);  // the store pass
void launch_yaw_sum(const YawBatch& yb, hipStream_t s);      // the tiles of each (pair, candidate) added in tile order in fp64
static_assert(sizeof(YawPair) == 48 && sizeof(YawBatch) <= 4096, "YawBatch fits the kernel arguments");

// placement scores of an object's fields on a background's (place_score.hip, include/pf_hip.h pf_place_scores): the packed (theta, latitude) planes of
// up to PlacePack::MAX fields per launch, then the sums of up to PlaceBatch::MAX (background, object) pairs per launch
struct PlacePack {
  static constexpr int MAX = 32;
  int n;                  // fields of this launch
  int npx[MAX];           // H * W
  const float* up[MAX];   // (2, H, W) degrees
  const float* lat[MAX];  // (H, W) degrees
  float2* out[MAX];       // (H, W) records (theta = atan2(u_y, u_x) in degrees, latitude), both NaN where the pixel is invalid
};
void launch_place_pack(const PlacePack& pp, hipStream_t s);
struct PlacePair {
  const float2 *bg, *obj;  // packed planes
  int W, w;                // row lengths of the background and of the object
  int obj_px;              // h * w
  int Q;                   // placements across
  int np;                  // P * Q placements
  int chunks;              // ceil(obj_px / CHUNK)
  size_t part0;            // the pair's first record in `part`; chunk c's records follow at part0 + c * np
  size_t out0;             // the pair's first record in `out`
};
struct PlaceBatch {
  static constexpr int MAX = 32;      // pairs per launch (the kernel arguments hold them: 56 bytes each)
  static constexpr int TILE = 256;    // placements per block, in row-major order: one per thread
  static constexpr int CHUNK = 1024;  // object pixels per block, in row-major order: the terms one thread adds in fp32
  int n, stride, max_tiles, max_chunks;  // pairs of this launch; placement stride; largest ceil(np / TILE) and `chunks` of the launch
  float* part;    // [record][3] fp32: S_up, S_lat, n of one (placement, chunk)
  double* out;    // [record][3]
  PlacePair pr[MAX];
};
void launch_place_score(const PlaceBatch& pb, hipStream_t s);  // the store pass
void launch_place_sum(const PlaceBatch& pb, hipStream_t s);    // the chunks of each placement added in chunk order in fp64
static_assert(sizeof(PlacePair) == 56 && sizeof(PlaceBatch) <= 4096 && sizeof(PlacePack) <= 4096, "PlaceBatch and PlacePack fit the kernel arguments");

// similarity transforms of perspective fields and the best placement over variants (field_xform.hip, include/pf_hip.h pf_fields_transform and
// pf_place_search): up to FieldXform::MAX (source, variant) jobs per launch, then up to BestBatch::MAX (pair, variant) score maps per launch
struct FieldXform {
  static constexpr int MAX = 32;
  int n;                         // jobs of this launch
  int h[MAX], w[MAX];            // source size
  int ho[MAX], wo[MAX];          // output size h', w'
  float c[MAX], s[MAX], inv[MAX];  // cos phi, sin phi, 1 / scale: fp64 on the host, rounded once
  const float* up[MAX];          // (2, h, w) degrees
  const float* lat[MAX];         // (h, w) degrees
  float* out_up[MAX];            // (2, h', w')
  float* out_lat[MAX];           // (h', w')
};
void launch_field_xform(const FieldXform& fx, hipStream_t s);
struct BestCount {
  static constexpr int MAX = 32;
  int n;                     // packed planes of this launch
  int npx[MAX];
  const float2* plane[MAX];  // place_pack_kernel's records
  int* cnt[MAX];             // the plane's valid pixels
};
void launch_place_count(const BestCount& bc, hipStream_t s);
struct BestHead {        // one per (pair, variant), written by the tile pass for the pair pass
  const double* map;     // the (pair, variant)'s [np][3] records, NULL for a skipped variant
  int tile0, tiles;      // its partial bests in `tile`
  int Q, cnt, ho, wo;    // placements across; valid pixels and size of the transformed object
};
struct BestTile { double pfd; long long at; };  // the lowest pfd of a tile and its row-major placement, the first of equal ones; at = -1 with +inf
struct BestEntry {
  const double* map;     // NULL: skipped
  const int* cnt;
  int np, Q, ho, wo;
  int tile0;             // the entry's first partial in `tile`
  int head;              // pair * n_var + variant
};
struct BestBatch {
  static constexpr int MAX = 32;
  static constexpr int TILE = 256;  // placements per block of the tile pass
  int n, max_tiles;                 // entries of this launch; largest max(1, ceil(np / TILE))
  double min_valid, w_up, w_lat;
  BestHead* head;
  BestTile* tile;
  BestEntry e[MAX];
};
void launch_place_best_tiles(const BestBatch& bb, hipStream_t s);
// one block per pair: d_var[pair][variant][6] and d_best[pair][7] from the heads and partials of every variant
void launch_place_best_pairs(int n_pair, int n_var, int stride, const BestHead* head, const BestTile* tile, double* d_best, double* d_var,
                             hipStream_t s);
static_assert(sizeof(FieldXform) <= 4096 && sizeof(BestCount) <= 4096 && sizeof(BestBatch) <= 4096, "FieldXform, BestCount and BestBatch fit the kernel arguments");

// objects pasted into backgrounds (composite.hip, include/pf_hip.h pf_composite): up to CompositeBatch::MAX jobs per launch, a job's pointers and sizes
// in the kernel arguments, its placement in a record that composite_prep_kernel writes from the caller's device table
struct CompositeJob {      // one per job, in the workspace
  int active;              // 0: the output is the background
  float c, s, inv;         // cos phi, sin phi, 1 / scale: fp64 on the device, rounded once
  int row, col, hb, wb;    // the box's top-left corner in the background and its size h', w'
  int r0, r1, c0, c1;      // the box clipped to the background: rows [r0, r1), columns [c0, c1); empty for an inactive job
};
struct CompositeBatch {
  static constexpr int MAX = 32;
  int n, first;            // jobs of this launch; the first one's index in `place` and `rec`
  int samples, hard;       // S; 1: PF_COMPOSITE_HARD
  double opacity;
  int H[MAX], W[MAX];      // background size
  int h[MAX], w[MAX];      // object size
  int vec[MAX];            // 1: background and output aligned for the 4-pixel accesses (uint8: 4 bytes, fp32: 16)
  int cvec[MAX];           // 1: the coverage plane is aligned to 16 bytes
  const void* bg[MAX];     // (H, W, 3) uint8 or fp32
  const void* obj[MAX];    // (h, w, 3) of the same type
  const float* alpha[MAX]; // (h, w) or NULL: opaque
  void* out[MAX];          // (H, W, 3)
  float* cov[MAX];         // (H, W) or NULL
  const double* place;     // [jobs of the call][6]: s, phi, row, col, h', w'
  CompositeJob* rec;       // [jobs of the call]
};
void launch_composite(const CompositeBatch& cb, int dtype, hipStream_t s);  // the records of the launch's jobs, then the pixels
static_assert(sizeof(CompositeJob) == 48 && sizeof(CompositeBatch) <= 4096, "CompositeBatch fits the kernel arguments");

// perspective fields drawn over their images (draw_fields.hip, include/pf_hip.h pf_draw_fields): up to DrawBatch::MAX images per launch, per-image sizes
// and pointers in the kernel arguments
struct DrawBatch {
  static constexpr int MAX = 32;
  static constexpr int CAP = 128;  // arrow records per LDS batch of a tile, 64 bytes each
  static constexpr int REC = 4;    // float4s of one record: (a, u), (tip, valid, -), (barb directions), (padded box x0, y0, x1, y1)
  int n, spacing, layers;          // images of this launch; anchor spacing; PF_DRAW_UP | PF_DRAW_LAT
  int max_tiles, max_anchors;      // largest number of 64 x 16 tiles and of anchors among the images: the grids
  float lat_step, alpha, line_width, rgb[3];
  int H[MAX], W[MAX];
  int nx[MAX], ny[MAX];            // anchors across and down (0 without PF_DRAW_UP)
  int reach[MAX];                  // pixels: no arrow is drawn further from its anchor's pixel than this
  int vec[MAX];                    // 1: W % 4 == 0 and image and output aligned for the 4-pixel vector loads and stores (uint8 4 bytes, fp32 16)
  int fvec[MAX];                   // 1: W % 4 == 0 and up and lat aligned to 16 bytes: 16-byte loads of the field planes
  float len[MAX];                  // L = arrow_len_rel W
  const void* img[MAX];            // (H, W, 3) uint8 or fp32
  const float* up[MAX];            // (2, H, W)
  const float* lat[MAX];           // (H, W) degrees
  void* out[MAX];                  // (H, W, 3), may be img
  float4* rec[MAX];                // [ny][nx][REC]
};
void launch_draw_fields(const DrawBatch& db, int dtype, hipStream_t s);  // the arrow records (with PF_DRAW_UP), then the tiles
static_assert(sizeof(DrawBatch) <= 4096, "DrawBatch fits the kernel arguments");

// predicted fields against ground truth (field_err.hip, include/pf_hip.h pf_field_errors): up to FerrBatch::MAX images per launch,
// per-image sizes and pointers in the kernel arguments
constexpr int FERR_REC = 10;         // doubles of one accumulate block's partial record
constexpr int FERR_LEVEL_BINS = 2048;  // bins of one radix level (11 bits; the last level uses 512 of them)
constexpr int FERR_SEL = 4;          // selections per image: ranks (n - 1) / 2 and n / 2 of e_up, then of e_lat
struct FerrState {                   // per image, written by the pick kernels
  double sums[2][5];                 // per metric, the PF_FERR_SUM_* columns
  unsigned long long rank[FERR_SEL]; // rank of the wanted element among those that share `prefix`
  unsigned prefix[FERR_SEL];         // the bits of the wanted element found so far
};
struct FerrBatch {
  static constexpr int MAX = 32;
  int n;
  int H[MAX], W[MAX], nblk[MAX];
  int vec[MAX];                 // 1: H * W % 4 == 0 and every plane 16-byte aligned: 16-byte loads and stores
  const float* up_pred[MAX];    // [2][H][W]
  const float* lat_pred[MAX];   // [H][W] degrees
  const float* up_gt[MAX];
  const float* lat_gt[MAX];
  float* err_up[MAX];           // [H][W] error maps (the caller's or the workspace's), NaN where invalid
  float* err_lat[MAX];
  double* part[MAX];            // [nblk][FERR_REC]
  unsigned* hist[MAX];          // [3 levels][FERR_SEL][FERR_LEVEL_BINS], zeroed before the first launch
  FerrState* state;             // [n]
  double* out;                  // [n][PF_FERR_COLS]
  float threshold;
};
int ferr_blocks_per_image(int H, int W);
void launch_field_errors(const FerrBatch& fb, hipStream_t s);  // accumulate + three (histogram, pick) levels
void launch_field_errors_hist(const FerrBatch& fb, long long* d_hist, double* d_hist_sums, hipStream_t s);  // after launch_field_errors

}  // namespace pf
