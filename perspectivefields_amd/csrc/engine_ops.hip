// Op-level entry points of libpf_hip.so (pf_op_*: one kernel family each, host weights uploaded per call) -- what tests/test_gpu_ops.py and the tuning scripts call.
// Not part of the inference path (the engine's forward, engine_forward.hip, never goes through here).
#include "host_pack.h"

using namespace pf;
using namespace pf_host;

// pf_op_set_saturation_watch: the counter / limit every pf_op_* launch of this thread hands to its kernel (nullptr = off); the timing loops and *_bench entries run without
static thread_local unsigned* t_op_sat = nullptr;
static thread_local float t_op_sat_limit = 65504.f;

// the form whose weights the conv entries also pack for the Winograd tiles ("wino256x64d" / "wino256x64c"); the launch's own rule is conv_wino_ok
static bool conv_wino_form(int KH, int KW, int stride, int pad, int C2, int Cin, int Cout, int KWC, int KWCp) {
  return KH == 3 && KW == 3 && stride == 1 && pad == 1 && C2 == 0 && Cin % 16 == 0 && Cout % 64 == 0 && KWCp == KWC;
}

extern "C" {

int pf_op_set_saturation_watch(void* d_counter_u32, float limit) {
  if (d_counter_u32 && !(limit > 0.f)) { g_create_error = "pf_op_set_saturation_watch: limit must be positive"; return PF_ERR_ARG; }
  t_op_sat = static_cast<unsigned*>(d_counter_u32);
  t_op_sat_limit = d_counter_u32 ? limit : 65504.f;
  return PF_OK;
}

int pf_op_num_conv_tiles(void) { return conv_num_tiles(); }
const char* pf_op_conv_tile_name(int id) { return conv_tile_name(id); }

int pf_op_conv2d(int device, const float* x, const float* x2, int B, int H, int W, int C1, int C2, const float* hw, const float* hb,
                 int Cout, int KH, int KW, int stride, int pad, int act, const float* res1, const float* res2, int post_relu,
                 int nchw_out, int tile_id, float* y, const uint16_t* x_planes, long x_plane_elems, const uint16_t* x2_planes,
                 long x2_plane_elems, uint16_t* y_planes, long y_plane_elems, int precision_flags, void* stream) {
  const int precision = precision_flags & 15;
  const bool allow_splitk = !(precision_flags & 16);
  if (precision != PF_PRECISION_FP32 && precision != PF_PRECISION_FP32_BF16X6) { g_create_error = "pf_op_conv2d: precision must be 0 (split-f16) or 3 (exact bf16 split)"; return PF_ERR_ARG; }
  std::string err;
  int rc = check_device(device, &err);
  if (rc != PF_OK) { g_create_error = err; return rc; }
  const int Cin = C1 + C2;
  if (Cin % 4 != 0 || (C2 > 0 && C1 % 32 != 0)) { g_create_error = "pf_op_conv2d: Cin must be a multiple of 4 (pad on the host), C1 of 32 when concatenating"; return PF_ERR_ARG; }
  hipStream_t s = static_cast<hipStream_t>(stream);
  TmpDev tmp;
  ConvParams p;
  std::vector<float> packed = pack_conv(hw, Cout, Cin, KH, KW, Cin, nullptr, &p.KWC, &p.KWCp);
  p.g[0].w = tmp.up(packed);
  std::vector<unsigned short> sb;
  if (Cin % 32 == 0 || Cin == 4) {
    sb = split_bf16x3(packed); p.g[0].w_sb = tmp.up_u16(sb);
    const F16Planes f = split_f16x2(packed, Cout);
    p.g[0].w_h16 = tmp.up_u16(f.planes); p.g[0].w_h16_inv_scale = tmp.up(f.inv_scale);
  }
  if (conv_wino_form(KH, KW, stride, pad, C2, Cin, Cout, p.KWC, p.KWCp)) {
    std::vector<unsigned short> planes;
    std::vector<float> inv;
    wino_pack_weights(packed.data(), Cout, Cin, p.KWCp, &planes, &inv);
    p.g[0].w_wino = tmp.up_u16(planes); p.g[0].w_wino_inv = tmp.up(inv);
  }
  p.g[0].bias = tmp.up(hb, Cout);
  p.g[0].x = x; p.g[0].x2 = x2; p.g[0].res1 = res1; p.g[0].res2 = res2; p.g[0].y = y;
  p.g[0].x_sb = x_planes; p.g[0].x2_sb = x2_planes; p.g[0].y_sb = y_planes;
  p.x_sb_plane = (size_t)x_plane_elems; p.x2_sb_plane = (size_t)x2_plane_elems; p.y_sb_plane = (size_t)y_plane_elems;
  p.B = B; p.H = H; p.W = W; p.C1 = C1; p.C2 = C2;
  p.KH = KH; p.KW = KW; p.stride = stride; p.pad = pad;
  p.Cout = Cout; p.act = act; p.post_relu = post_relu; p.nchw_out = nchw_out;
  p.nterms = precision == PF_PRECISION_FP32_BF16X6 ? 6 : NT_F16X3;
  // split-plane INPUT: the plane format (bit 0 of x_plane_elems, sb_split.h) fixes the scheme: fp16 planes <-> split-f16, bf16 planes <-> bf16 schemes
  if (x_planes) p.nterms = (x_plane_elems & 1) ? NT_F16X3 : (p.nterms == NT_F16X3 ? 6 : p.nterms);
  p.wino_half = conv_wino_half_env();
  p.sat = t_op_sat; p.sat_limit = t_op_sat_limit;
  p.finish();
  if ((!x && !x_planes) || (!y && !y_planes) || (C2 > 0 && !x2 && !x2_planes)) { g_create_error = "pf_op_conv2d: missing input or output"; return PF_ERR_ARG; }
  // an explicit tile that cannot read / write split planes is an error; with fp32 operands an unusable tile id falls back to the cost model
  if (tile_id >= 0 && !conv_tile_usable(p, tile_id) && (x_planes || y_planes)) { g_create_error = "pf_op_conv2d: tile config cannot run this operand format"; return PF_ERR_ARG; }
  {  // split-K by the engine's rule (scratch for the partial sums from a temporary allocation)
    const int S = allow_splitk ? conv_splitk_factor(p) : 1;
    if (S > 1) {
      void* d = nullptr;
      if (hipMalloc(&d, (size_t)S * p.M * p.Cout * 4) == hipSuccess) { tmp.p.push_back(d); p.g[0].partial = static_cast<float*>(d); p.splitk = S; }
    }
  }
  launch_conv_tile(p, tile_id, s);
  rc = hipGetLastError() == hipSuccess ? PF_OK : PF_ERR_DEVICE;
  tmp.sync_free(s);
  return rc;
}

int pf_op_linear_ln(int device, const float* x, long rows, int K, const float* hw, const float* hb, const float* hgamma, const float* hbeta, float eps, int N,
                    int act, const float* res1, int tile_id, float* y, int precision, void* stream) {
  std::string err;
  int rc = check_device(device, &err);
  if (rc != PF_OK) { g_create_error = err; return rc; }
  if (K % 32 != 0 || N % 4 != 0 || !x || !y || !hw || !hgamma || !hbeta || rows <= 0) { g_create_error = "pf_op_linear_ln: K must be a multiple of 32, N of 4"; return PF_ERR_ARG; }
  hipStream_t s = static_cast<hipStream_t>(stream);
  TmpDev tmp;
  ConvParams p;
  std::vector<float> wf, bf, cs;
  fold_ln_linear(hw, hb, hgamma, hbeta, N, K, &wf, &bf, &cs);
  std::vector<float> packed = pack_conv(wf.data(), N, K, 1, 1, K, nullptr, &p.KWC, &p.KWCp);
  p.g[0].w = tmp.up(packed);
  std::vector<unsigned short> sb = split_bf16x3(packed);
  p.g[0].w_sb = tmp.up_u16(sb);
  const F16Planes f = split_f16x2(packed, N);
  p.g[0].w_h16 = tmp.up_u16(f.planes); p.g[0].w_h16_inv_scale = tmp.up(f.inv_scale);
  p.g[0].bias = tmp.up(bf); p.g[0].ln_colsum = tmp.up(cs);
  p.g[0].x = x; p.g[0].res1 = res1; p.g[0].y = y;
  p.B = 1; p.H = (int)rows; p.W = 1; p.C1 = K; p.C2 = 0; p.KH = p.KW = 1; p.stride = 1; p.pad = 0;
  p.Cout = N; p.act = act; p.post_relu = 0; p.nchw_out = 0;
  p.nterms = precision == PF_PRECISION_FP32_BF16X6 ? 6 : NT_F16X3;
  p.ln = 1; p.ln_eps = eps;
  p.sat = t_op_sat; p.sat_limit = t_op_sat_limit;
  p.finish();
  if (tile_id >= 0 && !conv_tile_usable(p, tile_id)) { g_create_error = "pf_op_linear_ln: tile config cannot run the fused LayerNorm form"; return PF_ERR_ARG; }
  launch_conv_tile(p, tile_id, s);
  rc = hipGetLastError() == hipSuccess ? PF_OK : PF_ERR_DEVICE;
  tmp.sync_free(s);
  return rc;
}

int pf_op_rb_linear(int device, const float* x, long rows, int tokens, int K, const float* hw, const float* hb, const float* hgamma, const float* hbeta, float eps, int N,
                    int act, const float* res, float* y, int iters, float* ms_out, void* stream) {
  std::string err;
  int rc = check_device(device, &err);
  if (rc != PF_OK) { g_create_error = err; return rc; }
  if (!rb_linear_supported(K, N) || !x || !y || !hw || !hb || rows <= 0 || tokens <= 0 || rows % tokens != 0 || (hgamma && K != 320) || (K != 320 && act != ACT_NONE) || (act != ACT_NONE && act != ACT_GELU)) {
    g_create_error = "pf_op_rb_linear: (K, N) must be (320, multiple of 320) or (multiple of 256 above 320, 320); rows a multiple of tokens; LayerNorm / GELU only with K = 320";
    return PF_ERR_ARG;
  }
  hipStream_t s = static_cast<hipStream_t>(stream);
  TmpDev tmp;
  std::vector<unsigned short> st;
  std::vector<float> inv;
  rb_pack_w(hw, N, K, 320, &st, &inv);
  RbLinArgs a;
  a.x = x; a.ln_g = hgamma ? tmp.up(std::vector<float>(hgamma, hgamma + K)) : nullptr; a.ln_b = hgamma ? tmp.up(std::vector<float>(hbeta, hbeta + K)) : nullptr; a.ln_eps = eps;
  a.w = tmp.up_u16(st); a.w_bytes = st.size() * 2; a.inv = tmp.up(inv); a.bias = tmp.up(std::vector<float>(hb, hb + N)); a.res = res; a.y = y;
  a.M = (int)rows; a.tokens = tokens; a.bpi = (tokens + 63) / 64; a.N = N; a.act = act;
  a.sat = t_op_sat; a.sat_limit = t_op_sat_limit;
  launch_rb_linear(a, K, s);
  a.sat = nullptr;  // the stamp and timing launches below run unwatched
  if (getenv("PF_RB_STAMPS") && !hgamma) {  // timing aid: the s_memtime stamps of block 17's four waves of one more launch, to stderr
    unsigned long long* ds = nullptr;
    if (hipMalloc(&ds, 4 * 64 * 8) == hipSuccess) {
      (void)hipMemsetAsync(ds, 0, 4 * 64 * 8, s);
      RbLinArgs b = a; b.stamps = ds; b.res = nullptr;
      launch_rb_linear(b, K, s);
      std::vector<unsigned long long> hs(4 * 64);
      (void)hipStreamSynchronize(s);
      (void)hipMemcpy(hs.data(), ds, 4 * 64 * 8, hipMemcpyDeviceToHost);
      for (int w = 0; w < 4; ++w) {
        fprintf(stderr, "rb stamps K=%d N=%d wave %d:", K, N, w);
        for (int i = 1; i < 64; ++i) if (hs[w * 64 + i]) fprintf(stderr, " [%d]%lld", i, (long long)(hs[w * 64 + i] - hs[w * 64]));
        fprintf(stderr, "\n");
      }
      (void)hipFree(ds);
    }
  }
  if (iters > 0 && ms_out) {
    hipEvent_t e0, e1;
    (void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
    (void)hipEventRecord(e0, s);
    for (int i = 0; i < iters; ++i) launch_rb_linear(a, K, s);
    (void)hipEventRecord(e1, s);
    (void)hipEventSynchronize(e1);
    float t = 0.f;
    (void)hipEventElapsedTime(&t, e0, e1);
    *ms_out = t / iters;
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
  }
  rc = hipGetLastError() == hipSuccess ? PF_OK : PF_ERR_DEVICE;
  tmp.sync_free(s);
  return rc;
}

int pf_op_rb_proj_fc1(int device, const float* attn, float* x, int B, int tokens, int C, const float* proj_w, const float* proj_b, const float* ln2_g, const float* ln2_b,
                      float eps, const float* fc1_w, const float* fc1_b, float* hidden, int iters, float* ms_out, void* stream) {
  std::string err;
  int rc = check_device(device, &err);
  if (rc != PF_OK) { g_create_error = err; return rc; }
  if (C != 320 || !attn || !x || !hidden || !proj_w || !proj_b || !ln2_g || !ln2_b || !fc1_w || !fc1_b || B <= 0 || tokens <= 0) {
    g_create_error = "pf_op_rb_proj_fc1: C must be 320; all operands required";
    return PF_ERR_ARG;
  }
  hipStream_t s = static_cast<hipStream_t>(stream);
  TmpDev tmp;
  std::vector<unsigned short> st1, st2;
  std::vector<float> inv1, inv2;
  rb_pack_w(proj_w, C, C, 320, &st1, &inv1);
  rb_pack_w(fc1_w, 4 * C, C, 320, &st2, &inv2);
  st1.resize(st1.size() - (size_t)4 * 10 * 2 * 512);
  st1.insert(st1.end(), st2.begin(), st2.end());
  RbProjFc1Args a;
  a.attn = attn; a.x = x; a.w = tmp.up_u16(st1); a.w_bytes = st1.size() * 2; a.proj_inv = tmp.up(inv1); a.proj_bias = tmp.up(proj_b, C);
  a.ln2_g = tmp.up(ln2_g, C); a.ln2_b = tmp.up(ln2_b, C); a.ln2_eps = eps; a.fc1_inv = tmp.up(inv2); a.fc1_bias = tmp.up(fc1_b, 4 * C); a.hidden = hidden;
  a.B = B; a.tokens = tokens; a.bpi = (tokens + 63) / 64;
  a.sat = t_op_sat; a.sat_limit = a.hidden_limit = t_op_sat_limit;
  launch_rb_proj_fc1(a, C, s);
  a.sat = nullptr;
  if (iters > 0 && ms_out) {  // timing loop (x keeps accumulating: values are meaningless afterwards)
    hipEvent_t e0, e1;
    (void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
    (void)hipEventRecord(e0, s);
    for (int i = 0; i < iters; ++i) launch_rb_proj_fc1(a, C, s);
    (void)hipEventRecord(e1, s);
    (void)hipEventSynchronize(e1);
    float t = 0.f;
    (void)hipEventElapsedTime(&t, e0, e1);
    *ms_out = t / iters;
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
  }
  rc = hipGetLastError() == hipSuccess ? PF_OK : PF_ERR_DEVICE;
  tmp.sync_free(s);
  return rc;
}

int pf_op_mit_attn64(int device, const float* x, const float* kv, float* y, int B, int N, int M, const float* ln_g, const float* ln_b, float eps, const float* q_w, const float* q_b,
                     const float* p_w, const float* p_b, int iters, float* ms_out, void* stream) {
  std::string err;
  int rc = check_device(device, &err);
  if (rc != PF_OK) { g_create_error = err; return rc; }
  if (!x || !kv || !y || !ln_g || !ln_b || !q_w || !q_b || !p_w || !p_b || B <= 0 || N <= 0 || !mit_attn64_supported(64, 1, M)) {
    g_create_error = "pf_op_mit_attn64: all operands required; 1 <= kv rows <= 128";
    return PF_ERR_ARG;
  }
  hipStream_t s = static_cast<hipStream_t>(stream);
  TmpDev tmp;
  std::vector<unsigned short> wfr;
  std::vector<float> tab;
  attn64_pack(ln_g, ln_b, q_w, q_b, p_w, p_b, &wfr, &tab);
  MitAttn64Args a;
  a.x = x; a.kv = kv; a.y = y; a.wfr = tmp.up_u16(wfr); a.tab = tmp.up(tab); a.B = B; a.N = N; a.M = M; a.ln_eps = eps;
  a.sat = t_op_sat; a.sat_limit = t_op_sat_limit;
  int cus = 256;
  { hipDeviceProp_t pr; if (hipGetDeviceProperties(&pr, device) == hipSuccess && pr.multiProcessorCount > 0) cus = pr.multiProcessorCount; }
  launch_mit_attn64(a, cus, s);
  a.sat = nullptr;
  if (iters > 0 && ms_out) {  // timing loop (with y aliasing x the rows keep accumulating: values are meaningless afterwards)
    hipEvent_t e0, e1;
    (void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
    (void)hipEventRecord(e0, s);
    for (int i = 0; i < iters; ++i) launch_mit_attn64(a, cus, s);
    (void)hipEventRecord(e1, s);
    (void)hipEventSynchronize(e1);
    float t = 0.f;
    (void)hipEventElapsedTime(&t, e0, e1);
    *ms_out = t / iters;
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
  }
  rc = hipGetLastError() == hipSuccess ? PF_OK : PF_ERR_DEVICE;
  tmp.sync_free(s);
  return rc;
}

int pf_op_stem7x7(int device, const float* x, float* y, int B, int H, int W, int stride, const float* w, const float* bias, int relu, const float* ln_g, const float* ln_b, float eps,
                  int iters, float* ms_out, void* stream) {
  std::string err;
  int rc = check_device(device, &err);
  if (rc != PF_OK) { g_create_error = err; return rc; }
  if (!x || !y || !w || B <= 0 || H <= 0 || W <= 0 || !stem7x7_supported(3, 64, 7, stride, 3) || ((ln_g == nullptr) != (ln_b == nullptr))) {
    g_create_error = "pf_op_stem7x7: x, y, weight required; stride 2 or 4; LayerNorm gamma and beta together";
    return PF_ERR_ARG;
  }
  hipStream_t s = static_cast<hipStream_t>(stream);
  TmpDev tmp;
  std::vector<unsigned short> wfr;
  std::vector<float> tab;
  stem7x7_pack(w, nullptr, bias, ln_g, ln_b, &wfr, &tab);
  Stem7Args a;
  a.x = x; a.y = y; a.wfr = tmp.up_u16(wfr); a.tab = tmp.up(tab); a.B = B; a.H = H; a.W = W; a.stride = stride;
  a.Ho = (H + 6 - 7) / stride + 1; a.Wo = (W + 6 - 7) / stride + 1; a.relu = relu; a.ln = ln_g ? 1 : 0; a.ln_eps = eps;
  a.sat = t_op_sat; a.sat_limit = t_op_sat_limit;
  int cus = 256;
  { hipDeviceProp_t pr; if (hipGetDeviceProperties(&pr, device) == hipSuccess && pr.multiProcessorCount > 0) cus = pr.multiProcessorCount; }
  launch_stem7x7(a, cus, s);
  a.sat = nullptr;
  if (iters > 0 && ms_out) {
    hipEvent_t e0, e1;
    (void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
    (void)hipEventRecord(e0, s);
    for (int i = 0; i < iters; ++i) launch_stem7x7(a, cus, s);
    (void)hipEventRecord(e1, s);
    (void)hipEventSynchronize(e1);
    float t = 0.f;
    (void)hipEventElapsedTime(&t, e0, e1);
    *ms_out = t / iters;
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
  }
  rc = hipGetLastError() == hipSuccess ? PF_OK : PF_ERR_DEVICE;
  tmp.sync_free(s);
  return rc;
}

int pf_op_thin128(int device, const float* x, long rows, const float* w, const float* bias, const float* res, float* y, int iters, float* ms_out, void* stream) {
  std::string err;
  int rc = check_device(device, &err);
  if (rc != PF_OK) { g_create_error = err; return rc; }
  if (!x || !y || !w || rows <= 0) { g_create_error = "pf_op_thin128: x, y, weight required"; return PF_ERR_ARG; }
  hipStream_t s = static_cast<hipStream_t>(stream);
  TmpDev tmp;
  std::vector<unsigned short> wfr;
  std::vector<float> tab;
  thin128_pack(w, bias, &wfr, &tab);
  ThinLinArgs a;
  a.x = x; a.res = res; a.y = y; a.wfr = tmp.up_u16(wfr); a.tab = tmp.up(tab); a.M = rows;
  a.sat = t_op_sat; a.sat_limit = t_op_sat_limit;
  int cus = 256;
  { hipDeviceProp_t pr; if (hipGetDeviceProperties(&pr, device) == hipSuccess && pr.multiProcessorCount > 0) cus = pr.multiProcessorCount; }
  launch_thin128(a, cus, s);
  a.sat = nullptr;
  if (iters > 0 && ms_out) {
    hipEvent_t e0, e1;
    (void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
    (void)hipEventRecord(e0, s);
    for (int i = 0; i < iters; ++i) launch_thin128(a, cus, s);
    (void)hipEventRecord(e1, s);
    (void)hipEventSynchronize(e1);
    float t = 0.f;
    (void)hipEventElapsedTime(&t, e0, e1);
    *ms_out = t / iters;
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
  }
  rc = hipGetLastError() == hipSuccess ? PF_OK : PF_ERR_DEVICE;
  tmp.sync_free(s);
  return rc;
}

int pf_op_rb_srkv(int device, const float* x, int B, int Hr, int Wr, int C, const float* ln1_g, const float* ln1_b, float eps1, const float* sr_w, const float* sr_b,
                  const float* srn_g, const float* srn_b, float eps2, const float* kv_w, const float* kv_b, float* kv, int iters, float* ms_out, void* stream) {
  std::string err;
  int rc = check_device(device, &err);
  if (rc != PF_OK) { g_create_error = err; return rc; }
  if (!rb_srkv_supported(C, 2) || !x || !kv || !ln1_g || !ln1_b || !sr_w || !sr_b || !srn_g || !srn_b || !kv_w || !kv_b || B <= 0 || Hr <= 0 || Wr <= 0) {
    g_create_error = "pf_op_rb_srkv: C must be 320 (2 x 2 spatial reduction); all weights required";
    return PF_ERR_ARG;
  }
  hipStream_t s = static_cast<hipStream_t>(stream);
  TmpDev tmp;
  int kwc = 0, kwcp = 0;
  const std::vector<float> srp = pack_conv(sr_w, C, C, 2, 2, C, nullptr, &kwc, &kwcp);
  std::vector<unsigned short> st1, st2;
  std::vector<float> inv1, inv2;
  rb_pack_w(srp.data(), C, 2 * kwcp, 320, &st1, &inv1);
  rb_pack_w(kv_w, 2 * C, C, 320, &st2, &inv2);
  st1.resize(st1.size() - (size_t)4 * 10 * 2 * 512);
  st1.insert(st1.end(), st2.begin(), st2.end());
  RbSrKvArgs a;
  a.x = x; a.ln1_g = tmp.up(ln1_g, C); a.ln1_b = tmp.up(ln1_b, C); a.ln1_eps = eps1;
  a.w = tmp.up_u16(st1); a.w_bytes = st1.size() * 2; a.sr_inv = tmp.up(inv1); a.sr_bias = tmp.up(sr_b, C);
  a.srn_g = tmp.up(srn_g, C); a.srn_b = tmp.up(srn_b, C); a.srn_eps = eps2; a.kv_inv = tmp.up(inv2); a.kv_bias = tmp.up(kv_b, 2 * C);
  a.kv = kv; a.B = B; a.Hr = Hr; a.Wr = Wr; a.bpi = (Hr * Wr + 31) / 32;
  a.sat = t_op_sat;  // against the kernel's own window (4094)
  launch_rb_srkv(a, C, s);
  a.sat = nullptr;
  if (iters > 0 && ms_out) {
    hipEvent_t e0, e1;
    (void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
    (void)hipEventRecord(e0, s);
    for (int i = 0; i < iters; ++i) launch_rb_srkv(a, C, s);
    (void)hipEventRecord(e1, s);
    (void)hipEventSynchronize(e1);
    float t = 0.f;
    (void)hipEventElapsedTime(&t, e0, e1);
    *ms_out = t / iters;
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
  }
  rc = hipGetLastError() == hipSuccess ? PF_OK : PF_ERR_DEVICE;
  tmp.sync_free(s);
  return rc;
}

int pf_op_mit_mlp(int device, const float* x, float* y, int B, int Hs, int Ws, int C, const float* w1, const float* b1, const float* lng, const float* lnb, float eps,
                  const float* wdw, const float* bdw, const float* w2, const float* b2, int iters, float* ms_out, void* stream) {
  std::string err;
  int rc = check_device(device, &err);
  if (rc != PF_OK) { g_create_error = err; return rc; }
  if (!mit_mlp_supported(C) || !x || !y || x == y || B <= 0) { g_create_error = "pf_op_mit_mlp: C must be 64 or 128, x and y different buffers"; return PF_ERR_ARG; }
  hipStream_t s = static_cast<hipStream_t>(stream);
  TmpDev tmp;
  std::vector<unsigned short> wpk;
  std::vector<float> tab2;
  mit_mlp_pack(w1, b1, lng, lnb, wdw, bdw, w2, b2, C, &wpk, &tab2);
  const unsigned short* dw = tmp.up_u16(wpk);
  const float* dt = tmp.up(tab2);
  launch_mit_mlp(x, y, dw, dt, B, Hs, Ws, C, eps, s, t_op_sat, t_op_sat_limit);
  if (iters > 0 && ms_out) {
    hipEvent_t a, b;
    (void)hipEventCreate(&a); (void)hipEventCreate(&b);
    (void)hipEventRecord(a, s);
    for (int i = 0; i < iters; ++i) launch_mit_mlp(x, y, dw, dt, B, Hs, Ws, C, eps, s);
    (void)hipEventRecord(b, s);
    (void)hipEventSynchronize(b);
    float t = 0.f;
    (void)hipEventElapsedTime(&t, a, b);
    *ms_out = t / iters;
    (void)hipEventDestroy(a); (void)hipEventDestroy(b);
  }
  rc = hipGetLastError() == hipSuccess ? PF_OK : PF_ERR_DEVICE;
  tmp.sync_free(s);
  return rc;
}

int pf_op_cnx_mlp(int device, const float* d, float* y, long rows, int C, const float* w1, const float* b1, const float* lng, const float* lnb, float eps,
                  const float* w2, const float* b2, const float* ls, int iters, float* ms_out, void* stream) {
  std::string err;
  int rc = check_device(device, &err);
  if (rc != PF_OK) { g_create_error = err; return rc; }
  if ((!cnx_mlp_supported(C) && !cnx_rb_supported(C)) || !d || !y || rows <= 0 || rows > 0x7fffffffL / (4 * C)) { g_create_error = "pf_op_cnx_mlp: C must be 96, 192, 384 or 768"; return PF_ERR_ARG; }
  hipStream_t s = static_cast<hipStream_t>(stream);
  TmpDev tmp;
  std::vector<unsigned short> wpk;
  std::vector<float> tab;
  const bool rb = cnx_rb_supported(C);  // C = 384 / 768: the row-block form (cnx_rb.hip)
  if (rb) cnx_rb_pack(w1, b1, w2, b2, ls, C, &wpk, &tab);
  else cnx_mlp_pack(w1, b1, lng, lnb, w2, b2, ls, C, &wpk, &tab);
  const unsigned short* dw = tmp.up_u16(wpk);
  const float* dt = tmp.up(tab);
  CnxRbArgs ra{};
  if (rb) {
    ra.d = d; ra.y = y; ra.w = dw; ra.w_bytes = wpk.size() * 2; ra.tab = dt; ra.ln_g = tmp.up(lng, C); ra.ln_b = tmp.up(lnb, C); ra.ln_eps = eps; ra.M = (int)rows;
    ra.sat = t_op_sat; ra.sat_limit = t_op_sat_limit;
    if (!dw || !dt || !ra.ln_g || !ra.ln_b) { g_create_error = "pf_op_cnx_mlp: hipMalloc failed"; tmp.sync_free(s); return PF_ERR_DEVICE; }
  }
  unsigned* sat = t_op_sat;
  auto launch = [&]() { if (rb) launch_cnx_rb(ra, C, s); else launch_cnx_mlp(d, y, dw, dt, rows, C, eps, s, sat, t_op_sat_limit); };
  launch();
  sat = ra.sat = nullptr;
  if (iters > 0 && ms_out) {  // timing loop (y keeps accumulating: values are meaningless afterwards)
    hipEvent_t a, b;
    (void)hipEventCreate(&a); (void)hipEventCreate(&b);
    (void)hipEventRecord(a, s);
    for (int i = 0; i < iters; ++i) launch();
    (void)hipEventRecord(b, s);
    (void)hipEventSynchronize(b);
    float t = 0.f;
    (void)hipEventElapsedTime(&t, a, b);
    *ms_out = t / iters;
    (void)hipEventDestroy(a); (void)hipEventDestroy(b);
  }
  rc = hipGetLastError() == hipSuccess ? PF_OK : PF_ERR_DEVICE;
  tmp.sync_free(s);
  return rc;
}

int pf_op_conv2d_bench(int device, int B, int H, int W, int Cin, int Cout, int K, int stride, int pad, int tile_id, int iters, int fmt_prec, float* ms_out) {
  const int fmt = fmt_prec & 15, precision = fmt_prec >> 4;  // low 4 bits: operand format, upper bits: PF_PRECISION_* of the split tiles
  std::string err;
  int rc = check_device(device, &err);
  if (rc != PF_OK) { g_create_error = err; return rc; }
  if (Cin % 4 != 0 || iters <= 0 || !ms_out) { g_create_error = "pf_op_conv2d_bench: bad argument"; return PF_ERR_ARG; }
  ConvParams p;
  p.KWC = K * Cin; p.KWCp = roundup(p.KWC, 32);
  p.B = B; p.H = H; p.W = W; p.C1 = Cin; p.C2 = 0; p.KH = K; p.KW = K; p.stride = stride; p.pad = pad;
  p.Cout = Cout; p.act = ACT_RELU; p.post_relu = 0; p.nchw_out = 0;
  p.nterms = precision == PF_PRECISION_FP32_BF16X6 ? 6 : NT_F16X3;
  p.wino_half = conv_wino_half_env();
  p.finish();
  const size_t nx = (size_t)B * H * W * Cin, nw = (size_t)Cout * K * p.KWCp, ny = (size_t)p.M * Cout;
  float *dx = nullptr, *dw = nullptr, *dy = nullptr, *db = nullptr;
  unsigned short *dsb = nullptr, *dxs = nullptr, *dys = nullptr, *dh16 = nullptr;
  float* dinv = nullptr;
  TmpDev wino_tmp;                    // Winograd weights (freed below)
  unsigned short* dwino = nullptr;
  float* dwino_inv = nullptr;
  if (hipMalloc(&dx, nx * 4) != hipSuccess || hipMalloc(&dw, nw * 4) != hipSuccess || hipMalloc(&dy, ny * 4) != hipSuccess ||
      hipMalloc(&db, (size_t)Cout * 4) != hipSuccess || hipMalloc(&dsb, nw * 10) != hipSuccess || hipMalloc(&dh16, nw * 4) != hipSuccess ||
      hipMalloc(&dinv, (size_t)Cout * 4) != hipSuccess ||
      (fmt >= 1 && hipMalloc(&dxs, nx * 6) != hipSuccess) || (fmt >= 2 && hipMalloc(&dys, ny * 6) != hipSuccess)) { g_create_error = "pf_op_conv2d_bench: hipMalloc failed"; return PF_ERR_DEVICE; }
  {  // uniform [-1,1) data (never zero-fill a bench: DVFS gives zeros a higher clock); activations filled on the device
    std::vector<float> hw(nw), hb(Cout);
    uint32_t st = 12345u;
    auto rnd = [&]() { st = st * 1664525u + 1013904223u; return (float)((st >> 8) & 0xffff) / 32768.0f - 1.0f; };
    for (auto& v : hw) v = rnd() * 0.05f;
    for (auto& v : hb) v = rnd();
    launch_fill_random(dx, (long)nx, 777u, 1.0f, nullptr);
    (void)hipMemcpy(dw, hw.data(), nw * 4, hipMemcpyHostToDevice);
    (void)hipMemcpy(db, hb.data(), (size_t)Cout * 4, hipMemcpyHostToDevice);
    const std::vector<unsigned short> sb = split_bf16x3(hw);
    (void)hipMemcpy(dsb, sb.data(), nw * 10, hipMemcpyHostToDevice);
    const F16Planes f = split_f16x2(hw, Cout);
    (void)hipMemcpy(dh16, f.planes.data(), nw * 4, hipMemcpyHostToDevice);
    (void)hipMemcpy(dinv, f.inv_scale.data(), (size_t)Cout * 4, hipMemcpyHostToDevice);
    if (K == 3 && stride == 1 && pad == 1 && Cin % 16 == 0 && Cout % 64 == 0 && p.KWCp == p.KWC) {  // Winograd form (tiles "wino256x64d" / "wino256x64c")
      std::vector<unsigned short> planes;
      std::vector<float> inv;
      wino_pack_weights(hw.data(), Cout, Cin, p.KWCp, &planes, &inv);
      wino_tmp.sync_free(nullptr);
      dwino = wino_tmp.up_u16(planes); dwino_inv = wino_tmp.up(inv);
    }
  }
  p.g[0].x = dx; p.g[0].w = dw; p.g[0].bias = db; p.g[0].y = dy;
  if (Cin % 32 == 0 || Cin == 4) { p.g[0].w_sb = dsb; p.g[0].w_h16 = dh16; p.g[0].w_h16_inv_scale = dinv; }
  p.g[0].w_wino = dwino; p.g[0].w_wino_inv = dwino_inv;
  // fmt 1: A operand as split planes (fp32 copy withheld); fmt 2: split planes in and out
  const size_t fbit = p.nterms == NT_F16X3 ? SB_FMT_F16 : 0;  // plane format of the scheme under test (nx, ny are multiples of 4)
  if (fmt >= 1) { launch_split_planes(dx, dxs, nx | fbit, (long)nx, nullptr); p.g[0].x_sb = dxs; p.x_sb_plane = nx | fbit; p.g[0].x = nullptr; }
  if (fmt >= 2) { p.g[0].y_sb = dys; p.y_sb_plane = ny | fbit; p.g[0].y = nullptr; }
  if (!conv_tile_usable(p, tile_id) && tile_id >= 0) { *ms_out = -1.f; (void)hipFree(dx); (void)hipFree(dw); (void)hipFree(dy); (void)hipFree(db); (void)hipFree(dsb); (void)hipFree(dxs); (void)hipFree(dys); (void)hipFree(dh16); (void)hipFree(dinv); wino_tmp.sync_free(nullptr); return PF_OK; }
  hipEvent_t a, b;
  (void)hipEventCreate(&a); (void)hipEventCreate(&b);
  launch_conv_tile(p, tile_id, nullptr);
  launch_conv_tile(p, tile_id, nullptr);
  (void)hipEventRecord(a, nullptr);
  for (int i = 0; i < iters; ++i) launch_conv_tile(p, tile_id, nullptr);
  (void)hipEventRecord(b, nullptr);
  (void)hipEventSynchronize(b);
  float t = 0.f;
  (void)hipEventElapsedTime(&t, a, b);
  *ms_out = t / iters;
  if (getenv("PF_WINO_STAMPS") && strncmp(conv_tile_name(tile_id), "wino", 4) == 0) {  // timing aid: s_memtime stamps of block 17's waves of one more launch, to stderr
    unsigned long long* ds = nullptr;
    if (hipMalloc(&ds, 8 * 128 * 8) == hipSuccess) {
      (void)hipMemset(ds, 0, 8 * 128 * 8);
      p.stamps = ds;
      launch_conv_tile(p, tile_id, nullptr);
      p.stamps = nullptr;
      std::vector<unsigned long long> hs(8 * 128);
      (void)hipMemcpy(hs.data(), ds, hs.size() * 8, hipMemcpyDeviceToHost);
      (void)hipFree(ds);
      for (int w = 0; w < 8; ++w) {
        const unsigned long long t0 = hs[w * 128];
        if (!t0) continue;
        fprintf(stderr, "%s stamps %dx%d Cin=%d wave %d:", conv_tile_name(tile_id), H, W, Cin, w);
        for (int i = 1; i < 128; ++i) if (hs[w * 128 + i]) fprintf(stderr, " [%d]%llu", i, hs[w * 128 + i] - t0);
        fprintf(stderr, "\n");
      }
    }
  }
  rc = hipGetLastError() == hipSuccess ? PF_OK : PF_ERR_DEVICE;
  (void)hipEventDestroy(a); (void)hipEventDestroy(b);
  (void)hipFree(dx); (void)hipFree(dw); (void)hipFree(dy); (void)hipFree(db); (void)hipFree(dsb); (void)hipFree(dxs); (void)hipFree(dys); (void)hipFree(dh16); (void)hipFree(dinv);
  wino_tmp.sync_free(nullptr);
  return rc;
}

int pf_op_dwconv3x3_bench(int device, int variant, int B, int H, int W, int C, int iters, float* ms_out) {
  std::string err;
  int rc = check_device(device, &err);
  if (rc != PF_OK) { g_create_error = err; return rc; }
  if (C % 128 != 0 || iters <= 0 || !ms_out) { g_create_error = "pf_op_dwconv3x3_bench: bad argument"; return PF_ERR_ARG; }
  const size_t n = (size_t)B * H * W * C;
  float *dx = nullptr, *dy = nullptr, *dw = nullptr, *db = nullptr;
  if (hipMalloc(&dx, n * 4) != hipSuccess || hipMalloc(&dy, n * 4) != hipSuccess || hipMalloc(&dw, (size_t)9 * C * 4) != hipSuccess ||
      hipMalloc(&db, (size_t)C * 4) != hipSuccess) { g_create_error = "pf_op_dwconv3x3_bench: hipMalloc failed"; return PF_ERR_DEVICE; }
  {
    std::vector<float> hx(n), hw((size_t)9 * C), hb(C);
    uint32_t st = 777u;
    auto rnd = [&]() { st = st * 1664525u + 1013904223u; return (float)((st >> 8) & 0xffff) / 32768.0f - 1.0f; };
    for (auto& v : hx) v = rnd();
    for (auto& v : hw) v = rnd() * 0.3f;
    for (auto& v : hb) v = rnd() * 0.1f;
    (void)hipMemcpy(dx, hx.data(), n * 4, hipMemcpyHostToDevice);
    (void)hipMemcpy(dw, hw.data(), hw.size() * 4, hipMemcpyHostToDevice);
    (void)hipMemcpy(db, hb.data(), hb.size() * 4, hipMemcpyHostToDevice);
  }
  hipEvent_t a, b;
  (void)hipEventCreate(&a); (void)hipEventCreate(&b);
  launch_dwconv3x3_gelu_variant(variant, dx, dw, db, dy, B, H, W, C, nullptr);
  (void)hipEventRecord(a, nullptr);
  for (int i = 0; i < iters; ++i) launch_dwconv3x3_gelu_variant(variant, dx, dw, db, dy, B, H, W, C, nullptr);
  (void)hipEventRecord(b, nullptr);
  (void)hipEventSynchronize(b);
  float t = 0.f;
  (void)hipEventElapsedTime(&t, a, b);
  *ms_out = t / iters;
  rc = hipGetLastError() == hipSuccess ? PF_OK : PF_ERR_DEVICE;
  (void)hipEventDestroy(a); (void)hipEventDestroy(b);
  (void)hipFree(dx); (void)hipFree(dy); (void)hipFree(dw); (void)hipFree(db);
  return rc;
}

int pf_op_layernorm(int device, const float* x, const float* hg, const float* hbeta, float* y, long rows, int C, float eps, uint16_t* y_planes, long plane_elems, void* stream) {
  std::string err;
  int rc = check_device(device, &err);
  if (rc != PF_OK) { g_create_error = err; return rc; }
  hipStream_t s = static_cast<hipStream_t>(stream);
  TmpDev tmp;
  launch_layernorm(x, tmp.up(hg, C), tmp.up(hbeta, C), y, rows, C, eps, s, y_planes, (size_t)plane_elems);
  rc = hipGetLastError() == hipSuccess ? PF_OK : PF_ERR_DEVICE;
  tmp.sync_free(s);
  return rc;
}

int pf_op_dwconv3x3_gelu(int device, const float* x, const float* hw, const float* hb, float* y, int B, int H, int W, int C, uint16_t* y_planes, long plane_elems, void* stream) {
  std::string err;
  int rc = check_device(device, &err);
  if (rc != PF_OK) { g_create_error = err; return rc; }
  if (C % 128 != 0) { g_create_error = "pf_op_dwconv3x3_gelu: C must be a multiple of 128"; return PF_ERR_ARG; }
  hipStream_t s = static_cast<hipStream_t>(stream);
  TmpDev tmp;
  launch_dwconv3x3_gelu(x, tmp.up(pack_dw(hw, C, 3)), tmp.up(hb, C), y, B, H, W, C, s, y_planes, (size_t)plane_elems);
  rc = hipGetLastError() == hipSuccess ? PF_OK : PF_ERR_DEVICE;
  tmp.sync_free(s);
  return rc;
}

int pf_op_dwconv3x3_gelu_cfg(int device, const float* x, const float* hw, const float* hb, float* y, int B, int H, int W, int C, uint16_t* y_planes, long plane_elems, int variant, void* stream) {
  std::string err;
  int rc = check_device(device, &err);
  if (rc != PF_OK) { g_create_error = err; return rc; }
  if (C % 128 != 0) { g_create_error = "pf_op_dwconv3x3_gelu_cfg: C must be a multiple of 128"; return PF_ERR_ARG; }
  hipStream_t s = static_cast<hipStream_t>(stream);
  TmpDev tmp;
  launch_dwconv3x3_gelu_variant(variant, x, tmp.up(pack_dw(hw, C, 3)), tmp.up(hb, C), y, B, H, W, C, s, y_planes, (size_t)plane_elems);
  rc = hipGetLastError() == hipSuccess ? PF_OK : PF_ERR_DEVICE;
  tmp.sync_free(s);
  return rc;
}

int pf_op_dwconv7x7(int device, const float* x, const float* hw, const float* hb, float* y, int B, int H, int W, int C, void* stream) {
  std::string err;
  int rc = check_device(device, &err);
  if (rc != PF_OK) { g_create_error = err; return rc; }
  if (C % 96 != 0) { g_create_error = "pf_op_dwconv7x7: C must be a multiple of 96"; return PF_ERR_ARG; }
  hipStream_t s = static_cast<hipStream_t>(stream);
  TmpDev tmp;
  launch_dwconv7x7(x, tmp.up(pack_dw(hw, C, 7)), tmp.up(hb, C), y, B, H, W, C, s);
  rc = hipGetLastError() == hipSuccess ? PF_OK : PF_ERR_DEVICE;
  tmp.sync_free(s);
  return rc;
}

int pf_op_dwconv7x7_cfg(int device, const float* x, const float* hw, const float* hb, float* y, int B, int H, int W, int C, int variant, int nc, int nb, int th, void* stream) {
  std::string err;
  int rc = check_device(device, &err);
  if (rc != PF_OK) { g_create_error = err; return rc; }
  if (C % 96 != 0 && C % 32 != 0) { g_create_error = "pf_op_dwconv7x7_cfg: C must be a multiple of 32"; return PF_ERR_ARG; }
  hipStream_t s = static_cast<hipStream_t>(stream);
  TmpDev tmp;
  launch_dwconv7x7_cfg(variant, nc, nb, th, x, tmp.up(pack_dw(hw, C, 7)), tmp.up(hb, C), y, B, H, W, C, s);
  rc = hipGetLastError() == hipSuccess ? PF_OK : PF_ERR_DEVICE;
  tmp.sync_free(s);
  return rc;
}

// Yardstick beside the depthwise kernels (variant 100): a plain 16-byte-per-lane grid-stride copy of the same bytes -- what this memory system gives ANY launch that
// reads n floats and writes n floats (launch + first byte + drain included), the ceiling a stand-alone HBM-bound kernel of that size can be priced against.
__global__ __launch_bounds__(256) void copy_f4_kernel(const float4* __restrict__ x, float4* __restrict__ y, long n4) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) y[i] = x[i];
}
// PF_DW7_BENCH_COLD=K (K >= 2): the timed launches cycle through K input / output buffer pairs, so that a launch reads an input nobody has touched for K - 1 launches
// (K x 2 x bytes > 512 MB: not in the 256 MiB Infinity Cache, nor in L2) -- "cold"; default: ONE pair, re-read and re-written by every launch -- "warm" (L2 / Infinity
// Cache resident for the 20 - 160 MB maps of the ConvNeXt stages, which is also their state inside the forward: the previous kernel has just written them).
int pf_op_dwconv7x7_bench(int device, int variant, int nc, int nb, int th, int B, int H, int W, int C, int iters, float* ms_out) {
  std::string err;
  int rc = check_device(device, &err);
  if (rc != PF_OK) { g_create_error = err; return rc; }
  if (C % 32 != 0 || iters <= 0 || !ms_out) { g_create_error = "pf_op_dwconv7x7_bench: bad argument"; return PF_ERR_ARG; }
  const size_t n = (size_t)B * H * W * C;
  int K = 1;
  if (const char* e = getenv("PF_DW7_BENCH_COLD")) K = std::max(1, std::min(64, atoi(e)));
  std::vector<float*> dx(K, nullptr), dy(K, nullptr);
  float *dw = nullptr, *db = nullptr;
  bool ok = hipMalloc(&dw, (size_t)49 * C * 4) == hipSuccess && hipMalloc(&db, (size_t)C * 4) == hipSuccess;
  for (int k = 0; k < K && ok; ++k) ok = hipMalloc(&dx[k], n * 4) == hipSuccess && hipMalloc(&dy[k], n * 4) == hipSuccess;
  if (!ok) { g_create_error = "pf_op_dwconv7x7_bench: hipMalloc failed"; return PF_ERR_DEVICE; }
  for (int k = 0; k < K; ++k) launch_fill_random(dx[k], (long)n, 777u + k, 1.0f, nullptr);
  launch_fill_random(dw, (long)49 * C, 778u, 0.15f, nullptr);
  launch_fill_random(db, (long)C, 779u, 0.1f, nullptr);
  auto launch = [&](int k) {
    if (variant == 100) hipLaunchKernelGGL(copy_f4_kernel, dim3(256 * 8), dim3(256), 0, nullptr, reinterpret_cast<const float4*>(dx[k]), reinterpret_cast<float4*>(dy[k]), (long)(n / 4));
    else launch_dwconv7x7_cfg(variant, nc, nb, th, dx[k], dw, db, dy[k], B, H, W, C, nullptr);
  };
  hipEvent_t a, b;
  (void)hipEventCreate(&a); (void)hipEventCreate(&b);
  for (int k = 0; k < K; ++k) launch(k);
  (void)hipEventRecord(a, nullptr);
  for (int i = 0; i < iters; ++i) launch(i % K);
  (void)hipEventRecord(b, nullptr);
  (void)hipEventSynchronize(b);
  float t = 0.f;
  (void)hipEventElapsedTime(&t, a, b);
  *ms_out = t / iters;
  rc = hipGetLastError() == hipSuccess ? PF_OK : PF_ERR_DEVICE;
  (void)hipEventDestroy(a); (void)hipEventDestroy(b);
  for (int k = 0; k < K; ++k) { (void)hipFree(dx[k]); (void)hipFree(dy[k]); }
  (void)hipFree(dw); (void)hipFree(db);
  return rc;
}

int pf_op_sr_attention(int device, const float* q, const float* kv, float* out, int B, int N, int M, int heads, uint16_t* out_planes, long plane_elems, void* stream) {
  std::string err;
  int rc = check_device(device, &err);
  if (rc != PF_OK) { g_create_error = err; return rc; }
  if (M <= 0 || M > 128) { g_create_error = "pf_op_sr_attention: kv length must be in 1..128"; return PF_ERR_ARG; }
  launch_sr_attention(q, kv, out, B, N, M, heads, static_cast<hipStream_t>(stream), out_planes, (size_t)plane_elems);
  return hipGetLastError() == hipSuccess ? PF_OK : PF_ERR_DEVICE;
}

int pf_op_sr_attention_variant(int device, int variant, const float* q, const float* kv, float* out, int B, int N, int M, int heads, int iters, float* ms_out, void* stream) {
  std::string err;
  int rc = check_device(device, &err);
  if (rc != PF_OK) { g_create_error = err; return rc; }
  if (M <= 0 || M > 128 || (variant != 0 && variant != 1)) { g_create_error = "pf_op_sr_attention_variant: kv length must be in 1..128, variant 0 or 1"; return PF_ERR_ARG; }
  hipStream_t s = static_cast<hipStream_t>(stream);
  launch_sr_attention_variant(variant, q, kv, out, B, N, M, heads, s);
  if (iters > 0 && ms_out) {  // timing loop on the caller's data
    hipEvent_t a, b;
    (void)hipEventCreate(&a); (void)hipEventCreate(&b);
    (void)hipEventRecord(a, s);
    for (int i = 0; i < iters; ++i) launch_sr_attention_variant(variant, q, kv, out, B, N, M, heads, s);
    (void)hipEventRecord(b, s);
    (void)hipEventSynchronize(b);
    float t = 0.f;
    (void)hipEventElapsedTime(&t, a, b);
    *ms_out = t / iters;
    (void)hipEventDestroy(a); (void)hipEventDestroy(b);
  }
  return hipGetLastError() == hipSuccess ? PF_OK : PF_ERR_DEVICE;
}

int pf_op_upsample2x(int device, const float* x, float* y, int B, int H, int W, int C, uint16_t* y_planes, long plane_elems, void* stream) {
  std::string err;
  int rc = check_device(device, &err);
  if (rc != PF_OK) { g_create_error = err; return rc; }
  launch_upsample2x(x, y, B, H, W, C, static_cast<hipStream_t>(stream), y_planes, (size_t)plane_elems);
  return hipGetLastError() == hipSuccess ? PF_OK : PF_ERR_DEVICE;
}

int pf_op_split_bf16(int device, const float* x, long n, uint16_t* planes, long plane_elems, void* stream) {
  std::string err;
  int rc = check_device(device, &err);
  if (rc != PF_OK) { g_create_error = err; return rc; }
  if (!x || !planes || n <= 0 || (n & 3) || (plane_elems & ~1L) < n) { g_create_error = "pf_op_split_bf16: n must be a positive multiple of 4 and plane_elems >= n"; return PF_ERR_ARG; }
  launch_split_planes(x, planes, (size_t)plane_elems, n, static_cast<hipStream_t>(stream));
  return hipGetLastError() == hipSuccess ? PF_OK : PF_ERR_DEVICE;
}

int pf_op_merge_bf16(int device, const uint16_t* planes, long plane_elems, long n, float* y, void* stream) {
  std::string err;
  int rc = check_device(device, &err);
  if (rc != PF_OK) { g_create_error = err; return rc; }
  if (!y || !planes || n <= 0 || (n & 3) || (plane_elems & ~1L) < n) { g_create_error = "pf_op_merge_bf16: n must be a positive multiple of 4 and plane_elems >= n"; return PF_ERR_ARG; }
  launch_merge_planes(planes, (size_t)plane_elems, y, n, static_cast<hipStream_t>(stream));
  return hipGetLastError() == hipSuccess ? PF_OK : PF_ERR_DEVICE;
}

// ---- the kernels at the two ends of the forward (elem.hip) and the fused prediction-head epilogue (igemm_common.h), one entry each.  Device buffers are the caller's;
// an argument the kernel cannot take is PF_ERR_ARG before any launch.  Entries without host weights only enqueue; those with host weights upload them and, like the
// other pf_op_* entries, wait for the stream before they free the copies.
static bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
static int op_arg_error(const char* msg) { g_create_error = msg; return PF_ERR_ARG; }
static int op_begin(int device) {
  std::string err;
  const int rc = check_device(device, &err);
  if (rc != PF_OK) g_create_error = err;
  return rc;
}
static bool finite_nonzero3(const float* v) { return std::isfinite(v[0]) && std::isfinite(v[1]) && std::isfinite(v[2]) && v[0] != 0.f && v[1] != 0.f && v[2] != 0.f; }

int pf_op_prep_u8(int device, const uint8_t* x, int B, int H, int W, const float* mean3, const float* std3, float* y, void* stream) {
  if (!x || !y || !mean3 || !std3 || B < 1 || H < 1 || W < 1 || !aligned16(y) || !finite_nonzero3(std3)) return op_arg_error("pf_op_prep_u8: x, y (16-byte aligned), mean3, std3 (non-zero) required; B, H, W >= 1");
  const int rc = op_begin(device);
  if (rc != PF_OK) return rc;
  launch_prep_u8(x, y, (long)B * H * W, mean3, std3, static_cast<hipStream_t>(stream));
  return hipGetLastError() == hipSuccess ? PF_OK : PF_ERR_DEVICE;
}

int pf_op_prep_f32_nchw(int device, const float* x, int B, int H, int W, const float* mean3, const float* std3, float* y, void* stream) {
  if (!x || !y || !mean3 || !std3 || B < 1 || H < 1 || W < 1 || (long)H * W > 0x7fffffffL || !aligned16(y) || !finite_nonzero3(std3)) return op_arg_error("pf_op_prep_f32_nchw: x, y (16-byte aligned), mean3, std3 (non-zero) required; B, H, W >= 1, H W < 2^31");
  const int rc = op_begin(device);
  if (rc != PF_OK) return rc;
  launch_prep_f32_nchw(x, y, B, H * W, mean3, std3, static_cast<hipStream_t>(stream));
  return hipGetLastError() == hipSuccess ? PF_OK : PF_ERR_DEVICE;
}

int pf_op_pred_regression(int device, const float* tg, const float* tl, int B, int HW, const float* wg, const float* bg, const float* wl, const float* bl,
                          float* pg, float* pl, float* pn, void* stream) {
  if (!tg || !tl || !wg || !bg || !wl || !bl || !pg || !pl || B < 1 || HW < 1 || !aligned16(tg) || !aligned16(tl) || (pn && !aligned16(pn)))
    return op_arg_error("pf_op_pred_regression: features (16-byte aligned), both heads' weights and biases, pg, pl required (pn optional, 16-byte aligned); B, HW >= 1");
  const int rc = op_begin(device);
  if (rc != PF_OK) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  TmpDev tmp;
  const float *dwg = tmp.up(wg, 64), *dbg = tmp.up(bg, 2), *dwl = tmp.up(wl, 32), *dbl = tmp.up(bl, 1);
  if (!dwg || !dbg || !dwl || !dbl) { g_create_error = "pf_op_pred_regression: hipMalloc failed"; tmp.sync_free(s); return PF_ERR_DEVICE; }
  launch_pred_regression(tg, tl, dwg, dbg, dwl, dbl, pg, pl, pn, B, HW, s);
  const int out = hipGetLastError() == hipSuccess ? PF_OK : PF_ERR_DEVICE;
  tmp.sync_free(s);
  return out;
}

int pf_op_decode_cls(int device, const float* logit_g, int ng, const float* logit_l, int nl, int B, int HW, float* dg, float* dl, void* stream) {
  if (!logit_g || !logit_l || !dg || !dl || ng < 2 || nl < 1 || B < 1 || HW < 1) return op_arg_error("pf_op_decode_cls: logits and outputs required; ng >= 2, nl >= 1, B, HW >= 1");
  const int rc = op_begin(device);
  if (rc != PF_OK) return rc;
  launch_decode_cls(logit_g, ng, logit_l, nl, dg, dl, B, HW, static_cast<hipStream_t>(stream));
  return hipGetLastError() == hipSuccess ? PF_OK : PF_ERR_DEVICE;
}

int pf_op_nearest_nhwc4(int device, const float* x, int B, int H, int W, int Ho, int Wo, float* y, void* stream) {
  if (!x || !y || x == y || B < 1 || H < 1 || W < 1 || Ho < 1 || Wo < 1 || !aligned16(x) || !aligned16(y)) return op_arg_error("pf_op_nearest_nhwc4: x, y (different buffers, 16-byte aligned) required; all sizes >= 1");
  const int rc = op_begin(device);
  if (rc != PF_OK) return rc;
  launch_nearest_nhwc4(x, y, B, H, W, Ho, Wo, static_cast<hipStream_t>(stream));
  return hipGetLastError() == hipSuccess ? PF_OK : PF_ERR_DEVICE;
}

int pf_op_gap_ln_head(int device, const float* x, int B, int HW, int C, const float* gamma, const float* beta, float eps, const float* head_w, const float* head_b, int nout,
                      float* y, void* stream) {
  if (!x || !y || !gamma || !beta || !head_w || !head_b || B < 1 || HW < 1 || C < 1 || C > 1024 || nout < 1 || !(eps >= 0.f))
    return op_arg_error("pf_op_gap_ln_head: all operands required; B, HW, nout >= 1; 1 <= C <= 1024 (the pooled row lives in a fixed LDS array); eps >= 0");
  const int rc = op_begin(device);
  if (rc != PF_OK) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  TmpDev tmp;
  const float *dg = tmp.up(gamma, C), *db = tmp.up(beta, C), *dw = tmp.up(head_w, (size_t)nout * C), *dhb = tmp.up(head_b, nout);
  if (!dg || !db || !dw || !dhb) { g_create_error = "pf_op_gap_ln_head: hipMalloc failed"; tmp.sync_free(s); return PF_ERR_DEVICE; }
  launch_gap_ln_head(x, dg, db, dw, dhb, y, B, HW, C, nout, eps, s);
  const int out = hipGetLastError() == hipSuccess ? PF_OK : PF_ERR_DEVICE;
  tmp.sync_free(s);
  return out;
}

int pf_op_paramnet_scalars(int device, const float* raw, int B, int nraw, int mode, float* out8, void* stream) {
  if (!raw || !out8 || B < 1 || nraw < 1 || nraw > 8 || (mode != 0 && mode != 1) || (mode == 0 && nraw < 4)) return op_arg_error("pf_op_paramnet_scalars: raw, out8 required; B >= 1; 1 <= nraw <= 8; mode 0 (needs nraw >= 4) or 1");
  const int rc = op_begin(device);
  if (rc != PF_OK) return rc;
  launch_paramnet_scalars(raw, nraw, out8, B, mode, static_cast<hipStream_t>(stream));
  return hipGetLastError() == hipSuccess ? PF_OK : PF_ERR_DEVICE;
}

// the conv_fuse_conv1 form without the fused up-sampling: 3x3 / stride 1 / pad 1, Cin -> 32, split-f16 scheme, the 1x1 prediction head in the epilogue (no 32-channel map stored)
static void conv2d_head_params(ConvParams* p, int B, int H, int W, int Cin, int act, int head_kind) {
  p->KWC = 3 * Cin; p->KWCp = roundup(p->KWC, 32);
  p->B = B; p->H = H; p->W = W; p->C1 = Cin; p->C2 = 0; p->KH = p->KW = 3; p->stride = 1; p->pad = 1;
  p->Cout = 32; p->act = act; p->post_relu = 0; p->nchw_out = 0; p->nterms = NT_F16X3;
  p->g[0].head_kind = head_kind;
  p->finish();
}
static const char* conv2d_head_shape_error(int B, int H, int W, int Cin, int act, int head_kind) {
  if (B < 1 || H < 1 || W < 1 || Cin < 32 || Cin % 32 != 0) return "B, H, W >= 1 and Cin a positive multiple of 32 required";
  if ((long)B * H * W * std::max(Cin, 32) * 4 >= 0x7fffffffL) return "activations of 2 GiB and more are not addressable";
  if (act != ACT_NONE && act != ACT_RELU && act != ACT_GELU) return "act must be 0 (none), 1 (relu) or 2 (gelu)";
  if (head_kind != 1 && head_kind != 2) return "head_kind must be 1 (gravity: 32 -> 2, normalise) or 2 (latitude: 32 -> 1, clamp)";
  return nullptr;
}

int pf_op_conv2d_head_tile_usable(int B, int H, int W, int Cin, int act, int head_kind, int tile_id) {
  if (conv2d_head_shape_error(B, H, W, Cin, act, head_kind)) return 0;
  static const float dummy[4] = {0.f, 0.f, 0.f, 0.f};  // the usability rules look at which operands exist, never at their contents
  static const unsigned short dummy16[2] = {0, 0};
  ConvParams p;
  conv2d_head_params(&p, B, H, W, Cin, act, head_kind);
  p.g[0].x = dummy; p.g[0].w = dummy; p.g[0].w_sb = dummy16; p.g[0].w_h16 = dummy16; p.g[0].w_h16_inv_scale = dummy; p.g[0].bias = dummy;
  return conv_tile_usable(p, tile_id) ? 1 : 0;
}

int pf_op_conv2d_head(int device, const float* x, int B, int H, int W, int Cin, const float* hw, const float* hb, int act, int head_kind, const float* head_w, const float* head_b,
                      int tile_id, float* head_out, float* pn, void* stream) {
  if (const char* e = conv2d_head_shape_error(B, H, W, Cin, act, head_kind)) { g_create_error = std::string("pf_op_conv2d_head: ") + e; return PF_ERR_ARG; }
  if (!x || !hw || !head_w || !head_b || !head_out || !aligned16(x) || (pn && !aligned16(pn))) return op_arg_error("pf_op_conv2d_head: x (16-byte aligned), weight, head_w, head_b, head_out required (pn optional, 16-byte aligned)");
  if (tile_id < -1 || tile_id >= conv_num_tiles()) return op_arg_error("pf_op_conv2d_head: tile_id must be -1 (automatic) or a tile id");
  const int rc = op_begin(device);
  if (rc != PF_OK) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  TmpDev tmp;
  ConvParams p;
  const int nout = head_kind == 1 ? 2 : 1;
  {
    int kwc = 0, kwcp = 0;
    const std::vector<float> packed = pack_conv(hw, 32, Cin, 3, 3, Cin, nullptr, &kwc, &kwcp);
    const std::vector<unsigned short> sb = split_bf16x3(packed);
    const F16Planes f = split_f16x2(packed, 32);
    conv2d_head_params(&p, B, H, W, Cin, act, head_kind);
    p.g[0].w = tmp.up(packed); p.g[0].w_sb = tmp.up_u16(sb);
    p.g[0].w_h16 = tmp.up_u16(f.planes); p.g[0].w_h16_inv_scale = tmp.up(f.inv_scale);
  }
  p.g[0].bias = tmp.up(hb, 32);
  p.g[0].x = x;
  p.g[0].head_w = tmp.up(head_w, (size_t)nout * 32); p.g[0].head_b = tmp.up(head_b, nout);
  p.g[0].head_out = head_out; p.g[0].head_pn = pn;
  p.wino_half = conv_wino_half_env();
  p.sat = t_op_sat; p.sat_limit = t_op_sat_limit;
  if (!p.g[0].w || !p.g[0].w_sb || !p.g[0].w_h16 || !p.g[0].w_h16_inv_scale || (hb && !p.g[0].bias) || !p.g[0].head_w || !p.g[0].head_b) {
    g_create_error = "pf_op_conv2d_head: hipMalloc failed"; tmp.sync_free(s); return PF_ERR_DEVICE;
  }
  // unlike pf_op_conv2d, a named tile that cannot run this form is an error: a caller that names a tile has run that tile
  if (tile_id >= 0 && !conv_tile_usable(p, tile_id)) {
    g_create_error = fmt("pf_op_conv2d_head: tile %d (%s) cannot run the fused prediction head", tile_id, conv_tile_name(tile_id));
    tmp.sync_free(s);
    return PF_ERR_ARG;
  }
  if (tile_id < 0 && !conv_tile_usable(p, conv_default_tile(p))) { g_create_error = "pf_op_conv2d_head: no tile runs this shape"; tmp.sync_free(s); return PF_ERR_ARG; }
  launch_conv_tile(p, tile_id, s);
  const int out = hipGetLastError() == hipSuccess ? PF_OK : PF_ERR_DEVICE;
  tmp.sync_free(s);
  return out;
}

// ---- the conv forms only the forward's conv_g sets (engine_forward.hip): two problems in one grid, the first input at half resolution, the nine-case bias table
struct ConvGShape { int B, H, W, C1, C2, Cout, KH, KW, stride, pad, act, groups, ups, precision; };
static const char* conv2d_g_shape_error(const ConvGShape& c, const int* has_table, const int* head_kind) {
  if (c.groups != 1 && c.groups != 2) return "groups must be 1 or 2";
  if (c.precision != PF_PRECISION_FP32 && c.precision != PF_PRECISION_FP32_BF16X6) return "precision must be 0 (split-f16) or 3 (exact bf16 split)";
  if (c.B < 1 || c.H < 1 || c.W < 1 || c.C1 < 1 || c.C2 < 0 || c.Cout < 1 || c.KH < 1 || c.KW < 1 || c.stride < 1 || c.pad < 0) return "B, H, W, C1, Cout, KH, KW, stride >= 1 and C2, pad >= 0 required";
  if (c.H + 2 * c.pad < c.KH || c.W + 2 * c.pad < c.KW) return "the kernel does not fit the padded map";
  if (c.C1 % 32 != 0 || c.C2 % 32 != 0) return "C1 and C2 must be multiples of 32";
  if ((long)c.B * c.H * c.W * std::max(std::max(c.C1, c.C2), c.Cout) * 4 >= 0x7fffffffL || (long)c.Cout * c.KH * roundup(c.KW * (c.C1 + c.C2), 32) * 4 >= 0x7fffffffL) return "tensors of 2 GiB and more are not addressable";
  if (c.act != ACT_NONE && c.act != ACT_RELU && c.act != ACT_GELU) return "act must be 0 (none), 1 (relu) or 2 (gelu)";
  if (c.ups != 0 && c.ups != 1) return "ups must be 0 or 1";
  if (c.ups && ((c.H & 1) || (c.W & 1))) return "ups: H and W (the full-resolution size) must be even";
  if (c.ups && c.precision != PF_PRECISION_FP32) return "ups: the halo tiles interpolate in the split-f16 scheme only (precision 0)";
  const int Ho = (c.H + 2 * c.pad - c.KH) / c.stride + 1, Wo = (c.W + 2 * c.pad - c.KW) / c.stride + 1;
  for (int g = 0; g < c.groups; ++g) {
    if (has_table[g] && (Ho < 2 || Wo < 2)) return "a bias table needs Ho >= 2 and Wo >= 2: a pixel that is both the first and the last row (column) is none of the nine border cases";
    if (head_kind[g] < 0 || head_kind[g] > 2) return "head_kind must be 0 (none), 1 (gravity) or 2 (latitude)";
    if ((head_kind[g] != 0) != (head_kind[0] != 0)) return "every group has a fused head or none has";
    if (head_kind[g] && c.Cout != 32) return "a fused head needs Cout == 32";
  }
  return nullptr;
}
// the shape fields of the launch; the operands of the usability rules (which exist, never what they hold) from `dummy` when the caller has no real ones yet
static void conv2d_g_params(ConvParams* p, const ConvGShape& c, const int* has_table, const int* head_kind, bool dummies) {
  static const float dummy[4] = {0.f, 0.f, 0.f, 0.f};
  static const unsigned short dummy16[2] = {0, 0};
  static float dummy_out[4];
  p->groups = c.groups;
  p->KWC = c.KW * (c.C1 + c.C2); p->KWCp = roundup(p->KWC, 32);
  p->B = c.B; p->H = c.H; p->W = c.W; p->C1 = c.C1; p->C2 = c.C2; p->KH = c.KH; p->KW = c.KW; p->stride = c.stride; p->pad = c.pad;
  p->Cout = c.Cout; p->act = c.act; p->post_relu = 0; p->nchw_out = 0; p->ups = c.ups;
  p->nterms = c.precision == PF_PRECISION_FP32_BF16X6 ? 6 : NT_F16X3;
  p->wino_half = conv_wino_half_env();
  for (int g = 0; g < c.groups; ++g) p->g[g].head_kind = head_kind[g];
  p->finish();
  if (!dummies) return;
  const bool wino_form = conv_wino_form(c.KH, c.KW, c.stride, c.pad, c.C2, c.C1 + c.C2, c.Cout, p->KWC, p->KWCp);
  for (int g = 0; g < c.groups; ++g) {
    ConvPtrs& q = p->g[g];
    q.x = dummy; q.x2 = c.C2 > 0 ? dummy : nullptr; q.w = dummy; q.w_sb = dummy16; q.w_h16 = dummy16; q.w_h16_inv_scale = dummy;
    if (wino_form) { q.w_wino = dummy16; q.w_wino_inv = dummy; }
    if (has_table[g]) q.bias_tab = dummy; else q.bias = dummy;
    if (head_kind[g]) { q.head_w = dummy; q.head_b = dummy; q.head_out = dummy_out; } else q.y = dummy_out;
  }
}

// the tile and the split-K factor (linear split tiles only; the engine's rule or the caller's mode) of a launch, from which operands exist -- dummy or real;
// "" or why nothing runs the form.  launch_conv_tile would replace a tile that cannot run it, and launch_sbh_cfg returns without a launch for an up-sampling form
// on a tile that is not a 4-wave plain-tap tile: neither may be reached
static std::string conv2d_g_plan(ConvParams p, int tile_id, int splitk_mode, int* tile, int* S) {
  *tile = tile_id >= 0 ? tile_id : conv_default_tile(p);
  *S = 1;
  if (!conv_tile_usable(p, *tile)) return tile_id >= 0 ? fmt("tile %d (%s) cannot run this form", tile_id, conv_tile_name(tile_id)) : std::string("no tile runs this form");
  const char* nm = conv_tile_name(*tile);
  if (!conv_tile_is_sb(*tile) || strncmp(nm, "sbh", 3) == 0 || strncmp(nm, "wino", 4) == 0) return "";
  *S = splitk_mode < 0 ? conv_splitk_factor(p) : conv_splitk_factor(p, splitk_mode);
  if (*S > 1) {
    p.splitk = *S;
    for (int g = 0; g < p.groups; ++g) p.g[g].partial = p.g[g].y;  // exists; nothing here reads it
    if (!conv_tile_usable(p, *tile)) return "the tile cannot run the split-K form";
  }
  return "";
}

int pf_op_conv2d_g_tile_usable(int B, int H, int W, int C1, int C2, int Cout, int KH, int KW, int stride, int pad, int act, int groups, int ups, int has_table, int head_kind,
                               int precision, int tile_id) {
  const ConvGShape c{B, H, W, C1, C2, Cout, KH, KW, stride, pad, act, groups, ups, precision};
  const int tab[2] = {has_table ? 1 : 0, has_table ? 1 : 0}, hk[2] = {head_kind, head_kind};
  if (conv2d_g_shape_error(c, tab, hk)) return 0;
  ConvParams p;
  conv2d_g_params(&p, c, tab, hk, true);
  return conv_tile_usable(p, tile_id) ? 1 : 0;
}

int pf_op_conv2d_g(int device, int groups, const float* const* d_x, const float* const* d_x2, int B, int H, int W, int C1, int C2, const float* const* h_weight,
                   const float* const* h_bias, const int* bias_rows, int Cout, int KH, int KW, int stride, int pad, int act, const float* const* d_res1,
                   const float* const* d_res2, int post_relu, int ups, float* const* d_y, const int* head_kind, const float* const* h_head_w, const float* const* h_head_b,
                   float* const* d_head_out, float* const* d_pn, int tile_id, int precision, int splitk_mode, int* splitk_used, void* stream) {
  if (splitk_used) *splitk_used = 1;
  if (!d_x || !h_weight || !bias_rows || !head_kind) return op_arg_error("pf_op_conv2d_g: d_x, h_weight, bias_rows, head_kind (arrays of `groups` entries) required");
  const ConvGShape c{B, H, W, C1, C2, Cout, KH, KW, stride, pad, act, groups, ups, precision};
  int tab[2] = {0, 0}, hk[2] = {0, 0};
  for (int g = 0; g < std::min(std::max(groups, 0), 2); ++g) {
    if (bias_rows[g] != 1 && bias_rows[g] != 9) return op_arg_error("pf_op_conv2d_g: bias_rows must be 1 ([Cout]) or 9 ([9][Cout])");
    tab[g] = bias_rows[g] == 9; hk[g] = head_kind[g];
  }
  if (const char* e = conv2d_g_shape_error(c, tab, hk)) { g_create_error = std::string("pf_op_conv2d_g: ") + e; return PF_ERR_ARG; }
  if (tile_id < -1 || tile_id >= conv_num_tiles()) return op_arg_error("pf_op_conv2d_g: tile_id must be -1 (automatic) or a tile id");
  if (splitk_mode < -1 || splitk_mode == 1) return op_arg_error("pf_op_conv2d_g: splitk_mode must be -1 (the engine's rule), 0 (never) or a factor above 1");
  for (int g = 0; g < groups; ++g) {
    if (!d_x[g] || !aligned16(d_x[g]) || !h_weight[g] || (C2 > 0 && (!d_x2 || !d_x2[g] || !aligned16(d_x2[g]))) || (tab[g] && (!h_bias || !h_bias[g])))
      return op_arg_error("pf_op_conv2d_g: every group needs d_x (16-byte aligned), h_weight, d_x2 when C2 > 0, and its table when bias_rows is 9");
    if (hk[g] ? (!h_head_w || !h_head_w[g] || !h_head_b || !h_head_b[g] || !d_head_out || !d_head_out[g] || (d_pn && d_pn[g] && !aligned16(d_pn[g]))) : (!d_y || !d_y[g] || !aligned16(d_y[g])))
      return op_arg_error("pf_op_conv2d_g: every group needs d_y (16-byte aligned), or with a fused head head_w, head_b, head_out (pn optional, 16-byte aligned)");
    if ((d_res1 && d_res1[g] && !aligned16(d_res1[g])) || (d_res2 && d_res2[g] && !aligned16(d_res2[g]))) return op_arg_error("pf_op_conv2d_g: residuals must be 16-byte aligned");
  }
  int tile = -1, S = 1;
  {  // the tile and the split-K factor on the dummy operand set of the usability query, with the residuals as given: decided before any device work
    ConvParams probe;
    conv2d_g_params(&probe, c, tab, hk, true);
    probe.post_relu = post_relu;
    for (int g = 0; g < groups; ++g) { probe.g[g].res1 = d_res1 ? d_res1[g] : nullptr; probe.g[g].res2 = d_res2 ? d_res2[g] : nullptr; }
    const std::string e = conv2d_g_plan(probe, tile_id, splitk_mode, &tile, &S);
    if (!e.empty()) { g_create_error = "pf_op_conv2d_g: " + e; return PF_ERR_ARG; }
  }
  const int rc = op_begin(device);
  if (rc != PF_OK) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  TmpDev tmp;
  ConvParams p;
  conv2d_g_params(&p, c, tab, hk, false);
  p.post_relu = post_relu;
  p.sat = t_op_sat; p.sat_limit = t_op_sat_limit;
  const int Cin = C1 + C2;
  bool up_ok = true;
  for (int g = 0; g < groups; ++g) {  // weights packed as pf_op_conv2d packs them
    ConvPtrs& q = p.g[g];
    int kwc = 0, kwcp = 0;
    const std::vector<float> packed = pack_conv(h_weight[g], Cout, Cin, KH, KW, Cin, nullptr, &kwc, &kwcp);
    q.w = tmp.up(packed);
    q.w_sb = tmp.up_u16(split_bf16x3(packed));
    const F16Planes f = split_f16x2(packed, Cout);
    q.w_h16 = tmp.up_u16(f.planes); q.w_h16_inv_scale = tmp.up(f.inv_scale);
    up_ok = up_ok && q.w && q.w_sb && q.w_h16 && q.w_h16_inv_scale;
    if (conv_wino_form(KH, KW, stride, pad, C2, Cin, Cout, p.KWC, p.KWCp)) {
      std::vector<unsigned short> planes;
      std::vector<float> inv;
      wino_pack_weights(packed.data(), Cout, Cin, p.KWCp, &planes, &inv);
      q.w_wino = tmp.up_u16(planes); q.w_wino_inv = tmp.up(inv);
      up_ok = up_ok && q.w_wino && q.w_wino_inv;
    }
    const float* hb = h_bias ? h_bias[g] : nullptr;
    if (tab[g]) q.bias_tab = tmp.up(hb, (size_t)9 * Cout); else q.bias = tmp.up(hb, Cout);
    up_ok = up_ok && (!hb || q.bias || q.bias_tab);
    q.x = d_x[g]; q.x2 = C2 > 0 ? d_x2[g] : nullptr; q.res1 = d_res1 ? d_res1[g] : nullptr; q.res2 = d_res2 ? d_res2[g] : nullptr;
    if (hk[g]) {
      const int nout = hk[g] == 1 ? 2 : 1;
      q.head_w = tmp.up(h_head_w[g], (size_t)nout * 32); q.head_b = tmp.up(h_head_b[g], nout);
      q.head_out = d_head_out[g]; q.head_pn = d_pn ? d_pn[g] : nullptr;
      up_ok = up_ok && q.head_w && q.head_b;
    } else {
      q.y = d_y[g];
    }
  }
  if (!up_ok) { g_create_error = "pf_op_conv2d_g: hipMalloc failed"; tmp.sync_free(s); return PF_ERR_DEVICE; }
  if (S > 1) {  // the scratch laid out as conv_g lays it out: group g at part + g S M Cout
    void* d = nullptr;
    if (hipMalloc(&d, (size_t)S * groups * p.M * p.Cout * 4) != hipSuccess) { g_create_error = "pf_op_conv2d_g: hipMalloc failed"; tmp.sync_free(s); return PF_ERR_DEVICE; }
    tmp.p.push_back(d);
    for (int g = 0; g < groups; ++g) p.g[g].partial = static_cast<float*>(d) + (size_t)g * S * p.M * p.Cout;
    p.splitk = S;
  }
  if (!conv_tile_usable(p, tile)) {  // the real operand set must meet the rules the plan met
    g_create_error = fmt("pf_op_conv2d_g: tile %d (%s) refuses the uploaded operands", tile, conv_tile_name(tile));
    tmp.sync_free(s);
    return PF_ERR_ARG;
  }
  const long splitk_before = g_launch_counts.splitk;
  launch_conv_tile(p, tile, s);
  if (splitk_used && g_launch_counts.splitk != splitk_before) *splitk_used = p.splitk;  // what launch_conv_sb really did
  const int out = hipGetLastError() == hipSuccess ? PF_OK : PF_ERR_DEVICE;
  tmp.sync_free(s);
  return out;
}

}  // extern "C"
