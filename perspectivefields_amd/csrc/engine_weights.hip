// libpf_hip.so, the engine's weight store: checkpoint tensors -> packed, folded and split device weights (pf_finalize_weights -> pf_engine::build), the static
// bounds of tensors no kernel can watch, and the resize coefficient tables.  Host code only.
#include "engine.h"

namespace {

void resize_coeffs(int in_size, int out_size, ResizeTable* t) {
  const double scale = (double)in_size / out_size;
  const double filterscale = scale < 1.0 ? 1.0 : scale;
  const double support = 1.0 * filterscale;
  const int ksize = (int)std::ceil(support) * 2 + 1;
  t->ksize = ksize;
  t->bounds.assign((size_t)out_size * 2, 0);
  t->kk.assign((size_t)out_size * ksize, 0);
  std::vector<double> k(ksize);
  const double ss = 1.0 / filterscale;
  for (int xx = 0; xx < out_size; ++xx) {
    const double center = (xx + 0.5) * scale;
    double ww = 0.0;
    int xmin = (int)(center - support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(center + support + 0.5);
    if (xmax > in_size) xmax = in_size;
    xmax -= xmin;
    for (int x = 0; x < ksize; ++x) k[x] = 0.0;
    for (int x = 0; x < xmax; ++x) {
      double v = (x + xmin - center + 0.5) * ss;
      if (v < 0.0) v = -v;
      const double w = v < 1.0 ? 1.0 - v : 0.0;
      k[x] = w;
      ww += w;
    }
    for (int x = 0; x < xmax; ++x)
      if (ww != 0.0) k[x] /= ww;
    for (int x = 0; x < ksize; ++x)
      t->kk[(size_t)xx * ksize + x] = k[x] < 0 ? (int)(-0.5 + k[x] * (1 << 22)) : (int)(0.5 + k[x] * (1 << 22));
    t->bounds[2 * xx] = xmin;
    t->bounds[2 * xx + 1] = xmax;
  }
}

}  // namespace

// ------------------------------------------------------------------ weights
ResizeTable* pf_engine::resize_table(int in_size) {
  auto it = resize_tables.find(in_size);
  if (it != resize_tables.end()) return &it->second;
  ResizeTable& t = resize_tables[in_size];
  resize_coeffs(in_size, NET, &t);
  void *db = nullptr, *dk = nullptr;
  if (hipMalloc(&db, t.bounds.size() * 4) != hipSuccess || hipMalloc(&dk, t.kk.size() * 4) != hipSuccess) return nullptr;
  if (hipMemcpy(db, t.bounds.data(), t.bounds.size() * 4, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(dk, t.kk.data(), t.kk.size() * 4, hipMemcpyHostToDevice) != hipSuccess) return nullptr;
  dev_allocs.push_back(db); dev_allocs.push_back(dk);
  t.d_bounds = static_cast<int*>(db); t.d_kk = static_cast<int*>(dk);
  return &t;
}
float* pf_engine::upload(const std::vector<float>& v) {
  void* d = nullptr;
  if (host_only) {
    d = malloc(v.size() * sizeof(float) + 1);
    if (!d) throw std::string("malloc failed for weights");
    std::memcpy(d, v.data(), v.size() * sizeof(float));
    dev_allocs.push_back(d);
    return static_cast<float*>(d);
  }
  if (hipMalloc(&d, v.size() * sizeof(float)) != hipSuccess) throw std::string("hipMalloc failed for weights");
  if (hipMemcpy(d, v.data(), v.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) throw std::string("hipMemcpy H2D failed for weights");
  dev_allocs.push_back(d);
  return static_cast<float*>(d);
}
unsigned short* pf_engine::upload_u16(const std::vector<unsigned short>& v) {
  void* d = nullptr;
  if (host_only) {
    d = malloc(v.size() * 2 + 1);
    if (!d) throw std::string("malloc failed for weights");
    std::memcpy(d, v.data(), v.size() * 2);
    dev_allocs.push_back(d);
    return static_cast<unsigned short*>(d);
  }
  if (hipMalloc(&d, v.size() * 2) != hipSuccess) throw std::string("hipMalloc failed for weights");
  if (hipMemcpy(d, v.data(), v.size() * 2, hipMemcpyHostToDevice) != hipSuccess) throw std::string("hipMemcpy H2D failed for weights");
  dev_allocs.push_back(d);
  return static_cast<unsigned short*>(d);
}
// packed fp32 weights -> device, plus the split-bf16 planes when the layer is eligible for igemm_sb
void pf_engine::upload_conv_weights(ConvW& c, const std::vector<float>& packed, int CinP, int Cout) {
  c.w = upload(packed);
  if (split_bf16 && (CinP % 32 == 0 || CinP == 4)) {  // CinP == 4: the 3-channel stems (split-f16 "stem" form of igemm_sb_kernel)
    c.wsb = upload_u16(split_bf16x3(packed));
    const F16Planes f = split_f16x2(packed, Cout);
    c.wh16 = upload_u16(f.planes);
    c.wh16_inv = upload(f.inv_scale);
  }
}
const HostTensor& pf_engine::get(const std::string& key, std::initializer_list<int64_t> shape) {
  auto it = host.find(key);
  if (it == host.end()) throw fmt("missing checkpoint tensor '%s'", key.c_str());
  HostTensor& t = it->second;
  if (t.shape != std::vector<int64_t>(shape)) {
    std::string got, want;
    for (auto d : t.shape) got += std::to_string(d) + ",";
    for (auto d : shape) want += std::to_string(d) + ",";
    throw fmt("shape mismatch for '%s': got (%s) expected (%s)", key.c_str(), got.c_str(), want.c_str());
  }
  t.used = true;
  return t;
}
ConvW pf_engine::make_conv(const std::string& wkey, const std::string& bkey, int Cout, int Cin, int K, int stride, int pad,
                const double* out_scale, const std::vector<float>* bias_override) {
  ConvW c;
  const int CinP = roundup(Cin, 4);
  const HostTensor& w = get(wkey, {Cout, Cin, K, K});
  const std::vector<float> packed = pack_conv(w.data.data(), Cout, Cin, K, K, CinP, out_scale, &c.KWC, &c.KWCp);
  upload_conv_weights(c, packed, CinP, Cout);
  if (bias_override) c.b = upload(*bias_override);
  else if (!bkey.empty()) {
    std::vector<float> b = get(bkey, {Cout}).data;
    if (out_scale) for (int n = 0; n < Cout; ++n) b[n] = (float)(b[n] * out_scale[n]);
    c.b = upload(b);
  }
  c.Cout = Cout; c.Cin = CinP; c.CinReal = Cin; c.KH = c.KW = K; c.stride = stride; c.pad = pad;
  if (wino_min_hw > 0 && split_bf16 && K == 3 && stride == 1 && pad == 1 && CinP % 64 == 0 && Cout % 64 == 0 && c.KWCp == c.KWC) {
    std::vector<unsigned short> planes;
    std::vector<float> inv;
    wino_pack_weights(packed.data(), Cout, CinP, c.KWCp, &planes, &inv);
    c.wwino = upload_u16(planes);
    c.wwino_inv = upload(inv);
  }
  return c;
}
// ln_pfx != "" (and fuse_ln): the LayerNorm `ln_pfx` in front of this Linear is folded into it (fold_ln_linear)
ConvW pf_engine::make_linear(const std::string& pfx, int N, int K, const double* out_scale, const std::string& ln_pfx, float ln_eps) {
  ConvW c;
  const HostTensor& w = get(pfx + ".weight", {N, K});
  std::vector<float> b = get(pfx + ".bias", {N}).data;
  if (!ln_pfx.empty() && fuse_ln && K % 32 == 0 && N % 4 == 0) {
    const std::vector<float>& g = get(ln_pfx + ".weight", {K}).data;
    const std::vector<float>& be = get(ln_pfx + ".bias", {K}).data;
    std::vector<float> wf, bf, cs;
    fold_ln_linear(w.data.data(), b.data(), g.data(), be.data(), N, K, &wf, &bf, &cs);
    b = bf;
    upload_conv_weights(c, pack_conv(wf.data(), N, K, 1, 1, K, nullptr, &c.KWC, &c.KWCp), K, N);
    c.ln_s = upload(cs);
    c.ln_eps = ln_eps;
  } else {
    upload_conv_weights(c, pack_conv(w.data.data(), N, K, 1, 1, K, out_scale, &c.KWC, &c.KWCp), K, N);
    if (out_scale) for (int n = 0; n < N; ++n) b[n] = (float)(b[n] * out_scale[n]);
  }
  c.b = upload(b);
  c.Cout = N; c.Cin = K; c.CinReal = K; c.KH = c.KW = 1; c.stride = 1; c.pad = 0;
  return c;
}
// Linear(C -> 768) followed (no nonlinearity) by a zero-padded conv3x3(768 -> 256) is one conv3x3(C -> 256):
//   W'[o][ci][ky][kx] = sum_e Wp[o][e][ky][kx] * Wl[e][ci]
// and the Linear bias reaches an output pixel only through the taps that fall inside the map:
//   bias(y,x)[o] = bp[o] + sum_{valid (ky,kx)} T[o][ky][kx],   T[o][ky][kx] = sum_e Wp[o][e][ky][kx] * bl[e]
// -> a 9-entry table indexed by the 3x3 border case.  Folded in fp64 (reference: decode_head.py:49-53 +
// gravity_head.py:70-97,145-166).  8.2x fewer FLOPs for these layers (30.1 -> 3.7 GFLOP per head).
ConvW pf_engine::make_folded(const std::string& lin, const std::string& proc, int C) {
  const HostTensor& wl = get(lin + ".weight", {DEC_EMBED, C});
  const HostTensor& bl = get(lin + ".bias", {DEC_EMBED});
  const HostTensor& wp = get(proc + ".weight", {DEC_FEAT, DEC_EMBED, 3, 3});
  const HostTensor& bp = get(proc + ".bias", {DEC_FEAT});
  std::vector<float> wf((size_t)DEC_FEAT * C * 9);
  std::vector<double> T((size_t)DEC_FEAT * 9), acc(C);
  std::vector<double> wld(wl.data.begin(), wl.data.end());
  for (int o = 0; o < DEC_FEAT; ++o)
    for (int t = 0; t < 9; ++t) {
      std::fill(acc.begin(), acc.end(), 0.0);
      double tb = 0.0;
      for (int e = 0; e < DEC_EMBED; ++e) {
        const double a = wp.data[((size_t)o * DEC_EMBED + e) * 9 + t];
        const double* row = &wld[(size_t)e * C];
        for (int ci = 0; ci < C; ++ci) acc[ci] += a * row[ci];
        tb += a * (double)bl.data[e];
      }
      for (int ci = 0; ci < C; ++ci) wf[((size_t)o * C + ci) * 9 + t] = (float)acc[ci];
      T[(size_t)o * 9 + t] = tb;
    }
  ConvW c;
  upload_conv_weights(c, pack_conv(wf.data(), DEC_FEAT, C, 3, 3, C, nullptr, &c.KWC, &c.KWCp), C, DEC_FEAT);
  std::vector<float> tab((size_t)9 * DEC_FEAT);
  for (int cy = 0; cy < 3; ++cy)
    for (int cx = 0; cx < 3; ++cx)
      for (int o = 0; o < DEC_FEAT; ++o) {
        double b = bp.data[o];
        for (int ky = 0; ky < 3; ++ky)
          for (int kx = 0; kx < 3; ++kx) {
            const bool vy = !((cy == 0 && ky == 0) || (cy == 2 && ky == 2));  // top row has no tap above, bottom none below
            const bool vx = !((cx == 0 && kx == 0) || (cx == 2 && kx == 2));
            if (vy && vx) b += T[(size_t)o * 9 + ky * 3 + kx];
          }
        tab[(size_t)(cy * 3 + cx) * DEC_FEAT + o] = (float)b;
      }
  c.btab = upload(tab);
  c.b = nullptr;
  c.Cout = DEC_FEAT; c.Cin = C; c.CinReal = C; c.KH = c.KW = 3; c.stride = 1; c.pad = 1;
  return c;
}
LNW pf_engine::make_ln(const std::string& pfx, int C, float eps) {
  LNW l;
  l.g = upload(get(pfx + ".weight", {C}).data);
  l.b = upload(get(pfx + ".bias", {C}).data);
  l.C = C; l.eps = eps;
  return l;
}
// ---- static bounds of tensors no kernel can watch (LayerNorm outputs, the register-only hidden maps of the fused block MLPs): functions of the checkpoint alone
void pf_engine::note_static(double bound, float limit) { static_window_max = std::max(static_window_max, (float)std::min(3.0e38, bound * 65504.0 / std::max((double)limit, 1e-30))); }
double pf_engine::ln_bound(const std::string& pfx, int C) {  // |LN(x)_k| <= |gamma_k| sqrt(C) + |beta_k|
  const std::vector<float>& g = host.at(pfx + ".weight").data;
  const std::vector<float>& b = host.at(pfx + ".bias").data;
  double m = 0.0;
  for (int k = 0; k < C; ++k) m = std::max(m, std::fabs((double)g[k]) * std::sqrt((double)C) + std::fabs((double)b[k]));
  return m;
}
// hidden = GELU(dw3x3?(fc1(LN(x)))): max_n { sum_k |W1[n][k]| (|gamma_k| sqrt(C) + |beta_k|) + |b1[n]| }, through the depthwise conv when there is one
double pf_engine::mlp_hidden_bound(const std::string& ln, const std::string& fc1, const std::string& dw, int C) {
  const std::vector<float>& g = host.at(ln + ".weight").data;
  const std::vector<float>& be = host.at(ln + ".bias").data;
  const std::vector<float>& w = host.at(fc1 + ".weight").data;
  const std::vector<float>& b = host.at(fc1 + ".bias").data;
  const int H = 4 * C;
  double m = 0.0;
  for (int n = 0; n < H; ++n) {
    double a = std::fabs((double)b[n]);
    for (int k = 0; k < C; ++k) a += std::fabs((double)w[(size_t)n * C + k]) * (std::fabs((double)g[k]) * std::sqrt((double)C) + std::fabs((double)be[k]));
    if (!dw.empty()) {
      const std::vector<float>& dwv = host.at(dw + ".weight").data;
      const std::vector<float>& db = host.at(dw + ".bias").data;
      double ws = 0.0;
      for (int t = 0; t < 9; ++t) ws += std::fabs((double)dwv[(size_t)n * 9 + t]);
      a = ws * a + std::fabs((double)db[n]);
    }
    m = std::max(m, a);
  }
  return m;
}
DwW pf_engine::make_dw(const std::string& pfx, int C, int K) {
  DwW d;
  const std::vector<float>& wv = get(pfx + ".weight", {C, 1, K, K}).data;
  const std::vector<float>& bv = get(pfx + ".bias", {C}).data;
  d.w = upload(pack_dw(wv.data(), C, K));
  d.b = upload(bv);
  d.C = C;
  // |out| <= sum_k |w_k| max |in| + |b| (and |GELU(x)| <= |x| behind the 3x3): the producer of the input is watched with this limit (ConvW::sat_limit)
  double wsum = 0.0, bmax = 0.0;
  for (int ch = 0; ch < C; ++ch) {
    double a = 0.0;
    for (int k = 0; k < K * K; ++k) a += std::fabs((double)wv[(size_t)ch * K * K + k]);
    wsum = std::max(wsum, a);
    bmax = std::max(bmax, std::fabs((double)bv[ch]));
  }
  d.in_limit = (float)std::min(65504.0, std::max(0.0, 65504.0 - bmax) / std::max(wsum, 1e-30));
  return d;
}

RbLin pf_engine::make_rb(const std::string& pfx, int N, int K, int cols) {
  RbLin r;
  std::vector<unsigned short> st;
  std::vector<float> inv;
  rb_pack_w(get(pfx + ".weight", {N, K}).data.data(), N, K, cols, &st, &inv);
  r.w = upload_u16(st);
  r.bytes = st.size() * 2;
  r.inv = upload(inv);
  r.b = upload(get(pfx + ".bias", {N}).data);
  r.N = N; r.K = K;
  return r;
}

void pf_engine::build_head(Head& hd, const std::string& name, int nout, bool cls) {
  const std::string p = "persformer_heads." + name + "_head.";
  for (int k = 0; k < 4; ++k) {
    const std::string ks = std::to_string(k + 1);
    if (fold_mlp) {
      hd.fold[k] = make_folded(p + "linear_c" + ks + ".proj", p + "linear_c" + ks + "_proc", MIT_DIMS[k]);
    } else {
      hd.lin[k] = make_linear(p + "linear_c" + ks + ".proj", DEC_EMBED, MIT_DIMS[k]);
      hd.proc[k] = make_conv(p + "linear_c" + ks + "_proc.weight", p + "linear_c" + ks + "_proc.bias", DEC_FEAT, DEC_EMBED, 3, 1, 1);
    }
    const std::string f = p + "fusion" + ks + ".";
    if (k < 3) {
      hd.r1c1[k] = make_conv(f + "resConfUnit1.conv1.weight", f + "resConfUnit1.conv1.bias", DEC_FEAT, DEC_FEAT, 3, 1, 1);
      hd.r1c2[k] = make_conv(f + "resConfUnit1.conv2.weight", f + "resConfUnit1.conv2.bias", DEC_FEAT, DEC_FEAT, 3, 1, 1);
    }
    hd.r2c1[k] = make_conv(f + "resConfUnit2.conv1.weight", f + "resConfUnit2.conv1.bias", DEC_FEAT, DEC_FEAT, 3, 1, 1);
    hd.r2c2[k] = make_conv(f + "resConfUnit2.conv2.weight", f + "resConfUnit2.conv2.bias", DEC_FEAT, DEC_FEAT, 3, 1, 1);
  }
  if (wino_min_hw > 0)  // every 256-channel map of the decoder may be read by a Winograd conv (wino.hip: its input transform adds four values, no clamp)
    for (int k = 0; k < 4; ++k)
      for (ConvW* cw : {&hd.fold[k], &hd.proc[k], &hd.r1c1[k], &hd.r1c2[k], &hd.r2c1[k], &hd.r2c2[k]}) cw->sat_limit = 65504.f / 4.f;
  hd.conv0 = make_conv(p + "conv_fuse_conv0.conv.weight", p + "conv_fuse_conv0.conv.bias", 64, DEC_FEAT + LL_CH, 3, 1, 1);
  hd.conv1 = make_conv(p + "conv_fuse_conv1.conv.weight", p + "conv_fuse_conv1.conv.bias", 32, 64, 3, 1, 1);
  hd.nout = nout;
  const std::string pk = p + "linear_pred_" + name;
  if (cls) {
    hd.predcls = make_conv(pk + ".weight", pk + ".bias", nout, 32, 1, 1, 0);
  } else {
    hd.predw = upload(get(pk + ".weight", {nout, 32, 1, 1}).data);
    hd.predb = upload(get(pk + ".bias", {nout}).data);
  }
}

void pf_engine::build() {
  // MiT-B3
  int cin = 3;
  for (int s = 0; s < 4; ++s) {
    const int C = MIT_DIMS[s];
    const std::string pe = "backbone.patch_embed" + std::to_string(s + 1);
    stages[s].pe = make_conv(pe + ".proj.weight", pe + ".proj.bias", C, cin, MIT_PK[s], MIT_PS[s], MIT_PP[s]);
    stages[s].pen = make_ln(pe + ".norm", C, 1e-5f);  // nn.LayerNorm default eps (mix_transformers.py:224)
    if (s == 0 && stem7 && split_bf16 && stem7x7_supported(cin, C, MIT_PK[s], MIT_PS[s], MIT_PP[s])) {   // conv + LayerNorm of the first patch embedding as one kernel (stem7.hip)
      std::vector<unsigned short> wfr;
      std::vector<float> tab;
      stem7x7_pack(get(pe + ".proj.weight", {C, cin, 7, 7}).data.data(), nullptr, get(pe + ".proj.bias", {C}).data.data(), get(pe + ".norm.weight", {C}).data.data(),
                   get(pe + ".norm.bias", {C}).data.data(), &wfr, &tab);
      pe_s7_w = upload_u16(wfr); pe_s7_tab = upload(tab);
    }
    for (int i = 0; i < MIT_DEPTHS[s]; ++i) {
      const std::string b = "backbone.block" + std::to_string(s + 1) + "." + std::to_string(i);
      MitBlock mb;
      mb.n1 = make_ln(b + ".norm1", C, 1e-6f);  // mit_b3 norm_layer eps (:519)
      mb.n2 = make_ln(b + ".norm2", C, 1e-6f);
      // fused LayerNorms (fuse_ln): with spatial reduction norm1 also feeds the sr conv (several pixels per GEMM row) and stays a kernel;
      // without it (stage 4) q and kv are its only consumers.  The sr norm feeds kv only, norm2 feeds fc1 only.
      const bool sr1 = MIT_SR[s] == 1;
      mb.q = make_linear(b + ".attn.q", C, C, nullptr, sr1 ? b + ".norm1" : "", 1e-6f);
      mb.kv = make_linear(b + ".attn.kv", 2 * C, C, nullptr, sr1 ? b + ".norm1" : b + ".attn.norm", sr1 ? 1e-6f : 1e-5f);
      mb.proj = make_linear(b + ".attn.proj", C, C);
      if (MIT_SR[s] > 1) {
        mb.sr = make_conv(b + ".attn.sr.weight", b + ".attn.sr.bias", C, C, MIT_SR[s], MIT_SR[s], 0);
        mb.srn = make_ln(b + ".attn.norm", C, 1e-5f);  // Attention.norm default eps (:89)
      }
      mb.fc1 = make_linear(b + ".mlp.fc1", 4 * C, C, nullptr, b + ".norm2", 1e-6f);
      mb.dw = make_dw(b + ".mlp.dwconv.dwconv", 4 * C, 3);
      mb.fc2 = make_linear(b + ".mlp.fc2", C, 4 * C);
      if (fuse_mit_mlp && mit_mlp_preferred(C, mit_mlp128)) note_static(mlp_hidden_bound(b + ".norm2", b + ".mlp.fc1", b + ".mlp.dwconv.dwconv", C), 65504.f);  // hidden map of the fused Mlp (LDS / registers only)
      mb.q.sat_limit = 8188.f; mb.kv.sat_limit = 4094.f;  // the attention kernel's windows (attn.hip: q x 8, k / v x 16 inside the kernel)
      mb.fc1.sat_limit = mb.dw.in_limit;                   // fc1's output goes through the depthwise 3x3 before fc2 contracts it
      if (rb_chain && split_bf16 && rb_linear_supported(C, C) && MIT_SR[s] > 1) {  // stage 3: the row-block form of the block's linear layers
        mb.rq = make_rb(b + ".attn.q", C, C, 320);
        mb.rkv = make_rb(b + ".attn.kv", 2 * C, C, 320);
        mb.rproj = make_rb(b + ".attn.proj", C, C, 320);
        mb.rfc1 = make_rb(b + ".mlp.fc1", 4 * C, C, 320);
        mb.rfc2 = make_rb(b + ".mlp.fc2", C, 4 * C, 320);
        mb.rq.sat_limit = 8188.f; mb.rkv.sat_limit = 4094.f; mb.rfc1.sat_limit = mb.dw.in_limit;
        {  // proj followed by fc1 as ONE stream (rb_proj_fc1_kernel)
          std::vector<unsigned short> st1, st2;
          std::vector<float> inv1, inv2;
          rb_pack_w(get(b + ".attn.proj.weight", {C, C}).data.data(), C, C, 320, &st1, &inv1);
          rb_pack_w(get(b + ".mlp.fc1.weight", {4 * C, C}).data.data(), 4 * C, C, 320, &st2, &inv2);
          st1.resize(st1.size() - (size_t)4 * 10 * 2 * 512);
          st1.insert(st1.end(), st2.begin(), st2.end());
          mb.rpf.w = upload_u16(st1); mb.rpf.bytes = st1.size() * 2;
        }
        if (rb_srkv_supported(C, MIT_SR[s])) {
          int kwc = 0, kwcp = 0;
          const std::vector<float> srp = pack_conv(get(b + ".attn.sr.weight", {C, C, MIT_SR[s], MIT_SR[s]}).data.data(), C, C, MIT_SR[s], MIT_SR[s], C, nullptr, &kwc, &kwcp);  // [C][ky][kx C + ci]
          std::vector<unsigned short> st1, st2;
          std::vector<float> inv1, inv2;
          rb_pack_w(srp.data(), C, MIT_SR[s] * kwcp, 320, &st1, &inv1);
          rb_pack_w(get(b + ".attn.kv.weight", {2 * C, C}).data.data(), 2 * C, C, 320, &st2, &inv2);
          st1.resize(st1.size() - (size_t)4 * 10 * 2 * 512);  // drop the first stream's read-ahead padding: the kv steps follow directly
          st1.insert(st1.end(), st2.begin(), st2.end());
          mb.rsrkv.w = upload_u16(st1); mb.rsrkv.bytes = st1.size() * 2;
          mb.rsrkv.sr_inv = upload(inv1); mb.rsrkv.sr_b = upload(get(b + ".attn.sr.bias", {C}).data);
          mb.rsrkv.kv_inv = upload(inv2); mb.rsrkv.kv_b = upload(get(b + ".attn.kv.bias", {2 * C}).data);
          mb.qln = make_linear(b + ".attn.q", C, C, nullptr, b + ".norm1", 1e-6f);
          mb.qln.sat_limit = 8188.f;
        }
      }
      if (attn64 && split_bf16 && mit_attn64_supported(C, MIT_HEADS[s], 100) && MIT_SR[s] > 1) {
        std::vector<unsigned short> wfr;
        std::vector<float> tab;
        attn64_pack(get(b + ".norm1.weight", {C}).data.data(), get(b + ".norm1.bias", {C}).data.data(), get(b + ".attn.q.weight", {C, C}).data.data(), get(b + ".attn.q.bias", {C}).data.data(),
                    get(b + ".attn.proj.weight", {C, C}).data.data(), get(b + ".attn.proj.bias", {C}).data.data(), &wfr, &tab);
        mb.a64_w = upload_u16(wfr);
        mb.a64_tab = upload(tab);
      }
      if (thin128 && split_bf16 && thin128_supported(C, C) && MIT_SR[s] > 1) {   // stage 2: q (on norm1's output, which the spatial-reduction conv needs anyway) and proj + residual
        std::vector<unsigned short> wfr;
        std::vector<float> tab;
        thin128_pack(get(b + ".attn.q.weight", {C, C}).data.data(), get(b + ".attn.q.bias", {C}).data.data(), &wfr, &tab);
        mb.tq_w = upload_u16(wfr); mb.tq_tab = upload(tab);
        thin128_pack(get(b + ".attn.proj.weight", {C, C}).data.data(), get(b + ".attn.proj.bias", {C}).data.data(), &wfr, &tab);
        mb.tp_w = upload_u16(wfr); mb.tp_tab = upload(tab);
      }
      if (fuse_mit_mlp && mit_mlp_preferred(C, mit_mlp128)) {
        std::vector<unsigned short> wpk;
        std::vector<float> tab2;
        mit_mlp_pack(get(b + ".mlp.fc1.weight", {4 * C, C}).data.data(), get(b + ".mlp.fc1.bias", {4 * C}).data.data(), get(b + ".norm2.weight", {C}).data.data(),
                     get(b + ".norm2.bias", {C}).data.data(), get(b + ".mlp.dwconv.dwconv.weight", {4 * C, 1, 3, 3}).data.data(),
                     get(b + ".mlp.dwconv.dwconv.bias", {4 * C}).data.data(), get(b + ".mlp.fc2.weight", {C, 4 * C}).data.data(), get(b + ".mlp.fc2.bias", {C}).data.data(), C,
                     &wpk, &tab2);
        mb.mlp_w = upload_u16(wpk);
        mb.mlp_tab = upload(tab2);
      }
      stages[s].blocks.push_back(mb);
    }
    stages[s].norm = make_ln("backbone.norm" + std::to_string(s + 1), C, 1e-6f);
    cin = C;
  }
  // low-level encoder with eval BatchNorm folded (perspectivefields.py:70-83; BN eps 1e-5)
  {
    const std::vector<float>& g = get("ll_enc.bn1.weight", {LL_CH}).data;
    const std::vector<float>& be = get("ll_enc.bn1.bias", {LL_CH}).data;
    const std::vector<float>& mu = get("ll_enc.bn1.running_mean", {LL_CH}).data;
    const std::vector<float>& var = get("ll_enc.bn1.running_var", {LL_CH}).data;
    std::vector<double> sc(LL_CH);
    std::vector<float> bias(LL_CH);
    for (int n = 0; n < LL_CH; ++n) {
      sc[n] = (double)g[n] / std::sqrt((double)var[n] + 1e-5);
      bias[n] = (float)((double)be[n] - (double)mu[n] * sc[n]);
    }
    ll = make_conv("ll_enc.conv1.weight", "", LL_CH, 3, 7, 2, 3, sc.data(), &bias);
    if (stem7 && split_bf16 && stem7x7_supported(3, LL_CH, 7, 2, 3)) {
      std::vector<unsigned short> wfr;
      std::vector<float> tab;
      stem7x7_pack(get("ll_enc.conv1.weight", {LL_CH, 3, 7, 7}).data.data(), sc.data(), bias.data(), nullptr, nullptr, &wfr, &tab);
      ll_s7_w = upload_u16(wfr); ll_s7_tab = upload(tab);
    }
    auto it = host.find("ll_enc.bn1.num_batches_tracked");
    if (it != host.end()) it->second.used = true;
  }
  const bool cls = arch == PF_ARCH_PERSNET_CLS;
  build_head(heads[0], "gravity", cls ? 73 : 2, cls);
  build_head(heads[1], "latitude", cls ? 180 : 1, cls);
  has_param = arch != PF_ARCH_PERSNET_CLS;
  param_in = arch == PF_ARCH_PARAMNET_UNCENTERED ? 64 : NET;
  if (has_param) {
    const std::string p = "param_net.backbone.";
    cnx.nout = 5;
    cnx.stem = make_conv(p + "downsample_layers.0.0.weight", p + "downsample_layers.0.0.bias", CNX_DIMS[0], 3, 4, 4, 0);
    cnx.stemn = make_ln(p + "downsample_layers.0.1", CNX_DIMS[0], 1e-6f);
    for (int i = 1; i < 4; ++i) {
      const std::string d = p + "downsample_layers." + std::to_string(i);
      cnx.dsn[i - 1] = make_ln(d + ".0", CNX_DIMS[i - 1], 1e-6f);
      cnx.ds[i - 1] = make_conv(d + ".1.weight", d + ".1.bias", CNX_DIMS[i], CNX_DIMS[i - 1], 2, 2, 0);
    }
    for (int s = 0; s < 4; ++s) {
      const int C = CNX_DIMS[s];
      for (int j = 0; j < CNX_DEPTHS[s]; ++j) {
        const std::string b = p + "stages." + std::to_string(s) + "." + std::to_string(j);
        CnxBlock cb;
        cb.dw = make_dw(b + ".dwconv", C, 7);
        cb.n = make_ln(b + ".norm", C, 1e-6f);
        cb.pw1 = make_linear(b + ".pwconv1", 4 * C, C, nullptr, b + ".norm", 1e-6f);
        // layer scale gamma folded into pwconv2 (convnext.py:54-55: x = gamma * x)
        const std::vector<float>& gm = get(b + ".gamma", {C}).data;
        std::vector<double> sc(gm.begin(), gm.end());
        cb.pw2 = make_linear(b + ".pwconv2", C, 4 * C, sc.data());
        if (fuse_cnx_mlp && cnx_mlp_preferred(C)) {
          std::vector<unsigned short> wpk;
          std::vector<float> tab;
          cnx_mlp_pack(get(b + ".pwconv1.weight", {4 * C, C}).data.data(), get(b + ".pwconv1.bias", {4 * C}).data.data(), get(b + ".norm.weight", {C}).data.data(),
                       get(b + ".norm.bias", {C}).data.data(), get(b + ".pwconv2.weight", {C, 4 * C}).data.data(), get(b + ".pwconv2.bias", {C}).data.data(), gm.data(), C,
                       &wpk, &tab);
          cb.mlp_w = upload_u16(wpk);
          cb.mlp_tab = upload(tab);
        }
        // built whatever the precision mode or the batches to come (pf_set_precision may switch after the weights are loaded, the gate looks at each forward's batch):
        // 4.7 MB per 384-channel block, 19 MB per 768-channel block, 100 MB of HBM in all beside the GEMM pair's weights; PF_CNX_RB=5 leaves the 57 MB of stage 4 out
        if ((cnx_rb & 3) && cnx_rb_supported(C) && !((cnx_rb & 4) && C != 384)) {
          std::vector<unsigned short> wpk;
          std::vector<float> tab;
          cnx_rb_pack(get(b + ".pwconv1.weight", {4 * C, C}).data.data(), get(b + ".pwconv1.bias", {4 * C}).data.data(), get(b + ".pwconv2.weight", {C, 4 * C}).data.data(),
                      get(b + ".pwconv2.bias", {C}).data.data(), gm.data(), C, &wpk, &tab);
          cb.rb_w = upload_u16(wpk);
          cb.rb_w_bytes = wpk.size() * 2;
          cb.rb_tab = upload(tab);
        }
        cnx.blocks[s].push_back(cb);
      }
    }
    // windows of the residual stream: what block j writes is read by block j + 1's depthwise conv (then contracted raw by the LayerNorm-fused pwconv1)
    for (int s = 0; s < 4; ++s) {
      if (s > 0) cnx.ds[s - 1].sat_limit = cnx.blocks[s][0].dw.in_limit;
      for (size_t j = 0; j < cnx.blocks[s].size(); ++j) {
        const float lim = j + 1 < cnx.blocks[s].size() ? cnx.blocks[s][j + 1].dw.in_limit : 65504.f;
        cnx.blocks[s][j].out_limit = lim;
        cnx.blocks[s][j].pw2.sat_limit = lim;
      }
    }
    note_static(ln_bound(p + "downsample_layers.0.1", CNX_DIMS[0]), cnx.blocks[0][0].dw.in_limit);  // the stem's LayerNorm output feeds the first depthwise conv
    for (int s = 0; s < 4; ++s)
      for (int j = 0; j < CNX_DEPTHS[s]; ++j) {
        const std::string b = p + "stages." + std::to_string(s) + "." + std::to_string(j);
        if (cnx.blocks[s][j].mlp_w || cnx.blocks[s][j].rb_w) note_static(mlp_hidden_bound(b + ".norm", b + ".pwconv1", "", CNX_DIMS[s]), 65504.f);  // hidden map of the fused block MLP (registers only)
      }
    cnx.norm = make_ln(p + "norm", CNX_DIMS[3], 1e-6f);
    cnx.headw = upload(get(p + "head.weight", {cnx.nout, CNX_DIMS[3]}).data);
    cnx.headb = upload(get(p + "head.bias", {cnx.nout}).data);
  }
  for (auto& kv : host)
    if (!kv.second.used) throw fmt("unexpected checkpoint tensor '%s' for this architecture", kv.first.c_str());
  host.clear();
}
