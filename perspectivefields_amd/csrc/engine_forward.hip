// libpf_hip.so, the engine's forward: debug taps, layer helpers, the MiT-B3 walk with its fork windows, the decoders, ParamNet, run() and the workspace dry run.
// Host-side C++ here only *orchestrates* hand-written gfx950 kernels (igemm.hip, attn.hip, elem.hip, ...); there is no CPU or library (MIOpen / hipBLASLt) fallback.
#include "engine.h"

// ------------------------------------------------------------------ the internal streams and their events, created on first need
bool pf_engine::pstream_ready() {
  if (pstream) return true;
  int lo = 0, hi = 0;
  (void)hipDeviceGetStreamPriorityRange(&lo, &hi);  // lo = least urgent (largest number)
  const int prio = defer_prio > 0 ? hi : (defer_prio < 0 ? lo : 0);
  if ((defer_prio ? hipStreamCreateWithPriority(&pstream, hipStreamNonBlocking, prio) : hipStreamCreateWithFlags(&pstream, hipStreamNonBlocking)) != hipSuccess) { pstream = nullptr; return false; }
  if (hipEventCreateWithFlags(&ev_pn_in, hipEventDisableTiming) != hipSuccess || hipEventCreateWithFlags(&ev_pn_done, hipEventDisableTiming) != hipSuccess) {
    (void)hipStreamDestroy(pstream); pstream = nullptr; return false;
  }
  return true;
}
bool pf_engine::side_ready() {
  const bool need2 = side_stream_mode >= 2 || (dec_early > 0 && dec_early_stream != 1);  // caller's stream, side, side2, pstream: the four hardware queues of a process
  if (side && (side2 || !need2)) return true;
  if (!side) {
    if (hipStreamCreateWithFlags(&side, hipStreamNonBlocking) != hipSuccess) { side = nullptr; return false; }
    if (hipEventCreateWithFlags(&ev_fork, hipEventDisableTiming) != hipSuccess || hipEventCreateWithFlags(&ev_join, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&ev_ll, hipEventDisableTiming) != hipSuccess) return false;
    for (hipEvent_t* e : {&ev_de_fork, &ev_de[0], &ev_de[1], &ev_de[2]})
      if (hipEventCreateWithFlags(e, hipEventDisableTiming) != hipSuccess) { *e = nullptr; return false; }
  }
  if (need2 && !side2 && hipStreamCreateWithFlags(&side2, hipStreamNonBlocking) != hipSuccess) { side2 = nullptr; return false; }
  return true;
}

// ------------------------------------------------------------------ debug forward (shadow taps / range records)
void pf_engine::tap(Ctx& c, const std::string& name, const float* p, int B, int H, int W, int C) {
  DebugSink* d = c.dbg;
  if (!d || !d->shadow || !p) return;
  const size_t bytes = (size_t)B * H * W * C * 4, off = (d->used + 255) & ~(size_t)255;
  d->taps.push_back({name, off, {B, H, W, C}});
  d->used = off + bytes;
  if (c.dry) return;
  if (d->used > d->cap) { d->overflow = true; return; }
  (void)hipMemcpyAsync(d->buf + off, p, bytes, hipMemcpyDeviceToDevice, c.s);
}
void pf_engine::range_in(Ctx& c, const std::string& name, const float* p, size_t elems) {
  DebugSink* d = c.dbg;
  if (!d || !d->range || c.dry || !p || (int)d->ranges.size() >= d->max_ranges) return;
  launch_range_stats(p, (long)elems, d->stats + 4 * d->ranges.size(), c.s);
  d->ranges.push_back({name, (long long)elems});
}

// ------------------------------------------------------------------ layer helpers
// ups: calls[].x is stored at half resolution (H/2 x W/2); the conv runs on its bilinear x2 up-sampling (ConvParams::ups)
void pf_engine::conv_g(Ctx& c, int ngroups, const ConvCall* calls, int B, int H, int W, int act, int post_relu, int C1, int nchw, int ups) {
  const ConvW& w = *calls[0].w;
  const size_t Ho_ = (H + 2 * w.pad - w.KH) / w.stride + 1, Wo_ = (W + 2 * w.pad - w.KW) / w.stride + 1;
  // split-K scratch (conv_splitk_factor: deep-K launches with too few tiles for 256 CUs -- the MiT spatial-reduction convs); decided
  // from the shape and the call's operand set, so that the workspace dry run takes the same decision
  int splitk = 1;
  {
    bool plain = !nchw && !ups && !w.ln_s && w.Cin % 32 == 0 && w.KWCp > 0;
    for (int g = 0; g < ngroups; ++g)
      if (calls[g].head_kind || calls[g].w->btab || calls[g].res2 || calls[g].y.s.p || !calls[g].y.f || calls[g].x.s.p) plain = false;
    if (plain && split_bf16) splitk = conv_splitk_shape((long)B * Ho_ * Wo_, w.Cout, w.KH, w.KWCp, ngroups, splitk_mode);
  }
  const size_t mk_part = c.mark();
  float* part = splitk > 1 ? c.alloc((size_t)splitk * ngroups * B * Ho_ * Wo_ * w.Cout) : nullptr;
  struct Rel { Ctx& c; size_t m; ~Rel() { c.release(m); } } rel{c, mk_part};  // stream order makes the reuse safe
  if (c.dry) {
    c.max_conv_out = std::max(c.max_conv_out, (size_t)ngroups * B * Ho_ * Wo_ * w.Cout);
    return;
  }
  ConvParams p;
  p.groups = ngroups;
  for (int g = 0; g < ngroups; ++g) {
    const ConvW& wg = *calls[g].w;
    ConvPtrs& q = p.g[g];
    q.x = calls[g].x.f; q.x2 = calls[g].x2.f; q.w = wg.w; q.w_sb = wg.wsb; q.w_h16 = wg.wh16; q.w_h16_inv_scale = wg.wh16_inv; q.bias = wg.b; q.bias_tab = wg.btab;
    q.w_wino = wg.wwino; q.w_wino_inv = wg.wwino_inv;
    q.res1 = calls[g].res1; q.res2 = calls[g].res2; q.y = calls[g].y.f;
    q.x_sb = calls[g].x.s.p; q.x2_sb = calls[g].x2.s.p; q.y_sb = calls[g].y.s.p;
    q.ln_colsum = wg.ln_s;
    q.head_kind = calls[g].head_kind; q.head_w = calls[g].head_w; q.head_b = calls[g].head_b; q.head_out = calls[g].head_out; q.head_pn = calls[g].head_pn;
  }
  p.x_sb_plane = calls[0].x.s.plane; p.x2_sb_plane = calls[0].x2.s.plane; p.y_sb_plane = calls[0].y.s.plane;
  p.B = B; p.H = H; p.W = W;
  p.C1 = C1 < 0 ? w.Cin : C1; p.C2 = w.Cin - p.C1;
  p.KH = w.KH; p.KW = w.KW; p.stride = w.stride; p.pad = w.pad;
  p.Cout = w.Cout; p.KWC = w.KWC; p.KWCp = w.KWCp;
  p.act = act; p.post_relu = post_relu; p.nchw_out = nchw;
  p.nterms = nterms;
  p.ups = ups;
  p.wino_half = wino_half;
  p.ln = w.ln_s ? 1 : 0; p.ln_eps = w.ln_eps;
  p.sat = (c.tuning || c.dry) ? nullptr : d_sat; p.sat_limit = w.sat_limit;
  for (int g = 1; g < ngroups; ++g) p.sat_limit = std::min(p.sat_limit, calls[g].w->sat_limit);
  p.finish();
  if (part) {
    p.splitk = splitk;
    for (int g = 0; g < ngroups; ++g) p.g[g].partial = part + (size_t)g * splitk * p.M * p.Cout;
  }
  int tile = -1;
  {
    // operand formats are part of the key: a split-plane input changes which tile is fastest
    const int prec_code = nterms == NT_F16X3 ? 0 : 3;  // = PF_PRECISION_*
    const int fmt_bits = (calls[0].res1 ? 1 : 0) + (calls[0].res2 ? 2 : 0) + (calls[0].x.s.p ? 4 : 0) + (calls[0].y.s.p ? 8 : 0) + (calls[0].y.f ? 0 : 16) + 32 * prec_code + 128 * ups + 256 * (calls[0].head_kind ? 1 : 0);
    std::vector<int> key = {p.M, p.Cout, p.KH, p.KW, p.Cin, p.stride, p.H, p.W, ngroups, p.nchw_out, fmt_bits + 512 * p.ln, p.act};
    auto it = tile_cache.find(key);
    if (it == tile_cache.end() && p.ln && !(c.tuning && c.tune_scratch)) { key[10] = fmt_bits; it = tile_cache.find(key); }  // table without the fused form: same shape's tile
    if (it != tile_cache.end()) tile = it->second;
    else if (c.tuning && c.tune_scratch) { tile = tune_conv(p, c); tile_cache[key] = tile; }
  }
  if (!conv_tile_usable(p, tile)) tile = conv_default_tile(p);
  // Winograd form where it exists and the map is large enough (the tile table knows the direct tiles only); never while tuning (tune_conv times the direct tiles)
  if (wino_min_hw > 0 && wino_tile >= 0 && !(c.tuning && c.tune_scratch) && p.Ho >= wino_min_hw && p.Wo >= wino_min_hw && conv_tile_usable(p, wino_tile) &&
      conv_wino_blocks(p) >= wino_min_blocks) tile = wino_tile;
  if (c.dbg && c.dbg->range) {
    const int q = c.dbg->seq++;
    for (int g = 0; g < ngroups; ++g) {
      // "[winograd]": the layer runs as Winograd F(2x2, 3x3) -- its input transform adds four values, so its window ends at 65504 / 4 (PerspectiveFields._window_limit)
      const std::string nm = fmt("dense%03d%s %dx%d s%d %s%sM=%d N=%d K=%d", q, ngroups > 1 ? (g ? "[latitude]" : "[gravity]") : "", w.KH, w.KW, w.stride, w.ln_s ? "LN-fused " : "", tile >= 0 && strncmp(conv_tile_name(tile), "wino", 4) == 0 ? "[winograd] " : "", p.M, p.Cout, w.KH * w.KW * w.CinReal);
      range_in(c, nm + " x", calls[g].x.f, (size_t)B * (ups ? H / 2 : H) * (ups ? W / 2 : W) * p.C1);
      if (p.C2 > 0) range_in(c, nm + " x2", calls[g].x2.f, (size_t)B * H * W * p.C2);
    }
  }
  ProfScope ps(c.prof, c.s, conv_tile_is_sb(tile) ? PC_IGEMM_SB : PC_IGEMM, 2.0 * ngroups * p.M * (double)w.Cout * w.KH * w.KW * w.CinReal, p.M * ngroups, w.Cout, w.KH * w.KW * w.CinReal, w.KH);
  c.count(PF_DISPATCH_CONV_LAUNCHES);
  launch_conv_tile(p, tile, c.s);
}
// Measure, don't guess: run the launch with every tile configuration (outputs redirected to scratch so in-place
// residual layers are not disturbed) and keep the fastest.  Results are identical across tiles (same K order).
int pf_engine::tune_conv(const ConvParams& p0, Ctx& c) {
  ConvParams p = p0;
  const size_t out_elems = (size_t)p.M * p.Cout;
  unsigned short* sb_scratch = reinterpret_cast<unsigned short*>(c.tune_scratch + c.tune_scratch_elems);
  for (int g = 0; g < p.groups; ++g) {
    if (p.g[g].y) p.g[g].y = c.tune_scratch + g * out_elems;
    if (p.g[g].y_sb) p.g[g].y_sb = sb_scratch + g * out_elems;
  }
  p.y_sb_plane = (c.tune_scratch_elems & ~(size_t)1) | (p0.y_sb_plane & 1);
  hipEvent_t a, b;
  if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) return -1;
  int best = -1;
  float best_ms = 1e30f;
  for (int t = 0; t < conv_num_tiles(); ++t) {
    if (!conv_tile_usable(p, t)) continue;
    if (strncmp(conv_tile_name(t), "sbhA", 4) == 0 || strncmp(conv_tile_name(t), "sbhLA", 5) == 0 || strncmp(conv_tile_name(t), "sbhDMA", 6) == 0 || strncmp(conv_tile_name(t), "sbhREG", 6) == 0 || strncmp(conv_tile_name(t), "sbhV", 4) == 0 || strncmp(conv_tile_name(t), "sbA", 3) == 0 || strncmp(conv_tile_name(t), "sbPI_", 5) == 0 || strncmp(conv_tile_name(t), "sbI_", 4) == 0) continue;  // tuning builds: ablation forms (wrong results by construction) are for scripts/tune_conv.py only
    if (strncmp(conv_tile_name(t), "wino", 4) == 0) continue;  // the Winograd forms are chosen by map size (wino_min_hw), never by the table: a tuned-in Winograd tile on a small map would run with the
                                                               // 65504 / 4 window while the range records tag only `wino_tile` as "[winograd]"
    if (conv_tile_bn(t) > 32 && p.Cout <= 32) continue;
    if ((long)conv_tile_bm(t) * conv_tile_bn(t) > 16L * p.M * p.Cout) continue;  // tile far larger than the problem
    launch_conv_tile(p, t, c.s);  // warm-up (instruction cache, L2 state)
    float ms = 1e30f;
    bool ok = true;
    for (int rep = 0; rep < 2 && ok; ++rep) {  // best of two windows of two launches: one noisy window must not pick the tile
      (void)hipEventRecord(a, c.s);
      launch_conv_tile(p, t, c.s);
      launch_conv_tile(p, t, c.s);
      (void)hipEventRecord(b, c.s);
      ok = hipEventSynchronize(b) == hipSuccess;
      float w = 0.f;
      if (ok) { (void)hipEventElapsedTime(&w, a, b); ms = std::min(ms, w); }
    }
    if (!ok) break;
    if (ms < best_ms) { best_ms = ms; best = t; }
  }
  (void)hipEventDestroy(a); (void)hipEventDestroy(b);
  return best;
}
void pf_engine::conv(Ctx& c, const ConvW& w, Ten x, int B, int H, int W, Ten y, int act, const float* res1,
          const float* res2, int post_relu, Ten x2, int C1, int nchw) {
  ConvCall one{&w, x, y, res1, res2, x2};
  conv_g(c, 1, &one, B, H, W, act, post_relu, C1, nchw);
}
void pf_engine::gemm(Ctx& c, const ConvW& w, Ten x, long rows, Ten y, int act, const float* res1) {
  conv(c, w, x, 1, (int)rows, 1, y, act, res1);
}
// y.f may alias x; y may carry fp32, split planes, or both
void pf_engine::ln(Ctx& c, const LNW& l, const float* x, Ten y, long rows) {
  if (c.dry) return;
  c.count(PF_DISPATCH_LN_KERNEL_LAUNCHES);
  ProfScope ps(c.prof, c.s, PC_LAYERNORM, (4.0 + (y.f ? 4.0 : 0.0) + (y.s.p ? 6.0 : 0.0)) * rows * l.C);
  launch_layernorm(x, l.g, l.b, y.f, rows, l.C, l.eps, c.s, y.s.p, y.s.plane);
}

// a linear layer in the row-block form: y = act(LN?(x) W^T + b) + res on blocks of 64 tokens of one image (rb_gemm.hip)
void pf_engine::rb_linear(Ctx& c, const RbLin& r, const float* x, long M, int tokens, float* y, const LNW* lnw, int act, const float* res) {
  range_in(c, fmt("rb_linear %d->%d%s", r.K, r.N, lnw ? " (LN input)" : ""), x, (size_t)M * r.K);
  if (c.dry) return;
  RbLinArgs a;
  a.x = x; a.ln_g = lnw ? lnw->g : nullptr; a.ln_b = lnw ? lnw->b : nullptr; a.ln_eps = lnw ? lnw->eps : 0.f;
  a.w = r.w; a.w_bytes = r.bytes; a.inv = r.inv; a.bias = r.b; a.res = res; a.y = y;
  a.M = (int)M; a.tokens = tokens; a.bpi = (tokens + 63) / 64; a.N = r.N; a.act = act;
  a.sat = d_sat; a.sat_limit = r.sat_limit;
  ProfScope ps(c.prof, c.s, PC_IGEMM_SB, 2.0 * M * (double)r.N * r.K, (int)M, r.N, r.K, 1);
  c.count(PF_DISPATCH_RB_LAUNCHES);
  launch_rb_linear(a, r.K, c.s);
}

// a 128 -> 128 linear layer (+ residual) in the thin form (thin_linear.hip)
void pf_engine::thin(Ctx& c, const unsigned short* wfr, const float* tab, const float* x, const float* res, float* y, long M, float sat_limit, const char* what) {
  range_in(c, fmt("thin128 %s x", what), x, (size_t)M * 128);
  if (c.dry) return;
  ThinLinArgs a;
  a.x = x; a.res = res; a.y = y; a.wfr = wfr; a.tab = tab; a.M = M; a.sat = d_sat; a.sat_limit = sat_limit;
  ProfScope ps(c.prof, c.s, PC_IGEMM_SB, 2.0 * M * 128.0 * 128.0, (int)M, 128, 128, 1);
  c.count(PF_DISPATCH_THIN128_LAUNCHES);
  launch_thin128(a, num_cus, c.s);
}

// conv 7x7 on the normalised image (+ ReLU or + LayerNorm) as one launch of stem7.hip
void pf_engine::stem(Ctx& c, const unsigned short* wfr, const float* tab, const float* x4, float* y, int B, int H, int W, int stride, bool relu, bool lnorm, float eps, float sat_limit, const char* what) {
  range_in(c, fmt("stem7x7 s%d %s x", stride, what), x4, (size_t)B * H * W * 4);
  if (c.dry) return;
  Stem7Args a;
  a.x = x4; a.y = y; a.wfr = wfr; a.tab = tab; a.B = B; a.H = H; a.W = W; a.stride = stride; a.Ho = (H + 6 - 7) / stride + 1; a.Wo = (W + 6 - 7) / stride + 1;
  a.relu = relu ? 1 : 0; a.ln = lnorm ? 1 : 0; a.ln_eps = eps; a.sat = lnorm ? nullptr : d_sat; a.sat_limit = sat_limit;
  const long M = (long)B * a.Ho * a.Wo;
  ProfScope ps(c.prof, c.s, PC_IGEMM_SB, 2.0 * M * 64.0 * 147.0, (int)M, 64, 147, 7);
  launch_stem7x7(a, num_cus, c.s);
}

// ------------------------------------------------------------------ MiT-B3: one transformer block in three parts, the walk over the stages
// The attention inputs of a block, q and key / value, in their five forms (Attention.forward, mix_transformers.py:108-127).  Wherever q does not depend on the
// key / value branch's launches it may run beside them on `side` (beside(), window fw_q).  Returns whether it does: the caller joins in front of the attention.
bool pf_engine::block_attn_inputs(Ctx& c, MitBlock& mb, int blk, const StageDims& d, const BlockBufs& b, int B, const BlockForm& f, bool may_fork) {
  const int C = d.C, sr = d.sr;
  const long M = (long)B * d.N, Mkv = (long)B * d.kvh * d.kvw;
  float* const x = b.x;
  auto fork_q = [&] { return B >= 4 && (may_fork && can_fork(c)); };  // batch 1-3: a launch already under-fills the chip; the event pair would only add latency
  auto q_beside = [&](bool fork, auto q) { return beside(c, fork, side, ev_fork, ev_join, fw_q, q); };
  // the key / value branch launch by launch: spatial-reduction conv, its LayerNorm, kv
  auto sr_kv = [&](bool rb_kv) {
    conv(c, mb.sr, b.xn, B, d.Ho, d.Wo, Ten(b.srb));
    if (rb_kv) {  // measured slower than the LDS tile on these 3 200 rows (50 row blocks: 20.6 vs 12.7 us, profiles/r04_rb_linear.md)
      rb_linear(c, mb.rkv, b.srb, Mkv, d.kvh * d.kvw, b.kvb, &mb.srn);  // LayerNorm(sr conv) while the rows are staged
    } else if (mb.kv.ln_s) {
      gemm(c, mb.kv, Ten(b.srb), Mkv, Ten(b.kvb));  // LayerNorm(sr conv) inside the kv GEMM
    } else {
      ln(c, mb.srn, b.srb, b.srn, Mkv);
      gemm(c, mb.kv, b.srn, Mkv, Ten(b.kvb));
    }
  };
  if (sr > 1 && f.use_rb && (rb_chain & 32) && mb.rsrkv.w && mb.qln.ln_s && fuse_ln) {
    // key / value branch in ONE launch (LayerNorm-1 of the gathered source tokens, 2 x 2 conv, LayerNorm, kv: rb_chain.hip); q with LayerNorm-1 folded into its
    // GEMM beside it: no LayerNorm-1 launch, no split-K conv + reduce, no normalised map in HBM
    const bool forked = q_beside(fork_q(), [&](Ctx& cq) { gemm(cq, mb.qln, Ten(x), M, Ten(b.qb)); });
    range_in(c, fmt("rb_srkv s%d.b%d x (LN-fused)", d.s + 1, blk), x, (size_t)M * C);
    if (!c.dry) {
      RbSrKvArgs a;
      a.x = x; a.ln1_g = mb.n1.g; a.ln1_b = mb.n1.b; a.ln1_eps = mb.n1.eps;
      a.w = mb.rsrkv.w; a.w_bytes = mb.rsrkv.bytes; a.sr_inv = mb.rsrkv.sr_inv; a.sr_bias = mb.rsrkv.sr_b;
      a.srn_g = mb.srn.g; a.srn_b = mb.srn.b; a.srn_eps = mb.srn.eps; a.kv_inv = mb.rsrkv.kv_inv; a.kv_bias = mb.rsrkv.kv_b;
      a.kv = b.kvb; a.B = B; a.Hr = d.kvh; a.Wr = d.kvw; a.bpi = (d.kvh * d.kvw + 31) / 32; a.sat = d_sat;
      ProfScope ps(c.prof, c.s, PC_IGEMM_SB, 2.0 * Mkv * (double)C * (sr * sr * C + 2 * C), (int)Mkv, 3 * C, sr * sr * C + 2 * C, sr);
      c.count(PF_DISPATCH_RB_LAUNCHES);
      launch_rb_srkv(a, C, c.s);
    }
    return forked;
  }
  if (sr > 1 && f.fuse64) {
    // one head of 64 channels (stage 1): q, the attention core, proj and the residual run as ONE kernel (block_attn: attn_block.hip); norm1's output is still needed by
    // the spatial-reduction conv
    ln(c, mb.n1, x, b.xn, M);
    sr_kv(false);
    return false;
  }
  if (sr > 1) {
    const bool fork = fork_q(), rbq = f.use_rb && (rb_chain & 1);
    // q = LN1(x) Wq with the LayerNorm inside the kernel: independent of the LayerNorm launch below.  Forked it goes to the side stream in FRONT of that launch,
    // unforked it follows it
    auto q_rb = [&](Ctx& cq) { rb_linear(cq, mb.rq, x, M, (int)d.N, b.qb, &mb.n1); };
    if (rbq && fork) q_beside(true, q_rb);
    ln(c, mb.n1, x, b.xn, M);
    if (rbq) {
      if (!fork) q_rb(c);
    } else {  // q projection next to sr conv + kv GEMM: both read xn, attention needs both
      q_beside(fork, [&](Ctx& cq) { if (f.thin_q) thin(cq, mb.tq_w, mb.tq_tab, b.xn.f, nullptr, b.qb, M, mb.q.sat_limit, "q"); else gemm(cq, mb.q, b.xn, M, Ten(b.qb)); });
    }
    sr_kv(f.use_rb && (rb_chain & 2));
    return fork;
  }
  if (mb.q.ln_s && mb.kv.ln_s) {  // norm1 inside both of its consumers; q next to kv
    const bool forked = q_beside(fork_q(), [&](Ctx& cq) { gemm(cq, mb.q, Ten(x), M, Ten(b.qb)); });
    gemm(c, mb.kv, Ten(x), M, Ten(b.kvb));
    return forked;
  }
  ln(c, mb.n1, x, b.xn, M);
  gemm(c, mb.q, b.xn, M, Ten(b.qb));
  gemm(c, mb.kv, b.xn, M, Ten(b.kvb));
  return false;
}

// x += proj(attn(q, kv))            (Block.forward :199; Attention.forward :128-141)
void pf_engine::block_attn(Ctx& c, MitBlock& mb, int blk, const StageDims& d, const BlockBufs& b, int B, const BlockForm& f) {
  const int C = d.C, kvn = d.kvh * d.kvw;
  const long N = d.N, M = (long)B * N, Mkv = (long)B * kvn;
  float* const x = b.x;
  if (c.dbg && c.dbg->range) {
    if (!f.fuse64) range_in(c, fmt("attention s%d.b%d q", d.s + 1, blk), b.qb, (size_t)M * C);   // (fused: q never leaves the registers; the kernel watches it against the same window)
    range_in(c, fmt("attention s%d.b%d kv", d.s + 1, blk), b.kvb, (size_t)Mkv * 2 * C);
  }
  if (f.fuse64) {
    range_in(c, fmt("mit_attn64 s%d.b%d x (LN-fused)", d.s + 1, blk), x, (size_t)M * C);
    if (!c.dry) {
      MitAttn64Args a;
      a.x = x; a.kv = b.kvb; a.y = x; a.wfr = mb.a64_w; a.tab = mb.a64_tab; a.B = B; a.N = (int)N; a.M = kvn; a.ln_eps = mb.n1.eps; a.sat = d_sat; a.sat_limit = mb.proj.sat_limit;
      // work = q + proj (2 x 2 M C C) + QK^T + PV (4 M C kv)
      ProfScope ps(c.prof, c.s, PC_ATTN, 4.0 * M * C * (double)C + 4.0 * M * C * kvn);
      c.count(PF_DISPATCH_ATTN64_LAUNCHES);
      launch_mit_attn64(a, num_cus, c.s);
    }
    return;
  }
  if (!c.dry) {
    ProfScope ps(c.prof, c.s, PC_ATTN, 4.0 * M * C * kvn);  // QK^T + PV
    launch_sr_attention(b.qb, b.kvb, b.ab.f, B, (int)N, kvn, d.heads_n, c.s, b.ab.s.p, b.ab.s.plane);
  }
  if (f.pf_fused) {  // x += proj(attn); hidden = fc1(LN2(x)) in one launch (rb_chain.hip)
    range_in(c, fmt("rb_proj_fc1 s%d.b%d attn", d.s + 1, blk), b.ab.f, (size_t)M * C);
    if (!c.dry) {
      RbProjFc1Args a;
      a.attn = b.ab.f; a.x = x; a.w = mb.rpf.w; a.w_bytes = mb.rpf.bytes; a.proj_inv = mb.rproj.inv; a.proj_bias = mb.rproj.b;
      a.ln2_g = mb.n2.g; a.ln2_b = mb.n2.b; a.ln2_eps = mb.n2.eps; a.fc1_inv = mb.rfc1.inv; a.fc1_bias = mb.rfc1.b; a.hidden = b.hb;
      a.B = B; a.tokens = (int)N; a.bpi = ((int)N + 63) / 64; a.sat = d_sat; a.sat_limit = mb.rproj.sat_limit; a.hidden_limit = mb.rfc1.sat_limit;
      ProfScope ps(c.prof, c.s, PC_IGEMM_SB, 2.0 * M * (double)C * 5 * C, (int)M, 5 * C, C, 1);
      c.count(PF_DISPATCH_RB_LAUNCHES);
      launch_rb_proj_fc1(a, C, c.s);
    }
  } else if (f.use_rb && (rb_chain & 4)) rb_linear(c, mb.rproj, b.ab.f, M, (int)N, x, nullptr, ACT_NONE, x);
  else if (f.thin_q && mb.tp_w && b.ab.f) thin(c, mb.tp_w, mb.tp_tab, b.ab.f, x, x, M, mb.proj.sat_limit, "proj");
  else gemm(c, mb.proj, b.ab, M, Ten(x), ACT_NONE, x);
}

// x += fc2(gelu(dwconv(fc1(LN2(x)))))   (:200; Mlp.forward :49-56)
void pf_engine::block_mlp(Ctx& c, MitBlock& mb, int blk, const StageDims& d, BlockBufs& b, int B, const BlockForm& f) {
  const int C = d.C;
  const long N = d.N, M = (long)B * N;
  float* const x = b.x;
  if (d.fused_mlp && mb.mlp_w) {                  // norm2 + fc1 + depthwise 3x3 + GELU + fc2 + residual in one kernel, x -> xalt
    range_in(c, fmt("mit_mlp s%d.b%d x (LN-fused)", d.s + 1, blk), x, (size_t)M * C);
    if (!c.dry) {
      ProfScope ps(c.prof, c.s, PC_IGEMM_SB, 2.0 * 2.0 * M * (double)C * 4 * C, (int)M, C, 8 * C, 9);
      c.count(PF_DISPATCH_MIT_MLP_FUSED_LAUNCHES);
      launch_mit_mlp(x, b.xalt, mb.mlp_w, mb.mlp_tab, B, d.Ho, d.Wo, C, mb.n2.eps, c.s, d_sat, 65504.f);
    }
    std::swap(b.x, b.xalt);
    return;
  }
  if (f.pf_fused) {                               // fc1 ran with the output projection (block_attn)
  } else if (f.use_rb && (rb_chain & 8)) {
    rb_linear(c, mb.rfc1, x, M, (int)N, b.hb, &mb.n2);  // norm2 while the rows are staged
  } else if (mb.fc1.ln_s) {
    gemm(c, mb.fc1, Ten(x), M, Ten(b.hb));        // norm2 inside fc1
  } else {
    ln(c, mb.n2, x, b.xn, M);
    gemm(c, mb.fc1, b.xn, M, Ten(b.hb));
  }
  if (!c.dry) {
    ProfScope ps(c.prof, c.s, PC_DW3, (4.0 + (b.h2.f ? 4.0 : 0.0) + (b.h2.s.p ? 6.0 : 0.0)) * M * 4 * C);  // read + write of the hidden map
    launch_dwconv3x3_gelu(b.hb, mb.dw.w, mb.dw.b, b.h2.f, B, d.Ho, d.Wo, 4 * C, c.s, b.h2.s.p, b.h2.s.plane);
  }
  if (f.use_rb && (rb_chain & 16)) rb_linear(c, mb.rfc2, b.h2.f, M, (int)N, x, nullptr, ACT_NONE, x);
  else gemm(c, mb.fc2, b.h2, M, Ten(x), ACT_NONE, x);
}

// One transformer block on `B` images starting at token row 0 of the given buffers (Block.forward, mix_transformers.py:198-202).  gate_B: the batch the
// row-block gate is taken for (the whole batch, also when the block is issued for one half of it -- see the stage-3 split in mit())
void pf_engine::mit_block(Ctx& c, MitBlock& mb, int blk, const StageDims& d, BlockBufs& b, int B, int gate_B, bool may_fork) {
  const bool S = sba;
  const long M = (long)B * d.N;
  BlockForm f;
  f.thin_q = mb.tq_w && M >= thin128 && nterms == NT_F16X3 && !S && !c.tuning && b.xn.f;   // (thin_linear.hip; the same conditions hold for the output projection)
  f.fuse64 = attn64 && mb.a64_w && nterms == NT_F16X3 && !S && !c.tuning && d.sr > 1;
  // row-block form of the block's linear layers (stage 3 at batch >= ~14): q, kv, proj, fc1, fc2
  // one 64-row block per CU: the form pays only when the last round of blocks nearly fills the 256 CUs (same-box A/Bs, profiles/r04_rb_linear.md: B = 32 -> 224 blocks
  // +1.2 %, B = 64 -> 448 +1.2 %; B = 48 -> 336 -0.4 %, B = 24 -> 168 -0.9 %, B = 16 -> 112 -4.5 %)
  f.use_rb = rb_chain && mb.rq.w && nterms == NT_F16X3 && !S && !c.tuning && rb_gate((long)gate_B * ((d.N + 63) / 64));
  f.pf_fused = !f.fuse64 && f.use_rb && (rb_chain & 64) && mb.rpf.w;  // proj + norm2 + fc1 as one launch
  const bool forked = block_attn_inputs(c, mb, blk, d, b, B, f, may_fork);
  // "This block forked" is all the join asks.  (Before the fork helper it evaluated the fork's condition again, with `!fuse64` in front: the two differ only for a
  // block that takes the one-launch key / value branch AND the fused 64-channel attention, and build() gives no block both -- rsrkv.w needs C = 320
  // (rb_srkv_supported), a64_w needs C = 64 (mit_attn64_supported).)
  if (forked) (void)hipStreamWaitEvent(c.s, ev_join, 0);
  if (may_fork) fork_join(c, fw_q);  // (the stage-3 split keeps ITS window open over all blocks)
  block_attn(c, mb, blk, d, b, B, f);
  block_mlp(c, mb, blk, d, b, B, f);
}

// MiT-B3 forward_features (mix_transformers.py:449-485); feats[s] = NHWC stage outputs.
// With `sba` every tensor that only feeds GEMMs (LayerNorm outputs, attention output, the GELU'd hidden map) is
// written as split planes by its producer and never exists in fp32.
void pf_engine::mit(Ctx& c, int B, const float* x0, Ten feats[4], const Ten* llf) {
  const bool S = sba;
  Ten cur(const_cast<float*>(x0));
  int H = NET, W = NET;
  for (int s = 0; s < 4; ++s) {
    MitStage& st = stages[s];
    if (!c.dry && pn_later.armed && s + 1 == defer_at) issue_deferred();  // the previous forward's ParamNet branch goes beside this stage
    StageDims d;
    d.s = s; d.C = MIT_DIMS[s]; d.heads_n = MIT_HEADS[s]; d.sr = MIT_SR[s];
    d.Ho = (H + 2 * MIT_PP[s] - MIT_PK[s]) / MIT_PS[s] + 1; d.Wo = (W + 2 * MIT_PP[s] - MIT_PK[s]) / MIT_PS[s] + 1;
    d.N = (long)d.Ho * d.Wo; d.kvh = d.Ho / d.sr; d.kvw = d.Wo / d.sr;
    const int C = d.C, Ho = d.Ho, Wo = d.Wo;
    const long N = d.N, M = (long)B * N, Mkv = (long)B * d.kvh * d.kvw;
    BlockBufs b;
    b.x = c.alloc(M * C);  // token stream, updated in place by the residual epilogues
    // the fused Mlp (mit_mlp.hip) reads the halo rows of neighbouring blocks: it writes a second buffer and the two swap roles
    d.fused_mlp = !st.blocks.empty() && st.blocks[0].mlp_w && nterms == NT_F16X3 && (C != 128 || B >= mit_mlp128);
    b.xalt = d.fused_mlp ? c.alloc(M * C) : nullptr;
    const SbT xs = S ? c.alloc_sb(M * C) : SbT();  // split copy of the stage output (next patch embed + decoder)
    // PF_SIDE_STREAM=2 (measured: no gain): the low-level encoder conv (a full-chip launch of its own) next to the small launches of stages 3 / 4.
    // x0 is long since ready; ev_ll only orders the side stream behind this forward's beginning, and then says that the conv is done (run() waits for it)
    if (s == 2 && llf && B >= 4 && side_stream_mode >= 2 && can_fork(c))
      ll_forked = beside(c, true, side2, ev_ll, ev_ll, fw_ll, [&](Ctx& c2) { conv(c2, ll, Ten(const_cast<float*>(x0)), B, NET, NET, *llf, ACT_RELU); });
    if (s == 0 && pe_s7_w && nterms == NT_F16X3 && !c.tuning && cur.f) {
      stem(c, pe_s7_w, pe_s7_tab, cur.f, b.x, B, H, W, MIT_PS[s], false, true, st.pen.eps, 65504.f, "patch_embed1 + norm");
    } else {
      conv(c, st.pe, cur, B, H, W, Ten(b.x));
      ln(c, st.pen, b.x, Ten(b.x), M);
    }
    const size_t mk = c.mark();
    b.xn = c.ten(M * C, !S, S);
    b.qb = c.alloc(M * C);
    b.ab = c.ten(M * C, !S, S);
    b.srb = c.alloc(Mkv * C);
    b.srn = S ? Ten(nullptr, c.alloc_sb(Mkv * C)) : Ten(b.srb);  // LN(sr conv): in place, or planes only
    b.kvb = c.alloc(Mkv * 2 * C);
    b.hb = c.alloc(M * 4 * C);
    b.h2 = c.ten(M * 4 * C, !S, S);
    // PF_S3_SPLIT (stage 3 only, row-block form, batch >= 16 and even): the stage's 18 blocks are chains of ~6 dependent launches of <= 224 blocks each, every one
    // a single round whose time is a block's latency (prologue, K loop at one wave per SIMD, epilogue) -- the chip idles in every prologue, epilogue and launch gap.
    // Images are independent, so the batch is cut in two halves that walk the stage on TWO streams (the caller's and `side`, which gives up the q-beside-kv fork
    // for it: no additional hardware queue): two desynchronised chains of half-size launches fill each other's gaps.  Same kernels, same per-image arithmetic:
    // bit-identical to the one-stream walk (tests/test_gpu_r06.py::test_stage3_batch_split_is_bit_identical) wherever the LayerNorm-fused q GEMM, the one launch of
    // a block that goes through the row-count-keyed tile table, gets the same tile for M / 2 rows as for M (B = 32); at B = 64 the table has sb128x64 for 25 600
    // rows and sb64x64f2 for 12 800 (other roundings; with ONE tile forced for both, PF_CONV_TILE without a table, the walks are bit-identical): 1-cos 6e-8 between the
    // two walks (tests/test_gpu_batch_dispatch.py).
    // Measured (same box, profiles/r06_s3_split.md): batch 64 (two halves of 224 blocks, each a full round of its own) +2.2 %; batch 32 (halves of 112 blocks) -0.3 ... -1.8 %:
    // a half-size launch takes as long as the full one (a launch IS a block's latency), so the split pays only when EACH half still fills the chip -- the gate below
    // is the row-block form's gate taken for the half batch (PF_S3_SPLIT=2 forces the split whenever the whole batch passes it: the batch-32 A/B).
    const long rb_all = (long)B * ((N + 63) / 64), rb_half = rb_all / 2;
    bool split = s3_split && s == 2 && d.sr > 1 && !S && !d.fused_mlp && B >= 16 && B % 2 == 0 && !c.dry && !c.dbg && !c.tuning && !st.blocks.empty() && rb_chain && nterms == NT_F16X3 &&
                       st.blocks[0].rq.w && rb_gate(rb_all) && (s3_split >= 2 || rb_gate(rb_half)) && can_fork(c);
    // The second half walks the stage on a COPY of the bump allocator (a fork window, see fork_open): the split is sound only if a half-batch block allocates
    // NOTHING.  That holds for the default forms (key / value branch as one launch, LayerNorm-fused or row-block linears), but not for every PF_* combination: with
    // PF_FUSE_LN=0, or PF_RB_CHAIN without bit 32, each half runs the sr conv through conv_g, whose split-K partial (M = 3 200 rows at B = 64) both streams would
    // take from the same offset -- and which the unsplit dry run never sized.  So the gate ASKS: a dry walk of one block at the half batch (all blocks of the stage
    // have one shape; host arithmetic only, no launch) must leave the allocator untouched, whatever the switches are; otherwise the stage runs unsplit.
    if (split) {
      Ctx probe = c;
      probe.dry = true; probe.rep = nullptr;
      BlockBufs pb = b;
      mit_block(probe, st.blocks[0], 0, d, pb, B / 2, B, false);
      if (probe.nalloc != c.nalloc) split = false;
    }
    int blk = -1;
    if (split) {
      c.count(PF_DISPATCH_S3_SPLIT_TAKEN);
      BlockBufs b2 = b.second_half(M / 2, Mkv / 2, C);
      beside(c, true, side, ev_fork, ev_join, fw_q, [&](Ctx& c2) {  // the window's body issues BOTH halves, block by block: the first on c, the second on c2
        for (MitBlock& mb : st.blocks) {
          ++blk;
          mit_block(c, mb, blk, d, b, B / 2, B, false);
          mit_block(c2, mb, blk, d, b2, B / 2, B, false);
        }
      });
      (void)hipStreamWaitEvent(c.s, ev_join, 0);
      fork_join(c, fw_q);
    } else {
      for (MitBlock& mb : st.blocks) {
        if (blk >= 0) tap(c, fmt("mit.s%d.b%d", s + 1, blk), b.x, B, Ho, Wo, C);  // the previous block's output (token stream, pre stage norm)
        ++blk;
        mit_block(c, mb, blk, d, b, B, B, !(de.issued && dec_early_stream == 1));  // (`side` is taken while the early decoder window runs on it)
      }
    }
    c.release(mk);
    float* const x = b.x;
    if (blk >= 0) tap(c, fmt("mit.s%d.b%d", s + 1, blk), x, B, Ho, Wo, C);
    ln(c, st.norm, x, Ten(x, xs), M);  // stage norm; the normalised map is both the output and the next stage's input (:457-462)
    tap(c, fmt("c%d", s + 1), x, B, Ho, Wo, C);
    feats[s] = Ten(x, xs);
    cur = feats[s];
    H = Ho; W = Wo;
    if (s == 2) dec_early_issue(c, B, feats);  // c1 ... c3 are written: what the decoders can do without c4 starts here, beside stage 4
  }
}

// Both decoder heads up to their 32-channel 320x320 maps (gravity_head.py:139-173 / latitude_head.py:138-172).
// The two heads have identical shapes and independent weights, so every conv runs as ONE grouped launch
// (2x the grid: fewer partially filled last waves, half the launches); their tensors are allocated as
// [2][B][h][w][C] pairs so the bilinear kernels simply see a batch of 2B.
// Stored tensors are post-ReLU wherever every consumer applies ReLU first (ResidualConvUnit's in-place
// ReLU, decode_head.py:242-256): RCU(x) = conv2(relu(conv1(relu x))) + relu x.
// With `sba` a conv's epilogue writes split planes for the next conv (and fp32 only where a residual add reads it).
// pred_fused(): the regression heads' 1x1 prediction convs run inside conv_fuse_conv1's epilogue (no 32-channel map in HBM)
bool pf_engine::pred_fused() const { return fuse_pred && arch != PF_ARCH_PERSNET_CLS && nterms == NT_F16X3 && split_bf16; }
// a pair of per-head tensors, contiguous as [2][...] in fp32 and in every split plane
void pf_engine::dec_pair(Ctx& c, size_t per_head, bool want_f32, bool want_sb, Ten& a, Ten& b) {
  a = Ten(); b = Ten();
  if (want_f32) { a.f = c.alloc(2 * per_head); b.f = a.f + per_head; }
  if (want_sb) { a.s = c.alloc_sb(2 * per_head); b.s = a.s; b.s.p = a.s.p + per_head; }
}
bool pf_engine::dec_sr() const { return (sba && nterms != NT_F16X3) || (sba_heads && !sba && nterms == NT_F16X3 && split_bf16); }  // heads_fwd's SR
// The two decoder launches of a level that do not depend on the deeper level (heads_fwd): relu(fold[k](c_k)) and relu(r1c1[k](.)), both heads grouped
void pf_engine::dec_fold(Ctx& c, int k, int B, Ten feats[4], const Ten& p0, const Ten& p1) {
  const int h = NET >> (k + 2);
  ConvCall cc[2] = {{&heads[0].fold[k], feats[k], p0}, {&heads[1].fold[k], feats[k], p1}};
  conv_g(c, 2, cc, B, h, h, ACT_NONE, 1);                                   // relu(_ck), Linear folded into the conv
}
void pf_engine::dec_r1c1(Ctx& c, int k, int B, const Ten& p0, const Ten& p1, const Ten& t0, const Ten& t1) {
  const int h = NET >> (k + 2);
  ConvCall a[2] = {{&heads[0].r1c1[k], p0, t0}, {&heads[1].r1c1[k], p1, t1}};
  conv_g(c, 2, a, B, h, h, ACT_RELU);
}
// THE EARLY DECODER START (PF_DEC_EARLY).  heads_fwd walks the levels k = 3 ... 0 in order, but at levels 0-2 the folded first conv fold[k] reads only c_{k+1} =
// feats[k], and r1c1[k] reads only fold[k]'s output: the deeper level enters at r1c2[k], as the up[k+1] residual.  c1 ... c3 are complete when the stage-3 norm
// has run, so these launches -- large ones that fill the chip -- are issued there on a side stream, behind an event on the caller's stream, beside MiT stage 4
// (~25 dependent launches of 50 x N/64 small blocks) and the 10^2 / 20^2 decoder levels (one round of blocks each), which leave most CUs empty.  Same kernels, same
// tiles, same inputs: bit-identical to the forward order (tests/test_gpu_dec_early.py).
//   * order on the side stream: level 2, 1, 0 -- the order in which heads_fwd needs them; one event per level, which heads_fwd waits for in front of the
//     first consumer of the level's hoisted tensor (r1c1[k] in mode 1, r1c2[k] in mode 2).  The wait at level 0 is the join: every forward takes it.
//   * workspace: the hoisted outputs are allocated HERE, below stage 4's buffers, and are never released: no mark / release pair of stage 4 or of a decoder level
//     covers them.  The scratch of the early launches (split-K partials) lies right above them and the parent allocator SKIPS that range for the rest of the
//     forward, so the window's copy and the parent never allocate from one offset although both allocate.  The dry run walks the same code (dry_early), and
//     workspace_bytes sizes both layouts, this one and the forward order's, because the gates below can send a forward of either kind through one engine.
//   * the deferred ParamNet branch of the previous forward may still run: it reads its input map `pn` and works in its own region behind the main one; nothing
//     here touches either (run(): the join stays in front of the decoder levels; the first writer of `pn` is conv_fuse_conv1's epilogue).
//   * gates: the plain forward only -- not the debug forward (taps and range records keep forward order), not while tuning, not inside a full per-launch profile
//     (one stream; pf_profile_phases' decoder phase must hold the decoders' launches), not with PF_SIDE_STREAM=0, not below dec_early_min_batch.  Under graph
//     capture the fork and the join are event edges like the q fork's and are captured as such (the window closes inside every forward).
void pf_engine::dec_early_issue(Ctx& c, int B, Ten feats[4]) {
  const bool plain = !c.dbg && !c.tuning && (!c.prof || c.prof->min_work > 0.0);
  const bool want = dec_early > 0 && fold_mlp && side_stream_mode && B >= dec_early_min_batch && plain;
  // joined forwards (no deferred ParamNet branch) gain at B = 8 (+2.4 %) but LOSE at B = 32 (-2.6 %, profiles/r08_dec_early.md): there the path is taken only up to
  // dec_early_joined_max images; with the deferred branch it gains at every measured batch (8 ... 64)
  const bool pays = defer_params || B <= dec_early_joined_max;
  if (!want || !(c.dry ? dry_early : (pays && can_fork(c) && ev_de_fork && ev_de[0] && ev_de[1] && ev_de[2]))) return;
  const bool SR = dec_sr();
  de.layout = true;
  for (int k = 2; k >= 0; --k) {
    const size_t M = (size_t)B * (NET >> (k + 2)) * (NET >> (k + 2));
    dec_pair(c, M * DEC_FEAT, true, SR, de.p[k][0], de.p[k][1]);
    if (dec_early >= 2) dec_pair(c, M * DEC_FEAT, !SR, SR, de.t[k][0], de.t[k][1]);
  }
  hipStream_t es = dec_early_stream == 1 ? side : side2;
  Ctx c2 = c;
  if (!c.dry) {
    (void)hipEventRecord(ev_de_fork, c.s);
    (void)hipStreamWaitEvent(es, ev_de_fork, 0);
    c2 = fork_open(c, es, fw_de);
    c.count(PF_DISPATCH_DEC_EARLY_TAKEN);
    de.issued = true;
  }
  c2.peak = c2.off;  // from here: the high-water mark of the early launches' scratch
  for (int k = 2; k >= 0; --k) {
    dec_fold(c2, k, B, feats, de.p[k][0], de.p[k][1]);
    if (dec_early >= 2) dec_r1c1(c2, k, B, de.p[k][0], de.p[k][1], de.t[k][0], de.t[k][1]);
    if (!c.dry) (void)hipEventRecord(ev_de[k], es);
  }
  c.off = c2.peak;   // the parent skips that scratch: reserved until the forward ends
  if (c.off > c.peak) c.peak = c.off;
  if (c2.max_conv_out > c.max_conv_out) c.max_conv_out = c2.max_conv_out;
}
// heads_fwd, in front of the first consumer of level k's hoisted tensor
void pf_engine::dec_early_wait(Ctx& c, int k) {
  if (!de.issued) return;
  (void)hipStreamWaitEvent(c.s, ev_de[k], 0);
  if (k == 0) { fork_join(c, fw_de); de.issued = false; }
}
void pf_engine::heads_fwd(Ctx& c, int B, Ten feats[4], Ten llf, float* t32 /*[2][B][320][320][32], unused when the heads are fused*/, float* pg, float* pl, float* pn) {
  const bool S = sba && nterms != NT_F16X3;  // the 3x3 halo kernels of the decoder stage fp32 inputs: split-f16 planes only in MiT / ConvNeXt
  const bool SR = S || (sba_heads && !sba && nterms == NT_F16X3 && split_bf16);  // ResidualConvUnit chain in split planes (PF_SBA_HEADS: fp16 planes, halo kernel ASB)
  Head& hg = heads[0];
  Head& hl = heads[1];
  auto pair = [&](size_t per_head, bool want_f32, bool want_sb, Ten& a, Ten& b) { dec_pair(c, per_head, want_f32, want_sb, a, b); };
  // The two largest bilinear x2 maps -- up[0] (160^2 x 256) feeding conv_fuse_conv0 and the 320^2 x 64 map feeding
  // conv_fuse_conv1 (decode_head.py:284-286, gravity_head.py:170-172) -- are never materialised: the consuming 3x3 convs
  // interpolate them while staging their input halo tiles (ConvParams::ups; same expression, bit-identical results).
  const bool fuse_up = fuse_upsample && nterms == NT_F16X3 && split_bf16 && !S;
  Ten up[4][2], qfin[2];
  for (int k = 3; k >= 0; --k) {
    const int h = NET >> (k + 2);
    // up[k] is a residual operand (fp32) for k >= 1 and conv0's input (split planes) for k == 0
    if (k == 0 && fuse_up) pair((size_t)B * h * h * DEC_FEAT, true, false, qfin[0], qfin[1]);  // the 80^2 map conv0 up-samples on the fly
    else pair((size_t)B * 4 * h * h * DEC_FEAT, !(S && k == 0), S && k == 0, up[k][0], up[k][1]);
  }
  for (int k = 3; k >= 0; --k) {
    const int h = NET >> (k + 2);
    const size_t M = (size_t)B * h * h;
    const size_t mk = c.mark();
    // levels 0-2 of a forward with the early decoder start (dec_early_issue): fold[k] -- and r1c1[k] in mode 2 -- are already issued on the side stream, into
    // tensors allocated in front of MiT stage 4; this stream waits for the level's event in front of the first launch that reads one of them
    const bool hoist = de.layout && k < 3, hoist_t = hoist && dec_early >= 2;
    Ten p0, p1;
    if (hoist) { p0 = de.p[k][0]; p1 = de.p[k][1]; }
    else pair(M * DEC_FEAT, true, SR, p0, p1);
    if (hoist) {
    } else if (fold_mlp) {
      dec_fold(c, k, B, feats, p0, p1);
    } else {
      Ten e0, e1;
      pair(M * DEC_EMBED, !S, S, e0, e1);
      ConvCall l[2] = {{&hg.lin[k], feats[k], e0}, {&hl.lin[k], feats[k], e1}};
      conv_g(c, 2, l, 1, (int)M, 1);                                        // MLP (decode_head.py:49-53)
      ConvCall cc[2] = {{&hg.proc[k], e0, p0}, {&hl.proc[k], e1, p1}};
      conv_g(c, 2, cc, B, h, h, ACT_NONE, 1);                               // relu(_ck)
    }
    Ten o0 = p0, o1 = p1;
    if (k < 3) {                                                            // o = relu(up(prev) + RCU1(_ck))
      Ten t0, t1;
      if (hoist_t) { t0 = de.t[k][0]; t1 = de.t[k][1]; }
      else pair(M * DEC_FEAT, !SR, SR, t0, t1);
      if (hoist && !c.dry) dec_early_wait(c, k);                            // r1c1 reads p (mode 1); r1c2 reads t and p (mode 2)
      if (!hoist_t) dec_r1c1(c, k, B, p0, p1, t0, t1);
      pair(M * DEC_FEAT, true, SR, o0, o1);
      ConvCall b2[2] = {{&hg.r1c2[k], t0, o0, p0.f, up[k + 1][0].f}, {&hl.r1c2[k], t1, o1, p1.f, up[k + 1][1].f}};
      conv_g(c, 2, b2, B, h, h, ACT_NONE, 1);
    }
    Ten t0, t1, q0, q1;
    pair(M * DEC_FEAT, !SR, SR, t0, t1);
    ConvCall a[2] = {{&hg.r2c1[k], o0, t0}, {&hl.r2c1[k], o1, t1}};
    conv_g(c, 2, a, B, h, h, ACT_RELU);
    if (k == 0 && fuse_up) { q0 = qfin[0]; q1 = qfin[1]; }
    else pair(M * DEC_FEAT, true, false, q0, q1);
    ConvCall b2[2] = {{&hg.r2c2[k], t0, q0, o0.f}, {&hl.r2c2[k], t1, q1, o1.f}};
    conv_g(c, 2, b2, B, h, h);                                              // RCU2 output, raw
    if (!c.dry && !(k == 0 && fuse_up)) {                                   // decode_head.py:284-286
      const Ten& u = up[k][0];
      ProfScope ps(c.prof, c.s, PC_UPSAMPLE, (8.0 + (u.f ? 32.0 : 0.0) + (u.s.p ? 48.0 : 0.0)) * M * DEC_FEAT);
      launch_upsample2x(q0.f, u.f, 2 * B, h, h, DEC_FEAT, c.s, u.s.p, u.s.plane);
    }
    c.release(mk);
  }
  const int h = NET / 2;
  Ten z0, z1, zu0, zu1;
  pair((size_t)B * h * h * 64, true, false, z0, z1);
  ConvCall a[2] = {{&hg.conv0, fuse_up ? qfin[0] : up[0][0], z0, nullptr, nullptr, llf}, {&hl.conv0, fuse_up ? qfin[1] : up[0][1], z1, nullptr, nullptr, llf}};
  conv_g(c, 2, a, B, h, h, ACT_RELU, 0, DEC_FEAT, 0, fuse_up ? 1 : 0);     // cat (and the x2 up-sampling) fused into the A gather (:170-171)
  tap(c, "dec.gravity.conv0", z0.f, B, h, h, 64);
  tap(c, "dec.latitude.conv0", z1.f, B, h, h, 64);
  if (!fuse_up) {
    pair((size_t)B * NET * NET * 64, !S, S, zu0, zu1);
    if (!c.dry) {
      ProfScope ps(c.prof, c.s, PC_UPSAMPLE, (8.0 + (zu0.f ? 32.0 : 0.0) + (zu0.s.p ? 48.0 : 0.0)) * B * h * h * 64);
      launch_upsample2x(z0.f, zu0.f, 2 * B, h, h, 64, c.s, zu0.s.p, zu0.s.plane);
    }
  }
  ConvCall b2[2] = {{&hg.conv1, fuse_up ? z0 : zu0, Ten(t32)}, {&hl.conv1, fuse_up ? z1 : zu1, Ten(t32 ? t32 + (size_t)B * NET * NET * 32 : nullptr)}};
  if (pred_fused()) {
    b2[0].head_kind = 1; b2[0].head_w = hg.predw; b2[0].head_b = hg.predb; b2[0].head_out = pg; b2[0].head_pn = pn;
    b2[1].head_kind = 2; b2[1].head_w = hl.predw; b2[1].head_b = hl.predb; b2[1].head_out = pl; b2[1].head_pn = pn;
  }
  conv_g(c, 2, b2, B, NET, NET, ACT_RELU, 0, -1, 0, fuse_up ? 1 : 0);
}

// ConvNeXt-T + heads of the ParamNets (convnext.py:140-152)
void pf_engine::paramnet(Ctx& c, int B, const float* pn_in, float* d_params) {
  const bool S = sba;
  const float* src = pn_in;
  int H = NET;
  if (param_in != NET) {
    float* small = c.alloc((size_t)B * param_in * param_in * 4);
    if (!c.dry) launch_nearest_nhwc4(pn_in, small, B, NET, NET, param_in, param_in, c.s);
    src = small;
    H = param_in;
  }
  int h = H / 4;
  float* y = c.alloc((size_t)B * h * h * CNX_DIMS[0]);
  tap(c, "pn.in", src, B, H, H, 4);
  conv(c, cnx.stem, Ten(const_cast<float*>(src)), B, H, H, Ten(y));
  ln(c, cnx.stemn, y, Ten(y), (long)B * h * h);
  tap(c, "pn.stem", y, B, h, h, CNX_DIMS[0]);
  for (int s = 0; s < 4; ++s) {
    const int C = CNX_DIMS[s];
    if (s > 0) {
      const long Mi = (long)B * h * h;
      const Ten yn_in = S ? Ten(nullptr, c.alloc_sb(Mi * CNX_DIMS[s - 1])) : Ten(y);  // LN output feeds the 2x2 conv only
      ln(c, cnx.dsn[s - 1], y, yn_in, Mi);
      float* yn = c.alloc((size_t)B * (h / 2) * (h / 2) * C);
      conv(c, cnx.ds[s - 1], yn_in, B, h, h, Ten(yn));
      y = yn;
      h /= 2;
    }
    const long M = (long)B * h * h;
    const size_t mk = c.mark();
    float* d = c.alloc(M * C);
    const Ten dn = S ? Ten(nullptr, c.alloc_sb(M * C)) : Ten(d);
    const Ten hb = c.ten(M * 4 * C, !S, S);
    int blk = -1;
    // row-block form of the block MLP: one block per CU and one round, so it needs a batch that gives the stage enough row blocks
    const long cnx_rb_blocks = cnx_rb_supported(C) ? (M + cnx_rb_rows(C) - 1) / cnx_rb_rows(C) : 0;
    const bool use_cnx_rb = (cnx_rb & 3) && nterms == NT_F16X3 && !S && !c.tuning && cnx_rb_blocks > 0 && ((cnx_rb & 3) == 2 || cnx_rb_blocks >= cnx_rb_min_blocks[C == 384 ? 0 : 1]);
    for (CnxBlock& cb : cnx.blocks[s]) {
      if (blk >= 0) tap(c, fmt("pn.s%d.b%d", s + 1, blk), y, B, h, h, C);
      ++blk;
      if (!c.dry) {
        ProfScope ps(c.prof, c.s, PC_DW7, 8.0 * M * C);
        launch_dwconv7x7(y, cb.dw.w, cb.dw.b, d, B, h, h, C, c.s);
      }
      if (cb.mlp_w && nterms == NT_F16X3) {         // norm + pwconv1 + GELU + pwconv2 + layer scale + residual in one kernel
        range_in(c, fmt("cnx_mlp s%d.b%d d (LN-fused)", s + 1, blk), d, (size_t)M * C);
        if (!c.dry) {
          ProfScope ps(c.prof, c.s, PC_IGEMM_SB, 2.0 * 2.0 * M * (double)C * 4 * C, (int)M, C, 8 * C, 1);
          launch_cnx_mlp(d, y, cb.mlp_w, cb.mlp_tab, M, C, cb.n.eps, c.s, d_sat, cb.out_limit);
        }
        continue;
      }
      if (cb.rb_w && use_cnx_rb) {                  // the same, rows resident in LDS (cnx_rb.hip)
        range_in(c, fmt("cnx_rb s%d.b%d d (LN input)", s + 1, blk), d, (size_t)M * C);
        if (!c.dry) {
          CnxRbArgs a;
          a.d = d; a.y = y; a.w = cb.rb_w; a.w_bytes = cb.rb_w_bytes; a.tab = cb.rb_tab; a.ln_g = cb.n.g; a.ln_b = cb.n.b; a.ln_eps = cb.n.eps; a.M = (int)M;
          a.sat = d_sat; a.sat_limit = cb.out_limit;
          ProfScope ps(c.prof, c.s, PC_IGEMM_SB, 2.0 * 2.0 * M * (double)C * 4 * C, (int)M, C, 8 * C, 1);
          c.count(PF_DISPATCH_CNX_RB_LAUNCHES);
          launch_cnx_rb(a, C, c.s);
        }
        continue;
      }
      if (cb.pw1.ln_s) {
        gemm(c, cb.pw1, Ten(d), M, hb, ACT_GELU);   // block norm inside pwconv1
      } else {
        ln(c, cb.n, d, dn, M);
        gemm(c, cb.pw1, dn, M, hb, ACT_GELU);
      }
      gemm(c, cb.pw2, hb, M, Ten(y), ACT_NONE, y);  // y += gamma * pwconv2(...)  (gamma folded)
    }
    if (blk >= 0) tap(c, fmt("pn.s%d.b%d", s + 1, blk), y, B, h, h, C);
    c.release(mk);
  }
  float* raw = c.alloc((size_t)B * 8);
  if (!c.dry) {
    launch_gap_ln_head(y, cnx.norm.g, cnx.norm.b, cnx.headw, cnx.headb, raw, B, h * h, CNX_DIMS[3], cnx.nout, cnx.norm.eps, c.s);
    launch_paramnet_scalars(raw, cnx.nout, d_params, B, arch == PF_ARCH_PARAMNET_CENTERED ? 0 : 1, c.s);
  }
}

void pf_engine::run(Ctx& c, int B, const void* in, bool is_u8, float* pg, float* pl, float* params) {
  if (!c.dry && pn_pending && (B != pn_pending_B || c.base != pn_pending_base)) {
    // a deferred branch works at an offset that depends on ITS batch size (behind that batch's main region): a forward with another batch size, or in another
    // workspace buffer, would lay its main region over it (or leave it behind in a buffer the caller may free) -- join before anything of this forward is issued
    join_deferred(c.s);
  }
  float* x0 = c.alloc((size_t)B * NET * NET * 4);
  if (!c.dry && c.prof) c.prof->mark(PH_BACKBONE, c.s);   // input normalisation + MiT-B3
  if (!c.dry) {
    if (is_u8) launch_prep_u8(static_cast<const uint8_t*>(in), x0, (long)B * NET * NET, mean3, std3, c.s);
    else launch_prep_f32_nchw(static_cast<const float*>(in), x0, B, NET * NET, mean3, std3, c.s);
  }
  Ten feats[4];
  // low-level encoder output: conv0's second (concatenated) input only
  const bool Sh = sba && nterms != NT_F16X3;  // as in heads_fwd: the decoder's halo kernels read fp32
  const Ten llf = c.ten((size_t)B * (NET / 2) * (NET / 2) * LL_CH, !Sh, Sh);
  ll_forked = false;
  de = DecEarly();
  mit(c, B, x0, feats, &llf);
  if (!c.dry && c.prof) c.prof->mark(PH_LL, c.s);
  if (ll_forked) { (void)hipStreamWaitEvent(c.s, ev_ll, 0); fork_join(c, fw_ll); }
  else if (ll_s7_w && nterms == NT_F16X3 && !c.tuning && llf.f && !llf.s.p) stem(c, ll_s7_w, ll_s7_tab, x0, llf.f, B, NET, NET, 2, true, false, 0.f, ll.sat_limit, "low-level encoder");
  else conv(c, ll, Ten(x0), B, NET, NET, llf, ACT_RELU);  // BN folded (perspectivefields.py:79-83)
  tap(c, "ll", llf.f, B, NET / 2, NET / 2, LL_CH);
  const bool pf = pred_fused();
  float* tg = pf ? nullptr : c.alloc((size_t)2 * B * NET * NET * 32);
  float* tl = pf ? nullptr : tg + (size_t)B * NET * NET * 32;
  // ParamNet's input map and activations live in their own region behind the main one (run_pn_peak: its size, from the dry run), so that a deferred branch
  // (defer_params) never shares memory with the next forward's backbone / decoders
  Ctx cp = c;
  cp.off = 0; cp.peak = 0;
  if (!c.dry) cp.base = c.base + pn_off[B];
  float* pn = has_param ? cp.alloc((size_t)B * NET * NET * 4) : nullptr;
  // The join of the previous forward's deferred branch stays in front of the decoder levels.  The first launch of this forward that writes `pn` is the last one,
  // conv_fuse_conv1 (its fused prediction epilogue; launch_pred_regression when the heads are not fused), so the decoder launches that dec_early_issue() has
  // already put on a side stream -- fold[k] / r1c1[k], which read c1 ... c3 and write the main region only -- are on the safe side of it.
  if (!c.dry && pn_pending) join_deferred(c.s);  // the previous forward's deferred branch still reads pn / writes its activations: the decoders below overwrite pn
  const size_t mk = c.mark();
  if (!c.dry && c.prof) c.prof->mark(PH_DECODERS, c.s);   // both decoder heads + prediction heads
  heads_fwd(c, B, feats, llf, tg, pg, pl, pn);
  c.release(mk);
  if (arch == PF_ARCH_PERSNET_CLS) {
    // 1x1 convs to 73 / 180 logits, stored NCHW because the logits are API-visible (gravity_head.py:259)
    conv(c, heads[0].predcls, Ten(tg), B, NET, NET, Ten(pg), ACT_NONE, nullptr, nullptr, 0, Ten(), -1, 1);
    conv(c, heads[1].predcls, Ten(tl), B, NET, NET, Ten(pl), ACT_NONE, nullptr, nullptr, 0, Ten(), -1, 1);
    if (!c.dry && c.prof) c.prof->mark(PH_END, c.s);
    return;
  }
  if (!c.dry && !pf)
    launch_pred_regression(tg, tl, heads[0].predw, heads[0].predb, heads[1].predw, heads[1].predb, pg, pl, pn, B, NET * NET, c.s);
  if (!c.dry && c.prof) c.prof->mark(has_param ? PH_PARAMNET : PH_END, c.s);
  if (has_param) {
    const bool defer = defer_params && !c.dry && (!c.prof || c.prof->min_work > 0.0) && !c.dbg && !c.tuning && !in_capture && pstream_ready();
    if (defer) {
      (void)hipEventRecord(ev_pn_in, c.s);
      (void)hipStreamWaitEvent(pstream, ev_pn_in, 0);
      cp.s = pstream;
    }
    if (defer && defer_at > 0) {  // issued by the next forward (mit(), stage defer_at) or by whoever needs the result first
      pn_later.armed = true; pn_later.B = B; pn_later.pn = pn; pn_later.params = params; pn_later.ctx = cp;
      pn_pending = true; pn_pending_B = B; pn_pending_base = c.base;
    } else {
      paramnet(cp, B, pn, params);
      if (defer) {
        (void)hipEventRecord(ev_pn_done, pstream);
        pn_pending = true; pn_pending_B = B; pn_pending_base = c.base;
      }
    }
  }
  if (!c.dry && c.prof && has_param) c.prof->mark(PH_END, c.s);
  run_pn_peak = cp.peak;
  if (cp.max_conv_out > c.max_conv_out) c.max_conv_out = cp.max_conv_out;
}

// with_scratch: plus the target of the tuning launches (largest conv output as fp32 + 3 bf16 planes) -- pf_autotune only
size_t pf_engine::workspace_bytes(int B, bool with_scratch) {
  auto it = ws_cache.find(B);
  if (it == ws_cache.end()) {
    // two layouts, one engine: the forward order's and the early decoder start's (dec_early_issue: hoisted decoder tensors below stage 4) -- which one a forward
    // takes is decided per call (debug forward, profile window, ...), so the regions are sized for the larger of the two
    size_t main_peak = 0, pn_bytes = 0, conv_out = 0;
    for (int early = 0; early < 2; ++early) {
      Ctx c{nullptr, 4096, 0, 0, true, nullptr};
      c.sb_planes = nterms == NT_F16X3 ? 2 : 3;
      dry_early = early != 0;
      run(c, B, nullptr, true, nullptr, nullptr, nullptr);
      dry_early = false;
      main_peak = std::max(main_peak, (c.peak + 255) & ~(size_t)255);
      pn_bytes = std::max(pn_bytes, (run_pn_peak + 255) & ~(size_t)255);
      conv_out = std::max(conv_out, c.max_conv_out);
    }
    const size_t total = main_peak + pn_bytes;
    pn_off[B] = main_peak;
    pn_peak[B] = pn_bytes;
    ws_cache[B] = total + 4096;
    scratch_off[B] = total;
    scratch_elems[B] = conv_out;
    it = ws_cache.find(B);
  }
  return it->second + ((with_scratch || autotune) ? scratch_elems[B] * 10 + 4096 : 0);
}
int pf_engine::forward(int B, const void* in, bool is_u8, float* pg, float* pl, float* params, void* ws, size_t ws_bytes, hipStream_t s, bool tune) {
  if (host_only) return fail(PF_ERR_DEVICE, "this engine was created with PF_DEVICE_NONE (host side only): no forward");
  if (!finalized) return fail(PF_ERR_WEIGHTS, "pf_forward called before pf_finalize_weights");
  if (B <= 0 || !in || !pg || !pl || !ws) return fail(PF_ERR_ARG, "pf_forward: null pointer or batch <= 0");
  if (has_param && !params) return fail(PF_ERR_ARG, "pf_forward: d_params is required for a ParamNet architecture");
  // The implicit-GEMM kernels address every activation with 32-bit BYTE offsets and use offset 2^31 as the "reads as
  // zero" marker (igemm_common.h OOB): each per-head activation must stay below 2 GiB.  The largest are the
  // 160x160x256 decoder map and the 320x320x64 map before conv_fuse_conv1: B * 26.2 MB  ->  B <= PF_MAX_BATCH (81).
  if (B > PF_MAX_BATCH) return fail(PF_ERR_ARG, fmt("pf_forward: batch %d exceeds PF_MAX_BATCH = %d (32-bit byte offsets inside one activation); split the batch", B, PF_MAX_BATCH));
  const size_t need = workspace_bytes(B, tune);
  if (ws_bytes < need) return fail(PF_ERR_WORKSPACE, fmt("workspace too small: %zu < %zu bytes", ws_bytes, need));
  if (hipSetDevice(device) != hipSuccess) return fail(PF_ERR_DEVICE, "hipSetDevice failed");
  uintptr_t base = (reinterpret_cast<uintptr_t>(ws) + 255) & ~(uintptr_t)255;
  Ctx c{s, base, 0, 0, false, nullptr};
  c.sb_planes = nterms == NT_F16X3 ? 2 : 3;
  c.prof = prof.on ? &prof : nullptr;
  c.dbg = debug_sink;
  if (tune) {
    c.tuning = true;
    c.tune_scratch = reinterpret_cast<float*>(base + scratch_off[B]);
    c.tune_scratch_elems = scratch_elems[B];
  }
  std::fill(dispatch, dispatch + PF_DISPATCH_COLS, (int64_t)0);
  if (!tune) c.rep = dispatch;
  const LaunchCounts lc0 = g_launch_counts;
  g_launch_counts.splitk_max = 0;
  fw_q.open = fw_ll.open = fw_de.open = false;
  run(c, B, in, is_u8, pg, pl, params);
  const LaunchCounts lc1 = g_launch_counts;
  g_launch_counts.splitk_max = std::max(lc0.splitk_max, lc1.splitk_max);
  dispatch[PF_DISPATCH_BATCH] = B;
  dispatch[PF_DISPATCH_SPLITK_LAUNCHES] = lc1.splitk - lc0.splitk;
  dispatch[PF_DISPATCH_SPLITK_MAX_FACTOR] = lc1.splitk_max;
  dispatch[PF_DISPATCH_WINO_LAUNCHES] = lc1.wino - lc0.wino;
  dispatch[PF_DISPATCH_WINO_HALF_LAUNCHES] = lc1.wino_half - lc0.wino_half;
  // the dry run promised the caller's buffer two regions (main, ParamNet behind it at pn_off): the real run must have stayed inside both
  const size_t real_main = (c.peak + 255) & ~(size_t)255, real_pn = (run_pn_peak + 255) & ~(size_t)255;
  dispatch[PF_DISPATCH_REAL_PEAK_BYTES] = (int64_t)(real_main + real_pn);
  dispatch[PF_DISPATCH_DRY_PEAK_BYTES] = (int64_t)(pn_off[B] + pn_peak[B]);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(PF_ERR_DEVICE, fmt("kernel launch failed: %s", hipGetErrorString(e)));
  if (real_main > pn_off[B] || real_pn > pn_peak[B])
    return fail(PF_ERR_WORKSPACE, fmt("the forward allocated past what pf_workspace_bytes(%d) sized: main region %zu > %zu or ParamNet region %zu > %zu bytes (the launches were issued: the workspace and outputs of this call are not to be trusted)", B, real_main, pn_off[B], real_pn, pn_peak[B]));
  return PF_OK;
}
