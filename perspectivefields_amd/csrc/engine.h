// The engine of libpf_hip.so as its translation units share it: architecture constants, weight structs, the bump allocator's context, the debug and profile
// records, and struct pf_engine -- data members here, member functions in engine_weights.hip (checkpoint -> device weights), engine_forward.hip (the layer walk and
// the workspace sizing) and engine.hip (C ABI).
#pragma once
#include <map>
#include <unordered_map>

#include "host_pack.h"  // (brings the HIP runtime, include/pf_hip.h, pf_kernels.h and the standard headers the packers use)

namespace pf_host {

// ---- architecture constants (reference: mix_transformers.py:511-524, gravity_head.py:121-137, convnext.py:78-79)
constexpr int NET = PF_NET_SIZE;
static_assert((size_t)PF_MAX_BATCH * PF_NET_SIZE * PF_NET_SIZE * 64 * 4 <= 0x7fffffffull &&
              (size_t)PF_MAX_BATCH * (PF_NET_SIZE / 2) * (PF_NET_SIZE / 2) * 256 * 4 <= 0x7fffffffull,
              "PF_MAX_BATCH: every per-head activation must stay below 2 GiB (32-bit byte offsets, OOB marker 2^31)");
const int MIT_DIMS[4] = {64, 128, 320, 512};
const int MIT_HEADS[4] = {1, 2, 5, 8};
const int MIT_DEPTHS[4] = {3, 4, 18, 3};
const int MIT_SR[4] = {8, 4, 2, 1};
const int MIT_PK[4] = {7, 3, 3, 3}, MIT_PS[4] = {4, 2, 2, 2}, MIT_PP[4] = {3, 1, 1, 1};
constexpr int DEC_EMBED = 768, DEC_FEAT = 256, LL_CH = 64;
const int CNX_DEPTHS[4] = {3, 3, 9, 3};
const int CNX_DIMS[4] = {96, 192, 384, 768};

struct HostTensor {
  std::vector<float> data;
  std::vector<int64_t> shape;
  bool used = false;
};

struct ConvW {
  float* w = nullptr;
  float* b = nullptr;
  float* btab = nullptr;  // [9][Cout] border-case biases of a folded Linear->3x3 pair
  unsigned short* wsb = nullptr;  // weights split exactly into 3 bf16 planes (split-bf16 kernel), when Cin % 32 == 0
  unsigned short* wh16 = nullptr; // split-f16 scheme: per-channel power-of-two scaled weights as two fp16 planes wh, wl
  float* wh16_inv = nullptr;      //   and the inverse scale per output channel
  unsigned short* wwino = nullptr; // Winograd F(2x2, 3x3) form of a 3x3 / stride-1 conv (wino.hip): transformed weights in fragment order
  float* wwino_inv = nullptr;      //   and their inverse scale per output channel
  float* ln_s = nullptr;          // fused input LayerNorm (ConvParams::ln): column sums of the gamma-folded weights; nullptr = no fusion
  float ln_eps = 0.f;
  float sat_limit = 65504.f;      // window of the tensor this layer WRITES, set by its consumer (ConvParams::sat_limit): Winograd conv 65504 / 4, attention q / kv 8188 / 4094,
                                  // a depthwise conv behind it: (65504 - max |bias|) / max_c sum_k |w[k][c]|
  int Cout = 0, Cin = 0 /*padded*/, CinReal = 0, KH = 1, KW = 1, stride = 1, pad = 0, KWC = 0, KWCp = 0;
};
struct LNW { float* g = nullptr; float* b = nullptr; int C = 0; float eps = 1e-6f; };
struct DwW { float* w = nullptr; float* b = nullptr; int C = 0; float in_limit = 65504.f; /* its INPUT may reach this much and the output still fits 65504 */ };

// a linear layer in the row-block form (rb_gemm.hip): weight stream + inverse scales + bias
struct RbLin { unsigned short* w = nullptr; size_t bytes = 0; float* inv = nullptr; float* b = nullptr; int N = 0, K = 0; float sat_limit = 65504.f; };
// the key / value branch of a stage-3 block as one launch (rb_chain.hip): combined weight stream (conv as GEMM, then kv) + the two layers' scales / biases
struct RbSrKv { unsigned short* w = nullptr; size_t bytes = 0; float *sr_inv = nullptr, *sr_b = nullptr, *kv_inv = nullptr, *kv_b = nullptr; };
struct RbProjFc1 { unsigned short* w = nullptr; size_t bytes = 0; };  // combined weight stream of rb_proj_fc1_kernel (scales / biases: rproj, rfc1)
struct MitBlock { LNW n1, n2, srn; RbLin rq, rkv, rproj, rfc1, rfc2; RbSrKv rsrkv; RbProjFc1 rpf; ConvW qln /*q with norm1 folded (used next to rsrkv: no LayerNorm-1 launch)*/; ConvW q, kv, proj, sr, fc1, fc2; DwW dw; unsigned short* mlp_w = nullptr; float* mlp_tab = nullptr; /* fused Mlp (mit_mlp.hip), when built */
                  unsigned short* a64_w = nullptr; float* a64_tab = nullptr; /* fused attention half of a one-head, 64-channel block (attn_block.hip), when built */
                  unsigned short* tq_w = nullptr; float* tq_tab = nullptr; unsigned short* tp_w = nullptr; float* tp_tab = nullptr; /* 128 -> 128 q / proj in the thin form (thin_linear.hip), when built */ };
struct MitStage { ConvW pe; LNW pen, norm; std::vector<MitBlock> blocks; };
struct Head {
  ConvW lin[4], proc[4], fold[4], r1c1[4], r1c2[4], r2c1[4], r2c2[4], conv0, conv1, predcls;
  float* predw = nullptr; float* predb = nullptr; int nout = 0;
};
struct CnxBlock { float out_limit = 65504.f; /* window of the residual stream this block writes: the next block's depthwise conv */ DwW dw; LNW n; ConvW pw1, pw2; unsigned short* mlp_w = nullptr; float* mlp_tab = nullptr; /* fused MLP (cnx_mlp.hip), when built */
                  unsigned short* rb_w = nullptr; size_t rb_w_bytes = 0; float* rb_tab = nullptr; /* row-block fused MLP (cnx_rb.hip: C = 384 / 768), when built */ };
struct Cnx { ConvW stem, ds[3]; LNW stemn, dsn[3], norm; std::vector<CnxBlock> blocks[4]; float* headw = nullptr; float* headb = nullptr; int nout = 0; };

// Split-bf16 activation tensor (sb_split.h): three exact bf16 planes `plane` elements apart.
struct SbT {
  unsigned short* p = nullptr;
  size_t plane = 0;
};
// An activation as the kernels see it: fp32 NHWC and / or split planes (producers write what their consumers read).
struct Ten {
  float* f = nullptr;
  SbT s;
  Ten() {}
  Ten(float* f_) : f(f_) {}
  Ten(float* f_, SbT s_) : f(f_), s(s_) {}
};

struct Profiler;
// Debug forward (pf_debug_forward_u8): SHADOW taps -- named stage / block boundary tensors copied out for a layer-by-layer comparison with the oracle -- and RANGE
// records -- max |x|, sum x^2, saturated (|x| > 65504) and non-finite counts of every tensor that enters a dense contraction (the split-f16 scheme's window, sb_split.h).
struct DebugSink {
  bool shadow = false, range = false;
  char* buf = nullptr; size_t cap = 0, used = 0; bool overflow = false;  // shadow: caller's device buffer
  struct Tap { std::string name; size_t off; int shape[4]; };          // NHWC
  std::vector<Tap> taps;
  float* stats = nullptr; int max_ranges = 0;                          // range: device [max_ranges][4], zeroed before the forward
  struct Rng { std::string name; long long elems; };
  std::vector<Rng> ranges;
  int seq = 0;  // running number of dense launches
};

struct Ctx {
  hipStream_t s;
  uintptr_t base;
  size_t off = 0, peak = 0;
  bool dry;
  Profiler* prof = nullptr;
  DebugSink* dbg = nullptr;
  bool tuning = false;      // autotune pass: time every tile config per conv shape
  float* tune_scratch = nullptr;  // [max_conv_out] floats, followed by 3 bf16 planes of max_conv_out elements
  size_t tune_scratch_elems = 0;
  size_t max_conv_out = 0;  // elements of the largest (grouped) conv output seen by the dry run = tuning scratch size
  size_t nalloc = 0;        // alloc() calls so far: a fork window (pf_engine::fork_open) compares it at the fork and at the join
  int64_t* rep = nullptr;   // the engine's dispatch report (PF_DISPATCH_*: host counters of the real forward; nullptr in dry runs and probes)
  void count(int col, int64_t n = 1) { if (rep) rep[col] += n; }
  float* alloc(size_t nfloats) {
    const size_t bytes = (nfloats * 4 + 255) & ~(size_t)255;
    const size_t o = off;
    ++nalloc;
    off += bytes;
    if (off > peak) peak = off;
    return reinterpret_cast<float*>(base + o);
  }
  int sb_planes = 3;        // planes per split tensor: 3 (exact bf16 split) or 2 (split-f16 scheme; SbT::plane then carries SB_FMT_F16)
  SbT alloc_sb(size_t elems) {
    SbT t;
    const size_t stride = (elems + 127) & ~(size_t)127;
    count(PF_DISPATCH_SB_TENSORS);
    t.p = reinterpret_cast<unsigned short*>(alloc((sb_planes * stride * 2 + 3) / 4));
    t.plane = stride | (sb_planes == 2 ? SB_FMT_F16 : 0);
    return t;
  }
  // fp32 and / or split planes, as requested
  Ten ten(size_t elems, bool want_f32, bool want_sb) {
    Ten t;
    if (want_f32) t.f = alloc(elems);
    if (want_sb) t.s = alloc_sb(elems);
    return t;
  }
  size_t mark() const { return off; }
  void release(size_t m) { off = m; }
};

// Per-kernel-class timing with HIP events on the launch stream (bench.py's `roofline` object):
// every launch of a class is bracketed by an event pair; work = algorithmic FLOPs or bytes.
enum ProfCat { PC_IGEMM = 0, PC_ATTN, PC_LAYERNORM, PC_DW3, PC_DW7, PC_UPSAMPLE, PC_OTHER, PC_IGEMM_SB, PC_COUNT };
enum { PH_BACKBONE = 0, PH_LL = 1, PH_DECODERS = 2, PH_PARAMNET = 3, PH_POST = 4, PH_END = 5 };  // = PF_PHASE_* (include/pf_hip.h)
struct Profiler {
  struct Rec { int cat; double work; hipEvent_t a, b; int m, n, k, kh; float ms; };
  std::vector<Rec> recs;
  std::vector<hipEvent_t> pool;
  size_t used = 0;
  bool on = false;
  unsigned mask = 0xffffffffu;
  double min_work = 0.0;  // > 0: only launches with at least this much algorithmic work are bracketed (class-mask bit 31: the few large launches of a step --
                          // a dozen event records per step cost nothing, so EVERY timed step of bench.py can carry them, with the side stream left on)
  hipEvent_t get() {
    if (used == pool.size()) { hipEvent_t e; if (hipEventCreate(&e) != hipSuccess) return nullptr; pool.push_back(e); }
    return pool[used++];
  }
  // Phase marks of a FULL per-launch profile (one stream, no deferred branch): an event at the start of every component of the path (pf_profile_phases:
  // SURVEY 8d's component split).  A mark ends the phase before it; PH_END closes a phase without opening one.
  struct Mark { int phase; hipEvent_t e; };
  std::vector<Mark> marks;
  void mark(int phase, hipStream_t s) {
    if (!on || min_work > 0.0) return;
    hipEvent_t e = get();
    if (!e) return;
    (void)hipEventRecord(e, s);
    marks.push_back({phase, e});
  }
  void reset() { recs.clear(); marks.clear(); used = 0; }
  ~Profiler() { for (hipEvent_t e : pool) (void)hipEventDestroy(e); }
};
struct ProfScope {
  Profiler* p; hipStream_t s; hipEvent_t b = nullptr;
  ProfScope(Profiler* pr, hipStream_t st, int cat, double work, int m = 0, int n = 0, int k = 0, int kh = 0) : p(pr), s(st) {
    if (!p || !p->on || !((p->mask >> cat) & 1u) || work < p->min_work) { p = nullptr; return; }
    hipEvent_t a = p->get(); b = p->get();
    if (!a || !b) { p = nullptr; return; }
    (void)hipEventRecord(a, s);
    p->recs.push_back({cat, work, a, b, m, n, k, kh, 0.f});
  }
  ~ProfScope() { if (p) (void)hipEventRecord(b, s); }
};

struct ResizeTable { int ksize = 0; std::vector<int> bounds, kk; int *d_bounds = nullptr, *d_kk = nullptr; };

}  // namespace pf_host
using namespace pf;
using namespace pf_host;

struct pf_engine {
  int device = 0;
  int arch = 0;
  bool finalized = false;
  std::string err;
  std::unordered_map<std::string, HostTensor> host;
  std::vector<void*> dev_allocs;
  std::map<int, size_t> ws_cache;
  Profiler prof;
  bool autotune = false;     // PF_AUTOTUNE=1: the first forward of every new batch size times all tile configs per conv shape (a 1-2 s stall).
                             // Default off: tiles come from the shipped table (pf_load_tile_table, tuned/gfx950_tiles.txt) or the static
                             // heuristic -- deterministic, no first-call latency cliff; pf_autotune stays available as an explicit call
  std::map<std::vector<int>, int> tile_cache;  // conv shape (+batch) -> fastest tile config, measured on this device
  std::map<int, bool> tuned_batches;
  std::map<int, ResizeTable> resize_tables;  // input extent -> tables for resizing that extent to NET
  std::map<int, size_t> scratch_off, scratch_elems;
  bool split_bf16 = true;    // PF_SPLIT_BF16=0: exact-fp32 MFMA kernels only (no split-bf16 tiles)
  bool fuse_pred = true;     // PF_FUSE_PRED=0: keep the 32-channel 320x320 maps and run the regression prediction heads as their own kernel
  bool fuse_upsample = true; // PF_FUSE_UPSAMPLE=0: materialise the two largest bilinear x2 maps (160^2 x 256, 320^2 x 64 per head) instead of
                             // interpolating them inside the consuming 3x3 convs' halo staging (split-f16 scheme only)
  bool fuse_ln = true;       // PF_FUSE_LN=0: run every LayerNorm as its own kernel.  Default: a LayerNorm whose only consumers are 1x1 layers (MiT norm2 -> fc1,
                             // sr norm -> kv, stage-4 norm1 -> q / kv; ConvNeXt norm -> pwconv1) is folded into them (ConvParams::ln): gamma / beta go into the
                             // weights / bias at finalize, the row statistics are accumulated by the GEMM's own staging threads
  int thin128 = 25600;       // PF_THIN128 (0 = off, n = from n token rows up; 64 KB of weights per block is a prologue that 1 600 rows -- one image -- do not repay: B = 1 -1 %, B >= 16 +0.2 %): the 128 -> 128 q / output projections of the MiT stage-2 blocks in the transposed, register-epilogue form (thin_linear.hip)
  int stem7 = 1;             // PF_STEM7: the two 7 x 7 convs on the normalised image (low-level encoder; first patch embedding + its LayerNorm) as the specialised kernel of stem7.hip
  unsigned short* ll_s7_w = nullptr; float* ll_s7_tab = nullptr; unsigned short* pe_s7_w = nullptr; float* pe_s7_tab = nullptr;
  int attn64 = 1;            // PF_ATTN64: the attention half of the one-head stage-1 blocks (q, attention, proj, residual) as one kernel (attn_block.hip)
  int s3_split = 1;          // PF_S3_SPLIT: MiT stage 3 on two half-batches / two streams (mit(), "the stage-3 split")
  int dec_early = 2;         // PF_DEC_EARLY: the decoders' launches that need nothing of MiT stage 4 are issued on a side stream right after the stage-3 norm, beside stage 4 and
                             // decoder levels 3 / 2 (dec_early_issue(), "the early decoder start"): 1 the folded first convs fold[0..2], 2 also r1c1[0..2]; 0 = forward order
  int dec_early_stream = 2;  // PF_DEC_EARLY_STREAM: 2 = on `side2` (stage 4 keeps its q-beside-kv fork on `side`), 1 = on `side` (stage 4 runs unforked while the window is open)
  int dec_early_min_batch = 4;  // PF_DEC_EARLY_MIN_BATCH: as for the q fork -- below it every launch is a fraction of a round and a second stream only adds event traffic
  int dec_early_joined_max = 8;  // PF_DEC_EARLY_JOINED_MAX: largest batch that takes the path in a JOINED forward (pf_set_defer_params off, graph capture)
  bool dry_early = false;    // workspace_bytes: which of the two layouts (hoisted decoder tensors or not) the dry run walks
  int side_stream_mode = 1;  // 1 (default): the q projection of a MiT block runs on a second stream next to the sr conv + kv GEMM (both consume LayerNorm-1's
                             // output, attention joins them) -- small launches that each fill a fraction of the chip: +0.6 % (3 x A/B on one box, profiles/
                             // r02_negative_results.md); 2: also the low-level encoder conv next to MiT stage 3 (+0.1 %, noise); PF_SIDE_STREAM=0: one stream.
                             // Never forked while tuning or profiling (per-launch events time one stream)
  hipStream_t side = nullptr, side2 = nullptr;   // side: the q projections; side2: the low-level encoder conv, launched next to MiT stage 3
  hipEvent_t ev_fork = nullptr, ev_join = nullptr, ev_ll = nullptr;
  hipEvent_t ev_de_fork = nullptr, ev_de[3] = {nullptr, nullptr, nullptr};   // the early decoder start: c3 is written / level k's hoisted launches are done
  // Deferred ParamNet (pf_set_defer_params): the ConvNeXt branch of forward i runs on an internal stream behind the decoders of forward i and is NOT joined at the
  // end of the call -- forward i + 1's backbone (other images: no dependency) runs next to it.  Both are chains of small, latency-bound launches that leave most of
  // the chip idle (MiT stage 3: 13 % MFMA-busy; ConvNeXt stages 3-4 likewise), and their kernels co-reside (small LDS, 4 waves).  d_params of forward i is valid in
  // the caller's stream order once the NEXT pf_forward* has been issued on that stream (it waits for the branch before its decoders overwrite the branch's input),
  // or after pf_join_params.  The branch works in its own workspace region (input map + activations), behind the main one.
  bool host_only = false;    // pf_create(.., PF_DEVICE_NONE, ..): the host side only (weight repack / folds / splits, workspace dry run, tile table) with the "device" copies of the
                             // weights in host memory -- the sanitizer build's test seam; every entry point that would touch a GPU fails with PF_ERR_DEVICE
  int defer_params = 0;
  hipStream_t pstream = nullptr;
  hipEvent_t ev_pn_in = nullptr, ev_pn_done = nullptr;
  bool pn_pending = false, in_capture = false;
  int pn_pending_B = 0; uintptr_t pn_pending_base = 0;   // batch and workspace of the pending branch: another batch size lays the regions out differently
  // PF_DEFER_AT = k > 0: the deferred branch of forward i is ISSUED (on pstream) only when forward i + 1 reaches MiT stage k -- next to the stage whose launches leave
  // the most room -- instead of right away (k = 0); pf_join_params / the decoders' wait issue it if no forward came
  int defer_at = 0, defer_prio = 0;
  struct PnLater { bool armed = false; int B = 0; const float* pn = nullptr; float* params = nullptr; Ctx ctx; } pn_later;
  void issue_deferred() {
    if (!pn_later.armed) return;
    pn_later.armed = false;
    paramnet(pn_later.ctx, pn_later.B, pn_later.pn, pn_later.params);
    (void)hipEventRecord(ev_pn_done, pstream);
  }
  std::map<int, size_t> pn_off;   // batch -> byte offset of the ParamNet region in the workspace
  // the pending branch is issued if it is still armed, and `s` waits for it: what comes next on `s` overwrites its input map or its region
  void join_deferred(hipStream_t s) { issue_deferred(); (void)hipStreamWaitEvent(s, ev_pn_done, 0); pn_pending = false; }
  bool pstream_ready();
  bool ll_forked = false;
  // Streams are a scarce resource: the runtime multiplexes a process's streams onto a few hardware queues (4 by default), and two streams that share a queue do not
  // overlap -- the engine therefore creates only the streams its mode needs (side2 only for PF_SIDE_STREAM=2); with the null stream, `side` and the ParamNet stream
  // a forward uses three queues (profiles/r04_defer_params.md: with nine streams in one process the deferred branch lost its whole gain).
  bool side_ready();
  // A FORK WINDOW runs from a `Ctx c2 = c` -- a COPY of the bump allocator that issues launches on a side stream -- to the join of that stream.  Both contexts
  // continue from ONE offset, so the window is sound only while at most one of them allocates (the normal case: the parent's split-K partial for the sr conv while q
  // runs on the side stream).  Both allocating would hand two streams the same scratch: counted, timing-free, in PF_DISPATCH_FORK_ALLOC_CONFLICTS -- 0 after every forward.
  struct ForkWin { bool open = false, side_alloced = false; size_t nalloc0 = 0; };
  ForkWin fw_q, fw_ll;   // q beside kv / the stage-3 split (never nested in each other); the low-level encoder beside stages 3 / 4
  ForkWin fw_de;         // the early decoder start: open from the stage-3 norm to decoder level 0 (stage 4's q windows open and close inside it)
  // The early decoder start's state of one forward: the hoisted tensors of levels 0-2 (p: fold[k]'s outputs; t: r1c1[k]'s, mode 2), allocated in front of stage 4
  struct DecEarly { bool layout = false, issued = false; Ten p[3][2], t[3][2]; } de;
  Ctx fork_open(Ctx& c, hipStream_t s, ForkWin& w) {
    Ctx c2 = c;
    c2.s = s;
    w.open = true; w.side_alloced = false; w.nalloc0 = c.nalloc;
    c.count(PF_DISPATCH_FORKS);
    return c2;
  }
  void fork_side_done(ForkWin& w, const Ctx& c2) { w.side_alloced = c2.nalloc > w.nalloc0; }  // the side stream's launches are issued
  void fork_join(Ctx& c, ForkWin& w) {
    if (!w.open) return;
    if (w.side_alloced && c.nalloc > w.nalloc0) c.count(PF_DISPATCH_FORK_ALLOC_CONFLICTS);
    w.open = false;
  }
  // THE window, stated once: `body` runs beside the caller's stream.  fork = false: body(c), on the caller's stream, and nothing else.  fork = true: `ev_in` is
  // recorded on c.s and `side_s` waits for it, the window `w` opens, body(c2) issues on `side_s` through the window's copy of the allocator, `ev_out` is recorded
  // on `side_s` and the window notes whether the body allocated.  The caller owns the other half, where ITS next launch needs the body's result: a
  // hipStreamWaitEvent(c.s, ev_out) and fork_join(c, w).  Returns `fork`, so that the join asks "did this fork" instead of evaluating the fork's condition again.
  template <class Body>
  bool beside(Ctx& c, bool fork, hipStream_t side_s, hipEvent_t ev_in, hipEvent_t ev_out, ForkWin& w, Body body) {
    if (!fork) { body(c); return false; }
    (void)hipEventRecord(ev_in, c.s);
    (void)hipStreamWaitEvent(side_s, ev_in, 0);
    Ctx c2 = fork_open(c, side_s, w);
    body(c2);
    (void)hipEventRecord(ev_out, side_s);
    fork_side_done(w, c2);
    return true;
  }
  int64_t dispatch[PF_DISPATCH_COLS] = {};  // pf_last_dispatch: what the last forward launched
  int splitk_mode = -1;      // PF_SPLITK: 0 = no split-K, N > 1 forces the factor (conv_splitk_shape); read per engine, so that a process can hold engines of both kinds
  int wino_half = 1;         // PF_WINO_HALF=0: square Winograd patches always (ConvParams::wino_half)
  bool can_fork(const Ctx& c) { return side_stream_mode && !c.dry && !c.tuning && (!c.prof || c.prof->min_work > 0.0) && side_ready(); }  // (a full per-launch profile keeps one stream: its event pairs must bracket what they name)
  bool sba_heads = false;    // PF_SBA_HEADS=1: the tensors between the 3x3 convs of the decoders' ResidualConvUnits are written as split-f16 planes by the producing
                             // conv's epilogue (plus fp32 where a residual add reads them) and the halo kernel copies them (igemm_sbh ASB) instead of splitting
                             // every element once per n-tile and halo overlap; split-f16 scheme only
  int rb_chain = 60;         // PF_RB_CHAIN: which linear layers of MiT stage 3 run in the row-block form (rb_gemm.hip) instead of the LDS tiles (igemm_sb) once the batch gives
                             // at least rb_min_blocks row blocks: bit mask 1 q, 2 kv, 4 proj, 8 fc1, 16 fc2, 32 the whole key / value branch as one launch (rb_chain.hip; overrides 2), 64 proj + norm2 + fc1 as one launch (overrides 4, 8) (0 = none)
  int rb_min_blocks = 192;   // default for 256 CUs; pf_create rescales it to 3/4 of the device's CU count
  int num_cus = 256;         // hipDeviceProp_t::multiProcessorCount (partitioned / smaller gfx950 configurations: CPX / DPX modes)
  int wino_min_hw = 20;      // PF_WINO=<n>: 3x3 / stride-1 convs with Cin, Cout multiples of 64 on maps of at least n x n run as Winograd F(2x2, 3x3) (wino.hip; split-f16
                             // scheme only; 0 = never).  Their inputs' window ends at 65504 / 4 (the input transform adds four values).  r06: 20 instead of 40 -- with the
                             // half-patch geometry the 20 x 20 RCU convs run 1.45x faster than on the direct tile (profiles/r06_wino_gate.txt; r05's square patches: equal)
  int wino_min_blocks = 96;  // PF_WINO_MIN_BLOCKS: ... and only launches of at least this many blocks (one block per CU, 512 registers per wave: at batch 1 the 40 x 40 maps
                             // give 64 blocks and the direct tile, with more and smaller blocks, is 18 % faster there)
  int wino_tile = -1;        // tile id of the Winograd kernel in use
  unsigned* d_sat = nullptr; // pf_set_saturation_counter: caller-owned device counter of the always-on saturation watch (ConvParams::sat); nullptr = off
  float static_window_max = 0.f;  // largest STATIC bound of a tensor that never reaches HBM (the hidden maps of the fused block MLPs), pf_static_window_max
  int mit_mlp128 = 4;        // PF_MIT_MLP_128 (0 = never, n = from a batch of n images up): the one-kernel Mlp at MiT stage 2 (mit_mlp.hip, C = 128; 25 blocks per image: B = 1 -1.1 %, 2 -0.4 %, 4 +0.7 %, 8 +1.1 %, 32 +0.6 %)
  bool fuse_mit_mlp = true;  // PF_FUSE_MIT_MLP=0: the Mlp of MiT stages 1 / 2 as LayerNorm-fused fc1 + depthwise 3x3 / GELU + fc2 instead of the one-kernel form
                             // (mit_mlp.hip: hidden map in LDS / registers only); split-f16 scheme only
  bool fuse_cnx_mlp = true;  // PF_FUSE_CNX_MLP=0: ConvNeXt blocks of the 96- and 192-channel stages as LayerNorm-fused pwconv1 + pwconv2 GEMMs instead of
                             // the one-kernel MLP (cnx_mlp.hip, hidden map in registers only); split-f16 scheme only
  int cnx_rb = 1;            // PF_CNX_RB: ConvNeXt blocks of the 384- / 768-channel stages as ONE row-block kernel (cnx_rb.hip: rows resident in LDS, hidden map never in HBM)
                             // instead of LayerNorm-fused pwconv1 + pwconv2 on the generic tile.  Low two bits: 0 = GEMM pair, 1 = where the batch gives the stage at least
                             // cnx_rb_min_blocks[stage] row blocks, 2 = whenever supported (tests); + 4 = stage 3 (C = 384) only.  Split-f16 scheme only, not with PF_SBA
  int cnx_rb_min_blocks[2] = {96, 192};  // PF_CNX_RB_MIN_BLOCKS / PF_CNX_RB_MIN_BLOCKS_768: one block per CU and one block's latency per launch (90 / 210 us however few blocks
                             // there are), so the GEMM pair wins below a batch.  Defaults 3/8 and 3/4 of the device's CU count: C = 384 (64-row blocks, 6.25 per image) from
                             // B = 16, C = 768 (32-row blocks, 3.125 per image) from B = 62.  Alone, 50 blocks take 90 us against 69 us for the pair and a joined forward of
                             // B = 8 is 0.42 ms slower with them, B = 12 0.17 ms; at 100 blocks it is 94 against 105 us and B = 16 is level (profiles/r07_cnx_rb.md)
  bool fold_mlp = true;      // PF_FOLD_MLP=0 keeps Linear(C->768) and conv3x3(768->256) as two kernels
  int nterms = NT_F16X3;     // pf_set_precision: NT_F16X3 = 2-way fp16 split, 3 MFMAs per product (default parity mode); 6 = exact 3-way bf16 split
                             // (fp32-accurate, PF_PRECISION_FP32_BF16X6); 3 = "bf16x3", 1 = "bf16" (reduced precision, not parity modes)
  DebugSink dbg;  // records of the last pf_debug_forward_u8
  DebugSink* debug_sink = nullptr;  // non-null while pf_debug_forward_u8 runs
  // hipGraph replay of small-batch forwards (pf_forward_u8_graph): one graph per (batch, buffer set, precision)
  struct GraphEntry { std::vector<uintptr_t> key; hipGraphExec_t exec; };
  std::vector<GraphEntry> graphs;
  bool sba = false;          // PF_SBA=1: tensors that only feed GEMMs are stored as split-bf16 planes by their producers (sb_split.h);
                             // measured slower end to end (1.5x the bytes on HBM-bound layers), kept as an option -- DESIGN.md 4.2

  MitStage stages[4];
  ConvW ll;
  Head heads[2];  // 0 gravity, 1 latitude
  Cnx cnx;
  bool has_param = false;
  int param_in = NET;  // ParamNet input resolution
  float mean3[3] = {103.53f, 116.28f, 123.675f};
  float std3[3] = {1.f, 1.f, 1.f};

  int fail(int code, const std::string& m) { err = m; return code; }
  size_t run_pn_peak = 0;
  std::map<int, size_t> pn_peak;  // batch -> bytes of the ParamNet region as the dry run sized it
  struct ConvCall {  // one problem of a (possibly grouped) conv launch
    const ConvW* w; Ten x; Ten y;
    const float* res1 = nullptr; const float* res2 = nullptr; Ten x2 = Ten();
    // fused regression prediction head (ConvPtrs::head_*): kind 1 gravity, 2 latitude
    int head_kind = 0; const float* head_w = nullptr; const float* head_b = nullptr; float* head_out = nullptr; float* head_pn = nullptr;
  };

  // ------------------------------------------------------------------ weights (engine_weights.hip)
  ResizeTable* resize_table(int in_size);
  float* upload(const std::vector<float>& v);
  unsigned short* upload_u16(const std::vector<unsigned short>& v);
  void upload_conv_weights(ConvW& c, const std::vector<float>& packed, int CinP, int Cout);
  const HostTensor& get(const std::string& key, std::initializer_list<int64_t> shape);
  ConvW make_conv(const std::string& wkey, const std::string& bkey, int Cout, int Cin, int K, int stride, int pad, const double* out_scale = nullptr, const std::vector<float>* bias_override = nullptr);
  ConvW make_linear(const std::string& pfx, int N, int K, const double* out_scale = nullptr, const std::string& ln_pfx = "", float ln_eps = 0.f);
  ConvW make_folded(const std::string& lin, const std::string& proc, int C);
  LNW make_ln(const std::string& pfx, int C, float eps);
  void note_static(double bound, float limit);
  double ln_bound(const std::string& pfx, int C);
  double mlp_hidden_bound(const std::string& ln, const std::string& fc1, const std::string& dw, int C);
  DwW make_dw(const std::string& pfx, int C, int K);
  RbLin make_rb(const std::string& pfx, int N, int K, int cols);
  void build_head(Head& hd, const std::string& name, int nout, bool cls);
  void build();
  // ------------------------------------------------------------------ debug taps, layer helpers, the walk, workspace sizing (engine_forward.hip)
  void tap(Ctx& c, const std::string& name, const float* p, int B, int H, int W, int C);
  void range_in(Ctx& c, const std::string& name, const float* p, size_t elems);
  void conv_g(Ctx& c, int ngroups, const ConvCall* calls, int B, int H, int W, int act = ACT_NONE, int post_relu = 0, int C1 = -1, int nchw = 0, int ups = 0);
  int tune_conv(const ConvParams& p0, Ctx& c);
  void conv(Ctx& c, const ConvW& w, Ten x, int B, int H, int W, Ten y, int act = ACT_NONE, const float* res1 = nullptr, const float* res2 = nullptr, int post_relu = 0, Ten x2 = Ten(), int C1 = -1, int nchw = 0);
  void gemm(Ctx& c, const ConvW& w, Ten x, long rows, Ten y, int act = ACT_NONE, const float* res1 = nullptr);
  void ln(Ctx& c, const LNW& l, const float* x, Ten y, long rows);
  void rb_linear(Ctx& c, const RbLin& r, const float* x, long M, int tokens, float* y, const LNW* lnw = nullptr, int act = ACT_NONE, const float* res = nullptr);
  void thin(Ctx& c, const unsigned short* wfr, const float* tab, const float* x, const float* res, float* y, long M, float sat_limit, const char* what);
  void stem(Ctx& c, const unsigned short* wfr, const float* tab, const float* x4, float* y, int B, int H, int W, int stride, bool relu, bool lnorm, float eps, float sat_limit, const char* what);
  // The MiT walk.  StageDims: one stage's shape -- C channels, heads_n heads, an Ho x Wo map of N tokens per image, keys / values on the kvh x kvw map the spatial
  // reduction sr leaves; fused_mlp: the stage's blocks take the one-kernel Mlp (mit_mlp.hip), which writes a second buffer
  struct StageDims { int s, C, heads_n, sr, Ho, Wo; long N; int kvh, kvw; bool fused_mlp; };
  // The buffers one transformer block works in, from the token row of its first image
  struct BlockBufs {
    float *x = nullptr, *xalt = nullptr;  // token stream, updated in place by the residual epilogues; the fused Mlp's target (the two swap roles after every block)
    Ten xn; float* qb = nullptr; Ten ab;  // LayerNorm output, q, attention output
    float* srb = nullptr; Ten srn; float* kvb = nullptr;  // spatial-reduction conv, its LayerNorm (in place, or planes only), kv
    float* hb = nullptr; Ten h2;          // the Mlp's hidden map before / behind the depthwise conv
    // The view of the second half-batch (the stage-3 split), Mh token rows and Mkvh key / value rows further on.  fp32 only: the split never runs with split
    // planes or the fused Mlp, so planes are not carried and xalt stays null
    BlockBufs second_half(long Mh, long Mkvh, int C) const {
      BlockBufs h;
      h.x = x + Mh * C; h.xn = Ten(xn.f ? xn.f + Mh * C : nullptr); h.qb = qb + Mh * C; h.ab = Ten(ab.f + Mh * C);
      h.srb = srb + Mkvh * C; h.srn = Ten(srn.f ? srn.f + Mkvh * C : nullptr); h.kvb = kvb + Mkvh * 2 * C;
      h.hb = hb + Mh * 4 * C; h.h2 = Ten(h2.f + Mh * 4 * C);
      return h;
    }
  };
  struct BlockForm { bool thin_q, fuse64, use_rb, pf_fused; };  // which forms of its layers a block takes (mit_block)
  // one 64-row block per CU: the row-block form pays only when the last round of `nb` blocks nearly fills the CUs (mit_block)
  bool rb_gate(long nb) const { return nb >= rb_min_blocks && (nb % num_cus == 0 || nb % num_cus >= num_cus * 3 / 4); }
  void mit(Ctx& c, int B, const float* x0, Ten feats[4], const Ten* llf = nullptr);
  void mit_block(Ctx& c, MitBlock& mb, int blk, const StageDims& d, BlockBufs& b, int B, int gate_B, bool may_fork);
  bool block_attn_inputs(Ctx& c, MitBlock& mb, int blk, const StageDims& d, const BlockBufs& b, int B, const BlockForm& f, bool may_fork);
  void block_attn(Ctx& c, MitBlock& mb, int blk, const StageDims& d, const BlockBufs& b, int B, const BlockForm& f);
  void block_mlp(Ctx& c, MitBlock& mb, int blk, const StageDims& d, BlockBufs& b, int B, const BlockForm& f);
  bool pred_fused() const;
  static void dec_pair(Ctx& c, size_t per_head, bool want_f32, bool want_sb, Ten& a, Ten& b);
  bool dec_sr() const;
  void dec_fold(Ctx& c, int k, int B, Ten feats[4], const Ten& p0, const Ten& p1);
  void dec_r1c1(Ctx& c, int k, int B, const Ten& p0, const Ten& p1, const Ten& t0, const Ten& t1);
  void dec_early_issue(Ctx& c, int B, Ten feats[4]);
  void dec_early_wait(Ctx& c, int k);
  void heads_fwd(Ctx& c, int B, Ten feats[4], Ten llf, float* t32 /*[2][B][320][320][32], unused when the heads are fused*/, float* pg, float* pl, float* pn);
  void paramnet(Ctx& c, int B, const float* pn_in, float* d_params);
  void run(Ctx& c, int B, const void* in, bool is_u8, float* pg, float* pl, float* params);
  size_t workspace_bytes(int B, bool with_scratch = false);
  int forward(int B, const void* in, bool is_u8, float* pg, float* pl, float* params, void* ws, size_t ws_bytes, hipStream_t s, bool tune = false);
};
