// libpf_hip.so: the C ABI of the MI355X PerspectiveFields engine (include/pf_hip.h) -- pf_create and its switches, the graph, profile and debug entry points, the
// tile table, resize and post-processing.  The engine itself is declared in engine.h; its weight store is engine_weights.hip, its layer walk engine_forward.hip.
// Host-side C++ only *orchestrates* hand-written gfx950 kernels (igemm.hip, attn.hip, elem.hip); there is no CPU or library (MIOpen / hipBLASLt) fallback.
#include "engine.h"

namespace pf_host { thread_local std::string g_create_error; }

static void tune_cache_load(pf_engine* h);
static void tune_cache_save(pf_engine* h);

// =========================================================================== C ABI

extern "C" {

const char* pf_version(void) { return "pf_hip 0.2 (gfx950; split-f16 / split-bf16 / fp32 MFMA)"; }

#ifndef PF_BUILD_DIGEST
#define PF_BUILD_DIGEST "unknown"
#endif
// sha256 over csrc/ + include/ + flags at build time (perspectivefields_amd/build.py): lets the loader refuse a stale .so
const char* pf_build_digest(void) { return PF_BUILD_DIGEST; }

const char* pf_last_error(pf_handle h) { return h ? h->err.c_str() : g_create_error.c_str(); }

int pf_create(pf_handle* out, int device, int arch) {
  if (!out) { g_create_error = "pf_create: out is NULL"; return PF_ERR_ARG; }
  *out = nullptr;
  if (arch < 0 || arch > 2) { g_create_error = fmt("pf_create: unknown arch %d", arch); return PF_ERR_ARG; }
  const bool host_only = device == PF_DEVICE_NONE;
  if (!host_only) {
    const int rc = check_device(device, &g_create_error);
    if (rc != PF_OK) return rc;
  }
  pf_engine* e = new pf_engine();
  e->device = device;
  e->host_only = host_only;
  e->arch = arch;
  if (const char* v = getenv("PF_FOLD_MLP")) e->fold_mlp = atoi(v) != 0;
  if (const char* v = getenv("PF_FUSE_UPSAMPLE")) e->fuse_upsample = atoi(v) != 0;
  if (const char* v = getenv("PF_FUSE_PRED")) e->fuse_pred = atoi(v) != 0;
  if (const char* v = getenv("PF_FUSE_LN")) e->fuse_ln = atoi(v) != 0;
  if (const char* v = getenv("PF_FUSE_CNX_MLP")) e->fuse_cnx_mlp = atoi(v) != 0;
  if (const char* v = getenv("PF_FUSE_MIT_MLP")) e->fuse_mit_mlp = atoi(v) != 0;
  if (const char* v = getenv("PF_MIT_MLP_128")) e->mit_mlp128 = atoi(v);
  if (const char* v = getenv("PF_WINO")) e->wino_min_hw = atoi(v);
  if (const char* v = getenv("PF_WINO_MIN_BLOCKS")) e->wino_min_blocks = atoi(v);
  {
    const char* wt = getenv("PF_WINO_TILE");  // "wino256x64d" (default: 4 waves, B fragments computed in registers, hand-placed slots), or "wino256x64c" (its compiler-scheduled form)
    for (int t = 0; t < conv_num_tiles(); ++t) if (strcmp(conv_tile_name(t), wt ? wt : "wino256x64d") == 0) e->wino_tile = t;
  }
  if (const char* v = getenv("PF_RB_CHAIN")) e->rb_chain = atoi(v);
  if (const char* v = getenv("PF_DEFER_AT")) e->defer_at = atoi(v);
  if (const char* v = getenv("PF_DEFER_PRIO")) e->defer_prio = atoi(v);
  if (!host_only) {
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0) e->num_cus = prop.multiProcessorCount;
    e->rb_min_blocks = e->num_cus * 3 / 4;  // "the last round of blocks nearly fills the chip": 192 of 256 CUs
  }
  if (const char* v = getenv("PF_RB_MIN_BLOCKS")) e->rb_min_blocks = atoi(v);
  if (const char* v = getenv("PF_CNX_RB")) e->cnx_rb = atoi(v);
  if (!host_only) { e->cnx_rb_min_blocks[0] = e->num_cus * 3 / 8; e->cnx_rb_min_blocks[1] = e->num_cus * 3 / 4; }
  if (const char* v = getenv("PF_CNX_RB_MIN_BLOCKS")) e->cnx_rb_min_blocks[0] = atoi(v);
  if (const char* v = getenv("PF_CNX_RB_MIN_BLOCKS_768")) e->cnx_rb_min_blocks[1] = atoi(v);
  if (const char* v = getenv("PF_SIDE_STREAM")) e->side_stream_mode = atoi(v);
  if (const char* v = getenv("PF_S3_SPLIT")) e->s3_split = atoi(v);
  if (const char* v = getenv("PF_DEC_EARLY")) e->dec_early = atoi(v);
  if (const char* v = getenv("PF_DEC_EARLY_STREAM")) e->dec_early_stream = atoi(v) == 1 ? 1 : 2;
  if (const char* v = getenv("PF_DEC_EARLY_MIN_BATCH")) e->dec_early_min_batch = atoi(v);
  if (const char* v = getenv("PF_DEC_EARLY_JOINED_MAX")) e->dec_early_joined_max = atoi(v);
  if (const char* v = getenv("PF_ATTN64")) e->attn64 = atoi(v);
  if (const char* v = getenv("PF_STEM7")) e->stem7 = atoi(v);
  if (const char* v = getenv("PF_THIN128")) e->thin128 = atoi(v);
  if (const char* v = getenv("PF_SBA_HEADS")) e->sba_heads = atoi(v) != 0;
  if (const char* v = getenv("PF_AUTOTUNE")) e->autotune = atoi(v) != 0;
  if (const char* v = getenv("PF_SPLIT_BF16")) e->split_bf16 = atoi(v) != 0;
  if (const char* v = getenv("PF_SBA")) e->sba = atoi(v) != 0;
  e->splitk_mode = conv_splitk_env();
  e->wino_half = conv_wino_half_env();
  if (!e->split_bf16) e->sba = false;  // split planes are only read by the split-bf16 kernels
  if (!e->split_bf16 || e->sba) e->fuse_ln = false;  // the fused form lives in the split GEMM kernels and reads fp32 rows
  if (!e->split_bf16 || e->sba) e->fuse_cnx_mlp = false;
  if (!e->split_bf16 || e->sba) e->fuse_mit_mlp = false;
  if (!e->split_bf16 || e->sba) e->cnx_rb = 0;

  tune_cache_load(e);
  *out = e;
  return PF_OK;
}

int pf_set_precision(pf_handle h, int mode) {
  if (!h) return PF_ERR_ARG;
  if (mode != PF_PRECISION_FP32 && mode != PF_PRECISION_FP32_BF16X6) return h->fail(PF_ERR_ARG, "pf_set_precision: unknown mode (0 = FP32 split-f16, 3 = FP32_BF16X6; the reduced-precision modes 1 / 2 of earlier versions are gone)");
  if (mode != PF_PRECISION_FP32 && !h->split_bf16) return h->fail(PF_ERR_ARG, "pf_set_precision: this mode needs the split kernels (PF_SPLIT_BF16=0 is set)");
  if (h->pn_pending) { h->issue_deferred(); (void)hipStreamSynchronize(h->pstream); h->pn_pending = false; }  // a deferred ParamNet branch still works in the old layout
  h->ws_cache.clear();  // the split-plane activation format (2 fp16 / 3 bf16 planes) follows the scheme
  h->nterms = mode == PF_PRECISION_FP32_BF16X6 ? 6 : NT_F16X3;
  return PF_OK;
}

int pf_set_saturation_counter(pf_handle h, void* d_counter_u32) {
  if (!h) return PF_ERR_ARG;
  h->d_sat = static_cast<unsigned*>(d_counter_u32);
  return PF_OK;
}
int pf_static_window_max(pf_handle h, float* out) {
  if (!h || !out || !h->finalized) return PF_ERR_ARG;
  *out = h->static_window_max;
  return PF_OK;
}
int pf_set_defer_params(pf_handle h, int on) {
  if (!h) return PF_ERR_ARG;
  h->defer_params = on ? 1 : 0;
  return PF_OK;
}
int pf_join_params(pf_handle h, void* stream) {
  if (!h) return PF_ERR_ARG;
  if (h->pn_pending) h->issue_deferred();
  if (h->pn_pending && hipStreamWaitEvent(static_cast<hipStream_t>(stream), h->ev_pn_done, 0) != hipSuccess) return h->fail(PF_ERR_DEVICE, "pf_join_params: hipStreamWaitEvent failed");
  return PF_OK;
}

int pf_destroy(pf_handle h) {
  if (!h) return PF_ERR_ARG;
  if (h->host_only) {
    for (void* d : h->dev_allocs) free(d);
    delete h;
    return PF_OK;
  }
  (void)hipSetDevice(h->device);
  for (void* d : h->dev_allocs) (void)hipFree(d);
  if (h->dbg.stats) (void)hipFree(h->dbg.stats);
  for (auto& g : h->graphs) (void)hipGraphExecDestroy(g.exec);
  if (h->ev_fork) (void)hipEventDestroy(h->ev_fork);
  if (h->ev_join) (void)hipEventDestroy(h->ev_join);
  if (h->ev_ll) (void)hipEventDestroy(h->ev_ll);
  for (hipEvent_t e : {h->ev_de_fork, h->ev_de[0], h->ev_de[1], h->ev_de[2]}) if (e) (void)hipEventDestroy(e);
  if (h->side) (void)hipStreamDestroy(h->side);
  if (h->side2) (void)hipStreamDestroy(h->side2);
  if (h->pstream) { (void)hipStreamSynchronize(h->pstream); (void)hipStreamDestroy(h->pstream); }
  if (h->ev_pn_in) (void)hipEventDestroy(h->ev_pn_in);
  if (h->ev_pn_done) (void)hipEventDestroy(h->ev_pn_done);
  delete h;
  return PF_OK;
}

int pf_load_tensor(pf_handle h, const char* key, const float* data, const int64_t* shape, int rank) {
  if (!h || !key || (!data && rank > 0) || rank < 0 || rank > 4) return h ? h->fail(PF_ERR_ARG, "pf_load_tensor: bad argument") : PF_ERR_ARG;
  if (h->finalized) return h->fail(PF_ERR_WEIGHTS, "pf_load_tensor after pf_finalize_weights");
  HostTensor t;
  size_t n = 1;
  for (int i = 0; i < rank; ++i) { if (shape[i] <= 0) return h->fail(PF_ERR_ARG, "pf_load_tensor: non-positive dim"); t.shape.push_back(shape[i]); n *= (size_t)shape[i]; }
  if (data) t.data.assign(data, data + n);
  h->host[key] = std::move(t);
  return PF_OK;
}

int pf_finalize_weights(pf_handle h) {
  if (!h) return PF_ERR_ARG;
  if (h->finalized) return h->fail(PF_ERR_WEIGHTS, "weights already finalized");
  if (!h->host_only && hipSetDevice(h->device) != hipSuccess) return h->fail(PF_ERR_DEVICE, "hipSetDevice failed");
  try {
    h->build();
  } catch (const std::string& m) {
    return h->fail(PF_ERR_WEIGHTS, m);
  }
  h->finalized = true;
  return PF_OK;
}

int pf_output_info(pf_handle h, int* g, int* l, int* p) {
  if (!h) return PF_ERR_ARG;
  const bool cls = h->arch == PF_ARCH_PERSNET_CLS;
  if (g) *g = cls ? 73 : 2;
  if (l) *l = cls ? 180 : 1;
  if (p) *p = cls ? 0 : 5;
  return PF_OK;
}

int pf_max_batch(void) { return PF_MAX_BATCH; }

int pf_last_dispatch(pf_handle h, int64_t* out, int n) {
  if (!h || !out || n < PF_DISPATCH_COLS) return h ? h->fail(PF_ERR_ARG, "pf_last_dispatch: the array must hold PF_DISPATCH_COLS entries") : PF_ERR_ARG;
  std::copy(h->dispatch, h->dispatch + PF_DISPATCH_COLS, out);
  return PF_OK;
}

size_t pf_workspace_bytes(pf_handle h, int batch) {
  if (!h || batch <= 0 || batch > PF_MAX_BATCH) return 0;
  const bool was = h->has_param;
  if (!h->finalized) {  // architecture-only estimate is allowed before weights are loaded
    h->has_param = h->arch != PF_ARCH_PERSNET_CLS;
    h->param_in = h->arch == PF_ARCH_PARAMNET_UNCENTERED ? 64 : NET;
    for (int s = 0; s < 4; ++s)
      if (h->stages[s].blocks.empty()) h->stages[s].blocks.resize(MIT_DEPTHS[s]);
    if (h->has_param)
      for (int s = 0; s < 4; ++s)
        if (h->cnx.blocks[s].empty()) h->cnx.blocks[s].resize(CNX_DEPTHS[s]);
  }
  const size_t n = h->workspace_bytes(batch);
  if (!h->finalized) {
    h->has_param = was;
    for (int s = 0; s < 4; ++s) { h->stages[s].blocks.clear(); h->cnx.blocks[s].clear(); }
    h->ws_cache.clear();
  }
  return n;
}

int pf_forward_u8(pf_handle h, int batch, const uint8_t* in, float* pg, float* pl, float* params, void* ws, size_t ws_bytes, void* stream) {
  if (!h) return PF_ERR_ARG;
  return h->forward(batch, in, true, pg, pl, params, ws, ws_bytes, static_cast<hipStream_t>(stream));
}
// The forward of a small batch is ~430 launches of a few microseconds each: host launch cost, not GPU time, sets its
// latency.  Captured once per (batch, buffer set) into a hipGraph and replayed with a single launch.
int pf_forward_u8_graph(pf_handle h, int batch, const uint8_t* in, float* pg, float* pl, float* params, void* ws, size_t ws_bytes, void* stream) {
  if (!h) return PF_ERR_ARG;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (!s) return h->fail(PF_ERR_ARG, "pf_forward_u8_graph: needs an explicit (non-default) stream: the legacy default stream cannot be captured");
  if (h->prof.on || h->autotune) return h->forward(batch, in, true, pg, pl, params, ws, ws_bytes, s);  // event pairs / tuning launches are not capturable
  const std::vector<uintptr_t> key = {(uintptr_t)batch, (uintptr_t)in, (uintptr_t)pg, (uintptr_t)pl, (uintptr_t)params, (uintptr_t)ws, (uintptr_t)h->nterms};
  hipGraphExec_t exec = nullptr;
  for (auto& g : h->graphs) if (g.key == key) { exec = g.exec; break; }
  if (!exec) {
    if (hipSetDevice(h->device) != hipSuccess) return h->fail(PF_ERR_DEVICE, "hipSetDevice failed");
    (void)h->workspace_bytes(batch);  // dry run outside the capture
    if (h->pn_pending) h->join_deferred(s);  // a deferred ParamNet branch is joined outside the capture
    if (hipStreamBeginCapture(s, hipStreamCaptureModeRelaxed) != hipSuccess) return h->fail(PF_ERR_DEVICE, "hipStreamBeginCapture failed");
    h->in_capture = true;  // a captured forward keeps the branch on the capture stream
    const int rc = h->forward(batch, in, true, pg, pl, params, ws, ws_bytes, s);
    h->in_capture = false;
    hipGraph_t graph = nullptr;
    const hipError_t e = hipStreamEndCapture(s, &graph);
    if (rc != PF_OK) { if (graph) (void)hipGraphDestroy(graph); return rc; }
    if (e != hipSuccess || !graph) return h->fail(PF_ERR_DEVICE, fmt("hipStreamEndCapture failed: %s", hipGetErrorString(e)));
    const hipError_t e2 = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
    (void)hipGraphDestroy(graph);
    if (e2 != hipSuccess) return h->fail(PF_ERR_DEVICE, fmt("hipGraphInstantiate failed: %s", hipGetErrorString(e2)));
    if (h->graphs.size() >= 16) { (void)hipGraphExecDestroy(h->graphs.front().exec); h->graphs.erase(h->graphs.begin()); }
    h->graphs.push_back({key, exec});
  }
  // a replay, too, overwrites the ParamNet input map (or, with another batch size, the region) a pending deferred branch is still working in
  if (h->pn_pending) h->join_deferred(s);
  if (hipGraphLaunch(exec, s) != hipSuccess) return h->fail(PF_ERR_DEVICE, "hipGraphLaunch failed");
  return PF_OK;
}

// Debug forward: the ordinary forward plus SHADOW taps (flags & 1: stage / block boundary tensors copied into d_tap_buf, NHWC fp32) and / or RANGE records (flags & 2:
// statistics of every tensor that enters a dense contraction).  Synchronises the stream before it returns; the records are read with pf_debug_taps / pf_debug_ranges.
size_t pf_debug_tap_bytes(pf_handle h, int batch) {
  if (!h || batch <= 0 || batch > PF_MAX_BATCH || !h->finalized) return 0;
  DebugSink d;
  d.shadow = true;
  Ctx c{nullptr, 4096, 0, 0, true, nullptr};
  c.sb_planes = h->nterms == NT_F16X3 ? 2 : 3;
  c.dbg = &d;
  h->run(c, batch, nullptr, true, nullptr, nullptr, nullptr);
  return d.used + 256;
}
int pf_debug_forward_u8(pf_handle h, int batch, const uint8_t* in, float* pg, float* pl, float* params, void* ws, size_t ws_bytes, int flags, void* d_tap_buf,
                        size_t tap_bytes, void* stream) {
  if (!h) return PF_ERR_ARG;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if ((flags & 1) && !d_tap_buf) return h->fail(PF_ERR_ARG, "pf_debug_forward_u8: shadow taps need a buffer of pf_debug_tap_bytes(batch) bytes");
  if (h->prof.on || h->autotune) return h->fail(PF_ERR_ARG, "pf_debug_forward_u8: not inside a profiling window / with autotuning on");
  DebugSink& d = h->dbg;
  if (d.stats) { (void)hipFree(d.stats); }
  d = DebugSink();
  d.shadow = (flags & 1) != 0; d.range = (flags & 2) != 0;
  d.buf = static_cast<char*>(d_tap_buf); d.cap = tap_bytes;
  if (d.range) {
    d.max_ranges = 1024;
    if (hipMalloc(reinterpret_cast<void**>(&d.stats), (size_t)d.max_ranges * 16) != hipSuccess) { d.stats = nullptr; return h->fail(PF_ERR_DEVICE, "pf_debug_forward_u8: hipMalloc failed"); }
    (void)hipMemsetAsync(d.stats, 0, (size_t)d.max_ranges * 16, s);
  }
  h->debug_sink = &d;
  const int rc = h->forward(batch, in, true, pg, pl, params, ws, ws_bytes, s);
  h->debug_sink = nullptr;
  if (rc != PF_OK) return rc;
  if (hipStreamSynchronize(s) != hipSuccess) return h->fail(PF_ERR_DEVICE, "pf_debug_forward_u8: stream synchronisation failed");
  if (d.overflow) return h->fail(PF_ERR_WORKSPACE, fmt("pf_debug_forward_u8: tap buffer too small: %zu < %zu bytes", d.cap, d.used));
  return PF_OK;
}
int pf_debug_taps(pf_handle h, int max_records, char* names /*[max][64]*/, long long* byte_offsets, int* shapes /*[max][4]: B, H, W, C (NHWC)*/) {
  if (!h) return PF_ERR_ARG;
  const DebugSink& d = h->dbg;
  const int n = (int)std::min<size_t>(d.taps.size(), (size_t)(max_records < 0 ? 0 : max_records));
  for (int i = 0; i < n; ++i) {
    if (names) { std::strncpy(names + 64 * i, d.taps[i].name.c_str(), 63); names[64 * i + 63] = 0; }
    if (byte_offsets) byte_offsets[i] = (long long)d.taps[i].off;
    if (shapes) for (int k = 0; k < 4; ++k) shapes[4 * i + k] = d.taps[i].shape[k];
  }
  return (int)d.taps.size();
}
int pf_debug_ranges(pf_handle h, int max_records, char* names /*[max][96]*/, long long* elems, float* stats /*[max][4]: max |x|, sum x^2, saturated, non-finite*/) {
  if (!h) return PF_ERR_ARG;
  const DebugSink& d = h->dbg;
  const int n = (int)std::min<size_t>(d.ranges.size(), (size_t)(max_records < 0 ? 0 : max_records));
  if (n > 0 && stats && d.stats && hipMemcpy(stats, d.stats, (size_t)n * 16, hipMemcpyDeviceToHost) != hipSuccess) return h->fail(PF_ERR_DEVICE, "pf_debug_ranges: hipMemcpy failed");
  for (int i = 0; i < n; ++i) {
    if (names) { std::strncpy(names + 96 * i, d.ranges[i].name.c_str(), 95); names[96 * i + 95] = 0; }
    if (elems) elems[i] = d.ranges[i].elems;
    if (stats && d.stats) {  // the two counters are unsigned integers on the device (range_stats_kernel): hand them out as the floats the interface declares
      for (int k = 2; k < 4; ++k) { uint32_t u; std::memcpy(&u, &stats[4 * i + k], 4); stats[4 * i + k] = (float)u; }
    }
  }
  return (int)d.ranges.size();
}

int pf_forward_f32(pf_handle h, int batch, const float* in, float* pg, float* pl, float* params, void* ws, size_t ws_bytes, void* stream) {
  if (!h) return PF_ERR_ARG;
  return h->forward(batch, in, false, pg, pl, params, ws, ws_bytes, static_cast<hipStream_t>(stream));
}

// Optional on-disk tile cache (PF_TUNE_CACHE=<file>): read at pf_create, rewritten after every pf_autotune.
static int tile_table_load(pf_engine* h, const char* path);
static int tile_table_save(pf_engine* h, const char* path);
static void tune_cache_load(pf_engine* h) { if (const char* path = getenv("PF_TUNE_CACHE")) (void)tile_table_load(h, path); }
static void tune_cache_save(pf_engine* h) { if (const char* path = getenv("PF_TUNE_CACHE")) (void)tile_table_save(h, path); }

int pf_autotune(pf_handle h, int batch, const uint8_t* in, float* pg, float* pl, float* params, void* ws, size_t ws_bytes, void* stream) {
  if (!h) return PF_ERR_ARG;
  const int rc = h->forward(batch, in, true, pg, pl, params, ws, ws_bytes, static_cast<hipStream_t>(stream), true);
  if (rc == PF_OK) { h->tuned_batches[batch * 32 + h->nterms] = true; tune_cache_save(h); }
  return rc;
}

int pf_is_tuned(pf_handle h, int batch) { return (h && (!h->autotune || h->tuned_batches.count(batch * 32 + h->nterms))) ? 1 : 0; }

size_t pf_autotune_workspace_bytes(pf_handle h, int batch) {
  if (!h || !h->finalized || batch <= 0 || batch > PF_MAX_BATCH) return 0;
  return h->workspace_bytes(batch, true);
}

// Tile table files: one line per conv shape, "<12 key ints> <tile name>" (key = GEMM view, layout and precision of the
// launch).  Entries are keyed by shape and name, so a stale file can only cost speed, never correctness.
static int tile_table_load(pf_engine* h, const char* path) {
  FILE* f = fopen(path, "r");
  if (!f) return -1;
  char name[64];
  int k[12], n = 0;
  while (fscanf(f, "%d %d %d %d %d %d %d %d %d %d %d %d %63s", &k[0], &k[1], &k[2], &k[3], &k[4], &k[5], &k[6], &k[7], &k[8], &k[9], &k[10], &k[11], name) == 13) {
    for (int t = 0; t < conv_num_tiles(); ++t)
      if (std::strcmp(conv_tile_name(t), name) == 0) { h->tile_cache[std::vector<int>(k, k + 12)] = t; ++n; break; }
  }
  fclose(f);
  return n;
}
static int tile_table_save(pf_engine* h, const char* path) {
  FILE* f = fopen(path, "w");
  if (!f) return -1;
  int n = 0;
  for (auto& kv : h->tile_cache) {
    if (kv.second < 0) continue;
    for (int v : kv.first) fprintf(f, "%d ", v);
    fprintf(f, "%s\n", conv_tile_name(kv.second));
    ++n;
  }
  fclose(f);
  return n;
}
int pf_load_tile_table(pf_handle h, const char* path) {
  if (!h || !path) return PF_ERR_ARG;
  const int n = tile_table_load(h, path);
  return n < 0 ? h->fail(PF_ERR_ARG, fmt("pf_load_tile_table: cannot read '%s'", path)) : n;
}
int pf_save_tile_table(pf_handle h, const char* path) {
  if (!h || !path) return PF_ERR_ARG;
  const int n = tile_table_save(h, path);
  return n < 0 ? h->fail(PF_ERR_ARG, fmt("pf_save_tile_table: cannot write '%s'", path)) : n;
}

size_t pf_resize_workspace_bytes(int H, int W) { (void)W; return H > 0 ? (size_t)H * NET * 3 + 256 : 0; }

int pf_resize_bilinear_u8(pf_handle h, const uint8_t* d_img, int H, int W, uint8_t* d_out, void* ws, size_t ws_bytes, void* stream) {
  if (!h) return PF_ERR_ARG;
  if (!d_img || !d_out || H <= 0 || W <= 0) return h->fail(PF_ERR_ARG, "pf_resize_bilinear_u8: bad argument");
  if (!ws || ws_bytes < pf_resize_workspace_bytes(H, W)) return h->fail(PF_ERR_WORKSPACE, "pf_resize_bilinear_u8: workspace too small");
  if (hipSetDevice(h->device) != hipSuccess) return h->fail(PF_ERR_DEVICE, "hipSetDevice failed");
  ResizeTable* th = h->resize_table(W);  // first use of an extent builds + uploads its table (blocking copy, once)
  ResizeTable* tv = h->resize_table(H);
  if (!th || !tv) return h->fail(PF_ERR_DEVICE, "pf_resize_bilinear_u8: could not upload coefficient tables");
  uint8_t* tmp = reinterpret_cast<uint8_t*>((reinterpret_cast<uintptr_t>(ws) + 255) & ~(uintptr_t)255);
  launch_resize_u8(d_img, H, W, tmp, d_out, NET, NET, th->d_bounds, th->d_kk, th->ksize, tv->d_bounds, tv->d_kk, tv->ksize, static_cast<hipStream_t>(stream));
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return h->fail(PF_ERR_DEVICE, fmt("kernel launch failed: %s", hipGetErrorString(e)));
  return PF_OK;
}

int pf_resize_batch_u8(pf_handle h, int B, const uint8_t* const* h_imgs, const int32_t* h_hw, uint8_t* d_out, void* ws, size_t ws_bytes, void* stream) {
  if (!h) return PF_ERR_ARG;
  if (B <= 0 || !h_imgs || !h_hw || !d_out) return h->fail(PF_ERR_ARG, "pf_resize_batch_u8: bad argument");
  size_t need = 256;
  for (int i = 0; i < B; ++i) {
    if (!h_imgs[i] || h_hw[2 * i] <= 0 || h_hw[2 * i + 1] <= 0) return h->fail(PF_ERR_ARG, "pf_resize_batch_u8: bad image pointer or size");
    need += ((size_t)h_hw[2 * i] * NET * 3 + 255) & ~(size_t)255;
  }
  if (!ws || ws_bytes < need) return h->fail(PF_ERR_WORKSPACE, fmt("pf_resize_batch_u8: workspace too small: %zu < %zu bytes", ws_bytes, need));
  if (hipSetDevice(h->device) != hipSuccess) return h->fail(PF_ERR_DEVICE, "hipSetDevice failed");
  uint8_t* tmp = reinterpret_cast<uint8_t*>((reinterpret_cast<uintptr_t>(ws) + 255) & ~(uintptr_t)255);
  for (int i0 = 0; i0 < B; i0 += ResizeBatch::MAX) {
    ResizeBatch rb;
    rb.n = std::min(B - i0, (int)ResizeBatch::MAX);
    for (int k = 0; k < rb.n; ++k) {
      const int i = i0 + k, H = h_hw[2 * i], W = h_hw[2 * i + 1];
      ResizeTable* th = h->resize_table(W);  // first use of an extent builds + uploads its table (blocking copy, once)
      ResizeTable* tv = h->resize_table(H);
      if (!th || !tv) return h->fail(PF_ERR_DEVICE, "pf_resize_batch_u8: could not upload coefficient tables");
      rb.H[k] = H; rb.W[k] = W; rb.in[k] = h_imgs[i]; rb.tmp[k] = tmp; rb.out[k] = d_out + (size_t)i * NET * NET * 3;
      rb.bh[k] = th->d_bounds; rb.kh[k] = th->d_kk; rb.ksh[k] = th->ksize;
      rb.bv[k] = tv->d_bounds; rb.kv[k] = tv->d_kk; rb.ksv[k] = tv->ksize;
      tmp += ((size_t)H * NET * 3 + 255) & ~(size_t)255;
    }
    launch_resize_batch_u8(rb, NET, NET, static_cast<hipStream_t>(stream));
  }
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return h->fail(PF_ERR_DEVICE, fmt("kernel launch failed: %s", hipGetErrorString(e)));
  return PF_OK;
}

int pf_postprocess(pf_handle h, const float* pg, const float* pl, int H, int W, float* up, float* lat, void* ws, size_t ws_bytes, void* stream) {
  if (!h) return PF_ERR_ARG;
  if (!pg || !pl || !up || !lat || H <= 0 || W <= 0) return h->fail(PF_ERR_ARG, "pf_postprocess: bad argument");
  if (hipSetDevice(h->device) != hipSuccess) return h->fail(PF_ERR_DEVICE, "hipSetDevice failed");
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (h->arch == PF_ARCH_PERSNET_CLS) {
    const size_t need = (size_t)3 * NET * NET * 4 + 256;
    if (!ws || ws_bytes < need) return h->fail(PF_ERR_WORKSPACE, fmt("pf_postprocess: classification needs %zu workspace bytes", need));
    float* dg = reinterpret_cast<float*>((reinterpret_cast<uintptr_t>(ws) + 255) & ~(uintptr_t)255);
    float* dl = dg + 2 * NET * NET;
    launch_decode_cls(pg, 73, pl, 180, dg, dl, 1, NET * NET, s);
    launch_postprocess(dg, dl, NET, NET, up, lat, H, W, 0, s);
  } else {
    launch_postprocess(pg, pl, NET, NET, up, lat, H, W, 1, s);
  }
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return h->fail(PF_ERR_DEVICE, fmt("kernel launch failed: %s", hipGetErrorString(e)));
  return PF_OK;
}

int pf_postprocess_batch(pf_handle h, int B, const float* pg, const float* pl, const int32_t* hw, float* const* up, float* const* lat,
                         void* ws, size_t ws_bytes, void* stream) {
  if (!h) return PF_ERR_ARG;
  if (B <= 0 || !pg || !pl || !hw || !up || !lat) return h->fail(PF_ERR_ARG, "pf_postprocess_batch: bad argument");
  for (int i = 0; i < B; ++i)
    if (hw[2 * i] <= 0 || hw[2 * i + 1] <= 0 || !up[i] || !lat[i]) return h->fail(PF_ERR_ARG, "pf_postprocess_batch: bad size or output pointer");
  if (hipSetDevice(h->device) != hipSuccess) return h->fail(PF_ERR_DEVICE, "hipSetDevice failed");
  hipStream_t s = static_cast<hipStream_t>(stream);
  const bool cls = h->arch == PF_ARCH_PERSNET_CLS;
  const size_t npx = (size_t)NET * NET;
  float *dg = nullptr, *dl = nullptr;
  h->prof.mark(PH_POST, s);
  if (cls) {  // decode the argmax of all images first (workspace: 3 x 320 x 320 floats per image)
    const size_t need = (size_t)B * 3 * npx * 4 + 256;
    if (!ws || ws_bytes < need) return h->fail(PF_ERR_WORKSPACE, fmt("pf_postprocess_batch: classification needs %zu workspace bytes", need));
    dg = reinterpret_cast<float*>((reinterpret_cast<uintptr_t>(ws) + 255) & ~(uintptr_t)255);
    dl = dg + (size_t)B * 2 * npx;
    launch_decode_cls(pg, 73, pl, 180, dg, dl, B, NET * NET, s);
  }
  for (int i0 = 0; i0 < B; i0 += PostBatch::MAX) {
    PostBatch pb;
    pb.n = std::min(B - i0, (int)PostBatch::MAX);
    for (int k = 0; k < pb.n; ++k) {
      const int i = i0 + k;
      pb.H[k] = hw[2 * i]; pb.W[k] = hw[2 * i + 1];
      pb.g2[k] = cls ? dg + (size_t)i * 2 * npx : pg + (size_t)i * 2 * npx;
      pb.l1[k] = cls ? dl + (size_t)i * npx : pl + (size_t)i * npx;
      pb.up[k] = up[i]; pb.lat[k] = lat[i];
    }
    launch_postprocess_batch(pb, NET, NET, cls ? 0 : 1, s);
  }
  h->prof.mark(PH_END, s);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return h->fail(PF_ERR_DEVICE, fmt("kernel launch failed: %s", hipGetErrorString(e)));
  return PF_OK;
}

int pf_profile_begin(pf_handle h, unsigned class_mask) {
  if (!h) return PF_ERR_ARG;
  h->prof.reset();
  h->prof.mask = class_mask & 0x7fffffffu;
  h->prof.min_work = (class_mask & 0x80000000u) ? 2.0e11 : 0.0;  // bit 31: launches of >= 200 GFLOP only (the 256 -> 256 @80^2 convs, conv_fuse_conv0 / conv1 at B = 32)
  h->prof.on = true;
  return PF_OK;
}

int pf_profile_pause(pf_handle h) {
  if (!h) return PF_ERR_ARG;
  h->prof.on = false;  // no host synchronisation: the recorded events stay pending until pf_profile_end
  return PF_OK;
}

int pf_profile_end(pf_handle h, double* ms, double* work, long* launches, int n) {
  if (!h || n < PC_COUNT) return h ? h->fail(PF_ERR_ARG, "pf_profile_end: arrays must hold PF_PROFILE_CLASSES entries") : PF_ERR_ARG;
  h->prof.on = false;
  for (int i = 0; i < n; ++i) { ms[i] = 0; work[i] = 0; launches[i] = 0; }
  if (hipSetDevice(h->device) != hipSuccess) return h->fail(PF_ERR_DEVICE, "hipSetDevice failed");
  for (auto& r : h->prof.recs) {
    if (hipEventSynchronize(r.b) != hipSuccess) return h->fail(PF_ERR_DEVICE, "hipEventSynchronize failed");
    float t = 0.f;
    if (hipEventElapsedTime(&t, r.a, r.b) != hipSuccess) return h->fail(PF_ERR_DEVICE, "hipEventElapsedTime failed");
    r.ms = t;
    ms[r.cat] += t; work[r.cat] += r.work; launches[r.cat] += 1;
  }
  return PF_OK;  // records stay readable through pf_profile_records until the next pf_profile_begin
}

int pf_profile_records(pf_handle h, int max_records, int* cat, double* work, float* ms, int* mnk /*[max][4]: M, N, K, KH*/) {
  if (!h) return PF_ERR_ARG;
  const int n = (int)std::min<size_t>(h->prof.recs.size(), (size_t)(max_records < 0 ? 0 : max_records));
  for (int i = 0; i < n; ++i) {
    const auto& r = h->prof.recs[i];
    if (cat) cat[i] = r.cat;
    if (work) work[i] = r.work;
    if (ms) ms[i] = r.ms;
    if (mnk) { mnk[4 * i] = r.m; mnk[4 * i + 1] = r.n; mnk[4 * i + 2] = r.k; mnk[4 * i + 3] = r.kh; }
  }
  return (int)h->prof.recs.size();
}

int pf_profile_phases(pf_handle h, int n, double* ms) {
  if (!h || !ms || n < PF_PROFILE_PHASES) return h ? h->fail(PF_ERR_ARG, "pf_profile_phases: the array must hold PF_PROFILE_PHASES entries") : PF_ERR_ARG;
  for (int i = 0; i < n; ++i) ms[i] = 0.0;
  if (hipSetDevice(h->device) != hipSuccess) return h->fail(PF_ERR_DEVICE, "hipSetDevice failed");
  const auto& m = h->prof.marks;
  for (size_t i = 0; i + 1 < m.size(); ++i) {
    if (m[i].phase == PH_END) continue;   // the gap between two calls (forward -> post-process) belongs to nobody
    if (hipEventSynchronize(m[i + 1].e) != hipSuccess) return h->fail(PF_ERR_DEVICE, "hipEventSynchronize failed");
    float t = 0.f;
    if (hipEventElapsedTime(&t, m[i].e, m[i + 1].e) != hipSuccess) return h->fail(PF_ERR_DEVICE, "hipEventElapsedTime failed");
    ms[m[i].phase] += t;
  }
  return (int)m.size();
}

// ---- kernel-level entry points -------------------------------------------------------------

}  // extern "C"
