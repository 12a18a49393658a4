/* pf_hip.h -- C ABI of libpf_hip.so, the MI355X (gfx950) implementation of the
 * PerspectiveFields dense-field + ParamNet inference path.
 *
 * The reference (jinlinyi/PerspectiveFields) has no FFI layer: its boundary for this
 * path is the Python method PerspectiveFields.forward (perspective2d/perspectivefields.py:
 * 223-272), reached from .inference() (:194-205) and .inference_batch() (:207-221).
 * The entry points below are what a ctypes binding inside that class binds instead of
 * running the nn.Module tree:
 *
 *   pf_create / pf_load_tensor / pf_finalize_weights   <- PerspectiveFields.__init__ + _init_weights
 *                                                         (perspectivefields.py:122-192): build the
 *                                                         network for a zoo architecture and load
 *                                                         the {"model": state_dict} checkpoint
 *   pf_forward_u8 / pf_forward_f32                     <- forward() up to `results`
 *                                                         (perspectivefields.py:234-254,258): normalise,
 *                                                         backbone (mix_transformers.py:449-485), ll_enc
 *                                                         (:70-83), persformer_heads.inference
 *                                                         (persformer_heads.py:73-81), param_net
 *                                                         (param_network.py:46-69 / 193-221)
 *   pf_postprocess                                     <- persformer_heads.postprocess
 *                                                         (persformer_heads.py:83-101 ->
 *                                                         gravity_head.py:237-261, latitude_head.py:195-219,
 *                                                         utils/utils.py:483-507,114-130,148-162)
 *
 * Conventions: plain pointers and sizes only.  Every `d_` pointer is a DEVICE pointer owned
 * by the caller; `h_` pointers are host memory.  All work is enqueued on the given
 * hipStream_t (passed as void*) and never synchronises.  Return value 0 = success,
 * negative = pf_status; pf_last_error() gives the message.  A handle is bound to one
 * device and is not thread-safe.  A workspace (`d_ws`) belongs to the calls in flight on it: two calls that
 * share one workspace must be ordered by the caller (same stream, or an event between the streams) -- the
 * Python host side does this for its own workspace (Engine._order_scratch).  There is no CPU fallback: every entry point fails with
 * PF_ERR_DEVICE when no gfx950 device is usable.
 */
#ifndef PF_HIP_H
#define PF_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct pf_engine* pf_handle;

enum pf_status {
  PF_OK = 0,
  PF_ERR_ARG = -1,      /* bad argument (null pointer, bad shape, unknown arch) */
  PF_ERR_DEVICE = -2,   /* no usable HIP device / HIP runtime error */
  PF_ERR_WEIGHTS = -3,  /* missing / unexpected / mis-shaped checkpoint tensor, or forward before finalize */
  PF_ERR_WORKSPACE = -4 /* workspace too small */
};

/* architectures = the three module trees the reference zoo instantiates (perspectivefields.py:86-118) */
enum pf_arch {
  PF_ARCH_PARAMNET_CENTERED = 0,   /* regression heads (2 / 1 ch) + ParamNet (ConvNeXt-T, 5 raw outputs) */
  PF_ARCH_PERSNET_CLS = 1,         /* classification heads (73 / 180 logits), no ParamNet */
  PF_ARCH_PARAMNET_UNCENTERED = 2  /* regression heads + ParamNetConvNextRegress (64x64 input, 5 outputs) */
};

#define PF_NET_SIZE 320  /* the network always runs at 320x320 (every reference YAML: DATALOADER.RESIZE) */
#define PF_PARAMS_STRIDE 8
/* Largest batch one pf_forward_* call accepts: the kernels address each activation with 32-bit byte offsets, and the
 * largest per-head activation is 26.2 MB per image (2 GiB / 26.2 MB = 81).  Larger batches return PF_ERR_ARG; the host
 * layer (PerspectiveFields._run) splits longer image lists into chunks, as the reference's callers may pass any length. */
#define PF_MAX_BATCH 81

const char* pf_version(void);
const char* pf_build_digest(void); /* digest of the sources this library was built from (stale-library check of the loader) */
const char* pf_last_error(pf_handle h); /* h may be NULL: error of the last failed pf_create on this thread */

/* device = PF_DEVICE_NONE: the engine's HOST side only -- checkpoint loading, weight repack / folds / splits (kept in host memory), the workspace dry run and the tile
 * table work; every entry point that needs a GPU returns PF_ERR_DEVICE.  The seam the sanitizer build is tested through (PF_ASAN=1 python -m perspectivefields_amd.build,
 * tests/test_host_asan.py); not a CPU path of the network. */
#define PF_DEVICE_NONE (-1)
int pf_create(pf_handle* out, int device, int arch);
int pf_destroy(pf_handle h);

/* Checkpoint tensors by their reference state_dict key (schema: SURVEY.md appendix B), fp32, C-contiguous.
 * `ll_enc.bn1.num_batches_tracked` is accepted and ignored. */
int pf_load_tensor(pf_handle h, const char* key, const float* h_data, const int64_t* shape, int rank);
/* Strict validation (all keys of the architecture present, none unknown), BatchNorm / layer-scale folding,
 * repack to the kernels' layouts, upload. */
int pf_finalize_weights(pf_handle h);

/* channel counts of the API-visible 320x320 maps and number of raw ParamNet outputs (0 if none) */
int pf_output_info(pf_handle h, int* gravity_channels, int* latitude_channels, int* param_raw_outputs);

int pf_max_batch(void); /* = PF_MAX_BATCH */

/* bytes of scratch pf_forward_* needs for a batch of `batch` images (0 for batch <= 0 or > PF_MAX_BATCH) */
size_t pf_workspace_bytes(pf_handle h, int batch);

/* Forward pass for `batch` images already resized to 320x320.
 *   d_images_u8   : [batch][320][320][3] uint8, BGR (what ResizeTransform.apply_image returns, :201)
 *   d_images_f32  : [batch][3][320][320] fp32 BGR 0..255 (the "image" entries forward() receives, :234)
 *   d_pred_gravity : [batch][Cg][320][320] fp32 -- unit up-vectors (Cg=2) or 73 logits
 *   d_pred_latitude: [batch][Cl][320][320] fp32 -- sin(latitude) in [-1,1] (Cl=1) or 180 logits
 *   d_params       : [batch][PF_PARAMS_STRIDE] fp32 or NULL when the arch has no ParamNet:
 *                    CENTERED  : roll, pitch, vfov (deg), rel_focal, raw x0..x3   (param_network.py:62-67)
 *                    UNCENTERED: raw x0..x4 (roll/90, pitch/90, general_vfov/90, rel_cx, rel_cy), rel_focal (closed form of utils/utils.py:47-91 general_vfov_to_focal,
 *                                fp64 on the device), 0, 0   (param_network.py:204-220)
 */
/* Arithmetic of the dense contractions (everything else is always fp32).
 *   FP32 (default, the parity mode): "split-f16" -- every fp32 activation is split on the fly into two fp16 values
 *     (a ~ ah + al with ah = fp16(a), al = fp16(a - ah) UNSCALED: 22-23 significant bits for |a| >= 2^-3, an absolute 2^-25 per element below -- the matrix cores keep fp16 subnormals), the weights (scaled per output channel by a power of two) into wh + wl,
 *     and a product is three fp16 MFMA partial products (ah wh + ah wl + al wh) accumulated in fp32: per-product error
 *     <= 3 * 2^-22, below the fp32 accumulation noise of the contraction itself (scripts/emulate_split.py).
 *     Activations beyond the fp16 range (|x| > 65504) saturate.
 *   FP32_BF16X6: every operand split EXACTLY into three bf16 values, six bf16 MFMA partial products -- fp32-accurate
 *     for any fp32 input (no range restriction), twice the matrix-core work.
 * NO reduced-precision mode is offered (r05): r01-r04 carried "bf16x3" / "bf16" switches on these same kernels -- 98.9 % argmax agreement for +0.6 ... 4 % speed,
 * i.e. lower accuracy for nothing (profiles/r04_bench_configs.json) -- and a bf16 THROUGHPUT path (bf16 activations in HBM, one MFMA per product, its own tile
 * table) was not built; values 1 and 2 of earlier headers are rejected with PF_ERR_ARG.
 * May be called at any time; it applies to the following forwards (tile choices are tuned per mode). */
#define PF_PRECISION_FP32 0
#define PF_PRECISION_FP32_BF16X6 3
int pf_set_precision(pf_handle h, int mode);

/* Always-on saturation watch of the FP32 (split-f16) mode.  d_counter_u32: a caller-owned, zero-initialised 4-byte device counter (nullptr: off).  Every kernel that
 * WRITES a tensor a split-f16 contraction will read (GEMM / conv epilogues, the fused block MLPs, the Winograd convs) adds to it the number of 16-byte output groups
 * with an element beyond the window of that tensor's consumer (65504; 65504 / 4 = 16376 in front of a Winograd conv; 8188 / 4094 for the attention operands; the
 * input limit of a depthwise conv, from its weights).  Cost: one compare per 4 outputs; the counter only ever grows.  Read it in stream order behind a forward (a
 * 4-byte copy): unchanged = every dense-layer input of that forward was inside the window.
 *
 * THE CONTRACT FOR A CALLER THAT PINS PF_PRECISION_FP32 (mandatory reading since r05, when the 256 -> 256 decoder convs became Winograd F(2x2, 3x3)):
 *   - outside a window the direct tiles SATURATE (the split clamps to +-65504: a finite, wrong result), but the Winograd layers' input transform adds four values
 *     and splits WITHOUT the clamp: an input in (16376, 65504] may, and one beyond certainly does, turn into +-inf / NaN in that layer's output;
 *   - both cases move the counter: the producer of such an input is watched with the 16376 limit, and the Winograd / row-block / fused-MLP epilogues also count NaN
 *     (inf - inf) outputs; the register-capped GEMM tiles count saturation and +-inf only (a NaN reaches them only behind a producer that was already counted);
 *   - so: a forward that left the counter unchanged is inside every window and its results are fp32-class; a forward that moved it MUST be discarded and re-run
 *     with PF_PRECISION_FP32_BF16X6 (no window).  There is no third case, and no output of a counted forward is promised to be finite.
 *   The Python layer does exactly that with `precision="auto"` (the default) and stays in the exact mode afterwards; `precision="fp32"` skips the check -- and the
 *   host synchronisation it costs -- and leaves the counter to the caller (tests/test_gpu_e2e.py::test_pinned_fp32_window_contract).
 * Tensors no kernel can watch (LayerNorm outputs, the register-only hidden maps of the fused MLPs) are bounded from the weights alone: pf_static_window_max returns
 * the largest such bound, scaled so that a value > 65504 means "a static bound exceeds its window". */
int pf_set_saturation_counter(pf_handle h, void* d_counter_u32);
int pf_static_window_max(pf_handle h, float* out);

int pf_forward_u8(pf_handle h, int batch, const uint8_t* d_images_u8, float* d_pred_gravity, float* d_pred_latitude,
                  float* d_params, void* d_workspace, size_t workspace_bytes, void* stream);
int pf_forward_f32(pf_handle h, int batch, const float* d_images_f32, float* d_pred_gravity, float* d_pred_latitude,
                   float* d_params, void* d_workspace, size_t workspace_bytes, void* stream);

/* Deferred ParamNet branch (throughput option for callers that issue forward after forward on one stream; off by default).  With on != 0 the ConvNeXt branch of a
 * forward (param_network.py:46-69, convnext.py:140-152) runs on a stream owned by the engine, behind that forward's decoders, and the call returns without joining it:
 * the NEXT forward's backbone (other images, no dependency) runs beside it -- both are chains of small launches that leave most of the chip idle.  d_pred_gravity /
 * d_pred_latitude are valid in `stream` order as always; d_params of a forward becomes valid in `stream` order once the next pf_forward_* has been issued on that
 * stream (it waits for the branch before its decoders overwrite the branch's input) or after pf_join_params(h, stream).  The caller keeps d_params alive until then. */
int pf_set_defer_params(pf_handle h, int on);
int pf_join_params(pf_handle h, void* stream);

/* Low-latency form of pf_forward_u8 for small batches: the ~430 launches of a forward are captured once per (batch, buffer
 * set) into a hipGraph and replayed with one launch (host launch cost, not GPU time, bounds a batch-1 forward).  Same
 * arguments and results; `stream` must be an explicit stream (not the legacy NULL stream); the graph is re-captured when
 * any buffer pointer changes, so callers keep their buffers (the Python layer does). */
int pf_forward_u8_graph(pf_handle h, int batch, const uint8_t* d_images_u8, float* d_pred_gravity, float* d_pred_latitude,
                        float* d_params, void* d_workspace, size_t workspace_bytes, void* stream);

/* Device-side replacement of ResizeTransform.apply_image (perspectivefields.py:34-46,201): PIL's antialiased BILINEAR
 * resize of one uint8 [H][W][3] image to [320][320][3], bit-identical to PIL (integer two-pass filter; coefficient
 * tables built on the host exactly as Pillow does and cached per extent in the handle -- the first call for a new
 * extent performs a small blocking upload).  d_out may point into the batch tensor given to pf_forward_u8. */
size_t pf_resize_workspace_bytes(int H, int W);
int pf_resize_bilinear_u8(pf_handle h, const uint8_t* d_img, int H, int W, uint8_t* d_out_320, void* d_workspace,
                          size_t workspace_bytes, void* stream);

/* The same for a whole batch in two launches per 32 images (inference_batch's per-image resize loop, :210-216):
 * h_imgs = HOST array of B DEVICE pointers to uint8 [H_i][W_i][3] images, h_hw = HOST array [B][2] of (H_i, W_i);
 * d_out = [B][320][320][3] (the tensor pf_forward_u8 takes).  Workspace: sum over images of roundup(H_i * 320 * 3, 256) + 256 bytes. */
int pf_resize_batch_u8(pf_handle h, int batch, const uint8_t* const* h_imgs, const int32_t* h_hw, uint8_t* d_out_320,
                       void* d_workspace, size_t workspace_bytes, void* stream);

/* Tile configuration of the conv / GEMM launches.  Default: a table keyed by launch shape (loaded with pf_load_tile_table;
 * the Python layer loads the one shipped for gfx950, perspectivefields_amd/tuned/gfx950_tiles.txt) and a static heuristic
 * for shapes the table does not hold -- deterministic, no first-call stall.
 * pf_autotune: explicit one-time tuning for a batch size: a normal forward (same arguments and results as pf_forward_u8;
 * workspace of pf_autotune_workspace_bytes) in which every conv / GEMM launch is additionally timed with each tile
 * configuration on this device (HIP events; this call DOES wait on the stream); the fastest per shape is cached in the
 * handle (pf_save_tile_table writes the cache out).  With PF_AUTOTUNE=1 in the environment the Python layer runs it on the
 * first forward of every new batch size; pf_is_tuned then tells whether a batch size has been tuned.
 * pf_load_tile_table / pf_save_tile_table return the number of entries read / written, or a negative pf_status. */
size_t pf_autotune_workspace_bytes(pf_handle h, int batch);
int pf_autotune(pf_handle h, int batch, const uint8_t* d_images_u8, float* d_pred_gravity, float* d_pred_latitude,
                float* d_params, void* d_workspace, size_t workspace_bytes, void* stream);
int pf_is_tuned(pf_handle h, int batch);
int pf_load_tile_table(pf_handle h, const char* path);
int pf_save_tile_table(pf_handle h, const char* path);

/* Post-process ONE image's 320x320 predictions to its original size (H, W):
 *   d_up_out  : [2][H][W] unit up-vectors (x right, y down), d_lat_out : [H][W] degrees.
 * For the classification arch d_workspace must hold 3*320*320 floats (decoded fields). */
int pf_postprocess(pf_handle h, const float* d_pred_gravity, const float* d_pred_latitude, int H, int W,
                   float* d_up_out, float* d_lat_out, void* d_workspace, size_t workspace_bytes, void* stream);

/* ---- per-kernel-class timing with HIP events on the launch stream (bench.py `roofline`) ----
 * classes: 0 implicit-GEMM conv/GEMM (work = algorithmic FLOPs, 2*M*Cout*KH*KW*Cin), 1 attention (FLOPs),
 * 2 LayerNorm, 3 depthwise3x3+GELU, 4 depthwise7x7, 5 bilinear x2 (work = algorithmic bytes in+out), 6 other,
 * 7 implicit-GEMM launches served by the split-bf16 kernel (class 0 then counts only the exact-fp32 MFMA launches).
 * Between begin and end every launch of a class whose bit is set in class_mask is bracketed by an
 * event pair; pf_profile_end synchronises those events and sums elapsed ms / work / launches per class.
 * class_mask bit 31 (PF_PROFILE_LARGE_ONLY): only launches of >= 200 GFLOP are bracketed (a dozen per B = 32 step: the dominant
 * decoder convs) -- cheap enough for every timed step of a benchmark, and the internal side stream stays on. */
#define PF_PROFILE_CLASSES 8
#define PF_PROFILE_LARGE_ONLY 0x80000000u
int pf_profile_begin(pf_handle h, unsigned class_mask);
/* stop bracketing further launches without synchronising (the window can cover the first steps of a timed loop only) */
int pf_profile_pause(pf_handle h);
int pf_profile_end(pf_handle h, double* ms, double* work, long* launches, int n);
/* per-launch records of the last begin/end window (valid until the next pf_profile_begin); returns the
 * total number of records, fills at most max_records entries; mnk = GEMM view [M, N, K, KH] for class 0 */
int pf_profile_records(pf_handle h, int max_records, int* cat, double* work, float* ms, int* mnk);
/* Component split of the path: inside a FULL per-launch window (class_mask without PF_PROFILE_LARGE_ONLY: one stream, forwards joined) the engine also
 * records an event at the start of every component -- 0 input normalisation + MiT-B3 backbone (mix_transformers.py:449-485), 1 low-level encoder
 * (perspectivefields.py:70-83), 2 both decoder heads + prediction heads (gravity_head.py:139-197, latitude_head.py:138-193), 3 ParamNet (param_network.py:46-69),
 * 4 post-process (pf_postprocess_batch).  Call after pf_profile_end: ms[PF_PROFILE_PHASES] = elapsed stream time per component summed over the window (launch gaps and
 * the profile's own event pairs included); returns the number of marks recorded. */
#define PF_PROFILE_PHASES 5
#define PF_PHASE_BACKBONE 0
#define PF_PHASE_LOW_LEVEL 1
#define PF_PHASE_DECODERS 2
#define PF_PHASE_PARAMNET 3
#define PF_PHASE_POSTPROCESS 4
int pf_profile_phases(pf_handle h, int n, double* ms);

/* ---- Debug forward: localise a numerical problem layer by layer, and check a checkpoint's activations against the split-f16 scheme's window.
 * The reference has no such mode; it replaces "print the tensor after every module" in a PyTorch session (perspectivefields.py:223-272 run by hand).
 *   flags & 1  SHADOW taps: the boundary tensors of the path -- every MiT block output "mit.s<stage>.b<block>" (mix_transformers.py:198-202), the four stage
 *              outputs "c1".."c4" (:457-485), the low-level encoder output "ll" (perspectivefields.py:70-83), both decoders' "dec.<head>.conv0" maps
 *              (gravity_head.py:170-171), the ParamNet input "pn.in", stem "pn.stem" and every ConvNeXt block output "pn.s<stage>.b<block>" (convnext.py:46-59,
 *              140-152) -- are copied, NHWC fp32, into d_tap_buf (pf_debug_tap_bytes(batch) bytes); pf_debug_taps returns names, byte offsets and shapes.
 *   flags & 2  RANGE records: for every tensor that enters a dense contraction (all conv / linear layers incl. the fused block MLPs, attention q / kv) max |x|, sum x^2,
 *              the number of elements beyond the fp16 range (the default precision SATURATES them at 65504) and of non-finite elements; pf_debug_ranges returns them.
 *              A tensor whose rms is below ~2^-5 loses relative accuracy in the default precision (the low part of the split turns subnormal below |x| = 2^-3):
 *              run such a checkpoint with PF_PRECISION_FP32_BF16X6.
 * Same results as pf_forward_u8; synchronises the stream before returning.  The record functions return the total number of records and fill at most max_records. */
size_t pf_debug_tap_bytes(pf_handle h, int batch);
int pf_debug_forward_u8(pf_handle h, int batch, const uint8_t* d_in_u8, float* d_pred_gravity, float* d_pred_latitude, float* d_params, void* d_workspace,
                        size_t workspace_bytes, int flags, void* d_tap_buf, size_t tap_bytes, void* stream);
int pf_debug_taps(pf_handle h, int max_records, char* names /*[max][64]*/, long long* byte_offsets, int* shapes /*[max][4]: B, H, W, C*/);
int pf_debug_ranges(pf_handle h, int max_records, char* names /*[max][96]*/, long long* elems, float* stats /*[max][4]*/);

/* ---- Dispatch report: WHICH kernels the last pf_forward_* of this handle launched, on how many streams, out of how much scratch.  That is decided per forward from the
 * batch size and the PF_* switches; the report lets a caller (and the test-suite) see the decision instead of trusting it.  Plain host counters incremented at the
 * decision points: no device work, no synchronisation, the launches are the same with or without a reader.  out = HOST array of at least PF_DISPATCH_COLS entries.
 * A graph REPLAY (pf_forward_u8_graph after its capture) runs no host dispatch and leaves the report of the capturing call; pf_autotune's forward reports only the
 * peaks and the launcher counts.  With PF_DEFER_AT > 0 the previous forward's ParamNet branch is issued, and counted, inside the next forward. */
#define PF_DISPATCH_BATCH 0
#define PF_DISPATCH_S3_SPLIT_TAKEN 1          /* 1: MiT stage 3 walked the batch as two half-batches on two streams */
#define PF_DISPATCH_RB_LAUNCHES 2             /* row-block linears (rb_gemm.hip) and rb_chain.hip launches */
#define PF_DISPATCH_SPLITK_LAUNCHES 3         /* convs that really ran split-K (+ reduce) */
#define PF_DISPATCH_SPLITK_MAX_FACTOR 4       /* ... and their largest factor (0: none) */
#define PF_DISPATCH_WINO_LAUNCHES 5           /* Winograd F(2x2, 3x3) launches */
#define PF_DISPATCH_WINO_HALF_LAUNCHES 6      /* ... of them in the half-patch geometry */
#define PF_DISPATCH_THIN128_LAUNCHES 7        /* thin 128 -> 128 projections (thin_linear.hip) */
#define PF_DISPATCH_ATTN64_LAUNCHES 8         /* one-kernel attention halves of the stage-1 blocks (attn_block.hip) */
#define PF_DISPATCH_MIT_MLP_FUSED_LAUNCHES 9  /* one-kernel Mlps of MiT stages 1 / 2 (mit_mlp.hip) */
#define PF_DISPATCH_LN_KERNEL_LAUNCHES 10     /* stand-alone LayerNorm launches */
#define PF_DISPATCH_CONV_LAUNCHES 11          /* launches through the engine's conv / linear dispatcher (all tile kinds, Winograd included) */
#define PF_DISPATCH_SB_TENSORS 12             /* activations allocated as split planes (PF_SBA, PF_SBA_HEADS, the exact scheme's ParamNet) */
#define PF_DISPATCH_FORKS 13                  /* fork windows: copies of the workspace allocator handed to a side stream */
#define PF_DISPATCH_FORK_ALLOC_CONFLICTS 14   /* fork windows in which BOTH the copy and the parent allocated (two streams, one scratch offset): must be 0 */
#define PF_DISPATCH_REAL_PEAK_BYTES 15        /* what the forward allocated from the workspace (main region + ParamNet region) */
#define PF_DISPATCH_DRY_PEAK_BYTES 16         /* what pf_workspace_bytes' dry run sized for them; real > dry in either region: the call returns PF_ERR_WORKSPACE */
#define PF_DISPATCH_CNX_RB_LAUNCHES 17        /* row-block fused ConvNeXt block MLPs of the 384- / 768-channel stages (cnx_rb.hip); not part of RB_LAUNCHES */
#define PF_DISPATCH_DEC_EARLY_TAKEN 18        /* 1: the decoders' first convs of levels 0-2 (PF_DEC_EARLY=2: and r1c1) were issued on a side stream beside MiT stage 4 */
#define PF_DISPATCH_COLS 19
int pf_last_dispatch(pf_handle h, int64_t* out, int n);

/* The same for a whole batch in one launch per 32 images (the reference's per-image Python loop,
 * gravity_head.py:244-260 / latitude_head.py:201-218): h_hw = HOST array [B][2] of (H, W); h_up_out / h_lat_out = HOST
 * arrays of B DEVICE pointers ([2][H][W] and [H][W] each).  Classification arch: workspace of B*3*320*320 floats. */
int pf_postprocess_batch(pf_handle h, int batch, const float* d_pred_gravity, const float* d_pred_latitude, const int32_t* h_hw,
                         float* const* h_up_out, float* const* h_lat_out, void* d_workspace, size_t workspace_bytes, void* stream);

/* Row N4: camera parameters -> perspective fields on the device, the step every demo of the reference runs
 * right after inference (utils/utils.py:325-381 -> PanoCam.get_up_general / get_lat_general, utils/panocam.py:451-556).
 * d_cam5 = {roll, pitch (= elevation), both in RADIANS, rel_focal, rel_cx, rel_cy} in device memory (so the ParamNet
 * output can feed it without a host round trip); outputs in the layout of pred_gravity_original /
 * pred_latitude_original: d_up [2][H][W] unit vectors, d_lat [H][W] degrees.  No handle: the op is stateless. */
int pf_fields_from_params(int device, const float* d_cam5, int H, int W, float* d_up, float* d_lat, void* stream);

/* The inverse of pf_fields_from_params: perspective fields -> camera parameters, a batched per-image Levenberg-Marquardt
 * least-squares fit.  Parameters theta = (roll, pitch, f, cx, cy): roll / pitch in radians, f = rel_focal,
 * cx / cy = rel_cx / rel_cy.  free_pp = 0: 3 free parameters, cx / cy held at their start values (0 without d_init); 1: all 5 free.
 * Model at pixel (row, col) of an H x W image, with px = col + 0.5, py = row + 0.5, F = f*H, Cx = (cx + 0.5)*W, Cy = (cy + 0.5)*H:
 *   up  u = -(sin r cos p F + sin p (px - Cx), cos r cos p F + sin p (py - Cy)) / |.|   (the reference's (vvp - xy) sign(p) times
 *       |sin p|: same direction for p != 0, the reference's (-sin r, -cos r) at p = 0, no 1/sin p)
 *   lat = -atan2(y_w, sqrt(x_w^2 + z_w^2)) degrees on the reference's linspace grid x = (col W/(W-1) - Cx)/F, y = (row H/(H-1) - Cy)/F,
 *       exactly as pf_fields_from_params.
 * Residuals r_up = (u_model - u_pred) * 180/pi (2 components), r_lat = lat_model - lat_pred (degrees); pixels with a non-finite
 * input value are skipped.  Loss sum w_up rho(|r_up|) + w_lat rho(|r_lat|), rho = r^2/2 (PF_FIT_LOSS_L2) or Huber with
 * huber_delta_deg (PF_FIT_LOSS_HUBER, by IRLS weights).  Start: d_init = NULL -> roll / pitch from the fields at the image centre and
 * f from a 16-candidate vFoV search in [15, 150] deg; else d_init = DEVICE [B][5] theta (the layout of d_cam5).
 * Stops per image when an accepted step changes the cost by < 1e-10 relative, a step is < 1e-9, or after max_iter steps.
 * h_hw = HOST [B][2] (H, W), each >= 8; h_up / h_lat = HOST arrays of B DEVICE pointers ([2][H][W] and [H][W] degrees fp32).
 * d_out = DEVICE [B][PF_FIT_COLS] fp32, columns below (angles in degrees).  Workspace: pf_fit_camera_workspace_bytes(B, h_hw).
 * Enqueues max_iter + 1 (accumulate, solve) launch pairs per 32 images on `stream`, no host synchronisation; deterministic. */
#define PF_FIT_COL_ROLL 0
#define PF_FIT_COL_PITCH 1
#define PF_FIT_COL_VFOV 2          /* 2 atan(1 / (2 f)) */
#define PF_FIT_COL_REL_FOCAL 3
#define PF_FIT_COL_GENERAL_VFOV 4  /* acos((P + Q - 1) / (2 sqrt(P Q))), P = f^2 + cx^2 + (cy + 1/2)^2, Q = f^2 + cx^2 + (cy - 1/2)^2 */
#define PF_FIT_COL_REL_CX 5
#define PF_FIT_COL_REL_CY 6
#define PF_FIT_COL_RMS_UP 7        /* sqrt(mean |r_up|^2), degree scale */
#define PF_FIT_COL_RMS_LAT 8       /* sqrt(mean r_lat^2), degrees */
#define PF_FIT_COL_COST 9          /* the loss above at the result */
#define PF_FIT_COL_ITERATIONS 10   /* LM steps evaluated (accepted or rejected) */
#define PF_FIT_COL_CONVERGED 11    /* 1: a tolerance was met; 0: stopped at max_iter */
#define PF_FIT_COL_VALID_PIXELS 12 /* pixels with finite input */
#define PF_FIT_COLS 13
#define PF_FIT_LOSS_L2 0
#define PF_FIT_LOSS_HUBER 1
size_t pf_fit_camera_workspace_bytes(int batch, const int32_t* h_hw);
int pf_fit_camera(int device, int batch, const int32_t* h_hw, const float* const* h_up, const float* const* h_lat, const float* d_init,
                  int free_pp, int loss, float huber_delta_deg, float w_up, float w_lat, int max_iter, float* d_out, void* d_workspace,
                  size_t workspace_bytes, void* stream);

/* The same fit for the Unified Spherical Model (USM): the mirror parameter xi of pf_pano_crop's distorted views is one more unknown
 * (DESIGN.md section 14).  theta = (roll r, pitch p, f, cx, cy, xi).  free_pp = 0: 4 free parameters (r, p, f, xi), cx / cy held at their
 * start values (0 without d_init); 1: all 6 free.  THE MODEL -- pf_pano_crop's intrinsics, ray, rotation and label formulas; yaw does not enter:
 *   F = f*H, Cx = (cx + 1/2)*W, Cy = (cy + 1/2)*H
 *   image point (a, b) -> x = (a - Cx)/F, y = (b - Cy)/F, rho^2 = x^2 + y^2, disc = 1 + (1 - xi^2) rho^2, eta = (xi + sqrt(disc)) / (1 + rho^2),
 *       X = (eta x, eta y, eta - xi), X_w = R_pitch(p) R_roll(r) X
 *   up at (col + 1/2, row + 1/2): with g = R^T (0, -1, 0), D = X_z + xi, s = g_z + xi (X . g): (g_x D - X_x s, g_y D - X_y s) normalised
 *   lat in degrees: that of X_w at the linspace point (col W/(W-1), row H/(H-1))
 *   a pixel with disc < 0 at either point has no model value: weight 0, not counted in VALID_PIXELS
 * At xi = 0 this is the pinhole model of pf_fit_camera.  Residuals, loss, weights, accept / reject rule, damping and stopping rule: as pf_fit_camera.
 * Clamps: |pitch| <= 89.9 deg, f >= 1e-3, xi in [-0.5, 2] (negative on purpose: a pinhole truth is an interior point); roll is kept in
 * [-pi, pi] (it is periodic, and a long early step of the 6-parameter fit may land whole turns away).
 * Start: d_init = NULL -> roll / pitch from the fields at the image centre (the centre ray is (0, 0, 1) for every xi), xi = 0 and f from the
 * 16-candidate vFoV search; else d_init = DEVICE [B][6] theta (angles in radians).  xi > 1 leaves part of the image without a ray, a region
 * that moves with the parameters: such cameras are supported from a caller-supplied start, not promised from the blind one.
 * d_out = DEVICE [B][PF_USMFIT_COLS] fp32: the thirteen columns of pf_fit_camera in the same order, then xi.  VFOV and GENERAL_VFOV keep
 * their formulas in f, cx, cy: under xi != 0 they describe the intrinsics, not the angle the image subtends.
 * Sizes, pointers, argument checks (PF_ERR_ARG before any device work), launches (max_iter + 1 pairs per 32 images on `stream`, no host
 * synchronisation) and determinism (an image's bits do not depend on its batch) as pf_fit_camera; workspace pf_fit_camera_usm_workspace_bytes
 * (0 for batch <= 0 or a size below 8). */
#define PF_USMFIT_COL_ROLL 0
#define PF_USMFIT_COL_PITCH 1
#define PF_USMFIT_COL_VFOV 2
#define PF_USMFIT_COL_REL_FOCAL 3
#define PF_USMFIT_COL_GENERAL_VFOV 4
#define PF_USMFIT_COL_REL_CX 5
#define PF_USMFIT_COL_REL_CY 6
#define PF_USMFIT_COL_RMS_UP 7
#define PF_USMFIT_COL_RMS_LAT 8
#define PF_USMFIT_COL_COST 9
#define PF_USMFIT_COL_ITERATIONS 10
#define PF_USMFIT_COL_CONVERGED 11
#define PF_USMFIT_COL_VALID_PIXELS 12 /* pixels with finite input and a ray */
#define PF_USMFIT_COL_XI 13
#define PF_USMFIT_COLS 14
size_t pf_fit_camera_usm_workspace_bytes(int batch, const int32_t* h_hw);
int pf_fit_camera_usm(int device, int batch, const int32_t* h_hw, const float* const* h_up, const float* const* h_lat,
                      const float* d_init /* NULL or [B][6] */, int free_pp, int loss, float huber_delta_deg, float w_up, float w_lat,
                      int max_iter, float* d_out /* [B][PF_USMFIT_COLS] */, void* d_workspace, size_t workspace_bytes, void* stream);

/* The two fits above with the intrinsics shared across the images of one camera: the frames of a video, a photo set
 * of one device.  The batch is divided into camera groups of consecutive images: h_group_sizes = HOST [n_groups], every entry >= 1, summing to
 * batch.  Every image keeps its own roll and pitch; all images of a group share f, with free_pp = 1 also cx and cy, with model = 1 also xi.
 * model = 0: the pinhole fit (theta [5], rows of PF_FIT_COLS); 1: the USM fit (theta [6], rows of PF_USMFIT_COLS).  Model, residuals, loss,
 * weights and clamps per image: as pf_fit_camera / pf_fit_camera_usm; the objective of a group is the sum over its images.
 * One Levenberg-Marquardt iteration of a group, with H_i = [A_i B_i; B_i^T C_i] and g_i = (g_a, g_s) the normal matrix and gradient of image i,
 * A_i its 2 x 2 (roll, pitch) block and C_i the block of the NS shared parameters -- the whole block-arrow system is damped, then every A_i eliminated:
 *   A'_i = A_i + lambda diag A_i, C' = sum C_i + lambda diag(sum C_i), S = C' - sum B_i^T A'_i^-1 B_i, b = sum (g_s - B_i^T A'_i^-1 g_a)
 *   delta_s = -S^-1 b (Cholesky, fp64), delta_a_i = -A'_i^-1 (g_a + B_i delta_s)
 * One lambda per group; a trial is accepted when the cost summed over the group falls, otherwise lambda x 10 with the same linearisation.
 * Stopping: the constants of pf_fit_camera on the group's cost and longest step; all images of a group stop together.
 * Start: that of the per-image fit for every image (blind, or d_init = DEVICE [B][5 or 6]), then per group f = exp(mean log f) and cx, cy, xi =
 * the means over its images.  An image without a valid pixel contributes nothing to the steps: its row keeps its start roll and pitch,
 * VALID_PIXELS 0 and CONVERGED 0, and follows the group's shared parameters.  A group without any valid pixel keeps its start, CONVERGED 0.
 * d_out row of an image: its own roll and pitch; the group's f / cx / cy / xi (the same bits in every row of the group) and what derives from
 * them; its own RMS_*, COST and VALID_PIXELS; the group's ITERATIONS and CONVERGED.  The group's cost is the sum of its rows' COST.
 * All images of a group must have one size (rel_focal is relative to the height); sizes may differ between groups.  Argument checks
 * (PF_ERR_ARG before any device work): those of pf_fit_camera, model, the group sizes and their sum, one size per group.
 * pf_fit_camera_shared_workspace_bytes is 0 for batch <= 0, a size below 8, a model outside {0, 1} or bad group sizes.
 * Enqueues per iteration (max_iter + 1 of them) one (accumulate, reduce) launch pair per 32 images and one solve launch per 128 groups on
 * `stream`, no host synchronisation, no atomics; a group's bits depend on its own images only, not on its place in the batch. */
size_t pf_fit_camera_shared_workspace_bytes(int model, int batch, const int32_t* h_hw, int n_groups, const int32_t* h_group_sizes);
int pf_fit_camera_shared(int device, int model, int batch, const int32_t* h_hw, const float* const* h_up, const float* const* h_lat, int n_groups,
                         const int32_t* h_group_sizes, const float* d_init, int free_pp, int loss, float huber_delta_deg, float w_up, float w_lat,
                         int max_iter, float* d_out, void* d_workspace, size_t workspace_bytes, void* stream);

/* The forward direction of that model: d_cam6 = {roll, pitch (RADIANS), rel_focal, rel_cx, rel_cy, xi} in device memory -> d_up [2][H][W],
 * d_lat [H][W] degrees; NaN where a point has no ray (xi > 1).  xi == 0 gives the bits of pf_fields_from_params; otherwise pf_pano_crop's
 * label formulas.  xi is read on the device, so a fitted xi feeds it without a host round trip.  Stateless, no handle. */
int pf_fields_from_params_usm(int device, const float* d_cam6, int H, int W, float* d_up, float* d_lat, void* stream);

/* Equirectangular panoramas -> camera views and their ground-truth perspective fields on the device: the reference's labelled-data
 * tooling, PanoCam.get_image / crop_equi (utils/panocam.py:132-249), crop_distortion (:558-752, Unified Spherical Model) and
 * get_up_general / get_lat_general (:451-556).  DESIGN.md section 11.
 * Per crop theta = d_cam7 row = {roll r, pitch p, yaw psi (RADIANS), rel_focal f, rel_cx cx, rel_cy cy, xi}, DEVICE [batch][7]; xi = 0: pinhole.
 * Every crop is H x W (>= 1 each).  Model:
 *   intrinsics  F = f*H, Cx = (cx + 1/2)*W, Cy = (cy + 1/2)*H; image point (a, b) -> x = (a - Cx)/F, y = (b - Cy)/F
 *   ray         rho^2 = x^2 + y^2, disc = 1 + (1 - xi^2) rho^2, eta = (xi + sqrt(disc)) / (1 + rho^2), X = (eta x, eta y, eta - xi), |X| = 1;
 *               disc < 0 (only for xi > 1): the pixel has no ray
 *   world       X_w = R X, R = R_pitch(p) R_roll(r), R_roll = [[cos r, -sin r, 0], [sin r, cos r, 0], [0, 0, 1]],
 *               R_pitch = [[1, 0, 0], [0, cos p, -sin p], [0, sin p, cos p]] (pf_fields_from_params' rotation: x right, y down, z forward,
 *               world up = (0, -1, 0), positive pitch looks up)
 *   sphere      lat = -atan2(X_w.y, hypot(X_w.x, X_w.z)), lon = yaw + atan2(X_w.x, X_w.z) wrapped into [-pi, pi) (positive yaw turns the view
 *               towards higher panorama columns)
 *   panorama    Hp x Wp (each >= 2), pixel centres at integers: u = (lon/2pi + 1/2) Wp - 1/2, v = (1/2 - lat/pi) Hp - 1/2 (row 0 = north,
 *               lon = 0 at the centre column); bilinear, columns wrap modulo Wp, rows clamp to [0, Hp - 1]
 *   image       sampled at (a, b) = (col + 1/2, row + 1/2); PF_PANO_U8: the fp32 value rounded half up, clamped to [0, 255]; PF_PANO_F32: the
 *               value; no ray: 0
 *   labels      (layout of pred_gravity_original / pred_latitude_original; yaw does not enter; no ray: NaN)
 *               xi = 0: bit-identical to pf_fields_from_params with the same (r, p, f, cx, cy)
 *               otherwise up at (col + 1/2, row + 1/2): g = R^T (0, -1, 0), D = X_z + xi, s = g_z + xi (X . g),
 *               up ~ (g_x D - X_x s, g_y D - X_y s) normalised; lat in degrees at the linspace point (col W/(W-1), row H/(H-1)) (0 for a size of 1)
 * h_pano = HOST array of n_pano DEVICE pointers, (Hp, Wp, 3) channel-interleaved, all of type `dtype`; h_pano_hw = HOST [n_pano][2] (Hp, Wp);
 * h_pano_index = HOST [batch], the panorama of each crop.  d_img = DEVICE [batch][H][W][3] of `dtype` (required); d_up [batch][2][H][W] and
 * d_lat [batch][H][W] fp32: both or neither (NULL: no labels).  Argument errors return PF_ERR_ARG before any device work.
 * One launch per 32 crops on `stream`, no host synchronisation; stateless, no handle; deterministic, each crop's bits independent of the batch. */
#define PF_PANO_U8 0
#define PF_PANO_F32 1
int pf_pano_crop(int device, int n_pano, const void* const* h_pano, const int32_t* h_pano_hw /*[n_pano][2]*/, int dtype, int batch,
                 const int32_t* h_pano_index /*[batch]*/, const float* d_cam7 /*[batch][7]*/, int H, int W,
                 void* d_img /*[batch][H][W][3], dtype*/, float* d_up /*[batch][2][H][W]*/, float* d_lat /*[batch][H][W]*/, void* stream);

/* The image of one camera re-projected into another camera of the same centre, on the device: upright rectification (roll, or roll and
 * pitch, removed), undistortion of a Unified Spherical Model view (xi -> 0), a change of focal length, principal point or output size, or
 * any other camera of the same centre (reproject.hip).
 * Per output, two cameras theta = {roll r, pitch p, yaw psi (RADIANS), rel_focal f, rel_cx cx, rel_cy cy, xi}: the source's row of d_cam_src7 and
 * the destination's row of d_cam_dst7, DEVICE [batch][7] each.  Intrinsics, ray and rotation are pf_pano_crop's: F = f*H, Cx = (cx + 1/2)*W,
 * Cy = (cy + 1/2)*H (of the camera's own image: H x W for the destination, Hs x Ws for the source), R = R_pitch(p) R_roll(r), camera -> world.
 * Yaw is a turn about the world's vertical, Y(psi) = [[cos psi, 0, sin psi], [0, 1, 0], [-sin psi, 0, cos psi]], so that
 * atan2(x', z') = atan2(x, z) + psi: pf_pano_crop's longitude.  For destination pixel (row, col):
 *   1 ray       (a, b) = (col + 1/2, row + 1/2), x = (a - Cx_d)/F_d, y = (b - Cy_d)/F_d, X_d = pf_pano_crop's ray of (x, y, xi_d); disc < 0 (only for
 *               xi_d > 1): the pixel has no ray and is invalid
 *   2 source    X_s = M X_d, M = R_s^T Y(psi_d - psi_s) R_d, computed once per output on the device
 *   3 visible   iff X_s.z > z_min(xi_s), z_min = -xi_s for xi_s <= 1 (0 for the pinhole camera), -1/xi_s for xi_s > 1: exactly the rays that the
 *               ray formula's "+" root gives, so project o unproject is the identity on them
 *   4 point     D = X_s.z + xi_s |X_s|, a_s = F_s X_s.x / D + Cx_s, b_s = F_s X_s.y / D + Cy_s; pixel-edge coordinates, a pixel centre at integer + 1/2
 *   5 inside    valid iff visible and 0 <= a_s <= Ws and 0 <= b_s <= Hs
 *   6 sample    bilinear at (u, v) = (a_s - 1/2, b_s - 1/2), the four tap indices clamped to [0, Ws - 1] x [0, Hs - 1]: the outer half-pixel rim
 *               replicates the edge
 *   7 value     PF_PANO_U8: the fp32 value rounded half up, clamped to [0, 255]; PF_PANO_F32: the value.  Invalid: `fill` (converted like a
 *               value) in the image, 0 in the mask
 * Every comparison is a positive one: NaN or infinite coordinates (non-finite parameters) make a pixel invalid, and no load is issued for it.
 * No antialiasing and no mip levels: a strong minification aliases.
 * h_src = HOST array of n_src DEVICE pointers, (Hs, Ws, 3) channel-interleaved, all of type `dtype` (PF_PANO_U8 | PF_PANO_F32); h_src_hw = HOST
 * [n_src][2] (Hs, Ws), each >= 1; h_src_index = HOST [batch], the source of each output.  Every output is H x W (>= 1 each).
 * d_img = DEVICE [batch][H][W][3] of `dtype` (required); d_valid = DEVICE [batch][H][W] uint8, 1 where valid, or NULL; d_map = DEVICE
 * [batch][2][H][W] fp32, (a_s, b_s), NaN where not visible (finite where visible but outside the source), or NULL.
 * Argument errors (NULL pointers, n_src < 1, a source size < 1, an index out of range, a bad dtype, H or W < 1, batch < 1) return PF_ERR_ARG
 * before any device work.  One launch per 32 outputs on `stream`, no host synchronisation; stateless, no handle; deterministic, each output's
 * bits independent of the batch it is in. */
int pf_reproject(int device, int n_src, const void* const* h_src, const int32_t* h_src_hw /*[n_src][2]*/, int dtype /*PF_PANO_U8|PF_PANO_F32*/,
                 int batch, const int32_t* h_src_index /*[batch]*/, const float* d_cam_src7 /*[batch][7]*/, const float* d_cam_dst7 /*[batch][7]*/,
                 int H, int W, float fill, void* d_img, uint8_t* d_valid /*or NULL*/, float* d_map /*or NULL*/, void* stream);

/* Camera views of one centre composed into equirectangular panoramas on the device: the inverse direction of pf_pano_crop, several views
 * blended per panorama pixel (pano_compose.hip).
 * Per view theta = d_cam7 row = {roll r, pitch p, yaw psi (RADIANS), rel_focal f, rel_cx cx, rel_cy cy, xi}, exactly as in pf_reproject: F = f*Hs,
 * Cx = (cx + 1/2)*Ws, Cy = (cy + 1/2)*Hs of the view's own image Hs x Ws, R = R_pitch(p) R_roll(r) camera -> world, and the yaw turn Y(psi).
 * For pixel (row, col) of an Hp x Wp panorama (the inverse of pf_pano_crop's step from ray to pixel):
 *   lon = ((col + 1/2)/Wp - 1/2) 2 pi, lat = (1/2 - (row + 1/2)/Hp) pi, D = (cos lat sin lon, -sin lat, cos lat cos lon)
 * and for each view i of that panorama, in the caller's order:
 *   1 ray       X = M_i D, M_i = R_i^T Y(-psi_i), computed once per view on the device
 *   2 visible   iff X.z > z_min(xi_i) (pf_reproject's step 3)
 *   3 point     (a, b) = F_i (X.x, X.y) / (X.z + xi_i |X|) + (Cx_i, Cy_i), pixel-edge units
 *   4 covered   d = min(a, Ws_i - a, b, Hs_i - b); the view covers the pixel iff it is visible and d > 0, a positive comparison: a NaN or
 *               infinite coordinate (non-finite parameters) covers nothing and issues no load
 *   5 weight    blend = PF_BLEND_FEATHER: w_i = min(2 d / min(Hs_i, Ws_i), 1), 0 on the view's border and 1 in the middle of its short side;
 *               blend = PF_BLEND_MEAN: w_i = 1
 *   6 colour    c_i = bilinear at (a - 1/2, b - 1/2), the four taps clamped into the view (pf_reproject's step 6)
 * S = sum w_i and C = sum w_i c_i, accumulated in fp32 in view order.  The pixel is C / S where S > 0, else `fill`; PF_PANO_U8: rounded half up and
 * clamped to [0, 255] (`fill` converted like a value).  d_weight, when given, holds S (0 for an uncovered pixel).
 * The feather weight falls to 0 at a view's border, so the composite is continuous across view borders; MEAN with one view is the bilinear sample.
 * Each output value depends on its own panorama's views, their order and the options only: the same bits in any batch and on every run; a view
 * with non-finite parameters contributes nothing and leaves every other bit unchanged.  No antialiasing: a strongly minified view aliases.
 * h_view = HOST array of n_view DEVICE pointers, (Hs, Ws, 3) channel-interleaved, all of type `dtype`; h_view_hw = HOST [n_view][2] (Hs, Ws), each
 * >= 1; h_view_pano = HOST [n_view], the panorama of each view, non-decreasing, in [0, n_pano) (a panorama without views is all `fill`, weight 0).
 * d_pano = DEVICE [n_pano][Hp][Wp][3] of `dtype` (required); d_weight = DEVICE [n_pano][Hp][Wp] fp32 or NULL; d_acc = DEVICE [n_pano][Hp][Wp][4]
 * fp32 workspace, 16-byte aligned, needed only when a panorama has more than 32 views (its partial (C, S) travel through it between launches).
 * Argument errors (NULL required pointers, n_view < 1, n_pano < 1, a view side < 1, Hp or Wp < 1, a bad dtype or blend, an index out of range or
 * decreasing, d_acc missing when it is needed) return PF_ERR_ARG before any device work.  Panoramas share launches of at most 32 views and 32
 * panoramas; a panorama of n > 32 views takes ceil(n / 32) launches of its own.  All on `stream`, no host synchronisation; stateless, no handle. */
#define PF_BLEND_FEATHER 0
#define PF_BLEND_MEAN 1
int pf_pano_compose(int device, int n_view, const void* const* h_view, const int32_t* h_view_hw /*[n_view][2]*/, int dtype,
                    const int32_t* h_view_pano /*[n_view], non-decreasing, in [0, n_pano)*/, const float* d_cam7 /*[n_view][7]*/,
                    int n_pano, int Hp, int Wp, int blend /*PF_BLEND_FEATHER|PF_BLEND_MEAN*/, float fill,
                    void* d_pano /*[n_pano][Hp][Wp][3]*/, float* d_weight /*[n_pano][Hp][Wp] or NULL*/,
                    float* d_acc /*[n_pano][Hp][Wp][4] fp32 workspace; may be NULL unless a panorama has more than 32 views*/, void* stream);

/* Perspective fields transported between cameras of one centre, and from camera views onto equirectangular panoramas, on the device: the field
 * counterparts of pf_reproject and pf_pano_compose (field_transport.hip).  Latitude is a property of the ray, so it is
 * resampled.  An up vector is a tangent direction: it is lifted from the source's image plane to the sphere, rotated, and pushed to the destination's
 * image plane through the differential of (unproject, rotate, project), in closed form for the Unified Spherical Model and the equirectangular
 * projection (field_transport.h, no finite differences).  Gravity does not enter: the transport needs the relative rotation only, so predicted
 * fields move exactly as labels do.
 *   usm_push(X, t, xi)   the image direction of the tangent t at the ray X (any length): (t.x D - X.x s, t.y D - X.y s), D = X.z + xi |X|,
 *                        s = t.z + xi (X . t) / |X|
 *   usm_lift(X, m, xi)   the unit tangent t, t . X = 0, with usm_push(X, t, xi) a positive multiple of m: e1 = normalise(X x h), h = (1, 0, 0) where
 *                        |X.x| < 0.9 |X|, else (0, 1, 0), e2 = (X / |X|) x e1; the 2 x 2 system alpha push(e1) + beta push(e2) = m by Cramer's rule
 * Taps.  A sample at (u, v) in index units reads (floor v + {0, 1}, floor u + {0, 1}) with the bilinear weights.  A tap counts when it is inside the
 * array and valid by pf_place_scores' rule (finite latitude, 1e-12 <= |up|^2 < inf); taps are NOT clamped.  W = the sum of the weights that count;
 * sums in tap order in fp32.  Latitude lives on linspace(-c, size - c, size) (pf_fields_from_params' quirk): index j of a side of n sits at
 * pixel-edge coordinate j n / (n - 1), so every side of a field, source or output of pf_reproject_fields, is >= 2.
 *
 * pf_reproject_fields: one source per output, batched like pf_reproject; cameras = rows of d_cam_src7 / d_cam_dst7 as there (RADIANS).  For
 * destination pixel (row, col):
 *   up    steps 1 to 5 of pf_reproject at (col + 1/2, row + 1/2): X_d, X_s = M X_d, (a_s, b_s), valid.  Taps at (a_s - 1/2, b_s - 1/2): W_u and
 *         m = sum w_k u_k.  Valid iff step 5, W_u >= 1/2 and |m|^2 >= 1e-12.  t = usm_lift(X_s, m, xi_s); up' = normalise(usm_push(X_d, M^T t, xi_d))
 *   lat   the same steps for the destination point (col W / (W - 1), row H / (H - 1)); taps at the source index (a_s (Ws - 1) / Ws,
 *         b_s (Hs - 1) / Hs): W_l.  Valid iff step 5 and W_l >= 1/2.  lat' = sum w_k lat_k / W_l
 * The pixel is written iff both parts are valid, else NaN x 3.  A non-finite camera parameter makes every pixel of that output NaN.
 * h_src_up / h_src_lat = HOST arrays of n_src DEVICE pointers, fp32 planes [2][Hs][Ws] and [Hs][Ws]; h_src_hw = HOST [n_src][2]; h_src_index = HOST
 * [batch].  d_up = DEVICE [batch][2][H][W], d_lat = DEVICE [batch][H][W], fp32, both required.
 * Argument errors, in this order: no sources; a NULL field pointer; a source side < 2; batch < 1 or a NULL required pointer; H or W < 2; an index
 * out of range; return PF_ERR_ARG before any device work with a message that begins "pf_reproject_fields".  One launch per 32 outputs on `stream`.
 *
 * pf_compose_fields: several views blended per panorama pixel; h_view_pano, d_cam7, n_pano, Hp, Wp, blend, d_weight as in pf_pano_compose.  For
 * panorama pixel (row, col), D, lon, lat as there, and for view i of that panorama in the caller's order:
 *   geometry   steps 1 to 5 of pf_pano_compose: X = M_i D, visible, (a, b), covered iff d > 0, weight w_i
 *   taps       up at (a - 1/2, b - 1/2): W_u, m; latitude at the view's index (a (Ws - 1) / Ws, b (Hs - 1) / Hs): W_l, lat_i = sum w_k lat_k / W_l.
 *              The panorama's own latitude grid is its pixel centres (pf_pano_fields)
 *   up         t = M_i^T usm_lift(X, m, xi_i); p = (Wp / (2 pi) (t . e_lon) / cos lat, -Hp / pi (t . e_lat)), e_lon and e_lat of pf_pano_fields;
 *              u_i = p / |p|
 *   counts     iff covered, W_u >= 1/2, W_l >= 1/2, |m|^2 >= 1e-12 and 1e-12 <= |p|^2 < inf
 * S = sum w_i, L = sum w_i lat_i, U = sum w_i u_i in fp32 in view order.  lat = L / S and up = U / |U| where S > 0 and |U|^2 >= 1e-12, else NaN x 3;
 * d_weight, when given, holds S.  A view with a non-finite parameter contributes nothing and leaves every other bit unchanged.
 * At most PF_COMPOSE_FIELDS_MAX_VIEWS views per panorama: more is PF_ERR_ARG (there is no accumulator path).  View sides >= 2; Hp, Wp >= 1.
 * Argument errors, in this order: no views; a bad blend; a NULL field pointer; a view side < 2; n_pano < 1 or a NULL required pointer; Hp or Wp < 1;
 * an index out of range or decreasing; more than 32 views of one panorama; return PF_ERR_ARG before any device work with a message that begins
 * "pf_compose_fields".  Panoramas share launches of at most 32 views and 32 panoramas, on `stream`.
 * Both: every comparison is a positive one, so NaN or infinite coordinates issue no load; no host synchronisation; stateless, no handle;
 * deterministic, each output's bits independent of the batch it is in. */
#define PF_COMPOSE_FIELDS_MAX_VIEWS 32
int pf_reproject_fields(int device, int n_src, const float* const* h_src_up, const float* const* h_src_lat, const int32_t* h_src_hw /*[n_src][2]*/,
                        int batch, const int32_t* h_src_index /*[batch]*/, const float* d_cam_src7 /*[batch][7]*/, const float* d_cam_dst7 /*[batch][7]*/,
                        int H, int W, float* d_up /*[batch][2][H][W]*/, float* d_lat /*[batch][H][W]*/, void* stream);
int pf_compose_fields(int device, int n_view, const float* const* h_view_up, const float* const* h_view_lat, const int32_t* h_view_hw /*[n_view][2]*/,
                      const int32_t* h_view_pano /*[n_view], non-decreasing, in [0, n_pano)*/, const float* d_cam7 /*[n_view][7]*/, int n_pano, int Hp,
                      int Wp, int blend /*PF_BLEND_FEATHER|PF_BLEND_MEAN*/, float* d_up /*[n_pano][2][Hp][Wp]*/, float* d_lat /*[n_pano][Hp][Wp]*/,
                      float* d_weight /*[n_pano][Hp][Wp] or NULL*/, void* stream);

/* Equirectangular panoramas rotated into equirectangular panoramas on the device, with the perspective fields of the panoramic camera:
 * levelling a tilted panorama, tilting an upright one (labelled data), re-centring a composite (pano_rotate.hip).
 * Conventions of pf_pano_crop and pf_pano_compose: x right, y down, z forward, world up = (0, -1, 0), R(r, p) = R_pitch(p) R_roll(r) camera ->
 * world, Y(psi) = [[cos psi, 0, sin psi], [0, 1, 0], [-sin psi, 0, cos psi]] the turn about y that adds psi to the longitude.
 * Per output theta = d_rot3 row = {roll r, pitch p, yaw psi} (RADIANS), DEVICE [batch][3], and one flag `inverse` per call:
 *   Q = Y(psi) R(r, p), A = Q, or Q^T with inverse != 0.
 * For pixel (row, col) of an H x W output (pf_pano_compose's direction of a panorama pixel):
 *   lon = ((col + 1/2)/W - 1/2) 2 pi, lat = (1/2 - (row + 1/2)/H) pi, D = (cos lat sin lon, -sin lat, cos lat cos lon)
 *   1 source    X = A D; lat_s = -atan2(X.y, hypot(X.x, X.z)), lon_s = atan2(X.x, X.z); u = (lon_s/2pi + 1/2) Ws - 1/2, v = (1/2 - lat_s/pi) Hs - 1/2
 *               of the source Hs x Ws (each >= 2), pixel centres at integers
 *   2 image     bilinear at (u, v), columns wrap modulo Ws, rows clamp to [0, Hs - 1] (pf_pano_crop's sampling); PF_PANO_U8: the fp32 value
 *               rounded half up, clamped to [0, 255]; PF_PANO_F32: the value
 *               inverse = 0: what a panoramic camera with orientation (r, p, psi) inside an upright source sees;
 *               inverse != 0: a source shot by such a camera becomes the upright panorama (levelling)
 *   3 labels    the perspective fields of a panoramic camera whose camera -> world rotation is A (layout of pred_gravity_original /
 *               pred_latitude_original): latitude = lat_s in degrees, at the pixel centre; up = the image direction of a step along world up:
 *               g = A^T (0, -1, 0), t = g - (g . D) D, e_lon = (cos lon, 0, -sin lon), e_lat = (-sin lat sin lon, -cos lat, -sin lat cos lon),
 *               up ~ (W/(2 pi) (t . e_lon) / cos lat, -H/pi (t . e_lat)) normalised; |t|^2 = (t . e_lon)^2 + (t . e_lat)^2 < PF_PANO_UP_MIN_T2 (a
 *               pixel centre on the zenith or nadir of the world): up = NaN, the latitude stays
 * Non-finite r, p or psi: the output's image is 0 and its labels NaN, and no load is issued for it (pf_pano_crop's rule for a pixel without
 * a ray); every other output keeps its bits.  No antialiasing: a strong minification aliases.
 * pf_pano_rotate: h_pano = HOST array of n_pano DEVICE pointers, (Hs, Ws, 3) channel-interleaved, all of type `dtype`; h_pano_hw = HOST
 * [n_pano][2] (Hs, Ws); h_pano_index = HOST [batch], the source of each output.  d_img = DEVICE [batch][H][W][3] of `dtype` (required); d_up
 * [batch][2][H][W] and d_lat [batch][H][W] fp32: both or neither (NULL: no labels).  pf_pano_fields: the labels alone, no source; its bits
 * are those of pf_pano_rotate's labels for the same d_rot3 row, inverse, H and W.
 * Argument errors (NULL required pointers, n_pano < 1, batch < 1, a source side < 2, H or W < 1, a bad dtype, an index out of range, one of
 * d_up / d_lat alone) return PF_ERR_ARG before any device work.  One launch per 32 outputs on `stream`, no host synchronisation; stateless, no
 * handle; deterministic, each output's bits independent of the batch it is in. */
#define PF_PANO_UP_MIN_T2 1e-10f
int pf_pano_rotate(int device, int n_pano, const void* const* h_pano, const int32_t* h_pano_hw /*[n_pano][2]*/, int dtype, int batch,
                   const int32_t* h_pano_index /*[batch]*/, const float* d_rot3 /*[batch][3] roll, pitch, yaw, radians*/, int inverse, int H, int W,
                   void* d_img /*[batch][H][W][3], dtype*/, float* d_up /*[batch][2][H][W]*/, float* d_lat /*[batch][H][W]*/, void* stream);
int pf_pano_fields(int device, int batch, const float* d_rot3 /*[batch][3]*/, int inverse, int H, int W, float* d_up /*[batch][2][H][W]*/,
                   float* d_lat /*[batch][H][W]*/, void* stream);

/* Antialiased forms of pf_pano_crop, pf_reproject and pf_pano_rotate by supersampling (gather_ss.hip): the argument list of the
 * parent with `samples` = S, an integer in 1 ... PF_GATHER_MAX_SAMPLES, before `stream`.  Every output pixel is the mean of S x S sub-samples, and
 * each sub-sample is the parent's per-sample model, unchanged:
 *   point       sub-sample (i, j), i, j in [0, S), of output pixel (row, col) sits at (a, b) = (col + (j + 1/2)/S, row + (i + 1/2)/S), which replaces
 *               (col + 1/2, row + 1/2) in the parent's model (for pf_pano_rotate: in lon and lat).  Ray, validity, source coordinate, tap rule and
 *               blend order stay the parent's.  Because F = f*H and Cx = (cx + 1/2)*W scale with the size, sub-sample (i, j) of pixel (row, col) is
 *               the pixel centre (S row + i, S col + j) of the same call at the output size (S H, S W): the S x S block mean of that call
 *   image       the fp32 sum of the valid sub-samples' bilinear values, i-major then j, divided by their count n as sum / (float)n; S = 1 gives the
 *               parent's bits.  PF_PANO_U8: that value rounded half up, clamped to [0, 255].  A sub-sample is valid where the parent's pixel is: it
 *               has a ray (pf_pano_crop), it is valid in pf_reproject's step 5, always for pf_pano_rotate with finite angles
 *   empty       a pixel with no valid sub-sample is 0 for pf_pano_crop_ss and pf_pano_rotate_ss, `fill` for pf_reproject_ss.  Non-finite parameters
 *               behave as in the parent: 0 or `fill`, NaN labels, no load issued
 *   mask        pf_reproject_ss: 1 iff at least one sub-sample is valid, so mask = 0 <=> the pixel holds `fill`
 *   map         pf_reproject_ss: the pixel centre's (a_s, b_s), the bits of pf_reproject.  With an even S the centre is not itself a sub-sample, so
 *               the map may be finite and inside the source where the mask is 0, and the other way round, next to a border
 *   labels      pf_pano_crop_ss, pf_pano_rotate_ss: bit-identical to the parent's.  They describe the pixel, not its footprint
 * S <= 4 with bilinear taps covers minifications up to about 8x.  Sizes, pointers, the parent's argument checks and launches are the parent's;
 * `samples` outside 1 ... PF_GATHER_MAX_SAMPLES returns PF_ERR_ARG before any device work, with a message that begins with the function's name and
 * names `samples`.  Deterministic, each output's bits independent of the batch it is in.  pf_pano_compose and pf_yaw_moments (several views per
 * pixel, weights of their own) have no such form. */
#define PF_GATHER_MAX_SAMPLES 4
int pf_pano_crop_ss(int device, int n_pano, const void* const* h_pano, const int32_t* h_pano_hw /*[n_pano][2]*/, int dtype, int batch,
                    const int32_t* h_pano_index /*[batch]*/, const float* d_cam7 /*[batch][7]*/, int H, int W,
                    void* d_img /*[batch][H][W][3], dtype*/, float* d_up /*[batch][2][H][W]*/, float* d_lat /*[batch][H][W]*/, int samples, void* stream);
int pf_reproject_ss(int device, int n_src, const void* const* h_src, const int32_t* h_src_hw /*[n_src][2]*/, int dtype /*PF_PANO_U8|PF_PANO_F32*/,
                    int batch, const int32_t* h_src_index /*[batch]*/, const float* d_cam_src7 /*[batch][7]*/, const float* d_cam_dst7 /*[batch][7]*/,
                    int H, int W, float fill, void* d_img, uint8_t* d_valid /*or NULL*/, float* d_map /*or NULL*/, int samples, void* stream);
int pf_pano_rotate_ss(int device, int n_pano, const void* const* h_pano, const int32_t* h_pano_hw /*[n_pano][2]*/, int dtype, int batch,
                      const int32_t* h_pano_index /*[batch]*/, const float* d_rot3 /*[batch][3] roll, pitch, yaw, radians*/, int inverse, int H, int W,
                      void* d_img /*[batch][H][W][3], dtype*/, float* d_up /*[batch][2][H][W]*/, float* d_lat /*[batch][H][W]*/, int samples, void* stream);

/* Cube maps as a source: camera views and equirectangular panoramas out of six faces on the device (cube_gather.hip).
 * THE CUBE-MAP CONVENTION.  A cube map is (6, N, N, 3), uint8 or fp32, channel-interleaved, N >= 1.  Face k is the picture of a pf_pano_crop pinhole
 * camera with roll 0, rel_focal 1/2 (90 degrees), rel_cx = rel_cy = 0, xi = 0 and the (pitch, yaw) below, in the panorama's world frame (x right,
 * y down, z towards longitude 0); its frame (right r, down d, forward n) is the columns of Y(yaw) R(0, pitch), an exact signed permutation:
 *   k  name   pitch  yaw   r   d   n          k  name   pitch  yaw   r   d   n
 *   0  front    0      0   +x  +y  +z         3  left     0    270   +z  +y  -x
 *   1  right    0     90   -z  +y  +x         4  up     +90      0   +x  +z  -y
 *   2  back     0    180   -x  +y  -z         5  down   -90      0   +x  -z  +y
 * Texel (row, col) of face k has the direction n + a r + b d with a = 2 (col + 1/2) / N - 1, b = 2 (row + 1/2) / N - 1.
 * The value of the cube in a direction X:
 *   1 face      by the major axis: |z| >= |x| and |z| >= |y|: front (z >= 0) or back; else |x| >= |y|: right (x > 0) or left; else up (y < 0) or down
 *   2 point     a = (X . r) / (X . n), b = (X . d) / (X . n); u = (a + 1) N / 2 - 1/2, v = (b + 1) N / 2 - 1/2, both in [-1/2, N - 1/2]
 *   3 taps      rows (floor v, floor v + 1) x columns (floor u, floor u + 1), indices in [-1, N]; the indices -1 and N are the RING of the face
 *   4 ring      a tap beyond the edge in face direction e in {+r, -r, +d, -d}, at the in-face coordinate t along the other axis o, is the texel of
 *               the neighbouring face whose centre direction is e + (1 - 1/N) n + t o: the neighbour unfolded flat around the shared edge, the same
 *               position along the edge, the first row or column inwards.  That is always a texel centre of the face whose forward axis is e
 *   5 corner    a tap in the ring on both indices has no texel; its value is (T0 + Ta + Tb) * (1/3) in fp32, not rounded to the source's type: T0 the
 *               face's own corner texel, Ta the ring texel beside it across the column edge, Tb across the row edge, summed in that order
 *   6 blend     bilinear, the order of operations of the other gathers: top = (1 - fu) t00 + fu t01, bot likewise, (1 - fv) top + fv bot
 * This sampler is continuous over the whole sphere, the 12 edges and 8 corners included: a view that straddles an edge has no seam, which a
 * per-face clamped sampler leaves.  It is not the panorama's bilinear surface: next to an edge the flat unfolding misplaces a ring texel by up to
 * 1/N of a face along the edge.
 * pf_cube_crop: views of cameras theta = d_cam7 row = {roll, pitch, yaw (RADIANS), rel_focal, rel_cx, rel_cy, xi}: the ray of pf_pano_crop's pixel
 * (pinhole or Unified Spherical Model), X = Y(yaw) R(roll, pitch) ray, the cube's value in X.  A pixel without a ray is 0.  A non-finite
 * parameter: the view is 0 and no load is issued for it.
 * pf_cube_to_pano: equirectangular panoramas; pixel -> direction D and the rotation A = Q or Q^T of pf_pano_rotate (d_rot3, inverse), X = A D,
 * the cube's value in X: a tilted cube map is levelled into a panorama in one pass.  Non-finite angles: the output is 0, no load.
 * Both: `samples` = S in 1 ... PF_GATHER_MAX_SAMPLES under the rule of the supersampled gathers above: every pixel is the mean of the S x S
 * sub-samples at (col + (j + 1/2)/S, row + (i + 1/2)/S) that are valid (pf_cube_crop: that have a ray), the fp32 sum i-major then j divided by
 * their count, 0 without one; S = 1 is the pixel centre.  PF_PANO_U8: the fp32 value rounded half up, clamped to [0, 255].  There are no labels:
 * the fields of a view or of a panoramic camera do not depend on the source (pf_fields_from_params, pf_pano_fields).
 * h_cube = HOST array of n_cube DEVICE pointers to (6, N, N, 3) of type `dtype`; h_cube_hw = HOST [n_cube][2] (N, N), N >= 1; h_cube_index = HOST
 * [batch], the cube of each output.  d_img = DEVICE [batch][H][W][3] of `dtype`.  Argument errors (`samples` out of range, faces that are not
 * square, NULL required pointers, n_cube < 1, batch < 1, N < 1, H or W < 1, a bad dtype, an index out of range) return PF_ERR_ARG before any
 * device work with a message that begins with the function's name.  One launch per 32 outputs on `stream`, no workspace, no host
 * synchronisation; stateless, no handle; deterministic, each output's bits independent of the batch it is in. */
int pf_cube_crop(int device, int n_cube, const void* const* h_cube, const int32_t* h_cube_hw /*[n_cube][2]*/, int dtype /*PF_PANO_U8|PF_PANO_F32*/,
                 int batch, const int32_t* h_cube_index /*[batch]*/, const float* d_cam7 /*[batch][7]*/, int H, int W,
                 void* d_img /*[batch][H][W][3], dtype*/, int samples, void* stream);
int pf_cube_to_pano(int device, int n_cube, const void* const* h_cube, const int32_t* h_cube_hw /*[n_cube][2]*/, int dtype, int batch,
                    const int32_t* h_cube_index /*[batch]*/, const float* d_rot3 /*[batch][3] roll, pitch, yaw, radians*/, int inverse, int H, int W,
                    void* d_img /*[batch][H][W][3], dtype*/, int samples, void* stream);

/* Fisheye and dual-fisheye frames as a source: camera views and equirectangular panoramas out of one or two lenses of a frame on the device
 * (fisheye_gather.hip).
 * THE LENS MODEL.  Conventions are pf_pano_crop's and pf_cube_crop's: x right, y down, z forward, world up (0, -1, 0); R(r, p) = R_pitch R_roll, Y(psi)
 * the turn about y; pixel-edge image coordinates, a texel centre at integer + 1/2.  A FRAME is (Hs, Ws, 3), uint8 or fp32, channel-interleaved,
 * Hs, Ws >= 1, and carries up to PF_FISHEYE_MAX_LENSES = 2 LENSES.  A lens is PF_FISHEYE_LENS_FLOATS = 12 fp32 values in this order:
 *   {roll, pitch, yaw (RADIANS), F, Cx, Cy, theta_max, k1, k2, k3, k4, band}
 * Q = Y(yaw) R(roll, pitch) is the lens -> world rotation; F is in pixels per unit of rho; (Cx, Cy) is the centre of the image circle in pixel-edge
 * units of the frame; theta_max is the half field of view in radians, up to pi; band >= 0 is the feather width in radians.  The projection kind is
 * one integer per call: PF_FISHEYE_EQUIDISTANT rho(t) = t, PF_FISHEYE_EQUISOLID rho(t) = 2 sin(t / 2), PF_FISHEYE_STEREOGRAPHIC rho(t) = 2 tan(t / 2);
 * k1 ... k4 are the Kannala-Brandt polynomial (OpenCV's fisheye model is the equidistant kind with F = f).  These two entry points use only the forward
 * projection (direction -> pixel); the inverse is pf_pano_to_fisheye's, below.
 * The value of a frame in a unit world direction D, per lens l = 0, 1 in that order:
 *   1 angle     X = Ql^T D, h = hypot(X.x, X.y), theta = atan2(h, X.z)
 *   2 point     theta_d = theta (1 + theta^2 (k1 + theta^2 (k2 + theta^2 (k3 + theta^2 k4)))), Horner-wise as written; r = F rho(theta_d);
 *               (a, b) = (Cx, Cy) + r (X.x, X.y) / h, and (Cx, Cy) itself where h = 0
 *   3 covered   iff theta_max - theta > 0 and 0 <= a <= Ws and 0 <= b <= Hs.  Every comparison is a positive one: a lens with a non-finite entry or
 *               with theta_max <= 0 covers nothing and issues no load, which is also how an unused second lens is switched off
 *   4 weight    w = min((theta_max - theta) / band, 1) for band > 0, else 1
 *   5 colour    c = the bilinear sample of the other gathers at (a - 1/2, b - 1/2), taps clamped into the frame
 * Then S = sum of w and C = sum of w c, in fp32, in lens order; the direction is VALID iff S > 0 and its value is C / S.  For a dual-fisheye camera
 * `band` is the overlap of the two lenses (fov - 180 degrees): one lens fades out exactly where the other fades in.
 * pf_fisheye_crop: views of cameras theta = d_cam7 row = {roll, pitch, yaw (RADIANS), rel_focal, rel_cx, rel_cy, xi}: the ray of pf_pano_crop's pixel
 * (pinhole or Unified Spherical Model), D = Y(yaw) R(roll, pitch) ray as in pf_cube_crop, the frame's value in D.  A pixel without a ray or
 * without a covering lens is `fill`, and its mask is 0.
 * pf_fisheye_to_pano: equirectangular panoramas; pixel -> direction D0 and the rotation A = Q or Q^T of pf_pano_rotate (d_rot3, inverse), D = A D0,
 * the frame's value in D: a tilted rig is levelled into a panorama in one pass.
 * Both: `samples` = S in 1 ... PF_GATHER_MAX_SAMPLES under the rule of the supersampled gathers above: every pixel is the mean of the valid ones of
 * the S x S sub-samples at (col + (j + 1/2)/S, row + (i + 1/2)/S), each the blended value above: the fp32 sum i-major then j divided by their
 * count; `fill` without one; the mask is 1 iff a sub-sample is valid.  PF_PANO_U8: the fp32 value rounded half up, clamped to [0, 255].  A non-finite
 * camera or angle entry: the output is `fill`, its mask 0, and no load is issued for it.  There are no labels: the fields of a view or of a
 * panoramic camera do not depend on the source (pf_fields_from_params, pf_pano_fields).
 * h_frame = HOST array of n_frame DEVICE pointers to (Hs, Ws, 3) of type `dtype`; h_frame_hw = HOST [n_frame][2] (Hs, Ws); h_frame_index = HOST
 * [batch], the frame of each output; d_lens = DEVICE [batch][2][12], the two lenses of each output (of its frame); d_img = DEVICE
 * [batch][H][W][3] of `dtype`; d_valid = NULL or DEVICE [batch][H][W] bytes.  The 4-pixel vector stores are taken when W % 4 == 0 and d_img
 * (4 bytes uint8, 16 bytes fp32) and d_valid (4 bytes) are aligned; otherwise scalar stores give the same bits.  Argument errors return PF_ERR_ARG
 * before any device work with a message that begins with the function's name, checked in this order: `samples` out of range; an unknown `kind`;
 * then n_frame < 1 or NULL source lists, a bad dtype, a NULL frame or a frame side < 1, batch < 1 or a NULL required pointer (h_frame_index,
 * d_lens, d_cam7 / d_rot3, d_img), H or W < 1, an index out of range.  One launch per 32 outputs on `stream`, no workspace, no host
 * synchronisation; stateless, no handle; deterministic, each output's bits independent of the batch it is in. */
#define PF_FISHEYE_MAX_LENSES 2
#define PF_FISHEYE_LENS_FLOATS 12
#define PF_FISHEYE_EQUIDISTANT 0
#define PF_FISHEYE_EQUISOLID 1
#define PF_FISHEYE_STEREOGRAPHIC 2
int pf_fisheye_crop(int device, int n_frame, const void* const* h_frame, const int32_t* h_frame_hw /*[n_frame][2]*/, int dtype /*PF_PANO_U8|PF_PANO_F32*/,
                    int kind /*PF_FISHEYE_...*/, int batch, const int32_t* h_frame_index /*[batch]*/, const float* d_lens /*[batch][2][12]*/,
                    const float* d_cam7 /*[batch][7]*/, int H, int W, float fill, void* d_img /*[batch][H][W][3], dtype*/, uint8_t* d_valid /*or NULL*/,
                    int samples, void* stream);
int pf_fisheye_to_pano(int device, int n_frame, const void* const* h_frame, const int32_t* h_frame_hw /*[n_frame][2]*/, int dtype, int kind, int batch,
                       const int32_t* h_frame_index /*[batch]*/, const float* d_lens /*[batch][2][12]*/,
                       const float* d_rot3 /*[batch][3] roll, pitch, yaw, radians*/, int inverse, int H, int W, float fill,
                       void* d_img /*[batch][H][W][3], dtype*/, uint8_t* d_valid /*or NULL*/, int samples, void* stream);

/* Fisheye and dual-fisheye frames as a TARGET: equirectangular panoramas -> the frames of one or two lenses, with the perspective fields of the
 * fisheye camera (fisheye_target.hip).  Conventions and the 12-float lens row are those of pf_fisheye_crop above.
 * An OUTPUT is an H x W frame (H, W >= 1) with its two lens rows d_lens[batch][2][12]; the projection kind is one integer per call; the source is an
 * equirectangular panorama (Hp, Wp, 3), each side >= 2, in pf_pano_crop's longitude / latitude convention.
 * PER LENS (lane 0): Q = Y(yaw) R(roll, pitch); R = R_pitch R_roll; g = R^T (0, -1, 0), world up in the lens' coordinates; the lens is ON exactly as
 * above (its 12 entries finite and theta_max > 0); r_max = F rho(theta_d(theta_max)), the radius of its image circle, with theta_d and rho as above.
 * THE INVERSE PROJECTION at the image point (a, b), pixel-edge units, lens l = 0 first, then lens 1:
 *   1 radius    dx = a - Cx, dy = b - Cy, r = hypot(dx, dy)
 *   2 owner     the lens OWNS the point iff it is on and r_max - r > 0: a positive comparison, a NaN owns nothing.  The first owner wins: there is
 *               no blending in a target frame (`band` is not used).  fisheye_lens refuses a non-monotone r(theta), so r < r_max <=> theta <
 *               theta_max, the coverage of the source side
 *   3 theta_d   rho = r / F; theta_d = rho (equidistant) | 2 asin(min(rho / 2, 1)) (equisolid) | 2 atan(rho / 2) (stereographic)
 *   4 theta     theta = theta_d if k1 = ... = k4 = 0.  Otherwise from theta_0 = min(theta_d, theta_max) exactly PF_FISHEYE_NEWTON_STEPS = 10 steps
 *               theta <- clamp(theta - (P(theta) - theta_d) / P'(theta), 0, theta_max), with P(t) = t (1 + t^2 (k1 + t^2 (k2 + t^2 (k3 + t^2 k4))))
 *               Horner-wise as above and P'(t) = 1 + t^2 (3 k1 + t^2 (5 k2 + t^2 (7 k3 + 9 k4 t^2))): a fixed count, no data-dependent exit
 *   5 direction (c, s) = (dx, dy) / r, (1, 0) where r = 0; X = (sin theta c, sin theta s, cos theta) in the lens' coordinates
 * THE IMAGE: D = Q X; pf_pano_crop's sphere and panorama lines: lat = -atan2(D.y, hypot(D.x, D.z)), lon = atan2(D.x, D.z), u = (lon / 2 pi + 1/2) Wp
 * - 1/2, v = (1/2 - lat / pi) Hp - 1/2; the bilinear sample of the panorama gathers at (u, v) (columns wrap, rows clamp).  A point no lens owns has
 * no value.  `samples` = S in 1 ... PF_GATHER_MAX_SAMPLES under the rule of the supersampled gathers: a pixel is the mean of the valid ones of its
 * S x S sub-samples at (col + (j + 1/2)/S, row + (i + 1/2)/S), `fill` without one; the mask is 1 iff a sub-sample is valid.  PF_PANO_U8: the fp32
 * value rounded half up, clamped to [0, 255].  A lens row with a non-finite entry owns nothing and issues no load.
 * THE LABELS (the perspective fields of the fisheye camera) are taken at the pixel centre (col + 1/2, row + 1/2), whatever `samples`, and use R, not
 * Q: the yaw does not enter them, nor their bits.
 *   latitude    degrees: -atan2(W.y, hypot(W.x, W.z)) with W = R X
 *   up          the image direction of a step along world up.  t = g - (g . X) X; e_theta = (cos theta c, cos theta s, -sin theta), e_phi = (-s, c, 0)
 *               (t = (t . e_theta) e_theta + (t . e_phi) e_phi, and t . e = g . e for both); m = rho(theta_d) = r / F, m' = rho'(theta_d) P'(theta)
 *               with rho' = 1 | cos(theta_d / 2) | 1 / cos^2(theta_d / 2);
 *               up ~ m' (t . e_theta) (c, s) + (m / sin theta) (t . e_phi) (-s, c), normalised; at r = 0, m / sin theta is replaced by m'.
 *               Where |t|^2 < PF_PANO_UP_MIN_T2 (the pixel looks at the zenith or the nadir) up = NaN and the latitude stays.
 *   A pixel without an owner has NaN in all three planes.
 * pf_pano_to_fisheye: h_pano / h_pano_hw / h_pano_index as in pf_pano_crop; d_img = DEVICE [batch][H][W][3] of `dtype`; d_valid = NULL or DEVICE
 * [batch][H][W] bytes; d_up [batch][2][H][W] and d_lat [batch][H][W] fp32: both or neither (NULL: no labels).  pf_fisheye_fields: the labels alone,
 * no source; its bits are those of pf_pano_to_fisheye's labels.  The 4-pixel vector stores are taken when W % 4 == 0 and d_img (4 bytes uint8, 16
 * bytes fp32), d_valid (4 bytes), d_up and d_lat (16 bytes) are aligned; otherwise scalar stores give the same bits.  Argument errors return
 * PF_ERR_ARG before any device work with a message that begins with the function's name, checked in this order: `samples` out of range; an unknown
 * `kind`; then n_pano < 1 or NULL source lists, a bad dtype, a NULL panorama or a panorama side < 2, batch < 1 or a NULL required pointer
 * (h_pano_index, d_lens, d_img), H or W < 1, one of d_up / d_lat without the other, an index out of range.  One launch per 32 outputs on `stream`,
 * no workspace, no host synchronisation; stateless, no handle; deterministic, each output's bits independent of the batch it is in. */
#define PF_FISHEYE_NEWTON_STEPS 10
int pf_pano_to_fisheye(int device, int n_pano, const void* const* h_pano, const int32_t* h_pano_hw /*[n_pano][2]*/, int dtype /*PF_PANO_U8|PF_PANO_F32*/,
                       int kind /*PF_FISHEYE_...*/, int batch, const int32_t* h_pano_index /*[batch]*/, const float* d_lens /*[batch][2][12]*/, int H, int W,
                       float fill, void* d_img /*[batch][H][W][3], dtype*/, uint8_t* d_valid /*or NULL*/, float* d_up /*[batch][2][H][W] or NULL*/,
                       float* d_lat /*[batch][H][W], with d_up*/, int samples, void* stream);
int pf_fisheye_fields(int device, int kind, int batch, const float* d_lens /*[batch][2][12]*/, int H, int W, float* d_up /*[batch][2][H][W]*/,
                      float* d_lat /*[batch][H][W]*/, void* stream);

/* The other direction: a fisheye lens fitted to perspective fields, the batched per-image Levenberg-Marquardt fit of pf_fit_camera over the lens
 * model above (fit_camera_fisheye.hip).  theta = (roll r, pitch p, f, cx, cy, k1, k2), NTH = 7: roll and pitch in RADIANS,
 * the relative intrinsics of the other fits, F = f*H, Cx = (cx + 1/2)*W, Cy = (cy + 1/2)*H, and the first two Kannala-Brandt coefficients;
 * k3 = k4 = 0.  The projection kind is one integer per call (PF_FISHEYE_*).  Yaw, `band` and a second lens do not enter.
 * THE MODEL per pixel, at the pixel centre (a, b) = (col + 1/2, row + 1/2) for BOTH labels (there is no linspace grid):
 *   1 radius    dx = a - Cx, dy = b - Cy, r = hypot(dx, dy), rho = r / F; the equisolid kind needs rho < 2
 *   2 theta     theta_d = rho | 2 asin(rho / 2) | 2 atan(rho / 2).  theta = theta_d if k1 = k2 = 0 exactly; otherwise from min(theta_d, theta_max)
 *               exactly PF_FISHEYE_NEWTON_STEPS steps theta <- clamp(theta - (P(theta) - theta_d) / P'(theta), 0, theta_max), in plain floats
 *   3 domain    the pixel HAS A MODEL VALUE iff all of these hold (positive comparisons: a NaN has none):
 *               r - PF_FISHFIT_R_MIN > 0 (the polar form has no derivative at the centre; at most one pixel);
 *               theta_max - theta > 0, theta_max the call's argument in (0, pi): the widest half field of view the caller allows;
 *               theta > 0 (a clamped iteration may end on the axis when theta_d is within the root tolerance: m / sin theta has no value there);
 *               with a polynomial, P'(theta) >= PF_FISHFIT_SLOPE_MIN and |P(theta) - theta_d| <= PF_FISHFIT_ROOT_TOL.
 *               That is: the Newton iteration found an interior root on a rising branch.  It is NOT r < r_max(theta_max), which means nothing for
 *               a trial polynomial that is not monotone.  A pixel without a model value has weight 0 and is not counted in VALID_PIXELS.
 *   4 d theta   from the implicit function, not through the Newton loop: d theta = (d theta_d - theta^3 d k1 - theta^5 d k2) / P'(theta)
 *   5 labels    pf_pano_to_fisheye's: latitude = -atan2(W.y, hypot(W.x, W.z)) in degrees, W = R X; up from g, e_theta, e_phi, m = rho,
 *               m' = rho'(theta_d) P'(theta).  Where |t|^2 < PF_PANO_UP_MIN_T2 the two up rows have weight 0; the latitude row stays.
 * Residuals, loss, weights, damping, accept / reject and stopping rule: as pf_fit_camera.  Clamps: |pitch| <= 89.9 deg, f >= 1e-3, roll wrapped
 * into [-pi, pi], k1 and k2 in [-0.5, 0.5].  FREE SETS: (r, p, f); with free_pp also cx, cy; with poly also k1, k2; all seven with both.  Held
 * entries keep their start values, so a calibrated k1, k2 can be held while orientation and focal length are fitted.
 * Start: d_init = DEVICE [B][7] theta, or NULL: roll and pitch from the 4 x 4 centre pixels (at the circle centre up = (-sin r, -cos r) and
 * lat = p for every kind), cx = cy = k1 = k2 = 0, and f the best of the 16 candidates f = 0.5 / rho(h_c), h_c = (20 + 7 c) degrees the half field
 * of view over half the height.  Pixels outside the image circle are expected as NaN in the input.  An image without a pixel that has finite input
 * and a model value, or with a non-finite entry in its d_init row, ends with CONVERGED 0, VALID_PIXELS 0 and its start parameters.
 * d_out = DEVICE [B][PF_FISHFIT_COLS] fp32: the thirteen columns of pf_fit_camera in the same order, then k1, k2.  VFOV and GENERAL_VFOV keep
 * their formulas in f, cx, cy: for a fisheye lens they describe nothing.
 * Argument errors return PF_ERR_ARG before any device work with a message that begins with "pf_fit_fisheye: ", checked in this order: an unknown
 * `kind`; theta_max outside (0, pi) or not finite; then pf_fit_camera's checks (and poly other than 0 / 1 with free_pp).  Sizes, pointers,
 * launches (max_iter + 1 pairs per 32 images on `stream`, no host synchronisation) and determinism (an image's bits do not depend on its batch)
 * as pf_fit_camera; workspace pf_fit_fisheye_workspace_bytes (0 for batch <= 0 or a size below 8). */
#define PF_FISHFIT_R_MIN 1e-3f     /* pixels */
#define PF_FISHFIT_SLOPE_MIN 1e-2f
#define PF_FISHFIT_ROOT_TOL 4e-6f  /* 16 x the float32 Newton residual of the test lenses (2.4e-7), rounded up */
#define PF_FISHFIT_COL_ROLL 0
#define PF_FISHFIT_COL_PITCH 1
#define PF_FISHFIT_COL_VFOV 2
#define PF_FISHFIT_COL_REL_FOCAL 3
#define PF_FISHFIT_COL_GENERAL_VFOV 4
#define PF_FISHFIT_COL_REL_CX 5
#define PF_FISHFIT_COL_REL_CY 6
#define PF_FISHFIT_COL_RMS_UP 7
#define PF_FISHFIT_COL_RMS_LAT 8
#define PF_FISHFIT_COL_COST 9
#define PF_FISHFIT_COL_ITERATIONS 10
#define PF_FISHFIT_COL_CONVERGED 11
#define PF_FISHFIT_COL_VALID_PIXELS 12 /* pixels with finite input and a model value */
#define PF_FISHFIT_COL_K1 13
#define PF_FISHFIT_COL_K2 14
#define PF_FISHFIT_COLS 15
size_t pf_fit_fisheye_workspace_bytes(int batch, const int32_t* h_hw);
int pf_fit_fisheye(int device, int kind, int batch, const int32_t* h_hw, const float* const* h_up, const float* const* h_lat,
                   const float* d_init /* NULL or [B][7] */, int free_pp, int poly, float theta_max, int loss, float huber_delta_deg, float w_up,
                   float w_lat, int max_iter, float* d_out /* [B][PF_FISHFIT_COLS] */, void* d_workspace, size_t workspace_bytes, void* stream);

/* The relative yaw of camera views of one centre, from the pictures: for ordered pairs (a, b) of views and a list of candidate turns, the moments of
 * the two luminance images on their overlap, from which the zero-mean normalised cross-correlation follows (yaw_align.hip).
 * The fields give roll, pitch and intrinsics of a view but not the direction it faces; with those known, two views of one centre differ by a single
 * turn about the vertical, and the right turn is the one at which the pictures agree where they overlap.
 * Per view theta = d_cam6 row = {roll r, pitch p (RADIANS), rel_focal f, rel_cx cx, rel_cy cy, xi}: pf_reproject's camera without the yaw, the same
 * F, Cx, Cy of the view's own image, R = R_pitch(p) R_roll(r), Y(t), usm_ray, usm_project and z_min.
 * For the ordered pair (a, b), the candidate D (radians) and the stride s, the samples are the pixels (row, col) of b with row % s == 0 and col % s == 0:
 *   1 ray       X_b = the ray of (col + 1/2, row + 1/2) in b (pf_reproject's step 1); a pixel without a ray is no sample.  W = R_b X_b
 *   2 turn      X_a = R_a^T Y(D) W: pf_reproject's M with a as the source at yaw 0 and b as the destination at yaw D, so the pictures agree at
 *               D = yaw_b - yaw_a
 *   3 visible   iff X_a.z > z_min(xi_a)
 *   4 point     (p, q) = F_a (X_a.x, X_a.y) / (X_a.z + xi_a |X_a|) + (Cx_a, Cy_a), pixel-edge units
 *   5 covered   iff visible and p > 0, Ws_a - p > 0, q > 0, Hs_a - q > 0: positive comparisons, a NaN or infinite coordinate (non-finite
 *               parameters) covers nothing and issues no load
 *   6 values    luminance L = 0.299 c0 + 0.587 c1 + 0.114 c2 - c of the channels as stored, c = 127.5 (PF_PANO_U8) or 0.5 (PF_PANO_F32); c conditions
 *               the sums and leaves the correlation unchanged.  y = L_b at the pixel; x = L_a bilinear at (p - 1/2, q - 1/2), the four taps clamped
 *               into a (pf_reproject's step 6)
 * d_moments[pair][candidate] = {n, sum x, sum y, sum x^2, sum y^2, sum xy} over the covered samples, as fp64: fp32 sums over tiles of 1024 samples
 * in sample order (row-major in b), the tiles added in order in fp64.  The caller's score is
 *   ZNCC = (n sum xy - sum x sum y) / sqrt((n sum x^2 - (sum x)^2) (n sum y^2 - (sum y)^2))
 * where both variances are positive; one below 2^-16 of n times its sum of squares is within the rounding of the fp32 sums and counts as 0.
 * Every value depends on its pair's two views, their cameras, the candidate and the stride only: the same bits in any batch of pairs, for any
 * split of the candidates over calls and on every run.  A view with non-finite parameters has n = 0 in all its pairs.
 * h_view = HOST array of n_view (>= 2) DEVICE pointers, (H, W, 3) channel-interleaved, all of type `dtype`; h_view_hw = HOST [n_view][2] (H, W), each >= 1;
 * d_cam6 = DEVICE [n_view][6]; h_pairs = HOST [n_pair][2] (a, b) view indices, a != b; d_cand = DEVICE [n_cand] fp32 radians, 1 <= n_cand <=
 * PF_YAW_MAX_CAND; d_moments = DEVICE [n_pair][n_cand][6] fp64, 16-byte aligned; workspace of pf_yaw_moments_workspace_bytes (0 for arguments
 * pf_yaw_moments rejects): a luminance plane per view, converted once per call, and the tiles' records.
 * Argument errors (NULL pointers, n_view < 2, n_pair < 1, a view side < 1, an index out of range, a == b, stride < 1, n_cand out of range, a bad
 * dtype, a small workspace, a misaligned d_moments) return PF_ERR_ARG before any device work.  One luminance launch per 32 views, a store launch
 * and a sum launch per 64 pairs, all on `stream`, no atomics, no host synchronisation; stateless, no handle. */
#define PF_YAW_MAX_CAND 4096
size_t pf_yaw_moments_workspace_bytes(int n_view, const int32_t* h_view_hw /*[n_view][2]*/, int n_pair, const int32_t* h_pairs /*[n_pair][2]*/,
                                      int n_cand, int stride);
int pf_yaw_moments(int device, int n_view, const void* const* h_view, const int32_t* h_view_hw /*[n_view][2]*/, int dtype /*PF_PANO_U8|PF_PANO_F32*/,
                   const float* d_cam6 /*[n_view][6]*/, int n_pair, const int32_t* h_pairs /*[n_pair][2]: (a, b)*/, int n_cand,
                   const float* d_cand /*[n_cand] radians*/, int stride, double* d_moments /*[n_pair][n_cand][6]*/, void* d_workspace,
                   size_t workspace_bytes, void* stream);

/* Perspective-aware compositing: the Perspective Field Discrepancy of an object's fields against a background's at every place the object could be
 * pasted (place_score.hip).
 * Inputs: background up_bg [2][H][W] and lat_bg [H][W], object up_obj [2][h][w] and lat_obj [h][w], degrees, fp32 (the layout of
 * pred_gravity_original / pred_latitude_original and of pf_pano_crop's labels), 1 <= h <= H, 1 <= w <= W.
 * A field pixel is VALID when its three values are finite and the fp32 squared length of its up vector, fmaf(u_x, u_x, u_y u_y), is >= 1e-12 and
 * finite: pf_field_errors' rule, applied to each field on its own.  A caller masks a pixel by writing NaN into its latitude, so a silhouette is
 * NaN outside the object, and a background padded with NaN lets the object hang over the border.
 * Placements: (j, i) with 0 <= j < P = (H - h) / stride + 1 and 0 <= i < Q = (W - w) / stride + 1 (integer divisions); the object's pixel (r, c)
 * lies on the background's (j stride + r, i stride + c); the object is always fully inside the array.
 * Per pixel pair whose two pixels are valid:
 *   e_up   the angle between the two up vectors in degrees, in [0, 180]: mathematically pf_field_errors' atan2(|cross|, dot), computed as
 *          min(d, 360 - d) with d = |theta_bg - theta_obj| and theta = atan2f(u_y, u_x) in fp32 degrees, clamped to [-180, 180], taken once per
 *          pixel and not once per pair.  Equal vectors give exactly 0; two vectors on either side of +-180 give their small angle
 *   e_lat  |lat_bg - lat_obj|
 * Per placement n = the number of valid pairs, S_up = sum e_up, S_lat = sum e_lat over them:
 *   d_out[pair][j][i] = {S_up, S_lat, n} as fp64, the pairs one after the other, P Q 3 doubles each: fp32 sums over chunks of 1024 object pixels in
 *   row-major order, the chunks added in order in fp64.
 * The caller's scores are the means S_up / n and S_lat / n and their weighted sum, the paper's PFD at weights (1, 1).
 * Every value depends on its pair's two fields and the stride only: the same bits in any batch of pairs and on every run.
 * h_bg_up, h_bg_lat = HOST arrays of n_bg (>= 1) DEVICE pointers; h_bg_hw = HOST [n_bg][2] (H, W), each >= 1, H W < 2^31; h_obj_* likewise for the
 * n_obj (>= 1) objects; h_pairs = HOST [n_pair][2] (background, object) indices; stride >= 1, one per call; d_out 8-byte aligned; workspace of
 * pf_place_scores_workspace_bytes (0 for arguments pf_place_scores rejects): a packed plane per field, written once per call, and the chunks' records.
 * Argument errors (counts < 1, NULL pointers, a side < 1, a pair index out of range, an object larger than its background or of more than 65535
 * chunks, stride < 1, a small workspace, a misaligned d_out) return PF_ERR_ARG before any device work.  One pack launch per 32 fields, a store
 * launch and a sum launch per 32 pairs, all on `stream`, no atomics, no host-to-device copy, no host synchronisation; stateless, no handle. */
size_t pf_place_scores_workspace_bytes(int n_bg, const int32_t* h_bg_hw /*[n_bg][2]*/, int n_obj, const int32_t* h_obj_hw /*[n_obj][2]*/, int n_pair,
                                       const int32_t* h_pairs /*[n_pair][2]*/, int stride);
int pf_place_scores(int device, int n_bg, const float* const* h_bg_up, const float* const* h_bg_lat, const int32_t* h_bg_hw /*[n_bg][2]*/, int n_obj,
                    const float* const* h_obj_up, const float* const* h_obj_lat, const int32_t* h_obj_hw /*[n_obj][2]*/, int n_pair,
                    const int32_t* h_pairs /*[n_pair][2]: (background, object)*/, int stride, double* d_out /*[pair][P][Q][3]*/, void* d_workspace,
                    size_t workspace_bytes, void* stream);

/* Similarity transform of a perspective field: the fields of a picture that is resized by s and turned by phi in its plane (field_xform.hip, DESIGN.md
 * section 26).  Field layout and the VALID rule are pf_place_scores'.  A VARIANT is a scale s > 0 and a rotation phi in degrees.
 *   map        source (h, w) -> output (h', w'): a source point p goes to c_out + s R(phi) (p - c_src), R(phi) = [[cos phi, -sin phi], [sin phi, cos phi]]
 *              in array coordinates (x right, y down), c_src = (w/2, h/2), c_out = (w'/2, h'/2).  Positive phi turns the picture clockwise on the
 *              screen: the fields of a camera whose roll is lower by phi.  cos phi and sin phi are taken in fp64 from remainder(phi, 360) and are
 *              exactly 0 or +-1 at the multiples of 90.
 *   size       pf_fields_transform_size: h' = max(1, floor(s (h |cos phi| + w |sin phi|) + 1/2)), w' with h and w exchanged, in fp64; PF_ERR_ARG for
 *              h, w < 1, a scale that is not finite and > 0, a rotation that is not finite, or h' w' >= 2^31.  pf_fields_transform takes any h', w'.
 *   sampling   output pixel (r', c'): d = (c' + 1/2 - w'/2, r' + 1/2 - h'/2), source position (x, y) = c_src + R(-phi) d / s - (1/2, 1/2) in
 *              pixel-centre coordinates, computed in fp32 from cos phi, sin phi and 1 / s rounded to fp32.  Four bilinear taps at floor(x), floor(y) and
 *              their + 1 neighbours; a tap outside the array or on an invalid pixel is DROPPED, not clamped.  W_v = the weights of the taps left.  The
 *              pixel is valid iff W_v >= 1/2 and the mix m = sum w_k u_k, rounded to fp32, passes the length rule of VALID.
 *                lat' = sum w_k lat_k / W_v
 *                up'  = R(phi) m scaled to unit length (the taps are not normalised first); left unscaled where its squared length is within 2^-22
 *                       of 1 already, so that a vector that is of unit length in fp32 keeps its bits
 *              both in fp64 from the fp32 weights and rounded to fp32 once.  An invalid pixel is NaN in all three planes.
 *              So a silhouette keeps its outline to half a pixel, an array border behaves like a clamp, a position more than half a pixel outside the
 *              source is invalid, and s = 1, phi = 0 at the source's size returns the bits of a field of unit up vectors.
 *   no prefilter: fields are smooth; only a silhouette aliases when s is far below 1.
 * Job k transforms source field h_up[k], h_lat[k] of size h_hw[k] by variant h_variants[k] = (s, phi) into h_out_up[k] (2, h', w') and h_out_lat[k]
 * (h', w') of size h_out_hw[k]; a source may be named by any number of jobs, an output by one.  All h_* are HOST arrays; the fields are DEVICE pointers.
 * Argument errors (n < 1, NULL arrays or pointers, a side < 1, 2^31 pixels or more on either side, a bad variant) return PF_ERR_ARG before any device
 * work.  One launch per 32 jobs on `stream`; no atomics, no host-to-device copy, no host synchronisation; stateless, no handle. */
int pf_fields_transform_size(int h, int w, double scale, double rotation_deg, int32_t* h_out_hw /*[2]*/);
int pf_fields_transform(int device, int n, const float* const* h_up, const float* const* h_lat, const int32_t* h_hw /*[n][2]*/,
                        const double* h_variants /*[n][2]: (scale, rotation in degrees)*/, const int32_t* h_out_hw /*[n][2]*/, float* const* h_out_up,
                        float* const* h_out_lat, void* stream);

/* pf_place_scores over a set of variants of every object, and the best (variant, offset) of every pair found on the device.
 * Backgrounds, objects, pairs and stride as pf_place_scores takes them; h_variants = HOST [n_var][2] (scale, rotation in degrees), shared by all pairs.
 *   1. every object is transformed by every variant into the workspace (pf_fields_transform at pf_fields_transform_size's size);
 *   2. pf_place_scores' three kernels, unchanged, over every (pair, variant) whose transformed object fits its background, 32 per launch.  The raw
 *      records {S_up, S_lat, n} go to d_maps: pair by pair, variant by variant, P Q 3 doubles each (P, Q from the transformed size), nothing for a
 *      variant that does not fit.  They are the bits pf_place_scores gives on pf_fields_transform's output;
 *   3. per (pair, variant) and placement, in fp64: up_mean = S_up / n, lat_mean = S_lat / n, pfd = w_up up_mean + w_lat lat_mean (two products and
 *      a sum, each rounded), +inf where n < min_valid x (valid pixels of the transformed object) or n = 0.  The lowest pfd per variant, then per pair
 *      over the variants; ties go to the lowest variant, then to the first placement in row-major order.
 *   d_var[pair][variant]  = {best pfd, row, col, valid pixels of the variant, h', w'}; a variant that does not fit, or has no finite pfd: +inf, -1, -1
 *   d_best[pair]          = {pfd, up_mean, lat_mean, n, variant, row, col}; row, col in background pixels; all +inf: {+inf, NaN, NaN, 0, -1, -1, -1}
 * d_maps holds maps_doubles doubles, at least the sum above; d_maps, d_best, d_var 8-byte aligned.  Argument errors -- pf_place_scores' except that an
 * object larger than its background is no error here, n_var < 1, a bad variant (pf_fields_transform_size), a transformed object of more than 65535
 * chunks in a pair it fits, min_valid outside [0, 1], a weight that is negative or not finite, a small d_maps or workspace -- return PF_ERR_ARG before
 * any device work; pf_place_search_workspace_bytes is 0 for arguments that set the layout and are rejected.  All launches on `stream`, no atomics,
 * no host-to-device copy, no host synchronisation; every value depends on its pair's fields, the variants, the stride, the threshold and the weights
 * only: the same bits in any batch of pairs, in any order of them, and on every run.  Stateless, no handle. */
size_t pf_place_search_workspace_bytes(int n_bg, const int32_t* h_bg_hw /*[n_bg][2]*/, int n_obj, const int32_t* h_obj_hw /*[n_obj][2]*/, int n_pair,
                                       const int32_t* h_pairs /*[n_pair][2]*/, int n_var, const double* h_variants /*[n_var][2]*/, int stride);
int pf_place_search(int device, int n_bg, const float* const* h_bg_up, const float* const* h_bg_lat, const int32_t* h_bg_hw /*[n_bg][2]*/, int n_obj,
                    const float* const* h_obj_up, const float* const* h_obj_lat, const int32_t* h_obj_hw /*[n_obj][2]*/, int n_pair,
                    const int32_t* h_pairs /*[n_pair][2]: (background, object)*/, int n_var, const double* h_variants /*[n_var][2]*/, int stride,
                    double min_valid, double w_up, double w_lat, double* d_maps, size_t maps_doubles, double* d_best /*[n_pair][7]*/,
                    double* d_var /*[n_pair][n_var][6]*/, void* d_workspace, size_t workspace_bytes, void* stream);

/* Perspective fields drawn over their images on the device: a latitude tint, iso-latitude lines and up arrows (draw_fields.hip, DESIGN.md
 * section 22).  The drawing model is this library's own; parity with a plotting library's rasteriser is not offered.
 * Per image: the picture img [H][W][3] (channel-interleaved, uint8 or fp32, values on the 0 - 255 scale in both types: the colours below are given on
 * it), up [2][H][W] and lat [H][W] degrees, fp32 (the layout of pred_gravity_original / pred_latitude_original), all of the image's size; out of
 * the picture's type and shape, which may be the picture itself.
 * A pixel is VALID when its three field values are finite and the fp32 squared length of its up vector, fmaf(u_x, u_x, u_y u_y), is >= 1e-12 and
 * finite: the rule of pf_field_errors, so NaN is the mask.  A latitude is FINITE when it is neither NaN nor infinite.
 * Output pixel (row, col) has the centre p = (col + 1/2, row + 1/2).  v = the fp32 value of the input pixel, per channel; three layers are put
 * "over" it in this order:
 *   1 tint    (PF_DRAW_LAT)  valid pixels only: c = ramp(lat), the piecewise-linear map through PF_DRAW_RAMP at -90, -45, 0, 45, 90 degrees:
 *             t = clamp((lat + 90) / 45, 0, 4), i = min(floor(t), 3), c = (1 - (t - i)) RAMP[i] + (t - i) RAMP[i + 1];  v <- (1 - alpha) v + alpha c
 *   2 lines   (PF_DRAW_LAT)  g = (g_x, g_y), the gradient of lat in degrees per pixel: per component the central difference (next - previous) / 2
 *             where both neighbours are inside the image and finite, else the one-sided difference with the one that is, else 0.
 *             k = lat_step_deg rint(lat / lat_step_deg), ties to even; d = |lat - k| / |g|; w' = line_width, 2 line_width for k = 0 (the horizon);
 *             cov = clamp(1/2 + w' / 2 - d, 0, 1), 0 where the pixel is not valid or not |g| >= PF_DRAW_GRAD_FLOOR;
 *             v <- (1 - cov) v + cov PF_DRAW_LINE_RGB
 *   3 arrows  (PF_DRAW_UP)   anchors: the pixels (j s + s / 2, i s + s / 2) inside the image, s = spacing, integer divisions; a = the pixel's centre.
 *             A valid anchor pixel carries an arrow: u = its up vector times 1 / sqrt(its squared length) (x right, y down: an upright camera's
 *             arrows point to the top of the picture), L = arrow_len_rel W (the fp32 product), three segments given by a start, a unit
 *             direction and a length: the shaft (a, u, L) and two barbs (a + L u, R(+-PF_DRAW_HEAD_ANGLE) (-u), PF_DRAW_HEAD_RATIO L) with
 *             R(t) (x, y) = (x cos t - y sin t, x sin t + y cos t).  dist(p, (b, e, l)) = |r - clamp(r . e, 0, l) e| with r = p - b.
 *             cov = the maximum over all arrows and their segments of clamp(1/2 + line_width / 2 - dist, 0, 1), a maximum and not a sum: the
 *             bits do not depend on the order the arrows are visited in;  v <- (1 - cov) v + cov arrow_rgb.  An arrow that leaves the image
 *             is clipped by not being drawn there.
 * uint8 outputs are the value rounded half up and clamped to [0, 255], fp32 outputs the value.  A pixel that no layer covers, and every pixel
 * with layers = 0, is the input's bits.
 * h_hw = HOST [batch][2] (H, W), each >= 1, H W < 2^31; h_img, h_up, h_lat, h_out = HOST arrays of `batch` DEVICE pointers; dtype PF_PANO_U8 |
 * PF_PANO_F32; spacing >= 1, one per call; arrow_len_rel in [0, 1e6]; line_width finite and >= 0; lat_step_deg finite and > 0; alpha in [0, 1]; h_arrow_rgb = HOST
 * [3] finite; layers = PF_DRAW_UP | PF_DRAW_LAT or less.  Workspace of pf_draw_fields_workspace_bytes (0 for arguments pf_draw_fields
 * rejects): a 64-byte record per anchor, written once per call.  Argument errors return PF_ERR_ARG before any device work.  Two launches per 32
 * images (one without PF_DRAW_UP) on `stream`, no atomics, no host-to-device copy, no host synchronisation; stateless, no handle.  Every output
 * pixel depends on its own image and fields only: the same bits in any batch and on every run. */
#define PF_DRAW_UP 1
#define PF_DRAW_LAT 2
#define PF_DRAW_RAMP {{33.f, 102.f, 172.f}, {146.f, 197.f, 222.f}, {247.f, 247.f, 247.f}, {244.f, 165.f, 130.f}, {178.f, 24.f, 43.f}}
#define PF_DRAW_LINE_RGB {32.f, 32.f, 32.f}
#define PF_DRAW_GRAD_FLOOR 1e-6f      /* degrees per pixel: no iso-line where the latitude is flatter */
#define PF_DRAW_HEAD_ANGLE_DEG 25.0   /* of a barb against the shaft */
#define PF_DRAW_HEAD_COS 0.9063078f   /* the fp32 values nearest cos and sin of it */
#define PF_DRAW_HEAD_SIN 0.42261827f
#define PF_DRAW_HEAD_RATIO 0.35f      /* length of a barb in shaft lengths */
size_t pf_draw_fields_workspace_bytes(int batch, const int32_t* h_hw /*[batch][2]*/, int spacing);
int pf_draw_fields(int device, int batch, const int32_t* h_hw /*[batch][2]*/, const void* const* h_img, const float* const* h_up,
                   const float* const* h_lat, void* const* h_out, int dtype /*PF_PANO_U8|PF_PANO_F32*/, int spacing, float arrow_len_rel /*of W*/,
                   float lat_step_deg, float alpha, float line_width, const float* h_arrow_rgb /*[3]*/, int layers /*PF_DRAW_UP|PF_DRAW_LAT*/,
                   void* d_workspace, size_t workspace_bytes, void* stream);

/* Objects pasted into background pictures on the device: the object's pixels under pf_fields_transform's similarity, alpha-blended into the
 * background at a placement that is read from device memory (composite.hip).  What pf_place_search finds can be pasted
 * without a host synchronisation in between.
 *   images     channel-interleaved [H][W][3], uint8 or fp32 on the 0 - 255 scale (pf_draw_fields' pictures); backgrounds, objects and outputs of one
 *              dtype.  An object's alpha is an [h][w] fp32 plane; a NULL plane is opaque; a value is clamped to [0, 1] and NaN is 0.
 *   jobs       job k = background h_jobs[k][0], object h_jobs[k][1], output h_out[k] of the background's size, and the row
 *              d_place[k] = (s, phi in degrees, row, col, h', w'), six fp64 values in DEVICE memory.  (s, phi) is a variant of pf_fields_transform;
 *              (row, col) is where the top-left corner of the transformed object's h' x w' box lies in the background (pf_place_search's offset); it
 *              may be negative and the box may hang over the border: the paste is clipped to the background.  A row is INACTIVE when s is not finite
 *              and > 0; phi, row or col is not finite; row or col is not integer-valued or is 2^30 or more in magnitude; h' or w' is < 1, not
 *              integer-valued, or 2^31 or more.  An inactive row gives the background's bits and coverage 0.
 *   sampling   output pixel (R, C), r' = R - row, c' = C - col.  Outside [0, h') x [0, w'): the background's bits, coverage 0.  Inside, for the
 *              sub-samples a, b < S = `samples`, a-major (the order of the supersampled gathers): d = (c' + (b + 1/2) / S - w'/2,
 *              r' + (a + 1/2) / S - h'/2) with (b + 1/2) / S an fp32 quotient, source position (x, y) = (w/2, h/2) + R(-phi) d / s - (1/2, 1/2),
 *              in fp32 with pf_fields_transform's operations; four bilinear taps at floor(x), floor(y) and their + 1 neighbours.  A tap outside the
 *              array is TRANSPARENT -- it counts as alpha 0 and is not dropped and renormalised --, a tap whose alpha is 0 is skipped, so that what
 *              lies under a zero alpha, NaN included, never reaches the output.  A_ab = sum w_k alpha_k and P_ab = sum (w_k alpha_k) c_k per
 *              channel, in fp64 from the fp32 weights w_k; A and P are the means over the S x S sub-samples.
 *   cos, sin   of phi in fp64 from remainder(phi, 360), exactly 0 or +-1 at the multiples of 90, and 1 / s: computed once per job on the device
 *              and rounded to fp32 once.
 *   edge       PF_COMPOSITE_SOFT: cov = opacity A, out = bg (1 - cov) + opacity P.
 *              PF_COMPOSITE_HARD: where A >= 1/2, cov = opacity and out = bg (1 - opacity) + opacity P / A; elsewhere cov = 0 -- the silhouette that
 *              pf_fields_transform keeps, so the pasted pixels are the pixels the search scored.
 *              Where cov = 0 the output is the background's bits.
 *   blend      in fp64, rounded once: fp32 outputs by one rounding, uint8 outputs half up and clamped to [0, 255].
 * h_bg, h_obj = HOST arrays of n_bg, n_obj (>= 1) DEVICE pointers; h_obj_alpha = NULL (every object opaque) or a HOST array of n_obj DEVICE pointers
 * whose entries may be NULL; h_bg_hw, h_obj_hw = HOST [.][2] (H, W), each >= 1, H W < 2^31; dtype PF_PANO_U8 | PF_PANO_F32; h_jobs = HOST [n][2]; h_out =
 * HOST array of n DEVICE pointers, every job its own image, none of them a background; d_cov = NULL or DEVICE fp32, the coverage planes of
 * the jobs one after another, job k's of its background's size; workspace of pf_composite_workspace_bytes(n) (0 for n < 1): one record per job.
 * Argument errors (counts < 1, NULL arrays or pointers, a side < 1 or 2^31 pixels or more, a job index out of range, samples outside
 * 1 ... PF_GATHER_MAX_SAMPLES, opacity outside [0, 1] or not finite, an unknown edge or dtype, a small workspace, an output that is its background or another job's or is shared by two jobs,
 * fp32 data not aligned to 4 bytes, d_place not to 8) return PF_ERR_ARG before any device work.  Two launches per 32 jobs on `stream`, no atomics, no
 * host-to-device copy, no host synchronisation; stateless, no handle.  Every output pixel depends on its own job only: the same bits in any batch, in
 * any order of the jobs and on every run. */
#define PF_COMPOSITE_SOFT 0
#define PF_COMPOSITE_HARD 1
size_t pf_composite_workspace_bytes(int n);
int pf_composite(int device, int n_bg, const void* const* h_bg, const int32_t* h_bg_hw /*[n_bg][2]*/, int n_obj, const void* const* h_obj,
                 const float* const* h_obj_alpha /*entries may be NULL*/, const int32_t* h_obj_hw /*[n_obj][2]*/, int dtype /*PF_PANO_U8|PF_PANO_F32*/, int n,
                 const int32_t* h_jobs /*[n][2]: (background, object)*/, const double* d_place /*[n][6]: s, phi, row, col, h', w'*/, double opacity,
                 int edge /*PF_COMPOSITE_SOFT|PF_COMPOSITE_HARD*/, int samples, void* const* h_out /*n device pointers*/, float* d_cov /*[n] planes or NULL*/,
                 void* d_workspace, size_t workspace_bytes, void* stream);

/* Predicted perspective fields against ground truth on the device: per-pixel errors, per-image statistics with an exact median, and
 * a running histogram for dataset statistics (field_err.hip).
 * Inputs per image: up_pred, up_gt [2][H][W] and lat_pred, lat_gt [H][W] degrees, fp32 (the layout of pred_gravity_original /
 * pred_latitude_original and of pf_pano_crop's labels).  With p = up_pred, g = up_gt at one pixel:
 *   e_up  = atan2(|p_x g_y - p_y g_x|, p_x g_x + p_y g_y) in degrees, in [0, 180] (cross and dot, no normalisation, no acos)
 *   e_lat = |lat_pred - lat_gt| in degrees
 *   valid   all six input values finite and both vectors of squared length >= 1e-12 (and the fp32 cross, dot and difference finite: components
 *           beyond ~1e19 count as non-finite).  A caller masks a pixel by writing NaN into the label; pf_pano_crop's NaN labels mask themselves.
 *           Invalid pixels enter no statistic.
 * Per image and per metric over the n valid pixels: mean, rmse, max, median, frac_below (share with e < threshold_deg, strict) and n.  The
 * median is numpy's: with the errors sorted, (s[(n-1)/2] + s[n/2]) / 2, both order statistics exact elements of the fp32 error set (radix
 * selection on the bit patterns, which order like unsigned integers for non-negative floats), their average taken in fp64.  n = 0: NaN
 * statistics and n = 0, not an error.  Sums are reduced in fp64 in a fixed order and counts are integers: deterministic, each image's row
 * independent of the batch it is in.
 * h_hw = HOST [B][2] (H, W), each >= 1, H * W < 2^31; h_* = HOST arrays of B DEVICE pointers.  d_out = DEVICE [B][PF_FERR_COLS] fp64 (columns
 * below) or NULL.  h_err_up / h_err_lat: optional per-pixel error maps [H][W], NaN where invalid; both or neither.
 * d_hist = optional DEVICE [2][PF_FERR_BINS] int64 running histogram (up, lat), ADDED to: bins of 1 / PF_FERR_BINS_PER_DEG degree,
 * bin = min((int)(e * 64), PF_FERR_BINS - 1) (e * 64 is exact in fp32: the bin of an fp32 error is the same everywhere; errors >= 180 land in
 * the last bin).  d_hist_sums (required with d_hist, else NULL) = DEVICE [2][PF_FERR_SUMS] fp64 running totals per metric, columns
 * PF_FERR_SUM_*; a zeroed pair is an empty state, states merge by addition (the maximum by max).
 * threshold_deg finite and > 0.  Workspace: pf_field_errors_workspace_bytes(B, h_hw) (0 for bad sizes).  Argument errors return PF_ERR_ARG
 * before any device work.  Everything is enqueued on `stream`, no host synchronisation; stateless, no handle. */
#define PF_FERR_COL_UP_MEAN 0
#define PF_FERR_COL_UP_MEDIAN 1
#define PF_FERR_COL_UP_RMSE 2
#define PF_FERR_COL_UP_MAX 3
#define PF_FERR_COL_UP_FRAC_BELOW 4
#define PF_FERR_COL_LAT_MEAN 5
#define PF_FERR_COL_LAT_MEDIAN 6
#define PF_FERR_COL_LAT_RMSE 7
#define PF_FERR_COL_LAT_MAX 8
#define PF_FERR_COL_LAT_FRAC_BELOW 9
#define PF_FERR_COL_VALID_PIXELS 10
#define PF_FERR_COLS 11
#define PF_FERR_BINS 11520
#define PF_FERR_BINS_PER_DEG 64
#define PF_FERR_SUM_N 0        /* valid pixels */
#define PF_FERR_SUM_E 1        /* sum of the errors */
#define PF_FERR_SUM_E2 2       /* sum of their squares */
#define PF_FERR_SUM_MAX 3      /* largest error (0 for an empty state) */
#define PF_FERR_SUM_BELOW 4    /* errors < threshold_deg */
#define PF_FERR_SUMS 5
size_t pf_field_errors_workspace_bytes(int batch, const int32_t* h_hw);
int pf_field_errors(int device, int batch, const int32_t* h_hw, const float* const* h_up_pred, const float* const* h_lat_pred,
                    const float* const* h_up_gt, const float* const* h_lat_gt, float threshold_deg, double* d_out, float* const* h_err_up,
                    float* const* h_err_lat, int64_t* d_hist, double* d_hist_sums, void* d_workspace, size_t workspace_bytes, void* stream);

/* ---- kernel-level entry points (used by the parity tests; same kernels pf_forward runs) ----
 * NHWC fp32 device activations; weights are HOST pointers in the reference's layouts.
 * "planes": the engine's internal split activation formats -- an fp32 tensor stored as planes of 16-bit values, plane k at
 * `planes + k * (plane_elems & ~1)`, each laid out like the fp32 tensor.  Bit 0 of every *_plane_elems argument selects the
 * format: 0 = three bf16 planes (x == h + m + l exactly; read by the bf16 schemes), 1 = two fp16 planes of the split-f16
 * scheme (x ~ hi + lo, lo = fp16(x - hi) unscaled: what that scheme's GEMM computes from fp32 while staging; 4 bytes per element).
 * Producers write them for tensors that only feed GEMMs (PF_SBA=1); every *_planes argument is optional (NULL). */
/* kernel-level entry points only: until called again, every pf_op_* launch of this thread hands `d_counter_u32` (NULL = off, the default) to its kernel as
 * ConvParams::sat and friends, with `limit` as sat_limit.  Windows a kernel hard-codes (attention q 8188 in attn_block.hip, kv 4094 in rb_chain.hip) stay.
 * The timing loops (iters > 0) and the *_bench entries run with the watch off. */
int pf_op_set_saturation_watch(void* d_counter_u32, float limit);
int pf_op_conv2d(int device, const float* d_x, const float* d_x2, int B, int H, int W, int C1, int C2,
                 const float* h_weight /*[Cout][C1+C2][KH][KW]*/, const float* h_bias /*[Cout] or NULL*/,
                 int Cout, int KH, int KW, int stride, int pad, int act /*0 none 1 relu 2 gelu*/,
                 const float* d_res1, const float* d_res2, int post_relu, int nchw_out, int tile_id /*-1 auto*/,
                 float* d_y /*may be NULL when d_y_planes is given*/,
                 const uint16_t* d_x_planes /*replaces d_x*/, long x_plane_elems, const uint16_t* d_x2_planes, long x2_plane_elems,
                 uint16_t* d_y_planes, long y_plane_elems, int precision /*PF_PRECISION_* (split tiles only); + 16: no split-K (otherwise applied by the engine's rule)*/, void* stream);
/* times `iters` launches of one conv shape on random data with tile config `tile_id` (-1 auto); avg ms per launch.
 * fmt_prec = fmt + 16 * precision; fmt 0: fp32 in / out; 1: input as bf16 planes; 2: input and output as planes
 * (1 / 2: the exact bf16 split); precision = PF_PRECISION_* used by the split tiles */
/* y = act(Linear(LayerNorm(x))) + res1 with the LayerNorm fused into the GEMM (ConvParams::ln: row statistics accumulated while the rows are
 * staged, gamma / beta folded into the weights / bias here on the host) -- the engine's form of mix_transformers.py:200 (norm2 -> fc1),
 * :123-126 (sr norm -> kv) and convnext.py:50-51 (norm -> pwconv1).  K % 32 == 0, N % 4 == 0; tile_id as pf_op_conv2d (linear split tiles only). */
int pf_op_linear_ln(int device, const float* d_x, long rows, int K, const float* h_weight /*[N][K]*/, const float* h_bias, const float* h_gamma, const float* h_beta,
                    float eps, int N, int act, const float* d_res1, int tile_id, float* d_y, int precision, void* stream);
/* One nn.Linear of the MiT stage-3 / 4 blocks in the row-block form (rb_gemm.hip): y = act(Linear(LayerNorm?(x))) + res on blocks of 64 token rows of one image --
 * mix_transformers.py:80-88 (q, kv, proj), :26-29 (fc1, fc2), with :199-200 / :125 (norm1, norm2, attn.norm) applied while the rows are staged when h_gamma != NULL.
 * rows = images x tokens; (K, N) = (320, multiple of 320) or (multiple of 256 above 320, 320); res may alias y.  iters > 0 additionally times `iters` launches. */
int pf_op_rb_linear(int device, const float* d_x, long rows, int tokens, int K, const float* h_weight /*[N][K]*/, const float* h_bias, const float* h_gamma, const float* h_beta,
                    float eps, int N, int act, const float* d_res, float* d_y, int iters, float* ms_out, void* stream);
/* The seam between the attention half and the Mlp half of a MiT block in one launch (rb_chain.hip): x += proj(attn_out), hidden = fc1(LayerNorm_2(x)) --
 * mix_transformers.py:137-139 (proj), :199 (residual), :200 / :52 (norm2 -> fc1).  attn (B tokens, C), x (B tokens, C) read and written, hidden (B tokens, 4C);
 * C = 320; weights in the reference's shapes.  iters > 0 additionally times `iters` launches (x is then garbage). */
int pf_op_rb_proj_fc1(int device, const float* d_attn, float* d_x, int B, int tokens, int C, const float* h_proj_w, const float* h_proj_b, const float* h_ln2_gamma,
                      const float* h_ln2_beta, float eps, const float* h_fc1_w, const float* h_fc1_b, float* d_hidden, int iters, float* ms_out, void* stream);
/* The attention half of a one-head, 64-channel MiT block (stage 1 of MiT-B3) as ONE kernel (attn_block.hip): y = x + proj(softmax((LayerNorm_1(x) Wq^T + bq) K^T / 8) V)
 * -- Block.forward, mix_transformers.py:199, with Attention.forward :108-141 (q :110, softmax :133-134, proj :137-138).  x, y: (B, N, 64) token rows (y may alias x),
 * kv: (B, M, 128) keys | values of the spatially reduced tokens (1 <= M <= 128); weights in the reference's shapes.  iters > 0 additionally times `iters` launches. */
int pf_op_mit_attn64(int device, const float* d_x, const float* d_kv, float* d_y, int B, int N, int M, const float* h_ln1_gamma, const float* h_ln1_beta, float eps,
                     const float* h_q_w, const float* h_q_b, const float* h_proj_w, const float* h_proj_b, int iters, float* ms_out, void* stream);
/* The 7 x 7 convolutions that read the normalised image, as one specialised kernel (stem7.hip): conv 7x7 / stride 2 (the low-level encoder, perspectivefields.py:70-83: eval
 * BatchNorm folded by the caller into weight / bias, relu = 1) or stride 4 (MiT's first patch embedding + its LayerNorm, mix_transformers.py:205-246: ln gamma / beta given),
 * pad 3, 3 -> 64 channels.  x: (B, H, W, 4) NHWC4 with channel 3 = 0; y: (B, Ho, Wo, 64); weight in the reference's shape (64, 3, 7, 7).  iters > 0 also times launches. */
int pf_op_stem7x7(int device, const float* d_x, float* d_y, int B, int H, int W, int stride, const float* h_weight, const float* h_bias, int relu, const float* h_ln_gamma,
                  const float* h_ln_beta, float eps, int iters, float* ms_out, void* stream);
/* y = x W^T + b (+ res) for a 128 -> 128 nn.Linear over many rows (thin_linear.hip; the q / output projections of the MiT stage-2 blocks, mix_transformers.py:110,
 * :137-138): x, res, y (rows, 128) device fp32 (y may alias res), weight (128, 128) / bias (128) host, the reference's shapes.  iters > 0 also times launches. */
int pf_op_thin128(int device, const float* d_x, long rows, const float* h_weight, const float* h_bias, const float* d_res, float* d_y, int iters, float* ms_out, void* stream);
/* The key / value branch of a MiT block with 2 x 2 spatial reduction in one launch (rb_chain.hip): kv = Linear_kv(LayerNorm(Conv2d_2x2s2(LayerNorm_1(x)))),
 * mix_transformers.py:119-127 (norm1 of :199 applied to the gathered source tokens).  x: (B, 2 Hr, 2 Wr, C) NHWC token map, C = 320; weights in the reference's shapes
 * (sr [C][C][2][2], kv [2C][C]); kv out: (B, Hr Wr, 2C).  iters > 0 additionally times `iters` launches. */
int pf_op_rb_srkv(int device, const float* d_x, int B, int Hr, int Wr, int C, const float* h_ln1_gamma, const float* h_ln1_beta, float eps1, const float* h_sr_w,
                  const float* h_sr_b, const float* h_srn_gamma, const float* h_srn_beta, float eps2, const float* h_kv_w, const float* h_kv_b, float* d_kv, int iters,
                  float* ms_out, void* stream);
/* One ConvNeXt block MLP in one kernel: y += ls * pwconv2(GELU(pwconv1(LayerNorm(d)))), convnext.py:49-58; C = 96 or 192 (cnx_mlp.hip: hidden map in
 * registers) or C = 384 or 768 (cnx_rb.hip: row blocks resident in LDS); weights
 * in the reference's shapes (pwconv1 [4C][C], pwconv2 [C][4C], layer scale ls [C]); y is read (residual) and written.  iters > 0 additionally times
 * `iters` launches (avg ms in *ms_out; y is then garbage). */
int pf_op_cnx_mlp(int device, const float* d_d, float* d_y, long rows, int C, const float* h_w1, const float* h_b1, const float* h_ln_gamma, const float* h_ln_beta,
                  float eps, const float* h_w2, const float* h_b2, const float* h_layer_scale, int iters, float* ms_out, void* stream);
/* One MiT block Mlp in one kernel (mit_mlp.hip): y = x + fc2(GELU(dwconv3x3(fc1(LayerNorm(x))))), mix_transformers.py:49-56,200,497-508; x, y: (B, Hs, Ws, C) NHWC
 * token maps in DIFFERENT buffers, C = 64 or 128; weights in the reference's shapes (fc1 [4C][C], dwconv [4C][1][3][3], fc2 [C][4C]).  iters > 0 additionally
 * times `iters` launches (avg ms in *ms_out). */
int pf_op_mit_mlp(int device, const float* d_x, float* d_y, int B, int Hs, int Ws, int C, const float* h_fc1_w, const float* h_fc1_b, const float* h_ln_gamma,
                  const float* h_ln_beta, float eps, const float* h_dw_w, const float* h_dw_b, const float* h_fc2_w, const float* h_fc2_b, int iters, float* ms_out, void* stream);
int pf_op_conv2d_bench(int device, int B, int H, int W, int Cin, int Cout, int K, int stride, int pad, int tile_id, int iters, int fmt_prec, float* ms_out);
/* fp32 <-> planes in the format selected by bit 0 of plane_elems (the names are historical) */
int pf_op_split_bf16(int device, const float* d_x, long n, uint16_t* d_planes, long plane_elems, void* stream);
int pf_op_merge_bf16(int device, const uint16_t* d_planes, long plane_elems, long n, float* d_y, void* stream);
/* times one depthwise-3x3+GELU launch variant on random data (0 = LDS halo tile, 1-4 = register-window direct, 99 = plain copy; 0, 1, 3, 99: tuning builds only;
 * 1000 + 100 s + 10 t + c: multi-column kernel, block shape s, strip height t, (columns, prefetch) code c -- elem.hip) */
int pf_op_dwconv3x3_bench(int device, int variant, int B, int H, int W, int C, int iters, float* ms_out);
int pf_op_layernorm(int device, const float* d_x, const float* h_gamma, const float* h_beta, float* d_y, long rows, int C, float eps,
                    uint16_t* d_y_planes, long plane_elems, void* stream);
int pf_op_dwconv3x3_gelu(int device, const float* d_x, const float* h_weight /*[C][1][3][3]*/, const float* h_bias, float* d_y, int B, int H, int W, int C,
                         uint16_t* d_y_planes, long plane_elems, void* stream);
/* the same with an explicit kernel variant (pf_op_dwconv3x3_bench's ids; >= 1000: multi-column / prefetching kernel, falls back to the
 * default when the shape does not fit its block) */
int pf_op_dwconv3x3_gelu_cfg(int device, const float* d_x, const float* h_weight, const float* h_bias, float* d_y, int B, int H, int W, int C,
                             uint16_t* d_y_planes, long plane_elems, int variant, void* stream);
int pf_op_dwconv7x7(int device, const float* d_x, const float* h_weight /*[C][1][7][7]*/, const float* h_bias, float* d_y, int B, int H, int W, int C, void* stream);
/* the same with an explicit kernel: variant 3 = column-blocked streaming kernel (nc = 4 / 2 output columns per thread, nb = 2 / 3
 * row buffers, th = rows per strip; 0 = automatic), 2 = one column per lane; and a timing loop on random data (avg ms per launch) */
int pf_op_dwconv7x7_cfg(int device, const float* d_x, const float* h_weight, const float* h_bias, float* d_y, int B, int H, int W, int C,
                        int variant, int nc, int nb, int th, void* stream);
int pf_op_dwconv7x7_bench(int device, int variant, int nc, int nb, int th, int B, int H, int W, int C, int iters, float* ms_out);
int pf_op_sr_attention(int device, const float* d_q, const float* d_kv, float* d_out, int B, int N, int M, int heads,
                       uint16_t* d_out_planes, long plane_elems, void* stream);
/* explicit kernel: variant 1 = split-f16 MFMA (default of the forward), 0 = exact fp32 MFMA; iters > 0 additionally times
 * `iters` launches (avg ms per launch in *ms_out; synchronises) */
int pf_op_sr_attention_variant(int device, int variant, const float* d_q, const float* d_kv, float* d_out, int B, int N, int M, int heads,
                               int iters, float* ms_out, void* stream);
int pf_op_upsample2x(int device, const float* d_x, float* d_y, int B, int H, int W, int C, uint16_t* d_y_planes, long plane_elems, void* stream);
int pf_op_num_conv_tiles(void);
const char* pf_op_conv_tile_name(int tile_id);
/* ---- the kernels at the two ends of the forward, one entry each (tests/test_gpu_head_tail.py).  d_* are the caller's DEVICE buffers, h_* HOST arrays in the
 * reference's shapes.  Every argument a kernel cannot take (NULL, a size below 1, a pointer of a 16-byte access that is not 16-byte aligned, the limits named
 * below) returns PF_ERR_ARG before any device work.  One launch on `stream`; the entries without host weights do not synchronise, those with host weights wait
 * for the stream before they free their uploaded copies, as every pf_op_* entry with host weights does. */
/* input normalisation (perspectivefields.py:234-236): y (B, H, W, 4) = ((x - mean) / std, channel 3 = 0); x uint8 (B, H, W, 3), or fp32 planar (B, 3, H, W) */
int pf_op_prep_u8(int device, const uint8_t* d_x, int B, int H, int W, const float* h_mean3, const float* h_std3 /*non-zero*/, float* d_y, void* stream);
int pf_op_prep_f32_nchw(int device, const float* d_x, int B, int H, int W, const float* h_mean3, const float* h_std3 /*non-zero*/, float* d_y, void* stream);
/* the stand-alone regression prediction heads (gravity_head.py:117,190-193; latitude_head.py:118,189-192): 32-channel features tg, tl (B, HW, 32) ->
 * pg (B, 2, HW) = F.normalize(tg wg^T + bg) (eps 1e-12), pl (B, HW) = clamp(tl wl^T + bl, -1, 1), and, when d_pn != NULL, pn (B HW, 4) = (g0, g1, lat, 0) */
int pf_op_pred_regression(int device, const float* d_tg, const float* d_tl, int B, int HW, const float* h_wg /*[2][32]*/, const float* h_bg /*[2]*/,
                          const float* h_wl /*[1][32]*/, const float* h_bl /*[1]*/, float* d_pg, float* d_pl, float* d_pn /*or NULL*/, void* stream);
/* argmax decode of the classification heads (utils/utils.py:114-130,148-162): logits (B, ng, HW) / (B, nl, HW) -> dg (B, 2, HW) = (cos, sin) of bin * 360 / (ng - 1) - 180
 * degrees, (0, 0) for the last ("invalid") bin; dl (B, HW) = -90 + (bin + 1/2) 180 / nl degrees.  The first maximum wins, as torch.argmax; ng >= 2, nl >= 1; NaN logits
 * are outside the contract. */
int pf_op_decode_cls(int device, const float* d_logit_g, int ng, const float* d_logit_l, int nl, int B, int HW, float* d_dg, float* d_dl, void* stream);
/* F.interpolate(x, (Ho, Wo)) in its default (legacy) 'nearest' mode on NHWC4 data (param_network.py:197): x (B, H, W, 4) -> y (B, Ho, Wo, 4), different buffers */
int pf_op_nearest_nhwc4(int device, const float* d_x, int B, int H, int W, int Ho, int Wo, float* d_y, void* stream);
/* the ConvNeXt tail (convnext.py:144-151): y (B, nout) = Linear(LayerNorm(mean over HW of x (B, HW, C))).  1 <= C <= 1024: the pooled row lives in a fixed LDS array. */
int pf_op_gap_ln_head(int device, const float* d_x, int B, int HW, int C, const float* h_gamma, const float* h_beta, float eps, const float* h_head_w /*[nout][C]*/,
                      const float* h_head_b, int nout, float* d_y, void* stream);
/* raw ParamNet outputs (B, nraw) -> (B, PF_PARAMS_STRIDE) (param_network.py:62-67 / 204-220).  mode 0 (needs nraw >= 4): raw 0..2 x 90, 1 / (2 tan raw2), raw 0..3;
 * mode 1: the raw values, zero padded, and for nraw == 5 column 5 = the relative focal length of the general vertical FoV 90 raw2 with centre (raw3, raw4).  nraw <= 8. */
int pf_op_paramnet_scalars(int device, const float* d_raw, int B, int nraw, int mode, float* d_out8, void* stream);
/* The conv whose epilogue applies a regression prediction head, in the form conv_fuse_conv1 runs without the fused x2 up-sampling: 3x3 / stride 1 / pad 1,
 * Cin (a multiple of 32) -> 32 channels, act, then head_kind 1: F.normalize(32 -> 2) into head_out (B, 2, H W) and floats 0-1 of each pn row; head_kind 2:
 * clamp(32 -> 1, -1, 1) into head_out (B, H W) and (lat, 0) into floats 2-3 of each pn row (pn (B H W, 4) or NULL; the other half of a row is not touched).
 * The 32-channel map is never stored.  Split-f16 scheme.  tile_id -1: the cost model's tile; a tile id that cannot run this form is PF_ERR_ARG, never replaced --
 * pf_op_conv2d_head_tile_usable (host only, no device needed) says which can: 1 / 0. */
int pf_op_conv2d_head_tile_usable(int B, int H, int W, int Cin, int act, int head_kind, int tile_id);
int pf_op_conv2d_head(int device, const float* d_x, int B, int H, int W, int Cin, const float* h_weight /*[32][Cin][3][3]*/, const float* h_bias /*[32] or NULL*/, int act,
                      int head_kind, const float* h_head_w /*[nout][32]*/, const float* h_head_b /*[nout]*/, int tile_id, float* d_head_out, float* d_pn /*or NULL*/,
                      void* stream);
/* The conv forms that only the forward's grouped launches set (tests/test_gpu_conv_forms.py): `groups` (1 or 2) problems of one shape in one grid, as the two decoder
 * heads run; ups = 1: the first input is stored at HALF resolution, (B, H/2, W/2, C1), and the conv runs on its bilinear x2 up-sampling (align_corners = False),
 * interpolated while the halo is staged -- H, W are the full-resolution size, d_x2 (C2 channels, concatenated behind) is at full resolution; bias_rows[g] = 9: h_bias[g]
 * is the [9][Cout] border-case table of a folded Linear -> zero-padded 3x3 pair, row 3 cy + cx with cy = 0 on the first output row, 2 on the last, 1 between, cx likewise
 * by column; head_kind[g] = 1 / 2: the prediction head of pf_op_conv2d_head in group g's epilogue (then d_y[g] is not used; d_pn[g] optional, both groups may give the same
 * buffer: kind 1 writes floats 0-1 of a row, kind 2 floats 2-3).  Every per-group argument is a HOST array of `groups` pointers (d_x2, h_bias, d_res1, d_res2, d_y, the
 * head arrays and d_pn may be NULL as a whole when no group uses them); shape, stride, pad, act, post_relu, ups, tile and precision (0 split-f16 or 3 exact bf16 split)
 * are shared.  Weights are packed as pf_op_conv2d packs them.  splitk_mode -1: split-K by the engine's rule (conv_splitk_factor), 0: never, N > 1: that factor where the
 * rule allows split-K at all; it runs on the linear split tiles only, and *splitk_used (optional) receives the factor the launch really used (1 = none).
 * Preconditions, each PF_ERR_ARG before any device work (no device is asked for, nothing uploaded, nothing launched) and never a fallback: groups 1 or 2; C1 and C2 multiples of 32; precision 0 or 3; ups needs even H and W and
 * precision 0; a bias table needs Ho >= 2 and Wo >= 2 (a pixel that is both the first and the last row or column is none of the nine cases); a fused head needs
 * Cout == 32, and either every group has one or none; a tile id that cannot run the form (pf_op_conv2d_g_tile_usable says which can, host logic only: 1 / 0; its
 * has_table and head_kind hold for every group), and tile_id -1 when the cost model's tile cannot run it. */
int pf_op_conv2d_g_tile_usable(int B, int H, int W, int C1, int C2, int Cout, int KH, int KW, int stride, int pad, int act, int groups, int ups, int has_table, int head_kind,
                               int precision, int tile_id);
int pf_op_conv2d_g(int device, int groups, const float* const* d_x, const float* const* d_x2, int B, int H, int W, int C1, int C2,
                   const float* const* h_weight /*[Cout][C1+C2][KH][KW] each*/, const float* const* h_bias /*[Cout] or [9][Cout] each, or NULL*/, const int* bias_rows /*1 or 9*/,
                   int Cout, int KH, int KW, int stride, int pad, int act, const float* const* d_res1, const float* const* d_res2, int post_relu, int ups,
                   float* const* d_y, const int* head_kind, const float* const* h_head_w, const float* const* h_head_b, float* const* d_head_out, float* const* d_pn,
                   int tile_id, int precision, int splitk_mode, int* splitk_used, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PF_HIP_H */
