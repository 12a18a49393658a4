// Camera-geometry entry points of libpf_hip.so that take no pf_handle and use nothing of the engine (include/pf_hip.h): fields from parameters, the image
// gathers (pano_crop.hip, reproject.hip, pano_compose.hip, pano_rotate.hip, gather_ss.hip, cube_gather.hip, fisheye_gather.hip, fisheye_target.hip), the field transports (field_transport.hip), the yaw moments (yaw_align.hip), the placement scores (place_score.hip), the field transforms and the placement search (field_xform.hip), the drawing of fields (draw_fields.hip), the pasting of objects (composite.hip), the camera fits (fit_lm.h) and the field errors (field_err.hip).  Host-side argument checks and launch loops only.
#include <type_traits>

#include "host_pack.h"

using namespace pf;
using namespace pf_host;

// every entry point is declared extern "C" in include/pf_hip.h

int pf_fields_from_params(int device, const float* d_cam5, int H, int W, float* d_up, float* d_lat, void* stream) {
  std::string err;
  int rc = check_device(device, &err);
  if (rc != PF_OK) { g_create_error = err; return rc; }
  if (!d_cam5 || !d_up || !d_lat || H <= 0 || W <= 0) { g_create_error = "pf_fields_from_params: bad argument"; return PF_ERR_ARG; }
  launch_fields_from_params(d_cam5, H, W, d_up, d_lat, static_cast<hipStream_t>(stream));
  if (hipGetLastError() != hipSuccess) { g_create_error = "pf_fields_from_params: kernel launch failed"; return PF_ERR_DEVICE; }
  return PF_OK;
}

// The host path of the one-source image gathers (gather.h): argument checks in one order, the launch's GatherDims, launch groups of Batch::MAX outputs.
// A gather names its sources and outputs in the messages and says what it requires beyond the sources, the index and the image
struct GatherKind {
  const char *name, *src, *out;     // "pf_pano_crop", "panorama", "crop"
  int min_side;                     // smallest source height and width
  const char *no_src, *no_required; // the messages for missing source lists and for missing required arguments
};

// `required`: the gather's own required pointers are there; `out_err`: NULL or what is wrong with its optional outputs; `extras_misalign`: non-zero when one
// of those is not aligned for its vector store; `rest(batch, i0)` sets the cameras and the optional outputs of the group that begins at output i0
template <class Batch, class Rest>
static int gather_run(const GatherKind& g, void (*launch)(const Batch&, int, hipStream_t), int device, int n_src, const void* const* src, const int32_t* src_hw,
                      int dtype, int B, const int32_t* index, bool required, int H, int W, void* d_img, const char* out_err, uintptr_t extras_misalign,
                      void* stream, Rest rest) {
  auto bad = [&g](const std::string& m) { g_create_error = std::string(g.name) + ": " + m; return PF_ERR_ARG; };
  if (n_src < 1 || !src || !src_hw) return bad(g.no_src);
  if (dtype != PF_PANO_U8 && dtype != PF_PANO_F32) return bad(fmt("unknown dtype %d", dtype));
  for (int k = 0; k < n_src; ++k) {
    if (!src[k]) return bad(fmt("NULL pointer of %s %d", g.src, k));
    if (src_hw[2 * k] < g.min_side || src_hw[2 * k + 1] < g.min_side)
      return bad(fmt("%s %d is %d x %d, smaller than %d x %d", g.src, k, src_hw[2 * k], src_hw[2 * k + 1], g.min_side, g.min_side));
  }
  if (B < 1 || !index || !required || !d_img) return bad(g.no_required);
  if (H < 1 || W < 1) return bad(fmt("output size %d x %d", H, W));
  if (out_err) return bad(out_err);
  for (int i = 0; i < B; ++i)
    if (index[i] < 0 || index[i] >= n_src) return bad(fmt("%s %d: %s index %d of %d", g.out, i, g.src, index[i], n_src));
  const int tpr = 16;  // a 64 x 16 pixel tile (DESIGN.md sections 11 and 17)
  const long tiles_x = (W + 4 * tpr - 1) / (4 * tpr), tiles_y = (H + 256 / tpr - 1) / (256 / tpr);
  if (tiles_x * tiles_y > INT32_MAX) return bad(fmt("output size %d x %d too large", H, W));
  std::string err;
  const int rc = check_device(device, &err);
  if (rc != PF_OK) { g_create_error = err; return rc; }
  const size_t esz = dtype == PF_PANO_U8 ? 1 : 4, npx = (size_t)H * W;
  const uintptr_t align = (reinterpret_cast<uintptr_t>(d_img) & (dtype == PF_PANO_U8 ? 3 : 15)) | extras_misalign;
  hipStream_t s = static_cast<hipStream_t>(stream);
  for (int i0 = 0; i0 < B; i0 += Batch::MAX) {
    Batch b;
    b.d = GatherDims{std::min(B - i0, (int)Batch::MAX), H, W, tpr, (int)tiles_x, (int)tiles_y, (W % 4 == 0 && align == 0) ? 1 : 0};
    for (int k = 0; k < b.d.n; ++k) {
      const int p = index[i0 + k];
      b.src.p[k] = src[p];
      b.src.H[k] = src_hw[2 * p]; b.src.W[k] = src_hw[2 * p + 1];
    }
    b.img = static_cast<char*>(d_img) + (size_t)i0 * npx * 3 * esz;
    rest(b, i0);
    launch(b, dtype, s);
  }
  if (hipGetLastError() != hipSuccess) { g_create_error = fmt("%s: kernel launch failed", g.name); return PF_ERR_DEVICE; }
  return PF_OK;
}

static uintptr_t misalign(const void* p, uintptr_t mask) { return reinterpret_cast<uintptr_t>(p) & mask; }

static bool samples_ok(const char* name, int samples) {
  if (samples >= 1 && samples <= PF_GATHER_MAX_SAMPLES) return true;
  g_create_error = fmt("%s: samples %d, must be in [1, %d]", name, samples, PF_GATHER_MAX_SAMPLES);
  return false;
}

// A gather and its supersampled form (gather_ss.hip) are one body under two names.  The batch type says which of the two runs: the form checks
// `samples` first and sets it in its batch, the parent has neither; then the parent's checks in the parent's order under the entry point's name
template <class Batch>
static int pano_crop_run(const char* name, void (*launch)(const Batch&, int, hipStream_t), int samples, int device, int n_pano, const void* const* pano,
                         const int32_t* pano_hw, int dtype, int B, const int32_t* pano_index, const float* d_cam7, int H, int W, void* d_img, float* d_up,
                         float* d_lat, void* stream) {
  constexpr bool ss = std::is_same<Batch, PanoSsBatch>::value;
  const GatherKind kind{name, "panorama", "crop", 2, "needs at least one panorama (h_pano, h_pano_hw)",
                        "batch >= 1, h_pano_index, d_cam7 and d_img are required"};
  if (ss && !samples_ok(name, samples)) return PF_ERR_ARG;
  const size_t npx = (size_t)H * W;
  return gather_run(kind, launch, device, n_pano, pano, pano_hw, dtype, B, pano_index, d_cam7 != nullptr, H, W, d_img,
                    !d_up != !d_lat ? "d_up and d_lat are both given or both NULL" : nullptr, misalign(d_up, 15) | misalign(d_lat, 15), stream,
                    [=](Batch& pb, int i0) {
                      if constexpr (ss) pb.samples = samples;
                      pb.cam = d_cam7 + (size_t)i0 * 7;
                      pb.up = d_up ? d_up + (size_t)i0 * 2 * npx : nullptr;
                      pb.lat = d_lat ? d_lat + (size_t)i0 * npx : nullptr;
                    });
}

int pf_pano_crop(int device, int n_pano, const void* const* pano, const int32_t* pano_hw, int dtype, int B, const int32_t* pano_index,
                 const float* d_cam7, int H, int W, void* d_img, float* d_up, float* d_lat, void* stream) {
  return pano_crop_run("pf_pano_crop", launch_pano_crop, 1, device, n_pano, pano, pano_hw, dtype, B, pano_index, d_cam7, H, W, d_img, d_up, d_lat, stream);
}

int pf_pano_crop_ss(int device, int n_pano, const void* const* pano, const int32_t* pano_hw, int dtype, int B, const int32_t* pano_index,
                    const float* d_cam7, int H, int W, void* d_img, float* d_up, float* d_lat, int samples, void* stream) {
  return pano_crop_run("pf_pano_crop_ss", launch_pano_crop_ss, samples, device, n_pano, pano, pano_hw, dtype, B, pano_index, d_cam7, H, W, d_img, d_up,
                       d_lat, stream);
}

template <class Batch>
static int reproject_run(const char* name, void (*launch)(const Batch&, int, hipStream_t), int samples, int device, int n_src, const void* const* src,
                         const int32_t* src_hw, int dtype, int B, const int32_t* src_index, const float* d_cam_src7, const float* d_cam_dst7, int H, int W,
                         float fill, void* d_img, uint8_t* d_valid, float* d_map, void* stream) {
  constexpr bool ss = std::is_same<Batch, ReprojSsBatch>::value;
  const GatherKind kind{name, "source", "output", 1, "needs at least one source image (h_src, h_src_hw)",
                        "batch >= 1, h_src_index, d_cam_src7, d_cam_dst7 and d_img are required"};
  if (ss && !samples_ok(name, samples)) return PF_ERR_ARG;
  const size_t npx = (size_t)H * W;
  return gather_run(kind, launch, device, n_src, src, src_hw, dtype, B, src_index, d_cam_src7 && d_cam_dst7, H, W, d_img, nullptr,
                    misalign(d_valid, 3) | misalign(d_map, 15), stream, [=](Batch& rb, int i0) {
                      if constexpr (ss) rb.samples = samples;
                      rb.fill = fill;
                      rb.cam_src = d_cam_src7 + (size_t)i0 * 7;
                      rb.cam_dst = d_cam_dst7 + (size_t)i0 * 7;
                      rb.valid = d_valid ? d_valid + (size_t)i0 * npx : nullptr;
                      rb.map = d_map ? d_map + (size_t)i0 * 2 * npx : nullptr;
                    });
}

int pf_reproject(int device, int n_src, const void* const* src, const int32_t* src_hw, int dtype, int B, const int32_t* src_index,
                 const float* d_cam_src7, const float* d_cam_dst7, int H, int W, float fill, void* d_img, uint8_t* d_valid, float* d_map, void* stream) {
  return reproject_run("pf_reproject", launch_reproject, 1, device, n_src, src, src_hw, dtype, B, src_index, d_cam_src7, d_cam_dst7, H, W, fill, d_img,
                       d_valid, d_map, stream);
}

int pf_reproject_ss(int device, int n_src, const void* const* src, const int32_t* src_hw, int dtype, int B, const int32_t* src_index,
                    const float* d_cam_src7, const float* d_cam_dst7, int H, int W, float fill, void* d_img, uint8_t* d_valid, float* d_map, int samples,
                    void* stream) {
  return reproject_run("pf_reproject_ss", launch_reproject_ss, samples, device, n_src, src, src_hw, dtype, B, src_index, d_cam_src7, d_cam_dst7, H, W, fill,
                       d_img, d_valid, d_map, stream);
}

template <class Batch>
static int pano_rotate_run(const char* name, void (*launch)(const Batch&, int, hipStream_t), int samples, int device, int n_pano, const void* const* pano,
                           const int32_t* pano_hw, int dtype, int B, const int32_t* pano_index, const float* d_rot3, int inverse, int H, int W, void* d_img,
                           float* d_up, float* d_lat, void* stream) {
  constexpr bool ss = std::is_same<Batch, PanoRotSsBatch>::value;
  const GatherKind kind{name, "panorama", "output", 2, "needs at least one panorama (h_pano, h_pano_hw)",
                        "batch >= 1, h_pano_index, d_rot3 and d_img are required"};
  if (ss && !samples_ok(name, samples)) return PF_ERR_ARG;
  const size_t npx = (size_t)H * W;
  return gather_run(kind, launch, device, n_pano, pano, pano_hw, dtype, B, pano_index, d_rot3 != nullptr, H, W, d_img,
                    !d_up != !d_lat ? "d_up and d_lat are both given or both NULL" : nullptr, misalign(d_up, 15) | misalign(d_lat, 15), stream,
                    [=](Batch& rb, int i0) {
                      if constexpr (ss) rb.samples = samples;
                      rb.inverse = inverse ? 1 : 0;
                      rb.rot = d_rot3 + (size_t)i0 * 3;
                      rb.up = d_up ? d_up + (size_t)i0 * 2 * npx : nullptr;
                      rb.lat = d_lat ? d_lat + (size_t)i0 * npx : nullptr;
                    });
}

int pf_pano_rotate(int device, int n_pano, const void* const* pano, const int32_t* pano_hw, int dtype, int B, const int32_t* pano_index,
                   const float* d_rot3, int inverse, int H, int W, void* d_img, float* d_up, float* d_lat, void* stream) {
  return pano_rotate_run("pf_pano_rotate", launch_pano_rotate, 1, device, n_pano, pano, pano_hw, dtype, B, pano_index, d_rot3, inverse, H, W, d_img, d_up,
                         d_lat, stream);
}

int pf_pano_rotate_ss(int device, int n_pano, const void* const* pano, const int32_t* pano_hw, int dtype, int B, const int32_t* pano_index,
                      const float* d_rot3, int inverse, int H, int W, void* d_img, float* d_up, float* d_lat, int samples, void* stream) {
  return pano_rotate_run("pf_pano_rotate_ss", launch_pano_rotate_ss, samples, device, n_pano, pano, pano_hw, dtype, B, pano_index, d_rot3, inverse, H, W,
                         d_img, d_up, d_lat, stream);
}

// Cube maps as the source (cube_gather.hip): `samples`, then that every cube is square, then gather_run's checks with the source size (N, N)
static bool cubes_square(const char* name, int n_cube, const int32_t* cube_hw) {
  for (int k = 0; cube_hw && k < n_cube; ++k)
    if (cube_hw[2 * k] != cube_hw[2 * k + 1]) {
      g_create_error = fmt("%s: cube %d has faces of %d x %d, they must be square", name, k, cube_hw[2 * k], cube_hw[2 * k + 1]);
      return false;
    }
  return true;
}

int pf_cube_crop(int device, int n_cube, const void* const* cube, const int32_t* cube_hw, int dtype, int B, const int32_t* cube_index, const float* d_cam7,
                 int H, int W, void* d_img, int samples, void* stream) {
  static const GatherKind kind{"pf_cube_crop", "cube", "view", 1, "needs at least one cube (h_cube, h_cube_hw)",
                               "batch >= 1, h_cube_index, d_cam7 and d_img are required"};
  if (!samples_ok(kind.name, samples) || !cubes_square(kind.name, n_cube, cube_hw)) return PF_ERR_ARG;
  return gather_run(kind, launch_cube_crop, device, n_cube, cube, cube_hw, dtype, B, cube_index, d_cam7 != nullptr, H, W, d_img, nullptr, 0, stream,
                    [=](CubeCropBatch& cb, int i0) {
                      cb.samples = samples;
                      cb.cam = d_cam7 + (size_t)i0 * 7;
                    });
}

int pf_cube_to_pano(int device, int n_cube, const void* const* cube, const int32_t* cube_hw, int dtype, int B, const int32_t* cube_index, const float* d_rot3,
                    int inverse, int H, int W, void* d_img, int samples, void* stream) {
  static const GatherKind kind{"pf_cube_to_pano", "cube", "output", 1, "needs at least one cube (h_cube, h_cube_hw)",
                               "batch >= 1, h_cube_index, d_rot3 and d_img are required"};
  if (!samples_ok(kind.name, samples) || !cubes_square(kind.name, n_cube, cube_hw)) return PF_ERR_ARG;
  return gather_run(kind, launch_cube_to_pano, device, n_cube, cube, cube_hw, dtype, B, cube_index, d_rot3 != nullptr, H, W, d_img, nullptr, 0, stream,
                    [=](CubePanoBatch& cb, int i0) {
                      cb.samples = samples;
                      cb.inverse = inverse ? 1 : 0;
                      cb.rot = d_rot3 + (size_t)i0 * 3;
                    });
}

// Fisheye frames as the source (fisheye_gather.hip): `samples`, then the projection kind, then gather_run's checks; the lenses are a required argument
static bool fisheye_kind_ok(const char* name, int kind) {
  if (kind == PF_FISHEYE_EQUIDISTANT || kind == PF_FISHEYE_EQUISOLID || kind == PF_FISHEYE_STEREOGRAPHIC) return true;
  g_create_error = fmt("%s: unknown projection kind %d", name, kind);
  return false;
}

int pf_fisheye_crop(int device, int n_frame, const void* const* frame, const int32_t* frame_hw, int dtype, int kind, int B, const int32_t* frame_index,
                    const float* d_lens, const float* d_cam7, int H, int W, float fill, void* d_img, uint8_t* d_valid, int samples, void* stream) {
  static const GatherKind gk{"pf_fisheye_crop", "frame", "view", 1, "needs at least one frame (h_frame, h_frame_hw)",
                             "batch >= 1, h_frame_index, d_lens, d_cam7 and d_img are required"};
  if (!samples_ok(gk.name, samples) || !fisheye_kind_ok(gk.name, kind)) return PF_ERR_ARG;
  const size_t npx = (size_t)H * W;
  return gather_run(gk, launch_fisheye_crop, device, n_frame, frame, frame_hw, dtype, B, frame_index, d_lens && d_cam7, H, W, d_img, nullptr,
                    misalign(d_valid, 3), stream, [=](FisheyeCropBatch& fb, int i0) {
                      fb.samples = samples;
                      fb.kind = kind;
                      fb.fill = fill;
                      fb.lens = d_lens + (size_t)i0 * PF_FISHEYE_MAX_LENSES * PF_FISHEYE_LENS_FLOATS;
                      fb.cam = d_cam7 + (size_t)i0 * 7;
                      fb.valid = d_valid ? d_valid + (size_t)i0 * npx : nullptr;
                    });
}

int pf_fisheye_to_pano(int device, int n_frame, const void* const* frame, const int32_t* frame_hw, int dtype, int kind, int B, const int32_t* frame_index,
                       const float* d_lens, const float* d_rot3, int inverse, int H, int W, float fill, void* d_img, uint8_t* d_valid, int samples,
                       void* stream) {
  static const GatherKind gk{"pf_fisheye_to_pano", "frame", "output", 1, "needs at least one frame (h_frame, h_frame_hw)",
                             "batch >= 1, h_frame_index, d_lens, d_rot3 and d_img are required"};
  if (!samples_ok(gk.name, samples) || !fisheye_kind_ok(gk.name, kind)) return PF_ERR_ARG;
  const size_t npx = (size_t)H * W;
  return gather_run(gk, launch_fisheye_to_pano, device, n_frame, frame, frame_hw, dtype, B, frame_index, d_lens && d_rot3, H, W, d_img, nullptr,
                    misalign(d_valid, 3), stream, [=](FisheyePanoBatch& fb, int i0) {
                      fb.samples = samples;
                      fb.kind = kind;
                      fb.fill = fill;
                      fb.inverse = inverse ? 1 : 0;
                      fb.lens = d_lens + (size_t)i0 * PF_FISHEYE_MAX_LENSES * PF_FISHEYE_LENS_FLOATS;
                      fb.rot = d_rot3 + (size_t)i0 * 3;
                      fb.valid = d_valid ? d_valid + (size_t)i0 * npx : nullptr;
                    });
}

// Fisheye frames as the target (fisheye_target.hip): `samples`, then the projection kind, then gather_run's checks with the panoramas as the sources
int pf_pano_to_fisheye(int device, int n_pano, const void* const* pano, const int32_t* pano_hw, int dtype, int kind, int B, const int32_t* pano_index,
                       const float* d_lens, int H, int W, float fill, void* d_img, uint8_t* d_valid, float* d_up, float* d_lat, int samples, void* stream) {
  static const GatherKind gk{"pf_pano_to_fisheye", "panorama", "frame", 2, "needs at least one panorama (h_pano, h_pano_hw)",
                             "batch >= 1, h_pano_index, d_lens and d_img are required"};
  if (!samples_ok(gk.name, samples) || !fisheye_kind_ok(gk.name, kind)) return PF_ERR_ARG;
  const size_t npx = (size_t)H * W;
  return gather_run(gk, launch_pano_to_fisheye, device, n_pano, pano, pano_hw, dtype, B, pano_index, d_lens != nullptr, H, W, d_img,
                    !d_up != !d_lat ? "d_up and d_lat are both given or both NULL" : nullptr,
                    misalign(d_valid, 3) | misalign(d_up, 15) | misalign(d_lat, 15), stream, [=](PanoToFisheyeBatch& fb, int i0) {
                      fb.samples = samples;
                      fb.kind = kind;
                      fb.fill = fill;
                      fb.lens = d_lens + (size_t)i0 * PF_FISHEYE_MAX_LENSES * PF_FISHEYE_LENS_FLOATS;
                      fb.valid = d_valid ? d_valid + (size_t)i0 * npx : nullptr;
                      fb.up = d_up ? d_up + (size_t)i0 * 2 * npx : nullptr;
                      fb.lat = d_lat ? d_lat + (size_t)i0 * npx : nullptr;
                    });
}

// the labels of pf_pano_to_fisheye without a source: the projection kind, then its checks that concern the outputs, its tile and its launch groups
int pf_fisheye_fields(int device, int kind, int B, const float* d_lens, int H, int W, float* d_up, float* d_lat, void* stream) {
  auto bad = [](const std::string& m) { g_create_error = "pf_fisheye_fields: " + m; return PF_ERR_ARG; };
  if (!fisheye_kind_ok("pf_fisheye_fields", kind)) return PF_ERR_ARG;
  if (B < 1 || !d_lens || !d_up || !d_lat) return bad("batch >= 1, d_lens, d_up and d_lat are required");
  if (H < 1 || W < 1) return bad(fmt("output size %d x %d", H, W));
  const int tpr = 16;  // a 64 x 16 pixel tile, as the gathers
  const long tiles_x = (W + 4 * tpr - 1) / (4 * tpr), tiles_y = (H + 256 / tpr - 1) / (256 / tpr);
  if (tiles_x * tiles_y > INT32_MAX) return bad(fmt("output size %d x %d too large", H, W));
  std::string err;
  const int rc = check_device(device, &err);
  if (rc != PF_OK) { g_create_error = err; return rc; }
  const size_t npx = (size_t)H * W;
  const int vec = (W % 4 == 0 && (misalign(d_up, 15) | misalign(d_lat, 15)) == 0) ? 1 : 0;
  hipStream_t s = static_cast<hipStream_t>(stream);
  for (int i0 = 0; i0 < B; i0 += FisheyeFieldsBatch::MAX) {
    FisheyeFieldsBatch fb;
    fb.d = GatherDims{std::min(B - i0, (int)FisheyeFieldsBatch::MAX), H, W, tpr, (int)tiles_x, (int)tiles_y, vec};
    fb.kind = kind;
    fb.lens = d_lens + (size_t)i0 * PF_FISHEYE_MAX_LENSES * PF_FISHEYE_LENS_FLOATS;
    fb.up = d_up + (size_t)i0 * 2 * npx;
    fb.lat = d_lat + (size_t)i0 * npx;
    launch_fisheye_fields(fb, s);
  }
  if (hipGetLastError() != hipSuccess) { g_create_error = "pf_fisheye_fields: kernel launch failed"; return PF_ERR_DEVICE; }
  return PF_OK;
}

// the labels of pf_pano_rotate without a source: its checks that concern the outputs, its tile and its launch groups
int pf_pano_fields(int device, int B, const float* d_rot3, int inverse, int H, int W, float* d_up, float* d_lat, void* stream) {
  auto bad = [](const std::string& m) { g_create_error = "pf_pano_fields: " + m; return PF_ERR_ARG; };
  if (B < 1 || !d_rot3 || !d_up || !d_lat) return bad("batch >= 1, d_rot3, d_up and d_lat are required");
  if (H < 1 || W < 1) return bad(fmt("output size %d x %d", H, W));
  const int tpr = 16;  // a 64 x 16 pixel tile, as the gathers
  const long tiles_x = (W + 4 * tpr - 1) / (4 * tpr), tiles_y = (H + 256 / tpr - 1) / (256 / tpr);
  if (tiles_x * tiles_y > INT32_MAX) return bad(fmt("output size %d x %d too large", H, W));
  std::string err;
  const int rc = check_device(device, &err);
  if (rc != PF_OK) { g_create_error = err; return rc; }
  const size_t npx = (size_t)H * W;
  const int vec = (W % 4 == 0 && (misalign(d_up, 15) | misalign(d_lat, 15)) == 0) ? 1 : 0;
  hipStream_t s = static_cast<hipStream_t>(stream);
  for (int i0 = 0; i0 < B; i0 += PanoFieldsBatch::MAX) {
    PanoFieldsBatch fb;
    fb.d = GatherDims{std::min(B - i0, (int)PanoFieldsBatch::MAX), H, W, tpr, (int)tiles_x, (int)tiles_y, vec};
    fb.inverse = inverse ? 1 : 0;
    fb.rot = d_rot3 + (size_t)i0 * 3;
    fb.up = d_up + (size_t)i0 * 2 * npx;
    fb.lat = d_lat + (size_t)i0 * npx;
    launch_pano_fields(fb, s);
  }
  if (hipGetLastError() != hipSuccess) { g_create_error = "pf_pano_fields: kernel launch failed"; return PF_ERR_DEVICE; }
  return PF_OK;
}

// Several views per output, so not gather_run: the launches follow the panoramas, not the sources.  Panoramas share a launch while it holds at most
// ComposeBatch::MAX views and MAX panoramas; a panorama of more views takes launches of its own that hand (C, S) on through d_acc
int pf_pano_compose(int device, int n_view, const void* const* view, const int32_t* view_hw, int dtype, const int32_t* view_pano, const float* d_cam7,
                    int n_pano, int Hp, int Wp, int blend, float fill, void* d_pano, float* d_weight, float* d_acc, void* stream) {
  auto bad = [](const std::string& m) { g_create_error = "pf_pano_compose: " + m; return PF_ERR_ARG; };
  constexpr int MAX = ComposeBatch::MAX;
  if (n_view < 1 || !view || !view_hw) return bad("needs at least one view (h_view, h_view_hw)");
  if (dtype != PF_PANO_U8 && dtype != PF_PANO_F32) return bad(fmt("unknown dtype %d", dtype));
  if (blend != PF_BLEND_FEATHER && blend != PF_BLEND_MEAN) return bad(fmt("unknown blend %d", blend));
  for (int k = 0; k < n_view; ++k) {
    if (!view[k]) return bad(fmt("NULL pointer of view %d", k));
    if (view_hw[2 * k] < 1 || view_hw[2 * k + 1] < 1) return bad(fmt("view %d is %d x %d, smaller than 1 x 1", k, view_hw[2 * k], view_hw[2 * k + 1]));
  }
  if (n_pano < 1 || !view_pano || !d_cam7 || !d_pano) return bad("n_pano >= 1, h_view_pano, d_cam7 and d_pano are required");
  if (Hp < 1 || Wp < 1) return bad(fmt("panorama size %d x %d", Hp, Wp));
  std::vector<int> count(n_pano, 0);
  for (int k = 0; k < n_view; ++k) {
    if (view_pano[k] < 0 || view_pano[k] >= n_pano) return bad(fmt("view %d: panorama index %d of %d", k, view_pano[k], n_pano));
    if (k > 0 && view_pano[k] < view_pano[k - 1]) return bad(fmt("view %d: panorama index %d after %d, the indices must not decrease", k, view_pano[k], view_pano[k - 1]));
    ++count[view_pano[k]];
  }
  const bool carry = *std::max_element(count.begin(), count.end()) > MAX;
  if (carry && !d_acc) return bad(fmt("d_acc is required: a panorama has more than %d views", MAX));
  if (carry && misalign(d_acc, 15)) return bad("d_acc must be aligned to 16 bytes");
  const int tpr = 16;  // a 64 x 16 pixel tile, as the other gathers
  const long tiles_x = (Wp + 4 * tpr - 1) / (4 * tpr), tiles_y = (Hp + 256 / tpr - 1) / (256 / tpr);
  if (tiles_x * tiles_y > INT32_MAX) return bad(fmt("panorama size %d x %d too large", Hp, Wp));
  std::string err;
  const int rc = check_device(device, &err);
  if (rc != PF_OK) { g_create_error = err; return rc; }
  const size_t esz = dtype == PF_PANO_U8 ? 1 : 4, npx = (size_t)Hp * Wp;
  const int vec = (Wp % 4 == 0 && (misalign(d_pano, dtype == PF_PANO_U8 ? 3 : 15) | misalign(d_weight, 15)) == 0) ? 1 : 0;
  hipStream_t s = static_cast<hipStream_t>(stream);
  // the launch of the panoramas [p0, p0 + np) that reads the views [v0, v0 + nv): all views of those panoramas, or (np == 1) one slice of a panorama's
  auto launch = [&](int p0, int np, int v0, int nv, uint32_t carry_in, uint32_t carry_out) {
    ComposeBatch cb;
    cb.d = GatherDims{np, Hp, Wp, tpr, (int)tiles_x, (int)tiles_y, vec};
    cb.fill = fill;
    for (int k = 0; k < nv; ++k) {
      cb.src.p[k] = view[v0 + k];
      cb.src.H[k] = view_hw[2 * (v0 + k)]; cb.src.W[k] = view_hw[2 * (v0 + k) + 1];
    }
    cb.cam = d_cam7 + (size_t)v0 * 7;
    for (int k = 0, f = 0; k < np; ++k) {
      cb.first[k] = f;
      cb.count[k] = np == 1 ? nv : count[p0 + k];
      f += cb.count[k];
    }
    cb.carry_in = carry_in; cb.carry_out = carry_out;
    cb.img = static_cast<char*>(d_pano) + (size_t)p0 * npx * 3 * esz;
    cb.weight = d_weight ? d_weight + (size_t)p0 * npx : nullptr;
    cb.acc = d_acc ? d_acc + (size_t)p0 * npx * 4 : nullptr;
    launch_pano_compose(cb, dtype, blend, s);
  };
  int p0 = 0, np = 0, v0 = 0, nv = 0;  // the shared launch being filled
  for (int p = 0, v = 0; p < n_pano; v += count[p], ++p) {
    const int c = count[p];
    if (np > 0 && (c > MAX || nv + c > MAX || np == MAX)) { launch(p0, np, v0, nv, 0u, 0u); np = nv = 0; }
    if (c > MAX) {
      for (int i = 0; i < c; i += MAX) launch(p, 1, v + i, std::min(c - i, MAX), i > 0 ? 1u : 0u, i + MAX < c ? 1u : 0u);
      continue;
    }
    if (np == 0) { p0 = p; v0 = v; }
    ++np; nv += c;
  }
  if (np > 0) launch(p0, np, v0, nv, 0u, 0u);
  if (hipGetLastError() != hipSuccess) { g_create_error = "pf_pano_compose: kernel launch failed"; return PF_ERR_DEVICE; }
  return PF_OK;
}

// The field transports (field_transport.hip): pf_reproject's and pf_pano_compose's launch loops with pairs of field planes as the sources.  NULL, or
// what is wrong with the `n` sources (`noun`s) whose sides must be at least 2: the latitude grid needs size - 1 > 0
static const char* field_sources_error(const char* noun, int n, const float* const* up, const float* const* lat, const int32_t* hw, std::string* why) {
  for (int k = 0; k < n; ++k) {
    if (!up[k] || !lat[k]) { *why = fmt("NULL field pointer of %s %d", noun, k); return why->c_str(); }
    if (hw[2 * k] < 2 || hw[2 * k + 1] < 2) { *why = fmt("%s %d is %d x %d, smaller than 2 x 2", noun, k, hw[2 * k], hw[2 * k + 1]); return why->c_str(); }
  }
  return nullptr;
}

int pf_reproject_fields(int device, int n_src, const float* const* src_up, const float* const* src_lat, const int32_t* src_hw, int B, const int32_t* src_index,
                        const float* d_cam_src7, const float* d_cam_dst7, int H, int W, float* d_up, float* d_lat, void* stream) {
  auto bad = [](const std::string& m) { g_create_error = "pf_reproject_fields: " + m; return PF_ERR_ARG; };
  std::string why;
  if (n_src < 1 || !src_up || !src_lat || !src_hw) return bad("needs at least one source field (h_src_up, h_src_lat, h_src_hw)");
  if (const char* e = field_sources_error("source", n_src, src_up, src_lat, src_hw, &why)) return bad(e);
  if (B < 1 || !src_index || !d_cam_src7 || !d_cam_dst7 || !d_up || !d_lat) return bad("batch >= 1, h_src_index, d_cam_src7, d_cam_dst7, d_up and d_lat are required");
  if (H < 2 || W < 2) return bad(fmt("output size %d x %d, smaller than 2 x 2", H, W));
  for (int i = 0; i < B; ++i)
    if (src_index[i] < 0 || src_index[i] >= n_src) return bad(fmt("output %d: source index %d of %d", i, src_index[i], n_src));
  const int tpr = 16;  // a 64 x 16 pixel tile, as the other gathers
  const long tiles_x = (W + 4 * tpr - 1) / (4 * tpr), tiles_y = (H + 256 / tpr - 1) / (256 / tpr);
  if (tiles_x * tiles_y > INT32_MAX) return bad(fmt("output size %d x %d too large", H, W));
  std::string err;
  const int rc = check_device(device, &err);
  if (rc != PF_OK) { g_create_error = err; return rc; }
  const size_t npx = (size_t)H * W;
  const int vec = (W % 4 == 0 && (misalign(d_up, 15) | misalign(d_lat, 15)) == 0) ? 1 : 0;
  hipStream_t s = static_cast<hipStream_t>(stream);
  for (int i0 = 0; i0 < B; i0 += FieldReprojBatch::MAX) {
    FieldReprojBatch rb;
    rb.d = GatherDims{std::min(B - i0, (int)FieldReprojBatch::MAX), H, W, tpr, (int)tiles_x, (int)tiles_y, vec};
    for (int k = 0; k < rb.d.n; ++k) {
      const int p = src_index[i0 + k];
      rb.src.up[k] = src_up[p]; rb.src.lat[k] = src_lat[p];
      rb.src.H[k] = src_hw[2 * p]; rb.src.W[k] = src_hw[2 * p + 1];
    }
    rb.cam_src = d_cam_src7 + (size_t)i0 * 7;
    rb.cam_dst = d_cam_dst7 + (size_t)i0 * 7;
    rb.up = d_up + (size_t)i0 * 2 * npx;
    rb.lat = d_lat + (size_t)i0 * npx;
    launch_reproject_fields(rb, s);
  }
  if (hipGetLastError() != hipSuccess) { g_create_error = "pf_reproject_fields: kernel launch failed"; return PF_ERR_DEVICE; }
  return PF_OK;
}

// Panoramas share a launch while it holds at most FieldComposeBatch::MAX views and MAX panoramas, as in pf_pano_compose; a panorama of more views is
// an argument error: there is no accumulator path
int pf_compose_fields(int device, int n_view, const float* const* view_up, const float* const* view_lat, const int32_t* view_hw, const int32_t* view_pano,
                      const float* d_cam7, int n_pano, int Hp, int Wp, int blend, float* d_up, float* d_lat, float* d_weight, void* stream) {
  auto bad = [](const std::string& m) { g_create_error = "pf_compose_fields: " + m; return PF_ERR_ARG; };
  constexpr int MAX = FieldComposeBatch::MAX;
  std::string why;
  if (n_view < 1 || !view_up || !view_lat || !view_hw) return bad("needs at least one view (h_view_up, h_view_lat, h_view_hw)");
  if (blend != PF_BLEND_FEATHER && blend != PF_BLEND_MEAN) return bad(fmt("unknown blend %d", blend));
  if (const char* e = field_sources_error("view", n_view, view_up, view_lat, view_hw, &why)) return bad(e);
  if (n_pano < 1 || !view_pano || !d_cam7 || !d_up || !d_lat) return bad("n_pano >= 1, h_view_pano, d_cam7, d_up and d_lat are required");
  if (Hp < 1 || Wp < 1) return bad(fmt("panorama size %d x %d", Hp, Wp));
  std::vector<int> count(n_pano, 0);
  for (int k = 0; k < n_view; ++k) {
    if (view_pano[k] < 0 || view_pano[k] >= n_pano) return bad(fmt("view %d: panorama index %d of %d", k, view_pano[k], n_pano));
    if (k > 0 && view_pano[k] < view_pano[k - 1]) return bad(fmt("view %d: panorama index %d after %d, the indices must not decrease", k, view_pano[k], view_pano[k - 1]));
    ++count[view_pano[k]];
  }
  for (int p = 0; p < n_pano; ++p)
    if (count[p] > MAX) return bad(fmt("panorama %d has %d views, more than %d views per panorama", p, count[p], MAX));
  const int tpr = 16;  // a 64 x 16 pixel tile, as the other gathers
  const long tiles_x = (Wp + 4 * tpr - 1) / (4 * tpr), tiles_y = (Hp + 256 / tpr - 1) / (256 / tpr);
  if (tiles_x * tiles_y > INT32_MAX) return bad(fmt("panorama size %d x %d too large", Hp, Wp));
  std::string err;
  const int rc = check_device(device, &err);
  if (rc != PF_OK) { g_create_error = err; return rc; }
  const size_t npx = (size_t)Hp * Wp;
  const int vec = (Wp % 4 == 0 && (misalign(d_up, 15) | misalign(d_lat, 15) | misalign(d_weight, 15)) == 0) ? 1 : 0;
  hipStream_t s = static_cast<hipStream_t>(stream);
  auto launch = [&](int p0, int np, int v0, int nv) {  // the panoramas [p0, p0 + np), whose views are [v0, v0 + nv)
    FieldComposeBatch cb;
    cb.d = GatherDims{np, Hp, Wp, tpr, (int)tiles_x, (int)tiles_y, vec};
    for (int k = 0; k < nv; ++k) {
      cb.src.up[k] = view_up[v0 + k]; cb.src.lat[k] = view_lat[v0 + k];
      cb.src.H[k] = view_hw[2 * (v0 + k)]; cb.src.W[k] = view_hw[2 * (v0 + k) + 1];
    }
    cb.cam = d_cam7 + (size_t)v0 * 7;
    for (int k = 0, f = 0; k < np; ++k) {
      cb.first[k] = f;
      cb.count[k] = count[p0 + k];
      f += cb.count[k];
    }
    cb.up = d_up + (size_t)p0 * 2 * npx;
    cb.lat = d_lat + (size_t)p0 * npx;
    cb.weight = d_weight ? d_weight + (size_t)p0 * npx : nullptr;
    launch_compose_fields(cb, blend, s);
  };
  int p0 = 0, np = 0, v0 = 0, nv = 0;  // the launch being filled
  for (int p = 0, v = 0; p < n_pano; v += count[p], ++p) {
    if (np > 0 && (nv + count[p] > MAX || np == MAX)) { launch(p0, np, v0, nv); np = nv = 0; }
    if (np == 0) { p0 = p; v0 = v; }
    ++np; nv += count[p];
  }
  if (np > 0) launch(p0, np, v0, nv);
  if (hipGetLastError() != hipSuccess) { g_create_error = "pf_compose_fields: kernel launch failed"; return PF_ERR_DEVICE; }
  return PF_OK;
}

// pf_yaw_moments: workspace = every view's luminance plane, then the tiles' partial records of every pair, each region 256-byte aligned
static constexpr int kYawMaxCand = PF_YAW_MAX_CAND;
static size_t yaw_align(size_t n) { return (n + 255) & ~(size_t)255; }
static long long yaw_samples(int H, int W, int stride) { return (long long)((H + stride - 1) / stride) * ((W + stride - 1) / stride); }
// NULL, or what is wrong with the arguments that set the workspace's layout
static const char* yaw_layout_error(int n_view, const int32_t* view_hw, int n_pair, const int32_t* pairs, int n_cand, int stride, std::string* why) {
  if (n_view < 2 || !view_hw) return "needs at least two views (h_view, h_view_hw)";
  if (n_pair < 1 || !pairs) return "n_pair >= 1 and h_pairs are required";
  if (n_cand < 1 || n_cand > kYawMaxCand) { *why = fmt("n_cand %d, must be in [1, %d]", n_cand, kYawMaxCand); return why->c_str(); }
  if (stride < 1) { *why = fmt("stride %d, must be >= 1", stride); return why->c_str(); }
  for (int k = 0; k < n_view; ++k)
    if (view_hw[2 * k] < 1 || view_hw[2 * k + 1] < 1 || (long long)view_hw[2 * k] * view_hw[2 * k + 1] > INT32_MAX) {
      *why = fmt("view %d is %d x %d, smaller than 1 x 1 or of 2^31 pixels or more", k, view_hw[2 * k], view_hw[2 * k + 1]);
      return why->c_str();
    }
  for (int i = 0; i < n_pair; ++i) {
    const int a = pairs[2 * i], b = pairs[2 * i + 1];
    if (a < 0 || a >= n_view || b < 0 || b >= n_view) { *why = fmt("pair %d: view index (%d, %d) of %d", i, a, b, n_view); return why->c_str(); }
    if (a == b) { *why = fmt("pair %d: a == b (%d), a pair needs two views", i, a); return why->c_str(); }
  }
  return nullptr;
}
static int yaw_tiles(const int32_t* view_hw, int b, int stride) {
  return (int)((yaw_samples(view_hw[2 * b], view_hw[2 * b + 1], stride) + YawBatch::TILE - 1) / YawBatch::TILE);
}

size_t pf_yaw_moments_workspace_bytes(int n_view, const int32_t* view_hw, int n_pair, const int32_t* pairs, int n_cand, int stride) {
  std::string why;
  if (yaw_layout_error(n_view, view_hw, n_pair, pairs, n_cand, stride, &why)) return 0;
  size_t n = 256, tiles = 0;  // + 256: alignment of the caller's pointer
  for (int k = 0; k < n_view; ++k) n += yaw_align((size_t)view_hw[2 * k] * view_hw[2 * k + 1] * sizeof(float));
  for (int i = 0; i < n_pair; ++i) tiles += (size_t)yaw_tiles(view_hw, pairs[2 * i + 1], stride);
  if (tiles > (size_t)INT32_MAX) return 0;
  return n + yaw_align(tiles * n_cand * 6 * sizeof(float));
}

int pf_yaw_moments(int device, int n_view, const void* const* view, const int32_t* view_hw, int dtype, const float* d_cam6, int n_pair, const int32_t* pairs,
                   int n_cand, const float* d_cand, int stride, double* d_moments, void* ws, size_t ws_bytes, void* stream) {
  auto bad = [](const std::string& m) { g_create_error = "pf_yaw_moments: " + m; return PF_ERR_ARG; };
  std::string why;
  if (const char* e = yaw_layout_error(n_view, view_hw, n_pair, pairs, n_cand, stride, &why)) return bad(e);
  if (!view) return bad("needs at least two views (h_view, h_view_hw)");
  if (dtype != PF_PANO_U8 && dtype != PF_PANO_F32) return bad(fmt("unknown dtype %d", dtype));
  for (int k = 0; k < n_view; ++k)
    if (!view[k]) return bad(fmt("NULL pointer of view %d", k));
  if (!d_cam6 || !d_cand || !d_moments) return bad("d_cam6, d_cand and d_moments are required");
  if (misalign(d_moments, 15)) return bad("d_moments must be aligned to 16 bytes");
  const size_t need = pf_yaw_moments_workspace_bytes(n_view, view_hw, n_pair, pairs, n_cand, stride);
  if (need == 0) return bad("too many tiles: the pairs' samples / 1024 must stay below 2^31");
  if (!ws || ws_bytes < need) return bad(fmt("needs %zu workspace bytes, got %zu", need, ws_bytes));
  std::string err;
  const int rc = check_device(device, &err);
  if (rc != PF_OK) { g_create_error = err; return rc; }
  char* p = reinterpret_cast<char*>((reinterpret_cast<uintptr_t>(ws) + 255) & ~(uintptr_t)255);
  hipStream_t s = static_cast<hipStream_t>(stream);
  std::vector<float*> lum(n_view);
  for (int v0 = 0; v0 < n_view; v0 += YawLum::MAX) {
    YawLum yl;
    yl.n = std::min(n_view - v0, (int)YawLum::MAX);
    yl.c = dtype == PF_PANO_U8 ? 127.5f : 0.5f;
    for (int k = 0; k < yl.n; ++k) {
      const int v = v0 + k;
      yl.src.p[k] = view[v];
      yl.src.H[k] = view_hw[2 * v]; yl.src.W[k] = view_hw[2 * v + 1];
      yl.out[k] = lum[v] = reinterpret_cast<float*>(p);
      p += yaw_align((size_t)view_hw[2 * v] * view_hw[2 * v + 1] * sizeof(float));
    }
    launch_yaw_luminance(yl, dtype, s);
  }
  unsigned tile0 = 0;
  for (int i0 = 0; i0 < n_pair; i0 += YawBatch::MAX) {
    YawBatch yb;
    yb.n = std::min(n_pair - i0, (int)YawBatch::MAX);
    yb.n_cand = n_cand; yb.stride = stride; yb.max_tiles = 0;
    yb.cam = d_cam6; yb.cand = d_cand;
    yb.part = reinterpret_cast<float*>(p);
    yb.moments = d_moments + (size_t)i0 * n_cand * 6;
    for (int k = 0; k < yb.n; ++k) {
      const int a = pairs[2 * (i0 + k)], b = pairs[2 * (i0 + k) + 1];
      const int tiles = yaw_tiles(view_hw, b, stride);
      yb.pr[k] = YawPair{lum[a], lum[b], view_hw[2 * a], view_hw[2 * a + 1], view_hw[2 * b], view_hw[2 * b + 1], a, b, tile0, tiles};
      yb.max_tiles = std::max(yb.max_tiles, tiles);
      tile0 += (unsigned)tiles;
    }
    launch_yaw_moments(yb, s);
    launch_yaw_sum(yb, s);
  }
  if (hipGetLastError() != hipSuccess) { g_create_error = "pf_yaw_moments: kernel launch failed"; return PF_ERR_DEVICE; }
  return PF_OK;
}

// pf_place_scores: workspace = every field's packed plane (backgrounds, then objects), then the chunks' partial records of every pair, each region
// 256-byte aligned
struct PlaceDims { int P, Q, chunks; };
// NULL, or what is wrong with the arguments that set the workspace's layout
static const char* place_layout_error(int n_bg, const int32_t* bg_hw, int n_obj, const int32_t* obj_hw, int n_pair, const int32_t* pairs, int stride,
                                      std::string* why) {
  if (n_bg < 1 || !bg_hw) return "n_bg >= 1 and h_bg_hw are required";
  if (n_obj < 1 || !obj_hw) return "n_obj >= 1 and h_obj_hw are required";
  if (n_pair < 1 || !pairs) return "n_pair >= 1 and h_pairs are required";
  if (stride < 1) { *why = fmt("stride %d, must be >= 1", stride); return why->c_str(); }
  for (int f = 0; f < n_bg + n_obj; ++f) {
    const int32_t* hw = f < n_bg ? bg_hw + 2 * f : obj_hw + 2 * (f - n_bg);
    if (hw[0] < 1 || hw[1] < 1 || (long long)hw[0] * hw[1] > INT32_MAX) {
      *why = fmt("%s %d is %d x %d, smaller than 1 x 1 or of 2^31 pixels or more", f < n_bg ? "background" : "object", f < n_bg ? f : f - n_bg, hw[0], hw[1]);
      return why->c_str();
    }
  }
  for (int k = 0; k < n_pair; ++k) {
    const int b = pairs[2 * k], o = pairs[2 * k + 1];
    if (b < 0 || b >= n_bg || o < 0 || o >= n_obj) {
      *why = fmt("pair %d: index (%d, %d) of (%d backgrounds, %d objects)", k, b, o, n_bg, n_obj);
      return why->c_str();
    }
    if (obj_hw[2 * o] > bg_hw[2 * b] || obj_hw[2 * o + 1] > bg_hw[2 * b + 1]) {
      *why = fmt("pair %d: the object (%d x %d) is larger than its background (%d x %d)", k, obj_hw[2 * o], obj_hw[2 * o + 1], bg_hw[2 * b], bg_hw[2 * b + 1]);
      return why->c_str();
    }
    if (((long long)obj_hw[2 * o] * obj_hw[2 * o + 1] + PlaceBatch::CHUNK - 1) / PlaceBatch::CHUNK > 65535) {
      *why = fmt("pair %d: the object (%d x %d) has more than 65535 chunks of %d pixels", k, obj_hw[2 * o], obj_hw[2 * o + 1], (int)PlaceBatch::CHUNK);
      return why->c_str();
    }
  }
  return nullptr;
}
static PlaceDims place_dims(const int32_t* bg_hw, const int32_t* obj_hw, const int32_t* pair, int stride) {
  const int32_t *b = bg_hw + 2 * pair[0], *o = obj_hw + 2 * pair[1];
  return PlaceDims{(b[0] - o[0]) / stride + 1, (b[1] - o[1]) / stride + 1, (int)(((long long)o[0] * o[1] + PlaceBatch::CHUNK - 1) / PlaceBatch::CHUNK)};
}
static size_t place_plane_bytes(const int32_t* hw) { return yaw_align((size_t)hw[0] * hw[1] * sizeof(float2)); }

size_t pf_place_scores_workspace_bytes(int n_bg, const int32_t* bg_hw, int n_obj, const int32_t* obj_hw, int n_pair, const int32_t* pairs, int stride) {
  std::string why;
  if (place_layout_error(n_bg, bg_hw, n_obj, obj_hw, n_pair, pairs, stride, &why)) return 0;
  size_t n = 256, rec = 0;  // + 256: alignment of the caller's pointer
  for (int f = 0; f < n_bg; ++f) n += place_plane_bytes(bg_hw + 2 * f);
  for (int f = 0; f < n_obj; ++f) n += place_plane_bytes(obj_hw + 2 * f);
  for (int k = 0; k < n_pair; ++k) {
    const PlaceDims d = place_dims(bg_hw, obj_hw, pairs + 2 * k, stride);
    rec += (size_t)d.P * d.Q * d.chunks;
  }
  return n + yaw_align(rec * 3 * sizeof(float));
}

int pf_place_scores(int device, int n_bg, const float* const* bg_up, const float* const* bg_lat, const int32_t* bg_hw, int n_obj, const float* const* obj_up,
                    const float* const* obj_lat, const int32_t* obj_hw, int n_pair, const int32_t* pairs, int stride, double* d_out, void* ws, size_t ws_bytes,
                    void* stream) {
  auto bad = [](const std::string& m) { g_create_error = "pf_place_scores: " + m; return PF_ERR_ARG; };
  std::string why;
  if (const char* e = place_layout_error(n_bg, bg_hw, n_obj, obj_hw, n_pair, pairs, stride, &why)) return bad(e);
  if (!bg_up || !bg_lat || !obj_up || !obj_lat || !d_out) return bad("h_bg_up, h_bg_lat, h_obj_up, h_obj_lat and d_out are required");
  for (int f = 0; f < n_bg; ++f)
    if (!bg_up[f] || !bg_lat[f]) return bad(fmt("NULL field pointer of background %d", f));
  for (int f = 0; f < n_obj; ++f)
    if (!obj_up[f] || !obj_lat[f]) return bad(fmt("NULL field pointer of object %d", f));
  if (misalign(d_out, 7)) return bad("d_out must be aligned to 8 bytes");
  const size_t need = pf_place_scores_workspace_bytes(n_bg, bg_hw, n_obj, obj_hw, n_pair, pairs, stride);
  if (!ws || ws_bytes < need) return bad(fmt("needs %zu workspace bytes, got %zu", need, ws_bytes));
  std::string err;
  const int rc = check_device(device, &err);
  if (rc != PF_OK) { g_create_error = err; return rc; }
  char* p = reinterpret_cast<char*>((reinterpret_cast<uintptr_t>(ws) + 255) & ~(uintptr_t)255);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int n_field = n_bg + n_obj;
  std::vector<float2*> plane(n_field);  // backgrounds, then objects
  for (int f0 = 0; f0 < n_field; f0 += PlacePack::MAX) {
    PlacePack pp;
    pp.n = std::min(n_field - f0, (int)PlacePack::MAX);
    for (int k = 0; k < pp.n; ++k) {
      const int f = f0 + k;
      const int32_t* hw = f < n_bg ? bg_hw + 2 * f : obj_hw + 2 * (f - n_bg);
      pp.npx[k] = hw[0] * hw[1];
      pp.up[k] = f < n_bg ? bg_up[f] : obj_up[f - n_bg];
      pp.lat[k] = f < n_bg ? bg_lat[f] : obj_lat[f - n_bg];
      pp.out[k] = plane[f] = reinterpret_cast<float2*>(p);
      p += place_plane_bytes(hw);
    }
    launch_place_pack(pp, s);
  }
  size_t part0 = 0, out0 = 0;
  for (int i0 = 0; i0 < n_pair; i0 += PlaceBatch::MAX) {
    PlaceBatch pb;
    pb.n = std::min(n_pair - i0, (int)PlaceBatch::MAX);
    pb.stride = stride; pb.max_tiles = 0; pb.max_chunks = 0;
    pb.part = reinterpret_cast<float*>(p);
    pb.out = d_out;
    for (int k = 0; k < pb.n; ++k) {
      const int32_t* pair = pairs + 2 * (i0 + k);
      const PlaceDims d = place_dims(bg_hw, obj_hw, pair, stride);
      const int np = d.P * d.Q;  // <= the background's pixels < 2^31
      pb.pr[k] = PlacePair{plane[pair[0]], plane[n_bg + pair[1]], bg_hw[2 * pair[0] + 1], obj_hw[2 * pair[1] + 1], obj_hw[2 * pair[1]] * obj_hw[2 * pair[1] + 1],
                           d.Q, np, d.chunks, part0, out0};
      pb.max_tiles = std::max(pb.max_tiles, (int)(((long long)np + PlaceBatch::TILE - 1) / PlaceBatch::TILE));
      pb.max_chunks = std::max(pb.max_chunks, d.chunks);
      part0 += (size_t)np * d.chunks;
      out0 += (size_t)np;
    }
    launch_place_score(pb, s);
    launch_place_sum(pb, s);
  }
  if (hipGetLastError() != hipSuccess) { g_create_error = "pf_place_scores: kernel launch failed"; return PF_ERR_DEVICE; }
  return PF_OK;
}

// pf_fields_transform, pf_place_search (field_xform.hip).  cos and sin of a rotation in degrees in fp64, exactly 0 or +-1 at the multiples of 90
static void xform_trig(double rot_deg, double* c, double* s) {
  const double a = remainder(rot_deg, 360.0);  // exact, in [-180, 180]
  const double q = a / 90.0;
  if (q == floor(q)) {
    static const double C[5] = {-1.0, 0.0, 1.0, 0.0, -1.0}, S[5] = {0.0, -1.0, 0.0, 1.0, 0.0};
    *c = C[(int)q + 2]; *s = S[(int)q + 2];
    return;
  }
  const double rad = a * (M_PI / 180.0);
  *c = cos(rad); *s = sin(rad);
}
// NULL and the size of the transformed field in out[2], or what is wrong
static const char* xform_size(int h, int w, double scale, double rot, int32_t* out, std::string* why) {
  if (h < 1 || w < 1 || (long long)h * w > INT32_MAX) { *why = fmt("a field of %d x %d, smaller than 1 x 1 or of 2^31 pixels or more", h, w); return why->c_str(); }
  if (!(scale > 0.0) || !std::isfinite(scale)) { *why = fmt("scale %g, must be finite and > 0", scale); return why->c_str(); }
  if (!std::isfinite(rot)) { *why = fmt("rotation %g, must be finite", rot); return why->c_str(); }
  double c, s;
  xform_trig(rot, &c, &s);
  const double a = (double)h * fabs(c), b = (double)w * fabs(s), d = (double)w * fabs(c), e = (double)h * fabs(s);
  const double ho = std::max(1.0, floor(scale * (a + b) + 0.5)), wo = std::max(1.0, floor(scale * (d + e) + 0.5));
  if (!(ho * wo <= (double)INT32_MAX)) { *why = fmt("scale %g, rotation %g of a %d x %d field has 2^31 pixels or more", scale, rot, h, w); return why->c_str(); }
  out[0] = (int32_t)ho; out[1] = (int32_t)wo;
  return nullptr;
}

int pf_fields_transform_size(int h, int w, double scale, double rotation_deg, int32_t* out_hw) {
  std::string why;
  if (!out_hw) { g_create_error = "pf_fields_transform_size: h_out_hw is required"; return PF_ERR_ARG; }
  if (const char* e = xform_size(h, w, scale, rotation_deg, out_hw, &why)) { g_create_error = std::string("pf_fields_transform_size: ") + e; return PF_ERR_ARG; }
  return PF_OK;
}

// job k of a launch: the fp64 trig and 1 / s rounded to fp32 once
static void xform_job(FieldXform* fx, int k, const float* up, const float* lat, const int32_t* hw, const double* var, const int32_t* out_hw, float* out_up,
                      float* out_lat) {
  double c, s;
  xform_trig(var[1], &c, &s);
  fx->h[k] = hw[0]; fx->w[k] = hw[1]; fx->ho[k] = out_hw[0]; fx->wo[k] = out_hw[1];
  fx->c[k] = (float)c; fx->s[k] = (float)s; fx->inv[k] = (float)(1.0 / var[0]);
  fx->up[k] = up; fx->lat[k] = lat; fx->out_up[k] = out_up; fx->out_lat[k] = out_lat;
}

int pf_fields_transform(int device, int n, const float* const* up, const float* const* lat, const int32_t* hw, const double* variants, const int32_t* out_hw,
                        float* const* out_up, float* const* out_lat, void* stream) {
  auto bad = [](const std::string& m) { g_create_error = "pf_fields_transform: " + m; return PF_ERR_ARG; };
  if (n < 1 || !up || !lat || !hw || !variants || !out_hw || !out_up || !out_lat)
    return bad("n >= 1, h_up, h_lat, h_hw, h_variants, h_out_hw, h_out_up and h_out_lat are required");
  std::string why;
  for (int k = 0; k < n; ++k) {
    int32_t natural[2];
    if (!up[k] || !lat[k] || !out_up[k] || !out_lat[k]) return bad(fmt("NULL field pointer of job %d", k));
    if (const char* e = xform_size(hw[2 * k], hw[2 * k + 1], variants[2 * k], variants[2 * k + 1], natural, &why)) return bad(fmt("job %d: %s", k, e));
    if (out_hw[2 * k] < 1 || out_hw[2 * k + 1] < 1 || (long long)out_hw[2 * k] * out_hw[2 * k + 1] > INT32_MAX)
      return bad(fmt("job %d: output %d x %d, smaller than 1 x 1 or of 2^31 pixels or more", k, out_hw[2 * k], out_hw[2 * k + 1]));
    if (misalign(up[k], 3) || misalign(lat[k], 3) || misalign(out_up[k], 3) || misalign(out_lat[k], 3)) return bad(fmt("job %d: fields must be aligned to 4 bytes", k));
  }
  std::string err;
  const int rc = check_device(device, &err);
  if (rc != PF_OK) { g_create_error = err; return rc; }
  hipStream_t s = static_cast<hipStream_t>(stream);
  for (int k0 = 0; k0 < n; k0 += FieldXform::MAX) {
    FieldXform fx;
    fx.n = std::min(n - k0, (int)FieldXform::MAX);
    for (int k = 0; k < fx.n; ++k) {
      const int j = k0 + k;
      xform_job(&fx, k, up[j], lat[j], hw + 2 * j, variants + 2 * j, out_hw + 2 * j, out_up[j], out_lat[j]);
    }
    launch_field_xform(fx, s);
  }
  if (hipGetLastError() != hipSuccess) { g_create_error = "pf_fields_transform: kernel launch failed"; return PF_ERR_DEVICE; }
  return PF_OK;
}

// pf_place_search: workspace = the transformed (up, lat) planes of every (object, variant), the packed planes (backgrounds, then (object, variant)), the
// chunks' partial records of every (pair, variant) that fits, the valid pixels of every (object, variant), a BestHead per (pair, variant), the tiles'
// partial bests; each region 256-byte aligned
struct SearchPlan {
  std::vector<int32_t> ohw;    // [n_obj][n_var][2]
  size_t xf_bytes = 0, plane_bytes = 0, rec = 0, maps = 0, tiles = 0;
};
static bool search_fits(const int32_t* bg, const int32_t* o) { return o[0] <= bg[0] && o[1] <= bg[1]; }
static size_t search_xf_bytes(const int32_t* hw) { return yaw_align((size_t)hw[0] * hw[1] * 3 * sizeof(float)); }
static int search_tiles(long long np) { return (int)std::max(1LL, (np + BestBatch::TILE - 1) / BestBatch::TILE); }
// NULL and the plan, or what is wrong with the arguments that set the layout
static const char* search_plan(int n_bg, const int32_t* bg_hw, int n_obj, const int32_t* obj_hw, int n_pair, const int32_t* pairs, int n_var,
                               const double* variants, int stride, SearchPlan* pl, std::string* why) {
  if (n_bg < 1 || !bg_hw) return "n_bg >= 1 and h_bg_hw are required";
  if (n_obj < 1 || !obj_hw) return "n_obj >= 1 and h_obj_hw are required";
  if (n_pair < 1 || !pairs) return "n_pair >= 1 and h_pairs are required";
  if (n_var < 1 || !variants) return "n_var >= 1 and h_variants are required";
  if (stride < 1) { *why = fmt("stride %d, must be >= 1", stride); return why->c_str(); }
  if ((long long)n_pair * n_var > INT32_MAX || (long long)n_obj * n_var > INT32_MAX) return "2^31 (pair, variant) or (object, variant) combinations or more";
  for (int f = 0; f < n_bg; ++f)
    if (bg_hw[2 * f] < 1 || bg_hw[2 * f + 1] < 1 || (long long)bg_hw[2 * f] * bg_hw[2 * f + 1] > INT32_MAX) {
      *why = fmt("background %d is %d x %d, smaller than 1 x 1 or of 2^31 pixels or more", f, bg_hw[2 * f], bg_hw[2 * f + 1]);
      return why->c_str();
    }
  pl->ohw.resize((size_t)n_obj * n_var * 2);
  for (int o = 0; o < n_obj; ++o)
    for (int v = 0; v < n_var; ++v) {
      int32_t* t = &pl->ohw[((size_t)o * n_var + v) * 2];
      std::string w2;
      if (const char* e = xform_size(obj_hw[2 * o], obj_hw[2 * o + 1], variants[2 * v], variants[2 * v + 1], t, &w2)) {
        *why = fmt("object %d, variant %d: %s", o, v, e);
        return why->c_str();
      }
      pl->xf_bytes += search_xf_bytes(t);
      pl->plane_bytes += place_plane_bytes(t);
    }
  for (int f = 0; f < n_bg; ++f) pl->plane_bytes += place_plane_bytes(bg_hw + 2 * f);
  for (int k = 0; k < n_pair; ++k) {
    const int b = pairs[2 * k], o = pairs[2 * k + 1];
    if (b < 0 || b >= n_bg || o < 0 || o >= n_obj) {
      *why = fmt("pair %d: index (%d, %d) of (%d backgrounds, %d objects)", k, b, o, n_bg, n_obj);
      return why->c_str();
    }
    for (int v = 0; v < n_var; ++v) {
      const int32_t* t = &pl->ohw[((size_t)o * n_var + v) * 2];
      if (!search_fits(bg_hw + 2 * b, t)) { pl->tiles += 1; continue; }
      const long long chunks = ((long long)t[0] * t[1] + PlaceBatch::CHUNK - 1) / PlaceBatch::CHUNK;
      if (chunks > 65535) {
        *why = fmt("pair %d, variant %d: the transformed object (%d x %d) has more than 65535 chunks of %d pixels", k, v, t[0], t[1], (int)PlaceBatch::CHUNK);
        return why->c_str();
      }
      const long long np = (long long)((bg_hw[2 * b] - t[0]) / stride + 1) * ((bg_hw[2 * b + 1] - t[1]) / stride + 1);
      pl->rec += (size_t)np * chunks;
      pl->maps += (size_t)np * 3;
      pl->tiles += search_tiles(np);
    }
  }
  if (pl->tiles > (size_t)INT32_MAX) return "2^31 tiles of placements or more";
  return nullptr;
}
static size_t search_ws_bytes(const SearchPlan& pl, int n_obj, int n_pair, int n_var) {
  return 256 + pl.xf_bytes + pl.plane_bytes + yaw_align(pl.rec * 3 * sizeof(float)) + yaw_align((size_t)n_obj * n_var * sizeof(int)) +
         yaw_align((size_t)n_pair * n_var * sizeof(BestHead)) + yaw_align(pl.tiles * sizeof(BestTile));
}

size_t pf_place_search_workspace_bytes(int n_bg, const int32_t* bg_hw, int n_obj, const int32_t* obj_hw, int n_pair, const int32_t* pairs, int n_var,
                                       const double* variants, int stride) {
  SearchPlan pl;
  std::string why;
  if (search_plan(n_bg, bg_hw, n_obj, obj_hw, n_pair, pairs, n_var, variants, stride, &pl, &why)) return 0;
  return search_ws_bytes(pl, n_obj, n_pair, n_var);
}

int pf_place_search(int device, int n_bg, const float* const* bg_up, const float* const* bg_lat, const int32_t* bg_hw, int n_obj, const float* const* obj_up,
                    const float* const* obj_lat, const int32_t* obj_hw, int n_pair, const int32_t* pairs, int n_var, const double* variants, int stride,
                    double min_valid, double w_up, double w_lat, double* d_maps, size_t maps_doubles, double* d_best, double* d_var, void* ws, size_t ws_bytes,
                    void* stream) {
  auto bad = [](const std::string& m) { g_create_error = "pf_place_search: " + m; return PF_ERR_ARG; };
  SearchPlan pl;
  std::string why;
  if (const char* e = search_plan(n_bg, bg_hw, n_obj, obj_hw, n_pair, pairs, n_var, variants, stride, &pl, &why)) return bad(e);
  if (!bg_up || !bg_lat || !obj_up || !obj_lat || !d_best || !d_var) return bad("h_bg_up, h_bg_lat, h_obj_up, h_obj_lat, d_best and d_var are required");
  for (int f = 0; f < n_bg; ++f)
    if (!bg_up[f] || !bg_lat[f]) return bad(fmt("NULL field pointer of background %d", f));
  for (int f = 0; f < n_obj; ++f)
    if (!obj_up[f] || !obj_lat[f]) return bad(fmt("NULL field pointer of object %d", f));
  if (!(min_valid >= 0.0 && min_valid <= 1.0)) return bad(fmt("min_valid %g, must be in [0, 1]", min_valid));
  if (!(w_up >= 0.0 && w_lat >= 0.0) || !std::isfinite(w_up) || !std::isfinite(w_lat)) return bad(fmt("weights (%g, %g), must be finite and >= 0", w_up, w_lat));
  if (pl.maps > 0 && (!d_maps || maps_doubles < pl.maps)) return bad(fmt("d_maps needs %zu doubles, got %zu", pl.maps, d_maps ? maps_doubles : (size_t)0));
  if (misalign(d_maps, 7) || misalign(d_best, 7) || misalign(d_var, 7)) return bad("d_maps, d_best and d_var must be aligned to 8 bytes");
  const size_t need = search_ws_bytes(pl, n_obj, n_pair, n_var);
  if (!ws || ws_bytes < need) return bad(fmt("needs %zu workspace bytes, got %zu", need, ws_bytes));
  std::string err;
  const int rc = check_device(device, &err);
  if (rc != PF_OK) { g_create_error = err; return rc; }
  char* p = reinterpret_cast<char*>((reinterpret_cast<uintptr_t>(ws) + 255) & ~(uintptr_t)255);
  hipStream_t s = static_cast<hipStream_t>(stream);
  // 1. every (object, variant), object-major
  const int n_ov = n_obj * n_var;
  std::vector<float*> xf(n_ov);
  for (int k0 = 0; k0 < n_ov; k0 += FieldXform::MAX) {
    FieldXform fx;
    fx.n = std::min(n_ov - k0, (int)FieldXform::MAX);
    for (int k = 0; k < fx.n; ++k) {
      const int j = k0 + k, o = j / n_var, v = j - o * n_var;
      const int32_t* t = &pl.ohw[(size_t)j * 2];
      xf[j] = reinterpret_cast<float*>(p);
      xform_job(&fx, k, obj_up[o], obj_lat[o], obj_hw + 2 * o, variants + 2 * v, t, xf[j], xf[j] + (size_t)t[0] * t[1] * 2);
      p += search_xf_bytes(t);
    }
    launch_field_xform(fx, s);
  }
  // 2. the packed planes: backgrounds, then (object, variant)
  const int n_field = n_bg + n_ov;
  std::vector<float2*> plane(n_field);
  for (int f0 = 0; f0 < n_field; f0 += PlacePack::MAX) {
    PlacePack pp;
    pp.n = std::min(n_field - f0, (int)PlacePack::MAX);
    for (int k = 0; k < pp.n; ++k) {
      const int f = f0 + k;
      const int32_t* hw = f < n_bg ? bg_hw + 2 * f : &pl.ohw[(size_t)(f - n_bg) * 2];
      pp.npx[k] = hw[0] * hw[1];
      pp.up[k] = f < n_bg ? bg_up[f] : xf[f - n_bg];
      pp.lat[k] = f < n_bg ? bg_lat[f] : xf[f - n_bg] + (size_t)hw[0] * hw[1] * 2;
      pp.out[k] = plane[f] = reinterpret_cast<float2*>(p);
      p += place_plane_bytes(hw);
    }
    launch_place_pack(pp, s);
  }
  float* part = reinterpret_cast<float*>(p);
  p += yaw_align(pl.rec * 3 * sizeof(float));
  int* cnt = reinterpret_cast<int*>(p);
  p += yaw_align((size_t)n_ov * sizeof(int));
  BestHead* head = reinterpret_cast<BestHead*>(p);
  p += yaw_align((size_t)n_pair * n_var * sizeof(BestHead));
  BestTile* tile = reinterpret_cast<BestTile*>(p);
  for (int k0 = 0; k0 < n_ov; k0 += BestCount::MAX) {
    BestCount bc;
    bc.n = std::min(n_ov - k0, (int)BestCount::MAX);
    for (int k = 0; k < bc.n; ++k) {
      const int32_t* t = &pl.ohw[(size_t)(k0 + k) * 2];
      bc.npx[k] = t[0] * t[1];
      bc.plane[k] = plane[n_bg + k0 + k];
      bc.cnt[k] = cnt + k0 + k;
    }
    launch_place_count(bc, s);
  }
  // 3. the scores of every (pair, variant) that fits, pf_place_scores' launches; then every (pair, variant)'s partial bests
  const long long n_pv = (long long)n_pair * n_var;
  size_t part0 = 0, out0 = 0;
  int tile0 = 0;
  for (long long i0 = 0; i0 < n_pv; i0 += PlaceBatch::MAX) {
    PlaceBatch pb;
    BestBatch bb;
    pb.n = 0; pb.stride = stride; pb.max_tiles = 0; pb.max_chunks = 0; pb.part = part; pb.out = d_maps;
    bb.n = (int)std::min(n_pv - i0, (long long)BestBatch::MAX);
    bb.max_tiles = 1; bb.min_valid = min_valid; bb.w_up = w_up; bb.w_lat = w_lat; bb.head = head; bb.tile = tile;
    for (int k = 0; k < bb.n; ++k) {
      const int pair = (int)((i0 + k) / n_var), v = (int)((i0 + k) - (long long)pair * n_var);
      const int b = pairs[2 * pair], o = pairs[2 * pair + 1], ov = o * n_var + v;
      const int32_t *B = bg_hw + 2 * b, *t = &pl.ohw[(size_t)ov * 2];
      BestEntry& e = bb.e[k];
      e = BestEntry{nullptr, cnt + ov, 0, 1, t[0], t[1], tile0, (int)(i0 + k)};
      if (search_fits(B, t)) {
        const int P = (B[0] - t[0]) / stride + 1, Q = (B[1] - t[1]) / stride + 1, np = P * Q;  // <= the background's pixels < 2^31
        const int chunks = (int)(((long long)t[0] * t[1] + PlaceBatch::CHUNK - 1) / PlaceBatch::CHUNK);
        pb.pr[pb.n++] = PlacePair{plane[b], plane[n_bg + ov], B[1], t[1], t[0] * t[1], Q, np, chunks, part0, out0};
        pb.max_tiles = std::max(pb.max_tiles, (int)(((long long)np + PlaceBatch::TILE - 1) / PlaceBatch::TILE));
        pb.max_chunks = std::max(pb.max_chunks, chunks);
        e.map = d_maps + out0 * 3; e.np = np; e.Q = Q;
        part0 += (size_t)np * chunks;
        out0 += (size_t)np;
      }
      const int tiles = search_tiles(e.np);
      bb.max_tiles = std::max(bb.max_tiles, tiles);
      tile0 += tiles;
    }
    if (pb.n > 0) {
      launch_place_score(pb, s);
      launch_place_sum(pb, s);
    }
    launch_place_best_tiles(bb, s);
  }
  launch_place_best_pairs(n_pair, n_var, stride, head, tile, d_best, d_var, s);
  if (hipGetLastError() != hipSuccess) { g_create_error = "pf_place_search: kernel launch failed"; return PF_ERR_DEVICE; }
  return PF_OK;
}

// pf_draw_fields: workspace = every image's arrow records, [ny][nx] of 64 bytes, each region 256-byte aligned
struct DrawDims { int nx, ny; };
// anchors (j s + s / 2, i s + s / 2) inside an H x W image
static DrawDims draw_dims(int H, int W, int s) {
  const long long half = s / 2;
  return DrawDims{W > half ? (int)((W - half + s - 1) / s) : 0, H > half ? (int)((H - half + s - 1) / s) : 0};
}
static size_t draw_rec_bytes(int H, int W, int s) {
  const DrawDims d = draw_dims(H, W, s);
  return yaw_align((size_t)d.nx * d.ny * DrawBatch::REC * sizeof(float4));
}
// NULL, or what is wrong with the arguments that set the workspace's layout
static const char* draw_layout_error(int B, const int32_t* hw, int spacing, std::string* why) {
  if (B < 1 || !hw) return "batch >= 1 and h_hw are required";
  if (spacing < 1) { *why = fmt("spacing %d, must be >= 1", spacing); return why->c_str(); }
  for (int i = 0; i < B; ++i) {
    const int H = hw[2 * i], W = hw[2 * i + 1];
    if (H < 1 || W < 1 || H > (1 << 30) || W > (1 << 30) || (long long)H * W > INT32_MAX) {
      *why = fmt("image %d is %d x %d, smaller than 1 x 1 or of 2^31 pixels or more", i, H, W);
      return why->c_str();
    }
  }
  return nullptr;
}

size_t pf_draw_fields_workspace_bytes(int B, const int32_t* hw, int spacing) {
  std::string why;
  if (draw_layout_error(B, hw, spacing, &why)) return 0;
  size_t n = 256;  // alignment of the caller's pointer
  for (int i = 0; i < B; ++i) n += draw_rec_bytes(hw[2 * i], hw[2 * i + 1], spacing);
  return n;
}

int pf_draw_fields(int device, int B, const int32_t* hw, const void* const* img, const float* const* up, const float* const* lat, void* const* out, int dtype,
                   int spacing, float arrow_len_rel, float lat_step_deg, float alpha, float line_width, const float* arrow_rgb, int layers, void* ws,
                   size_t ws_bytes, void* stream) {
  auto bad = [](const std::string& m) { g_create_error = "pf_draw_fields: " + m; return PF_ERR_ARG; };
  std::string why;
  if (const char* e = draw_layout_error(B, hw, spacing, &why)) return bad(e);
  if (!img || !up || !lat || !out || !arrow_rgb) return bad("h_img, h_up, h_lat, h_out and h_arrow_rgb are required");
  if (dtype != PF_PANO_U8 && dtype != PF_PANO_F32) return bad(fmt("unknown dtype %d", dtype));
  if (layers < 0 || layers > (PF_DRAW_UP | PF_DRAW_LAT)) return bad(fmt("layers %d, must be a sum of PF_DRAW_UP and PF_DRAW_LAT", layers));
  if (!(lat_step_deg > 0.f && std::isfinite(lat_step_deg))) return bad("lat_step_deg must be finite and > 0");
  if (!(alpha >= 0.f && alpha <= 1.f)) return bad("alpha must be in [0, 1]");
  if (!(arrow_len_rel >= 0.f && arrow_len_rel <= 1e6f)) return bad("arrow_len_rel must be in [0, 1e6]");
  if (!(line_width >= 0.f && std::isfinite(line_width))) return bad("line_width must be finite and >= 0");
  if (!(std::isfinite(arrow_rgb[0]) && std::isfinite(arrow_rgb[1]) && std::isfinite(arrow_rgb[2]))) return bad("h_arrow_rgb must be finite");
  for (int i = 0; i < B; ++i)
    if (!img[i] || !up[i] || !lat[i] || !out[i]) return bad(fmt("NULL image, field or output pointer of image %d", i));
  const bool arrows = (layers & PF_DRAW_UP) != 0;
  const size_t need = pf_draw_fields_workspace_bytes(B, hw, spacing);
  if (arrows && (!ws || ws_bytes < need)) return bad(fmt("needs %zu workspace bytes, got %zu", need, ws_bytes));
  std::string err;
  const int rc = check_device(device, &err);
  if (rc != PF_OK) { g_create_error = err; return rc; }
  char* p = reinterpret_cast<char*>((reinterpret_cast<uintptr_t>(ws) + 255) & ~(uintptr_t)255);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const uintptr_t mask = dtype == PF_PANO_U8 ? 3 : 15;
  for (int i0 = 0; i0 < B; i0 += DrawBatch::MAX) {
    DrawBatch db;
    db.n = std::min(B - i0, (int)DrawBatch::MAX);
    db.spacing = spacing; db.layers = layers; db.max_tiles = 0; db.max_anchors = 0;
    db.lat_step = lat_step_deg; db.alpha = alpha; db.line_width = line_width;
    for (int c = 0; c < 3; ++c) db.rgb[c] = arrow_rgb[c];
    for (int k = 0; k < db.n; ++k) {
      const int i = i0 + k, H = hw[2 * i], W = hw[2 * i + 1];
      const DrawDims d = arrows ? draw_dims(H, W, spacing) : DrawDims{0, 0};
      db.H[k] = H; db.W[k] = W; db.nx[k] = d.nx; db.ny[k] = d.ny;
      db.len[k] = arrow_len_rel * (float)W;
      // no pixel further than this from an anchor's pixel, along a row or a column, is covered by its arrow; beyond the image's sides every value says the same
      db.reach[k] = (int)std::min(std::ceil((double)db.len[k] * (1.0 + (double)PF_DRAW_HEAD_RATIO) + (double)line_width + 1.0), (double)std::max(H, W));
      db.vec[k] = (W % 4 == 0 && ((misalign(img[i], mask) | misalign(out[i], mask)) == 0)) ? 1 : 0;
      db.fvec[k] = (W % 4 == 0 && ((misalign(up[i], 15) | misalign(lat[i], 15)) == 0)) ? 1 : 0;  // the second up plane starts H W floats on: aligned too
      db.img[k] = img[i]; db.up[k] = up[i]; db.lat[k] = lat[i]; db.out[k] = out[i];
      db.rec[k] = reinterpret_cast<float4*>(p);
      if (arrows) p += draw_rec_bytes(H, W, spacing);
      db.max_tiles = std::max(db.max_tiles, ((W - 1) / 64 + 1) * ((H - 1) / 16 + 1));
      db.max_anchors = std::max(db.max_anchors, d.nx * d.ny);
    }
    launch_draw_fields(db, dtype, s);
  }
  if (hipGetLastError() != hipSuccess) { g_create_error = "pf_draw_fields: kernel launch failed"; return PF_ERR_DEVICE; }
  return PF_OK;
}

// pf_composite (composite.hip): workspace = a CompositeJob record per job, 256-byte aligned
size_t pf_composite_workspace_bytes(int n) { return n < 1 ? 0 : 256 + yaw_align((size_t)n * sizeof(CompositeJob)); }

int pf_composite(int device, int n_bg, const void* const* bg, const int32_t* bg_hw, int n_obj, const void* const* obj, const float* const* obj_alpha,
                 const int32_t* obj_hw, int dtype, int n, const int32_t* jobs, const double* d_place, double opacity, int edge, int samples, void* const* out,
                 float* d_cov, void* ws, size_t ws_bytes, void* stream) {
  auto bad = [](const std::string& m) { g_create_error = "pf_composite: " + m; return PF_ERR_ARG; };
  if (n_bg < 1 || n_obj < 1 || n < 1) return bad(fmt("n_bg %d, n_obj %d and n %d must be >= 1", n_bg, n_obj, n));
  if (!bg || !bg_hw || !obj || !obj_hw || !jobs || !d_place || !out) return bad("h_bg, h_bg_hw, h_obj, h_obj_hw, h_jobs, d_place and h_out are required");
  if (dtype != PF_PANO_U8 && dtype != PF_PANO_F32) return bad(fmt("unknown dtype %d", dtype));
  if (edge != PF_COMPOSITE_SOFT && edge != PF_COMPOSITE_HARD) return bad(fmt("unknown edge %d", edge));
  if (!samples_ok("pf_composite", samples)) return PF_ERR_ARG;
  if (!(opacity >= 0.0 && opacity <= 1.0)) return bad(fmt("opacity %g, must be in [0, 1]", opacity));
  const uintptr_t elem = dtype == PF_PANO_U8 ? 0 : 3;
  for (int pass = 0; pass < 2; ++pass) {
    const int cnt = pass ? n_obj : n_bg;
    const int32_t* hw = pass ? obj_hw : bg_hw;
    const void* const* im = pass ? obj : bg;
    const char* what = pass ? "object" : "background";
    for (int i = 0; i < cnt; ++i) {
      const int H = hw[2 * i], W = hw[2 * i + 1];
      if (H < 1 || W < 1 || (long long)H * W > INT32_MAX) return bad(fmt("%s %d is %d x %d, smaller than 1 x 1 or of 2^31 pixels or more", what, i, H, W));
      if (!im[i]) return bad(fmt("NULL pointer of %s %d", what, i));
      if (misalign(im[i], elem) || (pass && obj_alpha && misalign(obj_alpha[i], 3))) return bad(fmt("%s %d: fp32 images and alpha planes must be aligned to 4 bytes", what, i));
    }
  }
  if (misalign(d_place, 7) || misalign(d_cov, 3)) return bad("d_place must be aligned to 8 bytes and d_cov to 4");
  for (int k = 0; k < n; ++k) {
    const int b = jobs[2 * k], o = jobs[2 * k + 1];
    if (b < 0 || b >= n_bg || o < 0 || o >= n_obj) return bad(fmt("job %d: index (%d, %d) out of range, %d backgrounds and %d objects", k, b, o, n_bg, n_obj));
    if (!out[k]) return bad(fmt("NULL output pointer of job %d", k));
    if (misalign(out[k], elem)) return bad(fmt("job %d: an fp32 output must be aligned to 4 bytes", k));
    if (out[k] == bg[b]) return bad(fmt("job %d: the output is its background; in-place composition is not offered", k));
    for (int f = 0; f < n_bg; ++f)
      if (out[k] == bg[f]) return bad(fmt("job %d: the output is background %d, which another job may be reading", k, f));
  }
  std::vector<const void*> sorted(out, out + n);  // two jobs never share an output: no order between them is defined
  std::sort(sorted.begin(), sorted.end());
  if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end()) return bad("two jobs share an output");
  const size_t need = pf_composite_workspace_bytes(n);
  if (!ws || ws_bytes < need) return bad(fmt("needs %zu workspace bytes, got %zu", need, ws_bytes));
  std::string err;
  const int rc = check_device(device, &err);
  if (rc != PF_OK) { g_create_error = err; return rc; }
  hipStream_t s = static_cast<hipStream_t>(stream);
  const uintptr_t mask = dtype == PF_PANO_U8 ? 3 : 15;
  float* cov = d_cov;
  for (int k0 = 0; k0 < n; k0 += CompositeBatch::MAX) {
    CompositeBatch cb;
    cb.n = std::min(n - k0, (int)CompositeBatch::MAX);
    cb.first = k0; cb.samples = samples; cb.hard = edge == PF_COMPOSITE_HARD ? 1 : 0; cb.opacity = opacity;
    cb.place = d_place;
    cb.rec = reinterpret_cast<CompositeJob*>((reinterpret_cast<uintptr_t>(ws) + 255) & ~(uintptr_t)255);
    for (int k = 0; k < cb.n; ++k) {
      const int b = jobs[2 * (k0 + k)], o = jobs[2 * (k0 + k) + 1];
      cb.H[k] = bg_hw[2 * b]; cb.W[k] = bg_hw[2 * b + 1]; cb.h[k] = obj_hw[2 * o]; cb.w[k] = obj_hw[2 * o + 1];
      cb.bg[k] = bg[b]; cb.obj[k] = obj[o]; cb.alpha[k] = obj_alpha ? obj_alpha[o] : nullptr; cb.out[k] = out[k0 + k];
      cb.cov[k] = cov;
      cb.vec[k] = (misalign(bg[b], mask) | misalign(out[k0 + k], mask)) == 0 ? 1 : 0;
      cb.cvec[k] = misalign(cov, 15) == 0 ? 1 : 0;
      if (cov) cov += (size_t)cb.H[k] * cb.W[k];
    }
    launch_composite(cb, dtype, s);
  }
  if (hipGetLastError() != hipSuccess) { g_create_error = "pf_composite: kernel launch failed"; return PF_ERR_DEVICE; }
  return PF_OK;
}

// workspace of pf_fit_camera / pf_fit_camera_usm / pf_fit_fisheye: per-image LM state, then every image's partial records, each region 256-byte aligned.
// The fits differ in their state, record, start and output row sizes and in their kernels only.
struct FitKind {
  const char* name;
  int state, rec, ntheta, cols;
  void (*init)(const FitBatch&, const FitParams&, hipStream_t);
  void (*iteration)(const FitBatch&, const FitParams&, hipStream_t);
};
static const FitKind kFitPinhole{"pf_fit_camera", FIT_STATE, FIT_REC, 5, PF_FIT_COLS, launch_fit_init<PinholeFit>, launch_fit_iteration<PinholeFit>};
static const FitKind kFitUsm{"pf_fit_camera_usm", USMFIT_STATE, USMFIT_REC, 6, PF_USMFIT_COLS, launch_fit_init<UsmFit>, launch_fit_iteration<UsmFit>};
// the lens fit: one per projection kind, without and with the polynomial's coefficients free
#define PF_FISHFIT_KIND(KIND, POLY) \
  FitKind{"pf_fit_fisheye", FISHFIT_STATE, FISHFIT_REC, 7, PF_FISHFIT_COLS, launch_fit_init<FisheyeFit<KIND, POLY>>, launch_fit_iteration<FisheyeFit<KIND, POLY>>}
static const FitKind kFitFisheye[3][2] = {{PF_FISHFIT_KIND(PF_FISHEYE_EQUIDISTANT, false), PF_FISHFIT_KIND(PF_FISHEYE_EQUIDISTANT, true)},
                                          {PF_FISHFIT_KIND(PF_FISHEYE_EQUISOLID, false), PF_FISHFIT_KIND(PF_FISHEYE_EQUISOLID, true)},
                                          {PF_FISHFIT_KIND(PF_FISHEYE_STEREOGRAPHIC, false), PF_FISHFIT_KIND(PF_FISHEYE_STEREOGRAPHIC, true)}};
#undef PF_FISHFIT_KIND
static_assert(PF_FISHEYE_EQUIDISTANT == 0 && PF_FISHEYE_EQUISOLID == 1 && PF_FISHEYE_STEREOGRAPHIC == 2, "kFitFisheye is indexed by the kind");
static_assert(PF_FISHFIT_COL_ROLL == PF_FIT_COL_ROLL && PF_FISHFIT_COL_PITCH == PF_FIT_COL_PITCH && PF_FISHFIT_COL_VFOV == PF_FIT_COL_VFOV &&
                  PF_FISHFIT_COL_REL_FOCAL == PF_FIT_COL_REL_FOCAL && PF_FISHFIT_COL_GENERAL_VFOV == PF_FIT_COL_GENERAL_VFOV &&
                  PF_FISHFIT_COL_REL_CX == PF_FIT_COL_REL_CX && PF_FISHFIT_COL_REL_CY == PF_FIT_COL_REL_CY && PF_FISHFIT_COL_RMS_UP == PF_FIT_COL_RMS_UP &&
                  PF_FISHFIT_COL_RMS_LAT == PF_FIT_COL_RMS_LAT && PF_FISHFIT_COL_COST == PF_FIT_COL_COST &&
                  PF_FISHFIT_COL_ITERATIONS == PF_FIT_COL_ITERATIONS && PF_FISHFIT_COL_CONVERGED == PF_FIT_COL_CONVERGED &&
                  PF_FISHFIT_COL_VALID_PIXELS == PF_FIT_COL_VALID_PIXELS && PF_FISHFIT_COL_K1 == PF_FIT_COLS && PF_FISHFIT_COL_K2 == PF_FIT_COLS + 1 &&
                  PF_FISHFIT_COLS == PF_FIT_COLS + 2,
              "the lens fit's output row is the pinhole row, then k1, k2");
static size_t fit_state_bytes(const FitKind& fk, int B) { return ((size_t)B * fk.state * sizeof(double) + 255) & ~(size_t)255; }
static size_t fit_part_bytes(const FitKind& fk, int H, int W) { return ((size_t)fit_blocks_per_image(H, W) * fk.rec * sizeof(double) + 255) & ~(size_t)255; }

static size_t fit_workspace_bytes(const FitKind& fk, int B, const int32_t* hw) {
  if (B <= 0 || !hw) return 0;
  size_t n = 256 + fit_state_bytes(fk, B);  // + 256: alignment of the caller's pointer
  for (int i = 0; i < B; ++i) {
    if (hw[2 * i] < 8 || hw[2 * i + 1] < 8) return 0;
    n += fit_part_bytes(fk, hw[2 * i], hw[2 * i + 1]);
  }
  return n;
}

// the argument checks every camera fit makes before any device work; PF_OK or PF_ERR_ARG with g_create_error set
static int fit_check_args(const char* name, int B, const int32_t* hw, const float* const* up, const float* const* lat, int free_pp, int loss,
                          float huber_delta_deg, float w_up, float w_lat, int max_iter, const float* d_out) {
  if (B <= 0 || !hw || !up || !lat || !d_out) { g_create_error = fmt("%s: bad argument", name); return PF_ERR_ARG; }
  if ((free_pp != 0 && free_pp != 1) || (loss != PF_FIT_LOSS_L2 && loss != PF_FIT_LOSS_HUBER) || max_iter < 1 || max_iter > 1000) {
    g_create_error = fmt("%s: bad option (free_pp %d, loss %d, max_iter %d)", name, free_pp, loss, max_iter);
    return PF_ERR_ARG;
  }
  if (!(w_up >= 0.f && w_lat >= 0.f && std::isfinite(w_up) && std::isfinite(w_lat) && w_up + w_lat > 0.f) ||
      (loss == PF_FIT_LOSS_HUBER && !(huber_delta_deg > 0.f && std::isfinite(huber_delta_deg)))) {
    g_create_error = fmt("%s: weights must be finite, >= 0 and not both 0; huber_delta_deg must be finite and > 0", name);
    return PF_ERR_ARG;
  }
  for (int i = 0; i < B; ++i) {
    if (hw[2 * i] < 8 || hw[2 * i + 1] < 8) { g_create_error = fmt("%s: image %d is %d x %d, smaller than 8 x 8", name, i, hw[2 * i], hw[2 * i + 1]); return PF_ERR_ARG; }
    if (!up[i] || !lat[i]) { g_create_error = fmt("%s: NULL field pointer of image %d", name, i); return PF_ERR_ARG; }
  }
  return PF_OK;
}

// the launch groups of a batch: FitBatch::MAX images each, their partial records laid out one after the other from `part`
static std::vector<FitBatch> fit_batches(const FitKind& fk, int B, const int32_t* hw, const float* const* up, const float* const* lat, const float* d_init,
                                         double* state, char* part, float* d_out) {
  std::vector<FitBatch> batches;
  for (int i0 = 0; i0 < B; i0 += FitBatch::MAX) {
    FitBatch fb;
    fb.n = std::min(B - i0, (int)FitBatch::MAX);
    for (int k = 0; k < fb.n; ++k) {
      const int i = i0 + k, H = hw[2 * i], W = hw[2 * i + 1];
      fb.H[k] = H; fb.W[k] = W; fb.nblk[k] = fit_blocks_per_image(H, W);
      fb.up[k] = up[i]; fb.lat[k] = lat[i];
      fb.part[k] = reinterpret_cast<double*>(part);
      part += fit_part_bytes(fk, H, W);
    }
    fb.state = state + (size_t)i0 * fk.state;
    fb.out = d_out + (size_t)i0 * fk.cols;
    fb.init = d_init ? d_init + (size_t)i0 * fk.ntheta : nullptr;
    batches.push_back(fb);
  }
  return batches;
}

static int fit_camera_run(const FitKind& fk, int device, int B, const int32_t* hw, const float* const* up, const float* const* lat, const float* d_init,
                          int free_pp, int loss, float huber_delta_deg, float w_up, float w_lat, int max_iter, float* d_out, void* ws, size_t ws_bytes,
                          void* stream, float theta_max = 0.f) {
  int rc = fit_check_args(fk.name, B, hw, up, lat, free_pp, loss, huber_delta_deg, w_up, w_lat, max_iter, d_out);
  if (rc != PF_OK) return rc;
  const size_t need = fit_workspace_bytes(fk, B, hw);
  if (!ws || ws_bytes < need) { g_create_error = fmt("%s: needs %zu workspace bytes, got %zu", fk.name, need, ws_bytes); return PF_ERR_WORKSPACE; }
  std::string err;
  rc = check_device(device, &err);
  if (rc != PF_OK) { g_create_error = err; return rc; }
  char* base = reinterpret_cast<char*>((reinterpret_cast<uintptr_t>(ws) + 255) & ~(uintptr_t)255);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const FitParams prm{free_pp, loss, huber_delta_deg, w_up, w_lat, theta_max};
  const std::vector<FitBatch> groups = fit_batches(fk, B, hw, up, lat, d_init, reinterpret_cast<double*>(base), base + fit_state_bytes(fk, B), d_out);
  // no host synchronisation: every image stops on its own flag, the launches run out as no-ops
  for (const FitBatch& fb : groups) fk.init(fb, prm, s);
  for (int it = 0; it <= max_iter; ++it)
    for (const FitBatch& fb : groups) fk.iteration(fb, prm, s);
  if (hipGetLastError() != hipSuccess) { g_create_error = fmt("%s: kernel launch failed", fk.name); return PF_ERR_DEVICE; }
  return PF_OK;
}

size_t pf_fit_camera_workspace_bytes(int B, const int32_t* hw) { return fit_workspace_bytes(kFitPinhole, B, hw); }

int pf_fit_camera(int device, int B, const int32_t* hw, const float* const* up, const float* const* lat, const float* d_init, int free_pp, int loss,
                  float huber_delta_deg, float w_up, float w_lat, int max_iter, float* d_out, void* ws, size_t ws_bytes, void* stream) {
  return fit_camera_run(kFitPinhole, device, B, hw, up, lat, d_init, free_pp, loss, huber_delta_deg, w_up, w_lat, max_iter, d_out, ws, ws_bytes, stream);
}

size_t pf_fit_camera_usm_workspace_bytes(int B, const int32_t* hw) { return fit_workspace_bytes(kFitUsm, B, hw); }

int pf_fit_camera_usm(int device, int B, const int32_t* hw, const float* const* up, const float* const* lat, const float* d_init, int free_pp, int loss,
                      float huber_delta_deg, float w_up, float w_lat, int max_iter, float* d_out, void* ws, size_t ws_bytes, void* stream) {
  return fit_camera_run(kFitUsm, device, B, hw, up, lat, d_init, free_pp, loss, huber_delta_deg, w_up, w_lat, max_iter, d_out, ws, ws_bytes, stream);
}

size_t pf_fit_fisheye_workspace_bytes(int B, const int32_t* hw) { return fit_workspace_bytes(kFitFisheye[0][0], B, hw); }

int pf_fit_fisheye(int device, int kind, int B, const int32_t* hw, const float* const* up, const float* const* lat, const float* d_init, int free_pp, int poly,
                   float theta_max, int loss, float huber_delta_deg, float w_up, float w_lat, int max_iter, float* d_out, void* ws, size_t ws_bytes,
                   void* stream) {
  const char* name = "pf_fit_fisheye";
  if (kind != PF_FISHEYE_EQUIDISTANT && kind != PF_FISHEYE_EQUISOLID && kind != PF_FISHEYE_STEREOGRAPHIC) {
    g_create_error = fmt("%s: unknown projection kind %d", name, kind);
    return PF_ERR_ARG;
  }
  if (!(std::isfinite(theta_max) && theta_max > 0.f && theta_max < 3.14159265358979323846)) {
    g_create_error = fmt("%s: theta_max must be finite and in (0, pi); got %g", name, (double)theta_max);
    return PF_ERR_ARG;
  }
  const int rc = fit_check_args(name, B, hw, up, lat, free_pp, loss, huber_delta_deg, w_up, w_lat, max_iter, d_out);
  if (rc != PF_OK) return rc;
  if (poly != 0 && poly != 1) { g_create_error = fmt("%s: bad option (poly %d)", name, poly); return PF_ERR_ARG; }
  return fit_camera_run(kFitFisheye[kind][poly], device, B, hw, up, lat, d_init, free_pp, loss, huber_delta_deg, w_up, w_lat, max_iter, d_out, ws, ws_bytes,
                        stream, theta_max);
}

// pf_fit_camera_shared: the per-image fits' init and accumulate kernels over launch groups of FitBatch::MAX images, and per iteration one
// reduction per image and one solve per camera group (fit_lm.h).  Workspace: that of the per-image fit, then the [B][rec] summed records.
struct FitSharedKind {
  const FitKind& fk;
  void (*start)(const FitGroups&, hipStream_t);
  void (*accum)(const FitBatch&, const FitParams&, double*, hipStream_t);
  void (*solve)(const FitGroups&, const FitParams&, hipStream_t);
};
static const FitSharedKind kFitShared[2] = {
    {kFitPinhole, launch_fit_shared_start<PinholeFit>, launch_fit_shared_accum<PinholeFit>, launch_fit_shared_solve<PinholeFit>},
    {kFitUsm, launch_fit_shared_start<UsmFit>, launch_fit_shared_accum<UsmFit>, launch_fit_shared_solve<UsmFit>}};
static size_t fit_rec_bytes(const FitKind& fk, int B) { return ((size_t)B * fk.rec * sizeof(double) + 255) & ~(size_t)255; }

// group sizes: every entry >= 1, summing to B
static bool fit_groups_ok(int B, int n_groups, const int32_t* gs, std::string* why) {
  if (n_groups < 1 || !gs) { *why = fmt("bad group sizes (n_groups %d)", n_groups); return false; }
  long sum = 0;
  for (int g = 0; g < n_groups; ++g) {
    if (gs[g] < 1) { *why = fmt("bad group sizes (group %d has %d images)", g, gs[g]); return false; }
    sum += gs[g];
  }
  if (sum != B) { *why = fmt("the group sizes sum to %ld, the batch is %d", sum, B); return false; }
  return true;
}

size_t pf_fit_camera_shared_workspace_bytes(int model, int B, const int32_t* hw, int n_groups, const int32_t* group_sizes) {
  std::string why;
  if ((model != 0 && model != 1) || B <= 0 || !fit_groups_ok(B, n_groups, group_sizes, &why)) return 0;
  const FitKind& fk = kFitShared[model].fk;
  const size_t n = fit_workspace_bytes(fk, B, hw);
  return n ? n + fit_rec_bytes(fk, B) : 0;
}

int pf_fit_camera_shared(int device, int model, int B, const int32_t* hw, const float* const* up, const float* const* lat, int n_groups,
                         const int32_t* group_sizes, const float* d_init, int free_pp, int loss, float huber_delta_deg, float w_up, float w_lat, int max_iter,
                         float* d_out, void* ws, size_t ws_bytes, void* stream) {
  const char* name = "pf_fit_camera_shared";
  if (model != 0 && model != 1) { g_create_error = fmt("%s: model must be 0 (pinhole) or 1 (USM), got %d", name, model); return PF_ERR_ARG; }
  int rc = fit_check_args(name, B, hw, up, lat, free_pp, loss, huber_delta_deg, w_up, w_lat, max_iter, d_out);
  if (rc != PF_OK) return rc;
  std::string why;
  if (!fit_groups_ok(B, n_groups, group_sizes, &why)) { g_create_error = fmt("%s: %s", name, why.c_str()); return PF_ERR_ARG; }
  for (int g = 0, i0 = 0; g < n_groups; i0 += group_sizes[g], ++g) {
    for (int i = i0 + 1; i < i0 + group_sizes[g]; ++i) {
      if (hw[2 * i] != hw[2 * i0] || hw[2 * i + 1] != hw[2 * i0 + 1]) {
        g_create_error = fmt("%s: the images of a group must have one size (rel_focal is relative to the height): group %d has %d x %d and %d x %d", name, g,
                             hw[2 * i0], hw[2 * i0 + 1], hw[2 * i], hw[2 * i + 1]);
        return PF_ERR_ARG;
      }
    }
  }
  const FitSharedKind& sk = kFitShared[model];
  const FitKind& fk = sk.fk;
  const size_t need = fit_workspace_bytes(fk, B, hw) + fit_rec_bytes(fk, B);
  if (!ws || ws_bytes < need) { g_create_error = fmt("%s: needs %zu workspace bytes, got %zu", name, need, ws_bytes); return PF_ERR_WORKSPACE; }
  std::string err;
  rc = check_device(device, &err);
  if (rc != PF_OK) { g_create_error = err; return rc; }
  char* base = reinterpret_cast<char*>((reinterpret_cast<uintptr_t>(ws) + 255) & ~(uintptr_t)255);
  double* state = reinterpret_cast<double*>(base);
  double* rec = reinterpret_cast<double*>(base + fit_state_bytes(fk, B));
  char* part = base + fit_state_bytes(fk, B) + fit_rec_bytes(fk, B);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const FitParams prm{free_pp, loss, huber_delta_deg, w_up, w_lat};
  const std::vector<FitBatch> batches = fit_batches(fk, B, hw, up, lat, d_init, state, part, d_out);
  std::vector<FitGroups> groups;
  for (int g0 = 0, i0 = 0; g0 < n_groups; g0 += FitGroups::MAX) {
    FitGroups fg;
    fg.n = std::min(n_groups - g0, (int)FitGroups::MAX);
    for (int k = 0; k < fg.n; ++k) { fg.start[k] = i0; fg.size[k] = group_sizes[g0 + k]; i0 += group_sizes[g0 + k]; }
    fg.state = state; fg.rec = rec; fg.out = d_out;
    groups.push_back(fg);
  }
  // no host synchronisation: every group stops on its own flag, the launches run out as no-ops
  for (const FitBatch& fb : batches) fk.init(fb, prm, s);
  for (const FitGroups& fg : groups) sk.start(fg, s);
  for (int it = 0; it <= max_iter; ++it) {
    for (size_t k = 0; k < batches.size(); ++k) sk.accum(batches[k], prm, rec + k * FitBatch::MAX * fk.rec, s);
    for (const FitGroups& fg : groups) sk.solve(fg, prm, s);
  }
  if (hipGetLastError() != hipSuccess) { g_create_error = fmt("%s: kernel launch failed", name); return PF_ERR_DEVICE; }
  return PF_OK;
}

int pf_fields_from_params_usm(int device, const float* d_cam6, int H, int W, float* d_up, float* d_lat, void* stream) {
  if (!d_cam6 || !d_up || !d_lat || H <= 0 || W <= 0) { g_create_error = "pf_fields_from_params_usm: bad argument"; return PF_ERR_ARG; }
  std::string err;
  const int rc = check_device(device, &err);
  if (rc != PF_OK) { g_create_error = err; return rc; }
  launch_fields_usm(d_cam6, H, W, d_up, d_lat, static_cast<hipStream_t>(stream));
  if (hipGetLastError() != hipSuccess) { g_create_error = "pf_fields_from_params_usm: kernel launch failed"; return PF_ERR_DEVICE; }
  return PF_OK;
}

// workspace of pf_field_errors: per-image selection state, output rows (used when d_out is NULL), the level histograms of every image (one
// region, zeroed per call), then per image the partial records and the two error maps (used unless the caller gives maps); 256-byte aligned
static size_t ferr_align(size_t n) { return (n + 255) & ~(size_t)255; }
static size_t ferr_hist_bytes() { return (size_t)3 * FERR_SEL * FERR_LEVEL_BINS * sizeof(unsigned); }
static size_t ferr_part_bytes(int H, int W) { return ferr_align((size_t)ferr_blocks_per_image(H, W) * FERR_REC * sizeof(double)); }
static size_t ferr_map_bytes(int H, int W) { return ferr_align((size_t)H * W * sizeof(float)); }
static bool ferr_size_ok(int H, int W) { return H >= 1 && W >= 1 && (long long)H * W < (1LL << 31); }

size_t pf_field_errors_workspace_bytes(int B, const int32_t* hw) {
  if (B <= 0 || !hw) return 0;
  size_t n = 256 + ferr_align((size_t)B * sizeof(FerrState)) + ferr_align((size_t)B * PF_FERR_COLS * sizeof(double)) + (size_t)B * ferr_hist_bytes();
  for (int i = 0; i < B; ++i) {
    if (!ferr_size_ok(hw[2 * i], hw[2 * i + 1])) return 0;
    n += ferr_part_bytes(hw[2 * i], hw[2 * i + 1]) + 2 * ferr_map_bytes(hw[2 * i], hw[2 * i + 1]);
  }
  return n;
}

int pf_field_errors(int device, int B, const int32_t* hw, const float* const* up_pred, const float* const* lat_pred, const float* const* up_gt,
                    const float* const* lat_gt, float threshold_deg, double* d_out, float* const* err_up, float* const* err_lat, int64_t* d_hist,
                    double* d_hist_sums, void* ws, size_t ws_bytes, void* stream) {
  auto bad = [](const std::string& m) { g_create_error = "pf_field_errors: " + m; return PF_ERR_ARG; };
  if (B <= 0 || !hw || !up_pred || !lat_pred || !up_gt || !lat_gt) return bad("batch >= 1, h_hw and the four field pointer arrays are required");
  if (!(threshold_deg > 0.f && std::isfinite(threshold_deg))) return bad("threshold_deg must be finite and > 0");
  if (!err_up != !err_lat) return bad("h_err_up and h_err_lat are both given or both NULL");
  if (!d_hist != !d_hist_sums) return bad("d_hist and d_hist_sums are both given or both NULL");
  for (int i = 0; i < B; ++i) {
    if (!ferr_size_ok(hw[2 * i], hw[2 * i + 1])) return bad(fmt("image %d is %d x %d", i, hw[2 * i], hw[2 * i + 1]));
    if (!up_pred[i] || !lat_pred[i] || !up_gt[i] || !lat_gt[i]) return bad(fmt("NULL field pointer of image %d", i));
    if (err_up && (!err_up[i] || !err_lat[i])) return bad(fmt("NULL error-map pointer of image %d", i));
  }
  const size_t need = pf_field_errors_workspace_bytes(B, hw);
  if (!ws || ws_bytes < need) { g_create_error = fmt("pf_field_errors: needs %zu workspace bytes, got %zu", need, ws_bytes); return PF_ERR_WORKSPACE; }
  std::string err;
  const int rc = check_device(device, &err);
  if (rc != PF_OK) { g_create_error = err; return rc; }
  char* p = reinterpret_cast<char*>((reinterpret_cast<uintptr_t>(ws) + 255) & ~(uintptr_t)255);
  FerrState* state = reinterpret_cast<FerrState*>(p);
  p += ferr_align((size_t)B * sizeof(FerrState));
  double* rows = d_out ? d_out : reinterpret_cast<double*>(p);
  p += ferr_align((size_t)B * PF_FERR_COLS * sizeof(double));
  char* hist = p;
  p += (size_t)B * ferr_hist_bytes();
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (hipMemsetAsync(hist, 0, (size_t)B * ferr_hist_bytes(), s) != hipSuccess) { g_create_error = "pf_field_errors: hipMemsetAsync failed"; return PF_ERR_DEVICE; }
  for (int i0 = 0; i0 < B; i0 += FerrBatch::MAX) {
    FerrBatch fb;
    fb.n = std::min(B - i0, (int)FerrBatch::MAX);
    for (int k = 0; k < fb.n; ++k) {
      const int i = i0 + k, H = hw[2 * i], W = hw[2 * i + 1];
      fb.H[k] = H; fb.W[k] = W; fb.nblk[k] = ferr_blocks_per_image(H, W);
      fb.up_pred[k] = up_pred[i]; fb.lat_pred[k] = lat_pred[i]; fb.up_gt[k] = up_gt[i]; fb.lat_gt[k] = lat_gt[i];
      fb.part[k] = reinterpret_cast<double*>(p);
      p += ferr_part_bytes(H, W);
      fb.err_up[k] = err_up ? err_up[i] : reinterpret_cast<float*>(p);
      fb.err_lat[k] = err_up ? err_lat[i] : reinterpret_cast<float*>(p + ferr_map_bytes(H, W));
      p += 2 * ferr_map_bytes(H, W);
      fb.hist[k] = reinterpret_cast<unsigned*>(hist + (size_t)i * ferr_hist_bytes());
      const uintptr_t align = reinterpret_cast<uintptr_t>(up_pred[i]) | reinterpret_cast<uintptr_t>(lat_pred[i]) | reinterpret_cast<uintptr_t>(up_gt[i]) |
                              reinterpret_cast<uintptr_t>(lat_gt[i]) | reinterpret_cast<uintptr_t>(fb.err_up[k]) | reinterpret_cast<uintptr_t>(fb.err_lat[k]);
      fb.vec[k] = (((size_t)H * W) % 4 == 0 && (align & 15) == 0) ? 1 : 0;  // H * W % 4: the second up plane starts at up + H * W
    }
    fb.state = state + i0;
    fb.out = rows + (size_t)i0 * PF_FERR_COLS;
    fb.threshold = threshold_deg;
    launch_field_errors(fb, s);
    if (d_hist) launch_field_errors_hist(fb, reinterpret_cast<long long*>(d_hist), d_hist_sums, s);
  }
  if (hipGetLastError() != hipSuccess) { g_create_error = "pf_field_errors: kernel launch failed"; return PF_ERR_DEVICE; }
  return PF_OK;
}
