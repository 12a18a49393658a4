"""The image gathers on the GPU -- crops, rotations and re-projections of panoramas, cube maps, fisheye frames and camera views, and the composition of
views into panoramas -- on one host skeleton: every entry point checks its arguments with the helpers at the top of this file, in its own order, and
hands its argument list to `_launch`.  Nothing moves to the device and the library is not loaded before the last check."""
from __future__ import annotations

import ctypes
import operator
from collections.abc import Mapping

import numpy as np
import torch

from .engine import PfError
from .fields import fields_from_params


# panorama element types of pf_pano_crop (include/pf_hip.h PF_PANO_*)
PANO_U8, PANO_F32 = 0, 1
_PANO_DTYPES = {torch.uint8: PANO_U8, torch.float32: PANO_F32}


def _cuda_image_list(fn, items, nouns, spec, min_side, ndim=3):
    """the sources of a gather: a non-empty list of (H, W, 3) CUDA tensors (ndim=4: the one tensor (B, H, W, 3)) of one dtype and one device with
    H, W >= min_side -> (list, device with its index).  nouns = (a source, sources); spec: the shape as the message words it"""
    if not items:
        raise ValueError(f"{fn} needs at least one {nouns[0]}")
    if not all(torch.is_tensor(p) for p in items):
        raise TypeError(f"{fn} takes torch tensors as {nouns[1]}")
    if not all(p.is_cuda for p in items):
        raise PfError(f"{fn} runs on the GPU only (no CPU path)")
    for p in items:
        if p.dim() != ndim or p.shape[-1] != 3 or p.shape[-2] < min_side or p.shape[-3] < min_side:
            raise ValueError(f"{spec}; got {tuple(p.shape)}")
        if p.dtype not in _PANO_DTYPES:
            raise ValueError(f"{nouns[1]} must be uint8 or float32; got {p.dtype}")
    if len({p.dtype for p in items}) != 1 or len({p.device for p in items}) != 1:
        raise ValueError(f"{fn}: all {nouns[1]} must have one dtype and one device")
    dev = items[0].device
    return items, dev if dev.index is not None else torch.device("cuda", torch.cuda.current_device())


def _sources(fn, images, nouns, spec, min_side, batched=False, ndim=3):
    """what a gather takes as its sources -- one tensor or a list of them; with batched=True also one tensor (B, Hs, Ws, 3), though not inside a list --
    checked by _cuda_image_list -> (list, n, the (H, W) of each source, device, a function that makes the n contiguous source tensors: to be called
    after every other check, it is the first thing that touches a device)"""
    batched = batched and torch.is_tensor(images) and images.dim() == 4
    srcs = [] if batched and images.shape[0] < 1 else [images] if torch.is_tensor(images) else list(images)
    srcs, dev = _cuda_image_list(fn, srcs, nouns, spec, min_side, ndim=4 if batched else ndim)
    if batched:
        n = int(srcs[0].shape[0])

        def make():
            whole = srcs[0].contiguous()
            return [whole[i] for i in range(n)]

        return srcs, n, [(int(srcs[0].shape[1]), int(srcs[0].shape[2]))] * n, dev, make
    return srcs, len(srcs), [(int(p.shape[ndim - 3]), int(p.shape[ndim - 2])) for p in srcs], dev, lambda: [p.contiguous() for p in srcs]


def _check_mode(mode):
    if mode not in ("deg", "rad"):
        raise ValueError("mode must be 'deg' or 'rad'")


def _out_size(height, width, noun):
    """height, width of a call's outputs as ints, at least 1 x 1; noun: what the message calls them"""
    H, W = int(height), int(width)
    if H < 1 or W < 1:
        raise ValueError(f"{noun} must be at least 1 x 1; got {H} x {W}")
    return H, W


def _param_tensors(named, label):
    """(name, value) pairs -> tensors (numbers or 1-d), checked where they are; nothing moves to the device.  label: how a message names a value, a
    format of its name ("{}", "crop_cubemap: {}", "src[{!r}]")"""
    ts = []
    for name, v in named:
        t = v if torch.is_tensor(v) else torch.as_tensor(np.asarray(v, dtype=np.float64))
        if t.dim() > 1:
            raise ValueError(f"{label.format(name)} must be a number or a 1-d sequence; got shape {tuple(t.shape)}")
        ts.append(t)
    return ts


def _rotation_tensors(fn, roll, pitch, yaw):
    return _param_tensors((("roll", roll), ("pitch", pitch), ("yaw", yaw)), fn + ": {}")


def _view_tensors(label, roll, pitch, yaw, rel_focal, rel_cx, rel_cy, xi):
    """the seven values of a cut view, in the row order of pf_pano_crop's d_cam7"""
    return _param_tensors((("roll", roll), ("pitch", pitch), ("yaw", yaw), ("rel_focal", rel_focal), ("rel_cx", rel_cx), ("rel_cy", rel_cy), ("xi", xi)), label)


def _broadcast_len(fn, ts, what=None):
    """the batch size that checked parameter tensors (numbers or 1-d) broadcast to, 1 when all are scalars; nothing moves to the device.  what: the noun of
    an output, for the calls whose batch size is this number and must be at least 1"""
    try:
        shape = torch.broadcast_shapes(*[tuple(t.shape) for t in ts])
    except RuntimeError as e:
        raise ValueError(f"{fn}: camera parameters do not broadcast: {e}") from None
    B = int(shape[0]) if shape else 1
    if what is not None and B < 1:
        raise ValueError(f"{fn} needs at least one {what}")
    return B


def _source_index(name, index, B, n, what):
    """the source of each of B outputs: None (all from source 0) or B integers in [0, n), as a list.  name: the argument's; what: the outputs' noun"""
    if index is None:
        return [0] * B
    idx = [operator.index(i) for i in (index.tolist() if torch.is_tensor(index) else index)]
    if len(idx) != B:
        raise ValueError(f"{name} has {len(idx)} entries for {B} {what}")
    if any(i < 0 or i >= n for i in idx):
        raise ValueError(f"{name} entries must be in [0, {n})")
    return idx


def _camera_rows(ts, angles, B, dev, mode):
    """parameter tensors that broadcast to B -> (B, len(ts)) fp32 rows on the device, after every check of the caller.  As fields_from_params:
    the `angles` columns go from degrees to radians in fp64 (mode "deg"), then everything to fp32"""
    ts = [t.to(device=dev, dtype=torch.float64) for t in ts]
    if mode == "deg":
        for k in angles:
            ts[k] = torch.deg2rad(ts[k])
    return torch.stack([t.expand(B) for t in ts], 1).to(torch.float32)


GATHER_MAX_SAMPLES = 4   # include/pf_hip.h PF_GATHER_MAX_SAMPLES


def _check_samples(fn, samples):
    """`samples` of a gather: an int in 1 .. GATHER_MAX_SAMPLES (the side of the grid of sub-samples per output pixel)"""
    if isinstance(samples, bool) or not isinstance(samples, (int, np.integer)) or not 1 <= samples <= GATHER_MAX_SAMPLES:
        raise ValueError(f"{fn}: samples must be an integer in [1, {GATHER_MAX_SAMPLES}]; got {samples!r}")
    return int(samples)


def _size_array(sizes):
    """the (H, W) pairs of the sources as the int32 array the library reads"""
    return (ctypes.c_int32 * (2 * len(sizes)))(*[s for hw in sizes for s in hw])


def _source_head(dev, srcs, c_hw):
    """the head of every gather's argument list: device, number of sources, their pointers, their (H, W) pairs, their element type"""
    n = len(srcs)
    return (dev.index, n, (ctypes.c_void_p * n)(*[p.data_ptr() for p in srcs]), c_hw, _PANO_DTYPES[srcs[0].dtype])


def _source_args(dev, srcs, sizes, idx):
    """the arguments that name a gather's sources and say which one each output reads: (_source_head, the int32 array of idx)"""
    return _source_head(dev, srcs, _size_array(sizes)), (ctypes.c_int32 * len(idx))(*idx)


def _ptr(t):
    """the address of an optional output"""
    return None if t is None else t.data_ptr()


def _image_and_fields(B, H, W, dtype, dev, fields):
    """the outputs of the panorama gathers: the images (B, H, W, 3) and, with fields, the labels up (B, 2, H, W) and lat (B, H, W); None without"""
    img = torch.empty((B, H, W, 3), dtype=dtype, device=dev)
    up = torch.empty((B, 2, H, W), dtype=torch.float32, device=dev) if fields else None
    lat = torch.empty((B, H, W), dtype=torch.float32, device=dev) if fields else None
    return img, up, lat


def _launch(entry, dev, args, samples=None, lib=None):
    """the one call of a gather into the library, on `dev`, with the current stream as its last argument.  samples: for the three families whose
    supersampled form is an entry point of its own, `entry`_ss, which takes the number after the common arguments; None elsewhere.  lib: the
    library, where the caller has loaded it already (for a workspace size)"""
    from .engine import _check, _stream_ptr, load_library

    if lib is None:
        lib = load_library()
    if samples is not None and samples > 1:
        entry, args = entry + "_ss", args + (samples,)
    with torch.cuda.device(dev):
        _check(getattr(lib, entry)(*args, _stream_ptr()), None, entry)


def _view_fields(ts, xi, B, H, W, mode, dev):
    """the labels of B cut views whose pictures do not come from a panorama: fields_from_params of every view, stacked.  ts: _view_tensors' seven;
    xi: as the caller gave it"""
    pinhole = not torch.is_tensor(xi) and np.ndim(xi) == 0 and float(xi) == 0.0   # fields_from_params' rule: the number 0 is the pinhole model
    rows = [t.expand(B) for t in ts]
    per_view = [fields_from_params(rows[0][i], rows[1][i], rows[3][i], rows[4][i], rows[5][i], height=H, width=W, mode=mode, device=dev,
                                   xi=0.0 if pinhole else rows[6][i]) for i in range(B)]
    return torch.stack([u for u, _ in per_view]), torch.stack([l for _, l in per_view])


def crop_panorama(pano, roll, pitch, rel_focal, rel_cx=0.0, rel_cy=0.0, *, yaw=0.0, xi=0.0, height, width, pano_index=None, mode="deg", fields=True, samples=1):
    """Equirectangular panoramas -> camera views and their ground-truth perspective fields on the GPU: the reference's labelled-data
    tooling (PanoCam.get_image / crop_equi, crop_distortion for the Unified Spherical Model, get_up_general / get_lat_general in
    utils/panocam.py).  Camera model, sampling and labels: include/pf_hip.h pf_pano_crop.

    pano: a CUDA tensor (Hp, Wp, 3), uint8 or float32, or a list of them (one dtype, one device).
    roll, pitch, yaw (degrees unless mode="rad"), rel_focal, rel_cx, rel_cy, xi (0: pinhole; > 0: Unified Spherical Model): numbers,
    0-d tensors or 1-d tensors / sequences, broadcast to the batch size B (1 when all are scalars); device tensors stay on the device.
    pano_index: None (every crop from panorama 0) or B integers.  height, width: the size of every crop.
    Returns (images (B, H, W, 3) in the panorama's dtype, up (B, 2, H, W), lat (B, H, W) degrees); up / lat are None with fields=False.
    The labels use the layout of pred_gravity_original / pred_latitude_original; at xi = 0 they are bit-identical to
    `fields_from_params` with the same arguments.  Pixels without a ray (xi > 1) are 0 in the image and NaN in the labels.

    The orientation conventions are those of `fields_from_params` (pinned to the reference by tests/golden): x right, y down,
    positive pitch looks up, positive yaw turns towards higher panorama columns, row 0 of the panorama is the north pole and its
    centre column is longitude 0.  samples=S (1 .. 4) antialiases a crop that minifies its panorama: every pixel is the mean of S x S bilinear
    sub-samples (include/pf_hip.h pf_pano_crop_ss); the labels do not depend on it, and S = 1 is the one sample at the pixel centre.
    Pixel parity with the reference's equilib backend is not checked.  The reference's
    get_image(vfov, im_w, im_h, azimuth, elevation, roll, ar) maps to height=im_h, width=im_w, yaw=azimuth, pitch=elevation, roll=roll,
    rel_focal = 0.5 / tan(vfov / 2) (a centred crop with square pixels), rel_cx = rel_cy = 0, xi = 0.
    GPU only: CPU panoramas raise PfError."""
    fn = "crop_panorama"
    samples = _check_samples(fn, samples)
    _, n, sizes, dev, make = _sources(fn, pano, ("panorama", "panoramas"), "a panorama must be (Hp, Wp, 3) with Hp, Wp >= 2", 2)
    H, W = _out_size(height, width, "crop size")
    _check_mode(mode)
    ts = _view_tensors("{}", roll, pitch, yaw, rel_focal, rel_cx, rel_cy, xi)
    B = _broadcast_len(fn, ts, "crop")
    idx = _source_index("pano_index", pano_index, B, n, "crops")
    cam = _camera_rows(ts, (0, 1, 2), B, dev, mode).contiguous()
    panos = make()
    img, up, lat = _image_and_fields(B, H, W, panos[0].dtype, dev, fields)
    head, c_idx = _source_args(dev, panos, sizes, idx)
    _launch("pf_pano_crop", dev, head + (B, c_idx, cam.data_ptr(), H, W, img.data_ptr(), _ptr(up), _ptr(lat)), samples)
    return img, up, lat


def rotate_panorama(pano, roll=0.0, pitch=0.0, yaw=0.0, *, inverse=False, height=None, width=None, pano_index=None, mode="deg", fields=False, samples=1):
    """Equirectangular panoramas -> rotated equirectangular panoramas on the GPU, with the perspective fields of the panoramic camera on request:
    levelling a tilted 360 degree picture, tilting an upright one (labelled data for tilted panoramas), re-centring a composite.  Model, sampling and
    labels: include/pf_hip.h pf_pano_rotate; the conventions are `crop_panorama`'s.

    pano: a CUDA tensor (Hs, Ws, 3), uint8 or float32, or a list of them (one dtype, one device).
    roll, pitch, yaw (degrees unless mode="rad"): numbers, 0-d tensors or 1-d tensors / sequences, broadcast to the batch size B (1 when all are
    scalars); device tensors stay on the device.  With Q = Y(yaw) R_pitch(pitch) R_roll(roll):
    inverse=False -- the output is what a panoramic camera with orientation (roll, pitch, yaw) inside the (upright) source sees;
    inverse=True  -- a source shot by such a camera becomes the upright panorama: the levelling direction, which undoes the other.
    pano_index: None (every output from panorama 0) or B integers.  height, width: the size of every output, default the sources' (required
    when they differ in size).
    Returns the images (B, H, W, 3) in the panorama's dtype; with fields=True (images, up (B, 2, H, W), lat (B, H, W) degrees), the perspective
    fields of the output's camera in the layout of pred_gravity_original / pred_latitude_original (up is NaN at a pixel centre on the world's zenith
    or nadir).  Non-finite angles give an image of 0 and NaN fields.  samples=S (1 .. 4) antialiases an output smaller than its source: every pixel
    is the mean of S x S bilinear sub-samples (include/pf_hip.h pf_pano_rotate_ss); the fields do not depend on it.
    GPU only: CPU panoramas raise PfError."""
    fn = "rotate_panorama"
    samples = _check_samples(fn, samples)
    _, n, sizes, dev, make = _sources(fn, pano, ("panorama", "panoramas"), "a panorama must be (Hs, Ws, 3) with Hs, Ws >= 2", 2)
    if (height is None) != (width is None):
        raise ValueError("rotate_panorama: height and width are both given or both left out")
    if height is None:
        if len(set(sizes)) != 1:
            raise ValueError("rotate_panorama: the panoramas differ in size, so height and width are required")
        height, width = sizes[0]
    H, W = _out_size(height, width, "output size")
    _check_mode(mode)
    ts = _rotation_tensors(fn, roll, pitch, yaw)
    B = _broadcast_len(fn, ts, "output")
    idx = _source_index("pano_index", pano_index, B, n, "outputs")
    rot = _camera_rows(ts, (0, 1, 2), B, dev, mode).contiguous()
    panos = make()
    img, up, lat = _image_and_fields(B, H, W, panos[0].dtype, dev, fields)
    head, c_idx = _source_args(dev, panos, sizes, idx)
    _launch("pf_pano_rotate", dev, head + (B, c_idx, rot.data_ptr(), 1 if inverse else 0, H, W, img.data_ptr(), _ptr(up), _ptr(lat)), samples)
    return (img, up, lat) if fields else img


def panorama_fields(roll, pitch, *, height, width, mode="deg", device=None):
    """The perspective fields of an equirectangular (panoramic) camera with the given roll and pitch on the GPU: the counterpart of
    `fields_from_params` for the equirectangular projection, and the labels of `rotate_panorama(..., fields=True)` for the same parameters, bit for
    bit (yaw does not enter).  Model: include/pf_hip.h pf_pano_fields.
    roll, pitch (degrees unless mode="rad"): numbers, 0-d tensors or 1-d tensors / sequences, broadcast to B.  Returns (up (B, 2, H, W) unit vectors,
    latitude (B, H, W) degrees); up is NaN at a pixel centre on the zenith or nadir.  device: a CUDA device, default that of a tensor argument,
    else the current one."""
    H, W = _out_size(height, width, "field size")
    _check_mode(mode)
    ts = _rotation_tensors("panorama_fields", roll, pitch, 0.0)
    B = _broadcast_len("panorama_fields", ts, "camera")
    if device is None:
        device = next((t.device for t in ts if t.is_cuda), None)
    dev = torch.device("cuda" if device is None else device)
    if dev.type != "cuda":
        raise PfError("panorama_fields runs on the GPU only (no CPU path)")
    if not torch.cuda.is_available():
        raise PfError("panorama_fields runs on the GPU only and no GPU is available")
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    rot = _camera_rows(ts, (0, 1, 2), B, dev, mode).contiguous()
    up = torch.empty((B, 2, H, W), dtype=torch.float32, device=dev)
    lat = torch.empty((B, H, W), dtype=torch.float32, device=dev)
    _launch("pf_pano_fields", dev, (dev.index, B, rot.data_ptr(), 0, H, W, up.data_ptr(), lat.data_ptr()))
    return up, lat


_CUBE_FACES = ("front", "right", "back", "left", "up", "down")
_CUBE_PITCH_YAW = ((0.0, 0.0), (0.0, 90.0), (0.0, 180.0), (0.0, 270.0), (90.0, 0.0), (-90.0, 0.0))   # include/pf_hip.h, the cube-map convention
_CUBE_CROSS = ((1, 1), (1, 2), (1, 3), (1, 0), (0, 1), (2, 1))   # (block row, block column) of face k in the "cross" layout


def cubemap_face_cameras(mode="deg"):
    """The six cameras whose pictures are the faces front, right, back, left, up, down of a cube map (include/pf_hip.h, the cube-map convention):
    a dict of per-face lists roll, pitch, yaw (degrees, radians with mode="rad") and rel_focal = 0.5, the parameters `crop_panorama` and
    `compose_panorama` take: compose_panorama(faces, cubemap_face_cameras(), ...) turns six faces into a panorama by blending views,
    crop_panorama(pano, **cubemap_face_cameras(), height=N, width=N) cuts them."""
    _check_mode(mode)
    conv = (lambda a: a) if mode == "deg" else (lambda a: float(np.radians(a)))
    return dict(roll=[0.0] * 6, pitch=[conv(p) for p, _ in _CUBE_PITCH_YAW], yaw=[conv(y) for _, y in _CUBE_PITCH_YAW], rel_focal=[0.5] * 6)


def _cube_list(fn, cube):
    """the cube maps of a gather: (6, N, N, 3) CUDA tensors of one dtype and one device -> what _sources returns, the sizes being (N, N)"""
    found = _sources(fn, cube, ("cube map", "cube maps"), "a cube map must be (6, N, N, 3) with N >= 1", 1, ndim=4)
    for c in found[0]:
        if c.shape[0] != 6 or c.shape[1] != c.shape[2]:
            raise ValueError(f"a cube map must be (6, N, N, 3) with N >= 1; got {tuple(c.shape)}")
    return found


def crop_cubemap(cube, roll, pitch, rel_focal, rel_cx=0.0, rel_cy=0.0, *, yaw=0.0, xi=0.0, height, width, cube_index=None, mode="deg", fields=True, samples=1):
    """Cube maps -> camera views and their ground-truth perspective fields on the GPU: `crop_panorama` for 360 degree material stored as six faces
    (skyboxes, environment maps, six-face camera exports), without a detour through a panorama.  Convention and sampling: include/pf_hip.h
    pf_cube_crop.

    cube: a CUDA tensor (6, N, N, 3), uint8 or float32, faces front, right, back, left, up, down (`cubemap_face_cameras`), or a list of them (one
    dtype, one device; N may differ).  The camera parameters, mode, height, width and samples are `crop_panorama`'s; cube_index: None (every view
    from cube 0) or B integers.  The bilinear sampler is continuous across the edges and corners of the cube: a view that straddles an edge has no
    seam.  Returns (images (B, H, W, 3) in the cube's dtype, up (B, 2, H, W), lat (B, H, W) degrees); up / lat are `fields_from_params` of the same
    parameters (they do not depend on the source) and None with fields=False.  Pixels without a ray (xi > 1) are 0; a view with a non-finite
    parameter is 0.  GPU only: CPU cubes raise PfError."""
    fn = "crop_cubemap"
    samples = _check_samples(fn, samples)
    _, n, sizes, dev, make = _cube_list(fn, cube)
    H, W = _out_size(height, width, "view size")
    _check_mode(mode)
    ts = _view_tensors(fn + ": {}", roll, pitch, yaw, rel_focal, rel_cx, rel_cy, xi)
    B = _broadcast_len(fn, ts, "view")
    idx = _source_index("cube_index", cube_index, B, n, "views")
    cam = _camera_rows(ts, (0, 1, 2), B, dev, mode).contiguous()
    cubes = make()
    img = torch.empty((B, H, W, 3), dtype=cubes[0].dtype, device=dev)
    head, c_idx = _source_args(dev, cubes, sizes, idx)
    _launch("pf_cube_crop", dev, head + (B, c_idx, cam.data_ptr(), H, W, img.data_ptr(), samples))
    return (img,) + (_view_fields(ts, xi, B, H, W, mode, dev) if fields else (None, None))


def cubemap_to_panorama(cube, *, height, width, roll=0.0, pitch=0.0, yaw=0.0, inverse=False, cube_index=None, mode="deg", fields=False, samples=1):
    """Cube maps -> equirectangular panoramas on the GPU, turned on the way if angles are given: a tilted cube map is levelled into a panorama in one
    pass.  Convention and sampling: include/pf_hip.h pf_cube_to_pano.

    cube: as `crop_cubemap`.  roll, pitch, yaw, inverse, mode, samples: `rotate_panorama`'s, with the cube in the place of the source panorama
    (inverse=False: what a panoramic camera with that orientation inside the cube sees; inverse=True: a cube shot by such a rig becomes upright).
    height, width: the size of every output; cube_index: None (every output from cube 0) or B integers.
    Returns the images (B, H, W, 3) in the cube's dtype; with fields=True (images, up, lat), the fields being `panorama_fields(roll, pitch)` (those
    of the output's camera for inverse=False).  Non-finite angles give an image of 0.  GPU only: CPU cubes raise PfError."""
    fn = "cubemap_to_panorama"
    samples = _check_samples(fn, samples)
    _, n, sizes, dev, make = _cube_list(fn, cube)
    H, W = _out_size(height, width, "output size")
    _check_mode(mode)
    ts = _rotation_tensors(fn, roll, pitch, yaw)
    B = _broadcast_len(fn, ts, "output")
    idx = _source_index("cube_index", cube_index, B, n, "outputs")
    rot = _camera_rows(ts, (0, 1, 2), B, dev, mode).contiguous()
    cubes = make()
    img = torch.empty((B, H, W, 3), dtype=cubes[0].dtype, device=dev)
    head, c_idx = _source_args(dev, cubes, sizes, idx)
    _launch("pf_cube_to_pano", dev, head + (B, c_idx, rot.data_ptr(), 1 if inverse else 0, H, W, img.data_ptr(), samples))
    if not fields:
        return img
    up, lat = panorama_fields(ts[0].expand(B), ts[1].expand(B), height=H, width=W, mode=mode, device=dev)
    return img, up, lat


# projection kinds and lens layout of the fisheye gathers (include/pf_hip.h PF_FISHEYE_*)
FISHEYE_PROJECTIONS = {"equidistant": 0, "equisolid": 1, "stereographic": 2}
FISHEYE_MAX_LENSES, FISHEYE_LENS_FLOATS = 2, 12
_FISHEYE_RHO = {"equidistant": lambda t: t, "equisolid": lambda t: 2.0 * np.sin(0.5 * t), "stereographic": lambda t: 2.0 * np.tan(0.5 * t)}


def _fisheye_kind(fn, projection):
    if projection not in FISHEYE_PROJECTIONS:
        raise ValueError(f"{fn}: projection must be one of {sorted(FISHEYE_PROJECTIONS)}; got {projection!r}")
    return FISHEYE_PROJECTIONS[projection]


def fisheye_lens(fov, *, radius, center, projection="equidistant", k=(0.0, 0.0, 0.0, 0.0), roll=0.0, pitch=0.0, yaw=0.0, band=0.0, mode="deg"):
    """One lens row of the fisheye gathers (include/pf_hip.h, the lens model): 12 float64 values {roll, pitch, yaw (radians), F, Cx, Cy, theta_max,
    k1, k2, k3, k4, band}, from what a user knows about the lens.

    fov: the full field of view, in (0, 360] degrees; `radius`: the radius in pixels of the image circle, where the ray at fov / 2 lands;
    center = (Cx, Cy): the circle's centre in pixel-edge units of the frame (a texel centre is at integer + 1/2); projection: "equidistant"
    (rho = theta), "equisolid" (2 sin(theta / 2)) or "stereographic" (2 tan(theta / 2)); k = (k1, k2, k3, k4): the Kannala-Brandt polynomial
    theta_d = theta (1 + k1 theta^2 + k2 theta^4 + k3 theta^6 + k4 theta^8), OpenCV's fisheye model with the equidistant kind; roll, pitch, yaw: the
    lens -> world rotation Y(yaw) R(roll, pitch) in the conventions of `crop_panorama`; band: the feather width, the angle before fov / 2 over
    which the lens fades out.  fov, band and the angles are degrees unless mode="rad".  F = radius / rho(theta_d(fov / 2)).
    r(theta) = rho(theta_d(theta)) is evaluated in fp64 on [0, fov / 2]; a ValueError is raised if it is not strictly increasing: the polynomial is
    then not a lens."""
    fn = "fisheye_lens"
    _check_mode(mode)
    _fisheye_kind(fn, projection)
    conv = np.radians if mode == "deg" else (lambda a: a)
    vals = [float(v) for v in (fov, radius, band, roll, pitch, yaw)]
    cx, cy = (float(c) for c in center)
    ks = [float(v) for v in k]
    if len(ks) != 4:
        raise ValueError(f"{fn}: k has 4 coefficients (k1, k2, k3, k4); got {len(ks)}")
    if not np.isfinite(vals + [cx, cy] + ks).all():
        raise ValueError(f"{fn}: every value must be finite")
    tmax, band_r = 0.5 * float(conv(vals[0])), float(conv(vals[2]))
    if not 0.0 < tmax <= np.pi:
        raise ValueError(f"{fn}: fov must be in (0, {'360] degrees' if mode == 'deg' else '2 pi] radians'}; got {fov!r}")
    if not vals[1] > 0.0:
        raise ValueError(f"{fn}: radius must be > 0; got {radius!r}")
    if band_r < 0.0:
        raise ValueError(f"{fn}: band must be >= 0; got {band!r}")
    t = np.linspace(0.0, tmax, 4097)
    t2 = t * t
    td = t * (1.0 + t2 * (ks[0] + t2 * (ks[1] + t2 * (ks[2] + t2 * ks[3]))))
    with np.errstate(all="ignore"):
        r = _FISHEYE_RHO[projection](td)
    if not (np.isfinite(r).all() and (np.diff(r) > 0.0).all()):
        raise ValueError(f"{fn}: r(theta) is not strictly increasing on [0, fov / 2]: projection {projection!r} with k = {tuple(ks)} is not a lens")
    return np.array([conv(vals[3]), conv(vals[4]), conv(vals[5]), vals[1] / r[-1], cx, cy, tmax, *ks, band_r], dtype=np.float64)


def dual_fisheye_lenses(height, width, fov, **kw):
    """The two lens rows (2, 12) of the usual side-by-side dual-fisheye frame (height, width) of a two-lens 360 degree camera: image circles centred
    at (width / 4, height / 2) and (3 width / 4, height / 2) with radius min(width / 4, height / 2), the second lens at yaw + 180 degrees, and
    band = fov - 180 degrees, the overlap of the two lenses, so that one lens fades out exactly where the other fades in.  fov and the keywords
    projection, k, roll, pitch, yaw, mode (and band, to override the default) are `fisheye_lens`'s."""
    fn = "dual_fisheye_lenses"
    H, W = float(height), float(width)
    if not (H >= 1 and W >= 2):
        raise ValueError(f"{fn}: the frame must be at least 1 x 2; got {height} x {width}")
    if "radius" in kw or "center" in kw:
        raise TypeError(f"{fn}: radius and center follow from the frame")
    mode = kw.get("mode", "deg")
    _check_mode(mode)
    half = 180.0 if mode == "deg" else np.pi
    band = kw.pop("band", max(float(fov) - half, 0.0))
    yaw = float(kw.pop("yaw", 0.0))
    radius = min(W / 4.0, H / 2.0)
    return np.stack([fisheye_lens(fov, radius=radius, center=(W / 4.0, H / 2.0), yaw=yaw, band=band, **kw),
                     fisheye_lens(fov, radius=radius, center=(3.0 * W / 4.0, H / 2.0), yaw=yaw + half, band=band, **kw)])


def _fisheye_frames(fn, frames):
    """the frames of a fisheye gather: (Hs, Ws, 3) CUDA tensors of one dtype and one device -> what _sources returns"""
    return _sources(fn, frames, ("frame", "frames"), "a frame must be (Hs, Ws, 3) with Hs, Ws >= 1", 1)


def _fisheye_per_frame(lenses):
    """whether `lenses` holds one entry per frame (an array (n, 1 or 2, 12) or a list of 2-d entries) and not one entry shared by every frame"""
    ndim = lambda e: e.dim() if torch.is_tensor(e) else np.ndim(e)
    if isinstance(lenses, (list, tuple)):
        return len(lenses) > 0 and all(ndim(e) == 2 for e in lenses)
    return ndim(lenses) == 3


def _fisheye_lens_table(fn, lenses, n_frame):
    """`lenses` -> (n_frame, 2, 12) float64.  Anything 1-d or 2-d is ONE entry shared by every frame: a row (12,), or 1 or 2 rows ((1, 12), (2, 12),
    also as a list of two rows, so two rows are always the two lenses of a frame, never one lens each for two frames).  Per frame: an array
    (n_frame, 1 or 2, 12), or a list of n_frame 2-d entries ((1, 12) for a frame with one lens).  A missing second lens is a row of zeros:
    theta_max = 0 switches it off"""
    def host(e):
        return e.detach().cpu().numpy() if torch.is_tensor(e) else e

    def entry(e):
        a = np.asarray(host(e), dtype=np.float64)
        if a.ndim == 1:
            a = a[None]
        if a.ndim != 2 or a.shape[1] != FISHEYE_LENS_FLOATS or not 1 <= a.shape[0] <= FISHEYE_MAX_LENSES:
            raise ValueError(f"{fn}: a frame's lenses are one row of {FISHEYE_LENS_FLOATS} values or {FISHEYE_MAX_LENSES} such rows; got shape {tuple(a.shape)}")
        return np.concatenate([a, np.zeros((FISHEYE_MAX_LENSES - a.shape[0], FISHEYE_LENS_FLOATS))])

    if not _fisheye_per_frame(lenses):
        return np.repeat(entry(lenses)[None], n_frame, axis=0)
    if len(lenses) != n_frame:
        raise ValueError(f"{fn}: lenses has {len(lenses)} entries for {n_frame} frames")
    return np.stack([entry(e) for e in lenses])


def crop_fisheye(frames, lenses, roll, pitch, rel_focal, rel_cx=0.0, rel_cy=0.0, *, yaw=0.0, xi=0.0, height, width, frame_index=None, projection="equidistant",
                 mode="deg", fields=True, samples=1, fill=0, return_mask=False):
    """Fisheye and dual-fisheye frames -> camera views and their ground-truth perspective fields on the GPU: `crop_panorama` for the raw frames of a
    fisheye lens or of a two-lens 360 degree camera, without stitching a panorama first; with xi = 0 the view is the undistorted picture.  Lens
    model and sampling: include/pf_hip.h pf_fisheye_crop.

    frames: a CUDA tensor (Hs, Ws, 3), uint8 or float32, or a list of them (one dtype, one device; sizes may differ).  lenses: a row of
    `fisheye_lens`, a pair of rows (`dual_fisheye_lenses`; two lenses are blended across their overlap), both shared by every frame, or one such
    entry per frame (a list of (1 or 2, 12) arrays, or an array (n_frames, 1 or 2, 12)); two plain rows are always the two lenses of one frame,
    so two frames with one lens each take two (1, 12) entries.  The rows hold radians and are read on the host.
    projection: the kind of every lens of the call.  The camera parameters, mode, height, width and samples are `crop_panorama`'s; frame_index:
    None (every view from frame 0) or B integers.  fill: the value of the pixels without a ray or without a covering lens.
    Returns (images (B, H, W, 3) in the frames' dtype, up (B, 2, H, W), lat (B, H, W) degrees), and the mask (B, H, W) bool as a fourth entry with
    return_mask=True; up / lat are `fields_from_params` of the same parameters (they do not depend on the source) and None with fields=False.  A
    view with a non-finite parameter is `fill`.  GPU only: CPU frames raise PfError."""
    fn = "crop_fisheye"
    samples = _check_samples(fn, samples)
    kind = _fisheye_kind(fn, projection)
    _, n, sizes, dev, make = _fisheye_frames(fn, frames)
    H, W = _out_size(height, width, "view size")
    _check_mode(mode)
    fill = float(fill)
    ts = _view_tensors(fn + ": {}", roll, pitch, yaw, rel_focal, rel_cx, rel_cy, xi)
    B = _broadcast_len(fn, ts, "view")
    idx = _source_index("frame_index", frame_index, B, n, "views")
    table = _fisheye_lens_table(fn, lenses, n)
    cam = _camera_rows(ts, (0, 1, 2), B, dev, mode).contiguous()
    lens = torch.from_numpy(np.ascontiguousarray(table[idx], dtype=np.float32)).to(dev)
    srcs = make()
    img = torch.empty((B, H, W, 3), dtype=srcs[0].dtype, device=dev)
    valid = torch.empty((B, H, W), dtype=torch.uint8, device=dev) if return_mask else None
    head, c_idx = _source_args(dev, srcs, sizes, idx)
    _launch("pf_fisheye_crop", dev, head + (kind, B, c_idx, lens.data_ptr(), cam.data_ptr(), H, W, fill, img.data_ptr(), _ptr(valid), samples))
    mask = (valid.view(torch.bool),) if return_mask else ()
    return (img,) + (_view_fields(ts, xi, B, H, W, mode, dev) if fields else (None, None)) + mask


def fisheye_to_panorama(frames, lenses, *, height, width, roll=0.0, pitch=0.0, yaw=0.0, inverse=False, frame_index=None, projection="equidistant", mode="deg",
                        fields=False, samples=1, fill=0, return_mask=False):
    """Fisheye and dual-fisheye frames -> equirectangular panoramas on the GPU, turned on the way if angles are given: the two lenses of a 360
    degree camera are blended across their overlap, and a tilted rig is levelled into a panorama in one pass.  Lens model and sampling:
    include/pf_hip.h pf_fisheye_to_pano.

    frames, lenses, projection, frame_index, fill: as `crop_fisheye`.  roll, pitch, yaw, inverse, mode, samples: `rotate_panorama`'s, with the
    frame in the place of the source panorama (inverse=False: what a panoramic camera with that orientation among the lenses sees;
    inverse=True: a frame shot by a rig with that orientation becomes upright).  height, width: the size of every output.
    Returns the images (B, H, W, 3) in the frames' dtype; with fields=True (images, up, lat), the fields being `panorama_fields(roll, pitch)`;
    with return_mask=True the mask (B, H, W) bool comes last: False where no lens covers the pixel, which then holds `fill`.  Non-finite angles
    give an image of `fill`.  GPU only: CPU frames raise PfError."""
    fn = "fisheye_to_panorama"
    samples = _check_samples(fn, samples)
    kind = _fisheye_kind(fn, projection)
    _, n, sizes, dev, make = _fisheye_frames(fn, frames)
    H, W = _out_size(height, width, "output size")
    _check_mode(mode)
    fill = float(fill)
    ts = _rotation_tensors(fn, roll, pitch, yaw)
    B = _broadcast_len(fn, ts, "output")
    idx = _source_index("frame_index", frame_index, B, n, "outputs")
    table = _fisheye_lens_table(fn, lenses, n)
    rot = _camera_rows(ts, (0, 1, 2), B, dev, mode).contiguous()
    lens = torch.from_numpy(np.ascontiguousarray(table[idx], dtype=np.float32)).to(dev)
    srcs = make()
    img = torch.empty((B, H, W, 3), dtype=srcs[0].dtype, device=dev)
    valid = torch.empty((B, H, W), dtype=torch.uint8, device=dev) if return_mask else None
    head, c_idx = _source_args(dev, srcs, sizes, idx)
    _launch("pf_fisheye_to_pano", dev, head + (kind, B, c_idx, lens.data_ptr(), rot.data_ptr(), 1 if inverse else 0, H, W, fill, img.data_ptr(), _ptr(valid),
                                              samples))
    out = (img,)
    if fields:
        out += tuple(panorama_fields(ts[0].expand(B), ts[1].expand(B), height=H, width=W, mode=mode, device=dev))
    if return_mask:
        out += (valid.view(torch.bool),)
    return out[0] if len(out) == 1 else out


def _cuda_device(fn, device, ts=()):
    """the CUDA device of a call without a source: `device`, else that of a tensor argument, else the current one, with its index"""
    if device is None:
        device = next((t.device for t in ts if torch.is_tensor(t) and t.is_cuda), None)
    dev = torch.device("cuda" if device is None else device)
    if dev.type != "cuda":
        raise PfError(f"{fn} runs on the GPU only (no CPU path)")
    if not torch.cuda.is_available():
        raise PfError(f"{fn} runs on the GPU only and no GPU is available")
    return dev if dev.index is not None else torch.device("cuda", torch.cuda.current_device())


def panorama_to_fisheye(pano, lenses, *, height, width, projection="equidistant", pano_index=None, fill=0, return_mask=False, fields=False, samples=1):
    """Equirectangular panoramas -> fisheye and dual-fisheye frames on the GPU, with the ground-truth perspective fields of the fisheye camera on
    request: `crop_panorama` for a real fisheye lens (labelled fisheye data out of panoramas), and the way back from `fisheye_to_panorama` /
    `crop_fisheye`.  Lens model, inverse projection and labels: include/pf_hip.h pf_pano_to_fisheye.

    pano: a CUDA tensor (Hp, Wp, 3), uint8 or float32, or a list of them (one dtype, one device).  lenses: as `crop_fisheye`, with the outputs in
    the place of the frames: a row of `fisheye_lens`, a pair of rows (`dual_fisheye_lenses(height, width, fov)` gives the side-by-side frame), both
    shared by every output, or one such entry per output; the rows hold radians and are read on the host.  A pixel belongs to the first lens whose
    image circle holds it: a target frame is not blended and `band` is not used.  projection: the kind of every lens of the call.
    height, width: the size of every frame.  The number of outputs B is that of pano_index (B integers, the panorama of each output), else that of
    per-output lenses, else one output per panorama; without pano_index output i reads panorama i, or panorama 0 when there is one panorama.
    fill: the value of the pixels outside every image circle.  samples=S (1 .. 4) antialiases a frame that minifies its panorama, as in
    `crop_panorama`; the fields do not depend on it.
    Returns the images (B, H, W, 3) in the panorama's dtype; with fields=True (images, up (B, 2, H, W), lat (B, H, W) degrees), which are
    `fisheye_fields` of the same lenses bit for bit: NaN outside every image circle, up NaN at a pixel centre on the zenith or nadir; with
    return_mask=True the mask (B, H, W) bool comes last: False where no lens owns the pixel, which then holds `fill`.
    GPU only: CPU panoramas raise PfError."""
    fn = "panorama_to_fisheye"
    samples = _check_samples(fn, samples)
    kind = _fisheye_kind(fn, projection)
    _, n, sizes, dev, make = _sources(fn, pano, ("panorama", "panoramas"), "a panorama must be (Hp, Wp, 3) with Hp, Wp >= 2", 2)
    H, W = _out_size(height, width, "frame size")
    fill = float(fill)
    if pano_index is not None:
        B = len(pano_index)
    elif _fisheye_per_frame(lenses):
        B = len(lenses)
    else:
        B = n
    if B < 1:
        raise ValueError(f"{fn} needs at least one output")
    if pano_index is None and n > 1 and B != n:
        raise ValueError(f"{fn}: {B} outputs of {n} panoramas, so pano_index is required")
    idx = _source_index("pano_index", list(range(B)) if pano_index is None and n > 1 else pano_index, B, n, "outputs")
    table = _fisheye_lens_table(fn, lenses, B)
    lens = torch.from_numpy(np.ascontiguousarray(table, dtype=np.float32)).to(dev)
    panos = make()
    img, up, lat = _image_and_fields(B, H, W, panos[0].dtype, dev, fields)
    valid = torch.empty((B, H, W), dtype=torch.uint8, device=dev) if return_mask else None
    head, c_idx = _source_args(dev, panos, sizes, idx)
    _launch("pf_pano_to_fisheye", dev, head + (kind, B, c_idx, lens.data_ptr(), H, W, fill, img.data_ptr(), _ptr(valid), _ptr(up), _ptr(lat), samples))
    out = (img,) + ((up, lat) if fields else ()) + ((valid.view(torch.bool),) if return_mask else ())
    return out[0] if len(out) == 1 else out


def fisheye_fields(lenses, *, height, width, projection="equidistant", device=None):
    """The perspective fields of a fisheye or dual-fisheye camera on the GPU: the counterpart of `fields_from_params` for a calibrated fisheye lens
    (OpenCV `fisheye` K and D, or a maker's equidistant, equisolid or stereographic lens) with a known roll and pitch, and the labels of
    `panorama_to_fisheye(..., fields=True)` for the same lenses, bit for bit (the yaw of a lens does not enter).  Model: include/pf_hip.h
    pf_fisheye_fields.
    lenses: a row of `fisheye_lens`, a pair of rows (one frame), or one such entry per frame (B frames); height, width: the size of the frames.
    Returns (up (B, 2, H, W) unit vectors, latitude (B, H, W) degrees) in the layout of pred_gravity_original / pred_latitude_original: what
    `field_errors` and `draw_perspective_fields` take.  Both are NaN outside every image circle; up is NaN at a pixel centre on the zenith or
    nadir.  device: a CUDA device, default that of a tensor argument, else the current one."""
    fn = "fisheye_fields"
    kind = _fisheye_kind(fn, projection)
    H, W = _out_size(height, width, "field size")
    B = len(lenses) if _fisheye_per_frame(lenses) else 1
    if B < 1:
        raise ValueError(f"{fn} needs at least one frame")
    table = _fisheye_lens_table(fn, lenses, B)
    dev = _cuda_device(fn, device, lenses if isinstance(lenses, (list, tuple)) else (lenses,))
    lens = torch.from_numpy(np.ascontiguousarray(table, dtype=np.float32)).to(dev)
    up = torch.empty((B, 2, H, W), dtype=torch.float32, device=dev)
    lat = torch.empty((B, H, W), dtype=torch.float32, device=dev)
    _launch("pf_fisheye_fields", dev, (dev.index, kind, B, lens.data_ptr(), H, W, up.data_ptr(), lat.data_ptr()))
    return up, lat


def panorama_to_cubemap(pano, size, *, roll=0.0, pitch=0.0, yaw=0.0, samples=1):
    """Equirectangular panoramas -> cube maps on the GPU: the six `crop_panorama` views of `cubemap_face_cameras()` at size x size, bit for bit.
    pano: a CUDA tensor (Hp, Wp, 3), uint8 or float32, or a list of B of them.  roll, pitch, yaw (degrees; numbers or B values): when one is given the
    panorama is first turned by `rotate_panorama` with these angles (the cube of a rig with that orientation inside the panorama), one more
    bilinear resampling.  samples: `crop_panorama`'s antialiasing of the faces.  Returns (B, 6, N, N, 3) in the panorama's dtype, faces front, right,
    back, left, up, down.  GPU only: CPU panoramas raise PfError."""
    fn = "panorama_to_cubemap"
    samples = _check_samples(fn, samples)
    panos, B = _sources(fn, pano, ("panorama", "panoramas"), "a panorama must be (Hp, Wp, 3) with Hp, Wp >= 2", 2)[:2]
    N = operator.index(size)
    if N < 1:
        raise ValueError(f"{fn}: size must be at least 1; got {N}")
    ts = _rotation_tensors(fn, roll, pitch, yaw)
    if _broadcast_len(fn, ts) not in (1, B) or any(t.dim() == 1 and t.shape[0] not in (1, B) for t in ts):
        raise ValueError(f"{fn}: roll, pitch and yaw are numbers or one value per panorama ({B})")
    if any(torch.is_tensor(v) or np.any(np.asarray(v) != 0) for v in (roll, pitch, yaw)):
        panos = [rotate_panorama(p, *(t if t.dim() == 0 else t[i % t.shape[0]] for t in ts))[0] for i, p in enumerate(panos)]
    cams = cubemap_face_cameras()
    faces, _, _ = crop_panorama(panos, cams["roll"] * B, cams["pitch"] * B, cams["rel_focal"] * B, yaw=cams["yaw"] * B, height=N, width=N,
                                pano_index=[i for i in range(B) for _ in range(6)], fields=False, samples=samples)
    return faces.view(B, 6, N, N, 3)


def _cube_layout(fn, layout):
    if layout not in ("strip", "cross"):
        raise ValueError(f"{fn}: layout must be 'strip' or 'cross'; got {layout!r}")


def cubemap_to_image(cube, layout):
    """A cube map (..., 6, N, N, 3) as one picture in an on-disk layout, by slicing alone (any device, any dtype): "strip" (..., N, 6 N, 3), faces
    0 ... 5 left to right; "cross" (..., 3 N, 4 N, 3), up at block (row 0, column 1), left, front, right, back at (1, 0 ... 3), down at (2, 1), the
    rest 0.  `cubemap_from_image` is the exact inverse."""
    fn = "cubemap_to_image"
    _cube_layout(fn, layout)
    if not torch.is_tensor(cube) or cube.dim() < 4 or cube.shape[-4] != 6 or cube.shape[-1] != 3 or cube.shape[-2] != cube.shape[-3] or cube.shape[-2] < 1:
        raise ValueError(f"{fn}: a cube map is a tensor (..., 6, N, N, 3) with N >= 1; got {tuple(cube.shape) if torch.is_tensor(cube) else type(cube)}")
    N = cube.shape[-2]
    if layout == "strip":
        return torch.cat([cube[..., k, :, :, :] for k in range(6)], dim=-2)
    img = cube.new_zeros(tuple(cube.shape[:-4]) + (3 * N, 4 * N, 3))
    for k, (br, bc) in enumerate(_CUBE_CROSS):
        img[..., br * N:(br + 1) * N, bc * N:(bc + 1) * N, :] = cube[..., k, :, :, :]
    return img


def cubemap_from_image(img, layout):
    """The cube map (..., 6, N, N, 3) of a picture (..., H, W, 3) in the layout "strip" (W = 6 H) or "cross" (H = 3 N, W = 4 N): `cubemap_to_image`'s
    inverse, by slicing alone; the blocks of a cross that hold no face are ignored."""
    fn = "cubemap_from_image"
    _cube_layout(fn, layout)
    if not torch.is_tensor(img) or img.dim() < 3 or img.shape[-1] != 3:
        raise ValueError(f"{fn}: a picture is a tensor (..., H, W, 3); got {tuple(img.shape) if torch.is_tensor(img) else type(img)}")
    H, W = img.shape[-3], img.shape[-2]
    if layout == "strip":
        if H < 1 or W != 6 * H:
            raise ValueError(f"{fn}: a strip is (N, 6 N, 3); got {H} x {W}")
        return torch.stack([img[..., :, k * H:(k + 1) * H, :] for k in range(6)], dim=-4)
    N = H // 3
    if N < 1 or H != 3 * N or W != 4 * N:
        raise ValueError(f"{fn}: a cross is (3 N, 4 N, 3); got {H} x {W}")
    return torch.stack([img[..., br * N:(br + 1) * N, bc * N:(bc + 1) * N, :] for br, bc in _CUBE_CROSS], dim=-4)


_CAM_KEYS = ("roll", "pitch", "yaw", "rel_focal", "rel_cx", "rel_cy", "xi")   # the row order of pf_reproject's d_cam_src7 / d_cam_dst7
_CAM_REQUIRED = ("roll", "pitch", "rel_focal")


def _camera_params(what, cam, fn="reproject_image"):
    """a camera dict -> its seven values as tensors in the order of _CAM_KEYS, checked where they are (nothing moves to the device yet)"""
    if not isinstance(cam, Mapping):
        raise TypeError(f"{fn}: {what} must be a dict of camera parameters; got {type(cam).__name__}")
    unknown = [k for k in cam if k not in _CAM_KEYS]
    missing = [k for k in _CAM_REQUIRED if k not in cam]
    if unknown or missing:
        raise ValueError(f"{fn}: {what} needs {_CAM_REQUIRED} and may hold {_CAM_KEYS[2:3] + _CAM_KEYS[4:]}; unknown {unknown}, missing {missing}")
    return _param_tensors([(k, cam.get(k, 0.0)) for k in _CAM_KEYS], what + "[{!r}]")


def reproject_image(images, src, dst, *, height=None, width=None, src_index=None, mode="deg", fill=0, return_valid=False, return_map=False, samples=1):
    """Images of one camera -> images of another camera of the same centre on the GPU: upright rectification (destination roll 0, or roll
    and pitch 0), undistortion of a Unified Spherical Model view (destination xi = 0), another focal length, principal point or output
    size, or any other view of the same centre.  Model: include/pf_hip.h pf_reproject; the cameras are those of
    `crop_panorama` and `fields_from_params`, so the perspective fields of the result are `fields_from_params` of `dst`.

    images: a CUDA tensor (Hs, Ws, 3) or (B, Hs, Ws, 3), uint8 or float32, or a list of (Hs, Ws, 3) tensors of one dtype and one device,
    whose sizes may differ.  src, dst: dicts with `roll`, `pitch`, `rel_focal` (required) and `yaw`, `rel_cx`, `rel_cy`, `xi` (default 0);
    angles in degrees unless mode="rad"; each value a number, a 0-d tensor or a 1-d sequence / tensor, broadcast to the batch size B;
    device tensors stay on the device.  src describes the camera that took the image, dst the camera to render.
    B and the source of each output: with src_index (B integers into the images) B = len(src_index); otherwise one output per image, or,
    for a single image, as many as the parameters broadcast to.  height, width: the size of every output; default: the size of the
    sources (a ValueError when they differ).  fill: the value of the pixels that see nothing of their source (no ray, behind the
    source camera, outside its image).
    Returns the images (B, H, W, 3) in the sources' dtype; with return_valid / return_map a tuple that adds the mask (B, H, W) bool and /
    or the map (B, 2, H, W) float32 of source coordinates (a_s, b_s) in pixel-edge units (NaN where the source camera does not see the ray).
    Bilinear sampling without mip levels; samples=S (1 .. 4) antialiases an output that minifies its source: every pixel is the mean of the valid
    ones of S x S bilinear sub-samples (include/pf_hip.h pf_reproject_ss).  The mask is then True where any sub-sample is valid
    (the pixels outside it, and only those, were given `fill`), and the map stays the pixel centre's.  GPU only: CPU images raise PfError."""
    fn = "reproject_image"
    samples = _check_samples(fn, samples)
    _, n, sizes, dev, make = _sources(fn, images, ("image", "images"), "an image must be (Hs, Ws, 3) with Hs, Ws >= 1, or a tensor (B, Hs, Ws, 3)", 1, batched=True)
    if height is None or width is None:
        if len(set(sizes)) != 1:
            raise ValueError("reproject_image: the images differ in size; give height and width")
    H, W = _out_size(sizes[0][0] if height is None else height, sizes[0][1] if width is None else width, "output size")
    _check_mode(mode)
    fill = float(fill)
    ts = _camera_params("src", src) + _camera_params("dst", dst)
    Bp = _broadcast_len(fn, ts)
    if src_index is not None:
        idx = [operator.index(i) for i in (src_index.tolist() if torch.is_tensor(src_index) else src_index)]
        if any(i < 0 or i >= n for i in idx):
            raise ValueError(f"src_index entries must be in [0, {n})")
    else:
        idx = list(range(n)) if n > 1 else [0] * Bp
    B = len(idx)
    if B < 1:
        raise ValueError("reproject_image needs at least one output")
    if Bp not in (1, B):
        raise ValueError(f"reproject_image: camera parameters of length {Bp} for {B} outputs")
    cam = _camera_rows(ts, (0, 1, 2, 7, 8, 9), B, dev, mode)
    cam_s, cam_d = cam[:, :7].contiguous(), cam[:, 7:].contiguous()
    srcs = make()
    img = torch.empty((B, H, W, 3), dtype=srcs[0].dtype, device=dev)
    valid = torch.empty((B, H, W), dtype=torch.uint8, device=dev) if return_valid else None
    cmap = torch.empty((B, 2, H, W), dtype=torch.float32, device=dev) if return_map else None
    head, c_idx = _source_args(dev, srcs, sizes, idx)
    _launch("pf_reproject", dev, head + (B, c_idx, cam_s.data_ptr(), cam_d.data_ptr(), H, W, fill, img.data_ptr(), _ptr(valid), _ptr(cmap)), samples)
    out = (img,) + ((valid.view(torch.bool),) if return_valid else ()) + ((cmap,) if return_map else ())
    return out[0] if len(out) == 1 else out


BLEND_FEATHER, BLEND_MEAN = 0, 1
_BLENDS ={"feather": BLEND_FEATHER, "mean": BLEND_MEAN}
_COMPOSE_MAX_VIEWS = 32   # views of one panorama per launch (csrc/pf_kernels.h ComposeBatch::MAX); more need the accumulator


def compose_panorama(images, cams, *, height, width, pano_index=None, n_pano=None, blend="feather", mode="deg", fill=0, return_weight=False):
    """Camera views of one centre -> equirectangular panoramas on the GPU: the inverse direction of `crop_panorama`, with several views
    blended per panorama pixel.  Model: include/pf_hip.h pf_pano_compose; the cameras and the panorama's
    longitude / latitude convention are those of `crop_panorama`, so composing its crops gives the panorama back where they cover it.

    images: what `reproject_image` takes -- a CUDA tensor (Hs, Ws, 3) or (B, Hs, Ws, 3), uint8 or float32, or a list of (Hs, Ws, 3) tensors of
    one dtype and one device, whose sizes may differ.  cams: a dict with `roll`, `pitch`, `rel_focal` (required) and `yaw`, `rel_cx`,
    `rel_cy`, `xi` (default 0); angles in degrees unless mode="rad"; each value a number, a 0-d tensor or a 1-d sequence / tensor of one
    entry per view; device tensors stay on the device.
    height, width: the size Hp x Wp of every panorama.  pano_index: None (one panorama from all views) or one integer per view, the panorama
    it belongs to; the views are sorted by it on the host, stably, so the blend order within a panorama is the caller's.  n_pano: the
    number of panoramas, default max(pano_index) + 1; a panorama without views is all `fill`.
    blend: "feather" -- a view's weight falls linearly from 1 in the middle of its short side to 0 on its border, so the composite is
    continuous across view borders; "mean" -- every covering view counts the same (one view: its bilinear sample).  fill: the value of
    the pixels that no view covers.
    Returns the panoramas (n_pano, Hp, Wp, 3) in the views' dtype; with return_weight=True also the summed weight (n_pano, Hp, Wp)
    float32, 0 where nothing covers the pixel.  Bilinear sampling without antialiasing: a strongly minified view aliases.
    GPU only: CPU images raise PfError."""
    _, n, sizes, dev, make = _sources("compose_panorama", images, ("view", "views"), "a view must be (Hs, Ws, 3) with Hs, Ws >= 1, or a tensor (B, Hs, Ws, 3)", 1,
                                      batched=True)
    Hp, Wp = _out_size(height, width, "panorama size")
    _check_mode(mode)
    if blend not in _BLENDS:
        raise ValueError(f"blend must be one of {tuple(_BLENDS)}; got {blend!r}")
    fill = float(fill)
    ts = _camera_params("cams", cams, "compose_panorama")
    Bp = _broadcast_len("compose_panorama", ts)
    if Bp not in (1, n):
        raise ValueError(f"compose_panorama: camera parameters of length {Bp} for {n} views")
    if pano_index is None:
        idx = [0] * n
    else:
        idx = [operator.index(i) for i in (pano_index.tolist() if torch.is_tensor(pano_index) else pano_index)]
        if len(idx) != n:
            raise ValueError(f"pano_index has {len(idx)} entries for {n} views")
        if any(i < 0 for i in idx):
            raise ValueError("pano_index entries must be >= 0")
    P = max(idx) + 1 if n_pano is None else operator.index(n_pano)
    if P < 1 or any(i >= P for i in idx):
        raise ValueError(f"pano_index entries must be in [0, {P}) (n_pano)")
    order = sorted(range(n), key=idx.__getitem__)   # stable: the caller's order within a panorama
    cam = _camera_rows(ts, (0, 1, 2), n, dev, mode)
    if order != list(range(n)):
        cam = cam[torch.as_tensor(order, device=dev)]
    cam = cam.contiguous()
    srcs = make()
    srcs = [srcs[i] for i in order]
    counts = [0] * P
    for i in idx:
        counts[i] += 1
    pano = torch.empty((P, Hp, Wp, 3), dtype=srcs[0].dtype, device=dev)
    weight = torch.empty((P, Hp, Wp), dtype=torch.float32, device=dev) if return_weight else None
    acc = torch.empty((P, Hp, Wp, 4), dtype=torch.float32, device=dev) if max(counts) > _COMPOSE_MAX_VIEWS else None
    head, c_idx = _source_args(dev, srcs, [sizes[i] for i in order], [idx[i] for i in order])
    _launch("pf_pano_compose", dev, head + (c_idx, cam.data_ptr(), P, Hp, Wp, _BLENDS[blend], fill, pano.data_ptr(), _ptr(weight), _ptr(acc)))
    return (pano, weight) if return_weight else pano


def _field_sources(fn, up, lat, noun):
    """the fields a transport takes as its sources, as the placement functions take them -- one pair up (2, h, w) / lat (h, w), a batched pair
    (B, 2, h, w) / (B, h, w) or lists of pairs, CUDA tensors of one device, every side at least 2 (the latitude grid needs size - 1 > 0) ->
    (n, the (h, w) of each field, device, a function that makes the n contiguous float32 (up, lat) pairs: the first thing that touches a device)"""
    from .field_metrics import _field_list

    _, ups, lats = _field_list(noun, up, lat, fn)
    if not ups:
        raise ValueError(f"{fn} needs at least one {noun} field")
    if not all(torch.is_tensor(t) for t in ups + lats):
        raise TypeError(f"{fn} takes torch tensors as fields")
    if not all(t.is_cuda for t in ups + lats):
        raise PfError(f"{fn} runs on the GPU only (no CPU path)")
    for u, l in zip(ups, lats):
        if u.dim() != 3 or u.shape[0] != 2 or min(u.shape[1:]) < 2 or tuple(l.shape) != tuple(u.shape[1:]):
            raise ValueError(f"{fn}: up must be (2, h, w) and lat (h, w) with h, w >= 2; got {tuple(u.shape)} and {tuple(l.shape)}")
    if len({t.device for t in ups + lats}) != 1:
        raise ValueError(f"{fn}: all fields must be on one device")
    dev = ups[0].device
    dev = dev if dev.index is not None else torch.device("cuda", torch.cuda.current_device())
    make = lambda: ([u.to(torch.float32).contiguous() for u in ups], [l.to(torch.float32).contiguous() for l in lats])
    return len(ups), [(int(u.shape[1]), int(u.shape[2])) for u in ups], dev, make


def _field_head(dev, ups, lats, sizes):
    """the head of a field transport's argument list: device, number of sources, their up and latitude pointers, their (h, w) pairs"""
    n = len(ups)
    return (dev.index, n, (ctypes.c_void_p * n)(*[t.data_ptr() for t in ups]), (ctypes.c_void_p * n)(*[t.data_ptr() for t in lats]), _size_array(sizes))


def reproject_fields(up, lat, src, dst, *, height=None, width=None, src_index=None, mode="deg"):
    """Perspective fields of one camera -> the fields in another camera of the same centre on the GPU: `reproject_image` for fields, predicted ones
    included.  The latitude is resampled (it belongs to the ray); an up vector is a tangent direction and is pushed through the differential of
    (unproject, rotate, project), which needs the relative rotation only, not gravity.  Model: include/pf_hip.h pf_reproject_fields (DESIGN.md
    section 38).  Exact fields of `src` come out as the exact fields of `dst` up to the bilinear interpolation error.

    up (2, h, w), lat (h, w) in degrees (the layout of pred_gravity_original / pred_latitude_original): one field of CUDA tensors, a batched pair
    (B, 2, h, w) / (B, h, w), or lists of pairs whose sizes may differ; every side at least 2.  src, dst, mode, src_index and the broadcasting are
    exactly `reproject_image`'s, with the fields in the place of the images; height, width: the size of every output (at least 2 x 2), default the
    sources'.  Four taps per pixel, not clamped: a tap outside the array or on an invalid pixel (a non-finite value, an up vector shorter than 1e-6)
    is dropped, and a pixel is valid where the taps left carry at least half of the weight, for the up vector and for the latitude: NaN in all
    three planes otherwise, and where the source camera does not see the pixel's ray.  So NaN is a mask that moves with the picture and does not
    spread.  There is no `samples`: fields are smooth, and only a mask edge aliases.
    Returns (up (B, 2, H, W) unit vectors, lat (B, H, W) degrees), float32.  GPU only: CPU tensors raise PfError."""
    fn = "reproject_fields"
    n, sizes, dev, make = _field_sources(fn, up, lat, "source")
    if height is None or width is None:
        if len(set(sizes)) != 1:
            raise ValueError(f"{fn}: the fields differ in size; give height and width")
    H, W = (int(v) for v in (sizes[0][0] if height is None else height, sizes[0][1] if width is None else width))
    if H < 2 or W < 2:
        raise ValueError(f"{fn}: output size must be at least 2 x 2; got {H} x {W}")
    _check_mode(mode)
    ts = _camera_params("src", src, fn) + _camera_params("dst", dst, fn)
    Bp = _broadcast_len(fn, ts)
    if src_index is not None:
        idx = [operator.index(i) for i in (src_index.tolist() if torch.is_tensor(src_index) else src_index)]
        if any(i < 0 or i >= n for i in idx):
            raise ValueError(f"src_index entries must be in [0, {n})")
    else:
        idx = list(range(n)) if n > 1 else [0] * Bp
    B = len(idx)
    if B < 1:
        raise ValueError(f"{fn} needs at least one output")
    if Bp not in (1, B):
        raise ValueError(f"{fn}: camera parameters of length {Bp} for {B} outputs")
    cam = _camera_rows(ts, (0, 1, 2, 7, 8, 9), B, dev, mode)
    cam_s, cam_d = cam[:, :7].contiguous(), cam[:, 7:].contiguous()
    ups, lats = make()
    out_up = torch.empty((B, 2, H, W), dtype=torch.float32, device=dev)
    out_lat = torch.empty((B, H, W), dtype=torch.float32, device=dev)
    c_idx = (ctypes.c_int32 * B)(*idx)
    _launch("pf_reproject_fields", dev, _field_head(dev, ups, lats, sizes) + (B, c_idx, cam_s.data_ptr(), cam_d.data_ptr(), H, W, out_up.data_ptr(), out_lat.data_ptr()))
    return out_up, out_lat


def compose_panorama_fields(up, lat, cams, *, height, width, pano_index=None, n_pano=None, blend="feather", mode="deg", return_weight=False):
    """The perspective fields of camera views of one centre -> the fields of equirectangular panoramas on the GPU: `compose_panorama` for fields.
    The way to dense fields of a 360 degree picture (`PerspectiveFields.inference_panorama`) and to one field out of several overlapping views.
    Model: include/pf_hip.h pf_compose_fields; the result is laid out as `panorama_fields` lays out its labels.

    up, lat: the views' fields as `reproject_fields` takes them (every side at least 2).  cams, height, width, pano_index, n_pano, blend, mode: as
    `compose_panorama`, one camera per view.  Per panorama pixel every covering view gives a latitude and a unit up vector in the panorama's image
    plane (taps and validity as `reproject_fields`); they are blended with the feather (or mean) weights, the up vectors as vectors and made
    unit again.  A pixel that no view covers with valid fields is NaN in all three planes.  At most 32 views per panorama (a ValueError beyond).
    Returns (up (n_pano, 2, Hp, Wp), lat (n_pano, Hp, Wp)) float32; with return_weight=True also the summed weight (n_pano, Hp, Wp), 0 where
    nothing contributes.  GPU only: CPU tensors raise PfError."""
    fn = "compose_panorama_fields"
    n, sizes, dev, make = _field_sources(fn, up, lat, "view")
    Hp, Wp = _out_size(height, width, "panorama size")
    _check_mode(mode)
    if blend not in _BLENDS:
        raise ValueError(f"blend must be one of {tuple(_BLENDS)}; got {blend!r}")
    ts = _camera_params("cams", cams, fn)
    Bp = _broadcast_len(fn, ts)
    if Bp not in (1, n):
        raise ValueError(f"{fn}: camera parameters of length {Bp} for {n} views")
    if pano_index is None:
        idx = [0] * n
    else:
        idx = [operator.index(i) for i in (pano_index.tolist() if torch.is_tensor(pano_index) else pano_index)]
        if len(idx) != n:
            raise ValueError(f"pano_index has {len(idx)} entries for {n} views")
        if any(i < 0 for i in idx):
            raise ValueError("pano_index entries must be >= 0")
    P = max(idx) + 1 if n_pano is None else operator.index(n_pano)
    if P < 1 or any(i >= P for i in idx):
        raise ValueError(f"pano_index entries must be in [0, {P}) (n_pano)")
    counts = [0] * P
    for i in idx:
        counts[i] += 1
    if max(counts) > _COMPOSE_MAX_VIEWS:
        raise ValueError(f"{fn}: a panorama has {max(counts)} views, more than {_COMPOSE_MAX_VIEWS} views per panorama")
    order = sorted(range(n), key=idx.__getitem__)   # stable: the caller's order within a panorama
    cam = _camera_rows(ts, (0, 1, 2), n, dev, mode)
    if order != list(range(n)):
        cam = cam[torch.as_tensor(order, device=dev)]
    cam = cam.contiguous()
    ups, lats = make()
    ups, lats = [ups[i] for i in order], [lats[i] for i in order]
    out_up = torch.empty((P, 2, Hp, Wp), dtype=torch.float32, device=dev)
    out_lat = torch.empty((P, Hp, Wp), dtype=torch.float32, device=dev)
    weight = torch.empty((P, Hp, Wp), dtype=torch.float32, device=dev) if return_weight else None
    c_idx = (ctypes.c_int32 * n)(*[idx[i] for i in order])
    _launch("pf_compose_fields", dev, _field_head(dev, ups, lats, [sizes[i] for i in order]) + (c_idx, cam.data_ptr(), P, Hp, Wp, _BLENDS[blend], out_up.data_ptr(),
                                                                                                 out_lat.data_ptr(), _ptr(weight)))
    return (out_up, out_lat, weight) if return_weight else (out_up, out_lat)
