"""Perspective fields drawn over their pictures on the GPU (pf_draw_fields)."""
from __future__ import annotations

import ctypes
import operator
from collections import OrderedDict

import numpy as np
import torch

from .engine import PfError
from .field_metrics import _field_list
from .fields import fields_from_params
from .gathers import _PANO_DTYPES, _cuda_image_list


DRAW_UP, DRAW_LAT = 1, 2   # include/pf_hip.h PF_DRAW_*


def _draw_images(fn, images):
    """the pictures of a drawing call -> (kind, list as given): 'single' (H, W, 3), 'batched' (B, H, W, 3) or 'list'"""
    if torch.is_tensor(images):
        return ("batched", [images]) if images.dim() == 4 else ("single", [images])
    if not isinstance(images, (list, tuple)):
        raise TypeError(f"{fn} takes a torch tensor or a list of them as images")
    return "list", list(images)


def draw_perspective_fields(images, up, lat, *, density=10, arrow_inv_len=20, lat_step_deg=10.0, alpha=0.5, arrow_color=(0, 255, 0), line_width=1.0,
                            draw_up=True, draw_lat=True, out=None):
    """Perspective fields drawn over their pictures on the GPU, the first look at a prediction: a latitude tint (a diverging colour ramp, light at
    the horizon), iso-latitude lines every lat_step_deg degrees (the horizon twice as wide) and a grid of green arrows along the up vectors.  The
    drawing model is this library's own -- include/pf_hip.h pf_draw_fields -- and not matplotlib's rasteriser.

    images: a CUDA tensor (H, W, 3) or (B, H, W, 3), uint8 or float32 on the 0 - 255 scale, or a list of (H, W, 3) tensors of one dtype and one
    device whose sizes may differ.  up (2, H, W) and lat (H, W) degrees, the layout of `pred_gravity_original` / `pred_latitude_original`: one
    pair, batched tensors or lists, one pair per image and of its image's size (resizing fields is the caller's job).  A pixel with a non-finite
    field value or an up vector shorter than 1e-6 is not drawn on: NaN is the mask.
    density: arrows along the shorter side (the anchors are s = max(1, min(H, W) // density) pixels apart); arrow_inv_len: an arrow is
    W / arrow_inv_len pixels long; alpha: opacity of the tint; arrow_color: RGB on the 0 - 255 scale; line_width: of lines and arrows, pixels;
    draw_up / draw_lat switch the arrows / the tint and the lines.  out: where to draw, of the images' type and shapes (the images themselves
    are allowed); default: new tensors.
    Returns what was given: a tensor (H, W, 3), a tensor (B, H, W, 3) or a list.  uint8 results are rounded half up.  One C call for all images
    whose spacing s is the same -- one call for images of one size -- on the current stream, without a host synchronisation.  Deterministic; a
    picture's bits do not depend on the batch it is in.  GPU only: CPU tensors raise PfError."""
    from .engine import _check, _stream_ptr, load_library

    fn = "draw_perspective_fields"
    kind, ims = _draw_images(fn, images)
    _, ups, lats = _field_list("the", up, lat, fn)
    # the checks that need no device, in the caller's terms, before anything is looked at on a device
    density, arrow_inv_len, lat_step_deg, alpha, line_width = operator.index(density), float(arrow_inv_len), float(lat_step_deg), float(alpha), float(line_width)
    if density < 1:
        raise ValueError(f"density must be at least 1; got {density}")
    if not (arrow_inv_len > 0.0 and np.isfinite(arrow_inv_len) and 1.0 / arrow_inv_len <= 1e6):
        raise ValueError(f"arrow_inv_len must be finite and > 0 (at least 1e-6); got {arrow_inv_len}")
    if not (lat_step_deg > 0.0 and np.isfinite(lat_step_deg)):
        raise ValueError(f"lat_step_deg must be finite and > 0; got {lat_step_deg}")
    if not 0.0 <= alpha <= 1.0:
        raise ValueError(f"alpha must be in [0, 1]; got {alpha}")
    if not (line_width >= 0.0 and np.isfinite(line_width)):
        raise ValueError(f"line_width must be finite and >= 0; got {line_width}")
    rgb = [float(c) for c in arrow_color]
    if len(rgb) != 3 or not all(np.isfinite(c) for c in rgb):
        raise ValueError(f"arrow_color must be three finite numbers; got {arrow_color}")
    if not all(torch.is_tensor(t) for t in ims + ups + lats):
        raise TypeError(f"{fn} takes torch tensors")
    shapes = [tuple(im.shape[1:3]) for im in ims for _ in range(im.shape[0])] if kind == "batched" else [tuple(im.shape[:2]) for im in ims]
    if len(ups) != len(shapes):
        raise ValueError(f"{fn}: {len(ups)} fields for {len(shapes)} images")
    for hw, u, l in zip(shapes, ups, lats):
        if u.dim() != 3 or u.shape[0] != 2 or tuple(l.shape) != tuple(u.shape[1:]):
            raise ValueError(f"up must be (2, H, W) and lat (H, W); got {tuple(u.shape)} and {tuple(l.shape)}")
        if tuple(l.shape) != hw:
            raise ValueError(f"{fn}: fields of size {tuple(l.shape)} for an image of size {hw}: the fields must have the size of their image")
    ims, dev = _cuda_image_list(fn, [] if kind == "batched" and ims[0].shape[0] < 1 else ims, ("image", "images"),
                                "an image must be (H, W, 3) with H, W >= 1, or a tensor (B, H, W, 3)", 1, ndim=4 if kind == "batched" else 3)
    if not all(t.is_cuda for t in ups + lats):
        raise PfError(f"{fn} runs on the GPU only (no CPU path)")
    if any((t.device if t.device.index is not None else torch.device("cuda", torch.cuda.current_device())) != dev for t in ups + lats):
        raise ValueError(f"{fn}: images and fields must be on one device")
    if out is not None:
        _, outs = _draw_images(fn, out)
        if len(outs) != len(ims) or any(not torch.is_tensor(o) or o.shape != im.shape or o.dtype != im.dtype or o.device != im.device or not o.is_contiguous()
                                       for o, im in zip(outs, ims)):
            raise ValueError(f"{fn}: out must be contiguous and of the images' type, shapes and device")
    ims = [im.contiguous() for im in ims]
    outs = [torch.empty_like(im) for im in ims] if out is None else outs
    if kind == "batched":
        src, dst = list(ims[0].unbind(0)), list(outs[0].unbind(0))
    else:
        src, dst = ims, outs
    ups, lats = ([t.to(torch.float32).contiguous() for t in ts] for ts in (ups, lats))
    layers = (DRAW_UP if draw_up else 0) | (DRAW_LAT if draw_lat else 0)
    groups = OrderedDict()   # spacing -> images: the C call takes one spacing
    for i, (h, w) in enumerate(shapes):
        groups.setdefault(max(1, min(h, w) // density), []).append(i)
    c_rgb = (ctypes.c_float * 3)(*rgb)
    lib = load_library()
    with torch.cuda.device(dev):
        for spacing, idx in groups.items():
            n = len(idx)
            ptrs = lambda ts: (ctypes.c_void_p * n)(*[ts[i].data_ptr() for i in idx])
            hw = (ctypes.c_int32 * (2 * n))(*[s for i in idx for s in shapes[i]])
            need = int(lib.pf_draw_fields_workspace_bytes(n, hw, spacing))
            if need == 0:
                raise ValueError(f"{fn}: image sizes that one call does not take (2^31 pixels or more)")
            ws = torch.empty(need, dtype=torch.uint8, device=dev)
            _check(lib.pf_draw_fields(dev.index, n, hw, ptrs(src), ptrs(ups), ptrs(lats), ptrs(dst), _PANO_DTYPES[src[0].dtype], spacing, 1.0 / arrow_inv_len,
                                      lat_step_deg, alpha, line_width, c_rgb, layers, ws.data_ptr(), need, _stream_ptr()), None, "pf_draw_fields")
    return outs if kind == "list" else outs[0]


def draw_camera(images, roll, pitch, rel_focal, rel_cx=0.0, rel_cy=0.0, *, xi=0.0, mode="deg", **kw):
    """The perspective fields of a camera drawn over pictures on the GPU: `fields_from_params` for every image's size, then
    `draw_perspective_fields` (whose options -- density, arrow_inv_len, lat_step_deg, alpha, arrow_color, line_width, draw_up, draw_lat, out --
    pass through); the reference's draw_from_r_p_f_cx_cy with the focal length given directly.  images as there.  roll, pitch (degrees unless
    mode="rad"), rel_focal, rel_cx, rel_cy, xi: numbers or 0-d tensors for all images, or 1-d sequences / tensors of one value per image."""
    fn = "draw_camera"
    kind, ims = _draw_images(fn, images)
    ims, dev = _cuda_image_list(fn, [] if kind == "batched" and torch.is_tensor(ims[0]) and ims[0].shape[0] < 1 else ims, ("image", "images"),
                                "an image must be (H, W, 3) with H, W >= 1, or a tensor (B, H, W, 3)", 1, ndim=4 if kind == "batched" else 3)
    shapes = [tuple(im.shape[1:3]) for im in ims for _ in range(im.shape[0])] if kind == "batched" else [tuple(im.shape[:2]) for im in ims]

    def pick(name, v, i):
        if isinstance(v, (list, tuple, np.ndarray)) or (torch.is_tensor(v) and v.dim() == 1):
            if len(v) != len(shapes):
                raise ValueError(f"{fn}: {len(v)} values of {name} for {len(shapes)} images")
            return v[i]
        return v

    params = (("roll", roll), ("pitch", pitch), ("rel_focal", rel_focal), ("rel_cx", rel_cx), ("rel_cy", rel_cy))
    fields = [fields_from_params(*[pick(k, v, i) for k, v in params], height=h, width=w, mode=mode, device=dev, xi=pick("xi", xi, i))
              for i, (h, w) in enumerate(shapes)]
    ups, lats = [f[0] for f in fields], [f[1] for f in fields]
    return draw_perspective_fields(images, ups[0] if kind == "single" else ups, lats[0] if kind == "single" else lats, **kw)
