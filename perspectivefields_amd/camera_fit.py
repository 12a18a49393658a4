"""Camera parameters fitted to perspective fields on the GPU: per image (pf_fit_camera, pf_fit_camera_usm), with intrinsics shared by the
images of one camera (pf_fit_camera_shared), and a fisheye lens per image (pf_fit_fisheye)."""
from __future__ import annotations

import ctypes
import math

import numpy as np
import torch

from .engine import PfError


# columns of the pf_fit_camera output row (include/pf_hip.h PF_FIT_COL_*)
_FIT_COLS = ("pred_roll", "pred_pitch", "pred_vfov", "pred_rel_focal", "pred_general_vfov", "pred_rel_cx", "pred_rel_cy",
             "fit_rms_up_deg", "fit_rms_lat_deg", "fit_cost", "fit_iterations", "fit_converged", "fit_valid_pixels")
_FIT_LOSSES = {"l2": 0, "huber": 1}
# columns of the pf_fit_camera_usm output row (PF_USMFIT_COL_*): the same, then xi
_USMFIT_COLS = _FIT_COLS + ("pred_xi",)


def _fit_init_rows(init, B, dev, distortion, extra=("pred_xi",)):
    """the `init` dicts of the camera fits -> None or a device [B][5 + len(extra)] fp32 tensor of theta (angles in radians); `extra`: the keys
    behind pred_rel_cy of a fit with distortion (default 0, like pred_rel_cx / pred_rel_cy)"""
    if init is None:
        return None
    inits = [init] if isinstance(init, dict) else list(init)
    if len(inits) != B:
        raise ValueError(f"init has {len(inits)} entries for {B} images")
    rows = []
    for d in inits:
        z = torch.zeros((), dtype=torch.float64, device=dev)
        v = [torch.as_tensor(d[k], dtype=torch.float64).to(dev).reshape(()) for k in ("pred_roll", "pred_pitch", "pred_rel_focal")]
        v += [torch.as_tensor(d[k], dtype=torch.float64).to(dev).reshape(()) if k in d else z
              for k in ("pred_rel_cx", "pred_rel_cy") + (tuple(extra) if distortion else ())]
        v[0], v[1] = torch.deg2rad(v[0]), torch.deg2rad(v[1])
        rows.append(torch.stack(v))
    return torch.stack(rows).to(torch.float32).contiguous()


def _fit_fields(fn, up, lat, loss):
    """the fields of a per-image fit, checked: one pair of device tensors or lists of pairs -> (single, ups, lats, device), fp32 and contiguous"""
    single = torch.is_tensor(up)
    ups, lats = ([up], [lat]) if single else (list(up), list(lat))
    if len(ups) != len(lats) or not ups:
        raise ValueError(f"{fn} needs as many latitude maps as up fields, at least one")
    if loss not in _FIT_LOSSES:
        raise ValueError(f"loss must be one of {sorted(_FIT_LOSSES)}")
    for u, l in zip(ups, lats):
        if not (torch.is_tensor(u) and torch.is_tensor(l)):
            raise TypeError(f"{fn} takes torch tensors")
        if not (u.is_cuda and l.is_cuda):
            raise PfError(f"{fn} runs on the GPU only (no CPU path)")
        if u.dim() != 3 or u.shape[0] != 2 or tuple(l.shape) != tuple(u.shape[1:]):
            raise ValueError(f"up must be (2, H, W) and lat (H, W); got {tuple(u.shape)} and {tuple(l.shape)}")
    dev = ups[0].device
    if any(t.device != dev for t in ups + lats):
        raise ValueError(f"{fn}: all fields must be on one device")
    return single, [u.to(torch.float32).contiguous() for u in ups], [l.to(torch.float32).contiguous() for l in lats], dev


def fit_camera_params(up, lat, *, free_principal_point=False, loss="l2", huber_delta_deg=2.0, weights=(1.0, 1.0), max_iter=20, init=None, distortion=False):
    """Perspective fields -> camera parameters on the GPU: the inverse of `fields_from_params`, a per-image Levenberg-Marquardt
    least-squares fit of its model to an up field (2,H,W) and a latitude map (H,W) in degrees (the layout of
    `pred_gravity_original` / `pred_latitude_original`).  Model, loss and stopping rule: include/pf_hip.h pf_fit_camera.

    up / lat: one pair of device tensors, or lists of pairs (sizes may differ; one launch sequence per 32 images).
    free_principal_point: fit rel_cx / rel_cy too (5 parameters); otherwise they stay at their start values (0 without `init`).
    loss: "l2" or "huber" (threshold huber_delta_deg); weights = (w_up, w_lat); max_iter: LM steps per image.
    init: optional start, one dict (or a list of dicts) with pred_roll, pred_pitch (degrees), pred_rel_focal and optionally
    pred_rel_cx / pred_rel_cy -- e.g. an inference() result of a ParamNet model.

    Returns one dict per image (a single dict for a single pair): pred_roll, pred_pitch, pred_vfov, pred_rel_focal,
    pred_general_vfov, pred_rel_cx, pred_rel_cy (angles in degrees), fit_rms_up_deg, fit_rms_lat_deg, fit_cost, fit_iterations,
    fit_converged, fit_valid_pixels -- 0-d device tensors (no host synchronisation), so `fields_from_params` can take the
    pred_* entries directly.  GPU only: CPU tensors raise PfError.

    distortion=True fits the Unified Spherical Model of crop_panorama(..., xi=) instead (include/pf_hip.h pf_fit_camera_usm): the
    mirror parameter xi is free too -- 4 parameters, 6 with free_principal_point -- clamped to [-0.5, 2], and each dict gains `pred_xi`.
    `init` dicts may carry `pred_xi` (default 0); without `init` the start is the pinhole one at xi = 0, which recovers xi <= 1; for
    xi > 1 (part of the image has no ray) give a start.  pred_vfov / pred_general_vfov keep their formulas in rel_focal, rel_cx and
    rel_cy: under xi != 0 they describe the intrinsics, not the angle the image subtends.  fit_valid_pixels counts the pixels with finite
    input and a ray.  `fields_from_params(..., xi=d["pred_xi"])` turns a result back into fields.  distortion=False is the pinhole fit,
    unchanged."""
    from .engine import _check, _stream_ptr, load_library

    single, ups, lats, dev = _fit_fields("fit_camera_params", up, lat, loss)
    B = len(ups)
    d_init = _fit_init_rows(init, B, dev, distortion)
    hw = (ctypes.c_int32 * (2 * B))(*[s for u in ups for s in (int(u.shape[1]), int(u.shape[2]))])
    p_up = (ctypes.c_void_p * B)(*[u.data_ptr() for u in ups])
    p_lat = (ctypes.c_void_p * B)(*[l.data_ptr() for l in lats])
    lib = load_library()
    entry, cols = ("pf_fit_camera_usm", _USMFIT_COLS) if distortion else ("pf_fit_camera", _FIT_COLS)
    ws_n = int(getattr(lib, entry + "_workspace_bytes")(B, hw))
    if ws_n == 0:
        small = [tuple(u.shape[1:]) for u in ups if min(u.shape[1:]) < 8]
        raise PfError(f"fit_camera_params: images must be at least 8 x 8 (got {small})")
    ws = torch.empty(ws_n, dtype=torch.uint8, device=dev)
    out = torch.empty((B, len(cols)), dtype=torch.float32, device=dev)
    w_up, w_lat = (float(w) for w in weights)
    with torch.cuda.device(dev):
        _check(getattr(lib, entry)(dev.index, B, hw, p_up, p_lat, d_init.data_ptr() if d_init is not None else None, int(bool(free_principal_point)),
                                   _FIT_LOSSES[loss], float(huber_delta_deg), w_up, w_lat, int(max_iter), out.data_ptr(), ws.data_ptr(), ws_n,
                                   _stream_ptr()), None, entry)
    iters = out[:, 10].to(torch.int32)
    conv = out[:, 11] != 0
    valid = out[:, 12].to(torch.int64)
    res = []
    for i in range(B):
        d = {k: out[i, j] for j, k in enumerate(_FIT_COLS[:10])}
        d["fit_iterations"], d["fit_converged"], d["fit_valid_pixels"] = iters[i], conv[i], valid[i]
        if distortion:
            d["pred_xi"] = out[i, 13]
        res.append(d)
    return res[0] if single else res


def fit_camera_shared(up, lat, groups=None, *, distortion=False, free_principal_point=False, loss="l2", huber_delta_deg=2.0, weights=(1.0, 1.0), max_iter=20,
                      init=None):
    """The camera fit of `fit_camera_params` for images that share a camera -- the frames of a video, a photo set of one device: every
    image keeps its own roll and pitch, all images of a group share rel_focal, with free_principal_point also rel_cx / rel_cy, with
    distortion=True also xi.  One joint Levenberg-Marquardt fit per group on the GPU (include/pf_hip.h pf_fit_camera_shared).

    up / lat: lists of device tensors (2,H,W) / (H,W), as for fit_camera_params.  groups: None -- all images are one camera -- or one hashable
    label per image, in any order; the images of a group must have one size (rel_focal is relative to the height), groups may differ.
    The other options are those of fit_camera_params; `init` gives every image's start, the group starts from its images' mean.

    Returns one dict per image, in the caller's order, with the entries of fit_camera_params: the image's own pred_roll, pred_pitch,
    fit_rms_*, fit_cost and fit_valid_pixels; the group's pred_rel_focal, pred_rel_cx, pred_rel_cy, pred_xi (the same bits in every dict
    of a group), fit_iterations and fit_converged; plus fit_group_cost (0-d device tensor: the group's summed cost) and fit_group (the
    label; 0 with groups=None).  An image without a valid pixel contributes nothing: fit_valid_pixels 0, fit_converged False.
    GPU only: CPU tensors raise PfError."""
    from .engine import _check, _stream_ptr, load_library

    if torch.is_tensor(up) or torch.is_tensor(lat):
        raise TypeError("fit_camera_shared takes lists of fields, one pair per image")
    ups, lats = list(up), list(lat)
    if len(ups) != len(lats) or not ups:
        raise ValueError("fit_camera_shared needs as many latitude maps as up fields, at least one")
    if loss not in _FIT_LOSSES:
        raise ValueError(f"loss must be one of {sorted(_FIT_LOSSES)}")
    B = len(ups)
    labels = [0] * B if groups is None else list(groups)
    if len(labels) != B:
        raise ValueError(f"groups has {len(labels)} labels for {B} images")
    for u, l in zip(ups, lats):
        if not (torch.is_tensor(u) and torch.is_tensor(l)):
            raise TypeError("fit_camera_shared takes torch tensors")
        if u.dim() != 3 or u.shape[0] != 2 or tuple(l.shape) != tuple(u.shape[1:]):
            raise ValueError(f"up must be (2, H, W) and lat (H, W); got {tuple(u.shape)} and {tuple(l.shape)}")
    members = {}   # label -> its images, in the caller's order; the groups in the order of their first image
    for i, g in enumerate(labels):
        members.setdefault(g, []).append(i)
    for g, idx in members.items():
        sizes = sorted({tuple(ups[i].shape[1:]) for i in idx})
        if len(sizes) > 1:
            raise ValueError(f"fit_camera_shared: the images of group {g!r} have different sizes {sizes}; a camera group needs one size")
    if not all(u.is_cuda and l.is_cuda for u, l in zip(ups, lats)):
        raise PfError("fit_camera_shared runs on the GPU only (no CPU path)")
    dev = ups[0].device
    if any(t.device != dev for t in ups + lats):
        raise ValueError("fit_camera_shared: all fields must be on one device")
    order = [i for idx in members.values() for i in idx]   # consecutive groups
    ups = [ups[i].to(torch.float32).contiguous() for i in order]
    lats = [lats[i].to(torch.float32).contiguous() for i in order]
    if init is not None and not isinstance(init, dict):
        init = list(init)
        if len(init) != B:
            raise ValueError(f"init has {len(init)} entries for {B} images")
        init = [init[i] for i in order]
    d_init = _fit_init_rows(init, B, dev, distortion)
    hw = (ctypes.c_int32 * (2 * B))(*[s for u in ups for s in (int(u.shape[1]), int(u.shape[2]))])
    gs = (ctypes.c_int32 * len(members))(*[len(idx) for idx in members.values()])
    p_up = (ctypes.c_void_p * B)(*[u.data_ptr() for u in ups])
    p_lat = (ctypes.c_void_p * B)(*[l.data_ptr() for l in lats])
    lib = load_library()
    model, cols = (1, _USMFIT_COLS) if distortion else (0, _FIT_COLS)
    ws_n = int(lib.pf_fit_camera_shared_workspace_bytes(model, B, hw, len(members), gs))
    if ws_n == 0:
        small = [tuple(u.shape[1:]) for u in ups if min(u.shape[1:]) < 8]
        raise PfError(f"fit_camera_shared: images must be at least 8 x 8 (got {small})")
    ws = torch.empty(ws_n, dtype=torch.uint8, device=dev)
    out = torch.empty((B, len(cols)), dtype=torch.float32, device=dev)
    w_up, w_lat = (float(w) for w in weights)
    with torch.cuda.device(dev):
        _check(lib.pf_fit_camera_shared(dev.index, model, B, hw, p_up, p_lat, len(members), gs, d_init.data_ptr() if d_init is not None else None,
                                        int(bool(free_principal_point)), _FIT_LOSSES[loss], float(huber_delta_deg), w_up, w_lat, int(max_iter),
                                        out.data_ptr(), ws.data_ptr(), ws_n, _stream_ptr()), None, "pf_fit_camera_shared")
    iters = out[:, 10].to(torch.int32)
    conv = out[:, 11] != 0
    valid = out[:, 12].to(torch.int64)
    res = [None] * B
    row = 0
    for g, idx in members.items():
        group_cost = out[row:row + len(idx), 9].to(torch.float64).sum()
        for i in idx:
            d = {k: out[row, j] for j, k in enumerate(_FIT_COLS[:10])}
            d["fit_iterations"], d["fit_converged"], d["fit_valid_pixels"] = iters[row], conv[row], valid[row]
            if distortion:
                d["pred_xi"] = out[row, 13]
            d["fit_group_cost"], d["fit_group"] = group_cost, g
            res[i] = d
            row += 1
    return res


# columns of the pf_fit_fisheye output row (PF_FISHFIT_COL_*): the pinhole row, then k1, k2
_FISHFIT_COLS = _FIT_COLS + ("pred_k1", "pred_k2")


def fit_fisheye_lens(up, lat, *, projection="equidistant", free_principal_point=False, distortion=False, max_fov=230.0, loss="l2", huber_delta_deg=2.0,
                     weights=(1.0, 1.0), max_iter=20, init=None):
    """Perspective fields -> a fisheye lens on the GPU: the inverse of `fisheye_fields` / `panorama_to_fisheye(fields=True)` for one lens, a per-image
    Levenberg-Marquardt fit of the lens model (include/pf_hip.h pf_fit_fisheye) to an up field (2,H,W) and a latitude map (H,W) in degrees.

    up / lat: one pair of device tensors, or lists of pairs (sizes may differ; one launch sequence per 32 images).  Pixels outside the image circle
    are expected as NaN in either field: they are skipped.  For a dual-fisheye frame fit each half on its own.
    projection: "equidistant", "equisolid" or "stereographic", the kind of the lens (it is not fitted).  Free parameters: roll, pitch and rel_focal
    (F = rel_focal * H); with free_principal_point also rel_cx / rel_cy (the circle's centre, (rel_cx + 1/2) W, (rel_cy + 1/2) H); with
    distortion=True also k1, k2 of the Kannala-Brandt polynomial, clamped to [-0.5, 0.5] (k3 = k4 = 0).  What is not free stays at its start
    value: 0 without `init`, so a calibrated k1, k2 in `init` is held while orientation and focal length are fitted.
    max_fov: the widest full field of view the lens may have, in (0, 360) degrees: a pixel whose ray would lie beyond max_fov / 2 has no model value.
    loss, huber_delta_deg, weights, max_iter: as fit_camera_params.  init: optional start, one dict (or a list of dicts) with pred_roll, pred_pitch
    (degrees), pred_rel_focal and optionally pred_rel_cx, pred_rel_cy, pred_k1, pred_k2 -- e.g. an earlier result.  Without it the start is blind:
    roll and pitch from the centre pixels, the centre in the middle, no polynomial, rel_focal the best of 16 candidates.

    Returns one dict per image (a single dict for a single pair): pred_roll, pred_pitch (degrees), pred_rel_focal, pred_rel_cx, pred_rel_cy,
    pred_k1, pred_k2, fit_rms_up_deg, fit_rms_lat_deg, fit_cost, fit_iterations, fit_converged, fit_valid_pixels (pixels with finite input and a
    model value) -- 0-d device tensors, no host synchronisation -- plus fit_projection and fit_max_fov, the two arguments, for
    `fisheye_lens_from_fit`.  GPU only: CPU tensors raise PfError."""
    from .engine import _check, _stream_ptr, load_library
    from .gathers import _fisheye_kind

    fn = "fit_fisheye_lens"
    kind = _fisheye_kind(fn, projection)
    max_fov = float(max_fov)
    if not 0.0 < max_fov < 360.0:
        raise ValueError(f"{fn}: max_fov must be in (0, 360) degrees; got {max_fov!r}")
    theta_max = float(np.float32(math.radians(0.5 * max_fov)))
    if not 0.0 < theta_max < math.pi:   # the float32 the library gets
        raise ValueError(f"{fn}: max_fov must be in (0, 360) degrees; got {max_fov!r}")
    single, ups, lats, dev = _fit_fields(fn, up, lat, loss)
    B = len(ups)
    d_init = _fit_init_rows(init, B, dev, True, ("pred_k1", "pred_k2"))
    hw = (ctypes.c_int32 * (2 * B))(*[s for u in ups for s in (int(u.shape[1]), int(u.shape[2]))])
    p_up = (ctypes.c_void_p * B)(*[u.data_ptr() for u in ups])
    p_lat = (ctypes.c_void_p * B)(*[l.data_ptr() for l in lats])
    lib = load_library()
    ws_n = int(lib.pf_fit_fisheye_workspace_bytes(B, hw))
    if ws_n == 0:
        small = [tuple(u.shape[1:]) for u in ups if min(u.shape[1:]) < 8]
        raise PfError(f"{fn}: images must be at least 8 x 8 (got {small})")
    ws = torch.empty(ws_n, dtype=torch.uint8, device=dev)
    out = torch.empty((B, len(_FISHFIT_COLS)), dtype=torch.float32, device=dev)
    w_up, w_lat = (float(w) for w in weights)
    with torch.cuda.device(dev):
        _check(lib.pf_fit_fisheye(dev.index, kind, B, hw, p_up, p_lat, d_init.data_ptr() if d_init is not None else None, int(bool(free_principal_point)),
                                  int(bool(distortion)), theta_max, _FIT_LOSSES[loss], float(huber_delta_deg), w_up, w_lat, int(max_iter), out.data_ptr(),
                                  ws.data_ptr(), ws_n, _stream_ptr()), None, "pf_fit_fisheye")
    iters = out[:, 10].to(torch.int32)
    conv = out[:, 11] != 0
    valid = out[:, 12].to(torch.int64)
    res = []
    for i in range(B):
        d = {k: out[i, j] for j, k in enumerate(_FISHFIT_COLS) if k.startswith("fit_") or k in _FISHEYE_PRED}
        d["fit_iterations"], d["fit_converged"], d["fit_valid_pixels"] = iters[i], conv[i], valid[i]
        d["fit_projection"], d["fit_max_fov"] = projection, max_fov
        res.append(d)
    return res[0] if single else res


# what a lens fit returns of the row: pred_vfov / pred_general_vfov describe nothing for a fisheye lens
_FISHEYE_PRED = ("pred_roll", "pred_pitch", "pred_rel_focal", "pred_rel_cx", "pred_rel_cy", "pred_k1", "pred_k2")


def fisheye_lens_from_fit(fit, *, height, width, fov=None, yaw=0.0, band=0.0):
    """A result of `fit_fisheye_lens` for a (height, width) frame -> the lens row of `fisheye_lens`, 12 float64 values as a numpy array, for
    `crop_fisheye`, `fisheye_to_panorama`, `panorama_to_fisheye` and `fisheye_fields`.  Reading the seven fitted values off the device costs ONE
    host synchronisation.  fov: the field of view the row covers, in degrees (default: the fit's max_fov); yaw, band (degrees): as fisheye_lens -- the
    fields say nothing about either.  The projection is the fit's.  A fitted polynomial that is not monotone on [0, fov / 2] raises fisheye_lens's
    ValueError: it is not a lens."""
    from .gathers import _FISHEYE_RHO, fisheye_lens

    fn = "fisheye_lens_from_fit"
    if not isinstance(fit, dict) or not set(_FISHEYE_PRED) <= set(fit):
        raise ValueError(f"{fn}: fit must be one result dict of fit_fisheye_lens with {', '.join(_FISHEYE_PRED)}")
    H, W = int(height), int(width)
    if H < 1 or W < 1:
        raise ValueError(f"{fn}: height and width must be >= 1; got {height} x {width}")
    projection = fit.get("fit_projection", "equidistant")
    fov = float(fit.get("fit_max_fov", 230.0) if fov is None else fov)
    vals = [fit[k] for k in _FISHEYE_PRED]
    if any(torch.is_tensor(v) for v in vals):   # one read for all seven
        dev = next(v.device for v in vals if torch.is_tensor(v))
        vals = torch.stack([torch.as_tensor(v, dtype=torch.float64).to(dev).reshape(()) for v in vals]).cpu().tolist()
    roll, pitch, f, cx, cy, k1, k2 = (float(v) for v in vals)
    F = f * H
    t = math.radians(0.5 * fov)
    t2 = t * t
    with np.errstate(all="ignore"):
        radius = F * float(_FISHEYE_RHO.get(projection, _FISHEYE_RHO["equidistant"])(t * (1.0 + t2 * (k1 + t2 * k2))))
    row = fisheye_lens(fov, radius=radius, center=((cx + 0.5) * W, (cy + 0.5) * H), projection=projection, k=(k1, k2, 0.0, 0.0), roll=roll, pitch=pitch,
                       yaw=yaw, band=band)
    row[3] = F   # exactly the fitted focal length, not radius / rho(theta_d(fov / 2)) rounded once more
    return row
