"""Perspective-aware compositing on the GPU: placement scores (pf_place_scores), field transforms (pf_fields_transform), the search over sizes and
tilts (pf_place_search) and the paste itself (pf_composite)."""
from __future__ import annotations

import ctypes
import operator

import numpy as np
import torch

from .draw import _draw_images
from .engine import PfError
from .field_metrics import _field_list
from .gathers import _PANO_DTYPES, _check_samples


def placement_scores(up_bg, lat_bg, up_obj, lat_obj, *, mask=None, stride=1, pairs=None, min_valid=0.5, weights=(1.0, 1.0)):
    """Perspective-aware compositing on the GPU: the Perspective Field Discrepancy (PFD) of an object cut from one picture against a background
    at every place it could be pasted -- the mean up-vector angle plus the mean latitude difference over the object's pixels; a low PFD is what
    people judge as "fits".  Definitions: include/pf_hip.h pf_place_scores.

    up_bg (2,H,W), lat_bg (H,W) and up_obj (2,h,w), lat_obj (h,w) in degrees with h <= H, w <= W (the layout of `pred_gravity_original` /
    `pred_latitude_original` and of crop_panorama's labels): one set of device tensors each, batched tensors, or lists (sizes may differ).  A
    pixel with a non-finite value or an up vector shorter than 1e-6 is invalid in its own field, and a pixel pair counts only where both are
    valid: a NaN latitude masks a pixel, a silhouette is NaN outside the object, a background padded with NaN lets the object hang over the
    border.  mask: a bool (h,w) tensor, or a list of one per object (None entries allowed), True on the object; applied as NaN on a copy of
    the object's latitude.  The placement (j, i) puts the object's corner on background pixel (j stride, i stride); there are
    P x Q = ((H - h) // stride + 1) x ((W - w) // stride + 1) of them.  pairs: (background, object) index pairs, default every combination,
    backgrounds outermost.
    Returns one dict per pair (a single dict when both sides are a single set) of device tensors, no host synchronisation:
    up_mean_deg, lat_mean_deg (P,Q) float64, the means over the valid pairs (NaN where there is none); pfd_deg (P,Q) float64 =
    weights[0] up_mean_deg + weights[1] lat_mean_deg, the paper's sum at the default (1, 1), +inf where fewer than min_valid x (valid pixels of
    the object) pairs are valid or the object has no valid pixel; valid_pixels (P,Q) int64; best_offset (2,) int64, (row, col) of the lowest
    PFD in background pixels, the first in row-major order, (-1, -1) when every placement is +inf; best_pfd_deg; stride.
    The fields of a resized crop are the resized fields: transform_fields resizes and turns them, and placement_search runs this function over a
    set of scales and rotations and finds the best of all on the device.  Deterministic; a pair's numbers do not depend on the other pairs.  GPU
    only: CPU tensors raise PfError."""
    from .engine import _check, _stream_ptr, load_library

    fn = "placement_scores"
    s_b, ups_b, lats_b = _field_list("background", up_bg, lat_bg, fn)
    s_o, ups_o, lats_o = _field_list("object", up_obj, lat_obj, fn)
    if not ups_b or not ups_o:
        raise ValueError(f"{fn} needs at least one background and one object")
    every = ups_b + lats_b + ups_o + lats_o
    if not all(torch.is_tensor(t) for t in every):
        raise TypeError(f"{fn} takes torch tensors")
    for u, l in zip(ups_b + ups_o, lats_b + lats_o):
        if u.dim() != 3 or u.shape[0] != 2 or min(u.shape[1:]) < 1 or tuple(l.shape) != tuple(u.shape[1:]):
            raise ValueError(f"up must be (2, H, W) and lat (H, W) with H, W >= 1; got {tuple(u.shape)} and {tuple(l.shape)}")
    stride = operator.index(stride)
    if stride < 1:
        raise ValueError(f"stride must be at least 1; got {stride}")
    min_valid = float(min_valid)
    if not 0.0 <= min_valid <= 1.0:
        raise ValueError(f"min_valid must be in [0, 1]; got {min_valid}")
    w_up, w_lat = (float(v) for v in weights)
    if not (w_up >= 0.0 and w_lat >= 0.0 and np.isfinite(w_up) and np.isfinite(w_lat)):
        raise ValueError(f"weights must be two finite numbers >= 0; got {weights}")
    nb, no = len(ups_b), len(ups_o)
    if pairs is None:
        plist = [(b, o) for b in range(nb) for o in range(no)]
    else:
        plist = [(operator.index(b), operator.index(o)) for b, o in (pairs.tolist() if torch.is_tensor(pairs) else pairs)]
        if not plist:
            raise ValueError(f"{fn} needs at least one pair")
    single = s_b and s_o and len(plist) == 1
    for b, o in plist:
        if not (0 <= b < nb and 0 <= o < no):
            raise ValueError(f"a pair is (background, object) with indices in [0, {nb}) and [0, {no}); got ({b}, {o})")
        if ups_o[o].shape[1] > ups_b[b].shape[1] or ups_o[o].shape[2] > ups_b[b].shape[2]:
            raise ValueError(f"the object {tuple(ups_o[o].shape[1:])} is larger than its background {tuple(ups_b[b].shape[1:])}")
    masks = [None] * no if mask is None else [mask] if torch.is_tensor(mask) else list(mask)
    if len(masks) != no:
        raise ValueError(f"{len(masks)} masks for {no} objects")
    for m, l in zip(masks, lats_o):
        if m is not None and (not torch.is_tensor(m) or m.dtype != torch.bool or tuple(m.shape) != tuple(l.shape)):
            raise ValueError(f"a mask is a bool tensor of its object's size {tuple(l.shape)}")
    every += [m for m in masks if m is not None]
    if not all(t.is_cuda for t in every):
        raise PfError(f"{fn} runs on the GPU only (no CPU path)")
    dev = every[0].device
    if any(t.device != dev for t in every):
        raise ValueError(f"{fn}: all fields and masks must be on one device")
    ups_b, lats_b, ups_o, lats_o = ([t.to(torch.float32).contiguous() for t in ts] for ts in (ups_b, lats_b, ups_o, lats_o))
    lats_o = [l if m is None else torch.where(m, l, torch.full_like(l, float("nan"))) for l, m in zip(lats_o, masks)]
    ptrs = lambda ts: (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])
    sizes = lambda ts: (ctypes.c_int32 * (2 * len(ts)))(*[s for u in ts for s in (int(u.shape[1]), int(u.shape[2]))])
    hw_b, hw_o = sizes(ups_b), sizes(ups_o)
    n_pair = len(plist)
    c_pairs = (ctypes.c_int32 * (2 * n_pair))(*[i for bo in plist for i in bo])
    dims = [((ups_b[b].shape[1] - ups_o[o].shape[1]) // stride + 1, (ups_b[b].shape[2] - ups_o[o].shape[2]) // stride + 1) for b, o in plist]
    lib = load_library()
    need = int(lib.pf_place_scores_workspace_bytes(nb, hw_b, no, hw_o, n_pair, c_pairs, stride))
    if need == 0:
        raise ValueError(f"{fn}: field sizes that one call does not take (2^31 pixels or more, or an object of more than 65535 x 1024 pixels)")
    out = torch.empty(3 * sum(P * Q for P, Q in dims), dtype=torch.float64, device=dev)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _check(lib.pf_place_scores(dev.index, nb, ptrs(ups_b), ptrs(lats_b), hw_b, no, ptrs(ups_o), ptrs(lats_o), hw_o, n_pair, c_pairs, stride,
                                   out.data_ptr(), ws.data_ptr(), need, _stream_ptr()), None, "pf_place_scores")
    # the valid pixels of every object, by the kernel's rule in float32 (a * a + b * b rounds twice where the kernel's fmaf rounds once: the two can
    # differ only for a squared length within an ulp of 1e-12)
    obj_valid = []
    for u, l in zip(ups_o, lats_o):
        l2 = u[0] * u[0] + u[1] * u[1]
        obj_valid.append((torch.isfinite(l) & (l2 >= 1e-12) & torch.isfinite(l2)).sum().to(torch.float64))
    inf = torch.tensor(float("inf"), dtype=torch.float64, device=dev)
    res, first = [], 0
    for (b, o), (P, Q) in zip(plist, dims):
        rec = out[first:first + 3 * P * Q].view(P, Q, 3)
        first += 3 * P * Q
        n = rec[..., 2]
        up_mean, lat_mean = rec[..., 0] / n, rec[..., 1] / n   # NaN where n = 0
        ok = (n >= min_valid * obj_valid[o]) & (n > 0)
        pfd = torch.where(ok, w_up * up_mean + w_lat * lat_mean, inf)
        best = pfd.min()
        flat = torch.where(pfd.reshape(-1) == best, torch.arange(P * Q, device=dev), P * Q).min()   # the first of equal minima
        at = torch.stack([torch.div(flat, Q, rounding_mode="floor"), flat % Q]) * stride
        res.append(dict(pfd_deg=pfd, up_mean_deg=up_mean, lat_mean_deg=lat_mean, valid_pixels=n.to(torch.int64),
                        best_offset=torch.where(torch.isfinite(best), at, torch.full_like(at, -1)), best_pfd_deg=best, stride=stride))
    return res[0] if single else res


def _variant_values(name, v, fn):
    """a scalar or a sequence of finite floats -> (is a scalar, [float])"""
    scalar = not isinstance(v, (list, tuple, np.ndarray)) and not (torch.is_tensor(v) and v.dim() > 0)
    vals = [float(v)] if scalar else [float(x) for x in (v.tolist() if torch.is_tensor(v) or isinstance(v, np.ndarray) else v)]
    if not vals:
        raise ValueError(f"{fn}: {name} is empty")
    if not all(np.isfinite(x) for x in vals) or (name.startswith("scale") and not all(x > 0.0 for x in vals)):
        raise ValueError(f"{fn}: {name} must be finite{' and > 0' if name.startswith('scale') else ''}; got {vals}")
    return scalar, vals


def _masked_latitudes(lats, mask, what, fn):
    """the checks of mask= and the masks as a list, one per field (None entries allowed)"""
    masks = [None] * len(lats) if mask is None else [mask] if torch.is_tensor(mask) else list(mask)
    if len(masks) != len(lats):
        raise ValueError(f"{fn}: {len(masks)} masks for {len(lats)} {what}")
    for m, l in zip(masks, lats):
        if m is not None and (not torch.is_tensor(m) or m.dtype != torch.bool or tuple(m.shape) != tuple(l.shape)):
            raise ValueError(f"{fn}: a mask is a bool tensor of its field's size {tuple(l.shape)}")
    return masks


def transform_fields(up, lat, *, scale=1.0, rotation=0.0, mask=None, height=None, width=None):
    """The perspective fields of a picture that is resized by `scale` and turned by `rotation` degrees in its plane, on the GPU: the field-aware
    resample that an image resize is not -- NaN is the mask and must not spread, up vectors are mixed as vectors and made unit again, and a rotation
    turns the vectors with the picture.  Definitions: include/pf_hip.h pf_fields_transform.

    up (2,h,w), lat (h,w) in degrees (the layout of `pred_gravity_original` / `pred_latitude_original`): one field of device tensors, a batched
    pair, or lists.  scale > 0; rotation in degrees, positive = clockwise on the screen, the fields of a camera whose roll is lower by that much.
    Both are scalars or sequences of one length: a sequence gives a list of (up', lat'), one per variant.  The output is
    h' = max(1, floor(scale (h |cos| + w |sin|) + 1/2)) high, w' likewise with h and w exchanged, unless height= / width= say otherwise; the picture's
    centre stays the centre.  Four bilinear taps per pixel; a tap outside the array or on an invalid pixel (a non-finite value, an up vector shorter
    than 1e-6) is dropped, and the pixel is valid where the taps left carry at least half of the weight: NaN in all three planes otherwise.  So a
    silhouette keeps its outline to half a pixel and the array border behaves like a clamp.  There is no prefilter: fields are smooth, and only a
    silhouette aliases when scale is far below 1.  mask: a bool (h,w) tensor (or one per field), True inside; applied as NaN on a copy of the latitude.
    scale=1, rotation=0 returns the bits of a field of unit up vectors.  Returns (up', lat') float32 device tensors, a list of them for sequences, a
    list per field for several fields; no host synchronisation.  Deterministic; a variant's bits do not depend on the others.  GPU only: CPU
    tensors raise PfError."""
    from .engine import _check, _stream_ptr, load_library

    fn = "transform_fields"
    single, ups, lats = _field_list("source", up, lat, fn)
    if not ups:
        raise ValueError(f"{fn} needs at least one field")
    if not all(torch.is_tensor(t) for t in ups + lats):
        raise TypeError(f"{fn} takes torch tensors")
    for u, l in zip(ups, lats):
        if u.dim() != 3 or u.shape[0] != 2 or min(u.shape[1:]) < 1 or tuple(l.shape) != tuple(u.shape[1:]):
            raise ValueError(f"up must be (2, h, w) and lat (h, w) with h, w >= 1; got {tuple(u.shape)} and {tuple(l.shape)}")
    s_scalar, scales = _variant_values("scale", scale, fn)
    r_scalar, rots = _variant_values("rotation", rotation, fn)
    if s_scalar != r_scalar:
        scales, rots = (scales * len(rots), rots) if s_scalar else (scales, rots * len(scales))
    if len(scales) != len(rots):
        raise ValueError(f"{fn}: {len(scales)} scales for {len(rots)} rotations")
    size = [None if v is None else operator.index(v) for v in (height, width)]
    if any(v is not None and v < 1 for v in size):
        raise ValueError(f"{fn}: height and width must be at least 1; got {height}, {width}")
    masks = _masked_latitudes(lats, mask, "fields", fn)
    every = ups + lats + [m for m in masks if m is not None]
    if not all(t.is_cuda for t in every):
        raise PfError(f"{fn} runs on the GPU only (no CPU path)")
    dev = every[0].device
    if any(t.device != dev for t in every):
        raise ValueError(f"{fn}: all fields and masks must be on one device")
    ups, lats = ([t.to(torch.float32).contiguous() for t in ts] for ts in (ups, lats))
    lats = [l if m is None else torch.where(m, l, torch.full_like(l, float("nan"))) for l, m in zip(lats, masks)]
    lib = load_library()
    jobs, outs = [], []
    for u, l in zip(ups, lats):
        res = []
        for s, r in zip(scales, rots):
            hw = (ctypes.c_int32 * 2)()
            if lib.pf_fields_transform_size(int(u.shape[1]), int(u.shape[2]), s, r, hw) != 0:
                raise ValueError(f"{fn}: {lib.pf_last_error(None).decode()}")
            ho, wo = (hw[0] if size[0] is None else size[0]), (hw[1] if size[1] is None else size[1])
            if ho * wo >= 2 ** 31:
                raise ValueError(f"{fn}: an output of {ho} x {wo} has 2^31 pixels or more")
            o_up, o_lat = torch.empty((2, ho, wo), dtype=torch.float32, device=dev), torch.empty((ho, wo), dtype=torch.float32, device=dev)
            jobs.append((u, l, s, r, ho, wo, o_up, o_lat))
            res.append((o_up, o_lat))
        outs.append(res[0] if s_scalar and r_scalar else res)
    n = len(jobs)
    ptrs = lambda k: (ctypes.c_void_p * n)(*[j[k].data_ptr() for j in jobs])
    c_hw = (ctypes.c_int32 * (2 * n))(*[v for j in jobs for v in (int(j[0].shape[1]), int(j[0].shape[2]))])
    c_var = (ctypes.c_double * (2 * n))(*[v for j in jobs for v in (j[2], j[3])])
    c_out = (ctypes.c_int32 * (2 * n))(*[v for j in jobs for v in (j[4], j[5])])
    with torch.cuda.device(dev):
        _check(lib.pf_fields_transform(dev.index, n, ptrs(0), ptrs(1), c_hw, c_var, c_out, ptrs(6), ptrs(7), _stream_ptr()), None, "pf_fields_transform")
    return outs[0] if single else outs


def placement_search(up_bg, lat_bg, up_obj, lat_obj, *, scales=(1.0,), rotations=(0.0,), mask=None, stride=1, pairs=None, min_valid=0.5, weights=(1.0, 1.0),
                     return_maps=False):
    """placement_scores over a set of sizes and in-plane tilts of the object, and the best of all of them found on the GPU: where, how large and how
    tilted the object fits its background best.  Definitions: include/pf_hip.h pf_place_search.

    The fields, mask, stride, pairs, min_valid and weights are placement_scores'; an object larger than its background is no error here.  The
    variants are the product scales x rotations, scales outermost: variant v = (scales[v // R], rotations[v % R]).  Each object is transformed by each
    variant (transform_fields, the mask applied first) and scored at every offset; min_valid counts against the valid pixels of the transformed
    object.  A variant whose transformed object does not fit its background is skipped: +inf, offset (-1, -1).
    Returns one dict per pair (a single dict under placement_scores' rule) of device tensors, no host synchronisation:
    best_scale, best_rotation_deg (float64, NaN when every placement of every variant is +inf), best_variant (int64, -1 then), best_offset (2,) int64
    (row, col) in background pixels, best_pfd_deg, best_up_mean_deg, best_lat_mean_deg, best_size (2,) int64 (h', w' of the best variant, (-1, -1)
    without one); variant_pfd_deg (V,), variant_offset (V,2), variant_size (V,2), variant_valid_pixels (V,); stride.  Ties go to the lowest variant,
    then to the first placement in row-major order.  With return_maps also maps: per variant the dict placement_scores returns for the transformed
    object (its arrays are views of one buffer; the same bits), None for a skipped variant.  Deterministic; a pair's numbers do not depend on the
    other pairs.  GPU only: CPU tensors raise PfError."""
    from .engine import _check, _stream_ptr, load_library

    fn = "placement_search"
    s_b, ups_b, lats_b = _field_list("background", up_bg, lat_bg, fn)
    s_o, ups_o, lats_o = _field_list("object", up_obj, lat_obj, fn)
    if not ups_b or not ups_o:
        raise ValueError(f"{fn} needs at least one background and one object")
    every = ups_b + lats_b + ups_o + lats_o
    if not all(torch.is_tensor(t) for t in every):
        raise TypeError(f"{fn} takes torch tensors")
    for u, l in zip(ups_b + ups_o, lats_b + lats_o):
        if u.dim() != 3 or u.shape[0] != 2 or min(u.shape[1:]) < 1 or tuple(l.shape) != tuple(u.shape[1:]):
            raise ValueError(f"up must be (2, H, W) and lat (H, W) with H, W >= 1; got {tuple(u.shape)} and {tuple(l.shape)}")
    sc = _variant_values("scales", scales, fn)[1]
    ro = _variant_values("rotations", rotations, fn)[1]
    variants = [(s, r) for s in sc for r in ro]
    V = len(variants)
    stride = operator.index(stride)
    if stride < 1:
        raise ValueError(f"stride must be at least 1; got {stride}")
    min_valid = float(min_valid)
    if not 0.0 <= min_valid <= 1.0:
        raise ValueError(f"min_valid must be in [0, 1]; got {min_valid}")
    w_up, w_lat = (float(v) for v in weights)
    if not (w_up >= 0.0 and w_lat >= 0.0 and np.isfinite(w_up) and np.isfinite(w_lat)):
        raise ValueError(f"weights must be two finite numbers >= 0; got {weights}")
    nb, no = len(ups_b), len(ups_o)
    if pairs is None:
        plist = [(b, o) for b in range(nb) for o in range(no)]
    else:
        plist = [(operator.index(b), operator.index(o)) for b, o in (pairs.tolist() if torch.is_tensor(pairs) else pairs)]
        if not plist:
            raise ValueError(f"{fn} needs at least one pair")
    single = s_b and s_o and len(plist) == 1
    for b, o in plist:
        if not (0 <= b < nb and 0 <= o < no):
            raise ValueError(f"a pair is (background, object) with indices in [0, {nb}) and [0, {no}); got ({b}, {o})")
    masks = _masked_latitudes(lats_o, mask, "objects", fn)
    every += [m for m in masks if m is not None]
    if not all(t.is_cuda for t in every):
        raise PfError(f"{fn} runs on the GPU only (no CPU path)")
    dev = every[0].device
    if any(t.device != dev for t in every):
        raise ValueError(f"{fn}: all fields and masks must be on one device")
    ups_b, lats_b, ups_o, lats_o = ([t.to(torch.float32).contiguous() for t in ts] for ts in (ups_b, lats_b, ups_o, lats_o))
    lats_o = [l if m is None else torch.where(m, l, torch.full_like(l, float("nan"))) for l, m in zip(lats_o, masks)]
    ptrs = lambda ts: (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])
    sizes = lambda ts: (ctypes.c_int32 * (2 * len(ts)))(*[s for u in ts for s in (int(u.shape[1]), int(u.shape[2]))])
    hw_b, hw_o = sizes(ups_b), sizes(ups_o)
    n_pair = len(plist)
    c_pairs = (ctypes.c_int32 * (2 * n_pair))(*[i for bo in plist for i in bo])
    c_var = (ctypes.c_double * (2 * V))(*[x for sr in variants for x in sr])
    lib = load_library()
    need = int(lib.pf_place_search_workspace_bytes(nb, hw_b, no, hw_o, n_pair, c_pairs, V, c_var, stride))
    if need == 0:
        raise ValueError(f"{fn}: sizes that one call does not take (a field or a transformed object of 2^31 pixels or more, or of more than 65535 x 1024)")
    # the sizes of the maps, as the library lays them out: the transformed size of every (object, variant)
    ohw = {}
    for o in {o for _, o in plist}:
        for v, (s, r) in enumerate(variants):
            hw = (ctypes.c_int32 * 2)()
            _check(lib.pf_fields_transform_size(int(ups_o[o].shape[1]), int(ups_o[o].shape[2]), s, r, hw), None, "pf_fields_transform_size")
            ohw[o, v] = (hw[0], hw[1])
    dims = []   # per pair, per variant: (P, Q) or None
    for b, o in plist:
        H, W = ups_b[b].shape[1:]
        dims.append([((H - ohw[o, v][0]) // stride + 1, (W - ohw[o, v][1]) // stride + 1) if ohw[o, v][0] <= H and ohw[o, v][1] <= W else None for v in range(V)])
    n_maps = 3 * sum(d[0] * d[1] for dv in dims for d in dv if d is not None)
    maps = torch.empty(max(n_maps, 1), dtype=torch.float64, device=dev)
    best = torch.empty((n_pair, 7), dtype=torch.float64, device=dev)
    var = torch.empty((n_pair, V, 6), dtype=torch.float64, device=dev)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _check(lib.pf_place_search(dev.index, nb, ptrs(ups_b), ptrs(lats_b), hw_b, no, ptrs(ups_o), ptrs(lats_o), hw_o, n_pair, c_pairs, V, c_var, stride,
                                   min_valid, w_up, w_lat, maps.data_ptr(), n_maps, best.data_ptr(), var.data_ptr(), ws.data_ptr(), need, _stream_ptr()),
               None, "pf_place_search")
    t_var = torch.tensor(variants + [(float("nan"), float("nan"))], dtype=torch.float64, device=dev)   # row -1: no variant
    t_size = var[..., 4:6].to(torch.int64)
    inf = torch.tensor(float("inf"), dtype=torch.float64, device=dev)
    res, first = [], 0
    for k, dv in enumerate(dims):
        bv = best[k, 4].to(torch.int64)
        d = dict(best_scale=t_var[bv, 0], best_rotation_deg=t_var[bv, 1], best_variant=bv, best_offset=best[k, 5:7].to(torch.int64), best_pfd_deg=best[k, 0],
                 best_up_mean_deg=best[k, 1], best_lat_mean_deg=best[k, 2],
                 best_size=torch.where(bv >= 0, t_size[k][bv.clamp(min=0)], torch.full_like(t_size[k][0], -1)),
                 variant_pfd_deg=var[k, :, 0], variant_offset=var[k, :, 1:3].to(torch.int64), variant_size=t_size[k],
                 variant_valid_pixels=var[k, :, 3].to(torch.int64), stride=stride)
        if return_maps:
            ms = []
            for v, pq in enumerate(dv):
                if pq is None:
                    ms.append(None)
                    continue
                P, Q = pq
                rec = maps[first:first + 3 * P * Q].view(P, Q, 3)
                first += 3 * P * Q
                n = rec[..., 2]
                up_mean, lat_mean = rec[..., 0] / n, rec[..., 1] / n
                ok = (n >= min_valid * var[k, v, 3]) & (n > 0)
                at = var[k, v, 1:3].to(torch.int64)
                ms.append(dict(pfd_deg=torch.where(ok, w_up * up_mean + w_lat * lat_mean, inf), up_mean_deg=up_mean, lat_mean_deg=lat_mean,
                               valid_pixels=n.to(torch.int64), best_offset=at, best_pfd_deg=var[k, v, 0], stride=stride))
            d["maps"] = ms
        res.append(d)
    return res[0] if single else res


COMPOSITE_SOFT, COMPOSITE_HARD = 0, 1   # include/pf_hip.h PF_COMPOSITE_*
_EDGES = {"soft": COMPOSITE_SOFT, "hard": COMPOSITE_HARD}


def _placement_columns(fn, name, v, width, n):
    """a per-job parameter of composite_objects -> (is a tensor, `width` columns): host numbers give lists of n floats, a device tensor gives float64
    tensors of shape (n,) that were never read"""
    if torch.is_tensor(v):
        shape = tuple(v.shape)
        ok = shape in ((), (n,)) if width == 1 else shape in ((width,), (n, width))
        if not ok or v.dtype == torch.bool or v.is_complex():
            raise ValueError(f"{fn}: {name} as a tensor is {'a number or (n,)' if width == 1 else f'({width},) or (n, {width})'} for n = {n} jobs; got {shape}")
        t = v.to(torch.float64).reshape(-1, width).expand(n, width)
        return True, [t[:, i] for i in range(width)]
    try:
        a = np.asarray(v, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"{fn}: {name} must be numbers or a tensor; got {v!r}") from None
    ok = a.shape in ((), (n,)) if width == 1 else a.shape in ((width,), (n, width))
    if not ok:
        raise ValueError(f"{fn}: {name} is {'a number or n numbers' if width == 1 else f'{width} numbers or n rows of them'} for n = {n} jobs; got shape {a.shape}")
    a = np.broadcast_to(a.reshape(-1, width), (n, width))
    return False, [[float(x) for x in a[:, i]] for i in range(width)]


def composite_objects(backgrounds, objects, *, scale=1.0, rotation=0.0, offset, size=None, alpha=None, pairs=None, opacity=1.0, edge="soft", samples=1,
                      return_coverage=False):
    """Objects pasted into background pictures on the GPU: the object's pixels resized by `scale` and turned by `rotation` degrees about its centre
    (transform_fields' similarity, so the pixels move as the fields did), alpha-blended into the background at `offset`.  It consumes what
    placement_search finds -- its best_scale, best_rotation_deg, best_offset and best_size can be passed as the device tensors they are, and nothing is
    read back.  Definitions: include/pf_hip.h pf_composite.

    backgrounds, objects: a CUDA tensor (H, W, 3), a batch (B, H, W, 3), or a list of (H, W, 3) tensors whose sizes may differ; uint8 or float32 on the
    0 - 255 scale, one dtype and one device for all.  An object may have 4 channels: colour and alpha on the 0 - 255 scale.  alpha: a bool or float
    (h, w) tensor in [0, 1] (one, or a list with one entry per object, None entries allowed), None = opaque; NaN counts as 0.
    pairs: (background, object) indices, one job each; default every background with every object, backgrounds outermost (placement_search's order).
    Per job, as host numbers (one for all jobs or one per job) or as device tensors (0-d / (n,), offset and size (2,) / (n, 2)):
    scale > 0; rotation in degrees, positive = clockwise on the screen; offset = (row, col) of the top-left corner of the transformed object's box in
    the background, which may be negative or hang over the border (the paste is clipped); size = (h', w') of that box, default the size
    transform_fields gives, which needs scale and rotation as host numbers: with tensors pass size=.  A job whose values cannot be pasted -- a scale
    that is not finite and > 0, a non-finite rotation, an offset that is not integer-valued, a size below 1 (placement_search's "nothing fits") --
    returns its background unchanged.
    opacity in [0, 1] multiplies the alpha.  edge="soft": the premultiplied bilinear mix, the object's outline and the array border fade over a pixel;
    edge="hard": a pixel is pasted in full where the resampled alpha is at least 1/2 and not at all elsewhere -- transform_fields' silhouette, the
    pixels the search scored.  samples=S in 1 .. 4: every pixel is the mean of S x S sub-samples (antialiasing for scale < 1), as for the gathers.
    Returns the composites: (H, W, 3) for one background tensor and one object tensor, (n, H, W, 3) for one background or a batch of them, a list for
    a list; with return_coverage also the coverage in [0, 1], float32, (H, W) per job in the same arrangement.  A pixel that is not covered keeps
    the background's bits.  uint8 results are rounded half up.  One C call on the current stream, no host synchronisation.  Deterministic; a
    job's bits do not depend on the other jobs.  GPU only: CPU tensors raise PfError."""
    from .engine import _check, _stream_ptr, load_library

    fn = "composite_objects"
    kind_b, bgs = _draw_images(fn, backgrounds)
    kind_o, objs = _draw_images(fn, objects)
    if not all(torch.is_tensor(t) for t in bgs + objs):
        raise TypeError(f"{fn} takes torch tensors")
    for what, kind, ts, chans in (("a background", kind_b, bgs, (3,)), ("an object", kind_o, objs, (3, 4))):
        for t in ts:
            if t.dim() != (4 if kind == "batched" else 3) or t.shape[-1] not in chans or min(t.shape[-3:-1]) < 1 or (kind == "batched" and t.shape[0] < 1):
                raise ValueError(f"{fn}: {what} must be (H, W, {' or '.join(map(str, chans))}) with H, W >= 1, or a non-empty batch of them; got {tuple(t.shape)}")
            if t.dtype not in _PANO_DTYPES:
                raise ValueError(f"{fn}: images must be uint8 or float32; got {t.dtype}")
    if not bgs or not objs:
        raise ValueError(f"{fn} needs at least one background and one object")
    if len({t.dtype for t in bgs + objs}) != 1:
        raise ValueError(f"{fn}: backgrounds and objects must have one dtype")
    bgs = list(bgs[0].unbind(0)) if kind_b == "batched" else bgs
    objs = list(objs[0].unbind(0)) if kind_o == "batched" else objs
    if len({o.shape[-1] for o in objs}) != 1:
        raise ValueError(f"{fn}: the objects must all have 3 or all have 4 channels")
    nb, no = len(bgs), len(objs)
    if objs[0].shape[-1] == 4:
        if alpha is not None:
            raise ValueError(f"{fn}: alpha= with 4-channel objects, which carry their own")
        alphas = [o[..., 3].to(torch.float32) / 255.0 for o in objs]
        objs = [o[..., :3] for o in objs]
    else:
        alphas = [None] * no if alpha is None else [alpha] if torch.is_tensor(alpha) else list(alpha)
        if len(alphas) != no:
            raise ValueError(f"{fn}: {len(alphas)} alpha planes for {no} objects")
        for a, o in zip(alphas, objs):
            if a is not None and (not torch.is_tensor(a) or tuple(a.shape) != tuple(o.shape[:2]) or not (a.dtype == torch.bool or a.is_floating_point())):
                raise ValueError(f"{fn}: an alpha is a bool or float tensor of its object's size {tuple(o.shape[:2])}")
    if pairs is None:
        plist = [(b, o) for b in range(nb) for o in range(no)]
    else:
        plist = [(operator.index(b), operator.index(o)) for b, o in (pairs.tolist() if torch.is_tensor(pairs) else pairs)]
        if not plist:
            raise ValueError(f"{fn} needs at least one pair")
    for b, o in plist:
        if not (0 <= b < nb and 0 <= o < no):
            raise ValueError(f"a pair is (background, object) with indices in [0, {nb}) and [0, {no}); got ({b}, {o})")
    n = len(plist)
    opacity = float(opacity)
    if not 0.0 <= opacity <= 1.0:
        raise ValueError(f"opacity must be in [0, 1]; got {opacity}")
    if edge not in _EDGES:
        raise ValueError(f"edge must be 'soft' or 'hard'; got {edge!r}")
    samples = _check_samples(fn, samples)
    t_scale, (c_scale,) = _placement_columns(fn, "scale", scale, 1, n)
    t_rot, (c_rot,) = _placement_columns(fn, "rotation", rotation, 1, n)
    t_off, c_off = _placement_columns(fn, "offset", offset, 2, n)
    if size is None:
        if t_scale or t_rot:
            raise ValueError(f"{fn}: scale or rotation as tensors are not read back, so the size of the transformed object cannot be derived: pass size=")
        if not all(np.isfinite(s) and s > 0.0 for s in c_scale) or not all(np.isfinite(r) for r in c_rot):
            raise ValueError(f"{fn}: without size=, scale must be finite and > 0 and rotation finite; got {c_scale}, {c_rot}")
        t_size, c_size = False, None
    else:
        t_size, c_size = _placement_columns(fn, "size", size, 2, n)
    params = [c for is_t, cs in ((t_scale, [c_scale]), (t_rot, [c_rot]), (t_off, c_off), (t_size, c_size or [])) if is_t for c in cs]
    every = bgs + objs + [a for a in alphas if a is not None] + params
    if not all(t.is_cuda for t in every):
        raise PfError(f"{fn} runs on the GPU only (no CPU path)")
    dev = bgs[0].device if bgs[0].device.index is not None else torch.device("cuda", torch.cuda.current_device())
    if any((t.device if t.device.index is not None else torch.device("cuda", torch.cuda.current_device())) != dev for t in every):
        raise ValueError(f"{fn}: images, alphas and placement tensors must be on one device")
    lib = load_library()
    if c_size is None:
        c_size = [[], []]
        for (b, o), s, r in zip(plist, c_scale, c_rot):
            hw = (ctypes.c_int32 * 2)()
            if lib.pf_fields_transform_size(int(objs[o].shape[0]), int(objs[o].shape[1]), s, r, hw) != 0:
                raise ValueError(f"{fn}: {lib.pf_last_error(None).decode()}")
            c_size[0].append(float(hw[0]))
            c_size[1].append(float(hw[1]))
    cols = [c_scale, c_rot, *c_off, *c_size]
    if any(torch.is_tensor(c) for c in cols):
        place = torch.stack([c if torch.is_tensor(c) else torch.tensor(c, dtype=torch.float64, device=dev) for c in cols], 1).contiguous()
    else:
        place = torch.tensor([list(row) for row in zip(*cols)], dtype=torch.float64, device=dev)
    bgs, objs = [t.contiguous() for t in bgs], [t.contiguous() for t in objs]
    alphas = [None if a is None else a.to(torch.float32).contiguous() for a in alphas]
    same = len({tuple(bgs[b].shape) for b, _ in plist}) == 1
    if kind_b != "list" and same:
        stack = torch.empty((n,) + tuple(bgs[0].shape), dtype=bgs[0].dtype, device=dev)
        outs = list(stack.unbind(0))
    else:
        stack, outs = None, [torch.empty_like(bgs[b]) for b, _ in plist]
    npx = [int(bgs[b].shape[0]) * int(bgs[b].shape[1]) for b, _ in plist]
    cov = torch.empty(sum(npx), dtype=torch.float32, device=dev) if return_coverage else None
    ptrs = lambda ts: (ctypes.c_void_p * len(ts))(*[None if t is None else t.data_ptr() for t in ts])
    sizes = lambda ts: (ctypes.c_int32 * (2 * len(ts)))(*[int(s) for t in ts for s in t.shape[:2]])
    c_jobs = (ctypes.c_int32 * (2 * n))(*[i for bo in plist for i in bo])
    need = int(lib.pf_composite_workspace_bytes(n))
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _check(lib.pf_composite(dev.index, nb, ptrs(bgs), sizes(bgs), no, ptrs(objs), ptrs(alphas), sizes(objs), _PANO_DTYPES[bgs[0].dtype], n, c_jobs,
                                place.data_ptr(), opacity, _EDGES[edge], samples, ptrs(outs), None if cov is None else cov.data_ptr(), ws.data_ptr(), need,
                                _stream_ptr()), None, "pf_composite")
    single = kind_b == "single" and kind_o == "single" and n == 1
    res = outs[0] if single else outs if stack is None else stack
    if not return_coverage:
        return res
    first = np.concatenate([[0], np.cumsum(npx)])
    covs = [cov[first[k]:first[k + 1]].view(bgs[b].shape[0], bgs[b].shape[1]) for k, (b, _) in enumerate(plist)]
    return res, (covs[0] if single else covs if stack is None else cov.view(n, *bgs[0].shape[:2]))
