"""The angles the perspective fields do not carry: the yaw of views of one centre from their pictures on the GPU (pf_yaw_moments, yaw_tree,
align_yaw), and a panorama's roll and pitch from what was said about views cut out of it (gravity_from_views)."""
from __future__ import annotations

import ctypes
import operator
from collections.abc import Mapping

import numpy as np
import torch

from .gathers import _broadcast_len, _camera_params, _camera_rows, _check_mode, _launch, _param_tensors, _size_array, _source_head, _sources


def _rot_roll_pitch(roll, pitch):
    """R = R_pitch(pitch) R_roll(roll), camera -> world, for fp64 tensors (..., ) of radians -> (..., 3, 3)"""
    cr, sr, cp, sp = torch.cos(roll), torch.sin(roll), torch.cos(pitch), torch.sin(pitch)
    z = torch.zeros_like(cr)
    return torch.stack([torch.stack([cr, -sr, z], -1), torch.stack([cp * sr, cp * cr, -sp], -1), torch.stack([sp * sr, sp * cr, cp], -1)], -2)


def _rot_yaw(yaw):
    """Y(yaw), the turn about y that adds yaw to the longitude"""
    c, s = torch.cos(yaw), torch.sin(yaw)
    z, o = torch.zeros_like(c), torch.ones_like(c)
    return torch.stack([torch.stack([c, z, s], -1), torch.stack([z, o, z], -1), torch.stack([-s, z, c], -1)], -2)


def gravity_from_views(view_cams, roll, pitch, *, weights=None, max_dev=15.0, mode="deg"):
    """The roll and pitch of a panorama from what was said about views cut out of it: every view's up direction, carried into the panorama's frame
    and averaged robustly.  Pure torch in fp64 on the device of its inputs (CPU or GPU); no host synchronisation.

    view_cams: a dict of the per-view `roll`, `pitch`, `yaw` with which the views were cut from one panorama (`crop_panorama`'s arguments; absent
    entries count as 0).  roll, pitch: what the model (pred_roll, pred_pitch) or `fit_camera` said about each view, N values.  Angles in degrees
    unless mode="rad"; max_dev and the returned `angles` are always degrees.
    View i votes v_i = V_i R(roll_i, pitch_i)^T (0, -1, 0) with V_i = Y(yaw_i) R(view roll_i, view pitch_i): the world's up in the panorama's
    frame.  The result is the weighted mean direction (weights: N values >= 0, default 1), re-averaged once over the views within max_dev
    degrees of it, and returned as the (roll, pitch) with R(roll, pitch)^T (0, -1, 0) = that direction -- what
    `rotate_panorama(pano, roll, pitch, inverse=True)` levels the panorama with.  A view with a non-finite prediction, camera or weight does not vote;
    without a voting view the result is NaN.
    Returns a dict: roll, pitch (0-d, in `mode` units), direction (3,), votes (N, 3; NaN rows for views that do not vote), inliers (N,) bool,
    angles (N,) degrees between each vote and the result."""
    if not isinstance(view_cams, Mapping):
        raise TypeError(f"gravity_from_views: view_cams must be a dict of roll, pitch, yaw; got {type(view_cams).__name__}")
    unknown = [k for k in view_cams if k not in ("roll", "pitch", "yaw")]
    if unknown:
        raise ValueError(f"gravity_from_views: view_cams may hold roll, pitch and yaw; unknown {unknown}")
    _check_mode(mode)
    if not (float(max_dev) > 0.0):
        raise ValueError("max_dev must be > 0 degrees")
    named = [("view roll", view_cams.get("roll", 0.0)), ("view pitch", view_cams.get("pitch", 0.0)), ("view yaw", view_cams.get("yaw", 0.0)),
             ("roll", roll), ("pitch", pitch), ("weights", 1.0 if weights is None else weights)]
    ts = _param_tensors(named, "gravity_from_views: {}")
    N = _broadcast_len("gravity_from_views", ts, "view")
    dev = next((t.device for t in ts if t.device.type != "cpu"), torch.device("cpu"))
    ts = [t.to(device=dev, dtype=torch.float64).expand(N) for t in ts]
    vr, vp, vy, r, p = [torch.deg2rad(t) if mode == "deg" else t for t in ts[:5]]
    w = ts[5]
    up = torch.tensor([0.0, -1.0, 0.0], dtype=torch.float64, device=dev)
    votes = (_rot_yaw(vy) @ _rot_roll_pitch(vr, vp) @ _rot_roll_pitch(r, p).transpose(-1, -2)) @ up
    voting = torch.isfinite(votes).all(-1) & torch.isfinite(w) & (w >= 0)
    v0 = torch.where(voting[:, None], votes, torch.zeros_like(votes))
    w0 = torch.where(voting, w, torch.zeros_like(w))

    def mean_dir(wk):
        s = (wk[:, None] * v0).sum(0)
        return s / torch.linalg.vector_norm(s)   # 0 / 0 = NaN without a voting view

    def angles_to(d):
        return torch.rad2deg(torch.atan2(torch.linalg.vector_norm(torch.linalg.cross(votes, d.expand_as(votes)), dim=-1), votes @ d))

    first = mean_dir(w0)
    near = voting & (angles_to(first) <= float(max_dev))
    d = mean_dir(torch.where(near, w0, torch.zeros_like(w0)))
    d = torch.where(torch.isfinite(d).all(), d, first)   # no view within max_dev of the first mean: it stands
    ang = angles_to(d)
    # R(roll, pitch)^T (0, -1, 0) = (-cos p sin r, -cos p cos r, sin p)
    out_pitch = torch.atan2(d[2], torch.linalg.vector_norm(d[:2]))
    out_roll = torch.atan2(-d[0], -d[1])
    if mode == "deg":
        out_roll, out_pitch = torch.rad2deg(out_roll), torch.rad2deg(out_pitch)
    return {"roll": out_roll, "pitch": out_pitch, "direction": d, "votes": votes, "inliers": voting & (ang <= float(max_dev)), "angles": ang}


_YAW_MAX_CAND = 4096   # include/pf_hip.h PF_YAW_MAX_CAND
_YAW_CAM_COLS = (0, 1, 3, 4, 5, 6)   # _CAM_KEYS without the yaw: the row order of pf_yaw_moments's d_cam6


def yaw_scores(images, cams, pairs, candidates, *, stride=None, min_overlap=0.1, mode="deg", return_moments=False):
    """How well the pictures of two views of one centre agree when the second is turned by a candidate angle about the vertical against the
    first, on the GPU.  Model: include/pf_hip.h pf_yaw_moments.

    images, cams: what `compose_panorama` takes (a `yaw` entry of cams is ignored).  pairs: a sequence of (a, b) view indices, a != b.
    candidates: the turns yaw_b - yaw_a to try, in degrees (also with mode="rad", which is about the cameras' angles), a 1-d sequence or
    tensor of at most 4096 entries.  stride: every stride-th row and column of b is a sample; default max(1, min(H, W) // 48) of the
    smallest view, one stride per call (a search in steps of 1 degree does not need more samples).
    Returns (score (P, K) float64, overlap (P, K) float64) on the device; with return_moments=True also the moments (P, K, 6) float64
    (n, sum x, sum y, sum x^2, sum y^2, sum xy of the luminances x of a and y of b over the covered samples).  score is the zero-mean
    normalised cross-correlation, in [-1, 1], computed from the moments in float64; it is -inf where fewer than min_overlap x (samples of b
    that have a ray) samples are covered or a variance is not positive (see _zncc).  overlap is the covered share of those samples.
    GPU only: CPU images raise PfError."""
    from .engine import load_library

    _, n, sizes, dev, make = _sources("yaw_scores", images, ("view", "views"), "a view must be (H, W, 3) with H, W >= 1, or a tensor (B, H, W, 3)", 1, batched=True)
    if n < 2:
        raise ValueError("yaw_scores needs at least two views")
    _check_mode(mode)
    if stride is None:
        stride = max(1, min(min(hw) for hw in sizes) // 48)
    stride = operator.index(stride)
    if stride < 1:
        raise ValueError(f"stride must be at least 1; got {stride}")
    min_overlap = float(min_overlap)
    if not 0.0 <= min_overlap <= 1.0:
        raise ValueError(f"min_overlap must be in [0, 1]; got {min_overlap}")
    ts = _camera_params("cams", cams, "yaw_scores")
    Bp = _broadcast_len("yaw_scores", ts)
    if Bp not in (1, n):
        raise ValueError(f"yaw_scores: camera parameters of length {Bp} for {n} views")
    plist = [(operator.index(a), operator.index(b)) for a, b in (pairs.tolist() if torch.is_tensor(pairs) else pairs)]
    if not plist:
        raise ValueError("yaw_scores needs at least one pair")
    for a, b in plist:
        if not (0 <= a < n and 0 <= b < n) or a == b:
            raise ValueError(f"a pair is two different view indices in [0, {n}); got ({a}, {b})")
    cand = candidates if torch.is_tensor(candidates) else torch.as_tensor(np.asarray(candidates, dtype=np.float64))
    if cand.dim() != 1 or not 1 <= cand.shape[0] <= _YAW_MAX_CAND:
        raise ValueError(f"candidates must be a 1-d sequence of 1 to {_YAW_MAX_CAND} angles; got shape {tuple(cand.shape)}")
    P, K = len(plist), int(cand.shape[0])
    cam = _camera_rows(ts, (0, 1, 2), n, dev, mode)[:, list(_YAW_CAM_COLS)].contiguous()
    cand = torch.deg2rad(cand.to(device=dev, dtype=torch.float64)).to(torch.float32).contiguous()
    srcs = make()   # held until the call is on the stream: the argument list carries addresses only
    c_hw = _size_array(sizes)
    c_pairs = (ctypes.c_int32 * (2 * P))(*[i for ab in plist for i in ab])
    lib = load_library()
    need = int(lib.pf_yaw_moments_workspace_bytes(n, c_hw, P, c_pairs, K, stride))
    if need == 0:
        raise ValueError("yaw_scores: the views, pairs and stride give more samples than one call takes")
    moments = torch.empty((P, K, 6), dtype=torch.float64, device=dev)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    _launch("pf_yaw_moments", dev, _source_head(dev, srcs, c_hw) + (cam.data_ptr(), P, c_pairs, K, cand.data_ptr(), stride, moments.data_ptr(), ws.data_ptr(), need),
            lib=lib)
    # the samples of b that have a ray: disc >= 0 (include/pf_hip.h pf_reproject step 1), in float64 from the float32 rows the kernel reads
    cam64, rays = cam.to(torch.float64), torch.empty(n, dtype=torch.float64, device=dev)
    for H, W in sorted(set(sizes)):   # the views of one size together
        own = torch.as_tensor([i for i, hw in enumerate(sizes) if hw == (H, W)], device=dev)
        r = cam64[own]
        x = (torch.arange(0, W, stride, device=dev, dtype=torch.float64)[None, :] + 0.5 - ((r[:, 3] + 0.5) * W)[:, None]) / (r[:, 2] * H)[:, None]
        y = (torch.arange(0, H, stride, device=dev, dtype=torch.float64)[None, :] + 0.5 - ((r[:, 4] + 0.5) * H)[:, None]) / (r[:, 2] * H)[:, None]
        disc = 1.0 + (1.0 - r[:, 5] * r[:, 5])[:, None, None] * (x[:, None, :] ** 2 + y[:, :, None] ** 2)
        rays[own] = (disc >= 0).sum((1, 2)).to(torch.float64)
    rays = rays[torch.as_tensor([b for _, b in plist], device=dev)]
    score, overlap = _zncc(moments, rays, min_overlap)
    return (score, overlap, moments) if return_moments else (score, overlap)


def _zncc(moments, rays, min_overlap):
    """moments (P, K, 6) float64 and the samples with a ray (P,) -> (score, overlap) (P, K) float64: include/pf_hip.h pf_yaw_moments's ZNCC, -inf
    where n < min_overlap x rays or a variance is not positive (not above 2^-16 of n x its sum of squares: the sums are kept in float32 per
    tile, which cannot tell such a variance from 0; one covered sample, or a flat picture, has no score)"""
    n, sx, sy, sxx, syy, sxy = moments.unbind(-1)
    va, vb = n * sxx - sx * sx, n * syy - sy * sy
    ok = (n >= min_overlap * rays[:, None]) & (va > 2.0 ** -16 * n * sxx) & (vb > 2.0 ** -16 * n * syy)
    one = torch.ones_like(va)
    score = torch.where(ok, (n * sxy - sx * sy) / torch.sqrt(torch.where(ok, va, one) * torch.where(ok, vb, one)), torch.full_like(va, float("-inf")))
    overlap = torch.where(rays[:, None] > 0, n / torch.clamp(rays[:, None], min=1.0), torch.zeros_like(n))
    return score, overlap


def _wrap180(x):
    """degrees wrapped to [-180, 180)"""
    return (x + 180.0) % 360.0 - 180.0


def yaw_tree(delta, peak, *, anchor=0, min_score=0.8):
    """The yaws of N views from the tables of their ordered pairs, on the host (no GPU): delta[a, b] (degrees) is the measured turn
    yaw_b - yaw_a of the ordered pair (a, b) and peak[a, b] its score (the diagonal is ignored; -inf or NaN: no measurement).
    Of the two orders of a pair the one with the higher peak is kept (a tie keeps a < b) and the other order's turn is its negative.  A
    maximum spanning tree grows from `anchor` (Prim) over the pairs with a kept peak >= min_score; equal peaks go to the lower new view, then
    to the lower parent.  The anchor's yaw is 0, a child's is its parent's plus the turn, wrapped to [-180, 180).
    Returns (yaw (N,) float64 with NaN for the views the tree does not reach, parent (N,) int64 with -1 for the anchor and for those
    views, linked (N,) bool)."""
    delta, peak = np.asarray(delta, dtype=np.float64), np.asarray(peak, dtype=np.float64)
    N = delta.shape[0]
    if delta.shape != (N, N) or peak.shape != (N, N):
        raise ValueError(f"delta and peak must be square tables of one size; got {delta.shape} and {peak.shape}")
    anchor = operator.index(anchor)
    if not 0 <= anchor < N:
        raise ValueError(f"anchor must be in [0, {N}); got {anchor}")
    pk = np.where(np.isfinite(peak) & np.isfinite(delta), peak, -np.inf)
    w, turn = np.full((N, N), -np.inf), np.zeros((N, N))   # turn[u, v] = yaw_v - yaw_u of the kept order
    for a in range(N):
        for b in range(a + 1, N):
            fwd = pk[a, b] >= pk[b, a]
            w[a, b] = w[b, a] = pk[a, b] if fwd else pk[b, a]
            turn[a, b] = delta[a, b] if fwd else -delta[b, a]
            turn[b, a] = -turn[a, b]
    yaw, parent, linked = np.full(N, np.nan), np.full(N, -1, dtype=np.int64), np.zeros(N, dtype=bool)
    yaw[anchor], linked[anchor] = 0.0, True
    while True:
        best = None
        for v in range(N):
            if linked[v]:
                continue
            for u in range(N):
                if linked[u] and w[u, v] >= min_score and (best is None or w[u, v] > best[0]):
                    best = (w[u, v], v, u)
        if best is None:
            return yaw, parent, linked
        _, v, u = best
        yaw[v], parent[v], linked[v] = _wrap180(yaw[u] + turn[u, v]), u, True


def align_yaw(images, cams, *, anchor=0, step=1.0, stride=None, min_overlap=0.1, min_score=0.8, refine=True, mode="deg", return_info=False):
    """The yaw of every view of one centre, recovered from the pictures on the GPU: the one camera parameter the perspective fields do not
    carry, and what `compose_panorama` takes as `yaw`.  Model: include/pf_hip.h pf_yaw_moments.

    images, cams: what `compose_panorama` takes, N >= 2 views with their roll, pitch and intrinsics (a `yaw` entry is ignored).  Every ordered
    pair (a, b), a != b, is scored by `yaw_scores` (see there for stride and min_overlap) at the candidates -180 + k step, k < round(360 / step)
    degrees; its turn is the candidate with the highest score, with refine=True moved by the vertex of the parabola through that score and its
    two circular neighbours (not moved where a neighbour has no score).  `yaw_tree` then places the views: a maximum spanning tree from
    `anchor` over the pairs whose score reaches min_score.
    Returns yaw (N,) float64 in degrees on the device, in [-180, 180), 0 for the anchor and NaN for a view that no pair of sufficient score
    ties to the anchor's tree.  With return_info=True also a dict: `delta`, `peak`, `overlap` (N, N) float64 on the device, by ordered pair
    [a, b] (NaN, -inf, 0 on the diagonal), and `parent` (N,) int64, `linked` (N,) bool on the host.
    min_score = 0.8 lies between the scores of overlapping views of one scene (0.98 and more on the low-pass test scenes) and of views
    that do not overlap or show different scenes (0.58 and less there).  It is a default, not a guarantee: repetitive scenes can score
    high at a wrong turn, and strongly differing exposure, parallax or moving objects lower the score of a right one.
    GPU only: CPU images raise PfError."""
    step = float(step)
    if not (step > 0 and round(360.0 / step) >= 1 and round(360.0 / step) <= _YAW_MAX_CAND):
        raise ValueError(f"step must give 1 to {_YAW_MAX_CAND} candidates (360 / step); got {step}")
    min_score = float(min_score)
    n = int(images.shape[0]) if torch.is_tensor(images) and images.dim() == 4 else 1 if torch.is_tensor(images) else len(images)
    if n >= 2 and not 0 <= operator.index(anchor) < n:
        raise ValueError(f"anchor must be in [0, {n}); got {anchor}")
    K = int(round(360.0 / step))
    cand = -180.0 + step * np.arange(K, dtype=np.float64)
    pairs = [(a, b) for a in range(n) for b in range(n) if a != b]
    score, overlap = yaw_scores(images, cams, pairs, cand, stride=stride, min_overlap=min_overlap, mode=mode)
    dev = score.device
    peak, k = score.max(dim=1)
    delta = torch.as_tensor(cand, device=dev)[k]
    if refine and K >= 3:
        zm, zp = score.gather(1, ((k - 1) % K)[:, None])[:, 0], score.gather(1, ((k + 1) % K)[:, None])[:, 0]
        curv = zm - 2.0 * peak + zp
        ok = torch.isfinite(zm) & torch.isfinite(zp) & torch.isfinite(peak) & (curv < 0)
        delta = delta + step * torch.where(ok, 0.5 * (zm - zp) / torch.where(ok, curv, torch.ones_like(curv)), torch.zeros_like(curv))
    idx = torch.as_tensor(pairs, device=dev)
    tables = torch.zeros((3, n, n), dtype=torch.float64, device=dev)
    tables[0].fill_(float("nan"))
    tables[1].fill_(float("-inf"))
    tables[:, idx[:, 0], idx[:, 1]] = torch.stack([delta, peak, overlap.gather(1, k[:, None])[:, 0]])
    host = tables[:2].cpu().numpy()   # the one copy to the host
    yaw, parent, linked = yaw_tree(host[0], host[1], anchor=anchor, min_score=min_score)
    yaw = torch.as_tensor(yaw, device=dev)
    if return_info:
        return yaw, dict(delta=tables[0], peak=tables[1], overlap=tables[2], parent=parent, linked=linked)
    return yaw
