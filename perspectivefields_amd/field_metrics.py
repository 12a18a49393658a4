"""Predicted perspective fields against ground truth on the GPU (pf_field_errors): per-image errors and their dataset-level accumulator."""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from .engine import PfError


# columns of the pf_field_errors output row (include/pf_hip.h PF_FERR_COL_*), bins and running totals of its histogram (PF_FERR_BINS, PF_FERR_SUM_*)
_FERR_COLS = ("up_mean_deg", "up_median_deg", "up_rmse_deg", "up_max_deg", "up_frac_below",
              "lat_mean_deg", "lat_median_deg", "lat_rmse_deg", "lat_max_deg", "lat_frac_below", "valid_pixels")
_FERR_BINS, _FERR_BINS_PER_DEG = 11520, 64
_FERR_SUMS = ("n", "sum", "sum_sq", "max", "below")


def _field_list(what, up, lat, fn="field_errors"):
    """one (2,H,W) / (H,W) pair, a batched (B,2,H,W) / (B,H,W) pair or lists of pairs -> (is a single pair, [up], [lat])"""
    if torch.is_tensor(up) != torch.is_tensor(lat):
        raise TypeError(f"{fn}: {what} up field and latitude must both be tensors or both be lists")
    if torch.is_tensor(up):
        if up.dim() == 4 and lat.dim() == 3:
            if up.shape[0] != lat.shape[0]:
                raise ValueError(f"{fn}: {what} up {tuple(up.shape)} and latitude {tuple(lat.shape)} differ in batch size")
            return False, list(up.unbind(0)), list(lat.unbind(0))
        return True, [up], [lat]
    if not isinstance(up, (list, tuple)) or not isinstance(lat, (list, tuple)):
        raise TypeError(f"{fn} takes torch tensors or lists of them")
    ups, lats = list(up), list(lat)
    if len(ups) != len(lats):
        raise ValueError(f"{fn}: {len(ups)} {what} up fields for {len(lats)} latitude maps")
    return False, ups, lats


def _field_errors(up_pred, lat_pred, up_gt, lat_gt, threshold_deg, return_maps, hist=None, sums=None):
    from .engine import _check, _stream_ptr, load_library

    s_p, ups_p, lats_p = _field_list("predicted", up_pred, lat_pred)
    s_g, ups_g, lats_g = _field_list("ground-truth", up_gt, lat_gt)
    if len(ups_p) != len(ups_g) or not ups_p:
        raise ValueError(f"field_errors needs as many ground-truth fields as predictions, at least one (got {len(ups_p)} and {len(ups_g)})")
    threshold_deg = float(threshold_deg)
    if not (threshold_deg > 0.0 and np.isfinite(threshold_deg)):
        raise ValueError("threshold_deg must be finite and > 0")
    every = ups_p + lats_p + ups_g + lats_g
    if not all(torch.is_tensor(t) for t in every):
        raise TypeError("field_errors takes torch tensors")
    for u, l, g, m in zip(ups_p, lats_p, ups_g, lats_g):
        if u.dim() != 3 or u.shape[0] != 2 or min(u.shape[1:]) < 1 or tuple(l.shape) != tuple(u.shape[1:]):
            raise ValueError(f"up must be (2, H, W) and lat (H, W) with H, W >= 1; got {tuple(u.shape)} and {tuple(l.shape)}")
        if tuple(g.shape) != tuple(u.shape) or tuple(m.shape) != tuple(l.shape):
            raise ValueError(f"ground truth {tuple(g.shape)} / {tuple(m.shape)} does not match the prediction {tuple(u.shape)} / {tuple(l.shape)}")
    if not all(t.is_cuda for t in every):
        raise PfError("field_errors runs on the GPU only (no CPU path)")
    dev = every[0].device
    if any(t.device != dev for t in every):
        raise ValueError("field_errors: all fields must be on one device")
    ups_p, lats_p, ups_g, lats_g = ([t.to(torch.float32).contiguous() for t in ts] for ts in (ups_p, lats_p, ups_g, lats_g))
    B = len(ups_p)
    ptrs = lambda ts: (ctypes.c_void_p * B)(*[t.data_ptr() for t in ts])
    hw = (ctypes.c_int32 * (2 * B))(*[s for u in ups_p for s in (int(u.shape[1]), int(u.shape[2]))])
    lib = load_library()
    ws_n = int(lib.pf_field_errors_workspace_bytes(B, hw))
    if ws_n == 0:
        raise PfError(f"field_errors: unsupported image sizes {[tuple(u.shape[1:]) for u in ups_p]}")
    ws = torch.empty(ws_n, dtype=torch.uint8, device=dev)
    out = torch.empty((B, len(_FERR_COLS)), dtype=torch.float64, device=dev)
    maps_up = [torch.empty_like(l) for l in lats_p] if return_maps else None
    maps_lat = [torch.empty_like(l) for l in lats_p] if return_maps else None
    with torch.cuda.device(dev):
        _check(lib.pf_field_errors(dev.index, B, hw, ptrs(ups_p), ptrs(lats_p), ptrs(ups_g), ptrs(lats_g), threshold_deg, out.data_ptr(),
                                   ptrs(maps_up) if return_maps else None, ptrs(maps_lat) if return_maps else None,
                                   hist.data_ptr() if hist is not None else None, sums.data_ptr() if sums is not None else None,
                                   ws.data_ptr(), ws_n, _stream_ptr()), None, "pf_field_errors")
    valid = out[:, len(_FERR_COLS) - 1].to(torch.int64)
    res = []
    valid = valid.unbind(0)
    for i, row in enumerate(out.unbind(0)):
        d = dict(zip(_FERR_COLS[:-1], row.unbind(0)))
        d["valid_pixels"] = valid[i]
        if return_maps:
            d["up_error_deg"], d["lat_error_deg"] = maps_up[i], maps_lat[i]
        res.append(d)
    return res[0] if (s_p and s_g) else res


def field_errors(up_pred, lat_pred, up_gt, lat_gt, *, threshold_deg=5.0, return_maps=False):
    """Predicted perspective fields against ground truth on the GPU: the per-pixel numbers of the paper's tables.  Definitions:
    include/pf_hip.h pf_field_errors.  Per pixel e_up = atan2(|cross|, dot) of the two up vectors and
    e_lat = |lat_pred - lat_gt|, both in degrees; a pixel with a non-finite value in any of its six inputs, or an up vector shorter
    than 1e-6, enters no statistic (crop_panorama's NaN labels mask themselves; mask a pixel by writing NaN into its label).

    up_* (2,H,W) and lat_* (H,W) degrees (the layout of `pred_gravity_original` / `pred_latitude_original` and of crop_panorama's
    labels): one set of device tensors, batched (B,2,H,W) / (B,H,W) tensors, or lists (sizes may differ; one launch sequence per
    32 images).  Returns one dict per image (a single dict for a single set) of 0-d float64 device tensors (no host
    synchronisation): up_mean_deg, up_median_deg, up_rmse_deg, up_max_deg, up_frac_below (share of valid pixels with
    e < threshold_deg, strict), lat_* likewise, valid_pixels (int64); with return_maps also up_error_deg, lat_error_deg (H,W)
    fp32, NaN where invalid.  The median is numpy's, exact: an element (or the fp64 mean of the two middle elements) of the fp32
    error map.  No valid pixel: NaN statistics and valid_pixels = 0.  Deterministic; an image's numbers do not depend on the batch
    it is in.  GPU only: CPU tensors raise PfError."""
    return _field_errors(up_pred, lat_pred, up_gt, lat_gt, threshold_deg, return_maps)


class FieldErrorAccumulator:
    """Dataset-level statistics of the field errors: a histogram of 1/64 degree bins over [0, 180] per metric (errors beyond land in
    the last bin) plus exact running totals, kept on `device`.  The state is additive, so it merges across batches (update /
    add_errors), accumulators (merge) and ranks (all_reduce).  summary() gives mean, rmse, max and frac_below exactly (fp64 sums,
    integer counts) and the MEDIAN TO WITHIN ONE BIN (1/64 degree): the centres of the bins that hold the two middle ranks."""

    def __init__(self, device, threshold_deg=5.0):
        self.device = torch.device(device)
        self.threshold_deg = float(threshold_deg)
        if not (self.threshold_deg > 0.0 and np.isfinite(self.threshold_deg)):
            raise ValueError("threshold_deg must be finite and > 0")
        self.hist = torch.zeros((2, _FERR_BINS), dtype=torch.int64, device=self.device)      # (up, lat) x bins
        self.sums = torch.zeros((2, len(_FERR_SUMS)), dtype=torch.float64, device=self.device)  # (up, lat) x (n, sum, sum_sq, max, below)

    def update(self, up_pred, lat_pred, up_gt, lat_gt, return_maps=False):
        """field_errors of one batch on the GPU, added to the state by the same call; returns its per-image dicts."""
        if self.device.type != "cuda":
            raise PfError("FieldErrorAccumulator.update runs on the GPU only; add_errors takes ready-made error maps on any device")
        return _field_errors(up_pred, lat_pred, up_gt, lat_gt, self.threshold_deg, return_maps, self.hist, self.sums)

    def add_errors(self, err_up, err_lat):
        """Adds ready-made error maps (tensors or lists of tensors, degrees, NaN = invalid, e.g. the maps field_errors returned) with
        torch ops on the accumulator's device: bookkeeping, the same bins as the kernel (min(int(e * 64), 11519) in fp32)."""
        for m, e in enumerate((err_up, err_lat)):
            for t in ([e] if torch.is_tensor(e) else list(e)):
                v = t.to(device=self.device, dtype=torch.float32).reshape(-1)
                v = v[~torch.isnan(v)]
                if v.numel() == 0:
                    continue
                bins = (v * float(_FERR_BINS_PER_DEG)).clamp(max=float(_FERR_BINS - 1)).to(torch.int64)
                self.hist[m] += torch.bincount(bins, minlength=_FERR_BINS)
                d = v.to(torch.float64)
                self.sums[m, 0] += v.numel()
                self.sums[m, 1] += d.sum()
                self.sums[m, 2] += (d * d).sum()
                self.sums[m, 3] = torch.maximum(self.sums[m, 3], d.max())
                self.sums[m, 4] += (v < self.threshold_deg).sum()
        return self

    def merge(self, other):
        if other.threshold_deg != self.threshold_deg:
            raise ValueError("merge needs accumulators of one threshold_deg")
        o_sums = other.sums.to(self.device)
        self.hist += other.hist.to(self.device)
        mx = torch.maximum(self.sums[:, 3], o_sums[:, 3])
        self.sums += o_sums
        self.sums[:, 3] = mx
        return self

    def all_reduce(self, group=None):
        """Combines the state over a torch.distributed group (sums; a max for the maxima), so every rank holds the statistics of the
        union -- composes with ShardedPerspectiveFields.  A no-op without an initialised process group."""
        import torch.distributed as dist

        if not (dist.is_available() and dist.is_initialized()):
            return self
        mx = self.sums[:, 3].clone()
        dist.all_reduce(self.hist, op=dist.ReduceOp.SUM, group=group)
        dist.all_reduce(self.sums, op=dist.ReduceOp.SUM, group=group)
        dist.all_reduce(mx, op=dist.ReduceOp.MAX, group=group)
        self.sums[:, 3] = mx
        return self

    def summary(self):
        """{up_mean_deg, up_median_deg, up_rmse_deg, up_max_deg, up_frac_below, lat_*..., valid_pixels} as Python numbers (reads the
        state back: synchronises).  The median is accurate to one bin, 1/64 degree; everything else is exact.  No pixel: NaN."""
        hist, sums = self.hist.cpu().numpy(), self.sums.cpu().numpy()
        out = {}
        for m, name in enumerate(("up", "lat")):
            n, s, s2, mx, below = (float(x) for x in sums[m])
            if n == 0:
                vals = [float("nan")] * 5
            else:
                cum = np.cumsum(hist[m])
                mid = [int(np.searchsorted(cum, r, side="right")) for r in ((int(n) - 1) // 2, int(n) // 2)]
                med = 0.5 * sum((b + 0.5) / _FERR_BINS_PER_DEG for b in mid)
                vals = [s / n, med, float(np.sqrt(s2 / n)), mx, below / n]
            for k, v in zip(_FERR_COLS[5 * m:5 * m + 5], vals):
                out[k] = v
        out["valid_pixels"] = int(sums[0, 0])
        return out
