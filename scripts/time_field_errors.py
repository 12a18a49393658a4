"""Time of field_errors (field_err.hip, pf_field_errors) next to the obvious PyTorch composition on the same GPU: B = 32 images of
640 x 640, noisy synthetic predictions against exact labels with 5 % of the label pixels masked (NaN).  Variants: statistics only,
with the per-pixel maps, with the running histogram (FieldErrorAccumulator.update).  The baseline computes the same numbers with torch
ops on the batched tensors: atan2 of cross and dot, |lat difference|, the validity mask, nanmean / max / share below the threshold and
nanmedian-style medians per image (torch.nanmedian returns the LOWER middle element; the upper one is taken from the negated map, so the
baseline pays two selections per metric as the definition needs).  Both are timed with device events after a warm-up, alternating in
one process; medians of 25 calls.  Prints the bytes the six input planes hold, for the kernel times of a separate
`rocprofv3 --kernel-trace --stats` run."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.getcwd())
from perspectivefields_amd import FieldErrorAccumulator, field_errors, fields_from_params

B, H, W, CALLS = 32, 640, 640, 25
rng = np.random.default_rng(0)
g = torch.Generator(device="cuda").manual_seed(0)
up_gt, lat_gt = [], []
for i in range(B):
    u, l = fields_from_params(float(rng.uniform(-20, 20)), float(rng.uniform(-45, 45)), float(0.5 / np.tan(np.radians(rng.uniform(40, 100)) / 2)), 0.0, 0.0, H, W)
    up_gt.append(u)
    lat_gt.append(l)
up_gt, lat_gt = torch.stack(up_gt), torch.stack(lat_gt)
ang = torch.deg2rad(2.0 * torch.randn((B, H, W), device="cuda", generator=g))
c, s = torch.cos(ang), torch.sin(ang)
up_pred = torch.stack([c * up_gt[:, 0] - s * up_gt[:, 1], s * up_gt[:, 0] + c * up_gt[:, 1]], 1).contiguous()
lat_pred = lat_gt + 2.0 * torch.randn((B, H, W), device="cuda", generator=g)
lat_gt = torch.where(torch.rand((B, H, W), device="cuda", generator=g) < 0.05, torch.full_like(lat_gt, float("nan")), lat_gt)
THR = 5.0


def torch_errors(maps):
    cross = (up_pred[:, 0] * up_gt[:, 1] - up_pred[:, 1] * up_gt[:, 0]).abs()
    dot = (up_pred * up_gt).sum(1)
    valid = torch.isfinite(up_pred).all(1) & torch.isfinite(up_gt).all(1) & torch.isfinite(lat_pred) & torch.isfinite(lat_gt)
    valid &= ((up_pred * up_pred).sum(1) >= 1e-12) & ((up_gt * up_gt).sum(1) >= 1e-12)
    nan = torch.full((), float("nan"), device="cuda")
    e_up = torch.where(valid, torch.rad2deg(torch.atan2(cross, dot)), nan)
    e_lat = torch.where(valid, (lat_pred - lat_gt).abs(), nan)
    n = valid.flatten(1).sum(1)
    out = []
    for e in (e_up, e_lat):
        f = e.flatten(1)
        d = torch.nan_to_num(f, nan=0.0).double()
        lower = torch.nanmedian(f, 1).values                       # element (n - 1) // 2
        upper = -torch.nanmedian(-f, 1).values                     # element n // 2
        out += [d.sum(1) / n, 0.5 * (lower.double() + upper.double()), torch.sqrt((d * d).sum(1) / n), torch.nan_to_num(f, nan=0.0).max(1).values,
                (f < THR).sum(1) / n]
    return (torch.stack(out, 1), n, e_up, e_lat) if maps else (torch.stack(out, 1), n)


acc = FieldErrorAccumulator("cuda", threshold_deg=THR)
VARIANTS = {
    "statistics": (lambda: field_errors(up_pred, lat_pred, up_gt, lat_gt, threshold_deg=THR), lambda: torch_errors(False)),
    "with maps": (lambda: field_errors(up_pred, lat_pred, up_gt, lat_gt, threshold_deg=THR, return_maps=True), lambda: torch_errors(True)),
    "with histogram": (lambda: acc.update(up_pred, lat_pred, up_gt, lat_gt), None),
}


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


ours = field_errors(up_pred, lat_pred, up_gt, lat_gt, threshold_deg=THR)
base, n_base = torch_errors(False)
ours_m = torch.stack([torch.stack([d[k] for k in list(d)[:10]]) for d in ours])
print(f"agreement with the baseline: max |difference| over the 10 statistics of {B} images {float((ours_m - base).abs().max()):.3e} deg; "
      f"medians: {float((ours_m[:, [1, 6]] - base[:, [1, 6]]).abs().max()):.3e}; valid pixels equal: {bool((torch.stack([d['valid_pixels'] for d in ours]) == n_base).all())}", flush=True)
in_bytes = B * H * W * 24
for name, (fn, ref) in VARIANTS.items():
    for _ in range(3):
        fn()
        if ref:
            ref()
    torch.cuda.synchronize()
    t_ours, t_ref = [], []
    for _ in range(CALLS):
        t_ours.append(timed(fn))
        if ref:
            t_ref.append(timed(ref))
    line = f"{name}: field_errors {np.median(t_ours):.3f} ms (min {np.min(t_ours):.3f})"
    if ref:
        line += f", torch {np.median(t_ref):.3f} ms (x{np.median(t_ref) / np.median(t_ours):.2f})"
    print(line + f"; inputs {in_bytes / 1e6:.1f} MB = {in_bytes / 6.3e12 * 1e3:.4f} ms at the 6.3 TB/s of a plain copy "
          f"(x{np.median(t_ours) / (in_bytes / 6.3e12 * 1e3):.1f} of that floor)", flush=True)
