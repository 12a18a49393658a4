"""Time of the placement search (field_xform.hip, pf_place_search, placement_search) next to what a caller can compose without it on the same GPU: a
640 x 640 background, a 160 x 120 object with an elliptical mask cut from another noisy realisation of the same camera's fields, 5 scales x 3
rotations, at stride 4 and at stride 1.
The baseline is the composition the library offered before: torch `grid_sample` (bilinear, zeros outside) on (up x valid, lat x valid, valid) with a
division by the resampled validity, a threshold of 1/2 on it, re-normalisation and rotation of the vectors -- the same model as pf_fields_transform
up to fp32 rounding -- then placement_scores per variant and torch minima over the variants, the winner read at the end as placement_search's is.
Both are timed with device events around the whole call after a warm-up, alternating in one process; medians of 25 calls.  The two must pick the
same variant and offset.
`--kernel-only N` runs N placement_search calls at stride 4 and N at stride 1 and nothing else: the process of a separate
`rocprofv3 --kernel-trace --stats` run."""
import ctypes
import math
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.getcwd())
from perspectivefields_amd import fields_from_params, placement_scores, placement_search
from perspectivefields_amd.engine import load_library

H = W = 640
h, w, AT, CALLS = 160, 120, (212, 344), 25
SCALES, ROTATIONS = (0.5, 0.75, 1.0, 1.5, 2.0), (-10.0, 0.0, 10.0)


def noisy_fields(seed):
    """the fields of roll 8, pitch 20, rel_focal 0.87 with 2 degrees of Gaussian noise on the up angle and on the latitude"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    up, lat = fields_from_params(8.0, 20.0, 0.87, height=H, width=W)
    ang = torch.atan2(up[1], up[0]) + np.radians(2.0) * torch.randn((H, W), device="cuda", generator=g)
    return torch.stack([torch.cos(ang), torch.sin(ang)]), lat + 2.0 * torch.randn((H, W), device="cuda", generator=g)


def out_size(s, r):
    hw = (ctypes.c_int32 * 2)()
    assert load_library().pf_fields_transform_size(h, w, s, r, hw) == 0
    return hw[0], hw[1]


def torch_transform(up, lat, valid, s, r):
    """the model of pf_fields_transform with grid_sample: (up', lat') with NaN where less than half of the weight is valid"""
    ho, wo = out_size(s, r)
    c, sn = math.cos(math.radians(r)), math.sin(math.radians(r))
    dy, dx = torch.meshgrid(torch.arange(ho, device="cuda") + 0.5 - ho / 2, torch.arange(wo, device="cuda") + 0.5 - wo / 2, indexing="ij")
    x, y = w / 2 + (c * dx + sn * dy) / s, h / 2 + (c * dy - sn * dx) / s      # pixel-edge coordinates
    grid = torch.stack([x / w * 2 - 1, y / h * 2 - 1], -1)[None].float()        # align_corners=False
    v = valid.float()
    src = torch.stack([torch.where(valid, up[0], 0.0), torch.where(valid, up[1], 0.0), torch.where(valid, lat, 0.0), v])[None]
    mx, my, ml, wv = F.grid_sample(src, grid, mode="bilinear", padding_mode="zeros", align_corners=False)[0]
    ok = wv >= 0.5
    rx, ry = c * mx - sn * my, sn * mx + c * my
    n = torch.sqrt(rx * rx + ry * ry)
    nan = torch.full_like(ml, float("nan"))
    return torch.stack([torch.where(ok, rx / n, nan), torch.where(ok, ry / n, nan)]), torch.where(ok, ml / wv, nan)


def torch_search(up_bg, lat_bg, up_obj, lat_obj, mask, stride):
    valid = mask & torch.isfinite(lat_obj) & ((up_obj * up_obj).sum(0) >= 1e-12)
    pfd, off = [], []
    for s in SCALES:
        for r in ROTATIONS:
            tu, tl = torch_transform(up_obj, lat_obj, valid, s, r)
            if tl.shape[0] > H or tl.shape[1] > W:
                pfd.append(torch.tensor(float("inf"), dtype=torch.float64, device="cuda"))
                off.append(torch.full((2,), -1, dtype=torch.int64, device="cuda"))
                continue
            d = placement_scores(up_bg, lat_bg, tu, tl, stride=stride)
            pfd.append(d["best_pfd_deg"])
            off.append(d["best_offset"])
    pfd, off = torch.stack(pfd), torch.stack(off)
    v = torch.where(pfd == pfd.min(), torch.arange(len(pfd), device="cuda"), len(pfd)).min()
    return v, off[v], pfd[v]


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


up_bg, lat_bg = noisy_fields(0)
up_o, lat_o = noisy_fields(1)
up_obj = up_o[:, AT[0]:AT[0] + h, AT[1]:AT[1] + w].contiguous()
lat_obj = lat_o[AT[0]:AT[0] + h, AT[1]:AT[1] + w].contiguous()
rr, cc = torch.meshgrid(torch.arange(h, device="cuda"), torch.arange(w, device="cuda"), indexing="ij")
mask = ((rr - (h - 1) / 2) / (h / 2)) ** 2 + ((cc - (w - 1) / 2) / (w / 2)) ** 2 <= 1.0
search = lambda stride: placement_search(up_bg, lat_bg, up_obj, lat_obj, scales=SCALES, rotations=ROTATIONS, mask=mask, stride=stride)
if "--kernel-only" in sys.argv:
    for stride in (4, 1):
        for _ in range(int(sys.argv[sys.argv.index("--kernel-only") + 1])):
            search(stride)
    torch.cuda.synchronize()
    sys.exit(0)
for stride in (4, 1):
    ours = lambda: search(stride)
    theirs = lambda: torch_search(up_bg, lat_bg, up_obj, lat_obj, mask, stride)
    for _ in range(2):
        ours()
        theirs()
    torch.cuda.synchronize()
    t_ours, t_torch = [], []
    for _ in range(CALLS):
        t_ours.append(timed(ours))
        t_torch.append(timed(theirs))
    got, (v, at, pfd) = ours(), theirs()
    assert int(got["best_variant"]) == int(v) and got["best_offset"].tolist() == at.tolist(), (got["best_variant"], got["best_offset"], v, at)
    print(f"background {H} x {W}, object {h} x {w} ({int(mask.sum())} pixels in the ellipse), {len(SCALES)} scales x {len(ROTATIONS)} rotations, stride {stride}: "
          f"placement_search {np.median(t_ours):.3f} ms, grid_sample + placement_scores per variant + torch minima {np.median(t_torch):.3f} ms "
          f"(x{np.median(t_torch) / np.median(t_ours):.1f}); both pick variant {int(v)} (scale {float(got['best_scale'])}, rotation "
          f"{float(got['best_rotation_deg'])}) at {at.tolist()}, best PFD {float(got['best_pfd_deg']):.4f} deg against {float(pfd):.4f}; sizes "
          f"{got['variant_size'].tolist()}", flush=True)
