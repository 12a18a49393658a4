"""Time of the placement scores (place_score.hip, pf_place_scores, placement_scores) next to the obvious PyTorch composition on the same GPU: a
640 x 640 background, a 160 x 120 object with an elliptical mask cut from another noisy realisation of the same camera's fields at (212, 344), at
stride 4 (121 x 131 placements) and at stride 1 (481 x 521).
The baseline computes the same model with torch ops: per object row the background rows it can fall on as a strided slice, `unfold` along the
columns to (P, Q, w) windows, atan2(|cross|, dot) and the latitude difference in float32, the masks, sums over the window in float64; then the means,
the threshold and the first minimum.  160 iterations of about 25 small launches; a single `unfold` of both axes would need P Q h w floats (19 GB per
plane at stride 1).  Both are timed with device events around the whole call after a warm-up, alternating in one process; medians of 25 calls.  The
two must pick the same best offset.
`--kernel-only N` runs N placement_scores calls at stride 4 and N at stride 1 and nothing else: the process of a separate
`rocprofv3 --kernel-trace --stats` run."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.getcwd())
from perspectivefields_amd import fields_from_params, placement_scores

H = W = 640
h, w, AT, CALLS = 160, 120, (212, 344), 25


def noisy_fields(seed):
    """the fields of roll 8, pitch 20, rel_focal 0.87 with 2 degrees of Gaussian noise on the up angle and on the latitude"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    up, lat = fields_from_params(8.0, 20.0, 0.87, height=H, width=W)
    ang = torch.atan2(up[1], up[0]) + np.radians(2.0) * torch.randn((H, W), device="cuda", generator=g)
    return torch.stack([torch.cos(ang), torch.sin(ang)]), lat + 2.0 * torch.randn((H, W), device="cuda", generator=g)


def torch_scores(up_bg, lat_bg, up_obj, lat_obj, mask, stride, min_valid=0.5):
    P, Q = (H - h) // stride + 1, (W - w) // stride + 1
    ok_obj = mask & torch.isfinite(lat_obj) & ((up_obj * up_obj).sum(0) >= 1e-12)
    ok_bg = torch.isfinite(lat_bg) & ((up_bg * up_bg).sum(0) >= 1e-12)
    S_up = torch.zeros((P, Q), dtype=torch.float64, device="cuda")
    S_lat, n = torch.zeros_like(S_up), torch.zeros_like(S_up)
    for r in range(h):
        rows = slice(r, r + (P - 1) * stride + 1, stride)
        win = lambda plane: plane[rows].unfold(1, w, stride)                       # (P, Q, w)
        bx, by, bl, m = win(up_bg[0]), win(up_bg[1]), win(lat_bg), win(ok_bg) & ok_obj[r]
        e_up = torch.rad2deg(torch.atan2((bx * up_obj[1, r] - by * up_obj[0, r]).abs(), bx * up_obj[0, r] + by * up_obj[1, r]))
        e_lat = (bl - lat_obj[r]).abs()
        zero = torch.zeros((), device="cuda")
        S_up += torch.where(m, e_up, zero).sum(-1, dtype=torch.float64)
        S_lat += torch.where(m, e_lat, zero).sum(-1, dtype=torch.float64)
        n += m.sum(-1, dtype=torch.float64)
    pfd = torch.where((n >= min_valid * ok_obj.sum()) & (n > 0), (S_up + S_lat) / n, torch.full_like(n, float("inf")))
    best = pfd.min()
    flat = torch.where(pfd.reshape(-1) == best, torch.arange(P * Q, device="cuda"), P * Q).min()
    return pfd, torch.stack([torch.div(flat, Q, rounding_mode="floor"), flat % Q]) * stride


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
if "--kernel-only" in sys.argv:
    for stride in (4, 1):
        for _ in range(int(sys.argv[sys.argv.index("--kernel-only") + 1])):
            placement_scores(up_bg, lat_bg, up_obj, lat_obj, mask=mask, stride=stride)
    torch.cuda.synchronize()
    sys.exit(0)
for stride in (4, 1):
    ours = lambda: placement_scores(up_bg, lat_bg, up_obj, lat_obj, mask=mask, stride=stride)
    theirs = lambda: torch_scores(up_bg, lat_bg, up_obj, lat_obj, mask, stride)
    for _ in range(2):
        ours()
        theirs()
    torch.cuda.synchronize()
    t_ours, t_torch = [], []
    for _ in range(CALLS):
        t_ours.append(timed(ours))
        t_torch.append(timed(theirs))
    got, (pfd, at) = ours(), theirs()
    assert got["best_offset"].tolist() == at.tolist(), (got["best_offset"], at)   # within the noise of the cut at AT, not on it: the fields vary slowly
    fin = torch.isfinite(pfd)
    assert (torch.isfinite(got["pfd_deg"]) == fin).all()
    pairs = float(got["valid_pixels"].sum())
    print(f"background {H} x {W}, object {h} x {w} ({int(mask.sum())} pixels in the ellipse), stride {stride}: {pfd.shape[0]} x {pfd.shape[1]} placements, "
          f"{pairs / 1e6:.1f} M pixel pairs: placement_scores {np.median(t_ours):.3f} ms, torch {np.median(t_torch):.3f} ms "
          f"(x{np.median(t_torch) / np.median(t_ours):.1f}); both pick {at.tolist()}, best PFD {float(got['best_pfd_deg']):.4f} deg, largest PFD difference "
          f"{float((got['pfd_deg'] - pfd)[fin].abs().max()):.2e} deg", flush=True)
