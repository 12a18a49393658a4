"""Time of the composition of camera views into a panorama (pano_compose.hip, pf_pano_compose) next to the obvious PyTorch composition on the
same GPU: 6 uint8 views of 480 x 640 (four of 100 degrees around the horizon, one per pole) into one 1024 x 2048 panorama, feather blend.
The baseline builds every view's sampling grid with torch ops from the same model (the panorama pixel's direction, M = R^T Y(-yaw) per
view, the pinhole projection, the coverage test, the feather weight), runs F.grid_sample (bilinear, border padding, align_corners=False) on a
float NCHW copy of the views (prepared outside the timed window), sums weight x colour and weight over the views, divides and converts to
uint8 NHWC.  Both are timed with device events around the whole call after a warm-up, alternating in one process; medians of 25 calls.
`--kernel-only N` runs N compose_panorama calls and nothing else: the process of a separate `rocprofv3 --kernel-trace --stats` run."""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.getcwd())
from perspectivefields_amd import compose_panorama

N, H, W, HP, WP, CALLS = 6, 480, 640, 1024, 2048, 25
rng = np.random.default_rng(0)
dev = lambda v: torch.tensor(v, dtype=torch.float64, device="cuda")
roll = np.array([3.0, -2.0, 1.5, -4.0, 0.0, 0.0])
pitch = np.array([4.0, -3.0, 2.0, -1.0, 90.0, -90.0])
yaw = np.array([0.0, 90.0, 180.0, 270.0, 0.0, 30.0])
focal = np.full(N, 0.5 / np.tan(np.radians(50.0)))
CAMS = dict(roll=dev(roll), pitch=dev(pitch), yaw=dev(yaw), rel_focal=dev(focal))


def rotation(r, p):
    cr, sr, cp, sp, z = torch.cos(r), torch.sin(r), torch.cos(p), torch.sin(p), torch.zeros_like(r)
    return torch.stack([cr, -sr, z, cp * sr, cp * cr, -sp, sp * sr, sp * cr, cp], -1).reshape(-1, 3, 3)


def yaw_matrix(t):
    c, s, z, o = torch.cos(t), torch.sin(t), torch.zeros_like(t), torch.ones_like(t)
    return torch.stack([c, z, s, z, o, z, -s, z, c], -1).reshape(-1, 3, 3)


def torch_compose(views_nchw):
    """the same model (centred pinhole views) with torch ops: uint8 (HP, WP, 3) and the summed weight"""
    r, p, y = (torch.deg2rad(CAMS[k].float()) for k in ("roll", "pitch", "yaw"))
    M = rotation(r, p).transpose(1, 2) @ yaw_matrix(-y)
    lon = ((torch.arange(WP, device="cuda", dtype=torch.float32) + 0.5) / WP - 0.5) * (2 * np.pi)
    lat = (0.5 - (torch.arange(HP, device="cuda", dtype=torch.float32) + 0.5) / HP) * np.pi
    lat, lon = torch.meshgrid(lat, lon, indexing="ij")
    D = torch.stack([torch.cos(lat) * torch.sin(lon), -torch.sin(lat), torch.cos(lat) * torch.cos(lon)], -1)
    X = torch.einsum("nij,hwj->nhwi", M, D)
    fs = CAMS["rel_focal"].float()[:, None, None] * H
    a, b = fs * X[..., 0] / X[..., 2] + 0.5 * W, fs * X[..., 1] / X[..., 2] + 0.5 * H
    d = torch.minimum(torch.minimum(a, W - a), torch.minimum(b, H - b))
    w = torch.where((X[..., 2] > 0) & (d > 0), (d * (2.0 / min(H, W))).clamp(max=1.0), torch.zeros_like(d))
    grid = torch.stack([a / W * 2 - 1, b / H * 2 - 1], -1)
    grid = torch.where((w > 0)[..., None], grid, torch.zeros_like(grid))   # no NaN into grid_sample
    c = F.grid_sample(views_nchw, grid, mode="bilinear", padding_mode="border", align_corners=False)
    S = w.sum(0)
    out = (c * w[:, None]).sum(0) / S.clamp(min=1e-30)
    img = (out * (S > 0) + 0.5).floor().clamp(0, 255).to(torch.uint8).permute(1, 2, 0).contiguous()
    return img, S


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


views = torch.from_numpy(rng.integers(0, 256, (N, H, W, 3), dtype=np.uint8)).cuda()
ours = lambda: compose_panorama(views, CAMS, height=HP, width=WP, return_weight=True)
if "--kernel-only" in sys.argv:
    for _ in range(int(sys.argv[sys.argv.index("--kernel-only") + 1])):
        ours()
    torch.cuda.synchronize()
    sys.exit(0)
views_nchw = views.permute(0, 3, 1, 2).float().contiguous()
theirs = lambda: torch_compose(views_nchw)
for _ in range(3):
    ours()
    theirs()
torch.cuda.synchronize()
t_ours, t_torch = [], []
for _ in range(CALLS):
    t_ours.append(timed(ours))
    t_torch.append(timed(theirs))
(a, sa), (b, sb) = ours(), theirs()
covered = (sa[0] > 1e-3) & (sb > 1e-3)
agree = float((a[0].int() - b.int()).abs().le(1).all(-1)[covered].float().mean())
written = HP * WP * (3 + 4)
print(f"{N} views {H} x {W} -> {HP} x {WP}, feather: compose_panorama {np.median(t_ours):.3f} ms, torch {np.median(t_torch):.3f} ms "
      f"(x{np.median(t_torch) / np.median(t_ours):.2f}); {written / 1e6:.1f} MB written per call (HBM write bound at 8 TB/s: {written / 8e12 * 1e3:.4f} ms); "
      f"covered share {float((sa[0] > 0).float().mean()):.3f}, largest weight difference {float((sa[0] - sb).abs().max()):.2e}, "
      f"images within 1 LSB of the baseline on {agree:.4f} of the covered pixels", flush=True)
