"""Time of the rotation of an equirectangular panorama (pano_rotate.hip, pf_pano_rotate) next to the obvious PyTorch composition on the same GPU:
one uint8 2048 x 4096 panorama rotated by (roll 20, pitch 35, yaw 50) degrees to the same size, without and with the perspective-field labels.
The baseline builds the sampling grid with torch ops from the same model (the output pixel's direction, A = Y(yaw) R(roll, pitch), the source
longitude and latitude), runs F.grid_sample (bilinear, border padding, align_corners=False) on a float NCHW copy of the panorama with one wrapped
column padded on either side (prepared outside the timed window), and converts to uint8 NHWC; with labels it also evaluates the latitude and the up
vector with torch ops.  Both are timed with device events around the whole call after a warm-up, alternating in one process; medians of 25 calls.
`--kernel-only N` runs N rotate_panorama calls of each kind and nothing else: the process of a separate `rocprofv3 --kernel-trace --stats` run."""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.getcwd())
from perspectivefields_amd import rotate_panorama

H, W, CALLS = 2048, 4096, 25
ROT = (20.0, 35.0, 50.0)
rng = np.random.default_rng(0)


def matrix():
    r, p, y = (torch.tensor(np.radians(v), dtype=torch.float32, device="cuda") for v in ROT)
    cr, sr, cp, sp, cy, sy, z, o = torch.cos(r), torch.sin(r), torch.cos(p), torch.sin(p), torch.cos(y), torch.sin(y), torch.zeros_like(r), torch.ones_like(r)
    R = torch.stack([cr, -sr, z, cp * sr, cp * cr, -sp, sp * sr, sp * cr, cp]).reshape(3, 3)
    Y = torch.stack([cy, z, sy, z, o, z, -sy, z, cy]).reshape(3, 3)
    return Y @ R


def torch_rotate(padded_nchw, labels):
    """the same model with torch ops: uint8 (H, W, 3), and with `labels` the up vectors (2, H, W) and the latitude (H, W) in degrees"""
    A = matrix()
    lon = ((torch.arange(W, device="cuda", dtype=torch.float32) + 0.5) / W - 0.5) * (2 * np.pi)
    lat = (0.5 - (torch.arange(H, device="cuda", dtype=torch.float32) + 0.5) / H) * np.pi
    lat, lon = torch.meshgrid(lat, lon, indexing="ij")
    sl, cl, so, co = torch.sin(lat), torch.cos(lat), torch.sin(lon), torch.cos(lon)
    D = torch.stack([cl * so, -sl, cl * co], -1)
    X = D @ A.T
    lat_s = -torch.atan2(X[..., 1], torch.hypot(X[..., 0], X[..., 2]))
    u = (torch.atan2(X[..., 0], X[..., 2]) / (2 * np.pi) + 0.5) * W - 0.5
    v = (0.5 - lat_s / np.pi) * H - 0.5
    # the padded source has W + 2 columns: column c of the panorama is column c + 1 there
    grid = torch.stack([(u + 1.5) / (W + 2) * 2 - 1, (v + 0.5) / H * 2 - 1], -1)[None]
    c = F.grid_sample(padded_nchw, grid, mode="bilinear", padding_mode="border", align_corners=False)
    img = (c[0] + 0.5).floor().clamp(0, 255).to(torch.uint8).permute(1, 2, 0).contiguous()
    if not labels:
        return img, None, None
    g = -A[1]
    a = g[0] * co - g[2] * so
    b = -(g[1] * cl + sl * (g[0] * so + g[2] * co))
    up = torch.stack([W / (2 * np.pi) * a / cl, -(H / np.pi) * b])
    return img, up / up.norm(dim=0), torch.rad2deg(lat_s)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


pano = torch.from_numpy(rng.integers(0, 256, (H, W, 3), dtype=np.uint8)).cuda()
ours = {False: lambda: rotate_panorama(pano, *ROT), True: lambda: rotate_panorama(pano, *ROT, fields=True)}
if "--kernel-only" in sys.argv:
    for _ in range(int(sys.argv[sys.argv.index("--kernel-only") + 1])):
        ours[False]()
        ours[True]()
    torch.cuda.synchronize()
    sys.exit(0)
nchw = pano.permute(2, 0, 1).float()[None]
padded = torch.cat([nchw[..., -1:], nchw, nchw[..., :1]], -1).contiguous()
for labels in (False, True):
    theirs = lambda: torch_rotate(padded, labels)
    for _ in range(3):
        ours[labels]()
        theirs()
    torch.cuda.synchronize()
    t_ours, t_torch = [], []
    for _ in range(CALLS):
        t_ours.append(timed(ours[labels]))
        t_torch.append(timed(theirs))
    a, b = ours[labels](), theirs()
    img = a[0][0] if labels else a[0]
    agree = float((img.int() - b[0].int()).abs().le(1).all(-1).float().mean())
    moved = H * W * (3 + (12 if labels else 0))
    extra = ""
    if labels:
        extra = f", largest latitude difference {float((a[2][0] - b[2]).abs().max()):.2e} deg, up vectors within 1e-3 on {float(((a[1][0] - b[1]).abs().amax(0) <= 1e-3).float().mean()):.5f}"
    print(f"uint8 {H} x {W} -> {H} x {W}, labels {labels}: rotate_panorama {np.median(t_ours):.3f} ms, torch {np.median(t_torch):.3f} ms "
          f"(x{np.median(t_torch) / np.median(t_ours):.2f}); {moved / 1e6:.1f} MB written per call (HBM write bound at 8 TB/s: {moved / 8e12 * 1e3:.4f} ms); "
          f"images within 1 LSB of the baseline on {agree:.5f} of the pixels{extra}", flush=True)
