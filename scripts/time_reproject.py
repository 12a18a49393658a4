"""Time of the re-projection between cameras (reproject.hip, pf_reproject) next to the obvious PyTorch composition on the same GPU:
B = 32 uint8 sources of 480 x 640 to 480 x 640 outputs; run 1 a pinhole roll-rectification (destination roll 0, same pitch), run 2 a
Unified Spherical Model view of xi = 0.8 to a pinhole view.  The baseline builds the sampling grid with torch ops from the same model
(destination ray, M = R_s^T R_d per output, USM projection, the inside test), runs F.grid_sample (bilinear, border padding,
align_corners=False) on a float NCHW copy of the sources (prepared outside the timed window), masks the invalid pixels and converts to
uint8 NHWC.  Both are timed with device events around the whole call after a warm-up, alternating in one process; medians of 25 calls.
Prints the bytes each call writes, for the kernel time of a separate `rocprofv3 --kernel-trace --stats` run."""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.getcwd())
from perspectivefields_amd import reproject_image

B, H, W, CALLS = 32, 480, 640, 25
rng = np.random.default_rng(0)
roll, pitch = rng.uniform(-20, 20, B), rng.uniform(-30, 30, B)
focal = 0.5 / np.tan(np.radians(rng.uniform(50, 90, B)) / 2)
dev = lambda v: torch.tensor(v, dtype=torch.float64, device="cuda")
RUNS = {
    "pinhole roll-rectification": (dict(roll=dev(roll), pitch=dev(pitch), rel_focal=dev(focal)), dict(roll=0.0, pitch=dev(pitch), rel_focal=dev(focal))),
    "USM xi = 0.8 -> pinhole": (dict(roll=dev(roll), pitch=dev(pitch), rel_focal=dev(focal), xi=0.8), dict(roll=dev(roll), pitch=dev(pitch), rel_focal=dev(focal) * 0.6)),
}


def rotation(r, p):
    cr, sr, cp, sp, z = torch.cos(r), torch.sin(r), torch.cos(p), torch.sin(p), torch.zeros_like(r)
    return torch.stack([cr, -sr, z, cp * sr, cp * cr, -sp, sp * sr, sp * cr, cp], -1).reshape(-1, 3, 3)


def torch_reproject(src_nchw, s, d):
    """the same model (no yaw, centred cameras) with torch ops; uint8 NHWC and the mask"""
    g = lambda c, k, default=0.0: (c[k] if torch.is_tensor(c.get(k)) else torch.full((B,), float(c.get(k, default)), device="cuda")).float()
    M = rotation(torch.deg2rad(g(s, "roll")), torch.deg2rad(g(s, "pitch"))).transpose(1, 2) @ rotation(torch.deg2rad(g(d, "roll")), torch.deg2rad(g(d, "pitch")))
    fd, fs, xs = g(d, "rel_focal")[:, None, None] * H, g(s, "rel_focal")[:, None, None] * H, g(s, "xi")[:, None, None]
    x = ((torch.arange(W, device="cuda", dtype=torch.float32) + 0.5 - 0.5 * W)[None, None, :] / fd).expand(B, H, W)
    y = ((torch.arange(H, device="cuda", dtype=torch.float32) + 0.5 - 0.5 * H)[None, :, None] / fd).expand(B, H, W)
    X = torch.stack([x, y, torch.ones_like(x)], -1)
    X = X / X.norm(dim=-1, keepdim=True)          # the pinhole destination's unit ray
    Xs = torch.einsum("bij,bhwj->bhwi", M, X)
    D = Xs[..., 2] + xs * Xs.norm(dim=-1)
    a, b = fs * Xs[..., 0] / D + 0.5 * W, fs * Xs[..., 1] / D + 0.5 * H
    valid = (Xs[..., 2] > -xs) & (a >= 0) & (a <= W) & (b >= 0) & (b <= H)
    grid = torch.stack([a / W * 2 - 1, b / H * 2 - 1], -1)
    out = F.grid_sample(src_nchw, grid, mode="bilinear", padding_mode="border", align_corners=False)
    img = (out * valid[:, None] + 0.5).floor().clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()
    return img, valid


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


src = torch.from_numpy(rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)).cuda()
src_nchw = src.permute(0, 3, 1, 2).float().contiguous()
for name, (s, d) in RUNS.items():
    ours = lambda: reproject_image(src, s, d, return_valid=True)
    theirs = lambda: torch_reproject(src_nchw, s, d)
    for _ in range(3):
        ours()
        theirs()
    torch.cuda.synchronize()
    t_ours, t_torch = [], []
    for _ in range(CALLS):
        t_ours.append(timed(ours))
        t_torch.append(timed(theirs))
    (a, va), (b, vb) = ours(), theirs()
    both = va & vb
    agree = float((a.int() - b.int()).abs().le(1).all(-1)[both].float().mean())
    written = B * H * W * 4
    print(f"{name}: reproject_image {np.median(t_ours):.3f} ms, torch {np.median(t_torch):.3f} ms (x{np.median(t_torch) / np.median(t_ours):.2f}); "
          f"{written / 1e6:.1f} MB written per call (HBM write bound at 8 TB/s: {written / 8e12 * 1e3:.4f} ms); valid share {float(va.float().mean()):.3f}, "
          f"masks equal on {float((va == vb).float().mean()):.5f}, images within 1 LSB of the baseline on {agree:.4f} of the valid pixels", flush=True)
