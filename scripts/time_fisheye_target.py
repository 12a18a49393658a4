"""Time of the fisheye target gather (fisheye_target.hip; panorama_to_fisheye) next to the obvious PyTorch composition on the same GPU:
  A  one uint8 panorama of 2048 x 4096 -> one dual-fisheye frame of 2880 x 5760 (two equidistant lenses of 200 degrees, side by side)
  B  the same panorama -> 32 single-lens frames of 640 x 640 (equidistant, 190 degrees, yaws around the horizon, pitches -60 ... 60)
The baseline computes the inverse projection with torch ops from the same model (equidistant, no polynomial: theta = r / F), turns the directions
into the world, and runs F.grid_sample (bilinear, border padding, align_corners=False) of the panorama once per lens over the whole output; the
first owner wins.  The float NCHW copy of the panorama, padded by one wrapped column on each side, is prepared outside the timed window.  Both are
timed with device events around the whole call after a warm-up, alternating in one process; medians of 25 calls.  The bytes of a call are the
output written plus the panorama read once.
`--kernel-only N` runs N calls of each case and nothing else: the process of a separate `rocprofv3 --kernel-trace --stats` run."""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.getcwd())
from perspectivefields_amd import dual_fisheye_lenses, fisheye_lens, panorama_to_fisheye

PANO, CALLS = (2048, 4096), 25
FRAME, FOV = (2880, 5760), 200.0
VIEWS, VIEW, VIEW_FOV = 32, 640, 190.0
rng = np.random.default_rng(0)
DUAL = dual_fisheye_lenses(*FRAME, FOV, roll=2.0, pitch=-3.0, yaw=5.0)
SINGLE = np.stack([fisheye_lens(VIEW_FOV, radius=VIEW / 2, center=(VIEW / 2, VIEW / 2), pitch=p, yaw=y)[None]
                   for p, y in zip(np.linspace(-60.0, 60.0, VIEWS), np.arange(VIEWS) * (360.0 / VIEWS))])   # (32, 1, 12)


def matrix(lens):
    r, p, y = (torch.as_tensor(lens[..., k], dtype=torch.float32, device="cuda") for k in range(3))
    cr, sr, cp, sp, cy, sy, z, o = torch.cos(r), torch.sin(r), torch.cos(p), torch.sin(p), torch.cos(y), torch.sin(y), torch.zeros_like(r), torch.ones_like(r)
    R = torch.stack([cr, -sr, z, cp * sr, cp * cr, -sp, sp * sr, sp * cr, cp], -1).reshape(*r.shape, 3, 3)
    Y = torch.stack([cy, z, sy, z, o, z, -sy, z, cy], -1).reshape(*r.shape, 3, 3)
    return Y @ R


def torch_frames(pano_nchw, table, H, W):
    """lens table (B, L, 12) -> uint8 (B, H, W, 3): per lens the inverse projection and one grid_sample of the padded panorama; the first owner wins"""
    Hp, Wp = pano_nchw.shape[-2], pano_nchw.shape[-1] - 2
    B = table.shape[0]
    b, a = torch.meshgrid(torch.arange(H, device="cuda", dtype=torch.float32) + 0.5, torch.arange(W, device="cuda", dtype=torch.float32) + 0.5, indexing="ij")
    out = torch.zeros((B, H, W, 3), dtype=torch.float32, device="cuda")
    owned = torch.zeros((B, H, W), dtype=torch.bool, device="cuda")
    for l in range(table.shape[1]):
        lens = torch.as_tensor(table[:, l], dtype=torch.float32, device="cuda")[:, :, None, None]   # (B, 12, 1, 1)
        dx, dy = a[None] - lens[:, 4], b[None] - lens[:, 5]
        r = torch.hypot(dx, dy)
        th = r / lens[:, 3]   # equidistant, k = 0
        own = (th < lens[:, 6]) & ~owned
        s = torch.sin(th) / r.clamp(min=1e-30)
        X = torch.stack([s * dx, s * dy, torch.cos(th)], -1)
        D = torch.einsum("bij,bhwj->bhwi", matrix(table[:, l]), X)
        u = (torch.atan2(D[..., 0], D[..., 2]) / (2 * np.pi) + 0.5) * Wp   # pixel-edge units, grid_sample's with align_corners=False
        v = (torch.atan2(D[..., 1], torch.hypot(D[..., 0], D[..., 2])) / np.pi + 0.5) * Hp
        grid = torch.stack([(u + 1.0) / (Wp + 2) * 2 - 1, v / Hp * 2 - 1], -1)
        c = F.grid_sample(pano_nchw.expand(B, -1, -1, -1), grid, mode="bilinear", padding_mode="border", align_corners=False)
        out = torch.where(own[..., None], c.permute(0, 2, 3, 1), out)
        owned = owned | own
    return (out + 0.5).floor().clamp(0, 255).to(torch.uint8)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


pano = torch.from_numpy(rng.integers(0, 256, PANO + (3,), dtype=np.uint8)).cuda()
ours = {"A": lambda: panorama_to_fisheye(pano, DUAL, height=FRAME[0], width=FRAME[1]),
        "B": lambda: panorama_to_fisheye(pano, SINGLE, height=VIEW, width=VIEW, pano_index=[0] * VIEWS)}
if "--kernel-only" in sys.argv:
    for _ in range(int(sys.argv[sys.argv.index("--kernel-only") + 1])):
        ours["A"]()
        ours["B"]()
    torch.cuda.synchronize()
    sys.exit(0)
nchw = pano.permute(2, 0, 1).float().contiguous()[None]
nchw = torch.cat([nchw[..., -1:], nchw, nchw[..., :1]], -1).contiguous()
theirs = {"A": lambda: torch_frames(nchw, DUAL[None], *FRAME), "B": lambda: torch_frames(nchw, SINGLE, VIEW, VIEW)}
for case, what in (("A", f"panorama {PANO[0]} x {PANO[1]} -> dual frame {FRAME[0]} x {FRAME[1]}"), ("B", f"panorama {PANO[0]} x {PANO[1]} -> {VIEWS} frames of {VIEW} x {VIEW}")):
    for _ in range(3):
        ours[case]()
        theirs[case]()
    torch.cuda.synchronize()
    t_ours, t_torch = [], []
    for _ in range(CALLS):
        t_ours.append(timed(ours[case]))
        t_torch.append(timed(theirs[case]))
    a, b = ours[case](), theirs[case]()
    agree = float((a.int() - b.int()).abs().le(1).all(-1).float().mean())
    moved = a.numel() + pano.numel()
    t = np.median(t_ours)
    print(f"uint8 {what}: library {t:.3f} ms, torch {np.median(t_torch):.3f} ms (x{np.median(t_torch) / t:.2f}); {moved / 1e6:.1f} MB per call (output written + "
          f"panorama read once), {moved / (t * 1e-3) / 1e9:.1f} GB/s achieved (at 8 TB/s: {moved / 8e12 * 1e3:.4f} ms); within 1 LSB of the baseline on "
          f"{agree:.5f} of the pixels", flush=True)
