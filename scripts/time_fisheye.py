"""Time of the fisheye gathers (fisheye_gather.hip; fisheye_to_panorama, crop_fisheye) next to the obvious PyTorch composition on the same GPU:
  A  one uint8 dual-fisheye frame of 2880 x 5760 (two equidistant lenses of 200 degrees) -> a 2048 x 4096 panorama turned by (roll 20, pitch 35,
     yaw 50) degrees
  B  the same frame -> 32 pinhole views of 640 x 640 (rel_focal 0.6, yaws around the horizon, pitches -60 ... 60)
The baseline computes the directions with torch ops from the same model, projects them into both lenses, runs F.grid_sample (bilinear, border
padding, align_corners=False) of the whole frame once per lens over the whole output and blends the two samples with the feather weights: two
samples per pixel.  The float NCHW copy of the frame is prepared outside the timed window.  Both are timed with device events around the whole call
after a warm-up, alternating in one process; medians of 25 calls.  The bytes of a call are the output written plus the frame read once.
`--kernel-only N` runs N calls of each case and nothing else: the process of a separate `rocprofv3 --kernel-trace --stats` run."""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.getcwd())
from perspectivefields_amd import crop_fisheye, dual_fisheye_lenses, fisheye_to_panorama

FRAME, FOV, CALLS = (2880, 5760), 200.0, 25
PANO, ROT = (2048, 4096), (20.0, 35.0, 50.0)
VIEWS, VIEW, FOCAL = 32, 640, 0.6
rng = np.random.default_rng(0)
LENSES = dual_fisheye_lenses(*FRAME, FOV, roll=2.0, pitch=-3.0, yaw=5.0)


def matrix(roll, pitch, yaw, deg=True):
    r, p, y = (torch.as_tensor(np.radians(v) if deg else v, dtype=torch.float32, device="cuda") for v in (roll, pitch, yaw))
    cr, sr, cp, sp, cy, sy, z, o = torch.cos(r), torch.sin(r), torch.cos(p), torch.sin(p), torch.cos(y), torch.sin(y), torch.zeros_like(r), torch.ones_like(r)
    R = torch.stack([cr, -sr, z, cp * sr, cp * cr, -sp, sp * sr, sp * cr, cp], -1).reshape(*r.shape, 3, 3)
    Y = torch.stack([cy, z, sy, z, o, z, -sy, z, cy], -1).reshape(*r.shape, 3, 3)
    return Y @ R


def torch_sample(frame_nchw, D):
    """world directions D (B, H, W, 3) -> uint8 (B, H, W, 3): one grid_sample of the frame per lens, blended with the feather weights"""
    Hs, Ws = frame_nchw.shape[-2:]
    S = torch.zeros(D.shape[:-1], dtype=torch.float32, device="cuda")
    C = torch.zeros(D.shape[:-1] + (3,), dtype=torch.float32, device="cuda")
    for lens in LENSES:
        X = D @ matrix(*lens[:3], deg=False)   # Q^T D
        h = torch.hypot(X[..., 0], X[..., 1])
        th = torch.atan2(h, X[..., 2])
        s = float(lens[3]) * th / h   # equidistant, k = 0
        a, b = float(lens[4]) + s * X[..., 0], float(lens[5]) + s * X[..., 1]
        cov = (th < float(lens[6])) & (a >= 0) & (a <= Ws) & (b >= 0) & (b <= Hs)
        w = torch.where(cov, ((float(lens[6]) - th) / float(lens[11])).clamp(max=1.0), torch.zeros_like(th))
        grid = torch.stack([a / Ws * 2 - 1, b / Hs * 2 - 1], -1)   # pixel-edge coordinates are grid_sample's with align_corners=False
        c = F.grid_sample(frame_nchw.expand(D.shape[0], -1, -1, -1), grid, mode="bilinear", padding_mode="border", align_corners=False)
        S = S + w
        C = C + w[..., None] * c.permute(0, 2, 3, 1)
    out = torch.where((S > 0)[..., None], C / S.clamp(min=1e-30)[..., None], torch.zeros_like(C))
    return (out + 0.5).floor().clamp(0, 255).to(torch.uint8)


def torch_panorama(frame_nchw):
    H, W = PANO
    lon = ((torch.arange(W, device="cuda", dtype=torch.float32) + 0.5) / W - 0.5) * (2 * np.pi)
    lat = (0.5 - (torch.arange(H, device="cuda", dtype=torch.float32) + 0.5) / H) * np.pi
    lat, lon = torch.meshgrid(lat, lon, indexing="ij")
    D = torch.stack([torch.cos(lat) * torch.sin(lon), -torch.sin(lat), torch.cos(lat) * torch.cos(lon)], -1)
    return torch_sample(frame_nchw, (D @ matrix(*ROT).T)[None])


def torch_views(frame_nchw, pitch, yaw):
    x = (torch.arange(VIEW, device="cuda", dtype=torch.float32) + 0.5 - 0.5 * VIEW) / (FOCAL * VIEW)
    y, x = torch.meshgrid(x, x, indexing="ij")
    rays = torch.stack([x, y, torch.ones_like(x)], -1)
    Q = matrix(np.zeros(VIEWS), pitch, yaw)
    return torch_sample(frame_nchw, torch.einsum("bij,hwj->bhwi", Q, rays))


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


frame = torch.from_numpy(rng.integers(0, 256, FRAME + (3,), dtype=np.uint8)).cuda()
pitch, yaw = np.linspace(-60.0, 60.0, VIEWS), np.arange(VIEWS) * (360.0 / VIEWS)
ours = {"A": lambda: fisheye_to_panorama(frame, LENSES, height=PANO[0], width=PANO[1], roll=ROT[0], pitch=ROT[1], yaw=ROT[2])[0],
        "B": lambda: crop_fisheye(frame, LENSES, 0.0, pitch, FOCAL, yaw=yaw, height=VIEW, width=VIEW, fields=False)[0]}
if "--kernel-only" in sys.argv:
    for _ in range(int(sys.argv[sys.argv.index("--kernel-only") + 1])):
        ours["A"]()
        ours["B"]()
    torch.cuda.synchronize()
    sys.exit(0)
nchw = frame.permute(2, 0, 1).float().contiguous()[None]
theirs = {"A": lambda: torch_panorama(nchw)[0], "B": lambda: torch_views(nchw, pitch, yaw)}
for case, what in (("A", f"frame {FRAME[0]} x {FRAME[1]} -> panorama {PANO[0]} x {PANO[1]}"), ("B", f"frame {FRAME[0]} x {FRAME[1]} -> {VIEWS} views of {VIEW} x {VIEW}")):
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
    moved = a.numel() + frame.numel()
    t = np.median(t_ours)
    print(f"uint8 {what}: library {t:.3f} ms, torch {np.median(t_torch):.3f} ms (x{np.median(t_torch) / t:.2f}); {moved / 1e6:.1f} MB per call (output written + "
          f"frame read once), {moved / (t * 1e-3) / 1e9:.1f} GB/s achieved (at 8 TB/s: {moved / 8e12 * 1e3:.4f} ms); within 1 LSB of the baseline on "
          f"{agree:.5f} of the pixels", flush=True)
