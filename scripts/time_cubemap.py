"""Time of the cube-map gathers (cube_gather.hip; cubemap_to_panorama, crop_cubemap) next to the obvious PyTorch composition on the same GPU:
  A  one uint8 cube of 1024 x 1024 faces -> a 2048 x 4096 panorama turned by (roll 20, pitch 35, yaw 50) degrees
  B  the same cube -> 32 pinhole views of 640 x 640 (rel_focal 0.6, yaws around the horizon, pitches -60 ... 60)
The baseline computes the directions with torch ops from the same model, picks the face by the major axis, runs F.grid_sample (bilinear, border
padding, align_corners=False) of every face over the whole output and selects per pixel: six samples per pixel, clamped at the face borders, so
with the seams the library's sampler does not have.  The float NCHW copy of the faces is prepared outside the timed window.  Both are timed with
device events around the whole call after a warm-up, alternating in one process; medians of 25 calls.  The bytes of a call are the output written
plus the cube read once.  `--kernel-only N` runs N calls of each case and nothing else: the process of a separate
`rocprofv3 --kernel-trace --stats` run."""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.getcwd())
from perspectivefields_amd import crop_cubemap, cubemap_to_panorama

N, CALLS = 1024, 25
PANO, ROT = (2048, 4096), (20.0, 35.0, 50.0)
VIEWS, VIEW, FOCAL = 32, 640, 0.6
rng = np.random.default_rng(0)
FRAMES = torch.tensor([[[1, 0, 0], [0, 1, 0], [0, 0, 1]], [[0, 0, -1], [0, 1, 0], [1, 0, 0]], [[-1, 0, 0], [0, 1, 0], [0, 0, -1]],
                       [[0, 0, 1], [0, 1, 0], [-1, 0, 0]], [[1, 0, 0], [0, 0, 1], [0, -1, 0]], [[1, 0, 0], [0, 0, -1], [0, 1, 0]]], dtype=torch.float32)   # r, d, n per face


def matrix(roll, pitch, yaw):
    r, p, y = (torch.as_tensor(np.radians(v), dtype=torch.float32, device="cuda") for v in (roll, pitch, yaw))
    cr, sr, cp, sp, cy, sy, z, o = torch.cos(r), torch.sin(r), torch.cos(p), torch.sin(p), torch.cos(y), torch.sin(y), torch.zeros_like(r), torch.ones_like(r)
    R = torch.stack([cr, -sr, z, cp * sr, cp * cr, -sp, sp * sr, sp * cr, cp], -1).reshape(*r.shape, 3, 3)
    Y = torch.stack([cy, z, sy, z, o, z, -sy, z, cy], -1).reshape(*r.shape, 3, 3)
    return Y @ R


def torch_sample(faces_nchw, X):
    """directions X (B, H, W, 3) -> uint8 (B, H, W, 3): per-face grid_sample, clamped at the borders, selected by the major axis"""
    ax = X.abs()
    fz = (ax[..., 2] >= ax[..., 0]) & (ax[..., 2] >= ax[..., 1])
    fx = ~fz & (ax[..., 0] >= ax[..., 1])
    face = torch.where(fz, torch.where(X[..., 2] < 0, 2, 0), torch.where(fx, torch.where(X[..., 0] > 0, 1, 3), torch.where(X[..., 1] < 0, 4, 5)))
    out = torch.zeros(X.shape[:-1] + (3,), dtype=torch.float32, device="cuda")
    frames = FRAMES.cuda()
    for k in range(6):
        xn = X @ frames[k, 2]
        grid = torch.stack([X @ frames[k, 0] / xn, X @ frames[k, 1] / xn], -1)   # (a, b) in [-1, 1] is grid_sample's coordinate with align_corners=False
        c = F.grid_sample(faces_nchw[k:k + 1].expand(X.shape[0], -1, -1, -1), grid, mode="bilinear", padding_mode="border", align_corners=False)
        out = torch.where((face == k)[..., None], c.permute(0, 2, 3, 1), out)
    return (out + 0.5).floor().clamp(0, 255).to(torch.uint8)


def torch_panorama(faces_nchw):
    H, W = PANO
    lon = ((torch.arange(W, device="cuda", dtype=torch.float32) + 0.5) / W - 0.5) * (2 * np.pi)
    lat = (0.5 - (torch.arange(H, device="cuda", dtype=torch.float32) + 0.5) / H) * np.pi
    lat, lon = torch.meshgrid(lat, lon, indexing="ij")
    D = torch.stack([torch.cos(lat) * torch.sin(lon), -torch.sin(lat), torch.cos(lat) * torch.cos(lon)], -1)
    return torch_sample(faces_nchw, (D @ matrix(*ROT).T)[None])


def torch_views(faces_nchw, pitch, yaw):
    x = (torch.arange(VIEW, device="cuda", dtype=torch.float32) + 0.5 - 0.5 * VIEW) / (FOCAL * VIEW)
    y, x = torch.meshgrid(x, x, indexing="ij")
    rays = torch.stack([x, y, torch.ones_like(x)], -1)
    Q = matrix(np.zeros(VIEWS), pitch, yaw)
    return torch_sample(faces_nchw, torch.einsum("bij,hwj->bhwi", Q, rays))


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


cube = torch.from_numpy(rng.integers(0, 256, (6, N, N, 3), dtype=np.uint8)).cuda()
pitch, yaw = np.linspace(-60.0, 60.0, VIEWS), np.arange(VIEWS) * (360.0 / VIEWS)
ours = {"A": lambda: cubemap_to_panorama(cube, height=PANO[0], width=PANO[1], roll=ROT[0], pitch=ROT[1], yaw=ROT[2])[0],
        "B": lambda: crop_cubemap(cube, 0.0, pitch, FOCAL, yaw=yaw, height=VIEW, width=VIEW, fields=False)[0]}
if "--kernel-only" in sys.argv:
    for _ in range(int(sys.argv[sys.argv.index("--kernel-only") + 1])):
        ours["A"]()
        ours["B"]()
    torch.cuda.synchronize()
    sys.exit(0)
faces = cube.permute(0, 3, 1, 2).float().contiguous()
theirs = {"A": lambda: torch_panorama(faces)[0], "B": lambda: torch_views(faces, pitch, yaw)}
for case, what in (("A", f"cube {N} -> panorama {PANO[0]} x {PANO[1]}"), ("B", f"cube {N} -> {VIEWS} views of {VIEW} x {VIEW}")):
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
    moved = a.numel() + cube.numel()
    t = np.median(t_ours)
    print(f"uint8 {what}: library {t:.3f} ms, torch {np.median(t_torch):.3f} ms (x{np.median(t_torch) / t:.2f}); {moved / 1e6:.1f} MB per call (output written + "
          f"cube read once), {moved / (t * 1e-3) / 1e9:.1f} GB/s achieved (at 8 TB/s: {moved / 8e12 * 1e3:.4f} ms); within 1 LSB of the clamped baseline on "
          f"{agree:.5f} of the pixels (the rest lies on the seams)", flush=True)
