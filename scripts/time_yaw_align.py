"""Time of the yaw alignment of camera views (yaw_align.hip, pf_yaw_moments, align_yaw) next to the obvious PyTorch composition on the same GPU:
8 uint8 views of 480 x 640 cropped from a low-pass noise panorama at yaws 45 degrees apart, the default stride (10: 48 x 64 samples of each view),
360 candidates of 1 degree, all 56 ordered pairs.
The baseline computes the same model with torch ops: the luminance planes once, per ordered pair the rays of b's samples, for all 360
candidates at once the turned rays, the pinhole projection into a and the coverage test, one F.grid_sample call per pair (bilinear, border
padding, align_corners=False; its batch dimension is the candidates, each with its own grid), the masked moments, the score in float64 and
the best candidate per pair.  That is 56 grid_sample calls; one call per (pair, candidate) would be 20160.  The tree on the host is not part
of the baseline.  Both are timed with device events around the whole call after a warm-up, alternating in one process; medians of 25 calls.
The two must agree on the best candidate of every pair that align_yaw scores at min_score (0.8) or more.
`--kernel-only N` runs N align_yaw calls and nothing else: the process of a separate `rocprofv3 --kernel-trace --stats` run."""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.getcwd())
from perspectivefields_amd import align_yaw, crop_panorama, yaw_scores

N, H, W, K, CALLS = 8, 480, 640, 360, 25
STRIDE = max(1, min(H, W) // 48)
dev = lambda v: torch.tensor(v, dtype=torch.float64, device="cuda")
roll = np.array([3.0, -4.0, 6.0, 0.0, -7.0, 2.0, 5.0, -3.0])
pitch = np.array([5.0, -8.0, 10.0, -5.0, 4.0, 0.0, -6.0, 8.0])
yaw = np.array([0.0, 45.5, 90.25, 134.0, 181.5, 226.0, 270.75, 315.0])
focal = np.full(N, 0.6)
CAMS = dict(roll=dev(roll), pitch=dev(pitch), rel_focal=dev(focal))
PAIRS = [(a, b) for a in range(N) for b in range(N) if a != b]
CAND = -180.0 + np.arange(K, dtype=np.float64)


def panorama(seed=0, Hp=256, Wp=512):
    """uint8 (Hp, Wp, 3): Gaussian noise low-passed in the Fourier domain, the scene of tests/test_yaw_align_ref.py at twice the size"""
    rng = np.random.default_rng(seed)
    fy, fx = np.meshgrid(np.fft.fftfreq(Hp) * Hp, np.fft.fftfreq(Wp) * Wp, indexing="ij")
    w = np.exp(-(fx ** 2 + (2 * fy) ** 2) / (2 * 12.0 ** 2))
    P = np.stack([np.fft.ifft2(np.fft.fft2(rng.standard_normal((Hp, Wp))) * w).real for _ in range(3)], -1)
    return np.floor(255.0 * (P - P.min()) / (P.max() - P.min()) + 0.5).astype(np.uint8)


def rotation(r, p):
    cr, sr, cp, sp, z = torch.cos(r), torch.sin(r), torch.cos(p), torch.sin(p), torch.zeros_like(r)
    return torch.stack([cr, -sr, z, cp * sr, cp * cr, -sp, sp * sr, sp * cr, cp], -1).reshape(-1, 3, 3)


def torch_scores(views):
    """the same model (centred pinhole views) with torch ops: the best candidate and its score per ordered pair"""
    L = (views.float() * torch.tensor([0.299, 0.587, 0.114], device="cuda")).sum(-1) - 127.5          # (N, H, W)
    R = rotation(torch.deg2rad(CAMS["roll"].float()), torch.deg2rad(CAMS["pitch"].float()))
    Fpx = CAMS["rel_focal"].float() * H
    cols = torch.arange(0, W, STRIDE, device="cuda", dtype=torch.float32) + 0.5 - 0.5 * W
    rows = torch.arange(0, H, STRIDE, device="cuda", dtype=torch.float32) + 0.5 - 0.5 * H
    rows, cols = torch.meshgrid(rows, cols, indexing="ij")
    d = torch.deg2rad(torch.as_tensor(CAND, device="cuda").float())
    cd, sd = torch.cos(d)[:, None, None], torch.sin(d)[:, None, None]
    best = []
    for a, b in PAIRS:
        X = torch.stack([cols / Fpx[b], rows / Fpx[b], torch.ones_like(cols)], -1)
        X = X / X.norm(dim=-1, keepdim=True)
        Wd = X @ R[b].T                                                                                # (Sr, Sc, 3)
        V = torch.stack([cd * Wd[..., 0] + sd * Wd[..., 2], Wd[..., 1].expand(K, -1, -1), cd * Wd[..., 2] - sd * Wd[..., 0]], -1)
        Xa = V @ R[a]                                                                                  # rows of R_a^T V: (K, Sr, Sc, 3)
        p, q = Fpx[a] * Xa[..., 0] / Xa[..., 2] + 0.5 * W, Fpx[a] * Xa[..., 1] / Xa[..., 2] + 0.5 * H
        m = (Xa[..., 2] > 0) & (p > 0) & (W - p > 0) & (q > 0) & (H - q > 0)
        grid = torch.stack([p / W * 2 - 1, q / H * 2 - 1], -1)
        grid = torch.where(m[..., None], grid, torch.zeros_like(grid))   # no NaN into grid_sample
        x = F.grid_sample(L[a][None, None].expand(K, -1, -1, -1), grid, mode="bilinear", padding_mode="border", align_corners=False)[:, 0].double()
        y = L[b][::STRIDE, ::STRIDE].double().expand(K, -1, -1)
        m = m.double()
        n, sx, sy = m.sum((1, 2)), (x * m).sum((1, 2)), (y * m).sum((1, 2))
        sxx, syy, sxy = (x * x * m).sum((1, 2)), (y * y * m).sum((1, 2)), (x * y * m).sum((1, 2))
        va, vb = n * sxx - sx * sx, n * syy - sy * sy
        ok = (n >= 0.1 * rows.numel()) & (va > 0) & (vb > 0)
        z = torch.where(ok, (n * sxy - sx * sy) / torch.sqrt(torch.where(ok, va * vb, torch.ones_like(va))), torch.full_like(va, float("-inf")))
        best.append(torch.stack([z.max(), z.argmax().double()]))
    return torch.stack(best)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


views, _, _ = crop_panorama(torch.from_numpy(panorama()).cuda(), CAMS["roll"], CAMS["pitch"], CAMS["rel_focal"], yaw=dev(yaw), height=H, width=W, fields=False)
ours = lambda: align_yaw(views, CAMS, return_info=True)
if "--kernel-only" in sys.argv:
    for _ in range(int(sys.argv[sys.argv.index("--kernel-only") + 1])):
        ours()
    torch.cuda.synchronize()
    sys.exit(0)
theirs = lambda: torch_scores(views)
for _ in range(3):
    ours()
    theirs()
torch.cuda.synchronize()
t_ours, t_torch = [], []
for _ in range(CALLS):
    t_ours.append(timed(ours))
    t_torch.append(timed(theirs))
(got, info), base = ours(), theirs().cpu().numpy()
score = yaw_scores(views, CAMS, PAIRS, CAND)[0]
peak, k = (t.cpu().numpy() for t in score.max(1))
high = peak >= 0.8
assert high.sum() >= 2 * N, high.sum()
assert (k[high] == base[high, 1].astype(np.int64)).all(), (k[high], base[high, 1])
err = np.abs((got.cpu().numpy() - (yaw - yaw[0]) + 180.0) % 360.0 - 180.0).max()
assert info["linked"].all() and err <= 0.5, (info["linked"], err)
samples = len(PAIRS) * K * (-(-H // STRIDE)) * (-(-W // STRIDE))
print(f"{N} views {H} x {W}, stride {STRIDE}, {K} candidates, {len(PAIRS)} ordered pairs ({samples / 1e6:.1f} M projected samples): align_yaw "
      f"{np.median(t_ours):.3f} ms, torch {np.median(t_torch):.3f} ms (x{np.median(t_torch) / np.median(t_ours):.2f}); {int(high.sum())} pairs score >= 0.8 and "
      f"both agree on their best candidates (largest score difference there {np.abs(peak[high] - base[high, 0]).max():.2e}); yaws within {err:.4f} deg of the truth", flush=True)
