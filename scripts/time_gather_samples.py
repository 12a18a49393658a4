"""Time of the supersampled gathers (gather_ss.hip; samples= of crop_panorama, reproject_image, rotate_panorama) at S = 1, 2, 3, 4 on the workloads of
scripts/time_pano_crop.py, scripts/time_reproject.py and scripts/time_pano_rotate.py, next to the composition the feature replaces: the existing
gather at S times the output size, then the block mean in float (over the valid samples for the re-projection, whose mask the composition also
has to fetch) and the uint8 conversion in torch.
  crop     B = 32 uint8 crops of 480 x 640 from a 4096 x 8192 panorama, no labels
  reproject B = 32 uint8 sources of 480 x 640 to 480 x 640, a pinhole roll-rectification, with the mask
  rotate   one uint8 2048 x 4096 panorama by (20, 35, 50) degrees to 1024 x 2048 (a minification by 2) and to 2048 x 4096, no labels
Both are timed with device events around the whole call after a warm-up, alternating in one process; medians of 25 calls.  Prints per workload and S:
both times, samples=S over samples=1 (the expectation is S x S: the kernels are VALU bound), and how many pixels of the two agree within 1 LSB.
`--kernel-only N` runs N calls of every workload and S and nothing else: the process of a separate `rocprofv3 --kernel-trace --stats` run."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.getcwd())
from perspectivefields_amd import crop_panorama, reproject_image, rotate_panorama

B, H, W, CALLS = 32, 480, 640, 25
rng = np.random.default_rng(0)
dev = lambda v: torch.tensor(v, dtype=torch.float64, device="cuda")
roll, pitch, yaw = rng.uniform(-20, 20, B), rng.uniform(-45, 45, B), rng.uniform(-180, 180, B)
focal = 0.5 / np.tan(np.radians(rng.uniform(40, 100, B)) / 2)
ROT = (20.0, 35.0, 50.0)


def to_u8(x):
    return (x + 0.5).floor().clamp(0, 255).to(torch.uint8)


def block_mean(img, valid, S):
    """(B, S h, S w, 3) uint8 -> (B, h, w, 3) uint8: the float mean of every S x S block, over the valid samples with a mask"""
    b, h, w = img.shape[0], img.shape[1] // S, img.shape[2] // S
    x = img.float().reshape(b, h, S, w, S, 3)
    if valid is None:
        return to_u8(x.mean((2, 4)))
    v = valid.reshape(b, h, S, w, S, 1).float()
    n = v.sum((2, 4))
    return to_u8((x * v).sum((2, 4)) / n.clamp(min=1)), n[..., 0] > 0


def workloads():
    pano = torch.from_numpy(rng.integers(0, 256, (4096, 8192, 3), dtype=np.uint8)).cuda()
    crop = lambda S, h, w: crop_panorama(pano, dev(roll), dev(pitch), dev(focal), yaw=dev(yaw), height=h, width=w, fields=False, samples=S)[0]
    yield "crop 4096 x 8192 -> 32 x 480 x 640", lambda S: crop(S, H, W), lambda S: block_mean(crop(1, S * H, S * W), None, S)

    src = torch.from_numpy(rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)).cuda()
    s = dict(roll=dev(roll), pitch=dev(pitch * 0.6), rel_focal=dev(focal))
    d = dict(roll=0.0, pitch=dev(pitch * 0.6), rel_focal=dev(focal))
    rep = lambda S, h, w: reproject_image(src, s, d, height=h, width=w, return_valid=True, samples=S)
    yield "reproject 32 x 480 x 640 -> 480 x 640, with the mask", lambda S: rep(S, H, W)[0], lambda S: block_mean(*rep(1, S * H, S * W), S)[0]

    small = pano[::2, ::2].contiguous()   # 2048 x 4096
    for h, w in ((1024, 2048), (2048, 4096)):
        rot = lambda S, hh, ww: rotate_panorama(small, *ROT, height=hh, width=ww, samples=S)
        yield f"rotate 2048 x 4096 -> {h} x {w}", (lambda S, h=h, w=w: rot(S, h, w)), (lambda S, h=h, w=w: block_mean(rot(1, S * h, S * w), None, S))


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


kernel_only = int(sys.argv[sys.argv.index("--kernel-only") + 1]) if "--kernel-only" in sys.argv else 0
for name, ours, composed in workloads():
    base = None
    for S in (1, 2, 3, 4):
        if kernel_only:
            for _ in range(kernel_only):
                ours(S)
            torch.cuda.synchronize()
            continue
        for _ in range(3):
            ours(S)
            composed(S)
        torch.cuda.synchronize()
        t_ours, t_comp = [], []
        for _ in range(CALLS):
            t_ours.append(timed(lambda: ours(S)))
            t_comp.append(timed(lambda: composed(S)))
        a, b = ours(S), composed(S)
        agree = float((a.int() - b.int()).abs().le(1).all(-1).float().mean())
        base = base or float(np.median(t_ours))
        print(f"{name}, S = {S}: samples=S {np.median(t_ours):.3f} ms (x{np.median(t_ours) / base:.2f} of S = 1), the S-times-larger gather + block mean "
              f"{np.median(t_comp):.3f} ms (x{np.median(t_comp) / np.median(t_ours):.2f}); within 1 LSB of each other on {agree:.5f} of the pixels", flush=True)
        del a, b
        torch.cuda.empty_cache()
