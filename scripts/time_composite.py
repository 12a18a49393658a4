"""Time of the paste (composite.hip, pf_composite, composite_objects) next to what a caller can compose without it on the same GPU: a 640 x 640
background, a 160 x 120 object with an elliptical alpha, the variants (1, 10 deg) and (0.5, -10 deg) at samples 1 and 2, uint8 and float32.
The baseline is the torch composition: `affine_grid` + `grid_sample` (bilinear, zeros outside) on the premultiplied colour and the alpha -- the same
model up to fp32 rounding; samples = 2 as a grid of twice the box and `avg_pool2d` --, then the blend into a copy of the background and, for uint8,
the rounding.  Both are timed with device events around the whole call after a warm-up, alternating in one process; medians of 25 calls.  The two
must agree to one uint8 step / 0.05 of the 0 - 255 scale.
Most of the kernel is a copy, so the yardstick for its bytes per second is `copy_` of the same image in the same process: the last lines time one
call of 32 jobs (32 backgrounds of 640 x 640 in one batch tensor) next to `copy_` of that batch, bytes = background read + output written.
`--kernel-only N` runs N calls of every configuration and N `copy_` of the single image and of the batch and nothing else: the process of a
separate `rocprofv3 --kernel-trace --stats` run, which gives the kernels' own times."""
import ctypes
import math
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.getcwd())
from perspectivefields_amd import composite_objects
from perspectivefields_amd.engine import load_library

H = W = 640
h, w, AT, CALLS, BATCH = 160, 120, (212, 244), 25, 32
VARIANTS, SAMPLES = ((1.0, 10.0), (0.5, -10.0)), (1, 2)


def out_size(s, r):
    hw = (ctypes.c_int32 * 2)()
    assert load_library().pf_fields_transform_size(h, w, s, r, hw) == 0
    return hw[0], hw[1]


def torch_composite(bg, obj, alpha, s, r, at, S):
    """pf_composite's soft edge at opacity 1 with affine_grid + grid_sample"""
    ho, wo = out_size(s, r)
    c, sn = math.cos(math.radians(r)), math.sin(math.radians(r))
    # normalised box coordinates -> normalised object coordinates (align_corners=False on both sides)
    theta = torch.tensor([[[c * wo / (w * s), sn * ho / (w * s), 0.0], [-sn * wo / (h * s), c * ho / (h * s), 0.0]]], dtype=torch.float32, device="cuda")
    grid = F.affine_grid(theta, (1, 4, S * ho, S * wo), align_corners=False)
    src = torch.cat([obj.permute(2, 0, 1).float() * alpha, alpha[None]])[None]   # premultiplied colour, alpha
    res = F.grid_sample(src, grid, mode="bilinear", padding_mode="zeros", align_corners=False)
    if S > 1:
        res = F.avg_pool2d(res, S)
    P, A = res[0, :3].permute(1, 2, 0), res[0, 3, :, :, None]
    out = bg.clone()
    box = out[at[0]:at[0] + ho, at[1]:at[1] + wo]
    mix = box.float() * (1.0 - A) + P
    box.copy_(torch.floor(mix + 0.5).clamp(0, 255) if bg.dtype == torch.uint8 else mix)
    return out


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def alternate(ours, theirs):
    for _ in range(3):
        ours()
        theirs()
    torch.cuda.synchronize()
    t_ours, t_theirs = [], []
    for _ in range(CALLS):
        t_ours.append(timed(ours))
        t_theirs.append(timed(theirs))
    return float(np.median(t_ours)), float(np.median(t_theirs))


g = torch.Generator(device="cuda").manual_seed(0)
rr, cc = torch.meshgrid(torch.arange(h, device="cuda"), torch.arange(w, device="cuda"), indexing="ij")
alpha = (((rr + 0.5 - h / 2) / (h / 2)) ** 2 + ((cc + 0.5 - w / 2) / (w / 2)) ** 2 <= 1.0).float()
pictures = {}
for dtype in (torch.uint8, torch.float32):
    make = lambda *s: torch.randint(0, 256, s, device="cuda", generator=g).to(dtype)
    pictures[dtype] = make(H, W, 3), make(h, w, 3), make(BATCH, H, W, 3)
kernel_only = int(sys.argv[sys.argv.index("--kernel-only") + 1]) if "--kernel-only" in sys.argv else 0

for dtype, (bg, obj, batch) in pictures.items():
    name = str(dtype).split(".")[1]
    esize = bg.element_size()
    spare, spare_batch = torch.empty_like(bg), torch.empty_like(batch)
    for (s, r), S in ((v, S) for v in VARIANTS for S in SAMPLES):
        ours = lambda: composite_objects(bg, obj, scale=s, rotation=r, offset=AT, alpha=alpha, samples=S)
        theirs = lambda: torch_composite(bg, obj, alpha, s, r, AT, S)
        if kernel_only:
            for _ in range(kernel_only):
                ours()
            continue
        diff = (ours().double() - theirs().double()).abs().max().item()
        assert diff <= (1.0 if dtype == torch.uint8 else 0.05), (name, s, r, S, diff)
        t_ours, t_torch = alternate(ours, theirs)
        print(f"{name} background {H} x {W}, object {h} x {w} ({int(alpha.sum())} pixels in the ellipse) -> box {out_size(s, r)}, scale {s}, rotation {r}, "
              f"samples {S}: composite_objects {t_ours:.3f} ms, affine_grid + grid_sample + blend {t_torch:.3f} ms (x{t_torch / t_ours:.1f}); "
              f"largest difference {diff:.3g}", flush=True)
    one = lambda: composite_objects(bg, obj, scale=1.0, rotation=10.0, offset=AT, alpha=alpha)
    many = lambda: composite_objects(batch, obj, scale=1.0, rotation=10.0, offset=AT, alpha=alpha)
    if kernel_only:
        for _ in range(kernel_only):
            many()
            spare.copy_(bg)
            spare_batch.copy_(batch)
        continue
    for what, fn, copy, nbytes in (("one image", one, lambda: spare.copy_(bg), 2 * H * W * 3 * esize), (f"{BATCH} jobs in one call", many, lambda: spare_batch.copy_(batch), 2 * BATCH * H * W * 3 * esize)):
        t_ours, t_copy = alternate(fn, copy)
        print(f"{name}, {what}, scale 1, rotation 10, samples 1, {nbytes / 1e6:.1f} MB read + written: composite_objects {t_ours:.3f} ms = "
              f"{nbytes / t_ours / 1e6:.1f} GB/s of the whole call, copy_ {t_copy:.3f} ms = {nbytes / t_copy / 1e6:.1f} GB/s", flush=True)
torch.cuda.synchronize()
