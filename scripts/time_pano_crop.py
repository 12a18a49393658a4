"""Time of the panorama crop (pano_crop.hip, pf_pano_crop) next to the obvious PyTorch composition on the same GPU: B = 32 crops of
480 x 640 from a uint8 panorama of 2048 x 4096 and of 4096 x 8192, with and without the ground-truth fields.  The baseline builds the
sampling grid with torch ops from the same parameters, runs F.grid_sample (bilinear, align_corners=False) on a float copy of the
panorama padded by one wrapped column on each side (prepared outside the timed window), converts to uint8 NHWC and, with labels, calls
fields_from_params once per crop.  Both are timed with device events after a warm-up, alternating in one process; medians of 25 calls.
Prints the bytes each call writes, for the kernel time of a separate `rocprofv3 --kernel-trace --stats` run."""
import math
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.getcwd())
from perspectivefields_amd import crop_panorama, fields_from_params

B, H, W, CALLS = 32, 480, 640, 25
rng = np.random.default_rng(0)
roll, pitch, yaw = rng.uniform(-20, 20, B), rng.uniform(-45, 45, B), rng.uniform(-180, 180, B)
focal = 0.5 / np.tan(np.radians(rng.uniform(40, 100, B)) / 2)
cam = [torch.tensor(v, dtype=torch.float64, device="cuda") for v in (roll, pitch, yaw, focal)]


def torch_crop(pano_pad, Hp, Wp, labels):
    """grid from the same model (pinhole), grid_sample on the padded float panorama, uint8 NHWC; fields_from_params per crop"""
    r, p, y = (torch.deg2rad(t).float() for t in cam[:3])
    f = cam[3].float()
    cols = torch.arange(W, device="cuda", dtype=torch.float32) + 0.5
    rows = torch.arange(H, device="cuda", dtype=torch.float32) + 0.5
    x = (cols[None, None, :] - 0.5 * W) / (f[:, None, None] * H)
    yy = (rows[None, :, None] - 0.5 * H) / (f[:, None, None] * H)
    x, yy = x.expand(B, H, W), yy.expand(B, H, W)
    z = torch.ones_like(x)
    cr, sr, cp, sp = (v[:, None, None] for v in (torch.cos(r), torch.sin(r), torch.cos(p), torch.sin(p)))
    xw = cr * x - sr * yy
    yw = cp * sr * x + cp * cr * yy - sp * z
    zw = sp * sr * x + sp * cr * yy + cp * z
    lat = -torch.atan2(yw, torch.sqrt(xw * xw + zw * zw))
    lon = torch.remainder(y[:, None, None] + torch.atan2(xw, zw) + math.pi, 2 * math.pi) - math.pi
    u = (lon / (2 * math.pi) + 0.5) * Wp - 0.5 + 1.0           # +1: the wrapped column on the left
    v = (0.5 - lat / math.pi) * Hp - 0.5
    grid = torch.stack([(u + 0.5) / (Wp + 2) * 2 - 1, (v + 0.5) / Hp * 2 - 1], -1)
    out = F.grid_sample(pano_pad, grid.reshape(1, B * H, W, 2), mode="bilinear", padding_mode="border", align_corners=False)   # one panorama, B crops stacked
    img = (out + 0.5).floor().clamp(0, 255).to(torch.uint8).reshape(3, B, H, W).permute(1, 2, 3, 0).contiguous()
    fields = [fields_from_params(cam[0][i], cam[1][i], cam[3][i], 0.0, 0.0, H, W) for i in range(B)] if labels else None
    return img, fields


def ours(pano, labels):
    return crop_panorama(pano, cam[0], cam[1], cam[3], yaw=cam[2], height=H, width=W, fields=labels)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


for Hp, Wp in ((2048, 4096), (4096, 8192)):
    pano = torch.from_numpy(rng.integers(0, 256, (Hp, Wp, 3), dtype=np.uint8)).cuda()
    pano_pad = pano.permute(2, 0, 1).float()
    pano_pad = torch.cat([pano_pad[:, :, -1:], pano_pad, pano_pad[:, :, :1]], 2)[None].contiguous()
    for labels in (False, True):
        for _ in range(3):
            ours(pano, labels)
            torch_crop(pano_pad, Hp, Wp, labels)
        torch.cuda.synchronize()
        t_ours, t_torch = [], []
        for _ in range(CALLS):
            t_ours.append(timed(lambda: ours(pano, labels)))
            t_torch.append(timed(lambda: torch_crop(pano_pad, Hp, Wp, labels)))
        a, b = ours(pano, labels)[0], torch_crop(pano_pad, Hp, Wp, labels)[0]
        agree = float((a.int() - b.int()).abs().le(1).float().mean())
        written = B * H * W * 3 + (B * H * W * 12 if labels else 0)
        print(f"pano {Hp}x{Wp} labels={labels}: crop_panorama {np.median(t_ours):.3f} ms, torch {np.median(t_torch):.3f} ms "
              f"(x{np.median(t_torch) / np.median(t_ours):.2f}); {written / 1e6:.1f} MB written per call "
              f"(HBM write bound at 8 TB/s: {written / 8e12 * 1e3:.4f} ms); images within 1 LSB of the baseline: {agree:.4f}", flush=True)
