"""Time of the field transports (field_transport.hip, pf_reproject_fields / pf_compose_fields) next to the image gathers of the same shapes on the same
GPU, as the yardstick: run 1, B = 32 fields of 640 x 640 to 640 x 640 (a roll-rectification of a Unified Spherical Model view to a pinhole view) next to
`reproject_image` on float32 images of the same shapes and cameras; run 2, 24 views of 320 x 320 (three rows of eight, 100 degrees) onto a 1024 x 2048
panorama next to `compose_panorama` on float32 images of the same shapes and cameras.  The yardsticks are existing kernels that read 3 floats per tap
from one interleaved image; the transports read 3 floats per tap from three planes, twice (the up sample and the latitude sample), and do the lift,
the rotation and the push per pixel.  Device events around the whole call after a warm-up, alternating in one process; medians of 25 calls."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.getcwd())
from perspectivefields_amd import compose_panorama, compose_panorama_fields, fields_from_params, reproject_fields, reproject_image

CALLS = 25
rng = np.random.default_rng(0)
dev = lambda v: torch.tensor(v, dtype=torch.float64, device="cuda")


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def compare(name, ours, yardstick, yard_name, written):
    for _ in range(3):
        ours()
        yardstick()
    torch.cuda.synchronize()
    t_ours, t_yard = [], []
    for _ in range(CALLS):
        t_ours.append(timed(ours))
        t_yard.append(timed(yardstick))
    lat = ours()[1]
    print(f"{name}: {np.median(t_ours):.3f} ms, {yard_name} {np.median(t_yard):.3f} ms (x{np.median(t_ours) / np.median(t_yard):.2f} of the yardstick); "
          f"{written / 1e6:.1f} MB written per call (HBM write bound at 8 TB/s: {written / 8e12 * 1e3:.4f} ms); valid share {float(torch.isfinite(lat).float().mean()):.3f}",
          flush=True)


# run 1: views -> views
B, H, W = 32, 640, 640
roll, pitch = rng.uniform(-20, 20, B), rng.uniform(-30, 30, B)
focal = 0.5 / np.tan(np.radians(rng.uniform(50, 90, B)) / 2)
src = dict(roll=dev(roll), pitch=dev(pitch), rel_focal=dev(focal), xi=0.5)
dst = dict(roll=0.0, pitch=dev(pitch), rel_focal=dev(focal) * 0.8)
fields = [fields_from_params(float(r), float(p), float(f), height=H, width=W, xi=0.5, device="cuda") for r, p, f in zip(roll, pitch, focal)]
up, lat = torch.stack([u for u, _ in fields]), torch.stack([l for _, l in fields])
images = torch.rand((B, H, W, 3), dtype=torch.float32, device="cuda")
compare(f"reproject_fields, {B} x {H} x {W} -> {H} x {W}", lambda: reproject_fields(up, lat, src, dst), lambda: reproject_image(images, src, dst), "reproject_image (float32)",
        B * H * W * 3 * 4)

# run 2: views -> panorama
n_yaw, pitches, size, Hp, Wp = 8, (-45.0, 0.0, 45.0), 320, 1024, 2048
f100 = 0.5 / np.tan(np.radians(50.0))
cams = dict(roll=0.0, pitch=[p for p in pitches for _ in range(n_yaw)], yaw=[k * 360.0 / n_yaw for _ in pitches for k in range(n_yaw)], rel_focal=f100)
fields = [fields_from_params(0.0, p, f100, height=size, width=size, device="cuda") for p in cams["pitch"]]
ups, lats = [u for u, _ in fields], [l for _, l in fields]
views = torch.rand((len(ups), size, size, 3), dtype=torch.float32, device="cuda")
compare(f"compose_panorama_fields, {len(ups)} x {size} x {size} -> {Hp} x {Wp}", lambda: compose_panorama_fields(ups, lats, cams, height=Hp, width=Wp),
        lambda: compose_panorama(views, cams, height=Hp, width=Wp), "compose_panorama (float32)", Hp * Wp * 3 * 4)
