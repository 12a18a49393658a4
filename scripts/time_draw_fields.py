"""Time of the drawing of perspective fields (draw_fields.hip, pf_draw_fields, draw_perspective_fields) on the GPU: B = 32 uint8 images of
480 x 640 with the fields of a synthetic camera, default arguments (tint, iso-latitude lines every 10 degrees, 10 x 13 arrows of 32 pixels).
The yardstick is NOT the same drawing: it is the tint alone in PyTorch -- the colour ramp by torch ops on the latitude, `lerp` with the image, the
conversion back to uint8 -- on the same batch, which shows what the plain memory traffic of such a pass costs in torch.  Both are timed with device
events around the whole call after a warm-up, alternating in one process; medians of 25 calls.  The bytes a call must move (image in, image out,
three field planes in) are set against the HBM peak.
`--kernel-only N` runs N draw_perspective_fields calls and nothing else: the process of a separate `rocprofv3 --kernel-trace --stats` run."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.getcwd())
from perspectivefields_amd import draw_perspective_fields, fields_from_params

B, H, W, CALLS = 32, 480, 640, 25
HBM_PEAK = 8.0e12   # bytes per second, MI355X
RAMP = torch.tensor([[33, 102, 172], [146, 197, 222], [247, 247, 247], [244, 165, 130], [178, 24, 43]], dtype=torch.float32, device="cuda")


def torch_tint(imgs, lat, alpha=0.5):
    t = ((lat + 90.0) / 45.0).clamp(0.0, 4.0)
    i = t.floor().clamp(max=3.0)
    f = (t - i).unsqueeze(-1)
    i = i.long()
    c = torch.lerp(RAMP[i], RAMP[i + 1], f)
    return torch.lerp(imgs.to(torch.float32), c, alpha).add_(0.5).floor_().clamp_(0.0, 255.0).to(torch.uint8)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


g = torch.Generator(device="cuda").manual_seed(0)
imgs = torch.randint(0, 256, (B, H, W, 3), dtype=torch.uint8, device="cuda", generator=g)
fields = [fields_from_params(-20.0 + 1.3 * k, -15.0 + 1.1 * k, 0.87, height=H, width=W) for k in range(B)]
up, lat = torch.stack([f[0] for f in fields]), torch.stack([f[1] for f in fields])
out = torch.empty_like(imgs)
ours = lambda: draw_perspective_fields(imgs, up, lat, out=out)
if "--kernel-only" in sys.argv:
    for _ in range(int(sys.argv[sys.argv.index("--kernel-only") + 1])):
        ours()
    torch.cuda.synchronize()
    sys.exit(0)
theirs = lambda: torch_tint(imgs, lat)
for _ in range(3):
    ours()
    theirs()
torch.cuda.synchronize()
t_ours, t_torch = [], []
for _ in range(CALLS):
    t_ours.append(timed(ours))
    t_torch.append(timed(theirs))
tint_only = draw_perspective_fields(imgs, up, lat, draw_up=False, lat_step_deg=1e6, line_width=0.0)   # no level but 0: only the horizon line differs
diff = (tint_only.to(torch.int16) - torch_tint(imgs, lat).to(torch.int16)).abs()
moved = B * H * W * (3 + 3 + 12)
ms = float(np.median(t_ours))
print(f"{B} uint8 images of {H} x {W}: draw_perspective_fields {ms:.3f} ms ({min(t_ours):.3f} - {max(t_ours):.3f}), {ms / B * 1e3:.1f} us per image, "
      f"{B / ms * 1e3:.0f} images/s; {moved / 1e6:.1f} MB to move, {moved / (ms * 1e-3) / 1e12:.2f} TB/s, {100 * moved / (ms * 1e-3) / HBM_PEAK:.1f} % of the HBM peak; "
      f"torch tint alone {np.median(t_torch):.3f} ms ({min(t_torch):.3f} - {max(t_torch):.3f}), x{np.median(t_torch) / ms:.1f}; "
      f"tint-only pictures differ from torch's by more than 1 on {float((diff > 1).float().mean()) * 100:.2f} % of the values (the horizon line)", flush=True)
