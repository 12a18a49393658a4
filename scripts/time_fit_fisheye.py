"""Time of the fisheye lens fit (fit_camera_fisheye.hip, pf_fit_fisheye) next to the Unified Spherical Model fit: 32 noisy synthetic equidistant fisheye
fields of fov 180 degrees at 640 x 640 for the four free sets of the lens fit, 32 noisy USM fields of the same size for the 4- and 6-parameter USM
fits; the six alternate in one process, device events around the whole call after a warm-up, medians of 10.  Under
`rocprofv3 --kernel-trace --stats -- python scripts/time_fit_fisheye.py` the kernel table gives the per-iteration accumulate and solve times."""
import os, sys, torch, numpy as np
sys.path.insert(0, os.getcwd())
from perspectivefields_amd import fisheye_fields, fisheye_lens, fit_camera_params, fit_fisheye_lens
from tests.test_fit_camera_usm_ref import focal_of, usm_fields

B, H, W = 32, 640, 640
ROUNDS = 10
rng = np.random.default_rng(0)
g = torch.Generator(device="cuda").manual_seed(0)
rows = [fisheye_lens(180.0, radius=rng.uniform(0.45, 0.5) * H, center=(W / 2 + rng.uniform(-8, 8), H / 2 + rng.uniform(-8, 8)), k=(rng.uniform(-0.02, 0.02), 0.0, 0.0, 0.0),
                     roll=rng.uniform(-30, 30), pitch=rng.uniform(-40, 40))[None] for _ in range(B)]
fu, fl = fisheye_fields(rows, height=H, width=W)
fu = fu + 0.01 * torch.randn(fu.shape, device="cuda", generator=g)   # noisy input: the fit runs its iterations instead of converging at once
fl = fl + 1.0 * torch.randn(fl.shape, device="cuda", generator=g)
f_ups, f_lats = list(fu), list(fl)
u_ups, u_lats = [], []
for k in range(B):
    xi = (0.0, 0.3, 0.6, 1.0)[k % 4]
    th = (np.radians(rng.uniform(-30, 30)), np.radians(rng.uniform(-40, 40)), focal_of(rng.uniform(50, 110), xi), 0.0, 0.0, xi)
    up, lat = usm_fields(th, H, W)
    u_ups.append(torch.from_numpy(up + rng.normal(0, 0.01, up.shape)).float().cuda())
    u_lats.append(torch.from_numpy(lat + rng.normal(0, 1.0, lat.shape)).float().cuda())
usm = lambda **kw: (lambda: fit_camera_params(u_ups, u_lats, distortion=True, **kw))
fish = lambda **kw: (lambda: fit_fisheye_lens(f_ups, f_lats, max_fov=200.0, **kw))
kinds = [("USM 4", usm(free_principal_point=False)), ("fisheye 3", fish()), ("fisheye 5 (k1, k2)", fish(distortion=True)),
         ("USM 6", usm(free_principal_point=True)), ("fisheye 5 (cx, cy)", fish(free_principal_point=True)), ("fisheye 7", fish(free_principal_point=True, distortion=True))]
for _, fn in kinds:
    for _ in range(2):
        fn()
torch.cuda.synchronize()
ms = {name: [] for name, _ in kinds}
last = {}
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
for _ in range(ROUNDS):
    for name, fn in kinds:
        e0.record()
        last[name] = fn()
        e1.record()
        torch.cuda.synchronize()
        ms[name].append(e0.elapsed_time(e1))
med = {name: sorted(v)[len(v) // 2] for name, v in ms.items()}
for name, _ in kinds:
    its = [int(d["fit_iterations"]) for d in last[name]]
    conv = sum(bool(d["fit_converged"]) for d in last[name])
    valid = np.mean([int(d["fit_valid_pixels"]) for d in last[name]]) / (H * W)
    ref = med["USM 4" if name in ("USM 4", "fisheye 3", "fisheye 5 (k1, k2)") else "USM 6"]
    print(f"{name}: B={B} {H}x{W}: median {med[name]:.3f} ms per batch (min {min(ms[name]):.3f}), {med[name] / ref:.2f} x the USM fit beside it; "
          f"LM steps max {max(its)}, mean {np.mean(its):.1f}, converged {conv}/{B}, valid pixels {valid:.2f} of the frame")
