"""Time of the Unified Spherical Model camera fit (fit_camera_usm.hip, pf_fit_camera_usm) next to the pinhole fit on the same batch of
32 noisy synthetic fields at 640 x 640: the 3- and 5-parameter pinhole fits and the 4- and 6-parameter USM fits alternate in one process,
device events around the whole call after a warm-up.  Under `rocprofv3 --kernel-trace --stats -- python scripts/time_fit_camera_usm.py`
the kernel table gives the per-iteration accumulate and solve times."""
import os, sys, torch, numpy as np
sys.path.insert(0, os.getcwd())
from perspectivefields_amd import fit_camera_params
from tests.test_fit_camera_usm_ref import focal_of, usm_fields

B, H, W = 32, 640, 640
ROUNDS = 10
rng = np.random.default_rng(0)
ups, lats = [], []
for k in range(B):
    xi = (0.0, 0.3, 0.6, 1.0)[k % 4]
    th = (np.radians(rng.uniform(-30, 30)), np.radians(rng.uniform(-40, 40)), focal_of(rng.uniform(50, 110), xi), 0.0, 0.0, xi)
    up, lat = usm_fields(th, H, W)
    up = up + rng.normal(0, 0.01, up.shape)   # noisy input: the fit runs its iterations instead of converging at once
    lat = lat + rng.normal(0, 1.0, lat.shape)
    ups.append(torch.from_numpy(up).float().cuda())
    lats.append(torch.from_numpy(lat).float().cuda())
kinds = [("pinhole 3", dict(distortion=False, free_principal_point=False)), ("USM 4", dict(distortion=True, free_principal_point=False)),
         ("pinhole 5", dict(distortion=False, free_principal_point=True)), ("USM 6", dict(distortion=True, free_principal_point=True))]
for _, kw in kinds:
    for _ in range(2):
        fit_camera_params(ups, lats, **kw)
torch.cuda.synchronize()
ms = {name: [] for name, _ in kinds}
last = {}
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
for _ in range(ROUNDS):
    for name, kw in kinds:
        e0.record()
        last[name] = fit_camera_params(ups, lats, **kw)
        e1.record()
        torch.cuda.synchronize()
        ms[name].append(e0.elapsed_time(e1))
med = {name: sorted(v)[len(v) // 2] for name, v in ms.items()}
for name, _ in kinds:
    its = [int(d["fit_iterations"]) for d in last[name]]
    conv = sum(bool(d["fit_converged"]) for d in last[name])
    ref = med["pinhole 3" if name.endswith(("3", "4")) else "pinhole 5"]
    print(f"{name} parameters: B={B} {H}x{W}: median {med[name]:.3f} ms per batch (min {min(ms[name]):.3f}), {med[name] / ref:.2f} x the pinhole fit; "
          f"LM steps max {max(its)}, mean {np.mean(its):.1f}, converged {conv}/{B}")
