"""Time of the camera fit with shared intrinsics (fit_lm.h, pf_fit_camera_shared) on 32 frames of one camera at 640 x 640 as ONE group, alternating in
the same process with the per-image fit (pf_fit_camera) on the same fields: device events around the whole call after a warm-up, medians, and the
numbers of LM steps each used.  The two run the same accumulate kernel once per step; they differ in the steps they take and in the solve."""
import os, sys, torch, numpy as np
sys.path.insert(0, os.getcwd())
from perspectivefields_amd import fit_camera_params, fit_camera_shared
from tests.test_fit_camera_ref import model_fields

B, H, W = 32, 640, 640
rng = np.random.default_rng(0)
f = 0.5 / np.tan(np.radians(70.0) / 2)
ups, lats = [], []
for k in range(B):
    th = (np.radians(rng.uniform(-30, 30)), np.radians(rng.uniform(-40, 40)), f, 0.0, 0.0)
    up, lat = model_fields(th, H, W)
    up = up + rng.normal(0, 0.01, up.shape)   # noisy input: the fit runs its iterations instead of converging at once
    lat = lat + rng.normal(0, 1.0, lat.shape)
    ups.append(torch.from_numpy(up).float().cuda())
    lats.append(torch.from_numpy(lat).float().cuda())
for free_pp, np_ in ((False, 3), (True, 5)):
    runs = {"shared": lambda: fit_camera_shared(ups, lats, free_principal_point=free_pp), "per image": lambda: fit_camera_params(ups, lats, free_principal_point=free_pp)}
    for _ in range(2):
        for fn in runs.values():
            fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms, res = {k: [] for k in runs}, {}
    for _ in range(10):   # alternating: both see the same clocks
        for k, fn in runs.items():
            e0.record()
            res[k] = fn()
            e1.record()
            torch.cuda.synchronize()
            ms[k].append(e0.elapsed_time(e1))
    for k in runs:
        its = [int(d["fit_iterations"]) for d in res[k]]
        conv = sum(bool(d["fit_converged"]) for d in res[k])
        fs = [float(d["pred_rel_focal"]) for d in res[k]]
        print(f"{np_} parameters, {k:9s}: B={B} {H}x{W}: median {sorted(ms[k])[len(ms[k]) // 2]:.3f} ms per batch (min {min(ms[k]):.3f}); LM steps used max {max(its)}, "
              f"mean {np.mean(its):.1f}, converged {conv}/{B}; |log(f / f_true)| max {max(abs(np.log(v / f)) for v in fs):.2e}")
