"""Time of the camera fit (fit_camera.hip, pf_fit_camera) on a batch of 32 fields at 640 x 640, 3 and 5 parameters: device events
around the whole call after a warm-up, plus the bytes and FLOPs of one iteration computed from the shapes."""
import os, sys, torch, numpy as np
sys.path.insert(0, os.getcwd())
from perspectivefields_amd import fit_camera_params
from tests.test_fit_camera_ref import model_fields

B, H, W = 32, 640, 640
rng = np.random.default_rng(0)
ups, lats = [], []
for k in range(B):
    th = (np.radians(rng.uniform(-30, 30)), np.radians(rng.uniform(-40, 40)), 0.5 / np.tan(np.radians(rng.uniform(30, 110)) / 2), 0.0, 0.0)
    up, lat = model_fields(th, H, W)
    up = up + rng.normal(0, 0.01, up.shape)   # noisy input: the fit runs its iterations instead of converging at once
    lat = lat + rng.normal(0, 1.0, lat.shape)
    ups.append(torch.from_numpy(up).float().cuda())
    lats.append(torch.from_numpy(lat).float().cuda())
px = B * H * W
for free_pp, np_ in ((False, 3), (True, 5)):
    for _ in range(2):
        fit_camera_params(ups, lats, free_principal_point=free_pp)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = []
    for _ in range(10):
        e0.record()
        res = fit_camera_params(ups, lats, free_principal_point=free_pp)
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    its = [int(d["fit_iterations"]) for d in res]
    conv = sum(bool(d["fit_converged"]) for d in res)
    # per pixel and iteration: 12 bytes of fields read; model + Jacobian + normal-equation update (counted per VALU op of the source:
    # ~60 + 30 NP for the model and its duals, NP (NP + 1) / 2 * 3 + NP * 3 for the accumulation)
    flops = 60 + 30 * np_ + 3 * np_ * (np_ + 1) // 2 + 3 * np_
    print(f"{np_} parameters: B={B} {H}x{W}: {min(ms):.3f} ms per batch (median {sorted(ms)[len(ms) // 2]:.3f}); LM steps used max {max(its)}, "
          f"mean {np.mean(its):.1f}, converged {conv}/{B}; per iteration {px * 12 / 1e6:.1f} MB read, {px * flops / 1e9:.2f} GFLOP")
