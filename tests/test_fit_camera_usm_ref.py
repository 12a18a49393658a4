"""fp64 numpy reference of the Unified Spherical Model camera fit (include/pf_hip.h pf_fit_camera_usm): the
objective over tests.test_pano_crop_ref.labels, the blind start of the kernel, a proof that the inputs of the GPU round-trip test
are recoverable by the reference alone, and the host-side contract of the new entry points (no GPU needed).
tests/test_gpu_fit_camera_usm.py uses the same reference on the GPU results."""
import ctypes
import itertools
import os
import re

import numpy as np
import pytest
import torch

from tests.test_fit_camera_ref import CASES, model_fields, rho
from tests.test_pano_crop_ref import labels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R2D = 180.0 / np.pi

# the grid of the GPU round-trip test
ROLLS = (-30.0, -5.0, 0.0, 12.0, 40.0)
PITCHES = (-70.0, -20.0, 0.0, 0.5, 35.0, 70.0)
XIS = (0.0, 0.25, 0.6, 1.0)
VFOVS = (55.0, 90.0, 120.0)
SIZES = ((640, 640), (384, 512), (97, 131))


def focal_of(vfov_deg, xi):
    """rel_focal whose centre magnification f / (1 + xi) is that of a pinhole of this vertical FoV"""
    return (1.0 + xi) * 0.5 / np.tan(np.radians(vfov_deg) / 2)


GRID = [(r, p, focal_of(v, xi), 0.0, 0.0, xi) for r, p, xi, v in itertools.product(ROLLS, PITCHES, XIS, VFOVS)]


def usm_fields(theta, H, W):
    """theta = (roll, pitch [rad], rel_focal, rel_cx, rel_cy, xi) -> up (2, H, W), latitude (H, W) degrees in fp64, NaN without a ray"""
    r, p, f, cx, cy, xi = (float(v) for v in theta)
    return labels((r, p, 0.0, f, cx, cy, xi), H, W)


def usm_residuals(theta, up_pred, lat_pred):
    """r_up (2, N) chordal in degree scale, r_lat (N,) degrees, over the pixels with finite input and a ray at both of their points"""
    H, W = lat_pred.shape
    up, lat = usm_fields(theta, H, W)
    ok = np.isfinite(up_pred).all(0) & np.isfinite(lat_pred) & np.isfinite(up).all(0) & np.isfinite(lat)
    return (up[:, ok] - up_pred[:, ok].astype(np.float64)) * R2D, lat[ok] - lat_pred[ok].astype(np.float64)


def usm_cost(theta, up_pred, lat_pred, loss="l2", delta=2.0, weights=(1.0, 1.0)):
    ru, rl = usm_residuals(theta, up_pred, lat_pred)
    return float(weights[0] * rho(np.sqrt((ru * ru).sum(0)), loss, delta).sum() + weights[1] * rho(rl, loss, delta).sum())


def usm_valid_pixels(theta, up_pred, lat_pred):
    return usm_residuals(theta, up_pred, lat_pred)[1].size


def usm_l2_residual_vector(theta, up_pred, lat_pred):
    """the L2 objective as scipy.optimize.least_squares sees it: cost = 0.5 * |this|^2 (while the set of pixels with a ray stays the same)"""
    ru, rl = usm_residuals(theta, up_pred, lat_pred)
    return np.concatenate([ru.ravel(), rl])


def blind_start(up, lat):
    """the start of pf_fit_camera_usm without d_init: roll / pitch from the 4 x 4 centre pixels, xi = 0, f = the best of 16 vFoV candidates in
    [15, 150] deg by the cost on a 32 x 32 subsample"""
    H, W = lat.shape
    rows, cols = np.arange(H // 2 - 2, H // 2 + 2), np.arange(W // 2 - 2, W // 2 + 2)
    u = up[:, rows][:, :, cols]
    roll = np.arctan2(-u[0].sum(), -u[1].sum())
    pitch = np.radians(lat[rows][:, cols].mean())
    pitch = min(max(pitch, -np.radians(89.9)), np.radians(89.9))
    s = np.arange(32)
    sr = np.minimum(((s + 0.5) * H / 32).astype(int), H - 1)
    sc = np.minimum(((s + 0.5) * W / 32).astype(int), W - 1)
    best = (np.inf, 1.0)
    for c in range(16):
        f = 0.5 / np.tan(0.5 * np.radians(15.0 + 9.0 * c))
        mu, ml = usm_fields((roll, pitch, f, 0.0, 0.0, 0.0), H, W)
        ru = (mu[:, sr][:, :, sc] - up[:, sr][:, :, sc]) * R2D
        rl = ml[sr][:, sc] - lat[sr][:, sc]
        cost = 0.5 * np.nansum(ru * ru) + 0.5 * np.nansum(rl * rl)
        if cost < best[0]:
            best = (cost, f)
    return np.array([roll, pitch, best[1], 0.0, 0.0, 0.0])


def reference_fit(up, lat, start, free=(0, 1, 2, 5)):
    """scipy's Levenberg-Marquardt on the fp64 reference over the free parameters of theta, from `start`"""
    from scipy.optimize import least_squares

    free = list(free)
    th0 = np.array(start, dtype=np.float64)

    def fun(t):
        th = th0.copy()
        th[free] = t
        return usm_l2_residual_vector(th, up, lat)

    scale = np.ones(len(free))
    scale[free.index(2)] = max(th0[2], 1e-3)
    s = least_squares(fun, th0[free], method="lm", x_scale=scale, xtol=1e-15, ftol=1e-15, gtol=1e-15, max_nfev=400)
    th = th0.copy()
    th[free] = s.x
    return th, s


@pytest.mark.parametrize("case", CASES)
def test_reference_usm_fields_at_xi_0_are_the_pinhole_model(case):
    roll, pitch, f, cx, cy, H, W = case
    up, lat = usm_fields((np.radians(roll), np.radians(pitch), f, cx, cy, 0.0), H, W)
    up_p, lat_p = model_fields((np.radians(roll), np.radians(pitch), f, cx, cy), H, W)
    assert np.abs(up - up_p).max() <= 1e-9
    assert np.abs(lat - lat_p).max() <= 1e-9


def _recovered(cases, H, W):
    bad = []
    for r, p, f, cx, cy, xi in cases:
        truth = np.array([np.radians(r), np.radians(p), f, cx, cy, xi])
        up, lat = usm_fields(truth, H, W)
        assert np.isfinite(up).all() and np.isfinite(lat).all()   # no pixel of the grid lacks a ray
        th, s = reference_fit(up, lat, blind_start(up, lat))
        err = np.abs(th - truth)
        if err.max() > 1e-6:
            bad.append(((r, p, f, xi), err, s.nfev))
    return bad


@pytest.mark.parametrize("xi", XIS)
def test_reference_recovers_the_round_trip_grid_from_the_blind_start(xi):
    """Every (roll, pitch, xi, vFoV) of the GPU round-trip grid, at 97 x 131: the reference alone, from the kernel's blind start, ends within
    1e-6 of the truth in every parameter.  (The two larger sizes of the GPU test differ in sampling density only; a sample of the grid at
    them is below, the whole grid there would take the reference half an hour.)"""
    bad = _recovered([c for c in GRID if c[5] == xi], 97, 131)
    assert not bad, bad[:6]


@pytest.mark.parametrize("H,W", SIZES[:2])
def test_reference_recovers_a_sample_of_the_grid_at_the_larger_sizes(H, W):
    rng = np.random.default_rng(H + W)
    cases = [GRID[k] for k in rng.choice(len(GRID), 3, replace=False)]
    cases += [c for c in GRID if (c[0], c[1]) == (40.0, 70.0) and c[5] == 1.0][:1]
    bad = _recovered(cases, H, W)
    assert not bad, bad


def test_usm_output_columns_match_the_header():
    """the Python dict keys follow the PF_USMFIT_COL_* order of include/pf_hip.h: the thirteen pf_fit_camera columns, then xi"""
    from perspectivefields_amd.perspectivefields import _FIT_COLS, _USMFIT_COLS

    hdr = open(os.path.join(ROOT, "include", "pf_hip.h")).read()
    cols = {m[0]: int(m[1]) for m in re.findall(r"#define PF_USMFIT_COL_([A-Z_]+) (\d+)", hdr)}
    pin = {m[0]: int(m[1]) for m in re.findall(r"#define PF_FIT_COL_([A-Z_]+) (\d+)", hdr)}
    assert int(re.search(r"#define PF_USMFIT_COLS (\d+)", hdr)[1]) == len(_USMFIT_COLS) == len(cols) == 14
    assert {k: v for k, v in cols.items() if k != "XI"} == pin and cols["XI"] == 13
    assert _USMFIT_COLS == _FIT_COLS + ("pred_xi",)


def test_new_symbols_are_in_the_library_with_the_declared_prototypes():
    from perspectivefields_amd.engine import _SIGNATURES, load_library

    lib = load_library()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pf_hip.h")).read(), flags=re.S)
    ctype = {"int": ctypes.c_int, "float": ctypes.c_float, "size_t": ctypes.c_size_t}
    for name in ("pf_fit_camera_usm_workspace_bytes", "pf_fit_camera_usm", "pf_fields_from_params_usm"):
        m = re.search(r"(\w+)\s+" + name + r"\(([^;]*)\);", hdr)
        assert m, name
        args = [a.strip() for a in m[2].split(",")]
        want = [ctypes.c_void_p if "*" in a else ctype[a.split()[0]] for a in args]
        res, got = _SIGNATURES[name]
        assert res is ctype[m[1]] and got == want, (name, got, want)
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == want
    # the USM fit takes the arguments of the pinhole fit
    assert _SIGNATURES["pf_fit_camera_usm"] == _SIGNATURES["pf_fit_camera"]


def test_usm_fit_workspace_size_and_small_images():
    from perspectivefields_amd.engine import load_library

    lib = load_library()
    hw = lambda *s: (ctypes.c_int32 * len(s))(*s)
    one = lib.pf_fit_camera_usm_workspace_bytes(1, hw(640, 640))
    two = lib.pf_fit_camera_usm_workspace_bytes(2, hw(640, 640, 97, 131))
    assert 0 < one < two
    assert one > lib.pf_fit_camera_workspace_bytes(1, hw(640, 640))   # larger records and state than the pinhole fit
    assert lib.pf_fit_camera_usm_workspace_bytes(1, hw(7, 640)) == 0
    assert lib.pf_fit_camera_usm_workspace_bytes(2, hw(640, 640, 8, 7)) == 0
    assert lib.pf_fit_camera_usm_workspace_bytes(0, hw(640, 640)) == 0


def test_distortion_fit_on_cpu_tensors_raises():
    from perspectivefields_amd import fit_camera_params
    from perspectivefields_amd.engine import PfError

    up, lat = usm_fields((0.1, 0.2, 0.9, 0.0, 0.0, 0.4), 16, 16)
    with pytest.raises(PfError):
        fit_camera_params(torch.from_numpy(up).float(), torch.from_numpy(lat).float(), distortion=True)
    with pytest.raises(PfError):
        fit_camera_params([torch.from_numpy(up).float()], [torch.from_numpy(lat).float()], distortion=True, free_principal_point=True)


def test_usm_fields_on_the_cpu_raise():
    from perspectivefields_amd import fields_from_params
    from perspectivefields_amd.engine import PfError

    with pytest.raises(PfError):
        fields_from_params(5.0, 10.0, 0.8, height=16, width=16, device="cpu", xi=0.4)
    with pytest.raises(PfError):
        fields_from_params(5.0, 10.0, 0.8, height=16, width=16, device="cpu", xi=torch.tensor(0.0))   # a tensor xi is the USM path, whatever it holds


def test_usm_entry_points_reject_bad_arguments_before_device_work():
    from perspectivefields_amd.engine import load_library

    lib = load_library()
    hw = lambda *s: (ctypes.c_int32 * len(s))(*s)
    ptrs = lambda *p: (ctypes.c_void_p * len(p))(*p)
    dev = ctypes.c_void_p(256)

    def fit(B=1, hw_=None, up=None, lat=None, free_pp=0, loss=0, delta=2.0, w=(1.0, 1.0), max_iter=20, out=dev, ws=dev, ws_n=1 << 30):
        rc = lib.pf_fit_camera_usm(0, B, hw_ or hw(16, 16), up or ptrs(256), lat or ptrs(256), None, free_pp, loss, delta, w[0], w[1], max_iter, out, ws,
                                   ws_n, None)
        return rc, lib.pf_last_error(None).decode()

    for kw, what in ((dict(B=0), "bad argument"), (dict(out=None), "bad argument"), (dict(free_pp=2), "bad option"), (dict(loss=3), "bad option"),
                     (dict(max_iter=0), "bad option"), (dict(w=(0.0, 0.0)), "weights"), (dict(w=(-1.0, 1.0)), "weights"),
                     (dict(loss=1, delta=0.0), "huber_delta_deg"), (dict(hw_=hw(7, 16)), "smaller than 8 x 8"), (dict(up=ptrs(None)), "NULL field pointer")):
        rc, msg = fit(**kw)
        assert rc == -1 and what in msg and msg.startswith("pf_fit_camera_usm"), (kw, rc, msg)
    rc, msg = fit(ws_n=16)
    assert rc == -4 and "workspace" in msg, (rc, msg)
    for args in ((None, 8, 8, dev, dev), (dev, 0, 8, dev, dev), (dev, 8, 8, None, dev), (dev, 8, 8, dev, None)):
        rc = lib.pf_fields_from_params_usm(0, args[0], args[1], args[2], args[3], args[4], None)
        assert rc == -1 and "pf_fields_from_params_usm" in lib.pf_last_error(None).decode(), args


def test_new_kernels_are_in_the_library_without_scratch():
    """scripts/kernel_resources.py on the built library: the USM kernels are there for gfx950, with no spilled register and no scratch, and
    the pinhole kernels next to them are as they were"""
    import importlib.util
    import shutil

    if not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf") or not shutil.which("c++filt"):
        pytest.skip("llvm-readelf / c++filt not available")
    from perspectivefields_amd import build as _b

    lib = _b.build(verbose=False)
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "scripts", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    by = {r["kernel"]: r for r in kr.kernels(lib)}
    for k in ("pf::fit_init_kernel<pf::UsmFit>", "pf::fit_accum_kernel<pf::UsmFit, 4>", "pf::fit_accum_kernel<pf::UsmFit, 6>", "pf::fit_solve_kernel<pf::UsmFit, 4>",
              "pf::fit_solve_kernel<pf::UsmFit, 6>", "pf::fields_usm_kernel", "pf::fit_accum_kernel<pf::PinholeFit, 3>", "pf::fit_accum_kernel<pf::PinholeFit, 5>",
              "pf::fit_init_kernel<pf::PinholeFit>", "pf::fit_solve_kernel<pf::PinholeFit, 3>", "pf::fit_solve_kernel<pf::PinholeFit, 5>"):
        assert k in by, k
        assert by[k]["spill"] == 0 and by[k]["scratch"] == 0, by[k]
    assert kr.blocks_per_cu(by["pf::fit_accum_kernel<pf::UsmFit, 6>"]) >= 3   # no worse than the 5-parameter pinhole kernel
