"""fp64 numpy statement of the camera fit with intrinsics shared across the frames of one camera (include/pf_hip.h pf_fit_camera_shared,
DESIGN.md section 16): the block-arrow Levenberg-Marquardt step over the residuals of tests/test_fit_camera_ref.py and
tests/test_fit_camera_usm_ref.py, a proof on the CPU alone that the inputs of tests/test_gpu_fit_camera_shared.py are recoverable by it,
its agreement with scipy on noisy input, and the host-side contract of the entry points (no GPU needed)."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest
import torch

from tests.test_fit_camera_ref import model_fields, residuals, rho
from tests.test_fit_camera_usm_ref import blind_start, focal_of, usm_fields, usm_residuals

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R2D = 180.0 / np.pi

# the frames of the round-trip group: (roll, pitch) in degrees
POSES = ((-30.0, -70.0), (-5.0, -20.0), (0.0, 0.0), (12.0, 0.5), (40.0, 35.0), (3.0, 70.0), (0.0, 10.0))
VFOVS = (20.0, 55.0, 90.0, 120.0)
XIS = (0.25, 0.6, 1.0)
FIVE = (0.8, 0.08, -0.1)   # f, cx, cy of the 5-parameter case (max_iter=60)
# the seed of the noisy set.  With it, at vFoV 30 and at vFoV 70, the reference's joint |log(f / f_true)| is at most the median of its eight
# single-frame values / 1.5 (asserted below, in fp64)
NOISY_SEED = 0
NOISY_VFOVS = (30.0, 70.0)


def free_index(usm, free_pp):
    """places in theta of the free parameters of one image, in the kernels' theta_of order; the first two are its own, the rest the group's"""
    if usm:
        return [0, 1, 2, 3, 4, 5] if free_pp else [0, 1, 2, 5]
    return [0, 1, 2, 3, 4] if free_pp else [0, 1, 2]


def clamp(th, usm):
    th = th.copy()
    if usm:
        th[0] = np.remainder(th[0] + np.pi, 2 * np.pi) - np.pi
        th[5] = min(max(th[5], -0.5), 2.0)
    th[1] = min(max(th[1], -np.radians(89.9)), np.radians(89.9))
    th[2] = max(th[2], 1e-3)
    return th


def _rows(th, up, lat, usm):
    ru, rl = (usm_residuals if usm else residuals)(th, up, lat)
    return ru, rl


def normal_equations(th, up, lat, idx, usm, loss="l2", delta=2.0, weights=(1.0, 1.0)):
    """J^T W J, J^T W r and the cost of one image at th, the Jacobian by central differences; Huber by IRLS weights as in the kernels"""
    ru, rl = _rows(th, up, lat, usm)
    J = []
    for k in idx:
        h = 1e-6 * max(1.0, abs(th[k]))
        a, b = th.copy(), th.copy()
        a[k] += h
        b[k] -= h
        (ua, la), (ub, lb) = _rows(a, up, lat, usm), _rows(b, up, lat, usm)
        J.append(((ua - ub) / (2 * h), (la - lb) / (2 * h)))
    nu, nl = np.sqrt((ru * ru).sum(0)), np.abs(rl)
    if loss == "l2":
        wu, wl = np.full_like(nu, weights[0]), np.full_like(nl, weights[1])
    else:
        wu = weights[0] * np.where(nu <= delta, 1.0, delta / np.maximum(nu, 1e-300))
        wl = weights[1] * np.where(nl <= delta, 1.0, delta / np.maximum(nl, 1e-300))
    n = len(idx)
    Hm, g = np.zeros((n, n)), np.zeros(n)
    for i in range(n):
        g[i] = (wu * (J[i][0] * ru).sum(0)).sum() + (wl * J[i][1] * rl).sum()
        for j in range(i, n):
            Hm[i, j] = Hm[j, i] = (wu * (J[i][0] * J[j][0]).sum(0)).sum() + (wl * J[i][1] * J[j][1]).sum()
    c = float(weights[0] * rho(nu, loss, delta).sum() + weights[1] * rho(nl, loss, delta).sum())
    return Hm, g, c, rl.size


def image_cost(th, up, lat, usm, loss="l2", delta=2.0, weights=(1.0, 1.0)):
    ru, rl = _rows(np.asarray(th, dtype=np.float64), up, lat, usm)
    return float(weights[0] * rho(np.sqrt((ru * ru).sum(0)), loss, delta).sum() + weights[1] * rho(rl, loss, delta).sum())


def shared_start(ups, lats, usm, starts=None):
    """every image's own start (the kernel's blind one, or the caller's), then the group's f = exp(mean log f) and cx, cy, xi = the means"""
    th = np.array([blind_start(u, l) if starts is None else np.asarray(s, dtype=np.float64) for u, l, s in zip(ups, lats, starts or [None] * len(ups))])
    if not usm:
        th = th[:, :5].copy()
    th[:, 2] = np.exp(np.log(th[:, 2]).mean())
    th[:, 3:] = th[:, 3:].mean(0)
    return np.array([clamp(t, usm) for t in th])


def shared_fit(ups, lats, *, usm=False, free_pp=False, max_iter=20, starts=None, loss="l2", delta=2.0, weights=(1.0, 1.0)):
    """The joint fit of one group.  Returns (theta [n][NTH], group cost, steps evaluated, converged).  An image without a valid pixel keeps its
    start roll and pitch and contributes nothing."""
    idx = free_index(usm, free_pp)
    NS = len(idx) - 2
    cur = shared_start(ups, lats, usm, starts)
    n = len(ups)
    trial = cur.copy()
    lam, cost_c, nev, conv = 1e-3, np.inf, 0, False
    live = None
    HG = [None] * n
    costs = np.zeros(n)
    for _ in range(max_iter + 1):
        ev = [normal_equations(trial[i], ups[i], lats[i], idx, usm, loss, delta, weights) for i in range(n)]
        if nev == 0:
            live = [i for i in range(n) if ev[i][3] > 0 and np.isfinite(ev[i][2])]
            if not live:
                return cur, 0.0, 0, False
        cost_t = sum(ev[i][2] for i in live)
        if nev == 0 or cost_t < cost_c:
            for i in live:
                cur[i] = trial[i]
                HG[i] = ev[i][:2]
                costs[i] = ev[i][2]
            if nev > 0:
                if cost_c - cost_t <= 1e-10 * cost_c:
                    conv = True
                lam = max(lam * 0.1, 1e-12)
            cost_c = cost_t
            if cost_t == 0.0:
                conv = True
        else:
            lam *= 10.0
            if lam > 1e16:
                conv = True
        nev += 1
        if conv:
            break
        # damp the whole block-arrow system, eliminate every image's 2 x 2 block, solve the shared one
        C, S, b = np.zeros((NS, NS)), np.zeros((NS, NS)), np.zeros(NS)
        elim = {}
        for i in live:
            Hm, g = HG[i]
            A = Hm[:2, :2] + lam * np.diag(np.diag(Hm[:2, :2]))
            B = Hm[:2, 2:]
            if not (A[0, 0] > 0.0 and A[0, 0] * A[1, 1] - A[0, 1] * A[0, 1] > 0.0):
                elim = None
                break
            Ai = np.linalg.inv(A)
            C += Hm[2:, 2:]
            S -= B.T @ Ai @ B
            b += g[2:] - B.T @ Ai @ g[:2]
            elim[i] = (Ai, B, g[:2])
        S += C + lam * np.diag(np.diag(C))
        try:
            if elim is None:
                raise np.linalg.LinAlgError
            L = np.linalg.cholesky(S)
        except np.linalg.LinAlgError:   # singular system: the data determine no step
            conv = True
            break
        ds = -np.linalg.solve(L.T, np.linalg.solve(L, b))
        step = 0.0
        for i in live:
            Ai, B, ga = elim[i]
            da = -Ai @ (ga + B @ ds)
            th = cur[i].copy()
            th[idx[:2]] += da
            th[idx[2:]] += ds
            th = clamp(th, usm)
            step = max(step, np.abs(th - cur[i]).max())
            trial[i] = th
        if step < 1e-9:
            conv = True
            break
    for i in set(range(n)) - set(live):   # a frame without a valid pixel follows the group's shared parameters
        cur[i][idx[2:]] = cur[live[0]][idx[2:]]
    return cur, float(cost_c), nev - 1, conv


def _theta(r, p, f, cx=0.0, cy=0.0, xi=None):
    return np.array([np.radians(r), np.radians(p), f, cx, cy] + ([] if xi is None else [xi]))


def round_trip_group(f, cx=0.0, cy=0.0, xi=None, H=48, W=64):
    """the fields of the seven frames of one camera -> ([theta], [up], [lat])"""
    ths = [_theta(r, p, f, cx, cy, xi) for r, p in POSES]
    fl = [(usm_fields if xi is not None else model_fields)(t, H, W) for t in ths]
    return ths, [u for u, _ in fl], [l for _, l in fl]


def _assert_recovered(ths, cur, steps):
    err = max(np.abs(np.array(ths) - cur).max(), 0.0)
    assert err <= 1e-6, (err, steps)
    assert np.ptp(cur[:, 2:], axis=0).max() == 0.0   # one set of shared numbers


@pytest.mark.parametrize("vfov", VFOVS)
def test_reference_recovers_the_pinhole_round_trips_from_the_blind_start(vfov):
    ths, ups, lats = round_trip_group(0.5 / np.tan(np.radians(vfov) / 2))
    cur, c, steps, conv = shared_fit(ups, lats)
    _assert_recovered(ths, cur, steps)


@pytest.mark.parametrize("xi", XIS)
def test_reference_recovers_the_usm_round_trips_from_the_blind_start(xi):
    for vfov in (55.0, 90.0):
        ths, ups, lats = round_trip_group(focal_of(vfov, xi), xi=xi)
        cur, c, steps, conv = shared_fit(ups, lats, usm=True)
        _assert_recovered(ths, cur, steps)


def test_reference_recovers_the_five_parameter_round_trip():
    ths, ups, lats = round_trip_group(*FIVE)
    cur, c, steps, conv = shared_fit(ups, lats, free_pp=True, max_iter=60)
    _assert_recovered(ths, cur, steps)


def noisy_group(vfov, seed=NOISY_SEED, n=8, H=48, W=64):
    """8 frames of one camera with seeded poses in +-20 / +-30 degrees and smooth noise: a seeded 6 x 8 grid of N(0, 3 deg) enlarged by np.kron,
    one on the up angle and one on the latitude -> (f_true, [theta], [up], [lat])"""
    rng = np.random.default_rng(seed)
    f = 0.5 / np.tan(np.radians(vfov) / 2)
    ths, ups, lats = [], [], []
    for _ in range(n):
        th = _theta(rng.uniform(-20.0, 20.0), rng.uniform(-30.0, 30.0), f)
        up, lat = model_fields(th, H, W)
        ang = np.radians(np.kron(rng.normal(0.0, 3.0, (6, 8)), np.ones((H // 6, W // 8))))
        c, s = np.cos(ang), np.sin(ang)
        up = np.stack([c * up[0] - s * up[1], s * up[0] + c * up[1]])
        lat = lat + np.kron(rng.normal(0.0, 3.0, (6, 8)), np.ones((H // 6, W // 8)))
        ths.append(th)
        ups.append(up.astype(np.float32))
        lats.append(lat.astype(np.float32))
    return f, ths, ups, lats


@functools.lru_cache(maxsize=None)
def noisy_reference(vfov):
    """(f_true, ups, lats, joint theta, joint cost, [single-frame f]) of the noisy set at this vFoV, by the reference alone; computed once"""
    f, ths, ups, lats = noisy_group(vfov)
    cur, c, steps, conv = shared_fit(ups, lats, max_iter=60)
    singles = [shared_fit([u], [l], max_iter=60)[0][0, 2] for u, l in zip(ups, lats)]
    return f, ups, lats, cur, c, singles


@pytest.mark.parametrize("vfov", NOISY_VFOVS)
def test_reference_agrees_with_scipy_on_the_noisy_set(vfov):
    from scipy.optimize import least_squares

    f, ups, lats, cur, c, _ = noisy_reference(vfov)
    n = len(ups)

    def fun(t):
        out = []
        for i in range(n):
            ru, rl = residuals((t[2 * i], t[2 * i + 1], t[2 * n], 0.0, 0.0), ups[i], lats[i])
            out += [ru.ravel(), rl]
        return np.concatenate(out)

    t0 = np.concatenate([cur[:, :2].ravel(), [cur[0, 2]]])
    start = shared_start(ups, lats, False)
    s0 = np.concatenate([start[:, :2].ravel(), [start[0, 2]]])
    s = least_squares(fun, s0, method="lm", xtol=1e-15, ftol=1e-15, gtol=1e-15, max_nfev=2000)
    assert abs(c - s.cost) <= 1e-6 * s.cost, (c, s.cost)
    assert abs(0.5 * (fun(t0) ** 2).sum() - c) <= 1e-9 * c


def test_joint_focal_beats_the_single_frame_median_on_the_fixed_seed():
    for vfov in NOISY_VFOVS:
        f, ups, lats, cur, c, singles = noisy_reference(vfov)
        joint = abs(np.log(cur[0, 2] / f))
        med = float(np.median([abs(np.log(s / f)) for s in singles]))
        assert joint <= med / 1.5, (NOISY_SEED, vfov, joint, med)


# ---------------------------------------------------------------- host contract
NEW_SYMBOLS = ("pf_fit_camera_shared_workspace_bytes", "pf_fit_camera_shared")


def test_shared_symbols_are_in_the_library_with_the_declared_prototypes():
    from perspectivefields_amd.engine import _SIGNATURES, load_library

    lib = load_library()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pf_hip.h")).read(), flags=re.S)
    ctype = {"int": ctypes.c_int, "float": ctypes.c_float, "size_t": ctypes.c_size_t}
    for name in NEW_SYMBOLS:
        m = re.search(r"(\w+)\s+" + name + r"\(([^;]*)\);", hdr)
        assert m, name
        args = [a.strip() for a in m[2].split(",")]
        want = [ctypes.c_void_p if "*" in a else ctype[a.split()[0]] for a in args]
        res, got = _SIGNATURES[name]
        assert res is ctype[m[1]] and got == want, (name, got, want)
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == want
    assert len(_SIGNATURES["pf_fit_camera_shared"][1]) == 19


def test_no_new_macro_counts_as_an_output_column():
    hdr = open(os.path.join(ROOT, "include", "pf_hip.h")).read()
    assert len(re.findall(r"#define PF_FIT_COL_([A-Z_]+) (\d+)", hdr)) == 13
    assert len(re.findall(r"#define PF_USMFIT_COL_([A-Z_]+) (\d+)", hdr)) == 14


def _i32(*s):
    return (ctypes.c_int32 * len(s))(*s)


def test_shared_workspace_size():
    from perspectivefields_amd.engine import load_library

    lib = load_library()
    ws = lib.pf_fit_camera_shared_workspace_bytes
    for model in (0, 1):
        one = ws(model, 1, _i32(640, 640), 1, _i32(1))
        two = ws(model, 2, _i32(640, 640, 640, 640), 1, _i32(2))
        split = ws(model, 2, _i32(640, 640, 97, 131), 2, _i32(1, 1))
        assert 0 < one < two and 0 < split
        assert ws(model, 1, _i32(7, 640), 1, _i32(1)) == 0
        assert ws(model, 2, _i32(640, 640, 8, 7), 1, _i32(2)) == 0
        assert ws(model, 0, _i32(640, 640), 1, _i32(1)) == 0
        assert ws(model, -1, _i32(640, 640), 1, _i32(1)) == 0
    assert ws(1, 1, _i32(640, 640), 1, _i32(1)) > ws(0, 1, _i32(640, 640), 1, _i32(1))   # larger records and state
    assert ws(2, 1, _i32(640, 640), 1, _i32(1)) == 0


def test_shared_entry_point_rejects_bad_arguments_before_device_work():
    from perspectivefields_amd.engine import load_library

    lib = load_library()
    ptrs = lambda *p: (ctypes.c_void_p * len(p))(*p)
    dev = ctypes.c_void_p(256)

    def fit(model=0, B=2, hw=None, up=None, lat=None, ng=1, gs=None, free_pp=0, loss=0, delta=2.0, w=(1.0, 1.0), max_iter=20, out=dev, ws=dev,
            ws_n=1 << 30):
        rc = lib.pf_fit_camera_shared(0, model, B, hw or _i32(16, 16, 16, 16), up or ptrs(256, 256), lat or ptrs(256, 256), ng, gs or _i32(2), None,
                                      free_pp, loss, delta, w[0], w[1], max_iter, out, ws, ws_n, None)
        return rc, lib.pf_last_error(None).decode()

    cases = ((dict(B=0), "bad argument"), (dict(out=None), "bad argument"), (dict(model=2), "model"), (dict(model=-1), "model"),
             (dict(free_pp=2), "bad option"), (dict(loss=3), "bad option"), (dict(max_iter=0), "bad option"), (dict(w=(0.0, 0.0)), "weights"),
             (dict(w=(-1.0, 1.0)), "weights"), (dict(loss=1, delta=0.0), "huber_delta_deg"), (dict(hw=_i32(7, 16, 7, 16)), "smaller than 8 x 8"),
             (dict(up=ptrs(256, None)), "NULL field pointer"),
             (dict(ng=0), "group sizes"), (dict(gs=_i32(0)), "group sizes"), (dict(ng=2, gs=_i32(2, 0)), "group sizes"),
             (dict(gs=_i32(3)), "sum to"), (dict(ng=2, gs=_i32(1, 2)), "sum to"), (dict(ng=2, gs=_i32(1, -1)), "group sizes"),
             (dict(hw=_i32(16, 16, 16, 24)), "one size"), (dict(hw=_i32(16, 16, 24, 16)), "one size"))
    for kw, what in cases:
        rc, msg = fit(**kw)
        assert rc == -1 and what in msg and msg.startswith("pf_fit_camera_shared"), (kw, rc, msg)
    # two groups may differ in size
    rc, msg = fit(hw=_i32(16, 16, 16, 24), ng=2, gs=_i32(1, 1), ws_n=16)
    assert rc == -4 and "workspace" in msg, (rc, msg)


def test_fit_camera_shared_on_cpu_tensors_raises():
    from perspectivefields_amd import fit_camera_shared
    from perspectivefields_amd.engine import PfError

    up, lat = model_fields((0.1, 0.2, 0.9, 0.0, 0.0), 16, 16)
    u, l = torch.from_numpy(up).float(), torch.from_numpy(lat).float()
    with pytest.raises(PfError):
        fit_camera_shared([u, u], [l, l])
    with pytest.raises(PfError):
        fit_camera_shared([u, u], [l, l], groups=["a", "b"], distortion=True, free_principal_point=True)


def test_fit_camera_shared_names_the_group_of_mixed_sizes():
    """the shapes are checked before the device: a group of unequal sizes is a ValueError that names it, on any tensors"""
    from perspectivefields_amd import fit_camera_shared

    def pair(H, W):
        return torch.zeros(2, H, W), torch.zeros(H, W)

    (u0, l0), (u1, l1) = pair(16, 16), pair(16, 24)
    with pytest.raises(ValueError, match="'cam-b'"):
        fit_camera_shared([u0, u1, u0, u0], [l0, l1, l0, l0], groups=["cam-a", "cam-b", "cam-a", "cam-b"])
    with pytest.raises(ValueError, match="group"):
        fit_camera_shared([u0, u1], [l0, l1])
    with pytest.raises(ValueError):
        fit_camera_shared([u0, u0], [l0, l0], groups=["a"])


def test_shared_kernels_are_in_the_library_without_scratch():
    """scripts/kernel_resources.py on the built library: the kernels of the shared fit are there for gfx950 with no spilled register and no
    scratch, and the eleven per-image fit kernels next to them are still there"""
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
    new = ["pf::fit_shared_start_kernel<pf::PinholeFit>", "pf::fit_shared_start_kernel<pf::UsmFit>"]
    for fit, nps in (("pf::PinholeFit", (3, 5)), ("pf::UsmFit", (4, 6))):
        for np_ in nps:
            new += [f"pf::fit_shared_reduce_kernel<{fit}, {np_}>", f"pf::fit_shared_solve_kernel<{fit}, {np_}>"]
    old = ["pf::fit_init_kernel<pf::UsmFit>", "pf::fit_accum_kernel<pf::UsmFit, 4>", "pf::fit_accum_kernel<pf::UsmFit, 6>", "pf::fit_solve_kernel<pf::UsmFit, 4>",
           "pf::fit_solve_kernel<pf::UsmFit, 6>", "pf::fields_usm_kernel", "pf::fit_accum_kernel<pf::PinholeFit, 3>", "pf::fit_accum_kernel<pf::PinholeFit, 5>",
           "pf::fit_init_kernel<pf::PinholeFit>", "pf::fit_solve_kernel<pf::PinholeFit, 3>", "pf::fit_solve_kernel<pf::PinholeFit, 5>"]
    for k in new + old:
        assert k in by, k
        assert by[k]["spill"] == 0 and by[k]["scratch"] == 0, by[k]
