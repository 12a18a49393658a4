"""fp64 numpy statement of the composition of camera views into equirectangular panoramas (include/pf_hip.h pf_pano_compose, DESIGN.md
section 19), built on the camera model of tests/test_pano_crop_ref.py and tests/test_reproject_ref.py: the panorama pixel's direction, the
view's coordinates, coverage, the feather weight, the blend; checks of that reference against itself and against the panorama crop's
conventions; the same formulas in numpy float32 (the rounding floor the GPU weights are measured against); the fixed inputs of
tests/test_gpu_pano_compose.py with the shares that test leaves out; plus the host-side contract of compose_panorama / pf_pano_compose
(no GPU needed)."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

from tests.test_pano_crop_ref import intrinsics, project, rotation, sample_coords, unproject
from tests.test_reproject_ref import FakeCuda, sample, theta_rad, yaw_matrix, z_min

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FEATHER, MEAN = "feather", "mean"


def pano_directions(Hp, Wp):
    """world unit vectors D (Hp, Wp, 3) of the panorama's pixel centres: the inverse of the panorama crop's step from ray to pixel"""
    lon = ((np.arange(Wp) + 0.5) / Wp - 0.5) * 2 * np.pi
    lat = (0.5 - (np.arange(Hp) + 0.5) / Hp) * np.pi
    lat, lon = np.meshgrid(lat, lon, indexing="ij")
    return np.stack([np.cos(lat) * np.sin(lon), -np.sin(lat), np.cos(lat) * np.cos(lon)], -1)


def view_coords(theta, Hs, Ws, D):
    """theta = (roll, pitch, yaw [rad], rel_focal, rel_cx, rel_cy, xi) of a view of Hs x Ws -> its coordinates (a, b) of the directions D in
    pixel-edge units (NaN where the view does not see the ray), the distance d to its border (NaN likewise), `covers`, and X.z"""
    M = rotation(theta[0], theta[1]).T @ yaw_matrix(-theta[2])
    X = D @ M.T
    with np.errstate(invalid="ignore", divide="ignore"):
        vis = X[..., 2] > z_min(theta[6])
        F, Cx, Cy = intrinsics(theta[3], theta[4], theta[5], Hs, Ws)
        xy = project(X, theta[6])
        a = np.where(vis, F * xy[..., 0] + Cx, np.nan)
        b = np.where(vis, F * xy[..., 1] + Cy, np.nan)
        d = np.minimum(np.minimum(a, Ws - a), np.minimum(b, Hs - b))
        covers = vis & (d > 0)
    return a, b, d, covers, X[..., 2]


def feather_weight(d, covers, Hs, Ws):
    with np.errstate(invalid="ignore"):
        return np.where(covers, np.minimum(2.0 * d / min(Hs, Ws), 1.0), 0.0)


def compose(images, thetas, Hp, Wp, blend=FEATHER, fill=0.0):
    """the composite in fp64 before any rounding (Hp, Wp, 3), the summed weight S (Hp, Wp), the number of covering views (Hp, Wp)"""
    D = pano_directions(Hp, Wp)
    C, S, n = np.zeros((Hp, Wp, 3)), np.zeros((Hp, Wp)), np.zeros((Hp, Wp), dtype=np.int64)
    for img, th in zip(images, thetas):
        Hs, Ws = img.shape[:2]
        if not np.isfinite(np.asarray(th, dtype=np.float64)).all():
            continue   # a view with non-finite parameters contributes nothing
        a, b, d, covers, _ = view_coords(th, Hs, Ws, D)
        w = feather_weight(d, covers, Hs, Ws) if blend == FEATHER else covers.astype(np.float64)
        C += w[..., None] * sample(img, a, b, covers, 0.0)
        S += w
        n += covers
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where((S > 0)[..., None], C / S[..., None], float(fill)), S, n


def view_coords_f32(theta, Hs, Ws, Hp, Wp):
    """the same formulas with every step in numpy float32, in the order of pano_compose.hip: (a, b) float32 (NaN where not visible) and the
    feather weight, 0 where the view does not cover the pixel"""
    f = np.float32
    r, p, yaw, rf, cx, cy, xi = [f(v) for v in theta]
    sr, cr, sp, cp = np.sin(r), np.cos(r), np.sin(p), np.cos(p)
    R = np.array([[cr, -sr, f(0)], [cp * sr, cp * cr, -sp], [sp * sr, sp * cr, cp]], dtype=f)
    t = f(0) - yaw
    Y = np.array([[np.cos(t), f(0), np.sin(t)], [f(0), f(1), f(0)], [-np.sin(t), f(0), np.cos(t)]], dtype=f)
    M = R.T @ Y
    lon = ((np.arange(Wp, dtype=f) + f(0.5)) / f(Wp) - f(0.5)) * f(2 * np.pi)
    lat = (f(0.5) - (np.arange(Hp, dtype=f) + f(0.5)) / f(Hp)) * f(np.pi)
    lat, lon = np.meshgrid(lat, lon, indexing="ij")
    D = np.stack([np.cos(lat) * np.sin(lon), f(0) - np.sin(lat), np.cos(lat) * np.cos(lon)], -1)
    assert D.dtype == f and M.dtype == f
    X = D @ M.T
    with np.errstate(invalid="ignore", divide="ignore"):
        vis = X[..., 2] > f(z_min(float(xi)))
        den = X[..., 2] + xi * np.sqrt((X * X).sum(-1))
        a = rf * f(Hs) * (X[..., 0] / den) + (cx + f(0.5)) * f(Ws)
        b = rf * f(Hs) * (X[..., 1] / den) + (cy + f(0.5)) * f(Hs)
        ra, rb = f(Ws) - a, f(Hs) - b
        covers = vis & (a > 0) & (ra > 0) & (b > 0) & (rb > 0)
        w = np.minimum(np.minimum(np.minimum(a, ra), np.minimum(b, rb)) * (f(2) / f(min(Hs, Ws))), f(1))
    assert a.dtype == f and w.dtype == f
    return np.where(vis, a, f(np.nan)), np.where(vis, b, f(np.nan)), np.where(covers, w, f(0))


def fp32_floor(views, Hp, Wp):
    """errors of the float32 evaluation of the feather composition of `views` = [(theta, Hs, Ws)] against fp64: (largest error of the summed
    weight S, of one view's weight, of a coordinate in px on the pixels the view covers)"""
    D = pano_directions(Hp, Wp)
    S64, S32 = np.zeros((Hp, Wp)), np.zeros((Hp, Wp), dtype=np.float32)
    e_w = e_c = 0.0
    for th, Hs, Ws in views:
        a, b, d, covers, _ = view_coords(th, Hs, Ws, D)
        w = feather_weight(d, covers, Hs, Ws)
        a32, b32, w32 = view_coords_f32(th, Hs, Ws, Hp, Wp)
        S64 += w
        S32 = S32 + w32
        e_w = max(e_w, float(np.abs(w32 - w).max()))
        if covers.any():
            e_c = max(e_c, float(np.abs(a32 - a)[covers].max()), float(np.abs(b32 - b)[covers].max()))
    return float(np.abs(S32 - S64).max()), e_w, e_c


def image_bound(n_cover, S_ref, e_w, e_c, grad, value_range=1.0):
    """allowed error of the float32 composite per pixel: every covering view's sample is off by at most its
    coordinate error x the largest gradient of the source x 2 (two coordinates), its weight by e_w, which moves the quotient by at most
    (covering views x e_w x value range) / S; 1e-6 for the fp32 roundings of the blend itself"""
    with np.errstate(divide="ignore", invalid="ignore"):
        return n_cover * e_c * grad * 2 + np.where(S_ref > 0, n_cover * e_w * value_range / S_ref, 0.0) + 1e-6


def near_a_border(theta, Hs, Ws, D):
    """pixels whose fp32 and fp64 coverage by this view may legitimately differ: within 1e-2 px of the view's border or 1e-3 of z_min"""
    a, b, d, _, z = view_coords(theta, Hs, Ws, D)
    with np.errstate(invalid="ignore"):
        return (np.abs(d) <= 1e-2) | (np.abs(z - z_min(theta[6])) <= 1e-3)


# ---------------------------------------------------------------- the fixed inputs of the GPU test
F100, F110 = 0.5 / np.tan(np.radians(50.0)), 0.5 / np.tan(np.radians(55.0))   # rel_focal of a 100 / 110 degree vertical field of view
# (roll, pitch, yaw [deg], rel_focal, rel_cx, rel_cy, xi), (Hs, Ws): four views of 100 degrees around the horizon, the two poles (110 degrees), one USM view
VIEWS = [((3.0, 4.0, 0.0, F100, 0.0, 0.0, 0.0), (48, 48)), ((-2.0, -3.0, 90.0, F100, 0.0, 0.0, 0.0), (48, 48)),
         ((1.5, 2.0, 180.0, F100, 0.03, -0.02, 0.0), (40, 56)), ((-4.0, -1.0, 270.0, F100, 0.0, 0.0, 0.0), (48, 48)),
         ((0.0, 90.0, 0.0, F110, 0.0, 0.0, 0.0), (48, 48)), ((0.0, -90.0, 30.0, F110, 0.0, 0.0, 0.0), (48, 48)),
         ((10.0, 20.0, 45.0, 0.6, 0.0, 0.0, 0.8), (61, 83))]
PANOS = [(32, 64), (37, 75)]   # the vector and the scalar store path
EDGE_PANOS = [(1, 17), (19, 1), (16, 64), (17, 68)]
SINGLE_VIEWS = (2, 6)   # the views of the GPU test of MEAN with one view: the off-centre pinhole view and the USM view


def views_rad(views=None):
    return [(theta_rad(*th), Hs, Ws) for th, (Hs, Ws) in (VIEWS if views is None else views)]


@functools.lru_cache(None)
def floor_of(size):
    return fp32_floor(views_rad(), *size)


# ---------------------------------------------------------------- the reference against itself
def test_direction_is_the_inverse_of_the_panorama_crop():
    """a view's world ray -> the crop's panorama coordinates (u, v) -> this model's direction at (u, v) is the ray again"""
    Hp, Wp = 64, 128
    for th, (Hs, Ws) in VIEWS:
        th = theta_rad(*th)
        u, v, Xw, ok = sample_coords(th, Hs, Ws, Hp, Wp)
        W = Xw @ yaw_matrix(th[2]).T
        lon = ((u + 0.5) / Wp - 0.5) * 2 * np.pi
        lat = (0.5 - (v + 0.5) / Hp) * np.pi
        D = np.stack([np.cos(lat) * np.sin(lon), -np.sin(lat), np.cos(lat) * np.cos(lon)], -1)
        assert ok.all() and np.abs(D - W).max() <= 1e-12


@pytest.mark.parametrize("size", PANOS)
def test_panorama_pixel_and_its_point_in_a_view_share_their_world_ray(size):
    D = pano_directions(*size)
    for th, (Hs, Ws) in VIEWS:
        th = theta_rad(*th)
        a, b, _, covers, _ = view_coords(th, Hs, Ws, D)
        F, Cx, Cy = intrinsics(th[3], th[4], th[5], Hs, Ws)
        X, ok = unproject((a[covers] - Cx) / F, (b[covers] - Cy) / F, th[6])
        back = X @ (yaw_matrix(th[2]) @ rotation(th[0], th[1])).T
        assert covers.any() and ok.all() and np.abs(back - D[covers]).max() <= 1e-12


def test_feather_weight_is_0_on_the_border_and_1_at_the_centre():
    Hs = Ws = 48
    th = theta_rad(0.0, 0.0, 0.0, 0.5, 0.0, 0.0, 0.0)
    F, Cx, Cy = intrinsics(th[3], th[4], th[5], Hs, Ws)

    def weight_at(a, b):   # the direction of the view's point (a, b), then the model
        X, _ = unproject(np.array([(a - Cx) / F]), np.array([(b - Cy) / F]), 0.0)
        _, _, d, covers, _ = view_coords(th, Hs, Ws, X)
        return feather_weight(d, covers, Hs, Ws)[0]

    assert abs(weight_at(24.0, 24.0) - 1.0) <= 1e-12
    assert abs(weight_at(0.0, 24.0)) <= 1e-12 and abs(weight_at(24.0, 48.0)) <= 1e-12 and weight_at(-1.0, 24.0) == 0.0 and weight_at(24.0, 49.0) == 0.0
    assert abs(weight_at(6.0, 24.0) - 0.25) <= 1e-12 and abs(weight_at(24.0, 36.0) - 0.5) <= 1e-12
    # a wide view: the weight is set by the short side
    _, _, d, covers, _ = view_coords(th, 40, 56, np.array([[0.0, 0.0, 1.0]]))
    assert abs(d[0] - 20.0) <= 1e-12 and feather_weight(d, covers, 40, 56)[0] == 1.0


def test_mean_of_one_view_is_its_bilinear_sample():
    rng = np.random.default_rng(2)
    img = rng.uniform(0, 1, (48, 48, 3))
    th, (Hs, Ws) = VIEWS[0]
    th = theta_rad(*th)
    out, S, n = compose([img], [th], 32, 64, MEAN, fill=0.5)
    a, b, _, covers, _ = view_coords(th, Hs, Ws, pano_directions(32, 64))
    assert np.array_equal(S, covers.astype(np.float64)) and np.array_equal(n, covers)
    assert np.array_equal(out, sample(img, a, b, covers, 0.5))


@pytest.mark.parametrize("size", PANOS + EDGE_PANOS)
def test_fixed_views_cover_the_panorama_and_nothing_is_left_out(size):
    """the seven views cover every pixel, with a total feather weight far above the 1e-3 under which the image test would leave a pixel out
    (so it leaves none out); the single-view test leaves out at most 1 % near a border of its view"""
    Hp, Wp = size
    imgs = [np.zeros((Hs, Ws, 3)) for _, (Hs, Ws) in VIEWS]
    _, S, n = compose(imgs, [theta_rad(*th) for th, _ in VIEWS], Hp, Wp)
    print(f"{Hp} x {Wp}: smallest total feather weight {S.min():.4f}, at most {n.max()} views on a pixel, at least {n.min()}")
    assert n.min() >= 1 and n.max() <= 4
    assert S.min() >= 0.1
    assert ((S > 0) & (S < 1e-3)).mean() == 0.0
    D = pano_directions(Hp, Wp)
    for k in SINGLE_VIEWS:
        th, (Hs, Ws) = VIEWS[k]
        share = near_a_border(theta_rad(*th), Hs, Ws, D).mean()
        print(f"    view {k} alone: {100 * share:.2f} % of the pixels within 1e-2 px of its border or 1e-3 of z_min")
        assert share <= 0.01, th


@pytest.mark.parametrize("size", PANOS)
def test_fp32_floor_of_the_weights_and_coordinates(size):
    """the float32 evaluation is close to fp64: its error is the floor the GPU weight is held to (x 4) and the image bound is built from"""
    e_S, e_w, e_c = floor_of(size)
    print(f"fp32 floor at {size}: S {e_S:.3e}, one view's weight {e_w:.3e}, coordinates {e_c:.3e} px")
    assert 0 < e_w <= 1e-5 and 0 < e_S <= 3e-5 and 0 < e_c <= 1e-3   # fp32 epsilon times ~50 px; a looser floor would make the GPU check empty


def test_view_order_and_non_finite_views():
    rng = np.random.default_rng(4)
    imgs = [rng.uniform(0, 1, (Hs, Ws, 3)) for _, (Hs, Ws) in VIEWS]
    ths = [theta_rad(*th) for th, _ in VIEWS]
    out, S, _ = compose(imgs, ths, 16, 32)
    bad = list(ths[1])
    bad[3] = np.nan
    out2, S2, _ = compose(imgs[:1] + [imgs[1]] + imgs[1:], ths[:1] + [tuple(bad)] + ths[1:], 16, 32)
    assert np.array_equal(out, out2) and np.array_equal(S, S2)
    none, S0, n0 = compose([], [], 4, 8, fill=0.25)
    assert (none == 0.25).all() and (S0 == 0).all() and (n0 == 0).all()


# ---------------------------------------------------------------- host-side contract (fails before the feature exists)
def test_compose_panorama_is_exported():
    import perspective2d
    import perspectivefields_amd

    assert "compose_panorama" in perspectivefields_amd.__all__
    assert callable(perspectivefields_amd.compose_panorama) and callable(perspective2d.compose_panorama)
    assert callable(perspectivefields_amd.PerspectiveFields.compose_panorama)


def test_blend_constants_match_the_header():
    from perspectivefields_amd import perspectivefields as pfm

    hdr = open(os.path.join(ROOT, "include", "pf_hip.h")).read()
    assert f"#define PF_BLEND_FEATHER {pfm.BLEND_FEATHER}" in hdr and f"#define PF_BLEND_MEAN {pfm.BLEND_MEAN}" in hdr
    assert "int pf_pano_compose(int device, int n_view, const void* const* h_view, const int32_t* h_view_hw" in hdr
    kh = open(os.path.join(ROOT, "perspectivefields_amd", "csrc", "pf_kernels.h")).read()
    assert f"static constexpr int MAX = {pfm._COMPOSE_MAX_VIEWS};" in kh


def test_symbol_and_prototype_are_present():
    from perspectivefields_amd.engine import _SIGNATURES, declared_symbols, load_library

    assert "pf_pano_compose" in declared_symbols()
    res, args = _SIGNATURES["pf_pano_compose"]
    assert res is ctypes.c_int and len(args) == 16 and args[11] is ctypes.c_float
    assert hasattr(load_library(), "pf_pano_compose")


CAM = dict(roll=0.0, pitch=0.0, rel_focal=1.0)


def test_compose_panorama_on_cpu_tensors_raises():
    from perspectivefields_amd import compose_panorama
    from perspectivefields_amd.engine import PfError

    for images in (torch.zeros((8, 16, 3), dtype=torch.uint8), torch.zeros((2, 8, 16, 3)), [torch.zeros((8, 16, 3))]):
        with pytest.raises(PfError):
            compose_panorama(images, CAM, height=8, width=16)


def test_pf_pano_compose_rejects_bad_arguments_before_device_work():
    from perspectivefields_amd.engine import load_library

    lib = load_library()
    ints = lambda *s: (ctypes.c_int32 * len(s))(*s)
    ptrs = lambda n: (ctypes.c_void_p * n)(*([0x1000] * n))
    dev = ctypes.c_void_p(256)

    def call(n=1, p=None, hw=None, dtype=0, idx=(0,), c_idx=True, cam=dev, n_pano=1, Hp=4, Wp=8, blend=0, pano=dev, weight=None, acc=None):
        rc = lib.pf_pano_compose(0, n, ptrs(max(n, 1)) if p is None else None if p == "null" else p, hw or ints(*([8, 16] * max(n, 1))), dtype, ints(*idx) if c_idx else None, cam,
                                 n_pano, Hp, Wp, blend, 0.0, pano, weight, acc, None)
        return rc, lib.pf_last_error(None).decode()

    for kw, what in ((dict(idx=(1,)), "index"), (dict(idx=(-1,)), "index"), (dict(n=2, idx=(1, 0), n_pano=2), "decrease"), (dict(dtype=2), "dtype"),
                     (dict(blend=2), "blend"), (dict(blend=-1), "blend"), (dict(hw=ints(0, 16)), "smaller"), (dict(hw=ints(8, 0)), "smaller"),
                     (dict(Hp=0), "size"), (dict(Wp=0), "size"), (dict(pano=None), "required"), (dict(cam=None), "required"), (dict(c_idx=False), "required"),
                     (dict(n_pano=0), "required"), (dict(n=0), "at least one"), (dict(p="null"), "at least one"), (dict(p=(ctypes.c_void_p * 1)()), "NULL"),
                     (dict(n=33, idx=(0,) * 33), "d_acc"), (dict(n=34, idx=(0,) + (1,) * 33, n_pano=2), "d_acc")):
        rc, msg = call(**kw)
        assert rc == -1 and what in msg and msg.startswith("pf_pano_compose"), (kw, rc, msg)
    # 32 views of one panorama and 33 over two need no accumulator: these pass the argument checks and fail on the missing device only
    if not torch.cuda.is_available():
        for kw in (dict(n=32, idx=(0,) * 32), dict(n=33, idx=(0,) * 16 + (1,) * 17, n_pano=2)):
            rc, msg = call(**kw)
            assert rc == -2 and "no HIP device" in msg, (kw, rc, msg)


def test_compose_panorama_argument_errors_before_the_library_is_loaded(monkeypatch):
    from perspectivefields_amd import engine
    from perspectivefields_amd import perspectivefields as pfm

    def no_library(*a, **k):
        raise AssertionError("the library was loaded before the arguments were checked")

    monkeypatch.setattr(engine, "load_library", no_library)
    monkeypatch.setattr(pfm.torch, "is_tensor", lambda v: isinstance(v, (torch.Tensor, FakeCuda)))
    ok, small = FakeCuda((8, 16, 3)), FakeCuda((6, 16, 3))
    bad = [
        dict(images=FakeCuda((8, 16, 4))), dict(images=FakeCuda((8, 16))), dict(images=FakeCuda((0, 16, 3))), dict(images=FakeCuda((8, 16, 3), torch.float16)),
        dict(images=[ok, FakeCuda((8, 16, 3), torch.float32)]), dict(images=[]), dict(images=FakeCuda((0, 8, 16, 3))), dict(images=[FakeCuda((2, 8, 16, 3))]),
        dict(height=0), dict(width=0), dict(mode="grad"), dict(blend="max"), dict(pano_index=[0, 0]), dict(pano_index=[-1]), dict(pano_index=[1], n_pano=1),
        dict(n_pano=0), dict(images=[ok, small], pano_index=[0]), dict(cams=dict(roll=0.0, pitch=0.0)), dict(cams=dict(CAM, fov=1.0)),
        dict(cams=dict(CAM, xi=np.zeros((2, 2)))), dict(cams=dict(CAM, roll=[1.0, 2.0], pitch=[1.0, 2.0, 3.0])), dict(images=[ok, small, ok], cams=dict(CAM, roll=[1.0, 2.0])),
    ]
    for kw in bad:
        args = dict(images=ok, cams=CAM, height=8, width=16)
        args.update(kw)
        with pytest.raises(ValueError):
            pfm.compose_panorama(args.pop("images"), args.pop("cams"), **args)
    with pytest.raises(TypeError):
        pfm.compose_panorama(ok, (0.0, 0.0, 1.0), height=8, width=16)
    with pytest.raises(TypeError):
        pfm.compose_panorama([ok, np.zeros((8, 16, 3))], CAM, height=8, width=16)
    with pytest.raises(TypeError):
        pfm.compose_panorama(ok, CAM)   # height and width are required


def test_model_method_argument_errors_without_a_gpu():
    from perspectivefields_amd import PerspectiveFields
    from perspectivefields_amd.engine import PfError

    ok = FakeCuda((8, 16, 3))
    fields_only = dict(pred_gravity_original=None, pred_latitude_original=None)
    with pytest.raises(PfError, match="fit_camera"):
        PerspectiveFields.compose_panorama(None, ok, fields_only, height=8, width=16)
    full = dict(pred_roll=1.0, pred_pitch=2.0, pred_rel_focal=0.8)
    with pytest.raises(ValueError):
        PerspectiveFields.compose_panorama(None, ok, full, height=8, width=16, mode="rad")
    with pytest.raises(ValueError):
        PerspectiveFields.compose_panorama(None, ok, [], height=8, width=16)


def test_compose_kernels_are_in_the_library_without_scratch():
    """scripts/kernel_resources.py on the built library: the four kernels are there for gfx950 with no spilled register and no scratch"""
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
    for t in ("unsigned char", "float"):
        for feather in ("false", "true"):
            r = by[f"pf::pano_compose_kernel<{t}, {feather}>"]
            assert r["spill"] == 0 and r["scratch"] == 0 and r["lds"] <= 2304, r
