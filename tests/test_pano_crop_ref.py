"""fp64 numpy statement of the panorama crop's camera model (include/pf_hip.h pf_pano_crop): sampling
coordinates, bilinear sampling of uint8 / float32 panoramas, and the ground-truth fields, checked against the oracle's
camera-parameters -> fields model (pinned to the reference by tests/golden/fields_from_params.npz); plus the host-side contract
of crop_panorama (no GPU needed).  tests/test_gpu_pano_crop.py uses the same reference on the GPU results."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from oracle import pf_oracle
from tests.test_fit_camera_ref import general_vfov_deg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R2D = 180.0 / np.pi


def rotation(roll, pitch):
    """camera -> world, R_pitch(p) R_roll(r)"""
    cr, sr, cp, sp = np.cos(roll), np.sin(roll), np.cos(pitch), np.sin(pitch)
    Rr = np.array([[cr, -sr, 0.0], [sr, cr, 0.0], [0.0, 0.0, 1.0]])
    Rp = np.array([[1.0, 0.0, 0.0], [0.0, cp, -sp], [0.0, sp, cp]])
    return Rp @ Rr


def unproject(x, y, xi):
    """Unified Spherical Model ray of normalised image points -> (X (..., 3) unit vectors, has_ray mask); NaN where there is no ray"""
    r2 = x * x + y * y
    disc = 1.0 + (1.0 - xi * xi) * r2
    ok = disc >= 0
    eta = (xi + np.sqrt(np.where(ok, disc, np.nan))) / (1.0 + r2)
    return np.stack([eta * x, eta * y, eta - xi], -1), ok


def project(X, xi):
    return X[..., :2] / (X[..., 2] + xi * np.linalg.norm(X, axis=-1))[..., None]


def intrinsics(f, cx, cy, H, W):
    return f * H, (cx + 0.5) * W, (cy + 0.5) * H


def pixel_rays(theta, H, W):
    """theta = (roll, pitch, yaw [rad], rel_focal, rel_cx, rel_cy, xi) -> camera rays at the pixel centres (H, W, 3), has_ray (H, W)"""
    r, p, yaw, f, cx, cy, xi = (float(v) for v in theta)
    F, Cx, Cy = intrinsics(f, cx, cy, H, W)
    a = np.arange(W, dtype=np.float64)[None, :] + 0.5 + np.zeros((H, 1))
    b = np.arange(H, dtype=np.float64)[:, None] + 0.5 + np.zeros((1, W))
    return unproject((a - Cx) / F, (b - Cy) / F, xi)


def sample_coords(theta, H, W, Hp, Wp):
    """panorama coordinates (u, v) of every output pixel (NaN without a ray), world rays (H, W, 3) and has_ray"""
    r, p, yaw = (float(v) for v in theta[:3])
    X, ok = pixel_rays(theta, H, W)
    Xw = X @ rotation(r, p).T
    lat = -np.arctan2(Xw[..., 1], np.hypot(Xw[..., 0], Xw[..., 2]))
    lon = yaw + np.arctan2(Xw[..., 0], Xw[..., 2])
    lon = lon - 2 * np.pi * np.floor((lon + np.pi) / (2 * np.pi))
    u = (lon / (2 * np.pi) + 0.5) * Wp - 0.5
    v = (0.5 - lat / np.pi) * Hp - 0.5
    return u, v, Xw, ok


def bilinear(pano, u, v):
    """bilinear sample of (Hp, Wp, 3) at (u, v) in fp64: columns wrap modulo Wp, rows clamp; 0 where u is NaN"""
    Hp, Wp = pano.shape[:2]
    ok = np.isfinite(u) & np.isfinite(v)
    u, v = np.where(ok, u, 0.0), np.where(ok, v, 0.0)
    uf, vf = np.floor(u), np.floor(v)
    fu, fv = (u - uf)[..., None], (v - vf)[..., None]
    c0 = np.mod(uf.astype(np.int64), Wp)
    c1 = np.mod(c0 + 1, Wp)
    r0 = np.clip(vf.astype(np.int64), 0, Hp - 1)
    r1 = np.clip(vf.astype(np.int64) + 1, 0, Hp - 1)
    P = pano.astype(np.float64)
    top = (1 - fu) * P[r0, c0] + fu * P[r0, c1]
    bot = (1 - fu) * P[r1, c0] + fu * P[r1, c1]
    return np.where(ok[..., None], (1 - fv) * top + fv * bot, 0.0)


def crop_image(pano, theta, H, W):
    """the crop in fp64 (before the uint8 rounding)"""
    u, v, _, _ = sample_coords(theta, H, W, pano.shape[0], pano.shape[1])
    return bilinear(pano, u, v)


def labels(theta, H, W):
    """ground-truth fields (up (2, H, W), lat (H, W) degrees) in fp64; NaN without a ray"""
    r, p, yaw, f, cx, cy, xi = (float(v) for v in theta)
    F, Cx, Cy = intrinsics(f, cx, cy, H, W)
    R = rotation(r, p)
    g = R.T @ np.array([0.0, -1.0, 0.0])
    X, _ = pixel_rays(theta, H, W)
    D = X[..., 2] + xi
    s = g[2] + xi * (X @ g)
    up = np.stack([g[0] * D - X[..., 0] * s, g[1] * D - X[..., 1] * s])
    up = up / np.sqrt((up * up).sum(0))
    sx = W / (W - 1) if W > 1 else 0.0
    sy = H / (H - 1) if H > 1 else 0.0
    a = (np.arange(W, dtype=np.float64) * sx)[None, :] + np.zeros((H, 1))
    b = (np.arange(H, dtype=np.float64) * sy)[:, None] + np.zeros((1, W))
    Xl, _ = unproject((a - Cx) / F, (b - Cy) / F, xi)
    Xw = Xl @ R.T
    lat = -np.arctan2(Xw[..., 1], np.hypot(Xw[..., 0], Xw[..., 2])) * R2D
    return up, lat


PINHOLE_CASES = [  # (roll, pitch [deg], rel_focal, rel_cx, rel_cy, H, W)
    (10.0, 25.0, 0.8, 0.0, 0.0, 48, 64),
    (-35.0, 0.0, 1.2, 0.0, 0.0, 31, 47),
    (5.0, -60.0, 0.45, 0.07, -0.05, 33, 29),
    (0.0, 0.0, 0.9, -0.1, 0.1, 40, 40),
    (20.0, 12.0, 0.7, 0.0, 0.0, 1, 17),
    (-8.0, -30.0, 0.6, 0.02, 0.0, 19, 1),
]


@pytest.mark.parametrize("case", PINHOLE_CASES)
def test_pinhole_labels_match_the_oracle(case):
    r, p, f, cx, cy, H, W = case
    up, lat = labels((np.radians(r), np.radians(p), 0.3, f, cx, cy, 0.0), H, W)
    upo, lato, fo = pf_oracle.fields_from_params(r, p, general_vfov_deg(f, cx, cy), cx, cy, H, W, mode="deg")
    assert abs(fo - f) <= 1e-12 * f
    assert np.abs(up - np.moveaxis(upo, 2, 0)).max() <= 1e-9
    assert np.abs(lat - lato).max() <= 1e-9


@pytest.mark.parametrize("xi", [0.3, 0.8, 1.0, 1.5])
def test_usm_ray_is_a_unit_vector_that_projects_back(xi):
    rng = np.random.default_rng(int(xi * 10))
    x, y = rng.uniform(-1.2, 1.2, (2, 2000))
    X, ok = unproject(x, y, xi)
    assert ok.any()
    X, x, y = X[ok], x[ok], y[ok]
    assert np.abs(np.linalg.norm(X, axis=-1) - 1).max() <= 1e-12
    assert np.abs(project(X, xi) - np.stack([x, y], -1)).max() <= 1e-12


@pytest.mark.parametrize("xi", [0.0, 0.5, 0.8, 1.2])
def test_usm_up_label_is_the_projected_step_along_world_up(xi):
    theta = (np.radians(12.0), np.radians(35.0), 0.0, 0.4, 0.03, -0.02, xi)
    H, W = 24, 32
    up, _ = labels(theta, H, W)
    X, ok = pixel_rays(theta, H, W)
    g = rotation(theta[0], theta[1]).T @ np.array([0.0, -1.0, 0.0])
    t = 1e-7
    d = project(X + t * g, xi) - project(X, xi)
    d = np.moveaxis(d / np.linalg.norm(d, axis=-1, keepdims=True), -1, 0)
    assert np.nanmax(np.abs(d - up)[:, ok]) <= 1e-6


def test_no_ray_region_is_exactly_beyond_the_critical_radius():
    xi = 1.6
    rng = np.random.default_rng(5)
    x, y = rng.uniform(-2, 2, (2, 20000))
    _, ok = unproject(x, y, xi)
    assert np.array_equal(~ok, x * x + y * y > 1.0 / (xi * xi - 1.0))
    theta = (0.1, 0.2, 0.0, 0.25, 0.0, 0.0, xi)
    up, lat = labels(theta, 40, 40)
    X, ok = pixel_rays(theta, 40, 40)
    assert (~ok).any() and ok.any()
    assert np.isnan(up[:, ~ok]).all() and np.isfinite(up[:, ok]).all()
    assert np.isnan(lat).any()


def test_yaw_does_not_change_the_labels():
    for xi in (0.0, 0.7):
        a = labels((0.2, -0.3, 0.0, 0.6, 0.05, 0.0, xi), 21, 34)
        b = labels((0.2, -0.3, 2.5, 0.6, 0.05, 0.0, xi), 21, 34)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_sampling_conventions():
    """the centre of a level view looks at the panorama point of its yaw; columns wrap at the seam, rows clamp"""
    Hp, Wp = 8, 16
    u, v, _, _ = sample_coords((0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0), 1, 1, Hp, Wp)   # a 1 x 1 crop: its pixel centre is the principal point
    assert np.allclose([u[0, 0], v[0, 0]], [Wp / 2 - 0.5, Hp / 2 - 0.5])
    u, v, _, _ = sample_coords((0.3, np.radians(30), np.radians(90), 1.0, 0.0, 0.0, 0.0), 1, 1, Hp, Wp)
    assert np.allclose([u[0, 0], v[0, 0]], [0.75 * Wp - 0.5, (0.5 - 30 / 180) * Hp - 0.5])
    u, _, _, _ = sample_coords((0.0, 0.0, np.radians(-180), 1.0, 0.0, 0.0, 0.0), 1, 1, Hp, Wp)
    assert np.allclose(u[0, 0], -0.5)   # lon = -pi: the seam, between column Wp - 1 and column 0
    pano = np.arange(Hp * Wp * 3, dtype=np.float64).reshape(Hp, Wp, 3)
    s = bilinear(pano, np.array([Wp - 0.5, -0.5]), np.array([-0.5, Hp - 0.5]))
    assert np.allclose(s[0], 0.5 * (pano[0, Wp - 1] + pano[0, 0]))
    assert np.allclose(s[1], 0.5 * (pano[Hp - 1, Wp - 1] + pano[Hp - 1, 0]))


# ---------------------------------------------------------------- host-side contract (fails before the feature exists)
def test_crop_panorama_is_exported():
    import perspectivefields_amd

    assert "crop_panorama" in perspectivefields_amd.__all__
    assert callable(perspectivefields_amd.crop_panorama)


def test_pano_dtype_constants_match_the_header():
    from perspectivefields_amd.perspectivefields import PANO_F32, PANO_U8

    hdr = open(os.path.join(ROOT, "include", "pf_hip.h")).read()
    consts = {m[0]: int(m[1]) for m in re.findall(r"#define PF_PANO_([A-Z0-9]+) (\d+)", hdr)}
    assert consts == {"U8": PANO_U8, "F32": PANO_F32}


def test_crop_panorama_on_cpu_tensors_raises():
    from perspectivefields_amd import crop_panorama
    from perspectivefields_amd.engine import PfError

    with pytest.raises(PfError):
        crop_panorama(torch.zeros((8, 16, 3), dtype=torch.uint8), 0.0, 0.0, 1.0, height=4, width=4)


def test_pf_pano_crop_rejects_bad_arguments_before_device_work():
    from perspectivefields_amd.engine import load_library

    lib = load_library()
    pano = (ctypes.c_void_p * 1)(0x1000)
    hw = lambda *s: (ctypes.c_int32 * len(s))(*s)
    dev = ctypes.c_void_p(256)

    def call(hw_=None, dtype=0, idx=(0,), H=4, W=4, img=dev, up=None, lat=None, n=1, p=pano):
        return lib.pf_pano_crop(0, n, p, hw_ or hw(8, 16), dtype, len(idx), hw(*idx), dev, H, W, img, up, lat, None), lib.pf_last_error(None).decode()

    for kw, what in ((dict(idx=(1,)), "index"), (dict(dtype=2), "dtype"), (dict(hw_=hw(1, 16)), "smaller"), (dict(H=0), "size"),
                     (dict(img=None), "required"), (dict(up=dev), "both"), (dict(lat=dev), "both"), (dict(p=(ctypes.c_void_p * 1)()), "NULL")):
        rc, msg = call(**kw)
        assert rc == -1 and what in msg, (kw, rc, msg)


def test_crop_panorama_argument_errors_without_a_gpu(monkeypatch):
    """shape / dtype / index / broadcast errors raise ValueError before anything is launched (a stand-in CUDA tensor: the checks read only
    .is_cuda, .dim(), .shape, .dtype and .device)"""
    from perspectivefields_amd import perspectivefields as pfm

    class FakeCuda:
        def __init__(self, shape, dtype=torch.uint8):
            self.shape, self.dtype, self.device, self.is_cuda = tuple(shape), dtype, torch.device("cuda", 0), True

        def dim(self):
            return len(self.shape)

    monkeypatch.setattr(pfm.torch, "is_tensor", lambda v: isinstance(v, (torch.Tensor, FakeCuda)))
    ok = FakeCuda((8, 16, 3))
    bad = [
        dict(pano=FakeCuda((8, 16, 4))), dict(pano=FakeCuda((8, 16))), dict(pano=FakeCuda((1, 16, 3))), dict(pano=FakeCuda((8, 16, 3), torch.float16)),
        dict(pano=[ok, FakeCuda((8, 16, 3), torch.float32)]), dict(height=0), dict(mode="grad"), dict(pano_index=[1]), dict(pano_index=[0, 0]),
        dict(roll=[1.0, 2.0], pitch=[1.0, 2.0, 3.0]), dict(roll=np.zeros((2, 2))),
    ]
    for kw in bad:
        args = dict(pano=ok, roll=0.0, pitch=0.0, rel_focal=1.0, height=4, width=4)
        args.update(kw)
        with pytest.raises(ValueError):
            pfm.crop_panorama(args.pop("pano"), args.pop("roll"), args.pop("pitch"), args.pop("rel_focal"), **args)
