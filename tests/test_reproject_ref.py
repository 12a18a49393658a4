"""fp64 numpy statement of the re-projection between two cameras of one centre (include/pf_hip.h pf_reproject),
built on the camera model of tests/test_pano_crop_ref.py: source coordinates, visibility, the inside test, bilinear sampling with clamped
taps; checks of that reference against itself and against the panorama crop's conventions; the same formulas in numpy float32 (the
rounding floor the GPU map is measured against); plus the host-side contract of reproject_image / pf_reproject (no GPU needed).
tests/test_gpu_reproject.py uses the same reference on the GPU results."""
import ctypes
import itertools
import os

import numpy as np
import pytest
import torch

from tests.test_pano_crop_ref import intrinsics, pixel_rays, project, rotation, sample_coords, unproject

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def yaw_matrix(psi):
    """a turn about the world's vertical: atan2(x', z') = atan2(x, z) + psi"""
    c, s = np.cos(psi), np.sin(psi)
    return np.array([[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]])


def z_min(xi):
    """a unit ray is seen by a camera of mirror parameter xi iff its z exceeds this: the rays of unproject's "+" root"""
    return -1.0 / xi if xi > 1 else 0.0 - xi


def source_rays(src, dst, H, W):
    """rays of the destination's pixel centres in the source camera's frame (H, W, 3), has_ray (H, W), disc of the destination"""
    Xd, ok = pixel_rays(dst, H, W)
    M = rotation(src[0], src[1]).T @ yaw_matrix(dst[2] - src[2]) @ rotation(dst[0], dst[1])
    F, Cx, Cy = intrinsics(dst[3], dst[4], dst[5], H, W)
    x = (np.arange(W)[None, :] + 0.5 - Cx) / F
    y = (np.arange(H)[:, None] + 0.5 - Cy) / F
    return Xd @ M.T, ok, 1.0 + (1.0 - dst[6] ** 2) * (x * x + y * y)


def source_coords(src, Hs, Ws, dst, H, W):
    """theta = (roll, pitch, yaw [rad], rel_focal, rel_cx, rel_cy, xi) of both cameras -> source coordinates (a, b) of every destination
    pixel in pixel-edge units (NaN where the source camera does not see the ray) and the mask `inside`"""
    Xs, ok, _ = source_rays(src, dst, H, W)
    with np.errstate(invalid="ignore"):
        vis = ok & (Xs[..., 2] > z_min(src[6]))
    F, Cx, Cy = intrinsics(src[3], src[4], src[5], Hs, Ws)
    with np.errstate(invalid="ignore", divide="ignore"):
        xy = project(Xs, src[6])
    a = np.where(vis, F * xy[..., 0] + Cx, np.nan)
    b = np.where(vis, F * xy[..., 1] + Cy, np.nan)
    with np.errstate(invalid="ignore"):
        inside = vis & (a >= 0) & (a <= Ws) & (b >= 0) & (b <= Hs)
    return a, b, inside


def sample(img, a, b, inside, fill=0.0):
    """bilinear sample of (Hs, Ws, 3) at (a - 1/2, b - 1/2) in fp64, the four taps clamped into the image; `fill` where not inside"""
    Hs, Ws = img.shape[:2]
    u, v = np.where(inside, a - 0.5, 0.0), np.where(inside, b - 0.5, 0.0)
    uf, vf = np.floor(u), np.floor(v)
    fu, fv = (u - uf)[..., None], (v - vf)[..., None]
    c0, c1 = np.clip(uf.astype(np.int64), 0, Ws - 1), np.clip(uf.astype(np.int64) + 1, 0, Ws - 1)
    r0, r1 = np.clip(vf.astype(np.int64), 0, Hs - 1), np.clip(vf.astype(np.int64) + 1, 0, Hs - 1)
    P = img.astype(np.float64)
    top = (1 - fu) * P[r0, c0] + fu * P[r0, c1]
    bot = (1 - fu) * P[r1, c0] + fu * P[r1, c1]
    return np.where(inside[..., None], (1 - fv) * top + fv * bot, float(fill))


def clear(src, Hs, Ws, dst, H, W):
    """pixels whose fp32 and fp64 results cannot legitimately fall on different sides of a discontinuity: not within 1e-4 of the
    destination's no-ray circle (disc), 1e-3 of the source's visibility limit (z), 1e-2 px of the source image's border"""
    Xs, _, disc = source_rays(src, dst, H, W)
    a, b, _ = source_coords(src, Hs, Ws, dst, H, W)
    with np.errstate(invalid="ignore"):   # NaN (no ray, not visible): the pixel is on no such border
        near = np.abs(disc) <= 1e-4
        near |= np.abs(Xs[..., 2] - z_min(src[6])) <= 1e-3
        for c, n in ((a, Ws), (b, Hs)):
            near |= (np.abs(c) <= 1e-2) | (np.abs(c - n) <= 1e-2)
    return ~near


def source_coords_f32(src, Hs, Ws, dst, H, W):
    """the same formulas with every step in numpy float32, in the order of reproject.hip (1 / F_d as a factor, M from float32 sines): the
    rounding floor of the model at fp32, against which the GPU map is judged.  (a, b) float32, NaN where not visible"""
    f = np.float32
    s, d = [f(v) for v in src], [f(v) for v in dst]

    def rot(roll, pitch):
        sr, cr, sp, cp = np.sin(roll), np.cos(roll), np.sin(pitch), np.cos(pitch)
        return np.array([[cr, -sr, f(0)], [cp * sr, cp * cr, -sp], [sp * sr, sp * cr, cp]], dtype=f)

    t = d[2] - s[2]
    Y = np.array([[np.cos(t), f(0), np.sin(t)], [f(0), f(1), f(0)], [-np.sin(t), f(0), np.cos(t)]], dtype=f)
    M = rot(s[0], s[1]).T @ (Y @ rot(d[0], d[1]))
    inv_fd = f(1) / (d[3] * f(H))
    x = (np.arange(W, dtype=f)[None, :] + f(0.5) - (d[4] + f(0.5)) * f(W)) * inv_fd + np.zeros((H, 1), f)
    y = (np.arange(H, dtype=f)[:, None] + f(0.5) - (d[5] + f(0.5)) * f(H)) * inv_fd + np.zeros((1, W), f)
    r2 = x * x + y * y
    disc = f(1) + (f(1) - d[6] * d[6]) * r2
    with np.errstate(invalid="ignore", divide="ignore"):
        eta = (d[6] + np.sqrt(np.where(disc >= 0, disc, f(np.nan)))) / (f(1) + r2)
        X = np.stack([eta * x, eta * y, eta - d[6]], -1)
        Xs = X @ M.T
        vis = Xs[..., 2] > f(z_min(float(s[6])))
        D = Xs[..., 2] + s[6] * np.sqrt((Xs * Xs).sum(-1))
        a = s[3] * f(Hs) * (Xs[..., 0] / D) + (s[4] + f(0.5)) * f(Ws)
        b = s[3] * f(Hs) * (Xs[..., 1] / D) + (s[5] + f(0.5)) * f(Hs)
    assert a.dtype == f and b.dtype == f
    return np.where(vis, a, f(np.nan)), np.where(vis, b, f(np.nan))


def spread(src, Hs, Ws, a, b):
    """1 + rho_s^2 of source points: the factor by which a rounding error of a ray grows on its way to (a, b) beyond the error at the
    principal point (d(x / D) ~ (1 + rho^2) d(angle)); it normalises the map error of points far outside the source image"""
    F, Cx, Cy = intrinsics(src[3], src[4], src[5], Hs, Ws)
    return 1.0 + ((a - Cx) ** 2 + (b - Cy) ** 2) / (F * F)


def map_errors(src, Hs, Ws, dst, H, W, a, b):
    """errors of a map (a, b) against the fp64 reference on clear pixels: (largest |error| in px over inside pixels, largest
    |error| / spread over pixels that are visible and outside the source image, NaN pattern equal to the reference's)"""
    ar, br, inside = source_coords(src, Hs, Ws, dst, H, W)
    cl = clear(src, Hs, Ws, dst, H, W)
    vis = np.isfinite(ar)
    same = np.array_equal(np.isnan(a)[cl], ~vis[cl]) and np.array_equal(np.isnan(b)[cl], ~vis[cl])
    with np.errstate(invalid="ignore"):
        e = np.maximum(np.abs(a.astype(np.float64) - ar), np.abs(b.astype(np.float64) - br))
    m_in, m_out = cl & inside, cl & vis & ~inside
    return (float(e[m_in].max()) if m_in.any() else 0.0,
            float((e / spread(src, Hs, Ws, ar, br))[m_out].max()) if m_out.any() else 0.0, same)


def theta_rad(roll, pitch, yaw, f, cx, cy, xi):
    return (np.radians(roll), np.radians(pitch), np.radians(yaw), f, cx, cy, xi)


# (src, dst) camera pairs in degrees: (roll, pitch, yaw, rel_focal, rel_cx, rel_cy, xi) each; the destination is centred
CASES = []
for k, ((ps, pd), (ys, yd), (xs, xd)) in enumerate(itertools.product(((-35.0, 0.0), (0.0, 0.0), (50.0, 20.0), (0.0, -40.0)),
                                                                      ((0.0, 0.0), (170.0, -175.0), (-70.0, -40.0)),
                                                                      ((0.0, 0.0), (0.8, 0.0), (0.0, 0.5), (1.3, 0.4), (0.5, 1.2)))):
    cx, cy = ((0.0, 0.0), (0.08, -0.05))[(k // 2) % 2]
    CASES.append(((( -30.0, 0.0, 25.0)[k % 3], ps, ys, (0.35, 0.6)[k % 2], cx, cy, xs),
                  ((0.0, 10.0, -20.0)[(k // 3) % 3], pd, yd, (0.5, 0.9)[(k // 2) % 2], 0.0, 0.0, xd)))
SIZES = [(96, 128, 40, 56), (61, 83, 37, 53)]   # (Hs, Ws, H, W): odd sizes and W % 4 != 0 in the second
CLOSURE_CASES = (0, 6, 17, 21, 32, 40)   # the six pairs of the GPU closure test with the panorama crop


def fp32_floor(size):
    """largest map error of the float32 evaluation over the cases at one size: (px on inside pixels, normalised outside)"""
    Hs, Ws, H, W = size
    worst = np.zeros(2)
    for s, d in CASES:
        s, d = theta_rad(*s), theta_rad(*d)
        e_in, e_out, same = map_errors(s, Hs, Ws, d, H, W, *source_coords_f32(s, Hs, Ws, d, H, W))
        assert same, (s, d)
        worst = np.maximum(worst, (e_in, e_out))
    return worst


def world_rays(theta, x, y):
    """world rays Y(yaw) R unproject(x, y, xi) of normalised image points"""
    X, ok = unproject(x, y, theta[6])
    return X @ (yaw_matrix(theta[2]) @ rotation(theta[0], theta[1])).T, ok


def closure_reference(pano, src, dst, H, W):
    """fp64: the crop at `src`, re-projected to `dst`, against the direct crop at `dst`; angles (degrees) between the two direction
    images on the pixels whose source point lies at least 1 px inside the source image"""
    from tests.test_pano_crop_ref import crop_image

    a, b, inside = source_coords(src, H, W, dst, H, W)
    with np.errstate(invalid="ignore"):
        use = inside & (a >= 1) & (a <= W - 1) & (b >= 1) & (b <= H - 1)
    return angles_deg(sample(crop_image(pano, src, H, W), a, b, inside), crop_image(pano, dst, H, W), use), use


def angles_deg(p, q, use):
    p, q = p[use], q[use]
    c = (p * q).sum(-1) / (np.linalg.norm(p, axis=-1) * np.linalg.norm(q, axis=-1))
    return np.degrees(np.arccos(np.clip(c, -1, 1)))


# ---------------------------------------------------------------- the reference against itself
def test_case_list_is_the_stated_product():
    assert len(CASES) == 60 and len(set(CASES)) == 60
    assert all(d[4] == 0 and d[5] == 0 for _, d in CASES)


@pytest.mark.parametrize("size", SIZES)
def test_source_point_and_destination_pixel_share_their_world_ray(size):
    Hs, Ws, H, W = size
    worst = 0.0
    for s, d in CASES:
        s, d = theta_rad(*s), theta_rad(*d)
        a, b, inside = source_coords(s, Hs, Ws, d, H, W)
        Fs, Cxs, Cys = intrinsics(s[3], s[4], s[5], Hs, Ws)
        Fd, Cxd, Cyd = intrinsics(d[3], d[4], d[5], H, W)
        ws, ok_s = world_rays(s, (a[inside] - Cxs) / Fs, (b[inside] - Cys) / Fs)
        cols, rows = np.meshgrid(np.arange(W) + 0.5, np.arange(H) + 0.5)
        wd, ok_d = world_rays(d, (cols[inside] - Cxd) / Fd, (rows[inside] - Cyd) / Fd)
        assert ok_s.all() and ok_d.all()
        worst = max(worst, np.abs(ws - wd).max())
    assert worst <= 1e-12, worst


def test_yaw_matrix_is_the_longitude_of_the_panorama_crop():
    for s, _ in CASES[::7]:
        th = theta_rad(*s)
        _, _, Xw, ok = sample_coords(th, 20, 30, 64, 128)
        u, _, _, _ = sample_coords(th, 20, 30, 64, 128)
        Xy = Xw @ yaw_matrix(th[2]).T
        lon = np.arctan2(Xy[..., 0], Xy[..., 2])
        lon_u = ((u + 0.5) / 128 - 0.5) * 2 * np.pi
        dl = np.abs((lon - lon_u + np.pi) % (2 * np.pi) - np.pi)
        assert ok.any() and dl[ok].max() <= 1e-12, dl[ok].max()


@pytest.mark.parametrize("xi", [0.0, 0.5, 1.0, 1.3])
def test_unprojected_rays_are_the_visible_ones_and_project_back(xi):
    rng = np.random.default_rng(int(xi * 10) + 1)
    x, y = rng.uniform(-3, 3, (2, 4000))
    X, ok = unproject(x, y, xi)
    assert ok.any() and (X[ok][:, 2] > z_min(xi)).all()
    assert np.abs(project(X[ok], xi) - np.stack([x, y], -1)[ok]).max() <= 1e-12
    # and the other way: a ray above the limit projects to a point whose ray it is
    v = rng.normal(size=(4000, 3))
    v /= np.linalg.norm(v, axis=-1, keepdims=True)
    v = v[v[:, 2] > z_min(xi) + 1e-6]
    p = project(v, xi)
    back, okb = unproject(p[:, 0], p[:, 1], xi)
    assert okb.all() and np.abs(back - v).max() <= 1e-9


@pytest.mark.parametrize("xi", [0.0, 0.5, 1.3])
def test_same_camera_and_size_is_the_identity_map(xi):
    th = theta_rad(12.0, -20.0, 33.0, 0.45, 0.04, -0.03, xi)
    H, W = 37, 53
    a, b, inside = source_coords(th, H, W, th, H, W)
    cols, rows = np.meshgrid(np.arange(W) + 0.5, np.arange(H) + 0.5)
    _, ok = pixel_rays(th, H, W)
    assert np.array_equal(inside, ok) and inside.any()
    assert np.abs(a - cols)[inside].max() <= 1e-12 and np.abs(b - rows)[inside].max() <= 1e-12
    img = np.random.default_rng(0).integers(0, 256, (H, W, 3)).astype(np.float64)
    assert np.abs(sample(img, a, b, inside) - img)[inside].max() <= 1e-9


def test_sampling_replicates_the_edge_and_fills_outside():
    img = np.arange(4 * 5 * 3, dtype=np.float64).reshape(4, 5, 3)
    a, b = np.array([0.0, 0.2, 5.0, 2.5, 7.0]), np.array([0.0, 4.0, 3.9, 1.0, 1.0])
    inside = np.array([True, True, True, True, False])
    s = sample(img, a, b, inside, fill=0.5)
    assert np.allclose(s[0], img[0, 0]) and np.allclose(s[1], img[3, 0]) and np.allclose(s[2], img[3, 4])
    assert np.allclose(s[3], 0.5 * (img[0, 2] + img[1, 2])) and np.allclose(s[4], 0.5)


@pytest.mark.parametrize("size", SIZES)
def test_excluded_share_is_small_and_no_case_is_empty(size):
    Hs, Ws, H, W = size
    for s, d in CASES:
        s, d = theta_rad(*s), theta_rad(*d)
        _, _, inside = source_coords(s, Hs, Ws, d, H, W)
        assert (~clear(s, Hs, Ws, d, H, W)).mean() <= 0.01, (s, d)
        assert inside.mean() >= 0.10, (s, d)


@pytest.mark.parametrize("size", SIZES)
def test_fp32_floor_of_the_map(size):
    """the float32 evaluation agrees with fp64 on the NaN pattern of clear pixels; its error is the floor the GPU map is held to (x 4)"""
    e_in, e_out = fp32_floor(size)
    print(f"fp32 floor at {size}: {e_in:.3e} px inside, {e_out:.3e} normalised outside")
    assert 0 < e_in <= 1e-3 and e_out <= 1e-4   # fp32 epsilon times a coordinate of ~100 px; a looser floor would make the GPU check empty


def test_reference_closure_with_the_panorama_crop():
    from tests.test_gpu_pano_crop import direction_panorama

    pano = direction_panorama(512, 1024)
    for k in CLOSURE_CASES:
        s, d = theta_rad(*CASES[k][0]), theta_rad(*CASES[k][1])
        ang, use = closure_reference(pano, s, d, 96, 128)
        assert use.sum() >= 500 and ang.max() <= 0.05, (k, use.sum(), ang.max())


# ---------------------------------------------------------------- host-side contract (fails before the feature exists)
def test_reproject_image_is_exported():
    import perspectivefields_amd

    assert "reproject_image" in perspectivefields_amd.__all__
    assert callable(perspectivefields_amd.reproject_image)
    assert callable(perspectivefields_amd.PerspectiveFields.rectify)


CAM = dict(roll=0.0, pitch=0.0, rel_focal=1.0)


def test_reproject_image_on_cpu_tensors_raises():
    from perspectivefields_amd import reproject_image
    from perspectivefields_amd.engine import PfError

    for images in (torch.zeros((8, 16, 3), dtype=torch.uint8), torch.zeros((2, 8, 16, 3)), [torch.zeros((8, 16, 3))]):
        with pytest.raises(PfError):
            reproject_image(images, CAM, CAM)


def test_pf_reproject_rejects_bad_arguments_before_device_work():
    from perspectivefields_amd.engine import load_library

    lib = load_library()
    one = (ctypes.c_void_p * 1)(0x1000)
    hw = lambda *s: (ctypes.c_int32 * len(s))(*s)
    dev = ctypes.c_void_p(256)

    def call(n=1, p=one, hw_=None, dtype=0, idx=(0,), B=None, cs=dev, cd=dev, H=4, W=4, img=dev, c_idx=True):
        rc = lib.pf_reproject(0, n, p, hw_ or hw(8, 16), dtype, len(idx) if B is None else B, hw(*idx) if c_idx else None, cs, cd, H, W, 0.0, img, None, None, None)
        return rc, lib.pf_last_error(None).decode()

    for kw, what in ((dict(idx=(1,)), "index"), (dict(idx=(-1,)), "index"), (dict(dtype=2), "dtype"), (dict(hw_=hw(0, 16)), "smaller"), (dict(hw_=hw(8, 0)), "smaller"),
                     (dict(H=0), "size"), (dict(W=0), "size"), (dict(img=None), "required"), (dict(cs=None), "required"), (dict(cd=None), "required"),
                     (dict(c_idx=False), "required"), (dict(B=0), "required"), (dict(n=0), "at least one"), (dict(p=None), "at least one"),
                     (dict(p=(ctypes.c_void_p * 1)()), "NULL")):
        rc, msg = call(**kw)
        assert rc == -1 and what in msg and msg.startswith("pf_reproject"), (kw, rc, msg)


class FakeCuda:
    """a stand-in CUDA tensor: the checks read only .is_cuda, .dim(), .shape, .dtype and .device"""

    def __init__(self, shape, dtype=torch.uint8):
        self.shape, self.dtype, self.device, self.is_cuda = tuple(shape), dtype, torch.device("cuda", 0), True

    def dim(self):
        return len(self.shape)


def test_reproject_image_argument_errors_before_the_library_is_loaded(monkeypatch):
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
        dict(images=[ok, small]), dict(images=[ok, small], height=4), dict(height=0), dict(width=0, height=3), dict(mode="grad"),
        dict(src_index=[1]), dict(src_index=[-1]), dict(images=[ok, small], height=4, width=4, src_index=[0, 2]),
        dict(src=dict(roll=0.0, pitch=0.0)), dict(dst=dict(CAM, fov=1.0)), dict(src=dict(CAM, xi=np.zeros((2, 2)))),
        dict(src=dict(CAM, roll=[1.0, 2.0]), dst=dict(CAM, pitch=[1.0, 2.0, 3.0])), dict(images=[ok, ok, ok], src=dict(CAM, roll=[1.0, 2.0])),
        dict(src_index=[0, 0, 0], dst=dict(CAM, roll=[1.0, 2.0])),
    ]
    for kw in bad:
        args = dict(images=ok, src=CAM, dst=CAM)
        args.update(kw)
        with pytest.raises(ValueError):
            pfm.reproject_image(args.pop("images"), args.pop("src"), args.pop("dst"), **args)
    with pytest.raises(TypeError):
        pfm.reproject_image(ok, (0.0, 0.0, 1.0), CAM)
    with pytest.raises(TypeError):
        pfm.reproject_image([ok, np.zeros((8, 16, 3))], CAM, CAM)


def test_rectify_argument_errors_without_a_gpu():
    from perspectivefields_amd import PerspectiveFields
    from perspectivefields_amd.engine import PfError

    ok = FakeCuda((8, 16, 3))
    fields_only = dict(pred_gravity_original=None, pred_latitude_original=None)
    with pytest.raises(PfError, match="fit_camera"):
        PerspectiveFields.rectify(None, ok, fields_only)
    full = dict(pred_roll=1.0, pred_pitch=2.0, pred_rel_focal=0.8)
    with pytest.raises(ValueError):
        PerspectiveFields.rectify(None, ok, full, level="pitch")
    with pytest.raises(ValueError):
        PerspectiveFields.rectify(None, ok, full, mode="rad")
    with pytest.raises(ValueError):
        PerspectiveFields.rectify(None, ok, [])


def test_reproject_kernels_are_in_the_library_without_scratch():
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
        for extras in ("false", "true"):
            r = by[f"pf::reproject_kernel<{t}, {extras}>"]
            assert r["spill"] == 0 and r["scratch"] == 0 and r["lds"] <= 128, r
