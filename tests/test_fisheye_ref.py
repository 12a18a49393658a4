"""fp64 numpy statement of fisheye and dual-fisheye frames as a source (include/pf_hip.h pf_fisheye_crop / pf_fisheye_to_pano),
built on the conventions of tests/test_pano_crop_ref.py, tests/test_pano_rotate_ref.py and tests/test_cubemap_ref.py: the lens model (angle, point,
coverage, weight, colour), the blend of two lenses, views and panoramas out of a frame; checks of that reference against itself; the same formulas
in numpy float32 in the order of fisheye_gather.hip (the rounding floor the GPU results are measured against); which pixels are left out of the
accuracy comparisons and how few they are; the fixed inputs of tests/test_gpu_fisheye.py; plus the host-side contract of fisheye_lens /
dual_fisheye_lenses / crop_fisheye / fisheye_to_panorama and of the two C entry points (no GPU needed)."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

from tests.test_cubemap_ref import block_mean, pano_out_directions, view_directions, view_rad
from tests.test_pano_compose_ref import pano_directions
from tests.test_pano_crop_ref import pixel_rays, project as usm_project
from tests.test_pano_rotate_ref import _rot_matrix_f32, rot_matrix, rot_rad
from tests.test_reproject_ref import FakeCuda, sample

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# ---------------------------------------------------------------- the lens model in fp64
EQUIDISTANT, EQUISOLID, STEREOGRAPHIC = 0, 1, 2
KIND_NAMES = ("equidistant", "equisolid", "stereographic")
ROLL, PITCH, YAW, FOCAL, CX, CY, TMAX, K1, K2, K3, K4, BAND = range(12)


def rho(kind, t):
    return t if kind == EQUIDISTANT else 2.0 * np.sin(0.5 * t) if kind == EQUISOLID else 2.0 * np.tan(0.5 * t)


def rho_inverse(kind, r):
    return r if kind == EQUIDISTANT else 2.0 * np.arcsin(0.5 * r) if kind == EQUISOLID else 2.0 * np.arctan(0.5 * r)


def distort(lens, t):
    """theta_d = theta (1 + theta^2 (k1 + theta^2 (k2 + theta^2 (k3 + theta^2 k4)))), Horner-wise as written"""
    t2 = t * t
    return t * (1.0 + t2 * (lens[K1] + t2 * (lens[K2] + t2 * (lens[K3] + t2 * lens[K4]))))


def lens_row(kind, roll, pitch, yaw, tmax, band, center, radius=None, F=None, k=(0.0, 0.0, 0.0, 0.0)):
    """a lens row in fp64 from degrees: F given, or F = radius / rho(theta_d(theta_max))"""
    row = np.array([np.radians(roll), np.radians(pitch), np.radians(yaw), 0.0, center[0], center[1], np.radians(tmax), *k, np.radians(band)])
    row[FOCAL] = F if F is not None else radius / rho(kind, distort(row, row[TMAX]))
    return row


def lens_on(lens):
    return bool(np.isfinite(lens).all() and lens[TMAX] > 0)


def lens_project(lens, kind, D):
    """world directions D (..., 3) -> (theta, a, b) of the lens: steps 1 and 2"""
    X = D @ rot_matrix(lens[:3])   # Q^T D
    h = np.hypot(X[..., 0], X[..., 1])
    th = np.arctan2(h, X[..., 2])
    r = lens[FOCAL] * rho(kind, distort(lens, th))
    with np.errstate(invalid="ignore", divide="ignore"):
        a = np.where(h > 0, lens[CX] + r * X[..., 0] / h, lens[CX])
        b = np.where(h > 0, lens[CY] + r * X[..., 1] / h, lens[CY])
    return th, a, b


def lens_unproject(lens, kind, a, b, newton=False):
    """the inverse of lens_project for points inside the image circle: closed form for k = 0, a Newton iteration on theta_d(theta) otherwise"""
    dx, dy = a - lens[CX], b - lens[CY]
    r = np.hypot(dx, dy)
    td = rho_inverse(kind, r / lens[FOCAL])
    th = td.copy()
    if newton:
        for _ in range(60):
            t2 = th * th
            d = 1.0 + t2 * (3 * lens[K1] + t2 * (5 * lens[K2] + t2 * (7 * lens[K3] + t2 * 9 * lens[K4])))
            th = th - (distort(lens, th) - td) / d
    with np.errstate(invalid="ignore", divide="ignore"):
        X = np.stack([np.where(r > 0, np.sin(th) * dx / r, 0.0), np.where(r > 0, np.sin(th) * dy / r, 0.0), np.cos(th)], -1)
    return X @ rot_matrix(lens[:3]).T


def lens_covers(lens, th, a, b, Hs, Ws):
    """step 3: positive comparisons only; a lens that is off covers nothing"""
    if not lens_on(lens):
        return np.zeros(np.shape(th), bool)
    with np.errstate(invalid="ignore"):
        return (lens[TMAX] - th > 0) & (a >= 0) & (a <= Ws) & (b >= 0) & (b <= Hs)


def lens_weight(lens, th):
    """step 4"""
    return np.minimum((lens[TMAX] - th) / lens[BAND], 1.0) if lens[BAND] > 0 else np.ones(np.shape(th))


def frame_value(frame, lenses, kind, D, ok=None):
    """the value of a frame in the directions D (..., 3) where `ok` (default: everywhere): (value (..., 3), 0 where not valid; valid; S; number of
    covering lenses)"""
    Hs, Ws = frame.shape[:2]
    ok = np.ones(D.shape[:-1], bool) if ok is None else ok
    D = np.where(ok[..., None], D, np.array([0.0, 0.0, 1.0]))
    S, C, n = np.zeros(D.shape[:-1]), np.zeros(D.shape), np.zeros(D.shape[:-1], np.int64)
    for lens in lenses:
        th, a, b = lens_project(lens, kind, D)
        cov = lens_covers(lens, th, a, b, Hs, Ws) & ok
        w = np.where(cov, lens_weight(lens, th), 0.0)
        S += w
        C += w[..., None] * sample(frame, a, b, cov)
        n += cov
    valid = S > 0
    return np.where(valid[..., None], C / np.where(valid, S, 1.0)[..., None], 0.0), valid, S, n


def block_mean_fill(fine, valid, S, fill):
    n = valid.reshape(valid.shape[0] // S, S, valid.shape[1] // S, S).sum((1, 3))
    return np.where((n > 0)[..., None], block_mean(fine, valid, S), float(fill)), n > 0


def crop_frame(frame, lenses, kind, theta, H, W, S=1, fill=0.0):
    """the view in fp64 before any rounding and its mask; `fill` for non-finite parameters"""
    if not np.isfinite(np.asarray(theta, dtype=np.float64)).all():
        return np.full((H, W, 3), float(fill)), np.zeros((H, W), bool)
    D, ok = view_directions(theta, S * H, S * W)
    value, valid, _, _ = frame_value(frame, lenses, kind, D, ok)
    return block_mean_fill(value, valid, S, fill)


def frame_to_pano(frame, lenses, kind, theta, inverse, H, W, S=1, fill=0.0):
    if not np.isfinite(np.asarray(theta, dtype=np.float64)).all():
        return np.full((H, W, 3), float(fill)), np.zeros((H, W), bool)
    value, valid, _, _ = frame_value(frame, lenses, kind, pano_out_directions(theta, inverse, S * H, S * W))
    return block_mean_fill(value, valid, S, fill)


# ---------------------------------------------------------------- the same formulas in numpy float32, in the order of fisheye_gather.hip
def view_rays_f32(theta, H, W):
    """(camera rays (H, W, 3) float32, has_ray, Qc float32): pf_pano_crop's ray as cube_gather.hip and fisheye_gather.hip compute it"""
    f = np.float32
    r, p, yaw, fo, cx, cy, xi = [f(x) for x in theta]
    inv_f = f(1) / (fo * f(H))
    x = (np.arange(W, dtype=f)[None, :] + f(0.5) - (cx + f(0.5)) * f(W)) * inv_f + np.zeros((H, 1), f)
    y = (np.arange(H, dtype=f)[:, None] + f(0.5) - (cy + f(0.5)) * f(H)) * inv_f + np.zeros((1, W), f)
    r2 = x * x + y * y
    disc = f(1) + (f(1) - xi * xi) * r2
    with np.errstate(invalid="ignore"):
        eta = (xi + np.sqrt(np.where(disc >= 0, disc, f(np.nan)))) / (f(1) + r2)
    C = np.stack([eta * x, eta * y, eta - xi], -1)
    assert C.dtype == f
    return C, disc >= 0, _rot_matrix_f32((r, p, yaw), False)


def pano_dirs_f32(theta, inverse, H, W):
    """(panorama directions (H, W, 3) float32 before the rotation, A float32)"""
    f = np.float32
    lon = ((np.arange(W, dtype=f) + f(0.5)) / f(W) - f(0.5)) * f(2 * np.pi)
    lat = (f(0.5) - (np.arange(H, dtype=f) + f(0.5)) / f(H)) * f(np.pi)
    lat, lon = np.meshgrid(lat, lon, indexing="ij")
    sl, cl, so, co = np.sin(lat), np.cos(lat), np.sin(lon), np.cos(lon)
    D = np.stack([cl * so, -sl, cl * co], -1)
    assert D.dtype == f
    return D, _rot_matrix_f32(theta, inverse)


def lens_eval_f32(lens, kind, v, A, Hs, Ws):
    """float32 vectors v (camera rays or panorama directions) and their matrix into the world A -> (theta, a, b, covered, weight) float32: the
    kernel's order, M = Ql^T A first, then one product per sample"""
    f = np.float32
    L = lens.astype(f)
    M = _rot_matrix_f32(L[:3], False).T @ A
    X = v @ M.T
    assert X.dtype == f
    h = np.sqrt(X[..., 0] * X[..., 0] + X[..., 1] * X[..., 1])
    th = np.arctan2(h, X[..., 2])
    t2 = th * th
    td = th * (t2 * (t2 * (t2 * (t2 * L[K4] + L[K3]) + L[K2]) + L[K1]) + f(1))
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        r = td if kind == EQUIDISTANT else f(2) * np.sin(td * f(0.5)) if kind == EQUISOLID else f(2) * np.tan(td * f(0.5))
        s = L[FOCAL] * r / h
        a = np.where(h > 0, s * X[..., 0] + L[CX], L[CX])
        b = np.where(h > 0, s * X[..., 1] + L[CY], L[CY])
        margin = L[TMAX] - th
        cov = (margin > 0) & (a >= 0) & (a <= f(Ws)) & (b >= 0) & (b <= f(Hs)) if lens_on(L) else np.zeros(th.shape, bool)
        w = np.minimum(margin / L[BAND], f(1)) if L[BAND] > 0 else np.ones(th.shape, f)
    assert th.dtype == f and a.dtype == f and b.dtype == f and w.dtype == f
    return th, a, b, cov, w


# ---------------------------------------------------------------- the floor, the pixels left out, the allowed error
BORDER_PX, S_MIN = 1e-3, 1e-3


def case_floor(lenses, kind, Hs, Ws, D, ok, v32, ok32, A32):
    """one output: fp64 directions / has_ray and the float32 vectors of the same pixels -> dict with
    kept      the pixels that are compared: every pixel but those where (1) fp64 and float32 disagree on a lens's coverage (a pixel without a ray is covered by no lens), (2) |theta - theta_max| <
              max(4 x the float32 floor of theta, 1e-5) rad for a lens, (3) the fp64 (a, b) of a lens lies within 1e-3 px of the frame's border,
              (4) 0 < S_ref < 1e-3
    left      the share of the output left out by the rules 1-3 and by the rule 4
    e_c, e_w  the float32 floors: the largest coordinate error in px and the largest weight error over the pixels a lens covers in both precisions
    n, S      covering lenses and the summed weight per pixel in fp64"""
    D = np.where(ok[..., None], D, np.array([0.0, 0.0, 1.0]))
    v32 = np.where(ok32[..., None], v32, np.float32([0.0, 0.0, 1.0]))
    out123 = np.zeros(ok.shape, bool)
    S, n = np.zeros(ok.shape), np.zeros(ok.shape, np.int64)
    e_c = e_w = 0.0
    for lens in lenses:
        if not lens_on(lens):
            continue
        th, a, b = lens_project(lens, kind, D)
        cov = lens_covers(lens, th, a, b, Hs, Ws) & ok
        w = np.where(cov, lens_weight(lens, th), 0.0)
        th32, a32, b32, cov32, w32 = lens_eval_f32(lens, kind, v32, A32, Hs, Ws)
        cov32 = cov32 & ok32
        both = ok & ok32
        e_t = float(np.abs(th32 - th)[both].max()) if both.any() else 0.0
        out123 |= cov != cov32
        out123 |= both & (np.abs(th - lens[TMAX]) < max(4.0 * e_t, 1e-5))
        inside_fov = both & (lens[TMAX] - th > 0)
        with np.errstate(invalid="ignore"):
            out123 |= inside_fov & ((np.abs(a) < BORDER_PX) | (np.abs(a - Ws) < BORDER_PX) | (np.abs(b) < BORDER_PX) | (np.abs(b - Hs) < BORDER_PX))
        m = cov & cov32
        if m.any():
            e_c = max(e_c, float(np.abs(a32 - a)[m].max()), float(np.abs(b32 - b)[m].max()))
            e_w = max(e_w, float(np.abs(w32 - w)[m].max()))
        S += w
        n += cov
    out4 = (S > 0) & (S < S_MIN)
    return dict(kept=~(out123 | out4), left=(float(out123.mean()), float((out4 & ~out123).mean())), e_c=e_c, e_w=e_w, n=n, S=S)


def image_bound(case, grad, value_range=1.0):
    """allowed error per pixel of the float32 image (DESIGN.md section 19's rule): (covering lenses x coordinate floor x largest gradient x 2) +
    (covering lenses x weight floor x value range) / S_ref + 1e-6"""
    with np.errstate(divide="ignore", invalid="ignore"):
        return case["n"] * case["e_c"] * grad * 2 + np.where(case["S"] > 0, case["n"] * case["e_w"] * value_range / case["S"], 0.0) + 1e-6


# ---------------------------------------------------------------- the fixed inputs of the GPU test
OFF = np.zeros(12)   # theta_max = 0: the unused second lens
# name -> ((Hs, Ws), kind, the two lens rows)
RIGS = {
    "A": ((41, 41), EQUIDISTANT, [lens_row(EQUIDISTANT, 7.0, -12.0, 20.0, 95.0, 10.0, (20.5, 20.5), radius=20.0), OFF]),
    "A-equisolid": ((41, 41), EQUISOLID, [lens_row(EQUISOLID, 7.0, -12.0, 20.0, 95.0, 10.0, (20.5, 20.5), radius=20.0), OFF]),
    "A-stereo": ((41, 41), STEREOGRAPHIC, [lens_row(STEREOGRAPHIC, 7.0, -12.0, 20.0, 85.0, 0.0, (20.5, 20.5), radius=20.0), OFF]),
    "B": ((24, 48), EQUIDISTANT, [lens_row(EQUIDISTANT, 3.0, 4.0, 10.0, 100.0, 20.0, (12.0, 12.0), radius=12.0),
                                  lens_row(EQUIDISTANT, -5.0, -4.0, 190.0, 100.0, 20.0, (36.0, 12.0), radius=12.0)]),
    "C": ((33, 47), EQUIDISTANT, [lens_row(EQUIDISTANT, 11.0, 25.0, -40.0, 80.0, 0.0, (25.3, 15.2), F=18.0, k=(-0.02, 0.003, -0.0004, 0.00002)), OFF]),
    "D": ((1, 1), EQUIDISTANT, [lens_row(EQUIDISTANT, 0.0, 0.0, 0.0, 90.0, 0.0, (0.5, 0.5), radius=0.5), OFF]),
}
RIG_NAMES = tuple(RIGS)
PANO_OUTPUTS = [(32, 64), (37, 75), (1, 17), (19, 1)]
PANO_ROTATIONS = [(0.0, 0.0, 0.0), (10.0, 20.0, 30.0), (-25.0, 50.0, 170.0)]   # (roll, pitch, yaw) degrees, each forward and inverse
PANO_CASES = [(rot, inverse) for rot in PANO_ROTATIONS for inverse in (False, True)]
VIEW_OUTPUTS = [(48, 64), (31, 47), (1, 1)]
# (roll, pitch, yaw [deg], rel_focal, rel_cx, rel_cy, xi)
VIEW_CAMERAS = [(5.0, 10.0, 15.0, 0.6, 0.0, 0.0, 0.0), (-20.0, -30.0, 100.0, 0.4, 0.1, -0.05, 0.8), (15.0, 35.0, 200.0, 0.5, 0.0, 0.0, 1.2)]


def rig_lenses(name):
    return np.stack(RIGS[name][2])


@functools.lru_cache(None)
def pano_case(name, rot, inverse, out, S=1):
    """the floor and the kept pixels of one panorama case; read only"""
    (Hs, Ws), kind, lenses = RIGS[name]
    th = rot_rad(*rot)
    H, W = S * out[0], S * out[1]
    ok = np.ones((H, W), bool)
    D32, A32 = pano_dirs_f32(th, inverse, H, W)
    return case_floor(lenses, kind, Hs, Ws, pano_out_directions(th, inverse, H, W), ok, D32, ok, A32)


@functools.lru_cache(None)
def view_case(name, cam, out, S=1):
    (Hs, Ws), kind, lenses = RIGS[name]
    th = view_rad(cam)
    H, W = S * out[0], S * out[1]
    D, ok = view_directions(th, H, W)
    C32, ok32, Q32 = view_rays_f32(th, H, W)
    return case_floor(lenses, kind, Hs, Ws, D, ok, C32, ok32, Q32)


SS_RIGS, SS_SAMPLES = ("A", "B"), (2, 3)   # the supersampling comparison: these rigs at PANO_OUTPUTS[1] and VIEW_OUTPUTS[1]


def block_kept(case, out, S):
    """the output pixels of a supersampled comparison that are compared: those whose S x S sub-pixels are all kept pixels of the fine case"""
    return case["kept"].reshape(out[0], S, out[1], S).all((1, 3))


def ss_pano_kept(name, rot, inverse, S):
    return block_kept(pano_case(name, rot, inverse, PANO_OUTPUTS[1], S), PANO_OUTPUTS[1], S)


def ss_view_kept(name, cam, S):
    return block_kept(view_case(name, cam, VIEW_OUTPUTS[1], S), VIEW_OUTPUTS[1], S)


# ---------------------------------------------------------------- the reference against itself
@pytest.mark.parametrize("kind", [EQUIDISTANT, EQUISOLID, STEREOGRAPHIC])
def test_project_after_unproject_closes_without_a_polynomial(kind):
    rng = np.random.default_rng(kind)
    lens = lens_row(kind, 17.0, -33.0, 140.0, 88.0, 0.0, (31.7, 22.4), radius=20.0)
    ang, rad = rng.uniform(0, 2 * np.pi, 2000), 20.0 * np.sqrt(rng.uniform(0, 1, 2000))
    a, b = lens[CX] + rad * np.cos(ang), lens[CY] + rad * np.sin(ang)
    th, a2, b2 = lens_project(lens, kind, lens_unproject(lens, kind, a, b))
    assert max(np.abs(a2 - a).max(), np.abs(b2 - b).max()) <= 1e-12 * 20.0 and th.max() <= lens[TMAX] + 1e-12
    centre = lens_project(lens, kind, rot_matrix(lens[:3]) @ np.array([0.0, 0.0, 1.0]))   # h = 0 up to rounding: the centre of the image circle
    assert abs(centre[1] - lens[CX]) <= 1e-12 and abs(centre[2] - lens[CY]) <= 1e-12


def test_project_after_unproject_closes_with_the_polynomial():
    lens = RIGS["C"][2][0]
    rng = np.random.default_rng(5)
    r_max = lens[FOCAL] * distort(lens, lens[TMAX])
    ang, rad = rng.uniform(0, 2 * np.pi, 2000), r_max * np.sqrt(rng.uniform(0, 1, 2000))
    a, b = lens[CX] + rad * np.cos(ang), lens[CY] + rad * np.sin(ang)
    _, a2, b2 = lens_project(lens, EQUIDISTANT, lens_unproject(lens, EQUIDISTANT, a, b, newton=True))
    assert max(np.abs(a2 - a).max(), np.abs(b2 - b).max()) <= 1e-12 * r_max


def test_the_stereographic_lens_is_the_usm_camera_of_xi_1_with_twice_the_focal():
    """pf_reproject's step 4 at xi = 1: x = X / (Z + |X|), a = F_s x + Cx, against r = F 2 tan(theta / 2) with F_s = 2 F"""
    lens = lens_row(STEREOGRAPHIC, 0.0, 0.0, 0.0, 120.0, 0.0, (40.0, 30.0), F=11.0)
    D = np.random.default_rng(2).normal(size=(4000, 3))
    D = D[D[:, 2] / np.linalg.norm(D, axis=-1) > np.cos(lens[TMAX])]
    _, a, b = lens_project(lens, STEREOGRAPHIC, D)
    xy = usm_project(D, 1.0)
    assert np.abs(a - (2 * 11.0 * xy[:, 0] + 40.0)).max() <= 1e-11 and np.abs(b - (2 * 11.0 * xy[:, 1] + 30.0)).max() <= 1e-11


def test_two_opposed_lenses_of_200_degrees_never_sum_below_1():
    front = lens_row(EQUIDISTANT, 0.0, 0.0, 0.0, 100.0, 20.0, (0.0, 0.0), radius=1.0)
    back = lens_row(EQUIDISTANT, 0.0, 0.0, 180.0, 100.0, 20.0, (0.0, 0.0), radius=1.0)
    D = np.random.default_rng(3).normal(size=(20000, 3))
    total = np.zeros(len(D))
    for lens in (front, back):
        th, _, _ = lens_project(lens, EQUIDISTANT, D)
        total += np.where(lens[TMAX] - th > 0, lens_weight(lens, th), 0.0)
    assert total.min() >= 1.0 - 1e-12 and total.max() <= 2.0
    th, _, _ = lens_project(front, EQUIDISTANT, D)
    overlap = np.abs(th - np.pi / 2) < np.radians(10.0)
    assert overlap.any() and np.abs(total[overlap] - 1.0).max() <= 1e-12 and (total[~overlap] >= 1.0).all()


def test_fisheye_lens_builds_the_row_and_rejects_what_is_not_a_lens():
    from perspectivefields_amd import dual_fisheye_lenses, fisheye_lens

    for kind, name in enumerate(KIND_NAMES):
        row = fisheye_lens(190.0, radius=20.0, center=(20.5, 20.5), projection=name, roll=7.0, pitch=-12.0, yaw=20.0, band=10.0)
        assert row.shape == (12,) and row.dtype == np.float64
        assert np.abs(row - lens_row(kind, 7.0, -12.0, 20.0, 95.0, 10.0, (20.5, 20.5), radius=20.0)).max() <= 1e-13
    rad = fisheye_lens(np.radians(160.0), radius=18.0, center=(25.3, 15.2), k=(-0.02, 0.003, -0.0004, 0.00002), yaw=np.radians(-40.0), mode="rad")
    assert np.abs(rad - lens_row(EQUIDISTANT, 0.0, 0.0, -40.0, 80.0, 0.0, (25.3, 15.2), radius=18.0, k=(-0.02, 0.003, -0.0004, 0.00002))).max() <= 1e-13
    with pytest.raises(ValueError, match="not strictly increasing"):
        fisheye_lens(180.0, radius=20.0, center=(20.0, 20.0), k=(-1.0, 0.0, 0.0, 0.0))   # theta (1 - theta^2) turns back at 0.577 rad
    with pytest.raises(ValueError, match="not strictly increasing"):
        fisheye_lens(200.0, radius=20.0, center=(20.0, 20.0), projection="stereographic", k=(0.5, 0.0, 0.0, 0.0))   # theta_d / 2 crosses the pole of tan
    for kw in (dict(fov=0.0), dict(fov=361.0), dict(radius=0.0), dict(band=-1.0), dict(projection="orthographic"), dict(k=(0.0, 0.0)), dict(mode="grad"),
               dict(yaw=np.nan), dict(center=(np.inf, 0.0))):
        args = dict(fov=180.0, radius=10.0, center=(10.0, 10.0))
        args.update(kw)
        with pytest.raises(ValueError):
            fisheye_lens(args.pop("fov"), **args)
    two = dual_fisheye_lenses(24, 48, 200.0, roll=3.0)
    assert two.shape == (2, 12)
    assert np.abs(two[0] - lens_row(EQUIDISTANT, 3.0, 0.0, 0.0, 100.0, 20.0, (12.0, 12.0), radius=12.0)).max() <= 1e-13
    assert np.abs(two[1] - lens_row(EQUIDISTANT, 3.0, 0.0, 180.0, 100.0, 20.0, (36.0, 12.0), radius=12.0)).max() <= 1e-13
    tall = dual_fisheye_lenses(20, 60, 190.0, projection="equisolid", yaw=30.0)
    assert tall[0, FOCAL] == 10.0 / rho(EQUISOLID, np.radians(95.0)) and np.allclose(tall[:, YAW], np.radians([30.0, 210.0]), atol=1e-15)
    assert np.allclose(tall[:, BAND], np.radians(10.0), atol=1e-15) and tall[1, CX] == 45.0 and tall[1, CY] == 10.0
    with pytest.raises(TypeError):
        dual_fisheye_lenses(24, 48, 200.0, radius=5.0)


def test_an_off_or_non_finite_lens_covers_nothing_and_the_blend_follows_the_lens_order():
    frame = np.random.default_rng(0).uniform(0, 1, (24, 48, 3))
    lenses = rig_lenses("B")
    D = pano_directions(16, 32)
    both, valid, S, n = frame_value(frame, lenses, EQUIDISTANT, D)
    assert valid.all() and n.max() == 2 and n.min() == 1 and S.min() >= 0.5
    first, v0, _, _ = frame_value(frame, [lenses[0], OFF], EQUIDISTANT, D)
    for k, bad in ((ROLL, np.nan), (FOCAL, np.inf), (BAND, -np.inf), (TMAX, 0.0), (TMAX, -1.0)):
        broken = lenses.copy()
        broken[1, k] = bad
        got, v, _, _ = frame_value(frame, broken, EQUIDISTANT, D)
        assert np.array_equal(got, first) and np.array_equal(v, v0) and not v.all()
    only = n == 1
    assert np.abs(both - first)[only & v0].max() <= 1e-15   # a single covering lens: its own sample, whatever its weight


def test_supersampling_is_the_block_mean_of_the_valid_sub_samples():
    (Hs, Ws), kind, lenses = RIGS["A"]
    frame = np.random.default_rng(1).uniform(0, 1, (Hs, Ws, 3))
    th = view_rad(VIEW_CAMERAS[2])
    fine, valid = crop_frame(frame, lenses, kind, th, 24, 32)
    assert valid.any() and not valid.all()
    coarse, any_valid = crop_frame(frame, lenses, kind, th, 12, 16, S=2, fill=0.25)
    want, want_any = block_mean_fill(fine, valid, 2, 0.25)
    assert np.array_equal(any_valid, want_any) and np.abs(coarse - want).max() <= 1e-15 and (coarse[~any_valid] == 0.25).all()


# ---------------------------------------------------------------- the float32 floor and the pixels left out
def test_at_most_1_percent_of_any_panorama_case_is_left_out():
    """the condition of tests/test_gpu_fisheye.py, asserted for every one of its inputs on the reference alone"""
    worst = (0.0, 0.0)
    for name in RIG_NAMES:
        for out in PANO_OUTPUTS:
            for rot, inverse in PANO_CASES:
                for S in ((1, 2, 3) if out == PANO_OUTPUTS[1] and name in ("A", "B") else (1,)):
                    c = pano_case(name, rot, inverse, out, S)
                    worst = (max(worst[0], c["left"][0]), max(worst[1], c["left"][1]))
                    assert 1.0 - c["kept"].mean() <= 0.01, (name, out, rot, inverse, S, c["left"])
    print(f"panoramas: at most {100 * worst[0]:.3f} % left out by coverage, theta_max and the border, {100 * worst[1]:.3f} % by S < 1e-3")


def test_at_most_1_percent_of_any_view_case_is_left_out():
    worst = (0.0, 0.0)
    for name in RIG_NAMES:
        for out in VIEW_OUTPUTS:
            for cam in VIEW_CAMERAS:
                for S in ((1, 2, 3) if out == VIEW_OUTPUTS[1] and name in ("A", "B") else (1,)):
                    c = view_case(name, cam, out, S)
                    worst = (max(worst[0], c["left"][0]), max(worst[1], c["left"][1]))
                    assert 1.0 - c["kept"].mean() <= 0.01, (name, out, cam, S, c["left"])
    print(f"views: at most {100 * worst[0]:.3f} % left out by coverage, theta_max and the border, {100 * worst[1]:.3f} % by S < 1e-3")


def test_at_most_1_percent_of_any_supersampled_output_is_left_out():
    """the same cap at the level of the output pixel: a pixel of a samples=S output is left out when any of its S x S sub-pixels is"""
    worst = 0.0
    for name in SS_RIGS:
        for S in SS_SAMPLES:
            for rot, inverse in PANO_CASES:
                left = 1.0 - ss_pano_kept(name, rot, inverse, S).mean()
                worst = max(worst, left)
                assert left <= 0.01, (name, rot, inverse, S, left)
            for cam in VIEW_CAMERAS:
                left = 1.0 - ss_view_kept(name, cam, S).mean()
                worst = max(worst, left)
                assert left <= 0.01, (name, cam, S, left)
    print(f"supersampled outputs: at most {100 * worst:.3f} % left out")


def test_fp32_floor_of_the_fixed_cases():
    """the float32 evaluation of the model is a few ulp of a coordinate of tens of px and of a weight of at most 1"""
    e_c = e_w = 0.0
    for name in RIG_NAMES:
        for rot, inverse in PANO_CASES:
            c = pano_case(name, rot, inverse, PANO_OUTPUTS[0])
            e_c, e_w = max(e_c, c["e_c"]), max(e_w, c["e_w"])
        for cam in VIEW_CAMERAS:
            c = view_case(name, cam, VIEW_OUTPUTS[0])
            e_c, e_w = max(e_c, c["e_c"]), max(e_w, c["e_w"])
    print(f"fp32 floor: coordinates {e_c:.3e} px, weights {e_w:.3e}")
    assert e_c <= 1e-4 and e_w <= 2e-5


# ---------------------------------------------------------------- host-side contract (fails before the feature exists)
NAMES = ("fisheye_lens", "dual_fisheye_lenses", "crop_fisheye", "fisheye_to_panorama")
ENTRY_POINTS = ("pf_fisheye_crop", "pf_fisheye_to_pano")


def test_names_are_exported_from_both_packages():
    import perspective2d
    import perspectivefields_amd

    for name in NAMES:
        assert name in perspectivefields_amd.__all__ and callable(getattr(perspectivefields_amd, name))
        assert getattr(perspective2d, name) is getattr(perspectivefields_amd, name)


def test_header_states_the_model_and_the_constants():
    from perspectivefields_amd import perspectivefields as pfm

    hdr = open(os.path.join(ROOT, "include", "pf_hip.h")).read()
    assert "int pf_fisheye_crop(int device, int n_frame, const void* const* h_frame, const int32_t* h_frame_hw" in hdr
    assert "int pf_fisheye_to_pano(int device, int n_frame, const void* const* h_frame, const int32_t* h_frame_hw" in hdr
    for text in ("#define PF_FISHEYE_MAX_LENSES 2", "#define PF_FISHEYE_EQUIDISTANT 0", "#define PF_FISHEYE_EQUISOLID 1", "#define PF_FISHEYE_STEREOGRAPHIC 2",
                 "{roll, pitch, yaw (RADIANS), F, Cx, Cy, theta_max, k1, k2, k3, k4, band}", "theta_max - theta > 0"):
        assert text in hdr, text
    assert pfm.FISHEYE_PROJECTIONS == dict(zip(KIND_NAMES, (EQUIDISTANT, EQUISOLID, STEREOGRAPHIC))) and pfm.FISHEYE_MAX_LENSES == 2 and pfm.FISHEYE_LENS_FLOATS == 12
    kh = open(os.path.join(ROOT, "perspectivefields_amd", "csrc", "pf_kernels.h")).read()
    assert "struct FisheyeCropBatch" in kh and "struct FisheyePanoBatch" in kh
    assert "offsetof(FisheyeCropBatch, src) == 32" in kh and "offsetof(FisheyePanoBatch, src) == 32" in kh


def test_symbols_and_prototypes_are_present():
    from perspectivefields_amd.engine import _SIGNATURES, declared_symbols, load_library

    assert all(name in declared_symbols() for name in ENTRY_POINTS)
    res, args = _SIGNATURES["pf_fisheye_crop"]
    assert res is ctypes.c_int and len(args) == 17 and args[5] is ctypes.c_int and args[12] is ctypes.c_float and args[15] is ctypes.c_int
    res, args = _SIGNATURES["pf_fisheye_to_pano"]
    assert res is ctypes.c_int and len(args) == 18 and args[10] is ctypes.c_int and args[13] is ctypes.c_float and args[16] is ctypes.c_int
    lib = load_library()
    assert all(hasattr(lib, name) for name in ENTRY_POINTS)


@pytest.mark.parametrize("name", ENTRY_POINTS)
def test_entry_points_reject_bad_arguments_before_device_work(name):
    from perspectivefields_amd.engine import load_library

    lib = load_library()
    frame = (ctypes.c_void_p * 1)(0x1000)
    ints = lambda *s: (ctypes.c_int32 * len(s))(*s)
    dev = ctypes.c_void_p(256)

    def call(hw=None, dtype=0, kind=0, idx=(0,), c_idx=True, H=4, W=8, img=dev, lens=dev, par=dev, n=1, p=frame, B=None, samples=1):
        head = (0, n, p, hw or ints(8, 9), dtype, kind, len(idx) if B is None else B, ints(*idx) if c_idx else None, lens, par)
        mid = () if name == "pf_fisheye_crop" else (0,)
        rc = getattr(lib, name)(*head, *mid, H, W, 0.0, img, None, samples, None)
        return rc, lib.pf_last_error(None).decode()

    # the stated order: samples, then kind, then gather_run's checks; each later error is given together with every earlier-checked argument right
    for kw, what in ((dict(samples=0, kind=3, lens=None), "samples"), (dict(samples=5, kind=-1, hw=ints(0, 8)), "samples"), (dict(kind=3, lens=None), "kind"),
                     (dict(kind=-1, hw=ints(8, 0), idx=(1,)), "kind"), (dict(lens=None), "required"), (dict(hw=ints(0, 8)), "smaller"), (dict(hw=ints(8, 0)), "smaller"),
                     (dict(idx=(1,)), "index"), (dict(idx=(-1,)), "index"), (dict(H=0), "size"), (dict(W=0), "size"),
                     (dict(dtype=2), "dtype"), (dict(img=None), "required"), (dict(par=None), "required"), (dict(c_idx=False), "required"), (dict(B=0), "required"),
                     (dict(p=(ctypes.c_void_p * 1)()), "NULL"), (dict(p=None), "at least one"), (dict(n=0), "at least one")):
        rc, msg = call(**kw)
        assert rc == -1 and what in msg and msg.startswith(name + ": "), (kw, rc, msg)
    for kind in (EQUIDISTANT, EQUISOLID, STEREOGRAPHIC):   # a 1 x 1 frame and every kind are good arguments: they fail on the missing device only
        if not torch.cuda.is_available():
            rc, msg = call(kind=kind, hw=ints(1, 1))
            assert rc == -2 and "no HIP device" in msg, (rc, msg)


def test_fisheye_functions_on_cpu_tensors_raise():
    from perspectivefields_amd import crop_fisheye, fisheye_to_panorama
    from perspectivefields_amd.engine import PfError

    frame = torch.zeros((8, 16, 3), dtype=torch.uint8)
    with pytest.raises(PfError):
        crop_fisheye(frame, rig_lenses("B"), 0.0, 0.0, 0.5, height=4, width=4)
    with pytest.raises(PfError):
        fisheye_to_panorama([frame], rig_lenses("A")[0], height=4, width=8)


def test_python_argument_errors_before_the_library_is_loaded(monkeypatch):
    from perspectivefields_amd import engine
    from perspectivefields_amd import perspectivefields as pfm

    def no_library(*a, **k):
        raise AssertionError("the library was loaded before the arguments were checked")

    monkeypatch.setattr(engine, "load_library", no_library)
    monkeypatch.setattr(pfm.torch, "is_tensor", lambda v: isinstance(v, (torch.Tensor, FakeCuda)))
    ok = FakeCuda((8, 16, 3))
    row = rig_lenses("A")[0]
    bad_frames = [FakeCuda((8, 16, 4)), FakeCuda((8, 16)), FakeCuda((0, 16, 3)), FakeCuda((8, 16, 3), torch.float16), [ok, FakeCuda((8, 16, 3), torch.float32)], []]
    bad_lenses = [np.zeros(11), np.zeros((3, 12)), np.zeros((2, 13)), [np.zeros((2, 12)), np.zeros((2, 12))], np.zeros((2, 2, 12))]   # the last two: 2 entries, 1 frame
    common = [dict(samples=0), dict(samples=5), dict(samples=2.0), dict(frame_index=[1]), dict(frame_index=[-1]), dict(frame_index=[0, 0]), dict(mode="grad"),
              dict(height=0), dict(width=0), dict(projection="orthographic")] + [dict(frames=f) for f in bad_frames] + [dict(lenses=l) for l in bad_lenses]
    for kw in common + [dict(roll=[1.0, 2.0], pitch=[1.0, 2.0, 3.0]), dict(xi=np.zeros((2, 2)))]:
        args = dict(frames=ok, lenses=row, roll=0.0, pitch=0.0, rel_focal=0.5, height=4, width=8)
        args.update(kw)
        with pytest.raises(ValueError):
            pfm.crop_fisheye(args.pop("frames"), args.pop("lenses"), args.pop("roll"), args.pop("pitch"), args.pop("rel_focal"), **args)
    for kw in common + [dict(roll=[1.0, 2.0], yaw=[1.0, 2.0, 3.0]), dict(yaw=np.zeros((2, 2)))]:
        args = dict(frames=ok, lenses=row, height=4, width=8)
        args.update(kw)
        with pytest.raises(ValueError):
            pfm.fisheye_to_panorama(args.pop("frames"), args.pop("lenses"), **args)
    with pytest.raises(TypeError):
        pfm.crop_fisheye([ok, np.zeros((8, 16, 3))], row, 0.0, 0.0, 0.5, height=4, width=4)
    with pytest.raises(TypeError):
        pfm.fisheye_to_panorama(ok, row)   # height and width are required


def test_lens_tables_expand_to_one_entry_per_frame():
    from perspectivefields_amd import perspectivefields as pfm

    a, b = rig_lenses("A")[0], rig_lenses("B")
    one = pfm._fisheye_lens_table("t", a, 3)
    assert one.shape == (3, 2, 12) and np.array_equal(one[2, 0], a) and (one[:, 1] == 0).all()
    pair = pfm._fisheye_lens_table("t", torch.from_numpy(b), 2)
    assert np.array_equal(pair[0], b) and np.array_equal(pair[1], b)
    per = pfm._fisheye_lens_table("t", [a[None], b], 2)
    assert np.array_equal(per[0, 0], a) and (per[0, 1] == 0).all() and np.array_equal(per[1], b)
    per = pfm._fisheye_lens_table("t", np.stack([b, b[::-1]]), 2)
    assert np.array_equal(per[1], b[::-1])


def test_fisheye_kernels_are_in_the_library_without_scratch():
    """scripts/kernel_resources.py on the built library: every instantiation is there for gfx950 with no spilled register and no scratch"""
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
    for name in [f"pf::{k}<{t}>" for k in ("fisheye_crop_kernel", "fisheye_to_pano_kernel") for t in ("unsigned char", "float")]:
        r = by[name]
        assert r["spill"] == 0 and r["scratch"] == 0 and r["lds"] <= 256 and r["vgpr"] <= 128, r
