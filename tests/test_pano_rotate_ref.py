"""fp64 numpy statement of the rotation of equirectangular panoramas and of the perspective fields of a panoramic camera (include/pf_hip.h
pf_pano_rotate / pf_pano_fields), built on the conventions of tests/test_pano_crop_ref.py and
tests/test_pano_compose_ref.py: the source point of every output pixel, the image, the labels; checks of that reference against itself and
against the conventions; the same formulas in numpy float32 (the rounding floor the GPU results are measured against); the fixed inputs of
tests/test_gpu_pano_rotate.py; gravity_from_views on CPU tensors; plus the host-side contract of rotate_panorama / panorama_fields /
level_panorama and of the two C entry points (no GPU needed)."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

from tests.test_pano_compose_ref import pano_directions
from tests.test_pano_crop_ref import bilinear, rotation
from tests.test_reproject_ref import FakeCuda, yaw_matrix

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R2D = 180.0 / np.pi
UP = np.array([0.0, -1.0, 0.0])


def rot_rad(roll, pitch, yaw):
    return (np.radians(roll), np.radians(pitch), np.radians(yaw))


def rot_matrix(theta, inverse=False):
    """theta = (roll, pitch, yaw) in radians -> A = Q = Y(yaw) R(roll, pitch), or Q^T with `inverse`"""
    Q = yaw_matrix(theta[2]) @ rotation(theta[0], theta[1])
    return Q.T if inverse else Q


def pixel_angles(H, W):
    lon = ((np.arange(W) + 0.5) / W - 0.5) * 2 * np.pi
    lat = (0.5 - (np.arange(H) + 0.5) / H) * np.pi
    return np.meshgrid(lat, lon, indexing="ij")


def point_of(X, Hs, Ws):
    """directions X (..., 3) -> the source point (u, v) in pixel-centre units of an Hs x Ws panorama, and lat_s in radians"""
    lat_s = -np.arctan2(X[..., 1], np.hypot(X[..., 0], X[..., 2]))
    lon_s = np.arctan2(X[..., 0], X[..., 2])
    return (lon_s / (2 * np.pi) + 0.5) * Ws - 0.5, (0.5 - lat_s / np.pi) * Hs - 0.5, lat_s


def source_coords(theta, inverse, H, W, Hs, Ws):
    """(u, v) of every pixel of the H x W output in the Hs x Ws source, and its latitude label in degrees"""
    u, v, lat_s = point_of(pano_directions(H, W) @ rot_matrix(theta, inverse).T, Hs, Ws)
    return u, v, lat_s * R2D


def rotate_image(src, theta, inverse, H, W):
    """the rotated panorama in fp64, before any rounding; non-finite theta: 0"""
    if not np.isfinite(np.asarray(theta, dtype=np.float64)).all():
        return np.zeros((H, W, 3))
    u, v, _ = source_coords(theta, inverse, H, W, src.shape[0], src.shape[1])
    return bilinear(src, u, v)


def fields(theta, inverse, H, W):
    """the labels in fp64: up (2, H, W), latitude (H, W) degrees, and |t| (H, W), the length of world up's part across the pixel's ray"""
    if not np.isfinite(np.asarray(theta, dtype=np.float64)).all():
        return np.full((2, H, W), np.nan), np.full((H, W), np.nan), np.full((H, W), np.nan)
    A = rot_matrix(theta, inverse)
    lat, lon = pixel_angles(H, W)
    D = pano_directions(H, W)
    g = A.T @ UP
    t = g - (D @ g)[..., None] * D
    e_lon = np.stack([np.cos(lon), np.zeros_like(lon), -np.sin(lon)], -1)
    e_lat = np.stack([-np.sin(lat) * np.sin(lon), -np.cos(lat), -np.sin(lat) * np.cos(lon)], -1)
    up = np.stack([W / (2 * np.pi) * (t * e_lon).sum(-1) / np.cos(lat), -H / np.pi * (t * e_lat).sum(-1)])
    with np.errstate(invalid="ignore", divide="ignore"):
        up = up / np.sqrt((up * up).sum(0))
    _, _, lat_s = point_of(D @ A.T, 2, 2)
    return up, lat_s * R2D, np.linalg.norm(t, axis=-1)


def pixel_of(D, H, W):
    """the inverse of pano_directions: directions -> (col, row) in pixel-centre units of the H x W panorama"""
    u, v, _ = point_of(D, H, W)
    return u, v


# ---------------------------------------------------------------- the same formulas in numpy float32, in the order of pano_rotate.hip
def _rot_matrix_f32(theta, inverse):
    f = np.float32
    r, p, y = [f(v) for v in theta]
    sr, cr, sp, cp, sy, cy = np.sin(r), np.cos(r), np.sin(p), np.cos(p), np.sin(y), np.cos(y)
    R = np.array([[cr, -sr, f(0)], [cp * sr, cp * cr, -sp], [sp * sr, sp * cr, cp]], dtype=f)
    Q = np.stack([cy * R[0] + sy * R[2], R[1], cy * R[2] - sy * R[0]])
    assert Q.dtype == f
    return Q.T.copy() if inverse else Q


def evaluate_f32(theta, inverse, H, W, Hs, Ws):
    """(u, v) float32, latitude label float32 (degrees), up float32 (2, H, W)"""
    f = np.float32
    A = _rot_matrix_f32(theta, inverse)
    lon = ((np.arange(W, dtype=f) + f(0.5)) / f(W) - f(0.5)) * f(2 * np.pi)
    lat = (f(0.5) - (np.arange(H, dtype=f) + f(0.5)) / f(H)) * f(np.pi)
    lat, lon = np.meshgrid(lat, lon, indexing="ij")
    sl, cl, so, co = np.sin(lat), np.cos(lat), np.sin(lon), np.cos(lon)
    D = np.stack([cl * so, -sl, cl * co], -1)
    X = D @ A.T
    nlat = np.arctan2(X[..., 1], np.sqrt(X[..., 0] * X[..., 0] + X[..., 2] * X[..., 2]))
    u = (np.arctan2(X[..., 0], X[..., 2]) * f(1 / (2 * np.pi)) + f(0.5)) * f(Ws) - f(0.5)
    v = (nlat * f(1 / np.pi) + f(0.5)) * f(Hs) - f(0.5)
    g = -A[1]
    a = g[0] * co - g[2] * so
    b = -(g[1] * cl + sl * (g[0] * so + g[2] * co))
    px, py = f(W) * f(1 / (2 * np.pi)) * a / cl, -(f(H) * f(1 / np.pi) * b)
    with np.errstate(invalid="ignore", divide="ignore"):
        n = np.sqrt(px * px + py * py)
        up = np.stack([px / n, py / n])
    lat_deg = -nlat * f(R2D)
    assert u.dtype == f and v.dtype == f and up.dtype == f and lat_deg.dtype == f
    return u, v, lat_deg, up


def wrap_px(d, Ws):
    """column differences modulo the panorama's width"""
    return (d + Ws / 2) % Ws - Ws / 2


def up_angle_deg(a, b):
    """angle in degrees between two fields of unit vectors (2, H, W)"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.degrees(np.arctan2(np.abs(a[0] * b[1] - a[1] * b[0]), a[0] * b[0] + a[1] * b[1]))


T_EXCLUDE = 1e-3   # up vectors are not compared where |t| of the reference is below this: the direction is ill-conditioned next to the zenith / nadir


def fp32_floor(theta, inverse, H, W, Hs, Ws):
    """errors of the float32 evaluation against fp64 for one case: (u in px x cos lat_s, v in px, latitude label in degrees, up in degrees away
    from the zenith / nadir).  The longitude of a source point is atan2(X.x, X.z): a rounding error of X moves it by that error over
    hypot(X.x, X.z) = cos lat_s, without bound next to the source's poles (a pixel centre on a pole has no longitude at all), so the floor of u
    is taken on the sphere, error x cos lat_s, and a pixel's own floor is that over its cos lat_s (u_floor_at)"""
    u, v, lat = source_coords(theta, inverse, H, W, Hs, Ws)
    up, _, tn = fields(theta, inverse, H, W)
    u32, v32, lat32, up32 = evaluate_f32(theta, inverse, H, W, Hs, Ws)
    use = tn >= T_EXCLUDE
    return (float((np.abs(wrap_px(u32 - u, Ws)) * np.cos(np.radians(lat))).max()), float(np.abs(v32 - v).max()), float(np.abs(lat32 - lat).max()),
            float(up_angle_deg(up32, up)[use].max()))


def u_floor_at(e_u, lat_deg, Ws):
    """a pixel's floor of u in px from the floor on the sphere: over cos lat_s, at most half the width (no two columns are further apart)"""
    with np.errstate(divide="ignore"):
        return np.minimum(e_u / np.cos(np.radians(lat_deg)), Ws / 2)


def local_steps(src, u, v):
    """per output pixel, the largest difference between horizontally and between vertically adjacent texels of `src` in the 4 x 4 window of
    texels around the sample (u, v) (columns wrap, rows clamp): the bilinear surface's gradient in the sample's cell and in every cell next to it"""
    Hs, Ws = src.shape[:2]
    P = src.astype(np.float64)
    c0, r0 = np.floor(u).astype(np.int64), np.floor(v).astype(np.int64)
    gu, gv = np.zeros(u.shape), np.zeros(u.shape)
    for dr in range(-1, 3):
        for dc in range(-1, 3):
            r, c = np.clip(r0 + dr, 0, Hs - 1), np.mod(c0 + dc, Ws)
            gu = np.maximum(gu, np.abs(P[r, np.mod(c + 1, Ws)] - P[r, c]).max(-1))
            gv = np.maximum(gv, np.abs(P[np.clip(r + 1, 0, Hs - 1), c] - P[r, c]).max(-1))
    return gu, gv


def image_bound(src, theta, inverse, H, W):
    """allowed error per pixel of the float32 image: 2 x (coordinate floor x local gradient) + 1e-6 (DESIGN.md section 17's rule), the floor
    being the error of the float32 evaluation of the same formulas, per coordinate, in the same run"""
    Hs, Ws = src.shape[:2]
    e_u, e_v, _, _ = fp32_floor(theta, inverse, H, W, Hs, Ws)
    u, v, lat = source_coords(theta, inverse, H, W, Hs, Ws)
    gu, gv = local_steps(src, u, v)
    return 2.0 * (u_floor_at(e_u, lat, Ws) * gu + e_v * gv) + 1e-6


def decompose(M):
    """a rotation M = Y(yaw) R_pitch(pitch) R_roll(roll) -> (roll, pitch, yaw) in radians, |pitch| <= 90 degrees"""
    return np.arctan2(M[1, 0], M[1, 1]), np.arcsin(np.clip(-M[1, 2], -1, 1)), np.arctan2(M[0, 2], M[2, 2])


# ---------------------------------------------------------------- the fixed inputs of the GPU test
SOURCES = [(32, 64), (40, 80)]
OUTPUTS = [(32, 64), (37, 75), (16, 32)]   # vector stores, scalar stores, a minification
EDGE_OUTPUTS = [(1, 17), (19, 1)]
ROTATIONS = [(20.0, 35.0, 50.0), (0.0, 90.0, 0.0), (-170.0, -80.0, 200.0), (0.0, 0.0, 0.0)]   # (roll, pitch, yaw) degrees


def direction_panorama(Hs, Ws):
    """a panorama whose pixel is its own direction: smooth, value range 2"""
    return pano_directions(Hs, Ws).astype(np.float32)


def u8_panorama(Hs, Ws, seed=0):
    """an analytic uint8 panorama: three smooth functions of the direction"""
    D = pano_directions(Hs, Ws)
    rng = np.random.default_rng(seed)
    M = rng.normal(size=(3, 3))
    return np.clip(np.round(127.5 + 100.0 * np.sin(2.0 * (D @ M.T))), 0, 255).astype(np.uint8)


def view_truth(tilt, n_yaw=8, pitches=(0.0, 30.0)):
    """views cut with (roll 0, pitch, yaw k 360 / n_yaw) out of a panorama whose camera has the orientation R(tilt): the views' cameras as
    level_panorama lays them out (degrees), and every view's true (roll, pitch) relative to gravity in degrees, from R(tilt) V_i = Y R_pitch R_roll"""
    Q = rotation(np.radians(tilt[0]), np.radians(tilt[1]))
    cams = {"roll": [0.0] * (n_yaw * len(pitches)), "pitch": [p for p in pitches for _ in range(n_yaw)],
            "yaw": [k * 360.0 / n_yaw for _ in pitches for k in range(n_yaw)]}
    true = [decompose(Q @ yaw_matrix(np.radians(y)) @ rotation(0.0, np.radians(p))) for p, y in zip(cams["pitch"], cams["yaw"])]
    return cams, np.degrees([t[0] for t in true]), np.degrees([t[1] for t in true])


@functools.lru_cache(None)
def floor_of(rot, inverse, out, src):
    return fp32_floor(rot_rad(*rot), inverse, *out, *src)


# ---------------------------------------------------------------- the reference against itself
@pytest.mark.parametrize("size", [(32, 64), (37, 75)])
def test_up_is_the_finite_difference_of_the_pixel_map_along_world_up(size):
    H, W = size
    D = pano_directions(H, W)
    for rot in ROTATIONS + [(5.0, -20.0, 130.0)]:
        for inverse in (False, True):
            th = rot_rad(*rot)
            up, _, tn = fields(th, inverse, H, W)
            g = rot_matrix(th, inverse).T @ UP
            u0, v0 = pixel_of(D, H, W)
            u1, v1 = pixel_of(D + 1e-6 * g, H, W)
            d = np.stack([wrap_px(u1 - u0, W), v1 - v0])
            with np.errstate(invalid="ignore"):
                d = d / np.sqrt((d * d).sum(0))
            use = tn >= T_EXCLUDE
            assert use.mean() >= 0.99
            assert np.abs(d - up)[:, use].max() <= 1e-4, (rot, inverse)


@pytest.mark.parametrize("size", [(32, 64), (37, 75), (1, 17), (19, 1)])
def test_upright_camera_has_up_0_minus_1_and_the_pixel_latitude(size):
    H, W = size
    lat, _ = pixel_angles(H, W)
    for inverse in (False, True):
        up, la, _ = fields((0.0, 0.0, 0.0), inverse, H, W)
        assert np.abs(up[0]).max() <= 1e-12 and np.abs(up[1] + 1).max() <= 1e-12
        assert np.abs(la - lat * R2D).max() <= 1e-12
    up, la, _ = fields(rot_rad(0.0, 0.0, 77.0), False, H, W)   # yaw alone keeps the camera upright
    assert np.abs(up[0]).max() <= 1e-12 and np.abs(up[1] + 1).max() <= 1e-12 and np.abs(la - lat * R2D).max() <= 1e-12


def test_direction_to_point_round_trips():
    for H, W in [(32, 64), (37, 75), (1, 17), (19, 1)]:
        u, v = pixel_of(pano_directions(H, W), H, W)
        assert np.abs(u - np.arange(W)[None, :]).max() <= 1e-12 * W and np.abs(v - np.arange(H)[:, None]).max() <= 1e-12 * H
    rng = np.random.default_rng(1)
    u, v = rng.uniform(-0.5, 63.5, 500), rng.uniform(-0.5, 31.5, 500)
    lon, lat = ((u + 0.5) / 64 - 0.5) * 2 * np.pi, (0.5 - (v + 0.5) / 32) * np.pi
    D = np.stack([np.cos(lat) * np.sin(lon), -np.sin(lat), np.cos(lat) * np.cos(lon)], -1)
    u2, v2 = pixel_of(D, 32, 64)
    assert np.abs(u2 - u).max() <= 1e-11 and np.abs(v2 - v).max() <= 1e-11


def test_zenith_hits_one_pixel_centre_at_pitch_90_on_37_x_75():
    _, _, tn = fields(rot_rad(0.0, 90.0, 0.0), False, 37, 75)
    hit = np.argwhere(tn < T_EXCLUDE)
    assert hit.tolist() == [[18, 37]]
    for out in OUTPUTS + EDGE_OUTPUTS:
        for rot in ROTATIONS:
            for inverse in (False, True):
                _, _, tn = fields(rot_rad(*rot), inverse, *out)
                n = int((tn < T_EXCLUDE).sum())
                if out in OUTPUTS:   # at most 1 % is left out; among these cases one pixel of 2775
                    assert n <= 0.01 * tn.size and (n == 0 or (out == (37, 75) and rot == (0.0, 90.0, 0.0))), (out, rot, inverse, n)
                else:   # the one-row and one-column outputs have their centre pixel on the zenith at pitch 90: one pixel, more than 1 % of 17 or 19
                    assert n <= 1 and (n == 0 or rot == (0.0, 90.0, 0.0)), (out, rot, inverse, n)


# ---------------------------------------------------------------- conventions
def test_a_yaw_of_whole_columns_is_a_roll_of_the_columns():
    rng = np.random.default_rng(3)
    src = rng.uniform(0, 1, (16, 32, 3))
    for k in (1, 5, -7, 32):
        out = rotate_image(src, rot_rad(0.0, 0.0, k * 360.0 / 32), False, 16, 32)
        assert np.abs(out - np.roll(src, -k, axis=1)).max() <= 1e-12   # the camera turns towards higher columns: they come to the centre
        back = rotate_image(src, rot_rad(0.0, 0.0, k * 360.0 / 32), True, 16, 32)
        assert np.abs(back - np.roll(src, k, axis=1)).max() <= 1e-12


def test_inverse_undoes_forward():
    for rot in ROTATIONS + [(5.0, -20.0, 130.0)]:
        th = rot_rad(*rot)
        assert np.abs(rot_matrix(th, True) @ rot_matrix(th, False) - np.eye(3)).max() <= 1e-15


def test_up_in_the_camera_gives_roll_and_pitch_back():
    for r, p in [(20.0, 35.0), (-170.0, -80.0), (0.0, 0.0), (91.0, 89.0), (-45.0, -10.0)]:
        d = rotation(np.radians(r), np.radians(p)).T @ UP
        assert abs(np.degrees(np.arctan2(d[2], np.hypot(d[0], d[1]))) - p) <= 1e-9
        dr = np.degrees(np.arctan2(-d[0], -d[1])) - r
        assert abs((dr + 180) % 360 - 180) <= 1e-9
    M = yaw_matrix(0.7) @ rotation(-0.3, 1.1)
    assert np.allclose(decompose(M), (-0.3, 1.1, 0.7), atol=1e-14)


def test_forward_is_the_view_of_a_camera_inside_the_source():
    """the output's centre pixel pair straddles the direction Q (0, 0, 1): for roll 0 the source point at longitude yaw and latitude pitch"""
    th = rot_rad(0.0, 30.0, 90.0)
    u, v, _ = point_of((rot_matrix(th) @ np.array([0.0, 0.0, 1.0]))[None], 8, 16)
    assert np.allclose([u[0], v[0]], [0.75 * 16 - 0.5, (0.5 - 30 / 180) * 8 - 0.5])


@pytest.mark.parametrize("out", OUTPUTS)
def test_fp32_floor_of_the_fixed_cases(out):
    """the float32 evaluation is close to fp64: its error is the floor the GPU results are held to; a looser floor would make the GPU check empty"""
    worst = np.zeros(4)
    for src in SOURCES:
        for rot in ROTATIONS:
            for inverse in (False, True):
                worst = np.maximum(worst, floor_of(rot, inverse, out, src))
    print(f"fp32 floor at {out}: u x cos lat_s {worst[0]:.3e} px, v {worst[1]:.3e} px, latitude {worst[2]:.3e} deg, up {worst[3]:.3e} deg")
    assert worst[0] <= 2e-4 and worst[1] <= 2e-5 and worst[2] <= 5e-5 and worst[3] <= 0.05


# ---------------------------------------------------------------- gravity_from_views on CPU tensors
TILT = (20.0, 35.0)


def test_gravity_from_views_recovers_the_tilt():
    from perspectivefields_amd import gravity_from_views

    cams, roll, pitch = view_truth(TILT)
    res = gravity_from_views(cams, roll, pitch)
    assert res["roll"].dtype == torch.float64 and res["votes"].shape == (16, 3) and res["inliers"].all()
    assert abs(float(res["roll"]) - TILT[0]) <= 1e-9 and abs(float(res["pitch"]) - TILT[1]) <= 1e-9
    assert float(res["angles"].max()) <= 1e-6
    g = rotation(np.radians(TILT[0]), np.radians(TILT[1])).T @ UP
    assert np.abs(res["direction"].numpy() - g).max() <= 1e-12 and np.abs(res["votes"].numpy() - g).max() <= 1e-12
    rad = gravity_from_views({k: np.radians(v) for k, v in cams.items()}, np.radians(roll), np.radians(pitch), mode="rad")
    assert abs(float(rad["roll"]) - np.radians(TILT[0])) <= 1e-11 and abs(float(rad["pitch"]) - np.radians(TILT[1])) <= 1e-11


def test_gravity_from_views_flags_outliers_and_honours_weights():
    from perspectivefields_amd import gravity_from_views

    cams, roll, pitch = view_truth(TILT)
    pitch_bad = pitch.copy()
    pitch_bad[[3, 12]] += 60.0   # R(r, p + 60)^T up is exactly 60 degrees from R(r, p)^T up
    res = gravity_from_views(cams, roll, pitch_bad)
    assert res["inliers"].tolist() == [k not in (3, 12) for k in range(16)]
    assert abs(float(res["roll"]) - TILT[0]) <= 1e-9 and abs(float(res["pitch"]) - TILT[1]) <= 1e-9
    assert np.abs(res["angles"].numpy()[[3, 12]] - 60.0).max() <= 1e-6
    # without the re-average the outliers pull the mean; a weight of 0 takes them out again
    loose = gravity_from_views(cams, roll, pitch_bad, max_dev=180.0)
    assert abs(float(loose["pitch"]) - TILT[1]) > 1.0
    w = np.ones(16)
    w[[3, 12]] = 0.0
    weighted = gravity_from_views(cams, roll, pitch_bad, max_dev=180.0, weights=w)
    assert abs(float(weighted["roll"]) - TILT[0]) <= 1e-9 and abs(float(weighted["pitch"]) - TILT[1]) <= 1e-9
    # two votes, weights 3 : 1: the mean direction is 3 v0 + v1
    two = gravity_from_views(dict(yaw=[0.0, 0.0]), [0.0, 0.0], [10.0, 50.0], weights=[3.0, 1.0], max_dev=180.0)
    v = two["votes"].numpy()
    d = 3 * v[0] + v[1]
    assert np.abs(two["direction"].numpy() - d / np.linalg.norm(d)).max() <= 1e-14


def test_gravity_from_views_non_finite_predictions_do_not_vote():
    from perspectivefields_amd import gravity_from_views

    cams, roll, pitch = view_truth(TILT)
    roll_nan = roll.copy()
    roll_nan[5] = np.nan
    pitch_inf = pitch.copy()
    pitch_inf[9] = np.inf
    res = gravity_from_views(cams, roll_nan, pitch_inf)
    assert not res["inliers"][5] and not res["inliers"][9] and int(res["inliers"].sum()) == 14
    assert abs(float(res["roll"]) - TILT[0]) <= 1e-9 and abs(float(res["pitch"]) - TILT[1]) <= 1e-9
    none = gravity_from_views(cams, np.full(16, np.nan), pitch)
    assert np.isnan(float(none["roll"])) and np.isnan(float(none["pitch"])) and not none["inliers"].any()
    with pytest.raises(ValueError):
        gravity_from_views(dict(cams, focal=1.0), roll, pitch)
    with pytest.raises(ValueError):
        gravity_from_views(cams, roll[:5], pitch)
    with pytest.raises(ValueError):
        gravity_from_views(cams, roll, pitch, mode="grad")
    with pytest.raises(TypeError):
        gravity_from_views([0.0], roll, pitch)


# ---------------------------------------------------------------- host-side contract (fails before the feature exists)
def test_names_are_exported():
    import perspectivefields_amd

    for name in ("rotate_panorama", "panorama_fields", "gravity_from_views"):
        assert name in perspectivefields_amd.__all__ and callable(getattr(perspectivefields_amd, name))
    assert callable(perspectivefields_amd.PerspectiveFields.level_panorama)


def test_header_states_the_model_and_the_bound():
    hdr = open(os.path.join(ROOT, "include", "pf_hip.h")).read()
    assert "int pf_pano_rotate(int device, int n_pano, const void* const* h_pano, const int32_t* h_pano_hw" in hdr
    assert "int pf_pano_fields(int device, int batch, const float* d_rot3" in hdr
    assert "#define PF_PANO_UP_MIN_T2 1e-10f" in hdr
    kh = open(os.path.join(ROOT, "perspectivefields_amd", "csrc", "pf_kernels.h")).read()
    assert "struct PanoRotBatch" in kh and "offsetof(PanoRotBatch, src) == 32" in kh


def test_symbols_and_prototypes_are_present():
    from perspectivefields_amd.engine import _SIGNATURES, declared_symbols, load_library

    assert "pf_pano_rotate" in declared_symbols() and "pf_pano_fields" in declared_symbols()
    res, args = _SIGNATURES["pf_pano_rotate"]
    assert res is ctypes.c_int and len(args) == 15 and args[8] is ctypes.c_int
    res, args = _SIGNATURES["pf_pano_fields"]
    assert res is ctypes.c_int and len(args) == 9
    lib = load_library()
    assert hasattr(lib, "pf_pano_rotate") and hasattr(lib, "pf_pano_fields")


def test_pf_pano_rotate_rejects_bad_arguments_before_device_work():
    from perspectivefields_amd.engine import load_library

    lib = load_library()
    pano = (ctypes.c_void_p * 1)(0x1000)
    ints = lambda *s: (ctypes.c_int32 * len(s))(*s)
    dev = ctypes.c_void_p(256)

    def call(hw=None, dtype=0, idx=(0,), c_idx=True, H=4, W=8, img=dev, rot=dev, up=None, lat=None, n=1, p=pano, B=None):
        rc = lib.pf_pano_rotate(0, n, p, hw or ints(8, 16), dtype, len(idx) if B is None else B, ints(*idx) if c_idx else None, rot, 0, H, W, img, up, lat, None)
        return rc, lib.pf_last_error(None).decode()

    for kw, what in ((dict(idx=(1,)), "index"), (dict(idx=(-1,)), "index"), (dict(dtype=2), "dtype"), (dict(hw=ints(1, 16)), "smaller"), (dict(hw=ints(8, 1)), "smaller"),
                     (dict(H=0), "size"), (dict(W=0), "size"), (dict(img=None), "required"), (dict(rot=None), "required"), (dict(c_idx=False), "required"),
                     (dict(B=0), "required"), (dict(up=dev), "both"), (dict(lat=dev), "both"), (dict(p=(ctypes.c_void_p * 1)()), "NULL"), (dict(p=None), "at least one"),
                     (dict(n=0), "at least one")):
        rc, msg = call(**kw)
        assert rc == -1 and what in msg and msg.startswith("pf_pano_rotate: "), (kw, rc, msg)
    if not torch.cuda.is_available():   # good arguments fail on the missing device only
        rc, msg = call(up=dev, lat=dev)
        assert rc == -2 and "no HIP device" in msg, (rc, msg)


def test_pf_pano_fields_rejects_bad_arguments_before_device_work():
    from perspectivefields_amd.engine import load_library

    lib = load_library()
    dev = ctypes.c_void_p(256)

    def call(B=1, rot=dev, H=4, W=8, up=dev, lat=dev):
        return lib.pf_pano_fields(0, B, rot, 0, H, W, up, lat, None), lib.pf_last_error(None).decode()

    for kw, what in ((dict(B=0), "required"), (dict(rot=None), "required"), (dict(up=None), "required"), (dict(lat=None), "required"), (dict(H=0), "size"), (dict(W=-1), "size")):
        rc, msg = call(**kw)
        assert rc == -1 and what in msg and msg.startswith("pf_pano_fields: "), (kw, rc, msg)
    if not torch.cuda.is_available():
        rc, msg = call()
        assert rc == -2 and "no HIP device" in msg, (rc, msg)


def test_rotate_panorama_on_cpu_tensors_raises():
    from perspectivefields_amd import rotate_panorama
    from perspectivefields_amd.engine import PfError

    for pano in (torch.zeros((8, 16, 3), dtype=torch.uint8), [torch.zeros((8, 16, 3))]):
        with pytest.raises(PfError):
            rotate_panorama(pano, 10.0, 20.0)


def test_python_argument_errors_before_the_library_is_loaded(monkeypatch):
    from perspectivefields_amd import engine
    from perspectivefields_amd import perspectivefields as pfm

    def no_library(*a, **k):
        raise AssertionError("the library was loaded before the arguments were checked")

    monkeypatch.setattr(engine, "load_library", no_library)
    monkeypatch.setattr(pfm.torch, "is_tensor", lambda v: isinstance(v, (torch.Tensor, FakeCuda)))
    ok, other = FakeCuda((8, 16, 3)), FakeCuda((10, 20, 3))
    bad = [
        dict(pano=FakeCuda((8, 16, 4))), dict(pano=FakeCuda((8, 16))), dict(pano=FakeCuda((1, 16, 3))), dict(pano=FakeCuda((8, 16, 3), torch.float16)),
        dict(pano=[ok, FakeCuda((8, 16, 3), torch.float32)]), dict(pano=[]), dict(height=0, width=8), dict(height=8, width=0), dict(height=8), dict(width=16),
        dict(mode="grad"), dict(pano_index=[1]), dict(pano_index=[-1]), dict(pano_index=[0, 0]), dict(roll=[1.0, 2.0], pitch=[1.0, 2.0, 3.0]),
        dict(yaw=np.zeros((2, 2))), dict(pano=[ok, other], pano_index=[0]),   # sources of two sizes need height and width
    ]
    for kw in bad:
        args = dict(pano=ok, roll=0.0, pitch=0.0, yaw=0.0)
        args.update(kw)
        with pytest.raises(ValueError):
            pfm.rotate_panorama(args.pop("pano"), **args)
    with pytest.raises(TypeError):
        pfm.rotate_panorama([ok, np.zeros((8, 16, 3))])
    for kw in (dict(height=0), dict(width=0), dict(mode="grad"), dict(roll=[1.0, 2.0], pitch=[1.0, 2.0, 3.0]), dict(roll=np.zeros((2, 2)))):
        args = dict(roll=0.0, pitch=0.0, height=4, width=8)
        args.update(kw)
        with pytest.raises(ValueError):
            pfm.panorama_fields(args.pop("roll"), args.pop("pitch"), **args)
    with pytest.raises(TypeError):
        pfm.panorama_fields(0.0, 0.0)   # height and width are required
    with pytest.raises(engine.PfError):
        pfm.panorama_fields(0.0, 0.0, height=4, width=8, device="cpu")


def test_level_panorama_argument_errors_without_a_gpu(monkeypatch):
    from perspectivefields_amd import PerspectiveFields
    from perspectivefields_amd import perspectivefields as pfm
    from perspectivefields_amd.engine import PfError

    monkeypatch.setattr(pfm.torch, "is_tensor", lambda v: isinstance(v, (torch.Tensor, FakeCuda)))
    ok = FakeCuda((8, 16, 3))
    level = PerspectiveFields.level_panorama
    for kw in (dict(use="network"), dict(n_yaw=0), dict(view_pitch=()), dict(vfov=180.0), dict(vfov=0.0), dict(view_size=4), dict(preds=[dict(pred_roll=0.0)])):
        with pytest.raises(ValueError):
            level(None, ok, **kw)
    with pytest.raises(ValueError):
        level(None, FakeCuda((8, 16, 4)))
    with pytest.raises(TypeError):
        level(None, [ok])
    with pytest.raises(PfError):
        level(None, torch.zeros((8, 16, 3), dtype=torch.uint8))
    fields_only = [dict(pred_gravity_original=None, pred_latitude_original=None)] * 8
    with pytest.raises(PfError, match="fit_camera"):   # a PersNet result has no scalars: the text of rectify
        level(None, ok, preds=fields_only)


def test_rotate_kernels_are_in_the_library_without_scratch():
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
    names = [f"pf::pano_rotate_kernel<{t}, {labels}>" for t in ("unsigned char", "float") for labels in ("false", "true")] + ["pf::pano_fields_kernel"]
    for name in names:
        r = by[name]
        assert r["spill"] == 0 and r["scratch"] == 0 and r["lds"] <= 64 and r["vgpr"] <= 128, r
