"""fp64 numpy statement of the transport of perspective fields between cameras of one centre and onto equirectangular panoramas (include/pf_hip.h
pf_reproject_fields / pf_compose_fields), built on the camera model of tests/test_pano_crop_ref.py and tests/test_reproject_ref.py.
The differential of (unproject, rotate, project) is the closed form of csrc/field_transport.h -- push and lift, no finite differences, no dual
numbers.  The two models are written once, generic in the number format: `f=np.float64` is the reference, `f=np.float32` the restatement in the
kernels' order of operations, whose error against the reference is the rounding floor the GPU results are held to (tests/test_gpu_field_transport.py).
Checks of the reference against itself, against an independent field synthesis (tests/test_pano_crop_ref.labels, itself checked against the oracle
here) and against the tilted panorama's own fields (tests/test_pano_rotate_ref.fields); plus the host-side contract (no GPU needed)."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

from oracle import pf_oracle
from tests.test_fit_camera_ref import general_vfov_deg
from tests.test_pano_crop_ref import labels, rotation
from tests.test_pano_rotate_ref import decompose, fields as pano_fields, up_angle_deg
from tests.test_reproject_ref import CASES, SIZES, FakeCuda, theta_rad, yaw_matrix

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIN_LEN2 = 1e-12   # pf_place_scores' length rule
FP64_NOISE = 1e-9  # degrees: where a field is constant (a camera without pitch) the interpolation error is 0 and only fp64 rounding is left
LAT_LIMIT = 75.0   # the closed loops are judged away from the world's zenith and nadir, where the up field is singular


# ---------------------------------------------------------------- the model, generic in the number format f
def _rot(roll, pitch, f):
    sr, cr, sp, cp = np.sin(roll), np.cos(roll), np.sin(pitch), np.cos(pitch)
    return np.array([[cr, -sr, f(0)], [cp * sr, cp * cr, -sp], [sp * sr, sp * cr, cp]], dtype=f)


def _yaw(t, f):
    return np.array([[np.cos(t), f(0), np.sin(t)], [f(0), f(1), f(0)], [-np.sin(t), f(0), np.cos(t)]], dtype=f)


def _z_min(xi, f):
    return f(-1) / xi if xi > 1 else f(0) - xi


def _ray(x, y, xi, f):
    """usm_ray: (X, has_ray, disc)"""
    r2 = x * x + y * y
    disc = f(1) + (f(1) - xi * xi) * r2
    ok = disc >= 0
    with np.errstate(invalid="ignore"):
        eta = (xi + np.sqrt(np.where(ok, disc, f(np.nan)))) / (f(1) + r2)
    return np.stack([eta * x, eta * y, eta - xi], -1), ok, disc


def _point(X, xi, F, Cx, Cy):
    with np.errstate(invalid="ignore", divide="ignore"):
        D = X[..., 2] + xi * np.sqrt((X * X).sum(-1))
        return F * (X[..., 0] / D) + Cx, F * (X[..., 1] / D) + Cy


def push(X, t, xi):
    """usm_push: the image direction (..., 2) of the tangents t at the rays X (any length)"""
    n = np.sqrt((X * X).sum(-1))
    D = X[..., 2] + xi * n
    s = t[..., 2] + xi * (X * t).sum(-1) / n
    return np.stack([t[..., 0] * D - X[..., 0] * s, t[..., 1] * D - X[..., 1] * s], -1)


def lift(X, mx, my, xi):
    """usm_lift: the unit tangents t, t . X = 0, whose push is a positive multiple of (mx, my)"""
    f = X.dtype.type
    with np.errstate(invalid="ignore", divide="ignore"):
        n = np.sqrt((X * X).sum(-1))
        x0, x1, x2 = X[..., 0] / n, X[..., 1] / n, X[..., 2] / n
        first = np.abs(X[..., 0]) < f(0.9) * n
        ka, kb = f(1) / np.sqrt(x2 * x2 + x1 * x1), f(1) / np.sqrt(x2 * x2 + x0 * x0)
        zero = np.zeros_like(x0)
        e1 = np.where(first[..., None], np.stack([zero, x2 * ka, -x1 * ka], -1), np.stack([-x2 * kb, zero, x0 * kb], -1))
        e2 = np.stack([x1 * e1[..., 2] - x2 * e1[..., 1], x2 * e1[..., 0] - x0 * e1[..., 2], x0 * e1[..., 1] - x1 * e1[..., 0]], -1)
        p1, p2 = push(X, e1, xi), push(X, e2, xi)
        sg = np.copysign(f(1), p1[..., 0] * p2[..., 1] - p1[..., 1] * p2[..., 0])
        al, be = (mx * p2[..., 1] - my * p2[..., 0]) * sg, (p1[..., 0] * my - p1[..., 1] * mx) * sg
        k = f(1) / np.sqrt(al * al + be * be)
        return (al[..., None] * e1 + be[..., None] * e2) * k[..., None]


def taps(up, lat, u, v, ok):
    """the four taps of the samples at (u, v), index units, where `ok`: (W, mx, my, ml), sums over the taps that count, in tap order"""
    f = lat.dtype.type
    Hs, Ws = lat.shape
    with np.errstate(invalid="ignore"):
        l2 = up[0] * up[0] + up[1] * up[1]
        good = np.isfinite(lat) & (l2 >= f(MIN_LEN2)) & (l2 < np.inf)
    u, v = np.where(ok, u, f(0)), np.where(ok, v, f(0))
    uf, vf = np.floor(u), np.floor(v)
    au, av = u - uf, v - vf
    c, r = uf.astype(np.int64), vf.astype(np.int64)
    W, mx, my, ml = (np.zeros(u.shape, dtype=f) for _ in range(4))
    for ty in (0, 1):
        for tx in (0, 1):
            ci, ri = c + tx, r + ty
            inside = (ci >= 0) & (ci < Ws) & (ri >= 0) & (ri < Hs)
            cq, rq = np.clip(ci, 0, Ws - 1), np.clip(ri, 0, Hs - 1)
            cnt = ok & inside & good[rq, cq]
            wk = (av if ty else f(1) - av) * (au if tx else f(1) - au)
            W = W + np.where(cnt, wk, f(0))
            mx = mx + np.where(cnt, wk * up[0][rq, cq], f(0))
            my = my + np.where(cnt, wk * up[1][rq, cq], f(0))
            ml = ml + np.where(cnt, wk * lat[rq, cq], f(0))
    return W, mx, my, ml


def _near_half(W):
    return np.abs(W - 0.5) < 1e-3


def _near_len(m2):
    return (m2 > MIN_LEN2 / 4) & (m2 < MIN_LEN2 * 4)


def _may_land_inside(a, b, Hs, Ws):
    """the visibility limit z_min is a discontinuity of the RESULT only where the ray's point, were it visible, could be inside the source: for
    xi <= 1 the points of rays next to z_min lie far outside every image, and whether such a ray counts as visible changes nothing"""
    with np.errstate(invalid="ignore"):
        return ~(np.isfinite(a) & np.isfinite(b)) | ((a >= -1) & (a <= Ws + 1) & (b >= -1) & (b <= Hs + 1))


def reproject_fields_model(up, lat, src, dst, H, W, f=np.float64):
    """views -> views: theta = (roll, pitch, yaw [rad], rel_focal, rel_cx, rel_cy, xi) of both cameras, source planes up (2, Hs, Ws), lat (Hs, Ws)
    -> up' (2, H, W), lat' (H, W) in the format f (NaN x 3 where invalid) and `near`, the pixels the `clear` rule leaves out"""
    Hs, Ws = lat.shape
    if not (np.isfinite(np.asarray(src, dtype=np.float64)).all() and np.isfinite(np.asarray(dst, dtype=np.float64)).all()):
        return np.full((2, H, W), np.nan, dtype=f), np.full((H, W), np.nan, dtype=f), np.zeros((H, W), dtype=bool)
    s, d = [f(v) for v in src], [f(v) for v in dst]
    up, lat = np.asarray(up, dtype=f), np.asarray(lat, dtype=f)
    M = _rot(s[0], s[1], f).T @ (_yaw(d[2] - s[2], f) @ _rot(d[0], d[1], f))
    inv_fd, Cxd, Cyd = f(1) / (d[3] * f(H)), (d[4] + f(0.5)) * f(W), (d[5] + f(0.5)) * f(H)
    Fs, Cxs, Cys, zmin = s[3] * f(Hs), (s[4] + f(0.5)) * f(Ws), (s[5] + f(0.5)) * f(Hs), _z_min(s[6], f)
    cols = np.arange(W, dtype=f)[None, :] + np.zeros((H, 1), f)
    rows = np.arange(H, dtype=f)[:, None] + np.zeros((1, W), f)

    def point(pa, pb):  # steps 1 to 5 of pf_reproject
        Xd, ok, disc = _ray((pa - Cxd) * inv_fd, (pb - Cyd) * inv_fd, d[6], f)
        Xs = Xd @ M.T
        with np.errstate(invalid="ignore"):
            vis = ok & (Xs[..., 2] > zmin)
            a, b = _point(Xs, s[6], Fs, Cxs, Cys)
            inside = vis & (a >= 0) & (a <= f(Ws)) & (b >= 0) & (b <= f(Hs))
            near = (np.abs(disc) <= 1e-4) | (ok & (np.abs(Xs[..., 2] - zmin) <= 1e-3) & _may_land_inside(a, b, Hs, Ws))
            for c, n in ((a, Ws), (b, Hs)):
                near |= vis & ((np.abs(c) <= 1e-2) | (np.abs(c - n) <= 1e-2))
        return Xd, Xs, a, b, inside, near

    Xd, Xs, a, b, in_u, near = point(cols + f(0.5), rows + f(0.5))
    Wu, mx, my, _ = taps(up, lat, a - f(0.5), b - f(0.5), in_u)
    m2 = mx * mx + my * my
    _, _, a2, b2, in_l, near_l = point(cols * (f(W) / f(W - 1)), rows * (f(H) / f(H - 1)))
    Wl, _, _, ml = taps(up, lat, a2 * (f(Ws - 1) / f(Ws)), b2 * (f(Hs - 1) / f(Hs)), in_l)
    valid = in_u & (Wu >= f(0.5)) & (m2 >= f(MIN_LEN2)) & in_l & (Wl >= f(0.5))
    near = near | near_l | (in_u & (_near_half(Wu) | _near_len(m2))) | (in_l & _near_half(Wl))
    with np.errstate(invalid="ignore", divide="ignore"):
        t = lift(Xs, mx, my, s[6])
        p = push(Xd, t @ M, d[6])   # M^T t
        inv = f(1) / np.sqrt((p * p).sum(-1))
        out_up = np.where(valid, np.stack([p[..., 0] * inv, p[..., 1] * inv]), f(np.nan))
        out_lat = np.where(valid, ml / Wl, f(np.nan))
    assert out_up.dtype == f and out_lat.dtype == f
    return out_up, out_lat, near


def compose_fields_model(ups, lats, thetas, Hp, Wp, blend="feather", f=np.float64):
    """views -> one equirectangular panorama: up (2, Hp, Wp), lat (Hp, Wp), S (Hp, Wp) in the format f, and `near`"""
    lon = ((np.arange(Wp, dtype=f) + f(0.5)) / f(Wp) - f(0.5)) * f(2 * np.pi)
    la = (f(0.5) - (np.arange(Hp, dtype=f) + f(0.5)) / f(Hp)) * f(np.pi)
    la, lon = np.meshgrid(la, lon, indexing="ij")
    sl, cl, so, co = np.sin(la), np.cos(la), np.sin(lon), np.cos(lon)
    D = np.stack([cl * so, f(0) - sl, cl * co], -1)
    kx, ky = f(Wp) * f(1 / (2 * np.pi)) / cl, f(Hp) * f(1 / np.pi)
    S, L, Ux, Uy = (np.zeros((Hp, Wp), dtype=f) for _ in range(4))
    near = np.zeros((Hp, Wp), dtype=bool)
    for up, lat, th in zip(ups, lats, thetas):
        if not np.isfinite(np.asarray(th, dtype=np.float64)).all():
            continue   # a view with non-finite parameters contributes nothing
        Hs, Ws = lat.shape
        up, lat = np.asarray(up, dtype=f), np.asarray(lat, dtype=f)
        r, p, yaw, rf, cx, cy, xi = [f(v) for v in th]
        M = _rot(r, p, f).T @ _yaw(f(0) - yaw, f)
        zmin = _z_min(xi, f)
        X = D @ M.T
        with np.errstate(invalid="ignore", divide="ignore"):
            vis = X[..., 2] > zmin
            a, b = _point(X, xi, rf * f(Hs), (cx + f(0.5)) * f(Ws), (cy + f(0.5)) * f(Hs))
            ra, rb = f(Ws) - a, f(Hs) - b
            covers = vis & (a > 0) & (ra > 0) & (b > 0) & (rb > 0)
            dmin = np.minimum(np.minimum(a, ra), np.minimum(b, rb))
            w = np.minimum(dmin * (f(2) / f(min(Hs, Ws))), f(1)) if blend == "feather" else np.ones_like(a)
            Wu, mx, my, _ = taps(up, lat, a - f(0.5), b - f(0.5), covers)
            m2 = mx * mx + my * my
            Wl, _, _, ml = taps(up, lat, a * (f(Ws - 1) / f(Ws)), b * (f(Hs - 1) / f(Hs)), covers)
            tw = lift(X, mx, my, xi) @ M   # M^T t: the view's camera -> world
            ta = tw[..., 0] * co - tw[..., 2] * so
            tb = -(tw[..., 1] * cl + sl * (tw[..., 0] * so + tw[..., 2] * co))
            px, py = kx * ta, -(ky * tb)
            p2 = px * px + py * py
            counts = covers & (Wu >= f(0.5)) & (m2 >= f(MIN_LEN2)) & (Wl >= f(0.5)) & (p2 >= f(MIN_LEN2)) & (p2 < np.inf)
            inv = f(1) / np.sqrt(p2)
            S = S + np.where(counts, w, f(0))
            L = L + np.where(counts, w * (ml / Wl), f(0))
            Ux = Ux + np.where(counts, w * (px * inv), f(0))
            Uy = Uy + np.where(counts, w * (py * inv), f(0))
            near |= (vis & (np.abs(dmin) <= 1e-2)) | ((np.abs(X[..., 2] - zmin) <= 1e-3) & _may_land_inside(a, b, Hs, Ws))
            near |= covers & (_near_half(Wu) | _near_half(Wl) | _near_len(m2))
    with np.errstate(invalid="ignore", divide="ignore"):
        u2 = Ux * Ux + Uy * Uy
        has = (S > 0) & (u2 >= f(MIN_LEN2))
        inv = f(1) / np.sqrt(u2)
        out_up = np.where(has, np.stack([Ux * inv, Uy * inv]), f(np.nan))
        out_lat = np.where(has, L / S, f(np.nan))
    near |= (S > 0) & (S < 1e-3)
    assert out_up.dtype == f and out_lat.dtype == f and S.dtype == f
    return out_up, out_lat, S, near


# ---------------------------------------------------------------- errors, and the comparison every check of a result uses
def field_errors_deg(up, lat, up_ref, lat_ref, keep):
    """largest up angle and latitude error in degrees over the pixels of `keep` that are valid in both, and whether validity agrees on all of `keep`"""
    v, vr = np.isfinite(lat), np.isfinite(lat_ref)
    same = np.array_equal(v[keep], vr[keep]) and np.array_equal(np.isfinite(up).all(0)[keep], vr[keep])
    m = keep & v & vr
    if not m.any():
        return 0.0, 0.0, same
    return float(up_angle_deg(up, up_ref)[m].max()), float(np.abs(lat.astype(np.float64) - lat_ref)[m].max()), same


# ---------------------------------------------------------------- the fixed inputs: view pairs and compositions
def pair_inputs(k, size, scale=1, dtype=np.float32):
    """case k of tests/test_reproject_ref.CASES at `size` = (Hs, Ws, H, W), the source `scale` times as large: the exact fields of the source camera
    (float32, as a network's output is and as the device reads them; fp64 for the closed loops, which are statements about the model), both cameras in
    radians, the output size"""
    Hs, Ws, H, W = size
    s, d = theta_rad(*CASES[k][0]), theta_rad(*CASES[k][1])
    up, lat = labels(s, Hs * scale, Ws * scale)
    return up.astype(dtype), lat.astype(dtype), s, d, H, W


TILT = (14.0, -22.0, 20.0)   # roll, pitch, yaw (degrees) of the tilted panorama's camera
F100 = 0.5 / np.tan(np.radians(50.0))
# name -> (views [((roll, pitch, yaw [deg], rel_focal, rel_cx, rel_cy, xi) in the panorama's own frame, (Hs, Ws))], (Hp, Wp))
COMPOSITIONS = {
    "tilted18": ([((0.0, p, y, F100, 0.0, 0.0, 0.0), (40, 40)) for p in (-45.0, 0.0, 45.0) for y in range(0, 360, 60)], (32, 64)),
    "ragged5": ([((5.0, 10.0, 0.0, 0.45, 0.0, 0.0, 0.0), (37, 53)), ((-8.0, -20.0, 80.0, 0.45, 0.03, -0.02, 0.6), (40, 40)),
                 ((0.0, 30.0, 160.0, 0.4, 0.0, 0.0, 0.0), (37, 53)), ((12.0, -35.0, 230.0, 0.5, 0.0, 0.0, 0.6), (40, 40)),
                 ((0.0, 60.0, 300.0, 0.42, 0.0, 0.0, 0.0), (40, 40))], (31, 61)),   # Wp % 4 != 0: the scalar stores
}
TWO_PANOS = ("ragged5", (0, 0, 0, 0, 0), 2)   # two panoramas in one call, the second one without a view


def view_fields(cam_deg, size, tilt=TILT, scale=1):
    """the exact fields (fp64) of a view with camera `cam_deg` in the frame of a panorama whose own camera is tilted by `tilt`: the view's camera ->
    world rotation is Q(tilt) Y(yaw) R(roll, pitch), and its fields are those of that rotation's (roll, pitch)"""
    Q = yaw_matrix(np.radians(tilt[2])) @ rotation(np.radians(tilt[0]), np.radians(tilt[1]))
    r, p, _ = decompose(Q @ yaw_matrix(np.radians(cam_deg[2])) @ rotation(np.radians(cam_deg[0]), np.radians(cam_deg[1])))
    return labels((r, p, 0.0) + tuple(cam_deg[3:]), size[0] * scale, size[1] * scale)


@functools.lru_cache(None)
def composition_inputs(name, scale=1, dtype=np.float32):
    views, (Hp, Wp) = COMPOSITIONS[name]
    pairs = [view_fields(c, hw, scale=scale) for c, hw in views]
    ups, lats = [u.astype(dtype) for u, _ in pairs], [l.astype(dtype) for _, l in pairs]
    for a in ups + lats:
        a.setflags(write=False)
    return ups, lats, [theta_rad(*c) for c, _ in views], Hp, Wp


def tilted_panorama_fields(Hp, Wp, tilt=TILT):
    up, lat, _ = pano_fields(tuple(np.radians(tilt)), False, Hp, Wp)
    return up, lat


@functools.lru_cache(None)
def pair_reference(k, size):
    up, lat, s, d, H, W = pair_inputs(k, size)
    return reproject_fields_model(up, lat, s, d, H, W)


@functools.lru_cache(None)
def fp32_floor(size):
    """largest error of the float32 restatement against the fp64 reference over the cases at one size: (up angle, latitude) in degrees, on clear pixels;
    the restatement's validity equals the reference's there"""
    worst = np.zeros(2)
    for k in range(len(CASES)):
        up, lat, s, d, H, W = pair_inputs(k, size)
        ur, lr, near = pair_reference(k, size)
        u32, l32, _ = reproject_fields_model(up, lat, s, d, H, W, f=np.float32)
        e_up, e_lat, same = field_errors_deg(u32, l32, ur, lr, ~near)
        assert same, k
        worst = np.maximum(worst, (e_up, e_lat))
    return tuple(worst)


@functools.lru_cache(None)
def composition_reference(name, blend="feather"):
    ups, lats, thetas, Hp, Wp = composition_inputs(name)
    return compose_fields_model(ups, lats, thetas, Hp, Wp, blend)


@functools.lru_cache(None)
def composition_floor(name, blend="feather"):
    """(up angle, latitude in degrees, summed weight) errors of the float32 restatement of a composition on clear pixels"""
    ups, lats, thetas, Hp, Wp = composition_inputs(name)
    ur, lr, Sr, near = composition_reference(name, blend)
    u32, l32, S32, _ = compose_fields_model(ups, lats, thetas, Hp, Wp, blend, f=np.float32)
    e_up, e_lat, same = field_errors_deg(u32, l32, ur, lr, ~near)
    assert same, name
    return e_up, e_lat, float(np.abs(S32 - Sr)[~near].max())


# ---------------------------------------------------------------- the reference against itself
@pytest.mark.parametrize("case", [(10.0, 25.0, 0.8, 0.0, 0.0, 48, 64), (-35.0, 0.0, 1.2, 0.05, -0.04, 31, 47), (0.0, -70.0, 0.35, 0.0, 0.0, 29, 61)])
def test_field_synthesis_matches_the_oracle(case):
    """the independent synthesis the closed loops are judged by equals the oracle's fields_from_params to 1e-9 (as tests/test_fit_camera_ref.py checks
    its own model), pitch 0 and the linspace latitude grid included"""
    roll, pitch, fr, cx, cy, H, W = case
    up_o, lat_o, f_o = pf_oracle.fields_from_params(roll, pitch, general_vfov_deg(fr, cx, cy), cx, cy, H, W, mode="deg")
    assert abs(f_o - fr) <= 1e-12 * fr
    up, lat = labels((np.radians(roll), np.radians(pitch), 0.0, fr, cx, cy, 0.0), H, W)
    assert np.abs(up - np.moveaxis(up_o, 2, 0)).max() <= 1e-9 and np.abs(lat - lat_o).max() <= 1e-9


@pytest.mark.parametrize("xi", [0.0, 0.5, 1.3])
def test_push_and_lift_are_inverse(xi):
    rng = np.random.default_rng(int(10 * xi) + 3)
    X = rng.normal(size=(4000, 3))
    X /= np.linalg.norm(X, axis=-1, keepdims=True)
    X = X[X[:, 2] > (-1.0 / xi if xi > 1 else -xi) + 1e-2] * rng.uniform(0.5, 2.0, (1, 1))   # rays the camera sees, of any length
    t = np.cross(X, rng.normal(size=X.shape))
    t /= np.linalg.norm(t, axis=-1, keepdims=True)
    m = push(X, t, xi)
    back = lift(X, m[:, 0], m[:, 1], xi)
    assert len(X) > 500 and np.abs(back - t).max() <= 1e-12 and np.abs((back * X).sum(-1)).max() <= 1e-12
    # and the push is the derivative of the projection: a central difference of the projected point along t, as a direction
    h = 1e-6
    proj = lambda Y: Y[:, :2] / (Y[:, 2] + xi * np.linalg.norm(Y, axis=-1))[:, None]
    fd = proj(X + h * t) - proj(X - h * t)
    cosang = (fd * m).sum(-1) / (np.linalg.norm(fd, axis=-1) * np.linalg.norm(m, axis=-1))
    assert cosang.min() >= 1.0 - 1e-8


@pytest.mark.parametrize("xi", [0.0, 0.5, 1.3])
def test_same_camera_and_size_is_the_identity(xi):
    th = theta_rad(12.0, -20.0, 33.0, 0.45, 0.04, -0.03, xi)
    H, W = 37, 53
    up, lat = labels(th, H, W)
    u2, l2, _ = reproject_fields_model(up, lat, th, th, H, W)
    both = np.isfinite(l2) & np.isfinite(lat)
    inner = np.zeros((H, W), dtype=bool)
    inner[1:-1, 1:-1] = True   # the first and last linspace points sit on the source's border itself
    src_ok = np.isfinite(lat) & np.isfinite(up).all(0)
    grown = np.ones((H, W), dtype=bool)   # pixels whose 3 x 3 neighbourhood is valid in the source
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            grown &= np.roll(src_ok, (dy, dx), (0, 1))
    assert both[inner & grown].all() and (inner & grown).mean() > 0.5
    assert np.abs(u2 - up)[:, both].max() <= 1e-12 and np.abs(l2 - lat)[both].max() <= 1e-12
    assert not np.isfinite(l2[~src_ok]).any()   # the source's mask stays a mask


@pytest.mark.parametrize("size", SIZES)
def test_closed_loop_views_to_views(size):
    """exact fields of the source camera come out as the exact fields of the destination camera up to the bilinear interpolation error, which is of
    second order: at twice the source size it is at most half (a quarter in the limit).  Judged on |destination latitude| <= 75 degrees"""
    worst = np.zeros(2)
    shares = []
    for k in range(len(CASES)):
        up, lat, s, d, H, W = pair_inputs(k, size, dtype=np.float64)
        tu, tl = labels(d, H, W)
        keep = np.abs(tl) <= LAT_LIMIT
        u1, l1, near = reproject_fields_model(up, lat, s, d, H, W)
        u2, l2, near2 = reproject_fields_model(*pair_inputs(k, size, scale=2, dtype=np.float64)[:4], H, W)
        keep = keep & ~near & ~near2 & np.isfinite(l1) & np.isfinite(l2)
        assert keep.sum() >= 50, k
        e1 = field_errors_deg(u1, l1, tu, tl, keep)
        e2 = field_errors_deg(u2, l2, tu, tl, keep)
        assert e2[0] <= 0.5 * e1[0] + FP64_NOISE and e2[1] <= 0.5 * e1[1] + FP64_NOISE, (k, e1, e2)
        worst = np.maximum(worst, e1[:2])
        shares.append(np.isfinite(l1).mean())
    print(f"closed loop at {size}: up {worst[0]:.3f} deg, latitude {worst[1]:.3f} deg; valid share {min(shares):.2f} .. {max(shares):.2f}")


def test_closed_loop_views_to_panorama():
    """the 18 views of the tilted panorama, composed, against the tilted panorama's own fields: every pixel covered, second order in the view size"""
    name = "tilted18"
    ups, lats, thetas, Hp, Wp = composition_inputs(name, dtype=np.float64)
    tu, tl = tilted_panorama_fields(Hp, Wp)
    u1, l1, S1, near = compose_fields_model(ups, lats, thetas, Hp, Wp)
    u2, l2, S2, near2 = compose_fields_model(*composition_inputs(name, 2, np.float64)[:3], Hp, Wp)
    assert np.isfinite(l1).all() and np.isfinite(u1).all() and (S1 > 0).all()
    keep = (np.abs(tl) <= LAT_LIMIT) & ~near & ~near2
    e1 = field_errors_deg(u1, l1, tu, tl, keep)
    e2 = field_errors_deg(u2, l2, tu, tl, keep)
    print(f"composition closed loop: up {e1[0]:.3f} deg, latitude {e1[1]:.3f} deg; at twice the view size {e2[0]:.3f}, {e2[1]:.3f}")
    assert e2[0] <= 0.5 * e1[0] + FP64_NOISE and e2[1] <= 0.5 * e1[1] + FP64_NOISE, (e1, e2)


@pytest.mark.parametrize("size", SIZES)
def test_excluded_share_is_small_and_no_case_is_empty(size):
    for k in range(len(CASES)):
        _, l, near = pair_reference(k, size)
        assert near.mean() <= 0.01, (k, near.mean())
        assert np.isfinite(l).mean() >= 0.10, k


@pytest.mark.parametrize("name", sorted(COMPOSITIONS))
def test_compositions_leave_little_out(name):
    _, l, S, near = composition_reference(name)
    assert near.mean() <= 0.01, near.mean()
    assert np.isfinite(l).mean() >= 0.5


@pytest.mark.parametrize("size", SIZES)
def test_fp32_floor_of_the_transport(size):
    e_up, e_lat = fp32_floor(size)
    print(f"fp32 floor at {size}: up {e_up:.3e} deg, latitude {e_lat:.3e} deg")
    # fp32 epsilon (6e-8) times a latitude of up to 90 degrees, and times a radian in degrees for a direction, each with the conditioning of a few taps
    # and a 2 x 2 solve: a floor beyond 1e-2 degrees would make the GPU check (4 x floor) empty against the closed-loop errors of ~0.1 degrees
    assert 0 < e_up <= 1e-2 and 0 < e_lat <= 1e-3


@pytest.mark.parametrize("name", sorted(COMPOSITIONS))
@pytest.mark.parametrize("blend", ["feather", "mean"])
def test_fp32_floor_of_the_compositions(name, blend):
    e_up, e_lat, e_S = composition_floor(name, blend)
    print(f"fp32 floor of {name} ({blend}): up {e_up:.3e} deg, latitude {e_lat:.3e} deg, weight {e_S:.3e}")
    assert 0 < e_up <= 1e-2 and 0 < e_lat <= 1e-3 and e_S <= 1e-4


def test_a_nan_block_stays_a_mask_and_does_not_spread():
    up, lat, s, d, H, W = pair_inputs(0, SIZES[0])
    Hs, Ws = lat.shape
    r0, r1, c0, c1 = 30, 50, 40, 70
    up_b, lat_b = up.copy(), lat.copy()
    up_b[:, r0:r1, c0:c1] = np.nan
    lat_b[r0:r1, c0:c1] = np.nan
    u0, l0, _ = reproject_fields_model(up, lat, s, d, H, W)
    u1, l1, _ = reproject_fields_model(up_b, lat_b, s, d, H, W)
    from tests.test_reproject_ref import source_coords

    a, b, inside = source_coords(s, Hs, Ws, d, H, W)   # of the pixel centres, pixel-edge units; index = a - 1/2
    with np.errstate(invalid="ignore"):
        x, y = a - 0.5, b - 0.5
        deep = inside & (x >= c0 + 1) & (x <= c1 - 2) & (y >= r0 + 1) & (y <= r1 - 2)      # every tap of the up sample is in the block
        far = ~((x > c0 - 2.5) & (x < c1 + 1.5) & (y > r0 - 2.5) & (y < r1 + 1.5))          # no tap of either sample is in it (the two samples lie < 1.5 px apart)
    assert deep.sum() >= 20 and not np.isfinite(l1[deep]).any() and not np.isfinite(u1[:, deep]).any()
    assert np.array_equal(np.isfinite(l1)[far], np.isfinite(l0)[far])
    same = far & np.isfinite(l0)
    assert np.array_equal(l1[same], l0[same]) and np.array_equal(u1[:, same], u0[:, same])
    lost = np.isfinite(l0) & ~np.isfinite(l1)
    assert lost.sum() < 1.6 * deep.sum() + 60   # a rim of less than a pixel around the block, not more
    # NaN never leaks into a valid pixel, and all three planes agree
    assert np.array_equal(np.isfinite(u1).all(0), np.isfinite(l1))
    # a source that is all NaN gives all NaN
    u2, l2, _ = reproject_fields_model(np.full_like(up, np.nan), np.full_like(lat, np.nan), s, d, H, W)
    assert not np.isfinite(u2).any() and not np.isfinite(l2).any()
    ups, lats, thetas, Hp, Wp = composition_inputs("ragged5")
    uc, lc, S, _ = compose_fields_model([np.full_like(u, np.nan) for u in ups], lats, thetas, Hp, Wp)
    assert not np.isfinite(uc).any() and not np.isfinite(lc).any() and (S == 0).all()


def test_view_order_non_finite_views_and_the_empty_panorama():
    ups, lats, thetas, Hp, Wp = composition_inputs("ragged5")
    base = compose_fields_model(ups, lats, thetas, Hp, Wp)
    bad = list(thetas)
    bad[2] = (np.nan,) + tuple(bad[2][1:])
    without = compose_fields_model(ups[:2] + ups[3:], lats[:2] + lats[3:], thetas[:2] + thetas[3:], Hp, Wp)
    with_nan = compose_fields_model(ups, lats, bad, Hp, Wp)
    for x, y in zip(without[:3], with_nan[:3]):
        assert np.array_equal(x, y, equal_nan=True)
    assert not np.array_equal(base[2], without[2])
    empty = compose_fields_model([], [], [], Hp, Wp)
    assert not np.isfinite(empty[0]).any() and not np.isfinite(empty[1]).any() and (empty[2] == 0).all()


# ---------------------------------------------------------------- host-side contract (fails before the feature exists)
NEW_SYMBOLS = ("pf_reproject_fields", "pf_compose_fields")
CAM = dict(roll=0.0, pitch=0.0, rel_focal=1.0)


def test_names_are_exported_and_all_keeps_its_names():
    import perspectivefields_amd
    from perspectivefields_amd import PerspectiveFields

    assert len(perspectivefields_amd.__all__) == 32
    for name in ("reproject_fields", "compose_panorama_fields"):
        assert perspectivefields_amd._HOME[name] == "gathers" and name not in perspectivefields_amd.__all__
        assert callable(getattr(perspectivefields_amd, name))
    assert callable(PerspectiveFields.inference_panorama)


def test_symbols_prototypes_and_the_limit():
    from perspectivefields_amd import perspectivefields as pfm
    from perspectivefields_amd.engine import _SIGNATURES, declared_symbols, load_library

    hdr = open(os.path.join(ROOT, "include", "pf_hip.h")).read()
    lib = load_library()
    for name in NEW_SYMBOLS:
        assert name in declared_symbols() and f"int {name}(int device, " in hdr and hasattr(lib, name)
    assert len(_SIGNATURES["pf_reproject_fields"][1]) == 14 and len(_SIGNATURES["pf_compose_fields"][1]) == 15
    assert f"#define PF_COMPOSE_FIELDS_MAX_VIEWS {pfm._COMPOSE_MAX_VIEWS}" in hdr
    kh = open(os.path.join(ROOT, "perspectivefields_amd", "csrc", "field_transport.h")).read()
    assert "usm_push" in kh and "usm_lift" in kh and "usm_push" in hdr and "usm_lift" in hdr


def test_cpu_tensors_raise():
    from perspectivefields_amd import compose_panorama_fields, reproject_fields
    from perspectivefields_amd.engine import PfError

    for up, lat in ((torch.zeros((2, 8, 16)), torch.zeros((8, 16))), (torch.zeros((3, 2, 8, 16)), torch.zeros((3, 8, 16))),
                    ([torch.zeros((2, 8, 16))], [torch.zeros((8, 16))])):
        with pytest.raises(PfError):
            reproject_fields(up, lat, CAM, CAM)
        with pytest.raises(PfError):
            compose_panorama_fields(up, lat, CAM, height=8, width=16)


def test_python_argument_errors_before_the_library_is_loaded(monkeypatch):
    from perspectivefields_amd import engine
    from perspectivefields_amd import perspectivefields as pfm

    def no_library(*a, **k):
        raise AssertionError("the library was loaded before the arguments were checked")

    monkeypatch.setattr(engine, "load_library", no_library)
    monkeypatch.setattr(pfm.torch, "is_tensor", lambda v: isinstance(v, (torch.Tensor, FakeCuda)))
    F = lambda *s: FakeCuda(s, torch.float32)
    up, lat = F(2, 8, 16), F(8, 16)
    bad = [
        dict(up=F(3, 8, 16)), dict(up=F(8, 16)), dict(lat=F(8, 15)), dict(up=F(2, 1, 16), lat=F(1, 16)), dict(up=F(2, 8, 1), lat=F(8, 1)), dict(up=[], lat=[]),
        dict(up=[up, up], lat=[lat]), dict(up=[up, F(2, 6, 16)], lat=[lat, F(6, 16)]), dict(up=[up, F(2, 6, 16)], lat=[lat, F(6, 16)], height=4),
        dict(height=1), dict(width=1, height=3), dict(mode="grad"), dict(src_index=[1]), dict(src_index=[-1]), dict(src_index=[]),
        dict(src=dict(roll=0.0, pitch=0.0)), dict(dst=dict(CAM, fov=1.0)), dict(src=dict(CAM, xi=np.zeros((2, 2)))),
        dict(src=dict(CAM, roll=[1.0, 2.0]), dst=dict(CAM, pitch=[1.0, 2.0, 3.0])), dict(up=[up, up, up], lat=[lat, lat, lat], src=dict(CAM, roll=[1.0, 2.0])),
        dict(src_index=[0, 0, 0], dst=dict(CAM, roll=[1.0, 2.0])),
    ]
    for kw in bad:
        args = dict(up=up, lat=lat, src=CAM, dst=CAM)
        args.update(kw)
        with pytest.raises(ValueError):
            pfm.reproject_fields(args.pop("up"), args.pop("lat"), args.pop("src"), args.pop("dst"), **args)
    with pytest.raises(TypeError):
        pfm.reproject_fields(up, [lat], CAM, CAM)
    with pytest.raises(TypeError):
        pfm.reproject_fields(up, lat, (0.0, 0.0, 1.0), CAM)
    with pytest.raises(TypeError):
        pfm.reproject_fields(up, lat, CAM, CAM, samples=2)   # out of scope: there is no such argument
    bad = [
        dict(up=F(3, 8, 16)), dict(up=F(2, 1, 16), lat=F(1, 16)), dict(up=[], lat=[]), dict(height=0), dict(width=0), dict(mode="grad"), dict(blend="max"),
        dict(pano_index=[0, 0]), dict(pano_index=[-1]), dict(pano_index=[1], n_pano=1), dict(n_pano=0), dict(cams=dict(roll=0.0, pitch=0.0)),
        dict(cams=dict(CAM, roll=[1.0, 2.0])), dict(up=[up] * 33, lat=[lat] * 33), dict(up=[up] * 34, lat=[lat] * 34, pano_index=[0] + [1] * 33),
    ]
    for kw in bad:
        args = dict(up=up, lat=lat, cams=CAM, height=8, width=16)
        args.update(kw)
        with pytest.raises(ValueError):
            pfm.compose_panorama_fields(args.pop("up"), args.pop("lat"), args.pop("cams"), **args)
    with pytest.raises(TypeError):
        pfm.compose_panorama_fields(up, lat, CAM)   # height and width are required
    with pytest.raises(TypeError):
        pfm.compose_panorama_fields(up, lat, CAM, height=8, width=16, fill=0)   # fields have no fill: NaN is the mask


def test_model_method_argument_errors_without_a_gpu():
    from perspectivefields_amd import PerspectiveFields

    ok = FakeCuda((8, 16, 3))
    for kw in (dict(n_yaw=0), dict(view_pitch=()), dict(n_yaw=12), dict(vfov=180.0), dict(blend="max"), dict(view_size=4), dict(height=8), dict(samples=5)):
        with pytest.raises(ValueError):
            PerspectiveFields.inference_panorama(None, ok, **kw)
    with pytest.raises(TypeError):
        PerspectiveFields.inference_panorama(None, np.zeros((8, 16, 3)))


def test_pf_reproject_fields_rejects_bad_arguments_in_the_stated_order():
    from perspectivefields_amd.engine import load_library

    lib = load_library()
    ints = lambda *s: (ctypes.c_int32 * len(s))(*s)
    ptrs = lambda n: (ctypes.c_void_p * n)(*([0x1000] * n))
    dev = ctypes.c_void_p(256)

    def call(n=1, pu="ok", pl="ok", hw=None, idx=(0,), B=None, c_idx=True, cs=dev, cd=dev, H=4, W=4, up=dev, lat=dev):
        pick = lambda p: ptrs(max(n, 1)) if p == "ok" else None if p == "null" else p
        rc = lib.pf_reproject_fields(0, n, pick(pu), pick(pl), hw or ints(*([8, 16] * max(n, 1))), len(idx) if B is None else B, ints(*idx) if c_idx else None, cs, cd,
                                     H, W, up, lat, None)
        return rc, lib.pf_last_error(None).decode()

    for kw, what in ((dict(n=0), "at least one"), (dict(pu="null"), "at least one"), (dict(pl="null"), "at least one"), (dict(pu=(ctypes.c_void_p * 1)()), "NULL"),
                     (dict(pl=(ctypes.c_void_p * 1)()), "NULL"), (dict(hw=ints(1, 16)), "smaller than 2 x 2"), (dict(hw=ints(8, 1)), "smaller than 2 x 2"),
                     (dict(B=0), "required"), (dict(c_idx=False), "required"), (dict(cs=None), "required"), (dict(cd=None), "required"), (dict(up=None), "required"),
                     (dict(lat=None), "required"), (dict(H=1), "output size"), (dict(W=1), "output size"), (dict(idx=(1,)), "index"), (dict(idx=(-1,)), "index"),
                     # the order: an earlier fault wins
                     (dict(hw=ints(1, 16), up=None, H=1, idx=(5,)), "smaller than 2 x 2"), (dict(up=None, H=1, idx=(5,)), "required"), (dict(H=1, idx=(5,)), "output size")):
        rc, msg = call(**kw)
        assert rc == -1 and what in msg and msg.startswith("pf_reproject_fields"), (kw, rc, msg)
    if not torch.cuda.is_available():
        rc, msg = call(n=2, idx=tuple(k % 2 for k in range(33)))
        assert rc == -2 and "no HIP device" in msg, (rc, msg)


def test_pf_compose_fields_rejects_bad_arguments_in_the_stated_order():
    from perspectivefields_amd.engine import load_library

    lib = load_library()
    ints = lambda *s: (ctypes.c_int32 * len(s))(*s)
    ptrs = lambda n: (ctypes.c_void_p * n)(*([0x1000] * n))
    dev = ctypes.c_void_p(256)

    def call(n=1, pu="ok", pl="ok", hw=None, idx=(0,), c_idx=True, cam=dev, n_pano=1, Hp=4, Wp=8, blend=0, up=dev, lat=dev, weight=None):
        pick = lambda p: ptrs(max(n, 1)) if p == "ok" else None if p == "null" else p
        rc = lib.pf_compose_fields(0, n, pick(pu), pick(pl), hw or ints(*([8, 16] * max(n, 1))), ints(*idx) if c_idx else None, cam, n_pano, Hp, Wp, blend, up, lat, weight,
                                   None)
        return rc, lib.pf_last_error(None).decode()

    for kw, what in ((dict(n=0), "at least one"), (dict(pu="null"), "at least one"), (dict(pl="null"), "at least one"), (dict(blend=2), "blend"), (dict(blend=-1), "blend"),
                     (dict(pu=(ctypes.c_void_p * 1)()), "NULL"), (dict(hw=ints(1, 16)), "smaller than 2 x 2"), (dict(hw=ints(8, 1)), "smaller than 2 x 2"),
                     (dict(n_pano=0), "required"), (dict(c_idx=False), "required"), (dict(cam=None), "required"), (dict(up=None), "required"), (dict(lat=None), "required"),
                     (dict(Hp=0), "size"), (dict(Wp=0), "size"), (dict(idx=(1,)), "index"), (dict(idx=(-1,)), "index"), (dict(n=2, idx=(1, 0), n_pano=2), "decrease"),
                     (dict(n=33, idx=(0,) * 33), "more than 32 views"), (dict(n=34, idx=(0,) + (1,) * 33, n_pano=2), "more than 32 views"),
                     (dict(blend=2, hw=ints(1, 16), up=None), "blend"), (dict(hw=ints(1, 16), up=None, Hp=0), "smaller than 2 x 2"), (dict(up=None, Hp=0), "required")):
        rc, msg = call(**kw)
        assert rc == -1 and what in msg and msg.startswith("pf_compose_fields"), (kw, rc, msg)
    if not torch.cuda.is_available():   # 32 views of one panorama and 33 over two pass the argument checks and fail on the missing device only
        for kw in (dict(n=32, idx=(0,) * 32), dict(n=33, idx=(0,) * 16 + (1,) * 17, n_pano=2), dict(Hp=1, Wp=1)):
            rc, msg = call(**kw)
            assert rc == -2 and "no HIP device" in msg, (kw, rc, msg)


def test_transport_kernels_are_in_the_library_without_scratch():
    """scripts/kernel_resources.py on the built library: the three kernels are there for gfx950 with no spilled register and no scratch"""
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
    for name in ("pf::reproject_fields_kernel", "pf::compose_fields_kernel<false>", "pf::compose_fields_kernel<true>"):
        r = by[name]
        assert r["spill"] == 0 and r["scratch"] == 0 and r["lds"] <= 3072, r
