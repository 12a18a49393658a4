"""fp64 numpy reference of the fisheye lens fit (include/pf_hip.h pf_fit_fisheye): the model with its domain rule, written once
over plain arrays and over forward-mode dual numbers (the analytic Jacobian), held against tests.test_fisheye_target_ref.target_fields, the fp64
statement of the labels; the blind start of the kernel; a Levenberg-Marquardt reference (scipy) and the proof that the inputs of
tests/test_gpu_fit_fisheye.py are recoverable by it alone; the float32 Newton residual behind PF_FISHFIT_ROOT_TOL; plus the host-side contract of
fit_fisheye_lens / fisheye_lens_from_fit and of the two C entry points (no GPU needed).

THE CASES.  A fit from the blind start holds what is not free at 0, so a case is a truth with its held entries set to 0: the free set (r, p, f) of a
truth is the lens (r, p, f, 0, 0, 0, 0), (r, p, f, k1, k2) is (r, p, f, 0, 0, k1, k2), all seven is the truth itself."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest
import torch

from tests.test_fisheye_ref import EQUIDISTANT, EQUISOLID, KIND_NAMES, STEREOGRAPHIC, distort
from tests.test_fisheye_target_ref import NEWTON_STEPS, UP_MIN_T2, newton, target_fields
from tests.test_fit_camera_ref import rho as loss_rho

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R2D = 180.0 / np.pi
R_MIN, SLOPE_MIN, ROOT_TOL = 1e-3, 1e-2, 4e-6   # include/pf_hip.h PF_FISHFIT_R_MIN, _SLOPE_MIN, _ROOT_TOL
KINDS = (EQUIDISTANT, EQUISOLID, STEREOGRAPHIC)
TMAX_DEG = 115.0                                # theta_max of the tests: max_fov = 230
TMAX = np.radians(TMAX_DEG)
# (roll, pitch [deg], f, cx, cy, k1, k2), the full field of view of the generated fields [deg]
TRUTHS = (((12.0, 35.0, 0.33, 0.0, 0.0, 0.0, 0.0), 190.0), ((-30.0, -60.0, 0.4, 0.05, -0.04, -0.03, 0.004), 170.0), ((5.0, 10.0, 0.55, 0.0, 0.0, 0.02, -0.002), 120.0))
FREE_SETS = {3: (0, 1, 2), "5pp": (0, 1, 2, 3, 4), "5k": (0, 1, 2, 5, 6), 7: (0, 1, 2, 3, 4, 5, 6)}   # free_pp, poly = (0, 0), (1, 0), (0, 1), (1, 1)
FREE_FLAGS = {3: (False, False), "5pp": (True, False), "5k": (False, True), 7: (True, True)}
REF_SETS = (3, "5k", 7)
SIZE = (48, 64)


def case_theta(truth, free):
    """the lens of a case, angles in radians: the truth with what the free set holds set to 0"""
    th = np.array(truth, dtype=np.float64)
    th[:2] = np.radians(th[:2])
    held = [k for k in range(7) if k not in FREE_SETS[free]]
    th[held] = 0.0
    return th


def lens_row_of(theta, H, W, tmax):
    """theta -> the 12-float lens row of the fisheye gathers"""
    r, p, f, cx, cy, k1, k2 = (float(v) for v in theta)
    return np.array([r, p, 0.0, f * H, (cx + 0.5) * W, (cy + 0.5) * H, tmax, k1, k2, 0.0, 0.0, 0.0])


@functools.lru_cache(None)
def case_fields(t_i, free, kind, H, W):
    """the exact input of a case: target_fields of its lens over its field of view; NaN outside the image circle.  Read only"""
    truth, fov = TRUTHS[t_i]
    th = case_theta(truth, free)
    up, lat, _, _ = target_fields([lens_row_of(th, H, W, np.radians(fov / 2))], kind, H, W)
    up.setflags(write=False)
    lat.setflags(write=False)
    return th, up, lat


# ---------------------------------------------------------------- forward-mode dual numbers over arrays: v (...), d (..., N)
class Dual:
    __array_ufunc__ = None   # ndarray - Dual is Dual.__rsub__, not an array of objects

    def __init__(self, v, d):
        self.v, self.d = v, d

    @staticmethod
    def lift(x, like):
        return x if isinstance(x, Dual) else Dual(np.asarray(x, dtype=np.float64) + 0 * like.v, 0 * like.d)

    def _fn(self, v, g):
        return Dual(v, self.d * np.asarray(g)[..., None])

    def __add__(self, o):
        o = Dual.lift(o, self)
        return Dual(self.v + o.v, self.d + o.d)

    __radd__ = __add__

    def __neg__(self):
        return Dual(-self.v, -self.d)

    def __sub__(self, o):
        return self + (-Dual.lift(o, self))

    def __rsub__(self, o):
        return Dual.lift(o, self) - self

    def __mul__(self, o):
        o = Dual.lift(o, self)
        return Dual(self.v * o.v, self.d * o.v[..., None] + o.d * self.v[..., None])

    __rmul__ = __mul__

    def __truediv__(self, o):
        o = Dual.lift(o, self)
        return self * o._fn(1.0 / o.v, -1.0 / (o.v * o.v))

    def __rtruediv__(self, o):
        return Dual.lift(o, self) / self


def _un(x, f, g):
    return x._fn(f(x.v), g(x.v)) if isinstance(x, Dual) else f(x)


def d_sqrt(x): return _un(x, np.sqrt, lambda v: 0.5 / np.sqrt(v))
def d_sin(x): return _un(x, np.sin, np.cos)
def d_cos(x): return _un(x, np.cos, lambda v: -np.sin(v))
def d_asin(x): return _un(x, np.arcsin, lambda v: 1.0 / np.sqrt(1.0 - v * v))
def d_atan(x): return _un(x, np.arctan, lambda v: 1.0 / (1.0 + v * v))
def val(x): return x.v if isinstance(x, Dual) else x


def d_atan2(y, x):
    if not isinstance(y, Dual):
        return np.arctan2(y, x)
    q = 1.0 / (x.v * x.v + y.v * y.v)
    return Dual(np.arctan2(y.v, x.v), y.d * (x.v * q)[..., None] - x.d * (y.v * q)[..., None])


# ---------------------------------------------------------------- the model
def lens_model(theta, kind, H, W, tmax=TMAX, free=None):
    """theta (radians) -> dict: up (2, H, W), lat (H, W) degrees, has (H, W) the pixel has a model value, ok_up (H, W) its up rows are on, t (theta),
    slope (P'), root (|P(theta) - theta_d|); with free = a tuple of places in theta also J_up (2, H, W, NP) and J_lat (H, W, NP), the analytic
    derivatives by the implicit function.  Values where has is False are meaningless (NaN or finite)."""
    a = np.arange(W)[None, :] + 0.5 + np.zeros((H, 1))
    b = np.arange(H)[:, None] + 0.5 + np.zeros((1, W))
    th = [np.float64(v) for v in theta]
    if free is not None:
        NP = len(free)
        z = np.zeros((H, W))
        th = [Dual(z + v, np.zeros((H, W, NP)) + (np.arange(NP) == free.index(k) if k in free else 0.0)) for k, v in enumerate(th)]
    roll, pitch, f, cx, cy, k1, k2 = th
    k1v, k2v = float(theta[5]), float(theta[6])
    sr, cr, sp, cp = d_sin(roll), d_cos(roll), d_sin(pitch), d_cos(pitch)
    g = (-(cp * sr), -(cp * cr), sp)
    F, Cx, Cy = f * H, (cx + 0.5) * W, (cy + 0.5) * H
    with np.errstate(all="ignore"):
        dx, dy = a - Cx, b - Cy
        r = d_sqrt(dx * dx + dy * dy)
        rho = r / F
        has = val(r) - R_MIN > 0
        if kind == EQUISOLID:
            has &= 2.0 - val(rho) > 0
        td = rho if kind == EQUIDISTANT else 2.0 * d_asin(rho * 0.5) if kind == EQUISOLID else 2.0 * d_atan(rho * 0.5)
        poly = k1v != 0.0 or k2v != 0.0
        lens = np.array([0, 0, 0, 0, 0, 0, tmax, k1v, k2v, 0.0, 0.0, 0])
        t = newton(lens, val(td)) if poly else val(td)
        slope = 1.0 + t * t * (3.0 * k1v + t * t * 5.0 * k2v)
        root = np.abs(distort(lens, t) - val(td))
        has &= (tmax - t > 0) & (t > 0)
        if poly:
            has &= (slope >= SLOPE_MIN) & (root <= ROOT_TOL)
        if free is not None:   # d theta = (d theta_d - theta^3 d k1 - theta^5 d k2) / P'(theta)
            t = Dual(t, (td.d - (t ** 3)[..., None] * k1.d - (t ** 5)[..., None] * k2.d) / slope[..., None])
        c, s = dx / r, dy / r
        st, ct = d_sin(t), d_cos(t)
        X = (st * c, st * s, ct)
        Xg = X[0] * g[0] + X[1] * g[1] + X[2] * g[2]
        xw = X[0] * cr - X[1] * sr
        zw = X[0] * (sp * sr) + X[1] * (sp * cr) + X[2] * cp
        lat = -(d_atan2(-Xg, d_sqrt(xw * xw + zw * zw)) * R2D)
        ge = ct * (g[0] * c + g[1] * s) - g[2] * st
        gp = g[1] * c - g[0] * s
        ms = 1.0 + t * t * (3.0 * k1 + t * t * (5.0 * k2))
        if kind != EQUIDISTANT:
            ch = d_cos(td * 0.5)
            ms = ms * ch if kind == EQUISOLID else ms / (ch * ch)
        A, B = ms * ge, rho / st * gp
        px, py = A * c - B * s, A * s + B * c
        n = d_sqrt(px * px + py * py)
        ux, uy = px / n, py / n
        ok_up = val(ge) ** 2 + val(gp) ** 2 >= UP_MIN_T2
    out = dict(up=np.stack([val(ux), val(uy)]), lat=val(lat), has=has, ok_up=ok_up & has, t=val(t), slope=slope, root=root)
    if free is not None:
        out["J_up"], out["J_lat"] = np.stack([ux.d, uy.d]), lat.d
    return out


def residuals(theta, kind, up_in, lat_in, tmax=TMAX, free=None):
    """the residual rows of every pixel, 0 where they are off: r_up (2, H, W) degree scale, r_lat (H, W) degrees, the pixels counted (finite input and
    a model value); with `free` the Jacobians of both as well"""
    H, W = lat_in.shape
    m = lens_model(theta, kind, H, W, tmax, free)
    fin = np.isfinite(up_in).all(0) & np.isfinite(lat_in)
    cnt = fin & m["has"]
    on_up = cnt & m["ok_up"]
    with np.errstate(invalid="ignore"):
        ru = np.where(on_up[None], (m["up"] - up_in) * R2D, 0.0)
        rl = np.where(cnt, m["lat"] - lat_in, 0.0)
    if free is None:
        return ru, rl, cnt
    return ru, rl, cnt, np.where(on_up[None, ..., None], m["J_up"] * R2D, 0.0), np.where(cnt[..., None], m["J_lat"], 0.0)


def cost(theta, kind, up_in, lat_in, tmax=TMAX, loss="l2", delta=2.0, weights=(1.0, 1.0)):
    ru, rl, _ = residuals(theta, kind, up_in, lat_in, tmax)
    return float(weights[0] * loss_rho(np.sqrt((ru * ru).sum(0)), loss, delta).sum() + weights[1] * loss_rho(rl, loss, delta).sum())


def valid_pixels(theta, kind, up_in, lat_in, tmax=TMAX):
    return int(residuals(theta, kind, up_in, lat_in, tmax)[2].sum())


def kind_rho(kind, h):
    return h if kind == EQUIDISTANT else 2.0 * np.sin(0.5 * h) if kind == EQUISOLID else 2.0 * np.tan(0.5 * h)


def blind_start(kind, up, lat, tmax=TMAX):
    """the start of pf_fit_fisheye without d_init: roll / pitch from the 4 x 4 centre pixels, zeros, f = the best of the 16 candidates
    0.5 / rho((20 + 7 c) deg) by the cost on a 32 x 32 subsample"""
    H, W = lat.shape
    rows, cols = np.arange(H // 2 - 2, H // 2 + 2), np.arange(W // 2 - 2, W // 2 + 2)
    u, l = up[:, rows][:, :, cols], lat[rows][:, cols]
    fu, fl = np.isfinite(u).all(0), np.isfinite(l)
    roll = np.arctan2(-u[0][fu].sum(), -u[1][fu].sum()) if fu.any() else 0.0
    pitch = np.radians(l[fl].mean()) if fl.any() else 0.0
    pitch = min(max(pitch, -np.radians(89.9)), np.radians(89.9))
    s = np.arange(32)
    sr = np.minimum(((s + 0.5) * H / 32).astype(int), H - 1)
    sc = np.minimum(((s + 0.5) * W / 32).astype(int), W - 1)
    best = (np.inf, 1.0)
    for c in range(16):
        f = 0.5 / kind_rho(kind, np.radians(20.0 + 7.0 * c))
        ru, rl, _ = residuals((roll, pitch, f, 0, 0, 0, 0), kind, up, lat, tmax)
        cst = 0.5 * (ru[:, sr][:, :, sc] ** 2).sum() + 0.5 * (rl[sr][:, sc] ** 2).sum()
        if cst < best[0]:
            best = (cst, f)
    return np.array([roll, pitch, best[1], 0.0, 0.0, 0.0, 0.0])


def clamp(th):
    th = np.array(th, dtype=np.float64)
    th[0] = np.remainder(th[0] + np.pi, 2 * np.pi) - np.pi
    th[1] = np.clip(th[1], -np.radians(89.9), np.radians(89.9))
    th[2] = max(th[2], 1e-3)
    th[5:7] = np.clip(th[5:7], -0.5, 0.5)
    return th


def reference_fit(kind, up, lat, start, free, tmax=TMAX):
    """scipy's Levenberg-Marquardt on the fp64 reference over the free places of theta, from `start`, with the analytic Jacobian; a pixel that is off
    keeps its (zero) rows, so the residual vector has one length"""
    from scipy.optimize import least_squares

    free = tuple(free)
    th0 = np.array(start, dtype=np.float64)

    def full(t):
        th = th0.copy()
        th[list(free)] = t
        return clamp(th)

    def fun(t):
        ru, rl, _ = residuals(full(t), kind, up, lat, tmax)
        return np.concatenate([ru.ravel(), rl.ravel()])

    def jac(t):
        _, _, _, ju, jl = residuals(full(t), kind, up, lat, tmax, free)
        return np.concatenate([ju.reshape(-1, len(free)), jl.reshape(-1, len(free))])

    scale = np.ones(len(free))
    scale[free.index(2)] = max(th0[2], 1e-3)
    s = least_squares(fun, th0[list(free)], jac=jac, method="lm", x_scale=scale, xtol=1e-15, ftol=1e-15, gtol=1e-15, max_nfev=400)
    return full(s.x), s


def smooth_noise(H, W, seed, amp_deg=1.5):
    """smooth noise of about amp_deg for the three planes: a few low-frequency waves with seeded phases -> (3, H, W) degrees"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W] / max(H, W)
    out = np.zeros((3, H, W))
    for p in range(3):
        for _ in range(4):
            fx, fy, ph = rng.uniform(-3, 3), rng.uniform(-3, 3), rng.uniform(0, 2 * np.pi)
            out[p] += np.sin(2 * np.pi * (fx * x + fy * y) + ph)
        out[p] *= amp_deg / 2.0
    return out


@functools.lru_cache(None)
def noisy_case(kind=EQUIDISTANT, H=SIZE[0], W=SIZE[1], seed=11):
    """the noisy input: the full second truth's fields with smooth 1.5 deg noise, the up vectors turned by their plane's noise, rounded to float32
    (what the GPU is given) and held in fp64.  Read only"""
    th, up, lat = case_fields(1, 7, kind, H, W)
    nz = smooth_noise(H, W, seed)
    ang = np.radians(nz[0])
    upn = np.stack([up[0] * np.cos(ang) - up[1] * np.sin(ang), up[0] * np.sin(ang) + up[1] * np.cos(ang)])
    latn = (lat + nz[2]).astype(np.float32).astype(np.float64)
    upn = upn.astype(np.float32).astype(np.float64)
    upn.setflags(write=False)
    latn.setflags(write=False)
    return th, upn, latn


@functools.lru_cache(None)
def noisy_reference(free, kind=EQUIDISTANT):
    """the reference fit of the noisy case over a free set, from the truth with the held entries at the truth -> (theta, cost)"""
    th, up, lat = noisy_case(kind)
    fit, _ = reference_fit(kind, up, lat, th, FREE_SETS[free])
    return fit, cost(fit, kind, up, lat)


# ---------------------------------------------------------------- the reference against the statement of the labels, and itself
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("t_i", range(3))
def test_the_model_is_target_fields_inside_the_image_circle(t_i, kind):
    for H, W in (SIZE, (33, 47)):
        th, up, lat = case_fields(t_i, 7, kind, H, W)
        m = lens_model(th, kind, H, W)
        a, b = np.meshgrid(np.arange(W) + 0.5 - (th[3] + 0.5) * W, np.arange(H) + 0.5 - (th[4] + 0.5) * H)
        centre = np.hypot(a, b) <= R_MIN   # the one pixel the polar form loses: where both sides are odd and the lens is centred
        assert centre.sum() == (1 if H % 2 and W % 2 and th[3] == 0 and th[4] == 0 else 0) and not m["has"][centre].any()
        own = np.isfinite(lat) & ~centre
        assert own.sum() > 0.3 * H * W
        assert m["has"][own].all()   # theta < fov / 2 < theta_max, and the iteration has converged
        fin = own & np.isfinite(up[0])
        assert np.abs(m["lat"] - lat)[own].max() <= 1e-9 and np.abs(m["up"] - up)[:, fin].max() <= 1e-9
        assert (m["ok_up"][own] == np.isfinite(up[0])[own]).all()


@pytest.mark.parametrize("kind", KINDS)
def test_implicit_derivative_and_jacobian_agree_with_central_differences(kind):
    H, W = 12, 16
    th = case_theta(TRUTHS[1][0], 7)
    th[2] = 0.6 if kind == EQUISOLID else 0.4   # the equisolid kind: rho < 2 over the whole frame
    free = FREE_SETS[7]
    up0, lat0 = np.zeros((2, H, W)), np.zeros((H, W))
    ru, rl, cnt, ju, jl = residuals(th, kind, up0, lat0, free=free)
    assert cnt.sum() >= 0.9 * H * W
    m = lens_model(th, kind, H, W)
    sel = cnt & (np.abs(m["t"] - TMAX) > 1e-3)
    a = lens_model(th, kind, H, W, free=free)
    for k in range(7):
        h = 1e-6
        tp, tm = th.copy(), th.copy()
        tp[k] += h
        tm[k] -= h
        mp, mm = lens_model(tp, kind, H, W), lens_model(tm, kind, H, W)
        # the implicit derivative of theta itself
        fd_t = (mp["t"] - mm["t"]) / (2 * h)
        an_t = _theta_derivative(th, kind, H, W, k)
        assert np.abs(fd_t - an_t)[sel].max() <= 1e-6 * max(1.0, np.abs(an_t[sel]).max()), k
        fd_u = (mp["up"] - mm["up"]) / (2 * h)
        fd_l = (mp["lat"] - mm["lat"]) / (2 * h)
        on = sel & m["ok_up"]
        assert np.abs(fd_u - a["J_up"][..., k])[:, on].max() <= 1e-6 * max(1.0, np.abs(fd_u[:, on]).max()), k
        assert np.abs(fd_l - a["J_lat"][..., k])[sel].max() <= 1e-6 * max(1.0, np.abs(fd_l[sel]).max()), k


def _theta_derivative(th, kind, H, W, k):
    """d theta / d parameter k by the implicit function, from the pieces of the model alone"""
    a = np.arange(W)[None, :] + 0.5 + np.zeros((H, 1))
    b = np.arange(H)[:, None] + 0.5 + np.zeros((1, W))
    r_, p_, f, cx, cy, k1, k2 = th
    dx, dy = a - (cx + 0.5) * W, b - (cy + 0.5) * H
    r = np.hypot(dx, dy)
    rho = r / (f * H)
    drho = {2: -rho / f, 3: -dx / r * W / (f * H), 4: -dy / r * H / (f * H)}.get(k, 0.0 * rho)
    dtd = drho * (1.0 if kind == EQUIDISTANT else 1.0 / np.sqrt(1.0 - rho * rho / 4) if kind == EQUISOLID else 1.0 / (1.0 + rho * rho / 4))
    m = lens_model(th, kind, H, W)
    t = m["t"]
    return (dtd - (t ** 3 if k == 5 else 0.0) - (t ** 5 if k == 6 else 0.0)) / m["slope"]


@pytest.mark.parametrize("kind", KINDS)
def test_blind_start_is_exact_at_the_circle_centre(kind):
    """at r -> 0 the up vector is (-sin roll, -cos roll) and the latitude is the pitch, for every kind, f and polynomial"""
    for truth, _ in TRUTHS:
        th = case_theta(truth, 7)
        H = W = 9
        eps = 1e-7   # a frame whose pixel centres surround the circle centre at 1e-7 of a pixel: scale the geometry, not the model
        th2 = th.copy()
        th2[2] = th[2] / eps
        th2[3] = th2[4] = 0.0
        m = lens_model(th2, kind, H, W)
        ring = m["has"] & (np.hypot(*np.meshgrid(np.arange(W) - 4.0, np.arange(H) - 4.0)) < 1.5)
        assert ring.sum() == 8
        assert np.abs(m["up"][0][ring] + np.sin(th[0])).max() <= 1e-5 and np.abs(m["up"][1][ring] + np.cos(th[0])).max() <= 1e-5
        assert np.abs(m["lat"][ring] - np.degrees(th[1])).max() <= 1e-4
    # and the start the kernel computes from exact fields: roll and pitch of the centre pixels of a centred lens to the size of a pixel's angle
    th, up, lat = case_fields(0, 3, kind, *SIZE)
    st = blind_start(kind, up, lat)
    assert abs(st[0] - th[0]) <= np.radians(1.0) and abs(st[1] - th[1]) <= np.radians(1.0) and 0.5 <= st[2] / th[2] <= 2.0


@pytest.mark.parametrize("free", REF_SETS)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("t_i", range(3))
def test_reference_recovers_the_cases_from_the_blind_start(t_i, kind, free):
    th, up, lat = case_fields(t_i, free, kind, *SIZE)
    fit, s = reference_fit(kind, up, lat, blind_start(kind, up, lat), FREE_SETS[free])
    err = np.abs(fit - th)
    print(f"truth {t_i} {KIND_NAMES[kind]} free {free}: angles {np.degrees(err[:2]).max():.2e} deg, rest {err[2:].max():.2e}, nfev {s.nfev}")
    assert np.degrees(err[:2]).max() <= 1e-5 and err[2:].max() <= 1e-6
    assert valid_pixels(fit, kind, up, lat) == int(np.isfinite(lat).sum())   # both sides are even: no pixel centre is at r = 0


@pytest.mark.parametrize("kind", KINDS)
def test_no_pixel_of_the_fov_170_cases_is_near_a_domain_border(kind):
    """the condition of the GPU test of fit_valid_pixels, on the reference alone: at the truth no finite pixel is within 1e-3 of a border of the domain"""
    for free in FREE_SETS:
        for H, W in (SIZE, (33, 47)):
            th, up, lat = case_fields(1, free, kind, H, W)
            m = lens_model(th, kind, H, W)
            fin = np.isfinite(lat)
            a, b = np.meshgrid(np.arange(W) + 0.5 - (th[3] + 0.5) * W, np.arange(H) + 0.5 - (th[4] + 0.5) * H)
            assert np.abs(np.hypot(a, b) - R_MIN)[fin].min() >= 1e-3   # the nearest: the centre pixel of a centred lens at 33 x 47, at r = 0 exactly
            assert (TMAX - m["t"])[fin].min() > 1e-3 and (m["slope"][fin] - SLOPE_MIN).min() > 1e-3 and m["root"][fin].max() < ROOT_TOL / 16
            assert (m["has"] == (np.hypot(a, b) > R_MIN))[fin].all() and (~m["has"][fin]).sum() <= 1   # all but that centre pixel


@pytest.mark.parametrize("free", tuple(FREE_SETS))
def test_every_finite_pixel_keeps_its_model_value_on_the_noisy_case(free):
    th, up, lat = noisy_case()
    fit, c = noisy_reference(free)
    assert valid_pixels(fit, EQUIDISTANT, up, lat) == int((np.isfinite(up).all(0) & np.isfinite(lat)).sum())
    assert 0 < c < cost(th, EQUIDISTANT, up, lat) * (1 + 1e-12)
    assert np.degrees(np.abs(fit - th)[:2]).max() < 3.0   # the noise moves the solution, it does not let it run away


def newton_residual_f32():
    """the largest |P(theta) - theta_d| in numpy float32 after the 10 steps, over the pixels of the test lenses with a polynomial at both test sizes"""
    f = np.float32
    worst = 0.0
    for t_i in (1, 2):
        for kind in KINDS:
            for H, W in (SIZE, (33, 47), (97, 131)):
                th = case_theta(TRUTHS[t_i][0], 7)
                m = lens_model(th, kind, H, W)
                a = (np.arange(W, dtype=f)[None, :] + f(0.5)) - f((th[3] + 0.5) * W)
                b = (np.arange(H, dtype=f)[:, None] + f(0.5)) - f((th[4] + 0.5) * H)
                rho = np.sqrt(a * a + b * b) / f(th[2] * H)
                with np.errstate(invalid="ignore"):
                    td = rho if kind == EQUIDISTANT else f(2) * np.arcsin(np.minimum(rho * f(0.5), f(1))) if kind == EQUISOLID else f(2) * np.arctan(rho * f(0.5))
                lens = np.array([0, 0, 0, 0, 0, 0, TMAX, th[5], th[6], 0, 0, 0], dtype=f)
                t = newton(lens, td, f=f)
                assert t.dtype == f
                res = np.abs(distort(lens, t) - td)
                worst = max(worst, float(res[m["has"]].max()))
    return worst


def test_fp32_newton_residual_of_the_test_lenses_is_under_a_sixteenth_of_the_tolerance():
    worst = newton_residual_f32()
    print(f"float32 Newton residual after {NEWTON_STEPS} steps: {worst:.3e}; PF_FISHFIT_ROOT_TOL = {ROOT_TOL:g}")
    assert 0 < worst <= ROOT_TOL / 16
    hdr = open(os.path.join(ROOT, "include", "pf_hip.h")).read()
    assert float(re.search(r"#define PF_FISHFIT_ROOT_TOL (\S+?)f\b", hdr)[1]) == ROOT_TOL


# ---------------------------------------------------------------- the host side
ENTRY_POINTS = ("pf_fit_fisheye_workspace_bytes", "pf_fit_fisheye")
NAMES = ("fit_fisheye_lens", "fisheye_lens_from_fit")


def test_header_states_the_model_and_the_columns():
    from perspectivefields_amd.camera_fit import _FISHFIT_COLS, _FIT_COLS

    hdr = open(os.path.join(ROOT, "include", "pf_hip.h")).read()
    cols = {m[0]: int(m[1]) for m in re.findall(r"#define PF_FISHFIT_COL_([A-Z_0-9]+) (\d+)", hdr)}
    pin = {m[0]: int(m[1]) for m in re.findall(r"#define PF_FIT_COL_([A-Z_]+) (\d+)", hdr)}
    assert int(re.search(r"#define PF_FISHFIT_COLS (\d+)", hdr)[1]) == len(_FISHFIT_COLS) == len(cols) == 15
    assert {k: v for k, v in cols.items() if k not in ("K1", "K2")} == pin and cols["K1"] == 13 and cols["K2"] == 14
    assert _FISHFIT_COLS == _FIT_COLS + ("pred_k1", "pred_k2")
    assert re.search(r"#define PF_FISHFIT_R_MIN 1e-3f", hdr) and re.search(r"#define PF_FISHFIT_SLOPE_MIN 1e-2f", hdr)
    for text in ("theta = (roll r, pitch p, f, cx, cy, k1, k2)", "r - PF_FISHFIT_R_MIN > 0", "theta_max - theta > 0", "P'(theta) >= PF_FISHFIT_SLOPE_MIN",
                 "|P(theta) - theta_d| <= PF_FISHFIT_ROOT_TOL", "It is NOT r < r_max(theta_max)", "d theta = (d theta_d - theta^3 d k1 - theta^5 d k2) / P'(theta)",
                 "h_c = (20 + 7 c) degrees", "k1 and k2 in [-0.5, 0.5]", "for a fisheye lens they describe nothing"):
        assert text in hdr, text
    kh = open(os.path.join(ROOT, "perspectivefields_amd", "csrc", "pf_kernels.h")).read()
    assert "FISHFIT_STATE = 64" in kh and "FISHFIT_REC = 40" in kh
    from perspectivefields_amd import build as _b

    assert "fit_camera_fisheye.hip" in _b.SOURCES and _b.EXTRA_FLAGS["fit_camera_fisheye.hip"] == _b.NO_PK_F32_FLAGS


def test_symbols_are_in_the_library_with_the_declared_prototypes():
    from perspectivefields_amd.engine import _SIGNATURES, load_library

    lib = load_library()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pf_hip.h")).read(), flags=re.S)
    ctype = {"int": ctypes.c_int, "float": ctypes.c_float, "size_t": ctypes.c_size_t}
    for name in ENTRY_POINTS:
        m = re.search(r"(\w+)\s+" + name + r"\(([^;]*)\);", hdr)
        assert m, name
        want = [ctypes.c_void_p if "*" in a else ctype[a.split()[0]] for a in (a.strip() for a in m[2].split(","))]
        res, got = _SIGNATURES[name]
        assert res is ctype[m[1]] and got == want, (name, got, want)
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == want
    assert len(_SIGNATURES["pf_fit_fisheye"][1]) == 19


def test_workspace_size_and_small_images():
    from perspectivefields_amd.engine import load_library

    lib = load_library()
    hw = lambda *s: (ctypes.c_int32 * len(s))(*s)
    one = lib.pf_fit_fisheye_workspace_bytes(1, hw(640, 640))
    two = lib.pf_fit_fisheye_workspace_bytes(2, hw(640, 640, 97, 131))
    assert 0 < one < two
    assert one > lib.pf_fit_camera_usm_workspace_bytes(1, hw(640, 640))   # larger records and state than the USM fit
    assert lib.pf_fit_fisheye_workspace_bytes(1, hw(7, 640)) == 0
    assert lib.pf_fit_fisheye_workspace_bytes(2, hw(640, 640, 8, 7)) == 0
    assert lib.pf_fit_fisheye_workspace_bytes(0, hw(640, 640)) == 0
    assert lib.pf_fit_fisheye_workspace_bytes(-1, hw(640, 640)) == 0


def test_pf_fit_fisheye_rejects_bad_arguments_before_device_work_in_the_stated_order():
    from perspectivefields_amd.engine import load_library

    lib = load_library()
    hw = lambda *s: (ctypes.c_int32 * len(s))(*s)
    ptrs = lambda *p: (ctypes.c_void_p * len(p))(*p)
    dev = ctypes.c_void_p(256)

    def fit(kind=0, B=1, hw_=None, up=None, lat=None, free_pp=0, poly=0, tmax=2.0, loss=0, delta=2.0, w=(1.0, 1.0), max_iter=20, out=dev, ws=dev, ws_n=1 << 30):
        rc = lib.pf_fit_fisheye(0, kind, B, hw_ or hw(16, 16), up or ptrs(256), lat or ptrs(256), None, free_pp, poly, tmax, loss, delta, w[0], w[1], max_iter, out,
                                ws, ws_n, None)
        return rc, lib.pf_last_error(None).decode()

    # each later error is given together with every earlier-checked argument right; an earlier one wins over every later one
    for kw, what in ((dict(kind=3, tmax=0.0, B=0), "kind"), (dict(kind=-1, free_pp=2), "kind"), (dict(tmax=0.0, B=0), "theta_max"), (dict(tmax=-1.0), "theta_max"),
                     (dict(tmax=3.1415927), "theta_max"), (dict(tmax=float("nan"), out=None), "theta_max"), (dict(tmax=float("inf")), "theta_max"),
                     (dict(B=0, poly=2), "bad argument"), (dict(out=None), "bad argument"), (dict(free_pp=2), "bad option"), (dict(loss=3), "bad option"),
                     (dict(max_iter=0), "bad option"), (dict(poly=2), "bad option"), (dict(poly=-1), "bad option"), (dict(w=(0.0, 0.0)), "weights"),
                     (dict(w=(-1.0, 1.0)), "weights"), (dict(loss=1, delta=0.0), "huber_delta_deg"), (dict(hw_=hw(7, 16)), "smaller than 8 x 8"),
                     (dict(up=ptrs(None)), "NULL field pointer")):
        rc, msg = fit(**kw)
        assert rc == -1 and what in msg and msg.startswith("pf_fit_fisheye: "), (kw, rc, msg)
    rc, msg = fit(ws_n=16)
    assert rc == -4 and "workspace" in msg and msg.startswith("pf_fit_fisheye: "), (rc, msg)
    if not torch.cuda.is_available():   # every kind, both flags and a theta_max just inside pi are good arguments: they fail on the missing device only
        for kind in KINDS:
            rc, msg = fit(kind=kind, free_pp=1, poly=1, tmax=3.14159)
            assert rc == -2 and "no HIP device" in msg, (rc, msg)


def test_lens_fit_on_cpu_tensors_raises():
    from perspectivefields_amd import fit_fisheye_lens
    from perspectivefields_amd.engine import PfError

    _, up, lat = case_fields(0, 3, EQUIDISTANT, 33, 47)
    up, lat = torch.from_numpy(up.copy()).float(), torch.from_numpy(lat.copy()).float()
    with pytest.raises(PfError):
        fit_fisheye_lens(up, lat)
    with pytest.raises(PfError):
        fit_fisheye_lens([up], [lat], projection="stereographic", distortion=True, free_principal_point=True)


def test_python_argument_errors_before_the_library_is_loaded(monkeypatch):
    from tests.test_reproject_ref import FakeCuda

    from perspectivefields_amd import camera_fit, engine

    def no_library(*a, **k):
        raise AssertionError("the library was loaded before the arguments were checked")

    monkeypatch.setattr(engine, "load_library", no_library)
    monkeypatch.setattr(camera_fit.torch, "is_tensor", lambda v: isinstance(v, (torch.Tensor, FakeCuda)))
    up, lat = FakeCuda((2, 16, 24), torch.float32), FakeCuda((16, 24), torch.float32)
    for kw in (dict(projection="orthographic"), dict(max_fov=0.0), dict(max_fov=360.0), dict(max_fov=float("nan")), dict(max_fov=-10.0), dict(loss="l1"),
               dict(up=[up, up], lat=[lat]), dict(up=[], lat=[]), dict(up=FakeCuda((3, 16, 24), torch.float32)), dict(lat=FakeCuda((16, 25), torch.float32)),
               dict(up=FakeCuda((16, 24), torch.float32))):
        args = dict(up=up, lat=lat)
        args.update(kw)
        with pytest.raises(ValueError):
            camera_fit.fit_fisheye_lens(args.pop("up"), args.pop("lat"), **args)
    with pytest.raises(TypeError):
        camera_fit.fit_fisheye_lens([up, np.zeros((2, 16, 24))], [lat, lat])
    with pytest.raises(TypeError):
        camera_fit.fit_fisheye_lens(up, lat, "equisolid")   # the options are keyword-only
    for bad in (None, [], {"pred_roll": 0.0}):
        with pytest.raises(ValueError):
            camera_fit.fisheye_lens_from_fit(bad, height=16, width=24)
    ok = dict(pred_roll=1.0, pred_pitch=2.0, pred_rel_focal=0.4, pred_rel_cx=0.0, pred_rel_cy=0.0, pred_k1=0.0, pred_k2=0.0)
    with pytest.raises(ValueError):
        camera_fit.fisheye_lens_from_fit(ok, height=0, width=24)
    with pytest.raises(ValueError):   # k1 = -0.5 turns r(theta) back before 95 degrees: not a lens
        camera_fit.fisheye_lens_from_fit(dict(ok, pred_k1=-0.5), height=16, width=24, fov=190.0)


def test_names_resolve_from_the_three_packages_and_all_keeps_32_names():
    import perspective2d
    import perspectivefields_amd
    from perspectivefields_amd import camera_fit
    from perspectivefields_amd import perspectivefields as pfm

    assert len(perspectivefields_amd.__all__) == 32 and not set(NAMES) & set(perspectivefields_amd.__all__)
    for name in NAMES:
        assert perspectivefields_amd._HOME[name] == "camera_fit" and callable(getattr(perspectivefields_amd, name))
        assert getattr(perspective2d, name) is getattr(perspectivefields_amd, name) is getattr(pfm, name) is getattr(camera_fit, name)
    assert callable(pfm.PerspectiveFields.fit_fisheye)


@pytest.mark.parametrize("projection", KIND_NAMES)
def test_fisheye_lens_from_fit_of_a_hand_made_dict_is_fisheye_lens_of_the_same_lens(projection):
    from perspectivefields_amd import fisheye_lens, fisheye_lens_from_fit
    from perspectivefields_amd.gathers import _FISHEYE_RHO

    H, W, fov = 48, 64, 170.0
    roll, pitch, f, cx, cy, k1, k2 = TRUTHS[1][0]
    fit = dict(pred_roll=roll, pred_pitch=pitch, pred_rel_focal=f, pred_rel_cx=cx, pred_rel_cy=cy, pred_k1=k1, pred_k2=k2, fit_projection=projection, fit_max_fov=230.0)
    t = np.radians(fov / 2)
    radius = f * H * _FISHEYE_RHO[projection](t * (1 + t * t * (k1 + t * t * k2)))
    want = fisheye_lens(fov, radius=radius, center=((cx + 0.5) * W, (cy + 0.5) * H), projection=projection, k=(k1, k2, 0.0, 0.0), roll=roll, pitch=pitch, yaw=33.0, band=4.0)
    got = fisheye_lens_from_fit(fit, height=H, width=W, fov=fov, yaw=33.0, band=4.0)
    assert got.dtype == np.float64 and got.shape == (12,)
    assert np.allclose(got, want, rtol=1e-14, atol=0) and got[3] == f * H
    # tensors in the dict (one read), and the default fov is the fit's max_fov
    tfit = {k: (torch.tensor(v, dtype=torch.float32) if k.startswith("pred_") else v) for k, v in fit.items()}
    tfit["pred_k1"] = tfit["pred_k2"] = torch.tensor(0.0)
    row = fisheye_lens_from_fit(tfit, height=H, width=W)
    assert row[6] == np.radians(115.0) and row[3] == float(np.float32(f)) * H and row[2] == 0.0 and row[11] == 0.0


def test_new_kernels_are_in_the_library_without_scratch():
    """scripts/kernel_resources.py on the built library: every instance of the lens fit is there for gfx950 with no spilled register and no scratch"""
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
    for kind in KINDS:
        for poly, nps in (("false", (3, 5)), ("true", (5, 7))):
            fit = f"pf::FisheyeFit<{kind}, {poly}>"
            names = [f"pf::fit_init_kernel<{fit} >"] + [f"pf::fit_{k}_kernel<{fit}, {n}>" for k in ("accum", "solve") for n in nps]
            for name in names:
                assert name in by, (name, [k for k in by if "Fisheye" in k][:4])
                assert by[name]["spill"] == 0 and by[name]["scratch"] == 0, by[name]
        assert kr.blocks_per_cu(by[f"pf::fit_accum_kernel<pf::FisheyeFit<{kind}, true>, 7>"]) >= 2
