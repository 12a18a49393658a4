"""fp64 numpy statement of fisheye and dual-fisheye frames as a target (include/pf_hip.h pf_pano_to_fisheye / pf_fisheye_fields, DESIGN.md section
33), built on the lens model of tests/test_fisheye_ref.py: the inverse projection (owner, theta_d, the clamped Newton steps, the direction), the
image out of a panorama, the perspective fields of the fisheye camera; checks of that reference against itself and against the forward projection;
the same formulas in numpy float32 (the rounding floor the GPU results are measured against); which pixels are left out of the accuracy comparisons
and how few they are; the fixed inputs of tests/test_gpu_fisheye_target.py; plus the host-side contract of panorama_to_fisheye / fisheye_fields
and of the two C entry points (no GPU needed)."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest
import torch

from tests.test_cubemap_ref import block_mean
from tests.test_fisheye_ref import (CX, CY, EQUIDISTANT, EQUISOLID, FOCAL, K1, K2, K3, K4, OFF, RIGS, STEREOGRAPHIC, TMAX, YAW, distort, lens_project, lens_row,
                                    rho)
from tests.test_pano_crop_ref import bilinear, labels as usm_labels, rotation
from tests.test_pano_rotate_ref import _rot_matrix_f32, point_of, rot_matrix, up_angle_deg, wrap_px
from tests.test_reproject_ref import FakeCuda

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEWTON_STEPS = 10          # include/pf_hip.h PF_FISHEYE_NEWTON_STEPS
UP_MIN_T2 = 1e-10          # include/pf_hip.h PF_PANO_UP_MIN_T2
R2D = 180.0 / np.pi


# ---------------------------------------------------------------- the model, in fp64 by default and in numpy float32 with f=np.float32
def rho_inverse(kind, r, f=np.float64):
    return r if kind == EQUIDISTANT else f(2) * np.arcsin(np.minimum(r * f(0.5), f(1))) if kind == EQUISOLID else f(2) * np.arctan(r * f(0.5))


def rho_slope(kind, td, f=np.float64):
    if kind == EQUIDISTANT:
        return np.ones_like(td)
    c = np.cos(td * f(0.5))
    return c if kind == EQUISOLID else f(1) / (c * c)


def poly_slope(lens, t, f=np.float64):
    t2 = t * t
    return f(1) + t2 * (f(3) * lens[K1] + t2 * (f(5) * lens[K2] + t2 * (f(7) * lens[K3] + t2 * (f(9) * lens[K4]))))


def has_poly(lens):
    return bool((lens[K1:K4 + 1] != 0).any())


def lens_is_on(lens):
    return bool(np.isfinite(lens).all() and lens[TMAX] > 0)


def r_max(lens, kind):
    return lens[FOCAL] * rho(kind, distort(lens, lens[TMAX]))


def newton(lens, td, steps=NEWTON_STEPS, f=np.float64):
    """theta of theta_d: `steps` clamped Newton steps from min(theta_d, theta_max)"""
    t = np.minimum(td, lens[TMAX])
    with np.errstate(invalid="ignore", divide="ignore"):
        for _ in range(steps):
            t = np.clip(t - (distort(lens, t) - td) / poly_slope(lens, t, f), f(0), lens[TMAX])
    return t


def unproject(lenses, kind, a, b, f=np.float64):
    """image points (a, b), pixel-edge units -> dict of arrays: owner (-1: no lens owns the point), X (..., 3) in the owner's coordinates, cp, sp, t
    (theta), td (theta_d), r, rho.  Lens 0 first: the first owner wins"""
    a, b = np.asarray(a, dtype=f), np.asarray(b, dtype=f)
    out = dict(owner=np.full(a.shape, -1), X=np.full(a.shape + (3,), np.nan, f), **{k: np.full(a.shape, np.nan, f) for k in ("cp", "sp", "t", "td", "r", "rho")})
    for l, lens64 in enumerate(lenses):
        if not lens_is_on(np.asarray(lens64, dtype=f)):
            continue
        lens = np.asarray(lens64, dtype=f)
        dx, dy = a - lens[CX], b - lens[CY]
        r = np.sqrt(dx * dx + dy * dy)
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            own = (r_max(lens, kind) - r > 0) & (out["owner"] < 0)
            rh = r / lens[FOCAL]
            td = rho_inverse(kind, rh, f)
            t = newton(lens, td, f=f) if has_poly(lens) else td
            cp, sp = np.where(r > 0, dx / r, f(1)), np.where(r > 0, dy / r, f(0))
        X = np.stack([np.sin(t) * cp, np.sin(t) * sp, np.cos(t)], -1)
        assert X.dtype == f and td.dtype == f, (X.dtype, td.dtype)
        out["owner"] = np.where(own, l, out["owner"])
        out["X"] = np.where(own[..., None], X, out["X"])
        for k, v in (("cp", cp), ("sp", sp), ("t", t), ("td", td), ("r", r), ("rho", rh)):
            out[k] = np.where(own, v, out[k])
    return out


def lens_rotations(lens, f=np.float64):
    """(Q, R) of a lens row: lens -> world with and without the yaw"""
    if f is np.float32:
        L = np.asarray(lens, dtype=f)
        return _rot_matrix_f32(L[:3], False), _rot_matrix_f32((L[0], L[1], f(0)), False)
    return rot_matrix(lens[:3]), rotation(lens[0], lens[1])


def pixel_points(H, W, S=1):
    """the sub-sample points of an H x W frame, (S H, S W) each: (col + (j + 1/2) / S, row + (i + 1/2) / S)"""
    a = (np.arange(S * W) + 0.5) / S
    b = (np.arange(S * H) + 0.5) / S
    return a[None, :] + np.zeros((S * H, 1)), b[:, None] + np.zeros((1, S * W))


def pano_coords(lenses, kind, a, b, Hp, Wp, f=np.float64):
    """(u, v) in the Hp x Wp panorama of the points (a, b), NaN without an owner, and the inverse projection"""
    p = unproject(lenses, kind, a, b, f)
    u, v = np.full(p["owner"].shape, np.nan, f), np.full(p["owner"].shape, np.nan, f)
    for l, lens in enumerate(lenses):
        m = p["owner"] == l
        if not m.any():
            continue
        Q, _ = lens_rotations(lens, f)
        D = p["X"][m] @ Q.T
        if f is np.float32:
            nlat = np.arctan2(D[:, 1], np.sqrt(D[:, 0] * D[:, 0] + D[:, 2] * D[:, 2]))
            u[m] = (np.arctan2(D[:, 0], D[:, 2]) * f(1 / (2 * np.pi)) + f(0.5)) * f(Wp) - f(0.5)
            v[m] = (nlat * f(1 / np.pi) + f(0.5)) * f(Hp) - f(0.5)
        else:
            u[m], v[m], _ = point_of(D, Hp, Wp)
    assert u.dtype == f and v.dtype == f
    return u, v, p


def block_mean_fill(fine, valid, S, fill):
    n = valid.reshape(valid.shape[0] // S, S, valid.shape[1] // S, S).sum((1, 3))
    return np.where((n > 0)[..., None], block_mean(fine, valid, S), float(fill)), n > 0


def target_image(pano, lenses, kind, H, W, S=1, fill=0.0):
    """the frame in fp64 before any rounding, and its mask"""
    a, b = pixel_points(H, W, S)
    u, v, p = pano_coords(lenses, kind, a, b, pano.shape[0], pano.shape[1])
    valid = p["owner"] >= 0
    return block_mean_fill(bilinear(pano, u, v), valid, S, fill)


def target_fields(lenses, kind, H, W, f=np.float64):
    """the labels at the pixel centres: up (2, H, W) (NaN without an owner or where |t|^2 < PF_PANO_UP_MIN_T2), latitude (H, W) degrees (NaN without an
    owner), |t|^2 (H, W), owner (H, W)"""
    a, b = pixel_points(H, W)
    p = unproject(lenses, kind, a, b, f)
    up, lat, t2 = np.full((2, H, W), np.nan, f), np.full((H, W), np.nan, f), np.full((H, W), np.nan, f)
    for l, lens64 in enumerate(lenses):
        m = p["owner"] == l
        if not m.any():
            continue
        lens = np.asarray(lens64, dtype=f)
        _, R = lens_rotations(lens64, f)
        g = -R[1]   # R^T (0, -1, 0)
        X, cp, sp, t, td, r, rh = (p[k][m] for k in ("X", "cp", "sp", "t", "td", "r", "rho"))
        Xw = X @ R.T
        lat[m] = -np.arctan2(Xw[:, 1], np.sqrt(Xw[:, 0] * Xw[:, 0] + Xw[:, 2] * Xw[:, 2])) * f(R2D)
        st, ct = np.sin(t), np.cos(t)
        if f is np.float32:   # the kernel's order: g . e for t . e
            te = g[0] * (ct * cp) + g[1] * (ct * sp) + g[2] * -st
            tp = g[1] * cp - g[0] * sp
            tt = te * te + tp * tp
        else:                 # as the model states it
            tv = g - (X @ g)[:, None] * X
            te = (tv * np.stack([ct * cp, ct * sp, -st], -1)).sum(-1)
            tp = (tv * np.stack([-sp, cp, np.zeros_like(cp)], -1)).sum(-1)
            tt = (tv * tv).sum(-1)
        ms = rho_slope(kind, td, f) * (poly_slope(lens, t, f) if has_poly(lens) else f(1))
        with np.errstate(invalid="ignore", divide="ignore"):
            mt = np.where(r > 0, rh / st, ms)
            px, py = ms * te * cp - mt * tp * sp, ms * te * sp + mt * tp * cp
            n = np.sqrt(px * px + py * py)
            up[0][m] = np.where(tt >= f(UP_MIN_T2), px / n, f(np.nan))
            up[1][m] = np.where(tt >= f(UP_MIN_T2), py / n, f(np.nan))
        t2[m] = tt
    assert up.dtype == f and lat.dtype == f
    return up, lat, t2, p["owner"]


# ---------------------------------------------------------------- the fixed inputs of the GPU test, the pixels left out, the floors
# the rigs of tests/test_fisheye_ref.py as targets (the frame's size is the rig's), and the two thin frames
TARGETS = dict(RIGS)
TARGETS["1x17"] = ((1, 17), EQUISOLID, [lens_row(EQUISOLID, 5.0, 15.0, -60.0, 90.0, 0.0, (8.5, 0.5), radius=8.6), OFF])
TARGETS["19x1"] = ((19, 1), STEREOGRAPHIC, [lens_row(STEREOGRAPHIC, -8.0, -20.0, 110.0, 75.0, 0.0, (0.5, 9.5), radius=9.7), OFF])
TARGET_NAMES = tuple(TARGETS)
PANOS = [(32, 64), (2, 2)]
SS_TARGETS, SS_SAMPLES = ("A", "B"), (2, 3)
BORDER_PX, UP_T2_EXCLUDE = 1e-3, 1e-8


def target_lenses(name):
    return np.stack(TARGETS[name][2])


def scaled_lenses(name, S):
    """the lenses of the frame S times as large: F, Cx and Cy times S"""
    lenses = target_lenses(name).copy()
    lenses[:, [FOCAL, CX, CY]] *= S
    return lenses


@functools.lru_cache(None)
def target_case(name, pano_hw, S=1):
    """one frame (at S times its size: the fine frame of a supersampling comparison) out of one panorama size -> dict with
    kept      the pixels that are compared: all but those where fp64 and float32 disagree on the owner, or |r - r_max| < 1e-3 px for a lens that is on
    kept_up   kept, and |t|^2 >= 1e-8
    e_c       the float32 floor of the panorama coordinate in px (columns modulo the panorama's width) over the pixels with one owner in both
    owner, up, lat, t2   the fp64 reference;  up32, lat32   the numpy float32 evaluation;  read only"""
    (H, W), kind, _ = TARGETS[name]
    lenses = scaled_lenses(name, S)
    H, W = S * H, S * W
    a, b = pixel_points(H, W)
    u, v, p = pano_coords(lenses, kind, a, b, *pano_hw)
    u32, v32, p32 = pano_coords(lenses, kind, a, b, *pano_hw, f=np.float32)
    out = p["owner"] != p32["owner"]
    for lens in lenses:
        if lens_is_on(lens):
            out |= np.abs(np.hypot(a - lens[CX], b - lens[CY]) - r_max(lens, kind)) < BORDER_PX * S
    up, lat, t2, owner = target_fields(lenses, kind, H, W)
    up32, lat32, _, _ = target_fields(lenses, kind, H, W, f=np.float32)
    both = (p["owner"] >= 0) & ~out
    e_c = max(float(np.abs(wrap_px(u32 - u, pano_hw[1]))[both].max()), float(np.abs(v32 - v)[both].max())) if both.any() else 0.0
    with np.errstate(invalid="ignore"):
        kept_up = ~out & ~(t2 < UP_T2_EXCLUDE)
    return dict(kept=~out, kept_up=kept_up, e_c=e_c, owner=owner, up=up, lat=lat, t2=t2, up32=up32, lat32=lat32)


def label_floors(case):
    """the errors of the numpy float32 evaluation of a case against fp64: (up angle in degrees, latitude in degrees), over the kept pixels with an owner"""
    m = case["kept_up"] & (case["owner"] >= 0) & np.isfinite(case["up"][0]) & np.isfinite(case["up32"][0])
    e_up = float(up_angle_deg(case["up32"], case["up"])[m].max()) if m.any() else 0.0
    m = case["kept"] & (case["owner"] >= 0)
    e_lat = float(np.abs(case["lat32"] - case["lat"])[m].max()) if m.any() else 0.0
    return e_up, e_lat


def pano_gradient(pano):
    """the largest step between neighbouring texels of a panorama, along a column and along a row with the wrap: the largest derivative per px of
    its bilinear interpolant"""
    p = pano.astype(np.float64)
    steps = [np.abs(p - np.roll(p, 1, axis=1)).max()]
    if p.shape[0] > 1:
        steps.append(np.abs(np.diff(p, axis=0)).max())
    return float(max(steps))


def block_kept(kept, out, S):
    return kept.reshape(out[0], S, out[1], S).all((1, 3))


# ---------------------------------------------------------------- the reference against itself
def points_in_circle(lens, kind, n, seed, share=0.999):
    rng = np.random.default_rng(seed)
    ang, rad = rng.uniform(0, 2 * np.pi, n), share * r_max(lens, kind) * np.sqrt(rng.uniform(0, 1, n))
    return lens[CX] + rad * np.cos(ang), lens[CY] + rad * np.sin(ang)


@pytest.mark.parametrize("poly", [False, True])
@pytest.mark.parametrize("kind", [EQUIDISTANT, EQUISOLID, STEREOGRAPHIC])
def test_project_after_unproject_closes_with_exactly_10_clamped_steps(kind, poly):
    k = RIGS["C"][2][0][K1:K4 + 1] if poly else (0.0, 0.0, 0.0, 0.0)
    lens = lens_row(kind, 17.0, -33.0, 140.0, 80.0, 0.0, (31.7, 22.4), F=18.0, k=tuple(k))
    a, b = points_in_circle(lens, kind, 2000, kind)
    p = unproject([lens], kind, a, b)
    assert (p["owner"] == 0).all() and p["t"].max() <= lens[TMAX]
    th, a2, b2 = lens_project(lens, kind, p["X"] @ rot_matrix(lens[:3]).T)
    err = max(np.abs(a2 - a).max(), np.abs(b2 - b).max())
    print(f"kind {kind}, polynomial {poly}: project(unproject) closes to {err:.2e} px")
    assert err <= 1e-9 and np.abs(th - p["t"]).max() <= 1e-12
    if poly:   # the count matters: one step is not enough, ten are as good as sixty
        one = newton(lens, p["td"], steps=1)
        assert np.abs(one - p["t"]).max() > 1e-6 and np.abs(newton(lens, p["td"], steps=60) - p["t"]).max() <= 1e-14


def finite_difference_up(lens, kind, p, h=1e-6):
    """the image direction of a step along world up, from the forward projection: central difference of lens_project along +-h t"""
    Q = rot_matrix(lens[:3])
    D = p["X"] @ Q.T
    t = np.array([0.0, -1.0, 0.0]) - D[:, 1:2] * -1.0 * D   # world up minus its part along D: up - (up . D) D, up . D = -D.y
    Dp, Dm = D + h * t, D - h * t
    _, ap, bp = lens_project(lens, kind, Dp / np.linalg.norm(Dp, axis=-1, keepdims=True))
    _, am, bm = lens_project(lens, kind, Dm / np.linalg.norm(Dm, axis=-1, keepdims=True))
    d = np.stack([ap - am, bp - bm])
    return d / np.sqrt((d * d).sum(0)), (t * t).sum(-1)


@pytest.mark.parametrize("poly", [False, True])
@pytest.mark.parametrize("kind", [EQUIDISTANT, EQUISOLID, STEREOGRAPHIC])
def test_analytic_up_is_the_finite_difference_of_the_forward_projection(kind, poly):
    k = RIGS["C"][2][0][K1:K4 + 1] if poly else (0.0, 0.0, 0.0, 0.0)
    lens = lens_row(kind, 17.0, -33.0, 140.0, 80.0, 0.0, (31.5, 22.5), F=18.0, k=tuple(k))
    H, W = 45, 63   # the lens' axis is the centre of pixel (22, 31): r = 0 is among the points
    up, lat, t2, owner = target_fields([lens], kind, H, W)
    a, b = pixel_points(H, W)
    m = (owner == 0) & (np.hypot(a - lens[CX], b - lens[CY]) < 0.99 * r_max(lens, kind)) & (t2 > 1e-4)
    assert m.sum() > 500 and m[22, 31]
    p = unproject([lens], kind, a[m], b[m])
    fd, _ = finite_difference_up(lens, kind, p)
    err = up_angle_deg(up[:, m], fd).max()
    print(f"kind {kind}, polynomial {poly}: analytic up against the central difference {err:.2e} degrees over {int(m.sum())} pixels")
    assert err <= 1e-5
    Dw = p["X"] @ rot_matrix(lens[:3]).T   # the latitude is that of the world direction, with the yaw or without
    assert np.abs(lat[m] + np.degrees(np.arctan2(Dw[:, 1], np.hypot(Dw[:, 0], Dw[:, 2])))).max() <= 1e-11


def test_the_stereographic_lens_gives_the_usm_up_vectors_of_xi_1():
    """the stereographic lens of F is the Unified Spherical Model camera of xi = 1 and focal 2 F: pf_pano_crop's up label at the pixel centres"""
    H, W, F = 40, 56, 20.0
    lens = lens_row(STEREOGRAPHIC, 12.0, -25.0, 70.0, 100.0, 0.0, (0.5 * W + 3.0, 0.5 * H - 2.0), F=F)
    up, lat, t2, owner = target_fields([lens], STEREOGRAPHIC, H, W)
    assert (owner == 0).all()
    cam = (lens[0], lens[1], lens[2], 2 * F / H, 3.0 / W, -2.0 / H, 1.0)
    want, _ = usm_labels(cam, H, W)
    m = t2 > 1e-6
    err = up_angle_deg(up[:, m], want[:, m]).max()
    print(f"stereographic up against the USM formula at xi = 1: {err:.2e} degrees")
    assert m.mean() > 0.99 and err <= 1e-9


def test_latitude_and_up_do_not_depend_on_the_yaw():
    for name in ("A", "B", "C"):
        (H, W), kind, _ = TARGETS[name]
        lenses = target_lenses(name)
        turned = lenses.copy()
        turned[:, YAW] += np.array([1.234, -2.5])
        for f in (np.float64, np.float32):
            one, other = target_fields(lenses, kind, H, W, f=f), target_fields(turned, kind, H, W, f=f)
            assert all(np.array_equal(x, y, equal_nan=True) for x, y in zip(one, other))   # the same bits: the yaw is never read
        img = np.random.default_rng(0).uniform(0, 1, (8, 16, 3))
        assert np.abs(target_image(img, lenses, kind, H, W)[0] - target_image(img, turned, kind, H, W)[0]).max() > 0.1   # the image does turn


def test_the_first_owner_wins():
    """two lenses whose circles overlap: the overlap is lens 0's, with lens 0's image and labels"""
    first = lens_row(EQUIDISTANT, 3.0, 4.0, 10.0, 100.0, 0.0, (14.0, 12.0), radius=12.0)
    second = lens_row(EQUIDISTANT, -5.0, -4.0, 190.0, 100.0, 0.0, (30.0, 12.0), radius=12.0)
    H, W = 24, 44
    a, b = pixel_points(H, W)
    in0, in1 = np.hypot(a - 14.0, b - 12.0) < 12.0, np.hypot(a - 30.0, b - 12.0) < 12.0
    assert (in0 & in1).sum() > 20
    for lenses, overlap in (([first, second], 0), ([second, first], 1)):
        owner = unproject(lenses, EQUIDISTANT, a, b)["owner"]
        want = np.where(in0 if overlap == 0 else in1, 0, np.where(in1 if overlap == 0 else in0, 1, -1))
        assert np.array_equal(owner, want)
    pano = np.random.default_rng(1).uniform(0, 1, (16, 32, 3))
    both, mask = target_image(pano, [first, second], EQUIDISTANT, H, W)
    alone, mask0 = target_image(pano, [first, OFF], EQUIDISTANT, H, W)
    assert np.array_equal(both[in0], alone[in0]) and np.array_equal(mask0, in0) and np.array_equal(mask, in0 | in1)
    up, lat, _, _ = target_fields([first, second], EQUIDISTANT, H, W)
    up0, lat0, _, _ = target_fields([first, OFF], EQUIDISTANT, H, W)
    assert np.array_equal(up[:, in0], up0[:, in0], equal_nan=True) and np.array_equal(lat[in0], lat0[in0])


def test_an_off_or_non_finite_lens_owns_nothing():
    (H, W), kind, _ = TARGETS["B"]
    lenses = target_lenses("B")
    pano = np.random.default_rng(2).uniform(0, 1, (16, 32, 3))
    alone, mask0 = target_image(pano, [lenses[0], OFF], kind, H, W, fill=0.25)
    assert mask0.any() and not mask0.all() and (alone[~mask0] == 0.25).all()
    fields0 = target_fields([lenses[0], OFF], kind, H, W)
    assert np.isnan(fields0[0][:, ~mask0]).all() and np.isnan(fields0[1][~mask0]).all() and np.isfinite(fields0[1][mask0]).all()
    for k in range(12):
        for bad in (np.nan, np.inf, -np.inf):
            broken = lenses.copy()
            broken[1, k] = bad
            got, mask = target_image(pano, broken, kind, H, W, fill=0.25)
            assert np.array_equal(got, alone) and np.array_equal(mask, mask0), (k, bad)
            assert all(np.array_equal(x, y, equal_nan=True) for x, y in zip(target_fields(broken, kind, H, W), fields0))
    for tmax in (0.0, -1.0):
        broken = lenses.copy()
        broken[0, TMAX] = tmax
        assert not target_image(pano, [broken[0], OFF], kind, H, W)[1].any()


def test_supersampling_is_the_block_mean_of_the_valid_sub_samples():
    (H, W), kind, _ = TARGETS["A"]
    pano = np.random.default_rng(3).uniform(0, 1, (16, 32, 3))
    for S in SS_SAMPLES:
        fine, valid = target_image(pano, scaled_lenses("A", S), kind, S * H, S * W)
        coarse, any_valid = target_image(pano, target_lenses("A"), kind, H, W, S=S, fill=0.25)
        want, want_any = block_mean_fill(fine, valid, S, 0.25)
        partly = valid.reshape(H, S, W, S).sum((1, 3))
        assert ((partly > 0) & (partly < S * S)).any()   # the rim: pixels with some sub-samples outside the circle
        assert np.array_equal(any_valid, want_any) and np.abs(coarse - want).max() <= 1e-12 and (coarse[~any_valid] == 0.25).all()


# ---------------------------------------------------------------- the pixels left out and the float32 floors
def test_at_most_1_percent_of_any_case_is_left_out():
    """the condition of tests/test_gpu_fisheye_target.py, asserted for every one of its inputs on the reference alone"""
    worst = worst_up = 0.0
    for name in TARGET_NAMES:
        for pano_hw in PANOS:
            c = target_case(name, tuple(pano_hw))
            worst, worst_up = max(worst, 1.0 - c["kept"].mean()), max(worst_up, 1.0 - c["kept_up"].mean())
            assert 1.0 - c["kept"].mean() <= 0.01 and 1.0 - c["kept_up"].mean() <= 0.01, (name, pano_hw)
            assert (c["owner"] >= 0).any(), name
    for name in SS_TARGETS:
        for S in SS_SAMPLES:
            left = 1.0 - block_kept(target_case(name, tuple(PANOS[0]), S)["kept"], TARGETS[name][0], S).mean()
            worst = max(worst, left)
            assert left <= 0.01, (name, S, left)
    print(f"at most {100 * worst:.3f} % of a case left out of the image and latitude comparisons, {100 * worst_up:.3f} % of the up comparison")


def test_fp32_floor_of_the_fixed_cases():
    """the float32 evaluation of the model is a few ulp of a panorama coordinate of tens of px, and of angles of tens of degrees"""
    for name in TARGET_NAMES:
        c = target_case(name, tuple(PANOS[0]))
        e_up, e_lat = label_floors(c)
        print(f"target {name}: float32 floor of the panorama coordinate {c['e_c']:.3e} px, of the up angle {e_up:.3e} degrees, of the latitude {e_lat:.3e} degrees")
        assert c["e_c"] <= 2e-4 and e_up <= 1e-2 and e_lat <= 1e-4


# ---------------------------------------------------------------- host-side contract (fails before the feature exists)
NAMES = ("panorama_to_fisheye", "fisheye_fields")
ENTRY_POINTS = ("pf_pano_to_fisheye", "pf_fisheye_fields")


def test_names_are_exported_from_both_packages():
    import perspective2d
    import perspectivefields_amd

    from perspectivefields_amd import gathers, perspectivefields as pfm

    for name in NAMES:
        assert perspectivefields_amd._HOME[name] == "gathers" and callable(getattr(perspectivefields_amd, name))
        assert getattr(perspective2d, name) is getattr(perspectivefields_amd, name) is getattr(pfm, name) is getattr(gathers, name)
    from perspectivefields_amd import fisheye_fields, panorama_to_fisheye  # noqa: F401


def test_header_states_the_model_and_the_newton_steps():
    hdr = open(os.path.join(ROOT, "include", "pf_hip.h")).read()
    assert "int pf_pano_to_fisheye(int device, int n_pano, const void* const* h_pano, const int32_t* h_pano_hw" in hdr
    assert "int pf_fisheye_fields(int device, int kind, int batch, const float* d_lens" in hdr
    assert re.search(r"#define PF_FISHEYE_NEWTON_STEPS\s+%d\b" % NEWTON_STEPS, hdr)
    assert re.search(r"#define PF_PANO_UP_MIN_T2\s+1e-10f", hdr)
    for text in ("r_max - r > 0", "The first owner wins", "theta_0 = min(theta_d, theta_max)", "2 asin(min(rho / 2, 1))", "2 atan(rho / 2)",
                 "P'(t) = 1 + t^2 (3 k1 + t^2 (5 k2 + t^2 (7 k3 + 9 k4 t^2)))", "g = R^T (0, -1, 0)", "rho' = 1 | cos(theta_d / 2) | 1 / cos^2(theta_d / 2)",
                 "at r = 0, m / sin theta is replaced by m'"):
        assert text in hdr, text
    kh = open(os.path.join(ROOT, "perspectivefields_amd", "csrc", "pf_kernels.h")).read()
    assert "struct PanoToFisheyeBatch" in kh and "struct FisheyeFieldsBatch" in kh and "offsetof(PanoToFisheyeBatch, src) == 32" in kh
    from perspectivefields_amd import build as _b

    assert "fisheye_target.hip" in _b.SOURCES and _b.EXTRA_FLAGS["fisheye_target.hip"] == _b.NO_PK_F32_FLAGS
    src = open(os.path.join(ROOT, "perspectivefields_amd", "csrc", "fisheye_target.hip")).read()
    assert "#pragma clang fp contract(off)" in src and '#include "fisheye_model.h"' in src


def test_symbols_and_prototypes_are_present():
    from perspectivefields_amd.engine import _SIGNATURES, declared_symbols, load_library

    assert all(name in declared_symbols() for name in ENTRY_POINTS)
    res, args = _SIGNATURES["pf_pano_to_fisheye"]
    assert res is ctypes.c_int and len(args) == 18 and args[5] is ctypes.c_int and args[11] is ctypes.c_float and args[16] is ctypes.c_int
    res, args = _SIGNATURES["pf_fisheye_fields"]
    assert res is ctypes.c_int and len(args) == 9 and args[1] is ctypes.c_int and args[3] is ctypes.c_void_p
    lib = load_library()
    assert all(hasattr(lib, name) for name in ENTRY_POINTS)


def test_pf_pano_to_fisheye_rejects_bad_arguments_before_device_work():
    from perspectivefields_amd.engine import load_library

    lib = load_library()
    name = "pf_pano_to_fisheye"
    pano = (ctypes.c_void_p * 1)(0x1000)
    ints = lambda *s: (ctypes.c_int32 * len(s))(*s)
    dev = ctypes.c_void_p(256)

    def call(hw=None, dtype=0, kind=0, idx=(0,), c_idx=True, H=4, W=8, img=dev, lens=dev, n=1, p=pano, B=None, samples=1, up=None, lat=None):
        rc = lib.pf_pano_to_fisheye(0, n, p, hw or ints(8, 16), dtype, kind, len(idx) if B is None else B, ints(*idx) if c_idx else None, lens, H, W, 0.0, img, None,
                                    up, lat, samples, None)
        return rc, lib.pf_last_error(None).decode()

    # the stated order: samples, then kind, then gather_run's checks; each later error is given together with every earlier-checked argument right
    for kw, what in ((dict(samples=0, kind=3, lens=None), "samples"), (dict(samples=5, kind=-1, hw=ints(1, 8)), "samples"), (dict(kind=3, lens=None), "kind"),
                     (dict(kind=-1, hw=ints(8, 1), idx=(1,)), "kind"), (dict(lens=None), "required"), (dict(hw=ints(1, 8)), "smaller"), (dict(hw=ints(8, 1)), "smaller"),
                     (dict(hw=ints(1, 8), lens=None), "smaller"), (dict(lens=None, up=dev), "required"), (dict(up=dev), "both"), (dict(lat=dev), "both"),
                     (dict(up=dev, idx=(1,)), "both"), (dict(idx=(1,)), "index"), (dict(idx=(-1,)), "index"), (dict(H=0), "size"), (dict(W=0), "size"),
                     (dict(dtype=2), "dtype"), (dict(img=None), "required"), (dict(c_idx=False), "required"), (dict(B=0), "required"),
                     (dict(p=(ctypes.c_void_p * 1)()), "NULL"), (dict(p=None), "at least one"), (dict(n=0), "at least one")):
        rc, msg = call(**kw)
        assert rc == -1 and what in msg and msg.startswith(name + ": "), (kw, rc, msg)
    if not torch.cuda.is_available():   # a 2 x 2 panorama, a 1 x 1 frame, labels and every kind are good arguments: they fail on the missing device only
        for kind in (EQUIDISTANT, EQUISOLID, STEREOGRAPHIC):
            rc, msg = call(kind=kind, hw=ints(2, 2), H=1, W=1, up=dev, lat=dev, samples=4)
            assert rc == -2 and "no HIP device" in msg, (rc, msg)


def test_pf_fisheye_fields_rejects_bad_arguments_before_device_work():
    from perspectivefields_amd.engine import load_library

    lib = load_library()
    dev = ctypes.c_void_p(256)

    def call(kind=0, B=1, lens=dev, H=4, W=8, up=dev, lat=dev):
        rc = lib.pf_fisheye_fields(0, kind, B, lens, H, W, up, lat, None)
        return rc, lib.pf_last_error(None).decode()

    for kw, what in ((dict(kind=3, lens=None), "kind"), (dict(kind=-1, H=0), "kind"), (dict(B=0), "required"), (dict(lens=None), "required"), (dict(up=None), "required"),
                     (dict(lat=None), "required"), (dict(H=0), "size"), (dict(W=0), "size")):
        rc, msg = call(**kw)
        assert rc == -1 and what in msg and msg.startswith("pf_fisheye_fields: "), (kw, rc, msg)
    if not torch.cuda.is_available():
        rc, msg = call(kind=STEREOGRAPHIC, H=1, W=1)
        assert rc == -2 and "no HIP device" in msg, (rc, msg)


def test_fisheye_target_functions_on_cpu_tensors_raise():
    from perspectivefields_amd import fisheye_fields, panorama_to_fisheye
    from perspectivefields_amd.engine import PfError

    pano = torch.zeros((8, 16, 3), dtype=torch.uint8)
    with pytest.raises(PfError):
        panorama_to_fisheye(pano, target_lenses("B"), height=24, width=48)
    with pytest.raises(PfError):
        panorama_to_fisheye([pano], target_lenses("A")[0], height=4, width=8, fields=True)
    with pytest.raises(PfError):
        fisheye_fields(target_lenses("A")[0], height=4, width=8, device="cpu")


def test_python_argument_errors_before_the_library_is_loaded(monkeypatch):
    from perspectivefields_amd import engine
    from perspectivefields_amd import perspectivefields as pfm

    def no_library(*a, **k):
        raise AssertionError("the library was loaded before the arguments were checked")

    monkeypatch.setattr(engine, "load_library", no_library)
    monkeypatch.setattr(pfm.torch, "is_tensor", lambda v: isinstance(v, (torch.Tensor, FakeCuda)))
    ok = FakeCuda((8, 16, 3))
    row = target_lenses("A")[0]
    bad_panos = [FakeCuda((8, 16, 4)), FakeCuda((8, 16)), FakeCuda((1, 16, 3)), FakeCuda((8, 1, 3)), FakeCuda((8, 16, 3), torch.float16),
                 [ok, FakeCuda((8, 16, 3), torch.float32)], []]
    bad_lenses = [np.zeros(11), np.zeros((3, 12)), np.zeros((2, 13)), np.zeros((2, 3, 12))]
    for kw in ([dict(samples=0), dict(samples=5), dict(samples=2.0), dict(pano_index=[1]), dict(pano_index=[-1]), dict(pano_index=[]), dict(height=0), dict(width=0),
                dict(projection="orthographic"), dict(pano=[ok, ok], lenses=np.zeros((3, 2, 12))), dict(pano_index=[0, 0], lenses=np.zeros((3, 2, 12)))]
               + [dict(pano=p) for p in bad_panos] + [dict(lenses=l) for l in bad_lenses]):
        args = dict(pano=ok, lenses=row, height=4, width=8)
        args.update(kw)
        with pytest.raises(ValueError):
            pfm.panorama_to_fisheye(args.pop("pano"), args.pop("lenses"), **args)
    with pytest.raises(TypeError):
        pfm.panorama_to_fisheye([ok, np.zeros((8, 16, 3))], row, height=4, width=4)
    with pytest.raises(TypeError):
        pfm.panorama_to_fisheye(ok, row)   # height and width are required
    for kw in [dict(height=0), dict(width=0), dict(projection="orthographic")] + [dict(lenses=l) for l in bad_lenses + [[]]]:
        args = dict(lenses=row, height=4, width=8)
        args.update(kw)
        with pytest.raises(ValueError):
            pfm.fisheye_fields(args.pop("lenses"), **args)
    with pytest.raises(TypeError):
        pfm.fisheye_fields(row)


def test_fisheye_target_kernels_are_in_the_library_without_scratch():
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
    names = [f"pf::pano_to_fisheye_kernel<{t}, {l}>" for t in ("unsigned char", "float") for l in ("true", "false")] + ["pf::fisheye_fields_kernel"]
    for name in names:
        r = by[name]
        assert r["spill"] == 0 and r["scratch"] == 0 and r["lds"] <= 512 and r["vgpr"] <= 128, r
