"""Similarity transforms of perspective fields and the placement search (include/pf_hip.h pf_fields_transform, pf_place_search;
perspectivefields_amd.transform_fields, placement_search): the fp64 reference the GPU tests compare against, the fixed inputs, and the host-side
contract.  No GPU here.

Model of the transform, in fp64 on the fp32 inputs.  Source (h, w), variant (s, phi in degrees), output (h', w') with
h' = max(1, floor(s (h |cos phi| + w |sin phi|) + 1/2)) and w' likewise with h and w exchanged, unless given.  cos and sin come from
remainder(phi, 360) and are exactly 0 or +-1 at the multiples of 90.  Output pixel (r', c'): d = (c' + 1/2 - w'/2, r' + 1/2 - h'/2), source position
(x, y) = (w/2, h/2) + R(-phi) d / s - (1/2, 1/2) in pixel-centre coordinates, R(phi) = [[cos, -sin], [sin, cos]] (x right, y down).  Four bilinear
taps at floor(x), floor(y) and their + 1 neighbours; a tap counts when it is inside the array and valid by the rule of tests/test_placement_ref.py.
W_v = the weights of the taps that count.  The pixel is valid iff W_v >= 1/2 and the mix m = sum w_k u_k, rounded to fp32, passes the length rule.
lat' = sum w_k lat_k / W_v; up' = R(phi) m scaled to unit length, and left as it is where its squared length is within 2^-22 of 1 already (a vector
that is of unit length in fp32 keeps its bits).  Invalid pixels are NaN in all three planes.
The search: every variant's transformed object, rounded to fp32, scored by tests/test_placement_ref.py's reference at every offset; min_valid counts
against the valid pixels of the transformed object; a variant that does not fit is +inf with offset (-1, -1); the best is the first minimum in
variant order, then in row-major order.

What the device may differ by (the GPU tests' tolerances).  u = 2^-24.  The device computes the source position in fp32:
d is exact; p_x = fma(c, d_x, rnd(s d_y)) with c, s rounded from fp64 has an error of at most 3 u (|d_x| + |d_y|); x = fma(p_x, rnd(1/s), w/2 - 1/2)
adds u |p_x| / s and one rounding u |x|: E = u (4 (|d_x| + |d_y|) / s + max(|x|, |y|, 1)) bounds the error of either coordinate.  The weights'
x-derivatives sum to 2 in absolute value, so do the y-derivatives, and a weight is a rounded product of rounded factors: the weights move by at most
D = 4 E + 3 u in total.  A weighted mean moves by at most D x (largest difference among the pixel's taps) / W_v.  The values are fp64 on the device
and rounded once: u |lat'| for the latitude; for the up vector a rotation by fp32 cos and sin (sqrt(2) u) and one rounding per component, 4 u in
all, and the mix's direction moves by D x (largest distance among the taps' vectors) / |m|.
A pixel with |W_v - 1/2| < 1e-3 is BORDERLINE: its validity may differ on the device, and the GPU tests leave it out."""
import ctypes
import functools
import math
import os

import numpy as np
import pytest
import torch

from oracle.pf_oracle import fields_from_params
from tests.test_placement_ref import BG_CAM, OTHER_CAM, PLANT, camera_fields, crop, ellipse, field_valid, reference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24
BORDER = 1e-3
UP_TOL, LAT_TOL, CHUNK = 2e-4, 1.1e-5, 1024   # the per-pair bounds of DESIGN.md section 21 and PlaceBatch::CHUNK


# ---------------------------------------------------------------- the reference
def trig(rot_deg):
    """(cos, sin) of a rotation in degrees, exact at the multiples of 90"""
    a = math.remainder(rot_deg, 360.0)
    q = a / 90.0
    if q == math.floor(q):
        return ((-1.0, 0.0), (0.0, -1.0), (1.0, 0.0), (0.0, 1.0), (-1.0, 0.0))[int(q) + 2]
    rad = a * (math.pi / 180.0)
    return math.cos(rad), math.sin(rad)


def out_size(h, w, scale, rot_deg):
    c, s = trig(rot_deg)
    return (max(1, int(math.floor(scale * (h * abs(c) + w * abs(s)) + 0.5))), max(1, int(math.floor(scale * (w * abs(c) + h * abs(s)) + 0.5))))


def ref_transform(up, lat, scale=1.0, rot_deg=0.0, height=None, width=None):
    """dict: up (2,h',w'), lat (h',w') float64 with NaN where invalid; valid; W_v; full (all four taps count); borderline; tol_up (per component of the
    unit vector), tol_lat (degrees): what the device may differ by"""
    up, lat = np.asarray(up), np.asarray(lat)
    u, l = up.astype(np.float64), lat.astype(np.float64)
    src_valid = field_valid(up, lat)
    h, w = l.shape
    ho, wo = out_size(h, w, scale, rot_deg)
    ho, wo = (ho if height is None else height), (wo if width is None else width)
    c, s = trig(rot_deg)
    dx, dy = np.meshgrid(np.arange(wo) + 0.5 - wo / 2, np.arange(ho) + 0.5 - ho / 2)
    x, y = w / 2 + (c * dx + s * dy) / scale - 0.5, h / 2 + (c * dy - s * dx) / scale - 0.5
    x0, y0 = np.floor(x), np.floor(y)
    ax, ay = x - x0, y - y0
    Wv, mx, my, ml = (np.zeros((ho, wo)) for _ in range(4))
    taps, cnt = [], np.zeros((ho, wo), dtype=int)
    for ty in (0, 1):
        for tx in (0, 1):
            xi, yi = (x0 + tx).astype(np.int64), (y0 + ty).astype(np.int64)
            inside = (xi >= 0) & (xi < w) & (yi >= 0) & (yi < h)
            xc, yc = np.clip(xi, 0, w - 1), np.clip(yi, 0, h - 1)
            v = inside & src_valid[yc, xc]
            wk = np.where(v, (ay if ty else 1 - ay) * (ax if tx else 1 - ax), 0.0)
            tu = np.where(v, u[:, yc, xc], 0.0)
            tl = np.where(v, l[yc, xc], 0.0)
            Wv, mx, my, ml = Wv + wk, mx + wk * tu[0], my + wk * tu[1], ml + wk * tl
            cnt += v
            taps.append((v, np.where(v, u[:, yc, xc], np.nan), np.where(v, l[yc, xc], np.nan)))
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        mxf, myf = mx.astype(np.float32), my.astype(np.float32)
        m2 = mxf * mxf + myf * myf
        valid = (Wv >= 0.5) & (m2 >= np.float32(1e-12)) & np.isfinite(m2)
        rx, ry = c * mx - s * my, s * mx + c * my
        l2 = rx * rx + ry * ry
        k = np.where(np.abs(l2 - 1.0) <= 2.0 ** -22, 1.0, 1.0 / np.sqrt(l2))
        o_up = np.where(valid, np.stack([rx * k, ry * k]), np.nan)
        o_lat = np.where(valid, ml / Wv, np.nan)
        # the largest differences among the taps that count
        d_up, d_lat = np.zeros((ho, wo)), np.zeros((ho, wo))
        for i in range(4):
            for j in range(i):
                both = taps[i][0] & taps[j][0]
                d_up = np.maximum(d_up, np.where(both, np.hypot(*(taps[i][1] - taps[j][1])), 0.0))
                d_lat = np.maximum(d_lat, np.where(both, np.abs(taps[i][2] - taps[j][2]), 0.0))
        E = U * (4 * (np.abs(dx) + np.abs(dy)) / scale + np.maximum(np.maximum(np.abs(x), np.abs(y)), 1.0))
        D = 4 * E + 3 * U
        tol_up = np.where(valid, D * d_up / np.sqrt(mx * mx + my * my) + 4 * U, 0.0)
        tol_lat = np.where(valid, D * d_lat / Wv + U * np.abs(o_lat), 0.0)
    return dict(up=o_up, lat=o_lat, valid=valid, W_v=Wv, full=cnt == 4, borderline=np.abs(Wv - 0.5) < BORDER, tol_up=tol_up, tol_lat=tol_lat)


def as_f32(t):
    """the transformed fields in the device's format"""
    return np.ascontiguousarray(t["up"].astype(np.float32)), np.ascontiguousarray(t["lat"].astype(np.float32))


def variant_list(scales, rotations):
    return [(s, r) for s in scales for r in rotations]


def _borderline_allowance(up_bg, lat_bg, tu, tl, t, d, stride, weights):
    """what the best PFD of a variant may move by when its borderline pixels change sides on the device: a pixel that is valid here and has the
    weighted error e moves the mean over n pairs by |e - mean| / (n - 1) when it leaves; one that is invalid here has no value to go by and may
    bring any error up to 180 + 180 degrees"""
    k_all = int(t["borderline"].sum())
    if k_all == 0 or not np.isfinite(d["best_pfd_deg"]):
        return 0.0
    j, i = d["best_offset"]
    n = int(d["valid_pixels"][j // stride, i // stride])
    ub, lb = np.asarray(up_bg, dtype=np.float64), np.asarray(lat_bg, dtype=np.float64)
    total = 0.0
    for r, c in zip(*np.nonzero(t["borderline"])):
        if t["valid"][r, c]:
            a, b = ub[:, j + r, i + c], tu[:, r, c].astype(np.float64)
            e = weights[0] * np.degrees(np.arctan2(abs(a[0] * b[1] - a[1] * b[0]), a[0] * b[0] + a[1] * b[1])) + weights[1] * abs(lb[j + r, i + c] - float(tl[r, c]))
            total += abs(e - d["best_pfd_deg"]) if np.isfinite(e) else 0.0
        else:
            total += 180.0 * (weights[0] + weights[1])
    return total / max(n - k_all, 1)


def ref_search(up_bg, lat_bg, up_obj, lat_obj, variants, stride=1, min_valid=0.5, weights=(1.0, 1.0)):
    """dict: per variant `maps` (the reference dict of tests/test_placement_ref.py or None), `size`, `valid_pixels`, `pfd`, `offset`, `bound` (what
    the device's best PFD of the variant may differ by); best_variant, best_offset, best_pfd_deg"""
    H, W = np.asarray(lat_bg).shape
    out = dict(maps=[], size=[], valid_pixels=[], pfd=[], offset=[], bound=[], transform=[])
    for s, r in variants:
        t = ref_transform(up_obj, lat_obj, s, r)
        tu, tl = as_f32(t)
        h, w = tl.shape
        out["transform"].append(t)
        out["size"].append((h, w))
        out["valid_pixels"].append(int(field_valid(tu, tl).sum()))
        if h > H or w > W:
            out["maps"].append(None)
            out["pfd"].append(np.inf)
            out["offset"].append((-1, -1))
            out["bound"].append(0.0)
            continue
        d = reference(up_bg, lat_bg, tu, tl, stride, min_valid=min_valid, weights=weights)
        out["maps"].append(d)
        out["pfd"].append(float(d["best_pfd_deg"]))
        out["offset"].append(tuple(d["best_offset"]))
        # section 21's bound of the two means, plus the transform's: an object pixel off by t moves its pair's error by at most t
        T = min(CHUNK, h * w)
        fin = np.isfinite(d["pfd_deg"])
        mean = (weights[0] * (UP_TOL + (T + 8) * U * np.nanmax(np.where(fin, d["up_mean_deg"], np.nan))) +
                weights[1] * (LAT_TOL + (T + 8) * U * np.nanmax(np.where(fin, d["lat_mean_deg"], np.nan)))) if fin.any() else 0.0
        out["bound"].append(float(mean + weights[0] * np.degrees(math.sqrt(2.0) * t["tol_up"].max()) + weights[1] * t["tol_lat"].max()) +
                            _borderline_allowance(up_bg, lat_bg, tu, tl, t, d, stride, weights))
    k = int(np.argmin(out["pfd"]))   # the first minimum
    found = np.isfinite(out["pfd"][k])
    out.update(best_variant=k if found else -1, best_offset=out["offset"][k] if found else (-1, -1), best_pfd_deg=out["pfd"][k])
    return out


# ---------------------------------------------------------------- fixed inputs (shared with tests/test_gpu_placement_search.py)
PLANT_AT = (14, 25, 15, 12)   # row, col, h, w of the patch in the 48 x 64 background
PLANT_SCALES, PLANT_ROTATIONS = (0.75, 1.0, 1.5), (-10.0, 0.0, 10.0)


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(None)
def planted_search():
    """(up_bg, lat_bg, [(up_obj, lat_obj, variant that undoes it, size of that variant)] x 2)"""
    up, lat = camera_fields(*BG_CAM, 48, 64)
    patch = crop(up, lat, *PLANT_AT)
    objs = []
    for s, r in ((1 / 1.5, -10.0), (1 / 0.75, 10.0)):
        objs.append(_frozen(*as_f32(ref_transform(*patch, s, r))))
    return _frozen(up, lat) + (objs,)


@functools.lru_cache(None)
def search_set(name):
    """(backgrounds [(up, lat)], objects [(up, lat)], pairs, scales, rotations, stride) of the noisy sets G, H, I"""
    if name == "G":
        bgs = [camera_fields(*BG_CAM, 40, 56, seed=1)]
        objs = [crop(*camera_fields(*BG_CAM, 40, 56, seed=2), *PLANT)]
        pairs, scales, rots = [(0, 0)], (0.75, 1.0, 1.5), (-10.0, 10.0)
    elif name == "H":
        bgs = [camera_fields(*BG_CAM, 40, 42, seed=5)]
        obj = crop(*camera_fields(*BG_CAM, 40, 42, seed=6), 4, 3, 33, 35)
        obj[1][~ellipse(33, 35)] = np.nan
        objs, pairs, scales, rots = [obj], [(0, 0)], (0.5, 1.0, 1.25), (-10.0, 10.0)
    elif name == "I":
        bgs = [camera_fields(*BG_CAM, 40, 56, seed=1), camera_fields(*BG_CAM, 37, 53, seed=3)]
        other = crop(*camera_fields(*OTHER_CAM, 20, 33, seed=4), 3, 5, 11, 10)
        other[1][~ellipse(11, 10)] = np.nan
        objs = [crop(*camera_fields(*BG_CAM, 40, 56, seed=2), *PLANT), other]
        pairs, scales, rots = [(0, 0), (1, 1), (0, 1)], (0.75, 1.5), (-10.0, 10.0)
    else:
        raise KeyError(name)
    for f in bgs + objs:
        _frozen(*f)
    return bgs, objs, pairs, scales, rots, 1


@functools.lru_cache(None)
def set_search_reference(name):
    bgs, objs, pairs, scales, rots, stride = search_set(name)
    return [ref_search(*bgs[b], *objs[o], variant_list(scales, rots), stride) for b, o in pairs]


def transform_cases():
    """(name, up, lat, scale, rotation) of every fixed variant: the objects of the planted search and of G, H, I under their searches' variants"""
    cases = []
    _, _, objs = planted_search()
    for i, (u, l) in enumerate(objs):
        cases += [(f"planted{i}", u, l, s, r) for s, r in variant_list(PLANT_SCALES, PLANT_ROTATIONS)]
    for name in "GHI":
        _, objs, _, scales, rots, _ = search_set(name)
        for i, (u, l) in enumerate(objs):
            cases += [(f"{name}{i}", u, l, s, r) for s, r in variant_list(scales, rots)]
    return cases


# ---------------------------------------------------------------- rotation is roll
def _roll_fields(roll, n=48):
    up, lat, _ = fields_from_params(roll, 20.0, 60.0, 0.0, 0.0, n, n)
    return np.ascontiguousarray(np.moveaxis(up, -1, 0)), lat


def _angle(a, b):
    return np.degrees(np.arctan2(np.abs(a[0] * b[1] - a[1] * b[0]), a[0] * b[0] + a[1] * b[1]))


def test_a_quarter_turn_is_a_roll_of_minus_ninety():
    up, lat = _roll_fields(8.0)
    t = ref_transform(up, lat, 1.0, 90.0, height=48, width=48)
    want_up, want_lat = _roll_fields(-82.0)
    assert t["valid"].all()   # every position is a pixel centre: one tap carries the weight
    e_up, e_lat = _angle(t["up"], want_up).max(), np.abs(t["lat"] - want_lat).max()
    print(f"quarter turn against roll -82: up {e_up:.1e} deg, latitude {e_lat:.1e} deg")
    assert e_up <= 1e-12 and e_lat <= 1e-12


@pytest.mark.parametrize("phi, roll", [(15.0, -7.0), (-30.0, 38.0)])
def test_a_rotation_is_a_roll_of_the_other_sign(phi, roll):
    """On a square array the oracle's latitude grid (end points included) is the pixel-centre grid stretched about the centre by the same factor in x
    and y, which commutes with the rotation: the transformed map is the map of the other roll on the same grid.  Bilinear interpolation on a unit
    grid errs by at most (max |f_xx| + max |f_yy|) / 8; the second differences of the target field stand for the derivatives, with a margin of 2."""
    up, lat = _roll_fields(8.0)
    t = ref_transform(up, lat, 1.0, phi, height=48, width=48)
    want_up, want_lat = _roll_fields(roll)
    full = t["full"]
    assert full.sum() > 0.6 * 48 * 48 and t["valid"][full].all()
    d2 = lambda f: np.abs(np.diff(f, 2, axis=-1)).max() + np.abs(np.diff(f, 2, axis=-2)).max()
    b_lat = 2.0 * d2(want_lat) / 8
    b_up = np.degrees(2.0 * math.sqrt(2.0) * max(d2(want_up[0]), d2(want_up[1])) / 8)
    e_up, e_lat = _angle(t["up"], want_up)[full].max(), np.abs(t["lat"] - want_lat)[full].max()
    print(f"phi {phi}: up {e_up:.2e} deg of {b_up:.2e}, latitude {e_lat:.2e} deg of {b_lat:.2e}; partially covered pixels "
          f"{_angle(t['up'], want_up)[t['valid'] & ~full].max():.3f} deg")
    assert e_up <= b_up and e_lat <= b_lat
    wrong = _roll_fields(8.0 + phi)[0]
    assert _angle(t["up"], wrong)[full].min() > 10.0


# ---------------------------------------------------------------- identity and exact cases
def _noisy(h=9, w=7, seed=11):
    up, lat = crop(*camera_fields(*BG_CAM, 40, 56, seed=seed), 5, 6, h, w)
    lat[1, 2] = np.nan
    up[:, 3, 3] = 0.0
    return up, lat


def test_identity_returns_the_bits():
    up, lat = _noisy()
    t = ref_transform(up, lat)
    tu, tl = as_f32(t)
    keep = field_valid(up, lat)
    assert np.array_equal(t["valid"], keep)
    assert np.array_equal(tu[:, keep].view(np.uint32), up[:, keep].view(np.uint32)) and np.array_equal(tl[keep].view(np.uint32), lat[keep].view(np.uint32))
    assert np.isnan(tu[:, ~keep]).all() and np.isnan(tl[~keep]).all()


def test_two_half_turns_are_the_input():
    up, lat = _noisy()
    once = as_f32(ref_transform(up, lat, 1.0, 180.0))
    keep = field_valid(up, lat)
    assert np.array_equal(once[0][:, keep[::-1, ::-1]], -up[:, ::-1, ::-1][:, keep[::-1, ::-1]]) and np.array_equal(np.isnan(once[1]), ~keep[::-1, ::-1])
    twice = as_f32(ref_transform(*once, 1.0, 180.0))
    assert np.array_equal(twice[0][:, keep], up[:, keep]) and np.array_equal(twice[1][keep], lat[keep]) and np.isnan(twice[1][~keep]).all()


def test_constant_one_pixel_and_empty_fields():
    up = np.broadcast_to(np.array([0.6, -0.8], dtype=np.float32)[:, None, None], (2, 5, 4)).copy()
    lat = np.full((5, 4), 12.5, dtype=np.float32)
    t = ref_transform(up, lat, 2.0, 0.0)
    assert t["lat"].shape == (10, 8) and t["valid"].all() and (t["lat"] == 12.5).all()
    assert np.abs(t["up"][0] - 0.6).max() < 1e-7 and np.abs(t["up"][1] + 0.8).max() < 1e-7
    one = ref_transform(up[:, :1, :1], lat[:1, :1], 3.0, 45.0)
    assert one["lat"].shape == (4, 4)
    inner = one["valid"]
    assert inner.any() and np.abs(one["lat"][inner] - 12.5).max() < 1e-12
    a = math.sqrt(0.5)
    assert np.abs(one["up"][0][inner] - (a * 0.6 + a * 0.8)).max() < 1e-7 and np.abs(one["up"][1][inner] - (a * 0.6 - a * 0.8)).max() < 1e-7
    empty = ref_transform(up, np.full_like(lat, np.nan), 1.5, 10.0)
    assert not empty["valid"].any() and np.isnan(empty["up"]).all() and np.isnan(empty["lat"]).all()


# ---------------------------------------------------------------- the mask rule
def test_half_pixel_shift_of_a_checkerboard_by_hand():
    """width = w + 1 at s = 1 puts every output column half-way between two source columns: the weights are (1/2, 1/2) across and (1, 0) down"""
    h, w = 4, 6
    up = np.zeros((2, h, w), dtype=np.float32)
    up[1] = -1.0
    lat = np.arange(h * w, dtype=np.float32).reshape(h, w)
    r, c = np.mgrid[0:h, 0:w]
    lat[(r + c) % 2 == 1] = np.nan
    t = ref_transform(up, lat, 1.0, 0.0, width=w + 1)
    assert t["lat"].shape == (h, w + 1)
    # column c' lies between source columns c' - 1 and c'; on a checkerboard exactly one of them is valid, with weight 1/2: valid; the two border columns
    # have one tap inside, valid or not
    assert (t["W_v"][:, 1:w] == 0.5).all() and t["valid"][:, 1:w].all()
    for rr in range(h):
        for cc in range(1, w):
            src = cc - 1 if (rr + cc - 1) % 2 == 0 else cc
            assert t["lat"][rr, cc] == lat[rr, src]
        assert t["valid"][rr, 0] == (rr % 2 == 0) and t["valid"][rr, w] == ((rr + w - 1) % 2 == 0)
    assert (t["up"][1][t["valid"]] == -1.0).all() and (t["up"][0][t["valid"]] == 0.0).all()
    assert t["borderline"][:, 1:w].all()   # W_v = 1/2 exactly: the GPU tests leave such pixels out


def test_validity_is_the_half_weight_rule():
    for name, u, l, s, r in transform_cases():
        t = ref_transform(u, l, s, r)
        length_ok = ~np.isnan(t["up"][0]) | (t["W_v"] < 0.5)
        assert np.array_equal(t["valid"], (t["W_v"] >= 0.5) & length_ok), name
        assert np.array_equal(t["valid"], t["W_v"] >= 0.5), name   # the fixed inputs have no mix of borderline length
        len_err = np.abs(np.hypot(*t["up"][:, t["valid"]]) - 1.0)
        assert len_err.size == 0 or len_err.max() <= 2.0 ** -22, name


def test_borderline_pixels_are_few():
    worst = (0.0, None)
    for name, u, l, s, r in transform_cases():
        t = ref_transform(u, l, s, r)
        share = t["borderline"].mean()
        worst = max(worst, (share, (name, s, r, t["lat"].shape)), key=lambda x: x[0])
        assert share <= 0.10, (name, s, r, share)
    print(f"largest share of borderline pixels: {100 * worst[0]:.1f} % in {worst[1]}")
    # the searched variants of the noisy sets have none, so n is the device's n and the search's bound needs no allowance for them
    for name in "GHI":
        for ref in set_search_reference(name):
            assert not any(t["borderline"].any() for t in ref["transform"]), name


# ---------------------------------------------------------------- the searches
def test_output_sizes():
    assert out_size(15, 12, 1 / 1.5, -10.0) == (11, 10) and out_size(15, 12, 1 / 0.75, 10.0) == (22, 19)
    assert out_size(9, 7, 1.0, 90.0) == (7, 9) and out_size(9, 7, 1.0, -90.0) == (7, 9) and out_size(9, 7, 1.0, 180.0) == (9, 7) and out_size(9, 7, 2.0, 270.0) == (14, 18)
    assert out_size(9, 7, 1.0, 360.0) == (9, 7) and out_size(11, 10, 1.5, 0.0) == (17, 15) and out_size(3, 3, 0.01, 0.0) == (1, 1)
    assert out_size(2, 3, 0.5, 0.0) == (1, 2)   # 1.0 + 0.5 and 1.5 + 0.5: halves round up
    assert trig(90.0) == (0.0, 1.0) and trig(-90.0) == (0.0, -1.0) and trig(180.0) == (-1.0, 0.0) and trig(-180.0) == (-1.0, 0.0) and trig(720.0) == (1.0, 0.0)


def test_planted_search_finds_scale_rotation_and_offset():
    up_bg, lat_bg, objs = planted_search()
    variants = variant_list(PLANT_SCALES, PLANT_ROTATIONS)
    for (up_obj, lat_obj), size, valid_share, want in zip(objs, ((11, 10), (22, 19)), (0.73, 0.77), ((1.5, 10.0), (0.75, -10.0))):
        assert lat_obj.shape == size and abs(field_valid(up_obj, lat_obj).mean() - valid_share) < 0.01
        r = ref_search(up_bg, lat_bg, up_obj, lat_obj, variants)
        order = np.sort(r["pfd"])
        print(f"object {size}: variant {variants[r['best_variant']]} at {r['best_offset']}, PFD {order[0]:.3f} deg, runner-up {order[1]:.3f} deg, "
              f"bound {r['bound'][r['best_variant']]:.2e}")
        assert variants[r["best_variant"]] == want and r["best_offset"] == (12, 22)
        assert order[1] - order[0] >= 0.3
        assert r["bound"][r["best_variant"]] < 0.01   # with the allowance for the variant's borderline pixels


@pytest.mark.parametrize("name", list("GHI"))
def test_noisy_sets_are_determined(name):
    bgs, objs, pairs, scales, rots, _ = search_set(name)
    for (b, o), r in zip(pairs, set_search_reference(name)):
        order = np.sort(np.asarray(r["pfd"])[np.isfinite(r["pfd"])])
        bound = max(r["bound"])
        print(f"set {name} pair ({b}, {o}): best {order[0]:.4f} deg, second {order[1]:.4f} deg, device bound {bound:.2e} deg")
        assert order[1] - order[0] > 2.0 * bound
        for m in r["maps"]:   # within a variant too, so the offset is determined
            if m is not None:
                fin = np.sort(m["pfd_deg"][np.isfinite(m["pfd_deg"])])
                assert fin.size < 2 or fin[1] - fin[0] > 2.0 * bound, name
    if name == "H":
        r = set_search_reference("H")[0]
        skipped = [v for v, m in enumerate(r["maps"]) if m is None]
        assert skipped == [4, 5] and all(r["pfd"][v] == np.inf and r["offset"][v] == (-1, -1) for v in skipped)
        assert max(h * w for h, w in r["size"][:4]) > CHUNK   # more than one chunk


# ---------------------------------------------------------------- host-side contract (fails before the feature exists)
def test_exports():
    import perspective2d
    import perspectivefields_amd

    for name in ("placement_search", "transform_fields"):
        assert name in perspectivefields_amd.__all__ and callable(getattr(perspectivefields_amd, name)) and callable(getattr(perspective2d, name))
    assert callable(perspectivefields_amd.PerspectiveFields.placement_search)


NEW_SYMBOLS = ("pf_fields_transform_size", "pf_fields_transform", "pf_place_search_workspace_bytes", "pf_place_search")


def test_symbols_prototypes_and_constants():
    from perspectivefields_amd.engine import _SIGNATURES, declared_symbols, load_library

    hdr = open(os.path.join(ROOT, "include", "pf_hip.h")).read()
    assert "int pf_fields_transform_size(int h, int w, double scale, double rotation_deg, int32_t* h_out_hw" in hdr
    assert "int pf_fields_transform(int device, int n, const float* const* h_up, const float* const* h_lat, const int32_t* h_hw" in hdr
    assert "size_t pf_place_search_workspace_bytes(int n_bg, const int32_t* h_bg_hw" in hdr
    assert "int pf_place_search(int device, int n_bg, const float* const* h_bg_up, const float* const* h_bg_lat, const int32_t* h_bg_hw" in hdr
    kh = open(os.path.join(ROOT, "perspectivefields_amd", "csrc", "pf_kernels.h")).read()
    assert "struct FieldXform {\n  static constexpr int MAX = 32;" in kh and "sizeof(FieldXform) <= 4096" in kh
    assert set(NEW_SYMBOLS) <= set(declared_symbols())
    for name, res, n_args in (("pf_fields_transform_size", ctypes.c_int, 5), ("pf_fields_transform", ctypes.c_int, 10),
                              ("pf_place_search_workspace_bytes", ctypes.c_size_t, 9), ("pf_place_search", ctypes.c_int, 24)):
        assert _SIGNATURES[name][0] is res and len(_SIGNATURES[name][1]) == n_args, name
    args = _SIGNATURES["pf_place_search"][1]
    assert args[14:17] == [ctypes.c_double] * 3 and args[18] is ctypes.c_size_t and args[22] is ctypes.c_size_t
    lib = load_library()
    assert all(hasattr(lib, s) for s in NEW_SYMBOLS)


def test_the_library_and_the_reference_agree_on_sizes():
    from perspectivefields_amd.engine import load_library

    lib = load_library()
    hw = (ctypes.c_int32 * 2)()
    for h, w in ((15, 12), (9, 7), (33, 35), (1, 1), (120, 160)):
        for s in (0.5, 1 / 1.5, 0.75, 1.0, 4 / 3, 1.5, 2.0):
            for r in (0.0, 10.0, -10.0, 90.0, -90.0, 137.0, 180.0, 270.0, 450.0):
                assert lib.pf_fields_transform_size(h, w, s, r, hw) == 0 and (hw[0], hw[1]) == out_size(h, w, s, r), (h, w, s, r)
    assert lib.pf_fields_transform_size(9, 7, 1.0, 90.0, hw) == 0 and (hw[0], hw[1]) == (7, 9)
    for bad in ((0, 7, 1.0, 0.0), (9, 0, 1.0, 0.0), (9, 7, 0.0, 0.0), (9, 7, -1.0, 0.0), (9, 7, float("nan"), 0.0), (9, 7, float("inf"), 0.0),
                (9, 7, 1.0, float("nan")), (9, 7, 1.0, float("inf")), (40000, 40000, 2.0, 0.0)):
        assert lib.pf_fields_transform_size(*bad, hw) == -1 and lib.pf_last_error(None).decode().startswith("pf_fields_transform_size: "), bad
    assert lib.pf_fields_transform_size(9, 7, 1.0, 0.0, None) == -1


def test_pf_fields_transform_rejects_bad_arguments_before_device_work():
    from perspectivefields_amd.engine import load_library

    lib = load_library()
    ints = lambda *s: (ctypes.c_int32 * len(s))(*s)
    dbls = lambda *s: (ctypes.c_double * len(s))(*s)
    ptrs = lambda *s: (ctypes.c_void_p * len(s))(*s)

    def call(n=2, up=ptrs(4096, 4096), lat=ptrs(4096, 4096), hw=ints(9, 7, 5, 4), var=dbls(1.5, 10.0, 0.5, 0.0), out_hw=ints(14, 12, 3, 2), o_up=ptrs(4096, 4096),
             o_lat=ptrs(4096, 4096)):
        return lib.pf_fields_transform(0, n, up, lat, hw, var, out_hw, o_up, o_lat, None), lib.pf_last_error(None).decode()

    for kw, what in ((dict(n=0), "required"), (dict(up=None), "required"), (dict(lat=None), "required"), (dict(hw=None), "required"), (dict(var=None), "required"),
                     (dict(out_hw=None), "required"), (dict(o_up=None), "required"), (dict(o_lat=None), "required"),
                     (dict(up=ptrs(4096, 0)), "NULL"), (dict(lat=ptrs(0, 4096)), "NULL"), (dict(o_up=ptrs(4096, 0)), "NULL"), (dict(o_lat=ptrs(4096, 0)), "NULL"),
                     (dict(hw=ints(9, 0, 5, 4)), "smaller"), (dict(out_hw=ints(14, 12, 0, 2)), "smaller"), (dict(out_hw=ints(65536, 32768, 3, 2)), "2^31"),
                     (dict(var=dbls(0.0, 10.0, 0.5, 0.0)), "scale"), (dict(var=dbls(1.5, 10.0, float("inf"), 0.0)), "scale"),
                     (dict(var=dbls(1.5, float("nan"), 0.5, 0.0)), "rotation"), (dict(up=ptrs(4098, 4096)), "aligned")):
        rc, msg = call(**kw)
        assert rc == -1 and what in msg and msg.startswith("pf_fields_transform: "), (kw, rc, msg)
    if not torch.cuda.is_available():
        rc, msg = call()
        assert rc == -2 and "no HIP device" in msg, (rc, msg)


def test_pf_place_search_rejects_bad_arguments_before_device_work():
    from perspectivefields_amd.engine import load_library

    lib = load_library()
    ints = lambda *s: (ctypes.c_int32 * len(s))(*s)
    dbls = lambda *s: (ctypes.c_double * len(s))(*s)
    ptrs = lambda n: (ctypes.c_void_p * n)(*([0x1000] * n))
    dev = ctypes.c_void_p(4096)
    null2 = (ctypes.c_void_p * 2)(0x1000, 0)

    def call(n_bg=2, bg_up="ok", bg_lat="ok", bg_hw=None, n_obj=2, obj_up="ok", obj_lat="ok", obj_hw=None, n_pair=2, pairs=(0, 0, 1, 1), n_var=2,
             var=(1.0, 0.0, 0.5, 10.0), stride=2, min_valid=0.5, w_up=1.0, w_lat=1.0, maps=dev, n_maps=1 << 20, best=dev, dvar=dev, ws=dev, ws_bytes=None):
        bg_hw = bg_hw or ints(16, 24, 9, 9)
        obj_hw = obj_hw or ints(8, 24, 3, 5)
        c_pairs = None if pairs is None else ints(*pairs)
        c_var = None if var is None else dbls(*var)
        if ws_bytes is None:
            ws_bytes = lib.pf_place_search_workspace_bytes(n_bg, bg_hw, n_obj, obj_hw, n_pair, c_pairs, n_var, c_var, stride)
        arr = lambda v, n: ptrs(max(n, 1)) if v == "ok" else v
        rc = lib.pf_place_search(0, n_bg, arr(bg_up, n_bg), arr(bg_lat, n_bg), bg_hw, n_obj, arr(obj_up, n_obj), arr(obj_lat, n_obj), obj_hw, n_pair, c_pairs,
                                 n_var, c_var, stride, min_valid, w_up, w_lat, maps, n_maps, best, dvar, ws, ws_bytes, None)
        return rc, lib.pf_last_error(None).decode()

    good = (2, ints(16, 24, 9, 9), 2, ints(8, 24, 3, 5), 2, ints(0, 0, 1, 1), 2, dbls(1.0, 0.0, 0.5, 10.0), 2)
    need = lib.pf_place_search_workspace_bytes(*good)
    # pair 0: variant 0 is 8 x 24 (5 x 1 placements), variant 1 is 6 x 13 (6 x 6); pair 1: 3 x 5 (4 x 3) and 2 x 3 (4 x 4)
    n_maps = 3 * (5 + 36 + 12 + 16)
    planes = (8 * 24 + 6 * 13 + 3 * 5 + 2 * 3)
    assert need >= 12 * planes + 8 * (16 * 24 + 9 * 9 + planes) + 12 * (n_maps // 3)
    assert lib.pf_place_search_workspace_bytes(2, ints(16, 24, 9, 9), 2, ints(8, 24, 3, 5), 1, ints(1, 0), 2, dbls(1.0, 0.0, 0.5, 10.0), 2) > 0   # too large: skipped
    assert lib.pf_place_search_workspace_bytes(*good[:6], 0, good[7], 2) == 0 and lib.pf_place_search_workspace_bytes(*good[:8], 0) == 0
    for kw, what in ((dict(n_bg=0), "n_bg"), (dict(n_obj=0), "n_obj"), (dict(n_pair=0), "n_pair"), (dict(pairs=None), "n_pair"), (dict(n_var=0), "n_var"),
                     (dict(var=None), "n_var"), (dict(bg_up=None), "required"), (dict(bg_lat=None), "required"), (dict(obj_up=None), "required"),
                     (dict(obj_lat=None), "required"), (dict(best=None), "required"), (dict(dvar=None), "required"),
                     (dict(bg_up=null2), "NULL"), (dict(bg_lat=null2), "NULL"), (dict(obj_up=null2), "NULL"), (dict(obj_lat=null2), "NULL"),
                     (dict(bg_hw=ints(16, 0, 9, 9)), "smaller"), (dict(obj_hw=ints(0, 24, 3, 5)), "smaller"),
                     (dict(pairs=(0, 0, 2, 1)), "index"), (dict(pairs=(0, 2, 1, 1)), "index"), (dict(pairs=(-1, 0, 1, 1)), "index"),
                     (dict(stride=0), "stride"), (dict(stride=-3), "stride"),
                     (dict(var=(0.0, 0.0, 0.5, 10.0)), "scale"), (dict(var=(-1.0, 0.0, 0.5, 10.0)), "scale"), (dict(var=(float("nan"), 0.0, 0.5, 10.0)), "scale"),
                     (dict(var=(float("inf"), 0.0, 0.5, 10.0)), "scale"), (dict(var=(1.0, float("nan"), 0.5, 10.0)), "rotation"),
                     (dict(var=(1.0, float("inf"), 0.5, 10.0)), "rotation"), (dict(var=(1e4, 0.0, 0.5, 10.0)), "2^31"),
                     (dict(min_valid=1.5), "min_valid"), (dict(min_valid=float("nan")), "min_valid"), (dict(w_up=-1.0), "weights"), (dict(w_lat=float("inf")), "weights"),
                     (dict(maps=None), "d_maps"), (dict(n_maps=n_maps - 1), "d_maps"),
                     (dict(ws=None, ws_bytes=need), "workspace"), (dict(ws_bytes=need - 1), "workspace"),
                     (dict(maps=ctypes.c_void_p(4100)), "aligned"), (dict(best=ctypes.c_void_p(4100)), "aligned"), (dict(dvar=ctypes.c_void_p(4100)), "aligned")):
        rc, msg = call(**kw)
        assert rc == -1 and what in msg and msg.startswith("pf_place_search: "), (kw, rc, msg)
    if not torch.cuda.is_available():   # good arguments pass the checks and fail on the missing device only; with a device they would launch on these pointers
        rc, msg = call(n_maps=n_maps)
        assert rc == -2 and "no HIP device" in msg, (rc, msg)


def test_python_argument_errors_without_a_gpu():
    from perspectivefields_amd import PerspectiveFields, placement_search, transform_fields
    from perspectivefields_amd.engine import PfError

    f = lambda *s: torch.zeros(s)
    up, lat = f(2, 5, 4), f(5, 4)
    for kw in (dict(scale=0.0), dict(scale=-1.0), dict(scale=float("nan")), dict(rotation=float("inf")), dict(scale=[1.0, 2.0], rotation=[0.0, 1.0, 2.0]), dict(scale=[]),
               dict(height=0), dict(width=-2), dict(mask=torch.ones(5, 5, dtype=torch.bool)), dict(mask=torch.ones(5, 4)), dict(mask=[None, None]),
               dict(up=f(3, 5, 4)), dict(lat=f(5, 5)), dict(up=f(2, 0, 4), lat=f(0, 4)), dict(up=[], lat=[])):
        args = dict(up=up, lat=lat)
        args.update(kw)
        with pytest.raises(ValueError):
            transform_fields(args.pop("up"), args.pop("lat"), **args)
    with pytest.raises(TypeError):
        transform_fields(up, [lat])
    with pytest.raises(TypeError):
        transform_fields(up, lat, height=4.5)
    for kw in (dict(), dict(scale=[0.5, 2.0], rotation=10.0), dict(mask=torch.ones(5, 4, dtype=torch.bool), height=3, width=9)):
        with pytest.raises(PfError):
            transform_fields(up, lat, **kw)

    up_bg, lat_bg, up_obj, lat_obj = f(2, 12, 16), f(12, 16), f(2, 5, 4), f(5, 4)
    for kw in (dict(up_obj=f(3, 5, 4)), dict(lat_obj=f(5, 5)), dict(up_bg=f(12, 16)), dict(up_bg=f(2, 0, 16), lat_bg=f(0, 16)), dict(stride=0), dict(min_valid=1.5),
               dict(min_valid=-0.1), dict(weights=(1.0, -1.0)), dict(weights=(1.0, float("nan"))), dict(weights=(1.0,)), dict(pairs=[]), dict(pairs=[(0, 1)]),
               dict(pairs=[(1, 0)]), dict(pairs=[(-1, 0)]), dict(mask=torch.ones(5, 5, dtype=torch.bool)), dict(mask=torch.ones(5, 4)), dict(mask=[None, None]),
               dict(up_bg=[up_bg, up_bg], lat_bg=[lat_bg]), dict(up_bg=[], lat_bg=[]), dict(scales=()), dict(rotations=()), dict(scales=(1.0, 0.0)),
               dict(scales=(float("inf"),)), dict(rotations=(float("nan"),))):
        args = dict(up_bg=up_bg, lat_bg=lat_bg, up_obj=up_obj, lat_obj=lat_obj)
        args.update(kw)
        with pytest.raises(ValueError):
            placement_search(args.pop("up_bg"), args.pop("lat_bg"), args.pop("up_obj"), args.pop("lat_obj"), **args)
    with pytest.raises(TypeError):
        placement_search(up_bg, [lat_bg], up_obj, lat_obj)
    with pytest.raises(TypeError):
        placement_search(up_bg, lat_bg, up_obj, lat_obj, stride=1.5)
    for kw in (dict(), dict(scales=(0.5, 1.0), rotations=(-10.0, 10.0), return_maps=True), dict(up_obj=f(2, 13, 4), lat_obj=f(13, 4))):   # larger: no error here
        args = dict(up_bg=up_bg, lat_bg=lat_bg, up_obj=up_obj, lat_obj=lat_obj)
        args.update(kw)
        with pytest.raises(PfError):
            placement_search(args.pop("up_bg"), args.pop("lat_bg"), args.pop("up_obj"), args.pop("lat_obj"), **args)
    pred = lambda u, l: dict(pred_gravity_original=u, pred_latitude_original=l)
    with pytest.raises(PfError):
        PerspectiveFields.placement_search(None, pred(up_bg, lat_bg), [pred(up_obj, lat_obj)] * 2, scales=(0.5, 1.0))
    with pytest.raises(ValueError):
        PerspectiveFields.placement_search(None, pred(up_bg, lat_bg), pred(up_obj, lat_obj), scales=(-1.0,))


def test_search_kernels_are_in_the_library_without_scratch():
    """scripts/kernel_resources.py on the built library: the four kernels are there for gfx950 with no spilled register and no scratch; the best
    kernels' LDS is one (pfd, placement) record per thread"""
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
    for name, lds in (("pf::field_xform_kernel", 0), ("pf::place_count_kernel", 4 * 1024), ("pf::place_best_tile_kernel", 16 * 256), ("pf::place_best_pair_kernel", 16 * 256)):
        r = by[name]
        print(name, {k: r[k] for k in r if k != "kernel"})
        assert r["spill"] == 0 and r["scratch"] == 0 and r["lds"] <= lds, r
