"""Objects pasted into backgrounds (include/pf_hip.h pf_composite; perspectivefields_amd.composite_objects, PerspectiveFields.composite): the fp64
reference the GPU tests compare against, the fixed inputs, checks of the reference itself, and the host-side contract.  No GPU here.

Model, in fp64 on the inputs as stored.  Background (H, W, 3), object (h, w, 3), both uint8 or float32 on the 0 - 255 scale; alpha (h, w) float32
clamped to [0, 1], NaN = 0, None = 1.  A row (s, phi in degrees, row, col, h', w') places the h' x w' box of the transformed object with its top-left
corner at (row, col) of the background.  The row is inactive -- the output is the background, the coverage 0 -- when s is not finite and > 0; phi,
row or col is not finite; row or col is not integer-valued or is 2^30 or more in magnitude; h' or w' is < 1, not integer-valued or 2^31 or more.
Output pixel (R, C), r' = R - row, c' = C - col; outside [0, h') x [0, w') the background.  Inside, for the sub-samples a, b < S, a-major:
d = (c' + (b + 1/2) / S - w'/2, r' + (a + 1/2) / S - h'/2), source position (x, y) = (w/2, h/2) + R(-phi) d / s - (1/2, 1/2) with cos and sin from
remainder(phi, 360), exact at the multiples of 90 (tests/test_placement_search_ref.py trig).  Four bilinear taps; a tap outside the array is
transparent (alpha 0: kept in the mean, not renormalised away); a tap whose alpha is 0 is skipped, so its colour is never read.
A_ab = sum w_k alpha_k, P_ab = sum (w_k alpha_k) c_k; A and P are the means over the S x S sub-samples.
edge "soft": cov = opacity A, out = bg (1 - cov) + opacity P.  edge "hard": where A >= 1/2, cov = opacity and out = bg (1 - opacity) + opacity P / A;
elsewhere cov = 0.  Where cov = 0 the output is the background's bits.  float32 outputs are the value rounded once; uint8 outputs are
floor(value + 1/2) clamped to [0, 255].

What the device may differ by (the GPU tests' tolerances), u = 2^-24, with the position bound of section 26 and a FULL fp32 ulp
(2 u relative) on cos and sin, which the device takes from its own fp64 library.  d is exact for S in {1, 2, 4}; for S = 3 the quotient
(b + 1/2) / 3, the sum with c' and the difference each round: e_d <= u (2 + c' + |d_x|), likewise down.  p_x = fma(c, d_x, rnd(s d_y)): 2 u |d_x| and
2 u |d_y| for the rounded c and s, u |d_y| for the product, u (|d_x| + |d_y|) for the result: <= 5 u (|d_x| + |d_y|), plus e_dx + e_dy.
x = fma(p_x, rnd(1 / s), w/2 - 1/2) adds u |p_x| / s for the rounded reciprocal and u |x| for the result:
    E = u (6 (|d_x| + |d_y|) / s + max(|x|, |y|, 1)) + (e_dx + e_dy) / s       per coordinate.
The weights' x-derivatives sum to 2 in absolute value, so do the y-derivatives, and a weight is a rounded product of rounded factors: the weights
move by D = 4 E + 3 u in total and their sum stays 1 to 3 u.  With v_k the taps' values (alpha or alpha c; 0 for a transparent tap) a mean
sum w_k v_k therefore moves by at most D x (largest difference among the v_k) + 3 u max |v_k|.  The position may cross into a neighbouring cell of the
source within E, so the largest difference is taken over the 4 x 4 taps around the cell, not its 4.  That gives tol_A and tol_P per sub-sample and
their means per pixel.  Soft: the value moves by opacity (|bg| tol_A + tol_P), the coverage by opacity tol_A.  Hard, with A >= 1/2: P / A moves by
(tol_P + |P / A| tol_A) / (A - tol_A).  Then the one rounding of an fp32 output, u |value|, and of the fp32 coverage.  A uint8 output equals the
reference's wherever the fp64 value is farther from a rounding tie than its bound, and is within 1 LSB everywhere.
A pixel with |A - 1/2| < 1e-3 is BORDERLINE for the hard edge: it may change sides on the device, and hard-edge comparisons leave it out.

Which combinations run (the full cross product of 7 variants x 3 alphas x 3 offsets x 3 S x 2 opacities x 2 edges x 2 dtypes is 1512 cases): CASES
below holds every (variant, alpha) pair with both edges where the edge applies, for both dtypes, the offsets, S and opacities cycling through them
so that each value meets each variant; then every (offset, S, opacity) on the variant (0.75, -10); then the dyadic cases in full.  The hard edge runs
with alpha in {0, 1} only (opaque, ellipse): a quarter alpha of exactly 1/2 is borderline everywhere.  (1.5, 0) runs with the soft edge only."""
import ctypes
import functools
import itertools
import math
import os

import numpy as np
import pytest
import torch

from tests.test_placement_search_ref import out_size, ref_transform, trig

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24
BORDER = 1e-3
BG_HW, OBJ_HW = (40, 56), (15, 12)
VARIANTS = ((1.0, 0.0), (0.75, -10.0), (1.5, 10.0), (2.0, 90.0), (0.5, 137.0), (1.25, 180.0), (1.5, 0.0))
SIZES = ((15, 12), (13, 11), (25, 22), (24, 30), (10, 10), (19, 15), (23, 18))
OFFSETS = ((13, 22), (-3, 50), (45, 60))   # inside; clipped at the top and at the right; wholly outside
SAMPLES, OPACITIES = (1, 2, 3), (1.0, 0.5)
ALPHAS = ("opaque", "ellipse", "quarter")
DTYPES = ("uint8", "float32")


# ---------------------------------------------------------------- the reference
def row_active(place):
    s, phi, row, col, hb, wb = (float(v) for v in place)
    whole = lambda v: math.isfinite(v) and v == math.floor(v)
    return (math.isfinite(s) and s > 0 and math.isfinite(phi) and whole(row) and whole(col) and abs(row) < 2 ** 30 and abs(col) < 2 ** 30 and
            whole(hb) and whole(wb) and 1 <= hb < 2 ** 31 and 1 <= wb < 2 ** 31)


def _window_range(v, x0, y0):
    """largest difference among the 4 x 4 taps around the cell (x0, y0) of the plane v (h, w), 0 outside the array"""
    h, w = v.shape
    pad = np.zeros((h + 6, w + 6))
    pad[3:h + 3, 3:w + 3] = v
    xc, yc = np.clip(x0, -2, w).astype(np.int64) + 3, np.clip(y0, -2, h).astype(np.int64) + 3
    lo, hi = np.full(x0.shape, np.inf), np.full(x0.shape, -np.inf)
    for ty in range(-1, 3):
        for tx in range(-1, 3):
            t = pad[yc + ty, xc + tx]
            lo, hi = np.minimum(lo, t), np.maximum(hi, t)
    return hi - lo, np.maximum(np.abs(lo), np.abs(hi))


def ref_composite(bg, obj, alpha, place, opacity=1.0, edge="soft", samples=1):
    """dict: value (H, W, 3) float64 -- the blend before its one rounding, the background's value where cov = 0; out: the output in bg's dtype;
    cov (H, W) float64; A (H, W), 0 outside the box; box (H, W) bool; borderline (H, W) bool; tol (H, W, 3), tol_cov (H, W): what the device may
    differ by before the output's rounding (tol includes the fp32 rounding for float32 backgrounds); 0 outside the box, and with the hard edge outside
    the covered pixels"""
    bg, obj = np.asarray(bg), np.asarray(obj)
    H, W = bg.shape[:2]
    h, w = obj.shape[:2]
    value = bg.astype(np.float64)
    res = dict(value=value, out=bg.copy(), cov=np.zeros((H, W)), A=np.zeros((H, W)), box=np.zeros((H, W), dtype=bool), borderline=np.zeros((H, W), dtype=bool),
               tol=np.zeros((H, W, 3)), tol_cov=np.zeros((H, W)), active=row_active(place))
    if not res["active"]:
        return res
    s, phi = float(place[0]), float(place[1])
    row, col, hb, wb = (int(v) for v in place[2:])
    r0, r1, c0, c1 = min(max(row, 0), H), min(max(row + hb, 0), H), min(max(col, 0), W), min(max(col + wb, 0), W)
    if r1 <= r0 or c1 <= c0:
        return res
    al = np.ones((h, w)) if alpha is None else np.asarray(alpha).astype(np.float64)
    with np.errstate(invalid="ignore"):
        al = np.where(al > 0, np.minimum(al, 1.0), 0.0)   # NaN -> 0
    col_f = np.where(al[..., None] > 0, obj.astype(np.float64), 0.0)   # what lies under a zero alpha is never read
    prem = al[..., None] * col_f
    cs, sn = trig(phi)
    S = samples
    rr, cc = np.meshgrid(np.arange(r0, r1) - row, np.arange(c0, c1) - col, indexing="ij")
    A, P = np.zeros(rr.shape), np.zeros(rr.shape + (3,))
    tol_A, tol_P = np.zeros(rr.shape), np.zeros(rr.shape + (3,))
    exact_d = S in (1, 2, 4)
    for a in range(S):
        for b in range(S):
            dx, dy = cc + (b + 0.5) / S - wb / 2, rr + (a + 0.5) / S - hb / 2
            x, y = w / 2 + (cs * dx + sn * dy) / s - 0.5, h / 2 + (cs * dy - sn * dx) / s - 0.5
            x0, y0 = np.floor(x), np.floor(y)
            ax, ay = x - x0, y - y0
            A_ab, P_ab = np.zeros(rr.shape), np.zeros(rr.shape + (3,))
            for ty in (0, 1):
                for tx in (0, 1):
                    xi, yi = (x0 + tx).astype(np.int64), (y0 + ty).astype(np.int64)
                    inside = (xi >= 0) & (xi < w) & (yi >= 0) & (yi < h)
                    xc, yc = np.clip(xi, 0, w - 1), np.clip(yi, 0, h - 1)
                    wa = np.where(inside, (ay if ty else 1 - ay) * (ax if tx else 1 - ax) * al[yc, xc], 0.0)
                    A_ab += wa
                    P_ab += wa[..., None] * col_f[yc, xc]
            A += A_ab
            P += P_ab
            e_d = 0.0 if exact_d else U * (2 + cc + np.abs(dx)) + U * (2 + rr + np.abs(dy))
            E = U * (6 * (np.abs(dx) + np.abs(dy)) / s + np.maximum(np.maximum(np.abs(x), np.abs(y)), 1.0)) + e_d / s
            D = 4 * E + 3 * U
            rng_a, max_a = _window_range(al, x0, y0)
            tol_A += D * rng_a + 3 * U * max_a
            for ch in range(3):
                rng_p, max_p = _window_range(prem[..., ch], x0, y0)
                tol_P[..., ch] += D * rng_p + 3 * U * max_p
    A, P, tol_A, tol_P = A / S ** 2, P / S ** 2, tol_A / S ** 2, tol_P / S ** 2
    b = value[r0:r1, c0:c1]
    if edge == "soft":
        cov = opacity * A
        val = b * (1 - cov)[..., None] + opacity * P
        tol = opacity * (np.abs(b) * tol_A[..., None] + tol_P)
        tol_cov = opacity * tol_A
    else:
        on = A >= 0.5
        with np.errstate(invalid="ignore", divide="ignore"):
            q = np.where(on[..., None], P / A[..., None], 0.0)
            tol = np.where(on[..., None], opacity * (tol_P + np.abs(q) * tol_A[..., None]) / (A - tol_A)[..., None], 0.0)
        cov = np.where(on, opacity, 0.0)
        val = b * (1 - cov)[..., None] + opacity * q
        tol_cov = np.zeros(rr.shape)
    covered = cov > 0
    val = np.where(covered[..., None], val, b)
    f32 = bg.dtype == np.float32
    # the soft edge keeps its bound where nothing is covered here: a position that differs in its last bits may reach a tap this one does not
    within = np.ones_like(covered) if edge == "soft" else covered
    tol = np.where(within[..., None], tol + 1e-12 + (U * np.abs(val) if f32 else 0.0), 0.0)
    res["value"][r0:r1, c0:c1] = val
    res["cov"][r0:r1, c0:c1] = cov
    res["A"][r0:r1, c0:c1] = A
    res["box"][r0:r1, c0:c1] = True
    res["borderline"][r0:r1, c0:c1] = np.abs(A - 0.5) < BORDER
    res["tol"][r0:r1, c0:c1] = tol
    res["tol_cov"][r0:r1, c0:c1] = np.where(within, tol_cov + U * cov + 1e-15, 0.0)
    rounded = val.astype(np.float32) if f32 else np.clip(np.floor(val + 0.5), 0, 255).astype(np.uint8)
    res["out"][r0:r1, c0:c1] = np.where(covered[..., None], rounded, bg[r0:r1, c0:c1])
    return res


def tie_distance(value):
    """distance of a uint8 output's fp64 value from the nearest rounding tie (the half-integers inside the clamp)"""
    return np.abs(value - np.floor(value) - 0.5)


# ---------------------------------------------------------------- fixed inputs (shared with tests/test_gpu_composite.py)
def ellipse(h, w):
    r, c = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    return ((r + 0.5 - h / 2) / (h / 2)) ** 2 + ((c + 0.5 - w / 2) / (w / 2)) ** 2 <= 1.0


@functools.lru_cache(None)
def picture(kind, dtype, hw=None, seed=None):
    """a background or an object: uint8, or float32 multiples of 1/4 in [0, 256) so that the dyadic cases stay exact"""
    h, w = hw or (BG_HW if kind == "bg" else OBJ_HW)
    rng = np.random.default_rng((11 if kind == "bg" else 23) if seed is None else seed)
    a = rng.integers(0, 256, size=(h, w, 3))
    a = a.astype(np.uint8) if dtype == "uint8" else (a + rng.integers(0, 4, size=(h, w, 3)) / 4).astype(np.float32)
    a.setflags(write=False)
    return a


@functools.lru_cache(None)
def alpha_plane(name, hw=OBJ_HW):
    h, w = hw
    if name == "opaque":
        return None
    a = ellipse(h, w).astype(np.float32)
    if name == "quarter":
        a = a * (np.random.default_rng(37).integers(0, 5, size=(h, w)) / 4).astype(np.float32)
    a.setflags(write=False)
    return a


def variant_size(v):
    return SIZES[VARIANTS.index(v)]


def make_place(variant, offset, size=None):
    return (variant[0], variant[1], float(offset[0]), float(offset[1])) + tuple(float(x) for x in (size or variant_size(variant)))


def is_dyadic(c):
    return c["variant"][0] in (1.0, 2.0) and c["variant"][1] % 90.0 == 0.0 and c["samples"] in (1, 2) and c["edge"] == "soft"


def _cases():
    out, i = [], 0
    for dtype in DTYPES:
        for variant, alpha in itertools.product(VARIANTS, ALPHAS):
            for edge in ("soft", "hard"):
                if edge == "hard" and (alpha == "quarter" or variant == (1.5, 0.0)):
                    continue
                out.append(dict(dtype=dtype, variant=variant, alpha=alpha, edge=edge, offset=OFFSETS[i % 3], samples=SAMPLES[(i // 3) % 3],
                                opacity=OPACITIES[(i // 9) % 2]))
                i += 4   # coprime to 3, so that the three cycles do not run in step
    for offset, S, op in itertools.product(OFFSETS, SAMPLES, OPACITIES):
        out.append(dict(dtype=DTYPES[len(out) % 2], variant=(0.75, -10.0), alpha="ellipse", edge="soft", offset=offset, samples=S, opacity=op))
    for dtype, variant, S, op in itertools.product(DTYPES, ((1.0, 0.0), (2.0, 90.0), (1.0, 180.0), (2.0, 270.0)), (1, 2), OPACITIES):
        size = variant_size(variant) if variant in VARIANTS else out_size(*OBJ_HW, *variant)
        out.append(dict(dtype=dtype, variant=variant, alpha="quarter", edge="soft", offset=(13, 22) if S == 1 else (-3, 50), samples=S, opacity=op, size=size))
    seen, uniq = set(), []
    for c in out:
        c.setdefault("size", variant_size(c["variant"]) if c["variant"] in VARIANTS else None)
        key = tuple(sorted(c.items()))
        if key not in seen:
            seen.add(key)
            uniq.append(c)
    return uniq


CASES = _cases()


def case_id(c):
    return f"{c['dtype']}-s{c['variant'][0]}-r{c['variant'][1]}-{c['alpha']}-{c['edge']}-at{c['offset'][0]}_{c['offset'][1]}-S{c['samples']}-op{c['opacity']}"


def case_inputs(c):
    return picture("bg", c["dtype"]), picture("obj", c["dtype"]), alpha_plane(c["alpha"]), make_place(c["variant"], c["offset"], c["size"])


@functools.lru_cache(None)
def _case_reference(i):
    c = CASES[i]
    bg, obj, al, place = case_inputs(c)
    r = ref_composite(bg, obj, al, place, c["opacity"], c["edge"], c["samples"])
    for v in r.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return r


def case_reference(c):
    return _case_reference(CASES.index(c))


# ---------------------------------------------------------------- the reference itself
def test_the_cases_cover_every_value():
    for key, values in (("variant", VARIANTS), ("alpha", ALPHAS), ("offset", OFFSETS), ("samples", SAMPLES), ("opacity", OPACITIES), ("dtype", DTYPES)):
        assert {c[key] for c in CASES} >= set(values), key
    for v in VARIANTS:   # every variant meets every offset, S and opacity
        mine = [c for c in CASES if c["variant"] == v]
        assert {c["samples"] for c in mine} == set(SAMPLES) and {c["opacity"] for c in mine} == set(OPACITIES), v
    assert not [c for c in CASES if c["variant"] == (1.5, 0.0) and c["edge"] == "hard"]
    assert sum(is_dyadic(c) for c in CASES) >= 32 and len(CASES) < 200
    print(len(CASES), "cases,", sum(is_dyadic(c) for c in CASES), "dyadic")


def test_sizes_are_the_transform_sizes():
    for v, hw in zip(VARIANTS, SIZES):
        assert out_size(*OBJ_HW, *v) == hw, v
    assert int(ellipse(*OBJ_HW).sum()) == 140
    q = alpha_plane("quarter")
    assert set(np.unique(q * 4)) <= {0.0, 1.0, 2.0, 3.0, 4.0} and (q[~ellipse(*OBJ_HW)] == 0).all()


@pytest.mark.parametrize("dtype", DTYPES)
def test_identity(dtype):
    bg, obj = picture("bg", dtype), picture("obj", dtype)
    al = alpha_plane("ellipse")
    for off in OFFSETS:
        r = ref_composite(bg, obj, al, make_place((1.0, 0.0), off), 1.0, "soft", 1)
        want, want_cov = bg.copy(), np.zeros(BG_HW)
        for i, j in zip(*np.nonzero(al == 1)):
            if 0 <= off[0] + i < BG_HW[0] and 0 <= off[1] + j < BG_HW[1]:
                want[off[0] + i, off[1] + j] = obj[i, j]
                want_cov[off[0] + i, off[1] + j] = 1.0
        assert np.array_equal(r["out"], want) and np.array_equal(r["value"], want.astype(np.float64)), off
        assert np.array_equal(r["cov"], want_cov)
    out = ref_composite(bg, obj, al, make_place((1.0, 0.0), OFFSETS[2]))
    assert np.array_equal(out["out"], bg) and not out["cov"].any()   # wholly outside


def test_what_lies_under_a_zero_alpha_never_leaks():
    bg, obj = picture("bg", "float32"), picture("obj", "float32").copy()
    al = alpha_plane("ellipse")
    clean = ref_composite(bg, obj, al, make_place((1.5, 10.0), (5, 7)), 0.5, "soft", 2)
    obj[al == 0] = np.nan
    al2 = al.copy()
    al2[0, 0] = np.nan   # a NaN alpha is 0, which (0, 0) is already
    dirty = ref_composite(bg, obj, al2, make_place((1.5, 10.0), (5, 7)), 0.5, "soft", 2)
    assert np.array_equal(clean["value"], dirty["value"]) and np.isfinite(dirty["value"]).all()


def test_inactive_rows():
    bg, obj = picture("bg", "uint8"), picture("obj", "uint8")
    nan, inf = float("nan"), float("inf")
    for place in ((nan, 0, 3, 4, 15, 12), (0.0, 0, 3, 4, 15, 12), (-1.0, 0, 3, 4, 15, 12), (inf, 0, 3, 4, 15, 12), (1, nan, 3, 4, 15, 12), (1, inf, 3, 4, 15, 12),
                  (1, 0, 3.5, 4, 15, 12), (1, 0, 3, nan, 15, 12), (1, 0, 2.0 ** 30, 4, 15, 12), (1, 0, 3, 4, 0, 12), (1, 0, 3, 4, 15, 12.5), (1, 0, 3, 4, 15, 2.0 ** 31),
                  (nan, nan, -1, -1, -1, -1)):   # the last one: placement_search's "nothing fits"
        assert not row_active(place), place
        r = ref_composite(bg, obj, None, place)
        assert np.array_equal(r["out"], bg) and not r["cov"].any() and not r["box"].any()
    assert row_active((1, 0, -3, 4, 15, 12)) and row_active((0.5, 720.0, -(2.0 ** 30) + 1, 0, 1, 1))


@pytest.mark.parametrize("S", (2, 3))
@pytest.mark.parametrize("variant", ((0.75, -10.0), (1.5, 10.0), (2.0, 90.0), (0.5, 137.0)))
def test_block_mean_property(variant, S):
    """samples = S equals the S x S block mean of samples = 1 on the background replicated S times per side under scale s S, offset S, size S"""
    bg, obj, al = picture("bg", "float32"), picture("obj", "float32"), alpha_plane("quarter")
    hb, wb = variant_size(variant)
    for off in OFFSETS[:2]:
        small = ref_composite(bg, obj, al, make_place(variant, off), 0.5, "soft", S)
        big_bg = np.repeat(np.repeat(bg, S, axis=0), S, axis=1)
        big = ref_composite(big_bg, obj, al, (variant[0] * S, variant[1], off[0] * S, off[1] * S, hb * S, wb * S), 0.5, "soft", 1)
        mean = lambda a: a.reshape(BG_HW[0], S, BG_HW[1], S, *a.shape[2:]).mean(axis=(1, 3))
        assert np.abs(mean(big["value"]) - small["value"]).max() <= 1e-10 and np.abs(mean(big["cov"]) - small["cov"]).max() <= 1e-13, (variant, S, off)
        assert small["cov"].max() > 0.2


@pytest.mark.parametrize("variant", [v for v in VARIANTS if v != (1.5, 0.0)])
@pytest.mark.parametrize("alpha", ("opaque", "ellipse"))
def test_hard_edge_is_the_silhouette_of_the_field_transform(variant, alpha):
    """outside the borderline pixels the covered set at S = 1 is the validity of section 26's reference transform of fields that are valid exactly
    where alpha = 1; and the borderline cap: at most 2 % of the box"""
    al = alpha_plane(alpha)
    valid = np.ones(OBJ_HW, dtype=bool) if al is None else al == 1
    up = np.stack([np.ones(OBJ_HW, dtype=np.float32), np.zeros(OBJ_HW, dtype=np.float32)])
    lat = np.where(valid, np.float32(0), np.float32(np.nan)).astype(np.float32)
    t = ref_transform(up, lat, *variant)
    hb, wb = variant_size(variant)
    assert t["valid"].shape == (hb, wb)
    big = picture("bg", "uint8", (hb + 4, wb + 6), 5)
    r = ref_composite(big, picture("obj", "uint8"), al, make_place(variant, (2, 3)), 1.0, "hard", 1)
    sl = (slice(2, 2 + hb), slice(3, 3 + wb))
    assert r["box"][sl].all() and r["box"].sum() == hb * wb
    keep = ~r["borderline"][sl]
    n_border = int((~keep).sum())
    print(f"{variant} {alpha}: {n_border} of {hb * wb} borderline ({100.0 * n_border / (hb * wb):.2f} %), {int((r['cov'] > 0).sum())} covered")
    assert n_border <= 0.02 * hb * wb
    assert np.array_equal((r["cov"][sl] > 0)[keep], t["valid"][keep]) and np.allclose(r["A"][sl], t["W_v"], atol=1e-12)
    assert set(np.unique(r["cov"])) <= {0.0, 1.0}


@pytest.mark.parametrize("i", [i for i, c in enumerate(CASES) if c["edge"] == "hard"], ids=lambda i: case_id(CASES[i]))
def test_borderline_cap(i):
    c, r = CASES[i], case_reference(CASES[i])
    hb, wb = c["size"]
    assert int(r["borderline"].sum()) <= 0.02 * hb * wb, case_id(c)


@pytest.mark.parametrize("i", [i for i, c in enumerate(CASES) if is_dyadic(c)], ids=lambda i: case_id(CASES[i]))
def test_dyadic_cases_are_exact_in_fp32(i):
    c, r = CASES[i], case_reference(CASES[i])
    assert c["alpha"] == "quarter" or c["variant"] in VARIANTS
    assert np.array_equal(r["value"].astype(np.float32).astype(np.float64), r["value"]), case_id(c)
    assert np.array_equal(r["cov"].astype(np.float32).astype(np.float64), r["cov"])
    assert np.array_equal((r["value"] * 2 ** 14) % 1, np.zeros_like(r["value"]))   # few bits: nothing an fp64 sum could round either


@pytest.mark.parametrize("i", [i for i, c in enumerate(CASES) if c["dtype"] == "uint8" and c["variant"][1] in (-10.0, 10.0, 137.0)], ids=lambda i: case_id(CASES[i]))
def test_uint8_tie_cap(i):
    """at most 1 % of a case's pixels lie within their bound of a rounding tie, where the device may round the other way"""
    c, r = CASES[i], case_reference(CASES[i])
    near = (tie_distance(r["value"]) <= r["tol"]) & (r["cov"] > 0)[..., None]
    share = near.any(-1).sum() / (BG_HW[0] * BG_HW[1])
    assert share <= 0.01, (case_id(c), share)


def test_the_tolerance_leaves_the_checks_their_meaning():
    """the bound is a few hundred u of the largest difference among neighbouring object pixels -- random pictures are its worst case --, far below one
    uint8 step and one per cent of coverage; and it is there wherever something is pasted off the pixel centres"""
    worst = 0.0, 0.0
    for c in CASES:
        r = case_reference(c)
        worst = max(worst[0], r["tol"].max()), max(worst[1], r["tol_cov"].max())
        assert r["tol"].max() <= 0.05 and r["tol_cov"].max() <= 2e-4, (case_id(c), r["tol"].max(), r["tol_cov"].max())
        assert not r["tol"][~r["box"]].any() and not r["tol_cov"][~r["box"]].any()   # outside the box: the background's bits
        if (r["cov"] > 0).any() and c["variant"][1] % 90.0 != 0.0:
            assert r["tol"][r["cov"] > 0].min() > 0
    print(f"largest allowed difference over all cases: {worst[0]:.2e} of 255, coverage {worst[1]:.2e}")


# ---------------------------------------------------------------- host-side contract (fails before the feature exists)
NEW_SYMBOLS = ("pf_composite_workspace_bytes", "pf_composite")


def test_exports():
    import perspective2d
    import perspectivefields_amd

    assert "composite_objects" in perspectivefields_amd.__all__
    assert callable(perspectivefields_amd.composite_objects) and callable(perspective2d.composite_objects)
    assert callable(perspectivefields_amd.PerspectiveFields.composite)


def test_symbols_prototypes_and_constants():
    from perspectivefields_amd import perspectivefields as pfm
    from perspectivefields_amd.engine import _SIGNATURES, declared_symbols, load_library

    hdr = open(os.path.join(ROOT, "include", "pf_hip.h")).read()
    assert "size_t pf_composite_workspace_bytes(int n);" in hdr
    assert "int pf_composite(int device, int n_bg, const void* const* h_bg, const int32_t* h_bg_hw /*[n_bg][2]*/, int n_obj, const void* const* h_obj," in hdr
    assert "#define PF_COMPOSITE_SOFT 0" in hdr and "#define PF_COMPOSITE_HARD 1" in hdr
    assert (pfm.COMPOSITE_SOFT, pfm.COMPOSITE_HARD) == (0, 1)
    kh = open(os.path.join(ROOT, "perspectivefields_amd", "csrc", "pf_kernels.h")).read()
    assert "struct CompositeBatch {\n  static constexpr int MAX = 32;" in kh and "sizeof(CompositeBatch) <= 4096" in kh
    assert set(NEW_SYMBOLS) <= set(declared_symbols())
    for name, res, n_args in (("pf_composite_workspace_bytes", ctypes.c_size_t, 1), ("pf_composite", ctypes.c_int, 20)):
        assert _SIGNATURES[name][0] is res and len(_SIGNATURES[name][1]) == n_args, name
    args = _SIGNATURES["pf_composite"][1]
    assert args[12] is ctypes.c_double and args[18] is ctypes.c_size_t
    lib = load_library()
    assert all(hasattr(lib, s) for s in NEW_SYMBOLS)
    assert lib.pf_composite_workspace_bytes(0) == 0 and lib.pf_composite_workspace_bytes(-3) == 0
    assert lib.pf_composite_workspace_bytes(1) >= 48 and lib.pf_composite_workspace_bytes(33) >= 33 * 48


def test_pf_composite_rejects_bad_arguments_before_device_work():
    from perspectivefields_amd.engine import load_library

    lib = load_library()
    ints = lambda *s: (ctypes.c_int32 * len(s))(*s)
    ptrs = lambda *s: (ctypes.c_void_p * len(s))(*s)
    dev = ctypes.c_void_p(0x10000)
    need = lib.pf_composite_workspace_bytes(2)

    def call(n_bg=2, bg=ptrs(0x1000, 0x2000), bg_hw=ints(40, 56, 9, 9), n_obj=2, obj=ptrs(0x3000, 0x4000), alpha=ptrs(0x5000, 0), obj_hw=ints(15, 12, 3, 5), dtype=1,
             n=2, jobs=ints(0, 0, 1, 1), place=dev, opacity=1.0, edge=0, samples=1, out=ptrs(0x6000, 0x7000), cov=None, ws=dev, ws_bytes=need):
        rc = lib.pf_composite(0, n_bg, bg, bg_hw, n_obj, obj, alpha, obj_hw, dtype, n, jobs, place, opacity, edge, samples, out, cov, ws, ws_bytes, None)
        return rc, lib.pf_last_error(None).decode()

    nan, inf = float("nan"), float("inf")
    for kw, what in ((dict(n_bg=0), ">= 1"), (dict(n_obj=0), ">= 1"), (dict(n=0), ">= 1"), (dict(n=-2), ">= 1"),
                     (dict(bg=None), "required"), (dict(bg_hw=None), "required"), (dict(obj=None), "required"), (dict(obj_hw=None), "required"),
                     (dict(jobs=None), "required"), (dict(place=None), "required"), (dict(out=None), "required"),
                     (dict(bg=ptrs(0x1000, 0)), "NULL"), (dict(obj=ptrs(0, 0x4000)), "NULL"), (dict(out=ptrs(0x6000, 0)), "NULL"),
                     (dict(bg_hw=ints(40, 0, 9, 9)), "smaller"), (dict(obj_hw=ints(15, 12, 0, 5)), "smaller"), (dict(bg_hw=ints(65536, 32768, 9, 9)), "2^31"),
                     (dict(obj_hw=ints(15, 12, 46341, 46341)), "2^31"),
                     (dict(jobs=ints(0, 0, 2, 1)), "out of range"), (dict(jobs=ints(0, 2, 1, 1)), "out of range"), (dict(jobs=ints(-1, 0, 1, 1)), "out of range"),
                     (dict(samples=0), "samples"), (dict(samples=5), "samples"),
                     (dict(opacity=-0.1), "opacity"), (dict(opacity=1.5), "opacity"), (dict(opacity=nan), "opacity"), (dict(opacity=inf), "opacity"),
                     (dict(edge=2), "edge"), (dict(edge=-1), "edge"), (dict(dtype=2), "dtype"), (dict(dtype=-1), "dtype"),
                     (dict(ws=None), "workspace"), (dict(ws_bytes=need - 1), "workspace"), (dict(ws_bytes=0), "workspace"),
                     (dict(out=ptrs(0x6000, 0x2000)), "its background"), (dict(out=ptrs(0x1000, 0x7000)), "its background"),
                     (dict(out=ptrs(0x6000, 0x1000)), "background 0"), (dict(out=ptrs(0x6000, 0x6000)), "share an output"),
                     (dict(bg=ptrs(0x1002, 0x2000)), "aligned"), (dict(alpha=ptrs(0x5001, 0)), "aligned"), (dict(out=ptrs(0x6000, 0x7002)), "aligned"),
                     (dict(place=ctypes.c_void_p(0x10004)), "aligned"), (dict(cov=ctypes.c_void_p(0x8002)), "aligned")):
        rc, msg = call(**kw)
        assert rc == -1 and what in msg and msg.startswith("pf_composite: "), (kw, rc, msg)
    if not torch.cuda.is_available():   # good arguments pass the checks and fail on the missing device only; with a device they would launch on these pointers
        for kw in (dict(), dict(alpha=None), dict(dtype=0, bg=ptrs(0x1001, 0x2000), out=ptrs(0x6003, 0x7000)), dict(cov=ctypes.c_void_p(0x8000), edge=1, samples=4, opacity=0.0)):
            rc, msg = call(**kw)
            assert rc == -2 and "no HIP device" in msg, (kw, rc, msg)


def test_python_argument_errors_before_the_library_is_loaded(monkeypatch):
    from perspectivefields_amd import PerspectiveFields, composite_objects, engine
    from perspectivefields_amd.engine import PfError

    def no_library():
        raise AssertionError("the library was loaded before the arguments were checked")

    monkeypatch.setattr(engine, "load_library", no_library)
    f = lambda *s: torch.zeros(s)
    u8 = lambda *s: torch.zeros(s, dtype=torch.uint8)
    bg, obj = f(12, 16, 3), f(5, 4, 3)
    for kw in (dict(offset=(1, 2, 3)), dict(offset=1), dict(offset=[(1, 2), (3, 4)]), dict(offset="here"), dict(scale=[1.0, 2.0]), dict(rotation=[0.0, 1.0, 2.0]),
               dict(scale=0.0), dict(scale=-1.0), dict(scale=float("nan")), dict(rotation=float("inf")),   # size=None needs a variant that has a size
               dict(scale=torch.ones(())), dict(rotation=torch.zeros(1)), dict(size=(5,)), dict(size=[(5, 4), (5, 4)]), dict(scale=torch.ones(2), size=(5, 4)),
               dict(offset=torch.zeros(3), size=(5, 4)), dict(size=torch.ones(1, 3)),
               dict(opacity=1.5), dict(opacity=-0.1), dict(opacity=float("nan")), dict(edge="feather"), dict(edge=1), dict(samples=0), dict(samples=5), dict(samples=2.0),
               dict(samples=True), dict(alpha=torch.ones(5, 5)), dict(alpha=torch.ones(5, 4, dtype=torch.int32)), dict(alpha=[None, None]),
               dict(pairs=[]), dict(pairs=[(0, 1)]), dict(pairs=[(1, 0)]), dict(pairs=[(-1, 0)]),
               dict(backgrounds=f(12, 16)), dict(backgrounds=f(12, 16, 4)), dict(backgrounds=f(0, 16, 3)), dict(backgrounds=f(0, 12, 16, 3)), dict(backgrounds=[]),
               dict(objects=f(5, 4, 2)), dict(objects=f(5, 0, 3)), dict(objects=[]), dict(objects=u8(5, 4, 3)), dict(backgrounds=bg.double()),
               dict(objects=[f(5, 4, 3), f(5, 4, 4)]), dict(objects=f(5, 4, 4), alpha=torch.ones(5, 4))):
        args = dict(backgrounds=bg, objects=obj, offset=(1, 2))
        args.update(kw)
        with pytest.raises(ValueError):
            composite_objects(args.pop("backgrounds"), args.pop("objects"), **args)
    with pytest.raises(TypeError):
        composite_objects(bg, [obj, None], offset=(1, 2))
    with pytest.raises(TypeError):
        composite_objects(np.zeros((12, 16, 3)), obj, offset=(1, 2))
    with pytest.raises(TypeError):
        composite_objects(bg, obj, offset=(1, 2), pairs=[(0.5, 0)])
    with pytest.raises(TypeError):
        composite_objects(bg, obj)   # offset is required
    # good arguments on CPU tensors: PfError, still before the library
    for kw in (dict(), dict(scale=0.5, rotation=10.0, edge="hard", samples=2, opacity=0.5, return_coverage=True), dict(objects=f(5, 4, 4)),
               dict(alpha=torch.ones(5, 4, dtype=torch.bool)), dict(backgrounds=[bg, f(9, 9, 3)], objects=[obj, obj], pairs=[(0, 0), (1, 1)], offset=[(1, 2), (3, 4)]),
               dict(scale=torch.ones(()), rotation=torch.zeros(1), offset=torch.zeros(2), size=torch.ones(1, 2)), dict(scale=float("nan"), size=(5, 4)),
               dict(backgrounds=u8(2, 12, 16, 3), objects=u8(5, 4, 3))):
        args = dict(backgrounds=bg, objects=obj, offset=(1, 2))
        args.update(kw)
        with pytest.raises(PfError):
            composite_objects(args.pop("backgrounds"), args.pop("objects"), **args)
    search = dict(best_scale=torch.ones((), dtype=torch.float64), best_rotation_deg=torch.zeros((), dtype=torch.float64), best_variant=torch.zeros((), dtype=torch.int64),
                  best_offset=torch.zeros(2, dtype=torch.int64), best_size=torch.tensor([5, 4]))
    with pytest.raises(PfError):
        PerspectiveFields.composite(None, bg, obj, search)
    with pytest.raises(PfError):
        PerspectiveFields.composite(None, [bg, bg], obj, [search, search], edge="hard")
    for bad in (dict(best_scale=torch.ones(())), [], None, [search, 3]):
        with pytest.raises((ValueError, TypeError)):
            PerspectiveFields.composite(None, bg, obj, bad)
    with pytest.raises(ValueError):
        PerspectiveFields.composite(None, bg, obj, [search, search])   # two rows for one pair
    with pytest.raises(ValueError):
        PerspectiveFields.composite(None, bg, obj, search, opacity=2.0)


def test_composite_kernels_are_in_the_library_without_scratch():
    """scripts/kernel_resources.py on the built library: the three kernels are there for gfx950 with no spilled register, no scratch and no LDS"""
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
    for name in ("pf::composite_prep_kernel", "pf::composite_kernel<float>", "pf::composite_kernel<unsigned char>"):
        r = by[name]
        print(name, {k: r[k] for k in r if k != "kernel"})
        assert r["spill"] == 0 and r["scratch"] == 0 and r["lds"] == 0, r
