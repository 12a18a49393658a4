"""Drawing of perspective fields (include/pf_hip.h pf_draw_fields, perspectivefields_amd.draw_perspective_fields): the fp64 reference the GPU tests
compare against, known answers of the reference itself, the fixed inputs with a proof that none is borderline, and the host-side contract.  No GPU here.

Model (the header states it once; this is the same in numpy, in the precision `dt`: float64 is the reference, float32 the emulation whose error
sets the GPU tests' tolerance).  Pixel (row, col) has the centre p = (col + 1/2, row + 1/2); v is the picture's value; a pixel is valid when its
field values are finite and the fp32 squared length of its up vector is >= 1e-12 and finite.  1. tint: v <- (1 - alpha) v + alpha ramp(lat) on valid
pixels.  2. lines: g = the gradient of lat (central differences, one-sided next to a non-finite or missing neighbour, 0 without any),
k = step rint(lat / step), d = |lat - k| / |g|, cov = clamp(1/2 + w' / 2 - d, 0, 1) with w' = w, 2 w for k = 0; 0 where invalid or |g| < floor;
v <- (1 - cov) v + cov line colour.  3. arrows: anchors at the pixels (j s + s // 2, i s + s // 2); a valid anchor has the shaft (a, u, L) and the
barbs (a + L u, R(+-25 deg)(-u), 0.35 L); cov = the largest clamp(1/2 + w / 2 - dist, 0, 1) over all segments of all arrows;
v <- (1 - cov) v + cov arrow colour."""
import ast
import ctypes
import functools
import os
import re

import numpy as np
import pytest
import torch

from tests.test_fit_camera_usm_ref import usm_fields
from tests.test_placement_ref import camera_fields, field_valid

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the header's constants (test_header_constants holds them to include/pf_hip.h)
RAMP = ((33.0, 102.0, 172.0), (146.0, 197.0, 222.0), (247.0, 247.0, 247.0), (244.0, 165.0, 130.0), (178.0, 24.0, 43.0))
LINE_RGB = (32.0, 32.0, 32.0)
GRAD_FLOOR = 1e-6
HEAD_ANGLE_DEG, HEAD_COS32, HEAD_SIN32, HEAD_RATIO = 25.0, 0.9063078, 0.42261827, 0.35
CAP = 128   # arrow records per LDS batch (csrc/pf_kernels.h DrawBatch::CAP)


# ---------------------------------------------------------------- the reference
def spacing(H, W, density):
    return max(1, min(H, W) // density)


def anchors(H, W, s):
    """anchor pixels (row, col) in row-major order"""
    return [(r, c) for r in range(s // 2, H, s) for c in range(s // 2, W, s)]


def tint_colour(lat, dt=np.float64):
    """ramp(lat) -> (H, W, 3); lat finite"""
    ramp = np.asarray(RAMP, dtype=dt)
    t = np.clip((lat.astype(dt) + dt(90)) / dt(45), 0, 4)
    fi = np.minimum(np.floor(t), 3)
    f = (t - fi)[..., None]
    i = fi.astype(np.int64)
    return (1 - f) * ramp[i] + f * ramp[i + 1]


def lat_gradient(lat, dt=np.float64):
    """(g_x, g_y) in degrees per pixel; lat may hold non-finite values"""
    la = np.pad(np.asarray(lat).astype(dt), 1, constant_values=np.nan)
    cur = la[1:-1, 1:-1]

    def diff(prev, nxt):
        hp, hn = np.isfinite(prev), np.isfinite(nxt)
        with np.errstate(invalid="ignore"):
            return np.where(hp & hn, (nxt - prev) * dt(0.5), np.where(hn, nxt - cur, np.where(hp, cur - prev, dt(0))))

    return diff(la[1:-1, :-2], la[1:-1, 2:]), diff(la[:-2, 1:-1], la[2:, 1:-1])


def line_coverage(up, lat, step, w, dt=np.float64):
    valid = field_valid(up, lat)
    la = np.where(valid, lat, 0).astype(dt)
    gx, gy = lat_gradient(lat, dt)
    g = np.sqrt(gx * gx + gy * gy)
    level = dt(step) * np.rint(la / dt(step))
    with np.errstate(divide="ignore", invalid="ignore"):
        d = np.abs(la - level) / g
    wl = np.where(level == 0, dt(2) * dt(w), dt(w))
    cov = np.clip(dt(0.5) + dt(0.5) * wl - d, 0, 1)
    return np.where(valid & (g >= dt(np.float32(GRAD_FLOOR))), cov, dt(0))


def arrow_segments(up, r, c, L, dt=np.float64):
    """the three (start x, start y, unit direction x, y, length) of the arrow anchored on the valid pixel (r, c)"""
    ux, uy = dt(up[0, r, c]), dt(up[1, r, c])
    inv = 1 / np.sqrt(ux * ux + uy * uy)
    ex, ey = ux * inv, uy * inv
    ax, ay = dt(c + 0.5), dt(r + 0.5)
    tx, ty = ax + L * ex, ay + L * ey
    if dt is np.float64:
        cs, sn = np.cos(np.radians(HEAD_ANGLE_DEG)), np.sin(np.radians(HEAD_ANGLE_DEG))
    else:
        cs, sn = dt(HEAD_COS32), dt(HEAD_SIN32)
    mx, my = -ex, -ey
    Lb = dt(HEAD_RATIO) * L
    return ((ax, ay, ex, ey, L), (tx, ty, mx * cs - my * sn, mx * sn + my * cs, Lb), (tx, ty, mx * cs + my * sn, my * cs - mx * sn, Lb))


def segment_distance(px, py, seg):
    bx, by, ex, ey, l = seg
    rx, ry = px - bx, py - by
    t = np.clip(rx * ex + ry * ey, 0, l)
    dx, dy = rx - t * ex, ry - t * ey
    return np.sqrt(dx * dx + dy * dy)


def arrow_length(W, arrow_inv_len, dt=np.float64):
    return dt(W) / dt(arrow_inv_len) if dt is np.float64 else np.float32(1.0 / arrow_inv_len) * np.float32(W)   # the C call takes 1 / arrow_inv_len as fp32


def arrow_coverage(up, lat, s, L, w, dt=np.float64, order=None):
    """the largest coverage over all arrows; order: a permutation of the anchors (the result must not depend on it)"""
    H, W = lat.shape
    valid = field_valid(up, lat)
    px, py = (np.arange(W) + 0.5).astype(dt)[None, :], (np.arange(H) + 0.5).astype(dt)[:, None]
    cov = np.zeros((H, W), dtype=dt)
    pts = anchors(H, W, s)
    for k in (range(len(pts)) if order is None else order):
        r, c = pts[k]
        if valid[r, c]:
            for seg in arrow_segments(up, r, c, L, dt):
                cov = np.maximum(cov, np.clip(dt(0.5) + dt(0.5) * dt(w) - segment_distance(px, py, seg), 0, 1))
    return cov


def draw_ref(img, up, lat, *, density=10, arrow_inv_len=20, lat_step_deg=10.0, alpha=0.5, arrow_color=(0, 255, 0), line_width=1.0, draw_up=True,
             draw_lat=True, dt=np.float64, order=None):
    """the value of every output pixel before the conversion to the picture's type, (H, W, 3) in `dt`"""
    v = np.asarray(img).astype(dt)
    H, W = lat.shape
    if draw_lat:
        valid = field_valid(up, lat)[..., None]
        v = np.where(valid, (1 - dt(alpha)) * v + dt(alpha) * tint_colour(np.where(valid[..., 0], lat, 0), dt), v)
        cov = line_coverage(up, lat, lat_step_deg, line_width, dt)[..., None]
        v = (1 - cov) * v + cov * np.asarray(LINE_RGB, dtype=dt)
    if draw_up:
        cov = arrow_coverage(up, lat, spacing(H, W, density), arrow_length(W, arrow_inv_len, dt), line_width, dt, order)[..., None]
        v = (1 - cov) * v + cov * np.asarray(arrow_color, dtype=dt)
    assert v.dtype == dt
    return v


def to_u8(v):
    return np.clip(np.floor(v + 0.5), 0, 255).astype(np.uint8)


# ---------------------------------------------------------------- fixed inputs (shared with tests/test_gpu_draw_fields.py)
CAM = (8.0, 20.0, 60.0)
SET_NAMES = "ABCDEFGH"


def picture(H, W):
    """float32 (H, W, 3) on the 0 - 255 scale: 127.5 + 110 sin(fx col + fy row + channel)"""
    rows, cols = np.meshgrid(np.arange(H) + 0.5, np.arange(W) + 0.5, indexing="ij")
    return np.stack([127.5 + 110.0 * np.sin(fx * cols + fy * rows + k) for k, (fx, fy) in enumerate(((0.31, 0.07), (0.05, 0.29), (0.23, 0.19)))], -1).astype(np.float32)


@functools.lru_cache(None)
def draw_set(name):
    """(up, lat, options) of the sets A - H, read only"""
    kw = {}
    if name in ("A", "D"):
        up, lat = camera_fields(*CAM, 40, 56)
        if name == "D":
            lat = np.array(lat)
            lat[10:15, :] = np.nan
            lat[:6, :6] = np.nan
    elif name == "B":
        up, lat = camera_fields(-30.0, -10.0, 60.0, 37, 53)
    elif name == "C":
        (up, lat), kw = camera_fields(*CAM, 24, 83), dict(arrow_inv_len=4)
    elif name in ("E", "H"):
        (up, lat), kw = camera_fields(*CAM, 16, 16), dict(density=16)
        if name == "H":   # E draws every pixel's own arrow over it; with holes a pixel is covered by its neighbours' arrows, of either batch of records
            lat = np.array(lat)
            rows, cols = np.mgrid[0:16, 0:16]
            lat[(3 * rows + 5 * cols) % 7 == 0] = np.nan
    elif name == "F":
        (up, lat), kw = camera_fields(*CAM, 8, 8), dict(density=1)
    elif name == "G":   # Unified Spherical Model, xi = 1.2: no ray beyond 27 pixels from the centre
        up, lat = usm_fields((np.radians(8.0), np.radians(20.0), 0.45, 0.0, 0.0, 1.2), 40, 56)
        up, lat = np.ascontiguousarray(up).astype(np.float32), np.ascontiguousarray(lat).astype(np.float32)
    else:
        raise KeyError(name)
    for a in (up, lat):
        a.setflags(write=False)
    return up, lat, kw


@functools.lru_cache(None)
def set_picture(name, dtype):
    H, W = draw_set(name)[1].shape
    img = picture(H, W)
    img = to_u8(img.astype(np.float64)) if dtype == "uint8" else img
    img.setflags(write=False)
    return img


@functools.lru_cache(None)
def set_reference(name, dtype):
    """the fp64 value of every output pixel for the set's picture in `dtype`"""
    up, lat, kw = draw_set(name)
    v = draw_ref(set_picture(name, dtype), up, lat, **kw)
    v.setflags(write=False)
    return v


@functools.lru_cache(None)
def fp32_floor(name, dtype="float32"):
    """largest error of the same formulas in numpy float32 against the fp64 reference, in units of the picture"""
    up, lat, kw = draw_set(name)
    return float(np.abs(draw_ref(set_picture(name, dtype), up, lat, dt=np.float32, **kw).astype(np.float64) - set_reference(name, dtype)).max())


# ---------------------------------------------------------------- known answers of the reference
def test_header_constants():
    hdr = open(os.path.join(ROOT, "include", "pf_hip.h")).read()

    def macro(name):
        text = re.search(rf"#define {name} (.*)", hdr).group(1).split("/*")[0]
        return ast.literal_eval(re.sub(r"(\d)\.?f\b", r"\1", text).replace("{", "(").replace("}", ")"))

    assert macro("PF_DRAW_RAMP") == RAMP and macro("PF_DRAW_LINE_RGB") == LINE_RGB
    assert macro("PF_DRAW_GRAD_FLOOR") == GRAD_FLOOR and macro("PF_DRAW_HEAD_ANGLE_DEG") == HEAD_ANGLE_DEG and macro("PF_DRAW_HEAD_RATIO") == HEAD_RATIO
    assert macro("PF_DRAW_HEAD_COS") == HEAD_COS32 and macro("PF_DRAW_HEAD_SIN") == HEAD_SIN32
    assert np.float32(HEAD_COS32) == np.float32(np.cos(np.radians(HEAD_ANGLE_DEG))) and np.float32(HEAD_SIN32) == np.float32(np.sin(np.radians(HEAD_ANGLE_DEG)))
    assert macro("PF_DRAW_UP") == 1 and macro("PF_DRAW_LAT") == 2
    kh = open(os.path.join(ROOT, "perspectivefields_amd", "csrc", "pf_kernels.h")).read()
    assert f"static constexpr int CAP = {CAP};  // arrow records per LDS batch" in kh


def test_ramp_is_light_at_the_horizon_and_goes_through_its_control_points():
    lat = np.array([[-90.0, -45.0, 0.0, 45.0, 90.0, -120.0, 200.0, 22.5]])
    c = tint_colour(lat)[0]
    assert np.array_equal(c[:5], np.asarray(RAMP)) and np.array_equal(c[5], RAMP[0]) and np.array_equal(c[6], RAMP[4])
    assert np.allclose(c[7], (np.asarray(RAMP[2]) + np.asarray(RAMP[3])) / 2)
    assert c[2].sum() == max(sum(p) for p in RAMP)


def test_an_upright_camera_has_arrows_that_point_to_the_top():
    up, lat = camera_fields(0.0, 0.0, 60.0, 40, 56)
    s, L = spacing(40, 56, 10), arrow_length(56, 20)
    assert s == 4 and L == 2.8 and len(anchors(40, 56, s)) == 10 * 14 and anchors(40, 56, s)[0] == (2, 2)
    for r, c in anchors(40, 56, s):
        shaft, barb1, barb2 = arrow_segments(up, r, c, L)
        assert (shaft[0], shaft[1]) == (c + 0.5, r + 0.5) and abs(barb1[0] - shaft[0]) < 1e-6 and abs(barb1[1] - (shaft[1] - L)) < 1e-6   # the tip, above
        assert barb1[3] > 0 and barb2[3] > 0 and barb1[2] * barb2[2] < 0   # both barbs run back down, one to each side
    cov = arrow_coverage(up, lat, s, L, 1.0)
    assert cov[1, 2] == 1.0 and cov[2, 2] == 1.0 and cov[38, 2] == 1.0 and cov[39, 2] == 0.0 and cov.max() == 1.0   # on a shaft; below the last anchor


def test_segment_form_equals_the_end_point_form():
    up, lat, _ = draw_set("B")
    rng = np.random.default_rng(0)
    p = rng.uniform(-5, 60, (200, 2))
    for seg in arrow_segments(up, 10, 13, 7.5):
        b, e = np.array(seg[:2]), np.array(seg[:2]) + seg[4] * np.array(seg[2:4])
        t = np.clip(((p - b) @ (e - b)) / ((e - b) @ (e - b)), 0, 1)
        want = np.linalg.norm(p - (b + t[:, None] * (e - b)), axis=1)
        assert np.abs(segment_distance(p[:, 0], p[:, 1], seg) - want).max() < 1e-12
    barb = arrow_segments(up, 10, 13, 7.5)[1]
    shaft = arrow_segments(up, 10, 13, 7.5)[0]
    assert abs(np.degrees(np.arccos(-(barb[2] * shaft[2] + barb[3] * shaft[3]))) - HEAD_ANGLE_DEG) < 1e-9 and abs(barb[4] - HEAD_RATIO * 7.5) < 1e-12


def test_iso_lines_lie_on_the_rows_of_the_levels():
    H, W = 41, 12
    lat = np.repeat(np.arange(H, dtype=np.float32)[:, None] - 20.0, W, 1)   # one degree per row, the horizon on row 20
    up = np.stack([np.zeros((H, W), np.float32), -np.ones((H, W), np.float32)])
    cov = line_coverage(up, lat, 10.0, 1.0)
    assert (cov == cov[:, :1]).all()
    col = cov[:, 0]
    for r in (0, 10, 30, 40):
        assert col[r] == 1.0 and (r == 0 or col[r - 1] == 0.0) and (r == 40 or col[r + 1] == 0.0)
    assert col[20] == 1.0 and col[19] == 0.5 and col[21] == 0.5 and col[18] == 0.0 and col[22] == 0.0   # twice as wide
    assert col.sum() == 4 * 1.0 + 2.0 and (col[[2, 8, 12, 28, 32, 38]] == 0.0).all()
    img = picture(H, W)
    v = draw_ref(img, up, lat, alpha=0.0, draw_up=False)
    assert np.array_equal(v[10], np.broadcast_to(LINE_RGB, (W, 3))) and np.array_equal(v[12], img[12].astype(np.float64))


def test_gradient_is_one_sided_next_to_a_missing_neighbour():
    lat = np.array([[0.0, 1.0, 3.0, np.nan, 10.0], [2.0, 4.0, np.nan, np.nan, np.inf]])
    gx, gy = lat_gradient(lat)
    assert np.array_equal(gx[0, :3], [1.0, 1.5, 2.0]) and gx[0, 4] == 0.0 and gx[1, 1] == 2.0
    assert np.array_equal(gy[:, 0], [2.0, 2.0]) and gy[0, 2] == 0.0 and gy[0, 4] == 0.0


def test_nothing_to_draw_returns_the_image():
    up, lat, kw = draw_set("A")
    for dtype in ("uint8", "float32"):
        img = set_picture("A", dtype)
        assert np.array_equal(draw_ref(img, up, lat, draw_up=False, draw_lat=False, **kw), img.astype(np.float64))
        assert np.array_equal(draw_ref(img, up, np.full_like(lat, np.nan), **kw), img.astype(np.float64))
        assert np.array_equal(draw_ref(img, np.zeros_like(up), lat, **kw), img.astype(np.float64))
    assert np.array_equal(to_u8(set_picture("A", "uint8").astype(np.float64)), set_picture("A", "uint8"))


def test_the_maximum_over_arrows_does_not_depend_on_their_order():
    for name in ("C", "E"):
        up, lat, kw = draw_set(name)
        n = len(anchors(*lat.shape, spacing(*lat.shape, kw.get("density", 10))))
        order = np.random.default_rng(3).permutation(n)
        for dt in (np.float64, np.float32):
            a = draw_ref(set_picture(name, "float32"), up, lat, dt=dt, **kw)
            assert np.array_equal(a, draw_ref(set_picture(name, "float32"), up, lat, dt=dt, order=order, **kw))


# ---------------------------------------------------------------- the fixed inputs, and that none is borderline
@pytest.mark.parametrize("name", SET_NAMES)
def test_no_fixed_input_is_borderline(name):
    up, lat, kw = draw_set(name)
    H, W = lat.shape
    valid = field_valid(up, lat)
    assert up.dtype == np.float32 and lat.dtype == np.float32 and valid.any()
    gx, gy = lat_gradient(lat)
    g = np.sqrt(gx * gx + gy * gy)
    assert g[valid].min() >= 100 * GRAD_FLOOR, g[valid].min()
    l2 = (up.astype(np.float64) ** 2).sum(0)
    ok = np.isfinite(l2)
    assert ((np.abs(l2[ok] - 1.0) < 1e-5) | (l2[ok] == 0.0)).all()   # every length is 1 or exactly 0: validity is never decided by a rounding
    assert not np.isinf(lat).any() and not np.isinf(up).any()
    # an anchor's arrow exists or not by the same clear margin, and so for its neighbours: a one-pixel shift of the mask moves no arrow silently
    for r, c in anchors(H, W, spacing(H, W, kw.get("density", 10))):
        assert valid[r, c] == (np.isfinite(lat[r, c]) and np.isfinite(l2[r, c]) and l2[r, c] > 0.5)
    # the level a pixel belongs to changes its line width only between 0 and +-step, at |lat| = step / 2; no pixel whose line could reach that far sits on the tie
    step, w = kw.get("lat_step_deg", 10.0), kw.get("line_width", 1.0)
    tie = np.abs(np.abs(np.where(valid, lat, 0).astype(np.float64)) - step / 2) < 1e-3 * step
    assert not (tie & valid & (g * (0.5 + w) >= 0.99 * step / 2)).any()
    # the colour ramp and the clamps are continuous: nothing else is decided by a comparison of computed values
    floor = fp32_floor(name)
    print(f"set {name}: {H} x {W}, {int(valid.sum())} valid pixels, |g| in [{g[valid].min():.3f}, {g[valid].max():.3f}] deg/px, float32 emulation error {floor:.3e}")
    assert 0 < floor < 0.05 or (name == "E" and floor == 0.0)   # E: every pixel lies on its own anchor and is the arrow colour exactly


def test_the_sets_exercise_what_they_are_for():
    sp = lambda n: spacing(*draw_set(n)[1].shape, draw_set(n)[2].get("density", 10))
    assert [sp(n) for n in SET_NAMES] == [4, 3, 2, 4, 1, 8, 4, 1]
    assert len(anchors(16, 16, 1)) == 256 > CAP and anchors(8, 8, 8) == [(4, 4)]   # E: two batches of records; F: one arrow
    assert arrow_length(83, 4) > 64 / 4 and arrow_length(83, 4) > 5 * sp("C")   # C: arrows several cells long
    up, lat, kw = draw_set("C")
    tips = [arrow_segments(up, r, c, arrow_length(83, 4))[1][:2] for r, c in anchors(24, 83, 2)]
    assert any(t[1] < 0 for t in tips) and any(a[1] >= 64 > t[0] for a, t in zip(anchors(24, 83, 2), tips))   # leave the image; cross column 64
    assert np.array_equal(set_reference("E", "float32"), np.broadcast_to((0.0, 255.0, 0.0), (16, 16, 3)))
    v = field_valid(*draw_set("H")[:2])
    assert not v[7, 0] and not v[8, 5] and v[8, 0] and v[9, 5] and 30 < (~v).sum() < 45   # holes whose cover comes from the other batch's arrows
    cov = arrow_coverage(*draw_set("H")[:2], 1, arrow_length(16, 20), 1.0)
    assert 0.5 < cov[7, 0] < 1.0 and cov[v].min() == 1.0
    for name in ("D", "G"):
        v = field_valid(*draw_set(name)[:2])
        assert 0.05 < (~v).mean() < 0.6 and any(not v[r, c] for r, c in anchors(40, 56, 4)) and any(v[r, c] for r, c in anchors(40, 56, 4))
    v = field_valid(*draw_set("D")[:2])
    assert not v[10:15].any() and not v[:6, :6].any() and v[9].all() and v[15].all()
    up, lat, _ = draw_set("A")
    assert any(r > 16 > arrow_segments(up, r, c, 2.8)[1][1] for r, c in anchors(40, 56, 4))   # A: an arrow across the tile boundary at row 16


# ---------------------------------------------------------------- host-side contract (fails before the feature exists)
def test_exports():
    import perspective2d
    import perspective2d.utils
    import perspectivefields_amd

    for name in ("draw_perspective_fields", "draw_camera"):
        assert name in perspectivefields_amd.__all__ and callable(getattr(perspectivefields_amd, name)) and callable(getattr(perspective2d, name))
    assert callable(perspectivefields_amd.PerspectiveFields.draw_fields)
    assert callable(perspective2d.utils.draw_perspective_fields) and callable(perspective2d.utils.draw_from_r_p_f_cx_cy)


def test_symbols_and_prototypes():
    from perspectivefields_amd.engine import _SIGNATURES, declared_symbols, load_library

    hdr = open(os.path.join(ROOT, "include", "pf_hip.h")).read()
    assert "int pf_draw_fields(int device, int batch, const int32_t* h_hw /*[batch][2]*/, const void* const* h_img, const float* const* h_up," in hdr
    assert "size_t pf_draw_fields_workspace_bytes(int batch, const int32_t* h_hw /*[batch][2]*/, int spacing);" in hdr
    assert {"pf_draw_fields", "pf_draw_fields_workspace_bytes"} <= set(declared_symbols())
    res, args = _SIGNATURES["pf_draw_fields"]
    assert res is ctypes.c_int and len(args) == 18 and args[16] is ctypes.c_size_t and args[9:13] == [ctypes.c_float] * 4
    res, args = _SIGNATURES["pf_draw_fields_workspace_bytes"]
    assert res is ctypes.c_size_t and len(args) == 3
    lib = load_library()
    assert hasattr(lib, "pf_draw_fields") and hasattr(lib, "pf_draw_fields_workspace_bytes")


def test_pf_draw_fields_rejects_bad_arguments_before_device_work():
    from perspectivefields_amd.engine import load_library

    lib = load_library()
    ints = lambda *s: (ctypes.c_int32 * len(s))(*s)
    ptrs = lambda n: (ctypes.c_void_p * n)(*([0x1000] * n))
    null2 = (ctypes.c_void_p * 2)(0x1000, 0)
    rgb = (ctypes.c_float * 3)(0.0, 255.0, 0.0)
    dev = ctypes.c_void_p(4096)

    def call(batch=2, hw="ok", img="ok", up="ok", lat="ok", out="ok", dtype=0, spacing=4, length=0.05, step=10.0, alpha=0.5, width=1.0, colour=rgb, layers=3,
             ws=dev, ws_bytes=None):
        hw = ints(40, 56, 37, 53) if hw == "ok" else hw
        if ws_bytes is None:
            ws_bytes = lib.pf_draw_fields_workspace_bytes(batch, hw, spacing)
        arr = lambda v: ptrs(max(batch, 1)) if v == "ok" else v
        rc = lib.pf_draw_fields(0, batch, hw, arr(img), arr(up), arr(lat), arr(out), dtype, spacing, length, step, alpha, width, colour, layers, ws, ws_bytes, None)
        return rc, lib.pf_last_error(None).decode()

    need = lib.pf_draw_fields_workspace_bytes(2, ints(40, 56, 37, 53), 4)
    assert need >= 64 * (10 * 14 + 9 * 13) and need == lib.pf_draw_fields_workspace_bytes(2, ints(40, 56, 37, 53), 4)
    assert lib.pf_draw_fields_workspace_bytes(1, ints(16, 16), 1) >= 64 * 256 and lib.pf_draw_fields_workspace_bytes(1, ints(8, 8), 100) == 256
    for args in ((0, ints(40, 56), 4), (-1, ints(40, 56), 4), (1, None, 4), (1, ints(0, 56), 4), (1, ints(40, -1), 4), (2, ints(40, 56, 37, 0), 4),
                 (1, ints(40, 56), 0), (1, ints(40, 56), -2), (1, ints(65536, 65536), 4)):
        assert lib.pf_draw_fields_workspace_bytes(*args) == 0, args
    nan, inf = float("nan"), float("inf")
    for kw, what in ((dict(batch=0), "batch"), (dict(batch=-3), "batch"), (dict(hw=None), "h_hw"), (dict(hw=ints(40, 0, 37, 53)), "smaller"),
                     (dict(hw=ints(40, 56, -1, 53)), "smaller"), (dict(hw=ints(65536, 65536, 37, 53)), "2^31"), (dict(spacing=0), "spacing"),
                     (dict(spacing=-1), "spacing"), (dict(step=0.0), "lat_step_deg"), (dict(step=-10.0), "lat_step_deg"), (dict(step=nan), "lat_step_deg"),
                     (dict(step=inf), "lat_step_deg"), (dict(alpha=-0.01), "alpha"), (dict(alpha=1.01), "alpha"), (dict(alpha=nan), "alpha"),
                     (dict(dtype=2), "dtype"), (dict(dtype=-1), "dtype"), (dict(layers=4), "layers"), (dict(layers=-1), "layers"),
                     (dict(length=-0.1), "arrow_len_rel"), (dict(length=nan), "arrow_len_rel"), (dict(length=inf), "arrow_len_rel"),
                     (dict(width=-1.0), "line_width"), (dict(width=nan), "line_width"), (dict(colour=(ctypes.c_float * 3)(0.0, nan, 0.0)), "h_arrow_rgb"),
                     (dict(colour=None), "required"), (dict(img=None), "required"), (dict(up=None), "required"), (dict(lat=None), "required"),
                     (dict(out=None), "required"), (dict(img=null2), "NULL"), (dict(up=null2), "NULL"), (dict(lat=null2), "NULL"), (dict(out=null2), "NULL"),
                     (dict(ws=None, ws_bytes=need), "workspace"), (dict(ws_bytes=need - 1), "workspace"), (dict(ws_bytes=0), "workspace")):
        rc, msg = call(**kw)
        assert rc == -1 and what in msg and msg.startswith("pf_draw_fields: "), (kw, rc, msg)
    if not torch.cuda.is_available():   # good arguments pass the checks and fail on the missing device only; without arrows no workspace is asked for
        for kw in ({}, dict(layers=2, ws=None, ws_bytes=0), dict(layers=0, ws=None, ws_bytes=0), dict(dtype=1), dict(alpha=0.0), dict(alpha=1.0), dict(length=0.0)):
            rc, msg = call(**kw)
            assert rc == -2 and "no HIP device" in msg, (kw, rc, msg)


def test_python_argument_errors_without_a_gpu():
    from perspectivefields_amd import PerspectiveFields, draw_camera, draw_perspective_fields
    from perspectivefields_amd.engine import PfError

    f = lambda *s: torch.zeros(s)
    img, up, lat = torch.zeros((12, 16, 3), dtype=torch.uint8), f(2, 12, 16), f(12, 16)
    for kw in (dict(up=f(2, 12, 15), lat=f(12, 15)), dict(up=f(2, 13, 16), lat=f(13, 16)), dict(lat=f(12, 15)), dict(up=f(3, 12, 16)), dict(up=f(12, 16)),
               dict(images=torch.zeros((2, 12, 16, 3), dtype=torch.uint8)), dict(images=[img, img]), dict(images=[img, img], up=[up, up], lat=[lat]),
               dict(images=[img], up=[up, up], lat=[lat, lat]), dict(images=torch.zeros((2, 12, 16, 3), dtype=torch.uint8), up=f(3, 2, 12, 16), lat=f(3, 12, 16)),
               dict(images=[], up=[], lat=[]), dict(density=0), dict(density=-2), dict(arrow_inv_len=0), dict(arrow_inv_len=float("nan")), dict(lat_step_deg=0.0),
               dict(lat_step_deg=float("inf")), dict(alpha=1.5), dict(alpha=-0.5), dict(line_width=-1.0), dict(arrow_color=(0, 255)),
               dict(arrow_color=(0.0, float("nan"), 0.0))):
        args = dict(images=img, up=up, lat=lat)
        args.update(kw)
        with pytest.raises(ValueError):
            draw_perspective_fields(args.pop("images"), args.pop("up"), args.pop("lat"), **args)
    with pytest.raises(TypeError):
        draw_perspective_fields(img, up, [lat])
    with pytest.raises(TypeError):
        draw_perspective_fields(img.numpy(), up, lat)
    with pytest.raises(TypeError):
        draw_perspective_fields(img, up, lat, density=2.5)
    # good arguments on the CPU: no CPU path
    for args in ((img, up, lat), ([img, img], [up, up], [lat, lat]), (torch.zeros((2, 12, 16, 3)), f(2, 2, 12, 16), f(2, 12, 16))):
        with pytest.raises(PfError):
            draw_perspective_fields(*args)
    with pytest.raises(PfError):
        draw_perspective_fields(img, up, lat, density=3, draw_up=False, out=torch.zeros_like(img))
    pred = dict(pred_gravity_original=up, pred_latitude_original=lat)
    with pytest.raises(PfError):
        PerspectiveFields.draw_fields(None, [img, img], [pred, pred])
    with pytest.raises(ValueError):
        PerspectiveFields.draw_fields(None, img, dict(pred_gravity_original=f(2, 5, 4), pred_latitude_original=f(5, 4)))
    with pytest.raises(PfError):
        draw_camera(img, 0.0, 10.0, 0.8)


def test_draw_kernels_are_in_the_library_without_scratch():
    """scripts/kernel_resources.py on the built library: the three kernels are there for gfx950 with no spilled register and no scratch; the tile
    kernel's LDS is one batch of records"""
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
    for name, lds in (("pf::draw_arrows_kernel", 0), ("pf::draw_fields_kernel<float>", 64 * CAP), ("pf::draw_fields_kernel<unsigned char>", 64 * CAP)):
        r = by[name]
        print(name, {k: r[k] for k in r if k != "kernel"})
        assert r["spill"] == 0 and r["scratch"] == 0 and r["lds"] <= lds, r
