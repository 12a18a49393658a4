"""fp64 numpy statement of cube maps as a source (include/pf_hip.h pf_cube_crop / pf_cube_to_pano), built on the conventions of
tests/test_pano_crop_ref.py, tests/test_pano_compose_ref.py and tests/test_reproject_ref.py: the six face cameras, the face and the face coordinate
of a direction, the ring of a face (the unfold rule and the corner mean), the sampler, views and panoramas out of a cube; checks of that reference
against itself; the same formulas in numpy float32 in the order of cube_gather.hip (the rounding floor the GPU results are measured against);
which pixels are left out of accuracy comparisons and how few they are; the fixed inputs of tests/test_gpu_cubemap.py; plus the host-side
contract of crop_cubemap / cubemap_to_panorama / panorama_to_cubemap / the layouts and of the two C entry points (no GPU needed)."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

from tests.test_pano_compose_ref import pano_directions
from tests.test_pano_crop_ref import crop_image, pixel_rays, rotation
from tests.test_pano_rotate_ref import ROTATIONS, _rot_matrix_f32, rot_matrix, rot_rad
from tests.test_reproject_ref import FakeCuda, yaw_matrix

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# ---------------------------------------------------------------- the convention
FACE_NAMES = ("front", "right", "back", "left", "up", "down")
FACE_PITCH_YAW = ((0.0, 0.0), (0.0, 90.0), (0.0, 180.0), (0.0, 270.0), (90.0, 0.0), (-90.0, 0.0))   # degrees; roll 0, rel_focal 0.5
X, Y, Z = np.eye(3)
FRAME_TABLE = ((X, Y, Z), (-Z, Y, X), (-X, Y, -Z), (Z, Y, -X), (X, Z, -Y), (X, -Z, Y))   # (right r, down d, forward n) of face k


def face_camera(k):
    """theta = (roll, pitch, yaw [rad], rel_focal, rel_cx, rel_cy, xi) of face k"""
    p, y = FACE_PITCH_YAW[k]
    return (0.0, np.radians(p), np.radians(y), 0.5, 0.0, 0.0, 0.0)


@functools.lru_cache(None)
def frames():
    """(6, 3, 3) fp64: rows r, d, n of face k, the columns of yaw_matrix(yaw) @ rotation(0, pitch) rounded to the signed permutation they are"""
    out = []
    for k in range(6):
        th = face_camera(k)
        out.append(np.round(yaw_matrix(th[2]) @ rotation(0.0, th[1])).T)
    return np.array(out)


def texel_directions(N):
    """(6, N, N, 3): n + a r + b d of every texel centre, not normalised"""
    t = 2.0 * (np.arange(N) + 0.5) / N - 1.0
    F = frames()
    return F[:, None, None, 2, :] + t[None, None, :, None] * F[:, None, None, 0, :] + t[None, :, None, None] * F[:, None, None, 1, :]


def face_of(D):
    """the face of directions D (..., 3) by the major axis with the tie order z, x, y"""
    ax, ay, az = np.abs(D[..., 0]), np.abs(D[..., 1]), np.abs(D[..., 2])
    fz = (az >= ax) & (az >= ay)
    fx = ~fz & (ax >= ay)
    return np.where(fz, np.where(D[..., 2] < 0, 2, 0), np.where(fx, np.where(D[..., 0] > 0, 1, 3), np.where(D[..., 1] < 0, 4, 5)))


def face_coords(D, N, k=None):
    """directions (..., 3) -> (face, u, v) with texel centres at integers; k: the face to use, default face_of(D)"""
    k = face_of(D) if k is None else k
    F = frames()[k]
    with np.errstate(invalid="ignore", divide="ignore"):
        xn = (D * F[..., 2, :]).sum(-1)
        a, b = (D * F[..., 0, :]).sum(-1) / xn, (D * F[..., 1, :]).sum(-1) / xn
    return k, (a + 1.0) * N / 2 - 0.5, (b + 1.0) * N / 2 - 0.5


def ring_texel(k, N, side, idx):
    """the unfold rule: the (face, row, col) of the ring tap of face k beyond its edge `side` in (+r, -r, +d, -d) = (0, 1, 2, 3), at index idx along
    the other axis.  The direction e + (1 - 1/N) n + t o must be a texel centre of the face whose forward axis is e: asserted"""
    r, d, n = frames()[k]
    e, o = ((r, d), (-r, d), (d, r), (-d, r))[side]
    t = 2.0 * (idx + 0.5) / N - 1.0
    P = e + (1.0 - 1.0 / N) * n + t * o
    k2 = int(np.argmax((frames()[:, 2, :] * e).sum(-1)))
    assert np.array_equal(frames()[k2, 2], e)
    _, u, v = face_coords(P, N, k2)
    assert abs(u - round(u)) <= 1e-12 * N and abs(v - round(v)) <= 1e-12 * N and 0 <= round(u) < N and 0 <= round(v) < N, (k, N, side, idx, u, v)
    return k2, int(round(v)), int(round(u))


def padded_faces(cube):
    """(6, N + 2, N + 2, 3) fp64: every face with its ring (index 0 and N + 1 are the taps -1 and N) and its four corner values"""
    N = cube.shape[1]
    C = cube.astype(np.float64)
    P = np.zeros((6, N + 2, N + 2, 3))
    P[:, 1:-1, 1:-1] = C
    for k in range(6):
        for i in range(N):
            P[k, i + 1, N + 1] = C[ring_texel(k, N, 0, i)]
            P[k, i + 1, 0] = C[ring_texel(k, N, 1, i)]
            P[k, N + 1, i + 1] = C[ring_texel(k, N, 2, i)]
            P[k, 0, i + 1] = C[ring_texel(k, N, 3, i)]
        for rr, rc in ((0, 0), (0, N + 1), (N + 1, 0), (N + 1, N + 1)):
            ir, ic = min(max(rr, 1), N), min(max(rc, 1), N)
            P[k, rr, rc] = (P[k, ir, ic] + P[k, ir, rc] + P[k, rr, ic]) * (1.0 / 3.0)
    return P


def sample_faces(P, k, u, v):
    """bilinear blend of the padded faces P at (face k, u, v), bilerp_rgb's order; 0 where u is not finite"""
    N = P.shape[1] - 2
    ok = np.isfinite(u) & np.isfinite(v)
    u, v = np.where(ok, u, 0.0), np.where(ok, v, 0.0)
    c0 = np.clip(np.floor(u).astype(np.int64), -1, N - 1)
    r0 = np.clip(np.floor(v).astype(np.int64), -1, N - 1)
    fu, fv = (u - c0)[..., None], (v - r0)[..., None]
    top = (1 - fu) * P[k, r0 + 1, c0 + 1] + fu * P[k, r0 + 1, c0 + 2]
    bot = (1 - fu) * P[k, r0 + 2, c0 + 1] + fu * P[k, r0 + 2, c0 + 2]
    return np.where(ok[..., None], (1 - fv) * top + fv * bot, 0.0)


def sample_cube(cube, D, P=None):
    """the cube's value in the directions D (..., 3) in fp64"""
    k, u, v = face_coords(D, cube.shape[1])
    return sample_faces(padded_faces(cube) if P is None else P, k, u, v)


def view_directions(theta, H, W):
    """world directions of the pixel centres of a view (H, W, 3), has_ray (H, W): crop_panorama's ray, turned by Y(yaw) R(roll, pitch)"""
    Xc, ok = pixel_rays(theta, H, W)
    return Xc @ rot_matrix(theta[:3]).T, ok


def pano_out_directions(theta, inverse, H, W):
    """world directions of the pixel centres of the output panorama: rotate_panorama's A D"""
    return pano_directions(H, W) @ rot_matrix(theta, inverse).T


def block_mean(fine, valid, S):
    """the mean over the valid sub-samples of every pixel (0 without one) of a fine grid (S H, S W, C)"""
    H, W = fine.shape[0] // S, fine.shape[1] // S
    f = fine.reshape(H, S, W, S, -1) * valid.reshape(H, S, W, S, 1)
    n = valid.reshape(H, S, W, S).sum((1, 3))
    return np.where((n > 0)[..., None], f.sum((1, 3)) / np.maximum(n, 1)[..., None], 0.0)


def crop_cube(cube, theta, H, W, S=1, P=None):
    """the view in fp64 before any rounding; 0 without a ray, 0 for non-finite parameters"""
    if not np.isfinite(np.asarray(theta, dtype=np.float64)).all():
        return np.zeros((H, W, 3))
    D, ok = view_directions(theta, S * H, S * W)
    return block_mean(np.where(ok[..., None], sample_cube(cube, np.where(ok[..., None], D, 1.0), P), 0.0), ok, S)


def cube_to_pano(cube, theta, inverse, H, W, S=1, P=None):
    if not np.isfinite(np.asarray(theta, dtype=np.float64)).all():
        return np.zeros((H, W, 3))
    return block_mean(sample_cube(cube, pano_out_directions(theta, inverse, S * H, S * W), P), np.ones((S * H, S * W), bool), S)


def pano_to_cube(pano, N):
    """the six crop_panorama faces in fp64"""
    return np.stack([crop_image(pano, face_camera(k), N, N) for k in range(6)])


# ---------------------------------------------------------------- the same formulas in numpy float32, in the order of cube_gather.hip
def coords_f32(Xw, N):
    """float32 world directions (..., 3) -> (face, u, v) float32"""
    f = np.float32
    assert Xw.dtype == f
    k = face_of(Xw)
    x, y, z = Xw[..., 0], Xw[..., 1], Xw[..., 2]
    xr = np.choose(k, [x, -z, -x, z, x, x])
    xd = np.choose(k, [y, y, y, y, z, -z])
    xn = np.choose(k, [np.abs(z), np.abs(x), np.abs(z), np.abs(x), np.abs(y), np.abs(y)])
    hN = f(N) * f(0.5)
    with np.errstate(invalid="ignore", divide="ignore"):
        u, v = xr / xn * hN + (hN - f(0.5)), xd / xn * hN + (hN - f(0.5))
    assert u.dtype == f and v.dtype == f
    return k, u, v


def view_directions_f32(theta, H, W):
    f = np.float32
    r, p, yaw, fo, cx, cy, xi = [f(x) for x in theta]
    Q = _rot_matrix_f32((r, p, yaw), False)
    inv_f = f(1) / (fo * f(H))
    x = (np.arange(W, dtype=f)[None, :] + f(0.5) - (cx + f(0.5)) * f(W)) * inv_f + np.zeros((H, 1), f)
    y = (np.arange(H, dtype=f)[:, None] + f(0.5) - (cy + f(0.5)) * f(H)) * inv_f + np.zeros((1, W), f)
    r2 = x * x + y * y
    disc = f(1) + (f(1) - xi * xi) * r2
    with np.errstate(invalid="ignore"):
        eta = (xi + np.sqrt(np.where(disc >= 0, disc, f(np.nan)))) / (f(1) + r2)
    Xw = np.stack([eta * x, eta * y, eta - xi], -1) @ Q.T
    assert Xw.dtype == f
    return Xw, disc >= 0


def pano_out_directions_f32(theta, inverse, H, W):
    f = np.float32
    A = _rot_matrix_f32(theta, inverse)
    lon = ((np.arange(W, dtype=f) + f(0.5)) / f(W) - f(0.5)) * f(2 * np.pi)
    lat = (f(0.5) - (np.arange(H, dtype=f) + f(0.5)) / f(H)) * f(np.pi)
    lat, lon = np.meshgrid(lat, lon, indexing="ij")
    sl, cl, so, co = np.sin(lat), np.cos(lat), np.sin(lon), np.cos(lon)
    Xw = np.stack([cl * so, -sl, cl * co], -1) @ A.T
    assert Xw.dtype == f
    return Xw


# ---------------------------------------------------------------- the floor, the pixels left out, the allowed error
def compare(D, ok, D32, ok32, N):
    """fp64 directions / has_ray and their float32 evaluation -> (same: both precisions have a ray on the same face, or both have none; the
    coordinate errors |du|, |dv| in texels (0 without a ray); fp64 (k, u, v))"""
    k, u, v = face_coords(np.where(ok[..., None], D, 1.0), N)
    k32, u32, v32 = coords_f32(np.where(ok32[..., None], D32, np.float32(1.0)), N)
    same = (ok == ok32) & (~ok | (k == k32))
    both = same & ok
    return same, np.where(both, np.abs(u32 - u), 0.0), np.where(both, np.abs(v32 - v), 0.0), (k, u, v)


def kept_and_floor(D, ok, D32, ok32, N):
    """the left-out rule: a pixel is compared unless the two evaluations choose different faces (or differ in having a ray) or its fp64 (u, v) lies
    within max(4 x floor, 1e-4) texel of a face border; the floor is the largest coordinate error over the pixels of one face in both precisions"""
    same, du, dv, (k, u, v) = compare(D, ok, D32, ok32, N)
    floor = float(max(du.max(), dv.max()))
    m = max(4.0 * floor, 1e-4)
    border = ok & ((np.abs(u + 0.5) <= m) | (np.abs(u - (N - 0.5)) <= m) | (np.abs(v + 0.5) <= m) | (np.abs(v - (N - 0.5)) <= m))
    return same & ~border, floor, (k, u, v)


def local_steps(P, k, u, v):
    """per pixel, the largest difference between horizontally and between vertically adjacent values of the padded (unfolded) face k in the 4 x 4
    window of taps around the sample (u, v), clipped to the ring"""
    N = P.shape[1] - 2
    c0 = np.clip(np.floor(u).astype(np.int64), -1, N - 1) + 1
    r0 = np.clip(np.floor(v).astype(np.int64), -1, N - 1) + 1
    gu, gv = np.zeros(u.shape), np.zeros(u.shape)
    for dr in range(-1, 3):
        for dc in range(-1, 3):
            r, c = np.clip(r0 + dr, 0, N + 1), np.clip(c0 + dc, 0, N + 1)
            gu = np.maximum(gu, np.abs(P[k, r, np.clip(c + 1, 0, N + 1)] - P[k, r, c]).max(-1))
            gv = np.maximum(gv, np.abs(P[k, np.clip(r + 1, 0, N + 1), c] - P[k, r, c]).max(-1))
    return gu, gv


def image_bound(P, floor, k, u, v):
    """allowed error per pixel of the float32 image: 2 x (coordinate floor x local texel step) + 1e-6 (DESIGN.md section 17's rule)"""
    gu, gv = local_steps(P, k, np.where(np.isfinite(u), u, 0.0), np.where(np.isfinite(v), v, 0.0))
    return 2.0 * floor * (gu + gv) + 1e-6


# ---------------------------------------------------------------- the fixed inputs of the GPU test
CUBE_SIZES = (5, 8, 16, 1)
PANO_OUTPUTS = [(32, 64), (37, 75), (1, 17), (19, 1)]
VIEW_OUTPUTS = [(48, 64), (31, 47), (1, 1)]
CORNER_PITCH = 35.2644   # atan(1 / sqrt 2) in degrees: the elevation of a cube corner
# (roll, pitch, yaw [deg], rel_focal, rel_cx, rel_cy, xi): on the faces, straddling an edge, straddling a corner, principal-point offsets, the mirror.
# The cameras that look along a seam are rolled: with roll 0 the seam is the centre column of an odd width, 1 / 47 of the image on the border
VIEW_CAMERAS = [(0.0, 0.0, 0.0, 0.5, 0.0, 0.0, 0.0), (0.0, 0.0, 90.0, 0.8, 0.0, 0.0, 0.0), (10.0, 90.0, 0.0, 0.6, 0.0, 0.0, 0.0),
                (0.0, -90.0, 30.0, 0.7, 0.0, 0.0, 0.0), (7.0, 0.0, 45.0, 0.9, 0.0, 0.0, 0.0), (-20.0, 0.0, 225.0, 0.5, 0.05, -0.03, 0.0),
                (12.0, CORNER_PITCH, 45.0, 1.1, 0.0, 0.0, 0.0), (15.0, -CORNER_PITCH, 135.0, 0.6, -0.1, 0.08, 0.0), (5.0, 20.0, 300.0, 0.4, 0.0, 0.0, 0.8),
                (-30.0, 50.0, 45.0, 0.3, 0.02, 0.0, 1.2), (25.0, CORNER_PITCH, -45.0, 0.45, 0.0, 0.0, 0.8)]


def view_rad(cam):
    return tuple(np.radians(cam[:3])) + tuple(cam[3:])


def direction_cube(N):
    """a cube whose texel is its own unit direction: smooth, value range 2"""
    D = texel_directions(N)
    return (D / np.linalg.norm(D, axis=-1, keepdims=True)).astype(np.float32)


def u8_cube(N, seed=0):
    """an analytic uint8 cube: three smooth functions of the direction"""
    D = texel_directions(N)
    D = D / np.linalg.norm(D, axis=-1, keepdims=True)
    M = np.random.default_rng(seed).normal(size=(3, 3))
    return np.clip(np.round(127.5 + 100.0 * np.sin(2.0 * (D @ M.T))), 0, 255).astype(np.uint8)


def random_cube(N, seed=0):
    return np.random.default_rng(seed).uniform(0.0, 1.0, (6, N, N, 3)).astype(np.float32)


def smooth_panorama(Hp, Wp):
    """a smooth float32 panorama of value range 2: its pixel is its own direction"""
    return pano_directions(Hp, Wp).astype(np.float32)


@functools.lru_cache(None)
def view_case(cam, out, N):
    """(kept, floor, (k, u, v)) of one view camera (degrees) at one output size and cube size; read only"""
    th = view_rad(cam)
    D, ok = view_directions(th, *out)
    D32, ok32 = view_directions_f32(th, *out)
    return kept_and_floor(D, ok, D32, ok32, N)


@functools.lru_cache(None)
def pano_case(rot, inverse, out, N):
    th = rot_rad(*rot)
    ok = np.ones(out, bool)
    return kept_and_floor(pano_out_directions(th, inverse, *out), ok, pano_out_directions_f32(th, inverse, *out), ok, N)


EDGES = [(a, b) for a in range(6) for b in range(a + 1, 6) if abs((frames()[a, 2] * frames()[b, 2]).sum()) < 0.5]
CORNERS = [(a, b, c) for a in (0, 2) for b in (1, 3) for c in (4, 5)]


def look_at(D):
    """(pitch, yaw) in degrees of a camera with roll 0 whose axis is D: Y(yaw) R(0, pitch) (0, 0, 1) = (cos p sin y, -sin p, cos p cos y)"""
    D = np.asarray(D, dtype=np.float64) / np.linalg.norm(D)
    return float(np.degrees(np.arcsin(-D[1]))), float(np.degrees(np.arctan2(D[0], D[2])))


def edge_direction(a, b):
    return frames()[a, 2] + frames()[b, 2]


def corner_direction(a, b, c):
    return frames()[a, 2] + frames()[b, 2] + frames()[c, 2]


# ---------------------------------------------------------------- the reference against itself
def test_face_frames_are_signed_permutations_and_equal_the_table():
    for k in range(6):
        th = face_camera(k)
        M = yaw_matrix(th[2]) @ rotation(0.0, th[1])
        assert np.abs(M - np.round(M)).max() <= 1e-15
        F = frames()[k]
        assert np.array_equal(np.abs(F).sum(0), np.ones(3)) and np.array_equal(np.abs(F).sum(1), np.ones(3)) and abs(np.linalg.det(F) - 1) <= 1e-15
        for row, want in zip(F, FRAME_TABLE[k]):
            assert np.array_equal(row, want), (k, F)
    assert len(EDGES) == 12 and len(CORNERS) == 8


@pytest.mark.parametrize("N", [1, 2, 5, 8])
def test_every_ring_tap_is_a_texel_of_the_face_beyond_the_edge(N):
    for k in range(6):
        r, d, n = frames()[k]
        for side, e in enumerate((r, -r, d, -d)):
            seen = set()
            for idx in range(N):
                k2, row, col = ring_texel(k, N, side, idx)   # asserts the integer texel
                assert np.array_equal(frames()[k2, 2], e)
                assert row in (0, N - 1) or col in (0, N - 1)   # the first row or column inwards of the neighbour
                seen.add((row, col))
            assert len(seen) == N


@pytest.mark.parametrize("N", [1, 2, 5, 8])
def test_the_face_centre_directions_return_the_cube(N):
    cube = np.random.default_rng(N).uniform(0, 1, (6, N, N, 3))
    D = texel_directions(N)
    assert np.array_equal(face_of(D), np.arange(6)[:, None, None] + np.zeros((N, N), np.int64))
    assert np.abs(sample_cube(cube, D) - cube).max() <= 1e-9


def _seam_directions(N, rng, n=400):
    """directions on the 12 edges and the 8 corners"""
    out = []
    for a, b in EDGES:
        along = np.cross(frames()[a, 2], frames()[b, 2])
        out.append(edge_direction(a, b)[None] + rng.uniform(-1, 1, (n, 1)) * along[None])
    out.append(np.array([corner_direction(*c) for c in CORNERS]))
    return np.concatenate(out)


@pytest.mark.parametrize("N", [1, 2, 5, 8])
def test_the_sampler_is_continuous_on_edges_and_corners(N):
    rng = np.random.default_rng(10 + N)
    cube = rng.uniform(0, 1, (6, N, N, 3))
    P = padded_faces(cube)
    step = max(np.abs(np.diff(P, axis=1)).max(), np.abs(np.diff(P, axis=2)).max())
    D = _seam_directions(N, rng)
    for _ in range(3):
        moved = D + 1e-9 * rng.normal(size=D.shape)
        assert np.abs(sample_cube(cube, moved, P) - sample_cube(cube, D, P)).max() <= step * N * 1e-8
    inside = rng.normal(size=(20000, 3))
    inside /= np.abs(inside).max(-1, keepdims=True)   # on the cube, as the seam directions are
    moved = inside + 1e-9 * rng.normal(size=inside.shape)
    assert np.abs(sample_cube(cube, moved, P) - sample_cube(cube, inside, P)).max() <= step * N * 1e-8


def test_constant_faces_give_the_means_on_edges_and_corners():
    cube = np.arange(6.0)[:, None, None, None] + np.zeros((6, 5, 5, 3))
    P = padded_faces(cube)
    for a, b in EDGES:
        assert np.abs(sample_cube(cube, edge_direction(a, b)[None], P) - (a + b) / 2).max() <= 1e-12
    for c in CORNERS:
        assert np.abs(sample_cube(cube, corner_direction(*c)[None], P) - sum(c) / 3).max() <= 1e-12


def test_a_cube_of_panorama_crops_gives_the_panorama_back():
    """cube faces of N = 48 cut out of a 64 x 128 panorama whose pixel is its direction, turned back into 64 x 128: the error is two bilinear
    interpolations of a unit vector field.  |second derivative| of a unit vector along a tangent coordinate is at most 1 per unit angle; the
    panorama's cell is pi / 64 across at most, the cube's 2 / 48 (tangent units, larger than the angle); a cell of side h adds at most h^2 / 8 per
    axis, two axes each.  A sample with a ring tap has one more term: the unfolded neighbour is flat where the true continuation of the face is
    not, so a ring texel sits up to |t| / N <= 1 / N (tangent units) along the edge from where the face's own grid would continue, and the corner
    value is a mean of texels up to 2 / N away; the field's gradient is at most 1, so 2 / N covers both"""
    N = 48
    pano = pano_directions(64, 128)
    cube = pano_to_cube(pano, N)
    back = cube_to_pano(cube, (0.0, 0.0, 0.0), False, 64, 128)
    bound = 2 * (np.pi / 64) ** 2 / 8 + 2 * (2 / N) ** 2 / 8
    k, u, v = face_coords(pano, N)
    ring = (np.floor(u) < 0) | (np.floor(u) >= N - 1) | (np.floor(v) < 0) | (np.floor(v) >= N - 1)
    err = np.abs(back - pano).max(-1)
    print(f"closure error {err[~ring].max():.3e} (bound {bound:.3e}) without a ring tap, {err[ring].max():.3e} (bound {bound + 2 / N:.3e}) with one")
    assert ring.any() and err[~ring].max() <= bound and err[ring].max() <= bound + 2 / N
    clamped = np.stack([bilinear_clamped(cube[f], u, v) for f in range(6)])   # the same without the ring: worse at the seams
    assert np.abs(np.take_along_axis(clamped, k[None, ..., None], 0)[0] - pano).max(-1)[ring].max() > err[ring].max()


def bilinear_clamped(face, u, v):
    """the per-face clamped sampler the ring replaces"""
    N = face.shape[0]
    u, v = np.clip(u, 0, N - 1), np.clip(v, 0, N - 1)
    c0, r0 = np.minimum(np.floor(u).astype(np.int64), N - 1), np.minimum(np.floor(v).astype(np.int64), N - 1)
    c1, r1 = np.minimum(c0 + 1, N - 1), np.minimum(r0 + 1, N - 1)
    fu, fv = (u - c0)[..., None], (v - r0)[..., None]
    return (1 - fv) * ((1 - fu) * face[r0, c0] + fu * face[r0, c1]) + fv * ((1 - fu) * face[r1, c0] + fu * face[r1, c1])


def test_the_six_face_cameras_see_their_faces():
    for N in (5, 8):
        cube = np.random.default_rng(N).uniform(0, 255, (6, N, N, 3))
        for k in range(6):
            assert np.abs(crop_cube(cube, face_camera(k), N, N) - cube[k]).max() <= 1e-9
    for a, b in EDGES:
        p, y = look_at(edge_direction(a, b))
        D, _ = view_directions((0.0, np.radians(p), np.radians(y), 0.5, 0.0, 0.0, 0.0), 1, 1)
        assert np.abs(np.cross(D[0, 0], edge_direction(a, b))).max() <= 1e-12


# ---------------------------------------------------------------- the float32 floor and the pixels left out
def test_fp32_floor_and_left_out_pixels_of_the_panorama_cases():
    worst, left = 0.0, 0.0
    for N in CUBE_SIZES:
        for out in PANO_OUTPUTS[:2]:
            for rot in ROTATIONS:
                for inverse in (False, True):
                    kept, floor, _ = pano_case(rot, inverse, out, N)
                    worst = max(worst, floor / N)
                    left = max(left, 1.0 - kept.mean())
                    assert kept.mean() >= 0.99, (N, out, rot, inverse, kept.mean())
                    if rot == (0.0, 0.0, 0.0):
                        assert kept.all(), (N, out, inverse)   # the axis-aligned grids have no pixel on a seam
    print(f"panoramas: fp32 floor {worst:.3e} of a face, at most {100 * left:.2f} % left out")
    assert worst <= 2e-6   # of a face: a few ulp of a coordinate in [0, N)
    for N in CUBE_SIZES:   # the one-row and one-column outputs: nothing is left out
        for out in PANO_OUTPUTS[2:]:
            for rot in ROTATIONS:
                for inverse in (False, True):
                    assert pano_case(rot, inverse, out, N)[0].all(), (N, out, rot, inverse)


def test_fp32_floor_and_left_out_pixels_of_the_view_cases():
    worst, left = 0.0, 0.0
    for N in CUBE_SIZES:
        for out in VIEW_OUTPUTS[:2]:
            for cam in VIEW_CAMERAS:
                kept, floor, _ = view_case(cam, out, N)
                worst = max(worst, floor / N)
                left = max(left, 1.0 - kept.mean())
                assert kept.mean() >= 0.99, (N, out, cam, kept.mean())
    print(f"views: fp32 floor {worst:.3e} of a face, at most {100 * left:.2f} % left out")
    assert worst <= 2e-6
    # a 1 x 1 view has one pixel, more than 1 % of itself: it is left out exactly for the cameras that look along a seam, which the seam tests cover
    seam = {cam for cam in VIEW_CAMERAS if cam[2] % 90.0 == 45.0 and cam[1] in (0.0, CORNER_PITCH, -CORNER_PITCH) and cam[4] == 0.0 and cam[5] == 0.0}
    for N in CUBE_SIZES:
        for cam in VIEW_CAMERAS:
            assert view_case(cam, (1, 1), N)[0].all() or cam in seam, (N, cam)


def test_supersampling_is_the_block_mean_of_the_fine_grid():
    cube = random_cube(5, 3)
    P = padded_faces(cube)
    th = view_rad(VIEW_CAMERAS[9])   # xi = 1.2: some pixels have no ray
    fine = crop_cube(cube, th, 24, 32, 1, P)
    _, ok = view_directions(th, 24, 32)
    assert (~ok).any() and ok.any()
    assert np.abs(crop_cube(cube, th, 12, 16, 2, P) - block_mean(fine, ok, 2)).max() <= 1e-12


# ---------------------------------------------------------------- host-side contract (fails before the feature exists)
def test_names_are_exported():
    import perspectivefields_amd

    for name in ("crop_cubemap", "cubemap_to_panorama", "panorama_to_cubemap", "cubemap_face_cameras", "cubemap_to_image", "cubemap_from_image"):
        assert name in perspectivefields_amd.__all__ and callable(getattr(perspectivefields_amd, name))


def test_face_cameras_are_the_table():
    from perspectivefields_amd import cubemap_face_cameras

    cams = cubemap_face_cameras()
    assert sorted(cams) == ["pitch", "rel_focal", "roll", "yaw"]
    assert cams["roll"] == [0.0] * 6 and cams["rel_focal"] == [0.5] * 6
    assert list(zip(cams["pitch"], cams["yaw"])) == list(FACE_PITCH_YAW)
    rad = cubemap_face_cameras("rad")
    assert np.allclose(rad["yaw"], np.radians(cams["yaw"]), atol=0, rtol=1e-15) and rad["rel_focal"] == [0.5] * 6
    with pytest.raises(ValueError):
        cubemap_face_cameras("grad")


def test_header_states_the_convention():
    hdr = open(os.path.join(ROOT, "include", "pf_hip.h")).read()
    assert "int pf_cube_crop(int device, int n_cube, const void* const* h_cube, const int32_t* h_cube_hw" in hdr
    assert "int pf_cube_to_pano(int device, int n_cube, const void* const* h_cube, const int32_t* h_cube_hw" in hdr
    kh = open(os.path.join(ROOT, "perspectivefields_amd", "csrc", "pf_kernels.h")).read()
    assert "struct CubeCropBatch" in kh and "struct CubePanoBatch" in kh and "offsetof(CubePanoBatch, src) == 32" in kh


def test_symbols_and_prototypes_are_present():
    from perspectivefields_amd.engine import _SIGNATURES, declared_symbols, load_library

    assert "pf_cube_crop" in declared_symbols() and "pf_cube_to_pano" in declared_symbols()
    res, args = _SIGNATURES["pf_cube_crop"]
    assert res is ctypes.c_int and len(args) == 13 and args[11] is ctypes.c_int
    res, args = _SIGNATURES["pf_cube_to_pano"]
    assert res is ctypes.c_int and len(args) == 14 and args[8] is ctypes.c_int and args[12] is ctypes.c_int
    lib = load_library()
    assert hasattr(lib, "pf_cube_crop") and hasattr(lib, "pf_cube_to_pano")


@pytest.mark.parametrize("name", ["pf_cube_crop", "pf_cube_to_pano"])
def test_entry_points_reject_bad_arguments_before_device_work(name):
    from perspectivefields_amd.engine import load_library

    lib = load_library()
    cube = (ctypes.c_void_p * 1)(0x1000)
    ints = lambda *s: (ctypes.c_int32 * len(s))(*s)
    dev = ctypes.c_void_p(256)

    def call(hw=None, dtype=0, idx=(0,), c_idx=True, H=4, W=8, img=dev, par=dev, n=1, p=cube, B=None, samples=1):
        head = (0, n, p, hw or ints(8, 8), dtype, len(idx) if B is None else B, ints(*idx) if c_idx else None, par)
        mid = () if name == "pf_cube_crop" else (0,)
        rc = getattr(lib, name)(*head, *mid, H, W, img, samples, None)
        return rc, lib.pf_last_error(None).decode()

    for kw, what in ((dict(idx=(1,)), "index"), (dict(idx=(-1,)), "index"), (dict(dtype=2), "dtype"), (dict(hw=ints(0, 0)), "smaller"), (dict(hw=ints(8, 9)), "square"),
                     (dict(H=0), "size"), (dict(W=0), "size"), (dict(img=None), "required"), (dict(par=None), "required"), (dict(c_idx=False), "required"),
                     (dict(B=0), "required"), (dict(p=(ctypes.c_void_p * 1)()), "NULL"), (dict(p=None), "at least one"), (dict(n=0), "at least one"),
                     (dict(samples=0), "samples"), (dict(samples=5), "samples")):
        rc, msg = call(**kw)
        assert rc == -1 and what in msg and msg.startswith(name + ": "), (kw, rc, msg)
    if not torch.cuda.is_available():   # good arguments fail on the missing device only
        rc, msg = call()
        assert rc == -2 and "no HIP device" in msg, (rc, msg)


def test_cubemap_functions_on_cpu_tensors_raise():
    from perspectivefields_amd import crop_cubemap, cubemap_to_panorama, panorama_to_cubemap
    from perspectivefields_amd.engine import PfError

    cube = torch.zeros((6, 4, 4, 3), dtype=torch.uint8)
    with pytest.raises(PfError):
        crop_cubemap(cube, 0.0, 0.0, 0.5, height=4, width=4)
    with pytest.raises(PfError):
        cubemap_to_panorama([cube], height=4, width=8)
    with pytest.raises(PfError):
        panorama_to_cubemap(torch.zeros((8, 16, 3)), 4)


def test_python_argument_errors_before_the_library_is_loaded(monkeypatch):
    from perspectivefields_amd import engine
    from perspectivefields_amd import perspectivefields as pfm

    def no_library(*a, **k):
        raise AssertionError("the library was loaded before the arguments were checked")

    monkeypatch.setattr(engine, "load_library", no_library)
    monkeypatch.setattr(pfm.torch, "is_tensor", lambda v: isinstance(v, (torch.Tensor, FakeCuda)))
    ok = FakeCuda((6, 8, 8, 3))
    bad_cubes = [FakeCuda((6, 8, 9, 3)), FakeCuda((5, 8, 8, 3)), FakeCuda((6, 8, 8, 4)), FakeCuda((8, 8, 3)), FakeCuda((6, 0, 0, 3)), FakeCuda((6, 8, 8, 3), torch.float16),
                 [ok, FakeCuda((6, 8, 8, 3), torch.float32)], []]
    common = [dict(samples=0), dict(samples=5), dict(samples=2.0), dict(cube_index=[1]), dict(cube_index=[-1]), dict(cube_index=[0, 0]), dict(mode="grad"),
              dict(height=0), dict(width=0)]
    for kw in [dict(cube=c) for c in bad_cubes] + common + [dict(roll=[1.0, 2.0], pitch=[1.0, 2.0, 3.0]), dict(xi=np.zeros((2, 2)))]:
        args = dict(cube=ok, roll=0.0, pitch=0.0, rel_focal=0.5, height=4, width=8)
        args.update(kw)
        with pytest.raises(ValueError):
            pfm.crop_cubemap(args.pop("cube"), args.pop("roll"), args.pop("pitch"), args.pop("rel_focal"), **args)
    for kw in [dict(cube=c) for c in bad_cubes] + common + [dict(roll=[1.0, 2.0], yaw=[1.0, 2.0, 3.0]), dict(yaw=np.zeros((2, 2)))]:
        args = dict(cube=ok, height=4, width=8)
        args.update(kw)
        with pytest.raises(ValueError):
            pfm.cubemap_to_panorama(args.pop("cube"), **args)
    with pytest.raises(TypeError):
        pfm.crop_cubemap([ok, np.zeros((6, 8, 8, 3))], 0.0, 0.0, 0.5, height=4, width=4)
    with pytest.raises(TypeError):
        pfm.cubemap_to_panorama(ok)   # height and width are required
    pano = FakeCuda((8, 16, 3))
    for kw in (dict(pano=FakeCuda((8, 16, 4))), dict(pano=FakeCuda((1, 16, 3))), dict(pano=FakeCuda((8, 16, 3), torch.float16)), dict(pano=[]),
               dict(pano=[pano, FakeCuda((8, 16, 3), torch.float32)]), dict(size=0), dict(samples=0), dict(samples=5), dict(roll=[0.0, 1.0])):
        args = dict(pano=pano, size=4)
        args.update(kw)
        with pytest.raises(ValueError):
            pfm.panorama_to_cubemap(args.pop("pano"), args.pop("size"), **args)


def test_layouts_round_trip_and_reject_bad_names():
    from perspectivefields_amd import cubemap_from_image, cubemap_to_image

    for dtype in (torch.uint8, torch.float32):
        cube = (torch.arange(6 * 3 * 3 * 3).reshape(6, 3, 3, 3) % 251).to(dtype)
        strip = cubemap_to_image(cube, "strip")
        assert strip.shape == (3, 18, 3) and strip.dtype == dtype
        for k in range(6):
            assert torch.equal(strip[:, 3 * k:3 * k + 3], cube[k])
        cross = cubemap_to_image(cube, "cross")
        assert cross.shape == (9, 12, 3)
        for k, (br, bc) in enumerate(((1, 1), (1, 2), (1, 3), (1, 0), (0, 1), (2, 1))):
            assert torch.equal(cross[3 * br:3 * br + 3, 3 * bc:3 * bc + 3], cube[k])
        assert int((cross != 0).sum()) == int((cube != 0).sum())
        for layout, img in (("strip", strip), ("cross", cross)):
            assert torch.equal(cubemap_from_image(img, layout), cube)
        batch = torch.stack([cube, cube.flip(0)])
        assert torch.equal(cubemap_from_image(cubemap_to_image(batch, "cross"), "cross"), batch)
    for call in (lambda: cubemap_to_image(cube, "row"), lambda: cubemap_from_image(strip, "dice"), lambda: cubemap_from_image(strip, "cross"),
                 lambda: cubemap_from_image(cross[:, :11], "cross"), lambda: cubemap_to_image(cube[:5], "strip"), lambda: cubemap_to_image(cube[:, :, :2], "strip")):
        with pytest.raises(ValueError):
            call()


def test_cube_kernels_are_in_the_library_without_scratch():
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
    for name in [f"pf::{k}<{t}>" for k in ("cube_crop_kernel", "cube_to_pano_kernel") for t in ("unsigned char", "float")]:
        r = by[name]
        assert r["spill"] == 0 and r["scratch"] == 0 and r["lds"] <= 128 and r["vgpr"] <= 128, r
