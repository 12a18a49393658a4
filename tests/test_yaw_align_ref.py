"""fp64 numpy statement of the yaw alignment of camera views of one centre (include/pf_hip.h pf_yaw_moments), built on the
camera model of tests/test_pano_crop_ref.py and tests/test_reproject_ref.py: the samples of b, their points in a, coverage, luminance, the six
moments, the zero-mean normalised cross-correlation, the peak with its parabola and the spanning tree; the same coordinates in numpy float32
(the rounding floor the GPU moments are judged against); the fixed inputs of tests/test_gpu_yaw_align.py; checks that the reference recovers
the true yaws of those inputs; plus the host-side contract of yaw_scores / align_yaw / pf_yaw_moments (no GPU needed)."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

from tests.test_pano_crop_ref import crop_image, intrinsics, pixel_rays, project, rotation
from tests.test_reproject_ref import FakeCuda, sample, source_coords, theta_rad, yaw_matrix, z_min

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE = 1024   # samples one thread of the moments kernel adds (csrc/pf_kernels.h YawBatch::TILE)
MIN_OVERLAP, MIN_SCORE = 0.1, 0.8
VAR_FLOOR = 2.0 ** -16


# ---------------------------------------------------------------- the model
def luminance(img):
    """(H, W, 3) uint8 or float -> the fp64 plane L = 0.299 c0 + 0.587 c1 + 0.114 c2 - c, c = 127.5 for uint8 and 0.5 otherwise"""
    P = img.astype(np.float64)
    return 0.299 * P[..., 0] + 0.587 * P[..., 1] + 0.114 * P[..., 2] - value_range(img)


def value_range(img):
    """V: the largest |L| of an image of this type"""
    return 127.5 if img.dtype == np.uint8 else 0.5


def sample_rays(tb, Hb, Wb, stride):
    """world rays W = R_b X_b (S, 3) of the samples of b (row % stride == 0 and col % stride == 0, row-major), has_ray (S,), rows, cols (S,)"""
    X, ok = pixel_rays(tb, Hb, Wb)
    X, ok = X[::stride, ::stride], ok[::stride, ::stride]
    rows, cols = np.meshgrid(np.arange(0, Hb, stride), np.arange(0, Wb, stride), indexing="ij")
    return X.reshape(-1, 3) @ rotation(tb[0], tb[1]).T, ok.reshape(-1), rows.reshape(-1), cols.reshape(-1)


def pair_points(ta, Ha, Wa, tb, Hb, Wb, stride, cand):
    """theta = (roll, pitch, yaw [rad, unused], rel_focal, rel_cx, rel_cy, xi) of a and b, candidates (K,) in radians -> the samples' points
    (p, q) (K, S) in a in pixel-edge units, `covered` (K, S), X_a.z (K, S) and has_ray (S,)"""
    W, ok, _, _ = sample_rays(tb, Hb, Wb, stride)
    Y = np.stack([yaw_matrix(d) for d in cand])               # (K, 3, 3)
    Xa = np.einsum("ij,kjl,sl->ksi", rotation(ta[0], ta[1]).T, Y, np.where(ok[:, None], W, np.nan))
    F, Cx, Cy = intrinsics(ta[3], ta[4], ta[5], Ha, Wa)
    with np.errstate(invalid="ignore", divide="ignore"):
        vis = Xa[..., 2] > z_min(ta[6])
        xy = project(Xa, ta[6])
        p, q = F * xy[..., 0] + Cx, F * xy[..., 1] + Cy
        covered = vis & (p > 0) & (Wa - p > 0) & (q > 0) & (Ha - q > 0)
    return p, q, covered, Xa[..., 2], ok


def band(ta, Ha, Wa, p, q, z):
    """the samples whose fp32 and fp64 coverage may legitimately differ: the point within 1 px of a's image and either within 1e-2 px of
    a's border or within 1e-3 of z_min (the band of tests/test_reproject_ref.clear)"""
    with np.errstate(invalid="ignore"):
        close = (p >= -1) & (p <= Wa + 1) & (q >= -1) & (q <= Ha + 1)
        edge = (np.abs(p) <= 1e-2) | (np.abs(p - Wa) <= 1e-2) | (np.abs(q) <= 1e-2) | (np.abs(q - Ha) <= 1e-2)
        return close & (edge | (np.abs(z - z_min(ta[6])) <= 1e-3))


def sample_plane(L, p, q, covered):
    """clamped bilinear sample of the plane L at (p - 1/2, q - 1/2), 0 where not covered: tests/test_reproject_ref.sample on one channel"""
    return sample(L[..., None], p, q, covered, 0.0)[..., 0]


def moments_of(x, y, covered):
    """(K, 6): n, sum x, sum y, sum x^2, sum y^2, sum xy over the covered samples; x (K, S), y (S,)"""
    c = covered.astype(np.float64)
    yy = y[None, :] * c
    return np.stack([c.sum(1), (x * c).sum(1), yy.sum(1), (x * x * c).sum(1), (yy * yy).sum(1), (x * yy).sum(1)], 1)


def zncc(M, rays, min_overlap=MIN_OVERLAP):
    """moments (..., 6) and the samples of b with a ray -> the score, -inf where n < min_overlap x rays or a variance is not positive: not above
    2^-16 of n x its sum of squares, under which sums kept in float32 cannot tell it from 0"""
    n, sx, sy, sxx, syy, sxy = np.moveaxis(np.asarray(M, dtype=np.float64), -1, 0)
    va, vb = n * sxx - sx * sx, n * syy - sy * sy
    ok = (n >= min_overlap * rays) & (va > VAR_FLOOR * n * sxx) & (vb > VAR_FLOOR * n * syy)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(ok, (n * sxy - sx * sy) / np.sqrt(np.where(ok, va * vb, 1.0)), -np.inf)


def wrap180(x):
    return (np.asarray(x, dtype=np.float64) + 180.0) % 360.0 - 180.0


def peak_of(score, cand_deg, refine=True):
    """(index of the best candidate, its score, the turn in degrees: the candidate, moved by the vertex of the parabola through the peak and
    its circular neighbours unless one of them is -inf)"""
    K = len(score)
    k = int(np.argmax(score))
    z0, zm, zp = score[k], score[(k - 1) % K], score[(k + 1) % K]
    step = cand_deg[1] - cand_deg[0] if K > 1 else 0.0
    off = 0.0
    if refine and K >= 3 and np.isfinite([z0, zm, zp]).all() and zm - 2 * z0 + zp < 0:
        off = 0.5 * (zm - zp) / (zm - 2 * z0 + zp)
    return k, z0, cand_deg[k] + off * step


def tree(delta, peak, anchor=0, min_score=MIN_SCORE):
    """the reference of perspectivefields_amd.yaw_tree, written independently: per unordered pair the order with the higher peak (a tie: a < b),
    the other order's turn negated; Prim's maximum spanning tree from the anchor over edges >= min_score, ties to the lower new view, then
    the lower parent -> (yaw, parent, linked)"""
    N = len(delta)
    edge = {}
    for a in range(N):
        for b in range(a + 1, N):
            pa = peak[a][b] if np.isfinite(peak[a][b]) and np.isfinite(delta[a][b]) else -np.inf
            pb = peak[b][a] if np.isfinite(peak[b][a]) and np.isfinite(delta[b][a]) else -np.inf
            s, d = (pa, delta[a][b]) if pa >= pb else (pb, -delta[b][a])
            if s >= min_score:
                edge[(a, b)], edge[(b, a)] = (s, d), (s, -d)
    yaw, parent, inside = {anchor: 0.0}, {}, [anchor]
    while True:
        cands = sorted((-edge[(u, v)][0], v, u) for u in inside for v in range(N) if v not in yaw and (u, v) in edge)
        if not cands:
            break
        _, v, u = cands[0]
        yaw[v], parent[v] = float(wrap180(yaw[u] + edge[(u, v)][1])), u
        inside.append(v)
    return (np.array([yaw.get(i, np.nan) for i in range(N)]), np.array([parent.get(i, -1) for i in range(N)]), np.array([i in yaw for i in range(N)]))


# ---------------------------------------------------------------- the same coordinates in float32: the rounding floor
def pair_points_f32(ta, Ha, Wa, tb, Hb, Wb, stride, cand):
    """(p, q) (K, S) with every step in numpy float32, in the order of yaw_align.hip: 1 / F_b as a factor, W = R_b X_b, Y(D) W from float32 sines,
    R_a^T last"""
    f = np.float32
    a, b = [f(v) for v in ta], [f(v) for v in tb]

    def rot(roll, pitch):
        sr, cr, sp, cp = np.sin(roll), np.cos(roll), np.sin(pitch), np.cos(pitch)
        return np.array([[cr, -sr, f(0)], [cp * sr, cp * cr, -sp], [sp * sr, sp * cr, cp]], dtype=f)

    inv_fb = f(1) / (b[3] * f(Hb))
    rows, cols = np.meshgrid(np.arange(0, Hb, stride), np.arange(0, Wb, stride), indexing="ij")
    x = (cols.reshape(-1).astype(f) + f(0.5) - (b[4] + f(0.5)) * f(Wb)) * inv_fb
    y = (rows.reshape(-1).astype(f) + f(0.5) - (b[5] + f(0.5)) * f(Hb)) * inv_fb
    r2 = x * x + y * y
    disc = f(1) + (f(1) - b[6] * b[6]) * r2
    with np.errstate(invalid="ignore", divide="ignore"):
        eta = (b[6] + np.sqrt(np.where(disc >= 0, disc, f(np.nan)))) / (f(1) + r2)
        W = np.stack([eta * x, eta * y, eta - b[6]], -1) @ rot(b[0], b[1]).T
        d = np.asarray(cand, dtype=f)
        cd, sd = np.cos(d)[:, None], np.sin(d)[:, None]
        V = np.stack([cd * W[None, :, 0] + sd * W[None, :, 2], np.broadcast_to(W[None, :, 1], (len(d), len(W))), cd * W[None, :, 2] - sd * W[None, :, 0]], -1)
        Xa = V @ rot(a[0], a[1])   # rows of R_a^T V
        D = Xa[..., 2] + a[6] * np.sqrt((Xa * Xa).sum(-1))
        p = a[3] * f(Ha) * (Xa[..., 0] / D) + (a[4] + f(0.5)) * f(Wa)
        q = a[3] * f(Ha) * (Xa[..., 1] / D) + (a[5] + f(0.5)) * f(Ha)
    assert p.dtype == f and q.dtype == f
    return p, q


# ---------------------------------------------------------------- the fixed inputs
# (roll, pitch, yaw [deg], rel_focal, rel_cx, rel_cy, xi)
VIEWS = [(3.0, 5.0, 0.0, 0.42, 0.0, 0.0, 0.0), (-4.0, -8.0, 55.4, 0.42, 0.0, 0.0, 0.0), (6.0, 10.0, 130.7, 0.5, 0.03, -0.02, 0.0),
         (0.0, -5.0, 169.5, 0.42, 0.0, 0.0, 0.0), (-7.0, 4.0, 250.25, 0.30, 0.0, 0.0, 0.8), (2.0, 0.0, 299.6, 0.42, 0.0, 0.0, 0.0)]
FOREIGN = (1.0, 2.0, 20.0, 0.42, 0.0, 0.0, 0.0)   # the camera of the view cropped from the other panorama
# name -> (sizes, stride).  A: one tile and a partial second one.  B: odd sizes, two sizes in one call.  B's views are 37 x 39 and 40 x 42 and not
# wider: at 37 x 53 and 40 x 56 the pinhole views 1 and 3 (114.1 degrees apart) and 1 and 5 (115.8) share 4 - 9 % of their samples at the truth,
# under min_overlap there, and score 0.89 - 0.95 a few degrees off it where the share reaches 10 %: neither an overlapping pair nor one that stays low
SETS = {"A": ([(40, 40)] * 6, 1), "B": ([(37, 39), (40, 42)] * 3, 3)}
CAND = -180.0 + np.arange(360.0)
TRUE_YAW = wrap180([v[2] for v in VIEWS])


@functools.lru_cache(None)
def panorama(seed):
    """128 x 256 x 3 in [0, 1]: Gaussian noise low-passed in the Fourier domain with the weight exp(-(f_x^2 + (2 f_y)^2) / (2 12^2))"""
    Hp, Wp = 128, 256
    rng = np.random.default_rng(seed)
    fy, fx = np.meshgrid(np.fft.fftfreq(Hp) * Hp, np.fft.fftfreq(Wp) * Wp, indexing="ij")
    w = np.exp(-(fx ** 2 + (2 * fy) ** 2) / (2 * 12.0 ** 2))
    P = np.stack([np.fft.ifft2(np.fft.fft2(rng.standard_normal((Hp, Wp))) * w).real for _ in range(3)], -1)
    P = (P - P.min()) / (P.max() - P.min())
    P.setflags(write=False)
    return P


def to_uint8(x):
    return np.clip(np.floor(x + 0.5), 0, 255).astype(np.uint8)


@functools.lru_cache(None)
def images(name, kind, foreign=False):
    """the views of a set as numpy, "u8" (the crop of 255 P0, rounded) or "f32" (the crop of P0, in [0, 1]); foreign=True adds the crop of P1"""
    sizes, _ = SETS[name]
    cams = [(panorama(0), th, hw) for th, hw in zip(VIEWS, sizes)] + ([(panorama(1), FOREIGN, sizes[0])] if foreign else [])
    out = []
    for P, th, (H, W) in cams:
        im = crop_image(P * 255.0 if kind == "u8" else P, theta_rad(*th), H, W)
        im = to_uint8(im) if kind == "u8" else im.astype(np.float32)
        im.setflags(write=False)
        out.append(im)
    return tuple(out)


def all_pairs(n):
    return [(a, b) for a in range(n) for b in range(n) if a != b]


class PairRef:
    """the reference of one ordered pair at the candidates CAND (or `cand`, degrees): moments, the count m of borderline samples, the samples
    with a ray, and what the error bounds of tests/test_gpu_yaw_align.py need"""

    def __init__(self, imgs, cams, sizes, a, b, stride, cand=CAND):
        ta, tb = theta_rad(*cams[a]), theta_rad(*cams[b])
        (Ha, Wa), (Hb, Wb) = sizes[a], sizes[b]
        rad = np.radians(cand)
        p, q, covered, z, ok = pair_points(ta, Ha, Wa, tb, Hb, Wb, stride, rad)
        La, Lb = luminance(imgs[a]), luminance(imgs[b])
        self.y = Lb[::stride, ::stride].reshape(-1)
        self.x = sample_plane(La, p, q, covered)
        self.covered, self.rays = covered, int(ok.sum())
        self.M = moments_of(self.x, self.y, covered)
        bd = band(ta, Ha, Wa, p, q, z)
        self.m = bd.sum(1)
        # the float32 floor of the coordinates, on the covered samples outside the band
        p32, q32 = pair_points_f32(ta, Ha, Wa, tb, Hb, Wb, stride, rad)
        use = covered & ~bd
        with np.errstate(invalid="ignore"):
            e = np.maximum(np.abs(p32.astype(np.float64) - p), np.abs(q32.astype(np.float64) - q))
        self.floor = float(e[use].max()) if use.any() else 0.0
        self.grad = float(max(np.abs(np.diff(La, axis=0)).max() if Ha > 1 else 0.0, np.abs(np.diff(La, axis=1)).max() if Wa > 1 else 0.0))
        self.V = value_range(imgs[a])
        self.score = zncc(self.M, self.rays)


@functools.lru_cache(None)
def set_reference(name, kind, foreign=False):
    """{(a, b): PairRef} over every ordered pair of a set; computed once, read only"""
    sizes, stride = SETS[name]
    cams = VIEWS + ([FOREIGN] if foreign else [])
    sizes = list(sizes) + ([sizes[0]] if foreign else [])
    imgs = images(name, kind, foreign)
    return {(a, b): PairRef(imgs, cams, sizes, a, b, stride) for a, b in all_pairs(len(cams))}


def tables_of(ref, n):
    """the N x N tables (delta, peak) of a set's reference"""
    delta, peak = np.full((n, n), np.nan), np.full((n, n), -np.inf)
    for (a, b), r in ref.items():
        _, peak[a, b], delta[a, b] = peak_of(r.score, CAND)
    return delta, peak


# ---------------------------------------------------------------- the reference against the re-projection's and against itself
def test_points_are_the_reprojection_source_coordinates():
    """the sign of the turn: (p, q) = source_coords(src = a at yaw 0, dst = b at yaw D) on b's sample pixels"""
    (Ha, Wa), (Hb, Wb), seen = (37, 53), (40, 56), 0
    for a, b, s in ((0, 1, 1), (4, 5, 3), (2, 4, 2)):
        ta, tb = list(theta_rad(*VIEWS[a])), list(theta_rad(*VIEWS[b]))
        cand = np.radians([-170.0, -55.4, 0.0, 49.35, 120.0])
        p, q, covered, _, ok = pair_points(ta, Ha, Wa, tb, Hb, Wb, s, cand)
        assert ok.all()
        for k, d in enumerate(cand):
            ta[2], tb[2] = 0.0, d
            pa, qa, _ = source_coords(ta, Ha, Wa, tb, Hb, Wb)
            pa, qa = pa[::s, ::s].reshape(-1), qa[::s, ::s].reshape(-1)
            vis = np.isfinite(pa)
            seen += int(vis.sum())
            far = np.maximum(1.0, np.maximum(np.abs(pa), np.abs(qa)))   # points far outside a have large coordinates: relative there
            assert (np.abs(p[k] - pa) / far)[vis].max(initial=0.0) <= 1e-10 and (np.abs(q[k] - qa) / far)[vis].max(initial=0.0) <= 1e-10
            assert not covered[k][~vis].any()
    assert seen > 1000


def test_score_is_invariant_to_the_constant_and_the_channel_order():
    r = set_reference("A", "u8")[(0, 1)]
    k = int(np.argmax(r.score))
    M2 = moments_of(r.x + 127.5, r.y + 127.5, r.covered)
    assert abs(zncc(M2, r.rays)[k] - r.score[k]) <= 1e-9
    assert zncc(np.array([10.0, 5.0, 5.0, 2.5, 2.5, 2.5]), 50) == -np.inf      # zero variance
    assert zncc(np.array([4.0, 1.0, 2.0, 3.0, 4.0, 2.0]), 50) == -np.inf       # n below the threshold


def overlaps(r, a, b):
    """the pair overlaps: at the candidate next to the true turn at least min_overlap of b's samples with a ray are covered, the share below
    which there is no score.  This is the pairs at most 120 degrees apart except the pinhole pairs 1 - 3 and 1 - 5 (114.1 and 115.8 degrees),
    whose 100 degree fields of view share nothing: 16 of the 30 ordered pairs in both sets"""
    k = int(round(float(wrap180(VIEWS[b][2] - VIEWS[a][2])) + 180.0)) % 360
    return r.M[k, 0] >= MIN_OVERLAP * r.rays


@pytest.mark.parametrize("name", ["A", "B"])
@pytest.mark.parametrize("kind", ["u8", "f32"])
def test_reference_recovers_the_truth(name, kind):
    """every overlapping pair peaks at >= 0.95 within 0.2 degrees of the truth, every other pair stays below 0.8, the tree gives every yaw
    within 0.5 degrees"""
    ref = set_reference(name, kind)
    worst_peak, worst_err, worst_other, n_over = 1.0, 0.0, -1.0, 0
    for (a, b), r in ref.items():
        true = float(wrap180(VIEWS[b][2] - VIEWS[a][2]))
        _, z, d = peak_of(r.score, CAND)
        if overlaps(r, a, b):
            n_over += 1
            worst_peak, worst_err = min(worst_peak, z), max(worst_err, abs(float(wrap180(d - true))))
            assert z >= 0.95 and abs(float(wrap180(d - true))) <= 0.2, (a, b, z, d, true)
        else:
            assert abs(true) > 110.0, (a, b)
            worst_other = max(worst_other, z)
            assert z < 0.8, (a, b, z)
    assert n_over == 16
    yaw, parent, linked = tree(*tables_of(ref, 6))
    err = np.abs(wrap180(yaw - TRUE_YAW)).max()
    print(f"set {name} {kind}: {n_over} overlapping pairs peak >= {worst_peak:.4f} within {worst_err:.4f} deg; other pairs <= {worst_other:.4f}; tree yaws within {err:.4f} deg")
    assert linked.all() and err <= 0.5


def test_the_foreign_view_links_to_nothing():
    ref = set_reference("A", "u8", True)
    best = max(peak_of(r.score, CAND)[1] for (a, b), r in ref.items() if 6 in (a, b))
    print(f"foreign view: highest peak against the six views {best:.4f}")
    assert best < 0.8
    yaw, parent, linked = tree(*tables_of(ref, 7))
    assert linked[:6].all() and not linked[6] and np.isnan(yaw[6]) and parent[6] == -1
    yaw6, _, _ = tree(*tables_of(set_reference("A", "u8"), 6))
    assert np.array_equal(yaw[:6], yaw6)


@pytest.mark.parametrize("name", ["A", "B"])
def test_borderline_samples_leave_half_of_the_entries_untouched(name):
    ref = set_reference(name, "u8")
    scored = np.concatenate([r.M[:, 0] >= MIN_OVERLAP * r.rays for r in ref.values()])
    m0 = np.concatenate([r.m == 0 for r in ref.values()])
    share = (scored & m0).sum() / scored.sum()
    print(f"set {name}: {100 * share:.1f} % of the {scored.sum()} scored entries have no borderline sample")
    assert share >= 0.5


def test_fp32_floor_of_the_coordinates():
    """the float32 evaluation is close to fp64: its error is the floor the GPU's sampled values are held to (x 4)"""
    worst = max(r.floor for name in SETS for r in set_reference(name, "u8").values())
    print(f"fp32 floor of (p, q) over both sets: {worst:.3e} px")
    assert 0 < worst <= 1e-3


# ---------------------------------------------------------------- the tree on hand-made tables
def _tables(n, edges):
    d, p = np.full((n, n), np.nan), np.full((n, n), -np.inf)
    for (a, b), (turn, score) in edges.items():
        d[a, b], p[a, b] = turn, score
    return d, p


def _both(d, p, **kw):
    from perspectivefields_amd import yaw_tree

    got, want = yaw_tree(d, p, **kw), tree(d, p, **kw)
    for g, w in zip(got, want):
        assert np.array_equal(g, w, equal_nan=True), (got, want)
    return got


def test_tree_chain_and_anchor():
    d, p = _tables(4, {(0, 1): (30.0, 0.9), (1, 2): (40.0, 0.95), (2, 3): (50.0, 0.85)})
    yaw, parent, linked = _both(d, p)
    assert np.allclose(yaw, [0, 30, 70, 120]) and list(parent) == [-1, 0, 1, 2] and linked.all()
    yaw, parent, _ = _both(d, p, anchor=2)
    assert np.allclose(yaw, [-70, -40, 0, 50]) and list(parent) == [1, 2, -1, 2]


def test_tree_tie_goes_to_the_lower_index():
    d, p = _tables(3, {(0, 1): (10.0, 0.9), (0, 2): (20.0, 0.9), (1, 2): (15.0, 0.9)})
    yaw, parent, _ = _both(d, p)
    assert list(parent) == [-1, 0, 0] and np.allclose(yaw, [0, 10, 20])   # view 1 first; then 2 from the lower parent 0, not from 1
    d, p = _tables(3, {(0, 2): (20.0, 0.9), (1, 2): (15.0, 0.9), (0, 1): (10.0, 0.85)})
    yaw, parent, _ = _both(d, p)
    assert list(parent) == [-1, 2, 0] and np.allclose(yaw, [0, 5, 20])    # the higher edge first, then the 0.9 edge to 1 beats the 0.85 one


def test_tree_edge_under_min_score_and_unreachable_view():
    d, p = _tables(4, {(0, 1): (30.0, 0.9), (1, 2): (40.0, 0.79), (2, 3): (5.0, 0.99)})
    yaw, parent, linked = _both(d, p)
    assert list(linked) == [True, True, False, False] and np.isnan(yaw[2:]).all() and list(parent) == [-1, 0, -1, -1]
    yaw, _, linked = _both(d, p, min_score=0.75)
    assert linked.all() and np.allclose(yaw, [0, 30, 70, 75])
    yaw, _, linked = _both(d, p, min_score=0.79)   # the threshold itself links
    assert linked.all()


def test_tree_reverse_order_is_negated_and_the_higher_peak_wins():
    d, p = _tables(2, {(0, 1): (30.0, 0.85), (1, 0): (-31.0, 0.9)})
    yaw, _, _ = _both(d, p)
    assert np.allclose(yaw, [0, 31])
    d, p = _tables(2, {(0, 1): (30.0, 0.9), (1, 0): (-31.0, 0.9)})      # a tie keeps (a < b)
    assert np.allclose(_both(d, p)[0], [0, 30])
    d, p = _tables(2, {(1, 0): (-31.0, 0.9)})                            # only the reverse order measured
    assert np.allclose(_both(d, p)[0], [0, 31])
    d, p = _tables(2, {(0, 1): (np.nan, 0.99), (1, 0): (-31.0, 0.9)})    # a peak without a turn is no measurement
    assert np.allclose(_both(d, p)[0], [0, 31])


def test_tree_wraps_at_180():
    d, p = _tables(3, {(0, 1): (170.0, 0.9), (1, 2): (20.0, 0.9)})
    assert np.allclose(_both(d, p)[0], [0, 170, -170])
    d, p = _tables(3, {(0, 1): (100.0, 0.9), (1, 2): (80.0, 0.9)})
    assert np.allclose(_both(d, p)[0], [0, 100, -180])                   # [-180, 180)
    d, p = _tables(2, {(1, 0): (180.0, 0.9)})
    assert np.allclose(_both(d, p)[0], [0, -180])


def test_tree_argument_errors():
    from perspectivefields_amd import yaw_tree

    with pytest.raises(ValueError):
        yaw_tree(np.zeros((2, 3)), np.zeros((2, 3)))
    with pytest.raises(ValueError):
        yaw_tree(np.zeros((2, 2)), np.zeros((2, 2)), anchor=2)


# ---------------------------------------------------------------- host-side contract (fails before the feature exists)
def test_exports():
    import perspective2d
    import perspectivefields_amd

    for name in ("yaw_scores", "align_yaw", "yaw_tree"):
        assert name in perspectivefields_amd.__all__ and callable(getattr(perspectivefields_amd, name))
    assert callable(perspective2d.align_yaw) and callable(perspectivefields_amd.PerspectiveFields.align_yaw)


def test_symbols_prototypes_and_constants():
    from perspectivefields_amd import perspectivefields as pfm
    from perspectivefields_amd.engine import _SIGNATURES, declared_symbols, load_library

    hdr = open(os.path.join(ROOT, "include", "pf_hip.h")).read()
    assert "int pf_yaw_moments(int device, int n_view, const void* const* h_view, const int32_t* h_view_hw" in hdr
    assert "size_t pf_yaw_moments_workspace_bytes(int n_view, const int32_t* h_view_hw" in hdr
    assert f"#define PF_YAW_MAX_CAND {pfm._YAW_MAX_CAND}" in hdr
    kh = open(os.path.join(ROOT, "perspectivefields_amd", "csrc", "pf_kernels.h")).read()
    assert f"static constexpr int TILE = {TILE};" in kh
    assert {"pf_yaw_moments", "pf_yaw_moments_workspace_bytes"} <= set(declared_symbols())
    res, args = _SIGNATURES["pf_yaw_moments"]
    assert res is ctypes.c_int and len(args) == 15 and args[13] is ctypes.c_size_t
    res, args = _SIGNATURES["pf_yaw_moments_workspace_bytes"]
    assert res is ctypes.c_size_t and len(args) == 6
    lib = load_library()
    assert hasattr(lib, "pf_yaw_moments") and hasattr(lib, "pf_yaw_moments_workspace_bytes")


CAM = dict(roll=0.0, pitch=0.0, rel_focal=1.0)


def test_cpu_tensors_raise():
    from perspectivefields_amd import align_yaw, yaw_scores
    from perspectivefields_amd.engine import PfError

    for imgs in (torch.zeros((2, 8, 16, 3), dtype=torch.uint8), [torch.zeros((8, 16, 3)), torch.zeros((8, 16, 3))]):
        with pytest.raises(PfError):
            yaw_scores(imgs, CAM, [(0, 1)], [0.0])
        with pytest.raises(PfError):
            align_yaw(imgs, CAM)


def test_pf_yaw_moments_rejects_bad_arguments_before_device_work():
    from perspectivefields_amd.engine import load_library

    lib = load_library()
    ints = lambda *s: (ctypes.c_int32 * len(s))(*s)
    ptrs = lambda n: (ctypes.c_void_p * n)(*([0x1000] * n))
    dev = ctypes.c_void_p(4096)

    def call(n=2, p=None, hw=None, dtype=0, cam=dev, n_pair=1, pairs=(0, 1), n_cand=4, cand=dev, stride=1, out=dev, ws=dev, ws_bytes=None):
        hw = hw or ints(*([8, 16] * max(n, 1)))
        c_pairs = None if pairs is None else ints(*pairs)
        if ws_bytes is None:
            ws_bytes = lib.pf_yaw_moments_workspace_bytes(n, hw, n_pair, c_pairs, n_cand, stride)
        rc = lib.pf_yaw_moments(0, n, ptrs(max(n, 1)) if p is None else None if p == "null" else p, hw, dtype, cam, n_pair, c_pairs, n_cand, cand, stride, out, ws, ws_bytes, None)
        return rc, lib.pf_last_error(None).decode()

    need = lib.pf_yaw_moments_workspace_bytes(2, ints(8, 16, 8, 16), 1, ints(0, 1), 4, 1)
    assert need >= 2 * 8 * 16 * 4 + 4 * 6 * 4
    assert lib.pf_yaw_moments_workspace_bytes(2, ints(8, 16, 8, 16), 1, ints(0, 0), 4, 1) == 0
    for kw, what in ((dict(n=1, pairs=(0, 0)), "two views"), (dict(p="null"), "two views"), (dict(p=(ctypes.c_void_p * 2)()), "NULL"), (dict(hw=ints(0, 16, 8, 16)), "smaller"),
                     (dict(hw=ints(8, 16, 8, 0)), "smaller"), (dict(dtype=2), "dtype"), (dict(cam=None), "required"), (dict(cand=None), "required"),
                     (dict(out=None), "required"), (dict(n_pair=0), "n_pair"), (dict(pairs=None), "n_pair"), (dict(pairs=(0, 2)), "index"), (dict(pairs=(-1, 1)), "index"),
                     (dict(pairs=(1, 1)), "a == b"), (dict(stride=0), "stride"), (dict(n_cand=0), "n_cand"), (dict(n_cand=4097), "n_cand"),
                     (dict(ws=None, ws_bytes=need), "workspace"), (dict(ws_bytes=need - 1), "workspace"), (dict(out=ctypes.c_void_p(4104)), "aligned")):
        rc, msg = call(**kw)
        assert rc == -1 and what in msg and msg.startswith("pf_yaw_moments"), (kw, rc, msg)
    if not torch.cuda.is_available():   # good arguments pass the checks and fail on the missing device only
        rc, msg = call(n_cand=4096)
        assert rc == -2 and "no HIP device" in msg, (rc, msg)


def test_python_argument_errors_before_the_library_is_loaded(monkeypatch):
    from perspectivefields_amd import engine
    from perspectivefields_amd import perspectivefields as pfm

    def no_library(*a, **k):
        raise AssertionError("the library was loaded before the arguments were checked")

    monkeypatch.setattr(engine, "load_library", no_library)
    monkeypatch.setattr(pfm.torch, "is_tensor", lambda v: isinstance(v, (torch.Tensor, FakeCuda)))
    ok, small = FakeCuda((8, 16, 3)), FakeCuda((6, 16, 3))
    two = [ok, small]
    bad = [
        dict(images=[ok, FakeCuda((8, 16, 4))]), dict(images=[ok, FakeCuda((8, 16))]), dict(images=[ok, FakeCuda((0, 16, 3))]), dict(images=[ok, FakeCuda((8, 16, 3), torch.float16)]),
        dict(images=[ok, FakeCuda((8, 16, 3), torch.float32)]), dict(images=[]), dict(images=[ok]), dict(images=ok), dict(images=FakeCuda((1, 8, 16, 3))),
        dict(mode="grad"), dict(stride=0), dict(min_overlap=1.5), dict(min_overlap=-0.1), dict(pairs=[]), dict(pairs=[(0, 0)]), dict(pairs=[(0, 2)]), dict(pairs=[(-1, 0)]),
        dict(candidates=[]), dict(candidates=np.zeros((2, 2))), dict(candidates=np.zeros(4097)), dict(cams=dict(roll=0.0, pitch=0.0)), dict(cams=dict(CAM, fov=1.0)),
        dict(cams=dict(CAM, roll=[1.0, 2.0, 3.0])),
    ]
    for kw in bad:
        args = dict(images=two, cams=CAM, pairs=[(0, 1)], candidates=[0.0, 1.0])
        args.update(kw)
        with pytest.raises(ValueError):
            pfm.yaw_scores(args.pop("images"), args.pop("cams"), args.pop("pairs"), args.pop("candidates"), **args)
    with pytest.raises(TypeError):
        pfm.yaw_scores(two, (0.0, 0.0, 1.0), [(0, 1)], [0.0])
    with pytest.raises(TypeError):
        pfm.yaw_scores([ok, np.zeros((8, 16, 3))], CAM, [(0, 1)], [0.0])
    for kw in (dict(step=0.0), dict(step=-1.0), dict(step=0.05), dict(step=float("nan")), dict(anchor=2), dict(anchor=-1), dict(images=[ok]), dict(mode="grad"), dict(stride=0)):
        args = dict(images=two, cams=CAM)
        args.update(kw)
        with pytest.raises(ValueError):
            pfm.align_yaw(args.pop("images"), args.pop("cams"), **args)


def test_model_method_argument_errors_without_a_gpu():
    from perspectivefields_amd import PerspectiveFields
    from perspectivefields_amd.engine import PfError

    two = [FakeCuda((8, 16, 3)), FakeCuda((8, 16, 3))]
    fields_only = dict(pred_gravity_original=None, pred_latitude_original=None)
    with pytest.raises(PfError, match="fit_camera"):
        PerspectiveFields.align_yaw(None, two, [fields_only, fields_only])
    full = dict(pred_roll=1.0, pred_pitch=2.0, pred_rel_focal=0.8)
    with pytest.raises(ValueError):
        PerspectiveFields.align_yaw(None, two, [full, full], mode="rad")
    with pytest.raises(ValueError):
        PerspectiveFields.align_yaw(None, two, [])


def test_yaw_kernels_are_in_the_library_without_scratch():
    """scripts/kernel_resources.py on the built library: the four kernels are there for gfx950 with no spilled register and no scratch; the
    moments kernel's LDS is the tile and the constants"""
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
    for name, lds in (("pf::yaw_luminance_kernel<unsigned char>", 0), ("pf::yaw_luminance_kernel<float>", 0), ("pf::yaw_moments_kernel", 16 * TILE + 128), ("pf::yaw_sum_kernel", 0)):
        r = by[name]
        assert r["spill"] == 0 and r["scratch"] == 0 and r["lds"] <= lds, r
