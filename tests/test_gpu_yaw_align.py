"""Yaw alignment of camera views of one centre on the GPU (include/pf_hip.h pf_yaw_moments, perspectivefields_amd.yaw_scores / align_yaw,
PerspectiveFields.align_yaw) against the fp64 reference of tests/test_yaw_align_ref.py: moments and scores of all 30 ordered pairs of the two
fixed sets as uint8 and float32, the chain crop -> align -> compose, determinism, edge shapes, non-finite cameras, a foreign view and the
model method.

Tolerances.  m is the number of a (pair, candidate)'s samples whose fp32 and fp64 coverage may differ (the reference's
band: within 1e-2 px of a's border or 1e-3 of z_min).  n is held to within m.  Every other moment is held to the sum of
  m x the largest possible term (V, V, V^2, V^2, V^2 with V = 127.5 or 0.5, the largest |L|);
  the value error e of one sample, summed over the covered samples with the partner factor (1 for sum x and sum y, 2 |x| + e for sum x^2, 2 |y| + e
  for sum y^2, |x| + |y| + e for sum xy): e = 2 x (coordinate floor) x (largest difference between adjacent texels of L_a) + 4 x 2^-24 x V, the
  coordinate floor being 4 x the largest error of the same formulas in numpy float32 over the set's pairs, computed in the same run;
  (T + 8) x 2^-24 x (sum of |term| + the value error above), the bound of recursive summation, T the samples one thread adds (<= 1024).
The score is held to what those bounds give for the ZNCC by interval propagation in fp64 (score_bound)."""
import functools

import numpy as np
import pytest
import torch

from tests.test_pano_compose_ref import compose
from tests.test_reproject_ref import theta_rad
from tests.test_yaw_align_ref import (CAND, FOREIGN, MIN_OVERLAP, SETS, TILE, TRUE_YAW, VIEWS, PairRef, all_pairs, images, panorama, peak_of, set_reference, tables_of,
                                      to_uint8, tree, wrap180)

pytestmark = pytest.mark.gpu
KEYS = ("roll", "pitch", "yaw", "rel_focal", "rel_cx", "rel_cy", "xi")
U = 2.0 ** -24


def cam_dict(views, with_yaw=False):
    c = np.asarray(views, dtype=np.float64)
    return {k: c[:, i] for i, k in enumerate(KEYS) if with_yaw or k != "yaw"}


def on_gpu(imgs):
    return [torch.from_numpy(np.array(im)).cuda() for im in imgs]   # a copy: the cached inputs are read-only


def bits(t):
    return t.contiguous().view(torch.int64)


def moment_bounds(r, floor, T):
    """(K, 6): the allowed distance of the GPU moments of one pair to the reference r (a PairRef), see the module docstring"""
    c = r.covered.astype(np.float64)
    ax, ay = np.abs(r.x) * c, np.abs(r.y)[None, :] * c
    e = 2.0 * floor * r.grad + 4.0 * U * r.V
    n = c.sum(1)
    value = np.stack([0 * n, n * e, n * e, (2 * ax * e + e * e * c).sum(1), (2 * ay * e + e * e * c).sum(1), ((ax + ay) * e + e * e * c).sum(1)], 1)
    terms = np.stack([0 * n, ax.sum(1), ay.sum(1), (ax * ax).sum(1), (ay * ay).sum(1), (ax * ay).sum(1)], 1)
    V = r.V
    return r.m[:, None] * np.array([1.0, V, V, V * V, V * V, V * V]) + value + (T + 8) * U * (terms + value)


def score_bound(M, B):
    """the largest distance of the ZNCC of moments within B of M (both (K, 6), fp64) to the ZNCC of M, by interval propagation; inf where a
    variance could vanish"""
    n, sx, sy, sxx, syy, sxy = M.T
    dn, dx, dy, dxx, dyy, dxy = B.T
    num = n * sxy - sx * sy
    va, vb = n * sxx - sx * sx, n * syy - sy * sy
    dnum = n * dxy + dn * np.abs(sxy) + dn * dxy + np.abs(sx) * dy + np.abs(sy) * dx + dx * dy
    dva = n * dxx + dn * sxx + dn * dxx + 2 * np.abs(sx) * dx + dx * dx
    dvb = n * dyy + dn * syy + dn * dyy + 2 * np.abs(sy) * dy + dy * dy
    with np.errstate(invalid="ignore", divide="ignore"):
        ok = (va > dva) & (vb > dvb)
        low = np.sqrt(np.where(ok, (va - dva) * (vb - dvb), 1.0))
        return np.where(ok, dnum / low + np.abs(num) * (1.0 / low - 1.0 / np.sqrt(np.where(ok, va * vb, 1.0))), np.inf)


def samples_per_thread(size, stride):
    return min(TILE, -(-size[0] // stride) * -(-size[1] // stride))


@functools.lru_cache(None)
def set_floor(name, kind):
    return 4.0 * max(r.floor for r in set_reference(name, kind).values())


@functools.lru_cache(None)
def gpu_set(name, kind):
    """(score, overlap, moments) of all 30 ordered pairs of a set as numpy; one GPU call, read only"""
    from perspectivefields_amd import yaw_scores

    _, stride = SETS[name]
    out = yaw_scores(on_gpu(images(name, kind)), cam_dict(VIEWS), all_pairs(6), CAND, stride=stride, return_moments=True)
    assert [o.shape for o in out] == [(30, 360), (30, 360), (30, 360, 6)] and all(o.dtype == torch.float64 and o.is_cuda for o in out)
    return tuple(o.cpu().numpy() for o in out)


def check_moments(M, r, floor, T, what):
    """the GPU moments M (K, 6) of one pair against its reference; returns the largest error / bound of the five sums"""
    B = moment_bounds(r, floor, T)
    err = np.abs(M - r.M)
    assert (err[:, 0] <= r.m).all(), (what, "n", err[:, 0].max())
    assert (err[:, 1:] <= B[:, 1:]).all(), (what, np.argwhere(err[:, 1:] > B[:, 1:])[:4], err.max(0), B.max(0))
    with np.errstate(invalid="ignore", divide="ignore"):
        return float(np.nanmax(np.where(B[:, 1:] > 0, err[:, 1:] / B[:, 1:], 0.0)))


@pytest.mark.parametrize("kind", ["u8", "f32"])
@pytest.mark.parametrize("name", ["A", "B"])
def test_moments_of_all_pairs_match_the_fp64_reference(name, kind):
    sizes, stride = SETS[name]
    _, _, M = gpu_set(name, kind)
    ref, floor = set_reference(name, kind), set_floor(name, kind)
    worst = 0.0
    for i, (a, b) in enumerate(all_pairs(6)):
        worst = max(worst, check_moments(M[i], ref[(a, b)], floor, samples_per_thread(sizes[b], stride), (name, kind, a, b)))
    print(f"moments of set {name} {kind}: coordinate floor x 4 = {floor:.3e} px; largest error / allowed over the 30 pairs {worst:.3f}")


@pytest.mark.parametrize("kind", ["u8", "f32"])
@pytest.mark.parametrize("name", ["A", "B"])
def test_scores_match_the_fp64_reference(name, kind):
    """on the entries without a borderline sample and with n above the threshold the score is within the bound the moment bounds imply;
    -inf sits where the reference has it (an entry whose reference n is within its m borderline samples of the threshold may fall on either side:
    the tolerance of n; their number is printed)"""
    sizes, stride = SETS[name]
    S, O, M = gpu_set(name, kind)
    ref, floor = set_reference(name, kind), set_floor(name, kind)
    worst = worst_ratio = 0.0
    free = checked = 0
    for i, (a, b) in enumerate(all_pairs(6)):
        r = ref[(a, b)]
        thr = MIN_OVERLAP * r.rays
        either = (r.m > 0) & (np.abs(r.M[:, 0] - thr) <= r.m)
        free += int(either.sum())
        assert np.array_equal(np.isneginf(S[i])[~either], np.isneginf(r.score)[~either]), (name, kind, a, b)
        assert np.isfinite(S[i][~np.isneginf(S[i])]).all()
        use = (r.m == 0) & np.isfinite(r.score)
        E = score_bound(r.M, moment_bounds(r, floor, samples_per_thread(sizes[b], stride)))
        err = np.abs(np.where(use, S[i], 0.0) - np.where(use, r.score, 0.0))[use]
        assert np.isfinite(E[use]).all() and (err <= E[use]).all(), (name, kind, a, b, err.max(), E[use].max())
        checked += int(use.sum())
        if use.any():
            worst, worst_ratio = max(worst, float(err.max())), max(worst_ratio, float((err / E[use]).max()))
        assert np.abs(O[i] - M[i][:, 0] / r.rays).max() <= 1e-15
    print(f"scores of set {name} {kind}: {checked} entries checked, largest error {worst:.3e}, largest error / allowed {worst_ratio:.3f}; {free} entries within m of the threshold")
    assert checked >= 1500


# ---------------------------------------------------------------- crop -> align -> compose
@functools.lru_cache(None)
def end_to_end():
    """P0 as uint8, cropped to set A on the GPU, aligned: the crops (device and numpy), the yaws and the info, and the fp64 reference on those crops"""
    from perspectivefields_amd import align_yaw, crop_panorama

    sizes, stride = SETS["A"]
    c = cam_dict(VIEWS, with_yaw=True)
    pano = torch.from_numpy(to_uint8(panorama(0) * 255.0)).cuda()
    crops, _, _ = crop_panorama(pano, c["roll"], c["pitch"], c["rel_focal"], c["rel_cx"], c["rel_cy"], yaw=c["yaw"], xi=c["xi"], height=40, width=40, fields=False)
    yaw, info = align_yaw(crops, cam_dict(VIEWS), stride=stride, return_info=True)
    host = [im for im in crops.cpu().numpy()]
    ref = {(a, b): PairRef(host, VIEWS, sizes, a, b, stride) for a, b in all_pairs(6)}
    return crops, host, yaw, info, ref


def test_align_yaw_end_to_end_gives_the_reference_peaks_turns_and_tree():
    sizes, stride = SETS["A"]
    crops, host, yaw, info, ref = end_to_end()
    assert yaw.shape == (6,) and yaw.dtype == torch.float64 and yaw.is_cuda
    from perspectivefields_amd import yaw_scores

    delta, peak = info["delta"].cpu().numpy(), info["peak"].cpu().numpy()
    pairs = all_pairs(6)
    best = yaw_scores(crops, cam_dict(VIEWS), pairs, CAND, stride=stride)[0].argmax(1).cpu().numpy()   # the candidates align_yaw's peaks sit at
    floor = 4.0 * max(r.floor for r in ref.values())
    worst = worst_ratio = 0.0
    n_high = 0
    for (a, b), r in ref.items():
        k, z, d = peak_of(r.score, CAND)
        if z < 0.95:
            continue
        n_high += 1
        E = score_bound(r.M, moment_bounds(r, floor, TILE))
        E = max(E[k], E[(k - 1) % 360], E[(k + 1) % 360])
        curv = abs(r.score[(k - 1) % 360] - 2 * z + r.score[(k + 1) % 360])
        allowed = 4 * E / curv * 1.0 + 1e-6   # x step = 1 degree
        assert best[pairs.index((a, b))] == k, (a, b, best[pairs.index((a, b))], k)
        assert abs(peak[a, b] - z) <= E, (a, b, peak[a, b], z, E)
        err = abs(float(wrap180(delta[a, b] - d)))
        worst, worst_ratio = max(worst, err), max(worst_ratio, err / allowed)
        assert err <= allowed, (a, b, delta[a, b], d, allowed)
    assert n_high == 16
    yaw_ref, parent_ref, linked_ref = tree(*tables_of(ref, 6))
    assert np.array_equal(info["parent"], parent_ref) and np.array_equal(info["linked"], linked_ref) and linked_ref.all()
    got = yaw.cpu().numpy()
    e_truth, e_ref = np.abs(wrap180(got - TRUE_YAW)).max(), np.abs(wrap180(got - yaw_ref)).max()
    print(f"align_yaw on the GPU crops of set A: refined turns within {worst:.3e} deg of the reference ({worst_ratio:.3f} of allowed); yaws within "
          f"{e_ref:.3e} deg of the reference's and {e_truth:.4f} deg of the truth")
    assert e_truth <= 0.5


def test_composition_with_the_recovered_yaws():
    """compose_panorama with the recovered yaws against compose_panorama with the true yaws: no further apart than the fp64 chain (reference
    alignment, reference composition, on the same crops) plus 1 LSB"""
    from perspectivefields_amd import compose_panorama

    crops, host, yaw, info, ref = end_to_end()
    Hp, Wp = 32, 64
    c = cam_dict(VIEWS)
    got = compose_panorama(crops, dict(c, yaw=yaw), height=Hp, width=Wp)
    want = compose_panorama(crops, dict(c, yaw=TRUE_YAW), height=Hp, width=Wp)
    d_gpu = float((got.to(torch.int32) - want.to(torch.int32)).abs().max())
    yaw_ref, _, _ = tree(*tables_of(ref, 6))
    thetas = lambda yaws: [theta_rad(v[0], v[1], y, *v[3:]) for v, y in zip(VIEWS, yaws)]
    a, _, _ = compose(host, thetas(yaw_ref), Hp, Wp)
    b, _, _ = compose(host, thetas(TRUE_YAW), Hp, Wp)
    d_ref = float(np.abs(a - b).max())
    print(f"composition with recovered against true yaws: GPU {d_gpu:.0f} LSB, fp64 reference chain {d_ref:.3f} LSB")
    assert d_gpu <= d_ref + 1.0


# ---------------------------------------------------------------- determinism and shapes
def test_moments_are_bit_identical_across_runs_batches_orders_and_candidate_splits():
    from perspectivefields_amd import yaw_scores

    _, stride = SETS["A"]
    dev, c, pairs = on_gpu(images("A", "u8")), cam_dict(VIEWS), all_pairs(6)
    run = lambda prs, cand: yaw_scores(dev, c, prs, cand, stride=stride, return_moments=True)[2]
    first = run(pairs, CAND)
    assert torch.equal(bits(first), bits(torch.from_numpy(gpu_set("A", "u8")[2]).cuda()))   # another run
    for i in (0, 17, 29):
        assert torch.equal(bits(run([pairs[i]], CAND)[0]), bits(first[i])), pairs[i]          # a pair alone
    order = np.random.default_rng(5).permutation(30)
    mixed = run([pairs[i] for i in order], CAND)
    assert torch.equal(bits(mixed), bits(first[torch.as_tensor(order).cuda()]))               # a permuted pair list
    halves = torch.cat([run(pairs, CAND[:180]), run(pairs, CAND[180:])], 1)
    assert torch.equal(bits(halves), bits(first))                                             # 360 candidates as two calls of 180
    for K in (1, 65):                                                                         # one lane of one chunk; one chunk and one lane of the next
        assert torch.equal(bits(run(pairs, CAND[100:100 + K])), bits(first[:, 100:100 + K])), K


def test_a_stride_larger_than_a_view_gives_one_sample():
    from perspectivefields_amd import yaw_scores

    imgs = images("A", "u8")
    S, O, M = yaw_scores(on_gpu(imgs), cam_dict(VIEWS), all_pairs(6), CAND, stride=64, return_moments=True)
    M = M.cpu().numpy()
    assert set(np.unique(M[..., 0])) == {0.0, 1.0} and torch.isneginf(S).all()   # one sample has no variance
    refs = {(a, b): PairRef(imgs, VIEWS, [(40, 40)] * 6, a, b, 64) for a, b in ((0, 1), (4, 5), (2, 3))}
    floor = max(set_floor("A", "u8"), 4.0 * max(r.floor for r in refs.values()))
    for (a, b), r in refs.items():
        assert r.rays == 1 and r.M[:, 0].max() == 1.0
        check_moments(M[all_pairs(6).index((a, b))], r, floor, 1, ("stride 64", a, b))


def test_one_row_and_one_column_views():
    """views of 1 x 17 and 19 x 1 against a 40 x 40 one, in every order"""
    from perspectivefields_amd import yaw_scores

    rng = np.random.default_rng(9)
    cams = [VIEWS[0], (2.0, 3.0, 30.0, 8.0, 0.0, 0.0, 0.0), (-3.0, -2.0, -25.0, 0.45, 0.0, 0.0, 0.3)]
    sizes = [(40, 40), (1, 17), (19, 1)]
    imgs = [images("A", "u8")[0]] + [rng.integers(0, 256, (H, W, 3), dtype=np.uint8) for H, W in sizes[1:]]
    pairs = all_pairs(3)
    S, O, M = yaw_scores(on_gpu(imgs), cam_dict(cams), pairs, CAND, stride=1, return_moments=True)
    M = M.cpu().numpy()
    refs = {p: PairRef(imgs, cams, sizes, p[0], p[1], 1) for p in pairs}
    floor = 4.0 * max(r.floor for r in refs.values())
    assert floor > 0
    for i, p in enumerate(pairs):
        check_moments(M[i], refs[p], floor, samples_per_thread(sizes[p[1]], 1), ("thin", p))
        assert 0 not in p or refs[p].M[:, 0].max() >= 5, p   # every pair with the 40 x 40 view has covered samples to compare


# ---------------------------------------------------------------- non-finite cameras, a foreign view
@pytest.mark.parametrize("key", ["rel_focal", "roll", "pitch"])
def test_a_non_finite_camera_drops_its_view_only(key):
    from perspectivefields_amd import align_yaw, yaw_scores

    _, stride = SETS["A"]
    dev, pairs = on_gpu(images("A", "u8")), all_pairs(6)
    c = cam_dict(VIEWS)
    c[key] = c[key].copy()
    c[key][2] = np.nan
    M = yaw_scores(dev, c, pairs, CAND, stride=stride, return_moments=True)[2]
    clean = torch.from_numpy(gpu_set("A", "u8")[2]).cuda()
    with2 = torch.as_tensor([2 in p for p in pairs]).cuda()
    assert (M[with2][..., 0] == 0).all() and (M[with2] == 0).all()
    assert torch.equal(bits(M[~with2]), bits(clean[~with2]))
    yaw, info = align_yaw(dev, c, stride=stride, return_info=True)
    assert torch.isnan(yaw[2]) and not info["linked"][2] and info["parent"][2] == -1
    keep = [0, 1, 3, 4, 5]
    others = align_yaw([dev[i] for i in keep], cam_dict([VIEWS[i] for i in keep]), stride=stride)
    assert torch.equal(bits(yaw[torch.as_tensor(keep).cuda()]), bits(others))
    assert np.abs(wrap180(others.cpu().numpy() - TRUE_YAW[keep])).max() <= 0.5


def test_a_foreign_view_comes_back_unlinked():
    from perspectivefields_amd import align_yaw

    _, stride = SETS["A"]
    seven = on_gpu(images("A", "u8", True))
    yaw, info = align_yaw(seven, cam_dict(VIEWS + [FOREIGN]), stride=stride, return_info=True)
    six = align_yaw(seven[:6], cam_dict(VIEWS), stride=stride)
    assert torch.isnan(yaw[6]) and not info["linked"][6] and info["linked"][:6].all()
    assert torch.equal(bits(yaw[:6]), bits(six))
    best = float(torch.maximum(info["peak"][6, :6].max(), info["peak"][:6, 6].max()))
    print(f"foreign view on the GPU: highest peak against the six views {best:.4f}")
    assert best < 0.8


# ---------------------------------------------------------------- the model method: crop -> fit -> align -> compose on the device
def test_model_method_on_fitted_cameras():
    """m.align_yaw on fit_camera results of the GPU crops' ground-truth fields: 96 x 96 crops, the default stride (2: 48 x 48 samples, three
    tiles).  No claim about the network's accuracy: the fields are the labels"""
    from perspectivefields_amd import PerspectiveFields
    from perspectivefields_amd import crop_panorama
    from perspectivefields_amd.engine import PfError

    c = cam_dict(VIEWS, with_yaw=True)
    pano = torch.from_numpy(to_uint8(panorama(0) * 255.0)).cuda()
    crops, up, lat = crop_panorama(pano, c["roll"], c["pitch"], c["rel_focal"], c["rel_cx"], c["rel_cy"], yaw=c["yaw"], xi=c["xi"], height=96, width=96)
    m = PerspectiveFields("Paramnet-360Cities-edina-centered", weights="synthetic:0").eval().cuda()
    labels = [dict(pred_gravity_original=u, pred_latitude_original=l) for u, l in zip(up, lat)]
    fits = m.fit_camera(labels, distortion=True, free_principal_point=True, max_iter=60)
    yaw, info = m.align_yaw(list(crops), fits, return_info=True)
    e = np.abs(wrap180(yaw.cpu().numpy() - TRUE_YAW)).max()
    print(f"model method on fitted cameras: yaws within {e:.4f} deg of the truth; fitted xi {[round(float(f['pred_xi']), 4) for f in fits]}")
    assert info["linked"].all() and e <= 0.5
    out = m.compose_panorama(crops, fits, yaw=yaw, height=32, width=64)
    assert out.shape == (1, 32, 64, 3) and out.dtype == torch.uint8
    with pytest.raises(PfError, match="fit_camera"):
        m.align_yaw(list(crops), labels)
    with pytest.raises(ValueError):
        m.align_yaw(list(crops), fits, mode="rad")
