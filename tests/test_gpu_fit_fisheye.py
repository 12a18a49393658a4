"""The fisheye lens fit on the GPU (include/pf_hip.h pf_fit_fisheye, fit_fisheye_lens, fisheye_lens_from_fit, PerspectiveFields.fit_fisheye) against
the fp64 reference of tests/test_fit_fisheye_ref.py: exact input from the blind start, the count of valid pixels, noisy input against the reference
fit, bitwise behaviour, degenerate input, the frame -> fit -> lens -> fields -> errors chain and the model-level entry.

Sizes: 48 x 64 takes the vector loads; 33 x 47 has n % 4 != 0 (scalar loads) and both sides odd, so the centre pixel of a centred lens sits at r = 0
at the blind start; 8 x 8 is the minimum; 97 x 131 is one more odd size with more than one accumulate block.

Bounds.  roll / pitch: the project's round-trip bound, 5e-3 deg.  f (relative), cx / cy and k1 / k2 (absolute): 4 x the worst error measured on an
MI355X over all cases, rounded up to one significant digit (the measured figures are in DESIGN.md section 37), under the ceilings 1e-3, 2e-4 and
5e-3.  The chain: 4 x measured under the project's 0.05 deg; measured 0 (the fitted lens row has the true row's float32 bits), so it is exact.  fit_cost against the fp64 cost: 4 x measured under 1e-5 relative.  Every test prints
its worst figures before it asserts.  The cases with a free principal point run with max_iter = 60, as those of the other two fits do."""
import ctypes

import numpy as np
import pytest
import torch

from tests.test_fisheye_ref import EQUIDISTANT, KIND_NAMES
from tests.test_fit_fisheye_ref import (FREE_FLAGS, FREE_SETS, KINDS, SIZE, TMAX, TMAX_DEG, TRUTHS, case_fields, cost, lens_model, noisy_case, noisy_reference,
                                        valid_pixels)

pytestmark = pytest.mark.gpu

ANGLE_BOUND = 5e-3                                          # degrees, roll and pitch
CEIL_F, CEIL_PP, CEIL_K, CEIL_CHAIN, CEIL_COST = 1e-3, 2e-4, 5e-3, 0.05, 1e-5
# 4 x the measured worst, one significant digit, rounded up
BOUND_F, BOUND_PP, BOUND_K = 6e-7, 3e-7, 6e-7               # f relative (measured 1.3e-7), cx / cy (6.3e-8), k1 / k2 (1.3e-7)
BOUND_COST = 4e-6                                           # fit_cost relative (measured 9.2e-7)
# The chain, measured: up_max 0, lat_max 0 and a crop difference of 0.  The fitted row (F 14.06069326, centre 24.29999945, 23.60000087 against 14.060694,
# 24.3, 23.6; roll and pitch to 1e-8 rad) rounds to the float32 bits of the true row, so fisheye_fields and crop_fisheye are given the same lens:
# 4 x 0 is 0, and the three comparisons are exact.
BOUND_CHAIN_UP, BOUND_CHAIN_LAT = 0.0, 0.0                  # degrees
BOUND_CROP = 0.0                                            # of the float32 frame's range of 255
assert BOUND_F <= CEIL_F and BOUND_PP <= CEIL_PP and BOUND_K <= CEIL_K and max(BOUND_CHAIN_UP, BOUND_CHAIN_LAT) <= CEIL_CHAIN and BOUND_COST <= CEIL_COST
SIZES = (SIZE, (33, 47))
MAX_ITER = {3: 20, "5k": 20, "5pp": 60, 7: 60}


def to_gpu(up, lat):
    return torch.tensor(np.asarray(up), dtype=torch.float32, device="cuda"), torch.tensor(np.asarray(lat), dtype=torch.float32, device="cuda")


def fit(ups, lats, kind, free, **kw):
    from perspectivefields_amd import fit_fisheye_lens

    pp, poly = FREE_FLAGS[free]
    kw.setdefault("max_iter", MAX_ITER[free])
    return fit_fisheye_lens(ups, lats, projection=KIND_NAMES[kind], free_principal_point=pp, distortion=poly, max_fov=2 * TMAX_DEG, **kw)


def theta_of(d):
    return np.array([np.radians(float(d["pred_roll"])), np.radians(float(d["pred_pitch"]))] + [float(d[k]) for k in ("pred_rel_focal", "pred_rel_cx", "pred_rel_cy",
                                                                                                                     "pred_k1", "pred_k2")])


def init_of(th):
    return dict(pred_roll=np.degrees(th[0]), pred_pitch=np.degrees(th[1]), pred_rel_focal=th[2], pred_rel_cx=th[3], pred_rel_cy=th[4], pred_k1=th[5], pred_k2=th[6])


def errors(th, d):
    """(roll, pitch [deg], f relative, cx, cy, k1, k2 absolute)"""
    e = np.abs(theta_of(d) - th)
    e[:2] = np.degrees(e[:2])
    e[2] /= th[2]
    return e


@pytest.mark.parametrize("free", tuple(FREE_SETS))
@pytest.mark.parametrize("kind", KINDS)
def test_exact_input_from_the_blind_start(kind, free):
    cases = [(t_i, H, W) for t_i in range(3) for H, W in SIZES]
    fields = [case_fields(t_i, free, kind, H, W) for t_i, H, W in cases]
    ups, lats = zip(*[to_gpu(up, lat) for _, up, lat in fields])
    res = fit(list(ups), list(lats), kind, free)
    err = np.array([errors(th, d) for (th, _, _), d in zip(fields, res)])
    its = [int(d["fit_iterations"]) for d in res]
    print(f"\nexact {KIND_NAMES[kind]} free {free}: steps {its}; worst roll/pitch {err[:, :2].max():.2e} deg, f rel {err[:, 2].max():.2e}, "
          f"cx/cy {err[:, 3:5].max():.2e}, k1/k2 {err[:, 5:].max():.2e}")
    for (th, up, lat), d in zip(fields, res):
        assert set(d) == {"pred_roll", "pred_pitch", "pred_rel_focal", "pred_rel_cx", "pred_rel_cy", "pred_k1", "pred_k2", "fit_rms_up_deg", "fit_rms_lat_deg",
                          "fit_cost", "fit_iterations", "fit_converged", "fit_valid_pixels", "fit_projection", "fit_max_fov"}
        assert all(v.is_cuda and v.dim() == 0 for k, v in d.items() if k not in ("fit_projection", "fit_max_fov"))
        held = [k for k in range(7) if k not in FREE_SETS[free]]
        assert (theta_of(d)[held] == 0).all()   # what is not free keeps its start value
    bad = [(c, e, n) for c, e, n in zip(cases, err, its) if e[:2].max() > ANGLE_BOUND or e[2] > BOUND_F or e[3:5].max() > BOUND_PP or e[5:].max() > BOUND_K]
    assert not bad, bad


@pytest.mark.parametrize("kind", KINDS)
def test_valid_pixels_are_the_reference_count_on_the_fov_170_cases(kind):
    for free in FREE_SETS:
        fields = [case_fields(1, free, kind, H, W) for H, W in SIZES]
        ups, lats = zip(*[to_gpu(up, lat) for _, up, lat in fields])
        res = fit(list(ups), list(lats), kind, free)
        for (th, up, lat), d in zip(fields, res):
            want = valid_pixels(th, kind, up, lat)
            assert 0 <= np.isfinite(lat).sum() - want <= 1   # the centre pixel of the centred cases at 33 x 47, nothing else
            assert int(d["fit_valid_pixels"]) == want, (kind, free, lat.shape, int(d["fit_valid_pixels"]), want)


@pytest.mark.parametrize("free", tuple(FREE_SETS))
def test_noisy_input_ends_no_higher_than_the_reference_fit(free):
    th, up, lat = noisy_case()
    ref, c_ref = noisy_reference(free)
    u, l = to_gpu(up, lat)
    d = fit(u, l, EQUIDISTANT, free, init=init_of(th), max_iter=100)
    got = theta_of(d)
    c_gpu = cost(got, EQUIDISTANT, up, lat)
    rel = abs(float(d["fit_cost"]) - c_gpu) / c_gpu
    print(f"\nnoisy free {free}: steps {int(d['fit_iterations'])}, fp64 cost at the GPU's theta {c_gpu:.9g}, reference {c_ref:.9g} (ratio - 1 = {c_gpu / c_ref - 1:.2e}), "
          f"fit_cost rel diff {rel:.2e}, theta - reference {np.abs(got - ref).max():.2e}")
    assert c_gpu <= c_ref * (1 + 1e-6)
    assert rel <= BOUND_COST
    assert int(d["fit_valid_pixels"]) == int((np.isfinite(up).all(0) & np.isfinite(lat)).sum())


def _mixed_batch():
    """40 images of the four sizes, every truth, the full lenses: two launch groups"""
    sizes = (SIZE, (33, 47), (8, 8), (97, 131))
    out = []
    for k in range(40):
        H, W = sizes[k % 4]
        _, up, lat = case_fields(k % 3, 7, EQUIDISTANT, H, W)
        out.append(to_gpu(up, lat))
    return out


def test_mixed_batch_is_bitwise_per_image_permutable_and_repeatable():
    fields = _mixed_batch()
    ups, lats = [u for u, _ in fields], [l for _, l in fields]
    perm = np.random.default_rng(5).permutation(len(fields))
    for free, kw in ((3, {}), (7, {"loss": "huber"})):
        batch = fit(ups, lats, EQUIDISTANT, free, **kw)
        again = fit(ups, lats, EQUIDISTANT, free, **kw)
        mixed = fit([ups[i] for i in perm], [lats[i] for i in perm], EQUIDISTANT, free, **kw)
        keys = [k for k in batch[0] if k not in ("fit_projection", "fit_max_fov")]
        for j, i in enumerate(perm):
            assert all(torch.equal(mixed[j][k], batch[i][k]) for k in keys), (free, i)
        for i in range(len(fields)):
            one = fit(ups[i], lats[i], EQUIDISTANT, free, **kw)
            for k in keys:
                assert torch.equal(one[k], batch[i][k]) and torch.equal(again[i][k], batch[i][k]), (free, i, k)


def _raw_fit(up, lat, kind, free_pp, poly, init=None):
    """pf_fit_fisheye through ctypes on planes wherever they are: the output row"""
    from perspectivefields_amd.engine import _check, _stream_ptr, load_library

    lib = load_library()
    H, W = lat.shape
    hw = (ctypes.c_int32 * 2)(H, W)
    ws_n = int(lib.pf_fit_fisheye_workspace_bytes(1, hw))
    ws = torch.empty(ws_n, dtype=torch.uint8, device="cuda")
    out = torch.empty((1, 15), dtype=torch.float32, device="cuda")
    _check(lib.pf_fit_fisheye(0, kind, 1, hw, (ctypes.c_void_p * 1)(up.data_ptr()), (ctypes.c_void_p * 1)(lat.data_ptr()), None if init is None else init.data_ptr(),
                              free_pp, poly, float(np.float32(TMAX)), 0, 2.0, 1.0, 1.0, 20, out.data_ptr(), ws.data_ptr(), ws_n, _stream_ptr()), None, "pf_fit_fisheye")
    return out[0].clone()


@pytest.mark.parametrize("kind", KINDS)
def test_planes_shifted_by_one_float_take_the_scalar_loads_and_give_the_same_bits(kind):
    H, W = SIZE
    _, up, lat = case_fields(1, 7, kind, H, W)
    u, l = to_gpu(up, lat)
    assert u.data_ptr() % 16 == 0 and l.data_ptr() % 16 == 0 and (H * W) % 4 == 0
    bu, bl = torch.empty(2 * H * W + 4, device="cuda"), torch.empty(H * W + 4, device="cuda")
    su, sl = bu[1:1 + 2 * H * W].view(2, H, W), bl[1:1 + H * W].view(H, W)
    su.copy_(u)
    sl.copy_(l)
    assert su.data_ptr() % 16 == 4 and sl.data_ptr() % 16 == 4
    for free_pp, poly in ((0, 0), (1, 1)):
        a, b = _raw_fit(u, l, kind, free_pp, poly), _raw_fit(su, sl, kind, free_pp, poly)
        assert torch.equal(a, b), (kind, free_pp, poly, a, b)
        if free_pp:   # the full fit is at the truth
            assert abs(float(a[0]) - TRUTHS[1][0][0]) <= ANGLE_BOUND and abs(float(a[1]) - TRUTHS[1][0][1]) <= ANGLE_BOUND, a


def test_degenerate_inputs():
    from perspectivefields_amd import fit_fisheye_lens
    from perspectivefields_amd.engine import PfError

    H, W = SIZE
    fields = [case_fields(t_i, 7, EQUIDISTANT, H, W) for t_i in range(3)]
    ups, lats = [list(x) for x in zip(*[to_gpu(up, lat) for _, up, lat in fields])]
    nan_u, nan_l = torch.full_like(ups[1], float("nan")), torch.full_like(lats[1], float("nan"))
    keys = ("pred_roll", "pred_pitch", "pred_rel_focal", "pred_rel_cx", "pred_rel_cy", "pred_k1", "pred_k2", "fit_cost", "fit_iterations", "fit_converged", "fit_valid_pixels")
    # an image without a finite pixel between two others: from the blind start and from a given one
    good = fit(ups, lats, EQUIDISTANT, 7)
    dead = fit([ups[0], nan_u, ups[2]], [lats[0], nan_l, lats[2]], EQUIDISTANT, 7)
    for i in (0, 2):
        assert all(torch.equal(dead[i][k], good[i][k]) for k in keys), i
    d = dead[1]
    assert not bool(d["fit_converged"]) and int(d["fit_valid_pixels"]) == 0 and int(d["fit_iterations"]) == 0
    assert [float(d[k]) for k in ("pred_roll", "pred_pitch", "pred_rel_cx", "pred_rel_cy", "pred_k1", "pred_k2")] == [0.0] * 6 and np.isfinite(float(d["pred_rel_focal"]))
    starts = [init_of(th * (1 + 0.01 * k)) for k, (th, _, _) in enumerate(fields)]
    good = fit(ups, lats, EQUIDISTANT, 7, init=starts)
    dead = fit([ups[0], nan_u, ups[2]], [lats[0], nan_l, lats[2]], EQUIDISTANT, 7, init=starts)
    for i in (0, 2):
        assert all(torch.equal(dead[i][k], good[i][k]) for k in keys), i
    d = dead[1]
    assert not bool(d["fit_converged"]) and int(d["fit_valid_pixels"]) == 0
    want = np.array([starts[1][k] for k in keys[:7]], dtype=np.float32)
    assert np.allclose(np.array([float(d[k]) for k in keys[:7]], dtype=np.float32), want, rtol=1e-6, atol=0)
    # a start with a non-finite entry: the same, and the neighbours do not see it
    for k in ("pred_rel_focal", "pred_roll", "pred_k2"):
        bad = [dict(s) for s in starts]
        bad[1][k] = float("nan") if k != "pred_roll" else float("inf")
        res = fit(ups, lats, EQUIDISTANT, 7, init=bad)
        for i in (0, 2):
            assert all(torch.equal(res[i][q], good[i][q]) for q in keys), (k, i)
        d = res[1]
        assert not bool(d["fit_converged"]) and int(d["fit_valid_pixels"]) == 0 and not np.isfinite(float(d[k])), (k, d)
        rest = [q for q in keys[:7] if q != k]
        assert np.allclose([float(d[q]) for q in rest], [np.float32(bad[1][q]) for q in rest], rtol=1e-6, atol=0), (k, d)
    # the truth with f off by 10 % returns to the truth
    for (th, _, _), u, l in zip(fields, ups, lats):
        st = th.copy()
        st[2] *= 1.1
        e = errors(th, fit(u, l, EQUIDISTANT, 7, init=init_of(st)))
        print(f"\nf off by 10 %: errors {e}")
        assert e[:2].max() <= ANGLE_BOUND and e[2] <= BOUND_F and e[3:5].max() <= BOUND_PP and e[5:].max() <= BOUND_K, e
    with pytest.raises(PfError):
        fit_fisheye_lens(torch.zeros((2, 7, 64), device="cuda"), torch.zeros((7, 64), device="cuda"))


def test_the_chain_frame_fit_lens_fields_errors_closes():
    from perspectivefields_amd import crop_fisheye, field_errors, fisheye_fields, fisheye_lens, fisheye_lens_from_fit, fit_fisheye_lens, panorama_to_fisheye

    H = W = 48
    rng = np.random.default_rng(3)
    pano = torch.from_numpy(rng.integers(0, 256, (32, 64, 3), dtype=np.uint8)).cuda()
    pano = torch.nn.functional.avg_pool2d(pano.permute(2, 0, 1)[None].float(), 5, 1, 2, count_include_pad=False)[0].permute(1, 2, 0).contiguous()   # smooth, float32
    lens = fisheye_lens(185.0, radius=22.7, center=(24.3, 23.6), roll=10.0, pitch=-25.0)   # nothing of it is a float32: the fitted row differs in its bits
    frame, up, lat = panorama_to_fisheye(pano, lens, height=H, width=W, fields=True)
    d = fit_fisheye_lens(up[0], lat[0], free_principal_point=True, max_iter=60)
    row = fisheye_lens_from_fit(d, height=H, width=W, fov=185.0)
    print(f"\nchain: true lens {lens[[0, 1, 3, 4, 5]]}, fitted {row[[0, 1, 3, 4, 5]]}, steps {int(d['fit_iterations'])}")
    u2, l2 = fisheye_fields(row, height=H, width=W)
    e = field_errors(u2[0], l2[0], up[0], lat[0])
    n_lab = int(torch.isfinite(lat[0]).sum())
    print(f"chain: up_max {float(e['up_max_deg']):.3e} deg, lat_max {float(e['lat_max_deg']):.3e} deg over {int(e['valid_pixels'])} of {n_lab} labelled pixels")
    assert n_lab - int(e["valid_pixels"]) <= 8   # the rim, where the two circles differ by rounding, and a zenith / nadir pixel
    assert float(e["up_max_deg"]) <= BOUND_CHAIN_UP and float(e["lat_max_deg"]) <= BOUND_CHAIN_LAT
    # the frame undistorted along the lens axis with the fitted lens and with the true one
    kw = dict(roll=10.0, pitch=-25.0, rel_focal=0.8, height=24, width=24, fields=False, return_mask=True)
    a, _, _, ma = crop_fisheye(frame[0], row, **kw)
    b, _, _, mb = crop_fisheye(frame[0], lens, **kw)
    both = (ma & mb)[0]
    diff = float((a[0] - b[0]).abs()[both].max())
    print(f"chain: 24 x 24 view along the axis, max difference {diff:.3e} grey levels over {int(both.sum())} pixels")
    assert int(both.sum()) == 24 * 24 and diff <= BOUND_CROP


def test_model_fit_fisheye_with_a_circle_mask():
    from perspectivefields_amd import PerspectiveFields
    from perspectivefields_amd.synth import synthetic_image

    sizes = [(96, 96), (97, 131)]
    model = PerspectiveFields("PersNet-360Cities", weights="synthetic:0").eval().to("cuda:0")
    preds = model.inference_batch([synthetic_image(h, w, seed=41 + k) for k, (h, w) in enumerate(sizes)])
    before = [dict(p) for p in preds]
    masks = []
    for h, w in sizes:
        y, x = np.mgrid[0:h, 0:w]
        masks.append(np.hypot(x + 0.5 - w / 2, y + 0.5 - h / 2) < 0.48 * min(h, w))
    fits = model.fit_fisheye(preds, valid=masks, projection="equisolid", distortion=True)
    for p, q in zip(preds, before):   # the inference results are left as they were
        assert p.keys() == q.keys() and all(p[k] is q[k] for k in p)
    for d, m in zip(fits, masks):
        assert all(np.isfinite(float(d[k])) for k in d if k.startswith("pred_") or k in ("fit_cost", "fit_rms_up_deg", "fit_rms_lat_deg")), d
        assert 0 < int(d["fit_valid_pixels"]) <= int(m.sum())
        print(f"\nmodel: f {float(d['pred_rel_focal']):.4f}, k1 {float(d['pred_k1']):.4f}, valid {int(d['fit_valid_pixels'])} of {int(m.sum())}, steps {int(d['fit_iterations'])}")
    one = model.fit_fisheye(preds[0], valid=torch.from_numpy(masks[0]).cuda())
    assert isinstance(one, dict) and "pred_k1" in one and int(one["fit_valid_pixels"]) <= int(masks[0].sum())
    with pytest.raises(ValueError):
        model.fit_fisheye(preds, valid=masks[:1])
