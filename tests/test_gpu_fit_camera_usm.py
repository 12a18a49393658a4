"""Unified Spherical Model camera fit and field synthesis on the GPU (include/pf_hip.h pf_fit_camera_usm / pf_fields_from_params_usm,
fit_camera_params(distortion=True), fields_from_params(xi=)) against the fp64 reference of tests/test_fit_camera_usm_ref.py: exact
round trips, stationarity on noisy input, free principal point, xi > 1 from a supplied start, bitwise behaviour, field synthesis, the
crop -> fit -> fields -> errors chain and the model-level entry.

Bounds.  roll / pitch: the project's round-trip bound, 5e-3 deg.  f / (1 + xi), f and xi: 4 x the worst error measured on an MI355X over
the whole grid, rounded up to one significant digit (the measured figures are in DESIGN.md section 14), under the ceilings 1e-3 / 5e-3 /
5e-3 -- the scatter of the fp64 optimum under 1 deg noise, beyond which a fit of exact input is not working.  Every test prints its
worst figures before it asserts.  Largest step count seen in the round trip at the default max_iter: 20 (all of it; mean 17.5 - 17.9): the
parameters are in place as early as in the fp64 reference (<= 9 steps), after which the accept / reject rule works on fp32 rounding noise."""
import itertools

import numpy as np
import pytest
import torch

from tests.test_fit_camera_usm_ref import (GRID, SIZES, focal_of, reference_fit, usm_cost, usm_fields, usm_valid_pixels)
from tests.test_pano_crop_ref import labels, pixel_rays

pytestmark = pytest.mark.gpu

ANGLE_BOUND = 5e-3                                     # degrees, roll and pitch
CEIL_MAG, CEIL_F, CEIL_XI, CEIL_PP, CEIL_CHAIN = 1e-3, 5e-3, 5e-3, 2e-3, 0.05
# 4 x the measured worst, one significant digit, rounded up
BOUND_MAG, BOUND_F, BOUND_XI = 2e-6, 2e-5, 2e-5        # f / (1 + xi) relative (measured 4.7e-7), f relative (3.3e-6), xi absolute (3.7e-6)
BOUND_PP = 2e-4                                        # rel_cx / rel_cy: the project's bound of the pinhole fit
BOUND_CHAIN_UP, BOUND_CHAIN_LAT = 8e-5, 7e-5           # degrees (measured 1.9e-5 and 1.6e-5)
assert BOUND_MAG <= CEIL_MAG and BOUND_F <= CEIL_F and BOUND_XI <= CEIL_XI and BOUND_PP <= CEIL_PP and max(BOUND_CHAIN_UP, BOUND_CHAIN_LAT) <= CEIL_CHAIN


def upload(case, H, W):
    r, p, f, cx, cy, xi = case
    up, lat = usm_fields((np.radians(r), np.radians(p), f, cx, cy, xi), H, W)
    return torch.from_numpy(up).float().cuda(), torch.from_numpy(lat).float().cuda()


def fit_many(cases, H, W, chunk=40, **kw):
    """cases: [(roll, pitch [deg], rel_focal, rel_cx, rel_cy, xi)] -> the fit dicts as host floats"""
    from perspectivefields_amd import fit_camera_params

    out = []
    for i0 in range(0, len(cases), chunk):
        ups, lats = zip(*[upload(c, H, W) for c in cases[i0:i0 + chunk]])
        res = fit_camera_params(list(ups), list(lats), distortion=True, **kw)
        out += [{k: float(v) for k, v in d.items()} for d in res]
    return out


def errors(case, d):
    """(roll, pitch [deg], f / (1 + xi) relative, f relative, xi absolute, cx, cy absolute)"""
    r, p, f, cx, cy, xi = case
    mag, mag_t = d["pred_rel_focal"] / (1 + d["pred_xi"]), f / (1 + xi)
    return np.array([abs(d["pred_roll"] - r), abs(d["pred_pitch"] - p), abs(mag - mag_t) / mag_t, abs(d["pred_rel_focal"] - f) / f, abs(d["pred_xi"] - xi),
                     abs(d["pred_rel_cx"] - cx), abs(d["pred_rel_cy"] - cy)])


def report(what, cases, res):
    err = np.array([errors(c, d) for c, d in zip(cases, res)])
    its = np.array([d["fit_iterations"] for d in res])
    print(f"\n{what}: steps mean {its.mean():.2f} max {its.max():.0f}; converged {sum(d['fit_converged'] for d in res):.0f} of {len(res)}")
    for k, name in enumerate(("roll deg", "pitch deg", "f/(1+xi) rel", "f rel", "xi abs", "cx abs", "cy abs")):
        i = int(err[:, k].argmax())
        print(f"  worst {name:13s} {err[i, k]:.3e} at (roll, pitch, f, cx, cy, xi) = {tuple(round(float(v), 4) for v in cases[i])} after {its[i]:.0f} steps")
    return err


@pytest.mark.parametrize("H,W", SIZES)
def test_round_trip_exact_input(H, W):
    res = fit_many(GRID, H, W)
    err = report(f"round trip {H} x {W}", GRID, res)
    assert all(d["fit_valid_pixels"] == H * W for d in res)
    bad = [(c, e, d["fit_iterations"]) for c, e, d in zip(GRID, err, res)
           if max(e[:2]) > ANGLE_BOUND or e[2] > BOUND_MAG or e[3] > BOUND_F or e[4] > BOUND_XI]
    assert not bad, bad[:6]


def _noisy(case, H, W, seed, sd_deg=1.0):
    """the case's fields with the up vector rotated and the latitude shifted by Gaussian noise"""
    rng = np.random.default_rng(seed)
    r, p, f, cx, cy, xi = case
    up, lat = usm_fields((np.radians(r), np.radians(p), f, cx, cy, xi), H, W)
    ang = np.radians(rng.normal(0.0, sd_deg, (H, W)))
    c, s = np.cos(ang), np.sin(ang)
    return np.stack([c * up[0] - s * up[1], s * up[0] + c * up[1]]), lat + rng.normal(0.0, sd_deg, (H, W))


def _theta(d):
    return np.array([np.radians(float(d["pred_roll"])), np.radians(float(d["pred_pitch"])), float(d["pred_rel_focal"]), float(d["pred_rel_cx"]),
                     float(d["pred_rel_cy"]), float(d["pred_xi"])])


def test_fit_of_noisy_input_is_a_stationary_point_of_the_fp64_objective():
    from perspectivefields_amd import fit_camera_params

    rng = np.random.default_rng(21)
    picks = [GRID[k] for k in rng.choice(len(GRID), 8, replace=False)]
    sizes = [SIZES[1 + k % 2] for k in range(8)]
    fields = [_noisy(c, H, W, 100 + k) for k, (c, (H, W)) in enumerate(zip(picks, sizes))]
    fits = fit_camera_params([torch.from_numpy(u).float().cuda() for u, _ in fields], [torch.from_numpy(l).float().cuda() for _, l in fields],
                             distortion=True, loss="l2", max_iter=100)
    for c, (up, lat), d in zip(picks, fields, fits):
        up, lat = up.astype(np.float32), lat.astype(np.float32)   # what the GPU saw
        th = _theta(d)
        c_gpu = usm_cost(th, up, lat)
        _, s = reference_fit(up, lat, th)
        print(f"\nnoisy {c}: steps {int(d['fit_iterations'])}, fit_cost rel diff {abs(float(d['fit_cost']) - c_gpu) / c_gpu:.2e}, "
              f"scipy lowers the cost by {(c_gpu - s.cost) / c_gpu:.2e} relative")
        assert abs(float(d["fit_cost"]) - c_gpu) <= 1e-4 * c_gpu, (c, d)
        assert c_gpu - s.cost < 1e-4 * c_gpu, (c, d, s.x, s.cost)


@pytest.mark.parametrize("H,W", SIZES)
def test_free_principal_point(H, W):
    rng = np.random.default_rng(H * 7 + W)
    cases = []
    for cx, cy in itertools.product((-0.1, 0.0, 0.08), repeat=2):
        for k in rng.choice(len(GRID), 6, replace=False):
            r, p, f, _, _, xi = GRID[k]
            cases.append((r, p, f, cx, cy, xi))
    res = fit_many(cases, H, W, free_principal_point=True, max_iter=60)
    err = report(f"free principal point {H} x {W}", cases, res)
    assert all(d["fit_valid_pixels"] == H * W for d in res)
    bad = [(c, e, d["fit_iterations"]) for c, e, d in zip(cases, err, res)
           if max(e[:2]) > ANGLE_BOUND or e[2] > BOUND_MAG or e[3] > BOUND_F or e[4] > BOUND_XI or max(e[5:]) > BOUND_PP]
    assert not bad, bad[:6]


@pytest.mark.parametrize("roll,pitch", [(40.0, 60.0), (0.0, 0.0), (-20.0, -35.0)])
def test_xi_above_1_from_a_supplied_start(roll, pitch):
    from perspectivefields_amd import fit_camera_params
    from tests.test_gpu_pano_crop import clear_of_the_no_ray_circle

    H, W = 97, 131
    case = (roll, pitch, 0.5, 0.0, 0.0, 1.2)
    u, l = upload(case, H, W)
    start = {"pred_roll": roll, "pred_pitch": pitch, "pred_rel_focal": 0.5 * 1.1, "pred_xi": 1.2 * 1.1}
    d = {k: float(v) for k, v in fit_camera_params(u, l, distortion=True, init=start).items()}
    truth = (np.radians(roll), np.radians(pitch), 0.5, 0.0, 0.0, 1.2)
    n_ref = usm_valid_pixels(truth, u.cpu().numpy(), l.cpu().numpy())
    th7 = (truth[0], truth[1], 0.0, 0.5, 0.0, 0.0, 1.2)
    hair = int((~clear_of_the_no_ray_circle(th7, H, W)).sum() + (~clear_of_the_no_ray_circle(th7, H, W, linspace=True)).sum())
    e = errors(case, d)
    print(f"\nxi = 1.2 at ({roll}, {pitch}): steps {d['fit_iterations']:.0f}, converged {d['fit_converged']:.0f}, valid {d['fit_valid_pixels']:.0f} "
          f"(reference {n_ref} of {H * W}, hair {hair}), errors {e[:5]}")
    assert 0.02 * H * W < H * W - n_ref < 0.05 * H * W   # about 3 % of the pixels have no ray
    # converged: at the truth, with no residual left.  (fit_converged says that a stopping tolerance was met; on exact input the fp32 cost
    # floor can keep the accept / reject rule busy for all of max_iter, with the parameters long since in place -- DESIGN.md section 14.)
    assert d["fit_rms_up_deg"] <= 1e-3 and d["fit_rms_lat_deg"] <= 1e-3, d
    assert abs(d["fit_valid_pixels"] - n_ref) <= hair
    assert max(e[:2]) <= ANGLE_BOUND and e[2] <= CEIL_MAG and e[3] <= CEIL_F and e[4] <= CEIL_XI, e


def test_mixed_batch_is_bitwise_per_image_and_repeatable():
    from perspectivefields_amd import fit_camera_params

    sizes = [SIZES[k % 3] if k % 9 == 0 else (40 + 3 * k, 57 + 5 * k) for k in range(40)]   # 40 images: two launch groups
    ups, lats = [], []
    for k, (H, W) in enumerate(sizes):
        xi = (0.0, 0.3, 0.7, 1.0)[k % 4]
        u, l = upload((-20 + 2 * k, 35 - 2.5 * k, focal_of(50 + 1.5 * k, xi), 0.0, 0.0, xi), H, W)
        ups.append(u)
        lats.append(l)
    for kw in ({}, {"free_principal_point": True, "loss": "huber"}):
        batch = fit_camera_params(ups, lats, distortion=True, **kw)
        again = fit_camera_params(ups, lats, distortion=True, **kw)
        for i in range(len(sizes)):
            one = fit_camera_params(ups[i], lats[i], distortion=True, **kw)
            assert "pred_xi" in one
            for k in one:
                assert torch.equal(one[k], batch[i][k]) and torch.equal(again[i][k], batch[i][k]), (i, sizes[i], k)


def test_the_pinhole_fit_is_unchanged_by_the_keyword():
    from perspectivefields_amd import fit_camera_params
    from tests.test_gpu_fit_camera import SIZES as PIN_SIZES
    from tests.test_gpu_fit_camera import upload as pin_upload

    sizes = [PIN_SIZES[k % 4] if k % 9 == 0 else (40 + 3 * k, 57 + 5 * k) for k in range(35)]   # the inputs of the pinhole fit's batch test
    ups, lats = zip(*[pin_upload((np.radians(-20 + 2 * k), np.radians(35 - 3 * k), 0.5 + 0.03 * k, 0.0, 0.0), H, W) for k, (H, W) in enumerate(sizes)])
    a = fit_camera_params(list(ups), list(lats), distortion=False)
    b = fit_camera_params(list(ups), list(lats))
    for x, y in zip(a, b):
        assert "pred_xi" not in x and x.keys() == y.keys() and len(x) == 13
        assert all(torch.equal(x[k], y[k]) for k in x)


@pytest.mark.parametrize("xi", [0.3, 0.8, 1.2, 1.6])
def test_usm_fields_match_the_fp64_reference(xi):
    from perspectivefields_amd import fields_from_params
    from tests.test_gpu_pano_crop import LABEL_CASES, clear_of_the_no_ray_circle, theta_rad

    H, W = 45, 60
    holes = 0
    for r, p, y, f, cx, cy in LABEL_CASES:
        c = (r, p, y, f * 0.6, cx, cy, xi)
        up, lat = fields_from_params(r, p, f * 0.6, cx, cy, H, W, xi=torch.tensor(xi, device="cuda") if r > 0 else xi)
        up, lat = up.cpu().numpy().astype(np.float64), lat.cpu().numpy().astype(np.float64)
        th = theta_rad(*c)
        up_r, lat_r = labels(th, H, W)
        _, ok = pixel_rays(th, H, W)
        clear = clear_of_the_no_ray_circle(th, H, W)
        assert np.array_equal(np.isnan(up[0])[clear], ~ok[clear]) and np.array_equal(np.isnan(up[1])[clear], ~ok[clear]), c
        m = ok & clear
        cos = (up[:, m] * up_r[:, m]).sum(0)
        assert (1 - cos).max() <= 1e-6, (c, (1 - cos).max())
        clear_l = clear_of_the_no_ray_circle(th, H, W, linspace=True)
        ml = np.isfinite(lat_r)
        assert np.array_equal(np.isnan(lat)[clear_l], ~ml[clear_l]), c
        lm = ml & clear_l
        assert np.abs(lat[lm] - lat_r[lm]).max() <= 2e-3, c
        holes += int(np.isnan(up).any() and np.isnan(lat).any())
    assert (holes > 0) == (xi > 1)


@pytest.mark.parametrize("H,W", [(48, 64), (31, 47)])
def test_a_device_xi_of_zero_gives_the_pinhole_bits(H, W):
    from perspectivefields_amd import fields_from_params
    from tests.test_gpu_pano_crop import LABEL_CASES

    for r, p, _, f, cx, cy in LABEL_CASES:
        up0, lat0 = fields_from_params(r, p, f, cx, cy, H, W, xi=0.0)
        up1, lat1 = fields_from_params(r, p, f, cx, cy, H, W, xi=torch.zeros((), device="cuda"))
        up2, lat2 = fields_from_params(r, p, f, cx, cy, H, W)
        assert torch.equal(up0, up1) and torch.equal(lat0, lat1) and torch.equal(up0, up2) and torch.equal(lat0, lat2), (r, p, f, cx, cy)


def test_the_chain_closes_for_distorted_views():
    from perspectivefields_amd import crop_panorama, field_errors, fields_from_params, fit_camera_params

    H, W, xi = 240, 320, 0.6
    cams = [(12.0, 35.0, 55.0), (-30.0, -20.0, 90.0), (5.0, 0.5, 120.0)]
    pano = torch.zeros((64, 128, 3), dtype=torch.uint8, device="cuda")
    _, up, lat = crop_panorama(pano, [c[0] for c in cams], [c[1] for c in cams], [focal_of(c[2], xi) for c in cams], xi=xi, height=H, width=W)
    fits = fit_camera_params(list(up), list(lat), distortion=True)
    pin = fit_camera_params(list(up), list(lat), distortion=False)
    for k, (c, d, q) in enumerate(zip(cams, fits, pin)):
        u2, l2 = fields_from_params(d["pred_roll"], d["pred_pitch"], d["pred_rel_focal"], d["pred_rel_cx"], d["pred_rel_cy"], H, W, xi=d["pred_xi"])
        e = field_errors(u2, l2, up[k], lat[k])
        print(f"\nchain {c}: xi {float(d['pred_xi']):.6f}, up_max {float(e['up_max_deg']):.3e} deg, lat_max {float(e['lat_max_deg']):.3e} deg, "
              f"rms_up USM {float(d['fit_rms_up_deg']):.3e} pinhole {float(q['fit_rms_up_deg']):.3e}")
        assert int(e["valid_pixels"]) == H * W
        assert float(e["up_max_deg"]) <= BOUND_CHAIN_UP and float(e["lat_max_deg"]) <= BOUND_CHAIN_LAT, (c, e)
        assert float(q["fit_rms_up_deg"]) >= 10 * float(d["fit_rms_up_deg"]), (c, q, d)


@pytest.mark.parametrize("version", ["PersNet-360Cities", "Paramnet-360Cities-edina-centered"])
def test_model_fit_camera_with_distortion(version):
    from perspectivefields_amd import PerspectiveFields
    from perspectivefields_amd.synth import synthetic_image

    sizes = [(320, 320), (97, 131)]
    model = PerspectiveFields(version, weights="synthetic:0").eval().to("cuda:0")
    preds = model.inference_batch([synthetic_image(h, w, seed=31 + k) for k, (h, w) in enumerate(sizes)])
    before = [dict(p) for p in preds]
    kws = [{}] + ([{"init": "paramnet"}] if model.param_on else [])
    for kw in kws:
        fits = model.fit_camera(preds, distortion=True, **kw)
        for p, q in zip(preds, before):   # the inference results are left as they were
            assert p.keys() == q.keys() and all(p[k] is q[k] for k in p)
        for p, d in zip(preds, fits):
            assert "pred_xi" in d and "pred_xi" not in p
            assert d["pred_xi"].is_cuda and d["pred_xi"].dim() == 0 and -0.5 <= float(d["pred_xi"]) <= 2.0
            assert all(np.isfinite(float(v)) for v in d.values()), (version, d)
            print(f"\n{version} {kw}: xi {float(d['pred_xi']):.4f}, f {float(d['pred_rel_focal']):.4f}, valid {int(d['fit_valid_pixels'])} of "
                  f"{p['pred_latitude_original'].numel()}, steps {int(d['fit_iterations'])}")
    one = model.fit_camera(preds[0], distortion=True)
    assert isinstance(one, dict) and "pred_xi" in one
