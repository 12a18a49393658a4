"""Camera fit on the GPU (include/pf_hip.h pf_fit_camera, perspectivefields_amd.fit_camera_params) against the fp64 reference
of tests/test_fit_camera_ref.py: exact round trips, free principal point, mixed batches, robust loss, fits of network
output, ParamNet refinement and degenerate input."""
import itertools

import numpy as np
import pytest
import torch

from tests.test_fit_camera_ref import cost, general_vfov_deg, l2_residual_vector, model_fields, rms

pytestmark = pytest.mark.gpu

ROLLS = (-30.0, -5.0, 0.0, 12.0, 40.0)
PITCHES = (-70.0, -20.0, 0.0, 0.5, 35.0, 70.0)
VFOVS = (20.0, 55.0, 90.0, 120.0)
SIZES = ((640, 640), (384, 512), (1024, 1365), (97, 131))


def focal_of_vfov(vfov_deg):
    return 0.5 / np.tan(np.radians(vfov_deg) / 2)


def upload(theta, H, W):
    up, lat = model_fields(theta, H, W)
    return torch.from_numpy(up).float().cuda(), torch.from_numpy(lat).float().cuda()


def fit_many(cases, H, W, chunk=40, **kw):
    """cases: [(roll, pitch, rel_focal, rel_cx, rel_cy)] with angles in degrees -> host arrays of the fit dicts"""
    from perspectivefields_amd import fit_camera_params

    out = []
    for i0 in range(0, len(cases), chunk):
        ups, lats = zip(*[upload((np.radians(r), np.radians(p), f, cx, cy), H, W) for r, p, f, cx, cy in cases[i0:i0 + chunk]])
        res = fit_camera_params(list(ups), list(lats), **kw)
        out += [{k: float(v) for k, v in d.items()} for d in res]
    return out


@pytest.mark.parametrize("H,W", SIZES)
def test_round_trip_exact_input(H, W):
    cases = [(r, p, focal_of_vfov(v), 0.0, 0.0) for r, p, v in itertools.product(ROLLS, PITCHES, VFOVS)]
    res = fit_many(cases, H, W)
    bad = []
    for (r, p, f, _, _), d in zip(cases, res):
        v = np.degrees(2 * np.arctan(0.5 / f))
        err = (abs(d["pred_roll"] - r), abs(d["pred_pitch"] - p), abs(d["pred_vfov"] - v), abs(d["pred_rel_focal"] - f) / f)
        if max(err[:3]) > 5e-3 or err[3] > 2e-4 or d["fit_valid_pixels"] != H * W:
            bad.append(((r, p, v), err, d["fit_iterations"]))
    assert not bad, bad[:6]


@pytest.mark.parametrize("H,W", SIZES)
def test_free_principal_point(H, W):
    from perspectivefields_amd.perspectivefields import general_vfov_to_focal

    rng = np.random.default_rng(H * 7 + W)
    grid = list(itertools.product(ROLLS, PITCHES, VFOVS))
    cases = []
    for cx, cy in itertools.product((-0.1, 0.0, 0.08), repeat=2):
        for k in rng.choice(len(grid), 6, replace=False):
            r, p, v = grid[k]
            cases.append((r, p, focal_of_vfov(v), cx, cy))
    # 5 free parameters from the centre start: at a narrow FoV roll and rel_cx are nearly collinear and the start is several
    # degrees off, so these fits get more than the default 20 steps
    res = fit_many(cases, H, W, free_principal_point=True, max_iter=60)
    bad = []
    for (r, p, f, cx, cy), d in zip(cases, res):
        err = (abs(d["pred_roll"] - r), abs(d["pred_pitch"] - p), abs(d["pred_rel_focal"] - f) / f, abs(d["pred_rel_cx"] - cx),
               abs(d["pred_rel_cy"] - cy), abs(d["pred_general_vfov"] - general_vfov_deg(f, cx, cy)))
        if max(err[:2]) > 5e-3 or max(err[2:5]) > 2e-4 or err[5] > 1e-2:
            bad.append(((r, p, f, cx, cy), err, d["fit_iterations"]))
        back = float(general_vfov_to_focal(d["pred_rel_cx"], d["pred_rel_cy"], d["pred_general_vfov"]))
        assert abs(back - d["pred_rel_focal"]) <= 1e-4 * d["pred_rel_focal"]
    assert not bad, bad[:6]


def test_mixed_batch_is_bitwise_per_image_and_repeatable():
    from perspectivefields_amd import fit_camera_params

    sizes = [SIZES[k % 4] if k % 9 == 0 else (40 + 3 * k, 57 + 5 * k) for k in range(35)]   # 35 images: two launch groups
    ups, lats = [], []
    for k, (H, W) in enumerate(sizes):
        u, l = upload((np.radians(-20 + 2 * k), np.radians(35 - 3 * k), 0.5 + 0.03 * k, 0.0, 0.0), H, W)
        ups.append(u)
        lats.append(l)
    for kw in ({}, {"free_principal_point": True, "loss": "huber"}):
        batch = fit_camera_params(ups, lats, **kw)
        again = fit_camera_params(ups, lats, **kw)
        for i in range(len(sizes)):
            one = fit_camera_params(ups[i], lats[i], **kw)
            for k in one:
                assert torch.equal(one[k], batch[i][k]) and torch.equal(again[i][k], batch[i][k]), (i, sizes[i], k)


def _noisy(theta, H, W, seed):
    rng = np.random.default_rng(seed)
    up, lat = model_fields(theta, H, W)
    ang = np.radians(rng.normal(0.0, 2.0, (H, W)))
    c, s = np.cos(ang), np.sin(ang)
    up = np.stack([c * up[0] - s * up[1], s * up[0] + c * up[1]])
    lat = lat + rng.normal(0.0, 2.0, (H, W))
    h, w = int(H * 0.45), int(W * 0.45)   # 20 % of the image: unrelated vectors and latitudes
    a = rng.uniform(-np.pi, np.pi, (h, w))
    up[0, -h:, :w], up[1, -h:, :w] = np.cos(a), np.sin(a)
    lat[-h:, :w] = rng.uniform(-90.0, 90.0, (h, w))
    return up, lat


def test_huber_is_robust_to_outliers():
    from perspectivefields_amd import fit_camera_params

    H, W = 480, 640
    truth = (12.0, -20.0, 70.0)
    up, lat = _noisy((np.radians(truth[0]), np.radians(truth[1]), focal_of_vfov(truth[2]), 0.0, 0.0), H, W, 3)
    u, l = torch.from_numpy(up).float().cuda(), torch.from_numpy(lat).float().cuda()
    err = {}
    for loss in ("huber", "l2"):
        d = fit_camera_params(u, l, loss=loss, huber_delta_deg=2.0)
        err[loss] = np.abs(np.array([float(d["pred_roll"]), float(d["pred_pitch"]), float(d["pred_vfov"])]) - np.array(truth))
    assert err["huber"][0] <= 0.3 and err["huber"][1] <= 0.3 and err["huber"][2] <= 0.5, err
    assert err["huber"].sum() < err["l2"].sum(), err


def _network_fields(version, sizes, seed):
    from perspectivefields_amd import PerspectiveFields
    from perspectivefields_amd.synth import synthetic_image

    model = PerspectiveFields(version, weights="synthetic:0").eval().to("cuda:0")
    return model, model.inference_batch([synthetic_image(h, w, seed=seed + k) for k, (h, w) in enumerate(sizes)])


def _theta(d):
    return (np.radians(float(d["pred_roll"])), np.radians(float(d["pred_pitch"])), float(d["pred_rel_focal"]), float(d["pred_rel_cx"]),
            float(d["pred_rel_cy"]))


@pytest.mark.parametrize("version", ["PersNet-360Cities", "Paramnet-360Cities-edina-centered"])
def test_fit_of_network_output_is_a_stationary_point_of_the_fp64_objective(version):
    from scipy.optimize import least_squares

    sizes = [(640, 640)] * 8 + [(97, 131), (301, 203)]
    model, preds = _network_fields(version, sizes, 11)
    fits = model.fit_camera(preds, max_iter=100)
    start = {"pred_roll": 5.0, "pred_pitch": -10.0, "pred_rel_focal": float(focal_of_vfov(60.0))}
    fits_from = model.fit_camera(preds, max_iter=100, init=[start] * len(preds))
    for p, d, d0 in zip(preds, fits, fits_from):
        up, lat = p["pred_gravity_original"].cpu().numpy(), p["pred_latitude_original"].cpu().numpy()
        th = _theta(d)
        fun = lambda t: l2_residual_vector((t[0], t[1], t[2], th[3], th[4]), up, lat)
        c_gpu = cost(th, up, lat)
        assert abs(float(d["fit_cost"]) - c_gpu) <= 1e-4 * c_gpu
        s = least_squares(fun, np.array(th[:3]), method="lm", x_scale=np.array([1.0, 1.0, max(th[2], 1e-3)]))
        assert c_gpu - s.cost < 1e-4 * c_gpu, (version, d, s.x, s.cost)
        assert np.degrees(np.abs(s.x[:2] - np.array(th[:2]))).max() < 0.01, (version, th, s.x)
        # from the same start, the GPU fit ends no higher than scipy's
        t0 = (np.radians(start["pred_roll"]), np.radians(start["pred_pitch"]), start["pred_rel_focal"])
        s0 = least_squares(fun, np.array(t0), method="lm", x_scale=np.array([1.0, 1.0, t0[2]]))
        assert cost(_theta(d0), up, lat) <= (1 + 1e-3) * s0.cost, (version, d0, s0.x, s0.cost)


@pytest.mark.parametrize("version,free_pp", [("Paramnet-360Cities-edina-centered", False), ("Paramnet-360Cities-edina-uncentered", True),
                                             ("Paramnet-360Cities-edina-uncentered", False)])
def test_paramnet_refinement(version, free_pp):
    from perspectivefields_amd import fields_from_params

    sizes = [(320, 320), (240, 427), (97, 131)]
    model, preds = _network_fields(version, sizes, 5)
    before = [dict(p) for p in preds]
    fits = model.fit_camera(preds, init="paramnet", free_principal_point=free_pp)
    for p, q in zip(preds, before):   # the inference results are left as they were
        assert p.keys() == q.keys() and all(p[k] is q[k] for k in p)
    for p, d, (H, W) in zip(preds, fits, sizes):
        up, lat = p["pred_gravity_original"].cpu().numpy(), p["pred_latitude_original"].cpu().numpy()
        c_param = cost(_theta(p), up, lat)
        c_fit = cost(_theta(d), up, lat)
        assert c_fit <= c_param * (1 + 1e-5), (version, c_fit, c_param)
        u2, l2 = fields_from_params(d["pred_roll"], d["pred_pitch"], d["pred_rel_focal"], d["pred_rel_cx"], d["pred_rel_cy"], H, W)
        ru = torch.sqrt(((u2 - p["pred_gravity_original"]) ** 2).sum(0).mean()).item() * 180 / np.pi
        rl = torch.sqrt(((l2 - p["pred_latitude_original"]) ** 2).mean()).item()
        assert abs(ru - float(d["fit_rms_up_deg"])) <= 1e-3 and abs(rl - float(d["fit_rms_lat_deg"])) <= 1e-3, (ru, rl, d)
        ref_up, ref_lat = rms(_theta(d), up, lat)
        assert abs(ref_up - float(d["fit_rms_up_deg"])) <= 1e-3 and abs(ref_lat - float(d["fit_rms_lat_deg"])) <= 1e-3


def test_persnet_has_no_paramnet_init():
    from perspectivefields_amd.engine import PfError

    model, preds = _network_fields("PersNet-360Cities", [(64, 96)], 2)
    with pytest.raises(PfError):
        model.fit_camera(preds[0], init="paramnet")
    with pytest.raises(PfError):
        model.fields_from_prediction(preds[0], 64, 96)
    d = model.fit_camera(preds[0])
    assert "pred_roll" in d and "pred_roll" not in preds[0]


def test_degenerate_input():
    from perspectivefields_amd import fit_camera_params
    from perspectivefields_amd.engine import PfError

    u, l = upload((0.2, -0.3, 0.8, 0.0, 0.0), 7, 64)
    with pytest.raises(PfError):
        fit_camera_params(u, l)
    H, W = 120, 160
    u, l = upload((np.radians(8.0), np.radians(15.0), 0.9, 0.0, 0.0), H, W)
    l[10:30, 100:140] = float("nan")
    u[1, 90:95, 5:9] = float("inf")
    d = fit_camera_params(u, l)
    assert int(d["fit_valid_pixels"]) == H * W - 20 * 40 - 5 * 4
    assert abs(float(d["pred_roll"]) - 8.0) <= 5e-3 and abs(float(d["pred_pitch"]) - 15.0) <= 5e-3
    assert np.isfinite(float(d["fit_cost"]))
