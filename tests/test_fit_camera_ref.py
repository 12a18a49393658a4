"""fp64 numpy reference of the camera fit's objective (include/pf_hip.h pf_fit_camera), checked against
the oracle's camera-parameters -> fields model, which tests/golden/fields_from_params.npz pins to the reference; plus the
host-side contract of the fit (no GPU needed).  tests/test_gpu_fit_camera.py uses the same reference on the GPU results."""
import os
import re

import numpy as np
import pytest
import torch

from oracle import pf_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R2D = 180.0 / np.pi


def model_fields(theta, H, W):
    """theta = (roll, pitch [rad], rel_focal, rel_cx, rel_cy) -> up (2, H, W), latitude (H, W) degrees, in fp64.  The up field is the
    reference's (vvp - xy) sign(p) times |sin p| (no 1/sin p); the latitude is the reference's, on its linspace grid."""
    r, p, f, cx, cy = (float(v) for v in theta)
    F, Cx, Cy = f * H, (cx + 0.5) * W, (cy + 0.5) * H
    sr, cr, sp, cp = np.sin(r), np.cos(r), np.sin(p), np.cos(p)
    px = np.arange(W, dtype=np.float64)[None, :] + 0.5
    py = np.arange(H, dtype=np.float64)[:, None] + 0.5
    a = sr * cp * F + sp * (px - Cx) + 0.0 * py
    b = cr * cp * F + sp * (py - Cy) + 0.0 * px
    n = np.sqrt(a * a + b * b)
    up = np.stack([-a / n, -b / n])
    x = ((np.arange(W, dtype=np.float64) * (W / (W - 1)))[None, :] - Cx) / F
    y = ((np.arange(H, dtype=np.float64) * (H / (H - 1)))[:, None] - Cy) / F
    xw = x * cr - y * sr
    yw = x * cp * sr + y * cp * cr - sp
    zw = x * sp * sr + y * sp * cr + cp
    lat = -np.arctan2(yw, np.sqrt(xw * xw + zw * zw)) * R2D
    return up, lat


def residuals(theta, up_pred, lat_pred):
    """per-pixel residuals over the pixels with finite input: r_up (2, N) chordal in degree scale, r_lat (N,) degrees"""
    H, W = lat_pred.shape
    up, lat = model_fields(theta, H, W)
    ok = np.isfinite(up_pred).all(0) & np.isfinite(lat_pred)
    return (up[:, ok] - up_pred[:, ok].astype(np.float64)) * R2D, lat[ok] - lat_pred[ok].astype(np.float64)


def rho(r, loss="l2", delta=2.0):
    r = np.abs(r)
    if loss == "l2":
        return 0.5 * r * r
    return np.where(r <= delta, 0.5 * r * r, delta * (r - 0.5 * delta))


def cost(theta, up_pred, lat_pred, loss="l2", delta=2.0, weights=(1.0, 1.0)):
    ru, rl = residuals(theta, up_pred, lat_pred)
    return float(weights[0] * rho(np.sqrt((ru * ru).sum(0)), loss, delta).sum() + weights[1] * rho(rl, loss, delta).sum())


def rms(theta, up_pred, lat_pred):
    ru, rl = residuals(theta, up_pred, lat_pred)
    return float(np.sqrt((ru * ru).sum(0).mean())), float(np.sqrt((rl * rl).mean()))


def l2_residual_vector(theta, up_pred, lat_pred, weights=(1.0, 1.0)):
    """the L2 objective as scipy.optimize.least_squares sees it: cost = 0.5 * |this|^2"""
    ru, rl = residuals(theta, up_pred, lat_pred)
    return np.concatenate([np.sqrt(weights[0]) * ru.ravel(), np.sqrt(weights[1]) * rl])


def general_vfov_deg(f, cx, cy):
    P = f * f + cx * cx + (cy + 0.5) ** 2
    Q = f * f + cx * cx + (cy - 0.5) ** 2
    return np.degrees(np.arccos((P + Q - 1.0) / (2.0 * np.sqrt(P * Q))))


CASES = [  # roll, pitch (deg), rel_focal, rel_cx, rel_cy, H, W
    (12.0, 35.0, 0.8, 0.0, 0.0, 48, 64),
    (-30.0, -20.0, 1.3, 0.0, 0.0, 37, 53),
    (5.0, 0.0, 0.6, 0.0, 0.0, 40, 40),      # p = 0: the reference's constant up field
    (-5.0, 0.0, 1.1, 0.08, -0.1, 31, 45),
    (40.0, 70.0, 2.0, -0.1, 0.08, 50, 33),
    (0.0, -70.0, 0.35, 0.05, 0.02, 29, 61),
]


@pytest.mark.parametrize("case", CASES)
def test_reference_model_matches_the_oracle(case):
    """the fit's model equals the oracle's fields_from_params (pinned to the reference's goldens) to 1e-9, p = 0 and the
    latitude grid's linspace spacing W / (W - 1) included"""
    roll, pitch, f, cx, cy, H, W = case
    gv = general_vfov_deg(f, cx, cy)
    up_o, lat_o, f_o = pf_oracle.fields_from_params(roll, pitch, gv, cx, cy, H, W, mode="deg")
    assert abs(f_o - f) <= 1e-12 * f
    up, lat = model_fields((np.radians(roll), np.radians(pitch), f, cx, cy), H, W)
    assert np.abs(up - np.moveaxis(up_o, 2, 0)).max() <= 1e-9
    assert np.abs(lat - lat_o).max() <= 1e-9


def test_reference_objective_is_zero_at_the_truth_and_skips_non_finite():
    theta = (np.radians(12.0), np.radians(-20.0), 0.9, 0.0, 0.0)
    up, lat = model_fields(theta, 24, 32)
    lat = lat.copy()
    lat[3, 4] = np.nan
    up = up.copy()
    up[1, 5, 6] = np.inf
    assert cost(theta, up, lat) == 0.0
    ru, rl = residuals(theta, up, lat)
    assert rl.shape == (24 * 32 - 2,) and ru.shape == (2, 24 * 32 - 2)
    moved = (theta[0] + 0.01,) + theta[1:]
    assert cost(moved, up, lat) > 0.0 and cost(moved, up, lat, "huber", 0.1) < cost(moved, up, lat)


def test_general_vfov_formula_inverts_general_vfov_to_focal():
    from perspectivefields_amd.perspectivefields import general_vfov_to_focal

    for f, cx, cy in ((0.8, 0.0, 0.0), (1.3, 0.08, -0.1), (0.4, -0.1, 0.08), (2.5, 0.05, 0.1)):
        gv = general_vfov_deg(f, cx, cy)
        assert abs(float(general_vfov_to_focal(cx, cy, gv)) - f) <= 1e-9 * f
    assert abs(general_vfov_deg(0.8, 0.0, 0.0) - np.degrees(2 * np.arctan(1 / 1.6))) <= 1e-12


def test_fit_camera_params_on_cpu_tensors_raises():
    from perspectivefields_amd import fit_camera_params
    from perspectivefields_amd.engine import PfError

    up, lat = model_fields((0.1, 0.2, 0.9, 0.0, 0.0), 16, 16)
    with pytest.raises(PfError):
        fit_camera_params(torch.from_numpy(up).float(), torch.from_numpy(lat).float())
    with pytest.raises(PfError):
        fit_camera_params([torch.from_numpy(up).float()], [torch.from_numpy(lat).float()], free_principal_point=True)


def test_output_columns_match_the_header():
    """the Python dict keys follow the PF_FIT_COL_* order of include/pf_hip.h"""
    from perspectivefields_amd.perspectivefields import _FIT_COLS

    hdr = open(os.path.join(ROOT, "include", "pf_hip.h")).read()
    cols = {m[0]: int(m[1]) for m in re.findall(r"#define PF_FIT_COL_([A-Z_]+) (\d+)", hdr)}
    assert int(re.search(r"#define PF_FIT_COLS (\d+)", hdr)[1]) == len(_FIT_COLS) == len(cols)
    names = {"ROLL": "pred_roll", "PITCH": "pred_pitch", "VFOV": "pred_vfov", "REL_FOCAL": "pred_rel_focal", "GENERAL_VFOV": "pred_general_vfov",
             "REL_CX": "pred_rel_cx", "REL_CY": "pred_rel_cy", "RMS_UP": "fit_rms_up_deg", "RMS_LAT": "fit_rms_lat_deg", "COST": "fit_cost",
             "ITERATIONS": "fit_iterations", "CONVERGED": "fit_converged", "VALID_PIXELS": "fit_valid_pixels"}
    assert {names[k]: v for k, v in cols.items()} == {k: i for i, k in enumerate(_FIT_COLS)}


def test_fit_workspace_size_and_small_images():
    """pf_fit_camera_workspace_bytes is host arithmetic: > 0 for valid sizes, growing with the images, 0 below 8 x 8"""
    import ctypes

    from perspectivefields_amd.engine import load_library

    lib = load_library()
    hw = lambda *s: (ctypes.c_int32 * len(s))(*s)
    one = lib.pf_fit_camera_workspace_bytes(1, hw(640, 640))
    two = lib.pf_fit_camera_workspace_bytes(2, hw(640, 640, 97, 131))
    assert 0 < one < two
    assert lib.pf_fit_camera_workspace_bytes(1, hw(7, 640)) == 0
    assert lib.pf_fit_camera_workspace_bytes(2, hw(640, 640, 8, 7)) == 0
    assert lib.pf_fit_camera_workspace_bytes(0, hw(640, 640)) == 0
