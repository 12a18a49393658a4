"""Error bounds shared by the kernel-level GPU tests (tests/test_gpu_head_tail.py, tests/test_gpu_conv_forms.py).  Every bound here is derived from the number formats
(u = 2^-24, the fp32 unit roundoff) or is an existing project tolerance named next to it; none comes from what a kernel returns."""
import numpy as np

U = 2.0 ** -24  # fp32 unit roundoff


def _ratio(err, bound):
    """worst err / bound; a zero bound asks for a zero error"""
    err, bound = np.asarray(err, dtype=np.float64), np.asarray(bound, dtype=np.float64)
    r = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err == 0, 0.0, np.inf))
    return float(r.max()) if r.size else 0.0


def _worse(worst, *ratios):
    """the largest of `worst` and the ratios, where a NaN -- an output element that is NaN, the poison of ops.checked_outputs() -- is worse than any number: max() would
    drop it, and `assert worst <= 1.0` then fails on it"""
    for r in ratios:
        if worst == worst and not r <= worst:  # a NaN, once taken, stays
            worst = r
    return worst


def _normalize_bounds(d, E, n):
    """F.normalize of the 2-vector d (fp64, (..., 2)) whose components carry absolute errors E: with g = d / n, d g_0 = g_1 (g_1 dd_0 - g_0 dd_1) / n, so
    |d g_i| <= |dd|_2 / n <= hypot(E_0, E_1) / n -- the dot products' error divided by the fp64 norm -- plus 4 u for the fp32 squares, sum, square root and division."""
    return np.hypot(E[..., 0], E[..., 1])[..., None] / n[..., None] + 4 * U


def _head_bounds(case, hw, hb):
    """fp64 head outputs on the fp64 map case["map"] (B, HW, 32), whose error is bounded by case["map_err"], and the bounds: the map's error through |w| (ReLU is
    1-Lipschitz) plus the head's own summation, then as for pred_regression"""
    hw, hb = np.asarray(hw, dtype=np.float64), np.asarray(hb, dtype=np.float64)
    raw = case["map"] @ hw.T + hb                                                   # (B, HW, nout)
    E = case["map_err"] @ np.abs(hw).T + 32 * U * (np.abs(case["map"]) @ np.abs(hw).T)
    return raw, E
