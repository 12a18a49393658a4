"""Field errors on the GPU (include/pf_hip.h pf_field_errors, perspectivefields_amd.field_errors / FieldErrorAccumulator) against the fp64
reference of tests/test_field_errors_ref.py: per-pixel maps, statistics, exactness of the selected median, masking, batch invariance, the
device-side accumulator and the crop -> inference -> comparison chain.

Bounds (derived, not fitted): e_lat is one fp32 subtraction of the inputs, at most half an ulp from the fp64 value.
For e_up, cross and dot of two fp32 vectors of length ~ 1 carry a few 2^-24 of absolute error (a few 1e-7 rad ~ 2e-5 deg) and atan2f with
the degree conversion a few ulp of a value <= 180 deg (one ulp: 1.5e-5 deg), so |d e_up| <= UP_TOL = 2e-4 deg everywhere.
Measured worst case on MI355X (test_maps_and_statistics_against_the_reference prints it): |d e_up| 2.85e-5 deg, e_lat 0.500 ulp."""
import numpy as np
import pytest
import torch

from tests.test_field_errors_ref import errors, stats
from tests.test_fit_camera_ref import model_fields
from tests.test_gpu_fit_camera import _noisy

pytestmark = pytest.mark.gpu

UP_TOL = 2e-4   # degrees, see the module docstring; measured worst case on MI355X 2.85e-5 (1024 x 1365, at e_up = 148.6 deg), e_lat 0.500 ulp
SIZES = ((640, 640), (384, 512), (1024, 1365), (37, 53), (1, 1))
STAT_KEYS = ("mean_deg", "median_deg", "rmse_deg", "max_deg")


def _pair(H, W, seed):
    """(up_pred, lat_pred, up_gt, lat_gt) fp32 numpy: exact fields of a camera as the label, the noisy fields of _noisy as the prediction
    (2 deg of noise and a patch of unrelated vectors: small and large angles)"""
    if H < 2 or W < 2:
        rng = np.random.default_rng(seed)
        a = rng.uniform(-np.pi, np.pi, (H, W))
        up_gt, lat_gt = np.stack([np.cos(a), np.sin(a)]), rng.uniform(-90, 90, (H, W))
        b = a + np.radians(rng.normal(0.0, 2.0, (H, W)))
        up, lat = np.stack([np.cos(b), np.sin(b)]), lat_gt + rng.normal(0.0, 2.0, (H, W))
    else:
        theta = (np.radians(-20.0 + 7 * (seed % 7)), np.radians(35.0 - 9 * (seed % 8)), 0.6 + 0.1 * (seed % 5), 0.0, 0.0)
        up_gt, lat_gt = model_fields(theta, H, W)
        up, lat = _noisy(theta, H, W, seed)
    return tuple(x.astype(np.float32) for x in (up, lat, up_gt, lat_gt))


def _cuda(arrs):
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrs]


def _run(sets, **kw):
    """sets: [(up_pred, lat_pred, up_gt, lat_gt) numpy] -> list of per-image dicts from one field_errors call"""
    from perspectivefields_amd import field_errors

    cols = [_cuda([s[k] for s in sets]) for k in range(4)]
    return field_errors(*cols, **kw)


def _host(d):
    return {k: (v.cpu().numpy() if v.dim() else (int(v) if k == "valid_pixels" else float(v))) for k, v in d.items()}


def _same(a, b):
    return a == b or (np.isnan(a) and np.isnan(b))


def _check_exact_selection(d):
    """the medians (and max, count) are exact functions of the returned fp32 maps"""
    for name in ("up", "lat"):
        m = d[f"{name}_error_deg"]
        v = m[np.isfinite(m)].astype(np.float64)
        assert d["valid_pixels"] == v.size
        if v.size == 0:
            assert all(np.isnan(d[f"{name}_{k}"]) for k in STAT_KEYS + ("frac_below",))
            continue
        assert d[f"{name}_median_deg"] == np.median(v), (name, d[f"{name}_median_deg"], np.median(v))
        assert d[f"{name}_max_deg"] == v.max()
        assert d[f"{name}_mean_deg"] == pytest.approx(v.mean(), rel=1e-12) and d[f"{name}_rmse_deg"] == pytest.approx(np.sqrt((v * v).mean()), rel=1e-12)
        assert d[f"{name}_frac_below"] == (m[np.isfinite(m)] < np.float32(5.0)).sum() / v.size


def test_maps_and_statistics_against_the_reference():
    sets = [_pair(H, W, 3 + k) for k, (H, W) in enumerate(SIZES)]
    res = [_host(d) for d in _run(sets, return_maps=True)]
    worst_up, worst_lat_ulp = 0.0, 0.0
    for (H, W), s, d in zip(SIZES, sets, res):
        e_up, e_lat = errors(*s)
        assert d["up_error_deg"].shape == (H, W) and d["up_error_deg"].dtype == np.float32
        assert not np.isnan(e_up).any() and np.isfinite(d["up_error_deg"]).all() and np.isfinite(d["lat_error_deg"]).all()
        d_up = np.abs(d["up_error_deg"].astype(np.float64) - e_up)
        d_lat = np.abs(d["lat_error_deg"].astype(np.float64) - e_lat)
        half_ulp = 0.5 * np.spacing(np.maximum(d["lat_error_deg"], np.float32(1.2e-38))).astype(np.float64)
        worst_up = max(worst_up, d_up.max())
        worst_lat_ulp = max(worst_lat_ulp, (d_lat / (2 * half_ulp)).max())
        print(f"{H} x {W}: max |d e_up| {d_up.max():.3e} deg (at e_up = {e_up.ravel()[d_up.argmax()]:.4f}), max |d e_lat| {d_lat.max():.3e} deg = {(d_lat / (2 * half_ulp)).max():.3f} ulp")
        assert d_up.max() <= UP_TOL, (H, W, d_up.max())
        assert (d_lat <= half_ulp).all(), (H, W, (d_lat / half_ulp).max())
        assert (e_up.min() < 0.01 and e_up.max() > 170.0) or H * W < 100000   # small and large angles are both present
        ref = stats(e_up, e_lat)
        assert d["valid_pixels"] == ref["valid_pixels"] == H * W
        for name, e in (("up", e_up), ("lat", e_lat)):
            for k in STAT_KEYS:   # order statistics move by no more than the largest per-element change: no pixel is left out
                assert abs(d[f"{name}_{k}"] - ref[f"{name}_{k}"]) <= UP_TOL, (H, W, name, k, d[f"{name}_{k}"], ref[f"{name}_{k}"])
            lo, hi = (e < 5.0 - UP_TOL).sum() / e.size, (e < 5.0 + UP_TOL).sum() / e.size
            assert lo <= d[f"{name}_frac_below"] <= hi, (H, W, name, lo, d[f"{name}_frac_below"], hi)
        _check_exact_selection(d)
    print(f"worst |d e_up| {worst_up:.3e} deg (bound {UP_TOL}), worst |d e_lat| {worst_lat_ulp:.3f} ulp (bound 0.5)")


def _adversarial():
    """name -> (up_pred, lat_pred, up_gt, lat_gt); latitude errors are exact by construction (label 0 or +-90), up errors are rotations"""
    rng = np.random.default_rng(5)
    cases = {}

    def fields(H, W, ang_deg, lat_err):
        a = rng.uniform(-np.pi, np.pi, (H, W))
        b = a + np.radians(np.broadcast_to(np.asarray(ang_deg, dtype=np.float64), (H, W)))
        return [np.stack([np.cos(b), np.sin(b)]).astype(np.float32), np.broadcast_to(np.asarray(lat_err, dtype=np.float32), (H, W)).copy(),
                np.stack([np.cos(a), np.sin(a)]).astype(np.float32), np.zeros((H, W), np.float32)]

    cases["all equal"] = fields(40, 52, 0.0, 3.25)
    cases["all equal"][0] = cases["all equal"][2] * np.float32(2.0)   # same direction, other length: e_up = 0 exactly
    half = (np.arange(48 * 50).reshape(48, 50) % 2).astype(np.float64)
    cases["two values split evenly"] = fields(48, 50, 10.0 + 20.0 * half, 1.0 + half)
    one = fields(33, 47, 12.0, 7.5)
    one[3][:] = np.nan
    one[3][17, 5] = 0.0
    cases["one valid pixel"] = one
    two = fields(33, 47, rng.uniform(0, 90, (33, 47)), rng.uniform(0, 9, (33, 47)))
    two[2][0][:] = np.nan
    two[2][0][4, 4] = 1.0; two[2][1][4, 4] = 0.0
    two[2][0][30, 46] = 0.0; two[2][1][30, 46] = -1.0
    cases["two valid pixels"] = two
    none = fields(16, 20, 1.0, 1.0)
    none[1][:] = np.inf
    cases["every pixel invalid"] = none
    ends = fields(32, 32, 0.0, 0.0)
    ends[0] = ends[2].copy()
    ends[0][:, 16:, :] *= -1.0                   # exactly opposite: e_up = 180
    ends[1][16:, :] = 90.0
    ends[3][16:, :] = -90.0                      # e_lat = 180
    ends[1][:3, :] = 1.0                         # an odd split so that the median is not the mean of 0 and 180
    cases["errors of 0 and of exactly 180"] = ends
    den = fields(24, 36, rng.uniform(0, 1e-5, (24, 36)), (rng.integers(1, 5000, (24, 36)) * 1e-42).astype(np.float32))
    cases["denormal-sized errors"] = den
    nanhalf = fields(64, 64, rng.normal(0, 3, (64, 64)), np.abs(rng.normal(0, 3, (64, 64))))
    nanhalf[3][rng.random((64, 64)) < 0.5] = np.nan
    cases["half of a plane NaN"] = nanhalf
    cases["H * W not a multiple of 4"] = fields(37, 53, rng.normal(0, 3, (37, 53)), np.abs(rng.normal(0, 30, (37, 53))))
    cases["5 x 7"] = fields(5, 7, rng.normal(0, 3, (5, 7)), np.abs(rng.normal(0, 30, (5, 7))))
    cases["wide spread"] = fields(128, 96, rng.uniform(0, 180, (128, 96)), 10.0 ** rng.uniform(-30, 2, (128, 96)))
    return cases


def test_selection_is_exact_on_adversarial_input():
    cases = _adversarial()
    res = [_host(d) for d in _run(list(cases.values()), return_maps=True)]
    for (name, s), d in zip(cases.items(), res):
        e_up, e_lat = errors(*s)
        assert (np.isnan(d["up_error_deg"]) == np.isnan(e_up)).all() and (np.isnan(d["lat_error_deg"]) == np.isnan(e_lat)).all(), name
        ok = ~np.isnan(e_lat)
        assert (d["lat_error_deg"][ok].astype(np.float64) == e_lat[ok]).all(), name    # exact by construction
        assert (np.abs(d["up_error_deg"][ok].astype(np.float64) - e_up[ok]) <= UP_TOL).all(), name
        _check_exact_selection(d)
        ref = stats(e_up, e_lat)
        for k in ("lat_median_deg", "lat_max_deg", "lat_frac_below", "valid_pixels"):
            assert _same(d[k], ref[k]), (name, k, d[k], ref[k])
    by = dict(zip(cases, res))
    assert by["two values split evenly"]["lat_median_deg"] == 1.5 and abs(by["two values split evenly"]["up_median_deg"] - 20.0) <= UP_TOL
    assert by["one valid pixel"]["valid_pixels"] == 1 and by["one valid pixel"]["lat_median_deg"] == 7.5
    assert by["two valid pixels"]["valid_pixels"] == 2
    assert by["every pixel invalid"]["valid_pixels"] == 0 and np.isnan(by["every pixel invalid"]["up_mean_deg"])
    assert by["errors of 0 and of exactly 180"]["up_max_deg"] == 180.0 and by["errors of 0 and of exactly 180"]["lat_max_deg"] == 180.0
    assert by["errors of 0 and of exactly 180"]["lat_median_deg"] in (1.0, 180.0, 90.5)
    assert 0.0 < by["denormal-sized errors"]["lat_median_deg"] < 1e-38


def test_non_contiguous_views_and_batched_tensors():
    from perspectivefields_amd import field_errors

    s = _cuda(_pair(96, 120, 9))
    want = field_errors(*s, return_maps=True)
    big_up = torch.full((2, 192, 240), 7.0, device="cuda")
    big_lat = torch.full((192, 240), 7.0, device="cuda")
    big_up[:, ::2, 1::2] = s[0]
    big_lat[1::2, ::2] = s[1]
    got = field_errors(big_up[:, ::2, 1::2], big_lat[1::2, ::2], s[2], s[3], return_maps=True)
    assert isinstance(got, dict) and got.keys() == want.keys()
    for k in want:
        assert torch.equal(got[k], want[k], ) or (torch.isnan(got[k]).all() and torch.isnan(want[k]).all()), k
    # contiguous but not 16-byte aligned (H * W is a multiple of 4): the element-wise path, same bits
    buf = torch.empty(1 + 96 * 120, device="cuda")
    buf[1:] = s[1].reshape(-1)
    off = field_errors(s[0], buf[1:].view(96, 120), s[2], s[3], return_maps=True)
    assert buf[1:].data_ptr() % 16 == 4 and all(torch.equal(off[k], want[k]) for k in want)
    # a batched (B, 2, H, W) / (B, H, W) tensor counts as a list of B
    sets = [_cuda(_pair(25, 31, 20 + k)) for k in range(3)]
    stacked = [torch.stack([x[k] for x in sets]) for k in range(4)]
    res = field_errors(*stacked)
    assert isinstance(res, list) and len(res) == 3
    for x, d in zip(sets, res):
        one = field_errors(*x)
        for k in one:
            assert torch.equal(one[k], d[k]), k


def test_latitudes_on_an_eighth_degree_grid_are_exact():
    rng = np.random.default_rng(21)
    sets = []
    for H, W in ((640, 640), (37, 53), (200, 301)):
        s = list(_pair(H, W, 4))
        s[1] = (rng.integers(-720, 721, (H, W)) / 8.0).astype(np.float32)
        s[3] = (rng.integers(-720, 721, (H, W)) / 8.0).astype(np.float32)
        s[3][rng.random((H, W)) < 0.05] = np.nan
        sets.append(s)
    for s, d in zip(sets, _run(sets, threshold_deg=22.5)):
        d = _host(d)
        ref = stats(*errors(*s), threshold=22.5)
        for k in ("lat_median_deg", "lat_max_deg", "lat_frac_below", "valid_pixels"):
            assert d[k] == ref[k], (k, d[k], ref[k])
        for k in ("lat_mean_deg", "lat_rmse_deg"):
            assert d[k] == pytest.approx(ref[k], rel=1e-13), (k, d[k], ref[k])


def test_crop_panorama_masks_go_straight_in():
    from perspectivefields_amd import crop_panorama, field_errors

    rng = np.random.default_rng(2)
    pano = torch.from_numpy(rng.integers(0, 256, (256, 512, 3), dtype=np.uint8)).cuda()
    H, W = 150, 200
    _, up, lat = crop_panorama(pano, [5.0, -10.0], [20.0, -15.0], [0.35, 0.3], xi=1.2, height=H, width=W)
    finite = torch.isfinite(up).all(1) & torch.isfinite(lat)
    assert 0 < int(finite[0].sum()) < H * W   # NaN outside the image circle
    noise = torch.from_numpy(rng.normal(0.0, 1.0, (2, H, W)).astype(np.float32)).cuda()
    pred_up = torch.nan_to_num(up, nan=0.3) + 0.01 * noise[:, None]
    pred_lat = torch.nan_to_num(lat, nan=1.0) + noise
    res = field_errors(pred_up, pred_lat, up, lat, return_maps=True)
    for i, d in enumerate(res):
        assert int(d["valid_pixels"]) == int(finite[i].sum())
        assert torch.equal(torch.isnan(d["up_error_deg"]), ~finite[i]) and torch.equal(torch.isnan(d["lat_error_deg"]), ~finite[i])
        _check_exact_selection(_host(d))


def test_rows_do_not_depend_on_the_batch_and_repeat():
    from perspectivefields_amd import FieldErrorAccumulator, field_errors

    sizes = [SIZES[k % 4] if k % 11 == 0 else (20 + 3 * k, 31 + 5 * k) for k in range(33)]   # 33 images: two launch groups
    sets = [_cuda(_pair(H, W, k)) for k, (H, W) in enumerate(sizes)]
    cols = [[s[k] for s in sets] for k in range(4)]
    batch = field_errors(*cols)
    again = field_errors(*cols)
    rev = field_errors(*[c[::-1] for c in cols])[::-1]
    for i in range(len(sizes)):
        one = field_errors(*sets[i])
        for k in one:
            assert torch.equal(one[k], batch[i][k]) and torch.equal(again[i][k], batch[i][k]) and torch.equal(rev[i][k], batch[i][k]), (i, sizes[i], k)
    # the accumulator's kernel path: the rows are those of field_errors; two updates of one accumulator = two accumulators merged
    a, b, c = (FieldErrorAccumulator("cuda") for _ in range(3))
    first, second = [c_[:20] for c_ in cols], [c_[20:] for c_ in cols]
    rows = a.update(*first) + a.update(*second)
    for i in range(len(sizes)):
        for k in rows[i]:
            assert torch.equal(rows[i][k], batch[i][k]), (i, k)
    b.update(*first)
    c.update(*second)
    b.merge(c)
    assert torch.equal(a.hist, b.hist) and int(a.hist[0].sum()) == sum(H * W for H, W in sizes)
    assert torch.equal(a.sums[:, [0, 3, 4]], b.sums[:, [0, 3, 4]])
    assert torch.allclose(a.sums, b.sums, rtol=1e-13, atol=0.0)


def test_accumulator_update_equals_add_errors_of_the_maps():
    from perspectivefields_amd import FieldErrorAccumulator

    from tests.test_field_errors_ref import BIN

    acc, ref, cpu = FieldErrorAccumulator("cuda", threshold_deg=3.0), FieldErrorAccumulator("cuda", threshold_deg=3.0), FieldErrorAccumulator("cpu", threshold_deg=3.0)
    all_up, all_lat = [], []
    for b, sizes in enumerate((((640, 640), (37, 53)), ((384, 512), (1, 1), (97, 131)), ((200, 301),))):
        sets = [_pair(H, W, 40 + 10 * b + k) for k, (H, W) in enumerate(sizes)]
        sets[0][3][:5, :] = np.nan   # some masked rows
        cols = [_cuda([s[k] for s in sets]) for k in range(4)]
        rows = acc.update(*cols, return_maps=True)
        ref.add_errors([d["up_error_deg"] for d in rows], [d["lat_error_deg"] for d in rows])
        cpu.add_errors([d["up_error_deg"].cpu() for d in rows], [d["lat_error_deg"].cpu() for d in rows])
        all_up += [d["up_error_deg"].cpu().numpy().ravel() for d in rows]
        all_lat += [d["lat_error_deg"].cpu().numpy().ravel() for d in rows]
    for other in (ref, cpu):
        assert torch.equal(acc.hist.cpu(), other.hist.cpu())
        assert torch.equal(acc.sums[:, [0, 3, 4]].cpu(), other.sums[:, [0, 3, 4]].cpu())
        assert torch.allclose(acc.sums.cpu(), other.sums.cpu(), rtol=1e-13, atol=0.0)
    s = acc.summary()
    want = stats(np.concatenate(all_up), np.concatenate(all_lat), threshold=3.0)
    assert s["valid_pixels"] == want["valid_pixels"]
    for k, v in want.items():
        if k.endswith("median_deg"):
            assert abs(s[k] - v) <= BIN, (k, s[k], v)
        elif k != "valid_pixels":
            assert s[k] == pytest.approx(v, rel=1e-12), (k, s[k], v)


@pytest.mark.parametrize("version", ["PersNet-360Cities", "Paramnet-360Cities-edina-centered"])
def test_crop_infer_compare_chain(version):
    from perspectivefields_amd import PerspectiveFields, crop_panorama, field_errors

    rng = np.random.default_rng(12)
    pano = torch.from_numpy(rng.integers(0, 256, (512, 1024, 3), dtype=np.uint8)).cuda()
    m = PerspectiveFields(version, weights="synthetic:0").eval().cuda()
    B, H, W = 3, 120, 160
    img, up, lat = crop_panorama(pano, [0.0, 10.0, -20.0], [5.0, -30.0, 40.0], [0.8, 1.1, 0.6], yaw=[0.0, 120.0, -170.0], height=H, width=W)
    preds = m.inference_batch(list(img))
    res = m.field_errors(preds, up, lat)
    assert isinstance(res, list) and len(res) == B
    # the regression heads predict unit vectors: every pixel counts.  PersNet's classification head has a "no up vector" class that
    # decodes to (0, 0) (decode_bin, utils/utils.py:114-130): those pixels have no direction to score and are invalid by definition
    has_up = [int(((p["pred_gravity_original"] ** 2).sum(0) >= 1e-12).sum()) for p in preds]
    assert has_up == [H * W] * B or version.startswith("PersNet")
    for d, n_up in zip(res, has_up):
        assert int(d["valid_pixels"]) == n_up > 0 and d["up_mean_deg"].dtype == torch.float64 and d["up_mean_deg"].shape == ()
        assert all(np.isfinite(float(v)) for v in d.values())
        assert 0.0 <= float(d["up_median_deg"]) <= float(d["up_max_deg"]) <= 180.0 and 0.0 <= float(d["up_frac_below"]) <= 1.0
    one = m.field_errors(preds[1], up[1], lat[1])
    assert isinstance(one, dict) and all(torch.equal(one[k], res[1][k]) for k in one)
    own = field_errors([p["pred_gravity_original"] for p in preds], [p["pred_latitude_original"] for p in preds],
                       [p["pred_gravity_original"] for p in preds], [p["pred_latitude_original"] for p in preds], return_maps=True)
    for d, n_up in zip(own, has_up):   # a prediction scored against itself
        assert int(d["valid_pixels"]) == n_up
        assert all(float(d[f"{n}_{k}"]) == 0.0 for n in ("up", "lat") for k in STAT_KEYS) and float(d["up_frac_below"]) == 1.0
        assert not torch.nan_to_num(d["up_error_deg"], nan=0.0).any() and not torch.nan_to_num(d["lat_error_deg"], nan=0.0).any()
        assert int(torch.isnan(d["up_error_deg"]).sum()) == H * W - n_up


def test_argument_errors():
    from perspectivefields_amd import field_errors
    from perspectivefields_amd.engine import PfError

    up, lat, up_gt, lat_gt = _cuda(_pair(16, 24, 1))
    with pytest.raises(PfError):
        field_errors(up.cpu(), lat.cpu(), up_gt.cpu(), lat_gt.cpu())
    with pytest.raises(PfError):
        field_errors(up, lat, up_gt.cpu(), lat_gt)
    with pytest.raises(ValueError):
        field_errors(up, lat, up_gt[:, :8], lat_gt[:8])
    with pytest.raises(ValueError):
        field_errors(up, lat[:8], up_gt, lat_gt)
    with pytest.raises(ValueError):
        field_errors([up, up], [lat, lat], [up_gt], [lat_gt])
    with pytest.raises(ValueError):
        field_errors([], [], [], [])
    for bad in (0.0, -5.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            field_errors(up, lat, up_gt, lat_gt, threshold_deg=bad)
    with pytest.raises(TypeError):
        field_errors(up.cpu().numpy(), lat, up_gt, lat_gt)
    d = field_errors(up, lat, up_gt, lat_gt, threshold_deg=1.0)
    assert int(d["valid_pixels"]) == 16 * 24 and "up_error_deg" not in d
