"""Placement scores on the GPU (include/pf_hip.h pf_place_scores, perspectivefields_amd.placement_scores, PerspectiveFields.placement_scores)
against the fp64 reference of tests/test_placement_ref.py on its fixed sets A - F, against field_errors on slices, the planted object, determinism,
the mask and the model method.

Tolerances: derived, not fitted.  Per pixel pair e_up is held to UP_TOL = 2e-4 deg, section 13's bound, which the
angle-difference form meets: two atan2f results of a few ulp of 180 deg each (one ulp: 1.5e-5 deg) and one subtraction; e_lat to LAT_TOL = 1.1e-5 deg,
one rounding of a difference of at most 180 deg.  A mean is held to its per-pair bound plus (T + 8) x 2^-24 x the reference mean, the bound of
recursive summation, T = min(1024, h w) being the terms one thread adds in fp32 before the fp64 pass (PlaceBatch::CHUNK).  n is exact: the sets have
no borderline length (asserted in the reference file).
The stride is one per call, so the call that holds all six sets runs at stride 1 and set B's stride-3 placements are every third of its rows and
columns: the same pixel pairs in the same order, so the same bits as B alone at stride 3 (asserted)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests.test_placement_ref import CHUNK, PLANT, ellipse, field_set, planted, reference, set_reference

pytestmark = pytest.mark.gpu
UP_TOL, LAT_TOL, U = 2e-4, 1.1e-5, 2.0 ** -24
NAMES = "ABCDEF"


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()   # a copy: the cached inputs are read-only


def fields(name):
    up_bg, lat_bg, up_obj, lat_obj, s = field_set(name)
    return dev(up_bg), dev(lat_bg), dev(up_obj), dev(lat_obj), s


def mean_bounds(ref, obj_px):
    """the allowed distance of up_mean_deg and lat_mean_deg to the reference's, (P, Q) each"""
    T = min(CHUNK, obj_px)
    return UP_TOL + (T + 8) * U * ref["up_mean_deg"], LAT_TOL + (T + 8) * U * ref["lat_mean_deg"]


def raw_scores(bgs, objs, pairs, stride):
    """pf_place_scores itself: d_out of every pair as a (P, Q, 3) float64 device tensor"""
    from perspectivefields_amd.engine import _check, _stream_ptr, load_library

    lib = load_library()
    ptrs = lambda ts: (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])
    hw = lambda fs: (ctypes.c_int32 * (2 * len(fs)))(*[s for u, _ in fs for s in u.shape[1:]])
    c_pairs = (ctypes.c_int32 * (2 * len(pairs)))(*[i for p in pairs for i in p])
    dims = [((bgs[b][1].shape[0] - objs[o][1].shape[0]) // stride + 1, (bgs[b][1].shape[1] - objs[o][1].shape[1]) // stride + 1) for b, o in pairs]
    need = lib.pf_place_scores_workspace_bytes(len(bgs), hw(bgs), len(objs), hw(objs), len(pairs), c_pairs, stride)
    assert need > 0
    out = torch.full((3 * sum(P * Q for P, Q in dims),), float("nan"), dtype=torch.float64, device="cuda")
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    _check(lib.pf_place_scores(0, len(bgs), ptrs([u for u, _ in bgs]), ptrs([l for _, l in bgs]), hw(bgs), len(objs), ptrs([u for u, _ in objs]),
                               ptrs([l for _, l in objs]), hw(objs), len(pairs), c_pairs, stride, out.data_ptr(), ws.data_ptr(), need, _stream_ptr()),
           None, "pf_place_scores")
    torch.cuda.synchronize()
    res, first = [], 0
    for P, Q in dims:
        res.append(out[first:first + 3 * P * Q].view(P, Q, 3))
        first += 3 * P * Q
    return res


@functools.lru_cache(None)
def joint_call():
    """all six sets in one placement_scores call at stride 1, pairs (k, k); the result dicts as numpy, read only"""
    from perspectivefields_amd import placement_scores

    f = [fields(n) for n in NAMES]
    res = placement_scores([x[0] for x in f], [x[1] for x in f], [x[2] for x in f], [x[3] for x in f], pairs=[(k, k) for k in range(6)])
    assert isinstance(res, list) and len(res) == 6
    for d in res:
        assert all(d[k].dtype == torch.float64 and d[k].is_cuda for k in ("pfd_deg", "up_mean_deg", "lat_mean_deg", "best_pfd_deg"))
        assert d["valid_pixels"].dtype == torch.int64 and d["best_offset"].dtype == torch.int64 and d["best_offset"].shape == (2,) and d["stride"] == 1
    return {n: {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in d.items()} for n, d in zip(NAMES, res)}


@functools.lru_cache(None)
def alone(name):
    from perspectivefields_amd import placement_scores

    up_bg, lat_bg, up_obj, lat_obj, s = fields(name)
    d = placement_scores(up_bg, lat_bg, up_obj, lat_obj, stride=s)
    assert isinstance(d, dict) and d["stride"] == s
    return {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in d.items()}


def check_against_reference(d, ref, obj_px, what):
    """the maps of one pair against the reference; returns the largest error / allowed of the two means"""
    assert d["pfd_deg"].shape == ref["pfd_deg"].shape, what
    assert (d["valid_pixels"] == ref["valid_pixels"]).all(), what
    inf = np.isinf(ref["pfd_deg"])
    assert (np.isinf(d["pfd_deg"]) == inf).all() and (d["pfd_deg"][inf] > 0).all(), what
    b_up, b_lat = mean_bounds(ref, obj_px)
    has = ref["valid_pixels"] > 0
    assert (np.isnan(d["up_mean_deg"]) == ~has).all() and (np.isnan(d["lat_mean_deg"]) == ~has).all(), what
    e_up, e_lat = np.abs(d["up_mean_deg"] - ref["up_mean_deg"])[has], np.abs(d["lat_mean_deg"] - ref["lat_mean_deg"])[has]
    e_pfd = np.abs(np.where(inf, 0.0, d["pfd_deg"]) - np.where(inf, 0.0, ref["pfd_deg"]))[~inf]
    worst = (float(e_up.max()), float((e_up / b_up[has]).max()), float(e_lat.max()), float((e_lat / b_lat[has]).max())) if has.any() else (0.0,) * 4
    print(f"{what}: up_mean error {worst[0]:.3e} deg = {worst[1]:.3f} of the allowed, lat_mean error {worst[2]:.3e} deg = {worst[3]:.3f} of the allowed")
    assert (e_up <= b_up[has]).all() and (e_lat <= b_lat[has]).all(), what
    assert (e_pfd <= (b_up + b_lat)[~inf]).all(), what
    return max(worst[1], worst[3])


def check_best_offset(d, ref, obj_px, must_be_clear, what):
    """best_offset equals the reference's wherever the reference's two best PFDs differ by more than twice the PFD bound"""
    b_up, b_lat = mean_bounds(ref, obj_px)
    finite = np.sort(ref["pfd_deg"][np.isfinite(ref["pfd_deg"])])
    clear = finite.size == 1 or (finite.size > 1 and finite[1] - finite[0] > 2.0 * float((b_up + b_lat)[np.isfinite(ref["pfd_deg"])].max()))
    if must_be_clear:
        assert clear, (what, finite[:2])
    if clear:
        assert tuple(d["best_offset"]) == ref["best_offset"], (what, d["best_offset"], ref["best_offset"])
        assert abs(d["best_pfd_deg"] - ref["best_pfd_deg"]) <= float((b_up + b_lat).max())
    if finite.size == 0:
        assert tuple(d["best_offset"]) == (-1, -1) and np.isinf(d["best_pfd_deg"])


@pytest.mark.parametrize("name", list(NAMES))
def test_sets_match_the_fp64_reference_in_one_call_and_alone(name):
    up_bg, lat_bg, up_obj, lat_obj, s = field_set(name)
    ref, obj_px = set_reference(name), lat_obj.size
    one = alone(name)
    check_against_reference(one, ref, obj_px, f"set {name} alone")
    check_best_offset(one, ref, obj_px, name in "ABC", f"set {name} alone")
    joint = joint_call()[name]
    for k in ("pfd_deg", "up_mean_deg", "lat_mean_deg", "valid_pixels"):   # stride 1 in the joint call: B's placements are every third
        assert np.array_equal(joint[k][::s, ::s], one[k], equal_nan=True), (name, k)
    if s == 1:
        assert tuple(joint["best_offset"]) == tuple(one["best_offset"]) and joint["best_pfd_deg"] == one["best_pfd_deg"]
    else:
        ref1 = reference(up_bg, lat_bg, up_obj, lat_obj, 1)
        check_against_reference(joint, ref1, obj_px, f"set {name} at stride 1 in the joint call")
        check_best_offset(joint, ref1, obj_px, False, f"set {name} at stride 1")


def test_set_shapes_cover_partial_tiles_chunks_and_masks():
    shapes = {n: set_reference(n)["pfd_deg"].shape for n in NAMES}
    assert shapes == dict(A=(32, 50), B=(6, 7), C=(8, 8), D=(1, 1), E=(40, 56), F=(32, 50))
    assert 32 * 50 > 6 * 256 and 32 * 50 % 256 != 0 and 33 * 35 > CHUNK   # several placement tiles with a partial one; two object chunks
    f = set_reference("F")
    assert np.isinf(f["pfd_deg"]).any() and np.isfinite(f["pfd_deg"]).any() and 0 < f["valid_pixels"].min() < f["valid_pixels"].max() == 63
    assert set_reference("C")["valid_pixels"].max() == ellipse(33, 35).sum() < 33 * 35


def test_five_placements_of_set_a_against_field_errors():
    from perspectivefields_amd import field_errors

    up_bg, lat_bg, up_obj, lat_obj, s = fields("A")
    d, ref = alone("A"), set_reference("A")
    b_up, b_lat = mean_bounds(ref, 63)
    for j, i in ((0, 0), (13, 22), (31, 49), (7, 40), (25, 3)):
        fe = field_errors(up_bg[:, j:j + 9, i:i + 7], lat_bg[j:j + 9, i:i + 7], up_obj, lat_obj)
        assert int(fe["valid_pixels"]) == d["valid_pixels"][j, i] == 63
        assert abs(float(fe["up_mean_deg"]) - d["up_mean_deg"][j, i]) <= UP_TOL + b_up[j, i]
        assert abs(float(fe["lat_mean_deg"]) - d["lat_mean_deg"][j, i]) <= LAT_TOL + b_lat[j, i]


def test_planted_object_scores_exactly_zero():
    from perspectivefields_amd import placement_scores

    up_bg, lat_bg, up_obj, lat_obj, s = planted()
    d = placement_scores(dev(up_bg), dev(lat_bg), dev(up_obj), dev(lat_obj))
    r, c = PLANT[:2]
    assert float(d["pfd_deg"][r, c]) == 0.0 and float(d["up_mean_deg"][r, c]) == 0.0 and float(d["lat_mean_deg"][r, c]) == 0.0
    assert d["best_offset"].tolist() == [r, c] and float(d["best_pfd_deg"]) == 0.0
    assert int((d["pfd_deg"] == 0).sum()) == 1
    ref = reference(up_bg, lat_bg, up_obj, lat_obj, s)
    check_against_reference({k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in d.items()}, ref, 63, "planted object")


def test_wrap_around_on_the_device():
    from perspectivefields_amd import placement_scores

    up = lambda x, y: torch.tensor([x, y], dtype=torch.float32, device="cuda").reshape(2, 1, 1)
    lat = torch.zeros((1, 1), device="cuda")
    d = placement_scores(up(-1.0, 1e-3), lat, up(-1.0, -1e-3), lat)
    assert abs(float(d["up_mean_deg"]) - 0.11459) <= UP_TOL and float(d["lat_mean_deg"]) == 0.0


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int64), b.contiguous().view(torch.int64))


def test_d_out_bits_do_not_depend_on_the_run_the_batch_or_the_order():
    f = {n: fields(n) for n in "ACDF"}
    bgs, objs = [f[n][:2] for n in "ACDF"], [f[n][2:4] for n in "ACDF"]
    pairs = [(0, 0), (1, 1), (2, 2), (3, 3), (0, 3), (3, 0), (2, 0), (2, 1)]
    first, again = raw_scores(bgs, objs, pairs, 1), raw_scores(bgs, objs, pairs, 1)
    assert all(not torch.isnan(a).any() for a in first)   # every record written
    assert all(same_bits(a, b) for a, b in zip(first, again))
    for k, (b, o) in enumerate(pairs):   # a pair alone
        assert same_bits(raw_scores([bgs[b]], [objs[o]], [(0, 0)], 1)[0], first[k]), (b, o)
    perm = [5, 2, 7, 0, 3, 6, 1, 4]
    shuffled = raw_scores(bgs, objs, [pairs[k] for k in perm], 1)
    assert all(same_bits(shuffled[at], first[k]) for at, k in enumerate(perm))
    # one background with three objects against three calls
    three = raw_scores([bgs[2]], [objs[0], objs[1], objs[3]], [(0, 0), (0, 1), (0, 2)], 1)
    for k, o in enumerate((0, 1, 3)):
        assert same_bits(three[k], raw_scores([bgs[2]], [objs[o]], [(0, 0)], 1)[0])
    # more pairs than one launch holds (32): the 33rd is the first again
    many = raw_scores(bgs, objs, [pairs[k % 8] for k in range(33)], 1)
    assert all(same_bits(many[k], first[k % 8]) for k in range(33))


def test_raw_sums_match_the_reference():
    up_bg, lat_bg, up_obj, lat_obj, s = fields("C")
    rec = raw_scores([(up_bg, lat_bg)], [(up_obj, lat_obj)], [(0, 0)], s)[0].cpu().numpy()
    ref = set_reference("C")
    b_up, b_lat = mean_bounds(ref, 33 * 35)
    assert (rec[..., 2] == ref["n"]).all()
    assert (np.abs(rec[..., 0] - ref["S_up"]) <= b_up * ref["n"]).all() and (np.abs(rec[..., 1] - ref["S_lat"]) <= b_lat * ref["n"]).all()


def test_mask_is_nan_written_by_hand():
    from perspectivefields_amd import placement_scores

    up_bg, lat_bg, up_obj, lat_obj, s = field_set("C")
    full = np.array(set_full_object())
    m = ellipse(33, 35)
    a = placement_scores(dev(up_bg), dev(lat_bg), dev(up_obj), dev(full), mask=dev(m))
    b = placement_scores(dev(up_bg), dev(lat_bg), dev(up_obj), dev(lat_obj))
    assert torch.isnan(dev(lat_obj)).sum() == (~m).sum()
    for k in ("pfd_deg", "up_mean_deg", "lat_mean_deg", "valid_pixels", "best_offset", "best_pfd_deg"):
        assert torch.equal(a[k], b[k]), k
    both = placement_scores(dev(up_bg), dev(lat_bg), [dev(up_obj), dev(up_obj)], [dev(full), dev(lat_obj)], mask=[dev(m), None])
    assert all(torch.equal(both[i]["pfd_deg"], b["pfd_deg"]) for i in range(2))


def set_full_object():
    """set C's object latitude before the ellipse was cut out"""
    from tests.test_placement_ref import BG_CAM, camera_fields, crop

    return crop(*camera_fields(*BG_CAM, 40, 42, seed=6), 4, 3, 33, 35)[1]


def test_threshold_weights_and_an_empty_object_on_the_device():
    from perspectivefields_amd import placement_scores

    up_bg, lat_bg, up_obj, lat_obj, s = field_set("F")
    for kw in (dict(min_valid=0.9), dict(min_valid=0.0, weights=(2.0, 0.5)), dict(min_valid=1.0, weights=(0.0, 1.0))):
        d = placement_scores(dev(up_bg), dev(lat_bg), dev(up_obj), dev(lat_obj), **kw)
        ref = reference(up_bg, lat_bg, up_obj, lat_obj, s, **kw)
        d = {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in d.items()}
        inf = np.isinf(ref["pfd_deg"])
        assert (np.isinf(d["pfd_deg"]) == inf).all() and not inf.all() and inf.any() == (kw["min_valid"] > 0)
        b_up, b_lat = mean_bounds(ref, 63)
        w = kw.get("weights", (1.0, 1.0))
        assert (np.abs(d["pfd_deg"][~inf] - ref["pfd_deg"][~inf]) <= (w[0] * b_up + w[1] * b_lat)[~inf]).all()
    d = placement_scores(dev(up_bg), dev(lat_bg), dev(up_obj), torch.full((9, 7), float("nan"), device="cuda"), min_valid=0.0)
    assert torch.isinf(d["pfd_deg"]).all() and d["best_offset"].tolist() == [-1, -1] and int(d["valid_pixels"].sum()) == 0


def test_model_method_equals_the_function():
    from perspectivefields_amd import PerspectiveFields, placement_scores

    rng = np.random.default_rng(21)
    m = PerspectiveFields("Paramnet-360Cities-edina-centered", weights="synthetic:0").eval().cuda()
    bg = m.inference_batch([rng.integers(0, 256, (64, 64, 3), dtype=np.uint8)])
    obj = m.inference_batch([rng.integers(0, 256, (24, 24, 3), dtype=np.uint8)])
    assert tuple(bg[0]["pred_gravity_original"].shape) == (2, 64, 64) and tuple(obj[0]["pred_latitude_original"].shape) == (24, 24)
    got = m.placement_scores(bg[0], obj[0], stride=4)
    want = placement_scores(bg[0]["pred_gravity_original"], bg[0]["pred_latitude_original"], obj[0]["pred_gravity_original"], obj[0]["pred_latitude_original"], stride=4)
    assert isinstance(got, dict) and got["pfd_deg"].shape == (11, 11) and got["stride"] == 4
    assert all(torch.equal(got[k], want[k]) for k in ("pfd_deg", "up_mean_deg", "lat_mean_deg", "valid_pixels", "best_offset", "best_pfd_deg"))
    assert torch.isfinite(got["pfd_deg"]).all() and 0 <= int(got["best_offset"][0]) <= 40 and int(got["best_offset"][0]) % 4 == 0
    lists = m.placement_scores(bg, obj, stride=4)
    assert isinstance(lists, list) and len(lists) == 1 and torch.equal(lists[0]["pfd_deg"], want["pfd_deg"])
