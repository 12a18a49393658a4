"""Camera fit with intrinsics shared across the frames of one camera on the GPU (include/pf_hip.h pf_fit_camera_shared,
perspectivefields_amd.fit_camera_shared, PerspectiveFields.fit_camera(shared_intrinsics=)) against the fp64 reference of
tests/test_fit_camera_shared_ref.py: exact round trips, bit-equal shared columns, groups of any length anywhere in the batch, invariance of a
group's bits, the group of one, noisy input, robust loss, labels in any order, frames without a valid pixel, and fits of network output.

Bounds: those of the per-image GPU tests -- roll / pitch 5e-3 deg, rel_focal 2e-4 relative, rel_cx / rel_cy 2e-4 (tests/test_gpu_fit_camera.py), xi
2e-5 absolute (tests/test_gpu_fit_camera_usm.py BOUND_XI).  Every test prints its worst figures before it asserts."""
import numpy as np
import pytest
import torch

from tests.test_fit_camera_ref import model_fields
from tests.test_fit_camera_shared_ref import FIVE, NOISY_VFOVS, POSES, VFOVS, XIS, image_cost, noisy_reference, round_trip_group
from tests.test_fit_camera_usm_ref import focal_of, usm_fields

pytestmark = pytest.mark.gpu

ANGLE, FOCAL, PP, XI = 5e-3, 2e-4, 2e-4, 2e-5
SHARED = ("pred_vfov", "pred_rel_focal", "pred_general_vfov", "pred_rel_cx", "pred_rel_cy", "pred_xi", "fit_iterations", "fit_converged", "fit_group_cost")


def _dev(arrs):
    return [torch.from_numpy(np.ascontiguousarray(a)).float().cuda() for a in arrs]


def _fit(ups, lats, groups=None, **kw):
    from perspectivefields_amd import fit_camera_shared

    return fit_camera_shared(_dev(ups), _dev(lats), groups, **kw)


def _errors(ths, res):
    """worst (roll, pitch [deg], rel_focal relative, cx, cy, xi absolute) over the frames"""
    e = np.zeros(6)
    for th, d in zip(ths, res):
        got = [float(d["pred_roll"]), float(d["pred_pitch"]), float(d["pred_rel_focal"]), float(d["pred_rel_cx"]), float(d["pred_rel_cy"])]
        err = [abs(got[0] - np.degrees(th[0])), abs(got[1] - np.degrees(th[1])), abs(got[2] - th[2]) / th[2], abs(got[3] - th[3]), abs(got[4] - th[4]),
               abs(float(d["pred_xi"]) - th[5]) if len(th) == 6 else 0.0]
        e = np.maximum(e, err)
    return e


def _assert_recovered(what, ths, res):
    e = _errors(ths, res)
    print(f"\n{what}: roll {e[0]:.2e} pitch {e[1]:.2e} deg, f rel {e[2]:.2e}, cx {e[3]:.2e} cy {e[4]:.2e}, xi {e[5]:.2e}; steps {int(res[0]['fit_iterations'])}, "
          f"converged {bool(res[0]['fit_converged'])}")
    assert e[0] <= ANGLE and e[1] <= ANGLE and e[2] <= FOCAL and e[3] <= PP and e[4] <= PP and e[5] <= XI, (what, e)


def _assert_shared_bits(res):
    for k in SHARED:
        if k in res[0]:
            assert all(torch.equal(d[k], res[0][k]) for d in res), k


@pytest.mark.parametrize("vfov", VFOVS)
def test_pinhole_round_trips(vfov):
    ths, ups, lats = round_trip_group(0.5 / np.tan(np.radians(vfov) / 2))
    res = _fit(ups, lats)
    _assert_recovered(f"pinhole vFoV {vfov}", ths, res)
    _assert_shared_bits(res)
    assert all(int(d["fit_valid_pixels"]) == 48 * 64 and d["fit_group"] == 0 for d in res)
    assert "pred_xi" not in res[0] and len(res[0]) == 15


@pytest.mark.parametrize("xi", XIS)
@pytest.mark.parametrize("vfov", (55.0, 90.0))
def test_usm_round_trips(xi, vfov):
    ths, ups, lats = round_trip_group(focal_of(vfov, xi), xi=xi)
    res = _fit(ups, lats, distortion=True)
    _assert_recovered(f"USM xi {xi} vFoV {vfov}", ths, res)
    _assert_shared_bits(res)


def test_five_parameter_round_trip():
    ths, ups, lats = round_trip_group(*FIVE)
    res = _fit(ups, lats, free_principal_point=True, max_iter=60)
    _assert_recovered("pinhole, free principal point", ths, res)
    _assert_shared_bits(res)


@pytest.mark.parametrize("xi", (None, 0.6))
def test_round_trip_at_an_unaligned_size(xi):
    """97 x 131: the accumulate kernel's scalar load path"""
    f = 0.5 / np.tan(np.radians(55.0) / 2) if xi is None else focal_of(55.0, xi)
    ths, ups, lats = round_trip_group(f, xi=xi, H=97, W=131)
    res = _fit(ups, lats, distortion=xi is not None)
    _assert_recovered(f"97 x 131, xi {xi}", ths, res)
    _assert_shared_bits(res)
    assert all(int(d["fit_valid_pixels"]) == 97 * 131 for d in res)


def _geometry():
    """105 frames of 24 x 32 in camera groups of 3, 31, 1 and 70: groups that start inside a launch group of 32 images, straddle its boundary and hold
    more images than a wave has lanes; each with its own focal length"""
    sizes, vfovs = (3, 31, 1, 70), (40.0, 75.0, 60.0, 100.0)
    rng = np.random.default_rng(7)
    ths, labels = [], []
    for g, (n, v) in enumerate(zip(sizes, vfovs)):
        for _ in range(n):
            ths.append(np.array([np.radians(rng.uniform(-30, 30)), np.radians(rng.uniform(-50, 50)), 0.5 / np.tan(np.radians(v) / 2), 0.0, 0.0]))
            labels.append(g)
    fl = [model_fields(t, 24, 32) for t in ths]
    return sizes, ths, labels, _dev([u for u, _ in fl]), _dev([l for _, l in fl])


def test_group_geometry_and_invariance():
    from perspectivefields_amd import fit_camera_shared

    sizes, ths, labels, ups, lats = _geometry()
    res = fit_camera_shared(ups, lats, labels)
    again = fit_camera_shared(ups, lats, labels)
    i0 = 0
    for g, n in enumerate(sizes):
        rows = res[i0:i0 + n]
        _assert_recovered(f"group {g} of {n}", ths[i0:i0 + n], rows)
        _assert_shared_bits(rows)
        alone = fit_camera_shared(ups[i0:i0 + n], lats[i0:i0 + n])
        for a, b, c in zip(rows, alone, again[i0:i0 + n]):
            assert a["fit_group"] == g and c["fit_group"] == g
            for k in a:
                if k != "fit_group":
                    assert torch.equal(a[k], b[k]) and torch.equal(a[k], c[k]), (g, k, a[k], b[k], c[k])
        i0 += n
    assert len({float(r["pred_rel_focal"]) for r in res}) == len(sizes)


def test_a_group_of_one_agrees_with_the_per_image_fit():
    """a noisy frame, so that the minimum both fits reach is a point and not the rounding noise of exact input; the two reach it on different
    arithmetic (block elimination against one Cholesky factorisation), so the agreement is not bitwise"""
    from perspectivefields_amd import fit_camera_params

    for vfov in NOISY_VFOVS:
        _, ups, lats, _, _, _ = noisy_reference(vfov)
        u, l = _dev(ups[:1]), _dev(lats[:1])
        one = fit_camera_params(u[0], l[0], max_iter=60)
        d = _fit(ups[:1], lats[:1], max_iter=60)[0]
        e = (abs(float(d["pred_roll"]) - float(one["pred_roll"])), abs(float(d["pred_pitch"]) - float(one["pred_pitch"])),
             abs(float(d["pred_rel_focal"]) / float(one["pred_rel_focal"]) - 1.0))
        print(f"\ngroup of one at vFoV {vfov}: roll {e[0]:.2e} pitch {e[1]:.2e} deg, f rel {e[2]:.2e}")
        assert e[0] <= 1e-4 and e[1] <= 1e-4 and e[2] <= 1e-5, e
        assert abs(float(d["fit_group_cost"]) - float(d["fit_cost"])) <= 1e-6 * float(d["fit_cost"])


@pytest.mark.parametrize("vfov", NOISY_VFOVS)
def test_noisy_set(vfov):
    from perspectivefields_amd import fit_camera_params

    f, ups, lats, ref_theta, ref_cost, _ = noisy_reference(vfov)
    res = _fit(ups, lats, max_iter=60)
    _assert_shared_bits(res)
    th = [(np.radians(float(d["pred_roll"])), np.radians(float(d["pred_pitch"])), float(d["pred_rel_focal"]), 0.0, 0.0) for d in res]
    c64 = sum(image_cost(t, u, l, False) for t, u, l in zip(th, ups, lats))
    got = float(res[0]["fit_group_cost"])
    singles = fit_camera_params(_dev(ups), _dev(lats), max_iter=60)
    joint = abs(np.log(float(res[0]["pred_rel_focal"]) / f))
    med = float(np.median([abs(np.log(float(d["pred_rel_focal"]) / f)) for d in singles]))
    print(f"\nnoisy set at vFoV {vfov}: group cost {got:.6f}, fp64 cost of the result {c64:.6f}, reference's {ref_cost:.6f}; |log f| joint {joint:.4f}, "
          f"median of the single-frame fits {med:.4f}; steps {int(res[0]['fit_iterations'])}")
    assert abs(got - c64) <= 1e-4 * c64
    assert c64 <= (1 + 1e-3) * ref_cost
    assert joint <= med
    assert abs(got - sum(float(d["fit_cost"]) for d in res)) <= 1e-5 * got


def test_huber_is_robust_to_outliers():
    from tests.test_gpu_fit_camera import _noisy, focal_of_vfov

    H, W, vfov = 120, 160, 70.0
    poses = ((12.0, -20.0), (-8.0, 15.0), (3.0, 30.0), (-15.0, -5.0))
    fl = [_noisy((np.radians(r), np.radians(p), focal_of_vfov(vfov), 0.0, 0.0), H, W, 3 + k) for k, (r, p) in enumerate(poses)]
    ups, lats = [u for u, _ in fl], [l for _, l in fl]
    err = {}
    for loss in ("huber", "l2"):
        res = _fit(ups, lats, loss=loss, huber_delta_deg=2.0)
        err[loss] = sum(abs(float(d["pred_roll"]) - r) + abs(float(d["pred_pitch"]) - p) for d, (r, p) in zip(res, poses)) + abs(float(res[0]["pred_vfov"]) - vfov)
    print(f"\nsummed parameter error in degrees: huber {err['huber']:.3f}, l2 {err['l2']:.3f}")
    assert err["huber"] < err["l2"], err


def test_labels_in_any_order_come_back_in_the_callers_order():
    labels = ["b", ("cam", 2), "a", "b", "a", ("cam", 2), "b", "a"]
    vfov = {"a": 50.0, "b": 80.0, ("cam", 2): 110.0}
    size = {"a": (48, 64), "b": (40, 40), ("cam", 2): (31, 45)}
    ths = [np.array([np.radians(-20.0 + 6 * k), np.radians(25.0 - 7 * k), 0.5 / np.tan(np.radians(vfov[g]) / 2), 0.0, 0.0]) for k, g in enumerate(labels)]
    fl = [model_fields(t, *size[g]) for t, g in zip(ths, labels)]
    res = _fit([u for u, _ in fl], [l for _, l in fl], labels)
    assert [d["fit_group"] for d in res] == labels
    _assert_recovered("shuffled labels", ths, res)
    for g in vfov:
        _assert_shared_bits([d for d in res if d["fit_group"] == g])


@pytest.mark.parametrize("xi", (None, 0.25))
def test_a_frame_without_a_valid_pixel(xi):
    f = 0.5 / np.tan(np.radians(55.0) / 2) if xi is None else focal_of(55.0, xi)
    ths, ups, lats = round_trip_group(f, xi=xi)
    ups.insert(2, np.full((2, 48, 64), np.nan))
    lats.insert(2, np.full((48, 64), np.nan))
    res = _fit(ups, lats, distortion=xi is not None)
    dead = res.pop(2)
    assert int(dead["fit_valid_pixels"]) == 0 and not bool(dead["fit_converged"])
    _assert_recovered(f"the other seven frames, xi {xi}", ths, res)
    _assert_shared_bits(res)
    for k in ("pred_rel_focal", "pred_xi", "fit_iterations", "fit_group_cost"):
        if k in dead:
            assert torch.equal(dead[k], res[0][k]), k
    # no frame has a valid pixel: every row keeps its start and says so
    none = _fit(ups[2:3] * 2, lats[2:3] * 2)
    assert all(int(d["fit_valid_pixels"]) == 0 and not bool(d["fit_converged"]) and int(d["fit_iterations"]) == 0 for d in none)


def test_through_the_model():
    from tests.test_gpu_fit_camera import _network_fields

    model, preds = _network_fields("Paramnet-360Cities-edina-centered", [(120, 160)] * 4, 21)
    free = model.fit_camera(preds, max_iter=60)
    res = model.fit_camera(preds, shared_intrinsics=True, max_iter=60)
    assert len(res) == 4 and all(torch.equal(d["pred_rel_focal"], res[0]["pred_rel_focal"]) for d in res)
    joint, apart = float(res[0]["fit_group_cost"]), sum(float(d["fit_cost"]) for d in free)
    print(f"\nnetwork output: joint cost {joint:.4f}, sum of the per-image costs {apart:.4f}")
    assert joint >= apart * (1 - 1e-4)   # a constrained minimum cannot lie below the free one
    two = model.fit_camera(preds, shared_intrinsics=["x", "y", "x", "y"], init="paramnet")
    assert [d["fit_group"] for d in two] == ["x", "y", "x", "y"]
    assert torch.equal(two[0]["pred_rel_focal"], two[2]["pred_rel_focal"]) and torch.equal(two[1]["pred_rel_focal"], two[3]["pred_rel_focal"])
    assert "fit_group" not in model.fit_camera(preds, shared_intrinsics=None)[0]
