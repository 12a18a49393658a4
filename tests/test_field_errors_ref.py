"""fp64 numpy statement of the field-error definitions (include/pf_hip.h pf_field_errors), checked on cases that
can be computed by hand; plus the host-side contract: output columns against the header, argument errors, and the dataset accumulator's
CPU bookkeeping (add_errors / merge / summary / all_reduce over gloo).  tests/test_gpu_field_errors.py uses the same reference on the
GPU results.  No GPU needed."""
import os
import re
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = 1.0 / 64.0   # the accumulator's bin width in degrees


def errors(up_pred, lat_pred, up_gt, lat_gt):
    """(2,H,W), (H,W), (2,H,W), (H,W) of any float type -> e_up, e_lat (H,W) fp64 degrees, NaN where the pixel is invalid"""
    p, g = np.asarray(up_pred, dtype=np.float64), np.asarray(up_gt, dtype=np.float64)
    lp, lg = np.asarray(lat_pred, dtype=np.float64), np.asarray(lat_gt, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        valid = np.isfinite(p).all(0) & np.isfinite(g).all(0) & np.isfinite(lp) & np.isfinite(lg)
        valid &= ((p * p).sum(0) >= 1e-12) & ((g * g).sum(0) >= 1e-12)
        e_up = np.degrees(np.arctan2(np.abs(p[0] * g[1] - p[1] * g[0]), p[0] * g[0] + p[1] * g[1]))
        e_lat = np.abs(lp - lg)
    return np.where(valid, e_up, np.nan), np.where(valid, e_lat, np.nan)


def metric_stats(e, threshold=5.0):
    """statistics of one metric over its non-NaN entries, in the order mean, median, rmse, max, frac_below"""
    v = np.asarray(e, dtype=np.float64).ravel()
    v = np.sort(v[~np.isnan(v)])
    n = v.size
    if n == 0:
        return [float("nan")] * 5
    return [float(v.mean()), float((v[(n - 1) // 2] + v[n // 2]) / 2), float(np.sqrt((v * v).mean())), float(v[-1]), float((v < threshold).sum() / n)]


def stats(e_up, e_lat, threshold=5.0):
    """the per-image dict of field_errors, from error maps"""
    from perspectivefields_amd.perspectivefields import _FERR_COLS

    vals = metric_stats(e_up, threshold) + metric_stats(e_lat, threshold) + [int((~np.isnan(np.asarray(e_up))).sum())]
    return dict(zip(_FERR_COLS, vals))


def _rotated(deg, base=(0.6, -0.8)):
    a = np.radians(deg)
    return np.array([np.cos(a) * base[0] - np.sin(a) * base[1], np.sin(a) * base[0] + np.cos(a) * base[1]])


@pytest.mark.parametrize("deg", [0.0, 1e-4, 5.0, 90.0, 180.0, -30.0, 179.999])
def test_up_error_is_the_rotation_angle(deg):
    g = np.array([0.6, -0.8])
    p = _rotated(deg) * 1.7   # no normalisation needed
    e_up, e_lat = errors(p.reshape(2, 1, 1), [[3.0]], g.reshape(2, 1, 1), [[-1.5]])
    assert abs(e_up[0, 0] - abs(deg)) <= 1e-9 * max(1.0, abs(deg)) + 1e-13
    assert e_lat[0, 0] == 4.5


def test_small_angles_keep_their_accuracy():
    """atan2 of cross and dot, not acos of the dot product: 1e-4 degree survives to 1e-6 relative (acos would return 0 or 1e-6 rad steps)"""
    e_up, _ = errors(_rotated(1e-4).reshape(2, 1, 1), [[0.0]], np.array([0.6, -0.8]).reshape(2, 1, 1), [[0.0]])
    assert abs(e_up[0, 0] - 1e-4) <= 1e-10


def test_masking_non_finite_and_zero_length():
    H, W = 3, 4
    g = np.tile(np.array([0.0, -1.0]).reshape(2, 1, 1), (1, H, W))
    p = np.tile(_rotated(10.0, (0.0, -1.0)).reshape(2, 1, 1), (1, H, W))
    lp, lg = np.full((H, W), 2.0), np.full((H, W), -1.0)
    p[0, 0, 0] = np.nan
    p[1, 0, 1] = np.inf
    g[1, 0, 2] = np.nan
    lp[0, 3] = np.nan
    lg[1, 0] = -np.inf
    p[:, 1, 1] = 0.0            # zero-length prediction
    g[:, 1, 2] = (1e-7, 0.0)    # squared length 1e-14 < 1e-12
    g[:, 1, 3] = (0.0, -2e-6)   # squared length 4e-12: valid
    e_up, e_lat = errors(p, lp, g, lg)
    invalid = np.zeros((H, W), bool)
    invalid[0, :] = True
    invalid[1, :3] = True
    assert (np.isnan(e_up) == invalid).all() and (np.isnan(e_lat) == invalid).all()
    assert np.allclose(e_up[~invalid], 10.0, atol=1e-9) and (e_lat[~invalid] == 3.0).all()
    s = stats(e_up, e_lat)
    assert s["valid_pixels"] == H * W - 7 and abs(s["up_median_deg"] - 10.0) < 1e-9 and s["lat_max_deg"] == 3.0


@pytest.mark.parametrize("vals,median", [([], None), ([7.0], 7.0), ([1.0, 4.0], 2.5), ([9.0, 1.0, 4.0], 4.0), ([9.0, 1.0, 4.0, 6.0], 5.0),
                                         ([2.0, 2.0, 2.0, 8.0, 8.0, 8.0], 5.0)])
def test_statistics_by_hand(vals, median):
    e = np.array(vals + [np.nan, np.nan], dtype=np.float64).reshape(1, -1)
    s = stats(e, 2 * e, threshold=5.0)
    assert s["valid_pixels"] == len(vals)
    if not vals:
        assert all(np.isnan(s[k]) for k in s if k != "valid_pixels")
        return
    v = np.array(vals)
    assert s["up_median_deg"] == median == np.median(v) and s["lat_median_deg"] == 2 * median
    assert s["up_mean_deg"] == pytest.approx(v.mean(), rel=1e-15) and s["up_rmse_deg"] == pytest.approx(np.sqrt((v * v).mean()), rel=1e-15)
    assert s["up_max_deg"] == v.max() and s["lat_max_deg"] == 2 * v.max()
    assert s["up_frac_below"] == (v < 5.0).mean() and s["lat_frac_below"] == (2 * v < 5.0).mean()   # strict: 5.0 itself is not below


def test_threshold_is_strict():
    e = np.array([[4.999, 5.0, 5.001]])
    assert stats(e, e)["up_frac_below"] == pytest.approx(1 / 3)


def test_output_columns_match_the_header():
    """the Python dict keys follow the PF_FERR_COL_* order of include/pf_hip.h; the bin and total constants agree too"""
    from perspectivefields_amd import perspectivefields as P

    hdr = open(os.path.join(ROOT, "include", "pf_hip.h")).read()
    cols = {m[0]: int(m[1]) for m in re.findall(r"#define PF_FERR_COL_([A-Z_]+) (\d+)", hdr)}
    assert int(re.search(r"#define PF_FERR_COLS (\d+)", hdr)[1]) == len(P._FERR_COLS) == len(cols)
    key = lambda c: "valid_pixels" if c == "VALID_PIXELS" else c.lower() + ("" if c.endswith("FRAC_BELOW") else "_deg")
    assert {key(c): v for c, v in cols.items()} == {k: i for i, k in enumerate(P._FERR_COLS)}
    assert int(re.search(r"#define PF_FERR_BINS (\d+)", hdr)[1]) == P._FERR_BINS == 180 * P._FERR_BINS_PER_DEG
    assert int(re.search(r"#define PF_FERR_BINS_PER_DEG (\d+)", hdr)[1]) == P._FERR_BINS_PER_DEG
    sums = {m[0]: int(m[1]) for m in re.findall(r"#define PF_FERR_SUM_([A-Z0-9]+) (\d+)", hdr)}
    assert sums == {"N": 0, "E": 1, "E2": 2, "MAX": 3, "BELOW": 4} and int(re.search(r"#define PF_FERR_SUMS (\d+)", hdr)[1]) == len(P._FERR_SUMS)


def test_public_names():
    import perspectivefields_amd as pkg

    assert {"field_errors", "FieldErrorAccumulator"} <= set(pkg.__all__)
    assert callable(pkg.field_errors) and callable(pkg.FieldErrorAccumulator)
    assert callable(pkg.PerspectiveFields.field_errors)


def test_every_public_name_resolves_to_one_object():
    """every name of __all__ resolves lazily, is a function or a class (model_zoo: the table), and is the object that perspectivefields.py re-exports"""
    from collections.abc import Mapping

    import perspectivefields_amd as pkg
    from perspectivefields_amd import perspectivefields as pfm

    assert len(pkg.__all__) == len(set(pkg.__all__)) == 32
    for name in pkg.__all__:
        obj = getattr(pkg, name)
        assert isinstance(obj, Mapping) if name == "model_zoo" else callable(obj), name
        assert getattr(pfm, name) is obj, name
    with pytest.raises(AttributeError):
        pkg.no_such_name


def test_field_errors_argument_errors_without_a_gpu():
    from perspectivefields_amd import FieldErrorAccumulator, field_errors
    from perspectivefields_amd.engine import PfError

    up, lat = torch.zeros(2, 8, 9), torch.zeros(8, 9)
    with pytest.raises(PfError):
        field_errors(up, lat, up, lat)                              # CPU tensors: no CPU path
    with pytest.raises(PfError):
        field_errors([up], [lat], [up], [lat], return_maps=True)
    with pytest.raises(ValueError):
        field_errors([up, up], [lat, lat], [up], [lat])             # list lengths
    with pytest.raises(ValueError):
        field_errors([up], [lat, lat], [up], [lat])
    with pytest.raises(ValueError):
        field_errors(up, lat, torch.zeros(2, 8, 8), torch.zeros(8, 8))   # shapes
    with pytest.raises(ValueError):
        field_errors(torch.zeros(3, 8, 9), lat, up, lat)
    with pytest.raises(ValueError):
        field_errors(up, lat, up, lat, threshold_deg=0.0)
    with pytest.raises(ValueError):
        field_errors(up, lat, up, lat, threshold_deg=float("nan"))
    with pytest.raises(TypeError):
        field_errors(up.numpy(), lat.numpy(), up, lat)
    with pytest.raises(TypeError):
        field_errors([up.numpy()], [lat], [up], [lat])
    with pytest.raises(ValueError):
        FieldErrorAccumulator("cpu", threshold_deg=-1.0)
    with pytest.raises(PfError):
        FieldErrorAccumulator("cpu").update(up, lat, up, lat)       # the kernel path is GPU only


def test_c_abi_argument_errors_and_workspace_size():
    """host arithmetic and argument checks of the C ABI: they return before any device work, so they run without a GPU"""
    import ctypes

    from perspectivefields_amd.engine import load_library

    lib = load_library()
    hw = lambda *s: (ctypes.c_int32 * len(s))(*s)
    one = lib.pf_field_errors_workspace_bytes(1, hw(640, 640))
    two = lib.pf_field_errors_workspace_bytes(2, hw(640, 640, 1, 1))
    assert 2 * 640 * 640 * 4 < one < two
    assert lib.pf_field_errors_workspace_bytes(1, hw(0, 640)) == 0
    assert lib.pf_field_errors_workspace_bytes(1, hw(65536, 65536)) == 0
    assert lib.pf_field_errors_workspace_bytes(0, hw(640, 640)) == 0
    ptr = (ctypes.c_void_p * 1)(0x1000)   # never dereferenced: every call below fails its argument check first
    nul = (ctypes.c_void_p * 1)(None)
    call = lambda **kw: lib.pf_field_errors(*[{**dict(device=0, batch=1, hw=hw(8, 8), up_p=ptr, lat_p=ptr, up_g=ptr, lat_g=ptr, thr=5.0, out=None, eu=None, el=None,
                                                      hist=None, sums=None, ws=None, wsn=0, stream=None), **kw}[k]
                                              for k in ("device", "batch", "hw", "up_p", "lat_p", "up_g", "lat_g", "thr", "out", "eu", "el", "hist", "sums", "ws", "wsn", "stream")])
    assert call(batch=0) == -1
    assert call(thr=0.0) == -1 and call(thr=float("inf")) == -1
    assert call(hw=hw(0, 8)) == -1
    assert call(up_g=nul) == -1
    assert call(eu=ptr) == -1               # one map without the other
    assert call(hist=0x1000) == -1          # histogram without its totals
    assert call() == -4                     # valid arguments, no workspace: PF_ERR_WORKSPACE, still before any device work
    assert b"workspace" in lib.pf_last_error(None)


def _maps(seed, shape=(37, 53)):
    """error maps as the kernel would return them: fp32, NaN where invalid, values spread over small and large angles"""
    rng = np.random.default_rng(seed)
    e_up = np.abs(rng.normal(0.0, 2.0, shape)).astype(np.float32)
    e_lat = np.abs(rng.normal(0.0, 6.0, shape)).astype(np.float32)
    e_up[rng.random(shape) < 0.1] = 180.0 * rng.random()
    bad = rng.random(shape) < 0.15
    e_up[bad] = np.nan
    e_lat[bad] = np.nan
    return e_up, e_lat


def _check_summary(summary, e_up_all, e_lat_all, threshold):
    """exact statistics equal numpy's to fp64 rounding; the median to within one bin"""
    ref = stats(np.concatenate([e.ravel() for e in e_up_all]), np.concatenate([e.ravel() for e in e_lat_all]), threshold)
    assert summary["valid_pixels"] == ref["valid_pixels"]
    for k, v in ref.items():
        if k.endswith("median_deg"):
            assert abs(summary[k] - v) <= BIN, (k, summary[k], v)
        elif k.endswith("max_deg") or k.endswith("frac_below"):
            assert summary[k] == v, (k, summary[k], v)
        elif k != "valid_pixels":
            assert summary[k] == pytest.approx(v, rel=1e-13), (k, summary[k], v)


def test_accumulator_add_errors_merge_summary_on_cpu():
    from perspectivefields_amd import FieldErrorAccumulator

    maps = [_maps(s, shape) for s, shape in ((1, (37, 53)), (2, (64, 64)), (3, (1, 1)), (4, (5, 7)))]
    acc = FieldErrorAccumulator("cpu", threshold_deg=3.0)
    assert np.isnan(acc.summary()["up_median_deg"]) and acc.summary()["valid_pixels"] == 0
    acc.add_errors([torch.from_numpy(m[0]) for m in maps[:2]], [torch.from_numpy(m[1]) for m in maps[:2]])
    other = FieldErrorAccumulator("cpu", threshold_deg=3.0)
    for e_up, e_lat in maps[2:]:
        other.add_errors(torch.from_numpy(e_up), torch.from_numpy(e_lat))
    _check_summary(acc.summary(), [m[0] for m in maps[:2]], [m[1] for m in maps[:2]], 3.0)
    acc.merge(other)
    _check_summary(acc.summary(), [m[0] for m in maps], [m[1] for m in maps], 3.0)
    assert int(acc.hist[0].sum()) == int(acc.sums[0, 0]) == int(acc.hist[1].sum()) == sum(int((~np.isnan(m[0])).sum()) for m in maps)
    # the bin of an error is min(int(e * 64), 11519): 180 and beyond land in the last bin
    edge = FieldErrorAccumulator("cpu")
    edge.add_errors(torch.tensor([0.0, 1 / 64, 1 / 64 - 1e-6, 179.99, 180.0, float("nan")]), torch.tensor([0.5, 5.0, 200.0, 1e9, 0.0, float("nan")]))
    assert edge.hist[0].nonzero().flatten().tolist() == [0, 1, 11519] and edge.hist[0, 0] == 2 and edge.hist[0, 11519] == 2
    assert edge.hist[1].nonzero().flatten().tolist() == [0, 32, 320, 11519] and edge.hist[1, 11519] == 2
    assert edge.summary()["lat_frac_below"] == 2 / 5 and edge.summary()["valid_pixels"] == 5
    with pytest.raises(ValueError):
        acc.merge(FieldErrorAccumulator("cpu", threshold_deg=5.0))
    assert acc.all_reduce() is acc   # no process group: a no-op


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, q):
    from perspectivefields_amd import FieldErrorAccumulator

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        acc = FieldErrorAccumulator("cpu", threshold_deg=4.0)
        for seed in range(10 + rank, 16, world):   # each rank adds its own maps
            e_up, e_lat = _maps(seed)
            acc.add_errors(torch.from_numpy(e_up), torch.from_numpy(e_lat))
        acc.all_reduce()
        q.put((rank, acc.summary(), acc.hist.sum(1).tolist()))
    finally:
        dist.destroy_process_group()


def test_accumulator_all_reduce_world2():
    from perspectivefields_amd import FieldErrorAccumulator

    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=120) for _ in procs]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    single = FieldErrorAccumulator("cpu", threshold_deg=4.0)
    maps = [_maps(seed) for seed in range(10, 16)]
    for e_up, e_lat in maps:
        single.add_errors(torch.from_numpy(e_up), torch.from_numpy(e_lat))
    want = single.summary()
    for rank, got, counts in res:
        assert counts == single.hist.sum(1).tolist()
        for k, v in want.items():   # sums of the two ranks' partial sums: equal to the one-process sums to fp64 rounding
            assert got[k] == pytest.approx(v, rel=1e-13), (rank, k, got[k], v)
        assert got["up_median_deg"] == want["up_median_deg"] and got["up_max_deg"] == want["up_max_deg"] and got["valid_pixels"] == want["valid_pixels"]
    _check_summary(want, [m[0] for m in maps], [m[1] for m in maps], 4.0)
