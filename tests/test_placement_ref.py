"""Placement scores (include/pf_hip.h pf_place_scores, perspectivefields_amd.placement_scores): the fp64 reference the GPU tests compare against, the
fixed inputs, and the host-side contract.  No GPU here.

Model, in fp64 on the fp32 inputs.  A field pixel is valid when its three values are finite and the fp32 squared length of its up vector is >= 1e-12
and finite.  The placements are (j, i), 0 <= j < P = (H - h) // stride + 1, 0 <= i < Q = (W - w) // stride + 1; the object's pixel (r, c) lies on the
background's (j stride + r, i stride + c).  Per pair of valid pixels e_up = atan2(|cross|, dot) of the two up vectors in degrees and e_lat =
|lat_bg - lat_obj|; per placement n = the valid pairs, S_up = sum e_up, S_lat = sum e_lat.  up_mean = S_up / n, lat_mean = S_lat / n,
pfd = w_up up_mean + w_lat lat_mean, +inf where n < min_valid x (valid pixels of the object) or n = 0; the best offset is the first minimum in
row-major order in background pixels, (-1, -1) if every placement is +inf."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

from oracle.pf_oracle import fields_from_params
from tests.test_field_errors_ref import errors

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNK = 1024   # object pixels one thread of the score kernel adds in fp32 (csrc/pf_kernels.h PlaceBatch::CHUNK)


# ---------------------------------------------------------------- the reference
def field_valid(up, lat):
    """(2,h,w), (h,w) -> bool (h,w)"""
    u, l = np.asarray(up, dtype=np.float32), np.asarray(lat, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        l2 = u[0] * u[0] + u[1] * u[1]   # float32
        return np.isfinite(u).all(0) & np.isfinite(l) & (l2 >= np.float32(1e-12)) & np.isfinite(l2)


def placements(H, h, stride):
    return (H - h) // stride + 1


def ref_placement(up_bg, lat_bg, up_obj, lat_obj, stride):
    """brute force: (S_up, S_lat, n), each (P, Q) float64"""
    ub, lb = np.asarray(up_bg, dtype=np.float64), np.asarray(lat_bg, dtype=np.float64)
    uo, lo = np.asarray(up_obj, dtype=np.float64), np.asarray(lat_obj, dtype=np.float64)
    vb, vo = field_valid(up_bg, lat_bg), field_valid(up_obj, lat_obj)
    (H, W), (h, w) = lb.shape, lo.shape
    P, Q = placements(H, h, stride), placements(W, w, stride)
    S_up, S_lat, n = np.zeros((P, Q)), np.zeros((P, Q)), np.zeros((P, Q))
    with np.errstate(invalid="ignore", over="ignore"):
        for r in range(h):
            for c in range(w):
                if not vo[r, c]:
                    continue
                win = (slice(r, r + (P - 1) * stride + 1, stride), slice(c, c + (Q - 1) * stride + 1, stride))
                bx, by, v = ub[0][win], ub[1][win], vb[win]
                e_up = np.degrees(np.arctan2(np.abs(bx * uo[1, r, c] - by * uo[0, r, c]), bx * uo[0, r, c] + by * uo[1, r, c]))
                e_lat = np.abs(lb[win] - lo[r, c])
                S_up += np.where(v, e_up, 0.0)
                S_lat += np.where(v, e_lat, 0.0)
                n += v
    return S_up, S_lat, n


def ref_scores(S_up, S_lat, n, obj_valid, stride, min_valid=0.5, weights=(1.0, 1.0)):
    """the maps and the best offset that placement_scores derives"""
    with np.errstate(invalid="ignore", divide="ignore"):
        up_mean, lat_mean = S_up / n, S_lat / n
    ok = (n >= min_valid * obj_valid) & (n > 0)
    pfd = np.where(ok, weights[0] * np.where(ok, up_mean, 0.0) + weights[1] * np.where(ok, lat_mean, 0.0), np.inf)
    k = int(np.argmin(pfd))   # the first minimum
    best = (k // pfd.shape[1] * stride, k % pfd.shape[1] * stride) if np.isfinite(pfd.flat[k]) else (-1, -1)
    return dict(pfd_deg=pfd, up_mean_deg=up_mean, lat_mean_deg=lat_mean, valid_pixels=n.astype(np.int64), best_offset=best, best_pfd_deg=pfd.flat[k])


def reference(up_bg, lat_bg, up_obj, lat_obj, stride, **kw):
    S_up, S_lat, n = ref_placement(up_bg, lat_bg, up_obj, lat_obj, stride)
    d = ref_scores(S_up, S_lat, n, int(field_valid(up_obj, lat_obj).sum()), stride, **kw)
    d.update(S_up=S_up, S_lat=S_lat, n=n)
    return d


# ---------------------------------------------------------------- fixed inputs (shared with tests/test_gpu_placement.py)
def camera_fields(roll, pitch, vfov, H, W, seed=None):
    """the oracle's fields in the device layout, float32: up (2,H,W), lat (H,W); with a seed, 2 degrees of Gaussian noise on the up angle and on
    the latitude"""
    up, lat, _ = fields_from_params(roll, pitch, vfov, 0.0, 0.0, H, W)
    if seed is not None:
        rng = np.random.default_rng(seed)
        ang = np.arctan2(up[..., 1], up[..., 0]) + np.radians(2.0) * rng.standard_normal((H, W))
        up = np.stack([np.cos(ang), np.sin(ang)], axis=-1)
        lat = lat + 2.0 * rng.standard_normal((H, W))
    return np.ascontiguousarray(np.moveaxis(up, -1, 0)).astype(np.float32), np.ascontiguousarray(lat).astype(np.float32)


def ellipse(h, w):
    r, c = np.mgrid[0:h, 0:w]
    return ((r - (h - 1) / 2) / (h / 2)) ** 2 + ((c - (w - 1) / 2) / (w / 2)) ** 2 <= 1.0


BG_CAM, OTHER_CAM = (8.0, 20.0, 60.0), (-5.0, 5.0, 60.0)
PLANT = (13, 22, 9, 7)   # row, col, h, w of the planted object


def crop(up, lat, r, c, h, w):
    return np.ascontiguousarray(up[:, r:r + h, c:c + w]), np.ascontiguousarray(lat[r:r + h, c:c + w])


@functools.lru_cache(None)
def field_set(name):
    """(up_bg, lat_bg, up_obj, lat_obj, stride) of the sets A - F of tests/test_gpu_placement.py, read only.  The objects of A, C, D, E, F are cut from
    another noisy realisation of the background's camera, B's from another camera."""
    if name in ("A", "F"):
        bg = camera_fields(*BG_CAM, 40, 56, seed=1)
        obj = crop(*camera_fields(*BG_CAM, 40, 56, seed=2), *PLANT)
        if name == "F":
            bg[1][10:15, :] = np.nan
            bg[1][:6, :6] = np.nan
        s = 1
    elif name == "B":
        bg, obj, s = camera_fields(*BG_CAM, 37, 53, seed=3), camera_fields(*OTHER_CAM, 20, 33, seed=4), 3
    elif name == "C":
        bg = camera_fields(*BG_CAM, 40, 42, seed=5)
        obj = crop(*camera_fields(*BG_CAM, 40, 42, seed=6), 4, 3, 33, 35)
        obj[1][~ellipse(33, 35)] = np.nan
        s = 1
    elif name == "D":
        bg, obj, s = camera_fields(*BG_CAM, 40, 56, seed=7), camera_fields(*BG_CAM, 40, 56, seed=8), 1
    elif name == "E":
        bg = camera_fields(*BG_CAM, 40, 56, seed=9)
        obj, s = crop(*camera_fields(*BG_CAM, 40, 56, seed=10), 20, 30, 1, 1), 1
    else:
        raise KeyError(name)
    out = (bg[0], bg[1], obj[0], obj[1])
    for a in out:
        a.setflags(write=False)
    return out + (s,)


@functools.lru_cache(None)
def set_reference(name):
    return reference(*field_set(name))


@functools.lru_cache(None)
def planted():
    up, lat = camera_fields(*BG_CAM, 40, 56)
    return (up, lat) + crop(up, lat, *PLANT) + (1,)


# ---------------------------------------------------------------- the reference against errors() and by hand
def test_reference_equals_field_errors_on_every_slice():
    up_bg, lat_bg, up_obj, lat_obj, s = field_set("B")
    up_obj, lat_obj = np.array(up_obj), np.array(lat_obj)
    lat_obj[3, 4], up_obj[:, 7, 7] = np.nan, 0.0
    up_bg = np.array(up_bg)
    up_bg[0, 20, 20] = np.inf
    S_up, S_lat, n = ref_placement(up_bg, lat_bg, up_obj, lat_obj, s)
    assert S_up.shape == (6, 7)
    for j in range(6):
        for i in range(7):
            e_up, e_lat = errors(up_bg[:, j * s:j * s + 20, i * s:i * s + 33], lat_bg[j * s:j * s + 20, i * s:i * s + 33], up_obj, lat_obj)
            assert n[j, i] == (~np.isnan(e_up)).sum()
            assert abs(S_up[j, i] - np.nansum(e_up)) <= 1e-9 and abs(S_lat[j, i] - np.nansum(e_lat)) <= 1e-9


def test_planted_object_is_found_exactly():
    up_bg, lat_bg, up_obj, lat_obj, s = planted()
    r = reference(up_bg, lat_bg, up_obj, lat_obj, s)
    pfd = r["pfd_deg"]
    assert pfd.shape == (32, 50) and (r["valid_pixels"] == 63).all()
    assert pfd[13, 22] == 0.0 and r["best_offset"] == (13, 22) and r["best_pfd_deg"] == 0.0
    assert (pfd == 0.0).sum() == 1
    second = np.sort(pfd.ravel())[1]
    print(f"second-best PFD {second:.3f} deg, up-only {np.sort(r['up_mean_deg'].ravel())[1]:.3f}, latitude-only {np.sort(r['lat_mean_deg'].ravel())[1]:.3f}")
    assert second >= 0.5
    assert np.sort(r["up_mean_deg"].ravel())[1] > 0 and np.sort(r["lat_mean_deg"].ravel())[1] > 0


def _one(up, lat=0.0):
    return np.asarray(up, dtype=np.float32).reshape(2, 1, 1), np.full((1, 1), lat, dtype=np.float32)


def test_wrap_around_gives_the_small_angle():
    S_up, S_lat, n = ref_placement(*_one((-1.0, 1e-3)), *_one((-1.0, -1e-3), 2.5), 1)
    assert n[0, 0] == 1 and abs(S_up[0, 0] - 0.1146) < 1e-4 and S_lat[0, 0] == 2.5
    # the angle-difference form the kernel uses: the same number from two angles on either side of +-180
    t = float(np.float32(1e-3))   # the fields are float32
    a, b = np.degrees(np.arctan2(t, -1.0)), np.degrees(np.arctan2(-t, -1.0))
    d = abs(a - b)
    assert d > 359.0 and abs(min(d, 360.0 - d) - S_up[0, 0]) < 1e-9


def test_masking_removes_exactly_its_pairs():
    up_bg, lat_bg, up_obj, lat_obj, s = (np.array(a) if isinstance(a, np.ndarray) else a for a in field_set("A"))
    base = ref_placement(up_bg, lat_bg, up_obj, lat_obj, s)[2]
    assert (base == 63).all()
    lat_obj[2, 3] = np.nan          # an object pixel: one pair less everywhere
    up_obj[:, 0, 0] = 0.0           # a zero up vector: another
    n = ref_placement(up_bg, lat_bg, up_obj, lat_obj, s)[2]
    assert (n == 61).all()
    up_bg[1, 20, 30] = np.inf       # a background pixel: one pair less at the placements that cover it with a valid object pixel
    n2 = ref_placement(up_bg, lat_bg, up_obj, lat_obj, s)[2]
    covered = np.zeros_like(n, dtype=bool)
    covered[20 - 8:20 + 1, 30 - 6:30 + 1] = True
    covered[20 - 2, 30 - 3] = covered[20, 30] = False   # there it meets the two invalid object pixels
    assert (n2 == np.where(covered, 60, 61)).all()


def test_threshold_and_best_offset_skip_thin_placements():
    S_up, S_lat = np.array([[1.0, 40.0], [30.0, 50.0]]), np.zeros((2, 2))
    n = np.array([[4.0, 10.0], [5.0, 10.0]])
    r = ref_scores(S_up, S_lat, n, obj_valid=10, stride=3)
    assert np.isinf(r["pfd_deg"][0, 0]) and r["pfd_deg"][1, 0] == 6.0 and r["best_offset"] == (0, 3) and r["best_pfd_deg"] == 4.0
    r = ref_scores(S_up, S_lat, n, obj_valid=10, stride=3, min_valid=0.4)
    assert r["best_offset"] == (0, 0) and r["best_pfd_deg"] == 0.25
    r = ref_scores(S_up, np.array([[8.0, 0.0], [0.0, 0.0]]), n, obj_valid=10, stride=1, min_valid=0.0, weights=(2.0, 0.5))
    assert r["pfd_deg"][0, 0] == 2.0 * 0.25 + 0.5 * 2.0


def test_empty_object_gives_inf_everywhere():
    up_bg, lat_bg, up_obj, lat_obj, s = field_set("A")
    r = reference(up_bg, lat_bg, up_obj, np.full_like(lat_obj, np.nan), s)
    assert np.isinf(r["pfd_deg"]).all() and r["best_offset"] == (-1, -1) and (r["valid_pixels"] == 0).all()
    r = reference(up_bg, lat_bg, up_obj, np.full_like(lat_obj, np.nan), s, min_valid=0.0)
    assert np.isinf(r["pfd_deg"]).all() and r["best_offset"] == (-1, -1)


def test_placement_counts():
    assert placements(37, 20, 3) == 6 and placements(37, 37, 5) == 1 and placements(37, 1, 1) == 37


def test_set_c_has_two_chunks_and_the_sets_have_no_borderline_length():
    assert 33 * 35 > CHUNK
    for name in "ABCDEF":
        up_bg, _, up_obj, _, _ = field_set(name)
        for u in (up_bg, up_obj):
            l2 = (u.astype(np.float64) ** 2).sum(0)
            assert ((np.abs(l2 - 1.0) < 1e-6) | (l2 == 0.0)).all()


# ---------------------------------------------------------------- host-side contract (fails before the feature exists)
def test_exports():
    import perspective2d
    import perspectivefields_amd

    assert "placement_scores" in perspectivefields_amd.__all__ and callable(perspectivefields_amd.placement_scores)
    assert callable(perspective2d.placement_scores) and callable(perspectivefields_amd.PerspectiveFields.placement_scores)


def test_symbols_prototypes_and_constants():
    from perspectivefields_amd.engine import _SIGNATURES, declared_symbols, load_library

    hdr = open(os.path.join(ROOT, "include", "pf_hip.h")).read()
    assert "int pf_place_scores(int device, int n_bg, const float* const* h_bg_up, const float* const* h_bg_lat, const int32_t* h_bg_hw" in hdr
    assert "size_t pf_place_scores_workspace_bytes(int n_bg, const int32_t* h_bg_hw" in hdr
    kh = open(os.path.join(ROOT, "perspectivefields_amd", "csrc", "pf_kernels.h")).read()
    assert f"static constexpr int CHUNK = {CHUNK};  // object pixels per block" in kh
    assert {"pf_place_scores", "pf_place_scores_workspace_bytes"} <= set(declared_symbols())
    res, args = _SIGNATURES["pf_place_scores"]
    assert res is ctypes.c_int and len(args) == 16 and args[14] is ctypes.c_size_t
    res, args = _SIGNATURES["pf_place_scores_workspace_bytes"]
    assert res is ctypes.c_size_t and len(args) == 7
    lib = load_library()
    assert hasattr(lib, "pf_place_scores") and hasattr(lib, "pf_place_scores_workspace_bytes")


def test_pf_place_scores_rejects_bad_arguments_before_device_work():
    from perspectivefields_amd.engine import load_library

    lib = load_library()
    ints = lambda *s: (ctypes.c_int32 * len(s))(*s)
    ptrs = lambda n: (ctypes.c_void_p * n)(*([0x1000] * n))
    dev = ctypes.c_void_p(4096)
    null2 = (ctypes.c_void_p * 2)(0x1000, 0)

    def call(n_bg=2, bg_up="ok", bg_lat="ok", bg_hw=None, n_obj=2, obj_up="ok", obj_lat="ok", obj_hw=None, n_pair=2, pairs=(0, 0, 1, 1), stride=2, out=dev,
             ws=dev, ws_bytes=None):
        bg_hw = bg_hw or ints(16, 24, 9, 9)
        obj_hw = obj_hw or ints(8, 24, 3, 5)
        c_pairs = None if pairs is None else ints(*pairs)
        if ws_bytes is None:
            ws_bytes = lib.pf_place_scores_workspace_bytes(n_bg, bg_hw, n_obj, obj_hw, n_pair, c_pairs, stride)
        arr = lambda v, n: ptrs(max(n, 1)) if v == "ok" else v
        rc = lib.pf_place_scores(0, n_bg, arr(bg_up, n_bg), arr(bg_lat, n_bg), bg_hw, n_obj, arr(obj_up, n_obj), arr(obj_lat, n_obj), obj_hw, n_pair, c_pairs,
                                 stride, out, ws, ws_bytes, None)
        return rc, lib.pf_last_error(None).decode()

    good = (2, ints(16, 24, 9, 9), 2, ints(8, 24, 3, 5), 2, ints(0, 0, 1, 1), 2)
    need = lib.pf_place_scores_workspace_bytes(*good)
    # two packed planes per side, and the records: pair 0 has 5 x 1 placements, pair 1 has 4 x 3, one chunk each
    assert need >= 8 * (16 * 24 + 9 * 9 + 8 * 24 + 3 * 5) + 12 * (5 + 12)
    assert lib.pf_place_scores_workspace_bytes(2, ints(16, 24, 9, 9), 2, ints(8, 24, 3, 5), 1, ints(1, 0), 2) == 0   # an object larger than its background
    assert lib.pf_place_scores_workspace_bytes(2, ints(16, 24, 9, 9), 2, ints(8, 24, 3, 5), 1, ints(0, 0), 0) == 0
    for kw, what in ((dict(n_bg=0), "n_bg"), (dict(n_obj=0), "n_obj"), (dict(n_pair=0), "n_pair"), (dict(pairs=None), "n_pair"), (dict(bg_up=None), "required"),
                     (dict(bg_lat=None), "required"), (dict(obj_up=None), "required"), (dict(obj_lat=None), "required"), (dict(out=None), "required"),
                     (dict(bg_up=null2), "NULL"), (dict(bg_lat=null2), "NULL"), (dict(obj_up=null2), "NULL"), (dict(obj_lat=null2), "NULL"),
                     (dict(bg_hw=ints(16, 0, 9, 9)), "smaller"), (dict(obj_hw=ints(0, 24, 3, 5)), "smaller"),
                     (dict(pairs=(0, 0, 2, 1)), "index"), (dict(pairs=(0, 2, 1, 1)), "index"), (dict(pairs=(-1, 0, 1, 1)), "index"),
                     (dict(pairs=(0, 0, 1, 0)), "larger than its background"), (dict(obj_hw=ints(17, 24, 3, 5)), "larger than its background"),
                     (dict(stride=0), "stride"), (dict(stride=-3), "stride"),
                     (dict(ws=None, ws_bytes=need), "workspace"), (dict(ws_bytes=need - 1), "workspace"), (dict(out=ctypes.c_void_p(4100)), "aligned")):
        rc, msg = call(**kw)
        assert rc == -1 and what in msg and msg.startswith("pf_place_scores: "), (kw, rc, msg)
    if not torch.cuda.is_available():   # good arguments pass the checks and fail on the missing device only
        rc, msg = call()
        assert rc == -2 and "no HIP device" in msg, (rc, msg)


def test_python_argument_errors_without_a_gpu():
    from perspectivefields_amd import PerspectiveFields, placement_scores
    from perspectivefields_amd.engine import PfError

    f = lambda *s: torch.zeros(s)
    up_bg, lat_bg, up_obj, lat_obj = f(2, 12, 16), f(12, 16), f(2, 5, 4), f(5, 4)
    for kw in (dict(up_obj=f(2, 13, 4), lat_obj=f(13, 4)), dict(up_obj=f(2, 5, 17), lat_obj=f(5, 17)), dict(up_obj=f(3, 5, 4)), dict(lat_obj=f(5, 5)),
               dict(up_bg=f(12, 16)), dict(up_bg=f(2, 0, 16), lat_bg=f(0, 16)), dict(stride=0), dict(min_valid=1.5), dict(min_valid=-0.1), dict(weights=(1.0, -1.0)),
               dict(weights=(1.0, float("nan"))), dict(weights=(1.0,)), dict(pairs=[]), dict(pairs=[(0, 1)]), dict(pairs=[(1, 0)]), dict(pairs=[(-1, 0)]),
               dict(mask=torch.ones(5, 5, dtype=torch.bool)), dict(mask=torch.ones(5, 4)), dict(mask=[None, None]),
               dict(up_bg=[up_bg, up_bg], lat_bg=[lat_bg]), dict(up_bg=[], lat_bg=[]), dict(up_obj=f(3, 2, 5, 4), lat_obj=f(2, 5, 4))):
        args = dict(up_bg=up_bg, lat_bg=lat_bg, up_obj=up_obj, lat_obj=lat_obj)
        args.update(kw)
        with pytest.raises(ValueError):
            placement_scores(args.pop("up_bg"), args.pop("lat_bg"), args.pop("up_obj"), args.pop("lat_obj"), **args)
    with pytest.raises(TypeError):
        placement_scores(up_bg, [lat_bg], up_obj, lat_obj)
    with pytest.raises(TypeError):
        placement_scores([up_bg.numpy()], [lat_bg.numpy()], up_obj, lat_obj)
    with pytest.raises(TypeError):
        placement_scores(up_bg, lat_bg, up_obj, lat_obj, stride=1.5)
    # good arguments on the CPU: no CPU path
    for args in ((up_bg, lat_bg, up_obj, lat_obj), ([up_bg, up_bg], [lat_bg, lat_bg], f(3, 2, 5, 4), f(3, 5, 4))):
        with pytest.raises(PfError):
            placement_scores(*args)
    with pytest.raises(PfError):
        placement_scores(up_bg, lat_bg, up_obj, lat_obj, mask=torch.ones(5, 4, dtype=torch.bool), stride=2, pairs=[(0, 0)])
    pred = lambda u, l: dict(pred_gravity_original=u, pred_latitude_original=l)
    with pytest.raises(PfError):
        PerspectiveFields.placement_scores(None, pred(up_bg, lat_bg), [pred(up_obj, lat_obj)] * 2)
    with pytest.raises(ValueError):
        PerspectiveFields.placement_scores(None, pred(up_obj, lat_obj), pred(up_bg, lat_bg))


def test_placement_kernels_are_in_the_library_without_scratch():
    """scripts/kernel_resources.py on the built library: the three kernels are there for gfx950 with no spilled register and no scratch; the score
    kernel's LDS is the chunk's records and offsets"""
    import importlib.util
    import shutil

    if not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf") or not shutil.which("c++filt"):
        pytest.skip("llvm-readelf / c++filt not available")
    from perspectivefields_amd import build as _b

    lib = _b.build(verbose=False)
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "scripts", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    by = {r["kernel"]: r for r in kr.kernels(lib)}
    for name, lds in (("pf::place_pack_kernel", 0), ("pf::place_score_kernel", 12 * CHUNK), ("pf::place_sum_kernel", 0)):
        r = by[name]
        assert r["spill"] == 0 and r["scratch"] == 0 and r["lds"] <= lds, r
