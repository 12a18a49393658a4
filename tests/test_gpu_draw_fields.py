"""Drawing of perspective fields on the GPU (include/pf_hip.h pf_draw_fields, perspectivefields_amd.draw_perspective_fields, draw_camera,
PerspectiveFields.draw_fields, perspective2d.utils) against the fp64 reference of tests/test_draw_fields_ref.py on its sets A - H.

Tolerance (section 17's rule).  The float32 picture is held to 4 x the error of the same formulas evaluated in numpy float32
in the same run (test_draw_fields_ref.fp32_floor: the device's division, sqrtf and contraction into fused multiply-adds differ from numpy's), in
units of the picture; set E's floor is 0 -- every pixel lies on its own anchor and is the arrow colour exactly -- and so is its allowance.  A uint8
pixel is held to 1/2 + that allowance of the fp64 value before rounding, which is less than the 1 LSB asked for.  No pixel is left out:
test_no_fixed_input_is_borderline shows that no input sits on a comparison."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests.test_draw_fields_ref import (SET_NAMES, arrow_coverage, arrow_length, draw_set, fp32_floor, picture, set_picture, set_reference, spacing, to_u8)
from tests.test_placement_ref import camera_fields, field_valid

pytestmark = pytest.mark.gpu


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()


@functools.lru_cache(None)
def gpu_run(name, dtype):
    from perspectivefields_amd import draw_perspective_fields

    up, lat, kw = draw_set(name)
    img = dev(set_picture(name, dtype))
    out = draw_perspective_fields(img, dev(up), dev(lat), **kw)
    assert out.shape == img.shape and out.dtype == img.dtype and out.data_ptr() != img.data_ptr()
    assert torch.equal(img.cpu(), torch.from_numpy(np.array(set_picture(name, dtype))))   # the input is left alone
    res = out.cpu().numpy()
    res.setflags(write=False)
    return res


@pytest.mark.parametrize("name", SET_NAMES)
def test_float32_picture_matches_the_fp64_reference(name):
    err = float(np.abs(gpu_run(name, "float32").astype(np.float64) - set_reference(name, "float32")).max())
    allowed = 4 * fp32_floor(name)
    print(f"set {name} float32: largest error {err:.3e} of the allowed {allowed:.3e} ({err / allowed if allowed else 0.0:.3f})")
    assert err <= allowed


@pytest.mark.parametrize("name", SET_NAMES)
def test_uint8_picture_is_within_one_lsb(name):
    got, ref = gpu_run(name, "uint8"), set_reference(name, "uint8")
    assert got.dtype == np.uint8
    err = float(np.abs(got.astype(np.float64) - np.clip(ref, 0, 255)).max())
    allowed = 0.5 + 4 * fp32_floor(name, "uint8")
    print(f"set {name} uint8: largest distance to the fp64 value {err:.4f} (allowed {allowed:.4f}); {int((got != to_u8(ref)).sum())} of {got.size} values differ from the rounded reference")
    assert err <= allowed < 1.0


@pytest.mark.parametrize("dtype", ["uint8", "float32"])
def test_nothing_to_draw_returns_the_input_bits(dtype):
    from perspectivefields_amd import draw_perspective_fields

    for name in ("A", "B"):   # the vector and the scalar loads and stores
        up, lat, kw = draw_set(name)
        img = dev(set_picture(name, dtype))
        assert torch.equal(draw_perspective_fields(img, dev(up), dev(lat), draw_up=False, draw_lat=False), img)
        assert torch.equal(draw_perspective_fields(img, dev(up), torch.full_like(dev(lat), float("nan"))), img)
        assert torch.equal(draw_perspective_fields(img, torch.zeros_like(dev(up)), dev(lat)), img)


@pytest.mark.parametrize("name", ["D", "G"])
def test_the_invalid_region_is_unchanged_except_under_arrows(name):
    up, lat, kw = draw_set(name)
    H, W = lat.shape
    valid = field_valid(up, lat)
    cov = arrow_coverage(up, lat, spacing(H, W, kw.get("density", 10)), arrow_length(W, kw.get("arrow_inv_len", 20)), 1.0)
    untouched, crossed = ~valid & (cov == 0), ~valid & (cov > 0.5)
    assert untouched.sum() > 300 and crossed.sum() >= 4
    for dtype in ("uint8", "float32"):
        got, img = gpu_run(name, dtype), set_picture(name, dtype)
        assert np.array_equal(got[untouched], img[untouched])
        assert (got[crossed] != img[crossed]).any(-1).all()


def test_batches_are_deterministic_and_independent():
    """33 images of two sizes and one spacing: one C call, two launches, both store paths in one launch"""
    from perspectivefields_amd import draw_perspective_fields

    other = camera_fields(-12.0, 33.0, 70.0, 43, 50)
    assert spacing(43, 50, 10) == spacing(40, 56, 10) == 4
    fields = [draw_set("A")[:2], other, draw_set("D")[:2], draw_set("G")[:2]]
    for dtype in (torch.uint8, torch.float32):
        imgs, ups, lats = [], [], []
        for k in range(33):
            up, lat = fields[k % 4]
            H, W = lat.shape
            imgs.append((dev(picture(H, W)) * (0.5 + k / 66)).to(dtype))
            ups.append(dev(up))
            lats.append(dev(lat))
        outs = draw_perspective_fields(imgs, ups, lats)
        assert isinstance(outs, list) and len(outs) == 33 and all(o.shape == i.shape and o.dtype == dtype for o, i in zip(outs, imgs))
        again = draw_perspective_fields(imgs, ups, lats)
        assert all(torch.equal(a, b) for a, b in zip(outs, again))
        for k in (0, 1, 2, 3, 17, 31, 32):
            assert torch.equal(draw_perspective_fields(imgs[k], ups[k], lats[k]), outs[k]), k
        perm = np.random.default_rng(5).permutation(33).tolist()
        shuffled = draw_perspective_fields([imgs[k] for k in perm], [ups[k] for k in perm], [lats[k] for k in perm])
        assert all(torch.equal(shuffled[j], outs[k]) for j, k in enumerate(perm))
        # batched tensors of one size, and images of two spacings (two C calls)
        same = [k for k in range(33) if k % 4 == 0][:5]
        batched = draw_perspective_fields(torch.stack([imgs[k] for k in same]), torch.stack([ups[k] for k in same]), torch.stack([lats[k] for k in same]))
        assert batched.shape == (5, 40, 56, 3) and all(torch.equal(batched[j], outs[k]) for j, k in enumerate(same))
        upb, latb, _ = draw_set("B")
        mixed = draw_perspective_fields([imgs[0], dev(picture(37, 53)).to(dtype), imgs[1]], [ups[0], dev(upb), ups[1]], [lats[0], dev(latb), lats[1]])
        assert torch.equal(mixed[0], outs[0]) and torch.equal(mixed[2], outs[1])
        assert torch.equal(mixed[1], draw_perspective_fields(dev(picture(37, 53)).to(dtype), dev(upb), dev(latb)))


@pytest.mark.parametrize("dtype", ["uint8", "float32"])
def test_out_and_in_place(dtype):
    from perspectivefields_amd import draw_perspective_fields

    up, lat, kw = draw_set("C")
    img = dev(set_picture("C", dtype))
    want = torch.from_numpy(np.array(gpu_run("C", dtype))).cuda()
    out = torch.empty_like(img)
    assert draw_perspective_fields(img, dev(up), dev(lat), out=out, **kw) is out and torch.equal(out, want)
    assert draw_perspective_fields(img, dev(up), dev(lat), out=img, **kw) is img and torch.equal(img, want)


@pytest.mark.parametrize("dtype", ["uint8", "float32"])
def test_c_entry_point_with_unaligned_pointers_takes_the_scalar_path(dtype):
    from perspectivefields_amd.engine import _stream_ptr, load_library

    lib = load_library()
    up, lat, kw = draw_set("A")   # W % 4 == 0: aligned pointers take the vector path
    H, W = lat.shape
    img, d_up, d_lat = dev(set_picture("A", dtype)), dev(up), dev(lat)
    esz = img.element_size()
    src = torch.zeros(img.numel() + 8, dtype=img.dtype, device="cuda")
    dst = torch.zeros(img.numel() + 8, dtype=img.dtype, device="cuda")
    src[1:1 + img.numel()] = img.reshape(-1)
    hw = (ctypes.c_int32 * 2)(H, W)
    one = lambda p: (ctypes.c_void_p * 1)(p)
    need = lib.pf_draw_fields_workspace_bytes(1, hw, 4)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    rgb = (ctypes.c_float * 3)(0.0, 255.0, 0.0)
    f_up, f_lat = torch.zeros(d_up.numel() + 4, device="cuda"), torch.zeros(d_lat.numel() + 4, device="cuda")   # the field planes one float off 16 bytes
    f_up[1:1 + d_up.numel()] = d_up.reshape(-1)
    f_lat[1:1 + d_lat.numel()] = d_lat.reshape(-1)
    for s_off, d_off, f_off in ((1, 1, 0), (0, 1, 0), (1, 0, 0), (0, 0, 1), (1, 1, 1)):
        dst.zero_()
        s_ptr = src.data_ptr() + esz if s_off else img.data_ptr()
        p_up, p_lat = (f_up.data_ptr() + 4, f_lat.data_ptr() + 4) if f_off else (d_up.data_ptr(), d_lat.data_ptr())
        rc = lib.pf_draw_fields(0, 1, hw, one(s_ptr), one(p_up), one(p_lat), one(dst.data_ptr() + d_off * esz), 0 if dtype == "uint8" else 1, 4,
                                1.0 / 20, 10.0, 0.5, 1.0, rgb, 3, ws.data_ptr(), need, _stream_ptr())
        assert rc == 0, lib.pf_last_error(None).decode()
        got = dst[d_off:d_off + img.numel()].reshape(H, W, 3).cpu().numpy()
        assert np.array_equal(got, gpu_run("A", dtype)), (s_off, d_off, f_off)
        assert int((dst[:d_off] != 0).sum()) == 0 and int((dst[d_off + img.numel():] != 0).sum()) == 0   # nothing outside the picture


def test_model_method_equals_the_function():
    from perspectivefields_amd import PerspectiveFields, draw_perspective_fields

    rng = np.random.default_rng(22)
    m = PerspectiveFields("Paramnet-360Cities-edina-centered", weights="synthetic:0").eval().cuda()
    pics = [rng.integers(0, 256, (64, 64, 3), dtype=np.uint8) for _ in range(2)]
    preds = m.inference_batch(pics)
    imgs = [dev(p) for p in pics]
    got = m.draw_fields(imgs, preds, density=8)
    want = draw_perspective_fields(imgs, [p["pred_gravity_original"] for p in preds], [p["pred_latitude_original"] for p in preds], density=8)
    assert isinstance(got, list) and all(torch.equal(a, b) for a, b in zip(got, want)) and got[0].shape == (64, 64, 3)
    one = m.draw_fields(imgs[1], preds[1], density=8)
    assert torch.equal(one, want[1]) and not torch.equal(one, imgs[1])


def test_draw_camera_is_fields_from_params_then_the_drawing():
    from perspectivefields_amd import draw_camera, draw_perspective_fields, fields_from_params

    imgs = [dev(set_picture("A", "uint8")), dev(set_picture("B", "uint8"))]
    rolls, xis = [8.0, -30.0], [0.0, 0.6]
    got = draw_camera(imgs, rolls, 20.0, 0.87, xi=xis, density=6)
    for k, (img, (H, W)) in enumerate(zip(imgs, ((40, 56), (37, 53)))):
        up, lat = fields_from_params(rolls[k], 20.0, 0.87, height=H, width=W, xi=xis[k])
        assert torch.equal(got[k], draw_perspective_fields(img, up, lat, density=6))
    single = draw_camera(imgs[0], 8.0, 20.0, 0.87)
    assert torch.equal(single, draw_perspective_fields(imgs[0], *fields_from_params(8.0, 20.0, 0.87, height=40, width=56)))
    tips_up = draw_camera(torch.zeros((40, 56, 3), device="cuda"), 0.0, 0.0, 0.87, draw_lat=False)   # an upright camera: arrows point to the top
    assert float(tips_up[0:2, 2, 1].min()) > 254.99 and float(tips_up[39, 2, 1]) < 0.01 and float(tips_up[..., 0].max()) == 0.0


def test_the_reference_shim_takes_radians_and_numpy():
    """deg -> rad in float32 by the caller (torch.deg2rad: one rounded constant, one product), rad -> deg in float64 and one rounding in the shim:
    the latitude comes back within 2.5 float32 ulps of 90 degrees, 1.9e-5 degrees.  The tint moves by at most alpha x 4.8 units per degree and
    a line's coverage by 1.9e-5 / |g| with |g| >= 1 degree per pixel in set A: less than 0.005 of a uint8 step in all, so a value may flip where
    it sits on a rounding boundary and bit equality is not asserted: at most 1 LSB, on at most 1 % of the values."""
    from perspective2d.utils import draw_from_r_p_f_cx_cy, draw_perspective_fields

    up, lat, kw = draw_set("A")
    img = np.array(set_picture("A", "uint8"))
    rad = torch.deg2rad(torch.from_numpy(np.array(lat)))
    got = draw_perspective_fields(img, torch.from_numpy(np.array(up)), rad, color=(0, 1, 0))
    want = gpu_run("A", "uint8")
    assert isinstance(got, np.ndarray) and got.dtype == np.uint8 and got.shape == img.shape
    diff = np.abs(got.astype(np.int64) - want.astype(np.int64))
    print(f"shim against the native call: {int((diff != 0).sum())} of {diff.size} values differ, largest {int(diff.max())} LSB")
    assert diff.max() <= 1 and (diff != 0).mean() <= 0.01
    red = draw_perspective_fields(img, np.array(up), rad.cuda(), color=(1, 0, 0), density=5, arrow_inv_len=10)
    assert red.shape == img.shape and (red[..., 0] == 255).any() and not np.array_equal(red, got)
    cam = draw_from_r_p_f_cx_cy(img, 8.0, 20.0, 60.0, 0.0, 0.0, "deg", up_color=(0, 1, 0))
    assert cam.dtype == np.uint8 and cam.shape == img.shape
    d2 = np.abs(cam.astype(np.int64) - want.astype(np.int64))   # the device's float32 fields against the oracle's: the same picture up to its roundings
    assert d2.max() <= 2 and (d2 != 0).mean() <= 0.05
    assert np.array_equal(draw_from_r_p_f_cx_cy(img, np.radians(8.0), np.radians(20.0), np.radians(60.0), 0.0, 0.0, mode="rad"), cam)
