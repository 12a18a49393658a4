"""fp64 statement of the supersampled gathers (include/pf_hip.h pf_pano_crop_ss / pf_reproject_ss / pf_pano_rotate_ss), built
only from the references of tests/test_reproject_ref.py, tests/test_pano_crop_ref.py and tests/test_pano_rotate_ref.py: sub-sample (i, j) of pixel
(row, col) at samples = S is the pixel centre (S row + i, S col + j) of the same call at (S H, S W), so the reference is the existing one at the
fine size, block-averaged over the valid samples.  Here too: which pixels are left out of accuracy comparisons and how few they are, known answers
of the reference, its effect on an aliasing source, the allowed error of the float32 images, the fixed inputs of tests/test_gpu_gather_samples.py,
and the host-side contract (no GPU needed).

Left out (ambiguous) is a pixel one of whose sub-samples lies within a margin of a discontinuity where fp32 and fp64 may disagree.  For the
re-projection the margins are a tenth of test_reproject_ref.clear's -- 1e-5 of the destination's no-ray circle, 1e-4 of z_min, 1e-3 px of the source
border, still 5 x the 4 x fp32 floor (5e-5 px) that the map is held to -- because with clear's own margins a pixel of S x S sub-samples is left out
S x S times as often (2.7 % of an image at S = 4).  For the crop it is the no-ray margin of tests/test_gpu_pano_crop.py per sub-sample.  At most
1 % of an image is left out (asserted here for every camera used)."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

from tests import test_pano_crop_ref as crop_ref
from tests import test_pano_rotate_ref as rot_ref
from tests import test_reproject_ref as rep_ref
from tests.test_gpu_pano_crop import clear_of_the_no_ray_circle
from tests.test_reproject_ref import CASES, SIZES, FakeCuda, theta_rad

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAMPLES = (2, 3, 4)


# ---------------------------------------------------------------- block means
def blocks(fine, S):
    """(S H, S W, ...) -> (H, W, S S, ...): the sub-samples of every pixel, i-major then j"""
    H, W = fine.shape[0] // S, fine.shape[1] // S
    b = fine.reshape((H, S, W, S) + fine.shape[2:])
    return np.moveaxis(b, 2, 1).reshape((H, W, S * S) + fine.shape[2:])


def block_mean(fine, valid, S, empty=0.0):
    """the mean over the valid sub-samples of every pixel, `empty` without one: (image (H, W, C), count (H, W))"""
    v = blocks(valid, S)
    n = v.sum(-1)
    s = (blocks(fine, S) * v[..., None]).sum(2)
    return np.where((n > 0)[..., None], s / np.maximum(n, 1)[..., None], float(empty)), n


def block_any(flag, S):
    return blocks(flag, S).any(-1)


# ---------------------------------------------------------------- the re-projection
def reproject_near(src, Hs, Ws, dst, H, W):
    """test_reproject_ref.clear's three tests with a tenth of its margins, negated: the pixels next to a discontinuity"""
    Xs, _, disc = rep_ref.source_rays(src, dst, H, W)
    a, b, _ = rep_ref.source_coords(src, Hs, Ws, dst, H, W)
    with np.errstate(invalid="ignore"):
        near = np.abs(disc) <= 1e-5
        near |= np.abs(Xs[..., 2] - rep_ref.z_min(src[6])) <= 1e-4
        for c, n in ((a, Ws), (b, Hs)):
            near |= (np.abs(c) <= 1e-3) | (np.abs(c - n) <= 1e-3)
    return near


@functools.lru_cache(None)
def reproject_reference(size, S):
    """per case of CASES at one size: (a, b, inside) of the fine grid (S H, S W) and the (H, W) mask of the pixels that are clear; read only"""
    Hs, Ws, H, W = size
    out = []
    for s, d in CASES:
        s, d = theta_rad(*s), theta_rad(*d)
        a, b, inside = rep_ref.source_coords(s, Hs, Ws, d, S * H, S * W)
        out.append((a, b, inside, ~block_any(reproject_near(s, Hs, Ws, d, S * H, S * W), S)))
    return out


def reproject_image(src_img, a, b, inside, S, fill=0.0):
    """(image (H, W, 3) in fp64 before any rounding, count of valid sub-samples (H, W))"""
    return block_mean(rep_ref.sample(src_img, a, b, inside, 0.0), inside, S, fill)


@functools.lru_cache(None)
def reproject_floor(size, S):
    """the error in px of the numpy-float32 evaluation of the source coordinates at the fine size, over CASES, on pixels inside the source"""
    Hs, Ws, H, W = size
    return float(rep_ref.fp32_floor((Hs, Ws, S * H, S * W))[0])


# ---------------------------------------------------------------- the crop
CROP_PANO = (64, 128)
CROP_SIZES = [(40, 56), (37, 53)]   # vector stores, scalar stores
CROP_CASES = [(0.0, 0.0, 0.0, 0.6, 0.0, 0.0, 0.0), (20.0, -40.0, 179.9, 0.35, 0.05, 0.02, 0.0), (-10.0, 85.0, -120.0, 0.9, 0.0, 0.0, 0.5),
              (5.0, 10.0, 180.0, 0.3, 0.0, 0.0, 1.2), (0.0, -88.0, 30.0, 0.25, -0.1, 0.1, 0.8)]   # tests/test_gpu_pano_crop.py's uint8 cameras; xi = 1.2 > 1


def crop_parts(th, H, W, S, Hp, Wp):
    """(u, v, has_ray) of the fine grid and the (H, W) mask of the clear pixels"""
    u, v, _, ok = crop_ref.sample_coords(th, S * H, S * W, Hp, Wp)
    return u, v, ok, ~block_any(~clear_of_the_no_ray_circle(th, S * H, S * W), S)


def crop_image(pano, th, H, W, S):
    u, v, ok, _ = crop_parts(th, H, W, S, pano.shape[0], pano.shape[1])
    return block_mean(crop_ref.bilinear(pano, u, v), ok, S, 0.0)


def crop_coords_f32(th, H, W, Hp, Wp):
    """pf_pano_crop's sampling coordinates with every step in numpy float32, in the order of pano_crop.hip: (u, v) float32, NaN without a ray"""
    f = np.float32
    r, p, yaw, fo, cx, cy, xi = [f(x) for x in th]
    sr, cr, sp, cp = np.sin(r), np.cos(r), np.sin(p), np.cos(p)
    R = np.array([[cr, -sr, f(0)], [cp * sr, cp * cr, -sp], [sp * sr, sp * cr, cp]], dtype=f)
    inv_f = f(1) / (fo * f(H))
    x = (np.arange(W, dtype=f)[None, :] + f(0.5) - (cx + f(0.5)) * f(W)) * inv_f + np.zeros((H, 1), f)
    y = (np.arange(H, dtype=f)[:, None] + f(0.5) - (cy + f(0.5)) * f(H)) * inv_f + np.zeros((1, W), f)
    r2 = x * x + y * y
    disc = f(1) + (f(1) - xi * xi) * r2
    with np.errstate(invalid="ignore"):
        eta = (xi + np.sqrt(np.where(disc >= 0, disc, f(np.nan)))) / (f(1) + r2)
    Xw = np.stack([eta * x, eta * y, eta - xi], -1) @ R.T
    t = yaw * f(1 / (2 * np.pi)) + f(0.5) + np.arctan2(Xw[..., 0], Xw[..., 2]) * f(1 / (2 * np.pi))
    t = t - np.floor(t)
    u = t * f(Wp) - f(0.5)
    v = (f(0.5) + np.arctan2(Xw[..., 1], np.sqrt(Xw[..., 0] * Xw[..., 0] + Xw[..., 2] * Xw[..., 2])) * f(1 / np.pi)) * f(Hp) - f(0.5)
    assert u.dtype == f and v.dtype == f
    return u, v


def crop_bound(pano, th, H, W, S):
    """allowed error per pixel of the float32 crop: the largest, over the pixel's sub-samples, of 2 x (coordinate floor x local gradient) + 1e-6
    (DESIGN.md section 17's rule in section 23's form: the floor of u is taken on the sphere, x cos lat, as test_pano_rotate_ref.fp32_floor says
    why), the floor being the error of the float32 evaluation at the fine size on the sub-samples that have a ray and are clear"""
    Hp, Wp = pano.shape[:2]
    u, v, Xw, ok = crop_ref.sample_coords(th, S * H, S * W, Hp, Wp)
    use = ok & clear_of_the_no_ray_circle(th, S * H, S * W)
    u32, v32 = crop_coords_f32(th, S * H, S * W, Hp, Wp)
    cos_lat = np.hypot(Xw[..., 0], Xw[..., 2])   # of a unit ray
    e_u = float((np.abs(rot_ref.wrap_px(u32 - u, Wp)) * cos_lat)[use].max())
    e_v = float(np.abs(v32 - v)[use].max())
    gu, gv = rot_ref.local_steps(pano, np.where(use, u, 0.0), np.where(use, v, 0.0))
    with np.errstate(divide="ignore", invalid="ignore"):
        per_sample = 2.0 * (np.minimum(e_u / cos_lat, Wp / 2) * gu + e_v * gv) + 1e-6
    return blocks(np.where(use, per_sample, 0.0), S).max(-1), (e_u, e_v)


# ---------------------------------------------------------------- the rotation
ROT_SOURCE = rot_ref.SOURCES[1]                                             # 40 x 80
ROT_OUTPUTS = [(16, 32), (37, 75)] + rot_ref.EDGE_OUTPUTS                   # a minification with vector stores, scalar stores, one row, one column
ROT_CASES = [(rot, inv) for rot in rot_ref.ROTATIONS[:2] for inv in (False, True)]   # (20, 35, 50) and pitch 90


def rotate_image(src, th, inverse, H, W, S):
    fine = rot_ref.rotate_image(src, th, inverse, S * H, S * W)
    return block_mean(fine, np.ones(fine.shape[:2], bool), S, 0.0)[0]


def rotate_bound(src, th, inverse, H, W, S):
    """allowed error per pixel of the float32 rotation: the largest of test_pano_rotate_ref.image_bound at the fine size over the pixel's sub-samples"""
    return blocks(rot_ref.image_bound(src, th, inverse, S * H, S * W), S).max(-1)


def on_the_axis(th, inverse, H, W, S):
    """pixels with a sub-sample that looks along the source's axis: it has no longitude (tests/test_gpu_pano_rotate.py's uint8 test)"""
    X = rot_ref.pano_directions(S * H, S * W) @ rot_ref.rot_matrix(th, inverse).T
    return block_any(np.hypot(X[..., 0], X[..., 2]) < 1e-6, S)


# ---------------------------------------------------------------- the aliasing pair: a source of period 2 texels, minified 4 x
ALIAS = dict(src=dict(roll=0.0, pitch=0.0, rel_focal=0.5), dst=dict(roll=10.0, pitch=0.0, rel_focal=0.47), Hs=96, Ws=128, H=24, W=32)


def checkerboard(Hs, Ws):
    r, c = np.meshgrid(np.arange(Hs), np.arange(Ws), indexing="ij")
    return np.repeat((((r + c) % 2) * 1.0)[..., None], 3, -1).astype(np.float32)


def alias_reference(S):
    A = ALIAS
    s = theta_rad(0.0, 0.0, 0.0, 0.5, 0.0, 0.0, 0.0)
    d = theta_rad(10.0, 0.0, 0.0, 0.47, 0.0, 0.0, 0.0)
    a, b, inside = rep_ref.source_coords(s, A["Hs"], A["Ws"], d, S * A["H"], S * A["W"])
    img, n = reproject_image(checkerboard(A["Hs"], A["Ws"]), a, b, inside, S)
    return img, n == S * S


# ---------------------------------------------------------------- the reference against itself
def test_block_mean_counts_the_valid_samples_only():
    fine = np.arange(4 * 6 * 3, dtype=np.float64).reshape(4, 6, 3)
    valid = np.ones((4, 6), bool)
    valid[0, 0] = valid[1, 1] = False
    valid[2:, 4:] = False
    img, n = block_mean(fine, valid, 2, empty=-1.0)
    assert n.tolist() == [[2, 4, 4], [4, 4, 0]]
    assert np.allclose(img[0, 0], (fine[0, 1] + fine[1, 0]) / 2) and np.allclose(img[1, 1], fine[2:4, 2:4].mean((0, 1))) and (img[1, 2] == -1.0).all()
    assert blocks(fine, 2)[0, 1, :, 0].tolist() == [fine[0, 2, 0], fine[0, 3, 0], fine[1, 2, 0], fine[1, 3, 0]]   # i-major, then j


@pytest.mark.parametrize("S", SAMPLES)
@pytest.mark.parametrize("size", SIZES)
def test_reproject_left_out_share_is_small_and_validity_is_mixed(size, S):
    worst, mixed = 0.0, 0.0
    for (s, d), (_, _, inside, cl) in zip(CASES, reproject_reference(size, S)):
        share = (~cl).mean()
        assert share <= 0.01, (s, d, share)
        n = blocks(inside, S).sum(-1)
        worst, mixed = max(worst, share), max(mixed, ((n > 0) & (n < S * S)).mean())
    print(f"re-projection at {size}, S = {S}: at most {100 * worst:.2f} % of an image left out, up to {100 * mixed:.1f} % of the pixels of mixed validity")
    assert mixed >= 0.01   # the mean over the valid sub-samples is exercised


@pytest.mark.parametrize("S", SAMPLES)
def test_crop_left_out_share_is_small(S):
    some_without_a_ray = False
    for H, W in CROP_SIZES:
        for c in CROP_CASES:
            th = theta_rad(*c)
            _, _, ok, cl = crop_parts(th, H, W, S, *CROP_PANO)
            assert (~cl).mean() <= 0.01 and ok.any(), (c, H, W, (~cl).mean())
            n = blocks(ok, S).sum(-1)
            some_without_a_ray |= bool(((n > 0) & (n < S * S)).any())
    assert some_without_a_ray   # xi = 1.2: pixels on the no-ray circle have sub-samples on both sides


@pytest.mark.parametrize("S", SAMPLES)
def test_rotation_axis_pixels_are_at_most_one(S):
    for out in ROT_OUTPUTS:
        for rot, inv in ROT_CASES:
            n = int(on_the_axis(rot_ref.rot_rad(*rot), inv, *out, S).sum())
            assert n <= 1 and (n == 0 or rot == (0.0, 90.0, 0.0)), (out, rot, inv, n)


@pytest.mark.parametrize("S", SAMPLES)
def test_known_answer_rotation_by_nothing_is_the_box_mean(S):
    H, W = 8, 16
    src = np.random.default_rng(S).uniform(0, 1, (S * H, S * W, 3))
    box = src.reshape(H, S, W, S, 3).mean((1, 3))
    assert np.abs(rotate_image(src, (0.0, 0.0, 0.0), False, H, W, S) - box).max() <= 1e-9


KNOWN_CAM = (0.0, 0.0, 0.0, 0.7, 0.04, -0.03, 0.0)   # a pinhole camera with roll = pitch = 0: the same relative parameters at both sizes


@pytest.mark.parametrize("S", SAMPLES)
def test_known_answer_reprojection_to_a_smaller_size_is_the_box_mean(S):
    H, W = 9, 13
    src = np.random.default_rng(10 + S).uniform(0, 1, (S * H, S * W, 3))
    th = theta_rad(*KNOWN_CAM)
    a, b, inside = rep_ref.source_coords(th, S * H, S * W, th, S * H, S * W)
    img, n = reproject_image(src, a, b, inside, S)
    assert (n == S * S).all()
    assert np.abs(img - src.reshape(H, S, W, S, 3).mean((1, 3))).max() <= 1e-9


def test_supersampling_takes_the_aliasing_out():
    one, full1 = alias_reference(1)
    four, full4 = alias_reference(4)
    use = full1 & full4
    s1, s4 = one[use].std(), four[use].std()
    print(f"a checkerboard of period 2 texels, minified 4 x: standard deviation {s1:.4f} at S = 1, {s4:.4f} at S = 4")
    assert use.mean() >= 0.5 and s1 >= 0.1 and s4 < 0.5 * s1   # most of the image (the rolled corners see nothing); a moire of a tenth of the range; halved at least


def test_crop_float32_floor_is_small():
    """the float32 evaluation of the crop's coordinates is close to fp64: a looser floor would make the GPU check empty"""
    pano = rot_ref.direction_panorama(*CROP_PANO)
    for c in CROP_CASES:
        _, (e_u, e_v) = crop_bound(pano, theta_rad(*c), *CROP_SIZES[0], 2)
        assert e_u <= 2e-4 and e_v <= 1e-4, (c, e_u, e_v)


# ---------------------------------------------------------------- host-side contract (fails before the feature exists)
CAM = dict(roll=0.0, pitch=0.0, rel_focal=1.0)
BAD_SAMPLES = (0, 5, -1, 2.0, "2", None, True)


def test_bad_samples_raise_before_the_library_is_loaded(monkeypatch):
    from perspectivefields_amd import PerspectiveFields, engine
    from perspectivefields_amd import perspectivefields as pfm

    def no_library(*a, **k):
        raise AssertionError("the library was loaded before the arguments were checked")

    monkeypatch.setattr(engine, "load_library", no_library)
    monkeypatch.setattr(pfm.torch, "is_tensor", lambda v: isinstance(v, (torch.Tensor, FakeCuda)))
    ok = FakeCuda((8, 16, 3))
    full = dict(pred_roll=1.0, pred_pitch=2.0, pred_rel_focal=0.8)
    for bad in BAD_SAMPLES:
        with pytest.raises(ValueError, match="samples"):
            pfm.crop_panorama(ok, 0.0, 0.0, 1.0, height=4, width=4, samples=bad)
        with pytest.raises(ValueError, match="samples"):
            pfm.reproject_image(ok, CAM, CAM, samples=bad)
        with pytest.raises(ValueError, match="samples"):
            pfm.rotate_panorama(ok, 1.0, 2.0, samples=bad)
        with pytest.raises(ValueError, match="samples"):
            PerspectiveFields.rectify(None, ok, full, samples=bad)   # rectify forwards its keywords
        with pytest.raises(ValueError, match="samples"):
            PerspectiveFields.level_panorama(None, ok, samples=bad)
    assert pfm.GATHER_MAX_SAMPLES == 4


def test_header_and_signatures_declare_the_three_entry_points():
    from perspectivefields_amd.engine import _SIGNATURES, declared_symbols, load_library

    hdr = open(os.path.join(ROOT, "include", "pf_hip.h")).read()
    assert "#define PF_GATHER_MAX_SAMPLES 4" in hdr
    for name, parent in (("pf_pano_crop_ss", "pf_pano_crop"), ("pf_reproject_ss", "pf_reproject"), ("pf_pano_rotate_ss", "pf_pano_rotate")):
        assert f"int {name}(int device, " in hdr and name in declared_symbols()
        decl = hdr[hdr.index(f"int {name}(int device, "):]
        assert decl[:decl.index(";")].rstrip().endswith("int samples, void* stream)")
        res, args = _SIGNATURES[name]
        pres, pargs = _SIGNATURES[parent]
        assert res is ctypes.c_int and args == pargs[:-1] + [ctypes.c_int, ctypes.c_void_p]
    kh = open(os.path.join(ROOT, "perspectivefields_amd", "csrc", "pf_kernels.h")).read()
    for name in ("PanoSsBatch", "ReprojSsBatch", "PanoRotSsBatch"):
        assert f"struct {name}" in kh and f"offsetof({name}, src) == 32" in kh
    lib = load_library()
    assert all(hasattr(lib, n) for n in ("pf_pano_crop_ss", "pf_reproject_ss", "pf_pano_rotate_ss"))


def test_ss_entry_points_reject_bad_arguments_before_device_work():
    from perspectivefields_amd.engine import load_library

    lib = load_library()
    one = (ctypes.c_void_p * 1)(0x1000)
    ints = lambda *s: (ctypes.c_int32 * len(s))(*s)
    dev = ctypes.c_void_p(256)

    def crop(samples=2, H=4, img=dev, up=None):
        return lib.pf_pano_crop_ss(0, 1, one, ints(8, 16), 0, 1, ints(0), dev, H, 4, img, up, None, samples, None)

    def reproject(samples=2, H=4, img=dev, up=None):
        return lib.pf_reproject_ss(0, 1, one, ints(8, 16), 0, 1, ints(0), dev, dev, H, 4, 0.0, img, None, None, samples, None)

    def rotate(samples=2, H=4, img=dev, up=None):
        return lib.pf_pano_rotate_ss(0, 1, one, ints(8, 16), 0, 1, ints(0), dev, 0, H, 8, img, up, None, samples, None)

    for name, call in (("pf_pano_crop_ss", crop), ("pf_reproject_ss", reproject), ("pf_pano_rotate_ss", rotate)):
        for bad in (0, 5, -3):
            rc, msg = call(samples=bad), lib.pf_last_error(None).decode()
            assert rc == -1 and msg.startswith(name + ": ") and "samples" in msg, (name, bad, rc, msg)
        # samples is looked at first, and the parent's checks follow under the new name
        rc, msg = call(samples=0, img=None), lib.pf_last_error(None).decode()
        assert rc == -1 and "samples" in msg
        for kw, what in ((dict(H=0), "size"), (dict(img=None), "required")) + (() if name == "pf_reproject_ss" else ((dict(up=dev), "both"),)):
            rc, msg = call(**kw), lib.pf_last_error(None).decode()
            assert rc == -1 and what in msg and msg.startswith(name + ": "), (name, kw, rc, msg)
        if not torch.cuda.is_available():   # good arguments fail on the missing device only
            for S in (1, 4):
                rc, msg = call(samples=S), lib.pf_last_error(None).decode()
                assert rc == -2 and "no HIP device" in msg, (name, rc, msg)


def test_ss_kernels_are_in_the_library_without_scratch():
    """scripts/kernel_resources.py on the built library: every instantiation is there for gfx950 with no spilled register and no scratch"""
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
    for kernel, lds in (("pano_crop_ss_kernel", 132), ("reproject_ss_kernel", 72), ("pano_rotate_ss_kernel", 60)):   # the parents' constants in LDS
        for t in ("unsigned char", "float"):
            for flag in ("false", "true"):
                r = by[f"pf::{kernel}<{t}, {flag}>"]
                assert r["spill"] == 0 and r["scratch"] == 0 and r["lds"] <= lds and r["vgpr"] <= 128, r
