"""Composition of camera views into equirectangular panoramas on the GPU (include/pf_hip.h pf_pano_compose, perspectivefields_amd.compose_panorama,
PerspectiveFields.compose_panorama) against the fp64 reference of tests/test_pano_compose_ref.py: the summed weight, float32 and uint8
composites, MEAN with one view, closure with the panorama crop, batch invariance with the carry over more than 32 views, non-finite
parameters, the vector and scalar store paths, edge sizes, and the model method.

Tolerances.  The summed feather weight S is held to 4 x the error of the same formulas evaluated in numpy float32 in the same run
(test_pano_compose_ref.fp32_floor; the device's sincosf / sqrtf / division differ from numpy's).  The float32 composite is held, per pixel, to
test_pano_compose_ref.image_bound: (covering views) x (coordinate error of that floor) x (largest analytic gradient of a source per px) x 2
+ (covering views) x (weight error of that floor) x (value range) / S_ref + 1e-6; pixels with 0 < S_ref < 1e-3 would be left out and the
fixed inputs have none (asserted on the CPU).  The uint8 composite is held to 1 LSB of the fp64 value before rounding.  With one view and
MEAN, pixels within 1e-2 px of the view's border or 1e-3 of z_min are left out (at most 0.35 %, asserted <= 1 % on the CPU)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests.test_gpu_pano_crop import direction_panorama
from tests.test_gpu_reproject import GRAD, KEYS, analytic_image
from tests.test_pano_compose_ref import (EDGE_PANOS, FEATHER, MEAN, PANOS, SINGLE_VIEWS, VIEWS, compose, fp32_floor, image_bound, near_a_border, pano_directions,
                                         theta_rad, views_rad)
from tests.test_pano_crop_ref import crop_image

pytestmark = pytest.mark.gpu


def cam_dict(views):
    c = np.asarray([th for th, _ in views], dtype=np.float64)
    return {k: c[:, i] for i, k in enumerate(KEYS)}


def thetas(views):
    return [theta_rad(*th) for th, _ in views]


@functools.lru_cache(None)
def sources(kind):
    """the seven views' images as numpy: "analytic" float32 in [0, 1], "random" uint8; computed once, read only"""
    rng = np.random.default_rng(31)
    return tuple(analytic_image(Hs, Ws) if kind == "analytic" else rng.integers(0, 256, (Hs, Ws, 3), dtype=np.uint8) for _, (Hs, Ws) in VIEWS)


def on_gpu(images):
    return [torch.from_numpy(np.ascontiguousarray(im)).cuda() for im in images]


@functools.lru_cache(None)
def floor_of(size):
    return fp32_floor(views_rad(), *size)


@functools.lru_cache(None)
def reference(size, kind, blend=FEATHER):
    return compose(sources(kind), thetas(VIEWS), *size, blend)


@functools.lru_cache(None)
def gpu_float_run(size):
    from perspectivefields_amd import compose_panorama

    pano, weight = compose_panorama(on_gpu(sources("analytic")), cam_dict(VIEWS), height=size[0], width=size[1], return_weight=True)
    assert pano.shape == (1, *size, 3) and pano.dtype == torch.float32 and weight.shape == (1, *size) and weight.dtype == torch.float32
    return pano[0].cpu().numpy(), weight[0].cpu().numpy()


def check_float_image(got, ref, S_ref, n_ref, floor, what):
    use = ~((S_ref > 0) & (S_ref < 1e-3))
    err = np.abs(got.astype(np.float64) - ref).max(-1)
    bound = image_bound(np.maximum(n_ref, 1), S_ref, floor[1], floor[2], GRAD)
    k = np.argmax(np.where(use, err / bound, 0))
    print(f"{what}: largest error {err[use].max():.3e}; worst pixel error {err.flat[k]:.3e} of allowed {bound.flat[k]:.3e} (S {S_ref.flat[k]:.3f}, {n_ref.flat[k]} views)")
    assert (err <= bound)[use].all(), (what, err.flat[k], bound.flat[k])


@pytest.mark.parametrize("size", PANOS)
def test_feather_weight_matches_the_fp64_reference(size):
    _, S = gpu_float_run(size)
    _, S_ref, _ = reference(size, "analytic")
    e, floor = np.abs(S.astype(np.float64) - S_ref).max(), floor_of(size)
    print(f"summed weight at {size}: GPU error {e:.3e}, fp32 floor {floor[0]:.3e}")
    assert e <= 4 * floor[0], (e, floor)
    assert (S > 0).all()


@pytest.mark.parametrize("size", PANOS)
def test_float32_image_of_analytic_sources(size):
    img, _ = gpu_float_run(size)
    ref, S_ref, n_ref = reference(size, "analytic")
    check_float_image(img, ref, S_ref, n_ref, floor_of(size), f"float32 composite at {size}")


@pytest.mark.parametrize("size", PANOS)
def test_uint8_feather_within_one_lsb(size):
    from perspectivefields_amd import compose_panorama

    pano = compose_panorama(on_gpu(sources("random")), cam_dict(VIEWS), height=size[0], width=size[1])
    assert torch.is_tensor(pano) and pano.dtype == torch.uint8 and pano.shape == (1, *size, 3)
    ref, _, _ = reference(size, "random")
    e = np.abs(pano[0].cpu().numpy().astype(np.float64) - ref).max()
    print(f"uint8 composite at {size}: largest distance to the fp64 value {e:.4f} LSB")
    assert e <= 1.0


@pytest.mark.parametrize("size", PANOS)
@pytest.mark.parametrize("k", SINGLE_VIEWS)
def test_mean_with_one_view(size, k):
    from perspectivefields_amd import compose_panorama

    th, (Hs, Ws) = VIEWS[k]
    src = sources("analytic")[k]
    ref, S_ref, n_ref = compose([src], [theta_rad(*th)], *size, MEAN)
    cl = ~near_a_border(theta_rad(*th), Hs, Ws, pano_directions(*size))
    floor = fp32_floor([(theta_rad(*th), Hs, Ws)], *size)
    for fill in (0.0, 0.5):
        pano, weight = compose_panorama(on_gpu([src]), cam_dict([VIEWS[k]]), height=size[0], width=size[1], blend="mean", fill=fill, return_weight=True)
        pano, weight = pano[0].cpu().numpy(), weight[0].cpu().numpy()
        assert set(np.unique(weight)) <= {0.0, 1.0}
        assert np.array_equal(weight[cl], S_ref[cl].astype(np.float32)), (k, size)
        assert (pano[weight == 0] == np.float32(fill)).all() and (weight[cl & (n_ref == 0)] == 0).all()
        m = cl & (n_ref == 1)
        assert m.any() and (cl & (n_ref == 0)).any()
        err = np.abs(pano.astype(np.float64) - ref).max(-1)
        bound = float(image_bound(1, 1.0, 0.0, floor[2], GRAD))
        print(f"MEAN of view {k} at {size}, fill {fill}: largest error {err[m].max():.3e}, allowed {bound:.3e}")
        assert err[m].max() <= bound


def smooth_of_direction(D):
    """a smooth function of the direction with values in [-1, 1] per channel: the direction itself"""
    return D


def test_closure_with_the_panorama_crop():
    """a panorama of a smooth function of direction, cropped to six views on the GPU and composed again, against the function at the
    panorama pixels' directions: no worse than the same chain in fp64 (two bilinear samplings) plus 1e-5 of the value range"""
    from perspectivefields_amd import compose_panorama, crop_panorama

    Hp, Wp, H, W = 32, 64, 48, 48
    pano = smooth_of_direction(direction_panorama(64, 128)).astype(np.float32)
    f = 0.5 / np.tan(np.radians(50.0))
    faces = [((0.0, 0.0, yaw, f, 0.0, 0.0, 0.0), (H, W)) for yaw in (0.0, 90.0, 180.0, 270.0)] + [((0.0, p, 0.0, f, 0.0, 0.0, 0.0), (H, W)) for p in (90.0, -90.0)]
    c = cam_dict(faces)
    crops, _, _ = crop_panorama(torch.from_numpy(pano).cuda(), c["roll"], c["pitch"], c["rel_focal"], yaw=c["yaw"], height=H, width=W, fields=False)
    out, weight = compose_panorama(crops, c, height=Hp, width=Wp, return_weight=True)
    assert (weight > 0).all()
    truth = smooth_of_direction(pano_directions(Hp, Wp))
    ref, _, _ = compose([crop_image(pano, th, H, W) for th in thetas(faces)], thetas(faces), Hp, Wp)
    e_gpu, e_ref = np.abs(out[0].cpu().numpy().astype(np.float64) - truth).max(), np.abs(ref - truth).max()
    print(f"closure crop -> compose: GPU error {e_gpu:.6f}, fp64 reference chain {e_ref:.6f} (value range 2)")
    assert e_gpu <= e_ref + 1e-5 * 2.0


def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


@pytest.mark.parametrize("dtype", [torch.uint8, torch.float32])
def test_batching_carry_and_determinism(dtype):
    """panoramas of 1, 3, 0 and 33 views in one call: each has the bits of its composition alone, on every run and for every call order of
    the views that keeps the order within a panorama; the 33 views (one more than a launch holds) travel through the accumulator, and
    their composite is also held to the reference, which a wrong carry misses by far"""
    from perspectivefields_amd import compose_panorama

    rng = np.random.default_rng(41)
    Hp, Wp = 20, 36
    few = [VIEWS[0], VIEWS[1], VIEWS[4], VIEWS[6]]
    many = [((float(rng.uniform(-20, 20)), float(rng.uniform(-80, 80)), float(rng.uniform(-180, 180)), 0.45, 0.0, 0.0, (0.0, 0.5)[i % 2]), (16, 16)) for i in range(33)]
    views = few + many
    index = [0, 1, 1, 1] + [3] * 33
    imgs = [rng.integers(0, 256, (Hs, Ws, 3), dtype=np.uint8) for _, (Hs, Ws) in views]
    if dtype == torch.float32:
        imgs = [(im / 255.0).astype(np.float32) for im in imgs]
    dev = on_gpu(imgs)
    run = lambda order, **kw: compose_panorama([dev[i] for i in order], cam_dict([views[i] for i in order]), height=Hp, width=Wp, fill=3, return_weight=True, **kw)
    every = list(range(len(views)))
    first = run(every, pano_index=index, n_pano=4)
    assert first[0].shape == (4, Hp, Wp, 3) and first[1].shape == (4, Hp, Wp)
    again = run(every, pano_index=index, n_pano=4)
    mixed = [4, 0, 5, 1, 6, 7, 2, 8, 3] + list(range(9, 37))   # another call order, the same order within each panorama
    third = run(mixed, pano_index=[index[i] for i in mixed], n_pano=4)
    for other in (again, third):
        for a, b in zip(first, other):
            assert torch.equal(_bits(a), _bits(b))
    assert (first[0][2] == 3).all() and (first[1][2] == 0).all()   # the panorama without views
    for p in (0, 1, 3):
        own = [i for i in every if index[i] == p]
        alone = run(own)
        for a, b in zip(first, alone):
            assert torch.equal(_bits(a[p]), _bits(b[0])), p
    # the 33 views against the reference
    own = [i for i in every if index[i] == 3]
    ref, S_ref, n_ref = compose([imgs[i] for i in own], thetas([views[i] for i in own]), Hp, Wp, fill=3)
    got, S = first[0][3].cpu().numpy().astype(np.float64), first[1][3].cpu().numpy()
    floor = fp32_floor(views_rad([views[i] for i in own]), Hp, Wp)
    assert n_ref.max() > 4 and (S_ref > 0).any()
    assert np.abs(S - S_ref).max() <= 4 * floor[0], (np.abs(S - S_ref).max(), floor)
    use = (S_ref == 0) | (S_ref >= 1e-3)
    # random texels: the largest gradient is the value range per px; uint8: that bound in LSB and half an LSB for the rounding
    bound = image_bound(np.maximum(n_ref, 1), S_ref, floor[1], floor[2], 1.0)
    bound = 0.5 + 255.0 * bound if dtype == torch.uint8 else bound
    err = np.abs(got - ref).max(-1)
    print(f"33 views, {dtype}: largest error {err[use].max():.3e}, largest error / allowed {(err / bound)[use].max():.3f}, S error {np.abs(S - S_ref).max():.3e} (floor {floor[0]:.3e})")
    assert (err <= bound)[use].all()


@pytest.mark.parametrize("key", ["rel_focal", "roll", "pitch"])
def test_non_finite_parameters_drop_their_view_only(key):
    from perspectivefields_amd import compose_panorama

    dev = on_gpu(sources("random"))
    good = compose_panorama(dev[:2] + dev[3:], cam_dict(VIEWS[:2] + VIEWS[3:]), height=37, width=75, return_weight=True)
    c = cam_dict(VIEWS)
    c[key] = c[key].copy()
    c[key][2] = np.nan
    got = compose_panorama(dev, c, height=37, width=75, return_weight=True)
    for a, b in zip(good, got):
        assert torch.equal(_bits(a), _bits(b))


def _raw_call(srcs, cam, Hp, Wp, blend, pano_ptr, weight_ptr):
    from perspectivefields_amd.engine import _check, load_library

    n = len(srcs)
    hw = (ctypes.c_int32 * (2 * n))(*[int(s) for p in srcs for s in p.shape[:2]])
    _check(load_library().pf_pano_compose(0, n, (ctypes.c_void_p * n)(*[p.data_ptr() for p in srcs]), hw, 0 if srcs[0].dtype == torch.uint8 else 1,
                                          (ctypes.c_int32 * n)(*([0] * n)), cam.data_ptr(), 1, Hp, Wp, blend, 0.0, pano_ptr, weight_ptr, None,
                                          ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), None, "pf_pano_compose")


@pytest.mark.parametrize("dtype", [torch.uint8, torch.float32])
def test_unaligned_outputs_take_the_scalar_stores_and_give_the_same_bits(dtype):
    """compose_panorama allocates its outputs itself, always aligned; storage that is not aligned reaches pf_pano_compose only through the C
    interface, called here directly: 32 x 64 into aligned outputs (vector stores) against the same call into buffers shifted by one element"""
    from perspectivefields_amd import compose_panorama

    Hp, Wp = PANOS[0]
    dev = [p.to(dtype) for p in on_gpu(sources("random"))]
    pano, weight = compose_panorama(dev, cam_dict(VIEWS), height=Hp, width=Wp, return_weight=True)
    c = cam_dict(VIEWS)
    cam = torch.from_numpy(np.stack([np.radians(c[k]) if k in KEYS[:3] else c[k] for k in KEYS], 1)).cuda().float().contiguous()
    n = Hp * Wp
    for shift_pano, shift_weight in ((1, 0), (0, 1), (1, 1)):
        pano2 = torch.zeros(n * 3 + 4, dtype=dtype, device="cuda")
        weight2 = torch.zeros(n + 4, dtype=torch.float32, device="cuda")
        p2, w2 = pano2[shift_pano:shift_pano + n * 3], weight2[shift_weight:shift_weight + n]
        _raw_call(dev, cam, Hp, Wp, 0, p2.data_ptr(), w2.data_ptr())
        assert (p2.data_ptr() % (4 if dtype == torch.uint8 else 16) != 0) == bool(shift_pano) and (w2.data_ptr() % 16 != 0) == bool(shift_weight)
        assert torch.equal(_bits(p2.reshape(pano.shape)), _bits(pano)) and torch.equal(_bits(w2.reshape(weight.shape)), _bits(weight))
        assert (pano2[:shift_pano] == 0).all() and (pano2[shift_pano + n * 3:] == 0).all()   # nothing written around the buffers
        assert (weight2[:shift_weight] == 0).all() and (weight2[shift_weight + n:] == 0).all()


@pytest.mark.parametrize("size", EDGE_PANOS)
def test_thin_and_tile_sized_panoramas(size):
    """one row, one column, exactly one tile, and one pixel row and one 4-pixel group past a tile; the fp32 floor of the 37 x 75 panorama bounds
    the weights here too (a view's error is set by its size and focal length, which are the same; a panorama's size only picks the directions)"""
    from perspectivefields_amd import compose_panorama

    floor = floor_of(PANOS[1])
    pano, weight = compose_panorama(on_gpu(sources("analytic")), cam_dict(VIEWS), height=size[0], width=size[1], return_weight=True)
    ref, S_ref, n_ref = reference(size, "analytic")
    assert np.abs(weight[0].cpu().numpy().astype(np.float64) - S_ref).max() <= 4 * floor[0]
    check_float_image(pano[0].cpu().numpy(), ref, S_ref, n_ref, floor, f"float32 composite at {size}")
    u8 = compose_panorama(on_gpu(sources("random")), cam_dict(VIEWS), height=size[0], width=size[1])
    assert np.abs(u8[0].cpu().numpy().astype(np.float64) - reference(size, "random")[0]).max() <= 1.0


def test_crop_infer_fit_compose_end_to_end():
    from perspectivefields_amd import PerspectiveFields, crop_panorama
    from perspectivefields_amd.engine import PfError

    pano = torch.from_numpy(np.random.default_rng(12).integers(0, 256, (256, 512, 3), dtype=np.uint8)).cuda()
    m = PerspectiveFields("Paramnet-360Cities-edina-centered", weights="synthetic:0").eval().cuda()
    B, H, W = 3, 120, 160
    yaw = [0.0, 120.0, -170.0]
    img, _, _ = crop_panorama(pano, [0.0, 10.0, -20.0], [5.0, -30.0, 40.0], [0.8, 1.1, 0.6], yaw=yaw, height=H, width=W, fields=False)
    preds = m.inference_batch(list(img))
    for p in (preds, m.fit_camera(preds), m.fit_camera(preds, distortion=True)):
        out, weight = m.compose_panorama(img, p, yaw=yaw, height=32, width=64, return_weight=True)
        assert out.shape == (1, 32, 64, 3) and out.dtype == torch.uint8 and out.device == img.device
        assert weight.shape == (1, 32, 64) and weight.dtype == torch.float32 and weight.device == img.device
    two = m.compose_panorama(list(img), preds, yaw=10.0, height=19, width=33, pano_index=[1, 0, 1], blend="mean")
    assert two.shape == (2, 19, 33, 3) and two.dtype == torch.uint8
    one = m.compose_panorama(img[0], preds[0], height=16, width=32)
    assert one.shape == (1, 16, 32, 3)
    fields_only = [{k: v for k, v in p.items() if k in ("pred_gravity_original", "pred_latitude_original")} for p in preds]
    with pytest.raises(PfError, match="fit_camera"):
        m.compose_panorama(img, fields_only, yaw=yaw, height=32, width=64)
