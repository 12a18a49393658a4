"""The supersampled gathers on the GPU (samples= of crop_panorama, reproject_image and rotate_panorama; include/pf_hip.h pf_pano_crop_ss /
pf_reproject_ss / pf_pano_rotate_ss) against the fp64 reference of tests/test_gather_samples_ref.py: accuracy, consistency with
the library's own samples = 1 run at S times the size, the bit identities (samples = 1, labels, map), the box-mean known answers, determinism and
isolation, the model methods, and the aliasing the feature is for.

Tolerances.  float32 image: 2 x (fp32 coordinate floor, measured in the same run by the numpy-float32 evaluation of the same formulas at the fine size
(S H, S W)) x (gradient) + 1e-6 per pixel, DESIGN.md section 17's and 23's rule: a mean of sub-samples each within that bound is within it.  uint8:
1 LSB of the fp64 mean before rounding.  Consistency with the library's own fine run: twice the float32 bound (both sides carry the error once).
Pixels that the reference leaves out as ambiguous (at most 0.45 % of an image, asserted <= 1 % there) are not compared."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests import test_gather_samples_ref as ss
from tests import test_pano_rotate_ref as rot_ref
from tests import test_reproject_ref as rep_ref
from tests.test_gather_samples_ref import ALIAS, CROP_CASES, CROP_PANO, CROP_SIZES, KNOWN_CAM, ROT_CASES, ROT_OUTPUTS, ROT_SOURCE, SAMPLES, block_mean, blocks
from tests.test_gpu_pano_crop import crop
from tests.test_gpu_reproject import GRAD, KEYS, analytic_image, cams
from tests.test_reproject_ref import CASES, SIZES, theta_rad

pytestmark = pytest.mark.gpu


def gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def same_bits(a, b):
    return all(torch.equal(_bits(x), _bits(y)) for x, y in zip(a, b))


def rotate(src, cases, out, S, fields=False):
    """[(rot degrees, inverse)] of one source: per case the tuple of numpy outputs of rotate_panorama"""
    from perspectivefields_amd import rotate_panorama

    res = []
    for rot, inv in cases:
        r = rotate_panorama(src, *rot, inverse=inv, height=out[0], width=out[1], fields=fields, samples=S)
        res.append(tuple(t[0].cpu().numpy() for t in (r if fields else (r,))))
    return res


# ---------------------------------------------------------------- accuracy against the fp64 reference
@functools.lru_cache(None)
def reproject_float_run(size, S, fill=0.5):
    from perspectivefields_amd import reproject_image

    Hs, Ws, H, W = size
    img, valid = reproject_image(gpu(analytic_image(Hs, Ws)), cams(CASES, 0), cams(CASES, 1), height=H, width=W, fill=fill, return_valid=True, samples=S)
    assert img.shape == (60, H, W, 3) and img.dtype == torch.float32 and valid.shape == (60, H, W) and valid.dtype == torch.bool
    return img.cpu().numpy(), valid.cpu().numpy()


@pytest.mark.parametrize("S", SAMPLES)
@pytest.mark.parametrize("size", SIZES)
def test_reproject_float32_image_and_mask(size, S):
    Hs, Ws, H, W = size
    img, valid = reproject_float_run(size, S)
    src = analytic_image(Hs, Ws)
    tol = 2 * ss.reproject_floor(size, S) * GRAD + 1e-6
    worst = 0.0
    for k, (a, b, inside, cl) in enumerate(ss.reproject_reference(size, S)):
        ref, n = ss.reproject_image(src, a, b, inside, S, fill=0.5)
        assert np.array_equal(valid[k][cl], (n > 0)[cl]), CASES[k]   # the mask: any sub-sample valid
        assert (img[k][~valid[k]] == np.float32(0.5)).all(), CASES[k]   # mask = 0 <=> fill
        worst = max(worst, np.abs(img[k].astype(np.float64) - ref)[cl].max())
    print(f"re-projection, float32, {size}, S = {S}: worst error {worst:.3e}, allowed {tol:.3e}, worst / allowed {worst / tol:.3f}")
    assert worst <= tol


@pytest.mark.parametrize("S", SAMPLES)
@pytest.mark.parametrize("size", SIZES)
def test_reproject_uint8_within_one_lsb(size, S):
    from perspectivefields_amd import reproject_image

    Hs, Ws, H, W = size
    src = np.random.default_rng(3).integers(0, 256, (Hs, Ws, 3), dtype=np.uint8)
    img = reproject_image(gpu(src), cams(CASES, 0), cams(CASES, 1), height=H, width=W, fill=9, samples=S)
    assert img.dtype == torch.uint8 and img.shape == (60, H, W, 3)
    img = img.cpu().numpy().astype(np.float64)
    worst = 0.0
    for k, (a, b, inside, cl) in enumerate(ss.reproject_reference(size, S)):
        ref, _ = ss.reproject_image(src, a, b, inside, S, fill=9.0)
        worst = max(worst, np.abs(img[k] - ref)[cl].max())
    print(f"re-projection, uint8, {size}, S = {S}: worst distance from the fp64 mean {worst:.4f} LSB")
    assert worst <= 1.0


@pytest.mark.parametrize("S", SAMPLES)
def test_crop_float32_and_uint8(S):
    pano_f = rot_ref.direction_panorama(*CROP_PANO)
    pano_u = np.random.default_rng(3).integers(0, 256, CROP_PANO + (3,), dtype=np.uint8)
    worst = [0.0, 0.0]
    for H, W in CROP_SIZES:
        img_f = crop(gpu(pano_f), CROP_CASES, H, W, fields=False, samples=S)[0].cpu().numpy().astype(np.float64)
        img_u = crop(gpu(pano_u), CROP_CASES, H, W, fields=False, samples=S)[0]
        assert img_u.dtype == torch.uint8
        img_u = img_u.cpu().numpy().astype(np.float64)
        for k, c in enumerate(CROP_CASES):
            th = theta_rad(*c)
            _, _, _, cl = ss.crop_parts(th, H, W, S, *CROP_PANO)
            ref, n = ss.crop_image(pano_f, th, H, W, S)
            bound, _ = ss.crop_bound(pano_f, th, H, W, S)
            err = np.abs(img_f[k] - ref).max(-1)
            use = cl & (n > 0)
            assert (err[use] <= bound[use]).all(), (c, H, W, (err[use] / bound[use]).max())
            assert not img_f[k][cl & (n == 0)].any() and not img_u[k][cl & (n == 0)].any(), c   # no valid sub-sample: 0
            d = np.abs(img_u[k] - ss.crop_image(pano_u, th, H, W, S)[0])[cl].max()
            assert d <= 1.0, (c, H, W, d)
            worst = [max(worst[0], (err[use] / bound[use]).max()), max(worst[1], d)]
    print(f"crop, S = {S}: float32 worst error / allowed {worst[0]:.3f}; uint8 worst distance from the fp64 mean {worst[1]:.4f} LSB")


@pytest.mark.parametrize("S", SAMPLES)
def test_rotate_float32_and_uint8(S):
    src_f = rot_ref.direction_panorama(*ROT_SOURCE)
    src_u = rot_ref.u8_panorama(*ROT_SOURCE)
    worst = [0.0, 0.0]
    for out in ROT_OUTPUTS:
        got_f = rotate(gpu(src_f), ROT_CASES, out, S)
        got_u = rotate(gpu(src_u), ROT_CASES, out, S)
        for (rot, inv), (img_f,), (img_u,) in zip(ROT_CASES, got_f, got_u):
            th = rot_ref.rot_rad(*rot)
            err = np.abs(img_f.astype(np.float64) - ss.rotate_image(src_f, th, inv, *out, S)).max(-1)
            bound = ss.rotate_bound(src_f, th, inv, *out, S)
            assert (err <= bound).all(), (out, rot, inv, (err / bound).max())
            axis = ss.on_the_axis(th, inv, *out, S)   # at most one pixel (asserted in the reference file): it has no longitude, in fp64 as little as in float32
            assert img_u.dtype == np.uint8
            d = np.abs(img_u.astype(np.float64) - ss.rotate_image(src_u, th, inv, *out, S))[~axis].max()
            assert d <= 1.0, (out, rot, inv, d)
            worst = [max(worst[0], (err / bound).max()), max(worst[1], d)]
    print(f"rotation, S = {S}: float32 worst error / allowed {worst[0]:.3f}; uint8 worst distance from the fp64 mean {worst[1]:.4f} LSB")


# ---------------------------------------------------------------- consistency with the library's own samples = 1 run at S times the size
@pytest.mark.parametrize("S", SAMPLES)
def test_samples_is_the_block_mean_of_the_fine_run(S):
    from perspectivefields_amd import reproject_image

    size = SIZES[0]
    Hs, Ws, H, W = size
    img, _ = reproject_float_run(size, S)
    fine, fvalid = reproject_image(gpu(analytic_image(Hs, Ws)), cams(CASES, 0), cams(CASES, 1), height=S * H, width=S * W, fill=0.5, return_valid=True)
    fine, fvalid = fine.cpu().numpy().astype(np.float64), fvalid.cpu().numpy()
    tol = 2 * (2 * ss.reproject_floor(size, S) * GRAD + 1e-6)
    worst = [0.0, 0.0, 0.0]
    for k, (_, _, _, cl) in enumerate(ss.reproject_reference(size, S)):
        mean, _ = block_mean(fine[k], fvalid[k], S, 0.5)
        worst[0] = max(worst[0], np.abs(img[k] - mean)[cl].max() / tol)
    assert worst[0] <= 1.0, worst

    H, W = CROP_SIZES[0]
    pano = rot_ref.direction_panorama(*CROP_PANO)
    img = crop(gpu(pano), CROP_CASES, H, W, fields=False, samples=S)[0].cpu().numpy().astype(np.float64)
    fine = crop(gpu(pano), CROP_CASES, S * H, S * W, fields=False)[0].cpu().numpy().astype(np.float64)
    for k, c in enumerate(CROP_CASES):
        th = theta_rad(*c)
        _, _, ok, cl = ss.crop_parts(th, H, W, S, *CROP_PANO)
        mean, n = block_mean(fine[k], ok, S)
        bound, _ = ss.crop_bound(pano, th, H, W, S)
        use = cl & (n > 0)
        worst[1] = max(worst[1], (np.abs(img[k] - mean).max(-1)[use] / (2 * bound[use])).max())
    assert worst[1] <= 1.0, worst

    out = ROT_OUTPUTS[0]
    src = rot_ref.direction_panorama(*ROT_SOURCE)
    got = rotate(gpu(src), ROT_CASES, out, S)
    fine = rotate(gpu(src), ROT_CASES, (S * out[0], S * out[1]), 1)
    for (rot, inv), (img,), (f,) in zip(ROT_CASES, got, fine):
        mean = blocks(f.astype(np.float64), S).mean(2)
        bound = ss.rotate_bound(src, rot_ref.rot_rad(*rot), inv, *out, S)
        worst[2] = max(worst[2], (np.abs(img - mean).max(-1) / (2 * bound)).max())
    print(f"S = {S} against the block mean of the library's own fine run, worst difference / allowed: re-projection {worst[0]:.3f}, crop {worst[1]:.3f}, "
          f"rotation {worst[2]:.3f}")
    assert worst[2] <= 1.0, worst


# ---------------------------------------------------------------- raw C calls
def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _raw(name, src, middle, outs, samples):
    """pf_<name> (samples None) or pf_<name>_ss with one source for every output; middle: the arguments between the index and the outputs"""
    from perspectivefields_amd.engine import _check, load_library

    B = middle[0].shape[0]
    fn = "pf_" + name + ("" if samples is None else "_ss")
    args = [0, 1, (ctypes.c_void_p * 1)(src.data_ptr()), (ctypes.c_int32 * 2)(int(src.shape[0]), int(src.shape[1])), 0 if src.dtype == torch.uint8 else 1, B,
            (ctypes.c_int32 * B)(*([0] * B))] + [m.data_ptr() if torch.is_tensor(m) else m for m in middle] + [None if o is None else o.data_ptr() for o in outs]
    _check(getattr(load_library(), fn)(*args, *(() if samples is None else (samples,)), _stream()), None, fn)


def raw_crop(pano, cam, H, W, outs, samples):
    _raw("pano_crop", pano, [cam, H, W], outs, samples)


def raw_reproject(src, cam_s, cam_d, H, W, fill, outs, samples):
    _raw("reproject", src, [cam_s, cam_d, H, W, ctypes.c_float(fill)], outs, samples)


def raw_rotate(pano, rot, inverse, H, W, outs, samples):
    _raw("pano_rotate", pano, [rot, inverse, H, W], outs, samples)


RAW_CROP = [(12.0, 20.0, 30.0, 0.6, 0.0, 0.0, 0.0), (-25.0, -40.0, -100.0, 0.9, 0.1, -0.08, 0.0), (8.0, 35.0, 170.0, 0.5, 0.0, 0.0, 0.8),
            (-15.0, -10.0, 60.0, 0.7, -0.05, 0.1, 0.8), (20.0, 5.0, -20.0, 0.3, 0.0, 0.0, 1.2)]   # tests/test_gpu_pano_crop.py's: both label forms, no-ray corners
RAW_PAIRS = CASES[:5]


def _crop_cam():
    return gpu(np.asarray([theta_rad(*c) for c in RAW_CROP])).float().contiguous()


def _pair_cams():
    return [gpu(np.stack([np.radians(cams(RAW_PAIRS, w)[k]) if k in KEYS[:3] else cams(RAW_PAIRS, w)[k] for k in KEYS], 1)).float().contiguous() for w in (0, 1)]


def _buffers(shapes, dtypes, shift, sentinel=77):
    """flat buffers of `sentinel` with 4 spare elements, and the views that begin `shift` elements in"""
    flat = [torch.full((int(np.prod(s)) + 4,), sentinel, dtype=d, device="cuda") for s, d in zip(shapes, dtypes)]
    return flat, [f[shift:shift + int(np.prod(s))] for f, s in zip(flat, shapes)]


def _guards_untouched(flat, views, shift, sentinel=77):
    return all((f[:shift] == sentinel).all() and (f[shift + v.numel():] == sentinel).all() for f, v in zip(flat, views))


@pytest.mark.parametrize("dtype", [torch.uint8, torch.float32])
def test_ss_entry_points_with_one_sample_give_the_parents_bits(dtype):
    """the new kernels at S = 1 against the existing ones: image, labels, mask and map, with vector and with scalar stores"""
    for H, W in ((20, 56), (37, 53)):
        pano = gpu(np.random.default_rng(21).integers(0, 256, (64, 128, 3), dtype=np.uint8)).to(dtype)
        shapes, dts = [(5, H, W, 3), (5, 2, H, W), (5, H, W)], [dtype, torch.float32, torch.float32]
        (_, want), (_, got) = _buffers(shapes, dts, 0), _buffers(shapes, dts, 0)
        raw_crop(pano, _crop_cam(), H, W, want, None)
        raw_crop(pano, _crop_cam(), H, W, got, 1)
        assert same_bits(want, got), ("crop", H, W)
        assert torch.isnan(got[2]).any() and not (got[0] == 77).all()
        (_, want), (_, got) = _buffers(shapes[:1], dts[:1], 0), _buffers(shapes[:1], dts[:1], 0)   # without labels: the other instantiation
        raw_crop(pano, _crop_cam(), H, W, want + [None, None], None)
        raw_crop(pano, _crop_cam(), H, W, got + [None, None], 1)
        assert same_bits(want, got), ("crop without labels", H, W)

        src = gpu(np.random.default_rng(11).integers(0, 256, (96, 128, 3), dtype=np.uint8)).to(dtype)
        cs, cd = _pair_cams()
        shapes, dts = [(5, H, W, 3), (5, H, W), (5, 2, H, W)], [dtype, torch.uint8, torch.float32]
        (_, want), (_, got) = _buffers(shapes, dts, 0), _buffers(shapes, dts, 0)
        raw_reproject(src, cs, cd, H, W, 3.0, want, None)
        raw_reproject(src, cs, cd, H, W, 3.0, got, 1)
        assert same_bits(want, got), ("reproject", H, W)
        assert 0 < int(got[1].sum()) < got[1].numel()
        (_, want), (_, got) = _buffers(shapes[:1], dts[:1], 0), _buffers(shapes[:1], dts[:1], 0)
        raw_reproject(src, cs, cd, H, W, 3.0, want + [None, None], None)
        raw_reproject(src, cs, cd, H, W, 3.0, got + [None, None], 1)
        assert same_bits(want, got), ("reproject without extras", H, W)

        pano = gpu(rot_ref.u8_panorama(*ROT_SOURCE)).to(dtype)
        rot = gpu(np.radians(np.array(rot_ref.ROTATIONS))).float().contiguous()
        shapes, dts = [(4, H, W, 3), (4, 2, H, W), (4, H, W)], [dtype, torch.float32, torch.float32]
        for inverse in (0, 1):
            (_, want), (_, got) = _buffers(shapes, dts, 0), _buffers(shapes, dts, 0)
            raw_rotate(pano, rot, inverse, H, W, want, None)
            raw_rotate(pano, rot, inverse, H, W, got, 1)
            assert same_bits(want, got), ("rotate", H, W, inverse)
        (_, want), (_, got) = _buffers(shapes[:1], dts[:1], 0), _buffers(shapes[:1], dts[:1], 0)
        raw_rotate(pano, rot, 0, H, W, want + [None, None], None)
        raw_rotate(pano, rot, 0, H, W, got + [None, None], 1)
        assert same_bits(want, got), ("rotate without labels", H, W)


def test_labels_and_map_do_not_depend_on_samples():
    from perspectivefields_amd import reproject_image, rotate_panorama

    pano = gpu(np.random.default_rng(21).integers(0, 256, (64, 128, 3), dtype=np.uint8))
    for H, W in ((20, 56), (37, 53)):
        base = crop(pano, RAW_CROP, H, W)
        rbase = rotate_panorama(pano, 20.0, 35.0, 50.0, height=H, width=W, fields=True)
        for S in SAMPLES:
            got = crop(pano, RAW_CROP, H, W, samples=S)
            assert same_bits(base[1:], got[1:]) and not torch.equal(base[0], got[0]), (H, W, S)
            rgot = rotate_panorama(pano, 20.0, 35.0, 50.0, height=H, width=W, fields=True, samples=S)
            assert same_bits(rbase[1:], rgot[1:]) and not torch.equal(rbase[0], rgot[0]), (H, W, S)
    for Hs, Ws, H, W in SIZES:
        src = gpu(analytic_image(Hs, Ws))
        one = reproject_image(src, cams(CASES, 0), cams(CASES, 1), height=H, width=W, return_map=True)
        four = reproject_image(src, cams(CASES, 0), cams(CASES, 1), height=H, width=W, return_map=True, samples=4)
        assert same_bits(one[1:], four[1:]) and not torch.equal(one[0], four[0])


@pytest.mark.parametrize("S", SAMPLES)
def test_box_mean_known_answers(S):
    """the two known answers of the reference file: a rotation by nothing and a re-projection between cameras of the same relative parameters, from
    (S H, S W) to (H, W), are the S x S box mean of the source"""
    from perspectivefields_amd import reproject_image, rotate_panorama

    H, W = 8, 16
    rng = np.random.default_rng(S)
    src_u = rng.integers(0, 256, (S * H, S * W, 3), dtype=np.uint8)
    src_f = rng.uniform(0, 1, (S * H, S * W, 3)).astype(np.float32)
    box = lambda a: a.astype(np.float64).reshape(a.shape[0] // S, S, a.shape[1] // S, S, 3).mean((1, 3))
    out_u = rotate_panorama(gpu(src_u), 0.0, 0.0, 0.0, height=H, width=W, samples=S)[0].cpu().numpy().astype(np.float64)
    out_f = rotate_panorama(gpu(src_f), 0.0, 0.0, 0.0, height=H, width=W, samples=S)[0].cpu().numpy().astype(np.float64)
    assert np.abs(out_u - box(src_u)).max() <= 1.0
    assert (np.abs(out_f - box(src_f)).max(-1) <= ss.rotate_bound(src_f, (0.0, 0.0, 0.0), False, H, W, S)).all()

    H, W = 9, 13
    src_u = rng.integers(0, 256, (S * H, S * W, 3), dtype=np.uint8)
    src_f = rng.uniform(0, 1, (S * H, S * W, 3)).astype(np.float32)
    cam = dict(zip(KEYS, KNOWN_CAM))
    out_u, valid = reproject_image(gpu(src_u), cam, cam, height=H, width=W, samples=S, return_valid=True)
    out_f = reproject_image(gpu(src_f), cam, cam, height=H, width=W, samples=S)[0].cpu().numpy().astype(np.float64)
    assert valid.all() and np.abs(out_u[0].cpu().numpy().astype(np.float64) - box(src_u)).max() <= 1.0
    th = theta_rad(*KNOWN_CAM)
    a, b, _ = rep_ref.source_coords(th, S * H, S * W, th, S * H, S * W)
    a32, b32 = rep_ref.source_coords_f32(th, S * H, S * W, th, S * H, S * W)
    floor = max(np.abs(a32 - a).max(), np.abs(b32 - b).max())
    step = np.abs(np.diff(src_f.astype(np.float64), axis=1)).max() + np.abs(np.diff(src_f.astype(np.float64), axis=0)).max()   # the largest gradient, both axes
    assert np.abs(out_f - box(src_f)).max() <= 2 * floor * step + 1e-6


# ---------------------------------------------------------------- determinism and isolation
def test_batching_and_determinism():
    """33 outputs (one more than a launch group) of two sources in one call: the same bits on a second run and computed alone"""
    from perspectivefields_amd import crop_panorama, reproject_image, rotate_panorama

    rng = np.random.default_rng(9)
    n = 33
    idx = rng.integers(0, 2, n).tolist()
    srcs = [gpu(rng.integers(0, 256, s, dtype=np.uint8)) for s in ((61, 83, 3), (96, 128, 3))]
    pairs = [CASES[(7 * i) % 60] for i in range(n)]
    run = lambda p, images, **kw: reproject_image(images, cams(p, 0), cams(p, 1), height=36, width=52, return_valid=True, return_map=True, samples=3, **kw)
    first = run(pairs, srcs, src_index=idx)
    assert same_bits(first, run(pairs, srcs, src_index=idx))
    for i in range(n):
        assert same_bits([t[i] for t in first], [t[0] for t in run(pairs[i:i + 1], srcs[idx[i]])]), i

    panos = [gpu(rng.integers(0, 256, s, dtype=np.uint8)) for s in ((40, 80, 3), (64, 128, 3))]
    cam = np.stack([rng.uniform(-40, 40, n), rng.uniform(-80, 80, n), rng.uniform(-180, 180, n), rng.uniform(0.3, 1.5, n),
                    rng.uniform(-0.1, 0.1, n), rng.uniform(-0.1, 0.1, n), rng.choice([0.0, 0.0, 0.5, 1.3], n)], 1)
    run = lambda c, p, **kw: crop_panorama(p, c[:, 0], c[:, 1], c[:, 3], c[:, 4], c[:, 5], yaw=c[:, 2], xi=c[:, 6], height=36, width=52, samples=2, **kw)
    first = run(cam, panos, pano_index=idx)
    assert same_bits(first, run(cam, panos, pano_index=idx))
    for i in range(n):
        assert same_bits([t[i] for t in first], [t[0] for t in run(cam[i:i + 1], panos[idx[i]])]), i

    rots = np.stack([rng.uniform(-180, 180, n), rng.uniform(-90, 90, n), rng.uniform(-180, 180, n)], 1)
    run = lambda r, p, **kw: rotate_panorama(p, r[:, 0], r[:, 1], r[:, 2], height=19, width=37, fields=True, samples=4, **kw)
    first = run(rots, panos, pano_index=idx)
    assert same_bits(first, run(rots, panos, pano_index=idx))
    for i in range(n):
        assert same_bits([t[i] for t in first], [t[0] for t in run(rots[i:i + 1], panos[idx[i]])]), i


@pytest.mark.parametrize("dtype", [torch.uint8, torch.float32])
def test_unaligned_outputs_take_the_scalar_stores_and_write_nothing_around_them(dtype):
    """W = 56 into aligned outputs (vector stores) against the same raw call into buffers shifted by one element (scalar stores): the same bits, and
    the guard bands in front of and behind every buffer keep their value"""
    H, W, S = 20, 56, 3
    pano = gpu(np.random.default_rng(21).integers(0, 256, (64, 128, 3), dtype=np.uint8)).to(dtype)
    shapes, dts = [(5, H, W, 3), (5, 2, H, W), (5, H, W)], [dtype, torch.float32, torch.float32]
    (_, want), (flat, got) = _buffers(shapes, dts, 0), _buffers(shapes, dts, 1)
    assert got[0].data_ptr() % (4 if dtype == torch.uint8 else 16) != 0 and want[0].data_ptr() % 16 == 0
    raw_crop(pano, _crop_cam(), H, W, want, S)
    raw_crop(pano, _crop_cam(), H, W, got, S)
    assert same_bits(want, got) and _guards_untouched(flat, got, 1)

    src = gpu(np.random.default_rng(11).integers(0, 256, (96, 128, 3), dtype=np.uint8)).to(dtype)
    cs, cd = _pair_cams()
    shapes, dts = [(5, H, W, 3), (5, H, W), (5, 2, H, W)], [dtype, torch.uint8, torch.float32]
    (_, want), (flat, got) = _buffers(shapes, dts, 0), _buffers(shapes, dts, 1)
    raw_reproject(src, cs, cd, H, W, 3.0, want, S)
    raw_reproject(src, cs, cd, H, W, 3.0, got, S)
    assert same_bits(want, got) and _guards_untouched(flat, got, 1)

    pano = gpu(rot_ref.u8_panorama(*ROT_SOURCE)).to(dtype)
    rot = gpu(np.radians(np.array(rot_ref.ROTATIONS[:3]))).float().contiguous()
    shapes, dts = [(3, H, W, 3), (3, 2, H, W), (3, H, W)], [dtype, torch.float32, torch.float32]
    (_, want), (flat, got) = _buffers(shapes, dts, 0), _buffers(shapes, dts, 1)
    raw_rotate(pano, rot, 0, H, W, want, S)
    raw_rotate(pano, rot, 0, H, W, got, S)
    assert same_bits(want, got) and _guards_untouched(flat, got, 1)


def test_a_nan_row_is_empty_and_leaves_the_other_rows_alone():
    from perspectivefields_amd import crop_panorama, reproject_image, rotate_panorama

    S = 3
    Hs, Ws, H, W = SIZES[1]
    src = gpu(np.random.default_rng(17).integers(0, 256, (Hs, Ws, 3), dtype=np.uint8))
    pairs = CASES[:4]
    run = lambda cs, cd: reproject_image(src, cs, cd, height=H, width=W, fill=7, return_valid=True, return_map=True, samples=S)
    good = run(cams(pairs, 0), cams(pairs, 1))
    for where, key in ((0, "rel_focal"), (1, "pitch")):
        c = [cams(pairs, 0), cams(pairs, 1)]
        c[where][key] = c[where][key].copy()
        c[where][key][1] = np.nan
        img, valid, cmap = run(*c)
        assert not valid[1].any() and (img[1] == 7).all()
        for i in (0, 2, 3):
            assert same_bits([t[i] for t in good], [img[i], valid[i], cmap[i]]), i

    pano = gpu(np.random.default_rng(18).integers(0, 256, (40, 80, 3), dtype=np.uint8))
    cam = np.asarray(CROP_CASES[:4], dtype=np.float64)
    run = lambda c: crop_panorama(pano, c[:, 0], c[:, 1], c[:, 3], c[:, 4], c[:, 5], yaw=c[:, 2], xi=c[:, 6], height=H, width=W, samples=S)
    good = run(cam)
    for col in (0, 3, 6):
        bad = cam.copy()
        bad[1, col] = np.nan
        got = run(bad)
        assert (got[0][1] == 0).all() and torch.isnan(got[1][1]).all() and torch.isnan(got[2][1]).all(), col
        for i in (0, 2, 3):
            assert same_bits([t[i] for t in good], [t[i] for t in got]), (col, i)

    rots = np.array(rot_ref.ROTATIONS[:3])
    good = rotate_panorama(pano, rots[:, 0], rots[:, 1], rots[:, 2], height=H, width=W, fields=True, samples=S)
    for bad in ((np.nan, 0.0, 0.0), (0.0, np.inf, 0.0), (0.0, 0.0, -np.inf)):
        with_bad = np.insert(rots, 1, bad, axis=0)
        got = rotate_panorama(pano, with_bad[:, 0], with_bad[:, 1], with_bad[:, 2], height=H, width=W, fields=True, samples=S)
        assert (got[0][1] == 0).all() and torch.isnan(got[1][1]).all() and torch.isnan(got[2][1]).all()
        assert same_bits(good, [t[[0, 2, 3]] for t in got])


# ---------------------------------------------------------------- model methods
def test_rectify_forwards_samples():
    from perspectivefields_amd import PerspectiveFields, reproject_image

    view = gpu(np.random.default_rng(21).integers(0, 256, (96, 128, 3), dtype=np.uint8))
    m = PerspectiveFields.__new__(PerspectiveFields)   # rectify reads nothing of the model
    preds = dict(pred_roll=20.0, pred_pitch=15.0, pred_rel_focal=0.7, pred_xi=0.4)
    got = PerspectiveFields.rectify(m, view, preds, height=40, width=56, return_valid=True, return_map=True, samples=3)
    src = dict(roll=20.0, pitch=15.0, rel_focal=0.7, rel_cx=0.0, rel_cy=0.0, xi=0.4)
    want = reproject_image(view, src, dict(roll=0.0, pitch=15.0, rel_focal=0.7, xi=0.0), height=40, width=56, return_valid=True, return_map=True, samples=3)
    assert same_bits(want, got)
    assert not torch.equal(got[0], PerspectiveFields.rectify(m, view, preds, height=40, width=56))


def test_level_panorama_passes_samples_to_its_rotation():
    from perspectivefields_amd import PerspectiveFields, rotate_panorama

    m = PerspectiveFields.__new__(PerspectiveFields)   # with preds given, nothing of the model is read
    upright = gpu(rot_ref.u8_panorama(64, 128, seed=3))
    tilted = rotate_panorama(upright, rot_ref.TILT[0], rot_ref.TILT[1])[0]
    _, roll, pitch = rot_ref.view_truth(rot_ref.TILT, pitches=(0.0,))
    preds = [dict(pred_roll=float(r), pred_pitch=float(p), pred_rel_focal=0.5) for r, p in zip(roll, pitch)]
    out, info = PerspectiveFields.level_panorama(m, tilted, preds=preds, return_info=True, samples=2)
    assert torch.equal(out, rotate_panorama(tilted, info["roll"], info["pitch"], inverse=True, samples=2)[0])
    assert not torch.equal(out, PerspectiveFields.level_panorama(m, tilted, preds=preds))


# ---------------------------------------------------------------- what it is for
def test_supersampling_takes_the_aliasing_out_on_the_device():
    from perspectivefields_amd import reproject_image

    A = ALIAS
    src = gpu(ss.checkerboard(A["Hs"], A["Ws"]))
    use = ss.alias_reference(1)[1] & ss.alias_reference(4)[1]
    one = reproject_image(src, A["src"], A["dst"], height=A["H"], width=A["W"])[0].cpu().numpy()
    four = reproject_image(src, A["src"], A["dst"], height=A["H"], width=A["W"], samples=4)[0].cpu().numpy()
    s1, s4 = one[use].std(), four[use].std()
    print(f"a checkerboard of period 2 texels, minified 4 x, on the device: standard deviation {s1:.4f} at S = 1, {s4:.4f} at S = 4")
    assert s1 >= 0.1 and s4 < 0.5 * s1
