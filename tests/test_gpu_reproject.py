"""Re-projection between cameras on the GPU (include/pf_hip.h pf_reproject, perspectivefields_amd.reproject_image, PerspectiveFields.rectify)
against the fp64 reference of tests/test_reproject_ref.py: the map, the mask, float32 and uint8 images, the identity, closure with the
panorama crop, batch invariance across launch groups, the vector and scalar store paths, non-finite parameters, and rectify.

Tolerances.  The map is held to 4 x the error of the same formulas evaluated in numpy float32 in the same run (test_reproject_ref.fp32_floor; the
device's sincosf / sqrtf / division differ from numpy's): in px on the pixels inside the source image, and divided by 1 + rho_s^2 on the
visible pixels outside it, where a ray's rounding error is magnified by that factor and the coordinate itself is unbounded.  The float32
image is held to (measured map error) x (largest analytic gradient of the source per px) x 2 + 1e-6, the uint8 image to 1 LSB of the fp64
value before rounding.  Pixels that test_reproject_ref.clear excludes (at most 0.36 % of an image, asserted <= 1 % there) are left out."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests.test_gpu_pano_crop import direction_panorama
from tests.test_reproject_ref import CASES, CLOSURE_CASES, SIZES, angles_deg, clear, closure_reference, fp32_floor, map_errors, sample, source_coords, theta_rad

pytestmark = pytest.mark.gpu

KEYS = ("roll", "pitch", "yaw", "rel_focal", "rel_cx", "rel_cy", "xi")
FX, FY = (0.31, 0.05, 0.23), (0.07, 0.29, 0.19)   # radians per pixel of the analytic image's three channels
GRAD = 0.5 * max(FX + FY)                         # its largest derivative along a row or a column, per px


def cams(cases, which):
    c = np.asarray([case[which] for case in cases], dtype=np.float64)
    return {k: c[:, i] for i, k in enumerate(KEYS)}


def analytic_image(Hs, Ws):
    """float32 (Hs, Ws, 3) in [0, 1]: 0.5 + 0.5 sin(fx col + fy row + channel), pixel centres at col + 1/2, row + 1/2"""
    rows, cols = np.meshgrid(np.arange(Hs) + 0.5, np.arange(Ws) + 0.5, indexing="ij")
    return np.stack([0.5 + 0.5 * np.sin(fx * cols + fy * rows + k) for k, (fx, fy) in enumerate(zip(FX, FY))], -1).astype(np.float32)


@functools.lru_cache(None)
def reference(size):
    """per case: (a, b, inside, clear) in fp64; computed once, read only"""
    Hs, Ws, H, W = size
    out = []
    for s, d in CASES:
        s, d = theta_rad(*s), theta_rad(*d)
        out.append(source_coords(s, Hs, Ws, d, H, W) + (clear(s, Hs, Ws, d, H, W),))
    return out


@functools.lru_cache(None)
def floor_of(size):
    return tuple(fp32_floor(size))


@functools.lru_cache(None)
def gpu_float_run(size, fill):
    """all 60 cases at one size in one call: (image, valid, map) as numpy"""
    from perspectivefields_amd import reproject_image

    Hs, Ws, H, W = size
    src = torch.from_numpy(analytic_image(Hs, Ws)).cuda()
    img, valid, cmap = reproject_image(src, cams(CASES, 0), cams(CASES, 1), height=H, width=W, fill=fill, return_valid=True, return_map=True)
    assert img.shape == (60, H, W, 3) and img.dtype == torch.float32 and valid.shape == (60, H, W) and valid.dtype == torch.bool
    assert cmap.shape == (60, 2, H, W) and cmap.dtype == torch.float32
    return img.cpu().numpy(), valid.cpu().numpy(), cmap.cpu().numpy()


def gpu_map_error(size):
    """largest map errors of the GPU over the cases (px inside, normalised outside) and whether every NaN pattern matches"""
    Hs, Ws, H, W = size
    _, _, cmap = gpu_float_run(size, 0.0)
    worst, same = np.zeros(2), True
    for k, (s, d) in enumerate(CASES):
        e_in, e_out, ok = map_errors(theta_rad(*s), Hs, Ws, theta_rad(*d), H, W, cmap[k, 0], cmap[k, 1])
        worst, same = np.maximum(worst, (e_in, e_out)), same and ok
    return worst, same


@pytest.mark.parametrize("size", SIZES)
def test_map_matches_the_fp64_reference(size):
    worst, same = gpu_map_error(size)
    floor = floor_of(size)
    print(f"map error at {size}: GPU {worst[0]:.3e} px inside (fp32 floor {floor[0]:.3e}), {worst[1]:.3e} normalised outside (floor {floor[1]:.3e})")
    assert same, "NaN where the reference is visible, or a value where it is not"
    assert worst[0] <= 4 * floor[0] and worst[1] <= 4 * floor[1], (worst, floor)


@pytest.mark.parametrize("size", SIZES)
def test_mask_is_the_inside_test(size):
    _, valid, _ = gpu_float_run(size, 0.0)
    for k, (_, _, inside, cl) in enumerate(reference(size)):
        assert np.array_equal(valid[k][cl], inside[cl]), CASES[k]


@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("fill", [0.0, 0.5])
def test_float32_image(size, fill):
    Hs, Ws, H, W = size
    img, valid, _ = gpu_float_run(size, fill)
    src = analytic_image(Hs, Ws)
    tol = gpu_map_error(size)[0][0] * GRAD * 2 + 1e-6
    worst = 0.0
    for k, (a, b, inside, cl) in enumerate(reference(size)):
        ref = sample(src, a, b, inside, fill)
        m = cl & inside
        worst = max(worst, np.abs(img[k].astype(np.float64) - ref)[m].max())
        assert (img[k][~valid[k]] == np.float32(fill)).all(), CASES[k]
        assert (img[k][cl & ~inside] == np.float32(fill)).all(), CASES[k]
    print(f"float32 image at {size}: largest error {worst:.3e}, allowed {tol:.3e}")
    assert worst <= tol


@pytest.mark.parametrize("size", SIZES)
def test_uint8_image_within_one_lsb(size):
    from perspectivefields_amd import reproject_image

    Hs, Ws, H, W = size
    src = np.random.default_rng(3).integers(0, 256, (Hs, Ws, 3), dtype=np.uint8)
    img = reproject_image(torch.from_numpy(src).cuda(), cams(CASES, 0), cams(CASES, 1), height=H, width=W)
    assert torch.is_tensor(img) and img.dtype == torch.uint8 and img.shape == (60, H, W, 3)
    img = img.cpu().numpy().astype(np.float64)
    for k, (a, b, inside, cl) in enumerate(reference(size)):
        assert np.abs(img[k] - sample(src, a, b, inside, 0.0))[cl].max() <= 1.0, CASES[k]


@pytest.mark.parametrize("xi", [0.0, 0.5])
def test_identity(xi):
    from perspectivefields_amd import reproject_image

    src = torch.from_numpy(np.random.default_rng(5).integers(0, 256, (61, 83, 3), dtype=np.uint8)).cuda()
    cam = dict(roll=12.0, pitch=-20.0, yaw=33.0, rel_focal=0.45, rel_cx=0.04, rel_cy=-0.03, xi=xi)
    img, valid = reproject_image(src, cam, cam, return_valid=True)
    assert img.shape == (1, 61, 83, 3) and valid.all()
    assert torch.equal(img[0], src)


def test_closure_with_the_panorama_crop():
    """crop at A, re-projected A -> B, against the direct crop at B, on a panorama of directions: no worse than the fp64 reference's own
    closure (the bilinear error of sampling twice) plus the 2e-3 degrees of the panorama crop's geometry test"""
    from perspectivefields_amd import crop_panorama, reproject_image

    H, W = 96, 128
    pano = direction_panorama(512, 1024)
    pano_gpu = torch.from_numpy(pano).float().cuda()
    pairs = [CASES[k] for k in CLOSURE_CASES]
    crops = []
    for which in (0, 1):
        c = cams(pairs, which)
        crops.append(crop_panorama(pano_gpu, c["roll"], c["pitch"], c["rel_focal"], c["rel_cx"], c["rel_cy"], yaw=c["yaw"], xi=c["xi"], height=H, width=W, fields=False)[0])
    warped = reproject_image(crops[0], cams(pairs, 0), cams(pairs, 1)).cpu().numpy().astype(np.float64)
    direct = crops[1].cpu().numpy().astype(np.float64)
    for i, (s, d) in enumerate(pairs):
        ref_ang, use = closure_reference(pano, theta_rad(*s), theta_rad(*d), H, W)
        ang = angles_deg(warped[i], direct[i], use)
        print(f"closure of case {CLOSURE_CASES[i]}: GPU {ang.max():.5f} deg, fp64 reference {ref_ang.max():.5f} deg over {use.sum()} pixels")
        assert ang.max() <= ref_ang.max() + 2e-3, (CLOSURE_CASES[i], ang.max(), ref_ang.max())


def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def test_batch_invariance_over_groups_and_sources():
    from perspectivefields_amd import reproject_image

    rng = np.random.default_rng(9)
    srcs = [torch.from_numpy(rng.integers(0, 256, s, dtype=np.uint8)).cuda() for s in ((61, 83, 3), (96, 128, 3))]
    n = 33   # one more than a launch group
    pairs = [CASES[(7 * i) % 60] for i in range(n)]
    idx = rng.integers(0, 2, n).tolist()
    H, W = 36, 52
    run = lambda s, d, images, **kw: reproject_image(images, s, d, height=H, width=W, return_valid=True, return_map=True, **kw)
    first = run(cams(pairs, 0), cams(pairs, 1), srcs, src_index=idx)
    again = run(cams(pairs, 0), cams(pairs, 1), srcs, src_index=idx)
    for a, b in zip(first, again):
        assert torch.equal(_bits(a), _bits(b))
    for i in range(n):
        one = run(cams(pairs[i:i + 1], 0), cams(pairs[i:i + 1], 1), srcs[idx[i]])
        for a, b in zip(first, one):
            assert torch.equal(_bits(a[i]), _bits(b[0])), i


def _raw_call(src, cam_s, cam_d, H, W, img_ptr, valid_ptr, map_ptr):
    from perspectivefields_amd.engine import _check, load_library

    lib = load_library()
    hw = (ctypes.c_int32 * 2)(int(src.shape[0]), int(src.shape[1]))
    B = cam_s.shape[0]
    _check(lib.pf_reproject(0, 1, (ctypes.c_void_p * 1)(src.data_ptr()), hw, 0 if src.dtype == torch.uint8 else 1, B, (ctypes.c_int32 * B)(*([0] * B)),
                            cam_s.data_ptr(), cam_d.data_ptr(), H, W, 0.0, img_ptr, valid_ptr, map_ptr, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)),
           None, "pf_reproject")


@pytest.mark.parametrize("dtype", [torch.uint8, torch.float32])
def test_unaligned_outputs_take_the_scalar_stores_and_give_the_same_bits(dtype):
    """reproject_image allocates its outputs itself, always aligned; storage that is not 16-byte aligned reaches pf_reproject only through
    the C interface, called here directly: W = 56 with aligned outputs (vector stores) against the same call into buffers shifted by one
    element (scalar stores)"""
    from perspectivefields_amd import reproject_image

    Hs, Ws, H, W = SIZES[0]
    pairs = CASES[:5]
    src = torch.from_numpy(np.random.default_rng(11).integers(0, 256, (Hs, Ws, 3), dtype=np.uint8)).cuda().to(dtype)
    rad = lambda which: {k: (np.radians(v) if k in KEYS[:3] else v) for k, v in cams(pairs, which).items()}
    img, valid, cmap = reproject_image(src, rad(0), rad(1), height=H, width=W, mode="rad", return_valid=True, return_map=True)
    cam = [torch.from_numpy(np.stack([rad(which)[k] for k in KEYS], 1)).cuda().float().contiguous() for which in (0, 1)]
    n = 5 * H * W
    img2 = torch.zeros(n * 3 + 1, dtype=dtype, device="cuda")
    valid2 = torch.zeros(n + 1, dtype=torch.uint8, device="cuda")
    map2 = torch.zeros(n * 2 + 1, dtype=torch.float32, device="cuda")
    _raw_call(src, cam[0], cam[1], H, W, img2[1:].data_ptr(), valid2[1:].data_ptr(), map2[1:].data_ptr())
    assert img2[1:].data_ptr() % (4 if dtype == torch.uint8 else 16) != 0
    assert torch.equal(_bits(img2[1:].reshape(img.shape)), _bits(img))
    assert torch.equal(valid2[1:].reshape(valid.shape), valid.view(torch.uint8))
    assert torch.equal(_bits(map2[1:].reshape(cmap.shape)), _bits(cmap))
    assert img2[0] == 0 and valid2[0] == 0 and map2[0] == 0   # nothing written in front of the buffers


@pytest.mark.parametrize("H,W", [(1, 17), (19, 1), (16, 64), (17, 68)])
def test_thin_and_tile_sized_outputs(H, W):
    """one row, one column, exactly one tile, and one pixel row and one 4-pixel group past a tile; the source of SIZES[1], whose fp32
    floor bounds the map here too (the error is set by the source's size and focal length, which are the same)"""
    from perspectivefields_amd import reproject_image

    Hs, Ws = SIZES[1][:2]
    pairs = CASES[:12]
    src = np.random.default_rng(13).integers(0, 256, (Hs, Ws, 3), dtype=np.uint8)
    img, valid, cmap = reproject_image(torch.from_numpy(src).cuda(), cams(pairs, 0), cams(pairs, 1), height=H, width=W, return_valid=True, return_map=True)
    img, valid, cmap = img.cpu().numpy().astype(np.float64), valid.cpu().numpy(), cmap.cpu().numpy()
    floor = floor_of(SIZES[1])
    for k, (s, d) in enumerate(pairs):
        s, d = theta_rad(*s), theta_rad(*d)
        a, b, inside = source_coords(s, Hs, Ws, d, H, W)
        cl = clear(s, Hs, Ws, d, H, W)
        e_in, e_out, same = map_errors(s, Hs, Ws, d, H, W, cmap[k, 0], cmap[k, 1])
        assert same and e_in <= 4 * floor[0] and e_out <= 4 * floor[1], (pairs[k], e_in, e_out)
        assert np.array_equal(valid[k][cl], inside[cl]), pairs[k]
        if cl.any():
            assert np.abs(img[k] - sample(src, a, b, inside, 0.0))[cl].max() <= 1.0, pairs[k]


@pytest.mark.parametrize("where,key", [(0, "rel_focal"), (1, "rel_focal"), (0, "roll"), (1, "pitch")])
def test_non_finite_parameters_invalidate_their_row_only(where, key):
    from perspectivefields_amd import reproject_image

    Hs, Ws, H, W = SIZES[1]
    pairs = CASES[:4]
    src = torch.from_numpy(np.random.default_rng(17).integers(0, 256, (Hs, Ws, 3), dtype=np.uint8)).cuda()
    good = reproject_image(src, cams(pairs, 0), cams(pairs, 1), height=H, width=W, fill=7, return_valid=True, return_map=True)
    c = [cams(pairs, 0), cams(pairs, 1)]
    c[where][key] = c[where][key].copy()
    c[where][key][1] = np.nan
    img, valid, cmap = reproject_image(src, c[0], c[1], height=H, width=W, fill=7, return_valid=True, return_map=True)
    assert not valid[1].any() and (img[1] == 7).all()
    for i in (0, 2, 3):
        for a, b in zip(good, (img, valid, cmap)):
            assert torch.equal(_bits(a[i]), _bits(b[i])), i


def _map_equal(a, b):
    return torch.equal(_bits(a), _bits(b))


def test_rectify_renders_the_documented_destination():
    from perspectivefields_amd import PerspectiveFields, crop_panorama, reproject_image

    H, W = 96, 128
    pano = torch.from_numpy(np.random.default_rng(21).integers(0, 256, (256, 512, 3), dtype=np.uint8)).cuda()
    view, _, _ = crop_panorama(pano, 20.0, 15.0, 0.7, height=H, width=W, fields=False)
    preds = dict(pred_roll=20.0, pred_pitch=15.0, pred_rel_focal=0.7)
    m = PerspectiveFields.__new__(PerspectiveFields)   # rectify reads nothing of the model
    src = dict(roll=20.0, pitch=15.0, rel_focal=0.7)
    img, valid, cmap = PerspectiveFields.rectify(m, view, preds, return_valid=True, return_map=True)   # level="roll"
    assert img.shape == (1, H, W, 3) and img.dtype == torch.uint8 and valid.dtype == torch.bool and img.is_cuda
    th_s, th_d = theta_rad(20.0, 15.0, 0.0, 0.7, 0.0, 0.0, 0.0), theta_rad(0.0, 15.0, 0.0, 0.7, 0.0, 0.0, 0.0)
    floor = floor_of(SIZES[0])   # the same source size, 96 x 128
    e_in, e_out, same = map_errors(th_s, H, W, th_d, H, W, *cmap[0].cpu().numpy())
    assert same and e_in <= 4 * floor[0] and e_out <= 4 * floor[1], (e_in, e_out, floor)
    a, b, inside = source_coords(th_s, H, W, th_d, H, W)
    cl = clear(th_s, H, W, th_d, H, W)
    assert np.abs(img[0].cpu().numpy().astype(np.float64) - sample(view[0].cpu().numpy(), a, b, inside))[cl].max() <= 1.0
    # every option against reproject_image with the destination the docstring states: the same call underneath, so the same bits
    full = dict(pred_roll=torch.tensor(20.0, device="cuda"), pred_pitch=torch.tensor(15.0, device="cuda"), pred_rel_focal=torch.tensor(0.7, device="cuda"),
                pred_rel_cx=0.03, pred_rel_cy=torch.tensor(-0.02, device="cuda"), pred_xi=0.4)
    src = dict(roll=20.0, pitch=15.0, rel_focal=0.7, rel_cx=0.03, rel_cy=-0.02, xi=0.4)
    for kw, dst, size in ((dict(), dict(roll=0.0, pitch=15.0, rel_focal=0.7, xi=0.0), {}),
                          (dict(level="full"), dict(roll=0.0, pitch=0.0, rel_focal=0.7, xi=0.0), {}),
                          (dict(level="none", undistort=False), dict(roll=20.0, pitch=15.0, rel_focal=0.7, xi=0.4), {}),
                          (dict(level="full", undistort=False, rel_focal=0.5), dict(roll=0.0, pitch=0.0, rel_focal=0.5, xi=0.4), dict(height=40, width=56)),
                          (dict(rel_focal=1.1), dict(roll=0.0, pitch=15.0, rel_focal=1.1, xi=0.0), dict(height=37, width=53))):
        got = PerspectiveFields.rectify(m, view[0], full, return_map=True, **kw, **size)
        want = reproject_image(view[0], src, dst, return_map=True, **size)
        assert got[0].shape == (1, size.get("height", H), size.get("width", W), 3)
        assert torch.equal(got[0], want[0]) and _map_equal(got[1], want[1]), kw
    # a list of results with a batched tensor
    _, cmap = PerspectiveFields.rectify(m, view, [preds], level="full", return_map=True)
    assert cmap.shape == (1, 2, H, W)


def test_crop_infer_fit_rectify_end_to_end():
    from perspectivefields_amd import PerspectiveFields, crop_panorama

    pano = torch.from_numpy(np.random.default_rng(12).integers(0, 256, (256, 512, 3), dtype=np.uint8)).cuda()
    m = PerspectiveFields("Paramnet-360Cities-edina-centered", weights="synthetic:0").eval().cuda()
    B, H, W = 3, 120, 160
    img, _, _ = crop_panorama(pano, [0.0, 10.0, -20.0], [5.0, -30.0, 40.0], [0.8, 1.1, 0.6], yaw=[0.0, 120.0, -170.0], height=H, width=W, fields=False)
    preds = m.inference_batch(list(img))
    for p in (preds, m.fit_camera(preds), m.fit_camera(preds, distortion=True)):
        out, valid = m.rectify(img, p, level="full", return_valid=True)
        assert out.shape == (B, H, W, 3) and out.dtype == torch.uint8 and out.device == img.device
        assert valid.shape == (B, H, W) and valid.dtype == torch.bool
    one = m.rectify(img[0], preds[0], height=60, width=80)
    assert one.shape == (1, 60, 80, 3) and one.dtype == torch.uint8
