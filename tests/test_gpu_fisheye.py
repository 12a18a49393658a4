"""crop_fisheye / fisheye_to_panorama on the GPU (include/pf_hip.h pf_fisheye_crop, pf_fisheye_to_pano) against the fp64
reference of tests/test_fisheye_ref.py: the mask, the float32 image held to the float32 floor of the same formulas, uint8 within one LSB, the
closure with the panorama crop of a stereographic view, the seam of two lenses, supersampling against the block mean, batching and determinism,
the scalar store path, non-finite lens entries and parameters, and the fields.

A pixel is left out of a value comparison only where test_fisheye_ref.case_floor says so (the two precisions disagree on a lens's coverage, the pixel
sits on theta_max or on the frame's border, or 0 < S < 1e-3); at most 1 % of any output, asserted per case."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests.test_cubemap_ref import smooth_panorama, view_rad
from tests.test_fisheye_ref import (EQUIDISTANT, KIND_NAMES, OFF, PANO_CASES, PANO_OUTPUTS, PANO_ROTATIONS, RIG_NAMES, RIGS, SS_RIGS, SS_SAMPLES, STEREOGRAPHIC, TMAX,
                                    VIEW_CAMERAS, VIEW_OUTPUTS, block_mean_fill, crop_frame, frame_to_pano, frame_value, image_bound, lens_project, lens_row,
                                    pano_case, rig_lenses, ss_pano_kept, ss_view_kept, view_case)
from tests.test_gpu_reproject import GRAD, analytic_image
from tests.test_pano_compose_ref import pano_directions
from tests.test_pano_crop_ref import crop_image, rotation
from tests.test_pano_rotate_ref import decompose, rot_matrix, rot_rad

pytestmark = pytest.mark.gpu
FILL = 0.25


def gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


@functools.lru_cache(None)
def frame_of(name, dtype):
    """the analytic frame of a rig: float32 in [0, 1], or its uint8 rounding of 255 x; read only"""
    img = analytic_image(*RIGS[name][0])
    return img if dtype == "f32" else np.clip(np.floor(255.0 * img.astype(np.float64) + 0.5), 0, 255).astype(np.uint8)


def fill_of(dtype):
    return FILL if dtype == "f32" else 37.0


@functools.lru_cache(None)
def run_panoramas(name, dtype, out, samples=1):
    """every rotation and direction of one rig at one output size, one call per direction: {(rot, inverse): (image, mask) as numpy}; read only"""
    from perspectivefields_amd import fisheye_to_panorama

    r = np.array(PANO_ROTATIONS)
    got = {}
    for inverse in (False, True):
        img, mask = fisheye_to_panorama(gpu(frame_of(name, dtype)), rig_lenses(name), height=out[0], width=out[1], roll=r[:, 0], pitch=r[:, 1], yaw=r[:, 2],
                                        inverse=inverse, projection=KIND_NAMES[RIGS[name][1]], samples=samples, fill=fill_of(dtype), return_mask=True)
        assert img.shape == (len(r), *out, 3) and mask.shape == (len(r), *out) and mask.dtype == torch.bool
        for i, rot in enumerate(PANO_ROTATIONS):
            got[rot, inverse] = (img[i].cpu().numpy(), mask[i].cpu().numpy())
    return got


@functools.lru_cache(None)
def run_views(name, dtype, out, samples=1):
    """every view camera of one rig at one output size in one call: {cam: (image, mask) as numpy}; read only"""
    from perspectivefields_amd import crop_fisheye

    c = np.array(VIEW_CAMERAS)
    img, _, _, mask = crop_fisheye(gpu(frame_of(name, dtype)), rig_lenses(name), c[:, 0], c[:, 1], c[:, 3], c[:, 4], c[:, 5], yaw=c[:, 2], xi=c[:, 6], height=out[0],
                                   width=out[1], projection=KIND_NAMES[RIGS[name][1]], fields=False, samples=samples, fill=fill_of(dtype), return_mask=True)
    return {cam: (img[i].cpu().numpy(), mask[i].cpu().numpy()) for i, cam in enumerate(VIEW_CAMERAS)}


def cases_of(name, out, views, dtype="f32"):
    """(key, the case's floor and kept pixels, (fp64 image, fp64 mask), (GPU image, GPU mask)) of every case of a rig at one output size"""
    (Hs, Ws), kind, lenses = RIGS[name]
    frame = frame_of(name, dtype)
    if views:
        got = run_views(name, dtype, out)
        for cam in VIEW_CAMERAS:
            yield cam, view_case(name, cam, out), crop_frame(frame, lenses, kind, view_rad(cam), *out, fill=fill_of(dtype)), got[cam]
    else:
        got = run_panoramas(name, dtype, out)
        for rot, inverse in PANO_CASES:
            yield (rot, inverse), pano_case(name, rot, inverse, out), frame_to_pano(frame, lenses, kind, rot_rad(*rot), inverse, *out, fill=fill_of(dtype)), got[rot, inverse]


OUTPUT_CASES = [(out, False) for out in PANO_OUTPUTS] + [(out, True) for out in VIEW_OUTPUTS]


# ---------------------------------------------------------------- the mask and the images
@pytest.mark.parametrize("out,views", OUTPUT_CASES)
def test_mask_and_float32_image_match_the_fp64_reference(out, views):
    """the mask equals the reference's on every kept pixel, at most 1 % of a case is left out, a pixel outside the mask holds `fill`, and every kept
    pixel inside it is within (covering lenses x coordinate floor x largest gradient x 2) + (covering lenses x weight floor x value range) / S_ref +
    1e-6 of the fp64 image; the floors are those of the numpy float32 evaluation of the same case"""
    worst = 0.0
    for name in RIG_NAMES:
        for key, case, (ref, ref_mask), (img, mask) in cases_of(name, out, views):
            kept = case["kept"]
            assert 1.0 - kept.mean() <= 0.01, (name, key, case["left"])
            assert np.array_equal(mask[kept], ref_mask[kept]), (name, key)
            assert (img[~mask] == np.float32(FILL)).all(), (name, key)
            m = kept & ref_mask
            if not m.any():
                continue
            err = np.abs(img.astype(np.float64) - ref).max(-1)
            ratio = (err / image_bound(case, GRAD))[m].max()
            worst = max(worst, ratio)
            print(f"rig {name}, {out}, {key}: error {err[m].max():.3e}, error / allowed {ratio:.3f}, floors {case['e_c']:.3e} px and {case['e_w']:.3e}, "
                  f"{int((~kept).sum())} pixels left out")
            assert ratio <= 1.0, (name, key, ratio)
    print(f"{out}, {'views' if views else 'panoramas'}: worst error / allowed {worst:.3f}")


@pytest.mark.parametrize("out,views", OUTPUT_CASES)
def test_uint8_within_one_lsb(out, views):
    """every kept pixel within 1 LSB of the rounded fp64 value"""
    for name in RIG_NAMES:
        for key, case, (ref, ref_mask), (img, mask) in cases_of(name, out, views, "u8"):
            assert img.dtype == np.uint8
            kept = case["kept"]
            assert np.array_equal(mask[kept], ref_mask[kept]) and (img[~mask] == 37).all(), (name, key)
            d = np.abs(img.astype(np.float64) - np.clip(np.floor(ref + 0.5), 0, 255)).max(-1)
            assert d[kept].max() <= 1.0, (name, key, d[kept].max())


# ---------------------------------------------------------------- closure and seam
def test_closure_panorama_to_stereographic_view_to_panorama():
    """a 64 x 128 float32 panorama of directions (value range 2) is cut by crop_panorama(xi=1) into a stereographic fisheye of 96 x 96 (the USM camera
    of xi = 1 and focal 2 F is the stereographic lens of F) and read back by fisheye_to_panorama: over the covered pixels no worse than the same
    chain in fp64 plus 4e-5"""
    from perspectivefields_amd import crop_panorama, fisheye_to_panorama

    src = smooth_panorama(64, 128)
    cam = (10.0, 20.0, 30.0, 0.25, 0.0, 0.0, 1.0)   # F_s = 0.25 x 96 = 24 = 2 F
    lens = lens_row(STEREOGRAPHIC, *cam[:3], 120.0, 0.0, (48.0, 48.0), F=12.0)   # r(120 degrees) = 41.6 px < 48
    frame, _, _ = crop_panorama(gpu(src), cam[0], cam[1], cam[3], yaw=cam[2], xi=cam[6], height=96, width=96, fields=False)
    back, mask = fisheye_to_panorama(frame[0], lens, height=64, width=128, projection="stereographic", return_mask=True)
    back, mask = back[0].cpu().numpy().astype(np.float64), mask[0].cpu().numpy()
    frame64 = crop_image(src.astype(np.float64), view_rad(cam), 96, 96)
    ref, ref_mask = frame_to_pano(frame64, [lens], STEREOGRAPHIC, (0.0, 0.0, 0.0), False, 64, 128)
    th, _, _ = lens_project(lens, STEREOGRAPHIC, pano_directions(64, 128))
    clear = np.abs(th - lens[TMAX]) > 1e-4
    assert np.array_equal(mask[clear], ref_mask[clear]) and 0.5 < ref_mask.mean() < 0.95
    m = mask & ref_mask
    e_gpu, e_ref = np.abs(back - src)[m].max(), np.abs(ref - src)[m].max()
    print(f"closure panorama -> stereographic view -> panorama: GPU error {e_gpu:.6f}, fp64 chain {e_ref:.6f}")
    assert e_ref <= 0.01 and e_gpu <= e_ref + 4e-5


def seam_frame():
    """rig B's frame with constant lens images: 0 in the left circle's half, 1 in the right one's"""
    frame = np.zeros((24, 48, 3), np.float32)
    frame[:, 24:] = 1.0
    return frame


def test_seam_of_two_lenses_is_0_or_1_outside_the_overlap_and_has_no_step():
    from perspectivefields_amd import fisheye_to_panorama

    lenses = rig_lenses("B")
    img = fisheye_to_panorama(gpu(seam_frame()), lenses, height=32, width=64)[0].cpu().numpy().astype(np.float64)
    ref, n = frame_value(seam_frame(), lenses, EQUIDISTANT, pano_directions(32, 64))[::3]
    kept = pano_case("B", (0.0, 0.0, 0.0), False, (32, 64))["kept"]
    outside, inside = kept & (n == 1), kept & (n == 2)
    assert outside.any() and inside.any() and ((img[outside] == 0.0) | (img[outside] == 1.0)).all()
    assert img[inside].min() >= 0.0 and img[inside].max() <= 1.0 and 0.0 < img[inside].mean() < 1.0
    for axis in (0, 1):
        d_gpu, d_ref = np.abs(np.diff(img, axis=axis)).max(), np.abs(np.diff(ref, axis=axis)).max()
        assert d_gpu <= d_ref + 1e-4, (axis, d_gpu, d_ref)


def test_seam_is_monotone_along_the_great_circles_through_the_lens_axis():
    """a panorama whose north pole is the axis of lens 0: its columns are the great circles through the axis, theta of lens 0 grows with the row, so
    every column goes from 0 (lens 0 alone) up to 1 (lens 1 alone) and never back"""
    from perspectivefields_amd import fisheye_to_panorama

    lenses = rig_lenses("B")
    polar = decompose(rot_matrix(lenses[0, :3]) @ rotation(0.0, -np.pi / 2))   # A (0, -1, 0) = Q0 (0, 0, 1)
    assert np.abs(rot_matrix(polar) @ [0.0, -1.0, 0.0] - rot_matrix(lenses[0, :3]) @ [0.0, 0.0, 1.0]).max() <= 1e-12
    img = fisheye_to_panorama(gpu(seam_frame()), lenses, height=32, width=64, roll=polar[0], pitch=polar[1], yaw=polar[2], mode="rad")[0].cpu().numpy().astype(np.float64)
    ref, _ = frame_to_pano(seam_frame(), lenses, EQUIDISTANT, polar, False, 32, 64)
    assert np.diff(ref, axis=0).min() >= -1e-12 and (ref[0] == 0).all() and (ref[-1] == 1).all()   # the property holds for the model
    assert np.diff(img, axis=0).min() >= -1e-6 and (img[:12] == 0).all() and (img[-12:] == 1).all()
    ramp = (img[..., 0] > 0) & (img[..., 0] < 1)
    assert ramp[14:18].any() and not ramp[:14].any() and not ramp[19:].any()


# ---------------------------------------------------------------- supersampling
@pytest.mark.parametrize("S", SS_SAMPLES)
@pytest.mark.parametrize("dtype", ["f32", "u8"])
def test_supersampling_is_the_block_mean_of_the_fine_call(dtype, S):
    """samples=S equals the S x S block mean, over the valid sub-pixels (the fine call's mask), of the same call at S times the size with samples=1:
    float32 within 1e-5 of the value range (1) on the analytic frame, uint8 within 1 LSB, and the mask is the "any" of the block.  The two calls
    evaluate the same points with different float32 roundings, so an output pixel is compared where all of its sub-pixels are kept pixels of the
    fine case (test_fisheye_ref.block_kept); at most 1 % of any output is left out, asserted per case here and on the reference alone there"""
    tol = 1e-5 if dtype == "f32" else 1.0
    worst = 0.0
    for name in SS_RIGS:
        for out, run, kept_of, keys in ((PANO_OUTPUTS[1], run_panoramas, lambda k: ss_pano_kept(name, *k, S), PANO_CASES),
                                        (VIEW_OUTPUTS[1], run_views, lambda k: ss_view_kept(name, k, S), VIEW_CAMERAS)):
            fine, coarse = run(name, dtype, (S * out[0], S * out[1])), run(name, dtype, out, S)
            for key in keys:
                (f_img, f_mask), (img, mask) = fine[key], coarse[key]
                kept = kept_of(key)
                assert 1.0 - kept.mean() <= 0.01, (name, key, S, kept.mean())
                want, want_any = block_mean_fill(f_img.astype(np.float64), f_mask, S, fill_of(dtype))
                assert np.array_equal(mask[kept], want_any[kept]), (name, key, S)
                d = np.abs(img.astype(np.float64) - want).max(-1)[kept].max()
                worst = max(worst, d)
                assert d <= tol, (name, key, S, d)
    print(f"samples = {S}, {dtype}: largest difference from the block mean {worst:.3e} (allowed {tol:g})")


# ---------------------------------------------------------------- batching, determinism, stores
@pytest.mark.parametrize("dtype", ["u8", "f32"])
def test_batching_and_determinism(dtype):
    """33 outputs over the frames of rigs A and B (two launches): the same bits repeated, permuted and alone on both sides of the launch boundary"""
    from perspectivefields_amd import crop_fisheye, fisheye_to_panorama

    rng = np.random.default_rng(8)
    frames = [gpu(frame_of(name, dtype)) for name in ("A", "B")]
    lenses = [rig_lenses("A"), rig_lenses("B")]
    n = 33
    rots = np.stack([rng.uniform(-180, 180, n), rng.uniform(-90, 90, n), rng.uniform(-360, 360, n)], 1)
    foc, xi = rng.uniform(0.3, 1.2, n), np.where(rng.uniform(size=n) < 0.5, 0.0, rng.uniform(0.0, 1.2, n))
    index = [int(i) for i in rng.integers(0, 2, n)]
    pano = lambda o: fisheye_to_panorama(frames, lenses, height=37, width=75, roll=rots[o, 0], pitch=rots[o, 1], yaw=rots[o, 2], inverse=True,
                                         frame_index=[index[i] for i in o], samples=2, fill=3.0, return_mask=True)
    view = lambda o: crop_fisheye(frames, lenses, rots[o, 0], rots[o, 1], foc[o], yaw=rots[o, 2], xi=xi[o], height=31, width=47, frame_index=[index[i] for i in o],
                                  fields=False, fill=3.0, return_mask=True)[::3]
    for run in (pano, view):
        every = list(range(n))
        first, again = run(every), run(every)
        assert first[0].shape[0] == n and first[0].dtype == frames[0].dtype and bool(first[1].any()) and not bool(first[1].all())
        perm = [int(i) for i in rng.permutation(n)]
        permuted = run(perm)
        for k in (0, 1):   # the image and the mask
            assert torch.equal(_bits(first[k]), _bits(again[k])) and torch.equal(_bits(first[k][perm]), _bits(permuted[k]))
            for i in (0, 31, 32):
                assert torch.equal(_bits(first[k][i]), _bits(run([i])[k][0])), i
            assert torch.equal(_bits(first[k][[3, 4, 32]]), _bits(run([3, 4, 32])[k]))


@pytest.mark.parametrize("dtype", [torch.uint8, torch.float32])
def test_unaligned_outputs_take_the_scalar_stores_and_give_the_same_bits(dtype):
    """the Python functions allocate aligned outputs; storage that is not aligned reaches the entry points only through the C interface: 32 x 64
    into aligned outputs (vector stores) against the same call into an image shifted by one element, and into a mask shifted by one byte, and
    nothing written around them"""
    from perspectivefields_amd import crop_fisheye, fisheye_to_panorama
    from perspectivefields_amd.engine import _check, load_library

    H, W = 32, 64
    frame = gpu(frame_of("B", "u8" if dtype == torch.uint8 else "f32"))
    rots = np.array(PANO_ROTATIONS)
    B, n = len(rots), H * W
    lib = load_library()
    stream = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    lens = gpu(np.repeat(rig_lenses("B")[None], B, axis=0).astype(np.float32))
    head = (0, 1, (ctypes.c_void_p * 1)(frame.data_ptr()), (ctypes.c_int32 * 2)(24, 48), 0 if dtype == torch.uint8 else 1, EQUIDISTANT, B,
            (ctypes.c_int32 * B)(*([0] * B)), lens.data_ptr())
    rot = torch.from_numpy(np.radians(rots)).cuda().float().contiguous()
    cam = torch.cat([rot, torch.tensor([[0.6, 0.0, 0.0, 0.8]] * B, device="cuda")], 1).contiguous()
    want_p = fisheye_to_panorama(frame, rig_lenses("B"), height=H, width=W, roll=rots[:, 0], pitch=rots[:, 1], yaw=rots[:, 2], samples=2, fill=5.0, return_mask=True)
    want_v = crop_fisheye(frame, rig_lenses("B"), rots[:, 0], rots[:, 1], 0.6, yaw=rots[:, 2], xi=0.8, height=H, width=W, fields=False, samples=2, fill=5.0,
                          return_mask=True)[::3]
    for shift_img, shift_mask in ((0, 0), (1, 0), (0, 1)):
        for want, call in ((want_p, lambda p, v: lib.pf_fisheye_to_pano(*head, rot.data_ptr(), 0, H, W, 5.0, p, v, 2, stream())),
                           (want_v, lambda p, v: lib.pf_fisheye_crop(*head, cam.data_ptr(), H, W, 5.0, p, v, 2, stream()))):
            buf = torch.zeros(B * n * 3 + 4, dtype=dtype, device="cuda")
            mbuf = torch.full((B * n + 4,), 9, dtype=torch.uint8, device="cuda")
            out, valid = buf[shift_img:shift_img + B * n * 3], mbuf[shift_mask:shift_mask + B * n]
            assert (out.data_ptr() % (4 if dtype == torch.uint8 else 16) != 0) == bool(shift_img) and (valid.data_ptr() % 4 != 0) == bool(shift_mask)
            _check(call(out.data_ptr(), valid.data_ptr()), None, "fisheye gather")
            assert torch.equal(_bits(out.reshape(want[0].shape)), _bits(want[0])) and torch.equal(valid.reshape(want[1].shape), want[1].view(torch.uint8))
            assert (buf[:shift_img] == 0).all() and (buf[shift_img + B * n * 3:] == 0).all()
            assert (mbuf[:shift_mask] == 9).all() and (mbuf[shift_mask + B * n:] == 9).all()


# ---------------------------------------------------------------- non-finite entries, fields
@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_a_non_finite_entry_of_lens_1_gives_the_bits_of_lens_0_alone(bad):
    from perspectivefields_amd import crop_fisheye, fisheye_to_panorama

    lenses = rig_lenses("B")
    cam = VIEW_CAMERAS[1]
    for dtype in ("u8", "f32"):
        frame = gpu(frame_of("B", dtype))
        pano = lambda l: fisheye_to_panorama(frame, l, height=37, width=75, roll=10.0, pitch=20.0, yaw=30.0, fill=2.0, return_mask=True)
        view = lambda l: crop_fisheye(frame, l, cam[0], cam[1], cam[3], cam[4], cam[5], yaw=cam[2], xi=cam[6], height=31, width=47, fields=False, fill=2.0,
                                      return_mask=True)[::3]
        for run in (pano, view):
            alone = run(np.stack([lenses[0], OFF]))
            assert not alone[1].all() and alone[1].any()
            assert torch.equal(_bits(alone[0]), _bits(run(lenses[0])[0]))   # one row: the second lens is switched off
            assert not torch.equal(_bits(alone[0]), _bits(run(lenses)[0]))
            for k in range(12):
                broken = lenses.copy()
                broken[1, k] = bad
                got = run(broken)
                assert torch.equal(_bits(got[0]), _bits(alone[0])) and torch.equal(got[1], alone[1]), (dtype, k)


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_non_finite_camera_and_angle_rows_give_fill_and_leave_the_rest_alone(bad):
    from perspectivefields_amd import crop_fisheye, fisheye_to_panorama

    lenses = rig_lenses("B")
    for dtype in ("u8", "f32"):
        frame = gpu(frame_of("B", dtype))
        rots = np.array(PANO_ROTATIONS)
        pano = lambda r: fisheye_to_panorama(frame, lenses, height=37, width=75, roll=r[:, 0], pitch=r[:, 1], yaw=r[:, 2], fill=7.0, samples=2, return_mask=True)
        good = pano(rots)
        for column in range(3):
            with_bad = np.insert(rots, 1, rots[1], axis=0)
            with_bad[1, column] = bad
            got = pano(with_bad)
            assert (got[0][1] == 7).all() and not got[1][1].any(), column
            assert torch.equal(_bits(good[0]), _bits(got[0][[0, 2, 3]])) and torch.equal(good[1], got[1][[0, 2, 3]])
        cams = np.array(VIEW_CAMERAS)
        view = lambda c: crop_fisheye(frame, lenses, c[:, 0], c[:, 1], c[:, 3], c[:, 4], c[:, 5], yaw=c[:, 2], xi=c[:, 6], height=31, width=47, fields=False, fill=7.0,
                                      return_mask=True)[::3]
        good = view(cams)
        for column in range(7):
            with_bad = np.insert(cams, 1, cams[1], axis=0)
            with_bad[1, column] = bad
            got = view(with_bad)
            assert (got[0][1] == 7).all() and not got[1][1].any(), column
            assert torch.equal(_bits(good[0]), _bits(got[0][[0, 2, 3]])) and torch.equal(good[1], got[1][[0, 2, 3]])


def test_fields_are_those_of_the_parameters():
    from perspectivefields_amd import crop_fisheye, fields_from_params, fisheye_to_panorama, panorama_fields

    frame = gpu(frame_of("A", "u8"))
    cams = np.array(VIEW_CAMERAS)
    out = crop_fisheye(frame, rig_lenses("A"), cams[:, 0], cams[:, 1], cams[:, 3], cams[:, 4], cams[:, 5], yaw=cams[:, 2], xi=cams[:, 6], height=31, width=47)
    assert len(out) == 3
    for i, c in enumerate(VIEW_CAMERAS):
        u, l = fields_from_params(c[0], c[1], c[3], c[4], c[5], height=31, width=47, xi=torch.tensor(c[6], dtype=torch.float64))
        assert torch.equal(_bits(out[1][i]), _bits(u)) and torch.equal(_bits(out[2][i]), _bits(l)), c
    _, up, lat, mask = crop_fisheye(frame, rig_lenses("A"), 10.0, 20.0, 0.7, yaw=30.0, height=31, width=47, return_mask=True)   # the number 0 for xi: the pinhole entry point
    u, l = fields_from_params(10.0, 20.0, 0.7, height=31, width=47)
    assert torch.equal(_bits(up[0]), _bits(u)) and torch.equal(_bits(lat[0]), _bits(l)) and mask.dtype == torch.bool
    rots = np.array(PANO_ROTATIONS)
    img, up, lat = fisheye_to_panorama(frame, rig_lenses("A"), height=37, width=75, roll=rots[:, 0], pitch=rots[:, 1], yaw=rots[:, 2], fields=True)
    u, l = panorama_fields(rots[:, 0], rots[:, 1], height=37, width=75)
    assert img.shape == (3, 37, 75, 3) and torch.equal(_bits(up), _bits(u)) and torch.equal(_bits(lat), _bits(l))
    assert len(fisheye_to_panorama(frame, rig_lenses("A"), height=37, width=75, fields=True, return_mask=True)) == 4
