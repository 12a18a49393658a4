"""rotate_panorama / panorama_fields / level_panorama on the GPU (include/pf_hip.h pf_pano_rotate, pf_pano_fields) against
the fp64 reference of tests/test_pano_rotate_ref.py: the float32 image held to the float32 floor of the same formulas, uint8 within one LSB, the
known answers, the labels, the closure with crop_panorama and of the two directions, determinism and batching, the scalar store path, non-finite
angles, and levelling end to end."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests.test_pano_compose_ref import pano_directions
from tests.test_pano_crop_ref import crop_image
from tests.test_pano_rotate_ref import (EDGE_OUTPUTS, OUTPUTS, ROTATIONS, SOURCES, T_EXCLUDE, TILT, UP, decompose, direction_panorama, fields, floor_of,
                                        image_bound, pixel_angles, rot_matrix, rot_rad, rotate_image, rotation, u8_panorama, up_angle_deg, view_truth,
                                        yaw_matrix)

pytestmark = pytest.mark.gpu
R2D = 180.0 / np.pi
CASES = [(rot, inverse) for rot in ROTATIONS for inverse in (False, True)]


def gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def run_cases(src, out, fields_=True):
    """every rotation, forward and inverse, of one source in one call: (images, up, lat) as numpy"""
    from perspectivefields_amd import rotate_panorama

    rots = np.array([rot for rot, _ in CASES])
    res = []
    for inverse in (False, True):
        sel = [i for i, (_, inv) in enumerate(CASES) if inv == inverse]
        res.append((sel, rotate_panorama(gpu(src), rots[sel, 0], rots[sel, 1], rots[sel, 2], inverse=inverse, height=out[0], width=out[1], fields=fields_)))
    per_case = [None] * len(CASES)
    for sel, r in res:
        r = r if fields_ else (r, None, None)
        for k, i in enumerate(sel):
            per_case[i] = tuple(None if t is None else t[k].cpu().numpy() for t in r)
    return per_case


@pytest.mark.parametrize("src_size", SOURCES)
@pytest.mark.parametrize("out", OUTPUTS + EDGE_OUTPUTS)
def test_float32_image_and_labels_match_the_fp64_reference(out, src_size):
    """a panorama of directions (value range 2): every pixel within 2 x (float32 coordinate floor x local gradient) + 1e-6 of the fp64 image; the
    latitude within 4 x its float32 floor (at least 1e-5 degrees), the up vectors within 4 x theirs by angle, away from the zenith and nadir"""
    src = direction_panorama(*src_size)
    got = run_cases(src, out)
    worst = np.zeros(3)
    for (rot, inverse), (img, up, lat) in zip(CASES, got):
        th = rot_rad(*rot)
        ref = rotate_image(src, th, inverse, *out)
        bound = image_bound(src, th, inverse, *out)
        err = np.abs(img.astype(np.float64) - ref).max(-1)
        _, _, f_lat, f_up = floor_of(rot, inverse, out, src_size)
        up_ref, lat_ref, tn = fields(th, inverse, *out)
        e_lat = np.abs(lat.astype(np.float64) - lat_ref).max()
        use = tn >= T_EXCLUDE
        e_up = up_angle_deg(up, up_ref)[use].max()
        worst = np.maximum(worst, [(err / bound).max(), e_lat / max(4 * f_lat, 1e-5), e_up / (4 * f_up) if f_up > 0 else 0.0])
        print(f"{out} from {src_size}, {rot}, inverse {inverse}: image error {err.max():.3e} (error / allowed {(err / bound).max():.3f}), latitude {e_lat:.3e} deg "
              f"(floor {f_lat:.3e}), up {e_up:.3e} deg (floor {f_up:.3e}), {int((~use).sum())} pixels left out")
        assert (err <= bound).all(), (rot, inverse, (err / bound).max())
        assert e_lat <= max(4 * f_lat, 1e-5), (rot, inverse)
        assert np.isfinite(up[:, use]).all() and e_up <= 4 * f_up, (rot, inverse)
        gone = up[:, ~use]   # a pixel centre on the zenith or nadir: NaN, or some unit vector
        assert (np.isnan(gone) | (np.abs((gone * gone).sum(0) - 1) <= 1e-5)).all()
    print(f"{out} from {src_size}: worst error / allowed: image {worst[0]:.3f}, latitude {worst[1]:.3f}, up {worst[2]:.3f}")


@pytest.mark.parametrize("src_size", SOURCES)
@pytest.mark.parametrize("out", OUTPUTS + EDGE_OUTPUTS)
def test_uint8_within_one_lsb(out, src_size):
    """within 1 LSB of the rounded fp64 value.  A pixel centre that looks along the source's axis (pitch 90 on 37 x 75 and on the one-row and
    one-column outputs: one pixel each) has no longitude, in fp64 as little as in float32: its sample is some point of the source's first or last
    row, so there the value is held to the range of that row's texels, 1 LSB beyond at the most"""
    src = u8_panorama(*src_size)
    got = run_cases(src, out, fields_=False)
    for (rot, inverse), (img, _, _) in zip(CASES, got):
        th = rot_rad(*rot)
        ref = rotate_image(src, th, inverse, *out)
        rounded = np.clip(np.floor(ref + 0.5), 0, 255)
        X = pano_directions(*out) @ rot_matrix(th, inverse).T
        axis = np.hypot(X[..., 0], X[..., 2]) < 1e-6
        assert axis.sum() <= 1 and (not axis.any() or rot == (0.0, 90.0, 0.0))
        d = np.abs(img.astype(np.float64) - ref)[~axis].max()
        print(f"{out} from {src_size}, {rot}, inverse {inverse}: largest distance from the unrounded fp64 value {d:.4f} LSB, {int(axis.sum())} pixels on the axis")
        assert img.dtype == np.uint8 and np.abs(img.astype(np.float64) - rounded)[~axis].max() <= 1.0
        for r, c in np.argwhere(axis):
            row = src[0 if X[r, c, 1] < 0 else -1].astype(np.float64)   # X.y = -1: the north pole, row 0
            assert (img[r, c] >= row.min(0) - 1).all() and (img[r, c] <= row.max(0) + 1).all()


def test_known_answers_uint8():
    """at equal sizes the sample lands on a texel (within 1e-5 px): no rotation gives the source back, a yaw of whole columns rolls them"""
    from perspectivefields_amd import rotate_panorama

    for size in SOURCES:
        src = gpu(np.random.default_rng(5).integers(0, 256, (*size, 3), dtype=np.uint8))
        for inverse in (False, True):
            assert torch.equal(rotate_panorama(src, inverse=inverse)[0], src)
            for k in (1, 7, -5, size[1] // 2, size[1]):
                out = rotate_panorama(src, yaw=k * 360.0 / size[1], inverse=inverse)[0]
                assert torch.equal(out, torch.roll(src, k if inverse else -k, dims=1)), (size, inverse, k)


def test_upright_camera_labels_and_panorama_fields_bits():
    from perspectivefields_amd import panorama_fields, rotate_panorama

    for out in OUTPUTS + EDGE_OUTPUTS:
        up, lat = panorama_fields(0.0, 0.0, height=out[0], width=out[1])
        assert up.shape == (1, 2, *out) and lat.shape == (1, *out)
        assert (up[0, 0] == 0).all() and (up[0, 1] == -1).all()
        ref_lat, _ = pixel_angles(*out)
        f_lat = floor_of((0.0, 0.0, 0.0), False, out, SOURCES[0])[2]
        assert np.abs(lat[0].cpu().numpy().astype(np.float64) - ref_lat * R2D).max() <= max(f_lat, 1e-5)
    # the labels alone are the bits of the labels of the gather, for every rotation and both store paths
    rots = np.array(ROTATIONS + [(5.0, -20.0, 130.0)])
    src = gpu(u8_panorama(*SOURCES[1]))
    for out in OUTPUTS + EDGE_OUTPUTS:
        _, up, lat = rotate_panorama(src, rots[:, 0], rots[:, 1], 0.0, height=out[0], width=out[1], fields=True)
        up2, lat2 = panorama_fields(rots[:, 0], rots[:, 1], height=out[0], width=out[1])
        assert torch.equal(_bits(up), _bits(up2)) and torch.equal(_bits(lat), _bits(lat2)), out


def view_thetas(views):
    f = 0.5 / np.tan(np.radians(45.0))
    return [(np.radians(r), np.radians(p), np.radians(y), f, 0.0, 0.0, 0.0) for r, p, y in views]


def test_closure_with_the_panorama_crop():
    """the panorama of directions rotated on the GPU, then cropped to 48 x 48 views of 90 degrees, against the crop of the unrotated panorama with
    the composed camera A V: no worse than the same two chains in fp64 plus 2e-5 of the value range.  This pins forward against inverse, against
    an independent kernel"""
    from perspectivefields_amd import crop_panorama, rotate_panorama

    src = direction_panorama(64, 128)
    views = [(0.0, 0.0, 0.0), (10.0, 20.0, 90.0), (-15.0, -40.0, 200.0), (0.0, 70.0, -60.0)]
    f = 0.5 / np.tan(np.radians(45.0))
    for rot in ROTATIONS[:3]:
        for inverse in (False, True):
            A = rot_matrix(rot_rad(*rot), inverse)
            rotated = rotate_panorama(gpu(src), *rot, inverse=inverse)[0]
            composed = [decompose(A @ yaw_matrix(y) @ rotation(r, p)) for r, p, y, *_ in view_thetas(views)]
            v = np.array(views)
            a, _, _ = crop_panorama(rotated, v[:, 0], v[:, 1], f, yaw=v[:, 2], height=48, width=48, fields=False)
            c = np.degrees(np.array(composed))
            b, _, _ = crop_panorama(gpu(src), c[:, 0], c[:, 1], f, yaw=c[:, 2], height=48, width=48, fields=False)
            e_gpu = float((a - b).abs().max())
            rot64 = rotate_image(src, rot_rad(*rot), inverse, 64, 128)
            e_ref = max(np.abs(crop_image(rot64, th, 48, 48) - crop_image(src, (*cm, f, 0.0, 0.0, 0.0), 48, 48)).max() for th, cm in zip(view_thetas(views), composed))
            print(f"closure rotate -> crop, {rot}, inverse {inverse}: GPU difference {e_gpu:.6f}, fp64 reference chain {e_ref:.6f} (value range 2)")
            assert e_gpu <= e_ref + 2e-5 * 2.0


def test_closure_of_the_two_directions():
    """rotate, then rotate with inverse, against the source on a smooth panorama: no worse than the fp64 chain plus 2e-5 of the value range"""
    from perspectivefields_amd import rotate_panorama

    for size in SOURCES:
        src = direction_panorama(*size)
        for rot in ROTATIONS:
            for first in (False, True):
                once = rotate_panorama(gpu(src), *rot, inverse=first)[0]
                back = rotate_panorama(once, *rot, inverse=not first)[0].cpu().numpy()
                th = rot_rad(*rot)
                ref = rotate_image(rotate_image(src, th, first, *size), th, not first, *size)
                e_gpu, e_ref = np.abs(back.astype(np.float64) - src).max(), np.abs(ref - src).max()
                print(f"closure of the two directions at {size}, {rot}, inverse first {first}: GPU error {e_gpu:.6f}, fp64 chain {e_ref:.6f}")
                assert e_gpu <= e_ref + 2e-5 * 2.0


@pytest.mark.parametrize("dtype", [torch.uint8, torch.float32])
def test_batching_and_determinism(dtype):
    """outputs of different sources in one call have the bits of each alone, in another order and on every run; 33 outputs span two launches"""
    from perspectivefields_amd import rotate_panorama

    rng = np.random.default_rng(8)
    srcs = [gpu(rng.integers(0, 256, (*s, 3), dtype=np.uint8)).to(dtype) for s in SOURCES]
    n = 33
    rots = np.stack([rng.uniform(-180, 180, n), rng.uniform(-90, 90, n), rng.uniform(-360, 360, n)], 1)
    index = [int(i) for i in rng.integers(0, 2, n)]
    run = lambda order: rotate_panorama(srcs, rots[order, 0], rots[order, 1], rots[order, 2], inverse=True, height=37, width=75, pano_index=[index[i] for i in order], fields=True)
    every = list(range(n))
    first, again = run(every), run(every)
    assert first[0].shape == (n, 37, 75, 3) and first[0].dtype == dtype
    perm = [int(i) for i in rng.permutation(n)]
    mixed = run(perm)
    for a, b, c in zip(first, again, mixed):
        assert torch.equal(_bits(a), _bits(b))
        assert torch.equal(_bits(a[perm]), _bits(c))
    for i in (0, 5, 31, 32):   # both sides of the launch boundary
        alone = rotate_panorama(srcs[index[i]], *rots[i], inverse=True, height=37, width=75, fields=True)
        for a, b in zip(first, alone):
            assert torch.equal(_bits(a[i]), _bits(b[0])), i
    few = run([3, 4, 32])
    for a, b in zip(first, few):
        assert torch.equal(_bits(a[[3, 4, 32]]), _bits(b))


@pytest.mark.parametrize("dtype", [torch.uint8, torch.float32])
def test_unaligned_outputs_take_the_scalar_stores_and_give_the_same_bits(dtype):
    """rotate_panorama allocates its outputs itself, always aligned; storage that is not aligned reaches pf_pano_rotate only through the C interface,
    called here directly: 32 x 64 into aligned outputs (vector stores) against the same call into buffers shifted by one element"""
    from perspectivefields_amd import rotate_panorama
    from perspectivefields_amd.engine import _check, load_library

    H, W = OUTPUTS[0]
    src = gpu(u8_panorama(*SOURCES[1])).to(dtype)
    rots = np.array(ROTATIONS[:3])
    B, n = len(rots), H * W
    img, up, lat = rotate_panorama(src, rots[:, 0], rots[:, 1], rots[:, 2], height=H, width=W, fields=True)
    rot = torch.from_numpy(np.radians(rots)).cuda().float().contiguous()
    lib = load_library()
    for s_img, s_up, s_lat in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1)):
        img2 = torch.zeros(B * n * 3 + 4, dtype=dtype, device="cuda")
        up2, lat2 = torch.zeros(B * n * 2 + 4, device="cuda"), torch.zeros(B * n + 4, device="cuda")
        i2, u2, l2 = img2[s_img:s_img + B * n * 3], up2[s_up:s_up + B * n * 2], lat2[s_lat:s_lat + B * n]
        assert (i2.data_ptr() % (4 if dtype == torch.uint8 else 16) != 0) == bool(s_img) and (u2.data_ptr() % 16 != 0) == bool(s_up) and (l2.data_ptr() % 16 != 0) == bool(s_lat)
        _check(lib.pf_pano_rotate(0, 1, (ctypes.c_void_p * 1)(src.data_ptr()), (ctypes.c_int32 * 2)(*SOURCES[1]), 0 if dtype == torch.uint8 else 1, B,
                                  (ctypes.c_int32 * B)(*([0] * B)), rot.data_ptr(), 0, H, W, i2.data_ptr(), u2.data_ptr(), l2.data_ptr(),
                                  ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), None, "pf_pano_rotate")
        assert torch.equal(_bits(i2.reshape(img.shape)), _bits(img))
        assert torch.equal(_bits(u2.reshape(up.shape)), _bits(up)) and torch.equal(_bits(l2.reshape(lat.shape)), _bits(lat))
        for buf, s, m in ((img2, s_img, B * n * 3), (up2, s_up, B * n * 2), (lat2, s_lat, B * n)):   # nothing written around the buffers
            assert (buf[:s] == 0).all() and (buf[s + m:] == 0).all()
    # the labels alone, into shifted buffers
    up2, lat2 = torch.zeros(B * n * 2 + 4, device="cuda"), torch.zeros(B * n + 4, device="cuda")
    _check(lib.pf_pano_fields(0, B, rot.data_ptr(), 0, H, W, up2[1:].data_ptr(), lat2[1:].data_ptr(), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), None,
           "pf_pano_fields")
    assert torch.equal(_bits(up2[1:1 + B * n * 2].reshape(up.shape)), _bits(up)) and torch.equal(_bits(lat2[1:1 + B * n].reshape(lat.shape)), _bits(lat))
    assert up2[0] == 0 and (up2[1 + B * n * 2:] == 0).all() and lat2[0] == 0 and (lat2[1 + B * n:] == 0).all()


@pytest.mark.parametrize("bad", [(np.nan, 0.0, 0.0), (0.0, np.inf, 0.0), (0.0, 0.0, -np.inf)])
def test_non_finite_angles_give_0_and_nan_and_leave_the_rest_alone(bad):
    from perspectivefields_amd import panorama_fields, rotate_panorama

    src = gpu(u8_panorama(*SOURCES[0]))
    rots = np.array(ROTATIONS[:3])
    good = rotate_panorama(src, rots[:, 0], rots[:, 1], rots[:, 2], height=37, width=75, fields=True)
    with_bad = np.insert(rots, 1, bad, axis=0)
    got = rotate_panorama(src, with_bad[:, 0], with_bad[:, 1], with_bad[:, 2], height=37, width=75, fields=True)
    assert (got[0][1] == 0).all() and torch.isnan(got[1][1]).all() and torch.isnan(got[2][1]).all()
    for a, b in zip(good, got):
        assert torch.equal(_bits(a), _bits(b[[0, 2, 3]]))
    f32 = rotate_panorama(src.float(), *bad, height=16, width=32)
    assert (f32 == 0).all()
    if np.isfinite(bad[2]):
        up, lat = panorama_fields(bad[0], bad[1], height=16, width=32)
        assert torch.isnan(up).all() and torch.isnan(lat).all()


@functools.lru_cache(None)
def model():
    from perspectivefields_amd import PerspectiveFields

    return PerspectiveFields("Paramnet-360Cities-edina-centered", weights="synthetic:0").eval().cuda()


def test_levelling_end_to_end_with_the_true_view_parameters():
    """an analytic panorama tilted by (20, 35); every view's prediction is its true roll and pitch: the estimate is the tilt and the image the bits of
    rotate_panorama with it; with the views' fields and fit_camera, the estimate is as good as the fit's own votes"""
    from perspectivefields_amd import fields_from_params, rotate_panorama

    m = model()
    upright = gpu(u8_panorama(64, 128, seed=3))
    tilted = rotate_panorama(upright, TILT[0], TILT[1])[0]
    cams, roll, pitch = view_truth(TILT, pitches=(0.0,))
    preds = [dict(pred_roll=float(r), pred_pitch=float(p), pred_rel_focal=0.5) for r, p in zip(roll, pitch)]
    out, info = m.level_panorama(tilted, preds=preds, return_info=True)
    assert abs(float(info["roll"]) - TILT[0]) <= 1e-6 and abs(float(info["pitch"]) - TILT[1]) <= 1e-6
    assert out.shape == tilted.shape and out.dtype == tilted.dtype and len(info["preds"]) == 8 and info["views"]["yaw"] == cams["yaw"]
    assert torch.equal(out, rotate_panorama(tilted, info["roll"], info["pitch"], inverse=True)[0])
    assert torch.equal(out, m.level_panorama(tilted, preds=preds))
    close = (out.int() - upright.int()).abs().float().mean()   # two bilinear samplings of a smooth picture: the upright panorama again, nearly
    assert float(close) <= 3.0
    # two rows of views, and fit_camera on their ground-truth fields
    cams, roll, pitch = view_truth(TILT, pitches=(0.0, 30.0))
    f = 0.5 / np.tan(np.radians(45.0))
    fields_ = [fields_from_params(float(r), float(p), f, height=64, width=64) for r, p in zip(roll, pitch)]
    preds = [dict(pred_gravity_original=up, pred_latitude_original=lat) for up, lat in fields_]
    _, info = m.level_panorama(tilted, view_pitch=(0.0, 30.0), use="fit", preds=preds, return_info=True)
    g = rotation(np.radians(TILT[0]), np.radians(TILT[1])).T @ UP
    angle = lambda v: np.degrees(np.arctan2(np.linalg.norm(np.cross(v, g), axis=-1), v @ g))
    per_view = angle(info["gravity"]["votes"].cpu().numpy())
    e = float(angle(info["gravity"]["direction"].cpu().numpy()))
    print(f"levelling with fit_camera on the views' true fields: estimate ({float(info['roll']):.5f}, {float(info['pitch']):.5f}) degrees, {e:.2e} degrees from "
          f"the tilt; the views' own votes are off by up to {per_view.max():.2e} degrees")
    assert len(info["preds"]) == 16 and e <= per_view.max() + 1e-3


def test_level_panorama_runs_on_a_synthetic_model():
    m = model()
    pano = gpu(u8_panorama(64, 128, seed=4))
    out, info = m.level_panorama(pano, return_info=True)
    assert out.shape == pano.shape and out.dtype == pano.dtype and out.device == pano.device
    assert len(info["preds"]) == 8 and all("pred_roll" in p for p in info["preds"]) and info["gravity"]["votes"].shape == (8, 3)
    out2 = m.level_panorama(pano.float(), n_yaw=3, view_pitch=(0.0, 20.0), view_size=96, use="fit")
    assert out2.shape == pano.shape and out2.dtype == torch.float32
