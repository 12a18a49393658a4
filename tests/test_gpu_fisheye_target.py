"""panorama_to_fisheye / fisheye_fields on the GPU (include/pf_hip.h pf_pano_to_fisheye, pf_fisheye_fields) against the fp64
reference of tests/test_fisheye_target_ref.py: the mask, the float32 image held to the float32 floor of the same formulas, uint8 within one LSB, the
labels held to four times the float32 floor, the closure with fisheye_to_panorama and crop_fisheye, supersampling against the block mean, batching
and determinism, the scalar store path and non-finite lens entries.

A pixel is left out of a comparison only where test_fisheye_target_ref.target_case says so (the two precisions disagree on the owner, or the pixel
sits within 1e-3 px of r_max; for the up vector also |t|^2 < 1e-8); at most 1 % of any frame, asserted per case here and on the reference there."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests.test_cubemap_ref import smooth_panorama, view_rad
from tests.test_fisheye_ref import KIND_NAMES, OFF, crop_frame, frame_to_pano
from tests.test_fisheye_target_ref import (PANOS, SS_SAMPLES, SS_TARGETS, TARGET_NAMES, TARGETS, block_kept, block_mean_fill, label_floors, pano_gradient,
                                           scaled_lenses, target_case, target_image, target_lenses)
from tests.test_gpu_reproject import analytic_image
from tests.test_pano_crop_ref import crop_image
from tests.test_pano_rotate_ref import up_angle_deg

pytestmark = pytest.mark.gpu
FILL = 0.25


def gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


@functools.lru_cache(None)
def pano_of(hw, dtype):
    """the analytic image of DESIGN.md section 17 as a panorama: float32 in [0, 1], or its uint8 rounding of 255 x; read only"""
    img = analytic_image(*hw)
    return img if dtype == "f32" else np.clip(np.floor(255.0 * img.astype(np.float64) + 0.5), 0, 255).astype(np.uint8)


def fill_of(dtype):
    return FILL if dtype == "f32" else 37.0


@functools.lru_cache(None)
def run_target(name, dtype, pano_hw, samples=1, scale=1):
    """one frame of a target (at `scale` times its size) out of one panorama: (image, up, lat, mask) as numpy; read only"""
    from perspectivefields_amd import panorama_to_fisheye

    (H, W), kind, _ = TARGETS[name]
    img, up, lat, mask = panorama_to_fisheye(gpu(pano_of(pano_hw, dtype)), scaled_lenses(name, scale), height=scale * H, width=scale * W, projection=KIND_NAMES[kind],
                                             fill=fill_of(dtype), return_mask=True, fields=True, samples=samples)
    assert img.shape == (1, scale * H, scale * W, 3) and up.shape == (1, 2, scale * H, scale * W) and lat.shape == mask.shape == (1, scale * H, scale * W)
    assert mask.dtype == torch.bool
    return img[0].cpu().numpy(), up[0].cpu().numpy(), lat[0].cpu().numpy(), mask[0].cpu().numpy()


# ---------------------------------------------------------------- the mask, the images, the labels
@pytest.mark.parametrize("pano_hw", [tuple(p) for p in PANOS])
def test_mask_and_float32_image_match_the_fp64_reference(pano_hw):
    """the mask equals the reference's on every kept pixel, at most 1 % of a frame is left out, a pixel outside the mask holds `fill`, and every kept
    pixel inside it is within 2 x (float32 floor of the panorama coordinate of the case) x (largest gradient of the panorama) + 1e-6 of the fp64
    image; the floor is that of the numpy float32 evaluation of the same case"""
    pano = pano_of(pano_hw, "f32")
    grad = pano_gradient(pano)
    for name in TARGET_NAMES:
        (H, W), kind, _ = TARGETS[name]
        case = target_case(name, pano_hw)
        ref, ref_mask = target_image(pano.astype(np.float64), target_lenses(name), kind, H, W, fill=FILL)
        img, _, _, mask = run_target(name, "f32", pano_hw)
        kept = case["kept"]
        assert 1.0 - kept.mean() <= 0.01, name
        assert np.array_equal(mask[kept], ref_mask[kept]), name
        assert (img[~mask] == np.float32(FILL)).all(), name
        m = kept & ref_mask
        assert m.any(), name
        err = np.abs(img.astype(np.float64) - ref).max(-1)[m].max()
        allowed = 2.0 * case["e_c"] * grad + 1e-6
        print(f"target {name} ({H} x {W}) out of {pano_hw}: error {err:.3e}, allowed {allowed:.3e}, error / allowed {err / allowed:.3f}, floor {case['e_c']:.3e} px, "
              f"{int((~kept).sum())} pixels left out")
        assert err <= allowed, (name, err, allowed)


@pytest.mark.parametrize("pano_hw", [tuple(p) for p in PANOS])
def test_uint8_within_one_lsb(pano_hw):
    """every kept pixel within 1 LSB of the rounded fp64 value"""
    pano = pano_of(pano_hw, "u8")
    for name in TARGET_NAMES:
        (H, W), kind, _ = TARGETS[name]
        kept = target_case(name, pano_hw)["kept"]
        ref, ref_mask = target_image(pano.astype(np.float64), target_lenses(name), kind, H, W, fill=37.0)
        img, _, _, mask = run_target(name, "u8", pano_hw)
        assert img.dtype == np.uint8 and np.array_equal(mask[kept], ref_mask[kept]) and (img[~mask] == 37).all(), name
        d = np.abs(img.astype(np.float64) - np.clip(np.floor(ref + 0.5), 0, 255)).max(-1)
        assert d[kept].max() <= 1.0, (name, d[kept].max())


def test_labels_match_the_fp64_reference_and_fisheye_fields_gives_their_bits():
    """up angle and latitude error each within 4 x the error of the numpy float32 evaluation of the same case + 1e-5 degrees (the factor covers the
    device's atan2f / asinf / sincosf against numpy's); NaN exactly where the reference has it; fisheye_fields gives the same bits; the labels do
    not depend on the panorama, its type or `samples`"""
    from perspectivefields_amd import fisheye_fields

    for name in TARGET_NAMES:
        (H, W), kind, _ = TARGETS[name]
        case = target_case(name, tuple(PANOS[0]))
        _, up, lat, mask = run_target(name, "f32", tuple(PANOS[0]))
        e_up, e_lat = label_floors(case)
        kept, kept_up = case["kept"], case["kept_up"]
        assert 1.0 - kept_up.mean() <= 0.01, name
        assert np.array_equal(np.isnan(lat)[kept], np.isnan(case["lat"])[kept]) and np.array_equal(np.isnan(lat), ~mask), name
        for k in (0, 1):
            assert np.array_equal(np.isnan(up[k])[kept_up], np.isnan(case["up"][k])[kept_up]), name
        m = kept & (case["owner"] >= 0)
        d_lat = np.abs(lat.astype(np.float64) - case["lat"])[m].max()
        m = kept_up & np.isfinite(case["up"][0])
        d_up = up_angle_deg(up, case["up"])[m].max() if m.any() else 0.0
        print(f"target {name}: up angle {d_up:.3e} degrees, allowed {4 * e_up + 1e-5:.3e}, ratio {d_up / (4 * e_up + 1e-5):.3f}; "
              f"latitude {d_lat:.3e} degrees, allowed {4 * e_lat + 1e-5:.3e}, ratio {d_lat / (4 * e_lat + 1e-5):.3f}")
        assert d_up <= 4 * e_up + 1e-5 and d_lat <= 4 * e_lat + 1e-5, (name, d_up, e_up, d_lat, e_lat)
        f_up, f_lat = fisheye_fields(target_lenses(name), height=H, width=W, projection=KIND_NAMES[kind])
        assert f_up.shape == (1, 2, H, W) and f_lat.shape == (1, H, W)
        assert np.array_equal(f_up[0].cpu().numpy().view(np.int32), up.view(np.int32)) and np.array_equal(f_lat[0].cpu().numpy().view(np.int32), lat.view(np.int32)), name
        for other in (run_target(name, "u8", tuple(PANOS[0])), run_target(name, "f32", tuple(PANOS[1]))):
            assert np.array_equal(other[1].view(np.int32), up.view(np.int32)) and np.array_equal(other[2].view(np.int32), lat.view(np.int32)), name


def test_a_turned_lens_has_the_same_label_bits():
    """the yaw of a lens does not enter the labels, nor their bits"""
    from perspectivefields_amd import fisheye_fields

    for name in ("B", "C"):
        (H, W), kind, _ = TARGETS[name]
        lenses = target_lenses(name)
        turned = lenses.copy()
        turned[:, 2] += np.array([1.234, -2.5])
        one, other = fisheye_fields(lenses, height=H, width=W, projection=KIND_NAMES[kind]), fisheye_fields(turned, height=H, width=W, projection=KIND_NAMES[kind])
        assert torch.equal(_bits(one[0]), _bits(other[0])) and torch.equal(_bits(one[1]), _bits(other[1]))


# ---------------------------------------------------------------- closure
def test_closure_panorama_to_dual_frame_to_panorama_and_to_a_view():
    """a 64 x 128 float32 panorama of directions (value range 2) is cut into rig B's dual frame at 96 x 192 and read back by fisheye_to_panorama: over
    the covered pixels no worse than the same chain in fp64 plus 4e-5; and crop_fisheye of that frame against crop_panorama of the panorama for a
    view wholly inside lens 0, under the same rule"""
    from perspectivefields_amd import crop_fisheye, fisheye_to_panorama, panorama_to_fisheye

    src = smooth_panorama(64, 128)
    (_, _), kind, _ = TARGETS["B"]
    lenses = scaled_lenses("B", 4)
    frame = panorama_to_fisheye(gpu(src), lenses, height=96, width=192, projection=KIND_NAMES[kind])
    assert frame.shape == (1, 96, 192, 3) and frame.dtype == torch.float32
    frame64, _ = target_image(src.astype(np.float64), lenses, kind, 96, 192)

    back, mask = fisheye_to_panorama(frame[0], lenses, height=64, width=128, projection=KIND_NAMES[kind], return_mask=True)
    back, mask = back[0].cpu().numpy().astype(np.float64), mask[0].cpu().numpy()
    ref, ref_mask = frame_to_pano(frame64, list(lenses), kind, (0.0, 0.0, 0.0), False, 64, 128)
    m = mask & ref_mask
    assert ref_mask.mean() > 0.95 and m.mean() > 0.95
    e_gpu, e_ref = np.abs(back - src)[m].max(), np.abs(ref - src)[m].max()
    print(f"closure panorama -> dual frame -> panorama: GPU error {e_gpu:.6f}, fp64 chain {e_ref:.6f}")
    assert e_ref <= 0.05 and e_gpu <= e_ref + 4e-5

    cam = (0.0, 4.0, 10.0, 0.8, 0.0, 0.0, 0.0)   # along the axis of lens 0, 64 degrees of field: inside the part of the lens with weight 1
    view, _, _, vmask = crop_fisheye(frame[0], lenses, cam[0], cam[1], cam[3], yaw=cam[2], height=40, width=40, projection=KIND_NAMES[kind], fields=False, return_mask=True)
    assert bool(vmask.all())
    want = crop_image(src.astype(np.float64), view_rad(cam), 40, 40)
    ref_view, ref_vmask = crop_frame(frame64, list(lenses), kind, view_rad(cam), 40, 40)
    assert ref_vmask.all()
    e_gpu, e_ref = np.abs(view[0].cpu().numpy().astype(np.float64) - want).max(), np.abs(ref_view - want).max()
    print(f"closure panorama -> dual frame -> view against the panorama's crop: GPU error {e_gpu:.6f}, fp64 chain {e_ref:.6f}")
    assert e_ref <= 0.05 and e_gpu <= e_ref + 4e-5


# ---------------------------------------------------------------- supersampling
@pytest.mark.parametrize("S", SS_SAMPLES)
@pytest.mark.parametrize("dtype", ["f32", "u8"])
def test_supersampling_is_the_block_mean_of_the_fine_call(dtype, S):
    """samples=S equals the S x S block mean, over the valid sub-pixels (the fine call's mask), of the frame at S times the size (F, Cx, Cy times S)
    with samples=1: float32 within 1e-5 of the value range (1), uint8 within 1 LSB, the mask is the "any" of the block, and the labels are those of
    samples=1, bit for bit.  The two calls evaluate the same points with different float32 roundings, so an output pixel is compared where all of
    its sub-pixels are kept pixels of the fine case; at most 1 % of a frame is left out, asserted here and on the reference alone"""
    tol = 1e-5 if dtype == "f32" else 1.0
    pano_hw = tuple(PANOS[0])
    for name in SS_TARGETS:
        out = TARGETS[name][0]
        f_img, _, _, f_mask = run_target(name, dtype, pano_hw, 1, S)
        img, up, lat, mask = run_target(name, dtype, pano_hw, S)
        kept = block_kept(target_case(name, pano_hw, S)["kept"], out, S)
        assert 1.0 - kept.mean() <= 0.01, (name, S)
        want, want_any = block_mean_fill(f_img.astype(np.float64), f_mask, S, fill_of(dtype))
        assert np.array_equal(mask[kept], want_any[kept]) and (img[~mask] == np.asarray(fill_of(dtype), img.dtype)).all(), (name, S)
        d = np.abs(img.astype(np.float64) - want).max(-1)[kept].max()
        print(f"target {name}, samples = {S}, {dtype}: largest difference from the block mean {d:.3e} (allowed {tol:g})")
        assert d <= tol, (name, S, d)
        _, up1, lat1, _ = run_target(name, dtype, pano_hw)
        assert np.array_equal(up.view(np.int32), up1.view(np.int32)) and np.array_equal(lat.view(np.int32), lat1.view(np.int32)), (name, S)


# ---------------------------------------------------------------- batching, determinism, stores
def batch_lenses(n, rng):
    """n frames of 24 x 48: rig B's two lenses turned at random, every third frame with its first lens alone"""
    table = np.repeat(target_lenses("B")[None], n, axis=0)
    table[:, :, :3] += rng.uniform(-0.5, 0.5, (n, 2, 3))
    table[::3, 1] = OFF
    return table


@pytest.mark.parametrize("dtype", ["u8", "f32"])
def test_batching_and_determinism(dtype):
    """33 frames out of two panoramas (two launches): the same bits repeated, permuted and alone on both sides of the launch boundary"""
    from perspectivefields_amd import panorama_to_fisheye

    rng = np.random.default_rng(8)
    panos = [gpu(pano_of((32, 64), dtype)), gpu(pano_of((17, 40), dtype))]
    n = 33
    table = batch_lenses(n, rng)
    index = [int(i) for i in rng.integers(0, 2, n)]
    run = lambda o: panorama_to_fisheye(panos, table[o], height=24, width=48, pano_index=[index[i] for i in o], samples=2, fill=3.0, return_mask=True, fields=True)
    every = list(range(n))
    first, again = run(every), run(every)
    assert first[0].shape == (n, 24, 48, 3) and first[0].dtype == panos[0].dtype and bool(first[3].any()) and not bool(first[3].all())
    perm = [int(i) for i in rng.permutation(n)]
    permuted = run(perm)
    for k in range(4):   # the image, up, the latitude and the mask
        assert torch.equal(_bits(first[k]), _bits(again[k])) and torch.equal(_bits(first[k][perm]), _bits(permuted[k])), k
        for i in (0, 31, 32):
            assert torch.equal(_bits(first[k][i]), _bits(run([i])[k][0])), (k, i)
        assert torch.equal(_bits(first[k][[3, 4, 32]]), _bits(run([3, 4, 32])[k])), k


def test_fisheye_fields_crosses_the_launch_boundary():
    from perspectivefields_amd import fisheye_fields

    table = batch_lenses(33, np.random.default_rng(9))
    up, lat = fisheye_fields(table, height=24, width=48)
    assert up.shape == (33, 2, 24, 48) and lat.shape == (33, 24, 48)
    for i in (0, 31, 32):
        u, l = fisheye_fields(table[i], height=24, width=48)
        assert torch.equal(_bits(up[i]), _bits(u[0])) and torch.equal(_bits(lat[i]), _bits(l[0])), i


@pytest.mark.parametrize("dtype", [torch.uint8, torch.float32])
def test_unaligned_outputs_take_the_scalar_stores_and_give_the_same_bits(dtype):
    """the Python functions allocate aligned outputs; storage that is not aligned reaches the entry points only through the C interface: 24 x 48 into
    aligned outputs (vector stores) against the same call into an image shifted by one element, into a mask shifted by one byte, into labels shifted
    by one element, and nothing written around them"""
    from perspectivefields_amd import panorama_to_fisheye
    from perspectivefields_amd.engine import _check, load_library

    H, W, B = 24, 48, 3
    n = H * W
    name = "u8" if dtype == torch.uint8 else "f32"
    pano = gpu(pano_of((32, 64), name))
    table = batch_lenses(B, np.random.default_rng(10))
    want = panorama_to_fisheye(pano, table, height=H, width=W, pano_index=[0] * B, samples=2, fill=5.0, return_mask=True, fields=True)
    lib = load_library()
    lens = gpu(table.astype(np.float32))
    head = (0, 1, (ctypes.c_void_p * 1)(pano.data_ptr()), (ctypes.c_int32 * 2)(32, 64), 0 if dtype == torch.uint8 else 1, 0, B, (ctypes.c_int32 * B)(*([0] * B)),
            lens.data_ptr(), H, W, 5.0)
    for s_img, s_mask, s_lab in ((0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1)):
        buf = torch.zeros(B * n * 3 + 4, dtype=dtype, device="cuda")
        mbuf = torch.full((B * n + 4,), 9, dtype=torch.uint8, device="cuda")
        ubuf = torch.full((B * n * 2 + 4,), -7.0, dtype=torch.float32, device="cuda")
        lbuf = torch.full((B * n + 4,), -7.0, dtype=torch.float32, device="cuda")
        out, valid = buf[s_img:s_img + B * n * 3], mbuf[s_mask:s_mask + B * n]
        up, lat = ubuf[s_lab:s_lab + B * n * 2], lbuf[s_lab:s_lab + B * n]
        assert (out.data_ptr() % (4 if dtype == torch.uint8 else 16) != 0) == bool(s_img) and (valid.data_ptr() % 4 != 0) == bool(s_mask)
        assert (up.data_ptr() % 16 != 0) == bool(s_lab) and (lat.data_ptr() % 16 != 0) == bool(s_lab)
        _check(lib.pf_pano_to_fisheye(*head, out.data_ptr(), valid.data_ptr(), up.data_ptr(), lat.data_ptr(), 2, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)),
               None, "pf_pano_to_fisheye")
        assert torch.equal(_bits(out.reshape(want[0].shape)), _bits(want[0])) and torch.equal(valid.reshape(want[3].shape), want[3].view(torch.uint8))
        assert torch.equal(_bits(up.reshape(want[1].shape)), _bits(want[1])) and torch.equal(_bits(lat.reshape(want[2].shape)), _bits(want[2]))
        assert (buf[:s_img] == 0).all() and (buf[s_img + B * n * 3:] == 0).all() and (mbuf[:s_mask] == 9).all() and (mbuf[s_mask + B * n:] == 9).all()
        assert (ubuf[:s_lab] == -7).all() and (ubuf[s_lab + B * n * 2:] == -7).all() and (lbuf[:s_lab] == -7).all() and (lbuf[s_lab + B * n:] == -7).all()
        if dtype == torch.float32:   # the labels alone, through pf_fisheye_fields
            ubuf.fill_(-7.0)
            lbuf.fill_(-7.0)
            _check(lib.pf_fisheye_fields(0, 0, B, lens.data_ptr(), H, W, up.data_ptr(), lat.data_ptr(), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)),
                   None, "pf_fisheye_fields")
            assert torch.equal(_bits(up.reshape(want[1].shape)), _bits(want[1])) and torch.equal(_bits(lat.reshape(want[2].shape)), _bits(want[2]))
            assert (ubuf[:s_lab] == -7).all() and (ubuf[s_lab + B * n * 2:] == -7).all() and (lbuf[:s_lab] == -7).all() and (lbuf[s_lab + B * n:] == -7).all()


# ---------------------------------------------------------------- non-finite lens entries
@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_a_non_finite_entry_of_lens_1_gives_the_bits_of_lens_0_alone(bad):
    """rig B with a non-finite entry in lens 1: lens 0's half bit for bit, `fill` / 0 / NaN elsewhere"""
    from perspectivefields_amd import panorama_to_fisheye

    (H, W), kind, _ = TARGETS["B"]
    lenses = target_lenses("B")
    for dtype in ("u8", "f32"):
        pano = gpu(pano_of((32, 64), dtype))
        run = lambda l: panorama_to_fisheye(pano, l, height=H, width=W, fill=2.0, samples=2, return_mask=True, fields=True)
        alone, whole = run(np.stack([lenses[0], OFF])), run(lenses)
        half = alone[3][0]
        assert bool(half.any()) and not bool(half[:, W // 2 + 1:].any()) and bool(whole[3][0][:, W // 2 + 1:].any())
        assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(alone, run(lenses[0])))   # one row: the second lens is switched off
        assert (alone[0][0][~half] == 2).all() and bool(torch.isnan(alone[1][0][:, ~half]).all()) and bool(torch.isnan(alone[2][0][~half]).all())
        assert torch.equal(_bits(whole[0][0][half]), _bits(alone[0][0][half])) and torch.equal(_bits(whole[2][0][half]), _bits(alone[2][0][half]))
        for k in range(12):
            broken = lenses.copy()
            broken[1, k] = bad
            got = run(broken)
            assert all(torch.equal(_bits(g), _bits(a)) for g, a in zip(got, alone)), (dtype, k)


def test_a_nan_in_lens_0_leaves_lens_1_and_the_other_outputs_alone():
    from perspectivefields_amd import panorama_to_fisheye

    (H, W), kind, _ = TARGETS["B"]
    lenses = target_lenses("B")
    pano = gpu(pano_of((32, 64), "f32"))
    run = lambda table: panorama_to_fisheye(pano, table, height=H, width=W, pano_index=[0] * len(table), fill=2.0, return_mask=True, fields=True)
    good = run(np.stack([lenses, lenses, lenses]))
    second = run(np.stack([OFF, lenses[1]])[None])
    for k in range(12):
        broken = lenses.copy()
        broken[0, k] = np.nan
        got = run(np.stack([lenses, broken, lenses]))
        for j in range(4):
            assert torch.equal(_bits(got[j][[0, 2]]), _bits(good[j][[0, 2]])) and torch.equal(_bits(got[j][1]), _bits(second[j][0])), (k, j)
    none = run(np.full((1, 2, 12), np.nan))
    assert (none[0] == 2).all() and not bool(none[3].any()) and bool(torch.isnan(none[1]).all()) and bool(torch.isnan(none[2]).all())
