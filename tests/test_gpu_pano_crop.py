"""Panorama crops on the GPU (include/pf_hip.h pf_pano_crop, perspectivefields_amd.crop_panorama) against the fp64 reference of
tests/test_pano_crop_ref.py: geometry on a panorama of unit vectors, the uint8 path, the labels (bit-identical to fields_from_params
at xi = 0), batch invariance, a camera-fit round trip, CUDA uint8 tensors as inference_batch input, and the chain end to end."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

from tests.test_pano_crop_ref import crop_image, labels, pixel_rays, sample_coords

pytestmark = pytest.mark.gpu


def focal_of_vfov(vfov_deg):
    return 0.5 / np.tan(np.radians(vfov_deg) / 2)


def theta_rad(roll, pitch, yaw, f, cx, cy, xi):
    return (np.radians(roll), np.radians(pitch), np.radians(yaw), f, cx, cy, xi)


def crop(pano, cases, H, W, **kw):
    """cases: [(roll, pitch, yaw [deg], rel_focal, rel_cx, rel_cy, xi)] -> crop_panorama on all of them at once"""
    from perspectivefields_amd import crop_panorama

    c = np.asarray(cases, dtype=np.float64)
    return crop_panorama(pano, c[:, 0], c[:, 1], c[:, 3], c[:, 4], c[:, 5], yaw=c[:, 2], xi=c[:, 6], height=H, width=W, **kw)


def direction_panorama(Hp, Wp):
    """float32 (Hp, Wp, 3): each pixel holds the world unit vector of its centre's (lat, lon)"""
    lon = ((np.arange(Wp) + 0.5) / Wp - 0.5) * 2 * np.pi
    lat = (0.5 - (np.arange(Hp) + 0.5) / Hp) * np.pi
    lat, lon = np.meshgrid(lat, lon, indexing="ij")
    return np.stack([np.cos(lat) * np.sin(lon), -np.sin(lat), np.cos(lat) * np.cos(lon)], -1)


def clear_of_the_no_ray_circle(th, H, W, linspace=False):
    """pixels whose disc (pf_pano_crop) is not within a hair of 0: fp32 and fp64 may put those on either side"""
    F, Cx, Cy = th[3] * H, (th[4] + 0.5) * W, (th[5] + 0.5) * H
    a = np.arange(W)[None, :] * (W / max(W - 1, 1)) if linspace else np.arange(W)[None, :] + 0.5
    b = np.arange(H)[:, None] * (H / max(H - 1, 1)) if linspace else np.arange(H)[:, None] + 0.5
    x, y = (a - Cx) / F, (b - Cy) / F
    return np.abs(1 + (1 - th[6] ** 2) * (x * x + y * y)) > 1e-4


GEOM_CASES = [(roll, pitch, yaw, focal_of_vfov(vfov), cx, cy, xi)
              for k, (pitch, yaw, xi) in enumerate(itertools.product((-80.0, -35.0, 0.0, 50.0, 80.0), (-180.0, -70.0, 0.0, 110.0, 180.0), (0.0, 0.5, 1.2)))
              for roll, vfov, (cx, cy) in [((-30.0, 0.0, 25.0)[k % 3], (40.0, 95.0)[k % 2], ((0.0, 0.0), (0.1, -0.08))[(k // 2) % 2])]]


@pytest.mark.parametrize("Hp,Wp", [(1024, 2048), (777, 1555)])
def test_geometry_on_a_panorama_of_directions(Hp, Wp):
    H, W = 40, 56
    pano = direction_panorama(Hp, Wp)
    img, _, _ = crop(torch.from_numpy(pano).float().cuda(), GEOM_CASES, H, W, fields=False)
    img = img.cpu().numpy().astype(np.float64)
    worst = []
    for k, c in enumerate(GEOM_CASES):
        th = theta_rad(*c)
        u, v, Xw, ok = sample_coords(th, H, W, Hp, Wp)
        yaw = th[2]
        lat = -np.arctan2(Xw[..., 1], np.hypot(Xw[..., 0], Xw[..., 2]))
        lon = np.arctan2(Xw[..., 0], Xw[..., 2]) + yaw
        ref = np.stack([np.cos(lat) * np.sin(lon), -np.sin(lat), np.cos(lat) * np.cos(lon)], -1)
        clear = clear_of_the_no_ray_circle(th, H, W)
        use = ok & clear & (np.abs(lat) < np.pi / 2 - np.pi / Hp)
        s = img[k][use]
        cosang = (s * ref[use]).sum(-1) / np.linalg.norm(s, axis=-1)
        ang = np.degrees(np.arccos(np.clip(cosang, -1, 1)))
        worst.append((float(ang.max()) if ang.size else 0.0, c))
        assert not img[k][~ok & clear].any(), c
    worst.sort(key=lambda t: -t[0])
    assert worst[0][0] <= 2e-3, worst[:4]


def test_uint8_path_within_one_lsb():
    rng = np.random.default_rng(3)
    pano = rng.integers(0, 256, (300, 611, 3), dtype=np.uint8)
    cases = [(0.0, 0.0, 0.0, 0.6, 0.0, 0.0, 0.0), (20.0, -40.0, 179.9, 0.35, 0.05, 0.02, 0.0), (-10.0, 85.0, -120.0, 0.9, 0.0, 0.0, 0.5),
             (5.0, 10.0, 180.0, 0.3, 0.0, 0.0, 1.2), (0.0, -88.0, 30.0, 0.25, -0.1, 0.1, 0.8)]
    for H, W in ((37, 53), (48, 64)):
        img, _, _ = crop(torch.from_numpy(pano).cuda(), cases, H, W, fields=False)
        img = img.cpu().numpy()
        assert img.dtype == np.uint8
        for k, c in enumerate(cases):
            ref = crop_image(pano, theta_rad(*c), H, W)
            clear = clear_of_the_no_ray_circle(theta_rad(*c), H, W)
            assert np.abs(img[k].astype(np.float64) - ref)[clear].max() <= 1.0, (c, H, W)


LABEL_CASES = [(10.0, 25.0, 0.0, 0.8, 0.0, 0.0), (-35.0, 0.0, 30.0, 1.2, 0.0, 0.0), (5.0, -60.0, -90.0, 0.45, 0.07, -0.05),
               (0.0, 0.0, 0.0, 0.9, -0.1, 0.1), (40.0, 70.0, 180.0, 2.0, -0.1, 0.08)]


@pytest.mark.parametrize("H,W", [(48, 64), (31, 47), (1, 17), (19, 1)])
def test_pinhole_labels_are_bit_identical_to_fields_from_params(H, W):
    from perspectivefields_amd import fields_from_params

    pano = torch.zeros((16, 32, 3), dtype=torch.uint8, device="cuda")
    cases = [(r, p, y, f, cx, cy, 0.0) for r, p, y, f, cx, cy in LABEL_CASES]
    _, up, lat = crop(pano, cases, H, W)
    for k, (r, p, _, f, cx, cy, _) in enumerate(cases):
        up_f, lat_f = fields_from_params(r, p, f, cx, cy, H, W)
        assert torch.equal(up[k], up_f) and torch.equal(lat[k], lat_f), (cases[k], H, W)


@pytest.mark.parametrize("xi", [0.3, 0.8, 1.2, 1.6])
def test_usm_labels_match_the_fp64_reference(xi):
    H, W = 45, 60
    pano = torch.full((16, 32, 3), 7, dtype=torch.uint8, device="cuda")
    cases = [(r, p, y, f * 0.6, cx, cy, xi) for r, p, y, f, cx, cy in LABEL_CASES]
    img, up, lat = crop(pano, cases, H, W)
    img, up, lat = img.cpu().numpy(), up.cpu().numpy().astype(np.float64), lat.cpu().numpy().astype(np.float64)
    for k, c in enumerate(cases):
        th = theta_rad(*c)
        up_r, lat_r = labels(th, H, W)
        _, ok = pixel_rays(th, H, W)
        clear = clear_of_the_no_ray_circle(th, H, W)
        assert np.array_equal(np.isnan(up[k, 0])[clear], ~ok[clear]) and np.array_equal(np.isnan(up[k, 1])[clear], ~ok[clear]), c
        assert (img[k][~ok & clear] == 0).all() and (img[k][ok & clear] == 7).all(), c
        m = ok & clear
        cos = (up[k][:, m] * up_r[:, m]).sum(0)
        assert (1 - cos).max() <= 1e-6, (c, (1 - cos).max())
        clear_l = clear_of_the_no_ray_circle(th, H, W, linspace=True)
        ml = np.isfinite(lat_r)
        assert np.array_equal(np.isnan(lat[k])[clear_l], ~ml[clear_l]), c
        lm = ml & clear_l
        assert np.abs(lat[k][lm] - lat_r[lm]).max() <= 2e-3, c
    if xi > 1:
        assert np.isnan(up).any() and np.isnan(lat).any()


def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def test_batch_invariance_over_groups_and_panoramas():
    from perspectivefields_amd import crop_panorama

    rng = np.random.default_rng(9)
    panos = [torch.from_numpy(rng.integers(0, 256, s, dtype=np.uint8)).cuda() for s in ((200, 400, 3), (333, 701, 3))]
    n = 40
    cam = np.stack([rng.uniform(-40, 40, n), rng.uniform(-80, 80, n), rng.uniform(-180, 180, n), rng.uniform(0.3, 1.5, n),
                    rng.uniform(-0.1, 0.1, n), rng.uniform(-0.1, 0.1, n), rng.choice([0.0, 0.0, 0.5, 1.3], n)], 1)
    idx = rng.integers(0, 2, n).tolist()
    H, W = 36, 52
    args = lambda c: (c[:, 0], c[:, 1], c[:, 3], c[:, 4], c[:, 5])
    img, up, lat = crop_panorama(panos, *args(cam), yaw=cam[:, 2], xi=cam[:, 6], height=H, width=W, pano_index=idx)
    again = crop_panorama(panos, *args(cam), yaw=cam[:, 2], xi=cam[:, 6], height=H, width=W, pano_index=idx)
    for a, b in zip((img, up, lat), again):
        assert torch.equal(_bits(a), _bits(b))
    for i in range(n):
        c = cam[i:i + 1]
        one = crop_panorama(panos[idx[i]], *args(c), yaw=c[:, 2], xi=c[:, 6], height=H, width=W)
        for a, b in zip((img[i], up[i], lat[i]), one):
            assert torch.equal(_bits(a), _bits(b[0])), i


def test_fit_recovers_the_crop_parameters():
    from perspectivefields_amd import fit_camera_params

    pano = torch.zeros((64, 128, 3), dtype=torch.uint8, device="cuda")
    cases = [(r, p, y, focal_of_vfov(v), 0.0, 0.0, 0.0) for (r, p, v), y in zip(itertools.product((-30.0, 0.0, 12.0), (-50.0, 0.0, 35.0), (45.0, 90.0)), itertools.cycle((0.0, 90.0, -150.0)))]
    H, W = 240, 320
    _, up, lat = crop(pano, cases, H, W)
    res = fit_camera_params(list(up), list(lat))
    bad = []
    for (r, p, _, f, _, _, _), d in zip(cases, res):
        v = np.degrees(2 * np.arctan(0.5 / f))
        d = {k: float(x) for k, x in d.items()}
        err = (abs(d["pred_roll"] - r), abs(d["pred_pitch"] - p), abs(d["pred_vfov"] - v), abs(d["pred_rel_focal"] - f) / f)
        if max(err[:3]) > 5e-3 or err[3] > 2e-4:
            bad.append(((r, p, v), err))
    assert not bad, bad[:4]


def _same_results(a, b):
    assert len(a) == len(b)
    for ra, rb in zip(a, b):
        assert list(ra) == list(rb)
        for k in ra:
            x, y = ra[k], rb[k]
            if torch.is_tensor(x):
                assert torch.equal(_bits(x.float()), _bits(y.float())), k
            else:
                assert x == y, k


def test_inference_batch_on_device_uint8_tensors():
    from perspectivefields_amd import PerspectiveFields

    m = PerspectiveFields("PersNet_Paramnet-GSV-centered", weights="synthetic:0", precision="fp32").eval().cuda()
    rng = np.random.default_rng(4)
    imgs = [rng.integers(0, 256, s, dtype=np.uint8) for s in ((240, 320, 3), (333, 221, 3), (320, 320, 3), (97, 131, 3))]
    tens = [torch.from_numpy(im).cuda() for im in imgs]
    for fmt in ("BGR", "RGB"):
        m.input_format = fmt
        for dev_resize in (False, True):
            m.device_resize = dev_resize
            _same_results(m.inference_batch(imgs), m.inference_batch(tens))
        _same_results([m.inference(imgs[1])], [m.inference(tens[1])])
    m.input_format = "BGR"
    with pytest.raises(TypeError):
        m.inference_batch([imgs[0], tens[1]])
    with pytest.raises(TypeError):
        m.inference_batch([tens[0].float()])
    with pytest.raises(ValueError):
        m.inference_batch([tens[0].cpu(), tens[1]])
    with pytest.raises(ValueError):
        m.inference_batch([tens[0][..., :2].contiguous()])
    with pytest.raises(ValueError):
        m.inference_batch([tens[0][0]])


@pytest.mark.parametrize("version", ["PersNet-360Cities", "Paramnet-360Cities-edina-centered"])
def test_crop_infer_fit_end_to_end(version):
    from perspectivefields_amd import PerspectiveFields, crop_panorama

    rng = np.random.default_rng(12)
    pano = torch.from_numpy(rng.integers(0, 256, (512, 1024, 3), dtype=np.uint8)).cuda()
    m = PerspectiveFields(version, weights="synthetic:0").eval().cuda()
    B, H, W = 3, 120, 160
    img, up, lat = crop_panorama(pano, [0.0, 10.0, -20.0], [5.0, -30.0, 40.0], [0.8, 1.1, 0.6], yaw=[0.0, 120.0, -170.0], height=H, width=W)
    assert img.shape == (B, H, W, 3) and up.shape == (B, 2, H, W) and lat.shape == (B, H, W)
    preds = m.inference_batch(list(img))
    assert len(preds) == B
    for p in preds:
        assert p["pred_gravity_original"].shape == (2, H, W) and p["pred_latitude_original"].shape == (H, W)
    fits = m.fit_camera(preds)
    assert len(fits) == B and all(d["pred_roll"].shape == () for d in fits)


@pytest.mark.parametrize("dtype", [torch.uint8, torch.float32])
def test_unaligned_outputs_take_the_scalar_stores_and_give_the_same_bits(dtype):
    """crop_panorama allocates its outputs itself, always aligned; storage that is not 16-byte aligned reaches pf_pano_crop only through the
    C interface, called here directly: W = 56 with aligned outputs (vector stores) against the same call into buffers shifted by one element
    (scalar stores).  20 x 56 is less than one 64 x 16 tile across and not a whole number of tiles down; xi = 0 takes the pinhole labels,
    xi > 0 the spherical ones, and at xi = 1.2 with this focal length the corners have no ray (image 0, labels NaN)"""
    from perspectivefields_amd.engine import _check, load_library

    H, W, B = 20, 56, 5
    cases = [(12.0, 20.0, 30.0, 0.6, 0.0, 0.0, 0.0), (-25.0, -40.0, -100.0, 0.9, 0.1, -0.08, 0.0), (8.0, 35.0, 170.0, 0.5, 0.0, 0.0, 0.8),
             (-15.0, -10.0, 60.0, 0.7, -0.05, 0.1, 0.8), (20.0, 5.0, -20.0, 0.3, 0.0, 0.0, 1.2)]
    pano = torch.from_numpy(np.random.default_rng(21).integers(0, 256, (64, 128, 3), dtype=np.uint8)).cuda().to(dtype)
    img, up, lat = crop(pano, cases, H, W)
    assert torch.isnan(lat[4]).any() and not torch.isnan(lat[4]).all() and not torch.isnan(lat[:4]).any()
    cam = torch.from_numpy(np.asarray([theta_rad(*c) for c in cases])).cuda().float().contiguous()
    n = B * H * W
    img2 = torch.zeros(n * 3 + 1, dtype=dtype, device="cuda")
    up2 = torch.zeros(n * 2 + 1, dtype=torch.float32, device="cuda")
    lat2 = torch.zeros(n + 1, dtype=torch.float32, device="cuda")
    _check(load_library().pf_pano_crop(0, 1, (ctypes.c_void_p * 1)(pano.data_ptr()), (ctypes.c_int32 * 2)(64, 128), 0 if dtype == torch.uint8 else 1, B,
                                       (ctypes.c_int32 * B)(*([0] * B)), cam.data_ptr(), H, W, img2[1:].data_ptr(), up2[1:].data_ptr(), lat2[1:].data_ptr(),
                                       ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), None, "pf_pano_crop")
    assert img2[1:].data_ptr() % (4 if dtype == torch.uint8 else 16) != 0
    assert torch.equal(_bits(img2[1:].reshape(img.shape)), _bits(img))
    assert torch.equal(_bits(up2[1:].reshape(up.shape)), _bits(up))
    assert torch.equal(_bits(lat2[1:].reshape(lat.shape)), _bits(lat))
    assert img2[0] == 0 and up2[0] == 0 and lat2[0] == 0   # nothing written in front of the buffers
