"""The transport of perspective fields on the GPU (include/pf_hip.h pf_reproject_fields / pf_compose_fields, perspectivefields_amd.reproject_fields /
compose_panorama_fields, PerspectiveFields.rectify(fields=True) / inference_panorama) against the fp64 reference of tests/test_field_transport_ref.py.

Tolerances.  The up angle and the latitude are held to 4 x the error of the same model evaluated in numpy float32 in the same run
(test_field_transport_ref.fp32_floor / composition_floor; the device's sincosf, sqrtf and divisions differ from numpy's by a few ulp, the margin
tests/test_gpu_reproject.py gives its map), on the pixels the reference's `clear` rule keeps (at least 99 %, asserted there), where validity must equal
the reference's.  The entry points write into the middle of a larger buffer filled with a finite sentinel: NaN is a legitimate output here and cannot
be the poison."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests.test_field_transport_ref import (CASES, COMPOSITIONS, LAT_LIMIT, SIZES, TWO_PANOS, composition_floor, composition_inputs, composition_reference,
                                            field_errors_deg, fp32_floor, pair_inputs, pair_reference, reproject_fields_model)
from tests.test_pano_crop_ref import labels
from tests.test_reproject_ref import theta_rad

pytestmark = pytest.mark.gpu

KEYS = ("roll", "pitch", "yaw", "rel_focal", "rel_cx", "rel_cy", "xi")
SENTINEL, MARGIN = -1234.5, 4096   # floats before and after every output; 4096 keeps the 16-byte alignment of the vector stores
BLEND = {"feather": 0, "mean": 1}


def cams(cases, which):
    c = np.asarray([case[which] for case in cases], dtype=np.float64)
    return {k: c[:, i] for i, k in enumerate(KEYS)}


def cams_rad(thetas):
    c = np.asarray(thetas, dtype=np.float64)
    return {k: c[:, i] for i, k in enumerate(KEYS)}


class Guarded:
    """n floats in the middle of a larger sentinel-filled buffer"""

    def __init__(self, shape):
        self.n = int(np.prod(shape))
        self.buf = torch.full((self.n + 2 * MARGIN,), SENTINEL, dtype=torch.float32, device="cuda")
        self.out = self.buf[MARGIN:MARGIN + self.n].view(shape)

    def check(self):
        assert bool((self.buf[:MARGIN] == SENTINEL).all()) and bool((self.buf[MARGIN + self.n:] == SENTINEL).all()), "a store outside the output"
        assert not bool((self.out == SENTINEL).any()), "an output element was not written"
        return self.out.cpu().numpy()


def _sources(ups, lats):
    ups = [torch.from_numpy(np.array(u, dtype=np.float32)).cuda() for u in ups]
    lats = [torch.from_numpy(np.array(l, dtype=np.float32)).cuda() for l in lats]
    n = len(ups)
    hw = (ctypes.c_int32 * (2 * n))(*[v for l in lats for v in l.shape])
    return ups, lats, (ctypes.c_void_p * n)(*[t.data_ptr() for t in ups]), (ctypes.c_void_p * n)(*[t.data_ptr() for t in lats]), hw


def raw_reproject_fields(ups, lats, idx, src, dst, H, W):
    """pf_reproject_fields through ctypes into guarded outputs: (up (B, 2, H, W), lat (B, H, W)) as numpy; cameras (B, 7) in radians"""
    from perspectivefields_amd.engine import _stream_ptr, load_library

    lib = load_library()
    B = len(idx)
    keep = _sources(ups, lats)
    cs, cd = (torch.from_numpy(np.asarray(c, dtype=np.float32).reshape(B, 7)).cuda() for c in (src, dst))
    up, lat = Guarded((B, 2, H, W)), Guarded((B, H, W))
    rc = lib.pf_reproject_fields(0, len(ups), keep[2], keep[3], keep[4], B, (ctypes.c_int32 * B)(*idx), cs.data_ptr(), cd.data_ptr(), H, W, up.out.data_ptr(),
                                 lat.out.data_ptr(), _stream_ptr())
    assert rc == 0, lib.pf_last_error(None).decode()
    torch.cuda.synchronize()
    return up.check(), lat.check()


def raw_compose_fields(ups, lats, pano_idx, thetas, n_pano, Hp, Wp, blend="feather"):
    from perspectivefields_amd.engine import _stream_ptr, load_library

    lib = load_library()
    n = len(ups)
    keep = _sources(ups, lats)
    cam = torch.from_numpy(np.asarray(thetas, dtype=np.float32).reshape(n, 7)).cuda()
    up, lat, wgt = Guarded((n_pano, 2, Hp, Wp)), Guarded((n_pano, Hp, Wp)), Guarded((n_pano, Hp, Wp))
    rc = lib.pf_compose_fields(0, n, keep[2], keep[3], keep[4], (ctypes.c_int32 * n)(*pano_idx), cam.data_ptr(), n_pano, Hp, Wp, BLEND[blend], up.out.data_ptr(),
                               lat.out.data_ptr(), wgt.out.data_ptr(), _stream_ptr())
    assert rc == 0, lib.pf_last_error(None).decode()
    torch.cuda.synchronize()
    return up.check(), lat.check(), wgt.check()


@functools.lru_cache(None)
def gpu_pairs(size):
    """all 60 cases at one size in one call (two launches), every output from its own source"""
    ins = [pair_inputs(k, size) for k in range(len(CASES))]
    H, W = ins[0][4], ins[0][5]
    return raw_reproject_fields([i[0] for i in ins], [i[1] for i in ins], list(range(len(ins))), [i[2] for i in ins], [i[3] for i in ins], H, W)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("size", SIZES)
def test_views_to_views_match_the_fp64_reference(size):
    up, lat = gpu_pairs(size)
    floor = fp32_floor(size)
    worst = np.zeros(2)
    for k in range(len(CASES)):
        ur, lr, near = pair_reference(k, size)
        assert near.mean() <= 0.01
        e_up, e_lat, same = field_errors_deg(up[k], lat[k], ur, lr, ~near)
        assert same, f"case {k}: validity differs from the reference on a kept pixel"
        worst = np.maximum(worst, (e_up, e_lat))
    print(f"views -> views at {size}: GPU up {worst[0]:.3e} deg (fp32 floor {floor[0]:.3e}), latitude {worst[1]:.3e} deg (floor {floor[1]:.3e})")
    assert worst[0] <= 4 * floor[0] and worst[1] <= 4 * floor[1], (worst, floor)


@pytest.mark.parametrize("name", sorted(COMPOSITIONS))
@pytest.mark.parametrize("blend", ["feather", "mean"])
def test_views_to_panorama_match_the_fp64_reference(name, blend):
    ups, lats, thetas, Hp, Wp = composition_inputs(name)
    up, lat, wgt = raw_compose_fields(ups, lats, [0] * len(ups), thetas, 1, Hp, Wp, blend)
    ur, lr, Sr, near = composition_reference(name, blend)
    floor = composition_floor(name, blend)
    assert near.mean() <= 0.01
    e_up, e_lat, same = field_errors_deg(up[0], lat[0], ur, lr, ~near)
    e_S = float(np.abs(wgt[0] - Sr)[~near].max())
    print(f"views -> panorama {name} ({blend}): GPU up {e_up:.3e} deg (floor {floor[0]:.3e}), latitude {e_lat:.3e} deg (floor {floor[1]:.3e}), weight {e_S:.3e} ({floor[2]:.3e})")
    assert same and e_up <= 4 * floor[0] and e_lat <= 4 * floor[1] and e_S <= 4 * floor[2], (e_up, e_lat, e_S, floor)
    assert np.array_equal(wgt[0] > 0, np.isfinite(lat[0]))


def test_bits_do_not_depend_on_the_batch_or_the_run():
    from perspectivefields_amd import reproject_fields

    size = SIZES[1]   # W = 53: the scalar stores
    up, lat = gpu_pairs(size)
    for k in (5, 40):   # one output of each launch of the batch of 60, alone
        u, l, s, d, H, W = pair_inputs(k, size)
        u1, l1 = raw_reproject_fields([u], [l], [0], [s], [d], H, W)
        assert np.array_equal(_bits(u1[0]), _bits(up[k])) and np.array_equal(_bits(l1[0]), _bits(lat[k])), k
    # a batch of 33 from one source through the Python entry point: output 32 is alone in the second launch; and a second run
    u, l, s, d, H, W = pair_inputs(7, SIZES[0])
    tu, tl = torch.from_numpy(u).cuda(), torch.from_numpy(l).cuda()
    many = cams([CASES[k] for k in range(33)], 1)
    src = {k: float(v) for k, v in zip(KEYS, CASES[7][0])}
    bu, bl = reproject_fields(tu, tl, src, many, height=H, width=W)
    assert bu.shape == (33, 2, H, W) and bl.shape == (33, H, W) and bu.dtype == torch.float32
    for k in (0, 31, 32):
        ou, ol = reproject_fields(tu, tl, src, {key: float(many[key][k]) for key in KEYS}, height=H, width=W)
        assert np.array_equal(_bits(ou[0].cpu().numpy()), _bits(bu[k].cpu().numpy())) and np.array_equal(_bits(ol[0].cpu().numpy()), _bits(bl[k].cpu().numpy())), k
    bu2, bl2 = reproject_fields(tu, tl, src, many, height=H, width=W)
    assert np.array_equal(_bits(bu2.cpu().numpy()), _bits(bu.cpu().numpy())) and np.array_equal(_bits(bl2.cpu().numpy()), _bits(bl.cpu().numpy()))
    # the Python entry point gives the bits of the raw one (case 7 of the batch of 60)
    ou, ol = reproject_fields(tu, tl, src, {k: float(v) for k, v in zip(KEYS, CASES[7][1])}, height=H, width=W)
    r_up, r_lat = gpu_pairs(SIZES[0])
    assert np.array_equal(_bits(ou[0].cpu().numpy()), _bits(r_up[7])) and np.array_equal(_bits(ol[0].cpu().numpy()), _bits(r_lat[7]))


def test_non_finite_parameters_and_an_all_nan_source():
    u, l, s, d, H, W = pair_inputs(3, SIZES[0])
    bad = (s[0], np.nan) + tuple(s[2:])
    inf_f = tuple(d[:3]) + (np.inf,) + tuple(d[4:])
    up, lat = raw_reproject_fields([u, np.full_like(u, np.nan)], [l, np.full_like(l, np.nan)], [0, 0, 0, 1], [s, bad, s, s], [d, d, inf_f, d], H, W)
    good = gpu_pairs(SIZES[0])
    assert np.array_equal(_bits(up[0]), _bits(good[0][3])) and np.array_equal(_bits(lat[0]), _bits(good[1][3]))
    assert np.isfinite(lat[0]).any() and not np.isfinite(up[1:]).any() and not np.isfinite(lat[1:]).any()


def test_composition_batches_and_a_view_with_nan_parameters():
    from perspectivefields_amd import compose_panorama_fields

    name, idx, n_pano = TWO_PANOS
    ups, lats, thetas, Hp, Wp = composition_inputs(name)
    one = raw_compose_fields(ups, lats, [0] * 5, thetas, 1, Hp, Wp)
    two = raw_compose_fields(ups, lats, list(idx), thetas, n_pano, Hp, Wp)
    for a, b in zip(one, two):
        assert np.array_equal(_bits(a[0]), _bits(b[0]))
    assert not np.isfinite(two[0][1]).any() and not np.isfinite(two[1][1]).any() and (two[2][1] == 0).all()   # the panorama without a view
    # seven panoramas of five views each: 35 views, two launches; every panorama has the bits of the one alone
    seven = raw_compose_fields(ups * 7, lats * 7, [p for p in range(7) for _ in range(5)], thetas * 7, 7, Hp, Wp)
    for p in range(7):
        for a, b in zip(one, seven):
            assert np.array_equal(_bits(a[0]), _bits(b[p])), p
    # one view with NaN parameters leaves every other bit unchanged
    bad = list(thetas)
    bad[2] = (np.nan,) + tuple(bad[2][1:])
    with_nan = raw_compose_fields(ups, lats, [0] * 5, bad, 1, Hp, Wp)
    without = raw_compose_fields(ups[:2] + ups[3:], lats[:2] + lats[3:], [0] * 4, thetas[:2] + thetas[3:], 1, Hp, Wp)
    for a, b in zip(with_nan, without):
        assert np.array_equal(_bits(a), _bits(b))
    assert not np.array_equal(_bits(one[2]), _bits(without[2]))
    # the Python entry point: the same bits, pano_index unsorted, and the weight on request
    t_up, t_lat = [torch.from_numpy(np.array(u)).cuda() for u in ups], [torch.from_numpy(np.array(l)).cuda() for l in lats]
    pu, pl, pw = compose_panorama_fields(t_up, t_lat, cams_rad(thetas), height=Hp, width=Wp, mode="rad", return_weight=True)
    assert np.array_equal(_bits(pu.cpu().numpy()), _bits(one[0])) and np.array_equal(_bits(pl.cpu().numpy()), _bits(one[1])) and np.array_equal(pw.cpu().numpy(), one[2])
    order = [3, 0, 4, 1, 2]   # views of panorama 1 first: sorted stably on the host
    qu, ql = compose_panorama_fields([t_up[i] for i in order], [t_lat[i] for i in order], cams_rad([thetas[i] for i in order]), height=Hp, width=Wp, mode="rad",
                                     pano_index=[1, 0, 1, 0, 0], n_pano=3)
    ref0 = raw_compose_fields([ups[i] for i in (0, 1, 2)], [lats[i] for i in (0, 1, 2)], [0] * 3, [thetas[i] for i in (0, 1, 2)], 1, Hp, Wp)
    ref1 = raw_compose_fields([ups[i] for i in (3, 4)], [lats[i] for i in (3, 4)], [0] * 2, [thetas[i] for i in (3, 4)], 1, Hp, Wp)
    assert qu.shape == (3, 2, Hp, Wp) and np.array_equal(_bits(qu[0].cpu().numpy()), _bits(ref0[0][0])) and np.array_equal(_bits(ql[1].cpu().numpy()), _bits(ref1[1][0]))
    assert not torch.isfinite(ql[2]).any()


@pytest.mark.parametrize("k", [0, 17, 32])
def test_device_only_chain_with_the_panorama_crop(k):
    """crop_panorama's labels of the source camera, transported, against crop_panorama's labels of the destination camera: no host data in between.
    Tolerance: the reference's closed-loop error for the pair, computed here, plus 4 x the fp32 floor"""
    from perspectivefields_amd import crop_panorama, reproject_fields

    size = SIZES[0]
    Hs, Ws, H, W = size
    src, dst = ({key: float(v) for key, v in zip(KEYS, CASES[k][w])} for w in (0, 1))
    pano = torch.zeros((16, 32, 3), dtype=torch.uint8, device="cuda")
    crop = lambda c, h, w: crop_panorama(pano, c["roll"], c["pitch"], c["rel_focal"], c["rel_cx"], c["rel_cy"], yaw=c["yaw"], xi=c["xi"], height=h, width=w)[1:]
    up_s, lat_s = crop(src, Hs, Ws)
    up_d, lat_d = crop(dst, H, W)
    got_up, got_lat = reproject_fields(up_s, lat_s, src, dst, height=H, width=W)
    s, d = theta_rad(*CASES[k][0]), theta_rad(*CASES[k][1])
    fu, fl = labels(s, Hs, Ws)
    tu, tl = labels(d, H, W)
    mu, ml, near = reproject_fields_model(fu, fl, s, d, H, W)
    keep = ~near & (np.abs(tl) <= LAT_LIMIT) & np.isfinite(ml)
    ref = field_errors_deg(mu, ml, tu, tl, keep)
    gpu = field_errors_deg(got_up[0].cpu().numpy(), got_lat[0].cpu().numpy(), up_d[0].cpu().numpy().astype(np.float64), lat_d[0].cpu().numpy().astype(np.float64), keep)
    floor = fp32_floor(size)
    print(f"chain, case {k}: GPU up {gpu[0]:.4f} deg, latitude {gpu[1]:.4f} deg; reference closed loop {ref[0]:.4f}, {ref[1]:.4f}")
    assert keep.sum() >= 200 and gpu[2]
    assert gpu[0] <= ref[0] + 4 * floor[0] and gpu[1] <= ref[1] + 4 * floor[1], (gpu, ref, floor)


def test_rectify_with_fields_is_reproject_fields():
    from perspectivefields_amd import PerspectiveFields, fields_from_params, reproject_fields, reproject_image

    H, W = 61, 83
    m = PerspectiveFields.__new__(PerspectiveFields)   # rectify reads nothing of the model
    imgs = torch.from_numpy(np.random.default_rng(3).integers(0, 256, (2, H, W, 3), dtype=np.uint8)).cuda()
    par = [(20.0, 15.0, 0.7, 0.4), (-10.0, -25.0, 0.9, 0.0)]
    preds = []
    for r, p, f, xi in par:
        up, lat = fields_from_params(r, p, f, height=H, width=W, xi=xi, device="cuda")
        preds.append(dict(pred_roll=r, pred_pitch=p, pred_rel_focal=f, pred_xi=xi, pred_gravity_original=up.reshape(2, H, W), pred_latitude_original=lat.reshape(H, W)))
    src = dict(roll=[p[0] for p in par], pitch=[p[1] for p in par], rel_focal=[p[2] for p in par], rel_cx=[0.0, 0.0], rel_cy=[0.0, 0.0], xi=[p[3] for p in par])
    dst = dict(roll=0.0, pitch=src["pitch"], rel_focal=src["rel_focal"], xi=0.0)
    (img, valid), (up, lat) = PerspectiveFields.rectify(m, imgs, preds, fields=True, return_valid=True, height=40, width=56)
    want_img, want_valid = reproject_image(imgs, src, dst, height=40, width=56, return_valid=True)
    want_up, want_lat = reproject_fields([p["pred_gravity_original"] for p in preds], [p["pred_latitude_original"] for p in preds], src, dst, height=40, width=56)
    assert torch.equal(img, want_img) and torch.equal(valid, want_valid)
    assert up.shape == (2, 2, 40, 56) and torch.equal(up.view(torch.int32), want_up.view(torch.int32)) and torch.equal(lat.view(torch.int32), want_lat.view(torch.int32))
    assert torch.isfinite(lat).float().mean() > 0.5
    # the default is the call as it was; one result dict, the image's size
    assert torch.equal(PerspectiveFields.rectify(m, imgs, preds, height=40, width=56), want_img)
    out, (u1, l1) = PerspectiveFields.rectify(m, imgs[0], preds[0], fields=True, level="full")
    assert out.shape == (1, H, W, 3) and u1.shape == (1, 2, H, W) and l1.shape == (1, H, W)
    # the transported prediction scores against the destination's labels: exact fields in, small errors out
    from perspectivefields_amd import field_errors

    gt_up, gt_lat = fields_from_params(0.0, 0.0, par[0][2], height=H, width=W, device="cuda")
    err = field_errors(u1[0], l1[0], gt_up.reshape(2, H, W), gt_lat.reshape(H, W))
    assert float(err["up_mean_deg"]) <= 1.0 and float(err["lat_mean_deg"]) <= 0.5, err


def test_inference_panorama_is_its_chain_and_feeds_draw_and_errors():
    from perspectivefields_amd import PerspectiveFields, compose_panorama_fields, crop_panorama, draw_perspective_fields, field_errors, panorama_fields

    m = PerspectiveFields("Paramnet-360Cities-edina-centered", weights="synthetic:0").eval().cuda()
    Hp, Wp = 64, 128
    pano = torch.from_numpy(np.random.default_rng(5).integers(0, 256, (Hp, Wp, 3), dtype=np.uint8)).cuda()
    res = m.inference_panorama(pano, n_yaw=4, view_pitch=(-30.0, 30.0), vfov=100.0, view_size=64)
    up, lat, wgt = res["pred_gravity_original"], res["pred_latitude_original"], res["weight"]
    assert up.shape == (2, Hp, Wp) and lat.shape == (Hp, Wp) and wgt.shape == (Hp, Wp) and up.dtype == torch.float32 and up.is_cuda
    f = 0.5 / np.tan(np.radians(50.0))
    cam = dict(roll=0.0, pitch=[-30.0] * 4 + [30.0] * 4, yaw=[0.0, 90.0, 180.0, 270.0] * 2, rel_focal=f)
    crops = crop_panorama(pano, 0.0, cam["pitch"], f, yaw=cam["yaw"], height=64, width=64, fields=False)[0]
    preds = m.inference_batch(list(crops))
    cu, cl, cw = compose_panorama_fields([p["pred_gravity_original"] for p in preds], [p["pred_latitude_original"] for p in preds], cam, height=Hp, width=Wp,
                                         return_weight=True)
    assert torch.equal(up.view(torch.int32), cu[0].view(torch.int32)) and torch.equal(lat.view(torch.int32), cl[0].view(torch.int32)) and torch.equal(wgt, cw[0])
    assert bool((wgt > 0).any()) and torch.equal(wgt > 0, torch.isfinite(lat))
    drawn = draw_perspective_fields(pano, up, lat)
    assert drawn.shape[-3:] == (Hp, Wp, 3)
    gt_up, gt_lat = panorama_fields(0.0, 0.0, height=Hp, width=Wp)
    err = field_errors(up, lat, gt_up[0], gt_lat[0])
    assert np.isfinite(float(err["up_mean_deg"])) and np.isfinite(float(err["lat_mean_deg"]))
    small = m.inference_panorama(pano.float(), n_yaw=3, view_pitch=0.0, view_size=32, height=16, width=32, blend="mean")
    assert small["pred_latitude_original"].shape == (16, 32)
