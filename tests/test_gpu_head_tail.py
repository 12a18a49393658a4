"""Kernel-level parity (-m gpu) of the kernels at the two ends of the forward -- input normalisation, the regression prediction heads (stand-alone and fused into
conv_fuse_conv1's epilogue), the classification decode, the nearest resize in front of the ParamNet, the ConvNeXt tail and the ParamNet scalars -- each called
through its own C-ABI entry (pf_op_*, include/pf_hip.h) on crafted inputs and compared with an fp64 reference.  Inside pf_forward_* these kernels only ever see what a
synthetic checkpoint feeds them; here they get the inputs their data-dependent branches exist for: the F.normalize eps, the latitude clamp at and beyond +-1, argmax
ties and the "invalid" gravity bin, both roots of the general-vertical-FoV quadratic, the grid-stride loops' second trip.

Every bound below is derived from the number formats (u = 2^-24, the fp32 unit roundoff) or is an existing project tolerance named next to it; none comes from what
the kernels return.  Every test prints its worst error over its bound."""
import math
import warnings

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import pf_oracle
from tests.kernel_bounds import U, _head_bounds, _normalize_bounds, _ratio

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from perspectivefields_amd import ops as _ops

    return _ops


@pytest.fixture(autouse=True)
def _checked_outputs(ops):
    """every test of this module runs inside ops.checked_outputs(): each output an entry point allocates is NaN before its launch, lies
    between guard bands that are compared when the test ends, and no block comes back from the allocator holding an earlier launch's result"""
    with ops.checked_outputs():
        yield


def _rand(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g, dtype=torch.float32) * scale


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _report(what, worst):
    print(f"[head/tail {what}] worst error / bound {worst:.3g}")
    assert worst <= 1.0, f"{what}: error is {worst:.3g} x its bound"


# --------------------------------------------------------------------------------------------------------------- input normalisation
MEAN = np.array([103.53, 116.28, 123.675], dtype=np.float32)
STDS = {"std1": np.ones(3, dtype=np.float32), "std": np.array([57.375, 57.12, 58.395], dtype=np.float32)}


def _prep_check(got, x_f64_nhwc3, std, what):
    """(x - mean) / std in fp64 on the fp32 mean / std; two correctly rounded fp32 operations on exact inputs: |err| <= (2 u + u^2) |ref| <= 3 u |ref|"""
    got = got.cpu().numpy()
    ref = (x_f64_nhwc3 - MEAN.astype(np.float64)) / std.astype(np.float64)
    assert got.shape == ref.shape[:-1] + (4,)
    c3 = got[..., 3]
    assert np.all(c3 == 0) and not np.signbit(c3).any(), f"{what}: channel 3 must be +0"
    return _ratio(np.abs(got[..., :3].astype(np.float64) - ref), 3 * U * np.abs(ref))


@pytest.mark.parametrize("std", list(STDS))
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("H,W", [(1, 1), (5, 7), (33, 65)])
def test_prep_u8(ops, H, W, B, std):
    n = B * H * W
    reps = -(-256 // n)  # enough calls for every channel to take each of 0..255
    seen = [set(), set(), set()]
    worst = 0.0
    for rep in range(reps):
        base = np.arange(n, dtype=np.int64) + rep * n
        x = np.stack([(base * m + o) % 256 for m, o in ((1, 0), (3, 85), (7, 170))], axis=-1).astype(np.uint8).reshape(B, H, W, 3)
        for c in range(3):
            seen[c].update(x[..., c].ravel().tolist())
        got = ops.prep_u8(torch.from_numpy(x).cuda(), MEAN, STDS[std])
        worst = max(worst, _prep_check(got, x.astype(np.float64), STDS[std], f"prep_u8 {B}x{H}x{W} {std}"))
    assert all(len(s) == 256 for s in seen), "the inputs must cover 0..255 in every channel"
    _report(f"prep_u8 B={B} {H}x{W} {std}", worst)


@pytest.mark.parametrize("std", list(STDS))
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("H,W", [(1, 1), (5, 7), (33, 65)])
def test_prep_f32_nchw(ops, H, W, B, std):
    x = _rand((B, 3, H, W), 11 + H, 100.0)
    special = torch.tensor([-1.0e4, 1.0e4, 0.0, -0.0, -255.0, 255.0, float(MEAN[0]), 1.0e-3, -3.5], dtype=torch.float32)
    flat = x.view(-1)
    k = min(flat.numel(), special.numel())
    flat[:k] = special[:k]
    flat[-k:] = special[:k].flip(0)  # the specials in the last channel plane as well
    got = ops.prep_f32_nchw(x.cuda(), MEAN, STDS[std])
    worst = _prep_check(got, x.double().permute(0, 2, 3, 1).numpy(), STDS[std], f"prep_f32_nchw {B}x{H}x{W} {std}")
    _report(f"prep_f32_nchw B={B} {H}x{W} {std}", worst)


# --------------------------------------------------------------------------------------------------------------- regression prediction heads
def _heads_reference(tg, tl, wg, bg, wl, bl):
    """fp64 dot products, their summation bounds 32 u sum_k |a_k w_k|, and the reference outputs"""
    tg, tl, wg, bg, wl, bl = (np.asarray(t, dtype=np.float64) for t in (tg, tl, wg, bg, wl, bl))
    d = tg @ wg.T + bg                       # (..., 2)
    Ed = 32 * U * (np.abs(tg) @ np.abs(wg).T)
    raw_l = tl @ wl[0] + bl[0]               # (...)
    El = 32 * U * (np.abs(tl) @ np.abs(wl[0]))
    n = np.sqrt((d * d).sum(-1))
    g = d / np.maximum(n, 1e-12)[..., None]  # F.normalize
    return d, Ed, n, g, raw_l, El, np.clip(raw_l, -1.0, 1.0)


def _pn_matches(pg, pl, pn):
    B, _, HW = pg.shape
    want = torch.stack((pg[:, 0].reshape(-1), pg[:, 1].reshape(-1), pl.reshape(-1), torch.zeros(B * HW, device=pg.device)), dim=1)
    return torch.equal(pn.view(torch.int32), want.view(torch.int32))


def _check_heads(ops, B, HW, seed, what, explicit=None):
    tg, tl = _rand((B, HW, 32), seed), _rand((B, HW, 32), seed + 1)
    wg, bg = _rand((2, 32), seed + 2, 1.0 / math.sqrt(32)), _rand((2,), seed + 3, 0.1)
    wl, bl = _rand((1, 32), seed + 4, 1.0 / math.sqrt(32)), _rand((1,), seed + 5, 0.1)
    d, Ed, n, g, raw_l, El, lat = _heads_reference(tg, tl, wg, bg, wl, bl)
    left_out = n < 1e-6  # direction ill-conditioned in fp64 too
    print(f"[head/tail {what}] pixels left out of the gravity comparison (fp64 norm < 1e-6): {left_out.mean():.3g}")
    assert left_out.mean() == 0.0, "the random case must not leave any pixel out"
    pg, pl, pn = ops.pred_regression(tg.cuda(), tl.cuda(), wg, bg, wl, bl)
    pg2, pl2, _ = ops.pred_regression(tg.cuda(), tl.cuda(), wg, bg, wl, bl, with_pn=False)
    assert _pn_matches(pg, pl, pn), f"{what}: pn rows must be (g0, g1, lat, 0) with the bits of pg / pl"
    assert torch.equal(pg.view(torch.int32), pg2.view(torch.int32)) and torch.equal(pl.view(torch.int32), pl2.view(torch.int32)), f"{what}: pn = NULL changes pg / pl"
    got_g = pg.cpu().double().numpy().transpose(0, 2, 1)  # (B, HW, 2)
    got_l = pl.cpu().double().numpy()
    err_g, bnd_g = np.abs(got_g - g), _normalize_bounds(d, Ed, n)
    err_l, bnd_l = np.abs(got_l - lat), El + U
    _report(f"{what} gravity", _ratio(err_g, bnd_g))
    _report(f"{what} latitude", _ratio(err_l, bnd_l))
    if explicit is not None:  # named pixels on their own (they are part of the maxima above as well)
        _report(f"{what} gravity, pixels {explicit.start}..", _ratio(err_g[:, explicit], bnd_g[:, explicit]))
        _report(f"{what} latitude, pixels {explicit.start}..", _ratio(err_l[:, explicit], bnd_l[:, explicit]))


@pytest.mark.parametrize("B,HW", [(1, 1), (2, 37), (3, 100)])
def test_pred_regression_random(ops, B, HW):
    _check_heads(ops, B, HW, 100 + HW, f"pred_regression B={B} HW={HW}")


def test_pred_regression_second_grid_trip(ops):
    """8 lanes per pixel and at most 8192 blocks of 256 threads: 262 144 pixels per trip of the grid-stride loop.  HW = 262 144 + 37 takes a second trip for the
    last 37 pixels; every pixel is compared (a superset of a random sample), the last 37 also on their own."""
    HW = 262144 + 37
    _check_heads(ops, 1, HW, 300, "pred_regression second grid trip", explicit=slice(262144, HW))


def test_pred_regression_crafted_pixels(ops):
    """Heads that read channel 0 alone -- gravity raw = (3, 4) a_0, latitude raw = c_0 exactly -- so that the kernel's data-dependent branches get the inputs they
    exist for: the F.normalize eps and the clamp."""
    wg = np.zeros((2, 32), dtype=np.float32)
    wg[0, 0], wg[1, 0] = 3.0, 4.0
    wl = np.zeros((1, 32), dtype=np.float32)
    wl[0, 0] = 1.0
    zero2, zero1 = np.zeros(2, dtype=np.float32), np.zeros(1, dtype=np.float32)
    a0 = np.array([0.0, 1e-13, 1e-12, 1.0, -2.5, 1e-30], dtype=np.float32)   # raw (0, 0); (3e-13, 4e-13): norm 5e-13 < eps; (3e-12, 4e-12); ...; squares underflow
    one_p, one_m = np.float32(1.0 + 2.0 ** -23), np.float32(1.0 - 2.0 ** -24)
    c0 = np.array([-2.0, -1.0, 1.0, 2.0, one_p, -one_p, one_m, -one_m, 0.25, 3e38, -3e38, 0.0], dtype=np.float32)
    HW = max(len(a0), len(c0))
    tg, tl = np.zeros((1, HW, 32), dtype=np.float32), np.zeros((1, HW, 32), dtype=np.float32)
    tg[0, :len(a0), 0] = a0
    tl[0, :len(c0), 0] = c0
    tg[0, :, 1:] = _rand((HW, 31), 7).numpy()  # channels the heads do not read
    pg, pl, pn = ops.pred_regression(torch.from_numpy(tg).cuda(), torch.from_numpy(tl).cuda(), wg, zero2, wl, zero1)
    assert _pn_matches(pg, pl, pn)
    g = pg.cpu().numpy()[0].T.astype(np.float64)  # (HW, 2)
    lat = pl.cpu().numpy()[0]
    assert g[0, 0] == 0.0 and g[0, 1] == 0.0, f"all-zero features and zero bias: exactly (0, 0) wanted, got {g[0]}"
    # fp64 F.normalize of the exact raw vectors (products with 3, 4 are exact in fp64; in fp32 they round: E = u |raw|)
    d = np.stack((3.0 * a0.astype(np.float64), 4.0 * a0.astype(np.float64)), axis=-1)
    n = np.sqrt((d * d).sum(-1))
    ref = d / np.maximum(n, 1e-12)[:, None]
    # the eps itself is 1e-12f in the kernel, 1e-12 in fp64: a relative 1e-12f / 1e-12 - 1 < u where the eps acts; the squares of 1e-30 underflow to 0 in fp32, the
    # eps path then returns raw / 1e-12 as the fp64 reference does
    bound = _normalize_bounds(d, U * np.abs(d), np.maximum(n, 1e-12)) + U
    worst = _ratio(np.abs(g[:len(a0)] - ref), bound)
    print(f"[head/tail pred_regression crafted] eps pixel (3e-13, 4e-13) -> {g[1]} (reference {ref[1]})")
    _report("pred_regression crafted gravity", worst)
    want = np.clip(c0, np.float32(-1.0), np.float32(1.0))  # a single exact product: the clamp must act exactly
    got = lat[:len(c0)]
    assert np.array_equal(_bits(got), _bits(want)), f"clamp: got {got}, want {want}"
    print("[head/tail pred_regression crafted latitude] worst error / bound 0 (bit-equal)")


# --------------------------------------------------------------------------------------------------------------- classification decode
NG, NL = 73, 180


def _check_decode(ops, lg, ll, what, sl=None):
    """bins = torch.argmax on the CPU; latitude exact (-89.5 + k: every term is an fp32 integer or half-integer); gravity within 2^-23 absolute of the oracle's
    decode (one fp32 ulp at 1: two libraries' double-precision cos / sin may round differently).  5 degrees between gravity bins: a wrong bin is off by >= 3.8e-3."""
    ng, nl = lg.shape[1], ll.shape[1]
    dg, dl = ops.decode_cls(lg.cuda(), ll.cuda())
    dg, dl = dg.cpu(), dl.cpu()
    bg, bl_ = lg.argmax(dim=1), ll.argmax(dim=1)  # (B, HW)
    ref_g = pf_oracle.decode_gravity_bins(bg, ng).permute(1, 0, 2)  # (B, 2, HW)
    ref_l = pf_oracle.decode_latitude_bins(bl_, nl).to(torch.float32)
    inval = (bg == ng - 1)[:, None, :].expand_as(dg)
    assert bool((dg[inval] == 0).all()), f"{what}: the invalid bin must decode to exactly (0, 0)"
    if sl is not None:
        dg, dl, ref_g, ref_l = dg[..., sl], dl[..., sl], ref_g[..., sl], ref_l[..., sl]
    assert torch.equal(dl, ref_l), f"{what}: latitude bins differ from torch.argmax at {int((dl != ref_l).sum())} pixels"
    _report(f"{what} gravity", _ratio((dg.double() - ref_g.double()).abs().numpy(), np.full(tuple(dg.shape), 2.0 ** -23)))
    return dg, dl


def _crafted_logits(n):
    """(n, k) logit columns for one pixel each, with the bin torch.argmax gives"""
    cols, want = [], []

    def add(v, b):
        cols.append(v)
        want.append(b)

    base = np.linspace(-1.0, 0.5, n).astype(np.float32)
    for c in (0, n - 1, 5 % n):                       # the maximum in channel 0, in the last channel, inside
        v = base.copy(); v[c] = 10.0; add(v, c)
    v = base.copy(); v[[1, n - 2]] = 7.0; add(v, 1)                   # two equal maxima: the first wins
    v = base.copy(); v[[n // 3, n // 2, n - 1]] = 7.0; add(v, n // 3)  # three, the last bin among them
    v = base.copy(); v[[0, n - 1]] = 7.0; add(v, 0)                   # bin 0 against the last bin
    add(np.full(n, 0.25, dtype=np.float32), 0)                       # all equal
    add(np.zeros(n, dtype=np.float32), 0)
    v = np.full(n, -3e38, dtype=np.float32); v[n // 4] = 3e38; add(v, n // 4)
    v = np.full(n, 3e38, dtype=np.float32); v[0] = -3e38; add(v, 1)   # ties at +3e38 from channel 1 on
    v = np.full(n, -np.inf, dtype=np.float32); v[n // 2] = -5.0; add(v, n // 2)
    v = np.full(n, -np.inf, dtype=np.float32); v[n - 1] = 0.0; add(v, n - 1)
    v = np.full(n, -np.inf, dtype=np.float32); add(v, 0)               # -inf everywhere: all equal
    return np.stack(cols, axis=1), np.array(want)


@pytest.mark.parametrize("B,HW", [(1, 1), (2, 300), (3, 257)])
def test_decode_cls_random_and_crafted(ops, B, HW):
    lg, ll = _rand((B, NG, HW), 400 + HW), _rand((B, NL, HW), 401 + HW)
    cg, want_g = _crafted_logits(NG)
    cl, want_l = _crafted_logits(NL)
    k = cg.shape[1]
    if HW >= k:  # crafted pixels at the start of the first image and at the end of the last
        lg[0, :, :k], ll[0, :, :k] = torch.from_numpy(cg), torch.from_numpy(cl)
        lg[B - 1, :, HW - k:], ll[B - 1, :, HW - k:] = torch.from_numpy(cg), torch.from_numpy(cl)
        assert np.array_equal(lg[0, :, :k].argmax(0).numpy(), want_g) and np.array_equal(ll[0, :, :k].argmax(0).numpy(), want_l), "torch.argmax is the tie rule"
    dg, dl = _check_decode(ops, lg, ll, f"decode_cls B={B} HW={HW}")
    if HW >= k:
        assert np.array_equal(dl[0, :k].numpy(), (-89.5 + want_l).astype(np.float32))
        last = want_g == NG - 1
        assert bool((dg[0, :, :k][:, last] == 0).all()) and float(dl[0, 1]) == 89.5  # the last channel: (0, 0) exactly and 89.5 degrees


def test_decode_cls_single_pixel_every_crafted_case(ops):
    """(B, HW) = (n, 1): the crafted pixels as images of one pixel each"""
    cg, want_g = _crafted_logits(NG)
    cl, want_l = _crafted_logits(NL)
    lg, ll = torch.from_numpy(cg.T.copy())[:, :, None], torch.from_numpy(cl.T.copy())[:, :, None]
    dg, dl = _check_decode(ops, lg, ll, "decode_cls crafted, one pixel per image")
    assert np.array_equal(dl[:, 0].numpy(), (-89.5 + want_l).astype(np.float32))


def test_decode_cls_second_grid_trip(ops):
    """one thread per pixel, at most 8192 blocks of 256: 2 097 152 pixels per trip; the last five pixels are beyond it"""
    HW = 2097152 + 5
    lg, ll = _rand((1, 3, HW), 500), _rand((1, 2, HW), 501)
    lg[0, :, -5:] = torch.tensor([[1.0, 0.0, 0.0, 2.0, -1.0], [0.0, 1.0, 0.0, 2.0, -1.0], [0.0, 0.0, 1.0, 2.0, -1.0]])  # bins 0, 1, 2 (invalid), tie, tie
    ll[0, :, -5:] = torch.tensor([[1.0, 0.0, 3.0, 3.0, -2.0], [0.0, 1.0, 3.0, 4.0, -1.0]])
    dg, dl = _check_decode(ops, lg, ll, "decode_cls second grid trip (all pixels)")
    _check_decode(ops, lg, ll, "decode_cls second grid trip (last five)", sl=slice(HW - 5, HW))
    assert dl[0, -5:].tolist() == [-45.0, 45.0, -45.0, 45.0, 45.0]
    assert dg[0, :, -3].tolist() == [0.0, 0.0] and dg[0, 0, -5:].tolist()[:2] == [-1.0, 1.0]


# --------------------------------------------------------------------------------------------------------------- decode -> post-process with invalid bins
NET = 320
POST_SIZES = [(1, 1), (1, 17), (19, 1), (64, 48), (97, 131)]


def _tap_rows(n_out, n_in):
    """the two source rows (columns) the post-process kernel blends for every output row: fp32 scale and source coordinate, clamped at 0 (elem.hip, as
    F.interpolate(mode="bilinear", align_corners=False))"""
    r = np.float32(n_in) / np.float32(n_out)
    s = np.maximum(r * (np.arange(n_out, dtype=np.float32) + np.float32(0.5)) - np.float32(0.5), np.float32(0))
    i0 = np.minimum(s.astype(np.int64), n_in - 1)
    return i0, i0 + (i0 < n_in - 1)


@pytest.fixture(scope="module")
def engines():
    from perspectivefields_amd.engine import Engine

    return {"cls": Engine(1, "cuda:0"), "reg": Engine(0, "cuda:0")}  # PF_ARCH_PERSNET_CLS / PF_ARCH_PARAMNET_CENTERED: pf_postprocess needs the architecture only


@pytest.mark.parametrize("pattern", ["isolated", "blocks2x2", "whole"])
def test_decode_then_postprocess_with_invalid_bins(ops, engines, pattern):
    """The zero vector of the invalid gravity bin blended with valid neighbours, from a 320 x 320 field.  The logits go through the classification post-process
    (decode + bilinear + normalise) and pf_op_decode_cls's own output goes through the regression post-process: the same up-vectors bit for bit, and both against the
    oracle within the tolerance tests/test_gpu_fullsize.py::test_postprocess_every_pixel_vs_oracle applies to this kernel (1 - cos <= 1e-6; latitude mean 1e-4, max
    5e-2 degrees).  Valid bins vary slowly over the image, so that no blend of valid neighbours cancels."""
    from tests.parity import one_minus_cos

    yy, xx = np.meshgrid(np.arange(NET), np.arange(NET), indexing="ij")
    gbin = ((yy // 2 + xx // 2) % (NG - 1)).astype(np.int64)  # neighbours at most two bins (10 degrees) apart, also across the wrap from bin 71 to bin 0
    lbin = ((yy // 4 + 2 * (xx // 8)) % NL).astype(np.int64)
    # (159, 159) is one of the four taps of the 1 x 1 output: it is invalid in every pattern
    inval = {"isolated": (yy % 7 == 5) & (xx % 5 == 4), "blocks2x2": ((yy // 2) % 4 == 3) & ((xx // 2) % 3 == 1), "whole": np.ones((NET, NET), dtype=bool)}[pattern]
    assert inval[159, 159]
    gbin[inval] = NG - 1
    lg = _rand((NG, NET, NET), 600, 0.1)
    ll = _rand((NL, NET, NET), 601, 0.1)
    lg.scatter_(0, torch.from_numpy(gbin)[None], 5.0)
    ll.scatter_(0, torch.from_numpy(lbin)[None], 5.0)
    lgd, lld = lg.cuda(), ll.cuda()
    dg, dl = ops.decode_cls(lgd.view(1, NG, NET * NET), lld.view(1, NL, NET * NET))
    dg, dl = dg.view(2, NET, NET), dl.view(NET, NET)
    assert bool((dg.cpu()[:, torch.from_numpy(inval)] == 0).all()) and np.array_equal(lg.argmax(0).numpy(), gbin)
    zeros = torch.zeros((1, NET, NET), device="cuda")
    worst_c = worst_mean = worst_max = 0.0
    for H, W in POST_SIZES:
        up, lat = engines["cls"].postprocess(lgd, lld, H, W)
        up2, _ = engines["reg"].postprocess(dg, zeros, H, W)
        assert torch.equal(up.view(torch.int32), up2.view(torch.int32)), f"{pattern} {H}x{W}: pf_op_decode_cls output through pf_postprocess differs from the classification path"
        up, lat = up.cpu().numpy(), lat.cpu().numpy()
        assert np.isfinite(up).all() and np.isfinite(lat).all()
        up_ref = pf_oracle.postprocess_gravity(lg, H, W, True, NG).numpy()
        lat_ref = pf_oracle.postprocess_latitude(ll, H, W, True, NL).numpy()
        y0, y1 = _tap_rows(H, NET)
        x0, x1 = _tap_rows(W, NET)
        taps = [inval[np.ix_(r, c)] for r in (y0, y1) for c in (x0, x1)]
        dead, mixed = taps[0] & taps[1] & taps[2] & taps[3], (taps[0] | taps[1] | taps[2] | taps[3])
        mixed &= ~dead
        assert pattern == "whole" or mixed.any(), "every size must blend an invalid tap with valid ones"
        assert np.all(up[:, dead] == 0), f"{pattern} {H}x{W}: four invalid taps must give exactly (0, 0)"
        assert np.all(up_ref[:, dead] == 0)
        if pattern == "whole":
            assert dead.all()
        live = ~dead
        nz = (up_ref ** 2).sum(0) > 0
        assert np.array_equal((up ** 2).sum(0) > 0, nz), f"{pattern} {H}x{W}: zero vectors in other places than the oracle's"
        c = one_minus_cos(up, up_ref)
        d = np.abs(lat.astype(np.float64) - lat_ref)
        worst_c, worst_mean, worst_max = max(worst_c, c.max() / 1e-6), max(worst_mean, d.mean() / 1e-4), max(worst_max, d.max() / 5e-2)
        print(f"[head/tail post {pattern} {H}x{W}] outputs with four invalid taps {dead.mean():.3f}, with one to three {mixed.mean():.3f}; of the others 1-cos max {c[live].max() if live.any() else 0.0:.2e}; |lat| max {d.max():.2e} mean {d.mean():.2e} deg")
    _report(f"decode -> postprocess {pattern}: 1-cos", worst_c)
    _report(f"decode -> postprocess {pattern}: latitude mean", worst_mean)
    _report(f"decode -> postprocess {pattern}: latitude max", worst_max)


# --------------------------------------------------------------------------------------------------------------- nearest resize
def _param_input_size():
    from perspectivefields_amd.config import arch_of, get_cfg

    return int(arch_of(get_cfg("Paramnet-360Cities-edina-uncentered"))["param_input_size"])


NEAREST_CASES = [(320, 320, "zoo", "zoo")] + [(320, 320, s, s) for s in (224, 96, 7, 1, 320, 319, 321, 640)] + [(13, 29, 5, 31)]


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("H,W,Ho,Wo", NEAREST_CASES, ids=[f"{c[0]}x{c[1]}-{c[2]}x{c[3]}" for c in NEAREST_CASES])
def test_nearest_equals_torch_interpolate(ops, H, W, Ho, Wo, B):
    """bit-equal to F.interpolate(x, (Ho, Wo)) (legacy 'nearest') on the CPU; every pixel carries its own values, so one wrong source index shows"""
    if Ho == "zoo":
        Ho = Wo = _param_input_size()
        assert Ho != NET, "the zoo's uncentered ParamNet runs on a resized input"
    x = torch.arange(B * H * W * 4, dtype=torch.float32).reshape(B, H, W, 4)  # < 2^24: exact
    ref = F.interpolate(x.permute(0, 3, 1, 2), (Ho, Wo)).permute(0, 2, 3, 1).contiguous()
    got = ops.nearest_nhwc4(x.cuda(), Ho, Wo).cpu()
    bad = int((got != ref).any(-1).sum())
    print(f"[head/tail nearest B={B} {H}x{W} -> {Ho}x{Wo}] pixels that differ {bad} (bound 0)")
    assert torch.equal(got, ref), f"{bad} of {B * Ho * Wo} pixels differ"


# --------------------------------------------------------------------------------------------------------------- ConvNeXt tail
def _gap_case(C, HW, nout, B, seed, outliers=False):
    x = _rand((B, HW, C), seed)
    if outliers:  # two channels 100 sigma out, every channel offset by 50: cancellation in the variance and in the serial sum over HW
        x[..., C // 3] += 100.0
        x[..., C - 5] -= 100.0
        x += 50.0
    g, be = 1 + _rand((C,), seed + 1, 0.3), _rand((C,), seed + 2, 0.2)
    w, hb = _rand((nout, C), seed + 3, 1.0 / math.sqrt(C)), _rand((nout,), seed + 4, 0.1)
    ref = F.linear(pf_oracle.layer_norm(x.double().mean(1), g.double(), be.double(), 1e-6), w.double(), hb.double())
    return x, g, be, w, hb, ref


def _gap_check(ops, case, what):
    """|err| <= 2e-5 (1 + |ref|): the convention of tests/test_gpu_ops.py::_close for fp32 accumulation, inside the 1e-4 ParamNet gate (tests/parity.py TOL_PARAM)"""
    x, g, be, w, hb, ref = case
    xd = x.cuda()
    got = ops.gap_ln_head(xd, g, be, 1e-6, w, hb)
    again = ops.gap_ln_head(xd, g, be, 1e-6, w, hb)
    assert torch.equal(got.view(torch.int32), again.view(torch.int32)), f"{what}: two runs differ"
    assert got.shape == ref.shape
    _report(what, _ratio((got.cpu().double() - ref).abs().numpy(), (2e-5 * (1.0 + ref.abs())).numpy()))


@pytest.mark.parametrize("C,HW,nout,B", [(768, 100, 4, 2), (768, 49, 5, 3), (768, 1, 4, 1), (320, 7, 5, 1), (1024, 3, 1, 1), (96, 513, 8, 2)])
def test_gap_ln_head(ops, C, HW, nout, B):
    _gap_check(ops, _gap_case(C, HW, nout, B, 700 + C + HW), f"gap_ln_head C={C} HW={HW} nout={nout} B={B}")


def test_gap_ln_head_outlier_channels_and_offset(ops):
    _gap_check(ops, _gap_case(768, 100, 4, 2, 750, outliers=True), "gap_ln_head C=768 HW=100 outlier channels + offset 50")


def test_gap_ln_head_rejects_wide_rows(ops):
    from perspectivefields_amd.engine import PfError

    x, g, be, w, hb, _ = _gap_case(1025, 2, 1, 1, 760)
    with pytest.raises(PfError, match="1024"):
        ops.gap_ln_head(x.cuda(), g, be, 1e-6, w, hb)


# --------------------------------------------------------------------------------------------------------------- ParamNet scalars
@pytest.mark.parametrize("B", [1, 63, 64, 65, 200])
def test_paramnet_scalars_centered(ops, B):
    """mode 0: roll, pitch, vfov = fp32(raw) * 90 exactly; rel_focal = 1 / (2 tan raw2) within 1e-6 max(1, |ref|) (the tolerance of
    tests/test_gpu_r06.py::test_uncentered_focal_is_computed_on_the_device); the raw bits behind them.  64-thread blocks: B around 64."""
    g = torch.Generator().manual_seed(800 + B)
    raw = torch.randn((B, 5), generator=g)
    mag = 0.05 + 1.45 * torch.rand(B, generator=g)
    raw[:, 2] = torch.where(torch.rand(B, generator=g) < 0.5, -mag, mag)
    raw[0, 2] = 1.5
    if B > 1:
        raw[1, 2], raw[B - 1, 2] = -0.05, 0.0
    out = ops.paramnet_scalars(raw.cuda(), 0).cpu().numpy()
    r = raw.numpy()
    want = r[:, :3] * np.float32(90.0)
    assert np.array_equal(_bits(out[:, :3]), _bits(want))
    assert np.array_equal(_bits(out[:, 4:8]), _bits(r[:, :4]))
    with np.errstate(divide="ignore"):
        ref = 1.0 / (2.0 * np.tan(r[:, 2].astype(np.float64)))
    fin = np.isfinite(ref)
    assert np.array_equal(np.isposinf(out[:, 3]), np.isposinf(ref)) and (B == 1 or np.isposinf(out[B - 1, 3])), "raw2 = 0 gives +inf"
    _report(f"paramnet_scalars mode 0 B={B} rel_focal", _ratio(np.abs(out[fin, 3] - ref[fin]), 1e-6 * np.maximum(1.0, np.abs(ref[fin]))))


def _cos_fov(f, cx, cy):
    """the reference's equation (utils/utils.py:47-91, h = 1): cosine of the angle between the rays through the top and the bottom of the image's vertical centre line,
    and its derivative in f"""
    P, Q = f * f + cx * cx + (cy + 0.5) ** 2, f * f + cx * cx + (cy - 0.5) ** 2
    N, D = P + Q - 1.0, 2.0 * np.sqrt(P * Q)
    dD = 2.0 * f * (P + Q) / np.sqrt(P * Q)
    return N / D, (4.0 * f * D - N * dD) / (D * D)


GVFOV = [5, 30, 60, 89.999, 90, 90.001, 100, 120, 150, 170]
CENTRES = [0.0, 0.1, -0.1, 0.45, -0.45]


def test_paramnet_scalars_general_vfov_residual(ops):
    """mode 1, nraw = 5: out[5] must SOLVE the reference's equation cos_FoV(f; cx, cy) = cos(gvfov) -- checked by the residual in fp64 at the fp32 output, not against
    the closed form the kernel evaluates: |residual| <= 1e-6 + 2^-23 |d cos_FoV / d f| f (the second term is the fp32 rounding of f).  The grid holds both roots of
    the quadratic (gvfov below and above 90 degrees) and disc == 0 (90 degrees).

    cos_FoV rises monotonically in f from cos_FoV(0) = (cx^2 + cy^2 - 1/4) / sqrt((cx^2 + (cy + 1/2)^2) (cx^2 + (cy - 1/2)^2)) to 1: a principal point off the centre
    line (cx != 0) caps the angle below 180 degrees, and 70 of the 250 grid points ask for more than their cap (e.g. cx = 0.45, cy = 0 ends at 96 degrees).  No f solves
    the equation there, the reference's fsolve does not converge either; at those points the device value is pinned to the host's general_vfov_to_focal instead
    (the documented behaviour, 1e-6 max(1, f)).  Which points these are is decided from the equation alone."""
    from perspectivefields_amd.perspectivefields import general_vfov_to_focal

    rows = [(gv, cx, cy) for gv in GVFOV for cx in CENTRES for cy in CENTRES]
    raw = np.zeros((len(rows), 5), dtype=np.float32)
    raw[:, :2] = _rand((len(rows), 2), 900).numpy()
    raw[:, 2] = np.array([r[0] for r in rows], dtype=np.float64) / 90.0
    raw[:, 3] = [r[1] for r in rows]
    raw[:, 4] = [r[2] for r in rows]
    out = ops.paramnet_scalars(torch.from_numpy(raw).cuda(), 1).cpu().numpy()
    assert np.array_equal(_bits(out[:, :5]), _bits(raw)) and np.all(out[:, 6:] == 0)
    f = out[:, 5].astype(np.float64)
    gv = (raw[:, 2] * np.float32(90.0)).astype(np.float64)  # the factor in fp32, as the reference's x[:, idx] * factor
    cx, cy = raw[:, 3].astype(np.float64), raw[:, 4].astype(np.float64)
    target = np.cos(np.radians(gv))
    floor, _ = _cos_fov(np.zeros_like(cx), cx, cy)
    feasible = target > floor
    print(f"[head/tail paramnet_scalars mode 1] grid points with a solution: {int(feasible.sum())} of {len(rows)}; '-' root among them: {int((feasible & (target < 0)).sum())}")
    assert int(feasible.sum()) == 180 and int((feasible & (target < 0)).sum()) == 63 and int((feasible & (target >= 0)).sum()) == 117  # counted on the CPU from the equation alone
    assert np.isfinite(f).all() and np.all(f >= 0)
    val, slope = _cos_fov(f, cx, cy)
    resid = np.abs(val - target)
    _report("paramnet_scalars mode 1 residual of cos_FoV(f) = cos(gvfov)", _ratio(resid[feasible], 1e-6 + 2.0 ** -23 * np.abs(slope[feasible]) * f[feasible]))
    # the reference's own solver, wherever it converged
    err, bnd = [], []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for i in range(len(rows)):
            fs = float(pf_oracle.general_vfov_to_focal([cx[i]], [cy[i]], [gv[i]])[0])
            if abs(_cos_fov(np.float64(fs), cx[i], cy[i])[0] - target[i]) < 1e-10:
                err.append(abs(f[i] - fs)); bnd.append(1e-6 * max(1.0, fs))
    print(f"[head/tail paramnet_scalars mode 1] fsolve converged (residual < 1e-10) at {len(err)} points")
    assert len(err) == int(feasible.sum()), "fsolve converges exactly where the equation has a solution"
    _report("paramnet_scalars mode 1 vs fsolve", _ratio(err, bnd))
    host = general_vfov_to_focal(cx, cy, gv)
    _report("paramnet_scalars mode 1 vs the host closed form, points without a solution", _ratio(np.abs(f - host)[~feasible], (1e-6 * np.maximum(1.0, host))[~feasible]))


def test_paramnet_scalars_general_vfov_zero_is_infinite(ops):
    from perspectivefields_amd.perspectivefields import general_vfov_to_focal

    raw = np.zeros((len(CENTRES), 5), dtype=np.float32)
    raw[:, 3], raw[:, 4] = CENTRES, CENTRES[::-1]
    out = ops.paramnet_scalars(torch.from_numpy(raw).cuda(), 1).cpu().numpy()
    with np.errstate(divide="ignore", invalid="ignore"):
        host = general_vfov_to_focal(raw[:, 3], raw[:, 4], raw[:, 2] * np.float32(90.0))
    print(f"[head/tail paramnet_scalars mode 1 gvfov = 0] device {out[:, 5]} host {host}")
    assert np.all(np.isposinf(host)) and np.all(np.isposinf(out[:, 5]))


@pytest.mark.parametrize("nraw", [3, 4, 6, 8])
def test_paramnet_scalars_other_output_counts(ops, nraw):
    """mode 1 without the zoo's five outputs: the raw bits, zero padded to 8 columns"""
    raw = _rand((65, nraw), 950 + nraw)
    out = ops.paramnet_scalars(raw.cuda(), 1).cpu().numpy()
    want = np.zeros((65, 8), dtype=np.float32)
    want[:, :nraw] = raw.numpy()
    assert np.array_equal(_bits(out), _bits(want))


def test_paramnet_scalars_rejects_what_the_kernel_cannot_take(ops):
    from perspectivefields_amd.engine import PfError

    for nraw, mode in ((9, 1), (3, 0), (5, 2)):
        with pytest.raises(PfError):
            ops.paramnet_scalars(torch.zeros((2, nraw), device="cuda"), mode)


# --------------------------------------------------------------------------------------------------------------- fused prediction-head epilogue
HB, HH, HWID, HCIN = 2, 17, 24, 64   # the form's test shape: 816 pixels, ragged against every tile (128 / 256 rows, 8 x 16 and 16 x 16 patches)


def _head_tile_params():
    """('auto', -1) and every tile conv_tile_usable accepts for the form -- host logic of the built library, no GPU needed at collection"""
    try:
        from perspectivefields_amd import ops as _ops

        names = _ops.conv_tiles()
        return [pytest.param(-1, id="auto")] + [pytest.param(t, id=names[t]) for t in _ops.conv2d_head_tiles(HB, HH, HWID, HCIN, 1, 1)]
    except Exception:  # library not built: the test itself reports it
        return [pytest.param(None, id="library-unavailable")]


HEAD_TILES = _head_tile_params()


@pytest.fixture(scope="module")
def head_case():
    """one input, one conv and its fp64 reference for all the epilogue tests"""
    x = _rand((HB, HH, HWID, HCIN), 1000)
    w = _rand((32, HCIN, 3, 3), 1001, 1.0 / math.sqrt(HCIN * 9))
    b = _rand((32,), 1002, 0.1)
    fmap = F.relu(F.conv2d(x.double().permute(0, 3, 1, 2), w.double(), b.double(), padding=1)).permute(0, 2, 3, 1).reshape(HB, HH * HWID, 32).numpy()
    return {"x": x, "xd": x.cuda(), "w": w, "b": b, "map": fmap, "map_err": 2e-5 * (1.0 + np.abs(fmap))}  # the bound of tests/test_gpu_ops.py::test_conv2d_all_tiles


def test_fused_head_tile_list():
    from perspectivefields_amd import ops as _ops

    names = _ops.conv_tiles()
    for kind in (1, 2):
        tiles = [names[t] for t in _ops.conv2d_head_tiles(HB, HH, HWID, HCIN, 1, kind)]
        print(f"[head/tail fused head] tiles that run head_kind {kind}: {tiles}")
        assert tiles and any(n.startswith("sbh") for n in tiles) and any(n.startswith("sb") and not n.startswith("sbh") for n in tiles)
    assert [p.values[0] for p in HEAD_TILES[1:]] == _ops.conv2d_head_tiles(HB, HH, HWID, HCIN, 1, 1) == _ops.conv2d_head_tiles(HB, HH, HWID, HCIN, 1, 2)


@pytest.mark.parametrize("tile", HEAD_TILES)
def test_fused_head_vs_fp64_and_standalone(ops, head_case, tile):
    """conv -> ReLU -> 1x1 head -> normalise / clamp inside the conv's epilogue: against fp64, and bit-equal to the same tile storing its 32-channel map followed by
    the stand-alone kernel (the identity tests/test_gpu_e2e.py::test_fused_prediction_heads_equal_standalone_kernel claims for the whole network)."""
    assert tile is not None, "libpf_hip.so could not be loaded at collection"
    c = head_case
    wg, bg = _rand((2, 32), 1010, 1.0 / math.sqrt(32)), _rand((2,), 1011, 0.1)
    wl, bl = _rand((1, 32), 1012, 1.0 / math.sqrt(32)), _rand((1,), 1013, 0.1)
    M = HB * HH * HWID
    pn = torch.full((M, 4), 7.0, device="cuda")
    g = ops.conv2d_head(c["xd"], c["w"], c["b"], 1, 1, wg, bg, tile=tile, pn=pn)
    assert bool((pn[:, 2:] == 7.0).all()) and torch.equal(pn[:, :2].reshape(HB, -1, 2).permute(0, 2, 1).contiguous().view(torch.int32), g.view(torch.int32))
    lat = ops.conv2d_head(c["xd"], c["w"], c["b"], 1, 2, wl, bl, tile=tile, pn=pn)
    assert torch.equal(pn[:, 2].reshape(HB, -1).view(torch.int32), lat.view(torch.int32)) and bool((pn[:, 3] == 0).all())
    assert torch.equal(ops.conv2d_head(c["xd"], c["w"], c["b"], 1, 1, wg, bg, tile=tile).view(torch.int32), g.view(torch.int32)), "pn = NULL changes the output"
    # fp64
    raw, E = _head_bounds(c, wg, bg)
    n = np.sqrt((raw * raw).sum(-1))
    keep = n >= 1e-6
    print(f"[head/tail fused head tile {tile}] pixels left out of the gravity comparison (fp64 norm < 1e-6): {1.0 - keep.mean():.3g}")
    assert keep.mean() >= 0.99
    ref_g = raw / np.maximum(n, 1e-12)[..., None]
    got_g = g.cpu().double().numpy().transpose(0, 2, 1)
    _report(f"fused head tile {tile} gravity", _ratio(np.abs(got_g - ref_g)[keep], _normalize_bounds(raw, E, n)[keep]))
    raw_l, El = _head_bounds(c, wl, bl)
    _report(f"fused head tile {tile} latitude", _ratio(np.abs(lat.cpu().double().numpy() - np.clip(raw_l[..., 0], -1, 1)), El[..., 0] + U))
    # the same tile with its map stored, then the stand-alone heads
    fmap = ops.conv2d(c["xd"], c["w"], c["b"], pad=1, act=1, tile=tile, splitk=False).reshape(HB, HH * HWID, 32)
    pg, pl, _ = ops.pred_regression(fmap, fmap, wg, bg, wl, bl)
    assert torch.equal(pg.view(torch.int32), g.view(torch.int32)), f"tile {tile}: fused gravity head differs from conv + pred_regression"
    assert torch.equal(pl.view(torch.int32), lat.view(torch.int32)), f"tile {tile}: fused latitude head differs from conv + pred_regression"


@pytest.mark.parametrize("tile", HEAD_TILES)
def test_fused_head_crafted_heads(ops, head_case, tile):
    assert tile is not None, "libpf_hip.so could not be loaded at collection"
    c = head_case
    z = ops.conv2d_head(c["xd"], c["w"], c["b"], 1, 1, np.zeros((2, 32), np.float32), np.zeros(2, np.float32), tile=tile)
    assert bool((z == 0).all()), "zero gravity head: (0, 0) everywhere (the eps path)"
    z = ops.conv2d_head(c["xd"], c["w"], c["b"], 1, 2, np.zeros((1, 32), np.float32), np.zeros(1, np.float32), tile=tile)
    assert bool((z == 0).all()), "zero latitude head: 0 everywhere"
    wl = _rand((1, 32), 1020, 0.1 / math.sqrt(32))
    raw, E = _head_bounds(c, wl, np.zeros(1))
    raw, E = raw[..., 0], E[..., 0]
    assert np.abs(raw).max() + E.max() < 1.0  # on the reference: +-2 clamps every pixel
    for sgn in (1.0, -1.0):
        got = ops.conv2d_head(c["xd"], c["w"], c["b"], 1, 2, wl, np.array([2.0 * sgn], np.float32), tile=tile)
        assert bool((got == sgn).all()), f"latitude bias {2 * sgn}: every pixel clamps to {sgn}"
    # a bias that puts the clamp through the middle of the image
    wl = _rand((1, 32), 1021, 1.0 / math.sqrt(32))
    raw, E = _head_bounds(c, wl, np.zeros(1))
    raw, E = raw[..., 0], E[..., 0]
    bias = np.float32(1.0 - np.median(raw))
    val = raw + np.float64(bias)
    share = float((val > 1.0).mean())
    print(f"[head/tail fused head tile {tile}] share of pixels the reference clamps at +1: {share:.3f}")
    assert 0.3 <= share <= 0.7
    got = ops.conv2d_head(c["xd"], c["w"], c["b"], 1, 2, wl, np.array([bias]), tile=tile).cpu().double().numpy()
    _report(f"fused head tile {tile} latitude, half the image clamped", _ratio(np.abs(got - np.clip(val, -1, 1)), E + U * (1.0 + np.abs(val))))
    sure = val > 1.0 + E + U * (1.0 + np.abs(val))
    assert sure.mean() >= 0.25 and np.all(got[sure] == 1.0) and got.max() <= 1.0, "beyond the bound the clamp gives exactly 1"


def test_fused_head_refuses_a_tile_that_cannot_run_it(ops, head_case):
    from perspectivefields_amd.engine import PfError

    c = head_case
    names = ops.conv_tiles()
    usable = set(ops.conv2d_head_tiles(HB, HH, HWID, HCIN, 1, 1))
    wg, bg = np.zeros((2, 32), np.float32), np.zeros(2, np.float32)
    refused = 0
    for t in [names.index("128x128p"), names.index("sb128x128"), names.index("sbh128x64"), len(names) - 1, len(names), -2]:
        assert t not in usable
        with pytest.raises(PfError):
            ops.conv2d_head(c["xd"], c["w"], c["b"], 1, 1, wg, bg, tile=t)
        refused += 1
    with pytest.raises(PfError):
        ops.conv2d_head(c["xd"], c["w"], c["b"], 1, 3, wg, bg)   # no such head
    with pytest.raises(PfError):
        ops.conv2d_head(c["xd"][..., :48].contiguous(), c["w"][:, :48], c["b"], 1, 1, wg, bg)  # Cin no multiple of 32
    print(f"[head/tail fused head] tiles refused {refused} (bound: all)")
