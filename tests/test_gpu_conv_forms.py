"""Kernel-level parity (-m gpu) of the conv forms that only the forward's grouped launches set (pf_engine::conv_g): the first input at half resolution with the bilinear
x2 interpolation inside the halo staging (ConvParams::ups), two problems in one grid (ConvParams::groups, both decoder heads), and the nine-case border bias table of
the folded Linear -> 3x3 pair (ConvPtrs::bias_tab) -- through pf_op_conv2d_g (include/pf_hip.h), on the smallest shapes at which each mechanism can go wrong, against
fp64 torch on the CPU and, bit for bit, against the launches they claim to equal.

Every test runs `auto` and every tile pf_op_conv2d_g_tile_usable accepts for its form; the entry refuses a tile it cannot run, so a test that names a tile has run it.
The base bound is the project's conv bound 2e-5 (1 + |ref|) (tests/test_gpu_ops.py::_close); the up-sampling forms add 3 u (|w| * |up(x)|) for the fp32 interpolation
(u = 2^-24: two products and one rounding of the sum per axis pair, |up(x)| <= the same combination of |x|); the head bounds are those of
tests/test_gpu_head_tail.py.  None comes from what a kernel returns.  Every test prints its worst error over its bound."""
import functools
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.conv_form_cases import (GROUP_FORMS, GROUP_SHAPES, Q_GROUP1, Q_GROUP3, Q_GROUP_HEAD, Q_SPLITK, Q_TABLE, Q_UPS, Q_UPS_HEAD, SHAPES, TABLE_FORMS, TABLE_SHAPES, UPS_FORMS,
                                   is_linear_sb as _is_linear_sb)
from tests.kernel_bounds import U, _head_bounds, _normalize_bounds, _ratio, _worse

pytestmark = pytest.mark.gpu

TOL = 2e-5  # tests/test_gpu_ops.py::test_conv2d_all_tiles


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


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _report(what, worst):
    print(f"[conv forms {what}] worst error / bound {worst:.3g}")
    assert worst <= 1.0, f"{what}: error is {worst:.3g} x its bound"


def _names():
    from perspectivefields_amd import ops as _ops

    return _ops.conv_tiles()


def _usable(**form):
    from perspectivefields_amd import ops as _ops

    return _ops.conv2d_g_tiles(**form)


def _tile_params(**form):
    """('auto', -1) and every tile the usability query accepts for the form -- host logic of the built library, no GPU needed at collection"""
    try:
        names = _names()
        return [pytest.param(-1, id="auto")] + [pytest.param(t, id=names[t]) for t in _usable(**form)]
    except Exception:  # library not built: the test itself reports it
        return [pytest.param(None, id="library-unavailable")]


# the query's answer for a form does not depend on the map size (asserted in test_tile_lists_hold_the_families_the_engine_uses), so one list serves every shape
UPS_TILES, UPS_HEAD_TILES = _tile_params(**Q_UPS), _tile_params(**Q_UPS_HEAD)
GROUP3_TILES, GROUP1_TILES, GROUP_HEAD_TILES = _tile_params(**Q_GROUP3), _tile_params(**Q_GROUP1), _tile_params(**Q_GROUP_HEAD)
TABLE_TILES = _tile_params(**Q_TABLE)


def _tn(tile):
    return "auto" if tile < 0 else _names()[tile]


# --------------------------------------------------------------------------------------------------------------- problems and their fp64 references
def border_case(Ho, Wo):
    """(Ho, Wo) int array: row 3 cy + cx of the bias table a pixel takes -- cy = 0 on the first output row, 2 on the last, 1 between; cx likewise by column"""
    cy = np.where(np.arange(Ho) == 0, 0, np.where(np.arange(Ho) == Ho - 1, 2, 1))
    cx = np.where(np.arange(Wo) == 0, 0, np.where(np.arange(Wo) == Wo - 1, 2, 1))
    return cy[:, None] * 3 + cx[None, :]


def make_problem(seed, B, H, W, C1, C2, Cout, K, ups=False, residuals=0, table=False):
    hs, ws = (H // 2, W // 2) if ups else (H, W)
    pad = K // 2
    Ho, Wo = H + 2 * pad - K + 1, W + 2 * pad - K + 1
    pr = {"x": _rand((B, hs, ws, C1), seed), "weight": _rand((Cout, C1 + C2, K, K), seed + 2, 1.0 / math.sqrt((C1 + C2) * K * K)),
          "bias": _rand((9, Cout), seed + 3, 0.5) if table else _rand((Cout,), seed + 3, 0.1)}
    if C2:
        pr["x2"] = _rand((B, H, W, C2), seed + 1)
    if residuals >= 1:
        pr["res1"] = _rand((B, Ho, Wo, Cout), seed + 4)
    if residuals >= 2:
        pr["res2"] = _rand((B, Ho, Wo, Cout), seed + 5)
    return pr


def reference(pr, act=0, post_relu=False, ups=False):
    """fp64: (output (B, Ho, Wo, Cout), bound) of one problem; the pre-residual activation map is what a fused head reads"""
    w = pr["weight"].double()
    K, C1 = w.shape[-1], pr["x"].shape[-1]
    xd = pr["x"].double().permute(0, 3, 1, 2)
    if ups:
        xd = F.interpolate(xd, scale_factor=2, mode="bilinear", align_corners=False)
    full = xd if "x2" not in pr else torch.cat([xd, pr["x2"].double().permute(0, 3, 1, 2)], dim=1)
    b = pr["bias"].double()
    y = F.conv2d(full, w, None if b.ndim == 2 else b, padding=K // 2).permute(0, 2, 3, 1)
    if b.ndim == 2:
        y = y + b[torch.from_numpy(border_case(y.shape[1], y.shape[2]))]
    if act == 1:
        y = torch.relu(y)
    for r in ("res1", "res2"):
        if r in pr:
            y = y + pr[r].double()
    if post_relu:
        y = torch.relu(y)
    bound = TOL * (1.0 + y.abs())
    if ups:  # the in-kernel fp32 interpolation, through |w| of the interpolated channels
        bound = bound + 3 * U * F.conv2d(xd.abs(), w[:, :C1].abs(), None, padding=K // 2).permute(0, 2, 3, 1)
    return y.contiguous().numpy(), bound.contiguous().numpy()


def _gpu(pr):
    """the problem with its device tensors on the GPU (host weights stay)"""
    if "_gpu" not in pr:
        pr["_gpu"] = {k: (v.cuda() if k in ("x", "x2", "res1", "res2") else v) for k, v in pr.items() if not k.startswith("_")}
    return dict(pr["_gpu"])


def _seed(*key):
    return 7000 + 131 * (sum((i + 1) * ord(c) for i, c in enumerate("/".join(str(k) for k in key))) % 9973)


@functools.lru_cache(maxsize=None)
def ups_case(form, shape):
    C1, C2, Cout, act = UPS_FORMS[form]
    pr = make_problem(_seed(form, shape), *shape, C1, C2, Cout, 3, ups=True)
    pr["_ref"], pr["_bound"] = reference(pr, act=act, ups=True)
    return pr


@functools.lru_cache(maxsize=None)
def group_case(form, shape):
    C1, Cout, K, pad, act, residuals, post_relu, _ = GROUP_FORMS[form]
    prs = [make_problem(_seed(form, shape, g), *shape, C1, 0, Cout, K, residuals=residuals) for g in (0, 1)]
    for pr in prs:
        pr["_ref"], pr["_bound"] = reference(pr, act=act, post_relu=post_relu)
    return prs


@functools.lru_cache(maxsize=None)
def table_case(form, shape):
    C1, Cout = TABLE_FORMS[form]
    prs = [make_problem(_seed(form, shape, g), *shape, C1, 0, Cout, 3, table=True) for g in (0, 1)]
    for pr in prs:
        pr["_ref"], pr["_bound"] = reference(pr)
    return prs


def head_weights(seed):
    return {1: (_rand((2, 32), seed, 1.0 / math.sqrt(32)), _rand((2,), seed + 1, 0.1)), 2: (_rand((1, 32), seed + 2, 1.0 / math.sqrt(32)), _rand((1,), seed + 3, 0.1))}


def head_reference(fmap, bound, kind, hw, hb):
    """fp64 head output on the fp64 map (B, Ho, Wo, 32) with the map's bound, in the output's layout ((B, 2, HW) / (B, HW)): (ref, bound, keep); keep leaves out the
    pixels whose gravity direction is ill-conditioned in fp64 too (norm < 1e-6), as tests/test_gpu_head_tail.py does"""
    B = fmap.shape[0]
    case = {"map": fmap.reshape(B, -1, 32), "map_err": bound.reshape(B, -1, 32)}
    raw, E = _head_bounds(case, hw, hb)
    if kind == 2:
        return np.clip(raw[..., 0], -1, 1), E[..., 0] + U, np.ones(raw.shape[:2], bool)
    n = np.sqrt((raw * raw).sum(-1))
    keep = n >= 1e-6
    return (raw / np.maximum(n, 1e-12)[..., None]).transpose(0, 2, 1), _normalize_bounds(raw, E, n).transpose(0, 2, 1), keep


def _check_head(got, fmap, bound, kind, hw, hb, what):
    ref, bnd, keep = head_reference(fmap, bound, kind, hw, hb)
    assert keep.mean() >= 0.99, f"{what}: {1.0 - keep.mean():.3g} of the pixels left out of the gravity comparison (at most 1 %)"
    got = got.cpu().double().numpy()
    assert got.shape == ref.shape and np.isfinite(got).all(), f"{what}: a head output is not finite (the NaN poison of checked_outputs: an element was not written)"
    err = np.abs(got - ref)
    if kind == 1:
        k2 = np.broadcast_to(keep[:, None, :], err.shape)
        return _ratio(err[k2], np.broadcast_to(bnd, err.shape)[k2])
    return _ratio(err, bnd)


def _check(got, pr, what):
    got = got.cpu().double().numpy()
    assert got.shape == pr["_ref"].shape and np.isfinite(got).all(), f"{what}: an output is not finite (the NaN poison of checked_outputs: an element was not written)"
    return _ratio(np.abs(got - pr["_ref"]), pr["_bound"])


# --------------------------------------------------------------------------------------------------------------- which tiles run which form
def test_tile_lists_hold_the_families_the_engine_uses():
    names = _names()
    ups = [names[t] for t in _usable(**Q_UPS)]
    print(f"[conv forms tiles] ups: {ups}")
    assert any(n.startswith("sbh128x") for n in ups) and "sbh256x32" in ups and "sbh256x64" in ups, ups
    assert all(n.startswith("sbh") for n in ups), ups
    for name, (C1, C2, Cout, act) in UPS_FORMS.items():  # one list for every channel form and every shape
        for B, H, W in SHAPES:
            assert _usable(B=B, H=H, W=W, C1=C1, C2=C2, Cout=Cout, K=3, pad=1, act=act, ups=True) == _usable(**Q_UPS), (name, B, H, W)
    ups_head = [names[t] for t in _usable(**Q_UPS_HEAD)]
    print(f"[conv forms tiles] ups + fused head: {ups_head}")
    assert ups_head and all(n.startswith("sbh") and n.endswith("x32") for n in ups_head) and _usable(**Q_UPS_HEAD) == _usable(**dict(Q_UPS_HEAD, head_kind=2)), ups_head
    g3 = [names[t] for t in _usable(**Q_GROUP3)]
    print(f"[conv forms tiles] groups = 2, 3x3: {g3}")
    assert any(_is_linear_sb(n) for n in g3) and any(n.startswith("sbh") for n in g3) and "wino256x64c" in g3 and "wino256x64d" in g3, g3
    for B, H, W in GROUP_SHAPES:
        assert _usable(**dict(Q_GROUP3, B=B, H=H, W=W)) == _usable(**Q_GROUP3) == _usable(**dict(Q_GROUP3, groups=1)), (B, H, W)
    g1 = [names[t] for t in _usable(**Q_GROUP1)]
    print(f"[conv forms tiles] groups = 2, 1x1: {g1}")
    assert any(_is_linear_sb(n) for n in g1) and not any(n.startswith(("sbh", "wino")) for n in g1), g1
    gh = [names[t] for t in _usable(**Q_GROUP_HEAD)]
    print(f"[conv forms tiles] groups = 2, fused heads: {gh}")
    assert any(_is_linear_sb(n) for n in gh) and any(n.startswith("sbh") for n in gh) and all(n.endswith(("x32", "x32f2")) for n in gh), gh
    sk = [names[t] for t in _usable(**Q_SPLITK)]
    assert any(_is_linear_sb(n) for n in sk), sk
    tab = [names[t] for t in _usable(**Q_TABLE)]
    print(f"[conv forms tiles] bias table: {tab}")
    assert any(_is_linear_sb(n) for n in tab) and any(n.startswith("sbh") for n in tab) and not any(n.startswith("wino") for n in tab), tab
    for form, (C1, Cout) in TABLE_FORMS.items():
        for B, H, W in TABLE_SHAPES:
            for groups in (1, 2):
                assert _usable(B=B, H=H, W=W, C1=C1, Cout=Cout, K=3, pad=1, groups=groups, has_table=True) == _usable(**Q_TABLE), (form, B, H, W, groups)
    for params, q in ((UPS_TILES, Q_UPS), (UPS_HEAD_TILES, Q_UPS_HEAD), (GROUP3_TILES, Q_GROUP3), (GROUP1_TILES, Q_GROUP1), (GROUP_HEAD_TILES, Q_GROUP_HEAD), (TABLE_TILES, Q_TABLE)):
        assert [p.values[0] for p in params[1:]] == _usable(**q)   # what the tests below were parametrised with at collection


# --------------------------------------------------------------------------------------------------------------- ups
@pytest.mark.parametrize("tile", UPS_TILES)
def test_ups_vs_fp64_and_materialised(ops, tile):
    """the conv on the half-resolution input, interpolated in the halo staging: against fp64 (F.interpolate on doubles, concat, conv), and bit-equal to the same tile on
    the tensor the stand-alone upsample2x kernel writes -- the identity engine_forward.hip claims for PF_FUSE_UPS and tests/test_gpu_e2e.py for the whole network"""
    assert tile is not None, "libpf_hip.so could not be loaded at collection"
    named = [t for t in _usable(**Q_UPS)]
    worst = 0.0
    for form, (C1, C2, Cout, act) in UPS_FORMS.items():
        for shape in SHAPES:
            pr = ups_case(form, shape)
            g = _gpu(pr)
            (got,), used = ops.conv2d_g([g], pad=1, act=act, ups=True, tile=tile)
            assert used == 1
            worst = _worse(worst, _check(got, pr, f"{form} {shape}"))
            up = ops.upsample2x(g["x"])
            if tile >= 0:
                assert tile in _usable(B=shape[0], H=shape[1], W=shape[2], C1=C1, C2=C2, Cout=Cout, K=3, pad=1, act=act)   # so ops.conv2d below really runs it
                mat = ops.conv2d(up, pr["weight"], pr["bias"], pad=1, act=act, x2=g.get("x2"), tile=tile, splitk=False)
                assert _same_bits(got, mat), f"{form} {shape} tile {tile}: fused up-sampling differs from upsample2x + conv on the same tile"
            else:  # the automatic choice of the plain form is another tile family: the fused result must be that of one of the form's own tiles
                assert any(_same_bits(got, ops.conv2d_g([g], pad=1, act=act, ups=True, tile=t)[0][0]) for t in named), f"{form} {shape}: auto ran none of {named}"
    _report(f"ups tile {_tn(tile)}", worst)


@pytest.mark.parametrize("tile", UPS_HEAD_TILES)
def test_ups_with_fused_head(ops, tile):
    """conv_fuse_conv1 as the forward runs it: half-resolution input, 64 -> 32, ReLU, the prediction head in the epilogue; both kinds, bounds as in
    tests/test_gpu_head_tail.py::test_fused_head_vs_fp64_and_standalone with the up-sampling term added to the map's bound; bit-equal to pf_op_conv2d_head on the
    materialised tensor"""
    assert tile is not None, "libpf_hip.so could not be loaded at collection"
    heads = head_weights(4100)
    worst = {1: 0.0, 2: 0.0}
    for shape in SHAPES:
        pr = ups_case("ups64-32", shape)
        g = _gpu(pr)
        M = shape[0] * shape[1] * shape[2]
        pn = torch.full((M, 4), 7.0, device="cuda")
        up = ops.upsample2x(g["x"])
        for kind in (1, 2):
            hw, hb = heads[kind]
            (got,), _ = ops.conv2d_g([dict(g, head_kind=kind, head_w=hw, head_b=hb, pn=pn)], pad=1, act=1, ups=True, tile=tile)
            worst[kind] = _worse(worst[kind], _check_head(got, pr["_ref"], pr["_bound"], kind, hw, hb, f"ups head {kind} {shape}"))
            if kind == 1:
                assert bool((pn[:, 2:] == 7.0).all()) and _same_bits(pn[:, :2].reshape(shape[0], -1, 2).permute(0, 2, 1), got)
            else:
                assert _same_bits(pn[:, 2].reshape(shape[0], -1), got) and bool((pn[:, 3] == 0).all())
            if tile >= 0:
                assert _same_bits(got, ops.conv2d_head(up, pr["weight"], pr["bias"], 1, kind, hw, hb, tile=tile)), f"{shape} kind {kind}: fused up-sampling changes the head"
    _report(f"ups fused head tile {_tn(tile)} gravity", worst[1])
    _report(f"ups fused head tile {_tn(tile)} latitude", worst[2])


# --------------------------------------------------------------------------------------------------------------- groups = 2
def _grouped_check(ops, form, tile, tiles_q):
    C1, Cout, K, pad, act, residuals, post_relu, shapes = GROUP_FORMS[form]
    worst = 0.0
    ran = 0
    for precision in (0, 3):
        if tile >= 0 and tile not in _usable(**dict(tiles_q, precision=precision)):
            continue   # a split-f16-only tile (sbh256x32, sbh256x64, the Winograd tiles) under the exact bf16 split
        for shape in shapes:
            prs = group_case(form, shape)
            g = [_gpu(pr) for pr in prs]
            both, used = ops.conv2d_g(g, pad=pad, act=act, post_relu=post_relu, tile=tile, precision=precision)
            assert used == 1, "none of these shapes meets the split-K rule"
            for i in (0, 1):
                (alone,), _ = ops.conv2d_g([g[i]], pad=pad, act=act, post_relu=post_relu, tile=tile, precision=precision)
                if tile >= 0:  # (auto: one problem and two may get different tiles from the cost model)
                    assert _same_bits(both[i], alone), f"{form} {shape} tile {tile} precision {precision}: group {i} differs from its own launch"
                worst = _worse(worst, _check(both[i], prs[i], f"{form} {shape} group {i}"), _check(alone, prs[i], f"{form} {shape} alone {i}"))
            ran += 1
    assert ran > 0
    _report(f"groups=2 {form} tile {_tn(tile)}", worst)


@pytest.mark.parametrize("tile", GROUP3_TILES)
@pytest.mark.parametrize("form", ["r1c2", "relu", "wino"])
def test_grouped_3x3(ops, form, tile):
    """two different problems in one grid: each group's output bit-equal to the groups = 1 launch of that problem on the same tile, and within the bound of fp64"""
    assert tile is not None, "libpf_hip.so could not be loaded at collection"
    _grouped_check(ops, form, tile, Q_GROUP3)


@pytest.mark.parametrize("tile", GROUP1_TILES)
def test_grouped_1x1(ops, tile):
    assert tile is not None, "libpf_hip.so could not be loaded at collection"
    _grouped_check(ops, "mlp1x1", tile, Q_GROUP1)


@pytest.mark.parametrize("tile", GROUP_HEAD_TILES)
def test_grouped_fused_heads_share_pn(ops, tile):
    """both prediction heads in one launch, as the forward runs them: group 0 the gravity head, group 1 the latitude head, one pn buffer; every pn row must be
    (g0, g1, lat, 0) with the bits of the two outputs, which equal the two groups = 1 launches and are within the head bounds of fp64"""
    assert tile is not None, "libpf_hip.so could not be loaded at collection"
    heads = head_weights(4200)
    worst = {1: 0.0, 2: 0.0}
    for shape in GROUP_SHAPES:
        prs = group_case("relu", shape)
        # 64 -> 32: the first 32 output channels of the 64 -> 64 problems
        sub = [dict(_gpu(pr), weight=pr["weight"][:32].contiguous(), bias=pr["bias"][:32].contiguous()) for pr in prs]
        B, M = shape[0], shape[0] * shape[1] * shape[2]
        pn = torch.full((M, 4), float("nan"), device="cuda")
        g = [dict(sub[0], head_kind=1, head_w=heads[1][0], head_b=heads[1][1], pn=pn), dict(sub[1], head_kind=2, head_w=heads[2][0], head_b=heads[2][1], pn=pn)]
        (grav, lat), _ = ops.conv2d_g(g, pad=1, act=1, tile=tile)
        want = torch.stack((grav[:, 0].reshape(-1), grav[:, 1].reshape(-1), lat.reshape(-1), torch.zeros(M, device="cuda")), dim=1)
        assert _same_bits(pn, want), f"{shape} tile {tile}: pn rows must be (g0, g1, lat, 0) with the bits of the two head outputs"
        for i, kind in ((0, 1), (1, 2)):
            fmap, bound = prs[i]["_ref"][..., :32], prs[i]["_bound"][..., :32]
            worst[kind] = _worse(worst[kind], _check_head((grav, lat)[i], fmap, bound, kind, *heads[kind], f"grouped head {kind} {shape}"))
            if tile >= 0:
                pn1 = torch.full((M, 4), float("nan"), device="cuda")
                (alone,), _ = ops.conv2d_g([dict(g[i], pn=pn1)], pad=1, act=1, tile=tile)
                assert _same_bits(alone, (grav, lat)[i]), f"{shape} tile {tile}: head {kind} differs from its own launch"
                assert _same_bits(pn1[:, :2] if kind == 1 else pn1[:, 2:], pn[:, :2] if kind == 1 else pn[:, 2:]) and bool(torch.isnan(pn1[:, 2:] if kind == 1 else pn1[:, :2]).all())
    _report(f"groups=2 fused heads tile {_tn(tile)} gravity", worst[1])
    _report(f"groups=2 fused heads tile {_tn(tile)} latitude", worst[2])


@functools.lru_cache(maxsize=None)
def splitk_case():
    prs = [make_problem(_seed("splitk", g), 1, 10, 10, 128, 0, 64, 3, residuals=1) for g in (0, 1)]
    for pr in prs:
        pr["_ref"], pr["_bound"] = reference(pr, act=1, post_relu=True)
    return prs


def _splitk_tiles():
    try:
        names = _names()
        return [pytest.param(-1, id="auto")] + [pytest.param(t, id=names[t]) for t in _usable(**Q_SPLITK) if _is_linear_sb(names[t])]
    except Exception:
        return [pytest.param(None, id="library-unavailable")]


@pytest.mark.parametrize("tile", _splitk_tiles())
def test_grouped_split_k(ops, tile):
    """3x3, 128 -> 64 on 10 x 10: 36 K steps and 4 tiles of 64 x 64, so the engine's rule (conv_splitk_shape) slices K; the partial sums of group 1 lie behind those of
    group 0 in one scratch buffer, and each group's reduce kernel applies its own scale, bias and residual.  The launch must report a factor above 1 -- this test cannot
    pass without split-K -- and equal, bit for bit, the two groups = 1 launches forced to the same factor."""
    assert tile is not None, "libpf_hip.so could not be loaded at collection"
    prs = splitk_case()
    g = [_gpu(pr) for pr in prs]
    worst = 0.0
    for precision in (0, 3):
        both, used = ops.conv2d_g(g, pad=1, act=1, post_relu=True, tile=tile, precision=precision)
        assert used > 1, f"split-K factor {used}: the launch did not slice K"
        (whole, whole1), one = ops.conv2d_g(g, pad=1, act=1, post_relu=True, tile=tile, precision=precision, splitk=0)
        assert one == 1
        for i in (0, 1):
            (alone,), used1 = ops.conv2d_g([g[i]], pad=1, act=1, post_relu=True, tile=tile, precision=precision, splitk=used)
            assert used1 == used
            if tile >= 0:
                assert _same_bits(both[i], alone), f"tile {tile} precision {precision}: group {i} of the split-K launch differs from its own launch with factor {used}"
            worst = _worse(worst, _check(both[i], prs[i], f"split-K group {i}"), _check((whole, whole1)[i], prs[i], f"single pass group {i}"))
        print(f"[conv forms split-K tile {_tn(tile)} precision {precision}] factor {used}")
    _report(f"groups=2 split-K tile {_tn(tile)}", worst)


# --------------------------------------------------------------------------------------------------------------- bias table
@pytest.mark.parametrize("tile", TABLE_TILES)
def test_bias_table(ops, tile):
    """nine distinct random rows: conv without bias plus table[case(oy, ox)], one problem and two problems with two tables"""
    assert tile is not None, "libpf_hip.so could not be loaded at collection"
    worst = 0.0
    for precision in (0, 3):
        if tile >= 0 and tile not in _usable(**dict(Q_TABLE, precision=precision)):
            continue
        for form in TABLE_FORMS:
            for shape in TABLE_SHAPES:
                prs = table_case(form, shape)
                g = [_gpu(pr) for pr in prs]
                (both, _used) = ops.conv2d_g(g, pad=1, tile=tile, precision=precision)
                for i in (0, 1):
                    (alone,), _ = ops.conv2d_g([g[i]], pad=1, tile=tile, precision=precision)
                    if tile >= 0:
                        assert _same_bits(both[i], alone), f"{form} {shape} tile {tile} precision {precision}: group {i} differs from its own launch"
                    worst = _worse(worst, _check(both[i], prs[i], f"{form} {shape} group {i}"), _check(alone, prs[i], f"{form} {shape} alone {i}"))
    _report(f"bias table tile {_tn(tile)}", worst)


def folded_pair(seed, C=32, E=64, Cout=64):
    """Linear(C -> E) followed by a zero-padded 3x3(E -> Cout), folded in fp64 as pf_engine::make_folded documents it:
    W'[o][ci][ky][kx] = sum_e Wp[o][e][ky][kx] Wl[e][ci];  T[o][ky][kx] = sum_e Wp[o][e][ky][kx] bl[e];
    table[3 cy + cx][o] = bp[o] + sum of T[o][ky][kx] over the taps inside the map: the first row (cy = 0) has no tap above (ky = 0), the last (cy = 2) none below
    (ky = 2); columns likewise."""
    wl, bl = _rand((E, C), seed, 1.0 / math.sqrt(C)).double().numpy(), _rand((E,), seed + 1, 0.5).double().numpy()
    wp, bp = _rand((Cout, E, 3, 3), seed + 2, 1.0 / math.sqrt(9 * E)).double().numpy(), _rand((Cout,), seed + 3, 0.1).double().numpy()
    wf = np.einsum("oeyx,ec->ocyx", wp, wl)
    T = np.einsum("oeyx,e->oyx", wp, bl)
    tab = np.zeros((9, Cout))
    for cy in range(3):
        for cx in range(3):
            valid = np.array([[not ((cy == 0 and ky == 0) or (cy == 2 and ky == 2)) and not ((cx == 0 and kx == 0) or (cx == 2 and kx == 2)) for kx in range(3)] for ky in range(3)])
            tab[cy * 3 + cx] = bp + (T * valid[None]).sum((1, 2))
    return wl, bl, wp, bp, wf, tab


@functools.lru_cache(maxsize=None)
def fold_case(shape):
    B, H, W = shape
    wl, bl, wp, bp, wf, tab = folded_pair(_seed("fold"))
    x = _rand((B, H, W, 32), _seed("fold", shape))
    t = torch.from_numpy(x.double().numpy() @ wl.T + bl)                      # the Linear, per pixel
    ref = F.conv2d(t.permute(0, 3, 1, 2), torch.from_numpy(wp), torch.from_numpy(bp), padding=1).permute(0, 2, 3, 1).contiguous().numpy()  # zero padding of the Linear's OUTPUT
    wf32, tab32 = torch.from_numpy(wf).float(), torch.from_numpy(tab).float()
    # the entry gets the fold rounded to fp32: u |W'| |x| summed and u |table| on top of the conv bound
    scale = F.conv2d(x.double().abs().permute(0, 3, 1, 2), torch.from_numpy(np.abs(wf)), None, padding=1).permute(0, 2, 3, 1).numpy()
    bound = TOL * (1.0 + np.abs(ref)) + U * (scale + np.abs(tab).max())
    return {"x": x, "weight": wf32, "bias": tab32, "_ref": ref, "_bound": bound}


@pytest.mark.parametrize("tile", TABLE_TILES)
def test_bias_table_is_the_fold_of_linear_and_padded_conv(ops, tile):
    """which of the nine rows means which border: the fold built here in fp64 exactly as make_folded documents it, run through the entry, against the fp64 UNFOLDED pair
    (Linear, then the 3x3 with zero padding of the Linear's output)"""
    assert tile is not None, "libpf_hip.so could not be loaded at collection"
    worst = 0.0
    for shape in TABLE_SHAPES:
        pr = fold_case(shape)
        (got,), _ = ops.conv2d_g([_gpu(pr)], pad=1, tile=tile)
        worst = _worse(worst, _check(got, pr, f"fold {shape}"))
    _report(f"bias table = fold, tile {_tn(tile)}", worst)


# --------------------------------------------------------------------------------------------------------------- refusals
def test_refusals(ops):
    """every precondition of pf_op_conv2d_g is PF_ERR_ARG before any launch, never a fallback"""
    from perspectivefields_amd.engine import PfError

    names = ops.conv_tiles()
    refused = 0

    def refuse(what, problems, **kw):
        nonlocal refused
        with pytest.raises(PfError):
            ops.conv2d_g(problems, **kw)
        refused += 1
        print(f"[conv forms refusals] refused: {what}")

    ups = _gpu(ups_case("ups64-32", (2, 6, 10)))
    for t in ("128x128p", "sb128x128", "sb128x32", "sbh256x64w8", "wino256x64c"):   # an exact-fp32 tile, linear split tiles, the 8-wave halo tile, a Winograd tile
        assert names.index(t) not in _usable(**Q_UPS)
        refuse(f"ups on {t}", [ups], pad=1, act=1, ups=True, tile=names.index(t))
    refuse("tile id out of range", [ups], pad=1, act=1, ups=True, tile=len(names))
    refuse("ups under the exact bf16 split", [ups], pad=1, act=1, ups=True, precision=3)
    x3 = torch.zeros((1, 3, 4, 64), device="cuda")
    refuse("ups with odd H", [dict(ups, x=x3)], pad=1, ups=True, size=(7, 8))
    refuse("ups with odd W", [dict(ups, x=x3)], pad=1, ups=True, size=(6, 9))
    refuse("ups on a 1x1 kernel (no tile for the automatic choice)", [dict(ups, weight=ups["weight"][:, :, :1, :1].contiguous())], ups=True)
    refuse("ups with stride 2 (no tile for the automatic choice)", [ups], pad=1, stride=2, ups=True)
    x48 = torch.zeros((1, 6, 6, 48), device="cuda")
    refuse("C1 = 48", [{"x": x48, "weight": torch.zeros((32, 48, 3, 3))}], pad=1)
    x32, x16 = torch.zeros((1, 6, 6, 32), device="cuda"), torch.zeros((1, 6, 6, 16), device="cuda")
    refuse("C2 = 16", [{"x": x32, "x2": x16, "weight": torch.zeros((32, 48, 3, 3))}], pad=1)
    tab = torch.zeros((9, 64))
    w64 = torch.zeros((64, 64, 3, 3))
    for H, W in ((1, 5), (5, 1), (1, 1)):
        refuse(f"bias table on a {H} x {W} map", [{"x": torch.zeros((1, H, W, 64), device="cuda"), "weight": w64, "bias": tab}], pad=1)
    x64 = torch.zeros((1, 6, 6, 64), device="cuda")
    for t in ("wino256x64c", "wino256x64d"):
        assert names.index(t) in _usable(B=1, H=6, W=6, C1=64, Cout=64, K=3, pad=1) and names.index(t) not in _usable(B=1, H=6, W=6, C1=64, Cout=64, K=3, pad=1, has_table=True)
        refuse(f"bias table on {t}", [{"x": x64, "weight": w64, "bias": tab}], pad=1, tile=names.index(t))
    head = dict(head_kind=1, head_w=torch.zeros((2, 32)), head_b=torch.zeros(2))
    refuse("fused head on Cout = 64", [dict({"x": x64, "weight": w64}, **head)], pad=1, act=1)
    w32 = torch.zeros((32, 64, 3, 3))
    refuse("fused head on a BN = 64 tile", [dict({"x": x64, "weight": w32}, **head)], pad=1, act=1, tile=names.index("sbh128x64"))
    refuse("fused head on an exact-fp32 tile", [dict({"x": x64, "weight": w32}, **head)], pad=1, act=1, tile=names.index("128x32p"))
    refuse("a head in one group only", [dict({"x": x64, "weight": w32}, **head), {"x": x64, "weight": w32}], pad=1, act=1)
    refuse("head_kind 3", [dict({"x": x64, "weight": w32}, **dict(head, head_kind=3))], pad=1, act=1)
    refuse("three problems", [{"x": x64, "weight": w32}] * 3, pad=1)
    refuse("precision 1", [{"x": x64, "weight": w32}], pad=1, precision=1)
    refuse("split-K factor 1", [{"x": x64, "weight": w32}], pad=1, splitk=1)
    print(f"[conv forms refusals] refused {refused} (bound: all)")
