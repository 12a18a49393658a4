"""The saturation watch, producer by producer (-m gpu).  Every kernel that writes a tensor a split-f16 contraction reads carries its own
copy of the watch; the engine-level tests pass as soon as ONE producer counts.  Here each producer is launched on its own through the kernel-level entry points with
pf_op_set_saturation_watch switched on (ops.saturation_watch), and the counter is compared with what a torch fp64 reference of the same op says it must be:

  (a) in window: limit = 1.5 max|ref|                                  -> counter == 0
  (b) limit = max|ref| (1 + 1e-3) -> 0;  limit = max|ref| (1 - 1e-3)   -> >= 1
  (c) the bias of ONE output channel c raised so that |ref[:, c]| >= 2 limit, every other channel <= limit / 2, c in {0, 3, 4, N - 1}
  (d) one channel of chosen rows spiked through the residual input: row 0 alone, then row 0, the last row (ragged tail), both sides of the 32 / 64 / 128-row block
      boundaries and of the image boundary
  (e) one +inf (every producer) / one NaN (sat_watch4 producers) in the residual                                          -> >= 1
  (f) the output with the watch on is bit-identical to the output with it off

Counting rule.  "watch4" producers (pf_kernels.h sat_watch4) count once per stored float4, and (c) / (d) put exactly one channel of a row out of the window, so the
counter equals the number of such rows whatever the kernel's channel grouping.  The GEMM tiles (sat_acc4 / sat_flush) count once per thread: 1 <= counter <= rows,
and exactly 1 for a single element.  Where a limit has to separate reference values it sits a relative 1e-3 -- 20 x the kernels' parity tolerance 5e-5 (1 + |ref|) --
or more away from every one of them: asserted on the reference before anything is launched.  Every check prints `[sat ...]` with the expected count, the counter,
the limit and that margin."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import pf_oracle
from perspectivefields_amd.config import arch_of, get_cfg
from perspectivefields_amd.synth import synthetic_image, synthetic_state_dict, to_torch

pytestmark = pytest.mark.gpu
MARGIN = 1e-3


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


def _f32_up(v):
    f = np.float32(v)
    return float(f if float(f) >= v else np.nextafter(f, np.float32(np.inf)))


def _f32_down(v):
    f = np.float32(v)
    return float(f if float(f) <= v else np.nextafter(f, np.float32(-np.inf)))


def _margin(refs, limit):
    """smallest relative distance between `limit` and a reference magnitude"""
    a = torch.cat([r.reshape(-1) for r in refs]).abs()
    return float(((a - limit).abs() / a.clamp_min(1e-300)).min())


class Producer:
    """One watched launch.  ref(bias, res) -> list of fp64 (rows, N_i) reference outputs (every watched output of the launch); run(bias, res_gpu) -> the same outputs
    from the kernel.  `bias` (N,) is the host bias that lands on output `target` with gain `gain` (N,), `res` (rows, N) its residual input (None: the op has none).
    kind "watch4": counts per stored float4; "tile": a GEMM tile, counts per thread.  nan_counts: False where a ReLU behind the residual turns a NaN into a stored 0."""

    def __init__(self, name, kind, ref, run, bias, res=None, gain=None, target=0, tokens=None, extra_rows=(), nan_counts=True):
        self.name, self.kind, self.ref, self.run, self.bias, self.res, self.target, self.tokens = name, kind, ref, run, bias, res, target, tokens
        self.gain = torch.ones_like(bias) if gain is None else gain
        self.extra_rows, self.nan_counts = tuple(extra_rows), nan_counts


def _spike_rows(p, rows):
    sel = {0, rows - 1}
    for blk in (32, 64, 128):
        if blk < rows:
            sel |= {blk - 1, blk}
    if p.tokens and p.tokens < rows:
        sel |= {p.tokens - 1, p.tokens}
    sel |= {r for r in p.extra_rows if 0 <= r < rows}
    return sorted(sel)


def _scenarios(p, channels_c=None, cases="abcdef"):
    """[(label, limit, bias, res, expect, margin, rows_out)]; expect: "zero", "some" or "rows" (rows_out of them).  All the conditions on the reference are asserted here."""
    base = p.ref(p.bias, p.res)
    mx = max(float(r.abs().max()) for r in base)
    assert mx >= 1.0, (p.name, mx)   # the parity tolerance 5e-5 (1 + |ref|) is then <= 1e-4 |ref| at the values the limits separate
    tgt = base[p.target]
    rows, N = tgt.shape
    out = []
    if "a" in cases:
        lim = _f32_up(1.5 * mx)
        out.append(("a in-window", lim, p.bias, p.res, "zero", _margin(base, lim), 0))
    if "b" in cases:
        # the float32 next OUTSIDE max|ref| (1 +- 1e-3), and one more: the margin below is then >= 1e-3 by two float32 steps, far above the fp64 rounding of its evaluation
        hi = float(np.nextafter(np.float32(_f32_up(mx * (1 + MARGIN))), np.float32(np.inf)))
        lo = float(np.nextafter(np.float32(_f32_down(mx * (1 - MARGIN))), np.float32(-np.inf)))
        for lab, lim, exp in (("b just-inside", hi, "zero"), ("b just-outside", lo, "some")):
            m = _margin(base, lim)
            assert m >= MARGIN, (p.name, lab, lim, mx, m)
            out.append((lab, lim, p.bias, p.res, exp, m, 0 if exp == "zero" else 1))
    lim = _f32_up(4.0 * mx)
    if "c" in cases:
        for c in (channels_c or sorted({0, 3, 4, N - 1})):
            b2 = p.bias.clone()
            b2[c] += (2.0 * lim + 2.0 * mx) / float(p.gain[c])
            ref2 = p.ref(b2, p.res)
            t = ref2[p.target].abs()
            others = t.clone()
            others[:, c] = 0
            rest = max([float(others.max())] + [float(r.abs().max()) for i, r in enumerate(ref2) if i != p.target])
            assert float(t[:, c].min()) >= 2 * lim and rest <= lim / 2, (p.name, c, float(t[:, c].min()), rest, lim)
            out.append((f"c channel {c}", lim, b2, p.res, "rows", _margin(ref2, lim), rows))
    if "d" in cases and p.res is not None:
        ch = 5
        for lab, sel in (("d row 0", [0]), ("d chosen rows", _spike_rows(p, rows))):
            r2 = p.res.clone()
            r2[sel, ch] = 16.0 * mx
            ref2 = p.ref(p.bias, r2)
            t = ref2[p.target].abs()
            others = t.clone()
            others[sel, ch] = 0
            rest = max([float(others.max())] + [float(r.abs().max()) for i, r in enumerate(ref2) if i != p.target])
            assert float(t[sel, ch].min()) >= 2 * lim and rest <= lim / 2, (p.name, lab, float(t[sel, ch].min()), rest, lim)
            out.append((f"{lab} {sel if len(sel) < 12 else len(sel)}", lim, p.bias, r2, "rows", _margin(ref2, lim), len(sel)))
    if "e" in cases and p.res is not None:
        for lab, v in (("e +inf", float("inf")), ("e NaN", float("nan"))):
            if v != v and (p.kind != "watch4" or not p.nan_counts):
                continue   # the GEMM tiles drop a NaN (pf_kernels.h sat_flush); a ReLU behind the residual stores 0 for it
            r2 = p.res.clone()
            r2[rows // 2, 9] = v
            out.append((lab, _f32_up(1.5 * mx), p.bias, r2, "some", float("inf"), 1))
    return out


def _check(ops, p, scen, run=None, kind=None, what=None):
    run, kind, what = run or p.run, kind or p.kind, what or p.name
    off = None
    for lab, lim, bias, res, exp, margin, k in scen:
        rg = None if res is None else res.cuda()
        with ops.saturation_watch(lim) as counter:
            got = run(bias, rg)
            n = int(counter.item())
        if exp == "zero":
            want, ok = "0", n == 0
        elif exp == "some":
            want, ok = ">= 1", n >= 1
        elif kind == "watch4" or k == 1:
            want, ok = str(k), n == k
        else:
            want, ok = f"1..{k}", 1 <= n <= k
        print(f"[sat {what} | {lab}] expected {want}  counter {n}  limit {lim:.6g}  margin of the reference {margin:.3g}")
        assert ok, f"{what} | {lab}: counter {n}, expected {want} (limit {lim:.6g}, margin {margin:.3g})"
        if lab.startswith("a "):   # (f): the watch changes nothing that is stored
            off = run(bias, rg)
            for a, b in zip(got, off):
                assert torch.equal(a, b), f"{what}: output differs with the watch on"
            print(f"[sat {what} | f no side effect] outputs bit-identical with the watch on and off")


def test_watch_counts_every_group_and_is_off_outside_the_block(ops):
    """ops.saturation_watch: with a limit below every output each stored float4 counts once (rows x 128 / 4); after the block -- left normally or by an exception -- the
    same launch adds nothing"""
    rows = 70
    x, w, b = (_rand((rows, 128), 591) * 2.0 + 0.3).cuda(), _rand((128, 128), 592, 1.0 / math.sqrt(128)), 0.1 * _rand((128,), 593)
    with ops.saturation_watch(1e-30) as counter:
        y = ops.thin128(x, w, b)
        n = int(counter.item())
    assert float(y.abs().reshape(rows, 32, 4).amax(-1).min()) > 1e-30
    print(f"[sat thin128 | every group out] expected {rows * 32}  counter {n}  limit 1e-30")
    assert n == rows * 32, n
    ops.thin128(x, w, b)
    with pytest.raises(RuntimeError):
        with ops.saturation_watch(1e-30) as c2:
            raise RuntimeError("left by an exception")
    ops.thin128(x, w, b)
    assert int(counter.item()) == n and int(c2.item()) == 0


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# conv2d / linear: the two GEMM epilogues (igemm_common.h), the Winograd epilogue, the split-K reduce

def _conv_producer(ops, name, x, w, b, stride, pad, variant, tokens, seed, kind="tile", **kw):
    """variant: "res1", "res1+res2+relu" or "planes" (y_sb only)"""
    z = F.conv2d(x.double().permute(0, 3, 1, 2), w.double(), None, stride=stride, padding=pad).permute(0, 2, 3, 1).contiguous()
    shape = tuple(z.shape)
    N = shape[-1]
    z = z.reshape(-1, N)
    r1 = _rand(z.shape, seed)
    r2 = _rand(z.shape, seed + 1) if "res2" in variant else None
    relu = "relu" in variant
    xd = x.cuda()
    r2d = None if r2 is None else r2.cuda().reshape(shape)
    fixed_tile = kw.pop("tile", -1)

    def ref(bias, res):
        y = torch.relu(z + bias.double()) if relu else z + bias.double()   # act = ReLU in the post_relu variant: relu(relu(conv + b) + r1 + r2), the ResidualConvUnit form
        y = y + res.double() + (r2.double() if r2 is not None else 0.0)
        return [torch.relu(y) if relu else y]

    def run(bias, res, tile=None):
        y = ops.conv2d(xd, w, bias, stride=stride, pad=pad, act=1 if relu else 0, res1=res.reshape(shape), res2=r2d, post_relu=relu, tile=fixed_tile if tile is None else tile,
                       planes_out=variant == "planes", planes_fmt="f16x2", **kw)
        return [y.reshape(-1, N)]

    return Producer(f"{name} {variant}", kind, ref, run, b, r1, tokens=tokens, nan_counts=not relu)


def _split_tiles(ops):
    return [(-1, "auto")] + [(i, n) for i, n in enumerate(ops.conv_tiles()) if n.startswith("sb")]


_TILE_RUNS = {}


def _tile_runs(ops, t, B, H, W, Cin, Cout, K, pad):
    """does tile id t run this shape itself (pf_op_conv2d_bench answers -1 for a tile that cannot), or does pf_op_conv2d fall back to the default tile?"""
    key = (t, B, H, W, Cin, Cout, K, pad)
    if key not in _TILE_RUNS:
        _TILE_RUNS[key] = ops.conv2d_bench(B, H, W, Cin, Cout, K, 1, pad, tile=t, iters=1) > 0
    return _TILE_RUNS[key]


@pytest.mark.parametrize("variant", ["res1", "res1+res2+relu", "planes"])
@pytest.mark.parametrize("shape", ["linear 1x1 K64 N64 rows129", "conv3x3 2x9x11 32->32"])
def test_gemm_tile_epilogues(ops, shape, variant):
    """epilogue_nhwc / epilogue_direct of every split tile: the linear tiles on a 1 x 1 layer with a ragged last block, the halo tiles on a 3 x 3 layer whose patches
    are cut by the border; fp32 output with one and with two residuals, and the output as split planes only.  A tile id the entry point refuses (one that cannot run the
    shape, when only planes are asked for: the halo tiles on the 1 x 1 layer) is not applicable; a tile id that cannot run the shape falls back to the default tile, as in test_conv2d_all_tiles: every line
    says which of the two happened, and both tile families must have run a kernel of their own."""
    from perspectivefields_amd.engine import PfError

    if shape.startswith("linear"):
        x, w, b, pad, tokens = _rand((1, 129, 1, 64), 501), _rand((64, 64, 1, 1), 502, 1.0 / 8.0), _rand((64,), 503, 0.1), 0, None
    else:
        x, w, b, pad, tokens = _rand((2, 9, 11, 32), 504), _rand((32, 32, 3, 3), 505, 1.0 / math.sqrt(288)), _rand((32,), 506, 0.1), 1, 99
    p = _conv_producer(ops, shape, x, w, b, 1, pad, variant, tokens, 507, splitk=False)
    scen = _scenarios(p)
    ran, own = 0, {False: 0, True: 0}
    for t, tname in _split_tiles(ops):
        try:
            p.run(p.bias, p.res.cuda(), tile=t)
        except PfError:
            assert variant == "planes", (tname, variant)
            print(f"[sat {p.name} tile {tname}] not applicable: refused for this shape with a planes-only output")
            continue
        mine = t < 0 or _tile_runs(ops, t, *x.shape, w.shape[0], w.shape[2], pad)
        own[tname.startswith("sbh")] += int(mine and t >= 0)
        _check(ops, p, scen, run=lambda bias, res, t=t: p.run(bias, res, tile=t), what=f"{p.name} tile {tname}" + ("" if mine else " (cannot run the shape: the default tile ran)"))
        ran += 1
    print(f"[sat {p.name}] {ran} tile ids checked; kernels of their own: {own[False]} linear tiles, {own[True]} halo tiles")
    assert ran >= (8 if variant == "planes" else 19), ran
    assert own[False] >= 1 and (own[True] >= 1 or variant == "planes" or shape.startswith("linear")), own


@pytest.mark.parametrize("half", [1, 0], ids=["half-patch", "square"])
@pytest.mark.parametrize("tile_name", ["wino256x64c", "wino256x64d"])
@pytest.mark.parametrize("H,W", [(20, 20), (9, 13)])
def test_winograd_epilogue(ops, monkeypatch, H, W, tile_name, half):
    """wino.hip (sat_watch4 on every stored float4): 3 x 3, 256 -> 256 on maps with ragged blocks, in the half-patch geometry (1 <= H mod 16 <= 8) and with square
    patches (PF_WINO_HALF=0, read by the entry point at the call)."""
    monkeypatch.setenv("PF_WINO_HALF", str(half))
    names = ops.conv_tiles()
    tw = names.index(tile_name)
    assert ops.conv2d_bench(1, H, W, 256, 256, 3, 1, 1, tile=tw, iters=1) > 0   # the tile really runs this shape
    x, w, b = _rand((1, H, W, 256), 511), _rand((256, 256, 3, 3), 512, 1.0 / math.sqrt(256 * 9)), _rand((256,), 513, 0.1)
    for variant in ("res1", "res1+res2+relu"):
        p = _conv_producer(ops, f"{tile_name} {H}x{W} {'half' if half else 'square'}", x, w, b, 1, 1, variant, None, 514, kind="watch4", splitk=False, tile=tw)
        _check(ops, p, _scenarios(p))


@pytest.mark.parametrize("splitk", [True, False], ids=["splitk", "no-splitk"])
def test_splitk_output_is_watched(ops, splitk):
    """The MiT stage-1 spatial-reduction conv at batch 1 (8 x 8 stride 8, 64 -> 64 on 40 x 40: K = 4096, M = 25 -- the engine's rule contracts it in K slices).  The
    partial passes hold raw scaled sums; the finished output is written, and watched, by splitk_reduce_kernel (one sat_watch4 per stored float4: exact counts).
    splitk=False is the control: the same layer through a GEMM tile's own epilogue."""
    x, w, b = _rand((1, 40, 40, 64), 521), _rand((64, 64, 8, 8), 522, 1.0 / 64.0), _rand((64,), 523, 0.1)
    for variant in ("res1", "res1+res2+relu") if not splitk else ("res1",):   # (the split-K rule does not take a second residual)
        p = _conv_producer(ops, f"sr8x8s8 {'split-K' if splitk else 'one pass'}", x, w, b, 8, 0, variant, None, 524, kind="watch4" if splitk else "tile", splitk=splitk)
        _check(ops, p, _scenarios(p))
    if splitk:   # the split really ran: another summation order than the one-pass launch (bit-identical would mean one pass)
        r = p.res.cuda()
        one = ops.conv2d(x.cuda(), w, b, stride=8, res1=r.reshape(1, 5, 5, 64), splitk=False)
        assert not torch.equal(p.run(p.bias, r)[0], one.reshape(-1, 64)), "pf_op_conv2d did not split K for this shape"


@pytest.mark.parametrize("K,N,rows", [(64, 256, 129), (96, 384, 33)])
def test_linear_ln_epilogue(ops, K, N, rows):
    """the 1 x 1 LayerNorm-fused form (ConvParams::ln) on every linear split tile that carries it (pf_op_linear_ln refuses a tile id that cannot run the form: no
    silent fall-back here, every id checked is a kernel of its own)"""
    x = _rand((rows, K), 531, 1.5) + 3.0 * _rand((rows, 1), 532)
    w, b = _rand((N, K), 533, 1.0 / math.sqrt(K)), _rand((N,), 534, 0.1)
    g, be = 1 + _rand((K,), 535, 0.3), _rand((K,), 536, 0.2)
    z = F.linear(F.layer_norm(x.double(), (K,), g.double(), be.double(), 1e-6), w.double(), None)
    xd = x.cuda()
    p = Producer(f"linear_ln K{K} N{N} rows{rows}", "tile", lambda bias, res: [z + bias.double() + res.double()],
                 lambda bias, res, tile=-1: [ops.linear_ln(xd, w, bias, g, be, 1e-6, res1=res, tile=tile)], b, _rand((rows, N), 537))
    scen = _scenarios(p)
    ran = 0
    for t, tname in _split_tiles(ops):
        if tname.startswith("sbh"):
            continue   # the halo tiles do not carry the fused form (test_linear_with_fused_layernorm: refused loudly)
        _check(ops, p, scen, run=lambda bias, res, t=t: p.run(bias, res, tile=t), what=f"{p.name} tile {tname}")
        ran += 1
    assert ran >= 13, ran


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# row-block layers (rb_gemm.hip, rb_chain.hip)

@pytest.mark.parametrize("K,N,tokens,images,ln", [(320, 320, 50, 2, True), (768, 320, 70, 3, False)])
def test_rb_linear_epilogue(ops, K, N, tokens, images, ln):
    rows = tokens * images
    x = _rand((rows, K), 541, 1.5)
    w, b = _rand((N, K), 542, 1.0 / math.sqrt(K)), _rand((N,), 543, 0.1)
    g, be = (1 + _rand((K,), 544, 0.3), _rand((K,), 545, 0.2)) if ln else (None, None)
    xn = F.layer_norm(x.double(), (K,), g.double(), be.double(), 1e-6) if ln else x.double()
    z = F.linear(xn, w.double(), None)
    xd = x.cuda()
    p = Producer(f"rb_linear K{K} N{N} {images}x{tokens}{' LN' if ln else ''}", "watch4", lambda bias, res: [z + bias.double() + res.double()],
                 lambda bias, res: [ops.rb_linear(xd, w, bias, tokens, gamma=g, beta=be, eps=1e-6, res=res)], b, _rand((rows, N), 546), tokens=tokens)
    _check(ops, p, _scenarios(p))


def _proj_fc1(ops, tokens, images, scale=1.0):
    """scale: of attn, x and the projection bias, i.e. of x1 -- LayerNorm_2 removes it again, hidden keeps its size"""
    C, rows = 320, tokens * images
    attn, x = _rand((rows, C), 551, 1.2) * scale, (_rand((rows, C), 552, 1.5) + 2.0 * _rand((rows, 1), 553)) * scale
    wp, bp = _rand((C, C), 554, 1.0 / math.sqrt(C)), _rand((C,), 555, 0.1) * scale
    g, be = 1 + _rand((C,), 556, 0.3), _rand((C,), 557, 0.2)
    w1, b1 = _rand((4 * C, C), 558, 1.0 / math.sqrt(C)), _rand((4 * C,), 559, 0.1)
    zp = F.linear(attn.double(), wp.double(), None)
    ad = attn.cuda()

    def ref(pb, fb, xr):
        x1 = xr.double() + zp + pb.double()
        return [x1, F.linear(F.layer_norm(x1, (C,), g.double(), be.double(), 1e-6), w1.double(), fb.double())]

    def run(pb, fb, xr):
        return list(ops.rb_proj_fc1(ad, xr, wp, pb, g, be, 1e-6, w1, fb, tokens))

    return x, bp, b1, ref, run


def test_rb_proj_fc1_both_outputs(ops):
    """x1 = x + proj(attn) and hidden = fc1(LayerNorm_2(x1)) leave one launch; both are watched (x1 where the new token rows are stored, hidden in the chain's
    epilogue).  (c) on each output through its own bias; (d) / (e) through the in-place token stream x, whose reference includes the LayerNorm the spiked row
    then goes through.  (b) needs the output under test to hold the launch's maximum: x1 does with O(1) token rows, hidden with token rows scaled to 0.1."""
    tokens, images = 70, 2
    x, bp, b1, ref, run = _proj_fc1(ops, tokens, images)
    xd = x.cuda()
    px = Producer("rb_proj_fc1 x1", "watch4", lambda bias, res: ref(bias, b1, res), lambda bias, res: run(bias, b1, res), bp, x, target=0, tokens=tokens)
    ph = Producer("rb_proj_fc1 hidden", "watch4", lambda bias, res: ref(bp, bias, x), lambda bias, res: run(bp, bias, xd), b1, None, target=1, tokens=tokens)
    _check(ops, px, _scenarios(px))
    r0 = ref(bp, b1, x)
    assert float(r0[0].abs().max()) >= 2 * float(r0[1].abs().max())   # the limits of (b) above separated values of x1; hidden stayed below half of them
    _check(ops, ph, _scenarios(ph, cases="ac"))   # hidden has no residual of its own: (d), (e) not applicable; its (b) follows
    xs, bps, b1s, refs, runs = _proj_fc1(ops, tokens, images, scale=0.1)
    xsd = xs.cuda()
    r1 = refs(bps, b1s, xs)
    mh = float(r1[1].abs().max())
    assert float(r1[0].abs().max()) <= mh * (1 - MARGIN) / 2   # x1 stays below half of either limit of (b): only hidden can count there
    ph2 = Producer("rb_proj_fc1 hidden (x1 scaled 0.1)", "watch4", lambda bias, res: refs(bps, bias, xs), lambda bias, res: runs(bps, bias, xsd), b1s, None, target=1, tokens=tokens)
    _check(ops, ph2, _scenarios(ph2, cases="abc"))


def test_rb_srkv_window_is_the_attention_kernels(ops):
    """kv is watched against the attention kernel's window for k / v, 4094, whatever limit the caller sets: in window -> 0; four kv channels (no two of them within one
    float4, however it is aligned) driven across it through kv_b -> rows x 4."""
    B, Hr, Wr, C = 2, 6, 7, 320
    x = _rand((B, 2 * Hr, 2 * Wr, C), 561, 1.5) + 2.0 * _rand((B, 2 * Hr, 2 * Wr, 1), 562)
    g1, b1 = 1 + _rand((C,), 563, 0.3), _rand((C,), 564, 0.2)
    wsr, bsr = _rand((C, C, 2, 2), 565, 1.0 / math.sqrt(4 * C)), _rand((C,), 566, 0.1)
    g2, b2 = 1 + _rand((C,), 567, 0.3), _rand((C,), 568, 0.2)
    wkv, bkv = _rand((2 * C, C), 569, 1.0 / math.sqrt(C)), _rand((2 * C,), 570, 0.1)
    xn = F.layer_norm(x.double(), (C,), g1.double(), b1.double(), 1e-6)
    y = F.conv2d(xn.permute(0, 3, 1, 2), wsr.double(), bsr.double(), stride=2).permute(0, 2, 3, 1).reshape(B * Hr * Wr, C)
    z = F.linear(F.layer_norm(y, (C,), g2.double(), b2.double(), 1e-5), wkv.double(), None)
    rows, xd, WIN = B * Hr * Wr, x.cuda(), 4094.0
    base = z + bkv.double()
    mx = float(base.abs().max())
    assert 1.5 * mx <= WIN
    raised = [1, 6, 322, 639]
    bk2 = bkv.clone()
    bk2[raised] += 2 * WIN + 2 * mx
    ref2 = (z + bk2.double()).abs()
    others = ref2.clone()
    others[:, raised] = 0
    assert float(ref2[:, raised].min()) >= 2 * WIN and float(others.max()) <= WIN / 2
    for lab, bias, ref, want in (("a in-window", bkv, base, 0), (f"c channels {raised}", bk2, ref2, rows * len(raised))):
        for lim in (3.0e38, 1.0):   # the caller's limit does not move this window
            with ops.saturation_watch(lim) as counter:
                got = ops.rb_srkv(xd, g1, b1, 1e-6, wsr, bsr, g2, b2, 1e-5, wkv, bias)
                n = int(counter.item())
            print(f"[sat rb_srkv | {lab}, caller's limit {lim:g}] expected {want}  counter {n}  limit 4094 (the kernel's own)  margin of the reference {_margin([ref], WIN):.3g}")
            assert n == want, (lab, lim, n, want)
        assert torch.equal(got, ops.rb_srkv(xd, g1, b1, 1e-6, wsr, bsr, g2, b2, 1e-5, wkv, bias)), "rb_srkv: output differs with the watch on"


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# fused blocks and the specialised layers

def _attn64(ops):
    B, N, M, C = 1, 70, 37, 64
    x, kv = _rand((B * N, C), 571) * 2.0 + 0.5, _rand((B, M, 2 * C), 572)
    g, be = 1.0 + 0.2 * _rand((C,), 573), 0.1 * _rand((C,), 574)
    qw, qb = _rand((C, C), 575, 1.0 / 8.0), 0.1 * _rand((C,), 576)
    pw, pb = _rand((C, C), 577, 1.0 / 8.0), 0.1 * _rand((C,), 578)
    k, v = kv.double()[0, :, :C], kv.double()[0, :, C:]
    kvd = kv.cuda()

    def ref(pbias, xr, qbias=qb):
        xd = xr.double()
        q = F.layer_norm(xd, (C,), g.double(), be.double(), 1e-6) @ qw.double().t() + qbias.double()
        a = ((q @ k.t()) * 0.125).softmax(-1)
        return [xd + (a @ v) @ pw.double().t() + pbias.double()], q

    def run(pbias, xr, qbias=qb):
        return [ops.mit_attn64(xr.reshape(B, N, C), kvd, g, be, 1e-6, qw, qbias, pw, pbias).reshape(B * N, C)]

    return x, qb, pb, ref, run, N


def test_mit_attn64_y(ops):
    """attn_block.hip, the output rows y (q stays far inside its own window, asserted on the reference); (d) / (e) go through x, the residual AND the LayerNorm's input"""
    x, qb, pb, ref, run, N = _attn64(ops)
    assert float(ref(pb, x)[1].abs().max()) <= 8188.0 / 2
    p = Producer("mit_attn64 y", "watch4", lambda bias, res: ref(bias, res)[0], run, pb, x)
    _check(ops, p, _scenarios(p))


def test_mit_attn64_q_window(ops):
    """q never leaves the registers; the kernel watches it against the attention window 8188.  One channel of q_b at 2 x 8188 and limit = 3e38, so that no finite y
    can count: every token row counts (rows of a ragged tile past the end may count again)."""
    x, qb, pb, ref, run, N = _attn64(ops)
    qb2 = qb.clone()
    qb2[3] += 2 * 8188.0 + 2 * float(ref(pb, x)[1].abs().max())
    q2 = ref(pb, x, qb2)[1].abs()
    others = q2.clone()
    others[:, 3] = 0
    assert float(q2[:, 3].min()) >= 2 * 8188.0 and float(others.max()) <= 8188.0 / 2
    for lab, qbias, lo in (("q in window", qb, 0), ("q channel 3 beyond 8188", qb2, N)):
        with ops.saturation_watch(3.0e38) as counter:
            y = run(pb, x.cuda(), qbias)[0]
            n = int(counter.item())
        print(f"[sat mit_attn64 q | {lab}] expected {'0' if lo == 0 else f'>= {lo}'}  counter {n}  limit 8188 (the kernel's own)  margin of the reference {_margin([q2 if lo else ref(pb, x)[1]], 8188.0):.3g}")
        assert (n == 0) if lo == 0 else (n >= lo), (lab, n)
        assert bool(torch.isfinite(y).all())


def test_stem7x7_relu_form(ops):
    """stem7.hip as the engine watches it: the low-level encoder (stride 2, ReLU).  No residual input: (d), (e) not applicable.  The LayerNorm form is not watched by
    the engine and the kernel documents nothing about it: not asserted."""
    B, H, W, stride = 1, 37, 53, 2
    x = _rand((B, H, W, 3), 581) * 60.0
    x4 = torch.cat([x, torch.zeros(B, H, W, 1)], dim=-1).cuda()
    w, b = _rand((64, 3, 7, 7), 582, 1.0 / math.sqrt(147)), 0.1 * _rand((64,), 583)
    z = F.conv2d(x.double().permute(0, 3, 1, 2), w.double(), None, stride=stride, padding=3).permute(0, 2, 3, 1).reshape(-1, 64)
    p = Producer("stem7x7 s2 ReLU", "watch4", lambda bias, res: [torch.relu(z + bias.double())], lambda bias, res: [ops.stem7x7(x4, w, bias, stride, relu=True).reshape(-1, 64)], b)
    _check(ops, p, _scenarios(p))


@pytest.mark.parametrize("rows,res", [(70, True), (70, False), (33, True), (33, False)])
def test_thin128_epilogue(ops, rows, res):
    x = _rand((rows, 128), 591) * 2.0 + 0.3
    w, b = _rand((128, 128), 592, 1.0 / math.sqrt(128)), 0.1 * _rand((128,), 593)
    z = x.double() @ w.double().t()
    xd = x.cuda()
    p = Producer(f"thin128 rows {rows}{' +res' if res else ''}", "watch4", lambda bias, r: [z + bias.double() + (r.double() if r is not None else 0.0)],
                 lambda bias, r: [ops.thin128(xd, w, bias, r)], b, _rand((rows, 128), 594) if res else None)
    _check(ops, p, _scenarios(p))   # without res: (d), (e) not applicable


@pytest.mark.parametrize("C,B,Hs,Ws", [(64, 1, 13, 21), (128, 1, 11, 9)])
def test_mit_mlp_epilogue(ops, C, B, Hs, Ws):
    """mit_mlp.hip: y = x + fc2(GELU(dwconv3x3(fc1(LayerNorm(x))))); (c) through fc2's bias, (d) / (e) through x (rows either side of the 8-row / 8- and 16-column
    patch borders as well)"""
    x = _rand((B * Hs * Ws, C), 601, 1.5) + 2.0 * _rand((B * Hs * Ws, 1), 602)
    w1, b1 = _rand((4 * C, C), 603, 1.0 / math.sqrt(C)), _rand((4 * C,), 604, 0.1)
    g, be = 1 + _rand((C,), 605, 0.3), _rand((C,), 606, 0.2)
    wd, bd = _rand((4 * C, 1, 3, 3), 607, 0.4), _rand((4 * C,), 608, 0.1)
    w2, b2 = _rand((C, 4 * C), 609, 1.0 / math.sqrt(4 * C)), _rand((C,), 610, 0.1)

    def ref(bias, xr):
        xd = xr.double().reshape(B, Hs, Ws, C)
        h = F.linear(F.layer_norm(xd, (C,), g.double(), be.double(), 1e-6), w1.double(), b1.double())
        h = F.conv2d(h.permute(0, 3, 1, 2), wd.double(), bd.double(), padding=1, groups=4 * C).permute(0, 2, 3, 1)
        return [(xd + F.linear(pf_oracle.gelu(h), w2.double(), bias.double())).reshape(-1, C)]

    extra = [7 * Ws, 8 * Ws, 7, 8, 15, 16, 8 * Ws + 7, 8 * Ws + 8]
    p = Producer(f"mit_mlp C{C} {Hs}x{Ws}", "watch4", ref, lambda bias, xr: [ops.mit_mlp(xr.reshape(B, Hs, Ws, C), w1, b1, g, be, 1e-6, wd, bd, w2, bias).reshape(-1, C)],
                 b2, x, extra_rows=extra)
    _check(ops, p, _scenarios(p))


@pytest.mark.parametrize("C,rows", [(96, 128), (192, 300), (384, 65), (768, 33)])
def test_cnx_mlp_epilogue(ops, C, rows):
    """cnx_mlp.hip (C = 96 / 192) and the row-block form cnx_rb.hip (C = 384 / 768): y + ls * pwconv2(GELU(pwconv1(LayerNorm(d)))); (c) through pwconv2's bias (it
    reaches the output scaled by the layer scale), (d) / (e) through the residual stream y"""
    d = _rand((rows, C), 611, 1.5) + 3.0 * _rand((rows, 1), 612)
    w1, b1 = _rand((4 * C, C), 613, 1.0 / math.sqrt(C)), _rand((4 * C,), 614, 0.1)
    g, be = 1 + _rand((C,), 615, 0.3), _rand((C,), 616, 0.2)
    w2, b2 = _rand((C, 4 * C), 617, 1.0 / math.sqrt(4 * C)), _rand((C,), 618, 0.1)
    ls = _rand((C,), 619, 0.5)
    ls = torch.where(ls.abs() < 0.05, torch.full_like(ls, 0.05), ls)   # a layer scale next to zero would need a bias beyond fp32 to move its channel
    h = pf_oracle.gelu(F.linear(F.layer_norm(d.double(), (C,), g.double(), be.double(), 1e-6), w1.double(), b1.double()))
    z = F.linear(h, w2.double(), None)
    dd = d.cuda()
    p = Producer(f"cnx_mlp C{C} rows {rows}", "watch4", lambda bias, y: [y.double() + ls.double() * (z + bias.double())],
                 lambda bias, y: [ops.cnx_mlp(dd, y, w1, b1, g, be, 1e-6, w2, bias, ls)], b2, _rand((rows, C), 620), gain=ls)
    _check(ops, p, _scenarios(p))


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# the engine at a batch where a watched layer runs split-K

def test_engine_watches_the_splitk_sr_conv():
    """A checkpoint whose stage-1 spatial-reduction conv (backbone.block1.0.attn.sr, 8 x 8 stride 8) is scaled so that its output -- read raw by the LayerNorm-fused kv
    GEMM -- leaves the split-f16 window by a factor of 4; the attn.norm LayerNorm behind it removes the scale, so nothing else moves.  At batch 1 the engine contracts
    that layer in K slices (last_dispatch proves it), and it still does at batch 16 (M = 100 B rows are ceil(100 B / 64) tiles of 64 x 64, far below the rule's
    300); the one-pass control is an engine created with PF_SPLITK=0, whose last_dispatch shows no split-K launch.  A model pinned to "fp32" must move its saturation
    counter in ALL three, and "auto" at batch 1 must agree with the oracle on the scaled checkpoint (that half alone proves nothing about the watch: the first "auto"
    batch also looks at the recorded ranges)."""
    import os

    from perspectivefields_amd import PerspectiveFields

    version = "Paramnet-360Cities-edina-centered"
    img = synthetic_image(96, 128, seed=7)
    sd = synthetic_state_dict(version, 0)
    _, _, rng = PerspectiveFields(version, weights=sd).eval().cuda().debug_forward([img], shadow=False, ranges=True)
    kv_in = [r for r in rng if "LN-fused" in r["name"] and "M=100 N=128 K=64" in r["name"] and r["name"].endswith(" x")]
    assert kv_in, [r["name"] for r in rng][:40]
    unscaled = float(min(kv_in, key=lambda r: r["name"])["max_abs"])   # the first block's kv GEMM: its input is the sr conv's output
    factor = np.float32(4.0 * 65504.0 / unscaled)
    sd2 = dict(sd)
    for k in ("backbone.block1.0.attn.sr.weight", "backbone.block1.0.attn.sr.bias"):
        sd2[k] = sd[k] * factor
    m = PerspectiveFields(version, weights=sd2, precision="fp32").eval().cuda()
    eng = m._get_engine()
    s0 = int(eng.saturation_snapshot())
    m.inference_batch([img])
    d1 = eng.last_dispatch()
    s1 = int(eng.saturation_snapshot())
    m.inference_batch([img] * 16)
    d16 = eng.last_dispatch()
    s2 = int(eng.saturation_snapshot())
    old = os.environ.get("PF_SPLITK")
    os.environ["PF_SPLITK"] = "0"   # read by pf_create: this engine never splits K
    try:
        mc = PerspectiveFields(version, weights=sd2, precision="fp32").eval().cuda()
        engc = mc._get_engine()
    finally:
        if old is None:
            del os.environ["PF_SPLITK"]
        else:
            os.environ["PF_SPLITK"] = old
    c0 = int(engc.saturation_snapshot())
    mc.inference_batch([img])
    dc = engc.last_dispatch()
    c1 = int(engc.saturation_snapshot())
    print(f"[sat engine] sr conv output max {unscaled:.4g} x {float(factor):.4g} = 4 windows; counter {s0} -> {s1} (batch 1, {d1['splitk_launches']} split-K launches) -> {s2} "
          f"(batch 16, {d16['splitk_launches']} split-K launches); one-pass control (PF_SPLITK=0, batch 1, {dc['splitk_launches']} split-K launches) {c0} -> {c1}")
    assert d1["batch"] == 1 and d1["splitk_launches"] > 0, d1
    assert d16["batch"] == 16, d16
    assert dc["batch"] == 1 and dc["splitk_launches"] == 0, dc
    assert c1 > c0, "one-pass sr conv (PF_SPLITK=0): the saturation counter did not move"
    assert s1 > s0, "batch 1 (split-K sr conv): the saturation counter did not move"
    assert s2 > s1, "batch 16: the saturation counter did not move"
    ma = PerspectiveFields(version, weights=sd2, precision="auto").eval().cuda()
    out = ma.inference_batch([img])[0]
    assert ma.precision == "fp32_bf16x6", ma.precision_reason
    with torch.no_grad():
        ref = pf_oracle.inference_batch(to_torch(sd2), arch_of(get_cfg(version)), [img])[0]
    g, go = out["pred_gravity_original"].double().cpu(), ref["pred_gravity_original"].double()
    dcos = float((1.0 - (g * go).sum(0) / torch.sqrt((g * g).sum(0) * (go * go).sum(0))).max())
    dlat = float((out["pred_latitude_original"].double().cpu() - ref["pred_latitude_original"].double()).abs().mean())
    dpar = max(abs(float(out[q]) - float(ref[q])) for q in ("pred_roll", "pred_pitch", "pred_vfov", "pred_rel_focal"))
    print(f"[sat engine: auto, batch 1] up 1-cos {dcos:.2e}  latitude L1 {dlat:.2e} deg  ParamNet max|d| {dpar:.2e}")
    assert dcos <= 1e-3 and dlat <= 1e-3 and dpar <= 1e-3, (dcos, dlat, dpar)
