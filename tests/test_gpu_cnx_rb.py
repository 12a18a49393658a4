"""Row-block fused ConvNeXt block MLP of the 384- / 768-channel stages (cnx_rb.hip, PF_CNX_RB): the kernel through ops.cnx_mlp against torch fp64 and against
the two GEMMs it replaces, the engine with the switch forced on against the GEMM pair and the oracle, determinism, and the built kernels' resources."""
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import pf_oracle
from perspectivefields_amd.config import arch_of, get_cfg
from perspectivefields_amd.synth import synthetic_image, synthetic_state_dict, to_torch
from tests.parity import l1, one_minus_cos

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = "Paramnet-360Cities-edina-centered"
SCALARS = ("pred_roll", "pred_pitch", "pred_vfov", "pred_rel_focal")


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


def _close(got, ref, tol, what):
    got = got.double().cpu()
    ref = ref.double()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err = (got - ref).abs()
    bound = tol * (1.0 + ref.abs())
    worst = float((err / bound).max())
    print(f"[{what}] max err {float(err.max()):.3e}, ratio to bound {worst:.3f}")
    assert worst <= 1.0, f"{what}: max err {float(err.max()):.3e} (ratio to bound {worst:.2f}), ref scale {float(ref.abs().max()):.3e}"


def _with_outlier_channels(x, seed, sigma=100.0):
    """a third of the rows get a `sigma`-sized outlier in channel 0, a third in a random channel, a third both with opposite signs (as test_gpu_ops.py)"""
    x = x.clone()
    flat = x.reshape(-1, x.shape[-1])
    g = torch.Generator().manual_seed(seed)
    ch = torch.randint(0, flat.shape[1], (flat.shape[0],), generator=g)
    sgn = torch.where(torch.rand(flat.shape[0], generator=g) < 0.5, -1.0, 1.0) * sigma * float(flat.std())
    r = torch.arange(flat.shape[0])
    a, b = r % 3 == 0, r % 3 == 1
    flat[a | ~(a | b), 0] += sgn[a | ~(a | b)]
    sel = b | ~(a | b)
    flat[r[sel], ch[sel]] -= sgn[sel]
    return x


def _weights(C):
    w1, b1 = _rand((4 * C, C), 44, 1.0 / math.sqrt(C)), _rand((4 * C,), 45, 0.1)
    g, be = 1 + _rand((C,), 46, 0.3), _rand((C,), 47, 0.2)
    w2, b2, ls = _rand((C, 4 * C), 48, 1.0 / math.sqrt(4 * C)), _rand((C,), 49, 0.1), _rand((C,), 50, 0.5)
    return w1, b1, g, be, w2, b2, ls


def _ref(d, y, w1, b1, g, be, w2, b2, ls):
    C = d.shape[1]
    h = pf_oracle.gelu(F.linear(F.layer_norm(d.double(), (C,), g.double(), be.double(), 1e-6), w1.double(), b1.double()))
    return y.double() + ls.double() * F.linear(h, w2.double(), b2.double())


@pytest.mark.gpu
@pytest.mark.parametrize("C,rows", [(384, 64), (384, 65), (384, 200), (768, 32), (768, 33), (768, 100)])
def test_row_block_convnext_mlp(ops, C, rows):
    """One full block, one full block plus a one-row tail block, several blocks with a ragged tail; rows with 30-sigma common offsets and a constant row.
    Against torch fp64 (LayerNorm 1e-6, erf GELU, y + ls * pwconv2) and against LayerNorm-fused pwconv1 + pwconv2 on the GEMM tiles."""
    d = _rand((rows, C), 41, 1.5) + 30.0 * _rand((rows, 1), 42)
    d[5] = 2.0
    y = _rand((rows, C), 43)
    w1, b1, g, be, w2, b2, ls = _weights(C)
    got = ops.cnx_mlp(d.cuda(), y.cuda(), w1, b1, g, be, 1e-6, w2, b2, ls)
    _close(got, _ref(d, y, w1, b1, g, be, w2, b2, ls), 5e-5, f"row-block ConvNeXt MLP C={C} rows={rows}")
    hid = ops.linear_ln(d.cuda(), w1, b1, g, be, 1e-6, act=2)
    two = ops.linear(hid, w2 * ls[:, None], b2 * ls, res1=y.cuda())
    _close(got, two.double().cpu(), 2e-5, f"row-block ConvNeXt MLP vs two GEMMs C={C} rows={rows}")


@pytest.mark.gpu
@pytest.mark.parametrize("C,rows", [(384, 129), (768, 33)])
def test_row_block_convnext_mlp_outlier_channels(ops, C, rows):
    d = _with_outlier_channels(_rand((rows, C), 141, 1.5) + 10.0 * _rand((rows, 1), 142), 143)
    y = _rand((rows, C), 43)
    w1, b1, g, be, w2, b2, ls = _weights(C)
    got = ops.cnx_mlp(d.cuda(), y.cuda(), w1, b1, g, be, 1e-6, w2, b2, ls)
    _close(got, _ref(d, y, w1, b1, g, be, w2, b2, ls), 5e-5, f"row-block ConvNeXt MLP with outlier channels C={C}")


def _fresh_model(monkeypatch, value):
    from perspectivefields_amd import PerspectiveFields

    monkeypatch.setenv("PF_CNX_RB", str(value))
    return PerspectiveFields(CFG, weights="synthetic:0").eval().cuda()


@pytest.mark.gpu
def test_engine_with_row_block_convnext_mlp_agrees_with_gemm_pair(monkeypatch):
    """PF_CNX_RB=2 (the fused form at any batch) against PF_CNX_RB=0 (the GEMM pair) on fresh engines, batch 3: the dispatch report shows which form ran, the
    workspace stays inside the dry run's, outputs inside the switch-parity bounds, and the forced-on scalars within 1e-4 of the oracle for slot 0."""
    imgs = [synthetic_image(72, 96, seed=700 + i) for i in range(3)]
    off_model = _fresh_model(monkeypatch, 0)
    off = off_model.inference_batch(imgs)
    off_rep = off_model._get_engine().last_dispatch()
    on_model = _fresh_model(monkeypatch, 2)
    on = on_model.inference_batch(imgs)
    on_rep = on_model._get_engine().last_dispatch()
    assert off_rep["cnx_rb_launches"] == 0 and on_rep["cnx_rb_launches"] == 12, (off_rep, on_rep)
    for rep in (off_rep, on_rep):
        assert rep["batch"] == 3 and rep["fork_alloc_conflicts"] == 0 and rep["real_peak_bytes"] <= rep["dry_peak_bytes"], rep
    for i, (a, b) in enumerate(zip(on, off)):
        c = one_minus_cos(a["pred_gravity"].cpu().numpy(), b["pred_gravity"].cpu().numpy()).max()
        e = l1(a["pred_latitude"].cpu().numpy(), b["pred_latitude"].cpu().numpy())
        dd = max(abs(float(a[k]) - float(b[k])) for k in SCALARS)
        print(f"[PF_CNX_RB=2 vs 0 img{i}] 1-cos {c:.2e} latL1 {e:.2e} param {dd:.2e}")
        assert c <= 1e-6 and e <= 1e-5 and dd <= 5e-5
    with torch.no_grad():
        ref = pf_oracle.inference_batch(to_torch(synthetic_state_dict(CFG, 0)), arch_of(get_cfg(CFG)), imgs[:1])[0]
    for k in SCALARS:
        print(f"[PF_CNX_RB=2 vs oracle] {k} {abs(float(on[0][k]) - float(ref[k])):.2e}")
        assert abs(float(on[0][k]) - float(ref[k])) <= 1e-4, (k, float(on[0][k]), float(ref[k]))


@pytest.mark.gpu
def test_engine_row_block_convnext_mlp_stage3_only(monkeypatch):
    """PF_CNX_RB=6 (forced, stage 3 only): the nine 384-channel blocks take the fused kernel, the three 768-channel blocks the GEMM pair; scalars inside the
    switch-parity bound of the all-fused engine."""
    imgs = [synthetic_image(72, 96, seed=700 + i) for i in range(3)]
    s3_model = _fresh_model(monkeypatch, 6)
    s3 = s3_model.inference_batch(imgs)
    rep = s3_model._get_engine().last_dispatch()
    assert rep["cnx_rb_launches"] == 9 and rep["fork_alloc_conflicts"] == 0 and rep["real_peak_bytes"] <= rep["dry_peak_bytes"], rep
    both = _fresh_model(monkeypatch, 2).inference_batch(imgs)
    for a, b in zip(s3, both):
        assert max(abs(float(a[k]) - float(b[k])) for k in SCALARS) <= 5e-5


@pytest.mark.gpu
def test_engine_with_row_block_convnext_mlp_is_deterministic(monkeypatch):
    """PF_CNX_RB=2: three forwards of one batch of 4 are bit-identical, the batch rolled by one gives the rolled outputs bit for bit (a row's result does not
    depend on its place in a block or in the batch), and a forward with the deferred ParamNet branch gives the parameters of a joined forward bit for bit."""
    m = _fresh_model(monkeypatch, 2)
    eng = m._get_engine()
    x = torch.from_numpy(np.stack([m.aug.apply_image(synthetic_image(80, 100, seed=760 + i)) for i in range(4)])).cuda()
    ref = [t.clone() for t in eng.forward(x)]
    torch.cuda.synchronize()
    assert eng.last_dispatch()["cnx_rb_launches"] == 12
    for _ in range(2):
        again = eng.forward(x)
        torch.cuda.synchronize()
        assert all(torch.equal(a, r) for a, r in zip(again, ref))
    rolled = [t.clone() for t in eng.forward(torch.roll(x, 1, 0))]
    torch.cuda.synchronize()
    assert all(torch.equal(a, torch.roll(r, 1, 0)) for a, r in zip(rolled, ref))
    try:
        eng.set_defer_params(True)
        first = eng.forward(x)
        eng.forward(x)                 # the first forward's ParamNet branch runs beside this one
        snap = first[2].clone()        # stream-ordered read: complete once the second forward has been issued
        eng.join_params()
        torch.cuda.synchronize()
        assert torch.equal(snap, ref[2])
    finally:
        eng.set_defer_params(False)


def test_row_block_convnext_mlp_kernels_fit():
    """scripts/kernel_resources.py on the built library (metadata only, no GPU): both kernels are there for gfx950, inside the 160 KB of LDS, with no spilled
    register and no scratch."""
    import importlib.util
    import shutil

    if not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf") or not shutil.which("c++filt"):
        pytest.skip("llvm-readelf / c++filt not available")
    from perspectivefields_amd import build as _b

    lib = _b.build(verbose=False)
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "scripts", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    by = {r["kernel"]: r for r in kr.kernels(lib)}
    for k in ("pf::cnx_rb_kernel<384>", "pf::cnx_rb_kernel<768>"):
        assert k in by, k
        assert by[k]["spill"] == 0 and by[k]["scratch"] == 0 and 0 < by[k]["lds"] <= 160 * 1024, by[k]
