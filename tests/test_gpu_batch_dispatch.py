"""Which kernels the engine launches, on which streams, out of which scratch, is decided per forward from the batch size and the PF_* switches (engine.hip: pf_create;
engine_forward.hip: mit(), conv_g).  The op tests check every kernel against an fp64 reference; this file checks the DECISION: every switch at the batches where the paths it switches
are live, with the dispatch report (Engine.last_dispatch) as the witness that the switch acted at all.

Every cell is a configuration a user can select.  Inputs are 320 x 320 uint8 images with a distinct seed per batch slot: identical images in both halves of a batch
would hide a cross-stream scratch race (both streams would write the same bytes).

The property most checks rest on is SLOT INVARIANCE: per-image arithmetic in this engine does not depend on the image's slot in the batch, so the forward of a rolled
batch is the rolled forward, bit for bit.  No tolerance is involved, which makes a scratch race between the two streams of the stage-3 split or a slot-dependent tile
bug visible.  No configuration below is exempt.

Cells that were dropped because the switch cannot act at the batch (the report would equal the default's -- a dead cell):
  * PF_S3_SPLIT=0 at B = 32: the default splits only when each HALF passes the row-block gate (rb_gate(rb_half), 192 row blocks: B = 64); run at B = 64.
  * PF_S3_SPLIT=2 at B = 64: the default already splits there; run at B = 32 (live) and at 16 / 17 / 31 (edges: the gate must refuse).
  * PF_THIN128=1 at B >= 16: the default takes the thin kernel from 25 600 rows (B = 16) on; run at B = 4, the only tested batch below the gate.
  * PF_THIN128=0 at B = 4: the default does not take the thin kernel there.
Batch 4 is the one edge the workspace dry run shows (tests/test_host_logic.py::test_workspace_dry_run_for_every_batch_and_configuration) and is where the side-stream
forks and the stage-2 one-kernel Mlp begin; it is run for the default, PF_THIN128=1 and PF_SIDE_STREAM=0."""
import ctypes
import gc
import time

import numpy as np
import pytest
import torch

from oracle import pf_oracle
from perspectivefields_amd.config import arch_of, get_cfg
from perspectivefields_amd.synth import synthetic_image, synthetic_state_dict, to_torch
from tests.parity import TOL_COS, TOL_LAT_L1, TOL_PARAM, assert_fields_close, one_minus_cos

pytestmark = pytest.mark.gpu

CASES = {"centered": "Paramnet-360Cities-edina-centered", "uncentered": "Paramnet-360Cities-edina-uncentered", "persnet": "PersNet-360Cities"}
NET = 320
SEED0 = 3000            # slot i of every batch is synthetic_image(320, 320, seed=SEED0 + i): batch B is the first B images of one pool
PARAM_KEYS = ("pred_roll", "pred_pitch", "pred_vfov", "pred_rel_focal")
PEAKS = ("real_peak_bytes", "dry_peak_bytes")

_pool = {}
_oracle = {}
_t0 = time.time()


def image(i):
    if i not in _pool:
        _pool[i] = synthetic_image(NET, NET, seed=SEED0 + i)
    return _pool[i]


def batch(B, first=0):
    return torch.from_numpy(np.stack([image(first + i) for i in range(B)])).cuda()


# pool images the oracle is asked for: slots 0, B/2 - 1, B/2, B - 1 of the batches 4, 16, 17, 31, 32, 64 (centered) and of 64 (the other two architectures)
ORACLE_IMAGES = {"centered": (0, 1, 2, 3, 7, 8, 14, 15, 16, 30, 31, 32, 63), "uncentered": (0, 31, 32, 63), "persnet": (0, 31, 32, 63)}


def oracle(tag, i):
    """fp64 CPU oracle of pool image i: computed once per architecture for all of ORACLE_IMAGES[tag] (the oracle has no cross-image arithmetic) and kept for every cell"""
    if (tag, i) not in _oracle:
        todo = [j for j in ORACLE_IMAGES[tag] if (tag, j) not in _oracle] if i in ORACLE_IMAGES[tag] else [i]
        sd, arch = to_torch(synthetic_state_dict(CASES[tag], 0)), arch_of(get_cfg(CASES[tag]))
        with torch.no_grad():
            for k in range(0, len(todo), 7):
                for j, r in zip(todo[k:k + 7], pf_oracle.inference_batch(sd, arch, [image(j) for j in todo[k:k + 7]], dtype=torch.float64)):
                    _oracle[(tag, j)] = {key: v for key, v in r.items() if key.startswith("pred_")}
    return _oracle[(tag, i)]


def make(tag, env, monkeypatch, precision="fp32"):
    """a fresh engine created AFTER the switches are set (pf_create reads them)"""
    from perspectivefields_amd import PerspectiveFields

    with monkeypatch.context() as mp:
        for k, v in env.items():
            mp.setenv(k, v)
        m = PerspectiveFields(CASES[tag], weights="synthetic:0", precision=precision).eval().cuda()
        eng = m._get_engine()
    return m, eng


def drop():
    """after the caller has let go of its engine: weights, workspace (7 GB at B = 64) and cached blocks go back to the device"""
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def fwd(eng, x):
    out = eng.forward(x)
    rep = eng.last_dispatch()
    assert rep["batch"] == x.shape[0]
    assert rep["fork_alloc_conflicts"] == 0, f"two streams allocated from one workspace offset: {rep}"
    assert 0 < rep["real_peak_bytes"] <= rep["dry_peak_bytes"], f"the forward allocated past the dry run's size: {rep}"
    return out, rep


def same(a, b):
    return all((u is None and v is None) or torch.equal(u, v) for u, v in zip(a, b))


def rolled(out, s):
    return tuple(None if t is None else torch.roll(t, s, 0) for t in out)


def check_run_to_run_and_slots(eng, x, what):
    """-> (outputs, report); three forwards bit-identical; the forward of the rolled batch is the rolled forward"""
    out, rep = fwd(eng, x)
    for k in range(2):
        again, rep2 = fwd(eng, x)
        assert rep2 == rep, f"{what}: the dispatch changed between two forwards of one input: {rep} / {rep2}"
        assert same(out, again), f"{what}: run {k + 2} differs from run 1"
    B = x.shape[0]
    for s in sorted({B // 2, 1}):
        got, _ = fwd(eng, torch.roll(x, s, 0))
        want = rolled(out, s)
        if not same(got, want):
            bad = sorted({int(i) for g, w in zip(got, want) if g is not None for i in torch.nonzero((g != w).flatten(1).any(1)).flatten().tolist()})
            raise AssertionError(f"{what}: slot invariance broken by a roll of {s}: rolled-batch slots {bad} differ from the unrolled forward")
    return out, rep


def scalars(m, params):
    d = m._param_dicts(params.cpu())
    return np.array([[float(e[k]) for k in PARAM_KEYS] for e in d], dtype=np.float64)


def check_oracle(m, eng, tag, out, slots, first, what):
    """the project's tolerances (tests/parity.py) on the named slots; prints the largest per-pixel |latitude error| in degrees (no threshold: a reference point)"""
    pg, pl, pr = out
    idx = torch.tensor(slots, device=pg.device)
    res = m._assemble(eng, pg[idx], pl[idx], None if pr is None else pr[idx], [(NET, NET)] * len(slots))
    worst = 0.0
    for r, i in zip(res, slots):
        o = oracle(tag, first + i)
        if pr is None and pg.shape[1] > 2:
            # classification heads (PersNet): the bounds of test_gpu_e2e.py::test_persnet_vs_golden -- logits atol 3e-4 / rtol 2e-4, at most 2e-3 of the pixels with another
            # argmax bin, at most 5e-3 of the decoded pixels beyond the field tolerances (a flipped bin moves a pixel by a whole bin)
            for key in ("pred_gravity", "pred_latitude"):
                np.testing.assert_allclose(r[key][:, 8::16, 8::16].cpu().numpy(), o[key][:, 8::16, 8::16].numpy(), atol=3e-4, rtol=2e-4, err_msg=f"{what} slot {i} {key}")
                flip = float((r[key].argmax(0).cpu() != o[key].argmax(0)).double().mean())
                assert flip <= 2e-3, f"{what} slot {i}: {key} argmax differs on {flip:.2e} of the pixels"
            dl = np.abs(r["pred_latitude_original"].cpu().numpy().astype(np.float64) - o["pred_latitude_original"].numpy().astype(np.float64))
            assert np.mean(dl > TOL_LAT_L1) <= 5e-3, f"{what} slot {i}"
            assert np.mean(one_minus_cos(r["pred_gravity_original"].cpu().numpy(), o["pred_gravity_original"].numpy()) > TOL_COS) <= 5e-3, f"{what} slot {i}"
            worst = max(worst, float(dl.max()))
            continue
        assert_fields_close(r["pred_gravity"].cpu().numpy(), o["pred_gravity"].numpy(), r["pred_latitude"].cpu().numpy(), o["pred_latitude"].numpy(), f"{what} slot {i} 320")
        assert_fields_close(r["pred_gravity_original"].cpu().numpy(), o["pred_gravity_original"].numpy(),
                            r["pred_latitude_original"].cpu().numpy(), o["pred_latitude_original"].numpy(), f"{what} slot {i} orig")
        if pr is not None:
            keys = [k for k, v in r.items() if k.startswith("pred_") and hasattr(v, "numel") and v.numel() == 1 and k in o]   # every scalar both sides name
            assert len(keys) >= 4, keys
            for k in keys:
                assert abs(float(r[k]) - float(o[k])) <= TOL_PARAM, (what, i, k, float(r[k]), float(o[k]))
        worst = max(worst, float(np.abs(r["pred_latitude_original"].cpu().numpy().astype(np.float64) - o["pred_latitude_original"].numpy().astype(np.float64)).max()))
    print(f"[{what}] slots {slots} vs fp64 oracle: inside TOL_COS {TOL_COS} / TOL_LAT_L1 {TOL_LAT_L1} / TOL_PARAM {TOL_PARAM}; max per-pixel |latitude error| {worst:.3e} deg")
    return worst


def check_vs_default(m, out, ref, what):
    """every slot against the default engine at the same batch: the numbers of the switch-parity tests in test_gpu_e2e.py (1-cos 1e-6, latitude L1 1e-5, scalars 5e-5)"""
    (pg, pl, pr), (rg, rl, rr) = out, ref
    a, b = pg.double(), rg.double()
    c = (1.0 - (a * b).sum(1) / ((a * a).sum(1) * (b * b).sum(1)).sqrt()).flatten(1).max(1).values
    e = (pl.double() - rl.double()).abs().flatten(1).mean(1)
    d = np.abs(scalars(m, pr) - scalars(m, rr)).max(1)
    print(f"[{what} vs default, {pg.shape[0]} slots] 1-cos max {float(c.max()):.2e} latL1 max {float(e.max()):.2e} scalars max {d.max():.2e}")
    assert float(c.max()) <= 1e-6, f"{what}: slot {int(c.argmax())} 1-cos {float(c.max()):.3e}"
    assert float(e.max()) <= 1e-5, f"{what}: slot {int(e.argmax())} latitude L1 {float(e.max()):.3e}"
    assert d.max() <= 5e-5, f"{what}: slot {int(d.argmax())} scalars {d.max():.3e}"


def oracle_slots(B):
    return sorted({0, B // 2 - 1, B // 2, B - 1})


def sans_peaks(rep):
    return {k: v for k, v in rep.items() if k not in PEAKS}


# ------------------------------------------------------------------------------------------------------------------ C1: switch x batch matrix
_default = {}   # batch -> (outputs, report) of the default engine


@pytest.fixture(scope="module")
def default_runs():
    """the default engine at every batch of the matrix: its outputs (kept on the device: ~80 MB per 64 images) and dispatch reports, checked like every other cell"""
    if not _default:
        mp = pytest.MonkeyPatch()
        try:
            m, eng = make("centered", {}, mp)
        finally:
            mp.undo()
        for B in (4, 16, 17, 31, 32, 64):
            _default[B] = check_run_to_run_and_slots(eng, batch(B), f"default B={B}")
            print(f"[default B={B}] {_default[B][1]}")
        _default["model"] = (m, eng)
    return _default


def test_default_engine_at_the_batch_gates(default_runs):
    """The default configuration at 4 (forks and the stage-2 one-kernel Mlp begin), 16 (thin128 begins; the split's B >= 16 edge), 17 and 31 (odd: must not split),
    32 (row-block forms of stage 3) and 64 (the stage-3 split): what the report must show at each, run-to-run and slot invariance (in the fixture), and the fp64
    oracle on slots 0, B/2 - 1, B/2, B - 1.

    Largest per-pixel |latitude error| against the oracle seen for this cell on the four slots (degrees at 320 x 320, synthetic weights; no threshold, a reference
    point for later changes): B = 4: 3.14e-03, 16: 9.86e-03, 17: 5.53e-03, 31: 4.67e-03, 32: 6.04e-03, 64: 5.15e-03 (the mean, latitude L1, is bounded by TOL_LAT_L1).
    The other cells of the matrix stayed between 3.1e-03 and 1.0e-02."""
    m, eng = default_runs["model"]
    rep = {B: default_runs[B][1] for B in (4, 16, 17, 31, 32, 64)}
    for B, r in rep.items():
        assert r["forks"] > 0 and r["splitk_launches"] > 0 and r["wino_launches"] > 0 and r["wino_half_launches"] > 0 and r["attn64_launches"] > 0, (B, r)
        assert r["mit_mlp_fused_launches"] > 0, (B, r)
        assert (r["thin128_launches"] > 0) == (B >= 16), (B, r)
        assert (r["rb_launches"] > 0) == (B >= 31), (B, r)        # 7 row blocks per image at stage 3, gate 192 with a last round >= 3/4 full: 28 ... 36, 55 ... 73
        assert r["s3_split_taken"] == (1 if B == 64 else 0), (B, r)   # each half must pass the row-block gate, and the batch be even
    for B in rep:
        check_oracle(m, eng, "centered", default_runs[B][0], oracle_slots(B), 0, f"default B={B}")


def _expect(col, rel):
    """precondition on one report column against the default engine's at the same batch"""
    def f(r, d):
        v, w = r[col], d[col]
        ok = {"zero": v == 0 and w > 0, "more": v > w, "differs": v != w, "plus1": v == w + 1, "one": v == 1 and w == 0, "none": v == 0 and w == 1}[rel]
        assert ok, f"the switch did not act: {col} = {v}, default {w} (expected '{rel}')"
    return f


# name, environment, {batch: [preconditions]}.  A batch listed with an empty list is an EDGE: the report must equal the default's there (stated below, not a dead cell).
MATRIX = [
    ("PF_FUSE_LN=0", {"PF_FUSE_LN": "0"}, {32: [_expect("ln_kernel_launches", "more")], 64: [_expect("ln_kernel_launches", "more")]}),
    ("PF_RB_CHAIN=0", {"PF_RB_CHAIN": "0"}, {32: [_expect("rb_launches", "zero")], 64: [_expect("rb_launches", "zero"), _expect("s3_split_taken", "none")]}),
    ("PF_RB_CHAIN=28", {"PF_RB_CHAIN": "28"}, {32: [_expect("rb_launches", "differs")], 64: [_expect("rb_launches", "differs")]}),
    ("PF_RB_CHAIN=31", {"PF_RB_CHAIN": "31"}, {32: [_expect("rb_launches", "differs")], 64: [_expect("rb_launches", "differs")]}),
    ("PF_RB_CHAIN=127", {"PF_RB_CHAIN": "127"}, {32: [_expect("rb_launches", "differs")], 64: [_expect("rb_launches", "differs")]}),
    ("PF_S3_SPLIT=0", {"PF_S3_SPLIT": "0"}, {64: [_expect("s3_split_taken", "none")]}),
    ("PF_S3_SPLIT=2", {"PF_S3_SPLIT": "2"}, {16: [], 17: [], 31: [], 32: [_expect("s3_split_taken", "one")]}),   # 16: 112 row blocks < 192; 17, 31: odd
    ("PF_SPLITK=0", {"PF_SPLITK": "0"}, {32: [_expect("splitk_launches", "zero")], 64: [_expect("splitk_launches", "zero")]}),
    ("PF_SIDE_STREAM=0", {"PF_SIDE_STREAM": "0"}, {4: [_expect("forks", "zero")], 32: [_expect("forks", "zero")], 64: [_expect("forks", "zero"), _expect("s3_split_taken", "none")]}),
    ("PF_SIDE_STREAM=2", {"PF_SIDE_STREAM": "2"}, {32: [_expect("forks", "plus1")], 64: [_expect("forks", "plus1")]}),
    ("PF_THIN128=0", {"PF_THIN128": "0"}, {32: [_expect("thin128_launches", "zero")], 64: [_expect("thin128_launches", "zero")]}),
    ("PF_THIN128=1", {"PF_THIN128": "1"}, {4: [_expect("thin128_launches", "more")]}),
    ("PF_WINO=0", {"PF_WINO": "0"}, {32: [_expect("wino_launches", "zero")], 64: [_expect("wino_launches", "zero")]}),
    ("PF_WINO_HALF=0", {"PF_WINO_HALF": "0"}, {32: [_expect("wino_half_launches", "zero")], 64: [_expect("wino_half_launches", "zero")]}),
    ("PF_FUSE_MIT_MLP=0", {"PF_FUSE_MIT_MLP": "0"}, {32: [_expect("mit_mlp_fused_launches", "zero")], 64: [_expect("mit_mlp_fused_launches", "zero")]}),
    ("PF_ATTN64=0", {"PF_ATTN64": "0"}, {32: [_expect("attn64_launches", "zero")], 64: [_expect("attn64_launches", "zero")]}),
    ("PF_SBA=1", {"PF_SBA": "1"}, {32: [_expect("sb_tensors", "more"), _expect("rb_launches", "zero")], 64: [_expect("sb_tensors", "more"), _expect("s3_split_taken", "none")]}),
    ("PF_SBA_HEADS=1", {"PF_SBA_HEADS": "1"}, {32: [_expect("sb_tensors", "more")], 64: [_expect("sb_tensors", "more")]}),
]


@pytest.mark.parametrize("name,env,cells", MATRIX, ids=[c[0] for c in MATRIX])
def test_switch_at_the_batches_where_it_acts(name, env, cells, default_runs, monkeypatch):
    """One switch, a fresh engine, at every batch listed for it: the dispatch report shows that the switch acted (a cell whose report equals the default's fails as
    vacuous; at an edge batch it must equal it), no fork window with two allocating streams, the real workspace peak inside the dry run's; three forwards are
    bit-identical; the rolled batch gives the rolled outputs bit for bit; slots 0, B/2 - 1, B/2, B - 1 against the fp64 oracle with the project's tolerances;
    every slot against the default engine with the switch-parity tests' bounds."""
    m, eng = make("centered", env, monkeypatch)
    try:
        for B, pre in cells.items():
            what = f"{name} B={B}"
            out, rep = check_run_to_run_and_slots(eng, batch(B), what)
            dout, drep = default_runs[B]
            print(f"[{what}] {rep}")
            if pre:
                assert sans_peaks(rep) != sans_peaks(drep), f"{what}: vacuous cell, the dispatch report equals the default engine's: {rep}"
                for p in pre:
                    p(rep, drep)
            else:
                assert sans_peaks(rep) == sans_peaks(drep), f"{what}: the switch must not act at this batch: {rep} / default {drep}"
            check_oracle(m, eng, "centered", out, oracle_slots(B), 0, what)
            check_vs_default(m, out, dout, what)
    finally:
        m = eng = None
        drop()


@pytest.mark.parametrize("name,env", [("PF_FUSE_LN=0", {"PF_FUSE_LN": "0"}), ("PF_RB_CHAIN=28", {"PF_RB_CHAIN": "28"})])
def test_stage3_split_with_allocating_halves(name, env, default_runs, monkeypatch):
    """The configurations in which a half-batch block of stage 3 ALLOCATES (the sr conv goes through conv_g, whose split-K partial comes from the bump allocator:
    M = 3 200 rows per half at B = 64 or, forced with PF_S3_SPLIT=2, 1 600 at B = 32).  The second half runs on a copy of the allocator: split, both streams
    would take their partial from one offset.  The split's gate asks a dry walk of one half-batch block and refuses when it allocates, so here
    s3_split_taken == 0 is the asserted precondition (were the gate to let these through, fork_alloc_conflicts > 0 fails every forward in fwd()).  With the
    default PF_S3_SPLIT at B = 16, 17, 31, 64 and PF_S3_SPLIT=2 at B = 32: the full cell checks, and split-on against PF_S3_SPLIT=0 bit for bit, also with the
    deferred ParamNet branch."""
    runs = {}
    for split in ("0", "1", "2"):
        m, eng = make("centered", dict(env, PF_S3_SPLIT=split), monkeypatch)
        try:
            for B in ((32, 64) if split == "0" else (16, 17, 31, 64) if split == "1" else (32,)):
                what = f"{name} PF_S3_SPLIT={split} B={B}"
                out, rep = check_run_to_run_and_slots(eng, batch(B), what)
                print(f"[{what}] {rep}")
                assert rep["s3_split_taken"] == 0, f"{what}: the split ran although its halves allocate: {rep}"
                if split != "0":
                    drep = default_runs[B][1]
                    if B >= 32:   # (below the row-block gate PF_RB_CHAIN is inert: 16 / 17 / 31 are the split's edges, where only "no split" is claimed)
                        assert sans_peaks(rep) != sans_peaks(drep), f"{what}: vacuous cell: {rep} / default {drep}"
                    check_oracle(m, eng, "centered", out, oracle_slots(B), 0, what)
                    check_vs_default(m, out, default_runs[B][0], what)
                eng.set_defer_params(True)
                deferred = [eng.forward(batch(B)) for _ in range(3)]
                eng.set_defer_params(False)
                torch.cuda.synchronize()
                assert eng.last_dispatch()["fork_alloc_conflicts"] == 0
                for k, d in enumerate(deferred):
                    assert same(out, d), f"{what}: forward {k} with the deferred ParamNet branch differs from the joined forward"
                runs[(split, B)] = out
        finally:
            m = eng = None
            drop()
    assert same(runs[("2", 32)], runs[("0", 32)]), f"{name}: PF_S3_SPLIT=2 differs from PF_S3_SPLIT=0 at B = 32"
    assert same(runs[("1", 64)], runs[("0", 64)]), f"{name}: the default PF_S3_SPLIT differs from PF_S3_SPLIT=0 at B = 64"


def test_stage3_split_default_forms_on_against_off(default_runs, monkeypatch):
    """The split where it IS taken (default forms: no allocation in a half), also with the deferred ParamNet branch beside it, against PF_S3_SPLIT=0.
    B = 32 with PF_S3_SPLIT=2: bit for bit.  B = 64 (the default): NOT bit for bit, and not by a race -- the split forward is run-to-run and slot invariant, and a
    roll by 32 swaps the halves between the two streams.  The one launch of a half-batch block that goes through the tile table is the LayerNorm-fused q GEMM, and
    the table is keyed by the row count: 25 600 rows (unsplit) take `sb128x64`, 12 800 rows (a half) `sb64x64f2`: another tile, other roundings.  Checked once by
    hand: with one tile forced for both row counts (PF_CONV_TILE=17, no table; process-wide, so not a test) the two walks are bit-identical, while forcing the
    attention kernel's query-tile count (PF_ATTN_QT, the other batch-dependent launch parameter) changes nothing.  (At B = 32 both walks are bit-identical.)  Seen: 1-cos 6.2e-08, latitude L1 3.5e-07, scalars 1.1e-05 over the 64 slots.  So
    at B = 64 the bound is the switch-parity tests' (two tile choices for one GEMM, as with any other switch): 1e-6 / 1e-5 / 5e-5 on every slot."""
    outs = {}
    for split, cells in (("0", ((64, 0), (32, 0))), ("2", ((32, 1),)), ("1", ((64, 1),))):
        m, eng = make("centered", {"PF_S3_SPLIT": split}, monkeypatch)
        try:
            for B, taken in cells:
                out, rep = fwd(eng, batch(B))
                assert rep["s3_split_taken"] == taken, (split, B, rep)
                eng.set_defer_params(True)
                deferred = [eng.forward(batch(B)) for _ in range(3)]
                eng.set_defer_params(False)
                torch.cuda.synchronize()
                assert eng.last_dispatch()["s3_split_taken"] == taken and eng.last_dispatch()["fork_alloc_conflicts"] == 0
                for d in deferred:
                    assert same(out, d), (split, B)
                outs[(split, B)] = out
        finally:
            m = eng = None
            drop()
    assert same(outs[("2", 32)], outs[("0", 32)]), "PF_S3_SPLIT=2 differs from PF_S3_SPLIT=0 at B = 32"
    assert same(outs[("1", 64)], default_runs[64][0]) and same(outs[("0", 32)], default_runs[32][0])   # an explicit PF_S3_SPLIT=1 is the default
    print(f"[split on vs off B=64] bit-identical: {same(outs[('1', 64)], outs[('0', 64)])}")
    check_vs_default(default_runs["model"][0], outs[("0", 64)], outs[("1", 64)], "PF_S3_SPLIT=0 B=64 against the split")


# ------------------------------------------------------------------------------------------------------------------ C3: workspace
GUARD = 1 << 20
PATTERN = 0xA5
WS_CONFIGS = [{}, {"PF_FUSE_LN": "0"}, {"PF_RB_CHAIN": "0"}, {"PF_RB_CHAIN": "28"}, {"PF_SPLITK": "0"}, {"PF_SBA": "1"}, {"PF_FOLD_MLP": "0"}, {"PF_FUSE_UPSAMPLE": "0"}]


def guarded_forward(eng, x, short=0):
    """pf_forward_u8 through the C ABI in exactly pf_workspace_bytes(B) - short bytes, placed between two guard bands of 1 MiB of a fixed byte -> (rc, intact, report)"""
    B = x.shape[0]
    need = eng.workspace_bytes(B)
    buf = torch.full((need + 2 * GUARD,), PATTERN, dtype=torch.uint8, device="cuda")
    pg = torch.empty((B, eng.gravity_channels, NET, NET), dtype=torch.float32, device="cuda")
    pl = torch.empty((B, eng.latitude_channels, NET, NET), dtype=torch.float32, device="cuda")
    pr = torch.empty((B, 8), dtype=torch.float32, device="cuda") if eng.param_outputs else None
    torch.cuda.synchronize()
    rc = eng.lib.pf_forward_u8(eng._h, B, x.data_ptr(), pg.data_ptr(), pl.data_ptr(), pr.data_ptr() if pr is not None else None, buf.data_ptr() + GUARD, need - short,
                               ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    eng.join_params()
    torch.cuda.synchronize()
    intact = bool((buf[:GUARD] == PATTERN).all()) and bool((buf[GUARD + need:] == PATTERN).all())
    rep = eng.last_dispatch()
    del buf
    return rc, intact, rep, (pg, pl, pr)


@pytest.mark.parametrize("env", WS_CONFIGS, ids=["default" if not e else "_".join(f"{k}={v}" for k, v in e.items()) for e in WS_CONFIGS])
def test_workspace_is_what_the_dry_run_sized(env, monkeypatch):
    """The forward in a workspace of exactly pf_workspace_bytes(B) bytes between two guard bands: both bands untouched, the real peak (main and ParamNet region)
    inside the dry run's.  B in {1, 16, 32, 64, 81} for the default configuration, B = 64 for every configuration that changes allocation; each also with the
    deferred ParamNet branch and in the exact scheme (3 planes per split tensor instead of 2).  One byte short: PF_ERR_WORKSPACE before any launch."""
    m, eng = make("centered", env, monkeypatch)
    try:
        for B in ((1, 16, 32, 64, 81) if not env else (64,)):
            x = batch(min(B, 64)) if B <= 64 else torch.cat([batch(64), batch(B - 64)])
            for precision in ("fp32", "fp32_bf16x6"):
                eng.set_precision(precision)
                for defer in (False, True):
                    eng.set_defer_params(defer)
                    what = f"{env or 'default'} B={B} {precision} defer={defer}"
                    rc, intact, rep, out = guarded_forward(eng, x)
                    assert rc == 0, (what, eng.lib.pf_last_error(eng._h))
                    assert intact, f"{what}: a guard band around the workspace was written"
                    assert rep["batch"] == B and 0 < rep["real_peak_bytes"] <= rep["dry_peak_bytes"] <= eng.workspace_bytes(B), (what, rep)
                    assert rep["fork_alloc_conflicts"] == 0, (what, rep)
                    assert bool(torch.isfinite(out[0]).all()) and bool(torch.isfinite(out[2]).all()), what
                eng.set_defer_params(False)
            eng.set_precision("fp32")
            before = eng.last_dispatch()
            rc, intact, rep, _ = guarded_forward(eng, x, short=1)
            assert rc == -4 and intact and rep == before, f"B={B}: a workspace one byte short must be refused before any launch (rc {rc})"
            assert b"workspace too small" in eng.lib.pf_last_error(eng._h)
    finally:
        m = eng = None
        drop()


# ------------------------------------------------------------------------------------------------------------------ C2: other architectures, graph replay
@pytest.mark.parametrize("tag", ["uncentered", "persnet"])
def test_other_architectures_at_batch_64(tag, monkeypatch):
    """Only the centered model is otherwise run at B >= 32: the uncentered ParamNet model and PersNet (classification heads, no ParamNet) at B = 64 in the default
    configuration: the split is taken, slot invariance, the fp64 oracle on slots 0 / 31 / 32 / 63."""
    m, eng = make(tag, {}, monkeypatch)
    try:
        out, rep = check_run_to_run_and_slots(eng, batch(64), f"{tag} B=64")
        print(f"[{tag} B=64] {rep}")
        assert rep["s3_split_taken"] == 1 and rep["rb_launches"] > 0, rep
        check_oracle(m, eng, tag, out, [0, 31, 32, 63], 0, f"{tag} B=64")
    finally:
        m = eng = None
        drop()


def test_graph_replay_at_batch_64_with_the_split(default_runs, monkeypatch):
    """hipGraph replay (Engine.graph_max_batch) where the capture contains the stage-3 split's two parallel branches: the eager report says s3_split_taken == 1, and
    three replays on changing inputs equal the eager forwards bit for bit."""
    m, eng = make("centered", {}, monkeypatch)
    try:
        xs = [batch(64), torch.roll(batch(64), 7, 0), torch.flip(batch(64), (0,))]
        eager = []
        for x in xs:
            out, rep = fwd(eng, x)
            assert rep["s3_split_taken"] == 1, rep
            eager.append(out)
        assert same(eager[0], default_runs[64][0])
        eng.graph_max_batch = 64
        replay = [eng.forward(x) for x in xs] + [eng.forward(xs[0])]   # the first call captures, the others replay
        torch.cuda.synchronize()
        eng.graph_max_batch = 0
        assert len(eng._graph_bufs) == 1
        for k, (a, b) in enumerate(zip(eager + [eager[0]], replay)):
            assert same(a, b), f"graph replay {k} differs from the eager forward"
        assert not torch.equal(replay[0][0], replay[1][0])
    finally:
        m = eng = None
        drop()
        print(f"[test_gpu_batch_dispatch.py] wall time of this file so far: {time.time() - _t0:.0f} s")
