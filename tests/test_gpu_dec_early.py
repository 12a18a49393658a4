"""The early decoder start (PF_DEC_EARLY, engine_forward.hip dec_early_issue()): at decoder levels 0-2 the folded first conv fold[k] reads only the MiT stage output c_{k+1}
and r1c1[k] only fold[k]'s output, so they are issued on a side stream right after the stage-3 norm, beside MiT stage 4 and decoder levels 3 / 2.  The same kernels
run with the same tiles on the same inputs: every comparison in this file is torch.equal, no tolerance.  The dispatch report (dec_early_taken) is the witness that
the path ran -- or, under each of its gates, did not.

Inputs: 320 x 320 uint8 images with a distinct seed per batch slot, synthetic weights, batches 3 (below the gate), 4 and 5 (odd)."""
import ctypes

import numpy as np
import pytest
import torch

from perspectivefields_amd.synth import synthetic_image

pytestmark = pytest.mark.gpu

CASES = {"centered": "Paramnet-360Cities-edina-centered", "persnet": "PersNet-360Cities"}
NET = 320
GUARD = 1 << 20
PATTERN = 0xA5

_engines = {}
_images = {}


def batch(B, first=0):
    for i in range(first, first + B):
        if i not in _images:
            _images[i] = synthetic_image(NET, NET, seed=5200 + i)
    return torch.from_numpy(np.stack([_images[first + i] for i in range(B)])).cuda()


def engine(tag, **env):
    """one engine per (architecture, switches), created after the switches are set (pf_create reads them) and kept for the module"""
    key = (tag, tuple(sorted(env.items())))
    if key not in _engines:
        from perspectivefields_amd import PerspectiveFields

        with pytest.MonkeyPatch.context() as mp:
            for k, v in env.items():
                mp.setenv(k, v)
            m = PerspectiveFields(CASES[tag], weights="synthetic:0").eval().cuda()
            _engines[key] = (m, m._get_engine())
    return _engines[key][1]


def fwd(eng, x):
    out = tuple(None if t is None else t.clone() for t in eng.forward(x))
    torch.cuda.synchronize()
    rep = eng.last_dispatch()
    assert rep["batch"] == x.shape[0] and rep["fork_alloc_conflicts"] == 0 and 0 < rep["real_peak_bytes"] <= rep["dry_peak_bytes"], rep
    return out, rep


def same(a, b):
    return all((u is None and v is None) or (u is not None and v is not None and torch.equal(u, v)) for u, v in zip(a, b))


_ref = {}


def reference(tag, B):
    """PF_DEC_EARLY=0 (the forward order) at batch B: computed once, shared"""
    if (tag, B) not in _ref:
        out, rep = fwd(engine(tag, PF_DEC_EARLY="0"), batch(B))
        assert rep["dec_early_taken"] == 0, rep
        _ref[(tag, B)] = out
    return _ref[(tag, B)]


@pytest.mark.parametrize("tag", ["centered", "persnet"])
@pytest.mark.parametrize("mode", ["1", "2"])
def test_early_decoder_start_is_bit_identical(tag, mode):
    """pred_gravity, pred_latitude and params of PF_DEC_EARLY = 1 / 2 against 0, B = 4 and B = 5, the centered ParamNet model (fused prediction heads) and PersNet
    (classification heads: 73 / 180 logits, no ParamNet); the report says the path ran; a second forward gives the same bits."""
    eng = engine(tag, PF_DEC_EARLY=mode)
    for B in (4, 5):
        want = reference(tag, B)
        got, rep = fwd(eng, batch(B))
        assert rep["dec_early_taken"] == 1 and rep["forks"] > 0, rep
        assert (got[2] is None) == (tag == "persnet")
        assert same(got, want), f"{tag} PF_DEC_EARLY={mode} B={B} differs from PF_DEC_EARLY=0"
        again, rep2 = fwd(eng, batch(B))
        assert rep2 == rep and same(again, want)


def test_default_is_a_value_of_the_switch():
    """the engine without the switch set behaves as one of its values: same outputs as PF_DEC_EARLY=0, the counter 0 or 1"""
    got, rep = fwd(engine("centered"), batch(4))
    assert rep["dec_early_taken"] in (0, 1), rep
    assert same(got, reference("centered", 4))


def test_gates():
    """dec_early_taken is 0 with the switch off, in the debug forward, inside a full per-launch profile window, below the batch gate and with PF_SIDE_STREAM=0;
    and 1 again in the plain forward that follows on the same engine.  Outputs equal the forward order's every time."""
    x4, x3 = batch(4), batch(3)
    want4 = reference("centered", 4)
    want3, rep = fwd(engine("centered", PF_DEC_EARLY="0"), x3)
    assert rep["dec_early_taken"] == 0, rep                                   # switch off
    eng = engine("centered", PF_DEC_EARLY="1")
    got, rep = fwd(eng, x3)
    assert rep["dec_early_taken"] == 0 and same(got, want3), rep              # batch below the gate (4)
    got, rep = fwd(eng, x4)
    assert rep["dec_early_taken"] == 1 and same(got, want4), rep
    dbg = eng.forward_debug(x4, shadow=True, ranges=True)                     # debug forward: taps and range records in forward order
    torch.cuda.synchronize()
    rep = eng.last_dispatch()
    assert rep["dec_early_taken"] == 0 and rep["fork_alloc_conflicts"] == 0 and rep["real_peak_bytes"] <= rep["dry_peak_bytes"], rep
    assert same(dbg[:3], want4)
    eng.profile_begin()                                                       # full per-launch profile: one stream
    try:
        got = tuple(t.clone() for t in eng.forward(x4))
        rep = eng.last_dispatch()
    finally:
        eng.profile_end()
    assert rep["dec_early_taken"] == 0 and rep["forks"] == 0 and rep["real_peak_bytes"] <= rep["dry_peak_bytes"], rep
    assert same(got, want4)
    eng.profile_begin(large_only=True)                                        # the large-launch profile keeps the side streams
    try:
        got = tuple(t.clone() for t in eng.forward(x4))
        rep = eng.last_dispatch()
    finally:
        eng.profile_end()
    assert rep["dec_early_taken"] == 1 and same(got, want4), rep
    got, rep = fwd(eng, x4)
    assert rep["dec_early_taken"] == 1 and same(got, want4), rep
    x9 = batch(9)                                                             # a JOINED forward above PF_DEC_EARLY_JOINED_MAX (8) keeps the forward order ...
    want9, rep = fwd(eng, x9)
    assert rep["dec_early_taken"] == 0, rep
    try:                                                                      # ... the same batch with the deferred ParamNet branch takes the early start
        eng.set_defer_params(True)
        got = eng.forward(x9)
        rep = eng.last_dispatch()
        eng.join_params()
        torch.cuda.synchronize()
    finally:
        eng.set_defer_params(False)
    assert rep["dec_early_taken"] == 1 and same(got, want9), rep
    got, rep = fwd(engine("centered", PF_DEC_EARLY="1", PF_SIDE_STREAM="0"), x4)
    assert rep["dec_early_taken"] == 0 and rep["forks"] == 0 and same(got, want4), rep


def test_stream_switch():
    """PF_DEC_EARLY_STREAM=1: the window runs on `side` and stage 4 gives its q-beside-kv fork up meanwhile (fewer fork windows than on `side2`); same bits."""
    want = reference("centered", 5)
    _, rep2 = fwd(engine("centered", PF_DEC_EARLY="2"), batch(5))
    got, rep = fwd(engine("centered", PF_DEC_EARLY="2", PF_DEC_EARLY_STREAM="1"), batch(5))
    assert rep["dec_early_taken"] == 1 and 0 < rep["forks"] < rep2["forks"], (rep, rep2)
    assert same(got, want)


def test_batch_gate_switch():
    """PF_DEC_EARLY_MIN_BATCH=6: batch 5 keeps the forward order, batch 6 takes the early start"""
    eng = engine("centered", PF_DEC_EARLY="1", PF_DEC_EARLY_MIN_BATCH="6")
    got, rep = fwd(eng, batch(5))
    assert rep["dec_early_taken"] == 0 and same(got, reference("centered", 5)), rep
    _, rep = fwd(eng, batch(6))
    assert rep["dec_early_taken"] == 1, rep


@pytest.mark.parametrize("mode", ["1", "2"])
def test_deferred_paramnet_branch_beside_the_early_start(mode):
    """Three forwards in a row with the deferred ParamNet branch (the branch of forward i runs beside forward i + 1, whose early decoder launches are issued BEFORE
    the join of that branch): the params of every step equal the joined forward's, the fields those of PF_DEC_EARLY=0, bit for bit."""
    eng = engine("centered", PF_DEC_EARLY=mode)
    off = engine("centered", PF_DEC_EARLY="0")
    xs = [batch(4, first=4 * i) for i in range(3)]
    want = [fwd(off, x)[0] for x in xs]
    joined = [fwd(eng, x)[0] for x in xs]
    for a, b in zip(joined, want):
        assert same(a, b)
    try:
        eng.set_defer_params(True)
        outs = []
        for x in xs:
            outs.append(eng.forward(x))
            assert eng.last_dispatch()["dec_early_taken"] == 1
        eng.join_params()
        torch.cuda.synchronize()
    finally:
        eng.set_defer_params(False)
    for k, (a, b) in enumerate(zip(outs, want)):
        assert same(a, b), f"step {k} of the deferred run differs"


@pytest.mark.parametrize("mode", ["1", "2"])
def test_workspace(mode):
    """pf_workspace_bytes with the path on is at least the figure with it off; a forward in exactly that many bytes between two guard bands succeeds and leaves the
    bands alone; forwards of different batch sizes back to back give what fresh engines give (the hoisted tensors follow the batch's own layout)."""
    eng = engine("centered", PF_DEC_EARLY=mode)
    off = engine("centered", PF_DEC_EARLY="0")
    for B in (3, 4, 5):
        assert eng.workspace_bytes(B) >= off.workspace_bytes(B) > 0, B
    assert eng.workspace_bytes(3) == off.workspace_bytes(3)                   # below the gate nothing is hoisted
    for B in (5, 4):
        x = batch(B)
        need = eng.workspace_bytes(B)
        buf = torch.full((need + 2 * GUARD,), PATTERN, dtype=torch.uint8, device="cuda")
        pg = torch.empty((B, eng.gravity_channels, NET, NET), dtype=torch.float32, device="cuda")
        pl = torch.empty((B, eng.latitude_channels, NET, NET), dtype=torch.float32, device="cuda")
        pr = torch.empty((B, 8), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        rc = eng.lib.pf_forward_u8(eng._h, B, x.data_ptr(), pg.data_ptr(), pl.data_ptr(), pr.data_ptr(), buf.data_ptr() + GUARD, need,
                                   ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        rep = eng.last_dispatch()
        assert rc == 0, eng.lib.pf_last_error(eng._h)
        assert rep["dec_early_taken"] == 1 and rep["fork_alloc_conflicts"] == 0 and 0 < rep["real_peak_bytes"] <= rep["dry_peak_bytes"] <= need, rep
        assert bool((buf[:GUARD] == PATTERN).all()) and bool((buf[GUARD + need:] == PATTERN).all()), f"B={B}: a guard band around the workspace was written"
        assert same((pg, pl, pr), reference("centered", B))
        rc = eng.lib.pf_forward_u8(eng._h, B, x.data_ptr(), pg.data_ptr(), pl.data_ptr(), pr.data_ptr(), buf.data_ptr() + GUARD, need - 1,
                                   ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == -4, rc                                                   # one byte short: refused before any launch
        del buf
    for B in (5, 4, 5, 3, 4):
        got, _ = fwd(eng, batch(B))
        want = reference("centered", B) if B > 3 else fwd(off, batch(3))[0]
        assert same(got, want), f"B={B} after another batch size"


def test_graph_capture_takes_the_early_start():
    """Under graph capture the fork and the join are event edges between the capture stream and a side stream, like the q fork's: the capturing call reports
    dec_early_taken == 1, and the capture and two replays on changing inputs equal the eager forwards."""
    eng = engine("centered", PF_DEC_EARLY="1")
    xs = [batch(4), torch.roll(batch(4), 1, 0), batch(4, first=4)]
    eager = [fwd(eng, x)[0] for x in xs]
    assert same(eager[0], reference("centered", 4))
    eng.graph_max_batch = 4
    try:
        replay = []
        for x in xs:
            replay.append(tuple(t.clone() for t in eng.forward(x)))           # the first call captures, the others replay
            assert eng.last_dispatch()["dec_early_taken"] == 1
        torch.cuda.synchronize()
    finally:
        eng.graph_max_batch = 0
    for k, (a, b) in enumerate(zip(eager, replay)):
        assert same(a, b), f"graph call {k} differs from the eager forward"
    got, rep = fwd(eng, xs[0])
    assert rep["dec_early_taken"] == 1 and same(got, eager[0])
