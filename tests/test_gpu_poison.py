"""The forward against its buffers (-m gpu).  pf_forward_* takes a caller-owned workspace per call, and every other engine test runs its forwards
on the same images through ONE reused buffer: an intermediate that is read before this forward wrote it (a padded lane under a zero weight, a halo row of a fused stage)
finds the previous forward's correct values there.  Here the test owns every buffer and calls pf_forward_u8 / pf_forward_f32 through Engine.lib:

  * the workspace is exactly pf_workspace_bytes(B) bytes; workspace, pred_gravity, pred_latitude and params each lie between two 256 KiB patterned guard bands
    (ops.checked_outputs, the harness of the kernel-level tests); the outputs hold 0xFF bytes (NaN) before every forward;
  * three forwards of the same images, with every byte of the workspace first 0x00, then 0xFF (NaN everywhere), then 0x4B (fp32 0x4B4B4B4B = 1.3e7, large finite garbage);
  * the three must be bit-identical, no output element NaN, every guard intact after every forward, and a saturation counter of the test's own
    (pf_set_saturation_counter) must move by the same amount under every fill as in a forward through Engine.forward -- a stale read that reached a watched producer
    would move it further.

The network only runs at 320 x 320; B = 3 is odd (partial row blocks in stage 4, a half-full group)."""
import numpy as np
import pytest
import torch

from perspectivefields_amd.synth import synthetic_image

pytestmark = pytest.mark.gpu

CASES = {"centered": "Paramnet-360Cities-edina-centered", "uncentered": "Paramnet-360Cities-edina-uncentered", "persnet": "PersNet-360Cities"}
NET = 320
FILLS = (0x00, 0xFF, 0x4B)
SEED0 = 4100

_models = {}


@pytest.fixture(scope="module", autouse=True)
def _release():
    yield
    _models.clear()
    torch.cuda.empty_cache()


def engine(tag, precision):
    from perspectivefields_amd import PerspectiveFields

    if (tag, precision) not in _models:
        _models[(tag, precision)] = PerspectiveFields(CASES[tag], weights="synthetic:0", precision=precision).eval().cuda()
    return _models[(tag, precision)]._get_engine()


def images(B, as_f32):
    x = torch.from_numpy(np.stack([synthetic_image(NET, NET, seed=SEED0 + i) for i in range(B)])).cuda()
    return x.permute(0, 3, 1, 2).float().contiguous() if as_f32 else x


def run_case(tag, precision, B, as_f32=False, defer=False):
    from perspectivefields_amd import ops
    from perspectivefields_amd.engine import PARAMS_STRIDE, _check, _stream_ptr

    eng = engine(tag, precision)
    lib, h, dev = eng.lib, eng._h, eng.device
    x = images(B, as_f32)
    # warm through the engine's own path: tunes the batch size (the timed autotune forward) and, on a second forward, says what one forward adds to the saturation counter
    eng.forward(x)
    before = int(eng.saturation_snapshot())
    eng.forward(x)
    per_forward = int(eng.saturation_snapshot()) - before
    assert lib.pf_is_tuned(h, B)
    nws = int(lib.pf_workspace_bytes(h, B))
    assert nws > 0
    fn = lib.pf_forward_f32 if as_f32 else lib.pf_forward_u8
    counter = torch.zeros(1, dtype=torch.int32, device=dev)
    runs = []
    try:
        _check(lib.pf_set_saturation_counter(h, counter.data_ptr()), h, "pf_set_saturation_counter")
        if defer:
            eng.set_defer_params(True)
        with ops.checked_outputs() as chk, torch.cuda.device(dev):
            ws = ops._out((nws,), torch.uint8, dev, "workspace", poison=False)
            pg = ops._out((B, eng.gravity_channels, NET, NET), torch.float32, dev, "pred_gravity")
            pl = ops._out((B, eng.latitude_channels, NET, NET), torch.float32, dev, "pred_latitude")
            params = ops._out((B, PARAMS_STRIDE), torch.float32, dev, "params") if eng.param_outputs else None
            outs = [t for t in (pg, pl, params) if t is not None]
            assert ws.numel() == nws and ws.data_ptr() % 256 == 0
            for k, fill in enumerate(FILLS):
                ws.fill_(fill)
                for g in chk.buffers[1:]:
                    g.body().fill_(ops.POISON_BYTE)
                assert all(bool(torch.isnan(t).all()) for t in outs)
                _check(fn(h, B, x.data_ptr(), pg.data_ptr(), pl.data_ptr(), params.data_ptr() if params is not None else None, ws.data_ptr(), nws, _stream_ptr()), h, "pf_forward")
                if defer:
                    _check(lib.pf_join_params(h, _stream_ptr()), h, "pf_join_params")   # before params is read, before its guards are compared, before the refill
                rep = eng.last_dispatch()
                assert rep["batch"] == B and 0 < rep["real_peak_bytes"] <= rep["dry_peak_bytes"] <= nws, rep
                chk.verify(release=False)      # synchronises; the same buffers take the next forward
                what = f"{tag} {precision} B={B}{' f32 input' if as_f32 else ''}{' deferred ParamNet' if defer else ''}, workspace filled with 0x{fill:02X}"
                for name, t in zip(("pred_gravity", "pred_latitude", "params"), outs):
                    n = int(torch.isnan(t).sum())
                    assert n == 0, f"{what}: {n} NaN of {t.numel()} in {name}"
                assert int(counter) == (k + 1) * per_forward, f"{what}: the saturation counter stands at {int(counter)} after {k + 1} forward(s) that add {per_forward} each in a clean workspace"
                runs.append([t.clone() for t in outs])
            assert len(chk.buffers) == 1 + len(outs) and chk.outputs == 1 + len(outs)   # nothing was released early: the guards compared last are the ones allocated first
    finally:
        if defer:
            eng.set_defer_params(False)
        lib.pf_set_saturation_counter(h, eng._sat.data_ptr())
    for k in (1, 2):
        for name, a, b in zip(("pred_gravity", "pred_latitude", "params"), runs[0], runs[k]):
            diff = int((a.view(torch.int32) != b.view(torch.int32)).sum())
            assert diff == 0, (f"{tag} {precision} B={B}: {name} depends on what the workspace held before the call: {diff} of {a.numel()} elements differ between the "
                               f"0x00-filled and the 0x{FILLS[k]:02X}-filled workspace")


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("precision", ["fp32", "fp32_bf16x6"])
@pytest.mark.parametrize("tag", list(CASES))
def test_forward_does_not_depend_on_its_workspace(tag, precision, B):
    run_case(tag, precision, B)


def test_forward_f32_input_does_not_depend_on_its_workspace():
    run_case("centered", "fp32", 3, as_f32=True)


def test_deferred_paramnet_does_not_depend_on_its_workspace():
    run_case("centered", "fp32", 3, defer=True)
