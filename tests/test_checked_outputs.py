"""ops.checked_outputs(), the harness the kernel-level GPU tests run under, shown to bite.  Only torch is involved, so everything here runs on
CPU tensors through ops._out; one case repeats the guard check on a device tensor with a torch slice assignment (no kernel).  A "kernel" here is a torch write into the
output, or, for a store outside it, into the backing buffer that checked_outputs() exposes."""
import re
import threading

import pytest
import torch

from perspectivefields_amd import ops

G = ops.GUARD_BYTES
CPU = torch.device("cpu")


def _damage(exc):
    """(label, side, count, offset, nbytes) of every guard an AssertionError of verify() names"""
    return [(m[1], m[2], int(m[3]), int(m[4]), int(m[5]))
            for m in re.finditer(r"(?:: |; )([^;:]+): (front|back) guard damaged: (\d+) byte\(s\), the first at offset ([+-]\d+) from the first byte of the (\d+)-byte output", str(exc))]


def test_constants_are_what_the_design_says():
    assert G == 256 * 1024 and G % 512 == 0 and G == 4 * 256 * 64 * 4 == 4 * 128 * 128 * 4   # four full 64 KB fp32 output tiles
    pat = ops.guard_pattern(CPU)
    assert pat.dtype == torch.uint8 and pat.shape == (G,)
    assert pat[:4].tolist() == [7, 138, 13, 144] and int(pat[G - 1]) == ((G - 1) * 131 + 7) & 0xFF
    assert len(set(pat[:256].tolist())) == 256, "131 is odd: every byte value occurs, no constant store can match the pattern"
    assert bool((pat[1:] != pat[:-1]).all())


@pytest.mark.parametrize("dtype,view", [(torch.float32, None), (torch.float16, None), (torch.bfloat16, None), (torch.int16, torch.bfloat16), (torch.int16, torch.float16)])
def test_poison_is_nan_in_every_format(dtype, view):
    """an untouched output reads as NaN everywhere: fp32, and the int16 plane words viewed as bf16 and as fp16"""
    with ops.checked_outputs():
        y = ops._out((3, 5, 8), dtype, CPU, "t")
        f = y if view is None else y.view(view)
        assert bool(torch.isnan(f).all())


def test_written_output_verifies_clean_and_layout():
    with ops.checked_outputs() as chk:
        y = ops._out((7, 5, 33), torch.float32, CPU, "conv")
        z = ops._out(384, torch.int16, CPU, "Planes", fill=0)
        assert y.shape == (7, 5, 33) and y.dtype == torch.float32 and y.is_contiguous()
        assert z.shape == (384,) and z.dtype == torch.int16
        assert [g.label for g in chk.buffers] == ["conv", "Planes"] and chk.outputs == 2
        g = chk.buffers[0]
        assert g.nbytes == 7 * 5 * 33 * 4 and g.backing.numel() == g.nbytes + 2 * G and g.backing.dtype == torch.uint8
        assert y.data_ptr() == g.backing.data_ptr() + G and y.data_ptr() % 16 == 0
        assert torch.equal(g.backing[:G], ops.guard_pattern(CPU)) and torch.equal(g.backing[G + g.nbytes:], ops.guard_pattern(CPU))
        y.copy_(torch.arange(y.numel(), dtype=torch.float32).view(y.shape))
        z.fill_(-3)
        chk.verify(release=False)          # an intermediate look keeps the buffers
        assert len(chk.buffers) == 2 and chk.held_bytes == g.nbytes + 384 * 2 + 4 * G
        chk.verify()                       # explicit: clean, and the buffers are released
        assert chk.buffers == [] and chk.held_bytes == 0
        assert float(y[6, 4, 32]) == y.numel() - 1 and int(z[383]) == -3   # the views outlive the manager's reference
    assert getattr(ops._checked, "mgr", None) is None


@pytest.mark.parametrize("dtype,view", [(torch.float32, None), (torch.int16, torch.bfloat16), (torch.int16, torch.float16)])
@pytest.mark.parametrize("where", ["first", "middle", "last"])
def test_one_unwritten_element_is_nan(dtype, view, where):
    """the comparisons the kernel tests make (_close: worst <= 1.0; torch.equal against a complete result) both fail on one element the "kernel" skipped"""
    n = 3 * 7 * 33
    full = torch.arange(1, n + 1, dtype=torch.float32)
    full = full if view is None else full.to(view).view(torch.int16)
    idx = {"first": 0, "middle": n // 2, "last": n - 1}[where]
    with ops.checked_outputs():
        y = ops._out((3, 7, 33), dtype, CPU, "t")
        flat = y.view(-1)
        flat[:idx] = full[:idx]
        flat[idx + 1:] = full[idx + 1:]
        f = flat if view is None else flat.view(view)
        ref = full if view is None else full.view(view)
        nan = torch.isnan(f)
        assert int(nan.sum()) == 1 and bool(nan[idx])
        assert not torch.equal(f, ref)
        worst = float(((f.double() - ref.double()).abs() / (2e-5 * (1.0 + ref.double().abs()))).max())
        assert not (worst <= 1.0)


def test_fill_and_copy_outputs_are_guarded_but_not_poisoned():
    with ops.checked_outputs() as chk:
        pn = ops._out((6, 4), torch.float32, CPU, "pn", fill=-7.0, poison=False)
        assert bool((pn == -7.0).all())
        src = torch.arange(24, dtype=torch.float32).view(4, 6).t()     # not contiguous
        cp = ops._out_copy(src, "copy")
        assert torch.equal(cp, src) and cp.is_contiguous() and cp.data_ptr() == chk.buffers[1].backing.data_ptr() + G
        nanfill = ops._out((2, 8), torch.float32, CPU, "scalars", fill=float("nan"))
        assert bool(torch.isnan(nanfill).all())


@pytest.mark.parametrize("dtype", [torch.float32, torch.int16, torch.int32, torch.uint8])
@pytest.mark.parametrize("side", ["front", "back"])
def test_one_byte_into_a_guard_is_reported(dtype, side):
    shape = (5, 13)
    with pytest.raises(AssertionError) as e:
        with ops.checked_outputs() as chk:
            ops._out((4,), torch.float32, CPU, "before").fill_(0)
            y = ops._out(shape, dtype, CPU, "the op")
            ops._out((4,), torch.float32, CPU, "after").fill_(0)
            y.fill_(1)
            g = chk.buffers[1]
            at = G - 1 if side == "front" else G + g.nbytes      # the byte just before the output / just behind it
            g.backing[at] ^= 0x10
    nbytes = 5 * 13 * torch.empty(0, dtype=dtype).element_size()
    assert _damage(e.value) == [("the op", side, 1, -1 if side == "front" else nbytes, nbytes)], str(e.value)


def test_far_end_of_the_guards_and_counts():
    """the first and the last byte of the whole backing buffer are watched; count and first offset are those of the damage"""
    with ops.checked_outputs() as chk:
        y = ops._out((10,), torch.int32, CPU, "op a")
        y.zero_()
        g = chk.buffers[0]
        g.backing[0] ^= 1
        g.backing[100:103] ^= 1
        g.backing[G + 40 + G - 1] ^= 1
        with pytest.raises(AssertionError) as e:
            chk.verify()
        assert _damage(e.value) == [("op a", "front", 4, -G, 40), ("op a", "back", 1, 40 + G - 1, 40)], str(e.value)
        assert chk.buffers == []           # reported once, then released


@pytest.mark.parametrize("value", [0x00, ops.POISON_BYTE, 0x4B])
@pytest.mark.parametrize("side", ["front", "back"])
def test_constant_stores_into_a_guard_are_caught(value, side):
    """a kernel that stores zeros, the poison or any other single byte value over a run of guard bytes: the pattern is not a constant, so at most 1 byte in 256 survives"""
    for run in (2, 16, 64 * 1024):
        with ops.checked_outputs() as chk:
            y = ops._out((33, 7), torch.float32, CPU, "op")
            y.zero_()
            g = chk.buffers[0]
            lo = G - run if side == "front" else G + g.nbytes
            g.backing[lo:lo + run] = value
            with pytest.raises(AssertionError) as e:
                chk.verify()
            (label, s, count, off, nbytes), = _damage(e.value)
            assert (label, s) == ("op", side) and run - (run + 255) // 256 <= count <= run
            assert (-run <= off <= -run + 1) if side == "front" else (nbytes <= off <= nbytes + 1)


def test_off_is_a_plain_tensor():
    assert getattr(ops._checked, "mgr", None) is None
    for fill in (None, 0, 2.5):
        y = ops._out((3, 5), torch.float32, CPU, "t", fill=fill)
        assert y.shape == (3, 5) and y.dtype == torch.float32 and y.storage_offset() == 0 and y.untyped_storage().nbytes() == 3 * 5 * 4
        if fill is not None:
            assert bool((y == fill).all())
    z = ops._out(12, torch.int16, CPU, "Planes", fill=0)
    assert z.shape == (12,) and z.dtype == torch.int16 and z.untyped_storage().nbytes() == 24 and not bool(z.any())
    src = torch.arange(6.0).view(2, 3).t()
    cp = ops._out_copy(src, "t")
    assert torch.equal(cp, src) and cp.is_contiguous() and cp.untyped_storage().nbytes() == 24 and cp.data_ptr() != src.data_ptr()


def test_nesting_is_refused_and_the_outer_block_survives():
    with ops.checked_outputs() as chk:
        with pytest.raises(RuntimeError, match="does not nest"):
            with ops.checked_outputs():
                pass
        assert ops._checked.mgr is chk     # the refusal did not switch the outer block off
        ops._out((2,), torch.float32, CPU, "t").zero_()
    assert getattr(ops._checked, "mgr", None) is None
    with ops.checked_outputs():            # one after the other is fine
        pass


def test_off_again_after_an_exception_and_the_exception_is_kept():
    with pytest.raises(ZeroDivisionError):
        with ops.checked_outputs() as chk:
            ops._out((2,), torch.float32, CPU, "t")
            chk.buffers[0].backing[0] ^= 1     # damage too: the block's own exception is what the caller sees
            1 / 0
    assert getattr(ops._checked, "mgr", None) is None
    assert ops._out((2,), torch.float32, CPU, "t").untyped_storage().nbytes() == 8


def test_thread_local():
    seen = {}

    def other():
        seen["mgr"] = getattr(ops._checked, "mgr", None)
        seen["bytes"] = ops._out((4,), torch.float32, CPU, "t").untyped_storage().nbytes()

    with ops.checked_outputs():
        t = threading.Thread(target=other)
        t.start()
        t.join()
    assert seen == {"mgr": None, "bytes": 16}


def test_early_release_past_the_hold_limit(monkeypatch):
    """past HOLD_LIMIT_BYTES the manager verifies what it holds and lets it go (damage is reported at that allocation, not lost)"""
    monkeypatch.setattr(ops, "HOLD_LIMIT_BYTES", 3 * (2 * G + 64))
    with ops.checked_outputs() as chk:
        for i in range(3):
            ops._out((16,), torch.float32, CPU, f"op {i}").zero_()
        assert len(chk.buffers) == 3
        ops._out((16,), torch.float32, CPU, "op 3").zero_()
        assert [g.label for g in chk.buffers] == ["op 3"] and chk.outputs == 4 and chk.held_bytes == 2 * G + 64
        chk.buffers[0].backing[G + 64] = 0     # pattern byte 7 there
        ops._out((16,), torch.float32, CPU, "op 4").zero_()
        ops._out((16,), torch.float32, CPU, "op 5").zero_()
        with pytest.raises(AssertionError) as e:
            ops._out((16,), torch.float32, CPU, "op 6")
        assert _damage(e.value) == [("op 3", "back", 1, 64, 64)]


@pytest.mark.gpu
def test_guard_damage_on_a_device_tensor():
    """the same on the GPU: torch slice assignments into the backing buffer, no kernel of the library"""
    dev = torch.device("cuda", torch.cuda.current_device())
    with ops.checked_outputs() as chk:
        y = ops._out((3, 129, 33), torch.float32, dev, "device op")
        assert y.device == dev and y.data_ptr() % 512 == 0 and bool(torch.isnan(y).all())
        y.copy_(torch.ones(3, 129, 33))
        chk.verify()
    for side in ("front", "back"):
        with pytest.raises(AssertionError) as e:
            with ops.checked_outputs() as chk:
                y = ops._out((3, 129, 33), torch.float32, dev, "device op")
                y.zero_()
                g = chk.buffers[0]
                at = G - 4 if side == "front" else G + g.nbytes
                g.backing[at:at + 4] = 0       # one fp32 zero just outside: pattern bytes there are never 0 four times in a row
        (label, s, count, off, nbytes), = _damage(e.value)
        assert (label, s, nbytes) == ("device op", side, 3 * 129 * 33 * 4) and 3 <= count <= 4
        assert (-4 <= off <= -3) if side == "front" else (nbytes <= off <= nbytes + 1)
