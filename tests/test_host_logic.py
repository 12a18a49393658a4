"""CPU-only tests of the host side: config / zoo, checkpoint schema and strict validation, synthetic
checkpoint determinism, C-ABI library loading + symbol export, weight-fold algebra, shard logic."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from perspectivefields_amd import config as cfgmod
from perspectivefields_amd.config import arch_of, get_cfg, model_zoo
from perspectivefields_amd.schema import checkpoint_schema, validate_state_dict
from perspectivefields_amd.synth import synthetic_image, synthetic_state_dict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_zoo_and_cfg():
    assert list(model_zoo) == [
        "Paramnet-360Cities-edina-centered", "Paramnet-360Cities-edina-uncentered", "PersNet-360Cities",
        "PersNet_Paramnet-GSV-uncentered", "PersNet_Paramnet-GSV-centered",
    ]
    c = get_cfg("Paramnet-360Cities-edina-centered")
    assert c.MODEL.GRAVITY_DECODER.LOSS_TYPE == "regression" and c.MODEL.RECOVER_RPF and not c.MODEL.RECOVER_PP
    assert c.DATALOADER.RESIZE == [320, 320] and c.INPUT.FORMAT == "BGR" and c.MODEL.PIXEL_MEAN == [103.53, 116.28, 123.675]
    with pytest.raises(AttributeError):
        c.MODEL.RECOVER_PP = True  # frozen like the reference's cfg
    with pytest.raises(KeyError):
        get_cfg("nope")
    a = arch_of(get_cfg("PersNet-360Cities"))
    assert (a["gravity_out"], a["latitude_out"], a["param_net"]) == (73, 180, None)
    a = arch_of(get_cfg("PersNet_Paramnet-GSV-uncentered"))
    assert a["param_net"] == "ParamNetConvNextRegress" and a["param_input_size"] == 64 and a["param_out"] == 5
    a = arch_of(get_cfg("PersNet_Paramnet-GSV-centered"))
    assert a["param_net"] == "ParamNet" and (a["gravity_out"], a["latitude_out"]) == (2, 1)


def test_schema_sizes():
    # 860 keys / 104,570,633 elements; 678 / 76,754,910
    s = checkpoint_schema("Paramnet-360Cities-edina-centered")
    assert len(s) == 860 and sum(int(np.prod(v)) if len(v) else 1 for v in s.values()) == 104570633
    s = checkpoint_schema("PersNet-360Cities")
    assert len(s) == 678 and sum(int(np.prod(v)) if len(v) else 1 for v in s.values()) == 76754910


def test_strict_validation():
    v = "Paramnet-360Cities-edina-centered"
    sd = synthetic_state_dict(v, 0)
    validate_state_dict(v, sd)
    bad = dict(sd); bad.pop("backbone.norm3.weight")
    with pytest.raises(ValueError, match="missing"):
        validate_state_dict(v, bad)
    bad = dict(sd); bad["extra.key"] = np.zeros(3, np.float32)
    with pytest.raises(ValueError, match="unexpected"):
        validate_state_dict(v, bad)
    bad = dict(sd); bad["ll_enc.conv1.weight"] = np.zeros((64, 3, 3, 3), np.float32)
    with pytest.raises(ValueError, match="shape"):
        validate_state_dict(v, bad)
    with pytest.raises(ValueError):
        validate_state_dict("PersNet-360Cities", sd)  # wrong architecture


def test_synth_deterministic():
    a = synthetic_state_dict("PersNet-360Cities", 0)
    b = synthetic_state_dict("PersNet-360Cities", 0)
    c = synthetic_state_dict("PersNet-360Cities", 1)
    k = "backbone.block3.7.mlp.fc1.weight"
    assert np.array_equal(a[k], b[k]) and not np.array_equal(a[k], c[k])
    assert a[k].dtype == np.float32
    # pinned values (platform-independent PCG64 streams): golden fixtures depend on them
    assert abs(float(a["backbone.norm1.weight"][0]) - float(b["backbone.norm1.weight"][0])) == 0
    im = synthetic_image(40, 30, 5)
    assert im.shape == (40, 30, 3) and im.dtype == np.uint8 and np.array_equal(im, synthetic_image(40, 30, 5))


def test_library_exports_every_declared_symbol():
    """The C-ABI library loads without a GPU and exports every symbol include/pf_hip.h declares."""
    from perspectivefields_amd.engine import LIB_PATH, declared_symbols, load_library

    hdr = open(os.path.join(ROOT, "include", "pf_hip.h")).read()
    declared = set(re.findall(r"\b(pf_[a-z0-9_]+)\s*\(", hdr))
    declared -= {"pf_engine"}
    assert declared, "no declarations parsed"
    checked = load_library()  # first: rebuilds a stale library (a raw dlopen before that would pin the old mapping in this process)
    assert os.path.exists(LIB_PATH), "libpf_hip.so not built (python -m perspectivefields_amd.build)"
    lib = ctypes.CDLL(LIB_PATH)
    missing = [s for s in sorted(declared) if not hasattr(lib, s)]
    assert not missing, f"library lacks {missing}"
    assert declared == set(declared_symbols()), (declared ^ set(declared_symbols()))
    assert checked.pf_version().startswith(b"pf_hip")


def test_no_gpu_means_loud_failure():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from perspectivefields_amd.engine import Engine, PfError, load_library

    with pytest.raises(PfError):
        Engine(0, "cuda:0")
    lib = load_library()
    h = ctypes.c_void_p()
    assert lib.pf_create(ctypes.byref(h), 0, 0) == -2  # PF_ERR_DEVICE, no CPU fallback
    assert b"no HIP device" in lib.pf_last_error(None)


def test_product_never_imports_oracle():
    pkg = os.path.join(ROOT, "perspectivefields_amd")
    for root, _, files in os.walk(pkg):
        for f in files:
            if f.endswith(".py"):
                src = open(os.path.join(root, f)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle|import_module\(.oracle", src, flags=re.M), f"{f} imports the oracle"


def test_fold_linear_into_conv_algebra():
    """The engine folds Linear(C->768) + zero-padded conv3x3(768->256) into one conv3x3(C->256) with a 9-case
    bias table (csrc/engine_weights.hip make_folded).  Same algebra in numpy, checked against the two-step form."""
    g = torch.Generator().manual_seed(0)
    C, E, O, H, W = 8, 24, 6, 5, 7
    x = torch.randn(2, C, H, W, generator=g, dtype=torch.float64)
    wl, bl = torch.randn(E, C, generator=g, dtype=torch.float64), torch.randn(E, generator=g, dtype=torch.float64)
    wp, bp = torch.randn(O, E, 3, 3, generator=g, dtype=torch.float64), torch.randn(O, generator=g, dtype=torch.float64)
    e = F.linear(x.permute(0, 2, 3, 1), wl, bl).permute(0, 3, 1, 2)
    ref = F.conv2d(e, wp, bp, padding=1)
    wf = torch.einsum("oekl,ec->ockl", wp, wl)
    T = torch.einsum("oekl,e->okl", wp, bl)
    out = F.conv2d(x, wf, None, padding=1)
    for y in range(H):
        for xx in range(W):
            cy = 0 if y == 0 else (2 if y == H - 1 else 1)
            cx = 0 if xx == 0 else (2 if xx == W - 1 else 1)
            b = bp.clone()
            for ky in range(3):
                for kx in range(3):
                    vy = not ((cy == 0 and ky == 0) or (cy == 2 and ky == 2))
                    vx = not ((cx == 0 and kx == 0) or (cx == 2 and kx == 2))
                    if vy and vx:
                        b = b + T[:, ky, kx]
            out[:, :, y, xx] += b
    assert torch.allclose(out, ref, atol=1e-10)


def test_general_vfov_closed_form_matches_fsolve():
    from oracle import pf_oracle
    from perspectivefields_amd.perspectivefields import general_vfov_to_focal

    rng = np.random.default_rng(0)
    cx, cy = rng.uniform(-0.3, 0.3, 50), rng.uniform(-0.3, 0.3, 50)
    fov = rng.uniform(15, 110, 50)
    np.testing.assert_allclose(general_vfov_to_focal(cx, cy, fov), pf_oracle.general_vfov_to_focal(cx, cy, fov), rtol=1e-7, atol=1e-9)


def test_shard_helpers():
    from perspectivefields_amd.dist import shard_range, shard_round_robin_by_bucket

    for n, w in [(256, 8), (10, 4), (3, 8), (33, 2)]:
        got = [shard_range(n, r, w) for r in range(w)]
        assert got[0][0] == 0 and got[-1][1] == n
        assert all(got[i][1] == got[i + 1][0] for i in range(w - 1))
        sizes = [hi - lo for lo, hi in got]
        assert max(sizes) - min(sizes) <= 1
    sizes = [(384, 512), (640, 640), (640, 640), (1024, 1365)] * 16
    parts = [shard_round_robin_by_bucket(sizes, r, 8) for r in range(8)]
    assert sorted(sum(parts, [])) == list(range(64))
    for p in parts:
        assert len(p) == 8 and sum(1 for i in p if sizes[i] == (640, 640)) == 4


def test_split_bf16_scheme_is_fp32_accurate():
    """The split-bf16 MFMA kernel (csrc/igemm_sb.hip) splits every fp32 value exactly into three bf16 parts by
    truncation and keeps six of the nine partial products.  Emulated here in numpy: the split is exact and the
    six-term dot product is as close to the fp64 result as a plain fp32 dot product."""
    rng = np.random.default_rng(0)

    def split(a):
        a = a.astype(np.float32)
        h = (a.view(np.uint32) & 0xFFFF0000).view(np.float32)
        r = a - h
        m = (r.view(np.uint32) & 0xFFFF0000).view(np.float32)
        l = r - m
        assert np.array_equal((l.view(np.uint32) & 0xFFFF0000).view(np.float32), l), "third part must fit 8 significant bits"
        return h, m, l

    a = (rng.standard_normal((64, 2304)) * np.exp(rng.uniform(-6, 6, (64, 2304)))).astype(np.float32)
    b = rng.standard_normal((2304, 32)).astype(np.float32) / 48
    ah, am, al = split(a)
    bh, bm, bl = split(b)
    assert np.array_equal(ah.astype(np.float64) + am + al, a.astype(np.float64))  # exact
    ref = a.astype(np.float64) @ b.astype(np.float64)
    six = sum((x.astype(np.float64) @ y.astype(np.float64)) for x, y in [(al, bh), (ah, bl), (am, bm), (am, bh), (ah, bm), (ah, bh)])
    scale = np.abs(a).astype(np.float64) @ np.abs(b).astype(np.float64)
    assert np.max(np.abs(six - ref) / scale) < 4 * 2.0 ** -24  # dropped terms: m*l, l*m, l*l
    f32 = (a @ b).astype(np.float64)
    assert np.max(np.abs(six - ref)) <= 2 * np.max(np.abs(f32 - ref)) + 1e-12


def test_split_f16_scheme_is_fp32_class():
    """The default parity scheme of the split kernels (csrc/sb_split.h, NT_F16X3): a ~ ah + al with ah = fp16_rn(a), al = fp16_rn(a - ah) UNSCALED (the matrix
    cores keep fp16 subnormals), weights scaled per output channel by a power of two and split as wh + wl, three partial products ah wh + ah wl + al wh in ONE fp32
    accumulator.  Emulated in numpy (fp16 rounding by numpy, which keeps subnormals; products and sums exact in float64): the per-product error is
    <= 3 * 2^-22 relative for |a| >= 2^-3 plus 2^-25 ABSOLUTE per element below (al is an fp16 subnormal there), and the dot-product error of O(1) data stays at the
    level of a plain fp32 dot product -- also with per-channel weight magnitudes over 2^+-20."""
    rng = np.random.default_rng(1)

    def split_a(a):
        a = np.clip(a.astype(np.float32), -65504, 65504)
        hi = a.astype(np.float16)
        lo = (a - hi.astype(np.float32)).astype(np.float16)
        return hi.astype(np.float64), lo.astype(np.float64)

    def split_w(w):  # rows = output channels
        mx = np.abs(w).max(axis=1, keepdims=True)
        e = np.where(mx > 0, 14 - np.frexp(mx)[1], 0)
        S = np.ldexp(np.float32(1), e).astype(np.float32)
        ws = (w * S).astype(np.float32)
        assert np.array_equal(ws.astype(np.float64), w.astype(np.float64) * S.astype(np.float64)), "power-of-two scale must be exact"
        hi = ws.astype(np.float16)
        lo = (ws - hi.astype(np.float32)).astype(np.float16)
        return hi.astype(np.float64), lo.astype(np.float64), 1.0 / S.astype(np.float64)

    for a_scale, w_spread in ((1.0, 0), (1.0, 20), (1e-3, 0), (1e-6, 0), (300.0, 8)):
        a = (rng.standard_normal((48, 2304)) * a_scale).astype(np.float32)
        w = (rng.standard_normal((40, 2304)) / 48).astype(np.float32) * np.exp2(rng.integers(-w_spread, w_spread + 1, (40, 1))).astype(np.float32)
        ah, al = split_a(a)
        wh, wl, inv = split_w(w)
        got = ((ah @ wh.T) + (ah @ wl.T) + (al @ wh.T)) * inv.T
        ref = a.astype(np.float64) @ w.astype(np.float64).T
        scale = np.abs(a).astype(np.float64) @ np.abs(w).astype(np.float64).T
        bound = 3 * 2.0 ** -22 * scale + 2.0 ** -25 * np.abs(w).astype(np.float64).sum(axis=1)[None, :]
        assert np.all(np.abs(got - ref) <= bound), (a_scale, w_spread)
        if a_scale >= 1.0:  # O(1) data: the level of a plain fp32 dot product
            f32 = (a @ w.T).astype(np.float64)
            assert np.max(np.abs(got - ref) / scale) <= 4 * np.max(np.abs(f32 - ref) / scale) + 2.0 ** -24, (a_scale, w_spread)
            assert np.max(np.abs(got - ref) / scale) <= 3 * 2.0 ** -22
    # representation: 22+ significant bits per operand from 2^-3 up, 2^-25 absolute below, saturation at the fp16 range
    x = (rng.standard_normal(100000) * np.exp(rng.uniform(-8, 8, 100000))).astype(np.float32)
    x = x[np.abs(x) <= 65504]
    hi, lo = split_a(x)
    big = np.abs(x) >= 0.125
    assert np.max(np.abs(hi + lo - x)[big] / np.abs(x[big])) <= 2.0 ** -22
    assert np.max(np.abs(hi + lo - x)[~big]) <= 2.0 ** -25
    hi, lo = split_a(np.array([1e9, -1e9], dtype=np.float32))
    assert np.array_equal(hi + lo, [65504.0, -65504.0])


def test_load_state_dict_strictness():
    """Missing keys / wrong shapes are always fatal; entries the architecture does not have are fatal when strict and
    dropped with a warning otherwise (the reference loads its zoo files with strict=False, perspectivefields.py:185,192)."""
    import warnings

    from perspectivefields_amd import PerspectiveFields
    from perspectivefields_amd.synth import synthetic_state_dict

    v = "PersNet-360Cities"
    sd = synthetic_state_dict(v, 0)
    extra = dict(sd)
    extra["trainer.iteration"] = np.zeros((1,), np.float32)
    extra["param_net.backbone.head.bias"] = np.zeros((5,), np.float32)
    with pytest.raises(ValueError):
        PerspectiveFields(v, weights=extra)  # in-memory state_dicts are held to the exact schema
    m = PerspectiveFields(v, weights="synthetic:0")
    with pytest.raises(ValueError):
        m.load_state_dict(extra)  # strict=True default
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        m.load_state_dict(extra, strict=False)
    assert any("ignoring 2 checkpoint entries" in str(r.message) for r in rec)
    assert "trainer.iteration" not in m.state_dict() and len(m.state_dict()) == len(sd)
    short = dict(sd)
    short.pop(next(iter(sd)))
    with pytest.raises(ValueError):
        m.load_state_dict(short, strict=False)  # a missing tensor is never tolerated


def test_pil_resize_algorithm_restatement():
    """The integer two-pass filter that csrc (resize_coeffs + resize_h/v_kernel) implements, restated in numpy and
    checked bit-for-bit against PIL (the reference's host resize, perspectivefields.py:34-46)."""
    import math

    from PIL import Image

    PREC = 22

    def coeffs(n_in, n_out):
        scale = n_in / n_out
        fs = max(scale, 1.0)
        support = fs
        ks = int(math.ceil(support)) * 2 + 1
        b, kk = [], np.zeros((n_out, ks), np.int64)
        for xx in range(n_out):
            c = (xx + 0.5) * scale
            x0 = max(int(c - support + 0.5), 0)
            x1 = min(int(c + support + 0.5), n_in) - x0
            k = np.array([max(0.0, 1.0 - abs((x + x0 - c + 0.5) / fs)) for x in range(x1)])
            k = k / k.sum() if k.sum() != 0 else k
            kk[xx, :x1] = [int(0.5 + v * (1 << PREC)) for v in k]
            b.append((x0, x1))
        return b, kk

    def one_pass(a, n_out):  # resample axis 1
        b, kk = coeffs(a.shape[1], n_out)
        out = np.zeros((a.shape[0], n_out, a.shape[2]), np.uint8)
        for xx, (x0, n) in enumerate(b):
            acc = (a[:, x0:x0 + n, :].astype(np.int64) * kk[xx, :n][None, :, None]).sum(1) + (1 << (PREC - 1))
            out[:, xx, :] = np.clip(acc >> PREC, 0, 255)
        return out

    rng = np.random.default_rng(1)
    for h, w in [(97, 211), (640, 640), (50, 30)]:
        img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        got = one_pass(one_pass(img, 320).transpose(1, 0, 2), 320).transpose(1, 0, 2)
        assert np.array_equal(got, np.asarray(Image.fromarray(img).resize((320, 320), Image.BILINEAR)))


def test_branch_free_gelu_is_fp32_accurate():
    """The kernels' erf-GELU (csrc/igemm_common.h gelu_erf, csrc/elem.hip gelu_fast): erf by Abramowitz-Stegun 7.1.26 on
    rcp / exp2, emulated here in float32.  It must be as close to the exact GELU as the float32 libm-erf form the reference
    effectively runs (torch GELU in fp32)."""
    import numpy as np
    from scipy.special import erf

    f = np.float32
    v = np.linspace(-12, 12, 400001).astype(f)
    x = np.abs(v) * f(0.70710678118654752440)
    t = (f(1.0) / (f(0.3275911) * x + f(1.0))).astype(f)
    p = (f(1.061405429) * t + f(-1.453152027)).astype(f)
    for c in (1.421413741, -0.284496736, 0.254829592):
        p = (p * t + f(c)).astype(f)
    p = (p * t).astype(f)
    e = np.exp2((x * x * f(-1.4426950408889634)).astype(f)).astype(f)
    er = np.copysign((f(1.0) - p * e).astype(f), v)
    fast = (f(0.5) * v * (f(1.0) + er)).astype(f)
    exact = 0.5 * v.astype(np.float64) * (1.0 + erf(v.astype(np.float64) / np.sqrt(2.0)))
    libm32 = (f(0.5) * v * (f(1.0) + erf(v * f(0.70710678118654752440)).astype(f))).astype(f)
    err_fast, err_libm = np.abs(fast - exact).max(), np.abs(libm32 - exact).max()
    assert err_fast <= 6e-7, err_fast
    assert err_fast <= 1.5 * err_libm + 1e-7, (err_fast, err_libm)


def test_bench_cli_contract_and_loud_failure_without_gpu():
    """bench.py keeps the driver's flags (--gpus/--steps/--warmup) and, on a box without a GPU, exits non-zero instead of
    printing a number from some fallback."""
    import subprocess
    import sys

    import torch

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    h = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--help"], capture_output=True, text=True, timeout=120)
    assert h.returncode == 0
    for flag in ("--gpus", "--steps", "--warmup", "--precision", "--events-in-timed", "--workload", "--full", "--dump-outputs"):
        assert flag in h.stdout, flag
    if not torch.cuda.is_available():
        r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--steps", "1", "--warmup", "0"], capture_output=True, text=True, timeout=300)
        assert r.returncode != 0
        assert '"metric"' not in r.stdout


def test_halo_kernel_lane_mapping_is_bank_conflict_free():
    """igemm_sbh.hip: ds_read_b128 is serviced in the lane groups {0-3, 12-15, 20-27} / {4-11, 16-19, 28-31} (and the same
    +32); a group conflicts when two of its lanes hit the same 16-byte slot of the 256-byte bank row.  With the odd patch
    rows rotated by -2 columns every group of every tap offset is conflict free; without the rotation it is not."""
    groups = [[0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27], [4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31]]
    hx = 18

    def slot(row, piece):  # row * 64 B + swizzled piece * 16 B, in 16-byte slots mod 16
        return (row & 3) * 4 + (piece ^ ((row >> 2) & 3))

    def extra_cycles(shift):
        bad = 0
        for r0 in range(0, 16, 2):
            for ky in range(3):
                for kx in range(3):
                    for piece in range(4):
                        for g in groups:
                            slots = []
                            for lane in g:
                                col = lane & 15
                                if lane >= 16:
                                    col = (col + shift) % 16
                                slots.append(slot((r0 + (lane >> 4) + ky) * hx + col + kx, piece))
                            bad += len(slots) - len(set(slots))
        return bad

    assert extra_cycles(14) == 0
    assert extra_cycles(0) > 0


def test_config_yaml_files_in_the_reference_format(tmp_path):
    """The config as YAML, the way the reference keeps it (perspective2d/config/*.yaml are yacs dumps; its constructor does defaults + merge_from_file,
    perspectivefields.py:129-132): write_zoo_yamls() files read back to the zoo configs, dump() -> merge_from_file() round-trips, a key the config does not model raises like
    yacs, training-only sections are skipped by name -- and, where the reference tree is present, ITS five files load to exactly the zoo configs."""
    files = cfgmod.write_zoo_yamls(str(tmp_path / "zoo"))
    assert sorted(files) == sorted({e["config_file"] for e in model_zoo.values()})
    for v, entry in model_zoo.items():
        written = cfgmod.get_cfg_from_file(files[entry["config_file"]])
        assert written == get_cfg(v) and written.is_frozen(), v
        p = tmp_path / f"{v}.yaml"
        p.write_text(get_cfg(v).dump())
        assert cfgmod.get_cfg_from_file(str(p)) == get_cfg(v)
        assert arch_of(written) == arch_of(get_cfg(v))
    # dump() has the reference files' layout: nested mappings, block lists, keys sorted
    text = get_cfg("PersNet-360Cities").dump()
    assert text.startswith("DATALOADER:\n  RESIZE:\n  - 320\n  - 320\n") and "LOSS_TYPE: classification" in text and "NUM_CLASSES: 180" in text
    bad = tmp_path / "bad.yaml"
    bad.write_text("MODEL:\n  NO_SUCH_KEY: 1\n")
    with pytest.raises(KeyError):
        cfgmod.get_cfg_from_file(str(bad))
    extra = tmp_path / "extra.yaml"
    extra.write_text("DATASETS:\n  TRAIN:\n  - x\nSOLVER:\n  BASE_LR: 0.1\nMODEL:\n  RECOVER_RPF: true\n")
    cfg = cfgmod.get_cfg_defaults()
    assert cfg.merge_from_file(str(extra)) == ["DATASETS", "SOLVER"] and cfg.MODEL.RECOVER_RPF is True
    with pytest.raises(AttributeError):
        get_cfg("PersNet-360Cities").merge_from_file(str(extra))   # frozen
    ref_dir = "/root/reference/perspective2d/config"
    if os.path.isdir(ref_dir):   # this container only; the GPU box has no reference tree
        for v, entry in model_zoo.items():
            cfg = cfgmod.get_cfg_defaults()
            skipped = cfg.merge_from_file(os.path.join(ref_dir, entry["config_file"]))
            assert skipped == ["DATASETS"], (v, skipped)
            assert cfg.freeze() == get_cfg(v), v


def test_no_packed_fp32_src1_high_half_forms_in_the_default_path():
    """ISA scan of the built library (no GPU): packed-fp32 instructions whose low lane reads the HIGH half of src1 -- ANY of them, the compiler's
    `v_pk_add_f32 d, x, x op_sel:[0,1]` reductions included.  Round 4 found such forms exact alone and wrong beside this library's kernels on another stream
    (profiles/r04_dw7_packed.md; scripts/microbench/pk_opsel_beside.hip) -- and every forward with the deferred ParamNet branch or the side stream is exactly that
    situation.  hipcc emits them on its own when it packs scalar code; the kernels it did that to are compiled with PF_NO_PK_F32 (pf_kernels.h), the hand-written
    packed depthwise kernels broadcast through src0 only.  Empty allow-list: the whole library must contain none."""
    import importlib.util

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-objdump"):
        pytest.skip("llvm-objdump not available")
    from perspectivefields_amd import build as _b

    lib = _b.build(verbose=False)
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(root, "scripts", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    hits = kr.packed_src1_high_forms(lib)
    assert not hits, hits[:8]


def test_no_valu_write_within_two_states_of_an_mfma_read():
    """ISA scan of the built library (no GPU): no MFMA reads, as A or B, a VGPR that a VALU instruction wrote fewer than two wait states earlier.  hipcc pads that
    hazard for the instructions it emits; the v_fma_mix pair of the split (inline asm, sb_split.h) it cannot see, and the kernels that feed the split straight into
    an MFMA from registers (attention, fused block, 7 x 7 stem, thin linear) pass the low part through split_f16_mfma_pad.  Found in r06 by the op test of
    thin128_kernel<false>: one s_waitcnt between the asm and the MFMA, 32 output columns wrong (profiles/r06_asm_mfma_hazard.md)."""
    import importlib.util

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-objdump"):
        pytest.skip("llvm-objdump not available")
    from perspectivefields_amd import build as _b

    lib = _b.build(verbose=False)
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(root, "scripts", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    hits = kr.valu_write_then_mfma_read(lib)
    assert not hits, hits[:8]


def test_hazard_scan_flags_the_listing_that_failed():
    """The scanner itself: the listing of thin128_kernel<false> that returned 32 wrong columns (one s_waitcnt between the asm's v_fma_mixhi_f16 and the MFMA) is flagged,
    the same listing with the pad is not, and neither is a write to a register the MFMA does not read."""
    import importlib.util

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(root, "scripts", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    head = ["0000000000001000 <_ZN2pf14thin128_kernelILb0EEEvNS_11ThinLinArgsE>:",
            "\tv_cvt_pk_f16_f32 v121, v3, v5 // 000000001000: D2680079",
            "\tv_fma_mixlo_f16 v3, v3, 1.0, -v121 op_sel_hi:[0,0,1] // 000000001008:",
            "\tv_fma_mixhi_f16 v3, v5, 1.0, -v121 op_sel:[0,0,1] op_sel_hi:[0,0,1] // 000000001010:"]
    mfma = "\tv_mfma_f32_32x32x16_f16 v[48:63], v[110:113], v[0:3], 0 // 000000001020:"
    bad = kr.scan_valu_write_then_mfma_read(head + ["\ts_waitcnt lgkmcnt(7) // 000000001018:", mfma])
    assert len(bad) == 1 and bad[0][0].startswith("_ZN2pf14thin128") and bad[0][1].startswith("v_fma_mixhi_f16 v3") and bad[0][3] == 1, bad
    assert kr.scan_valu_write_then_mfma_read(head + [mfma])[0][3] == 0
    assert not kr.scan_valu_write_then_mfma_read(head + ["\ts_nop 1", mfma])
    assert not kr.scan_valu_write_then_mfma_read(head + ["\ts_waitcnt lgkmcnt(7)", "\tds_read_b128 v[4:7], v71", mfma])
    assert not kr.scan_valu_write_then_mfma_read(head + [mfma.replace("v[0:3]", "v[4:7]")])
    assert kr.scan_valu_write_then_mfma_read(head[:1] + ["\tv_mov_b32_e32 v111, 0", "\ts_nop 0", mfma])   # the A operand counts too


def test_kernel_resources_static():
    """Static check of the built library (no GPU): every kernel is there for gfx950, fits the 160 KB LDS, and the kernels
    of the default path do not spill (scripts/kernel_resources.py reads the AMDGPU metadata of the embedded code objects)."""
    import importlib.util
    import shutil

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf") or not shutil.which("c++filt"):
        pytest.skip("llvm-readelf / c++filt not available")
    from perspectivefields_amd import build as _b

    lib = _b.build(verbose=False)
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(root, "scripts", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    rows = kr.kernels(lib)
    assert len(rows) >= 200
    assert all(r["lds"] <= 160 * 1024 for r in rows), [r for r in rows if r["lds"] > 160 * 1024]
    by = {r["kernel"]: r for r in rows}
    hot = [
        # default parity scheme (split-f16, NT_F16X3 = 23) and the exact bf16 split (6)
        "pf::igemm_sb_kernel<128, 128, 2, 2, 0, false, 1, 23, false>", "pf::igemm_sb_kernel<64, 64, 2, 2, 0, false, 1, 23, false>",
        "pf::igemm_sb_kernel<128, 64, 2, 2, 0, false, 1, 23, false>", "pf::igemm_sb_kernel<128, 32, 4, 1, 0, false, 1, 23, false>",
        "pf::igemm_sb_kernel<256, 256, 2, 4, 0, false, 1, 23, false>", "pf::igemm_sb_kernel<256, 128, 4, 2, 0, false, 1, 23, false>",
        "pf::igemm_sbh_kernel<8, 16, 128, 2, 2, 0, 1, 23, false, false, false>", "pf::igemm_sbh_kernel<8, 16, 64, 2, 2, 0, 1, 23, false, false, false>", "pf::igemm_sbh_kernel<8, 16, 32, 4, 1, 0, 1, 23, false, false, false>",
        "pf::igemm_sbh_kernel<16, 16, 64, 4, 2, 0, 1, 23, false, false, false>", "pf::igemm_sbh_kernel<8, 16, 64, 2, 2, 2, 1, 23, false, true, false>", "pf::igemm_sbh_kernel<8, 16, 32, 4, 1, 0, 1, 23, false, true, false>", "pf::sr_attention_f16_kernel", "pf::dwconv7x7_cb_kernel<4, 3, 0>", "pf::dwconv7x7_cb_kernel<2, 3, 0>",
        "pf::igemm_sb_kernel<128, 128, 2, 2, 0, false, 1, 6, false>", "pf::igemm_sb_kernel<64, 64, 2, 2, 0, false, 1, 6, false>",
        "pf::igemm_sb_kernel<128, 64, 2, 2, 0, false, 1, 6, false>", "pf::igemm_sb_kernel<128, 32, 4, 1, 0, false, 1, 6, false>",
        "pf::igemm_sb_kernel<256, 256, 2, 4, 0, false, 1, 6, false>",
        "pf::igemm_sbh_kernel<8, 16, 128, 2, 2, 0, 1, 6, false, false, false>", "pf::igemm_sbh_kernel<8, 16, 64, 2, 2, 0, 1, 6, false, false, false>", "pf::igemm_sbh_kernel<8, 16, 32, 4, 1, 0, 1, 6, false, false, false>",
        "pf::sr_attention_kernel", "pf::dwconv7x7_lane_kernel<1, 3, 256, 0>", "pf::upsample2x_cell_kernel",
        "pf::dwconv3x3_gelu_direct_kernel<32, 8, 8, 0>", "pf::layernorm_kernel<64, 2>",
        # r02: multi-column depthwise 3x3 (the three shipped forms) and the fused-LayerNorm GEMM forms of the 4-wave tiles
        "pf::dwconv3x3_gelu_mc_kernel<64, 2, 40, 2, 2, false>", "pf::dwconv3x3_gelu_mc_kernel<64, 4, 8, 1, 1, false>", "pf::dwconv3x3_gelu_mc_kernel<64, 4, 8, 2, 1, false>", "pf::dwconv3x3_gelu_mc_kernel<64, 5, 16, 1, 2, false>",
        "pf::cnx_mlp_kernel<96, 0>", "pf::mit_mlp_kernel<64, 8, 16, false>", "pf::mit_mlp_kernel<128, 8, 8, true>",  # fused block MLPs (hidden map on chip)
        "pf::igemm_sb_kernel<128, 128, 2, 2, 0, false, 1, 23, true>", "pf::igemm_sb_kernel<64, 64, 2, 2, 0, false, 2, 23, true>", "pf::igemm_sb_kernel<128, 256, 2, 4, 0, false, 1, 23, true>",
    ]
    # r03: the 128 x 64 halo tile with the two-buffer DMA weight ring keeps the 128-VGPR cap (four resident blocks) at the price of 8 registers spilled around the
    # once-per-chunk halo store (4 reloads per 32-channel chunk, none in the tap loop): measured faster than the uncapped form (profiles/r03_sbh_variants.txt)
    # ... and the LayerNorm-fused 128 x 256 / 8-wave tile spills 3 registers in its prologue since the pivot became a chunk mean
    few_spills = {"pf::igemm_sbh_kernel<8, 16, 64, 2, 2, 0, 1, 23, false, false, false>": 8, "pf::igemm_sb_kernel<128, 256, 2, 4, 0, false, 1, 23, true>": 3}
    hot += ["pf::dwconv7x7_lds_kernel<2, 13>"]
    for k in hot:
        assert k in by, (k, [n for n in by if n.startswith(k.split("<")[0])][:4])
        assert by[k]["spill"] <= few_spills.get(k, 0) and by[k]["scratch"] <= 6 * few_spills.get(k, 0), by[k]
    # the two-blocks-per-CU 8-wave tiles trade a handful of spilled registers for the second resident block
    assert by["pf::igemm_sb_kernel<256, 128, 4, 2, 0, false, 1, 6, false>"]["vgpr"] <= 128
    # Resident blocks per CU of the default-path GEMM tiles (r03, profiles/DESIGN_history_r01_r04.md 4.10): a shared epilogue that grew by 16 registers took `sb128x64` from 4 to 3 blocks and
    # the B = 64 stage-3 launches (1000 blocks) from one round to two, -2.9 % end to end with no spill to warn about.  512 VGPRs per SIMD lane in granules of 8, 160 KB LDS.
    blocks_per_cu = kr.blocks_per_cu
    floor = {"pf::igemm_sb_kernel<128, 64, 2, 2, 0, false, 1, 23, false>": 4, "pf::igemm_sb_kernel<128, 64, 2, 2, 0, false, 2, 23, false>": 3,
             "pf::igemm_sb_kernel<64, 64, 2, 2, 0, false, 1, 23, false>": 7, "pf::igemm_sb_kernel<64, 64, 2, 2, 0, false, 2, 23, false>": 5,
             "pf::igemm_sb_kernel<64, 64, 2, 2, 0, false, 1, 23, true>": 5, "pf::igemm_sb_kernel<64, 64, 2, 2, 0, false, 2, 23, true>": 4,
             "pf::igemm_sb_kernel<128, 32, 4, 1, 0, false, 1, 23, false>": 5, "pf::igemm_sb_kernel<128, 128, 2, 2, 0, false, 1, 23, false>": 3,
             "pf::igemm_sb_kernel<128, 128, 2, 2, 0, false, 1, 23, true>": 3, "pf::igemm_sb_kernel<128, 256, 2, 4, 0, false, 1, 23, true>": 2,
             "pf::igemm_sbh_kernel<16, 16, 64, 4, 2, 0, 1, 23, false, false, false>": 2, "pf::igemm_sbh_kernel<8, 16, 64, 2, 2, 0, 1, 23, false, false, false>": 4,
             "pf::mit_mlp_kernel<128, 8, 8, true>": 2}   # r06: the single-weight-buffer form exists for the second resident block
    for k, n in floor.items():
        assert blocks_per_cu(by[k]) >= n, (k, by[k], blocks_per_cu(by[k]), n)


def test_unscaled_low_plane_representation():
    """The split-f16 scheme's low plane (sb_split.h; adopted in r03, profiles/r03_candidates.md): lo = fp16_rn(x - hi) WITHOUT a 2^11 scale, relying
    on the matrix cores keeping fp16 subnormals (measured on gfx950).  Representation error: <= 2^-22 |x| while lo is a normal fp16 (|x| >= 2^-2 is sufficient),
    an ABSOLUTE 2^-25 below that (subnormal spacing 2^-24) -- i.e. what differs from the scaled form is the error of SMALL elements (2^-25 instead of 2^-36), which is
    harmless next to O(1) terms of the same dot product and a relative loss only for an all-tiny tensor."""
    rng = np.random.default_rng(3)
    x = (rng.standard_normal(200000) * np.exp(rng.uniform(-12, 8, 200000))).astype(np.float32)
    x = x[np.abs(x) <= 65504]
    hi = x.astype(np.float16)
    lo = (x - hi.astype(np.float32)).astype(np.float16)  # numpy keeps fp16 subnormals, like v_cvt_f16_f32 in the default float mode and like the MFMA inputs
    err = np.abs(hi.astype(np.float64) + lo.astype(np.float64) - x.astype(np.float64))
    big = np.abs(x) >= 0.25
    assert np.max(err[big] / np.abs(x[big])) <= 2.0 ** -22
    assert np.max(err[~big]) <= 2.0 ** -25
    # a dot product of O(1) data: same error level as the scaled form
    a = rng.standard_normal((32, 2304)).astype(np.float32)
    w = (rng.standard_normal((24, 2304)) / 48).astype(np.float32)
    ah = a.astype(np.float16); al = (a - ah.astype(np.float32)).astype(np.float16)
    mx = np.abs(w).max(axis=1, keepdims=True); S = np.ldexp(np.float32(1), 14 - np.frexp(mx)[1]).astype(np.float32)
    ws = w * S; wh = ws.astype(np.float16); wl = (ws - wh.astype(np.float32)).astype(np.float16)
    f = lambda t: t.astype(np.float64)
    got = (f(ah) @ f(wh).T + f(ah) @ f(wl).T + f(al) @ f(wh).T) / f(S).T
    ref = f(a) @ f(w).T
    scale = np.abs(f(a)) @ np.abs(f(w)).T
    assert np.max(np.abs(got - ref) / scale) <= 3 * 2.0 ** -22




def test_resize_transform_all_dtypes():
    """ResizeTransform.apply_image (reference perspectivefields.py:34-66): uint8 through PIL (3-channel and single-channel "L"), every other dtype through
    F.interpolate without antialiasing -- byte / bit identical to the unmodified reference where that tree exists, and to the stated formula everywhere."""
    import sys

    import torch
    from perspectivefields_amd.perspectivefields import ResizeTransform

    rng = np.random.default_rng(0)
    cases = [((97, 131, 3), np.float32), ((64, 64, 3), np.float64), ((50, 70, 1), np.uint8), ((50, 70, 3), np.uint8), ((33, 45), np.float32)]
    ref_rt = None
    if os.path.isdir("/root/reference/perspective2d"):
        sys.dont_write_bytecode = True
        from oracle import ref_shim

        ref_shim.install()
        import importlib

        ref_rt = importlib.import_module("perspective2d.perspectivefields").ResizeTransform  # ref_shim puts /root/reference first on sys.path: this is the reference's class
        if not importlib.import_module("perspective2d.perspectivefields").__file__.startswith("/root/reference"):
            ref_rt = None   # the repo's own alias package was imported earlier in this process: nothing to compare with
    for shape, dt in cases:
        img = (rng.random(shape) * 255).astype(dt)
        got = ResizeTransform(320, 320).apply_image(img)
        assert got.dtype == img.dtype and got.shape[:2] == (320, 320) and got.shape[2:] == img.shape[2:]
        if dt != np.uint8:
            t = torch.from_numpy(img)
            t4 = t.view(list(t.shape[:2]) + [1] * (4 - t.dim()) + list(t.shape[2:])).permute(2, 3, 0, 1)
            want = torch.nn.functional.interpolate(t4, (320, 320), mode="bilinear", align_corners=False).permute(2, 3, 0, 1).reshape(got.shape).numpy()
            assert np.array_equal(got, want)
        if ref_rt is not None:
            assert np.array_equal(got, ref_rt(320, 320).apply_image(img)), (shape, dt)


def test_verify_trained_script_without_weights(tmp_path):
    """scripts/verify_trained.py (the first-contact kit for trained checkpoints): without PF_WEIGHTS_DIR it lists the expected checkpoint files of the zoo and exits 2;
    it imports cleanly on a CPU box (no GPU work before the checks)."""
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k != "PF_WEIGHTS_DIR"}
    r = subprocess.run([sys.executable, os.path.join(root, "scripts", "verify_trained.py")], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 2, r.stderr[-500:]
    assert "paramnet_360cities_edina_rpf.pth" in r.stdout and "Paramnet-360Cities-edina-centered" in r.stdout
    r = subprocess.run([sys.executable, os.path.join(root, "scripts", "verify_trained.py")], capture_output=True, text=True, timeout=300, env=dict(env, PF_WEIGHTS_DIR=str(tmp_path)))
    # an (empty) weights directory: on a box without a GPU the script says so (2); on a GPU box every version is reported as "checkpoint not in PF_WEIGHTS_DIR" (0)
    assert (r.returncode == 2 and "no GPU visible" in r.stdout) or (r.returncode == 0 and "not in PF_WEIGHTS_DIR" in r.stdout), (r.returncode, r.stdout[-300:])


# Engine configurations that change what the forward allocates from the workspace (tests/test_gpu_batch_dispatch.py runs the same list on the GPU with guard bands)
WORKSPACE_CONFIGS = [{}, {"PF_FUSE_LN": "0"}, {"PF_RB_CHAIN": "0"}, {"PF_RB_CHAIN": "28"}, {"PF_SPLITK": "0"}, {"PF_SBA": "1"}, {"PF_FOLD_MLP": "0"}, {"PF_FUSE_UPSAMPLE": "0"}]


def test_workspace_dry_run_for_every_batch_and_configuration(monkeypatch):
    """The workspace dry run (a host-only engine, pf_create(PF_DEVICE_NONE), does it without a GPU) finishes for every batch 1..81, the three architectures, both
    precision schemes and every configuration of WORKSPACE_CONFIGS, and its size never shrinks when the batch grows.  The batches at which the per-image step
    changes are printed: each marks a batch gate that moves the peak.  (Seen: the steps into batch 4 and into batch 5 differ from their predecessors, i.e. ONE gate, at
    batch 4, in the split-f16 scheme; none in the exact scheme or with PF_SBA=1.  The decoders' 320 x 320 maps set the peak, so the stage-3 gates at 16 / 28 / 32 /
    64 do not show here: the GPU tests take those from the dispatch report, and run batch 4 as an edge of its own.)"""
    from concurrent.futures import ThreadPoolExecutor

    from perspectivefields_amd.engine import load_library

    lib = load_library()
    PF_DEVICE_NONE = -1
    engines = []
    for version in ("Paramnet-360Cities-edina-centered", "Paramnet-360Cities-edina-uncentered", "PersNet-360Cities"):
        sd = {k: (np.zeros((), dtype=np.float32) if k.endswith("num_batches_tracked") else np.ascontiguousarray(np.asarray(v), dtype=np.float32))
              for k, v in synthetic_state_dict(version, 0).items()}
        for cfg in WORKSPACE_CONFIGS:
            with monkeypatch.context() as m:   # the switches are read by pf_create
                for k, v in cfg.items():
                    m.setenv(k, v)
                h = ctypes.c_void_p()
                assert lib.pf_create(ctypes.byref(h), PF_DEVICE_NONE, arch_of(get_cfg(version))["arch_id"]) == 0, lib.pf_last_error(None)
            for key, arr in sd.items():
                shape = (ctypes.c_int64 * max(arr.ndim, 1))(*arr.shape)
                assert lib.pf_load_tensor(h, key.encode(), arr.ctypes.data_as(ctypes.c_void_p), shape, arr.ndim) == 0, lib.pf_last_error(h)
            engines.append((version, cfg, h))
    try:
        with ThreadPoolExecutor(max_workers=8) as pool:   # the weight folds / splits of the engines are independent (ctypes releases the GIL)
            rcs = list(pool.map(lambda e: lib.pf_finalize_weights(e[2]), engines))
        for (version, cfg, h), rc in zip(engines, rcs):
            assert rc == 0, (version, cfg, lib.pf_last_error(h))
            for precision, mode in (("fp32", 0), ("fp32_bf16x6", 3)):
                assert lib.pf_set_precision(h, mode) == 0, lib.pf_last_error(h)
                ws = [int(lib.pf_workspace_bytes(h, b)) for b in range(1, 82)]
                what = f"{version} {cfg or 'default'} {precision}"
                assert all(w > 0 for w in ws), what
                assert all(b >= a for a, b in zip(ws, ws[1:])), f"{what}: workspace_bytes shrinks with the batch: {ws}"
                assert int(lib.pf_workspace_bytes(h, 82)) == 0, what   # beyond PF_MAX_BATCH
                steps = [b - a for a, b in zip(ws, ws[1:])]
                edges = [b + 2 for b in range(1, len(steps)) if steps[b] != steps[b - 1]]
                print(f"{what}: B=1 {ws[0]} bytes, B=81 {ws[-1]} bytes, per-image step changes at batches {edges}")
            out = (ctypes.c_int64 * 32)()
            assert lib.pf_last_dispatch(h, out, 32) == 0 and not any(out), "a dry run must not touch the dispatch report"
            assert lib.pf_last_dispatch(h, out, 3) != 0   # too short an array is refused
    finally:
        for _, _, h in engines:
            lib.pf_destroy(h)


def test_fused_head_tile_list_is_host_logic():
    """pf_op_conv2d_head_tile_usable needs no device: tests/test_gpu_head_tail.py reads the tiles of the fused prediction head at collection.  The form runs on the
    BN = 32 split tiles only -- linear and halo ones -- for both head kinds; an exact-fp32 tile, a wider tile, a Winograd tile and a bad shape are refused."""
    from perspectivefields_amd import ops

    names = ops.conv_tiles()
    for kind in (1, 2):
        tiles = [names[t] for t in ops.conv2d_head_tiles(2, 17, 24, 64, 1, kind)]
        assert tiles and all(n.endswith(("x32", "x32f2")) for n in tiles), tiles
        assert any(n.startswith("sbh") for n in tiles) and any(n.startswith("sb") and not n.startswith("sbh") for n in tiles), tiles
    lib = ops.load_library()
    for bad in ("128x128p", "128x32p", "sb128x128", "sbh128x64", "wino256x64c"):
        assert lib.pf_op_conv2d_head_tile_usable(2, 17, 24, 64, 1, 1, names.index(bad)) == 0, bad
    ok = names.index("sb128x32")
    assert lib.pf_op_conv2d_head_tile_usable(2, 17, 24, 64, 1, 1, ok) == 1
    for args in ((0, 17, 24, 64, 1, 1), (2, 17, 24, 48, 1, 1), (2, 17, 24, 64, 3, 1), (2, 17, 24, 64, 1, 0), (2, 17, 24, 64, 1, 3), (81, 320, 320, 256, 1, 1)):
        assert lib.pf_op_conv2d_head_tile_usable(*args, ok) == 0, args
    assert lib.pf_op_conv2d_head_tile_usable(2, 17, 24, 64, 1, 1, -1) == 0 and lib.pf_op_conv2d_head_tile_usable(2, 17, 24, 64, 1, 1, len(names)) == 0


def test_conv2d_g_tile_lists_are_host_logic():
    """pf_op_conv2d_g_tile_usable needs no device: tests/test_gpu_conv_forms.py reads its tile lists at collection.  The fused x2 up-sampling runs on the 4-wave halo
    tiles of the split-f16 scheme only; two groups run wherever one does; a bias table runs everywhere but on the Winograd tiles; a fused head on the BN = 32 split
    tiles; and every precondition of pf_op_conv2d_g that the shape alone decides answers 0 for every tile."""
    from perspectivefields_amd import ops

    names = ops.conv_tiles()
    tiles = lambda **form: [names[t] for t in ops.conv2d_g_tiles(**form)]
    linear = lambda n: n.startswith("sb") and not n.startswith("sbh")
    halo = lambda n: n.startswith("sbh")
    ups = dict(B=2, H=6, W=10, C1=64, Cout=64, K=3, pad=1, ups=True)
    ups_t = tiles(**ups)
    assert all(halo(n) for n in ups_t) and any(n.startswith("sbh128x") for n in ups_t) and {"sbh256x32", "sbh256x64"} <= set(ups_t) and "sbh256x64w8" not in ups_t, ups_t
    assert tiles(**dict(ups, C2=32)) == ups_t == tiles(**dict(ups, groups=2)) == tiles(**dict(ups, has_table=True))
    ups_head = tiles(**dict(ups, Cout=32, act=1, head_kind=1))
    assert ups_head and set(ups_head) <= set(ups_t) and all(n.endswith("x32") for n in ups_head) and ups_head == tiles(**dict(ups, Cout=32, act=1, head_kind=2)), ups_head
    for bad in (dict(H=7), dict(W=9), dict(precision=3), dict(K=1, pad=0), dict(stride=2), dict(C1=48), dict(C2=16), dict(groups=3), dict(groups=0), dict(head_kind=1),
                dict(act=3), dict(precision=1), dict(B=0)):
        assert tiles(**dict(ups, **bad)) == [], bad
    plain = dict(B=1, H=10, W=10, C1=64, Cout=64, K=3, pad=1)
    plain_t = tiles(**plain)
    assert "128x128p" in plain_t and any(linear(n) for n in plain_t) and set(ups_t) <= set(plain_t) and {"wino256x64c", "wino256x64d"} <= set(plain_t), plain_t
    assert tiles(**dict(plain, groups=2)) == plain_t
    exact = tiles(**dict(plain, precision=3))   # the exact bf16 split: no Winograd, no split-f16-only halo tile
    assert set(exact) < set(plain_t) and "128x128p" in exact and any(linear(n) for n in exact) and any(halo(n) for n in exact), exact
    assert not any(n.startswith("wino") or n in ("sbh256x32", "sbh256x64") for n in exact), exact
    assert tiles(**dict(plain, has_table=True)) == [n for n in plain_t if not n.startswith("wino")]
    for H, W in ((1, 10), (10, 1)):
        assert tiles(**dict(plain, H=H, W=W)) and tiles(**dict(plain, H=H, W=W, has_table=True)) == []
    one = tiles(**dict(plain, K=1, pad=0, Cout=96, groups=2))
    assert "128x128p" in one and any(linear(n) for n in one) and not any(halo(n) or n.startswith("wino") for n in one), one
    heads = tiles(**dict(plain, Cout=32, act=1, groups=2, head_kind=1))
    assert any(linear(n) for n in heads) and any(halo(n) for n in heads) and all(n.endswith(("x32", "x32f2")) for n in heads), heads
    assert "128x32p" not in heads and tiles(**dict(plain, Cout=64, head_kind=1)) == []
    lib = ops.load_library()
    args = (1, 10, 10, 64, 0, 64, 3, 3, 1, 1, 0, 2, 0, 0, 0, 0)
    assert lib.pf_op_conv2d_g_tile_usable(*args, -1) == 0 and lib.pf_op_conv2d_g_tile_usable(*args, len(names)) == 0 and lib.pf_op_conv2d_g_tile_usable(*args, 0) == 1


def test_conv2d_g_refuses_a_tile_before_any_device_work():
    """pf_op_conv2d_g decides the tile on the operand set of the usability query, before it asks for a device or uploads a weight: a named tile that cannot run the form,
    and a form that no tile runs, are PF_ERR_ARG with that reason -- here too, where no call reaches a device.  Host buffers stand in for the device tensors: a refused
    call reads none of them (only refused calls are made)."""
    from perspectivefields_amd import ops

    PF_ERR_ARG = -1  # include/pf_hip.h
    lib = ops.load_library()
    names = ops.conv_tiles()
    B, H, W, C, Cout = 1, 6, 6, 64, 64
    x, y = np.zeros(B * H * W * C + 4, np.float32), np.zeros(B * H * W * Cout + 4, np.float32)
    w, tab = np.zeros((Cout, C, 3, 3), np.float32), np.zeros((9, Cout), np.float32)
    al = lambda a: a.ctypes.data + (-a.ctypes.data) % 16
    ptr = lambda v: (ctypes.c_void_p * 1)(v)
    used = ctypes.c_int(0)

    def call(tile, K=3, pad=1, stride=1, ups=0, rows=1):
        rc = lib.pf_op_conv2d_g(0, 1, ptr(al(x)), None, B, H, W, C, 0, ptr(w.ctypes.data), ptr(tab.ctypes.data), (ctypes.c_int * 1)(rows), Cout, K, K, stride, pad, 0,
                                None, None, 0, ups, ptr(al(y)), (ctypes.c_int * 1)(0), None, None, None, None, tile, 0, -1, ctypes.byref(used), None)
        return rc, (lib.pf_last_error(None) or b"").decode()

    for tile, kw in ((names.index("128x128p"), dict(ups=1)), (names.index("sb128x128"), dict(ups=1)), (names.index("sbh256x64w8"), dict(ups=1)),
                     (names.index("wino256x64c"), dict(rows=9)), (names.index("sbh128x64"), dict(K=1, pad=0))):
        rc, msg = call(tile, **kw)
        assert rc == PF_ERR_ARG and f"({names[tile]}) cannot run this form" in msg, (names[tile], kw, rc, msg)
    for kw in (dict(ups=1, K=1, pad=0), dict(ups=1, stride=2)):
        rc, msg = call(-1, **kw)
        assert rc == PF_ERR_ARG and "no tile runs this form" in msg, (kw, rc, msg)


def test_a_nan_output_cannot_pass_the_kernel_bounds():
    """the accumulation of the kernel-level GPU tests (tests/kernel_bounds.py): an output element that is NaN -- unwritten under ops.checked_outputs() -- gives a NaN
    ratio, the running worst keeps it whatever comes before or after, and `worst <= 1.0` is then false"""
    from tests.kernel_bounds import _ratio, _worse

    nan = float("nan")
    r = _ratio(np.abs(np.array([0.1, nan]) - np.array([0.1, 0.2])), np.array([1.0, 1.0]))
    assert math.isnan(r)
    for seq in ((r, 0.5), (0.5, r), (0.2, r, 0.9), (r,)):
        worst = 0.0
        for v in seq:
            worst = _worse(worst, v)
        assert math.isnan(worst) and not worst <= 1.0, seq
    assert math.isnan(_worse(0.0, 0.3, nan, 0.4)) and _worse(0.0, 0.3, 0.7, 0.4) == 0.7 and _worse(0.5, 0.3) == 0.5 and _worse(0.0, float("inf")) == float("inf")
