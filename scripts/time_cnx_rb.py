"""Timing of the row-block ConvNeXt block MLP (cnx_rb.hip, PF_CNX_RB) against the GEMM pair it replaces; the figures of profiles/r07_cnx_rb.md come from here.

  fused   [C] [M ...]   ops.cnx_mlp(iters=200): average us per launch of the fused kernel, launches back to back
  pair    [C] [M ...]   20 x (ops.linear_ln(act=2), ops.linear(res1=y)) per M, nothing printed: run it under
                        `rocprofv3 --kernel-trace --output-format csv -d DIR -o pair -- python scripts/time_cnx_rb.py pair`
  trace   DIR           average duration per (kernel, grid size) of every *kernel_trace.csv below DIR; the first launch of each is left out
  latency [B ...]       joined, synchronous forwards (the default-constructed model's way) of one engine with PF_CNX_RB=0 and one with the default, in ONE process,
                        alternating blocks of 30 forwards, 6 blocks each: ms per forward of every block, the mean and the spread (max - min) of each setting
"""
import csv
import glob
import math
import os
import re
import sys
import time
from collections import defaultdict

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _weights(C):
    import torch

    g = torch.Generator().manual_seed(7)
    r = lambda *s: torch.randn(s, generator=g)
    return r(4 * C, C) / math.sqrt(C), 0.1 * r(4 * C), 1 + 0.3 * r(C), 0.2 * r(C), r(C, 4 * C) / math.sqrt(4 * C), 0.1 * r(C), 0.5 * r(C)


def _args(argv, default_ms):
    C = int(argv[0]) if argv else 384
    return C, [int(a) for a in argv[1:]] or default_ms


def fused(argv):
    import torch
    from perspectivefields_amd import ops

    C, Ms = _args(argv, [3200, 6400, 12800])
    w1, b1, g, be, w2, b2, ls = _weights(C)
    for M in Ms:
        d, y = torch.randn(M, C, device="cuda"), torch.randn(M, C, device="cuda")
        ms = ops.cnx_mlp(d, y, w1, b1, g, be, 1e-6, w2, b2, ls, iters=200)
        print(f"cnx_rb C={C} M={M} blocks={-(-M // (64 if C == 384 else 32))}: {1e3 * ms:.1f} us/launch", flush=True)


def pair(argv):
    import torch
    from perspectivefields_amd import ops

    C, Ms = _args(argv, [3200, 6400, 12800])
    w1, b1, g, be, w2, b2, ls = _weights(C)
    w2s, b2s = w2 * ls[:, None], b2 * ls
    for M in Ms:
        d, y = torch.randn(M, C, device="cuda"), torch.randn(M, C, device="cuda")
        for _ in range(20):
            hid = ops.linear_ln(d, w1, b1, g, be, 1e-6, act=2)
            ops.linear(hid, w2s, b2s, res1=y)
        torch.cuda.synchronize()


def trace(argv):
    agg = defaultdict(list)
    for f in glob.glob(os.path.join(argv[0], "**", "*kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            name = re.sub(r"\(.*$", "", r["Kernel_Name"])
            agg[(name, int(r["Grid_Size_X"]), int(r["Workgroup_Size_X"]))].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    for (name, grid, wg), us in sorted(agg.items(), key=lambda kv: -sum(kv[1])):
        if "pf::" not in name:
            continue
        us = us[1:] or us
        print(f"{sum(us) / len(us):8.1f} us avg  min {min(us):7.1f}  calls {len(us):4d}  blocks {grid // wg:5d}  {name}")


def latency(argv):
    import numpy as np
    import torch
    from perspectivefields_amd import PerspectiveFields
    from perspectivefields_amd.synth import synthetic_image

    batches = [int(a) for a in argv] or [8, 16]
    engines = {}
    keep = []
    for name, val in (("PF_CNX_RB=0", "0"), ("default", None)):
        if val is None:
            os.environ.pop("PF_CNX_RB", None)
        else:
            os.environ["PF_CNX_RB"] = val
        m = PerspectiveFields("Paramnet-360Cities-edina-centered", weights="synthetic:0").eval().cuda()
        engines[name] = m._get_engine()
        keep.append(m)
    os.environ.pop("PF_CNX_RB", None)
    x_all = torch.from_numpy(np.stack([keep[0].aug.apply_image(synthetic_image(640, 640, seed=900 + i)) for i in range(max(batches))])).cuda()
    for B in batches:
        x = x_all[:B].contiguous()
        res = {k: [] for k in engines}
        for k, e in engines.items():
            for _ in range(5):
                e.forward(x)
            torch.cuda.synchronize()
            print(f"B={B} {k}: cnx_rb_launches {e.last_dispatch()['cnx_rb_launches']}", flush=True)
        for _ in range(6):
            for k, e in engines.items():
                for _ in range(3):
                    e.forward(x)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(30):
                    e.forward(x)
                    torch.cuda.synchronize()
                res[k].append(1e3 * (time.perf_counter() - t0) / 30)
        for k, v in res.items():
            print(f"B={B} {k:12s} ms/forward " + " ".join(f"{t:.3f}" for t in v) + f"  mean {sum(v) / len(v):.3f} spread {max(v) - min(v):.3f}", flush=True)
        off, on = res["PF_CNX_RB=0"], res["default"]
        print(f"B={B} default - off: {sum(on) / len(on) - sum(off) / len(off):+.3f} ms; fastest off {min(off):.3f} slowest off {max(off):.3f} fastest default {min(on):.3f} slowest default {max(on):.3f}", flush=True)


if __name__ == "__main__":
    {"fused": fused, "pair": pair, "trace": trace, "latency": latency}[sys.argv[1]](sys.argv[2:])
