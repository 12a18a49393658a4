"""Reads two rocprofv3 kernel traces of bench.py (profiles/r08_dec_early.md): per-kernel totals per step and, for the last two steps, the span on the timeline of
MiT stage 4 + decoder levels 3 / 2 on the main queue and which kernels, on which queue, overlap it.

    rocprofv3 --kernel-trace --stats -d DIR/parent -o parent --output-format csv -- python bench.py --gpus 1 --steps 10 --warmup 3   # library of the parent commit
    rocprofv3 --kernel-trace --stats -d DIR/branch -o branch --output-format csv -- python bench.py --gpus 1 --steps 10 --warmup 3
    python scripts/trace_dec_window.py DIR"""
import csv, glob, sys, collections

def load(d):
    f = glob.glob(d + "/**/*kernel_trace.csv", recursive=True)
    rows = []
    with open(f[0]) as fh:
        for r in csv.DictReader(fh):
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"], r.get("Stream_Id", r.get("Queue_Id", "?")), int(r.get("Grid_Size_X", r.get("Grid_Size", 0)) or 0), int(r.get("Workgroup_Size_X", r.get("Workgroup_Size", 1)) or 1)))
    rows.sort()
    return rows

def short(n):
    n = n.replace("pf::", "")
    return n[:n.index("<")] if "<" in n else n[:40]

for tag in ("parent", "branch"):
    rows = load(sys.argv[1] + "/" + tag)
    # steps are delimited by the conv_fuse_conv1 launch: the largest grid of the step; find it as the kernel with the largest blocks count
    blocks = [g // max(w, 1) for _, _, _, _, g, w in rows]
    big = max(blocks)
    ends = [i for i, b in enumerate(blocks) if b == big]
    print(f"== {tag}: {len(rows)} launches, {len(ends)} launches of the largest grid ({big} blocks: conv_fuse_conv1, one per step)")
    tot = collections.Counter(); cnt = collections.Counter()
    for s, e, n, q, g, w in rows:
        tot[short(n)] += e - s; cnt[short(n)] += 1
    steps = len(ends)
    for n, t in tot.most_common(14):
        print(f"   {n:44s} {cnt[n] / steps:7.1f} launches/step {t / steps / 1e6:8.3f} ms/step")
    print(f"   all kernels {sum(tot.values()) / steps / 1e6:.3f} ms/step (sum of kernel times)")
    # window: in the last full step, from the last sr_attention-free stage ... use the attention launches: stage 4 has sr = 1 -> its attention launches are the LAST
    # three attention launches before the step's first wino / decoder launch; the window runs from the end of the third-last layernorm before them to the first 80^2 wino launch
    if len(ends) < 3: continue
    for step in (len(ends) - 2, len(ends) - 1):
        lo, hi = ends[step - 1] + 1, ends[step]
        seg = rows[lo:hi + 1]
        att = [i for i, r in enumerate(seg) if "attention" in r[2] or "attn" in r[2]]
        if len(att) < 3: continue
        a0 = att[-3]
        # stage 4 begins with its patch embedding: walk back from the first stage-4 attention to the preceding dwconv3x3 (last launch kind of a stage-3 block is fc2; the dw before the embed)
        t0 = seg[a0][0]
        main_q = seg[a0][3]
        # window start: end of the last stage-3 launch on the attention's queue = the launch 4 before stage 4's first attention (embed, LN, [LN-fused q / kv])
        prev = [r for r in seg[:a0] if r[3] == main_q]
        t_start = prev[-5][1] if len(prev) >= 5 else t0
        winos = [r for r in seg[a0:] if "wino" in r[2] and (r[4] // max(r[5], 1)) >= 1000 and r[3] == main_q]
        t_end = winos[0][0] if winos else seg[-1][0]
        inside = collections.Counter(); busy = collections.Counter()
        for s, e, n, q, g, w in seg:
            ov = min(e, t_end) - max(s, t_start)
            if ov > 0:
                inside[(short(n), "same queue" if q == main_q else "other queue")] += 1; busy[(short(n), "same queue" if q == main_q else "other queue")] += ov
        print(f"   step {step}: window (stage-4 start -> first 80^2 Winograd launch on the main queue) {(t_end - t_start) / 1e3:.1f} us")
        for k, v in sorted(busy.items(), key=lambda kv: -kv[1])[:12]:
            print(f"      {k[0]:40s} {k[1]:12s} {inside[k]:3d} launches {v / 1e3:8.1f} us inside the window")
        print(f"      kernel time inside the window: same queue {sum(v for k, v in busy.items() if k[1] == 'same queue') / 1e3:.1f} us, other queues {sum(v for k, v in busy.items() if k[1] != 'same queue') / 1e3:.1f} us")
