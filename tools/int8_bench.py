"""Throughput of the int8 inference mode against the bf16 and fp32 paths, in one process (include/mbn.h, "int8 inference mode").

  python tools/int8_bench.py [--reps 5] [--steps 20] [--batch 512]
      images/s at 1.0x224 and 0.5x160: I8 after calibration, bf16 default, bf16 with every fusion off (set_fuse_blocks(0),
      set_fuse_resident(0)), fp32 default. The configurations alternate within every repetition; each figure is the median over the
      repetitions of `steps` back-to-back forwards between two stream marks. Then the I8 per-layer times of forward_timed with the
      layer's algorithmic HBM bytes (input + output + filter) over its time, as a fraction of 8 TB/s. One JSON object at the end.
  python tools/int8_bench.py --trace [--steps 20]
      I8 forwards only (1.0x224 batch 512), for `rocprofv3 --kernel-trace --stats -- python tools/int8_bench.py --trace`.
  python tools/int8_bench.py --stats kernel_stats.csv [--steps 20]
      the rocprofv3 stats of such a run as a table of the I8 kernels: calls, total time, algorithmic bytes, bytes over kernel time.
"""
import argparse
import csv
import json
import os
import statistics
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mbn_amd import import_package  # noqa: E402

HBM = 8.0e12
CLASSES = 1000


def layer_bytes(plan, l, batch):
    """algorithmic HBM bytes of one I8 layer launch: input read once, output written once, int8 filter (fp32 for conv1)"""
    inb = batch * l.in_rows * l.in_cols * l.in_ch * (4 if l.kind == 1 else 1)
    outb = batch * l.out_rows * l.out_cols * l.out_ch * (4 if l.kind == 5 else 1)
    wb = l.w_count * (4 if l.kind == 1 else 1) if l.kind != 4 else 0
    return inb + outb + wb


def kernel_class(l):
    return {1: "i8_conv_k", 2: "i8_dw_k<%d>" % l.stride, 3: "i8_pw", 4: "i8_pool_k", 5: "i8_pw"}[l.kind]


def make_weights(pkg, alpha, res, d):
    path = os.path.join(d, "w_%g_%d.h5" % (alpha, res))
    pkg.synthetic_h5(path, alpha=alpha, classes=CLASSES, seed=7)
    return pkg.HostWeights(path, res=res)


def build_nets(pkg, ctx, hw, batch, d_in):
    nets = {}
    for name in ("i8", "bf16", "bf16_nofuse", "fp32"):
        net = pkg.Net(ctx, hw.plan, hw.blob.copy(), batch)
        if name == "i8":
            net.calibrate_i8(d_in.ptr, min(batch, 64))
            net.set_dtype(pkg.DT_I8)
        elif name.startswith("bf16"):
            net.set_dtype(pkg.DT_BF16)
            if name == "bf16_nofuse":
                net.set_fuse_blocks(0)
                net.set_fuse_resident(0)
        nets[name] = net
    return nets


def timed(ctx, net, d_in, d_out, batch, steps):
    ctx.mark()
    for _ in range(steps):
        net.forward(d_in.ptr, d_out.ptr, batch)
    ctx.mark()
    ms = ctx.marks_read(4)
    return batch * steps / (sum(ms) / 1e3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--stats")
    a = ap.parse_args()
    pkg = import_package()
    if a.stats:
        plan = pkg.plan_build(1.0, 224, CLASSES)
        byts, calls_per_fwd = {}, {}
        for i in range(plan.n_layers):
            l = plan.layer[i]
            k = kernel_class(l)
            byts[k] = byts.get(k, 0) + layer_bytes(plan, l, a.batch)
            calls_per_fwd[k] = calls_per_fwd.get(k, 0) + 1
        rows = list(csv.DictReader(open(a.stats)))
        print("%-16s %7s %10s %12s %9s %8s" % ("kernel", "calls", "total ms", "GB / fwd", "TB/s", "of 8TB/s"))
        for k in byts:
            hit = [r for r in rows if k in r.get("Name", r.get("KernelName", ""))]
            calls = sum(int(r["Calls"]) for r in hit)
            ns = sum(float(r["TotalDurationNs"]) for r in hit)
            if not calls:
                continue
            fwds = calls / calls_per_fwd[k]
            tbs = byts[k] * fwds / (ns * 1e-9) / 1e12
            print("%-16s %7d %10.3f %12.3f %9.2f %8.2f" % (k, calls, ns / 1e6, byts[k] / 1e9, tbs, tbs * 1e12 / HBM))
        return
    result = {}
    with tempfile.TemporaryDirectory() as d, pkg.Context(0) as ctx:
        shapes = [(1.0, 224)] if a.trace else [(1.0, 224), (0.5, 160)]
        for alpha, res in shapes:
            hw = make_weights(pkg, alpha, res, d)
            imgs = np.random.default_rng(0).uniform(-1, 1, (a.batch, res, res, 3)).astype(np.float32)
            d_in = ctx.to_device(imgs)
            d_out = ctx.alloc(a.batch * CLASSES * 4)
            if a.trace:
                net = pkg.Net(ctx, hw.plan, hw.blob.copy(), a.batch)
                net.set_dtype(pkg.DT_I8)
                for _ in range(a.steps):
                    net.forward(d_in.ptr, d_out.ptr, a.batch)
                ctx.sync()
                net.destroy()
                return
            nets = build_nets(pkg, ctx, hw, a.batch, d_in)
            for net in nets.values():                     # warm-up
                timed(ctx, net, d_in, d_out, a.batch, 3)
            runs = {k: [] for k in nets}
            for _ in range(a.reps):
                for k, net in nets.items():
                    runs[k].append(timed(ctx, net, d_in, d_out, a.batch, a.steps))
            key = "%gx%d_b%d" % (alpha, res, a.batch)
            result[key] = {k: round(statistics.median(v)) for k, v in runs.items()}
            result[key]["runs"] = {k: [round(x) for x in v] for k, v in runs.items()}
            ms = nets["i8"].forward_timed(d_in.ptr, d_out.ptr, a.batch)
            per = []
            for i in range(hw.plan.n_layers):
                l = hw.plan.layer[i]
                b = layer_bytes(hw.plan, l, a.batch)
                per.append({"layer": i + 1, "kind": kernel_class(l), "ms": round(ms[i], 4), "MB": round(b / 1e6, 1),
                            "hbm_frac": round(b / (ms[i] * 1e-3) / HBM, 3) if ms[i] > 0 else None})
            result[key]["i8_layers"] = per
            for k in ("i8", "bf16", "bf16_nofuse", "fp32"):
                print("%s %-12s %9d images/s  %s" % (key, k, result[key][k], result[key]["runs"][k]))
            for p in per:
                print("  L%-2d %-12s %8.4f ms %9.1f MB  %.3f of 8 TB/s" % (p["layer"], p["kind"], p["ms"], p["MB"], p["hbm_frac"] or 0))
            for net in nets.values():
                net.destroy()
            d_in.free()
            d_out.free()
            hw.free()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
