"""Throughput of non-square inputs (rows x cols) against the square networks, in one process.

  python tools/rect_bench.py [--reps 7] [--steps 20] [--output-stride 32,16,8] [--configs f32_1.0_224x224,bf16_1.0_224x224]
      --output-stride: every chosen configuration once per listed output stride (mbn_plan_build_os; `_osN` is appended to the name
      of the 16 / 8 plans), timed alternately with the others; --configs: only the named configurations
      images/s and Mpixel/s (input pixels) of the configurations below, alternating within every repetition; each figure is the median
      over the repetitions of `steps` back-to-back forwards between two stream marks. Then each configuration's launch list (first layer,
      layers) and its per-layer forward_timed times (one launch per layer), so a shortfall names the layer responsible. Ratios: each
      non-square shape's Mpixel/s over its square companion's. One JSON object at the end.
"""
import argparse
import json
import os
import statistics
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mbn_amd import import_package  # noqa: E402

CLASSES = 1000
# (name, dtype, alpha, rows, cols, batch); a shape's square companion is the first entry of its (dtype, alpha) group
CONFIGS = [
    ("f32_1.0_224x224", "f32", 1.0, 224, 224, 256),
    ("f32_1.0_224x320", "f32", 1.0, 224, 320, 256),
    ("f32_1.0_320x224", "f32", 1.0, 320, 224, 256),
    ("f32_1.0_480x640", "f32", 1.0, 480, 640, 64),
    ("bf16_1.0_224x224", "bf16", 1.0, 224, 224, 512),
    ("bf16_1.0_224x320", "bf16", 1.0, 224, 320, 512),
    ("bf16_0.5_160x160", "bf16", 0.5, 160, 160, 512),
    ("bf16_0.5_160x128", "bf16", 0.5, 160, 128, 512),
]


def timed(ctx, net, d_in, d_out, batch, steps):
    ctx.mark()
    for _ in range(steps):
        net.forward(d_in.ptr, d_out.ptr, batch)
    ctx.mark()
    ms = ctx.marks_read(4)
    return batch * steps / (sum(ms) / 1e3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--output-stride", default="32", help="comma list of 32, 16, 8")
    ap.add_argument("--configs", default="", help="comma list of configuration names (default: all)")
    a = ap.parse_args()
    strides = [int(x) for x in a.output_stride.split(",")]
    chosen = [c for c in CONFIGS if not a.configs or c[0] in a.configs.split(",")]
    configs = [(name if os_ == 32 else "%s_os%d" % (name, os_), dtype, alpha, rows, cols, batch, os_)
               for name, dtype, alpha, rows, cols, batch in chosen for os_ in strides]
    pkg = import_package()
    result = {}
    with tempfile.TemporaryDirectory() as d, pkg.Context(0) as ctx:
        weights, runs = {}, {}
        for name, dtype, alpha, rows, cols, batch, os_ in configs:
            if alpha not in weights:
                path = os.path.join(d, "w_%g.h5" % alpha)
                pkg.synthetic_h5(path, alpha=alpha, classes=CLASSES, seed=7)
                weights[alpha] = path
            hw = pkg.HostWeights(weights[alpha], res=(rows, cols), output_stride=os_)
            net = pkg.Net(ctx, hw.plan, hw.blob.copy(), batch)
            if dtype == "bf16":
                net.set_dtype(pkg.DT_BF16)
            imgs = np.random.default_rng(0).uniform(-1, 1, (batch, rows, cols, 3)).astype(np.float32)
            d_in, d_out = ctx.to_device(imgs), ctx.alloc(batch * CLASSES * 4)
            runs[name] = dict(net=net, hw=hw, d_in=d_in, d_out=d_out, batch=batch, px=rows * cols, ips=[])
            timed(ctx, net, d_in, d_out, batch, 3)                  # warm-up
        for _ in range(a.reps):
            for name, r in runs.items():
                r["ips"].append(timed(ctx, r["net"], r["d_in"], r["d_out"], r["batch"], a.steps))
        for name, dtype, alpha, rows, cols, batch, os_ in configs:
            r = runs[name]
            ips = statistics.median(r["ips"])
            ms = r["net"].forward_timed(r["d_in"].ptr, r["d_out"].ptr, batch)
            result[name] = {"images_per_s": round(ips), "mpixel_per_s": round(ips * r["px"] / 1e6, 1),
                            "runs": [round(x) for x in r["ips"]], "launches": r["net"].launches(batch),
                            "layer_ms": [round(x, 4) for x in ms]}
            print("%-18s batch %4d %9d images/s %9.1f Mpixel/s  %s" % (name, batch, result[name]["images_per_s"], result[name]["mpixel_per_s"],
                                                                      [c for _, c in result[name]["launches"]]), flush=True)
        ratios = {}
        for name, dtype, alpha, rows, cols, batch, os_ in configs:
            sq = next((n for n, dt, al, rr, cc, _, o in configs if dt == dtype and al == alpha and rr == cc and o == os_), None)
            if sq is not None and name != sq:
                ratios[name] = round(result[name]["mpixel_per_s"] / result[sq]["mpixel_per_s"], 3)
        result["mpixel_ratio_to_square"] = ratios
        print("Mpixel/s over the square shape's:", ratios)
        for r in runs.values():
            r["net"].destroy()
            r["d_in"].free()
            r["d_out"].free()
            r["hw"].free()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
