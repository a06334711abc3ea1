"""The nearest-neighbour search (mbn_similarity_topk_f32) against torch-ROCm's (q @ g.T).topk(k) on the same buffers, in one process.

  python tools/similarity_bench.py [--reps 7] [--steps 20] [--cells 1x100000,32x100000,256x100000,4096x1000] [--k 1,8] [--log]
      Cells: D = 1024, (Q, G) as listed, k = 1 and 8. Inputs are integer-valued in [-8, 8] (torch-owned device tensors), so every sum is exact
      in fp32 in any order and the two routes must agree: the k best VALUES of every row are compared for equality, and the indices on every
      row whose k + 1 best values are distinct (torch.topk leaves the order of equal values open; the kernel's is the lowest index).
      Per cell, alternating within every repetition after a warm-up of both:
        kernel   mbn_similarity_topk_f32 (two launches), us per call
        torch    the yardstick, not the code under test: (q @ g.T).topk(k), which writes and re-reads the [Q][G] product
      Each figure is a host clock around `steps` calls that end in a device synchronise: the median over the repetitions and their range.
      floor = the larger of G * D * 4 bytes over 8 TB/s and 2 * Q * G * D over the fp32 MFMA peak (157.3 TFLOP/s): the share of it is floor /
      kernel time, a whole-call figure (both launches and their launch gaps), not a kernel's share of peak. Q is padded to 32 columns of the
      MFMA inside the kernel; the floor counts the Q asked for.
  python tools/similarity_bench.py --gallery-dtype bf16 [the same options]
      The search on a bf16 gallery, in one process on the same values (integers in [-8, 8] are exact in bf16, so all three routes must agree):
        kernel   mbn_similarity_topk_bf16 (three launches: the query split, the fused bf16 MFMA GEMM + top-k, the merge)
        f32      mbn_similarity_topk_f32 on the gallery widened to fp32 (twice the bytes): what a bf16 gallery cost before
        torch    (q.bfloat16() @ g.T).float().topk(k) on the bf16 gallery: it rounds the QUERIES to bf16, which the kernel does not, and its
                 PRODUCT to bf16 as well, so it is timed only: values and indices are compared with the exact fp32 product (q @ g.T).topk(k)
      floor = the larger of G * D * 2 bytes over 8 TB/s and the 3 * Q * G * D products of the three query planes over the bf16 MFMA peak
      (2516.6 TFLOP/s).
      One JSON object at the end; --log prints the table of profiles/LOG.md as well. No GPU: the Context raises; nothing falls back.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mbn_amd import import_package  # noqa: E402

D = 1024
HBM_BYTES_PER_S = 8.0e12                    # spec
MFMA_F32_FLOPS = 157.3e12                   # spec: the fp32 matrix peak
MFMA_BF16_FLOPS = 2516.6e12                 # spec: the bf16 matrix peak, dense


def floor_us(Q, G, bf16=False):
    mem, mfma = G * D * 4 / HBM_BYTES_PER_S, 2.0 * Q * G * D / MFMA_F32_FLOPS
    if bf16:
        mem, mfma = G * D * 2 / HBM_BYTES_PER_S, 2.0 * 3 * Q * G * D / MFMA_BF16_FLOPS
    return 1e6 * max(mem, mfma), "HBM" if mem >= mfma else "MFMA"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--cells", default="1x100000,32x100000,256x100000,4096x1000")
    ap.add_argument("--k", default="1,8")
    ap.add_argument("--gallery-dtype", default="f32", choices=["f32", "bf16"])
    ap.add_argument("--log", action="store_true")
    args = ap.parse_args()
    import torch
    pkg = import_package()
    dev = torch.device("cuda:0")
    bf16 = args.gallery_dtype == "bf16"
    results = []
    with pkg.Context(0) as ctx:
        for cell in args.cells.split(","):
            Q, G = (int(v) for v in cell.split("x"))
            gen = torch.Generator(device=dev).manual_seed(Q + G)
            q, g = (torch.randint(-8, 9, (n, D), device=dev, generator=gen).float() for n in (Q, G))
            for k in (int(v) for v in args.k.split(",")):
                idx, sc = torch.empty((Q, k), dtype=torch.int32, device=dev), torch.empty((Q, k), dtype=torch.float32, device=dev)
                ws = torch.empty(pkg.similarity_workspace_bytes(Q, G, D, k), dtype=torch.uint8, device=dev)
                if bf16:
                    gb, qb = g.bfloat16(), q.bfloat16()
                    wsb = torch.empty(pkg.similarity_workspace_bytes_bf16(Q, G, D, k), dtype=torch.uint8, device=dev)
                torch.cuda.synchronize()

                def kernel_f32():
                    ctx.similarity_topk(idx.data_ptr(), sc.data_ptr(), q.data_ptr(), g.data_ptr(), Q, G, D, k, ws.data_ptr())

                def kernel_bf16():
                    ctx.similarity_topk_bf16(idx.data_ptr(), sc.data_ptr(), q.data_ptr(), gb.data_ptr(), Q, G, D, k, wsb.data_ptr())

                def yardstick():
                    return (qb @ gb.T).float().topk(k) if bf16 else (q @ g.T).topk(k)
                kernel = kernel_bf16 if bf16 else kernel_f32

                def timed(fn, sync):
                    t0 = time.perf_counter()
                    for _ in range(args.steps):
                        fn()
                    sync()
                    return 1e6 * (time.perf_counter() - t0) / args.steps
                for _ in range(3):                                   # warm-up of both
                    kernel(), yardstick()
                ctx.sync(), torch.cuda.synchronize()
                tv, ti = (q @ g.T).topk(k)
                torch.cuda.synchronize()
                values_equal = bool(torch.equal(sc, tv))
                top = (q @ g.T).topk(min(k + 1, G)).values
                distinct = (top[:, 1:] != top[:, :-1]).all(1)
                indices_equal = bool(torch.equal(idx[distinct].long(), ti[distinct]))
                t_k, t_t, t_f = [], [], []
                for _ in range(args.reps):
                    t_k.append(timed(kernel, ctx.sync))
                    t_t.append(timed(yardstick, torch.cuda.synchronize))
                    if bf16:
                        t_f.append(timed(kernel_f32, ctx.sync))
                fl, bound = floor_us(Q, G, bf16)
                med_k, med_t = statistics.median(t_k), statistics.median(t_t)
                results.append(dict(Q=Q, G=G, D=D, k=k, kernel_us=med_k, kernel_range=[min(t_k), max(t_k)], torch_us=med_t,
                                    torch_range=[min(t_t), max(t_t)], floor_us=fl, bound=bound, share_of_floor=fl / med_k,
                                    values_equal=values_equal, indices_equal=indices_equal, rows_compared=int(distinct.sum())))
                r = results[-1]
                if bf16:
                    r.update(gallery_dtype="bf16", f32_us=statistics.median(t_f), f32_range=[min(t_f), max(t_f)])
                    print("    bf16 gallery; mbn_similarity_topk_f32 on the widened gallery %8.1f us (%.1f-%.1f): %.2f of it"
                          % (r["f32_us"], min(t_f), max(t_f), med_k / r["f32_us"]), flush=True)
                print("Q %5d G %6d k %d: kernel %8.1f us (%.1f-%.1f)  torch %8.1f us (%.1f-%.1f)  floor %6.1f us (%s) share %.2f  values %s indices %s (%d rows)"
                      % (Q, G, k, med_k, min(t_k), max(t_k), med_t, min(t_t), max(t_t), fl, bound, fl / med_k, values_equal, indices_equal,
                         r["rows_compared"]), flush=True)
                del ws, idx, sc
    if args.log:
        print("| Q | G | k | kernel us (range) | torch us (range) | floor us | share of floor | values / indices equal |")
        print("|---|---|---|---|---|---|---|---|")
        for r in results:
            print("| %d | %d | %d | %.1f (%.1f-%.1f) | %.1f (%.1f-%.1f) | %.1f (%s) | %.2f | %s / %s |"
                  % (r["Q"], r["G"], r["k"], r["kernel_us"], *r["kernel_range"], r["torch_us"], *r["torch_range"], r["floor_us"], r["bound"],
                     r["share_of_floor"], r["values_equal"], r["indices_equal"]))
    print(json.dumps(dict(bench="similarity", reps=args.reps, steps=args.steps, cells=results)))


if __name__ == "__main__":
    main()
