"""The dense head's read-out against the two-pass route it exists to avoid, in one process.

  python tools/dense_bench.py [--reps 7] [--steps 20] [--batch 32] [--configs f32_os8,bf16_os16] [--no-torch]
      1.0x224, 1000 classes, fp32 and bf16, output stride 8 and 16. Per configuration, alternating within every repetition:
        kernel   mbn_upsample_argmax_f32 alone on the net's own dense logits (labels + scores), ms per call
        segment  all of mbn_net_segment (layers 1-27, the FC at every pixel, the read-out), ms per call
        torch    the yardstick, not the code under test: torch-ROCm on the SAME device buffer,
                 interpolate(mode="bilinear", align_corners=False).argmax(1): the upsampled [batch][1000][224][224] tensor is written
                 and read back (the route the fused kernel avoids), ms per call
      Each figure is the median over the repetitions of `steps` back-to-back calls between two stream marks (torch: two torch events
      on its own stream, synchronised). Then what the kernel's time means: the bytes it has to move (coarse logits in once, 4 bytes of
      label + 4 of score per pixel out) over 8 TB/s, and its VALU work (per pixel and class: 3 interpolants of 2 multiplies + 1 add
      shared as the kernel shares them, + compare and two selects) over the vector rate. The labels of the two routes are compared
      once (agreement, not timing). One JSON object at the end. No GPU: the Context raises; nothing falls back.

  python tools/dense_bench.py --any [--reps 7] [--steps 20] [--batch 32] [--torch-steps 2] [--no-torch]
      mbn_resample_argmax_f32, the read-out at any output size (main_any): against mbn_upsample_argmax_f32 at equal shapes, to 375 x 500
      against torch, and ragged.

  python tools/dense_bench.py --any --fit pad [--reps 7] [--steps 20] [--batch 32]
      mbn_resample_argmax_window_f32, the read-out through the letterbox (main_any_pad): against mbn_resample_argmax_f32 to the same 375 x 500,
      alternating in one process.

  python tools/dense_bench.py --any --prob [--reps 7] [--steps 20] [--batch 32] [--torch-steps 2] [--no-torch]
      mbn_resample_softmax_f32 / _window_f32 / _ragged_f32, the read-out with confidence (main_prob): each beside the argmax kernel of the same
      form on the same buffers, alternating in one process, and torch's three-pass interpolate(size=...).softmax(1).max(1).

  python tools/dense_bench.py --topk [--reps 7] [--steps 20] [--batch 32] [--torch-steps 2] [--no-torch]
      mbn_resample_topk_f32, the read-out with runners-up (main_topk): k = 1, 5, 8, with and without prob, on random logits and on the ascending
      ramp (the worst case), beside the softmax and argmax kernels on the same buffers and torch's interpolate(...).softmax(1).topk(k).

  python tools/dense_bench.py --ensemble 1,2,3,6 [--reps 7] [--steps 20] [--batch 32] [--torch-steps 1] [--no-torch]
      mbn_resample_ensemble_f32, the fused multi-view read-out (main_ensemble): per view count K against the unchanged window kernel on one view,
      against K launches of it, and against torch's sum of K interpolate(...) then argmax / softmax(1).max(1), argmax and --prob forms alike.

  python tools/dense_bench.py --score [--reps 7] [--steps 20] [--batch 32] [--no-torch]
      mbn_confusion_i32, the confusion matrix of --batch label maps of 375 x 500 against a uint8 truth (main_score): 21 / 150 / 1000 classes,
      random and piecewise-constant inputs, beside torch.bincount on the same buffers.

  python tools/dense_bench.py --slide [--reps 7] [--steps 20] [--batch 8] [--torch-images 2] [--no-torch]
      mbn_resample_slide_f32, the sliding-window read-out (main_slide): a 512 x 1024 source at tile 224 / stride 150 (3 x 7 tiles) against one
      launch of the plain kernel per tile and against torch's per-tile interpolate accumulated into [classes][H][W]; all of Net.segment_slide too.
      --batch counts source images: the net and the logits hold 21 tiles of each.

  python tools/dense_bench.py --regions [--reps 7] [--steps 20] [--batch 32] [--host-maps 2] [--no-host] [--configs random,blocks,constant]
      mbn_components_i32, the connected regions of --batch label maps of 375 x 500 (main_regions): 21 / 150 / 1000 classes, random, 25 x 25-block
      and constant inputs, connectivity 4 and 8, min_area 1 (comp alone) and 50 (comp and labels_out), beside scipy.ndimage.label per class on
      the host, download included.

  python tools/dense_bench.py --boundary [--reps 7] [--steps 20] [--batch 32] [--torch-steps 2] [--host-maps 2] [--no-torch] [--no-host]
                              [--configs random,blocks,constant]
      mbn_boundary_score_i32, the trimap and boundary-IoU tables of --batch label maps of 375 x 500 against a uint8 truth (main_boundary):
      21 / 150 / 1000 classes, random, 25 x 25-block and constant inputs, d = 12 (ratio 0.02) and d = 3, edge 0 and 1, beside mbn_confusion_i32
      on the same buffers, torch's one-hot / max_pool2d / bincount route and scipy.ndimage.binary_erosion per class on the host.

  python tools/dense_bench.py --panoptic [--reps 7] [--steps 20] [--batch 32] [--torch-steps 2] [--no-torch] [--no-host]
                              [--configs blocks,random,constant]
      mbn_panoptic_i32, the panoptic quality of --batch label maps of 375 x 500 against a truth (main_panoptic): 21 / 1000 classes, 25 x 25-block
      (the prediction shifted and with noise), random and constant inputs; the scoring call alone and the whole chain of two mbn_components_i32
      and the score, beside torch.unique of the (predicted, truth) pairs on the same buffers and numpy's after a download.

  python tools/dense_bench.py --surface [--reps 7] [--steps 20] [--batch 32] [--torch-steps 2] [--torch-images 2] [--host-maps 2] [--no-torch] [--no-host]
                              [--configs blocks,constant,random,far]
      mbn_surface_score_i32, the surface-distance table of --batch label maps of 375 x 500 against a uint8 truth (main_surface): 21 / 1000
      classes, 64 bins, shifted noisy 25 x 25 blocks, constant, random and far-apart inputs, beside torch.cdist between each class's contour
      coordinates on the same buffers and scipy.ndimage.distance_transform_edt per class on the host, download included; equal tables required.

  python tools/dense_bench.py --nll [--reps 7] [--steps 20] [--batch 32] [--torch-steps 2] [--no-torch]
      mbn_resample_nll_f32, the NLL / Brier read-out with a temperature grid (main_nll): --batch maps to 375 x 500 from the 28 x 28 and the
      14 x 14 map against a uint8 truth of 25 x 25 blocks, 21 and 1000 classes, 1, 4 and 8 temperatures, beside mbn_resample_argmax_f32 and
      mbn_resample_softmax_f32 on the same buffers and torch's interpolate -> log_softmax -> nll_loss plus the Brier expression at 1 and 8
      temperatures.
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

CLASSES, RES, ALPHA = 1000, 224, 1.0
CONFIGS = [("f32_os8", "f32", 8), ("f32_os16", "f32", 16), ("bf16_os8", "bf16", 8), ("bf16_os16", "bf16", 16)]
HBM_BYTES_PER_S = 8.0e12                    # spec
VALU_LANE_OPS_PER_S = 256 * 4 * 32 * 2.4e9  # CUs x SIMDs x lanes per clock x max clock: fp32 vector instructions (an FMA counts once here)


def kernel_work(batch, h, w, classes, S):
    """(bytes the read-out must move, vector lane-operations it issues) from the shapes"""
    pix = batch * h * S * w * S
    bytes_ = 4.0 * batch * h * w * classes + 8.0 * pix
    # per class: a lane forms t0, t1 (3 ops each) once for its 4 rows, then per row 3 ops of interpolation, 1 compare, 2 selects
    ops = pix * classes * (6.0 / 4 + 6.0)
    return bytes_, ops


def marks_ms(ctx, fn, steps):
    ctx.mark()
    for _ in range(steps):
        fn()
    ctx.mark()
    return sum(ctx.marks_read(4)) / steps


def resample_work(batch, h, w, classes, pix, three=True):
    """(bytes, vector lane-operations) of mbn_resample_argmax_f32 for `pix` output pixels in all. three: counted as if every wave took the loop
    with three horizontal interpolants per class and lane and two more selects per row (an upper count: a wave whose rows cross no coarse row
    takes kernel_work's loop, and at an integer factor every wave does: three=False)"""
    return 4.0 * batch * h * w * classes + 8.0 * pix, pix * classes * ((9.0 / 4 + 8.0) if three else (6.0 / 4 + 6.0))


def main_any(a):
    """--any: mbn_resample_argmax_f32, the read-out at any output size, on the maps of a 1.0x224 net (1000 classes, --batch images of random
    logits; the kernels' time does not depend on the values):
      factor   at out = S x coarse (28 x 28 x 8, 14 x 14 x 16, 7 x 7 x 32) against mbn_upsample_argmax_f32 on the same buffer, alternating
      source   to 375 x 500 from the 28 x 28 and the 14 x 14 map; the yardstick is torch-ROCm's interpolate(size=(375, 500)).argmax(1) on the
               same buffer (it writes and reads back batch x 1000 x 375 x 500 floats, in slices of 8 images because its kernel refuses
               outputs of 2^31 elements: --torch-steps passes per repetition)
      ragged   --batch images of 300-600 x 300-700 in one launch from the 14 x 14 map (no torch counterpart: torch is timed uniform only)"""
    pkg = import_package()
    torch = None
    if not a.no_torch:
        import torch
        assert torch.cuda.is_available(), "the yardstick needs torch on the same GPU"
    n, rng = a.batch, np.random.default_rng(0)
    sizes = [(int(rng.integers(300, 601)), int(rng.integers(300, 701))) for _ in range(n)]
    offs = np.concatenate([[0], np.cumsum([r * c for r, c in sizes])]).astype(np.int64)
    cap = max(int(offs[-1]), n * 375 * 500, n * RES * RES)
    result = {}
    with pkg.Context(0) as ctx:
        d_lab, d_sc = ctx.alloc(cap * 4), ctx.alloc(cap * 4)
        maps, runs = {}, []
        for hw_ in (28, 14, 7):
            x = (3.0 * rng.standard_normal((n, hw_, hw_, CLASSES))).astype(np.float32)
            if torch is not None:
                t = torch.from_numpy(x).cuda()
                maps[hw_] = (t.data_ptr(), t)
            else:
                b = ctx.to_device(x)
                maps[hw_] = (b.ptr, b)
        for hw_ in (28, 14, 7):
            S, p = RES // hw_, maps[hw_][0]
            runs.append(("factor_%dx%d_any" % (hw_, S), lambda p=p, hw_=hw_: ctx.resample_argmax(d_lab.ptr, d_sc.ptr, p, n, hw_, hw_, CLASSES, RES, RES),
                         resample_work(n, hw_, hw_, CLASSES, n * RES * RES, three=False)))
            runs.append(("factor_%dx%d_factor_kernel" % (hw_, S), lambda p=p, hw_=hw_, S=S: ctx.upsample_argmax(d_lab.ptr, d_sc.ptr, p, n, hw_, hw_, CLASSES, S),
                         kernel_work(n, hw_, hw_, CLASSES, S)))
        for hw_ in (28, 14):
            p = maps[hw_][0]
            runs.append(("source_375x500_from_%d" % hw_, lambda p=p, hw_=hw_: ctx.resample_argmax(d_lab.ptr, d_sc.ptr, p, n, hw_, hw_, CLASSES, 375, 500),
                         resample_work(n, hw_, hw_, CLASSES, n * 375 * 500)))
        rd = pkg.RaggedReadout(ctx, n)
        rd.set(14, 14, CLASSES, [(int(o), r, c) for o, (r, c) in zip(offs, sizes)])
        runs.append(("ragged_%d_images_from_14" % n, lambda: rd.run(d_lab.ptr, d_sc.ptr, maps[14][0]), resample_work(n, 14, 14, CLASSES, int(offs[-1]))))
        times = {name: [] for name, _, _ in runs}
        for _, fn, _ in runs:
            marks_ms(ctx, fn, 3)
        t_times = {28: [], 14: []}
        for _ in range(a.reps):
            for name, fn, _ in runs:
                times[name].append(marks_ms(ctx, fn, a.steps))
            for hw_ in (28, 14) if torch is not None else ():
                ctx.sync()
                nchw = maps[hw_][1].permute(0, 3, 1, 2)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

                def two_pass():     # torch's kernel takes outputs below 2^31 elements: 8 images of 1000 x 375 x 500 a call
                    for i in range(0, n, 8):
                        torch.nn.functional.interpolate(nchw[i:i + 8], size=(375, 500), mode="bilinear", align_corners=False).argmax(1)
                two_pass()
                e0.record()
                for _ in range(a.torch_steps):
                    two_pass()
                e1.record()
                torch.cuda.synchronize()
                t_times[hw_].append(e0.elapsed_time(e1) / a.torch_steps)
        for name, _, (bytes_, ops) in runs:
            k = statistics.median(times[name])
            result[name] = {"batch": n, "kernel_ms": round(k, 4), "kernel_runs_ms": [round(v, 4) for v in times[name]], "kernel_bytes": int(bytes_),
                            "kernel_frac_of_8TBps": round(bytes_ / HBM_BYTES_PER_S / (k / 1e3), 4),
                            "kernel_frac_of_valu_rate": round(ops / VALU_LANE_OPS_PER_S / (k / 1e3), 4)}
            print("%-32s %.4f ms  (%.1f %% of 8 TB/s, %.1f %% of the VALU rate)" % (name, k, 100 * result[name]["kernel_frac_of_8TBps"],
                                                                                     100 * result[name]["kernel_frac_of_valu_rate"]), flush=True)
        for hw_ in (28, 14, 7):
            S = RES // hw_
            result["factor_%dx%d_any_over_factor_kernel" % (hw_, S)] = round(
                result["factor_%dx%d_any" % (hw_, S)]["kernel_ms"] / result["factor_%dx%d_factor_kernel" % (hw_, S)]["kernel_ms"], 3)
        for hw_, ts in t_times.items():
            if ts:
                t = statistics.median(ts)
                result["source_375x500_from_%d" % hw_].update({"torch_ms": round(t, 4), "torch_runs_ms": [round(v, 4) for v in ts],
                                                               "torch_over_kernel": round(t / result["source_375x500_from_%d" % hw_]["kernel_ms"], 2)})
        result["ragged_pixels"] = int(offs[-1])
        rd.close()
    print(json.dumps(result))


def main_any_pad(a):
    """--any --fit pad: the window kernel against the plain one at equal output size, 375 x 500 from the 28 x 28 and the 14 x 14 map of a
    224 x 224 input (1000 classes, --batch images of random logits). Per map, alternating within every repetition:
      plain        mbn_resample_argmax_f32 (what a stretch fit reads out)
      window_full  mbn_resample_argmax_window_f32 with the whole input as the window: the plain kernel's results, footprint and LDS, so the
                   difference is the window rule's per-lane set-up alone
      window_pad   the same with mbn_fit_pad's rectangle of a 375 x 500 source: what segment_fit(FIT_PAD) launches; the larger ratio of the
                   letterbox shrinks the footprint (printed)
    Each figure is the median over the repetitions of `steps` back-to-back calls between two stream marks; the runs are kept, and the spread
    is (max - min) / median of a name's own repetitions."""
    pkg = import_package()
    n, rng = a.batch, np.random.default_rng(0)
    H, W = 375, 500
    rect = tuple(pkg.fit_pad(H, W, RES, RES))
    full = (0, 0, RES, RES)
    result = {"rect": list(rect), "batch": n}
    with pkg.Context(0) as ctx:
        d_lab, d_sc = ctx.alloc(n * H * W * 4), ctx.alloc(n * H * W * 4)
        runs, keep = [], []
        for hw_ in (28, 14):
            b = ctx.to_device((3.0 * rng.standard_normal((n, hw_, hw_, CLASSES))).astype(np.float32))
            keep.append(b)
            p = b.ptr
            work = resample_work(n, hw_, hw_, CLASSES, n * H * W)
            runs.append(("plain_from_%d" % hw_, lambda p=p, hw_=hw_: ctx.resample_argmax(d_lab.ptr, d_sc.ptr, p, n, hw_, hw_, CLASSES, H, W), work,
                         pkg.resample_plan(hw_, hw_, H, W)))
            for name, r in (("window_full", full), ("window_pad", rect)):
                runs.append(("%s_from_%d" % (name, hw_),
                             lambda p=p, hw_=hw_, r=r: ctx.resample_argmax_window(d_lab.ptr, d_sc.ptr, p, n, hw_, hw_, CLASSES, RES, RES, r, H, W), work,
                             pkg.resample_window_plan(hw_, hw_, RES, RES, r, H, W)))
        times = {name: [] for name, _, _, _ in runs}
        for _, fn, _, _ in runs:
            marks_ms(ctx, fn, 3)
        for _ in range(a.reps):
            for name, fn, _, _ in runs:
                times[name].append(marks_ms(ctx, fn, a.steps))
        for name, _, (bytes_, ops), l in runs:
            k = statistics.median(times[name])
            result[name] = {"kernel_ms": round(k, 4), "kernel_runs_ms": [round(v, 4) for v in times[name]],
                            "spread": round((max(times[name]) - min(times[name])) / k, 4), "footprint": [l.fy, l.fx], "lds_bytes": l.lds_bytes,
                            "kernel_frac_of_valu_rate": round(ops / VALU_LANE_OPS_PER_S / (k / 1e3), 4)}
            print("%-24s %.4f ms  spread %.1f %%  footprint %d x %d  (%.1f %% of the VALU rate)"
                  % (name, k, 100 * result[name]["spread"], l.fy, l.fx, 100 * result[name]["kernel_frac_of_valu_rate"]), flush=True)
        for hw_ in (28, 14):
            for name in ("window_full", "window_pad"):
                result["%s_over_plain_from_%d" % (name, hw_)] = round(result["%s_from_%d" % (name, hw_)]["kernel_ms"] /
                                                                      result["plain_from_%d" % hw_]["kernel_ms"], 4)
        for b in keep + [d_lab, d_sc]:
            b.free()
    print(json.dumps(result))


def prob_work(batch, h, w, classes, pix):
    """(bytes, vector issue slots) of the softmax read-out: resample_work's upper count, 4 more bytes per pixel for prob and, per pixel and
    class, subtract, max, multiply, add, one v_exp_f32 at two slots, and a quarter of the group's three maxima, subtract and compare"""
    bytes_, ops = resample_work(batch, h, w, classes, pix)
    return bytes_ + 4.0 * pix, ops + pix * classes * (6.0 + 5.0 / 4)


def main_prob(a):
    """--any --prob: the softmax read-out beside the argmax read-out, 1000 classes, --batch images of random logits (sigma 3), to 375 x 500 from
    the 28 x 28 and the 14 x 14 map of a 224 x 224 input. Per shape, alternating within every repetition, on the same buffers:
      plain        mbn_resample_argmax_f32 / mbn_resample_softmax_f32 (labels + score / labels + score + prob)
      window_pad   the _window_f32 pair with mbn_fit_pad's rectangle of a 375 x 500 source: what segment_fit / segment_prob_fit(FIT_PAD) launch
      ragged       the ragged pair, --batch images of 300-600 x 300-700 in one launch from the 14 x 14 map (main_any's sizes)
      torch        the yardstick: interpolate(size=(375, 500)).softmax(1).max(1) on the same buffer, three passes over batch x 1000 x 375 x 500
                   floats, in slices of 8 images (its interpolate refuses outputs of 2^31 elements; a slice's two tensors are 12 GB)
    Each figure is the median over the repetitions of `steps` back-to-back calls between two stream marks; the runs are kept, the spread is
    (max - min) / median of a name's own repetitions. The argmax kernel is unchanged code: its times here belong beside main_any's."""
    pkg = import_package()
    torch = None
    if not a.no_torch:
        import torch
        assert torch.cuda.is_available(), "the yardstick needs torch on the same GPU"
    n, rng = a.batch, np.random.default_rng(0)
    H, W = 375, 500
    sizes = [(int(rng.integers(300, 601)), int(rng.integers(300, 701))) for _ in range(n)]
    offs = np.concatenate([[0], np.cumsum([r * c for r, c in sizes])]).astype(np.int64)
    cap = max(int(offs[-1]), n * H * W)
    rect = tuple(pkg.fit_pad(H, W, RES, RES))
    result = {"batch": n, "rect": list(rect), "ragged_pixels": int(offs[-1])}
    with pkg.Context(0) as ctx:
        d_lab, d_sc, d_pr = ctx.alloc(cap * 4), ctx.alloc(cap * 4), ctx.alloc(cap * 4)
        maps, runs = {}, []
        for hw_ in (28, 14):
            x = (3.0 * rng.standard_normal((n, hw_, hw_, CLASSES))).astype(np.float32)
            if torch is not None:
                t = torch.from_numpy(x).cuda()
                maps[hw_] = (t.data_ptr(), t)
            else:
                b = ctx.to_device(x)
                maps[hw_] = (b.ptr, b)
        for hw_ in (28, 14):
            p = maps[hw_][0]
            runs.append(("plain_from_%d" % hw_, lambda p=p, hw_=hw_: ctx.resample_argmax(d_lab.ptr, d_sc.ptr, p, n, hw_, hw_, CLASSES, H, W),
                         lambda p=p, hw_=hw_: ctx.resample_softmax(d_lab.ptr, d_pr.ptr, d_sc.ptr, p, n, hw_, hw_, CLASSES, H, W), (n, hw_, n * H * W)))
            runs.append(("window_pad_from_%d" % hw_,
                         lambda p=p, hw_=hw_: ctx.resample_argmax_window(d_lab.ptr, d_sc.ptr, p, n, hw_, hw_, CLASSES, RES, RES, rect, H, W),
                         lambda p=p, hw_=hw_: ctx.resample_softmax_window(d_lab.ptr, d_pr.ptr, d_sc.ptr, p, n, hw_, hw_, CLASSES, RES, RES, rect, H, W),
                         (n, hw_, n * H * W)))
        rd = pkg.RaggedReadout(ctx, n)
        rd.set(14, 14, CLASSES, [(int(o), r, c) for o, (r, c) in zip(offs, sizes)])
        runs.append(("ragged_from_14", lambda: rd.run(d_lab.ptr, d_sc.ptr, maps[14][0]),
                     lambda: rd.run_softmax(d_lab.ptr, d_pr.ptr, d_sc.ptr, maps[14][0]), (n, 14, int(offs[-1]))))
        times = {(name, k): [] for name, _, _, _ in runs for k in ("argmax", "softmax")}
        for _, f_arg, f_soft, _ in runs:
            marks_ms(ctx, f_arg, 3)
            marks_ms(ctx, f_soft, 3)
        t_times = {28: [], 14: []}
        for _ in range(a.reps):
            for name, f_arg, f_soft, _ in runs:
                times[(name, "argmax")].append(marks_ms(ctx, f_arg, a.steps))
                times[(name, "softmax")].append(marks_ms(ctx, f_soft, a.steps))
            for hw_ in (28, 14) if torch is not None else ():
                ctx.sync()
                nchw = maps[hw_][1].permute(0, 3, 1, 2)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

                def three_pass():
                    for i in range(0, n, 8):
                        torch.nn.functional.interpolate(nchw[i:i + 8], size=(H, W), mode="bilinear", align_corners=False).softmax(1).max(1)
                three_pass()
                e0.record()
                for _ in range(a.torch_steps):
                    three_pass()
                e1.record()
                torch.cuda.synchronize()
                t_times[hw_].append(e0.elapsed_time(e1) / a.torch_steps)
        for name, _, _, (nb, hw_, pix) in runs:
            out = {}
            for k, work in (("argmax", resample_work(nb, hw_, hw_, CLASSES, pix)), ("softmax", prob_work(nb, hw_, hw_, CLASSES, pix))):
                ts = times[(name, k)]
                m = statistics.median(ts)
                out[k] = {"kernel_ms": round(m, 4), "kernel_runs_ms": [round(v, 4) for v in ts], "spread": round((max(ts) - min(ts)) / m, 4),
                          "kernel_frac_of_8TBps": round(work[0] / HBM_BYTES_PER_S / (m / 1e3), 4),
                          "kernel_frac_of_valu_rate": round(work[1] / VALU_LANE_OPS_PER_S / (m / 1e3), 4)}
            out["softmax_over_argmax"] = round(out["softmax"]["kernel_ms"] / out["argmax"]["kernel_ms"], 3)
            result[name] = out
            print("%-20s argmax %.4f ms (spread %.1f %%)  softmax %.4f ms (spread %.1f %%, %.1f %% of the VALU rate)  ratio %.3f"
                  % (name, out["argmax"]["kernel_ms"], 100 * out["argmax"]["spread"], out["softmax"]["kernel_ms"], 100 * out["softmax"]["spread"],
                     100 * out["softmax"]["kernel_frac_of_valu_rate"], out["softmax_over_argmax"]), flush=True)
        for hw_, ts in t_times.items():
            if ts:
                t = statistics.median(ts)
                result["plain_from_%d" % hw_].update({"torch_ms": round(t, 4), "torch_runs_ms": [round(v, 4) for v in ts],
                                                      "torch_over_softmax": round(t / result["plain_from_%d" % hw_]["softmax"]["kernel_ms"], 2)})
                print("torch three-pass from %d: %.2f ms" % (hw_, t), flush=True)
        rd.close()
    print(json.dumps(result))


def nll_work(batch, h, w, classes, pix, temps):
    """(bytes, vector issue slots) of the NLL read-out: two passes of resample_work's upper count of lerps (the second without the compare's two
    selects but with the truth's compare and select and the subtract and max of d), and per temperature a multiply, one v_exp_f32 at two slots,
    an add, a multiply and an add; 8 bytes of maps per pixel and temperature and the truth's byte"""
    bytes_, ops = resample_work(batch, h, w, classes, pix)
    return bytes_ - 8.0 * pix + pix * (1.0 + 8.0 * temps), 2 * ops + pix * classes * (2.0 + 6.0 * temps)


def main_nll(a):
    """--nll: the NLL / Brier read-out, --batch images of random logits (sigma 3) to 375 x 500 from the 28 x 28 and the 14 x 14 map, 21 and 1000
    classes, against a uint8 truth of 25 x 25 blocks. Per shape, alternating within every repetition, on the same buffers:
      argmax, softmax   mbn_resample_argmax_f32 (labels + score) and mbn_resample_softmax_f32 (labels + score + prob): the two kernels whose sum
                        the NLL call at one temperature is expected to cost
      nll_1, _4, _8     mbn_resample_nll_f32 with both maps and the table at 1, 4 and 8 temperatures (the three capacities)
      torch_1, _8       the yardstick: interpolate(size=(375, 500)) -> log_softmax(beta v) -> nll_loss, and the Brier expression
                        1 - 2 p_t + sum p^2, per temperature, on the same buffers, in slices of 8 images
    Each figure is the median over the repetitions of `steps` back-to-back calls between two stream marks, with the range of the rounds."""
    pkg = import_package()
    torch = None
    if not a.no_torch:
        import torch
        assert torch.cuda.is_available(), "the yardstick needs torch on the same GPU"
    n, rng = a.batch, np.random.default_rng(0)
    H, W = 375, 500
    grid = [0.25, 0.35, 0.5, 0.7, 1.0, 1.4, 2.0, 4.0]
    betas = {1: [1.0], 4: grid[2:6], 8: grid}
    result = {"batch": n}
    with pkg.Context(0) as ctx:
        d_lab, d_sc, d_pr = ctx.alloc(n * H * W * 4), ctx.alloc(n * H * W * 4), ctx.alloc(n * H * W * 4)
        d_nll, d_brier = ctx.alloc(8 * n * H * W * 4), ctx.alloc(8 * n * H * W * 4)
        for classes in (21, 1000):
            blocks = rng.integers(0, min(classes, 255), (n, (H + 24) // 25, (W + 24) // 25)).astype(np.uint8)
            truth = np.ascontiguousarray(np.repeat(np.repeat(blocks, 25, axis=1), 25, axis=2)[:, :H, :W])
            d_tab = ctx.to_device(np.zeros(8 * (classes + 1) * 4, np.uint64))
            if torch is not None:
                t_truth = torch.from_numpy(truth).cuda()
                truth_ptr = t_truth.data_ptr()
            else:
                d_truth = ctx.to_device(truth)
                truth_ptr = d_truth.ptr
            for hw_ in (28, 14):
                x = (3.0 * rng.standard_normal((n, hw_, hw_, classes))).astype(np.float32)
                if torch is not None:
                    t = torch.from_numpy(x).cuda()
                    p, keep = t.data_ptr(), t
                else:
                    keep = ctx.to_device(x)
                    p = keep.ptr
                runs = {"argmax": lambda: ctx.resample_argmax(d_lab.ptr, d_sc.ptr, p, n, hw_, hw_, classes, H, W),
                        "softmax": lambda: ctx.resample_softmax(d_lab.ptr, d_pr.ptr, d_sc.ptr, p, n, hw_, hw_, classes, H, W)}
                for temps, b in betas.items():
                    runs["nll_%d" % temps] = lambda b=b: ctx.resample_nll(d_tab.ptr, d_nll.ptr, d_brier.ptr, p, truth_ptr, 1, n, hw_, hw_, classes, H, W, b)
                times = {k: [] for k in runs}
                t_times = {1: [], 8: []}
                for f in runs.values():
                    marks_ms(ctx, f, 3)
                for _ in range(a.reps):
                    for k, f in runs.items():
                        times[k].append(marks_ms(ctx, f, a.steps))
                    for temps in (1, 8) if torch is not None else ():
                        ctx.sync()
                        nchw = keep.permute(0, 3, 1, 2)
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

                        def route(temps=temps):
                            for i in range(0, n, 8):
                                v = torch.nn.functional.interpolate(nchw[i:i + 8], size=(H, W), mode="bilinear", align_corners=False)
                                tt = t_truth[i:i + 8].long()
                                for beta in betas[temps]:
                                    logp = torch.log_softmax(v * beta, dim=1)
                                    nll = torch.nn.functional.nll_loss(logp, tt, reduction="none")
                                    brier = 1.0 - 2.0 * torch.exp(-nll) + torch.exp(2.0 * logp).sum(1)
                                    del logp, nll, brier
                        route()
                        e0.record()
                        for _ in range(a.torch_steps):
                            route()
                        e1.record()
                        torch.cuda.synchronize()
                        t_times[temps].append(e0.elapsed_time(e1) / a.torch_steps)
                out = {}
                for k, ts in times.items():
                    m = statistics.median(ts)
                    out[k] = {"kernel_ms": round(m, 4), "kernel_runs_ms": [round(v, 4) for v in ts], "range_ms": [round(min(ts), 4), round(max(ts), 4)]}
                    if k.startswith("nll_"):
                        work = nll_work(n, hw_, hw_, classes, n * H * W, int(k[4:]))
                        out[k].update({"kernel_frac_of_8TBps": round(work[0] / HBM_BYTES_PER_S / (m / 1e3), 4),
                                       "kernel_frac_of_valu_rate": round(work[1] / VALU_LANE_OPS_PER_S / (m / 1e3), 4)})
                out["nll_1_over_argmax_plus_softmax"] = round(out["nll_1"]["kernel_ms"] / (out["argmax"]["kernel_ms"] + out["softmax"]["kernel_ms"]), 3)
                out["ms_per_further_temperature"] = round((out["nll_8"]["kernel_ms"] - out["nll_1"]["kernel_ms"]) / 7, 4)
                for temps, ts in t_times.items():
                    if ts:
                        m = statistics.median(ts)
                        out["torch_%d" % temps] = {"ms": round(m, 4), "runs_ms": [round(v, 4) for v in ts],
                                                   "over_nll": round(m / out["nll_%d" % temps]["kernel_ms"], 2)}
                name = "classes_%d_from_%d" % (classes, hw_)
                result[name] = out
                print("%-22s argmax %.4f  softmax %.4f  nll_1 %.4f  nll_4 %.4f  nll_8 %.4f ms  (nll_1 / (argmax + softmax) %.3f, %.4f ms a further "
                      "temperature)%s" % (name, out["argmax"]["kernel_ms"], out["softmax"]["kernel_ms"], out["nll_1"]["kernel_ms"], out["nll_4"]["kernel_ms"],
                                          out["nll_8"]["kernel_ms"], out["nll_1_over_argmax_plus_softmax"], out["ms_per_further_temperature"],
                                          "".join("  torch_%d %.2f ms" % (k, out["torch_%d" % k]["ms"]) for k in (1, 8) if "torch_%d" % k in out)), flush=True)
                del keep
    print(json.dumps(result))


def main_topk(a):
    """--topk: the top-k read-out beside the softmax and argmax read-outs, 1000 classes, --batch images, to 375 x 500 from the 28 x 28 and the 14 x 14
    map of a 224 x 224 input. Two kinds of logits: random (sigma 3; an insertion is rare) and the ascending ramp c / 4 over the classes with a
    little noise on it (nearly every class is a new maximum, so nearly every class is inserted at rank 0: the worst case). Per shape and kind,
    alternating within every repetition, on the same buffers:
      softmax, argmax   mbn_resample_softmax_f32 / mbn_resample_argmax_f32: at k = 1 the same arithmetic
      topk k prob       mbn_resample_topk_f32 with labels, score and prob, k = 1, 5, 8 (capacity 4, 8, 8)
      topk k logit      the same without prob: no exponential
      torch             the yardstick, random logits only: interpolate(size=(375, 500)).softmax(1).topk(k) on the same buffer, in slices of 8 images
    Each figure is the median over the repetitions of `steps` back-to-back calls between two stream marks; the spread is (max - min) / median of a
    name's own repetitions."""
    pkg = import_package()
    torch = None
    if not a.no_torch:
        import torch
        assert torch.cuda.is_available(), "the yardstick needs torch on the same GPU"
    n, rng = a.batch, np.random.default_rng(0)
    H, W, KS = 375, 500, (1, 5, 8)
    result = {"batch": n, "ks": list(KS)}
    with pkg.Context(0) as ctx:
        npix = n * H * W
        d_lab, d_sc, d_pr = ctx.alloc(8 * npix * 4), ctx.alloc(8 * npix * 4), ctx.alloc(8 * npix * 4)
        for hw_ in (28, 14):
            for kind in ("random", "ramp"):
                if kind == "random":
                    x = (3.0 * rng.standard_normal((n, hw_, hw_, CLASSES))).astype(np.float32)
                else:
                    x = (0.25 * np.arange(CLASSES, dtype=np.float32) + 0.01 * rng.standard_normal((n, hw_, hw_, CLASSES))).astype(np.float32)
                if torch is not None:
                    t = torch.from_numpy(x).cuda()
                    p, keep = t.data_ptr(), t
                else:
                    keep = ctx.to_device(x)
                    p = keep.ptr
                runs = [("softmax", lambda: ctx.resample_softmax(d_lab.ptr, d_pr.ptr, d_sc.ptr, p, n, hw_, hw_, CLASSES, H, W)),
                        ("argmax", lambda: ctx.resample_argmax(d_lab.ptr, d_sc.ptr, p, n, hw_, hw_, CLASSES, H, W))]
                for k in KS:
                    runs.append(("topk%d_prob" % k, lambda k=k: ctx.resample_topk(d_lab.ptr, d_pr.ptr, d_sc.ptr, p, n, hw_, hw_, CLASSES, H, W, k)))
                    runs.append(("topk%d_logit" % k, lambda k=k: ctx.resample_topk(d_lab.ptr, None, d_sc.ptr, p, n, hw_, hw_, CLASSES, H, W, k)))
                times = {name: [] for name, _ in runs}
                t_times = {k: [] for k in KS}
                for _, f in runs:
                    marks_ms(ctx, f, 2)
                for _ in range(a.reps):
                    for name, f in runs:
                        times[name].append(marks_ms(ctx, f, a.steps))
                    for k in KS if torch is not None and kind == "random" else ():
                        ctx.sync()
                        nchw = keep.permute(0, 3, 1, 2)
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

                        def passes():
                            for i in range(0, n, 8):
                                torch.nn.functional.interpolate(nchw[i:i + 8], size=(H, W), mode="bilinear", align_corners=False).softmax(1).topk(k, dim=1)
                        passes()
                        e0.record()
                        for _ in range(a.torch_steps):
                            passes()
                        e1.record()
                        torch.cuda.synchronize()
                        t_times[k].append(e0.elapsed_time(e1) / a.torch_steps)
                out = {}
                for name, _ in runs:
                    ts = times[name]
                    m = statistics.median(ts)
                    out[name] = {"kernel_ms": round(m, 4), "kernel_runs_ms": [round(v, 4) for v in ts], "spread": round((max(ts) - min(ts)) / m, 4)}
                for k in KS:
                    out["topk%d_prob" % k]["over_softmax"] = round(out["topk%d_prob" % k]["kernel_ms"] / out["softmax"]["kernel_ms"], 3)
                    out["topk%d_logit" % k]["over_argmax"] = round(out["topk%d_logit" % k]["kernel_ms"] / out["argmax"]["kernel_ms"], 3)
                    if t_times[k]:
                        t = statistics.median(t_times[k])
                        out["torch_topk%d" % k] = {"torch_ms": round(t, 4), "torch_runs_ms": [round(v, 4) for v in t_times[k]],
                                                   "torch_over_topk_prob": round(t / out["topk%d_prob" % k]["kernel_ms"], 2)}
                result["%s_from_%d" % (kind, hw_)] = out
                print("%s from %d: softmax %.4f ms (spread %.1f %%), argmax %.4f ms (spread %.1f %%)"
                      % (kind, hw_, out["softmax"]["kernel_ms"], 100 * out["softmax"]["spread"], out["argmax"]["kernel_ms"], 100 * out["argmax"]["spread"]))
                for k in KS:
                    pr_, lg = out["topk%d_prob" % k], out["topk%d_logit" % k]
                    print("    k %d: prob %.4f ms (spread %.1f %%, %.3f x softmax)  logit %.4f ms (spread %.1f %%, %.3f x argmax)%s"
                          % (k, pr_["kernel_ms"], 100 * pr_["spread"], pr_["over_softmax"], lg["kernel_ms"], 100 * lg["spread"], lg["over_argmax"],
                             "  torch %.2f ms" % out["torch_topk%d" % k]["torch_ms"] if "torch_topk%d" % k in out else ""), flush=True)
                if torch is None:
                    keep.free()
                del keep
    print(json.dumps(result))


TTA_VIEWS = [(1.0, 0), (1.0, 1), (0.75, 0), (0.75, 1), (0.5, 0), (0.5, 1), (0.875, 0), (0.875, 1)]      # (scale, mirror): the first K are timed


def main_ensemble(a):
    """--ensemble K[,K...]: the README's read-out shapes (1000 classes, to 375 x 500 from the 28 x 28 and the 14 x 14 map of a 224 x 224 input,
    through the letterbox, --batch output images of random logits, sigma 3), K views = the first K of TTA_VIEWS through mbn_fit_view, the logits
    view-major. Per map and K, alternating within every repetition, argmax form and prob form (labels + score / labels + score + prob):
      window     (a) the unchanged window kernel on view 0 alone: mbn_resample_argmax_window_f32 / _softmax_window_f32
      k_windows  (b) K launches of it, view k's rectangle over view k's logits (the yardstick: the ensemble forms K times its interpolants)
      ensemble   mbn_resample_ensemble_f32 over the K views, ONE launch
      torch      (c) on the same buffers: sum_k interpolate(view k, size=(375, 500)) then argmax(1) / softmax(1).max(1), in slices of 8 images
                 (its interpolate refuses outputs of 2^31 elements), in the first three repetitions only: a pass at K = 6 takes about a second
    Each figure is the median over the repetitions of `steps` back-to-back calls between two stream marks; the runs are kept, the spread is
    (max - min) / median of a name's own repetitions. ensemble_over_k_windows is the figure the issue asks for: at or under 1 plus the spread."""
    pkg = import_package()
    torch = None
    if not a.no_torch:
        import torch
        assert torch.cuda.is_available(), "the yardstick needs torch on the same GPU"
    ks = sorted({int(k) for k in a.ensemble.split(",")})
    assert ks and 1 <= ks[0] and ks[-1] <= len(TTA_VIEWS)
    n, rng, H, W = a.batch, np.random.default_rng(0), 375, 500
    views = [pkg.fit_view(H, W, RES, RES, s, m) for s, m in TTA_VIEWS[:ks[-1]]]
    result = {"batch": n, "views": [list(v.rect) + [v.mirror] for v in views]}
    with pkg.Context(0) as ctx:
        d_lab, d_sc, d_pr = ctx.alloc(n * H * W * 4), ctx.alloc(n * H * W * 4), ctx.alloc(n * H * W * 4)
        for hw_ in (28, 14):
            x = (3.0 * rng.standard_normal((ks[-1], n, hw_, hw_, CLASSES))).astype(np.float32)
            if torch is not None:
                t = torch.from_numpy(x).cuda()
                p = t.data_ptr()
            else:
                t = ctx.to_device(x)
                p = t.ptr
            stride = n * hw_ * hw_ * CLASSES * 4
            runs = []

            def window(k, prob, p=p, hw_=hw_, stride=stride):
                if prob:
                    ctx.resample_softmax_window(d_lab.ptr, d_pr.ptr, d_sc.ptr, p + k * stride, n, hw_, hw_, CLASSES, RES, RES, views[k].rect, H, W)
                else:
                    ctx.resample_argmax_window(d_lab.ptr, d_sc.ptr, p + k * stride, n, hw_, hw_, CLASSES, RES, RES, views[k].rect, H, W)

            for prob in (False, True):
                form = "prob" if prob else "argmax"
                runs.append(("window_%s" % form, lambda prob=prob: window(0, prob)))
                for K in ks:
                    runs.append(("k_windows_%s_K%d" % (form, K), lambda prob=prob, K=K: [window(k, prob) for k in range(K)]))
                    runs.append(("ensemble_%s_K%d" % (form, K),
                                 lambda prob=prob, K=K, p=p, hw_=hw_: ctx.resample_ensemble(d_lab.ptr, d_pr.ptr if prob else None, d_sc.ptr, p, n, hw_, hw_,
                                                                                            CLASSES, RES, RES, views[:K], H, W)))
            times = {name: [] for name, _ in runs}
            t_times = {(form, K): [] for form in ("argmax", "prob") for K in ks}
            for _, fn in runs:
                marks_ms(ctx, fn, 2)
            for rep in range(a.reps):
                for name, fn in runs:
                    times[name].append(marks_ms(ctx, fn, a.steps))
                if torch is None or rep >= 3:
                    continue
                ctx.sync()
                nchw = t.permute(0, 1, 4, 2, 3)
                for form in ("argmax", "prob"):
                    for K in ks:
                        def passes():
                            for i in range(0, n, 8):
                                acc = torch.nn.functional.interpolate(nchw[0, i:i + 8], size=(H, W), mode="bilinear", align_corners=False)
                                for k in range(1, K):
                                    acc += torch.nn.functional.interpolate(nchw[k, i:i + 8], size=(H, W), mode="bilinear", align_corners=False)
                                if form == "prob":
                                    acc.softmax(1).max(1)
                                else:
                                    acc.argmax(1)
                        if rep == 0:
                            passes()
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        for _ in range(a.torch_steps):
                            passes()
                        e1.record()
                        torch.cuda.synchronize()
                        t_times[(form, K)].append(e0.elapsed_time(e1) / a.torch_steps)
            out = {}
            for name, _ in runs:
                m = statistics.median(times[name])
                out[name] = {"kernel_ms": round(m, 4), "kernel_runs_ms": [round(v, 4) for v in times[name]],
                             "spread": round((max(times[name]) - min(times[name])) / m, 4)}
            for form in ("argmax", "prob"):
                one = out["window_%s" % form]["kernel_ms"]
                for K in ks:
                    l = pkg.resample_ensemble_plan(hw_, hw_, RES, RES, views[:K], H, W)
                    e, kw = out["ensemble_%s_K%d" % (form, K)], out["k_windows_%s_K%d" % (form, K)]
                    e.update({"footprint": [l.fy, l.fx], "chunk": l.ch, "lds_bytes": l.lds_bytes, "over_k_windows": round(e["kernel_ms"] / kw["kernel_ms"], 3),
                              "over_k_times_window": round(e["kernel_ms"] / (K * one), 3)})
                    ts = t_times[(form, K)]
                    if ts:
                        tm = statistics.median(ts)
                        e.update({"torch_ms": round(tm, 3), "torch_runs_ms": [round(v, 3) for v in ts], "torch_over_ensemble": round(tm / e["kernel_ms"], 1)})
                    print("from %d %-6s K %d: window %.4f  K windows %.4f (spread %.1f %%)  ensemble %.4f ms (spread %.1f %%, chunk %d, %d B LDS)  "
                          "ensemble / K windows %.3f  torch %s ms" % (hw_, form, K, one, kw["kernel_ms"], 100 * kw["spread"], e["kernel_ms"],
                                                                      100 * e["spread"], l.ch, l.lds_bytes, e["over_k_windows"],
                                                                      ("%.1f" % e["torch_ms"]) if ts else "-"), flush=True)
            result["from_%d" % hw_] = out
            if torch is not None:
                del t
                torch.cuda.empty_cache()
            else:
                t.free()
    print(json.dumps(result))


def main_slide(a):
    """--slide: mbn_resample_slide_f32, the sliding-window read-out (1000 classes, the 28 x 28 and the 14 x 14 map of a 224 x 224 input, a 512 x 1024
    source at tile 224 / stride 150: 3 x 7 tiles, --batch source images of random logits, sigma 3, image-major). Per map, alternating within every
    repetition, argmax form and prob form (labels + score / labels + score + prob):
      tile       the unchanged plain kernel on one tile: mbn_resample_argmax_f32 / _softmax_f32 of --batch maps to 224 x 224
      per_tile   ny * nx launches of it, one per tile (the yardstick: they form the same interpolants but cannot combine them)
      slide      mbn_resample_slide_f32 over the grid, ONE launch
      torch      on the same buffer, per source image: per tile interpolate(size=(224, 224)) added into [1][classes][512][1024], divided by the
                 count map, then argmax(1) / softmax(1).max(1); --torch-images images only (2 GB an image), in the first three repetitions,
                 scaled to the batch
    and segment_slide: all of Net.segment_slide (resize_tiles, forward_dense of batch * 21 tiles, the read-out) on an f32 net of that output stride.
    Each figure is the median over the repetitions of `steps` back-to-back calls between two stream marks; the runs are kept, the spread is
    (max - min) / median of a name's own repetitions. occupancy: active lanes / launched lanes of the slide launch, overall and of its worst cell."""
    pkg = import_package()
    torch = None
    if not a.no_torch:
        import torch
        assert torch.cuda.is_available(), "the yardstick needs torch on the same GPU"
    n, rng, H, W, TILE, STRIDE = a.batch, np.random.default_rng(0), 512, 1024, RES, 150
    plan = pkg.slide_plan(H, W, TILE, TILE, STRIDE, STRIDE)
    ys, xs, T = plan.ys, plan.xs, plan.ny * plan.nx

    def cells(pos):
        e = sorted(set(pos) | {v + TILE for v in pos})
        return [b - c for c, b in zip(e, e[1:])]

    def lanes(sizes):                           # (active, launched) outputs of an axis' pieces
        return sum(sizes), sum(32 * -(-s // 32) for s in sizes)

    (ay, ly), (ax, lx) = lanes(cells(ys)), lanes(cells(xs))
    worst = min((hc * wc) / (32 * -(-hc // 32) * 32 * -(-wc // 32)) for hc in cells(ys) for wc in cells(xs))
    result = {"batch": n, "source": [H, W], "tile": TILE, "stride": STRIDE, "ys": ys, "xs": xs, "cells": [cells(ys), cells(xs)],
              "occupancy": round(ay * ax / (ly * lx), 4), "occupancy_worst_cell": round(worst, 4)}
    with tempfile.TemporaryDirectory() as d, pkg.Context(0) as ctx:
        path = os.path.join(d, "w.h5")
        pkg.synthetic_h5(path, alpha=ALPHA, classes=CLASSES, seed=7)
        src = rng.integers(0, 256, (n, H, W, 3), dtype=np.uint8)
        d_src = ctx.to_device(src)
        d_lab, d_sc, d_pr = ctx.alloc(n * H * W * 4), ctx.alloc(n * H * W * 4), ctx.alloc(n * H * W * 4)
        for hw_ in (28, 14):
            x = (3.0 * rng.standard_normal((n, T, hw_, hw_, CLASSES))).astype(np.float32)
            if torch is not None:
                t = torch.from_numpy(x).cuda()
                p = t.data_ptr()
            else:
                t = ctx.to_device(x)
                p = t.ptr
            del x
            stride = n * hw_ * hw_ * CLASSES * 4           # a per-tile launch reads --batch consecutive maps: the same bytes, whichever tile's

            def tile(k, prob, p=p, hw_=hw_, stride=stride):
                if prob:
                    ctx.resample_softmax(d_lab.ptr, d_pr.ptr, d_sc.ptr, p + k * stride, n, hw_, hw_, CLASSES, TILE, TILE)
                else:
                    ctx.resample_argmax(d_lab.ptr, d_sc.ptr, p + k * stride, n, hw_, hw_, CLASSES, TILE, TILE)

            hw = pkg.HostWeights(path, res=RES, output_stride=RES // hw_)
            net = pkg.Net(ctx, hw.plan, hw.blob.copy(), n * T)
            net.set_input_u8(True)
            runs = []
            for prob in (False, True):
                form = "prob" if prob else "argmax"
                runs.append(("tile_%s" % form, lambda prob=prob: tile(0, prob)))
                runs.append(("per_tile_%s" % form, lambda prob=prob: [tile(k, prob) for k in range(T)]))
                runs.append(("slide_%s" % form, lambda prob=prob, p=p, hw_=hw_: ctx.resample_slide(d_lab.ptr, d_pr.ptr if prob else None, d_sc.ptr, p, n, hw_,
                                                                                                  hw_, CLASSES, plan, H, W)))
                runs.append(("segment_slide_%s" % form, lambda prob=prob: net.segment_slide(d_src.ptr, n, H, W, (TILE, TILE), (STRIDE, STRIDE), d_lab.ptr,
                                                                                            d_pr.ptr if prob else None, d_sc.ptr)))
            times = {name: [] for name, _ in runs}
            t_times = {"argmax": [], "prob": []}
            for _, fn in runs:
                marks_ms(ctx, fn, 2)
            for rep in range(a.reps):
                for name, fn in runs:
                    times[name].append(marks_ms(ctx, fn, a.steps if not name.startswith("segment") else max(1, a.steps // 4)))
                if torch is None or rep >= 3:
                    continue
                ctx.sync()
                nchw = t.permute(0, 1, 4, 2, 3)
                count = torch.zeros((H, W), device="cuda")
                for y in ys:
                    for x0 in xs:
                        count[y:y + TILE, x0:x0 + TILE] += 1
                images = min(n, a.torch_images)
                for form in ("argmax", "prob"):
                    def passes():
                        for b in range(images):
                            acc = torch.zeros((1, CLASSES, H, W), device="cuda")
                            for iy, y in enumerate(ys):
                                for ix, x0 in enumerate(xs):
                                    acc[:, :, y:y + TILE, x0:x0 + TILE] += torch.nn.functional.interpolate(
                                        nchw[b, iy * len(xs) + ix][None], size=(TILE, TILE), mode="bilinear", align_corners=False)
                            acc /= count
                            if form == "prob":
                                acc.softmax(1).max(1)
                            else:
                                acc.argmax(1)
                            del acc
                    if rep == 0:
                        passes()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    passes()
                    e1.record()
                    torch.cuda.synchronize()
                    t_times[form].append(e0.elapsed_time(e1) * n / images)
            out = {}
            for name, _ in runs:
                m = statistics.median(times[name])
                out[name] = {"kernel_ms": round(m, 4), "kernel_runs_ms": [round(v, 4) for v in times[name]],
                             "spread": round((max(times[name]) - min(times[name])) / m, 4)}
            l = pkg.resample_slide_plan(hw_, hw_, plan, H, W)
            for form in ("argmax", "prob"):
                s, pt = out["slide_%s" % form], out["per_tile_%s" % form]
                s.update({"footprint": [l.fy, l.fx], "chunk": l.ch, "lds_bytes": l.lds_bytes, "workgroups": l.tiles,
                          "over_per_tile": round(s["kernel_ms"] / pt["kernel_ms"], 3)})
                ts = t_times[form]
                if ts:
                    tm = statistics.median(ts)
                    s.update({"torch_ms": round(tm, 2), "torch_runs_ms": [round(v, 2) for v in ts], "torch_over_slide": round(tm / s["kernel_ms"], 1)})
                print("from %d %-6s: tile %.4f  %d tiles %.4f (spread %.1f %%)  slide %.4f ms (spread %.1f %%, chunk %d, %d B LDS, %d workgroups)  "
                      "slide / per tile %.3f  segment_slide %.3f ms  torch %s ms" % (
                          hw_, form, out["tile_%s" % form]["kernel_ms"], T, pt["kernel_ms"], 100 * pt["spread"], s["kernel_ms"], 100 * s["spread"], l.ch,
                          l.lds_bytes, l.tiles, s["over_per_tile"], out["segment_slide_%s" % form]["kernel_ms"], ("%.1f" % s["torch_ms"]) if ts else "-"),
                      flush=True)
            result["from_%d" % hw_] = out
            net.destroy()
            hw.free()
            if torch is not None:
                del t
                torch.cuda.empty_cache()
            else:
                t.free()
    print(json.dumps(result))


def main_score(a):
    """--score: mbn_confusion_i32 on --batch maps of 375 x 500 (6 M pixels at 32), int32 labels against uint8 truth, at 21 / 150 / 1000 classes
    (the LDS form with two workgroups a CU, the LDS form at its largest table, the global form). Three inputs per class count:
      random     labels and truth uniform over the classes (the truth over min(classes, 256)): no two neighbours agree, every add is its own
      blocks     piecewise constant: blocks of 25 x 25 pixels of one class, the prediction = the truth shifted by one pixel along the row: what a
                 label map looks like, and what the wave aggregation is for
      constant   one (truth, label) pair everywhere: every wave is uniform, one add per wave and chunk; what is left is the loads and the launch
    Per cell, alternating within every repetition: the kernel (counts cleared once in front; it accumulates) and torch's route on the SAME device
    buffers, conversions included: torch.bincount(t.long() * (C + 1) + p.long(), minlength=(C + 1) ** 2). The counts of the two routes are compared
    once. Each figure is the median over the repetitions of `steps` back-to-back calls between two stream marks (torch: two torch events); the runs
    are kept, the spread is (max - min) / median. share_of_hbm: 5 bytes a pixel over the kernel's time against 8 TB/s."""
    pkg = import_package()
    torch = None
    if not a.no_torch:
        import torch
        assert torch.cuda.is_available(), "the yardstick needs torch on the same GPU"
    n, H, W = a.batch, 375, 500
    pix = n * H * W
    rng = np.random.default_rng(0)
    result = {"batch": n, "pixels": pix, "bytes_per_pixel": 5}
    with pkg.Context(0) as ctx:
        for classes in (21, 150, 1000):
            tc = min(classes, 256)
            yy, xx = np.mgrid[0:H, 0:W]
            blocks = rng.integers(0, tc, (n, H // 25 + 1, W // 25 + 2))
            tr_b = blocks[:, yy // 25, xx // 25]
            lab_b = blocks[:, yy // 25, (xx + 1) // 25]
            inputs = {"random": (rng.integers(0, classes, pix).astype(np.int32), rng.integers(0, tc, pix).astype(np.uint8)),
                      "blocks": (lab_b.astype(np.int32).ravel(), tr_b.astype(np.uint8).ravel()),
                      "constant": (np.full(pix, classes - 1, np.int32), np.full(pix, tc - 1, np.uint8))}
            cells = (classes + 1) ** 2
            d_n = ctx.alloc(cells * 8)
            for name, (lab, tr) in inputs.items():
                if torch is not None:
                    t_lab, t_tr = torch.from_numpy(lab).cuda(), torch.from_numpy(tr).cuda()
                    p_lab, p_tr = t_lab.data_ptr(), t_tr.data_ptr()
                else:
                    t_lab, t_tr = ctx.to_device(lab), ctx.to_device(tr)
                    p_lab, p_tr = t_lab.ptr, t_tr.ptr
                ctx.lib.mbn_memset(ctx.h, d_n.ptr, 0, cells * 8)
                fn = lambda: ctx.confusion(d_n.ptr, p_lab, p_tr, 1, classes, pix)
                fn()
                ctx.sync()
                once = d_n.download((cells,), np.uint64)
                assert int(once.sum()) == pix
                agree = None
                if torch is not None:
                    route = lambda: torch.bincount(t_tr.long() * (classes + 1) + t_lab.long(), minlength=cells)
                    agree = bool(np.array_equal(route().cpu().numpy().astype(np.uint64), once))
                marks_ms(ctx, fn, 2)
                ks, ts = [], []
                for _ in range(a.reps):
                    ks.append(marks_ms(ctx, fn, a.steps))
                    if torch is None:
                        continue
                    ctx.sync()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(a.steps):
                        route()
                    e1.record()
                    torch.cuda.synchronize()
                    ts.append(e0.elapsed_time(e1) / a.steps)
                k = statistics.median(ks)
                out = {"form": "lds" if pkg.confusion_form(classes) == pkg.CONFUSION_FORM_LDS else "global", "kernel_ms": round(k, 4),
                       "kernel_runs_ms": [round(v, 4) for v in ks], "spread": round((max(ks) - min(ks)) / k, 4),
                       "share_of_hbm": round(5.0 * pix / (k * 1e-3) / HBM_BYTES_PER_S, 4), "nonzero_cells": int((once != 0).sum())}
                if ts:
                    tm = statistics.median(ts)
                    out.update({"torch_ms": round(tm, 4), "torch_runs_ms": [round(v, 4) for v in ts], "torch_over_kernel": round(tm / k, 2),
                                "counts_equal_torch": agree})
                print("classes %4d %-6s (%s): kernel %.4f ms (spread %.1f %%, %.1f %% of 8 TB/s at 5 B/pixel)  torch %s ms" %
                      (classes, name, out["form"], k, 100 * out["spread"], 100 * out["share_of_hbm"], ("%.4f" % out["torch_ms"]) if ts else "-"),
                      flush=True)
                result["classes_%d_%s" % (classes, name)] = out
                if torch is not None:
                    del t_lab, t_tr
                    torch.cuda.empty_cache()
                else:
                    t_lab.free()
                    t_tr.free()
            d_n.free()
    print(json.dumps(result))


CALIBRATION_LAB_PLAIN = 1010        # lab exp0 of mbn_f32_calibration.hip: every lane adds on its own (no wave aggregation)


def main_calibration(a):
    """--calibration: mbn_calibration_f32 on --batch maps of 375 x 500 (6 M pixels at 32), int32 labels and fp32 probabilities against a uint8
    truth, 21 classes, 15 and 1024 bins. Three inputs:
      random     prob uniform in [0, 1) per pixel, the truth uniform over the classes: the lanes of a wave hold many different bins
      blocks     25 x 25 blocks of one truth class and one prob: what a confident region looks like, and what the wave aggregation is for
      constant   one (truth, label, prob) everywhere: one leader per wave
    In all three the label equals the truth with probability prob (else the next class), so the table is a calibrated one.
    Per cell, alternating within every repetition: the kernel (table cleared once in front; it accumulates), with MBN_LAB=1 the kernel without the
    wave aggregation (lab exp0 = 1010), mbn_confusion_i32 on the same labels and truth, and torch's route on the SAME device buffers: the bin as
    the kernel forms it (one fp32 multiply, truncate, clamp: torch.bucketize over the edges j / bins gives the same buckets only for a power of
    two), then torch.bincount with float64 weights for each of the four columns. The tables are compared once (the float64 column after rounding).
    Each figure is the median over the repetitions of `steps` back-to-back calls between two stream marks (torch: two torch events); the runs are
    kept, the spread is (max - min) / median. share_of_hbm: 9 bytes a pixel over the kernel's time against 8 TB/s."""
    pkg = import_package()
    torch = None
    if not a.no_torch:
        import torch
        assert torch.cuda.is_available(), "the yardstick needs torch on the same GPU"
    n, H, W, classes = a.batch, 375, 500, 21
    pix = n * H * W
    rng = np.random.default_rng(0)
    result = {"batch": n, "pixels": pix, "bytes_per_pixel": 9, "classes": classes}
    yy, xx = np.mgrid[0:H, 0:W]
    tr_blocks = rng.integers(0, classes, (n, H // 25 + 1, W // 25 + 1))
    pr_blocks = rng.random((n, H // 25 + 1, W // 25 + 1)) ** 0.25
    truths = {"random": rng.integers(0, classes, pix), "blocks": tr_blocks[:, yy // 25, xx // 25].ravel(), "constant": np.full(pix, classes - 1)}
    probs = {"random": rng.random(pix), "blocks": pr_blocks[:, yy // 25, xx // 25].ravel(), "constant": np.full(pix, 0.97)}
    with pkg.Context(0) as ctx:
        lab_knob = ctx.lib.mbn_tune_set(b"exp0", 0) == pkg.OK          # the lab library: the plain form can be timed beside the shipped one
        result["lab"] = bool(lab_knob)
        d_counts = ctx.alloc((classes + 1) ** 2 * 8)
        for name in ("random", "blocks", "constant"):
            tr, pr = truths[name].astype(np.uint8), probs[name].astype(np.float32)
            lab = np.where(rng.random(pix) < pr, tr, (tr + 1) % classes).astype(np.int32) if name != "constant" else tr.astype(np.int32)
            if torch is not None:
                t_lab, t_pr, t_tr = torch.from_numpy(lab).cuda(), torch.from_numpy(pr).cuda(), torch.from_numpy(tr).cuda()
                p_lab, p_pr, p_tr = t_lab.data_ptr(), t_pr.data_ptr(), t_tr.data_ptr()
            else:
                t_lab, t_pr, t_tr = ctx.to_device(lab), ctx.to_device(pr), ctx.to_device(tr)
                p_lab, p_pr, p_tr = t_lab.ptr, t_pr.ptr, t_tr.ptr
            conf = lambda: ctx.confusion(d_counts.ptr, p_lab, p_tr, 1, classes, pix)
            for bins in (15, 1024):
                cells = (bins + 1) * 4
                d_cal = ctx.alloc(cells * 8)
                fn = lambda: ctx.calibration(d_cal.ptr, p_lab, p_pr, p_tr, 1, classes, bins, pix)

                def table_of(knob):
                    if lab_knob:
                        ctx.lib.mbn_tune_set(b"exp0", knob)
                    ctx.lib.mbn_memset(ctx.h, d_cal.ptr, 0, cells * 8)
                    fn()
                    ctx.sync()
                    return d_cal.download((bins + 1, 4), np.uint64)

                once = table_of(0)
                assert int(once[:, 0].sum() + once[:, 3].sum()) == pix
                plain_equal = bool(np.array_equal(table_of(CALIBRATION_LAB_PLAIN), once)) if lab_knob else None
                agree = None
                if torch is not None:
                    def route():
                        p = torch.clamp(torch.nan_to_num(t_pr, nan=0.0), 0.0, 1.0)
                        b = torch.clamp((p * float(bins)).to(torch.int64), max=bins - 1)
                        valid = t_tr.long() < classes
                        answered = valid & (t_lab >= 0) & (t_lab < classes)
                        q = (p * 16777216.0).to(torch.int64).to(torch.float64)
                        cols = [torch.bincount(b, weights=w, minlength=bins) for w in
                                (answered.double(), (answered & (t_lab == t_tr.long())).double(), answered.double() * q, (valid & ~answered).double())]
                        return torch.stack(cols, 1), (~valid).sum()
                    got, void = route()
                    want = np.zeros((bins + 1, 4), np.uint64)
                    want[:bins] = np.rint(got.cpu().numpy()).astype(np.uint64)
                    want[bins, 0] = int(void)
                    agree = bool(np.array_equal(want, once))
                marks_ms(ctx, fn, 2)
                marks_ms(ctx, conf, 2)
                ks, ps, cs, ts = [], [], [], []
                for _ in range(a.reps):
                    if lab_knob:
                        ctx.lib.mbn_tune_set(b"exp0", 0)
                    ks.append(marks_ms(ctx, fn, a.steps))
                    if lab_knob:
                        ctx.lib.mbn_tune_set(b"exp0", CALIBRATION_LAB_PLAIN)
                        ps.append(marks_ms(ctx, fn, a.steps))
                        ctx.lib.mbn_tune_set(b"exp0", 0)
                    cs.append(marks_ms(ctx, conf, a.steps))
                    if torch is None:
                        continue
                    ctx.sync()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(max(a.steps // 4, 1)):
                        route()
                    e1.record()
                    torch.cuda.synchronize()
                    ts.append(e0.elapsed_time(e1) / max(a.steps // 4, 1))
                k, c = statistics.median(ks), statistics.median(cs)
                out = {"kernel_ms": round(k, 4), "kernel_runs_ms": [round(v, 4) for v in ks], "spread": round((max(ks) - min(ks)) / k, 4),
                       "share_of_hbm": round(9.0 * pix / (k * 1e-3) / HBM_BYTES_PER_S, 4), "nonzero_cells": int((once != 0).sum()),
                       "confusion_ms": round(c, 4), "confusion_runs_ms": [round(v, 4) for v in cs], "kernel_over_confusion": round(k / c, 2)}
                if ps:
                    p_ms = statistics.median(ps)
                    out.update({"plain_ms": round(p_ms, 4), "plain_runs_ms": [round(v, 4) for v in ps], "plain_over_kernel": round(p_ms / k, 2),
                                "plain_table_equal": plain_equal})
                if ts:
                    tm = statistics.median(ts)
                    out.update({"torch_ms": round(tm, 4), "torch_runs_ms": [round(v, 4) for v in ts], "torch_over_kernel": round(tm / k, 2),
                                "table_equal_torch": agree})
                print("%-8s bins %4d: kernel %.4f ms (%.4f - %.4f, %.1f %% of 8 TB/s at 9 B/pixel)  plain %s ms  confusion %.4f ms  torch %s ms" %
                      (name, bins, k, min(ks), max(ks), 100 * out["share_of_hbm"], ("%.4f" % out["plain_ms"]) if ps else "-", c,
                       ("%.4f" % out["torch_ms"]) if ts else "-"), flush=True)
                result["%s_bins_%d" % (name, bins)] = out
                d_cal.free()
            if torch is not None:
                del t_lab, t_pr, t_tr
                torch.cuda.empty_cache()
            else:
                for buf in (t_lab, t_pr, t_tr):
                    buf.free()
        d_counts.free()
    print(json.dumps(result))


def main_regions(a):
    """--regions: mbn_components_i32 on --batch maps of 375 x 500 (6 M pixels at 32) at 21 / 150 / 1000 classes. Three inputs per class count:
      random     labels uniform over the classes: nearly every pixel its own region at 1000 classes, large tangled ones at 21 under connectivity 8
      blocks     blocks of 25 x 25 pixels of one class: what a label map looks like
      constant   one class everywhere: one region through every seam; every union and every area add of an image meets on one word
    x connectivity 4 / 8 x (min_area 1 writing comp alone: 8 bytes a pixel; min_area 50 writing comp and labels_out: 12 bytes a pixel). The table
    holds 4096 regions a map. Each figure is the median over the repetitions of `steps` back-to-back calls between two stream marks; the runs are
    kept, the spread is (max - min) / median. share_of_hbm: the bytes above over the call's time against 8 TB/s. The results are checked once per
    cell against the host's (n_regions of the first --host-maps maps).
    host_ms: what a user has without the call: the download of the maps, then scipy.ndimage.label once per class present, on the first --host-maps
    maps, scaled to the batch (host_maps says how many were really labelled)."""
    pkg = import_package()
    n, H, W = a.batch, 375, 500
    pix, max_regions = n * H * W, 4096
    rng = np.random.default_rng(0)
    result = {"batch": n, "pixels": pix, "max_regions": max_regions}
    eight, four = np.ones((3, 3), int), np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]])
    with pkg.Context(0) as ctx:
        handle = pkg.Components(ctx, n, pix)
        d_comp, d_out, d_reg, d_n = ctx.alloc(4 * pix), ctx.alloc(4 * pix), ctx.alloc(32 * n * max_regions), ctx.alloc(4 * n)
        for classes in (21, 150, 1000):
            yy, xx = np.mgrid[0:H, 0:W]
            coarse = rng.integers(0, classes, (n, H // 25 + 1, W // 25 + 1))
            inputs = {"random": rng.integers(0, classes, (n, H, W)).astype(np.int32), "blocks": coarse[:, yy // 25, xx // 25].astype(np.int32),
                      "constant": np.full((n, H, W), classes - 1, np.int32)}
            for name, maps in inputs.items():
                if a.configs and name not in a.configs.split(","):     # --configs random,blocks,constant: one input kind (a profiler run of its own)
                    continue
                d_lab = ctx.to_device(maps)
                for conn in (4, 8):
                    host_ms, host_n = None, None
                    if not a.no_host:
                        from scipy import ndimage
                        import time
                        k = min(a.host_maps, n)
                        t0 = time.perf_counter()
                        got = d_lab.download((n, H, W), np.int32)
                        host_n = []
                        for i in range(k):
                            host_n.append(sum(ndimage.label(got[i] == c, structure=eight if conn == 8 else four)[1] for c in np.unique(got[i])))
                        t1 = time.perf_counter()
                        t_dl = time.perf_counter()
                        d_lab.download((n, H, W), np.int32)
                        t_dl = time.perf_counter() - t_dl
                        host_ms = 1e3 * (t_dl + (t1 - t0 - t_dl) * n / k)
                    for min_area in (1, 50):
                        out_ptr = d_out.ptr if min_area > 1 else None
                        fn = lambda: ctx.components(handle, d_lab.ptr, n, H, W, classes, d_n.ptr, comp=d_comp.ptr, regions=d_reg.ptr,
                                                    labels_out=out_ptr, connectivity=conn, min_area=min_area, ignore_label=classes,
                                                    max_regions=max_regions)
                        fn()
                        ctx.sync()
                        counts = d_n.download((n,), np.int32)
                        if host_n is not None and min_area == 1:
                            assert counts[:len(host_n)].tolist() == host_n, (classes, name, conn, counts[:len(host_n)].tolist(), host_n)
                        marks_ms(ctx, fn, 2)
                        ks = [marks_ms(ctx, fn, a.steps) for _ in range(a.reps)]
                        k_ms = statistics.median(ks)
                        bpp = 12 if min_area > 1 else 8
                        out = {"call_ms": round(k_ms, 4), "runs_ms": [round(v, 4) for v in ks], "spread": round((max(ks) - min(ks)) / k_ms, 4),
                               "bytes_per_pixel": bpp, "floor_ms": round(1e3 * bpp * pix / HBM_BYTES_PER_S, 4),
                               "share_of_hbm": round(bpp * pix / (k_ms * 1e-3) / HBM_BYTES_PER_S, 4), "regions_per_map": round(float(counts.mean()), 1)}
                        if host_ms is not None:
                            out.update({"host_ms": round(host_ms, 1), "host_maps": len(host_n), "host_over_call": round(host_ms / k_ms, 1)})
                        print("classes %4d %-8s conn %d min_area %2d: call %.4f ms (spread %.1f %%, floor %.4f ms, %.1f %% of 8 TB/s)  regions/map %.1f  "
                              "host %s ms" % (classes, name, conn, min_area, k_ms, 100 * out["spread"], out["floor_ms"], 100 * out["share_of_hbm"],
                                              out["regions_per_map"], ("%.1f" % host_ms) if host_ms is not None else "-"), flush=True)
                        result["classes_%d_%s_c%d_a%d" % (classes, name, conn, min_area)] = out
                d_lab.free()
        handle.close()
    print(json.dumps(result))


def main_boundary(a):
    """--boundary: mbn_boundary_score_i32 (both tables) on --batch maps of 375 x 500 (6 M pixels at 32), int32 labels against uint8 truth, at
    21 / 150 / 1000 classes, main_score's three inputs (random: every pixel is in every band; blocks of 25 x 25 with the prediction shifted by one
    pixel: what a label map looks like; constant: no band but the frame's), d = 12 (375 x 500 at ratio 0.02) and d = 3, edge 0 and 1.
    Per cell, alternating within every repetition, on the SAME device buffers:
      kernel     the fused call, tables cleared once in front (it accumulates)
      confusion  mbn_confusion_i32: the price of contour scoring as a multiple of plain scoring
      torch      conversions included: one_hot -> the complement -> max_pool2d with one (2 d + 1) window (edge 1: the complement padded with ones
                 first; edge 0: the pool's own padding, which never wins) -> the own channel picks the band -> bincount of the masked cells, for
                 truth and prediction; in image chunks of at most 4096 planes. Its tables are compared with the kernel's once per cell.
    Each figure is the median over the repetitions of `steps` (torch: --torch-steps) back-to-back calls between two stream marks (torch: two torch
    events); the runs are kept, the spread is (max - min) / median. floor_ms: 5 bytes a pixel over 8 TB/s.
    host_ms, once per (classes, input, d) at edge 1: what a user has without the call: the download of both maps, then per class present
    mask & ~scipy.ndimage.binary_erosion(mask, ones((3, 3)), iterations=d, border_value=0) for truth and prediction and the three sums, on the
    first --host-maps maps, scaled to the batch; its biou table is compared with the kernel's on those maps."""
    pkg = import_package()
    torch = None
    if not a.no_torch:
        import torch
        import torch.nn.functional as F
        assert torch.cuda.is_available(), "the yardstick needs torch on the same GPU"
    n, H, W = a.batch, 375, 500
    pix = n * H * W
    rng = np.random.default_rng(0)
    result = {"batch": n, "pixels": pix, "bytes_per_pixel": 5, "floor_ms": round(1e3 * 5.0 * pix / HBM_BYTES_PER_S, 4)}

    def spread(v):
        return round((max(v) - min(v)) / statistics.median(v), 4)

    with pkg.Context(0) as ctx:
        for classes in (21, 150, 1000):
            tc = min(classes, 256)
            yy, xx = np.mgrid[0:H, 0:W]
            blocks = rng.integers(0, tc, (n, H // 25 + 1, W // 25 + 2))
            inputs = {"random": (rng.integers(0, classes, (n, H, W)).astype(np.int32), rng.integers(0, tc, (n, H, W)).astype(np.uint8)),
                      "blocks": (blocks[:, yy // 25, (xx + 1) // 25].astype(np.int32), blocks[:, yy // 25, xx // 25].astype(np.uint8)),
                      "constant": (np.full((n, H, W), classes - 1, np.int32), np.full((n, H, W), tc - 1, np.uint8))}
            inputs = {k: (np.ascontiguousarray(v[0]), np.ascontiguousarray(v[1])) for k, v in inputs.items()}     # [n][H][W] in memory
            cells, bcells = (classes + 1) ** 2, classes * 3
            d_tri, d_bio, d_n = ctx.alloc(cells * 8), ctx.alloc(bcells * 8), ctx.alloc(cells * 8)
            for name, (lab, tr) in inputs.items():
                if a.configs and name not in a.configs.split(","):
                    continue
                if torch is not None:
                    t_lab, t_tr = torch.from_numpy(lab).cuda(), torch.from_numpy(tr).cuda()
                    p_lab, p_tr = t_lab.data_ptr(), t_tr.data_ptr()
                else:
                    t_lab, t_tr = ctx.to_device(lab), ctx.to_device(tr)
                    p_lab, p_tr = t_lab.ptr, t_tr.ptr
                conf = lambda: ctx.confusion(d_n.ptr, p_lab, p_tr, 1, classes, pix)
                for d in (12, 3):
                    host_ms, host_bio, k_host = None, None, min(a.host_maps, n)
                    if not a.no_host:
                        from scipy import ndimage
                        import time
                        t0 = time.perf_counter()
                        h_lab = np.empty((n, H, W), np.int32)
                        h_tr = np.empty((n, H, W), np.uint8)
                        ctx.lib.mbn_download(ctx.h, h_lab.ctypes.data, p_lab, h_lab.nbytes)
                        ctx.lib.mbn_download(ctx.h, h_tr.ctypes.data, p_tr, h_tr.nbytes)
                        t_dl = time.perf_counter() - t0
                        host_bio = np.zeros((classes, 3), np.uint64)
                        t0 = time.perf_counter()
                        for i in range(k_host):
                            for c in np.union1d(np.unique(h_lab[i]), np.unique(h_tr[i])):
                                bands = []
                                for m in (h_tr[i] == c, h_lab[i] == c):
                                    bands.append(m & ~ndimage.binary_erosion(m, structure=np.ones((3, 3)), iterations=d, border_value=0))
                                host_bio[c] += np.array([bands[0].sum(), bands[1].sum(), (bands[0] & bands[1]).sum()], np.uint64)
                        host_ms = 1e3 * (t_dl + (time.perf_counter() - t0) * n / k_host)
                    for edge in (1, 0):
                        fn = lambda: ctx.boundary_score(d_tri.ptr, d_bio.ptr, p_lab, p_tr, 1, classes, n, H, W, d, edge)
                        ctx.lib.mbn_memset(ctx.h, d_tri.ptr, 0, cells * 8)
                        ctx.lib.mbn_memset(ctx.h, d_bio.ptr, 0, bcells * 8)
                        fn()
                        ctx.sync()
                        tri, bio = d_tri.download((cells,), np.uint64), d_bio.download((classes, 3), np.uint64)
                        agree_host = None
                        if host_bio is not None and edge == 1:
                            ctx.lib.mbn_memset(ctx.h, d_bio.ptr, 0, bcells * 8)
                            ctx.boundary_score(None, d_bio.ptr, p_lab, p_tr, 1, classes, k_host, H, W, d, 1)
                            ctx.sync()
                            agree_host = bool(np.array_equal(d_bio.download((classes, 3), np.uint64), host_bio))
                        agree = None
                        if torch is not None:
                            chunk = max(1, 4096 // classes)

                            def route():
                                tri_t = torch.zeros(cells, dtype=torch.int64, device="cuda")
                                bio_t = torch.zeros((3, classes), dtype=torch.int64, device="cuda")
                                for i0 in range(0, n, chunk):
                                    t, p = t_tr[i0:i0 + chunk].long(), t_lab[i0:i0 + chunk].long()
                                    band = []
                                    for x in (t, p):
                                        oh = F.one_hot(x, classes).permute(0, 3, 1, 2).to(torch.float16)
                                        comp = 1 - oh
                                        if edge:
                                            pooled = F.max_pool2d(F.pad(comp, (d, d, d, d), value=1.0), 2 * d + 1, stride=1)
                                        else:
                                            pooled = F.max_pool2d(comp, 2 * d + 1, stride=1, padding=d)
                                        band.append((pooled * oh).sum(1) > 0)
                                    tri_t += torch.bincount((t * (classes + 1) + p)[band[0]], minlength=cells)
                                    bio_t[0] += torch.bincount(t[band[0]], minlength=classes)
                                    bio_t[1] += torch.bincount(p[band[1]], minlength=classes)
                                    bio_t[2] += torch.bincount(t[band[0] & band[1] & (t == p)], minlength=classes)
                                return tri_t, bio_t

                            tri_t, bio_t = route()
                            agree = bool(np.array_equal(tri_t.cpu().numpy().astype(np.uint64), tri) and
                                         np.array_equal(bio_t.t().cpu().numpy().astype(np.uint64), bio))
                        marks_ms(ctx, fn, 2)
                        marks_ms(ctx, conf, 2)
                        ks, cs, ts = [], [], []
                        for _ in range(a.reps):
                            ks.append(marks_ms(ctx, fn, a.steps))
                            cs.append(marks_ms(ctx, conf, a.steps))
                            if torch is None:
                                continue
                            ctx.sync()
                            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                            e0.record()
                            for _ in range(a.torch_steps):
                                route()
                            e1.record()
                            torch.cuda.synchronize()
                            ts.append(e0.elapsed_time(e1) / a.torch_steps)
                        k, c_ms = statistics.median(ks), statistics.median(cs)
                        out = {"kernel_ms": round(k, 4), "kernel_runs_ms": [round(v, 4) for v in ks], "spread": spread(ks),
                               "confusion_ms": round(c_ms, 4), "confusion_runs_ms": [round(v, 4) for v in cs], "kernel_over_confusion": round(k / c_ms, 2),
                               "share_of_hbm": round(5.0 * pix / (k * 1e-3) / HBM_BYTES_PER_S, 4), "truth_band_share": round(int(tri.sum()) / pix, 4)}
                        if ts:
                            tm = statistics.median(ts)
                            out.update({"torch_ms": round(tm, 3), "torch_runs_ms": [round(v, 3) for v in ts], "torch_over_kernel": round(tm / k, 1),
                                        "tables_equal_torch": agree})
                        if host_ms is not None:
                            out.update({"host_ms": round(host_ms, 1), "host_maps": k_host, "host_over_kernel": round(host_ms / k, 1)})
                            if agree_host is not None:
                                out["biou_equal_host"] = agree_host
                        print("classes %4d %-8s d %2d edge %d: kernel %.4f ms (%.4f - %.4f, %.1f %% of 8 TB/s at 5 B/pixel, band %.1f %%)  confusion %.4f ms  "
                              "torch %s ms  host %s ms" % (classes, name, d, edge, k, min(ks), max(ks), 100 * out["share_of_hbm"], 100 * out["truth_band_share"],
                                                           c_ms, ("%.3f" % out["torch_ms"]) if ts else "-",
                                                           ("%.1f" % host_ms) if host_ms is not None else "-"), flush=True)
                        result["classes_%d_%s_d%d_e%d" % (classes, name, d, edge)] = out
                if torch is not None:
                    del t_lab, t_tr
                    torch.cuda.empty_cache()
                else:
                    t_lab.free()
                    t_tr.free()
            for b in (d_tri, d_bio, d_n):
                b.free()
    print(json.dumps(result))


def surface_rows(d2, bins):
    """the cells of one class and direction of a surface table from the int64 d2 of its matched queries (numpy), without n and unmatched"""
    import math
    row = np.zeros(4 + bins, np.uint64)
    if len(d2):
        row[2] = int(d2.max())
        row[3] = sum(math.isqrt(int(v) << 16) for v in d2)
        t = np.array([math.isqrt(int(v)) for v in d2], np.int64)
        row[4:] = np.bincount(np.minimum(t + (t * t < d2), bins - 1), minlength=bins).astype(np.uint64)
    return row


def main_surface(a):
    """--surface: mbn_surface_score_i32 on --batch maps of 375 x 500 (6 M pixels at 32), int32 labels against uint8 truth, 64 bins, edge 1, at 21 and
    1000 classes. Inputs: blocks (25 x 25 blocks against the same blocks shifted by one pixel, 3 % of the prediction's pixels redrawn: what a label
    map looks like), constant (no contour but the frame), random (every pixel is a contour pixel) and far (class 1 is a strip of 40 columns at the
    far left of the labels and at the far right of the truth: every one of its queries walks 420 rings or more, the worst case of an uncapped search).
    Per cell, on the SAME device buffers:
      kernel  the call (three kernels), table cleared once in front (it accumulates); with dist2 and without
      torch   per map and class the contour coordinates of both sides (eight shifted compares), torch.cdist between them (exact mode), the row
              minima both ways, squared and rounded, and the table's cells from them; on the first --torch-images maps, scaled to the batch
      host    what a user has without the call: the download of both maps, then per class present the contour (mask & ~binary_erosion) and
              scipy.ndimage.distance_transform_edt of the other side's complement read at the queries; on the first --host-maps maps, scaled
    Both yardsticks' tables are compared with the kernel's on their maps. Each kernel figure is the median over the repetitions of `steps`
    back-to-back calls between two stream marks; the runs are kept. floor_ms: 21 bytes a pixel over 8 TB/s (pass A reads 5 and writes the two
    contour maps, 8; pass B reads those 8 once as queries; what the search reads beyond that comes from the cache when the match is near)."""
    pkg = import_package()
    torch = None
    if not a.no_torch:
        import torch
        assert torch.cuda.is_available(), "the yardstick needs torch on the same GPU"
    import time
    n, H, W, bins, edge = a.batch, 375, 500, 64, 1
    pix = n * H * W
    rng = np.random.default_rng(0)
    result = {"batch": n, "pixels": pix, "bins": bins, "edge": edge, "bytes_per_pixel": 21, "floor_ms": round(1e3 * 21.0 * pix / HBM_BYTES_PER_S, 4)}

    def host_table(h_lab, h_tr, classes):
        from scipy import ndimage
        surf = np.zeros((classes, 2, 4 + bins), np.uint64)
        el = np.ones((3, 3))
        for lab, tr in zip(h_lab, h_tr):
            maps = (lab.astype(np.int64), tr.astype(np.int64))
            for c in np.union1d(np.unique(maps[0]), np.unique(maps[1])):
                if not 0 <= c < classes:
                    continue
                cont = [(m == c) & ~ndimage.binary_erosion(m == c, structure=el, border_value=0) for m in maps]
                for k in range(2):
                    q = int(cont[k].sum())
                    surf[c, k, 0] += np.uint64(q)
                    if not q:
                        continue
                    if not cont[1 - k].any():
                        surf[c, k, 1] += np.uint64(q)
                        continue
                    d2 = np.rint(ndimage.distance_transform_edt(~cont[1 - k]) ** 2).astype(np.int64)[cont[k]]
                    row = surface_rows(d2, bins)
                    surf[c, k, 2] = max(surf[c, k, 2], row[2])
                    surf[c, k, 3] += row[3]
                    surf[c, k, 4:] += row[4:]
        return surf

    def torch_table(t_lab, t_tr, classes, k_maps):
        surf = torch.zeros((classes, 2, 4 + bins), dtype=torch.int64, device="cuda")

        def contour(m):
            p = torch.nn.functional.pad(m, (1, 1, 1, 1), value=-7)
            out = torch.zeros_like(m, dtype=torch.bool)
            for dr in range(3):
                for dc in range(3):
                    out |= p[dr:dr + H, dc:dc + W] != m
            return out

        def isqrt(v):
            t = v.double().sqrt().floor().long()
            t = torch.where(t * t > v, t - 1, t)
            return torch.where((t + 1) * (t + 1) <= v, t + 1, t)

        for i in range(k_maps):
            maps = (t_lab[i].long(), t_tr[i].long())
            cont = [contour(m) for m in maps]
            present = torch.unique(torch.cat([maps[0][cont[0]], maps[1][cont[1]]]))
            for c in present.tolist():
                if not 0 <= c < classes:
                    continue
                pts = [torch.nonzero(cont[k] & (maps[k] == c)).double() for k in range(2)]
                for k in range(2):
                    q = pts[k].shape[0]
                    surf[c, k, 0] += q
                    if not q:
                        continue
                    if not pts[1 - k].shape[0]:
                        surf[c, k, 1] += q
                        continue
                    near = torch.cat([torch.cdist(pts[k][j:j + 2048], pts[1 - k], compute_mode="donot_use_mm_for_euclid_dist").min(1).values
                                      for j in range(0, q, 2048)])
                    d2 = (near.double() ** 2).round().long()
                    surf[c, k, 2] = torch.maximum(surf[c, k, 2], d2.max())
                    surf[c, k, 3] += isqrt(d2 << 16).sum()
                    t = isqrt(d2)
                    surf[c, k, 4:] += torch.bincount(torch.clamp(t + (t * t < d2).long(), max=bins - 1), minlength=bins)
        return surf

    with pkg.Context(0) as ctx:
        for classes in (21, 1000):
            tc = min(classes, 256)
            yy, xx = np.mgrid[0:H, 0:W]
            blocks = rng.integers(0, tc, (n, H // 25 + 1, W // 25 + 2))
            shifted = blocks[:, yy // 25, (xx + 1) // 25].astype(np.int32)
            noise = rng.random((n, H, W)) < 0.03
            shifted[noise] = rng.integers(0, classes, int(noise.sum()))
            far_l, far_t = np.zeros((n, H, W), np.int32), np.zeros((n, H, W), np.uint8)
            far_l[:, :, :40], far_t[:, :, W - 40:] = 1, 1
            inputs = {"blocks": (shifted, blocks[:, yy // 25, xx // 25].astype(np.uint8)),
                      "constant": (np.full((n, H, W), classes - 1, np.int32), np.full((n, H, W), tc - 1, np.uint8)),
                      "random": (rng.integers(0, classes, (n, H, W)).astype(np.int32), rng.integers(0, tc, (n, H, W)).astype(np.uint8)),
                      "far": (far_l, far_t)}
            inputs = {k: (np.ascontiguousarray(v[0]), np.ascontiguousarray(v[1])) for k, v in inputs.items()}
            cells = classes * 2 * (4 + bins)
            d_surf, d_d2 = ctx.alloc(cells * 8), ctx.alloc(pix * 4)
            h = pkg.Surface(ctx, n, pix, classes)
            for name, (lab, tr) in inputs.items():
                if a.configs and name not in a.configs.split(","):
                    continue
                if name == "far" and classes != 21:
                    continue
                if torch is not None:
                    t_lab, t_tr = torch.from_numpy(lab).cuda(), torch.from_numpy(tr).cuda()
                    p_lab, p_tr = t_lab.data_ptr(), t_tr.data_ptr()
                else:
                    t_lab, t_tr = ctx.to_device(lab), ctx.to_device(tr)
                    p_lab, p_tr = t_lab.ptr, t_tr.ptr

                def table_of(k_maps):
                    ctx.lib.mbn_memset(ctx.h, d_surf.ptr, 0, cells * 8)
                    ctx.surface_score(h, d_surf.ptr, p_lab, p_tr, 1, classes, bins, k_maps, H, W, edge)
                    ctx.sync()
                    return d_surf.download((classes, 2, 4 + bins), np.uint64)

                full = table_of(n)
                out = {"queries": int(full[:, :, 0].sum()), "unmatched": int(full[:, :, 1].sum()), "max_d2": int(full[:, :, 2].max())}
                k_host, k_torch = min(a.host_maps, n), min(a.torch_images, n)
                if not a.no_host:
                    t0 = time.perf_counter()
                    h_lab, h_tr = np.empty((n, H, W), np.int32), np.empty((n, H, W), np.uint8)
                    ctx.lib.mbn_download(ctx.h, h_lab.ctypes.data, p_lab, h_lab.nbytes)
                    ctx.lib.mbn_download(ctx.h, h_tr.ctypes.data, p_tr, h_tr.nbytes)
                    t_dl = time.perf_counter() - t0
                    t0 = time.perf_counter()
                    host = host_table(h_lab[:k_host], h_tr[:k_host], classes)
                    out.update({"host_ms": round(1e3 * (t_dl + (time.perf_counter() - t0) * n / k_host), 1), "host_maps": k_host,
                                "table_equal_host": bool(np.array_equal(host, table_of(k_host)))})
                if torch is not None:
                    want = torch_table(t_lab, t_tr, classes, k_torch)        # once in front: compared, and the allocator is warm
                    out["table_equal_torch"] = bool(np.array_equal(want.cpu().numpy().astype(np.uint64), table_of(k_torch)))
                    ts = []
                    for _ in range(max(1, a.torch_steps)):
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        torch_table(t_lab, t_tr, classes, k_torch)
                        torch.cuda.synchronize()
                        ts.append(1e3 * (time.perf_counter() - t0) * n / k_torch)
                    out.update({"torch_ms": round(statistics.median(ts), 1), "torch_runs_ms": [round(v, 1) for v in ts], "torch_maps": k_torch})
                for key, d2 in (("kernel", None), ("kernel_dist2", d_d2.ptr)):
                    fn = lambda: ctx.surface_score(h, d_surf.ptr, p_lab, p_tr, 1, classes, bins, n, H, W, edge, dist2=d2)
                    steps = 2 if name == "far" else a.steps
                    marks_ms(ctx, fn, 1)
                    ks = [marks_ms(ctx, fn, steps) for _ in range(a.reps)]
                    k = statistics.median(ks)
                    out.update({key + "_ms": round(k, 4), key + "_runs_ms": [round(v, 4) for v in ks]})
                k = out["kernel_ms"]
                out["share_of_hbm"] = round(21.0 * pix / (k * 1e-3) / HBM_BYTES_PER_S, 4)
                if "host_ms" in out:
                    out["host_over_kernel"] = round(out["host_ms"] / k, 1)
                if "torch_ms" in out:
                    out["torch_over_kernel"] = round(out["torch_ms"] / k, 1)
                print("classes %4d %-8s: kernel %.4f ms (%.4f - %.4f, %.2f %% of 8 TB/s at 21 B/pixel), with dist2 %.4f ms; queries %d, unmatched %d, "
                      "max_d2 %d; torch %s ms (equal %s)  host %s ms (equal %s)" %
                      (classes, name, k, min(out["kernel_runs_ms"]), max(out["kernel_runs_ms"]), 100 * out["share_of_hbm"], out["kernel_dist2_ms"],
                       out["queries"], out["unmatched"], out["max_d2"], out.get("torch_ms", "-"), out.get("table_equal_torch", "-"),
                       out.get("host_ms", "-"), out.get("table_equal_host", "-")), flush=True)
                result["classes_%d_%s" % (classes, name)] = out
                if torch is not None:
                    del t_lab, t_tr
                    torch.cuda.empty_cache()
                else:
                    t_lab.free()
                    t_tr.free()
            h.close()
            d_surf.free()
            d_d2.free()
    print(json.dumps(result))


def pq_from_pairs(img, p, g, cnt, rec_p, n_p, rec_t, n_t, classes):
    """pq uint64 [classes][4] from the pair histogram of a batch: (img, p, g) unique with p >= 0, g = -1 over void truth, cnt pixels each. The match
    rule of include/mbn.h, "score a segmentation by its regions", vectorised; rec_*: int64 [batch][cap][8], n_*: [batch]"""
    batch, cap_p, cap_t = rec_p.shape[0], rec_p.shape[1], rec_t.shape[1]
    void = np.zeros(batch * cap_p, np.int64)
    void[(img * cap_p + p)[g < 0]] = cnt[g < 0]
    k = g >= 0
    img, p, g, cnt = img[k], p[k], g[k], cnt[k]
    lab_p, lab_g = rec_p[img, p, 0], rec_t[img, g, 0]
    union = rec_p[img, p, 1] - void[img * cap_p + p] + rec_t[img, g, 1] - cnt
    match = (lab_p == lab_g) & (2 * cnt > union)
    pq = np.zeros((classes, 4), np.uint64)
    inside = match & (lab_p >= 0) & (lab_p < classes)
    pq[:, 0] = np.bincount(lab_p[inside], minlength=classes).astype(np.uint64)
    np.add.at(pq[:, 3], lab_p[inside], (cnt[inside].astype(np.uint64) << np.uint64(32)) // union[inside].astype(np.uint64))
    hit_p, hit_g = np.zeros(batch * cap_p, bool), np.zeros(batch * cap_t, bool)
    hit_p[(img * cap_p + p)[match]] = True
    hit_g[(img * cap_t + g)[match]] = True
    listed_p, listed_g = np.arange(cap_p)[None, :] < n_p[:, None], np.arange(cap_t)[None, :] < n_t[:, None]
    labs_p, labs_g = rec_p[:, :, 0], rec_t[:, :, 0]
    fp = listed_p & ~hit_p.reshape(batch, cap_p) & ~(2 * void.reshape(batch, cap_p) > rec_p[:, :, 1]) & (labs_p >= 0) & (labs_p < classes)
    fn = listed_g & ~hit_g.reshape(batch, cap_t) & (labs_g >= 0) & (labs_g < classes)
    pq[:, 1] = np.bincount(labs_p[fp], minlength=classes).astype(np.uint64)
    pq[:, 2] = np.bincount(labs_g[fn], minlength=classes).astype(np.uint64)
    return pq


def main_panoptic(a):
    """--panoptic: mbn_panoptic_i32 on --batch maps of 375 x 500 (6 M pixels at 32) at 21 / 1000 classes. Three inputs per class count:
      blocks     the truth is blocks of 25 x 25 pixels of one class; the prediction is the same blocks shifted by two columns with 3 % of the
                 pixels at random classes: what a label map looks like
      random     labels uniform over the classes on both sides: at 1000 classes nearly every pixel is a segment of its own, no majorities
      constant   one class everywhere on both sides: one segment a map, every wave inside it
    The segment maps, tables and counts come from mbn_components_i32 (connectivity 4, min_area 1) with tables of 375 x 500 records a side, so
    every image is scored. Per cell, alternating within every repetition, on the SAME device buffers:
      score      mbn_panoptic_i32 alone
      chain      mbn_components_i32 on the labels, on the truth, then the score: what mbn_net_segment_panoptic issues
      torch      torch.unique ((image * P + pred) * (T + 1) + truth + 1, return_counts=True) over the pixels of the predicted segments, the key's
                 construction included: the pair histogram alone, without the match rule (--torch-steps calls per repetition)
    Each figure is the median over the repetitions of `steps` back-to-back calls between two stream marks (torch: two torch events); the runs are
    kept, the spread is (max - min) / median. floor_ms: the two pixel passes read 16 bytes a pixel, over 8 TB/s.
    numpy_ms, once per cell: the download of both segment maps, np.unique of the same keys and the match rule in numpy (pq_from_pairs).
    pq_u64 of the call, of torch's pairs and of numpy's pairs are asserted equal, and every image scored."""
    import time
    pkg = import_package()
    torch = None
    if not a.no_torch:
        import torch
        assert torch.cuda.is_available(), "the yardstick needs torch on the same GPU"
    n, H, W = a.batch, 375, 500
    pix, cap = n * H * W, H * W
    rng = np.random.default_rng(0)
    result = {"batch": n, "pixels": pix, "max_regions": cap, "bytes_per_pixel": 16, "floor_ms": round(1e3 * 16.0 * pix / HBM_BYTES_PER_S, 4)}

    def spread(v):
        return round((max(v) - min(v)) / statistics.median(v), 4)

    with pkg.Context(0) as ctx:
        comps, handle = pkg.Components(ctx, n, pix), pkg.Panoptic(ctx, n, n * cap)
        result["scratch_bytes"] = pkg.panoptic_scratch_bytes(n, n * cap)
        if torch is not None:
            t_comp = [torch.empty((n, H, W), dtype=torch.int32, device="cuda") for _ in range(2)]
            comp_ptr, d_comp = [t.data_ptr() for t in t_comp], None
        else:
            d_comp = [ctx.alloc(4 * pix) for _ in range(2)]
            comp_ptr = [b.ptr for b in d_comp]
        d_reg, d_n = [ctx.alloc(32 * n * cap) for _ in range(2)], [ctx.alloc(4 * n) for _ in range(2)]
        d_scored = ctx.alloc(4 * n)
        for classes in (21, 1000):
            yy, xx = np.mgrid[0:H, 0:W]
            coarse = rng.integers(0, classes, (n, H // 25 + 1, W // 25 + 2))
            shifted = coarse[:, yy // 25, (xx + 23) // 25].astype(np.int32)              # the blocks of the truth, two columns to the right
            noise = rng.random((n, H, W)) < 0.03
            shifted[noise] = rng.integers(0, classes, int(noise.sum()))
            inputs = {"blocks": (shifted, coarse[:, yy // 25, xx // 25 + 1].astype(np.int32)),
                      "random": (rng.integers(0, classes, (n, H, W)).astype(np.int32), rng.integers(0, classes, (n, H, W)).astype(np.int32)),
                      "constant": (np.full((n, H, W), classes - 1, np.int32), np.full((n, H, W), classes - 1, np.int32))}
            d_pq = ctx.alloc(32 * classes)
            for name, maps in inputs.items():
                if a.configs and name not in a.configs.split(","):
                    continue
                d_lab = [ctx.to_device(m) for m in maps]

                def regions(k):
                    ctx.components(comps, d_lab[k].ptr, n, H, W, classes, d_n[k].ptr, comp=comp_ptr[k], regions=d_reg[k].ptr, connectivity=4,
                                   min_area=1, max_regions=cap)

                def score():
                    ctx.panoptic(handle, d_pq.ptr, d_scored.ptr, comp_ptr[0], d_reg[0].ptr, d_n[0].ptr, cap, comp_ptr[1], d_reg[1].ptr, d_n[1].ptr,
                                 cap, n, H, W, classes)

                def chain():
                    regions(0)
                    regions(1)
                    score()

                ctx.lib.mbn_memset(ctx.h, d_pq.ptr, 0, 32 * classes)
                chain()
                ctx.sync()
                ours = d_pq.download((classes, 4), np.uint64)
                assert d_scored.download((n,), np.int32).all(), "every image is scored"
                counts = [b.download((n,), np.int32).astype(np.int64) for b in d_n]
                recs = [b.download((n, cap, 8), np.int32).astype(np.int64) for b in d_reg]

                def keys_to_pq(keys, cnt):
                    g = keys % (cap + 1) - 1
                    ip = keys // (cap + 1)
                    return pq_from_pairs(ip // cap, ip % cap, g, cnt, recs[0], counts[0], recs[1], counts[1], classes)

                out = {"segments_per_map": [round(float(c.mean()), 1) for c in counts], "tp_fp_fn": [int(v) for v in ours[:, :3].sum(0)]}
                if not a.no_host:
                    t0 = time.perf_counter()
                    cp = np.empty((n, H, W), np.int32)
                    ct = np.empty((n, H, W), np.int32)
                    ctx.lib.mbn_download(ctx.h, cp.ctypes.data, comp_ptr[0], cp.nbytes)
                    ctx.lib.mbn_download(ctx.h, ct.ctypes.data, comp_ptr[1], ct.nbytes)
                    image = np.arange(n, dtype=np.int64)[:, None, None]
                    key = ((image * cap + cp) * (cap + 1) + ct + 1)[cp >= 0]
                    keys, cnt = np.unique(key, return_counts=True)
                    host = keys_to_pq(keys, cnt)
                    out["numpy_ms"] = round(1e3 * (time.perf_counter() - t0), 1)
                    assert np.array_equal(host, ours), (classes, name, "numpy")
                ts = []
                if torch is not None:
                    t_image = torch.arange(n, dtype=torch.int64, device="cuda")[:, None, None]

                    def pairs():
                        key = ((t_image * cap + t_comp[0]) * (cap + 1) + t_comp[1] + 1)[t_comp[0] >= 0]
                        return torch.unique(key, return_counts=True)

                    keys, cnt = pairs()
                    torch.cuda.synchronize()
                    assert np.array_equal(keys_to_pq(keys.cpu().numpy(), cnt.cpu().numpy()), ours), (classes, name, "torch")
                    del keys, cnt
                marks_ms(ctx, score, 2)
                marks_ms(ctx, chain, 2)
                ss, cs = [], []
                for _ in range(a.reps):
                    ss.append(marks_ms(ctx, score, a.steps))
                    cs.append(marks_ms(ctx, chain, a.steps))
                    if torch is not None:
                        ctx.sync()
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        for _ in range(a.torch_steps):
                            pairs()
                        e1.record()
                        torch.cuda.synchronize()
                        ts.append(e0.elapsed_time(e1) / a.torch_steps)
                s_ms, c_ms = statistics.median(ss), statistics.median(cs)
                out.update({"score_ms": round(s_ms, 4), "score_runs_ms": [round(v, 4) for v in ss], "score_spread": spread(ss),
                            "share_of_hbm": round(16.0 * pix / (s_ms * 1e-3) / HBM_BYTES_PER_S, 4),
                            "chain_ms": round(c_ms, 4), "chain_runs_ms": [round(v, 4) for v in cs], "chain_spread": spread(cs)})
                if ts:
                    t_ms = statistics.median(ts)
                    out.update({"torch_ms": round(t_ms, 4), "torch_runs_ms": [round(v, 4) for v in ts], "torch_over_score": round(t_ms / s_ms, 1)})
                print("classes %4d %-8s: score %.4f ms (spread %.1f %%, floor %.4f ms, %.1f %% of 8 TB/s)  chain %.4f ms (spread %.1f %%)  torch %s ms  "
                      "numpy %s ms  segments/map %s  tp, fp, fn %s" %
                      (classes, name, s_ms, 100 * out["score_spread"], result["floor_ms"], 100 * out["share_of_hbm"], c_ms, 100 * out["chain_spread"],
                       ("%.4f" % out["torch_ms"]) if ts else "-", out.get("numpy_ms", "-"), out["segments_per_map"], out["tp_fp_fn"]), flush=True)
                result["classes_%d_%s" % (classes, name)] = out
                for b in d_lab:
                    b.free()
            d_pq.free()
        handle.close()
        comps.close()
    print(json.dumps(result))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--configs", default="", help="comma list of configuration names (default: all)")
    ap.add_argument("--no-torch", action="store_true", help="skip the torch yardstick")
    ap.add_argument("--any", action="store_true", help="time mbn_resample_argmax_f32 (the read-out at any output size) instead: see main_any")
    ap.add_argument("--torch-steps", type=int, default=2, help="--any: torch calls per repetition (each writes batch x 1000 x 375 x 500 floats)")
    ap.add_argument("--fit", default="stretch", choices=("stretch", "pad"), help="--any: pad times the window kernel instead: see main_any_pad")
    ap.add_argument("--prob", action="store_true", help="--any: time the softmax read-out beside the argmax read-out instead: see main_prob")
    ap.add_argument("--topk", action="store_true", help="time mbn_resample_topk_f32 beside the softmax and argmax read-outs instead: see main_topk")
    ap.add_argument("--ensemble", default="", help="comma list of view counts: time mbn_resample_ensemble_f32 instead: see main_ensemble")
    ap.add_argument("--slide", action="store_true", help="time mbn_resample_slide_f32 (the sliding-window read-out) instead: see main_slide")
    ap.add_argument("--torch-images", type=int, default=2, help="--slide: the source images the torch yardstick really works on (scaled to the batch)")
    ap.add_argument("--score", action="store_true", help="time mbn_confusion_i32 beside torch.bincount instead: see main_score")
    ap.add_argument("--regions", action="store_true", help="time mbn_components_i32 beside scipy.ndimage.label on the host instead: see main_regions")
    ap.add_argument("--boundary", action="store_true", help="time mbn_boundary_score_i32 beside mbn_confusion_i32, torch and scipy instead: see main_boundary")
    ap.add_argument("--panoptic", action="store_true", help="time mbn_panoptic_i32 beside torch.unique and numpy's pair histogram instead: see main_panoptic")
    ap.add_argument("--host-maps", type=int, default=2, help="--regions, --boundary: the maps the host yardstick really works on (its time is scaled to the batch)")
    ap.add_argument("--no-host", action="store_true", help="--regions, --boundary: skip the host yardstick")
    ap.add_argument("--calibration", action="store_true", help="time mbn_calibration_f32 beside mbn_confusion_i32 and torch instead: see main_calibration")
    ap.add_argument("--surface", action="store_true", help="time mbn_surface_score_i32 beside torch.cdist and scipy's distance transform instead: see main_surface")
    ap.add_argument("--nll", action="store_true", help="time mbn_resample_nll_f32 beside the argmax and softmax read-outs and torch instead: see main_nll")
    a = ap.parse_args()
    if a.nll:
        return main_nll(a)
    if a.calibration:
        return main_calibration(a)
    if a.surface:
        return main_surface(a)
    if a.panoptic:
        return main_panoptic(a)
    if a.boundary:
        return main_boundary(a)
    if a.regions:
        return main_regions(a)
    if a.score:
        return main_score(a)
    if a.ensemble:
        return main_ensemble(a)
    if a.slide:
        return main_slide(a)
    if a.topk:
        return main_topk(a)
    if a.any and a.prob:
        return main_prob(a)
    if a.any:
        return main_any_pad(a) if a.fit == "pad" else main_any(a)
    chosen = [c for c in CONFIGS if not a.configs or c[0] in a.configs.split(",")]
    pkg = import_package()
    torch = None
    if not a.no_torch:
        import torch
        assert torch.cuda.is_available(), "the yardstick needs torch on the same GPU"
    n = a.batch
    result = {}
    with tempfile.TemporaryDirectory() as d, pkg.Context(0) as ctx:
        path = os.path.join(d, "w.h5")
        pkg.synthetic_h5(path, alpha=ALPHA, classes=CLASSES, seed=7)
        imgs = np.random.default_rng(0).uniform(-1, 1, (n, RES, RES, 3)).astype(np.float32)
        d_in = ctx.to_device(imgs)
        d_lab, d_sc = ctx.alloc(n * RES * RES * 4), ctx.alloc(n * RES * RES * 4)
        runs = {}
        for name, dtype, os_ in chosen:
            hw = pkg.HostWeights(path, res=RES, output_stride=os_)
            net = pkg.Net(ctx, hw.plan, hw.blob.copy(), n)
            if dtype == "bf16":
                net.set_dtype(pkg.DT_BF16)
            h = w = RES // os_
            if torch is not None:
                # the yardstick reads the SAME device memory the kernel reads: a torch tensor owns it, the library writes into it
                t_logits = torch.empty((n, h, w, CLASSES), dtype=torch.float32, device="cuda")
                dense_ptr, d_dense = t_logits.data_ptr(), None
            else:
                t_logits, d_dense = None, ctx.alloc(n * h * w * CLASSES * 4)
                dense_ptr = d_dense.ptr
            net.forward_dense(d_in.ptr, dense_ptr, n)
            ctx.sync()
            r = dict(net=net, hw=hw, os=os_, h=h, w=w, dense_ptr=dense_ptr, d_dense=d_dense, t_logits=t_logits, kernel=[], segment=[], torch=[])
            r["run_kernel"] = lambda r=r: ctx.upsample_argmax(d_lab.ptr, d_sc.ptr, r["dense_ptr"], n, r["h"], r["w"], CLASSES, r["os"])
            r["run_segment"] = lambda r=r: r["net"].segment(d_in.ptr, n, d_lab.ptr, d_sc.ptr)
            if torch is not None:
                nchw = t_logits.permute(0, 3, 1, 2)         # a view: the same bytes, channels-last strides
                r["run_torch"] = lambda nchw=nchw: torch.nn.functional.interpolate(nchw, size=(RES, RES), mode="bilinear",
                                                                                   align_corners=False).argmax(1)
            runs[name] = r
            marks_ms(ctx, r["run_kernel"], 3)               # warm-up of every timed shape
            marks_ms(ctx, r["run_segment"], 3)
            if torch is not None:
                for _ in range(3):
                    t_lab = r["run_torch"]()
                torch.cuda.synchronize()
                r["run_kernel"]()
                ctx.sync()
                ours = d_lab.download((n, RES, RES), np.int32)
                r["agree"] = float((ours == t_lab.cpu().numpy()).mean())
                del t_lab
        for _ in range(a.reps):
            for name, r in runs.items():
                r["kernel"].append(marks_ms(ctx, r["run_kernel"], a.steps))
                r["segment"].append(marks_ms(ctx, r["run_segment"], a.steps))
                if torch is not None:
                    ctx.sync()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(a.steps):
                        r["run_torch"]()
                    e1.record()
                    torch.cuda.synchronize()
                    r["torch"].append(e0.elapsed_time(e1) / a.steps)
        for name, r in runs.items():
            k, s = statistics.median(r["kernel"]), statistics.median(r["segment"])
            bytes_, ops = kernel_work(n, r["h"], r["w"], CLASSES, r["os"])
            out = {"batch": n, "kernel_ms": round(k, 4), "segment_ms": round(s, 4), "kernel_runs_ms": [round(x, 4) for x in r["kernel"]],
                   "kernel_bytes": int(bytes_), "kernel_frac_of_8TBps": round(bytes_ / HBM_BYTES_PER_S / (k / 1e3), 4),
                   "kernel_valu_lane_ops": int(ops), "kernel_frac_of_valu_rate": round(ops / VALU_LANE_OPS_PER_S / (k / 1e3), 4),
                   "two_pass_bytes": int(2 * 4.0 * n * CLASSES * RES * RES)}
            if r["torch"]:
                t = statistics.median(r["torch"])
                out.update({"torch_ms": round(t, 4), "torch_runs_ms": [round(x, 4) for x in r["torch"]], "torch_over_kernel": round(t / k, 2),
                            "label_agreement_with_torch": round(r["agree"], 6)})
            result[name] = out
            print("%-10s batch %d  kernel %.4f ms  segment %.4f ms  torch %s ms  (kernel: %.1f %% of 8 TB/s, %.1f %% of the VALU rate)" % (
                name, n, k, s, ("%.4f" % out["torch_ms"]) if r["torch"] else "-", 100 * out["kernel_frac_of_8TBps"],
                100 * out["kernel_frac_of_valu_rate"]), flush=True)
        for r in runs.values():
            r["net"].destroy()
            r["hw"].free()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
