"""The resize front-end (mbn_resize_u8, under any of Pillow's filters) against torch-ROCm's antialiased interpolate and against the forward it precedes, in one process.

  python tools/resize_bench.py [--reps 7] [--steps 20] [--configs photo_b256,identity_b256] [--no-torch] [--no-forward]
      Geometries (uint8 HWC sources, random bytes):
        photo_b256 / photo_b512   375 x 500 -> 224 x 224, fit CROP with crop fraction 0.875, batch 256 / 512
        hd_b64                    1080 x 1920 -> 224 x 224, fit CROP (the centred 1080 x 1080 box), batch 64
        identity_b256             224 x 224 -> 224 x 224, the whole image, batch 256
      Per geometry, alternating within every repetition:
        kernel   mbn_resize_u8 on a torch-owned device buffer, ms per call
        torch    the yardstick, not the code under test: on the SAME device buffer, the box's integer hull cut out as a view, then
                 F.interpolate(x.float(), size, mode="bilinear", antialias=True). Its arithmetic differs (float, integer crop): a time
                 comparison only, ms per call
      Each figure is the median over the repetitions of `steps` back-to-back calls between two stream marks (torch: two torch events on its own
      stream, synchronised). What the kernel's time means: the bytes it has to move — every source byte inside the rows and columns the tap
      tables reach, once, plus the output — over 8 TB/s. Then the forward the resize precedes (1.0x224, uint8 input): fp32 at batch 256 and bf16
      at batch 512, and the resize's share of it. The kernel's output is compared once with tests/resize_ref.py on image 0 (agreement, not timing).
      One JSON object at the end. No GPU: the Context raises; nothing falls back.
      --filter LIST: comma list of nearest, box, bilinear (the default), hamming, bicubic, lanczos, or `all`. Every geometry runs once per filter, all
      of them alternating within every repetition; the entries are named <geometry>:<filter> (the bilinear ones keep the bare name) and carry the
      taps per axis. The kernel's bytes are compared with tests/resize_filters_ref.py; the torch yardstick is mode="bicubic" under bicubic and
      lanczos, "nearest" under nearest, "bilinear" with antialias otherwise.
      --fit LIST: comma list of crop, stretch, pad: every geometry runs once per fit (crop with the geometry's own fraction) instead of its own fit, all
      alternating within every repetition; the entries are named <geometry>/<fit>. pad is the letterbox (mbn_resizer_create_pad, black border),
      compared with the rule + tests/resize_filters_ref.py; it has no torch yardstick.

  python tools/resize_bench.py --ragged [--seed 1] [--batch 256] [--reps 7] [--steps 20]
      The ragged resize (mbn_resize_ragged_u8) on a seeded batch of images of DIFFERENT sizes: rows 300-600, cols 300-700, each through its crop-0.875
      box to 224 x 224; the batch is built once and its seed printed. Two comparisons, the forms alternating within every repetition:
        mixed    the batch one image at a time, mbn_resize_u8 at batch 1 with one resizer per image built beforehand and NOT timed (the best case of
                 doing without the ragged launch); the same including the builds (create, launch, destroy per image: what mbn_net_resize_input pays
                 when every image has another size); and the ragged way, set + ONE launch
        uniform  `batch` x 375 x 500: mbn_resize_u8 (tables from the host) against the ragged launch alone and with its set: the price of forming the
                 taps on the device and of the descriptor lookup
      Every figure is a host clock around `steps` calls that end in a device synchronise, in ms per batch: median over the repetitions and their
      range. The ragged output of both batches is compared once with the table kernel's bytes, image by image (agreement, not timing).
      --filter NAME: one of nearest, box, bilinear (the default), bicubic, for the ragged and the table resizers alike.

  python tools/resize_bench.py --ragged --fit pad,stretch [--seed 1] [--batch 256] [--reps 7] [--steps 20] [--filter NAME]
      The same mixed batch under each fit of the list (crop: fraction 0.875; pad: mbn_ragged_resizer_create_pad, black border), one ragged handle per
      fit, the fits alternating within every repetition: set + launch, and the launch alone. Image 0 of every fit is compared with the reference.
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
from mbn_amd import import_package  # noqa: E402

RES = 224
HBM_BYTES_PER_S = 8.0e12                    # spec
# (name, H, W, fit, crop fraction, batch, the forward it is compared with)
CONFIGS = [("photo_b256", 375, 500, "crop", 0.875, 256, "f32_b256"), ("photo_b512", 375, 500, "crop", 0.875, 512, "bf16_b512"),
           ("hd_b64", 1080, 1920, "crop", 1.0, 64, None), ("identity_b256", 224, 224, "stretch", 1.0, 256, "f32_b256")]
FORWARDS = {"f32_b256": ("f32", 256), "bf16_b512": ("bf16", 512)}


def window(pkg, in_size, b0, b1, out_size, filt):
    """[lo, hi): the source positions the tap tables of an axis reach, and its taps per output"""
    first, count, w = pkg.resize_taps(in_size, float(b0), float(b1), out_size, filter=filt)
    return int(first[0]), int(first[-1] + count[-1]), int(w.shape[1])


def marks_ms(ctx, fn, steps):
    ctx.mark()
    for _ in range(steps):
        fn()
    ctx.mark()
    return sum(ctx.marks_read(4)) / steps


def wall_ms(ctx, fn, steps):
    """ms per call of fn: a host clock around `steps` calls and the synchronise behind them"""
    import time
    ctx.sync()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    ctx.sync()
    return (time.perf_counter() - t0) * 1e3 / steps


def figure(runs):
    return {"median_ms": round(statistics.median(runs), 4), "min_ms": round(min(runs), 4), "max_ms": round(max(runs), 4), "runs_ms": [round(x, 4) for x in runs]}


def canvas_ref(pkg, filt, img, fit, frac):
    """image 0's reference bytes under a fit: tests/resize_filters_ref.py on the fit's box, or into the letterbox's rectangle of a black canvas"""
    import resize_filters_ref
    H, W = img.shape[:2]
    if fit != "pad":
        return resize_filters_ref.resize(filt, img, RES, RES, pkg.fit_box(H, W, RES, RES, pkg.FIT_CROP if fit == "crop" else pkg.FIT_STRETCH, frac))
    x, y, iw, ih = pkg.fit_pad(H, W, RES, RES)
    out = np.zeros((RES, RES, 3), np.uint8)
    out[y:y + ih, x:x + iw] = resize_filters_ref.resize(filt, img, ih, iw)
    return out


def ragged_fit_main(a):
    """--ragged --fit LIST: the mixed batch under each fit, alternating"""
    pkg = import_package()
    import torch
    assert torch.cuda.is_available(), "the buffers are torch tensors on the same GPU"
    fits = a.fit.split(",")
    assert all(f in ("crop", "stretch", "pad") for f in fits), "--fit: unknown name in %r" % a.fit
    rng = np.random.default_rng(a.seed)
    n = a.batch
    filt = pkg.FILTER_NAMES[a.filter or "bilinear"]
    sizes = [(int(rng.integers(300, 601)), int(rng.integers(300, 701))) for _ in range(n)]
    print("ragged: seed %d, batch %d, rows 300-600 x cols 300-700 -> %d x %d, fits %s, filter %s" % (a.seed, n, RES, RES, a.fit, a.filter or "bilinear"), flush=True)
    result = {"seed": a.seed, "batch": n, "steps": a.steps, "reps": a.reps, "filter": a.filter or "bilinear"}
    with pkg.Context(0) as ctx:
        offs = np.concatenate([[0], np.cumsum([h * w * 3 for h, w in sizes])]).astype(np.int64)
        t_src = torch.randint(0, 256, (int(offs[-1]),), dtype=torch.uint8, device="cuda")
        t_out = torch.zeros((n, RES, RES, 3), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        img0 = t_src[:sizes[0][0] * sizes[0][1] * 3].cpu().numpy().reshape(sizes[0] + (3,))
        forms, keep = {}, []
        for fit in fits:
            code = {"crop": pkg.FIT_CROP, "stretch": pkg.FIT_STRETCH, "pad": pkg.FIT_PAD}[fit]
            items = pkg.resize_items([(int(o), h, w, pkg.fit_box(h, w, RES, RES, code, 0.875)) for o, (h, w) in zip(offs, sizes)])
            rr = pkg.RaggedResizer(ctx, n, RES, RES, filter=filt, pad=(0, 0, 0) if fit == "pad" else None)
            keep.append(rr)

            def set_and_launch(rr=rr, items=items):
                rr.set(items)
                rr.run(t_out.data_ptr(), t_src.data_ptr())

            set_and_launch()
            ctx.sync()
            differ = int((t_out[0].cpu().numpy() != canvas_ref(pkg, filt, img0, fit, 0.875)).sum())
            forms[fit] = dict(f={"set_and_launch": set_and_launch, "launch_alone": lambda rr=rr: rr.run(t_out.data_ptr(), t_src.data_ptr())},
                              runs={"set_and_launch": [], "launch_alone": []}, differ=differ)
        for _ in range(a.reps):
            for fit, r in forms.items():
                for k, fn in r["f"].items():               # the set of set_and_launch stays for the launch alone
                    r["runs"][k].append(wall_ms(ctx, fn, a.steps))
        for fit, r in forms.items():
            out = {k: figure(v) for k, v in r["runs"].items()}
            out["bytes_differ_from_ref_image0"] = r["differ"]
            result[fit] = out
            print("%-8s %s  differing bytes %d" % (fit, "  ".join("%s %.4f ms (%.4f-%.4f)" % (k, out[k]["median_ms"], out[k]["min_ms"], out[k]["max_ms"])
                                                                    for k in r["runs"]), r["differ"]), flush=True)
        for rr in keep:
            rr.close()
    print(json.dumps(result))


def ragged_main(a):
    if a.fit:
        return ragged_fit_main(a)
    pkg = import_package()
    import torch
    assert torch.cuda.is_available(), "the buffers are torch tensors on the same GPU"
    rng = np.random.default_rng(a.seed)
    n = a.batch
    filt = pkg.FILTER_NAMES[a.filter or "bilinear"]
    print("ragged: seed %d, batch %d, rows 300-600 x cols 300-700 -> %d x %d, crop 0.875, filter %s" % (a.seed, n, RES, RES, a.filter or "bilinear"), flush=True)
    batches = {"mixed": [(int(rng.integers(300, 601)), int(rng.integers(300, 701))) for _ in range(n)], "uniform": [(375, 500)] * n}
    result = {"seed": a.seed, "batch": n, "steps": a.steps, "reps": a.reps, "filter": a.filter or "bilinear"}
    with pkg.Context(0) as ctx:
        forms = {}
        for name, sizes in batches.items():
            offs = np.concatenate([[0], np.cumsum([h * w * 3 for h, w in sizes])]).astype(np.int64)
            t_src = torch.randint(0, 256, (int(offs[-1]),), dtype=torch.uint8, device="cuda")
            t_one, t_rag = (torch.zeros((n, RES, RES, 3), dtype=torch.uint8, device="cuda") for _ in range(2))
            torch.cuda.synchronize()
            boxes = [pkg.fit_box(h, w, RES, RES, pkg.FIT_CROP, 0.875) for h, w in sizes]
            items = pkg.resize_items([(int(o), h, w, b) for o, (h, w), b in zip(offs, sizes, boxes)])
            src, one, rag, img = t_src.data_ptr(), t_one.data_ptr(), t_rag.data_ptr(), RES * RES * 3
            rr = pkg.RaggedResizer(ctx, n, RES, RES, filter=filt)

            def ragged(rr=rr, items=items, rag=rag, src=src):
                rr.set(items)
                rr.run(rag, src)

            def with_builds(sizes=sizes, boxes=boxes, offs=offs, one=one, src=src):
                for i, ((h, w), b) in enumerate(zip(sizes, boxes)):
                    rz = pkg.Resizer(ctx, h, w, RES, RES, b, filter=filt)
                    rz.run(one + i * img, src + int(offs[i]), 1)
                    rz.close()

            f = {"ragged_set_and_launch": ragged}
            if name == "mixed":
                built = [pkg.Resizer(ctx, h, w, RES, RES, b, filter=filt) for (h, w), b in zip(sizes, boxes)]
                f["one_by_one_prebuilt"] = lambda built=built, offs=offs, one=one, src=src: [rz.run(one + i * img, src + int(offs[i]), 1) for i, rz in enumerate(built)]
                f["one_by_one_with_builds"] = with_builds
            else:
                built = [pkg.Resizer(ctx, 375, 500, RES, RES, boxes[0], filter=filt)]
                f["table_kernel"] = lambda rz=built[0], one=one, src=src: rz.run(one, src, n)
                f["ragged_launch_alone"] = lambda rr=rr, rag=rag, src=src: rr.run(rag, src)
            for fn in f.values():                           # warm-up of every timed form; the last ragged set stays for the launch alone
                fn()
            ragged()
            f[next(k for k in f if k != "ragged_set_and_launch")]()
            ctx.sync()
            differ = int((t_one != t_rag).sum().item())
            forms[name] = dict(f=f, runs={k: [] for k in f}, differ=differ, keep=(t_src, t_one, t_rag, built, rr), src_bytes=int(offs[-1]))
        for _ in range(a.reps):
            for name, r in forms.items():
                for k, fn in r["f"].items():
                    steps = max(1, a.steps // 10) if k == "one_by_one_with_builds" else a.steps
                    r["runs"][k].append(wall_ms(ctx, fn, steps))
        for name, r in forms.items():
            out = {k: figure(v) for k, v in r["runs"].items()}
            out["bytes_differ_from_table_kernel"] = r["differ"]
            out["src_bytes"] = r["src_bytes"]
            med = {k: v["median_ms"] for k, v in out.items() if isinstance(v, dict)}
            if name == "mixed":
                out["prebuilt_over_ragged"] = round(med["one_by_one_prebuilt"] / med["ragged_set_and_launch"], 2)
                out["with_builds_over_ragged"] = round(med["one_by_one_with_builds"] / med["ragged_set_and_launch"], 2)
            else:
                out["ragged_launch_over_table"] = round(med["ragged_launch_alone"] / med["table_kernel"], 3)
            result[name] = out
            print("%-8s %s  differing bytes %d" % (name, "  ".join("%s %.4f ms (%.4f-%.4f)" % (k, out[k]["median_ms"], out[k]["min_ms"], out[k]["max_ms"])
                                                                    for k in r["runs"]), r["differ"]), flush=True)
            for rz in r["keep"][3]:
                rz.close()
            r["keep"][4].close()
    print(json.dumps(result))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--configs", default="", help="comma list of geometry names (default: all)")
    ap.add_argument("--no-torch", action="store_true", help="skip the torch yardstick")
    ap.add_argument("--no-forward", action="store_true", help="skip the forwards the resize is compared with")
    ap.add_argument("--ragged", action="store_true", help="the ragged resize against one launch per image and against the table kernel")
    ap.add_argument("--seed", type=int, default=1, help="--ragged: seed of the batch's size list")
    ap.add_argument("--batch", type=int, default=256, help="--ragged: images per batch")
    ap.add_argument("--filter", default="", help="comma list of Pillow filter names, or all (--ragged: one name); default bilinear")
    ap.add_argument("--fit", default="", help="comma list of crop, stretch, pad: every geometry (--ragged: the mixed batch) under each of them")
    a = ap.parse_args()
    if a.ragged:
        return ragged_main(a)
    chosen = [c for c in CONFIGS if not a.configs or c[0] in a.configs.split(",")]
    pkg = import_package()
    import resize_filters_ref
    import torch
    assert torch.cuda.is_available(), "the buffers are torch tensors on the same GPU"
    F = torch.nn.functional
    result = {}
    with tempfile.TemporaryDirectory() as d, pkg.Context(0) as ctx:
        runs = {}
        names = [f for f in ("nearest", "box", "bilinear", "hamming", "bicubic", "lanczos") if a.filter == "all" or f in (a.filter or "bilinear").split(",")]
        assert names and (a.filter in ("", "all") or len(names) == len(a.filter.split(","))), "--filter: unknown name in %r" % a.filter
        assert all(f in ("crop", "stretch", "pad") for f in a.fit.split(",") if f), "--fit: unknown name in %r" % a.fit
        if a.fit:
            chosen = [(c[0] + "/" + f, c[1], c[2], f) + c[4:] for c in chosen for f in a.fit.split(",")]
        for name, H, W, fit, frac, n, fwd, fname in [c + (f,) for c in chosen for f in names]:
            filt = pkg.FILTER_NAMES[fname]
            name = name if fname == "bilinear" else "%s:%s" % (name, fname)
            box = pkg.fit_box(H, W, RES, RES, {"crop": pkg.FIT_CROP, "stretch": pkg.FIT_STRETCH, "pad": pkg.FIT_PAD}[fit], frac)
            x0, x1, kx = window(pkg, W, box[0], box[2], RES, filt)
            y0, y1, ky = window(pkg, H, box[1], box[3], RES, filt)
            t_src = torch.randint(0, 256, (n, H, W, 3), dtype=torch.uint8, device="cuda")       # the library reads what torch owns
            t_out = torch.zeros((n, RES, RES, 3), dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            rz = pkg.Resizer(ctx, H, W, RES, RES, filter=filt, pad=(0, 0, 0)) if fit == "pad" else pkg.Resizer(ctx, H, W, RES, RES, box, filter=filt)
            r = dict(rz=rz, n=n, fwd=fwd, filter=fname, kx=kx, ky=ky, t_src=t_src, t_out=t_out, kernel=[], torch=[],
                     bytes=3.0 * n * ((y1 - y0) * (x1 - x0) + RES * RES), box=[float(v) for v in box])
            r["run_kernel"] = lambda r=r: r["rz"].run(r["t_out"].data_ptr(), r["t_src"].data_ptr(), r["n"])
            hull = t_src[:, int(np.floor(box[1])):int(np.ceil(box[3])), int(np.floor(box[0])):int(np.ceil(box[2])), :].permute(0, 3, 1, 2)
            mode = {"bicubic": "bicubic", "lanczos": "bicubic", "nearest": "nearest"}.get(fname, "bilinear")
            r["run_torch"] = ((lambda hull=hull: F.interpolate(hull.float(), size=(RES, RES), mode="nearest")) if mode == "nearest" else
                              (lambda hull=hull, mode=mode: F.interpolate(hull.float(), size=(RES, RES), mode=mode, antialias=True)))
            r["torch_mode"] = mode
            marks_ms(ctx, r["run_kernel"], 3)               # warm-up of every timed shape
            ctx.sync()
            want = canvas_ref(pkg, filt, t_src[0].cpu().numpy(), fit, frac)
            r["bytes_differ_from_ref"] = int((t_out[0].cpu().numpy() != want).sum())
            r["has_torch"] = not a.no_torch and fit != "pad"
            if r["has_torch"]:
                for _ in range(3):
                    r["run_torch"]()
                torch.cuda.synchronize()
            runs[name] = r
        for _ in range(a.reps):
            for name, r in runs.items():
                r["kernel"].append(marks_ms(ctx, r["run_kernel"], a.steps))
                if r["has_torch"]:
                    ctx.sync()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(a.steps):
                        r["run_torch"]()
                    e1.record()
                    torch.cuda.synchronize()
                    r["torch"].append(e0.elapsed_time(e1) / a.steps)
        forward_ms = {}
        if not a.no_forward:
            path = os.path.join(d, "w.h5")
            pkg.synthetic_h5(path, alpha=1.0, classes=1000, seed=7)
            for key in sorted(set(r["fwd"] for r in runs.values() if r["fwd"])):
                dtype, n = FORWARDS[key]
                hw = pkg.HostWeights(path, res=RES)
                net = pkg.Net(ctx, hw.plan, hw.blob.copy(), n)
                if dtype == "bf16":
                    net.set_dtype(pkg.DT_BF16)
                net.set_input_u8(True)
                t_img = torch.randint(0, 256, (n, RES, RES, 3), dtype=torch.uint8, device="cuda")
                torch.cuda.synchronize()
                d_logits = ctx.alloc(n * 1000 * 4)
                run = lambda: net.forward(t_img.data_ptr(), d_logits.ptr, n)
                marks_ms(ctx, run, 3)
                forward_ms[key] = statistics.median(marks_ms(ctx, run, a.steps) for _ in range(a.reps))
                ctx.sync()
                net.destroy()
                hw.free()
                d_logits.free()
        for name, r in runs.items():
            k = statistics.median(r["kernel"])
            out = {"batch": r["n"], "box": r["box"], "filter": r["filter"], "kx": r["kx"], "ky": r["ky"], "kernel_ms": round(k, 4), "kernel_runs_ms": [round(x, 4) for x in r["kernel"]],
                   "kernel_bytes": int(r["bytes"]), "kernel_frac_of_8TBps": round(r["bytes"] / HBM_BYTES_PER_S / (k / 1e3), 4),
                   "bytes_differ_from_ref_image0": r["bytes_differ_from_ref"]}
            if r["torch"]:
                t = statistics.median(r["torch"])
                out.update({"torch_mode": r["torch_mode"], "torch_ms": round(t, 4), "torch_runs_ms": [round(x, 4) for x in r["torch"]], "torch_over_kernel": round(t / k, 2)})
            if r["fwd"] in forward_ms:
                out.update({"forward": r["fwd"], "forward_ms": round(forward_ms[r["fwd"]], 4), "kernel_over_forward": round(k / forward_ms[r["fwd"]], 4)})
            result[name] = out
            print("%-22s batch %3d  kernel %.4f ms (%.1f %% of 8 TB/s)  torch %s ms  forward %s ms" % (
                name, r["n"], k, 100 * out["kernel_frac_of_8TBps"], ("%.4f" % out["torch_ms"]) if r["torch"] else "-",
                ("%.4f (%s)" % (out["forward_ms"], r["fwd"])) if "forward_ms" in out else "-"), flush=True)
            r["rz"].close()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
