"""Writes tests/golden/resize_pillow_filters.npz: small uint8 images, boxes and the bytes PIL.Image.resize(..., filter, box=box) returns for them under
each of Pillow's six filters (NEAREST, LANCZOS, BILINEAR, BICUBIC, BOX, HAMMING), so that tests/resize_filters_ref.py (and through it the host
tables and the device kernels) stays pinned to Pillow where Pillow is not installed.

    python tests/golden/make_resize_filter_fixtures.py            write the fixture
    python tests/golden/make_resize_filter_fixtures.py --check    regenerate in memory and compare with the committed file (exit status 1 on a difference)

The inputs are seeded, so any Pillow whose 8-bit resize has not changed reproduces the file's arrays exactly. Recorded with Pillow 12.2.0 (the
`pillow_version` entry says what wrote the committed file). Arrays: `names` (the cases), per case `<case>_in` and `<case>_rect`, and per case and
filter `<case>_<filter>` = Pillow's bytes, for the filters in `<case>_filters`."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
PATH = os.path.join(HERE, "resize_pillow_filters.npz")

NEAREST, LANCZOS, BILINEAR, BICUBIC, BOX, HAMMING = 0, 1, 2, 3, 4, 5      # PIL.Image.Resampling's numbers
FILTER_NAMES = {NEAREST: "nearest", LANCZOS: "lanczos", BILINEAR: "bilinear", BICUBIC: "bicubic", BOX: "box", HAMMING: "hamming"}
ALL = (NEAREST, LANCZOS, BILINEAR, BICUBIC, BOX, HAMMING)

# (name, H, W, oh, ow, box (left, upper, right, lower) or None, values: "any" bytes, a constant, or "columns" (a pixel encodes its column), filters)
CASES = [
    ("inexact_box", 37, 53, 16, 24, (0.1, 0.3, 52.7, 36.9), "any", ALL),      # no edge has an exact float32 form
    ("up", 9, 7, 40, 33, None, "any", ALL),
    ("identity", 12, 10, 12, 10, None, "any", ALL),
    ("two_tiles", 80, 150, 35, 70, None, "any", ALL),                          # 70 > 64 columns, 35 > 32 rows: seams on both axes
    ("white", 20, 30, 8, 12, (0.5, 0.25, 29.0, 19.5), 255, ALL),               # weights that do not sum to 2^22 show here, and the clamp
    ("black", 20, 30, 8, 12, (0.5, 0.25, 29.0, 19.5), 0, ALL),
    # the steepest factor of each filter on one axis: 67 taps (bicubic: 65 at 16x; 16.5x has 67 as well)
    ("steep_lanczos", 264, 2, 24, 2, None, "any", (LANCZOS,)),                 # 11x
    ("steep_bicubic", 384, 2, 24, 2, None, "any", (BICUBIC,)),                 # 16x
    ("steep_bicubic_67", 396, 2, 24, 2, None, "any", (BICUBIC,)),              # 16.5x
    ("steep_33x", 792, 2, 24, 2, None, "any", (BILINEAR, HAMMING)),            # 33x
    ("steep_box", 1584, 2, 24, 2, None, "any", (BOX,)),                        # 66x
    # NEAREST accumulates xo: the closed form b0 + a * (i + 0.5) gives other columns here
    ("nearest_504", 3, 504, 3, 188, None, "columns", (NEAREST,)),
    ("nearest_1222", 3, 1222, 3, 65, None, "columns", (NEAREST,)),
]


def image(case_index, h, w, values):
    if values == "columns":                                   # pixel (y, x) = (x & 255, x >> 8, y): the bytes say which column was taken
        img = np.zeros((h, w, 3), np.uint8)
        img[:, :, 0] = (np.arange(w) & 255)[None, :]
        img[:, :, 1] = (np.arange(w) >> 8)[None, :]
        img[:, :, 2] = np.arange(h)[:, None]
        return img
    if values != "any":
        return np.full((h, w, 3), values, np.uint8)
    return np.random.default_rng(2000 + case_index).integers(0, 256, (h, w, 3), dtype=np.uint8)


def box_f32(h, w, box):
    return np.array(box if box is not None else (0.0, 0.0, w, h), np.float32)


def pillow_resize(filt, img, oh, ow, box):
    from PIL import Image
    b = tuple(float(v) for v in np.asarray(box, np.float32))               # the float32 values, exactly, as Python floats
    return np.asarray(Image.fromarray(img).resize((ow, oh), Image.Resampling(filt), box=b))


def generate():
    import PIL
    out = {"pillow_version": np.array(PIL.__version__), "names": np.array([c[0] for c in CASES])}
    for i, (name, h, w, oh, ow, box, values, filters) in enumerate(CASES):
        img, b = image(i, h, w, values), box_f32(h, w, box)
        out[name + "_in"] = img
        out[name + "_rect"] = b
        out[name + "_filters"] = np.array(filters, np.int32)
        for f in filters:
            out[name + "_" + FILTER_NAMES[f]] = pillow_resize(f, img, oh, ow, b)
            assert out[name + "_" + FILTER_NAMES[f]].shape == (oh, ow, 3)
    return out


if __name__ == "__main__":
    fresh = generate()
    if "--check" in sys.argv:
        old = np.load(PATH)
        keys = [k for k in fresh if k != "pillow_version"]
        bad = [k for k in keys if k not in old.files or not np.array_equal(old[k], fresh[k])]
        print("Pillow %s against the file written by Pillow %s: %s" % (fresh["pillow_version"], old["pillow_version"],
                                                                        "identical" if not bad else "DIFFERENT: %s" % bad))
        sys.exit(1 if bad else 0)
    np.savez_compressed(PATH, **fresh)
    print("%s: %d bytes, Pillow %s" % (PATH, os.path.getsize(PATH), fresh["pillow_version"]))
