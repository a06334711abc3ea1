"""Writes tests/golden/resize_pillow.npz: small uint8 images, boxes and the bytes PIL.Image.resize(..., Image.BILINEAR, box=box) returns for them,
so that tests/resize_ref.py (and through it the device kernel) stays pinned to Pillow where Pillow is not installed.

    python tests/golden/make_resize_fixtures.py            write the fixture
    python tests/golden/make_resize_fixtures.py --check    regenerate in memory and compare with the committed file (exit status 1 on a difference)

The inputs are seeded, so any Pillow whose 8-bit bilinear resize has not changed reproduces the file's arrays exactly (the container's zip
timestamps differ). Recorded with Pillow 12.2.0 (the `pillow_version` entry says what wrote the committed file)."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
PATH = os.path.join(HERE, "resize_pillow.npz")

# (name, H, W, oh, ow, box (left, upper, right, lower) or None, values: "any" bytes or only "extreme" 0 / 255)
CASES = [
    ("down", 37, 53, 32, 32, None, "any"),
    ("up", 20, 30, 64, 96, None, "any"),                                   # one-tap borders
    ("fractional_box", 33, 47, 32, 64, (3.5, 2.25, 40.0, 30.75), "extreme"),
    ("identity", 24, 24, 24, 24, None, "any"),                             # weights (2^22, 0) on both axes
    ("vertical_only", 32, 48, 16, 48, None, "any"),
    ("horizontal_only", 32, 48, 32, 16, None, "extreme"),
    ("one_pixel", 1, 1, 5, 7, None, "any"),
    ("down_31x", 310, 9, 10, 12, None, "any"),                             # 65 vertical taps, horizontal upscale
    ("inexact_box", 53, 41, 32, 20, (0.1, 0.3, 40.7, 52.9), "extreme"),    # no edge has an exact float32 form
    ("crop_0875", 45, 60, 28, 28, (10.3125, 2.8125, 49.6875, 42.1875), "any"),   # fit_box(45, 60, 28, 28, CROP, 0.875)
]


def image(case_index, h, w, values):
    rng = np.random.default_rng(1000 + case_index)
    if values == "extreme":
        return (rng.integers(0, 2, (h, w, 3)) * 255).astype(np.uint8)
    return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)


def box_f32(h, w, box):
    return np.array(box if box is not None else (0.0, 0.0, w, h), np.float32)


def pillow_resize(img, oh, ow, box):
    from PIL import Image
    b = tuple(float(v) for v in np.asarray(box, np.float32))               # the float32 values, exactly, as Python floats
    return np.asarray(Image.fromarray(img).resize((ow, oh), Image.BILINEAR, box=b))


def generate():
    import PIL
    out = {"pillow_version": np.array(PIL.__version__), "names": np.array([c[0] for c in CASES])}
    for i, (name, h, w, oh, ow, box, values) in enumerate(CASES):
        img, b = image(i, h, w, values), box_f32(h, w, box)
        out[name + "_in"] = img
        out[name + "_box"] = b
        out[name + "_out"] = pillow_resize(img, oh, ow, b)
        assert out[name + "_out"].shape == (oh, ow, 3) and oh <= 64 and ow <= 96
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
    np.savez(PATH, **fresh)
    print("%s: %d bytes, Pillow %s" % (PATH, os.path.getsize(PATH), fresh["pillow_version"]))
