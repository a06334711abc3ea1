"""Writes tests/golden/resize_pillow_pad.npz: small uint8 images and the canvases PIL.ImageOps.pad(image, (ow, oh), filter, color=fill) returns for them
(centering (0.5, 0.5), Pillow's default) under each of Pillow's six filters, so that the letterbox of the resize front-end (mbn_fit_pad,
mbn_resizer_create_pad, mbn_ragged_resizer_create_pad; include/mbn.h) stays pinned to Pillow where Pillow is not installed.

    python tests/golden/make_resize_pad_fixtures.py            write the fixture
    python tests/golden/make_resize_pad_fixtures.py --check    regenerate in memory and compare with the committed file (exit status 1 on a difference)

The inputs are seeded, so any Pillow whose ImageOps.pad and 8-bit resize have not changed reproduces the file's arrays exactly. Recorded with Pillow
12.2.0 (the `pillow_version` entry says what wrote the committed file). Arrays: `names` (the cases), `fill` (the colour of the coloured canvases), per
case `<case>_in`, `<case>_canvas` = (oh, ow) and `<case>_rect` = (x, y, iw, ih), the rectangle Pillow itself pasted into (read back from its canvas
sizes, not from the rule under test), per case and filter `<case>_<filter>` = Pillow's bytes with `fill`, and `<case>_black` = Pillow's bytes under
BILINEAR with the default colour."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
PATH = os.path.join(HERE, "resize_pillow_pad.npz")

NEAREST, LANCZOS, BILINEAR, BICUBIC, BOX, HAMMING = 0, 1, 2, 3, 4, 5      # PIL.Image.Resampling's numbers
FILTER_NAMES = {NEAREST: "nearest", LANCZOS: "lanczos", BILINEAR: "bilinear", BICUBIC: "bicubic", BOX: "box", HAMMING: "hamming"}
ALL = (NEAREST, LANCZOS, BILINEAR, BICUBIC, BOX, HAMMING)
FILL = (128, 7, 255)

# (H, W, oh, ow)
GEOMETRIES = [(45, 60, 28, 28), (60, 45, 28, 28), (37, 50, 32, 48), (50, 37, 32, 48),
              (31, 97, 64, 96),                       # top / bottom borders of a canvas with two column tiles
              (97, 31, 64, 96),                       # x = 38: the rectangle starts 2 bytes past a dword in every row
              (64, 96, 64, 96),                       # the canvas's own size: no border, the identity
              (128, 192, 64, 96),                     # the canvas's aspect ratio: no border
              (33, 100, 32, 32),                      # ih = 11, y = round(10.5) = 10: half to even
              (100, 3, 32, 32),                       # iw = 1
              (7, 5, 32, 64)]                         # an upscale


def name_of(g):
    return "%dx%d_to_%dx%d" % g


def image(index, h, w):
    """Seeded bytes. The two sources of the canvas's aspect ratio are random colours in 4 x 4 blocks: their canvases have no border to compress, and
    seven copies of 18 KB of noise each would be most of the file"""
    rng = np.random.default_rng(3000 + index)
    if (h, w) in ((64, 96), (128, 192)):
        return np.repeat(np.repeat(rng.integers(0, 256, (h // 4, w // 4, 3), dtype=np.uint8), 4, axis=0), 4, axis=1)
    return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)


def pillow_pad(filt, img, oh, ow, fill):
    from PIL import Image, ImageOps
    kw = {} if fill is None else {"color": tuple(fill)}
    return np.asarray(ImageOps.pad(Image.fromarray(img), (ow, oh), Image.Resampling(filt), **kw))


def pillow_rect(img, oh, ow):
    """where Pillow pastes: the size ImageOps.contain gives, and the offset ImageOps.pad computes for it"""
    from PIL import Image, ImageOps
    iw, ih = ImageOps.contain(Image.fromarray(img), (ow, oh)).size
    x = round((ow - iw) * 0.5) if iw != ow else 0
    y = round((oh - ih) * 0.5) if iw == ow and ih != oh else 0
    return np.array((x, y, iw, ih), np.int32)


def generate():
    import PIL
    out = {"pillow_version": np.array(PIL.__version__), "names": np.array([name_of(g) for g in GEOMETRIES]), "fill": np.array(FILL, np.uint8)}
    for i, g in enumerate(GEOMETRIES):
        h, w, oh, ow = g
        name, img = name_of(g), image(i, h, w)
        out[name + "_in"] = img
        out[name + "_canvas"] = np.array((oh, ow), np.int32)
        out[name + "_rect"] = pillow_rect(img, oh, ow)
        for f in ALL:
            out[name + "_" + FILTER_NAMES[f]] = pillow_pad(f, img, oh, ow, FILL)
            assert out[name + "_" + FILTER_NAMES[f]].shape == (oh, ow, 3)
        out[name + "_black"] = pillow_pad(BILINEAR, img, oh, ow, None)
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
