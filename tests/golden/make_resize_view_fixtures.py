"""Writes tests/golden/resize_pillow_views.npz: small uint8 images and the canvases Pillow gives for a VIEW of them (include/mbn.h, mbn_view,
mbn_fit_view, mbn_resizer_create_view): the whole image resized to iw x ih under each of Pillow's six filters, mirrored left-to-right or not,
pasted at (x, y) of an ow x oh canvas of one colour, so that the view resizer stays pinned to Pillow where Pillow is not installed.

    python tests/golden/make_resize_view_fixtures.py            write the fixture
    python tests/golden/make_resize_view_fixtures.py --check    regenerate in memory and compare with the committed file (exit status 1 on a difference)

The expected canvas is built by the explicit steps
    canvas = Image.new("RGB", (ow, oh), fill); inner = im.resize((iw, ih), filter)
    inner = inner.transpose(FLIP_LEFT_RIGHT) if mirror; canvas.paste(inner, (x, y))
and the generator asserts on the spot that an unmirrored view at scale 1 is ImageOps.pad's canvas byte for byte. A scaled view's rectangle is read
from Pillow (ImageOps.contain of the scaled canvas and ImageOps.pad's offsets, moved by the scaled canvas's own offset), not from the rule under
test. The inputs are seeded, so any Pillow whose 8-bit resize has not changed reproduces the arrays exactly. Recorded with Pillow 12.2.0 (the
`pillow_version` entry says what wrote the committed file). Arrays: `names`, `fill`, per case `<case>_in`, `<case>_canvas` = (oh, ow),
`<case>_view` = (x, y, iw, ih, mirror), `<case>_scale` (float32; 0 for a rectangle given outright) and per filter `<case>_<filter>`."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
PATH = os.path.join(HERE, "resize_pillow_views.npz")

NEAREST, LANCZOS, BILINEAR, BICUBIC, BOX, HAMMING = 0, 1, 2, 3, 4, 5      # PIL.Image.Resampling's numbers
FILTER_NAMES = {NEAREST: "nearest", LANCZOS: "lanczos", BILINEAR: "bilinear", BICUBIC: "bicubic", BOX: "box", HAMMING: "hamming"}
ALL = (NEAREST, LANCZOS, BILINEAR, BICUBIC, BOX, HAMMING)
FILL = (128, 7, 255)
SCALES = (1.0, 0.75, 0.5)

# the scaled views: (H, W, oh, ow), each at SCALES x mirror 0 / 1
SCALED = [(45, 60, 64, 96), (60, 45, 64, 96)]
# rectangles given outright: (name, H, W, oh, ow, (x, y, iw, ih)), each at mirror 0 / 1
EXPLICIT = [("four_borders_odd_x", 33, 40, 48, 64, (7, 5, 41, 30)),       # borders on all four sides, x odd: a row of the rectangle starts off a dword
            ("one_column", 40, 9, 32, 32, (10, 3, 1, 20)),                 # iw = 1
            ("upscale", 7, 5, 32, 32, (3, 2, 20, 28))]


def image(index, h, w):
    """Seeded bytes: random colours of four levels in 6 x 6 blocks. Inside a block every filter reproduces the colour, at the blocks' edges (a third
    of the pixels) it mixes neighbours into most byte values: the taps are still pinned, and the 108 canvases stay under 200 KB"""
    rng = np.random.default_rng(4000 + index)
    blocks = rng.integers(0, 4, ((h + 5) // 6, (w + 5) // 6, 3), dtype=np.uint8) * 85
    return np.ascontiguousarray(np.repeat(np.repeat(blocks, 6, axis=0), 6, axis=1)[:h, :w])


def pillow_view(filt, img, oh, ow, view, fill):
    from PIL import Image
    x, y, iw, ih, mirror = (int(v) for v in view)
    canvas = Image.new("RGB", (ow, oh), tuple(fill))
    inner = Image.fromarray(img).resize((iw, ih), Image.Resampling(filt))
    if mirror:
        inner = inner.transpose(Image.Transpose.FLIP_LEFT_RIGHT)
    canvas.paste(inner, (x, y))
    return np.asarray(canvas)


def pillow_rect(img, oh, ow, scale):
    """where Pillow pastes the image in the canvas scaled by `scale` about the centre of the oh x ow canvas"""
    from PIL import Image, ImageOps
    sc, sr = int(round(ow * float(np.float32(scale)))), int(round(oh * float(np.float32(scale))))
    iw, ih = ImageOps.contain(Image.fromarray(img), (sc, sr)).size
    x = round((sc - iw) * 0.5) if iw != sc else 0
    y = round((sr - ih) * 0.5) if iw == sc and ih != sr else 0
    return x + (ow - sc) // 2, y + (oh - sr) // 2, iw, ih


def cases():
    """(name, image, (oh, ow), (x, y, iw, ih, mirror), scale)"""
    out = []
    for i, (h, w, oh, ow) in enumerate(SCALED):
        img = image(i, h, w)
        for s in SCALES:
            rect = pillow_rect(img, oh, ow, s)
            for mirror in (0, 1):
                out.append(("%dx%d_to_%dx%d_s%d_m%d" % (h, w, oh, ow, round(100 * s), mirror), img, (oh, ow), rect + (mirror,), s))
    for i, (name, h, w, oh, ow, rect) in enumerate(EXPLICIT):
        img = image(100 + i, h, w)
        for mirror in (0, 1):
            out.append(("%s_m%d" % (name, mirror), img, (oh, ow), tuple(rect) + (mirror,), 0.0))
    return out


def generate():
    import PIL
    from PIL import Image, ImageOps
    all_cases = cases()
    out = {"pillow_version": np.array(PIL.__version__), "names": np.array([c[0] for c in all_cases]), "fill": np.array(FILL, np.uint8)}
    for name, img, (oh, ow), view, scale in all_cases:
        out[name + "_in"] = img
        out[name + "_canvas"] = np.array((oh, ow), np.int32)
        out[name + "_view"] = np.array(view, np.int32)
        out[name + "_scale"] = np.float32(scale)
        for f in ALL:
            canvas = pillow_view(f, img, oh, ow, view, FILL)
            assert canvas.shape == (oh, ow, 3)
            if scale == 1.0 and view[4] == 0:       # the letterbox itself
                pad = np.asarray(ImageOps.pad(Image.fromarray(img), (ow, oh), Image.Resampling(f), color=FILL))
                assert np.array_equal(canvas, pad), "%s under %s: resize / paste is not ImageOps.pad" % (name, FILTER_NAMES[f])
            out[name + "_" + FILTER_NAMES[f]] = canvas
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
