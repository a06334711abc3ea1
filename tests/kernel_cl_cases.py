"""The launches of the reference's kernel.cl that tests/golden/kernel_cl_vectors.npz records, and the ways a case is run:
through the compiled reference (oracle/kernel_cl.py), through the CPU oracle, and — in test_kernel_cl_gpu.py — through the
device. An ordinary helper module: tests/golden/make_kernel_cl_fixtures.py builds the cases from `specs()`, the tests read
them back with `load()`. The .npz holds data only: inputs, filters, arguments, NDRange and the bytes the reference wrote.

A case is a dict:
  name, kernel ("convolute" | "depthwise" | "pointwise" | "pool"), per_channel (False: the text as it stands, quirks 0xF;
  True: one call of the text per output channel, quirks PER_CHANNEL_QUIRKS[kernel]), g0, g1 (NDRange; 0 = the kernel's
  default), rows, cols, filtersize, stride, op_size, in_rows, in_cols (depthwise; 0 = rows * stride, cols * stride),
  x (uint8 input; convolute: r, g, b), f (int32 filter; none for pool), out0 (uint8 prefill of the output, or None),
  want (the reference's bytes), prev (name of the chain stage whose `want` is this case's x, or "").
"""
import os

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
VECTORS = os.path.join(GOLD, "kernel_cl_vectors.npz")
SHAPES = os.path.join(GOLD, "kernel_cl_shapes.txt")

KERNELS = ("convolute", "depthwise", "pointwise", "pool")
PER_CHANNEL_QUIRKS = {"convolute": 0x4, "depthwise": 0x4, "pointwise": 0x0, "pool": 0x8}   # = kernel_cl.PER_CHANNEL_QUIRKS
ARGS = ("kernel", "per_channel", "g0", "g1", "rows", "cols", "filtersize", "stride", "op_size", "in_rows", "in_cols")


def quirks_of(case) -> int:
    return PER_CHANNEL_QUIRKS[case["kernel"]] if case["per_channel"] else 0xF


def taps_of(filtersize) -> int:
    """Taps per plane that kernel.cl's loops -h..h (h = filtersize / 2) run: an even filtersize runs the next odd one's."""
    return (2 * (filtersize // 2) + 1) ** 2


# ----------------------------------------------------------------------------- the cases

def _weights(rng, kind, shape):
    if kind == "small":
        return rng.integers(-3, 4, shape, dtype=np.int32)
    if kind == "pos":                                # biased upwards, so that ReLU leaves a deep window or a chain alive
        return rng.integers(-2, 4, shape, dtype=np.int32)
    if kind == "int8":                               # the int8 limits, as test_literal_3x3_rows_on_dot4_are_bit_exact
        f = rng.integers(-128, 128, shape, dtype=np.int32)
        f[0] = 127
        f[1 % shape[0]] = -128
        return f
    if kind == "wide":                               # outside int8: the device's dot forms must fall back
        return rng.integers(-300, 301, shape, dtype=np.int32)
    if kind == "wrap":                               # up to 2^30: the int32 sum wraps
        return rng.integers(-2 ** 30, 2 ** 30 + 1, shape, dtype=np.int32)
    raise ValueError(kind)


def _case(name, kernel, per_channel=False, g0=0, g1=0, rows=0, cols=0, filtersize=0, stride=1, op_size=0, in_rows=0,
          in_cols=0, **more):
    c = dict(name=name, kernel=kernel, per_channel=bool(per_channel), g0=g0, g1=g1, rows=rows, cols=cols,
             filtersize=filtersize, stride=stride, op_size=op_size, in_rows=in_rows, in_cols=in_cols, out0=None, prev="")
    c.update(more)
    return c


def _dw(rng, name, rows, cols, ch, stride, fs=3, w="small", per_channel=False, g=(0, 0), in_hw=(0, 0), prefill=False):
    ih, iw = in_hw[0] or rows * stride, in_hw[1] or cols * stride
    c = _case(name, "depthwise", per_channel, g[0], g[1], rows, cols, fs, stride, ch, in_hw[0], in_hw[1])
    c["x"] = rng.integers(0, 256, ch * ih * iw, dtype=np.uint8)
    c["f"] = _weights(rng, w, (ch, taps_of(fs))).reshape(-1)
    if prefill:
        c["out0"] = rng.integers(0, 256, ch * rows * cols, dtype=np.uint8)
    return c


def _conv(rng, name, rows, cols, oc, w="small", per_channel=False):
    c = _case(name, "convolute", per_channel, 0, 0, rows, cols, 3, 2, oc)
    c["r"], c["g"], c["b"] = (rng.integers(0, 256, rows * cols, dtype=np.uint8) for _ in range(3))
    c["f"] = _weights(rng, w, (oc, 27)).reshape(-1)
    return c


def _pw(rng, name, rows, cols, cin, oc, fs, w="small", per_channel=False):
    c = _case(name, "pointwise", per_channel, 0, 0, rows, cols, fs, 1, oc)
    c["x"] = rng.integers(0, 256, cin * rows * cols, dtype=np.uint8)
    c["f"] = _weights(rng, w, (oc, fs)).reshape(-1)
    return c


def _pool(rng, name, rows, cols, fs, ch, per_channel=False):
    c = _case(name, "pool", per_channel, 1, 1, rows, cols, fs, 1, ch)
    c["x"] = rng.integers(0, 256, ch * rows * cols, dtype=np.uint8)
    return c


def specs():
    """Every case without its `want`. Chain stages after the first carry no x: the generator fills it from `prev`."""
    rng = np.random.default_rng(20240607)
    cs = [
        # depthwise, the text (0xF): (rows, cols, ch, stride)
        _dw(rng, "dw_text_8x8x5", 8, 8, 5, 1),
        _dw(rng, "dw_text_12x10x7", 12, 10, 7, 1),
        _dw(rng, "dw_text_5x9_s1", 5, 9, 3, 1),
        _dw(rng, "dw_text_9x5_s2", 9, 5, 3, 2),
        _dw(rng, "dw_text_fs1", 6, 7, 3, 1, fs=1),
        _dw(rng, "dw_text_fs5", 6, 7, 3, 1, fs=5, w="pos"),
        _dw(rng, "dw_text_fs4_even", 6, 7, 3, 1, fs=4, w="pos"),
        _dw(rng, "dw_text_wrap_2p30", 6, 6, 4, 1, w="wrap"),
        _dw(rng, "dw_text_g4x4_over_8x8", 8, 8, 3, 1, g=(4, 4), prefill=True),
        _dw(rng, "dw_text_g8x4_over_8x8", 8, 8, 3, 1, g=(8, 4), prefill=True),
        _dw(rng, "dw_text_in_9x7_for_6x6", 6, 6, 3, 1, in_hw=(9, 7)),
        _dw(rng, "dw_text_in_13x11_for_6x6_s2", 6, 6, 3, 2, in_hw=(13, 11)),
        # depthwise, per channel (0x4): where the device runs its v_dot4 rows
        _dw(rng, "dw_pc_10x10x5_wide", 10, 10, 5, 1, w="wide", per_channel=True),
        _dw(rng, "dw_pc_9x33x7_int8", 9, 33, 7, 1, w="int8", per_channel=True),
        _dw(rng, "dw_pc_28x28x32", 28, 28, 32, 1, per_channel=True),
        _dw(rng, "dw_pc_14x14x16_s2_int8", 14, 14, 16, 2, w="int8", per_channel=True),
        # convolute: (rows, cols, op_size), stride 2
        _conv(rng, "conv_text_8x8x4", 8, 8, 4),
        _conv(rng, "conv_text_16x12x8", 16, 12, 8),
        _conv(rng, "conv_text_12x16x3", 12, 16, 3),
        _conv(rng, "conv_pc_16x16x12_int8", 16, 16, 12, w="int8", per_channel=True),
        # pointwise: (rows, cols, Cin, Cout, filtersize)
        _pw(rng, "pw_text_4x4_3_5_3", 4, 4, 3, 5, 3),
        _pw(rng, "pw_text_7x7_64_48_1", 7, 7, 64, 48, 1),
        _pw(rng, "pw_text_3x5_8_6_8", 3, 5, 8, 6, 8),
        _pw(rng, "pw_pc_6x6_32_32", 6, 6, 32, 32, 32, w="int8", per_channel=True),
        _pw(rng, "pw_pc_5x7_48_20", 5, 7, 48, 20, 48, w="int8", per_channel=True),
        _pw(rng, "pw_pc_1x1_128_100", 1, 1, 128, 100, 128, w="int8", per_channel=True),
        _pw(rng, "pw_pc_4x5_3_7", 4, 5, 3, 7, 3, per_channel=True),
        # pool at NDRange 1 x 1: (rows, cols, filtersize, channels)
        _pool(rng, "pool_text_7x7_7_70", 7, 7, 7, 70),
        _pool(rng, "pool_text_5x5_3_33", 5, 5, 3, 33),
        _pool(rng, "pool_text_4x6_4_5", 4, 6, 4, 5),
        _pool(rng, "pool_pc_7x7_7_70", 7, 7, 7, 70, per_channel=True),
        _pool(rng, "pool_pc_5x5_3_33", 5, 5, 3, 33, per_channel=True),
        _pool(rng, "pool_pc_4x6_4_5", 4, 6, 4, 5, per_channel=True),
    ]
    # one chain under 0xF: conv 16x16x3 -> 8x8x4, depthwise, pointwise 4 -> 8, depthwise stride 2 -> 4x4, pointwise 8 -> 6, pool
    chain = [_conv(rng, "chain_0_conv", 16, 16, 4),
             _dw(rng, "chain_1_dw", 8, 8, 4, 1, w="pos"),
             _pw(rng, "chain_2_pw", 8, 8, 4, 8, 4, w="pos"),
             _dw(rng, "chain_3_dw_s2", 4, 4, 8, 2, w="pos"),
             _pw(rng, "chain_4_pw", 4, 4, 8, 6, 8, w="pos"),
             _pool(rng, "chain_5_pool", 4, 4, 4, 6)]
    for prev, c in zip(chain, chain[1:]):
        c["prev"] = prev["name"]
        del c["x"]
    return cs + chain


# ----------------------------------------------------------------------------- the fixture file

def save(cases, path=VECTORS):
    arrays = {"names": np.array([c["name"] for c in cases])}
    for c in cases:
        n = c["name"]
        arrays[n + "/args"] = np.array([KERNELS.index(c["kernel"]) if k == "kernel" else int(c[k]) for k in ARGS], np.int32)
        arrays[n + "/prev"] = np.array(c["prev"])
        for k in ("x", "r", "g", "b", "f", "out0", "want"):
            if c.get(k) is not None and not (k == "x" and c["prev"]):       # a chain stage's x is its predecessor's want
                arrays[n + "/" + k] = c[k]
    np.savez_compressed(path, **arrays)


def load(path=VECTORS):
    z = np.load(path)
    cases, by_name = [], {}
    for n in (str(s) for s in z["names"]):
        c = dict(zip(ARGS, (int(v) for v in z[n + "/args"])))
        c["name"], c["kernel"], c["per_channel"] = n, KERNELS[c["kernel"]], bool(c["per_channel"])
        c["prev"] = str(z[n + "/prev"])
        for k in ("x", "r", "g", "b", "f", "out0", "want"):
            c[k] = z[n + "/" + k] if n + "/" + k in z.files else None
        if c["prev"]:
            c["x"] = by_name[c["prev"]]["want"]
        cases.append(c)
        by_name[n] = c
    return cases


def shape_line(c) -> str:
    """The case as oracle/ref_selftest.c reads it."""
    in_bytes = c["r"].size if c["kernel"] == "convolute" else c["x"].size
    return "%s %d %d %d %d %d %d %d %d %d" % (c["kernel"], c["per_channel"], c["g0"] or default_ndrange(c)[0],
                                              c["g1"] or default_ndrange(c)[1], c["rows"], c["cols"], c["filtersize"],
                                              c["stride"], c["op_size"], in_bytes)


def default_ndrange(c):
    if c["kernel"] == "convolute":
        return c["cols"] // c["stride"], c["rows"] // c["stride"]
    if c["kernel"] == "pool":
        return 1, 1
    return c["cols"], c["rows"]


# ----------------------------------------------------------------------------- running a case on the CPU

def run_reference(kcl, c):
    """The bytes the compiled kernel.cl writes for the case (kcl = the oracle/kernel_cl.py module)."""
    k, pc = c["kernel"], c["per_channel"]
    nd = dict(g0=c["g0"], g1=c["g1"], out=c["out0"])
    if k == "convolute":
        fn = kcl.convolute_per_channel if pc else kcl.convolute
        return fn(c["r"], c["g"], c["b"], c["f"], c["rows"], c["cols"], c["filtersize"], c["stride"], c["op_size"], **nd)
    if k == "depthwise":
        fn = kcl.depthwise_per_channel if pc else kcl.depthwise
        return fn(c["x"], c["f"], c["rows"], c["cols"], c["filtersize"], c["stride"], c["op_size"], c["in_rows"], c["in_cols"], **nd)
    if k == "pointwise":
        fn = kcl.pointwise_per_channel if pc else kcl.pointwise
        return fn(c["x"], c["f"], c["rows"], c["cols"], c["filtersize"], c["op_size"], **nd)
    fn = kcl.pool_per_channel if pc else kcl.pool
    return fn(c["x"], c["rows"], c["cols"], c["filtersize"], c["op_size"], **nd)


def run_oracle(orc, c, quirks=None):
    """The same call through oracle/mbn_oracle.c under the case's quirk set."""
    k, q = c["kernel"], quirks_of(c) if quirks is None else quirks
    if k == "convolute":
        return orc.lit_convolute(c["r"], c["g"], c["b"], c["f"], c["rows"], c["cols"], c["filtersize"], c["stride"], c["op_size"],
                                 quirks=q, g0=c["g0"], g1=c["g1"], out=c["out0"])
    if k == "depthwise":
        return orc.lit_depthwise(c["x"], c["f"], c["rows"], c["cols"], c["filtersize"], c["stride"], c["op_size"], c["in_rows"],
                                 c["in_cols"], quirks=q, g0=c["g0"], g1=c["g1"], out=c["out0"])
    if k == "pointwise":
        return orc.lit_pointwise(c["x"], c["f"], c["rows"], c["cols"], c["filtersize"], c["op_size"], quirks=q)
    return orc.lit_pool(c["x"], c["rows"], c["cols"], c["filtersize"], c["op_size"], quirks=q)
