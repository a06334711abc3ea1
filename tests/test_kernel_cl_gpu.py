"""The device's LITERAL kernels (csrc/mbn_literal.hip, through the C-ABI) against the bytes that the reference's own kernel.cl,
compiled for the CPU, wrote for the same call: tests/golden/kernel_cl_vectors.npz (cases and generator: tests/kernel_cl_cases.py,
tests/golden/make_kernel_cl_fixtures.py). No oracle in between and nothing but the .npz is read: neither the reference nor
oracle/_ref/ is needed here.

A case is either the text as it stands (quirks 0xF: the carry kernels) or its per-channel composition (quirks 0x4 for
convolute / depthwise, 0x0 for pointwise, 0x8 for pool: the quirk sets under which the device takes its v_dot4 and MFMA forms).
Bit for bit, with a canary after every output.
"""
import ctypes as C

import numpy as np
import pytest

import kernel_cl_cases as kc

pytestmark = pytest.mark.gpu

CASES = kc.load()
BY_NAME = {c["name"]: c for c in CASES}
CANARY, CANARY_BYTES = 0xA5, 64


def _odd(fs):
    """The filter size whose taps kernel.cl runs for `fs` (loops -h..h, h = fs / 2). The ABI takes odd sizes only."""
    return 2 * (fs // 2) + 1


def _tune_modes(c):
    """tune lit_dot: 0 = the default choice, 1 = the tap-by-tap / scalar kernels; pointwise also 2 = v_dot4 and 3 = the MFMA form
    wherever eligible. pool has no such forms."""
    return {"pool": (0,), "pointwise": (0, 1, 2, 3)}.get(c["kernel"], (0, 1))


def _launch(pkg, ctx, c, d_out, d_in, d_f, ext):
    k, fs = c["kernel"], _odd(c["filtersize"])
    if k == "convolute":
        ctx.convolute(d_out.ptr, d_in[0].ptr, d_in[1].ptr, d_in[2].ptr, d_f.ptr, c["rows"], c["cols"], fs, c["stride"], c["op_size"], ext)
    elif k == "depthwise":
        ctx.depthwise(d_out.ptr, d_in[0].ptr, d_f.ptr, c["rows"], c["cols"], fs, c["stride"], c["op_size"], ext)
    elif k == "pointwise":
        ctx.pointwise(d_out.ptr, d_in[0].ptr, d_f.ptr, c["rows"], c["cols"], c["filtersize"], c["op_size"], ext)
    else:
        ctx.pool(d_out.ptr, d_in[0].ptr, c["rows"], c["cols"], c["filtersize"], c["op_size"], ext)
    ctx.sync()


def _ext(pkg, c, batch=1):
    # pool's NDRange is 1 x 1 in every case and the device computes work-item (0, 0) whatever gsize says
    g = (0, 0) if c["kernel"] == "pool" else (c["g0"], c["g1"])
    return pkg.make_ext(batch=batch, dtype=pkg.DT_U8, quirks=kc.quirks_of(c), gsize=g, in_rows=c["in_rows"], in_cols=c["in_cols"])


def _null_ext_says_the_same(c):
    """ext = NULL is the context default: quirks 0xF, the default NDRange, in_rows x in_cols = rows * stride x cols * stride."""
    return not c["per_channel"] and (c["kernel"] == "pool" or (c["g0"], c["g1"]) == (0, 0)) and not c["in_rows"] and not c["in_cols"]


class _Device:
    """The case's buffers on the device, `batch` copies of each activation; freed on exit."""

    def __init__(self, ctx, c, batch=1, d_in=None):
        self.ctx, self.c, self.batch, self.size = ctx, c, batch, c["want"].size * batch
        self.own = []
        if d_in is None:
            planes = (c["r"], c["g"], c["b"]) if c["kernel"] == "convolute" else (c["x"],)
            d_in = [self._keep(ctx.to_device(np.tile(p, batch))) for p in planes]
        self.d_in = d_in
        self.d_f = self._keep(ctx.to_device(c["f"])) if c["f"] is not None else None
        self.d_out = self._keep(ctx.alloc(self.size + CANARY_BYTES))

    def _keep(self, b):
        self.own.append(b)
        return b

    def reset_output(self):
        first = np.zeros(self.c["want"].size, np.uint8) if self.c["out0"] is None else self.c["out0"]
        self.d_out.upload(np.concatenate([np.tile(first, self.batch), np.full(CANARY_BYTES, CANARY, np.uint8)]))

    def read(self, what):
        raw = self.d_out.download((self.size + CANARY_BYTES,), np.uint8)
        assert (raw[self.size:] == CANARY).all(), "%s: bytes after the output were written" % what
        return raw[:self.size]

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for b in self.own:
            self.ctx._bufs.remove(b)
            b.free()


def _check(got, want, what):
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, "%s: %d of %d bytes differ from kernel.cl's, first at %d: device %d, kernel.cl %d" % (
        what, bad.size, want.size, bad[0], got[bad[0]], want[bad[0]])


def _run_all_forms(pkg, ctx, c, dev, want, what):
    exts = [("ext", _ext(pkg, c, dev.batch))] + ([("ext = NULL", None)] if dev.batch == 1 and _null_ext_says_the_same(c) else [])
    try:
        for mode in _tune_modes(c):
            assert ctx.lib.mbn_tune_set(b"lit_dot", mode) == 0
            for ext_name, ext in exts:
                dev.reset_output()
                _launch(pkg, ctx, c, dev.d_out, dev.d_in, dev.d_f, ext)
                _check(dev.read(what), want, "%s (%s, lit_dot %d)" % (what, ext_name, mode))
    finally:
        ctx.lib.mbn_tune_set(b"lit_dot", 0)


@pytest.mark.parametrize("case", CASES, ids=lambda c: c["name"])
def test_device_equals_compiled_kernel_cl(pkg, ctx, case):
    """Every recorded launch through ctx.convolute / depthwise / pointwise / pool with the case's quirks and NDRange; the text
    cases that ext = NULL can express also with ext = NULL; every dot form of the kernel, and the kernels they replace."""
    c = case
    with _Device(ctx, c) as dev:
        if c["filtersize"] != _odd(c["filtersize"]) and c["kernel"] in ("convolute", "depthwise"):
            # kernel.cl runs the taps -h..h whatever the parity, so filtersize 4 consumes 25 taps per channel. The ABI sizes the
            # filter as filtersize^2 and therefore refuses even sizes; the text's bytes are those of the next odd size.
            rc = ctx.lib.mbn_depthwise(ctx.h, dev.d_out.ptr, dev.d_in[0].ptr, dev.d_f.ptr, c["rows"], c["cols"], c["filtersize"],
                                       c["stride"], c["op_size"], C.byref(_ext(pkg, c)))
            assert rc == pkg.EINVAL
        _run_all_forms(pkg, ctx, c, dev, c["want"], c["name"])


@pytest.mark.parametrize("name", ["conv_text_16x12x8", "conv_pc_16x16x12_int8", "dw_text_12x10x7", "dw_pc_9x33x7_int8",
                                  "pw_text_3x5_8_6_8", "pw_pc_5x7_48_20", "pool_text_5x5_3_33", "pool_pc_5x5_3_33"])
def test_batch_of_three_is_three_copies(pkg, ctx, name):
    """ext->batch = 3 over three copies of the case's input = three copies of kernel.cl's bytes: the carry kernels (the text cases)
    and the dot forms (the per-channel cases) both stride by image."""
    c = BY_NAME[name]
    with _Device(ctx, c, batch=3) as dev:
        _run_all_forms(pkg, ctx, c, dev, np.tile(c["want"], 3), name + " x 3")


def test_chain_runs_end_to_end_on_the_device(pkg, ctx):
    """conv 16x16x3 -> 8x8x4, depthwise, pointwise, depthwise stride 2, pointwise, pool under quirks 0xF: each stage reads the
    previous stage's DEVICE output, and each is compared with what kernel.cl wrote from its own previous stage, so the first
    wrong stage is the one named."""
    chain = [c for c in CASES if c["name"].startswith("chain_")]
    assert [c["prev"] for c in chain[1:]] == [c["name"] for c in chain[:-1]] and len(chain) == 6
    devs, d_prev = [], None
    try:
        for c in chain:
            dev = _Device(ctx, c, d_in=None if d_prev is None else [d_prev])
            devs.append(dev)
            dev.reset_output()
            _launch(pkg, ctx, c, dev.d_out, dev.d_in, dev.d_f, _ext(pkg, c))
            _check(dev.read(c["name"]), c["want"], "chain stage " + c["name"])
            d_prev = dev.d_out
    finally:
        for dev in devs:
            dev.__exit__()
