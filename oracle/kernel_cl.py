"""ctypes front-end of the reference's own kernel.cl compiled for the CPU (oracle/_ref/libkernel_cl.so, built
by `make -C oracle` where the reference is present). TEST INFRASTRUCTURE ONLY.

kernel.cl checks no bounds and its launches in MobileNet.c race, so this module is the one place that makes a
call well-defined before the compiled text runs:

  * every input is copied into a buffer with a zeroed guard tail sized from the largest index the launch forms
    (kernel_cl_driver.c, ref_max_*). The zeros are what MBN_Q_LITERAL_INDEX defines: an index past the end
    of the input buffer reads 0;
  * the filter must hold every tap the launch consumes (ValueError otherwise: no defined value exists);
  * the output buffer holds the largest index written, is followed by a canary, and a write past the size
    the caller's output has is a ValueError;
  * the launch runs with ascending and with descending work-item order; RacyLaunch when the bytes differ.

`convolute`, `depthwise`, `pointwise`, `pool` are the text as it stands: every quirk on (quirks 0xF). The
`*_per_channel` functions call the text once per output channel with op_size = 1 and the pointers moved to
that channel; with one channel in the call neither the carried sum nor the plane-0 read can act, which gives
reference bytes for quirks 0x4 (convolute, depthwise), 0x0 (pointwise) and 0x8 (pool).
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "_ref", "libkernel_cl.so")

CANARY = 0xA5
CANARY_BYTES = 64

# the quirk sets that the per-channel composition yields, by kernel
PER_CHANNEL_QUIRKS = {"convolute": 0x4, "depthwise": 0x4, "pointwise": 0x0, "pool": 0x8}


class RacyLaunch(ValueError):
    """The launch's bytes depend on the order of its work-items: it has no expected output."""


def available() -> bool:
    return os.path.exists(LIB_PATH)


_lib = None


def lib():
    global _lib
    if _lib is None:
        l = C.CDLL(LIB_PATH)
        p, i = C.c_void_p, C.c_int
        l.ref_convolute.argtypes = [i, i, i, p, p, p, p, p, i, i, i, i, i]
        l.ref_depthwise.argtypes = [i, i, i, p, p, p, i, i, i, i, i]
        l.ref_pointwise.argtypes = [i, i, i, p, p, p, i, i, i, i]
        l.ref_pool.argtypes = [i, i, i, p, p, i, i, i, i]
        for f in (l.ref_convolute, l.ref_depthwise, l.ref_pointwise, l.ref_pool):
            f.restype = None
        l.ref_max_in_window.argtypes = [i, i, i, i]
        l.ref_taps.argtypes = [i]
        l.ref_max_in_pointwise.argtypes = [i, i, i, i, i]
        l.ref_max_in_pool.argtypes = [i, i, i, i]
        l.ref_max_out.argtypes = [i, i, C.c_long, i]
        for f in (l.ref_max_in_window, l.ref_taps, l.ref_max_in_pointwise, l.ref_max_in_pool, l.ref_max_out):
            f.restype = C.c_long
        _lib = l
    return _lib


def _flat(a, dtype):
    return np.ascontiguousarray(a, dtype=dtype).reshape(-1)


def _need(v, what):
    if v < 0:
        raise ValueError("kernel_cl: %s: arguments outside what the driver runs" % what)
    return int(v)


class _Guarded:
    """A copy of an input followed by zeros, so that `offset + max_index` is inside it for every launch made."""

    def __init__(self, data):
        self.data = _flat(data, np.uint8)
        self.buf = self.data

    def reach(self, offset, max_index):
        n = offset + max_index + 1
        if n > self.buf.size:
            grown = np.zeros(n, np.uint8)
            grown[:self.data.size] = self.data
            self.buf = grown

    def ptr(self, offset):
        return self.buf.ctypes.data + offset


def _run(launches, out_size, prefill):
    """launches: pairs (fn(order, address of the output's first byte), bytes of the output the call reaches: 1 + the largest
    index it writes). Runs them all under each work-item order in an output large enough for every write, then holds the
    result to the caller's out_size. Returns those bytes."""
    reach = max(r for _, r in launches)
    size = max(out_size, reach)
    outs = []
    for order in (0, 1):
        buf = np.full(size + CANARY_BYTES, CANARY, np.uint8)
        buf[:size] = 0
        if prefill is not None:
            buf[:out_size] = prefill
        for fn, _ in launches:
            fn(order, buf.ctypes.data)
        if not (buf[size:] == CANARY).all():
            raise AssertionError("kernel_cl: the compiled reference wrote past the largest index computed for its output")
        outs.append(buf[:size])
    if not np.array_equal(outs[0], outs[1]):
        raise RacyLaunch("kernel_cl: ascending and descending work-item order give different bytes (%d differ)"
                         % int((outs[0] != outs[1]).sum()))
    if reach > out_size:
        raise ValueError("kernel_cl: the launch writes index %d of an output of %d bytes" % (reach - 1, out_size))
    return outs[0][:out_size].copy()


def _prefill(out, out_size):
    if out is None:
        return None
    o = _flat(out, np.uint8)
    if o.size != out_size:
        raise ValueError("kernel_cl: out has %d bytes, the call's output has %d" % (o.size, out_size))
    return o


def _filter(filt, taps_needed):
    f = _flat(filt, np.int32).copy()
    if f.size < taps_needed:
        raise ValueError("kernel_cl: the launch reads %d filter taps, %d given" % (taps_needed, f.size))
    return f


def _channels(op_size, per_channel):
    """(first channel, channels in the call) for each call of the text."""
    return [(c, 1) for c in range(op_size)] if per_channel else [(0, op_size)]


# ----------------------------------------------------------------------------- the four kernels

def _convolute(inp_r, inp_g, inp_b, filt, rows, cols, filtersize, stride, op_size, g0, g1, out, per_channel):
    l = lib()
    g0, g1 = g0 or cols // stride, g1 or rows // stride
    shift = (rows // 2) * (cols // 2)
    taps = 3 * _need(l.ref_taps(filtersize), "convolute")
    f = _filter(filt, taps * op_size)
    planes = [_Guarded(p) for p in (inp_r, inp_g, inp_b)]
    for p in planes:
        p.reach(0, _need(l.ref_max_in_window(g0, g1, filtersize, stride), "convolute"))
    launches = []
    for c0, n in _channels(op_size, per_channel):
        def fn(order, base, c0=c0, n=n):
            l.ref_convolute(g0, g1, order, base + shift * c0, planes[0].ptr(0), planes[1].ptr(0), planes[2].ptr(0),
                            f.ctypes.data + 4 * taps * c0, rows, cols, filtersize, stride, n)
        launches.append((fn, shift * c0 + _need(l.ref_max_out(g0, g1, shift, n), "convolute") + 1))
    return _run(launches, op_size * shift, _prefill(out, op_size * shift))


def _depthwise(inp, filt, rows, cols, filtersize, stride, op_size, in_rows, in_cols, g0, g1, out, per_channel):
    l = lib()
    g0, g1 = g0 or cols, g1 or rows
    shift = rows * cols
    in_plane = (in_rows or rows * stride) * (in_cols or cols * stride)
    taps = _need(l.ref_taps(filtersize), "depthwise")
    f = _filter(filt, taps * op_size)
    x = _Guarded(inp)
    if x.data.size != in_plane * op_size:
        raise ValueError("kernel_cl: depthwise input has %d bytes, op_size planes of in_rows x in_cols have %d"
                         % (x.data.size, in_plane * op_size))
    reach_in = _need(l.ref_max_in_window(g0, g1, filtersize, stride), "depthwise")
    for c0, _ in _channels(op_size, per_channel):          # the guard is measured to the end of the whole buffer
        x.reach(in_plane * c0 if per_channel else 0, reach_in)
    launches = []
    for c0, n in _channels(op_size, per_channel):
        def fn(order, base, c0=c0, n=n):
            l.ref_depthwise(g0, g1, order, base + shift * c0, x.ptr(in_plane * c0 if per_channel else 0),
                            f.ctypes.data + 4 * taps * c0, rows, cols, filtersize, stride, n)
        launches.append((fn, shift * c0 + _need(l.ref_max_out(g0, g1, shift, n), "depthwise") + 1))
    return _run(launches, op_size * shift, _prefill(out, op_size * shift))


def _pointwise(inp, filt, rows, cols, filtersize, op_size, g0, g1, out, per_channel):
    l = lib()
    g0, g1 = g0 or cols, g1 or rows
    shift = rows * cols
    f = _filter(filt, filtersize * op_size)
    x = _Guarded(inp)
    x.reach(0, _need(l.ref_max_in_pointwise(g0, g1, rows, cols, filtersize), "pointwise"))
    launches = []
    for c0, n in _channels(op_size, per_channel):
        def fn(order, base, c0=c0, n=n):   # every output channel sums over the same input planes: the input stays put
            l.ref_pointwise(g0, g1, order, base + shift * c0, x.ptr(0), f.ctypes.data + 4 * filtersize * c0,
                            rows, cols, filtersize, n)
        launches.append((fn, shift * c0 + _need(l.ref_max_out(g0, g1, shift, n), "pointwise") + 1))
    return _run(launches, op_size * shift, _prefill(out, op_size * shift))


def _pool(inp, rows, cols, filtersize, op_size, g0, g1, out, per_channel):
    l = lib()
    g0, g1 = g0 or 1, g1 or 1
    plane = rows * cols
    x = _Guarded(inp)
    for c0, n in _channels(op_size, per_channel):
        x.reach(plane * c0, _need(l.ref_max_in_pool(rows, cols, filtersize, n), "pool"))
    launches = []
    for c0, n in _channels(op_size, per_channel):
        def fn(order, base, c0=c0, n=n):
            l.ref_pool(g0, g1, order, base + c0, x.ptr(plane * c0), rows, cols, filtersize, n)
        launches.append((fn, c0 + _need(l.ref_max_out(g0, g1, 1, n), "pool") + 1))
    return _run(launches, op_size, _prefill(out, op_size))


def convolute(inp_r, inp_g, inp_b, filt, rows, cols, filtersize, stride, op_size, g0=0, g1=0, out=None):
    """kernel.cl `convolute` at NDRange g0 x g1 (default: cols/stride x rows/stride). planes uint8 [rows*cols]; filt int32
    [op_size][3][k][k]. Returns uint8 [op_size * (rows/2) * (cols/2)]; `out` prefills it (cells the launch leaves alone)."""
    return _convolute(inp_r, inp_g, inp_b, filt, rows, cols, filtersize, stride, op_size, g0, g1, out, False)


def depthwise(inp, filt, rows, cols, filtersize, stride, op_size, in_rows=0, in_cols=0, g0=0, g1=0, out=None):
    """kernel.cl `depthwise` at NDRange g0 x g1 (default cols x rows). inp uint8 [op_size][in_rows][in_cols] (default
    rows*stride x cols*stride: the text never sees the plane size, it only sets where the buffer ends)."""
    return _depthwise(inp, filt, rows, cols, filtersize, stride, op_size, in_rows, in_cols, g0, g1, out, False)


def pointwise(inp, filt, rows, cols, filtersize, op_size, g0=0, g1=0, out=None):
    """kernel.cl `pointwise` at NDRange g0 x g1 (default cols x rows). inp uint8, at least filtersize planes of rows*cols."""
    return _pointwise(inp, filt, rows, cols, filtersize, op_size, g0, g1, out, False)


def pool(inp, rows, cols, filtersize, op_size, g0=0, g1=0, out=None):
    """kernel.cl `pool` at NDRange g0 x g1 (default 1 x 1, what MobileNet.c launches)."""
    return _pool(inp, rows, cols, filtersize, op_size, g0, g1, out, False)


def convolute_per_channel(inp_r, inp_g, inp_b, filt, rows, cols, filtersize, stride, op_size, g0=0, g1=0, out=None):
    """quirks 0x4: per call the filter moves by one channel's 3*k*k taps, the output by one plane."""
    return _convolute(inp_r, inp_g, inp_b, filt, rows, cols, filtersize, stride, op_size, g0, g1, out, True)


def depthwise_per_channel(inp, filt, rows, cols, filtersize, stride, op_size, in_rows=0, in_cols=0, g0=0, g1=0, out=None):
    """quirks 0x4: per call the input moves by one in_rows x in_cols plane, the filter by k*k taps, the output by one plane."""
    return _depthwise(inp, filt, rows, cols, filtersize, stride, op_size, in_rows, in_cols, g0, g1, out, True)


def pointwise_per_channel(inp, filt, rows, cols, filtersize, op_size, g0=0, g1=0, out=None):
    """quirks 0x0: per call the filter moves by one row of `filtersize` weights, the output by one plane; the input stays."""
    return _pointwise(inp, filt, rows, cols, filtersize, op_size, g0, g1, out, True)


def pool_per_channel(inp, rows, cols, filtersize, op_size, g0=0, g1=0, out=None):
    """quirks 0x8: per call the input moves by one plane, the output by one byte."""
    return _pool(inp, rows, cols, filtersize, op_size, g0, g1, out, True)
