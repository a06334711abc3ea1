"""Pins the CPU oracle's LITERAL functions (oracle/mbn_oracle.c: orc_lit_*) to the reference's own program text: kernel.cl,
compiled unmodified for the CPU into oracle/_ref/libkernel_cl.so (`make -C oracle`, where the reference is present) and
called through oracle/kernel_cl.py, which makes each call well-defined first (guarded inputs, canaries, both work-item orders).

  * tests/golden/kernel_cl_vectors.npz records what the compiled text wrote for the cases of tests/kernel_cl_cases.py;
    with the library present every case is run again and must give the recorded bytes (skips only without the library);
  * the oracle must give the recorded bytes: quirks 0xF for the text as it stands, the composed quirk set for the
    per-channel cases (these run everywhere: they need the .npz only);
  * the hand-derived KATs (tests/golden/kat_literal.json) must be what the compiled text gives, wherever the text (0xF) or
    its per-channel composition computes the KAT's quirk set.
"""
import json
import os
import subprocess

import numpy as np
import pytest

import kernel_cl as kcl
import kernel_cl_cases as kc

ORACLE_DIR = os.path.dirname(os.path.abspath(kcl.__file__))
CASES = kc.load()
SPECS = {c["name"]: c for c in kc.specs()}
needs_ref = pytest.mark.skipif(not kcl.available(), reason="oracle/_ref/libkernel_cl.so is not built (no reference on this machine)")


def test_fixture_file_is_small_and_complete():
    assert os.path.getsize(kc.VECTORS) < 256 * 1024
    assert [c["name"] for c in CASES] == list(SPECS)
    assert kcl.PER_CHANNEL_QUIRKS == kc.PER_CHANNEL_QUIRKS
    shapes = [l.strip() for l in open(kc.SHAPES) if l.strip() and not l.startswith("#")]
    assert shapes == [kc.shape_line(c) for c in CASES]              # ref-selftest runs exactly the recorded launches


# ----------------------------------------------------------------------------- the compiled text == the fixture

@needs_ref
@pytest.mark.parametrize("case", CASES, ids=lambda c: c["name"])
def test_compiled_kernel_cl_reproduces_the_fixture(case):
    spec = SPECS[case["name"]]
    for k in ("x", "r", "g", "b", "f", "out0"):                      # the recorded inputs are the generator's
        if spec.get(k) is not None:
            assert np.array_equal(spec[k], case[k]), k
    assert np.array_equal(kc.run_reference(kcl, case), case["want"])


# ----------------------------------------------------------------------------- the oracle == the fixture

@pytest.mark.parametrize("case", CASES, ids=lambda c: c["name"])
def test_oracle_equals_compiled_kernel_cl(orc, case):
    got = kc.run_oracle(orc, case)
    bad = np.flatnonzero(got != case["want"])
    assert bad.size == 0, "%s under quirks 0x%X: %d bytes differ, first at %d: oracle %d, kernel.cl %d" % (
        case["name"], kc.quirks_of(case), bad.size, bad[0], got[bad[0]], case["want"][bad[0]])


# ----------------------------------------------------------------------------- the hand-derived KATs == the compiled text

def _kat_mode(case):
    """"text", "per_channel" or None: whether kernel.cl as it stands (every quirk on) or its per-channel composition
    (PER_CHANNEL_QUIRKS) computes the KAT's quirk set. Only the bits that can act in the call count: with one output
    channel nothing is carried (0x1) and plane 0 is the channel's own plane (0x2); a 7 x 7 pool divides by 49 either way."""
    k, q, one = case["kernel"], case["quirks"], case["op_size"] == 1
    acts = {"convolute": (0 if one else 0x1) | 0x4,
            "depthwise": (0 if one else 0x3) | 0x4,
            "pointwise": 0 if one else 0x1,
            "pool": (0 if one else 0x1) | (0 if case["filtersize"] ** 2 == 49 else 0x8)}[k]
    if q & acts == acts:
        return "text"
    if q & acts == kc.PER_CHANNEL_QUIRKS[k] & acts:
        return "per_channel"
    return None


def _kats():
    cases = json.load(open(os.path.join(kc.GOLD, "kat_literal.json")))["cases"]
    return [c for c in cases if _kat_mode(c)]


def test_kat_selection_covers_every_quirk_set_the_composition_reaches():
    got = {(c["kernel"], c["quirks"]) for c in _kats()}
    assert {("depthwise", 0x4), ("convolute", 0x4), ("pointwise", 0x0), ("pointwise", 0x1), ("pool", 0x8), ("pool", 0x0),
            ("pool", 0x1)} <= got
    assert len(_kats()) >= 14


@needs_ref
@pytest.mark.parametrize("case", _kats(), ids=lambda c: c["name"])
def test_kat_equals_compiled_kernel_cl(case):
    k, pc = case["kernel"], _kat_mode(case) == "per_channel"
    rows, cols, fs, oc = case["rows"], case["cols"], case["filtersize"], case["op_size"]
    if k == "depthwise":
        fn = kcl.depthwise_per_channel if pc else kcl.depthwise
        got = fn(case["input"], case["filter"], rows, cols, fs, case["stride"], oc)
    elif k == "pointwise":
        fn = kcl.pointwise_per_channel if pc else kcl.pointwise
        got = fn(case["input"], case["filter"], rows, cols, fs, oc)
    elif k == "pool":
        x = (np.concatenate([np.full(rows * cols, v, np.uint8) for v in case["input_fill"]]) if "input_fill" in case
             else np.array(case["input"], np.uint8))
        got = (kcl.pool_per_channel if pc else kcl.pool)(x, rows, cols, fs, oc)
    else:
        g = np.array(case["input_g"], np.uint8) if "input_g" in case else np.full(rows * cols, case["input_g_fill"], np.uint8)
        b = np.array(case["input_b"], np.uint8) if "input_b" in case else np.full(rows * cols, case["input_b_fill"], np.uint8)
        f = np.array(case["filter"], np.int32) if "filter" in case else np.full(oc * 27, case["filter_fill"], np.int32)
        fn = kcl.convolute_per_channel if pc else kcl.convolute
        got = fn(case["input_r"], g, b, f, rows, cols, fs, case["stride"], oc)
    assert list(got) == case["expected"], case["why"]


# ----------------------------------------------------------------------------- what the loader refuses

@needs_ref
def test_reference_layer1_geometry_is_order_dependent():
    """MobileNet.c launches layer 1 with one work-item per INPUT pixel (224 x 224) over an output plane of (rows/2) x (cols/2):
    work-item wi of channel c and work-item wi + plane of channel c - 1 write the same byte. At 16 x 16 with 4 channels the
    bytes depend on the work-item order, so the launch has no expected output: what test_literal_racy_ndrange_is_rejected
    (the ABI's MBN_EINVAL) claims."""
    rng = np.random.default_rng(3)
    rows = cols = 16
    r, g, b = (rng.integers(0, 256, rows * cols, dtype=np.uint8) for _ in range(3))
    f = rng.integers(-3, 4, 4 * 27, dtype=np.int32)
    with pytest.raises(kcl.RacyLaunch):
        kcl.convolute(r, g, b, f, rows, cols, 3, 2, 4, g0=cols, g1=rows)
    kcl.convolute(r, g, b, f, rows, cols, 3, 2, 4)                      # the output-sized NDRange is race-free


@needs_ref
def test_loader_refuses_calls_without_defined_bytes():
    x = np.arange(2 * 16, dtype=np.uint8)
    f = np.ones(2 * 9, np.int32)
    with pytest.raises(ValueError, match="filter taps"):                # an even filtersize reads the next odd one's taps
        kcl.depthwise(x, f, 4, 4, 4, 1, 2)
    with pytest.raises(ValueError, match="writes index"):               # one channel cannot race, but 5 x 4 work-items leave a 4 x 4 plane
        kcl.depthwise(x[:16], f[:9], 4, 4, 3, 1, 1, g0=5, g1=4)
    with pytest.raises(ValueError, match="out has"):
        kcl.depthwise(x, f, 4, 4, 3, 1, 2, out=np.zeros(5, np.uint8))
    # guard zeros: the last work-item's window runs past the buffer and reads 0 there (MBN_Q_LITERAL_INDEX's definition)
    got = kcl.depthwise(np.full(16, 1, np.uint8), np.ones(9, np.int32), 4, 4, 3, 1, 1)
    # work-item (3, 3) forms indices 10 11 12 | 14 15 16 | 18 19 20: index 12 is the next row's first byte, 16 and up are guard zeros
    assert got[15] == 3 + 2 and got[5] == 9 and got[0] == 4


def test_lit_pool_refuses_a_window_longer_than_the_plane(orc):
    """kernel.cl's pool reads filtersize^2 consecutive bytes from the start of each plane: more than rows * cols runs into the next
    plane and, in the last channel, past the buffer. The C-ABI returns MBN_EINVAL (mbn_pool); the oracle wrapper raises."""
    x = np.zeros((2, 3, 3), np.uint8)
    for q in (0x0, 0xF):
        with pytest.raises(ValueError):
            orc.lit_pool(x, 3, 3, 4, 2, quirks=q)
    with pytest.raises(ValueError):
        orc.lit_pool(x, 3, 3, 3, 3)                                     # three planes asked of a two-plane input
    assert list(orc.lit_pool(x, 3, 3, 3, 2)) == [0, 0]


# ----------------------------------------------------------------------------- the sanitizer self-test

def test_ref_selftest_is_clean_under_asan_and_ubsan():
    """`make -C oracle ref-selftest`: kernel.cl and the driver in a plain executable under ASan + UBSan run every recorded launch in
    buffers of exactly the guard arithmetic's sizes. Needs the reference's source, so it skips only where that is absent."""
    if subprocess.run(["make", "-s", "-C", ORACLE_DIR, "ref-available"]).returncode != 0:
        pytest.skip("the reference's kernel.cl is not on this machine")
    r = subprocess.run(["make", "-C", ORACLE_DIR, "ref-selftest"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "%d launches in bounds" % len(CASES) in r.stdout
