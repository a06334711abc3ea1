"""The classifier read-out on the GPU, pinned at every class count, k, tie and planning CU count.

mbn_softmax_f32, mbn_softmax_topk_f32 (the block form), mbn_pool_fc and mbn_classifier_tail_fused (the one-wave form behind two hand-written
cross-workgroup hand-overs) against tests/readout_ref.py: the ranking exactly (a total order needs no tolerance), the probabilities against a
float64 softmax within the bound the arithmetic gives (readout_ref.prob_bound), the one-wave form against the block form byte for byte on logits
an FC reproduces exactly, the pooled sum on all three of its code paths, and every hand-over at planning counts 3 / 8 / 20 / 72 on ONE workspace
that is zeroed once. tests/test_readout_cpu.py gates the case tables. No call is repeated to coax a race out: each runs once or twice and is
compared. profiles/LOG.md ("Classifier read-out") holds the measured errors; every test prints its own.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import readout_ref as R

pytestmark = pytest.mark.gpu

TOL_PW = 1e-4          # tests/test_parity_gpu.py: max |got - want| <= TOL_PW * max|want| + 1e-7 per tensor, every value finite
FF = 0xFFFFFFFF
GUARD = 16             # words of 0xFF behind every output


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same(a, b, what):
    assert a.shape == b.shape and np.array_equal(_bits(a), _bits(b)), what


def _guarded(ctx, words):
    d = ctx.alloc((words + GUARD) * 4)
    assert ctx.lib.mbn_memset(ctx.h, d.ptr, 0xFF, (words + GUARD) * 4) == 0
    return d


def _take(d, shape, dtype, what):
    """download a guarded output: the 0xFF words behind it must be intact"""
    words = int(np.prod(shape))
    raw = d.download((words + GUARD,), np.uint32)
    assert (raw[words:] == FF).all(), "stores past the output: " + what
    return raw[:words].view(dtype).reshape(shape)


def _ws_clean(d_ws, what):
    assert not d_ws.download((128,), np.uint32).any(), "arrival counters not back to zero: " + what


def _workspace(ctx, channels, classes):
    nb = ctx.lib.mbn_pool_fc_workspace_bytes(channels, classes)
    assert nb >= 512 + (channels // 64) * 4 * classes * 4
    d = ctx.alloc(nb)
    assert ctx.lib.mbn_memset(ctx.h, d.ptr, 0, nb) == 0          # ZEROED ONCE: no test clears it again
    return d, nb


def _block(ctx, logits, k, probs=True):
    """mbn_softmax_topk_f32 over all rows in one call -> (idx [n][k], winners' probabilities [n][k], probabilities [n][classes] or None)"""
    n, classes = logits.shape
    d_l = ctx.to_device(logits)
    d_p, d_i, d_v = _guarded(ctx, n * classes), _guarded(ctx, n * k), _guarded(ctx, n * k)
    assert ctx.lib.mbn_softmax_topk_f32(ctx.h, d_p.ptr if probs else None, d_i.ptr, d_v.ptr, d_l.ptr, n, classes, k, None) == 0
    ctx.sync()
    out = (_take(d_i, (n, k), np.int32, "top-k idx"), _take(d_v, (n, k), np.float32, "top-k prob"),
           _take(d_p, (n, classes), np.float32, "probs") if probs else None)
    if not probs:
        assert (d_p.download((n * classes,), np.uint32) == FF).all(), "probs = NULL and yet written"
    for b in (d_l, d_p, d_i, d_v):
        b.free()
    return out


def _softmax(ctx, logits):
    n, classes = logits.shape
    d_l, d_p, d_a = ctx.to_device(logits), _guarded(ctx, n * classes), _guarded(ctx, n)
    assert ctx.lib.mbn_softmax_f32(ctx.h, d_p.ptr, d_a.ptr, d_l.ptr, n, classes, None) == 0
    ctx.sync()
    out = _take(d_p, (n, classes), np.float32, "softmax probs"), _take(d_a, (n,), np.int32, "softmax argmax")
    for b in (d_l, d_p, d_a):
        b.free()
    return out


def _prob_err(got, want):
    """worst over the rows of max_i |got_i - want_i| / max_i want_i, and of |sum_i got_i - 1|"""
    g, w = got.astype(np.float64), np.asarray(want, np.float64)
    return float((np.abs(g - w).max(axis=1) / w.max(axis=1)).max()), float(np.abs(g.sum(axis=1) - 1).max())


class _Tail:
    """mbn_classifier_tail_fused on chosen logits: an FC whose column j holds row j and 1 x 1 images e_j (readout_ref.fc_for_rows). Finite
    rows go 64 to a filter and a call of `batch` images takes `batch` consecutive ones; a row that is not finite goes alone, in column 0, `batch`
    times over. Every call writes its own slice of four big outputs, read back once per (k, batch).
    The e_j construction cannot put a finite and a non-finite row into ONE tail launch (0 x inf in the other image's column): that the other
    rows of a batch do not notice such a row is shown side by side for the block form and mbn_softmax_f32 (test_patterns_block_form), and for
    the one-wave form only through each row's byte equality with the block form."""

    def __init__(self, ctx, rows, channels, d_ws, nb):
        self.ctx, self.rows, self.channels, self.d_ws, self.nb = ctx, np.asarray(rows, np.float32), channels, d_ws, nb
        self.classes = self.rows.shape[1]
        fin = [i for i, r in enumerate(self.rows) if np.isfinite(r).all()]
        self.groups = [fin[i:i + 64] for i in range(0, len(fin), 64)] + [[i] for i in range(len(self.rows)) if i not in set(fin)]
        self.filters = []
        for g in self.groups:
            w, x = R.fc_for_rows(self.rows[g], channels)
            if len(g) == 1:
                x = np.repeat(x, 4, axis=0)                    # the one row for up to four images
            self.filters.append((ctx.to_device(w), ctx.to_device(x)))

    def calls(self, batch):
        """[(group, first image, images, source rows)]"""
        out = []
        for gi, g in enumerate(self.groups):
            if len(g) == 1:
                out.append((gi, 0, batch, [g[0]] * batch))
            else:
                out += [(gi, s, min(batch, len(g) - s), g[s:s + batch]) for s in range(0, len(g), batch)]
        return out

    def run(self, k, batch, probs=True):
        """-> (source row of every output row, logits, probs or None, idx, winners' probabilities)"""
        ctx, classes, ch = self.ctx, self.classes, self.channels
        calls = self.calls(batch)
        src = np.array([s for c in calls for s in c[3]])
        total = len(src)
        d_l, d_p, d_i, d_v = _guarded(ctx, total * classes), _guarded(ctx, total * classes), _guarded(ctx, total * k), _guarded(ctx, total * k)
        at = 0
        for gi, first, n, _ in calls:
            d_w, d_x = self.filters[gi]
            rc = ctx.lib.mbn_classifier_tail_fused(ctx.h, d_i.ptr + at * k * 4, d_v.ptr + at * k * 4, d_p.ptr + at * classes * 4 if probs else None,
                                                   d_l.ptr + at * classes * 4, d_x.ptr + first * ch * 4, d_w.ptr, None, n, 1, 1, ch, classes, k,
                                                   self.d_ws.ptr, self.nb, None)
            assert rc == 0, (rc, ctx.last_error())
            at += n
        ctx.sync()
        what = "tail k=%d batch=%d" % (k, batch)
        out = (src, _take(d_l, (total, classes), np.float32, what), _take(d_p, (total, classes), np.float32, what) if probs else None,
               _take(d_i, (total, k), np.int32, what), _take(d_v, (total, k), np.float32, what))
        _ws_clean(self.d_ws, what)
        for b in (d_l, d_p, d_i, d_v):
            b.free()
        return out

    def free(self):
        for d_w, d_x in self.filters:
            d_w.free()
            d_x.free()


def _logits_are(got, want, what):
    """the FC handed the chosen logits back: the same bits wherever they are numbers, a NaN where a NaN went in"""
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan) and np.array_equal(_bits(got)[~nan], _bits(want)[~nan]), what


# ----------------------------------------------------------------------------- 1. class counts

@pytest.mark.parametrize("classes", R.CLASS_COUNTS_BLOCK)
def test_class_counts(pkg, ctx, classes):
    """normal(0, 3) logits, batch 3, k = 1..8: the winners exactly; probabilities, winners' probabilities and row sums within prob_bound of the
    float64 softmax; mbn_softmax_f32's argmax is the top-1 index and its probabilities are the block form's bytes; probs = NULL changes no winner.
    Up to 1024 classes the one-wave form as well, through mbn_classifier_tail_fused."""
    logits = R.random_rows(classes, R.BATCH)
    want_p = R.softmax64(logits)
    bound = R.prob_bound(classes)
    sm_p, sm_a = _softmax(ctx, logits)
    worst = {"softmax_f32": _prob_err(sm_p, want_p)}
    forms = {}
    for k in R.KS:
        want_i = R.topk_order(logits, k)
        want_v = np.where(want_i >= 0, np.take_along_axis(want_p, np.maximum(want_i, 0).astype(np.int64), axis=1), 0.0)
        idx, val, probs = _block(ctx, logits, k)
        idx0, val0, _ = _block(ctx, logits, k, probs=False)
        assert np.array_equal(idx, want_i), "block form, k = %d" % k
        _same(idx0, idx, "probs = NULL: winners")
        _same(val0, val, "probs = NULL: winners' probabilities")
        assert np.array_equal(sm_a, idx[:, 0]), "mbn_softmax_f32's argmax is not the top-1 index"
        _same(sm_p, probs, "mbn_softmax_f32 and the block form sum in one order")
        forms.setdefault("block", []).append((probs, val, want_v))
    if classes <= 1024:
        d_ws, nb = _workspace(ctx, 64, classes)
        tail = _Tail(ctx, logits, 64, d_ws, nb)
        for k in R.KS:
            want_i = R.topk_order(logits, k)
            want_v = np.where(want_i >= 0, np.take_along_axis(want_p, np.maximum(want_i, 0).astype(np.int64), axis=1), 0.0)
            src, lg, probs, idx, val = tail.run(k, R.BATCH)
            assert src.tolist() == [0, 1, 2]
            _logits_are(lg, logits, "the FC does not reproduce the logits")
            assert np.array_equal(idx, want_i), "one-wave form, k = %d" % k
            _, _, _, idx0, val0 = tail.run(k, R.BATCH, probs=False)
            _same(idx0, idx, "probs = NULL: winners (one-wave form)")
            _same(val0, val, "probs = NULL: winners' probabilities (one-wave form)")
            forms.setdefault("wave", []).append((probs, val, want_v))
        tail.free()
        d_ws.free()
    for form, runs in forms.items():
        e = s = v = 0.0
        for probs, val, want_v in runs:
            a, b = _prob_err(probs, want_p)
            e, s = max(e, a), max(s, b)
            v = max(v, float((np.abs(val.astype(np.float64) - want_v).max(axis=1) / want_p.max(axis=1)).max()))
        worst[form] = (e, s, v)
    for form, errs in sorted(worst.items()):
        print("readout-error classes=%d form=%s probs=%.3e rowsum=%.3e%s bound=%.3e" % (classes, form, errs[0], errs[1],
                                                                                         " winners=%.3e" % errs[2] if len(errs) > 2 else "", bound))
    for form, errs in worst.items():
        assert max(errs) <= bound, "%s at %d classes: %s over the bound %.3e" % (form, classes, errs, bound)


# ----------------------------------------------------------------------------- 2, 3, 4. ties, magnitudes, rows without a finite maximum

@pytest.mark.parametrize("classes", R.CLASS_COUNTS_BLOCK)
def test_patterns_block_form(pkg, ctx, classes):
    """Every pattern row of items 2-4 through mbn_softmax_topk_f32 (k = 8) and mbn_softmax_f32 in ONE batch, the rows without a finite maximum
    between the others: the order exactly; probabilities within prob_bound of the float64 softmax of the UNSHIFTED row; -inf entries exactly 0;
    nothing NaN on a row with a maximum; rows without one as include/mbn.h states (indices in range or -1, every probability NaN, -1 beside
    probability 0); and the rows with a maximum the same bytes as in a batch that holds none of the others."""
    pats = R.all_patterns(classes)
    names = [n for n, _, _ in pats]
    order = np.random.default_rng(classes).permutation(len(pats))          # the non-finite rows scattered through the batch
    rows = np.stack([pats[i][1] for i in order])
    refs = np.stack([pats[i][2] for i in order])
    good = np.array([R.has_max(r) for r in rows])
    k = 8
    idx, val, probs = _block(ctx, rows, k)
    sm_p, sm_a = _softmax(ctx, rows)
    want_i = R.topk_order(rows, k)
    for r in range(len(rows)):
        assert np.array_equal(idx[r], want_i[r]), "order of row %s: %s, want %s" % (names[order[r]], idx[r], want_i[r])
    assert (((idx >= 0) & (idx < classes)) | (idx == -1)).all() and (((sm_a >= 0) & (sm_a < classes)) | (sm_a == -1)).all()
    assert np.array_equal(sm_a, idx[:, 0]), "mbn_softmax_f32's argmax is not the top-1 index"
    _same(sm_p[good], probs[good], "mbn_softmax_f32 and the block form")
    assert np.isnan(sm_p[~good]).all()
    # rows with a maximum
    want_p = R.softmax64(refs[good])
    assert np.isfinite(probs[good]).all() and np.isfinite(val[good]).all()
    e, s = _prob_err(probs[good], want_p)
    wi = want_i[good]
    want_v = np.where(wi >= 0, np.take_along_axis(want_p, np.maximum(wi, 0).astype(np.int64), axis=1), 0.0)
    v = float((np.abs(val[good].astype(np.float64) - want_v).max(axis=1) / want_p.max(axis=1)).max())
    print("readout-error classes=%d form=block-patterns probs=%.3e rowsum=%.3e winners=%.3e bound=%.3e" % (classes, e, s, v, R.prob_bound(classes)))
    assert max(e, s, v) <= R.prob_bound(classes)
    assert (probs[good][np.isneginf(rows[good])] == 0).all(), "-inf entries must have probability exactly 0"
    assert (val[good][wi == -1] == 0).all()
    # rows without one
    assert np.isnan(probs[~good]).all(), "a row without a finite maximum must be NaN throughout"
    bad_i, bad_v = idx[~good], val[~good]
    assert (bad_v[bad_i == -1] == 0).all() and np.isnan(bad_v[bad_i >= 0]).all()
    # the others do not notice them: the same rows in a batch of their own
    idx2, val2, probs2 = _block(ctx, rows[good], k)
    sm_p2, sm_a2 = _softmax(ctx, rows[good])
    _same(idx2, idx[good], "winners next to non-finite rows")
    _same(val2, val[good], "winners' probabilities next to non-finite rows")
    _same(probs2, probs[good], "probabilities next to non-finite rows")
    _same(sm_p2, sm_p[good], "mbn_softmax_f32 next to non-finite rows")
    _same(sm_a2, sm_a[good], "mbn_softmax_f32's argmax next to non-finite rows")


# ----------------------------------------------------------------------------- 5. block form and wave form

def _wave_equals_block(ctx, rows, channels, d_ws, nb, what):
    """every row, batch 1..4, k in TAIL_KS: logits, probabilities, winners and winners' probabilities of mbn_classifier_tail_fused byte for
    byte those of mbn_softmax_topk_f32 on the same logits. -> {(k, batch): (src, logits, idx)}"""
    tail = _Tail(ctx, rows, channels, d_ws, nb)
    seen = {}
    for k in R.TAIL_KS:
        b_idx, b_val, b_probs = _block(ctx, rows, k)
        assert np.array_equal(b_idx, R.topk_order(rows, k)), what
        for batch in (1, 2, 3, 4):
            src, lg, probs, idx, val = tail.run(k, batch)
            assert set(src.tolist()) == set(range(len(rows))), "a row was left out"
            w = "%s, k = %d, batch = %d" % (what, k, batch)
            _logits_are(lg, rows[src], "the FC does not reproduce the logits: " + w)
            _same(idx, b_idx[src], "winners: " + w)
            _same(val, b_val[src], "winners' probabilities: " + w)
            _same(probs, b_probs[src], "probabilities: " + w)
            seen[(k, batch)] = (src, lg, idx)
    tail.free()
    return seen


@pytest.mark.parametrize("classes", R.CLASS_COUNTS)
def test_wave_form_equals_block_form(pkg, ctx, classes):
    rows = np.stack([r for _, r, _ in R.all_patterns(classes)] + list(R.random_rows(classes, 4, seed=5)))
    d_ws, nb = _workspace(ctx, 64, classes)
    _wave_equals_block(ctx, rows, 64, d_ws, nb, "%d classes" % classes)
    d_ws.free()


# ----------------------------------------------------------------------------- 6. pool + FC geometry

@functools.lru_cache(maxsize=None)
def _fc_weights(channels):
    rng = np.random.default_rng(channels)
    return (rng.normal(0, (1.0 / channels) ** 0.5, (max(R.POOL_CLASSES), channels)).astype(np.float32),
            rng.normal(0, 0.5, max(R.POOL_CLASSES)).astype(np.float32))


def _pool_fc(ctx, d_x, d_w, d_b, n, rows, cols, ch, classes, d_ws, nb, what):
    d_o = _guarded(ctx, n * classes)
    rc = ctx.lib.mbn_pool_fc(ctx.h, d_o.ptr, d_x.ptr, d_w.ptr, d_b.ptr if d_b else None, n, rows, cols, ch, classes, d_ws.ptr, nb, None)
    assert rc == 0, (rc, ctx.last_error(), what)
    ctx.sync()
    got = _take(d_o, (n, classes), np.float32, what)
    _ws_clean(d_ws, what)
    d_o.free()
    return got


def _tail_fused(ctx, d_x, d_w, d_b, n, rows, cols, ch, classes, k, d_ws, nb, what):
    d_l, d_p, d_i, d_v = _guarded(ctx, n * classes), _guarded(ctx, n * classes), _guarded(ctx, n * k), _guarded(ctx, n * k)
    rc = ctx.lib.mbn_classifier_tail_fused(ctx.h, d_i.ptr, d_v.ptr, d_p.ptr, d_l.ptr, d_x.ptr, d_w.ptr, d_b.ptr if d_b else None, n, rows, cols, ch,
                                           classes, k, d_ws.ptr, nb, None)
    assert rc == 0, (rc, ctx.last_error(), what)
    ctx.sync()
    out = (_take(d_l, (n, classes), np.float32, what), _take(d_p, (n, classes), np.float32, what), _take(d_i, (n, k), np.int32, what),
           _take(d_v, (n, k), np.float32, what))
    _ws_clean(d_ws, what)
    for b in (d_l, d_p, d_i, d_v):
        b.free()
    return out


def _check_tail(lg, probs, idx, val, k, what):
    """the tail's ranking and probabilities against the reference on the tail's OWN logits"""
    classes = lg.shape[1]
    want_i = R.topk_order(lg, k)
    assert np.array_equal(idx, want_i), what
    want_p = R.softmax64(lg)
    e, s = _prob_err(probs, want_p)
    want_v = np.where(want_i >= 0, np.take_along_axis(want_p, np.maximum(want_i, 0).astype(np.int64), axis=1), 0.0)
    v = float((np.abs(val.astype(np.float64) - want_v).max(axis=1) / want_p.max(axis=1)).max())
    assert max(e, s, v) <= R.prob_bound(classes), (what, e, s, v)
    return max(e, s, v)


def _geometry(pkg, ctx, rows, cols, channels, class_counts, batches, workspaces, what):
    """mbn_pool_fc and mbn_classifier_tail_fused on a rows x cols map: against pool_fc64 within TOL_PW, an image's logits whatever its batch,
    the tail's logits those of mbn_pool_fc, bias NULL, the pooled values those of mbn_pool bit for bit (an identity FC reads them out), exact
    integers with the mean of an equal map, a guard behind every output, the counters back to zero after every call."""
    pix = rows * cols
    fs = max(rows, cols)
    for ch in channels:
        w_all, b_all = _fc_weights(ch)
        x = np.random.default_rng(pix * 4096 + ch).uniform(0, 6, (4, pix, ch)).astype(np.float32)
        d_x, d_w, d_b = ctx.to_device(x), ctx.to_device(w_all), ctx.to_device(b_all)
        if ch not in workspaces:
            workspaces[ch] = _workspace(ctx, ch, max(R.POOL_CLASSES))
        d_ws = workspaces[ch][0]
        worst = worst_p = 0.0
        for classes in class_counts:
            nb = ctx.lib.mbn_pool_fc_workspace_bytes(ch, classes)
            w, b = w_all[:classes], b_all[:classes]
            want = R.pool_fc64(x, w, b)
            full = None
            for n in sorted(batches, reverse=True):
                tag = "%s %dx%d ch %d classes %d batch %d" % (what, rows, cols, ch, classes, n)
                got = _pool_fc(ctx, d_x, d_w, d_b, n, rows, cols, ch, classes, d_ws, nb, tag)
                scale = max(float(np.abs(want[:n]).max()), 1e-6)
                err = float(np.abs(got.astype(np.float64) - want[:n]).max())
                worst = max(worst, err / scale)
                assert np.isfinite(got).all() and err <= TOL_PW * scale + 1e-7, "%s: %.3e of %.3e" % (tag, err, scale)
                if full is None:
                    full = got
                _same(got, full[:n], "logits depend on the batch: " + tag)
                nobias = _pool_fc(ctx, d_x, d_w, None, n, rows, cols, ch, classes, d_ws, nb, tag + " no bias")
                want0 = R.pool_fc64(x[:n], w)
                scale0 = max(float(np.abs(want0).max()), 1e-6)
                assert np.isfinite(nobias).all() and float(np.abs(nobias - want0).max()) <= TOL_PW * scale0 + 1e-7, tag + " no bias"
                if classes <= 1024:
                    k = 1 + (n + classes) % 8
                    lg, probs, idx, val = _tail_fused(ctx, d_x, d_w, d_b, n, rows, cols, ch, classes, k, d_ws, nb, tag + " tail")
                    _same(lg, got, "the tail's logits are not mbn_pool_fc's: " + tag)
                    worst_p = max(worst_p, _check_tail(lg, probs, idx, val, k, tag + " tail"))
        print("readout-error pool_fc %s %dx%d (%s) ch=%d rel=%.3e tol=%.1e tail-probs=%.3e" % (what, rows, cols, R.pool_path(pix), ch, worst, TOL_PW, worst_p))
        # the pooled values themselves: FC = identity hands them through (x + 0 is exact, and no pooled value here is -0.0)
        nbi = ctx.lib.mbn_pool_fc_workspace_bytes(ch, ch)
        d_id, d_pool = ctx.to_device(np.eye(ch, dtype=np.float32)), _guarded(ctx, 4 * ch)
        ctx.pool(d_pool.ptr, d_x.ptr, rows, cols, fs, ch, pkg.make_ext(batch=4, act=0))
        ctx.sync()
        pooled = _take(d_pool, (4, ch), np.float32, "mbn_pool")
        assert float(np.abs(pooled - x.astype(np.float64).mean(1)).max()) <= 1e-5 * 6 + 1e-7          # TOL_DW of test_parity_gpu.py
        for n in batches:
            tag = "%s pooled values %dx%d ch %d batch %d" % (what, rows, cols, ch, n)
            _same(_pool_fc(ctx, d_x, d_id, None, n, rows, cols, ch, ch, d_ws, nbi, tag), pooled[:n], tag)
            _same(_tail_fused(ctx, d_x, d_id, None, n, rows, cols, ch, ch, 3, d_ws, nbi, tag)[0], pooled[:n], tag + " (tail)")
        # exact integers: an equal value per map and channel (the mean is exact on every path), an asymmetric filter (slice / class-range maps)
        rng = np.random.default_rng(pix + ch)
        xi = np.repeat(rng.integers(0, 4, (4, 1, ch)), pix, axis=1).astype(np.float32)
        d_x.upload(xi)
        d_pooled = ctx.alloc(4 * ch * 4)
        for classes in class_counts:
            wi = rng.integers(-2, 3, (classes, ch)).astype(np.float32)
            wi[:, 0] = np.arange(classes) % 5
            wi[:, ch - 1] = np.arange(classes) % 3
            d_w.upload(wi)
            nb = ctx.lib.mbn_pool_fc_workspace_bytes(ch, classes)
            want = xi[:, 0].astype(np.float64) @ wi.astype(np.float64).T
            for n in batches:
                tag = "%s exact integers %dx%d ch %d classes %d batch %d" % (what, rows, cols, ch, classes, n)
                got = _pool_fc(ctx, d_x, d_w, None, n, rows, cols, ch, classes, d_ws, nb, tag)
                assert np.array_equal(got.astype(np.float64), want[:n]), tag
                if classes <= 1024:
                    assert np.array_equal(_tail_fused(ctx, d_x, d_w, None, n, rows, cols, ch, classes, 8, d_ws, nb, tag)[0], got), tag + " (tail)"
            # mbn_pool + mbn_pointwise: the two launches the one stands for
            n = max(batches)
            d_two = _guarded(ctx, n * classes)
            ctx.pool(d_pooled.ptr, d_x.ptr, rows, cols, fs, ch, pkg.make_ext(batch=n, act=0))
            ctx.pointwise(d_two.ptr, d_pooled.ptr, d_w.ptr, 1, 1, ch, classes, pkg.make_ext(batch=n, act=0))
            ctx.sync()
            assert np.array_equal(d_pooled.download((n, ch), np.float32), xi[:n, 0]), "mbn_pool on an equal map"
            assert np.array_equal(_take(d_two, (n, classes), np.float32, "two launches").astype(np.float64), want[:n]), "two launches, exact integers"
            d_two.free()
        for b in (d_x, d_w, d_b, d_id, d_pool, d_pooled):
            b.free()


@pytest.mark.parametrize("shape", R.MAPS, ids=lambda s: "%dx%d" % s)
def test_pool_fc_geometry(pkg, ctx, shape):
    workspaces = {}
    _geometry(pkg, ctx, shape[0], shape[1], R.POOL_CHANNELS, R.POOL_CLASSES, (1, 2, 3, 4), workspaces, "device count")
    for d_ws, _ in workspaces.values():
        d_ws.free()


# ----------------------------------------------------------------------------- 7. planning CU counts

def _set(ctx, cus):
    assert ctx.lib.mbn_set_planning_cus(ctx.h, cus) == 0, cus


@pytest.mark.parametrize("shape", R.CU_SHAPES, ids=lambda s: "%dch-%dclasses" % s)
def test_planning_counts(pkg, ctx, shape):
    """Items 5 and 6 at planning counts 3, 8, 20 and 72, then at the device's own: ONE workspace for every call of every count and batch size,
    zeroed once (a counter left non-zero by one plan would derail the next). At every count the logits are the bytes of the device's own count
    (the summation order is fixed per class) and the winners identical."""
    channels, classes = shape
    rows = np.stack([r for _, r, _ in R.all_patterns(classes)] + list(R.random_rows(classes, 4, seed=7)))
    d_ws, nb = _workspace(ctx, channels, max(classes, channels))      # the identity FC of _geometry has `channels` classes
    device = ctx.device_cus()
    seen = {}
    x = np.random.default_rng(channels + classes).uniform(0, 6, (4, 49, channels)).astype(np.float32)
    w_all, b_all = _fc_weights(channels)
    d_x, d_w, d_b = ctx.to_device(x), ctx.to_device(w_all[:classes]), ctx.to_device(b_all[:classes])
    net = {}
    try:
        assert device >= max(R.CU_COUNTS), "a device of %d CUs cannot plan for %s" % (device, R.CU_COUNTS)      # no count is dropped quietly
        for cus in R.CU_COUNTS + (0,):
            _set(ctx, cus)
            seen[cus] = _wave_equals_block(ctx, rows, channels, d_ws, nb, "%d classes x %d channels at %d CUs" % (classes, channels, cus))
            net[cus] = [_tail_fused(ctx, d_x, d_w, d_b, n, 7, 7, channels, classes, 5, d_ws, nb, "7x7 at %d CUs, batch %d" % (cus, n)) for n in (4, 1, 3, 2)]
            for r, c in R.MAPS:
                _geometry(pkg, ctx, r, c, (channels,), (classes,), (1 + (r * c + cus) % 4, 4), {channels: (d_ws, nb)}, "%d CUs" % cus)
    finally:
        _set(ctx, 0)
    assert ctx.device_cus() == device
    for cus in seen:
        for key, (src, lg, idx) in seen[cus].items():
            assert np.array_equal(src, seen[0][key][0])
            _same(lg, seen[0][key][1], "logits at %d CUs against the device's own count %s" % (cus, key))
            _same(idx, seen[0][key][2], "winners at %d CUs against the device's own count %s" % (cus, key))
        for got, own in zip(net[cus], net[0]):
            for a, b, name in zip(got, own, ("logits", "probabilities", "winners", "winners' probabilities")):
                _same(a, b, "%s of a 7x7 map at %d CUs against the device's own count" % (name, cus))
    for b in (d_x, d_w, d_b, d_ws):
        b.free()


@pytest.mark.parametrize("cus", [3, 0])
def test_tail_graph_replay(pkg, ctx, cus):
    """One capture of mbn_classifier_tail_fused, three replays: the eager call's bytes each time, the counters back to zero each time."""
    n, h, ch, classes, k = 3, 7, 1024, 1000, 5
    rng = np.random.default_rng(9)
    x = rng.uniform(0, 6, (n, h * h, ch)).astype(np.float32)
    w, b = _fc_weights(ch)
    d_x, d_w, d_b = ctx.to_device(x), ctx.to_device(w[:classes]), ctx.to_device(b[:classes])
    d_ws, nb = _workspace(ctx, ch, classes)
    outs = [ctx.alloc(s * 4) for s in (n * classes, n * classes, n * k, n * k)]
    shapes = (((n, classes), np.float32), ((n, classes), np.float32), ((n, k), np.int32), ((n, k), np.float32))
    g = C.c_void_p()
    try:
        _set(ctx, cus)
        eager = _tail_fused(ctx, d_x, d_w, d_b, n, h, h, ch, classes, k, d_ws, nb, "eager")
        assert ctx.lib.mbn_graph_begin(ctx.h, None) == 0
        rc = ctx.lib.mbn_classifier_tail_fused(ctx.h, outs[2].ptr, outs[3].ptr, outs[1].ptr, outs[0].ptr, d_x.ptr, d_w.ptr, d_b.ptr, n, h, h, ch, classes, k,
                                               d_ws.ptr, nb, None)
        assert ctx.lib.mbn_graph_end(ctx.h, None, C.byref(g)) == 0 and rc == 0
        for rep in range(3):
            for o in outs:
                assert ctx.lib.mbn_memset(ctx.h, o.ptr, 0xFF, o.nbytes) == 0          # outside the graph
            assert ctx.lib.mbn_graph_launch(ctx.h, g, None) == 0
            ctx.sync()
            for o, (shp, dt), want, name in zip(outs, shapes, eager, ("logits", "probabilities", "winners", "winners' probabilities")):
                _same(o.download(shp, dt), want, "replay %d: %s" % (rep, name))
            _ws_clean(d_ws, "replay %d" % rep)
    finally:
        _set(ctx, 0)
        if g.value:
            assert ctx.lib.mbn_graph_destroy(ctx.h, g) == 0
    for bfr in [d_x, d_w, d_b, d_ws] + outs:
        bfr.free()


# ----------------------------------------------------------------------------- 8. statuses

def test_statuses_and_nothing_written(pkg, ctx):
    ch, classes, h = 128, 1025, 2
    inv, uns = pkg.EINVAL, pkg.EUNSUPPORTED
    x = np.ones((5, h * h, ch), np.float32)
    w = np.ones((classes * ch + 4,), np.float32)
    d_x, d_w = ctx.to_device(x), ctx.to_device(w)
    d_ws, nb = _workspace(ctx, ch, classes)
    outs = [_guarded(ctx, s) for s in (5 * classes, 5 * classes, 5 * 8, 5 * 8)]
    d_l, d_p, d_i, d_v = outs
    lib = ctx.lib

    def tail(n=2, channels=ch, cls=1000, k=5, fc_w=d_w.ptr, ws_bytes=None):
        return lib.mbn_classifier_tail_fused(ctx.h, d_i.ptr, d_v.ptr, d_p.ptr, d_l.ptr, d_x.ptr, fc_w, None, n, h, h, channels, cls, k, d_ws.ptr,
                                             nb if ws_bytes is None else ws_bytes, None)

    def fc(n=2, channels=ch, cls=1000, fc_w=d_w.ptr, ws_bytes=None):
        return lib.mbn_pool_fc(ctx.h, d_l.ptr, d_x.ptr, fc_w, None, n, h, h, channels, cls, d_ws.ptr, nb if ws_bytes is None else ws_bytes, None)

    need = lib.mbn_pool_fc_workspace_bytes(ch, 1000)
    assert tail(k=0) == inv and tail(k=9) == inv
    assert tail(cls=1025) == uns                                             # only the tail keeps an image's logits in LDS
    assert tail(n=5) == uns and fc(n=5) == uns
    assert tail(channels=96) == uns and fc(channels=96) == uns
    assert tail(ws_bytes=need - 4) == inv and fc(ws_bytes=need - 4) == inv
    assert tail(fc_w=d_w.ptr + 4) == uns and fc(fc_w=d_w.ptr + 4) == uns
    assert lib.mbn_pool_fc_workspace_bytes(96, 1000) == 0
    assert lib.mbn_softmax_topk_f32(ctx.h, None, d_i.ptr, d_v.ptr, d_l.ptr, 2, 1000, 0, None) == inv
    assert lib.mbn_softmax_topk_f32(ctx.h, None, d_i.ptr, d_v.ptr, d_l.ptr, 2, 1000, 9, None) == inv
    ctx.sync()
    for o in outs:
        assert (o.download((o.nbytes // 4,), np.uint32) == FF).all(), "a refused call wrote"
    _ws_clean(d_ws, "refused calls")
    # the same calls just inside: the exact workspace size, and 1025 classes for the form without the read-out
    assert tail(ws_bytes=need) == 0 and fc(ws_bytes=need) == 0 and fc(cls=1025) == 0
    ctx.sync()
    assert (d_l.download((2 * 1025,), np.float32) == ch).all()               # the mean of ones times `ch` ones
    _ws_clean(d_ws, "accepted calls")
    for b in [d_x, d_w, d_ws] + outs:
        b.free()
