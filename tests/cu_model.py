"""The launchers' grid arithmetic and the kernels' tile assignment as pure Python, for any planning CU count.

Every launcher sizes its grid from ctx->num_cus (the planning count: mbn_set_planning_cus), and every persistent kernel derives the tiles a
workgroup (or a wave) walks from blockIdx and gridDim alone. Both are copied here from the sources, with the lines cited (paths relative to
the package's csrc/), so that tests/test_cu_count_cpu.py can show on the CPU, for every count 1..320, that each tile of a launch is taken
exactly once and that no index leaves its range, and so that tests/cu_cases.py can size the GPU cases from conditions instead of measurements.

Vectorised with numpy over the workgroups (and waves) of a launch; the formulas keep the kernels' names. Test infrastructure only; not a conftest.
"""
from __future__ import annotations

import numpy as np


def cdiv(a, b):
    return -(-a // b)


# ----------------------------------------------------------------------------- the strided tile list of a persistent grid

def xcd_remap(vb, nwg):
    """mbn_device.h:29-33 mbn_xcd_remap: virtual block id -> logical tile id; ids that share vb % 8 get a contiguous range."""
    vb = np.asarray(vb)
    q8, r8, xcd = nwg >> 3, nwg & 7, vb & 7
    return np.where(xcd < r8, xcd * (q8 + 1), r8 * (q8 + 1) + (xcd - r8) * q8) + (vb >> 3)


def strided(nwg, grid, remap=True):
    """vb = blockIdx + i * gridDim while vb < nwg (every tile kernel: e.g. mbn_f32_pw.hip:232, 402-403; mbn_bf16_pw_stream.hip:98-99, 337;
    mbn_f32_dwpw.hip:177; mbn_f32_stem.hip:296), each vb through mbn_xcd_remap where the kernel does (all but the stem, which takes t itself).
    Returns (workgroup of every visit, logical tile of every visit, tiles per workgroup by the kernels' own formula
    ntile = (nwg - 1 - blockIdx) / gridDim + 1 — mbn_bf16_pw_stream.hip:99 — or 0 for blockIdx >= nwg)."""
    assert grid >= 1, "a launch needs a workgroup"
    b = np.arange(grid)
    per_wg = np.where(b < nwg, (nwg - 1 - b) // grid + 1, 0)
    wg = np.repeat(b, per_wg)
    i = np.arange(wg.size) - np.repeat(np.cumsum(per_wg) - per_wg, per_wg)
    vb = wg + i * grid
    return wg, (xcd_remap(vb, nwg) if remap else vb), per_wg


def persistent_grid(cus, per_cu, nwg):
    """grid = num_cus * per_cu, clamped to the tiles (mbn_f32_pw.hip:528-530, mbn_f32_dwpw.hip:222-223, mbn_bf16_pw_stream.hip:417-419, ...)"""
    return min(cus * per_cu, nwg)


# (BM, BN, WM, WN) of mbn_f32_pw.hip:698-710 (fp32; 1, 4, 6-10 in the lab build only: a forced tile the shipped library lacks falls to the rule, :669)
PW_GEMM_F32_TILES = {2: (128, 64, 64, 32), 3: (64, 64, 32, 32), 5: (128, 128, 32, 64),
                     1: (128, 128, 64, 64), 4: (256, 128, 64, 64), 6: (128, 256, 64, 64), 7: (64, 128, 32, 64), 8: (128, 64, 32, 64)}
PW_GEMM_BF16_TILES = {3: (64, 128, 32, 64), 5: (128, 128, 32, 64), 2: (128, 64, 64, 32)}       # mbn_f32_pw.hip:679-685 (3 with N < 128: 64 x 64)
SHIPPED_PW_TILES = (2, 3, 5)


def pw_gemm_rule_tile(m, k, n, cus, bf=False):
    """mbn_f32_pw.hip:670-676: the per-layer tile rule (pw_tile = 0)"""
    big_tiles = cdiv(m, 128) * cdiv(n, 64)
    if big_tiles < 2 * cus or n <= 64 or m <= 16384:
        return 3
    if not bf and (k >= 512 or (k >= 256 and n >= 512)):
        return 3
    if (bf or k <= 256) and n >= 128:
        return 5
    return 2


def pw_gemm_plan(m, k, n, cus, cfg, esize=4, pw_xn=0):
    """launch_cfg, mbn_f32_pw.hip:513-541: mt, nt, the k-tile buffers, workgroups per CU, the grid and the XCD-group split xn."""
    bm, bn, wm, wn = cfg
    nt_threads = 64 * (bm // wm) * (bn // wn)
    bke = 8 * (16 // esize)
    mt, nt = cdiv(m, bm), cdiv(n, bn)
    nbuf = 1 if k <= bke else 2
    lds = nbuf * (bm + bn) * 128 + (2 * 1024 * 4 if nbuf == 2 else 0)
    per_cu = min(160 * 1024 // lds, 32 // (nt_threads // 64), 4)
    nwg = mt * nt
    grid = cus * per_cu
    if grid > nwg or nbuf == 1:
        grid = nwg
    filt_bytes = n * k * esize
    xn = 4 if filt_bytes >= 16 * 1048576 else 2 if filt_bytes >= 4 * 1048576 else 1
    if pw_xn > 0:
        xn = pw_xn
    a_xn = xn if (xn in (2, 4) and grid < nwg and grid % 8 == 0 and nt >= xn and mt >= 8 // xn) else 1
    return dict(mt=mt, nt=nt, nwg=nwg, nbuf=nbuf, per_cu=per_cu, grid=grid, xn=a_xn, nk=cdiv(k, bke))


def pw_gemm_visits(p):
    """Every (workgroup, m-tile, n-tile) pw_gemm visits: set_tile, mbn_f32_pw.hip:147-159, with vb_end of :232-240 and the step of :402-403."""
    mt, nt, nwg, grid, xn = p["mt"], p["nt"], p["nwg"], p["grid"], p["xn"]
    if xn == 1:
        wg, lid, per_wg = strided(nwg, grid)
        return wg, lid // nt, lid % nt, per_wg
    xm = 8 // xn
    b = np.arange(grid)
    x = b & 7
    gm, gn = x // xn, x % xn
    mlo, nlo = mt * gm // xm, nt * gn // xn
    nn = nt * (gn + 1) // xn - nlo
    cnt = (mt * (gm + 1) // xm - mlo) * nn
    vb_end = (cnt << 3) + x                                  # vb = 8 j + x < 8 cnt + x  <=>  j < cnt
    per_wg = np.where(b < vb_end, (vb_end - 1 - b) // grid + 1, 0)
    wg = np.repeat(b, per_wg)
    i = np.arange(wg.size) - np.repeat(np.cumsum(per_wg) - per_wg, per_wg)
    vb = wg + i * grid
    assert np.all((vb & 7) == x[wg]), "gridDim is a multiple of 8: a block stays in its XCD group"
    j = vb >> 3
    return wg, mlo[wg] + j // nn[wg], nlo[wg] + j % nn[wg], per_wg


def x6_per_cu(tile):
    """pw_emul's workgroups per CU: launch_xb (tile 11: pre-split filter image) mbn_f32_pw_x6.hip:483-501, launch_x (6, 7) :529-539. -> (BM, BN, per_cu)"""
    pw_words = 16
    if tile == 11:
        bm, bn, wm, wn, occ = 128, 128, 64, 64, 2
        lds = (3 * bm * pw_words + 2 * 3 * bn * pw_words + 4 * bn) * 4
        cap = 1 << 30
    else:
        bm, bn, wm, wn, occ = {6: (128, 128, 64, 64, 2), 7: (128, 64, 64, 32, 3)}[tile]
        lds = 1 * 3 * (bm + bn) * pw_words * 4 + 16 * bn
        cap = 4
    waves = (bm // wm) * (bn // wn)
    return bm, bn, max(1, min(160 * 1024 // lds, occ * 4 // waves, cap))


def stem_plan(batch, rows, cols, c1, bf16, cus):
    """mbn_launch_f32_stem, mbn_f32_stem.hip:568-575 and :607-610: 8 x 16 output tiles, per_cu 2 (fp32, c1 = 32) / 4 (c1 = 16) / 3 / 5 (bf16)."""
    ntiles = batch * (rows // 2 // 8) * (cols // 2 // 16)
    per_cu = (5 if bf16 else 4) if c1 == 16 else (3 if bf16 else 2)
    return dict(nwg=ntiles, per_cu=per_cu, grid=persistent_grid(cus, per_cu, ntiles), nk=1)


# ----------------------------------------------------------------------------- pw3 / dwpw3: XCD-sliced, wave-private tiles

def pw3_grid(tiles, nh, cus):
    """The launchers' per_xcd clamp: mbn_f32_pw3.hip:251 and :264-268; mbn_f32_dwpw3.hip:519 and :552-556. None: outside the envelope
    (num_cus / (8 * nh) < 1 — checked BEFORE per_xcd % nh and g8 / nh divide by a count-derived number)."""
    if cus // (8 * nh) < 1 or tiles < 1:
        return None
    per_xcd = cus // 8
    per_xcd -= per_xcd % nh
    tiles_xcd = (tiles + 7) // 8
    if per_xcd > tiles_xcd * nh:
        per_xcd = tiles_xcd * nh
    return per_xcd * 8


def pw3_visits(tiles, nh, grid, nw=8, mutant=None):
    """mbn_f32_pw3.hip:53-61 (nw = NW waves: 8, or 12 at K = 512) and mbn_f32_dwpw3.hip:101-109 (8 waves): per (workgroup, wave)
    xcd, slice, r0, r1, per_round, full, rem, slot, eslot, ntile and tile_at(i). Returns (slice, tile) of every visit, the per-wave tile
    counts [grid][nw] and the per-XCD (full, rem, per_round).
    mutant "swap": slot used in the remainder round where the kernel uses eslot."""
    b, wave = np.meshgrid(np.arange(grid), np.arange(nw), indexing="ij")
    xcd, j, g8 = b & 7, b >> 3, grid >> 3
    slice_, jm, JM = j % nh, j // nh, g8 // nh
    assert JM >= 1
    r0, r1 = (tiles * xcd) >> 3, (tiles * (xcd + 1)) >> 3
    per_round = JM * nw
    full = (r1 - r0) // per_round
    rem = (r1 - r0) - full * per_round
    slot, eslot = jm * nw + wave, wave * JM + jm
    ntile = full + (eslot < rem)
    n = ntile.ravel()
    idx = np.repeat(np.arange(n.size), n)
    i = np.arange(idx.size) - np.repeat(np.cumsum(n) - n, n)
    f = lambda a: np.broadcast_to(a, b.shape).ravel()[idx]
    last = f(slot) if mutant == "swap" else f(eslot)
    tile = np.where(i < f(full), f(r0) + i * per_round + f(slot), f(r0) + f(full) * per_round + last)
    per_xcd = [(int(full[x, 0]), int(rem[x, 0]), per_round) for x in range(min(8, grid))]
    return f(slice_), tile, ntile, per_xcd


# ----------------------------------------------------------------------------- rf: pixel streams per XCD

def rf_plan(mt, nh, cus):
    """mbn_bf16_pw_rf.hip:185 (the envelope: num_cus >= 8 * nh, before gq divides) and :196-206. None outside the envelope."""
    if cus < 8 * nh or mt < 1:
        return None
    gq = cus // 8 // nh
    gq = gq if mt >= 8 * gq else (mt + 7) // 8
    return dict(gq=gq, grid=8 * nh * gq)


def rf_visits(mt, nh, gq, grid):
    """mbn_bf16_pw_rf.hip:60-64: xcd, slot, half, grp, t0, tstep, nt; tile ti of a stream is t0 + ti * tstep (:73). -> (half, tile) of every visit, nt per workgroup"""
    b = np.arange(grid)
    xcd, slot = b & 7, b >> 3
    half, grp = slot % nh, slot // nh
    t0, tstep = xcd + 8 * grp, 8 * gq
    nt = np.where(t0 >= mt, 0, (mt - 1 - t0) // tstep + 1)
    idx = np.repeat(b, nt)
    ti = np.arange(idx.size) - np.repeat(np.cumsum(nt) - nt, nt)
    return half[idx], t0[idx] + ti * tstep, nt


# ----------------------------------------------------------------------------- resident blocks / tail, pool + FC, conv1, depthwise segments

def res_visits(batch, cus):
    """mbn_bf16_res.hip:284-286 (grid = min(num_cus, batch)) and :117 (n = blockIdx; n += gridDim). -> images visited, per workgroup count"""
    grid = min(cus, batch)
    wg, n, per_wg = strided(batch, grid, remap=False)
    return n, per_wg, grid


def tail_visits(batch, cus):
    """mbn_bf16_tail.hip:284-286 (grid = min(num_cus, (batch + 1) / 2): two images per pass) and :137 (n0 = 2 blockIdx; n0 += 2 gridDim)."""
    grid = min(cus, (batch + 1) // 2)
    wg, pas, per_wg = strided((batch + 1) // 2, grid, remap=False)
    n0 = 2 * pas
    imgs = np.concatenate([n0, n0[n0 + 1 < batch] + 1])
    return imgs, per_wg, grid


def poolfc_plan(channels, classes, cus):
    """mbn_launch_f32_pool_fc, mbn_f32_misc.hip:710-717: K slices of 64 channels x class ranges of npc (a multiple of 16)."""
    nks = channels // 64
    nns = min(cdiv(cus, nks), 64, cdiv(classes, 16))
    npc = cdiv(cdiv(classes, nns), 16) * 16
    nns = cdiv(classes, npc)
    return dict(nks=nks, nns=nns, npc=npc, grid=nks * nns)


def poolfc_visits(p, classes):
    """poolfc_f32, mbn_f32_misc.hip:347 (ks = blockIdx % nks, ns = blockIdx / nks) and :373 (n_lo, n_hi). -> (ks, n_lo, n_hi) per workgroup"""
    b = np.arange(p["grid"])
    ks, ns = b % p["nks"], b // p["nks"]
    n_lo = ns * p["npc"]
    return ks, n_lo, np.minimum(classes, n_lo + p["npc"])


def conv1_mfma_visits(nblk, cus):
    """mbn_f32_misc.hip:651-656 (4 waves per workgroup, at most 8 workgroups per CU) and :196 (blk = global wave; blk += waves)."""
    wgs = min(cdiv(nblk, 4), cus * 8)
    return strided(nblk, 4 * wgs, remap=False)[1], wgs


def dw_march_segments(row_lanes, rows, stride, cache_resident, cus, dw_nseg=0):
    """mbn_f32_dw.h:56-68 dw_march_segments, then launch_dw's nseg -> (seg_rows, nseg), mbn_f32_dw.hip:698-701 and :745-747."""
    target = cus * 64 * (12 if stride == 1 else 6)
    nseg = 1
    if dw_nseg > 0:
        nseg = dw_nseg
    elif row_lanes < target:
        nseg = cdiv(target, row_lanes)
        max_seg = rows // 4 if rows // 4 > 0 else 1
        if row_lanes * max_seg < cus * 64 or cache_resident:
            max_seg = rows
        nseg = min(nseg, max_seg)
    nseg = min(nseg, rows)
    seg_rows = cdiv(rows, nseg)
    return seg_rows, cdiv(rows, seg_rows)


def dw_lds_bf16_segments(batch, rows, cols, channels, cus, nseg_force=0):
    """launch_dw_lds_bf16, mbn_f32_dw.hip:437-453 (slots = 2 * num_cus). -> (seg_rows, nseg), or None outside the form's envelope (SW > 64)"""
    sw = (cols + 3) & ~1
    if sw > 64:
        return None
    base = cdiv(batch, 64 // sw) * (channels // 64)
    slots = 2 * cus
    ns = 1
    if nseg_force > 0:
        ns = nseg_force
    elif base * 10 < slots * 6:
        ns = cdiv(slots, base)
        if ns > rows // 2:
            ns = rows // 2 if rows // 2 > 0 else 1
    seg_rows = cdiv(rows, ns)
    return seg_rows, cdiv(rows, seg_rows)


def dw_lds_f32_segments(batch, rows, cols, stride, channels, ch64, la, cus, nseg_force=0):
    """launch_dw_lds, mbn_f32_dw.hip:619-643 (slots = num_cus * (160 / ring_kb); the cost search over k <= rows / 8). -> (seg_rows, nseg)"""
    px = 32 if ch64 else 64
    tw = px - 2 if stride == 1 else (px - 1) // 2
    nstrip = cdiv(cols, tw)
    nslab = channels // (64 if ch64 else 32)
    lao = (6 if la else 3) if stride == 1 else (3 if la else 2)
    ring_kb = 8 * (stride * lao + 3)
    slots = cus * (160 // ring_kb)
    base = batch * nslab * nstrip
    ns = 1
    if nseg_force > 0:
        ns = nseg_force
    elif base > slots or base * 10 < slots * 6:
        best = 1e30
        for k in range(1, min(rows // 8, 16) + 1):
            sr = cdiv(rows, k)
            kk = cdiv(rows, sr)
            w = base * kk / slots
            rounds = max(w, 0.6) if w <= 1.0 else float(np.ceil(w))
            cost = rounds / w * (1.0 + 0.5 / sr)
            if cost < best - 1e-9:
                best, ns = cost, k
    ns = min(ns, rows)
    seg_rows = cdiv(rows, ns)
    return seg_rows, cdiv(rows, seg_rows)


# ----------------------------------------------------------------------------- count-dependent envelopes and choices of the dispatch

def splitk_taken(m, k, n, batch, cus, mode=0):
    """mbn_launch_f32_pw_splitk, mbn_f32_pw_splitk.hip:123-139 (aligned operands). -> the workgroup tile's TB (1: 16 x 16, 2: 32 x 32; :144) or None"""
    if mode == 1 or k < 128 or k % 64 or m <= 0 or m > 65536:
        return None
    one_px = batch >= 1 and m == batch
    if mode not in (2, 16, 32) and not one_px:
        if batch < 1 or batch > 4 or m % batch:
            return None
        m4 = m // batch * 4
        if cdiv(m4, 64) * cdiv(n, 64) * 2 > cus:
            return None
    return 1 if mode == 16 else 2 if mode == 32 else (2 if cdiv(m, 16) * cdiv(n, 16) > 2 * cus else 1)


def pw3_default(m, k, n, cus):
    """MBN_PW3_DEFAULT, mbn_internal.h:229"""
    return k <= 256 and n <= 256 and m >= 128 * cus


def big_tiles(m, n, cus):
    """mbn_launch_bf16_pw_big, mbn_bf16_pw_stream.hip:453-459: whole rounds of whole row tiles; 0 = outside the envelope"""
    nt, mt = n // 256, m // 256
    tiles = (mt * nt // cus) * cus
    tiles -= tiles % nt
    return tiles if tiles >= cus else 0


def net_block_fused_f32(count, out_rows, out_cols, out_ch, cus):
    """block_fusable's few-tiles rule, host/mbn_net.c:354-358 (fp32, default mask)"""
    return cdiv(count * out_rows * out_cols, 128) * cdiv(out_ch, 128) * 2 >= cus
