"""CPU-only: rgbm_conv_border_plan (the host table of the border-class tiles, conv_plan.cpp) against a brute-force numpy enumeration.

Output pixels of a dilated 3 x 3 conv whose set of in-range taps is the same form a class; a tile is 256 rows of one class taken across
views and walks only that class's taps.  The table covers the GEMM rows of the 256 x 256 launch (rgbm_conv_plan's main_rows: whole rounds
of the persistent grid); the rows behind them keep the tail launch they had.  The plan is a pure function of the shape and the workgroup
count, so everything here runs without a GPU (n_cu > 0)."""
import ctypes as C

import numpy as np
import pytest

from rgbmanip_amd import _lib

HEAD = ("taken", "classes", "tiles", "n_wg", "rows", "max_wg_steps", "total_steps", "parent_steps", "steps_per_tap", "res_steps")
CIN = COUT = 256
SHAPES = [(28, 28, 2), (28, 28, 4), (28, 28, 1), (7, 9, 4)]
VIEWS = [1, 3, 96, 512]


def border_plan(V, H, W, dil, *, k=3, stride=1, pad=None, cin=CIN, cout=COUT, res_mode=0, n_cu=256, dtype=None):
    lib = _lib.load()
    dtype = _lib.BF16 if dtype is None else dtype
    pad = dil * (k // 2) if pad is None else pad
    head = (C.c_int32 * len(HEAD))()
    args = (dtype, V, H, W, cin, cout, k, stride, pad, dil, res_mode, n_cu)
    _lib.check(lib.rgbm_conv_border_plan(*args, head, None, 0, None, None, 0, None, 0, None, 0), "rgbm_conv_border_plan")
    h = dict(zip(HEAD, head))
    if not h["taken"]:
        return h
    cls = (C.c_int32 * (3 * h["classes"]))()
    tiles = (C.c_int32 * (5 * h["tiles"]))()
    order = (C.c_int32 * h["tiles"])()
    wg_off = (C.c_int32 * (h["n_wg"] + 1))()
    rows = (C.c_int32 * h["rows"])()
    _lib.check(lib.rgbm_conv_border_plan(*args, head, cls, h["classes"], tiles, order, h["tiles"], wg_off, h["n_wg"] + 1, rows, h["rows"]),
               "rgbm_conv_border_plan")
    h["class_info"] = np.array(cls, dtype=np.int64).reshape(-1, 3)      # pixels per view, mask, first row
    h["tile_info"] = np.array(tiles, dtype=np.int64).reshape(-1, 5)     # class, channel tile, mask, steps, first row
    h["order"] = np.array(order, dtype=np.int64)
    h["wg_off"] = np.array(wg_off, dtype=np.int64)
    h["row_map"] = np.array(rows, dtype=np.int64)
    return h


def main_rows(V, H, W, dil, n_cu, k=3, stride=1, pad=None, cin=CIN, cout=COUT):
    lib = _lib.load()
    pad = dil * (k // 2) if pad is None else pad
    out = (C.c_int32 * 9)()
    _lib.check(lib.rgbm_conv_plan(_lib.BF16, V, 1, H, W, cin, cin, cout, cout, 1, k, k, 1, stride, 0, pad, dil, 0, 0, 0, 1, 0, n_cu, out),
               "rgbm_conv_plan")
    return out[4] if out[0] == 7 else 0


def pixel_masks(H, W, dil, k=3):
    """tap mask (bit kh * k + kw) of every output pixel of a stride-1 conv with pad = dil * (k // 2), by enumeration"""
    pad = dil * (k // 2)
    m = np.zeros((H, W), dtype=np.int64)
    for h in range(H):
        for w in range(W):
            for kh in range(k):
                for kw in range(k):
                    y, x = h - pad + kh * dil, w - pad + kw * dil
                    if 0 <= y < H and 0 <= x < W:
                        m[h, w] |= 1 << (kh * k + kw)
    return m


def n_cu_for(V, H, W):
    """256 workgroups where the launch fills them; the small shapes are planned for an 8-CU device"""
    return 256 if V * H * W // 256 >= 256 else 8


@pytest.mark.parametrize("V", VIEWS)
@pytest.mark.parametrize("shape", SHAPES, ids=[f"{h}x{w}_dil{d}" for h, w, d in SHAPES])
def test_plan_matches_enumeration(shape, V):
    H, W, dil = shape
    n_cu = n_cu_for(V, H, W)
    p = border_plan(V, H, W, dil, n_cu=n_cu)
    M = main_rows(V, H, W, dil, n_cu)
    if M == 0:
        assert not p["taken"]          # below the persistent 256 x 256 path: nothing to re-order
        return
    masks = pixel_masks(H, W, dil)
    flat = masks.reshape(-1)
    assert M % 256 == 0 and M <= V * H * W
    row_mask = np.tile(flat, V)[:M]    # the tap mask of every GEMM row of the 256 x 256 launch
    # few views: the dead rows that pad every class to whole tiles can cost more taps than the classes save; then the plan declines
    class_taps = sum(-(-int(n) // 256) * bin(int(m)).count("1") for m, n in zip(*np.unique(row_mask, return_counts=True)))
    if class_taps >= M // 256 * 9:
        assert not p["taken"], (shape, V)
        return
    assert p["taken"], (shape, V)
    ci, ti, rows = p["class_info"], p["tile_info"], p["row_map"]
    # classes: one per distinct mask, with the enumerated pixel count
    uniq, counts = np.unique(masks, return_counts=True)
    assert sorted(ci[:, 1].tolist()) == sorted(uniq.tolist())
    for n_pix, mask, _ in ci:
        assert n_pix == counts[uniq.tolist().index(mask)]
    # every (view, pixel) of the launch in exactly one live row
    live = rows[rows >= 0]
    assert live.size == M
    assert np.array_equal(np.sort(live), np.arange(M))
    # class layout: padded to whole tiles, rows in (view, class pixel) order with the class's pixels row-major, cut at the launch's last row
    row0 = 0
    padded_of = {}
    for c, (n_pix, mask, first) in enumerate(ci):
        assert first == row0
        pix = np.flatnonzero(flat == mask)
        want = (np.arange(V)[:, None] * (H * W) + pix[None, :]).reshape(-1)
        want = want[want < M]
        padded = padded_of[c] = -(-want.size // 256) * 256
        seg = rows[row0:row0 + padded]
        assert np.array_equal(seg[:want.size], want) and (seg[want.size:] == -1).all()
        row0 += padded
    assert row0 == p["rows"] == rows.size
    # tiles: 256 rows of one class; the mask is the intersection and the union of its live rows' masks; steps = taps * Cin / 64
    assert p["steps_per_tap"] == CIN // 64 and p["res_steps"] == 0
    seen = set()
    for t, (cls, ch, mask, steps, first) in enumerate(ti):
        assert first % 256 == 0 and 0 <= ch < COUT // 256
        assert (first, ch) not in seen
        seen.add((first, ch))
        r = rows[first:first + 256]
        r = r[r >= 0]
        assert r.size > 0
        m = flat[r % (H * W)]
        assert np.bitwise_and.reduce(m) == mask == np.bitwise_or.reduce(m) == ci[cls, 1]
        assert ci[cls, 2] <= first < ci[cls, 2] + padded_of[cls]
        assert steps == bin(mask).count("1") * (CIN // 64)
    assert len(seen) == (p["rows"] // 256) * (COUT // 256) == p["tiles"]
    assert p["total_steps"] == ti[:, 3].sum()
    assert p["parent_steps"] == M // 256 * (COUT // 256) * 9 * (CIN // 64)
    assert p["total_steps"] < p["parent_steps"]
    # the order: every tile once; the busiest workgroup within one tile of the mean
    assert p["n_wg"] == n_cu and p["wg_off"][0] == 0 and p["wg_off"][-1] == p["tiles"]
    assert np.array_equal(np.sort(p["order"]), np.arange(p["tiles"]))
    totals = []
    for b in range(n_cu):
        totals.append(int(ti[p["order"][p["wg_off"][b]:p["wg_off"][b + 1]], 3].sum()))
    assert max(totals) == p["max_wg_steps"]
    if n_cu == 256:
        assert p["max_wg_steps"] - p["total_steps"] / n_cu <= ti[:, 3].max()


@pytest.mark.parametrize("dil,ratio", [(4, 0.819), (2, 0.907)])
def test_step_ratio_at_512_views(dil, ratio):
    """Σ steps / (tiles · 9 · Cin/64) is the valid-tap fraction averaged over the taps and the 784 pixels: no dead rows at V = 512.  (On
    224 workgroups the 1568 tiles are seven whole rounds, so the 256 x 256 launch has every row; on 256 the last 32 tiles are the tail's.)"""
    p = border_plan(512, 28, 28, dil, n_cu=224)
    assert p["taken"] and p["rows"] == 512 * 784
    got = p["total_steps"] / (p["tiles"] * 9 * (CIN // 64))
    f = (28 - dil) / 28
    assert got == pytest.approx((1 + 4 * f + 4 * f * f) / 9, abs=1e-12)
    assert round(got, 3) == ratio
    assert p["total_steps"] / p["parent_steps"] == pytest.approx(got, abs=1e-12)


def test_residual_steps_are_counted_per_tile():
    p0 = border_plan(512, 28, 28, 4, cin=512, cout=512, n_cu=224)
    p1 = border_plan(512, 28, 28, 4, cin=512, cout=512, res_mode=1, n_cu=224)
    assert p0["taken"] and p1["taken"] and p1["res_steps"] == 4 and p0["res_steps"] == 0
    assert np.array_equal(p1["tile_info"][:, 3], p0["tile_info"][:, 3] + 4)
    assert p1["tile_info"][:, 3].max() == 9 * 8 + 4 and p1["tile_info"][:, 3].min() == 4 * 8 + 4
    # class sizes of dilation 4 on 28 x 28: the interior, four edges, four corners
    assert sorted(p1["class_info"][:, 0].tolist()) == [16] * 4 + [80] * 4 + [400]


def test_plan_declines():
    assert not border_plan(512, 28, 28, 1, k=1, pad=0)["taken"]                      # 1 x 1
    assert not border_plan(512, 56, 56, 2, stride=2)["taken"]                        # stride 2
    assert not border_plan(8, 28, 28, 4)["taken"]                                    # a small batch: 128-pixel tiles
    assert not border_plan(512, 28, 28, 1, pad=0)["taken"]                           # no padding: no tap to save
    assert not border_plan(512, 28, 28, 4, dtype=_lib.F32)["taken"]                  # fp32 has no 256 x 256 kernel
    assert not border_plan(512, 28, 28, 4, cout=128)["taken"]                        # 128 channels: another kernel
    lib = _lib.load()
    try:
        lib.rgbm_debug_flags(32)
        assert not border_plan(512, 28, 28, 4)["taken"]                              # the A/B switch
    finally:
        lib.rgbm_debug_flags(0)
    assert border_plan(512, 28, 28, 4)["taken"]
