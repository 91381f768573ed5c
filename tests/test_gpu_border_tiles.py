"""-m gpu: the border-class tiles of conv_igemm_m32_kernel<T, 256, 256> (rgbm_conv_border_plan; debug flag 32 runs the row-major tiles).

A tile of one border class walks only the taps that are in range for its rows.  The skipped K steps multiplied finite weights by the
zeros of the padding, so every output must keep its bits; the float64 bound is the one tests/test_gpu_kernels.py holds this kernel to."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from rgbmanip_amd import _lib  # noqa: E402

NO_BORDER = 32
TOL = {_lib.BF16: 2.5e-2, _lib.F16: 4e-3}      # tests/test_gpu_kernels.py TOL
CH, HW = 256, 28


@functools.lru_cache(maxsize=None)
def first_views(dil):
    """the smallest V whose launch reaches the 256 x 256 tiles on this device (one whole round of the persistent grid)"""
    from gpu_util import conv_plan, KERNEL_M32
    for V in range(1, 4096):
        p = conv_plan(_lib.BF16, V, CH, HW, HW, CH, 3, 1, dil, dil, res_mode=1, act=1)
        if p["kernel"] == KERNEL_M32 and p["main_rows"] > 0:
            return V
    raise AssertionError("no batch reaches the 256 x 256 tiles")


@functools.lru_cache(maxsize=None)
def operands(dil, dtype):
    """rounded operands for first_views + 5 views (the smaller case takes the first views of the same tensors) and the float64 conv"""
    from gpu_util import quantise
    V = first_views(dil) + 5
    g = torch.Generator().manual_seed(100 * dil + dtype)
    x = quantise(torch.randn(V, CH, HW, HW, generator=g), dtype)
    w = quantise(torch.randn(CH, CH, 3, 3, generator=g) / np.sqrt(CH * 9), dtype)
    res = quantise(torch.randn(V, CH, HW, HW, generator=g), dtype)
    ref = F.conv2d(x.double(), w.double(), None, 1, dil, dil)
    return x, w, res, ref


def launches(fn):
    """fn(): (its result, how many launches it ran on border-class tiles)"""
    lib = _lib.load()
    a, b = C.c_int64(), C.c_int64()
    _lib.check(lib.rgbm_conv_border_launches(C.byref(a)), "rgbm_conv_border_launches")
    out = fn()
    torch.cuda.synchronize()
    _lib.check(lib.rgbm_conv_border_launches(C.byref(b)), "rgbm_conv_border_launches")
    return out, b.value - a.value


def run_both(dtype, x, w, res, dil):
    """the same call on border-class tiles (default) and with the switch set; raw device outputs and the launch counts of each"""
    from gpu_util import conv_nd_launcher
    lib = _lib.load()
    launch, fetch = conv_nd_launcher(dtype, x, w, stride=1, pad=dil, dil=dil, res=res, res_mode=1 if res is not None else 0, act=1)
    on, n_on = launches(launch)
    try:
        lib.rgbm_debug_flags(NO_BORDER)
        off, n_off = launches(launch)
    finally:
        lib.rgbm_debug_flags(0)
    return on, off, n_on, n_off, fetch


@pytest.mark.parametrize("with_res", [False, True], ids=["nores", "res"])
@pytest.mark.parametrize("dtype", [_lib.BF16, _lib.F16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("dil", [2, 4])
@pytest.mark.parametrize("extra", [0, 5], ids=["one_round", "ragged"])
def test_border_tiles_keep_every_bit(extra, dil, dtype, with_res):
    from gpu_util import rel_err
    V = first_views(dil) + extra
    x, w, res, ref = operands(dil, dtype)
    x, res, ref = x[:V], (res[:V] if with_res else None), ref[:V]
    on, off, n_on, n_off, fetch = run_both(dtype, x, w, res, dil)
    # the default ran the 256 x 256 launch on border-class tiles, the switch ran it row-major; both leave the rest to a tail launch
    from gpu_util import conv_plan
    p = conv_plan(dtype, V, CH, HW, HW, CH, 3, 1, dil, dil, res_mode=int(with_res), act=1)
    assert n_on == 1 and n_off == 0 and 0 < p["main_rows"] < p["M"] and p["tail_bch"]
    assert torch.equal(on.view(torch.int16), off.view(torch.int16))
    want = F.relu(ref + res.double()) if with_res else F.relu(ref)
    y = fetch(on)
    assert torch.isfinite(y).all()
    err = rel_err(y, want)
    print(f"V={V} dil={dil} dtype={dtype} res={with_res}: rel err {err:.3e} (bound {TOL[dtype]})")
    assert err < TOL[dtype]


@pytest.mark.parametrize("dtype", [_lib.BF16, _lib.F16], ids=["bf16", "fp16"])
def test_nan_weight_declines(dtype):
    """NaN * 0 is the one product a skipped padding tap would change: a layer whose weights hold a non-finite value runs the row-major
    tiles whatever the switch says, and gives the same bits"""
    dil = 4
    V = first_views(dil) + 5
    x, w, res, _ = operands(dil, dtype)
    w = w.clone()
    w[3, 5, 0, 2] = float("nan")
    on, off, n_on, n_off, fetch = run_both(dtype, x[:V], w, res[:V], dil)
    assert n_on == 0 and n_off == 0      # the plan declined
    assert torch.equal(on.view(torch.int16), off.view(torch.int16))
    y = fetch(on)
    assert torch.isnan(y[:, 3]).any() and torch.isfinite(y[:, 4]).all()
