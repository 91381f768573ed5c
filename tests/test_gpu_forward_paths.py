"""-m gpu: a handle reports the facts of its next forward and the paths that forward runs (rgbm_adapose_paths), they are what the pure
decision (rgbm_forward_paths) makes of those facts, and what a forward leaves behind - the feature map's element form, the refusal of
the 3-D taps, the workspace size - is what the paths say.  B = 1, seeded random weights."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from rgbmanip_amd import _lib, synth  # noqa: E402
from rgbmanip_amd.adapose import AdaPoseNet  # noqa: E402

from forward_paths_ref import FACTS, N_FACTS, N_PATHS, PATHS  # noqa: E402

DTYPES = ("bf16", "bf16x3", "fp32", "fp16")
OPTION_SETS = ({}, {"sparse_dec": 0}, {"sweep_f16": 0}, {"cost_impl": 1}, {"upconv": 0}, {"stem": 0})
I32P = C.POINTER(C.c_int32)
_nets = {}


def _net(dtype):
    """One handle per storage type for the whole module; `options` below sets and restores what a case changes."""
    if dtype not in _nets:
        _nets[dtype] = AdaPoseNet(synth.adapose_state_dict(seed=0, prefix="module."), dtype=dtype)
    return _nets[dtype]


class options:
    def __init__(self, net, opts):
        self.net, self.opts = net, opts
        self.defaults = {"sparse_dec": 2, "sweep_f16": 1, "cost_impl": 3, "upconv": 7, "stem": int(net.dtype_name != "fp32")}

    def _set(self, values):
        for k, v in values.items():
            _lib.check(self.net.lib.rgbm_adapose_set_option(self.net._h, k.encode(), int(v)), "rgbm_adapose_set_option")
        self.net._ws = None      # the plan follows the options: the next forward asks for its size again

    def __enter__(self):
        self._set(self.opts)
        return self.net

    def __exit__(self, *a):
        self._set({k: self.defaults[k] for k in self.opts})


def handle_paths(net, B=1, dense=0):
    facts, paths = np.zeros(N_FACTS, np.int32), np.zeros(N_PATHS, np.int32)
    _lib.check(net.lib.rgbm_adapose_paths(net._h, B, dense, facts.ctypes.data_as(I32P), paths.ctypes.data_as(I32P)), "rgbm_adapose_paths")
    return dict(zip(FACTS, facts)), dict(zip(PATHS, paths)), facts, paths


@pytest.fixture(scope="module")
def inp():
    return synth.adapose_inputs(1, seed=3)


def _forward(net, inp, **kw):
    net(inp["img1"], inp["choose1"], inp["img2"], inp["choose2"], inp["P1"], inp["P2"], inp["depths"], **kw)
    torch.cuda.synchronize()


def _feat(net):
    return net.fetch(1, "feat", 2 * 224 * 224 * 32).cpu()


@pytest.mark.parametrize("dtype", DTYPES)
def test_handle_paths_are_the_pure_decision_on_the_handles_facts(dtype):
    net = _net(dtype)
    for opts in OPTION_SETS:
        if "sweep_f16" in opts and dtype != "bf16":
            continue
        with options(net, opts):
            for dense in (0, 1):
                f, p, facts, paths = handle_paths(net, 1, dense)
                assert (f["dtype"], f["dense"], f["V"], f["Vh"], f["n_pts"], f["flags"]) == (net.dtype, dense, 2, 2, 1024, 0)
                assert all(f[k] == v for k, v in opts.items()), (opts, f)
                again = np.zeros(N_PATHS, np.int32)
                _lib.check(net.lib.rgbm_forward_paths(facts.ctypes.data_as(I32P), 1, again.ctypes.data_as(I32P)), "rgbm_forward_paths")
                assert np.array_equal(again, paths), (opts, dense, f, p)
                assert p["tail_sparse"] == 0 or not dense


@pytest.mark.parametrize("dtype", DTYPES)
def test_workspace_query_does_not_move_around_a_forward(dtype, inp):
    net = _net(dtype)
    before = net.workspace_bytes(1)
    _forward(net, inp)
    assert net.workspace_bytes(1) == before


@pytest.mark.parametrize("dtype", DTYPES)
def test_feat_tap_has_the_form_the_paths_report(dtype, inp):
    """The tap is the fp32 copy of whatever `final` wrote.  An f16 value has up to 11 significand bits, a bf16 value 8 (the low 16 bits of
    its fp32 copy are zero: the criterion of test_gpu_adapose.py::test_f16_feature_map_only_for_weights_that_fit_f16).  Siblings: the
    sparse cost regularisation does not touch the PSPNet (bit-identical features); sweep_f16 = 0 stores the same features as bf16, within
    the 2.0e-2 of the maximum that test_gpu_adapose.py::test_bf16_sweep_conv0_vs_tile_conv0 allows between the f16 and the bf16 features' c0."""
    net = _net(dtype)
    form = handle_paths(net)[1]["feat_form"]
    assert form == {"bf16": 2, "bf16x3": 1, "fp32": 0, "fp16": 0}[dtype]
    _forward(net, inp, stop_after=1)
    feat = _feat(net)
    assert torch.isfinite(feat).all() and float(feat.abs().max()) > 0
    low_bits = bool((feat.view(torch.int32) & 0xFFFF).any())
    if dtype == "bf16":
        assert low_bits                                       # f16
    with options(net, {"sparse_dec": 0}):
        assert handle_paths(net)[1]["feat_form"] == form
        _forward(net, inp, stop_after=1)
        assert torch.equal(_feat(net), feat)
    if dtype == "bf16":
        with options(net, {"sweep_f16": 0}):
            assert handle_paths(net)[1]["feat_form"] == 0
            _forward(net, inp, stop_after=1)
            bf = _feat(net)
            assert not bool((bf.view(torch.int32) & 0xFFFF).any())      # bf16
            assert float((bf - feat).abs().max() / feat.abs().max()) < 2.0e-2


@pytest.mark.parametrize("dtype", DTYPES)
def test_3d_taps_are_refused_exactly_under_tile_masks(dtype, inp):
    """test_gpu_adapose.py::test_3d_taps_are_refused_under_sparse_cost_regularisation through the paths: c0 is refused exactly when the
    forward skipped tiles of it."""
    net = _net(dtype)
    n = 2 * 24 * 224 * 224 * 8
    seen = set()
    for opts in ({}, {"sparse_dec": 0}, {"cost_impl": 1}):
        with options(net, opts):
            level = handle_paths(net)[1]["mask_level"]
            seen.add(level > 0)
            _forward(net, inp, stop_after=2)
            if level > 0:
                with pytest.raises(_lib.RgbmError, match="sparse_dec"):
                    net.fetch(1, "c0", n)
            else:
                assert net.fetch(1, "c0", n).numel() == n
    assert seen == ({False} if dtype == "fp32" else {True, False})
