"""-m gpu: what one forward wants travels with the call (AdaPose::Call, csrc/adapose.h), not through members of the net: a dense call
leaves the handle as it found it (also when it fails), rgbm_adapose_dense_workspace_bytes is a plain query, the hipGraph cache is keyed on
the capture stream, and the per-sample-BatchNorm and generic chunk bodies of cost_volume() walk two chunks like the default one."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

from rgbmanip_amd import _lib, synth  # noqa: E402
from rgbmanip_amd.adapose import AdaPoseNet  # noqa: E402

OUT_KEYS = ["view1_nocs", "view2_nocs", "view1_depth", "view2_depth", "view1_r", "view2_r", "view1_t", "view2_t", "view1_s", "view2_s"]
MAP_KEYS = ["view1_depth_map", "view1_depth_conf", "view2_depth_map", "view2_depth_conf"]
DTS = (torch.float32, torch.float32, torch.int32, torch.int32, torch.float32, torch.float32, torch.float32)
C_ORDER = ("img1", "img2", "choose1", "choose2", "P1", "P2", "depths")      # the C ABI's argument order


@pytest.fixture(scope="module")
def sd():
    return synth.adapose_state_dict(seed=0, prefix="module.")


@pytest.fixture(scope="module")
def golden_inputs():
    return synth.adapose_inputs(2, seed=0)        # the batch tests/golden/adapose_b2*.npz were recorded on


def _call(net, inp, **kw):
    out = net(inp["img1"], inp["choose1"], inp["img2"], inp["choose2"], inp["P1"], inp["P2"], inp["depths"], **kw)
    torch.cuda.synchronize()
    return {k: v.clone() for k, v in out.items()}


def _device_args(inp):
    return [torch.as_tensor(inp[k]).cuda().to(d).contiguous() for k, d in zip(C_ORDER, DTS)]


class _generic_kernels_only:
    """Every conv launch on the generic tiles (rgbm_set_tuning ws_min_rows = 2^30), as tests/test_gpu_dropout.py pins the selection to
    compare batches of different sizes bit for bit: the persistent kernels' dispatch depends on the number of rows."""
    def __enter__(self):
        _lib.check(_lib.load().rgbm_set_tuning(b"ws_min_rows", 1 << 30))

    def __exit__(self, *a):
        _lib.check(_lib.load().rgbm_set_tuning(b"ws_min_rows", 0))


# ------------------------------------------------------------------------------------------------------------------ 1. the net is left alone
def test_dense_calls_leave_the_net_alone_also_on_failure(sd, golden_inputs):
    """bf16, default options, B = 2 in two chunks: a plain forward, a dense depth + NOCS call, a raw rgbm_adapose_forward_maps call that
    fails on its workspace size, a plain forward again - the two plain forwards' ten outputs are bit-identical, and a 3-D tap is refused
    under the sparse cost regularisation after the dense calls with the message it had before them."""
    net = AdaPoseNet(sd, dtype="bf16", max_chunk_views=2)
    lib = _lib.load()

    def refusal():
        with pytest.raises(_lib.RgbmError, match="needs a dense cost regularisation") as e:
            net.fetch(2, "c0", 8)
        return str(e.value)
    before = _call(net, golden_inputs)
    msg = refusal()
    dense = _call(net, golden_inputs, dense_depth=True, dense_nocs=True)
    assert sorted(dense) == sorted(OUT_KEYS + MAP_KEYS + ["view1_nocs_map", "view2_nocs_map"])
    t = _device_args(golden_inputs)
    out = net._empty_outputs(2)
    o = _lib.AdaposeOut(*[out[n].data_ptr() for n, _ in _lib.AdaposeOut._fields_])
    maps = torch.zeros(2, 4, 224, 224, device="cuda")
    nmap = torch.zeros(4, 224, 224, 3, device="cuda")
    need = net.workspace_bytes(2)
    ws = torch.empty(need + 256, dtype=torch.uint8, device="cuda")
    ptr, _ = net._aligned(ws)
    rc = lib.rgbm_adapose_forward_maps(net._h, 2, *[_lib.ptr(x) for x in t], C.c_void_p(ptr), need - 256, C.byref(o), _lib.ptr(maps[0]),
                                       _lib.ptr(maps[1]), _lib.ptr(nmap), _lib.stream_ptr())
    assert rc < 0 and b"workspace too small" in lib.rgbm_last_error()
    torch.cuda.synchronize()
    assert float(maps.abs().max()) == 0.0 and float(nmap.abs().max()) == 0.0      # nothing ran
    after = _call(net, golden_inputs)
    assert sorted(after) == sorted(OUT_KEYS)
    for k in OUT_KEYS:
        assert torch.equal(before[k], after[k]), k
    assert refusal() == msg


# ------------------------------------------------------------------------------------------------------------------ 2. workspace sizes
@pytest.mark.parametrize("dtype", ["bf16", "bf16x3", "fp32"])
def test_dense_workspace_bytes_is_the_plain_size_and_a_pure_query(sd, dtype):
    """rgbm_adapose_dense_workspace_bytes(B) == rgbm_adapose_workspace_bytes(B) at B = 1 and 3 for sparse_dec in {0, 2} x sparse_tail in
    {0, 1} (the plan holds u11 whatever the options say), and asking does not change the next forward's outputs."""
    inp = synth.adapose_inputs(1, seed=0)
    for sparse_dec in (0, 2):
        for sparse_tail in (0, 1):
            net = AdaPoseNet(sd, dtype=dtype, sparse_tail=sparse_tail, options={"sparse_dec": sparse_dec})
            before = _call(net, inp)
            for B in (1, 3):
                assert net.dense_workspace_bytes(B) == net.workspace_bytes(B), (sparse_dec, sparse_tail, B)
            after = _call(net, inp)
            for k in OUT_KEYS:
                assert torch.equal(before[k], after[k]), (sparse_dec, sparse_tail, k)
            net.close()


# ------------------------------------------------------------------------------------------------------------------ 3. graph cache and stream
def test_graph_cache_is_keyed_on_the_capture_stream(sd):
    """Raw rgbm_adapose_forward_graph at B = 1 with one set of buffers: stream A captures, A again replays, stream B captures a graph of
    its own instead of replaying A's (whose launches use A's K-split scratch), then A and B each replay their own.  All results equal an eager
    forward bit for bit.  Every call is synchronised before the next: the two streams are never in flight together."""
    inp = synth.adapose_inputs(1, seed=0)
    net = AdaPoseNet(sd, dtype="bf16")
    lib = _lib.load()
    want = _call(net, inp)
    t = _device_args(inp)
    out = net._empty_outputs(1)
    o = _lib.AdaposeOut(*[out[n].data_ptr() for n, _ in _lib.AdaposeOut._fields_])
    ws = torch.empty(net.workspace_bytes(1) + 256, dtype=torch.uint8, device="cuda")
    ptr, nbytes = net._aligned(ws)
    A, B = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    for name, stream, expect in (("A", A, 1), ("A again", A, 0), ("B", B, 1), ("A after B", A, 0), ("B again", B, 0)):
        for v in out.values():
            v.zero_()
        torch.cuda.synchronize()
        nodes, captured = C.c_int32(), C.c_int32()
        _lib.check(lib.rgbm_adapose_forward_graph(net._h, 1, *[_lib.ptr(x) for x in t], C.c_void_p(ptr), nbytes, C.byref(o),
                                                  C.c_void_p(stream.cuda_stream), C.byref(nodes), C.byref(captured)), "rgbm_adapose_forward_graph")
        stream.synchronize()
        assert captured.value == expect, (name, captured.value)
        assert nodes.value > 50, name
        for k in OUT_KEYS:
            assert torch.equal(out[k], want[k]), (name, k)


# ------------------------------------------------------------------------------------------------------------------ 4. the other chunk bodies
@pytest.mark.parametrize("dtype,kw", [("fp32", dict(norm_mode=1)), ("bf16", dict(cost_impl=0))], ids=["norm_mode=1", "cost_impl=0"])
def test_two_chunks_of_the_other_bodies_equal_single_pose_calls(sd, dtype, kw):
    """The pattern of tests/test_gpu_dense_depth.py::test_two_chunks_equal_single_pose_calls for the per-sample-BatchNorm body and the
    generic implicit-GEMM body: B = 2 with max_chunk = 2 views walks the chunk loop twice (views 0-1, then 2-3) and writes rows v0 .. v0 + Vc
    of the maps; row by row the maps and the ten outputs equal single-pose calls bit for bit (kernel selection pinned; per-sample
    BatchNorm normalises per view, so the other view of a chunk does not enter)."""
    inp = synth.adapose_inputs(2, seed=5)
    with _generic_kernels_only():
        out = _call(AdaPoseNet(sd, dtype=dtype, max_chunk_views=2, **kw), inp, dense_depth=True)
        net1 = AdaPoseNet(sd, dtype=dtype, **kw)
        bad = []
        for b in range(2):
            o1 = _call(net1, {k: v[b:b + 1] for k, v in inp.items()}, dense_depth=True)
            for k in MAP_KEYS + OUT_KEYS:
                diff = float((out[k][b:b + 1] - o1[k]).abs().max())
                print(f"{dtype} {kw} pose {b} {k}: max |difference| {diff:.3e}")
                if not torch.equal(out[k][b:b + 1], o1[k]):
                    bad.append((b, k, diff))
    assert not bad, bad
