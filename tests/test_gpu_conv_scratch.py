"""-m gpu: the K-split scratch and the identity matrices of the implicit-GEMM launches belong to the net (ConvScratch, csrc/layers.h),
per stream inside it.  Everything runs the seeded bf16 net at B = 1, the smallest shape at which the K split runs (layer3: 2 views of
28 x 28 in 4 parts on 256 CUs): two nets on one stream and on two, nets created and destroyed in turn, a captured forward of a
re-created net, and one net on two side streams.  Forwards that make the same launches are compared bit for bit."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from gpu_util import conv_plan  # noqa: E402
from test_gpu_at_batch import GATE_BF16, _rel  # noqa: E402
from rgbmanip_amd import _lib, synth  # noqa: E402
from rgbmanip_amd.adapose import AdaPoseNet  # noqa: E402

OUT_KEYS = ["view1_nocs", "view2_nocs", "view1_depth", "view2_depth", "view1_r", "view2_r", "view1_t", "view2_t", "view1_s", "view2_s"]
ARGS = ("img1", "choose1", "img2", "choose2", "P1", "P2", "depths")      # AdaPoseNet.forward's order
DTS = (torch.float32, torch.int32, torch.float32, torch.int32, torch.float32, torch.float32, torch.float32)


@pytest.fixture(scope="module", autouse=True)
def k_split_runs():
    """layer3's conv at one pose (3 x 3, dilation 2, 256 -> 256, pre-activation residual, ReLU) is planned in K parts on this device."""
    p = conv_plan(_lib.BF16, 2, 256, 28, 28, 256, 3, 1, 2, 2, res_mode=1, act=1, n_cu=0)
    if p["parts"] < 2:
        pytest.skip(f"no K split at B = 1 on this device's CU count: {p}")


@pytest.fixture(scope="module")
def sd():
    return synth.adapose_state_dict(seed=0, prefix="module.")


def _device_inputs(B, seed):
    """Inputs already on the device in the forward's types: a forward on a side stream reads them without an upload on another stream."""
    inp = synth.adapose_inputs(B, seed=seed)
    args = [torch.as_tensor(inp[k]).cuda().to(d).contiguous() for k, d in zip(ARGS, DTS)]
    torch.cuda.synchronize()
    return args


@pytest.fixture(scope="module")
def inputs():
    return _device_inputs(1, 0)


def _launch(net, args, stream=None):
    return net(*args, stream=stream)      # not synchronised: the caller decides what is in flight together


def _same(got, want, what):
    for k in OUT_KEYS:
        assert torch.equal(got[k], want[k]), (what, k, float((got[k] - want[k]).abs().max()))


@pytest.fixture(scope="module")
def want(sd, inputs):
    """The eager B = 1 forward of a net that is created for it and destroyed behind it."""
    net = AdaPoseNet(sd, dtype="bf16")
    out = _launch(net, inputs)
    torch.cuda.synchronize()
    out = {k: v.clone() for k, v in out.items()}
    net.close()
    return out


def test_two_nets_on_one_stream_and_on_two(sd, inputs):
    """(a) Two nets with inputs of their own alternate forwards on one stream, then run at the same time on two streams; every result
    is the one that net computes alone.  Their split launches use their own partial sums and arrival counters."""
    other = _device_inputs(1, 1)
    nets = [AdaPoseNet(sd, dtype="bf16"), AdaPoseNet(sd, dtype="bf16")]
    args = [inputs, other]
    alone = []
    for net, a in zip(nets, args):
        out = _launch(net, a)
        torch.cuda.synchronize()
        alone.append({k: v.clone() for k, v in out.items()})
    assert not torch.equal(alone[0]["view1_nocs"], alone[1]["view1_nocs"])      # (the two are told apart)
    one = torch.cuda.Stream()
    got = [(i, _launch(nets[i], args[i], one)) for _ in range(3) for i in (0, 1)]
    torch.cuda.synchronize()
    for n, (i, out) in enumerate(got):
        _same(out, alone[i], f"one stream, forward {n} (net {i})")
    two = [torch.cuda.Stream(), torch.cuda.Stream()]
    got = [(i, _launch(nets[i], args[i], two[i])) for _ in range(3) for i in (0, 1)]
    torch.cuda.synchronize()
    for n, (i, out) in enumerate(got):
        _same(out, alone[i], f"two streams, forward {n} (net {i})")
    for net in nets:
        net.close()


def test_create_run_destroy_three_times(sd, inputs, want):
    """(b) Three times over: a net, one forward on a fresh stream, the net destroyed.  The same bits every time: the counters a new
    net allocates start at zero whatever the one before left behind."""
    for n in range(3):
        net = AdaPoseNet(sd, dtype="bf16")
        stream = torch.cuda.Stream()
        out = _launch(net, inputs, stream)
        stream.synchronize()
        _same(out, want, f"net {n}")
        net.close()


def test_captured_forward_of_a_recreated_net(sd, inputs, want):
    """(c) Behind a destroyed net (`want`'s), a new one captures its B = 1 forward and replays it: the eager result bit for bit, from the
    capture call and from a replay."""
    net = AdaPoseNet(sd, dtype="bf16", graph=True)
    for what in ("capture", "replay"):
        out = _launch(net, inputs)
        torch.cuda.synchronize()
        assert net._last_graph and net.last_graph_nodes > 50, what
        _same(out, want, what)
    net.close()


def test_one_net_on_two_side_streams(sd):
    """(d) split_streams = 2 from B = 2 on: the two poses run as B = 1 forwards of ONE net on two side streams at the same time, each
    stream with the net's scratch for it.  Two references, both the same net on one stream:
     * pose by pose at B = 1 - the launches the split forward makes, one after the other: bit for bit;
     * the two poses as one B = 2 forward: equal as far as two bf16 forwards of different tiles can be.  Four views are planned on other
       tiles and K parts than two (layer3: 2 parts instead of 4, rgbm_conv_plan), so the sums associate differently and bf16 roundings
       fall differently from layer3 on (measured, this commit and its parent alike: view1_nocs differs by up to 2.7e-3, view2_r by
       2.5e-4).  The bound is the one every bf16 forward is held to against the fp32 reference, GATE_BF16 of tests/test_gpu_at_batch.py
       (relative to the output's largest magnitude): both forwards are inside it, so is their difference up to a factor of two - the
       tighter single gate is asserted."""
    args = _device_inputs(2, 0)
    net = AdaPoseNet(sd, dtype="bf16", split_streams=2, split_min_batch=2)
    split = _launch(net, args)
    torch.cuda.synchronize()
    assert net._last_split
    net.split_streams = False
    for b in range(2):
        one = _launch(net, [t[b:b + 1] for t in args])
        torch.cuda.synchronize()
        _same({k: v[b:b + 1] for k, v in split.items()}, one, f"pose {b} alone")
    whole = _launch(net, args)
    torch.cuda.synchronize()
    assert not net._last_split
    for k in OUT_KEYS:
        err = _rel(split[k].cpu().numpy(), whole[k].cpu().numpy())
        print(f"{k}: max |split - one B = 2 forward| / max |.| = {err:.3e}")
        assert err < GATE_BF16[k.split("_")[1]], (k, err)
    net.close()
