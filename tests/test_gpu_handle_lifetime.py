"""-m gpu: device memory of a handle belongs to the objects that use it (csrc/layers.h: DevBuf) - a create that is refused half way
frees what it had uploaded, close() twice is harmless, nets are destroyed in any order without touching each other, and a one-shot
entry point that was refused leaves the next call what it was.  B = 1 forwards only; every failure here is a refused call with an error
code, none is a fault."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from rgbmanip_amd import _lib, synth  # noqa: E402
from rgbmanip_amd.adapose import AdaPoseNet  # noqa: E402

OUT_KEYS = ["view1_nocs", "view2_nocs", "view1_depth", "view2_depth", "view1_r", "view2_r", "view1_t", "view2_t", "view1_s", "view2_s"]


@pytest.fixture(scope="module")
def inputs():
    return synth.adapose_inputs(1, seed=0)


@pytest.fixture(scope="module")
def sd_v5():
    return synth.adapose_state_dict(seed=0, prefix="module.")


def _bytes(net, inp):
    """the ten outputs of one B = 1 forward, as bytes"""
    out = net(inp["img1"], inp["choose1"], inp["img2"], inp["choose2"], inp["P1"], inp["P2"], inp["depths"])
    torch.cuda.synchronize()
    assert sorted(out) == sorted(OUT_KEYS)
    return {k: out[k].cpu().numpy().tobytes() for k in OUT_KEYS}


@pytest.mark.parametrize("arch,key", [("v5", "size_estimator.4.bias"), ("baseline", "depth_head.4.weight")])
def test_refused_create_frees_the_partly_built_net(arch, key, inputs, sd_v5):
    """A state dict without a key that create() reads late: the create is refused with `missing weight <key>` after most of the net was
    uploaded (the destructor of the partly built net runs), and a net built afterwards from the full dict gives the ten outputs of the net
    built before the refusal."""
    sd = sd_v5 if arch == "v5" else synth.baseline_state_dict(seed=0)
    kw = dict(dtype="bf16", arch=arch)
    before = AdaPoseNet(sd, **kw)
    ref = _bytes(before, inputs)
    before.close()
    short = {k: v for k, v in sd.items() if not k.endswith(key)}
    assert len(short) == len(sd) - 1
    with pytest.raises(_lib.RgbmError, match="missing weight " + key.replace(".", r"\.")):
        AdaPoseNet(short, **kw)
    after = AdaPoseNet(sd, **kw)
    assert _bytes(after, inputs) == ref
    after.close()


def test_close_twice_is_harmless(inputs, sd_v5):
    net = AdaPoseNet(sd_v5, dtype="bf16")
    _bytes(net, inputs)
    net.close()
    net.close()
    other = AdaPoseNet(sd_v5, dtype="bf16")      # the device is as usable as before
    _bytes(other, inputs)
    other.close()
    other.close()


@pytest.mark.parametrize("close_first", [0, 1])
def test_nets_are_destroyed_in_any_order(close_first, inputs, sd_v5):
    """Two nets of different storage types alive at once: closing one (the first built, then in the other case the second built) leaves the
    other's next forward bit for bit what it was before."""
    nets = [AdaPoseNet(sd_v5, dtype="bf16"), AdaPoseNet(sd_v5, dtype="fp32")]
    before = [_bytes(n, inputs) for n in nets]
    keep = 1 - close_first
    nets[close_first].close()
    assert _bytes(nets[keep], inputs) == before[keep]
    nets[keep].close()


def test_one_shot_entry_after_a_refusal():
    """rgbm_conv3d_tile with a layer id outside the table is refused (-1) before anything is uploaded; the valid call behind it gives the
    bytes of the same call made before.  Shape: the one tests/test_gpu_kernels.py::test_conv3d_tile_layers uses."""
    from gpu_util import empty_out, host_f32, to_channels_last
    lib = _lib.load()
    layer, dtype, (Cin, Cout) = 1, _lib.BF16, (8, 16)
    N, D, H, W = 3, 6, 20, 12
    g = torch.Generator().manual_seed(101)
    xd = to_channels_last(torch.randn(N, Cin, D, H, W, generator=g), dtype)
    wa, wp = host_f32(torch.randn(Cout, Cin, 3, 3, 3, generator=g) / (Cin * 27) ** 0.5)
    sa, sp = host_f32(torch.rand(Cout, generator=g) + 0.5)
    ha, hp = host_f32(torch.randn(Cout, generator=g) * 0.1)

    def run(layer_id):
        out = empty_out((N, D // 2, H // 2, W // 2, Cout), dtype)
        rc = lib.rgbm_conv3d_tile(layer_id, dtype, _lib.ptr(xd), N, D, H, W, wp, sp, hp, _lib.ptr(None), _lib.ptr(out), _lib.stream_ptr())
        torch.cuda.synchronize()
        return rc, out.cpu().view(torch.int16).numpy().tobytes()

    rc, first = run(layer)
    assert rc == 0
    assert not torch.isnan(torch.frombuffer(bytearray(first), dtype=torch.bfloat16)).any()
    rc, _ = run(10)
    assert rc == -1 and b"conv3d_tile arguments" in lib.rgbm_last_error()
    rc, second = run(layer)
    assert rc == 0 and second == first
