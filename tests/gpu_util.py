"""Helpers shared by the -m gpu parity tests (device layout conversion, error metrics)."""
import ctypes as C

import numpy as np
import torch

from rgbmanip_amd import _lib

# BF16X3 tensors are raw 4-byte slots (int32): 16-byte chunks of 4 channels {hi01, hi23, lo01, lo23} (include/rgbm.h)
TORCH_DT = {_lib.F32: torch.float32, _lib.BF16: torch.bfloat16, _lib.F16: torch.float16, _lib.BF16X3: torch.int32}


def bx3_round(x):
    """fp32 -> the value a BF16X3 slot holds: bf16(x) + bf16(x - bf16(x))."""
    hi = x.float().bfloat16().float()
    return hi + (x.float() - hi).bfloat16().float()


def bx3_pack(x):
    """[..., C] fp32 (C % 4 == 0) -> int32 tensor of the same shape in the split-pair chunk layout."""
    x = x.float().contiguous()
    assert x.shape[-1] % 4 == 0
    hi = x.bfloat16()
    lo = (x - hi.float()).bfloat16()
    h = hi.view(torch.int16).to(torch.int32).bitwise_and(0xffff).reshape(*x.shape[:-1], -1, 4)
    l = lo.view(torch.int16).to(torch.int32).bitwise_and(0xffff).reshape(*x.shape[:-1], -1, 4)
    w = torch.stack([h[..., 0] | (h[..., 1] << 16), h[..., 2] | (h[..., 3] << 16),
                     l[..., 0] | (l[..., 1] << 16), l[..., 2] | (l[..., 3] << 16)], dim=-1)
    return w.reshape(x.shape).to(torch.int32)


def bx3_unpack(w):
    """inverse of bx3_pack: int32 [..., C] -> fp32 values hi + lo."""
    w = w.to(torch.int64).bitwise_and(0xffffffff).reshape(*w.shape[:-1], -1, 4)

    def f32_bits(u):    # 32-bit pattern held in an int64 -> fp32
        return (u - ((u >> 31) << 32)).to(torch.int32).view(torch.float32)

    def halves(d):      # dword -> (low half, high half), each a bf16 bit pattern widened to fp32
        return f32_bits((d & 0xffff) << 16), f32_bits(d & 0xffff0000)
    a0, a1 = halves(w[..., 0])
    a2, a3 = halves(w[..., 1])
    b0, b1 = halves(w[..., 2])
    b2, b3 = halves(w[..., 3])
    out = torch.stack([a0 + b0, a1 + b1, a2 + b2, a3 + b3], dim=-1)
    return out.reshape(*out.shape[:-2], -1)


def quantise(x, dtype):
    """fp32 -> the fp32 value the storage type keeps (identity for F32)."""
    if dtype == _lib.F32:
        return x
    if dtype == _lib.BF16X3:
        return bx3_round(x)
    return x.to(TORCH_DT[dtype]).float()


def empty_out(shape, dtype, fill=float("nan")):
    """device output tensor in the storage type; float types are pre-filled (NaN by default) to catch unwritten elements."""
    if dtype == _lib.BF16X3:
        return torch.full(tuple(shape), 0x7fc07fc0, dtype=torch.int32, device="cuda")      # NaN hi halves
    return torch.full(tuple(shape), fill, dtype=TORCH_DT[dtype], device="cuda")


def rel_err(a, b):
    a = torch.as_tensor(a).double().cpu()
    b = torch.as_tensor(b).double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-12))


def to_channels_last(x, dtype, cpad=None):
    """[N,C,*spatial] fp32 (cpu) -> device [N,*spatial,Cpad] in dtype."""
    nd = x.dim()
    perm = [0] + list(range(2, nd)) + [1]
    y = x.permute(*perm).contiguous()
    C_ = y.shape[-1]
    if cpad and cpad > C_:
        y = torch.nn.functional.pad(y, (0, cpad - C_))
    if dtype == _lib.BF16X3:
        return bx3_pack(y).to("cuda").contiguous()
    return y.to("cuda", TORCH_DT[dtype]).contiguous()


def from_channels_last(y, C_=None):
    """device [N,*spatial,Cpad] -> cpu fp32 [N,C,*spatial]."""
    y = bx3_unpack(y.cpu()) if y.dtype == torch.int32 else y.float().cpu()
    if C_ is not None:
        y = y[..., :C_]
    nd = y.dim()
    perm = [0, nd - 1] + list(range(1, nd - 1))
    return y.permute(*perm).contiguous()


def host_f32(a):
    if a is None:
        return None, C.c_void_p(0)
    arr = np.ascontiguousarray(a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a, dtype=np.float32)
    return arr, C.c_void_p(arr.ctypes.data)


def conv_nd_launcher(dtype, x, w, *, stride=1, stride_d=None, pad=0, pad_d=None, dil=1, transposed=False, bias=None, bn_scale=None,
                     bn_shift=None, res=None, res_mode=0, act=0, slope=0.0, cin_pad=None, cout_pad=None):
    """Uploads the operands of a HIP conv (arguments as conv_nd) and returns (launch, fetch): launch() runs rgbm_conv_nd on the current
    stream into a fresh NaN-filled output and returns it (device, channels-last); fetch(out) -> cpu fp32 [N,Cout,...]."""
    lib = _lib.load()
    is2d = x.dim() == 4
    if is2d:
        x = x.unsqueeze(2)
        w = w.unsqueeze(2)
        if res is not None:
            res = res.unsqueeze(2)
    N, Cin, D, H, W = x.shape
    if transposed:
        Cout = w.shape[1]
        KD, KH, KW = w.shape[2:]
        Do, Ho, Wo = 2 * D, 2 * H, 2 * W
    else:
        Cout = w.shape[0]
        KD, KH, KW = w.shape[2:]
        sd = stride_d if stride_d is not None else (1 if is2d else stride)
        pd = pad_d if pad_d is not None else (0 if is2d else pad)
        Do = (D + 2 * pd - (KD - 1) - 1) // sd + 1
        Ho = (H + 2 * pad - dil * (KH - 1) - 1) // stride + 1
        Wo = (W + 2 * pad - dil * (KW - 1) - 1) // stride + 1
    E = 4 if dtype in (_lib.F32, _lib.BF16X3) else 8
    cin_pad = cin_pad or (Cin + E - 1) // E * E
    cout_pad = cout_pad or (Cout + 3) // 4 * 4
    xd = to_channels_last(x, dtype, cin_pad)
    rd = to_channels_last(res, dtype, cout_pad) if res is not None else None
    wa, wp = host_f32(w)
    ba, bp = host_f32(bias)
    sa, sp = host_f32(bn_scale)
    ha, hp = host_f32(bn_shift)
    sd = stride_d if stride_d is not None else (1 if is2d else stride)
    pd = pad_d if pad_d is not None else (0 if is2d else pad)

    def launch():
        out = empty_out((N, Do, Ho, Wo, cout_pad), dtype)
        keep = (wa, ba, sa, ha)      # noqa: F841  (host arrays alive for the call)
        rc = lib.rgbm_conv_nd(dtype, _lib.ptr(xd), N, D, H, W, Cin, cin_pad, wp, Cout, cout_pad, KD, KH, KW,
                              2 if transposed else sd, 2 if transposed else stride, 1 if transposed else pd,
                              1 if transposed else pad, dil, int(transposed), bp, sp, hp, _lib.ptr(rd), res_mode, act, slope,
                              _lib.ptr(out), _lib.stream_ptr())
        _lib.check(rc, "rgbm_conv_nd")
        return out

    def fetch(out):
        y = from_channels_last(out, Cout)
        return y.squeeze(2) if is2d else y
    return launch, fetch


def conv_nd(dtype, x, w, **kw):
    """x [N,C,D,H,W] or [N,C,H,W] cpu fp32; w torch layout.  Returns cpu fp32 [N,Cout,...] via the HIP conv."""
    launch, fetch = conv_nd_launcher(dtype, x, w, **kw)
    torch.cuda.synchronize()
    out = launch()
    torch.cuda.synchronize()
    return fetch(out)


# ---------------------------------------------------------------- what the library would launch
PLAN_FIELDS = ("kernel", "bch", "bpix", "parts", "main_rows", "tail_bch", "identity", "M", "KT")      # rgbm_conv_plan's array (include/rgbm.h)
KERNEL_WS_SLIM, KERNEL_M32, KERNEL_M32_SMALL = 4, 7, 8


def device_n_cu(device=0):
    """persistent_grid_cus(): the device's compute units rounded down to a multiple of the 8 XCDs (at least 8)."""
    return max(torch.cuda.get_device_properties(device).multi_processor_count // 8 * 8, 8)


def conv_out_hw(H, W, k, stride, pad, dil):
    return (H + 2 * pad - dil * (k - 1) - 1) // stride + 1, (W + 2 * pad - dil * (k - 1) - 1) // stride + 1


def conv_plan(dtype, N, Cin, H, W, Cout, k, stride, pad, dil, has_bias=False, res_mode=0, act=0, n_cu=0):
    """rgbm_conv_plan for a 2-D conv as conv_nd launches it (channels padded the same way), under the process's current debug flags and
    tuning; n_cu = 0 asks the current device, a positive value needs no GPU.  Returns the array as a dict (PLAN_FIELDS)."""
    E = 4 if dtype in (_lib.F32, _lib.BF16X3) else 8
    out = (C.c_int32 * len(PLAN_FIELDS))()
    _lib.check(_lib.load().rgbm_conv_plan(dtype, N, 1, H, W, Cin, (Cin + E - 1) // E * E, Cout, (Cout + 3) // 4 * 4, 1, k, k, 1, stride, 0, pad,
                                          dil, 0, int(has_bias), res_mode, act, 0, n_cu, out), "rgbm_conv_plan")
    return dict(zip(PLAN_FIELDS, out))


def conv_case_plan(case, dtype, n_cu):
    """The library's plan for a conv case (name, N, Cin, H, W, Cout, k, stride, pad, dil, bias, act, res_mode) as conv_nd launches it.
    Returns a dict: tile (channels, pixels) of a small launch - the 128-pixel tiles of conv_igemm_m32_kernel, or the 64 x 256 tile of
    conv_igemm_ws_kernel kept for a layer of more than 64 channels - else None; parts; M; KT; and the residual path of a 128-pixel small
    launch ('epilogue': the Cout = 128 tile adds it after the reduction; 'identity': 256-multiple channels add a pre-activation residual
    by identity K steps)."""
    _, N, Cin, H, W, Cout, k, stride, pad, dil, has_bias, act, res_mode = case
    p = conv_plan(dtype, N, Cin, H, W, Cout, k, stride, pad, dil, has_bias, res_mode, act, n_cu)
    small = p["kernel"] == KERNEL_M32_SMALL
    tile = (p["bch"], p["bpix"]) if small or (p["kernel"] == KERNEL_WS_SLIM and Cout > 64) else None
    res = ("identity" if p["identity"] else "epilogue") if small and res_mode else None
    return {"M": p["M"], "KT": p["KT"], "tile": tile, "parts": p["parts"], "res": res}


def _backbone_small_cases():
    # ResNet-34 layer2..4 as PSPNet runs them (oracle/adapose_ref.py RESNET34_LAYERS) on a 28 x 28 feature map (layer2's block 0 reads
    # layer1's 56 x 56), at 2 .. 16 views = 1 .. 8 poses
    shapes = [
        # tag, Cin, H, Cout, k, stride, pad, dil, act, res_mode
        ("l2_b0_conv1", 64, 56, 128, 3, 2, 1, 1, 1, 0),
        ("l2_b0_down", 64, 56, 128, 1, 2, 0, 1, 0, 0),
        ("l2_conv2_res", 128, 28, 128, 3, 1, 1, 1, 1, 1),
        ("l3_b0_conv1", 128, 28, 256, 3, 1, 1, 1, 1, 0),
        ("l3_b0_down", 128, 28, 256, 1, 1, 0, 1, 0, 0),
        ("l3_conv2_res", 256, 28, 256, 3, 1, 2, 2, 1, 1),
        ("l4_b0_conv1", 256, 28, 512, 3, 1, 1, 1, 1, 0),
        ("l4_b0_down", 256, 28, 512, 1, 1, 0, 1, 0, 0),
        ("l4_conv2_res", 512, 28, 512, 3, 1, 4, 4, 1, 1),
    ]
    out = []
    for tag, Cin, H, Cout, k, s, p, d, act, rm in shapes:
        for N in (2, 4, 6, 8, 10, 16):
            out.append((f"{tag}_n{N}", N, Cin, H, H, Cout, k, s, p, d, False, act, rm))
    return out


SMALL_CONV_CASES = _backbone_small_cases() + [
    # synthetic (1x1: the only multi-K-step convs with a Cin that is not a power of two): K loops that do not divide into their parts
    # (25 / 50 K steps in 2, 3 or 4 parts: part p starts at p * KT / n, the parts differ in length), post-activation residuals, biases
    ("syn_1x1_cin1600_post_n2", 2, 1600, 28, 28, 128, 1, 1, 0, 1, True, 1, 2),
    ("syn_1x1_cin1600_post_n8", 8, 1600, 28, 28, 128, 1, 1, 0, 1, True, 2, 2),
    ("syn_1x1_cin1600_c256_res_n2", 2, 1600, 28, 28, 256, 1, 1, 0, 1, False, 1, 1),
    ("syn_1x1_cin1600_c256_post_n4", 4, 1600, 28, 28, 256, 1, 1, 0, 1, True, 2, 2),
]
