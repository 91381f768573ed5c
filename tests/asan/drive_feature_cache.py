"""Drives the feature cache's host side under AddressSanitizer (subprocess of tests/test_feature_cache_host.py; numpy only).

Same set-up as tests/asan/drive_host.py (RGBM_HIP_LIB = the host-only ASan build, "device" memory is host memory, kernel launches do
nothing): rgbm_adapose_feature_bytes / features_workspace_bytes / features / forward_cached in every storage type and norm mode —
the record layout per option, the workspace planner for odd and small V, the part loops of the store and the gather, the chunk loop
behind the seam, and the refusals (Dropout2d on, a workspace that is too small, a misaligned pool)."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from rgbmanip_amd import _lib, synth  # noqa: E402

assert "asan_host" in os.environ.get("RGBM_HIP_LIB", ""), "run through tests/test_feature_cache_host.py"
lib = _lib.load()
sd = synth.adapose_state_dict(seed=0, prefix="module.")
S, ONE = 224, 224 * 224 * 32


def create(dtype, norm_mode):
    keep, descs = [], []
    for k, v in sd.items():
        a = np.asarray(v)
        if a.dtype.kind != "f":
            continue
        a = np.ascontiguousarray(a, dtype=np.float32)
        shape, nd = (C.c_int64 * max(a.ndim, 1))(*(a.shape or (1,))), a.ndim
        name = k.encode()
        keep.append((a, shape, name))
        descs.append(_lib.WeightDesc(name, a.ctypes.data, nd, shape))
    arr = (_lib.WeightDesc * len(descs))(*descs)
    h = C.c_void_p()
    _lib.check(lib.rgbm_adapose_create(C.byref(h), 0, arr, len(descs), dtype, norm_mode), "create")
    return h


def vp(a):
    return C.c_void_p(a.ctypes.data)


def aligned(nbytes, align=256):
    buf = np.empty(nbytes + align, dtype=np.uint8)
    return buf, buf.ctypes.data + ((-buf.ctypes.data) % align)


def feature_bytes(h):
    n = C.c_size_t()
    _lib.check(lib.rgbm_adapose_feature_bytes(h, C.byref(n)), "feature_bytes")
    return n.value


def features(h, V, pool_base, records, slots, shrink=0):
    n = C.c_size_t()
    _lib.check(lib.rgbm_adapose_features_workspace_bytes(h, V, C.byref(n)), "features_workspace_bytes")
    ws, base = aligned(n.value)
    img = np.zeros((V, 3, S, S), np.float32)
    sl = np.asarray(slots, np.int32)
    return lib.rgbm_adapose_features(h, V, vp(img), vp(sl), C.c_void_p(pool_base), records, C.c_void_p(base), n.value - shrink, None), ws


def forward_cached(h, B, pool_base, records):
    n = C.c_size_t()
    _lib.check(lib.rgbm_adapose_workspace_bytes(h, B, C.byref(n)), "workspace_bytes")
    ws, base = aligned(n.value)
    inp = synth.adapose_inputs(B, seed=1)
    ch1, ch2 = (np.ascontiguousarray(inp[k], dtype=np.int32) for k in ("choose1", "choose2"))
    P1, P2, dep = (np.ascontiguousarray(inp[k], dtype=np.float32) for k in ("P1", "P2", "depths"))
    s1, s2 = np.arange(B, dtype=np.int32), np.arange(B, dtype=np.int32)[::-1].copy() + B
    outs = [np.empty(s, np.float32) for s in ((B, 1024, 3), (B, 1024, 3), (B, 1024), (B, 1024), (B, 3, 3), (B, 3, 3), (B, 3), (B, 3),
                                              (B, 3), (B, 3))]
    out = _lib.AdaposeOut(*[o.ctypes.data for o in outs])
    return lib.rgbm_adapose_forward_cached(h, B, C.c_void_p(pool_base), records, vp(s1), vp(s2), vp(ch1), vp(ch2), vp(P1), vp(P2), vp(dep),
                                           C.c_void_p(base), n.value, C.byref(out), None)


runs = 0
expect = {(_lib.F32, 0): 4, (_lib.F32, 1): 4, (_lib.BF16, 0): 2, (_lib.F16, 0): 2, (_lib.BF16X3, 0): 4, (_lib.BF16X3, 1): 8}
for (dtype, nm), per in expect.items():
    h = create(dtype, nm)
    fb = feature_bytes(h)
    assert fb == ONE * per, (dtype, nm, fb)
    records = 7
    pool, pbase = aligned(records * fb)
    for V, slots in ((1, [6]), (3, [4, 0, 2]), (6, [0, 1, 2, 3, 4, 5])):
        rc, _ = features(h, V, pbase, records, slots)
        assert rc == 0, lib.rgbm_last_error()
    assert forward_cached(h, 3, pbase, records) == 0, lib.rgbm_last_error()
    _lib.check(lib.rgbm_adapose_set_chunk(h, 2), "set_chunk")                 # 6 views in chunks of 2 behind the seam
    assert forward_cached(h, 3, pbase, records) == 0, lib.rgbm_last_error()
    _lib.check(lib.rgbm_adapose_set_option(h, b"view2_heads", 0), "set_option")
    assert forward_cached(h, 2, pbase, records) == 0, lib.rgbm_last_error()
    if dtype == _lib.BF16X3 and nm == 0:      # the halo-tile conv0 reads the split-pair map: the record grows to both maps
        _lib.check(lib.rgbm_adapose_set_option(h, b"cost_impl", 2), "set_option")
        assert feature_bytes(h) == ONE * 8
        _lib.check(lib.rgbm_adapose_set_option(h, b"cost_impl", 3), "set_option")
    if dtype == _lib.BF16:                    # sweep_f16 = 0: a bf16 map, the same size
        _lib.check(lib.rgbm_adapose_set_option(h, b"sweep_f16", 0), "set_option")
        assert feature_bytes(h) == ONE * 2
    # refusals: workspace one byte short, misaligned pool, Dropout2d on
    rc, _ = features(h, 2, pbase, records, [0, 1], shrink=1)
    assert rc != 0 and b"workspace too small" in lib.rgbm_last_error()
    rc, _ = features(h, 2, pbase + 4, records - 1, [0, 1])
    assert rc != 0 and b"aligned" in lib.rgbm_last_error()
    _lib.check(lib.rgbm_adapose_set_dropout(h, 0.15, 7), "set_dropout")
    rc, _ = features(h, 2, pbase, records, [0, 1])
    assert rc != 0 and b"Dropout2d" in lib.rgbm_last_error()
    assert forward_cached(h, 2, pbase, records) != 0 and b"Dropout2d" in lib.rgbm_last_error()
    _lib.check(lib.rgbm_adapose_set_dropout(h, 0.0, 0), "set_dropout")
    rc, _ = features(h, 2, pbase, records, [0, 1])
    assert rc == 0, lib.rgbm_last_error()
    _lib.check(lib.rgbm_adapose_destroy(h), "destroy")
    runs += 1
print("ASAN_FEATURE_CACHE_OK", runs, "configurations")
