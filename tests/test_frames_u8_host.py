"""CPU-only: the 8-bit frame entry points (rgbm_prepare_inputs_u8, rgbm_quantize_frames) are declared, exported and bound, the
controller refuses an unknown queue dtype, and the numerical contract of a byte (b means fl32(b / 255), quantise -> dequantise is the
identity on bytes) holds in its numpy restatement."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def quantize_ref(x):
    """rgbm_quantize_frames restated: min(max(rint(x * 255), 0), 255) in float32, round half to even, NaN -> 0."""
    x = np.asarray(x, dtype=np.float32)
    with np.errstate(all="ignore"):
        q = np.clip(np.rint(x * np.float32(255)), 0, 255)
    return np.where(np.isnan(x), np.float32(0), q).astype(np.uint8)


def test_symbols_are_declared_exported_and_bound():
    from rgbmanip_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rgbm.h")).read(), flags=re.S)
    lib = _lib.load()
    vp, i = C.c_void_p, C.c_int
    want = {"rgbm_prepare_inputs_u8": [vp, vp, vp, vp, i, i, i, i, i, i, C.c_uint32, vp, vp, vp, vp, vp, vp, vp, vp],
            "rgbm_quantize_frames": [vp, vp, C.c_size_t, vp]}
    for name, argtypes in want.items():
        assert re.search(r"\bint\s+" + name + r"\s*\(", src), f"{name} is not declared in include/rgbm.h"
        assert name in _lib.SIGNATURES, f"{name} is not bound in _lib.SIGNATURES"
        fn = getattr(lib, name)                                  # AttributeError: the built library does not export it
        assert fn.restype is C.c_int and list(fn.argtypes) == argtypes, (name, fn.argtypes)
    # the byte entry point takes rgbm_prepare_inputs_ex's arguments
    assert _lib.SIGNATURES["rgbm_prepare_inputs_u8"][1] == _lib.SIGNATURES["rgbm_prepare_inputs_ex"][1]
    decl = re.search(r"int\s+rgbm_prepare_inputs_u8\s*\(([^)]*)\)", src).group(1)
    assert re.match(r"\s*const\s+uint8_t\s*\*\s*rgb_dev", decl), decl


def test_unknown_queue_dtype_is_refused_at_construction():
    from rgbmanip_amd import synth
    from rgbmanip_amd.control_interface import ControlInterface
    env = types.SimpleNamespace(num_envs=2)
    est = types.SimpleNamespace(cfg={"task_name": "cabinet"})
    for bad in ("int8", "float16", "bytes", None):
        cfg = synth.control_cfg("cabinet", 0.0)
        cfg["controller"]["hip_queue_dtype"] = bad
        with pytest.raises(ValueError, match="hip_queue_dtype"):
            ControlInterface(env, est, None, cfg, device="cpu")
    with pytest.raises(ValueError, match="hip_queue_dtype"):
        ControlInterface.queue_only(2, est, 4, device="cpu", queue_dtype="int8")


def test_quantise_restatement_round_trips_every_byte():
    b = np.arange(256, dtype=np.uint8)
    deq = b.astype(np.float32) / np.float32(255)                # what a byte means
    # ... which the fp64 quotient rounded to float32 gives for every byte (the kernel's conversion)
    assert np.array_equal(deq, (b.astype(np.float64) / 255.0).astype(np.float32))
    assert np.array_equal(quantize_ref(deq), b)
    assert quantize_ref([np.nan, -1.0, -0.0, 0.0, 2.0, np.inf, -np.inf]).tolist() == [0, 0, 0, 0, 255, 255, 0]
    assert np.rint(np.float32([0.5, 1.5, 2.5])).tolist() == [0.0, 2.0, 2.0]      # ties go to even
