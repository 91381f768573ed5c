"""CPU-only: the 8-bit synthetic camera entry point (rgbm_synth_render_u8) is declared, exported and bound; the env refuses an unknown
color_dtype and the controller refuses hip_render_to_queue where it cannot work (a float32 queue, an env without render_into)."""
import ctypes as C
import os
import re
import types

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbol_is_declared_exported_and_bound():
    from rgbmanip_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rgbm.h")).read(), flags=re.S)
    name, vp = "rgbm_synth_render_u8", C.c_void_p
    assert re.search(r"\bint\s+" + name + r"\s*\(", src), f"{name} is not declared in include/rgbm.h"
    assert name in _lib.SIGNATURES, f"{name} is not bound in _lib.SIGNATURES"
    fn = getattr(_lib.load(), name)                              # AttributeError: the built library does not export it
    assert fn.restype is C.c_int and list(fn.argtypes) == [C.POINTER(_lib.SynthScene), vp, vp, vp, vp, vp, vp], fn.argtypes
    decl = re.search(r"int\s+" + name + r"\s*\(([^)]*)\)", src).group(1)
    assert re.search(r"uint8_t\s*\*\s*color_dev.*uint8_t\s*\*\s*mask_dev.*int32_t\s*\*\s*extent_dev.*int32_t\s*\*\s*count_dev", decl, re.S), decl


def test_unknown_color_dtype_is_refused():
    from rgbmanip_amd.synthetic_env import SyntheticMultiVecEnv
    for bad in ("int8", "float16", "bytes", None):
        with pytest.raises(ValueError, match="color_dtype"):     # before anything touches a device
            SyntheticMultiVecEnv(2, "cpu", color_dtype=bad)


def test_render_to_queue_is_refused_where_it_cannot_work():
    from rgbmanip_amd import synth
    from rgbmanip_amd.control_interface import ControlInterface
    est = types.SimpleNamespace(cfg={"task_name": "cabinet"})

    def cfg(queue_dtype):
        c = synth.control_cfg("cabinet", 0.0)
        c["controller"]["hip_render_to_queue"] = True
        if queue_dtype is not None:
            c["controller"]["hip_queue_dtype"] = queue_dtype
        return c
    with_render = types.SimpleNamespace(num_envs=2, render_into=lambda *a: None)
    without = types.SimpleNamespace(num_envs=2, get_image=lambda: None)
    for queue_dtype in (None, "float32"):                        # the float32 queue (also the default) cannot take the camera's bytes
        with pytest.raises(ValueError, match="hip_render_to_queue"):
            ControlInterface(with_render, est, None, cfg(queue_dtype), device="cpu")
    with pytest.raises(ValueError, match="hip_render_to_queue"):  # the reference's MultiVecEnv, a numpy view of an env, ...
        ControlInterface(without, est, None, cfg("uint8"), device="cpu")
