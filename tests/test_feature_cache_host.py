"""CPU-only checks of the feature cache (DESIGN.md "Feature cache"): the C ABI exports its entry points, `ControlInterface` tells
the estimator exactly which queue rows are new, the estimator refuses the cache together with Dropout2d, and the host side of the new
entry points is clean under AddressSanitizer."""
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

from rgbmanip_amd import _lib, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang"
NEW_SYMBOLS = ("rgbm_adapose_feature_bytes", "rgbm_adapose_features_workspace_bytes", "rgbm_adapose_features",
               "rgbm_adapose_forward_cached")


def test_library_exports_the_feature_cache_entry_points():
    src = open(os.path.join(ROOT, "include", "rgbm.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(rgbm_[a-z0-9_]+)\s*\(", src))
    lib = _lib.load()
    for n in NEW_SYMBOLS:
        assert n in declared, f"{n} is not declared in include/rgbm.h"
        assert n in _lib.SIGNATURES, f"{n} is not bound in _lib.SIGNATURES"
        assert getattr(lib, n) is not None
    import ctypes as C
    n = C.c_size_t()
    assert lib.rgbm_adapose_feature_bytes(None, C.byref(n)) != 0 and b"feature_bytes" in lib.rgbm_last_error()


class _NoKernels:
    """Stands for librgbm_hip.so where no GPU is: every entry point reports success and launches nothing.  The controller's
    bookkeeping under test is host data; the device values the kernels would have written are never looked at."""

    def __getattr__(self, name):
        return lambda *a: 0


class _RecordingEstimator:
    def __init__(self, cache):
        self.cfg = {"task_name": "cabinet"}
        if cache:
            self.cfg["hip_feature_cache"] = True
        self.calls, self.invalidated = [], 0

    def estimate_device_indexed(self, K, rgb_pool, mask_pool, E1, E2, map1, map2, **kw):
        self.calls.append(dict(kw, M=int(rgb_pool.shape[0]), n=int(K.shape[0]), invalidated=self.invalidated))
        return torch.zeros(K.shape[0], 8, 3, dtype=torch.float64)

    def invalidate_features(self):
        self.invalidated += 1


class _Manipulation:
    def plan_pathway(self, center, direction, eval):
        pass


def _drive(monkeypatch, cache, episodes=2):
    from rgbmanip_amd import control_interface as cim
    monkeypatch.setattr(cim._lib, "load", lambda: _NoKernels())
    monkeypatch.setattr(cim._lib, "stream_ptr", lambda stream=None: None)
    n_envs = 3
    est = _RecordingEstimator(cache)
    env = synth.ReplayVecEnv(n_envs, 4)
    ci = cim.ControlInterface(env, est, _Manipulation(), synth.control_cfg("cabinet", 0.0), device="cpu")      # reset_queue + reset_robot
    steps_per_episode = ci.max_steps - 1
    for step in range(episodes * steps_per_episode):
        ci.step(synth.control_actions(n_envs, step % 10, 4), eval=False)
    return ci, est, n_envs, steps_per_episode


def test_controller_names_exactly_the_rows_written_since_the_last_estimation(monkeypatch):
    ci, est, N, spe = _drive(monkeypatch, cache=True)
    assert len(est.calls) == 2 * spe and spe >= 2
    assert est.invalidated == 2                                   # the constructor's reset_queue and the reset between the episodes
    for i, call in enumerate(est.calls):
        s = i % spe + 1                                          # the step inside its episode = the queue row add_view wrote for it
        rows = [0, 1] if s == 1 else [s]                         # the first estimation after a reset also meets the reset row
        want = [e for k in rows for e in range(k * N, (k + 1) * N)]
        assert list(call["fresh"]) == want, (i, list(call["fresh"]), want)
        assert call["M"] == ci.max_steps * N and call["n"] == N
        assert call["invalidated"] == 1 + i // spe               # features were forgotten before the episode's first estimation
    # every row of an episode was named exactly once
    for ep in range(2):
        named = sorted(e for c in est.calls[ep * spe:(ep + 1) * spe] for e in c["fresh"])
        assert named == list(range(ci.max_steps * N))


def test_controller_calls_the_estimator_as_before_without_the_key(monkeypatch):
    ci, est, N, spe = _drive(monkeypatch, cache=False, episodes=1)
    assert len(est.calls) == spe
    assert all("fresh" not in c for c in est.calls)


def test_feature_cache_with_dropout_is_refused():
    from rgbmanip_amd.config import ADAPOSE_CFGS
    from rgbmanip_amd.estimator import AdaPoseEstimator_v5
    cfg = dict(ADAPOSE_CFGS["adapose_cabinet"], load=False, hip_feature_cache=True)
    with pytest.raises(ValueError, match="hip_feature_cache"):
        AdaPoseEstimator_v5(None, dict(cfg, hip_dropout=0.15), None, state_dict={})
    with pytest.raises(ValueError, match="hip_feature_cache"):
        AdaPoseEstimator_v5(None, dict(cfg, hip_as_shipped=True), None, state_dict={})


@pytest.mark.skipif(shutil.which("hipcc") is None or not os.path.exists(CLANG), reason="needs hipcc / the ROCm clang (ASan runtime)")
def test_feature_cache_host_side_is_clean_under_address_sanitizer():
    r = subprocess.run(["bash", os.path.join(ROOT, "tools", "build_asan_host.sh")], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    rt = subprocess.run([CLANG, "-print-file-name=libclang_rt.asan-x86_64.so"], capture_output=True, text=True).stdout.strip()
    assert os.path.exists(rt), rt
    env = dict(os.environ, LD_PRELOAD=rt, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1:halt_on_error=1",
               RGBM_HIP_LIB=os.path.join(ROOT, "rgbmanip_amd", "librgbm_hip_asan_host.so"))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "asan", "drive_feature_cache.py")], capture_output=True, text=True,
                       timeout=900, env=env)
    assert "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    assert r.returncode == 0 and "ASAN_FEATURE_CACHE_OK" in r.stdout, r.stdout[-1000:] + r.stderr[-3000:]
