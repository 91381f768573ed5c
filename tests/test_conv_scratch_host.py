"""Ownership of the device memory behind the implicit-GEMM launches (ConvScratch, the border tables of a ConvLayer), without a GPU:
tests/host/conv_scratch_main.cpp drives ConvLayer against the HIP stand-in (tests/asan/hip_stub.cpp), which counts the allocations
alive and can call a stream "being captured".  The program and the host objects it needs are compiled host-only with
-fsanitize=address,undefined into an executable of its own (nothing is preloaded); exit status 0 = every check held."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rgbmanip_amd", "csrc")
CLANGXX = "/opt/rocm/lib/llvm/bin/clang++"      # the link: plain clang++, no HIP runtime behind the stand-in
# the layer objects, the plan, the launchers they call, and what defines the globals those read
SOURCES = [os.path.join(CSRC, f) for f in ("layers.cpp", "conv_plan.cpp", "conv_launch.cpp", "prof.cpp", "igemm_generic.hip", "igemm_ws.hip",
                                           "igemm_m32.hip", "igemm_ws64.hip", "upconv.hip", "upconv_final.hip")] + \
          [os.path.join(ROOT, "tests", "asan", "hip_stub.cpp"), os.path.join(ROOT, "tests", "host", "conv_scratch_main.cpp")]
FLAGS = ["--cuda-host-only", "-x", "hip", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-gpu-sanitize",
         "-fno-omit-frame-pointer", "-O1", "-g", "-std=c++17", "-I", CSRC]


@pytest.mark.skipif(shutil.which("hipcc") is None or not os.path.exists(CLANGXX), reason="needs hipcc / the ROCm clang++")
def test_conv_scratch_and_border_tables_are_owned_and_freed(tmp_path):
    objs = [str(tmp_path / (os.path.basename(s) + ".o")) for s in SOURCES]
    procs = [subprocess.Popen(["hipcc"] + FLAGS + ["-c", s, "-o", o], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
             for s, o in zip(SOURCES, objs)]
    for s, p in zip(SOURCES, procs):
        out = p.communicate(timeout=900)[0]
        assert p.returncode == 0, s + "\n" + out[-3000:]
    # the host objects reference the embedded device code objects that a host-only compile does not produce
    undefined = subprocess.run(["nm", "-u"] + objs, capture_output=True, text=True, check=True).stdout
    fatbins = sorted({w for w in undefined.split() if w.startswith("__hip_fatbin_")})
    exe = str(tmp_path / "conv_scratch_main")
    r = subprocess.run([CLANGXX, "-fsanitize=address,undefined", "-o", exe] + objs + ["-Wl,--defsym=%s=0" % f for f in fatbins],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    # (the leak that matters here is of device memory, which the program counts itself)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0 and "CONV_SCRATCH_OK" in r.stdout, r.stdout[-1000:] + r.stderr[-4000:]
