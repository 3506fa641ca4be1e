"""csrc/dev_buf.h on the host: tests/native/dev_buf_check.cpp, built as a stand-alone program with the host C++ compiler
under AddressSanitizer (leak detection on) and UBSan against its own fakes of hipMalloc / hipFree.  No GPU, no HIP runtime,
nothing loaded into Python."""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rocm_include():
    for root in (os.environ.get("ROCM_PATH"), "/opt/rocm"):
        if root and os.path.exists(os.path.join(root, "include", "hip", "hip_runtime_api.h")):
            return os.path.join(root, "include")
    return None


def test_dev_buf_under_asan_and_ubsan(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++") or shutil.which("clang++")
    inc = _rocm_include()
    if cxx is None or inc is None:
        pytest.skip("no host C++ compiler or no ROCm headers")
    exe = str(tmp_path / "dev_buf_check")
    # the sanitizer runtimes are linked statically: the program then runs whatever else the environment loads before it
    static = ["-static-libsan"] if "clang" in os.path.basename(cxx) else ["-static-libasan", "-static-libubsan"]
    build = subprocess.run([cxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] + static + [
                            "-D__HIP_PLATFORM_AMD__", "-I" + inc, os.path.join(REPO, "tests", "native", "dev_buf_check.cpp"),
                            "-o", exe], capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1")
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60, env=env)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "dev_buf_check ok" in run.stdout
