"""The stage planner (cat_amd/csrc/stage_plan.cpp: plain host C++) under AddressSanitizer and UndefinedBehaviorSanitizer, as a
stand-alone program: tools/stage_plan_sweep.cpp plans T = 1 .. 4096 x B in {1, 80, 96} under every switch setting of
tests/test_stage_plan.py plus segments and gd_stage_launches and checks every plan's invariants; nothing is loaded into Python.  Skipped
only where no C++ compiler with sanitizer support is found."""
import os
import shutil
import subprocess

import pytest

from tests.conftest import ROOT

FLAGS = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-D_GLIBCXX_ASSERTIONS", "-D__HIP_PLATFORM_AMD__"]


def _compiler(tmp):
    """A C++ compiler that builds AND runs a sanitized program here, or None."""
    probe = os.path.join(tmp, "probe.cpp")
    open(probe, "w").write("int main() { return 0; }\n")
    for cxx in filter(None, [os.environ.get("CXX"), "c++", "g++", "clang++"]):
        exe = shutil.which(cxx)
        if not exe:
            continue
        out = os.path.join(tmp, "probe")
        if subprocess.run([exe, *FLAGS, probe, "-o", out], capture_output=True).returncode == 0 and subprocess.run([out], capture_output=True).returncode == 0:
            return exe
    return None


def test_stage_planner_under_host_sanitizers(tmp_path):
    cxx = _compiler(str(tmp_path))
    if cxx is None:
        pytest.skip("no C++ compiler with -fsanitize=address,undefined on this machine")
    exe = os.path.join(str(tmp_path), "stage_plan_sweep")
    srcs = [os.path.join(ROOT, "tools", "stage_plan_sweep.cpp"), os.path.join(ROOT, "cat_amd", "csrc", "stage_plan.cpp"), os.path.join(ROOT, "cat_amd", "csrc", "crf_opts.cpp")]
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")   # (crf_internal.h includes the HIP headers for its device-pointer records; no HIP call is linked)
    subprocess.run([cxx, *FLAGS, "-I" + os.path.join(rocm, "include"), *srcs, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr.strip(), (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert "every check held" in r.stdout, r.stdout
