"""The indexed inputs of mad::PeronaMalikDiffusionImageFilter (include/mad_itk.hpp) and the
descriptor word mad_pm_desc.channels from C++: compiles against the C ABI headers, links
libmad_hip.so, and runs (tests/cpp/pm_vector_facade_test.cpp)."""
import os
import subprocess

import pytest

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "cpp", "pm_vector_facade_test.cpp")
LIBDIR = os.path.join(ROOT, "multigridanisotropicdiffusion_amd")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("pm_vector_facade") / "pm_vector_facade_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I",
                           os.path.join(ROOT, "include"), SRC, "-o", out, "-L", LIBDIR,
                           "-lmad_hip", f"-Wl,-rpath,{LIBDIR}"])
    return out


def test_pm_vector_facade_builds_and_host_calls(exe):
    r = subprocess.run([exe, "host"], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "host ok" in r.stdout


@pytest.mark.gpu
def test_pm_vector_facade_runs_both_dimensions(exe):
    r = subprocess.run([exe, "run"], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "run ok" in r.stdout and "2D int16" in r.stdout and "3D float" in r.stdout
