"""The C++ host mirror's reporting overloads (tests/cpp/test_report_api.cpp: report_options, found): compiled everywhere with
the flags of test_host_cpp.py, executed on the GPU box."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "cpp", "test_report_api.bin")


def _compile():
    from kmer_index_amd import build
    build.build()
    libdir = os.path.join(ROOT, "kmer_index_amd")
    cmd = ["g++", "-std=c++20", "-O2", "-Wall", "-Wextra", "-Werror", f"-I{os.path.join(ROOT, 'include')}",
           os.path.join(ROOT, "tests", "cpp", "test_report_api.cpp"), "-o", BIN, f"-L{libdir}", "-lkmx", f"-Wl,-rpath,{libdir}",
           "-Wl,-rpath,/opt/rocm/lib"]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    return BIN


def test_report_mirror_compiles():
    assert os.path.exists(_compile())


@pytest.mark.gpu
def test_report_mirror_runs_on_gpu():
    exe = _compile()
    res = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "report api ok" in res.stdout
