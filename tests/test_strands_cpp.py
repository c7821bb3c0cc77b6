"""The C++ host mirror's both-strand search and complement_ranks (tests/cpp/test_strands_api.cpp): compiled everywhere with
the flags of test_host_cpp.py, executed on the GPU box."""
import os
import subprocess

import pytest

from tests.cpp_build import compile_cpp


def test_strands_mirror_compiles():
    assert os.path.exists(compile_cpp("test_strands_api"))


@pytest.mark.gpu
def test_strands_mirror_runs_on_gpu():
    exe = compile_cpp("test_strands_api")
    res = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "strands api ok" in res.stdout
