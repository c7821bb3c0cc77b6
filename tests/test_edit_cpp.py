"""The C++ host mirror's edit-distance search (tests/cpp/test_edit_api.cpp): compiled everywhere with the flags of
test_host_cpp.py, executed on the GPU box."""
import os
import subprocess

import pytest

from tests.cpp_build import compile_cpp


def test_edit_mirror_compiles():
    assert os.path.exists(compile_cpp("test_edit_api"))


@pytest.mark.gpu
def test_edit_mirror_runs_on_gpu():
    exe = compile_cpp("test_edit_api")
    res = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "edit api ok" in res.stdout
