"""The index arithmetic of the DiagPDF histograms (quokka_amd/csrc/qk_diag_index.hpp, shared by host and device) exercised by a stand-alone host program
(tests/host/diag_index_check.cpp) built with the address and undefined-behaviour sanitizers.  No GPU; nothing is loaded into Python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_diag_index_arithmetic_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    exe = str(tmp_path / "diag_index_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined,float-cast-overflow", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "quokka_amd", "csrc"), os.path.join(ROOT, "tests", "host", "diag_index_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "OK" in out.stdout
