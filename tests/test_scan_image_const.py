"""The host-only decision of the 4-byte scan image (csrc/scan_image.hpp): which dtypes get an image, which constants are representable in it, and their
truncation.  Compiled with the host compiler and the sanitizers into a stand-alone program (tests/scan_image_const_main.cpp) that runs the edge grid — the
image types' limits, one inside, one outside on either side, the 64-bit limits; nothing is loaded into Python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_scan_image_constant_rule_edge_grid_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler found")
    exe = str(tmp_path / "scan_image_const")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           os.path.join(ROOT, "tests", "scan_image_const_main.cpp"), "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    assert " 0 wrong" in r.stdout, r.stdout
