"""The host-only rule of the 2-byte coarse scan copy (csrc/scan_coarse.hpp): the plan (min, shift) at the limits of both signednesses, what a coarse
comparison decides against the exact one for all six operators, which constants are refused, and the dense-bucket guard's arithmetic.  Compiled with the host
compiler and the sanitizers into a stand-alone program (tests/scan_coarse_main.cpp) that runs the grid; nothing is loaded into Python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_scan_coarse_rule_edge_grid_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler found")
    exe = str(tmp_path / "scan_coarse")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           os.path.join(ROOT, "tests", "scan_coarse_main.cpp"), "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    assert " 0 wrong" in r.stdout, r.stdout


def test_scan_route_and_build_trigger_edge_grid_under_sanitizers(tmp_path):
    """which form a lone `col OP const` scan takes and when it builds the image (csrc/scan_route.hpp, the composition of scan_image.hpp and scan_coarse.hpp)
    against the rule of DESIGN.md §3 restated in plain 64-bit arithmetic (tests/scan_route_main.cpp): the same stand-alone pattern as above"""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler found")
    exe = str(tmp_path / "scan_route")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           os.path.join(ROOT, "tests", "scan_route_main.cpp"), "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    assert " 0 wrong" in r.stdout, r.stdout
