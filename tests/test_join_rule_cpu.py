"""The host-statable rules of the device join (csrc/join_rule.hpp): the bounded lower-bound search over arrays of exactly nr keys against std::lower_bound /
std::upper_bound, and the pairs a left row emits per kind.  Compiled with the host compiler and the sanitizers into a stand-alone program
(tests/join_rule_main.cpp) that runs the grid; nothing is loaded into Python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_join_rule_edge_grid_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler found")
    exe = str(tmp_path / "join_rule")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           os.path.join(ROOT, "tests", "join_rule_main.cpp"), "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    assert " 0 wrong" in r.stdout, r.stdout
