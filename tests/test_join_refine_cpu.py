"""The refinement stage of the join on several keys and the String chunk rule (csrc/join_rule.hpp: join_refine_stage, join_chunk_key) — the text the kernel
k_join_refine runs — over heap arrays of exactly as many keys as a stage may read, against std::lower_bound / std::upper_bound / std::equal_range and a
byte-by-byte restatement.  Compiled with the host compiler and the sanitizers into a stand-alone program (tests/join_refine_main.cpp) that runs the grid;
nothing is loaded into Python."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_join_refine_stage_and_chunk_rule_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler found")
    exe = str(tmp_path / "join_refine")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           os.path.join(ROOT, "tests", "join_refine_main.cpp"), "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    m = re.search(r"(\d+) checked, 0 wrong", r.stdout)
    assert m and int(m.group(1)) > 100_000, r.stdout
