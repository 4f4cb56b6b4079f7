"""CPU check of the adaptive rules of the AUTO search path (rag_project_icd10_amd/csrc/search_policy.hpp): plain C++ shared
by search_device and the corpus-shape probe of icd_index_create, compiled here with g++ and run. The checker
(tests/search_policy_check.cpp) drives the state the way a search does and pins wide mode of large batches, the second
pass's and the streaming pair's disarm rules, graph capture, the probe's reset and the searches that are not planned (MODE_EXACT,
one-query calls) between two planned ones; its expected values are literals taken
from the rules as the library stated them before they moved into the header."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_checker(out_dir):
    exe = os.path.join(str(out_dir), "search_policy_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "rag_project_icd10_amd", "csrc"),
                    os.path.join(ROOT, "tests", "search_policy_check.cpp"), "-o", exe], check=True)
    return exe


@pytest.mark.parametrize("group", ["wide", "pass2", "sparse", "capturing", "reset", "unplanned"])
def test_search_policy(tmp_path, group):
    exe = build_checker(tmp_path)
    out = subprocess.run([exe, group], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "checks ok" in out.stdout

