"""CPU check of the flat-partition index arithmetic the coarse kernel and its launcher share
(rag_project_icd10_amd/csrc/flat_partition.hpp): plain C++, compiled here with g++ and run. Besides the partition
invariants it sweeps the coarse list plan over shards up to what HBM holds (dim 768 / 1024, 1 - 100 000 queries, k up to
128, narrow plan, wide mode and the second pass): every list stays inside the reach of the kernel's per-list buffer
descriptor, and the plans of the measured shapes are pinned."""
import json
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_checker(out_dir):
    exe = os.path.join(str(out_dir), "flat_partition_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "rag_project_icd10_amd", "csrc"),
                    os.path.join(ROOT, "tests", "flat_partition_check.cpp"), "-o", exe], check=True)
    return exe


def coarse_plan(exe, n, dim, nq, k, wide_now=0, max_list_tiles=None):
    """the planner's plan for one search shape; max_list_tiles=-1: without the descriptor cap (the parent's rule)"""
    args = [exe, "plan", str(n), str(dim), str(nq), str(k), str(wide_now)]
    if max_list_tiles is not None:
        args.append(str(max_list_tiles))
    return json.loads(subprocess.run(args, capture_output=True, text=True, check=True).stdout)


def test_flat_partition_invariants(tmp_path):
    exe = build_checker(tmp_path)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "cases ok" in out.stdout


def test_coarse_plan_caps_lists_at_the_descriptor_reach(tmp_path):
    """BASELINE configs[4] on one GPU: 10 M x 768 rows, 16 384-query slices, k = 10. Lists limited by the corpus alone span
    4.77 GiB (a 32-bit soffset wraps); the planner keeps them at 10 922 tiles, 2^31 - 1 bytes at most."""
    exe = build_checker(tmp_path)
    free = coarse_plan(exe, 10_000_000, 768, 16384, 10, max_list_tiles=-1)
    assert free["in_reach"] == 0 and free["longest_list_bytes"] > 4 << 30
    capped = coarse_plan(exe, 10_000_000, 768, 16384, 10)
    assert capped["ok"] == 1 and capped["in_reach"] == 1
    assert capped["max_list_tiles"] == 10922 and capped["list_tiles"] == 10922 and capped["longest_list_bytes"] < 2 ** 31
    assert coarse_plan(exe, 7_000_000, 1024, 16384, 10)["max_list_tiles"] == 8191
