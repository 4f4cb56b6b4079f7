"""The derivation behind finalize's certificate (csrc/cert_bound.hpp), checked on the CPU - the
derivation, not the kernel:

* in float64, for 2 000 random (query, row) pairs of each of three data shapes, the rounding part of the bound,
  |dq| (cmax' + dcmax) + |q'| dcmax with the norms the conversion kernel measures, is never exceeded by
  |q'.c' - fp16(q').fp16(c')|, the images built the way the kernel builds them (a power-of-two scale per query, ONE for
  the corpus, the column mean subtracted where the index would centre);
* the header's fp32 arithmetic rounds upward: tests/cert_bound_check.cpp, compiled with g++ under ASan + UBSan, compares
  it with the same expressions in long double."""
import os
import subprocess

import numpy as np
import pytest

import tight_bound_data as data

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("kind", ["gauss", "family", "centred"])
def test_rounding_bound_holds_in_float64(kind):
    q, c, _ = data.scaled(kind)
    c16, cres = data.image(c)
    q16, qres = data.image(q)
    cmax, dcmax = np.linalg.norm(c, axis=1).max(), cres.max()
    assert np.linalg.norm(c16, axis=1).max() <= cmax + dcmax
    rng = np.random.default_rng(5)
    qi, ri = rng.integers(0, len(q), 2000), rng.integers(0, len(c), 2000)
    # the pairs that matter most ride along: every query's best row
    best = np.argmax(q @ c.T, axis=1)
    qi, ri = np.concatenate([qi, np.arange(len(q))]), np.concatenate([ri, best])
    err = np.abs(np.einsum("ij,ij->i", q[qi], c[ri]) - np.einsum("ij,ij->i", q16[qi], c16[ri]))
    bound = qres[qi] * (cmax + dcmax) + np.linalg.norm(q, axis=1)[qi] * dcmax
    print(f"{kind}: largest error / bound {float((err / bound).max()):.3f}; residual / norm of the queries "
          f"{float((qres / np.linalg.norm(q, axis=1)).mean()):.3e}, of the corpus {float((cres / np.linalg.norm(c, axis=1)).mean()):.3e}; "
          f"bound / (1.2e-3 |q'| cmax') {float((bound / (1.2e-3 * np.linalg.norm(q, axis=1)[qi] * cmax)).mean()):.3f}")
    assert (err <= bound).all()


def test_bound_arithmetic_rounds_up(tmp_path):
    exe = os.path.join(str(tmp_path), "cert_bound_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "rag_project_icd10_amd", "csrc"), os.path.join(ROOT, "tests", "cert_bound_check.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "checks ok" in out.stdout
