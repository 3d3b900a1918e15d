"""The signed column pairs of the i8w forward sweep (csrc/gml_i8_pairs.h) are a plain C++ header: tests/native/i8_pairs.cpp runs it
on the host.  For random and extreme pairs (q, q') with |q| <= 2^54 it checks that the seven balanced digits of q + q' and q - q'
recombine exactly, that the range predicate agrees with a 128-bit check (the last pair inside and the first outside included), that
the picks of the sparse MFMA operand over a 64-column step -- built from the sample bits as the kernel builds them, placed by the
operand layout measured on the device -- sum to sum_c x_c q_c for all four sign cases of a pair, whole values and plane by plane,
and that the column <-> slot map of a step is a bijection.  No GPU, no library."""
import os
import subprocess

import pytest

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "native", "i8_pairs.cpp")
CSRC = os.path.join(ROOT, "graphicalmodellearning.jl_amd", "csrc")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("i8_pairs") / "i8_pairs")
    # a host compiler and the plain headers: they must not need a device header to compile
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, SRC, "-o", out])
    return out


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_pairs(exe, seed):
    r = subprocess.run([exe, str(seed)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr
