"""The slot book of the solver's int8-limb workspace (csrc/gml_slots.h: which row owns which V planes, when a wrapped range makes
a row stale, what a rejected trial goes back to) is a plain C++ header: tests/native/plane_slots.cpp drives it on the host
through the sequences the solver makes of it and compares every state.  No GPU, no library."""
import os
import subprocess

import pytest

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "native", "plane_slots.cpp")
CSRC = os.path.join(ROOT, "graphicalmodellearning.jl_amd", "csrc")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("slots") / "plane_slots")
    # a host compiler and the one header: it must not need a device header to compile
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, SRC, "-o", out])
    return out


# 40, 200: not multiples of 32; 200, 1024: R / 2 > 96, the other arm of the main range's size; 64: no padding at all
@pytest.mark.parametrize("R", [40, 64, 200, 1024])
def test_slot_book_sequences(exe, R):
    r = subprocess.run([exe, str(R)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr
