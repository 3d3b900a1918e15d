"""The block mapping of the int8 forward kernels (csrc/gml_i8_map.h: block index -> sample tile, node tile, and the grid both
launchers compute) is a plain C++ header: tests/native/i8_fwd_map.cpp runs it on the host over every block of a grid and checks
that each (sample tile, node tile) pair is produced exactly once, that every other block reports itself idle, that blocks b and
b + 8 -- one XCD -- work on the sample tiles 8 i + (b % 8), and that within an XCD the blocks of a group of 8 node tiles are
contiguous (the group's Tq then stays in that XCD's L2).  No GPU, no library."""
import os
import subprocess

import pytest

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "native", "i8_fwd_map.cpp")
CSRC = os.path.join(ROOT, "graphicalmodellearning.jl_amd", "csrc")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("fwd_map") / "i8_fwd_map")
    # a host compiler and the plain headers: they must not need a device header to compile
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, SRC, "-o", out])
    return out


# (sample tiles, node tiles): fewer than 8 sample tiles; an exact multiple of 8 / a padded tail; no full group of 8 node tiles /
# exactly one / full groups plus a remainder
@pytest.mark.parametrize("ntk,ngroups", [(1, 1), (7, 3), (8, 8), (9, 11), (16, 17), (47, 10)])
def test_fwd_block_mapping(exe, ntk, ngroups):
    r = subprocess.run([exe, str(ntk), str(ngroups)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr
