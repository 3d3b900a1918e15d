"""The forward kernel of the i8w pass (csrc/gml_kernels_i8w.hip) multiplies all 7 digit planes of Theta in one sweep; the build
flag -DI8W_TWO_SWEEPS keeps the earlier two-sweep form.  Every integer sum is exact and the fold of the plane sums into the
energies is the same sequence of FP64 operations in both, so the two builds must produce THE SAME BITS: f (RPLE's, an FP64 sum
added with atomics, to 1e-13), G, the raw planes of V and the per-slot sums csum / asum / mmax -- for every form, the wide form
(more than 32768 columns), a compacted pass and a pass with every row of Theta zero.  Each build runs in a child process of its
own (GML_LIB_OVERRIDE)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the child: runs one scenario with the library GML_LIB_OVERRIDE names, saves every output to an .npz
CHILD = r'''
import ctypes as C, sys
import numpy as np
import gml_amd as gml
synthetic = __import__("importlib").import_module("gml_amd.synthetic")
scenario, out = sys.argv[1], sys.argv[2]
L = gml._lib.lib()
L.gml_test_i8_pass_state.argtypes = [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int), C.POINTER(C.c_int64), C.c_void_p, C.c_void_p]
L.gml_test_tune.restype = C.c_double
L.gml_test_tune.argtypes = [C.c_int, C.c_double]
res = {}

def state(p, tag):
    ns, npl, kp = C.c_int64(), C.c_int(), C.c_int64()
    assert L.gml_test_i8_pass_state(p._h, C.byref(ns), C.byref(npl), C.byref(kp), None, None) == 0
    vq = np.zeros(ns.value * npl.value * kp.value, np.int8)
    sums = np.zeros((5, ns.value), np.int64)
    assert L.gml_test_i8_pass_state(p._h, C.byref(ns), C.byref(npl), C.byref(kp), vq.ctypes.data, sums.ctypes.data) == 0
    res[tag + "_vq"], res[tag + "_sums"] = vq, sums

def run(p, tag, form, nodes, th):
    f, g = p.objgrad(form, nodes, th, precision="i8w")
    res[tag + "_f"], res[tag + "_g"] = f, g
    state(p, tag)

rng = np.random.default_rng(7)
if scenario == "forms":  # 10 node tiles, 320 statistics columns: 5 steps of 64, more than the ring's 4 stages
    n, K = 320, 12000
    J = synthetic.block_ising_model(n, block=16, seed=3)
    with gml.Problem(model=J, num_samples=K, seed=4) as p:
        nodes = np.arange(n, dtype=np.int64)
        th = rng.normal(scale=0.05, size=(n, p.P))
        for form in ("RISE", "logRISE", "RPLE"):
            run(p, form, form, nodes, th)
        # a compacted pass: every row of a tile non-zero on a few columns only (the operator compacts by default)
        ths = np.zeros((n, p.P))
        for r in range(n):
            ths[r, rng.choice(p.P, size=6, replace=False)] = rng.normal(scale=0.4, size=6)
        run(p, "compact", "RISE", nodes, ths)
        L.gml_test_tune(6, 1)  # GML_TUNE_NO_COMPACT: the same rows, swept over all columns
        run(p, "dense", "RISE", nodes, ths)
        L.gml_test_tune(6, 0)
        run(p, "zero", "RISE", nodes, np.zeros((n, p.P)))  # every row zero: the kernel sweeps nothing (nk = 0)
elif scenario == "wide":  # order 3, n = 258: 257 + 257 * 256 / 2 = 33153 statistics columns (> 32768: the WIDE fold)
    n, K = 258, 1024
    spins = rng.choice(np.array([-1, 1], dtype=np.int8), size=(K, n))
    with gml.Problem(spins=spins, order=3) as p:
        nodes = np.arange(64, dtype=np.int64)
        th = rng.normal(scale=0.0005, size=(len(nodes), p.P))  # (sum |theta| about 13: inside the planes' range)
        for form in ("RISE", "RPLE"):
            run(p, "wide_" + form, form, nodes, th)
np.savez(out, **res)
'''


@pytest.fixture(scope="module")
def two_sweep_lib(tmp_path_factory):
    """libgml_hip.so with gml_kernels_i8w.hip rebuilt under -DI8W_TWO_SWEEPS, linked with the objects of the current build (the
    Makefile's OBJS, compiled by build()), in a directory of the test's own."""
    d = tmp_path_factory.mktemp("i8w_two_sweeps")
    cs = os.path.join(ROOT, "graphicalmodellearning.jl_amd", "csrc")
    mk = open(os.path.join(cs, "Makefile")).read()
    objs = next(line for line in mk.splitlines() if line.startswith("OBJS = ")).split()[2:]
    hipcc = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
    kobj = str(d / "gml_kernels_i8w.o")
    subprocess.run([hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-Wall", "-Wno-unused-result", "-fno-slp-vectorize",
                    "-DI8W_TWO_SWEEPS", "-c", os.path.join(cs, "gml_kernels_i8w.hip"), "-o", kobj], check=True, capture_output=True,
                   timeout=600)
    paths = [kobj if o == "gml_kernels_i8w.o" else os.path.join(cs, o) for o in objs]
    assert all(os.path.exists(q) for q in paths), "build() first"
    lib = d / "libgml_two.so"
    subprocess.run([hipcc, "--offload-arch=gfx950", "-shared", "-Wl,--no-undefined", "-o", str(lib)] + paths + ["-lpthread", "-ldl"],
                   check=True, capture_output=True, timeout=600)
    return str(lib)


def _run(lib, scenario, out):
    env = dict(os.environ)
    env.pop("GML_LIB_OVERRIDE", None)
    if lib:
        env["GML_LIB_OVERRIDE"] = lib
    r = subprocess.run([sys.executable, "-c", CHILD, scenario, str(out)], cwd=ROOT, env=env, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return dict(np.load(out))


@pytest.mark.parametrize("scenario", ["forms", "wide"])
def test_single_sweep_is_bit_identical_to_two_sweeps(scenario, two_sweep_lib, tmp_path):
    one = _run(None, scenario, tmp_path / "one.npz")
    two = _run(two_sweep_lib, scenario, tmp_path / "two.npz")
    assert sorted(one) == sorted(two)
    for k in sorted(one):
        a, b = one[k], two[k]
        assert a.shape == b.shape and a.dtype == b.dtype, k
        if k.endswith("RPLE_f"):  # RPLE's f is the kernel's FP64 sum, added with atomics in no fixed order
            assert np.abs(a / b - 1).max() <= 1e-13, k
            continue
        # bits, not values: -0.0 against 0.0 or two NaNs would not pass
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), (k, int((a != b).sum()))
    # the comparison is not vacuous: the passes produced planes, sums and gradients
    for k in one:
        if k.endswith("_vq") and not k.startswith("zero"):
            assert np.count_nonzero(one[k]) > 0, k
        if k.endswith("_g") and not k.startswith("zero"):
            assert np.abs(one[k]).max() > 0, k
