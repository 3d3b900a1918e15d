"""The backward GEMM of the int8-limb passes (csrc/gml_i8_bwd.hip: k_bwd_i8) reads its limb fragments from LDS with pinned
ds_read_b128 into four rotating fragment registers, three fragments ahead of their use, and counts the waits itself (gml_i8.h:
FRAG_READ / FRAG_WAIT); the build flag -DGML_I8_PLAIN_FRAGS keeps the loop with plain loads, which the compiler schedules and
waits for.  Only the order of the reads changes: every sum is an exact integer, so the two builds must produce THE SAME BITS -- f
(RPLE's, an FP64 sum added with atomics, to 1e-13), G, the raw planes of V, the per-slot sums and the Hessian-vector products --
for every backward form: planes (6, 0) and coarse (3, 3) at i8w, (4, 0) and coarse (3, 1) at i8x, (2, 0) for a two-limb
Hessian-vector product; for RISE / logRISE / RPLE, a compacted pass and Theta = 0.  Shape: n = 320, K = 12000 -- 5 column steps
(more than the ring's 4 stages), a partial 256-column tile, K not a multiple of 256 (the last split-K chunk is shorter than the
others).  The passes run through the test hook gml_test_i8_pass (as tests/test_gpu_i8_pass_variants.py drives it); each build
runs in a child process of its own (GML_LIB_OVERRIDE).  (The single sweep of k_fwd_i8w was tried with the same reads and measured
no faster -- profiles/r11_ab_frag_pipeline.txt -- so it keeps its plain loads and has no scenario here.)"""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the child: runs every scenario with the library GML_LIB_OVERRIDE names, saves every output to an .npz
CHILD = r'''
import ctypes as C, sys
import numpy as np
import gml_amd as gml
synthetic = __import__("importlib").import_module("gml_amd.synthetic")
_lib = gml._lib
out = sys.argv[1]
L = _lib.lib()
v, i64 = C.c_void_p, C.c_int64
L.gml_test_i8_pass.argtypes = [v, C.c_int, C.c_int, i64, v, v, v, v, i64, v, v, v, v, v, v]
L.gml_test_i8_instances.argtypes = [v, C.c_int, C.c_int]
L.gml_test_i8_pass_state.argtypes = [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int), C.POINTER(C.c_int64), C.c_void_p, C.c_void_p]
res = {}

def i8_pass(p, form, prec, nodes, theta, *, coarse=False, lf=0, want_grad=True, compact=True, zero_theta=False, vec=None, hv=0, hv_lf=5,
            ksub=1, kchunk=0, kpart=0):
    nodes = np.ascontiguousarray(nodes, dtype=np.int64)
    theta = np.ascontiguousarray(theta, dtype=np.float64)
    R, P = theta.shape
    kn = np.array([coarse, lf, want_grad, compact, zero_theta, hv, hv_lf, ksub, kchunk, kpart, 0], dtype=np.int64)
    f, g, h = np.zeros(R), np.zeros((R, P)), np.zeros((R, P))
    slots, plan = np.zeros((2, R, 3)), np.zeros(2, dtype=np.int64)
    vv = None if vec is None else np.ascontiguousarray(vec, dtype=np.float64)
    _lib.check(L.gml_test_i8_pass(p._h, _lib.FORMULATION_IDS[form], _lib.PRECISIONS[prec], R, _lib._ptr(nodes), _lib._ptr(theta),
                                  None, None if vv is None else _lib._ptr(vv), P, _lib._ptr(kn),
                                  _lib._ptr(f), _lib._ptr(g), _lib._ptr(h), _lib._ptr(slots), _lib._ptr(plan)))
    return f, g, h, slots

def state(p, tag):
    ns, npl, kp = C.c_int64(), C.c_int(), C.c_int64()
    assert L.gml_test_i8_pass_state(p._h, C.byref(ns), C.byref(npl), C.byref(kp), None, None) == 0
    vq = np.zeros(ns.value * npl.value * kp.value, np.int8)
    sums = np.zeros((5, ns.value), np.int64)
    assert L.gml_test_i8_pass_state(p._h, C.byref(ns), C.byref(npl), C.byref(kp), vq.ctypes.data, sums.ctypes.data) == 0
    res[tag + "_vq"], res[tag + "_sums"] = vq, sums

def run(p, tag, form, prec, nodes, th, **kw):
    f, g, h, slots = i8_pass(p, form, prec, nodes, th, **kw)
    res[tag + "_f"], res[tag + "_g"], res[tag + "_slots"] = f, g, slots
    if kw.get("hv"):
        res[tag + "_hv"] = h
    state(p, tag)

rng = np.random.default_rng(11)
n, K = 320, 12000  # 10 node tiles; 320 statistics columns: 5 steps of 64, 1.25 column tiles of 256; 47 sample tiles of 256
J = synthetic.block_ising_model(n, block=16, seed=3)
nodes = np.arange(n, dtype=np.int64)
L.gml_test_i8_instances(None, 0, 1)
with gml.Problem(model=J, num_samples=K, seed=4) as p:
    th = rng.normal(scale=0.05, size=(n, p.P))
    ths = np.zeros((n, p.P))  # every row of a tile non-zero on a few columns only: the pass compacts
    for r in range(n):
        ths[r, rng.choice(p.P, size=6, replace=False)] = rng.normal(scale=0.4, size=6)
    for form in ("RISE", "logRISE", "RPLE"):
        run(p, "w_" + form, form, "i8w", nodes, th)                       # backward planes (6, 0)
    run(p, "w_coarse", "RISE", "i8w", nodes, th, coarse=True)            # (3, 3)
    run(p, "w_compact", "RISE", "i8w", nodes, ths)
    run(p, "w_dense", "RISE", "i8w", nodes, ths, compact=False)
    run(p, "w_zero", "RISE", "i8w", nodes, np.zeros((n, p.P)), zero_theta=True)
    run(p, "w_zero_swept", "RISE", "i8w", nodes, np.zeros((n, p.P)))
with gml.Problem(model=J, num_samples=K, seed=4) as p:
    vec = rng.normal(size=(n, p.P)) * (rng.random((n, p.P)) < 0.3)
    for form in ("RISE", "RPLE"):
        run(p, "x_" + form, form, "i8x", nodes, th)                       # (4, 0)
    run(p, "x_coarse", "RISE", "i8x", nodes, th, coarse=True)            # (3, 1)
    run(p, "x_hv2", "RISE", "i8x", nodes, th, vec=vec, hv=2, hv_lf=2)    # products in two limbs: (2, 0)
    run(p, "x_hv1_RPLE", "RPLE", "i8x", nodes, th, vec=vec, hv=1, hv_lf=5)    # products in four limbs: (4, 0)
inst = np.zeros(8, dtype=np.uint64)
L.gml_test_i8_instances(_lib._ptr(inst), 8, 0)
res["instances"] = inst
np.savez(out, **res)
'''


def _bits(words):
    return {b for b in range(64 * len(words)) if (int(words[b >> 6]) >> (b & 63)) & 1}


def bwd_bit(NL, pl0):  # the numbering of gml_i8.h (kI8InstBits)
    return 288 + {2: 0, 3: 1, 4: 2, 6: 3}[NL] * 4 + {0: 0, 1: 1, 3: 2}[pl0]


@pytest.fixture(scope="module")
def plain_frags_lib(tmp_path_factory):
    """libgml_hip.so with gml_i8_bwd.hip rebuilt under -DGML_I8_PLAIN_FRAGS, linked with the objects of the
    current build (the Makefile's OBJS, compiled by build()), in a directory of the test's own."""
    d = tmp_path_factory.mktemp("i8_plain_frags")
    cs = os.path.join(ROOT, "graphicalmodellearning.jl_amd", "csrc")
    mk = open(os.path.join(cs, "Makefile")).read()
    objs = next(line for line in mk.splitlines() if line.startswith("OBJS = ")).split()[2:]
    hipcc = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
    rebuilt = {}
    for stem in ("gml_i8_bwd",):
        rebuilt[stem + ".o"] = str(d / (stem + ".o"))
        subprocess.run([hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-Wall", "-Wno-unused-result", "-fno-slp-vectorize",
                        "-DGML_I8_PLAIN_FRAGS", "-c", os.path.join(cs, stem + ".hip"), "-o", rebuilt[stem + ".o"]], check=True,
                       capture_output=True, timeout=600)
    paths = [rebuilt.get(o, os.path.join(cs, o)) for o in objs]
    assert all(os.path.exists(q) for q in paths), "build() first"
    lib = d / "libgml_plain_frags.so"
    subprocess.run([hipcc, "--offload-arch=gfx950", "-shared", "-Wl,--no-undefined", "-o", str(lib)] + paths + ["-lpthread", "-ldl"],
                   check=True, capture_output=True, timeout=600)
    return str(lib)


def _run(lib, out):
    env = dict(os.environ)
    env.pop("GML_LIB_OVERRIDE", None)
    if lib:
        env["GML_LIB_OVERRIDE"] = lib
    r = subprocess.run([sys.executable, "-c", CHILD, str(out)], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return dict(np.load(out))


def _compare(new, ref):
    assert sorted(new) == sorted(ref)
    # the intended instances ran, in both builds: every backward form
    want = {bwd_bit(6, 0), bwd_bit(3, 3), bwd_bit(4, 0), bwd_bit(3, 1), bwd_bit(2, 0)}
    for res in (new, ref):
        ran = _bits(res["instances"])
        assert want <= ran, sorted(want - ran)
    for k in sorted(new):
        a, b = new[k], ref[k]
        assert a.shape == b.shape and a.dtype == b.dtype, k
        if "RPLE" in k and k.endswith("_f"):  # RPLE's f is the kernel's FP64 sum, added with atomics in no fixed order
            assert np.abs(a / b - 1).max() <= 1e-13, k
            continue
        if "RPLE" in k and k.endswith("_slots"):  # (f, tau, mmax) per slot: f as above
            assert np.abs(a[0, :, 0] / b[0, :, 0] - 1).max() <= 1e-13, k
            a, b = a[:, :, 1:].copy(), b[:, :, 1:].copy()
        # bits, not values: -0.0 against 0.0 or two NaNs would not pass
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), (k, int((a != b).sum()))
    # the comparison is not vacuous: the passes produced planes, sums, gradients and products
    for k in new:
        zero = k.startswith("w_zero")
        if k.endswith("_vq"):
            assert np.count_nonzero(new[k]) > 0, k
        if k.endswith("_g"):
            assert (np.abs(new[k]).max() > 0) or zero, k
        if k.endswith("_hv"):
            assert np.abs(new[k]).max() > 0, k
    assert np.abs(new["w_RISE_g"]).max() > 0 and np.abs(new["x_RISE_g"]).max() > 0


def test_pinned_fragment_reads_are_bit_identical_to_plain_loads(plain_frags_lib, tmp_path):
    _compare(_run(None, tmp_path / "pinned.npz"), _run(plain_frags_lib, tmp_path / "plain.npz"))
