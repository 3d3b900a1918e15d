"""Same bits from several builds of libgml_hip on one GPU (argv: tag=path ...; an empty path is the tree's own build).  The first
two tags are the reference build, run twice (where it does not repeat itself bit for bit a case cannot ask that of another build);
every further tag is held to the first one.  Cases: the scenarios `forms` and `wide` of tests/test_gpu_i8w_single_sweep.py at
precision i8w, `forms` at i8x (f, G, the raw V planes and the per-slot sums of every pass), and the learn() of bench.py's problem
at both precisions (out, kkt and the counters).  Everything is compared byte for byte, except RPLE's f: an FP64 sum added with
atomics in no fixed order, held to that test's 1e-13.
Every run is a child process with a time limit of its own (AB_TIMEOUT seconds, default 600); the first run that fails or overruns
ends the script with a non-zero status: nothing more is started on a GPU that has just failed a run."""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the child: runs one case with the library GML_LIB_OVERRIDE names, saves every output to an .npz
CHILD = r'''
import ctypes as C, sys
import numpy as np
import gml_amd as gml
synthetic = __import__("importlib").import_module("gml_amd.synthetic")
scenario, prec, out = sys.argv[1], sys.argv[2], sys.argv[3]
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
    f, g = p.objgrad(form, nodes, th, precision=prec)
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
        ths = np.zeros((n, p.P))  # a compacted pass: every row of a tile non-zero on a few columns only
        for r in range(n):
            ths[r, rng.choice(p.P, size=6, replace=False)] = rng.normal(scale=0.4, size=6)
        run(p, "compact", "RISE", nodes, ths)
        L.gml_test_tune(6, 1)  # GML_TUNE_NO_COMPACT: the same rows, swept over all columns
        run(p, "dense", "RISE", nodes, ths)
        L.gml_test_tune(6, 0)
        run(p, "zero", "RISE", nodes, np.zeros((n, p.P)))  # every row zero: the kernel sweeps nothing (nk = 0)
elif scenario == "wide":  # order 3, n = 258: 33153 statistics columns (> 32768: the WIDE fold)
    n, K = 258, 1024
    spins = rng.choice(np.array([-1, 1], dtype=np.int8), size=(K, n))
    with gml.Problem(spins=spins, order=3) as p:
        nodes = np.arange(64, dtype=np.int64)
        th = rng.normal(scale=0.0005, size=(len(nodes), p.P))
        for form in ("RISE", "RPLE"):
            run(p, "wide_" + form, form, nodes, th)
elif scenario == "learn":  # the learn leg of bench.py: n = 1024, K = 1e6, RISE 0.4, tol 1e-9
    J = synthetic.block_ising_model(1024, block=16, seed=0)
    with gml.Problem(model=J, num_samples=1000000, seed=0) as p:
        o, kkt, st = p.learn("RISE", 0.4, tol=1e-9, precision=prec, raise_on_fail=False)
    res["out"], res["kkt"] = np.asarray(o), np.asarray(kkt)
    keys = ("iterations", "passes", "forward_passes", "hessian_passes", "hv_evals", "node_evals", "polished", "not_converged")
    res["counters"] = np.array([int(st.get(k, -1)) for k in keys], np.int64)
    print("counters", {k: int(st.get(k, -1)) for k in keys}, flush=True)
np.savez(out, **res)
'''

CASES = (("forms", "i8w"), ("wide", "i8w"), ("forms", "i8x"), ("learn", "i8w"), ("learn", "i8x"))


def run(path, scenario, prec, out, limit):
    env = dict(os.environ)
    env.pop("GML_LIB_OVERRIDE", None)
    if path:
        env["GML_LIB_OVERRIDE"] = os.path.abspath(path)
    try:
        r = subprocess.run([sys.executable, "-c", CHILD, scenario, prec, out], cwd=ROOT, env=env, capture_output=True, text=True, timeout=limit)
    except subprocess.TimeoutExpired:
        print(scenario, prec, "TIMEOUT after", limit, "s", flush=True)
        sys.exit(124)
    if r.returncode != 0:
        print(scenario, prec, "FAILED: exit status", r.returncode, r.stdout[-300:], r.stderr[-1500:], flush=True)
        sys.exit(r.returncode if r.returncode > 0 else 1)
    return dict(np.load(out)), [l for l in r.stdout.splitlines() if l.startswith("counters")]


def differences(a, b):
    """keys of b that are not the bytes of a (RPLE's f: not within 1e-13), and the largest relative difference of RPLE's f"""
    assert sorted(a) == sorted(b)
    bad, frel = [], 0.0
    for k in sorted(a):
        if a[k].shape != b[k].shape or a[k].dtype != b[k].dtype:
            bad.append(k)
        elif k.endswith("RPLE_f"):
            d = float(np.abs(a[k] / b[k] - 1).max())
            frel = max(frel, d)
            if not d <= 1e-13:
                bad.append(k)
        elif not np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)):
            bad.append(k)
    return bad, frel


def main():
    libs = [a.split("=", 1) for a in sys.argv[1:]]
    assert len(libs) >= 3, "usage: ab_fwd_bits.py ref=PATH ref_again=PATH new=PATH ..."
    limit = float(os.environ.get("AB_TIMEOUT", "600"))
    misses = 0
    with tempfile.TemporaryDirectory() as tmp:
        for scenario, prec in CASES:
            got = {}
            for tag, path in libs:
                got[tag], info = run(path, scenario, prec, os.path.join(tmp, "o.npz"), limit)
            ref, again = got[libs[0][0]], got[libs[1][0]]
            assert any(np.count_nonzero(v) for v in ref.values()), "nothing computed"
            bad0, f0 = differences(ref, again)
            line = "%-6s %s | %d arrays | %s" % (scenario, prec, len(ref), "%s repeats itself (RPLE f to %.1e)" % (libs[0][0], f0) if not bad0
                                                 else "%s DIFFERS FROM ITSELF in %s" % (libs[0][0], bad0))
            for tag, _ in libs[2:]:
                bad, f1 = differences(ref, got[tag])
                bad = [k for k in bad if k not in bad0]  # (what the reference does not repeat cannot be asked of another build)
                misses += len(bad)
                line += " | %s: %s" % (tag, "same bytes (RPLE f to %.1e)" % f1 if not bad else "DIFFERENT: %s" % bad)
            print(line, " ".join(info), flush=True)
    print("# %d cases, %d misses" % (len(CASES), misses))
    sys.exit(1 if misses else 0)


if __name__ == "__main__":
    main()
