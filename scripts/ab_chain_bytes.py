"""Same bytes from two builds of libgml_hip.so over the term-list chain family (thinned chains, replica exchange, annealed importance
sampling, conditional chains under a fixed mask with the split at 0, 1 and 2, and under a mask per row).

    python scripts/ab_chain_bytes.py parent=/path/to/the/other/libgml_hip.so new=

The driver runs the first tag twice and then every other tag once, one fresh child process each (GML_LIB_OVERRIDE selects the
library; an empty path is the tree's own), every child under its own timeout; it stops at the first child that fails.  A child
runs the shapes of the GPU tests' own CASES plus, per entry point, one case whose chain count is no multiple of 64, and prints
one line per array: its name and the SHA-256 of its bytes.  The driver compares the lines."""
import hashlib
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD_TIMEOUT_S = 240


def child():
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    import numpy as np
    from gml_amd import _lib
    import test_gpu_ais as t_ais
    import test_gpu_conditional as t_cond
    import test_gpu_masked as t_mask
    import test_gpu_tempered as t_temp
    import test_gpu_term_chains as t_chains
    from _conditional_reference import random_rows

    def emit(name, a):
        a = np.ascontiguousarray(a)
        print(f"{name} {a.dtype} {a.shape} {hashlib.sha256(a.tobytes()).hexdigest()}", flush=True)

    for case in sorted(t_chains.CASES):
        terms, n, nch = t_chains.CASES[case]()
        emit(f"chains/{case}/spins", t_chains.run(terms, n, nch * 3, 3, 5, 2, seed=11))
    terms, n, _ = t_chains.CASES["n33"]()
    emit("chains/n33_77_chains/spins", t_chains.run(terms, n, 77 * 2, 2, 4, 3, seed=5))

    for case in sorted(t_temp.CASES):
        terms, n = t_temp.CASES[case]()
        for R, ladders in sorted(t_temp.LADDERS.items()):
            spins, swaps = t_temp.run(terms, n, ladders, 2, 4, 2, t_temp.ladder(R), 1, seed=11)
            emit(f"tempered/{case}/R{R}/spins", spins)
            emit(f"tempered/{case}/R{R}/swap_counts", swaps)
    terms, n = t_temp.CASES["n33"]()
    spins, swaps = t_temp.run(terms, n, 13, 2, 4, 2, t_temp.ladder(8), 3, seed=5)  # 104 lanes
    emit("tempered/n33_13_ladders/spins", spins)
    emit("tempered/n33_13_ladders/swap_counts", swaps)

    def ais(tag, terms, n, chains, sps):
        result, logw, en, spins = t_ais.run(terms, n, chains, np.linspace(0.0, 1.0, 12), sps, seed=11)
        for name, a in (("result", result), ("log_weights", logw), ("energies", en), ("spins", spins)):
            emit(f"ais/{tag}/{name}", a)

    for case in sorted(t_ais.CASES):
        terms, n = t_ais.CASES[case]()
        ais(case, terms, n, 2000, 1)
    terms, n = t_ais.CASES["n33"]()
    ais("n33_77_chains", terms, n, 77, 3)

    def cond(tag, terms, n, K, hidden, replicas, spc, burn_in, thin):
        ev = random_rows(K, n, 0)
        for split in (0, 1, 2):
            old = _lib.lib().gml_test_cond_split(split)
            try:
                states, means = t_cond.device_run(terms, n, ev, hidden, replicas, spc, burn_in, thin, seed=11)
            finally:
                _lib.lib().gml_test_cond_split(old)
            emit(f"conditional/{tag}/split{split}/spins", states)
            emit(f"conditional/{tag}/split{split}/means", means)

    for case in sorted(t_cond.CASES):
        cond(case, *t_cond.CASES[case]())
    cond("n33_77_chains", t_cond.CASES["n33_four_hidden"]()[0], 33, 77, [0, 5, 31, 32], 1, 2, 3, 2)

    def masked(tag, terms, n, K, mask, replicas, spc, burn_in, thin):
        states, means = t_mask.device_run(terms, n, random_rows(K, n, 0), mask, replicas, spc, burn_in, thin, seed=11)
        emit(f"masked/{tag}/spins", states)
        emit(f"masked/{tag}/means", means)

    for case in sorted(t_mask.CASES):
        masked(case, *t_mask.CASES[case]())
    masked("n33_77_chains", t_mask.CASES["n33_independent_masks"]()[0], 33, 77, t_mask.random_mask(77, 33, 0.3, 1), 1, 2, 3, 2)


def run_child(path):
    env = dict(os.environ, GML_LIB_OVERRIDE=path)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=env, capture_output=True, text=True, timeout=CHILD_TIMEOUT_S)
    if r.returncode != 0:
        print(r.stdout[-2000:], r.stderr[-4000:])
        raise SystemExit(f"the child on {path or 'the tree library'} ended with {r.returncode}: stopping")
    return dict(line.split(" ", 1) for line in r.stdout.splitlines() if "/" in line.split(" ", 1)[0])


def main():
    tags = [a.split("=", 1) for a in sys.argv[1:]]
    if len(tags) < 2:
        raise SystemExit(__doc__)
    first, first_path = tags[0]
    a, b = run_child(first_path), run_child(first_path)
    repeats = sorted(k for k in a if a[k] == b.get(k))
    print(f"{first} against itself: {len(repeats)} of {len(a)} arrays repeat bit for bit")
    for k in sorted(set(a) - set(repeats)):
        print(f"  {first} differs from itself: {k}")
    misses = 0
    for tag, path in tags[1:]:
        c = run_child(path)
        assert set(c) == set(a), (sorted(set(c) ^ set(a)))
        bad = [k for k in repeats if c[k] != a[k]]
        misses += len(bad)
        for k in sorted(a):
            print(f"{k:64s} {a[k].rsplit(' ', 1)[0]:28s} {'same bytes' if c[k] == a[k] else 'DIFFERENT'}")
        print(f"{tag} against {first}: {len(repeats) - len(bad)} of {len(repeats)} repeating arrays have the same bytes, {len(bad)} misses")
    raise SystemExit(1 if misses or len(repeats) != len(a) else 0)


if __name__ == "__main__":
    child() if sys.argv[1:] == ["--child"] else main()
