"""Per lane-sweep time of k_masked_chains on the sparse order-3 model of gpu_term_chains_bench.py (n = 1024) at 65 536 evidence rows,
one replica, one process, the runs interleaved:
  random 10 %   every entry hidden with probability 0.1, independently: the rows as they come ("unsorted") against the same rows in
                the stable order of their packed masks ("sorted"), which is what the front door does (inference._mask_order)
                so that the 64 chains of a wave share hidden spins;
  yardstick     k_cond_chains, the fixed-mask kernel, with every spin hidden: what a sweep over all n spins costs per lane;
  16 patterns   (for information) every row takes one of 16 random 10 % patterns at random: unsorted against sorted.
A wave pays for the union of the spins its 64 lanes hide.  The script prints the mean size of that union next to every time.
A per lane-sweep time is the difference of two runs that differ only in their sweep count, divided by the extra lane-sweeps, so record
building, uploads, the start pass and the handle cancel; the median of REPS such differences, and their spread (max - min).  Prints
one line per measurement (JSON)."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gml_amd as gml  # noqa: E402
from gml_amd import _lib  # noqa: E402
from gml_amd.inference import _mask_order  # noqa: E402
from gpu_conditional_bench import interleaved, rows, summary  # noqa: E402
from gpu_term_chains_bench import sparse3, wall  # noqa: E402

LANES, P_HIDDEN, SWEEPS = 65536, 0.1, (10, 210)


def emit(**kw):
    print(json.dumps(kw), flush=True)


def mean_union(mask):
    """the mean number of spins hidden by at least one of the 64 rows of a wave"""
    K, n = mask.shape
    return float(mask[:K // 64 * 64].reshape(K // 64, 64, n).any(axis=1).sum(axis=1).mean())


def masked_run(terms, n, order, ev, mask):
    p = gml.Problem(spins=ev)
    m = gml.Problem(spins=np.where(mask, -1, 1).astype(np.int8))
    return (p, m), lambda s: wall(lambda: _lib.conditional_chains_masked(terms, n, p, m, 1, 1, s, 1, seed=1, order=order))


def measure(name, terms, n, ev, mask, yardstick):
    order = max(2, max(len(k) for k in terms))
    perm = _mask_order(mask)
    handles, runs = [], {}
    for key, (e, m) in (("unsorted", (ev, mask)), ("sorted", (ev[perm], mask[perm]))):
        h, runs[key] = masked_run(terms, n, order, e, m)
        handles.extend(h)
    if yardstick:
        runs["k_cond_chains_all_hidden"] = lambda s: wall(lambda: _lib.conditional_chains(terms, n, handles[0], np.arange(n), 1, 1, s, 1,
                                                                                      seed=1, order=order))
    try:
        per = interleaved(runs, SWEEPS, LANES)
    finally:
        for h in handles:
            h.close()
    each, med, spread = summary(per)
    emit(case=name, model="sparse order 3", n=n, lanes=LANES, hidden_share=float(mask.mean()), sweeps=list(SWEEPS),
         union_per_wave={"unsorted": mean_union(mask), "sorted": mean_union(mask[perm])}, ns_per_lane_sweep=each,
         median_ns_per_lane_sweep=med, spread_ns=spread, ratio_sorted_over_unsorted=med["sorted"] / med["unsorted"])


def main():
    terms, n = sparse3()
    rng = np.random.default_rng(3)
    ev = rows(LANES, n)
    measure("random 10 %", terms, n, ev, rng.random((LANES, n)) < P_HIDDEN, True)
    patterns = rng.random((16, n)) < P_HIDDEN
    measure("16 patterns", terms, n, ev, patterns[rng.integers(0, 16, size=LANES)], False)


if __name__ == "__main__":
    main()
