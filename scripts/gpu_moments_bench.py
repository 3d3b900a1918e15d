"""Exact sample moments on the device (Problem.moments / Problem.term_moments): whole-call and kernel times at
  (u1) uniform counts, n = 1024,   K = 10^6      (the headline shape)
  (u2) uniform counts, n = 4096,   K = 2^18
  (u3) uniform counts, n = 16 384, K = 2^16
  (w)  a weighted histogram handle, n = 64, 10^5 distinct rows, counts up to 2^16 (17 count planes)
  (t)  10^6 order-3 terms at n = 1024, K = 10^5
and two comparisons, interleaved round by round on the (u1) handle:
  * the route without this call: Problem.spins() (a 1 GB download) + float32 BLAS on the host (exact: every sum stays below 2^24);
    the ratio is recorded, there is no threshold;
  * the fastest device route without this call: the RISE gradient at Theta = 0 through the FP64-grade int8 pass
    (Problem.objgrad(..., precision="i8w")).  The pair kernel must be faster in every round; the run fails if it is not.
Rates: pair-samples per second = n (n + 1) / 2 x K / time (the upper triangle the kernel computes), against the vector ALU's
peak for xor + v_bcnt_u32_b32: 157.3e12 / 2 lane-operations per second (the FP32 vector peak of the microarchitecture guide counts an
FMA as two), two operations per 32 pair-samples: 1.258e15 pair-samples per second.  The term kernel is reported in GB/s of sign rows
read (key length x Kp / 8 bytes per term).

Run without arguments it is the driver: every GPU step is a child process under its own `timeout`, the first failure ends the
run; the kernel times come from a `rocprofv3 --kernel-trace --stats` run of the step `trace`.  Output: <out>/r10_moments.txt and
<out>/r10_moments_kernel_stats.csv (--out, default profiles/)."""
import argparse
import glob
import json
import os
import shutil
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_PAIR_SAMPLES = 157.3e12 / 2 / 2 * 32
SHAPES = {"u1": (1024, 1000000), "u2": (4096, 1 << 18), "u3": (16384, 1 << 16)}


def emit(**kw):
    print(json.dumps(kw), flush=True)


def random_handle(gml, n, K, counts=None, seed=0):
    rng = np.random.default_rng(seed)
    words = gml._lib.lib().gml_packed_words(K)
    bits = rng.integers(0, 1 << 32, size=(n, words), dtype=np.uint32)
    return gml.Problem(packed=(bits, counts, K))


def timed(fn, rounds):
    fn()  # warm-up
    ts = []
    for _ in range(rounds):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return ts


def step_pairs(gml, name, rounds):
    n, K = SHAPES[name]
    with random_handle(gml, n, K) as p:
        out = {}

        def call():
            out["r"] = p.moments(raw=True)
        ts = timed(call, rounds)
        ts1 = timed(lambda: p.moments(pairs=False, raw=True), rounds)
        assert np.array_equal(np.diagonal(out["r"][1]), np.full(n, K))
    emit(step=name, n=n, K=K, counts="uniform", whole_call_s=ts, sum1_only_call_s=ts1, pair_samples=n * (n + 1) // 2 * K,
         pair_samples_per_s_whole_call=n * (n + 1) // 2 * K / min(ts))


def step_weighted(gml, rounds):
    n, K = 64, 100000
    rng = np.random.default_rng(1)
    counts = rng.integers(1, 1 << 16, size=K, endpoint=True).astype(np.float64)
    with random_handle(gml, n, K, counts) as p:
        ts = timed(lambda: p.moments(raw=True), rounds)
    emit(step="w", n=n, K=K, counts="1 .. 2^16 (17 planes)", whole_call_s=ts, pair_samples=n * (n + 1) // 2 * K)


def random_triples(n, T, seed=2):
    """T keys of three distinct spins, 0-based int32 [T, 3]"""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, n, size=T)
    b = (a + rng.integers(1, n, size=T)) % n
    c = rng.integers(0, n, size=T)
    while True:
        bad = (c == a) | (c == b)
        if not bad.any():
            break
        c[bad] = rng.integers(0, n, size=int(bad.sum()))
    return np.ascontiguousarray(np.stack([a, b, c], axis=1), dtype=np.int32)


def step_terms(gml, rounds):
    n, K, T = 1024, 100000, 1000000
    keys = random_triples(n, T)
    with random_handle(gml, n, K) as p:
        sums = np.zeros(T, dtype=np.int64)
        L = gml._lib.lib()

        def call():
            gml._lib.check(L.gml_problem_term_moments(p._h, gml._lib._ptr(keys), 3, T, gml._lib._ptr(sums)))
        ts = timed(call, rounds)
        terms = [tuple(r) for r in (keys + 1).tolist()]
        ts_py = timed(lambda: p.term_moments(terms, raw=True), 1)
        Kp = (K + 1023) // 1024 * 1024
    emit(step="t", n=n, K=K, terms=T, order=3, c_call_s=ts, python_call_s=ts_py, sign_row_bytes=3 * T * Kp // 8,
         gb_per_s_c_call=3 * T * Kp / 8 / min(ts) / 1e9)


def step_compare(gml, rounds):
    n, K = SHAPES["u1"]
    with random_handle(gml, n, K) as p:
        nodes, theta = np.arange(n), np.zeros((n, n))
        p.moments(raw=True)
        p.objgrad("RISE", nodes, theta, precision="i8w")
        rows = []
        for r in range(rounds):
            t0 = time.perf_counter()
            s1, s2 = p.moments(raw=True)
            t1 = time.perf_counter()
            f, g = p.objgrad("RISE", nodes, theta, precision="i8w")
            t2 = time.perf_counter()
            want = -s2 / p.M
            want[np.diag_indices(n)] = -s1 / p.M
            err = float(np.abs(g - want).max())
            rows.append({"round": r, "moments_s": t1 - t0, "rise_i8w_theta0_s": t2 - t1, "ratio": (t2 - t1) / (t1 - t0),
                         "max_abs_diff": err})
            emit(step="compare_device", **rows[-1])
        # the host route, once per round as well (seconds each): spins() + float32 BLAS in slabs of 2^16 rows
        for r in range(min(rounds, 2)):
            t0 = time.perf_counter()
            S = p.spins()
            t1 = time.perf_counter()
            acc = np.zeros((n, n), dtype=np.float64)
            for k0 in range(0, K, 1 << 16):
                A = S[k0:k0 + (1 << 16)].astype(np.float32)
                acc += A.T @ A
            t2 = time.perf_counter()
            tm = time.perf_counter()
            s1, s2 = p.moments(raw=True)
            tm = time.perf_counter() - tm
            assert np.array_equal(acc.astype(np.int64), s2)
            emit(step="compare_host", round=r, spins_download_s=t1 - t0, blas_s=t2 - t1, host_route_s=t2 - t0, moments_s=tm,
                 ratio=(t2 - t0) / tm, threads=os.environ.get("OMP_NUM_THREADS"))
            del S
    slower = [x for x in rows if not x["moments_s"] < x["rise_i8w_theta0_s"]]
    if slower:
        sys.exit(f"moments() was not faster than the RISE i8w pass at Theta = 0 in rounds {[x['round'] for x in slower]}")


def step_trace(gml):
    """every shape once (after a warm-up call), for the kernel trace"""
    for name, (n, K) in SHAPES.items():
        with random_handle(gml, n, K) as p:
            p.moments(raw=True)
            p.moments(raw=True)
            if name == "u1":
                p.objgrad("RISE", np.arange(n), np.zeros((n, n)), precision="i8w")
    rng = np.random.default_rng(1)
    with random_handle(gml, 64, 100000, rng.integers(1, 1 << 16, size=100000, endpoint=True).astype(np.float64)) as p:
        p.moments(raw=True)
    keys = random_triples(1024, 1000000)
    with random_handle(gml, 1024, 100000) as p:
        sums = np.zeros(len(keys), dtype=np.int64)
        gml._lib.check(gml._lib.lib().gml_problem_term_moments(p._h, gml._lib._ptr(keys), 3, len(keys), gml._lib._ptr(sums)))


PMC_SETS = ["SQ_WAVE_CYCLES SQ_BUSY_CYCLES", "SQ_INSTS_VALU SQ_ACTIVE_INST_VALU", "SQ_INSTS_LDS SQ_LDS_BANK_CONFLICT",
            "SQ_WAIT_INST_ANY SQ_WAIT_INST_LDS", "SQ_INSTS_VMEM_RD SQ_INST_CYCLES_VMEM"]


def step_pmc(gml):
    """(u1) and (u3), each called twice: the second k_moments_pairs dispatch of each is the one summarised"""
    for name in ("u1", "u3"):
        n, K = SHAPES[name]
        with random_handle(gml, n, K) as p:
            p.moments(raw=True)
            p.moments(raw=True)


def pmc_summary(csv_path):
    import collections
    import csv
    per = collections.OrderedDict()
    with open(csv_path, newline="") as f:
        for row in csv.DictReader(f):
            if "k_moments_pairs(" in row["Kernel_Name"]:
                key = int(row["Dispatch_Id"])
                per.setdefault(key, collections.defaultdict(float))[row["Counter_Name"]] += float(row["Counter_Value"])
    ids = sorted(per)
    assert len(ids) == 4, ids
    return {"u1": dict(per[ids[1]]), "u3": dict(per[ids[3]])}


def run_step(args):
    import gml_amd as gml
    if args.step in SHAPES:
        step_pairs(gml, args.step, args.rounds)
    elif args.step == "w":
        step_weighted(gml, args.rounds)
    elif args.step == "t":
        step_terms(gml, args.rounds)
    elif args.step == "compare":
        step_compare(gml, args.rounds)
    elif args.step == "trace":
        step_trace(gml)
    elif args.step == "pmc":
        step_pmc(gml)
    else:
        sys.exit(f"unknown step {args.step}")


def kernel_times(trace_csv):
    """per-shape kernel times (microseconds) from the dispatches of the `trace` step, which run in a known order"""
    import csv
    rows = []
    with open(trace_csv, newline="") as f:
        for row in csv.DictReader(f):
            rows.append((int(row["Start_Timestamp"]), row["Kernel_Name"], (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3))
    rows.sort()
    pick = lambda sub: [d for _, name, d in rows if sub in name]  # noqa: E731
    pairs, terms, fin, planes = pick("k_moments_pairs("), pick("k_moments_terms"), pick("k_moments_pairs_finish"), pick("k_count_planes")
    assert len(pairs) == 6 + 17 and len(terms) == 8 and len(fin) == 7, (len(pairs), len(terms), len(fin))
    p8, p4 = pairs[:6], pairs[6:]
    out = []
    for i, (name, (n, K)) in enumerate(SHAPES.items()):
        t = p8[2 * i + 1]  # the second call of the shape
        ps = n * (n + 1) // 2 * K / (t * 1e-6)
        out.append({"shape": name, "n": n, "K": K, "k_moments_pairs_us": t, "k_moments_pairs_finish_us": fin[2 * i + 1],
                    "k_moments_terms_sum1_us": terms[2 * i + 1], "pair_samples_per_s": ps, "share_of_valu_peak": ps / PEAK_PAIR_SAMPLES})
    out.append({"shape": "w", "n": 64, "K": 100000, "k_moments_pairs_17_planes_us": sum(p4), "k_count_planes_us": sum(planes),
                "k_moments_terms_sum1_us": terms[6]})
    Kp = 100352
    out.append({"shape": "t", "n": 1024, "K": 100000, "terms": 1000000, "k_moments_terms_us": terms[7],
                "gb_per_s": 3 * 1000000 * Kp / 8 / (terms[7] * 1e-6) / 1e9})
    fwd = sum(d for _, name, d in rows if "k_fwd_i8w" in name or "k_bwd_i8" in name)
    out.append({"shape": "u1", "rise_i8w_theta0_fwd_bwd_kernels_us": fwd, "ratio_to_k_moments_pairs": fwd / p8[1]})
    return out


def driver(args):
    os.makedirs(args.out, exist_ok=True)
    txt = os.path.join(args.out, "r10_moments.txt")
    me = os.path.abspath(__file__)
    steps = [("u1", 240), ("u2", 240), ("u3", 300), ("w", 120), ("t", 240), ("compare", 420)]
    with open(txt, "w") as log:
        log.write("# scripts/gpu_moments_bench.py: one JSON line per measurement (see the script's docstring for the definitions)\n")
        log.write(f"# peak used for the pair kernel: {PEAK_PAIR_SAMPLES:.4g} pair-samples/s (vector ALU xor + v_bcnt_u32_b32)\n")
        log.flush()
        for step, limit in steps:
            cmd = ["timeout", "-k", "10", str(limit), sys.executable, me, "--step", step, "--rounds", str(args.rounds)]
            r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
            log.write(r.stdout)
            log.flush()
            print(r.stdout, end="", flush=True)
            if r.returncode != 0:
                log.write(f"# step {step} failed with exit status {r.returncode}: stopping\n")
                sys.exit(f"step {step} failed with exit status {r.returncode}")
        tdir = os.path.join(args.out, "r10_moments_trace")
        shutil.rmtree(tdir, ignore_errors=True)
        cmd = ["timeout", "-k", "10", "420", "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tdir, "--",
               sys.executable, me, "--step", "trace"]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        if r.returncode != 0:
            log.write(r.stdout[-4000:])
            sys.exit(f"the rocprofv3 step failed with exit status {r.returncode}")
        found = glob.glob(os.path.join(tdir, "**", "*kernel_stats.csv"), recursive=True)
        trace = glob.glob(os.path.join(tdir, "**", "*kernel_trace.csv"), recursive=True)
        if not found or not trace:
            sys.exit("rocprofv3 wrote no kernel_stats.csv / kernel_trace.csv")
        shutil.copyfile(found[0], os.path.join(args.out, "r10_moments_kernel_stats.csv"))
        times = kernel_times(trace[0])
        shutil.rmtree(tdir, ignore_errors=True)
        log.write("# kernel times of the `trace` step (rocprofv3 --kernel-trace --stats; every shape above run twice, the pass once):\n")
        # counters of the pair kernel, every set in a --pmc-only run of its own
        counters = {"u1": {}, "u3": {}}
        for cs in PMC_SETS:
            shutil.rmtree(tdir, ignore_errors=True)
            cmd = ["timeout", "-k", "10", "300", "rocprofv3", "--pmc"] + cs.split() + ["--output-format", "csv", "-d", tdir, "--",
                                                                                   sys.executable, me, "--step", "pmc"]
            r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
            found = glob.glob(os.path.join(tdir, "**", "*counter_collection.csv"), recursive=True)
            if r.returncode != 0 or not found:
                log.write(r.stdout[-4000:])
                sys.exit(f"the rocprofv3 --pmc {cs} step failed with exit status {r.returncode}")
            for shape, c in pmc_summary(found[0]).items():
                counters[shape].update(c)
            print("pmc", cs, "done", flush=True)
        shutil.rmtree(tdir, ignore_errors=True)
        log.write("# counters of k_moments_pairs (rocprofv3 --pmc, one run per pair of counters; summed over the XCDs):\n")
        for shape, c in counters.items():
            times.append({"shape": shape, "k_moments_pairs_counters": c})
        for k in times:
            log.write(json.dumps(k) + "\n")
            print(json.dumps(k), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", default=None)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    a = ap.parse_args()
    if a.step:
        run_step(a)
    else:
        driver(a)
