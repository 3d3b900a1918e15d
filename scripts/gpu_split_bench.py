"""Splitting a resident handle into folds (Problem.split) at the headline shape, n = 1024, K = 10^6 rows of count 1, 5 folds:
  compare  the training part and the held-out part of fold 0 by two routes, alternating round by round in one process after a
           warm-up of each: (device) Problem.split twice; (host) what the library offered before -- Problem.sign_bits() download, the
           fold labels and the row selection / re-pack in numpy, Problem(packed=...) twice.  Both give the same handles (checked on
           the sign bits of the first round).  The device route must not be slower in any round; the run fails if it is.
  trace    the same two splits under `rocprofv3 --kernel-trace --stats` (a run of its own): the time of k_gather_bits against its
           algorithmic bytes n (K + K') / 8 -- every source sign word read once, every output word written once -- and the other
           kernels of a split.
  path     learn_path on a sampled block Ising problem (n = 64, K = 2 x 10^5, 5 folds, 6 values of c): the share of the wall-clock
           spent in split, solve and score.  For information.
Run without arguments it is the driver: every GPU step is a child process under its own `timeout`, the first failure ends the run.
Output: <out>/r16_split.txt and <out>/r16_split_kernel_stats.csv (--out, default profiles/)."""
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

N, K, FOLDS, SEED = 1024, 1000000, 5, 7


def emit(**kw):
    print(json.dumps(kw), flush=True)


def random_handle(gml, n, K, seed=0):
    rng = np.random.default_rng(seed)
    words = gml._lib.lib().gml_packed_words(K)
    bits = rng.integers(0, 1 << 32, size=(n, words), dtype=np.uint32)
    return gml.Problem(packed=(bits, None, K))


def host_route(gml, p, fold):
    """(training handle, held-out handle, seconds by stage) without Problem.split"""
    from _mcmc_chains_reference import u01
    t = {}
    t0 = time.perf_counter()
    bits = p.sign_bits()
    t["download_s"] = time.perf_counter() - t0
    t0 = time.perf_counter()
    u = u01(SEED, 0x8000000000000000, np.arange(p.K, dtype=np.uint64))  # (counts all 1: unit g = row g)
    label = np.minimum(FOLDS - 1, np.floor(FOLDS * u).astype(np.int64))
    t["labels_s"] = time.perf_counter() - t0
    out = []
    t["select_repack_s"] = t["create_packed_s"] = 0.0
    for complement in (True, False):
        t0 = time.perf_counter()
        keep = np.flatnonzero((label != fold) if complement else (label == fold))
        Kn = len(keep)
        words = (Kn + 1023) // 1024 * 32
        nb = np.zeros((p.n, words), dtype=np.uint32)
        for i0 in range(0, p.n, 64):  # 64 spins at a time: 64 MB of unpacked bits
            rows = np.unpackbits(bits[i0:i0 + 64].view(np.uint8), axis=1, bitorder="little")[:, keep]
            pk = np.packbits(rows, axis=1, bitorder="little")
            nb[i0:i0 + 64].view(np.uint8)[:, :pk.shape[1]] = pk
        t["select_repack_s"] += time.perf_counter() - t0
        t0 = time.perf_counter()
        out.append(gml.Problem(packed=(nb, None, Kn)))
        t["create_packed_s"] += time.perf_counter() - t0
    return out[0], out[1], t


def device_route(p, fold):
    t0 = time.perf_counter()
    train = p.split(FOLDS, fold, seed=SEED, complement=True)
    held = p.split(FOLDS, fold, seed=SEED, complement=False)
    return train, held, time.perf_counter() - t0


def step_compare(gml, rounds):
    with random_handle(gml, N, K) as p:
        # warm-up of both routes, and the check that they build the same handles
        a, b, _ = device_route(p, 0)
        c, d, _ = host_route(gml, p, 0)
        same = bool(np.array_equal(a.sign_bits(), c.sign_bits()) and np.array_equal(b.sign_bits(), d.sign_bits()) and
                    (a.K, a.M, b.K, b.M) == (c.K, c.M, d.K, d.M))
        emit(step="compare_check", same_handles=same, K_train=a.K, K_held=b.K, fold_sizes=p.fold_sizes(FOLDS, seed=SEED).tolist())
        parts = {"train": a.ingest_times(), "held": b.ingest_times()}
        for q in (a, b, c, d):
            q.close()
        if not same:
            sys.exit("the two routes built different handles")
        slower = []
        for r in range(rounds):
            a, b, td = device_route(p, 0)
            parts = {"train": a.ingest_times(), "held": b.ingest_times()}
            a.close(), b.close()
            t0 = time.perf_counter()
            c, d, th = host_route(gml, p, 0)
            th_total = time.perf_counter() - t0
            c.close(), d.close()
            emit(step="compare", round=r, device_route_s=td, host_route_s=th_total, ratio=th_total / td, host_stages=th,
                 device_stages={k: {"select_s": v["pack_s"], "gather_s": v["upload_s"], "images_s": v["images_s"], "total_s": v["total_s"]}
                                for k, v in parts.items()}, threads=os.environ.get("OMP_NUM_THREADS"))
            if not td <= th_total:
                slower.append(r)
        if slower:
            sys.exit(f"the device route was slower than the host route in rounds {slower}")


def step_trace(gml):
    with random_handle(gml, N, K) as p:
        for _ in range(2):  # the second pair is the one read
            a, b, _ = device_route(p, 0)
            emit(step="trace_shapes", K_train=a.K, K_held=b.K)
            a.close(), b.close()
        p.fold_sizes(FOLDS, seed=SEED)


def step_path(gml):
    synthetic = __import__("importlib").import_module("gml_amd.synthetic")
    n, Ks = 64, 200000
    spins, _ = synthetic.block_ising(n=n, K=Ks, seed=1)
    samples = np.concatenate([np.ones((Ks, 1)), spins.astype(np.float64)], axis=1)
    cs = [4.0, 1.0, 0.4, 0.2, 0.1, 0.05]
    gml.learn_path(samples, gml.RISE(), cs[:2], gml.HIP(), folds=2)  # warm-up
    t0 = time.perf_counter()
    res = gml.learn_path(samples, gml.RISE(), cs, gml.HIP(), folds=FOLDS, seed=SEED)
    total = time.perf_counter() - t0
    st = res.stats
    emit(step="path", n=n, K=Ks, folds=FOLDS, cs=cs, total_s=total, split_s=st["split_s"], solve_s=st["solve_s"], score_s=st["score_s"],
         final_learn_s=st["final_s"], share_split=st["split_s"] / total, share_solve=st["solve_s"] / total,
         share_score=st["score_s"] / total, c_min=res.c_min, c_1se=res.c_1se, mean=res.mean.tolist(), se=res.se.tolist(),
         iterations=st["iterations"].sum(axis=1).tolist())


def kernel_times(trace_csv, shapes):
    """the dispatches of the second pair of splits of the `trace` step (microseconds)"""
    import csv
    rows = []
    with open(trace_csv, newline="") as f:
        for row in csv.DictReader(f):
            rows.append((int(row["Start_Timestamp"]), row["Kernel_Name"], (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3))
    rows.sort()
    pick = lambda sub: [d for _, name, d in rows if sub in name]  # noqa: E731
    gather, counts, fold = pick("k_gather_bits"), pick("k_counts"), pick("k_fold_counts")
    assert len(gather) == 4 and len(fold) == 5, (len(gather), len(fold))
    out = []
    for name, t, Kn in (("train", gather[2], shapes["K_train"]), ("held", gather[3], shapes["K_held"])):
        by = N * (K + Kn) // 8
        out.append({"part": name, "K_out": Kn, "k_gather_bits_us": t, "algorithmic_bytes": by, "gb_per_s": by / (t * 1e-6) / 1e9})
    out.append({"k_fold_counts_split_us": fold[2:4], "k_fold_counts_sizes_us": fold[4], "k_counts_us": counts[2:4],
                "scans_us": pick("DeviceScan")[-6:] or pick("scan")[-6:], "k_write_src_us": pick("k_write_src")[2:4],
                "k_keep_flags_us": pick("k_keep_flags")[2:4]})
    return out


def driver(args):
    os.makedirs(args.out, exist_ok=True)
    txt = os.path.join(args.out, "r16_split.txt")
    me = os.path.abspath(__file__)
    with open(txt, "w") as log:
        log.write("# scripts/gpu_split_bench.py: one JSON line per measurement (see the script's docstring for the definitions)\n")
        log.flush()
        for step, limit in (("compare", 420), ("path", 300)):
            cmd = ["timeout", "-k", "10", str(limit), sys.executable, me, "--step", step, "--rounds", str(args.rounds)]
            r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
            log.write(r.stdout)
            log.flush()
            print(r.stdout, end="", flush=True)
            if r.returncode != 0:
                log.write(f"# step {step} failed with exit status {r.returncode}: stopping\n")
                sys.exit(f"step {step} failed with exit status {r.returncode}")
        tdir = os.path.join(args.out, "r16_split_trace")
        shutil.rmtree(tdir, ignore_errors=True)
        cmd = ["timeout", "-k", "10", "300", "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tdir, "--",
               sys.executable, me, "--step", "trace"]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        if r.returncode != 0:
            log.write(r.stdout[-4000:])
            sys.exit(f"the rocprofv3 step failed with exit status {r.returncode}")
        shapes = [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith('{"step": "trace_shapes"')][-1]
        found = glob.glob(os.path.join(tdir, "**", "*kernel_stats.csv"), recursive=True)
        trace = glob.glob(os.path.join(tdir, "**", "*kernel_trace.csv"), recursive=True)
        if not found or not trace:
            sys.exit("rocprofv3 wrote no kernel_stats.csv / kernel_trace.csv")
        shutil.copyfile(found[0], os.path.join(args.out, "r16_split_kernel_stats.csv"))
        log.write("# kernel times of the `trace` step (rocprofv3 --kernel-trace --stats; the second of two pairs of splits):\n")
        for k in kernel_times(trace[0], shapes):
            log.write(json.dumps(k) + "\n")
            print(json.dumps(k), flush=True)
        shutil.rmtree(tdir, ignore_errors=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", default=None)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    a = ap.parse_args()
    if a.step:
        import gml_amd as gml
        {"compare": lambda: step_compare(gml, a.rounds), "trace": lambda: step_trace(gml), "path": lambda: step_path(gml)}[a.step]()
    else:
        driver(a)
