"""Kernel-level comparison of the Gram sweep of gml_stderr (k_sandwich_gram + k_sandwich_reduce, csrc/gml_sandwich.hip) with the FP64
working-set Hessian kernel k_hess_f64 (csrc/gml_kernels_f64.hip) on the SAME block sizes: K = 1e6 configurations of the headline
samples, RISE, blocks of 32, 160 and 512 entries (supports of 31, 159, 511 + the unit statistic).  k_hess_f64 is reached through the
test hook gml_test_hessian_run at precision f64 (an FP64 objective pass leaves V, then launch_hess_f64 on the caller's lists with
Kh = all configurations); one k_hess_f64 launch builds ONE Gram, one k_sandwich_gram launch builds two.

The script times nothing itself.  Run it alone under
    rocprofv3 --kernel-trace --output-format csv -d <dir> -- python scripts/gpu_stderr_kernels.py
and read the kernels' durations from the trace with  python scripts/gpu_stderr_kernels.py --summarize <dir>:  every case runs twice
(the first launch warms the code object), the summary prints both and the executed FP64 rate of the second, counting the lower
32 x 32 tile pairs each kernel computes: pairs x 2 x 1024 x K flops per Gram and row."""
import csv
import ctypes as C
import glob
import os
import sys

import numpy as np

CASES = [(32, 128), (160, 128), (512, 16)]  # (block size, rows)
K = 1000000


def summarize(d):
    rows = []
    for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            name = r["Kernel_Name"]
            for key in ("k_hess_f64", "k_sandwich_gram", "k_sandwich_reduce", "k_sandwich_finish"):
                if key in name:
                    rows.append((int(r["Start_Timestamp"]), key, (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6))
    rows.sort()
    per = {}
    for _, key, ms in rows:
        per.setdefault(key, []).append(ms)
    for key, v in per.items():
        print(key, " ".join(f"{x:.3f}" for x in v), "ms")
    Kp = (K + 1023) // 1024 * 1024
    for i, (blk, R) in enumerate(CASES):
        mt = blk // 32
        fl = mt * (mt + 1) // 2 * 2.0 * 1024 * Kp * R  # one Gram
        h = per["k_hess_f64"][2 * i + 1]
        g = per["k_sandwich_gram"][2 * i + 1]
        rd = per["k_sandwich_reduce"][2 * i + 1]
        print(f"block {blk}, {R} rows: k_hess_f64 {h:.3f} ms = {fl / h / 1e9:.2f} TFLOP/s (one Gram); k_sandwich_gram {g:.3f} ms (+ reduce "
              f"{rd:.3f} ms) = {2 * fl / g / 1e9:.2f} TFLOP/s (two Grams); rate ratio {2 * h / g:.2f}; one sweep / two k_hess_f64 runs = "
              f"{g / (2 * h):.2f} ({(g + rd) / (2 * h):.2f} with the reduce)")


if len(sys.argv) > 2 and sys.argv[1] == "--summarize":
    summarize(sys.argv[2])
    sys.exit(0)

sys.path.insert(0, ".")
import gml_amd as gml  # noqa: E402
synthetic = __import__("importlib").import_module("gml_amd.synthetic")

_lib = gml._lib
L = _lib.lib()
v, i32, i64 = C.c_void_p, C.c_int, C.c_int64
L.gml_test_hessian_run.argtypes = [v, i32, i32, i64, v, v, i64, v, i32, i64, i64, i32, i32, v, v, v, v, v, v, i64, v]
n = 1024
J = synthetic.block_ising_model(n, block=16, seed=0)
rng = np.random.default_rng(0)
with gml.Problem(model=J, num_samples=K, seed=0, node_range=(0, 128)) as prob:
    Kp = (K + 1023) // 1024 * 1024
    for blk, R in CASES:
        m = blk - 1
        S = np.zeros((128, n), dtype=np.uint8)
        x = np.zeros((128, n))
        cols = np.zeros((R, blk), dtype=np.int32)
        for r in range(R):
            sup = np.sort(np.concatenate([[r], rng.choice(np.delete(np.arange(n), r), m - 1, replace=False)]))
            S[r, sup] = gml.FREE
            val = rng.normal(size=m)
            x[r, sup] = val / np.abs(val).sum()
            cols[r, :m] = sup
            cols[r, m] = sup[0]  # (the padding entry of the old kernel's list: any parameter)
        nodes = np.arange(R, dtype=np.int64)
        theta = np.ascontiguousarray(x[:R])
        mtV = np.full(R, blk // 32, dtype=np.int32)
        hoffV = (np.arange(R, dtype=np.int64) * blk * blk)
        H = np.zeros(R * blk * blk)
        for _ in range(2):
            _lib.check(L.gml_test_hessian_run(prob._h, 0, _lib.PRECISIONS["f64"], R, _lib._ptr(nodes), _lib._ptr(theta), n, _lib._ptr(cols), blk, Kp, 1,
                                              0, 0, None, None, None, None, _lib._ptr(mtV), _lib._ptr(hoffV), R * blk * blk, _lib._ptr(H)))
        for _ in range(2):
            se, status = prob.stderr("RISE", x, structure=S)
        assert np.all(status == 0)
        # the two kernels computed the same matrix: A of the sandwich = the old kernel's block (lower triangle, first row as a probe)
        print(f"block {blk}: H[0][0][0] = {H[0]:.12g}", flush=True)
