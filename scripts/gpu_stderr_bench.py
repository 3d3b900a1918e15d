"""gml_stderr (csrc/gml_sandwich.hip) at the headline shape -- n = 1024, K = 1e6, RISE, the rows of a refit on the l1 support -- and
on a synthetic support of 128 entries in every row (256 rows).  Device pointers throughout.  Per case: the median over WINDOWS
host-timed windows of `reps` back-to-back calls, about a second each (a call is host-blocking and ends with a stream
synchronisation), with their spread; the library's own three phase times (lists, Grams, factorisations) averaged over the median
window; and the PHASE rate of the Grams phase, counting 2 Grams x 2 K m_pad^2 flops per row (m_pad = the support + the unit
statistic, rounded up to 32).  That phase is host-timed and holds the workspace allocation, four small uploads, the sweep, the
reduce kernel and a stream synchronisation: it is a rate of the call's phase, not of a kernel -- kernel times come from
scripts/gpu_stderr_kernels.py under rocprofv3 --kernel-trace.  Also one learn() of the same handle, for the ratio.
Nothing is asserted but the statuses."""
import ctypes as C
import sys
import time

import numpy as np
import torch

sys.path.insert(0, ".")
import gml_amd as gml  # noqa: E402
synthetic = __import__("importlib").import_module("gml_amd.synthetic")

_lib = gml._lib
WINDOWS = 5
n, K = 1024, 1000000
L = _lib.lib()


def measure(prob, x, S, label, reps):
    R, P = x.shape
    dx, dS = torch.from_numpy(x).cuda(), torch.from_numpy(S).cuda()
    dse = torch.zeros((R, P), dtype=torch.float64, device="cuda")
    status = np.zeros(R, dtype=np.int32)
    t3 = np.zeros(3)

    def call():
        _lib.check(L.gml_stderr(prob._h, 0, C.c_void_p(dx.data_ptr()), P, C.c_void_p(dS.data_ptr()), P, C.c_void_p(dse.data_ptr()), _lib._ptr(status),
                                _lib._ptr(t3)))
    call()  # warm-up: allocator cache, code objects
    torch.cuda.synchronize()
    wall, phases = [], []
    for _ in range(WINDOWS):
        acc = np.zeros(3)
        t0 = time.perf_counter()
        for _ in range(reps):
            call()
            acc += t3
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) / reps)
        phases.append(acc / reps)
    assert np.all(status == 0), np.bincount(status)
    order = np.argsort(wall)
    med = order[len(order) // 2]
    m = ((S == gml.FREE) | ((S == gml.PENALISED) & (x != 0))).sum(axis=1)
    mpad = (m + 1 + 31) // 32 * 32
    flops = float((2 * 2.0 * K * mpad.astype(np.float64) ** 2).sum())
    ph = phases[med]
    print(f"{label}: {R} rows, support {m.min()}..{m.max()} (mean {m.mean():.1f}); {wall[med]:.4f} s per call (median of {WINDOWS} windows of {reps} calls: "
          f"{min(wall):.4f} .. {max(wall):.4f}); lists {ph[0]:.4f} s, Grams {ph[1]:.4f} s, finish {ph[2]:.4f} s; Grams phase "
          f"{flops / 1e12:.2f} TFLOP counted -> {flops / ph[1] / 1e12:.2f} TFLOP/s FP64 (phase rate)", flush=True)
    return wall[med]


J = synthetic.block_ising_model(n, block=16, seed=0)
with gml.Problem(model=J, num_samples=K, seed=0) as prob:
    prob.learn("RISE", 0.4)  # warm-up
    t0 = time.perf_counter()
    rows, kkt, st = prob.learn("RISE", 0.4)
    t_learn = time.perf_counter() - t0
    support, kept = gml.structure_from_rows(rows, n, 2, 0.05, rule="row", keep=gml.FREE, drop=gml.EXCLUDED, field=gml.FREE)
    t0 = time.perf_counter()
    refit, _, st2 = prob.learn("RISE", 0.4, structure=support, x0=rows)
    t_refit = time.perf_counter() - t0
    print(f"learn: {t_learn:.4f} s (library t_total {st['t_total']:.4f}); refit on {kept} kept couplings: {t_refit:.4f} s", flush=True)
    t_se = measure(prob, refit, support, "headline (refit rows)", 25)
    print(f"gml_stderr / learn = {t_se / t_learn:.2f}; / (learn + refit) = {t_se / (t_learn + t_refit):.2f}", flush=True)

with gml.Problem(model=J, num_samples=K, seed=0, node_range=(0, 256)) as prob:
    rng = np.random.default_rng(0)
    S = np.zeros((256, n), dtype=np.uint8)
    x = np.zeros((256, n))
    for r in range(256):
        sup = np.concatenate([[r], rng.choice(np.delete(np.arange(n), r), 127, replace=False)])
        S[r, sup] = gml.FREE
        v = rng.normal(size=128)
        x[r, sup] = v / np.abs(v).sum()
    measure(prob, x, S, "synthetic m = 128", 4)
