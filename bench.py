#!/usr/bin/env python3
"""Benchmark of the learn() hot path on MI355X (BASELINE.json metric).

A "step" is one objective+gradient pass of the RISE operator over all n node-wise problems
(= n node evaluations: each node's f and grad over all K configurations) on the synthetic
BASELINE workload: n=1024 spins, K=1e6 samples (block-Ising, 64 blocks x 16 spins, seed 0), drawn on
the device by the library's exact block sampler (no host sample matrix).  Inputs (packed spins,
weights, and the parameters Theta) are resident in HBM before the timed region.

    python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR] [--full]

--dump-outputs writes f and the gradient of the last timed pass to DIR as float64 .npy files (dump_outputs()); the inputs
are seeded, so two builds run with the same arguments can be compared output for output.

With N > 1 and no WORLD_SIZE in the environment this process only launches
`python -m torch.distributed.run --nproc-per-node N ... bench.py` (before anything touches a GPU) and
relays rank 0's line; under torchrun each rank takes the nodes [rank*n/N, (rank+1)*n/N) of the SAME
problem (strong scaling; no collective on the data path, one RCCL all-gather of the learned rows).

Prints ONE JSON line (rank 0).  The headline (`value`, `ms_per_step`, `dtype`, `roofline`) is measured at precision "i8w": the
int8 matrix cores at the width of the reference's Float64 arithmetic (Theta in 54-bit, the weights in 47-bit int8 limbs, exp in
FP64; tests/test_gpu_parity.py holds it to the same 1e-12 as the FP64-MFMA path).  A plain run does only that: set up, warm up,
time the steps, write --dump-outputs, print the line; `roofline` there comes from the timed passes' own kernel times.

--full adds the legs that take runs of their own (the --no-* switches skip single legs of it): the pass through the host-pointer
operator boundary (roofline.pcie_*), "f64" (the same pass on the FP64-MFMA path, checked against the headline), "i8x" (the
38/31-bit accelerated mode that learn() uses by default), the pass with column compaction on, the learn() wall-clock of this
config at all three precisions (`learn_wall_s` ...), learn() from a host histogram, the 8-GPU shard projection, one pass over a
weighted histogram, and "cpu_baseline" (the CPU oracle's blocked restatement timed on this box's host cores on a bounded sample:
all threads and one thread, a parity check of the timed output against it; CPU learn() wall-clock at config 2 and at this config).
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

# dense MFMA peaks (flop/s or op/s).  i8 / bf16: /opt/skills/guides/MI355X_MICROARCH.md (bf16
# ~2.5 PF dense, i8 = 2x bf16 per clock).  FP64: AMD datasheet (78.6 TF matrix = vector); the local
# guide lists no FP64 figure.
PEAKS = {"f64": 78.6e12, "i8x": 5.0e15, "i8w": 5.0e15}
HBM_PEAK = 8.0e12  # B/s (MI355X_MICROARCH.md: HBM3E ~8 TB/s)
KERNELS = {"f64": {"fwd": "k_fwd_f64", "bwd": "k_bwd_f64"}, "i8x": {"fwd": "k_fwd_i8", "bwd": "k_bwd_i8"},
           "i8w": {"fwd": "k_fwd_i8w", "bwd": "k_bwd_i8<1, 6>"}}
# int8 digit-plane products issued per algorithmic product (forward: planes of Theta, backward: planes of V)
LIMBS = {"i8x": {"fwd": 5, "bwd": 4}, "i8w": {"fwd": 7, "bwd": 6}}
PMC_FILES = {"i8w": ("r6_i8w_pmc_traffic.json", "r5_i8w_pmc_traffic.json", "r4_i8w_pmc_traffic.json"), "i8x": ("r3_i8x_pmc_traffic.json", "r2_i8x_pmc_traffic.json")}
# sources of the kernels of an int8-limb pass (forward, backward, quantisation, finalisation -- whichever of them dominates): the PMC
# summaries carry their hash (scripts/pmc_summarize.py), and a line whose traffic comes from counters of other kernels says so
PASS_KERNEL_SOURCES = ("gml_kernels_i8w.hip", "gml_i8_fwd.hip", "gml_i8_bwd.hip", "gml_i8_pack.hip", "gml_i8_pass.hip", "gml_i8.h", "gml_bits.h")


def pass_kernels_sha256():
    import hashlib
    h = hashlib.sha256()
    for fn in PASS_KERNEL_SOURCES:
        h.update(open(os.path.join(ROOT, "graphicalmodellearning.jl_amd", "csrc", fn), "rb").read())
    return h.hexdigest()


def parse_args():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--spins", dest="n", type=int, default=1024, help="number of spins n (not --n: torchrun's own parser would call that an ambiguous abbreviation)")
    ap.add_argument("--samples", type=int, default=1000000)
    ap.add_argument("--block", type=int, default=16)
    ap.add_argument("--precision", default=os.environ.get("GML_BENCH_PRECISION", "i8w"), choices=["f64", "i8x", "i8w"],
                    help="arithmetic of the headline: i8w = FP64-grade int8-limb pass (default); i8x = 38/31-bit int8-limb pass; "
                         "f64 = FP64 MFMA pass")
    ap.add_argument("--full", action="store_true", help="also run every leg beyond the headline (other precisions, learn(), CPU "
                                                         "baseline, ...); the --no-* switches below skip single legs of a --full run")
    ap.add_argument("--no-learn", action="store_true", help="skip the full learn() wall-clock leg")
    ap.add_argument("--no-cpu", action="store_true", help="skip the cpu_baseline leg")
    ap.add_argument("--no-f64", action="store_true", help="skip the FP64-path leg")
    ap.add_argument("--no-i8x", action="store_true", help="skip the i8x (accelerated mode) leg")
    ap.add_argument("--no-weighted", action="store_true", help="skip the weighted-histogram pass")
    ap.add_argument("--no-sparse-theta", action="store_true", help="skip the leg that times the pass with column compaction on (its launches carry the "
                                                                   "forward kernel's name: a rocprofv3 --stats average of the timed passes must not mix them in)")
    ap.add_argument("--no-shards", action="store_true", help="skip the one-GPU measurement of every rank's workload of an 8-GPU run")
    ap.add_argument("--cpu-learn-max-s", type=float, default=100.0, help="run the CPU learn() of THIS config in full when the "
                                                                           "measured CPU rate predicts at most this many seconds")
    ap.add_argument("--no-host-learn", action="store_true", help="skip learn() from an 8.2 GB host Matrix{Int64}")
    ap.add_argument("--cpu-seconds", type=float, default=10.0, help="budget of the timed CPU objective/gradient sample")
    ap.add_argument("--cpu-learn-full", action="store_true", help="run the CPU learn() of THIS config in full instead of extrapolating")
    ap.add_argument("--dry-run", action="store_true", help="no GPU work: only the rank launch, node partition and rendezvous "
                                                            "(gloo); used by the CPU test of the N > 1 launch path")
    ap.add_argument("--dump-outputs", metavar="DIR", help="write f and the gradient of the last timed pass (all nodes) to DIR/*.npy "
                                                          "so that two builds can be compared output for output")
    return ap.parse_args()


def launch_ranks(args):
    """N > 1 without torchrun: start the N ranks as children (this process never touches a GPU) and relay rank 0's
    JSON line."""
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus),
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env.setdefault("OMP_NUM_THREADS", str(max(1, (os.cpu_count() or 8) // args.gpus)))
    r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, text=True)
    line = None
    for ln in r.stdout.splitlines():
        if ln.startswith("{") and '"metric"' in ln:
            line = ln
        else:
            print(ln, file=sys.stderr)
    if line:
        print(line)
    sys.exit(r.returncode if r.returncode else (0 if line else 1))


DUMP_LIMIT = 64 * 10**6  # bytes of array data --dump-outputs writes at most


def dump_outputs(out_dir, f, g):
    """f (n,) and the gradient (n, P) of the last timed pass as DIR/f.npy and DIR/grad.npy, float64.  A gradient over the
    size limit is cut to a fixed, seeded sample of its rows, whose indices go to DIR/grad_rows.npy.  Returns the names."""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    arrays = {"f": f, "grad": g}
    rows_cap = (DUMP_LIMIT - f.nbytes) // (8 * (g.shape[1] + 1))
    if g.shape[0] > rows_cap:
        rows = np.sort(np.random.default_rng(0).choice(g.shape[0], size=rows_cap, replace=False))
        arrays.update(grad=g[rows], grad_rows=rows)
    elif os.path.exists(os.path.join(out_dir, "grad_rows.npy")):
        os.remove(os.path.join(out_dir, "grad_rows.npy"))  # (left by an earlier, larger run: it would mislabel this grad.npy)
    for name, a in arrays.items():
        np.save(os.path.join(out_dir, name + ".npy"), np.ascontiguousarray(a, dtype=np.float64))
    return sorted(arrays)


def pass_roofline(km, K, P, nloc, precision):
    """roofline object of the dominant kernel of one pass: algorithmic flops = 2*K*P*n_loc per kernel (forward
    energies or gradient accumulation; SURVEY.md 8(d): 4*K*P per node evaluation)."""
    flops_kernel = 2.0 * K * P * nloc
    dom = "bwd" if km["bwd_ms"] >= km["fwd_ms"] else "fwd"
    achieved = flops_kernel / (km[dom + "_ms"] * 1e-3)
    peak = PEAKS[precision]
    rf = {"bound": "mfma", "kernel": KERNELS[precision][dom], "achieved": achieved / 1e12, "peak": peak / 1e12,
          "unit": "TFLOP/s", "frac": achieved / peak, "traffic": None, "fwd_ms": km["fwd_ms"], "bwd_ms": km["bwd_ms"],
          "pass_tflops": 2 * flops_kernel / (km["pass_ms"] * 1e-3) / 1e12, "kernels_ms_per_step": km["pass_ms"],
          "device_ms_per_step": km["device_ms_per_pass"],
          # t_roof / t_measured per kernel and for the whole pass (algorithmic flops once, against the peak
          # of the instruction class issued)
          "frac_fwd": flops_kernel / (km["fwd_ms"] * 1e-3) / peak, "frac_bwd": flops_kernel / (km["bwd_ms"] * 1e-3) / peak,
          "frac_pass": 2 * flops_kernel / (km["device_ms_per_pass"] * 1e-3) / peak}
    if precision in LIMBS:
        limbs = LIMBS[precision][dom]
        rf["limb_products"] = limbs
        rf["mfma_issue_frac"] = limbs * achieved / peak
        rf["note"] = ("achieved counts algorithmic flops once; the kernel issues limb_products int8 MFMA products per "
                      "algorithmic product (fixed point), so frac <= 1/limb_products")
        if precision == "i8w":
            rf["note"] += ("; the backward GEMM of i8w is one launch over all six planes of V (k_bwd_i8<1, 6>), the forward "
                           "kernel as one launch sweeping the columns once over all seven planes of Theta")
    return rf, dom


def main():
    args = parse_args()
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        launch_ranks(args)

    import numpy as np
    import torch
    import torch.distributed as dist

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if args.dry_run:
        if world > 1:
            dist.init_process_group("gloo")
        parts = [((r * args.n) // world, ((r + 1) * args.n) // world) for r in range(world)]
        seen = [None] * world
        if world > 1:
            dist.all_gather_object(seen, (rank, parts[rank]))
        else:
            seen = [(0, parts[0])]
        if rank == 0:
            print(json.dumps({"metric": "dry run (no GPU work)", "value": 0.0, "n_gpus": world, "dry_run": True,
                              "steps": args.steps, "warmup": args.warmup, "partition": [list(p) for _, p in sorted(seen)]}))
        if world > 1:
            dist.barrier()
            dist.destroy_process_group()
        return
    assert torch.cuda.is_available(), "bench.py needs an MI355X (no CPU fallback)"
    # one rank per GPU over RCCL; on a box with fewer GPUs than ranks (the 1-GPU test box) the ranks share devices and
    # the rendezvous falls back to gloo with host tensors -- same code path otherwise
    ndev = torch.cuda.device_count()
    device = local_rank % ndev
    torch.cuda.set_device(device)
    backend = "nccl" if ndev >= world else "gloo"
    cdev = torch.device("cuda", device) if backend == "nccl" else torch.device("cpu")
    if world > 1:
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", device))
        else:
            dist.init_process_group("gloo")

    import gml_amd as gml
    synthetic = __import__("importlib").import_module("gml_amd.synthetic")

    n, K = args.n, args.samples
    J = synthetic.block_ising_model(n, block=args.block, seed=0)
    node0, node1 = (rank * n) // world, ((rank + 1) * n) // world
    nloc = node1 - node0

    # every rank draws the same K configurations on its own GPU (same seed): exact block sampler of the library
    t0 = time.time()
    prob = gml.Problem(model=J, num_samples=K, seed=0, node_range=(node0, node1), device=device)
    torch.cuda.synchronize()
    t_create = time.time() - t0

    # evaluation point: the generating couplings (rows of the true model; diagonal = fields)
    theta = np.ascontiguousarray(J[node0:node1])

    def sync():
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
            torch.cuda.synchronize()

    def max_over_ranks(x):
        if world == 1:
            return float(x), [float(x)]
        t = torch.tensor([x], dtype=torch.float64, device=cdev)
        allt = torch.empty(world, dtype=torch.float64, device=cdev)
        dist.all_gather_into_tensor(allt, t)
        v = allt.cpu().tolist()
        return max(v), v

    # Timed region: Theta resident in HBM (uploaded before the clock starts), the passes back to back on the library's
    # stream, no host round trip inside; f and the gradient are downloaded once after the last pass.
    def timed(precision, steps, warmup):
        if warmup > 0:
            prob.bench_pass_resident("RISE", theta, steps=warmup, warmup=0, precision=precision)
        sync()
        t0 = time.perf_counter()
        km, f_res, g_res = prob.bench_pass_resident("RISE", theta, steps=steps, warmup=0, precision=precision, want_output=True)
        sync()
        elapsed, per_rank = max_over_ranks(time.perf_counter() - t0)
        return elapsed, per_rank, km, f_res, g_res

    elapsed, per_rank, km, f_res, g_res = timed(args.precision, args.steps, args.warmup)
    ms_per_step = elapsed / args.steps * 1e3
    value = n * args.steps / elapsed  # node evaluations per second, whole job

    roofline, dom = pass_roofline(km, K, n, nloc, args.precision)
    if args.full:
        # the same pass through the host-pointer operator boundary (Theta up and gradient down over PCIe every pass)
        t0 = time.perf_counter()
        prob.bench_pass("RISE", theta, steps=3, warmup=1, precision=args.precision)
        pcie_ms = (time.perf_counter() - t0) / 4 * 1e3
        roofline["pcie_inclusive_ms_per_step"] = pcie_ms
        roofline["pcie_inclusive_node_evals_per_s_per_gpu"] = nloc / (pcie_ms * 1e-3)

    # HBM-side traffic of the dominant kernel: PMC counters cannot be read from inside this process, so the value
    # measured with `rocprofv3 --pmc FETCH_SIZE` / `--pmc WRITE_SIZE` on this same command (separate passes;
    # scripts/gpu_profile.sh) is reported from the committed summary, labelled with its file.  gfx950 correction per
    # MI355X_MICROARCH.md: FETCH_SIZE counts half the bytes of 16-B/lane loads -> doubled.
    # algorithmic bytes of an all-node pass = the spins once (bit-packed) + 8 K of weights + 16 n_loc P
    # (Theta in, G out); what this implementation moves on top (both operand images, the limb planes of V out and back) is
    # reported apart as traffic_impl.
    roofline["bytes_alg_per_pass"] = K * n / 8.0 + 8.0 * K + 16.0 * nloc * n
    # achieved HBM rate on the ALGORITHMIC bytes and its fraction of the 8 TB/s peak: ~0.2 % is the signature of a compute-bound
    # contraction (arithmetic intensity 4 n_loc ops per spin byte), not a defect -- the binding roofline is the MFMA one above
    roofline["hbm_gbps_alg"] = roofline["bytes_alg_per_pass"] / (km["device_ms_per_pass"] * 1e-3) / 1e9
    roofline["hbm_frac_alg"] = roofline["hbm_gbps_alg"] / (HBM_PEAK / 1e9)
    roofline["hbm_peak_gbps"] = HBM_PEAK / 1e9
    if args.precision in LIMBS:
        roofline["traffic_impl_per_pass"] = 2.0 * K * n / 8.0 + 2.0 * LIMBS[args.precision]["bwd"] * K * nloc
        roofline["traffic_impl_note"] = ("bytes this implementation must move per pass: the two operand bit images (K n / 8 each) and the "
                                         "%d int8 limb planes of V written by the forward and read by the backward kernel"
                                         % LIMBS[args.precision]["bwd"])
    if args.precision in PMC_FILES and (n, K, world) == (1024, 1000000, 1):
        for fn in PMC_FILES[args.precision]:
            try:
                pm = json.load(open(os.path.join(ROOT, "profiles", fn)))
                kn = [k for k in pm if KERNELS[args.precision][dom].split("<")[0] in k][0]
                roofline["traffic"] = (2.0 * pm[kn]["FETCH_SIZE_KB"] + pm[kn]["WRITE_SIZE_KB"]) * 1024.0
                roofline["traffic_note"] = ("HBM bytes per launch of %s from profiles/%s (2*FETCH_SIZE + WRITE_SIZE, KB; a separate "
                                            "rocprofv3 --pmc run of this command, not this run)" % (kn, fn))
                # were the counters taken on the kernels that ran just now?
                sha = pm.get("_pass_kernels_sha256")  # (summaries of rounds 2-4 hashed one file: reported as not matching)
                roofline["traffic_kernels_match"] = sha == pass_kernels_sha256()
                # SURVEY.md 8(d) / north_star: achieved HBM GB/s next to the 8 TB/s peak -- from the counters, per kernel and for
                # the pass (both GEMM kernels; the quantise / finalise kernels move < 0.2 % of it), over THIS run's kernel times
                per = {}
                for leg in ("fwd", "bwd"):
                    kk = [k for k in pm if KERNELS[args.precision][leg].split("<")[0] in k and not k.startswith("_")][0]
                    per[leg] = (2.0 * pm[kk]["FETCH_SIZE_KB"] + pm[kk]["WRITE_SIZE_KB"]) * 1024.0
                roofline["traffic_per_kernel"] = {"fwd": per["fwd"], "bwd": per["bwd"], "pass": per["fwd"] + per["bwd"]}
                roofline["hbm_gbps_counter"] = {leg: per[leg] / (km[leg + "_ms"] * 1e-3) / 1e9 for leg in ("fwd", "bwd")}
                roofline["hbm_gbps_counter"]["pass"] = (per["fwd"] + per["bwd"]) / ((km["fwd_ms"] + km["bwd_ms"]) * 1e-3) / 1e9
                roofline["hbm_frac_counter"] = {leg: v / (HBM_PEAK / 1e9) for leg, v in roofline["hbm_gbps_counter"].items()}
                roofline["traffic_ratio_vs_alg"] = {"fwd": per["fwd"] / roofline["bytes_alg_per_pass"],
                                                    "pass": (per["fwd"] + per["bwd"]) / roofline["bytes_alg_per_pass"]}
                break
            except Exception:
                continue

    step = np.sort(np.asarray(km["step_ms"]))
    extra = {"per_rank_ms_per_step": [e / args.steps * 1e3 for e in per_rank],
             # spread of the timed passes on this rank (HIP events around every pass, device time)
             "step_ms_min": float(step[0]), "step_ms_median": float(np.median(step)), "step_ms_max": float(step[-1])}
    if args.dump_outputs:
        # what the timed path handed back after its last step, every rank's node rows in node order
        f_all, g_all = f_res, g_res
        if world > 1:
            parts = [None] * world
            dist.all_gather_object(parts, (f_res, g_res))
            f_all, g_all = np.concatenate([q[0] for q in parts]), np.concatenate([q[1] for q in parts])
        if rank == 0:
            extra["dump_outputs"] = {"dir": os.path.abspath(args.dump_outputs), "files": dump_outputs(args.dump_outputs, f_all, g_all)}

    def gather_list(x):
        """one float per rank -> list over ranks (rank order)"""
        return max_over_ranks(x)[1]

    extra["collective_backend"] = (dist.get_backend() + (" (RCCL)" if backend == "nccl" else " (ranks share a GPU: host tensors)")) if world > 1 else "none (1 rank)"
    extra["collective_ranks"] = world
    extra["devices_visible"] = ndev
    # which physical GPU every rank drives: a wrong binding (two ranks on one device, a rank off its local GPU) shows in the line itself
    prop = torch.cuda.get_device_properties(device)
    me = {"rank": rank, "local_rank": local_rank, "device": device, "name": prop.name,
          "pci": "%04x:%02x:%02x" % (getattr(prop, "pci_domain_id", 0), getattr(prop, "pci_bus_id", -1) & 0xff, getattr(prop, "pci_device_id", 0) & 0xff),
          "uuid": str(getattr(prop, "uuid", "")), "hbm_gb": round(prop.total_memory / 2**30, 1), "nodes": [node0, node1],
          "visible_env": os.environ.get("HIP_VISIBLE_DEVICES", os.environ.get("ROCR_VISIBLE_DEVICES", ""))}
    ranks_info = [None] * world
    if world > 1:
        dist.all_gather_object(ranks_info, me)
    else:
        ranks_info = [me]
    extra["ranks"] = ranks_info
    extra["distinct_devices"] = len({(q["pci"], q["uuid"]) for q in ranks_info})
    try:
        extra["rccl_version"] = ".".join(str(v) for v in torch.cuda.nccl.version())
    except Exception as e:  # (not fatal: the line must come out)
        extra["rccl_version"] = "unknown (%s)" % type(e).__name__
    extra["torch_version"], extra["hip_version"] = torch.__version__, str(torch.version.hip)

    # ---- --full only from here on: the legs beyond the headline, each a run of its own ------------------------------------
    # ---- the other arithmetics on the same workload ------------------------------------------------------------------
    # f64: the FP64-MFMA path (fewer steps: ~85 ms each); i8x: the 38/31-bit int8-limb pass (learn()'s default)
    others = {}
    for prec, skip, nsteps in (("f64", args.no_f64, max(3, min(20, args.steps // 10))), ("i8x", args.no_i8x, max(3, min(50, args.steps // 4))),
                               ("i8w", True, 0)):
        if not args.full or skip or prec == args.precision:
            continue
        e_o, _, km_o, f_o, g_o = timed(prec, nsteps, 1)
        rf_o, _ = pass_roofline(km_o, K, n, nloc, prec)
        others[prec] = {"value": n * nsteps / e_o, "unit": "node-evals/s", "steps": nsteps, "ms_per_step": e_o / nsteps * 1e3, "dtype": prec,
                        "roofline": rf_o,
                        "max_abs_grad_diff_vs_headline": float(np.abs(g_o - g_res).max()),
                        "max_rel_f_diff_vs_headline": float(np.abs(f_res / f_o - 1).max())}
    f64 = others.get("f64")

    # ---- the same pass with the forward GEMM COMPACTED to the columns on which a node tile's rows are non-zero (round 6; what
    # gml_objgrad_batch does by default).  The evaluation point of this benchmark -- the rows of the generating model -- is sparse
    # (15 couplings + a field per node), so a 32-row tile sweeps 32-48 of the 1024 columns; the integer sums and therefore all results
    # are the same bits.  NOT the headline: `value` prices the contraction over all columns, which is what a dense Theta costs.
    if args.full and args.precision in LIMBS and not args.no_sparse_theta:
        import ctypes
        Lb = gml._lib.lib()
        Lb.gml_test_tune.restype = ctypes.c_double
        Lb.gml_test_tune.argtypes = [ctypes.c_int, ctypes.c_double]
        Lb.gml_test_tune(7, 1.0)  # (gml_solver.h: GML_TUNE_BENCH_COMPACT -- the timing hook compacts too)
        try:
            ns_c = max(3, min(50, args.steps // 4))
            e_c, _, km_c, f_c, g_c = timed(args.precision, ns_c, 2)
        finally:
            Lb.gml_test_tune(7, 0.0)
        extra["sparse_theta"] = {"what": "the timed pass with column compaction on (forward GEMM over each node tile's non-zero columns only); "
                                         "the evaluation point is sparse: nnz per row = %d of %d" % (int((theta != 0).sum(1).max()), n),
                                 "value": n * ns_c / e_c, "unit": "node-evals/s", "steps": ns_c, "ms_per_step": e_c / ns_c * 1e3,
                                 "fwd_ms": km_c["fwd_ms"], "bwd_ms": km_c["bwd_ms"], "device_ms_per_pass": km_c["device_ms_per_pass"],
                                 "same_bits_as_headline": bool(np.array_equal(g_c, g_res) and np.array_equal(f_c, f_res))}

    # ---- learn() wall-clock of this config ---------------------------------------------------------------------
    out = None
    STKEYS = ("iterations", "passes", "forward_passes", "node_evals", "max_kkt", "not_converged", "t_pass", "t_hess", "t_host", "polished")

    def learn_leg(prec, nruns):
        # nruns runs, the median reported (every run listed): a run now and then carries a one-off stall of the allocator or of
        # a lazily loaded code object that has nothing to do with the path
        runs = []
        for _ in range(nruns):
            sync()
            t0 = time.perf_counter()
            o_, kkt_, st_ = prob.learn("RISE", 0.4, tol=1e-9, precision=prec, raise_on_fail=False)
            sync()
            runs.append((max_over_ranks(time.perf_counter() - t0), st_, o_))
        (t_, per_rank_), st_, o_ = sorted(runs, key=lambda r: r[0][0])[len(runs) // 2]
        return t_, per_rank_, st_, o_, [r[0][0] for r in runs]

    if args.full and not args.no_learn:
        t_learn, learn_per_rank, st, out, runs_s = learn_leg(args.precision, 3)
        extra["learn_wall_runs_s"] = runs_s
        if world > 1:
            # final gather of the row blocks over RCCL/xGMI (the only collective of the path)
            sync()
            tg = time.perf_counter()
            buf = torch.from_numpy(out).to(cdev)
            allb = torch.empty((world * buf.shape[0], buf.shape[1]), dtype=buf.dtype, device=cdev)
            dist.all_gather_into_tensor(allb, buf)
            torch.cuda.synchronize()
            extra["gather_s"] = time.perf_counter() - tg
            full = allb.reshape(n, n).cpu().numpy()
            # stragglers among the node shards: iterations, passes and evaluated rows of every rank
            extra["learn_per_rank_iterations"] = [int(v) for v in gather_list(st["iterations"])]
            extra["learn_per_rank_passes"] = [int(v) for v in gather_list(st["passes"])]
            extra["learn_per_rank_node_evals"] = [int(v) for v in gather_list(st["node_evals"])]
            extra["learn_per_rank_t_pass_s"] = gather_list(st["t_pass"])
            extra["learn_per_rank_t_hess_s"] = gather_list(st["t_hess"])
        else:
            full = out
        sym_err = float(np.abs(0.5 * (full + full.T) - J).max())
        extra.update({"learn_wall_s": t_learn, "learn_precision": args.precision, "learn_per_rank_s": learn_per_rank, "learn_create_s": t_create,
                      "learn_iterations": st["iterations"], "learn_passes": st["passes"],
                      "learn_forward_passes": st["forward_passes"], "learn_node_evals": st["node_evals"],
                      "learn_max_kkt": st["max_kkt"], "learn_not_converged": st["not_converged"],
                      "learn_t_pass": st["t_pass"], "learn_t_hess": st["t_hess"], "learn_t_host": st["t_host"],
                      # what the passes cost INSIDE learn() (control uploads, scalar downloads and the per-pass sync included):
                      # the solver drives the same resident pass function the timed region above calls
                      "learn_pass_node_evals_per_s": st["node_evals"] / max(st["t_pass"], 1e-9) * world,
                      "max_err_vs_true_model": sym_err})
        # the same solve in the other arithmetics: the reference's own (FP64 MFMA throughout, one run) and the accelerated mode
        for prec, skip, nruns in (("f64", args.no_f64, 1), ("i8x", args.no_i8x, 3), ("i8w", True, 0)):
            if skip or prec == args.precision:
                continue
            t_o, _, st_o, out_o, runs_o = learn_leg(prec, nruns)
            extra["learn_wall_s_" + prec] = t_o
            extra["learn_" + prec] = dict({k: st_o[k] for k in STKEYS}, runs_s=runs_o,
                                          max_abs_diff_vs_headline_solution=float(np.abs(out_o - out).max()))

    # ---- N > 1: the front door of the process-per-GPU route, learn(samples, RISE(), HIP(distributed=True)) from a HOST matrix that
    # only rank 0 holds: rank 0 packs it once (1 bit per spin), the bits go out by one broadcast (RCCL over xGMI), every rank builds
    # its handle from them, solves its node range, and the rows are all-gathered (start / end collectives)
    if world > 1 and args.full and not args.no_learn and not args.no_host_learn:
        hist = None
        if rank == 0:
            sp = prob.spins()
            hist = np.empty((K, n + 1), dtype=np.int8)
            hist[:, 0] = 1
            hist[:, 1:] = sp
            del sp
        md = gml.HIP(distributed=True, device=device, tol=1e-9, precision=args.precision)
        try:  # (an extra leg: whatever goes wrong in it must not take the headline line down with it)
            sync()
            t0 = time.perf_counter()
            Rd = gml.learn(hist, gml.RISE(0.4, False), md)
            sync()
            t_fd, _ = max_over_ranks(time.perf_counter() - t0)
            extra["learn_distributed_front_door"] = {
                "wall_s": t_fd, "input": "K x (1+n) int8 histogram on rank 0 only; the other ranks pass None",
                "pack_s": gather_list(md.stats["pack_s"]), "bcast_s": gather_list(md.stats["bcast_s"]), "bcast_bytes": md.stats["bcast_bytes"],
                "solve_s": gather_list(md.stats["t_total"]), "handle_from_bits_s": gather_list(md.stats["t_pack"]),
                "same_rows_as_device_sampled_handles": bool(out is not None and np.array_equal(Rd, full))}
        except Exception as e:  # noqa: BLE001
            extra["learn_distributed_front_door"] = {"error": "%s: %s" % (type(e).__name__, e)}
        del hist

    # ---- learn() from a HOST histogram: what a `learn(samples, RISE(), HIP())` caller pays (pack + upload +
    # solve + gather + symmetrise).  The samples as the reference holds them: a column-major Matrix{Int64}, K x (1+n)
    # (sampling.jl:52-54), 8.2 GB at this config.  Rank 0 of a 1-GPU run only (the matrix is built from the device's samples).
    if rank == 0 and world == 1 and args.full and not args.no_learn and not args.no_host_learn:
        avail_gb = 0.0
        try:
            avail_gb = [int(ln.split()[1]) for ln in open("/proc/meminfo") if ln.startswith("MemAvailable")][0] / 1e6
        except Exception:
            pass
        need_gb = 8.0 * K * (n + 1) / 1e9 + K * n / 1e9
        if avail_gb > 1.5 * need_gb + 8:
            spins_h = prob.spins()
            hist = np.empty((K, n + 1), dtype=np.int64, order="F")
            hist[:, 0] = 1
            for j0 in range(0, n, 64):
                hist[:, 1 + j0:1 + j0 + 64] = spins_h[:, j0:j0 + 64]
            del spins_h
            runs = []
            for _ in range(3):
                t0 = time.perf_counter()
                with gml.Problem(hist, device=device) as ph:
                    t1 = time.perf_counter()
                    Rh, kh, sh = ph.learn("RISE", 0.4, tol=1e-9, precision=args.precision, raise_on_fail=False, matrix=True)  # solve + :184-186 on the device
                    t2 = time.perf_counter()
                    it = ph.ingest_times()
                runs.append({"pack_s": it["pack_s"], "upload_s": it["upload_s"], "images_s": it["images_s"], "alloc_s": it["alloc_s"],
                             "weights_s": it["weights_s"], "create_s": t1 - t0, "symmetrise_s": sh["t_assemble"],
                             "solve_s": t2 - t1, "total_s": t2 - t0})
            med = sorted(runs, key=lambda r: r["total_s"])[1]
            extra["learn_from_host"] = dict(med, input="column-major Int64 K x (1+n) histogram (Matrix{Int64} of sample())",
                                            host_bytes=int(hist.nbytes), pcie_bytes=int(K * n / 8 + 8 * K),
                                            runs_total_s=[r["total_s"] for r in runs],
                                            same_result_as_device_samples=bool(out is not None and np.array_equal(Rh, 0.5 * (out + out.T))),
                                            max_err_vs_true_model=float(np.abs(Rh - J).max()))
            del hist
        else:
            extra["learn_from_host"] = {"skipped": "needs %.0f GB of host memory, %.0f available" % (1.5 * need_gb + 8, avail_gb)}

    # ---- what every rank of an 8-GPU run of THIS problem would solve, measured one shard after the other on this GPU (rank 0 of a 1-GPU
    # run only).  A PROJECTION of the N = 8 line, clearly not a measurement of it: no second device, no RCCL, no contention for the host.
    # It exists because the one thing that does not scale with the node count -- the latency-bound direction phase of a small shard -- can
    # be measured on one GPU, and because an 8-GPU node is not always available to the driver (SCALE_r01..r04 are skip records).
    if rank == 0 and world == 1 and args.full and not args.no_learn and not args.no_shards and n % 8 == 0 and "learn_wall_s" in extra:
        parts, shard = 8, []
        for r8 in range(parts):
            a0, a1 = r8 * n // parts, (r8 + 1) * n // parts
            with gml.Problem(model=J, num_samples=K, seed=0, node_range=(a0, a1), device=device) as ps:
                ps.learn("RISE", 0.4, tol=1e-9, precision=args.precision, raise_on_fail=False)
                ts = []
                for _ in range(3):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    _, _, st8 = ps.learn("RISE", 0.4, tol=1e-9, precision=args.precision, raise_on_fail=False)
                    ts.append(time.perf_counter() - t0)
                km8 = ps.bench_pass_resident("RISE", np.ascontiguousarray(J[a0:a1]), steps=10, warmup=2, precision=args.precision)
            shard.append({"nodes": [a0, a1], "learn_s": sorted(ts)[1], "iterations": st8["iterations"], "passes": st8["passes"],
                          "t_pass_s": st8["t_pass"], "t_hess_s": st8["t_hess"], "not_converged": st8["not_converged"],
                          "pass_ms": float(km8["device_ms_per_pass"])})
        worst_learn, worst_pass = max(q["learn_s"] for q in shard), max(q["pass_ms"] for q in shard)
        extra["projection_8gpu"] = {
            "kind": "projection from one-GPU runs of every rank's workload (NOT a multi-GPU measurement)",
            "precision": args.precision, "shards": shard, "slowest_shard_learn_s": worst_learn, "slowest_shard_pass_ms": worst_pass,
            "learn_scaling": extra["learn_wall_s"] / worst_learn, "pass_scaling": km["device_ms_per_pass"] / worst_pass,
            "not_included": "the final all-gather of the n x n result (1 MiB per rank over xGMI), the ranks' barrier"}

    # ---- one pass over a WEIGHTED histogram (rank 0 of a 1-GPU run only): non-uniform counts take the weight-loading template
    # of the forward kernel (UNIW = false); the timed region above runs the uniform-weight one (every count equal) -----------
    spins = None
    if rank == 0 and world == 1 and args.full and not (args.no_cpu and args.no_weighted):
        spins = prob.spins()  # the K x n configurations the GPU path works on
    if spins is not None and not args.no_weighted:
        counts_w = 1.0 + (np.arange(K) % 3)
        with gml.Problem(counts=counts_w, spins=spins, device=device) as pw:
            sw = max(3, min(20, args.steps // 10))
            pw.bench_pass_resident("RISE", theta, steps=2, warmup=0, precision=args.precision)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            kmw = pw.bench_pass_resident("RISE", theta, steps=sw, warmup=0, precision=args.precision)
            torch.cuda.synchronize()
            ew = time.perf_counter() - t0
        extra["ms_per_step_weighted"] = ew / sw * 1e3
        extra["weighted"] = {"counts": "1 + (k mod 3)", "steps": sw, "fwd_ms": kmw["fwd_ms"], "bwd_ms": kmw["bwd_ms"],
                             "device_ms_per_pass": kmw["device_ms_per_pass"], "value": n * sw / ew, "unit": "node-evals/s"}

    # ---- CPU baseline (rank 0 of a 1-GPU run only) -----------------------------------------------------------------
    cpu = None
    if rank == 0 and world == 1 and args.full and not args.no_cpu:
        from oracle import oracle as O
        hc = O.host_cpus()
        threads = hc["threads"]
        cpu_model, phys = "unknown", None
        try:
            info = open("/proc/cpuinfo").read().split("\n\n")
            cpu_model = [ln.split(":", 1)[1].strip() for ln in info[0].splitlines() if ln.startswith("model name")][0]
            allowed = os.sched_getaffinity(0)
            ids = set()
            for blk in info:
                kv = {ln.split(":", 1)[0].strip(): ln.split(":", 1)[1].strip() for ln in blk.splitlines() if ":" in ln}
                if "processor" in kv and int(kv["processor"]) in allowed:
                    ids.add((kv.get("physical id", "0"), kv.get("core id", kv["processor"])))
            phys = len(ids)
        except Exception:
            pass
        # (1) objective/gradient rate: the oracle's blocked FP64 restatement (32 nodes share one sweep over the spins,
        # OpenMP over node blocks x sample chunks, all host threads), on a bounded sample of nodes at full K and n
        nodes = (np.arange(32, dtype=np.int64) * (n // 32)) % n
        O.objgrad_nodes("RISE", None, spins[:4096], nodes, J[nodes])  # load the library, warm the threads
        t0 = time.perf_counter()
        O.objgrad_nodes("RISE", None, spins, nodes, J[nodes])
        t1 = time.perf_counter() - t0
        nn = int(min(n, max(32, (args.cpu_seconds / max(t1, 1e-3)) * 32 // 32 * 32)))
        nodes = (np.arange(nn, dtype=np.int64) * max(1, n // nn)) % n
        t0 = time.perf_counter()
        f_cpu, g_cpu = O.objgrad_nodes("RISE", None, spins, nodes, J[nodes])
        t_cpu = time.perf_counter() - t0
        # parity spot check of the timed GPU operator against the oracle on the same rows
        f_gpu, g_gpu = prob.objgrad("RISE", nodes, J[nodes], precision=args.precision)
        assert np.array_equal(g_gpu, g_res[nodes]) and np.array_equal(f_gpu, f_res[nodes]), "timed passes != operator output"
        # ... and ONE thread: the per-node-evaluation time of the same code (one block of 32 nodes, a quarter of the samples,
        # scaled: the sweep is linear in K)
        O.lib().gml_oracle_set_threads(1)
        k1 = max(4096, K // 4)
        t0 = time.perf_counter()
        O.objgrad_nodes("RISE", None, spins[:k1], nodes[:32], J[nodes[:32]])
        t_one = (time.perf_counter() - t0) * (K / k1)
        O.lib().gml_oracle_set_threads(threads)
        cpu = {"value": nn / t_cpu, "unit": "node-evals/s", "cores": threads, "threads": threads, "cpu_model": cpu_model, "kind": "port",
               "cpus_visible": hc["visible"], "cgroup_cpu_quota": hc["quota"], "physical_cores_visible": phys,
               "cores_note": "`cores` = the OpenMP threads actually used (= `threads`; the contract's field); the container may use "
                             "`cgroup_cpu_quota` CPUs' worth of time out of `cpus_visible` logical CPUs (`physical_cores_visible` "
                             "physical cores); thread count = 2 x quota, the measured optimum on this box class",
               "sample": f"{nn} node evaluations (nodes spread over 0..{n - 1}) at full K={K}, n={n}; oracle/gml_oracle_fast.c "
                         f"gml_oracle_objgrad_nodes: FP64, 32-node blocks share one sweep over the spins, OpenMP with {threads} threads",
               "seconds": t_cpu, "gflops": 4.0 * K * n * nn / t_cpu / 1e9,
               "ms_per_node_eval_all_threads": t_cpu / nn * 1e3,
               "single_thread": {"ms_per_node_eval": t_one / 32 * 1e3, "value": 32 / t_one, "unit": "node-evals/s", "gflops": 4.0 * K * n * 32 / t_one / 1e9,
                                 "sample": f"32 node evaluations (one block) over {k1} of the {K} configurations, one thread, scaled to K"},
               "parity_max_abs_grad_diff": float(np.abs(g_gpu - g_cpu).max()),
               "parity_max_rel_f_diff": float(np.abs(f_gpu / f_cpu - 1).max())}
        # (2) CPU learn() wall-clock, same method (batched working-set Newton), same tolerance:
        #     config 2 (n=256, K=1e5) in full on both sides; this config in full when the measured rate predicts it fits the budget
        J2 = synthetic.block_ising_model(256, block=16, seed=0)
        with gml.Problem(model=J2, num_samples=100000, seed=0, device=device) as p2:
            t0 = time.perf_counter()
            o2, k2, s2 = p2.learn("RISE", 0.4, tol=1e-9, precision=args.precision, raise_on_fail=False)
            t_gpu2 = time.perf_counter() - t0
            sp2 = p2.spins()
        t0 = time.perf_counter()
        c2, ck2, cs2 = O.learn_pair_fast(None, sp2, "RISE", c=0.4, tol=1e-9)
        t_cpu2 = time.perf_counter() - t0
        cpu["learn_c2"] = {"config": "n=256, K=1e5, RISE(0.4), tol 1e-9", "cpu_s": t_cpu2, "gpu_s": t_gpu2,
                           "speedup": t_cpu2 / t_gpu2, "cpu_passes": cs2["passes"], "cpu_node_evals": cs2["node_evals"],
                           "cpu_max_kkt": float(ck2.max()), "gpu_max_kkt": float(k2.max()),
                           "max_abs_diff_cpu_vs_gpu": float(np.abs(c2 - o2).max())}
        if not args.no_learn:
            t_pred = extra["learn_node_evals"] / cpu["value"]
            if args.cpu_learn_full or t_pred <= args.cpu_learn_max_s:
                t0 = time.perf_counter()
                c3, ck3, cs3 = O.learn_pair_fast(None, spins, "RISE", c=0.4, tol=1e-9)
                t_cpu3 = time.perf_counter() - t0
                cpu["learn_this_config"] = {"cpu_s": t_cpu3, "gpu_s": extra["learn_wall_s"], "speedup": t_cpu3 / extra["learn_wall_s"],
                                            "kind": "measured", "cpu_max_kkt": float(ck3.max()), "cpu_passes": cs3["passes"],
                                            "cpu_node_evals": cs3["node_evals"], "predicted_s": t_pred,
                                            "max_abs_diff_cpu_vs_gpu": float(np.abs(c3 - out).max()),
                                            "rel_frobenius_diff_cpu_vs_gpu": float(np.linalg.norm(c3 - out) / np.linalg.norm(c3))}
            else:
                cpu["learn_this_config"] = {"cpu_s": t_pred, "gpu_s": extra["learn_wall_s"], "speedup": t_pred / extra["learn_wall_s"],
                                            "kind": "extrapolated: the GPU run's node evaluations / the measured CPU rate (Hessians and "
                                                    "solves not counted), because that predicts more than --cpu-learn-max-s = %g s; "
                                                    "--cpu-learn-full measures it" % args.cpu_learn_max_s}
    del spins

    if rank == 0:
        line = {"metric": "obj/grad evals/sec (RISE, n=%d spins, %d samples)" % (n, K), "value": value,
                "unit": "node-evals/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
                "ms_per_step": ms_per_step, "higher_is_better": True, "scaling": "strong", "vs_baseline": None,
                "dtype": args.precision, "data": "synthetic",
                "config": {"workload": "BASELINE configs[2]-shaped RISE pass: n=%d random block-Ising (%d-spin blocks), "
                                       "%d samples drawn on the device, all n node-wise objective+gradient evaluations per step"
                                       % (n, args.block, K),
                           "n": n, "samples": K, "nodes_per_gpu": nloc, "parallelism": "node-shard x%d" % world,
                           "sample_and_pack_s": t_create},
                "roofline": roofline, "f64": f64, "i8x": others.get("i8x"), "cpu_baseline": cpu}
        if f64 is not None:
            # the same pass on the FP64 matrix cores (the reference's arithmetic, instruction for instruction)
            line.update({"value_f64": f64["value"], "ms_per_step_f64": f64["ms_per_step"], "roofline_f64": f64["roofline"]})
        if others.get("i8x") is not None:
            line.update({"value_i8x": others["i8x"]["value"], "ms_per_step_i8x": others["i8x"]["ms_per_step"]})
        notes = {"i8w": "dtype i8w = fixed point on the int8 matrix cores at the width of Float64: Theta in 54-bit int8 limbs (entries within a "
                        "factor two of a row's largest exact, the rest to 2^-55 of it), the weights V in dithered 47-bit limbs, exp in FP64, "
                        "integer GEMMs exact.  f and grad agree with the FP64-MFMA path and with the CPU oracle to the 1e-12 that path is held "
                        "to (tests/test_gpu_parity.py: FTOL/GTOL; this run: f64.max_*_diff_vs_headline, cpu_baseline.parity_*) on well-scaled "
                        "inputs such as this workload.  Under dynamic range -- dense Theta, sum|theta| 40..100, a few configurations carrying "
                        "the sum -- the 47 bits are relative to the row's largest weight and the deviation from the FP64-MFMA path was MEASURED "
                        "at <= 1.0e-11 (relative f) / 2.7e-11 (gradient / f) at K = 1e6 (tests hold 3e-10: test_i8w_dense_theta_dynamic_range*); "
                        "rows whose energies spread over hundreds of units go to the FP64 path under precision auto.",
                 "i8x": "dtype i8x = fixed point on the int8 matrix cores: Theta in 38-bit, V in dithered 31-bit int8 limbs, integer GEMMs exact; "
                        "f and grad differ from the FP64 evaluation by ~0.4*sqrt(K)*2^-31 of the largest weight (tests hold 1e-7 where the FP64 "
                        "and i8w paths hold 1e-12); north_star tolerance 1e-6 on the learned couplings.",
                 "f64": "dtype f64 = FP64 MFMA (v_mfma_f64_16x16x4_f64) throughout."}
        line["precision_note"] = notes[args.precision]
        line.update(extra)
        print(json.dumps(line))
    prob.close()
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
