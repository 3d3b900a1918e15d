"""Interleaved timing of several builds of libgml_hip (argv: tag=path ...) on one GPU; prints (step, fwd, bwd) ms.
AB_I8X=1 also times the i8x pass (a leg bench.py runs only under --full, a quarter of --steps): (step, fwd, bwd, i8x step, i8x fwd).
Every run is a child process with a time limit of its own (AB_TIMEOUT seconds, default 300); the first run that fails or
overruns ends the script with a non-zero status: nothing more is started on a GPU that has just failed a run."""
import subprocess, sys, json, os
libs = [a.split("=", 1) for a in sys.argv[1:]]
res = {t: [] for t, _ in libs}
limit = float(os.environ.get("AB_TIMEOUT", "300"))
legs = ["--full", "--no-sparse-theta", "--no-shards", "--no-host-learn"] if os.environ.get("AB_I8X", "0") not in ("", "0") else ["--no-i8x"]
for rnd in range(int(os.environ.get("AB_ROUNDS", "3"))):
    for tag, path in libs:
        env = dict(os.environ)
        if path: env["GML_LIB_OVERRIDE"] = path
        try:
            out = subprocess.run([sys.executable, "bench.py", "--steps", "40", "--warmup", "3", "--no-cpu", "--no-learn", "--no-f64", "--no-weighted"] + legs + os.environ.get("AB_ARGS", "").split(), env=env,
                                 capture_output=True, text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            print(tag, "TIMEOUT after", limit, "s", flush=True)
            sys.exit(124)
        try:
            if out.returncode != 0:
                raise RuntimeError(f"exit status {out.returncode}")
            d = json.loads(out.stdout.strip().splitlines()[-1])
        except Exception as e:
            print(tag, "FAILED", e, out.stdout[-300:], out.stderr[-800:], flush=True)
            sys.exit(out.returncode if out.returncode > 0 else 1)
        res[tag].append((round(d["ms_per_step"], 3), round(d["roofline"]["fwd_ms"], 3), round(d["roofline"]["bwd_ms"], 3)))
        if d.get("i8x"):
            res[tag][-1] += (round(d["i8x"]["ms_per_step"], 3), round(d["i8x"]["roofline"]["fwd_ms"], 3))
        print(tag, res[tag][-1], flush=True)
for tag, rows in res.items():  # per column: median, then min .. max over the rounds
    cols = [sorted(c) for c in zip(*rows)]
    print(tag, "median", tuple(c[len(c) // 2] if len(c) % 2 else round((c[len(c) // 2 - 1] + c[len(c) // 2]) / 2, 3) for c in cols),
          "range", tuple((c[0], c[-1]) for c in cols), flush=True)
