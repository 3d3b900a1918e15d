"""gml_structure_from_rows (csrc/gml_terms.hip: k_struct_sym + k_struct_sym3, k_struct_row) at config-5 size: n = 512, order 3 --
67.0 M row entries, rows and structure resident in HBM (device pointers).  HIP-event time per call over several windows (their
spread is printed) and the achieved rate on the bytes the call must move: 8 n P read, n P written.  The calls are host-blocking
(each waits for its kernels and frees its counter), so the figure is a whole-call rate, not a kernel's; run under
rocprofv3 --kernel-trace --stats, in a run of its own, for the per-kernel split.  Nothing is asserted but the kept count."""
import ctypes as C
import sys

import torch

sys.path.insert(0, ".")
import gml_amd as gml  # noqa: E402

_lib = gml._lib
n, order = 512, 3
P = 1 + (n - 1) + (n - 1) * (n - 2) // 2
rows = torch.randn((n, P), dtype=torch.float64, device="cuda")
S = torch.empty((n, P), dtype=torch.uint8, device="cuda")
L = _lib.lib()
nbytes = 8.0 * n * P + 1.0 * n * P
thr = 0.6745 / 3 ** 0.5  # the median |mean of three standard normals|: half of the triples are kept
for rule in ("mean", "row"):
    kept = C.c_int64()

    def call():
        _lib.check(L.gml_structure_from_rows(rows.data_ptr(), P, n, order, _lib.RULES[rule], thr, gml.FREE, gml.EXCLUDED, gml.FREE, 0, S.data_ptr(), P,
                                             C.byref(kept)))
    for _ in range(5):
        call()
    torch.cuda.synchronize()
    windows, reps = [], 100
    for _ in range(5):
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record()
        for _ in range(reps):
            call()
        ev1.record()
        torch.cuda.synchronize()
        windows.append(ev0.elapsed_time(ev1) / reps)
    assert kept.value == int((S[:, 1:] == gml.FREE).sum().item())
    ms = sorted(windows)[len(windows) // 2]
    print(f"rule {rule}: n = {n}, order {order}, {n * P} entries, kept {kept.value}; {ms:.3f} ms per call (median of {len(windows)} windows of "
          f"{reps} calls: {min(windows):.3f} .. {max(windows):.3f}); {nbytes / 1e6:.0f} MB to move -> {nbytes / ms / 1e6:.0f} GB/s = "
          f"{nbytes / ms / 1e6 / 8000:.3f} of 8 TB/s", flush=True)
