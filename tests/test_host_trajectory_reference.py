"""The host model of learn()'s iterations (tests/_trajectory_reference.py) on the CPU: its set_kh against a table written out by hand
from the documented rule (DESIGN.md 4.2 "Hessian budget", include/gml.h: hess_samples), its end point against the oracle's optimum, and
the cap on the records the GPU comparison may leave out -- for the model alone, on every case tests/test_gpu_solver_trajectory.py uses."""
import numpy as np
import pytest

import _trajectory_reference as T
from oracle import oracle as O


# (K, Kp, R, nactive, prec, knob 0, hess_samples) -> (Kh_base, nb, kstride, Kh, the blocks summed, "all" when hscale is 1)
# Kp = K rounded up to 1024; blocks = Kp / 512; want = base x max(1, R // nactive) when hess_samples == 0, else base;
# nb = min(blocks, max(2, ceil(want / 512))); nb x 512 >= K: everything; kstride = blocks // nb
TABLE = [
    # the strided case: 10 blocks, 1024 configurations pinned -> 2 blocks, every 5th
    ((5000, 5120, 24, 24, "f64", 0, 1024), (1024, 2, 5, 1024, [0, 5], "")),
    ((5000, 5120, 24, 1, "f64", 0, 1024), (1024, 2, 5, 1024, [0, 5], "")),           # pinned: nactive does not matter
    ((5000, 5120, 24, 24, "f64", 0, -1), (5120, 10, 1, 5120, list(range(10)), "all")),
    ((5000, 5120, 24, 24, "f64", 0, 100), (100, 2, 5, 1024, [0, 5], "")),             # at least two blocks
    ((5000, 5120, 24, 24, "f64", 0, 1536), (1536, 3, 3, 1536, [0, 3, 6], "")),        # 10 // 3
    ((5000, 5120, 24, 24, "f64", 0, 4608), (4608, 9, 1, 4608, list(range(9)), "")),   # 9 x 512 = 4608 < 5000: the first nine
    ((5000, 5120, 24, 24, "f64", 0, 4900), (4900, 10, 1, 5120, list(range(10)), "all")),
    ((5000, 5120, 24, 24, "f64", 0, 0), (32768, 10, 1, 5120, list(range(10)), "all")),  # the FP64 base covers K
    # the adaptive case: 18 blocks, base 1024 by knob 0
    ((9000, 9216, 16, 16, "f64", 1024, 0), (1024, 2, 9, 1024, [0, 9], "")),
    ((9000, 9216, 16, 9, "f64", 1024, 0), (1024, 2, 9, 1024, [0, 9], "")),            # 16 // 9 = 1
    ((9000, 9216, 16, 8, "f64", 1024, 0), (1024, 4, 4, 2048, [0, 4, 8, 12], "")),     # 16 // 8 = 2
    ((9000, 9216, 16, 5, "f64", 1024, 0), (1024, 6, 3, 3072, [0, 3, 6, 9, 12, 15], "")),
    ((9000, 9216, 16, 3, "f64", 1024, 0), (1024, 10, 1, 5120, list(range(10)), "")),  # 16 // 3 = 5; 18 // 10 = 1: the first ten
    ((9000, 9216, 16, 2, "f64", 1024, 0), (1024, 16, 1, 8192, list(range(16)), "")),
    ((8700, 9216, 16, 16, "f64", 0, 8704), (8704, 18, 1, 9216, list(range(18)), "all")),  # 17 x 512 >= 8700: take it all, 18 blocks
    ((9000, 9216, 16, 16, "f64", 0, 8704), (8704, 17, 1, 8704, list(range(17)), "")),     # 17 x 512 < 9000: one block short of all
    ((9000, 9216, 16, 1, "f64", 1024, 0), (1024, 18, 1, 9216, list(range(18)), "all")),
    ((9000, 9216, 16, 0, "f64", 1024, 0), (1024, 2, 9, 1024, [0, 9], "")),            # nobody active: the base
    ((9000, 9216, 16, 16, "f64", 1024, 2048), (2048, 4, 4, 2048, [0, 4, 8, 12], "")),  # hess_samples beats the knob
    # the bases: FP64 32 768; int8 clamp(2^23 / R, 32 768, 131 072)
    ((140000, 140288, 8, 8, "f64", 0, 0), (32768, 64, 4, 32768, list(range(0, 256, 4)), "")),  # 274 // 64 = 4
    ((140000, 140288, 8, 8, "i8w", 0, 0), (131072, 256, 1, 131072, list(range(256)), "")),
    ((140000, 140288, 8, 8, "i8x", 0, 0), (131072, 256, 1, 131072, list(range(256)), "")),
    ((140000, 140288, 8, 4, "i8x", 0, 0), (131072, 274, 1, 140288, list(range(274)), "all")),
    ((140000, 140288, 128, 128, "i8x", 0, 0), (65536, 128, 2, 65536, list(range(0, 256, 2)), "")),  # 2^23 / 128
    ((140000, 140288, 1024, 1024, "i8w", 0, 0), (32768, 64, 4, 32768, list(range(0, 256, 4)), "")),
    ((140000, 140288, 1024, 300, "i8w", 0, 0), (32768, 192, 1, 98304, list(range(192)), "")),  # 1024 // 300 = 3
]


@pytest.mark.parametrize("args,want", TABLE)
def test_set_kh_table(args, want):
    K, Kp, R, nactive, prec, knob0, hs = args
    base, nb, kstride, Kh, blocks, everything = want
    wblk = np.random.default_rng(Kp).uniform(0.5, 1.5, Kp // 512)
    wblk /= wblk.sum()
    assert T.kh_base(prec, R, Kp, knob0, hs) == base
    kh = T.set_kh(K, Kp, R, nactive, base, hs, wblk)
    assert (kh["nb"], kh["kstride"], kh["Kh"], kh["blocks"]) == (nb, kstride, Kh, blocks)
    if everything:
        assert kh["hscale"] == 1.0
    else:
        assert kh["hscale"] == pytest.approx(1.0 / wblk[blocks].sum(), rel=1e-14) and kh["hscale"] > 1.0


def test_set_kh_without_weight_takes_everything():
    wblk = np.full(10, 0.125)
    wblk[[0, 5]] = 0.0
    kh = T.set_kh(5000, 5120, 24, 24, 1024, 1024, wblk)
    assert (kh["nb"], kh["kstride"], kh["Kh"], kh["hscale"], kh["blocks"]) == (10, 1, 5120, 1.0, list(range(10)))
    wblk[5] = 0.125  # weight on one of the two: the sub-sample stands
    kh = T.set_kh(5000, 5120, 24, 24, 1024, 1024, wblk)
    assert (kh["nb"], kh["kstride"], kh["hscale"]) == (2, 5, 8.0)


def test_face_rounds_rule():
    assert T.face_rounds(5000, 128) == 0 and T.face_rounds(1 << 21, 128) == 2 and T.face_rounds(5000, 128, 3) == 2 and T.face_rounds(1 << 21, 128, 1) == 0


@pytest.mark.parametrize("name", T.F64_CASES)
def test_model_reaches_the_optimum_within_the_cap(name):
    """The long-double run ends at the oracle's optimum with kkt <= tol (the capped case: not converged, by construction); the branch the
    case is named for occurs; and the records its fragile decisions leave out stay within the cap: at most 10 %, none in iterations 0 to
    3, none where the named branch first occurs."""
    case, hi, lo, first, why = T.model(name)
    branch = T.branch_iters(name, hi)
    share = T.check_cap(case, hi, first, branch)
    print(f"{name}: {hi['iterations']} iterations, named branch in {branch}, {share:.1%} of the records left out {why}")
    if name.startswith("cap"):
        assert hi["not_converged"] == case.R and hi["iterations"] == 3
        return
    assert hi["not_converged"] == 0 and (hi["kkt"] <= case.tol).all()
    ref, kkt, _ = O.learn_pair(case.samples(), case.form, c=case.c, symmetrize=False, tol=1e-12)
    # strictly convex: |x - x*| <= kkt / (smallest curvature); 1e-7 / 1e-3 and some room
    err = np.abs(hi["rows"] - ref[case.node0:case.node1]).max()
    assert err <= 1e-4, err
    assert (hi["kkt"] == np.minimum(hi["kkt"], [min(q["best"], q["kkt"]) for q in hi["iters"][-1]["rows"]])).all()
