"""The host model of the matrix-free direction phase (tests/_newton_cg_reference.py) against itself and against brute force, without a
GPU: the restated split plan against an enumeration of the participating samples, the PCG replay with supplied products against Pcg
with a dense matrix (bit for bit), and the comparison function against records that carry one deliberate mistake each -- every one of
them must be noticed."""
import numpy as np
import pytest

import _newton_cg_reference as N
import _solver_reference as M


# ---- the plan -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Kp", [2048, 5120, 14336, 26624, 140288, 1 << 20, (1 << 24) + 1024, (1 << 25) + 4096])
def test_plan_against_enumeration(Kp):
    """Over a grid of (ngroups, Qfp, ksub): the chunks tile [0, Kp) with only the last one short, their count follows the stated rule, the
    participating samples {k: k mod kchunk < kpart} are whole blocks of 512 -- exactly plan_blocks -- and make up 1 / ksub of every whole
    chunk; wsub is the sum of the weights of the blocks those samples lie in."""
    rng = np.random.default_rng(Kp % 9973)
    wblk = rng.random(Kp // 512)
    k = np.arange(Kp, dtype=np.int64)
    for ngroups in (1, 2, 3, 16, 40):
        for Qfp in (64, 192, 256, 320, 1024):
            for ksub in (1, 2, 3, 5, 8):
                kchunk, kpart, nsplit = N.split_plan(Kp, ngroups, Qfp, ksub)
                tag = (Kp, ngroups, Qfp, ksub, kchunk, kpart, nsplit)
                tiles = ngroups * ((Qfp + 255) // 256)
                want = 8
                while want * tiles < 512:  # the smallest multiple of 8 that fills 512 workgroup slots
                    want += 8
                want = min(256, max(24, want))
                gran = 512 * ksub if ksub > 1 else 256
                assert kchunk % gran == 0 and kchunk >= 2048 and kpart * ksub == kchunk and kpart % 256 == 0, tag
                assert (nsplit - 1) * kchunk < Kp <= nsplit * kchunk, tag
                if Kp > 1 << 24:
                    assert kchunk <= 1 << 22, tag
                # no finer plan would do: a chunk one granule shorter breaks a rule (more chunks than wanted, or below the floor)
                shorter = kchunk - gran
                assert shorter < 2048 or -(-Kp // want) > shorter or (Kp > 1 << 24 and kchunk == (1 << 22) // gran * gran), tag
                if Kp > 1 << 22 and (ngroups > 2 or ksub in (3, 5)):
                    continue  # (the enumeration below is the expensive part: a sample of the large sizes)
                part = (k % kchunk) < kpart
                if ksub > 1:
                    blocks = np.flatnonzero(part[::512])
                    assert part.reshape(-1, 512).all(axis=1)[blocks].all() and not part.reshape(-1, 512).any(axis=1)[np.setdiff1d(np.arange(Kp // 512), blocks)].any(), tag
                    assert list(blocks) == N.plan_blocks(Kp, kchunk, kpart), tag
                    assert part[:(nsplit - 1) * kchunk].sum() * ksub == (nsplit - 1) * kchunk, tag
                    s = 0.0
                    for b in blocks:
                        s += wblk[b]
                    assert N.wsub(wblk, Kp, kchunk, kpart) == s, tag
                else:
                    assert part.all(), tag


def test_rules_at_their_thresholds():
    assert N.ksub_rule(14000, 47, 0, True) == 8 and N.ksub_rule(26000, 200, 0, True) == 4 and N.ksub_rule(26000, 130, 0, True) == 6
    assert N.ksub_rule(26000, 5000, 0, True) == 1 and N.ksub_rule(26000, 200, 3, True) == 3 and N.ksub_rule(14000, 47, 0, False) == 1
    assert N.relax_schedule(14000, 47, 0, False) == [(2, 2), (4, 8)]
    assert N.relax_schedule(26000, 400, 0, False) == [(2, 2), (4, 4)] and N.relax_schedule(26000, 900, 0, False) == []
    assert N.relax_schedule(14000, 47, 3, False) == [] and N.relax_schedule(14000, 47, 1, False) == [] and N.relax_schedule(14000, 47, 0, True) == []
    assert N.is_coarse(0, 2, 31, 1e-3, 1e-7) and not N.is_coarse(0, 2, 32, 1e-3, 1e-7) and not N.is_coarse(1, 2, 31, 1e-3, 1e-7)
    assert not N.is_coarse(0, 2, 31, 0.5e-4, 1e-7) and N.is_coarse(0, 2, 31, 2e-4, 1e-7) and not N.is_coarse(0, 2, 31, 1e-5, 1e-9)
    assert N.eta_rule(2, 31, 1e-8) == 0.25 and N.eta_rule(2, 32, 1e-8) == 1e-4 and N.eta_rule(0, 5, 0.5) == 0.05 and N.eta_rule(0, 5, 1e-6, 0.0005) == 0.0005
    assert N.stays_live((1.0, 10.0, 1.0, 0.0), 0.25) and not N.stays_live((0.625, 10.0, 1.0, 0.0), 0.25) and not N.stays_live((1.0, 10.0, 0.0, 0.0), 0.25)
    assert N.solves_again(1, 0.06, 1.0) and not N.solves_again(0, 0.06, 1.0) and not N.solves_again(3, 0.05, 1.0)
    assert N.route_is_sparse(True, 19, 0.3, 64, 3) and not N.route_is_sparse(True, 20, 0.3, 64, 3) and N.route_is_sparse(True, 38, 0.3, 64, 33)
    assert not N.route_is_sparse(False, 1, 0.3, 64, 3) and not N.route_is_sparse(True, 1, -1.0, 64, 3) and N.route_is_sparse(True, 10 ** 9, 1e30, 64, 3)
    assert not N.sparse_allowed("RPLE", 2) and N.sparse_allowed("RISE", 3) and not N.sparse_allowed("RISE", 4) and N.sparse_allowed("logRISE", 2)
    assert N.tile_layout([5, 0, 8, 9], 4) == ([0, 2, 2, 4], [4, 1, 4, 4, 4, 4, 1], [0, 0, 2, 2, 3, 3, 3])
    sc = N.scales("logRISE", [0.5, 2.0], 4, 4096, 512, 0.25)
    assert sc[0] == 512 and list(sc[1]) == [8.0, 2.0, 4.0, 4.0]
    assert N.scales("logRISE", [0.5, 2.0], 4, 4096, 512, 0.0)[0] == 4096 and list(N.scales("RISE", [0.5, 2.0], 4, 4096, 4096, 0.25)[1]) == [1.0] * 4


# ---- the replay ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, np.longdouble])
@pytest.mark.parametrize("s2", [0.0, 1.0])
def test_supplied_products_replay_the_dense_model_bit_for_bit(dtype, s2):
    rng = np.random.default_rng(7)
    Qp, T = 40, 8
    X = rng.choice([-1.0, 1.0], size=(400, Qp))
    Hd = (X * rng.random(400)[:, None]).T @ X / 400
    g = rng.normal(size=Qp) * 0.05
    Hd = Hd + s2 * np.outer(g, g) / 0.7
    x = rng.normal(size=Qp) * (rng.random(Qp) < 0.5)
    kind = np.full(Qp, 2)
    kind[[3, 17]] = 0
    kind[Qp - 1] = 1
    pg = M.pseudo_grad(x, rng.normal(size=Qp), np.where(kind == 2, 0.3, 0.0))
    a = M.Pcg(Hd, 0.7, s2, x, pg, g, kind, T, dtype)
    b = M.Pcg(None, 0.7, s2, x, pg, g, kind, T, dtype, Minv=a.Minv)
    same = lambda: all(np.array_equal(getattr(a, k), getattr(b, k)) for k in ("d", "r", "z", "p", "Wm")) and \
        all(getattr(a, k) == getattr(b, k) for k in ("rs", "rs0", "pHp", "rz"))
    assert same()
    for _ in range(5):
        a.step()
        b.step(a.Hd @ b.p)
        assert same()
    fa = a.faces()
    fb = b.faces(lambda d: a.Hd @ d)
    assert fa["n"] == fb["n"] > 0 and same()
    for _ in range(3):
        a.step()
        b.update(a.Hd @ b.p)
        b.advance()
        assert same()


# ---- the comparison notices every mistake ----------------------------------------------------------------------------------------------
def _record(form, mut=None, **kw):
    S = N.Synthetic(form, seed=0, **kw)
    # rows 0 and 1 still admit violators far from their optimum (the coarse group), row 2 has its support and two different residuals
    nviol, nsupp, kkt = [3, 3, 0, 0], [8, 8, 9, 9], [1e-2, 3e-2, 1e-9, 1e-3]
    return S, N.simulate(S, nviol, nsupp, kkt, mut)


def _check(S, ev, replay=True):
    t = N.Tally()
    N.check_iteration(ev, S.par, S.wblk, t, product=S.product, replay=replay)
    return t


@pytest.mark.parametrize("form", ["RISE", "logRISE"])
def test_the_model_passes_its_own_comparison(form):
    S, ev = _record(form, R=4)
    t = _check(S, ev)
    print(f"{form}: {len(ev)} events, branches {sorted(t.seen)}, products checked {t.checked}, largest product error / bound {t.product:.3g}")
    assert {"coarse", "fine", "relax2", "relax4", "resolve", "entries", "shrank"} <= t.seen, sorted(t.seen)
    assert t.checked > 10 and t.pcg <= 1.0  # (the record is the float64 replay itself: at the distance delta_k, no further)


MUTATIONS = [("neighbour", "RISE", "product of row"), ("no_wsub", "RISE", "sc of row"), ("no_z", "logRISE", "sc of row"), ("relax_early", "RISE", "expected"),
             ("eta_row", "RISE", "rows"), ("negative_php", "RISE", "expected"), ("wsub_head", "RISE", "wsub"), ("wrow", "RISE", "wrow")]


@pytest.mark.parametrize("mut,form,what", MUTATIONS)
def test_each_mistake_is_noticed(mut, form, what):
    """a product taken from the neighbouring row's weights; sc without 1 / wsub; sc without 1 / Z; the relaxed products one step early (at
    steps 1 and 3); eta from another row's kkt; a live list that keeps a row with pHp <= 0; wsub over the first kpart samples only; a
    tile whose wrow is off by one.  The decisions are checked without the replay, so that it is the rule that notices."""
    S, ev = _record(form, mut, R=4)
    with pytest.raises(AssertionError) as ei:
        _check(S, ev, replay=False)
    assert what in str(ei.value), str(ei.value)
    S, ev = _record(form, None, R=4)
    _check(S, ev, replay=False)


def test_weightless_sub_sample_falls_back():
    """no counts on the blocks the coarse plan samples (blocks 0 and 8 of 12: kchunk 4096, kpart 512): kpart = kchunk, sc without 1 / wsub"""
    S, ev = _record("RISE", R=4, zero_blocks=(0, 8))
    t = _check(S, ev)
    plans = [e for e in ev if e["tag"] == "plan" and e["ksub"] == 8]
    assert plans and all(e["wsub"] == 0 and e["kpart"] == e["kchunk"] == 4096 and (e["sc"] == 1).all() for e in plans) and "weightless" in t.seen
