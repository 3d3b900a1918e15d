"""The order of refusals of the seven term-list chain entry points, without a GPU: every one of these faults is reported before the
device lookup.  Each case gives an entry point inputs that are wrong in two ways at once -- two neighbours of its check sequence -- and
asserts the code and the text of gml_last_error.  The expected pairs are literals, recorded from the library of the commit before the
host half of the family moved into its own file (gml_chains_host.cpp), so they hold that move, and any later one, to the same answers.

What the cases cover, per entry point, in the order of its checks:
  _chains      out, term pointers, chain arguments, term values (weight, then key), n limit, histogram limits, incidence limits
  _tempered    the same with the ladder between the chain arguments and the term values
  _ais         log_weights, term pointers, n, chains, schedule, term values, n limit, incidence limits
  _conditional, conditional_means, _masked, conditional_means_masked
               out / means, evidence, hidden / mask, term pointers, n against the evidence, the mask handle's shape (masked), replicas,
               chain arguments.  The handles are size-only stubs (no rows), so the chain arguments always answer and the checks after
               them (no hidden spin, term values, n limit, the masked tile, incidence limits) cannot be reached without a device:
               test_order_of_refusals_past_the_chain_arguments in tests/test_gpu_conditional.py and tests/test_gpu_masked.py pins
               those pairs on handles with rows."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import ROOT

SO = os.path.join(ROOT, "graphicalmodellearning.jl_amd", "libgml_hip.so")
EINVAL, EUNSUPPORTED = 1, 5
BIG = 20000  # above the kernels' limit of 16384 spins


def bind(L):
    p, i32, i64, u64 = C.c_void_p, C.c_int, C.c_int64, C.c_uint64
    L.gml_problem_create_mcmc_terms_chains.argtypes = [p, i32, p, i64, i64, i64, i64, i32, i32, u64, i32, i32, i64, i64, i32, p]
    L.gml_problem_create_mcmc_terms_tempered.argtypes = [p, i32, p, i64, i64, i64, i64, i32, i32, p, i32, i32, u64, i32, i32, i64, i64, i32, p, p]
    L.gml_log_partition_ais.argtypes = [p, i32, p, i64, i64, i64, p, i64, i32, u64, i32, p, p, p, p]
    L.gml_problem_create_mcmc_terms_conditional.argtypes = [p, i32, p, i64, i64, p, p, i32, i64, i32, i32, u64, i32, i64, i64, p]
    L.gml_conditional_means.argtypes = [p, i32, p, i64, i64, p, p, i32, i64, i32, i32, u64, p]
    L.gml_problem_create_mcmc_terms_masked.argtypes = [p, i32, p, i64, i64, p, p, i32, i64, i32, i32, u64, i32, i64, i64, p]
    L.gml_conditional_means_masked.argtypes = [p, i32, p, i64, i64, p, p, i32, i64, i32, i32, u64, p]
    L.gml_test_problem_stub.argtypes = [i64, i64, i32, i64, i64, C.POINTER(p)]
    L.gml_problem_destroy.argtypes = [p]
    L.gml_problem_destroy.restype = None
    L.gml_last_error.restype = C.c_char_p
    return L


def ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


# the term lists: a good one, and one fault each
GOOD = (np.array([[0, 1, -1], [1, 2, 0], [2, -1, -1]], dtype=np.int32), np.array([0.3, -0.2, 0.5]))
NONFINITE = (GOOD[0], np.array([0.3, np.inf, 0.5]))
KEY_OUT = (np.array([[0, 1, -1], [1, 7, 0], [2, -1, -1]], dtype=np.int32), GOOD[1])
NINE = (np.arange(9, dtype=np.int32).reshape(1, 9), np.array([0.1]))  # a term of nine distinct spins
NOKEYS = (None, GOOD[1])


def build_cases(L):
    """[(id, thunk)]: thunk() makes the call and returns its code; the stub handles live in the closure"""
    stubs = {}

    def stub(role, n):
        if (role, n) not in stubs:
            h = C.c_void_p()
            assert L.gml_test_problem_stub(n, n, 2, 0, n, C.byref(h)) == 0
            stubs[role, n] = h
        return stubs[role, n]

    out = C.c_void_p()
    betas2 = np.array([1.0, 0.5])
    sched = np.array([0.0, 0.5, 1.0])
    logw = np.zeros(4)
    means = np.zeros(64)
    hidden = np.array([1, 0, 1, 0, 0, 0, 0, 0, 0], dtype=np.uint8)

    def chains(terms, n=3, thin=1, histogram=0, o=True):
        k, w = terms
        stride = 1 if k is None else k.shape[1]
        return lambda: L.gml_problem_create_mcmc_terms_chains(ptr(k), stride, ptr(w), len(w), n, 4, 2, 5, thin, 0, histogram, 2, 0, n, 0,
                                                              C.byref(out) if o else None)

    def tempered(terms, n=3, thin=1, histogram=0, o=True, betas=betas2, replicas=2):
        k, w = terms
        stride = 1 if k is None else k.shape[1]
        return lambda: L.gml_problem_create_mcmc_terms_tempered(ptr(k), stride, ptr(w), len(w), n, 4, 2, 5, thin, ptr(betas), replicas, 1, 0,
                                                                histogram, 2, 0, n, 0, None, C.byref(out) if o else None)

    def ais(terms, n=3, nchains=4, betas=sched, lw=True):
        k, w = terms
        stride = 1 if k is None else k.shape[1]
        nb = 0 if betas is None else len(betas)
        return lambda: L.gml_log_partition_ais(ptr(k), stride, ptr(w), len(w), n, nchains, ptr(betas), nb, 1, 0, 0, ptr(logw) if lw else None,
                                               None, None, None)

    def cond(entry, terms=GOOD, n=3, ev=3, second=3, replicas=1, thin=1, sink=True):
        """entry: conditional / means / masked / means_masked.  ev, second: sizes of the stub handles (None: NULL); for the fixed-mask
        entries `second` not None gives the hidden array"""
        k, w = terms
        stride = 1 if k is None else k.shape[1]
        masked = "masked" in entry
        common = lambda: (ptr(k), stride, ptr(w), len(w), n, None if ev is None else stub("evidence", ev),
                          None if second is None else stub("mask", second) if masked else ptr(hidden), replicas, 1, 5, thin, 0)
        if entry == "conditional":
            return lambda: L.gml_problem_create_mcmc_terms_conditional(*common(), 2, 0, n, C.byref(out) if sink else None)
        if entry == "means":
            return lambda: L.gml_conditional_means(*common(), ptr(means) if sink else None)
        if entry == "masked":
            return lambda: L.gml_problem_create_mcmc_terms_masked(*common(), 2, 0, n, C.byref(out) if sink else None)
        return lambda: L.gml_conditional_means_masked(*common(), ptr(means) if sink else None)

    cases = []
    for name, f in (("chains", chains), ("tempered", tempered)):
        cases += [
            (f"{name}: out NULL + keys NULL", f(NOKEYS, o=False)),
            (f"{name}: keys NULL + thin 0", f(NOKEYS, thin=0)),
            (f"{name}: non-finite weight + n above the limit", f(NONFINITE, n=BIG)),
            (f"{name}: non-finite weight + key out of range", f((KEY_OUT[0], NONFINITE[1]))),
            (f"{name}: key out of range + histogram over 100 spins", f((np.array([[0, 200]], dtype=np.int32), np.array([0.1])), n=100, histogram=1)),
            (f"{name}: n above the limit + histogram over more than 64 spins", f(GOOD, n=BIG, histogram=1)),
            (f"{name}: n above the limit + nine distinct spins", f(NINE, n=BIG)),
            (f"{name}: histogram over more than 64 spins + nine distinct spins", f(NINE, n=100, histogram=1)),
            (f"{name}: nine distinct spins", f(NINE, n=9)),
        ]
    cases += [
        ("chains: thin 0 + non-finite weight", chains(NONFINITE, thin=0)),
        ("tempered: thin 0 + betas NULL", tempered(GOOD, thin=0, betas=None)),
        ("tempered: three replicas + non-finite weight", tempered(NONFINITE, betas=np.array([1.0, 0.5, 0.2]), replicas=3)),
        ("tempered: increasing betas + key out of range", tempered(KEY_OUT, betas=np.array([0.5, 1.0]))),
        ("ais: log_weights NULL + keys NULL", ais(NOKEYS, lw=False)),
        ("ais: keys NULL + n 0", ais(NOKEYS, n=0)),
        ("ais: n 0 + chains 0", ais(GOOD, n=0, nchains=0)),
        ("ais: chains 0 + betas NULL", ais(GOOD, nchains=0, betas=None)),
        ("ais: one beta + non-finite weight", ais(NONFINITE, betas=np.array([0.0]))),
        ("ais: betas[0] not 0 + key out of range", ais(KEY_OUT, betas=np.array([0.5, 1.0]))),
        ("ais: non-finite weight + n above the limit", ais(NONFINITE, n=BIG)),
        ("ais: n above the limit + nine distinct spins", ais(NINE, n=BIG)),
        ("ais: nine distinct spins", ais(NINE, n=9)),
    ]
    for entry in ("conditional", "means", "masked", "means_masked"):
        second = "mask" if "masked" in entry else "hidden"
        cases += [
            (f"{entry}: sink NULL + evidence NULL", cond(entry, ev=None, sink=False)),
            (f"{entry}: evidence NULL + {second} NULL", cond(entry, ev=None, second=None)),
            (f"{entry}: {second} NULL + mismatched n", cond(entry, second=None, n=4)),
            (f"{entry}: {second} NULL + keys NULL", cond(entry, terms=NOKEYS, second=None)),
            (f"{entry}: keys NULL + mismatched n", cond(entry, terms=NOKEYS, n=4)),
            (f"{entry}: mismatched n + replicas 0", cond(entry, n=4, replicas=0)),
            (f"{entry}: replicas 0 + key out of range", cond(entry, terms=KEY_OUT, replicas=0)),
            (f"{entry}: chain arguments + key out of range", cond(entry, terms=KEY_OUT, thin=0)),
            (f"{entry}: chain arguments + non-finite weight", cond(entry, terms=NONFINITE)),
        ]
        if "masked" in entry:
            cases += [
                (f"{entry}: mismatched n + mismatched mask handle", cond(entry, n=4, second=4)),
                (f"{entry}: mismatched mask handle + replicas 0", cond(entry, second=4, replicas=0)),
            ]
    return cases, stubs


# (code, gml_last_error) of every case, from the library of the parent commit
EXPECTED = {
    'chains: out NULL + keys NULL':
        (1, 'out is NULL'),
    'chains: keys NULL + thin 0':
        (1, 'NULL or malformed term list'),
    'chains: non-finite weight + n above the limit':
        (1, 'weight of term 1 is not finite'),
    'chains: non-finite weight + key out of range':
        (1, 'weight of term 1 is not finite'),
    'chains: key out of range + histogram over 100 spins':
        (1, 'term 0 names spin 200 outside [0,100)'),
    'chains: n above the limit + histogram over more than 64 spins':
        (5, 'the term-list chain kernel supports n <= 16384 spins (n = 20000)'),
    'chains: n above the limit + nine distinct spins':
        (5, 'the term-list chain kernel supports n <= 16384 spins (n = 20000)'),
    'chains: histogram over more than 64 spins + nine distinct spins':
        (5, 'histogramming on the device needs n <= 64 spins (n = 100)'),
    'chains: nine distinct spins':
        (5, 'term 0 names 9 distinct spins: the term-list chain kernel supports at most 8'),
    'tempered: out NULL + keys NULL':
        (1, 'out is NULL'),
    'tempered: keys NULL + thin 0':
        (1, 'NULL or malformed term list'),
    'tempered: non-finite weight + n above the limit':
        (1, 'weight of term 1 is not finite'),
    'tempered: non-finite weight + key out of range':
        (1, 'weight of term 1 is not finite'),
    'tempered: key out of range + histogram over 100 spins':
        (1, 'term 0 names spin 200 outside [0,100)'),
    'tempered: n above the limit + histogram over more than 64 spins':
        (5, 'the term-list chain kernel supports n <= 16384 spins (n = 20000)'),
    'tempered: n above the limit + nine distinct spins':
        (5, 'the term-list chain kernel supports n <= 16384 spins (n = 20000)'),
    'tempered: histogram over more than 64 spins + nine distinct spins':
        (5, 'histogramming on the device needs n <= 64 spins (n = 100)'),
    'tempered: nine distinct spins':
        (5, 'term 0 names 9 distinct spins: the term-list chain kernel supports at most 8'),
    'chains: thin 0 + non-finite weight':
        (1, 'chains, samples_per_chain, burn_in and thin must be at least 1'),
    'tempered: thin 0 + betas NULL':
        (1, 'chains, samples_per_chain, burn_in and thin must be at least 1'),
    'tempered: three replicas + non-finite weight':
        (1, 'replicas must be one of 1, 2, 4, 8, 16, 32, 64 (given 3)'),
    'tempered: increasing betas + key out of range':
        (1, 'betas must not increase (betas[1] > betas[0])'),
    'ais: log_weights NULL + keys NULL':
        (1, 'log_weights is NULL'),
    'ais: keys NULL + n 0':
        (1, 'NULL or malformed term list'),
    'ais: n 0 + chains 0':
        (1, 'n must be positive'),
    'ais: chains 0 + betas NULL':
        (1, 'chains must lie in [1, 2^31] (given 0)'),
    'ais: one beta + non-finite weight':
        (1, 'nbetas must be at least 2 (given 1)'),
    'ais: betas[0] not 0 + key out of range':
        (1, 'betas[0] must be 0 (the chains start from an exact draw at beta = 0)'),
    'ais: non-finite weight + n above the limit':
        (1, 'weight of term 1 is not finite'),
    'ais: n above the limit + nine distinct spins':
        (5, 'the term-list chain kernel supports n <= 16384 spins (n = 20000)'),
    'ais: nine distinct spins':
        (5, 'term 0 names 9 distinct spins: the term-list chain kernel supports at most 8'),
    'conditional: sink NULL + evidence NULL':
        (1, 'out is NULL'),
    'conditional: evidence NULL + hidden NULL':
        (1, 'evidence is NULL'),
    'conditional: hidden NULL + mismatched n':
        (1, 'hidden is NULL'),
    'conditional: hidden NULL + keys NULL':
        (1, 'hidden is NULL'),
    'conditional: keys NULL + mismatched n':
        (1, 'NULL or malformed term list'),
    'conditional: mismatched n + replicas 0':
        (1, "n = 4 differs from the evidence handle's 3 spins"),
    'conditional: replicas 0 + key out of range':
        (1, 'replicas must be at least 1 (given 0)'),
    'conditional: chain arguments + key out of range':
        (1, 'chains, samples_per_chain, burn_in and thin must be at least 1'),
    'conditional: chain arguments + non-finite weight':
        (1, 'chains, samples_per_chain, burn_in and thin must be at least 1'),
    'means: sink NULL + evidence NULL':
        (1, 'means is NULL'),
    'means: evidence NULL + hidden NULL':
        (1, 'evidence is NULL'),
    'means: hidden NULL + mismatched n':
        (1, 'hidden is NULL'),
    'means: hidden NULL + keys NULL':
        (1, 'hidden is NULL'),
    'means: keys NULL + mismatched n':
        (1, 'NULL or malformed term list'),
    'means: mismatched n + replicas 0':
        (1, "n = 4 differs from the evidence handle's 3 spins"),
    'means: replicas 0 + key out of range':
        (1, 'replicas must be at least 1 (given 0)'),
    'means: chain arguments + key out of range':
        (1, 'chains, samples_per_chain, burn_in and thin must be at least 1'),
    'means: chain arguments + non-finite weight':
        (1, 'chains, samples_per_chain, burn_in and thin must be at least 1'),
    'masked: sink NULL + evidence NULL':
        (1, 'out is NULL'),
    'masked: evidence NULL + mask NULL':
        (1, 'evidence is NULL'),
    'masked: mask NULL + mismatched n':
        (1, 'mask is NULL'),
    'masked: mask NULL + keys NULL':
        (1, 'mask is NULL'),
    'masked: keys NULL + mismatched n':
        (1, 'NULL or malformed term list'),
    'masked: mismatched n + replicas 0':
        (1, "n = 4 differs from the evidence handle's 3 spins"),
    'masked: replicas 0 + key out of range':
        (1, 'replicas must be at least 1 (given 0)'),
    'masked: chain arguments + key out of range':
        (1, 'chains, samples_per_chain, burn_in and thin must be at least 1'),
    'masked: chain arguments + non-finite weight':
        (1, 'chains, samples_per_chain, burn_in and thin must be at least 1'),
    'masked: mismatched n + mismatched mask handle':
        (1, "n = 4 differs from the evidence handle's 3 spins"),
    'masked: mismatched mask handle + replicas 0':
        (1, 'the mask handle (n = 4, 0 rows, device 0) differs from the evidence handle (n = 3, 0 rows, device 0)'),
    'means_masked: sink NULL + evidence NULL':
        (1, 'means is NULL'),
    'means_masked: evidence NULL + mask NULL':
        (1, 'evidence is NULL'),
    'means_masked: mask NULL + mismatched n':
        (1, 'mask is NULL'),
    'means_masked: mask NULL + keys NULL':
        (1, 'mask is NULL'),
    'means_masked: keys NULL + mismatched n':
        (1, 'NULL or malformed term list'),
    'means_masked: mismatched n + replicas 0':
        (1, "n = 4 differs from the evidence handle's 3 spins"),
    'means_masked: replicas 0 + key out of range':
        (1, 'replicas must be at least 1 (given 0)'),
    'means_masked: chain arguments + key out of range':
        (1, 'chains, samples_per_chain, burn_in and thin must be at least 1'),
    'means_masked: chain arguments + non-finite weight':
        (1, 'chains, samples_per_chain, burn_in and thin must be at least 1'),
    'means_masked: mismatched n + mismatched mask handle':
        (1, "n = 4 differs from the evidence handle's 3 spins"),
    'means_masked: mismatched mask handle + replicas 0':
        (1, 'the mask handle (n = 4, 0 rows, device 0) differs from the evidence handle (n = 3, 0 rows, device 0)'),
}


@pytest.fixture(scope="module")
def lib_cases():
    if not os.path.exists(SO):
        import __graft_entry__ as ge
        ge.build()
    L = bind(C.CDLL(SO))
    cases, stubs = build_cases(L)
    yield L, dict(cases)
    for h in stubs.values():
        L.gml_problem_destroy(h)


def test_every_case_has_a_recorded_answer(lib_cases):
    assert list(lib_cases[1]) == list(EXPECTED)


@pytest.mark.parametrize("case", list(EXPECTED))
def test_refusal_order(lib_cases, case):
    L, cases = lib_cases
    rc = cases[case]()
    msg = L.gml_last_error().decode()
    print(case, "->", rc, msg)
    assert (rc, msg) == EXPECTED[case]
