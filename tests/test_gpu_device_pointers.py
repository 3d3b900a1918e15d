"""The boundary where a caller's HBM-resident arrays enter and leave the library, held to what include/gml.h says about it.

A. Ordering.  A handle call runs on the handle's blocking stream and a handle-less call on the null stream: both are ordered after
   what the caller queued on the null stream (torch's default stream).  Every device INPUT in turn holds a decoy (valid data with
   another result); a delay, the device-to-device copy of the true input and an event are queued on the default stream; the event
   is asserted pending; the call follows with no synchronisation in between and must give the result of the true input.  Calls
   without a device input get the same treatment through their OUTPUT: a pending fill of the output array must not land on top of
   the result.
B. Completion.  When a call returns its stream is idle (gml_test_stream_idle / the default stream's query) and the outputs are read
   on a fresh non-blocking stream, with no synchronisation before.  Every run of every test below does both.
C. Layout.  Leading dimensions P + 3 (rows) and P + 5 (structures), every argument an interior pointer (doubles one element, bytes
   1 / 3 / 7 into an allocation), NaN / 0xFF in the padding of inputs, a sentinel bit pattern around every output: the data equal the
   host-pointer call's, everything outside the data keeps its bits.  In place where the header allows it.
D. Pointer kinds.  Pinned host arrays are host pointers; mixed operator arguments are refused position by position; gml_stderr takes
   each of its three arrays from either side.

References: the same call through host pointers (staging copies and the host-side layout code instead of the layout kernels), and for
the pure layout calls the models of tests/test_gpu_terms.py and tests/_structure_reference.py.  RISE throughout: its int8-limb results
are integers end to end, hence bit for bit; the FP64 operator calls add with floating-point atomics and are held to the 1e-13 of
tests/test_gpu_operator_export.py.

Measured on an MI355X (same process, device pointers, synchronised before the call, best of two warm calls; the library is the
parent commit's but for the hook), wall time at the shapes below -- pairwise n = 40, K = 3000; order 3 n = 12, K = 2000, P = 67:
gml_learn_terms 1.6-1.7 ms, gml_learn / gml_learn_matrix from x = 0 1.2-1.7 ms, gml_hessvec_batch_prec f64 0.8-1.1 ms,
gml_objgrad_batch f64 0.4-0.6 ms, gml_learn_warm / gml_learn_structured from the solution 0.29-0.34 ms, gml_stderr 0.26-0.35 ms,
the int8 operator calls 0.21-0.25 ms, the structure builders 0.04 ms, gml_matrix_symmetrize and gml_terms_assemble 0.02 ms.  The
longest is 1.7 ms; the delay of property A is DELAY_S = 0.1 s (torch.cuda._sleep, calibrated to 1.2 DELAY_S), sixty times that and
ample for the host-side preamble of any call.  Property B at size: the handle calls at K = 2^23 and gml_matrix_symmetrize at
n = 22528 -- between two events on the default stream around the synchronised call:
gml_objgrad_batch 3.6 ms (i8w), 3.5 ms (i8x), 14.2 ms (f64), gml_learn 29 ms, gml_matrix_symmetrize 2.15 ms.  (At K = 2^22 the int8 operator
calls took 1.8-2.0 ms and at n = 16384 the symmetrisation 1.2 ms: below the 2 ms asked for.)"""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import _structure_reference as SR
import gml_amd as gml
from oracle import oracle as O

pytestmark = pytest.mark.gpu
synthetic = __import__("importlib").import_module("gml_amd.synthetic")
_lib = gml._lib
EXCLUDED, FREE, PENALISED = gml.EXCLUDED, gml.FREE, gml.PENALISED
RISE = 0
DELAY_S = 0.1
K_LARGE, N_LARGE = 1 << 23, 22528
C_REG = 0.4
NAN_BITS = 0x7FF8000000000000   # the padding of double inputs
SENT = 0x7FF4DEADBEEF0123       # around and inside every output before the call (a signalling NaN no kernel produces)
SENT2 = 0x7FF4FEEDFACE0456      # what a pending fill of the caller's leaves in an output
TAIL = 5                        # elements behind the last row of every allocation
HANDLES = ["pair", "shard", "o3"]


# ---- the library ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def L():
    lib = _lib.lib()
    lib.gml_test_stream_idle.argtypes = [C.c_void_p]
    lib.gml_test_stream_idle.restype = C.c_int
    return lib


def opts(prec, tol=1e-9):
    o = _lib.Opts()
    L().gml_default_opts(C.byref(o))
    o.tol, o.precision = tol, _lib.PRECISIONS[prec]
    return o


def last_error():
    return L().gml_last_error().decode()


# ---- data, handles, solved rows (made once) ---------------------------------------------------------------------------------------------
class Ctx:
    def __init__(self, handles=None):
        """handles: {name: Problem} of the caller's (not closed here); None: the three small handles of the module"""
        rng = np.random.default_rng(11)
        spins, self.J = synthetic.block_ising(40, 3000, block=8, seed=5)
        self.memo, self.own = {}, handles is None
        if handles is not None:
            self.h = handles
            return
        counts = rng.integers(0, 4, size=3000).astype(np.float64)
        spins3, _ = synthetic.block_multibody(12, 2000, block=12, seed=3)
        counts3 = rng.integers(0, 4, size=2000).astype(np.float64)
        self.h = {"pair": _lib.Problem(counts=counts, spins=spins, node_range=(0, 40)),
                  "shard": _lib.Problem(counts=counts, spins=spins, node_range=(7, 19)),
                  "o3": _lib.Problem(counts=counts3, spins=spins3, order=3)}
        assert self.h["o3"].P == 67

    def close(self):
        for p in self.h.values() if self.own else ():
            p.close()

    def rows(self, name):
        p = self.h[name]
        return p.node1 - p.node0

    def structure(self, name, seed):
        """a structure with values in {0, 1, 2}: the field free, every other slot penalised or excluded by a coin"""
        p = self.h[name]
        R = self.rows(name)
        rng = np.random.default_rng(seed)
        S = np.where(rng.random((R, p.P)) < 0.5, PENALISED, EXCLUDED).astype(np.uint8)
        for r in range(R):
            S[r, (p.node0 + r) if p.order == 2 else 0] = FREE
        return S

    def solved(self, name, prec, c=C_REG, sseed=None):
        """the rows gml_learn_structured leaves at tol 1e-9 from x = 0 (host pointers); sseed: under self.structure(name, sseed)"""
        key = (name, prec, c, sseed)
        if key not in self.memo:
            p = self.h[name]
            S = None if sseed is None else self.structure(name, sseed)
            out = np.zeros((self.rows(name), p.P))
            _lib.check(L().gml_learn_structured(p._h, RISE, c, C.byref(opts(prec)), None if S is None else S.ctypes.data, p.P, None,
                                                out.ctypes.data, None, None))
            assert np.count_nonzero(out) > 2 * out.shape[0]  # (couplings survive the penalty: the solves have something to say)
            self.memo[key] = out
        return self.memo[key]


@pytest.fixture(scope="module")
def ctx():
    c = Ctx()
    yield c
    c.close()


# ---- the caller's arrays ----------------------------------------------------------------------------------------------------------------
class Arr:
    """One array argument: `shape` = (rows, row length); kind "rows" (doubles with the call's ld), "flat" (doubles, contiguous: the
    header gives them no leading dimension) or "struct" (bytes with the call's ld_s); true / decoy: the data of an input."""

    def __init__(self, shape, kind, true=None, decoy=None):
        self.shape, self.kind, self.true, self.decoy = tuple(int(v) for v in shape), kind, true, decoy
        self.dtype = np.uint8 if kind == "struct" else np.float64
        self.bits = np.uint8 if kind == "struct" else np.uint64

    def geom(self, stress, lead_s=1):
        """(ld, elements in front of the data)"""
        P = self.shape[1]
        if not stress:
            return P, 0
        return {"rows": (P + 3, 1), "flat": (P, 1), "struct": (P + 5, lead_s)}[self.kind]

    def image(self, data, pad, stress, lead_s=1):
        """the whole allocation as bit patterns: `pad` everywhere but the data (data None: everywhere)"""
        R, P = self.shape
        ld, lead = self.geom(stress, lead_s)
        flat = np.full(lead + R * ld + TAIL, pad & (0xFF if self.kind == "struct" else 0xFFFFFFFFFFFFFFFF), dtype=self.bits)
        if data is not None:
            flat[lead:lead + R * ld].reshape(R, ld)[:, :P] = np.ascontiguousarray(data, dtype=self.dtype).reshape(R, P).view(self.bits)
        return flat

    def split(self, flat, stress, lead_s=1):
        """(the data as bit patterns [R, P], everything else)"""
        R, P = self.shape
        ld, lead = self.geom(stress, lead_s)
        mask = np.ones(len(flat), dtype=bool)
        inner = mask[lead:lead + R * ld].reshape(R, ld)
        inner[:, :P] = False
        return flat[lead:lead + R * ld].reshape(R, ld)[:, :P].copy(), flat[mask]

    def address(self, base, stress, lead_s=1):
        return int(base) + self.geom(stress, lead_s)[1] * np.dtype(self.bits).itemsize


def _torch_view(flat):
    return flat.view(np.int64) if flat.dtype == np.uint64 else flat


def place(flat, where):
    """(holder, base address) of the bit image in pageable host memory, pinned host memory or HBM (a synchronous upload)"""
    import torch
    if where == "host":
        return flat, flat.ctypes.data
    t = torch.from_numpy(_torch_view(flat))
    t = t.pin_memory() if where == "pin" else t.cuda()
    return t, t.data_ptr()


def fill_dev(n, bits, pattern):
    """n elements of HBM filled with `pattern` by a kernel on the default stream (asynchronous: no host copy)"""
    import torch
    if bits == np.uint8:
        return torch.full((n,), pattern & 0xFF, dtype=torch.uint8, device="cuda")
    return torch.full((n,), pattern - (1 << 64) if pattern >> 63 else pattern, dtype=torch.int64, device="cuda")


def read_fresh(t):
    """a device tensor read on a stream of its own -- non-blocking: it waits for neither the handle's stream nor the null stream"""
    import torch
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        h = torch.empty(t.shape, dtype=t.dtype, pin_memory=True)
        h.copy_(t, non_blocking=True)
    s.synchronize()
    return h.numpy().copy()


def fetch(holder, where, bits):
    if where == "host":
        return holder
    a = read_fresh(holder) if where == "dev" else holder.numpy().copy()
    return a.view(np.uint64) if bits == np.uint64 else a


# ---- the calls ----------------------------------------------------------------------------------------------------------------------------
class Call:
    """One entry point at one shape: device-capable inputs and outputs as Arr, and invoke(addresses, ld, ld_s) -> status."""
    handle = None  # name of the handle in Ctx.h; None: a handle-less call on the null stream
    exact = True   # results are the same bits whichever way the arrays travel

    def __init__(self, ctx):
        self.ctx, self.ins, self.outs, self.host = ctx, {}, {}, {}

    @property
    def p(self):
        return self.ctx.h[self.handle]

    def lds(self, stress):
        rows = [a for a in list(self.ins.values()) + list(self.outs.values()) if a.kind == "rows"]
        st = [a for a in list(self.ins.values()) + list(self.outs.values()) if a.kind == "struct"]
        return (rows[0].geom(stress)[0] if rows else 0), (st[0].geom(stress)[0] if st else 0)

    def idle(self):
        import torch
        return L().gml_test_stream_idle(self.p._h) == 1 if self.handle else bool(torch.cuda.default_stream().query())


def operator_inputs(ctx, name, seed):
    """37 nodes, permuted with repeats (one full 32-row tile and a partial one), theta and a direction for them"""
    p = ctx.h[name]
    rng = np.random.default_rng(seed)
    base = rng.permutation(p.n)
    nodes = np.concatenate([np.tile(base, 3)[:30], rng.choice(base, size=7)]).astype(np.int64)
    assert len(nodes) == 37
    if p.order == 2:
        theta = ctx.J[nodes] + rng.normal(scale=0.05, size=(37, p.P)) * (rng.random((37, p.P)) < 0.2)
    else:
        theta = rng.normal(scale=0.05, size=(37, p.P))
    return nodes, theta, rng.normal(size=(37, p.P))


class ObjGrad(Call):
    def __init__(self, ctx, name, prec, want_g=True):
        super().__init__(ctx)
        self.handle, self.prec, self.exact = name, prec, prec != "f64"
        self.nodes, theta, _ = operator_inputs(ctx, name, 1)
        _, decoy, _ = operator_inputs(ctx, name, 2)
        P = self.p.P
        self.ins["theta"] = Arr((37, P), "rows", theta, decoy)
        self.outs["f"] = Arr((1, 37), "flat")
        if want_g:
            self.outs["g"] = Arr((37, P), "rows")

    def invoke(self, a, ld, ld_s):
        return L().gml_objgrad_batch(self.p._h, RISE, _lib.PRECISIONS[self.prec], 37, self.nodes.ctypes.data, a["theta"], ld, a["f"], a.get("g"))


class HessVec(Call):
    def __init__(self, ctx, name, prec):
        super().__init__(ctx)
        self.handle, self.prec, self.exact = name, prec, prec != "f64"
        self.nodes, theta, vec = operator_inputs(ctx, name, 1)
        _, dtheta, dvec = operator_inputs(ctx, name, 2)
        P = self.p.P
        self.ins["theta"] = Arr((37, P), "rows", theta, dtheta)
        self.ins["vec"] = Arr((37, P), "rows", vec, dvec)
        self.outs["hv"] = Arr((37, P), "rows")

    def invoke(self, a, ld, ld_s):
        return L().gml_hessvec_batch_prec(self.p._h, RISE, _lib.PRECISIONS[self.prec], 37, self.nodes.ctypes.data, a["theta"], a["vec"], ld, a["hv"])


class Learn(Call):
    """gml_learn / gml_learn_warm / gml_learn_structured.  warm: x0 = the solution at tol 1e-9 and the call asks for 1e-8, so the true
    input is complete at once and `out` is x0's bits; the decoy is other solved rows (those of c = 1.0), from which the solver has to
    iterate.  structured: under a structure of its own, x0 the solution under it; the decoys are another structure with values in
    {0, 1, 2} and the rows solved without any."""

    def __init__(self, ctx, name, prec, warm=False, structured=False):
        super().__init__(ctx)
        self.handle, self.prec, self.tol = name, prec, 1e-8 if (warm or structured) else 1e-9
        R, P = ctx.rows(name), self.p.P
        if structured:
            self.ins["structure"] = Arr((R, P), "struct", ctx.structure(name, 5), ctx.structure(name, 6))
            self.ins["x0"] = Arr((R, P), "flat", ctx.solved(name, prec, sseed=5), ctx.solved(name, prec))
        elif warm:
            self.ins["x0"] = Arr((R, P), "flat", ctx.solved(name, prec), ctx.solved(name, prec, c=1.0))
        self.outs["out"] = Arr((R, P), "flat")

    def invoke(self, a, ld, ld_s):
        R = self.ctx.rows(self.handle)
        kkt = np.full(R + 2, -7.0)
        st = _lib.Stats()
        rc = L().gml_learn_structured(self.p._h, RISE, C_REG, C.byref(opts(self.prec, self.tol)), a.get("structure"), ld_s, a.get("x0"), a["out"],
                                      kkt.ctypes.data, C.byref(st))
        assert (kkt[R:] == -7.0).all() and (rc != 0 or (kkt[:R] <= self.tol).all())  # kkt: R values, nothing behind them
        self.host = {"iterations": st.iterations}
        return rc


class LearnMatrix(Call):
    def __init__(self, ctx, prec, sym):
        super().__init__(ctx)
        self.handle, self.prec, self.sym = "pair", prec, sym
        self.outs["out"] = Arr((40, 40), "flat")

    def invoke(self, a, ld, ld_s):
        return L().gml_learn_matrix(self.p._h, RISE, C_REG, self.sym, C.byref(opts(self.prec)), a["out"], None, None)


class LearnTerms(Call):
    def __init__(self, ctx, prec, sym):
        super().__init__(ctx)
        self.handle, self.prec, self.sym = "o3", prec, sym
        self.outs["terms"] = Arr((1, _lib.terms_count(12, 3, sym)), "flat")

    def invoke(self, a, ld, ld_s):
        return L().gml_learn_terms(self.p._h, RISE, C_REG, self.sym, C.byref(opts(self.prec)), a["terms"], None, None)


class StdErr(Call):
    """x: the rows solved under a structure (exactly 0.0 where it excludes); the decoys are half of them (the same support, so no
    excluded slot becomes non-zero) and the structure with every slot free (another support)."""

    def __init__(self, ctx, name):
        super().__init__(ctx)
        self.handle = name
        R, P = ctx.rows(name), self.p.P
        x = ctx.solved(name, "i8w", sseed=5)
        self.ins["x"] = Arr((R, P), "rows", x, 0.5 * x)
        self.ins["structure"] = Arr((R, P), "struct", ctx.structure(name, 5), np.full((R, P), FREE, dtype=np.uint8))
        self.outs["se"] = Arr((R, P), "rows")

    def invoke(self, a, ld, ld_s):
        R = self.ctx.rows(self.handle)
        status = np.full(R + 1, -3, dtype=np.int32)
        rc = L().gml_stderr(self.p._h, RISE, a["x"], ld, a.get("structure"), ld_s, a["se"], status.ctypes.data, None)
        assert status[R] == -3
        self.host = {"status": status[:R].tolist()}
        return rc


def rows_per_node(n, order):
    return n if order == 2 else sum(math.comb(n - 1, s - 1) for s in range(1, order + 1))


def model_rows(n, order, seed):
    return np.random.default_rng(seed).normal(size=(n, rows_per_node(n, order)))


def dict_assembly(rows, n, order, sym):
    """the reference's dict assembly (tests/test_gpu_terms.py)"""
    keys = [[(u,) if i == u else (u, i) for i in range(n)] if order == 2 else O.multi_keys(n, order, u) for u in range(n)]
    rec = O.assemble_multi_dict(rows, keys, sym)
    return np.array([rec[k] for k in O.listing_order(rec)])


class TermsAssemble(Call):
    def __init__(self, ctx, n, order, sym):
        super().__init__(ctx)
        self.n, self.order, self.sym = n, order, sym
        self.ins["rows"] = Arr((n, rows_per_node(n, order)), "rows", model_rows(n, order, 1), model_rows(n, order, 2))
        self.outs["out"] = Arr((1, _lib.terms_count(n, order, sym)), "flat")

    def invoke(self, a, ld, ld_s):
        return L().gml_terms_assemble(a["rows"], ld, self.n, self.order, self.sym, 0, a["out"])

    def model(self):
        return dict_assembly(self.ins["rows"].true, self.n, self.order, self.sym)[None, :]


class Symmetrize(Call):
    def __init__(self, ctx, n=70):
        super().__init__(ctx)
        self.n = n
        self.ins["rows"] = Arr((n, n), "rows", model_rows(n, 2, 3), model_rows(n, 2, 4))
        self.outs["out"] = Arr((n, n), "flat")

    def invoke(self, a, ld, ld_s):
        return L().gml_matrix_symmetrize(a["rows"], ld, self.n, 0, a["out"])

    def model(self):
        R = self.ins["rows"].true
        return 0.5 * (R + R.T)


class StructureFromRows(Call):
    def __init__(self, ctx, n, order, rule):
        super().__init__(ctx)
        self.n, self.order, self.rule = n, order, rule
        P = rows_per_node(n, order)
        self.ins["rows"] = Arr((n, P), "rows", model_rows(n, order, 5), model_rows(n, order, 6))
        self.outs["structure"] = Arr((n, P), "struct")
        self.thr = float(np.median(np.abs(self.ins["rows"].true)))

    def invoke(self, a, ld, ld_s):
        kept = C.c_int64(-1)
        rc = L().gml_structure_from_rows(a["rows"], ld, self.n, self.order, _lib.RULES[self.rule], self.thr, PENALISED, EXCLUDED, FREE, 0,
                                         a["structure"], ld_s, C.byref(kept))
        self.host = {"kept": kept.value}
        return rc

    def model(self):
        return SR.structure_from_rows(self.ins["rows"].true, self.n, self.order, self.thr, self.rule, PENALISED, EXCLUDED, FREE)[0]


class StructureFromKeys(Call):
    def __init__(self, ctx, n, order):
        super().__init__(ctx)
        self.n, self.order = n, order
        rng = np.random.default_rng(100 + order)
        self.keys0 = [tuple(int(v) for v in rng.choice(n, size=int(rng.integers(1, order + 1)), replace=False)) for _ in range(60)] + [(3,), (n - 1,)]
        self.karr = np.full((len(self.keys0), order + 1), -1, dtype=np.int32)
        for t, k in enumerate(self.keys0):
            self.karr[t, 1:1 + len(k)] = k
        self.outs["structure"] = Arr((n, rows_per_node(n, order)), "struct")

    def invoke(self, a, ld, ld_s):
        return L().gml_structure_from_keys(self.karr.ctypes.data, self.order + 1, len(self.karr), self.n, self.order, PENALISED, EXCLUDED, FREE, 0,
                                           a["structure"], ld_s)

    def model(self):
        return SR.structure_from_keys(self.keys0, self.n, self.order, PENALISED, EXCLUDED, FREE)


# ---- one run of a call ----------------------------------------------------------------------------------------------------------------------
class Result:
    def __init__(self, call, stress, lead_s, flats, host):
        self.call, self.stress, self.lead_s, self.flats, self.host = call, stress, lead_s, flats, host

    def data(self, name):
        arr = self.call.outs[name]
        return arr.split(self.flats[name], self.stress, self.lead_s)[0].view(arr.dtype)

    def bits(self, name):
        return self.call.outs[name].split(self.flats[name], self.stress, self.lead_s)[0]

    def outside(self, name):
        return self.call.outs[name].split(self.flats[name], self.stress, self.lead_s)[1]


def run(call, where="dev", stress=True, lead_s=1, use=None, placed=None, outputs=None, sentinel=SENT, expect=0, pending=None):
    """The call with every array in `where` ("dev", "host", "pin", or a dict by argument name; missing names: "host").  Inputs: the true
    data (use = {name: data} replaces some) inside NaN / 0xFF padding, or what `placed` = {name: (holder, base address)} holds
    already.  Outputs: full of `sentinel` (device ones are filled by a kernel on the default stream: nothing here waits for the
    device), or the device tensors of `outputs`.  pending: an event of the caller's that must not have completed when the call is made.
    After the call: the expected status, the stream idle, every output read back --
    device ones on a fresh non-blocking stream."""
    kind = (lambda name: where.get(name, "host")) if isinstance(where, dict) else (lambda name: where)
    addr, held = {}, {}
    for name, arr in call.ins.items():
        if placed and name in placed:
            holder, base = placed[name]
        else:
            data = use[name] if use and name in use else arr.true
            holder, base = place(arr.image(data, 0xFF if arr.kind == "struct" else NAN_BITS, stress, lead_s), kind(name))
        held[name] = holder
        addr[name] = arr.address(base, stress, lead_s)
    outs = {}
    for name, arr in call.outs.items():
        if outputs and name in outputs:
            holder = outputs[name]
            base = holder.data_ptr()
        elif kind(name) == "dev":
            holder = fill_dev(len(arr.image(None, 0, stress, lead_s)), arr.bits, sentinel)
            base = holder.data_ptr()
        else:
            holder, base = place(arr.image(None, sentinel, stress, lead_s), kind(name))
        outs[name] = holder
        addr[name] = arr.address(base, stress, lead_s)
    ld, ld_s = call.lds(stress)
    assert pending is None or not pending.query(), "inconclusive: the caller's delayed work had drained before the call was made"
    rc = call.invoke(addr, ld, ld_s)
    idle = call.idle()  # (asked before anything else touches the device)
    assert rc == expect, (rc, last_error())
    assert idle, "the call returned with work pending on its stream"
    flats = {name: fetch(outs[name], "dev" if (outputs and name in outputs) else kind(name), call.outs[name].bits) for name in call.outs}
    return Result(call, stress, lead_s, flats, dict(call.host))


def assert_same(got, ref, sentinel=SENT):
    """the outputs of two runs of one call: the same data, and nothing written outside the data by either (got's surroundings were
    `sentinel`).  The data are the same bits, but for the FP64 operator calls, whose sums are added with floating-point atomics: they
    are held to the bounds of tests/test_gpu_operator_export.py -- f to 1e-13 relative, g to 1e-13 -- and hv, whose entries are sums
    of the same length over terms of size |hv|, to 1e-13 of the largest entry"""
    call = got.call
    for name, arr in call.outs.items():
        mask = 0xFF if arr.kind == "struct" else 0xFFFFFFFFFFFFFFFF
        assert (got.outside(name) == (sentinel & mask)).all(), f"{name}: written outside the data"
        assert (ref.outside(name) == (SENT & mask)).all(), f"{name}: the reference call wrote outside the data"
        if call.exact:
            assert np.array_equal(got.bits(name), ref.bits(name)), f"{name} differs"
            continue
        a, b = got.data(name), ref.data(name)
        assert np.isfinite(a).all() and np.isfinite(b).all()
        err = np.abs(a / b - 1).max() if name == "f" else np.abs(a - b).max() / (max(1.0, np.abs(b).max()) if name == "hv" else 1.0)
        assert err <= 1e-13, (name, err)
    assert got.host == ref.host


def differs(a, b):
    return any(not np.array_equal(a.bits(n), b.bits(n)) for n in a.call.outs) or a.host != b.host


# ---- the caller's pending work ------------------------------------------------------------------------------------------------------------
_delay = []


def enqueue_delay():
    """at least DELAY_S of work on the default stream: torch.cuda._sleep, calibrated once with two events; a chain of FP64 matrix
    products sized the same way if _sleep does not spin on this build"""
    import torch
    if not _delay:
        def timed(fn):
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1) * 1e-3
        cycles = 20_000_000
        t = timed(lambda: torch.cuda._sleep(cycles)) if hasattr(torch.cuda, "_sleep") else 0.0
        if t >= 1e-3:
            n = int(cycles * 1.2 * DELAY_S / t)
            _delay.append(lambda: torch.cuda._sleep(n))
        else:
            a = torch.rand((4096, 4096), dtype=torch.float64, device="cuda")
            b = torch.empty_like(a)
            timed(lambda: torch.mm(a, a, out=b))
            per = timed(lambda: [torch.mm(a, a, out=b) for _ in range(8)]) / 8
            reps = int(math.ceil(1.2 * DELAY_S / per))
            _delay.append(lambda: [torch.mm(a, a, out=b) for _ in range(reps)])
        print(f"delay: {'_sleep' if t >= 1e-3 else 'FP64 products'} for {timed(_delay[0]):.3f} s")
    _delay[0]()


def pending_event():
    """an event behind what was just queued on the default stream; the test is inconclusive -- and fails -- unless it is still pending"""
    import torch
    ev = torch.cuda.Event()
    ev.record()
    assert not ev.query(), "inconclusive: the caller's delayed work had drained before the call was made"
    return ev


def check_ordered_after_input(call, which):
    """property A for the device input `which` of `call`"""
    import torch
    assert torch.cuda.default_stream().cuda_stream == 0, "the contract names the null stream as torch's default stream"
    arr = call.ins[which]
    ref = run(call)                                   # the true input, after a full synchronise
    dec = run(call, use={which: arr.decoy})
    assert differs(dec, ref), "the decoy gives the same result: it could not be told apart"
    pad = lambda a: 0xFF if a.kind == "struct" else NAN_BITS
    # every input is in HBM before the delay starts (an upload from pageable memory would wait for the device)
    placed = {k: place(a.image(a.decoy if k == which else a.true, pad(a), True), "dev") for k, a in call.ins.items()}
    true_d, _ = place(arr.image(arr.true, pad(arr), True), "dev")
    torch.cuda.synchronize()
    enqueue_delay()
    placed[which][0].copy_(true_d, non_blocking=True)
    ev = pending_event()
    got = run(call, placed=placed, pending=ev)         # no synchronisation between the event and the call
    assert ev.query()
    assert_same(got, ref)
    assert differs(got, dec)


def check_ordered_after_output_fill(call):
    """property A for a call without device inputs: a pending fill of its outputs comes first, the results land on top of it"""
    import torch
    assert torch.cuda.default_stream().cuda_stream == 0, "the contract names the null stream as torch's default stream"
    ref = run(call)
    outputs = {name: fill_dev(len(arr.image(None, 0, True)), arr.bits, SENT) for name, arr in call.outs.items()}
    torch.cuda.synchronize()
    enqueue_delay()
    for name, arr in call.outs.items():
        outputs[name].fill_(SENT2 & 0xFF if arr.kind == "struct" else SENT2)
    ev = pending_event()
    got = run(call, outputs=outputs, pending=ev)
    assert ev.query()
    assert_same(got, ref, sentinel=SENT2)


# ---- A: ordered after the caller's null-stream work ---------------------------------------------------------------------------------------
OP_CASES = [(h, prec) for h in ("pair", "o3") for prec in ("i8w", "i8x", "f64")]
HV_CASES = [(h, prec) for h in ("pair", "o3") for prec in ("i8x", "f64")]
LEARN_CASES = [(h, prec) for h in HANDLES for prec in ("i8w", "i8x")]


@pytest.mark.parametrize("name,prec", OP_CASES)
def test_objgrad_waits_for_the_pending_theta(ctx, name, prec):
    check_ordered_after_input(ObjGrad(ctx, name, prec), "theta")


def test_objgrad_without_a_gradient_waits_for_the_pending_theta(ctx):
    check_ordered_after_input(ObjGrad(ctx, "pair", "i8w", want_g=False), "theta")


@pytest.mark.parametrize("which", ["theta", "vec"])
@pytest.mark.parametrize("name,prec", HV_CASES)
def test_hessvec_waits_for_the_pending_input(ctx, name, prec, which):
    check_ordered_after_input(HessVec(ctx, name, prec), which)


@pytest.mark.parametrize("name,prec", LEARN_CASES)
def test_learn_writes_after_a_pending_fill_of_out(ctx, name, prec):
    check_ordered_after_output_fill(Learn(ctx, name, prec))


@pytest.mark.parametrize("name,prec", LEARN_CASES)
def test_learn_warm_waits_for_the_pending_x0(ctx, name, prec):
    call = Learn(ctx, name, prec, warm=True)
    check_ordered_after_input(call, "x0")
    assert call.host["iterations"] == 0  # (the true x0 is the solution: what was read is what came back)


@pytest.mark.parametrize("which", ["structure", "x0"])
@pytest.mark.parametrize("name,prec", LEARN_CASES)
def test_learn_structured_waits_for_the_pending_input(ctx, name, prec, which):
    check_ordered_after_input(Learn(ctx, name, prec, structured=True), which)


@pytest.mark.parametrize("sym", [0, 1])
@pytest.mark.parametrize("prec", ["i8w", "i8x"])
def test_learn_matrix_writes_after_a_pending_fill_of_out(ctx, prec, sym):
    check_ordered_after_output_fill(LearnMatrix(ctx, prec, sym))


@pytest.mark.parametrize("sym", [0, 1])
@pytest.mark.parametrize("prec", ["i8w", "i8x"])
def test_learn_terms_writes_after_a_pending_fill_of_terms(ctx, prec, sym):
    check_ordered_after_output_fill(LearnTerms(ctx, prec, sym))


@pytest.mark.parametrize("which", ["x", "structure"])
@pytest.mark.parametrize("name", HANDLES)
def test_stderr_waits_for_the_pending_input(ctx, name, which):
    check_ordered_after_input(StdErr(ctx, name), which)


@pytest.mark.parametrize("sym", [0, 1])
def test_terms_assemble_waits_for_the_pending_rows(ctx, sym):
    check_ordered_after_input(TermsAssemble(ctx, 12, 3, sym), "rows")


def test_matrix_symmetrize_waits_for_the_pending_rows(ctx):
    check_ordered_after_input(Symmetrize(ctx), "rows")


def test_matrix_symmetrize_in_place_waits_for_the_pending_rows(ctx):
    import torch
    call = Symmetrize(ctx)
    arr, n = call.ins["rows"], call.n
    ld, lead = arr.geom(True)
    holder, base = place(arr.image(arr.decoy, NAN_BITS, True), "dev")
    true_d, _ = place(arr.image(arr.true, NAN_BITS, True), "dev")
    torch.cuda.synchronize()
    enqueue_delay()
    holder.copy_(true_d, non_blocking=True)
    ev = pending_event()
    a = arr.address(base, True)
    rc = L().gml_matrix_symmetrize(a, ld, n, 0, a)
    idle = call.idle()
    assert rc == 0 and idle and ev.query(), last_error()
    got = fetch(holder, "dev", np.uint64)[lead:lead + n * n].view(np.float64).reshape(n, n)
    assert np.array_equal(got, call.model())
    D = arr.decoy
    assert not np.array_equal(got, 0.5 * (D + D.T))


@pytest.mark.parametrize("n,order,rule", [(40, 2, "mean"), (12, 3, "row"), (12, 3, "any")])
def test_structure_from_rows_waits_for_the_pending_rows(ctx, n, order, rule):
    check_ordered_after_input(StructureFromRows(ctx, n, order, rule), "rows")


def test_structure_from_keys_writes_after_a_pending_fill(ctx):
    check_ordered_after_output_fill(StructureFromKeys(ctx, 12, 3))


# ---- C: the caller's memory layout (B in every run) -----------------------------------------------------------------------------------------
def check_layout(call, lead_s=1):
    """device arrays -- padded, interior, NaN / 0xFF around the inputs, a sentinel around the outputs -- against the host-pointer call
    on tight arrays and on padded ones"""
    dev = run(call, "dev", stress=True, lead_s=lead_s)
    tight = run(call, "host", stress=False)
    padded = run(call, "host", stress=True, lead_s=lead_s)
    assert_same(dev, tight)
    assert_same(padded, tight)
    return dev


@pytest.mark.parametrize("name,prec", OP_CASES)
def test_objgrad_layout(ctx, name, prec):
    check_layout(ObjGrad(ctx, name, prec))
    check_layout(ObjGrad(ctx, name, prec, want_g=False))  # g NULL: f alone, and nothing but f's 37 values is written


@pytest.mark.parametrize("name,prec", HV_CASES)
def test_hessvec_layout(ctx, name, prec):
    check_layout(HessVec(ctx, name, prec))


@pytest.mark.parametrize("name,prec", LEARN_CASES)
def test_learn_layout(ctx, name, prec):
    dev = check_layout(Learn(ctx, name, prec))
    assert np.array_equal(dev.data("out"), ctx.solved(name, prec))


@pytest.mark.parametrize("name,prec", LEARN_CASES)
def test_learn_warm_layout(ctx, name, prec):
    call = Learn(ctx, name, prec, warm=True)
    dev = check_layout(call)
    assert np.array_equal(dev.data("out"), call.ins["x0"].true)
    far = run(call, "dev", use={"x0": call.ins["x0"].decoy})  # from other solved rows: device and host pointers walk the same path
    assert_same(far, run(call, "host", stress=False, use={"x0": call.ins["x0"].decoy}))
    assert far.host["iterations"] > 0


@pytest.mark.parametrize("lead_s", [1, 3, 7])
@pytest.mark.parametrize("name,prec", LEARN_CASES)
def test_learn_structured_layout(ctx, name, prec, lead_s):
    call = Learn(ctx, name, prec, structured=True)
    dev = check_layout(call, lead_s)
    out, S = dev.data("out"), call.ins["structure"].true
    assert (out[S == EXCLUDED] == 0.0).all() and not np.signbit(out[S == EXCLUDED]).any()
    far = run(call, "dev", lead_s=lead_s, use={"x0": call.ins["x0"].decoy})
    assert_same(far, run(call, "host", stress=False, use={"x0": call.ins["x0"].decoy}))


@pytest.mark.parametrize("start", ["far", "solution"])
@pytest.mark.parametrize("structured", [False, True])
@pytest.mark.parametrize("name,prec", LEARN_CASES)
def test_learn_in_place_on_the_device(ctx, name, prec, structured, start):
    """out == x0, both the same interior device pointer: the result of the call with two arrays"""
    call = Learn(ctx, name, prec, warm=not structured, structured=structured)
    arr = call.ins["x0"]
    x0 = arr.true if start == "solution" else arr.decoy
    ref = run(call, "host", stress=False, use={"x0": x0})
    holder, base = place(arr.image(x0, SENT, True), "dev")
    got = run(call, "dev", placed={"x0": (holder, base)}, outputs={"out": holder})
    assert_same(got, ref)


@pytest.mark.parametrize("sym", [0, 1])
@pytest.mark.parametrize("prec", ["i8w", "i8x"])
def test_learn_matrix_layout(ctx, prec, sym):
    dev = check_layout(LearnMatrix(ctx, prec, sym))
    rows = ctx.solved("pair", prec)
    assert np.array_equal(dev.data("out"), 0.5 * (rows + rows.T) if sym else rows)


@pytest.mark.parametrize("sym", [0, 1])
@pytest.mark.parametrize("prec", ["i8w", "i8x"])
def test_learn_terms_layout(ctx, prec, sym):
    dev = check_layout(LearnTerms(ctx, prec, sym))
    assert np.array_equal(dev.data("terms")[0], dict_assembly(ctx.solved("o3", prec), 12, 3, sym))


@pytest.mark.parametrize("lead_s", [1, 3, 7])
@pytest.mark.parametrize("name", HANDLES)
def test_stderr_layout(ctx, name, lead_s):
    dev = check_layout(StdErr(ctx, name), lead_s)
    assert dev.host["status"] == [0] * ctx.rows(name)


@pytest.mark.parametrize("n,order", [(12, 3), (40, 2)])
@pytest.mark.parametrize("sym", [0, 1])
def test_terms_assemble_layout(ctx, n, order, sym):
    call = TermsAssemble(ctx, n, order, sym)
    assert np.array_equal(check_layout(call).data("out"), call.model())


def test_matrix_symmetrize_layout(ctx):
    call = Symmetrize(ctx)
    assert np.array_equal(check_layout(call).data("out"), call.model())  # (the source with ld = n + 3)
    assert np.array_equal(run(call, {"rows": "dev"}).data("out"), call.model())  # device rows, host out: through a staging block
    assert np.array_equal(run(call, {"out": "dev"}).data("out"), call.model())


@pytest.mark.parametrize("stress", [False, True])
def test_matrix_symmetrize_in_place(ctx, stress):
    """out == rows on the device; with ld > n the result is the packed n x n matrix at the same address"""
    call = Symmetrize(ctx)
    arr, n = call.ins["rows"], call.n
    ld, lead = arr.geom(stress)
    flat = arr.image(arr.true, NAN_BITS, stress)
    holder, base = place(flat, "dev")
    a = arr.address(base, stress)
    rc = L().gml_matrix_symmetrize(a, ld, n, 0, a)
    idle = call.idle()
    assert rc == 0 and idle, last_error()
    got = fetch(holder, "dev", np.uint64)
    assert np.array_equal(got[lead:lead + n * n].view(np.float64).reshape(n, n), call.model())
    assert np.array_equal(got[:lead], flat[:lead]) and np.array_equal(got[lead + n * n:], flat[lead + n * n:])


@pytest.mark.parametrize("lead_s", [1, 3, 7])
@pytest.mark.parametrize("n,order,rule", [(40, 2, "mean"), (12, 3, "row"), (12, 3, "mean"), (12, 3, "all")])
def test_structure_from_rows_layout(ctx, n, order, rule, lead_s):
    call = StructureFromRows(ctx, n, order, rule)
    dev = check_layout(call, lead_s)
    want = call.model()
    assert np.array_equal(dev.data("structure"), want)
    assert dev.host["kept"] == int((want == PENALISED).sum())


@pytest.mark.parametrize("lead_s", [1, 3, 7])
@pytest.mark.parametrize("n,order", [(12, 3), (40, 2)])
def test_structure_from_keys_layout(ctx, n, order, lead_s):
    call = StructureFromKeys(ctx, n, order)
    assert np.array_equal(check_layout(call, lead_s).data("structure"), call.model())


# ---- B at a size where the work behind the last host wait can be seen --------------------------------------------------------------------------
@pytest.fixture(scope="module")
def large():
    J = synthetic.block_ising_model(40, block=8, seed=5)
    with _lib.Problem(model=J, num_samples=K_LARGE, seed=9) as p:
        yield p


def test_objgrad_is_complete_at_return_at_size(large):
    c = Ctx({"pair": large})
    for prec in ("i8w", "i8x", "f64"):
        call = ObjGrad(c, "pair", prec)
        assert_same(run(call, "dev"), run(call, "host", stress=False))


def test_learn_is_complete_at_return_at_size(large):
    c = Ctx({"pair": large})
    call = Learn(c, "pair", "i8w")
    assert_same(run(call, "dev"), run(call, "host", stress=False))


def test_matrix_symmetrize_is_complete_at_return_at_size():
    """two device arrays, not in place: the call owns no block whose release would wait for the device"""
    import torch
    n = N_LARGE
    R = torch.rand((n, n), dtype=torch.float64, device="cuda")
    out = torch.empty_like(R)
    want = R + R.t()          # the host expression (a + b) * 0.5, on the device: the same bits
    want.mul_(0.5)
    torch.cuda.synchronize()
    rc = L().gml_matrix_symmetrize(R.data_ptr(), n, n, 0, out.data_ptr())
    idle = bool(torch.cuda.default_stream().query())
    assert rc == 0 and idle, "the call returned with work pending on the null stream"
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        same = torch.equal(out, want)
    assert same


# ---- D: pointer kinds ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,prec", [("pair", "i8w"), ("pair", "i8x"), ("o3", "i8w")])
def test_pinned_arrays_are_host_pointers(ctx, name, prec):
    for call in (ObjGrad(ctx, name, prec), Learn(ctx, name, prec, warm=True), StdErr(ctx, name)):
        assert_same(run(call, "pin"), run(call, "host"))


@pytest.mark.parametrize("name", ["pair", "o3"])
def test_mixed_operator_pointers_are_refused_position_by_position(ctx, name):
    """one argument on the other side, each of the three in turn, both ways round: GML_EINVAL naming the arguments, nothing written,
    the stream idle, and the handle goes on giving the same bits"""
    for call, names in ((ObjGrad(ctx, name, "i8w"), "theta, f and g"), (HessVec(ctx, name, "i8x"), "theta, vec and hv")):
        before = run(call)
        for odd in list(call.ins) + list(call.outs):
            for side, other in (("dev", "host"), ("host", "dev")):
                where = {k: side for k in list(call.ins) + list(call.outs)}
                where[odd] = other
                refused = run(call, where, expect=_lib.GML_EINVAL)
                assert names in last_error() and "all host or all device" in last_error()
                for out in call.outs:
                    assert (refused.flats[out] == SENT).all()
        assert_same(run(call), before)


def test_stderr_takes_each_array_from_either_side(ctx):
    for name in ("shard", "o3"):
        call = StdErr(ctx, name)
        ref = run(call, "host", stress=False)
        for combo in range(8):
            where = {k: ("dev" if combo >> i & 1 else "host") for i, k in enumerate(("x", "structure", "se"))}
            assert_same(run(call, where, lead_s=3), ref)


def test_stderr_without_a_structure(ctx):
    call = StdErr(ctx, "shard")
    del call.ins["structure"]
    call.ins["x"] = Arr(call.ins["x"].shape, "rows", ctx.solved("shard", "i8w"))
    assert_same(run(call, "dev"), run(call, "host", stress=False))


def test_a_refused_structure_leaves_the_handle_usable(ctx):
    """a device structure with a byte outside {0, 1, 2} is found by the kernel that reads it; the next call gives the old bits"""
    for call in (Learn(ctx, "shard", "i8w", structured=True), StdErr(ctx, "shard")):
        before = run(call)
        bad = call.ins["structure"].true.copy()
        bad[3, 2] = 3
        run(call, "dev", use={"structure": bad}, expect=_lib.GML_EINVAL)
        assert "row 3, slot 2" in last_error()
        assert_same(run(call), before)
