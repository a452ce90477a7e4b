"""Per-element accuracy of the three FusedMM forms (row: fusedMM_csr_udef_hip, task: fusedMM_csr_udef_tasks_hip, stream:
fusedMM_csr_udef_stream_hip) against the fp64 reference, held to the contract of tests/fusedmm_bound.py with the
scalar stage driven over its whole range: saturated sigmoids, e^-s underflowing, exp overflowing, both branches of leaky_exp.
tests/test_fusedmm_bound_host.py shows on the CPU that the contract is neither too tight for correct fp32 code nor too loose to
reject a subtly wrong kernel.  Every run writes into a fresh NaN-filled output and is launched twice for equal bits."""
import numpy as np
import pytest
import torch

from tests import cases
from tests import fusedmm_bound as fb
from tests import fusedmm_cases as fc

pytestmark = pytest.mark.gpu

FILE_OF = {"row": "general", "task": "general", "stream": "stream"}
STREAM_PLANS = ((3, 4, 64), (1, 2, 4096))          # (slices, waves per generation, chunk): a 300-edge row cut / whole


def _t(a, gpu):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def _streams_for(k):
    return 8 if k <= 32 else (4 if k <= 64 else 2)


def _bits(z):
    return z.view(torch.int32)


class _Device:
    """One graph on the GPU with its task plan and, on demand, its stream plans."""

    def __init__(self, gpu, rowptr, col, n, val=None, task_geom=(3, 128, 16)):
        from isplib_amd.plan import build_task_plan
        self.gpu, self.rowptr, self.col, self.n = gpu, rowptr, col, n
        self.d_rowptr, self.d_col, self.d_val = _t(rowptr, gpu), _t(col, gpu), _t(val, gpu)
        self.tasks = build_task_plan(self.d_rowptr, self.d_col, n, *task_geom)
        assert self.tasks is not None
        self._streams = {}

    def stream_plan(self, streams, geom):
        from isplib_amd import cabi
        key = (streams,) + tuple(geom)
        if key not in self._streams:
            slices, wpg, chunk = geom
            self._streams[key] = cabi.NativeStreamPlan(self.d_rowptr, self.d_col, None, self.n, streams, slices, chunk, wpg, fusedmm=True)
        return self._streams[key]

    def close(self):
        for plan in self._streams.values():
            plan.close()
        self._streams = {}

    def run(self, form, word, x, y, fn, prm, geom=None):
        """-> (z, arg | None) as NumPy, from the second of two launches whose outputs agree bit for bit."""
        from isplib_amd import cabi
        m, k = self.rowptr.size - 1, y.shape[1]
        d_x, d_y = _t(x, self.gpu), _t(y, self.gpu)
        got = []
        for _ in range(2):
            out = torch.full((m, k), float("nan"), dtype=torch.float32, device=self.gpu)
            if form == "stream":
                plan = self.stream_plan(_streams_for(k), geom)
                st, z = cabi.fusedmm_stream(word, self.d_rowptr, self.col.size, plan, d_x, d_y, sop_udef=fn, sop_param=prm, out=out)
                arg = None
            else:
                st, z, arg = cabi.fusedmm(word, self.d_rowptr, self.d_col, self.d_val, d_x, d_y, sop_udef=fn, sop_param=prm,
                                          plan=self.tasks if form == "task" else None, out=out)
            assert st == 0 and z.data_ptr() == out.data_ptr()
            got.append((z, arg))
        assert torch.equal(_bits(got[0][0]), _bits(got[1][0])), (form, hex(word), fn, "not bitwise reproducible")
        if got[0][1] is not None:
            assert torch.equal(got[0][1], got[1][1]), (form, hex(word), fn, "arg not reproducible")
        return got[1][0].cpu().numpy(), None if got[1][1] is None else got[1][1].cpu().numpy()


def _contract(case, word, k, fn, prm):
    """(rowptr, col, x, y, ref, {kernel file: bound}, aux) of a named input: one pass over the fp64 reference serves every form."""
    if case == "prescribed":
        (rowptr, col), (x, y) = fc.prescribed_graph(), fc.prescribed_operands(k)
    elif case == "spread":
        rowptr, col = fc.named_graph()
        x, y = fc.spread_operands(word, 400, 300, k)
    else:
        rowptr, col = fc.combo_graph(k)
        x, y = fc.spread_operands(word, 70, 55, k)
    kind = fb.KINDS[fn]
    ref, bound, aux = fb.fusedmm_bound(word, rowptr, col, None, x, y, kind, prm, c_f=fb.C_F["general"])
    bounds = {"general": bound}
    if ((word >> 16) & 0xF) == 1:
        bounds["stream"] = bound + (fb.C_F["stream"][kind] - fb.C_F["general"][kind]) * aux["scalar"]
    return rowptr, col, x, y, ref, bounds, aux


# ---- a. the transfer curve: single-edge rows, z is f(s) with nothing else rounded --------------------------------------------

@pytest.mark.parametrize("fn", fc.MENU)
def test_transfer_curve_of_every_menu_entry(gpu, fn):
    """512 values of s from 0 over +-2^-20 to +-100 (exp entries: up to 80; 1 / (1 + s): s >= 0).  Every point is held to
    C_f * df(s) + FLT_MIN, C_f as measured by scripts/fusedmm_sop_accuracy.py; on the norm word z = f(s) a, so the product's own
    half ulp is allowed on top."""
    kind, npts = fb.KINDS[fn], 512
    rowptr, col = fc.probe_graph(npts)
    dev = _Device(gpu, rowptr, col, npts, task_geom=(4, 256, 16))
    try:
        for word in (fc.DOT_WORD, fc.NORM_WORD):
            if word == fc.DOT_WORD:
                s = fc.probe_grid(fn, npts)
                (x, y), column, factor = fc.probe_dot(s), 1, None
            else:
                factor = fc.probe_norm_args(fn, npts)
                s, (x, y), column = factor.astype(np.float64) ** 2, fc.probe_norm(factor), 0
            outs = {}
            for form in ("row", "task", "stream"):
                z, _ = dev.run(form, word, x, y, fn, fc.PARAM, geom=(1, 4, 64))
                assert not np.any(np.isnan(z)), (fn, form, "an element was not written")
                excess, df = fb.probe_excess(kind, fc.PARAM, s, z[:, column], factor)
                limit = fb.C_F[FILE_OF[form]][kind] * df
                worst = int(np.argmax(excess - limit))
                print(f"{fn} {hex(word)} {form}: max excess / df = {np.max(excess / np.maximum(df, 1e-300)):.3f}")
                assert np.all(excess <= limit), (fn, hex(word), form, float(s[worst]), float(z[worst, column]), float(excess[worst]), float(limit[worst]))
                outs[form] = z
            assert np.array_equal(outs["row"], outs["task"]), (fn, "the task form shares sop_apply with the row form")
    finally:
        dev.close()


# ---- b. overflow and saturation are exact -----------------------------------------------------------------------------

def test_overflow_and_saturation_are_exact(gpu):
    """exp / leaky_exp at s = 100 and 1e4: exactly +-inf by the sign of y_j[c] (no column of y_j is zero, so no inf * 0);
    sigmoid at s = +-1e4: exactly 1 and exactly 0 (s = 100 too), 1 - sigmoid the other way round."""
    s = np.array([100.0, 100.0, 1e4, 1e4, -1e4, -1e4], np.float32)
    m, k = s.size, 8
    rowptr, col = fc.probe_graph(m)
    x = np.zeros((m, k), np.float32)
    x[:, 0] = 1.0
    y = np.abs(cases.dense(m, k, 9)) + np.float32(0.25)
    y[:, 0] = s
    y[:, 1] = np.where(np.arange(m) % 2 == 0, 1.0, -1.0)
    y[:, 3] *= -1.0
    dev = _Device(gpu, rowptr, col, m, task_geom=(2, 64, 4))
    try:
        for form in ("row", "task", "stream"):
            run = lambda fn, prm: dev.run(form, fc.DOT_WORD, x, y, fn, prm, geom=(1, 1, 64))[0]      # noqa: E731
            for fn in ("exp", "leaky_exp"):                          # e^-1e4 and e^(-0.2 * 1e4) are 0 in any arithmetic
                z = run(fn, fc.PARAM)
                assert np.array_equal(z[:4], np.sign(y[:4]) * np.float32(np.inf)) and np.all(z[4:] == 0.0), (form, fn)
            z = run("sigmoid", 0.0)
            assert np.array_equal(z[:4], y[:4]) and np.all(z[4:] == 0.0), (form, "sigmoid")
            z = run("one_minus_sigmoid", 0.0)
            assert np.all(z[:4] == 0.0) and np.array_equal(z[4:], y[4:]), (form, "one_minus_sigmoid")
    finally:
        dev.close()


# ---- c. prescribed s in real rows ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", (5, 8, 32, 41, 64, 128, 300))
def test_prescribed_s_in_real_rows(gpu, k):
    """60 rows over 84 columns, a 300-edge hub, duplicates, an empty row; the dot product with y_j is y_j[0] exactly, and that
    cycles through {0, +-1e-3, +-0.5, +-1, +-3, +-10, +-17, +-30, +-60, +-80, +-86}.  Every output element to the bound (column
    0 under exp holds e^86 * 86, beyond FLT_MAX: fusedmm_bound.violations says what is required there).  Stream form for
    k in {8, 32, 64, 128} on a plan that cuts the hub row and on one that keeps it whole."""
    forms = [("row", None), ("task", None)]
    if k % 4 == 0 and k <= 128:
        forms += [("stream", g) for g in STREAM_PLANS]
    dev = None
    try:
        for fn in fc.menu_on(fc.DOT_WORD):
            rowptr, col, x, y, ref, bounds, aux = _contract("prescribed", fc.DOT_WORD, k, fn, fc.PARAM)
            dev = dev or _Device(gpu, rowptr, col, y.shape[0])
            for form, geom in forms:
                z, _ = dev.run(form, fc.DOT_WORD, x, y, fn, fc.PARAM, geom=geom)
                worst = fb.assert_within(z, ref, bounds[FILE_OF[form]], aux["mag"], (fn, k, form, geom))
                print(f"prescribed s, {fn}, k={k}, {form} {geom}: max error / bound = {worst:.3f}")
    finally:
        if dev:
            dev.close()


# ---- d. wide-spread s on ordinary data ---------------------------------------------------------------------------------

@pytest.mark.parametrize("word", (fc.DOT_WORD, fc.NORM_WORD), ids=("dot", "norm"))
@pytest.mark.parametrize("k", (32, 128, 602))
def test_wide_spread_s_on_the_named_pattern_graph(gpu, monkeypatch, word, k):
    """The graph of test_named_patterns_within_tolerance (400 x 300, a 2,500-edge hub) with operands scaled so that <x, y> has
    standard deviation 3 and |y - x|^2 mean 3: every menu entry defined on the word, through the row, task and stream forms and
    the plug-in's fusedmm() (its own choice, and the stream form forced), to the bound -- and to the former 1e-4 * max|ref| as
    well: nothing was loosened."""
    import isplib_amd
    from isplib_amd import cabi
    forms = [("row", None), ("task", None)]
    stream_ok = k % 4 == 0 and k <= 128
    if stream_ok:
        forms += [("stream", g) for g in STREAM_PLANS]
    dev = None
    try:
        for fn in fc.menu_on(word):
            rowptr, col, x, y, ref, bounds, aux = _contract("spread", word, k, fn, fc.PARAM)
            assert np.mean(np.abs(aux["s"]) > 3.0) >= 0.10, "the scalar stage must leave the neighbourhood of zero"
            if dev is None:
                dev = _Device(gpu, rowptr, col, y.shape[0], task_geom=(6, 512, 64))
                adj = isplib_amd.SparseTensor.from_csr(dev.d_rowptr, dev.d_col, None, (400, 300))
            old = 1e-4 * np.abs(ref).max() + 1e-7
            outs = [(form, geom, dev.run(form, word, x, y, fn, fc.PARAM, geom=geom)[0]) for form, geom in forms]
            d_x, d_y = _t(x, gpu), _t(y, gpu)
            outs.append(("row", "plug-in", isplib_amd.fusedmm(adj, d_x, d_y, word, sop_param=fc.PARAM, sop_udef=fn).cpu().numpy()))
            if stream_ok:
                with monkeypatch.context() as mp:
                    mp.setattr(cabi, "suggest_fusedmm_stream", lambda *a_, **k_: (_streams_for(k), 2, 64))
                    outs.append(("stream", "plug-in", isplib_amd.fusedmm(adj, d_x, d_y, word, sop_param=fc.PARAM, sop_udef=fn).cpu().numpy()))
                assert adj.storage._fusedmm_streams[(_streams_for(k), 2, 64)] is not None
            for form, geom, z in outs:
                worst = fb.assert_within(z, ref, bounds[FILE_OF[form]], aux["mag"], (hex(word), fn, k, form, geom))
                print(f"spread s, {hex(word)}, {fn}, k={k}, {form} {geom}: max error / bound = {worst:.3f}, / old rule = {np.max(np.abs(z - ref)) / old:.4f}")
                assert np.all(np.abs(z - ref) <= old), (hex(word), fn, k, form, geom, "the former rule")
    finally:
        if dev:
            dev.close()


# ---- e. other stage combinations with a real menu function ----------------------------------------------------------------

@pytest.mark.parametrize("k", (5, 41, 300))
def test_menu_functions_under_vsc_add_and_max_min(gpu, k):
    """sigmoid and leaky_exp with VSC_ADD / AOP_ADD and with VSC_MUL / AOP_MAX, AOP_MIN (values and winners' positions), on the
    VOP / ROP of both hot words; row and task forms.  70 rows with empty ones, duplicates (exact ties) and a 300-edge hub."""
    dev = None
    try:
        for word in fc.combo_words():
            aop = (word >> 16) & 0xF
            for fn in ("sigmoid", "leaky_exp"):
                rowptr, col, x, y, ref, bounds, aux = _contract("combo", word, k, fn, fc.PARAM)
                dev = dev or _Device(gpu, rowptr, col, y.shape[0], task_geom=(5, 128, 16))
                for form in ("row", "task"):
                    z, arg = dev.run(form, word, x, y, fn, fc.PARAM)
                    worst = fb.assert_within(z, ref, bounds["general"], aux["mag"], (hex(word), fn, k, form))
                    print(f"{hex(word)}, {fn}, k={k}, {form}: max error / bound = {worst:.3f}")
                    assert (arg is None) == (aop == 1)
                    if arg is not None:
                        fb.assert_arg_within(arg, rowptr, col.size, ref, bounds["general"], aux, aop == 2, (hex(word), fn, k, form))
                        assert np.all(z[np.diff(rowptr) == 0] == 0.0)
    finally:
        if dev:
            dev.close()


# ---- f. special operands ------------------------------------------------------------------------------------------------

def _special_close(got, oracle_z, ref, bound, what):
    """The rule of tests/test_gpu_parity.py (_assert_sum_close): the oracle's NaN mask, the oracle's infinities, the bound elsewhere."""
    fin = np.isfinite(oracle_z) & np.isfinite(bound)
    assert np.array_equal(np.isnan(got[~fin]), np.isnan(oracle_z[~fin])), (what, "NaN mask")
    inf = ~fin & ~np.isnan(oracle_z)
    assert np.array_equal(got[inf], oracle_z[inf]), (what, "infinities")
    err = np.abs(got[fin].astype(np.float64) - ref[fin])
    assert np.all(err <= bound[fin]), (what, f"max err / bound = {np.max(err / bound[fin])}")


@pytest.mark.parametrize("kind", ("signed_zero", "nonfinite", "denormal"))
@pytest.mark.parametrize("k", (64, 100))
def test_special_operands(gpu, oracle_mod, kind, k):
    """Signed zeros, non-finite values and subnormals in y (non-finite ones in x too) through SCALE with p = 1 on both hot words
    (all three forms) and through COPY_RHS|NOOP|COPY|MUL|ADD (row and task forms).  signed_zero is exact: the oracle's bits.
    denormal: the dot word with x scaled by 2^124 (<x, y> is then O(1) and s * y subnormal) and the copy word must produce
    subnormal outputs, held to the bound WITHOUT its floors plus one quantum 2^-149 per product -- plain multiplies and adds
    carry no fast intrinsic, so nothing may be flushed.  (s * T of the norm word is cubic in the operands: no input of this
    kind gives it subnormal outputs, and it runs with an ordinary x.)"""
    rowptr, col = cases.random_csr(128, 96, 20.0, seed=5, empty_rows=(3,), duplicates=True)
    val = cases.weights(col.size, 4, "signed_int")
    y = cases.dense(96, k, 3, kind)
    x_of = {"signed_zero": cases.dense(128, k, 7, "integer"), "nonfinite": cases.dense(128, k, 7, "nonfinite"), "denormal": cases.dense(128, k, 7)}
    dev = _Device(gpu, rowptr, col, 96, val=val, task_geom=(4, 128, 16))
    quantum = 2.0 ** -149
    try:
        for word, forms in ((fc.DOT_WORD, ("row", "task", "stream")), (fc.NORM_WORD, ("row", "task", "stream")), (fc.COPY_WORD, ("row", "task"))):
            x = x_of[kind]
            if kind == "denormal" and word == fc.DOT_WORD:
                x = x * np.float32(2.0 ** 124)
            fn, prm = ("scale", 1.0) if word != fc.COPY_WORD else ("none", 0.0)
            v = val if word == fc.COPY_WORD else None
            ref, bound, aux = fb.fusedmm_bound(word, rowptr, col, v, x, y, fb.KINDS.get(fn, 0), prm, c_f=fb.C_F["stream"])
            st, oz, _ = oracle_mod.fusedmm_general(word, rowptr, col, v, x, y, fb.KINDS.get(fn, 0), prm)
            assert st == 0
            sub = (np.abs(ref) >= 2.0 ** -140) & (np.abs(ref) < fb.FLT_MIN)
            if kind == "denormal" and word != fc.NORM_WORD:
                assert np.count_nonzero(sub) >= 100, "the case must produce subnormal outputs"
            for form in forms:
                for geom in (STREAM_PLANS if form == "stream" else (None,)):
                    what = (kind, k, hex(word), form, geom)
                    z, _ = dev.run(form, word, x, y, fn, prm, geom=geom)
                    _special_close(z, oz, ref, bound, what)
                    if kind == "signed_zero":
                        assert np.array_equal(z.view(np.int32), oz.view(np.int32)), (what, "exact, the sign of zero included")
                    if kind == "denormal" and word != fc.NORM_WORD:
                        tight = bound - 1e-30 + (np.diff(rowptr)[:, None] + 2) * quantum
                        assert np.all(z[sub] != 0.0) and np.all(np.abs(z - ref) <= tight), (what, "subnormal results were flushed")
    finally:
        dev.close()


@pytest.mark.parametrize("streams,k", ((2, 128), (4, 64), (8, 32)))
def test_nan_row_beside_finite_rows_in_one_stream_wave(gpu, streams, k):
    """cases.stream_uneven_wave: one wave whose slots walk 33, 16, 1, 0, 0, ... edges, so most steps of most slots are padding
    words on the spare LDS row.  x of row 1 is NaN throughout (and x of the empty row 3): row 1 comes out NaN, row 3 exactly 0,
    and every other row within the bound -- neither the padding steps nor the spare row leak into rows that are written."""
    rowptr, col = cases.stream_uneven_wave(streams, 33, 97, seed=streams)
    m = rowptr.size - 1
    dev = _Device(gpu, rowptr, col, 97, task_geom=(2, 64, 8))
    try:
        for word in (fc.DOT_WORD, fc.NORM_WORD):
            a = fc.spread_scale(word, k)
            x, y = cases.dense(m, k, 3) * a, cases.dense(97, k, 5) * a
            x[1] = np.nan
            if m > 3:
                x[3] = np.nan
            for fn in ("sigmoid", "scale"):
                ref, bound, aux = fb.fusedmm_bound(word, rowptr, col, None, x, y, fb.KINDS[fn], fc.PARAM, c_f=fb.C_F["stream"])
                assert np.all(np.isnan(ref[1])) and np.count_nonzero(np.isnan(ref)) == k
                z, _ = dev.run("stream", word, x, y, fn, fc.PARAM, geom=(3, 1, 256))
                assert np.array_equal(np.isnan(z), np.isnan(ref)), (hex(word), fn)
                clean = ~np.isnan(ref)
                assert np.all(np.abs(z[clean] - ref[clean]) <= bound[clean]), (hex(word), fn)
                assert np.all(z[np.diff(rowptr) == 0] == 0.0)
    finally:
        dev.close()
