"""Sparse multi-head dot-product attention with separate keys and values, host side (no GPU): the formulas of tests/mha_ref.py are
those of a dense masked-softmax composition under torch's autograd and of central differences, at H = 1 and k = v they are those of
tests/attention_ref.py, the bound is not too loose (six planted faults each miss it), the Python mirror of the domain rule agrees with
the header's, the header, MHA_EXPORTS and the library's symbols are consistent, and the plug-in refuses bad operands before anything
touches a device and hands the operator the views it was given.
"""
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from tests import attention_cases
from tests import attention_ref
from tests import mha_cases as cases
from tests import mha_ref as ref
from tests.test_gat_host import DOMAIN_TABLE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("isplib_mha_csr_hip", "isplib_mha_bw_rows_hip", "isplib_mha_bw_cols_hip", "isplib_mha_domain")
SCHEMA = ("mha_spmm(Tensor rowptr, Tensor col, Tensor colptr, Tensor row_t, Tensor q, Tensor k, Tensor v, int heads, float scale) "
          "-> Tensor")


def test_every_case_is_inside_the_first_order_range():
    """The bound is first order in rho: rho <= 1e-3 on every row and head of every case but the large one, which is held to 4e-3 as
    the attention large case is (each Case asserts its cap when it is built).  The figures are conditions on the inputs."""
    top, smax = 0.0, 0.0
    for case in cases.all_cases():
        cap = cases.LARGE_RHO_MAX if case.kind == "large" else ref.RHO_MAX
        assert case.rho_max == cap and float(case.bound["rho"].max()) <= cap, case.name
        if case in cases.config_cases():
            top, smax = max(top, float(case.bound["rho"].max())), max(smax, float(np.abs(case.ref["s"]).max()))
    assert [(c.heads, c.d) for c in cases.config_cases()] == list(cases.CONFIGS) and len(cases.CONFIGS) == 19
    assert all(c.p == 1.0 / np.sqrt(c.d) for c in cases.config_cases())
    assert top <= 7.3e-4 and smax < 10.5
    assert {c.p for c in cases.scale_cases()} == set(cases.SCALES) and min(cases.SCALES) < 0 and 1.0 / np.sqrt(8) not in cases.SCALES
    large = cases.large_case()
    spread = np.zeros(large.m)
    np.maximum.at(spread, large.ref["row"], np.abs(large.ref["s"]).max(1))
    assert (spread > 150).sum() > large.m // 4 and large.ref["s"].max() > 150 and large.ref["s"].min() < -150
    single = cases.single_case()
    assert np.diff(single.rowptr).max() == 1 and np.abs(single.ref["s"]).max() > 30


def _simple_graph(m, n, seed):
    """A graph without duplicate entries, with an empty row and an unreferenced column: -> rowptr, col, the dense 0/1 mask."""
    rng = np.random.default_rng(seed)
    mask = rng.random((m, n)) < 0.3
    mask[2] = False
    mask[:, 3] = False
    mask[m - 1, n - 1] = True
    row, col = np.nonzero(mask)
    rowptr = np.zeros(m + 1, dtype=np.int64)
    np.cumsum(np.bincount(row, minlength=m), out=rowptr[1:])
    return rowptr, col.astype(np.int64), mask


@pytest.mark.parametrize("heads,d,p", ((1, 7, None), (4, 8, None), (3, 16, -0.7)))
def test_reference_equals_torch_autograd_of_the_dense_composition(heads, d, p):
    """scores [H, M, N] by einsum, -inf where no entry is stored, softmax over the columns, a matrix product with v -- in fp64 on the
    CPU, under autograd.  A graph without duplicates: a dense mask cannot say "twice"."""
    m, n, K = 23, 17, heads * d
    p = 1.0 / math.sqrt(d) if p is None else p
    rowptr, col, mask = _simple_graph(m, n, 3)
    q, k, v, g = (cases.normal(s, 40 + i).astype(np.float64) for i, s in enumerate(((m, K), (n, K), (n, K), (m, K))))
    r = ref.mha(rowptr, col, q, k, v, heads, p, g)
    tq, tk, tv = (torch.from_numpy(a).requires_grad_(True) for a in (q, k, v))
    tm = torch.from_numpy(mask)
    s = p * torch.einsum("ihc,jhc->hij", tq.view(m, heads, d), tk.view(n, heads, d))
    s = torch.where(tm[None], s, torch.full_like(s, -float("inf")))
    live = tm.any(1)
    a = torch.where(live[None, :, None], torch.softmax(torch.where(live[None, :, None], s, torch.zeros_like(s)), dim=2), torch.zeros_like(s))
    a = torch.where(tm[None], a, torch.zeros_like(a))
    z = torch.einsum("hij,jhc->ihc", a, tv.view(n, heads, d)).reshape(m, K)
    z.backward(torch.from_numpy(g))
    lse = torch.logsumexp(s, dim=2).t().detach().numpy()
    for name, got in (("z", z.detach().numpy()), ("dq", tq.grad.numpy()), ("dk", tk.grad.numpy()), ("dv", tv.grad.numpy())):
        assert np.abs(got - r[name]).max() <= 1e-12 * max(np.abs(r[name]).max(), 1.0), name
    assert np.array_equal(np.isneginf(lse), np.isneginf(r["lse"])) and np.isneginf(r["lse"][2]).all()
    fin = np.isfinite(lse)
    assert np.abs(lse[fin] - r["lse"][fin]).max() <= 1e-12 * np.abs(lse[fin]).max()
    assert not r["z"][2].any() and not r["dq"][2].any() and not r["D"][2].any()           # the empty row
    assert not r["dk"][3].any() and not r["dv"][3].any()                                   # the column nothing references


def test_reference_agrees_with_central_differences():
    """L = sum(g * z) in fp64; duplicates and a negative scale included."""
    heads, d, p = 3, 4, -0.6
    m = n = 12
    rng = np.random.default_rng(11)
    deg = rng.integers(0, 6, size=m)
    deg[4] = 0
    rowptr = np.zeros(m + 1, dtype=np.int64)
    np.cumsum(deg, out=rowptr[1:])
    col = rng.integers(0, n, size=int(deg.sum()))
    col[rowptr[1]:rowptr[2]] = col[rowptr[1]] if deg[1] else 0                           # a row of duplicates
    K = heads * d
    q, k, v, g = (rng.standard_normal(s) for s in ((m, K), (n, K), (n, K), (m, K)))
    r = ref.mha(rowptr, col, q, k, v, heads, p, g)

    def loss(q_, k_, v_):
        return float((g * ref.mha(rowptr, col, q_, k_, v_, heads, p)["z"]).sum())

    h = 1e-6
    for name, which in (("dq", 0), ("dk", 1), ("dv", 2)):
        ops = [q, k, v]
        for _ in range(12):
            i, c = int(rng.integers(0, ops[which].shape[0])), int(rng.integers(0, K))
            up, dn = [a.copy() for a in ops], [a.copy() for a in ops]
            up[which][i, c] += h
            dn[which][i, c] -= h
            fd = (loss(*up) - loss(*dn)) / (2 * h)
            assert abs(fd - r[name][i, c]) <= 1e-7 * max(1.0, np.abs(r[name]).max()), (name, i, c, fd, r[name][i, c])


@pytest.mark.parametrize("k", (3, 33, 129))
def test_one_head_with_k_equal_v_is_the_attention_reference(k):
    """At H = 1 and k = v the operator is attention_matmul: z, lse, dx and their bounds are attention_ref's, dk + dv = dy and the two
    bounds add up to dy's."""
    a = attention_cases.width_case(k)
    r = ref.mha(a.rowptr, a.col, a.x, a.y, a.y, 1, a.p, a.g)
    b = ref.bounds(a.rowptr, a.col, a.x, a.y, a.y, 1, a.p, r, a.g)
    for mine, theirs in (("z", "z"), ("dq", "dx")):
        assert np.abs(r[mine] - a.ref[theirs]).max() <= 1e-13 * np.abs(a.ref[theirs]).max(), mine
        assert np.abs(b[mine] - a.bound[theirs]).max() <= 1e-12 * a.bound[theirs].max(), mine
    live = a.live
    assert np.isneginf(r["lse"][~live, 0]).all() and np.abs(r["lse"][live, 0] - a.ref["lse"][live]).max() <= 1e-13 * np.abs(a.ref["lse"][live]).max()
    assert np.abs(b["lse"][:, 0] - a.bound["lse"]).max() <= 1e-15 and np.abs(b["rho"][:, 0] - a.bound["rho"]).max() <= 1e-15
    assert np.abs(r["dk"] + r["dv"] - a.ref["dy"]).max() <= 1e-13 * np.abs(a.ref["dy"]).max()
    assert np.abs(b["dk"] + b["dv"] - a.bound["dy"]).max() <= 1e-12 * a.bound["dy"].max()
    assert np.abs(r["D"][:, 0] - a.ref["D"]).max() <= 1e-13 * max(np.abs(a.ref["D"]).max(), 1.0)


PICKED = ((1, 47), (8, 8), (3, 128))
OUTPUTS = ("z", "lse", "D", "dq", "dk", "dv")


def fractions(case, got):
    """error / bound per output; lse over the rows that have entries (an empty row's -inf is compared for equality)."""
    live, out = case.live, {}
    for name in OUTPUTS:
        if name == "lse":
            assert np.all(np.isneginf(np.asarray(got["lse"])[~live]))
            out[name] = ref.worst(np.asarray(got["lse"])[live], case.ref["lse"][live], case.bound["lse"][live])
        else:
            out[name] = ref.worst(got[name], case.ref[name], case.bound[name])
    return out


def _restated(case, p_score=None, value=None, keep_d=True, p_in_dk=True, dv_from_ds=False):
    """The outputs from the operands in fp64, written apart from mha_ref.mha, with switches for the planted faults."""
    H, m, n, K = case.heads, case.m, case.n, case.width
    row, col = case.ref["row"], case.col
    p = case.p if p_score is None else p_score
    q3, k3, g3 = (ref.per_head(a.astype(np.float64), H) for a in (case.q, case.k, case.g))
    v3 = ref.per_head((case.v if value is None else value).astype(np.float64), H)
    s = p * np.einsum("ehc,ehc->eh", q3[row], k3[col])
    top = np.full((m, H), -np.inf)
    np.maximum.at(top, row, s)
    w = np.exp(s - top[row])
    den = ref.segment_sum(w, row, m)
    a = w / den[row]
    with np.errstate(divide="ignore", invalid="ignore"):
        lse = np.where(case.live[:, None], top + np.log(den), -np.inf)
    z = ref.segment_sum(a[:, :, None] * v3[col], row, m)
    D = (g3 * z).sum(2)
    ds = a * ((g3[row] * v3[col]).sum(2) - (D[row] if keep_d else 0.0))
    return dict(z=z.reshape(m, K), lse=lse, D=D, dq=p * ref.segment_sum(ds[:, :, None] * k3[col], row, m).reshape(m, K),
                dk=(p if p_in_dk else 1.0) * ref.segment_sum(ds[:, :, None] * q3[row], col, n).reshape(n, K),
                dv=ref.segment_sum((ds if dv_from_ds else a)[:, :, None] * g3[row], col, n).reshape(n, K))


# fault -> the outputs that must miss the bound on at least one picked case
FAULTS = (("scale_from_K_not_d", lambda c: _restated(c, p_score=1.0 / np.sqrt(c.width)), ("z", "lse", "dq", "dk", "dv")),
          ("key_used_as_value", lambda c: _restated(c, value=c.k), ("z", "D", "dq", "dk")),              # dv and lse do not read v
          ("bf16_scores", None, ("z", "lse", "dq", "dk", "dv")),
          ("no_d_term", lambda c: _restated(c, keep_d=False), ("dq", "dk")),
          ("scale_dropped_from_dk", lambda c: _restated(c, p_in_dk=False), ("dk",)),
          ("dv_from_ds", lambda c: _restated(c, dv_from_ds=True), ("dv",)))


def _bf16_scores(case):
    q = torch.from_numpy(np.array(case.q)).to(torch.bfloat16).float().numpy()
    shadow = cases.Case.__new__(cases.Case)
    shadow.__dict__.update(case.__dict__)
    shadow.q = q
    out = _restated(shadow)
    return out


def test_the_unfaulted_restatement_passes():
    for heads, d in PICKED:
        case = cases.config_case(heads, d)
        frac = fractions(case, _restated(case))
        assert all(v <= 1e-3 for v in frac.values()), (case.name, frac)


@pytest.mark.parametrize("name,fault,outputs", FAULTS, ids=[f[0] for f in FAULTS])
def test_bound_is_not_too_loose(name, fault, outputs):
    """Planted faults miss the bound: the scale taken from K instead of the head width (only where H > 1), the key used as the value
    ("this is not attention_matmul"), q rounded to bf16 before the score, the D term dropped, the scale dropped from dk, dv formed
    from ds instead of a.  A switch that touches the backward only leaves the other outputs alone."""
    picked = [cases.config_case(h, d) for h, d in PICKED]
    fracs = [fractions(c, (fault or _bf16_scores)(c)) for c in picked]
    print(name, [{k: round(v, 2) for k, v in f.items()} for f in fracs])
    for out in outputs:
        assert any(f[out] > 1.0 for f in fracs), (name, out)
    if name in ("no_d_term", "scale_dropped_from_dk", "dv_from_ds"):
        for out in set(OUTPUTS) - set(outputs):
            assert all(f[out] <= 1e-3 for f in fracs), (name, out)
    if name == "scale_from_K_not_d":                                        # one head: K is d, the two scales coincide
        assert all(v <= 1e-3 for v in fracs[0].values())


def test_python_mirror_of_the_domain_rule():
    from isplib_amd import cabi
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "isplib_hip_mha.h")).read(), flags=re.S)
    L = cabi.lib()
    top = cabi.DENSE_BYTES_MAX // 4
    table = DOMAIN_TABLE + ((top // 64, 8, 8, 64), (top // 64 + 1, 8, 8, 64), (top // 64, 4, 8, 64), (1000, 4, 4, top // 1000),
                            (1000, 4, 4, top // 1000 + 1), (top // 192, 8, 8, 192), (top // 192 + 1, 8, 8, 192), (10, 8, 8, 192))
    for rows, heads, d, ld in table:
        want = bool(L.isplib_mha_domain(rows, heads, d, ld))
        assert want == cabi.mha_serves(rows, heads, d, ld) == cabi.gat_serves(rows, heads, d, ld) == bool(L.isplib_gat_domain(rows, heads, d, ld)), \
            (rows, heads, d, ld)
    assert any(cabi.mha_serves(*t) for t in table) and not all(cabi.mha_serves(*t) for t in table)
    # stated once: the header's inline returns isplib_gat_serves(...)
    assert re.search(r"static inline int isplib_mha_serves\([^)]*\)\s*\{\s*return isplib_gat_serves\(rows_gathered, heads, d, ld\);\s*\}", header)


def test_header_exports_and_symbols_are_consistent():
    from isplib_amd import _lib, cabi
    main = open(os.path.join(ROOT, "include", "isplib_hip.h")).read()
    assert re.search(r'^#include "isplib_hip_mha.h"$', main, re.M)
    assert "isplib_mha_" not in re.sub(r"/\*.*?\*/", "", main, flags=re.S)                 # declared in the header of their own only
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "isplib_hip_mha.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"^\s*int\s+(\w+)\s*\(", header, flags=re.M)))
    assert declared == sorted(ENTRIES) == sorted(cabi.MHA_EXPORTS)
    nm = subprocess.check_output(["nm", "-D", "--defined-only", _lib.CABI_PATH], text=True)
    exported = {line.split()[-1] for line in nm.splitlines() if " T " in line}
    assert {n for n in exported if n.startswith("isplib_mha")} == set(ENTRIES)
    L = cabi.lib()
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in ENTRIES:
        assert name not in cabi.EXPORTS
        assert getattr(L, name) is not None
        assert name in integration, name
    assert int(re.search(r"#define\s+ISPLIB_HIP_ABI_VERSION\s+(\d+)", main).group(1)) == L.isplib_hip_abi_version()
    # the argument lists of the issue: the forward's operands lead the rows entry's; the columns entry writes two outputs
    fw = re.search(r"isplib_mha_csr_hip\((.*?)\);", header, re.S).group(1)
    rows = re.search(r"isplib_mha_bw_rows_hip\((.*?)\);", header, re.S).group(1)
    cols = re.search(r"isplib_mha_bw_cols_hip\((.*?)\);", header, re.S).group(1)
    names = lambda proto: [re.sub(r"\s+", " ", a).strip().split(" ")[-1].lstrip("*") for a in proto.split(",")]      # noqa: E731
    assert names(fw) == ["m", "n", "k", "nnz", "indx", "pntrb", "pntre", "heads", "scale", "q", "ldq", "key", "ldk", "v", "ldv", "z",
                         "ldz", "lse", "stream"]
    assert names(rows)[:15] == names(fw)[:15] and names(rows)[15:] == ["g", "ldg", "z", "ldz", "lse", "dq", "lddq", "dsum", "stream"]
    assert names(cols) == ["m", "n", "k", "nnz", "row_t", "colb", "cole", "heads", "scale", "q", "ldq", "g", "ldg", "lse", "dsum", "key",
                           "ldk", "v", "ldv", "dkey", "lddk", "dv", "lddv", "stream"]
    for fn, proto in ((L.isplib_mha_csr_hip, fw), (L.isplib_mha_bw_rows_hip, rows), (L.isplib_mha_bw_cols_hip, cols)):
        assert len(fn.argtypes) == len(names(proto))
    src = open(os.path.join(ROOT, "isplib_amd", "csrc", "Makefile")).read()
    assert re.search(r"^HIP_SRCS\s*:=.*\bmha\.hip\b", src, re.M)


def test_the_operator_schema_is_registered():
    import isplib_amd  # noqa: F401
    assert str(torch.ops.isplib.mha_spmm.default._schema) == "isplib::" + SCHEMA


def _adj(m, n):
    import isplib_amd
    rowptr = torch.arange(0, m + 1, dtype=torch.int64)
    col = torch.arange(m, dtype=torch.int64) % n
    return isplib_amd.SparseTensor.from_csr(rowptr, col, None, (m, n))


def test_plugin_refuses_bad_operands_before_any_library_call():
    import isplib_amd
    adj = _adj(6, 4)
    q, k, v = torch.zeros(6, 16), torch.zeros(4, 16), torch.zeros(4, 16)           # CPU tensors: a launch is impossible
    with pytest.raises(TypeError, match="GPU tensor"):
        isplib_amd.mha_matmul(adj, q, k, v, heads=2)                             # well-formed: there is no CPU path
    with pytest.raises(TypeError, match="GPU tensor"):
        adj.mha_matmul(q, k, k, 2, 0.25)                                         # k is v is well-formed
    with pytest.raises(TypeError, match="GPU tensor"):
        adj.mha_matmul(q, k, v, scale=-1)                                        # one head, a negative int scale
    for pos in range(3):
        for dt in (torch.bfloat16, torch.float16, torch.float64):
            ops = [q, k, v]
            ops[pos] = ops[pos].to(dt)
            with pytest.raises(TypeError, match="float32"):
                isplib_amd.mha_matmul(adj, *ops, heads=2)
        ops = [q, k, v]
        ops[pos] = ops[pos].numpy()
        with pytest.raises(TypeError, match="tensor"):
            isplib_amd.mha_matmul(adj, *ops, heads=2)
        ops = [q, k, v]
        ops[pos] = ops[pos][0]
        with pytest.raises(ValueError, match="2-D"):
            isplib_amd.mha_matmul(adj, *ops, heads=2)
    with pytest.raises(ValueError, match="`q` must have one row per row"):
        isplib_amd.mha_matmul(adj, torch.zeros(4, 16), k, v, heads=2)
    with pytest.raises(ValueError, match="`k` must have one row per column"):
        isplib_amd.mha_matmul(adj, q, torch.zeros(6, 16), v, heads=2)
    with pytest.raises(ValueError, match="`v` must have one row per column"):
        isplib_amd.mha_matmul(adj, q, k, torch.zeros(6, 16), heads=2)
    with pytest.raises(ValueError, match="same width"):
        isplib_amd.mha_matmul(adj, q, torch.zeros(4, 8), v, heads=2)
    with pytest.raises(ValueError, match="same width"):
        isplib_amd.mha_matmul(adj, q, k, torch.zeros(4, 32), heads=2)
    with pytest.raises(ValueError, match="heads \\* d"):
        isplib_amd.mha_matmul(adj, q, k, v, heads=3)
    for bad in (0, -1, True, 2.0):
        with pytest.raises(ValueError, match="positive int"):
            isplib_amd.mha_matmul(adj, q, k, v, heads=bad)
    with pytest.raises(ValueError, match="power of two"):
        isplib_amd.mha_matmul(adj, torch.zeros(6, 12), torch.zeros(4, 12), torch.zeros(4, 12), heads=2)        # d = 6
    with pytest.raises(ValueError, match="power of two"):
        isplib_amd.mha_matmul(adj, torch.zeros(6, 4), torch.zeros(4, 4), torch.zeros(4, 4), heads=2)           # d = 2
    with pytest.raises(ValueError, match="512"):
        adj.mha_matmul(torch.zeros(6, 513), torch.zeros(4, 513), torch.zeros(4, 513))
    with pytest.raises(ValueError, match="512"):
        adj.mha_matmul(torch.zeros(6, 1024), torch.zeros(4, 1024), torch.zeros(4, 1024), heads=2)
    for bad in (float("nan"), float("inf"), -float("inf"), "0.5", True, torch.tensor(0.5), np.float32(0.5)):
        with pytest.raises(ValueError, match="`scale` must be a finite Python number"):
            isplib_amd.mha_matmul(adj, q, k, v, heads=2, scale=bad)
    assert isplib_amd.mha_matmul is isplib_amd.plugin.mha_matmul and "mha_matmul" in isplib_amd.__all__
    doc = isplib_amd.plugin.mha_matmul.__doc__
    assert "dropout" in doc and "edge features" in doc and "beta" in doc and "no fallback" in doc


class _Flagged(torch.Tensor):                                           # CPU tensors that claim to be on the GPU: nothing is launched
    is_cuda = True


def _fake_ops(monkeypatch, calls):
    from isplib_amd import plugin

    class Ops:
        @staticmethod
        def mha_spmm(*args):
            calls.append(args)
            return "z"

    class FakeTorchOps:
        isplib = Ops

    monkeypatch.setattr(plugin.torch, "ops", FakeTorchOps)
    adj = _adj(6, 6)
    st = adj.storage
    st._colptr, st._csr2csc, st._row_t = torch.zeros(7, dtype=torch.int64), torch.arange(6), torch.arange(6)    # the cached transpose
    return adj, st


def test_the_plugin_passes_the_views_own_pitches_and_the_head_scale(monkeypatch):
    import isplib_amd
    calls = []
    adj, st = _fake_ops(monkeypatch, calls)
    K = 32
    fused = torch.zeros(6, 3 * K).as_subclass(_Flagged)
    q, k, v = fused[:, :K], fused[:, K:2 * K], fused[:, 2 * K:]
    assert isplib_amd.mha_matmul(adj, q, k, v, heads=4) == "z"
    assert adj.mha_matmul(q, k, k, 4, -0.5) == "z"
    assert adj.mha_matmul(q, k, v) == "z"
    a, b, c = calls
    assert len(a) == 9 and a[0] is st._rowptr and a[1] is st._col and a[2] is st._colptr and a[3] is st._row_t
    assert a[4] is q and a[5] is k and a[6] is v                             # the views themselves: no copy, no .contiguous()
    assert [t.stride(0) for t in a[4:7]] == [3 * K] * 3 and [t.storage_offset() for t in a[4:7]] == [0, K, 2 * K]
    assert a[7] == 4 and type(a[8]) is float and a[8] == 1.0 / math.sqrt(8)  # the HEAD width, not K
    assert b[5] is k and b[6] is k and b[7:] == (4, -0.5)
    assert c[7] == 1 and c[8] == 1.0 / math.sqrt(K)


def test_the_byte_domain_is_asked_of_every_operand_at_its_own_pitch(monkeypatch):
    """3.5 GiB behind one descriptor: rows * pitch * 4.  A contiguous operand of these sizes passes where a view of a fused
    [rows, 3 K] projection does not -- for k, v and q alike; the gradient is packed and passes with them.  Meta tensors: shapes and
    strides without storage."""
    import types

    import isplib_amd
    from isplib_amd import cabi
    calls = []
    _fake_ops(monkeypatch, calls)
    K, rows = 64, cabi.DENSE_BYTES_MAX // (4 * 64)                               # rows * K * 4 == the limit exactly
    st = types.SimpleNamespace(_rowptr=torch.empty(rows + 1, dtype=torch.int64, device="meta"), _sparse_sizes=(rows, rows),
                               _col=torch.empty(0, dtype=torch.int64, device="meta"), colptr=lambda: None, row_t=lambda: None)
    monkeypatch.setattr(isplib_amd.plugin, "_storage_of", lambda src, other: st)
    tight = torch.empty((rows, K), device="meta").as_subclass(_Flagged)
    wide = torch.empty((rows, 3 * K), device="meta")[:, K:2 * K].as_subclass(_Flagged)
    assert isplib_amd.mha_matmul(None, tight, tight, tight, heads=8) == "z"
    for pos, what in ((0, "`q`"), (1, "`k`"), (2, "`v`")):
        ops = [tight, tight, tight]
        ops[pos] = wide
        with pytest.raises(ValueError, match=what + r" \(\d+ rows at a pitch of 192 floats\) is outside"):
            isplib_amd.mha_matmul(None, *ops, heads=8)
    # one row more and the packed operands leave the domain too: q is named first, the packed gradient shares its rule
    st._rowptr = torch.empty(rows + 2, dtype=torch.int64, device="meta")
    with pytest.raises(ValueError, match=r"`q` \(\d+ rows at a pitch of 64 floats\) is outside"):
        isplib_amd.mha_matmul(None, torch.empty((rows + 1, K), device="meta").as_subclass(_Flagged), tight, tight, heads=8)
    assert len(calls) == 1


def test_ctypes_wrappers_refuse_bad_operands_before_the_call():
    from isplib_amd import cabi
    rowptr, col = torch.arange(0, 7, dtype=torch.int64), torch.arange(6, dtype=torch.int64) % 4
    colptr = torch.arange(0, 5, dtype=torch.int64)
    q, k, v, g = torch.zeros(6, 16), torch.zeros(4, 16), torch.zeros(4, 16), torch.zeros(6, 16)
    lse = torch.zeros(6, 2)
    with pytest.raises(TypeError, match="float32"):
        cabi.mha(rowptr, col, q, k.to(torch.bfloat16), v, 2)
    with pytest.raises(TypeError, match="float32"):
        cabi.mha(rowptr, col, q, k, v.to(torch.float16), 2)
    with pytest.raises(TypeError, match="int64"):
        cabi.mha(rowptr.to(torch.int32), col, q, k, v, 2)
    with pytest.raises(ValueError, match="unit inner stride"):
        cabi.mha(rowptr, col, q, torch.zeros(16, 4).t(), v, 2)
    with pytest.raises(ValueError, match=r"`v` must be \[4, 16\]"):
        cabi.mha(rowptr, col, q, k, torch.zeros(4, 8), 2)
    with pytest.raises(ValueError, match="heads \\* d"):
        cabi.mha(rowptr, col, q, k, v, 3)
    with pytest.raises(ValueError, match="`scale` must be a finite number"):
        cabi.mha(rowptr, col, q, k, v, 2, float("nan"))
    with pytest.raises(ValueError, match="GPU tensor"):
        cabi.mha(rowptr, col, q, k, v, 2)                                        # well-formed, but on the CPU
    with pytest.raises(ValueError, match="isplib_gat_serves"):
        cabi.mha(rowptr, col, torch.zeros(6, 12), torch.zeros(4, 12), torch.zeros(4, 12), 2)      # d = 6
    with pytest.raises(ValueError, match="isplib_gat_serves"):
        cabi.mha(rowptr, col, torch.zeros(6, 513), torch.zeros(4, 513), torch.zeros(4, 513), 1)
    with pytest.raises(ValueError, match=r"`lse` must be \[6, 2\]"):
        cabi.mha_bw_rows(rowptr, col, q, k, v, g, g, torch.zeros(5, 2), 2)
    with pytest.raises(ValueError, match=r"\[6, 16\]"):
        cabi.mha_bw_rows(rowptr, col, q, k, v, torch.zeros(6, 15), g, lse, 2)
    with pytest.raises(ValueError, match="GPU tensor"):
        cabi.mha_bw_rows(rowptr, col, q, k, v, g, g, lse, 2)
    with pytest.raises(ValueError, match=r"`dsum` must be \[6, 2\]"):
        cabi.mha_bw_cols(colptr, col, q, k, v, g, lse, torch.zeros(6, 1), 2)
    with pytest.raises(ValueError, match=r"`q` must be \[6, 16\]"):
        cabi.mha_bw_cols(colptr, col, torch.zeros(6, 8), k, v, g, lse, lse, 2)
    with pytest.raises(ValueError, match=r"\(dk, dv\)"):
        cabi.mha_bw_cols(colptr, col, q, k, v, g, lse, lse, 2, out=(torch.zeros(4, 16),))
    with pytest.raises(ValueError, match="GPU tensor"):
        cabi.mha_bw_cols(colptr, col, q, k, v, g, lse, lse, 2)
    assert cabi.mha_serves(10, 8, 8, 64) and not cabi.mha_serves(10, 8, 8, 63)
