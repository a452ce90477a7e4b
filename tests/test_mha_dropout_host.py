"""Sparse multi-head attention (q, k, v) with attention dropout, without a GPU: the reference of tests/mha_dropout_ref.py against a torch
fp64 autograd composition and against central differences, its bounds against planted faults, its cases, the argument checks of
mha_matmul(..., dropout=, training=, seed=) -- all raised before anything touches a device -- the call paths, and the new exports and
operator schema.
"""
import inspect
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from tests import mha_cases
from tests import mha_dropout_cases as cases
from tests import mha_dropout_ref as ref
from tests import mha_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("isplib_qkv_drop_csr_hip", "isplib_qkv_drop_bw_rows_hip", "isplib_qkv_drop_bw_cols_hip")
OUTPUTS = ("z", "lse", "D", "dq", "dk", "dv")
SCHEMA = ("mha_drop_spmm(Tensor rowptr, Tensor col, Tensor colptr, Tensor row_t, Tensor csr2csc, Tensor q, Tensor k, Tensor v, "
          "int heads, float scale, float p, int seed) -> Tensor")


@pytest.mark.parametrize("heads,d,scale,p", ((8, 8, None, 0.6), (1, 47, None, 0.6), (8, 8, -0.3, 0.9)))
def test_reference_equals_torch_autograd_of_the_composition_with_the_same_mask(heads, d, scale, p):
    """Per-edge dot products, a scatter softmax written with index_add_, mask * c ON THE COEFFICIENTS, a weighted sum -- fp64 on the
    CPU, under autograd; the mask is isplib_amd.gat_dropout_mask.  The graph has duplicates, which a per-edge composition can say."""
    import isplib_amd
    case = cases.config_case(heads, d, scale, p)
    row, col = torch.from_numpy(case.ref["row"]), torch.from_numpy(np.array(case.col))
    q, k, v = (torch.from_numpy(np.array(a)).double().requires_grad_(True) for a in (case.q, case.k, case.v))
    s = case.ps * (q.view(case.m, heads, d)[row] * k.view(case.n, heads, d)[col]).sum(-1)
    top = np.full((case.m, heads), -np.inf)
    np.maximum.at(top, row.numpy(), s.detach().numpy())
    w = torch.exp(s - torch.from_numpy(top)[row])
    den = torch.zeros(case.m, heads, dtype=torch.float64).index_add_(0, row, w)
    mask = isplib_amd.gat_dropout_mask(case.nnz, heads, case.p, case.seed)
    assert np.array_equal(mask.numpy(), case.ref["q"])
    a = (w / den[row]) * mask.double() * float(np.float32(1.0 / (1.0 - case.p)))
    z = torch.zeros(case.m, heads, d, dtype=torch.float64).index_add_(0, row, a[:, :, None] * v.view(case.n, heads, d)[col]).view(case.m, heads * d)
    z.backward(torch.from_numpy(np.array(case.g)).double())
    for name, got in (("z", z.detach()), ("dq", q.grad), ("dk", k.grad), ("dv", v.grad)):
        want = case.ref[name]
        assert np.abs(got.numpy() - want).max() <= 1e-9 * np.abs(want).max(), name


@pytest.mark.parametrize("heads,d,ps,p", ((1, 3, 0.7, 0.5), (3, 4, -0.6, 0.6), (2, 4, 0.5, 0.3)))
def test_reference_gradients_are_central_differences_of_its_forward(heads, d, ps, p):
    """L = <g, z> in fp64 with the mask and c fixed; a row of duplicates, an empty row and a negative score scale included."""
    m = n = 12
    rng = np.random.default_rng(11 * heads + d)
    deg = rng.integers(0, 6, size=m)
    deg[4], deg[1] = 0, 3
    rowptr = np.zeros(m + 1, dtype=np.int64)
    np.cumsum(deg, out=rowptr[1:])
    col = rng.integers(0, n, size=int(deg.sum()))
    col[rowptr[1]:rowptr[2]] = col[rowptr[1]]                                            # a row of duplicates
    K = heads * d
    q, k, v, g = (rng.standard_normal(s) for s in ((m, K), (n, K), (n, K), (m, K)))
    seed = next(s for s in range(1, 100) if len(set(map(tuple, ref.keep(s, col.size, heads, p)[rowptr[1]:rowptr[2]]))) > 1)
    got = ref.mha_drop(rowptr, col, q, k, v, heads, ps, p, seed, g)
    mask = got["q"]
    assert mask.any() and not mask.all() and len(set(map(tuple, mask[rowptr[1]:rowptr[2]]))) > 1      # the duplicates' bits differ

    def loss(q_, k_, v_):
        return float((g * ref.mha_drop(rowptr, col, q_, k_, v_, heads, ps, p, seed)["z"]).sum())

    h = 1e-6
    for name, which in (("dq", 0), ("dk", 1), ("dv", 2)):
        ops = [q, k, v]
        want = np.zeros_like(ops[which])
        for idx in np.ndindex(*want.shape):
            up, dn = [a.copy() for a in ops], [a.copy() for a in ops]
            up[which][idx] += h
            dn[which][idx] -= h
            want[idx] = (loss(*up) - loss(*dn)) / (2 * h)
        assert np.abs(want - got[name]).max() <= 1e-7 * max(1.0, np.abs(want).max()), name


@pytest.mark.parametrize("heads,d,scale", ((1, 7, None), (8, 8, -0.3), (3, 128, None), (8, 64, None)))
def test_zero_probability_is_the_reference_without_dropout(heads, d, scale):
    assert ref.threshold(0.0) == 0 and ref.scale(0.0) == np.float32(1.0)
    base = mha_cases.config_case(heads, d, scale)
    got = ref.mha_drop(base.rowptr, base.col, base.q, base.k, base.v, heads, base.p, 0.0, 77, base.g)
    assert got["q"].all()
    for name in OUTPUTS + ("s", "a", "t", "ds"):
        assert np.array_equal(got[name], base.ref[name]), name
    bound = ref.bounds(base.rowptr, base.col, base.q, base.k, base.v, heads, base.p, got, base.g)
    for name in OUTPUTS:                                                 # one more rounding on z and in dv: never tighter than without dropout
        assert np.all(bound[name] >= base.bound[name]), name
    for name in ("dq", "dk", "lse", "rho"):
        assert np.array_equal(bound[name], base.bound[name]), name
    assert mha_ref.per_head is ref.per_head


def test_every_case_builds_with_the_properties_its_tests_rely_on():
    built = cases.all_cases()
    assert len(built) == len(cases.CONFIGS) + 10 + 5 and len(cases.CONFIGS) == 19
    assert max(float(c.bound["rho"].max()) for c in built) <= ref.RHO_MAX
    for case in built:
        assert case.ref["lse"] is case.base.ref["lse"] and case.ref["a"] is case.base.ref["a"]       # the softmax does not see the mask
        assert case.ref["q"].any() and not case.ref["q"].all()
    assert {(c.heads, c.width // c.heads, c.ps, c.p) for c in cases.scale_cases()} == \
        {(8, 8, s, p) for s in cases.SCALES for p in (0.1, 0.9)} | \
        {(h, d, 1.0 / np.sqrt(d), p) for h, d in cases.FORM_CONFIGS for p in (0.1, 0.9)}
    assert min(cases.SCALES) < 0
    # the figures of the 200 x 200 graph at (8, 8) under SEED: kept fraction, all-dropped live (row, head) pairs, rows they lie in
    base = mha_cases.config_case(8, 8)
    assert base.col.size == 7100 and int((~base.live).sum()) == 8
    for p, frac, pairs, rows in ((0.1, 0.899, 9, 6), (0.6, 0.399, 82, 30), (0.9, 0.101, 341, 82)):
        case = cases.config_case(8, 8, None, p)
        gone = case.all_dropped()
        assert round(float(case.ref["q"].mean()), 3) == frac and int(gone.sum()) == pairs and int(gone.any(1).sum()) == rows, p
        assert np.all(ref.per_head(case.ref["z"], 8)[gone] == 0) and np.all(np.isfinite(case.ref["lse"][gone]))
    single = cases.single_case()
    assert int(np.diff(single.rowptr).max()) == 1 and single.live.sum() == 160
    assert (single.kept_in[single.has_in] == 0).any() and (single.kept_in[single.has_in] > 0).any()
    assert single.ref["q"].any(0).all() and (~single.ref["q"]).any(0).all()
    dup = cases.duplicate_case()
    e1, e2 = dup.pairs[0]
    assert dup.ref["row"][e1] == dup.ref["row"][e2] and dup.col[e1] == dup.col[e2] and np.any(dup.ref["q"][e1] != dup.ref["q"][e2])
    assert dup.wide.any() and len(dup.pairs) == 3298
    assert cases.position_case().ref["q"].shape == (dup.nnz, 8)
    rect = cases.rect_case()
    assert (rect.m, rect.n) == (67, 233)
    assert cases.shared_case().v is cases.shared_case().k
    for heads, d in cases.FUSED_CONFIGS:
        fused = cases.fused_case(heads, d)
        K = heads * d
        assert np.array_equal(fused.fused[:, K:2 * K], fused.k) and np.array_equal(fused.fused[:, 2 * K:], fused.v)


PICKED = ((1, 47), (8, 8), (3, 128))


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


def _restated(case, mask=None, mask_in_t=True, dropped_ds=True, c_in_dv=True, softmax_over_all=True):
    """The outputs from the operands in fp64, written apart from mha_dropout_ref.mha_drop, with switches for the planted faults."""
    H, m, n, K = case.heads, case.m, case.n, case.width
    row, col = case.ref["row"], case.col
    keep = (case.ref["q"] if mask is None else mask).astype(np.float64)
    c = float(np.float32(1.0 / (1.0 - case.p)))
    q3, k3, v3, g3 = (ref.per_head(a.astype(np.float64), H) for a in (case.q, case.k, case.v, case.g))
    s = case.ps * np.einsum("ehc,ehc->eh", q3[row], k3[col])
    top = np.full((m, H), -np.inf)
    np.maximum.at(top, row, s)
    w = np.exp(s - top[row])
    den = ref.segment_sum(w if softmax_over_all else w * keep, row, m)
    with np.errstate(divide="ignore", invalid="ignore"):
        a = np.where(den[row] > 0, w / den[row], 0.0)
        lse = np.where(case.live[:, None], top + np.log(den), -np.inf)
    z = c * ref.segment_sum((keep * a)[:, :, None] * v3[col], row, m)
    D = (g3 * z).sum(2)
    t = (keep * c if mask_in_t else 1.0) * (g3[row] * v3[col]).sum(2)
    ds = a * (t - D[row])
    if not dropped_ds:
        ds = ds * keep
    return dict(z=z.reshape(m, K), lse=lse, D=D, dq=case.ps * ref.segment_sum(ds[:, :, None] * k3[col], row, m).reshape(m, K),
                dk=case.ps * ref.segment_sum(ds[:, :, None] * q3[row], col, n).reshape(n, K),
                dv=(c if c_in_dv else 1.0) * ref.segment_sum((keep * a)[:, :, None] * g3[row], col, n).reshape(n, K))


def _headless(case):
    return np.repeat(case.ref["q"][:, :1], case.heads, axis=1)


# fault -> the outputs that must miss the bound on at least one picked case
FAULTS = (("mask_ignored_in_t", lambda c: _restated(c, mask_in_t=False), ("dq", "dk")),
          ("dropped_edge_gets_no_ds", lambda c: _restated(c, dropped_ds=False), ("dq", "dk")),
          ("c_left_out_of_dv", lambda c: _restated(c, c_in_dv=False), ("dv",)),
          ("lse_over_kept_entries_only", lambda c: _restated(c, softmax_over_all=False), ("z", "lse", "dv")),
          ("mask_ignores_the_head", lambda c: _restated(c, mask=_headless(c)), ("z", "D", "dq", "dk", "dv")))


def test_the_unfaulted_restatement_passes():
    for case in [cases.config_case(h, d) for h, d in PICKED] + [cases.duplicate_case(), cases.config_case(8, 8, -0.3, 0.9)]:
        frac = fractions(case, _restated(case))
        assert all(v <= 1e-3 for v in frac.values()), (case.name, frac)


@pytest.mark.parametrize("name,fault,outputs", FAULTS, ids=[f[0] for f in FAULTS])
def test_bound_is_not_too_loose(name, fault, outputs):
    """Planted faults miss the bound: t_e left unmasked while z is masked, a dropped edge given ds = 0 instead of -a_e D, c left out
    of dv, the softmax (and lse) taken over the kept entries only, a mask that gives every head the bit of head 0 (only where H > 1).
    A switch that touches the backward only leaves the other outputs alone."""
    picked = [cases.config_case(h, d) for h, d in PICKED]
    fracs = [fractions(c, fault(c)) for c in picked]
    print(name, [{k: round(v, 2) for k, v in f.items()} for f in fracs])
    for out in outputs:
        assert any(f[out] > 1.0 for f in fracs), (name, out)
    if name in ("mask_ignored_in_t", "dropped_edge_gets_no_ds", "c_left_out_of_dv"):
        for out in set(OUTPUTS) - set(outputs):
            assert all(f[out] <= 1e-3 for f in fracs), (name, out)
    if name == "mask_ignores_the_head":                                     # one head: the two masks coincide
        assert all(v <= 1e-3 for v in fracs[0].values())


def test_a_mask_indexed_by_row_and_column_misses_the_bound_on_the_duplicate_case():
    case = cases.duplicate_case()
    wrong = cases.pair_mask(case)
    e1, e2 = case.pairs[0]
    assert np.array_equal(wrong[e2], case.ref["q"][e1]) and np.any(wrong[e2] != case.ref["q"][e2])
    frac = fractions(case, _restated(case, mask=wrong))
    print({k: round(v, 2) for k, v in frac.items()})
    assert frac["z"] > 10.0 and frac["dv"] > 1.0 and frac["dq"] > 1.0 and frac["lse"] <= 1e-3


def test_header_exports_symbols_and_integration_are_consistent():
    from isplib_amd import _lib, cabi
    main = open(os.path.join(ROOT, "include", "isplib_hip.h")).read()
    bare = re.sub(r"/\*.*?\*/", "", main, flags=re.S)
    assert re.search(r'^#include "isplib_hip_mha_drop.h"$', bare, re.M)
    assert "qkv_drop_" not in bare and "mha_drop" not in bare.replace("isplib_hip_mha_drop.h", "")        # declared there only
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "isplib_hip_mha_drop.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"^\s*int\s+(\w+)\s*\(", header, flags=re.M)))
    assert declared == sorted(ENTRIES) == sorted(cabi.MHA_DROP_EXPORTS)
    nm = subprocess.check_output(["nm", "-D", "--defined-only", _lib.CABI_PATH], text=True)
    exported = {line.split()[-1] for line in nm.splitlines() if " T " in line}
    assert {n for n in exported if n.startswith("isplib_qkv_drop")} == set(ENTRIES)
    assert not any(n.startswith(("isplib_mha", "isplib_qkv16")) for n in ENTRIES)          # those two prefixes are pinned elsewhere
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    L = cabi.lib()
    for name in ENTRIES:
        assert name not in cabi.EXPORTS + cabi.MHA_EXPORTS + cabi.MHA16_EXPORTS
        assert getattr(L, name) is not None
        assert name in integration, name
    assert int(re.search(r"#define\s+ISPLIB_HIP_ABI_VERSION\s+(\d+)", main).group(1)) == 1
    assert L.isplib_hip_abi_version() == 1
    # the argument lists: those of the entries without dropout (csr2csc after cole in the columns entry), then threshold, keep_scale, seed
    plain = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "isplib_hip_mha.h")).read(), flags=re.S)
    names = lambda proto: [re.sub(r"\s+", " ", a).strip().split(" ")[-1].lstrip("*") for a in proto.split(",")]      # noqa: E731
    tail = ["threshold", "keep_scale", "seed"]
    for old, new, extra in (("isplib_mha_csr_hip", ENTRIES[0], 3), ("isplib_mha_bw_rows_hip", ENTRIES[1], 3),
                            ("isplib_mha_bw_cols_hip", ENTRIES[2], 4)):
        was = names(re.search(old + r"\((.*?)\);", plain, re.S).group(1))
        now = names(re.search(new + r"\((.*?)\);", header, re.S).group(1))
        assert len(now) == len(was) + extra and now[-3:] == tail
        assert now[:-3] == (was if extra == 3 else was[:7] + ["csr2csc"] + was[7:]), new
        assert len(getattr(L, new).argtypes) == len(getattr(L, old).argtypes) + extra == len(now)
    src = open(os.path.join(ROOT, "isplib_amd", "csrc", "mha.hip")).read()
    assert '#include "gat_dropout.h"' in src and "fmix32" not in src.replace("one fmix32", "")          # one statement of the bit
    mk = open(os.path.join(ROOT, "isplib_amd", "csrc", "Makefile")).read()
    assert re.search(r"^HIP_SRCS\s*:=.*\bmha\.hip\b", mk, re.M) and "mha_drop.hip" not in mk


def test_the_operator_schema_is_registered():
    import isplib_amd  # noqa: F401
    schema = str(torch.ops.isplib.mha_drop_spmm.default._schema)
    assert schema == "isplib::" + SCHEMA, schema


def test_signatures_carry_the_three_keywords_with_their_defaults():
    import isplib_amd
    for fn in (isplib_amd.mha_matmul, isplib_amd.SparseTensor.mha_matmul):
        par = inspect.signature(fn).parameters
        assert [(n, par[n].default) for n in ("dropout", "training", "seed")] == [("dropout", 0.0), ("training", True), ("seed", None)]
        names = [n for n in par if n != "self"]
        assert names[-5:] == ["heads", "scale", "dropout", "training", "seed"]
    doc = isplib_amd.gat_dropout_mask.__doc__
    assert "both operators" in doc and "mha_matmul" in doc
    doc = isplib_amd.plugin.mha_matmul.__doc__
    assert "kernel ARGUMENT" in doc and "no 16-bit dropout kernel" in doc
    gap = re.search(r"Not part of the operator:(.*?)\.", doc, re.S).group(1)
    assert "dropout" not in gap and "edge features" in gap and "root weight" in gap and "beta" in gap


def _adj(m, n):
    import isplib_amd
    rowptr = torch.arange(0, m + 1, dtype=torch.int64)
    col = torch.arange(m, dtype=torch.int64) % n
    return isplib_amd.SparseTensor.from_csr(rowptr, col, None, (m, n))


def test_plugin_refuses_bad_dropout_and_seed_before_anything_touches_a_device(monkeypatch):
    import isplib_amd
    monkeypatch.delenv("ISPLIB_HALF_MHA", raising=False)
    adj = _adj(6, 4)
    q, k, v = torch.zeros(6, 16), torch.zeros(4, 16), torch.zeros(4, 16)      # CPU tensors: a launch is impossible
    for bad in (1.0, -0.1, float("nan"), 1.5, 2):
        with pytest.raises(ValueError, match="`dropout` must lie in"):
            isplib_amd.mha_matmul(adj, q, k, v, heads=2, dropout=bad)
        with pytest.raises(ValueError, match="`dropout` must lie in"):                # a bad value is refused in eval mode too
            adj.mha_matmul(q, k, v, 2, None, bad, False)
    for bad in (True, "0.5", None, torch.tensor(0.5), np.float32(0.5)):
        with pytest.raises(TypeError, match="`dropout` must be a Python float or int"):
            isplib_amd.mha_matmul(adj, q, k, v, heads=2, dropout=bad)
    for bad in (-1, 2 ** 63):
        with pytest.raises(ValueError, match="`seed` must lie in"):
            isplib_amd.mha_matmul(adj, q, k, v, heads=2, dropout=0.6, seed=bad)
    for bad in (True, 1.0, "1"):
        with pytest.raises(TypeError, match="`seed` must be an int"):
            adj.mha_matmul(q, k, v, 2, dropout=0.6, seed=bad)
    with pytest.raises(ValueError, match="`dropout` must lie in"):                    # before the operands are looked at
        isplib_amd.mha_matmul(adj, q.numpy(), k, v, heads=2, dropout=1.0)
    # well-formed dropout: the operand checks of the call without it, then the device check
    with pytest.raises(ValueError, match="same width"):
        isplib_amd.mha_matmul(adj, q, torch.zeros(4, 8), v, heads=2, dropout=0.6, seed=1)
    with pytest.raises(ValueError, match="power of two"):
        isplib_amd.mha_matmul(adj, torch.zeros(6, 12), torch.zeros(4, 12), torch.zeros(4, 12), heads=2, dropout=0.6)
    with pytest.raises(ValueError, match="`scale` must be a finite Python number"):
        isplib_amd.mha_matmul(adj, q, k, v, heads=2, scale=float("inf"), dropout=0.6)
    with pytest.raises(TypeError, match="float32"):                     # the variable is unset: 16-bit operands raise what they always raised
        isplib_amd.mha_matmul(adj, q.bfloat16(), k.bfloat16(), v.bfloat16(), heads=2, dropout=0.6)
    with pytest.raises(TypeError, match="GPU tensors"):
        isplib_amd.mha_matmul(adj, q, k, v, heads=2, dropout=0.6, seed=2 ** 63 - 1)
    monkeypatch.setenv("ISPLIB_HALF_MHA", "native")                     # 16-bit operands: the conversion route, which raises what the fp32 call raises
    with pytest.raises(TypeError, match="GPU tensors"):
        adj.mha_matmul(q.bfloat16(), k.bfloat16(), v.bfloat16(), 2, dropout=0.6, seed=3)
    with pytest.raises(TypeError, match="share one 16-bit dtype"):
        adj.mha_matmul(q.bfloat16(), k.bfloat16(), v.half(), 2, dropout=0.6)


class _Flagged(torch.Tensor):                                           # CPU tensors that claim to be on the GPU: nothing is launched
    is_cuda = True


def _fake_ops(monkeypatch, calls):
    from isplib_amd import plugin

    class Ops:
        @staticmethod
        def mha_spmm(*args):
            calls.append(("mha_spmm", args))
            return "z"

        @staticmethod
        def mha_drop_spmm(*args):
            calls.append(("mha_drop_spmm", args))
            return "zd"

    class FakeTorchOps:
        isplib = Ops

    monkeypatch.setattr(plugin.torch, "ops", FakeTorchOps)
    adj = _adj(6, 6)
    st = adj.storage
    st._colptr, st._csr2csc, st._row_t = torch.zeros(7, dtype=torch.int64), torch.arange(6), torch.arange(6)    # the cached transpose
    K = 16
    fused = torch.zeros(6, 3 * K).as_subclass(_Flagged)
    return adj, st, fused[:, :K], fused[:, K:2 * K], fused[:, 2 * K:]


def test_no_dropout_and_eval_mode_take_the_old_call_path(monkeypatch):
    import isplib_amd
    monkeypatch.delenv("ISPLIB_HALF_MHA", raising=False)
    calls = []
    adj, st, q, k, v = _fake_ops(monkeypatch, calls)
    state = torch.get_rng_state()
    assert isplib_amd.mha_matmul(adj, q, k, v, heads=2, scale=0.25, dropout=0.0) == "z"
    assert adj.mha_matmul(q, k, v, 2, 0.25, 0.6, False) == "z"
    assert adj.mha_matmul(q, k, v, 2, 0.25, dropout=0, training=True, seed=5) == "z"
    assert adj.mha_matmul(q, k, v, 2, 0.25, dropout=0.6, training=False, seed=5) == "z"
    assert adj.mha_matmul(q, k, v, 2, 0.25) == "z"
    assert len(calls) == 5
    for name, args in calls:
        assert name == "mha_spmm" and len(args) == 9 and args[4] is q and args[5] is k and args[6] is v and args[7:] == (2, 0.25)
    assert torch.equal(torch.get_rng_state(), state)                    # and no seed was drawn
    del calls[:]
    # with dropout: the new operator, csr2csc before the dense operands -- the views themselves, no copy --, then the head scale, p, seed
    assert adj.mha_matmul(q, k, v, 2, 0.25, 0.6, True, 77) == "zd"
    assert isplib_amd.mha_matmul(adj, q, k, k, heads=2, dropout=0.25, seed=2 ** 63 - 1) == "zd"
    (n1, a1), (n2, a2) = calls
    assert n1 == n2 == "mha_drop_spmm" and len(a1) == len(a2) == 12
    assert a1[0] is st._rowptr and a1[1] is st._col and a1[2] is st._colptr and a1[3] is st._row_t and a1[4] is st._csr2csc
    assert a1[5] is q and a1[6] is k and a1[7] is v and a1[8:] == (2, 0.25, 0.6, 77)
    assert [t.stride(0) for t in a1[5:8]] == [48] * 3 and [t.storage_offset() for t in a1[5:8]] == [0, 16, 32]
    assert a2[6] is k and a2[7] is k and a2[8:] == (2, 1.0 / math.sqrt(8), 0.25, 2 ** 63 - 1)


def test_a_seed_of_none_is_drawn_from_the_default_generator_and_repeats_under_manual_seed(monkeypatch):
    calls = []
    adj, st, q, k, v = _fake_ops(monkeypatch, calls)
    torch.manual_seed(1234)
    adj.mha_matmul(q, k, v, 2, dropout=0.6)
    adj.mha_matmul(q, k, v, 2, dropout=0.6)
    torch.manual_seed(1234)
    adj.mha_matmul(q, k, k, heads=2, dropout=0.6)
    seeds = [args[11] for _, args in calls]
    assert all(type(s) is int and 0 <= s < 2 ** 63 for s in seeds)
    assert seeds[0] == seeds[2] and seeds[0] != seeds[1]


def test_ctypes_wrappers_refuse_bad_operands_before_the_call():
    from isplib_amd import cabi
    rowptr, col = torch.arange(0, 7, dtype=torch.int64), torch.arange(6, dtype=torch.int64) % 4
    colptr, pos = torch.arange(0, 5, dtype=torch.int64), torch.arange(6, dtype=torch.int64)
    q, k, v, g = torch.zeros(6, 16), torch.zeros(4, 16), torch.zeros(4, 16), torch.zeros(6, 16)
    lse = torch.zeros(6, 2)
    T, c = cabi.gat_drop_threshold(0.6), cabi.gat_drop_scale(0.6)
    for bad in (-1, 2 ** 32, True, 0.5):
        with pytest.raises(ValueError, match="`threshold` must be an int"):
            cabi.mha_drop(rowptr, col, q, k, v, bad, c, 1, 2)
    for bad in (0.0, -1.0, float("inf"), float("nan"), True, "2.5"):
        with pytest.raises(ValueError, match="`keep_scale` must be a positive finite number"):
            cabi.mha_drop(rowptr, col, q, k, v, T, bad, 1, 2)
        with pytest.raises(ValueError, match="`keep_scale` must be a positive finite number"):
            cabi.mha_drop_bw_cols(colptr, col, pos, q, k, v, g, lse, lse, T, bad, 1, 2)
    for bad in (-1, 2 ** 63, True, 1.0):
        with pytest.raises(ValueError, match="`seed` must be an int"):
            cabi.mha_drop_bw_rows(rowptr, col, q, k, v, g, g, lse, T, c, bad, 2)
    # the pre-call checks of cabi.mha*
    with pytest.raises(TypeError, match="float32"):
        cabi.mha_drop(rowptr, col, q, k.to(torch.bfloat16), v, T, c, 1, 2)
    with pytest.raises(ValueError, match=r"`v` must be \[4, 16\]"):
        cabi.mha_drop(rowptr, col, q, k, torch.zeros(4, 8), T, c, 1, 2)
    with pytest.raises(ValueError, match="`scale` must be a finite number"):
        cabi.mha_drop(rowptr, col, q, k, v, T, c, 1, 2, float("nan"))
    with pytest.raises(ValueError, match="isplib_gat_serves"):
        cabi.mha_drop(rowptr, col, torch.zeros(6, 12), torch.zeros(4, 12), torch.zeros(4, 12), T, c, 1, 2)      # d = 6
    with pytest.raises(ValueError, match="GPU tensor"):
        cabi.mha_drop(rowptr, col, q, k, v, T, c, 1, 2)                          # well-formed, but on the CPU
    with pytest.raises(ValueError, match=r"`lse` must be \[6, 2\]"):
        cabi.mha_drop_bw_rows(rowptr, col, q, k, v, g, g, torch.zeros(5, 2), T, c, 1, 2)
    with pytest.raises(ValueError, match="GPU tensor"):
        cabi.mha_drop_bw_rows(rowptr, col, q, k, v, g, g, lse, T, c, 1, 2)
    with pytest.raises(ValueError, match=r"`dsum` must be \[6, 2\]"):
        cabi.mha_drop_bw_cols(colptr, col, pos, q, k, v, g, lse, torch.zeros(6, 1), T, c, 1, 2)
    with pytest.raises((ValueError, TypeError), match="csr2csc"):
        cabi.mha_drop_bw_cols(colptr, col, None, q, k, v, g, lse, lse, T, c, 1, 2)
    with pytest.raises((ValueError, TypeError), match="csr2csc"):
        cabi.mha_drop_bw_cols(colptr, col, pos[:5], q, k, v, g, lse, lse, T, c, 1, 2)
    with pytest.raises(ValueError, match="GPU tensor"):
        cabi.mha_drop_bw_cols(colptr, col, pos, q, k, v, g, lse, lse, T, c, 1, 2)
