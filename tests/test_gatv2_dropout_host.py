"""GATv2 aggregation with attention dropout, without a GPU: the reference of tests/gatv2_dropout_ref.py against a torch fp64 autograd
composition and against central differences, its cases, the argument checks of gatv2_matmul(..., dropout=, training=, seed=) -- all
raised before anything touches a device -- the call paths, and the new exports and operator schema.
"""
import inspect
import os
import re

import numpy as np
import pytest
import torch

from tests import gatv2_cases
from tests import gatv2_dropout_cases as cases
from tests import gatv2_dropout_ref as ref
from tests import gatv2_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("isplib_gatv2_drop_csr_hip", "isplib_gatv2_drop_bw_rows_hip", "isplib_gatv2_drop_bw_cols_hip")
OUTPUTS = ("z", "lse", "D", "dx", "dy", "datt")
SCHEMA = ("gatv2_drop_spmm(Tensor rowptr, Tensor col, Tensor colptr, Tensor row_t, Tensor csr2csc, Tensor x, Tensor y, Tensor att, "
          "int heads, float negative_slope, float p, int seed) -> Tensor")


@pytest.mark.parametrize("heads,d,p", ((8, 8, 0.6), (1, 47, 0.6)))
def test_reference_equals_torch_autograd_of_the_pyg_composition_with_the_same_mask(heads, d, p):
    """leaky_relu(x_i + x_j), the att contraction, a scatter softmax written with index_add_, mask * c ON THE COEFFICIENTS, a weighted
    sum -- fp64 on the CPU, under autograd; the mask is isplib_amd.gat_dropout_mask."""
    import isplib_amd
    case = cases.config_case(heads, d, 0.2, p)
    ns = case.ns
    row, col = torch.from_numpy(case.ref["row"]), torch.from_numpy(np.array(case.col))
    x, y, att = (torch.from_numpy(np.array(a)).double().requires_grad_(True) for a in (case.x, case.y, case.att))
    e = torch.nn.functional.leaky_relu(x.view(case.m, heads, d)[row] + y.view(case.n, heads, d)[col], ns)
    s = (e * att.view(1, heads, d)).sum(-1)
    top = np.full((case.m, heads), -np.inf)
    np.maximum.at(top, row.numpy(), s.detach().numpy())
    w = torch.exp(s - torch.from_numpy(top)[row])
    den = torch.zeros(case.m, heads, dtype=torch.float64).index_add_(0, row, w)
    mask = isplib_amd.gat_dropout_mask(case.nnz, heads, case.p, case.seed)
    assert np.array_equal(mask.numpy(), case.ref["q"])
    a = (w / den[row]) * mask.double() * float(np.float32(1.0 / (1.0 - case.p)))
    z = torch.zeros(case.m, heads, d, dtype=torch.float64).index_add_(0, row, a[:, :, None] * y.view(case.n, heads, d)[col]).view(case.m, heads * d)
    z.backward(torch.from_numpy(np.array(case.g)).double())
    for name, got in (("z", z.detach()), ("dx", x.grad), ("dy", y.grad), ("datt", att.grad)):
        want = case.ref[name]
        assert np.abs(got.numpy() - want).max() <= 1e-9 * np.abs(want).max(), name


def _small(heads, d, seed):
    """A 12-row graph with an empty row, a duplicate, a one-entry row; every |u_ec| >= 0.05 so that no probe of 1e-6 crosses the kink."""
    rng = np.random.default_rng(seed)
    deg = np.array([3, 0, 2, 4, 1, 2, 5, 1, 3, 2, 0, 4], dtype=np.int64)
    rowptr = np.zeros(13, dtype=np.int64)
    np.cumsum(deg, out=rowptr[1:])
    n = 9
    col = rng.integers(0, n, size=int(rowptr[-1]))
    col[1] = col[0]                                                       # a duplicated (i, j)
    k = heads * d
    x = rng.standard_normal((12, k)).astype(np.float32)
    y = rng.standard_normal((n, k)).astype(np.float32)
    row = ref.edge_rows(rowptr)
    for _ in range(200):
        u = x[row].astype(np.float64) + y[col]
        near = np.abs(u) < 0.05
        if not near.any():
            break
        e, c = np.argwhere(near)[0]
        x[row[e], c] += np.float32(0.21)
    assert np.abs(x[row].astype(np.float64) + y[col]).min() >= 0.05
    att = rng.standard_normal((heads, d)).astype(np.float32)
    return rowptr, col, x, y, att, rng.standard_normal((12, k)).astype(np.float32)


@pytest.mark.parametrize("heads,d,ns,p", ((1, 3, 0.2, 0.5), (2, 4, 0.2, 0.6), (2, 4, 0.0, 0.3)))
def test_reference_gradients_are_central_differences_of_its_forward(heads, d, ns, p):
    rowptr, col, x, y, att, g = _small(heads, d, 13 * heads + d)
    seed = 9
    got = ref.gatv2_drop(rowptr, col, x, y, att, heads, ns, p, seed, g)
    assert got["q"].any() and not got["q"].all()
    g64, h, qc, row, m = g.astype(np.float64), 1e-6, got["qc"], got["row"], rowptr.size - 1

    def loss(xx, yy, aa):
        """<g, z> with fp64 operands, the mask and c fixed: the softmax over all entries, the mask on the coefficients."""
        u = ref.per_head(xx, heads)[row] + ref.per_head(yy, heads)[col]
        s = (aa.reshape(1, heads, d) * np.where(u > 0, u, ns * u)).sum(2)
        w = np.exp(s - s.max())
        a = qc * w / ref.segment_sum(w, row, m)[row]
        z = ref.segment_sum(a[:, :, None] * ref.per_head(yy, heads)[col], row, m)
        return float((ref.per_head(g64, heads) * z).sum())

    ops = [a.astype(np.float64) for a in (x, y, att)]
    assert abs(loss(*ops) - float((g64 * got["z"]).sum())) <= 1e-12
    for which, name in ((0, "dx"), (1, "dy"), (2, "datt")):
        want = np.zeros_like(ops[which])
        for idx in np.ndindex(*want.shape):
            up, down = [a.copy() for a in ops], [a.copy() for a in ops]
            up[which][idx] += h
            down[which][idx] -= h
            want[idx] = (loss(*up) - loss(*down)) / (2 * h)
        assert np.abs(want - got[name].reshape(want.shape)).max() <= 1e-7 * max(1.0, np.abs(want).max()), name


@pytest.mark.parametrize("heads,d,ns", ((1, 7, 0.2), (8, 8, 0.0), (3, 128, 1.0), (8, 64, 0.2)))
def test_zero_probability_is_the_reference_without_dropout(heads, d, ns):
    assert ref.threshold(0.0) == 0 and ref.scale(0.0) == np.float32(1.0)
    base = gatv2_cases.config_case(heads, d, ns)
    got = ref.gatv2_drop(base.rowptr, base.col, base.x, base.y, base.att, heads, ns, 0.0, 77, base.g)
    assert got["q"].all()
    for name in OUTPUTS + ("u", "s", "a", "t", "ds"):
        assert np.array_equal(got[name], base.ref[name]), name
    bound = ref.bounds(base.rowptr, base.col, base.x, base.y, base.att, heads, ns, got, base.g)
    for name in OUTPUTS:                                                 # one more rounding on z and in dy: never tighter than without dropout
        assert np.all(bound[name] >= base.bound[name]), name
    assert np.array_equal(bound["dx"], base.bound["dx"]) and np.array_equal(bound["lse"], base.bound["lse"])
    assert gatv2_ref.per_head is ref.per_head


def test_every_case_builds_with_the_properties_its_tests_rely_on():
    built = cases.all_cases()
    assert len(built) == len(cases.CONFIGS) + 18 + 4 and len(cases.CONFIGS) == 19
    assert max(float(c.bound["rho"].max()) for c in built) <= ref.RHO_MAX
    for case in built:
        assert case.ref["lse"] is case.base.ref["lse"] and case.ref["a"] is case.base.ref["a"]       # the softmax does not see the mask
        assert case.ref["q"].any() and not case.ref["q"].all()
    assert {(c.heads, c.k // c.heads, c.ns, c.p) for c in cases.slope_cases()} == \
        {(h, d, ns, p) for h, d in cases.SLOPE_CONFIGS for ns in (0.2, 0.0, 1.0) for p in (0.1, 0.9)}
    heavy = cases.config_case(8, 8, 0.2, 0.9)
    gone = heavy.all_dropped()
    assert gone.any() and np.all(ref.per_head(heavy.ref["z"], 8)[gone] == 0) and np.all(np.isfinite(heavy.ref["lse"][gone]))
    single = cases.single_case()
    assert int(np.diff(single.rowptr).max()) == 1 and single.live.sum() == 160
    assert (single.kept_in[single.has_in] == 0).any() and (single.kept_in[single.has_in] > 0).any()
    dup = cases.duplicate_case()
    e1, e2 = dup.pairs[0]
    assert dup.ref["row"][e1] == dup.ref["row"][e2] and dup.col[e1] == dup.col[e2] and np.any(dup.ref["q"][e1] != dup.ref["q"][e2])
    assert dup.wide.any() and dup.rowptr[dup.row + 1] - dup.rowptr[dup.row] == 4
    assert cases.position_case().ref["q"].shape == (dup.nnz, 8)
    rect = cases.rect_case()
    assert (rect.m, rect.n) == (67, 233)


def test_the_new_entries_resolve_and_the_abi_version_stays_1():
    from isplib_amd import cabi
    main = open(os.path.join(ROOT, "include", "isplib_hip.h")).read()
    assert re.search(r'^#include "isplib_hip_gatv2_drop.h"$', main, re.M)
    assert "gatv2_drop_" not in re.sub(r"/\*.*?\*/", "", main, flags=re.S).replace("isplib_hip_gatv2_drop.h", "")    # declared there only
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "isplib_hip_gatv2_drop.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"^\s*int\s+(\w+)\s*\(", header, flags=re.M)))
    assert declared == sorted(ENTRIES) == sorted(cabi.GATV2_DROP_EXPORTS)
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    L = cabi.lib()
    for name in ENTRIES:
        assert name not in cabi.EXPORTS                                   # listed apart, as the 16-bit GATv2 entries are
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert getattr(L, name) is not None
        assert name in integration, name
    assert int(re.search(r"#define\s+ISPLIB_HIP_ABI_VERSION\s+(\d+)", main).group(1)) == 1
    assert L.isplib_hip_abi_version() == 1
    assert len(L.isplib_gatv2_drop_bw_cols_hip.argtypes) == len(L.isplib_gatv2_bw_cols_hip.argtypes) + 4
    assert '#include "gat_dropout.h"' in open(os.path.join(ROOT, "isplib_amd", "csrc", "gatv2.hip")).read()   # one statement of the bit


def test_the_operator_schema_is_registered():
    import isplib_amd  # noqa: F401
    schema = str(torch.ops.isplib.gatv2_drop_spmm.default._schema)
    assert schema == "isplib::" + SCHEMA, schema


def test_signatures_carry_the_three_keywords_with_their_defaults():
    import isplib_amd
    for fn in (isplib_amd.gatv2_matmul, isplib_amd.SparseTensor.gatv2_matmul):
        par = inspect.signature(fn).parameters
        assert [(n, par[n].default) for n in ("dropout", "training", "seed")] == [("dropout", 0.0), ("training", True), ("seed", None)]
        names = [n for n in par if n != "self"]
        assert names[-5:] == ["heads", "negative_slope", "dropout", "training", "seed"]
    assert "both operators" in isplib_amd.gat_dropout_mask.__doc__


def _adj(m, n):
    import isplib_amd
    rowptr = torch.arange(0, m + 1, dtype=torch.int64)
    col = torch.arange(m, dtype=torch.int64) % n
    return isplib_amd.SparseTensor.from_csr(rowptr, col, None, (m, n))


def test_plugin_refuses_bad_dropout_and_seed_before_anything_touches_a_device(monkeypatch):
    import isplib_amd
    monkeypatch.delenv("ISPLIB_HALF_GATV2", raising=False)
    adj = _adj(6, 4)
    x, y, att = torch.zeros(6, 16), torch.zeros(4, 16), torch.zeros(2, 8)      # CPU tensors: a launch is impossible
    for bad in (1.0, -0.1, float("nan"), 1.5, 2):
        with pytest.raises(ValueError, match="`dropout` must lie in"):
            isplib_amd.gatv2_matmul(adj, x, att, y, heads=2, dropout=bad)
        with pytest.raises(ValueError, match="`dropout` must lie in"):                # a bad value is refused in eval mode too
            adj.gatv2_matmul(x, att, y, 2, 0.2, bad, False)
    for bad in (True, "0.5", None, torch.tensor(0.5), np.float32(0.5)):
        with pytest.raises(TypeError, match="`dropout` must be a Python float or int"):
            isplib_amd.gatv2_matmul(adj, x, att, y, heads=2, dropout=bad)
    for bad in (-1, 2 ** 63):
        with pytest.raises(ValueError, match="`seed` must lie in"):
            isplib_amd.gatv2_matmul(adj, x, att, y, heads=2, dropout=0.6, seed=bad)
    for bad in (True, 1.0, "1"):
        with pytest.raises(TypeError, match="`seed` must be an int"):
            adj.gatv2_matmul(x, att, y, 2, dropout=0.6, seed=bad)
    # well-formed dropout: the operand checks of the call without it, then the device check
    with pytest.raises(ValueError, match=r"`att` must be \[2, 8\]"):
        isplib_amd.gatv2_matmul(adj, x, att[:, :4], y, heads=2, dropout=0.6, seed=1)
    with pytest.raises(ValueError, match="power of two"):
        isplib_amd.gatv2_matmul(adj, torch.zeros(6, 12), torch.zeros(2, 6), torch.zeros(4, 12), heads=2, dropout=0.6)
    with pytest.raises(ValueError, match="square"):
        isplib_amd.gatv2_matmul(adj, x, att, heads=2, dropout=0.6)
    with pytest.raises(TypeError, match="float32"):                     # the variable is unset: 16-bit operands raise what they always raised
        isplib_amd.gatv2_matmul(adj, x.bfloat16(), att, y.bfloat16(), heads=2, dropout=0.6)
    with pytest.raises(TypeError, match="GPU tensors"):
        isplib_amd.gatv2_matmul(adj, x, att, y, heads=2, dropout=0.6, seed=2 ** 63 - 1)
    monkeypatch.setenv("ISPLIB_HALF_GATV2", "native")                   # 16-bit operands: the conversion route, which raises what the fp32 call raises
    with pytest.raises(TypeError, match="GPU tensors"):
        adj.gatv2_matmul(x.bfloat16(), att, y.bfloat16(), 2, dropout=0.6, seed=3)
    with pytest.raises(TypeError, match="share one 16-bit dtype"):
        adj.gatv2_matmul(x.bfloat16(), att, y.half(), 2, dropout=0.6)


class _Flagged(torch.Tensor):                                           # CPU tensors that claim to be on the GPU: nothing is launched
    is_cuda = True


def _fake_ops(monkeypatch, calls):
    from isplib_amd import plugin

    class Ops:
        @staticmethod
        def gatv2_spmm(*args):
            calls.append(("gatv2_spmm", args))
            return "z"

        @staticmethod
        def gatv2_drop_spmm(*args):
            calls.append(("gatv2_drop_spmm", args))
            return "zd"

    class FakeTorchOps:
        isplib = Ops

    monkeypatch.setattr(plugin.torch, "ops", FakeTorchOps)
    adj = _adj(6, 6)
    st = adj.storage
    st._colptr, st._csr2csc, st._row_t = torch.zeros(7, dtype=torch.int64), torch.arange(6), torch.arange(6)    # the cached transpose
    x, y, att = (t.as_subclass(_Flagged) for t in (torch.zeros(6, 16), torch.ones(6, 16), torch.zeros(2, 8)))
    return adj, st, x, y, att


def test_no_dropout_and_eval_mode_take_the_old_call_path(monkeypatch):
    import isplib_amd
    monkeypatch.delenv("ISPLIB_HALF_GATV2", raising=False)
    calls = []
    adj, st, x, y, att = _fake_ops(monkeypatch, calls)
    state = torch.get_rng_state()
    assert isplib_amd.gatv2_matmul(adj, x, att, y, heads=2, negative_slope=0.1, dropout=0.0) == "z"
    assert adj.gatv2_matmul(x, att, y, 2, 0.1, 0.6, False) == "z"
    assert adj.gatv2_matmul(x, att, y, 2, 0.1, dropout=0, training=True, seed=5) == "z"
    assert adj.gatv2_matmul(x, att, y, 2, 0.1, dropout=0.6, training=False, seed=5) == "z"
    for name, args in calls:
        assert name == "gatv2_spmm" and len(args) == 9 and args[4] is x and args[5] is y and args[6] is att and args[7:] == (2, 0.1)
    assert torch.equal(torch.get_rng_state(), state)                    # and no seed was drawn
    del calls[:]
    # with dropout: the new operator, csr2csc before the dense operands, then p and the seed; y=None shares the one tensor
    assert adj.gatv2_matmul(x, att, y, 2, 0.1, 0.6, True, 77) == "zd"
    assert adj.gatv2_matmul(x, att, heads=2, negative_slope=0.1, dropout=0.25, seed=2 ** 63 - 1) == "zd"
    (n1, a1), (n2, a2) = calls
    assert n1 == n2 == "gatv2_drop_spmm" and len(a1) == len(a2) == 12
    assert a1[4] is st._csr2csc and a1[5] is x and a1[6] is y and a1[7] is att and a1[8:] == (2, 0.1, 0.6, 77)
    assert a2[5] is x and a2[6] is x and a2[8:] == (2, 0.1, 0.25, 2 ** 63 - 1)


def test_a_seed_of_none_is_drawn_from_the_default_generator_and_repeats_under_manual_seed(monkeypatch):
    calls = []
    adj, st, x, y, att = _fake_ops(monkeypatch, calls)
    torch.manual_seed(1234)
    adj.gatv2_matmul(x, att, y, 2, dropout=0.6)
    adj.gatv2_matmul(x, att, y, 2, dropout=0.6)
    torch.manual_seed(1234)
    adj.gatv2_matmul(x, att, heads=2, dropout=0.6)
    seeds = [args[11] for _, args in calls]
    assert all(type(s) is int and 0 <= s < 2 ** 63 for s in seeds)
    assert seeds[0] == seeds[2] and seeds[0] != seeds[1]
