"""GAT aggregation with a per-edge score term, host side (no GPU): tests/gat_edge_ref.py reduces to tests/gat_ref.py at a_edge = 0, its
gradients (d a_edge included) are those of central differences of its own forward and of torch's autograd through the plain
composition, every case of tests/gat_edge_cases.py builds inside the first-order range, the Python mirror of the new domain rule agrees
with the header's and the exported symbol's, the three new entries resolve, and the plug-in refuses a bad `a_edge` before anything
touches a device -- while `a_edge=None` stays the call it was.
"""
import os
import re

import numpy as np
import pytest
import torch

from tests import gat_cases
from tests import gat_edge_cases as cases
from tests import gat_edge_ref as ref
from tests import gat_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUTPUTS = ("z", "lse", "D", "dadst", "dasrc", "dy")


def test_every_case_builds_inside_the_first_order_range():
    built = cases.all_cases()
    assert len(built) == len(cases.CONFIGS) + 6 + 5
    for case in built:
        assert float(case.bound["rho"].max()) <= ref.RHO_MAX, case.name
        assert case.a_edge.shape == (case.nnz, case.heads) and case.ref["daedge"].shape == (case.nnz, case.heads)
    assert [(c.heads, c.k // c.heads) for c in cases.config_cases()] == list(gat_cases.CONFIGS)
    assert {(c.heads, c.k // c.heads, c.ns) for c in cases.slope_cases()} == {(h, d, ns) for h, d in cases.SLOPE_CONFIGS for ns in (0.0, 1.0)}
    only = cases.edge_only_case()
    assert not only.a_dst.any() and not only.a_src.any() and only.a_edge.any()
    rect = cases.rect_case()
    assert rect.m != rect.n and rect.a_dst.shape[0] == rect.m and rect.a_src.shape[0] == rect.n
    dup = cases.duplicate_case()
    e1, e2 = dup.pairs[0]
    assert dup.ref["row"][e1] == dup.ref["row"][e2] and dup.col[e1] == dup.col[e2] and np.all(dup.a_edge[e1] != dup.a_edge[e2])
    large = cases.large_case()
    spread = np.zeros(large.m)
    np.maximum.at(spread, large.ref["row"], np.abs(large.ref["u"]).max(1))
    assert (spread > 100).sum() > large.m // 4                          # in real rows, not in one
    # the fp32 branch really differs from the exact sign nowhere by much: where it differs, |u| is rounding noise of the two adds
    for case in built:
        flip = case.ref["pos"] != (case.ref["u"] > 0)
        assert np.all(np.abs(case.ref["u"][flip]) <= ref.EPS * (np.abs(case.ref["u0"][flip]) + 2 * np.abs(case.ref["u"][flip])) + 1e-45)


@pytest.mark.parametrize("heads,d,ns", ((1, 7, 0.2), (8, 8, 0.0), (3, 128, 1.0), (8, 64, 0.2)))
def test_zero_edge_term_is_the_reference_without_it(heads, d, ns):
    base = gat_cases.config_case(heads, d, ns)
    zero = np.zeros((base.col.size, heads), np.float32)
    got = ref.gat_edge(base.rowptr, base.col, base.y, base.a_dst, base.a_src, zero, heads, ns, base.g)
    for name in OUTPUTS + ("u", "s", "a", "t", "ds", "du"):
        assert np.array_equal(got[name], base.ref[name]), name
    assert np.array_equal(got["daedge"], base.ref["du"])
    bound = ref.bounds(base.rowptr, base.col, base.y, base.a_dst, base.a_src, zero, heads, ns, got, base.g)
    for name in OUTPUTS:                                                # three roundings instead of two: never tighter than gat_ref's
        assert np.all(bound[name] >= base.bound[name]), name


def _small(heads, d, ns, seed):
    """A 6-row graph with a duplicate and an empty row; every |u_e| >= 0.25, so no probe of 1e-6 crosses the kink."""
    rng = np.random.default_rng(seed)
    rowptr = np.array([0, 3, 3, 5, 9, 10, 12], dtype=np.int64)
    col = np.array([1, 4, 1, 0, 2, 3, 3, 0, 2, 4, 1, 0], dtype=np.int64)
    n = 5
    y = rng.standard_normal((n, heads * d)).astype(np.float32)
    g = rng.standard_normal((6, heads * d)).astype(np.float32)
    a_dst = rng.standard_normal((6, heads)).astype(np.float32)
    a_src = rng.standard_normal((n, heads)).astype(np.float32)
    a_edge = rng.standard_normal((col.size, heads)).astype(np.float32)
    row = ref.edge_rows(rowptr)
    u = a_dst[row] + a_src[col] + a_edge
    a_edge = np.where(np.abs(u) < 0.25, a_edge + np.sign(u + 1e-9).astype(np.float32), a_edge).astype(np.float32)
    assert np.abs(a_dst[row].astype(np.float64) + a_src[col] + a_edge).min() >= 0.25
    return rowptr, col, y, a_dst, a_src, a_edge, g


@pytest.mark.parametrize("heads,d,ns", ((1, 3, 0.2), (2, 4, 0.2), (2, 4, 0.0)))
def test_reference_gradients_are_central_differences_of_its_forward(heads, d, ns):
    rowptr, col, y, a_dst, a_src, a_edge, g = _small(heads, d, ns, 11 * heads + d)
    got = ref.gat_edge(rowptr, col, y, a_dst, a_src, a_edge, heads, ns, g)
    g64, h = g.astype(np.float64), 1e-6

    def loss(yy, dst, src, edge):
        """<g, z> with fp64 operands: the branch is still the fp32 one of the unperturbed operands (no probe crosses the kink)."""
        row = got["row"]
        u = dst[row] + src[col] + edge
        s = np.where(got["pos"], u, ns * u)
        w = np.exp(s - s.max())
        den = ref.segment_sum(w, row, rowptr.size - 1)
        a = w / den[row]
        z = ref.segment_sum(a[:, :, None] * ref.per_head(yy, heads)[col], row, rowptr.size - 1)
        return float((ref.per_head(g64, heads) * z).sum())

    ops = [a.astype(np.float64) for a in (y, a_dst, a_src, a_edge)]
    assert abs(loss(*ops) - float((g64 * got["z"]).sum())) <= 1e-12
    for which, name in ((0, "dy"), (1, "dadst"), (2, "dasrc"), (3, "daedge")):
        want = np.zeros_like(ops[which])
        for idx in np.ndindex(*want.shape):
            up, down = [a.copy() for a in ops], [a.copy() for a in ops]
            up[which][idx] += h
            down[which][idx] -= h
            want[idx] = (loss(*up) - loss(*down)) / (2 * h)
        assert np.abs(want - got[name].reshape(want.shape)).max() <= 1e-7 * max(1.0, np.abs(want).max()), name


def test_reference_equals_torch_autograd_of_the_composition():
    """index, add, leaky_relu, a scatter softmax written with index_add_, a weighted sum -- in fp64 on the CPU, under autograd."""
    case = cases.config_case(8, 8)
    heads, d, ns = case.heads, case.k // case.heads, case.ns
    row, col = torch.from_numpy(case.ref["row"]), torch.from_numpy(np.array(case.col))
    y, a_dst, a_src, a_edge = (torch.from_numpy(np.array(a)).double().requires_grad_(True) for a in (case.y, case.a_dst, case.a_src, case.a_edge))
    u = a_dst[row] + a_src[col] + a_edge
    assert np.array_equal((u.detach().numpy() > 0), case.ref["pos"])       # no edge of this case sits on the kink's rounding noise
    s = torch.nn.functional.leaky_relu(u, ns)
    top = np.full((case.m, heads), -np.inf)
    np.maximum.at(top, row.numpy(), s.detach().numpy())
    top = torch.from_numpy(top)
    w = torch.exp(s - top[row])
    den = torch.zeros(case.m, heads, dtype=torch.float64).index_add_(0, row, w)
    a = w / den[row]
    z = torch.zeros(case.m, heads, d, dtype=torch.float64).index_add_(0, row, a[:, :, None] * y.view(case.n, heads, d)[col]).view(case.m, heads * d)
    z.backward(torch.from_numpy(np.array(case.g)).double())
    for name, got in (("z", z.detach().numpy()), ("dy", y.grad.numpy()), ("dadst", a_dst.grad.numpy()), ("dasrc", a_src.grad.numpy()),
                      ("daedge", a_edge.grad.numpy())):
        scale = max(np.abs(case.ref[name]).max(), np.abs(case.ref["du"]).max() if name.startswith("da") else 0.0)
        assert np.abs(got - case.ref[name]).max() <= 1e-10 * scale, name


def test_domain_rule_at_every_edge():
    from isplib_amd import cabi
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "isplib_hip.h")).read(), flags=re.S)
    assert "isplib_gat_edge_serves" in header
    L = cabi.lib()
    top = cabi.DENSE_BYTES_MAX // 4                                    # floats behind one descriptor
    assert cabi.DENSE_BYTES_MAX == 0xE0000000
    table = ((10, 0, False), (10, -1, False), (10, 1, True), (0, 1, True), (0, 0, False), (-1, 1, False),
             (2 ** 31 - 1, 1, False), (2 ** 31, 1, False), (2 ** 40, 1, False),    # with heads >= 1 the byte rule refuses both before nnz < 2^31 does
             (top // 128, 128, True), (top // 128 + 1, 128, False),         # the last admitted product and the first refused
             (top // 8, 8, True), (top // 8 + 1, 8, False), (top, 1, True), (top + 1, 1, False), (2 ** 31 - 1, 2, False),
             (1, top, True), (1, top + 1, False), (2 ** 40, 2 ** 40, False))
    for nnz, heads, want in table:
        assert cabi.gat_edge_serves(nnz, heads) is want, (nnz, heads)
        assert bool(L.isplib_gat_edge_domain(nnz, heads)) is want, (nnz, heads)
    assert (top // 128) * 128 * 4 <= cabi.DENSE_BYTES_MAX < (top // 128 + 1) * 128 * 4


def test_the_new_entries_resolve_and_the_abi_version_stays_1():
    from isplib_amd import cabi
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "isplib_hip.h")).read(), flags=re.S)
    L = cabi.lib()
    for name in ("isplib_gat_edge_csr_hip", "isplib_gat_edge_bw_rows_hip", "isplib_gat_edge_bw_cols_hip", "isplib_gat_edge_domain"):
        assert name in cabi.EXPORTS and re.search(r"\b%s\s*\(" % name, header), name
        assert getattr(L, name) is not None
    assert int(re.search(r"#define\s+ISPLIB_HIP_ABI_VERSION\s+(\d+)", header).group(1)) == 1
    assert L.isplib_hip_abi_version() == 1
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in ("isplib_gat_edge_csr_hip", "isplib_gat_edge_bw_rows_hip", "isplib_gat_edge_bw_cols_hip", "isplib_gat_edge_domain"):
        assert name in integration, name


def _adj(m, n):
    import isplib_amd
    rowptr = torch.arange(0, m + 1, dtype=torch.int64)
    col = torch.arange(m, dtype=torch.int64) % n
    return isplib_amd.SparseTensor.from_csr(rowptr, col, None, (m, n))


def test_plugin_refuses_a_bad_edge_term_before_anything_touches_a_device(monkeypatch):
    import isplib_amd
    monkeypatch.delenv("ISPLIB_HALF_GAT", raising=False)
    adj = _adj(6, 4)                                                    # nnz = 6
    y, a_dst, a_src, a_edge = torch.zeros(4, 16), torch.zeros(6, 2), torch.zeros(4, 2), torch.zeros(6, 2)
    with pytest.raises(TypeError, match="`a_edge` must be a tensor"):
        isplib_amd.gat_matmul(adj, y, a_dst, a_src, heads=2, a_edge=a_edge.numpy())
    for dt in (torch.float64, torch.bfloat16, torch.float16, torch.int64):
        with pytest.raises(TypeError, match="`a_edge` must be float32"):
            isplib_amd.gat_matmul(adj, y, a_dst, a_src, heads=2, a_edge=a_edge.to(dt))
    for dt in (torch.bfloat16, torch.float16):                          # a 16-bit y stays the TypeError it always was without the variable
        with pytest.raises(TypeError, match="float32"):
            adj.gat_matmul(y.to(dt), a_dst, a_src, 2, a_edge=a_edge)
    for bad in (torch.zeros(5, 2), torch.zeros(6, 1), torch.zeros(6, 3), torch.zeros(6), torch.zeros(2, 6), torch.zeros(6, 2, 1), torch.zeros(4, 2)):
        with pytest.raises(ValueError, match=r"`a_edge` must be \[6, 2\]"):
            isplib_amd.gat_matmul(adj, y, a_dst, a_src, heads=2, a_edge=bad)
    with pytest.raises(ValueError, match=r"`a_edge` must be \[6, 1\]"):
        adj.gat_matmul(y, a_dst[:, 0], a_src[:, 0], a_edge=torch.zeros(5))                 # [nnz] with one head, but the wrong nnz
    with pytest.raises(ValueError, match=r"`a_dst` must be \[6, 2\]"):
        isplib_amd.gat_matmul(adj, y, a_dst[:-1], a_src, heads=2, a_edge=a_edge)
    with pytest.raises(ValueError, match="positive int"):
        isplib_amd.gat_matmul(adj, y, a_dst, a_src, heads=0, a_edge=a_edge)
    with pytest.raises(ValueError, match="power of two"):
        isplib_amd.gat_matmul(adj, torch.zeros(4, 12), a_dst, a_src, heads=2, a_edge=a_edge)
    with pytest.raises(TypeError, match="GPU tensor"):                                     # well-formed, but on the CPU
        isplib_amd.gat_matmul(adj, y, a_dst, a_src, heads=2, a_edge=a_edge)
    with pytest.raises(TypeError, match="GPU tensor"):
        adj.gat_matmul(y, a_dst[:, 0], a_src[:, 0], a_edge=torch.zeros(6))                 # [nnz] with one head is well-formed
    with pytest.raises(TypeError, match="GPU tensor"):
        adj.gat_matmul(y, a_dst, a_src, 2, 0.2, a_edge.t().contiguous().t())               # non-contiguous is well-formed (copied later)
    # with the variable set, a 16-bit y takes the conversion route: a_edge float32 or of y's dtype, anything else refused
    monkeypatch.setenv("ISPLIB_HALF_GAT", "native")
    with pytest.raises(TypeError, match="float32 or of `y`'s dtype"):
        adj.gat_matmul(y.bfloat16(), a_dst, a_src, 2, a_edge=a_edge.half())
    with pytest.raises(TypeError, match="GPU tensor"):
        adj.gat_matmul(y.bfloat16(), a_dst, a_src, 2, a_edge=a_edge.bfloat16())


def test_the_domain_refusal_names_the_limit_and_the_way_out(monkeypatch):
    import isplib_amd
    from isplib_amd import cabi, plugin
    adj = _adj(6, 4)
    monkeypatch.setattr(cabi, "gat_edge_serves", lambda nnz, heads: False)
    with pytest.raises(ValueError, match=r"isplib_gat_edge_serves.*3\.5 GiB.*fewer heads per call, on column views of `y`"):
        plugin.gat_matmul(adj, torch.zeros(4, 16), torch.zeros(6, 2), torch.zeros(4, 2), heads=2, a_edge=torch.zeros(6, 2))
    with pytest.raises(ValueError, match=r"isplib_gat_edge_serves.*fewer"):
        cabi._gat_edge_domain(2 ** 31, 1)
    assert isplib_amd.gat_matmul is plugin.gat_matmul


def test_no_edge_term_reaches_gat_spmm_as_before(monkeypatch):
    """a_edge=None is the call it was: the same operator with the same nine arguments; with a_edge the new operator, csr2csc included."""
    import isplib_amd
    from isplib_amd import plugin
    calls = []

    class Ops:
        @staticmethod
        def gat_spmm(*args):
            calls.append(("gat_spmm", args))
            return "z"

        @staticmethod
        def gat_edge_spmm(*args):
            calls.append(("gat_edge_spmm", args))
            return "ze"

    class FakeTorchOps:
        isplib = Ops

    class Flagged(torch.Tensor):                                       # CPU tensors that claim to be on the GPU: nothing is launched
        is_cuda = True

    monkeypatch.setattr(plugin.torch, "ops", FakeTorchOps)
    adj = _adj(6, 4)
    st = adj.storage
    st._colptr, st._csr2csc, st._row_t = torch.zeros(5, dtype=torch.int64), torch.arange(6), torch.arange(6)    # the cached transpose
    y, a_dst, a_src = (t.as_subclass(Flagged) for t in (torch.zeros(4, 16), torch.zeros(6, 2), torch.zeros(4, 2)))
    a_edge = torch.zeros(2, 6).t().as_subclass(Flagged)
    assert isplib_amd.gat_matmul(adj, y, a_dst, a_src, heads=2, negative_slope=0.1) == "z"
    assert adj.gat_matmul(y, a_dst, a_src, 2, 0.1, None) == "z"
    for name, args in calls:
        assert name == "gat_spmm" and len(args) == 9 and args[4] is y and args[5] is a_dst and args[6] is a_src and args[7:] == (2, 0.1)
        assert args[0] is st._rowptr and args[1] is st._col and args[2] is st._colptr and args[3] is st._row_t
    del calls[:]
    assert adj.gat_matmul(y, a_dst, a_src, 2, 0.1, a_edge) == "ze"
    (name, args), = calls
    assert name == "gat_edge_spmm" and len(args) == 11 and args[4] is st._csr2csc and args[5] is y and args[9:] == (2, 0.1)
    assert args[8].is_contiguous() and tuple(args[8].shape) == (6, 2)                      # the non-contiguous a_edge was copied
