"""GAT attention dropout, host side (no GPU): the keep bit's three statements agree (NumPy in tests/gat_dropout_ref.py, the library's
exported host functions, isplib_amd.gat_dropout_mask in torch integer operations); its statistics hold; tests/gat_dropout_ref.py
reduces to the references without dropout at p = 0, and its gradients are those of central differences of its own forward and of
torch's autograd through the composition with the same mask on the coefficients; the new entries resolve; and the plug-in checks
`dropout` and `seed` before anything touches a device, takes the old call path without dropout and draws a reproducible seed.
"""
import os
import re

import numpy as np
import pytest
import torch

from tests import gat_cases, gat_edge_cases, gat_edge_ref, gat_ref
from tests import gat_dropout_cases as cases
from tests import gat_dropout_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUTPUTS = ("z", "lse", "D", "dadst", "dasrc", "dy")
SEEDS = (0, 1, 2, 12345, 2 ** 63 - 1, 0x1E3779B97F4A7C15, 2 ** 32, 2 ** 32 + 1)
PS = (0.1, 0.5, 0.6, 0.9)
ENTRIES = ("isplib_gat_drop_csr_hip", "isplib_gat_drop_bw_rows_hip", "isplib_gat_drop_bw_cols_hip")
HOST_FUNCTIONS = ("isplib_gat_drop_threshold", "isplib_gat_drop_word")


def test_numpy_word_and_threshold_are_the_library_s():
    from isplib_amd import cabi
    rng = np.random.default_rng(2024)
    n = 100000
    seed = rng.integers(0, 2 ** 63, n, dtype=np.int64, endpoint=False)
    pos = rng.integers(0, 2 ** 31, n, dtype=np.int64)
    head = rng.integers(0, 128, n, dtype=np.int64)
    mine = ref.word(seed.astype(np.uint64), pos, head)
    L = cabi.lib()
    theirs = np.fromiter((L.isplib_gat_drop_word(int(s), int(p), int(h)) for s, p, h in zip(seed, pos, head)), dtype=np.uint32, count=n)
    assert np.array_equal(mine, theirs)
    for s in (0, 2 ** 63 - 1):
        for p in (0, 2 ** 31 - 1):
            for h in (0, 127):
                assert int(ref.word(s, p, h)) == cabi.gat_drop_word(s, p, h), (s, p, h)
    assert int(ref.word(0, 0, 0)) == 0                                  # fmix32(0) = 0: the one fixed point, harmless (one entry of one seed)
    for p, want in ((0.0, 0), (1e-10, 0), (0.5, 2 ** 31), (1.0 - 2.0 ** -33, 2 ** 32 - 1), (0.6, 2576980377)):
        assert ref.threshold(p) == cabi.gat_drop_threshold(p) == cabi.gat_drop_threshold_py(p) == want, p
    for p in rng.random(1000):
        assert ref.threshold(p) == cabi.gat_drop_threshold(float(p)) == cabi.gat_drop_threshold_py(float(p))
    for p in PS:
        assert np.float32(cabi.gat_drop_scale(p)) == ref.scale(p) and float(ref.scale(p)) == cabi.gat_drop_scale(p)


@pytest.mark.parametrize("seed", (0, 12345, 2 ** 63 - 1, 2 ** 32 + 1))
def test_numpy_keep_bits_are_those_of_gat_dropout_mask(seed):
    import isplib_amd
    for heads, p in ((1, 0.6), (8, 0.1), (128, 0.9), (5, 0.0)):
        nnz = 4099
        mask = isplib_amd.gat_dropout_mask(nnz, heads, p, seed)
        assert mask.dtype == torch.bool and tuple(mask.shape) == (nnz, heads) and mask.device.type == "cpu"
        assert np.array_equal(mask.numpy(), ref.keep(seed, nnz, heads, p)), (heads, p)
        if p == 0.0:
            assert bool(mask.all())
    adj = _adj(6, 4)
    assert np.array_equal(isplib_amd.gat_dropout_mask(adj, 2, 0.5, seed).numpy(), ref.keep(seed, 6, 2, 0.5))
    far = torch.arange(2 ** 31 - 8, 2 ** 31, dtype=torch.int64)          # the far end of the position's domain, through the same integer ops
    from isplib_amd import plugin
    entry = plugin._fmix32(far ^ (seed & 0xFFFFFFFF))
    assert np.array_equal(entry.numpy().astype(np.uint32), ref.fmix32(((far.numpy() ^ (seed & 0xFFFFFFFF)) & 0xFFFFFFFF).astype(np.uint32)))
    for bad in (dict(heads=0), dict(dropout=1.0), dict(dropout=True), dict(seed=-1), dict(seed=2 ** 63)):
        kw = dict(heads=2, dropout=0.5, seed=1)
        kw.update(bad)
        with pytest.raises(ValueError):
            isplib_amd.gat_dropout_mask(10, kw["heads"], kw["dropout"], kw["seed"])


@pytest.mark.parametrize("seed", SEEDS)
def test_keep_rates_and_correlations_stay_within_five_sigma(seed):
    """2^17 positions x 8 heads per seed, p in {0.1, 0.5, 0.6, 0.9}: the keep rate overall and per head against the binomial sigma, and
    the centred bits against copies of themselves shifted by one and 64 positions, one and four heads, and under seed +- 1 and
    seed ^ 2^32 (sigma = p (1 - p) / sqrt(count)).  The largest deviations are printed."""
    N, H = 2 ** 17, 8
    pos, head = np.arange(N, dtype=np.int64)[:, None], np.arange(H, dtype=np.int64)[None, :]
    words = ref.word(seed, pos, head)
    others = {name: ref.word(s, pos, head) for name, s in (("seed+1", seed + 1), ("seed-1", seed - 1), ("seed^2^32", seed ^ 2 ** 32))
              if 0 <= s < 2 ** 63}
    assert "seed^2^32" in others and len(others) >= 2
    worst_rate = worst_corr = 0.0
    for p in PS:
        T = np.uint32(ref.threshold(p))
        q = words >= T
        sig = np.sqrt(p * (1 - p))
        rates = [abs(q.mean() - (1 - p)) / (sig / np.sqrt(N * H))] + [abs(q[:, h].mean() - (1 - p)) / (sig / np.sqrt(N)) for h in range(H)]
        b = q.astype(np.float64) - (1 - p)
        pairs = {"pos+1": (b[1:], b[:-1]), "pos+64": (b[64:], b[:-64]), "head+1": (b[:, 1:], b[:, :-1]), "head+4": (b[:, 4:], b[:, :-4])}
        for name, w in others.items():
            pairs[name] = (b, (w >= T).astype(np.float64) - (1 - p))
        corrs = {name: abs((x * y).mean()) / (p * (1 - p) / np.sqrt(x.size)) for name, (x, y) in pairs.items()}
        worst_rate, worst_corr = max(worst_rate, max(rates)), max(worst_corr, max(corrs.values()))
        assert max(rates) <= 5.0, (seed, p, rates)
        assert max(corrs.values()) <= 5.0, (seed, p, corrs)
    print(f"gat dropout keep bit, seed {seed}: rate {worst_rate:.2f} sigma, correlation {worst_corr:.2f} sigma")


@pytest.mark.parametrize("heads,d,ns", ((1, 7, 0.2), (8, 8, 0.0), (3, 128, 1.0), (8, 64, 0.2)))
def test_zero_probability_is_the_reference_without_dropout(heads, d, ns):
    assert ref.threshold(0.0) == 0 and ref.scale(0.0) == np.float32(1.0)
    base = gat_cases.config_case(heads, d, ns)
    got = ref.gat_drop(base.rowptr, base.col, base.y, base.a_dst, base.a_src, None, heads, ns, 0.0, 77, base.g)
    assert got["q"].all()
    for name in OUTPUTS + ("u", "s", "a", "t", "ds", "du"):
        assert np.array_equal(got[name], base.ref[name]), name
    edge = gat_edge_cases.config_case(heads, d, ns)
    got = ref.gat_drop(edge.rowptr, edge.col, edge.y, edge.a_dst, edge.a_src, edge.a_edge, heads, ns, 0.0, 77, edge.g)
    for name in OUTPUTS + ("daedge", "u", "s", "a", "t", "ds", "du", "pos"):
        assert np.array_equal(got[name], edge.ref[name]), name
    again = gat_edge_ref.gat_edge(edge.rowptr, edge.col, edge.y, edge.a_dst, edge.a_src, edge.a_edge, heads, ns, edge.g)
    assert np.array_equal(again["z"], got["z"]) and gat_ref.per_head is ref.per_head
    bound = ref.bounds(edge.rowptr, edge.col, edge.y, edge.a_dst, edge.a_src, edge.a_edge, heads, ns, got, edge.g)
    for name in OUTPUTS + ("daedge",):                                   # one more rounding on z and dy: never tighter than without dropout
        assert np.all(bound[name] >= edge.bound[name]), name


def test_every_case_builds_inside_the_first_order_range():
    built = cases.all_cases()
    assert len(built) == len(cases.CONFIGS) + 18 + len(cases.EDGE_CONFIGS) + 3
    for case in built:
        assert float(case.bound["rho"].max()) <= ref.RHO_MAX, case.name
        assert np.array_equal(case.ref["lse"], case.base.ref["lse"]) and np.array_equal(case.ref["a"], case.base.ref["a"])   # the softmax does not see the mask
    assert {(c.heads, c.k // c.heads, c.ns, c.p) for c in cases.slope_cases()} == \
        {(h, d, ns, p) for h, d in cases.SLOPE_CONFIGS for ns in (0.2, 0.0, 1.0) for p in (0.1, 0.9)}
    dup = cases.duplicate_case()
    e1, e2 = dup.pairs[0]
    assert dup.ref["row"][e1] == dup.ref["row"][e2] and dup.col[e1] == dup.col[e2] and np.any(dup.ref["q"][e1] != dup.ref["q"][e2])
    assert dup.wide.any()
    single = cases.single_case()
    assert int(np.diff(single.rowptr).max()) == 1 and (single.kept_in[single.has_in] == 0).any()
    # a (row, head) whose entries are all dropped: z is exactly 0 in the reference too, and lse is finite
    q_rows = np.zeros((single.m, single.heads), np.int64)
    np.add.at(q_rows, single.ref["row"], single.ref["q"].astype(np.int64))
    dropped = single.live[:, None] & (q_rows == 0)
    assert dropped.any() and np.all(ref.per_head(single.ref["z"], single.heads)[dropped] == 0) and np.all(np.isfinite(single.ref["lse"][dropped]))
    rect = cases.rect_case()
    assert (rect.m, rect.n) == (67, 233)


def _small(heads, d, ns, seed, edge):
    """The 6-row graph of the edge term's host tests, restated: a duplicate and an empty row; every |u_e| >= 0.25, so no probe of 1e-6
    crosses the kink."""
    rng = np.random.default_rng(seed)
    rowptr = np.array([0, 3, 3, 5, 9, 10, 12], dtype=np.int64)
    col = np.array([1, 4, 1, 0, 2, 3, 3, 0, 2, 4, 1, 0], dtype=np.int64)
    n = 5
    y = rng.standard_normal((n, heads * d)).astype(np.float32)
    g = rng.standard_normal((6, heads * d)).astype(np.float32)
    a_dst = rng.standard_normal((6, heads)).astype(np.float32)
    a_src = rng.standard_normal((n, heads)).astype(np.float32)
    a_edge = rng.standard_normal((col.size, heads)).astype(np.float32) if edge else np.zeros((col.size, heads), np.float32)
    row = ref.edge_rows(rowptr)
    u = a_dst[row] + a_src[col] + a_edge
    a_edge = np.where(np.abs(u) < 0.25, a_edge + np.sign(u + 1e-9).astype(np.float32), a_edge).astype(np.float32)
    assert np.abs(a_dst[row].astype(np.float64) + a_src[col] + a_edge).min() >= 0.25
    return rowptr, col, y, a_dst, a_src, a_edge, g


@pytest.mark.parametrize("heads,d,ns,p", ((1, 3, 0.2, 0.5), (2, 4, 0.2, 0.6), (2, 4, 0.0, 0.3)))
def test_reference_gradients_are_central_differences_of_its_forward(heads, d, ns, p):
    rowptr, col, y, a_dst, a_src, a_edge, g = _small(heads, d, ns, 11 * heads + d, True)
    seed = 9
    got = ref.gat_drop(rowptr, col, y, a_dst, a_src, a_edge, heads, ns, p, seed, g)
    assert got["q"].any() and not got["q"].all()
    g64, h, qc = g.astype(np.float64), 1e-6, got["qc"]

    def loss(yy, dst, src, edge):
        """<g, z> with fp64 operands, the mask and c fixed: the softmax over all entries, the mask on the coefficients."""
        row = got["row"]
        u = dst[row] + src[col] + edge
        s = np.where(got["pos"], u, ns * u)
        w = np.exp(s - s.max())
        den = ref.segment_sum(w, row, rowptr.size - 1)
        a = qc * w / den[row]
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
    # without the per-edge term the same gradients come from the a_edge = None form
    zero = np.zeros_like(a_edge)
    rowptr, col, y, a_dst, a_src, _, g = _small(heads, d, ns, 11 * heads + d, False)
    with_zero = ref.gat_drop(rowptr, col, y, a_dst, a_src, zero, heads, ns, p, seed, g)
    without = ref.gat_drop(rowptr, col, y, a_dst, a_src, None, heads, ns, p, seed, g)
    for name in OUTPUTS:
        assert np.array_equal(with_zero[name], without[name]), name


@pytest.mark.parametrize("edge", (False, True))
def test_reference_equals_torch_autograd_of_the_composition_with_the_same_mask(edge):
    """index, add, leaky_relu, a scatter softmax written with index_add_, the mask times c ON THE COEFFICIENTS, a weighted sum -- in fp64
    on the CPU, under autograd."""
    case = cases.edge_case(8, 8) if edge else cases.config_case(8, 8)
    heads, d, ns = case.heads, case.k // case.heads, case.ns
    row, col = torch.from_numpy(case.ref["row"]), torch.from_numpy(np.array(case.col))
    y, a_dst, a_src = (torch.from_numpy(np.array(a)).double().requires_grad_(True) for a in (case.y, case.a_dst, case.a_src))
    a_edge = torch.from_numpy(np.array(case.a_edge)).double().requires_grad_(True) if edge else None
    u = a_dst[row] + a_src[col] + (a_edge if edge else 0.0)
    assert np.array_equal((u.detach().numpy() > 0), case.ref["pos"])
    s = torch.nn.functional.leaky_relu(u, ns)
    top = np.full((case.m, heads), -np.inf)
    np.maximum.at(top, row.numpy(), s.detach().numpy())
    top = torch.from_numpy(top)
    w = torch.exp(s - top[row])
    den = torch.zeros(case.m, heads, dtype=torch.float64).index_add_(0, row, w)
    import isplib_amd
    mask = isplib_amd.gat_dropout_mask(case.nnz, heads, case.p, case.seed)
    a = (w / den[row]) * mask.double() * float(np.float32(1.0 / (1.0 - case.p)))
    z = torch.zeros(case.m, heads, d, dtype=torch.float64).index_add_(0, row, a[:, :, None] * y.view(case.n, heads, d)[col]).view(case.m, heads * d)
    z.backward(torch.from_numpy(np.array(case.g)).double())
    outs = [("z", z.detach().numpy()), ("dy", y.grad.numpy()), ("dadst", a_dst.grad.numpy()), ("dasrc", a_src.grad.numpy())]
    if edge:
        outs.append(("daedge", a_edge.grad.numpy()))
    for name, got in outs:
        scale = max(np.abs(case.ref[name]).max(), np.abs(case.ref["du"]).max() if name.startswith("da") else 0.0)
        assert np.abs(got - case.ref[name]).max() <= 1e-10 * scale, name


def test_the_new_entries_resolve_and_the_abi_version_stays_1():
    from isplib_amd import cabi
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "isplib_hip.h")).read(), flags=re.S)
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    L = cabi.lib()
    for name in ENTRIES + HOST_FUNCTIONS:
        assert name in (cabi.EXPORTS if name in ENTRIES else cabi.GAT_DROP_HOST_EXPORTS)
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert getattr(L, name) is not None
        assert name in integration, name
    assert int(re.search(r"#define\s+ISPLIB_HIP_ABI_VERSION\s+(\d+)", header).group(1)) == 1
    assert L.isplib_hip_abi_version() == 1
    # one statement of the bit: the header of the kernels and the host
    text = open(os.path.join(ROOT, "isplib_amd", "csrc", "gat_dropout.h")).read()
    assert "__host__ __device__" in text and "0x9E3779B9" in text
    assert '#include "gat_dropout.h"' in open(os.path.join(ROOT, "isplib_amd", "csrc", "gat.hip")).read()


def _adj(m, n):
    import isplib_amd
    rowptr = torch.arange(0, m + 1, dtype=torch.int64)
    col = torch.arange(m, dtype=torch.int64) % n
    return isplib_amd.SparseTensor.from_csr(rowptr, col, None, (m, n))


def test_plugin_refuses_bad_dropout_and_seed_before_anything_touches_a_device(monkeypatch):
    import isplib_amd
    monkeypatch.delenv("ISPLIB_HALF_GAT", raising=False)
    adj = _adj(6, 4)
    y, a_dst, a_src, a_edge = torch.zeros(4, 16), torch.zeros(6, 2), torch.zeros(4, 2), torch.zeros(6, 2)      # CPU tensors: a launch is impossible
    for a_e in (None, a_edge):
        for bad in (1.0, -0.1, float("nan"), 1.5, 2):
            with pytest.raises(ValueError, match="`dropout` must lie in"):
                isplib_amd.gat_matmul(adj, y, a_dst, a_src, heads=2, a_edge=a_e, dropout=bad)
            with pytest.raises(ValueError, match="`dropout` must lie in"):                # a bad value is refused in eval mode too
                adj.gat_matmul(y, a_dst, a_src, 2, 0.2, a_e, bad, False)
        for bad in (True, "0.5", None, torch.tensor(0.5), np.float32(0.5)):
            with pytest.raises(TypeError, match="`dropout` must be a Python float or int"):
                isplib_amd.gat_matmul(adj, y, a_dst, a_src, heads=2, a_edge=a_e, dropout=bad)
        for bad in (-1, 2 ** 63):
            with pytest.raises(ValueError, match="`seed` must lie in"):
                isplib_amd.gat_matmul(adj, y, a_dst, a_src, heads=2, a_edge=a_e, dropout=0.6, seed=bad)
        for bad in (True, 1.0, "1"):
            with pytest.raises(TypeError, match="`seed` must be an int"):
                adj.gat_matmul(y, a_dst, a_src, 2, a_edge=a_e, dropout=0.6, seed=bad)
        # well-formed dropout: the operand checks of the call without it, then the device check
        with pytest.raises(ValueError, match=r"`a_dst` must be \[6, 2\]"):
            isplib_amd.gat_matmul(adj, y, a_dst[:-1], a_src, heads=2, a_edge=a_e, dropout=0.6, seed=1)
        with pytest.raises(ValueError, match="power of two"):
            isplib_amd.gat_matmul(adj, torch.zeros(4, 12), a_dst, a_src, heads=2, a_edge=a_e, dropout=0.6)
        with pytest.raises(TypeError, match="float32"):
            isplib_amd.gat_matmul(adj, y.bfloat16(), a_dst, a_src, heads=2, a_edge=a_e, dropout=0.6)
        with pytest.raises(TypeError, match="GPU tensor"):
            isplib_amd.gat_matmul(adj, y, a_dst, a_src, heads=2, a_edge=a_e, dropout=0.6, seed=2 ** 63 - 1)
    with pytest.raises(ValueError, match=r"`a_edge` must be \[6, 2\]"):
        adj.gat_matmul(y, a_dst, a_src, 2, a_edge=torch.zeros(5, 2), dropout=0.6)
    monkeypatch.setenv("ISPLIB_HALF_GAT", "native")                     # a 16-bit y: the conversion route, which raises what the fp32 call raises
    with pytest.raises(TypeError, match="GPU tensor"):
        adj.gat_matmul(y.bfloat16(), a_dst, a_src.bfloat16(), 2, dropout=0.6, seed=3)
    with pytest.raises(TypeError, match="float32 or of `y`'s dtype"):
        adj.gat_matmul(y.bfloat16(), a_dst, a_src, 2, a_edge=a_edge.half(), dropout=0.6)


class _Flagged(torch.Tensor):                                           # CPU tensors that claim to be on the GPU: nothing is launched
    is_cuda = True


def _fake_ops(monkeypatch, calls):
    from isplib_amd import plugin

    class Ops:
        @staticmethod
        def gat_spmm(*args):
            calls.append(("gat_spmm", args))
            return "z"

        @staticmethod
        def gat_edge_spmm(*args):
            calls.append(("gat_edge_spmm", args))
            return "ze"

        @staticmethod
        def gat_drop_spmm(*args):
            calls.append(("gat_drop_spmm", args))
            return "zd"

    class FakeTorchOps:
        isplib = Ops

    monkeypatch.setattr(plugin.torch, "ops", FakeTorchOps)
    adj = _adj(6, 4)
    st = adj.storage
    st._colptr, st._csr2csc, st._row_t = torch.zeros(5, dtype=torch.int64), torch.arange(6), torch.arange(6)    # the cached transpose
    y, a_dst, a_src = (t.as_subclass(_Flagged) for t in (torch.zeros(4, 16), torch.zeros(6, 2), torch.zeros(4, 2)))
    a_edge = torch.zeros(2, 6).t().as_subclass(_Flagged)
    return adj, st, y, a_dst, a_src, a_edge


def test_no_dropout_and_eval_mode_take_the_old_call_path(monkeypatch):
    import isplib_amd
    calls = []
    adj, st, y, a_dst, a_src, a_edge = _fake_ops(monkeypatch, calls)
    state = torch.get_rng_state()
    assert isplib_amd.gat_matmul(adj, y, a_dst, a_src, heads=2, negative_slope=0.1, dropout=0.0) == "z"
    assert adj.gat_matmul(y, a_dst, a_src, 2, 0.1, None, 0.6, False) == "z"
    assert adj.gat_matmul(y, a_dst, a_src, 2, 0.1, dropout=0, training=True, seed=5) == "z"
    assert adj.gat_matmul(y, a_dst, a_src, 2, 0.1, dropout=0.6, training=False, seed=5) == "z"
    for name, args in calls:
        assert name == "gat_spmm" and len(args) == 9 and args[4] is y and args[5] is a_dst and args[6] is a_src and args[7:] == (2, 0.1)
    del calls[:]
    assert adj.gat_matmul(y, a_dst, a_src, 2, 0.1, a_edge, 0.0) == "ze"
    assert adj.gat_matmul(y, a_dst, a_src, 2, 0.1, a_edge, 0.9, training=False) == "ze"
    for name, args in calls:
        assert name == "gat_edge_spmm" and len(args) == 11 and args[4] is st._csr2csc and args[5] is y and args[9:] == (2, 0.1)
    assert torch.equal(torch.get_rng_state(), state)                    # and no seed was drawn
    del calls[:]
    # with dropout: the new operator, csr2csc included, a_edge None or copied, then p and the seed
    assert adj.gat_matmul(y, a_dst, a_src, 2, 0.1, None, 0.6, True, 77) == "zd"
    assert adj.gat_matmul(y, a_dst, a_src, 2, 0.1, a_edge, dropout=0.25, seed=2 ** 63 - 1) == "zd"
    (n1, a1), (n2, a2) = calls
    assert n1 == n2 == "gat_drop_spmm" and len(a1) == len(a2) == 13
    assert a1[4] is st._csr2csc and a1[5] is y and a1[8] is None and a1[9:] == (2, 0.1, 0.6, 77)
    assert a2[8].is_contiguous() and tuple(a2[8].shape) == (6, 2) and a2[9:] == (2, 0.1, 0.25, 2 ** 63 - 1)


def test_a_seed_of_none_is_drawn_from_the_default_generator_and_repeats_under_manual_seed(monkeypatch):
    calls = []
    adj, st, y, a_dst, a_src, a_edge = _fake_ops(monkeypatch, calls)
    torch.manual_seed(1234)
    adj.gat_matmul(y, a_dst, a_src, 2, dropout=0.6)
    adj.gat_matmul(y, a_dst, a_src, 2, dropout=0.6)
    torch.manual_seed(1234)
    adj.gat_matmul(y, a_dst, a_src, 2, a_edge=a_edge, dropout=0.6)
    seeds = [args[12] for _, args in calls]
    assert all(type(s) is int and 0 <= s < 2 ** 63 for s in seeds)
    assert seeds[0] == seeds[2] and seeds[0] != seeds[1]
