"""Inputs of the FusedMM accuracy tests, shared by the CPU tests of the bound (tests/test_fusedmm_bound_host.py), the GPU tests
(tests/test_gpu_fusedmm_accuracy.py) and the probe that measures C_f (scripts/fusedmm_sop_accuracy.py).  NumPy only."""
import numpy as np

from tests import cases

DOT_WORD = 0x2 | 0x10 | 0xF00 | 0x1000 | 0x10000        # COPY_RHS | DOT   | UDEF | MUL | ADD
NORM_WORD = 0x5 | 0x50 | 0xF00 | 0x1000 | 0x10000       # SUBR     | NORMR | UDEF | MUL | ADD
COPY_WORD = 0x2 | 0x00 | 0x100 | 0x1000 | 0x10000       # COPY_RHS | NOOP  | COPY | MUL | ADD (the SpMM sum)

MENU = ("sigmoid", "one_minus_sigmoid", "tdist", "scale", "exp", "leaky_exp")
PARAM = 0.2                                              # the menu parameter of every real-valued case (scale, leaky_exp)


def menu_on(word):
    """The menu entries defined on a word: 1 / (1 + s) has a pole at s = -1, and only the norm word keeps s >= 0."""
    return tuple(fn for fn in MENU if not (fn == "tdist" and word != NORM_WORD))


def word_of(vop, rop, sop, vsc, aop):
    return vop | (rop << 4) | (sop << 8) | (vsc << 12) | (aop << 16)


# ---- the single-edge probe: row i holds the one edge (i, i), so z[i] is f(s_i) with nothing else rounded ---------------------

def _keep_clear(mag):
    """Exponent arguments stay out of (87.0, 89.5): there expf and an exp2-based exponential may overflow an ulp of the argument
    apart, and neither answer is wrong."""
    mag = mag.copy()
    inside = (mag > 87.0) & (mag < 89.5)
    mag[inside] = np.where(mag[inside] < 88.25, 87.0, 89.5)
    return mag


def probe_grid(fn, npts):
    """npts values of s (fp32): 0, then both signs log-spaced over [2^-20, 100].  exp / leaky_exp: s in [-100, 80] (overflow has a
    test of its own); tdist: s >= 0 only."""
    if fn == "tdist":
        return np.concatenate(([0.0], _keep_clear(np.geomspace(2.0 ** -20, 100.0, npts - 1)))).astype(np.float32)
    half = (npts - 1) // 2
    pos = _keep_clear(np.geomspace(2.0 ** -20, 80.0 if fn in ("exp", "leaky_exp") else 100.0, npts - 1 - half))
    neg = -_keep_clear(np.geomspace(2.0 ** -20, 100.0, half))
    return np.concatenate(([0.0], pos, neg)).astype(np.float32)


def probe_graph(npts):
    return np.arange(npts + 1, dtype=np.int64), np.arange(npts, dtype=np.int64)


def probe_dot(s, k=8):
    """x_i = (1, 0, ...), y_j = (s_j, 1, 0, ...): the dot product is exactly s_j and z[i, 1] is the device's f(s_j)."""
    x = np.zeros((s.size, k), np.float32)
    x[:, 0] = 1.0
    y = np.zeros((s.size, k), np.float32)
    y[:, 0] = s
    y[:, 1] = 1.0
    return x, y


def probe_norm_args(fn, npts):
    """a_j >= 0 with 12 significant bits, so s_j = a_j^2 is exact in fp32; s covers [2^-20, 100] (exp entries: 80)."""
    top = 80.0 if fn in ("exp", "leaky_exp") else 100.0
    mant, expo = np.frexp(np.sqrt(np.geomspace(2.0 ** -20, top, npts - 1)))
    a = np.ldexp(np.floor(mant * 4096.0) / 4096.0, expo)
    a[(a * a > 87.0) & (a * a < 89.5)] = 9.25                      # s = 85.5625: see _keep_clear
    a = np.concatenate(([0.0], a)).astype(np.float32)
    s = a.astype(np.float64) ** 2
    assert np.array_equal(s, s.astype(np.float32).astype(np.float64)) and not np.any((s > 87.0) & (s < 89.5))
    return a


def probe_norm(a, k=8):
    """x = 0, y_j = (a_j, 0, ...): T = y_j, s = a_j^2 exactly, z[i, 0] = f(s) * a_j (one more rounding: the product's)."""
    y = np.zeros((a.size, k), np.float32)
    y[:, 0] = a
    return np.zeros((a.size, k), np.float32), y


# ---- prescribed s in real rows (dot word) -----------------------------------------------------------------------------

S_GRID = np.array([0.0] + [sg * v for v in (1e-3, 0.5, 1.0, 3.0, 10.0, 17.0, 30.0, 60.0, 80.0, 86.0) for sg in (1.0, -1.0)], np.float32)


def prescribed_graph(seed=6):
    return cases.random_csr(60, 4 * S_GRID.size, 9.0, seed, empty_rows=(0,), hub=(5, 300), duplicates=True)


def prescribed_operands(k):
    """x[:, 0] = 1 and the rest 0, so the dot product with y_j is y_j[0] exactly; y[:, 0] cycles through S_GRID, the other
    columns are uniform in [-1, 1]."""
    n = 4 * S_GRID.size
    x = np.zeros((60, k), np.float32)
    x[:, 0] = 1.0
    y = cases.dense(n, k, 21)
    y[:, 0] = S_GRID[np.arange(n) % S_GRID.size]
    return x, y


# ---- wide-spread s on ordinary data ---------------------------------------------------------------------------------

def spread_scale(word, k):
    """Both operands uniform in [-1, 1] times this: <x, y> has standard deviation a^2 sqrt(k) / 3 = 3 under ROP_DOT,
    |y - x|^2 has mean 2 k a^2 / 3 = 3 under ROP_NORMR (the words here pair it with VOP_SUBR)."""
    return np.float32(np.sqrt(4.5 / k) if ((word >> 4) & 0xF) == 5 else 3.0 / k ** 0.25)


def named_graph():
    """The graph of test_gpu_fusedmm.py::test_named_patterns_within_tolerance."""
    return cases.random_csr(400, 300, 20.0, seed=1, empty_rows=(7,), hub=(11, 2500))


def spread_operands(word, m, n, k):
    a = spread_scale(word, k)
    return cases.dense(m, k, 3) * a, cases.dense(n, k, 5) * a


# ---- other stage combinations with a real menu function -----------------------------------------------------------------

def combo_graph(k):
    return cases.random_csr(70, 55, 7.0, seed=k, empty_rows=(0, 33, 69), hub=(5, 300), duplicates=True)


def combo_words():
    """(VOP, ROP) of the two hot words with VSC_ADD / AOP_ADD and VSC_MUL / AOP_MAX, AOP_MIN."""
    return [word_of(vop, rop, 0xF, vsc, aop) for vop, rop in ((2, 1), (5, 5)) for vsc, aop in ((2, 1), (1, 2), (1, 3))]
