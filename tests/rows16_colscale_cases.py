"""Inputs shared by tests/test_gpu_rows16_colscale.py and the census of them in tests/test_rows16_colscale_host.py: the graphs are
those of tests/test_gpu_rows16.py, the scale tables are made here."""
import numpy as np

from tests import cases
from tests.test_gpu_rows16 import LONG_ROW, U, _edge_degrees, _hub_graph  # noqa: F401  (re-exported)

N = 200                                        # columns of both graphs
SUBNORMAL = np.float32(1e-40)


def hub_graph():
    """random_csr(300, 200, 12, 31, empty_rows=(0, 150, 299), hub=(7, 2500), duplicates=True)."""
    return _hub_graph()


def length_degrees():
    deg = _edge_degrees()
    return deg + deg[::-1]                     # every length in two places of a workgroup's four rows


def length_graph():
    return cases.csr_of_degrees(length_degrees(), N, 17)


def scale_table(n=N, seed=23):
    """One fp32 factor per column: 1 / deg for deg in 1 .. 40 mostly, a sixth of them negated, every 11th zero (both signs) and one
    subnormal."""
    rng = np.random.default_rng(seed)
    s = (np.float32(1.0) / rng.integers(1, 41, n).astype(np.float32)).astype(np.float32)
    s[rng.random(n) < 1 / 6] *= np.float32(-1.0)
    s[::11] = np.float32(0.0)
    s[11] = np.float32(-0.0)
    s[5] = SUBNORMAL
    return s


def integer_scale(n=N, seed=29):
    """Integers in [-5, 5]: with |x| <= 3 every fp32 product and sum of a row of up to 6,144 edges is exact (< 92,160 < 2^24)."""
    return np.random.default_rng(seed).integers(-5, 6, n).astype(np.float32)


def special_scale(kind, n):
    """A 1 / deg-like table with a few Inf / NaN entries, or a table of fp32 subnormals."""
    rng = np.random.default_rng(37)
    if kind == "denormal":
        return ((rng.random(n, np.float32) * 2 - 1) * np.float32(3e-38)).astype(np.float32)
    s = (np.float32(1.0) / rng.integers(1, 9, n).astype(np.float32)).astype(np.float32)
    s[3], s[n // 2], s[n - 2] = np.inf, -np.inf, np.nan
    return s
