"""The levelled deal of the stream plans (isplib_amd/plan.py: stream_plan_arrays(capacities=...); include/isplib_hip.h,
isplib_stream_capacities_hip), replayed on the CPU: what the capacities may and may not change."""
import numpy as np
import pytest
import torch

from tests import cases

ONE = 4096
STREAMS, RPW, WPG, CHUNK, SLICES = 4, 32, 8, 256, 3
PER = RPW // STREAMS
SKEWED = {"0.5 to 1.5": [ONE // 2 + (ONE * w) // 7 for w in range(WPG)],
          "one at a tenth": [ONE] * 3 + [ONE // 10] + [ONE] * 4}


SPREAD_PIN = {"0.5 to 1.5": 673.4, "one at a tenth": 1929.2}      # edges per unit of capacity, on _graph()


def _graph():
    """~3,000 rows of Poisson(30) entries, empty rows, and one row of 3,000 entries that is cut into virtual rows"""
    return cases.random_csr(3000, 500, 30, 11, empty_rows=tuple(range(0, 3000, 17)), hub=(7, 3000))


def _arrays(rowptr, col, capacities):
    from isplib_amd.plan import stream_plan_arrays
    return stream_plan_arrays(torch.from_numpy(rowptr), torch.from_numpy(col), 500, SLICES, WPG, RPW, STREAMS, CHUNK, capacities=capacities)


def _same(p, q):
    return all(torch.equal(p[k], q[k]) if torch.is_tensor(p[k]) else p[k] == q[k] for k in p)


def _vrow_lengths(rowptr):
    deg = np.diff(rowptr)
    nch = np.maximum(-(-deg // CHUNK), 1)
    return np.concatenate([[(d - ci + k - 1) // k for ci in range(k)] for d, k in zip(deg, nch)])


def _stream_loads(p):
    nw = p["gens"] * WPG
    perm, off = p["perm"].numpy().reshape(-1, STREAMS), p["wave_step_off"].numpy()
    return np.array([[(perm[off[w]:off[w + 1], g] >= 0).sum() for g in range(STREAMS)] for w in range(nw)]).reshape(-1)


def test_the_constant_is_the_headers():
    from isplib_amd import cabi
    from tests.stage_rule import header_constant
    assert cabi.STREAM_CAP_ONE == ONE == header_constant("STREAM_CAP_ONE")


@pytest.mark.parametrize("value", (ONE, ONE // 2, 3 * ONE))
def test_equal_capacities_are_todays_plan(value):
    """All capacities equal, whatever their common value: the arrays of the unlevelled plan, bit for bit."""
    rowptr, col = _graph()
    assert _same(_arrays(rowptr, col, None), _arrays(rowptr, col, [value] * WPG))


@pytest.mark.parametrize("name", sorted(SKEWED))
def test_skewed_capacities_move_rows_between_waves_and_nothing_else(name):
    """Every (virtual) row is placed exactly once, every stream still gets one row per round, a row's words and their order are
    what they are in the unlevelled plan, and two builds give identical arrays."""
    rowptr, col = _graph()
    caps = SKEWED[name]
    p, base = _arrays(rowptr, col, caps), _arrays(rowptr, col, None)
    assert _same(p, _arrays(rowptr, col, caps)), "two builds"
    assert not _same(p, base), "these capacities do change the deal"
    nw = p["gens"] * WPG
    vl = _vrow_lengths(rowptr)
    ns = nw * STREAMS
    rounds = -(-vl.size // ns)
    wr = p["wave_row"].numpy().reshape(nw, STREAMS, PER)
    wp = p["wave_part"].numpy().reshape(nw, STREAMS, PER)
    # placed once: whole rows by their id, pieces of the cut row by their partial-row id
    whole = wr[(wr >= 0) & (wp < 0)]
    assert np.array_equal(np.sort(whole), np.setdiff1d(np.arange(3000), [7]))
    assert np.array_equal(np.sort(wp[wp >= 0]), np.arange(p["n_parts"])) and (wr[wp >= 0] == 7).all()
    # one row per round: local row r of a stream is its row of round r -- full rounds fill every stream, the last one the rest
    used = (wr >= 0).reshape(ns, PER)
    assert used[:, :rounds - 1].all() and not used[:, rounds:].any()
    assert used[:, rounds - 1].sum() == vl.size - (rounds - 1) * ns
    # the words of a row, in order: the same CSR positions in the same sequence as in the unlevelled plan
    def row_words(q):
        perm = q["perm"].numpy().reshape(-1, STREAMS)
        off = q["wave_step_off"].numpy()
        words = (q["words"].numpy().astype(np.int64) & 0xFFFFFFFF).reshape(-1, STREAMS)
        rows = q["wave_row"].numpy().reshape(-1, RPW)
        parts = q["wave_part"].numpy().reshape(-1, RPW)
        out = {}
        for w in range(q["gens"] * WPG):
            for g in range(STREAMS):
                e, lr = perm[off[w]:off[w + 1], g], words[off[w]:off[w + 1], g] >> 24
                for j in np.unique(lr[e >= 0]):
                    out[(int(rows[w, j]), int(parts[w, j]))] = e[(e >= 0) & (lr == j)].tolist()
        return out
    assert row_words(p) == row_words(base)


@pytest.mark.parametrize("name", sorted(SKEWED))
def test_every_round_orders_the_streams_by_load_over_capacity(name):
    """The rule itself, round by round: before round r the streams are ordered by load * ONE // capacity (ties: the lower stream
    first) and receive the round's rows longest first -- so along that order the lengths of the rows received never increase.

    What this does NOT assert is a bound on the final spread of load / capacity by "the longest virtual row of the last
    round".  No such bound follows from the rule, levelled or not: a stream takes one row in EVERY round, the rows of a round
    differ by little (a round is a slice of the sorted lengths), so the deal can move at most (longest - shortest row) edges
    per stream in all, whatever the capacities ask for.  The test prints the spread on this graph (longest virtual row 250,
    the last round's longest 21): 203 edges with equal capacities, 673 with 0.5 to 1.5, 1,929 with one wave at a tenth.
    Capacities within a few percent of nominal -- what the calibration hands out, clamped to 8 % -- are inside that reach on
    graphs with a long tail of row lengths (the headline plan: steps per group follow the capacities to 0.1 %,
    profiles/stream_level.txt).  What the deal does guarantee is the ordering below; and the waves of the smallest capacity
    end with fewer edges than those of the largest."""
    rowptr, col = _graph()
    caps = SKEWED[name]
    p = _arrays(rowptr, col, caps)
    nw = p["gens"] * WPG
    ns = nw * STREAMS
    loads_final = _stream_loads(p)
    assert loads_final.sum() == col.size
    # length of the row a stream got in round r, from the words: edges per (stream, local row)
    perm, off = p["perm"].numpy().reshape(-1, STREAMS), p["wave_step_off"].numpy()
    words = (p["words"].numpy().astype(np.int64) & 0xFFFFFFFF).reshape(-1, STREAMS)
    got = np.zeros((ns, PER), np.int64)
    for w in range(nw):
        for g in range(STREAMS):
            e, lr = perm[off[w]:off[w + 1], g], words[off[w]:off[w + 1], g] >> 24
            np.add.at(got[w * STREAMS + g], lr[e >= 0] - g * PER, 1)
    used = (p["wave_row"].numpy().reshape(ns, PER) >= 0)
    cap_s = np.array([caps[(s // STREAMS) % WPG] for s in range(ns)], np.int64)
    loads = np.zeros(ns, np.int64)
    for r in range(PER):
        if not used[:, r].any():
            break
        order = np.argsort(np.minimum(loads * ONE // cap_s, 2 ** 32 - 1), kind="stable")
        takers = order[:used[:, r].sum()]
        assert used[takers, r].all() and not used[order[takers.size:], r].any(), "the round's rows go to the least loaded streams"
        lens = got[takers, r]
        assert (lens[:-1] >= lens[1:]).all(), f"round {r}"
        loads += got[:, r]
    assert np.array_equal(loads, loads_final)
    n = loads / (cap_s / ONE)
    print(f"{name}: spread of load / capacity {n.max() - n.min():.1f}; longest virtual row {_vrow_lengths(rowptr).max()}")
    assert loads[cap_s == cap_s.min()].mean() < loads[cap_s == cap_s.max()].mean()
    # pins of what the deal reaches on this graph (integer arithmetic: the figures are exact), so that a change of the rule shows:
    # the spread of load / capacity, and load / capacity falling strictly from the smallest capacity to the largest (the deal
    # moves every level towards its share and, out of reach, overshoots none)
    assert n.max() - n.min() <= SPREAD_PIN[name]
    ratio = [loads[cap_s == v].mean() * ONE / v for v in np.unique(cap_s)]
    assert all(a > b for a, b in zip(ratio, ratio[1:])), ratio


IN_REACH = {"pm4 alternating": [ONE * 96 // 100 if w % 2 else ONE * 104 // 100 for w in range(WPG)],
            "pm8 ramp": [ONE * 92 // 100 + (ONE * 16 // 100) * w // 7 for w in range(WPG)]}


@pytest.mark.parametrize("name", sorted(IN_REACH))
def test_capacities_within_the_deals_reach_are_met(name):
    """How well the deal levels where it can.  6,144 rows with lengths uniform on 0..250 (and one row of 3,000, cut), 768 streams,
    8 rounds: a round spans ~31 edges of length, a stream's load is ~956.  A stream that takes the rows above its round's median
    in every round ends ~8 x 31 / 4 = 62 edges above the mean when half of the streams want that, up to 8 x 31 / 2 = 125 when only
    the extremes of a ramp do.  +-4 % alternating asks for 38, the ends of the +-8 % ramp for 76: both inside the reach.  Then
      * load / capacity of all streams agrees to within the longest virtual row (250), and
      * the mean of load / capacity over the streams of each capacity level is within 1 % of the overall figure: a quarter of
        the smallest skew applied here (4 %), so a deal that under-corrects by half (2 % left) fails.
    (Outside the reach -- +-8 % alternating asks for 76 against 62 -- the levels stay ~2 % apart: the limit the one-row-per-round
    rule sets, which the headline plan, 16 rounds over rows up to a seventh of a stream's load, is far from.)"""
    rng = np.random.default_rng(3)
    deg = rng.integers(0, 251, 6144).astype(np.int64)
    deg[7] = 3000
    rowptr = np.zeros(deg.size + 1, np.int64)
    np.cumsum(deg, out=rowptr[1:])
    col = rng.integers(0, 500, rowptr[-1]).astype(np.int64)
    caps = IN_REACH[name]
    p = _arrays(rowptr, col, caps)
    loads = _stream_loads(p)
    assert loads.sum() == col.size
    cap_s = np.array([caps[(s // STREAMS) % WPG] for s in range(loads.size)], np.int64)
    n = loads * ONE / cap_s
    overall = loads.sum() * ONE / cap_s.sum()
    level = {int(v): n[cap_s == v].mean() / overall for v in np.unique(cap_s)}
    print(f"{name}: spread of load / capacity {n.max() - n.min():.1f}; by level {level}")
    assert n.max() - n.min() <= _vrow_lengths(rowptr).max()
    assert all(abs(v - 1.0) <= 0.01 for v in level.values()), level
