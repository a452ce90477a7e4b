#!/usr/bin/env python3
"""Per-rank work of the partitioned max / min backward, all-gathered form against the owner-bucketed exchange -- EMULATED ON ONE
GPU, NO COLLECTIVE: every rank of a P-rank 1-D row partition is played in turn on this device, and the exchange itself (xGMI)
is not measured at all.  Reddit-shaped synthetic graph (bench.py's), max, weighted, K = 64 and 128, P in {1, 2, 4, 8}.

For every emulated rank two legs alternate in the same run, each warmed up and timed with device events over a window of at
least 0.2 s, `--rounds` times; median and spread (min .. max) over the rounds are reported:
  (a) today's per-rank work: scatter_rows_det over all world * pad * K all-gathered pairs;
  (b) the owner exchange's:  minmax_bw_bucket on the rank's own rows + scatter_keys_det on the pairs the rank owns
      (also timed one by one, to tell which of the two holds the time).
Both legs' results are compared bit for bit first.  The bytes each form makes a rank receive are printed beside the times.

    python scripts/minmax_bw_scaling.py [--out profiles/owner_exchange_scaling.txt] [--scale 1.0] [--rounds 5]
"""
import argparse
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

WINDOW_S = 0.2
RECORDED_ONE_GPU_MS = 0.83       # the project's record of the one-GPU deterministic max backward at K = 64


def window_ms(fn, reps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps


def alternate(legs, rounds):
    """{name: [ms per call, one figure per round]}; the legs take turns inside every round."""
    reps = {}
    for name, fn in legs.items():
        for _ in range(3):
            fn()                                                           # warm-up: code objects, the allocator's blocks
        torch.cuda.synchronize()
        reps[name] = max(3, math.ceil(WINDOW_S * 1e3 / max(window_ms(fn, 3), 1e-3)))
    times = {name: [] for name in legs}
    for _ in range(rounds):
        for name, fn in legs.items():
            times[name].append(window_ms(fn, reps[name]))
    return times


def fmt(ts):
    return f"{statistics.median(ts):7.3f} ({min(ts):.3f} .. {max(ts):.3f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "owner_exchange_scaling.txt"))
    ap.add_argument("--scale", type=float, default=1.0, help="shrink the graph (rehearsals)")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--ks", default="64,128")
    ap.add_argument("--ranks", default="1,2,4,8")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("minmax_bw_scaling.py measures on the GPU; none is visible")
    from isplib_amd import cabi, synth
    from isplib_amd.dist import nnz_balanced_cuts
    dev = torch.device("cuda:0")
    rowptr, col, n = synth.dataset_like("reddit", device=dev, scale=a.scale)
    nnz = col.numel()
    w = synth.edge_weights(nnz, device=dev)
    lines = ["EMULATED ON ONE GPU, NO COLLECTIVE: per-rank work of the partitioned max backward, rank by rank on one MI355X;",
             "the exchange itself (xGMI) is NOT measured.  ms per call: median (min .. max) over %d alternating windows >= %.1f s." % (a.rounds, WINDOW_S),
             f"graph: reddit-shaped synthetic, n = {n}, nnz = {nnz}, scale = {a.scale}; max, weighted",
             "(a) scatter_rows_det over world * pad * K all-gathered pairs   (b) minmax_bw_bucket on own rows + scatter_keys_det on owned pairs", ""]
    verdicts = []
    for k in [int(v) for v in a.ks.split(",")]:
        x = synth.features(n, k, device=dev, integer=True)
        g = synth.features(n, k, seed=5, device=dev)
        _, arg = cabi.spmm(rowptr, col, w, x, "max")
        one = alternate({"one": lambda: cabi.spmm_minmax_bw(col, w, x, arg, g, need_val=False, deterministic=True)}, a.rounds)["one"]
        lines.append(f"K = {k}: one-GPU deterministic backward (isplib_spmm_minmax_bw_det_hip, grad_mat only) {fmt(one)} ms")
        lines.append(f"{'P':>2} {'rank':>4} {'rows':>7} {'pairs owned':>11} | {'(a) ms':>25} | {'(b) ms':>25} | {'(b) bucket':>25} | {'(b) scatter':>25} | "
                     f"{'(a) bytes received':>18} | {'(b) bytes received':>18}")
        ok = arg != nnz
        pos = arg.clamp(0, nnz - 1)
        dest = torch.where(ok, col[pos], col.new_full((), -1)).to(torch.int32)
        gval = torch.where(ok, w[pos] * g, g.new_zeros(()))
        del pos
        for world in [int(v) for v in a.ranks.split(",")]:
            cuts = nnz_balanced_cuts(rowptr, world)
            pad = max(cuts[p + 1] - cuts[p] for p in range(world))
            d_all = torch.full((world * pad, k), -1, dtype=torch.int32, device=dev)
            g_all = torch.zeros((world * pad, k), dtype=torch.float32, device=dev)
            for p in range(world):
                d_all[p * pad: p * pad + cuts[p + 1] - cuts[p]] = dest[cuts[p]:cuts[p + 1]]
                g_all[p * pad: p * pad + cuts[p + 1] - cuts[p]] = gval[cuts[p]:cuts[p + 1]]
            own = []                                                       # every sender's operands and what its bucket kernel makes
            for p in range(world):
                e0, e1 = int(rowptr[cuts[p]]), int(rowptr[cuts[p + 1]])
                ops = (arg[cuts[p]:cuts[p + 1]].contiguous(), e0, col[e0:e1].contiguous(), w[e0:e1].contiguous(), g[cuts[p]:cuts[p + 1]].contiguous())
                keys, vals, seg = cabi.minmax_bw_bucket(*ops, cuts)
                own.append((ops, keys, vals, seg.cpu().tolist()))
            worst = {"a": [], "b": []}
            for r in range(world):
                rows = cuts[r + 1] - cuts[r]
                r_keys = torch.cat([keys[seg[r]:seg[r + 1]] for _, keys, _, seg in own])
                r_vals = torch.cat([vals[seg[r]:seg[r + 1]] for _, _, vals, seg in own])
                want = cabi.scatter_rows_det(d_all, g_all, cuts[r], rows)
                got = cabi.scatter_keys_det(r_keys, r_vals, rows, k)
                if not torch.equal(got.view(torch.int32), want.view(torch.int32)):
                    raise SystemExit(f"K={k} P={world} rank {r}: the owner exchange's gradient differs from the all-gathered form's")
                del want, got
                ops = own[r][0]
                legs = {
                    "a": lambda: cabi.scatter_rows_det(d_all, g_all, cuts[r], rows),
                    "b": lambda: (cabi.minmax_bw_bucket(*ops, cuts), cabi.scatter_keys_det(r_keys, r_vals, rows, k)),
                    "bucket": lambda: cabi.minmax_bw_bucket(*ops, cuts),
                    "scatter": lambda: cabi.scatter_keys_det(r_keys, r_vals, rows, k),
                }
                t = alternate(legs, a.rounds)
                bytes_a = 2 * world * pad * k * 4
                bytes_b = 8 * r_keys.numel() + world * world * 8
                lines.append(f"{world:>2} {r:>4} {rows:>7} {r_keys.numel():>11} | {fmt(t['a']):>25} | {fmt(t['b']):>25} | {fmt(t['bucket']):>25} | "
                             f"{fmt(t['scatter']):>25} | {bytes_a:>18} | {bytes_b:>18}")
                print(lines[-1], flush=True)
                worst["a"].append(t["a"])
                worst["b"].append(t["b"])
                if world == 8:
                    sep = min(t["a"]) - max(t["b"])
                    verdicts.append((k, r, sep > 0, statistics.median(t["b"]), statistics.median(t["bucket"]), statistics.median(t["scatter"])))
                del r_keys, r_vals
            lines.append(f"{world:>2}  max over ranks of the medians: (a) {max(statistics.median(v) for v in worst['a']):.3f} ms, "
                         f"(b) {max(statistics.median(v) for v in worst['b']):.3f} ms")
            del d_all, g_all, own
            torch.cuda.empty_cache()
        one_med = statistics.median(one)
        mine = [v for v in verdicts if v[0] == k]
        if mine:
            b_max = max(v[3] for v in mine)
            holder = "scatter_keys_det" if max(v[5] for v in mine) >= max(v[4] for v in mine) else "minmax_bw_bucket"
            lines.append(f"K = {k}, P = 8: (b) below (a) by more than the spread (max of (b)'s windows < min of (a)'s) on "
                         f"{sum(v[2] for v in mine)} of {len(mine)} ranks; slowest rank (b) {b_max:.3f} ms = {b_max / one_med:.2f} x the one-GPU "
                         f"time measured here ({one_med:.3f} ms), {b_max / RECORDED_ONE_GPU_MS:.2f} x the recorded {RECORDED_ONE_GPU_MS} ms (K = 64); "
                         f"target <= 0.25 x: {'reached' if b_max <= 0.25 * one_med else 'NOT reached'} against this run's time; "
                         f"the larger share of (b) is {holder}")
        lines.append("")
        del x, g, arg, dest, gval
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
