#!/usr/bin/env python3
"""A/B of the GAT attention operator with attention dropout (isplib_amd.gat_matmul(..., dropout=p): isplib_gat_drop_csr_hip and its two
backward kernels, the mask regenerated from the seed) on the shapes of scripts/gat_ab.py: the Reddit-shaped synthetic graph at
(H, d) = (8, 8) and (8, 16) and the ogbn-products shape at (8, 16) (bench.py's graphs), fp32, negative_slope 0.2, p = 0.6, forward alone
and forward + backward with all gradients.

Three forms, launched alternating, `--runs` runs each; a run is a number of steps between two device events after a warm-up of all:
  (a) dropout  gat_matmul with dropout=p and seed=None: every step draws its seed from torch's CPU generator, as a training loop does;
  (b) without  gat_matmul without it, in the same process -- the operator as it was; the cost of the mask is read as a / b;
  (c) composed the PyG-style composition under torch autograd (scripts/gat_ab.py's) with F.dropout ON THE COEFFICIENTS: index, add,
               leaky_relu -- an [H, nnz] array; a scatter softmax from torch scatter ops; F.dropout of the [H, nnz] coefficients; H
               weighted isplib_amd.matmul calls on column views of y.  Every structure array is built once, before the timing.
Peak device memory of one step beyond what is allocated before it (operands, structure, plans) is reported for each form.  (a) and (c)
draw different masks, so their outputs are not comparable; once per shape, untimed, the composition is run with the operator's own mask
(isplib_amd.gat_dropout_mask on the device, in place of F.dropout) against the operator under the same seed, and the largest
|difference| of z and of the gradients is printed (two different fp32 computations).

usage: python3 scripts/gat_dropout_ab.py [--runs 5] [--reps 3] [--op-reps 20] [--scale 1.0] [--out FILE]"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SLOPE = 0.2
P = 0.6


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--runs", type=int, default=5)
    p.add_argument("--reps", type=int, default=3, help="steps per run of the composition (a step is about half a second)")
    p.add_argument("--op-reps", type=int, default=20, help="steps per run of the two operator forms")
    p.add_argument("--scale", type=float, default=1.0, help="shrink the graphs (rehearsal only)")
    p.add_argument("--out", default="")
    a = p.parse_args()
    if not torch.cuda.is_available():
        sys.exit("gat_dropout_ab.py measures on the GPU: none is visible")
    import isplib_amd
    from isplib_amd import cabi, synth
    dev = torch.device("cuda:0")
    lines = [f"# scripts/gat_dropout_ab.py: fp32, negative_slope {SLOPE}, p = {P}, {a.runs} alternating runs; a run is {a.op_reps} steps of an "
             f"operator form, {a.reps} of the composition; ms per step",
             f"# device: {torch.cuda.get_device_name(0)}"]

    def emit(line):
        lines.append(line)
        print(line, flush=True)
        if a.out:                                   # kept up to date: a run that is cut short leaves what it measured
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    def timed(fn, reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(reps):
            fn()
        e.record()
        torch.cuda.synchronize()
        return s.elapsed_time(e) / reps

    def peak_bytes(fn):
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        fn()
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - base

    def measure(tag, rowptr, col, n, heads, d):
        nnz, k = col.numel(), heads * d
        y = (synth.features(n, k, seed=3, device=dev) * 2.0).requires_grad_(True)
        a_dst = (synth.features(n, heads, seed=4, device=dev) * 2.0).requires_grad_(True)
        a_src = (synth.features(n, heads, seed=6, device=dev) * 2.0).requires_grad_(True)
        g = synth.features(n, k, seed=5, device=dev)
        adj = isplib_amd.SparseTensor.from_csr(rowptr, col, None, (n, n), validate=False)
        row = adj.storage.row()
        w_a = [isplib_amd.SparseTensor.from_csr(rowptr, col, torch.ones(nnz, device=dev), (n, n), validate=False) for _ in range(heads)]

        def composed_fw(keep=None):
            s = torch.nn.functional.leaky_relu(a_dst.t()[:, row] + a_src.t()[:, col], SLOPE)      # [H, nnz]
            top = torch.full((heads, n), float("-inf"), device=dev).scatter_reduce(1, row.expand(heads, nnz), s.detach(), "amax",
                                                                                    include_self=True)
            w = torch.exp(s - top[:, row])
            att = w / torch.zeros(heads, n, device=dev).index_add(1, row, w)[:, row]
            att = torch.nn.functional.dropout(att, P, True) if keep is None else att * keep
            out = []
            for h in range(heads):
                w_a[h].storage._value = att[h]
                out.append(isplib_amd.matmul(w_a[h], y[:, h * d:(h + 1) * d], "sum"))
            return torch.cat(out, 1)

        def dropout_fw():
            return isplib_amd.gat_matmul(adj, y, a_dst, a_src, heads=heads, negative_slope=SLOPE, dropout=P)

        def without_fw():
            return isplib_amd.gat_matmul(adj, y, a_dst, a_src, heads=heads, negative_slope=SLOPE)

        def clear():
            y.grad = a_dst.grad = a_src.grad = None

        def step(fw, grad):
            def run():
                clear()
                if not grad:
                    with torch.no_grad():
                        return fw()
                out = fw()
                out.backward(g)
                return out
            return run

        emit(f"{tag} n={n} nnz={nnz} H={heads} d={d}")
        for what, grad in (("forward", False), ("forward+backward", True)):
            forms = [("composed", step(composed_fw, grad), a.reps), ("without", step(without_fw, grad), a.op_reps),
                     ("dropout", step(dropout_fw, grad), a.op_reps)]
            for name, fn, _ in forms:               # warm-up: loads the code objects, builds the plans and the transposed structure
                fn()
            peaks = {}
            for name, fn, _ in forms:               # the gradients of the step before are not operands: dropped before the base is read
                clear()
                peaks[name] = peak_bytes(fn)
            times = {name: [] for name, _, _ in forms}
            for _ in range(a.runs):
                for name, fn, reps in forms:
                    times[name].append(timed(fn, reps))
            for name in ("composed", "without", "dropout"):
                emit(f"   {what:17s}{name:9s}" + " ".join(f"{t:9.3f}" for t in times[name]) +
                     f"   min {min(times[name]):.3f} max {max(times[name]):.3f}   peak beyond operands {peaks[name] / 2 ** 20:.1f} MiB")
            lo = {name: min(times[name]) for name in times}
            emit(f"   {what}: (a) dropout / (b) without min/min {lo['dropout'] / lo['without']:.3f} (max/max "
                 f"{max(times['dropout']) / max(times['without']):.3f}); (a) dropout / (c) composed min/min "
                 f"{lo['dropout'] / lo['composed']:.3f}; every (a) run below every (c) run: "
                 f"{'yes' if max(times['dropout']) < min(times['composed']) else 'NO'}"
                 f" ([nnz, H] fp32 = {heads * nnz * 4 / 2 ** 20:.1f} MiB, [n, K] fp32 = {n * k * 4 / 2 ** 20:.1f} MiB)")
            del forms
            torch.cuda.empty_cache()
        # the operator against the composition with the operator's own mask, once, untimed
        seed = 20240607
        keep = (isplib_amd.gat_dropout_mask(adj, heads, P, seed).t().float() * cabi.gat_drop_scale(P)).contiguous()      # [H, nnz]: q c
        clear()
        zc = composed_fw(keep)
        zc.backward(g)
        want = [t.detach().clone() for t in (zc, y.grad, a_dst.grad, a_src.grad)]
        del zc, keep
        clear()
        zo = isplib_amd.gat_matmul(adj, y, a_dst, a_src, heads=heads, negative_slope=SLOPE, dropout=P, seed=seed)
        zo.backward(g)
        got = (zo.detach(), y.grad, a_dst.grad, a_src.grad)
        emit(f"   same mask (seed {seed}): operator vs composition max |z difference| {float((got[0] - want[0]).abs().max()):.3g}, max "
             f"|gradient difference| {max(float((u - v).abs().max()) for u, v in zip(got[1:], want[1:])):.3g}")
        del adj, w_a, y, a_dst, a_src, g, want, got, zo
        torch.cuda.empty_cache()

    rowptr, col, n = synth.dataset_like("reddit", device=dev, scale=a.scale)
    for heads, d in ((8, 8), (8, 16)):
        measure("reddit", rowptr, col, n, heads, d)
    del rowptr, col
    torch.cuda.empty_cache()
    rowptr, col, n = synth.dataset_like("products", device=dev, scale=a.scale)
    measure("products", rowptr, col, n, 8, 16)


if __name__ == "__main__":
    main()
