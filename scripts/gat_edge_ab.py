#!/usr/bin/env python3
"""A/B of the GAT attention operator with a per-edge score term (isplib_amd.gat_matmul(..., a_edge=...): isplib_gat_edge_csr_hip and its
two backward kernels) on the shapes of scripts/gat_ab.py: the Reddit-shaped synthetic graph at (H, d) = (8, 8) and (8, 16) and the
ogbn-products shape at (8, 16) (bench.py's graphs), fp32, negative_slope 0.2, forward alone and forward + backward with all gradients.

Three forms, launched alternating, `--runs` runs each; a run is a number of steps between two device events after a warm-up of all:
  (a) with     gat_matmul with a_edge [nnz, H]; forward + backward asks for y, a_dst, a_src and a_edge;
  (b) without  gat_matmul without it, in the same process -- the operator as it was; the cost of the term is read as a / b;
  (c) composed the PyG-style composition with the edge term under torch autograd (scripts/gat_ab.py's, plus one add): index, add,
               add, leaky_relu -- an [H, nnz] array; a scatter softmax from torch scatter ops; H weighted isplib_amd.matmul calls on
               column views of y.  Every structure array is built once, before the timing.
a_edge must sit behind one buffer descriptor (isplib_gat_edge_serves: nnz * H * 4 <= 3.5 GiB).  The Reddit shape at 8 heads is 3.67 GB,
just inside; the products shape at 8 heads is 3.96 GB, outside: there (a) is the documented way out, `--split` calls of H / split heads
each on column views of y and of the scores, and the line says so.  (b) and (c) always run all heads at once.
Peak device memory of one step beyond what is allocated before it (operands, structure, plans) is reported for (a) and (c).  The
outputs of (a) and (c) are compared once per shape (two different fp32 computations: the largest |difference| is printed).

usage: python3 scripts/gat_edge_ab.py [--runs 5] [--reps 3] [--op-reps 20] [--scale 1.0] [--out FILE]"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SLOPE = 0.2


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--runs", type=int, default=5)
    p.add_argument("--reps", type=int, default=3, help="steps per run of the composition (a step is about half a second)")
    p.add_argument("--op-reps", type=int, default=20, help="steps per run of the two operator forms")
    p.add_argument("--scale", type=float, default=1.0, help="shrink the graphs (rehearsal only)")
    p.add_argument("--out", default="")
    a = p.parse_args()
    if not torch.cuda.is_available():
        sys.exit("gat_edge_ab.py measures on the GPU: none is visible")
    import isplib_amd
    from isplib_amd import cabi, synth
    dev = torch.device("cuda:0")
    lines = [f"# scripts/gat_edge_ab.py: fp32, negative_slope {SLOPE}, {a.runs} alternating runs; a run is {a.op_reps} steps of an operator "
             f"form, {a.reps} of the composition; ms per step",
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
        split = 1
        while not cabi.gat_edge_serves(nnz, heads // split):
            split *= 2
        hs = heads // split                         # heads per call of (a)
        y = (synth.features(n, k, seed=3, device=dev) * 2.0).requires_grad_(True)
        a_dst = (synth.features(n, heads, seed=4, device=dev) * 2.0).requires_grad_(True)
        a_src = (synth.features(n, heads, seed=6, device=dev) * 2.0).requires_grad_(True)
        # with a split, (a) gets its a_edge as `split` dense [nnz, hs] tensors (what a caller who splits the heads holds); (c) gets the
        # same numbers as one [nnz, H] tensor
        parts = [(synth.features(nnz, hs, seed=7 + c, device=dev) * 2.0).requires_grad_(True) for c in range(split)]
        whole = parts[0] if split == 1 else torch.cat([t.detach() for t in parts], 1).requires_grad_(True)
        g = synth.features(n, k, seed=5, device=dev)
        adj = isplib_amd.SparseTensor.from_csr(rowptr, col, None, (n, n), validate=False)
        row = adj.storage.row()
        w_a = [isplib_amd.SparseTensor.from_csr(rowptr, col, torch.ones(nnz, device=dev), (n, n), validate=False) for _ in range(heads)]

        def composed_fw():
            s = torch.nn.functional.leaky_relu(a_dst.t()[:, row] + a_src.t()[:, col] + whole.t(), SLOPE)      # [H, nnz]
            top = torch.full((heads, n), float("-inf"), device=dev).scatter_reduce(1, row.expand(heads, nnz), s.detach(), "amax",
                                                                                    include_self=True)
            w = torch.exp(s - top[:, row])
            att = w / torch.zeros(heads, n, device=dev).index_add(1, row, w)[:, row]
            out = []
            for h in range(heads):
                w_a[h].storage._value = att[h]
                out.append(isplib_amd.matmul(w_a[h], y[:, h * d:(h + 1) * d], "sum"))
            return torch.cat(out, 1)

        def with_fw():
            if split == 1:
                return isplib_amd.gat_matmul(adj, y, a_dst, a_src, heads=heads, negative_slope=SLOPE, a_edge=parts[0])
            return torch.cat([isplib_amd.gat_matmul(adj, y[:, c * hs * d:(c + 1) * hs * d], a_dst[:, c * hs:(c + 1) * hs],
                                                    a_src[:, c * hs:(c + 1) * hs], heads=hs, negative_slope=SLOPE, a_edge=parts[c])
                              for c in range(split)], 1)

        def without_fw():
            return isplib_amd.gat_matmul(adj, y, a_dst, a_src, heads=heads, negative_slope=SLOPE)

        def clear():
            y.grad = a_dst.grad = a_src.grad = whole.grad = None
            for t in parts:
                t.grad = None

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

        def grads(name):
            e = whole.grad if name == "composed" else (parts[0].grad if split == 1 else torch.cat([t.grad for t in parts], 1))
            return tuple(t.clone() for t in (y.grad, a_dst.grad, a_src.grad, e))

        emit(f"{tag} n={n} nnz={nnz} H={heads} d={d}  a_edge = {nnz * heads * 4 / 1e9:.2f} GB" +
             (f": outside isplib_gat_edge_serves at {heads} heads -- (a) is {split} calls of {hs} heads on column views" if split > 1 else
              ": inside isplib_gat_edge_serves, (a) is one call"))
        for what, grad in (("forward", False), ("forward+backward", True)):
            forms = [("composed", step(composed_fw, grad), a.reps), ("without", step(without_fw, grad), a.op_reps),
                     ("with", step(with_fw, grad), a.op_reps)]
            outs = {}
            for name, fn, _ in forms:               # warm-up: loads the code objects, builds the plans and the transposed structure
                outs[name] = fn().detach().clone()
                if grad and name != "without":
                    outs[name + "_g"] = grads(name)
            peaks = {}
            for name, fn, _ in forms:               # the gradients of the step before are not operands: dropped before the base is read
                clear()
                peaks[name] = peak_bytes(fn)
            times = {name: [] for name, _, _ in forms}
            for _ in range(a.runs):
                for name, fn, reps in forms:
                    times[name].append(timed(fn, reps))
            diff = float((outs["with"] - outs["composed"]).abs().max())
            gdiff = max((float((u - v).abs().max()) for u, v in zip(outs.get("with_g", ()), outs.get("composed_g", ()))), default=0.0)
            for name in ("composed", "without", "with"):
                emit(f"   {what:17s}{name:9s}" + " ".join(f"{t:9.3f}" for t in times[name]) +
                     f"   min {min(times[name]):.3f} max {max(times[name]):.3f}   peak beyond operands {peaks[name] / 2 ** 20:.1f} MiB")
            lo = {name: min(times[name]) for name in times}
            emit(f"   {what}: (a) with / (b) without min/min {lo['with'] / lo['without']:.3f} (max/max "
                 f"{max(times['with']) / max(times['without']):.3f}); (a) with / (c) composed min/min {lo['with'] / lo['composed']:.3f}; every (a) "
                 f"run below every (c) run: {'yes' if max(times['with']) < min(times['composed']) else 'NO'}; (a) vs (c) max |z difference| "
                 f"{diff:.3g}" + (f", max |gradient difference| {gdiff:.3g}" if grad else "") +
                 f" ([nnz, H] fp32 = {heads * nnz * 4 / 2 ** 20:.1f} MiB, [n, K] fp32 = {n * k * 4 / 2 ** 20:.1f} MiB)")
            del outs, forms
            torch.cuda.empty_cache()
        del adj, w_a, y, a_dst, a_src, parts, whole, g
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
