#!/usr/bin/env python3
"""A/B of the GAT attention operator (isplib_amd.gat_matmul: isplib_gat_csr_hip and its two backward kernels, all heads in one launch)
against the composition a caller had before it, on the Reddit-shaped synthetic graph at (H, d) = (8, 8) and (8, 16) and the
ogbn-products shape at (8, 16) (bench.py's graphs), fp32, negative_slope 0.2, forward alone and forward + backward.

The composition, with torch autograd through all of it and every structure array (row ids, colptr, csr2csc, plans) built once, before
the timing:
  1. scores   s[h, e] = leaky_relu(a_dst[i, h] + a_src[j, h]): two index ops, an add and leaky_relu -- an [H, nnz] array;
  2. softmax  over the entries of a row, per head, from torch scatter ops: scatter_reduce(amax), exp, index_add, a division -- four
              passes over [H, nnz] arrays;
  3. z[:, head h] = A(a[h]) y[:, head h]: H weighted isplib_amd.matmul calls on column views of y, whose own backward is an SDDMM
              (da) and a weighted SpMM on A^T (dy) each.
Autograd keeps s, a and the softmax's intermediates: several [H, nnz] tensors.  The operator keeps y, the scores, z and one scalar per
row and head.

Both forms are launched alternating, `--runs` runs each; a run is `--reps` steps between two device events after a warm-up of both.
Peak device memory of one step beyond what is allocated before it (operands, structure, plans) is reported for both.  The outputs
are compared once per shape (they are two different fp32 computations: the largest |difference| is printed).

usage: python3 scripts/gat_ab.py [--runs 5] [--reps 5] [--scale 1.0] [--out FILE]"""
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
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--scale", type=float, default=1.0, help="shrink the graphs (rehearsal only)")
    p.add_argument("--out", default="")
    a = p.parse_args()
    if not torch.cuda.is_available():
        sys.exit("gat_ab.py measures on the GPU: none is visible")
    import isplib_amd
    from isplib_amd import synth
    dev = torch.device("cuda:0")
    lines = [f"# scripts/gat_ab.py: fp32, negative_slope {SLOPE}, {a.runs} alternating runs x {a.reps} steps, ms per step",
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
        # the composition's structure, built once: row ids and one weighted graph per head whose values are swapped per step
        row = adj.storage.row()
        w_a = [isplib_amd.SparseTensor.from_csr(rowptr, col, torch.ones(nnz, device=dev), (n, n), validate=False) for _ in range(heads)]

        def composed_fw(yy, dst, src):
            s = torch.nn.functional.leaky_relu(dst.t()[:, row] + src.t()[:, col], SLOPE)                     # [H, nnz]
            top = torch.full((heads, n), float("-inf"), device=dev).scatter_reduce(1, row.expand(heads, nnz), s.detach(), "amax",
                                                                                    include_self=True)
            w = torch.exp(s - top[:, row])
            att = w / torch.zeros(heads, n, device=dev).index_add(1, row, w)[:, row]
            out = []
            for h in range(heads):
                w_a[h].storage._value = att[h]
                out.append(isplib_amd.matmul(w_a[h], yy[:, h * d:(h + 1) * d], "sum"))
            return torch.cat(out, 1)

        def fused_fw(yy, dst, src):
            return isplib_amd.gat_matmul(adj, yy, dst, src, heads=heads, negative_slope=SLOPE)

        def step(fw, grad):
            def run():
                y.grad = a_dst.grad = a_src.grad = None
                if not grad:
                    with torch.no_grad():
                        return fw(y, a_dst, a_src)
                out = fw(y, a_dst, a_src)
                out.backward(g)
                return out
            return run

        emit(f"{tag} n={n} nnz={nnz} H={heads} d={d}")
        for what, grad in (("forward", False), ("forward+backward", True)):
            forms = [("composed", step(composed_fw, grad)), ("operator", step(fused_fw, grad))]
            outs = {}
            for name, fn in forms:                  # warm-up: loads the code objects, builds the plans and the transposed structure
                outs[name] = fn().detach().clone()
                outs[name + "_g"] = (y.grad.clone(), a_dst.grad.clone(), a_src.grad.clone()) if grad else ()
            peaks = {name: peak_bytes(fn) for name, fn in forms}
            times = {name: [] for name, _ in forms}
            for _ in range(a.runs):
                for name, fn in forms:
                    times[name].append(timed(fn, a.reps))
            diff = float((outs["operator"] - outs["composed"]).abs().max())
            gdiff = max((float((u - v).abs().max()) for u, v in zip(outs["operator_g"], outs["composed_g"])), default=0.0)
            for name in ("composed", "operator"):
                emit(f"   {what:17s}{name:9s}" + " ".join(f"{t:9.3f}" for t in times[name]) +
                     f"   min {min(times[name]):.3f} max {max(times[name]):.3f}   peak beyond operands {peaks[name] / 2 ** 20:.1f} MiB")
            wins = max(times["operator"]) < min(times["composed"])
            emit(f"   {what}: operator / composed min/min {min(times['operator']) / min(times['composed']):.3f}; every operator run below every "
                 f"composed run: {'yes' if wins else 'NO'}; max |z difference| {diff:.3g}" + (f", max |gradient difference| {gdiff:.3g}" if grad else "") +
                 f" ([H, nnz] fp32 = {heads * nnz * 4 / 2 ** 20:.1f} MiB, [n, K] fp32 = {n * k * 4 / 2 ** 20:.1f} MiB)")
            del outs, forms
            torch.cuda.empty_cache()
        del adj, w_a, y, a_dst, a_src, g
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
