#!/usr/bin/env python3
"""A/B of the row-softmax attention operator (isplib_amd.attention_matmul: isplib_attention_csr_hip and its two backward kernels)
against the composition a caller had before it, on the Reddit-shaped synthetic graph at K = 64 and 128 and the ogbn-products shape
at K = 128 (bench.py's graphs), fp32, scale = 1 / sqrt(K), forward alone and forward + backward.

The composition, with torch autograd through all of it and every structure array (row ids, colptr, csr2csc, plans) built once, before
the timing:
  1. scores   s_e = scale * <x_i, y_j>: cabi.sddmm (isplib_sddmm_csr_hip) inside an autograd Function whose backward is two weighted
              SpMMs (dx = A(ds) y, dy = A^T(ds) x) through isplib_amd.matmul;
  2. softmax  over the entries of a row from torch scatter ops: scatter_reduce(amax), exp, index_add, a division -- four passes over
              edge-length arrays;
  3. z = A(a) y: the weighted isplib_amd.matmul, whose own backward is an SDDMM (da) and a weighted SpMM on A^T (dy).
Autograd keeps s, a and the softmax's intermediates: several [nnz] tensors.  The operator keeps x, y, z and one scalar per row.

Both forms are launched alternating, `--runs` runs each; a run is `--reps` steps between two device events after a warm-up of both.
Peak device memory of one step beyond what is allocated before it (operands, structure, plans) is reported for both.  The outputs
are compared once per shape (they are two different fp32 computations: the largest |difference| is printed).

usage: python3 scripts/attention_ab.py [--runs 5] [--reps 5] [--scale 1.0] [--out FILE]"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--runs", type=int, default=5)
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--scale", type=float, default=1.0, help="shrink the graphs (rehearsal only)")
    p.add_argument("--out", default="")
    a = p.parse_args()
    if not torch.cuda.is_available():
        sys.exit("attention_ab.py measures on the GPU: none is visible")
    import isplib_amd
    from isplib_amd import cabi, synth
    dev = torch.device("cuda:0")
    lines = [f"# scripts/attention_ab.py: fp32, scale 1/sqrt(K), {a.runs} alternating runs x {a.reps} steps, ms per step",
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

    def measure(tag, rowptr, col, n, k):
        nnz = col.numel()
        scale = 1.0 / float(k) ** 0.5
        x = (synth.features(n, k, seed=3, device=dev) * 2.0).requires_grad_(True)
        y = (synth.features(n, k, seed=4, device=dev) * 2.0).requires_grad_(True)
        g = synth.features(n, k, seed=5, device=dev)
        adj = isplib_amd.SparseTensor.from_csr(rowptr, col, None, (n, n), validate=False)
        # the composition's structure, built once: row ids, the transposed structure and its permutation, weighted graphs whose
        # values are swapped per step (the storage re-permutes its A^T weights when `value` changes, nothing else is rebuilt)
        base = adj.storage
        row, perm = base.row(), base.csr2csc()
        w_a = isplib_amd.SparseTensor.from_csr(rowptr, col, torch.ones(nnz, device=dev), (n, n), validate=False)
        w_ds = isplib_amd.SparseTensor.from_csr(rowptr, col, torch.ones(nnz, device=dev), (n, n), validate=False)
        w_dst = isplib_amd.SparseTensor.from_csr(base.colptr(), base.row_t(), torch.ones(nnz, device=dev), (n, n), validate=False)

        class Scores(torch.autograd.Function):
            @staticmethod
            def forward(ctx, xx, yy):
                ctx.save_for_backward(xx, yy)
                return cabi.sddmm(rowptr, col, yy, xx, check=False)

            @staticmethod
            def backward(ctx, ds):
                xx, yy = ctx.saved_tensors
                ds = ds.contiguous()
                w_ds.storage._value = ds
                w_dst.storage._value = ds[perm]
                with torch.no_grad():
                    return isplib_amd.matmul(w_ds, yy, "sum"), isplib_amd.matmul(w_dst, xx, "sum")

        def composed_fw(xx, yy):
            s = Scores.apply(xx, yy) * scale
            top = torch.full((n,), float("-inf"), device=dev).scatter_reduce(0, row, s.detach(), "amax", include_self=True)
            w = torch.exp(s - top[row])
            att = w / torch.zeros(n, device=dev).index_add(0, row, w)[row]
            w_a.storage._value = att
            return isplib_amd.matmul(w_a, yy, "sum")

        def fused_fw(xx, yy):
            return isplib_amd.attention_matmul(adj, xx, yy)

        def step(fw, grad):
            def run():
                x.grad = y.grad = None
                if not grad:
                    with torch.no_grad():
                        return fw(x, y)
                out = fw(x, y)
                out.backward(g)
                return out
            return run

        emit(f"{tag} n={n} nnz={nnz} K={k}")
        for what, grad in (("forward", False), ("forward+backward", True)):
            forms = [("composed", step(composed_fw, grad)), ("operator", step(fused_fw, grad))]
            outs = {}
            for name, fn in forms:                  # warm-up: loads the code objects, builds the plans and the transposed structure
                outs[name] = fn().detach().clone()
                grads = (x.grad.clone(), y.grad.clone()) if grad else ()
                outs[name + "_g"] = grads
            peaks = {name: peak_bytes(fn) for name, fn in forms}
            times = {name: [] for name, _ in forms}
            for _ in range(a.runs):
                for name, fn in forms:
                    times[name].append(timed(fn, a.reps))
            diff = float((outs["operator"] - outs["composed"]).abs().max())
            gdiff = max((float((u - v).abs().max()) for u, v in zip(outs["operator_g"], outs["composed_g"])), default=0.0)
            for name in ("composed", "operator"):
                emit(f"   {what:17s}{name:9s}" + " ".join(f"{t:8.3f}" for t in times[name]) +
                     f"   min {min(times[name]):.3f} max {max(times[name]):.3f}   peak beyond operands {peaks[name] / 2 ** 20:.1f} MiB")
            wins = max(times["operator"]) < min(times["composed"])
            emit(f"   {what}: operator / composed min/min {min(times['operator']) / min(times['composed']):.3f}; every operator run below every "
                 f"composed run: {'yes' if wins else 'NO'}; max |z difference| {diff:.3g}" + (f", max |gradient difference| {gdiff:.3g}" if grad else "") +
                 f" ([nnz] fp32 = {nnz * 4 / 2 ** 20:.1f} MiB, [n, K] fp32 = {n * k * 4 / 2 ** 20:.1f} MiB)")
            del outs, forms
            torch.cuda.empty_cache()
        del adj, w_a, w_ds, w_dst, x, y, g
        torch.cuda.empty_cache()

    rowptr, col, n = synth.dataset_like("reddit", device=dev, scale=a.scale)
    for k in (64, 128):
        measure("reddit", rowptr, col, n, k)
    del rowptr, col
    torch.cuda.empty_cache()
    rowptr, col, n = synth.dataset_like("products", device=dev, scale=a.scale)
    measure("products", rowptr, col, n, 128)


if __name__ == "__main__":
    main()
