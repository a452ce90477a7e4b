#!/usr/bin/env python3
"""A/B of the GATv2 attention operator (isplib_amd.gatv2_matmul: isplib_gatv2_csr_hip and its two backward kernels, all heads in one
launch) on the Reddit-shaped synthetic graph at (H, d) = (8, 8) and (8, 16) and the ogbn-products shape at (8, 16) (bench.py's graphs),
fp32, negative_slope 0.2, forward alone and forward + backward.  Two comparisons; both are records, nothing is gated on either.

(a) Against the plain composition a caller had before it, with torch autograd through all of it and every structure array (row ids,
    colptr, csr2csc, plans) built once, before the timing:
      1. u = x[row] + y[col] as [nnz, H, d] (two index ops and an add), v = leaky_relu(u) -- [nnz, K] arrays;
      2. s[h, e] = sum_c att[h, c] v[e, h, c]: a product [nnz, K] and a sum -- an [H, nnz] array;
      3. softmax over the entries of a row, per head, from torch scatter ops: scatter_reduce(amax), exp, index_add, a division;
      4. z[:, head h] = A(a[h]) y[:, head h]: H weighted isplib_amd.matmul calls on column views of y.
    Autograd keeps u, v and the softmax's intermediates.  Where the composition's [nnz, K] arrays do not fit in the device memory that
    is free (COPIES of them are assumed alive at the peak), the composition is measured on the graph's first R rows (all columns kept)
    and the operator on the SAME R rows beside it; the line of the shape says so.  If the composition still runs out of memory, R is
    halved for both.
(b) Against isplib_amd.gat_matmul (GAT v1) on the same, whole shapes: what v2 costs over v1.

Both forms of a comparison are launched alternating, `--runs` runs each; a run is `--reps` steps between two device events after a
warm-up of both.  Peak device memory of one step beyond what is allocated before it (operands, structure, plans) is reported.

usage: python3 scripts/gatv2_ab.py [--runs 5] [--reps 5] [--scale 1.0] [--out FILE]"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SLOPE = 0.2
COPIES = 7            # [nnz, K] fp32 arrays assumed alive at the composition's peak under autograd (x[row], y[col], u, v, v * att and gradients)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--runs", type=int, default=5)
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--scale", type=float, default=1.0, help="shrink the graphs (rehearsal only)")
    p.add_argument("--out", default="")
    a = p.parse_args()
    if not torch.cuda.is_available():
        sys.exit("gatv2_ab.py measures on the GPU: none is visible")
    import isplib_amd
    from isplib_amd import synth
    dev = torch.device("cuda:0")
    lines = [f"# scripts/gatv2_ab.py: fp32, negative_slope {SLOPE}, {a.runs} alternating runs x {a.reps} steps, ms per step",
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

    def alternate(what, forms, leaves, grad, note):
        """forms: two (name, fn); warm-up, peak and `runs` alternating timed runs; -> the min of each."""
        outs = {}
        for name, fn in forms:                      # warm-up: loads the code objects, builds the plans and the transposed structure
            outs[name] = fn().detach().clone()
            outs[name + "_g"] = tuple(t.grad.clone() for t in leaves if t.grad is not None) if grad else ()
        peaks = {name: peak_bytes(fn) for name, fn in forms}
        times = {name: [] for name, _ in forms}
        for _ in range(a.runs):
            for name, fn in forms:
                times[name].append(timed(fn, a.reps))
        for name, _ in forms:
            emit(f"   {what:17s}{name:12s}" + " ".join(f"{t:9.3f}" for t in times[name]) +
                 f"   min {min(times[name]):.3f} max {max(times[name]):.3f}   peak beyond operands {peaks[name] / 2 ** 20:.1f} MiB")
        (n0, _), (n1, _) = forms
        tail = ""
        if note == "same":                          # two fp32 computations of one function
            diff = float((outs[n1] - outs[n0]).abs().max())
            gdiff = max((float((u - v).abs().max()) for u, v in zip(outs[n1 + "_g"], outs[n0 + "_g"])), default=0.0)
            tail = f"; max |z difference| {diff:.3g}" + (f", max |gradient difference| {gdiff:.3g}" if grad else "")
        wins = max(times[n1]) < min(times[n0])
        emit(f"   {what}: {n1} / {n0} min/min {min(times[n1]) / min(times[n0]):.3f}; every {n1} run below every {n0} run: "
             f"{'yes' if wins else 'NO'}{tail}")
        del outs
        torch.cuda.empty_cache()

    def steps(fw, leaves, g, grad):
        def run():
            for t in leaves:
                t.grad = None
            if not grad:
                with torch.no_grad():
                    return fw()
            out = fw()
            out.backward(g)
            return out
        return run

    def composition_rows(rowptr, n, k):
        """All n rows if COPIES [nnz, K] fp32 arrays fit in 0.85 of the free device memory, else the first R rows whose COPIES arrays fit
        in half of it."""
        free = torch.cuda.mem_get_info()[0]
        nnz = int(rowptr[-1])
        if COPIES * nnz * k * 4 <= 0.85 * free:
            return n
        cap = int(0.5 * free / (COPIES * k * 4))
        return max(1, int(torch.searchsorted(rowptr, torch.tensor([cap], device=rowptr.device), right=True)[0]) - 1)

    def compare_composition(tag, rowptr, col, n, heads, d, x, y, att, g):
        k = heads * d
        rows = composition_rows(rowptr, n, k)
        while True:
            rp = rowptr[:rows + 1].contiguous()
            cl = col[:int(rp[-1])].contiguous()
            nnz = cl.numel()
            adj = isplib_amd.SparseTensor.from_csr(rp, cl, None, (rows, n), validate=False)
            row = adj.storage.row()
            w_a = [isplib_amd.SparseTensor.from_csr(rp, cl, torch.ones(nnz, device=dev), (rows, n), validate=False) for _ in range(heads)]
            xr = x.detach()[:rows].clone().requires_grad_(True)
            gr = g[:rows].contiguous()
            leaves = (xr, y, att)

            def composed_fw():
                v = torch.nn.functional.leaky_relu(xr.view(rows, heads, d)[row] + y.view(n, heads, d)[cl], SLOPE)      # [nnz, H, d]
                s = (v * att[None]).sum(2).t().contiguous()                                                                  # [H, nnz]
                top = torch.full((heads, rows), float("-inf"), device=dev).scatter_reduce(1, row.expand(heads, nnz), s.detach(), "amax",
                                                                                           include_self=True)
                w = torch.exp(s - top[:, row])
                aa = w / torch.zeros(heads, rows, device=dev).index_add(1, row, w)[:, row]
                out = []
                for h in range(heads):
                    w_a[h].storage._value = aa[h]
                    out.append(isplib_amd.matmul(w_a[h], y[:, h * d:(h + 1) * d], "sum"))
                return torch.cat(out, 1)

            def fused_fw():
                return isplib_amd.gatv2_matmul(adj, xr, att, y, heads=heads, negative_slope=SLOPE)

            fits = True
            try:
                steps(composed_fw, leaves, gr, True)()           # the largest step first: does it fit?
                torch.cuda.synchronize()
            except torch.cuda.OutOfMemoryError:
                fits = False
            if fits or rows <= 1:
                break
            del adj, w_a, row, xr, gr, rp, cl                    # outside the handler: the traceback no longer holds the step's arrays
            y.grad = att.grad = None
            torch.cuda.empty_cache()
            rows //= 2
        whole = "the whole graph" if rows == n else f"the graph's FIRST {rows} ROWS (all columns kept), composition AND operator"
        emit(f"{tag} (a) composition vs operator on {whole}: rows={rows} nnz={nnz} H={heads} d={d} ([nnz, K] fp32 = "
             f"{nnz * k * 4 / 2 ** 20:.1f} MiB, [n, K] fp32 = {n * k * 4 / 2 ** 20:.1f} MiB)")
        for what, grad in (("forward", False), ("forward+backward", True)):
            alternate(what, [("composed", steps(composed_fw, leaves, gr, grad)), ("operator", steps(fused_fw, leaves, gr, grad))], leaves, grad,
                      "same")
        del adj, w_a, row, xr, gr
        torch.cuda.empty_cache()

    def compare_gat(tag, rowptr, col, n, heads, d, x, y, att, g):
        adj = isplib_amd.SparseTensor.from_csr(rowptr, col, None, (n, n), validate=False)
        a_dst = (synth.features(n, heads, seed=4, device=dev) * 2.0).requires_grad_(True)
        a_src = (synth.features(n, heads, seed=6, device=dev) * 2.0).requires_grad_(True)
        leaves = (x, y, att, a_dst, a_src)
        emit(f"{tag} (b) gat_matmul vs gatv2_matmul on the whole graph: n={n} nnz={col.numel()} H={heads} d={d}")
        for what, grad in (("forward", False), ("forward+backward", True)):
            alternate(what, [("gat_matmul", steps(lambda: isplib_amd.gat_matmul(adj, y, a_dst, a_src, heads=heads, negative_slope=SLOPE),
                                                  leaves, g, grad)),
                             ("gatv2_matmul", steps(lambda: isplib_amd.gatv2_matmul(adj, x, att, y, heads=heads, negative_slope=SLOPE),
                                                    leaves, g, grad))], leaves, grad, "other")
        del adj, a_dst, a_src
        torch.cuda.empty_cache()

    def measure(tag, rowptr, col, n, heads, d):
        k = heads * d
        x = synth.features(n, k, seed=2, device=dev).requires_grad_(True)
        y = synth.features(n, k, seed=3, device=dev).requires_grad_(True)
        att = (synth.features(heads, d, seed=7, device=dev) / d ** 0.5).requires_grad_(True)
        g = synth.features(n, k, seed=5, device=dev)
        compare_gat(tag, rowptr, col, n, heads, d, x, y, att, g)
        compare_composition(tag, rowptr, col, n, heads, d, x, y, att, g)
        del x, y, att, g
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
