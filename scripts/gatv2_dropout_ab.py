#!/usr/bin/env python3
"""A/B of the GATv2 attention operator with attention dropout (isplib_amd.gatv2_matmul(..., dropout=p): isplib_gatv2_drop_csr_hip and
its two backward kernels, the mask regenerated from the seed) on the shapes of scripts/gatv2_ab.py: the Reddit-shaped synthetic graph at
(H, d) = (8, 8) and (8, 16) and the ogbn-products shape at (8, 16) (bench.py's graphs), fp32, negative_slope 0.2, p = 0.6, forward alone
and forward + backward with all gradients.

Three forms, launched alternating, `--runs` runs each; a run is a number of steps between two device events after a warm-up of all:
  (a) dropout  gatv2_matmul with dropout=p and seed=None: every step draws its seed from torch's CPU generator, as a training loop does;
  (b) without  gatv2_matmul without it, in the same process -- the operator as it was; the cost of the mask is read as a / b;
  (c) composed the PyG-style composition under torch autograd (scripts/gatv2_ab.py's) with F.dropout ON THE COEFFICIENTS: index, add,
               leaky_relu into [nnz, H, d]; the att contraction into [H, nnz]; a scatter softmax from torch scatter ops; F.dropout of
               the [H, nnz] coefficients; H weighted isplib_amd.matmul calls on column views of y.  Structure arrays are built once.
(a) and (b) are measured on the whole graph.  Where the composition's [nnz, K] arrays do not fit in the free device memory (COPIES of
them are assumed alive at the peak, as in gatv2_ab.py) it is measured on the graph's first R rows (all columns kept), with (a) on the
SAME R rows beside it, and the line says so; if it still runs out of memory R is halved.  Peak device memory of one step beyond what is
allocated before it (operands, structure, plans) is reported for each form.  (a) and (c) draw different masks, so their outputs are not
comparable; once per shape, untimed, the composition is run with the operator's own mask (isplib_amd.gat_dropout_mask on the device, in
place of F.dropout) against the operator under the same seed, and the largest |difference| of z and of the gradients is printed.

usage: python3 scripts/gatv2_dropout_ab.py [--runs 5] [--reps 3] [--op-reps 20] [--scale 1.0] [--out FILE]"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SLOPE = 0.2
P = 0.6
COPIES = 7            # [nnz, K] fp32 arrays assumed alive at the composition's peak under autograd (scripts/gatv2_ab.py)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--runs", type=int, default=5)
    p.add_argument("--reps", type=int, default=3, help="steps per run of the composition (a step is up to a second)")
    p.add_argument("--op-reps", type=int, default=20, help="steps per run of the two operator forms")
    p.add_argument("--scale", type=float, default=1.0, help="shrink the graphs (rehearsal only)")
    p.add_argument("--out", default="")
    a = p.parse_args()
    if not torch.cuda.is_available():
        sys.exit("gatv2_dropout_ab.py measures on the GPU: none is visible")
    import isplib_amd
    from isplib_amd import cabi, synth
    dev = torch.device("cuda:0")
    lines = [f"# scripts/gatv2_dropout_ab.py: fp32, negative_slope {SLOPE}, p = {P}, {a.runs} alternating runs; a run is {a.op_reps} steps of "
             f"an operator form, {a.reps} of the composition; ms per step",
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

    def step(fw, leaves, g, grad):
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

    def alternate(what, forms, leaves):
        """forms: (name, fn, reps); warm-up, peak and `runs` alternating timed runs; -> times, peaks"""
        for _, fn, _ in forms:                      # warm-up: loads the code objects, builds the plans and the transposed structure
            fn()
        peaks = {}
        for name, fn, _ in forms:                   # the gradients of the step before are not operands: dropped before the base is read
            for t in leaves:
                t.grad = None
            peaks[name] = peak_bytes(fn)
        times = {name: [] for name, _, _ in forms}
        for _ in range(a.runs):
            for name, fn, reps in forms:
                times[name].append(timed(fn, reps))
        for name, _, _ in forms:
            emit(f"   {what:17s}{name:9s}" + " ".join(f"{t:9.3f}" for t in times[name]) +
                 f"   min {min(times[name]):.3f} max {max(times[name]):.3f}   peak beyond operands {peaks[name] / 2 ** 20:.1f} MiB")
        return times, peaks

    def composition_rows(rowptr, n, k):
        free = torch.cuda.mem_get_info()[0]
        nnz = int(rowptr[-1])
        if COPIES * nnz * k * 4 <= 0.85 * free:
            return n
        cap = int(0.5 * free / (COPIES * k * 4))
        return max(1, int(torch.searchsorted(rowptr, torch.tensor([cap], device=rowptr.device), right=True)[0]) - 1)

    def measure(tag, rowptr, col, n, heads, d):
        k = heads * d
        x = synth.features(n, k, seed=2, device=dev).requires_grad_(True)
        y = synth.features(n, k, seed=3, device=dev).requires_grad_(True)
        att = (synth.features(heads, d, seed=7, device=dev) / d ** 0.5).requires_grad_(True)
        g = synth.features(n, k, seed=5, device=dev)
        leaves = (x, y, att)
        adj = isplib_amd.SparseTensor.from_csr(rowptr, col, None, (n, n), validate=False)
        emit(f"{tag} (a) dropout vs (b) without on the whole graph: n={n} nnz={col.numel()} H={heads} d={d} ([n, K] fp32 = "
             f"{n * k * 4 / 2 ** 20:.1f} MiB, csr2csc = {col.numel() * 8 / 2 ** 20:.1f} MiB)")
        for what, grad in (("forward", False), ("forward+backward", True)):
            times, peaks = alternate(what, [
                ("without", step(lambda: isplib_amd.gatv2_matmul(adj, x, att, y, heads=heads, negative_slope=SLOPE), leaves, g, grad), a.op_reps),
                ("dropout", step(lambda: isplib_amd.gatv2_matmul(adj, x, att, y, heads=heads, negative_slope=SLOPE, dropout=P), leaves, g, grad),
                 a.op_reps)], leaves)
            b, aa = times["without"], times["dropout"]
            emit(f"   {what}: (a) dropout / (b) without min/min {min(aa) / min(b):.3f} (max/max {max(aa) / max(b):.3f}); run-to-run spread of "
                 f"(b) max/min {max(b) / min(b):.3f}, of (a) {max(aa) / min(aa):.3f}; peak (a) - peak (b) = "
                 f"{(peaks['dropout'] - peaks['without']) / 2 ** 20:.1f} MiB")
            torch.cuda.empty_cache()
        del adj
        torch.cuda.empty_cache()

        rows = composition_rows(rowptr, n, k)
        while True:
            rp = rowptr[:rows + 1].contiguous()
            cl = col[:int(rp[-1])].contiguous()
            nnz = cl.numel()
            sub = isplib_amd.SparseTensor.from_csr(rp, cl, None, (rows, n), validate=False)
            row = sub.storage.row()
            w_a = [isplib_amd.SparseTensor.from_csr(rp, cl, torch.ones(nnz, device=dev), (rows, n), validate=False) for _ in range(heads)]
            xr = x.detach()[:rows].clone().requires_grad_(True)
            gr = g[:rows].contiguous()
            sub_leaves = (xr, y, att)

            def composed_fw(keep=None):
                v = torch.nn.functional.leaky_relu(xr.view(rows, heads, d)[row] + y.view(n, heads, d)[cl], SLOPE)      # [nnz, H, d]
                s = (v * att[None]).sum(2).t().contiguous()                                                                  # [H, nnz]
                top = torch.full((heads, rows), float("-inf"), device=dev).scatter_reduce(1, row.expand(heads, nnz), s.detach(), "amax",
                                                                                           include_self=True)
                w = torch.exp(s - top[:, row])
                aa = w / torch.zeros(heads, rows, device=dev).index_add(1, row, w)[:, row]
                aa = torch.nn.functional.dropout(aa, P, True) if keep is None else aa * keep
                out = []
                for h in range(heads):
                    w_a[h].storage._value = aa[h]
                    out.append(isplib_amd.matmul(w_a[h], y[:, h * d:(h + 1) * d], "sum"))
                return torch.cat(out, 1)

            fits = True
            try:
                step(composed_fw, sub_leaves, gr, True)()            # the largest step first: does it fit?
                torch.cuda.synchronize()
            except torch.cuda.OutOfMemoryError:
                fits = False
            if fits or rows <= 1:
                break
            del sub, w_a, row, xr, gr, rp, cl                        # outside the handler: the traceback no longer holds the step's arrays
            y.grad = att.grad = None
            torch.cuda.empty_cache()
            rows //= 2
        whole = "the whole graph" if rows == n else f"the graph's FIRST {rows} ROWS (all columns kept), composition AND operator"
        emit(f"{tag} (a) dropout vs (c) composed on {whole}: rows={rows} nnz={nnz} H={heads} d={d} ([nnz, K] fp32 = "
             f"{nnz * k * 4 / 2 ** 20:.1f} MiB, [H, nnz] fp32 = {heads * nnz * 4 / 2 ** 20:.1f} MiB)")
        for what, grad in (("forward", False), ("forward+backward", True)):
            times, _ = alternate(what, [
                ("composed", step(composed_fw, sub_leaves, gr, grad), a.reps),
                ("dropout", step(lambda: isplib_amd.gatv2_matmul(sub, xr, att, y, heads=heads, negative_slope=SLOPE, dropout=P), sub_leaves, gr,
                                 grad), a.op_reps)], sub_leaves)
            c, aa = times["composed"], times["dropout"]
            emit(f"   {what}: (a) dropout / (c) composed min/min {min(aa) / min(c):.3f}; every (a) run below every (c) run: "
                 f"{'yes' if max(aa) < min(c) else 'NO'}")
            torch.cuda.empty_cache()
        # the operator against the composition with the operator's own mask, once, untimed
        seed = 20240607
        keep = (isplib_amd.gat_dropout_mask(sub, heads, P, seed).t().float() * cabi.gat_drop_scale(P)).contiguous()      # [H, nnz]: q c
        for t in sub_leaves:
            t.grad = None
        zc = composed_fw(keep)
        zc.backward(gr)
        want = [t.detach().clone() for t in (zc, xr.grad, y.grad, att.grad)]
        del zc, keep
        for t in sub_leaves:
            t.grad = None
        zo = isplib_amd.gatv2_matmul(sub, xr, att, y, heads=heads, negative_slope=SLOPE, dropout=P, seed=seed)
        zo.backward(gr)
        got = (zo.detach(), xr.grad, y.grad, att.grad)
        emit(f"   same mask (seed {seed}): operator vs composition max |z difference| {float((got[0] - want[0]).abs().max()):.3g}, max "
             f"|gradient difference| {max(float((u - v).abs().max()) for u, v in zip(got[1:], want[1:])):.3g}")
        del sub, w_a, row, xr, gr, x, y, att, g, want, got, zo
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
