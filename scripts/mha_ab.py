#!/usr/bin/env python3
"""A/B of the sparse multi-head dot-product attention operator with separate keys and values (isplib_amd.mha_matmul: isplib_mha_csr_hip
and its two backward kernels) on the Reddit-shaped synthetic graph and the ogbn-products shape (bench.py's graphs) at (H, d) = (8, 8)
and (8, 16), fp32, scale 1 / sqrt(d), forward alone and forward + backward with all gradients.

Contenders, launched alternating, `--runs` runs each; a run is a number of steps between two device events after a warm-up of all:
  mha       mha_matmul(adj, q, k, v, heads): three different tensors;
  mha k=v   mha_matmul(adj, q, k, k, heads): what baseline (b) computes, in one launch;
  (b) attn  with k = v, H calls of attention_matmul on column views of q and k (one head per call), concatenated;
  (c) gatv2 gatv2_matmul(adj, x, att, y, heads) on the same shapes: the sibling whose step is closest (one gather per edge, not two);
  (a) composed  the composition under torch autograd: index q and k into [nnz, H, d], multiply and reduce into [H, nnz], a scatter
            softmax from torch scatter ops, H weighted isplib_amd.matmul calls on column views of v.  Structure arrays are built once.
The four operator forms are measured on the whole graph.  Where the composition's [nnz, K] arrays do not fit in the free device memory
(COPIES of them are assumed alive at the peak, as in scripts/gatv2_ab.py) it is measured on the graph's first R rows (all columns
kept), with mha_matmul on the SAME R rows beside it, and the line says so; if it still runs out of memory R is halved.  Peak device
memory of one step beyond what is allocated before it (operands, structure, plans) is reported for each form, and once per shape,
untimed, the largest |difference| of z and of the gradients between the operator and the composition.

--kernels: no timing; 5 steps of mha_matmul and 5 of gatv2_matmul, forward + backward with all gradients, alternating, on the Reddit
shape at both configurations -- the workload of the per-kernel record, run under the profiler in a run of its own:
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python3 scripts/mha_ab.py --kernels

usage: python3 scripts/mha_ab.py [--runs 5] [--reps 3] [--op-reps 20] [--scale 1.0] [--shapes reddit,products] [--out FILE] [--kernels]"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SLOPE = 0.2
COPIES = 7            # [nnz, K] fp32 arrays assumed alive at the composition's peak under autograd (scripts/gatv2_ab.py)
CONFIGS = ((8, 8), (8, 16))


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--runs", type=int, default=5)
    p.add_argument("--reps", type=int, default=3, help="steps per run of the composition (a step is up to a second)")
    p.add_argument("--op-reps", type=int, default=20, help="steps per run of the operator forms")
    p.add_argument("--scale", type=float, default=1.0, help="shrink the graphs (rehearsal only)")
    p.add_argument("--shapes", default="reddit,products")
    p.add_argument("--out", default="")
    p.add_argument("--kernels", action="store_true", help="the workload of the per-kernel record (run it under rocprofv3), untimed")
    a = p.parse_args()
    if not torch.cuda.is_available():
        sys.exit("mha_ab.py measures on the GPU: none is visible")
    import isplib_amd
    from isplib_amd import synth
    dev = torch.device("cuda:0")
    lines = [f"# scripts/mha_ab.py: fp32, scale 1/sqrt(d), {a.runs} alternating runs; a run is {a.op_reps} steps of an operator form, "
             f"{a.reps} of the composition; ms per step",
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
            emit(f"   {what:17s}{name:13s}" + " ".join(f"{t:9.3f}" for t in times[name]) +
                 f"   min {min(times[name]):.3f} max {max(times[name]):.3f}   peak beyond operands {peaks[name] / 2 ** 20:.1f} MiB")
        return times, peaks

    def ratio(what, times, num, den):
        x, y = times[num], times[den]
        emit(f"   {what}: {num} / {den} min/min {min(x) / min(y):.3f} (max/max {max(x) / max(y):.3f}); every {num} run below every {den} "
             f"run: {'yes' if max(x) < min(y) else 'NO'}; run-to-run spread max/min {num} {max(x) / min(x):.3f}, {den} {max(y) / min(y):.3f}")

    def composition_rows(rowptr, n, k):
        free = torch.cuda.mem_get_info()[0]
        nnz = int(rowptr[-1])
        if COPIES * nnz * k * 4 <= 0.85 * free:
            return n
        cap = int(0.5 * free / (COPIES * k * 4))
        return max(1, int(torch.searchsorted(rowptr, torch.tensor([cap], device=rowptr.device), right=True)[0]) - 1)

    def measure(tag, rowptr, col, n, heads, d):
        kk = heads * d
        scale = 1.0 / d ** 0.5
        q = synth.features(n, kk, seed=2, device=dev).requires_grad_(True)
        k = synth.features(n, kk, seed=3, device=dev).requires_grad_(True)
        v = synth.features(n, kk, seed=4, device=dev).requires_grad_(True)
        att = (synth.features(heads, d, seed=7, device=dev) / d ** 0.5).requires_grad_(True)
        g = synth.features(n, kk, seed=5, device=dev)
        leaves = (q, k, v, att)
        adj = isplib_amd.SparseTensor.from_csr(rowptr, col, None, (n, n), validate=False)
        emit(f"{tag} operator forms on the whole graph: n={n} nnz={col.numel()} H={heads} d={d} ([n, K] fp32 = "
             f"{n * kk * 4 / 2 ** 20:.1f} MiB)")

        def attention_per_head():
            return torch.cat([isplib_amd.attention_matmul(adj, q[:, h * d:(h + 1) * d], k[:, h * d:(h + 1) * d], scale)
                              for h in range(heads)], 1)

        for what, grad in (("forward", False), ("forward+backward", True)):
            times, _ = alternate(what, [
                ("mha", step(lambda: isplib_amd.mha_matmul(adj, q, k, v, heads), leaves, g, grad), a.op_reps),
                ("mha k=v", step(lambda: isplib_amd.mha_matmul(adj, q, k, k, heads), leaves, g, grad), a.op_reps),
                ("(b) attn", step(attention_per_head, leaves, g, grad), a.op_reps),
                ("(c) gatv2", step(lambda: isplib_amd.gatv2_matmul(adj, q, att, k, heads=heads, negative_slope=SLOPE), leaves, g, grad),
                 a.op_reps)], leaves)
            ratio(what, times, "mha k=v", "(b) attn")
            ratio(what, times, "mha", "(c) gatv2")
            torch.cuda.empty_cache()
        del adj
        torch.cuda.empty_cache()

        rows = composition_rows(rowptr, n, kk)
        while True:
            rp = rowptr[:rows + 1].contiguous()
            cl = col[:int(rp[-1])].contiguous()
            nnz = cl.numel()
            sub = isplib_amd.SparseTensor.from_csr(rp, cl, None, (rows, n), validate=False)
            row = sub.storage.row()
            w_a = [isplib_amd.SparseTensor.from_csr(rp, cl, torch.ones(nnz, device=dev), (rows, n), validate=False) for _ in range(heads)]
            qr = q.detach()[:rows].clone().requires_grad_(True)
            gr = g[:rows].contiguous()
            sub_leaves = (qr, k, v)

            def composed_fw():
                s = ((qr.view(rows, heads, d)[row] * k.view(n, heads, d)[cl]).sum(2) * scale).t().contiguous()          # [H, nnz]
                top = torch.full((heads, rows), float("-inf"), device=dev).scatter_reduce(1, row.expand(heads, nnz), s.detach(), "amax",
                                                                                           include_self=True)
                w = torch.exp(s - top[:, row])
                aa = w / torch.zeros(heads, rows, device=dev).index_add(1, row, w)[:, row]
                out = []
                for h in range(heads):
                    w_a[h].storage._value = aa[h]
                    out.append(isplib_amd.matmul(w_a[h], v[:, h * d:(h + 1) * d], "sum"))
                return torch.cat(out, 1)

            fits = True
            try:
                step(composed_fw, sub_leaves, gr, True)()            # the largest step first: does it fit?
                torch.cuda.synchronize()
            except torch.cuda.OutOfMemoryError:
                fits = False
            if fits or rows <= 1:
                break
            del sub, w_a, row, qr, gr, rp, cl                        # outside the handler: the traceback no longer holds the step's arrays
            k.grad = v.grad = None
            torch.cuda.empty_cache()
            rows //= 2
        whole = "the whole graph" if rows == n else f"the graph's FIRST {rows} ROWS (all columns kept), composition AND operator"
        emit(f"{tag} (a) composition vs mha on {whole}: rows={rows} nnz={nnz} H={heads} d={d} ([nnz, K] fp32 = "
             f"{nnz * kk * 4 / 2 ** 20:.1f} MiB, [H, nnz] fp32 = {heads * nnz * 4 / 2 ** 20:.1f} MiB)")
        for what, grad in (("forward", False), ("forward+backward", True)):
            times, _ = alternate(what, [
                ("(a) composed", step(composed_fw, sub_leaves, gr, grad), a.reps),
                ("mha", step(lambda: isplib_amd.mha_matmul(sub, qr, k, v, heads), sub_leaves, gr, grad), a.op_reps)], sub_leaves)
            ratio(what, times, "mha", "(a) composed")
            torch.cuda.empty_cache()
        for t in sub_leaves:
            t.grad = None
        zc = composed_fw()
        zc.backward(gr)
        want = [t.detach().clone() for t in (zc, qr.grad, k.grad, v.grad)]
        del zc
        for t in sub_leaves:
            t.grad = None
        zo = isplib_amd.mha_matmul(sub, qr, k, v, heads)
        zo.backward(gr)
        got = (zo.detach(), qr.grad, k.grad, v.grad)
        emit(f"   operator vs composition: max |z difference| {float((got[0] - want[0]).abs().max()):.3g}, max |gradient difference| "
             f"{max(float((x - y).abs().max()) for x, y in zip(got[1:], want[1:])):.3g}")
        del sub, w_a, row, qr, gr, q, k, v, att, g, want, got, zo
        torch.cuda.empty_cache()

    if a.kernels:
        rowptr, col, n = synth.dataset_like("reddit", device=dev, scale=a.scale)
        adj = isplib_amd.SparseTensor.from_csr(rowptr, col, None, (n, n), validate=False)
        for heads, d in CONFIGS:
            q, k, v, g = (synth.features(n, heads * d, seed=s, device=dev) for s in (2, 3, 4, 5))
            att = (synth.features(heads, d, seed=7, device=dev) / d ** 0.5).requires_grad_(True)
            leaves = (q.requires_grad_(True), k.requires_grad_(True), v.requires_grad_(True), att)
            for _ in range(5):
                step(lambda: isplib_amd.mha_matmul(adj, q, k, v, heads), leaves, g, True)()
                step(lambda: isplib_amd.gatv2_matmul(adj, q, att, k, heads=heads, negative_slope=SLOPE), leaves, g, True)()
            torch.cuda.synchronize()
        print(f"mha_ab.py --kernels: 5 + 5 steps at each of {CONFIGS} on n={n} nnz={col.numel()}")
        return
    for name in a.shapes.split(","):
        rowptr, col, n = synth.dataset_like(name, device=dev, scale=a.scale)
        for heads, d in CONFIGS:
            measure(name, rowptr, col, n, heads, d)
        del rowptr, col
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
