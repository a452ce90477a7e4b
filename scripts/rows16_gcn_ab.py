#!/usr/bin/env python3
"""A/B of the fused GCN layer on bf16 features: the 16-bit row kernel with the fused epilogue (fusedMM_csr_rows16_epilogue_hip, forward
and backward; ISPLIB_HALF_GCN=native) against the conversion route (ISPLIB_HALF_GCN=convert), which is what a bf16 caller had to write
by hand before: x.float() -> gcn_norm_matmul -> .to(bf16).

Shapes: scripts/rows16_ab.py's -- the ogbn-products-shaped Chung-Lu graph and its SBM twin (bench.py's config 4), K = 128 and 256, the
SBM twin both in index order (ISPLIB_REORDER=0) and in its community order; the products shape at a quarter of its size, K = 128; a
Cora-shaped graph and a fiftieth of the products shape at K = 16 and 64 -- and the Reddit shape at K = 32 and at K = 48 (the 41 classes
of the headline model padded to their 48-column pitch: K = 41 itself is odd, outside the 16-bit kernel's domain, and converts on
either route).  On the Reddit shape the conversion route's fp32 layer runs on the stream schedule.

What is timed is one forward `out = gcn_norm_matmul(adj, x, bias, relu=True)` plus `out.backward(g)`, x and bias requiring gradients.
Two forms, launched alternating, `--runs` runs each (a run = `--reps` forward + backward pairs between two device events, after a
warm-up that builds the per-graph operands).  Which route a form took is read off storage._last_schedule; the peak device memory of one
forward + backward beyond its operands is recorded for both.  The class of a call is (X beyond 256 MiB at 2 bytes per element or not,
rows in a community order or not); ISPLIB_HALF_GCN=auto may take the kernel for a class only where EVERY native run is below EVERY
convert run of every measured shape of that class (cabi.rows16_gcn_native_pays / isplib_rows16_gcn_native_pays restate the verdict
printed here; profiles/rows16_gcn_ab.txt records it).

usage: python3 scripts/rows16_gcn_ab.py [--runs 5] [--reps 5] [--scale 1.0] [--part all|big|small|reddit] [--out FILE]"""
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
    p.add_argument("--part", choices=("all", "big", "small", "reddit"), default="all", help="the shapes to measure (a long run split over calls)")
    p.add_argument("--out", default="")
    a = p.parse_args()
    if not torch.cuda.is_available():
        sys.exit("rows16_gcn_ab.py measures on the GPU: none is visible")
    import isplib_amd
    from isplib_amd import synth
    dev = torch.device("cuda:0")
    lines = [f"# scripts/rows16_gcn_ab.py --part {a.part}: bf16, gcn_norm_matmul with bias and ReLU, forward + backward, {a.runs} alternating runs x "
             f"{a.reps} pairs, ms per pair", f"# device: {torch.cuda.get_device_name(0)}"]
    verdict = {}

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

    def measure(tag, rowptr, col, n, k, reorder, reps=None):
        reps = a.reps if reps is None else reps
        nnz = col.numel()
        if reorder:
            os.environ.pop("ISPLIB_REORDER", None)
        else:
            os.environ["ISPLIB_REORDER"] = "0"
        adj = isplib_amd.SparseTensor.from_csr(rowptr, col, None, (n, n), validate=False)
        x = synth.features(n, k, device=dev).to(torch.bfloat16).requires_grad_(True)
        g = synth.features(n, k, seed=5, device=dev).to(torch.bfloat16)
        bias = (torch.arange(k, device=dev, dtype=torch.float32) / k - 0.5).requires_grad_(True)
        ran = {}

        def form(mode):
            def call():
                os.environ["ISPLIB_HALF_GCN"] = mode
                x.grad = bias.grad = None
                out = isplib_amd.gcn_norm_matmul(adj, x, bias, relu=True)
                ran[mode] = adj.storage._last_schedule
                out.backward(g)
                return out
            return call
        forms = (("convert", form("convert")), ("native", form("native")))
        outs, grads, peaks = {}, {}, {}
        for name, fn in forms:
            outs[name] = fn().detach()              # warm-up: builds the transpose and the plans, loads the code objects
            grads[name] = x.grad.detach().clone()
        for name, fn in forms:
            x.grad = bias.grad = None
            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            fn()
            torch.cuda.synchronize()
            peaks[name] = torch.cuda.max_memory_allocated() - base
        head = f"{tag} n={n} nnz={nnz} K={k} reorder={'on' if reorder else 'off'}" + ("" if reps == a.reps else f" ({reps} pairs per run)")
        if ran["native"][0] != "rows16gcn" or ran["convert"][0] != "convert":
            emit(f"{head}: the two forms are not the two routes (convert {ran['convert']}, native {ran['native']}): not measured")
            return
        ordered = len(ran["native"]) > 1
        beyond = n * k * 2 > (256 << 20)
        d_out = (outs["native"].float() - outs["convert"].float()).abs()
        d_grad = (grads["native"].float() - grads["convert"].float()).abs()
        times = {name: [] for name, _ in forms}
        for _ in range(a.runs):
            for name, fn in forms:
                times[name].append(timed(fn, reps))
        pays = max(times["native"]) < min(times["convert"])
        verdict.setdefault((beyond, ordered), []).append(pays)
        emit(f"{head} (class: X {n * k * 2 / 2 ** 20:.0f} MiB {'beyond' if beyond else 'inside'} 256 MiB, {'community order' if ordered else 'index order'})")
        for name in ("convert", "native"):
            emit(f"   {name:8s}" + " ".join(f"{t:8.3f}" for t in times[name]) + f"   min {min(times[name]):.3f} max {max(times[name]):.3f}")
        emit(f"   native vs convert: every native run below every convert run: {'yes' if pays else 'NO'} "
             f"(min/min {min(times['native']) / min(times['convert']):.3f}); out differs in {int((d_out != 0).sum())} of {d_out.numel()} elements "
             f"(max |diff| {float(d_out.max()):.4g}), x.grad in {int((d_grad != 0).sum())} (max |diff| {float(d_grad.max()):.4g})")
        emit(f"   peak device memory of one forward + backward beyond its operands, out and x.grad included: convert {peaks['convert'] / 2 ** 20:.1f} MiB, "
             f"native {peaks['native'] / 2 ** 20:.1f} MiB (X is {n * k * 2 / 2 ** 20:.1f} MiB)")
        del adj, x, g, outs, grads
        torch.cuda.empty_cache()

    if a.part in ("all", "big"):
        for tag, make in (("products-chunglu", lambda s: synth.dataset_like("products", device=dev, scale=s)),
                          ("products-sbm", lambda s: synth.sbm_like("products", device=dev, scale=s))):
            rowptr, col, n = make(a.scale)
            for k in (128, 256):
                for reorder in ((False, True) if tag == "products-sbm" else (True,)):
                    measure(tag, rowptr, col, n, k, reorder)
            del rowptr, col
            torch.cuda.empty_cache()
    if a.part in ("all", "small"):
        rowptr, col, n = synth.dataset_like("products", device=dev, scale=0.25 * a.scale)
        measure("products-chunglu/4", rowptr, col, n, 128, True)
        # the small end of "inside the Infinity Cache": launch-bound calls; 20 x the pairs per run
        for tag, (rowptr, col, n) in (("cora", synth.dataset_like("cora", device=dev)),
                                      ("products-chunglu/50", synth.dataset_like("products", device=dev, scale=0.02 * a.scale))):
            for k in (16, 64):
                measure(tag, rowptr, col, n, k, True, reps=20 * a.reps)
    if a.part in ("all", "reddit"):
        rowptr, col, n = synth.dataset_like("reddit", device=dev, scale=a.scale)
        for k in (32, 48):
            measure("reddit", rowptr, col, n, k, True)
    emit("# verdict per class (X beyond 256 MiB, community order) -> the 16-bit kernel under ISPLIB_HALF_GCN=auto:")
    for cls, pays in sorted(verdict.items()):
        emit(f"   ({'beyond' if cls[0] else 'inside'}, {'ordered' if cls[1] else 'index'}): {'rows16' if all(pays) else 'convert'} ({sum(pays)} of {len(pays)} shapes)")
    emit("   classes not measured here stay on convert")


if __name__ == "__main__":
    main()
