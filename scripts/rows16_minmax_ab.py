#!/usr/bin/env python3
"""A/B of the 16-bit max / min row kernel (fusedMM_csr_rows16_minmax_hip) against the route it replaces, on scripts/rows16_ab.py's
shapes and classes: the ogbn-products-shaped Chung-Lu graph and its SBM twin (bench.py's config 4), K = 128 and 256, unit and U(0,1)
weights, bf16 features, forward max through the plug-in's matmul; the SBM twin both in index order (ISPLIB_REORDER=0) and in its
community order; and three shapes inside the Infinity Cache: the products shape at a quarter of its size, K = 128, a Cora-shaped graph
and a fiftieth of the products shape at K = 16 and 64.  Every shape is measured values-only (a no-grad call: the *_values operators)
and with positions (x requires grad: the *_planned operators, forward only).

Three forms, launched alternating, `--runs` runs each (a run = `--reps` launches between two device events, after a warm-up):
  convert   x16.float() -> the fp32 plain kernel -> .to(bf16): the default route (ISPLIB_HALF_MINMAX=convert)
  rows16mm  the 16-bit max / min row kernel (ISPLIB_HALF_MINMAX=native)
  fp32      the fp32 plain kernel alone on the widened operand, for context
The class of a call is (operand beyond 256 MiB at 2 bytes per element or not, rows in a community order or not, weighted or not,
positions wanted or not); ISPLIB_HALF_MINMAX=auto may take the kernel for a class only where EVERY rows16mm run is below EVERY convert
run of every measured shape of that class (cabi.rows16_minmax_native_pays / isplib_rows16_minmax_native_pays restate the verdict
printed here; profiles/rows16_minmax_ab.txt records it).  The two routes must agree bit for bit; the count of differing elements is
printed.  Peak device memory of the two routes (torch.cuda.max_memory_allocated over one call) is printed at K = 256.

usage: python3 scripts/rows16_minmax_ab.py [--runs 5] [--reps 10] [--scale 1.0] [--out FILE]"""
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
    p.add_argument("--reps", type=int, default=10)
    p.add_argument("--scale", type=float, default=1.0, help="shrink the graphs (rehearsal only)")
    p.add_argument("--out", default="")
    a = p.parse_args()
    if not torch.cuda.is_available():
        sys.exit("rows16_minmax_ab.py measures on the GPU: none is visible")
    import isplib_amd
    from isplib_amd import synth
    dev = torch.device("cuda:0")
    lines = [f"# scripts/rows16_minmax_ab.py: bf16, forward max through matmul, {a.runs} alternating runs x {a.reps} launches, ms per launch",
             f"# device: {torch.cuda.get_device_name(0)}"]
    verdict = {}

    def emit(line):
        lines.append(line)
        print(line, flush=True)

    def timed(fn, reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(reps):
            fn()
        e.record()
        torch.cuda.synchronize()
        return s.elapsed_time(e) / reps

    def peak_mb(fn):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        out = fn()
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - base
        del out
        return peak / 2 ** 20

    def measure(tag, rowptr, col, n, k, weighted, reorder, want_arg, reps=None):
        reps = a.reps if reps is None else reps
        nnz = col.numel()
        if reorder:
            os.environ.pop("ISPLIB_REORDER", None)
        else:
            os.environ["ISPLIB_REORDER"] = "0"
        w = synth.edge_weights(nnz, device=dev) if weighted else None
        adj = isplib_amd.SparseTensor.from_csr(rowptr, col, w, (n, n))
        x16 = synth.features(n, k, device=dev).to(torch.bfloat16)
        x32 = x16.to(torch.float32)
        ran = {}

        def form(name, mode, x):
            xg = x.clone().requires_grad_(True) if want_arg else x

            def call():
                os.environ["ISPLIB_HALF_MINMAX"] = mode
                with torch.set_grad_enabled(want_arg):
                    out = isplib_amd.matmul(adj, xg, "max")
                ran[name] = adj.storage._last_schedule
                return out.detach()
            return call
        forms = (("convert", form("convert", "convert", x16)), ("rows16mm", form("rows16mm", "native", x16)), ("fp32", form("fp32", "convert", x32)))
        outs = {name: fn() for name, fn in forms}               # warm-up: finds the row order, loads the code objects
        for _, fn in forms:
            fn()
        torch.cuda.synchronize()
        head = f"{tag} n={n} nnz={nnz} K={k} weighted={int(weighted)} reorder={'on' if reorder else 'off'} positions={int(want_arg)}" + ("" if reps == a.reps else f" ({reps} launches per run)")
        if ran["rows16mm"][0] != "rows16mm" or ran["convert"] != ("convert", "plain") or ran["fp32"] != ("plain",):
            emit(f"{head}: not on the plain kernel (rows16mm {ran['rows16mm']}, convert {ran['convert']}, fp32 {ran['fp32']}): not measured")
            return
        ordered = ran["rows16mm"][1:] == ("ordered",)
        ordered32 = bool(adj.storage.row_order(False, k))
        beyond = n * k * 2 > (256 << 20)
        unequal = int((outs["rows16mm"].view(torch.int16) != outs["convert"].view(torch.int16)).sum())
        times = {name: [] for name, _ in forms}
        for _ in range(a.runs):
            for name, fn in forms:
                times[name].append(timed(fn, reps))
        pays = max(times["rows16mm"]) < min(times["convert"])
        cls = (beyond, ordered, weighted, want_arg)
        verdict.setdefault(cls, []).append(pays)
        emit(f"{head} (class: operand {n * k * 2 / 2 ** 20:.0f} MiB {'beyond' if beyond else 'inside'} 256 MiB, "
             f"{'community order' if ordered else 'index order'}{'' if ordered == ordered32 else ' (fp32 route: ' + ('community' if ordered32 else 'index') + ' order)'}, "
             f"{'weighted' if weighted else 'unit'}, {'positions' if want_arg else 'values only'})")
        for name in ("convert", "rows16mm", "fp32"):
            emit(f"   {name:8s}" + " ".join(f"{t:8.3f}" for t in times[name]) + f"   min {min(times[name]):.3f} max {max(times[name]):.3f}")
        emit(f"   rows16mm vs convert: every rows16mm run below every convert run: {'yes' if pays else 'NO'} "
             f"(min/min {min(times['rows16mm']) / min(times['convert']):.3f}); outputs differ in {unequal} of {outs['convert'].numel()} elements "
             f"(the contract is bit equality)")
        if k == 256:
            emit(f"   peak device memory of one call beyond its operands: convert {peak_mb(forms[0][1]):.0f} MiB, rows16mm {peak_mb(forms[1][1]):.0f} MiB")
        del adj, x16, x32, outs
        torch.cuda.empty_cache()

    for tag, make in (("products-chunglu", lambda s: synth.dataset_like("products", device=dev, scale=s)),
                      ("products-sbm", lambda s: synth.sbm_like("products", device=dev, scale=s))):
        rowptr, col, n = make(a.scale)
        for k in (128, 256):
            for weighted in (False, True):
                for reorder in ((False, True) if tag == "products-sbm" else (True,)):
                    for want_arg in (False, True):
                        measure(tag, rowptr, col, n, k, weighted, reorder, want_arg)
        del rowptr, col
        torch.cuda.empty_cache()
    rowptr, col, n = synth.dataset_like("products", device=dev, scale=0.25 * a.scale)
    for weighted in (False, True):
        for want_arg in (False, True):
            measure("products-chunglu/4", rowptr, col, n, 128, weighted, True, want_arg)
    # the small end of "inside the Infinity Cache": a Cora-shaped graph (4 edges per row) and a fiftieth of the products shape --
    # launch-bound calls, where the conversion route is three launches and the kernel one; 40 x the launches per run
    for tag, (rowptr, col, n) in (("cora", synth.dataset_like("cora", device=dev)),
                                  ("products-chunglu/50", synth.dataset_like("products", device=dev, scale=0.02 * a.scale))):
        for k in (16, 64):
            for weighted in (False, True):
                for want_arg in (False, True):
                    measure(tag, rowptr, col, n, k, weighted, True, want_arg, reps=40 * a.reps)
    emit("# verdict per class (operand beyond 256 MiB, community order, weighted, positions) -> rows16mm under ISPLIB_HALF_MINMAX=auto:")
    for cls, pays in sorted(verdict.items()):
        emit(f"   ({'beyond' if cls[0] else 'inside'}, {'ordered' if cls[1] else 'index'}, {'weighted' if cls[2] else 'unit'}, {'positions' if cls[3] else 'values only'}): "
             f"{'rows16mm' if all(pays) else 'convert'} ({sum(pays)} of {len(pays)} shapes)")
    emit("   classes not measured here stay on convert")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
