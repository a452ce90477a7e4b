#!/usr/bin/env python3
"""A/B of the unit-weight mean backward on the column-scaled 16-bit row kernel (fusedMM_csr_rows16_colscale_hip) against the route it
replaces, on scripts/rows16_ab.py's shapes: the ogbn-products-shaped Chung-Lu graph and its SBM twin (bench.py's config 4), K = 128
and 256, bf16 features, NO edge weights; the SBM twin both in index order (ISPLIB_REORDER=0) and in its community order; and three
shapes inside the Infinity Cache: the products shape at a quarter of its size, K = 128, a Cora-shaped graph and a fiftieth of the
products shape at K = 16 and 64.

What is timed is `out.backward(g)` of `out = matmul(adj, x, "mean")` alone -- the forward runs once per form, before the timing, and
its graph is kept.  Three forms, launched alternating, `--runs` runs each (a run = `--reps` backwards between two device events,
after a warm-up):
  convert   ISPLIB_HALF_MEAN_BW unset: dY.float() / deg -> the fp32 plain kernel on A^T -> .to(bf16), the default route
  native    ISPLIB_HALF_MEAN_BW=native: the column-scaled 16-bit row kernel on dY as it is, 1 / deg from an M-entry table
  edge      for context: the same graph given explicit all-ones weights, whose mean backward is the WEIGHTED 16-bit row kernel with
            1 / deg per edge -- the same arithmetic (x.grad must have native's bits) behind an nnz-long fp32 weight stream
Which route a backward took is read off what it allocates: the native one never holds as much as an fp32 copy of dY, the default one
always does; a shape whose two forms do not show exactly that is reported as not measured (e.g. a forward that the plug-in converts as
a whole, or a backward on a stream plan).  The class of a call is (dY beyond 256 MiB at 2 bytes per element or not, rows of A^T in a
community order or not); ISPLIB_HALF_MEAN_BW=auto may take the kernel for a class only where EVERY native run is below EVERY convert
run of every measured shape of that class (cabi.rows16_colscale_native_pays / isplib_rows16_colscale_native_pays restate the verdict
printed here; profiles/rows16_colscale_ab.txt records it).  The two routes round differently before the last rounding (dY / deg
rounded to fp32 and then summed, against one fused multiply-add per term), so their bits may differ in the last place: the count
and the largest difference are printed.

usage: python3 scripts/rows16_colscale_ab.py [--runs 5] [--reps 10] [--scale 1.0] [--out FILE]"""
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
        sys.exit("rows16_colscale_ab.py measures on the GPU: none is visible")
    import isplib_amd
    from isplib_amd import synth
    dev = torch.device("cuda:0")
    lines = [f"# scripts/rows16_colscale_ab.py: bf16, unweighted, backward of mean through matmul, {a.runs} alternating runs x {a.reps} launches, ms per backward",
             f"# device: {torch.cuda.get_device_name(0)}"]
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

    def peak_bytes(fn):
        fn.clear()                                  # the gradient of the call before is not this call's
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        fn()
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - base

    def measure(tag, rowptr, col, n, k, reorder, reps=None):
        reps = a.reps if reps is None else reps
        nnz = col.numel()
        if reorder:
            os.environ.pop("ISPLIB_REORDER", None)
        else:
            os.environ["ISPLIB_REORDER"] = "0"
        adj = isplib_amd.SparseTensor.from_csr(rowptr, col, None, (n, n))
        adj_ones = isplib_amd.SparseTensor.from_csr(rowptr, col, torch.ones(nnz, dtype=torch.float32, device=dev), (n, n))
        x16 = synth.features(n, k, device=dev).to(torch.bfloat16)
        g = synth.features(n, k, seed=5, device=dev).to(torch.bfloat16)
        ran = {}

        def form(name, mode, adj=adj):
            if mode is None:
                os.environ.pop("ISPLIB_HALF_MEAN_BW", None)
            else:
                os.environ["ISPLIB_HALF_MEAN_BW"] = mode
            x = x16.clone().requires_grad_(True)
            out = isplib_amd.matmul(adj, x, "mean")             # the route of the backward is decided here
            ran[name] = adj.storage._last_schedule
            os.environ.pop("ISPLIB_HALF_MEAN_BW", None)

            def clear():
                x.grad = None

            def call():
                clear()
                out.backward(g, retain_graph=True)
                return x.grad
            call.clear = clear
            return call
        forms = (("convert", form("convert", None)), ("native", form("native", "native")), ("edge", form("edge", None, adj_ones)))
        grads = {name: fn().detach().clone() for name, fn in forms}     # warm-up: loads the code objects
        peaks = {name: peak_bytes(fn) for name, fn in forms}
        torch.cuda.synchronize()
        fp32_copy = n * k * 4
        head = f"{tag} n={n} nnz={nnz} K={k} reorder={'on' if reorder else 'off'}" + ("" if reps == a.reps else f" ({reps} launches per run)")
        if not (peaks["native"] < fp32_copy <= peaks["convert"]):
            emit(f"{head}: the two backwards are not the two routes (forward: convert {ran['convert']}, native {ran['native']}; peak of the backward: "
                 f"convert {peaks['convert']}, native {peaks['native']} bytes, an fp32 copy of dY {fp32_copy}): not measured")
            return
        ordered = bool(adj.storage.row_order(True, k, itemsize=2))
        ordered32 = bool(adj.storage.row_order(True, k))
        beyond = n * k * 2 > (256 << 20)
        d = (grads["native"].float() - grads["convert"].float()).abs()
        unequal, maxdiff = int((d != 0).sum()), float(d.max())
        edge_ok = peaks["edge"] < fp32_copy                     # the weighted 16-bit kernel too (else: context only, whatever it ran on)
        edge_unequal = int((grads["native"].view(torch.int16) != grads["edge"].view(torch.int16)).sum())
        times = {name: [] for name, _ in forms}
        for _ in range(a.runs):
            for name, fn in forms:
                times[name].append(timed(fn, reps))
        pays = max(times["native"]) < min(times["convert"])
        verdict.setdefault((beyond, ordered), []).append(pays)
        emit(f"{head} (class: dY {n * k * 2 / 2 ** 20:.0f} MiB {'beyond' if beyond else 'inside'} 256 MiB, "
             f"{'community order' if ordered else 'index order'}{'' if ordered == ordered32 else ' (fp32 route: ' + ('community' if ordered32 else 'index') + ' order)'}; "
             f"forward on {ran['native']})")
        for name in ("convert", "native", "edge"):
            emit(f"   {name:8s}" + " ".join(f"{t:8.3f}" for t in times[name]) + f"   min {min(times[name]):.3f} max {max(times[name]):.3f}")
        emit(f"   native vs convert: every native run below every convert run: {'yes' if pays else 'NO'} "
             f"(min/min {min(times['native']) / min(times['convert']):.3f}); x.grad differs in {unequal} of {d.numel()} elements (max |diff| {maxdiff:.4g})")
        emit(f"   edge (per-edge 1 / deg, {nnz * 4 / 2 ** 20:.0f} MiB of weights{'' if edge_ok else '; NOT on the 16-bit kernel'}) vs native ({n * 4 / 2 ** 20:.1f} MiB table): "
             f"min/min {min(times['edge']) / min(times['native']):.3f}; x.grad differs from native's in {edge_unequal} elements")
        emit(f"   peak device memory of one backward beyond its operands, x.grad included: convert {peaks['convert'] / 2 ** 20:.1f} MiB, "
             f"native {peaks['native'] / 2 ** 20:.1f} MiB (dY and x.grad are {n * k * 2 / 2 ** 20:.1f} MiB each)")
        del adj, adj_ones, x16, g, grads, forms
        torch.cuda.empty_cache()

    for tag, make in (("products-chunglu", lambda s: synth.dataset_like("products", device=dev, scale=s)),
                      ("products-sbm", lambda s: synth.sbm_like("products", device=dev, scale=s))):
        rowptr, col, n = make(a.scale)
        for k in (128, 256):
            for reorder in ((False, True) if tag == "products-sbm" else (True,)):
                measure(tag, rowptr, col, n, k, reorder)
        del rowptr, col
        torch.cuda.empty_cache()
    rowptr, col, n = synth.dataset_like("products", device=dev, scale=0.25 * a.scale)
    measure("products-chunglu/4", rowptr, col, n, 128, True)
    # the small end of "inside the Infinity Cache": launch-bound calls, where the conversion route is four launches and the kernel one;
    # 40 x the launches per run
    for tag, (rowptr, col, n) in (("cora", synth.dataset_like("cora", device=dev)),
                                  ("products-chunglu/50", synth.dataset_like("products", device=dev, scale=0.02 * a.scale))):
        for k in (16, 64):
            measure(tag, rowptr, col, n, k, True, reps=40 * a.reps)
    emit("# verdict per class (dY beyond 256 MiB, community order) -> the column-scaled kernel under ISPLIB_HALF_MEAN_BW=auto:")
    for cls, pays in sorted(verdict.items()):
        emit(f"   ({'beyond' if cls[0] else 'inside'}, {'ordered' if cls[1] else 'index'}): {'rows16' if all(pays) else 'convert'} ({sum(pays)} of {len(pays)} shapes)")
    emit("   classes not measured here stay on convert")


if __name__ == "__main__":
    main()
