#!/usr/bin/env python3
"""A/B of the value gradient (dA, the SDDMM) of a bf16 sum / mean on the 16-bit SDDMM row kernel (isplib_sddmm_csr_rows16_hip) against
the route it replaces, on scripts/rows16_ab.py's shapes: the ogbn-products-shaped Chung-Lu graph and its SBM twin (bench.py's
config 4), K = 128 and 256, bf16 features, fp32 edge weights that require grad; the SBM twin both in index order (ISPLIB_REORDER=0)
and in its community order; and three shapes inside the Infinity Cache: the products shape at a quarter of its size, K = 128, a
Cora-shaped graph and a fiftieth of the products shape at K = 16 and 64.

What is timed is `out.backward(g)` of `out = matmul(adj, x, reduce)` with ONLY `value` requiring grad, so the backward is dA alone --
the forward runs once per form, before the timing, and its graph is kept.  Three forms, launched alternating, `--runs` runs each (a
run = `--reps` launches between two device events, after a warm-up), for sum and for mean:
  convert   ISPLIB_HALF_DA unset: X.float() and dY.float() -> the fp32 SDDMM (sddmm_csr_kernel), the default route
  native    ISPLIB_HALF_DA=native: the 16-bit SDDMM row kernel on X and dY as they are
  fp32      for context: isplib_sddmm_csr_hip alone on operands widened BEFORE the timing -- what convert costs beyond its two copies
Which route a backward took is read off what it allocates beyond value.grad: the native one never holds as much as an fp32 copy of
X, the default one always does; a shape whose two forms do not show exactly that is reported as not measured (a forward that the
plug-in converts as a whole or runs on a stream plan, or a graph whose dA the handle's whole-row task plan keeps).  The class of a
call is (X beyond
256 MiB at 2 bytes per element or not, rows in a community order or not); ISPLIB_HALF_DA=auto may take the kernel for a class only
where EVERY native run is below EVERY convert run of every measured shape of that class, sum and mean alike
(cabi.sddmm_rows16_native_pays / isplib_sddmm_rows16_native_pays restate the verdict printed here; profiles/sddmm_rows16_ab.txt
records it).  The two routes cut a row's columns into different slots, so their bits may differ in the last place: the count and
the largest difference are printed.

usage: python3 scripts/sddmm_rows16_ab.py [--runs 5] [--reps 10] [--scale 1.0] [--out FILE]"""
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
        sys.exit("sddmm_rows16_ab.py measures on the GPU: none is visible")
    import isplib_amd
    from isplib_amd import cabi, synth
    dev = torch.device("cuda:0")
    lines = [f"# scripts/sddmm_rows16_ab.py: bf16, fp32 weights, backward of sum / mean through matmul with only `value` requiring grad, "
             f"{a.runs} alternating runs x {a.reps} launches, ms per backward",
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
        value = synth.edge_weights(nnz, device=dev).requires_grad_(True)
        adj = isplib_amd.SparseTensor.from_csr(rowptr, col, value, (n, n))
        x16 = synth.features(n, k, device=dev).to(torch.bfloat16)
        g = synth.features(n, k, seed=5, device=dev).to(torch.bfloat16)
        whole = int(cabi.lib().isplib_suggest_slices_whole_rows(n, n, nnz, k))
        for red in ("sum", "mean"):
            ran = {}

            def form(name, mode):
                if mode is None:
                    os.environ.pop("ISPLIB_HALF_DA", None)
                else:
                    os.environ["ISPLIB_HALF_DA"] = mode
                out = isplib_amd.matmul(adj, x16, red)               # the route of the backward is decided here
                ran[name] = adj.storage._last_schedule
                os.environ.pop("ISPLIB_HALF_DA", None)

                def clear():
                    value.grad = None

                def call():
                    clear()
                    out.backward(g, retain_graph=True)
                    return value.grad
                call.clear = clear
                return call

            forms = [("convert", form("convert", None)), ("native", form("native", "native"))]
            grads = {name: fn().detach().clone() for name, fn in forms}     # warm-up: loads the code objects
            peaks = {name: peak_bytes(fn) for name, fn in forms}
            torch.cuda.synchronize()
            fp32_copy = n * k * 4
            head = f"{tag} {red} n={n} nnz={nnz} K={k} reorder={'on' if reorder else 'off'}" + ("" if reps == a.reps else f" ({reps} launches per run)")
            dval = nnz * 4                              # value.grad itself: both routes allocate it
            if not (peaks["native"] - dval < fp32_copy <= peaks["convert"] - dval):
                emit(f"{head}: the two backwards are not the two routes (forward: convert {ran['convert']}, native {ran['native']}; whole-row slices "
                     f"{whole}; peak of the backward: convert {peaks['convert']}, native {peaks['native']} bytes, an fp32 copy of X {fp32_copy}): not measured")
                continue
            x32, g32 = x16.float(), g.float()

            def fp32_alone():
                return cabi.sddmm(rowptr, col, x32, g32, red == "mean")
            fp32_alone.clear = lambda: None
            forms.append(("fp32", fp32_alone))
            fp32_alone()
            ordered = len(ran["native"]) > 1 and ran["native"][1] == "ordered"
            beyond = n * k * 2 > (256 << 20)
            d = (grads["native"] - grads["convert"]).abs()
            unequal, maxdiff = int((d != 0).sum()), float(d.max())
            times = {name: [] for name, _ in forms}
            for _ in range(a.runs):
                for name, fn in forms:
                    times[name].append(timed(fn, reps))
            pays = max(times["native"]) < min(times["convert"])
            verdict.setdefault((beyond, ordered), []).append(pays)
            emit(f"{head} (class: X {n * k * 2 / 2 ** 20:.0f} MiB {'beyond' if beyond else 'inside'} 256 MiB, "
                 f"{'community order' if ordered else 'index order'}; forward on {ran['native']})")
            for name in ("convert", "native", "fp32"):
                emit(f"   {name:8s}" + " ".join(f"{t:8.3f}" for t in times[name]) + f"   min {min(times[name]):.3f} max {max(times[name]):.3f}")
            emit(f"   native vs convert: every native run below every convert run: {'yes' if pays else 'NO'} "
                 f"(min/min {min(times['native']) / min(times['convert']):.3f}); native vs the fp32 kernel alone: min/min "
                 f"{min(times['native']) / min(times['fp32']):.3f}; value.grad differs in {unequal} of {d.numel()} elements (max |diff| {maxdiff:.4g})")
            emit(f"   peak device memory of one backward beyond its operands, value.grad included: convert {peaks['convert'] / 2 ** 20:.1f} MiB, "
                 f"native {peaks['native'] / 2 ** 20:.1f} MiB (X and dY are {n * k * 2 / 2 ** 20:.1f} MiB each, value.grad {nnz * 4 / 2 ** 20:.1f} MiB)")
            del x32, g32, forms, grads
            torch.cuda.empty_cache()
        del adj, value, x16, g
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
    # the small end of "inside the Infinity Cache": launch-bound calls, where the conversion route is three launches and the kernel
    # one; 40 x the launches per run
    for tag, (rowptr, col, n) in (("cora", synth.dataset_like("cora", device=dev)),
                                  ("products-chunglu/50", synth.dataset_like("products", device=dev, scale=0.02 * a.scale))):
        for k in (16, 64):
            measure(tag, rowptr, col, n, k, True, reps=40 * a.reps)
    emit("# verdict per class (X beyond 256 MiB, community order) -> the 16-bit SDDMM row kernel under ISPLIB_HALF_DA=auto:")
    for cls, pays in sorted(verdict.items()):
        emit(f"   ({'beyond' if cls[0] else 'inside'}, {'ordered' if cls[1] else 'index'}): {'rows16' if all(pays) else 'convert'} ({sum(pays)} of {len(pays)} runs of sum / mean on its shapes)")
    emit("   classes not measured here stay on convert")


if __name__ == "__main__":
    main()
