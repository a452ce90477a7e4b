#!/usr/bin/env python3
"""A/B of the 16-bit multi-head attention operator WITH attention dropout (torch.ops.isplib.mha_drop_spmm16: isplib_qkv_half_drop_csr_hip
and its two backward kernels) against the conversion route (`q.float()`, `k.float()`, `v.float()` -> the fp32 dropout operator ->
`.to(dtype)`, with autograd through the casts), in bf16 at p = 0.6, on the shapes of scripts/mha16_ab.py: the Reddit-shaped synthetic
graph at (H, d) = (8, 8) and (8, 16) and the ogbn-products shape at (8, 16), scale 1 / sqrt(d), forward alone and forward + backward
(gradients of q, k and v).  q, k, v and the gradient are bf16, as a layer under autocast produces them.

Both routes go through isplib_amd.mha_matmul(..., dropout=0.6, seed=...) with ISPLIB_HALF_MHA=native, switched by
ISPLIB_HALF_MHA_DROP=native|convert, and are launched alternating, `--runs` runs each; a run is `--reps` steps between two device
events after a warm-up of all forms.  A third form runs in the same alternation: the 16-bit call WITHOUT dropout (dropout=0, the
kernels of scripts/mha16_ab.py's native side), for the unthresholded second figure -- the time of the 16-bit dropout call relative to
it, which says how much of the hash the 16-bit step hides (the fp32 kernels hid it at 1.00-1.02: profiles/mha_dropout_ab.txt).  Peak
device memory of one step beyond what is allocated before it is reported for every form.  The outputs of the two dropout routes are
compared once per shape (one mask, two computations rounded to bf16: the largest |difference| is printed).

The verdict per class of the family (the gathered operand beyond 256 MiB at 2 bytes per element or not) is printed last: a class pays
only if EVERY native run lies below EVERY run of the conversion route, forward + backward, on every shape of the class measured here.
isplib_qkv_half_drop_native_pays (include/isplib_hip_mha16_drop.h) and cabi.mha16_drop_native_pays restate it;
profiles/mha16_dropout_ab.txt is the record.

usage: python3 scripts/mha16_dropout_ab.py [--runs 5] [--reps 5] [--scale 1.0] [--out FILE]"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

P = 0.6
SEED = 0x1E3779B97F4A7C15


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--runs", type=int, default=5)
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--scale", type=float, default=1.0, help="shrink the graphs (rehearsal only)")
    p.add_argument("--out", default="")
    a = p.parse_args()
    if not torch.cuda.is_available():
        sys.exit("mha16_dropout_ab.py measures on the GPU: none is visible")
    import isplib_amd
    from isplib_amd import synth
    from isplib_amd.plugin import mha16_drop_route
    dev = torch.device("cuda:0")
    dtype = torch.bfloat16
    lines = [f"# scripts/mha16_dropout_ab.py: bf16 (q, k, v and the gradient), dropout p = {P}, scale 1/sqrt(d), {a.runs} alternating runs x "
             f"{a.reps} steps, ms per step",
             "# convert: ISPLIB_HALF_MHA_DROP=convert (the parent's behaviour); native: =native; nodrop16: the 16-bit call with dropout=0",
             f"# device: {torch.cuda.get_device_name(0)}"]
    verdict = {}                                    # class -> every native run below every convert run, forward + backward

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
        q = synth.features(n, k, seed=2, device=dev).to(dtype).requires_grad_(True)
        key = synth.features(n, k, seed=3, device=dev).to(dtype).requires_grad_(True)
        v = synth.features(n, k, seed=4, device=dev).to(dtype).requires_grad_(True)
        g = synth.features(n, k, seed=5, device=dev).to(dtype)
        adj = isplib_amd.SparseTensor.from_csr(rowptr, col, None, (n, n), validate=False)
        os.environ["ISPLIB_HALF_MHA"] = "native"
        assert mha16_drop_route(dtype, heads, d, k, n, "native") == "mha16drop"
        beyond = n * k * 2 > (256 << 20)
        cls = "beyond 256 MiB" if beyond else "inside 256 MiB"

        def step(mode, grad):
            def run():
                os.environ["ISPLIB_HALF_MHA_DROP"] = "convert" if mode == "nodrop16" else mode
                q.grad = key.grad = v.grad = None
                drop = 0.0 if mode == "nodrop16" else P
                if not grad:
                    with torch.no_grad():
                        return isplib_amd.mha_matmul(adj, q, key, v, heads=heads, dropout=drop, seed=SEED)
                out = isplib_amd.mha_matmul(adj, q, key, v, heads=heads, dropout=drop, seed=SEED)
                out.backward(g)
                return out
            return run

        emit(f"{tag} n={n} nnz={nnz} H={heads} d={d} (gathered operand {n * k * 2 / 2 ** 20:.1f} MiB: {cls})")
        for what, grad in (("forward", False), ("forward+backward", True)):
            forms = [(name, step(name, grad)) for name in ("convert", "native", "nodrop16")]
            outs = {}
            for name, fn in forms:                  # warm-up: loads the code objects, builds the transposed structure
                outs[name] = fn().detach().float()
                outs[name + "_g"] = (q.grad.float(), key.grad.float(), v.grad.float()) if grad else ()
            peaks = {name: peak_bytes(fn) for name, fn in forms}
            times = {name: [] for name, _ in forms}
            for _ in range(a.runs):
                for name, fn in forms:
                    times[name].append(timed(fn, a.reps))
            diff = float((outs["native"] - outs["convert"]).abs().max())
            gdiff = max((float((s - t).abs().max()) for s, t in zip(outs["native_g"], outs["convert_g"])), default=0.0)
            for name, _ in forms:
                emit(f"   {what:17s}{name:9s}" + " ".join(f"{t:8.3f}" for t in times[name]) +
                     f"   min {min(times[name]):.3f} max {max(times[name]):.3f}   peak beyond operands {peaks[name] / 2 ** 20:.1f} MiB")
            wins = max(times["native"]) < min(times["convert"])
            emit(f"   {what}: native / convert min/min {min(times['native']) / min(times['convert']):.3f}; every native run below every "
                 f"convert run: {'yes' if wins else 'NO'}; max |z difference| {diff:.3g}" + (f", max |gradient difference| {gdiff:.3g}" if grad else "") +
                 f" ([n, K] fp32 = {n * k * 4 / 2 ** 20:.1f} MiB)")
            emit(f"   {what}: native with dropout / 16-bit call without dropout min/min {min(times['native']) / min(times['nodrop16']):.3f} "
                 f"(max/min {max(times['native']) / min(times['nodrop16']):.3f}, min/max {min(times['native']) / max(times['nodrop16']):.3f})")
            if grad:
                verdict[cls] = verdict.get(cls, True) and wins
            del outs, forms
            torch.cuda.empty_cache()
        del adj, q, key, v, g
        torch.cuda.empty_cache()

    rowptr, col, n = synth.dataset_like("reddit", device=dev, scale=a.scale)
    for heads, d in ((8, 8), (8, 16)):
        measure("reddit", rowptr, col, n, heads, d)
    del rowptr, col
    torch.cuda.empty_cache()
    rowptr, col, n = synth.dataset_like("products", device=dev, scale=a.scale)
    measure("products", rowptr, col, n, 8, 16)
    for cls in ("inside 256 MiB", "beyond 256 MiB"):
        if cls in verdict:
            emit(f"# verdict, gathered operand {cls}: native {'PAYS' if verdict[cls] else 'does NOT pay'} (forward + backward, every shape above)")
        else:
            emit(f"# verdict, gathered operand {cls}: not measured")
    os.environ.pop("ISPLIB_HALF_MHA", None)
    os.environ.pop("ISPLIB_HALF_MHA_DROP", None)


if __name__ == "__main__":
    main()
