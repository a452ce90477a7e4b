#!/usr/bin/env python3
"""A/B of the 16-bit stream kernel (fusedMM_csr_stream16_hip) against the route it replaces, on the Reddit-shaped synthetic graph
of bench.py: K = 64 and 128, unit and U(0,1) weights, bf16 features, forward sum through the plug-in's matmul.

Three forms, launched alternating, `--runs` runs each (a run = `--reps` launches between two device events, after a warm-up):
  convert  x16.float() -> the fp32 op -> .to(bf16): what a user does today (ISPLIB_HALF=convert)
  native   the 16-bit kernel on the same plan (ISPLIB_HALF=native)
  fp32     the fp32 op alone on the widened operand, for context
The class of a call is (slot count of its plan, weighted); the plug-in's `auto` may take the native route for a class only where
EVERY native run is below EVERY convert run of every measured shape of that class (cabi.stream16_native_pays /
isplib_stream16_native_pays restate the verdict printed here; profiles/stream16_ab.txt records it).

usage: python3 scripts/half_ab.py [--runs 5] [--reps 20] [--scale 1.0] [--out FILE]"""
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
    p.add_argument("--reps", type=int, default=20)
    p.add_argument("--scale", type=float, default=1.0, help="shrink the graph (rehearsal only)")
    p.add_argument("--out", default="")
    a = p.parse_args()
    if not torch.cuda.is_available():
        sys.exit("half_ab.py measures on the GPU: none is visible")
    import isplib_amd
    from isplib_amd import synth
    dev = torch.device("cuda:0")
    rowptr, col, n = synth.dataset_like("reddit", device=dev, scale=a.scale)
    nnz = col.numel()
    lines = [f"# scripts/half_ab.py: Reddit-shaped graph n={n} nnz={nnz}, bf16, forward sum, {a.runs} alternating runs x {a.reps} launches, ms per launch",
             f"# device: {torch.cuda.get_device_name(0)}"]
    verdict = {}

    def timed(fn):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(a.reps):
            fn()
        e.record()
        torch.cuda.synchronize()
        return s.elapsed_time(e) / a.reps

    for k in (64, 128):
        for weighted in (False, True):
            w = synth.edge_weights(nnz, device=dev) if weighted else None
            adj = isplib_amd.SparseTensor.from_csr(rowptr, col, w, (n, n))
            x16 = synth.features(n, k, device=dev).to(torch.bfloat16)
            x32 = x16.to(torch.float32)
            ran = {}

            def form(mode, x):
                def call():
                    os.environ["ISPLIB_HALF"] = mode
                    with torch.no_grad():
                        out = isplib_amd.matmul(adj, x, "sum")
                    ran[mode if x is x16 else "fp32"] = adj.storage._last_schedule
                    return out
                return call
            forms = (("convert", form("convert", x16)), ("native", form("native", x16)), ("fp32", form("auto", x32)))
            outs = {name: fn() for name, fn in forms}               # warm-up: builds the plan, loads the code objects
            for _, fn in forms:
                fn()
            torch.cuda.synchronize()
            if ran["native"][0] != "stream16" or ran["convert"][:2] != ("convert", "stream"):
                lines.append(f"K={k} weighted={int(weighted)}: not on the stream schedule (native {ran['native']}, convert {ran['convert']}): not measured")
                continue
            streams = int(ran["native"][1])
            diff = (outs["native"].float() - outs["convert"].float()).abs()
            unequal = int((outs["native"].view(torch.int16) != outs["convert"].view(torch.int16)).sum())
            times = {name: [] for name, _ in forms}
            for _ in range(a.runs):
                for name, fn in forms:
                    times[name].append(timed(fn))
            pays = max(times["native"]) < min(times["convert"])
            verdict.setdefault((streams, weighted), []).append(pays)
            lines.append(f"K={k} weighted={int(weighted)} plan={ran['native'][1:]} (class: {streams} streams, {'weighted' if weighted else 'unit'})")
            for name in ("convert", "native", "fp32"):
                lines.append(f"   {name:8s}" + " ".join(f"{t:8.3f}" for t in times[name]) + f"   min {min(times[name]):.3f} max {max(times[name]):.3f}")
            lines.append(f"   native vs convert: every native run below every convert run: {'yes' if pays else 'NO'};"
                         f" outputs differ in {unequal} of {diff.numel()} elements (max |diff| {float(diff.max()):.4g}; same plan, same order of additions: 0 expected)")
            del adj, x16, x32, outs
            torch.cuda.empty_cache()
    lines.append("# verdict per class (slot count, weighted) -> native under ISPLIB_HALF=auto:")
    for (streams, weighted), pays in sorted(verdict.items()):
        lines.append(f"   ({streams}, {'weighted' if weighted else 'unit'}): {'native' if all(pays) else 'convert'}")
    lines.append("   classes not measured here (8 streams: K <= 32; 2 streams with unit weights: 64 < K < 128) stay on convert")
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
