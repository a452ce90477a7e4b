"""Experiment behind the levelled deal of the stream plans (profiles/stream_level.txt): where does the spread of the
waves' loop times in a stream dispatch live -- per XCD, per physical CU -- and does it persist from dispatch to dispatch, launch
to launch and process to process?  While isplib_debug_wave_times holds a buffer the dispatches run the TIMED instance of
spmm_stream_kernel: every wave stamps its times and where it ran (XCC id, and CU / SH / SE of HW_ID).

  python3 scripts/exp_stream_level.py measure OUT.pt [launches]    one process: the headline launch (Reddit shape, K=128, unit
        weights, the plan as the process's ISPLIB_STREAM_LEVEL makes it), `launches` timed calls of four dispatches each, then
        the raw calibration (isplib_stream_calibrate_raw: the kernel on a synthetic plan) three times; everything to OUT.pt
  python3 scripts/exp_stream_level.py analyse A.pt B.pt            the figures of profiles/stream_level.txt from two processes

Run the two measuring processes one after the other, each under its own timeout."""
import ctypes
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

CALIB_DEGREE, CALIB_COLS = 512, 2          # the synthetic graph of the shipped calibration (stream_plan.hip)


def measure(out_path, launches):
    from isplib_amd import cabi, synth
    from isplib_amd.plan import build_stream_plan_native
    dev = torch.device("cuda:0")
    k = 128
    rowptr, col, n = synth.dataset_like("reddit", device=dev)
    nnz = col.numel()
    x = synth.features(n, k, device=dev)
    out = torch.empty((n, k), device=dev)
    streams, slices, chunk = cabi.suggest_stream(n, n, nnz, k)
    caps = cabi.stream_capacities(dev, streams, 0, nnz)
    plan = build_stream_plan_native(rowptr, col, n, slices, streams, chunk)
    ws = plan.workspace()
    L = cabi.lib()
    L.isplib_debug_wave_times.argtypes = [ctypes.c_void_p]
    L.isplib_debug_wave_times.restype = None
    for _ in range(3):
        cabi.fusedMM_csr_stream_hip(cabi.MSG_SPMM_SUM, rowptr, nnz, plan, x, out, ws)
    torch.cuda.synchronize()
    nw = plan.waves_per_gen
    stamps = []
    for _ in range(launches):
        buf = torch.zeros(4 * nw * 5, dtype=torch.int64, device=dev)
        L.isplib_debug_wave_times(ctypes.c_void_p(buf.data_ptr()))
        cabi.fusedMM_csr_stream_hip(cabi.MSG_SPMM_SUM, rowptr, nnz, plan, x, out, ws)
        torch.cuda.synchronize()
        L.isplib_debug_wave_times(None)
        stamps.append(buf.view(4, nw, 5).cpu())
    L.isplib_stream_calibrate_raw.restype = ctypes.c_int
    L.isplib_stream_calibrate_raw.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    calib = {}
    for rep in range(3):
        ticks = (ctypes.c_double * nw)()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rc = L.isplib_stream_calibrate_raw(streams, nw, 3, CALIB_DEGREE, CALIB_COLS, ticks, None)
        torch.cuda.synchronize()
        assert rc == 0, cabi.lib().isplib_hip_last_error()
        calib[rep] = (torch.tensor(list(ticks), dtype=torch.float64), (time.perf_counter() - t0) * 1e3)
    steps = (plan.wave_step_off[1:] - plan.wave_step_off[:-1]).cpu().view(-1, nw)
    torch.save({"stamps": torch.stack(stamps), "calib": calib, "steps": steps, "caps": caps, "streams": streams, "nw": nw}, out_path)
    print(f"{out_path}: {launches} launches of 4 dispatches x {nw} waves; plan {'levelled' if caps else 'unlevelled'}", flush=True)


def _factors(dur, key):
    """mean loop time of the waves of every key value, relative to the mean of all waves: {key: factor}"""
    m = dur.mean().item()
    return {int(kv): dur[key == kv].mean().item() / m for kv in torch.unique(key)}


def _apply(dur, key, fac):
    """mean / max of the loop times a dispatch would have had with every wave's work divided by the factor of its key (a wave of
    an unknown key keeps its work): the projection of levelling by that key"""
    f = torch.tensor([fac.get(int(kv), 1.0) for kv in key], dtype=torch.float64)
    t = dur / f
    return (t.mean() / t.max()).item()


def _corr(fa, fb):
    keys = sorted(set(fa) & set(fb))
    if len(keys) < 3:
        return float("nan")
    return torch.corrcoef(torch.tensor([[fa[q] for q in keys], [fb[q] for q in keys]], dtype=torch.float64))[0, 1].item()


def analyse(path_a, path_b):
    procs = [torch.load(p, weights_only=False) for p in (path_a, path_b)]
    nw = procs[0]["nw"]
    label = (torch.arange(nw) // 4) % 8                        # workgroup index modulo 8
    per = []                                                    # per process: [launch][dispatch] -> (dur, xcc, cu key)
    for pi, pr in enumerate(procs):
        st = pr["stamps"].double()
        rows = []
        for l in range(st.shape[0]):
            rows.append([])
            for d in range(4):
                a = st[l, d]
                dur = a[:, 2] - a[:, 1]
                where = pr["stamps"][l, d, :, 4]
                rows[-1].append((dur, where >> 24, where & 0xFF0000FF))      # (XCC; XCC + CU / SH / SE)
        per.append(rows)
        print(f"== process {'AB'[pi]}: plan {'levelled' if pr['caps'] else 'unlevelled'}")
        for l, launch in enumerate(rows):
            for d, (dur, xcc, cu) in enumerate(launch):
                same = all(len(torch.unique(xcc[label == q])) == 1 for q in range(8))
                lab2xcc = [int(xcc[label == q][0]) for q in range(8)]
                fx = _factors(dur, xcc)
                print(f"launch {l} dispatch {d}: mean/max {dur.mean().item() / dur.max().item():.4f}  p50 {dur.median().item():.0f} ticks  "
                      f"workgroup % 8 -> XCC {lab2xcc}{'' if same else ' (NOT one XCC per label)'}  per-XCC factors "
                      + " ".join(f"{fx.get(q, float('nan')):.3f}" for q in range(8))
                      + f"  physical CUs seen {len(torch.unique(cu))}  steps max/mean {(pr['steps'][d % pr['steps'].shape[0]].max() / pr['steps'][d % pr['steps'].shape[0]].double().mean()).item():.4f}")
    # per-CU factors: spread and persistence
    for pi, rows in enumerate(per):
        f00 = _factors(rows[0][0][0], rows[0][0][2])
        v = torch.tensor(list(f00.values()))
        print(f"== process {'AB'[pi]}: per-physical-CU factors of launch 0 dispatch 0: min {v.min():.3f} p10 {v.quantile(0.1):.3f} p90 {v.quantile(0.9):.3f} max {v.max():.3f}")
        print("   correlation of a CU's factor, dispatch 0 against dispatches 1, 2, 3 of the same launch: " +
              " ".join(f"{_corr(f00, _factors(rows[0][d][0], rows[0][d][2])):.2f}" for d in (1, 2, 3)))
        print("   launch 0 against the later launches (same dispatch, mean over the four): " +
              " ".join(f"{sum(_corr(_factors(rows[0][d][0], rows[0][d][2]), _factors(rows[l][d][0], rows[l][d][2])) for d in range(4)) / 4:.2f}" for l in range(1, len(rows))))
        # the same with the XCC's own factor divided out: what the CU adds to its XCD
        def resid(dur, xcc, cu):
            fx = _factors(dur, xcc)
            return _factors(dur / torch.tensor([fx[int(q)] for q in xcc], dtype=torch.float64), cu)
        print("   the same without the XCC's share (CU within its XCD): dispatches " +
              " ".join(f"{_corr(resid(*rows[0][0]), resid(*rows[0][d])):.2f}" for d in (1, 2, 3)) + "  launches " +
              " ".join(f"{sum(_corr(resid(*rows[0][d]), resid(*rows[l][d])) for d in range(4)) / 4:.2f}" for l in range(1, len(rows))))
    a, b = per
    print("== process A against process B (same dispatch of launch 0, mean over the four dispatches)")
    print(f"   correlation of per-XCC factors {sum(_corr(_factors(a[0][d][0], a[0][d][1]), _factors(b[0][d][0], b[0][d][1])) for d in range(4)) / 4:.2f}"
          f"   of per-CU factors {sum(_corr(_factors(a[0][d][0], a[0][d][2]), _factors(b[0][d][0], b[0][d][2])) for d in range(4)) / 4:.2f}")
    # projections: factors from the mean over the launches of one process, applied to every dispatch of another (or the same)
    def mean_factors(rows, which, d):
        acc = {}
        for launch in rows:
            for q, f in _factors(launch[d][0], launch[d][which]).items():
                acc.setdefault(q, []).append(f)
        return {q: sum(v) / len(v) for q, v in acc.items()}
    for name, src, dst in (("within process B (upper bound)", b, b), ("factors of A applied to B", a, b), ("factors of B applied to A", b, a)):
        for which, wname in ((1, "XCD only"), (2, "physical CU")):
            vals = []
            for launch in dst:
                vals.append(sum(_apply(launch[d][0], launch[d][which], mean_factors(src, which, d)) for d in range(4)) / 4)
            base = [sum((launch[d][0].mean() / launch[d][0].max()).item() for d in range(4)) / 4 for launch in dst]
            print(f"   projected mean/max, {name}, {wname}: " + " ".join(f"{v:.4f}" for v in vals) + "  (per launch; measured: " + " ".join(f"{v:.4f}" for v in base) + ")")
    # the calibration (the stream kernel on a synthetic plan) against the headline launch, by workgroup index
    print("== calibration (isplib_stream_calibrate_raw, 3 timed launches) against the headline launch's factors by workgroup index")
    nwg = nw // 4
    grp = (torch.arange(nwg) % 8) * 2 + (torch.arange(nwg) * 2 // nwg)          # XCD x residency order (2 workgroups per CU)
    def wg_factor(t):
        return (t / t.mean()).view(-1, 4).mean(1)
    def grouped(f):
        return torch.stack([f[grp == q].mean() for q in range(16)])[grp]
    for pi, pr in enumerate(procs):
        real = torch.stack([wg_factor(launch[d][0]) for launch in per[pi] for d in range(4)]).mean(0)
        print(f"   process {'AB'[pi]}: headline launch, by group (XCD 0 first / second workgroup of a CU, XCD 1 ...): " + " ".join(f"{v:.3f}" for v in torch.stack([real[grp == q].mean() for q in range(16)])))
        other = per[1 - pi]
        for rep, (ticks, ms) in sorted(pr["calib"].items()):
            fc = wg_factor(ticks)
            g = torch.stack([fc[grp == q].mean() for q in range(16)])
            xs, ys = grouped(fc) - 1, grouped(real) - 1
            slope = (xs * ys).sum().item() / max((xs * xs).sum().item(), 1e-30)
            fw = grouped(fc).repeat_interleave(4)
            proj = [sum(((launch[d][0] / fw).mean() / (launch[d][0] / fw).max()).item() for d in range(4)) / 4 for launch in other]
            print(f"   run {rep}: {ms:.1f} ms  p50 {ticks.median().item():.0f} ticks  by group " + " ".join(f"{v:.3f}" for v in g)
                  + f"  corr with the headline's groups {torch.corrcoef(torch.stack([xs, ys]))[0, 1].item():.3f}  slope {slope:.2f}  per workgroup corr {torch.corrcoef(torch.stack([fc, real]))[0, 1].item():.2f}"
                  + "  projected mean/max of the OTHER process's launches with these capacities: " + " ".join(f"{v:.4f}" for v in proj))
    # projection by workgroup index with the headline's own factors (16 groups, and every workgroup on its own)
    for name, src, dst in (("A applied to B", 0, 1), ("B applied to A", 1, 0), ("B applied to B", 1, 1)):
        real = torch.stack([wg_factor(launch[d][0]) for launch in per[src] for d in range(4)]).mean(0)
        for wname, f in (("16 groups", grouped(real)), ("every workgroup index", real)):
            fw = f.repeat_interleave(4)
            proj = [sum(((launch[d][0] / fw).mean() / (launch[d][0] / fw).max()).item() for d in range(4)) / 4 for launch in per[dst]]
            print(f"   projected mean/max, factors by workgroup index of {name}, {wname}: " + " ".join(f"{v:.4f}" for v in proj))
    # does a workgroup index land on the same CU again?
    ref = procs[0]["stamps"][0, 0, :, 4] & 0xFF0000FF
    same = [((pr["stamps"][l, d, :, 4] & 0xFF0000FF) == ref).double().mean().item() for pr in procs for l in range(pr["stamps"].shape[0]) for d in range(4)]
    print(f"   share of waves on the CU they had in launch 0 dispatch 0 of process A: min {min(same[1:]):.3f} max {max(same[1:]):.3f}")


if __name__ == "__main__":
    if len(sys.argv) >= 3 and sys.argv[1] == "measure":
        measure(sys.argv[2], int(sys.argv[3]) if len(sys.argv) > 3 else 4)
    elif len(sys.argv) == 4 and sys.argv[1] == "analyse":
        analyse(sys.argv[2], sys.argv[3])
    else:
        raise SystemExit(__doc__)
