#!/usr/bin/env python3
"""Per-instantiation ISA table of sddmm_task_kernel (isplib_amd/csrc/backward.hip) in two builds, from the compiler's own listings:
the parent, whose kernel has no RAGGED template parameter, and this tree, where the launcher picks RAGGED = (k % 4 != 0).

    hipcc -O3 --offload-arch=gfx950 -fPIC -std=c++17 -save-temps -c backward.hip       (the parent's file in directory A, this one in B)
    python scripts/sddmm_tasks_isa_table.py A B > profiles/sddmm_tasks_ragged_isa.txt

Every parent kernel <LPR, NCH, WAVES, ACCUM> is set against the new <.., false> (k % 4 == 0) and <.., true> (ragged k).  The bar
(exit status 1 if missed): the non-ragged form has the parent's instruction stream, mnemonics and operands, line for line (or, failing
that, the parent's VGPR, SGPR, scratch, LDS and occupancy figures, with the difference in instructions listed); the ragged form has
no scratch and at least the parent's occupancy.  scripts/rows16_isa_table.py is the model.
"""
import glob
import re
import sys

META = (("vgpr", "NumVgprs"), ("sgpr", "TotalNumSgprs"), ("scratch", "ScratchSize"), ("lds", "LDSByteSize"), ("occ", "Occupancy"))
NAME = re.compile(r"^_ZN6isplib17sddmm_task_kernelILi(\d+)ELi(\d+)ELi(\d+)ELb([01])E(?:Lb([01])E)?EEvNS_13SddmmTaskArgsE$")


def kernels(directory):
    out = {}
    for path in sorted(glob.glob(directory + "/*-hip-amdgcn-amd-amdhsa-gfx950.s")):
        name, body, code = None, None, False
        for line in open(path):
            m = re.match(r"^(_Z\w+):", line)
            if m and NAME.match(m.group(1)):
                name, body, code = m.group(1), {"stream": []}, True
            elif name is None:
                continue
            elif line.startswith(".Lfunc_end"):
                code = False
            elif code:
                m = re.match(r"^\s+([a-z][a-z0-9_]+.*?)\s*(?:;.*)?$", line)
                if m:
                    body["stream"].append(re.sub(r"\.LBB\d+_", ".LBB_", re.sub(r"\s+", " ", m.group(1))))     # labels carry the function's number
            else:                                   # the resource comments that follow a kernel's code
                m = re.match(r"^; (\w+): (\d+)", line)
                for key, word in META:
                    if m and m.group(1) == word:
                        body[key] = int(m.group(2))
                if all(k in body for k, _ in META):
                    out[NAME.match(name).groups()], name = body, None
    return out


def row(label, x, y, verdict):
    cells = ["%d/%d" % (x[k], y[k]) for k, _ in META] + ["%d/%d" % (len(x["stream"]), len(y["stream"]))]
    print(label, "  ".join(cells), verdict, sep="  ")


def main():
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    assert a and len(b) == 2 * len(a), (len(a), len(b))
    print("# sddmm_task_kernel<LPR, NCH, WAVES, ACCUM>: parent/new per instantiation.  %d parent kernels, %d new" % (len(a), len(b)))
    print("# kernel  vgpr  sgpr  scratch  lds  occ  insts  verdict")
    bad = 0
    for key in sorted(a, key=lambda t: (int(t[1]), int(t[0]), t[3])):
        lpr, nch, waves, accum, _ = key
        x = a[key]
        label = "<%s, %s, %s, %s" % (lpr, nch, waves, "true" if accum == "1" else "false")
        y = b[(lpr, nch, waves, accum, "0")]
        same = x["stream"] == y["stream"]
        figures = all(x[k] == y[k] for k, _ in META)
        bad += not (same or figures)
        row(label + ", RAGGED = false>", x, y, "identical instruction stream" if same else
            ("equal figures, %+d instructions" % (len(y["stream"]) - len(x["stream"])) if figures else "DIFFERS"))
        y = b[(lpr, nch, waves, accum, "1")]
        ok = y["scratch"] == 0 and y["occ"] >= x["occ"]
        bad += not ok
        valu = sum(s.startswith("v_cndmask") or s.startswith("v_and") for s in y["stream"]) - \
            sum(s.startswith("v_cndmask") or s.startswith("v_and") for s in x["stream"])
        row(label + ", RAGGED = true> ", x, y, ("no scratch, occupancy kept, %+d instructions (%+d selects / masks)" %
                                                (len(y["stream"]) - len(x["stream"]), valu)) if ok else "MISSES THE BAR")
    print("# %d of %d comparisons miss the bar" % (bad, 2 * len(a)))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
