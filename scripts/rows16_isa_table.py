#!/usr/bin/env python3
"""Per-kernel ISA table of two builds of a set of kernel files, from the compiler's own listings.

    hipcc -O3 --offload-arch=gfx950 -std=c++17 -save-temps -c isplib_amd/csrc/spmm_rows16.hip         (in directory A and in B)
    hipcc -O3 --offload-arch=gfx950 -std=c++17 -save-temps -c isplib_amd/csrc/spmm_rows16_minmax.hip
    python scripts/rows16_isa_table.py A B > profiles/rows16_frontend_isa.txt

It reads every gfx950 listing of a directory: the 16-bit row kernels above (profiles/rows16_frontend_isa.txt), the eight attention
files for attn_common.h / attn16_common.h (profiles/attn_common_isa.txt).  Kernels are matched by mangled name.  The bar (exit status
1 if missed): scratch, LDS, waves per SIMD and the count of every memory, LDS, scalar-load, packed-math, fma and barrier instruction
equal in both builds, and the opcode sequence equal (the mnemonics in order; operands, register numbers, labels and comments are not
compared); registers and total instructions are shown.  The kernel count of every listing follows the table.
"""
import collections
import glob
import os
import re
import sys

GATED = ("buffer_", "global_", "flat_", "scratch_", "ds_", "s_load", "s_buffer_load", "v_pk_", "v_fma", "s_barrier")
META = (("vgpr", "NumVgprs"), ("sgpr", "TotalNumSgprs"), ("scratch", "ScratchSize"), ("lds", "LDSByteSize"), ("occ", "Occupancy"))


def kernels(directory):
    out = {}
    for path in sorted(glob.glob(directory + "/*-hip-amdgcn-amd-amdhsa-gfx950.s")):
        name, body, code = None, None, False
        source = os.path.basename(path).split("-hip-amdgcn")[0]
        for line in open(path):
            m = re.match(r"^(_Z\w+):", line)
            if m:
                name, body, code = m.group(1), {"insts": 0, "ops": collections.Counter(), "seq": [], "file": source}, True
            elif name is None:
                continue
            elif line.startswith(".Lfunc_end"):
                code = False
            elif code:
                m = re.match(r"^\s+([a-z][a-z0-9_]+)", line)
                if m:
                    body["insts"] += 1
                    body["seq"].append(m.group(1))
                    body["ops"].update(g for g in GATED if m.group(1).startswith(g))
            else:                                   # the resource comments that follow a kernel's code
                m = re.match(r"^; (\w+): (\d+)", line)
                for key, word in META:
                    if m and m.group(1) == word:
                        body[key] = int(m.group(2))
                if all(k in body for k, _ in META):
                    out[name], name = body, None
    return out


def main():
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    assert a and set(a) == set(b), (len(a), len(b), sorted(set(a) ^ set(b))[:4])
    print("# parent/new per kernel; gated columns must be equal, the others are shown.  %d kernels" % len(a))
    print("# kernel  vgpr  sgpr  scratch  lds  occ  insts  " + "  ".join(g.rstrip("_") for g in GATED) + "  opcodes  verdict")
    bad = 0
    for name in sorted(a):
        x, y = a[name], b[name]
        same = x["seq"] == y["seq"]
        ok = all(x[k] == y[k] for k in ("scratch", "lds", "occ")) and all(x["ops"][g] == y["ops"][g] for g in GATED) and same
        bad += not ok
        cells = ["%d/%d" % (x[k], y[k]) for k in ("vgpr", "sgpr", "scratch", "lds", "occ", "insts")]
        cells += ["%d/%d" % (x["ops"][g], y["ops"][g]) for g in GATED]
        print(name, "  ".join(cells), "same" if same else "other", "equal" if ok else "DIFFERS", sep="  ")
    for source, count in sorted(collections.Counter(x["file"] for x in a.values()).items()):
        print("# %s: %d kernels" % (source, count))
    print("# %d of %d kernels miss the bar" % (bad, len(a)))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
