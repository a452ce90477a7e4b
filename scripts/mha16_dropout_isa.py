#!/usr/bin/env python3
"""ISA record of the DROP templates of isplib_amd/csrc/mha16.hip, from the compiler's own listings of two builds.

    hipcc -O3 --offload-arch=gfx950 -std=c++17 -fPIC -save-temps -c isplib_amd/csrc/mha16.hip      (in directory A: the parent commit's
                                                                                                    file; in directory B: this tree's)
    python scripts/mha16_dropout_isa.py A B > profiles/mha16_dropout_isa.txt

Part 1: every kernel <ELT, LPR, WAVES, U, false> of B against the parent's kernel <ELT, LPR, WAVES, U> of A -- every instruction with its
operands, in order (comments, the kernel's own name and the function's index in its labels set aside), and the resource figures that
scripts/rows16_isa_table.py reads (its `kernels`).  Part 2: the resource figures of every kernel <..., true> of B beside its <..., false>
twin; scratch and spills must be 0.  Exit status 1 if a kernel of part 1 differs or a kernel of part 2 uses scratch or spills.
"""
import glob
import re
import sys

from rows16_isa_table import kernels

def bodies(directory):
    """mangled name -> the instructions with operands"""
    out = {}
    for path in sorted(glob.glob(directory + "/*-hip-amdgcn-amd-amdhsa-gfx950.s")):
        name, code = None, False
        for line in open(path):
            m = re.match(r"^(_Z\w+):", line)
            if m:
                name, code = m.group(1), True
                out[name] = []
            elif name is None:
                continue
            elif line.startswith(".Lfunc_end"):
                code = False
            elif code:
                text = line.split(";")[0].strip()
                if text and not text.startswith("."):
                    out[name].append(re.sub(r"\.LBB\d+_", ".LBB_", text.replace(name, "@self")))
    return out


def spills(directory):
    """mangled name -> (sgpr spills, vgpr spills) of the code object's metadata"""
    out = {}
    for path in sorted(glob.glob(directory + "/*-hip-amdgcn-amd-amdhsa-gfx950.s")):
        name = None
        for line in open(path):
            m = re.match(r"^\s+\.(name|sgpr_spill_count|vgpr_spill_count):\s+(\S+)", line)
            if not m:
                continue
            if m.group(1) == "name":
                name = m.group(2)
                out[name] = [None, None]
            elif name in out:
                out[name][m.group(1) == "vgpr_spill_count"] = int(m.group(2))
    return out


def twin_of(table, prefix):
    """the one kernel of `table` whose mangled name starts with `prefix` (the argument type that follows depends on DROP)"""
    found = [n for n in table if n.startswith(prefix)]
    assert len(found) == 1, (prefix, found)
    return found[0]


def main():
    a_dir, b_dir = sys.argv[1], sys.argv[2]
    a, b = kernels(a_dir), kernels(b_dir)
    ab, bb = bodies(a_dir), bodies(b_dir)
    keys = ("vgpr", "sgpr", "scratch", "lds", "occ")
    bad = 0
    print("# The 16-bit multi-head attention kernels (q, k, v) with attention dropout (isplib_amd/csrc/mha16.hip, templates on DROP), from")
    print("# cross-compiled listings: hipcc -O3 --offload-arch=gfx950 -std=c++17 -fPIC -save-temps -c isplib_amd/csrc/mha16.hip (the")
    print("# parent's file and this one; no GPU needed).  scripts/mha16_dropout_isa.py wrote this file.")
    print("# The kernels without dropout take Mha16Args as it was and the kernels with dropout Mha16DropArgs (Mha16Args, then the dropout")
    print("# fields): with the fields written into Mha16Args itself -- a kernel argument of 256 bytes instead of 232 -- 16 of the 30 kernels")
    print("# of part 1 (every rows and columns kernel but LPR = 64) differed from the parent's, in scalar register allocation (columns) or")
    print("# in the sense of one branch (rows); the same 16 differ when the PARENT's file gets 16 unused bytes appended to the struct, and")
    print("# none while the struct stays within 240 bytes.")
    print("#")
    print("# 1. mha16_{fw,bw_rows,bw_cols}_kernel<ELT, LPR, WAVES, U, false> against the parent's kernels without the DROP parameter: every")
    print("#    instruction with its operands, in order; vgpr / sgpr / scratch / lds / occupancy parent/new.  %d kernels" % len(a))
    print("# kernel (parent)  insts parent  insts new  vgpr  sgpr  scratch  lds  occ  verdict")
    for name in sorted(a):
        twin = twin_of(b, name[:-len("EEEvNS_9Mha16ArgsE")] + "ELb0E")
        same = ab[name] == bb[twin] and all(a[name][k] == b[twin][k] for k in keys)
        bad += not same
        print(name, len(ab[name]), len(bb[twin]), "  ".join("%d/%d" % (a[name][k], b[twin][k]) for k in keys),
              "equal instruction for instruction" if same else "DIFFERS", sep="  ")
    print("#")
    print("# 2. the new kernels <..., true> beside their <..., false> twins: vgpr / sgpr / scratch / lds / occupancy / instructions,")
    print("#    without dropout -> with it, then the SGPR and VGPR spill counts of the code object's metadata.  Scratch and both spill")
    print("#    counts must be 0, and no LDS.")
    print("# kernel (DROP = true)  vgpr  sgpr  scratch  lds  occ  insts  sgpr_spills  vgpr_spills  verdict")
    sp = spills(b_dir)
    n_drop = 0
    for name in sorted(b):
        if "ELb1EEEv" not in name:
            continue
        n_drop += 1
        twin = twin_of(b, name[:name.index("ELb1EEEv")] + "ELb0E")
        x, y = b[twin], b[name]
        ok = y["scratch"] == 0 and y["ops"]["scratch_"] == 0 and y["lds"] == 0 and sp[name] == [0, 0]
        bad += not ok
        print(name, "  ".join("%d->%d" % (x[k], y[k]) for k in keys), "%d->%d" % (x["insts"], y["insts"]), sp[name][0], sp[name][1],
              "no scratch, no spills, no LDS" if ok else "SCRATCH, SPILLS OR LDS", sep="  ")
    assert n_drop == len(a), (n_drop, len(a))
    print("# %d of %d kernels miss the bar" % (bad, len(a) + n_drop))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
