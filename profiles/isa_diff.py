"""Compare the device assembly of two builds kernel by kernel:  python profiles/isa_diff.py DIR_A DIR_B

Each directory holds one .s file per .hip source, made with the build's own flags:
    hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC --cuda-device-only -S csrc/X.hip -o DIR/X.hip.s
A kernel may live in a different file on the two sides.  Compared per kernel symbol: the instruction text between its entry label and its end
(translation-unit-local label numbers normalised and the assembler's comments dropped: both renumber when functions move between files) and the
resource fields of its metadata.
Exit status 0 when every kernel is identical."""
import glob
import os
import re
import sys

FIELDS = (".vgpr_count", ".agpr_count", ".sgpr_count", ".vgpr_spill_count", ".sgpr_spill_count", ".group_segment_fixed_size",
          ".private_segment_fixed_size", ".max_flat_workgroup_size")
LOCAL = re.compile(r"\.(LBB|Lfunc_end|Lfunc_begin|Ltmp)(\d+)(_\d+)?")


def kernels(d):
    """{symbol: (file, [instruction lines], {field: value})}"""
    out = {}
    for path in sorted(glob.glob(os.path.join(d, "*.s"))):
        lines = open(path).read().split("\n")
        names = [ln.split()[1] for ln in lines if ln.startswith("\t.amdhsa_kernel ") or ln.startswith(".amdhsa_kernel ")]
        for name in names:
            a = next(i for i, ln in enumerate(lines) if ln.startswith(name + ":"))
            b = next(i for i in range(a, len(lines)) if lines[i].startswith(".Lfunc_end"))
            body = [LOCAL.sub(lambda m: "." + m.group(1) + "N" + (m.group(3) or ""), ln.split(";")[0].rstrip()) for ln in lines[a + 1:b]]
            body = [ln for ln in body if ln]          # (the compiler's comments name basic blocks by the same file-local numbers)
            out[name] = [os.path.basename(path), body, {}]
        # metadata: the YAML note at the end of the file, one block per kernel, fields in any order around `.name:`
        meta = "\n".join(lines[lines.index("amdhsa.kernels:"):]) if "amdhsa.kernels:" in lines else ""
        for block in re.split(r"\n  - ", meta)[1:]:
            m = re.search(r"^\s*\.name:\s+(\S+)", block, re.M)
            if m and m.group(1) in out:
                for f in FIELDS:
                    v = re.search(r"^\s*%s:\s+(\S+)" % re.escape(f), block, re.M)
                    out[m.group(1)][2][f] = v.group(1) if v else None
    return out


def main():
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    bad = sorted(set(a) ^ set(b))
    for k in bad: print("only in %s: %s" % (sys.argv[1] if k in a else sys.argv[2], k))
    same = 0
    for k in sorted(set(a) & set(b)):
        if a[k][1] == b[k][1] and a[k][2] == b[k][2] and None not in a[k][2].values() and len(a[k][2]) == len(FIELDS): same += 1; continue
        bad.append(k)
        what = "instructions" if a[k][1] != b[k][1] else "metadata %s vs %s" % (a[k][2], b[k][2])
        print("DIFFERENT %s (%s / %s): %s" % (k, a[k][0], b[k][0], what))
    print("%d of %d kernels identical" % (same, len(set(a) | set(b))))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
