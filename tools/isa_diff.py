#!/usr/bin/env python3
r"""Per-kernel comparison of two device-only assembly builds of the same source file (parent against branch).

    hipcc <hip.HIPCC_FLAGS minus -shared> -Iinclude --offload-device-only -S -o parent/ccdm_conv.s <parent's ccdm_conv.hip>   (likewise branch/)
    tools/isa_diff.py parent branch ccdm_conv [ccdm_conv_ks ...] [--mask-kernarg KERNEL:FROM:BY] [--rename OLD=NEW ...]

Prints one line per kernel in the format of profiles/r11_conv_refactor_isa.txt: `identical` (same instruction text and the same
five resource numbers) or `parent -> branch` resources.  Instruction text = the lines between a kernel's label and its `.section`,
without comments, blank lines, .loc / .file / .ident / .cfi / .p2align / .Ltmp lines and __hip_cuid_* symbols, with basic-block
labels renumbered by function (.LBB<n>_<m> -> .LBB_<m>: n is the function's position in the file).  --mask-kernarg k_conv:0x128:8
subtracts 8 from every scalar-load / pointer-add offset >= 0x128 in the PARENT's kernels named k_conv<...> (a kernel-argument
struct that lost 8 bytes moves the hidden arguments behind it).  --rename 'k_shaped(\w*)<(.*)>=k_guided\1<\2, false>' pairs a PARENT
kernel with the branch kernel that took its place under another name: OLD is a regular expression on the kernel's name as the lines
below print it, NEW its replacement (re.sub).  Exit status 1 if a kernel set or a kernel differs."""
import argparse
import difflib
import re
import subprocess
import sys

RES = ("vgpr_count", "sgpr_spill_count", "vgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size")
SKIP = (".loc", ".file", ".ident", ".cfi", ".p2align", ".Ltmp")


def parse(path, mask):
    txt = open(path).read()
    names = set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", txt, re.M))
    kernels, cur = {}, None
    for ln in txt.split("\n"):
        m = re.match(r"^(\S+):\s*(;.*)?$", ln)
        if cur is None:
            if m and m.group(1) in names:
                cur = m.group(1)
                kernels[cur] = []
            continue
        if ln.strip().startswith(".section"):
            cur = None
            continue
        s = ln.split(";")[0].rstrip()
        if not s.strip() or s.strip().startswith(SKIP) or "__hip_cuid" in s:
            continue
        if mask and re.search(r"\d%sI" % re.escape(mask[0]), cur):
            mm = re.match(r"^(\s*(?:s_load_\w+\s+.*|s_add_u32 s\d+, s0),\s*)(0x[0-9a-f]+)\s*$", s)
            if mm and int(mm.group(2), 16) >= mask[1]:
                s = mm.group(1) + hex(int(mm.group(2), 16) - mask[2])
        kernels[cur].append(re.sub(r"\.LBB\d+_", ".LBB_", s))
    res = {}
    for blk in txt.split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        res[name] = tuple(int(re.search(r"\." + k + r":\s+(\d+)", blk).group(1)) for k in RES)
    return kernels, res


def waves(vgprs):      # per SIMD: 512 VGPRs per lane, allocation granule 8
    return min(8, 512 // max(8, (vgprs + 7) // 8 * 8))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("parent")
    ap.add_argument("branch")
    ap.add_argument("files", nargs="+", help="source names without .hip; <dir>/<name>.s is read")
    ap.add_argument("--mask-kernarg", default="", metavar="KERNEL:FROM:BY")
    ap.add_argument("--rename", action="append", default=[], metavar="OLD=NEW")
    ap.add_argument("--show", type=int, default=0, help="print this many diff lines of each differing kernel to stderr")
    a = ap.parse_args()
    mask = None
    if a.mask_kernarg:
        k, frm, by = a.mask_kernarg.split(":")
        mask = (k, int(frm, 0), int(by, 0))
    renames = [r.split("=", 1) for r in a.rename]

    def by_name(kernels, res, rename):      # printed name -> (instruction text, resources)
        dem = subprocess.run(["c++filt"], input="\n".join(kernels), capture_output=True, text=True).stdout.split("\n")
        out = {}
        for n, d in zip(kernels, dem):
            name = re.sub(r"^void ccdm::|\(.*\)$", "", d)
            for old, new in rename:
                name = re.sub(old, new, name)
            out[name] = (kernels[n], res[n])
        return out

    bad = 0
    for f in a.files:
        p = by_name(*parse(f"{a.parent}/{f}.s", mask), renames)
        b = by_name(*parse(f"{a.branch}/{f}.s", None), [])
        print(f"## {f}.hip")
        if set(p) != set(b):
            print("kernel sets differ:", " ".join(sorted(set(p) ^ set(b))))
            bad += 1
        both = sorted(set(p) & set(b))
        lines = 0
        for name in both:
            (pk, pr), (bk, br) = p[name], b[name]
            lines += len(pk)
            if pk == bk and pr == br:
                print(f"{name}: identical")
                continue
            bad += 1
            print(f"{name}: {' '.join(map(str, pr))} -> {' '.join(map(str, br))} ({waves(pr[0])} -> {waves(br[0])})")
            if a.show:
                for x in list(difflib.unified_diff(pk, bk, lineterm="", n=0))[:a.show]:
                    print("    " + x, file=sys.stderr)
        print(f"{f}: {len(both)} kernels, {lines} instruction lines compared", file=sys.stderr)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
