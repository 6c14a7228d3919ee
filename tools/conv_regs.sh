#!/bin/bash
# Register / spill report of every kernel of one source file (device-only compile with the product's flags)
#   tools/conv_regs.sh [file.hip]      default: ccdm_conv.hip; a bare name is looked up in csrc/, a path is taken as given (from the repository root)
set -e
cd "$(dirname "$0")/.."
SRC=${1:-ccdm_conv.hip}
case "$SRC" in */*) ;; *) SRC=ccdm_stochastic_segmentation_amd/csrc/$SRC ;; esac      # a bare name: the product's source directory
OUT=$(mktemp -d)
trap 'rm -rf "$OUT"' EXIT
FLAGS=$(python -c "from ccdm_stochastic_segmentation_amd import hip; print(' '.join(f for f in hip.HIPCC_FLAGS if f != '-shared'))")
hipcc $FLAGS -Iinclude --offload-device-only -S -o "$OUT/k.s" "$SRC" > "$OUT/k.log" 2>&1 || { cat "$OUT/k.log"; exit 1; }
grep -c "warning\|error" "$OUT/k.log" || true
python - "$OUT/k.s" <<'PY'
import re, subprocess, sys
txt = open(sys.argv[1]).read()
print("kernel: vgpr_count sgpr_spill_count vgpr_spill_count private_segment_fixed_size group_segment_fixed_size")
rows = []
for blk in txt.split("  - .agpr_count:")[1:]:
    name = re.search(r'\.name:\s+(\S+)', blk).group(1)
    g = lambda k: re.search(r'\.' + k + r':\s+(\d+)', blk).group(1)
    rows.append((name, " ".join(g(k) for k in ("vgpr_count", "sgpr_spill_count", "vgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size"))))
names = subprocess.run(["c++filt"], input="\n".join(n for n, _ in rows), capture_output=True, text=True).stdout.split("\n")
for (_, r), n in sorted(zip(rows, names), key=lambda x: x[1]):
    print(re.sub(r"^void ccdm::|\(.*\)$", "", n) + ": " + r)
PY
