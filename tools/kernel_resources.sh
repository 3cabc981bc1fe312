#!/bin/bash
# Per-kernel register / LDS / scratch usage of the library's kernels (hipcc -Rpass-analysis=kernel-resource-usage): every unit that is
# compiled per state layout, in both layouts, and dr_probes.hip.
#   tools/kernel_resources.sh [OUT]     (CPU only: hipcc cross-compiles gfx950)
set -u
root="$(cd "$(dirname "$0")/.." && pwd)"
out="${1:-/dev/stdout}"
cd "$root/dartray_amd/csrc"
F="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -fno-fast-math -Wno-unused-function -x hip -c --cuda-device-only -Rpass-analysis=kernel-resource-usage -o /dev/null"
# Every source that is compiled per state layout in both layouts, and dr_probes.hip, whose walk shares the shading units' hit geometry,
# in the one layout it has.  The lists are read, in one call, from __graft_entry__.py, which only defines names when it is imported.
lists="$(cd "$root" && python3 -c 'import __graft_entry__ as g; print(" ".join(g.SECOND_LAYOUT["sources"])); print(" ".join(g.SECOND_LAYOUT["flags"]))')" || exit 1
two="$(echo "$lists" | sed -n 1p)"
sp4="$(echo "$lists" | sed -n 2p)"
{
for src in $two dr_probes.hip; do
  for lay in "" "$sp4"; do
    [ "$src" = dr_probes.hip ] && [ -n "$lay" ] && continue
    /opt/rocm/bin/hipcc $F $lay $src 2>&1 | python3 -c '
import re, sys
name = None
row = {}
for line in sys.stdin:
    m = re.search(r"Function Name: (\S+)", line)
    if m:
        name = m.group(1); row = {}
        continue
    for key, tag in (("VGPRs:", "vgpr"), ("AGPRs", "agpr"), ("SGPRs:", "sgpr"), ("ScratchSize", "scratch"), ("Occupancy", "occ"), ("LDS Size", "lds")):
        m = re.search(re.escape(key) + r".*?(\d+)", line)
        if m and name:
            row[tag] = int(m.group(1))
            if tag == "lds":
                print("%-90s vgpr %3d sgpr %3d scratch %4d occ %2d lds %6d" % (name, row.get("vgpr", -1), row.get("sgpr", -1), row.get("scratch", -1), row.get("occ", -1), row["lds"]))
                name = None
' | while read -r l; do n=$(echo "$l" | awk '{print $1}' | c++filt | sed 's/(.*//'); echo "$n | $(echo "$l" | cut -d' ' -f2- | sed 's/^ *//')"; done
  done
done
} | sort > "$out"
