#!/bin/bash
# register / spill summary of every instantiation of a kernel TU: tools/regs.sh bfhip_group.hip [extra flags]
# Compiled with the flags csrc/Makefile gives THIS translation unit (make -n prints its compile line: -ffp-contract=off for some, not
# for others), so the table is that of the shipped build.
cd "$(dirname "$0")/../bayesfast_amd/csrc" || exit 1
src=$1; shift
cmd=$(make -s -n -B "_obj/${src%.hip}.o" | grep -- " -c $src ")
[ -n "$cmd" ] || { echo "regs.sh: csrc/Makefile has no compile line for $src" >&2; exit 1; }
tmp=$(mktemp --suffix=.o)
$cmd -Rpass-analysis=kernel-resource-usage "$@" -o "$tmp" 2>&1 | python3 -c "
import sys,re
name=None; info={}
for l in sys.stdin:
    m=re.search(r'Function Name: (\S+)',l)
    if m: name=m.group(1); info[name]=[]
    for k in ('VGPRs:','AGPRs:','ScratchSize \[bytes/lane\]:','SGPRs Spill:','VGPRs Spill:'):
        m=re.search(k+r' (\d+)',l)
        if m and name: info[name].append(int(m.group(1)))
print('kernel : VGPR AGPR scratch sgpr_spill vgpr_spill')
for n,v in info.items(): print(n[:70], v)
"
rm -f "$tmp"
