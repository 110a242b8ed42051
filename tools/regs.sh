#!/bin/bash
# resource summary of one HIP source (compile-only): tools/regs.sh <file.hip> [extra flags]
#   tools/regs.sh --all   every .hip of csrc with the Makefile's flags (the per-file -ffp-contract=off included)
# per kernel: VGPRs, AGPRs, SGPRs, spilled VGPRs / SGPRs, scratch bytes per lane, waves per SIMD, LDS bytes
self=$(readlink -f $0)
cd $(dirname $self)/../rl-k8s-scheduler_amd/csrc
if [ "$1" = "--all" ]; then
  for f in *.hip; do
    echo "== $f"
    case $f in env.hip|rules.hip|action_mask.hip|rollout_metrics.hip|obs_filter.hip) x=-ffp-contract=off;; *) x=;; esac
    if [ $f = calib.hip ]; then $self $f; else $self $f -fno-slp-vectorize $x; fi
  done
  exit 0
fi
f=$1; shift
/opt/rocm/bin/hipcc -std=c++17 -O3 -fPIC --offload-arch=gfx950 -I../../include -Wall -Wno-unused-function -munsafe-fp-atomics "$@" -c $f -o /tmp/regs_$$.o -Rpass-analysis=kernel-resource-usage 2>&1 | python3 -c "
import sys,re
keys=[('VGPRs','vgpr'),('AGPRs','agpr'),('TotalSGPRs','sgpr'),('VGPRs Spill','spill'),('SGPRs Spill','sspill'),
      ('ScratchSize \[bytes/lane\]','scratch'),('Occupancy \[waves/SIMD\]','occ'),('LDS Size \[bytes/block\]','lds')]
name=None; d={}
for l in sys.stdin:
    m=re.search(r'Function Name: (\S+)',l)
    if m: name=m.group(1); d={}
    for k,s in keys:
        m=re.search(r' '+k+r': (\d+)',l)
        if m: d[s]=m.group(1)
    if 'LDS Size' in l and name:
        print(name+' '+' '.join(f'{s}={d.get(s,\"?\")}' for _,s in keys)); name=None
    if 'error' in l: print(l.strip())
"
rm -f /tmp/regs_$$.o
