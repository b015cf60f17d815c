#!/bin/bash
# kernel resource usage (VGPRs, SGPRs, LDS, scratch, occupancy) of the given files of csrc/ (default:
# hrt_kernels.hip), e.g. profiles/kres.sh hrt_channel.hip hrt_power.hip -- compile-only, no GPU
cd "$(dirname "$0")/../hermespy-rt_amd"
for f in "${@:-hrt_kernels.hip}"; do
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -fPIC -ffp-contract=off -fno-slp-vectorize -I../include -Icsrc $EXTRA \
  -c "csrc/$f" -o /tmp/kres.o -Rpass-analysis=kernel-resource-usage 2>&1 | python3 -c "
import sys,re
cur=None
for l in sys.stdin:
    m=re.search(r'remark:\s+(.*?) \[-Rpass', l)
    if not m: continue
    t=m.group(1).strip()
    if t.startswith('Function Name') or t.startswith('Name:'):
        if cur: print(cur)
        n=t.split(':',1)[1].strip()
        n=re.sub(r'_ZN12_GLOBAL__N_1\d+','',n)
        cur=n[:40].ljust(42)
    elif any(t.startswith(k) for k in ('VGPRs:','SGPRs:','TotalSGPRs','ScratchSize','Occupancy','SGPRs Spill','VGPRs Spill','LDS Size')):
        cur+=' '+t.replace(' [bytes/lane]','').replace(' [waves/SIMD]','').replace(' [bytes/block]','')
if cur: print(cur)
"
done
