#!/usr/bin/env python3
"""Every kernel of two builds side by side (development aid): isa_compare.py PARENT_DIR NEW_DIR

Each directory holds what `make -C carparkingmaps_amd/csrc asm ASMDIR=<dir> 2> <dir>/remarks.txt` left there: the gfx950 listing and the
-Rpass-analysis=kernel-resource-usage remarks.  Per kernel: the static instruction counts of tools/isa_count.py (total, VALU, SALU, DS) and
the remarks' registers, spills, scratch, occupancy and LDS; `same`, CHANGED, NEW or REMOVED.  profiles/flows_isa_compare.txt is one."""
import re, sys, subprocess
from collections import Counter
def counts(path):
    s = open(path).read()
    out = {}
    for m in re.finditer(r'^(_Z[\w]+):', s, flags=re.M):
        name = m.group(1)
        a = m.start(); b = s.find('.Lfunc_end', a)
        if b < 0: continue
        lines = [l.strip() for l in s[a:b].split('\n') if l.strip() and not l.strip().startswith(('.', ';', '//')) and not l.strip().endswith(':')]
        c = Counter(l.split()[0] for l in lines)
        out[name] = dict(total=len(lines), valu=sum(v for k, v in c.items() if k.startswith('v_')), salu=sum(v for k, v in c.items() if k.startswith('s_')),
                         ds=sum(v for k, v in c.items() if k.startswith('ds_')))
    return out
def remarks(path):
    out = {}; cur = None
    for l in open(path):
        m = re.search(r'remark: [^ ]+ +Function Name: (\S+)', l)
        if m: cur = m.group(1); out[cur] = {}; continue
        m = re.search(r'remark: [^ ]+ +(TotalSGPRs|VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|SGPRs Spill|VGPRs Spill|LDS Size \[bytes/block\]): (\S+)', l)
        if m and cur: out[cur][m.group(1)] = m.group(2)
    return out
P, N = sys.argv[1], sys.argv[2]
S = 'cpm_api-hip-amdgcn-amd-amdhsa-gfx950.s'
cp, cn = counts(f'{P}/{S}'), counts(f'{N}/{S}')
rp, rn = remarks(f'{P}/remarks.txt'), remarks(f'{N}/remarks.txt')
demangle = lambda names: dict(zip(names, subprocess.run(['c++filt'], input='\n'.join(names), capture_output=True, text=True).stdout.split('\n')))
names = sorted(set(cp) | set(cn))
dm = demangle(names)
lines = ['columns: instructions total/valu/salu/ds | SGPRs/VGPRs/AGPRs scratch occupancy spills(s/v) LDS', '']
diff = 0
def fmt(c, r):
    r = r or {}
    g = lambda k: r.get(k, '?')
    return (f"{c['total']}/{c['valu']}/{c['salu']}/{c['ds']} | {g('TotalSGPRs')}/{g('VGPRs')}/{g('AGPRs')} {g('ScratchSize [bytes/lane]')} "
            f"{g('Occupancy [waves/SIMD]')} {g('SGPRs Spill')}/{g('VGPRs Spill')} {g('LDS Size [bytes/block]')}")
for n in names:
    a, b, ra, rb = cp.get(n), cn.get(n), rp.get(n), rn.get(n)
    if a is None:
        lines.append(f'NEW      {fmt(b, rb)}  {dm[n]}')
    elif b is None:
        lines.append(f'REMOVED  {fmt(a, ra)}  {dm[n]}'); diff += 1
    elif a != b or ra != rb:
        lines.append(f'CHANGED  {dm[n]}\n         parent {fmt(a, ra)}\n         new    {fmt(b, rb)}'); diff += 1
    else:
        lines.append(f'same     {fmt(b, rb)}  {dm[n]}')
print(f'kernels in the parent tree: {len(cp)}, in this tree: {len(cn)}; changed or removed: {diff}')
print('\n'.join(lines))
