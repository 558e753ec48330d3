#!/usr/bin/env python3
# tools/barrier_intervals.py <file.s> <kernel name substring>: instructions of one kernel between consecutive s_barrier, in
# program order: VALU, LDS reads, LDS writes, ds_bpermute, global loads / stores, scratch accesses.  The assembly comes from
# tools/regs.sh (-save-temps).  Intervals of the row loop with LDS traffic and no VALU are the ones where every wave of the
# workgroup waits for the LDS at once.
import re
import sys

path, want = sys.argv[1], sys.argv[2]
rows, cur, inside = [], None, False
for line in open(path):
    m = re.match(r'^(\S+):', line)
    if m and not line.startswith('.L'):
        inside = re.search(r'\d' + re.escape(want), m.group(1)) is not None and not m.group(1).endswith('.kd')    # mangled: <length><name>
        if inside:
            cur = dict(valu=0, rd=0, rd2=0, wr=0, bperm=0, gld=0, gst=0, scr=0)
            rows = [cur]
        continue
    if not inside:
        continue
    op = line.split()[0] if line.split() else ''
    if op == 's_endpgm':
        inside = False
    elif op == 's_barrier':
        cur = dict(valu=0, rd=0, rd2=0, wr=0, bperm=0, gld=0, gst=0, scr=0)
        rows.append(cur)
    elif op.startswith('scratch_'):
        cur['scr'] += 1
    elif op.startswith('ds_bpermute'):
        cur['bperm'] += 1
    elif op.startswith('ds_read2'):
        cur['rd2'] += 1
    elif op.startswith('ds_read'):
        cur['rd'] += 1
    elif op.startswith('ds_write'):
        cur['wr'] += 1
    elif op.startswith('buffer_load'):
        cur['gld'] += 1
    elif op.startswith('buffer_store'):
        cur['gst'] += 1
    elif op.startswith('v_'):
        cur['valu'] += 1
print('interval  VALU  ds_read  ds_read2  ds_write  bpermute  loads  stores  scratch')
for i, r in enumerate(rows):
    print(f"{i:8d} {r['valu']:5d} {r['rd']:8d} {r['rd2']:9d} {r['wr']:9d} {r['bperm']:9d} {r['gld']:6d} {r['gst']:7d} {r['scr']:8d}")
print('total VALU', sum(r['valu'] for r in rows))
