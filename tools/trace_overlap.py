"""tools/trace_overlap.py <before_kernel_trace.csv> <after_kernel_trace.csv>: for two rocprofv3 --kernel-trace runs of the plain headline
(bench.py --gpus 1 --steps 20 --warmup 5: five launch sequences of four frames in the timed region) print the timed region's length, which
frame streams share a hardware queue, the mean number of traversal launches resident at once, the mean traversal blocks they ask for per
CU, and the grid of every traversal launch (profiles/r08_notes.md)."""
import csv, sys, collections
def load(fn):
    rows = list(csv.DictReader(open(fn)))
    rows.sort(key=lambda r: int(r['Start_Timestamp']))
    return rows
def trav(n): return 'rp_k_extend' in n or 'rp_k_connect' in n or 'rp_k_tail' in n
for tag, fn in (('before', sys.argv[1]), ('after', sys.argv[2])):
    rows = load(fn)
    frames = [r for r in rows if 'rp_k_extend<false, true' in r['Kernel_Name']]
    # timed region: the last five launch sequences (first extend of each)
    t0 = int(frames[-5]['Start_Timestamp']); t1 = max(int(r['End_Timestamp']) for r in rows)
    reg = [r for r in rows if int(r['Start_Timestamp']) >= t0 - 2000]
    tr = [r for r in reg if trav(r['Kernel_Name'])]
    ev = []
    for r in tr:
        ev.append((int(r['Start_Timestamp']), 1)); ev.append((int(r['End_Timestamp']), -1))
    ev.sort(); cur = 0; last = t0; acc = 0
    blocks_ev = []
    for r in tr:
        b = int(r['Grid_Size_X']) // int(r['Workgroup_Size_X'])
        blocks_ev.append((int(r['Start_Timestamp']), b)); blocks_ev.append((int(r['End_Timestamp']), -b))
    for t, d in ev:
        acc += cur * (t - last); last = t; cur += d
    mean_k = acc / (t1 - t0)
    blocks_ev.sort(); cur = 0; last = t0; acc = 0
    for t, d in blocks_ev:
        acc += cur * (t - last); last = t; cur += d
    mean_b = acc / (t1 - t0) / 256.0
    qs = collections.defaultdict(set)
    for r in reg:
        if r['Kernel_Name'].startswith('void rp_k') or r['Kernel_Name'].startswith('rp_k'):
            qs[r['Queue_Id']].add(r['Stream_Id'])
    grids = collections.Counter()
    for r in tr:
        k = 'extend_first' if 'rp_k_extend<false, true' in r['Kernel_Name'] else 'extend_later' if 'rp_k_extend' in r['Kernel_Name'] else 'connect' if 'connect' in r['Kernel_Name'] else 'tail'
        grids[(k, int(r['Grid_Size_X']) // int(r['Workgroup_Size_X']) // 256)] += 1
    print('%s: timed region %.2f ms (5 launch sequences of 4 frames, %.3f ms per frame); dispatches in the whole trace %d' % (tag, (t1 - t0) / 1e6, (t1 - t0) / 20e6, len(rows)))
    print('  frame streams per hardware queue:', {q: sorted(s, key=int) for q, s in sorted(qs.items())})
    print('  traversal kernels resident at once (time mean over the timed region): %.2f; traversal blocks asked for per CU (time mean): %.2f' % (mean_k, mean_b))
    print('  traversal launches by (kind, blocks per CU):', dict(sorted(grids.items())))
