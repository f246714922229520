#!/usr/bin/env python
"""The dependent memory round trips of a kernel's loops, read from its ISA (no GPU):
   tools/waitchain.py /tmp/k.s _Z6k_slotILi3ELb0EE [min_lines] [-v | -q]
(how the ISA is made: see tools/spillmap.py).  A pass of the slot kernel is a chain of loads that each need what the load before
brought; what the chain costs is the number of times the wave stands in front of an `s_waitcnt vmcnt` with loads still out.  For
every loop of the kernel (innermost text ranges closed by a backward branch, at least min_lines long) this prints
  * the sequence of vector-memory operations and of the vmcnt waits that retire some of them, in text order, per basic block;
  * the number of LOAD GROUPS: loads issued together and retired by one wait, or by several waits with no load between them
    (vmcnt(2), vmcnt(1), vmcnt(0) on loads that went out together are ONE round trip) - the dependent round trips;
  * per load, the instructions between it and the first wait that retires it (what runs beside its round trip).
The walk is in TEXT order: a loop body with branches is walked through every block once, the counter carried over block ends, so
the groups of an `if / else` stand one behind the other (the blocks' labels say where one ends).  vmcnt counts loads, stores and
returning atomics alike and retires them in order (gfx9); a wait `vmcnt(n)` leaves the youngest n in flight.  Scratch loads (spill
reloads) are vector-memory operations like any other and are marked.  Without -v only the summary line and the groups are printed, with -q the summary line alone."""
import re
import sys

args = [a for a in sys.argv[1:] if a not in ('-v', '-q')]
verbose = '-v' in sys.argv[1:]
quiet = '-q' in sys.argv[1:]
txt = open(args[0]).read()
m = re.search(r'^(%s[^\n]*):' % re.escape(args[1]), txt, re.M)
i = m.start(); j = txt.index('.Lfunc_end', i)
lines = txt[i:j].split('\n')
minl = int(args[2]) if len(args) > 2 else 300

labels = {}
for n, l in enumerate(lines):
    mm = re.match(r'^(\.LBB\d+_\d+):', l)
    if mm:
        labels[mm.group(1)] = n
loops = set()
for n, l in enumerate(lines):
    mm = re.search(r's_cbranch_\w+\s+(\.LBB\d+_\d+)|s_branch\s+(\.LBB\d+_\d+)', l)
    if mm:
        t = mm.group(1) or mm.group(2)
        if t in labels and labels[t] < n:
            loops.add((labels[t], n))
loops = sorted(loops)


def is_instr(l):
    l = l.strip()
    return bool(l) and l[0] not in '.;/' and not l.endswith(':')


VMEM = ('buffer_', 'global_', 'scratch_', 'flat_')


def vmem_kind(op, ops):
    """'L' load (or returning atomic / LDS-DMA load), 'S' store (or atomic without a result), None: not vector memory."""
    if not op.startswith(VMEM):
        return None
    if '_load' in op:
        return 'L'
    if '_atomic' in op:
        return 'L' if re.search(r'\b(sc0|glc)\b', ops) else 'S'
    if '_store' in op:
        return 'S'
    return None                                                    # (cache maintenance: buffer_wbl2, buffer_inv ..)


print(m.group(1)[:70], len(lines), 'lines,', len(loops), 'loops')
for a, b in loops:
    if b - a < minl or b - a > 4000:
        continue
    inner = [(x, y) for x, y in loops if a <= x and y <= b and (x, y) != (a, b) and y - x >= minl]
    out = []                                                       # in flight: [kind, op, line, instruction number]
    groups = []                                                    # per retiring wait: the loads it retired
    dist = []                                                      # (op, line, instructions to its retiring wait)
    seq = []
    ni = 0
    n_scratch = 0
    last_wait = 0
    for n in range(a, b + 1):
        l = lines[n]
        mm = re.match(r'^(\.LBB\d+_\d+):', l)
        if mm:
            seq.append('  %s:' % mm.group(1))
            continue
        if not is_instr(l):
            continue
        ni += 1
        s = l.strip()
        op = s.split()[0]
        k = vmem_kind(op, s)
        if k:
            out.append([k, op, n, ni])
            if k == 'L' and op.startswith('scratch_'):
                n_scratch += 1
            seq.append('    %5d  %s %s%s' % (n, 'load ' if k == 'L' else 'store', op, '   <-- scratch' if op.startswith('scratch_') else ''))
            continue
        if op == 's_waitcnt':
            mv = re.search(r'vmcnt\((\d+)\)', s)
            if not mv:
                continue
            keep = int(mv.group(1))
            gone = out[:max(0, len(out) - keep)]
            out = out[len(gone):]
            loads = [g for g in gone if g[0] == 'L']
            for g in loads:
                dist.append((g[1], g[2], ni - g[3] - 1))
            if loads and groups and all(g[3] < last_wait for g in loads):
                groups[-1][2].extend(g[1] for g in loads)           # (issued before the wait before this one: the same round trip)
                seq.append('    %5d  WAIT vmcnt(%d): retires %d load(s) more of group %d' % (n, keep, len(loads), len(groups)))
            elif loads:
                groups.append((n, keep, [g[1] for g in loads]))
                last_wait = ni
                seq.append('    %5d  WAIT vmcnt(%d): retires %d load(s)%s   == group %d' % (n, keep, len(loads), ', %d store(s)' % (len(gone) - len(loads)) if len(gone) > len(loads) else '', len(groups)))
            elif verbose:
                seq.append('    %5d  wait vmcnt(%d): retires %d store(s)' % (n, keep, len(gone)))
    print('loop %5d-%5d: %4d instr | %2d load groups (dependent round trips) | %3d loads, %d from scratch | left in flight at the back edge: %d%s'
          % (a, b, ni, len(groups), len(dist) + sum(1 for g in out if g[0] == 'L'), n_scratch, len(out),
             ' | holds %d inner loop(s): %s' % (len(inner), ' '.join('%d-%d' % x for x in inner)) if inner else ''))
    for gi, (n, keep, ops) in enumerate([] if quiet else groups):
        c = {}
        for o in ops:
            c[o] = c.get(o, 0) + 1
        print('    group %2d, closed at line %5d by vmcnt(%d): %s' % (gi + 1, n, keep, ', '.join('%d x %s' % (v, k) for k, v in c.items())))
    if verbose:
        print('  sequence:')
        print('\n'.join(seq))
        print('  instructions between a load and the first wait that retires it:')
        for op, n, d in dist:
            print('    %5d  %-28s %4d' % (n, op, d))
