#!/usr/bin/env python3
"""Instruction mix of the two event kernels' inner loops from the gfx950 ISA (hipcc -save-temps).
usage: python tools/isa_mix.py <file.s> > profiles/rNN/isa_instruction_mix.md

For each kernel the event loop is located (the innermost loop that contains v_exp_f32), its basic blocks are listed, and the
blocks of the common case - every tap inside the LDS window - are summed per instruction class.  The loops are unrolled by the
source (x3, or x2), and the compiler may gather the tap arithmetic of all events of a trip in one block: the per-event figure is
the trip's sum divided by the events per trip."""
import re
import sys
from collections import Counter, OrderedDict

CLASSES = OrderedDict([
    ('fp64 (add/mul/fma/rndne/cvt to or from f64)', re.compile(r'^v_(add|mul|fma|rndne|fract|min|max)_f64|^v_cvt_(f64_|[a-z0-9]+_f64)')),
    ('transcendental (exp/rcp/rsq/log/sqrt)', re.compile(r'^v_(exp|rcp|rsq|log|sqrt)_f32')),
    ('packed fp32 (v_pk_*)', re.compile(r'^v_pk_')),
    ('fp32 arithmetic', re.compile(r'^v_(add|sub|subrev|mul|fma|fmac|fmaak|fmamk|mac|mad|max|min|med3|rndne|fract)_f32|^v_(max3|min3)_f32')),
    ('convert (fp32 <-> int, no f64)', re.compile(r'^v_cvt_')),
    ('integer / address / select / move', re.compile(r'^v_(add|sub|subrev|mul|mad|lshl|lshr|ashr|and|or|xor|bfe|bfi|cndmask|mov|add3|lshl_add|lshl_or|and_or|or3|mad_u|mul_i|mul_u|min|max|med3|cmp|cmpx|readfirstlane|readlane|writelane|perm|alignbit|mbcnt|accvgpr)')),
    ('LDS (ds_*)', re.compile(r'^ds_')),
    ('global / flat memory', re.compile(r'^(global|flat|buffer|scratch)_')),
    ('scalar ALU / control (s_*)', re.compile(r'^s_')),
])


def classify(op):
    for name, rx in CLASSES.items():
        if rx.match(op):
            return name
    return 'other: ' + op


def kernels(text):
    for m in re.finditer(r'^(_ZN5eincm[^\n:]*):[^\n]*\n(.*?)\n\s*s_endpgm', text, re.S | re.M):
        yield m.group(1), m.group(2)


def blocks(body):
    cur, name, out = [], 'entry', []
    for line in body.splitlines():
        line = line.strip()
        m = re.match(r'^(\.LBB\d+_\d+):(.*)', line)
        if m:
            out.append((name, cur)); name, cur = m.group(1), []
            LOOP[name] = None
            line = m.group(2).strip()
        if line.startswith(';') and not cur and not name.endswith('+'):       # the compiler's own loop annotation of the label (one or two lines)
            h = re.search(r'in Loop: Header=(BB\d+_\d+)', line)
            if h:
                LOOP[name] = '.L' + h.group(1)
            elif 'Inner Loop Header' in line:
                LOOP[name] = name
            continue
        if not line or line.startswith(';') or line.startswith('.') or line.startswith('//'):
            continue
        op = line.split()[0]
        cur.append(op)
        if op.startswith('s_cbranch') or op == 's_branch':          # a branch ends the basic block: what follows is the fall-through path
            out.append((name, cur)); name, cur = name + '+', []
    out.append((name, cur))
    return out


LOOP = {}           # label -> header label of the innermost loop it belongs to (labels are unique over the file)


def event_loop(bl):
    """The blocks of the first innermost loop that holds the tap arithmetic (>= 3 v_exp_f32), in layout order."""
    for n, _ in bl:
        if LOOP.get(n) == n:
            body = [(m, ops) for m, ops in bl if LOOP.get(m.rstrip('+')) == n]
            if sum(o == 'v_exp_f32_e32' for _, ops in body for o in ops) >= 3:
                return body
    return []


def main():
    text = open(sys.argv[1]).read()
    want = [('k_splat<THETA_CONST>  (2-DoF theta, the bench configuration)', 'k_splatILi1E', 'ds_add_u32', 3),
            ('k_gather<THETA_CONST, 0>  (2-DoF theta)', 'k_gatherILi1ELi0E', 'ds_read', 1),
            ('k_splat<THETA_TILE>  (pyramid levels >= 1, dense)', 'k_splatILi2E', 'ds_add_u32', 3),
            ('k_gather<THETA_TILE, 0>', 'k_gatherILi2ELi0E', 'ds_read', 1)]
    print('# Instruction mix of the event kernels\' inner loops (gfx950 ISA, hipcc -O3, `tools/isa_mix.py`)\n')
    print('Counted from the disassembly: the basic blocks of the event loop that run in the common case (every tap of the event inside the LDS\n'
          'window).  "per event" = per lane-event and reference time, i.e. per warped event.  The out-of-window path (taps sent straight to HBM with\n'
          'the JAX wrap/drop rule) and the per-workgroup prologue / epilogue are excluded; they are in the PMC totals (`SQ_INSTS_VALU`).\n')
    for title, key, marker, events_per_trip in want:
        body = next((b for n, b in kernels(text) if key in n), None)
        if body is None:
            print(f'## {title}\n\nnot found\n'); continue
        bl = blocks(body)

        def has(ops, prefix, n):
            return sum(o.startswith(prefix) for o in ops) >= n
        # The common case inside the event loop (event_trips: unrolled x3 with renamed registers, or #pragma unroll 2): every block
        # but the out-of-window path, which runs from the block that warps an event and tests its taps against the window (fp64
        # arithmetic, closed by s_cbranch_execz) to the block with the nine LDS operations of that event.  One such block = one event.
        marker_n = 9 if marker == 'ds_add_u32' else 6
        fast, slow, events_per_trip = [], False, 0
        for n, ops in event_loop(bl):
            if slow and not has(ops, marker, marker_n):
                continue
            slow = False
            fast.append((n, ops))
            events_per_trip += has(ops, marker, marker_n)
            if ops and ops[-1] == 's_cbranch_execz' and sum('_f64' in o for o in ops) >= 8:
                slow = True
        events_per_trip = max(events_per_trip, 1)
        tot = Counter()
        for n, ops in fast:
            for o in ops:
                tot[classify(o)] += 1
        nvalu = sum(v for k, v in tot.items() if not k.startswith(('LDS', 'global', 'scalar', 'other')))
        print(f'## {title}\n')
        print(f'fast-path blocks: {", ".join(n for n, _ in fast)}; events per loop trip (unroll): {events_per_trip}\n')
        print('| class | instructions per warped event |')
        print('|---|---|')
        for k in list(CLASSES) + sorted(k for k in tot if k.startswith('other')):
            if tot.get(k):
                print(f'| {k} | {tot[k] / events_per_trip:.1f} |')
        print(f'| **VALU total** | **{nvalu / events_per_trip:.1f}** |\n')


if __name__ == '__main__':
    main()
