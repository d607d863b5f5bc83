#!/usr/bin/env python3
"""Developer tool: which kernels differ between two device-assembly files of the library.

Build each with the hipcc line of build() plus `--cuda-device-only -S -o X.s`, then

    python tools/kernel_diff.py PARENT.s NEW.s

It lists every kernel whose instruction text differs (or that only one file has), with its instruction counts and the .amdhsa
register, LDS and scratch lines of both.  It compares text only, with one allowance: the compiler numbers a function's local labels
(.LBB<f>_<n>, .LJTI<f>_<n>) by the function's place <f> in the module, which moves when other kernels are instantiated in another
order, so <f> is dropped before the comparison.  A kernel whose instructions agree and whose resource lines do not is listed too.
Exit status 0; the list is the result.
"""
import re
import sys

RESOURCES = ('.amdhsa_next_free_vgpr', '.amdhsa_next_free_sgpr', '.amdhsa_accum_offset', '.amdhsa_group_segment_fixed_size',
             '.amdhsa_private_segment_fixed_size')


def kernels(path):
    """name -> (instruction lines, {resource: value})"""
    text = open(path).read()
    body, res = {}, {}
    for m in re.finditer(r'^(\w+):\s*(?:;[^\n]*)?\n(.*?)^\s*\.size\s+\1,', text, re.S | re.M):
        name, lines = m.group(1), []
        for ln in m.group(2).splitlines():
            ln = ln.split(';')[0].strip()
            if ln and not ln.startswith('.') and not ln.endswith(':'):
                lines.append(re.sub(r'\.(LBB|LJTI)\d+_', r'.\1_', re.sub(r'\s+', ' ', ln)))
        body[name] = lines
    for m in re.finditer(r'^\s*\.amdhsa_kernel\s+(\w+)\n(.*?)^\s*\.end_amdhsa_kernel', text, re.S | re.M):
        res[m.group(1)] = {k: v for k, v in re.findall(r'^\s*(\.amdhsa_\w+)\s+(\S+)', m.group(2), re.M) if k in RESOURCES}
    return {n: (body[n], r) for n, r in res.items() if n in body}


def main():
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    same = 0
    for name in sorted(set(a) | set(b)):
        if name not in a or name not in b:
            print(f'{name}: only in {sys.argv[1] if name in a else sys.argv[2]}')
        elif a[name] == b[name]:
            same += 1
        else:
            print(f'{name}: instructions {len(a[name][0])} -> {len(b[name][0])}')
            for k in RESOURCES:
                print(f'    {k} {a[name][1].get(k)} -> {b[name][1].get(k)}')
    print(f'{same} kernels identical of {len(set(a) | set(b))}')
    return 0


if __name__ == '__main__':
    sys.exit(main())
