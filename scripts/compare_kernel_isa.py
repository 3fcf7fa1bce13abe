#!/usr/bin/env python3
"""Compare the device code of two builds kernel by kernel.

    hipcc <the Makefile's FLAGS> --cuda-device-only -S unit.hip -o before/unit.s      (every unit of interest, both trees)
    scripts/compare_kernel_isa.py before/ after/

For every `.amdhsa_kernel` symbol found in the `*.s` files of a directory (searched recursively; the units a kernel lives in do
not matter) it takes the instruction stream from the kernel's label to its last s_endpgm and the `.amdhsa_*` descriptor block (register
counts, accum_offset, LDS and scratch bytes).  Comments, blank lines and trailing space are dropped and the function ordinal is
taken out of local labels (.LBB12_3 -> .LBB_3), so that a kernel that merely moved to another file or position compares equal.
Reports kernels that are missing, added or different; exit status 1 on any difference, or on a symbol defined twice in one tree.

    scripts/compare_kernel_isa.py --reordered before/ after/

also sorts the different kernels: one with an equal descriptor, an equal number of instructions and an equal multiset of opcodes (the
same work, scheduled elsewhere or in other registers) is reported as `reordered`, not `different`.  The exit status stays 1: a
reordered kernel still owes a comparison of its output bits.
"""
import re
import sys
from collections import Counter
from pathlib import Path

LOCAL_LABEL = re.compile(r'(\.L[A-Za-z_$]+)\d+_')


def clean(line):
    line = line.split(';', 1)[0].split('//', 1)[0].rstrip()
    return LOCAL_LABEL.sub(r'\1_', line)


def kernels_of(directory):
    """symbol -> (instruction lines, descriptor lines); also the symbols defined more than once"""
    found, twice = {}, []
    for path in sorted(Path(directory).rglob('*.s')):
        lines = path.read_text(errors='replace').split('\n')
        labels = {m.group(1): i for i, l in enumerate(lines) if (m := re.match(r'^([A-Za-z_$][\w$.]*):', l))}
        for i, l in enumerate(lines):
            m = re.match(r'^\s*\.amdhsa_kernel\s+(\S+)', l)
            if not m:
                continue
            name = m.group(1)
            desc = []
            for d in lines[i + 1:]:
                if d.strip().startswith('.end_amdhsa_kernel'):
                    break
                if clean(d).strip():
                    desc.append(clean(d).strip())
            code = []
            for c in lines[labels[name] + 1:]:
                if re.match(r'^\.Lfunc_end\d+:', c):     # (a kernel may hold several s_endpgm: the stream ends with its last)
                    break
                c = clean(c).strip()
                if c and not re.match(r'^\.(p2align|loc|file|cfi_\w+)\b', c):
                    code.append(c)
            while code and code[-1] != 's_endpgm':
                code.pop()
            if name in found:
                twice.append(name)
            found[name] = (code, desc)
    return found, twice


def first_difference(a, b):
    for n, (x, y) in enumerate(zip(a, b)):
        if x != y:
            return 'line %d: %r != %r' % (n, x, y)
    return 'length %d != %d' % (len(a), len(b))


def opcodes(code):
    return Counter(c.split()[0] for c in code if not c.endswith(':'))


def main():
    sort_reordered = '--reordered' in sys.argv
    sys.argv = [a for a in sys.argv if a != '--reordered']
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    (before, twice_b), (after, twice_a) = kernels_of(sys.argv[1]), kernels_of(sys.argv[2])
    missing, added = sorted(set(before) - set(after)), sorted(set(after) - set(before))
    different, reordered = [], []
    for name in sorted(set(before) & set(after)):
        (code_b, desc_b), (code_a, desc_a) = before[name], after[name]
        if sort_reordered and code_b != code_a and desc_b == desc_a and len(code_b) == len(code_a) and opcodes(code_b) == opcodes(code_a):
            reordered.append('%s: %d instructions' % (name, len(code_a)))
            continue
        for what, x, y in (('instructions', before[name][0], after[name][0]), ('descriptor', before[name][1], after[name][1])):
            if x != y:
                different.append('%s: %s, %s' % (name, what, first_difference(x, y)))
    for title, items in (('missing', missing), ('added', added), ('different', different), ('reordered', reordered),
                         ('defined twice in ' + sys.argv[1], twice_b), ('defined twice in ' + sys.argv[2], twice_a)):
        for item in items:
            print('%s: %s' % (title, item))
    n_different = len({d.split(':')[0] for d in different})
    print('%d kernels before, %d after: %d identical, %d different, %d missing, %d added, %d defined twice'
          % (len(before), len(after), len(set(before) & set(after)) - n_different - len(reordered),
             n_different, len(missing), len(added), len(twice_b) + len(twice_a))
          + (', %d reordered' % len(reordered) if sort_reordered else ''))
    return 1 if (missing or added or different or reordered or twice_b or twice_a) else 0


if __name__ == '__main__':
    sys.exit(main())
