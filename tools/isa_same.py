"""Are the kernels of two builds the same instruction sequences? Disassembles both libraries (or
object files) with tools/isa_check.py `kernels_of` and compares every kernel of the first, by
mangled name, opcode for opcode with the second's; kernels only the second has are listed with
their scratch bytes and register counts (`resources_of`). For a change that adds kernel instances
and must leave the existing ones alone.

usage: python tools/isa_same.py OLD NEW   (exit 1 when a kernel of OLD is missing or different)
"""
import sys

import isa_check as ic


def main():
    old, new = sys.argv[1], sys.argv[2]
    ka, kb = ic.kernels_of(old), ic.kernels_of(new)
    same = bad = 0
    for k in sorted(ka):
        if k not in kb:
            print('MISSING  ', k)
            bad += 1
        elif ka[k] != kb[k]:
            print('DIFFERENT', k, len(ka[k]), '->', len(kb[k]), 'instructions')
            bad += 1
        else:
            same += 1
    added = sorted(set(kb) - set(ka))
    res = ic.resources_of(new) if added else {}
    for k in added:
        print('NEW      ', k, res.get(k))
    print(f'{same} kernels with identical opcode sequences, {bad} missing or different, {len(added)} new')
    return 1 if bad else 0


if __name__ == '__main__':
    sys.exit(main())
