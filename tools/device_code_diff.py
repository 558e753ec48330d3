#!/usr/bin/env python3
"""Compare the kernels of two device assembly listings (hipcc ... --cuda-device-only -S).

usage: device_code_diff.py A.s B.s [B2.s ...]

Several B listings count as one: a file of A that was split (each is read on its own; a concatenation would run the tail of one
listing into the first kernel of the next).

A kernel is its code, from the symbol's label to its .Lfunc_end, plus its .amdhsa_kernel descriptor block.  The labels that
carry the function's number (.LBB<n>_, .LJTI<n>_, .Ltmp<n>, .Lfunc_end<n>) are rewritten to a neutral form first: they
renumber when the order of instantiation changes.  Comments (';' to the end of the line) are dropped: they name those labels
too ("Header=BB178_4") and are padded to a column that moves with the width of the number.  Prints the kernels only in A, only in B and differing; exits 1 if any.
"""
import re
import sys

LOCAL = re.compile(r"\.(LBB|LJTI|Ltmp|Lfunc_end)\d+")
COMMENT = re.compile(r"[ \t]*;[^\n]*")


def kernels(path):
    text = open(path).read()
    found = {}
    for m in re.finditer(r"^\t\.amdhsa_kernel (\S+)\n.*?^\t\.end_amdhsa_kernel\n", text, re.M | re.S):
        found[m.group(1)] = [None, m.group(0)]
    for m in re.finditer(r"^(\S+):(?:[ \t]*;[^\n]*)?\n.*?^\.Lfunc_end\d+:\n", text, re.M | re.S):
        if m.group(1) in found:
            found[m.group(1)][0] = LOCAL.sub(r".\1N", COMMENT.sub("", m.group(0)))
    return found


def main():
    if len(sys.argv) < 3:
        sys.exit(__doc__)
    a, b = kernels(sys.argv[1]), {}
    for path in sys.argv[2:]:
        b.update(kernels(path))
    only_a, only_b = sorted(set(a) - set(b)), sorted(set(b) - set(a))
    differing = sorted(k for k in set(a) & set(b) if a[k] != b[k] or a[k][0] is None)
    for title, names in (("only in A", only_a), ("only in B", only_b), ("differing", differing)):
        for k in names:
            print("%s: %s" % (title, k))
    print("kernels: %d in A, %d in B; %d only in A, %d only in B, %d differing" % (len(a), len(b), len(only_a), len(only_b), len(differing)))
    sys.exit(1 if only_a or only_b or differing else 0)


if __name__ == "__main__":
    main()
