#!/usr/bin/env python3
"""Dev tool: are the gfx950 kernels of two builds of libdeepmod_hip.so the same?  For every kernel symbol of either library: present in
both, the same resource record (registers, LDS, private segment, spills) and the same instruction sequence, where a branch's absolute
target address is dropped (its <symbol+offset> stays), and so is the s_nop fill behind the last kernel of a code object.  What a change that only moves code between translation units has to show.
    tools/kernel_identity.py PARENT.so NEW.so  ->  a table on stdout, exit status 1 if a kernel differs."""
import re
import sys
import tempfile

import isa_lint


def kernels(lib):
    with tempfile.TemporaryDirectory(prefix="dm_kernel_identity_") as tmp:
        meta, dis = {}, {}
        for co in isa_lint.extract_code_objects(lib, tmp):
            meta.update(isa_lint.kernel_metadata(co))
            dis.update(isa_lint.disassemble(co))
    out = {}
    for k, m in meta.items():
        ins = [re.sub(r"\s(0x[0-9a-f]+|\d+) (<[^>]+>)$", r" \2", i) for i in dis[k] if i != "..."]
        while ins and ins[-1] == "s_nop 0":        # the fill between the last s_endpgm of a code object and its end belongs to no kernel
            ins.pop()
        assert ins, k
        out[k] = ({f: v for f, v in m.items() if f != "name"}, ins)
    return out


def main(parent, new):
    a, b = kernels(parent), kernels(new)
    differing = []
    for k in sorted(set(a) | set(b)):
        if k not in a or k not in b:
            differing.append("%s: only in %s" % (k, "the parent" if k in a else "the new library"))
        elif a[k][0] != b[k][0]:
            differing.append("%s: resources %r -> %r" % (k, a[k][0], b[k][0]))
        elif a[k][1] != b[k][1]:
            first = next((i for i, (x, y) in enumerate(zip(a[k][1], b[k][1])) if x != y), min(len(a[k][1]), len(b[k][1])))
            differing.append("%s: %d -> %d instructions, first difference at %d: %r -> %r" %
                             (k, len(a[k][1]), len(b[k][1]), first, a[k][1][first:first + 1], b[k][1][first:first + 1]))
    print("kernels: %d in the parent, %d in the new library; identical (name, resources, instructions): %d; differing: %d" %
          (len(a), len(b), len(set(a) | set(b)) - len(differing), len(differing)))
    print("instructions compared: %d" % sum(len(v[1]) for v in a.values()))
    for line in differing:
        print("  DIFFERS " + line)
    return 1 if differing else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
