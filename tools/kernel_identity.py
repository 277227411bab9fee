#!/usr/bin/env python3
"""Dev tool: are the gfx950 kernels of two builds of libdeepmod_hip.so the same?  For every kernel symbol of either library: present in
both, the same resource record (registers, LDS, private segment, spills) and the same instruction sequence, where a branch's absolute
target address is dropped (its <symbol+offset> stays), and so is the s_nop fill behind the last kernel of a code object.  What a change that only moves code between translation units has to show.
    tools/kernel_identity.py PARENT.so NEW.so [--rename OLD=NEW ...]  ->  a table on stdout, exit status 1 if a kernel differs.
--rename OLD=NEW: the one kernel of the parent whose symbol contains OLD is compared with the one kernel of the new library whose symbol
contains NEW (a kernel that became an instantiation of a template); a pair that differs is reported like any other, with its sizes."""
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


def renamed(a, b, pairs):
    """The parent's kernels with every renamed one under its new symbol, in its record's key and in its own branch targets."""
    for pair in pairs:
        old, new = pair.split("=", 1)
        was, now = [k for k in a if old in k], [k for k in b if new in k]
        if len(was) != 1 or len(now) != 1:
            sys.exit("--rename %s: %d kernels of the parent contain %r, %d of the new library contain %r (one each is needed)" % (pair, len(was), old, len(now), new))
        res, ins = a.pop(was[0])
        a[now[0]] = (res, [i.replace("<" + was[0], "<" + now[0]) for i in ins])
        print("renamed: %s -> %s" % (was[0], now[0]))
    return a


def main(parent, new, pairs=()):
    b = kernels(new)
    a = renamed(kernels(parent), b, pairs)
    differing = []
    for k in sorted(set(a) | set(b)):
        if k not in a or k not in b:
            differing.append("%s: only in %s" % (k, "the parent" if k in a else "the new library"))
        elif a[k][0] != b[k][0]:
            differing.append("%s: resources %r -> %r; %d -> %d instructions" % (k, a[k][0], b[k][0], len(a[k][1]), len(b[k][1])))
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
    args = sys.argv[1:]
    pairs = [args[i + 1] for i, v in enumerate(args) if v == "--rename"]
    libs = [v for i, v in enumerate(args) if v != "--rename" and (i == 0 or args[i - 1] != "--rename")]
    sys.exit(main(libs[0], libs[1], pairs))
