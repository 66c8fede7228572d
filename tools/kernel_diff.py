"""Which kernels differ between two builds of the library, read from their gfx950 code objects (no GPU).

A refactor that promises "the same kernels" is checked here instead of by a timing run: every
kernel of A.so and B.so is disassembled, addresses and encodings are dropped (a kernel that only
moved inside its code object, or to another translation unit, compares equal; branch operands are
relative and their targets are kept as offsets from the kernel's start), and the instruction
streams and the metadata (VGPR / AGPR / SGPR counts, LDS and scratch bytes) are compared by symbol
name.  Kernels present on one side only are listed too.  Exit status 1 if anything differs.

Usage: python tools/kernel_diff.py A.so B.so [name-substring ...]
"""
import re
import subprocess
import sys
import tempfile

from kernel_regs import READELF, code_objects, demangled, kernel_resources

OBJDUMP = '/opt/rocm/lib/llvm/bin/llvm-objdump'
KEYS = ('vgpr', 'agpr', 'sgpr', 'lds', 'scratch')


def kernel_streams(path, names, arch='gfx950'):
    """{symbol: [instruction lines]} for the symbols in `names`, over all code objects of the library."""
    out = {}
    for img in code_objects(path, arch):
        with tempfile.NamedTemporaryFile(suffix='.co') as f:
            f.write(img)
            f.flush()
            txt = subprocess.run([OBJDUMP, '-d', f.name], capture_output=True, text=True, check=True).stdout
            sym = subprocess.run([READELF, '-sW', f.name], capture_output=True, text=True, check=True).stdout
        # a function symbol's size ends at its last instruction: the padding up to the next symbol,
        # which depends on what follows the kernel in its code object, is not compared
        size = {r[7]: int(r[2]) for r in (l.split() for l in sym.splitlines()) if len(r) == 8 and r[3] == 'FUNC'}
        cur, end = None, 0
        for line in txt.splitlines():
            m = re.match(r'^([0-9a-f]+) <(\S+)>:$', line)
            if m:
                cur = out.setdefault(m.group(2), []) if m.group(2) in names else None
                end = int(m.group(1), 16) + size.get(m.group(2), 0)
                continue
            if cur is None or not line.startswith('\t'):
                continue
            ins, _, note = line.partition('//')
            addr = re.match(r'\s*([0-9A-Fa-f]+):', note)
            if not addr or int(addr.group(1), 16) >= end:   # no address: the '...' of a run of zeros
                continue
            tgt = re.search(r'<\S+?(\+0x[0-9a-f]+)?>\s*$', note)   # a branch: '<kernel+0xoff>'
            cur.append(' '.join(ins.split()) + (' -> ' + (tgt.group(1) or '+0x0') if tgt else ''))
    return out


def main(argv):
    if len(argv) < 2:
        sys.exit(__doc__)
    a, b, pats = argv[0], argv[1], argv[2:]
    ra, rb = kernel_resources(a), kernel_resources(b)
    dm = demangled(sorted(set(ra) | set(rb)))
    names = sorted((k for k in dm if not pats or any(p in dm[k] for p in pats)), key=lambda k: dm[k])
    sa, sb = kernel_streams(a, set(names)), kernel_streams(b, set(names))
    ndiff = 0
    for k in names:
        if k not in ra or k not in rb:
            print('only in %s: %s' % ('A' if k in ra else 'B', dm[k]))
            ndiff += 1
            continue
        what = []
        meta = [key for key in KEYS if ra[k][key] != rb[k][key]]
        if meta:
            what.append(', '.join('%s %d -> %d' % (key, ra[k][key], rb[k][key]) for key in meta))
        if sa.get(k) != sb.get(k):
            what.append('instructions %d -> %d lines' % (len(sa.get(k, [])), len(sb.get(k, []))))
        if what:
            print('differs: %s\n    %s\n    A: %s\n    B: %s' % (
                dm[k], '; '.join(what), ' '.join('%s %d' % (key, ra[k][key]) for key in KEYS),
                ' '.join('%s %d' % (key, rb[k][key]) for key in KEYS)))
            ndiff += 1
    print('%d kernels compared, %d differ' % (len(names), ndiff))
    return 1 if ndiff else 0


if __name__ == '__main__':
    sys.exit(main(sys.argv[1:]))
