"""profiles/ref_path/compare.py: every kernel of kernels_parent.txt must reappear in kernels_result.txt under the same name in
the same translation unit; prints the ones whose registers, scratch, LDS or spill counts differ (the instruction-text hashes
differ almost everywhere: the argument block grew by two words, which moves the offsets of the arguments behind it)."""
import os, re
here = os.path.dirname(os.path.abspath(__file__))
FIELDS = ("agpr", "vgpr", "sgpr", "scratch", "lds", "spilled v", "spilled s")


def load(f):
    d = {}
    for l in open(os.path.join(here, f)):
        tu, rest = l.split('  ', 1)
        m = re.match(r'(.*?)\s+agpr\s+(\d+) vgpr\s+(\d+) sgpr\s+(\d+) scratch\s+(\d+) lds\s+(\d+) spilled v\s+(\d+) s\s+(\d+) hash', rest)
        d[(tu, m.group(1))] = [int(v) for v in m.groups()[1:]]
    return d


P, R = load('kernels_parent.txt'), load('kernels_result.txt')
assert set(P) == set(R), set(P) ^ set(R)
worse = 0
for k in sorted(P):
    if P[k] != R[k]:
        print('%-24s %-62s %s' % (k[0], k[1], ', '.join('%s %d -> %d' % (n, a, b) for n, a, b in zip(FIELDS, P[k], R[k]) if a != b)))
        worse += any(b > a for n, a, b in zip(FIELDS, P[k], R[k]) if n in ("agpr", "vgpr", "sgpr", "scratch"))
print('%d kernels, %d with other numbers, %d of them with more registers or scratch' % (len(P), sum(P[k] != R[k] for k in P), worse))
