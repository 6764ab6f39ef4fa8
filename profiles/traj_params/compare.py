"""profiles/traj_params/compare.py: every line of kernels_parent.txt must reappear in kernels_result.txt in the same
translation unit with the same metadata and hash; a kernel family that gained the TP switch reappears with `, false`
appended to its template arguments.  Prints the verdict and the number of new instantiations."""
import os, re
here = os.path.dirname(os.path.abspath(__file__))


def load(f):
    d = {}
    for l in open(os.path.join(here, f)):
        tu, rest = l.split('  ', 1)
        m = re.match(r'(.*?)\s+(agpr .*)$', rest.rstrip())
        d[(tu, m.group(1))] = m.group(2)
    return d


P, R = load('kernels_parent.txt'), load('kernels_result.txt')
bad = 0
for (tu, n), v in sorted(P.items()):
    hit = [c for c in (n, n[:-1] + ', false>') if (tu, c) in R]
    if not hit or R[(tu, hit[0])] != v:
        bad += 1
        print('DIFFERS', tu, n)
print('%d parent kernels, %d differ, %d new instantiations' % (len(P), bad, len(R) - len(P)))
raise SystemExit(1 if bad else 0)
