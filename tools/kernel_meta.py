"""Register / scratch / LDS metadata of every kernel in a gfx950 assembly file (hipcc -S --cuda-device-only), and a hash
of its instruction text: tools/kernel_meta.py file.s [name-filter]
The hash covers the lines from the kernel's label to .end_amdhsa_kernel without comments and with the function
index taken out of local labels (.LBB<k>_<n>, .Lfunc_end<k>: it only counts the kernels of the file), so that two builds
can be compared kernel by kernel (profiles/launch_table/).  With a third argument the kernel's own mangled name is taken out
of the hashed text too, so that a kernel whose template argument list grew compares equal when its instructions did not
change (profiles/traj_params/)."""
import hashlib, re, subprocess, sys
s = open(sys.argv[1]).read()
flt = sys.argv[2] if len(sys.argv) > 2 else ""


def text_hash(name):
    body = s[s.index('\n%s:' % name) + 1:]
    body = body[:body.index('.end_amdhsa_kernel')]
    lines = [l.split(';')[0].rstrip() for l in body.split('\n')]  # (comments: whole lines and the loop notes behind labels)
    lines = [l for l in lines if l]
    body = re.sub(r'\.L(BB|func_begin|func_end|tmp)\d+', r'.L\1', '\n'.join(lines))
    if len(sys.argv) > 3:
        body = body.replace(name, 'KERNEL')
    return hashlib.sha1(body.encode()).hexdigest()[:16]


meta = s[s.index('amdhsa.kernels'):]
for blk in meta.split('  - .agpr_count:')[1:]:
    name = re.search(r'\.name:\s+(\S+)', blk).group(1)
    g = lambda k: re.search(r'\.%s:\s+(\d+)' % k, blk).group(1)
    dn = subprocess.run(['c++filt', name], capture_output=True, text=True).stdout.strip()
    dn = re.sub(r'\(aslr::KArgs.*', '', dn).replace('void aslr::', '')
    if flt and flt not in dn: continue
    print('%-60s agpr %3s vgpr %3s sgpr %3s scratch %5s lds %6s spilled v %4s s %4s hash %s' % (
        dn[:60], blk.split()[0], g('vgpr_count'), g('sgpr_count'), g('private_segment_fixed_size'),
        g('group_segment_fixed_size'), g('vgpr_spill_count'), g('sgpr_spill_count'), text_hash(name)))
