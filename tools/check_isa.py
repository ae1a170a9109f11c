#!/usr/bin/env python3
"""Register and scratch use of every kernel in the product library, from the
device ISA (`make -C baseband_amd/csrc asm` -> build/bbdecode.s).  Prints one
line per kernel; exit status 1 if a kernel spills to scratch or a streaming
decode kernel needs more than 128 VGPRs (fewer than 4 waves per SIMD: the LDS
staged byte-table kernel lost 15 % of its rate at 164 VGPRs, profiles/r03m).
    python tools/check_isa.py [--build]
    python tools/check_isa.py [--build] --against OLD.s
With --against: one line per kernel, `same` or `differs`, from a comparison of its whole
instruction body in build/bbdecode.s with the one in OLD.s (an assembly file of an
earlier tree), beside the register, LDS and scratch figures of both; exit status 1 if a
kernel differs or is in one file only.
"""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


NEW = os.path.join(ROOT, 'build', 'bbdecode.s')


def bodies(s):
    """-> {kernel: its instructions}: comments, directives and blank lines dropped, local
    labels (.LBB<function>_<block>) named by block alone."""
    out = {}
    for m in re.finditer(r'^(\w+):[^\n]*\n(.*?)^\.Lfunc_end\d+:', s, re.S | re.M):
        lines = (re.sub(r'\.LBB\d+_', '.LBB_', ln.split(';')[0]).strip() for ln in m.group(2).splitlines())
        out[m.group(1)] = [ln for ln in lines if ln and (not ln.startswith('.') or ln.endswith(':'))]
    return out


def kernels(path=NEW):
    with open(path) as f:
        s = f.read()
    out = []
    code = bodies(s)
    for m in re.finditer(r'\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel', s, re.S):
        body = m.group(2)

        def field(name):
            return int(re.search(r'\.amdhsa_%s (\d+)' % name, body).group(1))
        out.append(dict(name=m.group(1), code=code[m.group(1)], vgpr=field('next_free_vgpr'), sgpr=field('next_free_sgpr'),
                        scratch=field('private_segment_fixed_size'), lds=field('group_segment_fixed_size')))
    return out


def demangle(names):
    try:
        r = subprocess.run(['c++filt'] + names, capture_output=True, text=True, timeout=60)
        return r.stdout.splitlines()
    except Exception:
        return names


def against(old_path):
    old, new = ({k['name']: k for k in kernels(p)} for p in (old_path, NEW))
    names = sorted(set(old) | set(new))
    ndiff = 0

    def figures(k):
        return "{:3d} VGPR {:3d} SGPR {:6d} B LDS {:3d} B scratch".format(k['vgpr'], k['sgpr'], k['lds'], k['scratch'])
    for n, shown in sorted(zip(names, demangle(names)), key=lambda x: x[1]):
        shown = re.sub(r'^void ', '', shown)[:90]
        if n not in old or n not in new:
            verdict, ndiff = 'only in ' + ('the old file' if n in old else 'the new file'), ndiff + 1
            print("{:8s} {}  {}".format('differs', shown, verdict))
            continue
        same = old[n]['code'] == new[n]['code']
        ndiff += not same
        print("{:8s} old {} | new {}  {}".format('same' if same else 'differs', figures(old[n]), figures(new[n]), shown))
    print("{} kernels, {} differ".format(len(names), ndiff))
    return 1 if ndiff else 0


def main():
    if '--build' in sys.argv:
        subprocess.check_call(['make', '-C', os.path.join(ROOT, 'baseband_amd', 'csrc'), 'asm'],
                              stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    if '--against' in sys.argv:
        return against(sys.argv[sys.argv.index('--against') + 1])
    ks = kernels()
    names = demangle([k['name'] for k in ks])
    bad = 0
    for k, n in sorted(zip(ks, names), key=lambda x: x[1]):
        n = re.sub(r'^void ', '', n).replace('(bb_flat_args)', '').replace('(bb_gather_args)', '')
        flag = ''
        if k['scratch']:
            flag, bad = ' <-- SCRATCH', bad + 1
        elif k['vgpr'] > 128 and 'k_decode' in n:
            flag, bad = ' <-- more than 128 VGPRs', bad + 1
        print("{:4d} VGPR {:4d} SGPR {:6d} B LDS {:4d} B scratch  {}{}".format(
            k['vgpr'], k['sgpr'], k['lds'], k['scratch'], n[:110], flag))
    print("{} kernels, {} flagged".format(len(ks), bad))
    return 1 if bad else 0


if __name__ == '__main__':
    sys.exit(main())
