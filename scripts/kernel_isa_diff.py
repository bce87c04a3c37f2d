#!/usr/bin/env python3
"""Kernel-by-kernel comparison of the gfx950 device code of two builds.

    python scripts/kernel_isa_diff.py OLD_LIB_DIR NEW_LIB_DIR [--rename OLD=NEW ...] [--require REGEX ...] [--out FILE]

Both directories hold the objects nsynth_wavenet_amd.build leaves in nsynth_wavenet_amd/lib (wn_*.o).  Every object is
disassembled with hazard_audit.disassemble_object; a kernel is its instruction text with addresses, encodings and symbol
references stripped.  Kernels are paired by name, whatever object they sit in and without their namespace and
parameter types (a kernel that moved to another translation unit, or whose argument struct left an anonymous namespace, is
still the same kernel); --rename pairs a kernel that changed its name on purpose; what is left on either side is paired
by identical instructions.  The report lists every kernel that differs or has no partner, with instruction counts, and the
number of identical ones per old object.  --require: kernels (regex on the old name) that must be identical; exit status 1
if one of them is not.
"""
import argparse, collections, glob, os, re, sys, tempfile, shutil

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nsynth_wavenet_amd import hazard_audit


def short_name(sym):
    """tg_gemm_kernel<Li0ELi2E> of _ZN12_GLOBAL__N_114tg_gemm_kernelILi0ELi2EEEvNS_6TgArgsE: the kernel's own name and its
    literal template arguments, without namespace and parameter types; any other symbol as it is."""
    m = re.match(r'_Z(?:N12_GLOBAL__N_1)?(\d+)', sym)
    if not m:
        return sym
    at = m.end()
    name, rest = sym[at:at + int(m.group(1))], sym[at + int(m.group(1)):]
    t = re.match(r'I((?:L[a-z]\d+E)+)E', rest)
    return name + ('<' + t.group(1) + '>' if t else '')


def kernels_of(lib_dir):
    """{short kernel name: [(object, [instruction, ...]), ...]} of every wn_*.o in lib_dir (measurement variants excluded)."""
    found = []
    for obj in sorted(glob.glob(os.path.join(lib_dir, 'wn_*.o'))):
        base = os.path.basename(obj)
        if '_x2_' in base or base.endswith('_v.o'):
            continue
        tmp = tempfile.mkdtemp(prefix='wn_isa_')
        try:
            listing = hazard_audit.disassemble_object(obj, tmp, allow_no_kernels=base.startswith('wn_host'))
            lines = open(listing).read().split('\n') if listing else []
        finally:
            shutil.rmtree(tmp, ignore_errors=True)
        cur = None
        for l in lines:
            m = re.match(r'^[0-9a-f]+ <(.+)>:$', l)
            if m:
                cur = (base, m.group(1), [])
                found.append(cur)
            elif cur and l.startswith('\t'):
                cur[2].append(re.sub(r'\s+', ' ', l.split('//')[0].strip()))
    for _, _, ins in found:                     # alignment filler behind the last s_endpgm
        while ins and not ins[-1].startswith('s_endpgm'):
            ins.pop()
    out = collections.OrderedDict()
    for base, n, ins in found:
        if ins:
            out.setdefault(short_name(n), []).append((base, ins))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('old')
    ap.add_argument('new')
    ap.add_argument('--rename', action='append', default=[], metavar='OLD=NEW')
    ap.add_argument('--require', action='append', default=[], metavar='REGEX')
    ap.add_argument('--out')
    a = ap.parse_args()
    old, new = kernels_of(a.old), kernels_of(a.new)
    rename = dict(r.split('=', 1) for r in a.rename)
    same = collections.Counter()
    differ, used_new = [], set()
    left_old = []
    for name, copies in old.items():
        partner = name if name in new else rename.get(name)
        if partner not in new:
            left_old += [(name, o, ins) for o, ins in copies]
            continue
        used_new.add(partner)
        for o, ins in copies:
            for o2, ins2 in new[partner]:
                if ins == ins2:
                    same[o] += 1
                else:
                    differ.append((name, o, len(ins), partner, o2, len(ins2)))
    left_new = [(n, o, ins) for n, c in new.items() if n not in used_new for o, ins in c]
    moved, removed = [], []
    for name, o, ins in left_old:
        hit = next((x for x in left_new if x[2] == ins), None)
        if hit:
            left_new.remove(hit)
            same[o] += 1
            moved.append((name, o, hit[0], hit[1]))
        else:
            removed.append((name, o, len(ins)))
    rep = ['kernel ISA comparison: old = {} kernels, new = {} kernels'.format(sum(map(len, old.values())), sum(map(len, new.values())))]
    rep += ['identical kernels per old object:'] + ['  %-22s %d' % kv for kv in sorted(same.items())]
    rep += ['identical under another name (%d):' % len(moved)] + ['  %s [%s] -> %s [%s]' % m for m in moved]
    rep += ['DIFFERENT (%d): old instructions -> new instructions' % len(differ)]
    rep += ['  %s [%s] %d -> %s [%s] %d' % d for d in differ]
    rep += ['only in old (%d):' % len(removed)] + ['  %s [%s] %d instructions' % r for r in removed]
    rep += ['only in new (%d):' % len(left_new)] + ['  %s [%s] %d instructions' % (n, o, len(i)) for n, o, i in left_new]
    bad = sorted({d[0] for d in differ} | {r[0] for r in removed})
    failed = [n for n in bad if any(re.search(rx, n) for rx in a.require)]
    missing = [rx for rx in a.require if not any(re.search(rx, n) for n in old)]
    rep.append('required identical (%s): %s' % (', '.join(a.require) or 'none',
                                              'FAILED: ' + ', '.join(failed + missing) if failed or missing else 'ok'))
    text = '\n'.join(rep) + '\n'
    sys.stdout.write(text)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(text)
    return 1 if failed or missing else 0


if __name__ == '__main__':
    sys.exit(main())
