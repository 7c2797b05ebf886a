"""Are the kernels of one device assembly file unchanged in another?   python scripts/compare_kernel_asm.py [--by-body [--allow-new]] OLD.s NEW.s

Both files come from `hipcc <the unit's flags> -S --cuda-device-only unit.hip`.  Every function of OLD must exist in NEW with the same
instructions (comments, debug directives and local label numbers aside); functions only NEW has are counted.  Exit status 1 on a difference.
--by-body: for a change that renames kernels.  Names are ignored (a function's own name inside its body too): the bodies of OLD and of NEW
must be equal as multisets, and so must the resource figures of their "Kernel info" blocks (registers, scratch, LDS, occupancy).
--allow-new: with --by-body, for a change that renames kernels AND adds some: bodies and resource lines that only NEW has are listed and
counted, and only those of OLD without an equal in NEW are a difference."""
import collections
import re
import subprocess
import sys

RESOURCES = ('TotalNumSgprs', 'NumVgprs', 'NumAgprs', 'ScratchSize', 'LDSByteSize', 'Occupancy')


def funcs(path, resources=None):
    out, cur, name = {}, None, None
    for line in open(path):
        m = re.match(r'^(_Z\w+):', line)
        if m:
            name = m.group(1)
            cur = out.setdefault(name, [])
            continue
        m = re.match(r';\s*(\w+)\s*[:=]\s*(\d+)', line)
        if m and resources is not None and name and cur is None and m.group(1) in RESOURCES:  # (the Kernel-info block behind a body)
            resources.setdefault(name, []).append(m.group(1) + '=' + m.group(2))
        if cur is None:
            continue
        if line.startswith('.Lfunc_end'):
            cur = None
        elif not re.match(r'\s*(;|\.loc|\.file|\.cfi)', line):
            cur.append(re.sub(r'\.L(BB|tmp|func_\w+)?\d+_\d+', 'L', line.split(';')[0].rstrip()))
    return out


def by_body(old_path, new_path, allow_new=False):
    bad, files = 0, []
    for path in (old_path, new_path):
        res = {}
        fs = funcs(path, res)
        files.append({'bodies': {k: '\n'.join(l.replace(k, 'SELF') for l in v) for k, v in fs.items()},
                      'resources': {k: ' '.join(res.get(k, [])) for k in fs}})
    for what in ('bodies', 'resources'):
        old, new = (collections.Counter(f[what].values()) for f in files)
        gone, come = old - new, new - old
        bad += sum(gone.values()) + (0 if allow_new else sum(come.values()))
        print(f'{old_path} -> {new_path}, by body: {sum(old.values())} and {sum(new.values())} kernels, {len(old)} and {len(new)} '
              f'distinct {what}; {sum(gone.values())} of the first file have no equal in the second, {sum(come.values())} of the second none in the first')
        for label, side, f in (('only in the first file: ', gone, files[0]), ('only in the second file:', come, files[1])):
            names = sorted(k for k, v in f[what].items() if v in side)
            dem = subprocess.run(['c++filt'], input='\n'.join(names), capture_output=True, text=True).stdout.split('\n') if names else []
            for k, d in zip(names, dem):
                print(f'  {label} {d.split("(")[0]}' + (f'  [{f[what][k]}]' if what == 'resources' else ''))
    return 1 if bad else 0


def main():
    if len(sys.argv) == 4 and sys.argv[1] == '--by-body':
        return by_body(sys.argv[2], sys.argv[3])
    if len(sys.argv) == 5 and sys.argv[1:3] == ['--by-body', '--allow-new']:
        return by_body(sys.argv[3], sys.argv[4], True)
    if len(sys.argv) != 3:
        print(__doc__)
        return 2
    old, new = funcs(sys.argv[1]), funcs(sys.argv[2])
    bad = [k for k in sorted(old) if old[k] != new.get(k)]
    if bad:
        for d in subprocess.run(['c++filt'], input='\n'.join(bad), capture_output=True, text=True).stdout.split('\n'):
            print('DIFFERS or MISSING:', d)
    print(f'{sys.argv[1]} -> {sys.argv[2]}: {len(old) - len(bad)} of {len(old)} kernels identical instruction for instruction, '
          f'{len(bad)} differ, {len([k for k in new if k not in old])} only in the second file')
    return 1 if bad else 0


if __name__ == '__main__':
    sys.exit(main())
