"""Are the kernels of one device assembly file unchanged in another?   python scripts/compare_kernel_asm.py OLD.s NEW.s

Both files come from `hipcc <the unit's flags> -S --cuda-device-only unit.hip`.  Every function of OLD must exist in NEW with the same
instructions (comments, debug directives and local label numbers aside); functions only NEW has are counted.  Exit status 1 on a difference."""
import re
import subprocess
import sys


def funcs(path):
    out, cur = {}, None
    for line in open(path):
        m = re.match(r'^(_Z\w+):', line)
        if m:
            cur = out.setdefault(m.group(1), [])
            continue
        if cur is None:
            continue
        if line.startswith('.Lfunc_end'):
            cur = None
        elif not re.match(r'\s*(;|\.loc|\.file|\.cfi)', line):
            cur.append(re.sub(r'\.L(BB|tmp|func_\w+)?\d+_\d+', 'L', line.split(';')[0].rstrip()))
    return out


def main():
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
