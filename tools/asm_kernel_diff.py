"""Compare the kernels of two AMDGPU device-assembly files (hipcc --cuda-device-only -S), body by body.

    python tools/asm_kernel_diff.py parent/gemm_glds.s new/gemm_glds.s

For a refactor that must not change device code: each file is split into per-function bodies, a body is
keyed by the `.amdhsa_kernel` symbol it holds, and the bodies of the kernels both files have are compared
as text. Before the comparison, comments and the `.loc` / `.file` / `.ident` / `__hip_cuid_` lines are
dropped, and the function-index part of local labels (`.LBB<n>_<m>`, `.Lfunc_end<n>`, ...) is normalised,
since those renumber when a kernel ahead of them appears or disappears.

Prints the kernels only in A, the kernels only in B and the common kernels whose bodies differ (with a
short unified diff each); exits 1 if any common body differs, else 0. Host only; it compares text and
knows nothing about what the instructions are."""
import argparse
import difflib
import re
import sys

BEGIN = re.compile(r';\s*-- Begin function ')
END_OF_FUNCTIONS = re.compile(r'^\s*(\.section\s+\.AMDGPU\.gpr_maximums|\.amdgpu_metadata)')
KERNEL = re.compile(r'^\s*\.amdhsa_kernel\s+(\S+)')
DROPPED = re.compile(r'^\s*\.(loc|file|ident)\s|__hip_cuid_')
LOCAL_LABEL = re.compile(r'\.L(BB|JTI|CPI|func_begin|func_end)\d+')


def clean(line):
    """The line as compared: no comment, no trailing blanks, local labels without their function index;
    '' for a line that is not compared at all."""
    if DROPPED.search(line):
        return ''
    line = line.split(';', 1)[0].rstrip()
    return LOCAL_LABEL.sub(r'.L\1#', line)


def kernels(path):
    """{kernel symbol: [cleaned lines of its function body]}"""
    with open(path) as f:
        lines = f.read().split('\n')
    starts = []
    end = len(lines)
    for i, line in enumerate(lines):
        if BEGIN.search(line):
            # the function's own `.section .text.<symbol>` line, where it has one, belongs to it
            starts.append(i - 1 if i and lines[i - 1].lstrip().startswith('.section') else i)
        elif END_OF_FUNCTIONS.match(line):
            end = i
            break
    out = {}
    for a, b in zip(starts, starts[1:] + [end]):
        body = [c for c in map(clean, lines[a:b]) if c]
        names = [m.group(1) for m in map(KERNEL.match, body) if m]
        if len(names) == 1:  # (a device function that is no kernel has none)
            out[names[0]] = body
        elif names:
            raise SystemExit(f'{path}: one function body with {len(names)} kernel descriptors: {names}')
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('a')
    ap.add_argument('b')
    ap.add_argument('--diff-lines', type=int, default=20, help='lines of unified diff shown per differing kernel')
    args = ap.parse_args()
    ka, kb = kernels(args.a), kernels(args.b)
    only_a = sorted(set(ka) - set(kb))
    only_b = sorted(set(kb) - set(ka))
    differ = sorted(k for k in set(ka) & set(kb) if ka[k] != kb[k])
    print(f'A: {len(ka)} kernels ({args.a})')
    print(f'B: {len(kb)} kernels ({args.b})')
    for title, names in ((f'only in A: {len(only_a)}', only_a), (f'only in B: {len(only_b)}', only_b)):
        print(title)
        for k in names:
            print('  ' + k)
    print(f'in both: {len(set(ka) & set(kb))}, bodies that differ: {len(differ)}')
    for k in differ:
        print('  ' + k)
        d = list(difflib.unified_diff(ka[k], kb[k], 'A', 'B', lineterm='', n=1))
        for line in d[:args.diff_lines]:
            print('    ' + line)
        if len(d) > args.diff_lines:
            print(f'    ... ({len(d) - args.diff_lines} more diff lines)')
    return 1 if differ else 0


if __name__ == '__main__':
    sys.exit(main())
