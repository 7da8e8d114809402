#!/usr/bin/env python3
"""Compare the gfx950 machine code of two builds of a library, kernel by kernel.

    tools/kernel_isa_diff.py OLD.so NEW.so [--only REGEX]

For a change that only moves kernels between translation units (or is otherwise meant to leave code generation alone): build the
library before and after, and run this on the two.  Kernels are keyed by their mangled symbol across ALL code objects of a
library, so a kernel may change its translation unit (the copies of a kernel with internal linkage, one per translation unit
that uses it, are compared as a sorted list).  Per kernel it compares
  (a) the instruction list (llvm-objdump -d with addresses and encoding comments stripped; the s_nop / s_code_end / `...` filler
      behind a kernel's last instruction is ignored: how much of it there is depends on what follows in the code object), and
  (b) the resource fields of its metadata note (llvm-readelf --notes): registers, scratch, LDS, kernarg size, workgroup size.
Every difference is printed, kernels present on one side only are listed, and the exit status is non-zero if there is any.
The code objects are extracted as tests/test_isa_cpu.py does it."""
import argparse
import difflib
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get('LLVM_BIN', '/opt/rocm/lib/llvm/bin')
TARGET = 'hipv4-amdgcn-amd-amdhsa--gfx950'
FIELDS = ('.vgpr_count', '.sgpr_count', '.agpr_count', '.private_segment_fixed_size', '.group_segment_fixed_size',
          '.kernarg_segment_size', '.max_flat_workgroup_size')
FILLER = re.compile(r'^(s_nop 0|s_code_end|\.\.\.)$')


def code_objects(lib, tmp):
    fat = os.path.join(tmp, 'fat.bin')
    subprocess.check_call(['objcopy', '-O', 'binary', '--only-section=.hip_fatbin', lib, fat])
    data = open(fat, 'rb').read()
    offs = [m.start() for m in re.finditer(b'__CLANG_OFFLOAD_BUNDLE__', data)]
    if not offs:
        sys.exit('%s: no offload bundle' % lib)
    out = []
    for i, o in enumerate(offs):
        end = offs[i + 1] if i + 1 < len(offs) else len(data)
        b, co = os.path.join(tmp, 'm%d.bin' % i), os.path.join(tmp, 'm%d.co' % i)
        open(b, 'wb').write(data[o:end])
        subprocess.check_call([LLVM + '/clang-offload-bundler', '--unbundle', '--type=o', '--input=' + b, '--targets=' + TARGET,
                               '--output=' + co])
        out.append(co)
    return out


def kernels_of(lib):
    """{kernel symbol: sorted list of (instruction list, field values)} over every code object of lib.  The list has one entry
    per code object that defines the symbol: a kernel with internal linkage (a header's `static __global__`) exists once in
    every translation unit that uses it, under the same name."""
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for co in code_objects(lib, tmp):
            code, symbol = {}, None
            for ln in subprocess.run([LLVM + '/llvm-objdump', '-d', co], capture_output=True, text=True, check=True).stdout.split('\n'):
                m = re.match(r'^[0-9a-f]+ <(\S+)>:', ln)
                if m:
                    symbol = m.group(1)
                    code[symbol] = []
                    continue
                ins = ln.split('//')[0].strip()
                if ins and symbol:
                    code[symbol].append(ins)
            notes = subprocess.run([LLVM + '/llvm-readelf', '--notes', co], capture_output=True, text=True, check=True).stdout
            # amdhsa.kernels is a YAML list whose entries start at "  - .field:"; a kernel's own fields are indented by four
            # (those of its arguments by eight)
            for entry in re.split(r'\n  - (?=\.)', notes)[1:]:
                kv = dict(re.findall(r'^    (\.\w+):\s*(\S+)\s*$', '    ' + entry, re.M))
                name = kv['.name']
                ins = code[name]
                while ins and FILLER.match(ins[-1]):
                    ins.pop()
                out.setdefault(name, []).append((ins, tuple(kv[f] for f in FIELDS)))
    for copies in out.values():
        copies.sort()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('old')
    ap.add_argument('new')
    ap.add_argument('--only', metavar='REGEX', help='compare only kernels whose mangled symbol matches')
    args = ap.parse_args()
    keep = re.compile(args.only) if args.only else None
    old, new = ({k: v for k, v in kernels_of(lib).items() if not keep or keep.search(k)} for lib in (args.old, args.new))
    only_old, only_new = sorted(set(old) - set(new)), sorted(set(new) - set(old))
    for k in only_old:
        print('only in %s: %s' % (args.old, k))
    for k in only_new:
        print('only in %s: %s' % (args.new, k))
    n_code = n_meta = 0
    for k in sorted(set(old) & set(new)):
        if len(old[k]) != len(new[k]):
            n_code += 1
            print('%s: defined in %d code objects -> in %d' % (k, len(old[k]), len(new[k])))
            continue
        for (oi, of), (ni, nf) in zip(old[k], new[k]):
            if of != nf:
                n_meta += 1
                for f, a, b in zip(FIELDS, of, nf):
                    if a != b:
                        print('%s: %s %s -> %s' % (k, f, a, b))
            if oi != ni:
                n_code += 1
                print('%s: instructions differ (%d -> %d)' % (k, len(oi), len(ni)))
                for ln in list(difflib.unified_diff(oi, ni, 'old', 'new', lineterm='', n=2))[:60]:
                    print('    ' + ln)
    common = sum(min(len(old[k]), len(new[k])) for k in set(old) & set(new))
    print('kernel_isa_diff: %d kernels in both, %d only old, %d only new, %d with different instructions, %d with different '
          'descriptor fields' % (common, len(only_old), len(only_new), n_code, n_meta))
    if common == 0:
        print('kernel_isa_diff: nothing compared')
    return 1 if (only_old or only_new or n_code or n_meta or common == 0) else 0


if __name__ == '__main__':
    sys.exit(main())
