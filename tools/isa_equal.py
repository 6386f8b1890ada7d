#!/usr/bin/env python3
"""Machine-code identity of two source trees, kernel by kernel.

  tools/isa_equal.py compile OUT [TU.hip ...] [--tree ROOT] [--jobs N] [--rtc DIR]
      compiles every translation unit of the Makefile's SRCS, plus device_math_probe.hip (or the ones named), of the
      tree ROOT (default: the tree this file lies in) to gfx950 device-only assembly OUT/<TU>.s, with the Makefile's own
      flags (make print-flags) plus --cuda-device-only -S, at most 16 compiles at a time.  --rtc DIR: also every DIR/*.hip,
      a source hipRTC compiled at run time as the test build kept it (MJHMC_RTC_KEEP, tools/rtc_sources.py), with the same
      flags against ROOT's headers, to OUT/rtc_<name>.s -- one DIR compiled against two trees compares their headers.
  tools/isa_equal.py compare A B [--allow REGEX]
      compares two such directories.  Per translation unit the sets of kernel names must be equal; per kernel (keyed by
      its mangled name: instantiation order follows include order, so a whole-file diff will not do) the instruction
      text and the .amdhsa_* descriptor block must be equal, after dropping .file / .ident / comment-only lines and the
      function's running number from its local labels.  Prints every kernel that differs; exit status 1 if any does.
      --allow REGEX (searched in the demangled name): such a kernel may differ as long as none of vgpr_count,
      sgpr_spill_count, vgpr_spill_count, private_segment_fixed_size, group_segment_fixed_size or its instruction count
      is higher in B than in A; the figures of both sides are printed.
"""
import argparse
import concurrent.futures
import os
import re
import subprocess
import sys

HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
FIGURES = ('vgpr_count', 'sgpr_spill_count', 'vgpr_spill_count', 'private_segment_fixed_size', 'group_segment_fixed_size')


def compile_tree(root, out, jobs, only, rtc=None):
    csrc = os.path.join(root, 'mjhmc_amd', 'csrc')
    flags = subprocess.check_output(['make', '-s', 'print-flags'], cwd=csrc, text=True).split()
    srcs = re.search(r'^SRCS\s*=\s*(.*)$', open(os.path.join(csrc, 'Makefile')).read(), flags=re.M).group(1).split()
    srcs = only or srcs + ['device_math_probe.hip']
    os.makedirs(out, exist_ok=True)

    kept = {f: os.path.join(os.path.abspath(rtc), f) for f in sorted(os.listdir(rtc)) if f.endswith('.hip')} if rtc else {}

    def one(tu):
        dst = os.path.join(os.path.abspath(out), ('rtc_' if tu in kept else '') + tu[:-4] + '.s')
        r = subprocess.run([HIPCC] + flags + ['--cuda-device-only', '-S', '-I', os.path.abspath(csrc), kept.get(tu, tu), '-o', dst], cwd=csrc,
                           stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True)
        return tu, r.returncode, r.stderr

    failed = 0
    # longest first: the energies' translation units bound the wall time
    srcs.sort(key=lambda tu: (not tu.startswith('energy_'), not tu.startswith('dense_')))
    srcs += list(kept)
    with concurrent.futures.ThreadPoolExecutor(max(1, min(jobs, 16))) as pool:
        for tu, rc, err in pool.map(one, srcs):
            print('%-28s %s' % (tu, 'ok' if rc == 0 else 'FAILED\n' + err), flush=True)
            failed += rc != 0
    return 1 if failed else 0


def clean(line):
    line = re.sub(r'\s*;.*$', '', line).rstrip()                     # trailing and whole-line comments
    return re.sub(r'\.L(BB|JTI|func_begin|func_end|tmp)\d+', r'.L\1', line)  # the function's running number


def kernels_of(path):
    """{mangled name: dict(text=[instruction lines], desc=[.amdhsa_* lines], figures...)} of one assembly file."""
    lines = open(path).read().split('\n')
    out, k = {}, 0
    while k < len(lines):
        m = re.match(r'\s*\.amdhsa_kernel\s+(\S+)', lines[k])
        if not m:
            k += 1
            continue
        name, desc = m.group(1), []
        k += 1
        while '.end_amdhsa_kernel' not in lines[k]:
            desc.append(clean(lines[k]).strip())
            k += 1
        out[name] = dict(desc=[d for d in desc if d])
    names = set(out)
    k = 0
    while k < len(lines):
        m = re.match(r'^(\w+):', lines[k])
        if not (m and m.group(1) in names):
            k += 1
            continue
        name, text = m.group(1), []
        k += 1
        while not re.match(r'^\.Lfunc_end\d+:', lines[k]):
            c = clean(lines[k])
            if c.strip() and not re.match(r'\s*\.(file|ident|loc|cfi_)', c):
                text.append(c.strip())
            k += 1
        out[name]['text'] = text
        out[name]['instructions'] = sum(bool(re.match(r'[a-z]', t)) for t in text)
    meta = '\n'.join(lines).split('amdhsa.kernels:')[-1]
    for entry in re.split(r'^  - (?=\.)', meta, flags=re.M)[1:]:
        m = re.search(r'^\s+\.name:\s+(\S+)', entry, flags=re.M)
        if m and m.group(1) in out:
            for f in FIGURES:
                v = re.search(r'^\s+\.%s:\s+(\d+)' % f, entry, flags=re.M)
                out[m.group(1)][f] = int(v.group(1)) if v else 0
    return out


def demangle(names):
    if not names:
        return {}
    try:
        r = subprocess.run(['c++filt'], input='\n'.join(names), capture_output=True, text=True, check=True)
        return dict(zip(names, r.stdout.split('\n')))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def compare(a, b, allow):
    tus = sorted(set(f for d in (a, b) for f in os.listdir(d) if f.endswith('.s')))
    bad = total = allowed = 0
    for tu in tus:
        pa, pb = os.path.join(a, tu), os.path.join(b, tu)
        if not (os.path.exists(pa) and os.path.exists(pb)):
            print('%s: only in %s' % (tu, a if os.path.exists(pa) else b))
            bad += 1
            continue
        ka, kb = kernels_of(pa), kernels_of(pb)
        total += len(ka)
        for n in sorted(set(ka) ^ set(kb)):
            print('%s: kernel %s only in %s' % (tu, n, a if n in ka else b))
            bad += 1
        differ = [n for n in sorted(set(ka) & set(kb)) if ka[n]['text'] != kb[n]['text'] or ka[n]['desc'] != kb[n]['desc']]
        pretty = demangle(differ)
        for n in differ:
            keys = FIGURES + ('instructions',)
            fig = '  '.join('%s %d -> %d' % (f, ka[n][f], kb[n][f]) for f in keys)
            ok = allow and re.search(allow, pretty[n]) and all(kb[n][f] <= ka[n][f] for f in keys)
            print('%s: %s %s\n    %s\n    %s' % (tu, 'differs (allowed)' if ok else 'DIFFERS', n, pretty[n], fig))
            allowed += bool(ok)
            bad += not ok
    print('isa_equal: %d translation units, %d kernels, %d differ as allowed: %s'
          % (len(tus), total, allowed, 'FAILED: %d' % bad if bad else 'ok'))
    return 1 if bad else 0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest='cmd', required=True)
    c = sub.add_parser('compile')
    c.add_argument('out')
    c.add_argument('--tree', default=os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
    c.add_argument('--jobs', type=int, default=min(16, os.cpu_count() or 1))
    c.add_argument('--rtc')
    c.add_argument('tus', nargs='*')
    d = sub.add_parser('compare')
    d.add_argument('a')
    d.add_argument('b')
    d.add_argument('--allow')
    args = ap.parse_args()
    if args.cmd == 'compile':
        return compile_tree(args.tree, args.out, args.jobs, args.tus, args.rtc)
    return compare(args.a, args.b, args.allow)


if __name__ == '__main__':
    sys.exit(main())
