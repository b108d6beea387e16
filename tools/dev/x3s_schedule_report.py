#!/usr/bin/env python3
"""What the compiler made of conv3x3_halo_x3s_kernel's schedule (host only: no GPU, not a test).

Compiles csrc/keep_conv_x3s.hip with the command line `make -n` prints for keep_conv_x3s.o (device side only, to assembly, with the
resource remarks) and prints, per instantiation of the streaming kernel:
  * VGPRs and scratch bytes per lane from -Rpass-analysis=kernel-resource-usage;
  * the two step bodies (a run of v_mfma lines less than GAP instructions apart with as many MFMAs as a step has: 108, single-fp16
    form 36) with their instruction counts, and the instruction count of the code in front of, between and behind them;
  * every `s_waitcnt` that carries a vmcnt, with its operand and its place relative to the MFMAs.
It looks for v_mfma and s_waitcnt lines only; every other instruction is merely counted.

  python tools/dev/x3s_schedule_report.py [--asm FILE --remarks FILE] [--label TEXT]
(--asm / --remarks: report on an existing `hipcc -S` dump and its remark log instead of compiling.)
"""
import argparse
import os
import re
import shlex
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
CSRC = os.path.join(ROOT, 'comfyui-keep_amd', 'csrc')
KERNELS = ('conv3x3_halo_x3s_kernel', 'conv3x3_halo_x3s_act_kernel')      # <PRO, AFF, X1> and <PRO, AFF, X1, EACT>: one body
GAP = 60                 # two MFMAs further apart than this belong to different runs (a step body has ~5 instructions per MFMA gap)


def compile_asm(workdir):
    """The Makefile's own command for keep_conv_x3s.o, turned into a device-only -S compile with resource remarks."""
    out = subprocess.check_output(['make', '-C', CSRC, '-n', '-B', 'keep_conv_x3s.o'], text=True)
    line = next(l for l in out.splitlines() if 'keep_conv_x3s.hip' in l and ' -c ' in l)
    argv = shlex.split(line)
    asm, remarks = os.path.join(workdir, 'keep_conv_x3s.s'), os.path.join(workdir, 'remarks.txt')
    argv[argv.index('-o') + 1] = asm
    argv[argv.index('-c')] = '-S'
    argv += ['--cuda-device-only', '-Rpass-analysis=kernel-resource-usage']
    print('# ' + ' '.join(a if a != asm else 'keep_conv_x3s.s' for a in argv))
    with open(remarks, 'w') as f:
        subprocess.check_call(argv, cwd=CSRC, stderr=f)
    return asm, remarks


def read_remarks(path):
    """{mangled name: {'VGPRs': n, 'ScratchSize [bytes/lane]': n, ...}}"""
    res, cur = {}, None
    for line in open(path):
        m = re.search(r'remark:\s+Function Name: (\S+)', line)
        if m:
            cur = res.setdefault(m.group(1), {})
            continue
        m = re.search(r'remark:\s+([A-Za-z][^:]*): (\S+) \[-Rpass', line)
        if m and cur is not None:
            cur[m.group(1).strip()] = m.group(2)
    return res


def functions(path):
    """(mangled name, [instruction lines]) per function of the dump; an instruction is a tab-indented line that is no directive."""
    name, ins = None, []
    for line in open(path):
        if name is None:
            m = re.match(r'^(_Z\w+):', line)
            if m:
                name, ins = m.group(1), []
            continue
        if line.startswith('.Lfunc_end'):
            yield name, ins
            name = None
            continue
        s = line.strip()
        if line[:1] in '\t ' and s and s[0] not in '.;' and not s.endswith(':'):
            ins.append(s.split(';')[0].strip())


def demangle(names):
    for tool in ('/opt/rocm/llvm/bin/llvm-cxxfilt', 'c++filt'):
        try:
            out = subprocess.check_output([tool] + list(names), text=True).splitlines()
            return {n: re.sub(r'^void |\(.*$', '', o) for n, o in zip(names, out)}
        except (OSError, subprocess.CalledProcessError):
            continue
    return {n: n for n in names}


def report(name, shown, ins, rem):
    mf = [i for i, s in enumerate(ins) if s.startswith('v_mfma')]
    runs = []
    for i in mf:
        if runs and i - runs[-1][-1] <= GAP:
            runs[-1].append(i)
        else:
            runs.append([i])
    # the third template argument is the single-fp16 form (<PRO, AFF, X1[, EACT]>; the parent's x3 forms print two): 36 MFMAs per step instead of 108
    args = re.search(r'<(.*)>', shown).group(1).split(', ')
    per_step = 36 if len(args) > 2 and args[2] == 'true' else 108
    bodies = [r for r in runs if len(r) == per_step]
    print(f'{shown}')
    print(f'    VGPRs {rem.get("VGPRs", "?")}  scratch {rem.get("ScratchSize [bytes/lane]", "?")} B/lane  VGPR spills {rem.get("VGPRs Spill", "?")}  '
          f'SGPR spills {rem.get("SGPRs Spill", "?")}  occupancy {rem.get("Occupancy [waves/SIMD]", "?")} waves/SIMD  instructions {len(ins)}  MFMAs {len(mf)}')
    if not bodies:
        print(f'    no run of {per_step} MFMAs found (runs: {[len(r) for r in runs]})')
        return
    parts = []
    for k, b in enumerate(bodies):
        parts.append(f'body {k}: {b[-1] - b[0] + 1}')
    outside = [bodies[0][0]] + [bodies[k + 1][0] - bodies[k][-1] - 1 for k in range(len(bodies) - 1)] + [len(ins) - bodies[-1][-1] - 1]
    print(f'    step bodies ({per_step} MFMAs each, first to last MFMA): ' + ', '.join(parts))
    print(f'    code outside them: in front of body 0: {outside[0]}' + ''.join(f', between body {k} and {k + 1}: {outside[k + 1]}' for k in range(len(bodies) - 1)) +
          f', behind body {len(bodies) - 1}: {outside[-1]}')
    other = [len(r) for r in runs if len(r) != per_step]
    if other:
        print(f'    other MFMA runs (the prologue-less tails of the pipeline): {other}')
    # waits
    rows = []
    for i, s in enumerate(ins):
        if not s.startswith('s_waitcnt'):
            continue
        m = re.search(r'vmcnt\((\d+)\)', s)
        if not m:
            continue
        where = None
        for k, b in enumerate(bodies):
            if b[0] < i < b[-1]:
                done = sum(1 for j in b if j < i)
                where = f'body {k}, behind MFMA {done} of {per_step}'
            elif i < b[0] and (k == 0 or i > bodies[k - 1][-1]):
                where = f'{b[0] - i} instructions in front of body {k}' + (f' ({i - bodies[k - 1][-1]} behind body {k - 1})' if k else '')
        if where is None:
            where = f'{i - bodies[-1][-1]} instructions behind body {len(bodies) - 1}'
        rows.append((int(m.group(1)), where))
    inside = [(n, w) for n, w in rows if w.startswith('body')]
    near = [(n, w) for n, w in rows if not w.startswith('body')]
    print(f'    vmcnt waits inside the bodies ({len(inside)}):')
    for n, w in inside:
        print(f'        vmcnt({n})  {w}')
    zeros = sum(1 for n, _ in near if n == 0)
    print(f'    vmcnt waits outside the bodies: {len(near)}, of them vmcnt(0): {zeros}; the last one in front of each body and the first behind it:')
    for k, b in enumerate(bodies):
        before = [(n, w) for (n, w) in near if w.endswith(f'in front of body {k}') or f'in front of body {k} ' in w]
        if before:
            print(f'        vmcnt({before[-1][0]})  {before[-1][1]}')
    tail = [(n, w) for n, w in near if 'behind body %d' % (len(bodies) - 1) in w and 'front' not in w]
    if tail:
        print(f'        vmcnt({tail[0][0]})  {tail[0][1]}')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--asm')
    ap.add_argument('--remarks')
    ap.add_argument('--label', default='')
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        asm, remarks = (a.asm, a.remarks) if a.asm else compile_asm(tmp)
        rem = read_remarks(remarks) if remarks else {}
        fns = [(n, ins) for n, ins in functions(asm) if any(k in n for k in KERNELS)]
        names = demangle([n for n, _ in fns])
        if a.label:
            print(f'== {a.label}')
        for n, ins in sorted(fns, key=lambda t: names[t[0]]):
            report(n, names[n], ins, rem.get(n, {}))
    return 0


if __name__ == '__main__':
    sys.exit(main())
