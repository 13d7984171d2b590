"""Compares the device code of two builds of the same HIP units, kernel by kernel: what a refactor that must not change code generation is held to.

  python tools/kernel_codegen_diff.py BASE_CSRC HEAD_CSRC [-o table.txt] [unit.hip ...]

BASE_CSRC / HEAD_CSRC: two copies of pointdreamer_amd/csrc (the base usually from `git worktree add <dir> <commit>`).  Every unit (default: the five
conv units) is compiled to gfx950 assembly with the flags of the csrc/Makefile rule that builds it -- the nn_% rule, or the geometry rule (which adds
`-ffp-contract=off -mllvm -amdgpu-mfma-vgpr-form=1`) for a unit not named nn_* -- plus `--cuda-device-only -S`; no GPU is needed.  Per kernel
symbol the table holds the register counts, LDS and scratch sizes and spill count of the code object's metadata, the instruction count, and a verdict:

  identical   the instruction streams are equal once labels, comments and directive lines are stripped (branch targets compared by position)
  reordered   the same multiset of mnemonics, and equal counts: register numbering and / or scheduling order differ
  CHANGED     anything else -- such a kernel needs a timing; `d=` counts the instructions of either build without a partner of the same mnemonic in
              the other

Exit status 1 if any kernel is CHANGED or exists in one build only."""
import argparse
import collections
import concurrent.futures
import os
import re
import shutil
import subprocess
import sys
import tempfile

UNITS = ['nn_gemm.hip', 'nn_conv_halo.hip', 'nn_conv_ht.hip', 'nn_conv_sk.hip', 'nn_conv_rr.hip']
FLAGS = ['--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-Wall', '-Wno-unused-function', '--cuda-device-only', '-S']
GEO_FLAGS = ['-ffp-contract=off', '-mllvm', '-amdgpu-mfma-vgpr-form=1']          # what csrc/Makefile's rule for every unit not named nn_* adds
META = ('.vgpr_count', '.sgpr_count', '.group_segment_fixed_size', '.private_segment_fixed_size', '.vgpr_spill_count')
LABEL = re.compile(r'^([.\w$]+):')


def assemble(csrc, unit, out):
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    geo = [] if os.path.basename(unit).startswith('nn_') else GEO_FLAGS
    subprocess.run([hipcc] + FLAGS + geo + [unit, '-o', out], cwd=csrc, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE)
    return out


def parse(path):
    """{kernel symbol: dict(meta..., stream=[instruction text with branch targets as instruction positions])}"""
    lines = open(path).read().split('\n')
    meta, cur = {}, None
    for ln in lines[lines.index('amdhsa.kernels:') + 1:]:      # a YAML list: one `  - .key: value` block per kernel, its own keys indented by four
        if ln.startswith('  - .'):
            cur = {}
        m = re.match(r'^(?:  - |    )(\.\w+):\s+(\S+)$', ln)
        if m and cur is not None:
            cur[m.group(1)] = m.group(2)
            if m.group(1) == '.name':
                meta[m.group(2)] = cur
        if ln.startswith('amdhsa.target'):
            break
    kernels = {}
    i = 0
    while i < len(lines):
        m = re.match(r'\s*\.type\s+([.\w$]+),@function', lines[i])
        if not m or m.group(1) not in meta:
            i += 1
            continue
        name = m.group(1)
        while not lines[i].startswith(name + ':'):
            i += 1
        body, labels = [], {}
        i += 1
        while not re.match(r'\.Lfunc_end\d+:', lines[i]):
            ln = lines[i].split(';')[0].rstrip()
            i += 1
            lm = LABEL.match(ln)
            if lm:
                labels[lm.group(1)] = len(body)
            elif ln.strip() and not ln.strip().startswith('.'):
                body.append(' '.join(ln.split()))
        stream = [re.sub(r'\.L[\w$]+', lambda t: f"@{labels.get(t.group(0), '?')}", ins) for ins in body]
        kernels[name] = dict(meta[name], stream=stream)
    return kernels


def demangle(names):
    tool = shutil.which('llvm-cxxfilt') or shutil.which('c++filt')
    try:
        out = subprocess.run([tool], input='\n'.join(names), capture_output=True, text=True, check=True).stdout.split('\n')
        return dict(zip(names, out))
    except (TypeError, OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('base'); ap.add_argument('head'); ap.add_argument('units', nargs='*', default=UNITS)
    ap.add_argument('-o', '--out', default=None)
    ap.add_argument('-j', type=int, default=min(8, os.cpu_count() or 1))
    a = ap.parse_args()
    rows, bad = [], 0
    with tempfile.TemporaryDirectory() as tmp, concurrent.futures.ThreadPoolExecutor(a.j) as pool:
        jobs = {(side, u): pool.submit(assemble, os.path.abspath(root), u, os.path.join(tmp, f"{side}_{u}.s"))
                for side, root in (('base', a.base), ('head', a.head)) for u in a.units}
        for u in a.units:
            kb, kh = parse(jobs[('base', u)].result()), parse(jobs[('head', u)].result())
            nice = demangle(sorted(set(kb) | set(kh)))
            for name in sorted(set(kb) | set(kh), key=lambda n: nice[n]):
                b, h = kb.get(name), kh.get(name)
                if b is None or h is None:
                    rows.append(f"{u:18s} {'ONLY IN ' + ('head' if b is None else 'base'):10s} {nice[name]}")
                    bad += 1
                    continue
                same_meta = all(b.get(k) == h.get(k) for k in META)
                cb, ch = (collections.Counter(s.split()[0] for s in x['stream']) for x in (b, h))
                if b['stream'] == h['stream'] and same_meta:
                    verdict = 'identical'
                elif same_meta and cb == ch:
                    verdict = 'reordered'
                else:
                    verdict, bad = f"CHANGED d={sum(((cb - ch) + (ch - cb)).values())}", bad + 1
                cols = ' '.join(f"{b.get(k, '?')}/{h.get(k, '?')}".rjust(13) for k in META)
                rows.append(f"{u:18s} {verdict:13s} {cols} {len(b['stream']):6d}/{len(h['stream']):<6d} {nice[name]}")
    head = (f"# base/head per kernel: {' '.join(k[1:] for k in META)} instructions   (flags: {' '.join(FLAGS)}; units not named nn_*: + {' '.join(GEO_FLAGS)})\n"
            f"# {len(rows)} kernel instances, {bad} changed or unmatched")
    text = head + '\n' + '\n'.join(rows) + '\n'
    if a.out:
        with open(a.out, 'w') as fh:
            fh.write(text)
    sys.stdout.write(text if not a.out else head + '\n' + ''.join(r + '\n' for r in rows if ' identical ' not in r))
    return 1 if bad else 0


if __name__ == '__main__':
    sys.exit(main())
