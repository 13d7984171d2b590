"""Records tests/golden/conv_tail_parent.json: the SHA-256 of y and of the GroupNorm octet partials of every case of tests/conv_tail_common.py (the case
list of the conv-epilogue tests), computed on one MI355X.

  python tools/record_conv_tail_digests.py [--lib libpdhip.so] [out.json]      # default: the library built in the tree -> tests/golden/conv_tail_parent.json

Run it BEFORE a refactor of the conv kernels' tails (csrc/nn_conv_tail.h and the five units that include it) with the parent commit's library -- built
in a `git worktree` of that commit and named with --lib; tests/test_gpu_conv_tail_parent.py then holds the refactored library to these digests.  Every
case runs twice on one workspace; a case whose two launches differ is reported and left out (nothing can be held to it)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--lib', default=None, help="the parent commit's libpdhip.so")
    ap.add_argument('out', nargs='?', default=None)
    a = ap.parse_args()
    from pointdreamer_amd import _lib
    if a.lib:
        _lib.LIB_PATH = os.path.abspath(a.lib)
    import pointdreamer_amd.ddnm_inpainting  # noqa: F401  (registers the entry points)
    import conv_tail_common as ct
    L = _lib.lib()
    rec, dropped = {}, []
    for c in ct.CASES:
        first, second = ct.run_case(L, c)
        if first != second:
            dropped.append(c['name'])
            print(f"{c['name']}: two launches differ: left out", flush=True)
            continue
        rec[c['name']] = first
        print(f"{c['name']}: kernel {first['kernel']}, {first['chunks']} chunks", flush=True)
    out = a.out or ct.GOLDEN
    with open(out, 'w') as fh:
        json.dump(rec, fh, indent=1, sort_keys=True)
        fh.write('\n')
    print(f"{len(rec)} cases -> {out} (library {_lib.LIB_PATH}); dropped: {dropped}")
    return 1 if dropped else 0


if __name__ == '__main__':
    sys.exit(main())
