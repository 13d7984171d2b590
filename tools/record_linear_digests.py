"""Records tests/golden/linear_parent.json: per case of tests/linear_parent_common.py and `local` mode the SHA-256 of `out`, of `tri` and of the
integers pdhip_linear_fill leaves in its workspace, with the integers themselves and where the queries ended, computed on one MI355X.

  python tools/record_linear_digests.py [--lib libpdhip.so] [out.json]      # default: the library built in the tree -> tests/golden/linear_parent.json

Run it BEFORE a refactor of csrc/linear.hip with the parent commit's library -- built in a `git worktree` of that commit and named with --lib;
tests/test_gpu_linear_parent.py then holds the refactored library to these digests.  Every case runs twice on one workspace; a case whose two
launches differ is reported and recorded with both (the test fails on it): fix the case list, do not drop the case."""
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
    import linear_parent_common as lp
    L = _lib.lib()
    rec, unstable = {}, []
    for name, local in lp.IDS:
        first, second = lp.run_case(L, _lib, name, local)
        key = f"{name}-local{local}"
        rec[key] = first
        if first != second:
            unstable.append(key)
            rec[key] = dict(first, second_launch=second)
            print(f"{key}: TWO LAUNCHES DIFFER", flush=True)
        print(f"{key}: " + ' '.join(f"{k}={v}" for k, v in first.items() if k not in ('out', 'tri', 'ints')), flush=True)
    out = a.out or lp.GOLDEN
    with open(out, 'w') as fh:
        json.dump(rec, fh, indent=1, sort_keys=True)
        fh.write('\n')
    print(f"{len(rec)} cases -> {out} (library {_lib.LIB_PATH}); unstable: {unstable}")
    return 1 if unstable else 0


if __name__ == '__main__':
    sys.exit(main())
