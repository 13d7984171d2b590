#!/usr/bin/env python3
"""tests/golden/unet_route_table_hooks.txt: the production UNet's route table (pdhip_unet_route_table: host only, no device needed) under every
routing / fold hook flipped alone to each of its documented non-default values, at batch 1, 2, 8, 32 -- one line per (setting, batch):

    <setting> N=<batch> rows=<lines of the table> sha256=<of the table's text>

(the full tables come to ~1 MB).  The settings and the digest live in tests/nn_hooks_common.py, which tests/test_abi.py checks the file with.

    python tools/gen_route_table_hooks.py                      write the golden from the library as built
    python tools/gen_route_table_hooks.py --show conv_sk=2,3,2 --batch 8      print that setting's full table instead
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]
import nn_hooks_common as nh  # noqa: E402

GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'unet_route_table_hooks.txt')


def golden_text():
    out = []
    for label, setter, args in [('default', None, ())] + nh.ROUTE_SETTINGS:
        for N in nh.ROUTE_BATCHES:
            rows, sha = nh.route_table_digest(nh.route_table_lines(label, setter, args, N))
            out.append(f"{label} N={N} rows={rows} sha256={sha}\n")
    return ''.join(out)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--show', metavar='SETTING', help="print the full table of one setting ('default' or a label of the golden)")
    ap.add_argument('--batch', type=int, default=1)
    ap.add_argument('--out', default=GOLDEN)
    a = ap.parse_args()
    if a.show:
        known = {'default': (None, ())}
        known.update({label: (setter, args) for label, setter, args in nh.ROUTE_SETTINGS})
        if a.show not in known:
            sys.exit(f"unknown setting {a.show!r}; one of: {' '.join(known)}")
        print('\n'.join(nh.route_table_lines(a.show, *known[a.show], a.batch)))
        return
    with open(a.out, 'w') as f:
        f.write(golden_text())
    print(f"wrote {a.out}")


if __name__ == '__main__':
    main()
