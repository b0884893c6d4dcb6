#!/usr/bin/env python3
"""Rewrite tests/conv2d_routes.json from the built library (tests/route_cases.py describes the table).

    python tools/conv2d_routes.py            # rewrite the table
    python tools/conv2d_routes.py --check    # only say what would change

Needs a GPU (creating a layer uploads its weights; the query itself does no device work). Refuses to write when a
reported name is not a conv2d_* kernel of tests/isa_pins.json: the library and the pins are then out of step, and the
table would record a kernel whose instruction stream nothing pins.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--check", action="store_true", help="do not write; exit 1 when the table is out of date")
    args = ap.parse_args()
    from damvsnet_amd import build, _capi
    build.build()
    _capi.load_library()
    import route_cases as R
    table = R.current_routes()
    pinned = set(R.pinned_conv2d_names())
    unknown = sorted({n for part in table.values() for n in part.values()} - pinned)
    if unknown:
        print("not written: the library reports kernels that tests/isa_pins.json does not pin:", file=sys.stderr)
        for n in unknown:
            print("  " + n, file=sys.stderr)
        return 2
    old = R.load() if os.path.exists(R.TABLE) else {}
    changed = [(part, k) for part in table for k in sorted(set(table[part]) | set(old.get(part, {})))
               if table[part].get(k) != old.get(part, {}).get(k)]
    for part, k in changed:
        print("%s %s: %s -> %s" % (part, k, old.get(part, {}).get(k), table[part].get(k)))
    print("%d entries, %d changed" % (sum(len(p) for p in table.values()), len(changed)))
    if args.check:
        return 1 if changed else 0
    with open(R.TABLE, "w") as f:
        json.dump(table, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
