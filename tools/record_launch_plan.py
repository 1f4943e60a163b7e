#!/usr/bin/env python3
"""Record tests/golden/fav_launch_plan.json: what the library reports of every scenario of
tests/launch_plan_scenarios.py (launch counts per profiler name, batch work, fallback statistics, gather work).

The fixture pins the launch plan of each batch form against the library it was recorded from, so it is recorded
once, from the build a host-side change starts from, and never again from the changed code:

    python tools/record_launch_plan.py [OUT.json]

Needs an MI355X; refuses to write if any verdict differs from the construction."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "eth-consensus-specs_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main() -> int:
    import launch_plan_scenarios as S
    from bls_mi355x import _native, batch

    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "fav_launch_plan.json")
    ctx = _native.context()
    S.load_registry(batch, ctx)
    records = {}
    for name, run in S.scenarios().items():
        rec, out, expect = run(batch, ctx)
        if list(out) != list(expect):
            print("verdicts differ from the construction in", name, file=sys.stderr)
            return 1
        records[name] = rec
        print(name, json.dumps(rec, sort_keys=True))
    with open(out_path, "w") as fh:
        json.dump(records, fh, indent=1, sort_keys=True)
        fh.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
