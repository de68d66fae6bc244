#!/usr/bin/env python3
"""Regenerate tests/golden/clahe_goldens.json from the reference's own test DATA (not source).

Run in the build container only (it reads /root/reference, which does not
exist on the GPU box):   python tests/golden/make_clahe_fixtures.py

Produces
  clahe_goldens.json  every key of the reference's tests/goldens/clahe.json (42: Gray,
                      YUV 4:2:0 / 4:4:4 and RGB at 8 and 16 bits, full / odd / tiny
                      geometries), per-plane {avg (normalised by peak), min, max}.
                      All inputs are reproducible from tests/fixtures.py
                      (tests/clahe_ref.py golden_inputs; RGB48 = RGB24 x 257).
Only data (expected numbers) is copied; no reference source text.
"""
import json
import sys
from pathlib import Path

REF = Path("/root/reference/tests")
OUT = Path(__file__).resolve().parent


def main() -> int:
    if not REF.is_dir():
        print("reference tree not present; fixtures are already committed", file=sys.stderr)
        return 1
    data = json.loads((REF / "goldens" / "clahe.json").read_text())
    (OUT / "clahe_goldens.json").write_text(json.dumps(data, indent=1, sort_keys=True) + "\n")
    print("wrote", OUT / "clahe_goldens.json", len(data), "keys")
    return 0


if __name__ == "__main__":
    sys.exit(main())
