#!/usr/bin/env python3
"""Regenerate tests/golden/combmask_goldens.json from the reference's own test DATA (not source).

Needs a checkout of the reference project (not needed to run the tests: the fixture is committed):
    python tests/golden/make_combmask_fixtures.py REFERENCE_CHECKOUT

Produces
  combmask_goldens.json  every key of the reference's tests/goldens/combmask.json (39: 21 CombMask
                         keys read at frame 1 of the temporal clip, 18 CombMaskMT keys; GRAY8 full /
                         odd / tiny, YUV420P8 and YUV444P8 full), per-plane {avg (normalised by
                         peak), min, max}. All inputs are reproducible from tests/fixtures.py
                         (tests/combmask_ref.py golden_inputs).
Only data (expected numbers) is copied; no reference source text.
"""
import json
import sys
from pathlib import Path

OUT = Path(__file__).resolve().parent


def main() -> int:
    if len(sys.argv) != 2 or not (Path(sys.argv[1]) / "tests" / "goldens" / "combmask.json").is_file():
        print("usage: make_combmask_fixtures.py REFERENCE_CHECKOUT (the fixture is already committed)", file=sys.stderr)
        return 1
    data = json.loads((Path(sys.argv[1]) / "tests" / "goldens" / "combmask.json").read_text())
    (OUT / "combmask_goldens.json").write_text(json.dumps(data, indent=1, sort_keys=True) + "\n")
    print("wrote", OUT / "combmask_goldens.json", len(data), "keys")
    return 0


if __name__ == "__main__":
    sys.exit(main())
