#!/usr/bin/env python3
"""Regenerate tests/golden/checkmate_goldens.json from the reference's own test DATA (not source).

Needs a checkout of the reference project (not needed to run the tests: the fixture is committed):
    python tests/golden/make_checkmate_fixtures.py REFERENCE_CHECKOUT

Produces
  checkmate_goldens.json  every key of the reference's tests/goldens/checkmate.json (25 keys, 39
                          planes: GRAY8 full / odd / tiny, RGB24, YUV420P8, YUV422P8 and YUV444P8
                          full; each read at frame 1 of the 3-frame temporal clip), per-plane
                          {avg (normalised by peak), min, max}. All inputs are reproducible from
                          tests/fixtures.py (tests/checkmate_ref.py golden_inputs).
Only data (expected numbers) is copied; no reference source text.
"""
import json
import sys
from pathlib import Path

OUT = Path(__file__).resolve().parent


def main() -> int:
    if len(sys.argv) != 2 or not (Path(sys.argv[1]) / "tests" / "goldens" / "checkmate.json").is_file():
        print("usage: make_checkmate_fixtures.py REFERENCE_CHECKOUT (the fixture is already committed)", file=sys.stderr)
        return 1
    data = json.loads((Path(sys.argv[1]) / "tests" / "goldens" / "checkmate.json").read_text())
    (OUT / "checkmate_goldens.json").write_text(json.dumps(data, indent=1, sort_keys=True) + "\n")
    print("wrote", OUT / "checkmate_goldens.json", len(data), "keys")
    return 0


if __name__ == "__main__":
    sys.exit(main())
