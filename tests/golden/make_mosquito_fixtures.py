#!/usr/bin/env python3
"""Regenerate tests/golden/mosquito_goldens.json from the reference's own test DATA (not source).

Needs a checkout of the reference project (not needed to run the tests: the fixture is committed):
    python tests/golden/make_mosquito_fixtures.py REFERENCE_CHECKOUT

Produces
  mosquito_goldens.json  every key of the reference's tests/goldens/mosquito.json (22 keys, 38
                         planes: GRAY8 full / odd / tiny, GRAY10 / 12 / 14 / 16, GRAYS, YUV420P8,
                         YUV420P16, YUV444P16 and YUV444PS full), per-plane {avg (normalised by
                         2^bits - 1), min, max}. All inputs are reproducible from tests/fixtures.py
                         (tests/mosquito_ref.py golden_inputs).
Only data (expected numbers) is copied; no reference source text.
"""
import json
import sys
from pathlib import Path

OUT = Path(__file__).resolve().parent


def main() -> int:
    if len(sys.argv) != 2 or not (Path(sys.argv[1]) / "tests" / "goldens" / "mosquito.json").is_file():
        print("usage: make_mosquito_fixtures.py REFERENCE_CHECKOUT (the fixture is already committed)", file=sys.stderr)
        return 1
    data = json.loads((Path(sys.argv[1]) / "tests" / "goldens" / "mosquito.json").read_text())
    (OUT / "mosquito_goldens.json").write_text(json.dumps(data, indent=1, sort_keys=True) + "\n")
    print("wrote", OUT / "mosquito_goldens.json", len(data), "keys")
    return 0


if __name__ == "__main__":
    sys.exit(main())
