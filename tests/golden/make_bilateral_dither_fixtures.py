#!/usr/bin/env python3
"""Regenerate tests/golden/bilateral_dither_goldens.json from the reference's own test DATA (not source).

Needs a checkout of the reference project (not needed to run the tests: the fixture is committed):
    python tests/golden/make_bilateral_dither_fixtures.py REFERENCE_CHECKOUT

Produces
  bilateral_dither_goldens.json  every key of the reference's tests/goldens/bilateral_dither.json (23 keys, 43 planes: GRAY8 full
                                 in nine parameter sets and odd, GRAY16, GRAYS, YUV420P8 / P16, YUV444P16 / PS, RGB24 and RGBS full),
                                 per-plane {avg (normalised by 2^bits - 1), min, max}. The inputs of all keys are reproducible
                                 from tests/fixtures.py (tests/bilateral_dither_ref.py golden_inputs).
Only data (expected numbers) is copied; no reference source text.
"""
import json
import sys
from pathlib import Path

OUT = Path(__file__).resolve().parent


def main() -> int:
    if len(sys.argv) != 2 or not (Path(sys.argv[1]) / "tests" / "goldens" / "bilateral_dither.json").is_file():
        print("usage: make_bilateral_dither_fixtures.py REFERENCE_CHECKOUT (the fixture is already committed)", file=sys.stderr)
        return 1
    data = json.loads((Path(sys.argv[1]) / "tests" / "goldens" / "bilateral_dither.json").read_text())
    (OUT / "bilateral_dither_goldens.json").write_text(json.dumps(data, indent=1, sort_keys=True) + "\n")
    print("wrote", OUT / "bilateral_dither_goldens.json", len(data), "keys")
    return 0


if __name__ == "__main__":
    sys.exit(main())
