#!/usr/bin/env python3
"""Regenerate tests/golden/deband_goldens.json from the reference's own test DATA (not source).

Needs a checkout of the reference project (not needed to run the tests: the fixture is committed):
    python tests/golden/make_deband_fixtures.py REFERENCE_CHECKOUT

Produces
  deband_goldens.json  every key of the reference's tests/goldens/deband.json (43 keys, 61 planes: GRAY16 full
                       in 29 parameter sets, odd and tiny, GRAY8, GRAYS, YUV420P8 / P16, YUV422P8 / P16,
                       YUV444PS, RGB48 and RGBS full), per-plane {avg (normalised by 2^bits - 1), min, max}.
                       The inputs of the 40 keys at 16 bits or float are reproducible from tests/fixtures.py
                       (tests/deband_ref.py golden_inputs); the three 8-bit keys pass through the host's
                       resizer around the filter and are not rebuilt.
Only data (expected numbers) is copied; no reference source text.
"""
import json
import sys
from pathlib import Path

OUT = Path(__file__).resolve().parent


def main() -> int:
    if len(sys.argv) != 2 or not (Path(sys.argv[1]) / "tests" / "goldens" / "deband.json").is_file():
        print("usage: make_deband_fixtures.py REFERENCE_CHECKOUT (the fixture is already committed)", file=sys.stderr)
        return 1
    data = json.loads((Path(sys.argv[1]) / "tests" / "goldens" / "deband.json").read_text())
    (OUT / "deband_goldens.json").write_text(json.dumps(data, indent=1, sort_keys=True) + "\n")
    print("wrote", OUT / "deband_goldens.json", len(data), "keys")
    return 0


if __name__ == "__main__":
    sys.exit(main())
