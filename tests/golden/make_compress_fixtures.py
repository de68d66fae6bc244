#!/usr/bin/env python3
"""Regenerate tests/golden/compress_goldens.json from the reference's own test DATA (not source).

Needs a checkout of the reference project (not needed to run the tests: the fixture is committed):
    python tests/golden/make_compress_fixtures.py REFERENCE_CHECKOUT

Produces
  compress_goldens.json  every key of the reference's tests/goldens/compress.json (25 keys, 43 planes: GRAY8 full in twelve
                         parameter sets, odd and tiny for both codecs, YUV420P8 / YUV422P8 / YUV444P8 full for both codecs and
                         with chroma=0), per-plane {avg (normalised by 255), min, max}. The inputs of all keys are reproducible
                         from tests/fixtures.py (tests/compress_ref.py golden_inputs).
Only data (expected numbers) is copied; no reference source text.
"""
import json
import sys
from pathlib import Path

OUT = Path(__file__).resolve().parent


def main() -> int:
    if len(sys.argv) != 2 or not (Path(sys.argv[1]) / "tests" / "goldens" / "compress.json").is_file():
        print("usage: make_compress_fixtures.py REFERENCE_CHECKOUT (the fixture is already committed)", file=sys.stderr)
        return 1
    data = json.loads((Path(sys.argv[1]) / "tests" / "goldens" / "compress.json").read_text())
    (OUT / "compress_goldens.json").write_text(json.dumps(data, indent=1, sort_keys=True) + "\n")
    print("wrote", OUT / "compress_goldens.json", len(data), "keys")
    return 0


if __name__ == "__main__":
    sys.exit(main())
