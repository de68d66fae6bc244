#!/usr/bin/env python3
"""Regenerate tests/golden/packrgb_goldens.json and tests/golden/colormap_goldens.json from the reference's own test DATA (not source).

Needs a checkout of the reference project (not needed to run the tests: the fixtures are committed):
    python tests/golden/make_packrgb_fixtures.py REFERENCE_CHECKOUT

Produces
  packrgb_goldens.json   every key of the reference's tests/goldens/packrgb.json (6 keys: RGB24 and RGB30 in the geometries full, odd and
                         tiny), {avg (normalised by 255), min, max} of the packed plane seen as bytes. The inputs of all keys are
                         reproducible from tests/fixtures.py (tests/pack_rgb_ref.py golden_inputs).
  colormap_goldens.json  five of the 26 keys of the reference's tests/goldens/colormap.json: GRAY8|full|color=0, 3, 7, 8 and
                         GRAY8|odd|color=0, per-plane {avg, min, max}. These are the keys whose palettes are public formulas (autumn,
                         winter, spring, cool: tests/color_map_ref.py analytic_palette). Every other key needs the reference's palette tables,
                         which are its program text and are not in this repository; `summer` (color=6) is a formula too, but its
                         green plane does not reproduce from the formula. They are left out.
Only data (expected numbers) is copied; no reference source text.
"""
import json
import sys
from pathlib import Path

OUT = Path(__file__).resolve().parent
COLORMAP_KEYS = ["GRAY8|full|color=0", "GRAY8|full|color=3", "GRAY8|full|color=7", "GRAY8|full|color=8", "GRAY8|odd|color=0"]


def main() -> int:
    src = Path(sys.argv[1]) / "tests" / "goldens" if len(sys.argv) == 2 else None
    if src is None or not (src / "packrgb.json").is_file() or not (src / "colormap.json").is_file():
        print("usage: make_packrgb_fixtures.py REFERENCE_CHECKOUT (the fixtures are already committed)", file=sys.stderr)
        return 1
    pack = json.loads((src / "packrgb.json").read_text())
    (OUT / "packrgb_goldens.json").write_text(json.dumps(pack, indent=1, sort_keys=True) + "\n")
    print("wrote", OUT / "packrgb_goldens.json", len(pack), "keys")
    cmap = json.loads((src / "colormap.json").read_text())
    cmap = {k: cmap[k] for k in COLORMAP_KEYS}
    (OUT / "colormap_goldens.json").write_text(json.dumps(cmap, indent=1, sort_keys=True) + "\n")
    print("wrote", OUT / "colormap_goldens.json", len(cmap), "keys")
    return 0


if __name__ == "__main__":
    sys.exit(main())
