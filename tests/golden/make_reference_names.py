"""Writes tests/golden/reference_dart_names.json: every identifier of the reference's Dart library (lib/**/*.dart of a
DartRay checkout) that integration/hip_sampler_renderer.dart or integration/hip_render_manager.dart contains.

tests/test_abi_c_host.py checks the names those two files use against this list, so the suite needs no reference
checkout.  A name that is new to the integration files has to be found in the reference by re-running this script:

    python tests/golden/make_reference_names.py /path/to/dartray
"""
import glob
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "reference_dart_names.json")
WORD = re.compile(r"\b[A-Za-z_]\w*\b")


def main(reference):
    files = glob.glob(os.path.join(reference, "lib", "**", "*.dart"), recursive=True)
    if not files:
        raise SystemExit("no lib/**/*.dart under %s" % reference)
    ref_words = set()
    for f in files:
        ref_words |= set(WORD.findall(open(f, errors="ignore").read()))
    ours = set()
    for name in ("hip_sampler_renderer.dart", "hip_render_manager.dart"):
        ours |= set(WORD.findall(open(os.path.join(ROOT, "integration", name)).read()))
    names = sorted(ours & ref_words)
    with open(OUT, "w") as fh:
        json.dump({"what": "identifiers of the reference's lib/**/*.dart that integration/*.dart contains", "names": names}, fh, indent=0)
        fh.write("\n")
    print("%d names from %d reference files -> %s" % (len(names), len(files), os.path.relpath(OUT, ROOT)))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else ".")
