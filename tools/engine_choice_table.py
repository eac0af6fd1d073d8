#!/usr/bin/env python3
"""Write the engine-choice table of tests/engine_choices.py for one library, to compare it with
tests/golden/engine_choices.json (or with the table of another commit).

  tools/engine_choice_table.py --lib tests/emu/libfltx_emu.so --out /tmp/choices.json
  (the emulator of another checkout: EMU_OUT=/tmp/emu.so tests/emu/build.sh there)

Without --lib the HIP library (text_amd/lib/libfltx.so) on the first GPU is used."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import engine_choices  # noqa: E402
import helpers  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--lib", help="libfltx.so or an emulator build of it (default: the HIP library)")
    ap.add_argument("--out", required=True, help="JSON file to write")
    a = ap.parse_args()
    tab = engine_choices.table(helpers.FltxSession(os.path.abspath(a.lib) if a.lib else None))
    with open(a.out, "w") as f:
        f.write(engine_choices.dumps(tab))
    for fam, rows in sorted(engine_choices.family_counts(tab).items()):
        print("%-13s %s" % (fam, ", ".join("%s: %d" % (g, n) for g, n in sorted(rows.items()))))
    print("%d configurations -> %s" % (len(tab), a.out))


if __name__ == "__main__":
    main()
