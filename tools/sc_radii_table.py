"""Prints the C radius table of arpeggia_amd/csrc/sc.cpp (kScRadii) from tests/golden/sc_radii.csv, the reference's Lawrence & Colman
table (src/sc/atomic_radii.rs) as data, in table order.  Usage: python tools/sc_radii_table.py > table.txt, then paste."""
import csv
from pathlib import Path

with open(Path(__file__).resolve().parent.parent / "tests" / "golden" / "sc_radii.csv") as f:
    rows = list(csv.DictReader(f))
line = "   "
for r in rows:
    ent = f' {{"{r["residue"]}", "{r["atom"]}", {r["radius"]}}},'
    if len(line) + len(ent) > 140:
        print(line)
        line = "   "
    line += ent
print(line)
