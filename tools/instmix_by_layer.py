#!/usr/bin/env python3
"""Per-layer dynamic instruction mix from a counters-only rocprofv3 run (`--pmc ... --output-format csv`, no tracing).

usage: tools/instmix_by_layer.py <counter_collection.csv> [-o out.csv] [--cycle SUBSTR] [--names a,b,c]

A dispatch is keyed by its position since the last kernel whose name contains SUBSTR (default `gather_`: one UNet pass of the
resident slide = gather, 16 convolutions; the stitch follows a band of passes), which separates the layers that share a kernel
instantiation; `--names` labels the positions (default: the split-precision plan of the bench graph).  Counters are summed over the
dispatches of a position and divided by its SQ_WAVES: instructions PER WAVE, the unit of the static counts in docs/experiments.md."""
import argparse
import csv
from collections import OrderedDict

NAMES = ("pi2d.gather_normalise,ld0.conv,ld1.conv,ld2.conv,ld3.conv,ld4.conv,lb.conv,lu4.convT,lu4.conv,lu3.convT,lu3.conv,lu2.convT,"
         "lu2.conv,lu1.convT,lu1.conv,lu0.convT,lu0.conv,pi2d.stitch")
COLS = ["SQ_INSTS_VALU", "SQ_INSTS_MFMA", "SQ_INSTS_SALU", "SQ_INSTS_LDS", "SQ_INSTS_VMEM", "SQ_INSTS_BRANCH"]


def short(name):
    return name.replace("void ", "").split("(")[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("csv")
    ap.add_argument("-o", "--out")
    ap.add_argument("--cycle", default="gather_")
    ap.add_argument("--names", default=NAMES)
    a = ap.parse_args()
    names = a.names.split(",")
    table = OrderedDict()   # (pos, kernel) -> {"n": dispatches, counter: sum}
    pos, last = -1, None
    with open(a.csv, newline="") as f:
        for r in csv.DictReader(f):
            if r["Dispatch_Id"] != last:
                last = r["Dispatch_Id"]
                if a.cycle in r["Kernel_Name"]:
                    pos = 0
                elif pos >= 0:
                    pos += 1
                cur = None
                if pos >= 0 and "umx::" in r["Kernel_Name"]:
                    cur = table.setdefault((pos, short(r["Kernel_Name"])), {"n": 0})
                    cur["n"] += 1
            if cur is not None:
                cur[r["Counter_Name"]] = cur.get(r["Counter_Name"], 0.0) + float(r["Counter_Value"])
    rows = [["layer", "kernel", "dispatches", "waves_per_dispatch"] + [c + "_per_wave" for c in COLS]]
    for (p, k), e in table.items():
        waves = e.get("SQ_WAVES", 0.0)
        if not waves:
            continue
        rows.append([names[p] if p < len(names) else "pos%d" % p, k, e["n"], "%.0f" % (waves / e["n"])] +
                    ["%.1f" % (e.get(c, 0.0) / waves) for c in COLS])
    out = open(a.out, "w", newline="") if a.out else None
    w = csv.writer(out) if out else None
    for r in rows:
        if w:
            w.writerow(r)
        print(" ".join("%-14s" % str(x)[:40] if i != 1 else "%-62s" % str(x)[:60] for i, x in enumerate(r)))


if __name__ == "__main__":
    main()
