#!/usr/bin/env python3
"""Record what pal_plan_info / pal_plan_factors report for a fixed set of frame lengths under each plan switch.

    python tools/record_plan_table.py [out.json]        (PAL_LIB_PATH chooses the library, as for every A/B run)

The output is the fixture tests/golden/plan_table.json: it was recorded from the library of the commit before
csrc/plan_geometry.h existed, and both the host test (tests/host/test_plan_geometry.cpp, through
tests/test_host_plan_geometry.py) and the device test (tests/test_gpu_plan_table.py) compare against it.
One engine per switch set; the plans are dropped between sets.
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# one length per (convolution kind x cut outcome) class below 300 000 ...
CLASS_LENGTHS = [1, 2, 129, 257, 496, 513, 2049, 2050, 2051, 2052, 2053, 2071, 2478, 3073, 3076, 4097, 6148, 8193, 8195, 8196, 8197,
                 8204, 8206, 8208, 8424, 12465, 20010, 24577, 24579, 24580, 24581, 24584, 24588, 25172, 25271, 45091, 47139, 49153,
                 49154, 49156, 49165, 49167, 49907, 50046, 63535, 93412, 98310, 98317, 98326, 131079, 131098, 186505, 196649,
                 227384, 262146]
# ... and the lengths whose plans the device tests pin (test_gpu_parity.py, test_gpu_peak_positions.py)
PINNED_LENGTHS = [50, 496, 500, 1000, 2500, 6007, 2048, 2999, 3000, 5000, 10233, 24000, 12000, 11170, 44100,
                  11437, 8193, 8538, 16051, 23564, 1008, 11962, 15525, 22651, 7890,
                  16000, 18000, 20000, 22000, 30000, 36000, 40500, 44102, 48001, 60000, 90000]
SWITCH_LENGTHS = [496, 2999, 8193, 10233, 12000, 24000, 30000, 44100, 60000, 90000, 131079]
SWITCH_SETS = ["", "PAL_RADIX3=0", "PAL_FOUR_REG=0", "PAL_PFA_BIG=0", "PAL_RADER=0", "PAL_PFA=0"]
FIELDS = ["n", "conv_len", "m1", "m2", "n1", "n2", "tile_len"]


def record(switch, lengths):
    from pyaudiolocalization_amd import Engine
    name = switch.split("=")[0] if switch else None
    if name:
        os.environ[name] = switch.split("=")[1]
    try:
        eng = Engine(0)
        try:
            rows = {}
            for length in lengths:
                info = eng.plan_info(length)
                rows[str(length)] = [info[k] for k in FIELDS]
            eng.clear_plans()
        finally:
            eng.close()
    finally:
        if name:
            del os.environ[name]
    return rows


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "plan_table.json")
    table = {"fields": FIELDS, "sets": {}}
    for switch in SWITCH_SETS:
        lengths = sorted(set(CLASS_LENGTHS + PINNED_LENGTHS)) if not switch else SWITCH_LENGTHS
        table["sets"][switch or "default"] = record(switch, lengths)
    with open(out, "w") as fh:
        fh.write("{\n \"fields\": %s,\n \"sets\": {\n" % json.dumps(FIELDS))
        sets = list(table["sets"].items())
        for i, (name, rows) in enumerate(sets):
            body = ",\n".join("   %s: %s" % (json.dumps(k), json.dumps(v)) for k, v in rows.items())
            fh.write("  %s: {\n%s\n  }%s\n" % (json.dumps(name), body, "," if i + 1 < len(sets) else ""))
        fh.write(" }\n}\n")
    print("wrote", out, sum(len(r) for r in table["sets"].values()), "rows")


if __name__ == "__main__":
    main()
