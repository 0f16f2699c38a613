#!/usr/bin/env python3
"""The distinct launch shapes in a rocprofv3 kernel trace (csv), in order of first appearance:
kernel, grid (threads), workgroup, LDS bytes.  No durations and no counts (a timed warm-up repeats
a call a varying number of times), so two builds that launch the same kernels in the same shapes
print the same text.  It lists the whole trace, so it also serves where tree_trace.py finds no pass
(the run-time kernels: no kernel name marks the records' group).  The trace's LDS_Block_Size is a
kernel's static LDS only: the dynamic LDS a launch asks for does not show in it.

Usage: python3 tools/trace_shapes.py RUN_kernel_trace.csv [SUBSTRING ...]   (kernels to keep; default all)
"""
import csv
import sys


def short(name):
    name = name.replace("(anonymous namespace)", "anon")
    return name.split("(")[0].split("::")[-1]


def main():
    rows = list(csv.DictReader(open(sys.argv[1])))
    keep = sys.argv[2:]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    seen = set()
    for r in rows:
        if keep and not any(k in r["Kernel_Name"] for k in keep):
            continue
        shape = (short(r["Kernel_Name"]),
                 "x".join(r[f"Grid_Size_{a}"] for a in "XYZ"),
                 "x".join(r[f"Workgroup_Size_{a}"] for a in "XYZ"),
                 r.get("LDS_Block_Size", "?"))
        if shape not in seen:
            seen.add(shape)
            print(f"{shape[0]:28s} grid {shape[1]:>16s} wg {shape[2]:>10s} lds {shape[3]:>6s}")


if __name__ == "__main__":
    main()
