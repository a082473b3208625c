"""The launches of a rocprofv3 kernel trace in the order the host enqueued them, one per line: kernel name, grid, workgroup size.
    rocprofv3 --output-format csv --kernel-trace -d DIR -o NAME -- python tools/launch_fingerprint.py
    python tools/kernel_trace_list.py DIR/**/NAME_kernel_trace.csv > list.txt
Two builds of the library that launch the same kernels with the same shapes write the same list (tools/launch_fingerprint.py --lib takes
another build): the check that a change to the host side of a launcher picks the same template instantiations, which results cannot show
where two variants agree on the inputs at hand.  Grids are in workgroups."""
import csv
import sys

rows = list(csv.DictReader(open(sys.argv[1])))
rows.sort(key=lambda r: int(r["Dispatch_Id"]) if r.get("Dispatch_Id") else int(r["Start_Timestamp"]))
for r in rows:
    wg = [max(1, int(r["Workgroup_Size_" + a])) for a in "XYZ"]
    grid = [int(r["Grid_Size_" + a]) // w for a, w in zip("XYZ", wg)]
    print("%s grid=%dx%dx%d wg=%dx%dx%d" % (r["Kernel_Name"], *grid, *wg))
