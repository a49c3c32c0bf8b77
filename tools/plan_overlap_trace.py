"""Summarise the kernel traces of tools/gpu_prof_plan_overlap.sh: per variant, the k_stream
launches of the last (timed) call, each with the plan kernels that ran inside
its interval, and the stats rows of the three kernels."""
import csv
import glob
import json
import statistics as st
import sys

out = sys.argv[1]
res = {}
for v in ("base", "new"):
    tr = glob.glob(f"{out}/{v}/**/*kernel_trace.csv", recursive=True)
    if not tr:
        continue
    rows = []
    with open(tr[0]) as f:
        for r in csv.DictReader(f):
            n = r["Kernel_Name"]
            if "k_stream<" in n or "k_bplan" in n:
                kind = "stream" if "k_stream<" in n else ("sort" if "k_bplan_sort" in n else "build")
                rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), kind,
                             r.get("Stream_Id"), r.get("Queue_Id")))
    rows.sort()
    streams = [r for r in rows if r[2] == "stream" and r[1] - r[0] > 1_000_000]
    last = streams[-6:]
    t0 = last[0][0]
    chunks = []
    for s in last:
        inside = [(p[2], round((p[0] - s[0]) / 1e3, 1), round((p[1] - p[0]) / 1e3, 1), p[3], p[4])
                  for p in rows if p[2] != "stream" and p[0] >= s[0] and p[1] <= s[1]]
        chunks.append({"start_us": round((s[0] - t0) / 1e3, 1), "dur_us": round((s[1] - s[0]) / 1e3, 1),
                       "stream_id": s[3], "queue_id": s[4],
                       "plans_inside(kind,offset_us,dur_us,stream,queue)": inside})
    # plan kernels of the timed call that ran outside every k_stream interval
    outside = [(p[2], round((p[0] - t0) / 1e3, 1), round((p[1] - p[0]) / 1e3, 1)) for p in rows
               if p[2] != "stream" and p[0] >= t0 - 300_000 and not any(p[0] >= s[0] and p[1] <= s[1] for s in last)]
    full = [r[1] - r[0] for r in streams if abs((r[1] - r[0]) - st.median([x[1] - x[0] for x in last])) < 300_000]
    res[v] = {"timed_call_span_us": round((last[-1][1] - t0) / 1e3, 1),
              "k_stream_dur_us_timed_call": [c["dur_us"] for c in chunks],
              "k_stream_647_batches_median_us_all_calls": round(st.median(full) / 1e3, 1), "n_all": len(full),
              "plans_outside_timed_call(kind,start_us,dur_us)": outside, "chunks": chunks}
    stats = glob.glob(f"{out}/{v}/**/*kernel_stats.csv", recursive=True)
    if stats:
        with open(stats[0]) as f, open(f"{out}/kernel_stats_{v}.csv", "w") as g:
            for k, line in enumerate(f):
                if k == 0 or "k_stream" in line or "k_bplan" in line:
                    g.write(line)
json.dump(res, open(f"{out}/trace_summary.json", "w"), indent=1)
for v, r in res.items():
    print(v, json.dumps({k: r[k] for k in r if k != "chunks"})[:1500])
    for c in r["chunks"][:3]:
        print("  ", json.dumps(c)[:600])
