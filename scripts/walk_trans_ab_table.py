"""Table of scripts/walk_trans_ab.sh's output directory: per round and build the walk by
its own clock, rocprofv3's k_pll_walk average with the early hand-off off (and that run's
own-clock figure), and the 20-step and 100-step bench lines; then the bar of the A/B:
the walk lower in every round, and the mean gain against the larger min-max spread."""
import csv
import glob
import json
import os
import sys

out = sys.argv[1]


def line(path):
    with open(path) as f:
        rows = [ln for ln in f.read().splitlines() if ln.startswith("{")]
    return json.loads(rows[-1])


def trace_avg_ms(d):
    for p in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
        with open(p, newline="") as f:
            for row in csv.DictReader(f):
                if "k_pll_walk" in row["Name"]:
                    return float(row["AverageNs"]) / 1e6, int(row["Calls"])
    return float("nan"), 0


walk = {"parent": [], "new": []}
print("round build  walk_ms_per_launch  full20_ms_per_step  trace_walk_avg_ms (calls; own clock in that run)  "
      "plain20_ms_per_step  plain100_ms_per_step  entries/repairs/fallback_lane_blocks")
for r in (1, 2, 3):
    for b in ("parent", "new"):
        t = os.path.join(out, f"{b}_r{r}")
        full = line(t + ".full20.json")
        p20 = line(t + ".plain20.json")
        p100 = line(t + ".plain100.json")
        tr = line(t + ".trace.log")
        avg, calls = trace_avg_ms(t + ".trace")
        sc = full["roofline"].get("serial_chain", {})
        walk[b].append(full["roofline"]["ms_per_launch"])
        print(f"{r}     {b:6s} {full['roofline']['ms_per_launch']:<19.4f} {full['ms_per_step']:<19.4f} "
              f"{avg:.4f} ({calls}; {tr['roofline']['ms_per_launch']:.4f})".ljust(96)
              + f" {p20['ms_per_step']:<20.4f} {p100['ms_per_step']:<21.4f} "
              f"{sc.get('entries')}/{sc.get('repairs')}/{sc.get('fallback_lane_blocks')}")
gain = [p - n for p, n in zip(walk["parent"], walk["new"])]
spread = max(max(v) - min(v) for v in walk.values())
mean = sum(gain) / len(gain)
print(f"# walk by its own clock: parent {min(walk['parent']):.4f}-{max(walk['parent']):.4f} ms, "
      f"new {min(walk['new']):.4f}-{max(walk['new']):.4f} ms; gain per round "
      + ", ".join(f"{g:.4f}" for g in gain) + f" ms, mean {mean:.4f} ms")
print(f"# larger min-max spread of the two builds {spread:.4f} ms; mean gain / spread {mean / spread if spread else float('inf'):.1f} "
      f"(bar: lower in every round and >= 3): {'cleared' if min(gain) > 0 and mean >= 3 * spread else 'NOT cleared'}")
