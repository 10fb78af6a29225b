"""Prints the headline figures of a bench.py JSON line: print_bench.py <file>   (a plain run's line carries the headline and,
with --warmup >= 5, the solver roofline; the other configurations, the small-island sample and the CPU baseline come with --full)"""
import json, sys
j = json.load(open(sys.argv[1]))
print("value %.1f %s  ms/step %.4f  (%s run)" % (j["value"], j["unit"], j["ms_per_step"], "full" if j.get("full", True) else "plain"))
r = j.get("roofline") or {}
if r.get("frac") is not None:
    print("solver %.1f us  frac %.4f" % (r.get("mean_launch_us", 1000.0 * r.get("family_ms_per_step", 0.0)), r["frac"]))
print("device profile", j.get("device_profile_ms"))
for e in j.get("extra_configs") or []:
    if "ms_per_step" in e: print("  %-60s %.3f ms/step" % (e["workload"][:60], e["ms_per_step"]))
if (j.get("roofline_small_islands") or {}).get("frac") is not None: print("small islands", j["roofline_small_islands"]["mean_launch_us"], j["roofline_small_islands"]["frac"])
print("cpu", (j.get("cpu_baseline") or {}).get("value"))
