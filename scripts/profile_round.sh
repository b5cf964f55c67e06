#!/bin/bash
# usage (on the GPU box, from the repo root): scripts/profile_round.sh <tag>
# Everything the judge needs to recompute the bench line's roofline from files: written under gpurun_out/<tag>/ (copy to profiles/):
#   <tag>_bench_cfg3.json            the bench line (python bench.py --full, defaults otherwise)
#   <tag>_kernel_stats_cfg3.csv      rocprofv3 --kernel-trace --stats of the same command
#   <tag>_pmc_fetch.csv / _write.csv FETCH_SIZE and WRITE_SIZE, separate counter-only passes (MI355X_MICROARCH.md "HBM")
#   <tag>_pmc_traffic.json           per-kernel HBM bytes per launch (scripts/pmc_summary.py: corrections documented there)
#   <tag>_sq_counters.json           SQ / GRBM counters per kernel: MFMA busy, wave cycles, issue / wait split
#   manifest.json                    tag, git HEAD, kernel_source_sha (scripts/source_sha.py): bench.py checks it
TAG=${1:-round}
R=${GRAFT_REPO_ROOT:-$(pwd)}
OUT=$R/gpurun_out/$TAG
mkdir -p $OUT
SHA=$(python3 $R/scripts/source_sha.py)
cd /tmp && export TMPDIR=/tmp
# (the legs of the default command that are not the timed workload -- CPU baseline, deterministic-mode comparison, end-to-end two-phase run -- are
#  switched off under the profiler, so that a kernel's average is over the launches of the timed configuration only)
LEGS="--full --no-cpu-baseline --no-deterministic-leg --no-end-to-end"
# (every GPU step under its own time limit; a step that fails, faults or runs into its limit ends the script: nothing more is started on that card)
rm -rf /tmp/pr_trace; timeout -k 10 600 rocprofv3 --kernel-trace --stats --output-format csv -d /tmp/pr_trace -o cfg3 -- python $R/bench.py $LEGS > $OUT/${TAG}_bench_cfg3_under_rocprof.json 2> $OUT/rocprof.err || exit $?
cp $(find /tmp/pr_trace -name "*kernel_stats.csv" | head -1) $OUT/${TAG}_kernel_stats_cfg3.csv
for C in FETCH_SIZE WRITE_SIZE; do
  rm -rf /tmp/pr_$C
  timeout -k 10 600 rocprofv3 --pmc $C --output-format csv -d /tmp/pr_$C -o cfg3 -- python $R/bench.py --steps 4 --warmup 1 $LEGS > /dev/null 2> $OUT/pmc_$C.err || exit $?
done
F=$(find /tmp/pr_FETCH_SIZE -name "*counter_collection.csv" | head -1); W=$(find /tmp/pr_WRITE_SIZE -name "*counter_collection.csv" | head -1)
python3 $R/scripts/pmc_summary.py "$F" "$W" $OUT/${TAG}_pmc_traffic.json > $OUT/${TAG}_pmc_traffic_cfg3.txt
rm -rf /tmp/pr_sq
timeout -k 10 600 rocprofv3 --pmc SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_VALU_MFMA_BUSY_CYCLES SQ_INSTS_VALU SQ_INSTS_LDS SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY GRBM_GUI_ACTIVE \
  --output-format csv -d /tmp/pr_sq -o cfg3 -- python $R/bench.py --steps 4 --warmup 1 $LEGS > /dev/null 2> $OUT/pmc_sq.err || exit $?
python3 - "$(find /tmp/pr_sq -name '*counter_collection.csv' | head -1)" $OUT/${TAG}_sq_counters.json <<'PY'
import collections, csv, json, re, sys
tot = collections.defaultdict(lambda: collections.defaultdict(float)); n = collections.defaultdict(lambda: collections.defaultdict(int))
try:
    rows = list(csv.DictReader(open(sys.argv[1])))
except OSError:
    rows = []
for r in rows:
    m = re.search(r"(k_\w+)", r["Kernel_Name"]); k = m.group(1) if m else r["Kernel_Name"][:40]
    tot[k][r["Counter_Name"]] += float(r["Counter_Value"]); n[k][r["Counter_Name"]] += 1
out = {"_method": "rocprofv3 --pmc (one counter-only pass, 8 SQ slots + GRBM) of `bench.py --steps 4 --warmup 1 --no-cpu-baseline`; per launch averages. "
                  "SQ_WAVE_CYCLES / SQ_WAIT_* / SQ_ACTIVE_INST_* count quad-cycles summed over wavefronts, SQ_VALU_MFMA_BUSY_CYCLES counts cycles summed over SIMDs "
                  "(MI355X_MICROARCH.md); GRBM_GUI_ACTIVE comes out summed over the 8 XCDs (k_schur_window: 9.12 M per launch of 460 us = 8 x 2.48 GHz x 460 us), "
                  "so mfma_busy_frac = SQ_VALU_MFMA_BUSY_CYCLES / (GRBM_GUI_ACTIVE / 8 * 256 CUs * 4 SIMDs): busy cycles of the matrix pipes over the SIMD cycles of the launch "
                  "(sets up to r02g divided by GRBM_GUI_ACTIVE * 1024 and read 8 x too low)", "kernels": {}}
for k in tot:
    e = {c: tot[k][c] / max(1, n[k][c]) for c in tot[k]}
    e["launches"] = max(n[k].values())
    if e.get("GRBM_GUI_ACTIVE"):
        e["mfma_busy_frac"] = e.get("SQ_VALU_MFMA_BUSY_CYCLES", 0.0) / (e["GRBM_GUI_ACTIVE"] / 8.0 * 256 * 4)
    if e.get("SQ_WAVE_CYCLES"):
        e["wait_frac"] = e.get("SQ_WAIT_ANY", 0.0) / e["SQ_WAVE_CYCLES"]; e["issue_stall_frac"] = e.get("SQ_WAIT_INST_ANY", 0.0) / e["SQ_WAVE_CYCLES"]
        e["active_frac"] = e.get("SQ_ACTIVE_INST_ANY", 0.0) / e["SQ_WAVE_CYCLES"]
    out["kernels"][k] = e
json.dump(out, open(sys.argv[2], "w"), indent=1, sort_keys=True)
for k, e in sorted(out["kernels"].items(), key=lambda kv: -kv[1].get("GRBM_GUI_ACTIVE", 0) * kv[1]["launches"])[:12]:
    print("%-22s launches %5d  mfma_busy %6.3f  active %5.2f  wait %5.2f  issue-stall %5.2f" % (k, e["launches"], e.get("mfma_busy_frac", float("nan")), e.get("active_frac", float("nan")), e.get("wait_frac", float("nan")), e.get("issue_stall_frac", float("nan"))))
PY
# the manifest and the counter summaries go into profiles/ of THIS copy of the repo first, so that the bench line measured next carries
# traffic / rocprof_avg_us / sq from the set it belongs to (bench.py reads profiles/manifest.json and checks the kernel-source hash)
python3 - $OUT $TAG $SHA <<'PY'
import json, os, sys
out, tag, sha = sys.argv[1:4]
json.dump({"tag": tag, "kernel_source_sha": sha, "files": {"bench": tag + "_bench_cfg3.json", "measured_peaks": tag + "_measured_peaks.json", "kernel_stats": tag + "_kernel_stats_cfg3.csv", "pmc_traffic": tag + "_pmc_traffic.json",
                                                              "sq_counters": tag + "_sq_counters.json"},
           "note": "measured by scripts/profile_round.sh on one MI355X; kernel_source_sha = scripts/source_sha.py over obvi-slam_amd/csrc at measurement time"},
          open(os.path.join(out, "manifest.json"), "w"), indent=1)
PY
cp $OUT/manifest.json $OUT/${TAG}_kernel_stats_cfg3.csv $OUT/${TAG}_pmc_traffic.json $OUT/${TAG}_sq_counters.json $R/profiles/ 2>/dev/null
timeout -k 10 900 python $R/bench.py --full > $OUT/${TAG}_bench_cfg3.json 2> $OUT/bench.err || exit $?
python3 - $OUT $TAG $SHA <<'PY'
import json, os, subprocess, sys
out, tag, sha = sys.argv[1:4]
peaks = None
try:
    peaks = json.load(open(os.path.join(out, tag + "_bench_cfg3.json")))["roofline"]["peaks_measured"]
    json.dump({"_method": "obvi_ba_measure_peaks in the bench run of this set (csrc/peak_kernels.hip): HBM triad / copy / read over 1 GiB arrays, fp64 MFMA issue rate "
                          "(v_mfma_f64_16x16x4_f64, register operands, 8 accumulators per wavefront, 2 wavefronts per SIMD) and the LDS-fed 64x64x64 tile product", "peaks": peaks},
              open(os.path.join(out, tag + "_measured_peaks.json"), "w"), indent=1)
except (OSError, ValueError, KeyError):
    pass
json.dump({"tag": tag, "kernel_source_sha": sha, "files": {"bench": tag + "_bench_cfg3.json", "measured_peaks": tag + "_measured_peaks.json", "kernel_stats": tag + "_kernel_stats_cfg3.csv", "pmc_traffic": tag + "_pmc_traffic.json",
                                                              "sq_counters": tag + "_sq_counters.json"},
           "note": "measured by scripts/profile_round.sh on one MI355X; kernel_source_sha = scripts/source_sha.py over obvi-slam_amd/csrc at measurement time"},
          open(os.path.join(out, "manifest.json"), "w"), indent=1)
PY
ls $OUT | head -30
grep -h metric $OUT/${TAG}_bench_cfg3.json | cut -c1-300
