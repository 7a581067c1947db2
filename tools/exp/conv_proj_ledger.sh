#!/bin/bash
# usage (GPU box): tools/exp/conv_proj_ledger.sh "<tags>" [bench args] -- the message kernel's slot-step ledger: per-launch time of
# conv_proj_kernel (rocprofv3 kernel statistics, 30 eager steps of the 256 x 20 step) for the in-tree library ("cur") and for every
# timing-only build tools/exp/ab/lib_<tag>.so (tools/exp/build_conv_proj_exp.sh), the in-tree library again after every third
# variant so that the box's drift is seen.  The variants' results are wrong on purpose (ARREAU_BENCH_TIMING_ONLY=1 marks the lines).
# A run that fails or times out ends the script: nothing more is started on that GPU.
tags="$1"; shift
cd "$(dirname "$0")/../.." && root=$(pwd) && export TMPDIR=/tmp
# No per-model calibration (as tools/prof_bench.sh): arreau_model_create would otherwise score the fp8 formats THROUGH the variant library,
# find its wrong numbers out of bounds and switch the run to another instantiation of the kernel.  Every line names the kernel
# that was timed and the status word's conv_cross_fp8; a line with more than one conv_proj_kernel row lists them all.
export ARREAU_CALIBRATE=0
out=${ARREAU_OUT:-results}/cp_ledger; mkdir -p $out  # where the results go (relative to the repository root)
seq=""; i=0
for t in $tags; do if [ $((i % 3)) = 0 ]; then seq="$seq cur"; fi; seq="$seq $t"; i=$((i + 1)); done
seq="$seq cur"
k=0
for tag in $seq; do
  k=$((k + 1))
  if [ $tag = cur ]; then unset ARREAU_HIP_LIB ARREAU_BENCH_TIMING_ONLY
  else export ARREAU_HIP_LIB=$root/tools/exp/ab/lib_$tag.so ARREAU_BENCH_TIMING_ONLY=1; fi
  d=$out/${k}_$tag; rm -rf $d
  timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $d -- python bench.py --steps 30 --warmup 5 \
      --no-graph-loop --no-other-configs "$@" > $d.json 2> $d.err || { echo "$tag: run failed ($?), stopping" | tee -a $out/ledger.txt; exit 1; }
  python - $d $tag <<'PY' | tee -a $out/ledger.txt
import csv, glob, json, re, sys
d, tag = sys.argv[1:3]
f = glob.glob(d + "/*/*kernel_stats.csv")
rows = [(r["Name"], float(r["AverageNs"]) / 1e3, int(r["Calls"])) for r in csv.DictReader(open(f[0]))] if f else []
cp = [r for r in rows if "conv_proj_kernel" in r[0]]
res = json.loads(open(d + ".json").read().strip().splitlines()[-1])
x8 = re.search(r"conv_cross_fp8=(\S+)", res.get("dtype_note", ""))
if not cp:
    print("%-6s no conv_proj_kernel row" % tag)
for name, us, calls in cp:
    print("%-6s %-44s %7.2f us x %3d launches | conv_cross_fp8=%s | eager step %.4f ms"
          % (tag, name.split("(")[0].replace("void ", ""), us, calls, x8.group(1) if x8 else "?", res.get("ms_per_step", float("nan"))))
PY
  rm -rf $d  # (the traces are large; the ledger line is what is kept)
done
