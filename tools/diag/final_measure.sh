# One pass over the final sources: tests, bench line, rocprofv3 kernel stats (two step counts: which nodes are capture-time only),
# roofline-only run, the four PMC passes behind roofline.traffic, the other BASELINE configs, sampling.
# usage: bash tools/diag/final_measure.sh TAG OUT_DIR   (OUT_DIR relative to the repository root)
set -o pipefail
TAG=${1:?usage: bash tools/diag/final_measure.sh TAG OUT_DIR}
O=${2:?usage: bash tools/diag/final_measure.sh TAG OUT_DIR}
cd "$(dirname "$0")/../.." && mkdir -p "$O" || exit 1
export TMPDIR=/tmp
python3 bench.py --full > $O/${TAG}_bench128.json 2> $O/${TAG}_bench128.err; tail -c 1200 $O/${TAG}_bench128.json
rocprofv3 --kernel-trace --stats --output-format csv -d $O/prof_${TAG} -- python3 bench.py --steps 5 --warmup 2 > $O/${TAG}_prof.log 2>&1
rocprofv3 --kernel-trace --stats --output-format csv -d $O/prof_${TAG}_s15 -- python3 bench.py --steps 15 --warmup 2 > $O/${TAG}_prof_s15.log 2>&1
rocprofv3 --kernel-trace --stats --output-format csv -d $O/prof_${TAG}_roof -- python3 bench.py --roofline-only > $O/${TAG}_roofline_only.json 2> $O/${TAG}_roof.err
for k in fwd wgrad; do for c in FETCH_SIZE WRITE_SIZE; do
  rocprofv3 -d $O/pmc_${k}_${c} --output-format csv --kernel-trace --pmc $c -- python3 tools/pmc_conv.py $k 32 32 128 > $O/pmc_${k}_${c}.log 2>&1; done; done
python3 tools/pmc_traffic.py $O ${TAG} 128 > $O/${TAG}_pmc.log 2>&1; tail -5 $O/${TAG}_pmc.log
cp profiles/${TAG}_pmc_traffic.json profiles/${TAG}_pmc_dispatches.csv $O/
for f in $O/prof_${TAG}/*/*kernel_stats.csv; do cp $f $O/${TAG}_bench128_graph_kernel_stats.csv; done
for f in $O/prof_${TAG}_s15/*/*kernel_stats.csv; do cp $f $O/${TAG}_bench128_steps15_kernel_stats.csv; done
for f in $O/prof_${TAG}_roof/*/*kernel_stats.csv; do cp $f $O/${TAG}_roofline_only_kernel_stats.csv; done
for c in c2 c3a c3a_gan c3b c3b_ldm c5 c5_ckpt; do python3 tools/run_configs.py $c 10 2>/dev/null | tail -1; done > $O/${TAG}_configs.json; cut -c1-110 $O/${TAG}_configs.json
python3 tools/bench_sample.py 128 50 2>/dev/null | tail -1 > $O/${TAG}_sampling.json; cut -c1-200 $O/${TAG}_sampling.json
# the bench line again with the traffic record of THIS binary in place
python3 bench.py --full --no-cpu-baseline > $O/${TAG}_bench128_with_traffic.json 2>/dev/null; python3 -c "
import json;d=json.loads(open('$O/${TAG}_bench128_with_traffic.json').read().strip().splitlines()[-1]);print(d['ms_per_step'],d['roofline']['frac'],d['roofline']['traffic'],d['roofline_fwd']['frac'],d['roofline_fwd']['traffic'])"
