# usage: bash tools/gpu_train_timeline.sh <outdir-name> [train-batch] -- one training step as a time line with stream ids
cd "$(dirname "$0")/.."
. tools/gpu_step.sh
export TMPDIR=/tmp
O=gpurun_out/$1; mkdir -p $O
exec 3>&2; trap 's=$?; [ $s -eq 0 ] || echo "gpu_train_timeline: stopped with status $s (log: $O/rocprof_tl.log)" >&3' EXIT   # (fd 3: step's own message follows the caller's redirection into the log)
B=${2:-8}
rm -rf /tmp/prof_tl; mkdir -p /tmp/prof_tl
step 300 rocprofv3 --kernel-trace -d /tmp/prof_tl -o t -- python3 bench.py --workload train-synth256 --train-batch $B --steps 3 --warmup 1 --cpu-seconds 0 > $O/rocprof_tl.log 2>&1
DB=$(find /tmp/prof_tl -name '*results.db' | head -1)
python3 tools/timeline_rocprof.py $DB -o $O/train_b${B}_timeline.txt
tail -5 $O/train_b${B}_timeline.txt
