set -o pipefail
cd /tmp && export TMPDIR=/tmp
R=$GRAFT_REPO_ROOT; O=$R/gpurun_out/exp13; mkdir -p $O
cd $R
timeout -k 10 600 python3 -m pytest tests/test_generation_gpu.py tests/test_configs_gpu.py tests/test_range_gpu.py -x -q -m gpu -k "generation or decode or greedy or token or eos or sampl" > $O/tests.log 2>&1; tail -3 $O/tests.log
for cfg in "X=1" "TCAVT_DECODE_ATTN_NO_SPEC=1"; do
  for bs in 8 32; do
    echo -n "[$cfg] B=$bs " | tee -a $O/out.txt
    env $cfg timeout -k 10 200 python3 tools/bench_generate.py --batch $bs 2>/dev/null | tail -1 | python3 -c "import sys,json; d=json.loads(sys.stdin.read()); print(d['decode_ms_per_step'], d['decode_ms_per_step_min_max_of_5'])" | tee -a $O/out.txt
  done
done
for B in 8 16; do
for tile in 0 64 128; do
  echo -n "B=$B L=128 tile=$tile " | tee -a $O/out.txt
  timeout -k 10 200 python3 bench.py --full --no-lora --mode forward --batch $B --text-len 112 --steps 10 --warmup 3 --no-cpu-baseline --tile $tile 2>/dev/null | tail -1 | python3 -c "import sys,json; d=json.loads(sys.stdin.read()); print('step', d['ms_per_step'], {k:v['avg_us'] for k,v in d['kernels'].items()})" | tee -a $O/out.txt
done
done
