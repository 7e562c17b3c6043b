# developer helper: AEC parity tests + the default bench line
T=${1:-t}
python -m pytest tests/test_aec_gpu.py tests/test_configs_gpu.py tests/test_edges_gpu.py -m gpu -x -q > gpurun_out/${T}_pytest.log 2>&1; echo pytest rc=$?; tail -3 gpurun_out/${T}_pytest.log
python bench.py --steps 40 --warmup 8 --full --no-cpu | python -c "
import json,sys;d=json.loads(sys.stdin.read().strip().splitlines()[-1]);print(d['ms_per_step'],d['stage_ms'],d['roofline']['frac'])"
