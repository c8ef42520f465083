#!/bin/bash
# round-2 validation: GPU parity suite, full bench (headline + configs array), virtual-rank profile
#   gpu_validate.sh OUT_DIR
OUT=${1:?usage: scripts/gpu_validate.sh OUT_DIR}
cd "$GRAFT_REPO_ROOT" 2>/dev/null || cd /root/repo
mkdir -p "$OUT"
(time timeout 1500 python -m pytest tests -m gpu -x -q --durations=6) > "$OUT/pytest.log" 2>&1
tail -14 "$OUT/pytest.log"
(time timeout 900 python bench.py --full) > "$OUT/bench.json" 2> "$OUT/bench.err"
tail -4 "$OUT/bench.err"
timeout 600 python scripts/gpu_virtual_ranks.py > "$OUT/virtual_ranks.jsonl" 2>> "$OUT/err.log"
timeout 300 python scripts/gpu_host_path.py > "$OUT/host_path.log" 2>&1
python -c "
import json,sys
sys.path.insert(0,'scripts')
import _benchout
d=_benchout.legacy(*_benchout.load(open(sys.argv[1])))
print(d['value'], d['ms_per_step'], d['lcp'], d['verified'], d['roofline']['frac'], d['roofline'].get('traffic_commit'), d['roofline'].get('this_commit'))
for c in d['configs']: print({k:c.get(k) for k in ('config','sa_ms','lcp_ms','sa_MB/s','fused_sa_lcp','bit_exact_vs_pins','error','queries')})
" "$OUT/bench.json"
cat "$OUT/virtual_ranks.jsonl" | cut -c1-400; cat "$OUT/host_path.log" | tail -5
