#!/bin/bash
# the round's verification in one run: GPU suite, smoke(), the full bench line (-> <outdir>)     usage: run_t.sh <outdir>
out=${1:?usage: run_t.sh <outdir>}; mkdir -p "$out"
python -m pytest tests -m gpu -q -x 2>&1 | tail -3 > "$out/verify_tests.log"
python -c "import __graft_entry__ as g; g.smoke(); print('smoke ok')" > "$out/verify_smoke.log" 2>&1
python bench.py --full > "$out/verify_bench.json" 2> "$out/verify_bench.err"
cat "$out/verify_tests.log"; tail -1 "$out/verify_smoke.log"
python - "$out/verify_bench.json" <<'PY'
import json, sys
d = json.loads([l for l in open(sys.argv[1]) if l.startswith('{')][-1])
print(d['ms_per_step'], d['value'], d['roofline']['frac'], d['roofline']['avg_launch_us'])
for k, v in d['other_configs'].items():
    print(k, v.get('ms_per_step'), v.get('captions_per_s'), v.get('error'))
PY
