#!/bin/bash
# full -m gpu suite + the default bench line (what the driver runs at round end)
cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
tag=${1:-x}
export ZK_OUT=${ZK_OUT:-out}; out=$ZK_OUT; mkdir -p $out
timeout 1500 python -m pytest tests -m gpu -q --timeout 900 2>&1 | tail -15 > $out/r3_${tag}_gpu_tests.log; cat $out/r3_${tag}_gpu_tests.log
timeout 900 python bench.py --full > $out/r3_${tag}_bench.json 2> $out/r3_${tag}_bench.err; echo "bench rc=$?"; tail -3 $out/r3_${tag}_bench.err
python - <<PY
import json
l=json.load(open("$out/r3_${tag}_bench.json"))
print({k:l[k] for k in ("value","ms_per_step")}, l["encode"], l["round_trip"], l["roofline"]["frac"], l["reference_made_archive"]["value"], l["reference_made_archive"].get("level_3",{}).get("value"), l["seek"] and {k:v for k,v in l["seek"].items() if "p50" in str(k) or isinstance(v,(int,float))})
PY
