#!/bin/bash
# one-proof-in-flight kernel durations (uncontended) of the current build: LDE, leaf hash (quad form), quotient
R=${GRAFT_REPO_ROOT:-$(pwd)}
cd $R
J=$(mktemp); E=$(mktemp)
env $1 timeout -k 10 300 python3 bench.py --steps 3 --warmup 1 --inflight 1 --full --no-boundary --no-cpu-baseline > $J 2> $E || { tail -3 $E; rm -f $J $E; exit 1; }
python3 - $J <<'PY'
import json, sys
d = json.loads(open(sys.argv[1]).read().strip().splitlines()[-1])
print("latency", round(d["latency_ms_one_in_flight"], 1), {k: round(v["avg_ms"], 2) for k, v in d["kernels"].items()}, {k: round(v, 1) for k, v in d["phase_ms_one_in_flight"].items()})
PY
rm -f $J $E
