#!/bin/bash
# tools/mstg_cluster_rate.sh [OUT.json] [N_SMALL] : the legs of tools/mstg_cluster_rate.py, each GPU step under its own time
# limit, chained so that nothing starts after a failure; the record is merged into OUT (default
# profiles/mstg_cluster_rate_1m_d960.json).  Configuration A: max_posting_size 5000, k 10 at 1 M x 960.  Configuration B: the
# crate's Python default max_posting_size 16, k 10, with the host_below sweep, at N_SMALL rows (default 1 M; about N / 10
# splits).  The kernel split comes from a rocprofv3 run of its own (kernel trace only, no counters).
set -o pipefail
cd "$(dirname "$0")/.."
O=${1:-profiles/mstg_cluster_rate_1m_d960.json}
NB=${2:-1000000}
T=$(mktemp -d)
rm -f "$O"
timeout -k 10 600 python tools/mstg_cluster_rate.py --legs device --tag a_5000_k10 --out "$O" &&
timeout -k 10 900 python tools/mstg_cluster_rate.py --legs percall --tag a_5000_k10 --out "$O" &&
timeout -k 10 900 python tools/mstg_cluster_rate.py --legs cpu --tag a_5000_k10 --out "$O" &&
timeout -k 10 1100 python tools/mstg_cluster_rate.py --n "$NB" --max-posting-size 16 --legs sweep --tag b_16_k10 --out "$O" &&
timeout -k 10 900 python tools/mstg_cluster_rate.py --n "$NB" --max-posting-size 16 --legs cpu --cpu-n 5000 --tag b_16_k10 --out "$O" &&
timeout -k 10 900 rocprofv3 --kernel-trace --stats -d "$T" -o hc -- python tools/mstg_cluster_rate.py --legs device --tag a_5000_k10_traced --out "$O" &&
find "$T" -name '*kernel_stats.csv' -exec cp {} "${O%.json}_kernel_stats.csv" \;
