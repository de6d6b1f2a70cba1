#!/bin/bash
# tools/mstg_build_rate.sh [OUT.json] : the three legs of tools/mstg_build_rate.py, each GPU step under its own time limit,
# chained so that nothing starts after a failure; the record is merged into OUT (default profiles/mstg_build_rate_1m_d960.json)
set -o pipefail
cd "$(dirname "$0")/.."
O=${1:-profiles/mstg_build_rate_1m_d960.json}
rm -f "$O"
timeout -k 10 300 python tools/mstg_build_rate.py --legs closure --out "$O" &&
timeout -k 10 300 python tools/mstg_build_rate.py --legs build --out "$O" &&
timeout -k 10 600 python tools/mstg_build_rate.py --legs cpu --out "$O"
