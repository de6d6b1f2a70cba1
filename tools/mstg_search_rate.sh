#!/bin/bash
# tools/mstg_search_rate.sh : the records profiles/mstg_search_rate_<shape>.json (tools/mstg_search_rate.py); every GPU step under
# a time limit of its own, nothing started after a failure
cd "$(dirname "$0")/.."
timeout -k 10 900 python tools/mstg_search_rate.py --shape lists1k --out profiles/mstg_search_rate_lists1k.json &&
timeout -k 10 900 python tools/mstg_search_rate.py --shape lists60k --out profiles/mstg_search_rate_lists60k.json
