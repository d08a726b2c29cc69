#!/bin/bash
# Register / spill / scratch / occupancy table of every kernel in the library (development aid; profiles/rNN_kernel_resources.txt)
#   tools/kernel_resources.sh [name-filter-regex] [extra hipcc flags...]
# The compile and the parser are the resource tests' (tests/kernel_resources.py).
ROOT=$(cd "$(dirname "$0")/.." && pwd)
exec python3 "$ROOT/tests/kernel_resources.py" "$@"
