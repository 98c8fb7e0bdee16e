#!/bin/bash
# AddressSanitizer / UBSan on the CPU-side code (GPU ASan is not available on this pool): the C++ host mirror
# (grid, handler, connectivity, sparsity, flatten) and the planner of the C ABI (pdh_plan.cpp: validation + repacking, the choice
# of the row kernel and its tables, through the pdh_check_* entry points).  The planner is plain C++: g++ builds it with the same
# flags as the host mirror, no HIP object is linked and nothing is stubbed.  Usage: tools/run_sanitizers.sh
set -eo pipefail
cd "$(dirname "$0")/.."
OUT=build/asan
mkdir -p $OUT
SAN="-std=c++17 -O1 -g -fsanitize=address,undefined -fno-omit-frame-pointer"
g++ $SAN tools/sanitize/host_asan.cpp -o $OUT/host_asan
$OUT/host_asan
PLAN="-I include -I polydeal_amd/csrc polydeal_amd/csrc/pdh_plan.cpp"
g++ $SAN $PLAN tools/sanitize/capi_asan.cpp -pthread -o $OUT/capi_asan
ASAN_OPTIONS=detect_leaks=0 UBSAN_OPTIONS=halt_on_error=1 $OUT/capi_asan
# the planner's whole output on a fixed list of descriptions (tests/test_plan_fingerprint.py compares it with the recorded text)
g++ $SAN -ffp-contract=off $PLAN tools/sanitize/plan_fingerprint.cpp -pthread -o $OUT/plan_fingerprint
ASAN_OPTIONS=detect_leaks=0 UBSAN_OPTIONS=halt_on_error=1 $OUT/plan_fingerprint | cmp - tests/data/plan_fingerprint.txt
echo "sanitizers: clean"
