#!/bin/bash
# The host side of the front-end filter under the sanitizers (CPU only): tests/helpers/fir_check.c,
# a stand-alone program over gss_fir_host, gss_fir_check and gss_fir_make, built with the host
# sources with -fsanitize=address,undefined.  Any sanitizer report or failed check fails.  The log
# goes to $OUT (default profiles/fir).
set -o pipefail
cd "$(dirname "$0")/.."
OUT=${OUT:-profiles/fir}
mkdir -p $OUT
WORK=$(mktemp -d) || exit 1
trap 'rm -rf "$WORK"' EXIT
CF="-O1 -g -fno-omit-frame-pointer -ffp-contract=off -fno-fast-math -D_FILE_OFFSET_BITS=64 -Iinclude"
log=$OUT/sanitize_address.log
echo "== gcc -fsanitize=address,undefined, fir_check" > $log
gcc $CF -fsanitize=address,undefined -fno-sanitize-recover=all -o $WORK/fir_check \
    gps-sdr-sim_amd/csrc/host/*.c tests/helpers/fir_check.c -lm -lpthread || exit 1
ASAN_OPTIONS="detect_leaks=1 halt_on_error=1" UBSAN_OPTIONS="halt_on_error=1 print_stacktrace=1" \
    timeout -k 10 600 $WORK/fir_check >> $log 2>&1
r=$?
echo "exit $r" >> $log
grep -c "ERROR: AddressSanitizer\|runtime error\|LeakSanitizer" $log \
    | sed 's/^/sanitizer reports: /' >> $log
tail -3 $log
exit $r
