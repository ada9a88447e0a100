#!/bin/bash
# The host side of observables and fixes under the sanitizers (CPU only): tests/helpers/
# pvt_check.c, a stand-alone program over gss_obs_host, the gss_navdata calls and gss_pvt_solve,
# built with the host sources once with -fsanitize=address,undefined and once with
# -fsanitize=thread.  Any sanitizer report or failed check fails.  Logs go to $OUT (default
# profiles/pvt).
set -o pipefail
cd "$(dirname "$0")/.."
OUT=${OUT:-profiles/pvt}
mkdir -p $OUT
WORK=$(mktemp -d) || exit 1
trap 'rm -rf "$WORK"' EXIT
CF="-O1 -g -fno-omit-frame-pointer -ffp-contract=off -fno-fast-math -D_FILE_OFFSET_BITS=64 -Iinclude"
rc=0
for san in address,undefined thread; do
    tag=${san%%,*}
    log=$OUT/sanitize_$tag.log
    echo "== gcc -fsanitize=$san, pvt_check" > $log
    gcc $CF -fsanitize=$san -fno-sanitize-recover=all -o $WORK/pvt_check_$tag \
        gps-sdr-sim_amd/csrc/host/*.c tests/helpers/pvt_check.c -lm -lpthread || exit 1
    TSAN_OPTIONS="halt_on_error=1" ASAN_OPTIONS="detect_leaks=1 halt_on_error=1" \
    UBSAN_OPTIONS="halt_on_error=1 print_stacktrace=1" \
        timeout -k 10 600 $WORK/pvt_check_$tag >> $log 2>&1
    r=$?
    echo "exit $r" >> $log
    grep -c "WARNING: ThreadSanitizer\|ERROR: AddressSanitizer\|runtime error\|LeakSanitizer" $log \
        | sed 's/^/sanitizer reports: /' >> $log
    tail -3 $log
    [ $r -eq 0 ] || rc=1
done
exit $rc
