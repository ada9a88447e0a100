#!/bin/bash
# The host side of tracking under the sanitizers (CPU only): tests/helpers/trk_check.c, a
# stand-alone program over gss_track_host, gss_nav_decode and gss_trk_cn0, built with the host
# sources once with -fsanitize=address,undefined and once with -fsanitize=thread.  Any sanitizer
# report or failed check fails.  Logs go to $OUT (default profiles/track).
set -o pipefail
cd "$(dirname "$0")/.."
OUT=${OUT:-profiles/track}
mkdir -p $OUT
WORK=$(mktemp -d) || exit 1
trap 'rm -rf "$WORK"' EXIT
CF="-O1 -g -fno-omit-frame-pointer -ffp-contract=off -fno-fast-math -D_FILE_OFFSET_BITS=64 -Iinclude"
rc=0
for san in address,undefined thread; do
    tag=${san%%,*}
    log=$OUT/sanitize_$tag.log
    echo "== gcc -fsanitize=$san, trk_check" > $log
    gcc $CF -fsanitize=$san -fno-sanitize-recover=all -o $WORK/trk_check_$tag \
        gps-sdr-sim_amd/csrc/host/*.c tests/helpers/trk_check.c -lm -lpthread || exit 1
    TSAN_OPTIONS="halt_on_error=1" ASAN_OPTIONS="detect_leaks=1 halt_on_error=1" \
    UBSAN_OPTIONS="halt_on_error=1 print_stacktrace=1" \
        timeout -k 10 600 $WORK/trk_check_$tag >> $log 2>&1
    r=$?
    echo "exit $r" >> $log
    grep -c "WARNING: ThreadSanitizer\|ERROR: AddressSanitizer\|runtime error\|LeakSanitizer" $log \
        | sed 's/^/sanitizer reports: /' >> $log
    tail -3 $log
    [ $r -eq 0 ] || rc=1
done
exit $rc
