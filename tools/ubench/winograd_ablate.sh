#!/bin/bash
# Where do the cycles of a Winograd pipeline stage go?  Builds the library with s_memtime stamps (-DWG_STAMP, tools/lib_variants.sh) and
# prints the per-phase timeline of one CU (tools/ubench/winograd_stamps.py).  The timing ablations this script once looped over (no patch
# reads, no weight DMA / raw fetch inside the MFMA phase) were removed from the kernel; their numbers are in profiles/.
# WG_STAMP_SKIP skips that many marks first (3 per stage), WG_STAMP_TID picks the stamping lane (0 = wave 0, 256 = wave 4).
set -e
cd "$(dirname "$0")/../.."
tools/lib_variants.sh winograd "stamp:-DWG_STAMP -DWG_STAMP_TID=${WG_STAMP_TID:-0} -DWG_STAMP_SKIP=${WG_STAMP_SKIP:-194}"
WG_LIB=build/var_winograd/lib_stamp.so python tools/ubench/winograd_stamps.py --timeline 2>&1 | grep -E "phases|lifetime"
