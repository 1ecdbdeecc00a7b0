#!/bin/bash
# Development build: compile the library's translation units side by side, keeping the objects under /tmp/pobj so that
# only what changed is recompiled (pass the units to rebuild: gpu tesa rd rd_lo ...; default all), then link the normal
# library and, once every unit has a -DPCAMV_PROF object (--prof), that one (libpcamv_gpu_prof.so).
#   [EXTRA=<flags>] [OUT=<library>] tools/dbg/build_fast.sh [units...] [--prof]
set -e
cd "$(dirname "$0")/../../video-steganography-pcamv_amd"
ALL="gpu pass2_diag slice_write slice_write_cavlc tesa rd rd_lo rd_spec rd_spec2 rd_spec4 rd_tesa"        # csrc/pcamv_<unit>.hip: pcamv_amd/api.py UNITS
FLAGS="--offload-arch=gfx950 -O3 -ffp-contract=off -fPIC -std=c++17 -Wno-unused-value -Wno-unused-result"
UNITS=""; PROF=0
for a in "$@"; do if [ "$a" = "--prof" ]; then PROF=1; else UNITS="$UNITS $a"; fi; done
[ -z "$UNITS" ] && UNITS="$ALL"
mkdir -p /tmp/pobj
FLAGS="$FLAGS $EXTRA"        # e.g. EXTRA=-DPCAMV_RD_OCC=2
PIDS=""
for u in $UNITS; do
  hipcc $FLAGS -c -o /tmp/pobj/$u.o csrc/pcamv_$u.hip & PIDS="$PIDS $!"
  if [ $PROF = 1 ]; then hipcc $FLAGS -DPCAMV_PROF -c -o /tmp/pobj/${u}_prof.o csrc/pcamv_$u.hip & PIDS="$PIDS $!"; fi
done
for p in $PIDS; do wait $p || { echo "COMPILE FAILED"; exit 1; }; done
OBJS=""; POBJS=""; HAVE_PROF=1
for u in $ALL; do
  OBJS="$OBJS /tmp/pobj/$u.o"; POBJS="$POBJS /tmp/pobj/${u}_prof.o"
  [ -f /tmp/pobj/${u}_prof.o ] || HAVE_PROF=0
done
hipcc --offload-arch=gfx950 -fPIC -shared -o ${OUT:-libpcamv_gpu.so} $OBJS
[ $HAVE_PROF = 1 ] && hipcc --offload-arch=gfx950 -fPIC -shared -o libpcamv_gpu_prof.so $POBJS
ls -la *.so
