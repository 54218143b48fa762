#!/bin/bash
# Build libvqhip.so for gfx950 in-tree (hipcc cross-compiles without a GPU): one object per translation unit under build/obj/,
# compiled in parallel and linked (csrc/Makefile holds the list of units).  A later run recompiles only the stale units.
# Parallelism: MAX_JOBS, else CMAKE_BUILD_PARALLEL_LEVEL, capped at 16, else 16 — never the machine's core count; make starts no
# more jobs than there are units.
# VQ_KEEP_TEMPS=1 keeps the device assembly, one *gfx950.s per unit, under build/asm/ instead — and leaves the shipped library alone:
# the same sources built with -save-temps from another directory come out with another __hip_cuid (another sha256 of the file, same
# code), and bench.py reports the PMC traffic of profiles/pmc_latest.json only for the sha256 it was collected with.
# Experiment builds (tools/build_exp.sh): VQ_LIB_OUT names the library, VQ_OBJ_DIR its objects, VQ_EXTRA_FLAGS is added to every compile
# (shell-quoted words: the compile command's shell splits them again).
set -euo pipefail
HERE="$(cd "$(dirname "${BASH_SOURCE[0]}")" && pwd)"
ROOT="$(cd "$HERE/../.." && pwd)"
OUT="${VQ_LIB_OUT:-$HERE/../libvqhip.so}"
OBJDIR="${VQ_OBJ_DIR:-$ROOT/build/obj}"
EXTRA="${VQ_EXTRA_FLAGS:-}"
if [[ "${VQ_KEEP_TEMPS:-0}" == "1" ]]; then
    OBJDIR="$ROOT/build/asm"
    OUT="$OBJDIR/libvqhip_temps.so"
    EXTRA="$EXTRA -save-temps=obj"
fi
JOBS="${MAX_JOBS:-${CMAKE_BUILD_PARALLEL_LEVEL:-16}}"
if ! [[ "$JOBS" =~ ^[0-9]+$ ]] || (( JOBS < 1 || JOBS > 16 )); then JOBS=16; fi
mkdir -p "$OBJDIR" "$(dirname "$OUT")"
make -f "$HERE/Makefile" -j"$JOBS" HIPCC="${HIPCC:-/opt/rocm/bin/hipcc}" OUT="$OUT" OBJDIR="$OBJDIR" EXTRA="$EXTRA"
echo "built $OUT"
