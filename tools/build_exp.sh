#!/bin/bash
# Experiment builds of libvqhip: tools/build_exp.sh <name> [-DMACRO=value ...]  ->  build/exp/libvqhip_<name>.so
# (git-ignored, but they travel to the GPU box; select one with VQHIP_LIB=build/exp/libvqhip_<name>.so)
# The same build as the shipped library (csrc/build.sh and its list of units), with the flags added to every compile and objects
# of its own under build/exp/obj_<name>/; a name built again with other flags is recompiled.
set -euo pipefail
ROOT="$(cd "$(dirname "${BASH_SOURCE[0]}")/.." && pwd)"
name=$1; shift
flags=""
if (( $# )); then flags="$(printf '%q ' "$@")"; fi      # each flag stays one word, spaces and quotes included
VQ_LIB_OUT="$ROOT/build/exp/libvqhip_$name.so" VQ_OBJ_DIR="$ROOT/build/exp/obj_$name" VQ_EXTRA_FLAGS="$flags" \
    bash "$ROOT/vector_quantization_amd/csrc/build.sh"
echo "built build/exp/libvqhip_$name.so ($*)"
