#!/bin/bash
# Diagnostic build of the library with k_sytrd_resident's per-segment stamps (-DRES_STAMPS) next to the product library, by
# the product's own build:  bash tools/build_res_stamps_lib.sh  ->  springcraft_amd/libspringcraft_hip_res_stamps.so
# (git-ignored; select it with SPRINGCRAFT_HIP_LIB=...; tools/resident_check.py --stamps uses it)
SC_LIB_SUFFIX=_res_stamps SC_EXTRA_HIPCC_FLAGS=-DRES_STAMPS python "$(dirname "$0")/../springcraft_amd/csrc/build.py" --force
