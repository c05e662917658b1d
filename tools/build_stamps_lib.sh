#!/bin/bash
# Diagnostic build of the whole library next to the product library, by the product's own build (csrc/build.py):
#   bash tools/build_stamps_lib.sh [flags]  ->  springcraft_amd/libspringcraft_hip_stamps.so   (git-ignored; select it with
#   SPRINGCRAFT_HIP_LIB=...).  Flags: -DPAIR_STAMPS (the default; tools/pair_stamps.py), -DCHASE_STAMPS (chase_stamps.py),
#   -DBULGE_STAMPS (bulge_stamps.py), -DBT2_STAMPS (bt2_stamps.py), -DBT2_CLOCK (bt2_clock.py), -DBT2_TRACE (bt2_trace.py)
SC_LIB_SUFFIX=_stamps SC_EXTRA_HIPCC_FLAGS="${*:--DPAIR_STAMPS}" python "$(dirname "$0")/../springcraft_amd/csrc/build.py" --force
