#!/bin/bash
# A/B builds of fused units with experiment macros:
#   scripts/build_variant.sh <name> "<-D flags>" [unit ...]   -> nerfsafetyvalidation_amd/libngp_hip_<name>.so
# rebuilds the named units of csrc/ (default: render_fused; e.g. render_uniform fused_query) with the flags and links them with
# the other objects of the last `make`.  Select at run time with NGP_HIP_LIB=$PWD/nerfsafetyvalidation_amd/libngp_hip_<name>.so
set -e
cd "$(dirname "$0")/../nerfsafetyvalidation_amd/csrc"
name=$1; flags=$2; shift 2 || { echo "usage: $0 <name> \"<-D flags>\" [unit ...]" >&2; exit 2; }
units=${@:-render_fused}
objs=$(ls *.o)
for u in $units; do
    /opt/rocm/bin/hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -ffp-contract=off -fvisibility=hidden -Wall -Wno-unused-function -DNGP_BUILD $flags -c $u.hip -o /tmp/${u}_$name.o
    objs="$(echo "$objs" | grep -vx $u.o) /tmp/${u}_$name.o"
done
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o ../libngp_hip_$name.so $objs
echo built ../libngp_hip_$name.so
