#!/bin/bash
# Tuning build of the wave-per-chain sampler kernels: compile bfhip_sampler.hip with extra -D flags and link it with the
# other objects (the Makefile's SRCS, built by make) into bayesfast_amd/variants/libbfhip_s_<name>.so.  Select it with
# BFHIP_LIBRARY=<path>.  E.g. the unpacked form of the wave reductions next to the default: tools/svariant.sh unpacked -DBF_WSUM_UNPACKED;
# the U-turn tests that read every sum (the form before any_le0): tools/svariant.sh readall -DBF_UTURN_READ_ALL
# usage: tools/svariant.sh <name> [-DFLAG=..]...
set -e
name=$1; shift
root=$(cd "$(dirname "$0")/.." && pwd)
cd "$root/bayesfast_amd/csrc"
mkdir -p _obj ../variants
/opt/rocm/bin/hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -Wno-unused-function -Wno-unused-variable "$@" -c bfhip_sampler.hip -o _obj/bfhip_sampler_$name.o
objs=$(sed -n 's/^SRCS := //p' Makefile | tr ' ' '\n' | sed -e "s/^bfhip_sampler\.hip$/bfhip_sampler_$name.hip/" -e 's/^\(.*\)\.hip$/_obj\/\1.o/')
/opt/rocm/bin/hipcc -shared -fPIC --offload-arch=gfx950 -o ../variants/libbfhip_s_$name.so $objs
echo built bayesfast_amd/variants/libbfhip_s_$name.so
