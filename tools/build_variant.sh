#!/bin/bash
# usage: [SRC="file.hip ..."] tools/build_variant.sh <name> <extra hipcc flags...> -- builds spectrogram_rs_amd/ab/<name>.so with
# one kernel file (default stft4096_wg.hip), or the several SRC lists, recompiled under the extra flags (ablation / A-B builds).  A variant
# that issues add-TID LDS stores goes through the same ISA check as the product.
set -e
name=$1; shift
cd "$(dirname "$0")/../spectrogram_rs_amd/csrc"
make -s
mkdir -p ../ab build/ab
FLAGS="-O3 -std=c++17 -fPIC -fvisibility=hidden -ffp-contract=off -fno-slp-vectorize -Wall -Wno-unused-result --offload-arch=gfx950 -munsafe-fp-atomics"
objs=$(ls build/*.o)
for src in ${SRC:-stft4096_wg.hip}; do
    /opt/rocm/bin/hipcc $FLAGS "$@" -c $src -o build/ab/$name.$src.o
    /opt/rocm/bin/hipcc $FLAGS "$@" -S --cuda-device-only $src -o build/ab/$name.$src.s 2>/dev/null
    if grep -q addtid build/ab/$name.$src.s; then python3 ../../tools/isa_check_addtid.py build/ab/$name.$src.s; fi
    objs=$(printf '%s\n' $objs | grep -vx "build/$src.o"; echo build/ab/$name.$src.o)
done
/opt/rocm/bin/hipcc -shared -fPIC --offload-arch=gfx950 -munsafe-fp-atomics -o ../ab/$name.so $objs
echo built ../ab/$name.so
