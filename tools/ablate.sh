#!/bin/bash
# Build ablation variants of libgsgpu.so into build/ablate/ (developer tool, build container):
#   tools/ablate.sh [bits ...] -> libgsgpu_a0.so (reference), _a1 (no per-read reduce), _a2 (no probe), _a3 (neither), _a7 (no gate), _a8 (no statistics atomics)
# then on the GPU box: python tools/stream_times.py build/ablate/libgsgpu_a*.so
# Every variant is the Makefile's unit list with -DGS_ABLATE=<bits>, built in a copy of the sources of its own (as tools/phase_times.sh does).
set -e
cd "$(dirname "$0")/.."
mkdir -p build/ablate
for a in ${@:-0 1 2 3 7}; do
    t=build/ablate/src_a$a
    rm -rf $t && mkdir -p $t
    cp -r genestrip_amd include $t/
    make -s -C $t/genestrip_amd/csrc clean >/dev/null 2>&1 || true
    make -s -j8 -C $t/genestrip_amd/csrc CXXFLAGS="-O3 -std=c++17 -fPIC -Wall -Wno-unused-function -Wno-unused-result -Wno-unused-value -DGS_ABLATE=$a" ../libgsgpu.so
    cp $t/genestrip_amd/libgsgpu.so build/ablate/libgsgpu_a$a.so
    rm -rf $t
done
ls -la build/ablate
