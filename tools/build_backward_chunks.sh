#!/bin/bash
# Variants of libscone_hip.so that differ only in the backward's chunk length C (scone_backward_chunk), for
# tools/backward_compare.py:  build/bwd_chunks/libbwd_c<C>.so for C in 64 128 256 512 (git-ignored).  Only scone_backward.hip is
# recompiled; the other objects are the in-tree ones (run `make -C scone_amd/csrc` first).
set -eu
R=$(cd "$(dirname "$0")/.." && pwd)
C=$R/scone_amd/csrc
B=$R/build/bwd_chunks
mkdir -p "$B"
FLAGS="-O3 -std=c++17 -fPIC --offload-arch=gfx950 -ffp-contract=off -Wall -Wno-unused-function -Wno-pass-failed"
OBJS=$(ls "$C"/*.o | grep -v scone_backward.o)
for n in 64 128 256 512; do
  ( cd "$C" && hipcc $FLAGS -DSCONE_BWD_CHUNK=$n -c scone_backward.hip -o "$B/scone_backward_c$n.o" ) &
done
wait
for n in 64 128 256 512; do
  hipcc -shared --offload-arch=gfx950 -o "$B/libbwd_c$n.so" $OBJS "$B/scone_backward_c$n.o"
  echo "built build/bwd_chunks/libbwd_c$n.so"
done
