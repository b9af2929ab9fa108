#!/bin/bash
# Build libxq_hip.so with THIS tree's csrc/xq_conv.hip and extra compiler flags into tests/microbench/lab/libxq_<name>.so
# (the working-tree counterpart of build_ref.sh; the other objects are the built tree's, so run `make -C csrc` first).
#     tests/microbench/build_tree.sh <name> [flags, e.g. -DXQ_EPI_ROUNDS=4]
set -e
HERE=$(cd "$(dirname "$0")" && pwd); ROOT=$HERE/../..; CSRC=$ROOT/xiangqi-alphazero_amd/csrc; LAB=$HERE/lab
NAME=$1; shift
mkdir -p $LAB; TMP=$(mktemp -d)
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -fPIC -std=c++17 -ffp-contract=off -fno-fast-math -w "$@" -I$CSRC -c $CSRC/xq_conv.hip -o $TMP/xq_conv.o
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o $LAB/libxq_$NAME.so $TMP/xq_conv.o $(ls $CSRC/*.o | grep -v xq_conv.o)
rm -rf $TMP
