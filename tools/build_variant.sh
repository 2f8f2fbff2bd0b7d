#!/bin/bash
# Build a library variant for tools/ab_libs.sh:  bash tools/build_variant.sh <tag> [source root] [-DNAME=VALUE ...]
# (source root: another checkout, e.g. a `git worktree add /tmp/base HEAD`, for the "before" of an A/B)
TAG=$1; shift
ROOT=$(cd "$(dirname "$0")/.." && pwd)
SRC=$ROOT
if [ -d "$1" ]; then SRC=$1; shift; fi
mkdir -p $ROOT/build_variants
python $ROOT/panagram_amd/build.py --out=$ROOT/build_variants/lib_$TAG.so --csrc=$SRC/panagram_amd/csrc "$@" && echo built $TAG
