#!/bin/bash
# A library variant that differs in pg_deflate.hip only (defines on the command line), linked with the objects of the last
# `python panagram_amd/build.py` (seconds instead of minutes):  bash tools/build_deflate_variant.sh <tag> [-DNAME=VALUE ...]
TAG=$1; shift
ROOT=$(cd "$(dirname "$0")/.." && pwd)
mkdir -p $ROOT/build_variants
python $ROOT/panagram_amd/build.py --out=$ROOT/build_variants/lib_$TAG.so --only=pg_deflate.hip "$@" && echo built $TAG
