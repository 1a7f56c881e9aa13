#!/bin/bash
# dev helper: builds a variant of the engine into meltingpot_amd/lib/libmp_engine_<tag>.so
# usage: tools/ab_build.sh <tag> [-DFLAG ...]
# (every unit of the product build, meltingpot_amd/_build.py: SOURCES, in one hipcc call)
cd "$(dirname "$0")/.."; tag=$1; shift
sources=$(python3 -c "from meltingpot_amd import _build; print(' '.join('meltingpot_amd/csrc/' + s for s in _build.SOURCES))") || exit 1
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -shared -fPIC -fvisibility=hidden "$@" \
  -Wl,--version-script=meltingpot_amd/csrc/exports.map -o meltingpot_amd/lib/libmp_engine_$tag.so $sources && \
  rm -f meltingpot_amd/lib/*.hipv4* meltingpot_amd/lib/*host-x86* meltingpot_amd/lib/*.hipfb && ls -la meltingpot_amd/lib/
