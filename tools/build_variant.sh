#!/bin/bash
# Build an A/B variant of the library with extra compiler flags: [SRC=<file stem>] tools/build_variant.sh <name> <flags...>
#   -> open-solution-salt-identification_amd/csrc/_variants/libsaltnet_hip.<name>.so   (run with SALT_LIB=<that path>)
# SRC names the one source compiled with the flags (default conv_mfma: forward / data-gradient convolutions; conv_wgrad: the split-K
# weight-gradient kernels); the other objects come from csrc/_obj (build.py first).
# The source list is csrc/build.py's SOURCES.
set -e
cd "$(dirname "$0")/.."
name=$1; shift
SRC=${SRC:-conv_mfma}
C=open-solution-salt-identification_amd/csrc
mkdir -p $C/_variants/obj_$name
objs=""
for f in $(python -c "import sys; sys.path.insert(0, '$C'); import build; print(' '.join(s[:-4] for s in build.SOURCES))"); do
  if [ $f = $SRC ]; then
    /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -Iinclude -I$C -Wno-unused-value "$@" -c $C/$f.hip -o $C/_variants/obj_$name/$f.o
    objs="$objs $C/_variants/obj_$name/$f.o"
  else
    objs="$objs $C/_obj/$f.o"
  fi
done
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o $C/_variants/libsaltnet_hip.$name.so $objs
echo built $C/_variants/libsaltnet_hip.$name.so
