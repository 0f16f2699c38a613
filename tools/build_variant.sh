#!/bin/bash
# Build a side library for an experiment: spec_amd/libspec_amd_NAME.so with extra compiler flags
# (objects under spec_amd/csrc/build/v_NAME), then load it and precompile its Flat16 / Nested /
# pkg1-tree schema-specialised kernels into the shared jit_cache.  The runners that take variant
# names (tools/gpu_headline_ab.sh, gpu_wide_ab.sh, gpu_nenc_ab.sh, gpu_tree_ab.sh) swap it in.
# Usage: bash tools/build_variant.sh NAME "-DMY_EXPERIMENT=1 ..."
set -e
NAME=$1; FLAGS=$2
cd "$(dirname "$0")/.."
make -s -j8 -C spec_amd/csrc BUILD=build/v_$NAME OUT=../libspec_amd_$NAME.so \
  HIPFLAGS="-O3 -std=c++17 -fPIC --offload-arch=gfx950 -Wall -Wno-unused-function $FLAGS"
python3 - "$NAME" <<'PY'
import ctypes as C, sys
import spec_amd
from spec_amd import _lib
L = C.CDLL(_lib.LIB_PATH.replace("libspec_amd.so", f"libspec_amd_{sys.argv[1]}.so"))
_lib._declare(L)
L.spec_decode_flat_jit_compile(C.byref(spec_amd.FLAT16.c), 1 << 28, 1 << 20)
L.spec_encode_flat_jit_compile(C.byref(spec_amd.FLAT16.c))
L.spec_decode_nested_jit_compile(C.byref(spec_amd.NESTED.c))
L.spec_encode_nested_jit_compile(C.byref(spec_amd.NESTED.c))
print(L.spec_tree_jit_compile(C.byref(spec_amd.pkg1_tree().c)))
PY
echo built spec_amd/libspec_amd_$NAME.so
