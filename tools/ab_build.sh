#!/bin/bash
# Build A/B variants of libbsdfd.so into build_ab/ (travels to the GPU box, git-ignored):
#   tools/ab_build.sh NAME "EXTRA HIPCC FLAGS" [NAME2 "FLAGS2" ...]
# csrc/bsdfd.hip and csrc/host.hip are rebuilt per variant (the kernel's knobs in the one, run()'s — BSDFD_T32_RESIDENT_MIN_T, tools/tuning_knobs.h — in the other);
set -e
ROOT="$(cd "$(dirname "$0")/.." && pwd)"
OUT="$ROOT/build_ab"; mkdir -p "$OUT"
CS="$ROOT/bsdf_diffusion_sampling_amd/csrc"
COMMON="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wno-unused-value -Wno-pass-failed -I $ROOT/include"
SIDE="$(cd "$ROOT" && python -c "import os; from bsdf_diffusion_sampling_amd import _lib; print(' '.join(s for s in (os.path.basename(p)[:-4] for p in _lib.SRC_PATHS) if s not in 'bsdfd host'.split()))")"   # ... the library's other translation units once
for tu in $SIDE; do
  if [ ! -f "$OUT/$tu.o" ] || [ "$CS/$tu.hip" -nt "$OUT/$tu.o" ] || [ "$CS/flow_dev.h" -nt "$OUT/$tu.o" ] || [ "$CS/flow_kernels.h" -nt "$OUT/$tu.o" ] || [ "$ROOT/include/bsdfd.h" -nt "$OUT/$tu.o" ]; then
    hipcc $COMMON -c "$CS/$tu.hip" -o "$OUT/$tu.o" &
    if (( $(jobs -r | wc -l) >= 8 )); then wait -n; fi
  fi
done
wait
while [ $# -gt 0 ]; do
  name="$1"; flags="$2"; shift 2
  ( hipcc $COMMON $flags -c "$CS/bsdfd.hip" -o "$OUT/bsdfd_$name.o" && hipcc $COMMON $flags -c "$CS/host.hip" -o "$OUT/host_$name.o" && \
    hipcc --offload-arch=gfx950 -shared -fPIC "$OUT/bsdfd_$name.o" "$OUT/host_$name.o" $(for tu in $SIDE; do echo "$OUT/$tu.o"; done) -o "$OUT/lib_$name.so" && echo "built $name ($flags)" ) &
  if (( $(jobs -r | wc -l) >= 4 )); then wait -n; fi
done
wait
