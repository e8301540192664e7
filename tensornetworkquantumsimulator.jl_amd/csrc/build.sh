#!/bin/bash
# Build libtnqs_hip.so for gfx950 (MI355X).  hipcc cross-compiles without a GPU.
# Sources: every *.hip and *.cpp of this directory, one object each, at most 16 compiles at a time; only their objects are linked.
set -e
cd "$(dirname "$0")"
OUT=../libtnqs_hip.so
FLAGS="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wall -Wno-unused-result ${EXTRA_FLAGS:-}"
mkdir -p build
# an object is stale when its source, any header here or the C ABI header is newer than it
stale() { local d; [ -f "$2" ] || return 0; for d in "$1" *.hpp ../../include/tnqs.h ../../include/tnqs_debug.h; do [ "$d" -nt "$2" ] && return 0; done; return 1; }
objs=(); pids=()
for f in *.hip *.cpp; do
  o=build/${f%.*}.o; objs+=("$o")
  if stale "$f" "$o"; then
    while [ "$(jobs -rp | wc -l)" -ge 16 ]; do sleep 0.1; done
    if [[ "$f" == *.hip ]]; then hipcc $FLAGS -c "$f" -o "$o" & else hipcc $FLAGS -x hip -c "$f" -o "$o" & fi
    pids+=($!)
  fi
done
for p in "${pids[@]}"; do wait $p; done
hipcc --offload-arch=gfx950 -shared -fPIC "${objs[@]}" -ldl -o $OUT
echo "built $OUT"
