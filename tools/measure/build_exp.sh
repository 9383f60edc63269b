#!/bin/bash
# Experimental build of the library with one source compiled with extra defines: build/exp_<name>/libqoi_mi355x.so
# usage: tools/measure/build_exp.sh <name> <enc|dec|host|any source's name without .hip> <flags...>      (the other objects come from qoi_amd/lib/obj: run make first)
set -e
R="$(cd "$(dirname "$0")/../.." && pwd)"; name=$1; what=$2; shift 2
case $what in enc) src=qoi_encode;; dec) src=qoi_decode;; host) src=qoi_host;; *) src=$what; [ -f "$R/qoi_amd/csrc/$src.hip" ] || { echo "enc|dec|host|<source>"; exit 2; };; esac
mkdir -p "$R/build/exp_$name"
hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -Wno-unused-function -Wno-int-to-pointer-cast "$@" -c "$R/qoi_amd/csrc/$src.hip" -o "$R/build/exp_$name/$src.o"
objs=""; for f in "$R"/qoi_amd/csrc/*.hip; do o=$(basename "$f" .hip)   # (every .hip there is a translation unit: sources.mk)
  if [ $o = $src ]; then objs="$objs $R/build/exp_$name/$o.o"; else objs="$objs $R/qoi_amd/lib/obj/$o.o"; fi; done
hipcc --offload-arch=gfx950 -shared -fPIC -o "$R/build/exp_$name/libqoi_mi355x.so" $objs
echo "built build/exp_$name/libqoi_mi355x.so"
