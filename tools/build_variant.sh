#!/bin/bash
# Build a variant of the library for same-box A/B runs (tools/ab.sh):
#   tools/build_variant.sh <name> [--unit main|rays|split|bvh|film] [extra hipcc flags, e.g. -DPT_BOUNCE_WAVES_LDS=7]   ->  pathtrace_amd/libpt_<name>.so
# The kernel units are recompiled by the Makefile's own rules, each with its own options plus the extra flags (--unit: only that
# unit, the others are the regular build's objects); the host objects of the regular build are reused.
set -eu
name=${1:?usage: tools/build_variant.sh <name> [--unit main|rays|split|bvh|film] [flags]}; shift
case "$name" in */*|.*|"") echo "bad name: $name" >&2; exit 2;; esac
unit=""
if [ "${1:-}" = "--unit" ]; then unit=${2:?--unit main|rays|split|bvh|film}; shift 2; fi
cd "$(dirname "$0")/../pathtrace_amd/csrc"
make -j6 >/dev/null
tmp=/tmp/ptvar_$name
rm -rf "$tmp"; mkdir -p "$tmp"
if [ -n "$unit" ]; then
  ls pt_kernels_${unit}*.o >/dev/null      # (an unknown unit ends here)
  for o in pt_kernels_*.o; do case "$o" in pt_kernels_${unit}*) ;; *) cp "$o" "$tmp/";; esac; done
fi
make -j6 KOBJ="$tmp/" KDEFS="$*" OUT=../libpt_$name.so >/dev/null
echo "built pathtrace_amd/libpt_$name.so"
