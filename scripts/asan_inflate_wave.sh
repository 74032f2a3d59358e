#!/bin/sh
# The host twin of the device DEFLATE decoder (npore_amd/csrc/inflate_wave.hpp) under AddressSanitizer and
# UndefinedBehaviorSanitizer on the whole test corpus: a stand-alone program, host code only (scripts/asan_inflate_wave.cpp).
# Run it on a CPU before the kernel of the same code goes to a GPU.  Needs the built library (the corpus marks the streams
# that csrc/inflate.hpp takes).  usage: scripts/asan_inflate_wave.sh [work directory]
set -e
here=$(cd "$(dirname "$0")/.." && pwd)
work=${1:-$(mktemp -d)}
mkdir -p "$work"
(cd "$here/tests" && PYTHONPATH="$here:$here/tests" python inflate_device_cases.py "$work/corpus.bin")
${CXX:-g++} -std=c++17 -O1 -g -fno-omit-frame-pointer -fsanitize=address,undefined -fno-sanitize-recover=undefined \
    -o "$work/asan_inflate_wave" "$here/scripts/asan_inflate_wave.cpp"
"$work/asan_inflate_wave" "$work/corpus.bin"
