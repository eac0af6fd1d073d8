#!/bin/sh
# Build the emulation of the kernels together with tests/cpp/backtrace_walk_san.cpp (its own main) under
# AddressSanitizer and UndefinedBehaviorSanitizer, and run it.  Host code only: no device is involved.
set -e
HERE="$(cd "$(dirname "$0")" && pwd)"
ROOT="$(cd "$HERE/../.." && pwd)"
OUT="${SAN_OUT:-$HERE/backtrace_walk_san}"
g++ -std=c++17 -O0 -fno-omit-frame-pointer -fsanitize=address,undefined -fno-sanitize-recover=undefined -DFLTX_EMU -ffp-contract=off \
    -Wno-unused-function -Wno-unknown-pragmas -Wno-return-type \
    -I"$ROOT/tests/emu" -I"$ROOT/include" -I"$ROOT/text_amd/csrc" \
    "$HERE/backtrace_walk_san.cpp" "$ROOT/text_amd/csrc/fltx_api.cpp" "$ROOT/text_amd/csrc/fltx_host_trie.cpp" \
    "$ROOT/text_amd/csrc/fltx_arpa.cpp" "$ROOT/text_amd/csrc/fltx_group.cpp" "$ROOT/tests/emu/hip_emu.cpp" \
    -o "$OUT" -lpthread
"$OUT"
