#!/usr/bin/env bash
# AddressSanitizer + UBSan over the host side of conditional aggregate arguments (csrc/planvalue_rules.h, csrc/planvalue_expr.cpp):
# builds the stand-alone program tools/planvalue_rules_check.cpp (its own main, no GPU, no Python) and runs it.
# Exit status 0: clean and every pinned row matched.
#   tools/sanitize_planvalue.sh
set -euo pipefail
ROOT="$(cd "$(dirname "$0")/.." && pwd)"
OUT="${TMPDIR:-/tmp}/llkv_asan"
mkdir -p "$OUT"
"${CXX:-g++}" -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer -Wno-unknown-pragmas \
    -I"$ROOT/include" -I"$ROOT/rust-llkv_amd/csrc" "$ROOT/tools/planvalue_rules_check.cpp" "$ROOT/rust-llkv_amd/csrc/planvalue_expr.cpp" -o "$OUT/planvalue_rules_check"
"$OUT/planvalue_rules_check"
