#!/usr/bin/env bash
# AddressSanitizer + UBSan over the host side of HAVING (csrc/having.cpp, csrc/having_rules.h): builds the stand-alone program
# tools/having_expr_check.cpp (its own main, no GPU, no Python) and runs its edge table.  Exit status 0: clean and every row matched.
#   tools/sanitize_having.sh
set -euo pipefail
ROOT="$(cd "$(dirname "$0")/.." && pwd)"
OUT="${TMPDIR:-/tmp}/llkv_asan"
mkdir -p "$OUT"
"${HIPCC:-/opt/rocm/bin/hipcc}" -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer \
    -I"$ROOT/include" -I"$ROOT/rust-llkv_amd/csrc" "$ROOT/tools/having_expr_check.cpp" "$ROOT/rust-llkv_amd/csrc/having.cpp" -o "$OUT/having_expr_check"
"$OUT/having_expr_check"
