#!/usr/bin/env bash
# Device-ISA identity check for refactors: compile every csrc/*.hip of a git revision and of the working tree to gfx950
# assembly with the product flags, normalise what may legitimately differ and diff: assembler comments, the per-build
# __hip_cuid_* symbol, and the name, linkage and data definition (not the uses) of the per-translation-unit zero page and
# noinline activation wrapper, which were global symbols under per-file names once.
# Instructions, .amdhsa_* directives and the kernel metadata (register counts, segment and kernarg sizes) are compared.
# The flags of a file are those csrc/Makefile gives it (`make flags F=<file>`: CXXFLAGS and the per-file extras such as
# -ffp-contract=off).  Both sides are compiled with the flags of the working tree's Makefile, so a revision is compared
# as the working tree would build it.
#   tools/isa_diff.sh [REV] [WORKDIR]     REV defaults to HEAD^; a WORKDIR is kept and its REV-side assembly reused.
# Prints one line per file; exit status 1 if any file differs (the diffs are left in WORKDIR/<file>.diff).
set -euo pipefail
REV=${1:-HEAD^}
ROOT=$(git -C "$(dirname "$0")" rev-parse --show-toplevel)
CSRC=image-restoration-models_amd/csrc
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
if [ $# -ge 2 ]; then WORK=$2; mkdir -p "$WORK"; else WORK=$(mktemp -d); trap 'rm -rf "$WORK"' EXIT; fi
mkdir -p "$WORK/old/src" "$WORK/new"
git -C "$ROOT" archive "$REV" "$CSRC" | tar -x -C "$WORK/old/src"

compile() {  # <source dir> <output dir>: one .s per .hip that has none yet
    (cd "$1" && ls *.hip | xargs -P "${JOBS:-8}" -I{} sh -c '
        [ -s "$1/{}.s" ] && exit 0
        "$0" $(make -s -C "$2" flags F={}) --cuda-device-only -Wno-unused-command-line-argument -S {} -o "$1/{}.s.tmp" && mv "$1/{}.s.tmp" "$1/{}.s"' \
        "$HIPCC" "$2" "$ROOT/$CSRC")
}
normalise() {
    sed -E -e 's/[[:space:]]*;.*$//' -e '/^[[:space:]]*$/d' -e 's/__hip_cuid_[0-9a-f]+/__hip_cuid/g' \
           -e 's/\b(_ZL13)?(dg|cf|ft|irm)_zero_page\b/irm_zero_page/g' \
           -e '/^[[:space:]]*\.(protected|addrsig_sym)[[:space:]]+irm_zero_page$/d' -e '/^[[:space:]]*\.type[[:space:]]+irm_zero_page,@object/,/^[[:space:]]*\.(size|comm)[[:space:]]+irm_zero_page,/d' -e '/^[[:space:]]*\.section[[:space:]]+\.(bss|rodata)/d' \
           -e 's/_ZL?[0-9]+(irm_act_slow|xr_act|irm_act_noinline)fi/irm_act_noinline/g' -e '/^[[:space:]]*\.(hidden|protected|globl|weak)[[:space:]]+irm_act_noinline$/d' "$1"
}
compile "$WORK/old/src/$CSRC" "$WORK/old"
rm -f "$WORK"/new/*.s
compile "$ROOT/$CSRC" "$WORK/new"

status=0
for s in "$WORK"/new/*.s; do
    f=$(basename "$s" .s)
    if [ ! -f "$WORK/old/$f.s" ]; then echo "$f: new file"; continue; fi
    kernels=$(grep -c '^[[:space:]]*\.amdhsa_kernel ' "$s" || true)
    if diff <(normalise "$WORK/old/$f.s") <(normalise "$s") > "$WORK/$f.diff"; then
        echo "$f: identical ($kernels kernels, $(normalise "$s" | wc -l) lines)"
    else
        echo "$f: DIFFERS ($(grep -c '^[<>]' "$WORK/$f.diff") lines)"; status=1
    fi
done
exit $status
