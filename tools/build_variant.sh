#!/bin/bash
# tools/build_variant.sh NAME "-DFLAG=..."  ->  tools/build/libvitssl_NAME.so  (kernel A/B builds; use with VITSSL_LIB=...)
# The file list, the common flags and the per-file flags are those of __graft_entry__.py (SOURCES, FLAGS, PER_FILE_FLAGS).
set -e
ROOT="$(cd "$(dirname "$0")/.." && pwd)"
OUT="$ROOT/tools/build"; mkdir -p "$OUT/$1"
# CSRC_DIR: sources of another commit (git archive <rev> __graft_entry__.py vit-ssl_amd/csrc include | tar -x -C <dir>, then
# CSRC_DIR=<dir>/vit-ssl_amd/csrc).  That commit's own __graft_entry__.py is read if it was extracted too, else this tree's.
CS="${CSRC_DIR:-$ROOT/vit-ssl_amd/csrc}"
GE="$(cd "$CS/../.." && pwd)"; [ -f "$GE/__graft_entry__.py" ] || GE="$ROOT"
list="$(cd "$GE" && python3 -c '
import __graft_entry__ as ge
print(ge.HIPCC, *ge.FLAGS)
for s in ge.SOURCES:
    print(s, *ge.PER_FILE_FLAGS.get(s, []))')"
cc="$(head -n 1 <<< "$list")"
objs=()
while read -r f extra; do
  [ -f "$CS/$f" ] || continue     # sources of an older commit may lack a file
  $cc $2 $extra -x hip -c "$CS/$f" -o "$OUT/$1/$f.o" &
  objs+=("$OUT/$1/$f.o")
done < <(tail -n +2 <<< "$list")
wait
${cc%% *} --offload-arch=gfx950 -shared -fPIC -o "$OUT/libvitssl_$1.so" "${objs[@]}"
echo "built $OUT/libvitssl_$1.so"
