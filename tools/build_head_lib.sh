#!/bin/bash
# A/B helper: build libfacevae.so from the committed sources of a revision (default HEAD) into
# abl/libfacevae_<tag>.so.  The revision's face-vae_amd/csrc and include are checked out into a
# temporary directory and built there with that revision's own build.py (so python must be on
# PATH, as for every build of the library); the working tree and its objects are not touched.
# Select the result with FV_LIB_PATH.
#   bash tools/build_head_lib.sh [rev] [tag]      e.g.  bash tools/build_head_lib.sh HEAD~1 parent
# (The former third argument, one source file to rebuild at the revision and link against this
# tree's other objects, is gone: the convolution's files share internal declarations, so only a
# whole revision builds.)
set -e -o pipefail
REV=${1:-HEAD}; TAG=${2:-head}
[ $# -le 2 ] || { echo "usage: $0 [rev] [tag]" >&2; exit 2; }
cd "$(dirname "$0")/.."
TMP=$(mktemp -d)
trap 'rm -rf "$TMP"' EXIT
git archive "$REV" face-vae_amd/csrc include | tar -x -C "$TMP"
python "$TMP/face-vae_amd/csrc/build.py" --force
mkdir -p abl
cp "$TMP/face-vae_amd/libfacevae.so" "abl/libfacevae_$TAG.so"
echo "built abl/libfacevae_$TAG.so from $REV"
