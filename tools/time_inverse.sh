#!/bin/bash
# A/B timing of the stand-alone r = 64 Gauss-Jordan inverse (tools/probe/time_inverse.hip): the tree's csrc/inverse_gj64.h against the header of another revision.
#   tools/time_inverse.sh build [REV = HEAD]   needs git and hipcc, no GPU: tools/probe/time_inverse_this and tools/probe/time_inverse_other
#   tools/time_inverse.sh run [ROUNDS = 5]     on the GPU: the two programs in turn, ROUNDS times each (200 launches after a warm-up of 50, medians);
#                                              the spread of one build's medians over the rounds is what a difference between the builds has to exceed
set -euo pipefail
here="$(cd "$(dirname "$0")" && pwd)"
root="$(dirname "$here")"
arch="${NMFAMD_OFFLOAD_ARCH:-gfx950}"
case "${1:-}" in
build)
	rev="${2:-HEAD}"
	tmp="$(mktemp -d)"
	trap 'rm -rf "$tmp"' EXIT
	git -C "$root" show "$rev:nmfgpu_amd/csrc/inverse_gj64.h" > "$tmp/inverse_gj64.h"
	flags=(--offload-arch="$arch" -O3 -std=c++17 -fno-slp-vectorize)
	hipcc "${flags[@]}" -I"$root/nmfgpu_amd/csrc" "$here/probe/time_inverse.hip" -o "$here/probe/time_inverse_this"
	hipcc "${flags[@]}" -I"$tmp" "$here/probe/time_inverse.hip" -o "$here/probe/time_inverse_other"
	echo "built $here/probe/time_inverse_this (tree) and $here/probe/time_inverse_other ($rev)"
	;;
run)
	rounds="${2:-5}"
	for ((i = 1; i <= rounds; ++i)); do
		for which in other this; do
			echo "round $i $which"
			timeout -k 10 60 "$here/probe/time_inverse_$which" 200 50
		done
	done
	;;
*)
	echo "usage: $0 build [REV] | run [ROUNDS]" >&2
	exit 2
	;;
esac
