#!/bin/bash
# The host side of the owners every render call passes through (fermat_amd/csrc/fpt_host.h: RenderLanes, DeferredRun, LaunchTimer, merged_length) under
# AddressSanitizer + UBSan, as a stand-alone CPU program (tools/render_state_host_check.cpp).  Host code only: nothing runs on a GPU.
#   bash tools/sanitize_render_state_host.sh
set -e
cd "$(dirname "$0")/.."
O=tools/_build/sanitize; mkdir -p $O
${HIPCC:-hipcc} --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -x hip -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
    -Ifermat_amd/csrc -o $O/render_state_host_check tools/render_state_host_check.cpp
$O/render_state_host_check
