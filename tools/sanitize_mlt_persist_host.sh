#!/bin/bash
# The host-only helpers of the Metropolis renderers' persistent chains (fermat_amd/csrc/fpt_mlt_host.h) under AddressSanitizer + UBSan, as a stand-alone CPU program
# (tools/mlt_persist_host_check.cpp).  Host code only: nothing runs on a GPU.
#   bash tools/sanitize_mlt_persist_host.sh
set -e
cd "$(dirname "$0")/.."
O=tools/_build/sanitize; mkdir -p $O
${HIPCC:-hipcc} --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -x hip -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
    -Ifermat_amd/csrc -o $O/mlt_persist_host_check tools/mlt_persist_host_check.cpp
$O/mlt_persist_host_check
