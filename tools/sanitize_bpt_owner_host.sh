#!/bin/bash
# The host side of the bidirectional state's owner (fermat_amd/csrc/fpt_host.h, BptState) under AddressSanitizer + UBSan, as a stand-alone CPU program
# (tools/bpt_owner_host_check.cpp).  Host code only: nothing runs on a GPU.
#   bash tools/sanitize_bpt_owner_host.sh
set -e
cd "$(dirname "$0")/.."
O=tools/_build/sanitize; mkdir -p $O
${HIPCC:-hipcc} --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -x hip -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
    -Ifermat_amd/csrc -o $O/bpt_owner_host_check tools/bpt_owner_host_check.cpp
$O/bpt_owner_host_check
