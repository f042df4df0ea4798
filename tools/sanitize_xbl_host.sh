#!/bin/bash
# The host side of the XBL filter's entry points (the -filter option, fpt_xbl's argument checks, FPT_XBL_LAYOUT) under AddressSanitizer + UBSan, as a stand-alone CPU
# program (tools/xbl_host_check.cpp).  Host code only: nothing runs on a GPU.
#   bash tools/sanitize_xbl_host.sh
set -e
cd "$(dirname "$0")/.."
O=tools/_build/sanitize; mkdir -p $O
${HIPCC:-hipcc} --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -x hip -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
    -Ifermat_amd/csrc -o $O/xbl_host_check tools/xbl_host_check.cpp
$O/xbl_host_check
