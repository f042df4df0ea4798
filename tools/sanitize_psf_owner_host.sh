#!/bin/bash
# The host side of the path-space filter's owner (fermat_amd/csrc/fpt_host.h, PsfState) under AddressSanitizer + UBSan, as a stand-alone CPU program
# (tools/psf_owner_host_check.cpp).  Host code only: nothing runs on a GPU.
#   bash tools/sanitize_psf_owner_host.sh
set -e
cd "$(dirname "$0")/.."
O=tools/_build/sanitize; mkdir -p $O
${HIPCC:-hipcc} --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -x hip -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
    -Ifermat_amd/csrc -o $O/psf_owner_host_check tools/psf_owner_host_check.cpp
$O/psf_owner_host_check
