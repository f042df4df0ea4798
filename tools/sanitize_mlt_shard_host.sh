#!/bin/bash
# The host side of the Metropolis renderers' chain shards (fermat_amd/csrc/fpt_mlt_host.h, MltState in fermat_amd/csrc/fpt_host.h, the three entry points) under
# AddressSanitizer + UBSan, as a stand-alone CPU program (tools/mlt_shard_host_check.cpp) linked with the built library.  Host code only: nothing runs on a GPU.
#   bash tools/sanitize_mlt_shard_host.sh
set -e
cd "$(dirname "$0")/.."
O=tools/_build/sanitize; mkdir -p $O
${HIPCC:-hipcc} --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -x hip -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
    -Ifermat_amd/csrc -o $O/mlt_shard_host_check tools/mlt_shard_host_check.cpp -Lfermat_amd -lfermat_pt_hip -Wl,-rpath,"$PWD/fermat_amd"
$O/mlt_shard_host_check
