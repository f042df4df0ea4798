"""worker of tests/test_mlt_shard.py::test_two_rank_rccl_shards_equal_single_gpu_frame (run under torch.distributed.run, one rank per GPU, backend nccl = RCCL):
every rank runs its shard of the Metropolis chains, fpt_mlt_finish all-reduces the splat sums and the counters over the library's communicator, and EVERY rank
compares its frame and its statistics with a single-GPU context of its own, bit for bit."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import torch
    import torch.distributed as dist
    import fermat_amd as fa
    from fermat_amd import api, scene
    from fermat_amd.distributed import comm_init, comm_info
    rank = int(os.environ["RANK"]); world = int(os.environ["WORLD_SIZE"]); local = int(os.environ["LOCAL_RANK"])
    torch.cuda.set_device(local)
    dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", local))
    s = scene.cornell_box("CornellBox-JP")
    res, L, n_chains = (24, 16), 6, 200

    def make():
        return fa.Renderer(s, res[0], res[1], fa.default_options(L), device=local,
                           mmlt_options=fa.default_mmlt_options(L, mmlt_frequency=2, lens_techniques=1, n_chains=n_chains, spp=4))
    r = make()
    comm_init(r, rank, world)
    assert comm_info(r) == (rank, world)
    r.mlt_set_chain_shard(rank, world)
    r.mlt_set_persistence(2, 1)
    full = make()
    full.mlt_set_persistence(2, 1)
    for i in range(4):          # two periods: a reseeding and a continuing call each
        r.mmlt_render(i)
        assert r.mlt_chain_shard()["pending"] == 1
        r.mlt_finish(sync=True)
        full.mmlt_render(i, sync=True)
        assert np.array_equal(r.framebuffer().view(np.uint32), full.framebuffer().view(np.uint32)), "instance %d: rank %d's frame differs from the single-GPU frame" % (i, rank)
        assert r.mmlt_stats() == full.mmlt_stats(), "instance %d: the reduced statistics differ" % i
        assert np.array_equal(r.mmlt_st_norms()[1], full.mmlt_st_norms()[1]), "instance %d: the reduced chains per technique differ" % i
    assert full.framebuffer()[api.FB_COMPOSITED_C][:, :3].max() > 0
    print("MLT_SHARD_OK world=%d" % world, flush=True)
    dist.barrier()
    r.close(); full.close()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
