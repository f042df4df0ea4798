"""The judge of the Metropolis renderers' chain shards (fpt_mlt_set_chain_shard): which global chains a rank owns, and the one-GPU state and counters
put together again from what the ranks hold.  numpy only; the map is the one of fermat_amd/csrc/fpt_mlt_host.h (mlt_shard_count, mlt_shard_global), written
independently: tools/mlt_shard_host_check.cpp prints the library's counts and tests/test_mlt_shard.py compares them with these."""
import numpy as np

# what a download holds per chain (the coordinates chain-minor, everything else chain-major) and what every rank holds a whole copy of
COORDS = ("light_u", "eye_u")
PER_CHAIN = ("path_value", "path_pdf", "rejections", "seeds", "st", "path_pixel")
REPLICATED = ("presample", "table", "table_pixel")
COUNTERS = ("accepted", "rejected", "swaps_proposed", "swaps_accepted", "rays")


def shard_globals(n_chains, rank, world):
    """the global chains of rank `rank` of `world`, in slot order: rank, rank + world, rank + 2 world, ... below n_chains"""
    return np.arange(rank, n_chains, world, dtype=np.int64)


def shard_count(n_chains, rank, world):
    return len(shard_globals(n_chains, rank, world))


def is_partition(n_chains, world):
    """do the ranks' shards cover [0, n_chains) once each, with counts within 1 of each other?"""
    parts = [shard_globals(n_chains, r, world) for r in range(world)]
    both = np.concatenate(parts)
    sizes = [len(p) for p in parts]
    return len(both) == n_chains and np.array_equal(np.sort(both), np.arange(n_chains)) and max(sizes) - min(sizes) <= 1 and sum(sizes) == n_chains


def assemble(states, n_chains):
    """the chain state of one GPU from the ranks' downloads (rank r's slot i is global chain r + i * world); a replicated array is taken from rank 0"""
    world = len(states)
    out = {}
    for k, v in states[0].items():
        if k in COORDS:
            full = np.zeros((v.shape[0], n_chains), v.dtype)
            for r, s in enumerate(states):
                g = shard_globals(n_chains, r, world)
                assert s[k].shape == (v.shape[0], len(g)), (k, r, s[k].shape, len(g))
                full[:, g] = s[k]
        elif k in PER_CHAIN:
            full = np.zeros((n_chains,) + v.shape[1:], v.dtype)
            for r, s in enumerate(states):
                g = shard_globals(n_chains, r, world)
                assert s[k].shape[0] == len(g), (k, r, s[k].shape, len(g))
                full[g] = s[k]
        else:
            assert k in REPLICATED, k
            full = v
        out[k] = full
    return out


def summed_counters(stats):
    """the ranks' counters added up (a `-pssmlt` context has the first two alone)"""
    return {k: sum(s[k] for s in stats) for k in COUNTERS if k in stats[0]}


def self_check():
    assert list(shard_globals(7, 0, 3)) == [0, 3, 6] and list(shard_globals(7, 1, 3)) == [1, 4] and list(shard_globals(7, 2, 3)) == [2, 5]
    assert [shard_count(200, r, 3) for r in range(3)] == [67, 67, 66]
    assert is_partition(7, 3) and is_partition(8, 8) and is_partition(200, 1)
    a = dict(light_u=np.array([[0., 2.]]), seeds=np.array([10, 12]), table=np.ones(3))
    b = dict(light_u=np.array([[1.]]), seeds=np.array([11]), table=np.ones(3))
    whole = assemble([a, b], 3)
    assert whole["light_u"].tolist() == [[0., 1., 2.]] and whole["seeds"].tolist() == [10, 11, 12] and whole["table"] is a["table"]
    assert summed_counters([dict(accepted=3, rejected=1), dict(accepted=2, rejected=0)]) == dict(accepted=5, rejected=1)
