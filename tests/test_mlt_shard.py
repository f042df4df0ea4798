"""Chain shards (fpt_mlt_set_chain_shard / fpt_mlt_get_chain_shard / fpt_mlt_finish): the Metropolis renderers on N ranks give the frame of one GPU bit
for bit, because a chain is independent of the others, its mutation numbers are a function of its GLOBAL id and its deposits are integer sums.  That makes the claim
testable on one GPU: N contexts, one per rank, plus a reference context that runs every chain; the test is the "wire" (it adds the ranks' splat buffers in torch).
Every comparison is exact.

Shapes (CornellBox-JP, those of tests/test_mlt_persistence.py): A = 32 x 32, max_path_length 4, 256 chains, 4 spp (16 steps per call); B = 24 x 16, max_path_length 6,
200 chains, 4 spp (7 steps per call; 200 chains over 3 ranks are 67 / 67 / 66).  Modes: `-pssmlt`, `-mmlt` without swaps, `-mmlt` with a swap every 2nd step, and
`-mmlt` with its lens techniques and a swap every 2nd step."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mlt_shard_truth as S  # noqa: E402

import fermat_amd as fa  # noqa: E402
from fermat_amd import api  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U32 = np.uint32
SHAPES = {"A": dict(res=(32, 32), L=4, n_chains=256, spp=4), "B": dict(res=(24, 16), L=6, n_chains=200, spp=4)}
MODES = [("pssmlt", 0), ("mmlt", 0), ("mmlt", 2), ("lens", 2)]
MODE_IDS = ["pssmlt", "mmlt-F0", "mmlt-F2", "lens-F2"]
NAMES = ("fpt_mlt_set_chain_shard", "fpt_mlt_get_chain_shard", "fpt_mlt_finish")


def bits(a):
    return np.ascontiguousarray(a).view(U32)


# ---- CPU ----------------------------------------------------------------------------------------------------------------------------------------------------
def test_entry_points_declared_exported_wrapped_and_header_is_c99(tmp_path):
    """the three entry points are declared in the header, exported by the library and wrapped in Python; the header still compiles as C99 -pedantic"""
    text = open(os.path.join(ROOT, "include", "fermat_pt_hip.h")).read()
    lib = fa.lib()
    for n in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % n, text), "not declared: " + n
        assert n in api.ENTRY_POINTS and hasattr(lib, n), "not exported: " + n
    for m in ("mlt_set_chain_shard", "mlt_chain_shard", "mlt_finish", "mlt_splat_buffer"):
        assert callable(getattr(fa.Renderer, m))
    src = tmp_path / "header.c"
    src.write_text('#include "fermat_pt_hip.h"\nint main(void) { return fpt_mlt_finish(0, 0) == 0 && fpt_mlt_set_chain_shard(0, 0u, 1u) == 0; }\n')
    run = subprocess.run(["cc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr[-2000:]


def test_the_judges_shard_map_is_a_partition():
    """the judge on its own, and its map: for W in 1..9 the ranks' shards cover [0, n_chains) once each with counts within 1 of each other -- n_chains a multiple of
    W, not a multiple of W, and W == n_chains"""
    S.self_check()
    for world in range(1, 10):
        for n in sorted({world, world + 1, 2 * world, 7 * world + 3, 200, 256, 257}):
            assert S.is_partition(n, world), (n, world)
            assert [S.shard_count(n, r, world) for r in range(world)] == [(n - r + world - 1) // world for r in range(world)]
            for r in range(world):
                g = S.shard_globals(n, r, world)
                assert np.array_equal(g, r + np.arange(len(g)) * world) and (len(g) == 0 or g[-1] < n <= g[-1] + world)
        assert [S.shard_count(world, r, world) for r in range(world)] == [1] * world


def test_shard_host_helpers_under_sanitizers_agree_with_the_judge():
    """the stand-alone program over the host helpers (the partition for W in 1..9, every refusal string, MltState's reset, the three calls with no context), built
    with -fsanitize=address,undefined for the host and run here; the counts it prints are the judge's"""
    run = subprocess.run(["bash", os.path.join(ROOT, "tools", "sanitize_mlt_shard_host.sh")], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, (run.stdout + run.stderr)[-3000:]
    assert "all checks passed" in run.stdout and "chain shard" in run.stdout, run.stdout[-2000:]
    lines = re.findall(r"^shard n=(\d+) W=(\d+) counts=([\d,]+)$", run.stdout, re.M)
    assert len(lines) >= 50 and ("200", "3", "67,67,66") in lines
    for n, world, counts in lines:
        assert [int(c) for c in counts.split(",")] == [S.shard_count(int(n), r, int(world)) for r in range(int(world))], (n, world, counts)


# ---- GPU ----------------------------------------------------------------------------------------------------------------------------------------------------
def make(cornell, table, kind, shape, F=0, **kw):
    s = SHAPES[shape]
    if kind == "pssmlt":
        return fa.Renderer(cornell, s["res"][0], s["res"][1], fa.default_options(s["L"]), table=table,
                           pssmlt_options=api.default_pssmlt_options(s["L"], n_chains=s["n_chains"], spp=s["spp"], **kw))
    return fa.Renderer(cornell, s["res"][0], s["res"][1], fa.default_options(s["L"]), table=table,
                       mmlt_options=fa.default_mmlt_options(s["L"], mmlt_frequency=F, lens_techniques=int(kind == "lens"), n_chains=s["n_chains"], spp=s["spp"], **kw))


def render(r, kind, instance):
    (r.pssmlt_render if kind == "pssmlt" else r.mmlt_render)(instance, sync=True)


def snapshot(r, kind):
    """everything a render call leaves: (state arrays, frame, stats, st_norms and chains per technique or None)"""
    pss = kind == "pssmlt"
    return (r.pssmlt_state() if pss else r.mmlt_state(), r.framebuffer().copy(), r.pssmlt_stats() if pss else r.mmlt_stats(), None if pss else r.mmlt_st_norms())


def differences(a, b):
    """the names of what two snapshots differ in"""
    out = [k for k in a[0] if not np.array_equal(bits(a[0][k]), bits(b[0][k]))]
    out += ["stats." + k for k in a[2] if a[2][k] != b[2][k]]
    if not np.array_equal(bits(a[1]), bits(b[1])):
        out.append("frame")
    if a[3] is not None and not (np.array_equal(bits(a[3][0]), bits(b[3][0])) and np.array_equal(a[3][1], b[3][1])):
        out.append("st_norms")
    return out


class Ranks:
    """`world` rank contexts on one GPU, each with its shard and a torch int64 splat buffer of its own, and the reference context that runs every chain"""

    def __init__(self, cornell, table, kind, shape, F, world, persistence=None):
        self.kind, self.n, self.world = kind, SHAPES[shape]["n_chains"], world
        self.ref = make(cornell, table, kind, shape, F)
        self.ranks = [make(cornell, table, kind, shape, F) for _ in range(world)]
        self.bufs = []
        for k, r in enumerate(self.ranks):
            r.mlt_set_chain_shard(k, world)
            assert r.mlt_chain_shard() == dict(rank=k, world=world, n_local=S.shard_count(self.n, k, world), pending=0)
            self.bufs.append(r.mlt_splat_buffer())
        if persistence:
            for r in [self.ref] + self.ranks:
                r.mlt_set_persistence(*persistence)

    def call(self, instance):
        """one render call on everybody and every bit-for-bit claim about it; returns the names of what differs (empty: nothing)"""
        kind, ref, ranks = self.kind, self.ref, self.ranks
        torch = ref.torch
        render(ref, kind, instance)
        want = snapshot(ref, kind)
        for r in ranks:
            render(r, kind, instance)
        assert all(r.mlt_chain_shard()["pending"] == 1 for r in ranks) and ref.mlt_chain_shard() == dict(rank=0, world=1, n_local=self.n, pending=0)
        got = [snapshot(r, kind) for r in ranks]
        out = []
        # the ranks' chains, put back in the order of the global chains, are the reference's: coordinates, path_value, path_pdf, rejections, st, path_pixel, seeds
        whole = S.assemble([g[0] for g in got], self.n)
        out += [k for k in want[0] if not np.array_equal(bits(whole[k]), bits(want[0][k]))]
        # what the presampling pass leaves is everybody's: the table and its pixel plane, the brightness and the normalisation, st_norms
        for k, g in enumerate(got):
            out += ["rank %d %s" % (k, key) for key in S.REPLICATED if key in want[0] and not np.array_equal(bits(g[0][key]), bits(want[0][key]))]
            out += ["rank %d stats.%s" % (k, key) for key in ("image_brightness", "pdf_norm", "chain_length", "n_chains") if bits(g[2][key]).tolist() != bits(want[2][key]).tolist()]
            if want[3] is not None and not np.array_equal(bits(g[3][0]), bits(want[3][0])):
                out.append("rank %d st_norms" % k)
        # the counters and the chains seeded per technique add up to the reference's
        summed = S.summed_counters([g[2] for g in got])
        out += ["sum of " + k for k in summed if summed[k] != want[2][k]]
        assert summed["accepted"] + summed["rejected"] == self.n * want[2]["chain_length"]
        if want[3] is not None and not np.array_equal(sum(g[3][1].astype(np.int64) for g in got), want[3][1].astype(np.int64)):
            out.append("sum of st_chains")
        # the wire: the sum of the ranks' buffers into every rank's buffer; then every rank resolves the frame of one GPU
        total = torch.zeros_like(self.bufs[0])
        for b in self.bufs:
            total += b
        assert int((total != 0).sum()) > 0 or float(want[1][api.FB_COMPOSITED_C][:, :3].max()) == 0.0
        for b in self.bufs:
            b.copy_(total)
        torch.cuda.synchronize(ref.dev)
        for k, r in enumerate(ranks):
            r.mlt_finish(sync=True)
            assert r.mlt_chain_shard()["pending"] == 0 and int((self.bufs[k] != 0).sum()) == 0
            if not np.array_equal(bits(r.framebuffer()), bits(want[1])):
                out.append("rank %d frame" % k)
        assert float(want[1][api.FB_COMPOSITED_C][:, :3].max()) > 0
        return out

    def close(self):
        for r in [self.ref] + self.ranks:
            r.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind,F", MODES, ids=MODE_IDS)
def test_default_shard_is_todays_renderer(cornell, table, kind, F):
    """a. set_chain_shard(0, 1) after the init against a context that never called it, on B, instances 0..1: frame, chain state, table, seeds, stats and st_norms bit
    for bit; no call is ever pending and finish refuses"""
    a = make(cornell, table, kind, "B", F); b = make(cornell, table, kind, "B", F)
    b.mlt_set_chain_shard(0, 1)
    assert a.mlt_chain_shard() == dict(rank=0, world=1, n_local=200, pending=0) == b.mlt_chain_shard()
    for i in range(2):
        render(a, kind, i); render(b, kind, i)
        sa, sb = snapshot(a, kind), snapshot(b, kind)
        assert differences(sa, sb) == [] and sa[1][api.FB_COMPOSITED_C][:, :3].max() > 0
        assert b.mlt_chain_shard()["pending"] == 0
        with pytest.raises(api.FptError, match="fpt_mlt_finish: no render call is pending"):
            b.mlt_finish()
    a.close(); b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("shape,world", [("A", 2), ("A", 3), ("B", 2), ("B", 3)])
@pytest.mark.parametrize("kind,F", MODES, ids=MODE_IDS)
def test_n_contexts_on_one_gpu_give_the_frame_of_one(cornell, table, kind, F, shape, world):
    """b. W rank contexts and a reference context in one process, two consecutive instances (the second rescales a non-empty frame): the ranks' downloads reordered by
    g = r + i * W are the reference's state, their counters and chains per technique add up to its, and after the test has summed the splat buffers and every rank has
    called mlt_finish every rank's frame is the reference's, bit for bit"""
    run = Ranks(cornell, table, kind, shape, F, world)
    for i in range(2):
        assert run.call(i) == [], "instance %d" % i
    run.close()


@pytest.mark.gpu
def test_eight_ranks_on_one_gpu(cornell, table):
    """b, W = 8 at 200 chains (25 each), `-mmlt` with lens techniques and swaps, once"""
    run = Ranks(cornell, table, "lens", "B", 2, 8)
    assert [r.mlt_chain_shard()["n_local"] for r in run.ranks] == [25] * 8
    for i in range(2):
        assert run.call(i) == [], "instance %d" % i
    run.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind,F,shape", [("pssmlt", 0, "A"), ("lens", 2, "B")], ids=["pssmlt-A", "lens-F2-B"])
def test_shards_with_persistent_chains(cornell, table, kind, F, shape):
    """c. mlt_set_persistence(2, 1) over instances 0..3 with W = 3: calls 0 and 2 reseed (their first step deposits nothing), calls 1 and 3 continue the shard's chains;
    the same bit-for-bit claims after every call"""
    run = Ranks(cornell, table, kind, shape, F, 3, persistence=(2, 1))
    for i in range(4):
        assert run.call(i) == [], "instance %d" % i
        flags = [r.mlt_persistence()["last_call_reseeded"] for r in [run.ref] + run.ranks]
        assert flags == [1 - i % 2] * 4, (i, flags)
    run.close()


@pytest.mark.gpu
def test_ranks_run_different_chains(cornell, table):
    """d. ranks 0 and 1 of a W = 2 run do not hold the same slot-0 chain: rank 1's slot 0 is the reference's chain 1, not its chain 0 (a rank that ran the global
    chains 0, 1, 2, ... would pass no test above either, but this names the mistake)"""
    run = Ranks(cornell, table, "mmlt", "A", 2, 2)
    assert run.call(0) == []
    s0, s1, ref = run.ranks[0].mmlt_state(), run.ranks[1].mmlt_state(), run.ref.mmlt_state()
    for k in ("light_u", "eye_u"):
        assert not np.array_equal(bits(s0[k][:, 0]), bits(s1[k][:, 0])), k
        assert np.array_equal(bits(s0[k][:, 0]), bits(ref[k][:, 0])) and np.array_equal(bits(s1[k][:, 0]), bits(ref[k][:, 1])), k
    assert not np.array_equal(bits(s0["light_u"]), bits(s1["light_u"])) and not np.array_equal(s0["seeds"], s1["seeds"])
    run.close()


@pytest.mark.gpu
def test_refusals_name_the_call_and_leave_the_state_usable(cornell, table):
    """e. set_chain_shard before an init, a bad rank, a bad world, world > n_chains; with W = 2: a render call while one is pending, a shard change while pending, finish
    with nothing pending -- each refused with a message that names the call, and the two ranks still end with the reference's frame.  A refused shard leaves the next
    frame unchanged"""
    plain = fa.Renderer(cornell, 32, 32, fa.default_options(4), table=table)
    for call in (lambda: plain.mlt_set_chain_shard(0, 1), plain.mlt_chain_shard, plain.mlt_finish):
        with pytest.raises(api.FptError, match=r"^fpt_mlt_(set_chain_shard|get_chain_shard|finish): fpt_pssmlt_init / fpt_mmlt_init has not been called"):
            call()
    plain.close()
    # refused shards: nothing is written, the next frame is the one of a context that never asked
    a = make(cornell, table, "mmlt", "B", 2); b = make(cornell, table, "mmlt", "B", 2)
    for rank, world, why in ((0, 0, "world must be at least 1"), (3, 3, "rank must be below world"), (7, 2, "rank must be below world"), (0, 201, "world exceeds n_chains")):
        with pytest.raises(api.FptError, match="^fpt_mlt_set_chain_shard: " + why):
            b.mlt_set_chain_shard(rank, world)
        assert b.mlt_chain_shard() == dict(rank=0, world=1, n_local=200, pending=0)
    b.mlt_set_chain_shard(199, 200); assert b.mlt_chain_shard()["n_local"] == 1          # W == n_chains is the last world accepted
    b.mlt_set_chain_shard(0, 1)
    render(a, "mmlt", 0); render(b, "mmlt", 0)
    assert differences(snapshot(a, "mmlt"), snapshot(b, "mmlt")) == []
    a.close(); b.close()
    # around a pending finish
    run = Ranks(cornell, table, "mmlt", "A", 2, 2)
    r0 = run.ranks[0]
    with pytest.raises(api.FptError, match="^fpt_mlt_finish: no render call is pending"):
        r0.mlt_finish()
    render(r0, "mmlt", 0)
    held = run.bufs[0].clone()
    with pytest.raises(api.FptError, match="^fpt_mmlt_render: .*waits for fpt_mlt_finish"):
        render(r0, "mmlt", 0)
    with pytest.raises(api.FptError, match="^fpt_mlt_set_chain_shard: .*fpt_mlt_finish"):
        r0.mlt_set_chain_shard(0, 1)
    assert r0.mlt_chain_shard() == dict(rank=0, world=2, n_local=128, pending=1) and bool((run.bufs[0] == held).all())
    # an init is the way out of a pending call nobody will finish; here the call is finished with the sums as they are, and the rank starts over
    r0.mlt_finish(sync=True)
    with pytest.raises(api.FptError, match="^fpt_mlt_finish: no render call is pending"):
        r0.mlt_finish()
    r0.clear_framebuffer()
    for i in range(2):
        assert run.call(i) == [], "instance %d" % i
    run.close()


@pytest.mark.gpu
def test_two_rank_rccl_shards_equal_single_gpu_frame():
    """f. two processes, one GPU each, the all-reduces of fpt_mlt_finish over RCCL (tests/_mlt_shard_worker.py): both ranks end with the single-GPU frame and, the
    counters being reduced too, its statistics.  Needs two devices"""
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs; one visible here")
    env = dict(os.environ); env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    import socket
    with socket.socket() as sk:          # a free port: the box is shared
        sk.bind(("127.0.0.1", 0)); port = sk.getsockname()[1]
    p = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port", str(port),
                        os.path.join(ROOT, "tests", "_mlt_shard_worker.py")], capture_output=True, text=True, timeout=900, env=env)
    assert p.returncode == 0 and p.stdout.count("MLT_SHARD_OK world=2") == 2, (p.stdout[-1500:], p.stderr[-3000:])
