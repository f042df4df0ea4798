"""The multiplexed Metropolis renderer (`-mmlt`, one (s, t) technique per chain: fpt_mlt.hip, fpt_mlt_api.cpp, the technique table and the technique-fixed
evaluation of fpt_bpt.hip) against exact invariants, in the manner of tests/test_pssmlt.py.

(a) the new small kernels against the numpy judge tests/mmlt_truth.py, bit for bit; (b) identities with what is judged already: the technique table summed in sink
order IS the value PSSMLT's presampling pass gives (which tests/test_pssmlt.py proves equal to a BPT pass), a technique evaluated alone IS its table cell; (c) a
replay of whole render calls, swaps included, with three planted mistakes refused; (d) the estimator's mean against the BPT's.

Shapes: A = CornellBox-JP 32 x 32, max_path_length 4, 256 chains, 4 spp (chain length 16); B = 24 x 16, max_path_length 6, 200 chains (not a multiple of the
wave), 4 spp (chain length 7)."""
import copy
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mlt_truth as T  # noqa: E402
import mmlt_truth as M  # noqa: E402

import fermat_amd as fa  # noqa: E402
from fermat_amd import api  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
U32 = np.uint32
SHAPES = {"A": dict(res=(32, 32), L=4, n_chains=256, spp=4), "B": dict(res=(24, 16), L=6, n_chains=200, spp=4)}
NAMES = ("fpt_mmlt_init", "fpt_mmlt_render", "fpt_mmlt_get_stats", "fpt_mmlt_get_st_norms", "fpt_mmlt_download", "fpt_mmlt_debug_eval")


def bits(a):
    return np.ascontiguousarray(a).view(U32)


# ---- CPU ----------------------------------------------------------------------------------------------------------------------------------------------------
def test_entry_points_declared_exported_and_judge_sound():
    """1. declared in the header, exported by the library, wrapped in Python; the judge on its own"""
    text = open(os.path.join(ROOT, "include", "fermat_pt_hip.h")).read()
    lib = fa.lib()
    for n in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % n, text), "not declared: " + n
        assert n in api.ENTRY_POINTS and hasattr(lib, n), "not exported: " + n
    assert re.search(r"typedef struct fpt_mmlt_options", text) and re.search(r"typedef struct fpt_mmlt_stats", text)
    o = fa.default_mmlt_options(5, mmlt_frequency=3, n_chains=77)
    assert o.mmlt_frequency == 3 and o.mlt.n_chains == 77 and o.mlt.spp == 4 and o.mlt.bpt.max_path_length == 5 and fa.default_mmlt_options().mmlt_frequency == 0
    for m in ("mmlt_render", "mmlt_stats", "mmlt_st_norms", "mmlt_state", "mmlt_eval"):
        assert callable(getattr(fa.Renderer, m))
    assert int(api.tech_word(2, 3)) == int(M.word(2, 3))
    M.self_check()


def test_host_helpers_under_sanitizers():
    """2. the stand-alone program over the host helpers (technique count and index, swap proposal, refusals and their strings), built with
    -fsanitize=address,undefined for the host and run here"""
    run = subprocess.run(["bash", os.path.join(ROOT, "tools", "sanitize_mlt_host.sh")], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, (run.stdout + run.stderr)[-3000:]
    assert "all checks passed" in run.stdout and "mmlt" in run.stdout, run.stdout[-2000:]


# ---- GPU ----------------------------------------------------------------------------------------------------------------------------------------------------
def options(shape, **kw):
    s = SHAPES[shape]
    return fa.default_mmlt_options(s["L"], n_chains=s["n_chains"], spp=s["spp"], **kw)


def make(cornell, table, shape, **kw):
    s = SHAPES[shape]
    return fa.Renderer(cornell, s["res"][0], s["res"][1], fa.default_options(s["L"]), table=table, mmlt_options=options(shape, **kw))


def render_and_state(r, instance=0):
    r.mmlt_render(instance, sync=True)
    return r.mmlt_state(), r.framebuffer(), r.mmlt_stats()


@pytest.fixture(scope="module")
def started(cornell, table):
    """per shape: the state a render call with the perturbations and the swaps off leaves -- the chains' seeds, starting techniques and recovered coordinates, the
    technique table -- with its frame, stats and st_norms.  Computed once, left unchanged"""
    out = {}
    for shape in SHAPES:
        r = make(cornell, table, shape, light_perturbations=0, eye_perturbations=0)
        st, fb, stats = render_and_state(r)
        norms, chains = r.mmlt_st_norms()
        out[shape] = dict(state=st, fb=fb.copy(), stats=stats, norms=norms, chains=chains)
        r.close()
    return out


@pytest.fixture(scope="module")
def probe(cornell, table):
    r = fa.Renderer(cornell, 8, 8, fa.default_options(2), table=table, mmlt_options=fa.default_mmlt_options(2, n_chains=8, spp=1))
    yield r
    r.close()


@pytest.mark.gpu
def test_probes(probe):
    """3. technique index and swap proposal against the judge, bit for bit; t = 2, s = 0 and k = 1 among the inputs"""
    for L in (1, 2, 4, 6, 15):
        w = M.words(L)
        bad = np.array([M.word(0, 1), M.word(0, L + 2), M.word(L, 2), M.word(1, L + 1), M.word(0, 0)], U32)
        st = np.concatenate([w, bad])
        _, index, back = probe.debug_mlt(3, [st, np.zeros(len(st), U32), np.zeros(len(st), U32)], params=(L,), n=len(st))
        assert np.array_equal(index[:len(w)], np.arange(len(w), dtype=U32)) and np.array_equal(back[:len(w)], w)
        assert (index[len(w):] == 0xFFFFFFFF).all() and (back[len(w):] == 0xFFFFFFFF).all()
        rng = np.random.default_rng(L)
        st = np.tile(w, 64); chain = rng.integers(0, 1 << 20, len(st)).astype(U32)
        for instance, step in ((0, 2), (3, 14)):
            _, _, st_new, m = probe.debug_mlt(4, [st, chain, np.zeros(len(st), U32), np.zeros(len(st), F32)], params=(L, instance, step), n=len(st))
            want_m = T.mutation_number(instance, step, chain, U32(M.swap_dim(L)))
            assert np.array_equal(bits(m), bits(want_m))
            assert np.array_equal(st_new, M.swap_proposal(st, want_m))
            s, t = M.unword(st); sn, tn = M.unword(st_new)
            assert (sn + tn == s + t).all() and (tn >= 2).all()
            assert ((s + t == 2) <= (st_new == st)).all() and (s + t == 2).any()          # k = 1 proposes the chain's own technique
            if L > 1:
                assert (st_new != st).any() and ((s == 0) & (sn == s + t - 2)).any() and ((t == 2) & (sn == 0)).any()


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ["A", "B"])
def test_presampling_table(cornell, table, started, shape):
    """4. the table against PSSMLT's presampling value, its zero cells, st_norms / brightness / seeds against the judge, the chains per technique"""
    sh = SHAPES[shape]; L = sh["L"]; res = sh["res"]; npx = res[0] * res[1]; n = sh["n_chains"]
    got = started[shape]; st = got["state"]; tb = st["table"]
    assert tb.shape == (M.tech_count(L), npx, 4)
    # (a) the cells added in sink order == the ValueSink value of the same pass (a fresh PSSMLT context with the same options: the same sampler, the same instance)
    p = fa.Renderer(cornell, res[0], res[1], fa.default_options(L), table=table, pssmlt_options=fa.api.default_pssmlt_options(L, n_chains=n, spp=sh["spp"]))
    p.pssmlt_render(0, sync=True)
    presample = p.pssmlt_state()["presample"]
    p.close()
    assert presample[:, :3].max() > 0 and np.array_equal(bits(M.sink_order_sum(tb, L)), bits(presample))
    # (b) the table is dense over the valid techniques, so one with s + t > L + 1 (or t < 2) has no cell to be non-zero; in the (L + 2)^2 arrays it is zero
    valid = np.zeros((L + 2, L + 2), bool)
    for s, t in M.techniques(L):
        assert s + t <= L + 1 and t >= 2
        valid[t, s] = True
    assert not got["norms"][~valid].any() and not got["chains"][~valid].any()
    # (c) st_norms, brightness and every seed from the downloaded table
    q, cdf, norms, brightness = M.st_norms(tb, L)
    assert np.array_equal(bits(got["norms"]), bits(norms)) and got["stats"]["image_brightness"] == brightness and brightness > 0
    seeds = M.sample_seeds(cdf, n, 0)
    assert np.array_equal(st["seeds"], seeds)
    tech = seeds // npx
    assert (np.diff(tech.astype(np.int64)) >= 0).all()          # the chains start sorted by technique
    assert np.array_equal(st["st"], M.words(L)[tech])
    assert (T.max_comp(tb.reshape(-1, 4)[seeds]) > 0).all()
    # (d) chains per technique: the reported numbers are the seeds'; the stratified rule with one offset for all strata puts within 1 of n * share into every technique
    # and within 1 of the cumulative share below every block's end
    total = int(cdf[-1]); below = 0
    for k, (s, t) in enumerate(M.techniques(L)):
        count = int((tech == k).sum()); below += count
        assert got["chains"][t, s] == count
        end = int(cdf[(k + 1) * npx - 1])
        assert abs(below - n * (end / total)) <= 1.0, (s, t, below, n * end / total)
        assert abs(count - n * ((end - (int(cdf[k * npx - 1]) if k else 0)) / total)) <= 1.0, (s, t, count)
    assert got["chains"].sum() == n and (got["norms"] > 0).sum() > 1


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ["A", "B"])
def test_chains_per_technique_within_one(started, shape):
    """4 (d) as the issue states it: the number of chains seeded per technique is within 1 of n_chains * that technique's share of the total.

    A property of the stratified rule only when all strata share one offset (tests/mmlt_truth.py sample_seeds): with a jitter of its own in every stratum, PSSMLT's
    rule, the chains below a point x number within 1 of n x and a technique's count, a difference of two such numbers, is within 2 -- shape B then gave technique
    (1, 2) 38 chains where n * share = 39.33.  Hence the multiplexed renderer's exact common-offset targets."""
    sh = SHAPES[shape]; L = sh["L"]; npx = sh["res"][0] * sh["res"][1]; n = sh["n_chains"]
    got = started[shape]
    q, cdf, norms, brightness = M.st_norms(got["state"]["table"], L)
    total = int(cdf[-1])
    worst = 0.0
    for k, (s, t) in enumerate(M.techniques(L)):
        share = (int(cdf[(k + 1) * npx - 1]) - (int(cdf[k * npx - 1]) if k else 0)) / total
        d = abs(int(got["chains"][t, s]) - n * share)
        print("shape %s technique (%d, %d): %d chains, n * share = %.3f" % (shape, s, t, got["chains"][t, s], n * share))
        worst = max(worst, d)
    assert worst <= 1.0, worst


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ["A", "B"])
def test_technique_fixed_evaluation_is_its_table_cell(cornell, table, started, shape):
    """5. every seed, and 512 further (path, technique) pairs -- the paths are those whose coordinates the chains recovered, the techniques any of the table: zero cells,
    s = 0 and s = 1 among them -- evaluated alone give the table's cell bit for bit; and the rays of a render call stay within the technique's bound"""
    sh = SHAPES[shape]; L = sh["L"]; res = sh["res"]; npx = res[0] * res[1]; n = sh["n_chains"]
    got = started[shape]; st = got["state"]; tb = st["table"]
    path = st["seeds"] % npx
    r = make(cornell, table, shape)
    value, rays = r.mmlt_eval(st["light_u"], st["eye_u"], st["st"], with_rays=True)
    assert np.array_equal(bits(value), bits(tb.reshape(-1, 4)[st["seeds"]]))
    assert np.array_equal(bits(st["path_value"]), bits(value))          # and what the chains held after their steps with the perturbations off
    assert 0 < rays <= int(M.max_rays(st["st"]).sum())
    rng = np.random.default_rng(1234)
    w = M.words(L)
    for lo in range(0, 512, n):
        m = min(n, 512 - lo)
        c = rng.integers(0, n, m); k = rng.integers(0, len(w), m)
        value, rays = r.mmlt_eval(st["light_u"][:, c], st["eye_u"][:, c], w[k], with_rays=True)
        want = tb[k, path[c]]
        assert np.array_equal(bits(value), bits(want))
        s, t = M.unword(w[k])
        zero = T.max_comp(want) == 0
        assert zero.any() and (~zero).any() and (s == 0).any() and (s == 1).any()
        assert 0 < rays <= int(M.max_rays(w[k]).sum())
    r.close()
    # the truncation is real: a render call with swaps off queues at most chain_length * sum over the chains of max(s - 1, 0) + (t - 1) + [s > 0] rays
    stats = got["stats"]
    bound = stats["chain_length"] * int(M.max_rays(st["st"]).sum())
    print("rays of the render call: %d, bound %d, a full evaluation would queue up to %d" % (stats["rays"], bound, stats["chain_length"] * n * (2 * L + L * (L + 1) // 2)))
    assert 0 < stats["rays"] <= bound


def perturb_on_device(r, u, mutation, instance, step, chain, dim, radius=0.01):
    u = np.ascontiguousarray(u, F32).reshape(-1)
    out = r.debug_mlt(0, [u, None, np.ascontiguousarray(chain, U32), np.ascontiguousarray(dim, U32), np.zeros(len(u), F32), np.zeros(len(u), F32)],
                      params=(mutation, instance, step, int(F32(radius).view(U32))), n=len(u))
    return out[4]


def replay_render(r, start, stats, shape, F, mistake=None, norms=None):
    sh = SHAPES[shape]; L = sh["L"]; res = sh["res"]
    dims = (L + 1) * 3; n = sh["n_chains"]
    chain = np.tile(np.arange(n, dtype=U32), dims)

    def perturb(u, offset, mutation, step):
        dim = np.repeat(np.arange(dims, dtype=U32) + U32(offset), n)
        return perturb_on_device(r, u.reshape(-1), mutation, 0, step, chain, dim).reshape(dims, n)
    opts = dict(independent_samples=0.0, light_perturbations=1, eye_perturbations=1)
    return M.replay(start["light_u"], start["eye_u"], start["st"], L, stats["chain_length"], 0, opts, F, stats["pdf_norm"], res, np.zeros((res[0] * res[1], 4), F32), perturb,
                    lambda a, b, st: r.mmlt_eval(a, b, st, with_rays=True), norms=norms, mistake=mistake)


@pytest.mark.gpu
@pytest.mark.parametrize("shape,F", [("A", 0), ("A", 2), ("B", 2)])
def test_replay_of_a_render(cornell, table, started, shape, F):
    """6. all steps on the host: coordinates from the probe, values from mmlt_eval, acceptance and swap arithmetic from the judge -- COMPOSITED_C, the chains' final
    (s, t) and the counters equal render()'s bit for bit.  With F = 2 three planted mistakes are each refused"""
    r = make(cornell, table, shape, mmlt_frequency=F)
    st, fb, stats = render_and_state(r)
    start = started[shape]["state"]
    want, frame = replay_render(r, start, stats, shape, F)
    n_swaps = sum(M.is_swap_step(F, k) for k in range(stats["chain_length"]))
    assert n_swaps == (0 if F == 0 else (stats["chain_length"] - 1) // F) and 0 < want["rejected"]
    for k in ("accepted", "rejected", "swaps_proposed", "swaps_accepted", "rays"):
        assert want[k] == stats[k], (k, want[k], stats[k])
    assert stats["swaps_proposed"] == n_swaps * SHAPES[shape]["n_chains"] and (F == 0 or 0 < stats["swaps_accepted"] < stats["swaps_proposed"])
    assert np.array_equal(st["st"], want["st"]) and ((F != 0) == bool((st["st"] != start["st"]).any()))
    for k in ("light_u", "eye_u", "path_value", "path_pdf"):
        assert np.array_equal(bits(st[k]), bits(want[k])), k
    assert np.array_equal(st["rejections"], want["rejections"])
    assert np.array_equal(bits(fb[api.FB_COMPOSITED_C]), bits(frame)) and fb[api.FB_COMPOSITED_C][:, :3].max() > 0
    if F and shape == "A":
        for mistake in ("norm_ratio", "clamp", "commit"):
            bad, bad_frame = replay_render(r, start, stats, shape, F, mistake, norms=started[shape]["norms"])
            assert not np.array_equal(bits(fb[api.FB_COMPOSITED_C]), bits(bad_frame)), mistake
    r.close()


@pytest.mark.gpu
def test_determinism_and_swaps_do_something(cornell, table):
    """7. two fresh contexts, instances 0..2: the same bits in frame and state; the frame with F = 0 differs from the one with F = 2"""
    got = {}
    for key, F in (("a", 2), ("b", 2), ("c", 0)):
        r = make(cornell, table, "A", mmlt_frequency=F)
        for i in range(3):
            r.mmlt_render(i)
        got[key] = (r.mmlt_state(), r.framebuffer().copy(), r.mmlt_stats())
        r.close()
    assert np.array_equal(bits(got["a"][1]), bits(got["b"][1])) and got["a"][1][api.FB_COMPOSITED_C][:, :3].max() > 0
    for k in got["a"][0]:
        assert np.array_equal(bits(got["a"][0][k]), bits(got["b"][0][k])), k
    assert got["a"][2] == got["b"][2]
    assert not np.array_equal(bits(got["a"][1][api.FB_COMPOSITED_C]), bits(got["c"][1][api.FB_COMPOSITED_C]))
    for c in (0, 1, 2, 3, 4):
        assert not got["a"][1][c].any()          # COMPOSITED_C alone is written


# the smallest power of two at which the data scaled by 1.1 fall outside for F = 0 and for F = 2 (measured on the MI355X: DESIGN.md 6g)
N_PASSES = 64


def block_sums(frame, res):
    img = frame[:, :3].astype(np.float64).sum(1).reshape(res[1], res[0])
    return img.reshape(res[1] // 8, 8, res[0] // 8, 8).sum((1, 3)).reshape(-1)


def estimator_passes(cornell, table, n_passes, frequencies=(0, 2)):
    """the block sums of n_passes independent passes (instances 0 .. n_passes - 1, each on a cleared frame) of BPT and of MMLT per swap frequency"""
    res = SHAPES["A"]["res"]; L = SHAPES["A"]["L"]

    def passes(r, render):
        out = []
        for i in range(n_passes):
            r.clear_framebuffer()
            render(i)
            out.append(block_sums(r.framebuffer()[api.FB_COMPOSITED_C] * F32(i + 1), res))
        r.close()
        return np.array(out)
    b = fa.Renderer(cornell, res[0], res[1], fa.default_options(L), table=table, bpt_options=fa.default_bpt_options(L, light_tracing=0.0, single_connection=0))
    B = passes(b, lambda i: b.bpt_render(i, sync=True))
    P = {}
    for F in frequencies:
        r = make(cornell, table, "A", mmlt_frequency=F)
        P[F] = passes(r, lambda i: r.mmlt_render(i, sync=True))
    return B, P


def estimator_z(B, P, n):
    """|z| per 8 x 8 block of the first n passes of MMLT against BPT's, plain and with the MMLT data scaled by 1.1"""
    B = B[:n]; P = P[:n]
    mB = B.mean(0); seB = B.std(0, ddof=1) / np.sqrt(n)
    mP = P.mean(0); seP = P.std(0, ddof=1) / np.sqrt(n)
    z = np.abs(mP - mB) / np.sqrt(seP ** 2 + seB ** 2)
    z_scaled = np.abs(1.1 * mP - mB) / np.sqrt((1.1 * seP) ** 2 + seB ** 2)
    return z, z_scaled, mP.sum(), mB.sum()


@pytest.mark.gpu
def test_estimator_agrees_with_bpt(cornell, table):
    """8. N_PASSES independent passes each of MMLT (F = 0 and F = 2) and of BPT with the same options; the sums over the sixteen 8 x 8 blocks agree within 5 standard
    errors in EVERY block, and the same data scaled by 1.1 do not (the power of the check).  Measured figures: DESIGN.md 6g."""
    B, P = estimator_passes(cornell, table, N_PASSES)
    for F in P:
        z, z_scaled, tP, tB = estimator_z(B, P[F], N_PASSES)
        print("estimator F = %d, %d passes: worst |z| = %.2f, worst |z| of the data scaled by 1.1 = %.2f, total M %.4f B %.4f" % (F, N_PASSES, z.max(), z_scaled.max(), tP, tB))
        assert (z <= 5.0).all(), (F, z)
        assert (z_scaled > 5.0).any(), (F, z_scaled)


@pytest.mark.gpu
def test_refusals_and_black_scene(cornell, table):
    """9. what init refuses names the option; a scene without emitters renders without a fault and leaves the frame rescaled only"""
    L = 4

    def refused(word, pixels=None, **kw):
        with pytest.raises(fa.FptError) as e:
            fa.Renderer(cornell, 16, 16, fa.default_options(L), table=table, pixels=pixels, mmlt_options=fa.default_mmlt_options(L, **dict(dict(n_chains=64, spp=4), **kw)))
        assert "fpt_mmlt_init" in str(e.value) and word in str(e.value), str(e.value)
    refused("use_vpls", use_vpls=1)
    refused("pixels", pixels=np.arange(128, dtype=U32))
    refused("n_chains", n_chains=0)
    refused("n_chains", n_chains=1 << 24, spp=1 << 20)
    refused("spp", n_chains=300, spp=1)
    dark = copy.copy(cornell); dark.materials = cornell.materials.copy(); dark.materials["emissive"][:] = 0.0
    r = fa.Renderer(dark, 16, 16, fa.default_options(L), table=table, mmlt_options=fa.default_mmlt_options(L, n_chains=64, spp=4, mmlt_frequency=2))
    # a technique table of 2^32 cells or more: refused before anything is allocated (the view names a frame of 40000 x 1000 pixels, 120 techniques each)
    big = type(r.view).from_buffer_copy(r.view); big.res_x = 40000; big.res_y = 1000
    o = fa.default_mmlt_options(15, n_chains=64, spp=4)
    assert r.L.fpt_mmlt_init(r.ctx, C.byref(o), C.byref(big), r.samples_dir.encode(), None, C.c_uint32(0)) != 0
    msg = r.L.fpt_last_error(r.ctx).decode()
    assert "fpt_mmlt_init" in msg and "technique table" in msg and "32 bits" in msg, msg
    with pytest.raises(fa.FptError):
        r.mmlt_render(0)          # the refused init left no renderer behind
    r._check(r.L.fpt_mmlt_init(r.ctx, C.byref(r.mmlt_options), C.byref(r.view), r.samples_dir.encode(), None, C.c_uint32(0)))
    r.fb[api.FB_COMPOSITED_C] = 1.0
    r.mmlt_render(1, sync=True)
    fb = r.framebuffer(); stats = r.mmlt_stats(); norms, chains = r.mmlt_st_norms()
    assert stats["image_brightness"] == 0 and stats["accepted"] == 0 and stats["rejected"] == 0 and stats["rays"] == 0 and not norms.any() and not chains.any()
    assert np.array_equal(bits(fb[api.FB_COMPOSITED_C]), bits(np.full((256, 4), 0.5, F32)))
    r.close()


@pytest.mark.gpu
def test_cli_mmlt_writes_the_renderers_image(cornell, tmp_path, table):
    """`fermat_hip -i ... -mmlt -mmlt-swaps 2 -passes N -o ...` writes an image: the one the Renderer gives for the same options, and prints the (s, t) table"""
    from fermat_amd import scene
    exe = os.path.join(ROOT, "fermat_amd", "bin", "fermat_hip")
    d = os.path.join(scene.DATA_DIR, "scenes", "CornellBox")
    out = str(tmp_path / "mmlt")
    run = subprocess.run([exe, "-i", os.path.join(d, "CornellBox-JP.obj"), "-c", os.path.join(d, "camera-frontal.txt"), "-r", "48", "36", "-mmlt", "-chains", "1", "-spp", "4",
                          "-pl", "4", "-mmlt-swaps", "2", "-passes", "2", "-o", out], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr[-2000:]
    assert "st chains" in run.stderr and "[0,2] :" in run.stderr and "[3,2] :" in run.stderr and "[0,5] :" in run.stderr
    r = fa.Renderer(cornell, 48, 36, fa.default_options(4), table=table, mmlt_options=fa.default_mmlt_options(4, n_chains=1024, spp=4, mmlt_frequency=2))
    for i in range(3):
        r.mmlt_render(i)
    want = r.to_rgba()[..., :3]
    got = (scene.load_tga(out + ".tga")[..., :3] * 255.0 + 0.5).astype(np.uint8)
    assert want.max() > 0 and np.array_equal(got, want)
    r.close()
