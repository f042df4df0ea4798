"""The lens techniques of the multiplexed Metropolis renderer (`-mmlt -mmlt-lens 1`, fpt_mmlt_options::lens_techniques = 1: the connections (s, 1), s in [2, L], of a light
sub-path straight to the lens, beside the t >= 2 techniques, with light tracing on) against exact invariants, in the manner of tests/test_mmlt.py.

(a) the switch off is the renderer as it was; (b) identities with what is judged already: the lens block of the technique table IS the BPT's light-tracing splats, the
t >= 2 block plus those splats IS the BPT's frame, a technique evaluated alone IS its cell and lands on its cell's pixel; (c) a replay of whole render calls from the
probe's values and the judge tests/mmlt_lens_truth.py, with six planted mistakes refused; (d) the estimator's mean against the BPT's with light tracing on.

Shapes: those of tests/test_mmlt.py.  A = CornellBox-JP 32 x 32, max_path_length 4, 256 chains, 4 spp (chain length 16); B = 24 x 16, max_path_length 6, 200 chains, 4 spp."""
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
import mmlt_lens_truth as J  # noqa: E402

import fermat_amd as fa  # noqa: E402
from fermat_amd import api  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
U32 = np.uint32
NONE = J.NONE
SHAPES = {"A": dict(res=(32, 32), L=4, n_chains=256, spp=4), "B": dict(res=(24, 16), L=6, n_chains=200, spp=4)}
STATE_KEYS = ("light_u", "eye_u", "path_value", "path_pdf", "rejections", "seeds", "st", "table")


def bits(a):
    return np.ascontiguousarray(a).view(U32)


# ---- CPU ----------------------------------------------------------------------------------------------------------------------------------------------------
def test_switch_declared_wrapped_and_judge_sound():
    """the field is the last of fpt_mmlt_options in the header and in the ctypes mirror, the flag and the new entry points exist; the judge on its own"""
    text = open(os.path.join(ROOT, "include", "fermat_pt_hip.h")).read()
    assert re.search(r"uint32_t\s+mmlt_frequency;[^}]*uint32_t\s+lens_techniques;[^}]*}\s*fpt_mmlt_options;", text)
    assert [f[0] for f in api.MmltOptions._fields_] == ["mlt", "mmlt_frequency", "lens_techniques"]
    lib = fa.lib()
    for n in ("fpt_mmlt_download_pixels", "fpt_mmlt_debug_eval_pixels", "fpt_debug_bpt_splat_entries"):
        assert re.search(r"\bint\s+%s\s*\(" % n, text) and n in api.ENTRY_POINTS and hasattr(lib, n), n
    o = fa.default_mmlt_options(5, mmlt_frequency=3, lens_techniques=1, n_chains=77)
    assert o.lens_techniques == 1 and o.mmlt_frequency == 3 and o.mlt.n_chains == 77 and fa.default_mmlt_options().lens_techniques == 0
    assert "-mmlt-lens" in open(os.path.join(ROOT, "fermat_amd", "csrc", "host", "fpt_renderer.cpp")).read()
    assert "--lens" in open(os.path.join(ROOT, "tools", "time_pssmlt.py")).read()
    J.self_check()


def test_lens_host_helpers_under_sanitizers():
    """the stand-alone program over the lens-aware host helpers (index / inverse bijection for L = 1 .. 15, symmetry of the ring walk, the ray bound, the refusal
    strings), built with -fsanitize=address,undefined for the host and run here"""
    run = subprocess.run(["bash", os.path.join(ROOT, "tools", "sanitize_mlt_lens_host.sh")], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, (run.stdout + run.stderr)[-3000:]
    assert "all checks passed" in run.stdout and "lens" in run.stdout, run.stdout[-2000:]


# ---- GPU ----------------------------------------------------------------------------------------------------------------------------------------------------
def options(shape, **kw):
    s = SHAPES[shape]
    return fa.default_mmlt_options(s["L"], n_chains=s["n_chains"], spp=s["spp"], **dict(dict(lens_techniques=1), **kw))


def make(cornell, table, shape, **kw):
    s = SHAPES[shape]
    return fa.Renderer(cornell, s["res"][0], s["res"][1], fa.default_options(s["L"]), table=table, mmlt_options=options(shape, **kw))


def make_bpt(cornell, table, shape):
    s = SHAPES[shape]
    return fa.Renderer(cornell, s["res"][0], s["res"][1], fa.default_options(s["L"]), table=table,
                       bpt_options=fa.default_bpt_options(s["L"], light_tracing=1.0, single_connection=0))


def render_and_state(r, instance=0):
    r.mmlt_render(instance, sync=True)
    return r.mmlt_state(), r.framebuffer(), r.mmlt_stats()


@pytest.fixture(scope="module")
def started(cornell, table):
    """per shape: what a render call with lens on, perturbations and swaps off leaves -- seeds, starting techniques, recovered coordinates, the technique table and its
    pixel plane -- with frame, stats and st_norms.  Computed once, left unchanged"""
    out = {}
    for shape in SHAPES:
        r = make(cornell, table, shape, light_perturbations=0, eye_perturbations=0)
        st, fb, stats = render_and_state(r)
        norms, chains = r.mmlt_st_norms()
        out[shape] = dict(state=st, fb=fb.copy(), stats=stats, norms=norms, chains=chains)
        r.close()
    return out


@pytest.fixture(scope="module")
def bpt_pass(cornell, table):
    """per shape: pass 0 of the BPT with light_tracing = 1, single_connection = 0 -- the deferred splat sums, the splat entries, and (a second context) the frame"""
    out = {}
    for shape in SHAPES:
        b = make_bpt(cornell, table, shape)
        splats = b.bpt_defer_splats()
        b.bpt_render(0, sync=True)
        sums = splats.cpu().numpy().copy()
        entries, visible = b.bpt_splat_entries()
        b.close()
        b = make_bpt(cornell, table, shape)
        b.clear_framebuffer()
        b.bpt_render(0, sync=True)
        out[shape] = dict(sums=sums, entries=entries, visible=visible, frame=b.framebuffer()[api.FB_COMPOSITED_C].copy())
        b.close()
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("F", [0, 2])
def test_off_is_off(cornell, table, F):
    """1. lens_techniques = 0 against an options struct built the old way (two initialisers, as before the field existed): frame, chain state, counters and st_norms of
    one render call of A, bit for bit"""
    sh = SHAPES["A"]
    old_way = api.MmltOptions(api.default_pssmlt_options(sh["L"], n_chains=sh["n_chains"], spp=sh["spp"]), F)
    got = []
    for o in (old_way, options("A", lens_techniques=0, mmlt_frequency=F)):
        assert o.lens_techniques == 0
        r = fa.Renderer(cornell, sh["res"][0], sh["res"][1], fa.default_options(sh["L"]), table=table, mmlt_options=o)
        st, fb, stats = render_and_state(r)
        assert "table_pixel" not in st and st["table"].shape[0] == M.tech_count(sh["L"])
        got.append((st, fb.copy(), stats, r.mmlt_st_norms()))
        r.close()
    a, b = got
    assert np.array_equal(bits(a[1]), bits(b[1])) and a[1][api.FB_COMPOSITED_C][:, :3].max() > 0 and a[2] == b[2]
    for k in STATE_KEYS:
        assert np.array_equal(bits(a[0][k]), bits(b[0][k])), k
    assert np.array_equal(bits(a[3][0]), bits(b[3][0])) and np.array_equal(a[3][1], b[3][1])
    assert not a[3][0][1].any() and not a[3][1][1].any()          # no technique with t = 1


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ["A", "B"])
def test_lens_cells_are_the_bpt_splats(started, bpt_pass, shape):
    """2. the lens block's cells and pixel plane give, by the header's splat rule, the BPT's light-tracing splat sums of the same pass as integers; as many non-zero cells
    as the BPT splatted entries, and more than none"""
    sh = SHAPES[shape]; L = sh["L"]; npx = sh["res"][0] * sh["res"][1]
    st = started[shape]["state"]; tb = st["table"]
    assert tb.shape == (J.tech_count(L), npx, 4) and st["table_pixel"].shape == (L - 1, npx)
    block = tb[M.tech_count(L):]
    sums, n_live = J.lens_splat_sums(block, st["table_pixel"], npx, 0)
    want = bpt_pass[shape]
    nonzero = (block[..., :3] > 0).any(-1)
    print("shape %s: %d non-zero lens cells, BPT queued %d camera connections and splatted %d" % (shape, nonzero.sum(), want["entries"], want["visible"]))
    assert nonzero.sum() > 0, "the scene does not exercise the lens techniques"
    assert nonzero.sum() == n_live == want["visible"] <= want["entries"]
    assert np.array_equal(sums, want["sums"].reshape(npx, 3))
    # a cell is (c, 1) or zeros, and the pixel plane names a pixel exactly where there is a cell
    assert (block[nonzero][:, 3] == 1).all() and not block[~nonzero].any()
    assert (st["table_pixel"][nonzero] < npx).all() and (st["table_pixel"][~nonzero] == NONE).all()


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ["A", "B"])
def test_eye_cells_under_the_new_weights(started, bpt_pass, shape):
    """3. per pixel, the t >= 2 cells added from zero in sink order, then the resolved splat sums, are the BPT's COMPOSITED_C of that pass on a cleared frame, bit for bit:
    pass 0 has frame weight 1, the sink adds every sample in the table's own order and the splat sums are folded in once, last"""
    sh = SHAPES[shape]; L = sh["L"]; npx = sh["res"][0] * sh["res"][1]
    st = started[shape]["state"]; tb = st["table"]
    eye = M.sink_order_sum(tb[:M.tech_count(L)], L)
    sums, _ = J.lens_splat_sums(tb[M.tech_count(L):], st["table_pixel"], npx, 0)
    assert sums.any()
    frame = T.resolve(eye, sums)          # (clears the sums)
    assert frame[:, :3].max() > 0 and np.array_equal(bits(frame), bits(bpt_pass[shape]["frame"]))
    assert not np.array_equal(bits(eye), bits(frame))          # the splats are part of that frame


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ["A", "B"])
def test_norms_brightness_seeds_and_chains_per_technique(started, shape):
    """4. st_norms, brightness and every seed from the downloaded table by the judge's integer arithmetic, bit for bit; the chains start sorted by technique, and every
    technique, the lens block included, starts within 1 of its share of the chains"""
    sh = SHAPES[shape]; L = sh["L"]; npx = sh["res"][0] * sh["res"][1]; n = sh["n_chains"]
    got = started[shape]; st = got["state"]; tb = st["table"]
    q, cdf, norms, brightness = J.st_norms(tb, L)
    assert np.array_equal(bits(got["norms"]), bits(norms)) and got["stats"]["image_brightness"] == brightness and brightness > 0
    valid = np.zeros((L + 2, L + 2), bool)
    for s, t in J.techniques(L):
        valid[t, s] = True
    assert valid[1, 2:L + 1].all() and not valid[1, :2].any() and not got["norms"][~valid].any() and not got["chains"][~valid].any()
    seeds = J.sample_seeds(cdf, n, 0)
    assert np.array_equal(st["seeds"], seeds)
    tech = seeds // npx
    assert (np.diff(tech.astype(np.int64)) >= 0).all() and np.array_equal(st["st"], J.words(L)[tech])
    assert (T.max_comp(tb.reshape(-1, 4)[seeds]) > 0).all()
    total = int(cdf[-1])
    for k, (s, t) in enumerate(J.techniques(L)):
        count = int((tech == k).sum())
        share = (int(cdf[(k + 1) * npx - 1]) - (int(cdf[k * npx - 1]) if k else 0)) / total
        print("shape %s technique (%d, %d): %d chains, n * share = %.3f" % (shape, s, t, count, n * share))
        assert got["chains"][t, s] == count and abs(count - n * share) <= 1.0, (s, t, count, n * share)
    assert got["chains"].sum() == n and got["norms"][1].sum() > 0 and got["chains"][1].sum() > 0
    # a chain that starts on (s, 1) holds, after its steps with the perturbations off, its seed's cell and pixel
    lens = tech >= M.tech_count(L)
    assert np.array_equal(st["path_pixel"][lens], st["table_pixel"].reshape(-1)[seeds[lens] - M.tech_count(L) * npx]) and (st["path_pixel"][~lens] == NONE).all()
    held = tb.reshape(-1, 4)[seeds].copy()
    held[lens, :3] = (held[lens, :3] * (F32(1.0) / F32(npx))).astype(F32)          # a t = 1 state counts as c * light_weight
    assert np.array_equal(bits(st["path_value"]), bits(held))


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ["A", "B"])
def test_technique_evaluated_alone_is_its_cell(cornell, table, started, shape):
    """5. every seed, and 512 further (path, technique) pairs of which 128 are t = 1, evaluated alone: the value is the table's cell and the pixel the pixel plane's, bit
    for bit.  Rays: a seed's path exists in full, so with the perturbations off it queues exactly max(s - 1, 0) + (t - 1) + [s > 0] rays -- s for (s, 1): no eye ray --;
    any other pair at most that"""
    sh = SHAPES[shape]; L = sh["L"]; npx = sh["res"][0] * sh["res"][1]; n = sh["n_chains"]
    st = started[shape]["state"]; tb = st["table"]; n_old = M.tech_count(L)
    path = st["seeds"] % npx

    def want_pixel(k, p):
        out = np.full(len(k), NONE, U32)
        lens = k >= n_old
        out[lens] = st["table_pixel"][k[lens] - n_old, p[lens]]
        return out
    r = make(cornell, table, shape)
    value, rays, pixel = r.mmlt_eval(st["light_u"], st["eye_u"], st["st"], with_pixels=True)
    tech = st["seeds"] // npx
    assert np.array_equal(bits(value), bits(tb.reshape(-1, 4)[st["seeds"]])) and np.array_equal(pixel, want_pixel(tech, path))
    assert rays == int(J.max_rays(st["st"]).sum())
    lens = tech >= n_old
    assert lens.any() and (pixel[lens] < npx).all()
    # the t = 1 seeds alone: s rays each, so none of them is an eye ray
    value, rays, pixel = r.mmlt_eval(st["light_u"][:, lens], st["eye_u"][:, lens], st["st"][lens], with_pixels=True)
    s1, t1 = J.unword(st["st"][lens])
    assert (t1 == 1).all() and rays == int(s1.sum()) and np.array_equal(bits(value), bits(tb.reshape(-1, 4)[st["seeds"][lens]]))
    rng = np.random.default_rng(4321)
    w = J.words(L)
    n_t1 = 0
    for lo in range(0, 512, 128):
        c = rng.integers(0, n, 128)
        k = rng.integers(n_old, len(w), 128) if lo == 0 else rng.integers(0, len(w), 128)
        value, rays, pixel = r.mmlt_eval(st["light_u"][:, c], st["eye_u"][:, c], w[k], with_pixels=True)
        want = tb[k, path[c]]
        assert np.array_equal(bits(value), bits(want)) and np.array_equal(pixel, want_pixel(k, path[c]))
        s, t = J.unword(w[k])
        n_t1 += int((t == 1).sum())
        bound = int(J.max_rays(w[k]).sum())
        assert bound == int((np.maximum(s - 1, 0) + (t - 1) + (s > 0)).sum()) and 0 < rays <= bound
        if lo == 0:
            zero = T.max_comp(want) == 0
            assert (t == 1).all() and zero.any() and (~zero).any() and rays <= int(s.sum())
    assert n_t1 >= 128
    r.close()
    stats = started[shape]["stats"]
    assert 0 < stats["rays"] <= stats["chain_length"] * int(J.max_rays(st["st"]).sum())


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

    def evaluate(a, b, st):
        # (1, 1) is no technique of the library's (only the planted walk 'with_11' proposes it): depth 0 never splats, so its value is zero and it queues nothing more
        # than its light vertex needs (no ray)
        bad = st == J.word(1, 1)
        value, rays, pixel = r.mmlt_eval(a, b, np.where(bad, J.word(0, 2), st).astype(U32), with_pixels=True)
        value[bad] = 0; pixel[bad] = NONE
        return value, rays, pixel
    opts = dict(independent_samples=0.0, light_perturbations=1, eye_perturbations=1)
    return J.replay(start["light_u"], start["eye_u"], start["st"], L, stats["chain_length"], 0, opts, F, stats["pdf_norm"], res, np.zeros((res[0] * res[1], 4), F32), perturb,
                    evaluate, norms=norms, mistake=mistake)


COUNTERS = ("accepted", "rejected", "swaps_proposed", "swaps_accepted", "rays")


def same_as_render(want, frame, st, fb, stats):
    """the names of what a replay got differently from render()"""
    out = [k for k in COUNTERS if want[k] != stats[k]]
    out += [k for k in ("st", "path_pixel", "rejections") if not np.array_equal(st[k], want[k])]
    out += [k for k in ("light_u", "eye_u", "path_value", "path_pdf") if not np.array_equal(bits(st[k]), bits(want[k]))]
    if not np.array_equal(bits(fb[api.FB_COMPOSITED_C]), bits(frame)):
        out.append("frame")
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("shape,F", [("A", 0), ("A", 2), ("B", 0), ("B", 2)])
def test_replay_of_a_render(cornell, table, started, shape, F):
    """6. all steps on the host: coordinates from the probe, values and lens pixels from mmlt_eval, acceptance, pixel and swap arithmetic from the judge -- COMPOSITED_C,
    the chains' final (s, t), their final pixels and the counters equal render()'s bit for bit.  On A with F = 2 six planted mistakes are each refused"""
    r = make(cornell, table, shape, mmlt_frequency=F)
    st, fb, stats = render_and_state(r)
    start = started[shape]["state"]
    want, frame = replay_render(r, start, stats, shape, F)
    n_swaps = sum(J.is_swap_step(F, k) for k in range(stats["chain_length"]))
    assert stats["swaps_proposed"] == n_swaps * SHAPES[shape]["n_chains"] and 0 < want["rejected"]
    assert same_as_render(want, frame, st, fb, stats) == []
    assert fb[api.FB_COMPOSITED_C][:, :3].max() > 0 and (F != 0 or np.array_equal(st["st"], start["st"]))
    assert shape != "A" or (F != 0) == bool((st["st"] != start["st"]).any())          # (B has three swap steps: too few for a move to be certain)
    t_final = J.unword(st["st"])[1]
    assert (t_final == 1).any() and ((st["path_pixel"] != NONE) == (t_final == 1)).all()          # a state's pixel is kept exactly for t = 1
    if F and shape == "A":
        s0, t0 = J.unword(start["st"])
        assert ((s0 == 0) & (t0 == 2)).any(), "no chain of path length 1: 'with_11' would not be exercised"
        assert want["into_lens"] > 0 and want["out_of_lens"] > 0
        refused = {}
        for mistake in ("pixel_from_eye", "pixel_commit", "no_stop", "with_11", "light_weight", "norm_ratio"):
            bad, bad_frame = replay_render(r, start, stats, shape, F, mistake, norms=started[shape]["norms"])
            refused[mistake] = same_as_render(bad, bad_frame, st, fb, stats)
            print("planted mistake %-15s differs in: %s" % (mistake, ", ".join(refused[mistake])))
        for mistake, diff in refused.items():
            assert diff, mistake
        # the cases that name them: a wrong pixel moves light in the frame and leaves the counters alone; a wrong walk or value changes what is accepted
        assert "frame" in refused["pixel_from_eye"] and not set(refused["pixel_from_eye"]) & set(COUNTERS)
        assert "path_pixel" in refused["pixel_commit"] and "frame" in refused["pixel_commit"] and not set(refused["pixel_commit"]) & set(COUNTERS)
        assert "st" in refused["no_stop"] and "accepted" in refused["with_11"] and "frame" in refused["light_weight"] and "swaps_accepted" in refused["norm_ratio"]
    r.close()


@pytest.mark.gpu
def test_determinism_and_the_lens_does_something(cornell, table, started):
    """7. two fresh contexts, instances 0..2, lens on with F = 2: the same bits in frame and state; lens on differs from lens off; and in render call 0 at least one swap
    into t = 1 and one out of it is accepted -- every chain's technique before and after each swap step, from the replay that reproduces the call's final techniques"""
    got = {}
    for key, lens in (("a", 1), ("b", 1), ("c", 0)):
        r = make(cornell, table, "A", mmlt_frequency=2, lens_techniques=lens)
        first = None
        for i in range(3):
            r.mmlt_render(i)
            if i == 0 and key == "a":
                first = (r.mmlt_state(), r.mmlt_stats())
                first += (replay_render(r, started["A"]["state"], first[1], "A", 2)[0],)
        got[key] = (r.mmlt_state(), r.framebuffer().copy(), r.mmlt_stats(), first)
        r.close()
    assert np.array_equal(bits(got["a"][1]), bits(got["b"][1])) and got["a"][1][api.FB_COMPOSITED_C][:, :3].max() > 0
    for k in got["a"][0]:
        assert np.array_equal(bits(got["a"][0][k]), bits(got["b"][0][k])), k
    assert got["a"][2] == got["b"][2]
    assert not np.array_equal(bits(got["a"][1][api.FB_COMPOSITED_C]), bits(got["c"][1][api.FB_COMPOSITED_C]))
    for c in (0, 1, 2, 3, 4):
        assert not got["a"][1][c].any()          # COMPOSITED_C alone is written
    state0, stats0, want = got["a"][3]
    assert np.array_equal(state0["st"], want["st"]) and stats0["swaps_accepted"] == want["swaps_accepted"]
    print("render call 0: %d accepted swaps into t = 1, %d out of it, of %d accepted" % (want["into_lens"], want["out_of_lens"], stats0["swaps_accepted"]))
    assert want["into_lens"] > 0 and want["out_of_lens"] > 0


# the smallest power of two, from 64, at which the data scaled by 1.1 fall outside for F = 0 and for F = 2 (measured on the MI355X, DESIGN.md 6h: at 64 passes the
# scaled data of F = 2 reach only 4.92)
N_PASSES = 128


def block_sums(frame, res):
    img = frame[:, :3].astype(np.float64).sum(1).reshape(res[1], res[0])
    return img.reshape(res[1] // 8, 8, res[0] // 8, 8).sum((1, 3)).reshape(-1)


def estimator_passes(cornell, table, n_passes, frequencies=(0, 2)):
    """the block sums of n_passes independent passes (instances 0 .. n_passes - 1, each on a cleared frame) of the BPT with light tracing on and of MMLT with the lens
    techniques per swap frequency"""
    res = SHAPES["A"]["res"]

    def passes(r, render):
        out = []
        for i in range(n_passes):
            r.clear_framebuffer()
            render(i)
            out.append(block_sums(r.framebuffer()[api.FB_COMPOSITED_C] * F32(i + 1), res))
        r.close()
        return np.array(out)
    b = make_bpt(cornell, table, "A")
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
def test_estimator_agrees_with_bpt_with_light_tracing(cornell, table):
    """8. N_PASSES independent passes each of MMLT with the lens techniques (F = 0 and F = 2) and of the BPT with light_tracing = 1, single_connection = 0; the sums over
    the sixteen 8 x 8 blocks agree within 5 standard errors in EVERY block, and the same data scaled by 1.1 do not (the power of the check).  Measured figures: DESIGN.md 6h."""
    B, P = estimator_passes(cornell, table, N_PASSES)
    for F in P:
        z, z_scaled, tP, tB = estimator_z(B, P[F], N_PASSES)
        print("estimator lens on, F = %d, %d passes: worst |z| = %.2f, worst |z| of the data scaled by 1.1 = %.2f, total M %.4f B %.4f" % (F, N_PASSES, z.max(), z_scaled.max(), tP, tB))
        assert (z <= 5.0).all(), (F, z)
        assert (z_scaled > 5.0).any(), (F, z_scaled)


@pytest.mark.gpu
def test_refusals_and_black_scene(cornell, table):
    """9. what init refuses names the option, the table's bound with the larger count; a scene without emitters renders without a fault and leaves the frame rescaled"""
    L = 4

    def refused(word, pixels=None, **kw):
        with pytest.raises(fa.FptError) as e:
            fa.Renderer(cornell, 16, 16, fa.default_options(L), table=table, pixels=pixels,
                        mmlt_options=fa.default_mmlt_options(L, **dict(dict(n_chains=64, spp=4, lens_techniques=1), **kw)))
        assert "fpt_mmlt_init" in str(e.value) and word in str(e.value), str(e.value)
    refused("use_vpls", use_vpls=1)
    refused("pixels", pixels=np.arange(128, dtype=U32))
    refused("n_chains", n_chains=0)
    refused("n_chains", n_chains=1 << 24, spp=1 << 20)
    refused("spp", n_chains=300, spp=1)
    refused("lens_techniques", lens_techniques=2)
    dark = copy.copy(cornell); dark.materials = cornell.materials.copy(); dark.materials["emissive"][:] = 0.0
    r = fa.Renderer(dark, 16, 16, fa.default_options(L), table=table, mmlt_options=fa.default_mmlt_options(L, n_chains=64, spp=4, mmlt_frequency=2, lens_techniques=1))
    # L = 15 has 120 cells per pixel without and 134 with the lens block: 32051995 pixels (6410399 x 5) fit the one and not the other
    big = type(r.view).from_buffer_copy(r.view); big.res_x = 6410399; big.res_y = 5
    o = fa.default_mmlt_options(15, n_chains=64, spp=4, lens_techniques=1)
    assert r.L.fpt_mmlt_init(r.ctx, C.byref(o), C.byref(big), r.samples_dir.encode(), None, C.c_uint32(0)) != 0
    msg = r.L.fpt_last_error(r.ctx).decode()
    assert "fpt_mmlt_init" in msg and "technique table" in msg and "32 bits" in msg and "lens_techniques" in msg, msg
    with pytest.raises(fa.FptError):
        r.mmlt_render(0)          # the refused init left no renderer behind
    r._check(r.L.fpt_mmlt_init(r.ctx, C.byref(r.mmlt_options), C.byref(r.view), r.samples_dir.encode(), None, C.c_uint32(0)))
    r.fb[api.FB_COMPOSITED_C] = 1.0
    r.mmlt_render(1, sync=True)
    fb = r.framebuffer(); stats = r.mmlt_stats(); norms, chains = r.mmlt_st_norms()
    assert stats["image_brightness"] == 0 and stats["accepted"] == 0 and stats["rejected"] == 0 and stats["rays"] == 0 and not norms.any() and not chains.any()
    assert np.array_equal(bits(fb[api.FB_COMPOSITED_C]), bits(np.full((256, 4), 0.5, F32)))
    assert (r.mmlt_state()["table_pixel"] == NONE).all()
    r.close()
    # L = 1 with the switch on is legal and adds nothing: the one technique (0, 2)
    r = fa.Renderer(cornell, 16, 16, fa.default_options(1), table=table, mmlt_options=fa.default_mmlt_options(1, n_chains=64, spp=4, lens_techniques=1))
    r.mmlt_render(0, sync=True)
    st = r.mmlt_state()
    norms, chains = r.mmlt_st_norms()
    assert st["table"].shape[0] == 1 and st["table_pixel"].shape == (0, 256) and not norms[1].any() and not chains[1].any()
    assert (st["st"] == (J.word(0, 2) if r.mmlt_stats()["image_brightness"] > 0 else 0)).all()
    r.close()


@pytest.mark.gpu
def test_cli_mmlt_lens_writes_the_renderers_image(cornell, tmp_path, table):
    """`fermat_hip -i ... -mmlt -mmlt-lens 1 -mmlt-swaps 2 -passes N -o ...` writes the image the Renderer gives for the same options, and prints the t = 1 rows"""
    from fermat_amd import scene
    exe = os.path.join(ROOT, "fermat_amd", "bin", "fermat_hip")
    d = os.path.join(scene.DATA_DIR, "scenes", "CornellBox")
    out = str(tmp_path / "mmlt_lens")
    run = subprocess.run([exe, "-i", os.path.join(d, "CornellBox-JP.obj"), "-c", os.path.join(d, "camera-frontal.txt"), "-r", "48", "36", "-mmlt", "-chains", "1", "-spp", "4",
                          "-pl", "4", "-mmlt-swaps", "2", "-mmlt-lens", "1", "-passes", "2", "-o", out], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr[-2000:]
    assert "st chains" in run.stderr and "[0,2] :" in run.stderr and "[2,1] :" in run.stderr and "[4,1] :" in run.stderr and "[1,1] :" not in run.stderr
    r = fa.Renderer(cornell, 48, 36, fa.default_options(4), table=table, mmlt_options=fa.default_mmlt_options(4, n_chains=1024, spp=4, mmlt_frequency=2, lens_techniques=1))
    for i in range(3):
        r.mmlt_render(i)
    want = r.to_rgba()[..., :3]
    got = (scene.load_tga(out + ".tga")[..., :3] * 255.0 + 0.5).astype(np.uint8)
    assert want.max() > 0 and np.array_equal(got, want)
    r.close()
