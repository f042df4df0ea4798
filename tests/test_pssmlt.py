"""The primary-sample-space Metropolis renderer (`-pssmlt`: fpt_mlt.hip, fpt_mlt_api.cpp, the chain mode of fpt_bpt.hip) against exact invariants.

There is no twin restatement of the renderer: the bidirectional kernels it runs on are judged on their own (tests/test_bpt_truth.py), so the new code is held
to (a) its small kernels against a numpy judge, bit for bit (tests/mlt_truth.py), (b) identities with the judged BPT -- the presampling pass IS a BPT pass, a
seed re-evaluated from its recovered coordinates IS its presampled value --, (c) a replay of a whole render call from the probe's coordinates, the library's
own path evaluation and the judge's acceptance arithmetic, and (d) the estimator's mean against the BPT's.

Shapes: A = CornellBox-JP 32 x 32, max_path_length 4, 256 chains, 4 spp (chain length 16); B = 16 x 16, 300 chains, 8 spp (chain length 6: more chains than
pixels, a partial last workgroup)."""
import copy
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mlt_truth as T  # noqa: E402

import fermat_amd as fa  # noqa: E402
from fermat_amd import api  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
U32 = np.uint32
L = 4
SHAPES = {"A": dict(res=(32, 32), n_chains=256, spp=4), "B": dict(res=(16, 16), n_chains=300, spp=8)}
NAMES = ("fpt_pssmlt_init", "fpt_pssmlt_render", "fpt_pssmlt_get_stats", "fpt_pssmlt_download", "fpt_pssmlt_debug_eval", "fpt_debug_mlt")


def bits(a):
    return np.ascontiguousarray(a).view(U32)


# ---- 1. CPU -------------------------------------------------------------------------------------------------------------------------------------------------
def test_entry_points_declared_exported_and_judge_sound():
    text = open(os.path.join(ROOT, "include", "fermat_pt_hip.h")).read()
    lib = fa.lib()
    for n in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % n, text), "not declared: " + n
        assert n in api.ENTRY_POINTS and hasattr(lib, n), "not exported: " + n
    assert re.search(r"typedef struct fpt_pssmlt_options", text) and re.search(r"typedef struct fpt_pssmlt_stats", text)
    o = fa.api.default_pssmlt_options(L)
    assert o.n_chains == 65536 and o.spp == 4 and o.bpt.max_path_length == L and abs(o.radius - 0.01) < 1e-9
    T.self_check()


# ---- GPU ----------------------------------------------------------------------------------------------------------------------------------------------------
def options(shape, **kw):
    s = SHAPES[shape]
    return fa.api.default_pssmlt_options(L, n_chains=s["n_chains"], spp=s["spp"], **kw)


def bpt_base_options():
    return fa.default_bpt_options(L, light_tracing=0.0, single_connection=0)


def make(cornell, table, shape, **kw):
    s = SHAPES[shape]
    return fa.Renderer(cornell, s["res"][0], s["res"][1], fa.default_options(L), table=table, pssmlt_options=options(shape, **kw))


@pytest.fixture(scope="module")
def probe(cornell, table):
    r = fa.Renderer(cornell, 8, 8, fa.default_options(2), table=table, pssmlt_options=fa.api.default_pssmlt_options(2, n_chains=8, spp=1))
    yield r
    r.close()


def perturb_on_device(r, u, mutation, instance=0, step=0, m=None, chain=None, dim=None, radius=0.01):
    u = np.ascontiguousarray(u, F32).reshape(-1)
    n = len(u)
    chain = np.zeros(n, U32) if chain is None else np.ascontiguousarray(chain, U32)
    dim = np.zeros(n, U32) if dim is None else np.ascontiguousarray(dim, U32)
    out = r.debug_mlt(0, [u, None if m is None else np.ascontiguousarray(m, F32), chain, dim, np.zeros(n, F32), np.zeros(n, F32)],
                      params=(mutation, instance, step, int(F32(radius).view(U32))), n=n)
    return out[4], out[5]


@pytest.mark.gpu
def test_probe_perturbed_u(probe):
    """2. Null and Independent bit for bit; Cauchy within the judge's derived bound on the circle, and always in [0, 1)"""
    rng = np.random.default_rng(3)
    special = F32([0.0, 1e-45, 0.25, np.nextafter(F32(0.5), F32(0)), 0.5, np.nextafter(F32(0.5), F32(1)), 1 - 2.0 ** -24])
    gu, gm = np.meshgrid(special, special)
    u = np.concatenate([gu.ravel(), rng.random(4096, dtype=F32)]).astype(F32)
    m = np.concatenate([gm.ravel(), rng.random(4096, dtype=F32)]).astype(F32)
    out0, _ = perturb_on_device(probe, u, 0, m=m)
    out2, _ = perturb_on_device(probe, u, 2, m=m)
    assert np.array_equal(bits(out0), bits(u)) and np.array_equal(bits(out2), bits(m))
    out1, _ = perturb_on_device(probe, u, 1, m=m)
    assert (out1 >= 0).all() and (out1 < 1).all()
    ref, B = T.cauchy_reference(u, m, 0.01)
    d = T.circular_distance(out1, ref)
    decided = T.MARGIN * B < 0.5
    print("cauchy: %d of %d decided, worst distance / bound = %.3g" % (decided.sum(), len(u), float((d[decided] / (T.MARGIN * B[decided])).max())))
    assert decided.sum() > 4000 and (d[decided] <= T.MARGIN * B[decided]).all()
    # the mutation numbers themselves, where they are computed: the counter-based function
    chain = rng.integers(0, 1 << 20, 2048).astype(U32); dim = rng.integers(0, 31, 2048).astype(U32)
    out, mm = perturb_on_device(probe, np.zeros(2048, F32), 2, instance=5, step=9, chain=chain, dim=dim)
    want = T.mutation_number(5, 9, chain, dim)
    assert np.array_equal(bits(mm), bits(want)) and np.array_equal(bits(out), bits(want))


@pytest.mark.gpu
def test_probe_seeds(probe):
    """3. the integer CDF, the brightness and every seed equal the judge's"""
    v = T.hand_made_values()
    q, cdf, brightness = T.seed_cdf(v)
    for n_seeds in (7, 300):
        _, d_cdf, d_seeds = probe.debug_mlt(1, [v, np.zeros(len(v), np.uint64), np.full(n_seeds, 0xFFFFFFFF, U32)], params=(n_seeds,), n=len(v))
        assert np.array_equal(d_cdf, cdf)
        assert np.array_equal(d_seeds, T.sample_seeds(cdf, n_seeds))
        assert F32(np.float64(int(d_cdf[-1])) * 2.0 ** -32 / len(v)) == brightness
    z = np.zeros((1000, 4), F32)
    _, d_cdf, d_seeds = probe.debug_mlt(1, [z, np.ones(1000, np.uint64), np.full(7, 0xFFFFFFFF, U32)], params=(7,), n=1000)
    assert not d_cdf.any() and (d_seeds == 0xFFFFFFFF).all()          # a black frame: no seed is written


@pytest.mark.gpu
def test_probe_accept_reject(probe):
    """4. splat integers, resolved frame, values, pdfs, rejection counters and copied coordinates, bit for bit, on chains that meet every branch"""
    h = T.hand_made_chains()
    Lh, res = h["L"], h["res"]; dims = (Lh + 1) * 3; n = h["light_u"].shape[1]; npx = res[0] * res[1]
    norm = F32(0.37)
    # mutation Independent with known numbers: the device's proposals are the mutation numbers themselves, which the judge computes exactly
    for instance, step, mutation, lp, ep in ((0, 3, 2, 1, 1), (2, 1, 2, 0, 1), (1, 0, 0, 1, 1)):
        chains = np.arange(n, dtype=U32)
        d_idx = np.arange(dims, dtype=U32)[:, None]
        nl = T.mutation_number(instance, step, chains[None, :], d_idx) if (mutation and lp) else h["light_u"].copy()
        ne = T.mutation_number(instance, step, chains[None, :], d_idx + U32(dims)) if (mutation and ep) else h["eye_u"].copy()
        if not (mutation and ep):
            ne = h["eye_u"].copy()
        st = T.new_state(h["light_u"], h["eye_u"]); st["path_value"][:] = h["path_value"]; st["path_pdf"][:] = h["path_pdf"]
        st["rejections"][:] = 2
        splat = np.zeros((npx, 3), np.int64)
        u_ar = T.mutation_number(instance, step, chains, U32(dims * 2))
        T.accept_reject(st, h["new_value"], nl, ne, u_ar, norm, instance, res, splat)
        frame0 = np.random.default_rng(5).random((npx, 4), dtype=F32)
        want_splat = splat.copy()
        want_frame = T.resolve(frame0, splat)
        out = probe.debug_mlt(2, [h["light_u"], h["eye_u"], h["new_value"], h["path_value"], h["path_pdf"], np.full(n, 2, U32), np.zeros((npx, 3), np.int64),
                                  np.zeros((npx, 3), np.int64), frame0, np.zeros(2, np.uint64)],
                              params=(Lh, instance, step, mutation, lp, ep, int(F32(0.01).view(U32)), int(norm.view(U32)), res[0], res[1]), n=n)
        assert np.array_equal(out[7], want_splat), (instance, step)
        assert not out[6].any() and np.array_equal(bits(out[8]), bits(want_frame))
        assert np.array_equal(bits(out[3]), bits(st["path_value"])) and np.array_equal(bits(out[4]), bits(st["path_pdf"]))
        assert np.array_equal(out[5], st["rejections"])
        assert np.array_equal(bits(out[0]), bits(st["light_u"])) and np.array_equal(bits(out[1]), bits(st["eye_u"]))
        assert [int(x) for x in out[9]] == [st["accepted"], st["rejected"]]
    # the hand-made branches themselves, with the proposals as the current coordinates (Null): what test 1 asserts of the judge holds of the device
    assert np.isnan(h["new_value"][3]).all()


def render_and_state(r, instance=0):
    r.pssmlt_render(instance, sync=True)
    return r.pssmlt_state(), r.framebuffer(), r.pssmlt_stats()


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ["A", "B"])
def test_presampling_pass_is_a_bpt_pass(cornell, table, shape):
    """5. presample[p].xyz == COMPOSITED_C[p].xyz of bpt_render(0) on a fresh context with the same options: the same sums in the same order from zero"""
    r = make(cornell, table, shape)
    st, _, stats = render_and_state(r)
    s = SHAPES[shape]
    b = fa.Renderer(cornell, s["res"][0], s["res"][1], fa.default_options(L), table=table, bpt_options=bpt_base_options())
    b.bpt_render(0, sync=True)
    fb = b.framebuffer()
    assert fb[api.FB_COMPOSITED_C][:, :3].max() > 0
    assert np.array_equal(bits(st["presample"][:, :3]), bits(fb[api.FB_COMPOSITED_C][:, :3]))
    q, cdf, brightness = T.seed_cdf(st["presample"])
    assert stats["image_brightness"] == brightness and np.array_equal(st["seeds"], T.sample_seeds(cdf, s["n_chains"]))
    r.close(); b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ["A", "B"])
def test_seed_path_re_evaluated(cornell, table, shape):
    """6. perturbations off: every step re-evaluates the seed path from its recovered coordinates, and gets the presampled value back bit for bit"""
    s = SHAPES[shape]; res = s["res"]; n = s["n_chains"]
    r = make(cornell, table, shape, light_perturbations=0, eye_perturbations=0)
    st, fb, stats = render_and_state(r)
    want = st["presample"][st["seeds"]]
    assert np.array_equal(bits(st["path_value"]), bits(want))
    assert (st["rejections"][T.max_comp(want) > 0] == 0).all() and (T.max_comp(want) > 0).all()
    length = T.chain_length(s["spp"], res[0] * res[1], n)
    assert stats["chain_length"] == length and stats["pdf_norm"] == T.pdf_norm(stats["image_brightness"], res[0] * res[1], length, n)
    # the frame from seeds, presample and pdf_norm alone: the eye coordinates 3 and 4 of a seed are its pixel's (px + jitter) / res
    px = st["seeds"] % res[0]; py = st["seeds"] // res[0]
    assert np.array_equal(T.quantize(st["eye_u"][3], res[0]), px) and np.array_equal(T.quantize(st["eye_u"][4], res[1]), py)
    assert not st["eye_u"][:3].any()
    _, frame = T.replay(st["light_u"], st["eye_u"], L, length, 0, dict(independent_samples=0.01, light_perturbations=0, eye_perturbations=0), stats["pdf_norm"], res,
                        np.zeros((res[0] * res[1], 4), F32), None, lambda a, b: want)
    assert np.array_equal(bits(fb[api.FB_COMPOSITED_C]), bits(frame))
    for c in (0, 1, 2, 3, 4):
        assert not fb[c].any()
    r.close()


def replay_render(r, st0_light, st0_eye, stats, res, n_steps, opts, mistake=None):
    dims = (L + 1) * 3
    n = st0_light.shape[1]
    chain = np.tile(np.arange(n, dtype=U32), dims)

    def perturb(u, offset, mutation, step):
        dim = np.repeat(np.arange(dims, dtype=U32) + U32(offset), n)
        out, _ = perturb_on_device(r, u.reshape(-1), mutation, instance=0, step=step, chain=chain, dim=dim)
        return out.reshape(dims, n)
    return T.replay(st0_light, st0_eye, L, n_steps, 0, opts, stats["pdf_norm"], res, np.zeros((res[0] * res[1], 4), F32), perturb, lambda a, b: r.pssmlt_eval(a, b), mistake)


def seed_coordinates(cornell, table, shape):
    """the coordinates a render call starts its chains from: those a render with the perturbations off leaves (test 6 checks them)"""
    r = make(cornell, table, shape, light_perturbations=0, eye_perturbations=0)
    st, _, _ = render_and_state(r)
    r.close()
    return st["light_u"], st["eye_u"]


@pytest.fixture(scope="module")
def seeds_A(cornell, table):
    return seed_coordinates(cornell, table, "A")


@pytest.mark.gpu
@pytest.mark.parametrize("independent", [0.0, 0.5])
def test_replay_of_a_render(cornell, table, seeds_A, independent):
    """7. all 16 steps on the host: coordinates from the probe, values from pssmlt_eval, acceptance and sums from the judge -- equal to render() bit for bit"""
    s = SHAPES["A"]; res = s["res"]
    r = make(cornell, table, "A", independent_samples=independent)
    st, fb, stats = render_and_state(r)
    opts = dict(independent_samples=independent, light_perturbations=1, eye_perturbations=1)
    kinds = [T.mutation_type(independent, 0, k) for k in range(stats["chain_length"])]
    assert kinds[0] == 0 and 1 in kinds and (independent < 0.5 or 2 in kinds)
    want, frame = replay_render(r, seeds_A[0], seeds_A[1], stats, res, stats["chain_length"], opts)
    assert 0 < want["rejected"] and want["accepted"] > s["n_chains"]
    assert (want["accepted"], want["rejected"]) == (stats["accepted"], stats["rejected"])
    for k in ("light_u", "eye_u", "path_value", "path_pdf"):
        assert np.array_equal(bits(st[k]), bits(want[k])), k
    assert np.array_equal(st["rejections"], want["rejections"])
    assert np.array_equal(bits(fb[api.FB_COMPOSITED_C]), bits(frame))
    r.close()


@pytest.mark.gpu
def test_mistakes_refused(cornell, table, seeds_A):
    """the replay with a mistake in it must disagree with render(): (a) the acceptance inequality turned round, (b) old and new pixel swapped, (c) the eye side's
    mutation dims not offset by (L+1)*3"""
    s = SHAPES["A"]; res = s["res"]
    r = make(cornell, table, "A")
    st, fb, stats = render_and_state(r)
    opts = dict(independent_samples=0.0, light_perturbations=1, eye_perturbations=1)
    for mistake in ("inequality", "pixels", "offset"):
        want, frame = replay_render(r, seeds_A[0], seeds_A[1], stats, res, stats["chain_length"], opts, mistake)
        assert not np.array_equal(bits(fb[api.FB_COMPOSITED_C]), bits(frame)), mistake
    r.close()


@pytest.mark.gpu
def test_determinism(cornell, table):
    """8. two fresh contexts, instances 0..3: the same bits in frame and state"""
    got = []
    for _ in range(2):
        r = make(cornell, table, "A")
        for i in range(4):
            r.pssmlt_render(i)
        st = r.pssmlt_state(); fb = r.framebuffer()
        got.append((st, fb.copy()))
        r.close()
    assert np.array_equal(bits(got[0][1]), bits(got[1][1])) and got[0][1][api.FB_COMPOSITED_C][:, :3].max() > 0
    for k in got[0][0]:
        assert np.array_equal(bits(got[0][0][k]), bits(got[1][0][k])), k


N_PASSES = 64


def block_sums(frame, res):
    img = frame[:, :3].astype(np.float64).sum(1).reshape(res[1], res[0])
    return img.reshape(res[1] // 8, 8, res[0] // 8, 8).sum((1, 3)).reshape(-1)


@pytest.mark.gpu
def test_estimator_agrees_with_bpt(cornell, table):
    """9. N_PASSES independent passes each of PSSMLT (defaults, and independent samples only) and of BPT with the same options; the sums over the sixteen 8 x 8 blocks
    agree within 5 standard errors in EVERY block, and the same data scaled by 1.1 do not (the power of the check).  Measured figures: DESIGN.md."""
    res = SHAPES["A"]["res"]

    def passes(r, render):
        out = []
        for i in range(N_PASSES):
            r.clear_framebuffer()
            render(i)
            out.append(block_sums(r.framebuffer()[api.FB_COMPOSITED_C] * F32(i + 1), res))
        r.close()
        return np.array(out)
    b = fa.Renderer(cornell, res[0], res[1], fa.default_options(L), table=table, bpt_options=bpt_base_options())
    B = passes(b, lambda i: b.bpt_render(i, sync=True))
    mB = B.mean(0); seB = B.std(0, ddof=1) / np.sqrt(N_PASSES)
    for name, kw in (("defaults", {}), ("independent", dict(independent_samples=1.0))):
        r = make(cornell, table, "A", **kw)
        P = passes(r, lambda i: r.pssmlt_render(i, sync=True))
        mP = P.mean(0); seP = P.std(0, ddof=1) / np.sqrt(N_PASSES)
        z = np.abs(mP - mB) / np.sqrt(seP ** 2 + seB ** 2)
        z_scaled = np.abs(1.1 * mP - mB) / np.sqrt((1.1 * seP) ** 2 + seB ** 2)
        print("estimator %s: worst |z| = %.2f, worst |z| of the data scaled by 1.1 = %.2f, total P %.4f B %.4f" % (name, z.max(), z_scaled.max(), mP.sum(), mB.sum()))
        assert (z <= 5.0).all(), (name, z)
        assert (z_scaled > 5.0).any(), (name, z_scaled)


@pytest.mark.gpu
def test_refusals_and_black_scene(cornell, table):
    """10. what init refuses names the option; a scene without emitters renders without a fault and leaves the frame rescaled only"""
    def refused(word, pixels=None, **kw):
        with pytest.raises(fa.FptError) as e:
            fa.Renderer(cornell, 16, 16, fa.default_options(L), table=table, pixels=pixels, pssmlt_options=fa.api.default_pssmlt_options(L, **dict(dict(n_chains=64, spp=4), **kw)))
        assert word in str(e.value), str(e.value)
    refused("use_vpls", use_vpls=1)
    refused("pixels", pixels=np.arange(128, dtype=U32))
    refused("n_chains", n_chains=0)
    refused("spp", n_chains=300, spp=1)
    dark = copy.copy(cornell); dark.materials = cornell.materials.copy(); dark.materials["emissive"][:] = 0.0
    r = fa.Renderer(dark, 16, 16, fa.default_options(L), table=table, pssmlt_options=fa.api.default_pssmlt_options(L, n_chains=64, spp=4))
    r.fb[api.FB_COMPOSITED_C] = 1.0
    r.pssmlt_render(1, sync=True)
    fb = r.framebuffer(); stats = r.pssmlt_stats()
    assert stats["image_brightness"] == 0 and stats["accepted"] == 0 and stats["rejected"] == 0
    assert np.array_equal(bits(fb[api.FB_COMPOSITED_C]), bits(np.full((256, 4), 0.5, F32)))
    r.close()


@pytest.mark.gpu
def test_cli_pssmlt_writes_the_renderers_image(cornell, tmp_path, table):
    """`fermat_hip -i ... -pssmlt -passes N -o ...` writes an image: the one the Renderer gives for the same options (-chains counts in units of 1024)"""
    import subprocess
    from fermat_amd import scene
    exe = os.path.join(ROOT, "fermat_amd", "bin", "fermat_hip")
    d = os.path.join(scene.DATA_DIR, "scenes", "CornellBox")
    out = str(tmp_path / "pssmlt")
    run = subprocess.run([exe, "-i", os.path.join(d, "CornellBox-JP.obj"), "-c", os.path.join(d, "camera-frontal.txt"), "-r", "48", "36", "-pssmlt", "-chains", "1", "-spp", "4",
                          "-pl", "4", "-is", "0.25", "-passes", "2", "-o", out], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr[-2000:]
    r = fa.Renderer(cornell, 48, 36, fa.default_options(4), table=table, pssmlt_options=fa.api.default_pssmlt_options(4, n_chains=1024, spp=4, independent_samples=0.25))
    for i in range(3):
        r.pssmlt_render(i)
    want = r.to_rgba()[..., :3]
    got = (scene.load_tga(out + ".tga")[..., :3] * 255.0 + 0.5).astype(np.uint8)
    assert want.max() > 0 and np.array_equal(got, want)
    r.close()
