"""The traversal kernels' hand-out of rays -- ticket draws, stealing, the partial-wave refill, the retire block -- at sizes a test can afford.

A traversal launch of n rays on a grid of `blocks` blocks takes the path without atomics (one fixed 64-ray batch per wave) whenever n <= 256 blocks, and every launch
site sizes its grid from the context's persistent grid, 7 blocks per CU: below 458 752 rays on a 256-CU part nothing ever draws a ticket.  Every other test of what
the kernels return is below that size or a full-size frame.  Here the grid is capped (Renderer.debug_set_trace_blocks) at 1 and 3 blocks -- 4 and 12 waves; at 12
waves wave_id % 8 wraps -- so that a few hundred rays run on tickets, and since the kernels' answers do not depend on which lane takes which ray, the capped
answers must be the uncapped ones bit for bit.  tests/trace_schedule_truth.py restates the hand-out in integers; the eight ticket counters read back after every
plain launch (Renderer.debug_trace_tickets) must satisfy its final_counters: that is what shows that a capped launch really drew tickets and exhausted every shard.

  * CPU leg: the judge's self-checks, its constants against the kernel's text, the two entry points, and the ray set's properties (with the oracle's hits judged).
  * (a) plain launches (CLOSEST, ANY, bits, counted) on one set of 5000 rays, by prefixes, on every tree and both intersectors.
  * (b) the queue modes through the renderers: PT sequential / in flight / two lanes, PSFPT, BPT -sc 0 / 1, one -mmlt call, capped against uncapped and the oracle.
  * (c) the knob: refusal, restore, flush.
"""
import functools
import os
import re

import numpy as np
import pytest

import fermat_amd as fa
from fermat_amd import api, scene

import test_trace_truth as ttt
import trace_schedule_truth as J
import trace_truth as tt
import watertight_spec as wt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAPS = (1, 3)
PREFIXES = (256, 257, 320, 768, 769, 2049, 5000)
N_RAYS = 5000
SCENES = ("icosphere", "needles")
TREES = ["quality", "fast", "trbvh", "quality+refit"]
NAN_NEAR = (9, 300, 2050, 4990)          # rays with a NaN origin (the empty-interval branch at the refill): the first ray at or after each that crosses the scene


@pytest.fixture(autouse=True)
def _no_override(monkeypatch):
    """the tests choose intersector and build mode themselves"""
    monkeypatch.delenv("FPT_INTERSECTOR", raising=False)
    monkeypatch.delenv("FPT_BVH_BUILD", raising=False)


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# the ray set

def away_lanes(n=N_RAYS, seed=5):
    """which rays start outside the scene and point away from it: in every aligned group of 64 indices 16 to 23 of them, at random lanes"""
    rng = np.random.default_rng(seed)
    away = np.zeros(n, bool)
    for g in range(0, n, 64):
        size = min(64, n - g)
        k = min(size, 16 + int(rng.integers(0, 8)))
        away[g + rng.choice(size, k, replace=False)] = True
    return away


def nan_rays(away):
    return np.array([i + int(np.flatnonzero(~away[i:])[0]) for i in NAN_NEAR if i < len(away)], np.int64)


def schedule_rays(s, n=N_RAYS, seed=77):
    """(closest-hit rays, any-hit rays, away): one set built so that a wave on tickets must refill around live lanes.

    Every origin lies 1.5 extents from the centre of the scene's box, whose corners are 0.87 extents from it: outside (and outside the box of the moved mesh).
    `away` rays point straight away from the centre.  Every point of such a ray is farther from the centre than any box of the tree, so its root step misses all
    eight children and the ray finishes in the first iteration of the burst.  The other rays aim at a point of the central half of the box and cross the whole
    scene (tmax 1e30); those that hit something need more than one iteration, every tree here being deeper than one level.

    What follows from the kernel's text: a wave that drew a chunk of 64 or more gives each lane a ray and is not dry; after the first iteration of the burst its
    16 or more `away` lanes are idle and other lanes are live, so `64 - n_busy >= REFILL_MIN` ends the burst, the retire block writes the finished lanes, and the
    refill hands the idle lanes -- by rank among them -- the next rays of the chunk while the live lanes keep their registers.  On the static path the same set
    just runs one batch per wave.  The any-hit rays are the same rays with shadow masks 0x1 / 0x2 in turn."""
    rng = np.random.default_rng(seed)
    lo, hi, ext = ttt._extent(s)
    c = 0.5 * (lo + hi)
    u = ttt._unit(rng, n)
    org = c + 1.5 * ext * u
    target = c + 0.5 * (hi - lo) * (rng.random((n, 3)) - 0.5)
    d = target - org
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    away = away_lanes(n)
    d[away] = u[away]
    rays = ttt._make(org, d, 5e-4 * ext, 1e30)
    nan = nan_rays(away)
    rays["origin"][nan, 0] = np.nan
    shadow = rays.copy()
    shadow["mask"] = np.where(np.arange(n) % 2 == 0, 0x2, 0x1).astype(np.uint32)
    return rays, shadow, away


@functools.lru_cache(maxsize=None)
def case(key, moved=False):
    """scene (shadow masks 0, 1, 2 in turn; `moved`: every vertex moved as test_trace_truth._moved does), the rays (built on the unmoved scene), the fp64 truths
    and the watertight specification's answers.  Computed once, shared by every test, left unchanged"""
    s0 = ttt.masked(ttt.get_scene(key))
    rays, shadow, away = schedule_rays(s0)
    s = ttt._with_vertices(s0, ttt._moved(s0)) if moved else s0
    with np.errstate(all="ignore"):
        T = tt.truth(s.vertex_indices, s.vertex_data, rays)
        TA = tt.truth(s.vertex_indices, s.vertex_data, shadow, shadow=True)
        W = wt.closest(s.vertex_indices, s.vertex_data, rays)
        WA = wt.occluded(s.vertex_indices, s.vertex_data, shadow)
    return dict(scene=s, rays=rays, shadow=shadow, away=away, T=T, TA=TA, W=W, WA=WA)


def _prefix(T, n):
    return {k: v[:n] for k, v in T.items()}


def _same_hits(a, b):
    return all(np.array_equal(np.ascontiguousarray(a[f]).view(np.uint32), np.ascontiguousarray(b[f]).view(np.uint32)) for f in ("t", "triId", "u", "v"))


def _first_difference(a, b):
    bad = np.zeros(len(a), bool)
    for f in ("t", "triId", "u", "v"):
        bad |= np.ascontiguousarray(a[f]).view(np.uint32) != np.ascontiguousarray(b[f]).view(np.uint32)
    i = int(np.flatnonzero(bad)[0])
    return "%d of %d rays differ, the first is ray %d: %s instead of %s" % (bad.sum(), len(a), i, a[i], b[i])


def _unpack(bits, n):
    i = np.arange(n)
    return ((bits[i >> 5] >> (i & 31)) & 1).astype(bool)


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# CPU leg

def test_schedule_judge_self_checks():
    report = J.self_check()
    assert report[257, 1] == (8, False, 64) and report[458753, 1792][1] is False and report[458752, 1792][1] is True
    # every prefix of the GPU leg, at the grid rt_launch gives it under each cap
    for cap in CAPS:
        for n in PREFIXES:
            J.covers_once(n, J.launch_blocks(n, cap))
    # the non-vacuity of the GPU leg: which (cap, n) run on tickets
    on_tickets = {cap: [n for n in PREFIXES if not J.is_static(n, J.launch_blocks(n, cap))] for cap in CAPS}
    assert on_tickets == {1: [257, 320, 768, 769, 2049, 5000], 3: [769, 2049, 5000]}
    # the three chunk sizes between the clamps are all met: 64, 128, 256
    assert {J.chunk_of(n, J.launch_blocks(n, cap)) for cap in CAPS for n in on_tickets[cap]} == {64, 128, 256}


def test_schedule_judge_has_the_kernels_constants():
    """the judge imports nothing, so its constants are compared with the kernel's text here: a change of one without the other fails"""
    text = open(os.path.join(ROOT, "fermat_amd", "csrc", "fpt_trace_kernel.inc")).read()
    host = open(os.path.join(ROOT, "fermat_amd", "csrc", "fpt_host.h")).read()
    assert int(re.search(r"#define FPT_REFILL_MIN (\d+)", text).group(1)) == J.REFILL_MIN
    assert int(re.search(r"#define FPT_CHUNK_MAX (\d+)", text).group(1)) == J.CHUNK_MAX
    assert int(re.search(r"TICKET_SHARDS = (\d+);", text).group(1)) == J.SHARDS
    assert int(re.search(r"TRACE_BLOCK = (\d+);", text).group(1)) == J.WAVES_PER_BLOCK * J.WAVE
    assert "static_batches = n_rays <= total_waves * 64u;" in text and "((n_rays / (total_waves * 2u)) + 63u) & ~63u" in text
    assert "chunk = chunk < 64u ? 64u : " in text and "(shard + 1 == TICKET_SHARDS) ? n_rays : shard_size * (shard + 1)" in text
    # the counters sit TICKET_PAD words apart, eight to a launch's ticket area
    stride = re.search(r"TICKET_STRIDE = (\d+) \* (\d+),", host)
    assert int(re.search(r"TICKET_PAD\s+= (\d+);", text).group(1)) * J.SHARDS == int(stride.group(1)) * int(stride.group(2))


def test_the_two_debug_calls_are_declared_exported_and_wrapped():
    text = open(os.path.join(ROOT, "include", "fermat_pt_hip.h")).read()
    lib = fa.lib()
    for n in ("fpt_debug_set_trace_blocks", "fpt_debug_trace_tickets"):
        assert re.search(r"\bint\s+%s\s*\(" % n, text) and n in api.ENTRY_POINTS and hasattr(lib, n), n
    assert callable(fa.Renderer.debug_set_trace_blocks) and callable(fa.Renderer.debug_trace_tickets)
    # every launch site sizes its grid from trace_blocks(): nothing multiplies CUs by blocks per CU on its own
    csrc = os.path.join(ROOT, "fermat_amd", "csrc")
    for name in sorted(os.listdir(csrc)) + [os.path.join("host", f) for f in sorted(os.listdir(os.path.join(csrc, "host")))]:
        if name.endswith((".cpp", ".hip", ".h", ".inc")):
            body = open(os.path.join(csrc, name)).read()
            uses = len(re.findall(r"n_cus\s*\*\s*(?:\w+->)?blocks_per_cu|blocks_per_cu\s*\*\s*(?:\w+->)?n_cus", body))
            assert uses == (1 if name == "fpt_host.h" else 0), name


@pytest.mark.parametrize("key", SCENES)
def test_schedule_rays_force_refills(key):
    """what the GPU leg assumes of its rays, on the fp64 truth, and the oracle (= fpt-MT on the quality tree, bit for bit) judged on the whole set with no slip"""
    from oracle import binding as ob
    c = case(key)
    s, rays, away, T = c["scene"], c["rays"], c["away"], c["T"]
    lo, hi, ext = ttt._extent(s)
    assert len(rays) == N_RAYS and all(n <= N_RAYS for n in PREFIXES)
    for g in range(0, N_RAYS, 64):
        grp = slice(g, min(g + 64, N_RAYS))
        assert away[grp].sum() >= min(J.REFILL_MIN, len(away[grp])), g
        if g + 64 <= N_RAYS:
            assert (T["tri"][grp] >= 0).any(), "group %d: no ray with work beyond the root step" % g          # one live lane keeps the wave in its burst
    o, d = rays["origin"].astype(np.float64), rays["dir"].astype(np.float64)
    finite = np.isfinite(o).all(1)
    nan = nan_rays(away)
    assert np.array_equal(np.flatnonzero(~finite), nan) and len(nan) == len(NAN_NEAR) and nan[0] < PREFIXES[0] and not away[nan].any()
    # away rays: outside the ball that holds the box (and the moved mesh's), moving outwards; they hit nothing, nor do the NaN rays
    centre = 0.5 * (lo + hi)
    a = away & finite
    assert (np.linalg.norm(o[a] - centre, axis=1) > 1.4 * ext).all() and (((o[a] - centre) * d[a]).sum(1) > 0).all()
    assert np.linalg.norm(ttt._moved(s).astype(np.float64) - centre, axis=1).max() < 1.2 * ext
    assert (T["tri"][away] < 0).all() and (T["tri"][~finite] < 0).all() and not c["TA"]["occluded"][away].any()
    # (the needles are 1e-4 wide: most rays through their cloud reach the floor or nothing)
    assert 0.1 < (T["tri"] >= 0).mean() < 0.9 and 0.1 < c["TA"]["occluded"].mean() < 0.9 and T["robust"].mean() > 0.9
    table = np.fromfile(os.path.join(scene.DATA_DIR, "glossy_reflectance.dat"), np.float32)
    orc = ob.OraclePT(s, 4, 4, ob.default_options(2), table, scene.DATA_DIR)
    with np.errstate(all="ignore"):
        assert ttt.judge_closest(s, rays, T, orc.trace(rays, n_threads=4), key + "/schedule [oracle]") == 0
        assert ttt.judge_any(s, c["shadow"], c["TA"], orc.trace(c["shadow"], shadow=True, n_threads=4)["t"] > 0, key + "/schedule any [oracle]") == 0


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# (a) plain launches on chosen rays

def _renderer(s, tree, table, intersector):
    """an 8 x 8 context whose tree was built for `intersector` by the named builder; "+refit": the vertices moved as test_trace_truth._moved does, device refit"""
    r = fa.Renderer(s, 8, 8, fa.default_options(2), table=table)
    r.set_intersector(intersector)
    r.set_build_mode({"quality": 0, "fast": 1, "trbvh": 2}[tree.split("+")[0]])
    r.rebuild_geometry()
    if tree.endswith("+refit"):
        r.refit_geometry(ttt._with_vertices(s, ttt._moved(s)).vertex_data)
    assert r.intersector() == (intersector, intersector)
    return r


def _plain_launches(r, rays, shadow, blocks, label):
    """the five plain launches on one prefix, the ticket counters judged after each"""
    n = len(rays)
    out = {}

    def tickets(what):
        try:
            J.check_counters(n, blocks, r.debug_trace_tickets())
        except AssertionError as e:
            raise AssertionError("%s, %s: %s" % (label, what, e))
    out["closest"] = r.trace(rays); tickets("fpt_rt_trace")
    out["any"] = r.trace(shadow, shadow=True); tickets("fpt_rt_trace_shadow")
    out["bits"] = r.trace_shadow_bits(shadow); tickets("fpt_rt_trace_shadow_bits")
    out["closest_counted"], cc = r.trace(rays, counted=True); tickets("fpt_rt_trace_counted, closest")
    out["any_counted"], ca = r.trace(shadow, shadow=True, counted=True); tickets("fpt_rt_trace_counted, shadow")
    out["counters"] = ((int(cc.rays), int(cc.nodes_visited), int(cc.tris_tested)), (int(ca.rays), int(ca.nodes_visited), int(ca.tris_tested)))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("intersector", [fa.INTERSECTOR_MT, fa.INTERSECTOR_WATERTIGHT], ids=["mt", "wt"])
@pytest.mark.parametrize("tree", TREES)
def test_capped_plain_launches_equal_uncapped_and_exhaust_their_tickets(tree, intersector, table):
    """Every prefix under caps 1 and 3 against the same call with no cap, bit for bit; the counted launches' work; the ticket counters against the judge after
    EVERY launch (no case skipped: a capped launch that stayed static where the judge says tickets, or left a shard unexhausted, fails here); on the quality tree
    the capped hits against the fp64 truth with no slip allowed (this set is in no list of test_trace_truth.SLIP_BOUND); fpt-WT against its specification."""
    counts = {}
    for key in SCENES:
        c = case(key, tree.endswith("+refit"))
        s, rays, shadow = c["scene"], c["rays"], c["shadow"]
        r = _renderer(ttt.masked(ttt.get_scene(key)), tree, table, intersector)
        assert r.bvh_info()["max_depth"] >= 2
        base = {}
        for n in PREFIXES:
            # no cap: the grid is ceil(n / 256) blocks (the default grid is larger: cap 20 is accepted in test_the_knob), always static
            base[n] = _plain_launches(r, rays[:n], shadow[:n], (n + 255) // 256, "%s [%s, %d] n = %d, no cap" % (key, tree, intersector, n))
        for cap in CAPS:
            r.debug_set_trace_blocks(cap)
            for n in PREFIXES:
                label = "%s [%s, intersector %d] cap %d, n = %d" % (key, tree, intersector, cap, n)
                got, want = _plain_launches(r, rays[:n], shadow[:n], J.launch_blocks(n, cap), label), base[n]
                assert _same_hits(got["closest"], want["closest"]), "%s: closest hits: %s" % (label, _first_difference(got["closest"], want["closest"]))
                assert _same_hits(got["any"], want["any"]), "%s: occlusion records: %s" % (label, _first_difference(got["any"], want["any"]))
                assert np.array_equal(got["bits"], want["bits"]), "%s: %d bit words differ" % (label, (got["bits"] != want["bits"]).sum())
                assert _same_hits(got["closest_counted"], want["closest"]) and _same_hits(got["any_counted"], want["any"]), label + ": the counted launches' results"
                # per-ray work depends on the ray and the tree alone: a ray handed out twice writes the same hit and shows only here
                assert got["counters"][0][0] == n and got["counters"][1][0] == n, (label, got["counters"])
                assert got["counters"] == want["counters"], "%s: (rays, nodes, triangles) closest / shadow %s, uncapped %s" % (label, got["counters"], want["counters"])
                assert np.array_equal(_unpack(got["bits"], n), got["any"]["t"] > 0), label + ": bits against records"
                if intersector == fa.INTERSECTOR_WATERTIGHT:
                    assert _same_hits(got["closest"], c["W"][:n]), "%s: against the specification: %s" % (label, _first_difference(got["closest"], c["W"][:n]))
                    assert np.array_equal(got["any"]["t"] > 0, c["WA"][:n]), label + ": occlusion against the specification"
                if tree == "quality":
                    with np.errstate(all="ignore"):
                        slips = ttt.judge_closest(s, rays[:n], _prefix(c["T"], n), got["closest"], label)
                        lost = ttt.judge_any(s, shadow[:n], _prefix(c["TA"], n), got["any"]["t"] > 0, label)
                    assert slips <= ttt.SLIP_BOUND.get(key + "/schedule", 0) and lost <= ttt.SLIP_BOUND.get("any/" + key + "/schedule", 0), (label, slips, lost)
            r.debug_set_trace_blocks(0)
        counts[key] = base[N_RAYS]["counters"]
        r.close()
    print("counted [%s, intersector %d], %d rays, (rays, nodes, triangles) closest / shadow: %s" % (tree, intersector, N_RAYS, counts))


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# (b) the queue modes, through the renderers

W, H, PASSES, L = 40, 30, 3, 5
KINDS = ["pt", "pt_in_flight", "pt_in_flight_two_lanes", "psfpt", "psfpt_in_flight", "bpt_sc0", "bpt_sc1", "mmlt"]
MMLT = dict(n_chains=1024, spp=4, mmlt_frequency=2, lens_techniques=1)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint8) if a.dtype.itemsize not in (4, 8) else a.view(np.uint32 if a.dtype.itemsize == 4 else np.uint64)


def _run(kind, s, table, intersector, cap):
    """one renderer of `kind` under `cap` (0 = none): everything the criterion compares, as a dict of arrays"""
    kw = {}
    if kind.startswith("psfpt"):
        kw["psf_options"] = fa.default_psf_options()
    elif kind.startswith("bpt"):
        kw["bpt_options"] = fa.default_bpt_options(L, single_connection=int(kind[-1]))
    elif kind == "mmlt":
        kw["mmlt_options"] = fa.default_mmlt_options(L, **MMLT)
    r = fa.Renderer(s, W, H, fa.default_options(L), table=table, **kw)
    r.set_intersector(intersector); r.rebuild_geometry()
    assert r.intersector() == (intersector, intersector)
    r.debug_set_trace_blocks(cap)
    out = {}
    if kind == "pt":
        r.clear_gbuffer()
        for i in range(PASSES):
            r.render_pass(i)
    elif kind.startswith("pt_in_flight"):
        r.set_batch(PASSES)
        if kind.endswith("two_lanes"):
            r.set_lanes(2)          # each lane has its own counter block, and with it its own ticket areas
            assert r.lane_count() == 2
        r.render_batch(0, PASSES)
    elif kind == "psfpt":
        for i in range(PASSES):
            r.psf_render(i, sync=True)
    elif kind == "psfpt_in_flight":
        r.psf_set_batch(PASSES); r.psf_render_batch(0, PASSES, sync=True)
    elif kind.startswith("bpt"):
        for i in range(PASSES):
            r.bpt_render(i, sync=True)
        lv = r.bpt_light_vertices()
        out["lv_counts"] = lv["counts"]
        n = W * H
        for d in range(L):
            live = lv["counts"] > d          # as test_gpu_bpt_parity reads the store
            for k in ("path_id", "input", "gbuffer", "pos", "weights"):
                out["lv_%s_%d" % (k, d)] = lv[k][d * n:(d + 1) * n][live]
    else:
        r.mmlt_render(0, sync=True)
        for k, v in r.mmlt_state().items():
            out["chain_" + k] = v
        st = r.mmlt_stats()
        out["stats"] = np.array([st["accepted"], st["rejected"], st["swaps_proposed"], st["swaps_accepted"], st["rays"], st["chain_length"]], np.uint64)
        assert st["rays"] > 0 and st["swaps_proposed"] > 0
    if kind.startswith("psfpt"):
        for k, v in r.psf_cells().items():          # as test_psfpt compares them
            out["cells_" + k] = v
        assert len(out["cells_keys"]) > 50
    fb = r.framebuffer()
    for ch in range(8):
        out["channel %d" % ch] = fb[ch]
    if kind == "pt":
        for k in ("gb_geo", "gb_uv", "gb_tri", "gb_depth"):
            out[k] = getattr(r, k).cpu().numpy()
    assert np.isfinite(fb).all() and fb[api.FB_COMPOSITED_C][:, :3].mean() > 1e-3
    r.close()
    return out


def _oracle_run(kind, s, table):
    from oracle import binding as ob
    o = ob.OraclePT(s, W, H, ob.default_options(L), table, scene.DATA_DIR)
    if kind == "psfpt":
        o.psf_enable(ob.default_psf_options())
    else:
        o.clear_gbuffer()
    for i in range(PASSES):
        o.render_pass(i)
    out = {"channel %d" % ch: o.fb[ch] for ch in range(8)}
    if kind == "psfpt":
        for k, v in o.psf_cells().items():
            out["cells_" + k] = v
    else:
        out.update(gb_geo=o.gb_geo, gb_uv=o.gb_uv, gb_tri=o.gb_tri, gb_depth=o.gb_depth)
    return out


def _assert_same(got, want, label, keys=None):
    for k in (keys or sorted(want)):
        a, b = _bits(got[k]).ravel(), _bits(want[k]).ravel()
        assert a.shape == b.shape and np.array_equal(a, b), "%s: %s differs (%s words)" % (label, k, (a != b).sum() if a.shape == b.shape else "another number of")


@pytest.mark.gpu
@pytest.mark.parametrize("intersector", [fa.INTERSECTOR_MT, fa.INTERSECTOR_WATERTIGHT], ids=["mt", "wt"])
@pytest.mark.parametrize("kind", KINDS)
def test_capped_renderers_equal_uncapped(kind, intersector, table, cornell_glossy):
    """40 x 30 = 1200 paths, three passes: the first bounces' queues are above 256 and 768 rays and the later ones below, so one run crosses the static threshold
    under both caps.  Frames, g-buffer, cache cells, light-vertex store and chain state are the criterion: a fused resolve applied twice or a lost shadow ray
    changes a sum or a count.  fpt-MT under cap 1 is also held to the oracle (PT and PSFPT), so that the file stands without the uncapped promise of other modules."""
    want = _run(kind, cornell_glossy, table, intersector, 0)
    for cap in CAPS:
        got = _run(kind, cornell_glossy, table, intersector, cap)
        assert sorted(got) == sorted(want)
        _assert_same(got, want, "%s, intersector %d, cap %d against no cap" % (kind, intersector, cap))
        if cap == 1 and intersector == fa.INTERSECTOR_MT and kind in ("pt", "psfpt"):
            orc = _oracle_run(kind, cornell_glossy, table)
            _assert_same(got, orc, "%s, cap 1 against the oracle" % kind)


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# (c) the knob itself

@pytest.mark.gpu
def test_the_knob(table, cornell_glossy):
    c = case("icosphere")
    rays = c["rays"]
    r = fa.Renderer(ttt.masked(ttt.get_scene("icosphere")), 8, 8, fa.default_options(2), table=table)
    base = r.trace(rays)
    assert not r.debug_trace_tickets().any()
    r.debug_set_trace_blocks(20)          # the default grid is at least the 20 blocks 5000 rays ask for
    r.debug_set_trace_blocks(1)
    # a cap above the default is refused by name and leaves the cap as it was
    with pytest.raises(fa.FptError) as e:
        r.debug_set_trace_blocks(1 << 20)
    assert "fpt_debug_set_trace_blocks" in str(e.value)
    got = r.trace(rays[:257])
    J.check_counters(257, 1, r.debug_trace_tickets())
    assert r.debug_trace_tickets().all() and _same_hits(got, base[:257])
    # 0 restores the default: static again, the same bits
    r.debug_set_trace_blocks(0)
    got = r.trace(rays)
    assert not r.debug_trace_tickets().any() and _same_hits(got, base)
    r.close()
    # setting the cap between two deferred passes renders them first: the frame on the device is the sequential one before anything else flushed
    seq = fa.Renderer(cornell_glossy, W, H, fa.default_options(L), table=table)
    seq.render_pass(0); seq.render_pass(1)
    two = seq.framebuffer().copy()
    seq.render_pass(2); seq.render_pass(3)
    four = seq.framebuffer().copy()
    seq.close()
    d = fa.Renderer(cornell_glossy, W, H, fa.default_options(L), table=table)
    d.set_deferred(4)
    d.render_pass(0); d.render_pass(1)
    d.debug_set_trace_blocks(1)
    d.torch.cuda.synchronize(d.dev)          # waits for the device, asks the library for nothing
    for ch in (0, 1, 2, 3, 4, 5, 7):
        assert np.array_equal(d.fb[ch].cpu().numpy().view(np.uint32), two[ch].view(np.uint32)), "channel %d after the flush" % ch
    d.render_pass(2); d.render_pass(3)
    fb = d.framebuffer()
    for ch in (0, 1, 2, 3, 4, 5, 7):
        assert np.array_equal(fb[ch].view(np.uint32), four[ch].view(np.uint32)), "channel %d, two passes capped" % ch
    d.close()
