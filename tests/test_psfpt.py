"""Path-space-filtering path tracer (`-psfpt`): oracle properties on CPU, HIP-vs-oracle parity on GPU."""
import numpy as np
import pytest

import fermat_amd as fa
from fermat_amd import scene
from oracle import binding as ob


def _oracle(s, table, W, H, L, n, psf=True, **kw):
    o = ob.OraclePT(s, W, H, ob.default_options(L), table, scene.DATA_DIR)
    if psf:
        o.psf_enable(ob.default_psf_options(**kw))
    for i in range(n):
        o.render_pass(i)
    return o


def test_psf_cache_properties(table, cornell):
    W, H, L = 40, 30, 4
    o = _oracle(cornell, table, W, H, L, 8)
    cells = o.psf_cells()
    assert len(cells["keys"]) > 50 and len(np.unique(cells["keys"])) == len(cells["keys"])
    assert (cells["counts"] >= 1).all() and (cells["sums"] >= 0).all()
    # a path opens a cache vertex at most once per bounce (again after a glossy bounce, which keeps the cache id invalid)
    assert 0 < o.psf_ref_count() <= W * H * L
    # key layout: 3 x 17-bit cell coordinates, 5-bit level, 4-bit normal (src/spatial_hash.h:160-166)
    level = (cells["keys"] >> np.uint64(51)) & np.uint64(31)
    assert level.max() <= 17 and (cells["keys"] >> np.uint64(60) == 0).all()
    coords = [(cells["keys"] >> np.uint64(sh)) & np.uint64((1 << 17) - 1) for sh in (0, 17, 34)]
    assert all((c <= (np.uint64(1) << level) + np.uint64(3)).all() for c in coords)      # the jitter disk may step just outside the box
    # the cache is kept across passes and cleared every psf_temporal_reuse passes
    o2 = _oracle(cornell, table, W, H, L, 5, psf_temporal_reuse=4)      # passes 0..3 fill, pass 4 clears and refills
    o1 = _oracle(cornell, table, W, H, L, 4, psf_temporal_reuse=4)
    assert o2.psf_cells()["counts"].sum() < o1.psf_cells()["counts"].sum()
    # clamp_frame(100): no radiance above the clamp; filtering lowers the pixel-to-pixel noise of the indirect term
    pt = _oracle(cornell, table, W, H, L, 8, psf=False)
    assert o.fb[5][:, :3].max() <= 100.0 and np.isfinite(o.fb).all()
    rough = lambda a: float(np.abs(np.diff(a.reshape(H, W, 3), axis=1)).mean())   # noqa: E731
    ind_pt = pt.fb[0][:, :3] + pt.fb[2][:, :3]; ind_psf = o.fb[0][:, :3] + o.fb[2][:, :3]
    assert rough(ind_psf) < 0.9 * rough(ind_pt)
    # direct lighting seen from the eye is not cached (psf_depth = 1): DIRECT_C equals the path tracer's
    assert np.array_equal(o.fb[4].view(np.uint32), pt.fb[4].view(np.uint32))


def test_psf_depth_beyond_path_length_is_the_clamped_path_tracer(table, cornell):
    """with no vertex eligible for caching the PSFPT vertex processor only differs from the PT one by its NEE weights
    (no doubled indirect term) and the firefly clamp: the BSDF-sampling-only estimates coincide"""
    W, H, L = 24, 18, 3
    opt = ob.default_options(L); opt.direct_lighting_nee = 0; opt.indirect_lighting_nee = 0
    a = ob.OraclePT(cornell, W, H, opt, table, scene.DATA_DIR)
    b = ob.OraclePT(cornell, W, H, opt, table, scene.DATA_DIR)
    b.psf_enable(ob.default_psf_options(psf_depth=99, firefly_filter=1e30))
    for i in range(3):
        a.render_pass(i); b.render_pass(i)
    assert b.psf_ref_count() == 0 and len(b.psf_cells()["keys"]) == 0
    assert np.array_equal(a.fb[5][:, :3].view(np.uint32), b.fb[5][:, :3].view(np.uint32))


@pytest.mark.gpu
def test_cli_psfpt_matches_oracle_image(tmp_path, table):
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "fermat_amd", "bin", "fermat_hip")
    d = os.path.join(scene.DATA_DIR, "scenes", "CornellBox")
    out = str(tmp_path / "psf")
    r = subprocess.run([exe, "-i", os.path.join(d, "CornellBox-Glossy.obj"), "-c", os.path.join(d, "camera-frontal.txt"), "-r", "48", "36", "-psfpt",
                        "-pl", "4", "-filter-width", "2.5", "-passes", "2", "-o", out], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    s = scene.cornell_box("CornellBox-Glossy")
    o = ob.OraclePT(s, 48, 36, ob.default_options(4), table, scene.DATA_DIR)
    o.psf_enable(ob.default_psf_options(psf_width=2.5))
    for i in range(3):
        o.render_pass(i)
    got = (scene.load_tga(out + ".tga")[..., :3] * 255.0 + 0.5).astype(np.uint8)
    assert np.array_equal(got, o.to_rgba().reshape(36, 48, 4)[..., :3])
    # -batch: 5 passes as 3 + 2 in flight (the first run above used the default, 3 in flight): the image is the pass-by-pass one, bit for bit;
    # -batch 1 (one pass per call) gives it too
    for i in range(3, 5):
        o.render_pass(i)
    want = o.to_rgba().reshape(36, 48, 4)[..., :3].astype(np.int32)
    r = subprocess.run([exe, "-i", os.path.join(d, "CornellBox-Glossy.obj"), "-c", os.path.join(d, "camera-frontal.txt"), "-r", "48", "36", "-psfpt",
                        "-pl", "4", "-filter-width", "2.5", "-passes", "4", "-batch", "3", "-o", out + "_b"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    got = (scene.load_tga(out + "_b.tga")[..., :3] * 255.0 + 0.5).astype(np.int32)
    assert np.array_equal(got, want)
    r = subprocess.run([exe, "-i", os.path.join(d, "CornellBox-Glossy.obj"), "-c", os.path.join(d, "camera-frontal.txt"), "-r", "48", "36", "-psfpt",
                        "-pl", "4", "-filter-width", "2.5", "-passes", "4", "-batch", "1", "-o", out + "_s"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert np.array_equal((scene.load_tga(out + "_s.tga")[..., :3] * 255.0 + 0.5).astype(np.int32), want)


@pytest.mark.gpu
@pytest.mark.parametrize("scene_name,L,kw", [("CornellBox-JP", 4, {}), ("CornellBox-Glossy", 5, dict(psf_width=2.0, psf_max_prob=8.0)),
                                               ("CornellBox-JP", 4, dict(psf_temporal_reuse=2, firefly_filter=5.0)),
                                               # deep levels: 8..14; 15..21, where the coordinates pass 2^17 and are masked; and the regime beyond level 31
                                               # that tests/psf_truth.py defines (masked shift, level bits over the normal digits)
                                               ("CornellBox-Glossy", 5, dict(psf_width=0.001)), ("CornellBox-Glossy", 5, dict(psf_width=1.0e-5)),
                                               ("CornellBox-Glossy", 5, dict(psf_width=1.0e-9))])
def test_gpu_psfpt_parity(table, scene_name, L, kw):
    s = scene.cornell_box(scene_name)
    W, H = 64, 48
    r = fa.Renderer(s, W, H, fa.default_options(L), table=table, psf_options=fa.default_psf_options(**kw))
    o = ob.OraclePT(s, W, H, ob.default_options(L), table, scene.DATA_DIR)
    o.psf_enable(ob.default_psf_options(**kw))
    for i in range(4):
        r.psf_render(i, sync=True); o.render_pass(i)
        cg, co = r.psf_cells(), o.psf_cells()
        assert np.array_equal(cg["keys"], co["keys"]) and np.array_equal(cg["counts"], co["counts"]) and np.array_equal(cg["sums"], co["sums"]), i
    fb = r.framebuffer()
    for c in range(8):
        assert np.array_equal(fb[c].view(np.uint32), o.fb[c].view(np.uint32)), "channel %d" % c
    r.close()


@pytest.mark.gpu
def test_gpu_psfpt_full_size_is_deterministic(table):
    """1600x900, 8 bounces, 2^24-cell cache on the bathroom stand-in: cache sums are fixed-point integer atomics and cells are addressed
    by key, so two runs give the same cells (as multisets) and the same frame bit for bit; the frame is finite and clamped to 100."""
    W, H, L = 1600, 900, 9
    s = scene.bathroom_standin(0.25)
    frames, cells = [], []
    for _ in range(2):
        r = fa.Renderer(s, W, H, fa.default_options(L), table=table, gbuffer=False, psf_options=fa.default_psf_options())
        for i in range(2):
            r.psf_render(i, sync=True)
        frames.append(r.framebuffer()[5].copy())
        c = r.psf_cells()
        order = np.argsort(c["keys"], kind="stable")
        cells.append((c["keys"][order], c["counts"][order], c["sums"][order]))
        r.close()
    assert np.array_equal(frames[0].view(np.uint32), frames[1].view(np.uint32))
    for a, b in zip(cells[0], cells[1]):
        assert np.array_equal(a, b)
    assert np.isfinite(frames[0]).all() and frames[0][:, :3].min() >= 0 and frames[0][:, :3].max() <= 100.0 and len(cells[0][0]) > 1000


@pytest.mark.gpu
@pytest.mark.parametrize("scene_name,W,H,L,n_ranks", [("CornellBox-Glossy", 64, 48, 5, 2), ("CornellBox-JP", 96, 64, 6, 3)])
def test_gpu_psfpt_tile_sharded_equals_full_frame(table, scene_name, W, H, L, n_ranks):
    """PSFPT under tile sharding (fpt_psfpt_set_sharded): n rank contexts on ONE GPU, each rendering its scanlines; after every pass the
    ranks' cell records are merged by key into every rank's global table (export / import, the hand-driven twin of the RCCL exchange) and
    fpt_psfpt_finish blends.  The tables of all ranks equal the full-frame renderer's cell for cell, and the assembled frame equals the
    full-frame one bit for bit on every channel -- the cache sums are integers, so the sharding changes nothing."""
    import torch
    from fermat_amd.distributed import device_bytes, PSF_RECORD_BYTES
    s = scene.cornell_box(scene_name)
    psf = dict(psf_temporal_reuse=3)                      # the reset of the cache happens inside the test's 5 passes
    full = fa.Renderer(s, W, H, fa.default_options(L), table=table, psf_options=fa.default_psf_options(**psf))
    lists = fa.tile_pixel_lists(W, H, n_ranks, tile=(W, 1))
    ranks = [fa.Renderer(s, W, H, fa.default_options(L), table=table, pixels=lists[k], psf_options=fa.default_psf_options(**psf)) for k in range(n_ranks)]
    for r in ranks:
        r.psf_set_sharded(True)
    total_records = 0
    for i in range(5):
        full.psf_render(i, sync=True)
        for r in ranks:
            r.psf_render(i)
        exported = []
        for r in ranks:
            ptr, n = r.psf_export_cells()
            exported.append(device_bytes(ptr, n * PSF_RECORD_BYTES, r.dev).clone() if n else None)      # what a host would put on the wire
            total_records += n
        for r in ranks:
            for t in exported:
                if t is not None:
                    r.psf_import_cells(t.data_ptr(), t.numel() // PSF_RECORD_BYTES)
            r.psf_finish(sync=True)
        want = full.psf_cells()
        for r in ranks:
            got = r.psf_cells()
            assert np.array_equal(got["keys"], want["keys"]) and np.array_equal(got["counts"], want["counts"]) and np.array_equal(got["sums"], want["sums"]), i
    assert total_records > 0
    ref = full.framebuffer()
    for k, r in enumerate(ranks):
        fb = r.framebuffer()
        px = lists[k]
        for c in range(8):
            assert np.array_equal(fb[c][px].view(np.uint32), ref[c][px].view(np.uint32)), "rank %d channel %d" % (k, c)
    # errors: a second render before the pending pass is finished is refused
    ranks[0].psf_render(5)
    with pytest.raises(fa.FptError):
        ranks[0].psf_render(6)
    for r in ranks + [full]:
        r.close()


@pytest.mark.gpu
@pytest.mark.parametrize("scene_name,W,H,L,groups,reuse", [("CornellBox-Glossy", 64, 48, 5, (3, 3), 64), ("CornellBox-JP", 96, 64, 6, (4, 2, 1), 3)])
def test_gpu_psfpt_passes_in_flight(table, scene_name, W, H, L, groups, reuse):
    """fpt_psfpt_render_batch: passes in flight, each into its own pass table, folded into the cache in pass order (a reset of the reuse
    window may fall inside a batch).  After every batch the cache equals the sequential renderer's (= the oracle's) cell for cell, bit for
    bit; and since round 3 so does the FRAME, every channel, .w included: a path's frame contributions -- emission, the frame share of its light samples,
    the blends of its cache references -- are kept in the cells of a contribution log and applied by the merge in the sequential order."""
    s = scene.cornell_box(scene_name)
    seq = fa.Renderer(s, W, H, fa.default_options(L), table=table, psf_options=fa.default_psf_options(psf_temporal_reuse=reuse))
    bat = fa.Renderer(s, W, H, fa.default_options(L), table=table, psf_options=fa.default_psf_options(psf_temporal_reuse=reuse))
    bat.psf_set_batch(max(groups))
    first = 0
    for g in groups:
        for i in range(first, first + g):
            seq.psf_render(i, sync=True)
        if g > 1:
            bat.psf_render_batch(first, g, sync=True)
        else:
            bat.psf_render(first, sync=True)
        first += g
        a, b = seq.psf_cells(), bat.psf_cells()
        assert np.array_equal(a["keys"], b["keys"]) and np.array_equal(a["counts"], b["counts"]) and np.array_equal(a["sums"], b["sums"]), first
    want, got = seq.framebuffer(), bat.framebuffer()
    assert np.isfinite(got).all()
    for c in (5, 0, 1, 2, 3, 4, 7):
        d = got[c][:, :3].astype(np.float64) - want[c][:, :3].astype(np.float64)
        assert np.array_equal(got[c].view(np.uint32), want[c].view(np.uint32)), (c, float(np.sqrt((d * d).sum(1).mean())))
    assert want[5][:, :3].mean() > 1e-3
    seq.close(); bat.close()


# ---- the cache under load: a table a test sized (fpt_psfpt_debug_set_table_log2) -------------------------------------------------------------------------------
CROWD = dict(psf_width=0.001)          # CornellBox-Glossy, 64x48, L = 5, 3 passes: 3905 cells at levels 8..14


def _same_cells(got, want, what):
    assert np.array_equal(got["keys"], want["keys"]) and np.array_equal(got["counts"], want["counts"]) and np.array_equal(got["sums"], want["sums"]), what


@pytest.fixture(scope="module")
def crowd_oracle(table):
    s = scene.cornell_box("CornellBox-Glossy")
    return s, _oracle(s, table, 64, 48, 5, 3, **CROWD)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["sequential", "in_flight", "sharded"])
def test_gpu_psfpt_crowded_table(table, crowd_oracle, mode):
    """The cache in a table just large enough: the power of two above the oracle's cell count (3905 cells in 2^12 slots: load 0.95, probe chains of hundreds of
    slots that wrap past the end).  Cells are addressed by key, so cache and frame must still equal the oracle's -- which has no table -- bit for bit: pass by pass,
    as passes in flight (2 + 1; the pass tables and the fold into the global table probe the same way) and tile-sharded over two rank contexts (pass table,
    records, merge, look-up by key in the blend)."""
    s, o = crowd_oracle
    W, H, L = 64, 48, 5
    want = o.psf_cells()
    log2 = max(8, int(len(want["keys"])).bit_length())
    assert len(want["keys"]) > 0.45 * (1 << log2)
    mk = lambda **kw: fa.Renderer(s, W, H, fa.default_options(L), table=table, psf_options=fa.default_psf_options(**CROWD), **kw)  # noqa: E731
    if mode == "sharded":
        from fermat_amd.distributed import device_bytes, PSF_RECORD_BYTES
        lists = fa.tile_pixel_lists(W, H, 2, tile=(W, 1))
        ranks = [mk(pixels=lists[k]) for k in range(2)]
        for r in ranks:
            r.psf_debug_set_table_log2(log2); r.psf_set_sharded(True)
        for i in range(3):
            for r in ranks:
                r.psf_render(i)
            exported = []
            for r in ranks:
                ptr, n = r.psf_export_cells()
                exported.append(device_bytes(ptr, n * PSF_RECORD_BYTES, r.dev).clone() if n else None)
            for r in ranks:
                for t in exported:
                    if t is not None:
                        r.psf_import_cells(t.data_ptr(), t.numel() // PSF_RECORD_BYTES)
                r.psf_finish(sync=True)
        for k, r in enumerate(ranks):
            _same_cells(r.psf_cells(), want, "rank %d" % k)
            fb = r.framebuffer()
            for c in range(8):
                assert np.array_equal(fb[c][lists[k]].view(np.uint32), o.fb[c][lists[k]].view(np.uint32)), "rank %d channel %d" % (k, c)
            r.close()
        return
    r = mk()
    r.psf_debug_set_table_log2(log2)
    if mode == "in_flight":
        r.psf_set_batch(2)
        r.psf_render_batch(0, 2, sync=True); r.psf_render(2, sync=True)
    else:
        for i in range(3):
            r.psf_render(i, sync=True)
    _same_cells(r.psf_cells(), want, mode)
    fb = r.framebuffer()
    for c in range(8):
        assert np.array_equal(fb[c].view(np.uint32), o.fb[c].view(np.uint32)), "channel %d" % c
    # the setter is refused once the context has rendered, and outside 8..24
    with pytest.raises(fa.FptError):
        r.psf_debug_set_table_log2(log2)
    r.close()


def test_psf_energy_brackets_oracle(table):
    """The two estimators a vertex of a FULL table falls between, on the oracle: path-space filtering with every vertex cached (an unbounded table) and with none
    (psf_depth beyond the path length).  Mean of COMPOSITED_C over the pixels below 20 (the light source is left out), CornellBox-Glossy 64x48, L = 5, width
    0.001, 3 passes: 0.4440 cached, 0.4552 uncached; the mean of ONE pass moves by 0.0152 (standard deviation over the passes 0..7, each rendered alone).
    test_gpu_psfpt_full_table allows three times that, PSF_ENERGY_MARGIN, beyond the bracket."""
    s = scene.cornell_box("CornellBox-Glossy")
    a, b, mask = _energy_brackets(s, table)
    assert 0.3 < min(a, b) and max(a, b) < 0.6 and abs(a - b) < PSF_ENERGY_MARGIN and mask.mean() > 0.9
    one = []
    for i in range(8):
        o = ob.OraclePT(s, 64, 48, ob.default_options(5), table, scene.DATA_DIR)
        o.psf_enable(ob.default_psf_options(**CROWD))
        o.render_pass(i)
        one.append(float(o.fb[5][:, :3][mask].mean()) * (i + 1))              # a first pass rendered as instance i carries the frame weight 1 / (i + 1)
    sd = float(np.std(one, ddof=1))
    print("brackets %.5f %.5f, pass-to-pass sd %.5f" % (a, b, sd))
    assert 3.0 * sd <= 1.25 * PSF_ENERGY_MARGIN and PSF_ENERGY_MARGIN <= 1.25 * 3.0 * sd          # the constant is this measurement


PSF_ENERGY_MARGIN = 0.0455


def _energy_brackets(s, table):
    a = _oracle(s, table, 64, 48, 5, 3, **CROWD)
    b = _oracle(s, table, 64, 48, 5, 3, psf_depth=99, **CROWD)
    mask = (a.fb[5][:, :3] < 20.0).all(axis=1) & (b.fb[5][:, :3] < 20.0).all(axis=1)
    return float(a.fb[5][:, :3][mask].mean()), float(b.fb[5][:, :3][mask].mean()), mask


@pytest.mark.gpu
def test_gpu_psfpt_full_table(table, crowd_oracle):
    """The same run in a table of 2^10 slots, a quarter of what it needs: the table fills up in the first pass and every later key is refused -- its vertex stays
    uncached.  WHICH vertices those are is a race, so only what must hold is asserted: the run completes, the table holds exactly 1024 distinct keys, the frame
    is finite and clamped, DIRECT_C (which never touches the cache) equals the unbounded cache's bit for bit -- and the plain path tracer's on every pixel that
    does not show the emitter, whose emission this renderer clamps --, the energy of the frame lies between the
    all-cached and the none-cached estimate of the oracle (test_psf_energy_brackets_oracle: margin 3 x 0.0152 = 0.0455, the pass-to-pass deviation of that mean), and a
    second renderer of the same process still matches the oracle exactly at full size."""
    s, o = crowd_oracle
    W, H, L = 64, 48, 5
    r = fa.Renderer(s, W, H, fa.default_options(L), table=table, psf_options=fa.default_psf_options(**CROWD))
    with pytest.raises(fa.FptError):
        r.psf_debug_set_table_log2(7)
    r.psf_debug_set_table_log2(10)
    pt = fa.Renderer(s, W, H, fa.default_options(L), table=table)
    for i in range(3):
        r.psf_render(i, sync=True); pt.render_pass(i)
    cells = r.psf_cells()
    assert len(cells["keys"]) == 1024 and len(np.unique(cells["keys"])) == 1024 and (cells["counts"] >= 1).all()
    assert np.isin(cells["keys"], o.psf_cells()["keys"]).all()                       # every key is one the unbounded cache holds too
    fb = r.framebuffer()
    assert np.isfinite(fb).all()
    for c in (0, 2, 4, 5):
        assert fb[c][:, :3].max() <= 100.0, c
    # DIRECT_C holds the emission seen at bounce 0 and nothing of the cache: the unbounded cache's frame has the same one, all four components, on every pixel;
    # and so has the plain path tracer wherever it saw no light source (the emitter's 200 is above firefly_filter = 100, which this vertex processor clamps
    # emission to before clamp_frame cuts the frame at 100: on the emitter's pixels the two renderers differ with ANY table, the oracle's included)
    want_dc, pt_dc = o.fb[4], pt.framebuffer()[4]
    assert np.array_equal(fb[4].view(np.uint32), want_dc.view(np.uint32))
    lit = (pt_dc != 0.0).any(axis=1)
    assert 0 < lit.sum() < 0.1 * W * H and (pt_dc[lit][:, :3].max(axis=1) > 0.0).all()
    assert np.array_equal(fb[4][~lit].view(np.uint32), pt_dc[~lit].view(np.uint32))
    a, b, mask = _energy_brackets(s, table)
    got = float(fb[5][:, :3][mask].mean())
    print("energy: %.5f between %.5f and %.5f" % (got, a, b))
    assert min(a, b) - PSF_ENERGY_MARGIN <= got <= max(a, b) + PSF_ENERGY_MARGIN, (got, a, b)
    r.close(); pt.close()
    r2 = fa.Renderer(s, W, H, fa.default_options(L), table=table, psf_options=fa.default_psf_options(**CROWD))
    for i in range(3):
        r2.psf_render(i, sync=True)
    _same_cells(r2.psf_cells(), o.psf_cells(), "full size, afterwards")
    fb = r2.framebuffer()
    for c in range(8):
        assert np.array_equal(fb[c].view(np.uint32), o.fb[c].view(np.uint32)), "channel %d" % c
    r2.close()
