"""A whole path-space-filtering pass replayed from its judged pieces: tests/psfpt_truth.py strings the probes together the way the reference's text says and must
reproduce, with no tolerance anywhere, the cache cells (key, count, three integer sums), the reference queue of every bounce (as a set keyed by pixel, the cache
word through the KEY of the slot it names) and all eight channels of the frame as uint32 bits.  Every key a probe returns for a vertex of a replayed pass must lie
in psf_truth's admissible set for that vertex.

The CPU leg runs the replay on the ORACLE's probes against the oracle's PSFPT; it is where the replay was developed, and it shows that each deliberate mistake of
psfpt_truth.WRONG is refused by a named case (REFUSED_BY).  The `gpu` leg runs the same cases on the DEVICE probes against the device, rendered through psf_render
in the production configuration (no profiling, no capture), and holds the device's cells, references and frame to the oracle's as well; `batch` and `sharded`
exist only there."""
import os
import re

import numpy as np
import pytest

from fermat_amd import scene
import psf_truth as PSF
import psfpt_truth as T
import test_path_truth as TP

# ---- the cases ----------------------------------------------------------------------------------------------------------------------------------------------
# name -> (scene, res_x, res_y, path-tracer options, PSF options, instances, family).  path_truth's shapes, the smallest at which the glue can still go wrong
# (tests/test_path_truth.py says why each).  The counts behind the non-vacuity conditions are written next to FAMILY_NEEDS.
VARIANTS = dict(no_nee=dict(direct_lighting_nee=0, indirect_lighting_nee=0), no_bsdf=dict(direct_lighting_bsdf=0, indirect_lighting_bsdf=0),
                L2=dict(max_path_length=2), L1=dict(max_path_length=1))
CASES = {
    "jp_vpl":     ("jp", 23, 17, dict(max_path_length=4, nee_type=1), {}, (0,), "cornell"),
    "jp_mesh":    ("jp", 23, 17, dict(max_path_length=4, nee_type=0), {}, (0,), "cornell"),
    "reuse":      ("jp", 23, 17, dict(max_path_length=4), dict(psf_temporal_reuse=4), (0, 1, 2, 3, 4), "cornell"),
    "glossy":     ("glossy", 29, 21, dict(max_path_length=5), {}, (0,), "glossy"),
    # firefly_filter 0.25: the light's emission (17, 12, 4) times any path weight above 1 / 68 is clamped; NEE terms and cell means of the box lie around 0.1 .. 1
    "firefly":    ("glossy", 29, 21, dict(max_path_length=5), dict(firefly_filter=0.25), (0,), "glossy"),
    # psf_max_prob 0.3: below the pdf of most scatterings (a cosine lobe's pdf is cos / pi <= 0.318), so vertices are refused and cells open late
    "maxprob":    ("glossy", 29, 21, dict(max_path_length=5), dict(psf_max_prob=0.3), (0,), "glossy"),
    "standin":    ("standin", 31, 19, dict(max_path_length=5), {}, (0,), "standin"),
    "depth0":     ("jp", 16, 12, dict(max_path_length=4), dict(psf_depth=0), (0,), "options"),
    "depth2":     ("jp", 16, 12, dict(max_path_length=4), dict(psf_depth=2), (0,), "options"),
    "depth99":    ("jp", 16, 12, dict(max_path_length=4), dict(psf_depth=99), (0,), "options"),
    "width_half": ("jp", 16, 12, dict(max_path_length=4), dict(psf_width=0.5), (0,), "options"),
    "width_8":    ("jp", 16, 12, dict(max_path_length=4), dict(psf_width=8.0), (0,), "options"),
    "one":        ("jp", 1, 1, dict(max_path_length=3), {}, (0,), "one"),
    "tile_x":     ("jp", 300, 3, dict(max_path_length=2), {}, (0,), "tiles"),
    "tile_y":     ("jp", 6, 300, dict(max_path_length=2), {}, (0,), "tiles"),
}
for _k, _v in VARIANTS.items():
    CASES[_k] = ("jp", 16, 12, dict(dict(max_path_length=4), **_v), {}, (0,), "options")

# which case refuses which deliberate mistake (found on the CPU leg; test_mistakes_refused asserts every line)
REFUSED_BY = {
    "shadow_out_vertex_info": "jp_vpl", "filter_scale_2": "jp_vpl", "jitter_no_instance": "reuse", "normal_not_flipped": "standin", "count_on_creation": "jp_vpl",
    "scatter_demod_cached": "glossy", "glossy_opens_all": "glossy", "emission_to_frame": "jp_vpl", "emission_unclamped": "firefly", "reset_at_1": "reuse",
    "blend_after_clamp": "glossy", "max_prob_dropped": "maxprob", "nee_cell_clamped": "firefly", "ref_unmodulated": "jp_vpl",
}


def psf_options_dict(o):
    return {k: getattr(o, k) for k in T.PSF_OPTION_NAMES}


class PsfProviderMixin:
    def psf(self, op, data, size=0, firefly=100.0):
        """0: the keys of (n, 32) records; 2: the cells (size, 4) int64 of (n, 4) records after psf_clamp + psf_add"""
        out = self.psf_probe(op, data, size, firefly)
        return out["cells"] if op == 2 else out


class OracleProvider(PsfProviderMixin, TP.OracleProvider):
    def psf_probe(self, op, data, size, firefly):
        from oracle import binding as ob
        return ob.psf_probe(op, data, size, firefly)


class DeviceProvider(PsfProviderMixin, TP.DeviceProvider):
    def psf_probe(self, op, data, size, firefly):
        return self.r.debug_psf(op, data, size, firefly)


# ---- what the renderer under test made, and the comparisons ---------------------------------------------------------------------------------------------------
def refs_by_pixel(refs):
    """a renderer's psf_refs() -> per bounce {pixel: (pixel_info, key, w_d bits, w_g bits)}; the cache word of a reference is (slot, ALL_COMPS, not new)"""
    out = []
    for d in refs:
        assert d["n"] == len(d["ref_pixels"]) and ((d["ref_cache"] >> np.uint32(29)) == 3).all(), "a reference's cache word is not (slot, ALL_COMPS, 0)"
        pix = d["ref_pixels"] & np.uint32(0x7FFFFFF)
        assert len(np.unique(pix)) == len(pix), "a path owns two references of one bounce"
        out.append({int(p): (int(d["ref_pixels"][i]), int(d["keys"][i]), tuple(d["ref_wd"][i].view(np.uint32)), tuple(d["ref_wg"][i].view(np.uint32))) for i, p in enumerate(pix)})
    return out


def replay_refs(rep, n_bounces):
    return [{pi & 0x7FFFFFF: (pi, key, tuple(w_d.view(np.uint32)), tuple(w_g.view(np.uint32))) for pi, key, w_d, w_g in rep["refs"].get(b, [])} for b in range(n_bounces)]


def compare_cells(mine, theirs, what):
    diff = []
    if not np.array_equal(mine["keys"], theirs["keys"]):
        a, b = set(mine["keys"].tolist()), set(theirs["keys"].tolist())
        return ["%s: %d keys only in the replay, %d only in the renderer (of %d / %d)" % (what, len(a - b), len(b - a), len(a), len(b))]
    for f in ("counts", "sums"):
        if not np.array_equal(mine[f], theirs[f]):
            bad = np.nonzero((mine[f] != theirs[f]).reshape(len(mine[f]), -1).any(1))[0]
            diff.append("%s: %s differ at %d cells, first key %#x: %s vs %s" % (what, f, len(bad), int(mine["keys"][bad[0]]), mine[f][bad[0]], theirs[f][bad[0]]))
    return diff


def compare_refs(mine, theirs, what):
    diff = []
    for b, (m, t) in enumerate(zip(mine, theirs)):
        if m != t:
            bad = sorted(p for p in set(m) | set(t) if m.get(p) != t.get(p))
            diff.append("%s: the references of bounce %d differ at %d pixels (of %d / %d), first %d: %s vs %s" % (what, b, len(bad), len(m), len(t), bad[0], m.get(bad[0]), t.get(bad[0])))
    return diff


def replay_case(t, prov, wrong=None, cache=None):
    """the replay of a case's passes on a zero frame and (unless one is handed in) an empty cache: per instance the replay, its cells and references; the frame"""
    rx, ry = t["res"]
    frame = np.zeros((8, rx * ry, 4), np.float32)
    cache = T.Cache() if cache is None else cache
    out = {}
    for inst in t["instances"]:
        rep = T.replay_pass(prov, t["scn"], rx, ry, t["options"], t["psf_options"], inst, t["shifts"], cache, t.get("pixels"), wrong)
        T.apply_pass(frame, rep, inst, wrong)
        out[inst] = dict(rep=rep, cells=cache.as_arrays(), refs=replay_refs(rep, t["options"]["max_path_length"]))
    return out, frame


def differences(t, mine, frame):
    diff = []
    for inst in t["instances"]:
        diff += compare_cells(mine[inst]["cells"], t["cells"][inst], "instance %d cells" % inst)
        diff += compare_refs(mine[inst]["refs"], t["refs"][inst], "instance %d" % inst)
    return diff + TP.compare_frames(frame, t["frame"], t.get("pixels"))


def check_keys_admissible(mine):
    """every key a probe returned for a vertex of the replayed passes lies in psf_truth's admissible set for that vertex; no vertex is excepted"""
    n = wide = 0
    for r in mine.values():
        for rec, keys in r["rep"]["key_log"]:
            ok, w = PSF.check_keys(rec, keys)
            assert ok.all(), "a key outside its admissible set: record %s, key %#x" % (rec[np.nonzero(~ok)[0][0]], int(keys[np.nonzero(~ok)[0][0]]))
            n += len(keys); wide += int(w.sum())
    return n, wide


_ORACLE = {}


def oracle_truth(name, olib, table):
    if name in _ORACLE:
        return _ORACLE[name]
    from oracle import binding as ob
    key, rx, ry, kw, pkw, instances, _ = CASES[name]
    scn = TP.scene_of(key)
    opts = TP.make_options(ob, kw)
    popts = ob.default_psf_options(**pkw)
    o = ob.OraclePT(scn, rx, ry, opts, table, scene.DATA_DIR)
    o.psf_enable(popts)
    cells, refs = {}, {}
    for inst in instances:
        o.render_pass(inst)
        cells[inst] = o.psf_cells(); refs[inst] = refs_by_pixel(o.psf_refs())
    shifts, _ = o.sequence(instances[0])
    t = dict(scn=scn, res=(rx, ry), options=TP.options_dict(opts), psf_options=psf_options_dict(popts), instances=instances, cells=cells, refs=refs, frame=o.fb.copy(),
             shifts=shifts, provider=OracleProvider(olib, o, table), keep=o)
    _ORACLE[name] = t
    return t


def log_case(name, mine):
    for inst, r in mine.items():
        print("%s instance %d: queue sizes %s; %s; %d cells" % (name, inst, r["rep"]["stats"], r["rep"]["psf_counts"], len(r["cells"]["keys"])))


# ---- non-vacuity ------------------------------------------------------------------------------------------------------------------------------------------------
# What a family must contain over its cases, so that no rule is judged on nothing; the tests print the totals, and those seen (the same on the oracle's probes and
# on the device's) stand next to each family.  EVERY: a cell opened at bounce 1, a cell shared by at least two paths, an emission that reaches a cell and one that
# reaches the frame, a light sample that reaches a cell and one that reaches the frame, a scattering weight that is demodulated.  AFTER_GLOSSY: a cell opened after a
# glossy bounce, a reference with a non-zero glossy weight, an invalid id retained by a vertex that had itself opened a cell.  The glossy family adds what its two
# option cases are there for: a vertex refused by psf_max_prob, and a term that firefly_filter actually clamps in each of an emission, a frame NEE term and a blend.
# The options family adds the cell opened at bounce 0 (psf_depth 0).  `tiles` stops at L = 2: bounce 1 opens the cells and counts the paths that share them, but
# neither a light sample (3 > L) nor a later vertex follows, so nothing is ever added to them; its keys, counts, references and frame are what it is there for.
# `one` is ONE path, which leaves the box at bounce 1 before a cell can open: it claims its frame alone.
EVERY = ("opened_b1", "shared", "emission_to_cell", "emission_to_frame", "nee_to_cell", "nee_to_frame", "scatter_demodulated")
AFTER_GLOSSY = ("opened_after_glossy", "glossy_ref", "id_retained")
FAMILY_NEEDS = {
    # opened_b1 1507, shared 1430, emission_to_cell 10, emission_to_frame 41, nee_to_cell 1400, nee_to_frame 2048, scatter_demodulated 975, opened_after_glossy 585, id_retained 262
    "cornell": EVERY + AFTER_GLOSSY,
    # opened_b1 739, shared 642, emission_to_cell 3, emission_to_frame 15, nee_to_cell 738, nee_to_frame 1182, scatter_demodulated 317, opened_after_glossy 263,
    # id_retained 95, max_prob_refused 104, emission_clamped 9, nee_frame_clamped 195, blend_clamped 128
    "glossy":  EVERY + AFTER_GLOSSY + ("max_prob_refused", "emission_clamped", "nee_frame_clamped", "blend_clamped"),
    # opened_b1 290, shared 251, emission_to_cell 3, emission_to_frame 3, nee_to_cell 302, nee_to_frame 481, scatter_demodulated 179, opened_after_glossy 106, id_retained 53
    "standin": EVERY + AFTER_GLOSSY,
    # opened_b0 192, opened_b1 582, shared 493, emission_to_cell 6, emission_to_frame 41, nee_to_cell 559, nee_to_frame 992, scatter_demodulated 447, opened_after_glossy 249
    "options": EVERY + AFTER_GLOSSY + ("opened_b0",),
    # opened_b1 506 (481 + 25), shared 399, emission_to_frame 8, nee_to_frame 842, opened_after_glossy 106
    "tiles":   ("opened_b1", "shared", "emission_to_frame", "nee_to_frame", "opened_after_glossy", "glossy_ref"),
    "one":     ("nee_to_frame",),
}
FAMILIES = sorted(FAMILY_NEEDS)


def cases_of(family):
    return [k for k, v in CASES.items() if v[6] == family]


def check_family(family, replays):
    total = {}
    for mine in replays.values():
        for r in mine.values():
            for k, v in r["rep"]["psf_counts"].items():
                total[k] = total.get(k, 0) + v
    for k in FAMILY_NEEDS[family]:
        assert total[k] >= 1, (family, k, total)
    return total


# =============================================================================================================================================================
# CPU leg
# =============================================================================================================================================================
def test_entry_point_declared_exported_wrapped():
    import fermat_amd as fa
    from fermat_amd import api
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "fermat_pt_hip.h")).read()
    n = "fpt_psfpt_debug_download_refs"
    assert re.search(r"\bint\s+%s\s*\(" % n, text) and n in api.ENTRY_POINTS and hasattr(fa.Renderer, "psf_refs")


@pytest.mark.parametrize("family", FAMILIES)
def test_replay_equals_oracle(olib, table, family):
    replays = {}
    for name in cases_of(family):
        t = oracle_truth(name, olib, table)
        mine, frame = replay_case(t, t["provider"])
        log_case(name, mine)
        diff = differences(t, mine, frame)
        assert not diff, (name, diff[:6])
        print(name, "keys judged / with a wide set:", check_keys_admissible(mine))
        replays[name] = mine
    print(family, check_family(family, replays))


@pytest.mark.parametrize("wrong", T.WRONG)
def test_mistakes_refused(olib, table, wrong):
    name = REFUSED_BY[wrong]
    t = oracle_truth(name, olib, table)
    mine, frame = replay_case(t, t["provider"], wrong)
    diff = differences(t, mine, frame)
    print(wrong, "refused by", name, ":", diff[:2])
    assert diff, "%s is not told from the truth by %s" % (wrong, name)


def test_every_mistake_has_its_case():
    assert set(REFUSED_BY) == set(T.WRONG) and all(v in CASES for v in REFUSED_BY.values())


@pytest.mark.parametrize("wrong,name", [("glossy_ref_bounce0", "depth0"), ("mode2_below_depth", "depth2"), ("blend_from_0", "depth2")])
def test_implied_rules_decide_nothing(olib, table, wrong, name):
    """the three tests of the reference's text that another rule implies (psfpt_truth's docstring): leaving one out gives the same pass, where it could matter most"""
    t = oracle_truth(name, olib, table)
    mine, frame = replay_case(t, t["provider"], wrong)
    assert not differences(t, mine, frame)
    if wrong == "glossy_ref_bounce0":
        assert mine[0]["rep"]["psf_counts"]["opened_b0"] > 0 and all((pi >> 27) & 0xF == 0 for pi, _, _, _ in mine[0]["rep"]["refs"][0])


# =============================================================================================================================================================
# GPU leg
# =============================================================================================================================================================
_DEVICE = {}


def run_device_case(name, table, olib):
    if name in _DEVICE:
        if isinstance(_DEVICE[name], BaseException):
            raise _DEVICE[name]          # what went wrong on the device once is not started there a second time in one session
        return _DEVICE[name]
    try:
        _DEVICE[name] = device_case(name, table, olib)
    except BaseException as e:
        _DEVICE[name] = e
        raise
    return _DEVICE[name]


def device_case(name, table, olib):
    import fermat_amd as fa
    key, rx, ry, kw, pkw, instances, _ = CASES[name]
    scn = TP.scene_of(key)
    opts = TP.make_options(fa, kw)
    popts = fa.default_psf_options(**pkw)
    r = fa.Renderer(scn, rx, ry, opts, table=table, psf_options=popts)
    try:
        cells, refs = {}, {}
        for inst in instances:
            r.psf_render(inst, sync=True)
            cells[inst] = r.psf_cells(); refs[inst] = refs_by_pixel(r.psf_refs())
        frame = r.framebuffer().copy()
        shifts, _ = r.sequence(instances[0])
        t = dict(scn=scn, res=(rx, ry), options=TP.options_dict(opts), psf_options=psf_options_dict(popts), instances=instances, cells=cells, refs=refs, frame=frame,
                 shifts=shifts)
        mine, mframe = replay_case(t, DeviceProvider(r, table))
        log_case(name, mine)
        diff = differences(t, mine, mframe)
        assert not diff, (name, diff[:6])
        print(name, "keys judged / with a wide set:", check_keys_admissible(mine))
        # ... and the oracle's pass is the device's
        o = oracle_truth(name, olib, table)
        diff = []
        for inst in instances:
            diff += compare_cells(cells[inst], o["cells"][inst], "device vs oracle, instance %d cells" % inst) + compare_refs(refs[inst], o["refs"][inst], "device vs oracle, instance %d" % inst)
        diff += TP.compare_frames(frame, o["frame"])
        assert not diff, (name, diff[:6])
    finally:
        r.close()
    return mine


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_replay_equals_device(table, olib, name):
    run_device_case(name, table, olib)


@pytest.mark.gpu
@pytest.mark.parametrize("family", FAMILIES)
def test_device_cases_not_vacuous(table, olib, family):
    print(family, check_family(family, {name: run_device_case(name, table, olib) for name in cases_of(family)}))


JP = ("jp", 23, 17, dict(max_path_length=4))


def sequential_replay(r, table, instances, popts, opts, pixels=None):
    key, rx, ry, _ = JP
    shifts, _ = r.sequence(instances[0])
    t = dict(scn=TP.scene_of(key), res=(rx, ry), options=TP.options_dict(opts), psf_options=psf_options_dict(popts), instances=instances, shifts=shifts, pixels=pixels)
    return replay_case(t, DeviceProvider(r, table))


@pytest.mark.gpu
def test_batch_equals_three_replayed_passes(table, olib):
    """three passes in flight through psf_render_batch against three sequential replayed passes: the cells exact, the frame bit for bit (prefix, batch blend, merge,
    clear).  The references of a batch name slots of its pass tables, which are cleared when it ends: they are judged in the sequential and the sharded runs."""
    import fermat_amd as fa
    from oracle import binding as ob
    key, rx, ry, kw = JP
    instances = (0, 1, 2)
    opts, popts = TP.make_options(fa, kw), fa.default_psf_options()
    r = fa.Renderer(TP.scene_of(key), rx, ry, opts, table=table, psf_options=popts)
    try:
        r.psf_set_batch(3)
        r.psf_render_batch(0, 3, sync=True)
        cells, frame = r.psf_cells(), r.framebuffer().copy()
        mine, mframe = sequential_replay(r, table, instances, popts, opts)
        diff = compare_cells(mine[2]["cells"], cells, "cells after the batch") + TP.compare_frames(mframe, frame)
        assert not diff, diff[:6]
        o = ob.OraclePT(TP.scene_of(key), rx, ry, TP.make_options(ob, kw), table, scene.DATA_DIR)
        o.psf_enable(ob.default_psf_options())
        for inst in instances:
            o.render_pass(inst)
        diff = compare_cells(cells, o.psf_cells(), "device vs oracle cells") + TP.compare_frames(frame, o.fb)
        assert not diff, diff[:6]
    finally:
        r.close()


@pytest.mark.gpu
def test_sharded_equals_one_replay(table, olib):
    """two contexts on one GPU with checkerboard pixel lists, each importing the other's records: the union of the cells and the assembled frame equal ONE replay of
    the full frame (psf_set_sharded, psf_export_cells / psf_import_cells, psf_finish: collect, merge, clear); the references, read while the pass is pending, are
    the replay's, split by pixel list"""
    import fermat_amd as fa
    key, rx, ry, kw = JP
    opts, popts = TP.make_options(fa, kw), fa.default_psf_options()
    a = TP.pixel_list("checker", rx, ry)
    b = np.setdiff1d(np.arange(rx * ry, dtype=np.uint32), a).astype(np.uint32)
    rs = [fa.Renderer(TP.scene_of(key), rx, ry, opts, table=table, psf_options=popts, pixels=p) for p in (a, b)]
    try:
        for r in rs:
            r.psf_set_sharded(True)
            r.psf_render(0, sync=True)
        refs = [refs_by_pixel(r.psf_refs()) for r in rs]
        # every rank's records, as a host would put them on the wire, merged into every rank's copy of the global table (its own included, as the exchange does)
        from fermat_amd.distributed import device_bytes, PSF_RECORD_BYTES
        exported = []
        for r in rs:
            ptr, n = r.psf_export_cells()
            assert n > 0
            exported.append(device_bytes(ptr, n * PSF_RECORD_BYTES, r.dev).clone())
        for r in rs:
            for e in exported:
                r.psf_import_cells(e.data_ptr(), e.numel() // PSF_RECORD_BYTES)
            r.psf_finish(sync=True)
        cells = [r.psf_cells() for r in rs]
        frames = [r.framebuffer().copy() for r in rs]
        mine, mframe = sequential_replay(rs[0], table, (0,), popts, opts)
        diff = []
        for k, px in enumerate((a, b)):
            diff += compare_cells(mine[0]["cells"], cells[k], "rank %d: the global table" % k)
            for c in range(8):
                if not np.array_equal(mframe[c][px].view(np.uint32), frames[k][c][px].view(np.uint32)):
                    diff.append("rank %d: frame channel %d differs" % (k, c))
            own = [{p: v for p, v in bounce.items() if p in set(px.tolist())} for bounce in mine[0]["refs"]]
            diff += compare_refs(own, refs[k], "rank %d" % k)
        assert not diff, diff[:6]
    finally:
        for r in rs:
            r.close()
