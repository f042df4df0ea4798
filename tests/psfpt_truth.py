"""The judge of the glue of the path-space-filtering path tracer: ONE pass of `-psfpt` for a list of pixels, restated in plain numpy float32 and Python integers from
the reference's text.  It is tests/path_truth.py's replay (the loop, the queues, the samplers, the light samples, the scattering) with the PSFPT's vertex processor
plugged into the reference's five call sites, plus the reference queue, the blend and the pass's tail:

  src/psfpt_vertex_processor.h:83-90      clamp_sample
  src/psfpt_vertex_processor.h:101-195    preprocess_vertex: when a cache vertex opens, the jitter, the flipped normal, the filter scale, the count, the reference
  src/psfpt_vertex_processor.h:213-266    compute_nee_weights: out_vertex_info, the demodulated diffuse weight at a new and valid entry
  src/psfpt_vertex_processor.h:283-317    compute_scattering_weights: the id that travels on, the demodulated weight of a new entry that scatters diffusely
  src/psfpt_vertex_processor.h:330-379    accumulate_emissive: the clamp, the image before a cache vertex exists, the previous vertex's cell after
  src/psfpt_vertex_processor.h:393-469    accumulate_nee: the cell's share (stated here); the frame's share is frame_truth.psf_accumulate_nee
  src/pathtracer_core.h:851-858           preprocess_vertex is handed prev_vertex_info, the word the scatter queue carried
  src/pathtracer_core.h:943-984, 1064-1102  compute_nee_weights computes out_vertex_info -- and trace_shadow_ray is handed vertex_info
  src/pathtracer_core.h:1147              accumulate_emissive reads prev_vertex_info
  src/pathtracer_core.h:1196-1241         compute_scattering_weights' out_vertex_info goes on the scatter queue
  src/renderers/psfpt_impl.h:55-72        PSFRefQueue: PixelInfo, CacheInfo(slot, ALL_COMPS, 0), the two float4 weights
  src/renderers/psfpt_impl.h:110-152      psf_blending_kernel: the cell over its count, the comp-selected total through min(., firefly), the two channel terms
  src/renderers/psfpt_impl.h:287-299      render: rescale, the pass, update_variances, clamp_frame(100)
  src/renderers/psfpt_impl.h:387-406      the cache reset at instance % psf_temporal_reuse == 0, the reference queue reset, the loop, the blend
  src/filters.h:57-72                     modulate / demodulate: by max(c, 1e-4)

Like path_truth it imports neither the library nor the oracle and owns ONLY the glue.  Every piece with a judge of its own comes from the provider:
path_truth's provider (vertex ops 7 and 9 now with psf_mode and the demodulating albedo passed as DATA: the decision is made here), and

  provider.psf(0, rec) -> uint64 keys         the jittered spatial hash of (n, 32) records (include/fermat_pt_hip.h, fpt_debug_psf op 0)
  provider.psf(2, rec, size, firefly) -> (size, 4) int64   psf_clamp + psf_add of (n, 4) records (slot bits, value): the clamped emissions as 2^-32 fixed point

Every key the provider returns is logged with its record (Processor.key_log); tests/test_psfpt_truth.py holds each of them to psf_truth's admissible set.  The table
is a Python dict keyed by the KEY; a cell is four Python integers (three 2^-32 fixed-point sums, the count), psf_truth.fixed / mean_f32 are the arithmetic.  Slot
numbers do not exist here: under collisions they depend on thread order, keys do not.  The frame goes through frame_truth.render_pass(psf=True, firefly,
clamp_max=100); an emission arrives there clamped, because the clamp is this replay's rule.

DEFINED HERE as the device and the oracle define it (the reference is order dependent): the cells are integer sums, so their value does not depend on the order of
the additions; a pixel's blends are applied bounce by bounce after all its samples (the reference appends to ONE queue in warp order).

OUT OF SCOPE: a table that fills up (psf_debug_set_table_log2(8)): which vertex gets the last slot is decided by thread order there, and no replay can be exact.

Reference quirks reproduced on purpose:
  * the shadow queue carries vertex_info, NOT compute_nee_weights' out_vertex_info (src/pathtracer_core.h:984, 1102): its comp bits are 0, so `diffuse_only` never
    fires, and at a new entry w_d + w_g -- the demodulated diffuse term and the un-demodulated glossy one -- goes to the cell and nothing to the frame; below
    psf_depth the word is invalid either way
  * the NEE term is added to the cell UNCLAMPED (:429-431); only emissions and the frame's terms go through clamp_sample
  * a glossy bounce from an invalid id retains the invalid id even where THIS vertex opened a cell (:304-306): that cell gets its own NEE and nothing from further on,
    and the next vertex may open another
  * the reference of a new entry is weighted by w modulate(diffuse) with .w = 0 x max(diffuse.w, 1e-4) = 0

Three tests of the reference's text decide nothing, because another rule already implies them; a mistake about one of them yields the same program, so they are
NOT in WRONG (UNOBSERVABLE below names them, tests/test_psfpt_truth.py shows the replays equal):
  * "the glossy reference is zero at bounce 0" (`&& context.in_bounce`, :185): the primary PixelInfo has comp 0, so both references are zero at bounce 0 anyway
  * "psf_mode 2 only at or beyond psf_depth" (`out_cache_info.is_valid()`, :256): an entry is new only where in_bounce >= psf_depth let it open
  * "the blend starts at psf_depth" (the device's per-bounce loop): no reference exists below psf_depth

`wrong` names ONE deliberate mistake (WRONG below): the same replay with that mistake built in; tests/test_psfpt_truth.py records which case refuses which."""
import numpy as np

import frame_truth as FT
import path_truth as PT
import psf_truth as PSF

F32 = np.float32
U32 = np.uint32
EMPTY = PSF.EMPTY                                   # the key of "no cache vertex": CacheInfo::INVALID_SLOT
DIFFUSE_COMP, ALL_COMPS = 1, 3
VINFO = np.dtype([("key", "<u8"), ("new", "?")])    # CacheInfo(slot, 0, new_entry) with the slot named by its key

WRONG = ("shadow_out_vertex_info",      # 1  the shadow queue carries out_vertex_info
         "filter_scale_2",              # 2  filter scale 2 at every bounce
         "jitter_no_instance",          # 3  the jitter hash without the instance term
         "normal_not_flipped",          # 4  the normal not flipped towards `in`
         "count_on_creation",           # 5  the count incremented only by the vertex that creates the cell
         "scatter_demod_cached",        # 6  the scattering weight demodulated at every cached vertex, not only a new one
         "glossy_opens_all",            # 7  a glossy bounce from an invalid id carries (slot, ALL_COMPS) instead of the invalid id
         "emission_to_frame",           # 8  emission after a cache vertex sent to the frame
         "emission_unclamped",          # 9  the emission not clamped
         "reset_at_1",                  # 10 the cache reset at instance % reuse == 1
         "blend_after_clamp",           # 11 the blend after clamp_frame
         "max_prob_dropped",            # 12 the p_prev < psf_max_prob test dropped
         "nee_cell_clamped",            # 13 the cell's NEE share clamped like the frame's
         "ref_unmodulated")             # 14 the reference weighted by w without the albedo
UNOBSERVABLE = ("glossy_ref_bounce0", "mode2_below_depth", "blend_from_0")

PSF_OPTION_NAMES = ("psf_depth", "psf_width", "psf_min_dist", "psf_max_prob", "psf_temporal_reuse", "firefly_filter")


def sel_max(a, b):
    """cugar::max(a, b) = a > b ? a : b, elementwise"""
    return np.where(a > b, a, b)


def modulate(f, c):
    return f * sel_max(c, F32(1.0e-4))


def demodulate(f, c):
    return f / sel_max(c, F32(1.0e-4))


def scene_bbox(scn):
    """renderer.compute_bbox(): over the mesh vertices"""
    v = np.asarray(scn.vertex_data, F32)[:, :3]
    return v.min(0), v.max(0)


class Cache:
    """what outlives a pass: key -> [sum x, sum y, sum z, count], Python integers"""

    def __init__(self):
        self.cells = {}

    def as_arrays(self):
        keys = sorted(self.cells)
        wrap = lambda q: ((q + (1 << 63)) & EMPTY) - (1 << 63)  # noqa: E731
        return dict(keys=np.array(keys, np.uint64), counts=np.array([self.cells[k][3] for k in keys], np.uint64),
                    sums=np.array([[wrap(q) for q in self.cells[k][:3]] for k in keys], np.int64).reshape(-1, 3))


class Processor:
    """PSFPTVertexProcessor for one pass, as path_truth.replay_pass calls it"""

    def __init__(self, prov, scn, res_x, res_y, instance, popt, cache, wrong=None):
        assert wrong is None or wrong in WRONG or wrong in UNOBSERVABLE
        self.prov, self.res, self.instance, self.o, self.cache, self.wrong = prov, (res_x, res_y), int(instance), popt, cache, wrong
        self.lo, self.hi = scene_bbox(scn)
        self.ff = F32(popt["firefly_filter"])
        self.refs = {}                    # bounce -> list of (pixel_info, key, w_d float4, w_g float4)
        self.key_log = []                 # (records, keys) of every vertex that asked for a key
        self.diffuse = None
        self.counts = dict(opened=0, opened_b0=0, opened_b1=0, opened_after_glossy=0, shared=0, max_prob_refused=0, emission_to_cell=0, emission_to_frame=0,
                           emission_clamped=0, nee_to_cell=0, nee_to_frame=0, nee_frame_clamped=0, glossy_ref=0, id_retained=0, scatter_demodulated=0, mode2=0)

    def primary(self, n):
        v = np.zeros(n, VINFO); v["key"] = EMPTY          # CacheInfo::INVALID
        return v

    def add(self, key, v):
        c = self.cache.cells[int(key)]
        for k in range(3):
            c[k] += PSF.fixed(v[k])

    # ---- preprocess_vertex ---------------------------------------------------------------------------------------------------------------------------------
    def preprocess(self, b, pinfo, prev, sp, pos, inn, cone_radius, w, p_prev, diffuse):
        o, wr = self.o, self.wrong
        m = len(pinfo)
        self.diffuse = np.asarray(diffuse, F32)
        vx = np.zeros(m, VINFO); vx["key"] = prev["key"]          # new_cache_slot = prev_cache_info.pixel
        low = p_prev < F32(o["psf_max_prob"])
        eligible = (prev["key"] == EMPTY) & (b >= o["psf_depth"])
        self.counts["max_prob_refused"] += int((eligible & ~low).sum())
        opens = np.nonzero(eligible & (low | (wr == "max_prob_dropped")))[0]
        if not len(opens):
            return vx
        pixel = (pinfo[opens] & U32(0x7FFFFFF)).astype(np.int64)
        comp = ((pinfo[opens] >> U32(27)) & U32(0xF)).astype(np.int64)
        # pixel_hash = pixel + instance * res_x * res_y, in uint32
        inst = 0 if wr == "jitter_no_instance" else self.instance
        base = (((inst * self.res[0]) & 0xFFFFFFFF) * self.res[1]) & 0xFFFFFFFF
        jitter = np.array([[PT.randfloat(k, (int(p) + base) & 0xFFFFFFFF) for k in range(6)] for p in pixel], F32).reshape(-1, 6)
        n_s = sp[opens, 6:9]
        toward = PT.dot(inn[opens], n_s) > 0
        N = n_s if wr == "normal_not_flipped" else np.where(toward[:, None], n_s, -n_s)
        rec = np.zeros((len(opens), 32), F32)
        rec[:, 0:3] = pos[opens]; rec[:, 3:6] = N; rec[:, 6:9] = sp[opens, 9:12]; rec[:, 9:12] = sp[opens, 12:15]; rec[:, 12:15] = self.lo; rec[:, 15:18] = self.hi
        rec[:, 18:24] = jitter
        rec[:, 24] = cone_radius[opens] * F32(o["psf_width"])                                   # cone_radius * cone_scale
        rec[:, 25] = 2.0 if (b == 0 or wr == "filter_scale_2") else 1.0                          # filter_scale
        keys = np.asarray(self.prov.psf(0, rec), np.uint64)
        self.key_log.append((rec, keys))
        # modulate(Vector4f(w, 0), diffuse): .w = 0 x max(diffuse.w, 1e-4) = 0
        w_mod = np.zeros((len(opens), 4), F32)
        w_mod[:, :3] = w[opens] if wr == "ref_unmodulated" else modulate(w[opens], self.diffuse[opens])
        zero = np.zeros(4, F32)
        for j, k in enumerate(opens):
            key = int(keys[j])
            created = key not in self.cache.cells
            if created:
                self.cache.cells[key] = [0, 0, 0, 0]
            if created or wr != "count_on_creation":
                self.cache.cells[key][3] += 1
            self.counts["shared"] += 0 if created else 1
            w_d = w_mod[j] if (comp[j] & FT.DIFFUSE_MASK) else zero
            w_g = w_mod[j] if ((comp[j] & FT.GLOSSY_MASK) and (b or wr == "glossy_ref_bounce0")) else zero
            self.refs.setdefault(b, []).append((int(pinfo[k]), key, w_d.copy(), w_g.copy()))
            self.counts["glossy_ref"] += int(w_g.any())
            self.counts["opened_after_glossy"] += int(bool(comp[j] & FT.GLOSSY_MASK))
        self.counts["opened"] += len(opens)
        if b <= 1:
            self.counts["opened_b0" if b == 0 else "opened_b1"] += len(opens)
        vx["key"][opens] = keys; vx["new"][opens] = True
        return vx

    # ---- compute_nee_weights ---------------------------------------------------------------------------------------------------------------------------------
    def nee_mode(self, b, vx):
        """psf_mode 2 (the diffuse weight demodulated) at a new AND valid entry: valid = at or beyond psf_depth with a slot"""
        deep = (b >= self.o["psf_depth"]) or self.wrong == "mode2_below_depth"
        mode = np.where(vx["new"] & deep & (vx["key"] != EMPTY), 2, 1)
        return mode, self.diffuse

    def shadow_word(self, b, vx, k):
        """(key, comp) of the word trace_shadow_ray is handed: vertex_info = CacheInfo(slot, 0, new)"""
        key = int(vx["key"][k])
        if self.wrong != "shadow_out_vertex_info":
            return key, 0
        if b < self.o["psf_depth"]:
            return EMPTY, ALL_COMPS
        return key, (DIFFUSE_COMP if vx["new"][k] else ALL_COMPS)

    # ---- accumulate_nee (an unoccluded sample) ---------------------------------------------------------------------------------------------------------------
    def nee(self, b, kind, pix, comp, vx, k, w_d, w_g, samples):
        key, ccomp = self.shadow_word(b, vx, k)
        cached, diffuse_only = key != EMPTY, ccomp == DIFFUSE_COMP
        self.counts["mode2"] += int(bool(vx["new"][k]))
        if cached:
            v = w_d if diffuse_only else w_d + w_g
            self.add(key, PSF.clamp(v, self.ff) if self.wrong == "nee_cell_clamped" else v)
            self.counts["nee_to_cell"] += 1
        if not cached or diffuse_only:
            self.counts["nee_to_frame"] += 1
            terms = [w_d + w_g] + ([w_d, w_g] if b == 0 else [])
            self.counts["nee_frame_clamped"] += int(any((t > self.ff).any() for t in terms))
        samples[pix].append((b, kind, comp, w_d, w_g, cached, diffuse_only))          # frame_truth.psf_accumulate_nee: the frame's share, nothing when all went to the cell

    # ---- accumulate_emissive ---------------------------------------------------------------------------------------------------------------------------------
    def emissive(self, b, pix, comp, prev, e, samples):
        c = e if self.wrong == "emission_unclamped" else PSF.clamp(e, self.ff)
        self.counts["emission_clamped"] += int((e > self.ff).any())
        if prev["key"] == EMPTY or self.wrong == "emission_to_frame":
            samples[pix].append((b, FT.EMISSIVE, comp, c))
            self.counts["emission_to_frame"] += 1
        else:
            self.add(prev["key"], c)
            self.counts["emission_to_cell"] += 1
            self.cell_emissions.append((int(prev["key"]), np.asarray(e, F32)))

    cell_emissions = None

    # ---- compute_scattering_weights --------------------------------------------------------------------------------------------------------------------------
    def scatter_weight(self, b, vx, comp, g, w, out_w):
        fresh = (vx["key"] != EMPTY) if self.wrong == "scatter_demod_cached" else vx["new"]
        sel = fresh & ((comp & FT.DIFFUSE_MASK) != 0)
        self.counts["scatter_demodulated"] += int(sel.sum())
        return np.where(sel[:, None], demodulate(g, self.diffuse), out_w).astype(F32)

    def scatter_info(self, b, prev, vx, comp, keep):
        out = np.zeros(len(comp), VINFO)
        retain = (prev["key"] == EMPTY) & ((comp & FT.GLOSSY_MASK) != 0)
        if self.wrong == "glossy_opens_all":
            retain[:] = False
        out["key"] = np.where(retain, np.uint64(EMPTY), vx["key"])          # the invalid id retained, or CacheInfo(slot, ALL_COMPS, 0)
        self.counts["id_retained"] += int((retain & (vx["key"] != EMPTY))[keep].sum())
        return out[keep]


def blend_samples(proc, samples):
    """psf_blending_kernel on the pass's references, bounce by bounce: per reference the sample frame_truth.psf_blend takes.  Returns the number of blends whose
    composited term the firefly filter clamped"""
    clamped = 0
    with np.errstate(all="ignore"):
        first = 0 if proc.wrong == "blend_from_0" else proc.o["psf_depth"]          # bounce by bounce from psf_depth
        for b in sorted(k for k in proc.refs if k >= first):
            for pinfo, key, w_d, w_g in proc.refs[b]:
                c = proc.cache.cells[key]
                wrap = lambda q: ((q + (1 << 63)) & EMPTY) - (1 << 63)  # noqa: E731
                cv = PSF.mean_f32(np.array([[wrap(c[0]), wrap(c[1]), wrap(c[2]), c[3]]], np.int64))[0]          # cache_value /= cache_value.w
                comp = (pinfo >> 27) & 0xF
                zero = np.zeros(3, F32)
                w = (w_d[:3] if comp & FT.DIFFUSE_MASK else zero) + (w_g[:3] if comp & FT.GLOSSY_MASK else zero)
                cvw = cv * w
                composited = np.asarray([FT.sel_min(x, proc.ff) for x in cvw], F32)                               # cugar::min(v, firefly)
                clamped += int((cvw > proc.ff).any())
                samples[pinfo & 0x7FFFFFF].append((b, FT.BLEND, comp, composited, cv * w_d[:3], cv * w_g[:3]))
    return clamped


def replay_pass(prov, scn, res_x, res_y, options, psf_options, instance, shifts, cache, pixels=None, wrong=None):
    """ONE pass of PSFPT::render_pass on `cache` (updated in place; shared by the passes of a reuse window).  Returns path_truth's replay plus refs (per bounce a list
    of (pixel_info, key, w_d, w_g)), psf_counts, key_log and the options the frame needs"""
    popt = {k: (float(psf_options[k]) if k in ("psf_width", "psf_min_dist", "psf_max_prob", "firefly_filter") else int(psf_options[k])) for k in PSF_OPTION_NAMES}
    # initialize the shading cache: instance % psf_temporal_reuse == 0
    if instance % popt["psf_temporal_reuse"] == (1 if wrong == "reset_at_1" else 0):
        cache.cells.clear()
    proc = Processor(prov, scn, res_x, res_y, instance, popt, cache, wrong)
    proc.cell_emissions = []
    rep = PT.replay_pass(prov, scn, res_x, res_y, options, instance, shifts, pixels, None, psf=proc)
    # psf_clamp + psf_add as the provider's probe runs them: the emissions that went to a cell, one slot each, against psf_truth's arithmetic used above
    if proc.cell_emissions and wrong is None:
        er = np.zeros((len(proc.cell_emissions), 4), F32)
        er[:, 0] = PT.bits_f32(np.arange(len(er))); er[:, 1:] = [e for _, e in proc.cell_emissions]
        got = np.asarray(prov.psf(2, er, len(er), float(proc.ff)), np.int64).reshape(-1, 4)
        assert np.array_equal(got, PSF.judge_cells(er, len(er), proc.ff)), "the provider's psf_clamp / psf_add disagree with psf_truth"
    proc.counts["blend_clamped"] = blend_samples(proc, rep["samples"])
    rep.update(refs=proc.refs, psf_counts=proc.counts, key_log=proc.key_log, firefly=proc.ff)
    return rep


def apply_pass(frame, rep, instance, wrong=None):
    """PSFPT::render on the frame (8, n_pixels, 4), in place: rescale, the pass's samples, its blends, update_variances, clamp_frame(100)"""
    with np.errstate(all="ignore"):
        for p in rep["pixels"]:
            p = int(p)
            px = frame[:, p, :].copy()
            s = rep["samples"][p]
            if wrong == "blend_after_clamp":
                FT.render_pass(px, instance, [x for x in s if x[1] != FT.BLEND], rep["albedo"].get(p), psf=True, firefly=rep["firefly"], clamp_max=100.0)
                add = FT.Adder(px, FT.frame_weight(instance), None, rep["firefly"])
                for x in FT.pass_order([x for x in s if x[1] == FT.BLEND]):
                    FT.apply_sample(add, x, True, rep["firefly"])
            else:
                FT.render_pass(px, instance, s, rep["albedo"].get(p), psf=True, firefly=rep["firefly"], clamp_max=100.0)
            frame[:, p, :] = px
