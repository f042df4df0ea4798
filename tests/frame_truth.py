"""The judge of the frame path: what a pass does to ONE pixel of the eight-channel frame, written from the reference's text in plain numpy float32, one operation per
rounding (the library is built without contraction and with a correctly rounded divide, so float32 numpy is exact):

  src/renderer.cu:292-362                         multiply_frame, clamp_frame, update_variances
  src/framebuffer.h:425-444                       add_in
  src/pathtracer_vertex_processor.h:151-239       accumulate_emissive, accumulate_nee
  src/psfpt_vertex_processor.h:84-90, 395-469     clamp_sample, accumulate_nee (the frame's part)
  src/renderers/psfpt_impl.h:139-149, 290-298     the blend's three terms; rescale, the pass, variances, clamp_frame(100)

It knows nothing of the device code but the LAYOUT of the contribution log (the comment above ContribLog in fermat_amd/csrc/fpt_device.h), which has no counterpart
in the reference: `merge_replay` reads a log the way that comment says and applies each pass as render() would have.

Spelled out, because each is a place to go wrong:
  * max_comp is max(max(x, y), z) and max / min are `a > b ? a : b` / `a < b ? a : b` (contrib/cugar/basic/numbers.h:536-540, linalg/vector_inl.h:509-516)
  * update_variances divides by n * n, a uint32 product converted to float; n = instance + 1.  Defined here for base_instance + n_passes < 65536 (beyond, the
    product wraps -- in the reference too)
  * LUMINANCE is written by multiply_frame, before the scaling, and only there
  * a merge leaves the albedo planes and the mask words it visited zero, and never reads a cell whose bit is clear

The PSFPT's clamp of an EMISSION is not this judge's rule: PSFPTVertexProcessor::accumulate_emissive clamps its sample itself (src/psfpt_vertex_processor.h:351) and
then adds it as the path tracer's does; on the device that clamp (and the choice between the image and the cache cell) sits in shade_kernel, at the call of
accumulate_emissive, which the frame probe does not run.  So `accumulate_emissive` below takes the value as it arrives, for both renderers, and an emission here is
what is left after the clamp.  The clamp and the choice are judged by the replay of a whole pass, tests/psfpt_truth.py (Processor.emissive; its mistakes
"emission_unclamped" and "emission_to_frame"), which hands this module emissions that are already clamped.

`wrong` names ONE deliberate mistake (WRONG below): the same replay with that mistake built in.  tests/test_frame_truth.py uses them to show that its inputs are
sharp enough to tell each mistake from the truth."""
import numpy as np

F32 = np.float32
U32 = np.uint32
DIFFUSE_C, DIFFUSE_A, SPECULAR_C, SPECULAR_A, DIRECT_C, COMPOSITED_C, FILTERED_C, LUMINANCE = range(8)
DIFFUSE_MASK, GLOSSY_MASK = 0x3, 0xC          # Bsdf::kDiffuseMask, kGlossyMask
EMISSIVE, NEE_DIRECTIONAL, NEE_MESH, BLEND = 0, 1, 2, 3          # the kinds of a sample, in the order a pass delivers them within a bounce (the blends: after all bounces)

WRONG = ("swapped_kinds",            # two kinds of one bounce applied in swapped order
         "composited_variance",      # COMPOSITED_C with the variance term
         "comp_ignored",             # comp bits ignored at bounce > 0
         "emission_to_diffuse",      # bounce-0 emission also sent to DIFFUSE_C
         "mask_kept",                # the merge does not clear the mask
         "blends_first",             # blends applied before the samples
         "psf_wd_alone",             # w_d without w_g in the un-cached PSF term at bounce > 0
         "clamp_after_sum",          # the firefly clamp applied to the channel after the add instead of to each term before it
         "clamp_skips_w",            # clamp_frame leaves .w alone
         "variance_n",               # update_variances with n in place of n - 1
         "stale_cell_read")          # a cell whose bit is clear is applied too


def sel_max(a, b):
    return a if a > b else b


def sel_min(a, b):
    return a if a < b else b


def max_comp(v):
    return sel_max(sel_max(v[0], v[1]), v[2])


def frame_weight(instance):
    return F32(1.0) / F32(instance + 1)


# ---- the bracket --------------------------------------------------------------------------------------------------------------------------------------------------------
def multiply_frame(px, scale):
    """px: one pixel, (8, 4) float32, in place"""
    px[LUMINANCE] = (max_comp(px[DIRECT_C]), max_comp(px[DIFFUSE_C]), max_comp(px[SPECULAR_C]), max_comp(px[COMPOSITED_C]))
    for c in (DIFFUSE_C, DIFFUSE_A, SPECULAR_C, SPECULAR_A, DIRECT_C, COMPOSITED_C):
        px[c] = px[c] * F32(scale)


def rescale_frame(px, instance):
    multiply_frame(px, F32(instance) / F32(instance + 1))


def clamp_frame(px, max_value, wrong=None):
    for c in (DIFFUSE_C, SPECULAR_C, DIRECT_C, COMPOSITED_C):
        for k in range(3 if wrong == "clamp_skips_w" else 4):
            px[c, k] = sel_min(px[c, k], F32(max_value))


def update_variances(px, n, wrong=None):
    n = int(n)
    assert 1 <= n < 65536
    fn, fn1, fnn = F32(n), F32(n if wrong == "variance_n" else n - 1), F32(int(U32((n * n) & 0xFFFFFFFF)))
    old = px[LUMINANCE].copy()
    new = (max_comp(px[DIRECT_C]), max_comp(px[DIFFUSE_C]), max_comp(px[SPECULAR_C]), max_comp(px[COMPOSITED_C]))
    for k, c in enumerate((DIRECT_C, DIFFUSE_C, SPECULAR_C, COMPOSITED_C)):
        d = F32(new[k] - old[k])
        px[c, 3] = px[c, 3] + ((fn * d) * (fn1 * d)) / fnn


# ---- add_in and the vertex processors -----------------------------------------------------------------------------------------------------------------------------------
def add_in(px, c, f, inv_n, variance):
    f = np.asarray(f, F32)
    delta = f - px[c, :3]
    px[c, :3] = px[c, :3] + f * inv_n
    if variance:
        ld = max_comp(delta)
        px[c, 3] = px[c, 3] + (ld * ld) * inv_n


class Adder:
    """add_in on one pixel with one frame weight; the place where the mistakes about single adds live"""

    def __init__(self, px, w, wrong=None, firefly=None):
        self.px, self.w, self.wrong, self.firefly = px, F32(w), wrong, firefly

    def __call__(self, c, variance, f, clamped=False):
        """clamped: the term went through clamp_sample (the PSFPT's); with "clamp_after_sum" it arrives raw and the channel is clamped after the add"""
        if c == COMPOSITED_C and self.wrong == "composited_variance":
            variance = True
        add_in(self.px, c, f, self.w, variance)
        if clamped and self.wrong == "clamp_after_sum":
            self.px[c, :3] = clamp_sample(self.px[c, :3], self.firefly)


def clamp_sample(v, firefly):
    v = np.asarray(v, F32)
    if not np.isfinite(v).all():
        return np.zeros(3, F32)
    return np.asarray([sel_min(x, F32(firefly)) for x in v], F32)


def accumulate_emissive(add, bounce, comp, e):
    add(COMPOSITED_C, False, e)
    if bounce == 0:
        add(DIRECT_C, False, e)
        if add.wrong == "emission_to_diffuse":
            add(DIFFUSE_C, True, e)
    else:
        every = add.wrong == "comp_ignored"
        if (comp & DIFFUSE_MASK) or every:
            add(DIFFUSE_C, True, e)
        if (comp & GLOSSY_MASK) or every:
            add(SPECULAR_C, True, e)


def accumulate_nee(add, bounce, comp, w_d, w_g):
    w_d = np.asarray(w_d, F32); w_g = np.asarray(w_g, F32)
    add(COMPOSITED_C, False, w_d + w_g)
    if bounce == 0:
        add(DIFFUSE_C, True, w_d)
        add(SPECULAR_C, True, w_g)
    else:
        every = add.wrong == "comp_ignored"
        if (comp & DIFFUSE_MASK) or every:
            add(DIFFUSE_C, True, w_d)
        if (comp & GLOSSY_MASK) or every:
            add(SPECULAR_C, True, w_g)


def psf_accumulate_nee(add, bounce, comp, cached, diffuse_only, w_d, w_g, firefly):
    """the frame's part of PSFPTVertexProcessor::accumulate_nee for an unoccluded sample: `cached` = cache_info.is_valid(), `diffuse_only` = its comp is DIFFUSE_COMP"""
    w_d = np.asarray(w_d, F32); w_g = np.asarray(w_g, F32)
    late = add.wrong == "clamp_after_sum"
    cl = (lambda v: np.asarray(v, F32)) if late else (lambda v: clamp_sample(v, firefly))
    if cached:
        if diffuse_only:
            add(COMPOSITED_C, False, cl(w_g), True)
            add(SPECULAR_C if (bounce == 0 or (comp & GLOSSY_MASK)) else DIFFUSE_C, True, cl(w_g), True)
        return
    add(COMPOSITED_C, False, cl(w_d + w_g), True)
    if bounce == 0:
        add(DIFFUSE_C, True, cl(w_d), True)
        add(SPECULAR_C, True, cl(w_g), True)
    else:
        both = w_d if add.wrong == "psf_wd_alone" else w_d + w_g
        every = add.wrong == "comp_ignored"
        if (comp & DIFFUSE_MASK) or every:
            add(DIFFUSE_C, True, cl(both), True)
        if (comp & GLOSSY_MASK) or every:
            add(SPECULAR_C, True, cl(both), True)


def psf_blend(add, comp, composited, diffuse, glossy):
    """psf_blending_kernel's three adds, on the three terms as the blend computed them (composited already through min(., firefly))"""
    add(COMPOSITED_C, False, composited)
    every = add.wrong == "comp_ignored"
    if (comp & DIFFUSE_MASK) or every:
        add(DIFFUSE_C, True, diffuse)
    if (comp & GLOSSY_MASK) or every:
        add(SPECULAR_C, True, glossy)


# ---- one pass on one pixel --------------------------------------------------------------------------------------------------------------------------------------------
def apply_sample(add, s, psf, firefly):
    """s = (bounce, kind, comp, a, b[, c][, cached, diffuse_only]): EMISSIVE a = the emission; NEE_* a = w_d, b = w_g (psf: + the two cache flags); BLEND a, b, c = the three terms"""
    bounce, kind, comp = s[0], s[1], s[2]
    if kind == EMISSIVE:
        accumulate_emissive(add, bounce, comp, s[3])
    elif kind == BLEND:
        psf_blend(add, comp, s[3], s[4], s[5])
    elif psf:
        psf_accumulate_nee(add, bounce, comp, s[5], s[6], s[3], s[4], firefly)
    else:
        accumulate_nee(add, bounce, comp, s[3], s[4])


def pass_order(samples, wrong=None):
    """the order render() delivers a pixel's samples in: bounce by bounce, emission, directional light, mesh light; then the blends, bounce by bounce"""
    kind_rank = {EMISSIVE: 0, NEE_DIRECTIONAL: 1, NEE_MESH: 2}
    if wrong == "swapped_kinds":
        kind_rank = {EMISSIVE: 2, NEE_DIRECTIONAL: 0, NEE_MESH: 1}          # every pair of kinds changes places with at least one other
    blend_rank = 0 if wrong == "blends_first" else 2
    return sorted(samples, key=lambda s: (blend_rank, s[0], 0) if s[1] == BLEND else (1, s[0], kind_rank[s[1]]))


def render_pass(px, instance, samples, albedo=None, psf=False, firefly=None, clamp_max=None, wrong=None):
    """one render() on one pixel: rescale_frame, the pass's samples in order, update_variances and, for the PSFPT, clamp_frame.  albedo = (diffuse, specular) float4
    terms of the primary vertex, added as they are (the merge's planes)"""
    rescale_frame(px, instance)
    if albedo is not None:
        px[DIFFUSE_A] = px[DIFFUSE_A] + np.asarray(albedo[0], F32)
        px[SPECULAR_A] = px[SPECULAR_A] + np.asarray(albedo[1], F32)
    add = Adder(px, frame_weight(instance), wrong, firefly)
    for s in pass_order(samples, wrong):
        apply_sample(add, s, psf, firefly)
    update_variances(px, instance + 1, wrong)
    if psf and clamp_max is not None and clamp_max > 0:
        clamp_frame(px, clamp_max, wrong)


# ---- the contribution log ---------------------------------------------------------------------------------------------------------------------------------------------
def as_u32(x):
    return int(np.asarray(x, F32).view(U32))


def log_samples(log, pidx, cap, mask_words, n_bounces, psf, wrong=None):
    """the samples of path `pidx` that the log holds -- the cells its mask bits name (all cells with "stale_cell_read") -- as apply_sample takes them.
    emissive [bounce * cap + pidx]; nee[kind] [(bounce * cap + pidx) * 2 + {0, 1}]; blend [(bounce * cap + pidx) * 3 + {0, 1, 2}];
    bit 3 * bounce + {0 emissive, 1 directional, 2 mesh}, 3 * n_bounces + bounce for a blend; .w of a cell's first float4 = comp (| 0x100 cached | 0x200 diffuse_only)"""
    words = log["mask"].reshape(-1, mask_words)[pidx]
    is_set = lambda bit: wrong == "stale_cell_read" or bool((int(words[bit >> 5]) >> (bit & 31)) & 1)  # noqa: E731
    out = []
    for b in range(n_bounces):
        if is_set(3 * b):
            e = log["emissive"][b * cap + pidx]
            out.append((b, EMISSIVE, as_u32(e[3]), e[:3].copy()))
        for kind, name in ((NEE_DIRECTIONAL, "nee0"), (NEE_MESH, "nee1")):
            if is_set(3 * b + kind):
                c = log[name][(b * cap + pidx) * 2:(b * cap + pidx) * 2 + 2]
                tag = as_u32(c[0, 3])
                if psf:
                    out.append((b, kind, tag & 0xF, c[0, :3].copy(), c[1, :3].copy(), bool(tag & 0x100), bool(tag & 0x200)))
                else:
                    out.append((b, kind, tag, c[0, :3].copy(), c[1, :3].copy()))
        if psf and log.get("blend") is not None and is_set(3 * n_bounces + b):
            c = log["blend"][(b * cap + pidx) * 3:(b * cap + pidx) * 3 + 3]
            out.append((b, BLEND, as_u32(c[0, 3]), c[0, :3].copy(), c[1, :3].copy(), c[2, :3].copy()))
    return out


def merge_replay(frame, log, n, acc_stride, cap, mask_words, n_bounces, base_instance, n_passes, pixels=None, p0=0, psf=False, firefly=None, clamp_max=None,
                 wrong=None, only=None):
    """n sequential render() calls on the lane's n pixels from the log of a batch, in place: frame (8, n_pixels, 4), log = dict(albedo_d, albedo_s, emissive, nee0, nee1,
    blend, mask).  Entry i of the lane is path p0 + i of every pass (pidx = k * acc_stride + p0 + i) and pixel pixels[p0 + i] (i without a list).  only: the entries
    to replay (default all)"""
    assert base_instance + n_passes < 65536
    mask = log["mask"].reshape(-1, mask_words)
    with np.errstate(all="ignore"):
        for i in (range(n) if only is None else only):
            p = int(pixels[p0 + i]) if pixels is not None else i
            px = frame[:, p, :].copy()
            for k in range(n_passes):
                pidx = k * acc_stride + p0 + i
                samples = log_samples(log, pidx, cap, mask_words, n_bounces, psf, wrong)
                render_pass(px, base_instance + k, samples, (log["albedo_d"][pidx].copy(), log["albedo_s"][pidx].copy()), psf, firefly, clamp_max, wrong)
                log["albedo_d"][pidx] = 0; log["albedo_s"][pidx] = 0
                if wrong != "mask_kept":
                    mask[pidx] = 0
            frame[:, p, :] = px
