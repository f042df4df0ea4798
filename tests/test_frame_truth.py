"""The frame path of the path tracer and the path-space-filtering path tracer on arrays a test built: the one-pass bracket (rescale_kernel, the FrameAdd adds,
variance_kernel, clamp_frame_kernel), the writers of the contribution log and merge_passes_exact_kernel<false | true>, through the device probe fpt_debug_frame
(Renderer.debug_frame), against tests/frame_truth.py -- plain float32 numpy written from the reference's text, which knows nothing of the device code but the log's
layout.  Every comparison is bit for bit over all eight channels, both albedo planes and every mask word: there are no tolerances here.  Outside this module: the
PSFPT's clamp of an emission, which the device applies in shade_kernel before accumulate_emissive is called (see frame_truth's docstring).

The cases (CASES) are built once.  The CPU tests show that the judge is exact (dyadic inputs against fractions.Fraction, a case done by hand), that it agrees with
the oracle's frame, and that every case tells the truth from each deliberate mistake of frame_truth.WRONG that can show on it; the `gpu` tests run the cases on the
device."""
import functools
from fractions import Fraction

import numpy as np
import pytest

import frame_truth as T

F32, U32 = np.float32, np.uint32
POISON = F32(3.0e30)          # what every cell without a mask bit holds: applied once, it ruins the pixel


def bits(a):
    return np.ascontiguousarray(a).view(U32)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def new_frame(rng, n_pixels, top=4.0):
    """all eight channels filled, FILTERED_C and LUMINANCE too: what a kernel must not touch holds something to lose"""
    return (rng.random((8, n_pixels, 4)) * top).astype(F32)


# ---- merge cases ------------------------------------------------------------------------------------------------------------------------------------------------------
def empty_log(cap, words, nb, psf):
    log = dict(albedo_d=np.zeros((cap, 4), F32), albedo_s=np.zeros((cap, 4), F32), emissive=np.full((nb * cap, 4), POISON, F32),
               nee0=np.full((nb * cap * 2, 4), POISON, F32), nee1=np.full((nb * cap * 2, 4), POISON, F32), mask=np.zeros(cap * words, U32),
               blend=np.full((nb * cap * 3, 4), POISON, F32) if psf else None)
    for k in ("emissive", "nee0", "nee1", "blend"):
        if log[k] is not None:
            log[k][:, 3] = U32(0xF).view(F32)          # a stale cell's tag: every comp bit, so that a stale read lands in every channel
    return log


def big_or_small(rng, shape, big):
    """sample values: most below 4; a share `big` of them (the PSFPT's cases) between 50 and 400, so that the firefly clamp (100) and the per-pass clamp_frame (100)
    bite on some pixels -- and not on all of them: a channel that sits at the clamp hides what went before"""
    v = rng.random(shape) * 4
    if big:
        v = np.where(rng.random(shape) < big, 50 + rng.random(shape) * 350, v)
    return v.astype(F32)


def merge_case(n_pixels, n_passes, base_instance, n_bounces, with_list=False, psf=False, share=0.33, forced_bits=(), acc_stride=None, frame_pixels=None, lanes=None, big=0.1, seed=41):
    """a frame, albedo planes and a log with about `share` of its cells set (plus forced_bits on every path); every cell without a bit is poison.  With a list the
    merge touches a shuffled two thirds of the frame's pixels and must leave the rest alone.  lanes: ((p0, n), ...) = the calls that together cover the paths"""
    rng = np.random.default_rng(seed)
    frame_pixels = frame_pixels or n_pixels
    pixels = rng.permutation(frame_pixels)[:n_pixels].astype(U32) if with_list else None
    acc_stride = acc_stride or n_pixels
    cap = acc_stride * n_passes
    n_bits = (4 if psf else 3) * n_bounces
    words = (n_bits + 31) // 32
    log = empty_log(cap, words, n_bounces, psf)
    log["albedo_d"][:] = rng.random((cap, 4)); log["albedo_s"][:] = rng.random((cap, 4))
    setb = rng.random((cap, n_bits)) < share
    setb[:, list(forced_bits)] = True
    mask = log["mask"].reshape(cap, words)
    for b in range(n_bits):
        mask[:, b >> 5] |= setb[:, b].astype(U32) << U32(b & 31)
    comp = lambda n: rng.integers(0, 16, n).astype(U32)  # noqa: E731   every comp value: no bit, one of a mask's two, both masks
    for b in range(n_bounces):
        rows = np.arange(cap) + b * cap
        on = setb[:, 3 * b]
        log["emissive"][rows[on], :3] = big_or_small(rng, (on.sum(), 3), False); log["emissive"][rows[on], 3] = comp(on.sum()).view(F32)
        for kind, name in ((1, "nee0"), (2, "nee1")):
            on = setb[:, 3 * b + kind]; m = int(on.sum())
            wd, wg = big_or_small(rng, (m, 3), psf and big), big_or_small(rng, (m, 3), psf and big)
            tag = comp(m)
            if psf:
                # all four (cached, diffuse_only) tags; about 2 % of the components +-inf or NaN: each must vanish in the firefly clamp
                tag |= rng.choice(np.asarray([0x000, 0x100, 0x200, 0x300], U32), m)
                for w in (wd, wg):
                    bad = rng.random(w.shape) < 0.02
                    w[bad] = rng.choice(np.asarray([np.inf, -np.inf, np.nan], F32), int(bad.sum()))
            log[name][rows[on] * 2, :3] = wd; log[name][rows[on] * 2, 3] = tag.view(F32)
            log[name][rows[on] * 2 + 1, :3] = wg; log[name][rows[on] * 2 + 1, 3] = 0
        if psf:
            on = setb[:, 3 * n_bounces + b]; m = int(on.sum())
            for j in range(3):
                log["blend"][rows[on] * 3 + j, :3] = np.minimum(big_or_small(rng, (m, 3), big), F32(100)) if j == 0 else big_or_small(rng, (m, 3), False)
                log["blend"][rows[on] * 3 + j, 3] = comp(m).view(F32) if j == 0 else 0
    par = dict(acc_stride=acc_stride, cap=cap, mask_words=words, n_bounces=n_bounces, base_instance=base_instance, n_passes=n_passes, psf=psf,
               firefly=100.0 if psf else 0.0, clamp_max=100.0 if psf else 0.0)
    return dict(kind="merge", frame=new_frame(rng, frame_pixels), log=log, pixels=pixels, par=par, lanes=lanes or ((0, n_pixels),))


def copy_log(log):
    return {k: (None if v is None else v.copy()) for k, v in log.items()}


def judge_merge(case, wrong=None, only=None):
    """the judge's ONE replay over all the case's paths (the lanes are the device's business)"""
    frame, log, p = case["frame"].copy(), copy_log(case["log"]), case["par"]
    n = sum(m for _, m in case["lanes"])
    T.merge_replay(frame, log, n, p["acc_stride"], p["cap"], p["mask_words"], p["n_bounces"], p["base_instance"], p["n_passes"], case["pixels"], 0, p["psf"],
                   p["firefly"], p["clamp_max"], wrong, only)
    return frame, log


def device_merge(r, case):
    frame, log = case["frame"], copy_log(case["log"])
    for p0, n in case["lanes"]:
        frame, log = r.debug_frame("merge", frame, log, pixels=case["pixels"], n=n, p0=p0, **case["par"])
    return frame, log


def assert_merged(got, want, case):
    (gf, gl), (wf, wl) = got, want
    for c in range(8):
        assert same_bits(gf[c], wf[c]), "channel %d differs on %d pixels" % (c, (bits(gf[c]) != bits(wf[c])).any(axis=1).sum())
    for k in ("albedo_d", "albedo_s", "mask", "emissive", "nee0", "nee1", "blend"):
        assert (gl[k] is None and wl[k] is None) or same_bits(gl[k], wl[k]), k
    assert np.isfinite(gf).all()
    if case["pixels"] is not None:
        rest = np.setdiff1d(np.arange(gf.shape[1]), case["pixels"])
        assert len(rest) and same_bits(gf[:, rest], case["frame"][:, rest])
    assert same_bits(gf[T.FILTERED_C], case["frame"][T.FILTERED_C])
    # the planes and the visited mask words are left zero
    seen = np.concatenate([np.arange(p0, p0 + n) for p0, n in case["lanes"]])
    pidx = (np.arange(case["par"]["n_passes"])[:, None] * case["par"]["acc_stride"] + seen[None, :]).reshape(-1)
    assert not gl["albedo_d"][pidx].any() and not gl["albedo_s"][pidx].any() and not gl["mask"].reshape(-1, case["par"]["mask_words"])[pidx].any()


# ---- bracket cases ----------------------------------------------------------------------------------------------------------------------------------------------------
def bracket_case(instance, with_list, seed=43):
    """rescale_kernel and variance_kernel of pass `instance` around nothing but a nudge of the colours (so that the luminance moved), on 300 pixels"""
    rng = np.random.default_rng(seed + instance)
    pixels = rng.permutation(300)[:200].astype(U32) if with_list else None
    return dict(kind="bracket", frame=new_frame(rng, 300), nudge=(rng.random((8, 300, 4)) * 2 - 1).astype(F32), pixels=pixels,
                steps=(("rescale", instance), ("nudge", None), ("variance", instance + 1)))


def clamp_case(with_list, seed=47):
    """clamp_frame_kernel at 100 on a frame with values either side of it in all four components, .w included"""
    rng = np.random.default_rng(seed)
    frame = new_frame(rng, 300, top=200.0)
    frame[:, 7, 3] = 150.0; frame[:, 8, 3] = 50.0; frame[:, 9, :] = 100.0
    pixels = rng.permutation(300)[:200].astype(U32) if with_list else None
    return dict(kind="bracket", frame=frame, nudge=None, pixels=pixels, steps=(("clamp", 100.0),))


def nudged(case, frame):
    """the colours move between the two halves of the bracket, as a pass's samples would move them (host arithmetic on both sides: not under test)"""
    out = frame.copy()
    idx = case["pixels"] if case["pixels"] is not None else np.arange(frame.shape[1])
    for c in (T.DIFFUSE_C, T.SPECULAR_C, T.DIRECT_C, T.COMPOSITED_C):
        out[c, idx, :3] = (frame[c, idx, :3] + case["nudge"][c, idx, :3]).astype(F32)
    return out


def judge_bracket(case, wrong=None, only=None):
    frame = case["frame"].copy()
    idx = case["pixels"] if case["pixels"] is not None else np.arange(frame.shape[1])
    for what, v in case["steps"]:
        if what == "nudge":
            frame = nudged(case, frame)
            continue
        with np.errstate(all="ignore"):
            for p in (idx if only is None else idx[list(only)]):
                px = frame[:, p, :].copy()
                if what == "rescale":
                    T.rescale_frame(px, v)
                elif what == "variance":
                    T.update_variances(px, v, wrong)
                else:
                    T.clamp_frame(px, v, wrong)
                frame[:, p, :] = px
    return frame


def device_bracket(r, case):
    frame = case["frame"]
    for what, v in case["steps"]:
        if what == "nudge":
            frame = nudged(case, frame)
        elif what == "rescale":
            frame, _ = r.debug_frame("bracket", frame, pixels=case["pixels"], kind=0, value=F32(v) / F32(v + 1))
        elif what == "variance":
            frame, _ = r.debug_frame("bracket", frame, pixels=case["pixels"], kind=1, value=v)
        else:
            frame, _ = r.debug_frame("bracket", frame, pixels=case["pixels"], kind=2, value=v)
    return frame


def assert_bracket(got, want, case):
    for c in range(8):
        assert same_bits(got[c], want[c]), "channel %d differs on %d pixels" % (c, (bits(got[c]) != bits(want[c])).any(axis=1).sum())
    if case["pixels"] is not None:
        rest = np.setdiff1d(np.arange(got.shape[1]), case["pixels"])
        assert len(rest) and same_bits(got[:, rest], case["frame"][:, rest])


# ---- the writers' case ------------------------------------------------------------------------------------------------------------------------------------------------
W_PASSES, W_SLOTS, W_PIXELS, W_BOUNCES, W_BASE = 3, 300, 450, 4, 2


def writer_case(psf, seed=53):
    """one list of samples for 3 passes x 300 paths (a shuffled list over a frame of 450 pixels) x 4 bounces x {emission, directional light, mesh light}, about a third
    of them present.  PT: the mesh-light samples go through accumulate_nee or through the FusedResolve block at random.  PSFPT: the light samples go through the
    resolve's frame share with every (cached, diffuse_only) pair -- (cached, all of it) reaches neither frame nor log"""
    rng = np.random.default_rng(seed + int(psf))
    pixels = rng.permutation(W_PIXELS)[:W_SLOTS].astype(U32)
    samples = []          # (k, slot, bounce, kind, comp, a, b, what, flags)
    for k in range(W_PASSES):
        for slot in range(W_SLOTS):
            for b in range(W_BOUNCES):
                for kind in (T.EMISSIVE, T.NEE_DIRECTIONAL, T.NEE_MESH):
                    if rng.random() >= 0.33:
                        continue
                    comp = int(rng.integers(0, 16))
                    a, bb = big_or_small(rng, 3, 0.1 * (psf and kind != T.EMISSIVE)), big_or_small(rng, 3, 0.1 * (psf and kind != T.EMISSIVE))
                    flags = 0
                    if kind == T.EMISSIVE:
                        what = 0
                    elif psf:
                        what, flags = 4, int(rng.integers(0, 4)) | (4 if kind == T.NEE_MESH else 0)
                        if rng.random() < 0.05:
                            a[int(rng.integers(0, 3))] = rng.choice(np.asarray([np.inf, -np.inf, np.nan], F32))
                    else:
                        what = kind if kind == T.NEE_DIRECTIONAL else int(rng.choice([2, 3]))
                    samples.append((k, slot, b, kind, comp, a, bb, what, flags))
    return dict(kind="writer", psf=psf, frame=new_frame(rng, W_PIXELS), pixels=pixels, samples=samples)


def reaches_frame(s):
    return not (s[7] == 4 and (s[8] & 3) == 1)          # cached and not diffuse_only: the whole sample went to the cache cell


def judge_writer(case, wrong=None, only=None):
    """n sequential render() calls, straight from the list of samples: no log here"""
    frame, psf = case["frame"].copy(), case["psf"]
    per = {}
    for s in case["samples"]:
        if reaches_frame(s):
            t = (s[2], s[3], s[4], s[5], s[6]) + ((bool(s[8] & 1), bool(s[8] & 2)) if psf and s[3] != T.EMISSIVE else ())
            per.setdefault((s[0], s[1]), []).append(t)
    with np.errstate(all="ignore"):
        for slot in (range(W_SLOTS) if only is None else only):
            p = int(case["pixels"][slot])
            px = frame[:, p, :].copy()
            for k in range(W_PASSES):
                T.render_pass(px, W_BASE + k, per.get((k, slot), []), None, psf, 100.0, 100.0 if psf else None, wrong)
            frame[:, p, :] = px
    return frame


def records_of(case, samples, batch, fused_as_plain=False):
    rec = np.zeros((len(samples), 16), U32)
    for i, s in enumerate(samples):
        k, slot, b, kind, comp, a, bb, what, flags = s
        where = slot if batch else int(case["pixels"][slot])
        rec[i, 0] = where | (comp << 27); rec[i, 1] = k; rec[i, 2] = b; rec[i, 3] = 2 if (fused_as_plain and what == 3) else what
        rec[i, 4:7] = bits(a); rec[i, 7] = flags; rec[i, 8:11] = bits(bb)
    return rec


def writer_log_shape():
    cap = W_SLOTS * W_PASSES
    return dict(acc_stride=W_SLOTS, cap=cap, mask_words=1, n_bounces=W_BOUNCES)


def expected_log(case):
    """where the layout comment of fpt_device.h puts each sample: pidx = k * acc_stride + slot; emissive [bounce * cap + pidx]; nee[kind] [(bounce * cap + pidx) * 2 +
    {0, 1}]; bit 3 * bounce + {0, 1, 2} of word pidx * mask_words; everything else as it was"""
    sh = writer_log_shape(); cap = sh["cap"]
    log = empty_log(cap, 1, W_BOUNCES, False)
    for s in case["samples"]:
        if not reaches_frame(s):
            continue
        k, slot, b, kind, comp, a, bb, what, flags = s
        pidx = k * sh["acc_stride"] + slot
        if kind == T.EMISSIVE:
            log["emissive"][b * cap + pidx, :3] = a; bits(log["emissive"])[b * cap + pidx, 3] = comp
        else:
            cell = log["nee0" if kind == T.NEE_DIRECTIONAL else "nee1"]
            tag = comp | ((0x100 if flags & 1 else 0) | (0x200 if flags & 2 else 0) if what == 4 else 0)
            cell[(b * cap + pidx) * 2, :3] = a; bits(cell)[(b * cap + pidx) * 2, 3] = tag
            cell[(b * cap + pidx) * 2 + 1, :3] = bb; cell[(b * cap + pidx) * 2 + 1, 3] = 0
        log["mask"][pidx] |= U32(1 << (3 * b + kind))
    return log


def launches(case, of_pass=None):
    """the samples in the launches of a pass: bounce by bounce, emission, directional light, mesh light; a launch holds one sample per path at the most"""
    for b in range(W_BOUNCES):
        for kind in (T.EMISSIVE, T.NEE_DIRECTIONAL, T.NEE_MESH):
            group = [s for s in case["samples"] if s[2] == b and s[3] == kind and (of_pass is None or s[0] == of_pass)]
            if group:
                yield b, group


def device_one_pass(r, case):
    """bracket, adds, bracket, pass by pass"""
    frame, psf, px = case["frame"], case["psf"], case["pixels"]
    for k in range(W_PASSES):
        inst = W_BASE + k
        frame, _ = r.debug_frame("bracket", frame, pixels=px, kind=0, value=F32(inst) / F32(inst + 1))
        for b, group in launches(case, k):
            frame, _ = r.debug_frame("write", frame, records=records_of(case, group, False), base_instance=inst, n_passes=1, fused_bounce=b, firefly=100.0,
                                     acc_stride=W_PIXELS, cap=W_PIXELS, mask_words=1, n_bounces=W_BOUNCES)
        frame, _ = r.debug_frame("bracket", frame, pixels=px, kind=1, value=inst + 1)
        if psf:
            frame, _ = r.debug_frame("bracket", frame, pixels=px, kind=2, value=100.0)
    return frame


def device_batch_write(r, case, fused_as_plain=False):
    frame, log = case["frame"], empty_log(W_SLOTS * W_PASSES, 1, W_BOUNCES, False)
    log = {k: log[k] for k in ("emissive", "nee0", "nee1", "mask")}
    for b, group in launches(case):
        frame, log = r.debug_frame("write", frame, log, records=records_of(case, group, True, fused_as_plain), pixels=case["pixels"], base_instance=W_BASE, n_passes=W_PASSES,
                                   fused_bounce=b, firefly=100.0, **writer_log_shape())
    return frame, log


# ---- the cases --------------------------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def cases():
    c = {}
    for inst in (0, 1, 5, 4097):          # 4097: n * n = 16 785 409 lies past 2^24
        for wl in (False, True):
            c["bracket-%d%s" % (inst, "-list" if wl else "")] = bracket_case(inst, wl)
    for wl in (False, True):
        c["clamp%s" % ("-list" if wl else "")] = clamp_case(wl)
    for n_passes in (1, 3):
        for base in (0, 5):
            for wl in (False, True):
                c["merge-pt-%dx-from-%d%s" % (n_passes, base, "-list" if wl else "")] = merge_case(300 if not wl else 200, n_passes, base, 4, wl, frame_pixels=300)
    # two mask words: bits 0, 31, 32 and the last one on every path (PT: 36 bits of 12 bounces; PSFPT: 27 + 9 bits of 9 bounces, so 31, 32 and 35 are blends)
    c["merge-pt-two-words"] = merge_case(40, 2, 3, 12, forced_bits=(0, 31, 32, 35))
    c["merge-psfpt-two-words"] = merge_case(40, 2, 3, 9, psf=True, forced_bits=(0, 31, 32, 35), big=0.01)
    # a lane narrower than the planes' stride: two lanes of 750 over one frame and one log
    c["merge-pt-lanes"] = merge_case(1500, 2, 1, 4, with_list=True, frame_pixels=1600, lanes=((0, 750), (750, 750)), share=0.2)
    c["merge-psfpt"] = merge_case(300, 3, 1, 4, psf=True)
    c["merge-psfpt-list"] = merge_case(200, 3, 0, 4, with_list=True, psf=True, frame_pixels=300)
    c["writers-pt"] = writer_case(False)
    c["writers-psfpt"] = writer_case(True)
    return c


JUDGES = dict(merge=lambda case, wrong=None, only=None: judge_merge(case, wrong, only)[0:2], bracket=judge_bracket, writer=judge_writer)
CASE_NAMES = ("bracket-0", "bracket-0-list", "bracket-1", "bracket-1-list", "bracket-5", "bracket-5-list", "bracket-4097", "bracket-4097-list", "clamp", "clamp-list",
              "merge-pt-1x-from-0", "merge-pt-1x-from-0-list", "merge-pt-1x-from-5", "merge-pt-1x-from-5-list", "merge-pt-3x-from-0", "merge-pt-3x-from-0-list",
              "merge-pt-3x-from-5", "merge-pt-3x-from-5-list", "merge-pt-two-words", "merge-psfpt-two-words", "merge-pt-lanes", "merge-psfpt", "merge-psfpt-list",
              "writers-pt", "writers-psfpt")


def test_case_names():
    assert tuple(cases()) == CASE_NAMES


# ---- CPU: the judge is exact ------------------------------------------------------------------------------------------------------------------------------------------
def fraction_pass(px, instance, samples):
    """render() on one pixel in exact arithmetic (PT): px = 8 x 4 Fractions"""
    mc = lambda v: max(v[0], v[1], v[2])  # noqa: E731
    px[T.LUMINANCE] = [mc(px[T.DIRECT_C]), mc(px[T.DIFFUSE_C]), mc(px[T.SPECULAR_C]), mc(px[T.COMPOSITED_C])]
    scale, w = Fraction(instance, instance + 1), Fraction(1, instance + 1)
    for c in range(6):
        px[c] = [x * scale for x in px[c]]

    def add(c, variance, f):
        delta = [f[j] - px[c][j] for j in range(3)]
        for j in range(3):
            px[c][j] += f[j] * w
        if variance:
            px[c][3] += mc(delta) ** 2 * w
    for bounce, kind, comp, a, b in sorted(samples, key=lambda s: (s[0], s[1])):
        if kind == T.EMISSIVE:
            add(T.COMPOSITED_C, False, a)
            if bounce == 0:
                add(T.DIRECT_C, False, a)
            else:
                if comp & 3:
                    add(T.DIFFUSE_C, True, a)
                if comp & 12:
                    add(T.SPECULAR_C, True, a)
        else:
            add(T.COMPOSITED_C, False, [x + y for x, y in zip(a, b)])
            if bounce == 0 or comp & 3:
                add(T.DIFFUSE_C, True, a)
            if bounce == 0 or comp & 12:
                add(T.SPECULAR_C, True, b)
    n = instance + 1
    new = [mc(px[T.DIRECT_C]), mc(px[T.DIFFUSE_C]), mc(px[T.SPECULAR_C]), mc(px[T.COMPOSITED_C])]
    for j, c in enumerate((T.DIRECT_C, T.DIFFUSE_C, T.SPECULAR_C, T.COMPOSITED_C)):
        d = new[j] - px[T.LUMINANCE][j]
        px[c][3] += (n * d) * ((n - 1) * d) / (n * n)


def test_judge_is_exact_on_dyadic_inputs():
    """two passes from instance 0: the weights are 1 and 1/2, the samples multiples of 2^-8 below 1, so every float32 operation of the judge is exact and it must
    equal rational arithmetic -- no tolerance"""
    rng = np.random.default_rng(59)
    dy = lambda n: (rng.integers(0, 256, n) / 256.0).astype(F32)  # noqa: E731
    for _ in range(64):
        px = (rng.integers(0, 256, (8, 4)) / 256.0).astype(F32)
        fx = [[Fraction(float(x)) for x in row] for row in px]
        for inst in (0, 1):
            samples = []
            for b in range(3):
                for kind in (T.EMISSIVE, T.NEE_DIRECTIONAL, T.NEE_MESH):
                    if rng.random() < 0.5:
                        samples.append((b, kind, int(rng.integers(0, 16)), dy(3), dy(3)))
            rng.shuffle(samples)
            T.render_pass(px, inst, [s[:4] if s[1] == T.EMISSIVE else s for s in samples])
            fraction_pass(fx, inst, [(s[0], s[1], s[2], [Fraction(float(x)) for x in s[3]], [Fraction(float(x)) for x in s[4]]) for s in samples])
        assert [[Fraction(float(x)) for x in row] for row in px] == fx


def test_judge_by_hand():
    """one pixel, two passes from instance 1, done by hand: pass 1 has an emission at bounce 0, pass 2 a mesh-light sample at bounce 1 with only the glossy comp"""
    frame = np.full((8, 1, 4), 6.0, F32)
    log = empty_log(2, 1, 2, False)
    log["albedo_d"][:] = ((1, 1, 1, 1), (2, 2, 2, 2))
    log["emissive"][0] = (3, 3, 3, 0); log["mask"][0] = 1                                      # pass 0 (instance 1): bounce 0, emission 3
    log["nee1"][(1 * 2 + 1) * 2] = (1, 2, 4, U32(4).view(F32)); log["nee1"][(1 * 2 + 1) * 2 + 1] = (0.5, 0.5, 0.5, 0); log["mask"][1] = 1 << 5      # pass 1: bounce 1, mesh
    T.merge_replay(frame, log, 1, 1, 2, 1, 2, 1, 2)
    half, third, tt = F32(0.5), F32(1) / F32(3), F32(2) / F32(3)
    c1 = F32(6) * half + F32(3) * half                                                         # COMPOSITED and DIRECT after pass 1
    assert frame[T.COMPOSITED_C, 0, 0] == c1 * tt + F32(1.5) * third and frame[T.COMPOSITED_C, 0, 2] == c1 * tt + F32(4.5) * third
    assert frame[T.DIRECT_C, 0, 0] == c1 * tt and frame[T.DIFFUSE_C, 0, 0] == F32(3) * tt and frame[T.DIFFUSE_A, 0, 0] == (F32(3) + F32(1)) * tt + F32(2)
    # SPECULAR_C: 6 -> 3 -> 3 * 2/3, then w_g = .5 with weight 1/3; its .w: 6 -> 3 -> + 0 (variance of pass 1: no change of luminance beyond the rescale... d = 3 - 6)
    s1 = F32(3) * tt
    assert frame[T.SPECULAR_C, 0, 0] == s1 + half * third
    w1 = F32(3) + ((F32(2) * F32(-3)) * (F32(1) * F32(-3))) / F32(4)                             # pass 1: n = 2, d = 3 - 6
    ld = half - s1; d2 = (s1 + half * third) - F32(3)                                            # pass 2: add_in's delta, then n = 3, d against the luminance before the rescale
    assert frame[T.SPECULAR_C, 0, 3] == (w1 * tt + (ld * ld) * third) + ((F32(3) * d2) * (F32(2) * d2)) / F32(9)
    assert frame[T.LUMINANCE, 0, 2] == F32(3) and frame[T.FILTERED_C, 0, 0] == F32(6) and not log["mask"].any() and not log["albedo_d"].any()


def test_judge_agrees_with_oracle(olib, table, cornell):
    """The oracle exposes no hook on its adds, but with one-vertex paths the only sample a pixel can get is the emission of the light it sees: three passes of
    OraclePT on a 16 x 12 Cornell frame equal the judge's bracket around one emissive add per pixel that hit the light (the hit comes from the oracle's capture of
    the primary vertices; the light's emission is constant and it faces the camera).  The albedo channels, which the oracle's shading writes, stay out of it."""
    from oracle import binding as ob
    from fermat_amd import scene
    o = ob.OraclePT(cornell, 16, 12, ob.default_options(1), table, scene.DATA_DIR)
    frame = np.zeros((8, 16 * 12, 4), F32)
    ke = cornell.materials["emissive"][:, :3]
    lit = 0
    o.set_capture(0)
    for inst in range(3):
        o.render_pass(inst)
        cap = o.captured()
        assert len(cap) == 16 * 12
        for entry in cap:
            p = int(entry["pixel_info"]) & 0x7FFFFFF
            tri = int(entry["hit"]["triId"])
            e = ke[cornell.material_indices[tri]] if tri >= 0 else np.zeros(3, F32)
            px = frame[:, p, :].copy()
            T.render_pass(px, inst, [(0, T.EMISSIVE, 0, e)] if e.max() > 0 else [])
            frame[:, p, :] = px
            lit += int(e.max() > 0)
        for c in (T.DIFFUSE_C, T.SPECULAR_C, T.DIRECT_C, T.COMPOSITED_C, T.LUMINANCE, T.FILTERED_C):
            assert same_bits(frame[c], o.fb[c]), (inst, c)
    assert lit >= 6 and frame[T.DIRECT_C, :, 3].max() > 0


# ---- CPU: the cases discriminate --------------------------------------------------------------------------------------------------------------------------------------
def holds(case):
    """what a case contains, read off the case itself: the steps of a bracket, a merge's log and its blend cells, a writer's list of samples"""
    if case["kind"] == "bracket":
        return {what for what, _ in case["steps"]} - {"nudge", "rescale"}
    psf = case["psf"] if case["kind"] == "writer" else case["par"]["psf"]
    has = {"variance", "samples"}                                 # every pass of a merge or of a list of samples ends in update_variances
    if psf:
        has |= {"clamp", "psf samples"}                           # the PSFPT's pass ends in clamp_frame, and its light samples go through clamp_sample
    if case["kind"] == "merge":
        has |= {"log"} | ({"blends"} if case["log"]["blend"] is not None else set())
    return has


# what a case must hold for a mistake to be able to show on it; a mistake is left out of a case for no other reason, and test_cases_discriminate also asks that a
# mistake left out changes NOTHING there -- so a mistake cannot be dropped from a case on which it could have shown
NEEDS = dict(swapped_kinds="samples", composited_variance="samples", comp_ignored="samples", emission_to_diffuse="samples",          # the order and routing of the adds: no adds in a bracket
             mask_kept="log", stale_cell_read="log",          # the mask and the cells without a bit exist only in a log: a list of samples written pass by pass has neither
             blends_first="blends",                           # the path tracer's log has no blend cells, and the writers' probe writes none
             psf_wd_alone="psf samples", clamp_after_sum="psf samples",          # the path tracer's samples are not clamped and have no cache tags
             clamp_skips_w="clamp",                           # clamp_frame runs in a clamp bracket and at the end of a PSFPT pass only
             variance_n="variance")                           # a clamp bracket runs no update_variances


def shows_on(case):
    return {w for w in T.WRONG if NEEDS[w] in holds(case)}


def differs(a, b):
    if isinstance(a, tuple):
        return any(differs(x, y) for x, y in zip(a, b))
    if isinstance(a, dict):
        return any(a[k] is not None and differs(a[k], b[k]) for k in a)
    return not same_bits(a, b)


def test_every_mistake_shows_somewhere():
    assert set(NEEDS) == set(T.WRONG)
    assert set().union(*[shows_on(c) for c in cases().values()]) == set(T.WRONG)


@pytest.mark.parametrize("name", CASE_NAMES)
def test_cases_discriminate(name):
    """each deliberately wrong replay that can show on the case differs from the true one in at least one word -- looked for on the case's first entries, which is
    enough and keeps this quick -- and each of the others leaves every word as it was: the case holds nothing that the mistake touches"""
    case = cases()[name]
    judge = JUDGES[case["kind"]]
    only = range(40)
    true = judge(case, None, only)
    assert not differs(true, judge(case, None, only))
    can = shows_on(case)
    for wrong in T.WRONG:
        assert differs(true, judge(case, wrong, only)) == (wrong in can), wrong


# ---- CPU: the wrapper's own check --------------------------------------------------------------------------------------------------------------------------------------
class NoDevice:
    """Renderer.debug_frame with the library call and the upload replaced: what is left is the wrapper's own checking and packing of the arguments"""

    class L:
        calls = 0

        @classmethod
        def fpt_debug_frame(cls, *args):
            cls.calls += 1
            return 0

    dev, ctx = "cpu", None

    def __init__(self):
        import types
        import torch
        self.torch = types.SimpleNamespace(from_numpy=torch.from_numpy, cuda=types.SimpleNamespace(synchronize=lambda dev: None))

    def _check(self, rc):
        assert rc == 0

    def debug_frame(self, *args, **kw):
        import fermat_amd as fa
        return fa.Renderer.debug_frame(self, *args, **kw)


def test_wrapper_refuses_two_samples_for_one_pixel():
    """the frame adds are plain read-modify-write, so the wrapper refuses a launch that holds two samples for one pixel before anything reaches the device"""
    c = cases()["writers-pt"]
    with pytest.raises(AssertionError, match="at most one sample per pixel"):
        NoDevice().debug_frame("write", c["frame"], records=np.zeros((2, 16), U32), base_instance=0, n_passes=1, fused_bounce=0, firefly=100.0, acc_stride=W_PIXELS, cap=W_PIXELS,
                               mask_words=1, n_bounces=W_BOUNCES)
    assert NoDevice.L.calls == 0


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------------------------------------
def merge_written(r, case, log):
    sh = writer_log_shape()
    full = dict(log, albedo_d=np.zeros((sh["cap"], 4), F32), albedo_s=np.zeros((sh["cap"], 4), F32), blend=np.zeros((W_BOUNCES * sh["cap"] * 3, 4), F32) if case["psf"] else None)
    return r.debug_frame("merge", case["frame"], full, pixels=case["pixels"], n=W_SLOTS, p0=0, base_instance=W_BASE, n_passes=W_PASSES, psf=case["psf"], firefly=100.0,
                         clamp_max=100.0 if case["psf"] else 0.0, **sh)


@pytest.fixture(scope="module")
def device(table):
    import fermat_amd as fa
    from fermat_amd import scene
    r = fa.Renderer(scene.cornell_box("CornellBox-JP"), 8, 8, fa.default_options(4), table=table)
    yield r
    r.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", [n for n in CASE_NAMES if n.startswith(("bracket", "clamp"))])
def test_bracket_device(device, name):
    case = cases()[name]
    assert_bracket(device_bracket(device, case), judge_bracket(case), case)


@pytest.mark.gpu
@pytest.mark.parametrize("name", [n for n in CASE_NAMES if n.startswith("merge")])
def test_merge_device(device, name):
    case = cases()[name]
    assert_merged(device_merge(device, case), judge_merge(case), case)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ("writers-pt", "writers-psfpt"))
def test_writers_agree_with_merge_device(device, name):
    """the same samples through the one-pass route (bracket, adds, bracket, pass by pass) and through the log (write with three passes in flight, then the merge):
    the two frames equal each other and the judge; the log's cells and bits sit where the layout says; the FusedResolve route fills the cells the plain route fills"""
    case = cases()[name]
    want = judge_writer(case)
    one = device_one_pass(device, case)
    for c in range(8):
        assert same_bits(one[c], want[c]), "one pass at a time: channel %d differs on %d pixels" % (c, (bits(one[c]) != bits(want[c])).any(axis=1).sum())
    frame, log = device_batch_write(device, case)
    assert same_bits(frame, case["frame"])          # passes in flight: the writers leave the frame alone
    layout = expected_log(case)
    for k in ("emissive", "nee0", "nee1", "mask"):
        assert same_bits(log[k], layout[k]), k
    if not case["psf"]:
        _, plain = device_batch_write(device, case, fused_as_plain=True)
        for k in ("emissive", "nee0", "nee1", "mask"):
            assert same_bits(plain[k], log[k]), k
    merged, after = merge_written(device, case, log)
    for c in range(8):
        assert same_bits(merged[c], want[c]), "passes in flight: channel %d differs on %d pixels" % (c, (bits(merged[c]) != bits(want[c])).any(axis=1).sum())
    assert same_bits(merged, one) and not after["mask"].any() and np.isfinite(merged).all()
