"""A numpy judge of chains that persist across render calls (fpt_mlt_set_persistence: `reseeding`, `startup_skips`) for the two Metropolis renderers.  It imports
tests/mlt_truth.py, tests/mmlt_truth.py and tests/mmlt_lens_truth.py for what is unchanged -- hashes, mutation numbers, the acceptance arithmetic with its deposits, the
swap walks, the resolve -- and neither the library nor the oracle.

What this file states on its own:
  * which call reseeds: one that finds no live chains, or whose instance is a multiple of R;
  * a CONTINUING call starts from the state the previous call left (coordinates, value, pdf, rejections; `-mmlt`: technique; lens: pixel), and its step 0 is a real
    mutation whose type is the later steps' rule at step 0: randfloat(0, hash32(instance + 0x9e3779b9)) < independent_samples ? Independent : Cauchy;
  * swap steps are l > 0 with l % F == 0 of the call's own step index;
  * the first K steps of a RESEEDING call run the acceptance test in full -- commit, rejection counters, counts -- and deposit nothing; a continuing call deposits
    every step;
  * pdf_norm = brightness * n_pixels / (steps that deposit * n_chains), the brightness being the period's (its reseed's).
One replay serves the three kinds of chain ('pssmlt', 'mmlt', 'lens'); every comparison and integer step is exact: bit for bit."""
import numpy as np

import mlt_truth as T
import mmlt_truth as M
import mmlt_lens_truth as J

F32 = np.float32
U32 = np.uint32
NONE = J.NONE
KINDS = ("pssmlt", "mmlt", "lens")
MISTAKES = (None, "null_step0", "pdf_zeroed", "rejections_zeroed", "global_swaps", "deposit_skipped")


def call_reseeds(instance, reseeding, live):
    return (not live) or instance % reseeding == 0


def flags(instances, reseeding):
    """last_call_reseeded of a sequence of calls whose chains stay live once started"""
    out = []; live = False
    for i in instances:
        out.append(int(call_reseeds(i, reseeding, live))); live = True
    return out


def mutation_type(independent_samples, instance, step, continuing):
    """tests/mlt_truth.py mutation_type for every step but step 0 of a continuing call, where the rule of the later steps applies to step 0"""
    if step == 0 and continuing:
        with np.errstate(over="ignore"):
            key = T.hash32(U32(instance) + U32(0x9e3779b9))
        return 2 if T.randfloat(U32(0), key) < F32(independent_samples) else 1
    return T.mutation_type(independent_samples, instance, step)


def clamp_skips(skips, chain_length):
    return min(int(skips), chain_length - 1) if chain_length else 0


def accumulated_steps(chain_length, skips, reseeds):
    return chain_length - clamp_skips(skips, chain_length) if reseeds else chain_length


def pdf_norm(brightness, n_pixels, chain_length, n_chains, skips, reseeds):
    return T.pdf_norm(brightness, n_pixels, accumulated_steps(chain_length, skips, reseeds), n_chains)


def fresh_state(kind, light_u, eye_u, st=None):
    """the chains of a reseeding call before step 0: the recovered coordinates, no value, no pdf, no rejections (lens: no pixel)"""
    s = T.new_state(light_u, eye_u)
    return _with_counters(kind, s, st, None)


def left_state(kind, d):
    """the chains as a render call left them, from its download `d` (light_u, eye_u, path_value, path_pdf, rejections; st; path_pixel)"""
    s = dict(light_u=np.array(d["light_u"], F32), eye_u=np.array(d["eye_u"], F32), path_value=np.array(d["path_value"], F32), path_pdf=np.array(d["path_pdf"], F32),
             rejections=np.array(d["rejections"], U32), accepted=0, rejected=0)
    return _with_counters(kind, s, d.get("st"), d.get("path_pixel"))


def _with_counters(kind, s, st, pixel):
    assert kind in KINDS
    n = s["light_u"].shape[1]
    s["swaps_proposed"] = s["swaps_accepted"] = s["rays"] = s["accepted_at_step0"] = 0
    if kind != "pssmlt":
        s["st"] = np.array(st, U32)
    if kind == "lens":
        s["path_pixel"] = np.full(n, NONE, U32) if pixel is None else np.array(pixel, U32)
    return s


def replay_call(kind, st, L, n_steps, instance, opts, F, norm, res, frame, perturb, evaluate, continuing, skips=0, mistake=None, first_step_of_period=0):
    """One render call's chain steps on the host, from chain state `st` (fresh_state for a reseeding call, left_state for a continuing one), which is advanced in place.
    opts: dict(independent_samples, light_perturbations, eye_perturbations); F the swap frequency ('pssmlt': ignored); norm the call's pdf_norm;
    perturb(u (dims, n), dim offset, mutation, instance, step) -> proposed coordinates; evaluate(light, eye, st words or None) -> ((n, 4) values, rays queued, (n,) lens
    pixels or None).  `skips`: startup_skips as clamped, which a continuing call ignores.
    mistake: 'null_step0' (step 0 of a continuing call proposes the state itself), 'pdf_zeroed' / 'rejections_zeroed' (a continuing call forgets them),
    'global_swaps' (the swap schedule on the period's step index first_step_of_period + l), 'deposit_skipped' (skipped steps deposit).  Returns (st, frame)."""
    assert kind in KINDS and mistake in MISTAKES
    n = st["light_u"].shape[1]; dims = (L + 1) * 3
    if continuing and mistake == "pdf_zeroed":
        st["path_pdf"][:] = 0
    if continuing and mistake == "rejections_zeroed":
        st["rejections"][:] = 0
    splat = np.zeros((res[0] * res[1], 3), np.int64)
    chains = np.arange(n, dtype=U32)
    proposal = J.swap_proposal if kind == "lens" else M.swap_proposal
    for step in range(n_steps):
        swap = kind != "pssmlt" and M.is_swap_step(F, step + (first_step_of_period if mistake == "global_swaps" else 0))
        mut = 0 if swap else mutation_type(opts["independent_samples"], instance, step, continuing and mistake != "null_step0")
        nl = perturb(st["light_u"], 0, mut, instance, step) if (mut and opts["light_perturbations"]) else st["light_u"].copy()
        ne = perturb(st["eye_u"], dims, mut, instance, step) if (mut and opts["eye_perturbations"]) else st["eye_u"].copy()
        st_eval = None
        if kind != "pssmlt":
            st_eval = proposal(st["st"], T.mutation_number(instance, step, chains, U32(M.swap_dim(L)))) if swap else st["st"]
        w, rays, lens_pixel = evaluate(nl, ne, st_eval)
        st["rays"] += rays
        u_ar = T.mutation_number(instance, step, chains, U32(dims * 2))
        deposits = continuing or step >= skips or mistake == "deposit_skipped"
        sums = splat if deposits else np.zeros_like(splat)          # a skipped step: the test in full, its deposits thrown away
        if kind == "lens":
            acc = J.accept_reject(st, w, nl, ne, lens_pixel, u_ar, norm, instance, res, sums)
        else:
            acc = T.accept_reject(st, w, nl, ne, u_ar, norm, instance, res, sums)
        if step == 0:
            st["accepted_at_step0"] = int(acc.sum())
        if swap:
            st["st"][acc] = st_eval[acc]
            st["swaps_proposed"] += n; st["swaps_accepted"] += int(acc.sum())
    return st, T.resolve(frame, splat)


def self_check():
    """the judge on hand-made chains: a continuing step 0 mutates where a reseeding one does not; a skipped step deposits nothing but commits"""
    assert flags(range(7), 3) == [1, 0, 0, 1, 0, 0, 1] and flags(range(4), 1) == [1, 1, 1, 1] and flags([5, 6, 7, 8, 9], 8) == [1, 0, 0, 1, 0]
    assert call_reseeds(5, 8, False) and not call_reseeds(5, 8, True) and call_reseeds(16, 8, True)
    for inst in range(32):
        assert mutation_type(0.25, inst, 0, False) == 0 == T.mutation_type(0.25, inst, 0) and mutation_type(0.25, inst, 0, True) in (1, 2)
        assert all(mutation_type(0.25, inst, k, True) == T.mutation_type(0.25, inst, k) == mutation_type(0.25, inst, k, False) for k in range(1, 20))
    assert mutation_type(0.0, 3, 0, True) == 1 and mutation_type(1.0, 3, 0, True) == 2
    assert {mutation_type(0.5, i, 0, True) for i in range(64)} == {1, 2}
    assert clamp_skips(100, 16) == 15 and clamp_skips(2, 16) == 2 and accumulated_steps(16, 2, True) == 14 and accumulated_steps(16, 2, False) == 16
    assert pdf_norm(2.0, 1024, 16, 256, 8, True) == F32(1.0) and pdf_norm(2.0, 1024, 16, 256, 8, False) == F32(0.5) == T.pdf_norm(2.0, 1024, 16, 256)
    h = T.hand_made_chains()
    L = h["L"]; res = h["res"]; n = h["light_u"].shape[1]
    opts = dict(independent_samples=0.0, light_perturbations=1, eye_perturbations=1)
    seen = []

    def perturb(u, offset, mutation, instance, step):
        seen.append((step, mutation))
        return ((u + F32(0.25)) % F32(1.0)).astype(F32)

    def evaluate(a, b, st):
        v = np.zeros((n, 4), F32); v[:, 0] = a[0] + F32(0.125); v[:, 1] = b[3]; v[:, 3] = 1
        return v, 0, None
    left = dict(light_u=h["light_u"], eye_u=h["eye_u"], path_value=h["path_value"], path_pdf=h["path_pdf"], rejections=np.arange(n, dtype=U32))
    # (a) a continuing call: step 0 proposes mutated coordinates, some chains accept them and move, some reject and count one more rejection
    st, frame = replay_call("pssmlt", left_state("pssmlt", left), L, 1, 3, opts, 0, F32(1.0), res, np.zeros((res[0] * res[1], 4), F32), perturb, evaluate, True)
    assert seen == [(0, 1), (0, 1)] and 0 < st["accepted_at_step0"] < n and st["accepted"] + st["rejected"] == n
    moved = (st["light_u"] != h["light_u"]).any(0)
    assert moved.sum() == st["accepted"] and (st["rejections"][moved] == 0).all() and (st["rejections"][~moved] == np.arange(n)[~moved] + 1).all()
    assert frame[:, :3].sum() > 0
    # the planted step-0 Null proposes the state itself
    del seen[:]
    replay_call("pssmlt", left_state("pssmlt", left), L, 1, 3, opts, 0, F32(1.0), res, np.zeros((res[0] * res[1], 4), F32), perturb, evaluate, True, mistake="null_step0")
    assert seen == []
    # (b) a reseeding call: step 0 is Null; with one skipped step it commits every chain (their pdf was 0) and deposits nothing
    fresh = fresh_state("pssmlt", h["light_u"], h["eye_u"])
    st, frame = replay_call("pssmlt", fresh, L, 1, 0, opts, 0, F32(1.0), res, np.zeros((res[0] * res[1], 4), F32), perturb, evaluate, False, skips=1)
    assert seen == [] and st["accepted"] == n and (st["path_pdf"] > 0).all() and not frame.any()
    st2, frame2 = replay_call("pssmlt", fresh_state("pssmlt", h["light_u"], h["eye_u"]), L, 1, 0, opts, 0, F32(1.0), res, np.zeros((res[0] * res[1], 4), F32), perturb, evaluate, False)
    assert frame2[:, :3].sum() > 0 and all(np.array_equal(st[k], st2[k]) for k in ("light_u", "eye_u", "path_value", "path_pdf", "rejections"))
    st3, frame3 = replay_call("pssmlt", fresh_state("pssmlt", h["light_u"], h["eye_u"]), L, 1, 0, opts, 0, F32(1.0), res, np.zeros((res[0] * res[1], 4), F32), perturb, evaluate, False,
                              skips=1, mistake="deposit_skipped")
    assert np.array_equal(frame3, frame2)
    # a continuing call ignores the skips
    a = replay_call("pssmlt", left_state("pssmlt", left), L, 2, 3, opts, 0, F32(1.0), res, np.zeros((res[0] * res[1], 4), F32), perturb, evaluate, True, skips=1)[1]
    b = replay_call("pssmlt", left_state("pssmlt", left), L, 2, 3, opts, 0, F32(1.0), res, np.zeros((res[0] * res[1], 4), F32), perturb, evaluate, True, skips=0)[1]
    assert np.array_equal(a, b) and a.any()
    # the swap schedule: per call, l > 0; the planted period-global index swaps at step 0 of the second call of 16 steps
    lens_left = dict(left, st=np.full(n, M.word(1, 2), U32), path_pixel=np.full(n, NONE, U32))
    for kind in ("mmlt", "lens"):
        def ev(a_, b_, w):
            v, _, _ = evaluate(a_, b_, w)
            return v, n, np.full(n, NONE, U32) if kind == "lens" else None
        good = replay_call(kind, left_state(kind, lens_left), L, 1, 1, opts, 2, F32(1.0), res, np.zeros((res[0] * res[1], 4), F32), perturb, ev, True, first_step_of_period=16)[0]
        bad = replay_call(kind, left_state(kind, lens_left), L, 1, 1, opts, 2, F32(1.0), res, np.zeros((res[0] * res[1], 4), F32), perturb, ev, True, mistake="global_swaps",
                          first_step_of_period=16)[0]
        assert good["swaps_proposed"] == 0 and bad["swaps_proposed"] == n and good["rays"] == n
