"""A numpy judge of what the lens techniques (lens_techniques = 1: the connections (s, 1), s in [2, L], of a light sub-path straight to the lens) add to the multiplexed
Metropolis renderer.  It imports tests/mmlt_truth.py and tests/mlt_truth.py for what is unchanged and neither the library nor the oracle.

The table's order is stated here by ENUMERATION: the t >= 2 techniques in tests/mmlt_truth.py's order, then (2, 1), (3, 1), ..., (L, 1).  (1, 1) is not a technique: a
light vertex of depth 0 never splats.

The swap walk with the lens techniques: with k = s + t - 1 >= 2 the states are s in [0, k], s = k being (k, 1); u > 1/2 proposes s + 1 and wraps to 0 from t = 1,
otherwise s - 1 and wraps to k from s = 0; t_new = k + 1 - s_new.  k = 1 proposes the chain's own technique.

A chain's pixel: 0xFFFFFFFF (NONE) means "quantize eye coordinates 3 and 4"; a t = 1 state carries the pixel its lens connection landed on.  The pixel is committed
with the value on acceptance and kept on rejection.  Every comparison and integer step is exact: bit for bit."""
import numpy as np

import mlt_truth as T
import mmlt_truth as M

F32 = np.float32
U32 = np.uint32
NONE = U32(0xFFFFFFFF)

word = M.word
unword = M.unword
max_rays = M.max_rays          # max(s - 1, 0) + (t - 1) + [s > 0]: s for (s, 1)
swap_dim = M.swap_dim
is_swap_step = M.is_swap_step
sample_seeds = M.sample_seeds


def techniques(L):
    """[(s, t)] in table order: the t >= 2 block unchanged, then the lens block with s rising"""
    return M.techniques(L) + [(s, 1) for s in range(2, L + 1)]


def tech_count(L):
    return len(techniques(L))


def tech_index(s, t, L):
    return techniques(L).index((int(s), int(t)))


def words(L):
    return np.array([word(s, t) for s, t in techniques(L)], U32)


def tech_indices(st, L):
    lut = {int(w): i for i, w in enumerate(words(L))}
    return np.array([lut[int(w)] for w in np.asarray(st, U32)], np.int64)


def swap_proposal(st, u, mistake=None):
    """the proposed words.  mistakes: 'no_stop' -- the ring without the t = 1 stop (the t >= 2 walk of tests/mmlt_truth.py; a chain on t = 1 steps as on the ring);
    'with_11' -- the ring with (1, 1) on it: path length 1 walks between (0, 2) and (1, 1) instead of proposing its own technique"""
    s, t = unword(st)
    k = s + t - 1
    up = np.asarray(u, F32) > F32(0.5)
    s_ring = np.where(up, np.where(t > 1, s + 1, 0), np.where(s > 0, s - 1, k))
    if mistake == "no_stop":
        s_old = np.where(up, np.where(t > 2, s + 1, 0), np.where(s > 0, s - 1, s + t - 2))
        s_ring = np.where(t >= 2, s_old, s_ring)
    s_new = s_ring if mistake == "with_11" else np.where(k < 2, s, s_ring)
    t_new = k + 1 - s_new
    return (s_new | (t_new << 8)).astype(U32)


def swap_matrix(k, L):
    """transition matrix of the walk on the techniques of path length k (s = 0 .. k, or s = 0 alone for k = 1), each direction with probability 1/2"""
    states = [(s, k + 1 - s) for s in range(0, k + 1) if (s, k + 1 - s) in techniques(L)]
    P = np.zeros((len(states), len(states)))
    for i, (s, t) in enumerate(states):
        for u in (F32(0.75), F32(0.25)):
            sn, tn = unword(swap_proposal(np.array([word(s, t)]), np.array([u])))
            assert sn[0] + tn[0] == s + t
            P[i, states.index((int(sn[0]), int(tn[0])))] += 0.5          # .index raises for a technique outside the table
    return states, P


def st_norms(table, L):
    """(q, cdf, norms[(L+2), (L+2)] indexed [t, s], brightness) of a technique table (n_tech, n_pixels, 4) with the lens block: the integer CDF over all cells"""
    n_tech, n_pixels = table.shape[:2]
    assert n_tech == tech_count(L)
    # a lens cell holds c and counts as c * light_weight per component, what it adds to the frame: the total over n_pixels is then the frame's mean
    scaled = np.array(table, F32)
    scaled[M.tech_count(L):, :, :3] = (scaled[M.tech_count(L):, :, :3] * (F32(1.0) / F32(n_pixels))).astype(F32)
    q, cdf, _ = T.seed_cdf(scaled.reshape(-1, 4))
    ends = [int(cdf[(k + 1) * n_pixels - 1]) for k in range(n_tech)]
    norms = np.zeros((L + 2, L + 2), F32)
    for k, (s, t) in enumerate(techniques(L)):
        norms[t, s] = F32(np.float64(ends[k] - (ends[k - 1] if k else 0)) * (1.0 / 4294967296.0) / np.float64(n_pixels))
    return q, cdf, norms, F32(np.float64(ends[-1]) * (1.0 / 4294967296.0) / np.float64(n_pixels))


def lens_splat_sums(cells, pixels, n_pixels, instance=0):
    """the BPT's light-tracing splat sums (n_pixels, 3) int64 from the lens block: cells (L - 1, n_pixels, 4) hold c, pixels (L - 1, n_pixels) where each lands.  The
    header's splat rule: w = float32(c * light_weight) per component, light_weight = float32(1 / n_pixels); the sum receives round-half-even(float32(w * frame_weight)
    * 2^32), frame_weight = float32(1 / (instance + 1)); an entry is added when some component of w is positive.  Returns (sums, number of entries added)"""
    lw = F32(1.0) / F32(n_pixels); fw = F32(1.0) / F32(instance + 1)
    c = np.asarray(cells, F32).reshape(-1, 4)[:, :3]; p = np.asarray(pixels, U32).reshape(-1)
    w = (c * lw).astype(F32)
    live = (w > 0).any(1)
    assert (p[live] < n_pixels).all()
    sums = np.zeros((n_pixels, 3), np.int64)
    q = T.splat_fixed((w * fw).astype(F32))
    for k in range(3):
        np.add.at(sums[:, k], p[live].astype(np.int64), q[live, k])
    return sums, int(live.sum())


def accept_reject(st, new_value, new_light, new_eye, new_lens, u_ar, norm, instance, res, splat, mistake=None):
    """tests/mlt_truth.py accept_reject with the chains' pixels: a state whose pixel is not NONE lands there.  mistakes: 'pixel_from_eye' (the pixel of every state taken
    from eye coordinates 3 and 4), 'pixel_commit' (the proposal's pixel kept on rejection too).
    A proposal that carries a pixel arrives as c, the light-tracing sample before the multiplication by light_weight = float32(1 / n_pixels) (the table's cell).  What it
    adds to a pixel of the frame is c * light_weight per component, the BPT's splat: that is the state's value in the test, in the deposit and in path_value"""
    rx, ry = res
    one = F32(1.0); norm = F32(norm); count = F32(instance + 1); lw = F32(1.0) / F32(rx * ry)
    w = np.array(new_value, F32); new_lens = np.asarray(new_lens, U32)
    with np.errstate(all="ignore"):
        w[new_lens != NONE, :3] = (w[new_lens != NONE, :3] * lw).astype(F32)
        new_pdf = T.max_comp(w); old_pdf = st["path_pdf"]
        old_pixel = T.quantize(st["eye_u"][3], rx) + T.quantize(st["eye_u"][4], ry) * rx
        new_pixel = T.quantize(new_eye[3], rx) + T.quantize(new_eye[4], ry) * rx
        if mistake != "pixel_from_eye":
            old_pixel = np.where(st["path_pixel"] != NONE, st["path_pixel"].astype(np.int64), old_pixel)
            new_pixel = np.where(new_lens != NONE, new_lens.astype(np.int64), new_pixel)
        ratio = (new_pdf / old_pdf).astype(F32)
        ar = np.where(old_pdf != 0, np.where(ratio < one, ratio, one), one).astype(F32)

        def add(sel, pixel, weight, value, pdf):
            for k in range(3):
                v = ((weight * (value[:, k] / pdf).astype(F32)).astype(F32) / count).astype(F32)
                q = T.splat_fixed(v)
                np.add.at(splat[:, k], pixel[sel], q[sel])
        add(old_pdf > 0, old_pixel, (norm * (one - ar).astype(F32)).astype(F32), st["path_value"], old_pdf)
        add(new_pdf > 0, new_pixel, (norm * ar).astype(F32), w, new_pdf)
        acc = (np.asarray(u_ar, F32) * old_pdf).astype(F32) < new_pdf
    st["path_value"][acc] = w[acc]; st["path_pdf"][acc] = new_pdf[acc]
    keep = np.ones(len(acc), bool) if mistake == "pixel_commit" else acc
    st["path_pixel"][keep] = new_lens[keep]
    st["light_u"][:, acc] = np.asarray(new_light, F32)[:, acc]; st["eye_u"][:, acc] = np.asarray(new_eye, F32)[:, acc]
    st["rejections"][acc] = 0; st["rejections"][~acc] += U32(1)
    st["accepted"] += int(acc.sum()); st["rejected"] += int((~acc).sum())
    return acc


def replay(light_u, eye_u, st0, L, n_steps, instance, opts, F, norm, res, frame, perturb, evaluate, norms=None, mistake=None):
    """One render call's chain steps on the host, lens techniques on.  As tests/mmlt_truth.py replay; evaluate(light, eye, st) -> ((n, 4) values, rays queued, (n,) pixels:
    where a t = 1 evaluation landed, NONE otherwise).  mistake: None, 'pixel_from_eye', 'pixel_commit', 'no_stop', 'with_11' (above), 'light_weight' (the value of a
    t = 1 evaluation times float32(1 / n_pixels), the BPT's splat instead of the cell), 'norm_ratio' (the swap's test multiplied by st_norms[new] / st_norms[old]; `norms`
    indexed [t, s]).  Returns (state, frame); the state also holds `into_lens` / `out_of_lens`, the accepted swaps into and out of t = 1."""
    st = T.new_state(light_u, eye_u)
    st["st"] = np.array(st0, U32)
    n = st["light_u"].shape[1]; dims = (L + 1) * 3
    st["path_pixel"] = np.full(n, NONE, U32)
    st["swaps_proposed"] = st["swaps_accepted"] = st["rays"] = st["into_lens"] = st["out_of_lens"] = 0
    splat = np.zeros((res[0] * res[1], 3), np.int64)
    chains = np.arange(n, dtype=U32)
    lw = F32(1.0) / F32(res[0] * res[1])
    for step in range(n_steps):
        swap = is_swap_step(F, step)
        mut = 0 if swap else T.mutation_type(opts["independent_samples"], instance, step)
        nl = perturb(st["light_u"], 0, mut, step) if (mut and opts["light_perturbations"]) else st["light_u"].copy()
        ne = perturb(st["eye_u"], dims, mut, step) if (mut and opts["eye_perturbations"]) else st["eye_u"].copy()
        st_eval = swap_proposal(st["st"], T.mutation_number(instance, step, chains, U32(swap_dim(L))), mistake if mistake in ("no_stop", "with_11") else None) if swap else st["st"]
        w, rays, lens_pixel = evaluate(nl, ne, st_eval)
        if mistake == "light_weight":
            t1 = unword(st_eval)[1] == 1
            w = np.array(w, F32); w[t1] = (w[t1] * lw).astype(F32)
        st["rays"] += rays
        u_ar = T.mutation_number(instance, step, chains, U32(dims * 2))
        if swap and mistake == "norm_ratio":
            so, to = unword(st["st"]); sn, tn = unword(st_eval)
            with np.errstate(all="ignore"):
                u_ar = (u_ar / (norms[tn, sn] / norms[to, so]).astype(F32)).astype(F32)
        acc = accept_reject(st, w, nl, ne, lens_pixel, u_ar, norm, instance, res, splat, mistake if mistake in ("pixel_from_eye", "pixel_commit") else None)
        if swap:
            t_old = unword(st["st"])[1]; t_new = unword(st_eval)[1]
            st["into_lens"] += int((acc & (t_old != 1) & (t_new == 1)).sum()); st["out_of_lens"] += int((acc & (t_old == 1) & (t_new != 1)).sum())
            st["st"][acc] = st_eval[acc]
            st["swaps_proposed"] += n; st["swaps_accepted"] += int(acc.sum())
    return st, T.resolve(frame, splat)


def self_check():
    """the judge on its own: the index is a bijection onto L (L + 1) / 2 + (L - 1) that leaves the t >= 2 indices alone, the walk is symmetric, keeps s + t, stays in
    the table and never visits (1, 1)"""
    for L in range(1, 16):
        ts = techniques(L)
        assert len(ts) == L * (L + 1) // 2 + (L - 1) == tech_count(L) and len(set(ts)) == len(ts) and (1, 1) not in ts
        assert ts[:M.tech_count(L)] == M.techniques(L) and ts[M.tech_count(L):] == [(s, 1) for s in range(2, L + 1)]
        assert sorted(tech_index(s, t, L) for s, t in ts) == list(range(len(ts)))
        assert all(tech_index(s, 1, L) == M.tech_count(L) + s - 2 for s in range(2, L + 1))
        w = words(L); s, t = unword(w)
        assert [(int(a), int(b)) for a, b in zip(s, t)] == ts and list(tech_indices(w, L)) == list(range(len(ts)))
        assert list(max_rays(w[M.tech_count(L):])) == list(range(2, L + 1))
        for k in range(1, L + 1):
            states, P = swap_matrix(k, L)
            assert len(states) == (1 if k == 1 else k + 1)
            assert np.array_equal(P, P.T) and np.allclose(P.sum(1), 1.0)
    assert swap_matrix(1, 4)[1][0, 0] == 1.0                       # k = 1: the chain's own technique
    assert int(swap_proposal([word(0, 3)], [F32(0.1)])[0]) == int(word(2, 1)) and int(swap_proposal([word(2, 1)], [F32(0.9)])[0]) == int(word(0, 3))
    assert int(swap_proposal([word(2, 1)], [F32(0.1)])[0]) == int(word(1, 2)) and int(swap_proposal([word(1, 2)], [F32(0.9)])[0]) == int(word(2, 1))
    assert int(swap_proposal([word(1, 2)], [F32(0.5)])[0]) == int(word(0, 3))
    # the planted walks differ from the true one where they should, and only there
    assert int(swap_proposal([word(0, 3)], [F32(0.1)], "no_stop")[0]) == int(word(1, 2)) and int(swap_proposal([word(1, 2)], [F32(0.9)], "no_stop")[0]) == int(word(0, 3))
    assert int(swap_proposal([word(0, 2)], [F32(0.9)], "with_11")[0]) == int(word(1, 1)) and int(swap_proposal([word(0, 2)], [F32(0.9)])[0]) == int(word(0, 2))
    assert int(swap_proposal([word(0, 3)], [F32(0.1)], "with_11")[0]) == int(word(2, 1))
    # the splat rule on a hand-made lens block: two samples on one pixel, one worth nothing
    cells = np.zeros((2, 4, 4), F32); pixels = np.full((2, 4), NONE, U32)
    cells[0, 1] = (1.0, 0.5, 0.0, 1.0); pixels[0, 1] = 3; cells[1, 2] = (0.25, 0.0, 0.0, 1.0); pixels[1, 2] = 3
    sums, n = lens_splat_sums(cells, pixels, 4)
    assert n == 2 and list(sums[3]) == [(1 << 30) + (1 << 28), 1 << 29, 0] and not sums[:3].any()
    # a chain's pixel: taken from the plane when there is one, committed on acceptance only
    st = T.new_state(np.zeros((9, 2), F32), np.full((9, 2), 0.5, F32)); st["path_pixel"] = np.array([NONE, 7], U32)
    st["path_value"][:] = 1.0; st["path_pdf"][:] = 1.0
    splat = np.zeros((16, 3), np.int64)
    # (both proposals carry a pixel: they count times light_weight = 1 / 16, i.e. as 2 and 0.5)
    acc = accept_reject(st, np.array([[32, 32, 32, 1], [8, 8, 8, 1]], F32), st["light_u"], st["eye_u"], np.array([5, 9], U32), np.array([0.9, 0.9], F32), 1.0, 0, (4, 4), splat)
    assert list(acc) == [True, False] and list(st["path_pixel"]) == [5, 7]
    assert splat[5, 0] == 1 << 32 and splat[7, 0] == 1 << 31 and splat[9, 0] == 1 << 31 and splat[10, 0] == 0
