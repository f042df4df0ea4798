"""A numpy judge of what the multiplexed Metropolis renderer (`-mmlt`: one (s, t) technique per chain) adds to the PSSMLT kernels.  It imports tests/mlt_truth.py
(hashes, mutation numbers, the integer CDF, the seeds, the acceptance arithmetic, the resolve) and neither the library nor the oracle.

A technique is (s light vertices, t eye vertices).  With light tracing off: t in [2, L + 1], s in [0, L + 1 - t].  The table's order is stated here by ENUMERATION
(all techniques of t = 2 with s rising, then t = 3, ...), not by the library's closed form, so that the two can disagree.  A chain keeps its technique as the word
s | t << 8.

The swap walk (mmlt_swap_kernel, src/renderers/cmlt.cu:496-544): with k = s + t - 1, the states are s in [0, k - 1]; u > 1/2 proposes s + 1 and wraps to 0 from
t = 2, otherwise s - 1 and wraps to s + t - 2 from s = 0; t_new = s + t - s_new.  Every comparison and integer step is exact: bit for bit."""
import numpy as np

import mlt_truth as T

F32 = np.float32
U32 = np.uint32


def techniques(L):
    """[(s, t)] in table order"""
    return [(s, t) for t in range(2, L + 2) for s in range(0, L + 2 - t)]


def tech_count(L):
    return len(techniques(L))


def tech_index(s, t, L):
    return techniques(L).index((int(s), int(t)))


def word(s, t):
    return U32(int(s) | (int(t) << 8))


def words(L):
    return np.array([word(s, t) for s, t in techniques(L)], U32)


def unword(w):
    w = np.asarray(w, U32)
    return (w & U32(0xFF)).astype(np.int64), (w >> U32(8)).astype(np.int64)


def tech_indices(st, L):
    """table index of every word of `st`"""
    lut = {int(w): i for i, w in enumerate(words(L))}
    return np.array([lut[int(w)] for w in np.asarray(st, U32)], np.int64)


def max_rays(st):
    """the most rays one proposal of each technique may queue: max(s - 1, 0) + (t - 1) + [s > 0]"""
    s, t = unword(st)
    return np.maximum(s - 1, 0) + (t - 1) + (s > 0)


def swap_dim(L):
    return (L + 1) * 6 + 1


def swap_proposal(st, u, mistake=None):
    """the proposed words; mistake 'clamp': a walk that stops at its ends instead of wrapping"""
    s, t = unword(st)
    up = np.asarray(u, F32) > F32(0.5)
    if mistake == "clamp":
        s_new = np.where(up, np.where(t > 2, s + 1, s), np.where(s > 0, s - 1, s))
    else:
        s_new = np.where(up, np.where(t > 2, s + 1, 0), np.where(s > 0, s - 1, s + t - 2))
    t_new = s + t - s_new
    return (s_new | (t_new << 8)).astype(U32)


def swap_matrix(k):
    """transition matrix of the walk on the k techniques of path length k (s = 0 .. k - 1), each direction with probability 1/2"""
    P = np.zeros((k, k))
    for s in range(k):
        t = k + 1 - s
        for u in (F32(0.75), F32(0.25)):
            s_new, t_new = unword(swap_proposal(np.array([word(s, t)]), np.array([u])))
            assert s_new[0] + t_new[0] == s + t and t_new[0] >= 2 and 0 <= s_new[0] < k
            P[s, s_new[0]] += 0.5
    return P


def is_swap_step(F, step):
    return F != 0 and step != 0 and step % F == 0


def st_norms(table, L):
    """(q, cdf, norms[(L+2), (L+2)] indexed [t, s], brightness) of a technique table (n_tech, n_pixels, 4): the integer CDF over all cells"""
    n_tech, n_pixels = table.shape[:2]
    q, cdf, _ = T.seed_cdf(table.reshape(-1, 4))
    ends = [int(cdf[(k + 1) * n_pixels - 1]) for k in range(n_tech)]
    norms = np.zeros((L + 2, L + 2), F32)
    for k, (s, t) in enumerate(techniques(L)):
        norms[t, s] = F32(np.float64(ends[k] - (ends[k - 1] if k else 0)) * (1.0 / 4294967296.0) / np.float64(n_pixels))
    return q, cdf, norms, F32(np.float64(ends[-1]) * (1.0 / 4294967296.0) / np.float64(n_pixels))


def seed_offset(instance):
    """the offset common to all strata of render call `instance`, in units of 2^-24: floor(randfloat(instance, hash32(0x5eed5eed)) * 2^24)"""
    u = T.randfloat(U32(instance), T.hash32(U32(0x5eed5eed)))
    return int(F32(u) * F32(16777216.0)) & 0xFFFFFF


def sample_seeds(cdf, n_seeds, instance):
    """the multiplexed renderer's seeds, or None for a zero total: stratum i's target is floor(total * (i * 2^24 + m) / (n * 2^24)) in exact integers, m the common
    offset; the seed is the first cell whose CDF exceeds it.  With ONE offset for all strata a block [A, B) of the CDF gets the strata with i + m 2^-24 in
    [n A / total, n B / total): within 1 (strictly) of n * its share"""
    import bisect
    ints = [int(c) for c in np.asarray(cdf, np.uint64)]
    total = ints[-1]
    if total == 0:
        return None
    m = seed_offset(instance)
    last = bisect.bisect_left(ints, total)
    return np.array([min(bisect.bisect_right(ints, total * ((i << 24) | m) // (n_seeds << 24)), last) for i in range(n_seeds)], U32)


def sink_order_sum(table, L):
    """per eye path, the cells added from zero in the order the value sink meets them: bounce-major (t rising), the emission (s = 0), then the connections in light-depth
    order (s rising) -- the table's own order.  float32 additions, all four components"""
    out = np.zeros(table.shape[1:], F32)
    for k in range(table.shape[0]):
        out = (out + table[k]).astype(F32)
    return out


def replay(light_u, eye_u, st0, L, n_steps, instance, opts, F, norm, res, frame, perturb, evaluate, norms=None, mistake=None):
    """One render call's chain steps on the host.  opts as mlt_truth.replay's; F the swap frequency; perturb(u, dim offset, mutation, step) -> proposed coordinates;
    evaluate(light, eye, st) -> ((n, 4) values, rays queued).  mistake: None, 'norm_ratio' (the swap's test multiplied by st_norms[new] / st_norms[old], the reference's
    rule, `norms` indexed [t, s]), 'clamp' (the walk stops at its ends), 'commit' (the proposed technique kept on rejection too).  Returns (state, frame)."""
    st = T.new_state(light_u, eye_u)
    st["st"] = np.array(st0, U32)
    st["swaps_proposed"] = st["swaps_accepted"] = st["rays"] = 0
    n = st["light_u"].shape[1]; dims = (L + 1) * 3
    splat = np.zeros((res[0] * res[1], 3), np.int64)
    chains = np.arange(n, dtype=U32)
    for step in range(n_steps):
        swap = is_swap_step(F, step)
        mut = 0 if swap else T.mutation_type(opts["independent_samples"], instance, step)
        nl = perturb(st["light_u"], 0, mut, step) if (mut and opts["light_perturbations"]) else st["light_u"].copy()
        ne = perturb(st["eye_u"], dims, mut, step) if (mut and opts["eye_perturbations"]) else st["eye_u"].copy()
        st_eval = swap_proposal(st["st"], T.mutation_number(instance, step, chains, U32(swap_dim(L))), "clamp" if mistake == "clamp" else None) if swap else st["st"]
        w, rays = evaluate(nl, ne, st_eval)
        st["rays"] += rays
        u_ar = T.mutation_number(instance, step, chains, U32(dims * 2))
        if swap and mistake == "norm_ratio":
            so, to = unword(st["st"]); sn, tn = unword(st_eval)
            with np.errstate(all="ignore"):
                u_ar = (u_ar / (norms[tn, sn] / norms[to, so]).astype(F32)).astype(F32)
        acc = T.accept_reject(st, w, nl, ne, u_ar, norm, instance, res, splat)
        if swap:
            keep = np.ones(n, bool) if mistake == "commit" else acc
            st["st"][keep] = st_eval[keep]
            st["swaps_proposed"] += n; st["swaps_accepted"] += int(acc.sum())
    return st, T.resolve(frame, splat)


def self_check():
    """the judge on its own: the index is a bijection onto L (L + 1) / 2, the walk is symmetric and keeps s + t"""
    for L in range(1, 16):
        ts = techniques(L)
        assert len(ts) == L * (L + 1) // 2 == tech_count(L) and len(set(ts)) == len(ts)
        assert sorted(tech_index(s, t, L) for s, t in ts) == list(range(len(ts)))
        assert all(2 <= t <= L + 1 and 0 <= s <= L + 1 - t for s, t in ts)
        w = words(L); s, t = unword(w)
        assert [(int(a), int(b)) for a, b in zip(s, t)] == ts and list(tech_indices(w, L)) == list(range(len(ts)))
        for k in range(1, L + 1):
            P = swap_matrix(k)
            assert np.array_equal(P, P.T) and np.allclose(P.sum(1), 1.0)
    assert swap_matrix(1)[0, 0] == 1.0                       # k = 1: the chain's own technique
    assert int(swap_proposal([word(0, 2)], [F32(0.9)])[0]) == int(word(0, 2)) and int(swap_proposal([word(0, 4)], [F32(0.1)])[0]) == int(word(2, 2))
    assert int(swap_proposal([word(2, 2)], [F32(0.9)])[0]) == int(word(0, 4)) and int(swap_proposal([word(1, 3)], [F32(0.5)])[0]) == int(word(0, 4))
    assert int(swap_proposal([word(2, 2)], [F32(0.9)], "clamp")[0]) == int(word(2, 2))
    assert list(max_rays([word(0, 2), word(1, 2), word(3, 4)])) == [1, 2, 6]
    assert not is_swap_step(0, 4) and not is_swap_step(2, 0) and is_swap_step(2, 4) and not is_swap_step(2, 3)
    # st_norms of a hand-made table: two techniques (L = 2 has three), exact
    tb = np.zeros((3, 4, 4), F32); tb[0, 1, :3] = 0.5; tb[2, 3, :3] = (0.25, 0.125, 0)
    q, cdf, norms, b = st_norms(tb, 2)
    assert norms[2, 0] == F32(0.125) and norms[2, 1] == 0 and norms[3, 0] == F32(0.0625) and b == F32(0.1875)
    assert np.array_equal(sink_order_sum(tb, 2)[1], F32([0.5, 0.5, 0.5, 0]))
    # the seeds: every offset puts within 1 of n * share into every block of a hand-made CDF, and a cell worth nothing is never drawn
    cdf = np.cumsum(np.array([0, 5, 0, 1, 1, 90, 0, 3, 0], np.uint64))
    for n in (1, 7, 200):
        for inst in range(6):
            s = sample_seeds(cdf, n, inst)
            assert 0 <= seed_offset(inst) < (1 << 24) and not set(int(x) for x in s) & {0, 2, 6, 8} and (np.diff(s.astype(np.int64)) >= 0).all()
            for lo, hi in ((0, 3), (3, 5), (5, 9), (1, 2), (5, 6)):
                share = (int(cdf[hi - 1]) - (int(cdf[lo - 1]) if lo else 0)) / 100.0
                assert abs(int(((s >= lo) & (s < hi)).sum()) - n * share) < 1.0
    assert sample_seeds(np.zeros(4, np.uint64), 3, 0) is None
