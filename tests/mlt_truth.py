"""A numpy judge of the Metropolis kernels (fermat_amd/csrc/fpt_mlt.hip, the chain mode of fpt_bpt.hip).  It imports neither the library nor the oracle.

What is integer or one correctly rounded float32 operation per step is restated in exactly that arithmetic and must match the device bit for bit: the hashes and
the mutation numbers, the Null and the Independent mutation, the seed CDF (uint64) and its brightness, the seeds, the acceptance test with its splats (float32
operation order, 2^-32 fixed point, int64 sums) and the resolve.

THE CAUCHY MUTATION, the one step that is not: out = (u + radius * s / c) mod 1 with (s, c) = det_sincos(x), x = fl(pi32 * fl(m - 1/2)).  The judge forms x in
float32 as the device does (two correctly rounded operations: the same bits), then t = tan(x) in float64.  The device's s', c' lie within E = 2.5e-7 absolute of
sin x, cos x -- the bound tests/test_oracle.py::test_detmath_accuracy pins on [-0.8, 6.4].  x lies in [-pi/2 - 5e-8, pi/2); on its part below -0.8 the same
bound holds by symmetry: the reduction's quadrant is k = floor(x 2/pi + 1/2), which for -x is -k except at exact ties, the remainder r changes sign with x, and the
two polynomials are odd and even in r, so det_sincos(-x) = (-s, c) of det_sincos(x), whose argument the pinned range covers.  Propagation, U = 2^-24:
    |s'/c' - s/c| <= E (|s| + |c|) / (|c| (|c| - E))                    (no bound when |c| <= 2 E: any value of [0, 1) is then accepted)
    the division rounds once: U |t|;  the product with the radius once: U |radius t|;  the sum with u once: U |u + radius t|;
    floor is exact, and x - floor(x) rounds once more only for a negative x: U (the result is below 1)
    B = radius (dt + U |t|) + U |radius t| + U |u + radius t| + U
A check accepts 2 B (the margin tests/bpt_truth.py takes, for the second-order terms) as the CIRCULAR distance between the device's value and the float64 one;
the distance on the circle is at most 1/2, so a bound above it decides nothing, and what remains checked there is that the value lies in [0, 1)."""
import numpy as np

F32 = np.float32
U32 = np.uint32
U = 2.0 ** -24
E_SINCOS = 2.5e-7
PI32 = F32(np.pi)
SEED_CLAMP = F32(2147483648.0)
MARGIN = 2.0


def _u32(x):
    return np.asarray(x, np.uint64).astype(U32) if np.asarray(x).dtype != U32 else np.asarray(x)


def hash32(a):
    """contrib/cugar/basic/numbers.h hash, on uint32 arrays (wrapping)"""
    a = np.array(a, dtype=U32, copy=True)
    with np.errstate(over="ignore"):
        a = (a + U32(0x7ed55d16)) + (a << U32(12))
        a = (a ^ U32(0xc761c23c)) ^ (a >> U32(19))
        a = (a + U32(0x165667b1)) + (a << U32(5))
        a = (a + U32(0xd3a2646c)) ^ (a << U32(9))
        a = (a + U32(0xfd7046c5)) + (a << U32(3))
        a = (a ^ U32(0xb55a4f09)) ^ (a >> U32(16))
    return a


def randfloat(i, p):
    i = np.array(i, dtype=U32, copy=True); p = np.asarray(p, dtype=U32)
    with np.errstate(over="ignore"):
        i = i ^ p
        i = i ^ (i >> U32(17))
        i = i ^ (i >> U32(10)); i = i * U32(0xb36534e5)
        i = i ^ (i >> U32(12))
        i = i ^ (i >> U32(21)); i = i * U32(0x93fc4795)
        i = i ^ U32(0xdf6e307f)
        i = i ^ (i >> U32(17)); i = i * (U32(1) | (p >> U32(18)))
    return i.astype(F32) * (F32(1.0) / F32(4294967808.0))


def mutation_number(instance, step, chain, dim):
    """randfloat(chain, hash32(hash32(hash32(instance) + step) + dim))"""
    with np.errstate(over="ignore"):
        key = hash32(hash32(hash32(U32(instance)) + U32(step)) + np.asarray(dim, U32))
    return randfloat(np.asarray(chain, U32), key)


def mutation_type(independent_samples, instance, step):
    if step == 0:
        return 0
    with np.errstate(over="ignore"):
        key = hash32(U32(instance) + U32(0x9e3779b9))
    return 2 if randfloat(U32(step), key) < F32(independent_samples) else 1


def chain_length(spp, n_pixels, n_chains):
    return (spp * n_pixels) // n_chains


def pdf_norm(brightness, n_pixels, length, n_chains):
    return F32(F32(brightness) * F32(n_pixels)) / F32(length * n_chains)


def cauchy_reference(u, m, radius):
    """(float64 value in [0, 1), bound B) of the Cauchy mutation; see the module's docstring"""
    u = np.asarray(u, F32); m = np.asarray(m, F32); radius = F32(radius)
    x = (PI32 * (m - F32(0.5))).astype(F32).astype(np.float64)
    s, c = np.sin(x), np.cos(x)
    t = s / c
    r = float(radius)
    with np.errstate(divide="ignore", invalid="ignore"):
        dt = np.where(np.abs(c) > 2 * E_SINCOS, E_SINCOS * (np.abs(s) + np.abs(c)) / (np.abs(c) * (np.abs(c) - E_SINCOS)), np.inf)
    y = u.astype(np.float64) + r * t
    B = r * (dt + U * np.abs(t)) + U * np.abs(r * t) + U * np.abs(y) + U
    return y - np.floor(y), B


def circular_distance(a, b):
    d = np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)) % 1.0
    return np.minimum(d, 1.0 - d)


# ---- seeds ----------------------------------------------------------------------------------------------------------------------------------------------
def sel_max(a, b):
    return np.where(a > b, a, b)


def max_comp(v):
    """the project's max_comp: sel_max(x, sel_max(y, z)), a > b ? a : b"""
    v = np.asarray(v, F32)
    return sel_max(v[..., 0], sel_max(v[..., 1], v[..., 2])).astype(F32)


def seed_cdf(values):
    """(q, cdf) as uint64, brightness as float32, of (n, >= 3) float32 values"""
    m = max_comp(values)
    ok = np.isfinite(m) & (m > 0)
    q = np.zeros(len(m), np.uint64)
    q[ok] = (np.minimum(m[ok], SEED_CLAMP).astype(np.float64) * 4294967296.0).astype(np.uint64)
    with np.errstate(over="ignore"):
        cdf = np.cumsum(q, dtype=np.uint64)
    total = int(cdf[-1])
    return q, cdf, F32(np.float64(total) * (1.0 / 4294967296.0) / np.float64(len(m)))


def sample_seeds(cdf, n_seeds):
    """the seeds, or None for a zero total"""
    cdf = np.asarray(cdf, np.uint64); total = int(cdf[-1])
    if total == 0:
        return None
    i = np.arange(n_seeds, dtype=U32)
    r = (i.astype(F32) + randfloat(i, U32(0))) / F32(n_seeds)
    x = r.astype(np.float64) * np.float64(total)
    out = np.zeros(n_seeds, U32)
    last = int(np.searchsorted(cdf, np.uint64(total), side="left"))
    ints = [int(c) for c in cdf]
    import bisect
    for k in range(n_seeds):
        target = (1 << 64) - 1 if x[k] >= 18446744073709551616.0 else int(x[k])
        out[k] = min(bisect.bisect_right(ints, target), last)
    return out


# ---- accept / reject ----------------------------------------------------------------------------------------------------------------------------------------
def quantize(x, n):
    with np.errstate(invalid="ignore", over="ignore"):
        p = (np.asarray(x, F32) * F32(n)).astype(F32)
        v = np.where(np.isnan(p), 0.0, np.clip(np.trunc(p.astype(np.float64)), -2147483648.0, 2147483647.0)).astype(np.int64)
    return np.clip(v, 0, n - 1).astype(np.int64)


def splat_fixed(v):
    x = np.asarray(v, F32).astype(np.float64) * 4294967296.0
    out = np.zeros(x.shape, np.int64)
    big = x >= 9223372036854775808.0; small = x <= -9223372036854775808.0; nan = np.isnan(x)
    mid = ~(big | small | nan)
    out[mid] = np.rint(x[mid]).astype(np.int64)
    out[big] = np.iinfo(np.int64).max; out[small] = np.iinfo(np.int64).min
    return out


def new_state(light_u, eye_u):
    n = np.asarray(light_u).shape[1]
    return dict(light_u=np.array(light_u, F32), eye_u=np.array(eye_u, F32), path_value=np.zeros((n, 4), F32), path_pdf=np.zeros(n, F32), rejections=np.zeros(n, U32),
                accepted=0, rejected=0)


def accept_reject(st, new_value, new_light, new_eye, u_ar, norm, instance, res, splat, mistake=None):
    """accept_reject_accumulate (pssmlt.cu:153-222) in float32 operation order on every chain; `splat` (n_pixels, 3) int64 receives the sums.  mistake: None,
    'inequality' (the acceptance rule turned round) or 'pixels' (old and new pixel swapped)"""
    rx, ry = res
    one = F32(1.0); norm = F32(norm); count = F32(instance + 1)
    w = np.asarray(new_value, F32)
    with np.errstate(all="ignore"):
        new_pdf = max_comp(w); old_pdf = st["path_pdf"]
        old_pixel = quantize(st["eye_u"][3], rx) + quantize(st["eye_u"][4], ry) * rx
        new_pixel = quantize(new_eye[3], rx) + quantize(new_eye[4], ry) * rx
        if mistake == "pixels":
            old_pixel, new_pixel = new_pixel, old_pixel
        ratio = (new_pdf / old_pdf).astype(F32)
        ar = np.where(old_pdf != 0, np.where(ratio < one, ratio, one), one).astype(F32)

        def add(sel, pixel, weight, value, pdf):
            for k in range(3):
                v = ((weight * (value[:, k] / pdf).astype(F32)).astype(F32) / count).astype(F32)
                q = splat_fixed(v)
                np.add.at(splat[:, k], pixel[sel], q[sel])
        add(old_pdf > 0, old_pixel, (norm * (one - ar).astype(F32)).astype(F32), st["path_value"], old_pdf)
        add(new_pdf > 0, new_pixel, (norm * ar).astype(F32), w, new_pdf)
        lhs = (np.asarray(u_ar, F32) * old_pdf).astype(F32)
        acc = (lhs > new_pdf) if mistake == "inequality" else (lhs < new_pdf)
    st["path_value"][acc] = w[acc]; st["path_pdf"][acc] = new_pdf[acc]
    st["light_u"][:, acc] = np.asarray(new_light, F32)[:, acc]; st["eye_u"][:, acc] = np.asarray(new_eye, F32)[:, acc]
    st["rejections"][acc] = 0; st["rejections"][~acc] += U32(1)
    st["accepted"] += int(acc.sum()); st["rejected"] += int((~acc).sum())
    return acc


def resolve(composited, splat):
    """COMPOSITED_C.xyz += float32(double(sum) * 2^-32) where a pixel has a non-zero sum; the sums are cleared"""
    out = np.array(composited, F32)
    hit = (splat != 0).any(1)
    out[hit, :3] = (out[hit, :3] + (splat[hit].astype(np.float64) * (1.0 / 4294967296.0)).astype(F32)).astype(F32)
    splat[:] = 0
    return out


def replay(light_u, eye_u, L, n_steps, instance, opts, norm, res, frame, perturb, evaluate, mistake=None):
    """One render call's chain steps on the host.  opts: dict(independent_samples, light_perturbations, eye_perturbations).  perturb(u (dims, n), dim offset, mutation,
    step) -> the proposed coordinates (the probe's op 0); evaluate(light, eye) -> (n, 4) values.  mistake: as accept_reject's, or 'offset' (the eye side's mutation
    dims not offset by (L+1)*3).  Returns (state, frame)."""
    st = new_state(light_u, eye_u)
    n = st["light_u"].shape[1]; dims = (L + 1) * 3
    splat = np.zeros((res[0] * res[1], 3), np.int64)
    chains = np.arange(n, dtype=U32)
    for step in range(n_steps):
        mut = mutation_type(opts["independent_samples"], instance, step)
        nl = perturb(st["light_u"], 0, mut, step) if (mut and opts["light_perturbations"]) else st["light_u"].copy()
        ne = perturb(st["eye_u"], 0 if mistake == "offset" else dims, mut, step) if (mut and opts["eye_perturbations"]) else st["eye_u"].copy()
        w = evaluate(nl, ne)
        u_ar = mutation_number(instance, step, chains, U32(dims * 2))
        accept_reject(st, w, nl, ne, u_ar, norm, instance, res, splat, mistake if mistake in ("inequality", "pixels") else None)
    return st, resolve(frame, splat)


# ---- self-checks on hand-made inputs (tests/test_pssmlt.py runs them without a GPU) -------------------------------------------------------------------------
def hand_made_values():
    """1000 entries: zeros, a run of equal values, one of 1e9, one of 1e10 (above the 2^31 clamp), denormals, a NaN, an infinity, a negative one"""
    rng = np.random.default_rng(7)
    v = np.zeros((1000, 4), F32)
    v[100:400, :3] = rng.random((300, 3), dtype=F32)
    v[400:450, :3] = F32(0.375)
    v[500, :3] = (F32(1e9), 0, 0); v[501, :3] = (0, F32(1e10), 0)
    v[600:610, :3] = F32(1e-45); v[610:620, 2] = F32(3e-39)
    v[700, :3] = np.nan; v[701, :3] = (0, 0, np.inf); v[702, :3] = (-1, -2, -3)
    v[990:, :3] = 0
    return v


def hand_made_chains(L=2, res=(8, 4), pdf=1.0):
    """chains that meet every branch of the acceptance test (see tests/test_pssmlt.py test 4); returns dict of arrays and the expected labels"""
    dims = (L + 1) * 3
    n = 8 + 64
    rng = np.random.default_rng(11)
    lu = rng.random((dims, n), dtype=F32); eu = rng.random((dims, n), dtype=F32)
    nl = rng.random((dims, n), dtype=F32); ne = rng.random((dims, n), dtype=F32)
    old = np.zeros((n, 4), F32); new = np.zeros((n, 4), F32); old_pdf = np.zeros(n, F32)
    # 0: old_pdf = 0 -> accepts, no old splat
    new[0] = (0.5, 0.25, 0.125, 1)
    # 1: new_pdf = 0 -> rejects, the old pixel gets the full weight
    old[1] = (0.2, 0.7, 0.1, 1); old_pdf[1] = 0.7
    # 2: equal pdfs
    old[2] = (0.3, 0.6, 0.2, 1); old_pdf[2] = 0.6; new[2] = (0.6, 0.1, 0.2, 1)
    # 3: NaN new value -> rejects, splats nothing, state untouched
    old[3] = (0.4, 0.4, 0.9, 1); old_pdf[3] = 0.9; new[3] = (np.nan, np.nan, np.nan, np.nan)
    # 4, 5: u at 0 and at 1 - 2^-24: corner pixels, old and new
    old[4] = (1, 2, 3, 1); old_pdf[4] = 3; new[4] = (0.5, 1.5, 0.25, 1); eu[3:5, 4] = 0; ne[3:5, 4] = F32(1) - F32(2.0 ** -24)
    old[5] = (3, 2, 1, 1); old_pdf[5] = 3; new[5] = (4, 5, 6, 1); eu[3:5, 5] = F32(1) - F32(2.0 ** -24); ne[3:5, 5] = 0
    # 6, 7: a plain downhill and a plain uphill move
    old[6] = (2, 2, 2, 1); old_pdf[6] = 2; new[6] = (0.1, 0.3, 0.2, 1)
    old[7] = (0.1, 0.1, 0.1, 1); old_pdf[7] = 0.1; new[7] = (5, 1, 1, 1)
    # 8..71: 64 chains on one pixel, old and new
    old[8:] = rng.random((64, 4), dtype=F32) + F32(0.01); old_pdf[8:] = max_comp(old[8:]); new[8:] = rng.random((64, 4), dtype=F32) + F32(0.01)
    eu[3, 8:] = F32(0.3); eu[4, 8:] = F32(0.6); ne[3, 8:] = F32(0.3); ne[4, 8:] = F32(0.6)
    return dict(L=L, res=res, light_u=lu, eye_u=eu, new_light=nl, new_eye=ne, path_value=old, path_pdf=old_pdf, new_value=new)


def self_check():
    """the judge on hand-made inputs, against answers worked out by hand"""
    # hashes: fixed points of the definition
    assert int(hash32(U32(0))) == int(hash32(np.zeros(1, U32))[0])
    m = mutation_number(3, 5, np.arange(1000, dtype=U32), U32(7))
    assert m.dtype == F32 and (m >= 0).all() and (m < 1).all() and 0.4 < m.mean() < 0.6
    assert mutation_type(1.0, 0, 0) == 0 and mutation_type(1.0, 0, 3) == 2 and mutation_type(0.0, 9, 3) == 1
    # the CDF: integers, clamp, the values that count nothing
    v = np.zeros((6, 4), F32); v[1, :3] = (0.5, 0.25, 0); v[2, :3] = (0.5, 0.5, 0.5); v[3, :3] = np.nan; v[4, :3] = (0, 1e10, 0); v[5, :3] = (-1, -1, -1)
    q, cdf, b = seed_cdf(v)
    assert [int(x) for x in q] == [0, 1 << 31, 1 << 31, 0, 1 << 63, 0] and int(cdf[-1]) == (1 << 63) + (1 << 32)
    assert b == F32((2.0 ** 31 + 1.0) / 6.0)
    s = sample_seeds(cdf, 7)
    assert s is not None and set(int(x) for x in s) <= {1, 2, 4} and int(s[-1]) == 4
    assert sample_seeds(np.zeros(5, np.uint64), 3) is None
    # one entry: every seed is that entry, however the target rounds
    assert (sample_seeds(np.array([0, 0, 5, 5, 5], np.uint64), 300) == 2).all()
    # fixed point: half to even, saturation, NaN
    assert [int(x) for x in splat_fixed(F32([0.5, 2.0 ** -33, 3 * 2.0 ** -33, np.nan, 1e30, -1e30]))] == [1 << 31, 0, 2, 0, (1 << 63) - 1, -(1 << 63)]
    assert [int(x) for x in quantize(F32([0, 1 - 2.0 ** -24, -0.5, np.nan, 2.0]), 8)] == [0, 7, 0, 0, 7]
    # accept / reject on the hand-made chains
    h = hand_made_chains()
    st = new_state(h["light_u"], h["eye_u"]); st["path_value"][:] = h["path_value"]; st["path_pdf"][:] = h["path_pdf"]
    before = {k: np.array(x) for k, x in st.items() if isinstance(x, np.ndarray)}
    splat = np.zeros((h["res"][0] * h["res"][1], 3), np.int64)
    u_ar = np.full(len(h["path_pdf"]), F32(0.5))
    acc = accept_reject(st, h["new_value"], h["new_light"], h["new_eye"], u_ar, F32(1.0), 0, h["res"], splat)
    assert acc[0] and not acc[1] and acc[2] and not acc[3] and not acc[6] and acc[7]
    assert st["rejections"][1] == 1 and st["rejections"][3] == 1 and st["rejections"][0] == 0
    for k in ("light_u", "eye_u"):
        assert np.array_equal(st[k][:, 3], before[k][:, 3]) and np.array_equal(st[k][:, 0], h["new_" + k[:-2]][:, 0])
    assert np.array_equal(st["path_value"][3], before["path_value"][3]) and st["path_pdf"][3] == before["path_pdf"][3]
    # chain 1 alone on its pixel gives old / old_pdf in full; chain 3 gives nothing anywhere
    one = {k: (x[:, 1:2] if x.ndim == 2 and x.shape[0] == 9 else x[1:2]) for k, x in h.items() if isinstance(x, np.ndarray)}
    st1 = new_state(one["light_u"], one["eye_u"]); st1["path_value"][:] = one["path_value"]; st1["path_pdf"][:] = one["path_pdf"]
    sp1 = np.zeros_like(splat)
    accept_reject(st1, one["new_value"], one["new_light"], one["new_eye"], u_ar[:1], F32(1.0), 0, h["res"], sp1)
    px = int(quantize(one["eye_u"][3], 8)[0] + quantize(one["eye_u"][4], 4)[0] * 8)
    assert [int(x) for x in sp1[px]] == [int(x) for x in splat_fixed((one["path_value"][0, :3] / F32(0.7)).astype(F32))] and (np.delete(sp1, px, 0) == 0).all()
    thr = {k: (x[:, 3:4] if x.ndim == 2 and x.shape[0] == 9 else x[3:4]) for k, x in h.items() if isinstance(x, np.ndarray)}
    st3 = new_state(thr["light_u"], thr["eye_u"]); st3["path_value"][:] = thr["path_value"]; st3["path_pdf"][:] = thr["path_pdf"]
    sp3 = np.zeros_like(splat)
    accept_reject(st3, thr["new_value"], thr["new_light"], thr["new_eye"], u_ar[:1], F32(1.0), 0, h["res"], sp3)
    assert not sp3.any()
    # corners: chain 4 moves from pixel 0 to the last pixel, chain 5 the other way
    assert splat[0].any() and splat[-1].any()
    frame = resolve(np.zeros((32, 4), F32), splat)
    assert not splat.any() and frame[:, 3].max() == 0 and frame[:, :3].sum() > 0
    # the Cauchy bound: finite in the bulk, without a decision at the poles, values in [0, 1)
    ref, B = cauchy_reference(F32([0.25, 0.25, 0.9]), F32([0.5, 0.0, 0.75]), 0.01)
    assert ref[0] == 0.25 and B[0] < 1e-6 and B[1] > 0.5 and abs(ref[2] - 0.91) < 1e-6 and (ref >= 0).all() and (ref < 1).all()
    assert circular_distance(0.999, 0.001) < 0.0021
