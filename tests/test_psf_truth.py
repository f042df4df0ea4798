"""The path-space-filtering cache of `-psfpt` on its own: the key function, the open-addressing table and the fixed-point cell arithmetic on inputs a test
chose.  The device probe (fpt_debug_psf, fermat_amd/csrc/fpt_pt.hip -- it calls spatial_hash, psf_insert, psf_clamp, psf_add and psf_cell_mean, the functions
the shading, resolve and blend kernels call) and its oracle twin (orc_psf_probe_n, oracle/oracle_capi.cpp) are judged by tests/psf_truth.py: a float64
restatement of the reference's hash with admissible sets, a Python dictionary, Python integers and fractions.

The CPU leg runs every check on the oracle twin; it also set the constants of the bounds, and the worst error it saw, as a fraction of the bound, is written
next to each check ("margin").  The `gpu` leg runs the same checks on the device probe and compares probe and twin bit for bit on every grid."""
import numpy as np
import pytest

from fermat_amd import scene
import psf_truth as T

F32 = np.float32


class OracleProbe:
    def __call__(self, op, data, **kw):
        from oracle import binding as ob
        return ob.psf_probe(op, data, **kw)


class DeviceProbe:
    def __init__(self, r):
        self.r = r

    def __call__(self, op, data, **kw):
        return self.r.debug_psf(op, data, **kw)


@pytest.fixture(scope="module")
def oprobe(olib):
    return OracleProbe()


@pytest.fixture(scope="module")
def dprobe(table):
    import fermat_amd as fa
    r = fa.Renderer(scene.cornell_box("CornellBox-JP"), 8, 8, fa.default_options(4), table=table)
    yield DeviceProbe(r)
    r.close()


# ---- key: the random grid -----------------------------------------------------------------------------------------------------------------------------------
def key_grid(n=4096, seed=5):
    """boxes of any extent whose corner lies within one extent of the origin (so the cancellation in P - lo loses at most two bits), points inside and a few
    outside, any normal with its frame, any jitter, and cone radii that spread the levels evenly over 0..17 (a tenth of them at 0: cones larger than the box)"""
    rng = np.random.default_rng(seed)
    ext = rng.uniform(1.0, 20.0, (n, 3)); we = ext.max(axis=1)
    lo = rng.uniform(-1.0, 1.0, (n, 3)) * we[:, None]
    P = lo + rng.uniform(0.0, 1.0, (n, 3)) * ext
    out = rng.random(n) < 0.05
    P[out] += rng.uniform(-0.3, 0.3, (int(out.sum()), 3)) * we[out, None]
    N = rng.normal(size=(n, 3)); N /= np.linalg.norm(N, axis=1, keepdims=True)
    N[::97] = [0.0, 0.0, 1.0]; N[1::97] = [0.0, 0.0, -1.0]                                       # the poles: phi = 0
    a = rng.normal(size=(n, 3))
    Tn = np.cross(N, a); Tn /= np.linalg.norm(Tn, axis=1, keepdims=True)
    B = np.cross(N, Tn)
    lev = rng.uniform(-2.0, 17.9, n)
    rec = np.zeros((n, 32), F32)
    rec[:, 0:3] = P; rec[:, 3:6] = N; rec[:, 6:9] = Tn; rec[:, 9:12] = B; rec[:, 12:15] = lo; rec[:, 15:18] = lo + ext
    rec[:, 18:24] = rng.random((n, 6))
    rec[:, 24] = we / 2.0 ** (lev + 1.0)
    rec[:, 25] = rng.choice([1.0, 2.0], n)
    return rec


def run_key_grid(probe):
    rec = key_grid()
    keys = probe(0, rec)
    ok, wide = T.check_keys(rec, keys)
    assert ok.all(), "%d keys with a field outside its admissible set, first %s" % ((~ok).sum(), np.flatnonzero(~ok)[:5])
    # a judge whose sets are mostly two wide proves little: at most a quarter of the elements may have ANY field with more than one admissible value
    assert wide.mean() <= 0.25, wide.mean()
    level = T.key_fields(keys)["level"]
    hist = np.bincount(level, minlength=19)
    assert level.max() <= 18 and (hist[:18] >= len(rec) // 40).all(), hist                       # every level 0..17 is there, none piled
    margin = T.key_margin(rec, keys)
    print("key grid: %d elements, %.1f %% with a wide field, levels %s, margin %.4f" % (len(rec), 100 * wide.mean(), hist.tolist(), margin))
    assert margin <= 0.5           # margin 0.125 (oracle twin): every key stays admissible with an eighth of the bounds
    return rec, keys


# ---- key: exact known answers -------------------------------------------------------------------------------------------------------------------------------
def krec(P, N=(0, 0, 1), s=(0.5, 0.5, 0, 0, 0, 0), cone=0.5, filt=1.0, T_=(1, 0, 0), B=(0, 1, 0), lo=(0, 0, 0), hi=(16, 8, 4)):
    r = np.zeros(32, F32)
    r[0:3] = P; r[3:6] = N; r[6:9] = T_; r[9:12] = B; r[12:15] = lo; r[15:18] = hi; r[18:24] = s; r[24] = cone; r[25] = filt
    return r


def known_answers():
    """Inputs on which every float32 step is exact: the box (0,0,0)..(16,8,4) has extent 16, a cone of 2^-k makes the grid 2^(3+k) (det_log2 of a power of two is
    exact, its fraction 0), the jitter (1/2, 1/2) is the disk's centre and (1, 1/2) its point (1, 0), P is dyadic.  At cone 1/2 the level is 4 and the location is
    P itself.  Normal digits: N = +z gives phi = 0, whose nu = 0 wraps to 1 (cugar::mod sends 0 to 1) -> digit 2; nv = 1 -> digit 2 (quantize clamps 3 to 2)."""
    cut = T.PHI_CUT
    under = np.nextafter(cut, F32(0))
    Z = (2, 2)
    K = []
    add = lambda name, rec, x, y, z, level, nn: K.append((name, rec, T.make_key(x, y, z, level, nn[0], nn[1])))  # noqa: E731
    add("halves round down", krec((2.5, 3.5, 0.5)), 2, 3, 0, 4, Z)
    add("one ulp above / below a half", krec((2.5 + 2.0 ** -20, 3.5 - 2.0 ** -20, 1.5)), 3, 3, 1, 4, Z)
    add("negative locations clamp to 0", krec((-3.0, -0.5, -0.25)), 0, 0, 0, 4, Z)
    add("a half left of the origin, inside the box", krec((-0.5, 0.5, 1.0), lo=(-2, 0, 0), hi=(14, 8, 4)), 1, 0, 1, 4, Z)          # location 1.5 -> 1
    add("P outside the box", krec((20.5, 9.0, 100.0)), 20, 9, 100, 4, Z)
    add("the jitter moves P by filter * cone along T", krec((2.5, 3.0, 1.0), s=(1.0, 0.5, 0, 0, 0, 0), filt=2.0), 3, 3, 1, 4, Z)      # 3.5 -> 3
    add("... and along another T", krec((2.5, 3.0, 1.0), s=(1.0, 0.5, 0, 0, 0, 0), filt=2.0, T_=(0, 0, 1), B=(1, 0, 0)), 2, 3, 2, 4, Z)
    add("level 17: 2^17 is masked to 0 (its bit would be y's lowest)", krec((16.0, 4 * 2.0 ** -13, 5 * 2.0 ** -13), cone=2.0 ** -14), 0, 4, 5, 17, Z)
    add("level 18: 2^17 + 5 is masked to 5 (its bit would be the level's lowest)", krec((0.0, 16.0 + 6 * 2.0 ** -14, 8.0 + 5 * 2.0 ** -14), cone=2.0 ** -15), 0, 6, 5, 18, Z)
    add("level 17: 2^17 - 1 fits", krec((16.0 - 2.0 ** -13, 0.0, 2.0 ** -13), cone=2.0 ** -14), (1 << 17) - 1, 0, 1, 17, Z)
    add("level 20: the low 17 bits", krec((16.0 + 2.0 ** -15, 1.0, 3 * 2.0 ** -16), cone=2.0 ** -17), 2, 1 << 16, 3, 20, Z)
    add("|N.z| just under the cut: phi = pi / 2", krec((1, 1, 1), N=(0.0, 0.004, under)), 1, 1, 1, 4, (0, 2))
    add("|N.z| at the cut: phi = 0", krec((1, 1, 1), N=(0.0, 0.004, cut)), 1, 1, 1, 4, (2, 2))
    add("N.z at minus the cut", krec((1, 1, 1), N=(0.0, 0.004, -cut)), 1, 1, 1, 4, (2, 0))
    add("phi exactly 0 wraps to the top digit", krec((1, 1, 1), N=(1.0, 0.0, 0.0)), 1, 1, 1, 4, (2, 1))
    add("phi just below 0: + 2 pi rounds to 2 pi, nu = 1 wraps to 0", krec((1, 1, 1), N=(1.0, -1.0e-8, 0.0)), 1, 1, 1, 4, (0, 1))
    add("phi just below 2 pi", krec((1, 1, 1), N=(1.0, -1.0e-3, 0.0)), 1, 1, 1, 4, (2, 1))
    add("phi = pi / 2 and a quarter turn of jitter", krec((1, 1, 1), N=(0.0, 1.0, 0.0), s=(0.5, 0.5, 0, 1.0, 0, 0)), 1, 1, 1, 4, (1, 1))      # nu = 1/4 + 1/4
    add("nv + s4 / 4 reaching 1", krec((1, 1, 1), N=(0.8660254, 0.0, 0.5), s=(0.5, 0.5, 0, 0, 1.0, 0)), 1, 1, 1, 4, (2, 2))
    add("nv = 1/2 + 3/16", krec((1, 1, 1), N=(1.0, 0.0, 0.0), s=(0.5, 0.5, 0, 0, 0.75, 0)), 1, 1, 1, 4, (2, 2))
    add("nv = 1/2 + 1/8", krec((1, 1, 1), N=(1.0, 0.0, 0.0), s=(0.5, 0.5, 0, 0, 0.5, 0)), 1, 1, 1, 4, (2, 1))
    add("s5 equal to the fractional level (0): no step up", krec((2.5, 1, 1), s=(0.5, 0.5, 0, 0, 0, 0.0)), 2, 1, 1, 4, Z)
    add("s5 below the fractional level: one level up", krec((1.25, 1.0, 0.5), s=(0.5, 0.5, 0, 0, 0, 0.25), cone=0.375), 2, 2, 1, 5, Z)       # log2(64/3) = 4.415
    add("s5 above it", krec((1.25, 1.0, 0.5), s=(0.5, 0.5, 0, 0, 0, 0.5), cone=0.375), 1, 1, 0, 4, Z)
    add("level 0 from a cone larger than the scene", krec((12.0, 4.0, 2.0), cone=100.0), 1, 0, 0, 0, Z)
    # the out-of-range regime (psf_truth.py's header): level 43 = 32 + 11 -> grid 2^11, its bit 5 lands on the first normal digit's low bit, OR-ed
    add("level 43", krec((1.0, 0.5, 0.25), N=(0.0, 1.0, 0.0), s=(0.5, 0.5, 0, 0.5, 0, 0), cone=2.0 ** -40), 128, 64, 32, 43, (1, 1))
    add("level 32: grid 1", krec((24.0, 8.0, 40.0), cone=2.0 ** -29), 1, 0, 2, 32, Z)
    add("cone radius 0: level 128, grid 1", krec((24.0, 8.0, 40.0), cone=0.0), 1, 0, 2, 128, Z)
    add("level 31: a location of 2^32, of 2^31, and the low bits of 2^30 + 3 * 2^15", krec((32.0, 16.0, 8.0 + 3 * 2.0 ** -12), cone=2.0 ** -28), 0, 0, 3 << 15, 31, Z)
    assert T.make_key(128, 64, 32, 43, 1, 1) != 128 + (64 << 17) + (32 << 34) + (43 << 51) + (5 << 56)                                    # OR-ed, not added
    return K


def run_key_known(probe):
    K = known_answers()
    keys = probe(0, np.stack([k[1] for k in K]))
    bad = ["%s: got %016x, want %016x" % (name, int(got), want) for (name, _, want), got in zip(K, keys) if int(got) != want]
    assert not bad, "\n".join(bad)
    return keys


# ---- table --------------------------------------------------------------------------------------------------------------------------------------------------
def table_cases():
    rng = np.random.default_rng(9)
    rand = lambda n: rng.integers(0, 1 << 63, n, dtype=np.uint64) * np.uint64(2) + np.uint64(rng.integers(0, 2))  # noqa: E731
    cases = []
    for log2 in (1, 2, 6, 10):
        cap = 1 << log2
        for load in (0.5, 0.9, 1.0, 1.5):
            k = rand(max(1, int(round(load * cap))))
            k = np.concatenate([k, k, k]); rng.shuffle(k)                                      # every key three times, anywhere in the launch
            cases.append(("2^%d load %.1f" % (log2, load), log2, k))
    cases.append(("all keys equal", 6, np.full(2048, 0x0123456789ABCDEF, np.uint64)))
    for log2 in (2, 6, 10):
        cap = 1 << log2
        last = T.keys_for_slot(cap - 1, log2, cap // 2 + 1)
        cases.append(("2^%d: all in the last slot, probing wraps" % log2, log2, np.concatenate([last, last[::-1]])))
        cases.append(("2^%d: last slot, more keys than slots" % log2, log2, T.keys_for_slot(cap - 1, log2, cap + 3)))
    run = T.keys_for_slot(17, 10, 700)
    cases.append(("a run of 700 from one slot, then others into the run", 10, np.concatenate([run, T.keys_for_slot(300, 10, 200), run[:50]])))
    cases.append(("the key 0", 6, np.concatenate([np.zeros(5, np.uint64), rand(20), np.zeros(5, np.uint64)])))
    hi = np.uint64(0x00FFFFFFFFFFFFFF) & rand(1)[0]
    cases.append(("keys that differ only above bit 56", 6, np.array([int(hi) | (j << 57) for j in range(48)] * 2, np.uint64)))
    return cases


def run_table(probe):
    filled = 0
    for i, (name, log2, keys) in enumerate(table_cases()):
        assert T.EMPTY not in [int(k) for k in keys]
        for touched in ((False, True) if i % 3 == 0 or "last" in name else (False,)):
            res = probe(1, keys, size=log2, touched=touched)
            try:
                filled += T.check_table(keys, log2, res)
            except AssertionError as e:
                raise AssertionError("%s (touched %s): %s" % (name, touched, e))
    assert filled > 5000


# ---- accumulate ---------------------------------------------------------------------------------------------------------------------------------------------
def slot_bits(i):
    return np.array([i], np.uint32).view(F32)[0]


def acc_records(values, slots):
    rec = np.zeros((len(values), 4), F32)
    rec[:, 0] = np.asarray(slots, np.uint32).view(F32)
    rec[:, 1:] = np.asarray(values, F32).reshape(len(values), -1)
    return rec


def accumulate_cases():
    rng = np.random.default_rng(21)
    ff = F32(2.5)
    up = np.nextafter(ff, F32(np.inf))
    edge = [0.0, 2.0 ** -33, -2.0 ** -33, 1.5 * 2.0 ** -32, 2.5 * 2.0 ** -32, -1.5 * 2.0 ** -32, 1.0e-40, -1.0e-45, 2.0 ** -126, -1.0, -3.0e30, float(ff), float(up), 1.0e9,
            0.1, 1.0 / 3.0, 2.0 ** -32, 2.0 ** -32 + 2.0 ** -55]
    vals = [(v, 0.25, -v) for v in edge] + [(np.nan, 1.0, 1.0), (1.0, np.inf, 1.0), (1.0, 1.0, -np.inf), (np.inf, np.nan, 0.0)]
    small = acc_records(vals, np.arange(len(vals)) % 3)                                        # slots 0..2 of 4: slot 3 stays empty
    n = 6144                                                                                     # 24 blocks: every slot is hit from many waves at once
    many = acc_records(np.where(rng.random((n, 3)) < 0.1, rng.choice(F32(edge), (n, 3)), rng.normal(0.5, 1.5, (n, 3))), rng.integers(0, 5, n))
    many[::50, 0] = slot_bits(7)                                                                 # beyond the cells: skipped
    big = [(2.0 ** 31 - 2.0 ** 7, 2.0 ** 31, 1.0e20), (-(2.0 ** 31 - 2.0 ** 7), -2.0 ** 31, -1.0e20), (2.0 ** 31, 2.0 ** 31, 3.0e38), (2.0 ** 31, 2.0 ** 30, -3.0e38), (1.0e30, 1.0e31, 1.0)]
    huge = acc_records(big, [0, 1, 2, 2, 3])
    return [("edges", small, 4, float(ff)), ("many per slot", many, 5, float(ff)), ("beyond 2^31", huge, 4, 1.0e30)]


def run_accumulate(probe):
    # the saturating conversion, pinned: what the device's double -> int64 gives beyond the range
    assert T.fixed(2.0 ** 31 - 2.0 ** 7) == (1 << 63) - (1 << 39) and T.fixed(2.0 ** 31) == T.fixed(1.0e20) == (1 << 63) - (1 << 32)
    assert T.fixed(-2.0 ** 31) == T.fixed(-1.0e20) == -(1 << 63) and T.fixed(1.5 * 2.0 ** -32) == 2 and T.fixed(2.0 ** -33) == T.fixed(-2.0 ** -33) == 0
    out = []
    for name, rec, n_cells, ff in accumulate_cases():
        got = probe(2, rec, size=n_cells, firefly=ff)
        want = T.judge_cells(rec, n_cells, ff)
        assert np.array_equal(got["cells"], want), "%s:\n%s\n%s" % (name, got["cells"], want)
        live = want[:, 3] != 0
        assert np.array_equal(got["mean"][live].view(np.uint32), T.mean_f32(want)[live].view(np.uint32)), name
        assert (got["mean"][~live] == 0).all(), name                                             # a count of 0 is never divided
        out.append(got)
    return out


def mean_cells():
    S = [0, 1, -1, 3, 12345678901234, -98765432109876, (1 << 53) - 1, 1 << 53, (1 << 53) + 1, (1 << 53) + 3, -((1 << 53) + 1), (1 << 54) + 2, (1 << 54) + 6,
         (1 << 62) + (1 << 9), T.FIXED_MAX, T.FIXED_MIN, 3 << 32, (1 << 32) // 3]
    cells = [(a, b, S[(i * 7 + j) % len(S)], c) for c in (1, 3, (1 << 24) + 1, (1 << 24) + 3, 1 << 40, 0) for i, a in enumerate(S) for j, b in enumerate(S[::5])]
    return np.array(cells, np.int64)


def run_mean(probe):
    cells = mean_cells()
    got = probe(3, cells)
    live = cells[:, 3] != 0
    assert (got[~live] == 0).all()
    want = T.mean_f32(cells)
    assert np.array_equal(got[live].view(np.uint32), want[live].view(np.uint32))
    worst = 0.0
    for c, g in zip(cells[live], got[live]):
        for e, v in zip(T.mean_exact(c), g):
            bound = T.MEAN_REL * abs(float(e)) + T.MEAN_ABS
            err = abs(float(abs(e - T.Fraction(float(v)))))
            assert err <= bound, (c, v, float(e))
            worst = max(worst, err / bound)
    print("cell mean: %d cells, worst error / bound %.3f" % (int(live.sum()), worst))
    assert worst <= 1.0            # margin 0.51 (oracle twin and device)
    return got


# ---- the CPU leg: the oracle twin ---------------------------------------------------------------------------------------------------------------------------
def test_key_grid_admissible_sets_oracle(oprobe):
    run_key_grid(oprobe)


def test_key_known_answers_oracle(oprobe):
    run_key_known(oprobe)


def test_judge_sets_are_tight_and_catch_a_wrong_key(oprobe):
    """the judge on its own: a key with one field moved by one, two fields swapped or the level raised is refused on (nearly) every element it changes"""
    rec = key_grid(1024, seed=6)
    keys = oprobe(0, rec)
    f = T.key_fields(keys)
    u = lambda a, sh: a.astype(np.uint64) << np.uint64(sh)  # noqa: E731
    mk = lambda **kw: (lambda g: u(g["x"], 0) | u(g["y"], 17) | u(g["z"], 34) | u(g["level"], 51) | u(g["nu"], 56) | u(g["nv"], 58))({**f, **kw})  # noqa: E731
    assert np.array_equal(mk(), keys)
    for name, wrong in (("x + 1", mk(x=f["x"] + 1)), ("z + 1", mk(z=f["z"] + 1)), ("x <-> y", mk(x=f["y"], y=f["x"])), ("level + 1", mk(level=f["level"] + 1)),
                        ("nu + 1", mk(nu=(f["nu"] + 1) % 3)), ("nv <-> nu", mk(nu=f["nv"], nv=f["nu"]))):
        ok, _ = T.check_keys(rec, wrong)
        changed = wrong != keys
        assert changed.mean() > 0.3 and ok[changed].mean() < 0.25, (name, changed.mean(), ok[changed].mean())


def test_table_invariants_oracle(oprobe):
    run_table(oprobe)


def test_judge_refuses_broken_tables():
    """the dictionary judge on tables that are wrong in the ways open addressing goes wrong"""
    keys = T.keys_for_slot(3, 2, 4)
    good = dict(slots=np.array([3, 0, 1, 2], np.uint32), table=np.array([keys[1], keys[2], keys[3], keys[0]], np.uint64))
    T.check_table(keys, 2, good)
    twice = dict(slots=np.array([3, 0, 1, 1], np.uint32), table=np.array([keys[1], keys[2], T.EMPTY, keys[0]], np.uint64))          # two keys, one slot
    early = dict(slots=np.array([3, 0, 1, T.REFUSED], np.uint32), table=np.array([keys[1], keys[2], T.EMPTY, keys[0]], np.uint64))  # refused with room left
    dup = dict(slots=np.array([3, 0, 3, 0], np.uint32), table=np.array([keys[0], T.EMPTY, T.EMPTY, keys[0]], np.uint64))            # one key in two slots
    for bad, k in ((twice, keys), (early, keys), (dup, keys[[0, 0, 0, 0]])):
        with pytest.raises(AssertionError):
            T.check_table(k, 2, bad)
    with pytest.raises(AssertionError):
        T.check_table(keys, 2, dict(good, touched=np.array([0, 1, 2, 2], np.uint32), touched_n=4))


def test_accumulate_sums_oracle(oprobe):
    run_accumulate(oprobe)


def test_cell_mean_oracle(oprobe):
    run_mean(oprobe)


# ---- the GPU leg: the device probe, and probe == twin bit for bit ----------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_key_grid_admissible_sets_device(dprobe, oprobe):
    rec, keys = run_key_grid(dprobe)
    assert np.array_equal(keys, oprobe(0, rec))


@pytest.mark.gpu
def test_key_known_answers_device(dprobe, oprobe):
    assert np.array_equal(run_key_known(dprobe), run_key_known(oprobe))


@pytest.mark.gpu
def test_table_invariants_device(dprobe, oprobe):
    run_table(dprobe)
    # where every key fits, the table holds the same keys as the twin's (in other slots, perhaps: the winners of a race differ)
    for name, log2, keys in table_cases():
        if len(set(keys.tolist())) <= (1 << log2):
            assert np.array_equal(np.sort(dprobe(1, keys, size=log2)["table"]), np.sort(oprobe(1, keys, size=log2)["table"])), name


@pytest.mark.gpu
def test_accumulate_sums_device(dprobe, oprobe):
    for a, b in zip(run_accumulate(dprobe), run_accumulate(oprobe)):
        assert np.array_equal(a["cells"], b["cells"]) and np.array_equal(a["mean"].view(np.uint32), b["mean"].view(np.uint32))


@pytest.mark.gpu
def test_cell_mean_device(dprobe, oprobe):
    assert np.array_equal(run_mean(dprobe).view(np.uint32), run_mean(oprobe).view(np.uint32))
