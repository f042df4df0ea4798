"""Judges of the path-space-filtering cache (`-psfpt`), independent of the oracle's headers: plain numpy float64, Python integers and fractions.

  key         the jittered spatial hash, src/spatial_hash.h:86-167 of the reference, restated over the reals.  A float32 evaluation differs from the real
              value by rounding, and every field of the key is a DECISION on such a value (a floor, the half-down rounding, a comparison, quantize), so the
              judge returns for every field the SET of integers a correct float32 evaluation can produce: the decision taken at the real value and at +- a bound.
  table       a Python dictionary: what any correct find-or-insert table must satisfy, whichever key wins a race.
  accumulate  the cell sums as Python integers, the cell mean as float32 arithmetic and as an exact fraction.

What the reference leaves undefined is given ONE meaning here, and the oracle and the device are held to it (reference quirks):
  * the grid size is 1 << (level & 31): a cone radius below 2^-32 of the scene (or 0) gives a level above 31 (det_log2(inf) = 128), where the reference's
    `1u << level` is undefined;
  * the level field is the reference's own `uint64(level) << 51`: from level 32 on it runs into the normal digits (bits 56..59) and beyond, OR-ed with them;
  * a coordinate is the low 17 bits of the rounded location (from level 17 on the grid is wider than the field); the rounding goes through a saturating
    int32, so a location of 2^31 or more rounds to 2^31: coordinate 0;
  * a sample of magnitude 2^31 or more (only a firefly value above that lets one through) adds FIXED_MAX = 2^63 - 2^32, resp. FIXED_MIN = -2^63: the device's
    double -> int64 conversion saturates the high word as a signed 32-bit integer and keeps the low word of the value, which is 0 for every float that large."""
from fractions import Fraction

import numpy as np

U = 2.0 ** -24                                   # float32 unit round-off
MULT = 0x9E3779B97F4A7C15                        # the table's multiplicative hash
MULT_INV = pow(MULT, -1, 1 << 64)
EMPTY = (1 << 64) - 1
REFUSED = 0x1FFFFFFF
COORD_MASK = (1 << 17) - 1
FIXED_MAX = (1 << 63) - (1 << 32)
FIXED_MIN = -(1 << 63)

# The bounds, in units of U.  Level: the argument world_extent / (2 cone) carries two roundings (the extent's subtraction, the division; 2 cone is exact), which
# move its log2 by 2 U / ln 2 < 3 U; det_log2 is within 2 ulp = 4 U of max(1, |log2|) (tests/test_bsdf_truth.py, run_detmath_judge): 7 U max(1, log2) in all.
# Coordinates: the location is grid * (((P + T rx) + B ry) - lo) / extent.  rx, ry carry the disk map (a division, det_sincos, three products: < 8 U of the
# radius); the three additions round once each, relative to their own result, which is at most 4 m, m = the largest of |P|, |lo|, |T rx|, |B ry| -- the operands
# that cancel; the product with the grid is exact (a power of two), the division and the extent round once each.  Summed: < 16 U * max(|location|, grid m / extent) in the worst case; the constant in use, 8, is four times the worst the oracle twin showed on three grids of 8192.
# Normal: phi / 2 pi + s3 / 4 carries det_atan2 (< 4 U of pi after its own division), the wrap, one division and one addition: 8 U of a value <= 1.25; (N.z + 1) / 2 + s4 / 4 two additions: 3 U.
# (The level's and the normal digits' bounds are a few U of values of order 1 to 18: a grid of thousands of elements comes that close to one of their decision
# points too rarely to measure them; they stand as derived.)  The worst error seen, as a fraction of the bound, is written next to each check as "margin".
C_LEVEL, C_COORD, C_NU, C_NV = 7.0, 8.0, 8.0, 3.0
PHI_CUT = np.float32(1.0) - np.float32(1.0e-5)   # |N.z| at and above it: phi = 0 (the comparison is made on the float32 input: exact)


def key_fields(key):
    """the fields of 64-bit keys as the reference lays them out (src/spatial_hash.h:155-160); `level` is the 5-bit field, `top` what lies above the normal digits"""
    k = np.asarray(key, np.uint64)
    f = lambda sh, bits: ((k >> np.uint64(sh)) & np.uint64((1 << bits) - 1)).astype(np.int64)  # noqa: E731
    return dict(x=f(0, 17), y=f(17, 17), z=f(34, 17), level=f(51, 5), nu=f(56, 2), nv=f(58, 2), top=f(60, 4))


def make_key(x, y, z, level, nu, nv):
    """Python integers -> the key, the level shifted as the reference shifts it (it may run into the digits above it)"""
    return ((x & COORD_MASK) | ((y & COORD_MASK) << 17) | ((z & COORD_MASK) << 34) | ((level << 51) & EMPTY) | ((nu | (nv << 2)) << 56)) & EMPTY


def _disk(s0, s1):
    """the concentric square -> disk map (contrib/cugar/spherical/mappings_inline.h:56-87) over the reals"""
    a = 2.0 * s0 - 1.0; b = 2.0 * s1 - 1.0
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(a > -b, np.where(a > b, a, b), np.where(a < b, -a, -b))
        phi = np.where(a > -b, np.where(a > b, (np.pi / 4) * (b / a), (np.pi / 4) * (2.0 - a / b)),
                       np.where(a < b, (np.pi / 4) * (4.0 + b / a), np.where(b != 0, (np.pi / 4) * (6.0 - a / b), 0.0)))
    phi = np.where(np.isfinite(phi), phi, 0.0)
    return r * np.cos(phi), r * np.sin(phi)


def _round_half_down(x):
    """cugar::round (contrib/cugar/basic/numbers.h:512-516): the nearest integer, an exact half going DOWN"""
    return np.ceil(x - 0.5)


def _coord(x):
    """uint32(max(round(x), 0)) & mask.  cugar::round goes through int(x), which saturates at 2^31 - 1: from 2^31 on it returns float(2^31 - 1) + 1 = 2^31, so
    the unsigned conversion after it never saturates -- a location that large has the coordinate 0."""
    v = np.where(x >= 2.0 ** 31, 2.0 ** 31, np.maximum(_round_half_down(np.minimum(x, 2.0 ** 31)), 0.0))
    return v.astype(np.uint64).astype(np.int64) & COORD_MASK


def _quantize3(x):
    """cugar::quantize(x, 3) (numbers.h:600-603): int(3 x) clamped to 0..2"""
    return np.clip(np.trunc(x * 3.0), 0, 2).astype(np.int64)


def _mod1(x):
    """cugar::mod(x, 1) (numbers.h:606): x > 0 ? fmod(x, 1) : 1 - fmod(-x, 1) -- so 0 goes to 1"""
    return np.where(x > 0, x - np.trunc(x), 1.0 - (-x - np.trunc(-x)))


def _level(f, s5):
    f = np.maximum(f, 0.0)
    i = np.floor(f)
    return (i + (s5 < f - i)).astype(np.int64)


def judge_key(rec, level, scale=1.0):
    """rec: (n, 32) float32 probe records; level: the level each element's coordinates are judged at (the device's own, once it is admissible).
    Returns for every field an (n, 3) integer array: the decision at the real value minus the bound, at the value, and plus the bound -- the admissible set.
    `scale` shrinks the bounds (the margin search)."""
    r = np.asarray(rec, np.float32).astype(np.float64)
    P, N, T, B, lo, hi = (r[:, 3 * k:3 * k + 3] for k in range(6))
    s = r[:, 18:24]; cone = r[:, 24]; filt = r[:, 25]
    ext = (hi - lo).max(axis=1)
    with np.errstate(divide="ignore"):
        flog = np.log2(np.maximum(ext / (2.0 * cone), 1.0))
    d = scale * C_LEVEL * U * np.maximum(1.0, flog)
    out = dict(level=np.stack([_level(flog + k * d, s[:, 5]) for k in (-1, 0, 1)], axis=1))
    grid = 2.0 ** (np.asarray(level, np.int64) & 31)
    dx, dy = _disk(s[:, 0], s[:, 1])
    rs = filt * cone
    tx = T * (rs * dx)[:, None]; by = B * (rs * dy)[:, None]
    q = ((P + tx) + by) - lo
    loc = grid[:, None] * q / ext[:, None]
    m = np.maximum.reduce([np.abs(P), np.abs(lo), np.abs(tx), np.abs(by)])
    d = scale * C_COORD * U * np.maximum(np.abs(loc), grid[:, None] * m / ext[:, None])
    for c, name in enumerate("xyz"):
        out[name] = np.stack([_coord(loc[:, c] + k * d[:, c]) for k in (-1, 0, 1)], axis=1)
    flat = np.abs(np.asarray(rec, np.float32)[:, 5]) >= PHI_CUT
    phi = np.arctan2(N[:, 1], N[:, 0]); phi = np.where(phi < 0, phi + 2 * np.pi, phi)
    nu = np.where(flat, 0.0, phi / (2 * np.pi))
    d = np.where(flat, 0.0, scale * C_NU * U)              # phi = 0 is exact there, and so are s3 / 4 and 0 + s3 / 4
    out["nu"] = np.stack([_quantize3(_mod1(nu + k * d + s[:, 3] / 4.0)) for k in (-1, 0, 1)], axis=1)
    nv = (N[:, 2] + 1.0) * 0.5 + s[:, 4] / 4.0
    d = scale * C_NV * U
    out["nv"] = np.stack([_quantize3(np.minimum(nv + k * d, 1.0)) for k in (-1, 0, 1)], axis=1)
    return out


def check_keys(rec, keys, scale=1.0):
    """-> (ok per element, wide per element): every field of the key in its admissible set; any field with more than one admissible value"""
    f = key_fields(keys)
    sets = judge_key(rec, f["level"], scale)
    ok = f["top"] == 0
    wide = np.zeros(len(ok), bool)
    for name, cand in sets.items():
        ok &= (cand == f[name][:, None]).any(axis=1)
        wide |= (cand != cand[:, :1]).any(axis=1)
    return ok, wide


def key_margin(rec, keys):
    """the smallest fraction of the bounds (on a ladder of powers of two) under which every key is still admissible"""
    for k in range(-10, 1):
        if check_keys(rec, keys, 2.0 ** k)[0].all():
            return 2.0 ** k
    return float("inf")


# ---- table ----------------------------------------------------------------------------------------------------------------------------------------------------
def home_slot(key, log2_size):
    return ((int(key) * MULT) & EMPTY) >> (64 - log2_size)


def keys_for_slot(slot, log2_size, count, start=0):
    """`count` distinct keys whose home is `slot` of a 2^log2_size table: the multiplier is odd, so key = h * MULT^-1 (mod 2^64) for any h with these top bits"""
    out = [(((slot << (64 - log2_size)) + start + j) * MULT_INV) & EMPTY for j in range(count)]
    assert all(home_slot(k, log2_size) == slot for k in out) and EMPTY not in out
    return np.array(out, np.uint64)


def check_table(keys, log2_size, res):
    """the invariants of a find-or-insert table of 2^log2_size slots after ONE concurrent launch over `keys`; res = the probe's dict"""
    cap = 1 << log2_size
    keys = [int(k) for k in np.asarray(keys, np.uint64)]
    slots = [int(x) for x in res["slots"]]
    table = [int(k) for k in res["table"]]
    assert len(table) == cap and len(slots) == len(keys)
    distinct = set(keys)
    live = [k for k in table if k != EMPTY]
    assert len(live) == len(set(live)), "a key sits in two slots"
    assert set(live) <= distinct, "the table holds something that is no key"
    where = {k: i for i, k in enumerate(table) if k != EMPTY}
    for k, sl in zip(keys, slots):
        if sl == REFUSED:
            assert k not in where, "a refused key is in the table"
        else:
            assert 0 <= sl < cap and table[sl] == k, "an element's slot does not hold its key"
    # (equal keys -> equal slots and different keys -> different slots follow: a slot holds one key, a key sits in one slot)
    if len(distinct) <= cap:
        assert REFUSED not in slots and set(live) == distinct, "a key was refused although all fit"
    else:
        assert len(live) == cap, "keys were refused before the table was full"
        assert all((sl == REFUSED) == (k not in where) for k, sl in zip(keys, slots))
    if "touched" in res:
        n = res["touched_n"]
        t = [int(x) for x in res["touched"][:n]]
        assert n == len(live) and sorted(t) == sorted(where.values()), "the touched list is not the occupied slots, once each"
    return len(live)


# ---- accumulate -----------------------------------------------------------------------------------------------------------------------------------------------
def fixed(v):
    """round_half_even(v * 2^32) of a float32, saturating as stated in the header"""
    q = round(Fraction(float(np.float32(v))) * (1 << 32))
    return FIXED_MAX if q >= (1 << 63) else FIXED_MIN if q < -(1 << 63) else q


def clamp(v, firefly):
    """psf_clamp: a sample with a non-finite component is dropped whole; min(v, firefly) per component (negatives pass)"""
    v = np.asarray(v, np.float32)
    if not np.isfinite(v).all():
        return np.zeros(3, np.float32)
    return np.where(v < np.float32(firefly), v, np.float32(firefly)).astype(np.float32)


def judge_cells(rec, n_cells, firefly):
    """rec: (n, 4) float32 (slot bits, value) -> (n_cells, 4) int64: the sums as 64-bit two's-complement integers (the additions wrap), the counts"""
    rec = np.asarray(rec, np.float32).reshape(-1, 4)
    slots = rec[:, 0].copy().view(np.uint32)
    cells = [[0, 0, 0, 0] for _ in range(n_cells)]
    for sl, v in zip(slots, rec[:, 1:]):
        if sl >= n_cells:
            continue
        c = clamp(v, firefly)
        for k in range(3):
            cells[sl][k] += fixed(c[k])
        cells[sl][3] += 1
    wrap = lambda q: ((q + (1 << 63)) & EMPTY) - (1 << 63)  # noqa: E731
    return np.array([[wrap(q) for q in c] for c in cells], np.int64).reshape(n_cells, 4)


def mean_f32(cells):
    """float(double(sum) * 2^-32) / float(count), evaluated in numpy's float32 / float64 (IEEE, round to nearest even): what the blends compute, bit for bit"""
    cells = np.asarray(cells, np.int64).reshape(-1, 4)
    cw = cells[:, 3].view(np.uint64).astype(np.float32)
    s = (cells[:, :3].astype(np.float64) * 2.0 ** -32).astype(np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):
        return (s / cw[:, None]).astype(np.float32)


def mean_exact(cell):
    return [Fraction(int(cell[k]), 1 << 32) / int(np.uint64(cell[3])) for k in range(3)]


# double(sum) rounds from 2^53 on (2^-53), float() of the scaled sum, float(count) and the division round once each (2^-24 each): to first order 3 U + 2^-53; the
# second-order terms are below U^2 * 4.  Below the float32 normal range (2^-126) the roundings are absolute, half a denormal step each.
MEAN_REL = 3 * U + 2.0 ** -53 + 4 * U * U
MEAN_ABS = 2.0 ** -149
