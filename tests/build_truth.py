"""The exact judge of the device tree build (fermat_amd/csrc/fpt_build_lbvh.hip) and of the wide tree's bytes (fpt_bvh.cpp build_wide8 / refit_wide8, fpt_build.hip):
numpy, no GPU, no device code.  The builder computes with plain IEEE arithmetic (no contraction, areas in fp64 rounded once to float), so everything here is held to bits.

Layer A -- a wide tree's bytes as a function of its topology and the mesh.  Given the mesh, words 4..7 of every node (child_base, tri_base, valid, 0), the imask byte,
the records' tri_id column and the intersector, `predict` gives every other byte: the records, the padded triangle boxes, every node's exact box bottom-up (the union of
its used slots' exact boxes; a leaf slot's box is the union of its triangles' padded boxes), the origin words, the three grid exponents and the 48 quantised bytes.
  exponent   the smallest e in [-100, 120] with ext / 2^e <= 255 (-100 for ext <= 0).  A division by a power of two is exact, so this is ext <= 255 * 2^e: with
             ext = m * 2^k, 0.5 <= m < 1 (frexp), 255 * 2^(k-9) < 2^(k-1) <= ext < 2^k < 255 * 2^(k-7), so e is k - 8 or k - 7, decided by one exact comparison.
  qlo / qhi  the largest q in 0..255 with p + q * cell <= lo, the smallest with p + q * cell >= hi, both sides evaluated in double; an empty slot is 255 / 0.
`stack_need_rule` restates the builders' bound of the traversal stack, `stack_model` the stack discipline of fpt_trace_kernel.inc (the traversal burst), driven by hit sets.

The slot check (`slot_check`).  A wide node's children go to the octant slots by the placement that maximises the summed score, score[c][s] = (child centre - node
centre) . direction of slot s: centres 0.5f * (lo + hi) in float, differences and the sum over x, y, z in double, in that order, from 0.0.  The builders find it with
Kuhn-Munkres in double (fpt_cw8_slots.h), so the placement they choose may fall short of the best total by their rounding.  The admissible shortfall is derived, not
measured: for row i = 1..8 the augmenting loop runs at most i times (every run marks one more of the i - 1 matched columns or ends on a free one); a run makes at most
8 x 2 subtractions for the reduced costs (a - u - v over the unmarked columns) and at most 9 x 2 additions for the potentials and the column minima (u += delta and
v -= delta on a marked column, minv -= delta on an unmarked one, j = 0..8): 34.  (1 + 2 + ... + 8) x 34 = 36 x 34 = 1224 double additions, each wrong by at most
2^-53 of a value no larger than the largest |score| of the node: shortfall = 1224 x 2^-53 x max |score| (SLOT_ADDITIONS).  The check evaluates the chosen placement's
total and the best of all placements of the children into the 8 slots in exact rational arithmetic (fractions.Fraction over the doubles, brought to one power-of-two
denominator; the best, the runner-up and an optimal placement by a dynamic programme over the sets of used slots -- the same maximum as the <= 8! = 40 320 placements
one by one, which `slot_check_brute` does for the self-check).  Where the best total is attained by one placement only and the runner-up is more than the shortfall below it, the chosen
placement must be that one.

Layer B -- the device builder's stages replayed from the mesh: 1 references and the 12 bounds words, 2a the 63-bit keys, 2b the stable sort, 3 the radix tree as the
Cartesian tree over the n - 1 common-prefix lengths of neighbouring augmented keys (key, position) -- whose minimum in a range is unique -- in Karras' numbering, 3b the
treelet passes, 4 boxes and the collapse's cost rows, 5 the children every wide node gathers; `Judge.wide_tree` completes it with an optimal slot assignment.

Mutations: `Judge(flags={...})` plants one deliberate mistake (MUTATIONS); the device's data must refuse each (tests/test_build_truth.py)."""
from fractions import Fraction

import numpy as np

F = np.float32
MUTATIONS = ("swap_xz", "round_cell", "no_tiebreak", "dp_tie_larger", "treelet_leaf_limit", "c_prim_half", "leaf_strict", "k8_from_k6", "exp_plus_one", "qlo_nearest",
             "pad_no_scene", "need_no_leaf")
SLOT_ADDITIONS = 36 * 34
MAX_LEAF = 2
GAMMAS = (7, 14, 28)
CELL_DTYPE = np.dtype([("c", "<f4", 7), ("k", "u1", 7), ("k8", "u1"), ("leaf", "u1"), ("count", "u1"), ("spare", "u1", 2)])


# ---- small exact helpers -------------------------------------------------------------------------------------------------------------------------------------
def ordered(f):
    i = np.asarray(f, F).view(np.int32)
    return i ^ ((i >> 31) & 0x7FFFFFFF)


def unordered(i):
    i = np.asarray(i, np.int32)
    return (i ^ ((i >> 31) & 0x7FFFFFFF)).view(F)


def half_area(b):
    """fp64 half area of float boxes [..., 6]; an inverted box has none"""
    b = np.asarray(b, F).astype(np.float64)
    ex, ey, ez = b[..., 3] - b[..., 0], b[..., 4] - b[..., 1], b[..., 5] - b[..., 2]
    return np.where((ex < 0) | (ey < 0) | (ez < 0), 0.0, ex * ey + ez * (ex + ey))


def union(a, b):
    return np.concatenate([np.minimum(a[..., :3], b[..., :3]), np.maximum(a[..., 3:], b[..., 3:])], -1)


def bit_length(v):
    """of non-negative integers below 2^32 (exact through frexp)"""
    return np.frexp(np.asarray(v, np.uint64).astype(np.float64))[1]


def popcount(v):
    v = np.asarray(v, np.uint64); n = np.zeros(v.shape, np.int64)
    for b in range(16):
        n += ((v >> np.uint64(b)) & np.uint64(1)).astype(np.int64)
    return n


class Judge:
    def __init__(self, flags=()):
        assert set(flags) <= set(MUTATIONS)
        self.flags = set(flags)
        self.c_prim = F(0.5) if "c_prim_half" in self.flags else F(0.6)

    # ---- the mesh's share ------------------------------------------------------------------------------------------------------------------------------------
    def scene_mag(self, vtx):
        return F(np.abs(np.asarray(vtx, F)[:, :3]).max()) if len(vtx) else F(0)

    def tri_boxes(self, idx, vtx):
        """lbvh_refs_kernel / refit_records_kernel / build_bvh2: the box of the three vertices padded by (|tri|max + |scene|max) * 2e-6f + 1e-30f, float throughout"""
        P = np.asarray(vtx, F)[np.asarray(idx)[:, :3], :3]
        m0 = np.abs(P).max((1, 2)).astype(F)
        base = m0 if "pad_no_scene" in self.flags else m0 + self.scene_mag(vtx)
        pad = (base * F(2.0e-6) + F(1.0e-30)).astype(F)
        return np.concatenate([P.min(1) - pad[:, None], P.max(1) + pad[:, None]], 1).astype(F)

    def records(self, idx, vtx, tri_id, watertight):
        idx = np.asarray(idx); V = np.asarray(vtx, F)
        ix = idx[tri_id]
        p0, p1, p2 = V[ix[:, 0], :3], V[ix[:, 1], :3], V[ix[:, 2], :3]
        r = np.zeros((len(tri_id), 12), F)
        r[:, 0:3] = p0; r[:, 3:6] = p1 if watertight else p1 - p0; r[:, 6:9] = p2 if watertight else p2 - p0
        r[:, 9] = np.asarray(tri_id, np.int32).view(F); r[:, 10] = ix[:, 3].astype(np.int32).view(F)
        mv = np.maximum(np.abs(p0), np.maximum(np.abs(p1), np.abs(p2))).max(1).astype(F)
        r[:, 11] = (mv + self.scene_mag(vtx)) * F(5.0e-7)
        return r

    # ---- layer A ---------------------------------------------------------------------------------------------------------------------------------------------
    @staticmethod
    def topology(words47, imask):
        """per node and slot: inner (bool), tris (0..2), child (node index), first (record index); and the levels of the breadth-first numbering"""
        w = np.asarray(words47, np.uint32).reshape(-1, 4); N = len(w)
        imask = np.asarray(imask, np.uint32).reshape(N); valid = w[:, 2]
        assert (w[:, 3] == 0).all() and (valid >> 16 == 0).all()
        s = np.arange(8, dtype=np.uint32)
        inner = ((imask[:, None] >> s) & 1).astype(bool)
        pair = (valid[:, None] >> (2 * s)) & 3
        assert np.isin(pair, (0, 1, 3)).all() and not (inner & (pair != 0)).any(), "valid bits are unary and belong to leaf slots"
        tris = np.where(pair == 3, 2, pair).astype(np.int64)
        child = w[:, 0:1].astype(np.int64) + popcount(imask[:, None] & ((1 << s) - 1))
        first = w[:, 1:2].astype(np.int64) + popcount(valid[:, None] & ((1 << (2 * s)) - 1))
        levels = [0, 1]
        while levels[-1] < N:
            nxt = int(inner[levels[-2]:levels[-1]].sum())
            assert nxt > 0, "nodes no level reaches"
            levels.append(levels[-1] + nxt)
        assert levels[-1] == N
        return dict(N=N, inner=inner, tris=tris, child=child, first=first, levels=levels, child_base=w[:, 0].astype(np.int64), tri_base=w[:, 1].astype(np.int64),
                    valid=valid, imask=imask)

    @staticmethod
    def check_numbering(T):
        """breadth-first numbering: child_base and tri_base are the running counts of inner children and triangles in node order"""
        n_inner = T["inner"].sum(1); n_tris = T["tris"].sum(1)
        assert np.array_equal(T["child_base"], 1 + np.concatenate([[0], np.cumsum(n_inner)[:-1]])), "child_base is not the running count of inner children"
        assert np.array_equal(T["tri_base"], np.concatenate([[0], np.cumsum(n_tris)[:-1]])), "tri_base is not the running count of triangles"
        return int(n_tris.sum())

    def grid_exponent(self, ext):
        ext = np.asarray(ext, np.float64)
        m, k = np.frexp(np.where(ext > 0, ext, 1.0))
        e = np.where(ext <= np.ldexp(255.0, k - 8), k - 8, k - 7)
        e = np.where(ext > 0, np.clip(e, -100, 120), -100)
        if "exp_plus_one" in self.flags:
            e = np.minimum(e + 1, 120)
        return e.astype(np.int64)

    def quantise(self, p, e, lo, hi, used):
        """p, e: [N, 3]; lo, hi: [N, 8, 3] float; used [N, 8] -> qlo, qhi uint8 [N, 8, 3]"""
        p = p.astype(np.float64)[:, None, :]; cell = np.ldexp(1.0, e)[:, None, :]
        lo = lo.astype(np.float64); hi = hi.astype(np.float64)
        with np.errstate(all="ignore"):
            ql = np.clip(np.nan_to_num(np.floor((lo - p) / cell)), 0, 255)
            if "qlo_nearest" in self.flags:
                ql = np.clip(np.nan_to_num(np.rint((lo - p) / cell)), 0, 255)
            else:
                for _ in range(300):
                    down = (ql > 0) & ~(p + ql * cell <= lo) & used[..., None]
                    up = (ql < 255) & (p + (ql + 1) * cell <= lo) & ~down & used[..., None]
                    if not (down | up).any():
                        break
                    ql = ql - down + up
            qh = np.clip(np.nan_to_num(np.ceil((hi - p) / cell)), 0, 255)
            for _ in range(300):
                up = (qh < 255) & ~(p + qh * cell >= hi) & used[..., None]
                down = (qh > 0) & (p + (qh - 1) * cell >= hi) & ~up & used[..., None]
                if not (down | up).any():
                    break
                qh = qh + up - down
        ql = np.where(used[..., None], ql, 255); qh = np.where(used[..., None], qh, 0)
        return ql.astype(np.uint8), qh.astype(np.uint8)

    def predict(self, idx, vtx, words47, imask, tri_id, watertight=False):
        """-> dict(nodes [N, 20] uint32, records [m, 12] float32, node_box [N, 6], slot_box [N, 8, 6], topology)"""
        T = self.topology(words47, imask); N = T["N"]
        recs = self.records(idx, vtx, np.asarray(tri_id, np.int64), watertight)
        tb = self.tri_boxes(idx, vtx)[np.asarray(tri_id, np.int64)]
        empty = np.array([3.0e38] * 3 + [-3.0e38] * 3, F)
        slot_box = np.tile(empty, (N, 8, 1)); node_box = np.zeros((N, 6), F)
        used = T["inner"] | (T["tris"] > 0)
        one = T["tris"] >= 1; two = T["tris"] == 2
        f1 = np.where(one, T["first"], 0)
        slot_box[one] = tb[f1[one]]
        slot_box[two] = union(slot_box[two], tb[f1[two] + 1])
        L = T["levels"]
        for lv in range(len(L) - 2, -1, -1):
            a, z = L[lv], L[lv + 1]
            inn = T["inner"][a:z]
            sb = slot_box[a:z]
            sb[inn] = node_box[T["child"][a:z][inn]]
            nb = np.concatenate([sb[..., :3].min(1), sb[..., 3:].max(1)], 1)
            nb[~used[a:z].any(1)] = 0
            node_box[a:z] = nb
        nodes = np.zeros((N, 20), np.uint32); b = nodes.view(np.uint8).reshape(N, 80)
        nodes[:, 0:3] = node_box[:, :3].view(np.uint32)
        e = self.grid_exponent(node_box[:, 3:].astype(np.float64) - node_box[:, :3].astype(np.float64))
        b[:, 12:15] = (e + 127).astype(np.uint8); b[:, 15] = T["imask"].astype(np.uint8)
        nodes[:, 4:8] = np.asarray(words47, np.uint32).reshape(N, 4)
        ql, qh = self.quantise(node_box[:, :3], e, slot_box[..., :3], slot_box[..., 3:], used)
        b[:, 32:56] = np.transpose(ql, (0, 2, 1)).reshape(N, 24); b[:, 56:80] = np.transpose(qh, (0, 2, 1)).reshape(N, 24)
        return dict(nodes=nodes, records=recs, node_box=node_box, slot_box=slot_box, topology=T, exponents=e, used=used)

    def predict_from(self, idx, vtx, nodes, recs, watertight=False):
        nodes = np.asarray(nodes, np.uint32)
        return self.predict(idx, vtx, nodes[:, 4:8], nodes.view(np.uint8).reshape(len(nodes), 80)[:, 15], np.asarray(recs, F)[:, 9].view(np.int32), watertight)

    def stack_need_rule(self, T):
        """lbvh_need_kernel / build_wide8: a node with leaf children may park a triangle group (1), a node with two or more inner children leaves the rest of its group (1),
        plus the largest need below"""
        need = np.zeros(T["N"], np.int64)
        n_inner = T["inner"].sum(1); has_leaf = (T["tris"] > 0).any(1)
        for n in range(T["N"] - 1, -1, -1):
            below = need[T["child_base"][n]:T["child_base"][n] + n_inner[n]].max() if n_inner[n] else 0
            need[n] = (0 if "need_no_leaf" in self.flags else int(has_leaf[n])) + ((1 if n_inner[n] >= 2 else 0) + below if n_inner[n] else 0)
        return need

    @staticmethod
    def stack_model(T, x, hit=None):
        """The traversal burst of fpt_trace_kernel.inc for one ray whose octant word is x = 7 - octant, as the largest stack pointer reached.  hit: [N, 8] bool, the slots
        whose box the ray meets (None: every used slot -- the all-hit adversary; no triangle hit ever shortens the ray).  Per iteration: (1) if the node group in hand
        still holds inner hits, its nearest (highest bit of slot ^ x) is taken and the rest, when not empty, is pushed; the node is tested; its hit triangles become the
        group in hand, after an older triangle group with something pending has been parked on the stack; (2) ONE triangle of the group in hand is tested; (3) with no
        node group in hand: an empty stack ends the ray once no triangle is pending; a node group on top is taken now; a parked triangle group only when none is pending."""
        inner, tris, child = T["inner"].tolist(), T["tris"].tolist(), T["child"].tolist()
        hit = hit.tolist() if hit is not None else None
        order = sorted(range(8), key=lambda s: -(s ^ x))
        grp = [0]; tri = 0; stack = []; sp_max = 0
        while True:
            if grp:
                n = grp[0]; rest = grp[1:]
                if rest:
                    stack.append(rest); sp_max = max(sp_max, len(stack))
                h = hit[n] if hit is not None else None
                grp = [child[n][s] for s in order if inner[n][s] and (h is None or h[s])]
                t = sum(tris[n][s] for s in range(8) if tris[n][s] and (h is None or h[s]))
                if t:
                    if tri:
                        stack.append(tri); sp_max = max(sp_max, len(stack))
                    tri = t
            if tri:
                tri -= 1
            if not grp:
                if not stack:
                    if not tri:
                        return sp_max
                elif isinstance(stack[-1], list):
                    grp = stack.pop()
                elif not tri:
                    tri = stack.pop()

    def stack_model_max(self, T, decoded=None, n_rays=300, seed=1):
        """the adversary in the 8 octant orders and, given the decoded slot boxes (lo, hi [N, 8, 3]), the hit sets of n_rays real rays through the root's box"""
        worst = max(self.stack_model(T, x) for x in range(8))
        if decoded is not None:
            lo, hi = decoded; used = T["inner"] | (T["tris"] > 0)
            rng = np.random.default_rng(seed)
            a = np.where(used[0][:, None], lo[0], np.inf).min(0); z = np.where(used[0][:, None], hi[0], -np.inf).max(0)
            for r in range(n_rays):
                o = a + rng.random(3) * (z - a); d = rng.normal(size=3)
                if r % 7 == 0:
                    d[r % 3] = 0.0
                with np.errstate(all="ignore"):
                    inv = 1.0 / d
                    t0 = (lo - o) * inv; t1 = (hi - o) * inv
                    tn = np.fmax(np.nanmax(np.fmin(t0, t1), -1), 0.0); tf = np.nanmin(np.fmax(t0, t1), -1)
                hit = (tn <= tf) & used
                x = 7 - ((4 if d[0] < 0 else 0) | (2 if d[1] < 0 else 0) | (1 if d[2] < 0 else 0))
                worst = max(worst, self.stack_model(T, x, hit))
        return worst

    # ---- the slot check ----------------------------------------------------------------------------------------------------------------------------------------
    @staticmethod
    def slot_scores(child_box, node_box):
        """[n_ch, 8] doubles: centres in float, differences and the sum over the axes in double"""
        cb = np.asarray(child_box, F); nb = np.asarray(node_box, F)
        cc = (F(0.5) * (cb[:, :3] + cb[:, 3:])).astype(np.float64); nc = (F(0.5) * (nb[:3] + nb[3:])).astype(np.float64)
        d = cc - nc
        sc = np.zeros((len(cb), 8))
        for sl in range(8):
            v = np.zeros(len(cb))
            for k in range(3):
                v = v + d[:, k] * (1.0 if (sl >> (2 - k)) & 1 else -1.0)
            sc[:, sl] = v
        return sc

    @staticmethod
    def _exact_ints(sc):
        fr = [[Fraction(float(v)) for v in row] for row in sc]
        den = max([f.denominator for row in fr for f in row] + [1])
        return [[int(f * den) for f in row] for row in fr], den

    @staticmethod
    def _merge(cur, v, c, p):
        """a state's (best, runner-up, placements attaining the best, one of them) with one more total v attained by c placements (c = 0: a runner-up handed on)"""
        if cur is None:
            assert c
            return (v, None, c, p)
        b, s2, cnt, pl = cur
        if v > b:
            assert c
            return (v, b, c, p)
        if v == b:
            return (b, s2, cnt + c, pl)
        return (b, v if s2 is None or v > s2 else s2, cnt, pl)

    @classmethod
    def best_placement(cls, sc):
        """exact: (best total, runner-up total or None, number of placements attaining the best, one optimal placement, the integer scores, their denominator)"""
        ints, den = cls._exact_ints(sc)
        states = {0: (0, None, 1, ())}          # set of used slots -> the placements of the children so far that use exactly these
        for row in ints:
            nxt = {}
            for mask, (b, s2, cnt, pl) in states.items():
                for s in range(8):
                    if mask >> s & 1:
                        continue
                    m2 = mask | 1 << s
                    cur = cls._merge(nxt.get(m2), b + row[s], cnt, pl + (s,))
                    nxt[m2] = cls._merge(cur, s2 + row[s], 0, None) if s2 is not None else cur
            states = nxt
        best = None
        for b, s2, cnt, pl in sorted(states.values(), key=lambda t: -t[0]):
            best = cls._merge(best, b, cnt, pl)
            if s2 is not None:
                best = cls._merge(best, s2, 0, None)
        return best + (ints, den)

    @classmethod
    def slot_check(cls, child_box, node_box, placed):
        """placed[c] = the slot child c was given.  Returns 'unique' when the check pinned the placement, 'bound' when it held it to the shortfall only"""
        sc = cls.slot_scores(child_box, node_box)
        if len(sc) == 0:
            return "bound"
        assert len(set(placed)) == len(placed) == len(sc)
        best, second, count, pl, ints, den = cls.best_placement(sc)
        got = sum(ints[c][s] for c, s in enumerate(placed))
        short = Fraction(SLOT_ADDITIONS) * Fraction(1, 2 ** 53) * Fraction(float(np.abs(sc).max()))
        assert Fraction(best - got, den) <= short, "slot placement falls short of the best total by %g (admissible %g)" % (float(Fraction(best - got, den)), float(short))
        if count == 1 and (second is None or Fraction(best - second, den) > short):
            assert tuple(placed) == tuple(pl), "the best placement is unique and clear of the shortfall, the builder chose another: %s, best %s" % (tuple(placed), pl)
            return "unique"
        return "bound"

    @classmethod
    def slot_check_brute(cls, sc):
        """every placement one by one in Fractions (the self-check of best_placement; small n only)"""
        import itertools
        tot = sorted((sum(Fraction(float(sc[c][s])) for c, s in enumerate(p)), p) for p in itertools.permutations(range(8), len(sc)))
        best = tot[-1][0]
        n_best = sum(1 for t, _ in tot if t == best)
        second = max((t for t, _ in tot if t < best), default=None)
        return best, second, n_best

    def slot_check_nodes(self, pred, which=None):
        """the check on the nodes `which` of a predicted tree (its exact slot boxes and node boxes): -> number decided uniquely"""
        T = pred["topology"]; used = pred["used"]; unique = 0
        for n in (range(T["N"]) if which is None else which):
            sl = np.flatnonzero(used[n])
            unique += self.slot_check(pred["slot_box"][n, sl], pred["node_box"][n], [int(s) for s in sl]) == "unique"
        return unique

    # ---- layer B: stages 1..3 ----------------------------------------------------------------------------------------------------------------------------------
    def stage1(self, idx, vtx):
        refs = self.tri_boxes(idx, vtx)
        c = (F(0.5) * refs[:, :3] + F(0.5) * refs[:, 3:]).astype(F)
        bounds = np.concatenate([ordered(refs[:, :3]).min(0), ordered(refs[:, 3:]).max(0), ordered(c).min(0), ordered(c).max(0)]).astype(np.int32)
        return refs, bounds

    def stage2(self, refs, bounds):
        c = (F(0.5) * refs[:, :3] + F(0.5) * refs[:, 3:]).astype(F).astype(np.float64)
        lo = unordered(bounds[6:9]).astype(np.float64); hi = unordered(bounds[9:12]).astype(np.float64)
        ext = hi - lo
        with np.errstate(all="ignore"):
            f = np.where(ext > 0, (c - lo) / np.where(ext > 0, ext, 1.0), 0.0)
        f = np.clip(f, 0.0, 1.0)
        s = f * 2097152.0
        q = np.where(s >= 2097151.0, 2097151, np.rint(s) if "round_cell" in self.flags else np.trunc(s)).astype(np.uint64)
        q = np.minimum(q, np.uint64(2097151))
        if "swap_xz" in self.flags:
            q = q[:, ::-1]

        def spread(v):
            x = v & np.uint64(0x1FFFFF)
            for sh, m in ((32, 0x1F00000000FFFF), (16, 0x1F0000FF0000FF), (8, 0x100F00F00F00F00F), (4, 0x10C30C30C30C30C3), (2, 0x1249249249249249)):
                x = (x | (x << np.uint64(sh))) & np.uint64(m)
            return x
        keys = (spread(q[:, 0]) << np.uint64(2)) | (spread(q[:, 1]) << np.uint64(1)) | spread(q[:, 2])
        order = np.argsort(keys, kind="stable")
        return keys[order], order.astype(np.uint32), q

    def radix_tree(self, keys):
        """the Cartesian tree over delta[j] = common prefix of the augmented keys j and j + 1: the split of a range is the position of its (unique) minimum; the node
        of a range is numbered by the end it shares with its parent's split (Karras: node i has i as an end of its range), the root is 0; leaves are ~position"""
        n = len(keys)
        k = np.asarray(keys, np.uint64)
        x = k[:-1] ^ k[1:]
        j = np.arange(n - 1, dtype=np.uint64)
        clz = np.where(x >> np.uint64(32) > 0, 32 - bit_length(x >> np.uint64(32)), 64 - bit_length(x & np.uint64(0xFFFFFFFF)))
        tie = 64 if "no_tiebreak" in self.flags else 64 + 32 - bit_length(j ^ (j + np.uint64(1)))
        delta = np.where(x == 0, tie, clz).astype(np.int64).tolist()
        m = n - 1
        prev = [-1] * m; nxt = [m] * m; st = []
        for i in range(m):
            while st and delta[st[-1]] > delta[i]:          # (a mutated judge without the tie-break: the leftmost minimum)
                nxt[st.pop()] = i
            prev[i] = st[-1] if st else -1
            st.append(i)
        left = np.zeros(m, np.int32); right = np.zeros(m, np.int32)
        for i in range(m):
            l, r = prev[i] + 1, nxt[i]          # the range of keys [l, r], split between i and i + 1
            p, q = prev[i], nxt[i]
            if p < 0 and q >= m:
                node = 0
            elif q >= m or (p >= 0 and delta[p] > delta[q]):
                node = l          # the right child of the split at p: its range starts behind it
            else:
                node = r          # the left child of the split at q: its range ends on it
            left[node] = ~i if l == i else i
            right[node] = ~(i + 1) if r == i + 1 else i + 1
        return left, right

    # ---- layer B: stage 3b -------------------------------------------------------------------------------------------------------------------------------------
    def inv_root_area(self, bounds):
        ra = float(half_area(np.concatenate([unordered(bounds[0:3]), unordered(bounds[3:6])])))
        return 1.0 / (ra if ra > 1.0e-300 else 1.0e-300)

    def rel_area(self, boxes, inv):
        return (half_area(boxes) * inv).astype(F)

    def trbvh_cost(self, area, count, split):
        lim = MAX_LEAF + 1 if "treelet_leaf_limit" in self.flags else MAX_LEAF
        area = np.asarray(area, F); split = np.asarray(split, F)
        c_inner = (area * F(1.0) + split).astype(F)
        c_leaf = np.where(np.asarray(count) <= lim, ((area * np.asarray(count).astype(F)).astype(F) * self.c_prim).astype(F), F(3.0e38)).astype(F)
        return np.where(c_leaf < c_inner, c_leaf, c_inner).astype(F)

    @staticmethod
    def rounds(left, right, visit):
        """the bottom-up sweep in rounds: a node is visited in the first round in which its inner children carry earlier stamps, on the topology as that round finds it
        (visit(round, nodes) may rewire below the nodes it is given); -> the stamps"""
        m = len(left); stamp = np.zeros(m, np.int64); r = 0
        while stamp[0] == 0:
            r += 1
            assert r <= m + 1
            ok = lambda c: (c < 0) | ((stamp[np.maximum(c, 0)] != 0) & (stamp[np.maximum(c, 0)] < r))
            ready = np.flatnonzero((stamp == 0) & ok(left) & ok(right))
            stamp[ready] = r
            visit(r, ready)
        return stamp

    def prep(self, S):
        """box, triangle count and binary SAH cost of every inner node"""
        left, right = S["left"], S["right"]; m = len(left)
        S["node_box"] = np.zeros((m, 6), F); S["tcount"] = np.zeros(m, np.int64); S["tcost"] = np.zeros(m, F)

        def visit(r, p):
            if not len(p):
                return
            b0, n0, c0 = self.ref_data(S, left[p]); b1, n1, c1 = self.ref_data(S, right[p])
            nb = union(b0, b1)
            S["node_box"][p] = nb; S["tcount"][p] = n0 + n1
            S["tcost"][p] = self.trbvh_cost(self.rel_area(nb, S["inv"]), n0 + n1, (c0 + c1).astype(F))
        self.rounds(left, right, visit)

    def ref_data(self, S, ref):
        ref = np.asarray(ref); inner = ref >= 0
        i = np.where(inner, ref, 0); t = S["vals"][np.where(inner, 0, ~ref)]
        box = np.where(inner[..., None], S["node_box"][i], S["refs"][t])
        cnt = np.where(inner, S["tcount"][i], 1)
        cost = np.where(inner, S["tcost"][i], (self.rel_area(S["refs"][t], S["inv"]) * self.c_prim).astype(F)).astype(F)
        return box, cnt, cost

    # the subsets of the 7 leaves with >= 2 members by size, then by mask; for each, its partitions {P, S \ P} with S's lowest leaf in P, P ascending
    SUBSETS = [sorted(s for s in range(1, 128) if bin(s).count("1") == k) for k in range(2, 8)]

    PARTS = {S: np.array([P for P in range(1, S) if (P & ~S) == 0 and (P & S & -S)]) for S in range(3, 128) if S & (S - 1)}

    def treelet_pass(self, S, gamma):
        left, right = S["left"], S["right"]
        stats = dict(rewritten=0, kept=0)

        def visit(r, ready):
            roots = [int(p) for p in ready if S["tcount"][p] >= gamma]
            if not roots:
                return
            T = len(roots)
            refs7 = np.zeros((T, 7), np.int64); inners = []
            for t, R in enumerate(roots):          # formation
                ref = [int(left[R]), int(right[R])]; inner = [R]
                area = lambda x: float(self.rel_area(S["node_box"][x], S["inv"])) if x >= 0 else -1.0
                ar = [area(x) for x in ref]
                while len(ref) < 7:
                    b = -1
                    for k in range(len(ref)):
                        if ref[k] >= 0 and (b < 0 or ar[k] > ar[b] or (ar[k] == ar[b] and ref[k] < ref[b])):
                            b = k
                    assert b >= 0, "a treelet root with fewer than 7 triangles"
                    x = ref[b]; inner.append(x)
                    ref[b:b + 1] = [int(left[x]), int(right[x])]; ar[b:b + 1] = [area(ref[b]), area(ref[b + 1])]
                refs7[t] = ref; inners.append(inner)
            box, cnt, cost1 = self.ref_data(S, refs7)          # [T, 7, 6], [T, 7], [T, 7]
            area = np.zeros((T, 128), F); cost = np.zeros((T, 128), F); N = np.zeros((T, 128), np.int64); part = np.zeros((T, 128), np.int64)
            ub = np.zeros((T, 128, 6), F)
            for s in range(1, 128):
                low = (s & -s).bit_length() - 1
                ub[:, s] = box[:, low] if s == 1 << low else union(ub[:, s & (s - 1)], box[:, low])
                N[:, s] = cnt[:, low] + (N[:, s & (s - 1)] if s != 1 << low else 0)
            area[:] = self.rel_area(ub, S["inv"])
            for k in range(7):
                cost[:, 1 << k] = cost1[:, k]
            for subs in self.SUBSETS:          # the DP, by size: a sequential minimum over all partitions of every subset, equal cost: the smaller P
                for s in subs:
                    P = self.PARTS[s]
                    c = (cost[:, P] + cost[:, s ^ P]).astype(F)
                    if "dp_tie_larger" in self.flags:
                        j = c.shape[1] - 1 - np.argmin(c[:, ::-1], 1)
                    else:
                        j = np.argmin(c, 1)
                    part[:, s] = P[j]
                    cost[:, s] = self.trbvh_cost(area[:, s], N[:, s], c[np.arange(T), j])
            for t, R in enumerate(roots):          # the old topology's cost under the same arithmetic, and the rewrite when the new one is strictly cheaper
                ref = refs7[t].tolist(); inner = inners[t]

                def old(x):
                    mk = 0; cs = []
                    for c in (int(left[x]), int(right[x])):
                        if c in inner[1:] and c >= 0:
                            m2, c2 = old(c)
                        else:
                            m2 = 1 << ref.index(c); c2 = cost[t, m2]
                        mk |= m2; cs.append(c2)
                    return mk, self.trbvh_cost(area[t, mk], N[t, mk], F(cs[0] + cs[1]))
                mk, c_old = old(R)
                assert mk == 127 and not cost[t, 127] > c_old, "the DP's optimum is dearer than the old topology"
                if not cost[t, 127] < c_old:
                    stats["kept"] += 1
                    continue
                stats["rewritten"] += 1
                names = iter([R] + sorted(inner[1:]))

                def write(s):          # pre-order, indices in ascending order
                    if s & (s - 1) == 0:
                        return ref[s.bit_length() - 1]
                    node = next(names)
                    P = int(part[t, s])
                    S["node_box"][node] = ub[t, s]; S["tcount"][node] = N[t, s]; S["tcost"][node] = cost[t, s]
                    l = write(P); rr = write(s ^ P)
                    left[node] = l; right[node] = rr
                    return node
                write(127)
        self.rounds(left, right, visit)
        return stats

    # ---- layer B: stage 4 --------------------------------------------------------------------------------------------------------------------------------------
    def fit(self, S):
        left, right = S["left"], S["right"]; m = len(left)
        S["node_box"] = np.zeros((m, 6), F); cells = np.zeros(m, CELL_DTYPE); S["cells"] = cells

        def row(ref, box):
            inner = ref >= 0; i = np.where(inner, ref, 0)
            v = (self.rel_area(box, S["inv"]) * self.c_prim).astype(F)
            return np.where(inner[:, None], cells["c"][i], v[:, None]).astype(F), np.where(inner, cells["count"][i].astype(np.int64), 1)

        def visit(r, p):
            if not len(p):
                return
            l, rr = left[p], right[p]
            b0 = np.where((l >= 0)[:, None], S["node_box"][np.maximum(l, 0)], S["refs"][S["vals"][np.where(l >= 0, 0, ~l)]])
            b1 = np.where((rr >= 0)[:, None], S["node_box"][np.maximum(rr, 0)], S["refs"][S["vals"][np.where(rr >= 0, 0, ~rr)]])
            nb = union(b0, b1); S["node_box"][p] = nb
            area = self.rel_area(nb, S["inv"])
            cl, pl = row(l, b0); cr, pr = row(rr, b1)
            P = pl + pr
            X = np.zeros(len(p), CELL_DTYPE); X["count"] = np.minimum(P, 255)
            dist = {}; dk = {}
            for j in range(2, 9):
                ks = [k for k in range(1, j) if k <= 7 and j - k <= 7]
                v = np.stack([(cl[:, k - 1] + cr[:, j - k - 1]).astype(F) for k in ks], 1)
                a = np.argmin(v, 1); best = v[np.arange(len(p)), a]
                none = ~(best < F(3.0e38))
                dist[j] = np.where(none, F(3.0e38), best).astype(F); dk[j] = np.where(none, 1, np.array(ks)[a])
            c_internal = (dist[8] + area * F(1.0)).astype(F)
            c_leaf = np.where((P >= 1) & (P <= MAX_LEAF), ((area * P.astype(F)).astype(F) * self.c_prim).astype(F), F(3.0e38)).astype(F)
            leaf = (c_leaf < c_internal) if "leaf_strict" in self.flags else (c_leaf <= c_internal)
            X["leaf"] = leaf
            X["c"][:, 0] = np.where(leaf, c_leaf, c_internal); X["k"][:, 0] = 0
            for i in range(2, 8):
                take = dist[i] < X["c"][:, i - 2]
                X["c"][:, i - 1] = np.where(take, dist[i], X["c"][:, i - 2]); X["k"][:, i - 1] = np.where(take, dk[i], 0)
            X["k8"] = X["k"][:, 6] if "k8_from_k6" in self.flags else dk[8]
            cells[p] = X
        stamp = self.rounds(left, right, visit)
        S["depth_binary"] = int(stamp[0])

    # ---- layer B: stage 5 --------------------------------------------------------------------------------------------------------------------------------------
    def collect(self, S, root):
        """the children the binary subtree `root` contributes to a wide node: [(inner ref or None, triangles, box)], depth-first, left before right"""
        left, right, cells, vals = S["left"], S["right"], S["cells"], S["vals"]
        out = []

        def run(ref, budget):
            assert len(out) < 8
            if ref < 0:
                t = int(vals[~ref]); out.append((None, (t,), S["refs"][t])); return
            X = cells[ref]
            i = budget
            while i > 1 and X["k"][i - 1] == 0:
                i -= 1
            if i <= 1:
                if X["leaf"]:
                    l, r = int(left[ref]), int(right[ref])
                    assert l < 0 and r < 0
                    out.append((None, (int(vals[~l]), int(vals[~r])), S["node_box"][ref]))
                else:
                    out.append((int(ref), (), S["node_box"][ref]))
                return
            run(int(left[ref]), int(X["k"][i - 1])); run(int(right[ref]), i - int(X["k"][i - 1]))
        k8 = int(cells[root]["k8"])
        run(int(left[root]), k8); run(int(right[root]), 8 - k8)
        return out

    # ---- the whole replay --------------------------------------------------------------------------------------------------------------------------------------
    def replay(self, idx, vtx, mode, passes=3, upto=5):
        """-> JudgeTree: every array the device builder's stages leave behind (upto: 3 = through the radix tree, 4 = through the cost rows, 5 = with the wide children)"""
        S = {}
        S["refs"], S["bounds"] = self.stage1(idx, vtx)
        S["keys"], S["vals"], S["cells_q"] = self.stage2(S["refs"], S["bounds"])
        S["left"], S["right"] = self.radix_tree(S["keys"])
        S["inv"] = self.inv_root_area(S["bounds"])
        S["radix_left"], S["radix_right"] = S["left"].copy(), S["right"].copy()
        S["passes"] = []
        if upto >= 4:
            if mode == 2:
                self.prep(S)
                for g in GAMMAS[:passes]:
                    S["passes"].append(self.treelet_pass(S, g))
                S["tcount_final"] = S["tcount"].copy(); S["tcost_final"] = S["tcost"].copy()
            self.fit(S)
        if upto >= 5:
            S["wide"] = {0: self.collect(S, 0)}
            todo = [0]
            while todo:
                b = todo.pop()
                for ref, _, _ in S["wide"][b]:
                    if ref is not None:
                        S["wide"][ref] = self.collect(S, ref); todo.append(ref)
        return S

    def wide_tree(self, S, idx, vtx, watertight=False):
        """the judge's own tree: the children of stage 5 placed by an optimal slot assignment, numbered breadth-first, bytes by layer A -> (nodes, records, stack_need, depth)"""
        queue = [0]; words = []; imasks = []; tri_ids = []; i = 0; levels = [0]
        level_end = 1
        while i < len(queue):
            if i == level_end:
                levels.append(i); level_end = len(queue)
            ch = S["wide"][queue[i]]
            nb = ch[0][2]
            for c in ch[1:]:
                nb = union(nb, c[2])
            pl = self.best_placement(self.slot_scores(np.array([c[2] for c in ch]), nb))[3]
            at = {s: c for c, s in zip(ch, pl)}
            imask = 0; valid = 0; child_base = len(queue); tri_base = len(tri_ids)
            for s in range(8):
                if s not in at:
                    continue
                ref, tris, _ = at[s]
                if ref is not None:
                    imask |= 1 << s; queue.append(ref)
                else:
                    valid |= ((1 << len(tris)) - 1) << (2 * s); tri_ids.extend(tris)
            words.append((child_base, tri_base, valid, 0)); imasks.append(imask); i += 1
        pred = self.predict(idx, vtx, np.array(words, np.uint32), np.array(imasks, np.uint32), np.array(tri_ids, np.int64), watertight)
        need = self.stack_need_rule(pred["topology"])
        return pred["nodes"], pred["records"], int(need[0]), len(pred["topology"]["levels"]) - 1, pred

    # ---- a device (or host) wide tree against stage 5 ------------------------------------------------------------------------------------------------------------
    def same_children(self, S, pred):
        """walks the judged wide children and a given tree's topology side by side from the roots: every wide node must hold the multiset of children stage 5 gathers
        (an inner child is known by the triangles below it, a leaf by its triangles in record order, both with their exact boxes); -> wide nodes compared"""
        T = pred["topology"]; tri_id = pred["records"][:, 9].view(np.int32)
        lo_tri = np.full(T["N"], 1 << 62, np.int64); cnt = np.zeros(T["N"], np.int64)          # the triangles below every wide node: (smallest id, count)
        for n in range(T["N"] - 1, -1, -1):
            for s in range(8):
                if T["inner"][n, s]:
                    c = T["child"][n, s]; lo_tri[n] = min(lo_tri[n], lo_tri[c]); cnt[n] += cnt[c]
                elif T["tris"][n, s]:
                    ids = tri_id[T["first"][n, s]:T["first"][n, s] + T["tris"][n, s]]; lo_tri[n] = min(lo_tri[n], ids.min()); cnt[n] += len(ids)
        left, right, vals = S["left"], S["right"], S["vals"]
        m = len(left); b_lo = np.zeros(m, np.int64); b_cnt = np.zeros(m, np.int64)
        order = []; st = [0]
        while st:
            x = st.pop(); order.append(x)
            st.extend(int(c) for c in (left[x], right[x]) if c >= 0)
        for x in reversed(order):
            v = [(b_lo[c], b_cnt[c]) if c >= 0 else (int(vals[~c]), 1) for c in (int(left[x]), int(right[x]))]
            b_lo[x] = min(v[0][0], v[1][0]); b_cnt[x] = v[0][1] + v[1][1]
        pairs = [(0, 0)]; done = 0
        while pairs:
            b, n = pairs.pop(); done += 1
            want = sorted((("i", int(b_lo[r]), int(b_cnt[r])) if r is not None else ("t",) + tuple(t), np.asarray(box, F).tobytes()) for r, t, box in S["wide"][b])
            got = []; by_sig = {}
            for s in range(8):
                if T["inner"][n, s]:
                    c = int(T["child"][n, s]); sig = ("i", int(lo_tri[c]), int(cnt[c])); by_sig[sig] = c
                    got.append((sig, pred["slot_box"][n, s].tobytes()))
                elif T["tris"][n, s]:
                    f = T["first"][n, s]; got.append((("t",) + tuple(int(t) for t in tri_id[f:f + T["tris"][n, s]]), pred["slot_box"][n, s].tobytes()))
            assert sorted(got) == want, "wide node %d (binary root %d) does not hold the children the collapse's decisions give" % (n, b)
            for r, _, _ in S["wide"][b]:
                if r is not None:
                    pairs.append((r, by_sig[("i", int(b_lo[r]), int(b_cnt[r]))]))
        assert done == T["N"]
        return done


def decode_boxes(nodes):
    """the decoded slot boxes (tests/test_wide_bvh.decode, all nodes at once): lo, hi [N, 8, 3] double"""
    nodes = np.asarray(nodes, np.uint32); N = len(nodes)
    b = nodes.view(np.uint8).reshape(N, 80)
    p = nodes[:, :3].view(F).astype(np.float64); cell = np.ldexp(1.0, b[:, 12:15].astype(np.int64) - 127)
    q = b[:, 32:80].reshape(N, 6, 8).astype(np.float64)
    return p[:, None, :] + np.transpose(q[:, 0:3], (0, 2, 1)) * cell[:, None, :], p[:, None, :] + np.transpose(q[:, 3:6], (0, 2, 1)) * cell[:, None, :]
