"""fpt-WT's specification (tests/watertight_spec.py, float32 numpy, brute force) against the float64 judge of tests/trace_truth.py -- no GPU.

The restatement is to the watertight kernels what the oracle is to fpt-MT's: tests/test_watertight_gpu.py demands its answers of the kernels bit for bit, and here
it is itself held to what the rays really cross.

  * every closest-hit and any-hit case of tests/test_trace_truth.py, judged by that file's own judges with nothing loosened: robust rays get the fp64 answer within
    the judge's tolerances on t, u and v, no phantom hit, no hit beyond a robust crossing; the rays that lose their true closest crossing stay within the case's
    existing SLIP_BOUND (0 where it has none);
  * rays cast from INSIDE the two closed meshes at their shared edges and vertices: every ray reports a hit and none slips.  These two zeros are what the algorithm
    guarantees: within one ray every triangle sees the same rounded vertices and the edge functions are exactly antisymmetric, so no ray passes between
    two triangles that share an edge or a vertex.  No allowance is attached to them.  (From OUTSIDE a convex mesh the guarantee does not give the fp64 answer at the
    silhouette -- the icosphere/edges and icosphere/vertices cases above lose 15 of 6000 and 22 of 4000 rays, all to "no hit", against bounds of 250 and 400.)
"""
import functools

import numpy as np
import pytest

import test_trace_truth as ttt
import trace_truth as tt
import watertight_spec as wt

INSIDE = [(key, what) for key in ("icosphere", "fan_room") for what in ("edges", "vertices")]
INSIDE_COUNT = {"edges": 6000, "vertices": 4000}


def inside_rays(s, n, seed, what):
    """rays from origins centre + 0.3 extent (U - 0.5) -- well inside either closed mesh -- at a uniform point of a uniformly chosen unique edge, or at a uniformly
    chosen vertex; normalised directions, tmin = 5e-4 extent, tmax = 1e30"""
    rng = np.random.default_rng(seed); lo, hi, ext = ttt._extent(s)
    P = s.vertex_data[:, :3].astype(np.float64); vi = s.vertex_indices[:, :3]
    if what == "edges":
        e = np.unique(np.sort(np.concatenate([vi[:, [0, 1]], vi[:, [1, 2]], vi[:, [2, 0]]]), 1), axis=0)
        e = e[rng.integers(0, len(e), n)]; x = rng.random((n, 1))
        target = P[e[:, 0]] + x * (P[e[:, 1]] - P[e[:, 0]])
    else:
        target = P[rng.integers(0, len(P), n)]
    org = 0.5 * (lo + hi) + (0.3 * ext) * (rng.random((n, 3)) - 0.5)
    d = target - org
    return ttt._make(org, d / np.linalg.norm(d, axis=1, keepdims=True), 5e-4 * ext, 1e30)


@functools.lru_cache(maxsize=None)
def inside_case(key, what):
    """(scene, rays, fp64 truth), computed once and shared with the GPU tests"""
    s = ttt.get_scene(key)
    rays = inside_rays(s, INSIDE_COUNT[what], 41, what)
    return s, rays, tt.truth(s.vertex_indices, s.vertex_data, rays)


@functools.lru_cache(maxsize=None)
def spec_closest(name):
    """the restatement's hits of a closest-hit case of test_trace_truth (computed once, shared with the GPU tests)"""
    s, rays, _ = ttt.closest_case(name)
    return wt.closest(s.vertex_indices, s.vertex_data, rays)


@functools.lru_cache(maxsize=None)
def spec_inside(key, what):
    s, rays, _ = inside_case(key, what)
    return wt.closest(s.vertex_indices, s.vertex_data, rays)


@pytest.mark.parametrize("name", sorted(ttt.CLOSEST))
def test_spec_closest_hits_against_fp64_truth(name):
    hits = spec_closest(name)
    slips = ttt.check_closest_case(name, hits)          # the judge's assertions and the case's SLIP_BOUND, unchanged
    print("%s: %d slips (bound %d)" % (name, slips, ttt.SLIP_BOUND.get(name, 0)))


@pytest.mark.parametrize("key", sorted(ttt.ANY))
def test_spec_any_hit_against_fp64_truth(key):
    s, rays, T = ttt.any_case(key)
    lost = ttt.judge_any(s, rays, T, wt.occluded(s.vertex_indices, s.vertex_data, rays), key)
    print("any/%s: %d lost occluders (bound %d)" % (key, lost, ttt.SLIP_BOUND.get("any/" + key, 0)))
    assert lost <= ttt.SLIP_BOUND.get("any/" + key, 0), (key, lost)


@pytest.mark.parametrize("key,what", INSIDE)
def test_spec_is_watertight_from_inside_a_closed_mesh(key, what):
    s, rays, T = inside_case(key, what)
    assert (T["tri"] >= 0).all(), "the mesh is not closed around the origins"
    hits = spec_inside(key, what)
    escaped = int((hits["triId"] < 0).sum())
    assert escaped == 0, "%s/%s: %d of %d rays from inside the closed mesh report no hit" % (key, what, escaped, len(rays))
    slips = ttt.judge_closest(s, rays, T, hits, "%s/inside-%s" % (key, what))
    assert slips == 0, "%s/%s: %d rays slipped past their closest crossing" % (key, what, slips)
    assert (~T["robust"]).mean() > 0.5          # the sets are aimed at what is ambiguous: edges and vertices


def test_spec_fp64_branch_and_clause_statistics():
    """two figures DESIGN.md 5 and EXPERIMENTS W record, pinned loosely enough to survive another numpy: the fp64 branch is taken by a few per cent of the pairs of axis-parallel rays, and
    the box clause rejects nothing the watertight test accepts on the inside sets"""
    s, rays, _ = ttt.closest_case("jp/axis")
    st = {}
    wt.closest(s.vertex_indices, s.vertex_data, rays, st)
    assert 0.01 < st["fp64"] / st["pairs"] < 0.2, st
    st = {}
    s, rays, _ = inside_case("fan_room", "edges")
    wt.closest(s.vertex_indices, s.vertex_data, rays, st)
    assert st["clause"] == 0, st
