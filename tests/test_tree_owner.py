"""The acceleration structure has one owner (fpt_host.h AccelTree) and is replaced all or nothing: a build that is refused -- in any of the three build modes --
leaves the old tree, its description and its hits exactly as they were, and the tree still refits afterwards; releasing the device builder's scratch
(fpt_rt_set_build_mode(0)) costs nothing but the next device build's allocation."""
import ctypes as C

import numpy as np
import pytest

import fermat_amd as fa

from test_gpu_parity import _random_rays

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _no_mode_override(monkeypatch):
    """every test here picks its build modes itself: an FPT_BVH_BUILD of the caller's would override them (monkeypatch restores it afterwards)"""
    monkeypatch.delenv("FPT_BVH_BUILD", raising=False)


def _state(r, rays):
    """what a caller can see of the tree: bvh_info, bvh_stats without its times, the downloaded arrays, the hits of a fixed ray set"""
    stats = {k: v for k, v in r.bvh_stats().items() if not k.startswith("seconds_")}
    nodes, recs = r.download_bvh()
    return r.bvh_info(), stats, nodes.tobytes(), recs.tobytes(), r.trace(rays).tobytes()


def _built(s, table, mode):
    r = fa.Renderer(s, 16, 16, fa.default_options(2), table=table)
    r.set_build_mode(mode); r.rebuild_geometry()
    return r


def _create(r, d_idx, d_vtx):
    s = r.scene
    rc = r.L.fpt_rt_create_geometry(r.ctx, C.c_uint32(s.num_triangles), C.c_void_p(d_idx.data_ptr()), C.c_uint32(s.num_vertices), C.c_void_p(d_vtx.data_ptr()))
    return rc, r.L.fpt_last_error(r.ctx)


@pytest.mark.parametrize("good_mode", [0, 1, 2], ids=["quality", "fast", "trbvh"])
def test_a_refused_build_leaves_the_old_geometry_usable(good_mode, table, standin_small):
    s = standin_small
    L = fa.lib()
    # The non-finite mesh of the quality case.  A NaN coordinate is NOT refused: every min / max of the builder skips it (test_gpu_parity's refit test says the
    # same), the tree is built and only that triangle's own tests fail.  What the host builder refuses is an INFINITE coordinate, so that is the case here -- and
    # that it refuses it, rather than building something, is asked without a context and without a device first
    v_inf = int(s.vertex_indices[s.num_triangles // 2, 1])
    h_inf = np.array(s.vertex_data, np.float32, copy=True); h_inf[v_inf, 1] = np.inf
    idx = np.ascontiguousarray(s.vertex_indices, np.int32)
    nn, nr, dp, nw = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_uint32()
    assert L.fpt_debug_build_bvh(C.c_uint32(s.num_triangles), C.c_void_p(idx.ctypes.data), C.c_uint32(s.num_vertices), C.c_void_p(h_inf.ctypes.data),
                                 C.byref(nn), C.byref(nr), C.byref(dp), C.byref(nw), None, None, None) != 0
    assert b"quantisation error" in L.fpt_last_error(None)

    r = _built(s, table, good_mode)
    rays = _random_rays(s, 20000, 21)
    want = _state(r, rays)
    assert want[0]["leaf_tris"] == s.num_triangles and want[0]["nodes"] > 8
    bad_idx = r.d_vi.clone(); bad_idx[7, 1] = s.num_vertices + 5
    for mode in (0, 1, 2):
        r.set_build_mode(mode)
        rc, err = _create(r, bad_idx, r.d_vd)
        assert rc != 0 and b"vertex index out of range" in err, (mode, err)
        assert _state(r, rays) == want, "a refused build (mode %d, index out of range) changed the geometry" % mode
    r.set_build_mode(0)
    rc, err = _create(r, r.d_vi, r.torch.from_numpy(h_inf).to(r.dev))
    assert rc != 0 and b"quantisation error" in err, err
    assert _state(r, rays) == want, "a refused build (quality, infinite vertex) changed the geometry"
    # ... and the tree still follows the vertices: the same refit as on a context that never saw a refused build
    rng = np.random.default_rng(4)
    ext = float(np.max(np.asarray(s.bbox[1]) - np.asarray(s.bbox[0])))
    moved = s.vertex_data.copy(); moved[:, :3] += (rng.standard_normal((len(moved), 3)) * 0.02 * ext).astype(np.float32)
    r.refit_geometry(moved)
    fresh = _built(s, table, good_mode)
    assert _state(fresh, rays) == want
    fresh.refit_geometry(moved)
    got, ref = _state(r, rays), _state(fresh, rays)
    assert got == ref and got[2:] != want[2:]
    r.close(); fresh.close()


def test_releasing_the_build_scratch_is_harmless(table, standin_small):
    s = standin_small
    rays = _random_rays(s, 20000, 22)
    r = _built(s, table, 0)
    quality = _state(r, rays)
    r.set_build_mode(1); r.rebuild_geometry()
    fast = _state(r, rays)
    assert fast[4] == quality[4] and fast[2] != quality[2]
    r.set_build_mode(0)                      # releases the device builder's scratch
    r.rebuild_geometry()
    assert _state(r, rays) == quality
    r.set_build_mode(1); r.rebuild_geometry()          # ... which the next device build allocates again
    assert _state(r, rays) == fast
    r.set_build_mode(0); r.set_build_mode(2); r.rebuild_geometry()
    assert _state(r, rays)[4] == quality[4] and r.bvh_stats()["optimise_iterations"] == 3
    r.close()
