"""What every render call passes through has one owner each (fpt_host.h): the render lanes (RenderLanes), the render calls the library holds back
(DeferredRun) and the launch timing (LaunchTimer).

CornellBox-Glossy 128 x 64 -- 8192 pixels, the smallest frame two lanes really split (a lane takes at least 4096) -- max_path_length 4, frames compared bit for
bit.  A pass of one lane is then 9 timed launches: the primary trace, 4 shading launches, 3 MIXED traversal launches and no shadow launch at the last bounce
(the Cornell boxes have no directional light, and the last bounce draws no light sample).

Every fpt_pt_init draws its shift table from the context's random stream, so a context that went through a detour is compared with one that made the same inits
without it (as tests/test_psf_owner.py does)."""
import ctypes as C

import numpy as np
import pytest

import fermat_amd as fa
from fermat_amd import api

U32 = np.uint32
RES = (128, 64)
L = 4
SHADE_PER_PASS = L          # shading launches of one pass of one lane


def bits(a):
    return np.ascontiguousarray(a).view(U32)


def make(scn, table, **kw):
    return fa.Renderer(scn, RES[0], RES[1], fa.default_options(L), table=table, **kw)


def last_error(r):
    return r.L.fpt_last_error(r.ctx).decode()


def pt_init(r):
    o = fa.default_options(L)
    return r.L.fpt_pt_init(r.ctx, C.byref(o), C.byref(r.view), r.samples_dir.encode(), None, C.c_uint32(r.n_local))


def psf_init(r):
    o = fa.default_options(L); p = fa.default_psf_options()
    return r.L.fpt_psfpt_init(r.ctx, C.byref(o), C.byref(p), C.byref(r.view), r.samples_dir.encode(), None, C.c_uint32(r.n_local))


def reinit_at(r, res_x, res_y):
    """fpt_pt_init of the same context, without a pixel list, for a frame of another size"""
    t = r.torch
    n = res_x * res_y
    r.synchronize()
    r.res = (res_x, res_y); r.n_local = n
    r.fb = t.zeros((8, n, 4), dtype=t.float32, device=r.dev)
    r.gb_geo = t.zeros((n, 4), dtype=t.float32, device=r.dev); r.gb_uv = t.zeros((n, 4), dtype=t.float32, device=r.dev)
    r.gb_tri = t.full((n,), -1, dtype=t.int32, device=r.dev); r.gb_depth = t.zeros((n,), dtype=t.float32, device=r.dev)
    r.view = r._make_view(1.0, 2.2)
    t.cuda.synchronize(r.dev)
    r._check(pt_init(r))


def same_frame(x, y, what="", channels=range(8)):
    fx, fy = x.framebuffer(), y.framebuffer()
    for c in channels:
        assert np.array_equal(bits(fx[c]), bits(fy[c])), (what, c)
    assert fx[api.FB_COMPOSITED_C][:, :3].max() > 0, what


def two_passes(r):
    r.clear_framebuffer()
    r.render_pass(0); r.render_pass(1)
    return r.collect_timings()["shade"][1]


@pytest.mark.gpu
def test_lanes_and_reinit(cornell_glossy, table):
    """1. two lanes run two launch chains; an fpt_pt_init for another pixel count leaves ONE lane and says so (before the owner it kept reporting two while the
    identity list of the old size made every render fall back to one, silently); two lanes set again run two chains again"""
    x, one = make(cornell_glossy, table), make(cornell_glossy, table)
    x.set_lanes(2); x.set_profiling(2)
    assert x.lane_count() == 2
    assert two_passes(x) == 2 * 2 * SHADE_PER_PASS
    one.render_pass(0); one.render_pass(1)
    same_frame(x, one, "two lanes against one")
    reinit_at(x, 128, 96)
    assert x.lane_count() == 1
    assert two_passes(x) == 1 * 2 * SHADE_PER_PASS
    reinit_at(one, 128, 96)
    one.render_pass(0); one.render_pass(1)
    same_frame(x, one, "after the re-init")
    x.set_lanes(2)
    assert x.lane_count() == 2
    assert two_passes(x) == 2 * 2 * SHADE_PER_PASS
    same_frame(x, one, "two lanes set again")
    x.close(); one.close()


@pytest.mark.gpu
def test_lane_cycling(cornell_glossy, table):
    """2. fpt_pt_set_lanes 3 -> 1 -> 2 -> 4 -> 1 with a batch of three passes in flight at every step: set() synchronises every lane before it swaps the new ones
    in, and every frame is the first one.  The context is closed with four lanes, level-2 profiling and a batch in flight"""
    r = make(cornell_glossy, table)
    r.set_batch(3)
    first = None
    for n in (3, 1, 2, 4, 1):
        r.set_lanes(n)
        assert r.lane_count() == n
        r.clear_framebuffer()
        r.render_batch(0, 3)
        f = r.framebuffer()
        if first is None:
            first = f
            assert f[api.FB_COMPOSITED_C][:, :3].max() > 0
        assert np.array_equal(bits(f), bits(first)), n
        r.render_batch(3, 3)          # in flight when the next step replaces the lanes
    r.set_lanes(4); r.set_profiling(2)
    r.render_batch(0, 3)
    r.close()


def _deferred_detour(x, y, render, resize, who, rearm, y_init=None, channels=range(8)):
    """x: two passes pending, then `resize` (a call that re-sizes storage), then two more render calls.  The re-size call succeeds or refuses naming itself; no later
    synchronize reports an error; every pass whose render call returned success is in the frame: y renders those one by one (and makes the same init, `y_init`, where
    the re-size call is one).  Then the deferral is set up again (`rearm`) and three more passes follow"""
    render(x, 0); render(x, 1)
    done = [0, 1]
    st = resize(x)
    assert st == 0 or who in last_error(x), last_error(x)
    for i in (2, 3):
        try:
            render(x, len(done))
            done.append(len(done))
        except fa.FptError:
            pass
    x.synchronize()
    for i in done[:2]:
        render(y, i); y.synchronize()
    if y_init is not None:
        y._check(y_init(y))
    for i in done[2:]:
        render(y, i); y.synchronize()
    same_frame(x, y, "passes %s" % done, channels)
    rearm(x)
    for i in range(len(done), len(done) + 3):
        render(x, i)
        render(y, i); y.synchronize()
    x.synchronize()
    same_frame(x, y, "after the deferral was set up again", channels)
    return done


@pytest.mark.gpu
def test_deferred_storage_psfpt_then_pt_set_batch(cornell_glossy, table):
    """3a. fpt_psfpt_set_deferred(8), then fpt_pt_set_batch(2): the store loses the PSFPT's extras.  Before the owner the deferral stayed on with a maximum of 2 and
    the refusal came from the flush inside a later call, after a pass whose render call had returned success was dropped"""
    kw = dict(psf_options=fa.default_psf_options())
    x, y = make(cornell_glossy, table, **kw), make(cornell_glossy, table, **kw)
    x.psf_set_deferred(8)
    done = _deferred_detour(x, y, lambda r, i: r.psf_render(i), lambda r: r.L.fpt_pt_set_batch(r.ctx, C.c_uint32(2), C.byref(r.view)), "fpt_pt_set_batch",
                            lambda r: r.psf_set_deferred(2))
    print("3a: passes whose render call returned success:", done)
    cx, cy = x.psf_cells(), y.psf_cells()
    assert len(cx["keys"]) > 0
    for k in cx:
        assert np.array_equal(cx[k], cy[k]), k
    x.close(); y.close()


@pytest.mark.gpu
def test_deferred_storage_bpt_then_pt_init(cornell_glossy, table):
    """3b. a BPT deferral, then fpt_pt_init: the BPT's storage is not touched; an init leaves no deferral.  The six colour channels, as tests/test_bpt.py compares a
    BPT batch with passes one by one (the luminance channel of a BPT batch is not the sequential one bit for bit)"""
    kw = dict(bpt_options=fa.default_bpt_options(L))
    x, y = make(cornell_glossy, table, **kw), make(cornell_glossy, table, **kw)
    x.bpt_set_deferred(4)
    done = _deferred_detour(x, y, lambda r, i: r.bpt_render(i), pt_init, "fpt_pt_init", lambda r: r.bpt_set_deferred(4), y_init=pt_init, channels=range(6))
    assert done == [0, 1, 2, 3]
    x.close(); y.close()


@pytest.mark.gpu
def test_deferred_storage_pt_then_psfpt_init(cornell_glossy, table):
    """3c. a PT deferral, then fpt_psfpt_init: the store is re-shaped for one pass; an init leaves no deferral, and the PT renders on one pass at a time"""
    x, y = make(cornell_glossy, table), make(cornell_glossy, table)
    x.set_deferred(4)
    done = _deferred_detour(x, y, lambda r, i: r.render_pass(i), psf_init, "fpt_psfpt_init", lambda r: r.set_deferred(4), y_init=psf_init)
    assert done == [0, 1, 2, 3]
    x.close(); y.close()


@pytest.mark.gpu
def test_timing_read_out_with_two_lanes(cornell_glossy, table):
    """4. the launch counts add up to the launch list; per bucket the time at least one launch was running is at most the launches' summed time, and so is slot 4
    against buckets 0, 1 and 2.  The only tolerance is float32 summation error: (number of launches) x 2^-23 x the sum"""
    r = make(cornell_glossy, table)
    r.set_lanes(2)
    r.render_pass(0, sync=True)
    r.set_profiling(2)
    r.render_pass(1); r.render_pass(2)
    listed = r.launch_list()
    t = r.collect_timings(); u = r.union_timings()
    names = ("primary_trace", "path_trace", "shadow_trace", "shade")
    counts = [t[k][1] for k in names]
    print("launches per bucket", counts, "listed", len(listed), "summed ms", [t[k][0] for k in names], "union ms", dict(u))
    assert sum(counts) == len(listed) == 2 * 2 * (1 + SHADE_PER_PASS + (L - 1))
    assert counts == [sum(1 for b, _ in listed if b == k) for k in range(4)]
    for k in names:
        ms, n = t[k]
        assert u[k] <= ms + n * 2.0 ** -23 * ms, k
    ms = sum(t[k][0] for k in names[:3]); n = sum(t[k][1] for k in names[:3])
    assert 0 < u["all_trace"] <= ms + n * 2.0 ** -23 * ms
    r.close()
