"""The bidirectional path tracer's state has one owner (fpt::BptState, fpt_host.h): an init replaces everything that describes a pass in progress, a refused init or
re-size leaves the old state as it was and usable, and an array the new shape does not use is released.

fpt_bpt_init draws its shift table from the context's random stream at every call, so a context that went through a detour is compared, bit for bit, with one that made
the same number of inits of the same max_path_length without it (as tests/test_mlt_owner.py does): whatever of the detour survived the init -- a pending marker, a
stale option, an array of the other mode -- is the only thing that can tell the two apart.

CornellBox-JP 32 x 32, max_path_length 4."""
import ctypes as C

import numpy as np
import pytest

import fermat_amd as fa
from fermat_amd import api

U32 = np.uint32
RES = (32, 32)
L = 4


def bits(a):
    return np.ascontiguousarray(a).view(U32)


def make(cornell, table, **bpt):
    return fa.Renderer(cornell, RES[0], RES[1], fa.default_options(L), table=table, bpt_options=fa.default_bpt_options(L, **bpt))


def bpt_init(r, o, d_pixels=None, n_local=None):
    """fpt_bpt_init's status; the whole frame unless a device pixel list is given"""
    px = None if d_pixels is None else C.c_void_p(d_pixels.data_ptr())
    return r.L.fpt_bpt_init(r.ctx, C.byref(o), C.byref(r.view), r.samples_dir.encode(), px, C.c_uint32(r.n_local if n_local is None else n_local))


def pssmlt_init(r):
    o = fa.default_pssmlt_options(L, n_chains=256, spp=4)
    r._check(r.L.fpt_pssmlt_init(r.ctx, C.byref(o), C.byref(r.view), r.samples_dir.encode(), None, C.c_uint32(0)))
    r.pssmlt_options = o


def last_error(r):
    return r.L.fpt_last_error(r.ctx).decode()


def lit(fb):
    return fb[api.FB_COMPOSITED_C][:, :3].max() > 0


def same_frame_and_lit(x, y):
    fx, fy = x.framebuffer(), y.framebuffer()
    assert np.array_equal(bits(fx), bits(fy)) and lit(fx)


@pytest.mark.gpu
def test_reinit_forgets_a_pending_light_phase(cornell, table):
    """a. -sc 1 with shared light vertices: a render call stops after the light sub-paths; an init then replaces the state, and the next call does not wait for an
    fpt_bpt_finish of a batch that no longer exists (the parent commit, by reading, refuses x's second render)"""
    o = dict(single_connection=1)
    x = make(cornell, table, **o)
    x.bpt_set_shared_light_vertices(True)
    x.bpt_render(0)
    x._check(bpt_init(x, fa.default_bpt_options(L, **o)))
    x.clear_framebuffer()
    x.bpt_render(0); x.bpt_finish(sync=True)
    y = make(cornell, table, **o)
    y._check(bpt_init(y, fa.default_bpt_options(L, **o)))
    y.bpt_set_shared_light_vertices(True)
    y.bpt_render(0); y.bpt_finish(sync=True)
    same_frame_and_lit(x, y)
    x.close(); y.close()


def deferred(cornell, table, first_render):
    r = make(cornell, table)
    splats = r.bpt_defer_splats()
    if first_render:
        r.bpt_render(0)          # leaves a batch whose splats wait for fpt_bpt_resolve_splats
    return r, splats


@pytest.mark.gpu
def test_reinit_forgets_unresolved_splats(cornell, table):
    """b. deferred splats: a pass is rendered and never resolved; an init replaces the state (the splat tensor is the test's own, which the library does not clear)"""
    frames = []
    for first_render in (True, False):
        r, splats = deferred(cornell, table, first_render)
        r._check(bpt_init(r, fa.default_bpt_options(L)))
        splats.zero_(); r.clear_framebuffer()
        r.bpt_render(0); r.bpt_resolve_splats()
        frames.append(r.framebuffer()); r.close()
    assert np.array_equal(bits(frames[0]), bits(frames[1])) and lit(frames[0])


@pytest.mark.gpu
def test_metropolis_init_on_a_state_with_a_pass_pending(cornell, table):
    """c. as b, but the init that replaces the state is fpt_pssmlt_init's: frame, chain state and stats of a context that never rendered the unresolved pass (the
    parent commit, by reading, refuses every render of x: "the bidirectional state is not the one the Metropolis renderer's init made")"""
    x, splats = deferred(cornell, table, True)
    pssmlt_init(x)
    splats.zero_(); x.clear_framebuffer()
    x.pssmlt_render(0, sync=True)
    y = make(cornell, table)
    pssmlt_init(y)
    y.pssmlt_render(0, sync=True)
    same_frame_and_lit(x, y)
    sx, sy = x.pssmlt_state(), y.pssmlt_state()
    assert sx.keys() == sy.keys()
    for k in sx:
        assert np.array_equal(bits(sx[k]), bits(sy[k])), k
    assert x.pssmlt_stats() == y.pssmlt_stats()
    x.close(); y.close()


@pytest.mark.gpu
def test_refused_calls_leave_the_old_state_usable(cornell, table):
    """d. three refusals between two passes -- max_path_length out of range; an empty pixel set behind a real device pixel list, with another path length; a batch
    whose light-vertex slots pass 32 bits -- change nothing: pass 1 renders on the state pass 0 ran on"""
    x, y = make(cornell, table), make(cornell, table)
    for r in (x, y):
        r.bpt_render(0, sync=True)
    bytes_before = x.bytes_per_path_in_flight(2)
    assert bpt_init(x, fa.default_bpt_options(16)) != 0 and "max_path_length out of range" in last_error(x)
    pixels = x._dev(np.arange(4, dtype=U32))
    assert bpt_init(x, fa.default_bpt_options(15), pixels, 0) != 0 and "empty pixel set" in last_error(x)
    assert x.L.fpt_bpt_set_batch(x.ctx, C.c_uint32(1 << 20)) != 0 and "must stay below 2^32" in last_error(x)          # 2^20 passes x 2^10 pixels x 4
    assert x.bytes_per_path_in_flight(2) == bytes_before == y.bytes_per_path_in_flight(2)
    for r in (x, y):
        r.bpt_render(1, sync=True)
    same_frame_and_lit(x, y)
    x.close(); y.close()


@pytest.mark.gpu
def test_sc1_then_sc0_is_sc0_twice(cornell, table):
    """e. an init under -sc 0 on a context that rendered under -sc 1 (the flat vertex list, its scan's block sums and bounds are released: BptState::each_array)"""
    x = make(cornell, table, single_connection=1)
    x.bpt_render(0, sync=True)
    x._check(bpt_init(x, fa.default_bpt_options(L)))
    x.clear_framebuffer()
    x.bpt_render(0, sync=True)
    y = make(cornell, table)
    y._check(bpt_init(y, fa.default_bpt_options(L)))
    y.bpt_render(0, sync=True)
    same_frame_and_lit(x, y)
    x.close(); y.close()


@pytest.mark.gpu
def test_metropolis_refusal_before_bpt_init_keeps_the_bidirectional_state(cornell, table):
    """f. A Metropolis init that throws AFTER bpt_init resets the bidirectional state (BptState::reset: fpt_bpt_render would answer "fpt_bpt_init has not been called");
    one that refuses BEFORE bpt_init -- n_chains = 0, the refusal of test_mlt_owner.py::test_refused_init_leaves_nothing -- never touched it.  The code does the second
    here: the state the `-mmlt` init made (its options, one pass in flight) still renders"""
    r = fa.Renderer(cornell, RES[0], RES[1], fa.default_options(L), table=table, mmlt_options=fa.default_mmlt_options(L, n_chains=256, spp=4, lens_techniques=1))
    o = fa.default_pssmlt_options(L, n_chains=0, spp=4)
    assert r.L.fpt_pssmlt_init(r.ctx, C.byref(o), C.byref(r.view), r.samples_dir.encode(), None, C.c_uint32(0)) != 0 and "n_chains" in last_error(r)
    with pytest.raises(fa.FptError) as e:
        r.mmlt_render(0)
    assert "fpt_mmlt_init has not been called" in str(e.value)
    r.bpt_render(0, sync=True)
    assert lit(r.framebuffer())
    r.close()
