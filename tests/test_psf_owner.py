"""The path-space filter's state has one owner (fpt::PsfState, fpt_host.h): an init replaces everything -- the state is unsharded, has one pass in flight and no
pending pass -- a refused init or set-up call leaves PSFPT, PT, store and random stream as they were and usable, what a mode no longer uses is released, and a
store re-shaped under a pending sharded pass forgets that pass.

Every fpt_pt_init draws its shift table from the context's random stream, so a context that went through a detour is compared, bit for bit, with one that made the
same number of inits of the same max_path_length without it (as tests/test_bpt_owner.py does): whatever of the detour survived -- a pending marker, a sharded flag, a
table of another size -- is the only thing that can tell the two apart.  None of the detours is sound on the commit before the owner: they were found
by reading and have not been run there.

CornellBox-Glossy 32 x 32, max_path_length 5, default PSF options (psf_temporal_reuse 64: the cache survives from pass 0 to pass 1)."""
import ctypes as C

import numpy as np
import pytest

import fermat_amd as fa
from fermat_amd import api

U32 = np.uint32
RES = (32, 32)
L = 5


def bits(a):
    return np.ascontiguousarray(a).view(U32)


def make(scn, table, psf=True):
    return fa.Renderer(scn, RES[0], RES[1], fa.default_options(L), table=table, psf_options=fa.default_psf_options() if psf else None)


def psf_init(r, length=L, psf=True, d_pixels=None, n_local=None):
    """fpt_psfpt_init's status (psf: True = the defaults, None = a null pointer, else the options); the whole frame unless a device pixel list is given"""
    o = fa.default_options(length)
    p = fa.default_psf_options() if psf is True else psf
    px = None if d_pixels is None else C.c_void_p(d_pixels.data_ptr())
    return r.L.fpt_psfpt_init(r.ctx, C.byref(o), None if p is None else C.byref(p), C.byref(r.view), r.samples_dir.encode(), px, C.c_uint32(r.n_local if n_local is None else n_local))


def pt_init(r, length=L, d_pixels=None, n_local=None):
    o = fa.default_options(length)
    px = None if d_pixels is None else C.c_void_p(d_pixels.data_ptr())
    return r.L.fpt_pt_init(r.ctx, C.byref(o), C.byref(r.view), r.samples_dir.encode(), px, C.c_uint32(r.n_local if n_local is None else n_local))


def last_error(r):
    return r.L.fpt_last_error(r.ctx).decode()


def sharded_pass(r, i):
    """a sharded pass in one context: the rank's own records are the only ones"""
    r.psf_render(i)
    r.psf_import_cells(*r.psf_export_cells())
    r.psf_finish(sync=True)


def lit(fb):
    return fb[api.FB_COMPOSITED_C][:, :3].max() > 0


def same_frame_and_cells(x, y):
    fx, fy = x.framebuffer(), y.framebuffer()
    assert np.array_equal(bits(fx), bits(fy)) and lit(fx)
    cx, cy = x.psf_cells(), y.psf_cells()
    assert len(cx["keys"]) > 0
    for k in cx:
        assert np.array_equal(cx[k], cy[k]), k


@pytest.mark.gpu
def test_reinit_forgets_a_pending_sharded_pass(cornell_glossy, table):
    """a. a sharded pass is rendered and never finished; an init then replaces the state: nothing is pending, and the next render is an unsharded one that does not
    wait for the fpt_psfpt_finish of a pass that no longer exists"""
    x = make(cornell_glossy, table)
    x.psf_set_sharded(True)
    x.psf_render(0)
    x._check(psf_init(x))
    assert x.L.fpt_psfpt_finish(x.ctx, C.byref(x.view)) != 0 and "no sharded pass is pending" in last_error(x)
    x.clear_framebuffer()
    x.psf_render(0, sync=True)
    y = make(cornell_glossy, table)
    y._check(psf_init(y))
    y.psf_render(0, sync=True)
    same_frame_and_cells(x, y)
    x.close(); y.close()


@pytest.mark.gpu
def test_reinit_after_a_shrunken_sharded_table(cornell_glossy, table):
    """b. a 2^10-slot table, sharded (pass table, list and records of 2^10 entries); the init puts the 2^24-slot table back and releases the shard's arrays, and
    fpt_psfpt_set_sharded sizes them anew for it"""
    x = make(cornell_glossy, table)
    x.psf_debug_set_table_log2(10)
    x.psf_set_sharded(True)
    sharded_pass(x, 0)
    x._check(psf_init(x))
    x.psf_set_sharded(True)
    x.clear_framebuffer()
    sharded_pass(x, 0)
    y = make(cornell_glossy, table)
    y._check(psf_init(y))
    y.psf_set_sharded(True)
    sharded_pass(y, 0)
    same_frame_and_cells(x, y)
    x.close(); y.close()


@pytest.mark.gpu
def test_refused_calls_change_nothing(cornell_glossy, table):
    """c. six refusals between pass 0 and pass 1 -- of the PSF options, of the PT options, of the pixel set, of the batch, of the table's size -- change nothing: pass 1
    renders on the state, the PT set-up, the store and the random stream pass 0 ran on"""
    x, y = make(cornell_glossy, table), make(cornell_glossy, table)
    for r in (x, y):
        r.psf_render(0, sync=True)
    assert psf_init(x, psf=None) != 0 and "null options" in last_error(x)
    assert psf_init(x, psf=fa.default_psf_options(psf_temporal_reuse=0)) != 0 and "psf_temporal_reuse must be >= 1" in last_error(x)
    assert psf_init(x, length=32) != 0 and "max_path_length out of range" in last_error(x)
    pixels = x._dev(np.arange(4, dtype=U32))
    assert psf_init(x, length=7, d_pixels=pixels, n_local=0) != 0 and "empty pixel set" in last_error(x)
    assert x.L.fpt_psfpt_set_batch(x.ctx, C.c_uint32(1 << 22), C.byref(x.view)) != 0 and "must stay below 2^32" in last_error(x)          # 2^22 passes x 2^10 pixels
    assert x.L.fpt_psfpt_debug_set_table_log2(x.ctx, C.c_uint32(12)) != 0 and "before the first render" in last_error(x)
    for r in (x, y):
        r.psf_render(1, sync=True)
    same_frame_and_cells(x, y)
    x.close(); y.close()


@pytest.mark.gpu
def test_refused_pt_init_changes_nothing(cornell_glossy, table):
    """c, on a plain PT context with a batch of 2 set up: fpt_pt_init with an empty pixel list and another path length, between two batches"""
    x, y = make(cornell_glossy, table, psf=False), make(cornell_glossy, table, psf=False)
    for r in (x, y):
        r.set_batch(2)
        r.render_batch(0, 2, sync=True)
    pixels = x._dev(np.arange(4, dtype=U32))
    assert pt_init(x, length=7, d_pixels=pixels, n_local=0) != 0 and "empty pixel set" in last_error(x)
    for r in (x, y):
        r.render_batch(2, 2, sync=True)
    fx, fy = x.framebuffer(), y.framebuffer()
    assert np.array_equal(bits(fx), bits(fy)) and lit(fx)
    x.close(); y.close()


@pytest.mark.gpu
def test_store_reshaped_under_a_pending_pass(cornell_glossy, table):
    """d. a plain fpt_pt_init re-shapes the store -- the reference queue is gone -- under a sharded pass that waits for fpt_psfpt_finish: the finish is refused and
    launches nothing, the context stays usable, and an fpt_psfpt_init makes it a fresh one"""
    x = make(cornell_glossy, table)
    x.psf_set_sharded(True)
    x.psf_render(0)
    x._check(pt_init(x))
    assert x.L.fpt_psfpt_finish(x.ctx, C.byref(x.view)) != 0
    assert "fpt_psfpt_finish" in last_error(x)
    x.synchronize()
    x._check(psf_init(x))
    x.clear_framebuffer()
    x.psf_render(0, sync=True)
    y = make(cornell_glossy, table)
    y._check(pt_init(y))
    y._check(psf_init(y))
    y.psf_render(0, sync=True)
    same_frame_and_cells(x, y)
    x.close(); y.close()


@pytest.mark.gpu
def test_batch_then_init(cornell_glossy, table):
    """e. an init leaves one pass in flight (the batch's pass tables are released): a batch is refused until fpt_psfpt_set_batch has sized them again"""
    x = make(cornell_glossy, table)
    x.psf_set_batch(3)
    x.psf_render_batch(0, 3, sync=True)
    x._check(psf_init(x))
    with pytest.raises(fa.FptError) as e:
        x.psf_render_batch(0, 3)
    assert "fpt_psfpt_set_batch" in str(e.value)
    x.psf_set_batch(3)
    x.clear_framebuffer()
    x.psf_render_batch(0, 3, sync=True)
    y = make(cornell_glossy, table)
    y._check(psf_init(y))
    y.psf_set_batch(3)
    y.psf_render_batch(0, 3, sync=True)
    same_frame_and_cells(x, y)
    x.close(); y.close()
