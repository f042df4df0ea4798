"""The Metropolis renderers' state has one owner (fpt_context::MltState, fpt_host.h): `-pssmlt` and `-mmlt` are two modes of it, an init of either leaves nothing of the
other, a refused init leaves nothing at all, and fpt_bpt_init invalidates it through the owner.

A context that switched modes is compared, bit for bit, with one that ran the init of its final mode twice: both have then initialised the bidirectional state twice
with the same max_path_length, and its shift table draws equal amounts from the context's random stream at every init (bpt_init, fpt_bpt_api.cpp), so anything of the
first mode that survived the switch -- a stale flag, frequency, technique count or array -- is the only thing that can tell the two apart.

Shape A of tests/test_pssmlt.py: CornellBox-JP 32 x 32, max_path_length 4, 256 chains, 4 spp (chain length 16)."""
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


def pssmlt_options(**kw):
    return fa.default_pssmlt_options(L, **dict(dict(n_chains=256, spp=4), **kw))


def mmlt_options():
    return fa.default_mmlt_options(L, n_chains=256, spp=4, mmlt_frequency=2, lens_techniques=1)


def make(cornell, table, **kw):
    return fa.Renderer(cornell, RES[0], RES[1], fa.default_options(L), table=table, **kw)


def init(r, name, o):
    return getattr(r.L, name)(r.ctx, C.byref(o), C.byref(r.view), r.samples_dir.encode(), None, C.c_uint32(0))


def pssmlt_init(r, o):
    r._check(init(r, "fpt_pssmlt_init", o))
    r.pssmlt_options = o


def mmlt_init(r, o):
    r._check(init(r, "fpt_mmlt_init", o))
    r.mmlt_options = o


def same_bits(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert np.array_equal(bits(a[k]), bits(b[k])), k


def lit(fb):
    return fb[api.FB_COMPOSITED_C][:, :3].max() > 0


@pytest.mark.gpu
def test_mmlt_then_pssmlt_is_pssmlt_twice(cornell, table):
    """a. `-mmlt` with the lens techniques and swaps, then fpt_pssmlt_init on the same context: frame, chain state and stats of a context that only ever was `-pssmlt`"""
    x = make(cornell, table, mmlt_options=mmlt_options())
    x.mmlt_render(0, sync=True)
    x.clear_framebuffer()
    pssmlt_init(x, pssmlt_options())
    x.pssmlt_render(0, sync=True)
    y = make(cornell, table, pssmlt_options=pssmlt_options())
    pssmlt_init(y, pssmlt_options())
    y.pssmlt_render(0, sync=True)
    fx, fy = x.framebuffer(), y.framebuffer()
    assert np.array_equal(bits(fx), bits(fy)) and lit(fx)
    same_bits(x.pssmlt_state(), y.pssmlt_state())
    assert x.pssmlt_stats() == y.pssmlt_stats()
    x.close(); y.close()


@pytest.mark.gpu
def test_pssmlt_then_mmlt_is_mmlt_twice(cornell, table):
    """b. the reverse switch, to `-mmlt` with the lens techniques and F = 2: frame, chain state with both pixel planes, stats and st_norms"""
    x = make(cornell, table, pssmlt_options=pssmlt_options())
    x.pssmlt_render(0, sync=True)
    x.clear_framebuffer()
    mmlt_init(x, mmlt_options())
    x.mmlt_render(0, sync=True)
    y = make(cornell, table, mmlt_options=mmlt_options())
    mmlt_init(y, mmlt_options())
    y.mmlt_render(0, sync=True)
    fx, fy = x.framebuffer(), y.framebuffer()
    assert np.array_equal(bits(fx), bits(fy)) and lit(fx)
    sx, sy = x.mmlt_state(), y.mmlt_state()
    assert "table_pixel" in sx and "path_pixel" in sx
    same_bits(sx, sy)
    assert x.mmlt_stats() == y.mmlt_stats() and x.mmlt_stats()["swaps_proposed"] > 0
    for a, b in zip(x.mmlt_st_norms(), y.mmlt_st_norms()):
        assert np.array_equal(bits(a), bits(b))
    assert x.mmlt_st_norms()[0][1].any()          # the lens techniques (t = 1) hold a share of the norms
    x.close(); y.close()


def readers(r):
    """every reader of the state by family: (entry point, call)"""
    return {"fpt_mmlt_init": [("fpt_mmlt_render", lambda: r.mmlt_render(0)), ("fpt_mmlt_get_stats", r.mmlt_stats), ("fpt_mmlt_download", r.mmlt_state),
                              ("fpt_mmlt_get_st_norms", r.mmlt_st_norms)],
            "fpt_pssmlt_init": [("fpt_pssmlt_render", lambda: r.pssmlt_render(0)), ("fpt_pssmlt_get_stats", r.pssmlt_stats), ("fpt_pssmlt_download", r.pssmlt_state)]}


def all_refuse(r, calls):
    for init_name, family in calls.items():
        for entry, call in family:
            with pytest.raises(fa.FptError) as e:
                call()
            assert entry in str(e.value) and init_name + " has not been called" in str(e.value), (entry, str(e.value))


@pytest.mark.gpu
def test_refused_init_leaves_nothing(cornell, table):
    """c. a refused fpt_pssmlt_init on a working `-mmlt` context: no reader of either family answers any more, each naming its own init; a valid init renders again"""
    r = make(cornell, table, mmlt_options=mmlt_options())
    r.mmlt_render(0, sync=True)
    assert init(r, "fpt_pssmlt_init", pssmlt_options(n_chains=0)) != 0
    msg = r.L.fpt_last_error(r.ctx).decode()
    assert "fpt_pssmlt_init" in msg and "n_chains" in msg, msg
    r.pssmlt_options = pssmlt_options()          # the sizes of the arrays pssmlt_state() offers
    all_refuse(r, readers(r))
    r.clear_framebuffer()
    mmlt_init(r, mmlt_options())
    r.mmlt_render(0, sync=True)
    assert lit(r.framebuffer())
    r.close()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["pssmlt", "mmlt"])
def test_bpt_init_invalidates_through_the_owner(cornell, table, mode):
    """d. fpt_bpt_init replaces the bidirectional state under the Metropolis state: render and download of both families refuse, and the BPT renders"""
    r = make(cornell, table, **({"pssmlt_options": pssmlt_options()} if mode == "pssmlt" else {"mmlt_options": mmlt_options()}))
    (r.pssmlt_render if mode == "pssmlt" else r.mmlt_render)(0, sync=True)
    r._check(init(r, "fpt_bpt_init", fa.default_bpt_options(L)))
    r.pssmlt_options = pssmlt_options(); r.mmlt_options = mmlt_options()
    calls = readers(r)
    all_refuse(r, {k: [c for c in v if c[0].endswith(("_render", "_download"))] for k, v in calls.items()})
    r.clear_framebuffer()
    r.bpt_render(0, sync=True)
    assert lit(r.framebuffer())
    r.close()
