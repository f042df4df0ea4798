"""The storage behind passes in flight (fpt_host.h WavefrontStore, the BPT's array list): what a set-up call sized is what a render may use, a
re-shape clears what it must, and fpt_bytes_per_path_in_flight is the sum of the arrays.  Every refusal here is a host-side check before any launch."""
import numpy as np
import pytest

import fermat_amd as fa
from fermat_amd import scene

W, H = 64, 48


def _same_frame(got, want, what):
    assert np.isfinite(got).all(), what
    for c in range(len(want)):
        assert np.array_equal(got[c].view(np.uint32), want[c].view(np.uint32)), (what, c)
    assert want[5][:, :3].mean() > 1e-3, what


def _same_cells(got, want):
    assert len(want["keys"]) > 0
    assert np.array_equal(got["keys"], want["keys"]) and np.array_equal(got["counts"], want["counts"]) and np.array_equal(got["sums"], want["sums"])


@pytest.mark.gpu
def test_gpu_pt_reshape_under_the_psfpt_is_refused_until_set_up_again(table, cornell_glossy):
    """The PT and the PSFPT share the store: fpt_pt_set_batch re-shapes it without the PSFPT's extras, the PSFPT's batch is then refused with the call to
    repeat, and after that call it renders what a fresh renderer renders, frame and cache bit for bit."""
    mk = lambda: fa.Renderer(cornell_glossy, W, H, fa.default_options(5), table=table, psf_options=fa.default_psf_options())      # noqa: E731
    r = mk()
    r.psf_set_batch(3)
    r.set_batch(3)
    with pytest.raises(fa.FptError, match="fpt_psfpt_set_batch"):
        r.psf_render_batch(0, 3, sync=True)
    r.psf_set_batch(3)
    r.psf_render_batch(0, 3, sync=True)
    fresh = mk()
    fresh.psf_set_batch(3)
    fresh.psf_render_batch(0, 3, sync=True)
    _same_cells(r.psf_cells(), fresh.psf_cells())
    _same_frame(r.framebuffer(), fresh.framebuffer(), "psfpt after a re-shape")
    r.close(); fresh.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["pt", "psfpt", "bpt"])
def test_gpu_more_passes_than_the_storage_holds_are_refused(table, cornell_glossy, kind):
    """set_batch(2), then a batch of 3 is refused (naming the set-up call); a batch of 2 then renders what a fresh renderer's does."""
    L = 4
    kw = dict(pt={}, psfpt=dict(psf_options=fa.default_psf_options()), bpt=dict(bpt_options=fa.default_bpt_options(L)))[kind]
    pre = dict(pt="", psfpt="psf_", bpt="bpt_")[kind]
    mk = lambda: fa.Renderer(cornell_glossy, W, H, fa.default_options(L), table=table, **kw)      # noqa: E731
    r, fresh = mk(), mk()
    for x in (r, fresh):
        getattr(x, pre + "set_batch")(2)
    with pytest.raises(fa.FptError, match=dict(pt="fpt_pt_set_batch", psfpt="fpt_psfpt_set_batch", bpt="fpt_bpt_set_batch")[kind]):
        getattr(r, pre + "render_batch")(0, 3, sync=True)
    for x in (r, fresh):
        getattr(x, pre + "render_batch")(0, 2, sync=True)
    _same_frame(r.framebuffer(), fresh.framebuffer(), kind)
    if kind == "psfpt":
        _same_cells(r.psf_cells(), fresh.psf_cells())
    r.close(); fresh.close()


@pytest.mark.gpu
@pytest.mark.parametrize("res,lanes", [((64, 48), 1), ((128, 96), 2)])      # two lanes need 4096 pixels each
def test_gpu_pt_shrinking_and_growing_the_batch_keeps_the_frame(table, cornell_glossy, res, lanes):
    """Batches of 4, 2 and 4 passes with a re-size of the store between them leave the frame of ten sequential passes, bit for bit: a re-size clears the planes and
    the log's fill bits, and the resolve blocks that name the store's buffers are uploaded again."""
    mk = lambda: fa.Renderer(cornell_glossy, res[0], res[1], fa.default_options(4), table=table)      # noqa: E731
    seq = mk()
    for i in range(10):
        seq.render_pass(i, sync=True)
    r = mk()
    if lanes > 1:
        r.set_lanes(lanes)
        assert r.lane_count() == lanes
    first = 0
    for n in (4, 2, 4):
        r.set_batch(n)
        r.render_batch(first, n, sync=True)
        first += n
    _same_frame(r.framebuffer(), seq.framebuffer(), "4 + 2 + 4 passes, %d lane(s)" % lanes)
    seq.close(); r.close()


# ---- bytes per path in flight: every array by hand, from the element types in fpt_host.h (QueueStorage, ShadowStorage, WavefrontStore, BptState), fpt_device.h
# (ContribLog) and fpt_bpt.h (BptQueue, LightVertexRecord, BptLog).  float4 = 16 B, float2 / uint2 = 8, uint32 = 4, uint8 = 1, int64 = 8
def _pt_terms(L, psf):
    """no directional lights (the Cornell boxes have none): their shadow queue and log cells take nothing per path"""
    t = dict(path_queue_rays=2 * (2 * 16), path_queue_hits=2 * 16, path_queue_weights=2 * 16, path_queue_cones=2 * 8,
             shadow_rays=2 * 16, shadow_w_d=16, shadow_w_g=16,
             albedo_diffuse_plane=16, albedo_specular_plane=16,
             log_emission=L * 16, log_mesh_light=L * 2 * 16, log_fill_bits=4 * (((4 if psf else 3) * L + 31) // 32))
    if psf:
        t.update(path_queue_cache_info=2 * 4, shadow_cache_info=4, shadow_hit_records=16, log_blend=L * 3 * 16,
                 ref_pixels=(L + 1) * 4, ref_cache=(L + 1) * 4, ref_pass=(L + 1) * 4, ref_w_d=(L + 1) * 16, ref_w_g=(L + 1) * 16)
    return t


def _bpt_terms(L, sc):
    cells = L * (1 + (1 if sc else L))          # per bounce an emission cell + 1 (-sc 1) or L connection cells
    t = dict(queue_rays=2 * (2 * 16), queue_hits=2 * 16, queue_weights=2 * 16, queue_path_weights=2 * 16, queue_pixels=2 * 4, queue_channel=2 * 1,
             connection_rays=L * 2 * 16, connection_hits=L * 16, connection_weights=L * 16, connection_pixels=L * 4, connection_channel=L * 1, connection_ranges=8,
             light_vertex_positions=L * 16, light_vertex_records=L * 64, light_vertex_counts=4,
             splat_sums=3 * 8, albedo_diffuse_plane=16, albedo_specular_plane=16,
             log_values=cells * 16, log_channels=cells * 4, log_fill_bits=4 * ((cells + 31) // 32))
    if sc:
        t.update(flat_vertex_list=L * 4)          # its scan's block sums (one word per 4096 entries) and per-pass bounds are not per path
    return t


def test_hand_counts():
    """the terms add up as counted: the path tracer's at L = 4 is the closed formula the library had before the store, 2 x 72 + 64 + 32 + 4 x 48 + 4"""
    assert sum(_pt_terms(4, False).values()) == 2 * 72 + 64 + 32 + 4 * 48 + 4 == 436
    assert sum(_pt_terms(5, True).values()) == 1016
    assert sum(_bpt_terms(9, 0).values()) == 3391
    assert sum(_bpt_terms(4, 0).values()) == 1238 and sum(_bpt_terms(4, 1).values()) == 1014


@pytest.mark.gpu
@pytest.mark.parametrize("kind,L,sc", [("pt", 4, 0), ("psfpt", 5, 0), ("bpt", 4, 0), ("bpt", 4, 1)])
def test_gpu_bytes_per_path_in_flight_is_the_sum_of_the_arrays(table, cornell_glossy, kind, L, sc):
    kw = dict(pt={}, psfpt=dict(psf_options=fa.default_psf_options()), bpt=dict(bpt_options=fa.default_bpt_options(L, single_connection=sc)))[kind]
    r = fa.Renderer(cornell_glossy, W, H, fa.default_options(L), table=table, **kw)
    terms = _bpt_terms(L, sc) if kind == "bpt" else _pt_terms(L, kind == "psfpt")
    got = r.bytes_per_path_in_flight(dict(pt=0, psfpt=1, bpt=2)[kind])
    print("bytes per path in flight, %s L = %d sc = %d: %d (by hand %d)" % (kind, L, sc, got, sum(terms.values())))
    assert got == sum(terms.values()), terms
    if kind == "pt":
        assert r.bytes_per_path_in_flight(2) == sum(_bpt_terms(9, 0).values())          # no fpt_bpt_init: the default path length, -sc 0
    r.close()
