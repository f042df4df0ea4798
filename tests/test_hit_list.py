"""The hit list of the path tracer's passes in flight: from bounce 1 on the traversal kernel writes no record per closest-hit ray but a LIST of the
hits -- record and source index, in the order the rays finish -- and the shading kernel runs one thread per list entry (fpt_trace_kernel.inc MODE_MIXED_LOG_DENSE,
fpt_pt.hip shade_kernel, ShadeParams::in_hit_src).  A miss leaves no entry.

The kernel alone, through fpt_debug_trace_hit_list (Renderer.debug_trace_hit_list), against a plain closest-hit launch (fpt_rt_trace, MODE_CLOSEST) of the same rays
with the queue's interval (1e-3, 1e8) in their .w words:
  * the list holds every hit of the plain launch exactly once, bit for bit, and its source index names the ray;
  * every other entry below the cursor is filler (t = -1, triId = -1, u = v = 0, source 0), and there are at most waves x chunk of them;
  * the cursor never exceeds the capacity, and nothing at or beyond the cursor was written (the arrays are pre-set to a pattern the kernel never writes).
Sizes: 1, 63, 64, 65 rays (one wave, partial and full, and one ray into a second wave); with the grid capped at three blocks -- twelve waves --
768 rays (the last size that runs on fixed batches: n <= waves x 64), 769 (the first that draws tickets) and 20000 (each wave draws tickets, refills and, with some 750
hits per wave and more, takes several chunks of the list).  Rays: a mix of hits and misses; every ray a hit (the Cornell box with its front closed, rays from inside); every
ray a miss (the list stays empty: cursor 0).  Both intersectors.

The renders: a frame of passes in flight must equal the same passes rendered one by one -- the route without a list, one hit record per ray -- in every bit of all
eight channels (the pattern of tests/test_nee_log_direct.py).  50 x 30 pixels, five passes in flight: CornellBox-JP, the open-box stand-in (many misses), a lone floor
quad under nothing (every ray of bounce 1 misses, so bounce 1 is shaded from an empty list and the later launches run on empty queues), a pixel list, two render lanes
(130 x 65, where the lanes really split), two batches on one context, the watertight intersector; and 200 x 150 with 32 in flight, where the launches draw tickets.
None of this provokes a fault: every store of the kernel is guarded by the capacity, and the probe refuses a capacity below count + waves x chunk before it launches."""
import os

import numpy as np
import pytest

import fermat_amd as fa
from fermat_amd import scene

W, H, PATH_LENGTH, IN_FLIGHT = 50, 30, 6, 5
CAP_BLOCKS = 3                                  # 12 waves: 768 rays are the last static launch
N_MANY = 20000                                  # under that cap: some 1700 rays per wave
QUEUE_TMIN, QUEUE_TMAX = 1.0e-3, 1.0e8          # fpt_device.h QUEUE_SCATTER_*


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# the kernel alone

@pytest.fixture(scope="module")
def closed_cornell(tmp_path_factory):
    """CornellBox-JP with a wall across its open front"""
    base = scene.cornell_box("CornellBox-JP")
    lo, hi = np.asarray(base.bbox[0], np.float64), np.asarray(base.bbox[1], np.float64)
    d = str(tmp_path_factory.mktemp("closed"))
    with open(os.path.join(d, "front.mtl"), "w") as f:
        f.write("newmtl front\nKd 0.5 0.5 0.5\n")
    with open(os.path.join(d, "front.obj"), "w") as f:
        f.write("mtllib front.mtl\n")
        m = 0.05 * (hi - lo)
        for x, y in ((lo[0] - m[0], lo[1] - m[1]), (hi[0] + m[0], lo[1] - m[1]), (hi[0] + m[0], hi[1] + m[1]), (lo[0] - m[0], hi[1] + m[1])):
            f.write("v %.9g %.9g %.9g\n" % (x, y, hi[2]))
        f.write("vt 0.5 0.5\nvn 0 0 -1\ng front\nusemtl front\nf 1/1/1 2/1/1 3/1/1 4/1/1\n")
    cornell = os.path.join(scene.DATA_DIR, "scenes", "CornellBox")
    with open(os.path.join(d, "closed.fa"), "w") as f:
        f.write("LoadScene %s/CornellBox-JP.obj\nLoadScene front.obj\n" % cornell)
    s = scene.load_scene(os.path.join(d, "closed.fa"))
    s.camera = scene.load_camera(os.path.join(cornell, "camera-frontal.txt"))
    return s


def make_rays(scn, n, kind, seed=7):
    """`inside`: from points in the middle of the box in random directions; `away`: from outside the scene's ball, moving outwards; `mixed`: every second group of
    1..5 rays one or the other, so that the lanes of a wave finish at different times and a retire holds hits and misses"""
    rng = np.random.default_rng(seed)
    lo, hi = np.asarray(scn.bbox[0], np.float64), np.asarray(scn.bbox[1], np.float64)
    centre, ext = 0.5 * (lo + hi), float(np.max(hi - lo))
    d = rng.normal(size=(n, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
    inside = centre + (rng.random((n, 3)) - 0.5) * 0.3 * (hi - lo)
    outside = centre + 2.0 * ext * d
    away = {"inside": np.zeros(n, bool), "away": np.ones(n, bool), "mixed": (np.cumsum(rng.integers(0, 2, n)) % 2).astype(bool)}[kind]
    rays = np.zeros(n, fa.RAY_DTYPE)
    rays["origin"] = np.where(away[:, None], outside, inside).astype(np.float32)
    rays["dir"] = d.astype(np.float32)
    rays["mask"] = np.float32(QUEUE_TMIN).view(np.uint32)
    rays["tmax"] = QUEUE_TMAX
    return rays


def judge_list(out, plain, n, label):
    """the list of one launch against the plain launch's records"""
    cursor, waves, chunk, lst, src = out["cursor"], out["waves"], out["chunk"], out["list"], out["src"]
    capacity = len(lst)
    assert capacity == n + waves * chunk and chunk % 64 == 0 and chunk > 0, (label, capacity, waves, chunk)
    assert cursor <= capacity and cursor % chunk == 0, (label, cursor, capacity)
    # nothing at or beyond the cursor was written
    assert not bits(lst[cursor:]).any() and (src[cursor:] == 0xFFFFFFFF).all(), label + ": a store beyond the list's end"
    head, hsrc = lst[:cursor], src[:cursor]
    is_hit = (head["t"] > 0) & (head["triId"] >= 0)
    want = np.flatnonzero((plain["t"] > 0) & (plain["triId"] >= 0))
    # every hit of the plain launch exactly once, bit for bit
    got_src = hsrc[is_hit]
    assert (got_src < n).all(), label
    assert len(got_src) == len(want) and np.array_equal(np.sort(got_src), want), "%s: %d hits listed, %d in the plain launch" % (label, len(got_src), len(want))
    assert np.array_equal(bits(head[is_hit]), bits(plain[got_src])), label + ": a listed record differs from the plain launch's"
    # no miss other than filler
    filler = head[~is_hit]
    assert (bits(filler["t"]) == bits(np.float32([-1.0]))[0]).all() and (filler["triId"] == -1).all() and not bits(filler["u"]).any() and not bits(filler["v"]).any(), label
    assert (hsrc[~is_hit] == 0).all(), label
    assert len(filler) <= waves * chunk, (label, len(filler), waves, chunk)
    return len(want), len(filler)


@pytest.mark.gpu
@pytest.mark.parametrize("intersector", [fa.INTERSECTOR_MT, fa.INTERSECTOR_WATERTIGHT], ids=["mt", "wt"])
def test_the_list_holds_every_hit_once(closed_cornell, cornell, table, intersector):
    report = []
    for name, scn, kind in (("mixed", cornell, "mixed"), ("all hit", closed_cornell, "inside"), ("all miss", cornell, "away")):
        r = fa.Renderer(scn, 8, 8, fa.default_options(2), table=table)
        r.set_intersector(intersector); r.rebuild_geometry()
        assert r.intersector() == (intersector, intersector)
        rays = make_rays(scn, N_MANY, kind)
        plain_all = r.trace(rays)
        hit_all = (plain_all["t"] > 0) & (plain_all["triId"] >= 0)
        if kind == "inside":
            assert hit_all.all(), "the closed box leaks"
        elif kind == "away":
            assert not hit_all.any()
        else:
            assert 0.2 < hit_all.mean() < 0.8
        for cap, sizes in ((0, (1, 63, 64, 65)), (CAP_BLOCKS, (768, 769, N_MANY))):
            r.debug_set_trace_blocks(cap)
            for n in sizes:
                label = "%s, intersector %d, cap %d, %d rays" % (name, intersector, cap, n)
                out = r.debug_trace_hit_list(rays[:n])
                assert out["waves"] == 4 * (min(cap, (n + 255) // 256) if cap else (n + 255) // 256), label
                hits, filler = judge_list(out, plain_all[:n], n, label)
                if kind == "away":
                    assert out["cursor"] == 0, label          # nothing was drawn: the launches that follow run on an empty queue
                if cap and n == N_MANY and kind != "away":
                    assert hits > 2 * out["waves"] * out["chunk"], label          # several chunks per wave
                report.append((label, hits, filler, out["cursor"]))
        r.debug_set_trace_blocks(0)
        # a capacity below count + waves x chunk is refused before anything is launched
        with pytest.raises(fa.FptError, match="capacity"):
            r.debug_trace_hit_list(rays[:65], capacity=65)
        r.close()
    for line in report:
        print("%s: %d hits, %d filler entries, cursor %d" % line)


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# the renders

def assert_same_frame(got, want, pixels=None):
    for c in range(8):
        g, w = (got[c], want[c]) if pixels is None else (got[c][pixels], want[c][pixels])
        assert np.array_equal(bits(g), bits(w)), "channel %d: %d of %d words differ" % (c, int((bits(g) != bits(w)).sum()), bits(g).size)


def renderer(scn, table, res, pixels, intersector):
    r = fa.Renderer(scn, res[0], res[1], fa.default_options(PATH_LENGTH), table=table, pixels=pixels)
    if intersector != fa.INTERSECTOR_MT:
        r.set_intersector(intersector); r.rebuild_geometry()
    return r


def one_by_one(scn, table, n, res=(W, H), pixels=None, intersector=fa.INTERSECTOR_MT):
    r = renderer(scn, table, res, pixels, intersector)
    for i in range(n):
        r.render_pass(i)
    fb = r.framebuffer().copy()
    r.close()
    return fb


def in_flight(scn, table, batches, res=(W, H), pixels=None, lanes=1, intersector=fa.INTERSECTOR_MT, max_batch=IN_FLIGHT, stats=False):
    r = renderer(scn, table, res, pixels, intersector)
    r.set_batch(max_batch)
    if lanes > 1:
        r.set_lanes(lanes)
        assert r.lane_count() == lanes
    if stats:
        r.set_profiling(True)
    for first, n in batches:
        r.render_batch(first, n)
    fb = r.framebuffer().copy()
    st = r.stats() if stats else None
    r.close()
    return (fb, st) if stats else fb


@pytest.fixture(scope="module")
def floor_scene(tmp_path_factory):
    """a diffuse floor quad and, beside it in the same plane, an emissive quad (the renderer wants an emitter): nothing above them, so every scattered ray misses"""
    d = str(tmp_path_factory.mktemp("floor"))
    with open(os.path.join(d, "floor.mtl"), "w") as f:
        f.write("newmtl floor\nKd 0.6 0.5 0.4\nnewmtl lamp\nKd 0.1 0.1 0.1\nKe 5 5 5\n")
    with open(os.path.join(d, "floor.obj"), "w") as f:
        f.write("mtllib floor.mtl\n")
        for x, z in ((-1, -1), (1, -1), (1, 1), (-1, 1), (1.5, -0.5), (2.5, -0.5), (2.5, 0.5), (1.5, 0.5)):
            f.write("v %g 0 %g\n" % (x, z))
        f.write("vt 0.5 0.5\nvn 0 1 0\ng floor\nusemtl floor\nf 1/1/1 4/1/1 3/1/1 2/1/1\ng lamp\nusemtl lamp\nf 5/1/1 8/1/1 7/1/1 6/1/1\n")
    with open(os.path.join(d, "floor.fa"), "w") as f:
        f.write("LoadScene floor.obj\n")
    s = scene.load_scene(os.path.join(d, "floor.fa"))
    s.camera = scene.make_camera((0.3, 3.0, 0.4), (0.2, 0.0, 0.0), (0.0, 0.0, -1.0), 0.7)
    return s


@pytest.mark.gpu
def test_cornell_equals_one_by_one(cornell, table):
    want = one_by_one(cornell, table, IN_FLIGHT)
    assert want[5][:, :3].max() > 0.0
    assert_same_frame(in_flight(cornell, table, [(0, IN_FLIGHT)]), want)


@pytest.mark.gpu
def test_open_box_with_many_misses_equals_one_by_one(standin_small, table):
    want = one_by_one(standin_small, table, IN_FLIGHT)
    got, st = in_flight(standin_small, table, [(0, IN_FLIGHT)], stats=True)          # (profiling level 1: one lane, synchronous; the same kernels)
    assert st.n_bounces >= 3 and st.in_size[1] > 0
    assert_same_frame(got, want)


@pytest.mark.gpu
def test_lone_floor_where_every_scattered_ray_misses(floor_scene, table):
    want = one_by_one(floor_scene, table, IN_FLIGHT)
    assert want[1].any()                                         # the camera sees the floor: its albedo is in the frame
    got, st = in_flight(floor_scene, table, [(0, IN_FLIGHT)], stats=True)
    assert st.in_size[0] == W * H * IN_FLIGHT and st.in_size[1] > 0          # scattered rays were traced ...
    assert st.n_bounces == 2 or st.in_size[2] == 0                              # ... and none of them hit: bounce 1 queued nothing
    assert_same_frame(got, want)
    assert_same_frame(in_flight(floor_scene, table, [(0, IN_FLIGHT)]), want)   # and without the synchronous stats: every later launch runs on an empty queue


@pytest.mark.gpu
def test_pixel_list_equals_one_by_one(standin_small, table):
    px = fa.tile_pixel_lists(W, H, 2, tile=(W, 1))[1]
    want = one_by_one(standin_small, table, IN_FLIGHT, pixels=px)
    got = in_flight(standin_small, table, [(0, IN_FLIGHT)], pixels=px)
    assert_same_frame(got, want, pixels=px)
    assert not got[:, np.setdiff1d(np.arange(W * H), px), :].any()


@pytest.mark.gpu
def test_two_lanes_equal_one_by_one(standin_small, table):
    """8450 pixels: two lanes of 4225, each with its own list behind its share of the queue arrays"""
    res = (130, 65)
    want = one_by_one(standin_small, table, IN_FLIGHT, res=res)
    assert_same_frame(in_flight(standin_small, table, [(0, IN_FLIGHT)], res=res, lanes=2), want)


@pytest.mark.gpu
def test_two_batches_on_one_context(standin_small, table):
    want = one_by_one(standin_small, table, 2 * IN_FLIGHT)
    assert_same_frame(in_flight(standin_small, table, [(0, IN_FLIGHT), (IN_FLIGHT, IN_FLIGHT)]), want)


@pytest.mark.gpu
def test_watertight_equals_one_by_one(standin_small, table):
    want = one_by_one(standin_small, table, IN_FLIGHT, intersector=fa.INTERSECTOR_WATERTIGHT)
    assert_same_frame(in_flight(standin_small, table, [(0, IN_FLIGHT)], intersector=fa.INTERSECTOR_WATERTIGHT), want)


@pytest.mark.gpu
def test_a_launch_that_draws_tickets_equals_one_by_one(standin_small, table):
    """200 x 150 x 32 in flight = 960 000 paths: the scattered and shadow rays of bounce 1 outnumber waves x 64 of the persistent grid, so the launch hands its rays out
    by tickets and its waves take many chunks of the list"""
    res, n = (200, 150), 32
    want = one_by_one(standin_small, table, n, res=res)
    assert_same_frame(in_flight(standin_small, table, [(0, n)], res=res, max_batch=n), want)
