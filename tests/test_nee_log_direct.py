"""The path tracer's passes in flight write a light sample into its cell of the contribution log from the shading kernel, and the traversal kernel only sets the
cell's mask bit when the shadow ray turns out unoccluded (fpt_pt.hip write_shadow_entry_logged, fpt_trace.hip MODE_MIXED_LOG / MODE_ANY_LOG).  One pass per call keeps
the older route -- the sample travels in the shadow queue and the traversal kernel adds it to the frame -- and is the judge here: the batched frame must equal the
same passes rendered one by one in every bit of all eight channels, .w included.

The frame is 50 x 30: 1500 pixels, no multiple of 64 or 256, so the last wave and the last block of every kernel are partial.  CornellBox-Glossy, 9-vertex paths, five
passes in flight.  A frame of this size is below the library's floor of 4096 pixels per render lane, so the two-lane case is run a second time on 130 x 65 (8450 pixels:
two lanes of 4225, again no multiple of 64), where the lanes really split.

The last test needs no GPU: it compiles the traversal kernel to a gfx950 listing, the way tests/test_trace_retire_isa.py does, and compares the two new instantiations
with MODE_MIXED in register count, scratch size and the number of global loads and stores."""
import copy
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import fermat_amd as fa
from fermat_amd import scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, PATH_LENGTH, IN_FLIGHT = 50, 30, 9, 5
COLOUR_CHANNELS = (0, 2, 4, 5)          # FPT_FB_DIFFUSE_C, SPECULAR_C, DIRECT_C, COMPOSITED_C: everything a light sample or an emission can reach


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def assert_same_frame(got, want, pixels=None):
    for c in range(8):
        g, w = (got[c], want[c]) if pixels is None else (got[c][pixels], want[c][pixels])
        assert np.array_equal(bits(g), bits(w)), "channel %d: %d of %d words differ" % (c, int((bits(g) != bits(w)).sum()), bits(g).size)


def one_by_one(scn, table, n, res=(W, H), pixels=None, snapshot_at=()):
    """passes 0 .. n-1 by n calls of one pass each (the route without the log); the frame after the last pass, and the frames after the passes of `snapshot_at`"""
    r = fa.Renderer(scn, res[0], res[1], fa.default_options(PATH_LENGTH), table=table, pixels=pixels)
    snaps = {}
    for i in range(n):
        r.render_pass(i)
        if i + 1 in snapshot_at:
            snaps[i + 1] = r.framebuffer().copy()
    fb = r.framebuffer().copy()
    r.close()
    return fb, snaps


def in_flight(scn, table, batches, res=(W, H), pixels=None, lanes=1):
    """the batches (first pass, number of passes) on one context, IN_FLIGHT passes in flight at the most"""
    r = fa.Renderer(scn, res[0], res[1], fa.default_options(PATH_LENGTH), table=table, pixels=pixels)
    r.set_batch(IN_FLIGHT)
    if lanes > 1:
        r.set_lanes(lanes)
    for first, n in batches:
        r.render_batch(first, n)
    fb = r.framebuffer().copy()
    r.close()
    return fb


@pytest.fixture(scope="module")
def lit_scene(cornell_glossy):
    """the Cornell glossy box with one directional light shining in through its open front: both kinds of light sample, each with its own shadow queue and log cells"""
    s = copy.copy(cornell_glossy)
    s.dir_lights = np.float32([[0.25, -0.35, -1.0, 3.0, 2.8, 2.4]])
    return s


@pytest.fixture(scope="module")
def lit_reference(lit_scene, table):
    """ten passes one by one, computed once: (frame after ten passes, frame after five)"""
    fb, snaps = one_by_one(lit_scene, table, 2 * IN_FLIGHT, snapshot_at=(IN_FLIGHT,))
    return fb, snaps[IN_FLIGHT]


@pytest.fixture(scope="module")
def enclosed_scene(tmp_path_factory):
    """CornellBox-Glossy with its emitter (the quad at y = 1.58, |x|, |z| < 0.25) shut into a closed box of opaque diffuse triangles: every mesh-light sample is occluded"""
    d = str(tmp_path_factory.mktemp("enclosed"))
    lo, hi = (-0.4, 1.45, -0.4), (0.4, 1.585, 0.35)
    with open(os.path.join(d, "lid.mtl"), "w") as f:
        f.write("newmtl lid\nKd 0.5 0.5 0.5\n")
    with open(os.path.join(d, "lid.obj"), "w") as f:
        f.write("mtllib lid.mtl\n")
        for k in range(8):
            f.write("v %g %g %g\n" % tuple((hi if (k >> a) & 1 else lo)[a] for a in range(3)))
        f.write("vt 0.5 0.5\n")
        for n in ((-1, 0, 0), (1, 0, 0), (0, -1, 0), (0, 1, 0), (0, 0, -1), (0, 0, 1)):
            f.write("vn %d %d %d\n" % n)
        f.write("g lid\nusemtl lid\n")
        for n, quad in enumerate(((0, 4, 6, 2), (1, 3, 7, 5), (0, 1, 5, 4), (2, 6, 7, 3), (0, 2, 3, 1), (4, 5, 7, 6))):
            f.write("f " + " ".join("%d/1/%d" % (v + 1, n + 1) for v in quad) + "\n")
    cornell = os.path.join(scene.DATA_DIR, "scenes", "CornellBox")
    with open(os.path.join(d, "enclosed.fa"), "w") as f:
        f.write("LoadScene %s/CornellBox-Glossy.obj\nLoadScene lid.obj\n" % cornell)
    s = scene.load_scene(os.path.join(d, "enclosed.fa"))
    s.camera = scene.load_camera(os.path.join(cornell, "camera-frontal.txt"))
    return s


@pytest.mark.gpu
def test_both_light_kinds_equal_one_by_one(lit_scene, lit_reference, table):
    """the mesh light's samples retire in the MIXED launch, the directional light's in a shadow-only launch, and so do the mesh light's of the last bounce"""
    want = lit_reference[1]
    assert want[5][:, :3].max() > 0.0
    assert_same_frame(in_flight(lit_scene, table, [(0, IN_FLIGHT)]), want)


@pytest.mark.gpu
def test_two_lanes_equal_one_by_one(lit_scene, lit_reference, table):
    assert_same_frame(in_flight(lit_scene, table, [(0, IN_FLIGHT)], lanes=2), lit_reference[1])


@pytest.mark.gpu
def test_two_lanes_that_really_split_equal_one_by_one(lit_scene, table):
    """8450 pixels: each of the two lanes has its own queues, counters and resolve blocks, and its view of the log starts at pixel 4225"""
    res = (130, 65)
    want, _ = one_by_one(lit_scene, table, IN_FLIGHT, res=res)
    r = fa.Renderer(lit_scene, res[0], res[1], fa.default_options(PATH_LENGTH), table=table)
    r.set_batch(IN_FLIGHT); r.set_lanes(2)
    r.render_batch(0, IN_FLIGHT)
    got = r.framebuffer().copy()
    r.close()
    assert_same_frame(got, want)


@pytest.mark.gpu
def test_every_second_row_equals_one_by_one(lit_scene, table):
    """a pixel list: the first pixel, the stride of the log's planes and the number of slots all differ from the frame's size"""
    px = fa.tile_pixel_lists(W, H, 2, tile=(W, 1))[1]
    assert len(px) == W * H // 2 and px[0] == W
    want, _ = one_by_one(lit_scene, table, IN_FLIGHT, pixels=px)
    got = in_flight(lit_scene, table, [(0, IN_FLIGHT)], pixels=px)
    assert_same_frame(got, want, pixels=px)
    untouched = np.setdiff1d(np.arange(W * H), px)
    assert not got[:, untouched, :].any()


@pytest.mark.gpu
def test_enclosed_emitter_adds_nothing(enclosed_scene, table):
    """every sample is written to its cell at shade time and none of them is unoccluded: a mask bit set at shade time, or a cell applied without its bit, shows as light"""
    want, _ = one_by_one(enclosed_scene, table, IN_FLIGHT)
    r = fa.Renderer(enclosed_scene, W, H, fa.default_options(PATH_LENGTH), table=table)
    r.set_batch(IN_FLIGHT)
    r.set_profiling(True)
    r.render_batch(0, IN_FLIGHT)
    st = r.stats()
    assert sum(st.shadow_size[:st.n_bounces]) > 0          # light samples were taken, and their shadow rays traced
    got = r.framebuffer().copy()
    r.close()
    assert_same_frame(got, want)
    for c in COLOUR_CHANNELS:
        assert not bits(got[c]).any(), "channel %d" % c
    assert got[1].any()                                      # (the frame is not empty: the albedo of what the camera sees)


@pytest.mark.gpu
def test_two_batches_on_one_context(lit_scene, lit_reference, table):
    """passes 0-4, then 5-9: the cells the first batch wrote for occluded samples are still in the log when the second runs, and must stay out of the frame"""
    assert_same_frame(in_flight(lit_scene, table, [(0, IN_FLIGHT), (IN_FLIGHT, IN_FLIGHT)]), lit_reference[0])


# ---- the two instantiations in the gfx950 listing (no GPU needed) ----
STD = "-O3 -std=c++17 -fPIC -ffp-contract=off -fno-fast-math -fhip-fp32-correctly-rounded-divide-sqrt -fno-slp-vectorize".split()      # fermat_amd/csrc/Makefile
MODE_MIXED, MODE_MIXED_LOG, MODE_ANY_LOG = 3, 9, 10
OVF_BYTES = (48 - 8) * 8 + 16          # uint2 ovf[OVF_STACK] and the 16 bytes the compiler puts in front of it (tests/test_trace_retire_isa.py)


@pytest.fixture(scope="module")
def listing(tmp_path_factory):
    if shutil.which("hipcc") is None:
        pytest.skip("no hipcc: the traversal kernel cannot be compiled to a listing here")
    out = tmp_path_factory.mktemp("isa") / "fpt_trace.s"
    subprocess.check_call(["hipcc", "--offload-arch=gfx950"] + STD + ["-S", "--cuda-device-only", os.path.join(ROOT, "fermat_amd", "csrc", "fpt_trace.hip"), "-o", str(out)],
                          stderr=subprocess.DEVNULL, timeout=600)
    return out.read_text()


def kernel_facts(text, mode):
    """(metadata {key: int}, global loads, global stores) of trace_kernel<mode, false>"""
    tag = "trace_kernelILi%dELb0E" % mode
    for f in re.split(r"\n(?=_Z[^\n]*:\s*; @)", text):
        m = re.match(r"(_Z\S+):", f)
        if m and tag in m.group(1):
            name = m.group(1)
            ins = [l.split()[0] for l in f.split(".Lfunc_end")[0].split("\n") if re.match(r"\s+[a-z]", l)]
            block = [b for b in text.split("  - .agpr_count:") if ".name:           %s\n" % name in b or ".name: %s\n" % name in b]
            assert len(block) == 1, name
            md = {k: int(v) for k, v in re.findall(r"\.(\w+):\s+(\d+)\s*$", block[0], re.M)}
            return md, sum(x.startswith("global_load") for x in ins), sum(x.startswith("global_store") for x in ins)
    raise AssertionError("no %s in the listing" % tag)


def test_log_modes_are_leaner_than_mixed(listing):
    mixed, mixed_loads, mixed_stores = kernel_facts(listing, MODE_MIXED)
    for mode in (MODE_MIXED_LOG, MODE_ANY_LOG):
        md, _, _ = kernel_facts(listing, mode)
        assert md["vgpr_count"] <= mixed["vgpr_count"] and md["vgpr_spill_count"] == 0, (mode, md)
        assert md["private_segment_fixed_size"] == OVF_BYTES, (mode, md)
    _, loads, stores = kernel_facts(listing, MODE_MIXED_LOG)
    assert loads < mixed_loads and stores < mixed_stores, (loads, mixed_loads, stores, mixed_stores)
