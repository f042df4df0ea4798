"""The emitter tables built on the DEVICE from the device mesh (fpt_mesh_lights_init_device / fpt_mesh_lights_update_device, fpt_lights_device.hip) against the exact
judge: api.host_emitter_tables, the host builder with no GPU.  Every comparison is bitwise -- the VPLs, their CDF, the triangle CDF, the inverse areas -- and exact on
`norm`; frames rendered from device-built tables equal, in every channel and bit, the frames rendered from host-built ones."""
import copy
import ctypes as C

import numpy as np
import pytest

import fermat_amd as fa
from fermat_amd import scene

pytestmark = pytest.mark.gpu

TABLES = ("vpls", "vpl_cdf", "mesh_cdf", "mesh_inv_area")


def bit_equal(a, b):
    a = np.ascontiguousarray(a); b = np.ascontiguousarray(b)
    return a.nbytes == b.nbytes and a.tobytes() == b.tobytes()


def assert_tables_equal(got, want, what=""):
    for k in TABLES:
        assert len(got[k]) == len(want[k]), "%s %s: %d entries, the judge has %d" % (what, k, len(got[k]), len(want[k]))
        if not bit_equal(got[k], want[k]):
            g = np.ascontiguousarray(got[k]).view(np.uint32).reshape(len(got[k]), -1); w = np.ascontiguousarray(want[k]).view(np.uint32).reshape(len(want[k]), -1)
            bad = np.flatnonzero((g != w).any(1))
            raise AssertionError("%s %s: %d of %d entries differ from the judge's, the first at %d: %r != %r" % (what, k, len(bad), len(g), bad[0], got[k][bad[0]], want[k][bad[0]]))
    assert np.float32(got["norm"]).tobytes() == np.float32(want["norm"]).tobytes(), "%s norm: %r != %r" % (what, got["norm"], want["norm"])


def frames_equal(a, b):
    for c in range(8):
        assert bit_equal(a[c], b[c]), "channel %d differs" % c


@pytest.fixture(scope="module")
def cornell_renderer(table, cornell):
    r = fa.Renderer(cornell, 16, 12, fa.default_options(3), table=table)
    yield r
    r.close()


# 1 ---- CornellBox-JP: sizes around wave (64), workgroup (256) and sort-block edges; 70000 is past the host sort's switch to its radix sort at 65536; the planar
#        ceiling light gives the Morton codes an axis of NaNs
@pytest.mark.parametrize("instance", [0, 3])
@pytest.mark.parametrize("n_vpls", [1, 63, 64, 65, 255, 257, 6144, 70000])
def test_cornell_tables_equal_the_host_builders(cornell_renderer, cornell, n_vpls, instance):
    r = cornell_renderer
    r.init_emitters_device(n_vpls, instance)
    want = fa.api.host_emitter_tables(cornell, n_vpls, instance)
    assert len(want["vpls"]) == n_vpls
    assert_tables_equal(r.lights(), want, "n_vpls=%d instance=%d" % (n_vpls, instance))


# 2 ---- an emissive map: the static part's mip estimates, and the 20 draws a mapped triangle costs the stream with or without texture coordinates
@pytest.mark.parametrize("with_texture_data", [True, False])
def test_emissive_map(tmp_path, table, with_texture_data):
    from conftest import make_glow_panel_scene
    rng = np.random.default_rng(11)
    tex = rng.integers(0, 256, (24, 40, 3), dtype=np.uint8); tex[:, :13] //= 8
    s = make_glow_panel_scene(tmp_path, tex)
    assert s.texture_data is not None
    if not with_texture_data:
        s = copy.copy(s); s.texture_data = None
    n = 3000
    want = fa.api.host_emitter_tables(s, n)
    assert len(want["vpls"]) == n
    r = fa.Renderer(s, 16, 12, fa.default_options(3), table=table)
    r.init_emitters_device(n)
    assert_tables_equal(r.lights(), want)
    r.close()


# 3 ---- no emitters: a uniform triangle CDF, no VPLs, and a renderer initialised afterwards falls back to mesh NEE and renders black
def test_scene_without_emitters(table, cornell):
    s = copy.copy(cornell)
    s.materials = cornell.materials.copy(); s.materials["emissive"][:] = 0.0
    W, H = 24, 16
    r = fa.Renderer(s, W, H, fa.default_options(3), table=table)
    r.init_emitters_device()
    got = r.lights()
    nt = s.num_triangles
    assert len(got["vpls"]) == 0 and len(got["vpl_cdf"]) == 0
    assert bit_equal(got["mesh_cdf"], (np.arange(1, nt + 1, dtype=np.uint32).astype(np.float32) / np.float32(nt)).astype(np.float32))
    assert_tables_equal(got, fa.api.host_emitter_tables(s, W * H))
    assert r.L.fpt_pt_init(r.ctx, C.byref(r.options), C.byref(r.view), r.samples_dir.encode(), None, C.c_uint32(r.n_local)) == 0, r.L.fpt_last_error(r.ctx)
    for i in range(2):
        r.render_pass(i)
    fb = r.framebuffer()
    assert np.isfinite(fb).all() and not fb[5][:, :3].any()
    r.close()


# 4 ---- random soups
SOUP_MATERIALS = (2, 2, 3, 2, 3, 1, 2, 3)
ZERO_AREA_SEED, ALL_EMIT_SEED = 3, 5


def make_soup(seed):
    """50-3000 small triangles in the unit cube, 1-3 materials.  Material 0 of two or three does not emit, of the others a random non-empty subset does.  Even seeds
    end in a run of non-emitting triangles (the CDF's trailing fix-up), odd seeds in an emitter; ZERO_AREA_SEED holds a zero-area emissive triangle (inverse area inf,
    weight 0); ALL_EMIT_SEED has one material, which emits: no sparsity for the CDF's sum.  Returns (scene, emits per triangle, index of the zero-area triangle or -1)."""
    rng = np.random.default_rng(1000 + seed)
    nt = int(rng.integers(50, 3001))
    n_mats = SOUP_MATERIALS[seed]
    centre = rng.random((nt, 1, 3)); P = (centre + (rng.random((nt, 3, 3)) - 0.5) * 0.08).astype(np.float32)
    if n_mats == 1:
        emits = np.array([True])
    else:
        emits = np.zeros(n_mats, bool)
        emits[1:] = rng.random(n_mats - 1) < 0.5
        if not emits.any():
            emits[1 + int(rng.integers(0, n_mats - 1))] = True
    mat_idx = rng.integers(0, n_mats, nt).astype(np.int32)
    lit = np.flatnonzero(emits)
    if n_mats > 1 and seed % 2 == 0:
        mat_idx[nt - int(rng.integers(1, 41)):] = 0
        mat_idx[nt // 2] = lit[0]
    else:
        mat_idx[nt - 1] = lit[-1]
    zero = -1
    if seed == ZERO_AREA_SEED:
        zero = nt // 3
        mat_idx[zero] = lit[0]; P[zero, 1] = P[zero, 0]; P[zero, 2] = P[zero, 0]
    raw = scene.RawMesh()
    raw.positions = P.reshape(-1, 3)
    raw.v_idx = np.arange(3 * nt, dtype=np.int32).reshape(nt, 3); raw.n_idx = np.full((nt, 3), -1, np.int32); raw.t_idx = np.full((nt, 3), -1, np.int32)
    raw.mat_idx = mat_idx
    raw.materials = []
    for m in range(n_mats):
        p = scene.default_material_params()
        p.update(diffuse=[0.5, 0.4, 0.3], emissive=[float(x) for x in (rng.random(3) * 5.0 + 0.1)] if emits[m] else [0.0, 0.0, 0.0])
        raw.materials.append(p)
    s = scene.Scene(raw, scene.make_camera([0.5, 0.5, 3.0], [0.5, 0.5, 0.5], [0, 1, 0], 0.6))
    return s, emits[s.material_indices], zero


@pytest.mark.parametrize("seed", range(8))
def test_random_soups(table, seed):
    s, lit, zero = make_soup(seed)
    nt = s.num_triangles
    assert 50 <= nt <= 3000 and len(lit) == nt and lit.any()
    n = 1000 + 371 * seed
    want = fa.api.host_emitter_tables(s, n)
    assert len(want["vpls"]) == n, "the host judge builds no table for this seed"
    # the seed is what its description says
    if seed == ALL_EMIT_SEED:
        assert lit.all()
    elif seed % 2 == 0:
        assert not lit[-1] and want["mesh_cdf"][-1] == 1.0 and want["mesh_cdf"][-2] == 1.0
    else:
        assert lit[-1]
    if seed == ZERO_AREA_SEED:
        assert lit[zero] and np.isinf(want["mesh_inv_area"][zero]) and want["mesh_cdf"][zero] == want["mesh_cdf"][zero - 1]
    r = fa.Renderer(s, 8, 8, fa.default_options(3), table=table)
    r.init_emitters_device(n)
    assert_tables_equal(r.lights(), want, "seed %d" % seed)
    r.close()


def moved_cornell(what):
    """CornellBox-JP with the ceiling light slid 0.2 to the left ("light") or the top of the short box pushed 0.25 to the right ("box"), as
    test_update_model_moves_an_object_between_passes moves them"""
    moved = scene.cornell_box("CornellBox-JP")
    v = moved.vertex_data
    if what == "box":
        box = np.isclose(v[:, 1], 0.6)
        assert 8 <= box.sum() <= 40 and len(np.unique(v[box, :3], axis=0)) == 4
        v[box, 0] += np.float32(0.25)
        touched = np.flatnonzero(box)
    else:
        emissive = np.array([np.any(np.asarray(m["emissive"][:3]) > 0) for m in moved.materials])
        touched = np.unique(moved.vertex_indices[emissive[moved.material_indices], :3])
        assert 3 <= len(touched) <= 64
        v[touched, 0] -= np.float32(0.2)
    moved.bbox = (v[:, :3].min(0), v[:, :3].max(0))
    return moved, touched


# 5 ---- the light moves: the tables follow the device mesh, and the frame is the one the host route gives
@pytest.mark.parametrize("nee_type", [1, 0])
def test_moved_light(table, nee_type):
    W, H = 40, 30
    s = scene.cornell_box("CornellBox-JP")
    moved, _ = moved_cornell("light")
    r = fa.Renderer(s, W, H, fa.default_options(4, nee_type), table=table)
    r.init_emitters_device()
    assert_tables_equal(r.lights(), fa.api.host_emitter_tables(s, W * H), "before the move")
    r.refit_geometry(moved.vertex_data)
    r.update_emitters_device()
    want = fa.api.host_emitter_tables(moved, W * H)
    assert_tables_equal(r.lights(), want, "after the move")
    for i in range(2):
        r.render_pass(i)
    fb = r.framebuffer()
    # the host route: the renderer's host view reads s2.vertex_data, which takes the moved vertices in place
    s2 = scene.cornell_box("CornellBox-JP")
    r2 = fa.Renderer(s2, W, H, fa.default_options(4, nee_type), table=table)
    s2.vertex_data[:] = moved.vertex_data
    r2.refit_geometry(s2.vertex_data)
    r2.reinit_emitters(W * H)
    assert_tables_equal(r2.lights(), want, "the host route")
    for i in range(2):
        r2.render_pass(i)
    fb2 = r2.framebuffer()
    assert fb[5][:, :3].max() > 0.5
    frames_equal(fb, fb2)
    r.close(); r2.close()


# 6 ---- only a non-emitter moves: every table is rebuilt all the same, the inverse areas of the moved triangles included
def test_moved_non_emitter(table):
    W, H = 24, 16
    s = scene.cornell_box("CornellBox-JP")
    moved, touched = moved_cornell("box")
    r = fa.Renderer(s, W, H, fa.default_options(3), table=table)
    r.init_emitters_device()
    r.refit_geometry(moved.vertex_data)
    r.update_emitters_device()
    want = fa.api.host_emitter_tables(moved, W * H)
    before = fa.api.host_emitter_tables(s, W * H)
    changed = np.flatnonzero(want["mesh_inv_area"].view(np.uint32) != before["mesh_inv_area"].view(np.uint32))
    assert len(changed) >= 2 and np.isin(moved.vertex_indices[changed, :3], touched).any(1).all()
    got = r.lights()
    assert_tables_equal(got, want)
    assert bit_equal(got["mesh_inv_area"][changed], want["mesh_inv_area"][changed])
    r.close()


# 7 ---- render parity at init, through the three renderers
@pytest.mark.parametrize("kind", ["pt", "bpt", "psfpt"])
def test_render_parity_at_init(table, cornell, kind):
    W, H, L = 40, 30, 4
    kw = dict(bpt_options=fa.default_bpt_options(L)) if kind == "bpt" else dict(psf_options=fa.default_psf_options()) if kind == "psfpt" else {}
    frames = []
    for device in (True, False):
        r = fa.Renderer(cornell, W, H, fa.default_options(L), table=table, **kw)
        if device:
            r.init_emitters_device()
        for i in range(2):
            (r.bpt_render if kind == "bpt" else r.psf_render if kind == "psfpt" else r.render_pass)(i)
        frames.append(r.framebuffer())
        r.close()
    assert frames[0][5][:, :3].max() > 0.5
    frames_equal(frames[0], frames[1])


# 8 ---- the C++ mirror: `-lights device` changes no bit of the frame of the update-model run with a moved light
DEVICE_BUILDER_LINE = "build_emitter_tables (device)"          # what the device builder prints under FPT_BVH_TIMERS


def mirror_run(table, extra_args, refit, in_place=False):
    """two passes, update_model with the light moved, two more passes through the C++ mirror; in_place: one more update_model(NULL) -- the route of a mesh edited
    on the device -- before the last passes.  Returns COMPOSITED_C."""
    L = fa.lib()
    L.fpt_host_context_create.restype = C.c_void_p
    L.fpt_host_last_error.restype = C.c_char_p

    class SceneArrays(C.Structure):
        _fields_ = [("mesh", fa.api.MeshView), ("textures", C.c_void_p), ("num_textures", C.c_uint32), ("dir_lights", C.c_void_p),
                    ("dir_lights_count", C.c_uint32), ("glossy_reflectance", C.c_void_p), ("camera", fa.api.Camera), ("samples_dir", C.c_char_p)]
    s = scene.cornell_box("CornellBox-JP")
    moved, _ = moved_cornell("light")
    sa = SceneArrays()
    sa.mesh.num_triangles = s.num_triangles; sa.mesh.num_vertices = s.num_vertices; sa.mesh.num_materials = len(s.materials)
    sa.mesh.vertex_indices = s.vertex_indices.ctypes.data; sa.mesh.vertex_data = s.vertex_data.ctypes.data
    sa.mesh.material_indices = s.material_indices.ctypes.data; sa.mesh.materials = s.materials.ctypes.data
    sa.mesh.tex_bias = (C.c_float * 2)(*s.tex_bias); sa.mesh.tex_scale = (C.c_float * 2)(*s.tex_scale)
    sa.glossy_reflectance = table.ctypes.data
    cam = s.camera
    sa.camera.eye = (C.c_float * 3)(*cam[0:3]); sa.camera.aim = (C.c_float * 3)(*cam[3:6]); sa.camera.up = (C.c_float * 3)(*cam[6:9])
    sa.camera.dx = (C.c_float * 3)(*cam[9:12]); sa.camera.fov = float(cam[12])
    sa.samples_dir = scene.DATA_DIR.encode()
    W, H = 64, 48
    args = [b"fermat", b"-pt", b"-r", b"%d" % W, b"%d" % H, b"-bounces", b"3"] + list(extra_args)
    argv = (C.c_char_p * len(args))(*args)
    h = L.fpt_host_context_create(C.c_int(len(args)), argv, C.byref(sa))
    assert h, L.fpt_host_last_error()
    h = C.c_void_p(h)
    for i in range(2):
        assert L.fpt_host_context_render(h, C.c_uint32(i)) == 0, L.fpt_host_last_error()
    assert L.fpt_host_context_update_model(h, C.c_void_p(moved.vertex_data.ctypes.data), C.c_int(refit)) == 0, L.fpt_host_last_error()
    if in_place:
        assert L.fpt_host_context_update_model(h, None, C.c_int(refit)) == 0, L.fpt_host_last_error()
    for i in range(2, 4):
        assert L.fpt_host_context_render(h, C.c_uint32(i)) == 0, L.fpt_host_last_error()
    img = np.zeros((W * H, 4), np.float32)
    assert L.fpt_host_context_download(h, C.c_uint32(5), C.c_void_p(img.ctypes.data)) == 0
    L.fpt_host_context_destroy(h)
    return img


@pytest.mark.parametrize("refit", [0, 1])
def test_mirror_with_lights_on_the_device(table, refit, monkeypatch, capfd):
    monkeypatch.delenv("FPT_LIGHTS_BUILD", raising=False)          # it overrides the flag: both runs would use one builder
    monkeypatch.setenv("FPT_BVH_TIMERS", "1")                     # the builders say who they are
    on_device = mirror_run(table, [b"-lights", b"device"], refit)
    assert capfd.readouterr().err.count(DEVICE_BUILDER_LINE) == 2, "init and update_scene each build on the device"
    on_host = mirror_run(table, [], refit)
    assert DEVICE_BUILDER_LINE not in capfd.readouterr().err
    assert on_device[:, :3].max() > 0.5
    assert bit_equal(on_device, on_host)


def test_mirror_environment_override_and_in_place_update(table, monkeypatch, capfd):
    """FPT_LIGHTS_BUILD overrides the flag both ways; update_model(NULL) -- vertices edited in place on the device -- rebuilds from the device mesh in device mode (no
    vertex array is read back for the builder) and gives the frame of the host mode, which reads them back"""
    monkeypatch.setenv("FPT_BVH_TIMERS", "1")
    monkeypatch.setenv("FPT_LIGHTS_BUILD", "device")
    on_device = mirror_run(table, [b"-lights", b"host"], 1, in_place=True)
    assert capfd.readouterr().err.count(DEVICE_BUILDER_LINE) == 3, "init, update_model(vertices) and update_model(NULL) each build on the device"
    monkeypatch.setenv("FPT_LIGHTS_BUILD", "host")
    on_host = mirror_run(table, [b"-lights", b"device"], 1, in_place=True)
    assert DEVICE_BUILDER_LINE not in capfd.readouterr().err
    assert on_device[:, :3].max() > 0.5
    assert bit_equal(on_device, on_host)


# 9 ---- errors leave the tables alone
def test_errors_leave_the_tables_alone(table, cornell):
    r = fa.Renderer(cornell, 16, 12, fa.default_options(3), table=table)
    before = r.lights()
    assert r.L.fpt_mesh_lights_update_device(r.ctx, C.byref(r.view.mesh)) != 0
    assert b"fpt_mesh_lights_init_device" in r.L.fpt_last_error(r.ctx)
    assert_tables_equal(r.lights(), before, "after update_device without init_device")
    r.init_emitters_device(500)
    built = r.lights()
    assert len(built["vpls"]) == 500
    assert r.L.fpt_mesh_lights_update_device(r.ctx, None) != 0
    assert b"null mesh" in r.L.fpt_last_error(r.ctx)
    assert r.L.fpt_mesh_lights_init_device(r.ctx, C.c_uint32(500), C.byref(r.h_mesh), C.byref(r._h_tex), None, C.c_void_p(r.d_tex_views.data_ptr()), C.c_uint32(0)) != 0
    assert b"null mesh" in r.L.fpt_last_error(r.ctx)
    assert_tables_equal(r.lights(), built, "after a null device mesh")
    r.update_emitters_device()
    assert_tables_equal(r.lights(), built, "rebuilt from the same vertices")
    r.close()
