"""ctypes binding of include/fermat_pt_hip.h and the torch-backed Renderer used by tests and bench.py."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

from . import scene as _scene

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None

RAY_DTYPE = np.dtype([("origin", "<f4", (3,)), ("mask", "<u4"), ("dir", "<f4", (3,)), ("tmax", "<f4")])
HIT_DTYPE = np.dtype([("t", "<f4"), ("triId", "<i4"), ("u", "<f4"), ("v", "<f4")])
VPL_DTYPE = np.dtype([("uv", "<f4", (2,)), ("prim_id", "<u4"), ("E", "<f4")])

FB_DIFFUSE_C, FB_DIFFUSE_A, FB_SPECULAR_C, FB_SPECULAR_A, FB_DIRECT_C, FB_COMPOSITED_C, FB_FILTERED_C, FB_LUMINANCE = range(8)


class FptError(RuntimeError):
    pass


def lib_path():
    """the product library; FPT_LIB_PATH selects a tuning variant built by tools/build_variant.sh (kernel experiments only)"""
    return os.environ.get("FPT_LIB_PATH") or os.path.join(_HERE, "libfermat_pt_hip.so")


def build_extension(verbose=False):
    """Compile every HIP source for gfx950 (hipcc cross-compiles without a GPU)."""
    cmd = ["make", "-C", os.path.join(_HERE, "csrc"), "-j8"]
    subprocess.check_call(cmd, stdout=None if verbose else subprocess.DEVNULL)
    return lib_path()


# ---- C structs (mirror include/fermat_pt_hip.h) ------------------------------------------------------------------------------
class TextureRef(C.Structure):
    _fields_ = [("texture", C.c_uint32), ("_pad", C.c_uint32), ("scaling", C.c_float * 2)]


class Texture(C.Structure):
    _fields_ = [("texels", C.c_void_p), ("res_x", C.c_uint32), ("res_y", C.c_uint32)]


class MeshView(C.Structure):
    _fields_ = [("num_triangles", C.c_int32), ("num_vertices", C.c_int32), ("num_materials", C.c_int32), ("_pad", C.c_int32),
                ("vertex_indices", C.c_void_p), ("vertex_data", C.c_void_p), ("texture_indices_comp", C.c_void_p),
                ("material_indices", C.c_void_p), ("materials", C.c_void_p), ("tex_bias", C.c_float * 2), ("tex_scale", C.c_float * 2),
                ("texture_data", C.c_void_p)]


class PsfOptions(C.Structure):
    """fpt_psf_options: PSFPTOptions beyond PTOptions (src/renderers/psfpt.h:39-78)"""
    _fields_ = [("psf_depth", C.c_uint32), ("psf_width", C.c_float), ("psf_min_dist", C.c_float), ("psf_max_prob", C.c_float),
                ("psf_temporal_reuse", C.c_uint32), ("firefly_filter", C.c_float)]


def default_psf_options(**kw):
    o = PsfOptions(1, 3.0, 0.1, 32.0, 64, 100.0)
    for k, v in kw.items():
        setattr(o, k, v)
    return o


class BptOptions(C.Structure):
    """fpt_bpt_options: BPTOptionsBase + rr + single_connection (src/bpt_options.h:42-66, src/renderers/bpt.h:47-72)"""
    _fields_ = [("max_path_length", C.c_uint32), ("direct_lighting_nee", C.c_uint32), ("direct_lighting_bsdf", C.c_uint32),
                ("indirect_lighting_nee", C.c_uint32), ("indirect_lighting_bsdf", C.c_uint32), ("visible_lights", C.c_uint32),
                ("use_vpls", C.c_uint32), ("rr", C.c_uint32), ("light_tracing", C.c_float), ("single_connection", C.c_uint32)]


class BptStats(C.Structure):
    _fields_ = [("n_bounces_light", C.c_uint32), ("n_bounces_eye", C.c_uint32), ("light_queue", C.c_uint32 * 32), ("eye_queue", C.c_uint32 * 32),
                ("shadow_eye", C.c_uint32 * 32), ("n_light_vertices", C.c_uint32), ("shadow_light_tracing", C.c_uint32)]


def default_bpt_options(max_path_length=6, **kw):
    o = BptOptions(max_path_length, 1, 1, 1, 1, 1, 0, 1, 1.0, 0)          # single_connection=0: all connections (the CLI default is the reference's -sc 1)
    for k, v in kw.items():
        setattr(o, k, v)
    return o


class PssmltOptions(C.Structure):
    """fpt_pssmlt_options: PSSMLTOptions (src/renderers/pssmlt.h) over the bidirectional base options"""
    _fields_ = [("bpt", BptOptions), ("n_chains", C.c_uint32), ("spp", C.c_uint32), ("light_perturbations", C.c_uint32), ("eye_perturbations", C.c_uint32),
                ("independent_samples", C.c_float), ("radius", C.c_float)]


class PssmltStats(C.Structure):
    _fields_ = [("image_brightness", C.c_float), ("pdf_norm", C.c_float), ("chain_length", C.c_uint32), ("n_chains", C.c_uint32),
                ("accepted", C.c_uint64), ("rejected", C.c_uint64)]


def default_pssmlt_options(max_path_length=6, **kw):
    """the reference's defaults: 64 K chains, 4 spp, both perturbations on, no independent samples, Cauchy radius 0.01.  Keywords name fields of the
    structure or of its bidirectional base options (light_tracing and single_connection are forced to 0 at init)"""
    o = PssmltOptions(default_bpt_options(max_path_length, light_tracing=0.0), 64 * 1024, 4, 1, 1, 0.0, 0.01)
    own = {f[0] for f in PssmltOptions._fields_}
    for k, v in kw.items():
        setattr(o if k in own else o.bpt, k, v)
    return o


class MmltOptions(C.Structure):
    """fpt_mmlt_options: the PSSMLT options plus the swap frequency (CMLTOptions::mmlt_frequency, src/renderers/cmlt.h) and the lens-techniques switch"""
    _fields_ = [("mlt", PssmltOptions), ("mmlt_frequency", C.c_uint32), ("lens_techniques", C.c_uint32)]


class MmltStats(C.Structure):
    _fields_ = [("image_brightness", C.c_float), ("pdf_norm", C.c_float), ("chain_length", C.c_uint32), ("n_chains", C.c_uint32),
                ("accepted", C.c_uint64), ("rejected", C.c_uint64), ("swaps_proposed", C.c_uint64), ("swaps_accepted", C.c_uint64), ("rays", C.c_uint64)]


def default_mmlt_options(max_path_length=6, mmlt_frequency=0, lens_techniques=0, **kw):
    """the multiplexed Metropolis renderer (the reference's `-cmlt -charted-swaps 0`): default_pssmlt_options' keywords, mmlt_frequency = F > 0 for a technique
    swap at every F-th chain step, and lens_techniques = 1 for the lens connections (s, 1), s in [2, L], beside the others (light tracing is then on)"""
    return MmltOptions(default_pssmlt_options(max_path_length, **kw), mmlt_frequency, lens_techniques)


def tech_word(s, t):
    """a chain's technique (s light vertices, t eye vertices) as the library keeps it: s | t << 8"""
    return np.asarray(s, np.uint32) | (np.asarray(t, np.uint32) << np.uint32(8))


class EawParams(C.Structure):
    _fields_ = [("phi_normal", C.c_float), ("phi_position", C.c_float), ("phi_color", C.c_float),
                ("E", C.c_float * 3), ("U", C.c_float * 3), ("V", C.c_float * 3), ("W", C.c_float * 3)]


class XblParams(C.Structure):
    _fields_ = [("phi_normal", C.c_float), ("phi_position", C.c_float), ("phi_color", C.c_float), ("taps", C.c_uint32),
                ("E", C.c_float * 3), ("U", C.c_float * 3), ("V", C.c_float * 3), ("W", C.c_float * 3)]


# ShadingMode (src/renderer_view.h:61-76) and FilterOp (src/filters.h:44-57)
BUILD_QUALITY, BUILD_FAST, BUILD_TRBVH = 0, 1, 2          # fpt_rt_set_build_mode / Renderer.set_build_mode
INTERSECTOR_MT, INTERSECTOR_WATERTIGHT = 0, 1             # fpt_rt_set_intersector / Renderer.set_intersector
SHADING_SHADED, SHADING_UV, SHADING_ALBEDO, SHADING_DIFFUSE_ALBEDO, SHADING_SPECULAR_ALBEDO = 0, 1, 4, 5, 6
SHADING_DIFFUSE_COLOR, SHADING_SPECULAR_COLOR, SHADING_DIRECT_LIGHTING, SHADING_FILTERED, SHADING_VARIANCE, SHADING_NORMAL = 7, 8, 9, 10, 11, 12
FILTER_OP_MODULATE_INPUT, FILTER_OP_DEMODULATE_INPUT, FILTER_OP_MODULATE_OUTPUT, FILTER_OP_DEMODULATE_OUTPUT, FILTER_OP_ADD_MODE, FILTER_OP_REPLACE_MODE = 1, 2, 4, 8, 16, 32


class Camera(C.Structure):
    _fields_ = [("eye", C.c_float * 3), ("aim", C.c_float * 3), ("up", C.c_float * 3), ("dx", C.c_float * 3), ("fov", C.c_float)]


class FramebufferView(C.Structure):
    _fields_ = [("channels", C.c_void_p * 8), ("gbuffer_geo", C.c_void_p), ("gbuffer_uv", C.c_void_p), ("gbuffer_tri", C.c_void_p), ("gbuffer_depth", C.c_void_p)]


class RenderingContextView(C.Structure):
    _fields_ = [("camera", Camera), ("dir_lights_count", C.c_uint32), ("d_dir_lights", C.c_void_p), ("mesh", MeshView),
                ("d_textures", C.c_void_p), ("num_textures", C.c_uint32), ("d_glossy_reflectance", C.c_void_p),
                ("res_x", C.c_uint32), ("res_y", C.c_uint32), ("aspect", C.c_float), ("exposure", C.c_float), ("gamma", C.c_float),
                ("fb", FramebufferView)]


class PTOptions(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in ("max_path_length", "direct_lighting", "direct_lighting_nee", "direct_lighting_bsdf",
                                          "indirect_lighting_nee", "indirect_lighting_bsdf", "visible_lights", "diffuse_scattering",
                                          "glossy_scattering", "indirect_glossy", "rr", "nee_type")]


class PTStats(C.Structure):
    _fields_ = [("primary_rt_ms", C.c_float), ("path_rt_ms", C.c_float), ("shadow_rt_ms", C.c_float), ("path_shade_ms", C.c_float),
                ("shadow_shade_ms", C.c_float), ("n_bounces", C.c_uint32), ("in_size", C.c_uint32 * 32), ("shadow_dir_size", C.c_uint32 * 32),
                ("shadow_size", C.c_uint32 * 32), ("shade_events", C.c_uint64), ("rays_traced", C.c_uint64), ("shadow_rays_traced", C.c_uint64)]


class TraceCounters(C.Structure):
    _fields_ = [("rays", C.c_uint64), ("nodes_visited", C.c_uint64), ("tris_tested", C.c_uint64)]


class BvhStats(C.Structure):
    """fpt_bvh_stats (include/fermat_pt_hip.h)"""
    _fields_ = [("n_nodes", C.c_uint32), ("n_records", C.c_uint32), ("depth", C.c_uint32), ("stack_need", C.c_uint32), ("slot_hist", C.c_uint32 * 9),
                ("n_inner_children", C.c_uint32), ("n_leaf_children", C.c_uint32), ("build_threads", C.c_uint32), ("avg_used_slots", C.c_float),
                ("sah_cost_binary", C.c_float), ("sah_cost_wide", C.c_float), ("seconds_binary", C.c_float), ("seconds_wide", C.c_float),
                ("seconds_optimise", C.c_float), ("inner_area_before", C.c_float), ("inner_area_after", C.c_float), ("optimise_iterations", C.c_uint32), ("depth_binary", C.c_uint32),
                ("seconds_refit", C.c_float)]

    def as_dict(self):
        return dict(nodes=self.n_nodes, records=self.n_records, depth=self.depth, stack_need=self.stack_need, slot_hist=list(self.slot_hist),
                    inner_children=self.n_inner_children, leaf_children=self.n_leaf_children, build_threads=self.build_threads,
                    avg_used_slots=round(self.avg_used_slots, 3), sah_cost_binary=round(self.sah_cost_binary, 3), sah_cost_wide=round(self.sah_cost_wide, 3),
                    seconds_binary=round(self.seconds_binary, 3), seconds_wide=round(self.seconds_wide, 3), seconds_optimise=round(self.seconds_optimise, 3),
                    optimise_iterations=self.optimise_iterations, inner_area_before=round(self.inner_area_before, 3), inner_area_after=round(self.inner_area_after, 3),
                    depth_binary=self.depth_binary, seconds_refit=round(self.seconds_refit, 3))


def default_options(max_path_length=6, nee_type=1):
    """PTOptions defaults (src/renderers/pathtracer.h:186-199)."""
    return PTOptions(max_path_length, 1, 1, 1, 1, 1, 1, 1, 1, 0, 1, nee_type)


# every entry point include/fermat_pt_hip.h declares (the not-gpu test checks the .so exports them all)
ENTRY_POINTS = ["fpt_create", "fpt_destroy", "fpt_last_error", "fpt_stream", "fpt_synchronize", "fpt_rt_create_geometry", "fpt_rt_trace",
                "fpt_rt_trace_shadow", "fpt_rt_trace_shadow_bits", "fpt_rt_trace_counted", "fpt_rt_bvh_info", "fpt_rt_bvh_stats", "fpt_sequence_setup",
                "fpt_sequence_set_instance", "fpt_sequence_download", "fpt_mesh_lights_init", "fpt_mesh_lights_download", "fpt_pt_init",
                "fpt_pt_render", "fpt_pt_set_batch", "fpt_pt_render_batch", "fpt_pt_get_stats", "fpt_pt_set_profiling", "fpt_pt_collect_timings", "fpt_pt_set_counting", "fpt_pt_get_trace_counters", "fpt_pt_set_capture", "fpt_pt_get_captured", "fpt_rescale_frame",
                "fpt_update_variances", "fpt_to_rgba", "fpt_to_rgba_mode", "fpt_filter_variance", "fpt_eaw", "fpt_filter", "fpt_debug_math", "fpt_debug_bsdf", "fpt_debug_vertex",
                "fpt_psfpt_init", "fpt_psfpt_render", "fpt_psfpt_download_cells", "fpt_psfpt_set_sharded", "fpt_psfpt_exchange_cells",
                "fpt_psfpt_export_cells", "fpt_psfpt_import_cells", "fpt_psfpt_finish", "fpt_psfpt_set_batch", "fpt_psfpt_render_batch", "fpt_psfpt_set_deferred",
                "fpt_bpt_init", "fpt_bpt_render", "fpt_bpt_set_batch", "fpt_bpt_render_batch", "fpt_bpt_set_deferred", "fpt_bpt_get_stats", "fpt_bpt_set_profiling", "fpt_bpt_download_light_vertices",
                "fpt_bpt_splat_buffer", "fpt_bpt_use_splat_buffer", "fpt_bpt_set_deferred_splats", "fpt_bpt_resolve_splats", "fpt_debug_build_bvh",
                "fpt_comm_unique_id", "fpt_comm_last_error", "fpt_comm_init", "fpt_comm_adopt", "fpt_comm_destroy", "fpt_comm_info", "fpt_gather_framebuffer",
                "fpt_bpt_allreduce_splats", "fpt_comm_selftest", "fpt_pt_last_union_ms", "fpt_pt_lane_count", "fpt_pt_set_lanes", "fpt_pt_set_deferred", "fpt_pt_flush", "fpt_pt_launch_list", "fpt_set_tile_lists", "fpt_gather_pack", "fpt_gather_unpack", "fpt_device_memory", "fpt_bytes_per_path_in_flight", "fpt_bpt_set_shared_light_vertices", "fpt_bpt_export_light_vertices", "fpt_bpt_import_light_vertices", "fpt_bpt_exchange_light_vertices", "fpt_bpt_finish",
                "fpt_multiply_frame", "fpt_clamp_frame", "fpt_sequence_device_view", "fpt_mesh_lights_device_view", "fpt_mesh_invalidate", "fpt_rt_refit_geometry", "fpt_debug_refit_bvh",
                "fpt_debug_build_emitter_tables", "fpt_clear_gbuffer", "fpt_rt_download_bvh", "fpt_mesh_lights_update", "fpt_rt_set_build_mode",
                "fpt_mesh_lights_init_device", "fpt_mesh_lights_update_device", "fpt_rt_set_intersector", "fpt_rt_intersector",
                "fpt_debug_psf", "fpt_psfpt_debug_set_table_log2", "fpt_psfpt_debug_download_refs", "fpt_debug_bpt", "fpt_debug_frame",
                "fpt_pssmlt_init", "fpt_pssmlt_render", "fpt_pssmlt_get_stats", "fpt_pssmlt_download", "fpt_pssmlt_debug_eval", "fpt_debug_mlt", "fpt_debug_device_build",
                "fpt_mmlt_init", "fpt_mmlt_render", "fpt_mmlt_get_stats", "fpt_mmlt_get_st_norms", "fpt_mmlt_download", "fpt_mmlt_debug_eval",
                "fpt_mmlt_download_pixels", "fpt_mmlt_debug_eval_pixels", "fpt_debug_bpt_splat_entries",
                "fpt_mlt_set_persistence", "fpt_mlt_restart_chains", "fpt_mlt_get_persistence",
                "fpt_mlt_set_chain_shard", "fpt_mlt_get_chain_shard", "fpt_mlt_finish",
                "fpt_xbl", "fpt_filter_xbl",
                "fpt_debug_set_trace_blocks", "fpt_debug_trace_tickets", "fpt_debug_trace_hit_list"]

# fpt_debug_device_build: the arrays of the last device build, by their `which` (name -> (which, dtype, columns)); rows: n triangles, n - 1 binary nodes or the wide nodes
LBVH_CELL_DTYPE = np.dtype([("c", "<f4", 7), ("k", "u1", 7), ("k8", "u1"), ("leaf", "u1"), ("count", "u1"), ("spare", "u1", 2)])
DEVICE_BUILD_ARRAYS = {"refs": (1, np.float32, 6), "bounds": (2, np.int32, 12), "keys": (3, np.uint64, 1), "vals": (4, np.uint32, 1), "left": (5, np.int32, 1),
                       "right": (6, np.int32, 1), "node_box": (7, np.float32, 6), "cells": (8, LBVH_CELL_DTYPE, 1), "need": (9, np.uint32, 1), "tcount": (10, np.uint32, 1),
                       "tcost": (11, np.float32, 1)}


def kernel_source_hash():
    """sha256 over the sources the traversal kernel and its tree are built from: what a PMC collection under profiles/ is stamped with (tools/summarize_pmc.py) and
    what bench.py compares before it prints counters next to a freshly measured rate -- counters of another kernel or another builder are not this run's (VERDICT r4 task 2c)"""
    import hashlib
    d = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc")
    h = hashlib.sha256()
    for name in ("fpt_trace.hip", "fpt_trace_kernel.inc", "fpt_trace_wt.hip", "fpt_trace_dense.hip", "fpt_pt.hip", "fpt_device.h", "fpt_kernels.h", "fpt_math.h", "fpt_shading.h", "fpt_psf.h", "fpt_bvh.h", "fpt_bvh.cpp", "fpt_build.hip", "fpt_build_lbvh.hip",
                 "fpt_cw8_slots.h", "Makefile", "fpt_bpt.h", "fpt_bpt_device.h", "fpt_bpt.hip", "fpt_mlt.h", "fpt_mlt.hip", "fpt_mlt_host.h", "fpt_mlt_api.cpp"):
        with open(os.path.join(d, name), "rb") as f:
            h.update(name.encode()); h.update(f.read())
    return h.hexdigest()[:16]


def lib():
    """Load libfermat_pt_hip.so; fails loudly when it has not been built (no fallback path exists)."""
    global _LIB
    if _LIB is None:
        p = lib_path()
        if not os.path.exists(p):
            raise FptError("libfermat_pt_hip.so is not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
                           "(or make -C fermat_amd/csrc); there is no CPU fallback")
        # This binding hands the library torch-owned device memory, and PyTorch-ROCm ships its own copy of the HIP runtime: load torch's first, so that one process
        # holds ONE runtime (the library loaded first, then torch, ended in "no ROCm-capable device is detected" at fpt_create on the GPU box)
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        L = C.CDLL(p)
        L.fpt_last_error.restype = C.c_char_p
        L.fpt_last_error.argtypes = [C.c_void_p]
        L.fpt_stream.restype = C.c_void_p
        L.fpt_stream.argtypes = [C.c_void_p]
        _LIB = L
    return _LIB


def tile_pixel_lists(res_x, res_y, world_size, tile=32):
    """Image-tile sharding: tile t (row-major over ceil(W/tw) x ceil(H/th)) belongs to rank t % world_size.
    `tile` is the tile edge, or (tw, th); (res_x, 1) shards by interleaved scanlines.  Returns one uint32 array of ABSOLUTE
    pixel indices per rank, tile-major (raster order inside a tile) so neighbouring paths stay coherent."""
    tw, th = (tile, tile) if np.isscalar(tile) else (int(tile[0]), int(tile[1]))
    tx = (res_x + tw - 1) // tw; ty = (res_y + th - 1) // th
    ys, xs = np.mgrid[0:res_y, 0:res_x]
    t = (ys // th) * tx + (xs // tw)
    pix = (ys * res_x + xs).astype(np.uint32)
    out = []
    for r in range(world_size):
        sel = (t % world_size) == r
        order = np.lexsort((pix[sel], t[sel]))            # by tile, then raster order inside the tile
        out.append(np.ascontiguousarray(pix[sel][order]))
    assert tx * ty >= 1
    return out


def host_emitter_tables(scn, n_vpls, instance=0):
    """the emitter tables fpt_mesh_lights_init builds, on the host alone (fpt_debug_build_emitter_tables: no GPU): dict(vpls, vpl_cdf, mesh_cdf, mesh_inv_area, norm)"""
    L = lib()
    m = MeshView()
    m.num_triangles = scn.num_triangles; m.num_vertices = scn.num_vertices; m.num_materials = len(scn.materials)
    m.vertex_indices = scn.vertex_indices.ctypes.data; m.vertex_data = scn.vertex_data.ctypes.data
    m.material_indices = scn.material_indices.ctypes.data; m.materials = scn.materials.ctypes.data
    m.texture_indices_comp = scn.texture_indices_comp.ctypes.data if scn.texture_indices_comp is not None else None
    m.texture_data = scn.texture_data.ctypes.data if scn.texture_data is not None else None
    m.tex_bias = (C.c_float * 2)(*scn.tex_bias); m.tex_scale = (C.c_float * 2)(*scn.tex_scale)
    keep = []
    h_tex = (Texture * max(1, len(scn.textures)))()
    for i, tx in enumerate(scn.textures):
        if tx is None:
            continue
        tx = np.ascontiguousarray(tx, np.float32); keep.append(tx)
        h_tex[i].texels = tx.ctypes.data; h_tex[i].res_x = tx.shape[1]; h_tex[i].res_y = tx.shape[0]
    nt = scn.num_triangles
    vpls = np.zeros(n_vpls, VPL_DTYPE); cdf = np.zeros(n_vpls, np.float32); mcdf = np.zeros(nt, np.float32); minv = np.zeros(nt, np.float32)
    norm = C.c_float(); n_out = C.c_uint32()
    if L.fpt_debug_build_emitter_tables(C.c_uint32(n_vpls), C.byref(m), C.byref(h_tex), C.c_uint32(instance), C.c_void_p(vpls.ctypes.data), C.c_void_p(cdf.ctypes.data),
                                        C.c_void_p(mcdf.ctypes.data), C.c_void_p(minv.ctypes.data), C.byref(norm), C.byref(n_out)) != 0:
        raise FptError(L.fpt_last_error(None).decode())
    return dict(vpls=vpls[:n_out.value], vpl_cdf=cdf[:n_out.value], mesh_cdf=mcdf, mesh_inv_area=minv, norm=norm.value)


class Renderer:
    """RenderingContext + PathTracer for one GPU: owns torch device tensors, calls the C-ABI with their pointers."""

    def __init__(self, scn: "_scene.Scene", res_x, res_y, options=None, device=0, table=None, samples_dir=None, pixels=None,
                 exposure=1.0, gamma=2.2, gbuffer=True, replay_context_sequence=True, bpt_options=None, psf_options=None, pssmlt_options=None, mmlt_options=None):
        import torch
        if not torch.cuda.is_available():
            raise FptError("no HIP device visible: fermat_amd has no CPU fallback")
        self.torch = torch
        self.L = lib()
        self.scene = scn
        self.res = (int(res_x), int(res_y))
        self.dev = torch.device("cuda", device)
        self.options = options or default_options()
        self.samples_dir = samples_dir or _scene.DATA_DIR
        if table is None:
            table = np.fromfile(os.path.join(_scene.DATA_DIR, "glossy_reflectance.dat"), np.float32)
        assert table.size == 32 ** 4
        self.table = np.ascontiguousarray(table, np.float32)
        ctx = C.c_void_p()
        if self.L.fpt_create(C.c_int(device), C.byref(ctx)) != 0:
            raise FptError(self.L.fpt_last_error(None).decode())
        self.ctx = ctx
        self._keep = []
        t = lambda a: self._dev(a)  # noqa: E731
        n = self.res[0] * self.res[1]
        # device scene
        self.d_vi = t(scn.vertex_indices); self.d_vd = t(scn.vertex_data); self.d_mi = t(scn.material_indices)
        self.d_mats = t(scn.materials.view(np.uint8).reshape(-1)); self.d_table = t(self.table)
        self.d_tc = t(scn.texture_indices_comp) if scn.texture_indices_comp is not None else None
        self.d_dl = t(scn.dir_lights.reshape(-1)) if len(scn.dir_lights) else None
        tex_views = (Texture * max(1, len(scn.textures)))()
        self._h_tex = (Texture * max(1, len(scn.textures)))()
        self.d_tex_data = []
        for i, tx in enumerate(scn.textures):
            if tx is None:
                continue
            tx = np.ascontiguousarray(tx, np.float32); self._keep.append(tx)
            d = t(tx.reshape(-1)); self.d_tex_data.append(d)
            tex_views[i].texels = d.data_ptr(); tex_views[i].res_x = tx.shape[1]; tex_views[i].res_y = tx.shape[0]
            self._h_tex[i].texels = tx.ctypes.data; self._h_tex[i].res_x = tx.shape[1]; self._h_tex[i].res_y = tx.shape[0]
        self.d_tex_views = t(np.frombuffer(bytes(tex_views), np.uint8).copy())
        # frame buffer
        self.fb = torch.zeros((8, n, 4), dtype=torch.float32, device=self.dev)
        self.gb_geo = torch.zeros((n, 4), dtype=torch.float32, device=self.dev) if gbuffer else None
        self.gb_uv = torch.zeros((n, 4), dtype=torch.float32, device=self.dev) if gbuffer else None
        self.gb_tri = torch.full((n,), -1, dtype=torch.int32, device=self.dev) if gbuffer else None
        self.gb_depth = torch.zeros((n,), dtype=torch.float32, device=self.dev) if gbuffer else None
        self.d_pixels = None
        self.n_local = n
        if pixels is not None:
            pixels = np.ascontiguousarray(pixels, np.uint32)
            self.d_pixels = t(pixels.view(np.int32)); self.n_local = len(pixels)
        self.h_pixels = pixels
        # views
        self.view = self._make_view(exposure, gamma)
        self.h_mesh = self._mesh_view(host=True)
        torch.cuda.synchronize(self.dev)
        # init in the reference's order: RTContext geometry, context sequence (72 dims), renderer
        self._check(self.L.fpt_rt_create_geometry(self.ctx, C.c_uint32(scn.num_triangles), C.c_void_p(self.d_vi.data_ptr()),
                                                  C.c_uint32(scn.num_vertices), C.c_void_p(self.d_vd.data_ptr())))
        sd = self.samples_dir.encode()
        if replay_context_sequence:
            self._check(self.L.fpt_sequence_setup(self.ctx, C.c_uint32(72), C.c_uint32(256), sd))
        self._check(self.L.fpt_mesh_lights_init(self.ctx, C.c_uint32(n), C.byref(self.h_mesh), C.byref(self._h_tex), C.c_uint32(0)))
        px = C.c_void_p(self.d_pixels.data_ptr()) if self.d_pixels is not None else None
        self.bpt_options = bpt_options
        self.psf_options = psf_options
        self.pssmlt_options = pssmlt_options
        self.mmlt_options = mmlt_options
        if mmlt_options is not None:
            # `-mmlt`: one bidirectional technique per Metropolis chain; initialises the bidirectional state itself
            self._check(self.L.fpt_mmlt_init(self.ctx, C.byref(mmlt_options), C.byref(self.view), sd, px, C.c_uint32(self.n_local)))
        elif pssmlt_options is not None:
            # `-pssmlt`: Metropolis chains over the bidirectional kernels; initialises the bidirectional state itself
            self._check(self.L.fpt_pssmlt_init(self.ctx, C.byref(pssmlt_options), C.byref(self.view), sd, px, C.c_uint32(self.n_local)))
        elif psf_options is not None:
            # `-psfpt`: the path tracer's loop with the path-space-filtering vertex processor
            self._check(self.L.fpt_psfpt_init(self.ctx, C.byref(self.options), C.byref(psf_options), C.byref(self.view), sd, px, C.c_uint32(self.n_local)))
        elif bpt_options is None:
            self._check(self.L.fpt_pt_init(self.ctx, C.byref(self.options), C.byref(self.view), sd, px, C.c_uint32(self.n_local)))
        else:
            # `-bpt`: the bidirectional renderer takes the path tracer's place (its sampler consumes the same rand() stream position)
            self._check(self.L.fpt_bpt_init(self.ctx, C.byref(bpt_options), C.byref(self.view), sd, px, C.c_uint32(self.n_local)))

    # -- helpers
    def _dev(self, a):
        a = np.ascontiguousarray(a)
        if a.dtype == np.uint32:
            a = a.view(np.int32)
        return self.torch.from_numpy(a).to(self.dev)

    def _check(self, status):
        if status != 0:
            raise FptError(self.L.fpt_last_error(self.ctx).decode())

    def _mesh_view(self, host):
        s = self.scene
        m = MeshView()
        m.num_triangles = s.num_triangles; m.num_vertices = s.num_vertices; m.num_materials = len(s.materials)
        if host:
            m.vertex_indices = s.vertex_indices.ctypes.data; m.vertex_data = s.vertex_data.ctypes.data
            m.material_indices = s.material_indices.ctypes.data; m.materials = s.materials.ctypes.data
            m.texture_indices_comp = s.texture_indices_comp.ctypes.data if s.texture_indices_comp is not None else None
            m.texture_data = s.texture_data.ctypes.data if s.texture_data is not None else None
        else:
            m.vertex_indices = self.d_vi.data_ptr(); m.vertex_data = self.d_vd.data_ptr()
            m.material_indices = self.d_mi.data_ptr(); m.materials = self.d_mats.data_ptr()
            m.texture_indices_comp = self.d_tc.data_ptr() if self.d_tc is not None else None
        m.tex_bias = (C.c_float * 2)(*s.tex_bias); m.tex_scale = (C.c_float * 2)(*s.tex_scale)
        return m

    def _make_view(self, exposure, gamma):
        s = self.scene
        v = RenderingContextView()
        cam = s.camera
        v.camera.eye = (C.c_float * 3)(*cam[0:3]); v.camera.aim = (C.c_float * 3)(*cam[3:6]); v.camera.up = (C.c_float * 3)(*cam[6:9])
        v.camera.dx = (C.c_float * 3)(*cam[9:12]); v.camera.fov = float(cam[12])
        v.dir_lights_count = len(s.dir_lights)
        v.d_dir_lights = self.d_dl.data_ptr() if self.d_dl is not None else None
        v.mesh = self._mesh_view(host=False)
        v.d_textures = self.d_tex_views.data_ptr(); v.num_textures = len(s.textures)
        v.d_glossy_reflectance = self.d_table.data_ptr()
        v.res_x, v.res_y = self.res
        v.aspect = np.float32(self.res[0]) / np.float32(self.res[1]); v.exposure = exposure; v.gamma = gamma
        for c in range(8):
            v.fb.channels[c] = self.fb[c].data_ptr()
        if self.gb_geo is not None:
            v.fb.gbuffer_geo = self.gb_geo.data_ptr(); v.fb.gbuffer_uv = self.gb_uv.data_ptr()
            v.fb.gbuffer_tri = self.gb_tri.data_ptr(); v.fb.gbuffer_depth = self.gb_depth.data_ptr()
        return v

    def close(self):
        if getattr(self, "ctx", None):
            self.L.fpt_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- rendering
    def render_pass(self, instance, sync=False):
        self._check(self.L.fpt_pt_render(self.ctx, C.c_uint32(instance), C.byref(self.view)))
        if sync:
            self.synchronize()

    # -- path-space filtering (Renderer(..., psf_options=default_psf_options()))
    def psf_render(self, instance, sync=False):
        self._check(self.L.fpt_psfpt_render(self.ctx, C.c_uint32(instance), C.byref(self.view)))
        if sync:
            self.synchronize()

    def psf_set_deferred(self, max_passes):
        """psf_render(i) calls are collected and rendered up to `max_passes` at a time (bit-identical cache and frame); flushed by synchronize() / any frame access"""
        self._check(self.L.fpt_psfpt_set_deferred(self.ctx, C.c_uint32(max_passes), C.byref(self.view)))

    # passes in flight (fpt_psfpt_set_batch / fpt_psfpt_render_batch): cache and frame bit-identical to sequential passes
    def psf_set_batch(self, max_passes):
        self._check(self.L.fpt_psfpt_set_batch(self.ctx, C.c_uint32(max_passes), C.byref(self.view)))

    def psf_render_batch(self, first_instance, n_passes, sync=False):
        self._check(self.L.fpt_psfpt_render_batch(self.ctx, C.c_uint32(first_instance), C.c_uint32(n_passes), C.byref(self.view)))
        if sync:
            self.synchronize()

    # tile sharding of the PSFPT (include/fermat_pt_hip.h): psf_render then stops before the blend; exchange the pass's cells, then psf_finish
    def psf_set_sharded(self, on=True):
        self._check(self.L.fpt_psfpt_set_sharded(self.ctx, C.c_int(1 if on else 0)))

    def psf_export_cells(self):
        """(device pointer, count) of this rank's records of the pending pass (40 B each: key, three fixed-point sums, count)"""
        ptr = C.c_void_p(); n = C.c_uint32(0)
        self._check(self.L.fpt_psfpt_export_cells(self.ctx, C.byref(ptr), C.byref(n)))
        return ptr.value or 0, n.value

    def psf_import_cells(self, ptr, n):
        self._check(self.L.fpt_psfpt_import_cells(self.ctx, C.c_void_p(ptr), C.c_uint32(n)))

    def psf_exchange_cells(self):
        """the exchange over the library's RCCL communicator (fermat_amd.distributed.comm_init) + the merge of every rank's records"""
        self._check(self.L.fpt_psfpt_exchange_cells(self.ctx))

    def psf_finish(self, sync=False):
        self._check(self.L.fpt_psfpt_finish(self.ctx, C.byref(self.view)))
        if sync:
            self.synchronize()

    def psf_debug_set_table_log2(self, log2_size):
        """tests of the cache under load: 2^log2_size slots (8..24) instead of 2^24; before the first render, psf_set_batch and psf_set_sharded"""
        self._check(self.L.fpt_psfpt_debug_set_table_log2(self.ctx, C.c_uint32(log2_size)))

    def psf_refs(self):
        """the reference queue of the last rendered pass, read only: per bounce 0..L-1 a dict of n, ref_pixels, ref_cache, ref_wd, ref_wg (in append order, which is
        not defined) and keys: the key of the slot each cache word names (~0 after a batch or a finished sharded pass, whose pass tables are gone)"""
        out = []
        for b in range(int(self.options.max_path_length)):
            n = C.c_uint32(0)
            self._check(self.L.fpt_psfpt_debug_download_refs(self.ctx, C.c_uint32(b), None, None, None, None, None, C.c_uint32(0), C.byref(n)))
            m = n.value
            d = dict(n=m, ref_pixels=np.zeros(m, np.uint32), ref_cache=np.zeros(m, np.uint32), ref_wd=np.zeros((m, 4), np.float32), ref_wg=np.zeros((m, 4), np.float32),
                     keys=np.zeros(m, np.uint64))
            if m:
                self._check(self.L.fpt_psfpt_debug_download_refs(self.ctx, C.c_uint32(b), *[C.c_void_p(d[k].ctypes.data) for k in ("ref_pixels", "ref_cache", "ref_wd", "ref_wg", "keys")],
                                                                 C.c_uint32(m), C.byref(n)))
            out.append(d)
        return out

    def psf_cells(self):
        """occupied cache cells sorted by key: keys, sample counts, 2^-32 fixed-point sums"""
        n = C.c_uint32(0)
        self._check(self.L.fpt_psfpt_download_cells(self.ctx, None, None, None, C.c_uint32(0), C.byref(n)))
        keys = np.zeros(n.value, np.uint64); counts = np.zeros(n.value, np.uint64); sums = np.zeros((n.value, 3), np.int64)
        if n.value:
            self._check(self.L.fpt_psfpt_download_cells(self.ctx, C.c_void_p(keys.ctypes.data), C.c_void_p(counts.ctypes.data), C.c_void_p(sums.ctypes.data), n, C.byref(n)))
        o = np.argsort(keys, kind="stable")
        return dict(keys=keys[o], counts=counts[o], sums=sums[o])

    # -- bidirectional path tracer (Renderer(..., bpt_options=default_bpt_options(L)))
    def bpt_render(self, instance, sync=False):
        self._check(self.L.fpt_bpt_render(self.ctx, C.c_uint32(instance), C.byref(self.view)))
        if sync:
            self.synchronize()

    def bpt_set_batch(self, max_passes):
        """size the BPT's queues, light-vertex store, splat sums and accumulation planes for `max_passes` passes in flight"""
        self._check(self.L.fpt_bpt_set_batch(self.ctx, C.c_uint32(max_passes)))
        self.bpt_max_batch = int(max_passes)

    def bpt_render_batch(self, first_instance, n_passes, sync=False):
        self._check(self.L.fpt_bpt_render_batch(self.ctx, C.c_uint32(first_instance), C.c_uint32(n_passes), C.byref(self.view)))
        if sync:
            self.synchronize()

    def bpt_set_deferred(self, max_passes):
        """bpt_render(i) calls are collected and rendered up to `max_passes` at a time (bit-identical frame); flushed by synchronize() / any frame access"""
        self._check(self.L.fpt_bpt_set_deferred(self.ctx, C.c_uint32(max_passes)))

    # -sc 1 under tile sharding with the same image for any number of ranks (include/fermat_pt_hip.h "shared light vertices")
    def bpt_set_shared_light_vertices(self, on=True):
        self._check(self.L.fpt_bpt_set_shared_light_vertices(self.ctx, C.c_int(1 if on else 0)))

    def bpt_export_light_vertices(self):
        """(device pointer, count) of this rank's 80-byte vertex records of the batch in flight"""
        p, n = C.c_void_p(), C.c_uint32()
        self._check(self.L.fpt_bpt_export_light_vertices(self.ctx, C.byref(p), C.byref(n)))
        return p.value, n.value

    def bpt_import_light_vertices(self, ptr, count):
        self._check(self.L.fpt_bpt_import_light_vertices(self.ctx, C.c_void_p(ptr), C.c_uint32(count)))

    def bpt_exchange_light_vertices(self):
        self._check(self.L.fpt_bpt_exchange_light_vertices(self.ctx))

    def bpt_finish(self, sync=False):
        self._check(self.L.fpt_bpt_finish(self.ctx, C.byref(self.view)))
        if sync:
            self.synchronize()

    def bpt_defer_splats(self):
        """tile-sharded runs: keep the light-tracing splat sums (int64, 3 per pixel per pass in flight) in a torch tensor so that the
        ranks can all-reduce them (fermat_amd.distributed.allreduce_splats) before bpt_resolve_splats folds them into the frame;
        call after bpt_set_batch"""
        n = self.res[0] * self.res[1] * getattr(self, "bpt_max_batch", 1)
        self.splats = self.torch.zeros((n, 3), dtype=self.torch.int64, device=self.dev)
        self.torch.cuda.synchronize(self.dev)
        self._check(self.L.fpt_bpt_use_splat_buffer(self.ctx, C.c_void_p(self.splats.data_ptr())))
        self._check(self.L.fpt_bpt_set_deferred_splats(self.ctx, C.c_int(1)))
        return self.splats

    def bpt_resolve_splats(self):
        self._check(self.L.fpt_bpt_resolve_splats(self.ctx, C.byref(self.view)))
        self.synchronize()

    def bpt_splat_entries(self):
        """(entries, splatted) of the light-tracing stage's queue after the last bpt_render: all camera connections queued, and those with an unoccluded shadow ray"""
        n = C.c_uint32(0); v = C.c_uint32(0)
        self._check(self.L.fpt_debug_bpt_splat_entries(self.ctx, C.byref(n), C.byref(v)))
        return int(n.value), int(v.value)

    def bpt_set_profiling(self, on):
        self._check(self.L.fpt_bpt_set_profiling(self.ctx, C.c_int(1 if on else 0)))

    def bpt_stats(self):
        st = BptStats()
        self._check(self.L.fpt_bpt_get_stats(self.ctx, C.byref(st)))
        return dict(light_queue=np.array(st.light_queue[:st.n_bounces_light], np.uint32), eye_queue=np.array(st.eye_queue[:st.n_bounces_eye], np.uint32),
                    shadow_eye=np.array(st.shadow_eye[:st.n_bounces_eye], np.uint32), n_light_vertices=int(st.n_light_vertices),
                    shadow_light_tracing=int(st.shadow_light_tracing))

    def bpt_light_vertices(self):
        n = self.res[0] * self.res[1]; nv = n * self.bpt_options.max_path_length
        pos = np.zeros((nv, 4), np.float32); inp = np.zeros((nv, 2), np.uint32); gb = np.zeros((nv, 4), np.uint32)
        w = np.zeros((nv, 2), np.float32); pid = np.zeros(nv, np.uint32); cnt = np.zeros(n, np.uint32)
        self._check(self.L.fpt_bpt_download_light_vertices(self.ctx, *[C.c_void_p(x.ctypes.data) for x in (pos, inp, gb, w, pid, cnt)]))
        return dict(pos=pos, input=inp, gbuffer=gb, weights=w, path_id=pid, counts=cnt)

    # -- primary-sample-space Metropolis renderer (Renderer(..., pssmlt_options=default_pssmlt_options(L)))
    def pssmlt_render(self, instance, sync=False):
        self._check(self.L.fpt_pssmlt_render(self.ctx, C.c_uint32(instance), C.byref(self.view)))
        if sync:
            self.synchronize()

    def pssmlt_stats(self):
        st = PssmltStats()
        self._check(self.L.fpt_pssmlt_get_stats(self.ctx, C.byref(st)))
        return dict(image_brightness=np.float32(st.image_brightness), pdf_norm=np.float32(st.pdf_norm), chain_length=int(st.chain_length), n_chains=int(st.n_chains),
                    accepted=int(st.accepted), rejected=int(st.rejected))

    def _pssmlt_dims(self):
        return (self.pssmlt_options.bpt.max_path_length + 1) * 3

    def pssmlt_state(self):
        """what the last pssmlt_render left: light_u / eye_u (dims, n_chains), path_value (n_chains, 4), path_pdf, rejections, seeds (n_chains), presample (n_pixels, 4).
        Under a chain shard (mlt_set_chain_shard) n_chains is the shard's n_local: its chains in slot order"""
        n = self._mlt_n_local(self.pssmlt_options.n_chains); d = self._pssmlt_dims(); npx = self.res[0] * self.res[1]
        out = dict(light_u=np.zeros((d, n), np.float32), eye_u=np.zeros((d, n), np.float32), path_value=np.zeros((n, 4), np.float32), path_pdf=np.zeros(n, np.float32),
                   rejections=np.zeros(n, np.uint32), seeds=np.zeros(n, np.uint32), presample=np.zeros((npx, 4), np.float32))
        self._check(self.L.fpt_pssmlt_download(self.ctx, *[C.c_void_p(out[k].ctypes.data) for k in ("light_u", "eye_u", "path_value", "path_pdf", "rejections", "seeds", "presample")]))
        return out

    def pssmlt_eval(self, light_u, eye_u):
        """the value (n, 4) of n coordinate sets, light_u / eye_u of shape (dims, n), through the chain-mode kernels with mutation Null"""
        light_u = np.ascontiguousarray(light_u, np.float32); eye_u = np.ascontiguousarray(eye_u, np.float32)
        d = self._pssmlt_dims()
        assert light_u.shape == eye_u.shape and light_u.shape[0] == d
        n = light_u.shape[1]
        out = np.zeros((n, 4), np.float32)
        self._check(self.L.fpt_pssmlt_debug_eval(self.ctx, C.byref(self.view), C.c_uint32(n), C.c_void_p(light_u.ctypes.data), C.c_void_p(eye_u.ctypes.data), C.c_void_p(out.ctypes.data)))
        return out

    # -- multiplexed Metropolis renderer (Renderer(..., mmlt_options=default_mmlt_options(L)))
    def mmlt_render(self, instance, sync=False):
        self._check(self.L.fpt_mmlt_render(self.ctx, C.c_uint32(instance), C.byref(self.view)))
        if sync:
            self.synchronize()

    def mmlt_stats(self):
        st = MmltStats()
        self._check(self.L.fpt_mmlt_get_stats(self.ctx, C.byref(st)))
        return dict(image_brightness=np.float32(st.image_brightness), pdf_norm=np.float32(st.pdf_norm), chain_length=int(st.chain_length), n_chains=int(st.n_chains),
                    accepted=int(st.accepted), rejected=int(st.rejected), swaps_proposed=int(st.swaps_proposed), swaps_accepted=int(st.swaps_accepted), rays=int(st.rays))

    def _mmlt_L(self):
        return int(self.mmlt_options.mlt.bpt.max_path_length)

    def mmlt_st_norms(self):
        """(st_norms, chains) of the last mmlt_render, both (L + 2, L + 2) arrays indexed [t, s] (the reference's s + t * (L + 2))"""
        w = self._mmlt_L() + 2
        norms = np.zeros((w, w), np.float32); chains = np.zeros((w, w), np.uint32)
        self._check(self.L.fpt_mmlt_get_st_norms(self.ctx, C.c_void_p(norms.ctypes.data), C.c_void_p(chains.ctypes.data)))
        return norms, chains

    def mmlt_state(self):
        """what the last mmlt_render left: light_u / eye_u (dims, n_chains), path_value (n_chains, 4), path_pdf, rejections, seeds (cells of the table), st (s | t << 8) per
        chain, and the technique table (n_techniques, n_pixels, 4).  With lens_techniques = 1 the table has the L - 1 lens techniques after the others, and the
        state also holds table_pixel (L - 1, n_pixels), the pixel of every lens cell's sample, and path_pixel (n_chains), the pixel of every chain's state (0xFFFFFFFF:
        none / the one of eye coordinates 3 and 4).  Under a chain shard (mlt_set_chain_shard) n_chains is the shard's n_local: its chains in slot order"""
        L = self._mmlt_L()
        n = self._mlt_n_local(self.mmlt_options.mlt.n_chains); d = (L + 1) * 3; npx = self.res[0] * self.res[1]
        lens = int(self.mmlt_options.lens_techniques) != 0
        out = dict(light_u=np.zeros((d, n), np.float32), eye_u=np.zeros((d, n), np.float32), path_value=np.zeros((n, 4), np.float32), path_pdf=np.zeros(n, np.float32),
                   rejections=np.zeros(n, np.uint32), seeds=np.zeros(n, np.uint32), st=np.zeros(n, np.uint32), table=np.zeros((L * (L + 1) // 2 + (L - 1 if lens else 0), npx, 4), np.float32))
        self._check(self.L.fpt_mmlt_download(self.ctx, *[C.c_void_p(out[k].ctypes.data) for k in ("light_u", "eye_u", "path_value", "path_pdf", "rejections", "seeds", "st", "table")]))
        if lens:
            out["table_pixel"] = np.full((L - 1, npx), 0xFFFFFFFF, np.uint32); out["path_pixel"] = np.full(n, 0xFFFFFFFF, np.uint32)
            self._check(self.L.fpt_mmlt_download_pixels(self.ctx, C.c_void_p(out["table_pixel"].ctypes.data), C.c_void_p(out["path_pixel"].ctypes.data)))
        return out

    def mmlt_eval(self, light_u, eye_u, st, with_rays=False, with_pixels=False):
        """the value (n, 4) of n coordinate sets (light_u / eye_u of shape (dims, n)), set i through technique st[i] = s | t << 8 alone, mutation Null; with_rays: also the
        number of rays the evaluation queued; with_pixels: (value, rays, pixel), pixel[i] where a t = 1 evaluation landed (0xFFFFFFFF otherwise)"""
        light_u = np.ascontiguousarray(light_u, np.float32); eye_u = np.ascontiguousarray(eye_u, np.float32); st = np.ascontiguousarray(st, np.uint32)
        d = (self._mmlt_L() + 1) * 3
        assert light_u.shape == eye_u.shape and light_u.shape[0] == d and st.shape == (light_u.shape[1],)
        n = light_u.shape[1]
        out = np.zeros((n, 4), np.float32); rays = C.c_uint64(0)
        if with_pixels:
            pixel = np.full(n, 0xFFFFFFFF, np.uint32)
            self._check(self.L.fpt_mmlt_debug_eval_pixels(self.ctx, C.byref(self.view), C.c_uint32(n), C.c_void_p(light_u.ctypes.data), C.c_void_p(eye_u.ctypes.data),
                                                          C.c_void_p(st.ctypes.data), C.c_void_p(out.ctypes.data), C.byref(rays), C.c_void_p(pixel.ctypes.data)))
            return out, int(rays.value), pixel
        self._check(self.L.fpt_mmlt_debug_eval(self.ctx, C.byref(self.view), C.c_uint32(n), C.c_void_p(light_u.ctypes.data), C.c_void_p(eye_u.ctypes.data), C.c_void_p(st.ctypes.data),
                                               C.c_void_p(out.ctypes.data), C.byref(rays)))
        return (out, int(rays.value)) if with_rays else out

    # -- chains that persist across render calls, either Metropolis renderer (fpt_mlt_set_persistence, include/fermat_pt_hip.h)
    def mlt_set_persistence(self, reseeding, startup_skips=0):
        """a render call reseeds when there are no live chains or instance % reseeding == 0 and continues the chains otherwise; the first startup_skips steps of a
        reseeding call deposit nothing.  Drops live chains"""
        self._check(self.L.fpt_mlt_set_persistence(self.ctx, C.c_uint32(reseeding), C.c_uint32(startup_skips)))

    def mlt_restart_chains(self):
        """drops live chains (after an edit the library cannot see: materials or textures changed in place on the device): the next render call reseeds"""
        self._check(self.L.fpt_mlt_restart_chains(self.ctx))

    def mlt_persistence(self):
        """dict(reseeding, startup_skips (as clamped), last_call_reseeded, calls_since_reseed)"""
        v = [C.c_uint32() for _ in range(4)]
        self._check(self.L.fpt_mlt_get_persistence(self.ctx, *[C.byref(x) for x in v]))
        return dict(zip(("reseeding", "startup_skips", "last_call_reseeded", "calls_since_reseed"), (int(x.value) for x in v)))

    # -- chain shards, either Metropolis renderer: the same frame on any number of GPUs (fpt_mlt_set_chain_shard, include/fermat_pt_hip.h)
    def mlt_set_chain_shard(self, rank, world):
        """this context runs the global chains rank + i * world, chain rank + i * world in slot i; with world > 1 a render call leaves its sums in the splat buffer and
        waits for mlt_finish.  Drops live chains; (0, 1) is the renderer without shards"""
        self._check(self.L.fpt_mlt_set_chain_shard(self.ctx, C.c_uint32(rank), C.c_uint32(world)))

    def mlt_chain_shard(self):
        """dict(rank, world, n_local, pending)"""
        v = [C.c_uint32() for _ in range(4)]
        self._check(self.L.fpt_mlt_get_chain_shard(self.ctx, *[C.byref(x) for x in v]))
        return dict(zip(("rank", "world", "n_local", "pending"), (int(x.value) for x in v)))

    def _mlt_n_local(self, n_chains):
        """the chains a download returns: the shard's; without a Metropolis state the options' n_chains, so that the download itself says what is missing"""
        n = C.c_uint32(0)
        return int(n.value) if self.L.fpt_mlt_get_chain_shard(self.ctx, None, None, C.byref(n), None) == 0 else int(n_chains)

    def mlt_splat_buffer(self):
        """keep the chains' splat sums (int64, 3 per pixel, 2^-32 fixed point) in a torch tensor, so that the ranks of a chain shard can sum them between a render call
        and mlt_finish (torch.distributed.all_reduce, or by hand between contexts on one GPU); returns it.  Call after the init, before the first render call"""
        self.splats = self.torch.zeros((self.res[0] * self.res[1], 3), dtype=self.torch.int64, device=self.dev)
        self.torch.cuda.synchronize(self.dev)
        self._check(self.L.fpt_bpt_use_splat_buffer(self.ctx, C.c_void_p(self.splats.data_ptr())))
        return self.splats

    def mlt_finish(self, sync=False):
        """the second half of a shard's render call: sums the ranks' splat sums and counters over the context's communicator (without one the caller has summed the
        buffers itself) and folds them into the frame"""
        self._check(self.L.fpt_mlt_finish(self.ctx, C.byref(self.view)))
        if sync:
            self.synchronize()

    def debug_mlt(self, op, arrays, params=(), n=None):
        """fpt_debug_mlt (layouts: include/fermat_pt_hip.h); arguments and result as debug_bpt's"""
        torch = self.torch
        hosts = [None if a is None else np.ascontiguousarray(a) for a in arrays]
        devs = [None if a is None else torch.from_numpy(a.view(np.uint8).reshape(-1).copy() if a.size else np.zeros(8, np.uint8)).to(self.dev) for a in hosts]
        n = len(hosts[0]) if n is None else int(n)
        ptrs = (C.c_void_p * max(1, len(devs)))(*[None if d is None else d.data_ptr() for d in devs])
        par = (C.c_uint32 * max(1, len(params)))(*[int(p) for p in params])
        torch.cuda.synchronize(self.dev)
        self._check(self.L.fpt_debug_mlt(self.ctx, C.c_int(op), C.c_uint32(n), par, C.c_uint32(len(params)), ptrs, C.c_uint32(len(devs))))
        return [None if a is None else d.cpu().numpy()[:a.nbytes].view(a.dtype).reshape(a.shape) for a, d in zip(hosts, devs)]

    def device_memory(self):
        """(free, total) bytes of the context's device"""
        f = C.c_uint64(0); t = C.c_uint64(0)
        self._check(self.L.fpt_device_memory(self.ctx, C.byref(f), C.byref(t)))
        return int(f.value), int(t.value)

    def bytes_per_path_in_flight(self, renderer=0):
        """bytes one path in flight takes in queues, albedo planes and contribution log (renderer 0 = pt, 1 = psfpt, 2 = bpt)"""
        b = C.c_uint64(0)
        self._check(self.L.fpt_bytes_per_path_in_flight(self.ctx, C.c_uint32(renderer), C.byref(self.view), C.byref(b)))
        return int(b.value)

    def set_batch(self, max_passes):
        """size queues/accumulation planes for up to `max_passes` passes in flight per render_batch call"""
        self._check(self.L.fpt_pt_set_batch(self.ctx, C.c_uint32(max_passes), C.byref(self.view)))
        self.max_batch = max_passes

    def render_batch(self, first_instance, n_passes, sync=False):
        self._check(self.L.fpt_pt_render_batch(self.ctx, C.c_uint32(first_instance), C.c_uint32(n_passes), C.byref(self.view)))
        if sync:
            self.synchronize()

    def set_deferred(self, max_passes):
        """render_pass(i) calls are collected and rendered up to `max_passes` at a time (bit-identical frames); flushed by synchronize() / any frame access"""
        self._check(self.L.fpt_pt_set_deferred(self.ctx, C.c_uint32(max_passes), C.byref(self.view)))
        self.max_batch = max(getattr(self, "max_batch", 1), max_passes)

    def flush(self):
        self._check(self.L.fpt_pt_flush(self.ctx))

    def synchronize(self):
        self._check(self.L.fpt_synchronize(self.ctx))

    def set_profiling(self, level):
        """0 off, 1/True = synchronous per-launch timing + queue sizes (tests), 2 = asynchronous event pairs (bench)"""
        self._check(self.L.fpt_pt_set_profiling(self.ctx, C.c_int(int(level))))

    def collect_timings(self):
        ms = (C.c_float * 5)(); n = (C.c_uint32 * 5)()
        self._check(self.L.fpt_pt_collect_timings(self.ctx, ms, n))
        names = ("primary_trace", "path_trace", "shadow_trace", "shade", "unused")
        return {k: (ms[i], n[i]) for i, k in enumerate(names)}

    def launch_list(self, cap=4096):
        """(bucket, ms) of the launches timed since the last collect_timings, in issue order (profiling level 2)"""
        b = (C.c_int * cap)(); ms = (C.c_float * cap)(); n = C.c_uint32(0)
        self._check(self.L.fpt_pt_launch_list(self.ctx, C.c_uint32(cap), b, ms, C.byref(n)))
        return [(int(b[i]), float(ms[i])) for i in range(n.value)]

    def union_timings(self):
        """per bucket, the time at least one launch of the bucket was running (valid after collect_timings)"""
        ms = (C.c_float * 5)()
        self._check(self.L.fpt_pt_last_union_ms(self.ctx, ms))
        names = ("primary_trace", "path_trace", "shadow_trace", "shade", "all_trace")
        return {k: ms[i] for i, k in enumerate(names)}

    def lane_count(self):
        return int(self.L.fpt_pt_lane_count(self.ctx))

    def set_lanes(self, n):
        """cut the pixel list into n contiguous ranges rendered by their own launch chains on their own streams (bit-identical frames)"""
        self._check(self.L.fpt_pt_set_lanes(self.ctx, C.c_uint32(n)))

    def set_counting(self, on):
        self._check(self.L.fpt_pt_set_counting(self.ctx, C.c_int(1 if on else 0)))

    def trace_counters(self):
        a, b = TraceCounters(), TraceCounters()
        self._check(self.L.fpt_pt_get_trace_counters(self.ctx, C.byref(a), C.byref(b)))
        return a, b

    def stats(self):
        st = PTStats()
        self._check(self.L.fpt_pt_get_stats(self.ctx, C.byref(st)))
        return st

    def set_capture(self, bounce):
        self._check(self.L.fpt_pt_set_capture(self.ctx, C.c_int(bounce)))

    def captured(self):
        n = C.c_uint32()
        self._check(self.L.fpt_pt_get_captured(self.ctx, C.byref(n), None, None, None, None, None))
        n = n.value
        rays = np.zeros(n, RAY_DTYPE); hits = np.zeros(n, HIT_DTYPE); w = np.zeros((n, 4), np.float32)
        pix = np.zeros(n, np.uint32); cones = np.zeros((n, 2), np.float32)
        if n:
            self._check(self.L.fpt_pt_get_captured(self.ctx, None, C.c_void_p(rays.ctypes.data), C.c_void_p(hits.ctypes.data), C.c_void_p(w.ctypes.data),
                                                   C.c_void_p(pix.ctypes.data), C.c_void_p(cones.ctypes.data)))
        return dict(rays=rays, hits=hits, weights=w, pixel_info=pix, cones=cones)

    def framebuffer(self):
        self.synchronize()
        return self.fb.cpu().numpy()

    def clear_framebuffer(self):
        """zero the frame buffer.  The library works on its own (non-blocking) HIP stream, torch on its current stream: both are
        synchronised here, so the clear can neither overtake the library's pending work nor be overtaken by its next launch"""
        self.synchronize()
        self.fb.zero_()
        self.torch.cuda.synchronize(self.dev)

    def to_rgba(self, mode=None):
        """to_rgba_kernel (src/renderer.cu:83-282); mode = a ShadingMode id (SHADING_*), None = kShaded through fpt_to_rgba"""
        out = self.torch.zeros((self.res[1], self.res[0], 4), dtype=self.torch.uint8, device=self.dev)
        self.torch.cuda.synchronize(self.dev)
        if mode is None:
            self._check(self.L.fpt_to_rgba(self.ctx, C.byref(self.view), C.c_void_p(out.data_ptr())))
        else:
            self._check(self.L.fpt_to_rgba_mode(self.ctx, C.byref(self.view), C.c_uint32(mode), C.c_void_p(out.data_ptr())))
        self.synchronize()
        return out.cpu().numpy()

    # -- post-process (kFiltered shading mode)
    def clear_gbuffer(self):
        """GBufferStorage::clear (src/framebuffer.h:178-185): 0xFF fill, i.e. every pixel starts as a miss"""
        for t in (self.gb_geo, self.gb_uv, self.gb_tri, self.gb_depth):
            if t is not None:
                t.view(self.torch.int32).fill_(-1)
        self.torch.cuda.synchronize(self.dev)

    def refit_geometry(self, vertex_data):
        """the mesh's vertices moved (same indices): upload them over the device mesh and refit the acceleration structure ON THE DEVICE (fpt_rt_refit_geometry)"""
        v = np.ascontiguousarray(vertex_data, np.float32)
        assert v.shape == tuple(self.d_vd.shape) or v.size == self.d_vd.numel()
        self.d_vd.copy_(self.torch.from_numpy(v).reshape(self.d_vd.shape).to(self.dev)); self.torch.cuda.synchronize(self.dev)
        self._check(self.L.fpt_rt_refit_geometry(self.ctx, C.c_uint32(self.scene.num_triangles), C.c_void_p(self.d_vi.data_ptr()), C.c_uint32(self.scene.num_vertices),
                                                 C.c_void_p(self.d_vd.data_ptr())))

    def set_build_mode(self, mode):
        """what the next create_geometry / rebuild uses: BUILD_QUALITY (0, the default: host binned SAH + re-insertion + collapse), BUILD_FAST (1: device Morton radix
        tree + collapse) or BUILD_TRBVH (2: the device radix tree restructured by 7-leaf treelets before the collapse -- a few ms more than BUILD_FAST on the device,
        fewer node steps per ray).  FPT_BVH_BUILD=quality|fast|trbvh overrides it."""
        self._check(self.L.fpt_rt_set_build_mode(self.ctx, C.c_uint32(mode)))

    def set_intersector(self, intersector):
        """what the next create_geometry / rebuild writes its triangle records for: INTERSECTOR_MT (0, the default: fpt-MT, bit for bit the oracle's) or
        INTERSECTOR_WATERTIGHT (1: fpt-WT, Woop-Benthin-Wald on the exact vertices -- no ray passes between two triangles that share an edge or a vertex).
        The live tree keeps its own until it is rebuilt.  FPT_INTERSECTOR=mt|watertight overrides it."""
        self._check(self.L.fpt_rt_set_intersector(self.ctx, C.c_uint32(intersector)))

    def intersector(self):
        """(requested, of_tree): what the next build will use, and what the live tree's records were written for"""
        req, live = C.c_uint32(), C.c_uint32()
        self._check(self.L.fpt_rt_intersector(self.ctx, C.byref(req), C.byref(live)))
        return req.value, live.value

    def rebuild_geometry(self, vertex_data=None):
        """fpt_rt_create_geometry over the device mesh again (after set_build_mode, or with new vertices)"""
        if vertex_data is not None:
            v = np.ascontiguousarray(vertex_data, np.float32)
            self.d_vd.copy_(self.torch.from_numpy(v).reshape(self.d_vd.shape).to(self.dev)); self.torch.cuda.synchronize(self.dev)
        self._check(self.L.fpt_rt_create_geometry(self.ctx, C.c_uint32(self.scene.num_triangles), C.c_void_p(self.d_vi.data_ptr()), C.c_uint32(self.scene.num_vertices),
                                                  C.c_void_p(self.d_vd.data_ptr())))

    def download_bvh(self):
        """the device tree as it stands: (nodes [n, 20] uint32, records [m, 12] float32: {v0, e1, e2, id, mask, delta}, or {v0, v1, v2, id, mask, delta} in a watertight tree)"""
        nn, nt, dp = C.c_uint32(), C.c_uint32(), C.c_uint32()
        self._check(self.L.fpt_rt_bvh_info(self.ctx, C.byref(nn), C.byref(nt), C.byref(dp)))
        nodes = np.zeros((nn.value, 20), np.uint32); recs = np.zeros((max(nt.value, 1), 12), np.float32)
        self._check(self.L.fpt_rt_download_bvh(self.ctx, C.c_void_p(nodes.ctypes.data), C.c_void_p(recs.ctypes.data)))
        return nodes, recs

    def debug_build_arrays(self):
        """the working arrays of the last DEVICE build of this context (fpt_debug_device_build; build modes 1 and 2), as the stages left them in the builder's scratch:
        a dict of numpy arrays -- refs, bounds, keys, vals, left, right, node_box, cells (LBVH_CELL_DTYPE), need, in mode 2 also tcount and tcost -- and the description
        words n, mode, nodes, passes, sort_buffer, depth_binary.  Raises FptError when the context holds no such build."""
        d = np.zeros(16, np.uint32)
        self._check(self.L.fpt_debug_device_build(self.ctx, C.c_uint32(0), C.c_void_p(d.ctypes.data), C.c_uint64(64)))
        n, mode, n_nodes, cell_bytes = (int(x) for x in d[:4])
        assert cell_bytes == LBVH_CELL_DTYPE.itemsize
        out = dict(n=n, mode=mode, nodes=n_nodes, passes=int(d[4]), sort_buffer=int(d[5]), depth_binary=int(d[6]))
        for name, (which, dt, cols) in DEVICE_BUILD_ARRAYS.items():
            if which >= 10 and mode != 2:
                continue
            rows = 1 if name == "bounds" else n if which in (1, 3, 4) else n_nodes if name == "need" else n - 1
            a = np.zeros((rows, cols) if cols > 1 else rows, dt)
            self._check(self.L.fpt_debug_device_build(self.ctx, C.c_uint32(which), C.c_void_p(a.ctypes.data), C.c_uint64(a.nbytes)))
            out[name] = a[0] if name == "bounds" else a
        return out

    def debug_set_treelet_passes(self, passes):
        """the NEXT device build of this context runs `passes` (0..3) treelet passes instead of 3 (mode 2 only; consumed by that build)"""
        self._check(self.L.fpt_debug_device_build(self.ctx, C.c_uint32(100 + int(passes)), None, C.c_uint64(0)))

    def clear_gbuffer_async(self):
        """the same clear as RenderingContextImpl::render issues it before every renderer->render (src/renderer.cu:1039): on the library's stream, no host synchronisation,
        in sequence with the passes a deferred render() holds back (fpt_clear_gbuffer)"""
        self._check(self.L.fpt_clear_gbuffer(self.ctx, C.byref(self.view)))

    def filter(self, instance):
        """RenderingContextImpl::filter (src/renderer.cu:1099-1151) -> FILTERED_C"""
        self._check(self.L.fpt_filter(self.ctx, C.byref(self.view), C.c_uint32(instance)))
        self.synchronize()

    def filter_variance(self, img, fw):
        torch = self.torch
        img = np.ascontiguousarray(img, np.float32); h, w = img.shape[:2]
        d_i = torch.from_numpy(img).to(self.dev); d_v = torch.zeros((h, w), dtype=torch.float32, device=self.dev)
        torch.cuda.synchronize(self.dev)
        self._check(self.L.fpt_filter_variance(self.ctx, C.c_uint32(w), C.c_uint32(h), C.c_void_p(d_i.data_ptr()), C.c_void_p(d_v.data_ptr()), C.c_uint32(fw)))
        self.synchronize()
        return d_v.cpu().numpy()

    def eaw(self, dst, op, w_img, w_min, img, gb_geo, var, params, step):
        """one EAW step on host arrays (H, W, 4); op < 0 = EAW_kernel, else EAW_mad_kernel with FilterOp bits; returns the new dst"""
        torch = self.torch
        img = np.ascontiguousarray(img, np.float32); h, w = img.shape[:2]
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(self.dev)  # noqa: E731
        d_dst, d_img, d_geo = up(dst), up(img), up(gb_geo)
        d_w = up(w_img) if w_img is not None else None
        d_v = up(var) if var is not None else None
        p = EawParams(); flat = np.asarray(params, np.float32)
        p.phi_normal, p.phi_position, p.phi_color = float(flat[0]), float(flat[1]), float(flat[2])
        p.E = (C.c_float * 3)(*flat[3:6]); p.U = (C.c_float * 3)(*flat[6:9]); p.V = (C.c_float * 3)(*flat[9:12]); p.W = (C.c_float * 3)(*flat[12:15])
        torch.cuda.synchronize(self.dev)
        self._check(self.L.fpt_eaw(self.ctx, C.c_uint32(w), C.c_uint32(h), C.c_void_p(d_dst.data_ptr()), C.c_int(op), C.c_void_p(d_w.data_ptr()) if d_w is not None else None,
                                   C.c_float(w_min), C.c_void_p(d_img.data_ptr()), C.c_void_p(d_geo.data_ptr()), C.c_void_p(d_v.data_ptr()) if d_v is not None else None,
                                   C.byref(p), C.c_uint32(step)))
        self.synchronize()
        return d_dst.cpu().numpy()

    def filter_xbl(self, instance):
        """the XBL driver of RenderingContextImpl::filter (src/renderer.cu:1161-1215) -> FILTERED_C; needs the context's shift table (any Renderer has one)"""
        self._check(self.L.fpt_filter_xbl(self.ctx, C.byref(self.view), C.c_uint32(instance)))
        self.synchronize()

    def xbl(self, dst, op, w_img, w_min, img, gb_geo, var, params, taps, filter_radius, step, shifts=None, tile=None):
        """one XBL step on host arrays (H, W, 4), the twin of eaw(): op = FilterOp bits, params = the 15 floats eaw() takes, taps / filter_radius / step as in
        fpt_xbl; shifts = (2, tile, tile) or (2, tile * tile) host floats, the planes of dimensions 0 and 1 (None: the context's own table); returns the new dst"""
        torch = self.torch
        img = np.ascontiguousarray(img, np.float32); h, w = img.shape[:2]
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(self.dev)  # noqa: E731
        d_dst, d_img, d_geo = up(dst), up(img), up(gb_geo)
        d_w = up(w_img) if w_img is not None else None
        d_v = up(var) if var is not None else None
        p = XblParams(); flat = np.asarray(params, np.float32)
        p.phi_normal, p.phi_position, p.phi_color, p.taps = float(flat[0]), float(flat[1]), float(flat[2]), int(taps)
        p.E = (C.c_float * 3)(*flat[3:6]); p.U = (C.c_float * 3)(*flat[6:9]); p.V = (C.c_float * 3)(*flat[9:12]); p.W = (C.c_float * 3)(*flat[12:15])
        if shifts is None:
            ptr, nd, ts = C.c_void_p(), C.c_uint32(), C.c_uint32()
            self._check(self.L.fpt_sequence_device_view(self.ctx, C.byref(ptr), C.byref(nd), C.byref(ts)))
            d_s, s_ptr, tile = None, ptr, ts.value
        else:
            shifts = np.ascontiguousarray(shifts, np.float32)
            tile = int(tile) if tile is not None else int(shifts.shape[-1])
            assert shifts.size == 2 * tile * tile, "shifts: two planes of tile x tile floats"
            d_s = up(shifts.reshape(-1)); s_ptr = C.c_void_p(d_s.data_ptr())
        torch.cuda.synchronize(self.dev)
        self._check(self.L.fpt_xbl(self.ctx, C.c_uint32(w), C.c_uint32(h), C.c_void_p(d_dst.data_ptr()), C.c_uint32(op), C.c_void_p(d_w.data_ptr()) if d_w is not None else None,
                                   C.c_float(w_min), C.c_void_p(d_img.data_ptr()), C.c_void_p(d_geo.data_ptr()), C.c_void_p(d_v.data_ptr()) if d_v is not None else None,
                                   C.byref(p), C.c_uint32(filter_radius), C.c_uint32(step), s_ptr, C.c_uint32(tile)))
        self.synchronize()
        return d_dst.cpu().numpy()

    # -- RT sub-boundary (device pointers in, device pointers out)
    def trace(self, rays, shadow=False, counted=False):
        torch = self.torch
        rays = np.ascontiguousarray(rays, RAY_DTYPE)
        d_r = torch.from_numpy(rays.view(np.float32).reshape(-1)).to(self.dev)
        d_h = torch.zeros(len(rays) * 4, dtype=torch.float32, device=self.dev)
        torch.cuda.synchronize(self.dev)
        cnt = TraceCounters()
        if counted:
            self._check(self.L.fpt_rt_trace_counted(self.ctx, C.c_uint32(len(rays)), C.c_void_p(d_r.data_ptr()), C.c_void_p(d_h.data_ptr()), C.c_int(1 if shadow else 0), C.byref(cnt)))
        else:
            fn = self.L.fpt_rt_trace_shadow if shadow else self.L.fpt_rt_trace
            self._check(fn(self.ctx, C.c_uint32(len(rays)), C.c_void_p(d_r.data_ptr()), C.c_void_p(d_h.data_ptr())))
        self.synchronize()
        hits = d_h.cpu().numpy().view(HIT_DTYPE).reshape(-1)
        return (hits, cnt) if counted else hits

    def trace_shadow_bits(self, rays):
        torch = self.torch
        rays = np.ascontiguousarray(rays, RAY_DTYPE)
        d_r = torch.from_numpy(rays.view(np.float32).reshape(-1)).to(self.dev)
        d_b = torch.zeros((len(rays) + 31) // 32, dtype=torch.int32, device=self.dev)
        torch.cuda.synchronize(self.dev)
        self._check(self.L.fpt_rt_trace_shadow_bits(self.ctx, C.c_uint32(len(rays)), C.c_void_p(d_r.data_ptr()), C.c_void_p(d_b.data_ptr())))
        self.synchronize()
        return d_b.cpu().numpy().view(np.uint32)

    def debug_set_trace_blocks(self, n_blocks):
        """fpt_debug_set_trace_blocks: every traversal launch of this context runs at most n_blocks 256-thread blocks from now on (0 = the default grid again; a value
        above the default is refused).  Results do not depend on the grid; a launch of more than 256 * n_blocks rays then draws tickets, steals and refills."""
        self._check(self.L.fpt_debug_set_trace_blocks(self.ctx, C.c_uint32(n_blocks)))

    def debug_trace_tickets(self):
        """fpt_debug_trace_tickets: the eight shard counters of the hand-out as the last trace / trace_shadow_bits call left them (uint32[8])"""
        out = (C.c_uint32 * 8)()
        self._check(self.L.fpt_debug_trace_tickets(self.ctx, out))
        return np.array(list(out), np.uint32)

    def debug_trace_hit_list(self, rays, capacity=None):
        """fpt_debug_trace_hit_list: the hit-listing traversal launch of the passes in flight on `rays` (taken as a path queue's scattered rays: interval (1e-3, 1e8)).
        Returns dict(list=HIT_DTYPE[capacity], src=uint32[capacity], cursor, waves, chunk); entries at and beyond `cursor` are as this call initialised them
        (t = 0, triId = 0, src = 0xFFFFFFFF), so a store past the list's end shows.  capacity None = the smallest the library accepts, count + waves x chunk."""
        torch = self.torch
        rays = np.ascontiguousarray(rays, RAY_DTYPE)
        cursor, waves, chunk = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
        if capacity is None:          # the query form of the call: no arrays, capacity 0 -> waves and chunk of a launch of this many rays, nothing launched
            self._check(self.L.fpt_debug_trace_hit_list(self.ctx, C.c_uint32(len(rays)), None, None, None, C.c_uint32(0), C.byref(cursor), C.byref(waves), C.byref(chunk)))
            capacity = len(rays) + waves.value * chunk.value
        d_r = torch.from_numpy(rays.view(np.float32).reshape(-1).copy()).to(self.dev) if len(rays) else torch.zeros(8, dtype=torch.float32, device=self.dev)
        d_l = torch.zeros(max(capacity, 1) * 4, dtype=torch.float32, device=self.dev)
        d_s = torch.full((max(capacity, 1),), -1, dtype=torch.int32, device=self.dev)
        torch.cuda.synchronize(self.dev)
        self._check(self.L.fpt_debug_trace_hit_list(self.ctx, C.c_uint32(len(rays)), C.c_void_p(d_r.data_ptr()), C.c_void_p(d_l.data_ptr()), C.c_void_p(d_s.data_ptr()),
                                                    C.c_uint32(capacity), C.byref(cursor), C.byref(waves), C.byref(chunk)))
        self.synchronize()
        return dict(list=d_l.cpu().numpy().view(HIT_DTYPE).reshape(-1)[:capacity], src=d_s.cpu().numpy().view(np.uint32)[:capacity],
                    cursor=int(cursor.value), waves=int(waves.value), chunk=int(chunk.value))

    def sequence(self, instance=None):
        if instance is not None:
            self._check(self.L.fpt_sequence_set_instance(self.ctx, C.c_uint32(instance)))
        nd = 6 * (self.options.max_path_length + 1)
        shifts = np.zeros((nd, 65536), np.float32); samples = np.zeros((nd, 65536), np.float32)
        self._check(self.L.fpt_sequence_download(self.ctx, C.c_void_p(shifts.ctypes.data), C.c_void_p(samples.ctypes.data)))
        return shifts, samples

    def lights(self):
        n = C.c_uint32()
        self._check(self.L.fpt_mesh_lights_download(self.ctx, C.byref(n), None, None, None, None, None))
        n = n.value; nt = self.scene.num_triangles
        vpls = np.zeros(n, VPL_DTYPE); cdf = np.zeros(n, np.float32); mcdf = np.zeros(nt, np.float32); minv = np.zeros(nt, np.float32)
        norm = C.c_float()
        self._check(self.L.fpt_mesh_lights_download(self.ctx, None, C.c_void_p(vpls.ctypes.data) if n else None, C.c_void_p(cdf.ctypes.data) if n else None,
                                                    C.c_void_p(mcdf.ctypes.data), C.c_void_p(minv.ctypes.data), C.byref(norm)))
        return dict(vpls=vpls, vpl_cdf=cdf, mesh_cdf=mcdf, mesh_inv_area=minv, norm=norm.value)

    def bvh_info(self):
        a, b, c = C.c_uint32(), C.c_uint32(), C.c_uint32()
        self._check(self.L.fpt_rt_bvh_info(self.ctx, C.byref(a), C.byref(b), C.byref(c)))
        return dict(nodes=a.value, leaf_tris=b.value, max_depth=c.value)

    def bvh_stats(self):
        st = BvhStats()
        self._check(self.L.fpt_rt_bvh_stats(self.ctx, C.byref(st)))
        return st.as_dict()

    def debug_math(self, op, a, b=None):
        torch = self.torch
        a = np.ascontiguousarray(a, np.float32); b = np.ascontiguousarray(b if b is not None else np.zeros_like(a), np.float32)
        da, db = torch.from_numpy(a).to(self.dev), torch.from_numpy(b).to(self.dev)
        o0, o1 = torch.zeros_like(da), torch.zeros_like(da)
        torch.cuda.synchronize(self.dev)
        self._check(self.L.fpt_debug_math(self.ctx, C.c_int(op), C.c_uint32(len(a)), C.c_void_p(da.data_ptr()), C.c_void_p(db.data_ptr()),
                                          C.c_void_p(o0.data_ptr()), C.c_void_p(o1.data_ptr())))
        return o0.cpu().numpy(), o1.cpu().numpy()

    def debug_bsdf(self, op, rec, mats, table, flags=0, vary=None, as_tensor=False):
        """fpt_debug_bsdf: one function of the device surface model per element (layouts: include/fermat_pt_hip.h).  rec: (n, 32) float32 records, or ONE record
        (shape (32,)) that every element reads, then with `vary` (n, 3) supplying each element's w_o / z; mats: scene.MATERIAL_DTYPE records.  Returns (n, 16) float32
        (as_tensor: the device tensor, for reductions that stay on the GPU)."""
        torch = self.torch
        rec = np.ascontiguousarray(rec, np.float32); mats = np.ascontiguousarray(mats)
        broadcast = rec.ndim == 1
        if broadcast and vary is None:
            raise ValueError("a broadcast record needs `vary`")
        n = len(vary) if broadcast else len(rec)
        assert rec.shape[-1] == 32 and mats.dtype.itemsize == 208 and len(mats) > 0 and (vary is None or np.shape(vary) == (n, 3))
        dr = torch.from_numpy(rec.reshape(-1)).to(self.dev)
        dm = torch.from_numpy(mats.view(np.uint8).reshape(-1)).to(self.dev)
        dt = torch.from_numpy(np.ascontiguousarray(table, np.float32)).to(self.dev)
        dv = torch.from_numpy(np.ascontiguousarray(vary, np.float32)).to(self.dev) if vary is not None else None
        out = torch.zeros(max(n, 1) * 16, dtype=torch.float32, device=self.dev)
        torch.cuda.synchronize(self.dev)
        self._check(self.L.fpt_debug_bsdf(self.ctx, C.c_int(op), C.c_uint32(flags), C.c_uint32(n), C.c_void_p(dm.data_ptr()), C.c_uint32(len(mats)),
                                          C.c_void_p(dt.data_ptr()), C.c_void_p(dr.data_ptr()), C.c_uint32(0 if broadcast else 32),
                                          C.c_void_p(dv.data_ptr() if dv is not None else None), C.c_void_p(out.data_ptr())))
        out = out[:n * 16].reshape(n, 16)
        return out if as_tensor else out.cpu().numpy()

    def debug_vertex(self, op, rec, flags=0, mats=None, textures=None, n=None):
        """fpt_debug_vertex: one function of the vertex set-up, the emitter sampler or the light-sample weights per element, on this renderer's scene and
        emitter tables (layouts: include/fermat_pt_hip.h).  rec: (n, 48) float32 records, or ONE record (shape (48,)) read by `n` elements; mats:
        scene.MATERIAL_DTYPE records (the NEE ops); textures: a list of (H, W, 4) float32 arrays that replace the scene's.  Returns (n, 32) float32."""
        torch = self.torch
        rec = np.ascontiguousarray(rec, np.float32)
        broadcast = rec.ndim == 1
        n = int(n) if broadcast else len(rec)
        assert rec.shape[-1] == 48
        dr = torch.from_numpy(rec.reshape(-1)).to(self.dev)
        dm, n_mats = None, 0
        if mats is not None:
            mats = np.ascontiguousarray(mats)
            assert mats.dtype.itemsize == 208 and len(mats) > 0
            dm, n_mats = torch.from_numpy(mats.view(np.uint8).reshape(-1)).to(self.dev), len(mats)
        dtex, keep = None, []
        if textures is not None:
            views = (Texture * max(1, len(textures)))()
            for i, tx in enumerate(textures):
                tx = np.ascontiguousarray(tx, np.float32); assert tx.ndim == 3 and tx.shape[2] == 4
                d = torch.from_numpy(tx.reshape(-1)).to(self.dev); keep.append(d)
                views[i].texels = d.data_ptr(); views[i].res_x = tx.shape[1]; views[i].res_y = tx.shape[0]
            dtex = torch.from_numpy(np.frombuffer(bytes(views), np.uint8).copy()).to(self.dev)
        out = torch.zeros(max(n, 1) * 32, dtype=torch.float32, device=self.dev)
        torch.cuda.synchronize(self.dev)
        self._check(self.L.fpt_debug_vertex(self.ctx, C.byref(self.view), C.c_int(op), C.c_uint32(flags), C.c_uint32(n),
                                            C.c_void_p(dm.data_ptr() if dm is not None else None), C.c_uint32(n_mats),
                                            C.c_void_p(dtex.data_ptr() if dtex is not None else None), C.c_uint32(len(textures) if textures is not None else 0),
                                            C.c_void_p(dr.data_ptr()), C.c_uint32(0 if broadcast else 48), C.c_void_p(out.data_ptr())))
        return out[:n * 32].reshape(n, 32).cpu().numpy()

    def debug_psf(self, op, data, size=0, firefly=100.0, touched=False):
        """fpt_debug_psf (layouts: include/fermat_pt_hip.h).  op 0: (n, 32) float32 records -> uint64 keys.  op 1: uint64 keys, size = log2 of the table ->
        dict(slots, table[, touched, touched_n]).  op 2: (n, 4) float32 (slot bits, value), size = cells -> dict(cells (size, 4) int64, mean (size, 3) float32).
        op 3: (n, 4) int64 cells -> (n, 3) float32 means."""
        torch = self.torch
        up = lambda a: torch.from_numpy(a.view(np.uint8).reshape(-1)).to(self.dev)  # noqa: E731
        zeros = lambda nbytes: torch.zeros(max(int(nbytes), 8), dtype=torch.uint8, device=self.dev)  # noqa: E731
        down = lambda t, dt, n: t.cpu().numpy()[:n * np.dtype(dt).itemsize].view(dt).copy()  # noqa: E731
        ptr = lambda t: C.c_void_p(t.data_ptr() if t is not None else None)  # noqa: E731
        o0 = o1 = tl = tn = None
        if op == 0:
            a = np.ascontiguousarray(data, np.float32).reshape(-1, 32); n = len(a)
            o0 = zeros(8 * n)
        elif op == 1:
            a = np.ascontiguousarray(data, np.uint64).reshape(-1); n = len(a); size = int(size)
            assert 1 <= size <= 16
            o0 = zeros(4 * n); o1 = zeros(8 << size)
            if touched:
                tl = zeros(4 << size); tn = zeros(4)
        elif op == 2:
            a = np.ascontiguousarray(data, np.float32).reshape(-1, 4); n = len(a); size = int(size)
            assert 1 <= size <= 65536
            o0 = zeros(32 * size); o1 = zeros(12 * size)
        elif op == 3:
            a = np.ascontiguousarray(data, np.int64).reshape(-1, 4); n = size = len(a)
            o1 = zeros(12 * n)
        else:
            raise ValueError("unknown op")
        d_in = up(a) if n else zeros(8)
        torch.cuda.synchronize(self.dev)
        self._check(self.L.fpt_debug_psf(self.ctx, C.c_int(op), C.c_uint32(1 if touched else 0), C.c_uint32(n), ptr(d_in), C.c_uint32(size), C.c_float(firefly),
                                         ptr(o0), ptr(o1), ptr(tl), ptr(tn)))
        if op == 0:
            return down(o0, np.uint64, n)
        if op == 1:
            out = dict(slots=down(o0, np.uint32, n), table=down(o1, np.uint64, 1 << size))
            if touched:
                out["touched"] = down(tl, np.uint32, 1 << size); out["touched_n"] = int(down(tn, np.uint32, 1)[0])
            return out
        if op == 2:
            return dict(cells=down(o0, np.int64, 4 * size).reshape(size, 4), mean=down(o1, np.float32, 3 * size).reshape(size, 3))
        return down(o1, np.float32, 3 * n).reshape(n, 3)

    def debug_bpt(self, op, arrays, params=(), n=None):
        """fpt_debug_bpt (layouts: include/fermat_pt_hip.h).  arrays: the op's arrays in order, each a numpy array (uploaded; None = a NULL pointer); params: the
        op's words; n: the element count (default: the rows of the first array).  Returns the arrays as the device left them, in order, with their dtypes and shapes."""
        torch = self.torch
        hosts = [None if a is None else np.ascontiguousarray(a) for a in arrays]
        devs = [None if a is None else torch.from_numpy(a.view(np.uint8).reshape(-1).copy() if a.size else np.zeros(8, np.uint8)).to(self.dev) for a in hosts]
        n = len(hosts[0]) if n is None else int(n)
        ptrs = (C.c_void_p * max(1, len(devs)))(*[None if d is None else d.data_ptr() for d in devs])
        par = (C.c_uint32 * max(1, len(params)))(*[int(p) for p in params])
        torch.cuda.synchronize(self.dev)
        self._check(self.L.fpt_debug_bpt(self.ctx, C.c_int(op), C.c_uint32(n), par, C.c_uint32(len(params)), ptrs, C.c_uint32(len(devs))))
        return [None if a is None else d.cpu().numpy()[:a.nbytes].view(a.dtype).reshape(a.shape) for a, d in zip(hosts, devs)]

    def debug_frame(self, op, frame, log=None, records=None, pixels=None, n=None, **par):
        """fpt_debug_frame (layouts: include/fermat_pt_hip.h).  frame: (8, n_pixels, 4) float32; log: dict of the op's log arrays -- emissive (n_bounces * cap, 4),
        nee0 / nee1 (n_bounces * cap * 2, 4), mask (cap * mask_words) uint32 and, for the merge, albedo_d / albedo_s (cap, 4) and blend (n_bounces * cap * 3, 4) or
        None; records: (n, 16) uint32; pixels: uint32 list or None.  op "bracket": kind, value.  op "write": base_instance, n_passes, acc_stride, cap, mask_words,
        n_bounces, fused_bounce, firefly[, n_slot].  op "merge": acc_stride, cap, mask_words, n_bounces, base_instance, n_passes, psf, firefly, clamp_max, p0.
        Returns (frame, log) as the device left them.  Everything the kernels index with is checked against the arrays here, before the launch."""
        torch = self.torch
        f32 = lambda v: int(np.float32(v).view(np.uint32))  # noqa: E731
        frame = np.ascontiguousarray(frame, np.float32)
        assert frame.ndim == 3 and frame.shape[0] == 8 and frame.shape[2] == 4 and frame.shape[1] >= 1
        n_pixels = frame.shape[1]
        if pixels is not None:
            pixels = np.ascontiguousarray(pixels, np.uint32).reshape(-1)
            assert len(pixels) and int(pixels.max()) < n_pixels
        log = dict(log or {})
        names = {"bracket": (), "write": ("emissive", "nee0", "nee1", "mask"), "merge": ("albedo_d", "albedo_s", "emissive", "nee0", "nee1", "blend", "mask")}[op]
        g = lambda k: par[k]  # noqa: E731
        if op == "bracket":
            n = (len(pixels) if pixels is not None else n_pixels) if n is None else int(n)
            assert n <= (len(pixels) if pixels is not None else n_pixels) and g("kind") in (0, 1, 2)
            params = [n_pixels, g("kind"), int(g("value")) if g("kind") == 1 else f32(g("value"))]
            arrays = list(frame) + [pixels]
            code = 0
        else:
            cap, words, nb, stride, n_passes = g("cap"), g("mask_words"), g("n_bounces"), g("acc_stride"), g("n_passes")
            batch = n_passes > 1 or op == "merge"
            want = dict(albedo_d=(cap, 4), albedo_s=(cap, 4), emissive=(nb * cap, 4), nee0=(nb * cap * 2, 4), nee1=(nb * cap * 2, 4), blend=(nb * cap * 3, 4), mask=(cap * words,))
            for k in names:
                a = log.get(k)
                if a is None:
                    assert (k == "blend" and not g("psf")) if op == "merge" else n_passes == 1
                    continue
                log[k] = a = np.ascontiguousarray(a, np.uint32 if k == "mask" else np.float32)
                assert a.shape == want[k], (k, a.shape, want[k])
            assert nb >= 1 and (not batch or (stride * n_passes <= cap and 32 * words >= (4 if op == "merge" and g("psf") else 3) * nb))
            if op == "write":
                records = np.ascontiguousarray(records, np.uint32).reshape(-1, 16)
                n = len(records)
                n_slot = par.get("n_slot", stride if pixels is None else len(pixels))
                v = records[:, 0] & 0x7FFFFFF
                assert g("fused_bounce") < nb and (records[:, 2] < nb).all() and (records[:, 3] <= 4).all() and (records[records[:, 3] == 3, 2] == g("fused_bounce")).all()
                if n_passes == 1:
                    assert (v < n_pixels).all() and len(np.unique(v)) == n, "one launch carries at most one sample per pixel"
                else:
                    assert n_slot <= stride and (v < n_slot).all() and (records[:, 1] < n_passes).all()
                    assert len(np.unique(records[:, 1].astype(np.int64) * stride + v)) == n, "one launch carries at most one sample per path"
                params = [n_pixels, g("base_instance"), n_passes, n_slot, stride, cap, words, nb, g("fused_bounce"), f32(g("firefly"))]
                arrays = list(frame) + [log.get(k) for k in names] + [pixels, records]
                code = 1
            else:
                p0 = g("p0")
                n = int(n)
                assert p0 + n <= stride and (pixels is not None or (p0 == 0 and n <= n_pixels)) and (pixels is None or p0 + n <= len(pixels))
                params = [n_pixels, stride, cap, words, nb, g("base_instance"), n_passes, 1 if g("psf") else 0, f32(g("firefly")), f32(g("clamp_max")), p0]
                arrays = list(frame) + [log.get(k) for k in names] + [pixels]
                code = 2
        devs = [None if a is None else torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy() if a.size else np.zeros(8, np.uint8)).to(self.dev) for a in arrays]
        ptrs = (C.c_void_p * len(devs))(*[None if d is None else d.data_ptr() for d in devs])
        prm = (C.c_uint32 * len(params))(*[int(x) for x in params])
        torch.cuda.synchronize(self.dev)
        self._check(self.L.fpt_debug_frame(self.ctx, C.c_int(code), C.c_uint32(n), prm, C.c_uint32(len(params)), ptrs, C.c_uint32(len(devs))))
        down = lambda a, d: d.cpu().numpy()[:a.nbytes].view(a.dtype).reshape(a.shape)  # noqa: E731
        out = np.stack([down(frame[c], devs[c]) for c in range(8)])
        for i, k in enumerate(names):
            if log.get(k) is not None:
                log[k] = down(log[k], devs[8 + i])
        return out, log

    def init_emitters_device(self, n_vpls=None, instance=0):
        """fpt_mesh_lights_init_device: the emitter tables built ON THE DEVICE from the device mesh (self.view.mesh, self.d_tex_views), bit for bit the tables
        fpt_mesh_lights_init builds from a host mesh with the same vertices; the host views give the static part only (materials, texture coordinates, texels)"""
        n = self.res[0] * self.res[1] if n_vpls is None else int(n_vpls)
        self._check(self.L.fpt_mesh_lights_init_device(self.ctx, C.c_uint32(n), C.byref(self.h_mesh), C.byref(self._h_tex), C.byref(self.view.mesh),
                                                       C.c_void_p(self.d_tex_views.data_ptr()), C.c_uint32(instance)))

    def update_emitters_device(self):
        """fpt_mesh_lights_update_device: the device mesh's vertices moved (refit_geometry / rebuild_geometry): all four tables are rebuilt on the device"""
        self._check(self.L.fpt_mesh_lights_update_device(self.ctx, C.byref(self.view.mesh)))

    def update_emitters(self, n_vpls=None):
        """fpt_mesh_lights_update: the host mesh's vertices moved in place.  The tables are rebuilt (returns 1) unless the live ones were built on the host from this
        mesh with this VPL count and no emitting triangle moved since (returns 0)"""
        n = self.res[0] * self.res[1] if n_vpls is None else int(n_vpls)
        rebuilt = C.c_int(-1)
        self._check(self.L.fpt_mesh_lights_update(self.ctx, C.c_uint32(n), C.byref(self.h_mesh), C.byref(self._h_tex), C.c_uint32(0), C.byref(rebuilt)))
        return rebuilt.value

    def reinit_emitters(self, n_vpls):
        """fpt_mesh_lights_init again with another VPL count (the probe's emitter tables)"""
        self._check(self.L.fpt_mesh_lights_init(self.ctx, C.c_uint32(n_vpls), C.byref(self.h_mesh), C.byref(self._h_tex), C.c_uint32(0)))
