#!/usr/bin/env python3
"""bench.py — the reference's headline benchmark on MI355X: Msample/s (and Mray/s) of the 8-bounce -pt path tracer on a
1600x900 frame (BASELINE.json `metric`, configs[2]).

  python bench.py --gpus N --steps K --warmup W
  N>1: python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P bench.py --gpus N ...

One "step" = one progressive pass (1 sample per pixel) of the full hot path over the synthetic frame: rescale -> QMC set-up ->
primary rays -> per bounce {closest-hit traversal, shade (BSDF, NEE, MIS), any-hit traversal fused with occlusion resolve} ->
variance update.  The passes of the timed region are kept in flight together (fpt_pt_render_batch; the frame is bit-identical to rendering them one
by one -- DESIGN.md 6b; --api render issues one fpt_pt_render call per pass and lets the library batch them).  Scene, BVH, textures and tables are
resident in HBM before the timed region.  N>1 shards the frame by interleaved scanlines (tile = one row; no data-path collective) and gathers
COMPOSITED_C to rank 0 over RCCL once, inside the timed region; `value` is then the STRONG-scaling rate (a step = one pass of the frame whatever N), with
`value_weak` (a step = N passes) measured beside it under --full.
Prints ONE JSON line on rank 0.

A plain run does what its headline figure needs and nothing else: set-up, warm-up, the timed steps, --dump-outputs, the line (`value`, `ms_per_step`,
the configuration and the per-launch timings of the timed steps).  --full adds everything else the benchmark measures: the instrumented re-run behind
`mray_per_s` and the `roofline` object, the measured copy bandwidth, the other scaling mode and the speed-up over a committed single-GPU line (N>1), the
single-GPU line's `extra` scenes, jobs and renderers (unless --no-extra) and the CPU baseline (unless --no-cpu-baseline).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

CONFIGS = {"c3": (1600, 900), "c4": (3840, 2160)}     # BASELINE.json configs[2] (the metric's configuration) and configs[3] (the 8-GPU tile-parallel job)
MAX_PATH_LENGTH = 9            # "-bounces 8"  (src/renderers/pathtracer.h:210-211)
                               # N>1: scanlines interleaved over ranks (tile = one row).  Measured on one GPU with tools/emulate_scaling.sh:
                               # a rank's share of an 8-way split takes 11.9 ms with rows, 12.1 ms with 64x4 or 8x8 tiles, 12.8 ms with 32x32 tiles
HBM_PEAK_GBS = 8000.0          # /opt/skills/guides/MI355X_MICROARCH.md: HBM3E 8 TB/s spec (6.3 TB/s achievable)
NODE_BYTES, TRI_BYTES, RAY_BYTES = 80, 48, 48    # 80-B 8-wide compressed node (one fetch per node step), 48-B triangle record, 32-B ray + 16-B hit
SURVEY_NODE_BYTES, SURVEY_TRI_BYTES = 256, 64    # SURVEY.md §8(d)'s uncompressed records: 64 B per PAIR of fp32 child boxes + refs -> 256 B for the eight
                                                 # children a node step tests; 48-B positions + 16-B index/flags per triangle


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=256)
    ap.add_argument("--warmup", type=int, default=64)
    ap.add_argument("--detail", type=float, default=1.0, help="tessellation of the bathroom2 stand-in (1.0 ~ 0.8M triangles)")
    ap.add_argument("--batch", type=int, default=int(os.environ.get("FPT_BENCH_BATCH", "0")),
                    help="passes in flight per launch chain (fpt_pt_render_batch); 1 = the reference's one pass per render(); "
                         "0 = 64 per GPU share (64*N under N-way sharding), capped by --steps; memory: ~0.7 KB per path in flight (fpt_bytes_per_path_in_flight)")
    ap.add_argument("--full", action="store_true",
                    help="also measure what the headline figure does not need (off by default): the instrumented re-run behind mray_per_s and the roofline "
                         "object, the measured copy bandwidth, the other scaling mode and speedup_vs_n1 (N>1), the single-GPU line's extra scenes, jobs and "
                         "renderers, and the CPU baseline")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full: skip the CPU baseline")
    ap.add_argument("--renderer", choices=("pt", "bpt", "psfpt"), default="pt",
                    help="pt = the headline path (default); bpt / psfpt = the widened rows (SURVEY 8f-1, 8f-3) measured the same way, "
                         "one pass per step (--batch passes in flight, default 32)")
    ap.add_argument("--sc", type=int, choices=(0, 1), default=1,
                    help="--renderer bpt: the reference's -sc flag; 1 = one connection per eye vertex into the flat light-vertex list (the reference's "
                         "default, src/renderers/bpt.h:62), 0 = connect every eye vertex to every vertex of its light path")
    ap.add_argument("--scaling", choices=("strong", "weak"), default="strong",
                    help="--gpus N > 1, headline path: strong (default) = the job is fixed, a step is one pass of the frame whatever N -- north_star's "
                         "'tile-parallel speed-up' of a fixed-spp render (BASELINE.md 3: t(1 GPU) / t(N GPUs)); the line also carries `value_weak`, measured "
                         "in a second timed region where a step is N passes (per-GPU work fixed).  weak = report that second figure as `value` instead")
    ap.add_argument("--config", choices=tuple(CONFIGS), default="c3",
                    help="c3 = BASELINE configs[2], 1600x900 (the configuration the metric is quoted on; default); c4 = configs[3], 3840x2160 (the 8-GPU tile job)")
    ap.add_argument("--lanes", type=int, default=0,
                    help="render lanes (fpt_pt_set_lanes: pixel ranges on their own HIP streams, bit-identical frames); 0 = 1.  Measured: 2 lanes +3 %% at 20 passes "
                         "in flight (1467 -> 1515 Msample/s), +1 %% at 64; one-pass mode (--batch 1): 2 / 4 / 8 lanes +3 / -20 / -44 %%.  Not the default: with lanes the "
                         "launches of different streams share the chip, and a launch's duration -- what the roofline object prices -- no longer measures the kernel alone")
    ap.add_argument("--api", choices=("batch", "render"), default="batch",
                    help="how the passes in flight are requested: batch = fpt_pt_render_batch(first, n) (default); render = the reference's calling convention, one "
                         "fpt_pt_render(instance) call per pass, with the library deferring and batching them (fpt_pt_set_deferred) -- same kernels, same frame")
    ap.add_argument("--no-extra", action="store_true", help="--full: skip the extra scenes, jobs and renderers (extra.*) of the single-GPU line")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write the frame buffer the timed path left after its last step to DIR/framebuffer.npy: its 8 float32 RGBA "
                         "channels at a fixed, seeded sample of 2^18 pixels (32 MB); one GPU only")
    ap.add_argument("--workload", choices=("bathroom2", "standin", "testball-room", "water-caustic"), default=None,
                    help="default: bathroom2 for --renderer pt / psfpt, water-caustic for --renderer bpt (BASELINE configs[4]: the bidirectional tracer on water_caustic).  "
                         "water-caustic (round 5) = the reference's own models/water_caustic/water_caustic.mtl and water_caustic.fa camera on procedural geometry "
                         "(water_caustic.obj is absent from the reference checkout): a pool with a wavy, nearly specular water surface, Silver objects, two small emitters of "
                         "radiance 8000, 0.86 M triangles (scene.water_caustic_standin, tools/gen_water_caustic_standin.py).  bathroom2 (default since round 4) = the reference's own models/bathroom2 materials, textures and camera on procedural bathroom geometry "
                         "(bathroom.obj is absent from the reference checkout): 493 instanced objects, 1.8 M triangles, ~11 node steps per ray (scene.bathroom2_standin, "
                         "tools/gen_bathroom2_standin.py); standin = rounds 1-3's stand-in (an open box with six big spheres, 0.8 M triangles at --detail 1, 3.3 node "
                         "steps per ray; --detail 4 gives a 13 M-triangle BVH that no longer fits the 256 MB Infinity Cache); testball-room = the room filled with "
                         "instanced material-testball meshes, textured surfaces and deep occlusion (scene.testball_room)")
    args = ap.parse_args()
    if args.workload is None:
        args.workload = "water-caustic" if args.renderer == "bpt" else "bathroom2"
    if args.dump_outputs and args.gpus > 1:
        ap.error("--dump-outputs needs --gpus 1 (under N-way sharding no rank holds the whole frame buffer)")
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        return self_launch(args.gpus)
    if args.renderer != "pt":
        return main_widened(args)

    import torch
    import fermat_amd as fa
    from fermat_amd import scene
    from fermat_amd.distributed import gather_framebuffer, comm_init, gather_framebuffer_capi

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if args.gpus > 1 and world != args.gpus:
        raise SystemExit("--gpus %d but WORLD_SIZE=%d: launch with --nproc-per-node %d (or with no launcher at all)" % (args.gpus, world, args.gpus))
    dist = None
    if "FPT_BENCH_FORCE_DEVICE" in os.environ:        # dry run of the N>1 path on a single GPU (with FPT_BENCH_BACKEND=gloo)
        local_rank = int(os.environ["FPT_BENCH_FORCE_DEVICE"])
    torch.cuda.set_device(local_rank)
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        backend = os.environ.get("FPT_BENCH_BACKEND", "nccl")     # "nccl" is RCCL on ROCm
        if backend == "nccl":
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", local_rank))
        else:
            dist.init_process_group(backend, rank=rank, world_size=world)

    W, H = CONFIGS[args.config]
    s, workload = load_workload(scene, args, (W, H))
    env = dict(torch=torch, fa=fa, dist=dist, world=world, rank=rank, local_rank=local_rank, gather_framebuffer=gather_framebuffer, comm_init=comm_init,
               gather_framebuffer_capi=gather_framebuffer_capi)
    out = bench_scene(env, args, s, workload, W, H, headline=True)
    if rank == 0:
        if args.full and world == 1 and not args.no_extra and args.workload == "bathroom2" and args.config == "c3" and args.detail == 1.0:
            # the same measurement on the two other stand-ins, so that the record shows the scene sensitivity of the headline number: rounds 1-3's headline scene
            # (easy: an open box, 3.3 node steps per ray) and the testball room (4.4 M triangles, ~15 node steps per ray)
            import copy
            out["extra"] = {}
            for key, wl in (("standin_r1_r3", "standin"), ("testball_room", "testball-room")):
                a2 = copy.copy(args); a2.workload = wl
                s2, w2 = load_workload(scene, a2, (W, H))
                o2 = bench_scene(env, a2, s2, w2, W, H, headline=False)
                out["extra"][key] = {"value": o2["value"], "unit": o2["unit"], "ms_per_step": o2["ms_per_step"], "mray_per_s": o2["mray_per_s"],
                                     "nodes_per_ray": o2["roofline"]["nodes_per_ray"], "tris_per_ray": o2["roofline"]["tris_per_ray"],
                                     "roofline_frac": o2["roofline"]["frac"], "kernel_ms_per_step": o2["kernel_ms_per_step"],
                                     "triangles": int(s2.num_triangles), "bvh": o2["config"]["bvh"], "workload": w2}
                del s2
            # the metric's own job and the reference's own calling convention, driver-visible (VERDICT r5 task 3): `spp256` = BASELINE configs[2] as specified -- 256 passes
            # of the frame, 64 in flight --, `sequential` = one pass per render() with nothing deferred (--batch 1: what a host that reads the frame after every pass gets)
            for key, over in (("spp256", dict(steps=256, warmup=64, batch=0)), ("sequential", dict(steps=min(args.steps, 20), warmup=min(args.warmup, 5), batch=1))):
                a2 = copy.copy(args)
                for k, v in over.items():
                    setattr(a2, k, v)
                o2 = out if (a2.steps, a2.warmup, a2.batch if a2.batch else 64) == (args.steps, args.warmup, args.batch if args.batch else 64) else \
                    bench_scene(env, a2, s, workload, W, H, headline=False)
                out["extra"][key] = {"value": o2["value"], "unit": o2["unit"], "steps": o2["steps"], "warmup": o2["warmup"], "ms_per_step": o2["ms_per_step"],
                                     "passes_in_flight": o2["config"]["passes_in_flight"], "api": o2["config"]["api"], "mray_per_s": o2["mray_per_s"],
                                     "kernel_ms_per_step": o2["kernel_ms_per_step"], "roofline_frac": o2["roofline"]["frac"],
                                     "job": {"spp256": "BASELINE configs[2] as specified: 256 spp of the 1600x900 frame on one GPU, 64 passes in flight",
                                             "sequential": "the reference's calling convention without deferral: one pass per fpt_pt_render, frame complete after every call"}[key]}
            # the widened rows (src/renderers/bpt_impl.h:196-259, src/renderers/psfpt_impl.h:275-284) measured the same way on the same frame, one
            # short run each, so that their rates are driver-visible too (VERDICT r3 task 6): 32 passes in flight, the reference's default -sc 1 for the BPT
            for kind in ("bpt", "psfpt"):
                a3 = copy.copy(args)
                if kind == "bpt":
                    a3.workload = "water-caustic"          # configs[4]'s scene in kind (VERDICT r4 task 1); the PSFPT stays on the headline scene
                o3 = main_widened(a3, kind=kind, quick_steps=32)
                out["extra"][kind] = {"value": o3["value"], "unit": o3["unit"], "ms_per_step": o3["ms_per_step"], "steps": o3["steps"], "mray_per_s": o3["mray_per_s"],
                                      "metric": o3["metric"], "passes_in_flight": o3["config"]["passes_in_flight"], "kernel_ms_per_step": o3["kernel_ms_per_step"],
                                      "roofline_frac": o3["roofline"]["frac"], "nodes_per_ray": o3["roofline"]["nodes_per_ray"], "tris_per_ray": o3["roofline"]["tris_per_ray"],
                                      "workload": o3["config"]["workload"]}
        if args.full and world == 1 and not args.no_cpu_baseline:
            out["cpu_baseline"] = cpu_baseline(s, W, H)
        print(json.dumps(out))
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()


def bench_scene(env, args, s, workload, W, H, headline):
    """the timed measurement of one scene: returns the JSON object on rank 0 (None elsewhere); headline = the line's own scene, not one of its extras"""
    torch, fa, dist, world, rank, local_rank = env["torch"], env["fa"], env["dist"], env["world"], env["rank"], env["local_rank"]
    K, Wu = args.steps, args.warmup
    tile = (W, 1)
    if os.environ.get("FPT_BENCH_TILE"):        # tuning aid: "32" or "1600x1"
        tile = tuple(int(v) for v in os.environ["FPT_BENCH_TILE"].split("x")) if "x" in os.environ["FPT_BENCH_TILE"] else int(os.environ["FPT_BENCH_TILE"])
    lists = fa.tile_pixel_lists(W, H, world, tile=tile)
    pixels = lists[rank] if world > 1 else None
    emulate = int(os.environ.get("FPT_BENCH_EMULATE_WORLD", "0"))       # tuning aid: time rank 0's share of an N-way tile split on one GPU
    if world == 1 and emulate > 1:
        pixels = fa.tile_pixel_lists(W, H, emulate, tile=tile)[int(os.environ.get("FPT_BENCH_EMULATE_RANK", "0"))]
    elif world == 1 and os.environ.get("FPT_BENCH_TILE"):
        pixels = lists[0]
    # the gbuffer is part of the pass: the reference clears it before every render() (src/renderer.cu:1039) and writes it at bounce 0 of every pass
    # (src/pathtracer_core.h:801-807); until round 5 this line ran without one
    r = fa.Renderer(s, W, H, fa.default_options(MAX_PATH_LENGTH), device=local_rank, pixels=pixels, gbuffer=True)
    dev = r.dev
    cdev = dev if (dist is None or dist.get_backend() != "gloo") else torch.device("cpu")     # where small collectives live

    def barrier():
        torch.cuda.synchronize(dev); r.synchronize()
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize(dev)

    n_share = emulate if (world == 1 and emulate > 1) else world
    n_here = len(pixels) if pixels is not None else W * H

    def batch_for(passes):
        P = args.batch if args.batch > 0 else 64 * n_share        # measured on one MI355X: 8 -> 970, 16 -> 1093, 32 -> 1198, 64 -> 1265 Msample/s
        return max(1, min(P, passes))          # (until round 3 also capped by PixelInfo's 27-bit field; the pass offset now travels beside it)

    # strong scaling: a step is one pass of the frame whatever N (the fixed job of north_star's speed-up); weak: a step is N passes, each rank
    # rendering its 1/N of the rows of every one of them (the work per GPU and per step is that of the single-GPU run)
    pps_primary = world if (args.scaling == "weak") else 1
    P = batch_for(K * pps_primary)
    P_max = max(P, batch_for(K * world)) if world > 1 else P
    if P_max > 1:
        r.set_batch(P_max)
    if args.api == "render" and P > 1:
        r.set_deferred(P)
    n_lanes = args.lanes if args.lanes > 0 else 1
    if n_lanes > 1:
        r.set_lanes(n_lanes)
    n_lanes = r.lane_count()

    def run(first, count, P):
        """render passes first .. first+count-1, P at a time"""
        if args.api == "render":          # one {gbuffer clear, render(instance)} per pass, as RenderingContextImpl::render issues them; the library collects P per batch
            for i in range(first, first + count):
                r.clear_gbuffer_async()
                r.render_pass(i)
            r.flush()
            return
        i = first
        while i < first + count:
            n = min(P, first + count - i)
            r.clear_gbuffer_async()          # n {clear, render} pairs leave the last clear under the last pass's hits: one stream-ordered clear per batch
            if n > 1:
                r.render_batch(i, n)
            else:
                r.render_pass(i)
            i += n

    # the gather: the library's own RCCL path (fpt_gather_framebuffer: pack, ONE group of ncclSend / ncclRecv on its stream, unpack) whenever the ranks sit on
    # distinct GPUs.  There is NO fallback on that route: if RCCL cannot be bound inside the library, or its communicator does not span `world` ranks by
    # RCCL's own count, the run aborts (VERDICT r3 task 2d) -- config.gather can only read "torch.distributed" for the explicit gloo dry run of the N>1
    # code on one GPU (FPT_BENCH_BACKEND=gloo)
    capi = dist is not None and dist.get_backend() == "nccl"
    rccl_ranks = None
    if capi:
        from fermat_amd.distributed import comm_info, set_tile_lists
        try:
            env["comm_init"](r, rank, world)
            rccl_ranks = comm_info(r)[1]            # ncclCommCount: what RCCL itself says the communicator spans
        except Exception as e:          # noqa: BLE001 - fatal
            raise SystemExit("[bench] rank %d: the library could not set up its RCCL communicator (%s): no fallback, aborting" % (rank, e))
        if rccl_ranks != world:
            raise SystemExit("[bench] rank %d: the library's RCCL communicator spans %s ranks, expected %d" % (rank, rccl_ranks, world))
        print("[bench] rank %d: RCCL communicator inside libfermat_pt_hip.so spans %d ranks (ncclCommCount)" % (rank, rccl_ranks), file=sys.stderr)
        set_tile_lists(r, lists, rank, root=0)      # the tile tables go to the device once, outside the timed region

    def gather():
        # stream-ordered behind the render calls: nothing synchronises in front of it (the barrier of the timed region synchronises afterwards)
        if capi:
            env["gather_framebuffer_capi"](r, None, root=0, channels=(5,))
        elif dist is not None:
            r.synchronize()
            env["gather_framebuffer"](r.fb, lists, rank, world, dst=0, channels=(5,))

    def timed(first, passes, P):
        barrier()
        t0 = time.perf_counter()
        run(first, passes, P)
        gather()
        barrier()
        elapsed = time.perf_counter() - t0
        if dist is not None:
            te = torch.tensor([elapsed], dtype=torch.float64, device=cdev)
            dist.all_reduce(te, op=dist.ReduceOp.MAX)
            elapsed = float(te.item())
        return elapsed

    Kp, Wp = K * pps_primary, Wu * pps_primary
    run(0, Wp, P)
    gather()                  # warm the communicator too
    r.set_profiling(2)        # asynchronous hipEvent pairs around every trace/shade launch, on the library's stream
    elapsed = timed(Wp, Kp, P)
    timings = r.collect_timings()
    union = r.union_timings()
    r.set_profiling(0)
    if headline and args.dump_outputs:          # before the instrumented re-run below renders the same passes again
        dump_outputs(r, args.dump_outputs)
    # the other scaling mode, measured the same way in a second timed region (N > 1 only: at N = 1 the two coincide)
    other = None
    if world > 1 and headline and args.full:
        pps_o = 1 if pps_primary > 1 else world
        P_o = batch_for(K * pps_o)
        run(Wp + Kp, Wu * pps_o, P_o)
        e_o = timed(Wp + Kp + Wu * pps_o, K * pps_o, P_o)
        other = {"passes_per_step": pps_o, "passes_in_flight": P_o, "value": float(W) * H * K * pps_o / e_o / 1e6, "ms_per_step": e_o / K * 1e3}

    tms = torch.tensor([timings["primary_trace"][0] + timings["path_trace"][0], timings["shadow_trace"][0], timings["shade"][0], union["all_trace"], union["shade"]],
                       dtype=torch.float64, device=cdev)
    if dist is not None:
        dist.all_reduce(tms, op=dist.ReduceOp.MAX)
    tms = tms.cpu().numpy()
    if args.full:
        # instrumented re-run of the same K passes: exact rays / nodes popped / triangles tested of the timed launches
        r.set_counting(True)
        run(Wp, Kp, P)
        r.synchronize()
        closest, shadow = r.trace_counters()
        r.set_counting(False)
        counts = torch.tensor([closest.rays, closest.nodes_visited, closest.tris_tested, shadow.rays, shadow.nodes_visited, shadow.tris_tested],
                              dtype=torch.float64, device=cdev)
        if dist is not None:
            dist.all_reduce(counts, op=dist.ReduceOp.SUM)
        counts = counts.cpu().numpy()

    out = None
    if rank == 0:
        pps = pps_primary
        samples = float(W) * H * Kp
        if world == 1 and emulate > 1:
            samples = float(len(pixels)) * K
        config_key = pmc_config_key(args.workload, s.num_triangles, P, world, (W, H), n_lanes)
        bvh = r.bvh_stats()
        value = samples / elapsed / 1e6
        out = {
            "metric": "Msample/s, %dx%d 8-bounce PT + NEE (Mray/s alongside)" % (W, H),
            "value": value,
            "unit": "Msample/s",
            "n_gpus": world, "steps": K, "warmup": Wu,
            "ms_per_step": elapsed / K * 1e3,
            "higher_is_better": True,
            "scaling": args.scaling,
            "vs_baseline": None,
            "dtype": "f32",
            "data": "synthetic",
            "config": {"workload": workload + ", %d spp/step, 8-bounce PT + VPL NEE" % pps, "baseline_config": {"c3": "configs[2]", "c4": "configs[3]"}[args.config],
                       "passes_per_step": pps, "passes_timed": Kp,
                       "resolution": [W, H], "max_path_length": MAX_PATH_LENGTH, "nee": "vpl", "triangles": int(s.num_triangles),
                       "passes_in_flight": P, "render_lanes": n_lanes, "api": ("fpt_pt_render x %d per batch, deferred by the library" % P) if (args.api == "render" and P > 1) else ("fpt_pt_render_batch" if P > 1 else "fpt_pt_render"),
                       "config_key": config_key, "bvh": bvh,
                       "sharding": ("scanlines (%dx1 tiles) round-robin over ranks; " % W + ("weak scaling: a step = %d passes of the frame, each rank renders its rows of every pass" % pps
                                     if pps > 1 else "strong scaling: a step = one pass of the frame")) if world > 1 else "none",
                       "gather": ("fpt_gather_framebuffer (RCCL grouped send/recv inside libfermat_pt_hip.so)" if capi else "torch.distributed gather (%s)" % dist.get_backend()) if world > 1 else "none",
                       "rccl_ranks": rccl_ranks},
            # sums of launch durations (HIP events around every launch); with render lanes > 1 launches of different lanes overlap, and the
            # *_busy figures are the time at least one such launch was running
            "kernel_ms_per_step": {"trace_primary+mixed": float(tms[0]) / K, "trace_shadow_only": float(tms[1]) / K, "shade": float(tms[2]) / K,
                                   "trace_busy": float(tms[3]) / K, "shade_busy": float(tms[4]) / K, "render_lanes": n_lanes},
        }
        if args.full:
            rays_total = counts[0] + counts[3]
            out["mray_per_s"] = rays_total / elapsed / 1e6
            out["rays_per_step"] = rays_total / K
            out["roofline"] = trace_roofline(timings, union, counts, closest.rays + shadow.rays, bvh, config_key, P, fa)
            if other is not None:
                # both scaling modes in the one line: `value` is the one --scaling names, the other one sits beside it
                out["value_weak" if pps == 1 else "value_strong"] = other["value"]
                out["other_scaling"] = other
            if world > 1:
                # north_star's tile-parallel speed-up = this run's strong-scaling rate over the committed single-GPU line of the same job
                strong = value if pps == 1 else (other["value"] if other else None)
                ref, ref_file = find_single_gpu_line(args, (W, H), K, s.num_triangles)
                # CROSS-RUN: the denominator is a committed single-GPU line of an earlier run, not a measurement of this session; the driver computes its own
                # efficiency from its own per-N runs
                out["speedup_vs_n1"] = (strong / ref["value"]) if (ref and strong) else None
                out["speedup_vs_n1_source"] = ("cross-run: profiles/%s (value %.1f Msample/s, same workload, resolution and --steps on one GPU, measured in an earlier session)" % (ref_file, ref["value"])) if ref else \
                    "no single-GPU line of this job (workload, resolution, --steps %d) under profiles/" % K
            if headline:
                out["roofline"]["measured_copy_gbs"] = measured_copy_bandwidth(torch, dev)
    r.close()
    return out


def trace_roofline(timings, union, counts, rank0_rays, bvh, config_key, P, fa):
    """--full: the roofline object of the dominant kernel = the wide-BVH traversal kernel (trace_kernel: closest-hit launch for the primary rays, then
    one MIXED launch per bounce = closest-hit rays of bounce b+1 + any-hit shadow rays of bounce b), priced against HBM as SURVEY 8(d) asks:
    algorithmic bytes = closest rays*(32+16) + shadow rays*32 + node steps*80 + triangle records tested*48,
    over the summed launch time of every traversal launch in the timed region (HIP events on the library's stream).
    Three prices of the same launches, side by side: the algorithmic bytes of THIS layout (80-B node, 48-B
    record) -> `achieved`/`frac` as the contract defines them; the same counts priced with SURVEY 8(d)'s 64-B records; and the
    bytes that really crossed the HBM interface according to the PMC counters of a rocprofv3 collection over this same
    configuration (`traffic`; null when profiles/ holds none for this scene + passes in flight).  A frac >= 1 means the tree is
    served from L2 / Infinity Cache: the roof that binds then is the VALU (`valu`, same PMC collection)."""
    n_trace_launches = timings["primary_trace"][1] + timings["path_trace"][1] + timings["shadow_trace"][1]
    trace_ms = float(timings["primary_trace"][0] + timings["path_trace"][0] + timings["shadow_trace"][0])      # rank 0's own launches
    all_rays = counts[0] + counts[3]
    rank0_share = (rank0_rays / all_rays) if all_rays else 1.0
    alg_bytes = (counts[0] * RAY_BYTES + counts[3] * 32 + (counts[1] + counts[4]) * NODE_BYTES + (counts[2] + counts[5]) * TRI_BYTES) * rank0_share
    achieved = alg_bytes / (trace_ms * 1e-3) / 1e9 if trace_ms > 0 else 0.0
    # the same counts priced with SURVEY 8(d)'s record sizes (what the kernel would move with uncompressed records)
    survey_bytes = (counts[0] * RAY_BYTES + counts[3] * 32 + (counts[1] + counts[4]) * SURVEY_NODE_BYTES + (counts[2] + counts[5]) * SURVEY_TRI_BYTES) * rank0_share
    avg_launch_ms = trace_ms / max(1, n_trace_launches)
    pmc, pmc_file, pmc_note = find_pmc_summary(config_key, fa)
    traffic = pmc.get("hbm_bytes_per_launch") if pmc else None
    rf = {"bound": "hbm", "kernel": "trace_kernel (8-wide compressed BVH traversal: closest-hit + any-hit/resolve)", "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s",
          "frac": achieved / HBM_PEAK_GBS, "traffic": traffic,
          "traffic_source": ("profiles/%s: rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE (separate passes) over this same command line "
                             "(same scene, %d passes in flight, same kernel sources: %s), bytes per traversal launch of the timed region" % (pmc_file, P, pmc.get("source_hash"))) if pmc else pmc_note,
          # the chip-level rate: the same bytes over the time at least one traversal launch was running (= achieved when lanes == 1)
          "achieved_chip": (alg_bytes / (union["all_trace"] * 1e-3) / 1e9) if union["all_trace"] > 0 else None,
          "frac_chip": (alg_bytes / (union["all_trace"] * 1e-3) / 1e9 / HBM_PEAK_GBS) if union["all_trace"] > 0 else None,
          # counter bytes of the timed region's launches over THIS run's live durations of the same launches; beside it the same bytes over the durations
          # rocprofv3 itself timed them at (bytes and time of the same launches of one run: VERDICT r4 task 2a)
          "counter_gbs": (traffic / (avg_launch_ms * 1e-3) / 1e9) if (traffic and avg_launch_ms > 0) else None,
          "counter_frac": (traffic / (avg_launch_ms * 1e-3) / 1e9 / HBM_PEAK_GBS) if (traffic and avg_launch_ms > 0) else None,
          "counter_gbs_profiled": pmc.get("counter_gbs_profiled") if pmc else None,
          "survey_model_gbs": survey_bytes / (trace_ms * 1e-3) / 1e9 if trace_ms > 0 else 0.0,
          "survey_model_frac": survey_bytes / (trace_ms * 1e-3) / 1e9 / HBM_PEAK_GBS if trace_ms > 0 else 0.0,
          "launches": int(n_trace_launches), "avg_launch_ms": avg_launch_ms,
          "alg_bytes_per_launch": alg_bytes / max(1, n_trace_launches),
          "record_bytes": {"node": NODE_BYTES, "triangle": TRI_BYTES, "ray+hit": RAY_BYTES},
          "bvh_bytes": int(bvh["nodes"]) * NODE_BYTES + int(bvh["records"]) * TRI_BYTES,
          "valu": pmc.get("valu") if pmc else None,
          "nodes_per_ray": (counts[1] + counts[4]) / max(1.0, all_rays), "tris_per_ray": (counts[2] + counts[5]) / max(1.0, all_rays)}
    binding_roof(rf, pmc_file)
    return rf


def load_workload(scene, args, res):
    """the scene of the bench line + the words that name it (never a silent stand-in: bathroom.obj is absent from the reference checkout)"""
    if args.workload == "bathroom2":
        s = scene.bathroom2_standin()
        return s, ("bathroom2-standin-r4 %dx%d (models/bathroom2/bathroom.obj is absent from the reference checkout: geometry = procedural bathroom, 493 objects instanced "
                   "through the .fa front-end, %d triangles; materials, textures and camera = the reference's own models/bathroom2/bathroom.mtl, textures/ and "
                   "bathroom.fa; tools/gen_bathroom2_standin.py)" % (res[0], res[1], s.num_triangles))
    if args.workload == "water-caustic":
        s = scene.water_caustic_standin()
        return s, ("water_caustic-standin %dx%d (models/water_caustic/water_caustic.obj is absent from the reference checkout: geometry = procedural pool room, 49 objects "
                   "instanced through the .fa front-end, %d triangles, 819200 of them the wavy water surface; materials and camera = the reference's own "
                   "models/water_caustic/water_caustic.mtl and water_caustic.fa; tools/gen_water_caustic_standin.py)" % (res[0], res[1], s.num_triangles))
    if args.workload == "testball-room":
        s = scene.testball_room()
        return s, ("testball-room %dx%d (the HARDER bathroom2 stand-in, tools/gen_testball_room.py: the room filled with 196 instanced "
                   "material-testball meshes through the .fa front-end, 13 textured/glossy/coated/transmissive/emissive materials, %d triangles)" % (res[0], res[1], s.num_triangles))
    s = scene.bathroom_standin(args.detail)
    return s, ("bathroom2-standin-r1 %dx%d (rounds 1-3's headline scene: models/bathroom2/bathroom.obj is absent from the reference checkout; an open box with six big "
               "spheres, %d triangles, Cornell materials + 2 procedural textures, instanced CornellBox-Glossy shelf, --detail %g)" % (res[0], res[1], s.num_triangles, args.detail))


def self_launch(n):
    """`python bench.py --gpus N` without a launcher: re-exec under torch.distributed.run, one rank per GPU of this node over RCCL
    (the form the driver documents for N>1 is the same command line, so both routes run the same code)"""
    import socket
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0)); port = sk.getsockname()[1]
    env = dict(os.environ); env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0"); env.setdefault("OMP_NUM_THREADS", "4")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n), "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    os.execve(sys.executable, cmd, env)


def main_widened(args, kind=None, quick_steps=None):
    """(kind / quick_steps: the single-GPU --full line's `extra.bpt` / `extra.psfpt` -- a short run of the same measurement, returned instead of printed)
    BPT (`-bpt`, BASELINE config 5's renderer) and PSFPT on the same frame, scene and JSON contract as the PT line.  A step is one
    pass.  BPT shards light and eye sub-paths by scanline and sums the light-tracing splats with one integer all-reduce per pass
    (fermat_amd.distributed.allreduce_splats); PSFPT's cache is shared by all pixels: its ranks exchange the cells they touched after every pass."""
    import torch
    import fermat_amd as fa
    from fermat_amd import scene
    from fermat_amd.distributed import gather_framebuffer, allreduce_splats, comm_init, exchange_psf_cells, exchange_light_vertices

    as_extra = kind is not None
    kind = kind or args.renderer
    world = int(os.environ.get("WORLD_SIZE", "1")); rank = int(os.environ.get("RANK", "0")); local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if args.gpus > 1 and world != args.gpus:
        raise SystemExit("--gpus %d needs torch.distributed.run with --nproc-per-node %d" % (args.gpus, args.gpus))
    if "FPT_BENCH_FORCE_DEVICE" in os.environ:
        local_rank = int(os.environ["FPT_BENCH_FORCE_DEVICE"])
    torch.cuda.set_device(local_rank)
    dist = None
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        backend = os.environ.get("FPT_BENCH_BACKEND", "nccl")
        if backend == "nccl":
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", local_rank))
        else:
            dist.init_process_group(backend, rank=rank, world_size=world)
    W, H = CONFIGS[args.config]
    K = args.steps
    if as_extra:
        K = quick_steps
    # BPT and PSFPT keep passes in flight like the PT (fpt_bpt_render_batch, fpt_psfpt_render_batch: the PSFPT's passes are independent until
    # the blend, and the cache is folded in pass order); a tile-sharded PSFPT exchanges its cache cells after every pass, one pass at a time
    P = 1
    if kind == "bpt" or (kind == "psfpt" and world == 1):
        P = args.batch if args.batch > 0 else 32 * world
        P = max(1, min(P, K))
    Wu = min(args.warmup, 8) if P == 1 else P
    s, workload_words = load_workload(scene, args, (W, H))
    lists = fa.tile_pixel_lists(W, H, world, tile=(W, 1))
    pixels = lists[rank] if world > 1 else None
    L = MAX_PATH_LENGTH

    def make():
        if kind == "bpt":
            r = fa.Renderer(s, W, H, fa.default_options(L), device=local_rank, pixels=pixels, gbuffer=True, bpt_options=fa.default_bpt_options(L, single_connection=args.sc))
            if P > 1:
                r.bpt_set_batch(P)
            sp = r.bpt_defer_splats() if world > 1 else None
            if world > 1 and args.sc == 1:
                # -sc 1 draws its connections from the light vertices of ALL light paths: the ranks exchange theirs after the light sub-paths (the image
                # is then the single-GPU one for any N) -- over RCCL inside the library between GPUs, through torch.distributed in the gloo dry run
                r.bpt_set_shared_light_vertices(True)
                if dist.get_backend() == "nccl":
                    comm_init(r, rank, world)
            return r, sp
        r = fa.Renderer(s, W, H, fa.default_options(L), device=local_rank, pixels=pixels, gbuffer=True, psf_options=fa.default_psf_options())
        if P > 1:
            r.psf_set_batch(P)
        if world > 1:
            # the cache is shared by every pixel: the ranks exchange the cells they touched after every pass (integer sums merged by key) -- over
            # RCCL inside the library on distinct GPUs, through torch.distributed in the gloo dry run on one GPU
            r.psf_set_sharded(True)
            if dist.get_backend() == "nccl":
                comm_init(r, rank, world)
        return r, None

    def run(r, sp, first, count):
        i = first
        while i < first + count:
            n = min(P, first + count - i)
            r.clear_gbuffer_async()
            if kind == "bpt":
                if n > 1:
                    r.bpt_render_batch(i, n)
                else:
                    r.bpt_render(i)
                if world > 1 and args.sc == 1:
                    if dist.get_backend() == "nccl":
                        r.bpt_exchange_light_vertices()
                    else:
                        exchange_light_vertices(r, rank, world)
                    r.bpt_finish()
                if sp is not None:          # one integer all-reduce of the splat sums per batch, then fold + merge
                    r.synchronize(); allreduce_splats(sp, world); torch.cuda.synchronize(r.dev)
                    r.bpt_resolve_splats()
            elif n > 1:
                r.psf_render_batch(i, n)
            else:
                r.psf_render(i)
                if world > 1:
                    if dist.get_backend() == "nccl":
                        r.psf_exchange_cells()
                    else:
                        exchange_psf_cells(r, rank, world)
                    r.psf_finish()
            i += n

    r, sp = make()
    dev = r.dev
    cdev = dev if (dist is None or dist.get_backend() != "gloo") else torch.device("cpu")

    def barrier():
        torch.cuda.synchronize(dev); r.synchronize()
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize(dev)

    run(r, sp, 0, Wu)
    if dist is not None:
        gather_framebuffer(r.fb, lists, rank, world, dst=0, channels=(5,))
    r.set_profiling(2)
    barrier()
    t0 = time.perf_counter()
    run(r, sp, Wu, K)
    r.synchronize()
    if dist is not None:
        gather_framebuffer(r.fb, lists, rank, world, dst=0, channels=(5,))
    barrier()
    elapsed = time.perf_counter() - t0
    if dist is not None:
        te = torch.tensor([elapsed], dtype=torch.float64, device=cdev)
        dist.all_reduce(te, op=dist.ReduceOp.MAX)
        elapsed = float(te.item())
    timings = r.collect_timings()
    r.set_profiling(0)
    if not as_extra and args.dump_outputs:
        dump_outputs(r, args.dump_outputs)
    if args.full:
        # instrumented re-run of the same passes from the same starting state (PSFPT's cache and frame carry over between passes)
        r.close()
        r, sp = make()
        run(r, sp, 0, Wu)
        r.set_counting(True)
        run(r, sp, Wu, K)
        r.synchronize()
        closest, shadow = r.trace_counters()
        r.set_counting(False)
        counts = torch.tensor([closest.rays, closest.nodes_visited, closest.tris_tested, shadow.rays, shadow.nodes_visited, shadow.tris_tested], dtype=torch.float64, device=cdev)
        if dist is not None:
            dist.all_reduce(counts, op=dist.ReduceOp.SUM)
        counts = counts.cpu().numpy()
    if rank == 0:
        config_key = pmc_config_key("%s/%s%s" % (args.workload, kind, "-sc%d" % args.sc if kind == "bpt" else ""), s.num_triangles, P, world)
        name = {"bpt": "BPT (-bpt -sc %d: %s, light tracing)" % (args.sc, "one connection per eye vertex, the reference's default" if args.sc else "all connections"),
                "psfpt": "PSFPT (path-space filtering)"}[kind]
        out = {
            "metric": "Msample/s, 1600x900 8-bounce %s (Mray/s alongside)" % name,
            "value": float(W) * H * K / elapsed / 1e6, "unit": "Msample/s", "n_gpus": world, "steps": K, "warmup": Wu,
            "ms_per_step": elapsed / K * 1e3, "higher_is_better": True, "scaling": "strong", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
            "config": {"workload": workload_words + ", 1 spp/step, 8-bounce %s" % kind.upper(),
                       "baseline_config": "configs[4] (the reference's water_caustic.obj is absent: a named stand-in)" if (kind == "bpt" and args.workload == "water-caustic") else None,
                       "resolution": [W, H], "max_path_length": L, "triangles": int(s.num_triangles), "passes_in_flight": P, "config_key": config_key,
                       "sharding": ("scanlines round-robin over ranks + " + ("one integer all-reduce of the light-tracing splat sums per batch" if kind == "bpt" else
                                                                          "the touched cache cells exchanged and merged by key after every pass")) if world > 1 else "none"},
            "kernel_ms_per_step": {("trace_closest+mixed" if kind == "bpt" else "trace_closest"): float(timings["primary_trace"][0]) / K,      # BPT: the eye path's connections ride in the next bounce's closest-hit launch
                                   "trace_any_hit": float(timings["shadow_trace"][0]) / K,
                                   "vertex_kernels": float(timings["shade"][0]) / K},
        }
        if args.full:
            trace_ms = float(timings["primary_trace"][0] + timings["shadow_trace"][0])
            n_launches = int(timings["primary_trace"][1] + timings["shadow_trace"][1])
            all_rays = counts[0] + counts[3]
            share = ((closest.rays + shadow.rays) / all_rays) if all_rays else 1.0
            alg_bytes = (counts[0] * RAY_BYTES + counts[3] * RAY_BYTES + (counts[1] + counts[4]) * NODE_BYTES + (counts[2] + counts[5]) * TRI_BYTES) * share
            achieved = alg_bytes / (trace_ms * 1e-3) / 1e9 if trace_ms > 0 else 0.0
            avg_launch_ms = trace_ms / max(1, n_launches)
            pmc, pmc_file, pmc_note = find_pmc_summary(config_key, fa)
            traffic = pmc.get("hbm_bytes_per_launch") if pmc else None
            out["mray_per_s"] = all_rays / elapsed / 1e6
            out["rays_per_step"] = all_rays / K
            out["roofline"] = {
                "bound": "hbm", "kernel": "trace_kernel (8-wide compressed BVH traversal: closest-hit and any-hit launches; any-hit results are written, 16 B per ray)",
                "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": achieved / HBM_PEAK_GBS, "traffic": traffic,
                "traffic_source": ("profiles/%s: rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE (separate passes) over this same command line (same kernel sources: %s), bytes per "
                                   "traversal launch of the timed region" % (pmc_file, pmc.get("source_hash"))) if pmc else pmc_note,
                "counter_gbs": (traffic / (avg_launch_ms * 1e-3) / 1e9) if (traffic and avg_launch_ms > 0) else None,
                "counter_frac": (traffic / (avg_launch_ms * 1e-3) / 1e9 / HBM_PEAK_GBS) if (traffic and avg_launch_ms > 0) else None,
                "counter_gbs_profiled": pmc.get("counter_gbs_profiled") if pmc else None,
                "valu": pmc.get("valu") if pmc else None,
                "launches": n_launches, "avg_launch_ms": avg_launch_ms, "alg_bytes_per_launch": alg_bytes / max(1, n_launches),
                "record_bytes": {"node": NODE_BYTES, "triangle": TRI_BYTES, "ray+hit": RAY_BYTES},
                "nodes_per_ray": (counts[1] + counts[4]) / max(1.0, all_rays), "tris_per_ray": (counts[2] + counts[5]) / max(1.0, all_rays)}
            binding_roof(out["roofline"], pmc_file)
        if as_extra:
            r.close()
            return out
        if args.full and world == 1 and not args.no_cpu_baseline:
            out["cpu_baseline"] = cpu_baseline_widened(kind, s, W, H, args.sc)
        print(json.dumps(out))
    r.close()
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()


def dump_outputs(r, out_dir):
    """--dump-outputs: the frame buffer a caller of the timed path reads after its last pass (Renderer.framebuffer(): 8 channels x pixels x RGBA, float32;
    184 MB at 1600x900), at a fixed, seeded sample of 2^18 pixels, the same for every channel and every run: DIR/framebuffer.npy, (8, 262144, 4), 32 MB"""
    fb = r.framebuffer()
    n = fb.shape[1]
    idx = np.sort(np.random.default_rng(0).choice(n, min(n, 1 << 18), replace=False))
    os.makedirs(out_dir, exist_ok=True)
    np.save(os.path.join(out_dir, "framebuffer.npy"), np.ascontiguousarray(fb[:, idx], np.float32))


def cap_frac(rf):
    """`frac` is a fraction: algorithmic bytes served mostly from L2 / Infinity Cache can exceed what HBM could deliver (BPT: 1.07 in round 5) -- the contract's price is
    kept as `frac_algorithmic`, `frac` is capped at 1 and says why (VERDICT r5 task 1a)"""
    rf["frac_algorithmic"] = rf["frac"]
    if rf["frac"] > 1.0:
        rf["frac"] = 1.0
        rf["frac_note"] = ("algorithmic bytes / launch time = %.0f GB/s exceeds the %.0f GB/s HBM roof: the tree is served from L2 / Infinity Cache, HBM is not what bounds this kernel "
                           "(see counter_frac and valu); frac capped at 1, the uncapped ratio is frac_algorithmic" % (rf["achieved"], rf["peak"]))


def binding_roof(rf, pmc_file):
    """Which roof binds (VERDICT r3 task 8): the contract's object prices the traversal kernel against HBM, but when the counters of the matching PMC collection say
    that little of that traffic reaches HBM (counter_frac < 0.4) while the VALU is busy (valu.frac > 0.8), the record itself says so: bound = "valu", with the lane
    utilisation -- the counter that then measures the distance to the roof -- at the top level of the object (null without a matching collection)"""
    cap_frac(rf)
    v = rf.get("valu")
    rf["lane_utilisation"] = v.get("lane_utilisation") if v else None
    rf["valu_useful_frac"] = v.get("useful_frac") if v else None
    if v and rf.get("counter_frac") is not None and rf["counter_frac"] < 0.4 and v.get("frac", 0.0) > 0.8:
        rf["bound"] = "valu"
        rf["bound_note"] = ("VALU issue binds, not HBM: the PMC collection %s puts HBM traffic at %.2f of the 8 TB/s roof and VALU issue at %.2f of what 1024 SIMDs x 2.4 GHz can issue of this kernel's own instruction mix, with %.0f %% of "
                            "the lanes active; achieved / peak / frac stay the contract's HBM pricing of the ALGORITHMIC bytes (mostly L2 / Infinity-Cache hits)"
                            % (pmc_file, rf["counter_frac"], v["frac"], 100.0 * (v.get("lane_utilisation") or 0.0)))


def cpu_baseline_widened(kind, s, W, H, sc=1):
    """the oracle's BPT / PSFPT on a bounded sample: BPT on every 8th scanline of the frame (its light and eye sub-paths, the same
    sharding rule the GPUs use), PSFPT on the full frame (its cache is global); passes until ~12 s have elapsed"""
    import fermat_amd as fa
    from fermat_amd import scene
    from oracle import binding as ob
    table = np.fromfile(os.path.join(scene.DATA_DIR, "glossy_reflectance.dat"), np.float32)
    o = ob.OraclePT(s, W, H, ob.default_options(MAX_PATH_LENGTH), table, scene.DATA_DIR)
    cores = usable_host_cores()
    o.set_trace_threads(cores)
    if kind == "bpt":
        o.bpt_init(ob.default_bpt_options(MAX_PATH_LENGTH, single_connection=sc), scene.DATA_DIR)
        px = fa.tile_pixel_lists(W, H, 8, tile=(W, 1))[0]
    else:
        o.psf_enable(ob.default_psf_options())
        px = None
    n_passes = 0
    t0 = time.perf_counter()
    while True:
        if kind == "bpt":
            o.bpt_render(n_passes, pixels=px)
        else:
            o.render_pass(n_passes)
        n_passes += 1
        dt = time.perf_counter() - t0
        if dt > 12.0 or n_passes >= 64:
            break
    n_px = len(px) if px is not None else W * H
    return {"value": float(n_px) * n_passes / dt / 1e6, "unit": "Msample/s", "cores": cores, "kind": "port",
            "sample": "%d passes of the oracle's %s over %s of the same 1600x900 frame (same scene and options); host-BVH traces on %d threads, "
                      "vertex processing sequential; BVH build excluded; %.1f s in total"
                      % (n_passes, kind.upper(), "every 8th scanline (%d pixels: light and eye sub-paths of those pixels)" % n_px if px is not None else "all pixels", cores, dt)}


def pmc_config_key(workload, triangles, passes_in_flight, world, res=(1600, 900), lanes=1):
    # (a tree built in the fast mode is another configuration: counters collected over the quality tree are not its counters)
    mode = "|bvh=fast" if os.environ.get("FPT_BVH_BUILD") == "fast" else ""
    return "%s|triangles=%d|passes_in_flight=%d|lanes=%d|gpus=%d|%dx%d L=9%s" % (workload, triangles, passes_in_flight, lanes, world, res[0], res[1], mode)


def find_single_gpu_line(args, res, steps, triangles):
    """the newest committed single-GPU bench line (profiles/r*_bench_line*.json) of the same job -- workload, triangle count, resolution, --steps, one
    pass per step -- or (None, None): the denominator of north_star's tile-parallel speed-up"""
    d = os.path.join(ROOT, "profiles")
    best = (None, None)
    for name in sorted(os.listdir(d)) if os.path.isdir(d) else []:
        if not (name.endswith(".json") and "_bench_line" in name):
            continue
        try:
            j = json.load(open(os.path.join(d, name)))
            c = j["config"]
            if (j.get("n_gpus") == 1 and j.get("steps") == steps and c.get("resolution") == [res[0], res[1]] and c.get("triangles") == int(triangles)
                    and c.get("passes_per_step", 1) == 1 and j.get("metric", "").endswith("PT + NEE (Mray/s alongside)") and c.get("max_path_length") == MAX_PATH_LENGTH
                    and c.get("render_lanes", 1) == 1 and c.get("api", "fpt_pt_render_batch") == "fpt_pt_render_batch" and "|bvh=fast" not in c.get("config_key", "")):
                best = (j, name)
        except Exception:
            continue
    return best


def find_pmc_summary(config_key, fa=None):
    """the newest profiles/r*_pmc_*.json (written by tools/summarize_pmc.py from a rocprofv3 --pmc collection) whose `config_key` names exactly this configuration AND whose
    `source_hash` is that of the kernel sources this run was built from (fermat_amd.api.kernel_source_hash: a kernel or builder change without a re-collection must not
    ship stale counters under a fresh `value`) -> (summary, file name, None), or (None, None, why not)"""
    d = os.path.join(ROOT, "profiles")
    best = (None, None)
    stale = None
    try:
        from fermat_amd.api import kernel_source_hash
        want = kernel_source_hash()
    except Exception:          # noqa: BLE001
        want = None
    for name in sorted(os.listdir(d)) if os.path.isdir(d) else []:
        if not (name.endswith(".json") and "_pmc_" in name):
            continue
        try:
            j = json.load(open(os.path.join(d, name)))
        except Exception:
            continue
        if j.get("config_key") != config_key or "timed_launches" not in j:          # (summaries older than round 5 averaged over warm-up launches too: not used)
            continue
        if want is not None and j.get("source_hash") == want:
            best = (j, name)
        else:
            stale = name
    if best[0] is not None:
        return best[0], best[1], None
    if stale:
        return None, None, ("profiles/%s holds counters of this configuration but of OTHER kernel sources (its source_hash differs from %s): traffic is not reported beside this "
                            "run's rate; re-collect with tools/collect_pmc.sh" % (stale, want))
    return None, None, "no PMC collection for this configuration (%s) under profiles/; not measurable from inside the process" % config_key


def measured_copy_bandwidth(torch, dev):
    """attainable HBM bandwidth on this box (SURVEY 8d asks for it next to the nominal peak): device-to-device copy of 1 GiB,
    bytes read + bytes written over the best of 5 timings"""
    a = torch.empty(1 << 28, dtype=torch.float32, device=dev)
    b = torch.empty_like(a)
    a.fill_(1.0); b.copy_(a)
    best = 1e30
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); b.copy_(a); e1.record(); e1.synchronize()
        best = min(best, e0.elapsed_time(e1))
    return 2.0 * a.numel() * 4 / (best * 1e-3) / 1e9


def usable_host_cores():
    """Threads this process can actually keep busy: the affinity mask, capped by the cgroup CPU quota (the GPU boxes expose 256
    hardware threads under a 16-CPU quota; 256 OpenMP threads there run 10x SLOWER than 16)."""
    try:
        cores = len(os.sched_getaffinity(0))
    except AttributeError:
        cores = os.cpu_count() or 1
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        if quota != "max":
            cores = max(1, min(cores, -(-int(quota) // int(period))))
    except (OSError, ValueError):
        pass
    return cores


def cpu_baseline(s, W, H):
    """The oracle ("port": CUGAR-style host SAH BVH + the CPU restatement of the PT) timed on this node's host cores over a
    bounded sample of the SAME workload: full passes of the 1600x900 frame until ~12 s have elapsed.  The BVH traces of every
    queue (closest-hit and shadow rays, the same rays the GPU traces for these passes) and the shading of every queue run on all
    usable host cores (results are identical for any thread count); ray generation, occlusion resolve and the variance update
    stay sequential.  `value` is the whole-pass rate, `trace_mray_per_s` the rate of the traces alone."""
    import fermat_amd as fa
    from fermat_amd import scene
    from oracle import binding as ob
    table = np.fromfile(os.path.join(scene.DATA_DIR, "glossy_reflectance.dat"), np.float32)
    o = ob.OraclePT(s, W, H, ob.default_options(MAX_PATH_LENGTH), table, scene.DATA_DIR)
    cores = usable_host_cores()
    o.set_trace_threads(cores)
    n_passes = 0
    t0 = time.perf_counter()
    while True:
        o.render_pass(n_passes)
        n_passes += 1
        dt = time.perf_counter() - t0
        if dt > 12.0 or n_passes >= 64:
            break
    c = o.counters()
    ts = o.trace_seconds()
    return {"value": float(W) * H * n_passes / dt / 1e6, "unit": "Msample/s", "cores": cores, "kind": "port",
            "sample": "%d full passes of the same 1600x900 frame (same scene, options and QMC instances 0..%d): host-BVH traces (%.1f s) and shading (%.1f s) "
                      "of all queues on %d threads; BVH build excluded; %.1f s in total" % (n_passes, n_passes - 1, ts, o.shade_seconds(), cores, dt),
            "mray_per_s": (c[0] + c[1]) / dt / 1e6,
            "trace_mray_per_s": (c[0] + c[1]) / ts / 1e6 if ts > 0 else None,
            # north_star's baseline by name: "a CUGAR host-BVH CPU trace of the same rays on the node's own cores (core count stated)" -- the traces alone, shading excluded
            "host_bvh_trace_of_the_same_rays": {"value": (c[0] + c[1]) / ts / 1e6 if ts > 0 else None, "unit": "Mray/s", "cores": cores, "rays": int(c[0] + c[1]),
                                                "what": "closest-hit and any-hit queues of these %d passes traced through the oracle's CUGAR-style full-sweep SAH BVH2 (oracle/o_bvh.h) "
                                                        "on %d host threads: the rays the GPU's trace_kernel launches trace for the same passes (compare the line's mray_per_s)" % (n_passes, cores)}}


if __name__ == "__main__":
    main()
