"""Times one render() of a Metropolis renderer -- the primary-sample-space one (`--renderer pssmlt`, the default) or the multiplexed one (`--renderer mmlt`, one
(s, t) technique per chain) -- on the water_caustic stand-in (the scene of bench.py --renderer bpt), at the reference's defaults (64 K chains, 4 spp) and at 1 M
chains.  A timing tool, not a bench line: bench.py measures the flagship workloads and knows nothing of these renderers.

    python tools/time_pssmlt.py [--renderer pssmlt|mmlt] [--mmlt-swaps F] [--lens] [--res 1600 900] [--path-length 9] [--chains 65536 1048576] [--spp 4] [--repeats 3]
                                [--reseeding R [R ...] --startup-skips K] [--shard R/N]

With `--reseeding` (chains that persist across render calls, fpt_mlt_set_persistence) the tool times PERIODS instead: one context per value of R, all alive, run in
turn -- a warm-up block of max(R) calls each, then `--repeats` timed blocks of max(R) consecutive instances each, alternating between the settings -- and prints per
setting the median time per call by position in the period (position 0 reseeds, the others continue), the mutations per second over a whole period and the frame mean
after 16 calls.

With `--shard R/N` (chain shards, fpt_mlt_set_chain_shard) every context runs rank R's share of the chains of an N-rank run, on this one GPU: a timed call is the
render call plus fpt_mlt_finish WITHOUT a communicator -- the whole presampling pass, the shard's chain steps and the resolve of the shard's own sums, but no
all-reduce.  The lines are labelled "emulated": they say what one rank computes, not what N GPUs achieve; the frame they leave is one rank's part of the sums.

After the timed calls: one call at 2 x spp, from which the time of everything but the chain steps (rescale, presampling pass, seed CDF and seeds, coordinate
recovery, resolve) is extrapolated as  t(spp) - chain_length(spp) x the time per step,  and one call with the traversal kernels' counters on, which gives the rays
the traversal fetched per mutation (the presampling pass and null rays included).  `--renderer mmlt` also reports the rays its chain steps queued (its own counter).

Per configuration: one warm-up render call (code objects, allocations), then `--repeats` timed calls of consecutive instances, each timed by the host clock
around a call that ends in a device synchronise (fpt_pssmlt_render reads its counters back, and synchronize() follows).  Prints one JSON line per configuration:
the times of the calls, their median and spread, the chain length, the launches a call enqueues and Msample/s = spp x pixels / median (mutations, not pixels
converged).  Needs the GPU; there is no CPU path."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import fermat_amd as fa  # noqa: E402
from fermat_amd import scene  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, nargs=2, default=(1600, 900))
    ap.add_argument("--path-length", type=int, default=9)
    ap.add_argument("--chains", type=int, nargs="+", default=[64 * 1024, 1024 * 1024])
    ap.add_argument("--spp", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--renderer", choices=("pssmlt", "mmlt"), default="pssmlt")
    ap.add_argument("--mmlt-swaps", type=int, default=0)
    ap.add_argument("--lens", action="store_true", help="--renderer mmlt: the lens connections (s, 1) beside the other techniques (light tracing on)")
    ap.add_argument("--reseeding", type=int, nargs="+", default=None, help="time periods of R calls with persistent chains, one context per value, alternating")
    ap.add_argument("--startup-skips", type=int, default=0)
    ap.add_argument("--shard", default=None, metavar="R/N", help="emulated: time rank R's share of the chains of an N-rank run on this GPU, without the all-reduce")
    args = ap.parse_args()
    args.shard = tuple(int(x) for x in args.shard.split("/")) if args.shard else None
    assert args.shard is None or (len(args.shard) == 2 and 0 <= args.shard[0] < args.shard[1]), "--shard R/N needs 0 <= R < N"
    mmlt = args.renderer == "mmlt"
    W, H = args.res
    L = args.path_length
    s = scene.water_caustic_standin()
    table = np.fromfile(os.path.join(scene.DATA_DIR, "glossy_reflectance.dat"), np.float32)
    for n_chains in args.chains:
        if args.reseeding:
            time_periods(args, s, table, n_chains)
            continue

        def renderer(spp):
            if mmlt:
                r = fa.Renderer(s, W, H, fa.default_options(L), table=table, mmlt_options=fa.default_mmlt_options(L, mmlt_frequency=args.mmlt_swaps, lens_techniques=int(args.lens), n_chains=n_chains, spp=spp))
            else:
                r = fa.Renderer(s, W, H, fa.default_options(L), table=table, pssmlt_options=fa.default_pssmlt_options(L, n_chains=n_chains, spp=spp))
            set_shard(r, args)
            return r

        def timed(r, first, repeats):
            render = render_call(r, mmlt, args)
            render(0, sync=True)                                           # warm-up: every shape the timed calls use
            out = []
            for i in range(repeats):
                r.synchronize()
                t0 = time.perf_counter()
                render(first + i, sync=True)
                out.append(time.perf_counter() - t0)
            return out
        r = renderer(args.spp)
        times = timed(r, 1, args.repeats)
        st = r.mmlt_stats() if mmlt else r.pssmlt_stats()
        # the traversal's own count of the rays it fetched in one more call
        r.set_counting(True)
        render_call(r, mmlt, args)(1 + args.repeats, sync=True)
        closest, shadow = r.trace_counters()
        r.set_counting(False)
        traced = int(closest.rays) + int(shadow.rays)
        r2 = renderer(2 * args.spp)
        med2 = float(np.median(timed(r2, 1, args.repeats)))
        st2 = r2.mmlt_stats() if mmlt else r2.pssmlt_stats()
        r2.close()
        fb = r.framebuffer()[5][:, :3]
        med = float(np.median(times))
        # launches a call enqueues: the presampling pass and chain_length steps, each a BPT wavefront of (L - 1) x 2 light launches + 1 + 3 L + 2 eye launches + the acceptance test
        per_wavefront = 1 + 2 * (L - 1) + 1 + 3 * L + 2
        step_s = (med2 - med) / max(1, st2["chain_length"] - st["chain_length"])
        extra = {"renderer": args.renderer, "step_ms": round(step_s * 1e3, 3), "presample_and_seed_s": round(med - st["chain_length"] * step_s, 4),
                 "traced_rays_per_mutation": round(traced / (st["chain_length"] * n_chains), 3)}
        if mmlt:
            n_tech = L * (L + 1) // 2 + (L - 1 if args.lens else 0)
            norms, _ = r.mmlt_st_norms()          # indexed [t, s]: the share of the norms the lens connections (t = 1) hold
            extra.update({"lens": int(args.lens), "st_norm_share_t1": round(float(norms[1].sum() / max(float(norms.sum()), 1e-30)), 4)})
            extra.update({"mmlt_swaps": args.mmlt_swaps, "queued_rays_per_mutation": round(st["rays"] / (st["chain_length"] * n_chains), 3), "swaps_proposed": st["swaps_proposed"],
                          "swaps_accepted": st["swaps_accepted"], "table_cells": n_tech * W * H, "table_MiB": round(n_tech * W * H * 16 / 2 ** 20, 1)})
        extra.update(shard_labels(r, args))
        print(json.dumps({**extra, "tool": "time_pssmlt", "scene": "water_caustic-standin", "triangles": int(s.num_triangles), "resolution": [W, H], "max_path_length": L,
                          "n_chains": n_chains, "spp": args.spp, "chain_length": st["chain_length"], "render_s": [round(t, 4) for t in times], "median_s": round(med, 4),
                          "spread_s": round(max(times) - min(times), 4), "launches_per_call_approx": (st["chain_length"] + 1) * per_wavefront + st["chain_length"] + 6,
                          "mutations_per_s_M": round(st["chain_length"] * n_chains / med / 1e6, 2), "msample_per_s": round(args.spp * W * H / med / 1e6, 2),
                          "accepted": st["accepted"], "rejected": st["rejected"], "image_brightness": float(st["image_brightness"]),
                          "frame_finite": bool(np.isfinite(fb).all()), "frame_mean": float(fb.mean())}))
        r.close()


def set_shard(r, args):
    if args.shard:
        r.mlt_set_chain_shard(*args.shard)


def render_call(r, mmlt, args):
    """render(instance, sync): the renderer's call, followed under --shard R/N with N > 1 by mlt_finish (no communicator: the shard's own sums are resolved)"""
    render = r.mmlt_render if mmlt else r.pssmlt_render
    if not args.shard or args.shard[1] == 1:
        return render

    def both(instance, sync=False):
        render(instance)
        r.mlt_finish(sync=sync)
    return both


def shard_labels(r, args):
    if not args.shard:
        return {}
    return {"emulated": True, "shard": "%d/%d" % args.shard, "n_local": r.mlt_chain_shard()["n_local"], "allreduce": "not run"}


def time_periods(args, s, table, n_chains):
    """--reseeding: per-call times by position in the period, the settings alternating block by block"""
    mmlt = args.renderer == "mmlt"
    W, H = args.res
    L = args.path_length
    block = max(args.reseeding)
    runs = []
    for R in args.reseeding:
        if mmlt:
            r = fa.Renderer(s, W, H, fa.default_options(L), table=table, mmlt_options=fa.default_mmlt_options(L, mmlt_frequency=args.mmlt_swaps, lens_techniques=int(args.lens), n_chains=n_chains, spp=args.spp))
        else:
            r = fa.Renderer(s, W, H, fa.default_options(L), table=table, pssmlt_options=fa.default_pssmlt_options(L, n_chains=n_chains, spp=args.spp))
        r.mlt_set_persistence(R, args.startup_skips)
        set_shard(r, args)
        runs.append(dict(R=R, r=r, next=0, times=[[] for _ in range(R)], reseeded=[[] for _ in range(R)], mean16=None))
    for rep in range(args.repeats + 1):          # block 0 warms up: code objects, allocations, and the first period's reseed
        for run in runs:
            r = run["r"]; render = render_call(r, mmlt, args)
            for _ in range(block):
                i = run["next"]; run["next"] += 1
                r.synchronize()
                t0 = time.perf_counter()
                render(i, sync=True)
                dt = time.perf_counter() - t0
                if rep > 0:
                    run["times"][i % run["R"]].append(dt); run["reseeded"][i % run["R"]].append(r.mlt_persistence()["last_call_reseeded"])
                if run["next"] == 16:
                    run["mean16"] = float(r.framebuffer()[5][:, :3].mean())
    for run in runs:
        r = run["r"]; R = run["R"]
        st = r.mmlt_stats() if mmlt else r.pssmlt_stats()
        med = [float(np.median(t)) for t in run["times"]]
        assert all(all(f == int(k == 0) for f in flags) for k, flags in enumerate(run["reseeded"]))
        fb = r.framebuffer()[5][:, :3]
        print(json.dumps({**shard_labels(r, args), "tool": "time_pssmlt", "mode": "periods", "renderer": args.renderer, "scene": "water_caustic-standin", "resolution": [W, H], "max_path_length": L,
                          "n_chains": n_chains, "spp": args.spp, "chain_length": st["chain_length"], "mmlt_swaps": args.mmlt_swaps if mmlt else None, "lens": int(args.lens) if mmlt else None,
                          "reseeding": R, "startup_skips": r.mlt_persistence()["startup_skips"], "timed_calls": sum(len(t) for t in run["times"]),
                          "median_ms_by_position": [round(m * 1e3, 3) for m in med], "reseeding_call_median_ms": round(med[0] * 1e3, 3),
                          "continuing_call_median_ms": round(float(np.median(np.concatenate(run["times"][1:]))) * 1e3, 3) if R > 1 else None,
                          "period_ms": round(sum(med) * 1e3, 3), "mutations_per_s_M_over_a_period": round(R * st["chain_length"] * n_chains / sum(med) / 1e6, 2),
                          "calls": run["next"], "frame_mean_after_16_calls": run["mean16"], "frame_mean": float(fb.mean()), "frame_finite": bool(np.isfinite(fb).all())}))
        r.close()


if __name__ == "__main__":
    main()
