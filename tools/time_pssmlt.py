"""Times one render() of the primary-sample-space Metropolis renderer on the water_caustic stand-in (the scene of bench.py --renderer bpt), at the reference's
defaults (64 K chains, 4 spp) and at 1 M chains.  A timing tool, not a bench line: bench.py measures the flagship workloads and knows nothing of this renderer.

    python tools/time_pssmlt.py [--res 1600 900] [--path-length 9] [--chains 65536 1048576] [--spp 4] [--repeats 3]

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
    args = ap.parse_args()
    W, H = args.res
    L = args.path_length
    s = scene.water_caustic_standin()
    table = np.fromfile(os.path.join(scene.DATA_DIR, "glossy_reflectance.dat"), np.float32)
    for n_chains in args.chains:
        opts = fa.default_pssmlt_options(L, n_chains=n_chains, spp=args.spp)
        r = fa.Renderer(s, W, H, fa.default_options(L), table=table, pssmlt_options=opts)
        r.pssmlt_render(0, sync=True)                                  # warm-up: every shape the timed calls use
        times = []
        for i in range(args.repeats):
            r.synchronize()
            t0 = time.perf_counter()
            r.pssmlt_render(1 + i, sync=True)
            times.append(time.perf_counter() - t0)
        st = r.pssmlt_stats()
        fb = r.framebuffer()[5][:, :3]
        med = float(np.median(times))
        # launches a call enqueues: the presampling pass and chain_length steps, each a BPT wavefront of (L - 1) x 2 light launches + 1 + 3 L + 2 eye launches + the acceptance test
        per_wavefront = 1 + 2 * (L - 1) + 1 + 3 * L + 2
        print(json.dumps({"tool": "time_pssmlt", "scene": "water_caustic-standin", "triangles": int(s.num_triangles), "resolution": [W, H], "max_path_length": L,
                          "n_chains": n_chains, "spp": args.spp, "chain_length": st["chain_length"], "render_s": [round(t, 4) for t in times], "median_s": round(med, 4),
                          "spread_s": round(max(times) - min(times), 4), "launches_per_call_approx": (st["chain_length"] + 1) * per_wavefront + st["chain_length"] + 6,
                          "mutations_per_s_M": round(st["chain_length"] * n_chains / med / 1e6, 2), "msample_per_s": round(args.spp * W * H / med / 1e6, 2),
                          "accepted": st["accepted"], "rejected": st["rejected"], "image_brightness": float(st["image_brightness"]),
                          "frame_finite": bool(np.isfinite(fb).all()), "frame_mean": float(fb.mean())}))
        r.close()


if __name__ == "__main__":
    main()
