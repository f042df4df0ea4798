#!/usr/bin/env python3
"""Time the two kFiltered denoisers on the same rendered frame: fpt_filter (the EAW chain: 2 x (variance + 7 a-trous steps)) and fpt_filter_xbl (2 x (variance + one
32-tap cross-bilateral step)), the latter in every layout its driver knows (FPT_XBL_LAYOUT 0 = plain, 1 = colour + normal planes, 2 = one 48-byte record per pixel, 3 = the colour plane alone).

Method: one process, one frame (the bench stand-in after --passes passes, 1600x900 unless told otherwise), every variant warmed up, then ROUNDS rounds in which the
variants take turns; a turn is K back-to-back calls between two device events on the library's stream.  Reported per variant: the median and the minimum over the
rounds of the per-call time, and the algorithmic bytes (what the definition must move: inputs read once, output written once) over the median.  The XBL layouts are
compared bit for bit before they are timed.  Without a GPU this fails; it does not fall back.

  python tools/time_filter.py [--res W H] [--passes N] [--rounds R] [--calls K] [--detail D] [--json out.json]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, nargs=2, default=(1600, 900))
    ap.add_argument("--passes", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--detail", type=float, default=0.3)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import torch
    import fermat_amd as fa
    from fermat_amd import scene
    if not torch.cuda.is_available():
        raise SystemExit("time_filter: no GPU")
    W, H = a.res
    r = fa.Renderer(scene.bathroom_standin(a.detail), W, H, fa.default_options(5))
    for i in range(a.passes):
        r.clear_gbuffer_async(); r.render_pass(i)
    r.synchronize()
    n = W * H
    stream = torch.cuda.ExternalStream(r.L.fpt_stream(r.ctx))

    def eaw():
        r._check(r.L.fpt_filter(r.ctx, C.byref(r.view), C.c_uint32(a.passes - 1)))

    def xbl(layout):
        def run():
            os.environ["FPT_XBL_LAYOUT"] = layout
            r._check(r.L.fpt_filter_xbl(r.ctx, C.byref(r.view), C.c_uint32(a.passes - 1)))
        return run
    d_var = torch.zeros(n, dtype=torch.float32, device=r.dev)

    def variance_twice():          # what both drivers spend on filter_variance: reported, not a filter
        for ch in (0, 2):
            r._check(r.L.fpt_filter_variance(r.ctx, C.c_uint32(W), C.c_uint32(H), C.c_void_p(r.fb[ch].data_ptr()), C.c_void_p(d_var.data_ptr()), C.c_uint32(2)))
    variants = [("variance_x2", variance_twice), ("eaw", eaw), ("xbl_plain", xbl("0")), ("xbl_planes", xbl("1")), ("xbl_record", xbl("2")), ("xbl_colour", xbl("3"))]
    # the layouts give one image
    frames = {}
    for name, fn in variants:
        fn(); r.synchronize()
        frames[name] = r.framebuffer()[6].copy()
    del frames["variance_x2"]
    same = all(np.array_equal(frames["xbl_plain"].view(np.uint32), frames[k].view(np.uint32)) for k in ("xbl_planes", "xbl_record", "xbl_colour"))
    assert same, "the XBL layouts differ"
    assert np.isfinite(frames["eaw"]).all() and np.isfinite(frames["xbl_plain"]).all() and frames["xbl_plain"][:, :3].max() > 0, "empty frame"
    times = {name: [] for name, _ in variants}
    with torch.cuda.stream(stream):
        for name, fn in variants:
            for _ in range(3):
                fn()
        r.synchronize()
        for _ in range(a.rounds):
            for name, fn in variants:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                for _ in range(a.calls):
                    fn()
                e1.record(stream); e1.synchronize()
                times[name].append(e0.elapsed_time(e1) / a.calls)
    # algorithmic bytes per pixel: the copy DIRECT_C -> FILTERED_C 32; per channel: variance 16 + 4, then
    #   EAW: first step 16 img + 16 w + 16 geo + 4 var + 16 dst = 68, five plain steps 52, last step 52 + 16 w + 16 dst read = 84
    #   XBL: 16 img + 16 w + 16 geo + 4 var + 8 shifts + 16 dst read + 16 dst write = 92
    alg = {"eaw": n * (32 + 2 * (20 + 68 + 5 * 52 + 84)), "xbl": n * (32 + 2 * (20 + 92))}
    res = {"res": [W, H], "passes": a.passes, "rounds": a.rounds, "calls_per_round": a.calls, "xbl_layouts_bit_identical": bool(same),
           "xbl_differs_from_eaw_rmse": float(np.sqrt(((frames["eaw"][:, :3].astype(np.float64) - frames["xbl_plain"][:, :3]) ** 2).mean()))}
    for name, _ in variants:
        t = times[name]; med = statistics.median(t)
        res[name] = {"median_ms": med, "min_ms": min(t), "max_ms": max(t)}
        if name != "variance_x2":
            res[name]["alg_gbs_at_median"] = alg["eaw" if name == "eaw" else "xbl"] / (med * 1e-3) / 1e9
    for name in ("xbl_plain", "xbl_planes", "xbl_record", "xbl_colour"):
        res[name]["speedup_over_eaw_median"] = res["eaw"]["median_ms"] / res[name]["median_ms"]
    print(json.dumps(res))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)
    r.close()


if __name__ == "__main__":
    main()
