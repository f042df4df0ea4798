#!/usr/bin/env python3
"""The miss share of the path queues, bounce by bounce (EXPERIMENTS B6): on bench.py's configuration -- its scene, 1600 x 900, 9-vertex paths -- one pass is rendered per
bounce with the queue that ENTERS the bounce captured (Renderer.set_capture: the route with a hit record per ray), and the entries with t > 0 and triId >= 0 are
counted.  Prints one JSON line: per bounce the entries, the hits and the miss share; the totals over bounces >= 1, which is what the hit list of the passes in flight
takes out of the shading launches.
    python tools/miss_share.py [--workload bathroom2|standin|testball-room] [--instance 0]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
import fermat_amd as fa  # noqa: E402
from fermat_amd import scene  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--workload", default="bathroom2")
ap.add_argument("--instance", type=int, default=0)
ap.add_argument("--detail", type=float, default=1.0)
a = ap.parse_args()
W, H = bench.CONFIGS["c3"]
s, _ = bench.load_workload(scene, a, (W, H))
r = fa.Renderer(s, W, H, fa.default_options(bench.MAX_PATH_LENGTH), device=0, gbuffer=True)
rows = []
for bounce in range(bench.MAX_PATH_LENGTH):
    r.set_capture(bounce)
    r.render_pass(a.instance, sync=True)
    h = r.captured()["hits"]
    hits = int(((h["t"] > 0) & (h["triId"] >= 0)).sum())
    rows.append({"bounce": bounce, "entries": int(len(h)), "hits": hits, "miss_share": round(1.0 - hits / len(h), 4) if len(h) else None})
    if not len(h):
        break
r.set_capture(-1)
r.close()
later = [x for x in rows if x["bounce"] >= 1]
e, k = sum(x["entries"] for x in later), sum(x["hits"] for x in later)
print(json.dumps({"workload": a.workload, "resolution": [W, H], "instance": a.instance, "bounces": rows,
                  "bounces_ge_1": {"entries": e, "hits": k, "miss_share": round(1.0 - k / e, 4) if e else None},
                  "all": {"entries": e + rows[0]["entries"], "hits": k + rows[0]["hits"]}}))
