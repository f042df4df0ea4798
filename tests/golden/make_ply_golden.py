#!/usr/bin/env python3
"""Regenerates tests/golden/ply_cases.npz: what the reference's own PLY parser (rply 1.01, driven like MeshBase::loadFromPly by
oracle/_ref/ply_dump -- `make -C oracle ref`, needs /root/reference) returns for the files of tests/ply_cases.py, and
tests/golden/ply_models.json: the digests of what it returns for the reference's material-testball models (shipped byte-identical
under fermat_amd/data/scenes/testball_room).
Run from the repo root in the build container:  python tests/golden/make_ply_golden.py"""
import hashlib, json, os, subprocess, sys, tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ply_cases


def ref_dump(path):
    exe = os.path.join(ROOT, "oracle", "_ref", "ply_dump")
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "o.bin")
        if subprocess.call([exe, path, out]) != 0:
            return None
        b = open(out, "rb").read()
    nv, nn, nt, ntri = np.frombuffer(b, np.int32, 4)
    o = 16
    P = np.frombuffer(b, np.float32, nv * 3, o).reshape(-1, 3); o += nv * 12
    N = np.frombuffer(b, np.float32, nn * 3, o).reshape(-1, 3); o += nn * 12
    T = np.frombuffer(b, np.float32, nt * 2, o).reshape(-1, 2); o += nt * 8
    tri = np.frombuffer(b, np.int32, ntri * 3, o).reshape(-1, 3)
    return dict(P=P.copy(), N=N.copy(), T=T.copy(), tri=tri.copy())


def digest(a):
    """[shape, sha256 of the bytes]: tests/test_ply.py computes the same of the loaders' float32 / int32 arrays"""
    a = np.ascontiguousarray(a)
    return [list(a.shape), hashlib.sha256(a.tobytes()).hexdigest()]


if __name__ == "__main__":
    models = {}
    for name in ("Mesh000", "Mesh001", "Mesh002"):
        path = os.path.join(ROOT, "fermat_amd", "data", "scenes", "testball_room", name + ".ply")
        r = ref_dump(path)
        assert r is not None, name
        models[name] = dict(file_sha256=hashlib.sha256(open(path, "rb").read()).hexdigest(), **{k: digest(v) for k, v in r.items()})
        print(name, {k: v.shape for k, v in r.items()})
    with open(os.path.join(ROOT, "tests", "golden", "ply_models.json"), "w") as f:
        json.dump(models, f, indent=1)
        f.write("\n")
    with tempfile.TemporaryDirectory() as d:
        files = ply_cases.cases(d)
        out = {}
        for name, path in files.items():
            r = ref_dump(path)
            assert r is not None, name
            for k, v in r.items():
                out[name + "." + k] = v
            print(name, {k: v.shape for k, v in r.items()})
    np.savez_compressed(os.path.join(ROOT, "tests", "golden", "ply_cases.npz"), **out)
