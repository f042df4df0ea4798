"""CPU tests of the XBL part of the C-ABI: include/fermat_pt_hip.h still compiles as C99 with fpt_xbl_params and the two entry points in it, the ctypes mirror has the
C size and field offsets, and the built library exports fpt_xbl and fpt_filter_xbl.  No compute entry point is called here."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

import fermat_amd as fa
from fermat_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_the_xbl_entry_points():
    L = fa.lib()
    for n in ("fpt_xbl", "fpt_filter_xbl"):
        assert n in api.ENTRY_POINTS and hasattr(L, n), "missing export: " + n


def test_header_is_plain_c_with_the_xbl_declarations(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    fields = ("phi_normal", "phi_position", "phi_color", "taps", "E", "U", "V", "W")
    inc = os.path.join(ROOT, "include")
    # the declarations, used as a C host would: compiled, not linked
    use = tmp_path / "use.c"
    use.write_text('#include "fermat_pt_hip.h"\n'
                   "int filter_both(fpt_context* ctx, const fpt_rendering_context_view* v, float* dst, const float* img, const float* geo, const float* shifts) {\n"
                   "  fpt_xbl_params p = { 32.0f, 1.0f, 0.0f, 32u, {0, 0, 0}, {1, 0, 0}, {0, 1, 0}, {0, 0, -1} };\n"
                   "  int (*one)(fpt_context*, uint32_t, uint32_t, float*, uint32_t, const float*, float, const float*, const float*, const float*, const fpt_xbl_params*, uint32_t, uint32_t,\n"
                   "             const float*, uint32_t) = fpt_xbl;\n"
                   "  int (*all)(fpt_context*, const fpt_rendering_context_view*, uint32_t) = fpt_filter_xbl;\n"
                   "  return one(ctx, v->res_x, v->res_y, dst, FPT_FILTER_OP_REPLACE_MODE, 0, 0.0f, img, geo, 0, &p, 21u, 1u, shifts, 256u) | all(ctx, v, 0u); }\n")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", inc, "-c", "-o", str(tmp_path / "use.o"), str(use)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    # the layout the C compiler gives the struct
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "fermat_pt_hip.h"\nint main(void) {\n  printf("size %zu\\n", sizeof(fpt_xbl_params));\n' +
                   "".join('  printf("%s %%zu\\n", offsetof(fpt_xbl_params, %s));\n' % (f, f) for f in fields) + "  return 0; }\n")
    exe = tmp_path / "layout"
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", inc, "-o", str(exe), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    got = dict((l.split()[0], int(l.split()[1])) for l in out.stdout.splitlines())
    assert got["size"] == C.sizeof(api.XblParams) == 64
    for f in fields:
        assert got[f] == getattr(api.XblParams, f).offset, f
