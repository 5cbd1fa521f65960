"""CPU: the parametric-equaliser sections of the non-uniform convolver (bfhip_nupc_render_biquads* and
bfhip_biquad_design, include/bfhip_nupc.h) are exported, bound in Python, and fail cleanly on a NULL handle;
the designer -- host code that needs no device -- equals the float64 model (tests/biquad_ref.py) and answers
its argument errors without touching coef; and the designer and the section check, built into a
stand-alone program with the address and undefined-behaviour sanitizers, run clean.  What needs a live
convolver: tests/test_gpu_nupc_biquads.py."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import biquad_ref
import brutefir_amd as bf

CALLS = ["bfhip_nupc_render_biquads", "bfhip_nupc_render_biquads_async", "bfhip_nupc_render_biquads_base",
         "bfhip_nupc_render_biquads_base_async", "bfhip_nupc_render_biquads_group_async"]
EINVAL = -1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "bfhip_nupc.h")
F0 = [15.0 / 48000.0, 0.01, 0.25, 0.49]


@pytest.mark.parametrize("name", CALLS + ["bfhip_biquad_design"])
def test_calls_are_exported(name):
    assert hasattr(C.CDLL(bf.LIB_PATH), name)


def test_calls_and_constants_are_declared():
    text = open(HEADER).read()
    for name in CALLS:
        assert re.search(r"\bint %s\(bfhip_nupc \*n," % name, text), name
    assert re.search(r"\bint bfhip_biquad_design\(int type, double f0, double gain_db, double q, double coef\[5\]\);", text)
    for name, value in [("MAX", 32), ("OWN", 0), ("LINEAR", 1), ("PEAK", 0), ("LOW_SHELF", 1), ("HIGH_SHELF", 2),
                        ("LOW_PASS", 3), ("HIGH_PASS", 4), ("NOTCH", 5), ("ALL_PASS", 6)]:
        assert re.search(r"#define BFHIP_BIQUAD_%s +%d\b" % (name, value), text), name


def test_binding_has_the_methods_and_constants():
    for meth in ("render_biquads", "render_biquads_async", "render_biquads_base", "render_biquads_base_async",
                 "render_biquads_group_async"):
        assert callable(getattr(bf.Nupc, meth, None)), meth
        par = inspect.signature(getattr(bf.Nupc, meth)).parameters
        assert list(par)[-2:] == ["sections", "phase"] and par["phase"].default == "own", meth
    assert (bf.BIQUAD_OWN, bf.BIQUAD_LINEAR) == (0, 1) and bf.BIQUAD_PHASES == {"own": 0, "linear": 1}
    assert (bf.BIQUAD_PEAK, bf.BIQUAD_LOW_SHELF, bf.BIQUAD_HIGH_SHELF, bf.BIQUAD_LOW_PASS, bf.BIQUAD_HIGH_PASS,
            bf.BIQUAD_NOTCH, bf.BIQUAD_ALL_PASS) == tuple(range(7))
    assert callable(bf.biquad_design)
    assert bf.EQ_MODES == {"linear": 0, "minimum": 1}                  # the band modes are a namespace apart


def test_calls_fail_on_a_null_handle():
    L = bf.lib()
    coef = (C.c_double * 5)(1.0, 0.0, 0.0, 0.0, 0.0)
    two = (C.c_int * 2)(0, 1)
    out = (C.c_double * 8)()
    for call in (lambda: L.bfhip_nupc_render_biquads(None, 8, 1, coef, 0, out),
                 lambda: L.bfhip_nupc_render_biquads_async(None, 0, 1, 8, 1, coef, 0),
                 lambda: L.bfhip_nupc_render_biquads_base(None, 0, 8, 1, coef, 1, out),
                 lambda: L.bfhip_nupc_render_biquads_base_async(None, 0, 1, 8, 1, coef, 0),
                 lambda: L.bfhip_nupc_render_biquads_group_async(None, 2, two, two, two, 8, 1, coef, 0),
                 lambda: L.bfhip_nupc_render_biquads_group_async(None, 2, two, two, None, 8, 1, coef, 1)):
        L.bfhip_nupc_set_format(None, 0, 0, None)              # leaves another text behind
        assert call() < 0
        assert b"null" in L.bfhip_nupc_last_error()


@pytest.mark.parametrize("type", range(7))
def test_designer_is_the_models(type):
    """both sides evaluate the same well-conditioned formulas: 1e-13 max|coef| covers the few ulp by which two
    math libraries' sin / cos / pow differ"""
    for f0 in F0:
        for gain_db, q in [(6.0, 0.707), (-9.0, 8.0), (0.0, 30.0)]:
            got = bf.biquad_design(type, f0, gain_db, q)
            want = biquad_ref.design(type, f0, gain_db, q)
            assert got.dtype == np.float64 and got.shape == (5,)
            err = np.abs(got - want).max()
            assert err <= 1e-13 * np.abs(want).max(), (f0, gain_db, q, err)
            assert biquad_ref.stable(got)


def test_designer_ignores_gain_where_the_type_has_none():
    for type in (bf.BIQUAD_LOW_PASS, bf.BIQUAD_HIGH_PASS, bf.BIQUAD_NOTCH, bf.BIQUAD_ALL_PASS):
        assert np.array_equal(bf.biquad_design(type, 0.1, 0.0, 2.0), bf.biquad_design(type, 0.1, -7.5, 2.0))


def test_designer_errors_leave_coef_untouched():
    L = bf.lib()
    nan, inf = float("nan"), float("inf")
    coef = (C.c_double * 5)(*[7.0] * 5)
    bad = [(-1, 0.1, 0.0, 1.0), (7, 0.1, 0.0, 1.0), (0, 0.0, 0.0, 1.0), (0, -0.1, 0.0, 1.0), (0, 0.5, 0.0, 1.0),
           (0, 0.6, 0.0, 1.0), (0, nan, 0.0, 1.0), (0, 0.1, 0.0, 0.0), (0, 0.1, 0.0, -2.0), (0, 0.1, 0.0, nan),
           (0, 0.1, nan, 1.0), (0, 0.1, inf, 1.0), (0, 0.1, -inf, 1.0)]
    for args in bad:
        assert L.bfhip_biquad_design(*args, coef) == EINVAL, args
        assert list(coef) == [7.0] * 5, args
    assert L.bfhip_biquad_design(0, 0.1, 0.0, 1.0, None) == EINVAL
    assert b"biquad_design" in L.bfhip_nupc_last_error()
    with pytest.raises(bf.BfhipError):
        bf.biquad_design(0, 0.5, 0.0, 1.0)
    assert L.bfhip_biquad_design(0, 0.1, 0.0, 1.0, coef) == 0 and list(coef) != [7.0] * 5


def test_host_code_runs_clean_under_the_sanitizers(tmp_path):
    """the designer and the section check are plain host code (csrc/biquad_host.h): tests/biquad_host_check.cpp
    is a program of its own around them, built here with -fsanitize=address,undefined and run on the CPU"""
    exe = str(tmp_path / "biquad_host_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "biquad_host_check.cpp"), "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout
