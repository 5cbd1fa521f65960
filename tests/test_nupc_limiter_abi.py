"""CPU: the look-ahead peak limiter of the non-uniform convolver (include/bfhip_nupc.h) is exported, declared
and bound in Python; its calls fail cleanly on a NULL handle; the selftest -- host code that needs no device
-- rejects bad arguments; and csrc/limiter_host.h, built into a stand-alone program with the address and
undefined-behaviour sanitizers, runs clean.  What needs a live convolver: tests/test_gpu_nupc_limiter.py."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import brutefir_amd as bf

CALLS = ["bfhip_nupc_enable_limiter", "bfhip_nupc_add_limiter_group", "bfhip_nupc_set_limiter_threshold",
         "bfhip_nupc_get_limiter_threshold", "bfhip_nupc_limiter_delay", "bfhip_nupc_get_limiter_reduction",
         "bfhip_selftest_limiter_envelope"]
EINVAL = -1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "bfhip_nupc.h")


@pytest.mark.parametrize("name", CALLS)
def test_calls_are_exported(name):
    assert hasattr(C.CDLL(bf.LIB_PATH), name)


def test_calls_and_constants_are_declared():
    text = open(HEADER).read()
    for name in CALLS:
        assert re.search(r"\b(int|double) %s\(" % name, text), name
    for name, value in [("LOOKAHEAD_MAX", 1024), ("GROUPS_MAX", 32), ("GROUP_MAX", 8)]:
        assert re.search(r"#define BFHIP_NUPC_LIMIT_%s +%d\b" % (name, value), text), name


def test_binding_has_the_methods():
    for meth in ("enable_limiter", "add_limiter_group", "set_limiter_threshold", "limiter_threshold", "limiter_delay",
                 "limiter_reduction"):
        assert callable(getattr(bf.Nupc, meth, None)), meth
    assert callable(bf.limiter_envelope)


def test_calls_fail_on_a_null_handle():
    L = bf.lib()
    two = (C.c_int * 2)(0, 1)
    v = C.c_double(-3.0)
    assert L.bfhip_nupc_enable_limiter(None, 16, 50.0) == EINVAL
    assert L.bfhip_nupc_add_limiter_group(None, two, 2, 0.5) == EINVAL
    assert L.bfhip_nupc_set_limiter_threshold(None, 0, 0.5) == EINVAL
    assert math.isnan(L.bfhip_nupc_get_limiter_threshold(None, 0))
    assert L.bfhip_nupc_limiter_delay(None) == EINVAL
    assert L.bfhip_nupc_get_limiter_reduction(None, 0, C.byref(v)) == EINVAL and v.value == -3.0
    assert L.bfhip_nupc_last_error()


def test_selftest_rejects_bad_arguments():
    L = bf.lib()
    dp = C.POINTER(C.c_double)
    p = np.array([0.5, 2.0, 0.5])
    s = np.full(3, -1.0)
    pp, sp = p.ctypes.data_as(dp), s.ctypes.data_as(dp)
    for D, release, n, a, b in [(0, 0.0, 3, pp, sp), (1025, 0.0, 3, pp, sp), (4, 0.5, 3, pp, sp), (4, -1.0, 3, pp, sp),
                                (4, float("nan"), 3, pp, sp), (4, float("inf"), 3, pp, sp), (4, 2e7, 3, pp, sp),
                                (4, 0.0, -1, pp, sp), (4, 0.0, 3, None, sp), (4, 0.0, 3, pp, None)]:
        assert L.bfhip_selftest_limiter_envelope(D, release, n, a, b) == EINVAL, (D, release, n)
        assert np.all(s == -1.0)
    assert L.bfhip_selftest_limiter_envelope(1, 0.0, 3, pp, sp) == 0
    assert list(s) == [1.0, 0.75, 0.5]                 # e = 1, 1/2, 1/2 (the minimum looks one frame back)
    with pytest.raises(bf.BfhipError):
        bf.limiter_envelope(0, 0.0, p)


def test_host_code_runs_clean_under_sanitizers(tmp_path):
    """the checks and the envelope are plain host code (csrc/limiter_host.h): tests/limiter_host_check.cpp is a
    program of its own around them, built here with -fsanitize=address,undefined and run on the CPU"""
    exe = str(tmp_path / "limiter_host_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "limiter_host_check.cpp"), "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout
