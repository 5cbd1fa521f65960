"""CPU: the limiter's true-peak detector (include/bfhip_nupc.h) is exported, declared and bound in Python; its
calls fail cleanly on a NULL handle; the selftests -- host code that needs no device -- reject bad arguments;
and csrc/truepeak_host.h, built into a stand-alone program with the address and undefined-behaviour
sanitizers, runs clean.  That program holds the detector check at both sides of its limit (a look-ahead of 23
is refused with a message that names 24, 24 is accepted, other detector values are refused) through the very
function bfhip_nupc_set_limiter_detector calls.  A convolver handle cannot be made without a device
(bfhip_nupc_create opens it), so the state rules on a live handle are in tests/test_gpu_nupc_truepeak.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import brutefir_amd as bf

CALLS = ["bfhip_nupc_set_limiter_detector", "bfhip_nupc_get_limiter_detector", "bfhip_nupc_get_limiter_true_peak",
         "bfhip_selftest_truepeak_filter", "bfhip_selftest_truepeak"]
EINVAL = -1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "bfhip_nupc.h")


def test_calls_are_exported():
    L = C.CDLL(bf.LIB_PATH)
    for name in CALLS:
        assert hasattr(L, name), name


def test_calls_and_constants_are_declared():
    text = open(HEADER).read()
    for name in CALLS:
        assert re.search(r"\bint %s\(" % name, text), name
    for name, value in [("SAMPLE_PEAK", 0), ("TRUE_PEAK", 1), ("TP_HALF", 12)]:
        assert re.search(r"#define BFHIP_NUPC_LIMIT_%s +%d\b" % (name, value), text), name
    assert (bf.LIMIT_SAMPLE_PEAK, bf.LIMIT_TRUE_PEAK, bf.LIMIT_TP_HALF) == (0, 1, 12)


def test_binding_has_the_methods():
    for meth in ("set_limiter_detector", "limiter_detector", "limiter_true_peak"):
        assert callable(getattr(bf.Nupc, meth, None)), meth
    assert callable(bf.truepeak_filter) and callable(bf.truepeak)


def test_calls_fail_on_a_null_handle():
    L = bf.lib()
    v = C.c_double(-3.0)
    assert L.bfhip_nupc_set_limiter_detector(None, 1) == EINVAL
    assert L.bfhip_nupc_get_limiter_detector(None) == EINVAL
    assert L.bfhip_nupc_get_limiter_true_peak(None, 0, C.byref(v)) == EINVAL and v.value == -3.0
    assert L.bfhip_nupc_last_error()


def test_selftests_reject_bad_arguments():
    L = bf.lib()
    dp = C.POINTER(C.c_double)
    x = np.array([0.5, 2.0, 0.5])
    tp = np.full(3, -1.0)
    xp, tpp = x.ctypes.data_as(dp), tp.ctypes.data_as(dp)
    for n, a, b in [(-1, xp, tpp), (3, None, tpp), (3, xp, None)]:
        assert L.bfhip_selftest_truepeak(n, a, b) == EINVAL, n
        assert np.all(tp == -1.0)
    assert L.bfhip_selftest_truepeak_filter(None) == EINVAL
    assert L.bfhip_selftest_truepeak(0, None, None) == 0
    assert L.bfhip_selftest_truepeak(3, xp, tpp) == 0
    g = bf.truepeak_filter()
    # three frames in: only taps 0 .. 2 have met a sample, phase 0 is still in front of frame 0
    want = [np.abs(g[:, :t + 1] @ x[t::-1]).max() for t in range(3)]
    assert np.allclose(tp, want, rtol=1e-15, atol=0)


def test_host_code_runs_clean_under_sanitizers(tmp_path):
    """taps, checks and the detector are plain host code (csrc/truepeak_host.h): tests/truepeak_host_check.cpp is
    a program of its own around them, built here with -fsanitize=address,undefined and run on the CPU"""
    exe = str(tmp_path / "truepeak_host_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "truepeak_host_check.cpp"), "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout
