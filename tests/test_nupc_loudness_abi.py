"""CPU: the BS.1770 loudness meter of the non-uniform convolver (include/bfhip_nupc.h) is exported, declared and
bound in Python; its calls fail cleanly on a NULL handle and leave their out-parameters alone; the selftests --
host code that needs no device -- reject bad arguments; and csrc/loudness_host.h, built into a stand-alone program
with the address and undefined-behaviour sanitizers, runs clean.  What needs a live convolver:
tests/test_gpu_nupc_loudness.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import brutefir_amd as bf

CALLS = ["bfhip_nupc_enable_loudness", "bfhip_nupc_add_loudness_group", "bfhip_nupc_get_loudness",
         "bfhip_nupc_get_loudness_energy", "bfhip_nupc_reset_loudness", "bfhip_selftest_kweighting",
         "bfhip_selftest_loudness_energy", "bfhip_selftest_loudness_gate"]
EINVAL = -1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "bfhip_nupc.h")


@pytest.mark.parametrize("name", CALLS)
def test_calls_are_exported(name):
    assert hasattr(C.CDLL(bf.LIB_PATH), name)


def test_calls_and_constants_are_declared():
    text = open(HEADER).read()
    for name in CALLS:
        assert re.search(r"\bint %s\(" % name, text), name
    for name, value in [("GROUPS_MAX", 32), ("GROUP_MAX", 16)]:
        assert re.search(r"#define BFHIP_NUPC_LOUD_%s +%d\b" % (name, value), text), name
    assert re.search(r"\}\s*bfhip_loudness;", text)


def test_binding_has_the_methods():
    for meth in ("enable_loudness", "add_loudness_group", "loudness", "loudness_energy", "reset_loudness"):
        assert callable(getattr(bf.Nupc, meth, None)), meth
    for fn in ("kweighting", "loudness_energy", "loudness_gate"):
        assert callable(getattr(bf, fn, None)), fn
    assert bf.Loudness._fields == ("momentary", "short_term", "integrated", "subblocks", "first", "wrapped")


def _untouched():
    s = bf.LoudnessStruct(-3.0, -4.0, -5.0, 7, 8, 9)
    return s, lambda: (s.momentary, s.short_term, s.integrated, s.subblocks, s.first, s.wrapped) == (-3.0, -4.0, -5.0, 7, 8, 9)


def test_calls_fail_on_a_null_handle():
    L = bf.lib()
    two = (C.c_int * 2)(0, 1)
    w = (C.c_double * 2)(1.0, 1.0)
    e = np.full(4, -1.0)
    s, same = _untouched()
    assert L.bfhip_nupc_enable_loudness(None, 48000, 36000) == EINVAL
    assert L.bfhip_nupc_add_loudness_group(None, two, w, 2) == EINVAL
    assert L.bfhip_nupc_add_loudness_group(None, two, None, 2) == EINVAL
    assert L.bfhip_nupc_get_loudness(None, 0, C.byref(s)) == EINVAL and same()
    assert L.bfhip_nupc_get_loudness_energy(None, 0, 0, 4, e.ctypes.data_as(C.POINTER(C.c_double))) == EINVAL
    assert np.all(e == -1.0)
    assert L.bfhip_nupc_reset_loudness(None, 0) == EINVAL
    assert L.bfhip_nupc_last_error()


def test_selftests_reject_bad_arguments():
    L = bf.lib()
    dp = C.POINTER(C.c_double)
    c = np.full(10, -1.0)
    for rate in (8001, 7990, 0, -48000, 768010):
        assert L.bfhip_selftest_kweighting(rate, c.ctypes.data_as(dp)) == EINVAL, rate
        assert np.all(c == -1.0)
    assert L.bfhip_selftest_kweighting(48000, None) == EINVAL
    assert L.bfhip_selftest_kweighting(48000, c.ctypes.data_as(dp)) == 0 and c[5:8].tolist() == [1.0, -2.0, 1.0]
    v = np.full(1700, 0.5)
    E = np.full(3, -1.0)
    vp_, Ep = v.ctypes.data_as(dp), E.ctypes.data_as(dp)
    for rate, n, a, b in [(8001, 1700, vp_, Ep), (7990, 1700, vp_, Ep), (8000, -1, vp_, Ep), (8000, 1700, None, Ep),
                          (8000, 1700, vp_, None)]:
        assert L.bfhip_selftest_loudness_energy(rate, n, a, b) == EINVAL, (rate, n)
        assert np.all(E == -1.0)
    assert L.bfhip_selftest_loudness_energy(8000, 1700, vp_, Ep) == 2 and E[0] > 0 and E[1] > 0 and E[2] == -1.0
    s, same = _untouched()
    E4 = np.full(4, 80.0)
    for rate, n, a, out in [(8001, 4, E4.ctypes.data_as(dp), C.byref(s)), (7990, 4, E4.ctypes.data_as(dp), C.byref(s)),
                            (8000, -1, E4.ctypes.data_as(dp), C.byref(s)), (8000, 4, None, C.byref(s)),
                            (8000, 4, E4.ctypes.data_as(dp), None)]:
        assert L.bfhip_selftest_loudness_gate(rate, n, a, out) == EINVAL, (rate, n)
        assert same()
    assert L.bfhip_selftest_loudness_gate(8000, 4, E4.ctypes.data_as(dp), C.byref(s)) == 0
    assert s.subblocks == 4 and abs(s.momentary - (-0.691 - 10.0)) < 1e-12 and s.short_term == float("-inf")
    with pytest.raises(bf.BfhipError):
        bf.kweighting(8001)
    with pytest.raises(bf.BfhipError):
        bf.loudness_energy(7990, v)
    with pytest.raises(bf.BfhipError):
        bf.loudness_gate(8001, E4)


def test_host_code_runs_clean_under_sanitizers(tmp_path):
    """the checks, the design, the energies and the read-outs are plain host code (csrc/loudness_host.h):
    tests/loudness_host_check.cpp is a program of its own around them, built here with
    -fsanitize=address,undefined and run on the CPU"""
    exe = str(tmp_path / "loudness_host_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "loudness_host_check.cpp"), "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout
