"""kmws_resident_utf8_counters (include/kmws_bench.h) without a GPU: the
library exports it, bind() sets its signature, a device the process does not
have gives KMWS_ERR_INVALID_PARAM and leaves the outputs alone, and NULL
out-pointers are accepted."""
import ctypes as C
import os
import re

from kuma_amd import kmws

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = 0x5EA15EA15EA15EA1


def test_exported_declared_and_listed():
    assert hasattr(kmws.lib(), "kmws_resident_utf8_counters")
    assert "kmws_resident_utf8_counters" in kmws.BENCH_EXPORTS
    with open(os.path.join(ROOT, "include", "kmws_bench.h")) as f:
        assert re.search(r"kmws_status\s+kmws_resident_utf8_counters\s*\(\s*int device,\s*uint64_t\*\s*checked_jobs,"
                         r"\s*uint64_t\*\s*variant_switches\)", f.read())


def test_bind_sets_the_signature():
    fn = kmws.lib().kmws_resident_utf8_counters
    assert fn.restype is C.c_int
    assert list(fn.argtypes) == [C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    # a library loaded by path gets it from bind() too
    L = kmws.bind(C.CDLL(kmws.lib_path()))
    assert list(L.kmws_resident_utf8_counters.argtypes) == [C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]


def test_a_device_the_process_does_not_have():
    fn = kmws.lib().kmws_resident_utf8_counters
    for device in (kmws.device_count(), -1, 64, 1 << 20, -(1 << 20)):
        a, b = C.c_uint64(SENTINEL), C.c_uint64(SENTINEL)
        assert fn(device, C.byref(a), C.byref(b)) == kmws.ERR_INVALID_PARAM, device
        assert a.value == SENTINEL and b.value == SENTINEL, device
        assert fn(device, None, None) == kmws.ERR_INVALID_PARAM, device


def test_null_out_pointers_are_skipped():
    fn = kmws.lib().kmws_resident_utf8_counters
    want = kmws.OK if kmws.device_count() > 0 else kmws.ERR_INVALID_PARAM
    a = C.c_uint64(SENTINEL)
    assert fn(0, None, None) == want
    assert fn(0, C.byref(a), None) == want
    assert fn(0, None, C.byref(a)) == want
    assert (a.value != SENTINEL) == (want == kmws.OK)


def test_python_wrapper_raises_without_a_device():
    if kmws.device_count() > 0:
        assert set(kmws.resident_utf8()) == {"checked_jobs", "variant_switches"}
        return
    try:
        kmws.resident_utf8()
    except kmws.KmwsError as e:
        assert e.status == kmws.ERR_INVALID_PARAM
    else:
        raise AssertionError("resident_utf8() succeeded without a device")
