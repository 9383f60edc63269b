"""What the host core tests (test_*_core_host.py, test_stage_plan_host.py, test_decode_scheme.py) share: the build of a tests/host/ source as a
shared library bound with ctypes, its build as a stand-alone program under the address and undefined-behaviour sanitizers (a program of its
own with the sanitizer runtimes linked statically: nothing sanitized is loaded into the test process), and the guarded output array the
checking memory functors of tests/host/host_mem.h write into.  A new core's test starts from these."""
import ctypes
import os
import subprocess

import numpy as np

HOST = os.path.join(os.path.dirname(os.path.abspath(__file__)), "host")
GUARD = 0xA5
BASE = 1 << 20                      # the virtual address of out[0]: a multiple of 16
BAND = 48

u8, u32, u64, f32 = ctypes.c_uint8, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_float
cint, cuint, i64, ull = ctypes.c_int, ctypes.c_uint, ctypes.c_longlong, ctypes.c_ulonglong
u8p, u32p, u64p, f32p = ctypes.POINTER(u8), ctypes.POINTER(u32), ctypes.POINTER(u64), ctypes.POINTER(f32)
cintp, i64p, ullp = ctypes.POINTER(cint), ctypes.POINTER(i64), ctypes.POINTER(ull)

WARNINGS = ("-Wall", "-Werror")


def shared(source, tmp, symbols, warnings=WARNINGS):
    """tests/host/<source> as a shared library in tmp (a directory or tmp_path_factory); symbols: {name: (restype, [argtypes])}"""
    stem = os.path.splitext(source)[0]
    tmp = tmp.mktemp(stem) if hasattr(tmp, "mktemp") else tmp
    out = os.path.join(str(tmp), "lib%s.so" % stem)
    subprocess.run(["g++", "-O2", "-std=c++17", *warnings, "-shared", "-fPIC", "-o", out, os.path.join(HOST, source)], check=True)
    lib = ctypes.CDLL(out)
    for name, (restype, argtypes) in symbols.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, argtypes
    return lib


def sanitized(source, define, tmp_path):
    """tests/host/<source> with -D<define> (its own main()) built under the sanitizers and run directly; returns its stdout"""
    exe = os.path.join(str(tmp_path), os.path.splitext(source)[0] + "_main")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", *WARNINGS, "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                    "-D" + define, "-o", exe, os.path.join(HOST, source)], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout[-400:], r.stderr[-2000:])
    assert "runtime error" not in r.stderr, r.stderr[-2000:]
    return r.stdout


class Banded:
    """B output bytes at BASE + band + a between two bands of GUARD, and the count of the writes to each byte.  args: what every _run of
    tests/host/ takes for them: q, base, out, writes, out_len."""

    def __init__(self, B, a, band=BAND):
        self.lo, self.hi = band + a, band + a + B
        self.out = np.full(self.hi + band, GUARD, dtype=np.uint8)
        self.writes = np.zeros(self.out.size, dtype=np.uint8)
        self.q = BASE + self.lo
        self.args = (self.q, BASE, self.out.ctypes.data_as(u8p), self.writes.ctypes.data_as(u8p), self.out.size)

    def inside(self, what):
        """the output bytes, once every one of them is written exactly once, none beside them is written and the bands still hold GUARD"""
        lo, hi = self.lo, self.hi
        assert np.all(self.writes[lo:hi] == 1) and not self.writes[:lo].any() and not self.writes[hi:].any(), what
        assert np.all(self.out[:lo] == GUARD) and np.all(self.out[hi:] == GUARD), what
        return self.out[lo:hi]
