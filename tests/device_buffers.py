"""Device buffers for the GPU tests, through the HIP runtime the library itself runs on (torch is not needed for them)."""
import ctypes as C

import numpy as np


class Device:
    """put() / fill() allocate and return device addresses (ints); free() releases everything allocated through this object."""

    def __init__(self):
        self.hip = C.CDLL("libamdhip64.so")
        self.hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        self.hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        self.hip.hipFree.argtypes = [C.c_void_p]
        self.bufs = []

    def put(self, a):
        a = np.ascontiguousarray(a, dtype=np.float64)
        p = C.c_void_p()
        assert self.hip.hipMalloc(C.byref(p), max(a.nbytes, 8)) == 0
        self.bufs.append(p.value)
        assert self.hip.hipMemcpy(p, C.c_void_p(a.ctypes.data), a.nbytes, 1) == 0
        return p.value

    def fill(self, n, value):
        """n doubles (at least one, so that the address is never NULL) of `value`"""
        return self.put(np.full(max(int(n), 1), value))

    def write(self, ptr, a, offset=0):
        """a -> ptr[offset : offset + len(a)] (doubles)"""
        a = np.ascontiguousarray(a, dtype=np.float64)
        if a.nbytes:
            assert self.hip.hipMemcpy(C.c_void_p(ptr + 8 * int(offset)), C.c_void_p(a.ctypes.data), a.nbytes, 1) == 0

    def get(self, ptr, n):
        out = np.empty(n)
        if n:
            assert self.hip.hipMemcpy(C.c_void_p(out.ctypes.data), C.c_void_p(ptr), out.nbytes, 2) == 0
        return out

    def free(self):
        for p in self.bufs:
            self.hip.hipFree(C.c_void_p(p))
        self.bufs = []
