"""The segment kernels' geometry as the kernels compile it (finch_rs_amd/csrc/fh_core.h: seg_sub_for, seg_geom, seg_lane_take,
segw_geom ...), from the host build of that header which tests/test_core_logic_host.py also uses.  No GPU needed."""
import ctypes as C
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
FAILS = {1: "a tile offset nobody takes", 2: "a tile offset taken twice", 3: "a lane takes more than a round holds", 4: "a position outside the tile",
         5: "a view that leaves the tile's strings", 6: "LDS words outside the strings' blocks", 7: "a resume round that does not partition the tile",
         8: "no such kernel form"}


class SegModel:
    def __init__(self, extra_flags=(), so_name="libfhcore_host.so"):
        src = os.path.join(HERE, "hostcore", "fhcore_host.cpp")
        so = os.path.join(HERE, "hostcore", so_name)
        hdr = os.path.join(HERE, "..", "finch_rs_amd", "csrc", "fh_core.h")
        if (not os.path.exists(so)) or os.path.getmtime(so) < max(os.path.getmtime(src), os.path.getmtime(hdr)):
            tmp = "%s.tmp.%d" % (so, os.getpid())
            subprocess.check_call(["g++", "-O1", "-std=c++17", "-shared", "-fPIC"] + list(extra_flags) + ["-o", tmp, src])
            os.replace(tmp, so)
        L = self.L = C.CDLL(so)
        L.fhcore_seg_check.restype = C.c_int
        L.fhcore_seg_check.argtypes = [C.c_uint32] * 3 + [C.c_void_p]
        L.fhcore_seg_sub_for.restype = C.c_uint32
        L.fhcore_seg_sub_for.argtypes = [C.c_uint32] * 2
        L.fhcore_seg_launch_ok.restype = C.c_int
        L.fhcore_seg_launch_ok.argtypes = [C.c_uint32] * 3
        L.fhcore_seg_geom.restype = None
        L.fhcore_seg_geom.argtypes = [C.c_uint32] * 3 + [C.c_void_p]
        g = self._geom(21, 151, 1)
        self.min_stride, self.max_stride, self.max_record = g[5], g[6], g[7]

    def _geom(self, k, S, sub):
        out = (C.c_uint32 * 8)()
        self.L.fhcore_seg_geom(k, S, sub, out)
        return list(out)

    def sub_for(self, k, S):
        """lanes per record the dispatcher and launch_k2 go by; 0: the pair takes the tile kernel"""
        return int(self.L.fhcore_seg_sub_for(k, S))

    def launch_ok(self, k, S, sub):
        return bool(self.L.fhcore_seg_launch_ok(k, S, sub))

    def check(self, k, S, sub):
        """(failure code or 0, tile offsets nobody takes) of one tile walked lane by lane, round by round"""
        lost = C.c_uint32(0)
        rc = self.L.fhcore_seg_check(k, S, sub, C.byref(lost))
        return int(rc), int(lost.value)

    def geom(self, k, S, sub):
        """RO, H, LAST, NR of (k, stride, lanes per record)"""
        return tuple(self._geom(k, S, sub)[:4])

    def strides(self, k):
        """every stride the dispatcher can hand a segment kernel at this k"""
        return [S for S in range(self.min_stride, self.max_record + 1) if self.sub_for(k, S)]
