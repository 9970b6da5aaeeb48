"""Host-side mirror of `Superchunk::build` (dcdf/src/superchunk.rs:88-270) over the MI355X library: the caller of the chunk
path.  Tiling, elision and the reference table are control flow; the per-tile (min, max), the fractional bits, every
Chunk::build, the min / max Dacs and the CIDs are computed on the GPU (dcdf_superchunk_build)."""
import ctypes as C

import numpy as np

from . import _lib as L
from .chunk import _ENC, _desc


class SuperchunkBuild:  # MMStruct3Build (mmstruct.rs:24-34) of a Superchunk, plus what resolver.save would have stored
    def __init__(self, objects, root_cid, size, elided, local, external, snapshots, logs):
        self.objects = objects      # {cid bytes: stored object bytes}, sub-objects and the Superchunk node itself
        self.cid = root_cid         # CID of the Superchunk node
        self.data = objects[root_cid]
        self.size, self.elided, self.local, self.external = size, elided, local, external
        self.snapshots, self.logs = snapshots, logs


class Superchunk:
    @staticmethod
    def build(buffer, levels, k=2, fractional_bits=0, round=False):
        """superchunk.rs:88.  `buffer`: ndarray[instants, rows, cols]; `levels`: the k2_levels of the variable."""
        a = np.asarray(buffer)
        return _build(_desc(a, fractional_bits, round), levels, k, L.MEM_HOST)

    @staticmethod
    def build_device(ptr, dtype, strides, shape, levels, k=2, fractional_bits=0, round=False):
        """The same over a view already in HBM: `ptr` = device address of its first element, `dtype` = its numpy type, `strides`
        (instant, row, col) in elements -- zero and negative ones allowed --, `shape` = (instants, rows, cols).  Nothing is
        uploaded or re-densified: the strides reach the kernels as they are, so every element the view can reach must lie inside
        the caller's allocation."""
        d = L.TileDesc()
        d.base = int(ptr)
        d.dtype = _ENC[np.dtype(dtype)]
        d.stride_t, d.stride_r, d.stride_c = [int(s) for s in strides]
        d.instants, d.rows, d.cols = [int(n) for n in shape]
        d.fractional_bits = int(fractional_bits)
        d.round = 1 if round else 0
        return _build(d, levels, k, L.MEM_DEVICE)


def _build(d, levels, k, mem):
    """dcdf_superchunk_build on a tile desc, its result read into a SuperchunkBuild."""
    lv = (C.c_uint32 * max(1, len(levels)))(*[int(x) for x in levels])
    out = C.POINTER(L.SuperchunkBuild)()
    L.check(L.lib().dcdf_superchunk_build(C.byref(d), lv, C.c_size_t(len(levels)), int(k), mem, C.byref(out)), "Superchunk::build")
    owner = _Owner(out)  # frees the C result when the last view of it is gone
    s = out.contents
    objects = {}
    cid = None
    for i in range(s.n_objects):
        o = s.objects[i]
        cid = bytes(o.cid)
        if o.len < _VIEW_FROM:
            objects[cid] = C.string_at(o.bytes, o.len)
        else:
            # the sub-chunk objects are the bulk (hundreds of MB per slice): read-only views of the library's buffers, no copy
            arr = (C.c_uint8 * o.len).from_address(C.addressof(o.bytes.contents))
            arr._owner = owner
            objects[cid] = memoryview(arr).cast("B").toreadonly()
    return SuperchunkBuild(objects, cid, s.size, s.elided, s.local, s.external, s.snapshots, s.logs)


_VIEW_FROM = 1 << 16


class _Owner:
    def __init__(self, out):
        self._out = out

    def __del__(self):
        try:
            L.lib().dcdf_free_superchunk(self._out)
        except Exception:
            pass
