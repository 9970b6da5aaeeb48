"""ctypes binding of libdcdf_k2r.so (the HIP/gfx950 product library).  There is no fallback: if the
library is missing or no GPU is present every operation raises."""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("DCDF_K2R_LIB", os.path.join(_HERE, "libdcdf_k2r.so"))  # override: diagnostic builds

DCDF_I32, DCDF_I64, DCDF_F32, DCDF_F64 = 4, 8, 32, 64
MEM_HOST, MEM_DEVICE = 0, 1


class TileDesc(C.Structure):
    _fields_ = [("base", C.c_void_p), ("dtype", C.c_int32), ("_pad0", C.c_int32), ("stride_t", C.c_int64),
                ("stride_r", C.c_int64), ("stride_c", C.c_int64), ("instants", C.c_uint32), ("rows", C.c_uint32),
                ("cols", C.c_uint32), ("fractional_bits", C.c_uint8), ("round", C.c_uint8), ("_pad1", C.c_uint8 * 2)]


class Encoded(C.Structure):
    _fields_ = [("bytes", C.POINTER(C.c_uint8)), ("len", C.c_size_t), ("snapshots", C.c_uint32), ("logs", C.c_uint32),
                ("status", C.c_int32), ("kernel", C.c_int32), ("minmax", C.POINTER(C.c_int64))]


class StoredObject(C.Structure):
    _fields_ = [("cid", C.c_uint8 * 36), ("bytes", C.POINTER(C.c_uint8)), ("len", C.c_size_t)]


class SuperchunkBuild(C.Structure):
    _fields_ = [("objects", C.POINTER(StoredObject)), ("n_objects", C.c_size_t), ("size", C.c_uint64), ("elided", C.c_uint32),
                ("local", C.c_uint32), ("external", C.c_uint32), ("snapshots", C.c_uint32), ("logs", C.c_uint32)]


class Cube(C.Structure):
    _fields_ = [("start", C.c_uint32), ("end", C.c_uint32), ("top", C.c_uint32), ("bottom", C.c_uint32),
                ("left", C.c_uint32), ("right", C.c_uint32)]


class RasterTile(C.Structure):  # dcdf_raster_tile
    _fields_ = [("chunk", C.c_void_p), ("row0", C.c_uint32), ("col0", C.c_uint32), ("values", C.c_void_p), ("minmax", C.c_void_p),
                ("encoding", C.c_int32), ("fractional_bits", C.c_uint8), ("minmax_exact", C.c_uint8), ("_pad", C.c_uint8 * 2)]


class DcdfError(RuntimeError):
    def __init__(self, code, what=""):
        self.code = code
        msg = what
        try:
            msg = "%s: %s" % (what, lib().dcdf_strerror(code).decode())
        except Exception:
            pass
        super().__init__("dcdf_k2r error %d %s" % (code, msg))


_lib = None

# every symbol include/dcdf_k2r.h declares
SYMBOLS = [
    "dcdf_chunk_build_batch", "dcdf_chunk_build", "dcdf_free_encoded", "dcdf_encoder_create", "dcdf_encoder_tile_kernel", "dcdf_encoder_run",
    "dcdf_encoder_result", "dcdf_encoder_fetch", "dcdf_encoder_gather_size", "dcdf_encoder_gather", "dcdf_encoder_total_bytes", "dcdf_encoder_destroy", "dcdf_superchunk_build", "dcdf_free_superchunk", "dcdf_chunk_open",
    "dcdf_chunk_close", "dcdf_chunk_info", "dcdf_chunk_get", "dcdf_chunk_fill_cell", "dcdf_chunk_fill_window",
    "dcdf_chunk_search", "dcdf_query_fill_window_batch", "dcdf_query_search_batch", "dcdf_query_fill_window_batch_typed", "dcdf_query_search_batch_mem", "dcdf_query_get_batch", "dcdf_query_fill_cell_batch", "dcdf_chunk_open_batch", "dcdf_chunk_instant_layout", "dcdf_raster_create", "dcdf_raster_destroy", "dcdf_raster_fill_window_batch", "dcdf_raster_search_batch", "dcdf_suggest_fraction", "dcdf_encoder_object_sha256",
    "dcdf_synth_fill", "dcdf_calib_read", "dcdf_device_alloc", "dcdf_device_free", "dcdf_device_copy", "dcdf_strerror", "dcdf_device_name", "dcdf_abi_version", "dcdf_last_hip_error", "dcdf_device_pool_trim",
    "dcdf_value_bounds", "dcdf_chunk_search_values", "dcdf_query_search_values_batch", "dcdf_raster_search_values_batch",
    "dcdf_raster_create_tiles", "dcdf_raster_get_batch", "dcdf_raster_fill_cell_batch", "dcdf_raster_decode_batch",
    "dcdf_raster_reduce_time_batch", "dcdf_raster_reduce_space_batch", "dcdf_space_fold_records",
    "dcdf_raster_histogram_batch", "dcdf_histogram_bounds", "dcdf_raster_spells_batch",
    "dcdf_raster_zonal_batch", "dcdf_zonal_fold_limbs", "dcdf_raster_quantile_time_batch", "dcdf_quantile_select_host",
    "dcdf_raster_reduce_time_groups_batch",
    "dcdf_raster_moments_time_batch", "dcdf_raster_moments_time_groups_batch", "dcdf_moments_host",
    "dcdf_regress_host", "dcdf_raster_regress_time_batch", "dcdf_raster_regress_time_groups_batch",
    "dcdf_raster_rolling_time_batch", "dcdf_raster_rolling_time_groups_batch",
]
# dcdf_raster_reduce_time_batch: the statistics, in plane order
REDUCE_OPS = {"min": 1, "max": 2, "sum": 4, "count": 8, "mean": 16}
HIST_MAX_BINS = 256  # DCDF_HIST_MAX_BINS
# dcdf_raster_spells_batch: the statistics, in plane order, and the "no hit" value of longest_start / first / last
SPELL_OPS = {"count": 1, "longest": 2, "longest_start": 4, "first": 8, "last": 16}
SPELL_NONE = 0xffffffff  # DCDF_SPELL_NONE
ZONE_NONE = 0xffff  # DCDF_ZONE_NONE: the label of no zone
GROUP_NONE = 0xffff  # DCDF_GROUP_NONE: the label of an instant of no group (dcdf_raster_reduce_time_groups_batch)
# dcdf_raster_moments_time_batch / dcdf_raster_moments_time_groups_batch: the statistics (DCDF_MOMENT_*), in plane order
MOMENT_OPS = {"count": 1, "mean": 2, "var": 4, "std": 8}
# dcdf_regress_host / dcdf_raster_regress_time_batch / dcdf_raster_regress_time_groups_batch: the statistics (DCDF_REGRESS_*), in
# plane order
REGRESS_OPS = {"count": 1, "slope": 2, "intercept": 4, "corr": 8}
# dcdf_raster_rolling_time_batch / dcdf_raster_rolling_time_groups_batch: the statistics (DCDF_ROLLING_*), in plane order; the
# kinds; the widest window
ROLLING_OPS = {"max": 1, "argmax": 2, "min": 4, "argmin": 8, "count": 16}
ROLLING_SUM, ROLLING_MEAN = 0, 1
ROLLING_MAX_WINDOW = 65535
# dcdf_raster_quantile_time_batch: DCDF_QUANTILE_*, and the most probabilities of one call
QUANTILE_METHODS = {"lower": 0, "higher": 1, "nearest": 2, "linear": 3}
QUANTILE_MAX_PROBS = 16


def lib():
    """Loads the HIP library; raises (loudly) when it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError("libdcdf_k2r.so not built (run __graft_entry__.build() / make -C dcdf_amd/csrc); "
                               "the MI355X path has no CPU fallback")
        L = C.CDLL(LIB_PATH)
        L.dcdf_strerror.restype = C.c_char_p
        L.dcdf_device_name.restype = C.c_char_p
        L.dcdf_encoder_total_bytes.restype = C.c_uint64
        L.dcdf_encoder_total_bytes.argtypes = [C.c_void_p]
        L.dcdf_free_encoded.argtypes = [C.c_void_p, C.c_size_t]
        L.dcdf_free_encoded.restype = None
        L.dcdf_encoder_destroy.argtypes = [C.c_void_p]
        L.dcdf_encoder_destroy.restype = None
        L.dcdf_chunk_close.argtypes = [C.c_void_p]
        L.dcdf_chunk_close.restype = None
        L.dcdf_free_superchunk.argtypes = [C.c_void_p]
        L.dcdf_free_superchunk.restype = None
        # value search: the real-valued bounds are doubles (ctypes would pass a Python float as one only when told)
        L.dcdf_value_bounds.restype = C.c_int
        L.dcdf_value_bounds.argtypes = [C.c_int32, C.c_uint32, C.c_double, C.c_double, C.POINTER(C.c_int64), C.POINTER(C.c_int64),
                                        C.POINTER(C.c_int32)]
        L.dcdf_chunk_search_values.restype = C.c_int
        L.dcdf_chunk_search_values.argtypes = [C.c_void_p, C.POINTER(Cube), C.c_double, C.c_double, C.c_void_p, C.c_size_t,
                                               C.POINTER(C.c_size_t)]
        L.dcdf_raster_reduce_space_batch.restype = C.c_int
        L.dcdf_raster_reduce_space_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint32, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                                     C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_float)]
        L.dcdf_space_fold_records.restype = C.c_int
        L.dcdf_space_fold_records.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_double)]
        L.dcdf_raster_histogram_batch.restype = C.c_int
        L.dcdf_raster_histogram_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_int,
                                                  C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_float)]
        L.dcdf_raster_spells_batch.restype = C.c_int
        L.dcdf_raster_spells_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint32, C.c_void_p, C.c_int,
                                               C.c_void_p, C.c_void_p, C.POINTER(C.c_float)]
        L.dcdf_raster_zonal_batch.restype = C.c_int
        L.dcdf_raster_zonal_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint32, C.c_void_p, C.c_void_p, C.c_int, C.c_uint32,
                                              C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_float)]
        L.dcdf_raster_reduce_time_groups_batch.restype = C.c_int
        L.dcdf_raster_reduce_time_groups_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32,
                                                           C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_float)]
        L.dcdf_raster_moments_time_batch.restype = C.c_int
        L.dcdf_raster_moments_time_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint32, C.c_uint32, C.c_void_p, C.c_int, C.c_void_p,
                                                     C.c_void_p, C.POINTER(C.c_float)]
        L.dcdf_raster_moments_time_groups_batch.restype = C.c_int
        L.dcdf_raster_moments_time_groups_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p,
                                                            C.c_uint32, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_float)]
        L.dcdf_moments_host.restype = C.c_int
        L.dcdf_moments_host.argtypes = [C.c_void_p, C.c_size_t, C.c_uint32, C.c_void_p, C.c_void_p]
        L.dcdf_regress_host.restype = C.c_int
        L.dcdf_regress_host.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
        L.dcdf_raster_regress_time_batch.restype = C.c_int
        L.dcdf_raster_regress_time_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                                     C.c_void_p, C.c_void_p, C.POINTER(C.c_float)]
        L.dcdf_raster_regress_time_groups_batch.restype = C.c_int
        L.dcdf_raster_regress_time_groups_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p,
                                                            C.c_void_p, C.c_uint32, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                                            C.POINTER(C.c_float)]
        L.dcdf_raster_rolling_time_batch.restype = C.c_int
        L.dcdf_raster_rolling_time_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int32, C.c_void_p,
                                                     C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_float)]
        L.dcdf_raster_rolling_time_groups_batch.restype = C.c_int
        L.dcdf_raster_rolling_time_groups_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int32,
                                                            C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                                            C.POINTER(C.c_float)]
        L.dcdf_zonal_fold_limbs.restype = C.c_int
        L.dcdf_zonal_fold_limbs.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
        L.dcdf_raster_quantile_time_batch.restype = C.c_int
        L.dcdf_raster_quantile_time_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_uint32, C.c_int32, C.c_void_p, C.c_int,
                                                      C.c_void_p, C.c_void_p, C.POINTER(C.c_float)]
        L.dcdf_quantile_select_host.restype = C.c_int
        L.dcdf_quantile_select_host.argtypes = [C.c_void_p, C.c_uint32, C.c_uint64, C.c_void_p, C.c_uint32, C.c_int32, C.c_void_p, C.c_void_p]
        L.dcdf_histogram_bounds.restype = C.c_int
        L.dcdf_histogram_bounds.argtypes = [C.c_int32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
        _lib = L
    return _lib


def space_fold_records(records):
    """dcdf_space_fold_records (host only, no GPU): records = [(integer, shift, negative)], integer within 128 signed bits.  Returns
    sum((-1)^negative * integer * 2^shift) / 2^63 as the nearest double, ties to even."""
    import numpy as np
    n = len(records)
    hi = np.array([((int(v) >> 64) & (2 ** 64 - 1)) for v, _, _ in records], dtype=np.uint64)
    lo = np.array([(int(v) & (2 ** 64 - 1)) for v, _, _ in records], dtype=np.uint64)
    sc = np.array([int(s) | (256 if g else 0) for _, s, g in records], dtype=np.uint32)
    out = C.c_double()
    check(lib().dcdf_space_fold_records(hi.ctypes.data if n else None, lo.ctypes.data if n else None, sc.ctypes.data if n else None, n,
                                        C.byref(out)), "space_fold_records")
    return out.value


def quantile_select_host(x, probs, method="linear"):
    """dcdf_quantile_select_host (host only, no GPU): the quantiles `probs` over axis 0 of x [instants, ...] as the device selects
    them.  Returns (float64 [n_probs, ...], uint32 [...] passes over each cell's series after the first)."""
    import numpy as np
    x = np.ascontiguousarray(np.asarray(x, dtype=np.float64))
    p = np.ascontiguousarray(np.asarray(probs, dtype=np.float64).ravel())
    cells = int(np.prod(x.shape[1:], dtype=np.int64))
    out = np.empty((max(p.size, 1),) + x.shape[1:], dtype=np.float64)
    passes = np.zeros(x.shape[1:], dtype=np.uint32)
    check(lib().dcdf_quantile_select_host(x.ctypes.data, x.shape[0], cells, p.ctypes.data, p.size, QUANTILE_METHODS[method], out.ctypes.data,
                                          passes.ctypes.data), "quantile_select_host")
    return out[:p.size], passes


def moments_host(x, ddof=0, state=None, finish=True):
    """dcdf_moments_host (host only, no GPU): continues the state (c, K, s1, s2) of the moments over time -- None: the initial one
    -- over the float64 series x, NaN skipped, with the step the kernels run.  Returns (state float64[4], (count, mean, var, std)
    float64[4] or None without `finish`)."""
    import numpy as np
    x = np.ascontiguousarray(np.asarray(x, dtype=np.float64).ravel())
    st = np.array([0.0, np.nan, 0.0, 0.0]) if state is None else np.array(state, dtype=np.float64)
    if st.shape != (4,):
        raise ValueError("moments_host: the state is (c, K, s1, s2)")
    out = np.empty(4, dtype=np.float64) if finish else None
    check(lib().dcdf_moments_host(x.ctypes.data if x.size else None, x.size, ddof, st.ctypes.data, None if out is None else out.ctypes.data),
          "moments_host")
    return st, out


def regress_host(x, e, state=None, finish=True):
    """dcdf_regress_host (host only, no GPU): continues the state (c, K, sy, syy, se, see, sey) of the regression over time --
    None: the initial one -- over the float64 pairs (x, e), NaN x skipped, with the contract's step (k2r_regress.h).  Returns (state
    float64[7], (count, slope, intercept, corr) float64[4] or None without `finish`)."""
    import numpy as np
    x = np.ascontiguousarray(np.asarray(x, dtype=np.float64).ravel())
    e = np.ascontiguousarray(np.asarray(e, dtype=np.float64).ravel())
    st = np.array([0.0, np.nan, 0.0, 0.0, 0.0, 0.0, 0.0]) if state is None else np.array(state, dtype=np.float64)
    if st.shape != (7,) or e.size != x.size:
        raise ValueError("regress_host: the state is (c, K, sy, syy, se, see, sey), x and e are as long")
    out = np.empty(4, dtype=np.float64) if finish else None
    check(lib().dcdf_regress_host(x.ctypes.data if x.size else None, e.ctypes.data if e.size else None, x.size, st.ctypes.data,
                                  None if out is None else out.ctypes.data), "regress_host")
    return st, out


def zonal_fold_limbs(limbs):
    """dcdf_zonal_fold_limbs (host only, no GPU): six int64 counters, limb i weighing 2^(32 i).  Returns their total / 2^63 as the
    nearest double, ties to even."""
    import numpy as np
    a = np.ascontiguousarray(np.asarray(limbs, dtype=np.int64))
    if a.shape != (6,):
        raise ValueError("zonal_fold_limbs: six limbs")
    out = C.c_double()
    check(lib().dcdf_zonal_fold_limbs(a.ctypes.data, C.byref(out)), "zonal_fold_limbs")
    return out.value


def histogram_bounds(encoding, fractional_bits, edges):
    """dcdf_histogram_bounds (host only, no GPU): (lo, hi) int64[bins] -- the inclusive interval of stored integers of a chunk of
    this encoding and these fractional bits that every bin of `edges` (bins + 1 increasing values) takes; lo[b] > hi[b] when
    bin b takes none.  Stored 0 of a float encoding belongs to no bin."""
    import numpy as np
    e = np.ascontiguousarray(np.asarray(edges, dtype=np.float64).ravel())
    bins = max(int(e.size) - 1, 0)
    lo, hi = np.zeros(max(bins, 1), dtype=np.int64), np.zeros(max(bins, 1), dtype=np.int64)
    check(lib().dcdf_histogram_bounds(int(encoding), int(fractional_bits), e.ctypes.data, bins, lo.ctypes.data, hi.ctypes.data),
          "histogram_bounds")
    return lo[:bins], hi[:bins]


def value_bounds(encoding, fractional_bits, lower, upper):
    """dcdf_value_bounds (host only, no GPU): (lo, hi, skip_zero) -- the stored integers of a chunk of this encoding and these
    fractional bits whose typed value lies in [lower, upper], less 0 when skip_zero; lo > hi when none does."""
    lo, hi, sz = C.c_int64(), C.c_int64(), C.c_int32()
    check(lib().dcdf_value_bounds(int(encoding), int(fractional_bits), float(lower), float(upper), C.byref(lo), C.byref(hi), C.byref(sz)),
          "value_bounds")
    return lo.value, hi.value, bool(sz.value)


def unpack_kernel(word):
    """dcdf_encoded.kernel as Encoder.tile_kernel returns it: (log2_sidelen, padded, loader, generic_key); None for a
    rejected tile."""
    if word == 0:
        return None
    if word < (1 << 24):
        return (-1, -1, -1, word)
    return (word & 0xff, (word >> 8) & 0xff, (word >> 16) & 0xff, 0)


def check(rc, what=""):
    if rc != 0:
        raise DcdfError(rc, what)
