"""ctypes binding of the C ABI in include/bwtm.h (the same stub a maintainer of another host
language would write).  There is no CPU fallback: if libbwtm.so is
missing or no GPU is usable, calls raise."""
import ctypes as C
import os
from functools import partial

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
# BWTM_LIB selects another build of the same library (A/B measurements of kernel variants on one GPU box)
LIB_PATH = os.environ.get("BWTM_LIB") or os.path.join(HERE, "libbwtm.so")
SIGMA = 6

u64 = C.c_uint64
p_u8 = C.POINTER(C.c_uint8)
p_u32 = C.POINTER(C.c_uint32)
p_u64 = C.POINTER(C.c_uint64)
vp = C.c_void_p


class _ArrayArg:
    """Argument type of a `T*` parameter that takes the numpy array itself, so that the owner and the pointer are one object: None, a
    C-contiguous array of exactly `dtype`, or whatever the plain pointer type takes (a pointer, a ctypes array, a byref).  Anything else is a
    TypeError, which ctypes raises as ArgumentError before the library is entered."""

    @classmethod
    def from_param(cls, x):
        if not isinstance(x, np.ndarray):
            return cls.pointer.from_param(x)
        if x.dtype != cls.dtype or not x.flags["C_CONTIGUOUS"]:
            raise TypeError("a C-contiguous %s array is wanted, not %s%s" % (cls.dtype, x.dtype, "" if x.flags["C_CONTIGUOUS"] else " (not contiguous)"))
        return x.ctypes.data_as(cls.pointer)


class a_u8(_ArrayArg):
    dtype, pointer = np.dtype(np.uint8), p_u8


class a_u32(_ArrayArg):
    dtype, pointer = np.dtype(np.uint32), p_u32


class a_u64(_ArrayArg):
    dtype, pointer = np.dtype(np.uint64), p_u64


class HostInput(C.Structure):
    """bwtm_host_input"""
    _fields_ = [("data", C.c_void_p), ("nbytes", u64), ("sequences", u64), ("bases", u64), ("C", p_u64)]


class HostOutput(C.Structure):
    """bwtm_host_output"""
    _fields_ = [("data", C.c_void_p), ("nbytes", u64), ("blocks", u64), ("sequences", u64), ("bases", u64),
                ("C", u64 * (SIGMA + 1)), ("block_end", C.c_void_p), ("cum", C.c_void_p),
                ("sample_width", C.c_int), ("fields", C.c_void_p), ("anchors", C.c_void_p),
                ("ms_upload", C.c_double), ("ms_search", C.c_double), ("ms_interleave", C.c_double),
                ("ms_encode_download", C.c_double), ("ms_samples", C.c_double), ("ms_total", C.c_double)]


ALLOC_FN = C.CFUNCTYPE(C.c_void_p, C.c_void_p, C.c_int, u64)


class Piece(C.Structure):
    """bwtm_piece"""
    _fields_ = [("byte_first", u64), ("nbytes", u64), ("data", C.c_void_p), ("sample_block_first", u64), ("sample_blocks", u64),
                ("sample_width", C.c_int), ("fields", C.c_void_p), ("anchors", C.c_void_p), ("anchor_first", u64), ("nanchors", u64),
                ("block_end", C.c_void_p), ("cum", C.c_void_p), ("last", C.c_int)]


class StreamStats(C.Structure):
    """bwtm_stream_stats"""
    _fields_ = [("pieces", u64), ("slice_records", u64), ("slice_bytes_peak", u64),
                ("ms_upload", C.c_double), ("ms_search", C.c_double), ("ms_second_half", C.c_double), ("ms_total", C.c_double)]


class UploadStats(C.Structure):
    """bwtm_upload_stats"""
    _fields_ = [("chunks", u64), ("chunk_bytes", u64), ("staging_bytes_peak", u64), ("ms_total", C.c_double)]


PIECE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(Piece))


class HostIndex(C.Structure):
    """bwtm_host_index"""
    _fields_ = [("data", C.c_void_p), ("nbytes", u64), ("blocks", u64), ("sequences", u64), ("bases", u64), ("C", u64 * (SIGMA + 1)), ("cum", C.c_void_p)]


class IndexHeader(C.Structure):
    """bwtm_index_header"""
    _fields_ = [("bases", u64), ("sequences", u64), ("C", u64 * (SIGMA + 1))]


class PartInfo(C.Structure):
    """bwtm_part_info"""
    _fields_ = [("steps", u64), ("node_levels", u64), ("elements", u64), ("largest", u64), ("pulled_bytes", u64), ("boundary_bytes", u64),
                ("record_bytes", u64), ("bitvector_bytes", u64), ("ms_search", C.c_double), ("ms_search_wait", C.c_double), ("ms_finish", C.c_double)]

# Every symbol include/bwtm.h declares: (name, restype, argtypes)
SYMBOLS = [
    ("bwtm_init", C.c_int, [C.c_int]),
    ("bwtm_context_create", C.c_int, [C.c_int, C.POINTER(vp)]),
    ("bwtm_context_make_current", C.c_int, [vp]),
    ("bwtm_context_destroy", None, [vp]),
    ("bwtm_device_bytes_peak", u64, [C.c_int]),
    ("bwtm_host_alloc", C.c_int, [u64, C.POINTER(vp)]),
    ("bwtm_host_free", None, [vp]),
    ("bwtm_ra_download_runs", C.c_int, [vp, a_u64, a_u64, u64, a_u64]),
    ("bwtm_ra_or_from", C.c_int, [vp, vp, u64]),
    ("bwtm_merge_consume", C.c_int, [vp, vp, C.POINTER(vp)]),
    ("bwtm_merged_records", u64, [vp, vp]),
    ("bwtm_slice_bounds", C.c_int, [u64, C.c_int, C.c_int, a_u64, a_u64]),
    ("bwtm_slice_bounds_equal", C.c_int, [u64, C.c_int, C.c_int, a_u64, a_u64, a_u64]),
    ("bwtm_ra_range_counts", C.c_int, [vp, u64, u64, a_u64, a_u64, a_u64]),
    ("bwtm_ra_finalize_range", C.c_int, [vp, u64, u64, u64, u64, a_u64, a_u64]),
    ("bwtm_interleave_range", C.c_int, [vp, vp, vp, u64, u64, C.POINTER(vp)]),
    ("bwtm_slice_free", None, [vp]),
    ("bwtm_slice_lasthead", C.c_int, [vp, a_u64]),
    ("bwtm_slice_size_table", C.c_int, [vp, u64, a_u64]),
    ("bwtm_fold_offsets", C.c_int, [a_u64, C.c_int, a_u64]),
    ("bwtm_slice_encode", C.c_int, [vp, u64]),
    ("bwtm_slice_byte_first", u64, [vp]),
    ("bwtm_slice_bytes", u64, [vp]),
    ("bwtm_slice_block_first", u64, [vp]),
    ("bwtm_slice_blocks", u64, [vp]),
    ("bwtm_slice_first_block_start", C.c_int, [vp, a_u64]),
    ("bwtm_slice_download_data", C.c_int, [vp, a_u8, u64]),
    ("bwtm_slice_download_samples", C.c_int, [vp, u64, a_u64, a_u64]),
    ("bwtm_slice_extract", C.c_int, [vp, u64, u64, a_u8]),
    ("bwtm_merge_host", C.c_int, [C.POINTER(HostInput), C.POINTER(HostInput), ALLOC_FN, vp, C.c_int, C.POINTER(HostOutput), C.POINTER(vp)]),
    ("bwtm_merge_host_chained", C.c_int, [vp, C.POINTER(HostInput), ALLOC_FN, vp, C.c_int, C.POINTER(HostOutput), C.POINTER(vp)]),
    ("bwtm_merge_host_pipelined", C.c_int, [vp, C.POINTER(HostInput), C.POINTER(HostInput), vp, C.POINTER(HostInput), C.POINTER(vp), ALLOC_FN, vp, C.c_int,
                                            C.POINTER(HostOutput), C.POINTER(vp)]),
    ("bwtm_merge_host_streamed", C.c_int, [vp, C.POINTER(HostInput), C.POINTER(HostInput), u64, C.c_int, PIECE_FN, vp, C.POINTER(HostOutput),
                                           C.POINTER(StreamStats)]),
    ("bwtm_upload_begin", C.c_int, [C.POINTER(HostInput), C.POINTER(vp)]),
    ("bwtm_upload_finish", C.c_int, [vp, C.POINTER(vp)]),
    ("bwtm_upload_free", None, [vp]),
    ("bwtm_last_error", C.c_char_p, []),
    ("bwtm_synchronize", C.c_int, []),
    ("bwtm_trim", C.c_int, []),
    ("bwtm_tune", C.c_int, [C.c_char_p, C.c_longlong]),
    ("bwtm_index_upload", C.c_int, [a_u8, u64, u64, u64, a_u64, C.POINTER(vp)]),
    ("bwtm_index_upload_streamed", C.c_int, [a_u8, u64, u64, u64, a_u64, C.POINTER(vp), C.POINTER(UploadStats)]),
    ("bwtm_index_from_device", C.c_int, [vp, u64, u64, u64, a_u64, C.POINTER(vp)]),
    ("bwtm_index_from_device_borrowed", C.c_int, [vp, u64, u64, u64, a_u64, C.POINTER(vp)]),
    ("bwtm_index_from_symbols_device", C.c_int, [vp, u64, C.POINTER(vp)]),
    ("bwtm_index_free", None, [vp]),
    ("bwtm_index_bases", u64, [vp]),
    ("bwtm_index_sequences", u64, [vp]),
    ("bwtm_index_bytes", u64, [vp]),
    ("bwtm_index_blocks", u64, [vp]),
    ("bwtm_index_C", None, [vp, a_u64]),
    ("bwtm_index_encode", C.c_int, [vp]),
    ("bwtm_index_drop_native", C.c_int, [vp]),
    ("bwtm_index_device_data", C.c_int, [vp, C.POINTER(vp), a_u64]),
    ("bwtm_index_download_data", C.c_int, [vp, a_u8, u64]),
    ("bwtm_index_download_samples", C.c_int, [vp, a_u64, a_u64]),
    ("bwtm_index_samples_width", C.c_int, [vp, C.POINTER(C.c_int)]),
    ("bwtm_index_download_samples_compact", C.c_int, [vp, C.c_int, vp, a_u64]),
    ("bwtm_rank_batch", C.c_int, [vp, a_u64, a_u8, u64, a_u64]),
    ("bwtm_inverse_select_batch", C.c_int, [vp, a_u64, u64, a_u64, a_u8]),
    ("bwtm_find_batch", C.c_int, [vp, a_u8, a_u64, u64, a_u64, a_u64]),
    ("bwtm_find_approx_batch", C.c_int, [vp, a_u8, a_u64, u64, C.c_uint32, u64, a_u64, a_u64, a_u64, a_u8, u64]),
    ("bwtm_find_approx_stats", C.c_int, [a_u64]),
    ("bwtm_find_edit_batch", C.c_int, [vp, a_u8, a_u64, u64, C.c_uint32, u64, a_u64, a_u64, a_u64, a_u8, a_u32, u64]),
    ("bwtm_find_edit_stats", C.c_int, [a_u64]),
    ("bwtm_matching_stats_batch", C.c_int, [vp, a_u8, a_u64, u64, a_u32, a_u64, a_u64]),
    ("bwtm_mem_batch", C.c_int, [vp, a_u8, a_u64, u64, C.c_uint32, a_u64, a_u32, a_u32, a_u64, a_u64, u64]),
    ("bwtm_mem_stats", C.c_int, [a_u64]),
    ("bwtm_extract", C.c_int, [vp, u64, u64, a_u8]),
    ("bwtm_sequences_extract", C.c_int, [vp, a_u64, u64, u64, u64, a_u64, a_u8, u64]),
    ("bwtm_locator_create", C.c_int, [vp, u64, C.POINTER(vp)]),
    ("bwtm_locator_free", None, [vp]),
    ("bwtm_locator_bytes", u64, [vp]),
    ("bwtm_locate_batch", C.c_int, [vp, a_u64, u64, a_u64, a_u64]),
    ("bwtm_locate_ranges", C.c_int, [vp, a_u64, a_u64, u64, u64, a_u64, a_u64, a_u64, u64]),
    ("bwtm_overlap_batch", C.c_int, [vp, a_u8, a_u64, u64, u64, u64, a_u64, a_u64, a_u64, u64]),
    ("bwtm_overlap_sequences", C.c_int, [vp, a_u64, u64, u64, u64, u64, a_u64, a_u64, a_u64, u64]),
    ("bwtm_kmers_create", C.c_int, [vp, C.c_uint32, C.c_uint32, u64, C.POINTER(vp)]),
    ("bwtm_kmers_free", None, [vp]),
    ("bwtm_kmers_distinct", u64, [vp]),
    ("bwtm_kmers_total", u64, [vp]),
    ("bwtm_kmers_bytes", u64, [vp]),
    ("bwtm_kmers_levels", C.c_int, [vp, a_u64]),
    ("bwtm_kmers_download", C.c_int, [vp, u64, u64, a_u64, a_u64, a_u64]),
    ("bwtm_kmers_histogram", C.c_int, [vp, u64, a_u64]),
    ("bwtm_kmer_join_create", C.c_int, [vp, vp, C.c_uint32, C.c_uint32, u64, u64, u64, u64, u64, C.POINTER(vp)]),
    ("bwtm_kmer_join_free", None, [vp]),
    ("bwtm_kmer_join_distinct", u64, [vp]),
    ("bwtm_kmer_join_bytes", u64, [vp]),
    ("bwtm_kmer_join_levels", C.c_int, [vp, a_u64]),
    ("bwtm_kmer_join_download", C.c_int, [vp, u64, u64, a_u64, a_u64, a_u64, a_u64, a_u64]),
    ("bwtm_kmer_join_summary", C.c_int, [vp, a_u64]),
    ("bwtm_corrector_create", C.c_int, [vp, C.c_uint32, u64, C.POINTER(vp)]),
    ("bwtm_corrector_free", None, [vp]),
    ("bwtm_corrector_solid", u64, [vp]),
    ("bwtm_corrector_bytes", u64, [vp]),
    ("bwtm_corrector_k", C.c_uint32, [vp]),
    ("bwtm_correct_batch", C.c_int, [vp, a_u8, a_u64, u64, C.c_uint32, a_u8, a_u8, a_u32]),
    ("bwtm_correct_sequences", C.c_int, [vp, vp, a_u64, u64, u64, u64, C.c_uint32, a_u64, a_u8, u64, a_u8, a_u32]),
    ("bwtm_correct_stats", C.c_int, [a_u64]),
    ("bwtm_unitigs_create", C.c_int, [vp, C.c_uint32, u64, C.POINTER(vp)]),
    ("bwtm_unitigs_free", None, [vp]),
    ("bwtm_unitigs_count", u64, [vp]),
    ("bwtm_unitigs_nodes", u64, [vp]),
    ("bwtm_unitigs_symbols", u64, [vp]),
    ("bwtm_unitigs_bytes", u64, [vp]),
    ("bwtm_unitigs_k", C.c_uint32, [vp]),
    ("bwtm_unitigs_download", C.c_int, [vp, u64, u64, a_u64, a_u8, u64, a_u64, a_u64, a_u8, a_u64]),
    ("bwtm_unitigs_place", C.c_int, [vp, a_u64, u64, a_u64, a_u64]),
    ("bwtm_unitigs_stats", C.c_int, [a_u64]),
    ("bwtm_ra_create", C.c_int, [vp, vp, C.POINTER(vp)]),
    ("bwtm_ra_buffer_bytes", u64, [vp, vp]),
    ("bwtm_ra_create_on", C.c_int, [vp, vp, vp, u64, C.POINTER(vp)]),
    ("bwtm_ra_free", None, [vp]),
    ("bwtm_search", C.c_int, [vp, vp, u64, u64, vp]),
    ("bwtm_ra_device_buffer", C.c_int, [vp, C.POINTER(vp), a_u64]),
    ("bwtm_ra_finalize", C.c_int, [vp]),
    ("bwtm_ra_subset_check", C.c_int, [vp, vp, a_u64, a_u64]),
    ("bwtm_ra_values", u64, [vp]),
    ("bwtm_ra_download", C.c_int, [vp, a_u64, u64]),
    ("bwtm_ra_download_bits", C.c_int, [vp, a_u64, u64]),
    ("bwtm_interleave", C.c_int, [vp, vp, vp, C.POINTER(vp)]),
    ("bwtm_merge", C.c_int, [vp, vp, C.POINTER(vp)]),
    ("bwtm_builder_create", C.c_int, [u64, C.POINTER(vp)]),
    ("bwtm_builder_add", C.c_int, [vp, vp, u64, C.c_uint32, u64, vp, C.c_int]),
    ("bwtm_builder_reads", u64, [vp]),
    ("bwtm_builder_finish", C.c_int, [vp, C.POINTER(vp)]),
    ("bwtm_builder_free", None, [vp]),
    ("bwtm_pool_stats", C.c_int, [vp]),
    ("bwtm_pool_poison_stats", C.c_int, [a_u64, a_u64]),
    ("bwtm_group_create", C.c_int, [C.c_char_p, C.c_int, C.c_int, C.POINTER(vp)]),
    ("bwtm_group_free", None, [vp]),
    ("bwtm_group_part", C.c_int, [vp]),
    ("bwtm_group_parts", C.c_int, [vp]),
    ("bwtm_group_barrier", C.c_int, [vp]),
    ("bwtm_group_allgather", C.c_int, [vp, vp, u64, vp]),
    ("bwtm_group_abort", None, [vp]),
    ("bwtm_partition_cuts_host", C.c_int, [C.POINTER(HostIndex), C.POINTER(HostIndex), C.c_int, C.c_int, a_u64, a_u64]),
    ("bwtm_window_blocks", C.c_int, [C.POINTER(HostIndex), u64, u64, a_u64, a_u64, a_u64, a_u64]),
    ("bwtm_index_upload_window", C.c_int, [vp, u64, u64, a_u64, u64, u64, a_u64, C.c_int, C.POINTER(vp)]),
    ("bwtm_index_record_bytes", u64, [vp]),
    ("bwtm_ra_create_range", C.c_int, [vp, vp, u64, u64, C.POINTER(vp)]),
    ("bwtm_ra_bytes", u64, [vp]),
    ("bwtm_part_create", C.c_int, [vp, C.POINTER(IndexHeader), C.POINTER(IndexHeader), a_u64, a_u64, C.POINTER(vp)]),
    ("bwtm_part_free", None, [vp]),
    ("bwtm_part_window", C.c_int, [vp, C.c_int, a_u64, a_u64]),
    ("bwtm_part_upload", C.c_int, [vp, C.c_int, vp, u64, u64, a_u64, C.c_int]),
    ("bwtm_part_search", C.c_int, [vp]),
    ("bwtm_part_finish", C.c_int, [vp, C.POINTER(vp), a_u64, a_u64, a_u64]),
    ("bwtm_part_stats", C.c_int, [vp, C.POINTER(PartInfo)]),
    ("bwtm_profile_enable", C.c_int, [C.c_int]),
    ("bwtm_profile_only", C.c_int, [C.c_char_p]),
    ("bwtm_profile_reset", C.c_int, []),
    ("bwtm_profile_read", C.c_int, [C.POINTER(C.c_char_p), C.POINTER(C.c_double), a_u64, C.c_int]),
]


class BwtmError(RuntimeError):
    pass


_lib = None


def lib():
    """Loads libbwtm.so; raises (loudly) when the HIP extension has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise BwtmError("HIP extension %s is missing: run `python __graft_entry__.py build` "
                            "(there is no CPU fallback)" % LIB_PATH)
        # PyTorch bundles its own libamdhip64 (SONAME libamdhip64.so.7).  Processes that use both
        # (bench.py, torch.distributed) must share ONE HIP runtime, so torch is loaded first and
        # libbwtm.so's NEEDED libamdhip64.so.7 then resolves to the already loaded copy.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        L = C.CDLL(LIB_PATH)
        for name, res, args in SYMBOLS:
            f = getattr(L, name)       # AttributeError if the library does not export it
            f.restype = res
            f.argtypes = args
        _lib = L
    return _lib


def check(rc):
    if rc != 0:
        raise BwtmError("bwtm error %d: %s" % (rc, lib().bwtm_last_error().decode()))


def _new(create, *args):
    """The handle a create call makes: create(*args, &out), checked."""
    out = vp()
    check(create(*args, C.byref(out)))
    return out


class Handle:
    """Base of the handle classes: h, released once through the C function the class names in _free.  _freed is the message of _live(),
    for the classes whose methods check before they call.  A create call fills h in one line: self.h = _new(lib().bwtm_x_create, ...)."""
    _free = _freed = h = None              # h = None: __del__ of an object made by __new__ finds nothing to free

    def free(self):
        if self.h:
            getattr(lib(), self._free)(self.h)
            self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass

    def _live(self):
        if not self.h:
            raise BwtmError(self._freed)


def _scalar(getter):
    """A property that reads one number of a handle through the C function `getter`."""
    return property(lambda s: int(getattr(lib(), getter)(s.h)))


def _stats(call, names, *handle):
    """The len(names) uint64 that call(*handle, stats) fills, by name."""
    stats = np.zeros(len(names), dtype=np.uint64)
    check(call(*handle, stats))
    return dict(zip(names, (int(v) for v in stats)))


def _u8(a):
    return np.ascontiguousarray(a, dtype=np.uint8)


def _u64(a):
    return np.ascontiguousarray(a, dtype=np.uint64)


def pack_texts(patterns):
    """A list of patterns (sequences of comp values) as the batch calls take them: (text uint8, offsets uint64 [len(patterns) + 1]);
    pattern k is text[offsets[k]: offsets[k + 1]]."""
    lens = np.array([len(p) for p in patterns], dtype=np.uint64)
    offsets = np.zeros(len(patterns) + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum(lens)
    text = np.concatenate([np.asarray(p, dtype=np.uint8) for p in patterns] + [np.zeros(0, dtype=np.uint8)])
    return _u8(text), offsets


def _size_then_fill(call, count, *dtypes):
    """The sizing call, then the filling one: call(hit_offsets, *outputs, capacity) is a C call with its queries bound.  First with every
    output None and capacity 0, which fills hit_offsets [count + 1]; then, only if there are hits, with arrays of exactly hit_offsets[-1]
    entries of `dtypes`.  Returns (hit_offsets, *outputs)."""
    hit_offsets = np.zeros(int(count) + 1, dtype=np.uint64)
    check(call(hit_offsets, *[None] * len(dtypes), 0))
    total = int(hit_offsets[-1])
    outputs = [np.zeros(total, dtype=d) for d in dtypes]
    if total > 0:
        check(call(hit_offsets, *outputs, total))
    return (hit_offsets, *outputs)


def _ids_or_range(index, ids, first, count):
    """(ids array or None, first, count) of a call whose queries are `ids` (any order, repeats allowed), or the sequences first .. first +
    count - 1 of `index` (count=None: up to the last one)."""
    if ids is not None:
        ids = _u64(ids)
        return ids, int(first), ids.size
    if count is None:
        count = max(index.sequences - int(first), 0)
    return None, int(first), int(count)


def init(device=0):
    check(lib().bwtm_init(device))


def synchronize():
    check(lib().bwtm_synchronize())


def tune(key, value):
    check(lib().bwtm_tune(key.encode(), int(value)))


def trim():
    check(lib().bwtm_trim())


def device_bytes_peak(reset=False):
    """Peak bytes of device memory the library's context has held since the last reset."""
    return int(lib().bwtm_device_bytes_peak(1 if reset else 0))


class Context:
    """An additional library context (device + streams + memory pool); make_current() binds the calling thread."""

    def __init__(self, device=0):
        self.h = _new(lib().bwtm_context_create, device)

    def make_current(self):
        check(lib().bwtm_context_make_current(self.h))

    def destroy(self):
        if self.h:
            lib().bwtm_context_destroy(self.h)
            self.h = None


def make_default_current():
    check(lib().bwtm_context_make_current(None))


class HostBuffer:
    """Page-locked host memory (bwtm_host_alloc) viewed as a numpy array."""

    def __init__(self, nbytes, dtype=np.uint8, ptr=None):
        self.nbytes = int(nbytes)
        if ptr is None:
            ptr = _new(lib().bwtm_host_alloc, self.nbytes).value
        self.ptr = ptr
        raw = (C.c_uint8 * max(self.nbytes, 1)).from_address(self.ptr)
        self.array = np.frombuffer(raw, dtype=np.uint8)[: self.nbytes].view(dtype)

    def free(self):
        if self.ptr:
            self.array = None
            lib().bwtm_host_free(vp(self.ptr))
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class HostMerge:
    """Result of merge_host: page-locked data / block_end / cum arrays + the phase times of the call."""

    def __init__(self):
        self.buffers = {}
        self.out = HostOutput()
        self.keep = None

    def free(self):
        for b in self.buffers.values():
            b.free()
        self.buffers = {}
        if self.keep is not None:
            self.keep.free()
            self.keep = None

    def expanded_samples(self):
        """(block_end, cum) whatever form the call returned."""
        if self.out.sample_width == 8:
            return self.block_end, self.cum
        return expand_samples(self.out.sample_width, self.fields, self.anchors, self.out.blocks, self.out.bases)

    fields = property(lambda s: s.buffers[3].array[: SIGMA * s.out.blocks * s.out.sample_width].view(FIELD_DTYPES[s.out.sample_width]).reshape(SIGMA, s.out.blocks))
    anchors = property(lambda s: s.buffers[4].array.view(np.uint64)[: SIGMA * ((s.out.blocks + 63) // 64)].reshape(SIGMA, (s.out.blocks + 63) // 64))
    data = property(lambda s: s.buffers[0].array[: s.out.nbytes])
    block_end = property(lambda s: s.buffers[1].array.view(np.uint64)[: s.out.blocks])
    cum = property(lambda s: s.buffers[2].array.view(np.uint64)[: SIGMA * (s.out.blocks + 1)].reshape(SIGMA, s.out.blocks + 1))
    C = property(lambda s: np.array(list(s.out.C), dtype=np.uint64))
    times = property(lambda s: {k: getattr(s.out, k) for k in ("ms_upload", "ms_search", "ms_interleave", "ms_encode_download", "ms_samples", "ms_total")})


FIELD_DTYPES = {1: np.uint8, 2: np.uint16, 4: np.uint32}


def expand_samples(width, fields, anchors, blocks, bases):
    """Compact samples -> (block_end[blocks], cum[6][blocks + 1]) as bwtm_index_download_samples returns them."""
    f = fields.astype(np.uint64)
    k = np.arange(blocks, dtype=np.int64)
    group = k // 64
    excl = np.cumsum(f, axis=1) - f                                  # exclusive prefix over all blocks ...
    first = excl[:, (group * 64)]                                    # ... minus the prefix at the block's anchor
    at = anchors[:, group] + (excl - first)                          # row 0: block starts; rows 1..5: counts before the block
    starts = at[0]
    block_end = np.concatenate([starts[1:], np.array([bases], dtype=np.uint64)]) - np.uint64(1) if blocks > 0 else np.zeros(0, dtype=np.uint64)
    cum = np.zeros((SIGMA, blocks + 1), dtype=np.uint64)
    if blocks > 0:
        cum[1:, :blocks] = at[1:]
        cum[1:, blocks] = at[1:, -1] + f[1:, -1]
        cum[0, :blocks] = starts - at[1:].sum(axis=0)
        cum[0, blocks] = np.uint64(bases) - cum[1:, blocks].sum()
    return block_end, cum


def _host_input(data, sequences, bases):
    """data: numpy uint8 array (ideally the .array of a HostBuffer)."""
    assert data.dtype == np.uint8 and data.flags["C_CONTIGUOUS"]
    return HostInput(data.ctypes.data, data.size, sequences, bases, None)


def merge_host(a, b, samples=True, keep=False, chained=None, buffers=None):
    """FMI::FMI(a, b) from host-resident inputs to a host-resident result (bwtm_merge_host).
    a, b: (data uint8 array, sequences, bases); chained: a device Index (consumed) instead of a.
    samples: False / 0 = none, True / 1 = block_end + cum, 2 = the compact form (fields + anchors).
    buffers: a dict that keeps the page-locked output buffers between calls (they are reused when large enough)."""
    res = HostMerge()
    if buffers is not None:
        res.buffers = buffers

    def alloc(user, what, nbytes):
        buf = res.buffers.get(what)
        if buf is None or buf.nbytes < nbytes:
            if buf is not None:
                buf.free()
            buf = HostBuffer(nbytes)
            res.buffers[what] = buf
        return buf.ptr

    cb = ALLOC_FN(alloc)
    hb = _host_input(*b)
    kp = vp()
    if chained is not None:
        h, chained.h = chained.h, None                     # consumed by the call
        rc = lib().bwtm_merge_host_chained(h, C.byref(hb), cb, None, int(samples), C.byref(res.out), C.byref(kp) if keep else None)
    else:
        ha = _host_input(*a)
        rc = lib().bwtm_merge_host(C.byref(ha), C.byref(hb), cb, None, int(samples), C.byref(res.out), C.byref(kp) if keep else None)
    if rc != 0:
        if buffers is None:
            res.free()
        check(rc)
    if keep:
        res.keep = Index(kp)
    return res


RESULT_ON_DEVICE = -1


def _copy_from(ptr, count, dtype):
    """A numpy copy of `count` items at a C address (the library's staging is only valid until the sink returns)."""
    if not ptr or count == 0:
        return np.zeros(0, dtype=dtype)
    nbytes = count * np.dtype(dtype).itemsize
    return np.frombuffer((C.c_uint8 * nbytes).from_address(ptr), dtype=dtype).copy()


class PieceCopy:
    """The contents of one bwtm_piece, copied out of the library's staging."""

    def __init__(self, piece):
        self.byte_first, self.nbytes = int(piece.byte_first), int(piece.nbytes)
        self.sample_block_first, self.sample_blocks = int(piece.sample_block_first), int(piece.sample_blocks)
        self.sample_width, self.last = int(piece.sample_width), bool(piece.last)
        self.anchor_first, self.nanchors = int(piece.anchor_first), int(piece.nanchors)
        ns = self.sample_blocks
        self.data = _copy_from(piece.data, self.nbytes, np.uint8)
        self.fields = self.anchors = self.block_end = self.cum = None
        if ns > 0 and self.sample_width in FIELD_DTYPES:
            self.fields = _copy_from(piece.fields, SIGMA * ns, FIELD_DTYPES[self.sample_width]).reshape(SIGMA, ns)
            self.anchors = _copy_from(piece.anchors, SIGMA * self.nanchors, np.uint64).reshape(SIGMA, self.nanchors)
        elif ns > 0 and self.sample_width == 8:
            self.block_end = _copy_from(piece.block_end, ns, np.uint64)
            self.cum = _copy_from(piece.cum, SIGMA * ns, np.uint64).reshape(SIGMA, ns)


def assemble_pieces(pieces, C_array):
    """The pieces of a streamed merge laid end to end: (data, width, fields, anchors) with the fields widened to the largest width of any
    piece -- what bwtm_index_download_samples_compact gives for the whole result --, or (data, 8, block_end, cum[6][blocks + 1]) as
    bwtm_index_download_samples gives them (the column behind the last block comes from C), or (data, 0, None, None) without samples.
    A pure function of the pieces (objects with PieceCopy's attributes); raises BwtmError when they do not fit together."""
    if not pieces or [bool(p.last) for p in pieces].count(True) != 1 or not pieces[-1].last:
        raise BwtmError("streamed merge: exactly the final piece must be marked last")
    at_byte = at_block = 0
    for p in pieces:
        if p.byte_first != at_byte or (p.sample_blocks > 0 and p.sample_block_first != at_block):
            raise BwtmError("streamed merge: piece at byte %d / block %d, expected %d / %d" % (p.byte_first, p.sample_block_first, at_byte, at_block))
        at_byte += p.nbytes
        at_block += p.sample_blocks
    data = np.concatenate([p.data for p in pieces]) if pieces else np.zeros(0, dtype=np.uint8)
    sampled = [p for p in pieces if p.sample_blocks > 0]
    width = max([p.sample_width for p in pieces])
    if width == 0:
        return data, 0, None, None
    blocks = at_block
    if width != 8:
        dtype = FIELD_DTYPES[width]
        fields = np.concatenate([p.fields.astype(dtype) for p in sampled], axis=1) if sampled else np.zeros((SIGMA, 0), dtype=dtype)
        at_anchor = 0
        for p in sampled:
            if p.nanchors != (p.sample_block_first + p.sample_blocks + 63) // 64 - (p.sample_block_first + 63) // 64 or (p.nanchors > 0 and p.anchor_first != at_anchor):
                raise BwtmError("streamed merge: a piece's anchors do not continue those of the pieces before it")
            at_anchor += p.nanchors
        anchors = np.concatenate([p.anchors for p in sampled], axis=1) if sampled else np.zeros((SIGMA, 0), dtype=np.uint64)
        return data, width, fields, anchors
    # the full arrays; compact pieces among them (a compact-mode merge in which one piece held a block of 2^32 - 1 positions or more) are
    # expanded from the back: the position and counts behind the last block are C's, and a piece ends where the next one starts
    C_array = np.asarray(C_array, dtype=np.uint64)
    totals = C_array[1: SIGMA + 1] - C_array[:SIGMA]
    end = np.concatenate([C_array[SIGMA: SIGMA + 1], totals[1:]])   # start position and counts of 1..5 behind the piece
    block_end, cum = [], []
    for p in reversed(sampled):
        if p.sample_width == 8:
            block_end.append(p.block_end); cum.append(p.cum)
            end = np.concatenate([p.cum[:, :1].sum(axis=0, dtype=np.uint64), p.cum[1:, 0]])
            continue
        f = p.fields.astype(np.uint64)
        start = end - f.sum(axis=1, dtype=np.uint64)
        at = start[:, None] + (np.cumsum(f, axis=1, dtype=np.uint64) - f)
        block_end.append(at[0] + f[0] - np.uint64(1))
        full = at.copy(); full[0] = at[0] - at[1:].sum(axis=0, dtype=np.uint64)
        cum.append(full)
        end = start
    block_end.reverse(); cum.reverse()
    return (data, 8, np.concatenate(block_end) if block_end else np.zeros(0, dtype=np.uint64),
            np.concatenate(cum + [totals.reshape(SIGMA, 1)], axis=1))


SAMPLES_NONE, SAMPLES_FULL, SAMPLES_COMPACT = 0, 1, 2


def merge_host_streamed(a, b, slice_records=0, samples=SAMPLES_COMPACT, chained=None, sink=None):
    """bwtm_merge_host_streamed: the merged BWT leaves the device slice by slice (slice_records records each, 0 = the library chooses).
    a, b: (data uint8 array, sequences, bases); chained: a device Index (consumed) instead of a.
    sink(PieceCopy) -> falsy to go on, truthy to stop (the call then raises BwtmError); given a sink, the call returns (out, stats).
    Without one the pieces are collected and the call returns (data, width, fields, anchors, out, stats) -- or (data, 8, block_end,
    cum, out, stats) with the full samples, (data, 0, None, None, out, stats) without samples -- assembled by assemble_pieces."""
    pieces = []
    failure = []

    def on_piece(user, piece):
        try:
            pc = PieceCopy(piece.contents)
            if sink is None:
                pieces.append(pc)
                return 0
            return 1 if sink(pc) else 0
        except BaseException as e:               # an exception must not unwind through the C frames
            failure.append(e)
            return 2

    cb = PIECE_FN(on_piece)
    out, stats = HostOutput(), StreamStats()
    hb = _host_input(*b)
    if chained is not None:
        h, chained.h = chained.h, None                     # consumed by the call
        rc = lib().bwtm_merge_host_streamed(h, None, C.byref(hb), int(slice_records), int(samples), cb, None, C.byref(out), C.byref(stats))
    else:
        ha = _host_input(*a)
        rc = lib().bwtm_merge_host_streamed(None, C.byref(ha), C.byref(hb), int(slice_records), int(samples), cb, None, C.byref(out), C.byref(stats))
    if failure:
        raise failure[0]
    check(rc)
    if sink is not None:
        return out, stats
    data, width, x, y = assemble_pieces(pieces, list(out.C))
    return data, width, x, y, out, stats


class Upload(Handle):
    """An input on its way to the device (bwtm_upload): keeps the host array alive until it is consumed."""
    _free = "bwtm_upload_free"

    def __init__(self, handle, source):
        self.h, self.source = handle, source

    def finish(self):
        """-> Index (bwtm_upload_finish: waits for the copies, decodes, validates, transcodes)."""
        h, self.h = self.h, None
        out = _new(lib().bwtm_upload_finish, h)
        self.source = None
        return Index(out)

    def free(self):
        super().free()
        self.source = None


def upload_begin(data, sequences, bases):
    hi = _host_input(data, sequences, bases)
    return Upload(_new(lib().bwtm_upload_begin, C.byref(hi)), data)


def merge_host_pipelined(a=None, b=None, chained=None, pending=None, next=None, samples=True, keep=False, buffers=None):
    """bwtm_merge_host_pipelined: a = (data, sequences, bases) or chained = device Index (consumed); b likewise or pending = Upload
    (consumed); next = (data, sequences, bases) of the FOLLOWING merge's input, whose copies run under this merge's search.
    samples = RESULT_ON_DEVICE: nothing is encoded or downloaded (needs keep).  Returns (HostMerge, Upload or None)."""
    res = HostMerge()
    if buffers is not None:
        res.buffers = buffers

    def alloc(user, what, nbytes):
        buf = res.buffers.get(what)
        if buf is None or buf.nbytes < nbytes:
            if buf is not None:
                buf.free()
            buf = HostBuffer(nbytes)
            res.buffers[what] = buf
        return buf.ptr

    cb = ALLOC_FN(alloc)
    ha = _host_input(*a) if a is not None else None
    hb = _host_input(*b) if b is not None else None
    hn = _host_input(*next) if next is not None else None
    dev = None
    if chained is not None:
        dev, chained.h = chained.h, None
    pend = None
    if pending is not None:
        pend, pending.h = pending.h, None
    kp, np_ = vp(), vp()
    rc = lib().bwtm_merge_host_pipelined(dev, C.byref(ha) if ha else None, C.byref(hb) if hb else None, pend, C.byref(hn) if hn else None,
                                         C.byref(np_) if hn else None, cb, None, int(samples), C.byref(res.out), C.byref(kp) if keep else None)
    if pending is not None:
        pending.source = None
    if rc != 0:
        if buffers is None:
            res.free()
        check(rc)
    if keep:
        res.keep = Index(kp)
    return res, (Upload(np_, next[0]) if hn else None)


class SequenceCount(int):
    """What Index.sequences gives: the number of sequences, as the int it has always been -- and, called,
    Index.sequences(ids=None, first=0, count=None, max_len=0) -> (offsets, text): the sequences themselves (Index.extract_sequences)."""

    def __new__(cls, value, index):
        self = super().__new__(cls, value)
        self.index = index
        return self

    def __call__(self, ids=None, first=0, count=None, max_len=0):
        return self.index.extract_sequences(ids, first, count, max_len)

    def __reduce__(self):                 # copied or sent to another process it is the plain number (a handle does not travel)
        return (int, (int(self),))


def _opt_u64(a):
    return None if a is None else _u64(a)


class Index(Handle):
    """Device-resident FM-index (handle on bwtm_index)."""
    _free = "bwtm_index_free"

    def __init__(self, handle):
        self.h = vp(handle) if not isinstance(handle, vp) else handle

    @staticmethod
    def upload(data, sequences, bases, C_array=None):
        data = _u8(data)
        return Index(_new(lib().bwtm_index_upload, data, data.size, sequences, bases, _opt_u64(C_array)))

    @staticmethod
    def upload_streamed(data, sequences, bases, C_array=None):
        """bwtm_index_upload_streamed: the index (records and super table only) from chunks of the bytes, the stream never resident as a whole.
        Returns (Index, UploadStats)."""
        data = _u8(data)
        out, stats = vp(), UploadStats()
        check(lib().bwtm_index_upload_streamed(data, data.size, sequences, bases, _opt_u64(C_array), C.byref(out), C.byref(stats)))
        return Index(out), stats

    @staticmethod
    def from_device(ptr, nbytes, sequences, bases, C_array=None, borrow=False):
        """borrow=True: the index reads the caller's buffer in place (it must outlive the index)."""
        f = lib().bwtm_index_from_device_borrowed if borrow else lib().bwtm_index_from_device
        return Index(_new(f, vp(ptr), nbytes, sequences, bases, _opt_u64(C_array)))

    @staticmethod
    def from_symbols_device(ptr, bases):
        return Index(_new(lib().bwtm_index_from_symbols_device, vp(ptr), bases))

    bases = _scalar("bwtm_index_bases")
    sequences = property(lambda s: SequenceCount(lib().bwtm_index_sequences(s.h), s))
    nbytes = _scalar("bwtm_index_bytes")
    blocks = _scalar("bwtm_index_blocks")

    @property
    def C(self):
        out = np.zeros(SIGMA + 1, dtype=np.uint64)
        lib().bwtm_index_C(self.h, out)
        return out

    def encode(self):
        check(lib().bwtm_index_encode(self.h))
        return self

    def drop_native(self):
        check(lib().bwtm_index_drop_native(self.h))
        return self

    def device_data(self):
        """(device pointer, nbytes) of the native byte stream."""
        ptr = vp()
        n = u64(0)
        check(lib().bwtm_index_device_data(self.h, C.byref(ptr), C.byref(n)))
        return int(ptr.value or 0), int(n.value)

    total_nbytes = nbytes            # a slice of a sharded result reports the size of the whole stream here

    def data(self):
        out = np.zeros(self.nbytes, dtype=np.uint8)
        check(lib().bwtm_index_download_data(self.h, out, out.size))
        return out

    def download_into(self, out):
        """Native bytes into a caller's uint8 array (e.g. page-locked memory)."""
        assert out.dtype == np.uint8 and out.size >= self.nbytes
        check(lib().bwtm_index_download_data(self.h, out, out.size))
        return out

    def samples(self):
        nb = self.blocks
        be = np.zeros(nb, dtype=np.uint64)
        cum = np.zeros((SIGMA, nb + 1), dtype=np.uint64)
        check(lib().bwtm_index_download_samples(self.h, be, cum))
        return be, cum

    def samples_compact(self, width=None):
        """(width, fields [6][blocks] of uint8 / uint16 / uint32, anchors [6][ceil(blocks / 64)] uint64); see include/bwtm.h."""
        if width is None:
            w = C.c_int(0)
            check(lib().bwtm_index_samples_width(self.h, C.byref(w)))
            width = w.value
        if width == 8:
            return 8, None, None
        nb = self.blocks
        fields = np.zeros((SIGMA, nb), dtype=FIELD_DTYPES[width])
        anchors = np.zeros((SIGMA, (nb + 63) // 64), dtype=np.uint64)
        check(lib().bwtm_index_download_samples_compact(self.h, width, fields.ctypes.data_as(vp), anchors))
        return width, fields, anchors

    def rank(self, positions, comps):
        positions, comps = _u64(positions), _u8(comps)
        out = np.zeros(positions.size, dtype=np.uint64)
        check(lib().bwtm_rank_batch(self.h, positions, comps, positions.size, out))
        return out

    def inverse_select(self, positions):
        positions = _u64(positions)
        r = np.zeros(positions.size, dtype=np.uint64)
        c = np.zeros(positions.size, dtype=np.uint8)
        check(lib().bwtm_inverse_select_batch(self.h, positions, positions.size, r, c))
        return r, c

    def find(self, patterns):
        """Backward search of a list of patterns (sequences of comp values); returns (sp, ep) arrays."""
        text, offsets = pack_texts(patterns)
        sp = np.zeros(len(patterns), dtype=np.uint64)
        ep = np.zeros(len(patterns), dtype=np.uint64)
        check(lib().bwtm_find_batch(self.h, text, offsets, len(patterns), sp, ep))
        return sp, ep

    def find_approx(self, patterns, max_mismatches, max_hits=0):
        """Backward search with up to max_mismatches substitutions (bwtm_find_approx_batch).  Returns (hit_offsets [count + 1], sp, count,
        mismatches): the hits of pattern k are [hit_offsets[k], hit_offsets[k + 1]), each the range [sp, sp + count - 1] of one matched
        string, ascending when those strings are compared from their last symbol backwards.  One sizing call, then the filling call."""
        text, offsets = pack_texts(patterns)
        return _size_then_fill(partial(lib().bwtm_find_approx_batch, self.h, text, offsets, len(patterns), int(max_mismatches), int(max_hits)),
                               len(patterns), np.uint64, np.uint64, np.uint8)

    def find_edit(self, patterns, max_edits, max_hits=0):
        """Backward search within edit distance max_edits, indels included (bwtm_find_edit_batch).  Returns (hit_offsets [count + 1], sp,
        count, edits, lengths): the hits of pattern k are [hit_offsets[k], hit_offsets[k + 1]), each the range [sp, sp + count - 1] of one
        matched string of `lengths` symbols at distance `edits`, shortest first and, within a length, ascending when the strings are
        compared from their last symbol backwards.  One sizing call, then the filling call."""
        text, offsets = pack_texts(patterns)
        return _size_then_fill(partial(lib().bwtm_find_edit_batch, self.h, text, offsets, len(patterns), int(max_edits), int(max_hits)),
                               len(patterns), np.uint64, np.uint64, np.uint8, np.uint32)

    def matching_stats(self, patterns):
        """Matching statistics of a list of patterns (bwtm_matching_stats_batch).  Returns (lengths, sp, count), arrays over all symbols of
        the patterns in order: the entry of symbol i of pattern k, at sum(len(patterns[:k])) + i, is the longest match that ends with that
        symbol, lengths symbols long, and its range [sp, sp + count - 1]; (0, 0, 0) when the symbol alone does not occur."""
        text, offsets = pack_texts(patterns)
        total = int(offsets[-1])
        lengths = np.zeros(total, dtype=np.uint32)
        sp = np.zeros(total, dtype=np.uint64)
        count = np.zeros(total, dtype=np.uint64)
        check(lib().bwtm_matching_stats_batch(self.h, text, offsets, len(patterns), lengths, sp, count))
        return lengths, sp, count

    def mems(self, patterns, min_length=1):
        """Maximal exact matches of a list of patterns (bwtm_mem_batch).  Returns (hit_offsets [count + 1], begin, length, sp, count): the
        MEMs of pattern k are [hit_offsets[k], hit_offsets[k + 1]), begins (and ends) ascending; MEM h is patterns[k][begin[h]: begin[h] +
        length[h]], length[h] >= min_length, and occurs at the positions [sp[h], sp[h] + count[h] - 1].  One sizing call, then the filling call."""
        text, offsets = pack_texts(patterns)
        return _size_then_fill(partial(lib().bwtm_mem_batch, self.h, text, offsets, len(patterns), int(min_length)),
                               len(patterns), np.uint32, np.uint32, np.uint64, np.uint64)

    def extract(self, first, count):
        out = np.zeros(count, dtype=np.uint8)
        check(lib().bwtm_extract(self.h, first, count, out))
        return out

    def extract_sequences(self, ids=None, first=0, count=None, max_len=0):
        """Index.sequences(...): sequences by id (bwtm_sequences_extract): ids = an array of ids in any order, repeats allowed, or None for the ids
        first .. first + count - 1 (count=None: up to the last sequence).  Returns (offsets uint64 [count + 1], text uint8): sequence j is
        text[offsets[j]: offsets[j + 1]], comp values 1..5 in forward order.  One sizing call, then the extracting call."""
        ids, first, count = _ids_or_range(self, ids, first, count)
        offsets = np.zeros(count + 1, dtype=np.uint64)
        check(lib().bwtm_sequences_extract(self.h, ids, first, count, int(max_len), offsets, None, 0))
        text = np.zeros(int(offsets[-1]), dtype=np.uint8)
        if text.size > 0:
            check(lib().bwtm_sequences_extract(self.h, ids, first, count, int(max_len), offsets, text, text.size))
        return offsets, text

    def locator(self, max_len=0):
        """The table that turns BWT positions into (sequence id, offset) (bwtm_locator_create).  The locator borrows this index."""
        return Locator(self, max_len)

    def kmers(self, k, skip=5, min_count=1):
        """The distinct k-mers of the collection with their counts and BWT ranges (bwtm_kmers_create); skip = the comp of N."""
        return Kmers(self, k, skip, min_count)

    def kmer_join(self, other, k, skip=5, min_a=0, max_a=None, min_b=0, max_b=None, min_sum=1):
        """The k-mers of this index (a) and of `other` (b) side by side, with their counts and insertion points in each
        (bwtm_kmer_join_create); max_x=None: no upper bound."""
        return KmerJoin(self, other, k, skip, min_a, max_a, min_b, max_b, min_sum)


KMER_MAX_K = 32


def kmer_comps(skip):
    """The comp values of the k-mer alphabet: 1..5 without skip, ascending."""
    return np.array([c for c in range(1, 6) if c != int(skip)], dtype=np.uint8)


def decode_kmers(codes, k, skip):
    """Codes of k-mers (2 bits per symbol, the first symbol in the highest used bits) -> rows of k comp values."""
    codes = np.ascontiguousarray(codes, dtype=np.uint64)
    shifts = (2 * np.arange(int(k) - 1, -1, -1)).astype(np.uint64)
    return kmer_comps(skip)[((codes[:, None] >> shifts[None, :]) & np.uint64(3)).astype(np.int64)]


class Kmers(Handle):
    """The kept k-mers of an index in ascending order, on the device (handle on bwtm_kmers).  It does not borrow the index."""
    _free, _freed = "bwtm_kmers_free", "the k-mers have been freed"

    def __init__(self, index, k, skip=5, min_count=1):
        self.h = _new(lib().bwtm_kmers_create, index.h, int(k), int(skip), int(min_count))
        self.k, self.skip = int(k), int(skip)

    distinct = _scalar("bwtm_kmers_distinct")
    total = _scalar("bwtm_kmers_total")
    nbytes = _scalar("bwtm_kmers_bytes")

    def levels(self):
        """nodes[t] = distinct (t + 1)-mers with count >= min_count, t < k."""
        self._live()
        nodes = np.zeros(KMER_MAX_K, dtype=np.uint64)
        check(lib().bwtm_kmers_levels(self.h, nodes))
        return nodes[: self.k]

    def download(self, first=0, count=None):
        """(codes, counts, sp) of the entries [first, first + count) (count=None: up to the last one)."""
        self._live()
        if count is None:
            count = max(self.distinct - int(first), 0)
        if int(first) + int(count) > self.distinct:                      # the library says so, before arrays of that size are made
            check(lib().bwtm_kmers_download(self.h, int(first), int(count), None, None, None))
        codes, counts, sp = (np.zeros(int(count), dtype=np.uint64) for _ in range(3))
        check(lib().bwtm_kmers_download(self.h, int(first), int(count), codes, counts, sp))
        return codes, counts, sp

    def histogram(self, bins):
        """hist[j] = kept k-mers of count j, the last bin those of count >= bins - 1."""
        self._live()
        hist = np.zeros(max(int(bins), 0), dtype=np.uint64)
        check(lib().bwtm_kmers_histogram(self.h, int(bins), hist))
        return hist

    def corrector(self, threshold, skip=5):
        """The solid k-mers (count >= threshold) as a lookup table for error correction (bwtm_corrector_create); skip = the comp of N,
        the one the k-mers were made with.  The corrector copies what it needs: these k-mers may be freed at once."""
        self._live()
        return Corrector(self, threshold, skip)

    def unitigs(self, threshold, skip=5):
        """The unitigs of the k-mer graph over the k-mers of count >= threshold (bwtm_unitigs_create); skip = the comp of N, the one the
        k-mers were made with.  The graph copies what it needs: these k-mers may be freed at once."""
        self._live()
        return Unitigs(self, threshold, skip)


CORRECT_CLEAN, CORRECT_CORRECTED, CORRECT_FAILED, CORRECT_SHORT = 0, 1, 2, 3
CORRECT_STATS = ("lookups", "rounds", "max_edits", "batches")


class Corrector(Handle):
    """The solid k-mers of a spectrum on the device, and the correction of reads against them (handle on bwtm_corrector)."""
    _free, _freed = "bwtm_corrector_free", "the corrector has been freed"

    def __init__(self, kmers, threshold, skip=5):
        self.h = _new(lib().bwtm_corrector_create, kmers.h, int(skip), int(threshold))
        self.skip, self.threshold = int(skip), max(int(threshold), 1)

    solid = _scalar("bwtm_corrector_solid")
    nbytes = _scalar("bwtm_corrector_bytes")
    k = _scalar("bwtm_corrector_k")

    def correct(self, patterns, max_rounds=10):
        """Reads from the host (bwtm_correct_batch): a list of sequences of comp values 1..5.  Returns (list of uint8 arrays, status
        uint8 [count], edits uint32 [count]); status is one of CORRECT_CLEAN / _CORRECTED / _FAILED / _SHORT."""
        self._live()
        text, offsets = pack_texts(patterns)
        out = np.zeros(max(text.size, 1), dtype=np.uint8)
        status = np.zeros(len(patterns), dtype=np.uint8)
        edits = np.zeros(len(patterns), dtype=np.uint32)
        check(lib().bwtm_correct_batch(self.h, text, offsets, len(patterns), int(max_rounds), out, status, edits))
        return [out[int(offsets[j]): int(offsets[j + 1])] for j in range(len(patterns))], status, edits

    def correct_sequences(self, index, ids=None, first=0, count=None, max_len=0, max_rounds=10, text=True):
        """Reads of an index, extracted and corrected on the device (bwtm_correct_sequences); ids / first / count / max_len as in
        Index.sequences.  Returns (offsets uint64 [count + 1], text uint8 or None, status, edits).  text=False: one status call.
        Otherwise the sizing call of bwtm_sequences_extract, then the filling call."""
        self._live()
        ids, first, count = _ids_or_range(index, ids, first, count)
        offsets = np.zeros(count + 1, dtype=np.uint64)
        status = np.zeros(count, dtype=np.uint8)
        edits = np.zeros(count, dtype=np.uint32)
        args = (self.h, index.h, ids, first, count, int(max_len), int(max_rounds), offsets)
        if not text:
            check(lib().bwtm_correct_sequences(*args, None, 0, status, edits))
            return offsets, None, status, edits
        check(lib().bwtm_sequences_extract(index.h, ids, first, count, int(max_len), offsets, None, 0))     # the size
        out = np.zeros(int(offsets[-1]), dtype=np.uint8)
        check(lib().bwtm_correct_sequences(*args, out if out.size else None, out.size, status, edits))
        return offsets, out, status, edits

    @staticmethod
    def correct_stats():
        return correct_stats()


UNITIG_CIRCULAR = 1
UNITIG_NONE = (1 << 64) - 1
UNITIG_STATS = ("lookups", "longest", "circular_nodes", "jump_rounds")


class Unitigs(Handle):
    """The compacted de Bruijn graph over the solid k-mers of a spectrum, on the device (handle on bwtm_unitigs)."""
    _free, _freed = "bwtm_unitigs_free", "the unitigs have been freed"

    def __init__(self, kmers, threshold, skip=5):
        self.h = _new(lib().bwtm_unitigs_create, kmers.h, int(skip), int(threshold))
        self.skip, self.threshold = int(skip), max(int(threshold), 1)

    count = _scalar("bwtm_unitigs_count")
    nodes = _scalar("bwtm_unitigs_nodes")
    symbols = _scalar("bwtm_unitigs_symbols")
    bytes = _scalar("bwtm_unitigs_bytes")
    k = _scalar("bwtm_unitigs_k")

    def download(self, first=0, count=None):
        """(offsets uint64 [count + 1], text uint8, nodes, occurrences uint64 [count], flags uint8 [count], links uint64 [count, 4]) of the
        unitigs [first, first + count) (count=None: up to the last one): the sizing call, then the filling call.  Unitig first + j has the
        text text[offsets[j]: offsets[j + 1]] (comp values); a link is a unitig's number in the whole graph or UNITIG_NONE."""
        self._live()
        if count is None:
            count = max(self.count - int(first), 0)
        first, count = int(first), int(count)
        offsets = np.zeros(count + 1, dtype=np.uint64)
        check(lib().bwtm_unitigs_download(self.h, first, count, offsets, None, 0, None, None, None, None))     # the size
        text = np.zeros(int(offsets[-1]), dtype=np.uint8)
        nodes, occurrences = np.zeros(count, dtype=np.uint64), np.zeros(count, dtype=np.uint64)
        flags, links = np.zeros(count, dtype=np.uint8), np.zeros((count, 4), dtype=np.uint64)
        check(lib().bwtm_unitigs_download(self.h, first, count, offsets, text if text.size else None, text.size, nodes, occurrences, flags, links))
        return offsets, text, nodes, occurrences, flags, links

    def place(self, codes):
        """(unitig, offset) uint64 arrays: where each code sits in the graph, UNITIG_NONE twice for a code that is no node."""
        self._live()
        codes = _u64(codes)
        unitig, offset = np.zeros(codes.size, dtype=np.uint64), np.zeros(codes.size, dtype=np.uint64)
        check(lib().bwtm_unitigs_place(self.h, codes, codes.size, unitig, offset))
        return unitig, offset

    @staticmethod
    def stats():
        return unitigs_stats()


def unitigs_stats():
    """What the calling thread's last bwtm_unitigs_create did (bwtm_unitigs_stats): table lookups, the longest unitig in nodes, nodes in
    circular unitigs, rounds of pointer jumping."""
    return _stats(lib().bwtm_unitigs_stats, UNITIG_STATS)


def correct_stats():
    """What the calling thread's last correct call did (bwtm_correct_stats): table lookups, rounds run over all reads, the most edits in one
    read, batches."""
    return _stats(lib().bwtm_correct_stats, CORRECT_STATS)


KMER_JOIN_NO_BOUND = (1 << 64) - 1
KMER_JOIN_STATS = ("only_a", "only_b", "both", "only_a_occurrences_a", "only_b_occurrences_b", "both_occurrences_a", "both_occurrences_b")


class KmerJoin(Handle):
    """The kept k-mers of two indexes in ascending order with their counts and insertion points in each, on the device (handle on
    bwtm_kmer_join).  It does not borrow the indexes."""
    _free, _freed = "bwtm_kmer_join_free", "the k-mer join has been freed"

    def __init__(self, a, b, k, skip=5, min_a=0, max_a=None, min_b=0, max_b=None, min_sum=1):
        self.h = _new(lib().bwtm_kmer_join_create, a.h, b.h, int(k), int(skip), int(min_a), KMER_JOIN_NO_BOUND if max_a is None else int(max_a),
                      int(min_b), KMER_JOIN_NO_BOUND if max_b is None else int(max_b), int(min_sum))
        self.k, self.skip = int(k), int(skip)

    distinct = _scalar("bwtm_kmer_join_distinct")
    nbytes = _scalar("bwtm_kmer_join_bytes")

    def levels(self):
        """nodes[t] = the (t + 1)-mers the lower bounds keep for t < k - 1; nodes[k - 1] = the result (upper bounds applied)."""
        self._live()
        nodes = np.zeros(KMER_MAX_K, dtype=np.uint64)
        check(lib().bwtm_kmer_join_levels(self.h, nodes))
        return nodes[: self.k]

    def download(self, first=0, count=None):
        """(codes, count_a, count_b, sp_a, sp_b) of the entries [first, first + count) (count=None: up to the last one)."""
        self._live()
        if count is None:
            count = max(self.distinct - int(first), 0)
        if int(first) + int(count) > self.distinct:                      # the library says so, before arrays of that size are made
            check(lib().bwtm_kmer_join_download(self.h, int(first), int(count), None, None, None, None, None))
        arrays = tuple(np.zeros(int(count), dtype=np.uint64) for _ in range(5))
        check(lib().bwtm_kmer_join_download(self.h, int(first), int(count), *arrays))
        return arrays

    def summary(self):
        """The seven numbers of bwtm_kmer_join_summary by name (KMER_JOIN_STATS)."""
        self._live()
        return _stats(lib().bwtm_kmer_join_summary, KMER_JOIN_STATS, self.h)


class Locator(Handle):
    """From BWT positions of an index to (sequence id, offset of the suffix in that sequence) (handle on bwtm_locator).  It keeps a reference to
    the index it borrows; free it before the index is consumed by a merge."""
    _free, _freed = "bwtm_locator_free", "the locator has been freed"

    def __init__(self, index, max_len=0):
        self.h = _new(lib().bwtm_locator_create, index.h, int(max_len))
        self.index = index

    nbytes = _scalar("bwtm_locator_bytes")

    def free(self):
        super().free()
        self.index = None

    def locate(self, positions):
        """(ids, offsets) of an array of BWT positions."""
        self._live()
        positions = _u64(positions)
        ids = np.zeros(positions.size, dtype=np.uint64)
        offs = np.zeros(positions.size, dtype=np.uint64)
        check(lib().bwtm_locate_batch(self.h, positions, positions.size, ids, offs))
        return ids, offs

    def locate_ranges(self, sp, ep, max_hits=0):
        """(hit_offsets [count + 1], ids, offsets) of closed ranges [sp, ep] (sp > ep: empty): the hits of range r are
        [hit_offsets[r], hit_offsets[r + 1]) in ascending BWT position.  One sizing call, then the locating call."""
        self._live()
        sp, ep = _u64(sp), _u64(ep)
        assert sp.size == ep.size
        return _size_then_fill(partial(lib().bwtm_locate_ranges, self.h, sp, ep, sp.size, int(max_hits)), sp.size, np.uint64, np.uint64)

    def locate_patterns(self, patterns, max_hits=0):
        """Every occurrence of every pattern (sequences of comp values): find, the sizing call, the locating call.  Returns
        (hit_offsets, ids, offsets); pattern k occurs at offset offsets[h] of sequence ids[h] for h in [hit_offsets[k], hit_offsets[k + 1])."""
        sp, ep = self.index.find(patterns)
        return self.locate_ranges(sp, ep, max_hits)

    def locate_approx(self, patterns, max_mismatches, max_hits=0):
        """Every occurrence of every pattern with up to max_mismatches substitutions: Index.find_approx, then locate_ranges on the hits'
        ranges.  Returns (hit_offsets, sp, count, mismatches) of find_approx (max_hits caps the hits of a pattern, not their occurrences)
        and (occ_offsets, ids, offsets) of locate_ranges over the hits: hit h occurs at offsets[j] of sequence ids[j] for j in
        [occ_offsets[h], occ_offsets[h + 1])."""
        hit_offsets, sp, count, mismatches = self.index.find_approx(patterns, max_mismatches, max_hits)
        occ_offsets, ids, offs = self.locate_ranges(sp, sp + count - np.uint64(1))
        return hit_offsets, sp, count, mismatches, occ_offsets, ids, offs

    def locate_edit(self, patterns, max_edits, max_hits=0):
        """Every occurrence of every pattern within edit distance max_edits: Index.find_edit, then locate_ranges on the hits' ranges.
        Returns (hit_offsets, sp, count, edits, lengths) of find_edit (max_hits caps the hits of a pattern, not their occurrences) and
        (occ_offsets, ids, offsets) of locate_ranges over the hits: hit h occurs at offsets[j] of sequence ids[j] for j in
        [occ_offsets[h], occ_offsets[h + 1]), over lengths[h] symbols."""
        hit_offsets, sp, count, edits, lengths = self.index.find_edit(patterns, max_edits, max_hits)
        occ_offsets, ids, offs = self.locate_ranges(sp, sp + count - np.uint64(1))
        return hit_offsets, sp, count, edits, lengths, occ_offsets, ids, offs

    def locate_mems(self, patterns, min_length, max_hits=0):
        """Every occurrence of every maximal exact match of every pattern: Index.mems, then locate_ranges on the MEMs' ranges.  Returns
        (hit_offsets, begin, length, sp, count) of mems and (occ_offsets, ids, offsets) of locate_ranges over the MEMs (max_hits caps the
        occurrences of a MEM): MEM h occurs at offsets[j] of sequence ids[j] for j in [occ_offsets[h], occ_offsets[h + 1])."""
        hit_offsets, begin, length, sp, count = self.index.mems(patterns, min_length)
        occ_offsets, ids, offs = self.locate_ranges(sp, sp + count - np.uint64(1), max_hits)
        return hit_offsets, begin, length, sp, count, occ_offsets, ids, offs

    def overlaps(self, ids=None, first=0, count=None, min_overlap=1, max_hits=0, skip_self=False):
        """Suffix-prefix overlaps of sequences of the index (bwtm_overlap_sequences): the queries are ids (any order, repeats allowed), or
        first .. first + count - 1 (count=None: up to the last sequence).  Returns (hit_offsets [count + 1], ids, lengths): for h in
        [hit_offsets[k], hit_offsets[k + 1]), the first lengths[h] symbols of sequence ids[h] are the last lengths[h] symbols of query k,
        lengths[h] >= min_overlap; longest overlap first, then targets in BWT order.  max_hits > 0 keeps the first max_hits hits of every
        query.  skip_self drops, on the host, the hit of a query with itself over its whole length and recomputes hit_offsets; it applies
        AFTER the max_hits cut, so a query can keep max_hits - 1 hits."""
        self._live()
        ids, first, count = _ids_or_range(self.index, ids, first, count)
        queries = ids if ids is not None else np.arange(first, first + count, dtype=np.uint64)
        hit_offsets, targets, lengths = _size_then_fill(
            partial(lib().bwtm_overlap_sequences, self.h, ids, first, count, int(min_overlap), int(max_hits)), count, np.uint64, np.uint64)
        if skip_self and targets.size > 0:
            per_query = np.diff(hit_offsets).astype(np.int64)
            owner = np.repeat(np.arange(count), per_query)
            # a query that has hits at all hits itself over its whole length L, and no hit is longer: the first hit of a query has length L
            full = lengths[hit_offsets[:-1].astype(np.int64)[owner]]
            drop = (targets == queries[owner]) & (lengths == full)
            keep = ~drop
            kept_per_query = np.bincount(owner[keep], minlength=count).astype(np.uint64)
            hit_offsets = np.zeros(count + 1, dtype=np.uint64)
            hit_offsets[1:] = np.cumsum(kept_per_query)
            targets, lengths = targets[keep], lengths[keep]
        return hit_offsets, targets, lengths

    def overlap_patterns(self, patterns, min_overlap, max_hits=0):
        """Suffix-prefix overlaps of patterns that need not be sequences of the index (bwtm_overlap_batch): (hit_offsets, ids, lengths) as in
        overlaps(); a pattern holds comp values 1..5 and may be longer than every sequence."""
        self._live()
        text, offsets = pack_texts(patterns)
        return _size_then_fill(partial(lib().bwtm_overlap_batch, self.h, text, offsets, len(patterns), int(min_overlap), int(max_hits)),
                               len(patterns), np.uint64, np.uint64)


class RankArray(Handle):
    """Device-resident rank array (handle on bwtm_ra)."""
    _free = "bwtm_ra_free"

    def __init__(self, a, b, device_buffer=None, nbytes=0):
        if device_buffer is None:
            self.h = _new(lib().bwtm_ra_create, a.h, b.h)
        else:
            self.h = _new(lib().bwtm_ra_create_on, a.h, b.h, vp(device_buffer), nbytes)
        self.n_out = a.bases + b.bases
        self.nb = b.bases

    def search(self, a, b, seq_first, seq_last):
        check(lib().bwtm_search(a.h, b.h, seq_first, seq_last, self.h))

    def device_buffer(self):
        ptr = vp()
        n = u64(0)
        check(lib().bwtm_ra_device_buffer(self.h, C.byref(ptr), C.byref(n)))
        return int(ptr.value), int(n.value)

    def or_from(self, other):
        """self |= other's bits (another rank array for the same inputs on the same device)."""
        ptr, n = other.device_buffer()
        check(lib().bwtm_ra_or_from(self.h, vp(ptr), n))

    def subset_check(self, whole):
        """(set bits of this array, 64-bit words in which it has a bit that `whole` lacks)."""
        ones, bad = u64(0), u64(0)
        check(lib().bwtm_ra_subset_check(self.h, whole.h, C.byref(ones), C.byref(bad)))
        return int(ones.value), int(bad.value)

    def finalize(self):
        check(lib().bwtm_ra_finalize(self.h))
        return self

    def range_counts(self, rec_first, rec_last):
        """Output-range finalize, step 1: (set bits of the range, per-super local counts [nsup], the words of the range's last chunk [128])."""
        nsup = (self.n_out >> 25) + 1
        ones = u64(0)
        local = np.zeros(nsup, dtype=np.uint64)
        tail = np.zeros(128, dtype=np.uint64)
        check(lib().bwtm_ra_range_counts(self.h, rec_first, rec_last, C.byref(ones), local, tail))
        return int(ones.value), local, tail

    def finalize_range(self, rec_first, rec_last, ones_before, ones_total, super_boff, halo_words=None):
        """Output-range finalize, step 2 (include/bwtm.h: bwtm_ra_finalize_range)."""
        super_boff, halo = _u64(super_boff), _opt_u64(halo_words)
        assert super_boff.size == (self.n_out >> 25) + 1
        assert halo is None or halo.size == 128
        check(lib().bwtm_ra_finalize_range(self.h, rec_first, rec_last, ones_before, ones_total, super_boff, halo))
        return self

    values = _scalar("bwtm_ra_values")

    def download(self):
        out = np.zeros(self.nb, dtype=np.uint64)
        check(lib().bwtm_ra_download(self.h, out, out.size))
        return out

    def runs(self):
        """The rank array as maximal (rank, count) runs (the reference's own form)."""
        n = u64(0)
        check(lib().bwtm_ra_download_runs(self.h, None, None, 0, C.byref(n)))
        ranks = np.zeros(n.value, dtype=np.uint64)
        counts = np.zeros(n.value, dtype=np.uint64)
        check(lib().bwtm_ra_download_runs(self.h, ranks, counts, n.value, C.byref(n)))
        return ranks, counts

    def bits(self):
        words = (self.n_out + 63) // 64
        out = np.zeros(words, dtype=np.uint64)
        check(lib().bwtm_ra_download_bits(self.h, out, out.size))
        return out


class Slice(Handle):
    """One GPU's share of a merged index: the output records [rec_first, rec_last) (handle on bwtm_slice)."""
    _free = "bwtm_slice_free"

    def __init__(self, a, b, ra, rec_first, rec_last):
        self.h = _new(lib().bwtm_interleave_range, a.h, b.h, ra.h, rec_first, rec_last)
        self.total_nbytes = 0

    def lasthead(self):
        v = u64(0)
        check(lib().bwtm_slice_lasthead(self.h, C.byref(v)))
        return int(v.value)

    def size_table(self, heads_before):
        t = np.zeros(64, dtype=np.uint64)
        check(lib().bwtm_slice_size_table(self.h, int(heads_before), t))
        return t

    def encode(self, byte_offset):
        check(lib().bwtm_slice_encode(self.h, int(byte_offset)))
        return self

    byte_first = _scalar("bwtm_slice_byte_first")
    nbytes = _scalar("bwtm_slice_bytes")
    block_first = _scalar("bwtm_slice_block_first")
    blocks = _scalar("bwtm_slice_blocks")

    def first_block_start(self):
        """Sequence position at which the slice's first block starts; None if it has no block."""
        v = u64(0)
        check(lib().bwtm_slice_first_block_start(self.h, C.byref(v)))
        return None if v.value == (1 << 64) - 1 else int(v.value)

    def data(self):
        out = np.zeros(self.nbytes, dtype=np.uint8)
        check(lib().bwtm_slice_download_data(self.h, out, out.size))
        return out

    def data_into(self, out):
        """The slice's bytes into a caller-provided uint8 array (e.g. page-locked: HostBuffer.array)."""
        check(lib().bwtm_slice_download_data(self.h, out, out.size))
        return out[: self.nbytes]

    def samples(self, next_block_start):
        nb = self.blocks
        be = np.zeros(nb, dtype=np.uint64)
        cum = np.zeros((SIGMA, nb), dtype=np.uint64)
        check(lib().bwtm_slice_download_samples(self.h, int(next_block_start), be, cum))
        return be, cum

    def extract(self, first, count):
        out = np.zeros(count, dtype=np.uint8)
        check(lib().bwtm_slice_extract(self.h, first, count, out))
        return out


class Group:
    """The parts of a merge over partitioned records (bwtm_group): `name` = a POSIX shared-memory name unique to the group (None for one part)."""

    def __init__(self, name, part, parts):
        self.h = _new(lib().bwtm_group_create, name.encode() if name else None, int(part), int(parts))
        self.part, self.parts = int(part), int(parts)

    def free(self):
        if self.h:
            lib().bwtm_group_free(self.h)
            self.h = None

    def barrier(self):
        check(lib().bwtm_group_barrier(self.h))

    def allgather(self, mine):
        """mine: a numpy array; returns [parts, ...] of the same dtype."""
        mine = np.ascontiguousarray(mine)
        out = np.zeros((self.parts,) + mine.shape, dtype=mine.dtype)
        check(lib().bwtm_group_allgather(self.h, mine.ctypes.data, mine.nbytes, out.ctypes.data))
        return out

    def abort(self):
        if self.h:
            lib().bwtm_group_abort(self.h)


def host_index(data, cum, sequences, bases):
    """bwtm_host_index over numpy arrays (kept alive by the returned object): data = the native bytes, cum[6][blocks + 1] = the samples."""
    assert data.dtype == np.uint8 and data.flags["C_CONTIGUOUS"]
    cum = np.ascontiguousarray(cum, dtype=np.uint64)
    blocks = cum.shape[1] - 1
    x = HostIndex()
    x.data = data.ctypes.data; x.nbytes = data.size; x.blocks = blocks; x.sequences = int(sequences); x.bases = int(bases)
    totals = [int(cum[c][blocks]) for c in range(SIGMA)]
    for c in range(SIGMA + 1):
        x.C[c] = sum(totals[:c])
    x.cum = cum.ctypes.data
    x._keep = (data, cum)
    return x


def partition_cuts_host(a, b, parts, kmer=0):
    """(cut_a, cut_b): parts + 1 ranks each (bwtm_partition_cuts_host); a, b = host_index() objects."""
    ca = np.zeros(parts + 1, dtype=np.uint64); cb = np.zeros(parts + 1, dtype=np.uint64)
    check(lib().bwtm_partition_cuts_host(C.byref(a), C.byref(b), int(parts), int(kmer), ca, cb))
    return [int(v) for v in ca], [int(v) for v in cb]


def window_blocks(x, pos_first, pos_last):
    """(block_first, block_end, first_position, counts_before[6]) of the blocks that cover the records of [pos_first, pos_last] (bwtm_window_blocks)."""
    b0, b1, fp = u64(0), u64(0), u64(0)
    before = (u64 * 6)()
    check(lib().bwtm_window_blocks(C.byref(x), int(pos_first), int(pos_last), C.byref(b0), C.byref(b1), C.byref(fp), before))
    return int(b0.value), int(b1.value), int(fp.value), before


class Part(Handle):
    """One part of a merge over partitioned records (bwtm_part): created in the calling thread's context."""
    _free = "bwtm_part_free"

    def __init__(self, group, a, b, cut_a, cut_b):
        """a, b: host_index() objects (or anything with bases / sequences / C)."""
        ha, hb = IndexHeader(), IndexHeader()
        for h, x in ((ha, a), (hb, b)):
            h.bases = int(x.bases); h.sequences = int(x.sequences)
            for c in range(SIGMA + 1):
                h.C[c] = int(x.C[c])
        ca = (u64 * len(cut_a))(*[int(v) for v in cut_a]); cb = (u64 * len(cut_b))(*[int(v) for v in cut_b])
        self.h = _new(lib().bwtm_part_create, group.h, C.byref(ha), C.byref(hb), ca, cb)
        self.group = group

    def window(self, which):
        lo, hi = u64(0), u64(0)
        check(lib().bwtm_part_window(self.h, int(which), C.byref(lo), C.byref(hi)))
        return int(lo.value), int(hi.value)

    def share(self, which, x):
        """(byte offset, byte count, first_position, counts_before) of this part's share of host index x's stream."""
        lo, hi = self.window(which)
        b0, b1, fp, before = window_blocks(x, lo, hi)
        return b0 * 64, min(b1 * 64, int(x.nbytes)) - b0 * 64, fp, before

    def upload(self, which, ptr, nbytes, first_position, counts_before, on_device=False):
        check(lib().bwtm_part_upload(self.h, int(which), vp(ptr), int(nbytes), int(first_position), counts_before, 1 if on_device else 0))

    def upload_host(self, which, x):
        off, count, fp, before = self.share(which, x)
        self.upload(which, x.data + off, count, fp, before, on_device=False)

    def search(self):
        check(lib().bwtm_part_search(self.h))

    def finish(self):
        """The part's encoded Slice (total_nbytes, byte_offset, next_block_start set)."""
        out, off, total, nxt = vp(), u64(0), u64(0), u64(0)
        check(lib().bwtm_part_finish(self.h, C.byref(out), C.byref(off), C.byref(total), C.byref(nxt)))
        s = Slice.__new__(Slice)
        s.h = out; s.total_nbytes = int(total.value); s.byte_offset = int(off.value); s.next_block_start = int(nxt.value)
        return s

    def stats(self):
        info = PartInfo()
        check(lib().bwtm_part_stats(self.h, C.byref(info)))
        return {k: getattr(info, k) for k, _ in PartInfo._fields_}


def merged_records(a, b):
    return int(lib().bwtm_merged_records(a.h, b.h))


def slice_bounds(nrecs, parts, part):
    f, l = u64(0), u64(0)
    check(lib().bwtm_slice_bounds(nrecs, parts, part, C.byref(f), C.byref(l)))
    return int(f.value), int(l.value)


def slice_bounds_equal(nrecs, parts, part):
    """(rec_first, rec_last, bytes of the bitvector per range) of EQUAL output ranges (what a reduce-scatter wants)."""
    f, l, sb = u64(0), u64(0), u64(0)
    check(lib().bwtm_slice_bounds_equal(nrecs, parts, part, C.byref(f), C.byref(l), C.byref(sb)))
    return int(f.value), int(l.value), int(sb.value)


def fold_offsets(tables):
    """tables: [parts, 64] uint64 -> offsets [parts + 1] (byte offset of every slice, then the size of the stream)."""
    tables = np.ascontiguousarray(tables, dtype=np.uint64)
    out = np.zeros(tables.shape[0] + 1, dtype=np.uint64)
    check(lib().bwtm_fold_offsets(tables, tables.shape[0], out))
    return out


def ra_buffer_bytes(a, b):
    return int(lib().bwtm_ra_buffer_bytes(a.h, b.h))


def interleave(a, b, ra):
    return Index(_new(lib().bwtm_interleave, a.h, b.h, ra.h))


def merge(a, b):
    """FMI::FMI(a, b): search + finalize + interleave + encode + samples on the device."""
    return Index(_new(lib().bwtm_merge, a.h, b.h))


def merge_consume(a, b):
    """The same with the reference's ownership: a and b are destroyed, their memory released progressively."""
    ha, hb = a.h, b.h
    a.h = None; b.h = None
    return Index(_new(lib().bwtm_merge_consume, ha, hb))


class Builder(Handle):
    """Reads -> index on the GPU (bwtm_builder_*): leaves by suffix sort, grown by the merger itself."""
    _free = "bwtm_builder_free"

    def __init__(self, leaf_reads=0):
        self.h = _new(lib().bwtm_builder_create, leaf_reads)

    def add(self, reads, lengths=None):
        """reads: [n, width] uint8 numpy array of comp values 1..5 (host); lengths: optional uint32 [n]."""
        reads = np.ascontiguousarray(reads, dtype=np.uint8)
        n, width = reads.shape
        lp = None
        if lengths is not None:
            lengths = np.ascontiguousarray(lengths, dtype=np.uint32)
            assert lengths.shape == (n,)
            lp = vp(lengths.ctypes.data)
        check(lib().bwtm_builder_add(self.h, vp(reads.ctypes.data), n, width, width, lp, 0))

    def add_device(self, ptr, nreads, width, stride=None, lengths_ptr=None):
        """The same for rows already on the device (lengths_ptr: device uint32 [nreads] or None)."""
        check(lib().bwtm_builder_add(self.h, vp(ptr), nreads, width, width if stride is None else stride,
                                     vp(lengths_ptr) if lengths_ptr else None, 1))

    reads = _scalar("bwtm_builder_reads")

    def finish(self):
        h, self.h = self.h, None                           # given up before the call
        return Index(_new(lib().bwtm_builder_finish, h))


class PoolInfo(C.Structure):
    _fields_ = [("held_bytes", u64), ("cached_bytes", u64), ("peak_bytes", u64), ("mapped_blocks", u64), ("address_bytes_reserved", u64),
                ("address_space_exhausted", C.c_int), ("hipmalloc_fallbacks", u64)]


def pool_stats():
    info = PoolInfo()
    check(lib().bwtm_pool_stats(C.byref(info)))
    return {k: int(getattr(info, k)) for k, _ in PoolInfo._fields_}


FIND_STATS = ("expanded", "frontier_peak", "batch_hits", "levels")
MEM_STATS = ("steps", "tasks", "mems", "batches")


def find_approx_stats():
    """What the calling thread's last Index.find_approx call did (bwtm_find_approx_stats; of its second, filling call when there were hits):
    nodes expanded, the largest frontier of a batch, the most hits of a batch before max_hits, levels run."""
    return _stats(lib().bwtm_find_approx_stats, FIND_STATS)


def find_edit_stats():
    """What the calling thread's last Index.find_edit call did (bwtm_find_edit_stats; of its second, filling call when there were hits):
    nodes expanded, the largest frontier of a batch, the most hits of a batch before max_hits, levels run."""
    return _stats(lib().bwtm_find_edit_stats, FIND_STATS)


def mem_stats():
    """What the calling thread's last Index.matching_stats or Index.mems call did (bwtm_mem_stats; of its second, filling call when there
    were MEMs): LF steps taken, tasks run, MEMs before min_length, batches."""
    return _stats(lib().bwtm_mem_stats, MEM_STATS)


def pool_poison_stats():
    """(fills, bytes) of the poison mode (BWTM_POOL_POISON in the environment), process-wide; (0, 0) when it is off."""
    fills, nbytes = u64(0), u64(0)
    check(lib().bwtm_pool_poison_stats(C.byref(fills), C.byref(nbytes)))
    return int(fills.value), int(nbytes.value)


def profile_enable(on=True):
    check(lib().bwtm_profile_enable(1 if on else 0))


def profile_only(name=None):
    check(lib().bwtm_profile_only(name.encode() if name else None))


def profile_reset():
    check(lib().bwtm_profile_reset())


def frontier_step_forms():
    """Step-kernel launches since the last profile_reset by the form of the frontier's coordinates: (absolute, absolute in and
    class-relative out, class-relative); counted whether or not profiling is enabled."""
    f = lib().bwtm_frontier_step_forms      # bound on first use, not with SYMBOLS: a library of an earlier round (BWTM_LIB, the A/B tools) still loads
    f.restype = C.c_int; f.argtypes = [p_u64]
    n = (u64 * 3)()
    check(f(n))
    return tuple(int(v) for v in n)


def transcode_forms():
    """Launches of k_build_recs / k_build_recs_chunk since the last profile_reset by instantiation, 16 counts: index 8 * chunk + 2 * w +
    uniform, w = 0 / 1 / 2 for the windows of 8192 / 16384 / 32768 positions and 3 for 32768 with the cooperative fill; counted whether or
    not profiling is enabled."""
    f = lib().bwtm_transcode_forms          # bound on first use, as frontier_step_forms is
    f.restype = C.c_int; f.argtypes = [p_u64]
    n = (u64 * 16)()
    check(f(n))
    return tuple(int(v) for v in n)


def profile_read():
    """{kernel name: (total_ms, launches)} since the last reset."""
    cap = 64
    names = (C.c_char_p * cap)()
    ms = (C.c_double * cap)()
    n = (u64 * cap)()
    k = lib().bwtm_profile_read(names, ms, n, cap)
    return {names[i].decode(): (ms[i], int(n[i])) for i in range(min(k, cap))}
