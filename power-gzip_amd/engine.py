"""ctypes binding of libnxz_engine.so (include/nxz_engine.h).

Fails loudly when the shared library is missing or no gfx950 device is present: there is
no CPU fallback on the product path.
"""
import ctypes as C
import errno
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))

FC_COMPRESS_FHT = 0x00
FC_COMPRESS_DHT = 0x02
FC_COMPRESS_FHT_COUNT = 0x04
FC_COMPRESS_DHT_COUNT = 0x06
FC_COMPRESS_RESUME_FHT = 0x08
FC_COMPRESS_RESUME_DHT_COUNT = 0x0E
FC_COMPRESS_DHTGEN = 0x22           # additive: the engine builds the job's own table (include/nxz_engine.h)
FC_COMPRESS_DHTGEN_COUNT = 0x26
FC_COMPRESS_RESUME_DHTGEN = 0x2A
FC_DECOMPRESS = 0x10
FC_DECOMPRESS_RESUME = 0x14
FC_WRAP = 0x1E

# nxz_batch_job_t / nxz_batch_result_t / nxz_batch_dht_t
JOB_DTYPE = np.dtype([("src", "<u8"), ("dst", "<u8"), ("src_len", "<u4"), ("hist_len", "<u4"),
                      ("dst_cap", "<u4"), ("in_crc", "<u4"), ("in_adler", "<u4"), ("dht_index", "<u4"),
                      ("resume", "<u4"), ("reserved", "<u4")])
RESULT_DTYPE = np.dtype([("cc", "<u4"), ("tpbc", "<u4"), ("tebc", "<u4"), ("spbc", "<u4"),
                         ("crc", "<u4"), ("adler", "<u4"), ("subc", "<u4"), ("sfbt", "<u4")])
DHT_DTYPE = np.dtype([("dhtlen", "<u4"), ("dht", "u1", (292,))])
assert JOB_DTYPE.itemsize == 48 and RESULT_DTYPE.itemsize == 32 and DHT_DTYPE.itemsize == 296

# framed streams (include/nxz_engine.h: nxz_batch_decompress_framed / nxz_batch_unpack_gzip)
FMT_ZLIB, FMT_GZIP, FMT_AUTO = 1, 2, 3
FMT_RAW = 0                         # nxz_batch_deflate_streams only: no framing
(FRAME_OK, FRAME_BAD_HEADER, FRAME_BAD_METHOD, FRAME_NEED_DICT, FRAME_BAD_HCRC, FRAME_TRUNCATED, FRAME_DEFLATE,
 FRAME_BAD_CHECK, FRAME_BAD_LENGTH) = range(9)
FRAME_DTYPE = np.dtype([("status", "<u4"), ("format", "<u4"), ("hdr_len", "<u4"), ("end", "<u4"), ("check", "<u4"),
                        ("isize", "<u4"), ("mtime", "<u4"), ("dictid", "<u4"), ("extra_off", "<u4"), ("extra_len", "<u4"),
                        ("name_off", "<u4"), ("comment_off", "<u4"), ("flg", "u1"), ("xfl", "u1"), ("os", "u1"), ("cinfo", "u1")])
assert FRAME_DTYPE.itemsize == 52

# one stream per device buffer (include/nxz_engine.h: nxz_batch_deflate_streams)
STREAM_JOB_DTYPE = np.dtype([("src", "<u8"), ("dst", "<u8"), ("src_len", "<u8"), ("dst_cap", "<u8")])
STREAM_RESULT_DTYPE = np.dtype([("cc", "<u4"), ("blocks", "<u4"), ("out_len", "<u8"), ("crc", "<u4"), ("adler", "<u4"),
                                ("stored", "<u4"), ("reserved", "<u4")])
assert STREAM_JOB_DTYPE.itemsize == 32 and STREAM_RESULT_DTYPE.itemsize == 32
# a stream written in parts (include/nxz_engine.h: nxz_batch_deflate_streams_part)
PART_FIRST, PART_LAST = 1, 2
STREAM_PART_JOB_DTYPE = np.dtype([("src", "<u8"), ("dst", "<u8"), ("src_len", "<u8"), ("dst_cap", "<u8"), ("prev", "<u8"), ("prev_len", "<u4"),
                                  ("flags", "<u4")])
STREAM_CARRY_DTYPE = np.dtype([("crc", "<u4"), ("adler", "<u4"), ("total_in", "<u8"), ("total_out", "<u8"), ("parts", "<u4"), ("status", "<u4")])
assert STREAM_PART_JOB_DTYPE.itemsize == 48 and STREAM_CARRY_DTYPE.itemsize == 32
# a stream read in parts (include/nxz_engine.h: nxz_batch_inflate_streams_part)
INFLATE_PART_TAIL = 288
INFLATE_PHASE_HEADER, INFLATE_PHASE_BODY, INFLATE_PHASE_TRAILER, INFLATE_PHASE_DONE, INFLATE_PHASE_FAILED = range(5)
INFLATE_PART_MORE, INFLATE_PART_DONE, INFLATE_PART_DST_FULL, INFLATE_PART_FAILED = range(4)
INFLATE_PART_JOB_DTYPE = np.dtype([("src", "<u8"), ("dst", "<u8"), ("prev", "<u8"), ("src_len", "<u4"), ("dst_cap", "<u4"), ("prev_len", "<u4"),
                                   ("flags", "<u4")])
INFLATE_CARRY_DTYPE = np.dtype([("phase", "<u4"), ("hpos", "<u4"), ("hleft", "<u4"), ("hcrc", "<u4"), ("frame", FRAME_DTYPE), ("hfirst", "<u4"),
                                ("sfbt", "<u4"), ("rem", "<u4"), ("dhtlen", "<u4"), ("subc", "<u4"), ("crc", "<u4"), ("adler", "<u4"),
                                ("parts", "<u4"), ("tail_len", "<u4"), ("reserved", "<u4", (2,)), ("total_in", "<u8"), ("total_out", "<u8"),
                                ("dht", "u1", (288,)), ("tail", "u1", (INFLATE_PART_TAIL,))])
INFLATE_PART_RESULT_DTYPE = np.dtype([("cc", "<u4"), ("status", "<u4"), ("in_used", "<u4"), ("out_len", "<u4"), ("crc", "<u4"), ("adler", "<u4"),
                                      ("reserved", "<u4", (2,))])
assert INFLATE_PART_JOB_DTYPE.itemsize == 40 and INFLATE_CARRY_DTYPE.itemsize == 704 and INFLATE_PART_RESULT_DTYPE.itemsize == 32

# the byte-shuffle filter (include/nxz_engine.h: nxz_batch_shuffle / nxz_batch_unshuffle)
SHUFFLE_ELEM_MAX = 256
SHUFFLE_JOB_DTYPE = np.dtype([("src", "<u8"), ("dst", "<u8"), ("len", "<u8"), ("elem", "<u4"), ("reserved", "<u4")])
assert SHUFFLE_JOB_DTYPE.itemsize == 32

# multi-member gzip jobs (include/nxz_engine.h: nxz_batch_gzip_members_size / _decode)
GZIP_MEMBER_DTYPE = np.dtype([("uoff", "<u8"), ("coff", "<u4"), ("clen", "<u4"), ("hdr_len", "<u4"), ("isize", "<u4"),
                              ("check", "<u4"), ("status", "<u4")])
GZIP_STREAM_DTYPE = np.dtype([("status", "<u4"), ("members", "<u4"), ("failed", "<u4"), ("consumed", "<u4"), ("out_len", "<u8"),
                              ("cc", "<u4"), ("reserved", "<u4")])
assert GZIP_MEMBER_DTYPE.itemsize == 32 and GZIP_STREAM_DTYPE.itemsize == 32
GZS_OK, GZS_MEMBER_FAILED, GZS_MORE_MEMBERS, GZS_TARGET_SPACE, GZS_INVALID = range(5)

# BGZF random access (include/nxz_engine.h: nxz_bgzf_index / nxz_bgzf_read_ranges)
RANGE_UOFF, RANGE_VOFF = 0, 1
RANGE_OK, RANGE_OUT_OF_BOUNDS, RANGE_BAD_VOFFSET, RANGE_DAMAGED, RANGE_BAD_STREAM = range(5)

# checkpoints inside raw / zlib / gzip streams (include/nxz_engine.h: nxz_batch_checkpoint_index / nxz_checkpoint_read_ranges)
CHECKPOINT_STREAM_DTYPE = np.dtype([("status", "<u4"), ("count", "<u4"), ("format", "<u4"), ("hdr_len", "<u4"), ("out_len", "<u8"),
                                    ("cc", "<u4"), ("frame_status", "<u4")])
assert CHECKPOINT_STREAM_DTYPE.itemsize == 32
CPS_OK, CPS_STREAM_FAILED, CPS_MORE, CPS_NO_OUTPUT, CPS_INVALID = range(5)
CHECKPOINT_WINDOW = 32768
# ... and inside blocks (nxz_batch_checkpoint_index_fine / nxz_checkpoint_read_ranges_fine): the state entry beside cbit / uoff
CHECKPOINT_STATE_DTYPE = np.dtype([("tbit", "<u8"), ("resume", "<u4"), ("dhtlen", "<u4")])
assert CHECKPOINT_STATE_DTYPE.itemsize == 16
CHECKPOINT_SPAN_MIN = 258
# ... and ranges across all the rows of a batch's index (nxz_batch_checkpoint_read_ranges): job, then [begin, end) of that stream
BATCH_RANGE_DTYPE = np.dtype([("job", "<u4"), ("reserved", "<u4"), ("begin", "<u8"), ("end", "<u8")])
assert BATCH_RANGE_DTYPE.itemsize == 24


# jobs[].reserved (include/nxz_engine.h)
JOB_SUSPEND_WHEN_FULL, JOB_NO_DICT = 1, 2
DICT_WINDOW = 32768


def dict_inflate_window(n):
    """bytes of an n-byte dictionary the decompress calls use: its last min(n, 32768)"""
    return min(n, DICT_WINDOW)


def dict_deflate_window(n):
    """... and the compress calls: its last min(n, 32768) & ~15 (a compress job then carries 65536 - that many bytes at most)"""
    return min(n, DICT_WINDOW) & ~15


def stream_dict_window(n, hist_max):
    """bytes of an n-byte dictionary that block 0 of a deflate_streams_dict stream sees: its last min(H, n) & ~15, H the window of
    hist_max (nxz_streams_dict.h) -- the `prev` rule of nxz_deflate_host_hist, not dict_deflate_window"""
    return min(min(hist_max & ~15, 32768), n) & ~15


class Dict:
    """nxz_dict_t: a preset dictionary on the device, shared by all jobs of the *_dict calls (Engine.dict_create)"""

    def __init__(self, eng, data):
        self.eng = eng
        self.length = len(data)
        h = C.c_void_p()
        eng._check(eng.L.nxz_dict_create(eng.ctx, bytes(data), len(data), C.byref(h)), "nxz_dict_create")
        self.handle = h
        self.id = eng.L.nxz_dict_id(h)
        self.inflate_window = dict_inflate_window(len(data))
        self.deflate_window = dict_deflate_window(len(data))

    def close(self):
        if self.handle:
            self.eng.L.nxz_dict_destroy(self.eng.ctx, self.handle)
            self.handle = None


class StreamResume(C.Structure):
    """nxz_stream_resume_t (include/nxz_engine.h): where a deflate stream stands between two calls"""
    _fields_ = [("sfbt", C.c_uint32), ("rem", C.c_uint32), ("dhtlen", C.c_uint32), ("final", C.c_uint32), ("dht", C.c_uint8 * 288)]


class EngineError(RuntimeError):
    pass


def lib_path():
    # NXZ_ENGINE_LIB: another build of the engine in this directory (A/B runs of kernel variants, tools/)
    return os.path.join(HERE, os.environ.get("NXZ_ENGINE_LIB", "libnxz_engine.so"))


_lib = None


def load_library():
    """dlopen the in-tree engine.  Raises EngineError (never falls back) when it is missing."""
    global _lib
    if _lib is None:
        # torch first: it ships its own libamdhip64.so.7; loading it before the engine makes both
        # share ONE HIP runtime (same soname), which is what lets them share streams and pointers
        import torch  # noqa: F401
        p = lib_path()
        if not os.path.exists(p):
            raise EngineError("%s not built: run `make -C power-gzip_amd/csrc` (or __graft_entry__.build())" % p)
        L = C.CDLL(p)
        L.nxz_ctx_create.restype = C.c_void_p
        L.nxz_ctx_create.argtypes = [C.c_int]
        L.nxz_ctx_destroy.argtypes = [C.c_void_p]
        L.nxz_last_error.restype = C.c_char_p
        L.nxz_engine_version.restype = C.c_char_p
        L.nxz_compress_bound.restype = C.c_size_t
        L.nxz_compress_bound.argtypes = [C.c_size_t]
        L.nxz_batch_compress.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t,
                                         C.c_void_p, C.c_void_p, C.c_void_p]
        L.nxz_batch_dhtgen.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
        L.nxz_batch_decompress.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]
        L.nxz_batch_wrap.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
        L.nxz_batch_pack_gzip.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]
        L.nxz_batch_pack_zlib.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]
        L.nxz_batch_decompress_framed.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]
        # one preset dictionary for all jobs of a batch
        L.nxz_dict_create.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t, C.POINTER(C.c_void_p)]
        L.nxz_dict_destroy.argtypes = [C.c_void_p, C.c_void_p]
        L.nxz_dict_id.restype = C.c_uint32
        L.nxz_dict_id.argtypes = [C.c_void_p]
        L.nxz_batch_compress_dict.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t,
                                              C.c_void_p, C.c_void_p, C.c_void_p]
        L.nxz_batch_decompress_dict.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
        L.nxz_batch_pack_zlib_dict.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p,
                                               C.c_void_p]
        L.nxz_batch_decompress_framed_dict.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p,
                                                       C.c_void_p]
        # output sizes without a decode
        L.nxz_batch_decompress_size.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
        L.nxz_batch_decompress_size_framed.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p,
                                                       C.c_void_p]
        # ... and their checksums and trailer checks
        L.nxz_batch_decompress_verify.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
        L.nxz_batch_decompress_verify_framed.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p,
                                                         C.c_void_p]
        L.nxz_deflate_stream_bound.restype = C.c_size_t
        L.nxz_batch_gzip_members_size.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
        L.nxz_batch_gzip_members_decode.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint32, C.c_void_p, C.c_void_p, C.c_size_t,
                                                    C.c_void_p]
        L.nxz_deflate_stream_bound.argtypes = [C.c_uint64, C.c_uint32, C.c_int]
        L.nxz_batch_deflate_streams.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_uint32, C.c_void_p, C.c_size_t, C.c_void_p,
                                                C.c_void_p]
        L.nxz_deflate_stream_bound_dict.restype = C.c_size_t
        L.nxz_batch_deflate_streams_indexed.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_uint32, C.c_void_p, C.c_size_t, C.c_void_p,
                                                        C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                        C.c_void_p]
        L.nxz_deflate_stream_bound_dict.argtypes = [C.c_uint64, C.c_uint32, C.c_int]
        L.nxz_batch_deflate_streams_dict.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_uint32, C.c_void_p, C.c_void_p, C.c_size_t,
                                                     C.c_void_p, C.c_void_p]
        L.nxz_deflate_stream_part_bound.restype = C.c_size_t
        L.nxz_deflate_stream_part_bound.argtypes = [C.c_uint64, C.c_uint32, C.c_int, C.c_uint32]
        L.nxz_batch_deflate_streams_part.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_uint32, C.c_void_p, C.c_size_t, C.c_void_p,
                                                     C.c_void_p, C.c_void_p]
        L.nxz_batch_inflate_streams_part.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]
        L.nxz_batch_shuffle.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
        L.nxz_batch_unshuffle.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
        L.nxz_shuffle_tile_elems.restype = C.c_uint32
        L.nxz_shuffle_tile_elems.argtypes = [C.c_uint32]
        L.nxz_batch_unpack_gzip.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p,
                                            C.c_size_t, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.c_void_p]
        L.nxz_bgzf_index.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_uint64), C.c_void_p]
        L.nxz_bgzf_read_ranges.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_void_p,
                                           C.c_size_t, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64),
                                           C.POINTER(C.c_uint64), C.c_void_p]
        L.nxz_batch_checkpoint_index.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p,
                                                 C.c_void_p, C.c_void_p, C.c_void_p]
        L.nxz_checkpoint_read_ranges.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p,
                                                 C.c_size_t, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64),
                                                 C.POINTER(C.c_uint64), C.c_void_p]
        L.nxz_batch_checkpoint_index_fine.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p,
                                                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.nxz_batch_checkpoint_build.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p,
                                                 C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.nxz_checkpoint_read_ranges_fine.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64,
                                                      C.c_void_p, C.c_size_t, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64),
                                                      C.POINTER(C.c_uint64), C.c_void_p]
        L.nxz_batch_checkpoint_read_ranges.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                       C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p,
                                                       C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.c_void_p]
        L.nxz_inflate_stream.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64,
                                         C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64),
                                         C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.c_void_p]
        L.nxz_inflate_stream_part.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64,
                                              C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64),
                                              C.POINTER(StreamResume), C.POINTER(C.c_uint32), C.c_void_p]
        L.nxz_deflate_host_bound.restype = C.c_size_t
        L.nxz_deflate_host_bound.argtypes = [C.c_size_t]
        L.nxz_deflate_host.argtypes = [C.c_void_p, C.c_int, C.c_char_p, C.c_size_t, C.c_int, C.c_void_p, C.c_size_t,
                                       C.POINTER(C.c_size_t), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
        L.nxz_ctx_sync.argtypes = [C.c_void_p, C.c_void_p]
        L.nxz_copy_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
        L.nxz_ctx_wg_reasons.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.nxz_ctx_wg_prof.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.nx_function_begin.argtypes = [C.c_int, C.c_int, C.c_void_p]
        L.nx_function_end.argtypes = [C.c_void_p]
        L.nxu_run_job.argtypes = [C.c_void_p, C.c_void_p]
        L.nx_wait_ticks.restype = C.c_uint64
        L.nx_wait_ticks.argtypes = [C.c_uint64, C.c_uint64, C.c_int]
        L.__crc32_vpmsum.restype = C.c_uint
        L.__crc32_vpmsum.argtypes = [C.c_uint, C.c_char_p, C.c_ulong]
        _lib = L
    return _lib


class Engine:
    """One engine context on a HIP device; batch calls take torch CUDA tensors."""

    def __init__(self, device=0):
        import torch
        self.torch = torch
        self.L = load_library()
        if not torch.cuda.is_available():
            raise EngineError("no GPU visible: the DEFLATE engine has no CPU fallback")
        self.device = device
        self.ctx = self.L.nxz_ctx_create(device)
        if not self.ctx:
            raise EngineError("nxz_ctx_create failed: %s" % self.L.nxz_last_error().decode())
        self.dev = torch.device("cuda", device)

    def close(self):
        if self.ctx:
            self.L.nxz_ctx_destroy(self.ctx)
            self.ctx = None

    # ---- helpers -------------------------------------------------------
    def stream_handle(self):
        return C.c_void_p(self.torch.cuda.current_stream(self.dev).cuda_stream)

    def to_device(self, arr: np.ndarray):
        t = self.torch.from_numpy(arr.view(np.uint8).reshape(-1).copy())
        return t.to(self.dev)

    def jobs_strided(self, src, src_stride, src_lens, dst, dst_stride, dst_cap, hist_len=0, dht_index=None,
                     in_crc=0, in_adler=1, resume=0):
        """Job array for n buffers laid out at fixed strides inside two device tensors."""
        n = len(src_lens)
        j = np.zeros(n, JOB_DTYPE)
        idx = np.arange(n, dtype=np.uint64)
        j["src"] = np.uint64(src.data_ptr()) + idx * np.uint64(src_stride)
        j["dst"] = np.uint64(dst.data_ptr()) + idx * np.uint64(dst_stride)
        j["src_len"] = src_lens
        j["hist_len"] = hist_len
        j["dst_cap"] = dst_cap
        j["in_crc"] = in_crc
        j["in_adler"] = in_adler
        j["resume"] = resume
        if dht_index is not None:
            j["dht_index"] = dht_index
        return self.to_device(j)

    def _check(self, rc, what):
        if rc != 0:
            raise EngineError("%s failed (%d): %s" % (what, rc, self.L.nxz_last_error().decode()))

    # ---- batched entry points (asynchronous on torch's current stream) --
    def compress(self, fc, jobs, n, results=None, dht=None, ntables=0, counts=None):
        t = self.torch
        if results is None:
            results = t.empty(n * RESULT_DTYPE.itemsize, dtype=t.uint8, device=self.dev)
        if (fc & 0x4) and counts is None:
            counts = t.empty(n * 316, dtype=t.int32, device=self.dev)
        rc = self.L.nxz_batch_compress(self.ctx, fc, jobs.data_ptr(), n,
                                       dht.data_ptr() if dht is not None else None, ntables,
                                       results.data_ptr(), counts.data_ptr() if counts is not None else None,
                                       self.stream_handle())
        self._check(rc, "nxz_batch_compress")
        return results, counts

    def dhtgen(self, counts, n, tables=None):
        """device dhtgen: counts = int32/uint32 tensor [n * 316] -> uint8 tensor of n nxz_batch_dht_t"""
        t = self.torch
        if tables is None:
            tables = t.zeros(n * DHT_DTYPE.itemsize, dtype=t.uint8, device=self.dev)
        self._check(self.L.nxz_batch_dhtgen(self.ctx, counts.data_ptr(), n, tables.data_ptr(), self.stream_handle()),
                    "nxz_batch_dhtgen")
        return tables

    def decompress(self, jobs, n, results=None, dht_io=None):
        t = self.torch
        if results is None:
            results = t.empty(n * RESULT_DTYPE.itemsize, dtype=t.uint8, device=self.dev)
        rc = self.L.nxz_batch_decompress(self.ctx, jobs.data_ptr(), n, results.data_ptr(),
                                         dht_io.data_ptr() if dht_io is not None else None, self.stream_handle())
        self._check(rc, "nxz_batch_decompress")
        return results

    def decompress_framed(self, fmt, jobs, n, results=None, frames=None):
        """zlib / gzip streams (FMT_ZLIB / FMT_GZIP / FMT_AUTO), nxz_batch_decompress_framed.  Returns (results, frames),
        device tensors of n RESULT_DTYPE / FRAME_DTYPE records."""
        t = self.torch
        if results is None:
            results = t.empty(n * RESULT_DTYPE.itemsize, dtype=t.uint8, device=self.dev)
        if frames is None:
            frames = t.empty(n * FRAME_DTYPE.itemsize, dtype=t.uint8, device=self.dev)
        rc = self.L.nxz_batch_decompress_framed(self.ctx, fmt, jobs.data_ptr(), n, results.data_ptr(), frames.data_ptr(),
                                                self.stream_handle())
        self._check(rc, "nxz_batch_decompress_framed")
        return results, frames

    # ---- one preset dictionary for all jobs (zlib's deflateSetDictionary / inflateSetDictionary) ----
    def dict_create(self, data):
        """bytes -> Dict (nxz_dict_create); close() it when no call that uses it is still running"""
        return Dict(self, data)

    def compress_dict(self, fc, d, jobs, n, results=None, dht=None, ntables=0, counts=None):
        """nxz_batch_compress_dict: jobs[].src is the source alone, the dictionary's deflate window is every job's history"""
        t = self.torch
        if results is None:
            results = t.empty(n * RESULT_DTYPE.itemsize, dtype=t.uint8, device=self.dev)
        if (fc & 0x4) and counts is None:
            counts = t.empty(n * 316, dtype=t.int32, device=self.dev)
        rc = self.L.nxz_batch_compress_dict(self.ctx, fc, d.handle, jobs.data_ptr(), n,
                                            dht.data_ptr() if dht is not None else None, ntables,
                                            results.data_ptr(), counts.data_ptr() if counts is not None else None,
                                            self.stream_handle())
        self._check(rc, "nxz_batch_compress_dict")
        return results, counts

    def decompress_dict(self, d, jobs, n, results=None):
        """nxz_batch_decompress_dict: raw deflate streams that may refer to the dictionary's inflate window"""
        t = self.torch
        if results is None:
            results = t.empty(n * RESULT_DTYPE.itemsize, dtype=t.uint8, device=self.dev)
        self._check(self.L.nxz_batch_decompress_dict(self.ctx, d.handle, jobs.data_ptr(), n, results.data_ptr(), self.stream_handle()),
                    "nxz_batch_decompress_dict")
        return results

    def pack_zlib_dict(self, level, d, jobs, results, n, packed, offsets=None):
        """zlib streams with FDICT / DICTID from a compress_dict batch, nxz_batch_pack_zlib_dict.  Returns the offsets."""
        t = self.torch
        if offsets is None:
            offsets = t.empty(n + 1, dtype=t.int64, device=self.dev)
        self._check(self.L.nxz_batch_pack_zlib_dict(self.ctx, level, d.handle, jobs.data_ptr(), results.data_ptr(), n, offsets.data_ptr(),
                                                    packed.data_ptr(), self.stream_handle()), "nxz_batch_pack_zlib_dict")
        return offsets

    def decompress_framed_dict(self, fmt, d, jobs, n, results=None, frames=None):
        """nxz_batch_decompress_framed_dict: as decompress_framed; zlib streams that name the dictionary are decoded with it"""
        t = self.torch
        if results is None:
            results = t.empty(n * RESULT_DTYPE.itemsize, dtype=t.uint8, device=self.dev)
        if frames is None:
            frames = t.empty(n * FRAME_DTYPE.itemsize, dtype=t.uint8, device=self.dev)
        rc = self.L.nxz_batch_decompress_framed_dict(self.ctx, fmt, d.handle, jobs.data_ptr(), n, results.data_ptr(), frames.data_ptr(),
                                                     self.stream_handle())
        self._check(rc, "nxz_batch_decompress_framed_dict")
        return results, frames

    # ---- output sizes: what the streams would produce, nothing decoded, dst never touched ----
    def decompress_size(self, jobs, n, results=None):
        """nxz_batch_decompress_size: results[i] as decompress() would report for a target of jobs[i].dst_cap bytes (0xffffffff: no
        limit), crc = adler = 0.  jobs[i].dst may be 0; hist_len only says how far a distance may reach."""
        t = self.torch
        if results is None:
            results = t.empty(n * RESULT_DTYPE.itemsize, dtype=t.uint8, device=self.dev)
        self._check(self.L.nxz_batch_decompress_size(self.ctx, jobs.data_ptr(), n, results.data_ptr(), self.stream_handle()),
                    "nxz_batch_decompress_size")
        return results

    def decompress_size_framed(self, fmt, jobs, n, d=None, results=None, frames=None):
        """nxz_batch_decompress_size_framed: as decompress_framed / decompress_framed_dict (d: a Dict or None) without the decode;
        FRAME_BAD_CHECK cannot occur.  Returns (results, frames)."""
        t = self.torch
        if results is None:
            results = t.empty(n * RESULT_DTYPE.itemsize, dtype=t.uint8, device=self.dev)
        if frames is None:
            frames = t.empty(n * FRAME_DTYPE.itemsize, dtype=t.uint8, device=self.dev)
        rc = self.L.nxz_batch_decompress_size_framed(self.ctx, fmt, d.handle if d is not None else None, jobs.data_ptr(), n,
                                                     results.data_ptr(), frames.data_ptr(), self.stream_handle())
        self._check(rc, "nxz_batch_decompress_size_framed")
        return results, frames

    # ---- verify: the same walk with the output's checksums, dst never touched ----
    def decompress_verify(self, jobs, n, results=None):
        """nxz_batch_decompress_verify: decompress_size's record with crc and adler of the bytes the stream makes, continued from
        in_crc / in_adler.  jobs[i].dst may be 0; the hist_len bytes at src are read as the window."""
        t = self.torch
        if results is None:
            results = t.empty(n * RESULT_DTYPE.itemsize, dtype=t.uint8, device=self.dev)
        self._check(self.L.nxz_batch_decompress_verify(self.ctx, jobs.data_ptr(), n, results.data_ptr(), self.stream_handle()),
                    "nxz_batch_decompress_verify")
        return results

    def decompress_verify_framed(self, fmt, jobs, n, d=None, results=None, frames=None):
        """nxz_batch_decompress_verify_framed: what decompress_framed / decompress_framed_dict (d: a Dict or None) reports, FRAME_BAD_CHECK
        included, without a target.  Returns (results, frames)."""
        t = self.torch
        if results is None:
            results = t.empty(n * RESULT_DTYPE.itemsize, dtype=t.uint8, device=self.dev)
        if frames is None:
            frames = t.empty(n * FRAME_DTYPE.itemsize, dtype=t.uint8, device=self.dev)
        rc = self.L.nxz_batch_decompress_verify_framed(self.ctx, fmt, d.handle if d is not None else None, jobs.data_ptr(), n,
                                                       results.data_ptr(), frames.data_ptr(), self.stream_handle())
        self._check(rc, "nxz_batch_decompress_verify_framed")
        return results, frames

    # ---- multi-member gzip jobs: the member index, then every stored member decoded as one framed batch ----
    def gzip_members_size(self, jobs, n, member_cap, members=None, streams=None):
        """nxz_batch_gzip_members_size: jobs whose src is a series of gzip members.  Returns (members, streams), uint8 device
        tensors of n * member_cap GZIP_MEMBER_DTYPE and n GZIP_STREAM_DTYPE records; dst is not touched."""
        t = self.torch
        if members is None:
            members = t.empty(n * member_cap * GZIP_MEMBER_DTYPE.itemsize, dtype=t.uint8, device=self.dev)
        if streams is None:
            streams = t.empty(n * GZIP_STREAM_DTYPE.itemsize, dtype=t.uint8, device=self.dev)
        self._check(self.L.nxz_batch_gzip_members_size(self.ctx, jobs.data_ptr(), n, member_cap, members.data_ptr(), streams.data_ptr(),
                                                       self.stream_handle()), "nxz_batch_gzip_members_size")
        return members, streams

    def gzip_members_decode(self, jobs, n, member_cap, members, streams, total_members=None):
        """nxz_batch_gzip_members_decode on what gzip_members_size returned (updated in place).  total_members: an upper bound of
        the members to decode, n * member_cap when None."""
        total = n * member_cap if total_members is None else total_members
        self._check(self.L.nxz_batch_gzip_members_decode(self.ctx, jobs.data_ptr(), n, member_cap, members.data_ptr(), streams.data_ptr(),
                                                         total, self.stream_handle()), "nxz_batch_gzip_members_decode")
        return members, streams

    # ---- one stream per device buffer: buffers of any length, each as one raw / zlib / gzip stream ----
    def deflate_stream_bound(self, src_len, hist_max=0, fmt=FMT_ZLIB):
        """nxz_deflate_stream_bound: the dst_cap a buffer of src_len bytes needs"""
        return self.L.nxz_deflate_stream_bound(src_len, hist_max, fmt)

    def deflate_stream_jobs(self, fc, fmt, jobs, results=None, hist_max=0, level=-1):
        """nxz_batch_deflate_streams on a HOST array of STREAM_JOB_DTYPE records (device addresses).  Returns (rc, results): rc 0 /
        -errno, results a uint8 device tensor of len(jobs) STREAM_RESULT_DTYPE records.  Asynchronous on torch's current stream."""
        t = self.torch
        jobs = np.ascontiguousarray(jobs, STREAM_JOB_DTYPE)
        n = len(jobs)
        if results is None:
            results = t.empty(max(n, 1) * STREAM_RESULT_DTYPE.itemsize, dtype=t.uint8, device=self.dev)
        rc = self.L.nxz_batch_deflate_streams(self.ctx, fc, fmt, level, hist_max, jobs.ctypes.data if n else None, n, results.data_ptr(),
                                              self.stream_handle())
        return rc, results

    def deflate_stream_part_bound(self, src_len, hist_max=0, fmt=FMT_ZLIB, flags=PART_FIRST | PART_LAST):
        """nxz_deflate_stream_part_bound: the dst_cap a part of src_len bytes needs"""
        return self.L.nxz_deflate_stream_part_bound(src_len, hist_max, fmt, flags)

    def deflate_stream_parts(self, fc, fmt, jobs, carry, results=None, hist_max=0, level=-1):
        """nxz_batch_deflate_streams_part on a HOST array of STREAM_PART_JOB_DTYPE records (device addresses): a part of a stream each.
        carry: a uint8 device tensor of len(jobs) STREAM_CARRY_DTYPE records, read and written by the device (None is passed on as
        NULL, which the call refuses); results_to_host(carry, STREAM_CARRY_DTYPE) reads it.  Returns (rc, results) as
        deflate_stream_jobs.  Asynchronous on torch's current stream: the next part may be queued without a wait in between."""
        t = self.torch
        jobs = np.ascontiguousarray(jobs, STREAM_PART_JOB_DTYPE)
        n = len(jobs)
        if results is None:
            results = t.empty(max(n, 1) * STREAM_RESULT_DTYPE.itemsize, dtype=t.uint8, device=self.dev)
        rc = self.L.nxz_batch_deflate_streams_part(self.ctx, fc, fmt, level, hist_max, jobs.ctypes.data if n else None, n,
                                                   carry.data_ptr() if carry is not None else None, results.data_ptr(), self.stream_handle())
        return rc, results

    def inflate_stream_parts(self, fmt, jobs, carry, results=None):
        """nxz_batch_inflate_streams_part on a HOST array of INFLATE_PART_JOB_DTYPE records (device addresses): a part of a stream each.
        carry: a uint8 device tensor of len(jobs) INFLATE_CARRY_DTYPE records, read and written by the device (None is passed on as
        NULL, which the call refuses); results_to_host(carry, INFLATE_CARRY_DTYPE) reads it.  Returns (rc, results): rc 0 / -errno,
        results a uint8 device tensor of len(jobs) INFLATE_PART_RESULT_DTYPE records.  Asynchronous on torch's current stream: the
        next part may be queued without a wait in between."""
        t = self.torch
        jobs = np.ascontiguousarray(jobs, INFLATE_PART_JOB_DTYPE)
        n = len(jobs)
        if results is None:
            results = t.empty(max(n, 1) * INFLATE_PART_RESULT_DTYPE.itemsize, dtype=t.uint8, device=self.dev)
        rc = self.L.nxz_batch_inflate_streams_part(self.ctx, fmt, jobs.ctypes.data if n else None, n,
                                                   carry.data_ptr() if carry is not None else None, results.data_ptr(), self.stream_handle())
        return rc, results

    def deflate_streams(self, fc, fmt, bufs, hist_max=0, level=-1):
        """bufs: uint8 device tensors (16-byte aligned, any length) -> one stream each (FMT_RAW / FMT_ZLIB / FMT_GZIP).  Returns
        (out, offsets, results): stream i stands at out[offsets[i]:] (a uint8 device tensor with room for every stream's bound),
        results[i].out_len bytes long; results as deflate_stream_jobs.  Asynchronous: results_to_host(results, STREAM_RESULT_DTYPE)."""
        return self._deflate_streams(fc, fmt, None, bufs, hist_max, level)

    # ---- ... with the streams' checkpoint index written on the way ----
    def deflate_stream_jobs_indexed(self, fc, fmt, jobs, span, cp_cap, windows=True, index_jobs=True, results=None, hist_max=0, level=-1,
                                    cbit=None, uoff=None, streams=None):
        """nxz_batch_deflate_streams_indexed: deflate_stream_jobs that also writes the checkpoint index of every stream, in the shapes
        checkpoint_read_ranges_batch takes.  Returns (rc, results, cbit, uoff, windows, streams, index_jobs): cbit / uoff int64
        device tensors of shape (n, cp_cap + 1); windows a uint8 device tensor of shape (n, cp_cap, 32768) (True, or a tensor to
        write to; False / None: positions only, None returned); streams a uint8 device tensor of n CHECKPOINT_STREAM_DTYPE records;
        index_jobs a uint8 device tensor of n JOB_DTYPE records, the reader's jobs (True, or a tensor; False / None: none).  Any
        of cbit, uoff, streams may be passed as a tensor to write to, or as False for NULL (which the call refuses).
        Asynchronous on torch's current stream."""
        t = self.torch
        jobs = np.ascontiguousarray(jobs, STREAM_JOB_DTYPE)
        n = len(jobs)
        if results is None:
            results = t.empty(max(n, 1) * STREAM_RESULT_DTYPE.itemsize, dtype=t.uint8, device=self.dev)
        if cbit is None:
            cbit = t.zeros((max(n, 1), cp_cap + 1), dtype=t.int64, device=self.dev)
        if uoff is None:
            uoff = t.zeros((max(n, 1), cp_cap + 1), dtype=t.int64, device=self.dev)
        if windows is True:
            windows = t.zeros((max(n, 1), cp_cap, CHECKPOINT_WINDOW), dtype=t.uint8, device=self.dev)
        if streams is None:
            streams = t.zeros(max(n, 1) * CHECKPOINT_STREAM_DTYPE.itemsize, dtype=t.uint8, device=self.dev)
        if index_jobs is True:
            index_jobs = t.zeros(max(n, 1) * JOB_DTYPE.itemsize, dtype=t.uint8, device=self.dev)

        def ptr(x):
            return x.data_ptr() if x is not None and x is not False else None
        rc = self.L.nxz_batch_deflate_streams_indexed(self.ctx, fc, fmt, level, hist_max, jobs.ctypes.data if n else None, n, results.data_ptr(),
                                                      span, cp_cap, ptr(cbit), ptr(uoff), ptr(windows), ptr(streams), ptr(index_jobs),
                                                      self.stream_handle())
        return rc, results, cbit, uoff, (windows if ptr(windows) else None), streams, (index_jobs if ptr(index_jobs) else None)

    def deflate_streams_indexed(self, fc, fmt, bufs, span, cp_cap, windows=True, hist_max=0, level=-1):
        """deflate_streams with the checkpoint index of every stream: a checkpoint at the first block header behind every `span`
        bytes of source, cp_cap of them stored per stream at most.  Returns (out, offsets, results, cbit, uoff, windows, streams,
        index_jobs): the first three as deflate_streams, the rest as deflate_stream_jobs_indexed -- what
        checkpoint_read_ranges_batch(index_jobs, len(bufs), cp_cap, cbit, uoff, None, windows, streams, ranges) takes, with no
        host step in between."""
        j, out, offsets = self._stream_jobs(None, bufs, hist_max, fmt)
        rc, results, cbit, uoff, windows, streams, index_jobs = self.deflate_stream_jobs_indexed(fc, fmt, j, span, cp_cap, windows=windows,
                                                                                                 hist_max=hist_max, level=level)
        self._check(rc, "nxz_batch_deflate_streams_indexed")
        return out, offsets, results, cbit, uoff, windows, streams, index_jobs

    # ---- ... with one preset dictionary as the window of every stream's first block ----
    def deflate_stream_bound_dict(self, src_len, hist_max=0, fmt=FMT_ZLIB):
        """nxz_deflate_stream_bound_dict: the dst_cap a buffer of src_len bytes needs (FMT_RAW / FMT_ZLIB; 0 for FMT_GZIP)"""
        return self.L.nxz_deflate_stream_bound_dict(src_len, hist_max, fmt)

    def deflate_stream_jobs_dict(self, fc, fmt, d, jobs, results=None, hist_max=0, level=-1):
        """nxz_batch_deflate_streams_dict: as deflate_stream_jobs; d: a Dict (None is passed on as NULL, which the call refuses)"""
        t = self.torch
        jobs = np.ascontiguousarray(jobs, STREAM_JOB_DTYPE)
        n = len(jobs)
        if results is None:
            results = t.empty(max(n, 1) * STREAM_RESULT_DTYPE.itemsize, dtype=t.uint8, device=self.dev)
        rc = self.L.nxz_batch_deflate_streams_dict(self.ctx, fc, fmt, level, hist_max, d.handle if d is not None else None,
                                                   jobs.ctypes.data if n else None, n, results.data_ptr(), self.stream_handle())
        return rc, results

    def deflate_streams_dict(self, fc, fmt, d, bufs, hist_max=0, level=-1):
        """as deflate_streams with the Dict d: block 0 of every stream sees the dictionary's last stream_dict_window(len, hist_max)
        bytes -- none at hist_max 0, where the stream only names the dictionary (FMT_RAW / FMT_ZLIB)"""
        return self._deflate_streams(fc, fmt, d, bufs, hist_max, level)

    def _stream_jobs(self, d, bufs, hist_max, fmt):
        """the STREAM_JOB_DTYPE records of bufs, their targets in one device tensor `out` at `offsets` -> (jobs, out, offsets)"""
        t = self.torch
        j = np.zeros(len(bufs), STREAM_JOB_DTYPE)
        bound = self.deflate_stream_bound if d is None else self.deflate_stream_bound_dict
        caps = [bound(b.numel(), hist_max, fmt) for b in bufs]
        offsets = np.zeros(len(bufs) + 1, np.int64)
        offsets[1:] = np.cumsum([(c + 15) & ~15 for c in caps])
        out = t.empty(max(int(offsets[-1]), 1), dtype=t.uint8, device=self.dev)
        for i, b in enumerate(bufs):
            assert b.dtype == t.uint8 and b.is_contiguous() and b.device == out.device
            j[i] = (b.data_ptr() if b.numel() else 0, out.data_ptr() + int(offsets[i]), b.numel(), caps[i])
        return j, out, offsets

    def _deflate_streams(self, fc, fmt, d, bufs, hist_max, level):
        j, out, offsets = self._stream_jobs(d, bufs, hist_max, fmt)
        if d is None:
            rc, results = self.deflate_stream_jobs(fc, fmt, j, hist_max=hist_max, level=level)
        else:
            rc, results = self.deflate_stream_jobs_dict(fc, fmt, d, j, hist_max=hist_max, level=level)
        self._check(rc, "nxz_batch_deflate_streams" if d is None else "nxz_batch_deflate_streams_dict")
        return out, offsets, results

    # ---- the byte-shuffle filter of HDF5 / numcodecs: byte j of every element, plane after plane ----
    def shuffle_tile_elems(self, elem):
        """nxz_shuffle_tile_elems: the elements a workgroup takes of a job with this element size"""
        return self.L.nxz_shuffle_tile_elems(elem)

    def shuffle(self, jobs, status=None, undo=False):
        """nxz_batch_shuffle (undo: nxz_batch_unshuffle) on a HOST array of SHUFFLE_JOB_DTYPE records (device addresses).  Returns
        (rc, status): rc 0 / -errno, status a uint32 device tensor of len(jobs) entries (False is passed on as NULL, which the call
        refuses).  Asynchronous on torch's current stream."""
        t = self.torch
        jobs = np.ascontiguousarray(jobs, SHUFFLE_JOB_DTYPE)
        n = len(jobs)
        if status is None:
            status = t.empty(max(n, 1), dtype=t.int32, device=self.dev)
        f = self.L.nxz_batch_unshuffle if undo else self.L.nxz_batch_shuffle
        rc = f(self.ctx, jobs.ctypes.data if n else None, n, status.data_ptr() if status is not False else None, self.stream_handle())
        return rc, status

    def shuffle_bufs(self, bufs, elem, undo=False):
        """bufs: uint8 device tensors of any length and alignment -> their shuffled (undo: unshuffled) forms with element size
        `elem`.  Returns (out, offsets, status): buffer i's result is out[offsets[i]:offsets[i] + bufs[i].numel()] (a uint8 device
        tensor, every result 16-byte aligned in it); status as shuffle.  Asynchronous."""
        t = self.torch
        offsets = np.zeros(len(bufs) + 1, np.int64)
        offsets[1:] = np.cumsum([(b.numel() + 15) & ~15 for b in bufs])
        out = t.empty(max(int(offsets[-1]), 1), dtype=t.uint8, device=self.dev)
        j = np.zeros(len(bufs), SHUFFLE_JOB_DTYPE)
        for i, b in enumerate(bufs):
            assert b.dtype == t.uint8 and b.is_contiguous() and b.device == out.device
            j[i] = (b.data_ptr() if b.numel() else 0, out.data_ptr() + int(offsets[i]), b.numel(), elem, 0)
        rc, status = self.shuffle(j, undo=undo)
        self._check(rc, "nxz_batch_unshuffle" if undo else "nxz_batch_shuffle")
        return out, offsets, status

    def frames_to_host(self, frames):
        self.torch.cuda.synchronize(self.dev)
        return frames.cpu().numpy().view(FRAME_DTYPE)

    def unpack_gzip(self, packed, length, dst, max_members, offsets=None, frames=None, results=None):
        """a BGZF image (uint8 device tensor, `length` bytes from its start) -> dst (uint8 device tensor), nxz_batch_unpack_gzip.
        Returns (rc, dict): rc 0 / -errno; dict holds members, consumed, out_len and the device tensors offsets, frames, results."""
        t = self.torch
        if offsets is None:
            offsets = t.empty(max_members + 1, dtype=t.int64, device=self.dev)
        if frames is None:
            frames = t.empty(max(1, max_members) * FRAME_DTYPE.itemsize, dtype=t.uint8, device=self.dev)
        if results is None:
            results = t.empty(max(1, max_members) * RESULT_DTYPE.itemsize, dtype=t.uint8, device=self.dev)
        members, consumed, out_len = C.c_uint64(), C.c_uint64(), C.c_uint64()
        rc = self.L.nxz_batch_unpack_gzip(self.ctx, packed.data_ptr(), length, dst.data_ptr(), dst.numel(), offsets.data_ptr(),
                                          frames.data_ptr(), results.data_ptr(), max_members, C.byref(members), C.byref(consumed),
                                          C.byref(out_len), self.stream_handle())
        return rc, {"members": members.value, "consumed": consumed.value, "out_len": out_len.value,
                    "offsets": offsets, "frames": frames, "results": results}

    def bgzf_index(self, packed, length, max_members):
        """the member index of a BGZF image (uint8 device tensor, `length` bytes from its start), nxz_bgzf_index.
        Returns (coff, uoff): int64 device tensors of members + 1 entries.  Raises EngineError on -EILSEQ / -E2BIG."""
        t = self.torch
        coff = t.empty(max_members + 1, dtype=t.int64, device=self.dev)
        uoff = t.empty(max_members + 1, dtype=t.int64, device=self.dev)
        members = C.c_uint64()
        rc = self.L.nxz_bgzf_index(self.ctx, packed.data_ptr(), length, coff.data_ptr(), uoff.data_ptr(), max_members, C.byref(members),
                                   self.stream_handle())
        self._check(rc, "nxz_bgzf_index")
        return coff[:members.value + 1], uoff[:members.value + 1]

    def bgzf_read_ranges(self, packed, length, coff, uoff, ranges, kind=RANGE_UOFF, dst=None):
        """ranges of a BGZF image through its index (coff / uoff: int64 device tensors, a slice of an index with `packed` holding
        the image from coff[0] on), nxz_bgzf_read_ranges.  ranges: (n, 2) int64 device tensor of [begin, end).  dst: uint8
        device tensor (None: room for the bytes asked for).  Returns (rc, offsets, status, out_len, decoded, dst): rc 0 /
        -errno, offsets (n + 1) int64 and status (n) int32 device tensors."""
        t = self.torch
        n = ranges.shape[0]
        offsets = t.zeros(n + 1, dtype=t.int64, device=self.dev)
        status = t.zeros(max(n, 1), dtype=t.int32, device=self.dev)
        out_len, decoded = C.c_uint64(), C.c_uint64()
        if dst is None:                  # (a first call for the size; the second call runs the map again)
            rc = self._read_ranges(packed, length, coff, uoff, ranges, kind, None, 0, offsets, status, out_len, decoded)
            dst = t.empty(max(out_len.value, 1), dtype=t.uint8, device=self.dev)
            if rc != -errno.E2BIG:
                return rc, offsets, status[:n], out_len.value, decoded.value, dst
        rc = self._read_ranges(packed, length, coff, uoff, ranges, kind, dst, dst.numel(), offsets, status, out_len, decoded)
        return rc, offsets, status[:n], out_len.value, decoded.value, dst

    def _read_ranges(self, packed, length, coff, uoff, ranges, kind, dst, cap, offsets, status, out_len, decoded):
        assert coff.numel() == uoff.numel() and ranges.is_contiguous() and ranges.dtype == self.torch.int64
        return self.L.nxz_bgzf_read_ranges(self.ctx, packed.data_ptr(), length, coff.data_ptr(), uoff.data_ptr(), coff.numel(), kind,
                                           ranges.data_ptr(), ranges.shape[0], dst.data_ptr() if dst is not None else None, cap, offsets.data_ptr(), status.data_ptr(),
                                           C.byref(out_len), C.byref(decoded), self.stream_handle())

    # ---- checkpoints: an index into raw / zlib / gzip streams, and ranges read through it ----
    def checkpoint_index(self, fmt, jobs, n, span, cp_cap, windows=False, cbit=None, uoff=None, streams=None):
        """nxz_batch_checkpoint_index (fmt: FMT_RAW / FMT_ZLIB / FMT_GZIP / FMT_AUTO).  Returns (rc, cbit, uoff, windows, streams):
        rc 0 / -errno; cbit / uoff int64 device tensors of shape (n, cp_cap + 1); windows a uint8 device tensor of shape
        (n, cp_cap, 32768) when asked for (True, or a tensor to write to; jobs[i].dst then holds the decoded output), else None;
        streams a uint8 device tensor of n CHECKPOINT_STREAM_DTYPE records.  Asynchronous on torch's current stream."""
        t = self.torch
        if cbit is None:
            cbit = t.zeros((max(n, 1), cp_cap + 1), dtype=t.int64, device=self.dev)
        if uoff is None:
            uoff = t.zeros((max(n, 1), cp_cap + 1), dtype=t.int64, device=self.dev)
        if windows is True:
            windows = t.zeros((max(n, 1), cp_cap, CHECKPOINT_WINDOW), dtype=t.uint8, device=self.dev)
        elif windows is False:
            windows = None
        if streams is None:
            streams = t.zeros(max(n, 1) * CHECKPOINT_STREAM_DTYPE.itemsize, dtype=t.uint8, device=self.dev)
        rc = self.L.nxz_batch_checkpoint_index(self.ctx, fmt, jobs.data_ptr() if jobs is not None else None, n, span, cp_cap, cbit.data_ptr(),
                                               uoff.data_ptr(), windows.data_ptr() if windows is not None else None, streams.data_ptr(),
                                               self.stream_handle())
        return rc, cbit, uoff, windows, streams

    def checkpoint_read_ranges(self, src, length, cbit, uoff, windows, ranges, dst=None):
        """ranges of ONE stream (src: uint8 device tensor, `length` bytes, framing included) through its checkpoint index: cbit / uoff
        int64 device tensors of count + 1 entries, windows a contiguous uint8 device tensor of count slots of 32768 bytes (None for
        an index of one segment), ranges an (n, 2) int64 device tensor of [begin, end) in uncompressed offsets.  Returns what
        bgzf_read_ranges returns: (rc, offsets, status, out_len, decoded, dst)."""
        t = self.torch
        n = ranges.shape[0]
        offsets = t.zeros(n + 1, dtype=t.int64, device=self.dev)
        status = t.zeros(max(n, 1), dtype=t.int32, device=self.dev)
        out_len, decoded = C.c_uint64(), C.c_uint64()
        assert cbit.numel() == uoff.numel() and cbit.is_contiguous() and uoff.is_contiguous() and ranges.is_contiguous() and ranges.dtype == t.int64
        assert windows is None or windows.is_contiguous()

        def call(d, cap):
            return self.L.nxz_checkpoint_read_ranges(self.ctx, src.data_ptr(), length, cbit.data_ptr(), uoff.data_ptr(),
                                                     windows.data_ptr() if windows is not None else None, cbit.numel(), ranges.data_ptr(), n,
                                                     d.data_ptr() if d is not None else None, cap, offsets.data_ptr(), status.data_ptr(),
                                                     C.byref(out_len), C.byref(decoded), self.stream_handle())
        if dst is None:                  # (a first call for the size; the second call runs the map again)
            rc = call(None, 0)
            dst = t.empty(max(out_len.value, 1), dtype=t.uint8, device=self.dev)
            if rc != -errno.E2BIG:
                return rc, offsets, status[:n], out_len.value, decoded.value, dst
        rc = call(dst, dst.numel())
        return rc, offsets, status[:n], out_len.value, decoded.value, dst

    def checkpoint_index_fine(self, fmt, jobs, n, span, cp_cap, windows=False, cbit=None, uoff=None, state=None, streams=None):
        """nxz_batch_checkpoint_index_fine: checkpoint_index with checkpoints inside blocks, every span (>= 258) bytes of output.
        Returns (rc, cbit, uoff, state, windows, streams): state a uint8 device tensor of shape (n, (cp_cap + 1) * 16) that holds
        CHECKPOINT_STATE_DTYPE records beside cbit / uoff; the others as there."""
        t = self.torch
        if cbit is None:
            cbit = t.zeros((max(n, 1), cp_cap + 1), dtype=t.int64, device=self.dev)
        if uoff is None:
            uoff = t.zeros((max(n, 1), cp_cap + 1), dtype=t.int64, device=self.dev)
        if state is None:
            state = t.zeros((max(n, 1), (cp_cap + 1) * CHECKPOINT_STATE_DTYPE.itemsize), dtype=t.uint8, device=self.dev)
        if windows is True:
            windows = t.zeros((max(n, 1), cp_cap, CHECKPOINT_WINDOW), dtype=t.uint8, device=self.dev)
        elif windows is False:
            windows = None
        if streams is None:
            streams = t.zeros(max(n, 1) * CHECKPOINT_STREAM_DTYPE.itemsize, dtype=t.uint8, device=self.dev)
        rc = self.L.nxz_batch_checkpoint_index_fine(self.ctx, fmt, jobs.data_ptr() if jobs is not None else None, n, span, cp_cap, cbit.data_ptr(),
                                                    uoff.data_ptr(), state.data_ptr(), windows.data_ptr() if windows is not None else None,
                                                    streams.data_ptr(), self.stream_handle())
        return rc, cbit, uoff, state, windows, streams

    def checkpoint_build(self, fmt, jobs, n, span, cp_cap, state=True, cbit=None, uoff=None, windows=None, streams=None):
        """nxz_batch_checkpoint_build: the index AND its windows from the source alone, in one pass -- jobs[i].dst is never looked at.
        state True (or a tensor to write to): checkpoints inside blocks every span (>= 258) bytes, as checkpoint_index_fine;
        state None / False: at block headers only, as checkpoint_index.  Returns what checkpoint_index_fine returns:
        (rc, cbit, uoff, state, windows, streams), state None without states, windows always a tensor of shape (n, cp_cap, 32768)."""
        t = self.torch
        if cbit is None:
            cbit = t.zeros((max(n, 1), cp_cap + 1), dtype=t.int64, device=self.dev)
        if uoff is None:
            uoff = t.zeros((max(n, 1), cp_cap + 1), dtype=t.int64, device=self.dev)
        if state is True:
            state = t.zeros((max(n, 1), (cp_cap + 1) * CHECKPOINT_STATE_DTYPE.itemsize), dtype=t.uint8, device=self.dev)
        elif state is False:
            state = None
        if windows is None:
            windows = t.zeros((max(n, 1), cp_cap, CHECKPOINT_WINDOW), dtype=t.uint8, device=self.dev)
        if streams is None:
            streams = t.zeros(max(n, 1) * CHECKPOINT_STREAM_DTYPE.itemsize, dtype=t.uint8, device=self.dev)
        rc = self.L.nxz_batch_checkpoint_build(self.ctx, fmt, jobs.data_ptr() if jobs is not None else None, n, span, cp_cap, cbit.data_ptr(),
                                               uoff.data_ptr(), state.data_ptr() if state is not None else None, windows.data_ptr(),
                                               streams.data_ptr(), self.stream_handle())
        return rc, cbit, uoff, state, windows, streams

    def checkpoint_read_ranges_fine(self, src, length, cbit, uoff, state, windows, ranges, dst=None):
        """checkpoint_read_ranges through a fine index: state a contiguous uint8 device tensor of count + 1 CHECKPOINT_STATE_DTYPE
        records (one job's row of what checkpoint_index_fine returned).  Returns (rc, offsets, status, out_len, decoded, dst)."""
        t = self.torch
        n = ranges.shape[0]
        offsets = t.zeros(n + 1, dtype=t.int64, device=self.dev)
        status = t.zeros(max(n, 1), dtype=t.int32, device=self.dev)
        out_len, decoded = C.c_uint64(), C.c_uint64()
        assert cbit.numel() == uoff.numel() and cbit.is_contiguous() and uoff.is_contiguous() and ranges.is_contiguous() and ranges.dtype == t.int64
        assert state.is_contiguous() and state.dtype == t.uint8 and state.numel() == cbit.numel() * CHECKPOINT_STATE_DTYPE.itemsize
        assert windows is None or windows.is_contiguous()

        def call(d, cap):
            return self.L.nxz_checkpoint_read_ranges_fine(self.ctx, src.data_ptr(), length, cbit.data_ptr(), uoff.data_ptr(), state.data_ptr(),
                                                          windows.data_ptr() if windows is not None else None, cbit.numel(), ranges.data_ptr(), n,
                                                          d.data_ptr() if d is not None else None, cap, offsets.data_ptr(), status.data_ptr(),
                                                          C.byref(out_len), C.byref(decoded), self.stream_handle())
        if dst is None:                  # (a first call for the size; the second call runs the map again)
            rc = call(None, 0)
            dst = t.empty(max(out_len.value, 1), dtype=t.uint8, device=self.dev)
            if rc != -errno.E2BIG:
                return rc, offsets, status[:n], out_len.value, decoded.value, dst
        rc = call(dst, dst.numel())
        return rc, offsets, status[:n], out_len.value, decoded.value, dst

    def checkpoint_read_ranges_batch(self, jobs, n_jobs, cp_cap, cbit, uoff, state, windows, streams, ranges, dst=None, n=None):
        """nxz_batch_checkpoint_read_ranges: ranges across ALL the streams of an indexed batch in one call.  jobs: the device tensor
        of n_jobs JOB_DTYPE records the index call was given; cbit / uoff / state / windows / streams: what checkpoint_index,
        checkpoint_index_fine or checkpoint_build returned for them with the same cp_cap (state None: a coarse index); ranges: a
        contiguous uint8 device tensor of BATCH_RANGE_DTYPE records (n of them: all by default).  Any tensor may be None (the call
        then says -EINVAL).  Returns (rc, offsets, status, out_len, decoded, dst) as checkpoint_read_ranges does."""
        t = self.torch
        if n is None:
            n = ranges.numel() // BATCH_RANGE_DTYPE.itemsize
        offsets = t.zeros(n + 1, dtype=t.int64, device=self.dev)
        status = t.zeros(max(n, 1), dtype=t.int32, device=self.dev)
        out_len, decoded = C.c_uint64(), C.c_uint64()
        for x in (jobs, cbit, uoff, state, windows, streams, ranges):
            assert x is None or x.is_contiguous()

        def ptr(x):
            return x.data_ptr() if x is not None else None

        def call(d, cap):
            return self.L.nxz_batch_checkpoint_read_ranges(self.ctx, ptr(jobs), n_jobs, cp_cap, ptr(cbit), ptr(uoff), ptr(state), ptr(windows),
                                                           ptr(streams), ptr(ranges), n, ptr(d), cap, offsets.data_ptr(), status.data_ptr(),
                                                           C.byref(out_len), C.byref(decoded), self.stream_handle())
        if dst is None:                  # (a first call for the size; the second call runs the map again)
            rc = call(None, 0)
            dst = t.empty(max(out_len.value, 1), dtype=t.uint8, device=self.dev)
            if rc != -errno.E2BIG:
                return rc, offsets, status[:n], out_len.value, decoded.value, dst
        rc = call(dst, dst.numel())
        return rc, offsets, status[:n], out_len.value, decoded.value, dst

    def pack_gzip(self, jobs, results, n, packed, offsets=None):
        """BGZF members from a compress batch, nxz_batch_pack_gzip.  Returns the offsets (int64 device tensor, n + 1)."""
        t = self.torch
        if offsets is None:
            offsets = t.empty(n + 1, dtype=t.int64, device=self.dev)
        self._check(self.L.nxz_batch_pack_gzip(self.ctx, jobs.data_ptr(), results.data_ptr(), n, offsets.data_ptr(), packed.data_ptr(),
                                               self.stream_handle()), "nxz_batch_pack_gzip")
        return offsets

    def pack_zlib(self, level, jobs, results, n, packed, offsets=None):
        """zlib streams from a compress batch, nxz_batch_pack_zlib.  Returns the offsets (int64 device tensor, n + 1)."""
        t = self.torch
        if offsets is None:
            offsets = t.empty(n + 1, dtype=t.int64, device=self.dev)
        self._check(self.L.nxz_batch_pack_zlib(self.ctx, level, jobs.data_ptr(), results.data_ptr(), n, offsets.data_ptr(),
                                               packed.data_ptr(), self.stream_handle()), "nxz_batch_pack_zlib")
        return offsets

    def copy_device(self, dst, src):
        """dst <- src (uint8 device tensors of equal size, a multiple of 16 bytes) by the engine's 16-bytes-a-lane copy kernel"""
        self._check(self.L.nxz_copy_device(self.ctx, dst.data_ptr(), src.data_ptr(), src.numel(), self.stream_handle()), "nxz_copy_device")

    def wg_reasons(self):
        """of the last decompress batch that went a stream per workgroup: {"handed_back": n, reason: count}"""
        out = (C.c_uint32 * 16)()
        rc = self.L.nxz_ctx_wg_reasons(self.ctx, self.stream_handle(), out)
        if rc:
            return None
        names = ["", "job", "header", "stored", "dht", "tables", "rounds", "no_eob", "token", "space", "dist"]
        d = {names[i]: out[i] for i in range(1, 11) if out[i]}
        d["handed_back"] = out[15]
        return d

    def wg_prof(self):
        """NXZ_WG_PROF=1: one lane's cycles by phase, per stream, of the last batch that went a stream per workgroup"""
        out = (C.c_uint64 * 32)()
        if self.L.nxz_ctx_wg_prof(self.ctx, self.stream_handle(), out):
            return None
        names = ["load", "header", "dht", "tables", "first", "rounds", "write", "list", "match", "out"]
        ns = max(1, out[11])
        d = {names[i]: out[i] / ns for i in range(10)}
        d["total"] = sum(out[i] for i in range(10)) / ns
        d.update(nrounds=out[10] / max(1, out[12]), streams=out[11], blocks=out[12] / ns, pieces=out[13] / max(1, out[12]),
                 jump_rounds=out[14] / ns, jump_cycles=out[16] / ns, redone=out[17] / max(1, out[12]), redone_in_2=out[15] / max(1, out[12]), per_round=[round(out[18 + i] / ns) for i in range(6)], cnt_r3_6=[round(out[24 + i] / max(1, out[12]), 1) for i in range(4)])
        return d

    def inflate_stream(self, src, src_len, dst, first_bit=0, hist=None):
        """one long raw-deflate stream (uint8 device tensor) -> dst (uint8 device tensor), in parallel by
        block-boundary speculation.  Returns (rc, dict): rc 0 / -errno as nxz_inflate_stream."""
        out_len, end_bit = C.c_uint64(), C.c_uint64()
        crc, adler, pieces, rounds = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_uint32()
        rc = self.L.nxz_inflate_stream(self.ctx, src.data_ptr(), src_len, first_bit,
                                       hist.data_ptr() if hist is not None else None, hist.numel() if hist is not None else 0,
                                       dst.data_ptr(), dst.numel(), C.byref(out_len), C.byref(crc), C.byref(adler),
                                       C.byref(end_bit), C.byref(pieces), C.byref(rounds), self.stream_handle())
        return rc, {"out_len": out_len.value, "crc": crc.value, "adler": adler.value, "end_bit": end_bit.value,
                    "pieces": pieces.value, "rounds": rounds.value}

    def inflate_stream_part(self, src, src_len, dst, state=None, first_bit=0, hist=None):
        """a PART of a raw-deflate stream (uint8 device tensor) -> dst, nxz_inflate_stream_part.  `state`: None at a
        block header / the stream's start, else the StreamResume a previous call returned.  Returns (rc, dict);
        dict["state"] is where the stream stands at dict["end_bit"] (state.final: the final block ended there)."""
        st = state if state is not None else StreamResume()
        out_len, end_bit = C.c_uint64(), C.c_uint64()
        crc, adler, pieces = C.c_uint32(), C.c_uint32(), C.c_uint32()
        rc = self.L.nxz_inflate_stream_part(self.ctx, src.data_ptr(), src_len, first_bit,
                                            hist.data_ptr() if hist is not None else None, hist.numel() if hist is not None else 0,
                                            dst.data_ptr(), dst.numel(), C.byref(out_len), C.byref(crc), C.byref(adler),
                                            C.byref(end_bit), C.byref(st), C.byref(pieces), self.stream_handle())
        return rc, {"out_len": out_len.value, "crc": crc.value, "adler": adler.value, "end_bit": end_bit.value,
                    "pieces": pieces.value, "state": st}

    def deflate_host(self, data, fc=FC_COMPRESS_DHTGEN, final=True, cap=None):
        """a HOST buffer (bytes) -> one raw deflate stream (bytes), nxz_deflate_host.  Returns (rc, stream, crc, adler)."""
        bound = self.L.nxz_deflate_host_bound(len(data)) if cap is None else cap
        dst = C.create_string_buffer(max(bound, 1))
        n, crc, adler = C.c_size_t(), C.c_uint32(), C.c_uint32()
        rc = self.L.nxz_deflate_host(self.ctx, fc, data, len(data), 1 if final else 0, dst, bound, C.byref(n), C.byref(crc), C.byref(adler))
        return rc, dst.raw[:n.value] if rc == 0 else b"", crc.value, adler.value

    def wrap(self, jobs, n, results=None):
        t = self.torch
        if results is None:
            results = t.empty(n * RESULT_DTYPE.itemsize, dtype=t.uint8, device=self.dev)
        self._check(self.L.nxz_batch_wrap(self.ctx, jobs.data_ptr(), n, results.data_ptr(), self.stream_handle()),
                    "nxz_batch_wrap")
        return results

    def results_to_host(self, results, dtype=RESULT_DTYPE):
        self.torch.cuda.synchronize(self.dev)
        return results.cpu().numpy().view(dtype)
