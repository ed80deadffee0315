"""power-gzip_amd: MI355X-native DEFLATE engine behind the libnxz engine boundary.

The product is csrc/ (HIP kernels + the C ABI of include/nxz_engine.h, built in-tree as
libnxz_engine.so).  This Python package is a thin ctypes view of that C ABI for tests and
bench.py; torch is used only for device memory and streams.
"""
from .engine import (Engine, EngineError, JOB_DTYPE, RESULT_DTYPE, DHT_DTYPE, lib_path,
                     FC_COMPRESS_FHT, FC_COMPRESS_FHT_COUNT, FC_COMPRESS_DHT, FC_COMPRESS_DHT_COUNT,
                     FC_COMPRESS_RESUME_FHT, FC_COMPRESS_RESUME_DHT_COUNT, FC_COMPRESS_DHTGEN,
                     FC_COMPRESS_DHTGEN_COUNT, FC_COMPRESS_RESUME_DHTGEN, FC_DECOMPRESS,
                     FC_DECOMPRESS_RESUME, FC_WRAP, FRAME_DTYPE, FMT_ZLIB, FMT_GZIP, FMT_AUTO, FRAME_OK,
                     FRAME_BAD_HEADER, FRAME_BAD_METHOD, FRAME_NEED_DICT, FRAME_BAD_HCRC, FRAME_TRUNCATED, FRAME_DEFLATE,
                     FRAME_BAD_CHECK, FRAME_BAD_LENGTH, RANGE_UOFF, RANGE_VOFF, RANGE_OK, RANGE_OUT_OF_BOUNDS,
                     RANGE_BAD_VOFFSET, RANGE_DAMAGED, Dict, JOB_SUSPEND_WHEN_FULL, JOB_NO_DICT, dict_inflate_window,
                     dict_deflate_window, stream_dict_window, GZIP_MEMBER_DTYPE, GZIP_STREAM_DTYPE, GZS_OK, GZS_MEMBER_FAILED, GZS_MORE_MEMBERS,
                     GZS_TARGET_SPACE, GZS_INVALID, CHECKPOINT_STREAM_DTYPE, CHECKPOINT_WINDOW, CHECKPOINT_STATE_DTYPE, CHECKPOINT_SPAN_MIN, CPS_OK, CPS_STREAM_FAILED, CPS_MORE,
                     CPS_NO_OUTPUT, CPS_INVALID, RANGE_BAD_STREAM, BATCH_RANGE_DTYPE)
