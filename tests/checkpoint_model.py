"""The checkpoint index of a raw / zlib / gzip stream as system zlib sees it (the model the device is held to in
tests/test_gpu_checkpoints.py, proven itself in tests/test_checkpoint_model_host.py).

The block headers come from inflate(..., Z_BLOCK) through ctypes: a return with data_type & 128 set and & 64 clear is a block
boundary at bit total_in * 8 - (data_type & 7) of the stream, with total_out bytes of output in front of it; with & 64 set it is
the end of the final block.  The first boundary (behind the framing's header; bit 0 of a raw stream, where zlib does not stop) is
checkpoint 0; the checkpoint rule of include/nxz_engine.h is applied in Python:
    a later header with u bytes of output in front of it is a checkpoint when u - uoff_of_last_checkpoint >= span.
resume() decodes one segment the way a reader of the index would, with zlib alone: inflatePrime for the bits of the first byte,
inflateSetDictionary for the window."""
import ctypes as C
import ctypes.util
import zlib

Z_BLOCK, Z_OK, Z_STREAM_END, Z_BUF_ERROR = 5, 0, 1, -5
WINDOW = 32768
FMT_RAW, FMT_ZLIB, FMT_GZIP = 0, 1, 2
WBITS = {FMT_RAW: -15, FMT_ZLIB: 15, FMT_GZIP: 31}


class ZStream(C.Structure):
    _fields_ = [("next_in", C.c_void_p), ("avail_in", C.c_uint), ("total_in", C.c_ulong),
                ("next_out", C.c_void_p), ("avail_out", C.c_uint), ("total_out", C.c_ulong),
                ("msg", C.c_char_p), ("state", C.c_void_p), ("zalloc", C.c_void_p), ("zfree", C.c_void_p),
                ("opaque", C.c_void_p), ("data_type", C.c_int), ("adler", C.c_ulong), ("reserved", C.c_ulong)]


_Z = None


def libz():
    global _Z
    if _Z is None:
        L = C.CDLL(ctypes.util.find_library("z") or "libz.so.1")
        L.zlibVersion.restype = C.c_char_p
        L.inflateInit2_.argtypes = [C.POINTER(ZStream), C.c_int, C.c_char_p, C.c_int]
        L.inflate.argtypes = [C.POINTER(ZStream), C.c_int]
        L.inflateEnd.argtypes = [C.POINTER(ZStream)]
        L.inflatePrime.argtypes = [C.POINTER(ZStream), C.c_int, C.c_int]
        L.inflateSetDictionary.argtypes = [C.POINTER(ZStream), C.c_char_p, C.c_uint]
        _Z = L
    return _Z


def _init(wbits):
    L = libz()
    zs = ZStream()
    rc = L.inflateInit2_(C.byref(zs), wbits, L.zlibVersion(), C.sizeof(ZStream))
    assert rc == Z_OK, rc
    return L, zs


def block_boundaries(stream, fmt):
    """-> (headers, end, plain): headers = [(bit, output bytes in front)] of every block header, end = (bit behind the final
    end-of-block code, out_len) or None when the stream fails or is cut short, plain = the bytes decoded.
    For a gzip stream: the first member."""
    L, zs = _init(WBITS[fmt])
    src = C.create_string_buffer(bytes(stream), len(stream))
    out = C.create_string_buffer(1 << 16)
    plain = bytearray()
    headers, end = ([(0, 0)] if fmt == FMT_RAW else []), None      # (a raw stream: zlib does not stop in front of the first header)
    zs.next_in = C.cast(src, C.c_void_p).value
    zs.avail_in = len(stream)
    while True:
        zs.next_out = C.cast(out, C.c_void_p).value
        zs.avail_out = len(out)
        before = (zs.avail_in, zs.total_out)
        rc = L.inflate(C.byref(zs), Z_BLOCK)
        plain += out.raw[:len(out) - zs.avail_out]
        if rc not in (Z_OK, Z_STREAM_END):
            break                                   # (a data error, or Z_BUF_ERROR: the source ran out)
        if rc == Z_OK and (zs.data_type & 128):
            bit = zs.total_in * 8 - (zs.data_type & 7)
            if zs.data_type & 64:
                end = (bit, zs.total_out)
            else:
                headers.append((bit, zs.total_out))
        if rc == Z_STREAM_END:
            break
        if rc == Z_OK and end is not None and fmt == FMT_RAW:
            break
        if (zs.avail_in, zs.total_out) == before and not (zs.data_type & 128):
            break                                   # (no progress: the source ran out)
    L.inflateEnd(C.byref(zs))
    return headers, end, bytes(plain)


def index(stream, fmt, span):
    """-> None for a stream that fails or does not reach the end of its final block, else a dict: cbit / uoff (count + 1 entries,
    the sentinel last), count, out_len, plain."""
    assert span >= 1
    headers, end, plain = block_boundaries(stream, fmt)
    if end is None or not headers:
        return None
    cbit, uoff = [], []
    for bit, u in headers:
        if not cbit or u - uoff[-1] >= span:
            cbit.append(bit)
            uoff.append(u)
    return {"cbit": cbit + [end[0]], "uoff": uoff + [end[1]], "count": len(cbit), "out_len": end[1], "plain": plain}


def segment(idx, k):
    """segment k of an index: (first source byte, end source byte, in_subc, window length, output bytes)"""
    c0, c1, u0, u1 = idx["cbit"][k], idx["cbit"][k + 1], idx["uoff"][k], idx["uoff"][k + 1]
    return c0 >> 3, (c1 + 7) >> 3, (8 - (c0 & 7)) & 7, min(u0, WINDOW), u1 - u0


def resume(stream, idx, k):
    """decodes segment k with zlib: a raw inflate primed with the upper in_subc bits of the segment's first byte, the window as
    its dictionary, fed the segment's source bytes and no more -> the bytes it makes"""
    b, e, in_subc, wlen, olen = segment(idx, k)
    L, zs = _init(-15)
    data = bytes(stream[b:e])
    if in_subc:
        assert L.inflatePrime(C.byref(zs), in_subc, data[0] >> (8 - in_subc)) == Z_OK
        data = data[1:]
    u0 = idx["uoff"][k]
    if wlen:
        assert L.inflateSetDictionary(C.byref(zs), idx["plain"][u0 - wlen:u0], wlen) == Z_OK
    src = C.create_string_buffer(data, len(data))
    out = C.create_string_buffer(max(olen, 1) + 64)
    zs.next_in = C.cast(src, C.c_void_p).value
    zs.avail_in = len(data)
    zs.next_out = C.cast(out, C.c_void_p).value
    zs.avail_out = len(out)
    rc = L.inflate(C.byref(zs), 0)
    n = zs.total_out
    L.inflateEnd(C.byref(zs))
    assert rc in (Z_OK, Z_STREAM_END, Z_BUF_ERROR), rc
    return out.raw[:n]


def deflate(data, fmt, level=6, mem_level=8, strategy=zlib.Z_DEFAULT_STRATEGY):
    c = zlib.compressobj(level, zlib.DEFLATED, WBITS[fmt], mem_level, strategy)
    return c.compress(data) + c.flush()
