"""nxu_run_job on host buffers, on the GPU engine and on the CPU engine model (oracle/nxz_engine_model.c), for the tests
that compare the two."""
import ctypes as C
import importlib

import oracle_lib as O

crb = importlib.import_module("power-gzip_amd.crb")


def run_both(eng, handle, setup_kwargs, src_bufs_bytes, dst_sizes):
    """returns (gpu_job, gpu_dst_bytes, cpu_job, cpu_dst_bytes)"""
    res = []
    for which in ("gpu", "cpu"):
        j = crb.Job()
        srcs = [C.create_string_buffer(b, len(b)) for b in src_bufs_bytes]
        dsts = [C.create_string_buffer(n) for n in dst_sizes]
        j.setup(src_bufs=srcs, dst_bufs=dsts, **setup_kwargs)
        if which == "gpu":
            rc = eng.L.nxu_run_job(C.c_void_p(j.addr), C.byref(handle))
        else:
            rc = O.lib().nxo_run_job(C.c_void_p(j.addr))
        assert rc == 0 and j.valid == 1
        res.append((j, b"".join(d.raw for d in dsts)))
    return res[0][0], res[0][1], res[1][0], res[1][1]
