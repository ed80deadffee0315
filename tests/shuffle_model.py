"""The byte-shuffle filter's rule (HDF5's H5Z_FILTER_SHUFFLE, numcodecs.Shuffle; include/nxz_engine.h: nxz_batch_shuffle) as numpy: the
N = len // elem whole elements are a matrix of N rows and elem columns, shuffled they are its transpose; the len % elem bytes behind
them stay where they are.  tests/test_shuffle_model_host.py pins this to byte strings written out by hand."""
import numpy as np


def shuffle(data, elem):
    a = np.frombuffer(bytes(data), np.uint8)
    n = len(a) // elem
    return a[:n * elem].reshape(n, elem).T.tobytes() + a[n * elem:].tobytes()


def unshuffle(data, elem):
    a = np.frombuffer(bytes(data), np.uint8)
    n = len(a) // elem
    return a[:n * elem].reshape(elem, n).T.tobytes() + a[n * elem:].tobytes()
