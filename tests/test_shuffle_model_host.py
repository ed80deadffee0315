"""tests/shuffle_model.py, the yardstick of tests/test_gpu_shuffle.py, against byte strings written out by hand (the rule of
include/nxz_engine.h: dst[j * N + i] = src[i * elem + j], the len % elem bytes behind the elements unchanged), and against itself in
both directions over random (len, elem)."""
import random

from shuffle_model import shuffle, unshuffle

H = bytes.fromhex


def test_elem_4_len_10():
    assert shuffle(bytes(range(10)), 4) == H("00 04 01 05 02 06 03 07 08 09")
    assert unshuffle(H("00 04 01 05 02 06 03 07 08 09"), 4) == bytes(range(10))


def test_elem_3_len_7():
    # two elements a0 a1 a2, b0 b1 b2 and one byte behind them
    assert shuffle(H("a0 a1 a2 b0 b1 b2 ee"), 3) == H("a0 b0 a1 b1 a2 b2 ee")
    assert unshuffle(H("a0 b0 a1 b1 a2 b2 ee"), 3) == H("a0 a1 a2 b0 b1 b2 ee")


def test_elem_2_three_elements():
    assert shuffle(H("11 22 33 44 55 66"), 2) == H("11 33 55 22 44 66")


def test_elem_1_is_a_copy():
    x = H("09 08 07 06 05")
    assert shuffle(x, 1) == x and unshuffle(x, 1) == x


def test_shorter_than_an_element_is_a_copy():
    x = H("01 02 03")
    assert shuffle(x, 4) == x and unshuffle(x, 4) == x
    assert shuffle(H("01 02 03 04 05 06 07"), 8) == H("01 02 03 04 05 06 07")


def test_one_element_is_a_copy():
    assert shuffle(H("01 02 03 04"), 4) == H("01 02 03 04")
    assert shuffle(H("01 02 03 04 05"), 4) == H("01 02 03 04 05")


def test_empty():
    for elem in (1, 2, 4, 255, 256):
        assert shuffle(b"", elem) == b"" and unshuffle(b"", elem) == b""


def test_the_two_directions_undo_each_other():
    rnd = random.Random(26)
    for _ in range(400):
        elem = rnd.choice([1, 2, 3, 4, 5, 6, 7, 8, 12, 16, 17, 31, 255, 256, rnd.randrange(1, 257)])
        n = rnd.choice([0, 1, elem - 1, elem, elem + 1, rnd.randrange(0, 5000)])
        x = rnd.randbytes(n)
        y = shuffle(x, elem)
        assert len(y) == n and unshuffle(y, elem) == x and shuffle(unshuffle(x, elem), elem) == x
        assert y[n - n % elem:] == x[n - n % elem:]
        assert sorted(y) == sorted(x)
