"""The entropy kernel's CRC-32 / Adler-32 arithmetic (power-gzip_amd/csrc/nxz_cksum_slices.h, the product code
itself), compiled for the host, run serially "as 256 lanes would" under AddressSanitizer and UBSan, against zlib:
every length round the slice / round / tile / block edges, histories in front of the source, seeds, and all-0xFF
data at 65536 bytes -- where an Adler partial sum that is reduced too late passes 2^32."""
import os
import struct
import subprocess

import cksum_grid

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cksum_slices_equal_zlib(tmp_path):
    exe = tmp_path / "cksum_slices_host"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize=alignment",
                    "-I", os.path.join(ROOT, "power-gzip_amd", "csrc"),
                    os.path.join(ROOT, "tests", "native", "cksum_slices_host.cpp"), "-o", str(exe)], check=True)
    cases = cksum_grid.cases()
    assert any(n == 65536 and buf == b"\xff" * 65536 for _, n, _, _, buf in cases)
    inp = tmp_path / "cases.bin"
    with open(inp, "wb") as f:
        f.write(struct.pack("<I", len(cases)))
        for h, n, in_crc, in_adler, buf in cases:
            f.write(struct.pack("<4I", h, n, in_crc, in_adler))
            f.write(buf)
    r = subprocess.run([str(exe), str(inp)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = r.stdout.split("\n")[:-1]
    assert len(lines) == len(cases)
    bad = []
    for c, line in zip(cases, lines):
        got = tuple(int(x, 16) for x in line.split())
        if got != cksum_grid.expected(c):
            bad.append((c[0], c[1], hex(c[2]), hex(c[3]), [hex(x) for x in got], [hex(x) for x in cksum_grid.expected(c)]))
    assert not bad, bad[:10]
