#!/usr/bin/env python3
"""Generate libdeflate_blocks.npz: raw DEFLATE streams written by libdeflate (the encoder of htslib built with libdeflate,
hence of many BGZF files), for the GPU inflate tests.  libdeflate need not exist where the tests run: they read only the
fixture.

    python tests/golden/inflate/make_libdeflate.py [--lib PATH/libdeflate.so] [--version X.Y]

Payloads are rebuilt from fixed seeds (rows of 1, 8, 9 and 17 bytes, runs, random bytes), in a small (<= 8 KB) and a
large size (65280 bytes, a BGZF block's payload); each is compressed at levels 0..12 with libdeflate_deflate_compress.
The fixture holds the compressed streams back to back (``bodies``, ``body_offsets``), each one's level, payload name and
ISIZE, the sha256 of every payload and the libdeflate version."""
import argparse
import ctypes
import ctypes.util
import hashlib
import os
import re

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def payloads():
    rng = np.random.default_rng(20240)
    out = {}
    for size, tag in ((6000, "small"), (65280, "large")):  # (65280: a BGZF writer's block payload)
        for w in (1, 8, 9, 17):
            base = rng.integers(0, 256, (48, w), dtype=np.uint8)
            rows = np.repeat(base, rng.integers(1, 40 if size < 10000 else 200, 48), axis=0)
            rows = np.concatenate([rows] * (size // rows.nbytes + 1))[:size // w]
            flip = rng.integers(0, len(rows), max(1, len(rows) // 50))
            rows[flip, 0] ^= 0x11
            out[f"rows{w}_{tag}"] = rows.tobytes()
        out[f"runs_{tag}"] = np.repeat(rng.integers(0, 5, size, dtype=np.uint8), rng.integers(1, 60, size))[:size].tobytes()
    out["random_small"] = rng.integers(0, 256, 4000, dtype=np.uint8).tobytes()
    return out


def version_of(lib_path):
    hdr = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(lib_path))), "include", "libdeflate.h")
    if os.path.exists(hdr):
        m = re.search(r'LIBDEFLATE_VERSION_STRING\s+"([^"]+)"', open(hdr).read())
        if m:
            return m.group(1)
    return "unknown"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=ctypes.util.find_library("deflate"))
    ap.add_argument("--version", default=None, help="the library's version (default: from its libdeflate.h)")
    ap.add_argument("--out", default=os.path.join(HERE, "libdeflate_blocks.npz"))
    a = ap.parse_args()
    lib = ctypes.CDLL(a.lib)
    lib.libdeflate_alloc_compressor.restype = ctypes.c_void_p
    lib.libdeflate_alloc_compressor.argtypes = [ctypes.c_int]
    lib.libdeflate_deflate_compress.restype = ctypes.c_size_t
    lib.libdeflate_deflate_compress.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p,
                                                ctypes.c_size_t]
    lib.libdeflate_free_compressor.argtypes = [ctypes.c_void_p]
    bodies, levels, names, isizes = [], [], [], []
    pays = payloads()
    for name, p in pays.items():
        for level in range(13):
            c = lib.libdeflate_alloc_compressor(level)
            assert c, f"level {level}"
            buf = ctypes.create_string_buffer(len(p) + 1024)
            n = lib.libdeflate_deflate_compress(c, p, len(p), buf, len(buf))
            lib.libdeflate_free_compressor(c)
            assert n > 0
            bodies.append(buf.raw[:n])
            levels.append(level)
            names.append(name)
            isizes.append(len(p))
    offs = np.concatenate([[0], np.cumsum([len(b) for b in bodies])]).astype(np.int64)
    np.savez_compressed(a.out, bodies=np.frombuffer(b"".join(bodies), np.uint8), body_offsets=offs,
                        level=np.array(levels, np.int32), payload=np.array(names), isize=np.array(isizes, np.int64),
                        payload_names=np.array(list(pays)),
                        payload_sha256=np.array([hashlib.sha256(p).hexdigest() for p in pays.values()]),
                        version=np.array(a.version or version_of(a.lib)))
    print(a.out, os.path.getsize(a.out), "bytes,", len(bodies), "streams")


if __name__ == "__main__":
    main()
