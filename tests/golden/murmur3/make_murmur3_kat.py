"""Known answers of MurmurHash3_x64_128 (Austin Appleby's public-domain smhasher code) for tests/minhash_ref.py:
murmur3_kat.npz holds one 64-byte message, and for seeds 0 and 42 and every length 0..40 of its prefixes the two
64-bit output words (h1, h2).

Generated once, not by any test: compile the smhasher file that scikit-learn ships (sklearn/utils/src/MurmurHash3.cpp
and MurmurHash3.h) next to the driver below and run

    python tests/golden/murmur3/make_murmur3_kat.py <dir holding MurmurHash3.cpp and MurmurHash3.h>

(The file lives in this subdirectory because every *.npz directly under tests/golden/ is taken for an anchor fixture.)
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

DRIVER = r"""
#include "MurmurHash3.h"
#include <cstdint>
#include <cstdio>
int main() {
    unsigned char buf[64];
    for (int i = 0; i < 64; ++i) buf[i] = (unsigned char)("ACGTNacgtn"[(i * 7 + 3) % 10] + (i % 5 == 4 ? 1 : 0));
    for (int i = 0; i < 64; ++i) std::printf("%02x", buf[i]);
    std::printf("\n");
    const uint32_t seeds[2] = {0u, 42u};
    for (uint32_t seed : seeds)
        for (int len = 0; len <= 40; ++len) {
            uint64_t out[2];
            MurmurHash3_x64_128(buf, len, seed, out);
            std::printf("%u %d %llu %llu\n", seed, len, (unsigned long long)out[0], (unsigned long long)out[1]);
        }
}
"""


def main(src_dir: str) -> None:
    with tempfile.TemporaryDirectory() as tmp:
        drv = os.path.join(tmp, "kat.cpp")
        with open(drv, "w") as f:
            f.write(DRIVER)
        exe = os.path.join(tmp, "kat")
        subprocess.run(["g++", "-O1", "-I", src_dir, "-o", exe, drv, os.path.join(src_dir, "MurmurHash3.cpp")], check=True)
        lines = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split("\n")
    msg = np.frombuffer(bytes.fromhex(lines[0]), np.uint8)
    rows = [ln.split() for ln in lines[1:] if ln.strip()]
    np.savez(os.path.join(os.path.dirname(os.path.abspath(__file__)), "murmur3_kat.npz"), message=msg,
             seed=np.array([int(r[0]) for r in rows], np.uint32), length=np.array([int(r[1]) for r in rows], np.int32),
             h1=np.array([int(r[2]) for r in rows], np.uint64), h2=np.array([int(r[3]) for r in rows], np.uint64))


if __name__ == "__main__":
    main(sys.argv[1])
