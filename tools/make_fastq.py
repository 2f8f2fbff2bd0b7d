"""A synthetic four-line FASTQ file of a given size, for tools/place_rate.py and for trying `place` by hand.

    python tools/make_fastq.py OUT.fq [--mb 1024] [--read-len 150] [--seed 7]

Records of one fixed width: "@read" and ten digits, a read of --read-len i.i.d. uniform bases, "+", and as many 'I'."""
import argparse

import numpy as np


def fastq_records(nrec: int, read_len: int = 150, seed: int = 7, seqs=None) -> np.ndarray:
    """(nrec, record bytes) uint8: one record per row; ``seqs`` (nrec, read_len) uint8 ASCII replaces the random reads"""
    rng = np.random.default_rng(seed)
    width = 16 + read_len + 1 + 2 + read_len + 1
    rec = np.empty((nrec, width), np.uint8)
    rec[:, :5] = np.frombuffer(b"@read", np.uint8)
    idx = np.arange(nrec, dtype=np.int64)
    for j in range(10):
        rec[:, 14 - j] = (idx // 10 ** j % 10 + 48).astype(np.uint8)
    rec[:, 15] = 10
    if seqs is None:
        seqs = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, (nrec, read_len), dtype=np.uint8)]
    rec[:, 16:16 + read_len] = seqs
    at = 16 + read_len
    rec[:, at:at + 3] = np.frombuffer(b"\n+\n", np.uint8)
    rec[:, at + 3:at + 3 + read_len] = ord("I")
    rec[:, -1] = 10
    return rec


def record_bytes(read_len: int) -> int:
    return 16 + read_len + 1 + 2 + read_len + 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--mb", type=float, default=1024.0)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--seed", type=int, default=7)
    a = ap.parse_args()
    nrec = max(1, int(a.mb * (1 << 20)) // record_bytes(a.read_len))
    with open(a.out, "wb") as f:
        for r0 in range(0, nrec, 1 << 18):  # (pieces of about 80 MB)
            n = min(1 << 18, nrec - r0)
            rec = fastq_records(n, a.read_len, a.seed + r0)
            for j in range(10):
                rec[:, 14 - j] = ((np.arange(n, dtype=np.int64) + r0) // 10 ** j % 10 + 48).astype(np.uint8)
            f.write(rec.tobytes())
    print(f"{a.out}: {nrec} records, {nrec * record_bytes(a.read_len)} bytes")


if __name__ == "__main__":
    main()
