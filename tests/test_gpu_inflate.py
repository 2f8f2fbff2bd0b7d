"""GPU: k_bgzf_inflate (pg_inflate.hip) against zlib.decompress, byte for byte, for every writer of BGZF blocks the
project has (pg_bgzf.cpp at every level, the row-aware encoder, k_row_deflate) and for zlib at every level and strategy;
malformed blocks built here return PG_E_FORMAT naming the block, and the context stays usable."""
import gzip
import struct
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PG_E_FORMAT = -3


@pytest.fixture(scope="module")
def ctx():
    from panagram_amd import build, engine
    build.build(verbose=False)
    c = engine.Context(0)
    yield c
    c.close()


def bgzf_member(payload: bytes, body: bytes) -> bytes:
    bsize = 18 + len(body) + 8
    hdr = b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00" + struct.pack("<H", bsize - 1)
    return hdr + body + struct.pack("<II", zlib.crc32(payload) & 0xFFFFFFFF, len(payload))


EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def zlib_bgzf(data: bytes, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, block=65280, flushes=0, mem=8):
    """BGZF written by zlib with the given level / strategy; ``flushes`` > 0 cuts every member into that many more DEFLATE
    blocks (Z_FULL_FLUSH: an empty stored block between them)"""
    out, coffs, roffs = [], [0], [0]
    for s in range(0, len(data), block):
        p = data[s:s + block]
        c = zlib.compressobj(level, zlib.DEFLATED, -15, mem, strategy)
        body = b""
        cuts = np.linspace(0, len(p), flushes + 2).astype(int)
        for a, b in zip(cuts[:-1], cuts[1:]):
            body += c.compress(p[a:b])
            if b < len(p):
                body += c.flush(zlib.Z_FULL_FLUSH)
        body += c.flush()
        out.append(bgzf_member(p, body))
        coffs.append(coffs[-1] + len(out[-1]))
        roffs.append(roffs[-1] + len(p))
    return b"".join(out) + EOF, coffs, roffs


def payloads():
    rng = np.random.default_rng(11)
    rand = rng.integers(0, 256, 200_000, dtype=np.uint8).tobytes()
    runs = np.repeat(rng.integers(0, 4, 3000, dtype=np.uint8), rng.integers(1, 400, 3000)).tobytes()
    rows = []
    for w in (1, 4, 8, 9, 16, 17):
        base = rng.integers(0, 256, (40, w), dtype=np.uint8)
        rows.append(np.repeat(base, rng.integers(1, 300, 40), axis=0).tobytes())
    return {"random": rand, "runs": runs, **{f"rows{i}": r for i, r in enumerate(rows)}}


def inflate(ctx, comp, coffs=None, roffs=None):
    from panagram_amd import engine
    return engine.bgzf_inflate(ctx, comp, coffs, roffs)


@pytest.mark.parametrize("name", sorted(payloads()))
def test_zlib_levels_and_strategies(ctx, name):
    data = payloads()[name]
    for level in range(10):
        comp, co, ro = zlib_bgzf(data, level)
        assert inflate(ctx, comp) == data, f"zlib level {level}"
    for strat in (zlib.Z_FIXED, zlib.Z_HUFFMAN_ONLY, zlib.Z_RLE, zlib.Z_FILTERED):
        comp, co, ro = zlib_bgzf(data, 6, strat)
        assert inflate(ctx, comp) == data, f"strategy {strat}"
        assert inflate(ctx, comp[:co[-1]], co, ro) == data, f"strategy {strat}, given offsets"
    # several DEFLATE blocks per member (stored ones among them), and zlib's small-memory mode (short blocks)
    comp, _, _ = zlib_bgzf(data, 6, flushes=3)
    assert inflate(ctx, comp) == data
    comp, _, _ = zlib_bgzf(data, 9, mem=1, block=32768)  # (random bytes: many short stored blocks, room for them)
    assert inflate(ctx, comp) == data


def test_project_writers_every_level(ctx, tmp_path):
    from panagram_amd import engine
    for name, data in sorted(payloads().items()):
        for level in list(range(10)) + [6 | engine.BgzfWriter.RLE, 6 | engine.BgzfWriter.ROWS(9), 1 | engine.BgzfWriter.ROWS(17)]:
            p = tmp_path / f"{name}.{level}.gz"
            w = engine.BgzfWriter(str(p), level=level, threads=3)
            w.write(np.frombuffer(data, np.uint8))
            w.close(str(p) + ".gzi")
            assert inflate(ctx, p.read_bytes()) == data, (name, level)


@pytest.mark.parametrize("ngenomes", [8, 32, 64, 72, 128, 136])
def test_row_buffers_read_back_and_rewritten(ctx, tmp_path, ngenomes):
    """rows of 1, 4, 8, 9, 16 and 17 bytes: a host-written bitmap inflated into a rows result (pg_result_inflate_bgzf, contigs
    at their padded places), written again at levels 1, 6 and -2 (k_row_deflate), each file inflated again"""
    from panagram_amd import engine
    nb = (ngenomes + 7) // 8
    rng = np.random.default_rng(ngenomes)
    nk = [70001, 3, 0, 150000, 17]
    base = rng.integers(0, 256, (64, nb), dtype=np.uint8)
    rows = np.repeat(base, rng.integers(1, 9000, 64), axis=0)
    rows = np.concatenate([rows] * (sum(nk) // len(rows) + 1))[:sum(nk)]
    rows[rng.integers(0, len(rows), 500)] ^= 0x5A
    payload = rows.tobytes()
    src = tmp_path / "bitmap.1.gz"
    w = engine.BgzfWriter(str(src), level=6 | (engine.BgzfWriter.RLE if nb == 1 else engine.BgzfWriter.ROWS(nb)), threads=4)
    w.write(rows)
    w.close(str(tmp_path / "bitmap.1.gzi"))
    res = engine.AnchorResult.from_bgzf(ctx, 21, ngenomes, nk, str(src), str(tmp_path / "bitmap.1.gzi"))
    try:
        off = np.concatenate([[0], np.cumsum(nk)])
        for c in range(len(nk)):
            got = res.download(c, True, False)[0]
            assert np.array_equal(got, rows[off[c]:off[c + 1]]), f"contig {c}"
        for level in (1, 6, -2):
            out = tmp_path / f"again{level}.gz"
            res.write_bgzf(1, str(out), str(out) + ".gzi", level=level, threads=4)
            assert gzip.decompress(out.read_bytes()) == payload, f"level {level}"
            assert inflate(ctx, out.read_bytes()) == payload, f"level {level}"
    finally:
        res.close()
    # a batch of contigs in the middle of the file (file_row0), through the .gzi
    part = engine.AnchorResult.from_bgzf(ctx, 21, ngenomes, nk[3:], str(src), str(tmp_path / "bitmap.1.gzi"), file_row0=int(off[3]))
    try:
        assert np.array_equal(part.download(0, True, False)[0], rows[off[3]:off[4]])
        assert np.array_equal(part.download(1, True, False)[0], rows[off[4]:off[5]])
    finally:
        part.close()


def test_one_block_many_blocks_and_empty(ctx):
    data = b"ACGT" * 1000
    comp, _, _ = zlib_bgzf(data)
    assert comp.count(b"BC\x02\x00") == 2
    assert inflate(ctx, comp) == data
    rng = np.random.default_rng(3)
    big = np.repeat(rng.integers(0, 3, 40000, dtype=np.uint8), rng.integers(1, 1000, 40000)).tobytes()
    comp, co, ro = zlib_bgzf(big, 1, zlib.Z_RLE, block=4096)
    assert len(co) > 3000
    assert inflate(ctx, comp) == big
    assert inflate(ctx, EOF) == b""
    assert inflate(ctx, b"") == b""


class Bits:
    def __init__(self):
        self.v, self.n = 0, 0

    def put(self, val, n):  # LSB first
        self.v |= val << self.n
        self.n += n

    def huff(self, code, n):  # a Huffman code goes in MSB first
        self.put(int(f"{code:0{n}b}"[::-1], 2), n)

    def bytes(self):
        return self.v.to_bytes((self.n + 7) // 8, "little")


def oversubscribed_block():
    b = Bits()
    b.put(1, 1)
    b.put(2, 2)  # dynamic
    b.put(0, 5)
    b.put(0, 5)
    b.put(0, 4)  # HCLEN = 4: code lengths of symbols 16, 17, 18, 0
    for _ in range(4):
        b.put(1, 3)  # four codes of length 1: over-subscribed
    b.put(0, 32)
    return bgzf_member(b"x", b.bytes())


def distance_before_start_block():
    b = Bits()
    b.put(1, 1)
    b.put(1, 2)  # fixed Huffman
    b.huff(1, 7)  # symbol 257: length 3
    b.huff(0, 5)  # distance code 0: distance 1, at output position 0
    b.huff(0, 7)  # end of block
    return bgzf_member(b"aaa", b.bytes())


@pytest.mark.parametrize("kind", ["crc", "isize", "oversubscribed", "distance"])
def test_malformed_block_is_named(ctx, kind):
    from panagram_amd import engine
    rng = np.random.default_rng(5)
    data = rng.integers(0, 4, 300_000, dtype=np.uint8).tobytes()
    comp, co, ro = zlib_bgzf(data, 6)
    blocks = [bytearray(comp[co[i]:co[i + 1]]) for i in range(len(co) - 1)]
    bad = 2
    if kind == "crc":
        blocks[bad][-6] ^= 0x40
    elif kind == "isize":
        blocks[bad][-4] ^= 0x01
    elif kind == "oversubscribed":
        blocks[bad] = bytearray(oversubscribed_block())
    else:
        blocks[bad] = bytearray(distance_before_start_block())
    bad_off = sum(len(b) for b in blocks[:bad])
    comp2 = b"".join(bytes(b) for b in blocks) + EOF
    with pytest.raises(engine.PanagramHipError) as ei:
        inflate(ctx, comp2)
    assert ei.value.code == PG_E_FORMAT
    assert f"file offset {bad_off}:" in str(ei.value), str(ei.value)
    # the context goes on working
    assert inflate(ctx, comp) == data
