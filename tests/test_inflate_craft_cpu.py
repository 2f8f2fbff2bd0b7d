"""CPU: the DEFLATE writer of tests/deflate_craft.py pinned to zlib (every valid recipe inflates to its intended bytes, every
invalid one is refused with the message expected for it), its decoder pinned to zlib, the mutation sweep's balance, and
the BGZF header walk engine.bgzf_inflate sizes its output with."""
import zlib

import numpy as np
import pytest

from tests import deflate_craft as dc


def _valid():
    r = dc.recipes_valid()
    r.update(dc.recipes_stored_offsets())
    return r


VALID = _valid()
INVALID = dc.recipes_invalid()


@pytest.mark.parametrize("name", sorted(VALID))
def test_valid_recipe_inflates_to_its_bytes(name):
    body, payload = VALID[name]
    assert len(payload) <= 65536
    assert len(dc.bgzf_member(body, payload, before=dc.subfield(b"X", b"Y", b"\x07" * 6))) <= 65536  # (fits a BGZF member)
    ok, out, msg = dc.zlib_verdict(body)
    assert ok, msg
    assert out == payload
    assert dc.Inflater(body).run() == payload


@pytest.mark.parametrize("name", sorted(INVALID))
def test_invalid_recipe_refused_by_zlib(name):
    body, declared, zmsg, _ = INVALID[name]
    ok, out, msg = dc.zlib_verdict(body)
    if zmsg == "":  # a valid stream; its footer declares another size
        assert ok and len(out) != len(declared)
    else:
        assert not ok and msg == zmsg, msg


def test_recipes_reach_what_they_claim():
    """the headers and code lengths the crafted streams are named for"""
    def blocks(name):
        inf = dc.Inflater(VALID[name][0])
        inf.run()
        return inf.blocks

    b = blocks("long_codes_ll15_d15")[0]
    assert b["max_ll"] == 15 and b["max_d"] == 15
    used = {L for L in b["ll_lens"] if L}
    assert set(range(11, 16)) <= used and set(range(9, 16)) <= {L for L in b["d_lens"] if L}
    b = blocks("long_codes_far")[0]
    assert b["max_ll"] == 15 and b["max_d"] == 15
    b = blocks("hlit286_hdist30_hclen19")[0]
    assert (b["hlit"], b["hdist"], b["hclen"]) == (286, 30, 19)
    assert all(b["ll_lens"]) and all(b["d_lens"]) and b["max_ll"] > 10
    b = blocks("hclen8_six_bit_code")[0]
    assert b["hclen"] == 8 and b["hdist"] == 1 and b["d_lens"] == [0]
    for sym in (16, 17, 18):
        b = blocks(f"repeat{sym}_crosses")[0]
        assert b["hlit"] == 286
    assert blocks("one_distance_code_dist1")[0]["d_lens"] == [1]
    assert blocks("eob_only_empty")[0]["ll_lens"].count(0) == 256
    assert [x["type"] for x in blocks("mixed_blocks")] == ["stored", "fixed", "dynamic", "stored", "fixed", "dynamic", "stored"]
    # every stored-offset recipe puts its stored block at the bit offset it is named for
    for name, (body, _) in VALID.items():
        if name.startswith("stored_off"):
            off = int(name[len("stored_off"):].split("_")[0])
            st = [x for x in blocks(name) if x["type"] == "stored"][0]
            assert st["start_bit"] % 8 == off, name


def test_rle_crosses_the_alphabets():
    """the repeat codes of the *_crosses recipes really run from the literal/length lengths into the distance lengths"""
    for sym in (16, 17, 18):
        body = VALID[f"repeat{sym}_crosses"][0]
        inf = dc.Inflater(body)
        inf.run()
        assert inf.blocks[0]["hlit"] == 286
    # rle_lengths over ll + d lengths: a run over the boundary is one token
    toks = dc.rle_lengths([5] * 10 + [0] * 20, use16=True)
    assert (16, 3) in toks and (18, 9) in toks


def test_canonical_codes_rfc1951_example():
    """RFC 1951 3.2.2: lengths (3, 3, 3, 3, 3, 2, 4, 4) -> 010 011 100 101 110 00 1110 1111"""
    codes = dc.canonical([3, 3, 3, 3, 3, 2, 4, 4])
    assert codes == [(2, 3), (3, 3), (4, 3), (5, 3), (6, 3), (0, 2), (14, 4), (15, 4)]
    fib = [1, 1, 2, 3, 5, 8, 13, 21, 34, 55, 89, 144, 233, 377, 610, 987, 1597, 2584]
    assert dc.kraft(dc.huffman_lengths(fib, 15)) == 1 << 15
    lens = dc.huffman_lengths([1] * 2 + [1 << i for i in range(20)], 15)
    assert max(lens) == 15 and dc.kraft(lens) == 1 << 15


def test_decoder_agrees_with_zlib_on_its_output():
    rng = np.random.default_rng(7)
    for data in (bytes(rng.integers(0, 4, 20000, dtype=np.uint8)), bytes(rng.integers(0, 256, 3000, dtype=np.uint8)), b""):
        for level in (0, 1, 6, 9):
            for strat in (zlib.Z_DEFAULT_STRATEGY, zlib.Z_FIXED, zlib.Z_RLE):
                assert dc.Inflater(dc.zlib_raw(data, level, strat)).run() == data


def test_bgzf_member_with_extra_subfields():
    body, payload = VALID["mixed_blocks"]
    extra = dc.subfield(b"X", b"Y", b"abcdef")
    for before, after in ((b"", b""), (extra, b""), (b"", extra), (extra, dc.subfield(b"Z", b"Z", b""))):
        m = dc.bgzf_member(body, payload, before, after)
        assert dc.member_body(m)[0] == body
        import gzip
        assert gzip.decompress(m) == payload


def test_engine_sizes_blocks_with_extra_subfields():
    """engine.bgzf_inflate sizes its output by walking BSIZE: with an extra subfield before BC the walk must find BC, not
    read BSIZE at bytes 16-17 (three such blocks of 12000 bytes: 36000, not 0)"""
    from panagram_amd import engine
    rng = np.random.default_rng(1)
    blocks = []
    for i in range(3):
        p = bytes(rng.integers(0, 4, 12000, dtype=np.uint8))
        blocks.append(dc.bgzf_member(dc.zlib_raw(p), p, before=dc.subfield(b"X", b"Y", b"\x01" * 6)))
    buf = np.frombuffer(b"".join(blocks) + dc.EOF_MEMBER, np.uint8)
    assert engine._bgzf_payload_bytes(buf) == 36000
    after = [dc.bgzf_member(dc.zlib_raw(b"x" * 500), b"x" * 500, after=dc.subfield(b"R", b"G", b"\x00" * 40))] * 2
    assert engine._bgzf_payload_bytes(np.frombuffer(b"".join(after + blocks), np.uint8)) == 37000
    # no BC subfield: the walk stops there (the library names the block)
    bad = bytearray(blocks[1])
    bad[22:24] = b"QQ"  # (BC, behind the 10-byte XY subfield)
    assert engine._bgzf_payload_bytes(np.frombuffer(blocks[0] + bytes(bad) + blocks[2], np.uint8)) == 12000


def test_mutants_both_verdicts():
    """the sweep's default seeds give accepted and rejected mutants, each at least a tenth; an accepted one fits a block"""
    ms = dc.mutants()
    assert len(ms) == dc.fuzz_count()
    acc = sum(1 for m in ms if m[3])
    assert acc >= 0.1 * len(ms) and len(ms) - acc >= 0.1 * len(ms), (acc, len(ms))
    assert all(len(m[4]) <= 65536 for m in ms if m[3])
    assert {m[1].split("_")[0] for m in ms} >= {"zlib0", "zlib6", "libdeflate", "craft"}
    # the verdict is zlib's own
    for seed, _, body, ok, data in ms[:300]:
        d = zlib.decompressobj(-15)
        try:
            out = d.decompress(body)
            assert ok == (d.eof and len(out) <= 65536), seed
            if ok:
                assert out == data
        except zlib.error:
            assert not ok


def test_libdeflate_fixture():
    """the committed libdeflate streams: zlib inflates each to a payload whose sha256 the fixture records"""
    import hashlib
    import os
    z = np.load(os.path.join(os.path.dirname(__file__), "golden", "inflate", "libdeflate_blocks.npz"))
    sha = dict(zip(z["payload_names"].tolist(), z["payload_sha256"].tolist()))
    offs = z["body_offsets"]
    assert str(z["version"]) != "unknown" and sorted(set(z["level"].tolist())) == list(range(13))
    for j in range(len(offs) - 1):
        out = zlib.decompress(z["bodies"][offs[j]:offs[j + 1]].tobytes(), -15)
        assert len(out) == z["isize"][j] and hashlib.sha256(out).hexdigest() == sha[str(z["payload"][j])]
