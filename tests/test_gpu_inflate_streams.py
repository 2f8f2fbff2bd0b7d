"""GPU: k_bgzf_inflate (pg_inflate.hip) on DEFLATE streams that zlib's encoder never writes (tests/deflate_craft.py), on
libdeflate's streams, on mutants of small blocks judged by zlib, and across the host's piece boundaries (pg_bgzf_inflate's
2^18 blocks per launch, pg_result_inflate_bgzf's 64 MiB staging piece).  Valid streams must come back byte for byte;
malformed ones must fail with PG_E_FORMAT, the block's file offset and the reason for its status."""
import hashlib
import os
import struct
import zlib

import numpy as np
import pytest

from tests import deflate_craft as dc

pytestmark = pytest.mark.gpu

PG_E_FORMAT = -3
PIECE_BLOCKS = 1 << 18  # pg_api_bgzf.hip INF_PIECE_BLOCKS
STAGING = 64 << 20  # pg_api_bgzf.hip INF_PIECE_BYTES


@pytest.fixture(scope="module")
def ctx():
    from panagram_amd import build, engine
    build.build(verbose=False)
    c = engine.Context(0)
    yield c
    c.close()


def inflate(ctx, comp, coffs=None, roffs=None):
    from panagram_amd import engine
    return engine.bgzf_inflate(ctx, comp, coffs, roffs)


def offsets(members, payloads):
    co = np.concatenate([[0], np.cumsum([len(m) for m in members])]).astype(np.uint64)
    ro = np.concatenate([[0], np.cumsum([len(p) for p in payloads])]).astype(np.uint64)
    return co, ro


def check_both_ways(ctx, members, payloads, names):
    """the members inflated twice (blocks walked from the headers; offsets given), each block's bytes compared"""
    comp = b"".join(members)
    co, ro = offsets(members, payloads)
    for label, got in (("walked", inflate(ctx, comp + dc.EOF_MEMBER)), ("offsets", inflate(ctx, comp, co, ro))):
        if got != b"".join(payloads):
            assert len(got) == int(ro[-1]), (label, len(got), int(ro[-1]))
            bad = [names[i] for i in range(len(names)) if got[ro[i]:ro[i + 1]] != payloads[i]]
            raise AssertionError(f"{label}: blocks differ from zlib: {bad[:20]}")


def good_members(n=4, seed=5):
    rng = np.random.default_rng(seed)
    pays = [bytes(rng.integers(0, 4, int(rng.integers(1000, 60000)), dtype=np.uint8)) for _ in range(n)]
    return [dc.bgzf_member(dc.zlib_raw(p, 6), p) for p in pays], pays


def expect_format_error(ctx, comp, off, reason, coffs=None, roffs=None):
    from panagram_amd import engine
    with pytest.raises(engine.PanagramHipError) as ei:
        inflate(ctx, comp, coffs, roffs)
    assert ei.value.code == PG_E_FORMAT, str(ei.value)
    assert str(ei.value).endswith(f"BGZF block at file offset {off}: {reason}"), str(ei.value)


def test_crafted_valid_streams(ctx):
    """every crafted stream (long codes, HLIT 286 / HDIST 30 / HCLEN 8 and 19, repeats across the alphabets, one or no
    distance codes, EOB-only codes, length 258 both ways, distances 1 and 32768, dist < len for 2..70, stored blocks at bit
    offsets 0..7, mixed blocks, trailing bytes after the final block, ISIZE 0 .. 65536), behind headers with and without
    extra subfields, at every coff mod 4"""
    rec = dc.recipes_valid()
    rec.update(dc.recipes_stored_offsets())
    names = sorted(rec)
    members, pays, mods = [], [], set()
    extra = [b"", dc.subfield(b"X", b"Y", b"\x07" * 6), dc.subfield(b"R", b"G", b"")]
    pos = 0
    for i, n in enumerate(names):
        body, payload = rec[n]
        k = i % 5
        m = dc.bgzf_member(body, payload, before=extra[1] if k in (1, 3) else b"", after=extra[2] if k in (2, 3) else
                           extra[1] if k == 4 else b"")
        mods.add(pos % 4)
        pos += len(m)
        members.append(m)
        pays.append(payload)
    assert mods == {0, 1, 2, 3}
    # trailing bytes after the final block are accepted (zlib accepts them too: end of stream inside the body)
    assert "trailing_bytes" in rec and dc.zlib_verdict(rec["trailing_bytes"][0])[0]
    check_both_ways(ctx, members, pays, names)
    # each stream alone as well (a block at coff 0, a single-block launch)
    for n in ("long_codes_ll15_d15", "isize65536_stored", "isize65536_dynamic", "isize0_dynamic", "eob_only_empty",
              "len258_both_dist_extremes", "trailing_bytes"):
        body, payload = rec[n]
        m = dc.bgzf_member(body, payload, before=extra[1])
        assert inflate(ctx, m) == payload, n
        assert inflate(ctx, m, [0, len(m)], [0, len(payload)]) == payload, n


def test_libdeflate_streams(ctx):
    """libdeflate at levels 0..12 (the committed fixture): the kernel's bytes equal zlib's and the recorded sha256"""
    z = np.load(os.path.join(os.path.dirname(__file__), "golden", "inflate", "libdeflate_blocks.npz"))
    sha = dict(zip(z["payload_names"].tolist(), z["payload_sha256"].tolist()))
    offs = z["body_offsets"]
    members, pays, names = [], [], []
    for j in range(len(offs) - 1):
        body = z["bodies"][offs[j]:offs[j + 1]].tobytes()
        p = zlib.decompress(body, -15)
        assert hashlib.sha256(p).hexdigest() == sha[str(z["payload"][j])]
        members.append(dc.bgzf_member(body, p))
        pays.append(p)
        names.append(f"{z['payload'][j]}@{z['level'][j]}")
    check_both_ways(ctx, members, pays, names)


INVALID = dc.recipes_invalid()


@pytest.mark.parametrize("name", sorted(INVALID))
def test_crafted_invalid_stream_is_named(ctx, name):
    body, declared, _, reason = INVALID[name]
    good, gp = good_members(4)
    bad = dc.bgzf_member(body, declared, before=dc.subfield(b"X", b"Y", b"ab") if len(name) % 2 else b"")
    members = good[:2] + [bad] + good[2:]
    pays = gp[:2] + [declared] + gp[2:]
    off = len(good[0]) + len(good[1])
    comp = b"".join(members)
    expect_format_error(ctx, comp + dc.EOF_MEMBER, off, reason)
    co, ro = offsets(members, pays)
    expect_format_error(ctx, comp, off, reason, co, ro)
    # the context goes on working
    assert inflate(ctx, b"".join(good)) == b"".join(gp)


def test_footer_and_offsets_statuses(ctx):
    """ISIZE from the footer and from roffs, CRC, and the host's header checks"""
    good, gp = good_members(3, seed=9)
    p = b"footer checks " * 300
    body = dc.zlib_raw(p)
    off = len(good[0])

    def with_bad(m):
        return good[0] + m + good[1] + good[2]

    # the footer's ISIZE one more than the data (blocks walked: the kernel's ISIZE is the footer's)
    expect_format_error(ctx, with_bad(dc.bgzf_member(body, p, isize=len(p) + 1)), off, "ISIZE mismatch")
    # the footer right, roffs one more (or one less: the data overruns it)
    members = [good[0], dc.bgzf_member(body, p), good[1]]
    co, ro = offsets(members, [gp[0], p, gp[1]])
    ro2 = ro.copy()
    ro2[2:] += 1
    expect_format_error(ctx, b"".join(members), off, "ISIZE mismatch", co, ro2)
    ro2[2:] -= 2
    expect_format_error(ctx, b"".join(members), off, "output overruns ISIZE", co, ro2)
    # the footer one more than roffs (which match the data)
    members[1] = dc.bgzf_member(body, p, isize=len(p) + 1)
    expect_format_error(ctx, b"".join(members), off, "ISIZE mismatch", co, ro)
    # roffs that give a block more than 65536 bytes: refused by the host
    ro3 = ro.copy()
    ro3[2:] += 70000
    expect_format_error(ctx, b"".join(members), off, "ISIZE mismatch", co, ro3)
    # CRC
    expect_format_error(ctx, with_bad(dc.bgzf_member(body, p, crc=zlib.crc32(p) ^ 0x10000)), off, "CRC32 mismatch")
    # headers: no BC subfield; BSIZE past the buffer; ISIZE over 65536 in the footer
    m = bytearray(dc.bgzf_member(body, p, before=dc.subfield(b"X", b"Y", b"12")))
    m[18:20] = b"QC"
    expect_format_error(ctx, with_bad(bytes(m)), off, "bad header")
    expect_format_error(ctx, good[0] + dc.bgzf_member(body, p, bsize=65535), off, "bad header")
    expect_format_error(ctx, with_bad(dc.bgzf_member(body, p, isize=65537)), off, "bad header")
    assert inflate(ctx, b"".join(good)) == b"".join(gp)


def test_mutants_against_zlib(ctx):
    """mutants of small blocks (zlib at several levels / strategies, libdeflate, the crafted writer): what zlib accepts
    (end of stream inside the body, <= 65536 bytes, footer written for zlib's output) the kernel returns byte for byte;
    what zlib refuses fails with PG_E_FORMAT naming the block (footer: that of the unmutated stream)"""
    ms = dc.mutants()
    base = {n: zlib.decompress(b, -15) for n, b in dc.base_streams()}
    acc = [m for m in ms if m[3]]
    rej = [m for m in ms if not m[3]]
    assert acc and rej
    for i in range(0, len(acc), 400):
        chunk = acc[i:i + 400]
        members = [dc.bgzf_member(m[2], m[4]) for m in chunk]
        check_both_ways(ctx, members, [m[4] for m in chunk], [f"seed {m[0]} ({m[1]})" for m in chunk])
    good, gp = good_members(2, seed=13)
    off = len(good[0]) + len(good[1])
    from panagram_amd import engine
    wrong = []
    for seed, name, body, _, _ in rej:
        comp = good[0] + good[1] + dc.bgzf_member(body, base[name])
        try:
            inflate(ctx, comp)
            wrong.append((seed, name, "accepted"))
        except engine.PanagramHipError as e:
            if e.code != PG_E_FORMAT or f"BGZF block at file offset {off}:" not in str(e):
                wrong.append((seed, name, str(e)))
    assert not wrong, f"{len(wrong)} of {len(rej)} mutants zlib refuses: {wrong[:10]}"
    assert inflate(ctx, b"".join(good)) == b"".join(gp)


def test_more_blocks_than_one_launch(ctx):
    """2^18 + 300 tiny blocks: two launches; a corrupt block in the second is named at its own offset"""
    rng = np.random.default_rng(17)
    tpl_p = [bytes(rng.integers(0, 256, int(rng.integers(0, 6)), dtype=np.uint8)) for _ in range(61)]
    tpl_m = [dc.bgzf_member(dc.zlib_raw(p, 6), p) for p in tpl_p]
    n = PIECE_BLOCKS + 300
    idx = rng.integers(0, len(tpl_p), n)
    members = [tpl_m[i] for i in idx]
    pays = [tpl_p[i] for i in idx]
    comp = b"".join(members)
    want = b"".join(pays)
    assert inflate(ctx, comp + dc.EOF_MEMBER) == want
    co, ro = offsets(members, pays)
    assert inflate(ctx, comp, co, ro) == want
    bad = PIECE_BLOCKS + 150
    p = b"piece two"
    members[bad] = dc.bgzf_member(dc.zlib_raw(p), p, crc=zlib.crc32(p) ^ 1)
    expect_format_error(ctx, b"".join(members), int(co[bad]), "CRC32 mismatch")
    assert inflate(ctx, comp + dc.EOF_MEMBER) == want


def _stored_bgzf(payload: bytes, rng):
    """BGZF of stored blocks of random sizes; (file bytes, the blocks' compressed offsets, their payload offsets)"""
    members, co, ro = [], [0], [0]
    pos = 0
    while pos < len(payload):
        L = min(int(rng.integers(20000, 65506)), len(payload) - pos)  # (BSIZE: a member is at most 64 KiB)
        bw = dc.BitWriter()
        dc.stored_block(bw, payload[pos:pos + L], True)
        members.append(dc.bgzf_member(bw.getvalue(), payload[pos:pos + L]))
        pos += L
        co.append(co[-1] + len(members[-1]))
        ro.append(pos)
    return members, co, ro


def test_rows_read_across_the_staging_piece(ctx, tmp_path):
    """AnchorResult.from_bgzf on a bitmap of more than 64 MiB compressed (stored blocks, 8-byte rows): a contig whose rows
    straddle the staging boundary, a file_row0 past it through the .gzi, and a corrupt block past it named at its offset"""
    from panagram_amd import engine
    rng = np.random.default_rng(23)
    nk = [3_000_000, 6_000_000, 700_000]
    rows = rng.integers(0, 256, (sum(nk), 8), dtype=np.uint8)
    members, co, ro = _stored_bgzf(rows.tobytes(), rng)
    assert co[-1] > STAGING + (1 << 20)
    gz = tmp_path / "bitmap.1.gz"
    gz.write_bytes(b"".join(members) + dc.EOF_MEMBER)
    gzi = tmp_path / "bitmap.1.gzi"
    entries = b"".join(struct.pack("<QQ", co[i], ro[i]) for i in range(1, len(members)))
    gzi.write_bytes(struct.pack("<Q", len(members) - 1) + entries)
    off = np.concatenate([[0], np.cumsum(nk)])
    # the staging boundary falls inside contig 1's rows
    b_after = next(i for i in range(len(co)) if co[i] > STAGING) - 1
    assert off[1] * 8 < ro[b_after] < off[2] * 8
    for gzi_path in (str(gzi), None):
        res = engine.AnchorResult.from_bgzf(ctx, 21, 64, nk, str(gz), gzi_path)
        try:
            for c in range(len(nk)):
                assert np.array_equal(res.download(c, True, False)[0], rows[off[c]:off[c + 1]]), (gzi_path, c)
        finally:
            res.close()
    # contig 2 alone: file_row0 past the boundary (the .gzi starts the walk there)
    part = engine.AnchorResult.from_bgzf(ctx, 21, 64, nk[2:], str(gz), str(gzi), file_row0=int(off[2]))
    try:
        assert np.array_equal(part.download(0, True, False)[0], rows[off[2]:off[3]])
    finally:
        part.close()
    # a corrupt block past 64 MiB (one payload byte flipped: its CRC fails), and one inside contig 2
    j = b_after + 3
    k = next(i for i in range(len(ro)) if ro[i] > off[2] * 8 + 100_000) - 1
    assert ro[j + 1] <= off[2] * 8 < ro[k]
    blob = bytearray(gz.read_bytes())
    for b in (j, k):
        blob[co[b] + 18 + 5 + 100] ^= 0xFF
    gz.write_bytes(bytes(blob))
    for gzi_path in (str(gzi), None):
        with pytest.raises(engine.PanagramHipError) as ei:
            engine.AnchorResult.from_bgzf(ctx, 21, 64, nk, str(gz), gzi_path)
        assert ei.value.code == PG_E_FORMAT
        assert str(ei.value).endswith(f"BGZF block at file offset {co[j]}: CRC32 mismatch"), str(ei.value)
    with pytest.raises(engine.PanagramHipError) as ei:
        engine.AnchorResult.from_bgzf(ctx, 21, 64, nk[2:], str(gz), str(gzi), file_row0=int(off[2]))
    assert str(ei.value).endswith(f"BGZF block at file offset {co[k]}: CRC32 mismatch"), str(ei.value)
