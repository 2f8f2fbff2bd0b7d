"""A model of the GPU BGZF encoder (pg_deflate.hip: k_df_sample_hist, k_df_build_code, k_row_deflate) in plain numpy / Python,
restated from the RULE in that file's header comment, not from its code, and the crafted payloads that aim at the places where
the kernels can go wrong.  No tests in here: tests/test_deflate_rows_cpu.py ties the model to zlib and proves that the payloads
hold what they promise, tests/test_gpu_deflate_rows.py holds the kernels to the model.

The rule.  The payload is cut into blocks of 65280 bytes.  Byte i of a block (i counts from the block's start) is EQUAL iff
i >= row and b[i] == b[i - row].  A maximal run of R equal bytes becomes R // 258 matches of 258, then one match of
r = R % 258 if r >= 3, else r literals; every other byte is a literal; one end-of-block per block.  Every match has the
distance ``row``.  ONE literal/length code per file: the counts of the sampled blocks (``sample_blocks``) + 1 for every
symbol, end-of-block = the number of sampled blocks; the distance code is the row width's symbol alone, one bit.  A block whose
dynamic form is longer than 65510 bytes is written as a stored block."""
import heapq
import struct
import zlib

import numpy as np

from tests import deflate_craft as dc

BLOCK = 65280
CHUNK = 68            # bytes per thread of k_row_deflate
SAMPLE = 512          # blocks k_df_sample_hist looks at, at most
MAX_DYNAMIC = 65510   # 65536 - 18 (BGZF header) - 8 (CRC32, ISIZE)
POISON = 0xA5

LSYM = np.zeros(259, np.int64)  # length symbol of a match of L bytes
for _L in range(3, 259):
    LSYM[_L] = dc.len_symbol(_L)
LEN_EXTRA = np.zeros(286, np.int64)
LEN_EXTRA[257:] = dc.LEN_EXTRA


def row_bytes(n):
    return (n + 7) // 8


# ---------------------------------------------------------------------------
# the token rule
# ---------------------------------------------------------------------------
def _structure(block, row, tail_min=3, cut=258, before=None, split=None):
    """(literal mask, match starts, match lengths) of one block.  The keyword arguments are the MUTATED rules of the
    sensitivity test (tests/test_deflate_rows_cpu.py): the tail becomes a match from ``tail_min`` bytes, runs are cut into
    matches of ``cut``, the block's first ``row`` bytes are compared with ``before`` (the payload ahead of the block), runs
    end at every multiple of ``split``."""
    b = np.asarray(block, np.uint8)
    n = len(b)
    eq = np.zeros(n, bool)
    if n > row:
        eq[row:] = b[row:] == b[:-row]
    if before is not None and len(before) >= row:
        k = min(row, n)
        eq[:k] = b[:k] == np.asarray(before, np.uint8)[len(before) - row:len(before) - row + k]
    pos = np.arange(n)
    first = eq & ~np.concatenate(([False], eq[:-1]))
    last = eq & ~np.concatenate((eq[1:], [False]))
    if split:
        first |= eq & (pos % split == 0)
        last |= eq & ((pos + 1) % split == 0)
    starts, ends = np.flatnonzero(first), np.flatnonzero(last) + 1
    R = ends - starts
    q, r = R // cut, R % cut
    tail = r >= tail_min
    lit = ~eq
    for k in range(1, tail_min):  # the r < tail_min last bytes of a run: literals
        lit[ends[~tail & (r >= k)] - k] = True
    rep = np.repeat(np.arange(len(R)), q)
    j = np.arange(len(rep)) - np.repeat(np.cumsum(q) - q, q)
    mstart = np.concatenate((starts[rep] + cut * j, (starts + cut * q)[tail]))
    mlen = np.concatenate((np.full(len(rep), cut, np.int64), r[tail]))
    o = np.argsort(mstart, kind="stable")
    return lit, mstart[o], mlen[o]


def tokens(block, row, **rule):
    """the block's tokens in order, as tests/deflate_craft.py writes them: ints are literals, ("m", length, row) matches"""
    b = np.asarray(block, np.uint8)
    lit, mstart, mlen = _structure(b, row, **rule)
    lp = np.flatnonzero(lit)
    ev = [(int(p), int(b[p])) for p in lp] + [(int(p), ("m", int(L), row)) for p, L in zip(mstart, mlen)]
    ev.sort(key=lambda x: x[0])
    return [t for _, t in ev]


def hist(block, row, **rule):
    """286 symbol counts of the block's tokens, end-of-block included"""
    b = np.asarray(block, np.uint8)
    lit, _, mlen = _structure(b, row, **rule)
    h = np.zeros(286, np.int64)
    h[:256] = np.bincount(b[lit], minlength=256)
    h += np.bincount(LSYM[mlen], minlength=286)
    h[256] = 1
    return h


def blocks_of(payload):
    p = np.frombuffer(bytes(payload), np.uint8) if not isinstance(payload, np.ndarray) else payload
    return [p[i:i + BLOCK] for i in range(0, len(p), BLOCK)]


def sample_blocks(nblocks):
    ns = min(nblocks, SAMPLE)
    return [i * nblocks // ns for i in range(ns)]


def file_hist(payload, row, hists=None):
    """what k_df_build_code makes the file's code from (``hists``: the blocks' counts, where the caller has them)"""
    blks = blocks_of(payload)
    take = sample_blocks(len(blks))
    h = np.zeros(286, np.int64)
    for i in take:
        h += hists[i] if hists is not None else hist(blks[i], row)
    h += 1
    h[256] = max(1, len(take))
    return h


# ---------------------------------------------------------------------------
# the size law
# ---------------------------------------------------------------------------
def code_bits(h, ll_lens):
    """bits of the literal/length CODES alone (no extra bits): what the quality of a code is measured in"""
    return int(np.dot(np.asarray(h, np.int64), np.asarray(list(ll_lens)[:286], np.int64)))


def token_bits(h, ll_lens, row, d_lens):
    """all bits behind the block header: codes, the length symbols' extra bits, and per match the distance code and the
    extra bits of the row width's distance symbol"""
    h = np.asarray(h, np.int64)
    ds = dc.dist_symbol(row)
    nmatch = int(h[257:].sum())
    return code_bits(h, ll_lens) + int(np.dot(h, LEN_EXTRA)) + nmatch * (int(d_lens[ds]) + dc.DIST_EXTRA[ds])


def sbytes(h, ll_lens, row, d_lens, hdr_bits):
    return (hdr_bits + token_bits(h, ll_lens, row, d_lens) + 7) // 8


def member_size(h, n, ll_lens, row, d_lens, hdr_bits):
    """(BSIZE + 1, stored?) of a block of n bytes with counts h"""
    s = sbytes(h, ll_lens, row, d_lens, hdr_bits)
    if s <= MAX_DYNAMIC:
        return 18 + s + 8, False
    return 18 + 5 + n + 8, True


# ---------------------------------------------------------------------------
# reference code lengths
# ---------------------------------------------------------------------------
def huffman_cost(h):
    """(cost in bits, depth) of the unlimited Huffman optimum; among equal weights the shallower subtree merges first, which
    gives the optimum of least depth"""
    heap = [(int(f), 0) for f in h if f > 0]
    if len(heap) == 1:
        return heap[0][0], 1
    heapq.heapify(heap)
    cost = 0
    while len(heap) > 1:
        (a, da), (b, db) = heapq.heappop(heap), heapq.heappop(heap)
        cost += a + b
        heapq.heappush(heap, (a + b, max(da, db) + 1))
    return cost, heap[0][1]


def limited_cost(h, maxbits=15):
    """cost of the optimal code of at most ``maxbits`` bits (package-merge)"""
    return code_bits(h, dc.huffman_lengths([int(f) for f in h], maxbits))


def fixed_cost(h):
    return code_bits(h, dc.FIXED_LL)


# ---------------------------------------------------------------------------
# reading a BGZF file
# ---------------------------------------------------------------------------
def members(gz):
    """[dict(offset, bsize, body, crc, isize)] of a BGZF file, the EOF block included"""
    out, at = [], 0
    while at < len(gz):
        assert gz[at:at + 4] == b"\x1f\x8b\x08\x04", f"no BGZF member at {at}"
        xlen = gz[at + 10] | gz[at + 11] << 8
        x, bsize = at + 12, None
        while x < at + 12 + xlen:
            slen = gz[x + 2] | gz[x + 3] << 8
            if gz[x:x + 2] == b"BC":
                assert slen == 2
                bsize = gz[x + 4] | gz[x + 5] << 8
            x += 4 + slen
        assert bsize is not None and at + bsize + 1 <= len(gz), f"member at {at}: no BC subfield or a BSIZE past the file"
        end = at + bsize + 1
        crc, isize = struct.unpack("<II", gz[end - 8:end])
        out.append(dict(offset=at, bsize=bsize, body=gz[at + 12 + xlen:end - 8], crc=crc, isize=isize))
        at = end
    return out


def read_header(body):
    """(ll_lens, d_lens, hdr_bits) of a body that is one final dynamic block — hdr_bits counts its BFINAL / BTYPE bits too —
    or None for a stored block"""
    inf = dc.Inflater(body)
    final, btype = inf.bits(1), inf.bits(2)
    assert final == 1, "a BGZF member of the encoder holds ONE block"
    if btype == 0:
        return None
    assert btype == 2, f"block type {btype}"
    h = inf.dynamic_header()
    return h["ll_lens"], h["d_lens"], inf.pos


def stored_payload(body):
    n, nn = struct.unpack("<HH", body[1:5])
    assert body[0] == 1 and n ^ 0xFFFF == nn and len(body) == 5 + n
    return body[5:]


def check_file(gz, gzi, payload, row, modelled=True, hists=None):
    """assertions (a) to (f) of tests/test_gpu_deflate_rows.py on one file; ``modelled=False`` (a file of the host writer):
    (a) to (c) only; ``hists``: {block: its counts} where the caller has them already.  Returns dict(ll_lens, d_lens,
    hdr_bits, hdr, stored: [bool per block], sizes, want_sizes, hists)."""
    payload = bytes(payload)
    blks = blocks_of(payload)
    mem = members(gz)
    # (b) footers, EOF block
    assert gz[-28:] == dc.EOF_MEMBER and mem[-1]["isize"] == 0
    mem = mem[:-1]
    if modelled:
        assert len(mem) == len(blks), (len(mem), len(blks))
    # (a) the payload, by zlib
    out = bytearray()
    for i, m in enumerate(mem):
        d = zlib.decompressobj(-15)
        data = d.decompress(m["body"])
        assert d.eof and not d.unused_data, f"block {i}: the deflate stream does not end with the body"
        assert m["isize"] == len(data) and m["crc"] == zlib.crc32(data) & 0xFFFFFFFF, f"block {i}: CRC32 / ISIZE"
        out += data
    assert bytes(out) == payload, "the file does not inflate to the payload"
    # (c) the index
    if gzi is not None:
        g = np.frombuffer(gzi, "<u8")
        assert g[0] == max(0, len(mem) - 1) and len(g) == 1 + 2 * int(g[0])
        offs = np.cumsum([0] + [m["bsize"] + 1 for m in mem])
        assert np.array_equal(g[1::2], offs[1:len(mem)].astype(np.uint64)), ".gzi compressed offsets"
        isz = np.cumsum([0] + [m["isize"] for m in mem])
        assert np.array_equal(g[2::2], isz[1:len(mem)].astype(np.uint64)), ".gzi uncompressed offsets"
        if modelled:
            assert np.array_equal(g[2::2], np.arange(1, len(mem), dtype=np.uint64) * BLOCK)
    res = dict(stored=[], sizes=[m["bsize"] + 1 for m in mem], want_sizes=[], hists=[], ll_lens=None, d_lens=None, hdr_bits=None)
    if not modelled:
        return res
    # (d) one header for the file
    for i, m in enumerate(mem):
        h = read_header(m["body"])
        res["stored"].append(h is None)
        if h is None:
            assert stored_payload(m["body"]) == blks[i].tobytes(), f"block {i}: stored bytes"
            continue
        if res["ll_lens"] is None:
            res["ll_lens"], res["d_lens"], res["hdr_bits"] = h
            res["hdr"] = int.from_bytes(m["body"][:(h[2] + 7) // 8], "little") & ((1 << h[2]) - 1)
        hb = res["hdr_bits"]
        assert int.from_bytes(m["body"][:(hb + 7) // 8], "little") & ((1 << hb) - 1) == res["hdr"], f"block {i}: another header"
    res["hists"] = [hists[i] if hists and i in hists else hist(b, row) for i, b in enumerate(blks)]
    if res["ll_lens"] is None:  # every block stored: the law needs no code
        res["want_sizes"] = [18 + 5 + len(b) + 8 for b in blks]
        assert res["sizes"] == res["want_sizes"]
        return res
    ll, dl = res["ll_lens"], res["d_lens"]
    # (e) the code
    ds = dc.dist_symbol(row)
    assert len(ll) == 286 and all(1 <= L <= 15 for L in ll) and dc.kraft(ll) == 1 << 15, "literal/length code"
    assert len(dl) == ds + 1 and dl[ds] == 1 and not any(dl[:ds]), "distance code: the row width's symbol alone, one bit"
    # (f) the exact size
    bad = []
    for i, (m, b) in enumerate(zip(mem, blks)):
        want, st = member_size(res["hists"][i], len(b), ll, row, dl, res["hdr_bits"])
        res["want_sizes"].append(want)
        if (want, st) != (m["bsize"] + 1, res["stored"][i]):
            bad.append((i, want, st, m["bsize"] + 1, res["stored"][i]))
    assert not bad, f"(block, expected BSIZE+1, stored, actual BSIZE+1, stored) {bad[:8]} ... {len(bad)} blocks differ"
    return res


def check_code(ll_lens, fh):
    """assertion (g) on the file's counts; returns (cost, huffman cost, depth, limited cost)"""
    cost = code_bits(fh, ll_lens)
    hc, depth = huffman_cost(fh)
    lc = limited_cost(fh, 15)
    if depth <= 15:
        assert hc == lc and cost == hc, (cost, hc, depth)
    else:
        assert lc <= cost <= fixed_cost(fh), (lc, cost, fixed_cost(fh))
        f, L = np.asarray(fh, np.int64), np.asarray(ll_lens, np.int64)
        assert not ((f[:, None] > f[None, :]) & (L[:, None] > L[None, :])).any(), "a more frequent symbol has the longer code"
    return cost, hc, depth, lc


# ---------------------------------------------------------------------------
# the model as a writer (CPU only: proves tokens, size law and checker on real bytes)
# ---------------------------------------------------------------------------
class FastBits(dc.BitWriter):
    """dc.BitWriter with the finished bytes moved out of the integer (a block holds 65 000 tokens)"""

    def __init__(self):
        super().__init__()
        self.done = bytearray()

    def put(self, val, n):
        super().put(val, n)
        if self.n >= 256:
            k = self.n // 8
            self.done += (self.v & ((1 << (8 * k)) - 1)).to_bytes(k, "little")
            self.v >>= 8 * k
            self.n -= 8 * k
        return self

    def align(self):
        self.n = (self.n + 7) // 8 * 8
        return self

    def bits(self):
        return 8 * len(self.done) + self.n

    def getvalue(self):
        return bytes(self.done) + super().getvalue()


def dynamic_body(toks, ll_lens, row):
    """one final dynamic block of the tokens: 286 literal/length lengths, the row width's distance symbol alone"""
    ds = dc.dist_symbol(row)
    bw = FastBits()
    dc.dynamic_block(bw, toks, True, ll_lens=list(ll_lens), d_lens=[0] * ds + [1], hlit=286, hdist=ds + 1)
    return bw.getvalue()


def model_file(payload, row):
    """(gz bytes, gzi bytes): the BGZF file the rule gives, with package-merge code lengths"""
    blks = blocks_of(payload)
    ll = dc.huffman_lengths([int(f) for f in file_hist(payload, row)], 15)
    out, offs = bytearray(), []
    for b in blks:
        body = dynamic_body(tokens(b, row), ll, row)
        if len(body) > MAX_DYNAMIC:
            bw = dc.BitWriter()
            dc.stored_block(bw, b.tobytes(), True)
            body = bw.getvalue()
        offs.append(len(out))
        out += dc.bgzf_member(body, b.tobytes())
    out += dc.EOF_MEMBER
    gzi = struct.pack("<Q", max(0, len(blks) - 1)) + b"".join(struct.pack("<QQ", offs[i], i * BLOCK) for i in range(1, len(blks)))
    return bytes(out), gzi


# ---------------------------------------------------------------------------
# crafted payloads: bytes from a mask of UNEQUAL bytes
# ---------------------------------------------------------------------------
def from_mask(mask, row, seed, n=None, bits=8):
    """b[i] = b[i - row] where the mask is clear, b[i - row] ^ (something non-zero) where it is set; the first row is
    random.  Only the ``bits`` low bits of a byte are used, and in a row's last byte only the bits below N (n genomes)."""
    mask = np.asarray(mask, bool)
    assert len(mask) % row == 0
    n = 8 * row if n is None else n
    assert row_bytes(n) == row
    rng = np.random.default_rng(seed)
    d = rng.integers(1, 1 << bits, len(mask)).astype(np.uint8)
    last_bits = min(bits, n - 8 * (row - 1))
    if last_bits < bits:
        col = np.arange(len(mask)) % row == row - 1
        d[col] = rng.integers(1, 1 << last_bits, int(col.sum()))
    first = d[:row].copy()
    d[~mask] = 0
    d[:row] = first
    return np.bitwise_xor.accumulate(d.reshape(-1, row), axis=0).reshape(-1)


LADDER_LENGTHS = sorted(set(range(1, 6)) | set(range(30, 35)) | set(range(62, 71)) | set(range(94, 99)) | set(range(134, 139))
                        | set(range(255, 262)) | set(range(515, 520)) | set(range(774, 778)) | {1032})


def ladder_mask(row):
    """the unequal mask of ``ladder``: for every L of LADDER_LENGTHS a run of exactly L clear bytes starting at every residue
    0..67 of the offset mod 68, between separators of 1, 2 or 3 set bytes (more where the next residue or a block's end asks
    for them), then one run of every length 3..258; no run touches a block's first ``row`` bytes or its end"""
    mask = np.ones(4 << 20, bool)
    p, cnt = row + 1, 0
    for L in LADDER_LENGTHS:
        todo = set(range(CHUNK))
        while todo:
            at = p % BLOCK
            if p % CHUNK not in todo or at < row + 1 or at + L + 1 > BLOCK:
                p += 1
                continue
            mask[p:p + L] = False
            todo.discard(p % CHUNK)
            p += L
            ws = [(cnt + j) % 3 + 1 for j in range(3)]
            p += next((w for w in ws if (p + w) % CHUNK in todo), ws[0])
            cnt += 1
    for L in range(3, 259):  # ... and one run of every match length (every length symbol, every value of its extra bits)
        while p % BLOCK < row + 1 or p % BLOCK + L + 1 > BLOCK:
            p += 1
        mask[p:p + L] = False
        p += L + 1 + L % 3
    p += 1
    return mask[:(p + row - 1) // row * row]


def ladder(row, n=None):
    return from_mask(ladder_mask(row), row, 1000 + row, n)


def promised_runs(mask, row):
    """{(L, start mod 68)} of the maximal runs of clear bytes of a mask (what ``ladder`` promises, from its mask alone)"""
    eq = ~np.asarray(mask, bool)
    d = np.diff(np.concatenate(([0], eq.astype(np.int8), [0])))
    s, e = np.flatnonzero(d == 1), np.flatnonzero(d == -1)
    return set(zip((e - s).tolist(), (s % CHUNK).tolist())), s, e


def edges_mask(row):
    """block-boundary runs: one run over three whole blocks (from the middle of block 0 into block 4), one that ends on the last
    byte of block 4, one that starts at byte ``row`` of block 5, no equal byte in block 6, a short mixed block 7"""
    rng = np.random.default_rng(77)
    total = (7 * BLOCK + 5000 + row - 1) // row * row
    mask = rng.random(total) < 0.3
    mask[BLOCK // 2:4 * BLOCK + BLOCK // 3] = False
    mask[4 * BLOCK + BLOCK // 3:5 * BLOCK - 1000] = True
    mask[5 * BLOCK - 1000:5 * BLOCK] = False
    mask[5 * BLOCK - 1001] = True
    mask[5 * BLOCK:5 * BLOCK + row] = True
    mask[5 * BLOCK + row:5 * BLOCK + row + 700] = False
    mask[5 * BLOCK + row + 700] = True
    mask[6 * BLOCK - 300:7 * BLOCK + row] = True
    return mask


def edges(row, n=None):
    return from_mask(edges_mask(row), row, 2000 + row, n)


SKEW_VALUES = [0x10 + 7 * j for j in range(10)]  # ten literals, counts 300 * 2^j


def skewed_block_bytes(counts, seed):
    """bytes with the given counts of SKEW_VALUES, all of them LITERALS at row width 1: the most frequent value before every
    other byte — twice where it has more than the others together (two equal bytes are a run of one: a literal) — and no
    other two equal neighbours"""
    rng = np.random.default_rng(seed)
    others = np.repeat(np.array(SKEW_VALUES[:-1], np.uint8), counts[:-1])
    rng.shuffle(others)
    extra = counts[-1] - len(others)
    assert 0 <= extra <= len(others)
    rep = np.full(len(others), 2)
    rep[:extra] = 3
    rng.shuffle(rep)
    out = np.full(int(rep.sum()), SKEW_VALUES[-1], np.uint8)
    out[np.cumsum(rep) - 1] = others
    return out


def skewed(row=1):
    """306 900 bytes (5 blocks, all sampled) of ten literals with counts 300 * 2^j: the file's counts have an unlimited Huffman
    depth of 19"""
    assert row == 1
    return skewed_block_bytes([300 << j for j in range(10)], 3)


SEGMENT_ROWS = [1] * 300 + [2, 3, 5, 15, 16, 17, 100, 1, 4000, 1, 1, 70001]


def many_segments(n):
    """(rows per contig) for N = 8 or 24: one pattern of runs and unequal bytes cut into SEGMENT_ROWS contigs, so that runs
    and matches cross the contigs' boundaries; no byte has its high bit, so none equals the poison 0xA5"""
    row = row_bytes(n)
    total = sum(SEGMENT_ROWS) * row
    rng = np.random.default_rng(5 + n)
    mask = np.ones(total, bool)
    p = row
    while p < total:  # runs of 1..700 clear bytes between 1..4 set ones; short ones first, over the one-row contigs
        L = int(rng.integers(1, 12 if p < 400 * row else 700))
        mask[p:p + L] = False
        p += L + int(rng.integers(1, 5))
    b = from_mask(mask, row, 9 + n, n, bits=7)
    assert not (b == POISON).any()
    rows = b.reshape(-1, row)
    at = np.cumsum([0] + SEGMENT_ROWS)
    return [rows[at[i]:at[i + 1]] for i in range(len(SEGMENT_ROWS))]


def background_blocks(nblocks, seed=11):
    """``nblocks`` blocks of skewed-like bytes at row width 1: every block the same counts 63 * 2^j of nine literals and the
    tenth for the rest, in an order of its own"""
    counts = [63 << j for j in range(9)]
    counts.append(BLOCK - sum(counts))
    base = skewed_block_bytes(counts, seed)
    assert len(base) == BLOCK
    out = np.tile(base, nblocks)
    rng = np.random.default_rng(seed)
    for i in range(nblocks):  # (a rotation keeps the counts and, away from the seam, the literals)
        out[i * BLOCK:(i + 1) * BLOCK] = np.roll(base, int(rng.integers(0, BLOCK // 3)) * 3)
    return out


def unsampled(nblocks):
    return sorted(set(range(nblocks)) - set(sample_blocks(nblocks)))


def fit_block(ll_lens, d_lens, hdr_bits, target, seed):
    """a block of 65280 bytes (row width 1) whose dynamic form takes exactly ``target`` bytes under the given code: literals
    with long codes up to some byte, then the two literals with the shortest codes in turn; the last long one is exchanged
    for a literal whose code length trims the remainder"""
    rng = np.random.default_rng(seed)
    ll = np.asarray(ll_lens[:256])
    order = np.argsort(ll, kind="stable")
    a, b = int(order[0]), int(order[1])
    rare = np.flatnonzero(ll >= 9)
    assert len(rare) >= 16
    prefix = rng.choice(rare, BLOCK).astype(np.uint8)
    prefix[1:][prefix[1:] == prefix[:-1]] ^= 1  # (no two equal neighbours; a value next to a rare one is rare or not: the model counts)
    pad = np.where(np.arange(BLOCK) % 2 == 0, a, b).astype(np.uint8)

    def make(k, v=None):
        blk = np.concatenate((prefix[:k], pad[k:]))
        if v is not None:
            blk[k - 1] = v
        return blk

    def size(blk):
        return sbytes(hist(blk, 1), ll_lens, 1, d_lens, hdr_bits)

    lo, hi = 1, BLOCK
    assert size(make(lo)) < target <= size(make(hi)), (size(make(lo)), target, size(make(hi)))
    while hi - lo > 1:  # smallest k with size >= target (the size grows with k: a long code replaces a short one)
        mid = (lo + hi) // 2
        if size(make(mid)) >= target:
            hi = mid
        else:
            lo = mid
    for k in (hi, hi - 1, hi + 1):
        for v in [None] + [int(x) for x in order]:
            blk = make(k, v)
            if size(blk) == target:
                return blk
    raise AssertionError(f"no block of {target} bytes found")
