"""A DEFLATE (RFC 1951) writer and reader for tests: streams built symbol by symbol, including the parts of the format that
zlib's encoder never writes (long codes, incomplete codes, code-length repeats across the two alphabets, forced length
symbols, stored blocks at any bit offset), wrapped in BGZF members with any gzip extra subfields.  What the GPU inflate
(k_bgzf_inflate) is tested against.  Written from the specification, not from the product's code; zlib is the judge of
every stream (tests/test_inflate_craft_cpu.py).

* ``BitWriter``: LSB-first bits; Huffman codes go in MSB-first (RFC 1951 3.1.1)
* ``canonical``: the codes of given code lengths (RFC 1951 3.2.2); ``huffman_lengths``: length-limited Huffman (package-merge)
* tokens: an int 0..255 is a literal; ``("m", length, dist[, lsym])`` a match (``lsym`` forces the length symbol, e.g. 284
  with extra bits 31 for 258); ``("ll", sym, extra, nextra)`` / ``("d", sym, extra, nextra)`` raw symbols of either code
* code-length tokens: ``(sym, extra)`` with sym 0..18; 16 / 17 / 18 carry 2 / 3 / 7 extra bits
* ``stored_block`` / ``fixed_block`` / ``dynamic_block``; ``bgzf_member`` with extra subfields before or after BC
* ``Inflater``: a plain bit-by-bit decoder that reports each block (type, HLIT / HDIST / HCLEN, code lengths, the longest
  codes its symbols really used)
* ``recipes_valid`` / ``recipes_invalid``: the crafted streams; ``mutants``: the mutation sweep and zlib's verdict on it"""
import os
import struct
import zlib
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145,
             8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0] + [i // 2 for i in range(2, 28)]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
CL_EXTRA = {16: 2, 17: 3, 18: 7}
FIXED_LL = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_D = [5] * 32
EOF_MEMBER = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


class BitWriter:
    def __init__(self):
        self.v, self.n = 0, 0

    def put(self, val: int, n: int) -> "BitWriter":  # LSB first
        assert 0 <= val < (1 << n) or n == 0 and val == 0, (val, n)
        self.v |= val << self.n
        self.n += n
        return self

    def huff(self, code: int, n: int) -> "BitWriter":  # MSB first
        return self.put(int(f"{code:0{n}b}"[::-1], 2) if n else 0, n)

    def align(self) -> "BitWriter":
        self.n = (self.n + 7) // 8 * 8
        return self

    def raw(self, data: bytes) -> "BitWriter":
        assert self.n % 8 == 0
        return self.put(int.from_bytes(data, "little"), 8 * len(data)) if data else self

    def getvalue(self) -> bytes:
        return self.v.to_bytes((self.n + 7) // 8, "little")


def canonical(lengths: Sequence[int]) -> List[Optional[Tuple[int, int]]]:
    """(code, length) per symbol, None where the length is 0 (RFC 1951 3.2.2).  Over-subscribed lengths still get codes
    (of the overflowed values); nothing checks them here: the caller writes what it asks for."""
    bl = [0] * 16
    for L in lengths:
        bl[L] += 1
    bl[0] = 0
    code, nxt = 0, [0] * 16
    for b in range(1, 16):
        code = (code + bl[b - 1]) << 1
        nxt[b] = code
    out: List[Optional[Tuple[int, int]]] = []
    for L in lengths:
        if L:
            out.append((nxt[L], L))
            nxt[L] += 1
        else:
            out.append(None)
    return out


def kraft(lengths: Sequence[int]) -> int:
    """sum of 2^(15 - L) over the nonzero lengths: 2^15 for a complete code"""
    return sum(1 << (15 - L) for L in lengths if L)


def huffman_lengths(freqs: Sequence[int], maxbits: int = 15) -> List[int]:
    """length-limited Huffman code lengths (package-merge); one used symbol gets length 1"""
    used = [(f, s) for s, f in enumerate(freqs) if f > 0]
    lens = [0] * len(freqs)
    if not used:
        return lens
    if len(used) == 1:
        lens[used[0][1]] = 1
        return lens
    assert len(used) <= 1 << maxbits
    leaves = sorted(((f, (s,)) for f, s in used), key=lambda x: x[0])
    cur = leaves
    for _ in range(maxbits - 1):
        pkg = [(cur[i][0] + cur[i + 1][0], cur[i][1] + cur[i + 1][1]) for i in range(0, len(cur) - 1, 2)]
        cur = sorted(leaves + pkg, key=lambda x: x[0])
    for _, ss in cur[:2 * len(used) - 2]:
        for s in ss:
            lens[s] += 1
    return lens


def skewed_lengths(n: int, symbols: Sequence[int], maxlen: int = 15) -> List[int]:
    """a complete code in which symbols[i] has length i + 1 and the last two have maxlen (len(symbols) == maxlen + 1)"""
    assert len(symbols) == maxlen + 1
    lens = [0] * n
    for i, s in enumerate(symbols):
        lens[s] = min(i + 1, maxlen)
    assert kraft(lens) == 1 << 15
    return lens


def len_symbol(length: int) -> int:
    assert 3 <= length <= 258
    if length == 258:
        return 285
    return 257 + max(i for i in range(28) if LEN_BASE[i] <= length)


def dist_symbol(dist: int) -> int:
    assert 1 <= dist <= 32768
    return max(i for i in range(30) if DIST_BASE[i] <= dist)


def symbols(tokens) -> Tuple[List[int], List[int]]:
    """(literal/length symbols, distance symbols) the tokens use, EOB not included"""
    ll, d = [], []
    for t in tokens:
        if isinstance(t, int):
            ll.append(t)
        elif t[0] == "m":
            ll.append(t[3] if len(t) > 3 else len_symbol(t[1]))
            d.append(dist_symbol(t[2]))
        elif t[0] == "ll":
            ll.append(t[1])
        elif t[0] == "d":
            d.append(t[1])
    return ll, d


def write_tokens(bw: BitWriter, tokens, ll_lens: Sequence[int], d_lens: Sequence[int], eob: bool = True) -> None:
    llc, dc = canonical(ll_lens), canonical(d_lens)

    def code(table, s):
        assert s < len(table) and table[s] is not None, f"symbol {s} has no code"
        bw.huff(*table[s])

    for t in tokens:
        if isinstance(t, int):
            code(llc, t)
        elif t[0] == "m":
            length, dist = t[1], t[2]
            ls = t[3] if len(t) > 3 else len_symbol(length)
            code(llc, ls)
            bw.put(length - LEN_BASE[ls - 257], LEN_EXTRA[ls - 257])
            ds = dist_symbol(dist)
            code(dc, ds)
            bw.put(dist - DIST_BASE[ds], DIST_EXTRA[ds])
        elif t[0] == "ll":
            code(llc, t[1])
            bw.put(t[2], t[3])
        elif t[0] == "d":
            code(dc, t[1])
            bw.put(t[2], t[3])
        elif t[0] == "bits":
            bw.put(t[1], t[2])
        else:
            raise ValueError(t)
    if eob:
        code(llc, 256)


def apply_tokens(tokens, out: Optional[bytearray] = None) -> bytearray:
    """the bytes a decoder writes for the tokens (literals and matches; raw symbols are not interpreted)"""
    out = bytearray() if out is None else out
    for t in tokens:
        if isinstance(t, int):
            out.append(t)
        elif t[0] == "m":
            length, dist = t[1], t[2]
            assert dist <= len(out), "distance past the start"
            for _ in range(length):
                out.append(out[-dist])
    return out


def stored_block(bw: BitWriter, data: bytes, final: bool, nlen: Optional[int] = None, length: Optional[int] = None) -> None:
    """a stored block; ``length`` / ``nlen`` override LEN / NLEN (default: len(data) and its complement)"""
    L = len(data) if length is None else length
    bw.put(int(final), 1).put(0, 2).align()
    bw.put(L, 16).put((L ^ 0xFFFF) if nlen is None else nlen, 16).raw(data)


def fixed_block(bw: BitWriter, tokens, final: bool, eob: bool = True) -> None:
    bw.put(int(final), 1).put(1, 2)
    write_tokens(bw, tokens, FIXED_LL, FIXED_D, eob)


def rle_lengths(lengths: Sequence[int], use16=True, use17=True, use18=True) -> List[Tuple[int, int]]:
    """code-length tokens for ``lengths`` (the two alphabets concatenated: runs cross from one into the other)"""
    out: List[Tuple[int, int]] = []
    i, n = 0, len(lengths)
    while i < n:
        v = lengths[i]
        j = i
        while j < n and lengths[j] == v:
            j += 1
        run = j - i
        if v == 0 and (use17 or use18) and run >= 3:
            while run >= 3:
                if use18 and run >= 11:
                    r = min(run, 138)
                    out.append((18, r - 11))
                elif use17:
                    r = min(run, 10)
                    out.append((17, r - 3))
                else:
                    break
                run -= r
                i += r
        elif v and use16 and run >= 4:
            out.append((v, 0))
            i += 1
            run -= 1
            while run >= 3:
                r = min(run, 6)
                out.append((16, r - 3))
                run -= r
                i += r
        for _ in range(run):
            out.append((v, 0))
            i += 1
    return out


def cl_lengths_for(cl_tokens) -> List[int]:
    """a complete code-length code over the code-length symbols the tokens use (two at least)"""
    f = [0] * 19
    for s, _ in cl_tokens:
        f[s] += 1
    if sum(1 for x in f if x) < 2:  # a complete code needs two symbols: give an unused one a length too
        f[next(s for s in (0, 8, 1) if not f[s])] = 1
    return huffman_lengths(f, 7)


def dynamic_block(bw: BitWriter, tokens, final: bool, ll_lens: Optional[Sequence[int]] = None,
                  d_lens: Optional[Sequence[int]] = None, cl_tokens=None, cl_lens: Optional[Sequence[int]] = None,
                  hlit: Optional[int] = None, hdist: Optional[int] = None, hclen: Optional[int] = None, eob: bool = True,
                  rle: bool = True) -> None:
    """a dynamic-Huffman block.  hlit / hdist / hclen are the NUMBERS of code lengths (257..286, 1..30, 4..19; written as
    that minus 257 / 1 / 4: values past the ranges make invalid headers); defaults are the shortest that hold every nonzero
    length.  ll_lens / d_lens default to Huffman codes of the tokens' symbols; cl_tokens to rle_lengths of the two."""
    ll, d = symbols(tokens)
    if ll_lens is None:
        f = [0] * 286
        for s in ll:
            f[s] += 1
        if eob:
            f[256] += 1
        ll_lens = huffman_lengths(f, 15)
    if d_lens is None:
        f = [0] * 30
        for s in d:
            f[s] += 1
        d_lens = huffman_lengths(f, 15)
    ll_lens, d_lens = list(ll_lens), list(d_lens)
    if hlit is None:
        hlit = max(257, max([i + 1 for i, L in enumerate(ll_lens) if L] + [0]))
    if hdist is None:
        hdist = max(1, max([i + 1 for i, L in enumerate(d_lens) if L] + [0]))
    ll_lens = (ll_lens + [0] * hlit)[:hlit]
    d_lens = (d_lens + [0] * hdist)[:hdist]
    if cl_tokens is None:
        cl_tokens = rle_lengths(ll_lens + d_lens) if rle else [(L, 0) for L in ll_lens + d_lens]
    if cl_lens is None:
        cl_lens = cl_lengths_for(cl_tokens)
    if hclen is None:
        hclen = max(4, max(i + 1 for i, s in enumerate(CL_ORDER) if cl_lens[s]))
    bw.put(int(final), 1).put(2, 2)
    bw.put(hlit - 257, 5).put(hdist - 1, 5).put(hclen - 4, 4)
    for i in range(hclen):
        bw.put(cl_lens[CL_ORDER[i]], 3)
    clc = canonical(cl_lens)
    for s, extra in cl_tokens:
        assert clc[s] is not None, f"code-length symbol {s} has no code"
        bw.huff(*clc[s])
        if s in CL_EXTRA:
            bw.put(extra, CL_EXTRA[s])
    write_tokens(bw, tokens, ll_lens, d_lens, eob)


def subfield(si1: bytes, si2: bytes, data: bytes) -> bytes:
    return si1 + si2 + struct.pack("<H", len(data)) + data


def bgzf_member(body: bytes, payload: bytes, before: bytes = b"", after: bytes = b"", crc: Optional[int] = None,
                isize: Optional[int] = None, bsize: Optional[int] = None) -> bytes:
    """one BGZF member around a raw deflate body; ``before`` / ``after``: whole extra subfields around BC.  crc / isize /
    bsize override the footer and BSIZE (default: those of ``payload`` and of the member's true size minus one)"""
    xlen = len(before) + 6 + len(after)
    total = 12 + xlen + len(body) + 8
    bc = subfield(b"B", b"C", struct.pack("<H", (total - 1) if bsize is None else bsize))
    hdr = b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff" + struct.pack("<H", xlen) + before + bc + after
    c = (zlib.crc32(payload) & 0xFFFFFFFF) if crc is None else crc
    n = len(payload) if isize is None else isize
    return hdr + body + struct.pack("<II", c, n)


def member_body(member: bytes) -> Tuple[bytes, int]:
    """(the raw deflate body, header length) of one BGZF member; the extra subfields walked for BC"""
    xlen = member[10] | member[11] << 8
    return member[12 + xlen:len(member) - 8], 12 + xlen


def zlib_raw(data: bytes, level: int = 6, strategy: int = zlib.Z_DEFAULT_STRATEGY, mem: int = 8) -> bytes:
    c = zlib.compressobj(level, zlib.DEFLATED, -15, mem, strategy)
    return c.compress(data) + c.flush()


def zlib_verdict(body: bytes, limit: int = 65536) -> Tuple[bool, bytes, str]:
    """(accepted, output, zlib's message): accepted when zlib reaches the end of the stream inside ``body`` with at most
    ``limit`` bytes out; the message is zlib's error text, "incomplete" or "too long" otherwise"""
    d = zlib.decompressobj(-15)
    try:
        out = d.decompress(body, limit + 1)
    except zlib.error as e:
        return False, b"", str(e).split(": ", 1)[-1]
    if len(out) > limit:
        return False, out, "too long"
    if not d.eof:
        return False, out, "incomplete"
    return True, out, ""


# --------------------------------------------------------------------------------------------------------------------
# a plain decoder: reports what each block is made of


class InflateError(Exception):
    pass


class Inflater:
    """bit-by-bit RFC 1951 decoder.  ``blocks``: one dict per block (type; for dynamic blocks hlit / hdist / hclen and the
    code lengths; max_ll / max_d: the longest codes of the symbols the block's data used)"""

    def __init__(self, data: bytes):
        self.data, self.pos = data, 0
        self.out = bytearray()
        self.blocks: List[dict] = []

    def bit(self) -> int:
        if self.pos >= 8 * len(self.data):
            raise InflateError("incomplete")
        b = (self.data[self.pos >> 3] >> (self.pos & 7)) & 1
        self.pos += 1
        return b

    def bits(self, n: int) -> int:
        v = 0
        for i in range(n):
            v |= self.bit() << i
        return v

    @staticmethod
    def table(lengths):
        return {(L, c): s for s, cl in enumerate(canonical(lengths)) if cl for c, L in [cl]}

    def sym(self, table, what: str) -> Tuple[int, int]:
        code = 0
        for L in range(1, 16):
            code = (code << 1) | self.bit()
            s = table.get((L, code))
            if s is not None:
                return s, L
        raise InflateError(what)

    def dynamic_header(self) -> dict:
        """the header of a dynamic block behind its three BFINAL / BTYPE bits: HLIT / HDIST / HCLEN and the code lengths"""
        hlit, hdist, hclen = self.bits(5) + 257, self.bits(5) + 1, self.bits(4) + 4
        cl = [0] * 19
        for i in range(hclen):
            cl[CL_ORDER[i]] = self.bits(3)
        clt = self.table(cl)
        lens: List[int] = []
        while len(lens) < hlit + hdist:
            s, _ = self.sym(clt, "invalid code lengths set")
            if s < 16:
                lens.append(s)
            elif s == 16:
                lens += [lens[-1]] * (3 + self.bits(2))
            elif s == 17:
                lens += [0] * (3 + self.bits(3))
            else:
                lens += [0] * (11 + self.bits(7))
        if len(lens) > hlit + hdist:
            raise InflateError("invalid bit length repeat")
        return dict(hlit=hlit, hdist=hdist, hclen=hclen, cl_lens=cl, ll_lens=lens[:hlit], d_lens=lens[hlit:])

    def run(self) -> bytes:
        last = 0
        while not last:
            last = self.bits(1)
            t = self.bits(2)
            blk = dict(type=("stored", "fixed", "dynamic", "reserved")[t], start_bit=self.pos - 3, max_ll=0, max_d=0)
            self.blocks.append(blk)
            if t == 3:
                raise InflateError("invalid block type")
            if t == 0:
                self.pos = (self.pos + 7) // 8 * 8
                L, NL = self.bits(16), self.bits(16)
                if L ^ 0xFFFF != NL:
                    raise InflateError("invalid stored block lengths")
                if self.pos // 8 + L > len(self.data):
                    raise InflateError("incomplete")
                self.out += self.data[self.pos // 8:self.pos // 8 + L]
                self.pos += 8 * L
                blk["len"] = L
                continue
            if t == 1:
                ll_lens, d_lens = FIXED_LL, FIXED_D
            else:
                hdr = self.dynamic_header()
                ll_lens, d_lens = hdr["ll_lens"], hdr["d_lens"]
                blk.update(hdr)
            llt, dt = self.table(ll_lens), self.table(d_lens)
            while True:
                s, L = self.sym(llt, "invalid literal/length code")
                blk["max_ll"] = max(blk["max_ll"], L)
                if s < 256:
                    self.out.append(s)
                elif s == 256:
                    break
                else:
                    if s > 285:
                        raise InflateError("invalid literal/length code")
                    length = LEN_BASE[s - 257] + self.bits(LEN_EXTRA[s - 257])
                    ds, L = self.sym(dt, "invalid distance code")
                    blk["max_d"] = max(blk["max_d"], L)
                    if ds > 29:
                        raise InflateError("invalid distance code")
                    dist = DIST_BASE[ds] + self.bits(DIST_EXTRA[ds])
                    if dist > len(self.out):
                        raise InflateError("invalid distance too far back")
                    for _ in range(length):
                        self.out.append(self.out[-dist])
        return bytes(self.out)


def longest_codes(body: bytes) -> Tuple[int, int]:
    """(longest literal/length code, longest distance code) the stream's symbols used"""
    inf = Inflater(body)
    inf.run()
    return max(b["max_ll"] for b in inf.blocks), max(b["max_d"] for b in inf.blocks)


# --------------------------------------------------------------------------------------------------------------------
# the crafted streams


def _stream(*parts) -> bytes:
    """parts: (kind, args...) blocks in order, the last one final"""
    bw = BitWriter()
    for i, (kind, *a) in enumerate(parts):
        final = i == len(parts) - 1
        if kind == "stored":
            stored_block(bw, a[0], final, *a[1:])
        elif kind == "fixed":
            fixed_block(bw, a[0], final, *a[1:])
        else:
            dynamic_block(bw, a[0], final, **(a[1] if len(a) > 1 else {}))
    return bw.getvalue()


def _payload(*parts) -> bytes:
    out = bytearray()
    for kind, *a in parts:
        if kind == "stored":
            out += a[0]
        else:
            apply_tokens(a[0], out)
    return bytes(out)


def _long_code_tokens(rng, ll_syms, d_syms):
    """tokens using every one of ll_syms (literals < 256, length symbols >= 257) and every distance symbol of d_syms"""
    lits = [s for s in ll_syms if s < 256]
    toks = [int(x) for x in rng.choice(lits, 300)]  # history for the distances
    for _ in range(3):
        for s in ll_syms:
            if s < 256:
                toks.append(s)
            elif s != 256:
                ln = LEN_BASE[s - 257] + int(rng.integers(0, 1 << LEN_EXTRA[s - 257]))
                ds = int(rng.choice(d_syms))
                toks.append(("m", ln, DIST_BASE[ds] + int(rng.integers(0, 1 << DIST_EXTRA[ds])), s))
        for ds in d_syms:
            toks.append(("m", 3, DIST_BASE[ds] + int(rng.integers(0, 1 << DIST_EXTRA[ds])), 257))
    return toks


def _all_symbols_tokens(rng, n: int):
    """random tokens over every literal, every length symbol and every distance symbol"""
    toks = [int(x) for x in rng.integers(0, 256, 33000)]
    for s in range(257, 286):
        ds = (s - 257) % 30
        toks.append(("m", LEN_BASE[s - 257], DIST_BASE[ds] + int(rng.integers(0, 1 << DIST_EXTRA[ds])), s))
    for ds in range(30):
        toks.append(("m", 3, DIST_BASE[ds] + int(rng.integers(0, 1 << DIST_EXTRA[ds])), 257))
    toks += [int(x) for x in rng.integers(0, 256, n)]
    return toks


def recipes_valid() -> Dict[str, Tuple[bytes, bytes]]:
    """name -> (raw deflate stream, the bytes it inflates to); every payload <= 65536 bytes"""
    rng = np.random.default_rng(1951)
    R: Dict[str, Tuple[bytes, bytes]] = {}

    def add(name, *parts, trailing=b""):
        R[name] = (_stream(*parts) + trailing, _payload(*parts))

    # long codes: literal/length codes of 1..15 bits, distance codes of 1..15 bits, every one used
    ll_syms = [ord(c) for c in "ETAONIRSHDLCUM"[:9]] + [256, 257, 258, 265, 270, 280, 285]
    d_syms = list(range(16))
    ll = skewed_lengths(286, ll_syms)
    dl = skewed_lengths(30, d_syms)
    toks = _long_code_tokens(rng, [s for s in ll_syms if s != 256], d_syms)
    add("long_codes_ll15_d15", ("dynamic", toks, dict(ll_lens=ll, d_lens=dl)))
    # the long codes on the other symbols: length symbols short, literals long; distance codes 9..15 on far distances
    ll_syms2 = [285, 257, 260, 256, 0, 1, 2, 3, 4, 250, 251, 252, 253, 254, 255, 127]
    d_syms2 = [0, 1, 2, 3, 4, 5, 6, 7, 22, 23, 24, 25, 26, 27, 28, 29]
    toks = [int(x) for x in rng.choice([0, 1, 2, 3, 4, 250, 251, 252, 253, 254, 255, 127], 33000)]
    toks += _long_code_tokens(rng, [s for s in ll_syms2 if s != 256], d_syms2)
    add("long_codes_far", ("dynamic", toks, dict(ll_lens=skewed_lengths(286, ll_syms2), d_lens=skewed_lengths(30, d_syms2))))
    # HLIT 286, HDIST 30, HCLEN 19, every symbol used, Huffman codes of the data (lengths to 15)
    toks = _all_symbols_tokens(rng, 200)
    add("hlit286_hdist30_hclen19", ("dynamic", toks, dict(hlit=286, hdist=30, hclen=19)))
    # HCLEN 8 (the field's value 4): code lengths from {0, 8, 7, 9, 6} only; 64 symbols of 6 bits, no distance codes
    ll6 = [6 if s < 63 or s == 256 else 0 for s in range(286)]
    toks = [int(x) for x in rng.integers(0, 63, 3000)]
    add("hclen8_six_bit_code", ("dynamic", toks, dict(ll_lens=ll6, d_lens=[0], hclen=8, hlit=257, hdist=1)))
    # code-length repeats that run from the literal/length lengths into the distance lengths: 16, 17 and 18 each
    toks = [int(x) for x in rng.integers(0, 200, 2000)] + [("m", 10, 5), ("m", 40, 300), ("m", 3, 1)]
    for sym in (16, 17, 18):
        ll_l = [0] * 286
        d_l = [0] * 30
        if sym == 16:  # the last 4 ll lengths and all 16 d lengths are 4: the 16s run across the boundary
            ll_l = [8 if s < 191 or s == 256 else 4 if s >= 282 else 0 for s in range(286)]
            d_l = [4] * 16
            assert kraft(ll_l) == kraft(d_l) == 1 << 15
            t16 = [int(x) for x in rng.integers(0, 191, 300)]
            for i, ls in enumerate([282, 283, 284, 285] * 4):
                ds = i % 16
                t16 += [("m", LEN_BASE[ls - 257] + (i % 4 if ls != 285 else 0), DIST_BASE[ds], ls), int(rng.integers(0, 191))]
            cl = rle_lengths(ll_l + d_l)
            assert any(s == 16 for s, _ in cl)
            add("repeat16_crosses", ("dynamic", t16, dict(ll_lens=ll_l, d_lens=d_l, hlit=286, hdist=16, cl_tokens=cl)))
            continue
        # zeros across the boundary: ll lengths end in zeros, the first d lengths are zero too
        ll_l = huffman_lengths([1] * 200 + [0] * 56 + [1] + [1, 1] + [0] * 27, 15)  # literals 0..199, EOB, 257, 258
        d_l = [0] * 6 + [2, 2, 2, 2]  # distance symbols 6..9: distances 9..32
        run_ll = 286 - 259  # zeros at the end of the ll lengths
        if sym == 17:
            cl = [(L, 0) for L in ll_l[:259]] + [(17, 7), (17, 7), (17, 7), (17, run_ll + 6 - 30 - 3)] + [(2, 0)] * 4
        else:
            cl = [(L, 0) for L in ll_l[:259]] + [(18, run_ll + 6 - 11)] + [(2, 0)] * 4
        assert sum(3 + e if s == 17 else 11 + e if s == 18 else 1 for s, e in cl) == 286 + 10
        t = [int(x) for x in rng.integers(0, 200, 500)] + [("m", 3, 9), ("m", 4, 20), ("m", 3, 32), ("m", 4, 13)]
        add(f"repeat{sym}_crosses", ("dynamic", t, dict(ll_lens=ll_l, d_lens=d_l, hlit=286, hdist=10, cl_tokens=cl)))
    # a repeat 17 / 18 as the very first code-length token (i == 0)
    ll_l = huffman_lengths([1 if 65 <= s < 91 or s == 256 else 0 for s in range(286)], 15)
    toks = [int(x) for x in rng.integers(65, 91, 500)]
    add("repeat18_first", ("dynamic", toks, dict(ll_lens=ll_l, d_lens=[0], hlit=257, hdist=1,
                                                 cl_tokens=[(18, 65 - 11)] + rle_lengths(ll_l[65:257]) + [(0, 0)])))
    add("repeat17_first", ("dynamic", toks, dict(ll_lens=ll_l, d_lens=[0], hlit=257, hdist=1,
                                                 cl_tokens=[(17, 7)] * 6 + [(17, 2)]
                                                 + rle_lengths(ll_l[65:257]) + [(0, 0)])))
    # one distance code of one bit (symbol 0: distance 1; symbol 5: distances 7..8), no distance codes at all
    ll_l = huffman_lengths([1] * 256 + [1, 1, 1] + [0] * 27, 15)
    toks = [int(x) for x in rng.integers(0, 256, 800)]
    t1 = toks[:100] + [("m", 3, 1), ("m", 4, 1)] + toks[100:] + [("m", 4, 1)]
    add("one_distance_code_dist1", ("dynamic", t1, dict(ll_lens=ll_l, d_lens=[1], hdist=1)))
    t5 = toks[:100] + [("m", 3, 7), ("m", 4, 8)] + toks[100:] + [("m", 4, 8)]
    add("one_distance_code_sym5", ("dynamic", t5, dict(ll_lens=ll_l, d_lens=[0] * 5 + [1], hdist=6)))
    add("no_distance_codes", ("dynamic", toks, dict(ll_lens=huffman_lengths([1] * 257, 15), d_lens=[0], hdist=1)))
    add("no_distance_codes_hdist30", ("dynamic", toks, dict(ll_lens=huffman_lengths([1] * 257, 15), d_lens=[0] * 30)))
    # a literal/length code that holds only end-of-block (one code of one bit), then data in another block
    eob_only = [0] * 256 + [1]
    add("eob_only_then_data", ("dynamic", [], dict(ll_lens=eob_only, d_lens=[0])), ("fixed", toks[:50]))
    add("eob_only_empty", ("dynamic", [], dict(ll_lens=eob_only, d_lens=[0])))
    # length 258 as symbol 285 and as 284 + 31; distances 1 and 32768
    big = bytes(rng.integers(0, 256, 32768, dtype=np.uint8))
    add("len258_both_dist_extremes", ("stored", big),
        ("fixed", [("m", 258, 32768, 285), ("m", 258, 32768, 284), ("m", 258, 1), ("m", 258, 1, 284), 7,
                   ("m", 258, 32768), ("m", 3, 32768), ("m", 257, 1, 284)]))
    add("len258_dynamic", ("stored", big), ("dynamic", [("m", 258, 32768, 285), ("m", 258, 32767, 284), ("m", 258, 1, 284),
                                                         ("m", 258, 1, 285), ("m", 227, 2, 284)]))
    # dist < len for every dist 2..70: a periodic copy
    t = []
    for d in range(2, 71):
        t += [int(x) for x in rng.integers(0, 256, d)] + [("m", int(rng.integers(d + 1, 259)), d), ("m", 258, d)]
    add("overlap_dist2_70", ("fixed", t))
    add("overlap_dist2_70_dynamic", ("dynamic", t))
    # dist == pos: the copy starts at the first byte
    add("dist_equals_pos", ("fixed", [1, 2, 3, 4, 5, ("m", 10, 5), ("m", 258, 15)]))
    # several blocks of mixed types in one member, then bytes after the final block
    parts = [("stored", b"stored one "), ("fixed", [ord(c) for c in "fixed one "] + [("m", 9, 10)]),
             ("dynamic", [int(x) for x in rng.integers(0, 8, 400)] + [("m", 100, 37)]), ("stored", b""),
             ("fixed", []), ("dynamic", [("m", 258, 500)]), ("stored", bytes(range(256)))]
    add("mixed_blocks", *parts)
    add("trailing_bytes", *parts, trailing=b"\x00junk after the final block\xff")
    # ISIZE at the edges: empty, 1, the 68-byte CRC chunk, 64 chunks, the whole LDS buffer
    for n in (0, 1, 67, 68, 69, 4351, 4352, 4353, 65535, 65536):
        data = bytes(rng.integers(0, 4, n, dtype=np.uint8))
        add(f"isize{n}_dynamic", ("dynamic", [int(x) for x in data]))
        if n <= 65000:
            add(f"isize{n}_stored", ("stored", data))
        else:  # (a member holds at most 64 KiB: the last bytes Huffman-coded behind the stored run)
            add(f"isize{n}_stored", ("stored", data[:n - 600]), ("dynamic", [int(x) for x in data[n - 600:]]))
    return R


def recipes_stored_offsets() -> Dict[str, Tuple[bytes, bytes]]:
    """stored blocks that start at every bit offset 0..7, of lengths 0..12, 63..65 and longer, each followed by a match
    back into it (the reader realigned behind the run)"""
    rng = np.random.default_rng(1952)
    R = {}
    for off in range(8):
        for L in list(range(13)) + [63, 64, 65, 1000, 65535 - 300]:
            data = bytes(rng.integers(0, 256, L, dtype=np.uint8))
            # fixed block: 3 + 7 (EOB) bits + 8 per literal < 144 + 9 per literal >= 144: start at bit 10 + 8a + 9b
            b = (off - 2) % 8
            lead = [int(x) for x in rng.integers(144, 256, b)] + [int(x) for x in rng.integers(0, 144, 3)]
            back = ("m", max(3, min(L, 258)), max(1, min(L, 32768)))
            parts = [("fixed", lead), ("stored", data), ("fixed", [("m", 3, 3), 65, back])] \
                if off else [("stored", data), ("fixed", [0, 1, ("m", 3, 2)])]
            body = _stream(*parts)
            if off:
                assert (10 + 8 * 3 + 9 * b) % 8 == off
            R[f"stored_off{off}_len{L}"] = (body, _payload(*parts))
    return R


def recipes_invalid() -> Dict[str, Tuple[bytes, bytes, str, str]]:
    """name -> (raw deflate stream, the payload its footer declares, zlib's verdict, the reason the GPU inflate gives).
    zlib's verdict is its error text, "incomplete" (no end of stream inside the body) or "" (zlib accepts the stream: the
    footer is what is wrong)"""
    rng = np.random.default_rng(1953)
    R = {}
    lits = [int(x) for x in rng.integers(0, 256, 300)]
    lit_payload = bytes(lits)
    ll_all = huffman_lengths([1] * 258 + [0] * 28, 15)  # literals, EOB, 257

    def dyn(**kw):
        bw = BitWriter()
        toks = kw.pop("tokens", lits)
        dynamic_block(bw, toks, True, **kw)
        return bw.getvalue()

    CODES, SYMBOL = "over-subscribed or incomplete Huffman code", "invalid Huffman symbol"
    # TYPE, STORED
    R["type3"] = (BitWriter().put(1, 1).put(3, 2).put(0, 29).getvalue(), b"x", "invalid block type", "reserved block type")
    bw = BitWriter()
    stored_block(bw, b"abcdef", True, nlen=0xFFFF ^ 6 ^ 0x100)
    R["stored_nlen"] = (bw.getvalue(), b"abcdef", "invalid stored block lengths", "stored block LEN / NLEN mismatch")
    # CODES, each cause
    R["hlit287"] = (dyn(ll_lens=ll_all, hlit=287), lit_payload, "too many length or distance symbols", CODES)
    R["hlit288"] = (dyn(ll_lens=ll_all, hlit=288), lit_payload, "too many length or distance symbols", CODES)
    R["hdist31"] = (dyn(ll_lens=ll_all, hdist=31), lit_payload, "too many length or distance symbols", CODES)
    R["hdist32"] = (dyn(ll_lens=ll_all, hdist=32), lit_payload, "too many length or distance symbols", CODES)
    cl_over = [0] * 19
    for s in (0, 8, 9, 1, 2):  # five codes of 2 bits
        cl_over[s] = 2
    R["cl_oversubscribed"] = (dyn(ll_lens=ll_all, cl_lens=cl_over, rle=False), lit_payload, "invalid code lengths set", CODES)
    cl_inc = [0] * 19
    for s in (0, 8, 9):  # three codes of 2 bits
        cl_inc[s] = 2
    R["cl_incomplete"] = (dyn(ll_lens=[8] * 256 + [9, 9], cl_lens=cl_inc, rle=False, d_lens=[0]),
                          lit_payload, "invalid code lengths set", CODES)
    cl_one = [0] * 19
    cl_one[8] = 1  # a single code-length code of one bit: incomplete, refused for this code
    R["cl_single_code"] = (dyn(ll_lens=[8] * 256 + [8] * 30, cl_lens=cl_one, cl_tokens=[(8, 0)] * 287, d_lens=[8], hlit=286,
                               tokens=lits[:10], eob=False) + b"\x00" * 4, lit_payload[:10], "invalid code lengths set", CODES)
    ll8 = [8] * 256 + [8] * 30
    R["repeat16_first"] = (dyn(ll_lens=ll8, d_lens=[0], hlit=286, cl_tokens=[(16, 0)] + [(8, 0)] * 285 + [(0, 0)]),
                           lit_payload, "invalid bit length repeat", CODES)
    for sym, e in ((16, 3), (17, 7), (18, 127)):
        # the repeat runs past HLIT + HDIST: 284 lengths of 8, then the repeat (6 / 10 / 138 more) with 3 left
        cl = [(8, 0)] * 284 + [(sym, e)] + [(8, 0)] * 3
        R[f"repeat{sym}_too_long"] = (dyn(ll_lens=ll8, d_lens=[0], hlit=286, cl_tokens=cl, hdist=1) + b"\x00" * 4,
                                      lit_payload, "invalid bit length repeat", CODES)
    no_eob = [8] * 256 + [0] + [8] * 29
    R["missing_eob"] = (dyn(ll_lens=no_eob, d_lens=[0], hlit=286, eob=False) + b"\x00" * 64, lit_payload,
                        "invalid code -- missing end-of-block", CODES)
    cl4 = [0] * 19
    for s in (16, 17, 18, 0):
        cl4[s] = 2
    R["hclen4_all_zero"] = (dyn(ll_lens=[0] * 257, d_lens=[0], hclen=4, cl_lens=cl4, cl_tokens=[(18, 127), (18, 109)],
                                hlit=257, eob=False, tokens=[]) + b"\x00" * 8, b"",
                            "invalid code -- missing end-of-block", CODES)
    R["ll_oversubscribed"] = (dyn(ll_lens=[8] * 256 + [8, 8], d_lens=[0], tokens=lits), lit_payload,
                              "invalid literal/lengths set", CODES)
    R["ll_incomplete"] = (dyn(ll_lens=[9] * 256 + [2], d_lens=[0], tokens=lits), lit_payload, "invalid literal/lengths set",
                          CODES)
    t_d = lits + [("m", 3, 2)]
    p_d = bytes(apply_tokens(t_d))
    R["d_oversubscribed"] = (dyn(ll_lens=ll_all, d_lens=[1, 1, 1], tokens=t_d), p_d, "invalid distances set", CODES)
    R["d_incomplete"] = (dyn(ll_lens=ll_all, d_lens=[1, 2], tokens=t_d), p_d, "invalid distances set", CODES)
    # SYMBOL
    for s in (286, 287):
        bw = BitWriter()
        fixed_block(bw, lits[:20] + [("ll", s, 0, 0)], True)
        R[f"fixed_ll{s}"] = (bw.getvalue(), lit_payload[:20], "invalid literal/length code", SYMBOL)
    for ds in (30, 31):
        bw = BitWriter()
        fixed_block(bw, lits[:20] + [("ll", 257, 0, 0), ("d", ds, 0, 0)], True)
        R[f"fixed_d{ds}"] = (bw.getvalue(), lit_payload[:20] + b"xyz", "invalid distance code", SYMBOL)
    bw = BitWriter()  # only EOB has a code ("0"): the unused code "1"
    dynamic_block(bw, [], False, ll_lens=[0] * 256 + [1], d_lens=[0], eob=False)
    bw.put(1, 1).put(0, 16)
    R["ll_unused_code"] = (bw.getvalue(), b"", "invalid literal/length code", SYMBOL)
    bw = BitWriter()  # one distance code "0": the unused code "1"
    dynamic_block(bw, lits[:30] + [("ll", 257, 0, 0), ("bits", 1, 1)], True, ll_lens=ll_all, d_lens=[1])
    R["d_unused_code"] = (bw.getvalue(), lit_payload[:33], "invalid distance code", SYMBOL)
    bw = BitWriter()  # no distance codes at all, and a length symbol
    dynamic_block(bw, lits[:30] + [("ll", 257, 0, 0), ("bits", 0, 1)], True, ll_lens=ll_all, d_lens=[0])
    R["d_none_used"] = (bw.getvalue(), lit_payload[:33], "invalid distance code", SYMBOL)
    # DISTANCE: dist == pos + 1 (dist == pos is a valid recipe)
    bw = BitWriter()
    fixed_block(bw, [1, 2, 3, 4, 5, ("ll", 257, 0, 0), ("d", 4, 1, 1)], True)
    R["dist_pos_plus_1"] = (bw.getvalue(), b"\x01\x02\x03\x04\x05" * 2, "invalid distance too far back",
                            "distance reaches back past the start of the output")
    bw = BitWriter()
    dynamic_block(bw, lits + [("ll", 285, 0, 0), ("d", 29, 32768 - 24577, 13)], True,
                  ll_lens=huffman_lengths([1] * 257 + [0] * 28 + [1], 15), d_lens=[1] + [0] * 28 + [1])
    R["dist_32768_too_far"] = (bw.getvalue(), lit_payload + b"\x00" * 258, "invalid distance too far back",
                               "distance reaches back past the start of the output")
    # OVERRUN: zlib takes the stream; the footer declares one byte less than it holds
    OVR = "output overruns ISIZE"
    bw = BitWriter()
    fixed_block(bw, lits[:40], True)
    R["overrun_literal"] = (bw.getvalue(), lit_payload[:39], "", OVR)
    bw = BitWriter()
    fixed_block(bw, lits[:40] + [("m", 100, 40)], True)
    R["overrun_match"] = (bw.getvalue(), bytes(apply_tokens(lits[:40] + [("m", 99, 40)])), "", OVR)
    bw = BitWriter()
    stored_block(bw, lit_payload[:100], True)
    R["overrun_stored"] = (bw.getvalue(), lit_payload[:99], "", OVR)
    # INPUT: truncated inside the Huffman data (the cut symbol decodes as a literal from the footer bits) / a stored run
    INP = "deflate data overruns BSIZE"
    bw = BitWriter()
    fixed_block(bw, [ord("A")] * 200, True)
    R["truncated_huffman"] = (bw.getvalue()[:120], b"A" * 200, "incomplete", INP)
    bw = BitWriter()
    stored_block(bw, lit_payload[:200], True)
    R["truncated_stored"] = (bw.getvalue()[:150], lit_payload[:200], "incomplete", INP)
    bw = BitWriter()
    stored_block(bw, lit_payload[:100], False)
    R["truncated_no_final"] = (bw.getvalue(), lit_payload[:100] + b"more", "incomplete", INP)
    R["truncated_dynamic_header"] = (dyn(ll_lens=ll_all)[:3], lit_payload, "incomplete", INP)
    R["truncated_code_lengths"] = (dyn(ll_lens=ll_all)[:30], lit_payload, "incomplete", INP)
    return R


# --------------------------------------------------------------------------------------------------------------------
# the mutation sweep


def base_streams() -> List[Tuple[str, bytes]]:
    """small raw deflate streams (payloads <= 8 KB) from zlib at several levels / strategies, libdeflate (the committed
    fixture) and the crafted writer"""
    rng = np.random.default_rng(2024)
    pays = [bytes(rng.integers(0, 256, 700, dtype=np.uint8)),
            bytes(np.repeat(rng.integers(0, 4, 300, dtype=np.uint8), rng.integers(1, 30, 300))[:8000]),
            np.repeat(rng.integers(0, 256, (30, 9), dtype=np.uint8), rng.integers(1, 20, 30), axis=0).tobytes(),
            b"ACGT" * 500 + b"N" * 300]
    out = []
    for i, p in enumerate(pays):
        for level in (0, 1, 6, 9):
            out.append((f"zlib{level}_{i}", zlib_raw(p, level)))
        for strat in (zlib.Z_FIXED, zlib.Z_HUFFMAN_ONLY, zlib.Z_RLE):
            out.append((f"zlib_s{strat}_{i}", zlib_raw(p, 6, strat)))
    fx = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "inflate", "libdeflate_blocks.npz")
    z = np.load(fx)
    offs = z["body_offsets"]
    for j in range(len(offs) - 1):
        if z["isize"][j] <= 8192:
            out.append((f"libdeflate_{j}", z["bodies"][offs[j]:offs[j + 1]].tobytes()))
    for name, (body, payload) in sorted(recipes_valid().items()):
        if len(payload) <= 8192 and len(body) > 2:
            out.append((f"craft_{name}", body))
    return out


def mutate(body: bytes, rng) -> bytes:
    """one mutant of a raw deflate body: 1..3 bits flipped, a byte overwritten, 1..16 bytes cut off, or junk appended"""
    b = bytearray(body)
    kind = int(rng.integers(0, 4))
    if kind == 0:
        for _ in range(int(rng.integers(1, 4))):
            i = int(rng.integers(0, 8 * len(b)))
            b[i >> 3] ^= 1 << (i & 7)
    elif kind == 1:
        b[int(rng.integers(0, len(b)))] = int(rng.integers(0, 256))
    elif kind == 2:
        b = b[:max(1, len(b) - int(rng.integers(1, 17)))]
    else:
        b += bytes(rng.integers(0, 256, int(rng.integers(1, 17)), dtype=np.uint8))
    return bytes(b)


def fuzz_count(default: int = 3000) -> int:
    return int(os.environ.get("PG_FUZZ_SEEDS", default))


def mutants(n: Optional[int] = None):
    """[(seed, base name, mutant body, accepted, zlib's output)] for seeds 0..n-1 (n from PG_FUZZ_SEEDS, default 3000)"""
    n = fuzz_count() if n is None else n
    bases = base_streams()
    out = []
    for seed in range(n):
        rng = np.random.default_rng([seed, 1951])
        name, body = bases[int(rng.integers(0, len(bases)))]
        m = mutate(body, rng)
        ok, data, _ = zlib_verdict(m)
        out.append((seed, name, m, ok, data))
    return out
