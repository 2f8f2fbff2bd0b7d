"""FASTQ texts crafted for the edges of pg_fastq.hip (k_fastq_scan, k_fastq_offsets, k_fastq_join): a byte pair split between two
lanes' 16-byte loads or between two tiles, tiles that start on a line in every line class, tiles behind the last complete record,
lengths that fill the last lane or tile, tile counts around the 256 threads of k_fastq_offsets, and malformed lines at all of
these.  No tests in here: tests/test_fastq_craft_cpu.py proves from offsets that every text holds the edge it claims,
tests/test_gpu_fastq_edges.py holds the kernels to the models on them.

Two models: place_ref.fastq_model / fastq_malformed (Python's split) and ``walk`` below (one pass, byte by byte, with a line
counter — the header comment of pg_fastq.hip restated).  A case is ``Case(text, claim)``; ``claim`` is what the builder meant the
text to hold, for the CPU test to check against a survey of the text itself (``line_starts``, ``tile_starts``, ``tile_of_line``).

  well_formed()  {name: Case}  accepted texts: slide, phases, lengths, torn_tail, tile_counts, hidden (malformed lines only
                               behind line 4 * nreads)
  malformed()    {name: Case}  refused texts; claim["first"] = (record, kind) of the line that has to be reported
  batch_text()                 the CRLF text tests stream through place.FastqBatches in batches of BATCH_SIZES"""
import collections
import functools

import numpy as np

from tests.place_ref import FASTQ_TILE, as_packed, fastq_malformed, fastq_model, fastq_text, rand  # noqa: F401 (re-exported)

T = FASTQ_TILE
LF, CRLF = b"\n", b"\r\n"
EOLS = {"lf": LF, "crlf": CRLF}
NTHREADS = 256  # of k_fastq_offsets' one block
FEATURES = tuple(f"{kind}{line}" for kind in ("first", "lf", "cr") for line in range(4))
SLIDE_OFFSETS = (T - 1, T, T + 1, T + 15, T + 16, T + 17)
LENGTHS = (T, 2 * T, T - 16, T + 16, 16, 15)
# tiles: bytes, line end.  255: the last tile full; 256: its only byte the last line feed; 257 / 513: a last tile with lines to break
TILE_COUNTS = {255: (255 * T, CRLF), 256: (255 * T + 1, LF), 257: (256 * T + 1000, LF), 512: (512 * T - 16, LF),
               513: (512 * T + 2000, CRLF)}
BATCH_SIZES = (T - 1, T, T + 1, 3 * T + 5)

Case = collections.namedtuple("Case", "text claim")


# ---------------------------------------------------------------------------
# the second model, and the survey of a text
# ---------------------------------------------------------------------------
def _walk(text):
    out, seq = bytearray(), bytearray()
    line = nreads = consumed = 0
    start, pending, first_bad = True, None, None
    for i, c in enumerate(text):
        cls = line & 3
        if start:  # the first byte of line `line` (an empty line's is its line feed: neither '@' nor '+')
            start = False
            if pending is None:
                if cls == 0 and c != 0x40:
                    pending = (line >> 2, "header")
                elif cls == 2 and c != 0x2B:
                    pending = (line >> 2, "separator")
        if c == 0x0A:
            if cls == 1:
                if seq and seq[-1] == 0x0D:  # the '\r' right before the line feed
                    del seq[-1]
            elif cls == 3:  # the record is complete: only now do its bytes and its malformed line count
                if nreads:
                    out.append(0x4E)
                out += seq
                del seq[:]
                nreads += 1
                consumed = i + 1
                if first_bad is None:
                    first_bad = pending
                pending = None
            line += 1
            start = True
        elif cls == 1:
            seq.append(c)
    return bytes(out), nreads, consumed, first_bad


_walk_cached = functools.lru_cache(maxsize=None)(_walk)


def walk(text):
    """(joined, nreads, consumed, first_bad) in one pass over the bytes with a line counter; first_bad = None or (record, "header" |
    "separator") of the malformed line with the lowest number below 4 * nreads"""
    return _walk_cached(bytes(text))


def ntiles(text):
    return -(-len(text) // T)


def _lfs(text):
    return np.flatnonzero(np.frombuffer(bytes(text), np.uint8) == 0x0A)


def line_starts(text):
    """the offset of the first byte of every line that has one, by line number"""
    s = np.concatenate(([0], _lfs(text) + 1))
    return s[s < len(text)]


def line_at(text, offset):
    """the line number of the byte at ``offset``: the line feeds before it"""
    return int(np.searchsorted(_lfs(text), offset, side="left"))


def tile_starts(text):
    """per tile (line number of its first byte, whether that byte is the first of a line)"""
    text = bytes(text)
    return [(line_at(text, k * T), k == 0 or text[k * T - 1] == 0x0A) for k in range(ntiles(text))]


def tile_of_line(text, line):
    return int(line_starts(text)[line]) // T


def per_thread(nt):
    """the tiles each thread of k_fastq_offsets takes: thread i owns [i * per, (i + 1) * per)"""
    return -(-nt // NTHREADS)


def owner(nt, tile):
    return tile // per_thread(nt)


def malformed_lines(text):
    """the numbers of the malformed lines below line 4 * nreads, from the lines' first bytes"""
    a, lfs = np.frombuffer(bytes(text), np.uint8), _lfs(text)
    starts = np.concatenate(([0], lfs + 1))[:len(lfs) // 4 * 4]
    first = a[starts]
    n = np.arange(len(starts))
    return n[((n & 3) == 0) & (first != 0x40) | ((n & 3) == 2) & (first != 0x2B)].tolist()


def broken(text, *lines):
    """``text`` with the first byte of the header / separator lines ``lines`` (by number) made wrong, nothing moved"""
    a, starts = bytearray(text), line_starts(text)
    for n in lines:
        at = int(starts[n])
        assert a[at] == {0: 0x40, 2: 0x2B}[n & 3], (n, at)
        a[at] = {0: ord("x"), 2: ord("-")}[n & 3]
    return bytes(a)


def first_line_in_tile(text, tile, cls, last=False):
    """the number of the first (last) line of class ``cls`` whose first byte lies in ``tile``"""
    starts = line_starts(text)
    hit = [n for n in range(cls, len(starts), 4) if int(starts[n]) // T == tile]
    return hit[-1 if last else 0]


def kind_of(line):
    return {0: "header", 2: "separator"}[line & 3]


# ---------------------------------------------------------------------------
# builders
# ---------------------------------------------------------------------------
def placed(feature, offset, eol=LF, record=1, reads=None, override=None, torn=None, seed=0):
    """(text, offsets): records of ``reads`` in which ``feature`` of record ``record`` — first0..3 the first byte of its four
    lines, lf0..3 their line feeds, cr0..3 the '\\r' before them (eol == CRLF) — lies at the absolute ``offset``, by padding record
    0's name.  override[(record, line)] replaces a line's bytes (without its line end); torn = (k, m) keeps of the last record k
    whole lines and m bytes of the next.  offsets: where each feature of ``record`` lies, as far as the text reaches."""
    rng = np.random.default_rng(seed)
    if reads is None:
        reads = [rand(rng, 60), rand(rng, 70), rand(rng, T // 2), rand(rng, 50)]
    e = len(eol)

    def build(pad):
        lines = []
        for i, r in enumerate(reads):
            rec = [b"@r%d" % i, bytes(r), b"+", b"I" * len(r)]
            for l in range(4):
                if override and (i, l) in override:
                    rec[l] = override[(i, l)]
            if i == 0:
                rec[0] += b"p" * pad
            lines += rec
        starts = np.concatenate(([0], np.cumsum([len(x) + e for x in lines]))).tolist()
        feats = {}
        for l in range(4):
            s = starts[4 * record + l]
            feats[f"first{l}"] = s
            feats[f"lf{l}"] = s + len(lines[4 * record + l]) + e - 1
            if eol == CRLF:
                feats[f"cr{l}"] = feats[f"lf{l}"] - 1
        text = eol.join(lines) + eol
        if torn is not None:
            k, m = torn
            n = 4 * (len(reads) - 1) + k
            if not 0 <= m < len(lines[n]) + e:
                raise ValueError(f"placed: {m} bytes of a line of {len(lines[n])}")
            text = text[:starts[n] + m]
        return text, {f: o for f, o in feats.items() if o < len(text)}

    base = build(0)[1]
    if feature not in base:
        raise ValueError(f"placed: no {feature} with this line end / tear")
    pad = offset - base[feature]
    if pad < 0 or (pad and record == 0 and feature == "first0"):
        raise ValueError(f"placed: {feature} of record {record} cannot lie at {offset}")
    return build(pad)


def whole(nbytes, eol=LF, seed=0):
    """a well-formed text of exactly ``nbytes``: records of about 100 bases, the last record's quality line padded"""
    rng = np.random.default_rng(seed)
    e, parts, pos, i = len(eol), [], 0, 0
    while nbytes - pos > 600:
        rec = fastq_text([rand(rng, int(rng.integers(90, 111)))], eol, names={0: b"r%d" % i})
        parts.append(rec)
        pos += len(rec)
        i += 1
    read = rand(rng, 100) if nbytes - pos > 300 else b"A"
    stem = b"@r%d" % i + eol + read + eol + b"+" + eol
    q = nbytes - pos - len(stem) - e
    if q < 0:
        raise ValueError(f"whole: no record fits {nbytes} bytes")
    parts.append(stem + b"I" * q + eol)
    return b"".join(parts)


def phases_text(eol, seed=0):
    """(text, want): at least 9 tiles; tile k of want = {k: (line class, at line start)} starts so, k = 1..8 covering all eight"""
    rng = np.random.default_rng(seed)
    e, parts, n = len(eol), [], 0
    pos = 0

    def add(rec):
        nonlocal pos, n
        parts.append(rec)
        pos += len(rec)
        n += 1

    def filler():
        add(fastq_text([rand(rng, int(rng.integers(80, 121)))], eol, names={0: b"r%d" % n}))

    inside = {0: 3, 1: 20, 2: 1, 3: 20}  # how far into a line of the class a mid-line tile starts
    want = {}
    for k, (at_start, cls) in enumerate(((s, c) for s in (True, False) for c in range(4)), 1):
        want[k] = (cls, at_start)
        while k * T - pos > 700:
            filler()
        # a record P with a padded name, then the record R whose line `cls` starts at k T (or `inside` bytes before it)
        read = rand(rng, 60)
        r_lines = [b"@r%d" % (n + 1), read, b"+", b"I" * 60]
        before = sum(len(x) + e for x in r_lines[:cls])
        r_start = k * T - (0 if at_start else inside[cls]) - before
        p = fastq_text([rand(rng, 50)], eol, names={0: b"r%d" % n})
        pad = r_start - pos - len(p)
        assert pad >= 0, (k, pad)
        add(fastq_text([rand(rng, 50)], eol, names={0: b"r%d" % n + b"p" * pad}))
        add(eol.join(r_lines) + eol)
    while pos < 9 * T + 500:
        filler()
    return b"".join(parts), want


def torn_text(line, eol, bad=False, seed=0):
    """(text, nreads): 30 complete records, then a torn record whose line ``line`` is 3 tiles long and unfinished; bad: its header
    and separator lines would be malformed"""
    rng = np.random.default_rng(seed)
    head = fastq_text([rand(rng, int(n)) for n in rng.integers(80, 121, 30)], eol)
    long = [b"@" + b"n" * (3 * T), rand(rng, 3 * T), b"+" + b"s" * (3 * T), b"I" * (3 * T - 1) + b"\r"][line]
    short = [b"xtorn" if bad else b"@torn", rand(rng, 90), b"" if bad else b"+"]
    return head + b"".join(x + eol for x in short[:line]) + long, 30


def batch_text(seed=3):
    """about 40 KB with CRLF line ends: a read longer than 3 tiles among short ones, some of them empty"""
    rng = np.random.default_rng(seed)
    reads = [rand(rng, int(n)) for n in rng.integers(1, 200, 70)]
    for i in (0, 7, 8, 50, 69):
        reads[i] = b""
    reads[40] = rand(rng, 3 * T + 200)
    return fastq_text(reads, CRLF)


# ---------------------------------------------------------------------------
# families
# ---------------------------------------------------------------------------
def _features(eol):
    return [f for f in FEATURES if eol == CRLF or not f.startswith("cr")]


def _last_complete(rng):
    """reads for placed(): record 1 is the last complete one, record 2 is torn in its sequence line (torn=(1, T // 2))"""
    return [rand(rng, 60), rand(rng, 70), rand(rng, T // 2 + 5)]


def slide():
    """every feature of record 1 at a tile edge and at a lane edge well inside a tile, both line ends; the '\\r\\n' that ends
    ``consumed`` and that of an empty sequence line across them"""
    out = {}
    rng = np.random.default_rng(11)
    for en, eol in EOLS.items():
        for f in _features(eol):
            for off in SLIDE_OFFSETS:
                text, offs = placed(f, off, eol, seed=off)
                out[f"slide_{en}_{f}_{off}"] = Case(text, dict(family="slide", feature=f, offset=off, offsets=offs, eol=eol))
        # the last complete record's quality line: its line end is the one that ends `consumed`
        for f in ("first3", "lf3") + (("cr3",) if eol == CRLF else ()):
            for off in SLIDE_OFFSETS:
                text, offs = placed(f, off, eol, reads=_last_complete(rng), torn=(1, T // 2))
                out[f"slide_{en}_last_{f}_{off}"] = Case(text, dict(family="slide", feature=f, offset=off, offsets=offs, eol=eol,
                                                                    last=True))
    # an empty sequence line whose "\r\n" is split by the tile edge / the lane edge, in the middle and as the last complete record
    for off in (T - 1, T + 15):
        reads = [rand(rng, 60), b"", rand(rng, T // 2), rand(rng, 50)]
        text, offs = placed("cr1", off, CRLF, reads=reads)
        out[f"slide_crlf_empty_seq_{off}"] = Case(text, dict(family="slide", feature="cr1", offset=off, offsets=offs, eol=CRLF,
                                                             empty=True))
        reads = [rand(rng, 60), b"", rand(rng, T // 2 + 5)]
        text, offs = placed("cr1", off, CRLF, reads=reads, torn=(1, T // 2))
        out[f"slide_crlf_last_empty_seq_{off}"] = Case(text, dict(family="slide", feature="cr1", offset=off, offsets=offs, eol=CRLF,
                                                                  empty=True, last=True))
    return out


def phases():
    out = {}
    for en, eol in EOLS.items():
        text, want = phases_text(eol, seed=21 + len(eol))
        out[f"phases_{en}"] = Case(text, dict(family="phases", want=want, eol=eol))
    return out


def lengths():
    out = {}
    for en, eol in EOLS.items():
        for n in LENGTHS:
            out[f"length_{en}_{n}"] = Case(whole(n, eol, seed=n), dict(family="lengths", nbytes=n, eol=eol, torn=False))
    # exactly T bytes, the last one a '\r' that no line feed follows: of a torn sequence line, of a torn quality line
    rng = np.random.default_rng(31)
    reads = [rand(rng, 60), rand(rng, 70), rand(rng, 50)]
    for line in (1, 3):
        text, _ = placed(f"cr{line}", T - 1, CRLF, record=2, reads=reads, torn=(line, 51))
        out[f"length_cr_last_line{line}"] = Case(text, dict(family="lengths", nbytes=T, eol=CRLF, torn=True))
    return out


def torn_tail():
    out = {}
    for en, eol in EOLS.items():
        for line in range(4):
            text, n = torn_text(line, eol, seed=41 + line)
            out[f"torn_{en}_line{line}"] = Case(text, dict(family="torn_tail", nreads=n, line=line, hidden=False))
        text, n = torn_text(3, eol, bad=True, seed=45)
        out[f"torn_{en}_bad_tail"] = Case(text, dict(family="torn_tail", nreads=n, line=3, hidden=True))
    return out


@functools.lru_cache(maxsize=None)
def tile_counts():
    return {f"tiles_{nt}": Case(whole(nbytes, eol, seed=nt), dict(family="tile_counts", ntiles=nt, eol=eol))
            for nt, (nbytes, eol) in TILE_COUNTS.items()}


def hidden():
    """accepted: the malformed lines lie behind line 4 * nreads, the first of them at a tile's first byte / a lane's"""
    out = {}
    rng = np.random.default_rng(51)
    reads = [rand(rng, 60), rand(rng, 70), rand(rng, 80)]
    for en, eol in EOLS.items():
        for kind, f in (("header", "first0"), ("separator", "first2")):
            for off in (T - 1, T, T + 16):
                text, offs = placed(f, off, eol, record=2, reads=reads, override={(2, 0): b"xr2", (2, 2): b"-"}, torn=(3, 40))
                out[f"hidden_{en}_{kind}_{off}"] = Case(text, dict(family="hidden", feature=f, offset=off, offsets=offs, nreads=2))
    return out


@functools.lru_cache(maxsize=None)
def well_formed():
    out = {}
    for fam in (slide, phases, lengths, torn_tail, tile_counts, hidden):
        out.update(fam())
    return out


def _bad(text, first_line, **claim):
    return Case(text, dict(family="malformed", first=(first_line >> 2, kind_of(first_line)), first_line=first_line, **claim))


@functools.lru_cache(maxsize=None)
def malformed():
    out = {}
    rng = np.random.default_rng(61)
    wrong = {0: b"xr", 2: b"-"}
    # the offending first byte at a tile edge and a lane edge: of record 1 in the middle, of record 0, of the last complete record
    for en, eol in EOLS.items():
        for cls in (0, 2):
            f, kind = f"first{cls}", kind_of(cls)
            for off in (T - 1, T, T + 15, T + 16):
                text, offs = placed(f, off, eol, override={(1, cls): wrong[cls]}, seed=off)
                out[f"bad_{en}_{kind}_{off}"] = _bad(text, 4 + cls, offset=off, offsets=offs, feature=f)
                text, offs = placed(f, off, eol, reads=_last_complete(rng), override={(1, cls): wrong[cls]}, torn=(1, T // 2))
                out[f"bad_{en}_last_{kind}_{off}"] = _bad(text, 4 + cls, offset=off, offsets=offs, feature=f, last=True)
            for off in (T - 1, T, T + 16):
                text, offs = placed("first2", off, eol, record=0, override={(0, 2): b"-"}, seed=off)
                out[f"bad_{en}_record0_separator_{off}"] = _bad(text, 2, offset=off, offsets=offs, feature="first2")
        text, offs = placed("first0", 0, eol, record=0, override={(0, 0): b"xr0"})
        out[f"bad_{en}_record0_header_0"] = _bad(text, 0, offset=0, offsets=offs, feature="first0")
        # an empty header line and an empty separator line whose first byte (the lone line end) is a tile's first
        for cls in (0, 2):
            for k in (1, 2):
                reads = [rand(rng, 60), rand(rng, 70), rand(rng, T // 2), rand(rng, 50)] if k == 1 else \
                        [rand(rng, T // 2), rand(rng, 70), rand(rng, T // 2), rand(rng, 50)]
                text, offs = placed(f"first{cls}", k * T, eol, reads=reads, override={(1, cls): b""})
                out[f"bad_{en}_empty_{kind_of(cls)}_{k}T"] = _bad(text, 4 + cls, offset=k * T, offsets=offs, feature=f"first{cls}",
                                                                   empty=True)
    # the phases texts with one line broken in each of the tiles 1..8: the line at the tile's first byte where it is a header or a
    # separator, else the tile's first header (odd tiles) or separator (even tiles)
    for name, case in phases().items():
        for k, (cls, at_start) in case.claim["want"].items():
            if at_start and cls in (0, 2):
                line = line_at(case.text, k * T)
            else:
                line = first_line_in_tile(case.text, k, 0 if k & 1 else 2)
            out[f"bad_{name}_tile{k}"] = _bad(broken(case.text, line), line, tile=k, phase=cls, at_start=at_start)
    # k_fastq_offsets' threads with several tiles each: one broken line in tile 0, in the last tile, in the last tile of a thread's
    # range and in the first of the next thread's; two in one thread's range; pairs in two threads' ranges, the later line the
    # only one of its kind
    for nt, thread, far in ((257, 57, ((20, 120), (100, 128))), (513, 149, ((20, 160), (130, 170)))):
        text = tile_counts()[f"tiles_{nt}"].text
        per = per_thread(nt)
        spots = {"tile0": 0, "last_tile": nt - 1, "range_end": thread * per + per - 1, "next_range": (thread + 1) * per}
        for i, (spot, tile) in enumerate(spots.items()):
            line = first_line_in_tile(text, tile, (0, 2)[i & 1], last=spot == "last_tile")
            out[f"bad_tiles_{nt}_{spot}"] = _bad(broken(text, line), line, tile=tile, thread=owner(nt, tile))
        t0 = thread * per
        a, b = first_line_in_tile(text, t0, 2), first_line_in_tile(text, t0 + per - 1, 0)
        out[f"bad_tiles_{nt}_one_thread"] = _bad(broken(text, a, b), a, tile=t0, thread=thread, later=(b, t0 + per - 1, thread))
        for tag, ca, cb, (ta, tb) in (("sep_then_header", 2, 0, far[0]), ("header_then_sep", 0, 2, far[1]),
                                      ("neighbours", 2, 0, (thread, thread + 1))):
            a, b = first_line_in_tile(text, ta * per + per - 1, ca), first_line_in_tile(text, tb * per, cb)
            out[f"bad_tiles_{nt}_{tag}"] = _bad(broken(text, a, b), a, tile=ta * per + per - 1, thread=ta,
                                                later=(b, tb * per, tb))
    return out
